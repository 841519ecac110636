"""CPU (no GPU): the numpy statement of the probabilistic-CAM pooling head (chexpert_amd.heads: pcam_reference, pcam_backward_reference)
against torch float64 autograd over the shape list of tests/test_csra_head_cpu.py, for both activations, with and without the
per-(image, channel) multiplier and the bias; the anchors of the definition (one pixel, equal scores, W = 0, a permutation of the
pixels, a large bias against the average head); scores of +-1e4; the surface of FusedNet.set_head("pcam"); the refusals of the paths that
read the head as pool + classifier; the argument checks of the cx_pcam_* entry points before any launch; the command line's flags."""
import os
import re

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from chexpert_amd import heads as H

ACTS = ["relu", "swish"]
SHAPES = [(1, 1, 8, 1), (3, 25, 16, 5), (2, 9, 24, 42)]              # B, HW, C, n
np_ = lambda t: None if t is None else t.detach().numpy()                                                   # noqa: E731


def _inputs(seed, B, HW, C, n, with_m):
    g = torch.Generator().manual_seed(seed)
    r = lambda *s: torch.randn(*s, generator=g, dtype=torch.float64)                                        # noqa: E731
    x, sc, sh = r(B, HW, C), torch.rand(C, generator=g, dtype=torch.float64) + 0.5, r(C) * 0.3
    sc[1] = -sc[1]                                                     # a negative gamma is legal
    x[:, :, 2] = (-1.0 - sh[2]) / sc[2] - x[:, :, 2].abs() * sc[2].sign()            # one dead channel: z < 0 everywhere
    W, b = r(n, C) * 0.5, r(n)
    m = (torch.rand(B, C, generator=g, dtype=torch.float64) > 0.3).double() / 0.7 if with_m else None
    return x, sc, sh, W, b, m


def _torch_pcam(x, sc, sh, W, b, m, act):
    """The head as the paper's code computes it: the plain quotient sigmoid / sum sigmoid, nothing detached."""
    z = x * sc + sh
    a = F.relu(z) if act == "relu" else z * torch.sigmoid(z)
    if m is not None:
        a = a * m[:, None, :]
    s = torch.einsum("kc,bpc->bkp", W, a)
    u = s if b is None else s + b[None, :, None]
    P = torch.sigmoid(u)
    w = P / P.sum(2, keepdim=True)
    return (w * u).sum(2), a, s, w, P


@pytest.mark.parametrize("with_b", [True, False], ids=["bias", "nobias"])
@pytest.mark.parametrize("with_m", [False, True], ids=["plain", "m"])
@pytest.mark.parametrize("act", ACTS)
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "B%d_HW%d_C%d_n%d" % s)
def test_references_against_torch_autograd(shape, act, with_m, with_b):
    B, HW, C, n = shape
    x, sc, sh, W, b, m = _inputs(17, B, HW, C, n, with_m)
    assert bool(((x * sc + sh)[:, :, 2] < 0).all())
    g = torch.Generator().manual_seed(5)
    dl = torch.randn(B, n, generator=g, dtype=torch.float64)
    mean, rstd = torch.randn(C, generator=g, dtype=torch.float64), torch.rand(C, generator=g, dtype=torch.float64) + 0.5
    es = torch.randn(C, generator=g, dtype=torch.float64)
    xr, Wr = x.clone().requires_grad_(True), W.clone().requires_grad_(True)
    br = b.clone().requires_grad_(True) if with_b else None
    logits_t, _, s_t, w_t, P_t = _torch_pcam(xr, sc, sh, Wr, br, m, act)
    (logits_t * dl).sum().backward()
    logits, s, w, P = H.pcam_reference(np_(x), np_(sc), np_(sh), np_(W), np_(b) if with_b else None, act, np_(m))
    np.testing.assert_allclose(logits, np_(logits_t), rtol=1e-12, atol=1e-13)
    np.testing.assert_allclose(s, np_(s_t), rtol=1e-12, atol=1e-13)
    np.testing.assert_allclose(w, np_(w_t), rtol=1e-12, atol=1e-15)
    np.testing.assert_allclose(P, np_(P_t), rtol=1e-12, atol=1e-15)
    np.testing.assert_allclose(w.sum(2), 1.0, rtol=1e-12)
    assert P.min() >= 0.0 and P.max() <= 1.0
    gout, S1, S2, dW, db = H.pcam_backward_reference(np_(dl), np_(x), np_(sc), np_(sh), np_(mean), np_(rstd), np_(es), np_(W),
                                                     np_(b) if with_b else None, act, np_(m))
    dz = xr.grad / sc                                                  # d loss / d z: x.grad = dz * sc
    np.testing.assert_allclose(gout, np_(dz * es), rtol=1e-10, atol=1e-13)
    np.testing.assert_allclose(S1, np_(dz.sum((0, 1))), rtol=1e-10, atol=1e-13)
    np.testing.assert_allclose(S2, np_((dz * (x - mean) * rstd).sum((0, 1))), rtol=1e-10, atol=1e-13)
    np.testing.assert_allclose(dW, np_(Wr.grad), rtol=1e-10, atol=1e-13)
    if with_b:
        np.testing.assert_allclose(db, np_(br.grad), rtol=1e-10, atol=1e-13)
        if HW > 1:                                                     # ... which is not csra's sum of dlogit
            assert np.abs(db - np_(dl).sum(0)).max() > 1e-3
    if act == "relu":                                                  # the dead channel: nothing flows
        assert not gout[:, :, 2].any() and S1[2] == 0.0 and not dW[:, 2].any()


def _plain(seed=31, B=2, HW=9, C=8, n=3):
    x, sc, sh, W, b, _ = _inputs(seed, B, HW, C, n, False)
    return [np_(t) for t in (x, sc, sh, W, b)]


def test_anchor_one_pixel():
    x, sc, sh, W, b = _plain(HW=1)
    logits, s, w, _ = H.pcam_reference(x, sc, sh, W, b)
    np.testing.assert_allclose(logits, b + s[:, :, 0], rtol=1e-14, atol=1e-14)
    assert (w == 1.0).all()


def test_anchor_equal_scores():
    x, sc, sh, W, b = _plain()
    x[:] = x[:, :1]                                                    # every pixel of an image holds the same features
    logits, s, w, _ = H.pcam_reference(x, sc, sh, W, b)
    np.testing.assert_allclose(logits, s[:, :, 0] + b, rtol=1e-13, atol=1e-13)
    np.testing.assert_allclose(w, 1.0 / 9, rtol=1e-13)


def test_anchor_zero_weights():
    x, sc, sh, W, b = _plain()
    logits, _, w, P = H.pcam_reference(x, sc, sh, W * 0, b)
    np.testing.assert_allclose(logits, np.broadcast_to(b, logits.shape), rtol=1e-14, atol=1e-14)
    np.testing.assert_allclose(w, 1.0 / 9, rtol=1e-14)
    np.testing.assert_allclose(P, np.broadcast_to((1 / (1 + np.exp(-b)))[None, :, None], P.shape), rtol=1e-14)


def test_anchor_pixel_permutation():
    x, sc, sh, W, b = _plain()
    perm = np.random.RandomState(3).permutation(9)
    a, _, wa, _ = H.pcam_reference(x, sc, sh, W, b)
    c, _, wc, _ = H.pcam_reference(x[:, perm], sc, sh, W, b)
    np.testing.assert_allclose(a, c, rtol=1e-13, atol=1e-14)
    np.testing.assert_allclose(wa[:, :, perm], wc, rtol=1e-13, atol=1e-16)


def test_anchor_large_bias_tends_to_the_average_head():
    x, sc, sh, W, b = _plain()
    a = np.maximum(x * sc + sh, 0.0)
    gaps = []
    for shift in (10.0, 20.0, 40.0):
        want = a.mean(1) @ W.T + b + shift
        gaps.append(np.abs(H.pcam_reference(x, sc, sh, W, b + shift)[0] - want).max())
    assert gaps[0] > gaps[1] > gaps[2] or gaps[2] < 1e-12              # sigmoid saturates: the weights tend to 1 / HW
    assert gaps[2] < 1e-12 and gaps[0] < 1e-2


@pytest.mark.parametrize("sign", [1.0, -1.0], ids=["plus", "minus"])
@pytest.mark.parametrize("where", ["all", "one"])
def test_large_scores_stay_finite(where, sign):
    x, sc, sh, W, b = _plain(seed=29)
    W = W.copy()
    W[:, 5] = sign                                                     # channel 5's activation of 1e4 becomes a score of +-1e4
    big = (1e4 - sh[5]) / sc[5]
    if where == "all":
        x[:, :, 5] = big
    else:
        x[1, 4, 5] = big
    logits, s, w, P = H.pcam_reference(x, sc, sh, W, b)
    assert np.abs(s).max() > 9e3
    out = (logits, w, P) + H.pcam_backward_reference(np.ones((2, 3)), x, sc, sh, np.zeros(8), np.ones(8), np.ones(8), W, b)
    assert all(np.isfinite(t).all() for t in out)
    np.testing.assert_allclose(w.sum(2), 1.0, rtol=1e-12)
    xt, Wt, bt = (torch.from_numpy(t).requires_grad_(True) for t in (x, W, b))
    lt = _torch_pcam(xt, torch.from_numpy(sc), torch.from_numpy(sh), Wt, bt, None, "relu")[0]
    if bool(torch.isfinite(lt).all()):                                # where the plain quotient is finite, the log sigma form equals it
        lt.sum().backward()
        np.testing.assert_allclose(logits, np_(lt), rtol=1e-12, atol=1e-12)
        if bool(torch.isfinite(bt.grad).all()) and bool(torch.isfinite(Wt.grad).all()):
            np.testing.assert_allclose(out[-1], np_(bt.grad), rtol=1e-9, atol=1e-9)
            np.testing.assert_allclose(out[-2], np_(Wt.grad), rtol=1e-9, atol=1e-9 * np.abs(out[-2]).max())


def test_check_head():
    assert H.KINDS == ("linear", "csra", "pcam")
    assert H.check_head("pcam") == ("pcam", 0.1, 1.0) and H.check_head("pcam", 0, 2) == ("pcam", 0.0, 2.0)
    assert H.check_head() == ("linear", 0.1, 1.0) and H.check_head("csra", lam="0.25", T=3) == ("csra", 0.25, 3.0)
    for kw in (dict(kind="pcam", lam=-0.1), dict(kind="pcam", T=0.0), dict(kind="pcam", lam=float("nan")), dict(kind="pcam", T=None),
               dict(kind="PCAM"), dict(kind="cam")):
        with pytest.raises(ValueError):
            H.check_head(**kw)


def _small(n=5):
    from chexpert_amd.models import DenseNet
    return DenseNet(32, (2, 2, 2, 2), 64, num_classes=n)


def test_set_head_surface():
    model = _small()
    base, n_params = list(model.state_dict().keys()), len(list(model.parameters()))
    buffers = [k for k, _ in model.named_buffers()]
    assert model.set_head("pcam") is model and model.head_kind == "pcam"
    assert model.head_state() == {"kind": "pcam", "lam": None, "T": None}
    assert list(model.state_dict().keys()) == base and len(list(model.parameters())) == n_params
    assert [k for k, _ in model.named_buffers()] == buffers and not hasattr(model, "head_attn")
    model.load_state_dict(_small().state_dict(), strict=True)
    dst = _small().load_head_state(model.head_state())
    assert dst.head_kind == "pcam" and dst.head_state() == model.head_state() and not hasattr(dst, "head_attn")
    assert _small().load_head_state({"kind": "pcam"}).head_kind == "pcam"
    with pytest.raises(ValueError):
        model.set_head("pcam", lam=-1.0)
    assert model.head_kind == "pcam"
    # csra -> pcam drops csra's buffer; pcam -> linear leaves the model it was
    assert not hasattr(_small().set_head("csra").set_head("pcam"), "head_attn")
    model.set_head()
    assert model.head_kind == "linear" and list(model.state_dict().keys()) == base
    # the average pool, both ways
    for kind in ("max", "lse", "gem"):
        with pytest.raises(ValueError, match="average pool"):
            _small().set_pool(kind).set_head("pcam")
    m2 = _small().set_head("pcam")
    for kind in ("max", "lse", "gem"):
        with pytest.raises(ValueError, match="set_head"):
            m2.set_pool(kind)
    assert m2.set_pool("avg").pool_kind == "avg" and m2.head_kind == "pcam" and "pool_p" not in m2.state_dict()
    with pytest.raises(ValueError, match="at most 64"):
        _small(65).set_head("pcam")
    assert _small(42).set_head("pcam").head_kind == "pcam"            # the 3n-wide multiclass head
    assert _small(64).set_head("pcam").head_kind == "pcam"


def test_set_head_is_refused_once_the_engine_has_bound():
    from chexpert_amd.models import Bottleneck, ResNet, construct_model
    for model in (_small(), ResNet(Bottleneck, [1, 1, 1, 1], num_classes=3), construct_model("efficientnet-b0", 3)):
        eng = model._eng()
        model.set_head("pcam")                                         # an engine that has not bound yet does not lock the choice
        eng = model._eng()
        assert eng.head_kind() == "pcam" and eng._head_path() == "pcam"  # (the one name _head_fwd / _head_bwd pick their kernels by)
        eng.flat = torch.zeros(4)                                      # what bind_params leaves behind
        for kind in ("linear", "csra"):
            with pytest.raises(RuntimeError, match="before the engine has bound"):
                model.set_head(kind)
        assert model.head_kind == "pcam"
        with pytest.raises(ValueError):                                # validation comes first
            model.set_head("attention")
        eng.flat = None
    from chexpert_amd.optim import FusedAdam
    model = _small().set_head("pcam")
    FusedAdam(model, lr=1e-3)
    with pytest.raises(RuntimeError, match="before the engine has bound"):
        model.set_head("linear")
    assert model.head_kind == "pcam"
    model = _small()
    FusedAdam(model, lr=1e-3)
    with pytest.raises(RuntimeError, match="before the engine has bound"):
        model.set_head("pcam")
    assert model.head_kind == "linear"


def test_paths_that_read_pool_and_classifier_refuse_pcam():
    from chexpert_amd import gradcam
    from chexpert_amd.models import DenseNet
    model = _small().set_head("pcam")
    x = torch.zeros(2, 3, 64, 64)
    with pytest.raises(NotImplementedError, match="set_head"):
        gradcam.class_cam(model, x)
    with pytest.raises(NotImplementedError, match="set_head"):
        gradcam.hooked_eval_forward(model, x)
    with pytest.raises(NotImplementedError, match="set_head"):
        model.require_avg_pool("grad_cam")
    with pytest.raises(NotImplementedError, match="set_head"):
        DenseNet(12, (2, 2, 2), 24, num_classes=10).set_head("pcam")._eng()       # CIFAR DenseNet-BC: the channel-padded twin
    with pytest.raises(NotImplementedError, match="set_head"):
        H.class_maps(_small(), x)                                      # class_maps wants the csra or the pcam head
    with pytest.raises(RuntimeError, match="GPU only"):
        H.class_maps(model.eval(), x)


def test_entry_points_validate_without_launching():
    from chexpert_amd import _lib, ops
    EINVAL, EALIGN, ESHAPE, EUNSUPPORTED, ESTATROWS = -1, -2, -3, -4, -5
    L = _lib.lib()
    assert L.cx_abi_version() == 10
    f = [torch.zeros(1 << 14, dtype=torch.float32) for _ in range(6)]
    X, V, O, A, Sc, G = (t.data_ptr() for t in f)
    RELU, SWISH = 1, 2
    for shape in ((2, 4, 16, 5), (2, 4, 16, 33), (256, 100, 1024, 14), (1, 1, 8, 1), (300, 7, 24, 64)):
        B, _, _, n = shape
        assert L.cx_pcam_bwd_scratch(*shape) == L.cx_csra_bwd_scratch(*shape) + B * n, shape
    assert L.cx_pcam_bwd_scratch(2, 4, 16, 65) == EUNSUPPORTED and L.cx_pcam_bwd_scratch(0, 4, 16, 5) == ESHAPE
    assert L.cx_pcam_bwd_scratch(2, 4, 16, 0) == ESHAPE
    assert ops.pcam_bwd_scratch(2, 4, 16, 5) == 298 == ops.csra_bwd_scratch(2, 4, 16, 5) + 10
    with pytest.raises(RuntimeError):
        ops.pcam_bwd_scratch(2, 4, 16, 65)
    for (fwd, bwd), q in (((L.cx_pcam_head_fwd, L.cx_pcam_head_bwd), 8), ((L.cx_pcam_head_fwd_f32, L.cx_pcam_head_bwd_f32), 4)):
        fw = lambda x=X, sc=V, sh=V, m=None, W=V, bias=V, logits=O, s=O, stat=A, B=2, HW=4, C=16, ldx=16, n=5, act=RELU: \
            fwd(x, sc, sh, m, W, bias, logits, s, stat, B, HW, C, ldx, n, act, None)                      # noqa: E731
        for name in ("x", "sc", "sh", "W", "logits", "s", "stat"):
            assert fw(**{name: None}) == EINVAL, name
        assert fw(act=0) == EINVAL and fw(act=3) == EINVAL
        assert fw(n=0) == ESHAPE and fw(B=0) == ESHAPE and fw(HW=0) == ESHAPE and fw(C=0, ldx=0) == ESHAPE
        assert fw(C=16 + q // 2, ldx=32) == ESHAPE and fw(ldx=8) == ESHAPE and fw(ldx=16 + q // 2) == ESHAPE
        assert fw(n=65) == EUNSUPPORTED
        assert fw(x=X + 4) == EALIGN
        bw = lambda dl=O, s=O, stat=A, x=X, sc=V, sh=V, m=None, mean=V, rstd=V, es=V, W=V, g=G, S1=A, S2=A, dW=O, db=O, scr=Sc, \
            slen=1 << 14, B=2, HW=4, C=16, ldx=16, ldg=16, n=5, act=SWISH, rows=0: \
            bwd(dl, s, stat, x, sc, sh, m, mean, rstd, es, W, g, S1, S2, dW, db, scr, slen, B, HW, C, ldx, ldg, n, act, rows, None)   # noqa: E731
        for name in ("dl", "s", "stat", "x", "sc", "sh", "mean", "rstd", "es", "W", "g", "S1", "S2", "dW", "scr"):
            assert bw(**{name: None}) == EINVAL, name
        assert bw(act=0) == EINVAL
        assert bw(n=0) == ESHAPE and bw(B=-1) == ESHAPE and bw(HW=0) == ESHAPE and bw(ldx=8) == ESHAPE and bw(ldg=8) == ESHAPE
        assert bw(ldg=16 + q // 2) == ESHAPE
        assert bw(n=65) == EUNSUPPORTED
        # a scratch that is too small is refused: csra's length is B n floats short
        assert bw(slen=297) == EUNSUPPORTED and bw(slen=288) == EUNSUPPORTED and bw(slen=0) == EUNSUPPORTED
        assert bw(x=X + 8) == EALIGN and bw(g=G + 4) == EALIGN and bw(scr=Sc + 4) == EALIGN
        assert bw(B=3, rows=2, slen=1 << 14) == ESTATROWS
    assert all(not t.any() for t in f)                                 # nothing ran


def test_header_signatures_and_makefile_agree():
    from chexpert_amd import _lib, ops
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(root, "include", "chexpert_hip.h")).read(), flags=re.S)
    for name, n in (("cx_pcam_head_fwd", 16), ("cx_pcam_head_bwd", 27), ("cx_pcam_head_fwd_f32", 16), ("cx_pcam_head_bwd_f32", 27)):
        m = re.search(r"\bint\s+%s\s*\(([^;{]*?)\)\s*;" % name, hdr, flags=re.S)
        assert m and len(_lib.SIGNATURES[name]) == m.group(1).count(",") + 1 == n, name
        assert "lam_T" not in m.group(1)
        csra = re.search(r"\bint\s+%s\s*\(([^;{]*?)\)\s*;" % name.replace("pcam", "csra"), hdr, flags=re.S).group(1)
        strip = lambda a: [re.sub(r"\s+", " ", t).strip() for t in a.split(",")]                          # noqa: E731
        assert strip(m.group(1)) == [t for t in strip(csra) if not t.endswith("lam_T")], name            # csra's list without lam_T
    m = re.search(r"\blong long\s+cx_pcam_bwd_scratch\s*\(([^;{]*?)\)\s*;", hdr, flags=re.S)
    assert m and len(_lib.SIGNATURES["cx_pcam_bwd_scratch"]) == m.group(1).count(",") + 1 == 4
    assert _lib.lib().cx_pcam_bwd_scratch.restype is _lib.C.c_longlong
    mk = open(os.path.join(root, "chexpert_amd", "csrc", "Makefile")).read()
    src = [f for f in os.listdir(os.path.join(root, "chexpert_amd", "csrc")) if f.endswith(".hip") and
           "cx_pcam_head_fwd" in open(os.path.join(root, "chexpert_amd", "csrc", f)).read()]
    assert len(src) == 1 and src[0] in mk
    assert ops.CSRA_MAX_CLASSES == H.MAX_CLASSES == 64
    assert _lib.lib().cx_abi_version() == 10


def test_cli_flags():
    from chexpert_amd import cli
    p = cli.build_parser()
    assert cli.resolve_head(p.parse_args(["--head", "pcam"])) == {"kind": "pcam", "lam": None, "T": None}
    for bad in (["--head", "pcam", "--csra_lambda", "0.3"], ["--head", "pcam", "--csra_T", "2"],
                ["--head", "pcam", "--csra_lambda", "0.3", "--csra_T", "2"]):
        with pytest.raises(ValueError, match="--head csra"):
            cli.resolve_head(p.parse_args(bad))
    for kind in ("max", "lse", "gem"):
        a = p.parse_args(["--head", "pcam", "--pool", kind])
        with pytest.raises(ValueError, match="--head pcam .* --pool %s" % kind):
            cli.resolve_head(a, cli.resolve_pool(a))
    a = p.parse_args(["--head", "pcam", "--pool", "avg"])
    assert cli.resolve_head(a, cli.resolve_pool(a))["kind"] == "pcam"
    # the checkpoint's head
    none = {"lam": None, "T": None}
    ck = {"kind": "pcam", **none}
    assert cli.head_for_checkpoint(None, ck) == {"kind": "pcam"}
    assert cli.head_for_checkpoint({"kind": "pcam", **none}, ck) == {"kind": "pcam"}
    assert cli.head_for_checkpoint({"kind": "pcam", **none}, None) == {"kind": "pcam"}                  # a linear checkpoint: allowed
    assert cli.head_for_checkpoint({"kind": "pcam", **none}, {"kind": "linear", **none}) == {"kind": "pcam"}
    with pytest.raises(ValueError, match="--head linear contradicts the checkpoint, which was trained with --head pcam"):
        cli.head_for_checkpoint({"kind": "linear", **none}, ck)
    with pytest.raises(ValueError, match="--head csra contradicts the checkpoint, which was trained with --head pcam"):
        cli.head_for_checkpoint({"kind": "csra", "lam": 0.3, "T": None}, ck)
    with pytest.raises(ValueError, match="--head pcam contradicts the checkpoint, which was trained with --head csra"):
        cli.head_for_checkpoint({"kind": "pcam", **none}, {"kind": "csra", "lam": 0.25, "T": 3.0})
    # what the model and the checkpoint say to each other at load time
    model = _small().set_head("pcam")
    cli.check_checkpoint_head_kind({}, model, "ck.pt")
    cli.check_checkpoint_head_kind({"head_state": ck}, model, "ck.pt")
    for other in (_small(), _small().set_head("csra")):
        with pytest.raises(ValueError, match="trained with --head pcam"):
            cli.check_checkpoint_head_kind({"head_state": ck}, other, "ck.pt")
    with pytest.raises(ValueError, match="trained with --head csra"):
        cli.check_checkpoint_head_kind({"head_state": {"kind": "csra", "lam": 0.1, "T": 1.0}}, model, "ck.pt")
    # Grad-CAM alone cannot be drawn on a pcam model
    assert "--cam_classes" in cli.visualize_needs_linear(p.parse_args(["--visualize"]), "pcam")
    assert cli.visualize_needs_linear(p.parse_args(["--visualize", "--cam_classes", "0"]), "pcam") is None


def test_cli_refuses_pcam_with_another_pool_or_csra_flags_before_anything_runs(tmp_path):
    from chexpert_amd import cli
    for extra in (["--pool", "max"], ["--pool", "lse"], ["--pool", "gem"], ["--csra_lambda", "0.2"]):
        with pytest.raises((SystemExit, ValueError)):
            cli.main(["--train", "--synthetic", "32", "--head", "pcam", "--output_dir", str(tmp_path / "o")] + extra)
        assert not (tmp_path / "o").exists()


def test_restore_head_reads_the_checkpoint_and_says_that_the_function_changes(tmp_path, capsys):
    from chexpert_amd import cli
    p = cli.build_parser()
    lin, pc = str(tmp_path / "lin.pt"), str(tmp_path / "pc.pt")
    torch.save({"state_dict": {}}, lin)
    torch.save({"state_dict": {}, "head_state": {"kind": "pcam", "lam": None, "T": None}}, pc)
    a = p.parse_args(["--head", "pcam", "--restore", lin])
    assert cli.restore_head(a, cli.resolve_head(a)) == {"kind": "pcam"}
    assert "function" in capsys.readouterr().out                      # one line: unlike csra at lambda 0, the function changes
    a = p.parse_args(["--restore", pc])
    assert cli.restore_head(a, cli.resolve_head(a)) == {"kind": "pcam"}
    assert capsys.readouterr().out == ""
    for kind in ("linear", "csra"):
        a = p.parse_args(["--head", kind, "--restore", pc])
        with pytest.raises(ValueError, match="--head %s contradicts the checkpoint" % kind):
            cli.restore_head(a, cli.resolve_head(a))
    a = p.parse_args(["--restore", pc])
    with pytest.raises(ValueError, match="average pool"):
        cli.restore_head(a, None, "max")
