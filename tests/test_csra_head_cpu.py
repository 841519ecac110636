"""CPU (no GPU): the numpy statement of the class-specific residual attention head (chexpert_amd.heads: csra_reference,
csra_backward_reference) against torch float64 autograd for both activations, with and without the per-(image, channel) multiplier;
lambda = 0 against the linear head on the average pool; the surface of FusedNet.set_head (validation, the state_dict keys, the refusal
after binding, the average pool both ways, head_state); the refusals of the paths that read the head as pool + classifier; the argument
checks of the entry points of chexpert_amd/csrc/csra_head.hip before any launch; the command line's flags."""
import os
import re

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from chexpert_amd import heads as H

ACTS = ["relu", "swish"]
SHAPES = [(1, 1, 8, 1), (3, 25, 16, 5), (2, 9, 24, 42)]              # B, HW, C, n


def _inputs(seed, B, HW, C, n, with_m):
    g = torch.Generator().manual_seed(seed)
    r = lambda *s: torch.randn(*s, generator=g, dtype=torch.float64)                                        # noqa: E731
    x, sc, sh = r(B, HW, C), torch.rand(C, generator=g, dtype=torch.float64) + 0.5, r(C) * 0.3
    sc[1] = -sc[1]                                                     # a negative gamma is legal
    x[:, :, 2] = (-1.0 - sh[2]) / sc[2] - x[:, :, 2].abs() * sc[2].sign()            # one dead channel: z < 0 everywhere
    W, b = r(n, C) * 0.5, r(n)
    m = (torch.rand(B, C, generator=g, dtype=torch.float64) > 0.3).double() / 0.7 if with_m else None
    return x, sc, sh, W, b, m


def _torch_csra(x, sc, sh, W, b, m, lam, T, act):
    """The head as the paper's code computes it (without its division by |W_k|), on torch tensors."""
    z = x * sc + sh
    a = F.relu(z) if act == "relu" else z * torch.sigmoid(z)
    if m is not None:
        a = a * m[:, None, :]
    s = torch.einsum("kc,bpc->bkp", W, a)
    att = (torch.softmax(T * s, 2) * s).sum(2)
    return b + s.mean(2) + lam * att, a, s


@pytest.mark.parametrize("with_m", [False, True], ids=["plain", "m"])
@pytest.mark.parametrize("act", ACTS)
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "B%d_HW%d_C%d_n%d" % s)
def test_references_against_torch_autograd(shape, act, with_m):
    B, HW, C, n = shape
    lam, T = 0.3, 2.0
    x, sc, sh, W, b, m = _inputs(17, B, HW, C, n, with_m)
    assert bool(((x * sc + sh)[:, :, 2] < 0).all())
    g = torch.Generator().manual_seed(5)
    dl = torch.randn(B, n, generator=g, dtype=torch.float64)
    mean, rstd = torch.randn(C, generator=g, dtype=torch.float64), torch.rand(C, generator=g, dtype=torch.float64) + 0.5
    es = torch.randn(C, generator=g, dtype=torch.float64)
    xr, Wr, br = x.clone().requires_grad_(True), W.clone().requires_grad_(True), b.clone().requires_grad_(True)
    logits_t, _, s_t = _torch_csra(xr, sc, sh, Wr, br, m, lam, T, act)
    (logits_t * dl).sum().backward()
    np_ = lambda t: None if t is None else t.detach().numpy()                                               # noqa: E731
    logits, s, w, att = H.csra_reference(np_(x), np_(sc), np_(sh), np_(W), np_(b), lam, T, act, np_(m))
    np.testing.assert_allclose(logits, np_(logits_t), rtol=1e-12, atol=1e-13)
    np.testing.assert_allclose(s, np_(s_t), rtol=1e-12, atol=1e-13)
    np.testing.assert_allclose(w.sum(2), 1.0, rtol=1e-12)
    gout, S1, S2, dW, db = H.csra_backward_reference(np_(dl), np_(x), np_(sc), np_(sh), np_(mean), np_(rstd), np_(es), np_(W), lam, T, act,
                                                     np_(m))
    dz = xr.grad / sc                                                  # d loss / d z: x.grad = dz * sc
    np.testing.assert_allclose(gout, np_(dz * es), rtol=1e-10, atol=1e-13)
    np.testing.assert_allclose(S1, np_(dz.sum((0, 1))), rtol=1e-10, atol=1e-13)
    np.testing.assert_allclose(S2, np_((dz * (x - mean) * rstd).sum((0, 1))), rtol=1e-10, atol=1e-13)
    np.testing.assert_allclose(dW, np_(Wr.grad), rtol=1e-10, atol=1e-13)
    np.testing.assert_allclose(db, np_(br.grad), rtol=1e-10, atol=1e-13)
    if act == "relu":                                                  # the dead channel: nothing flows
        assert not gout[:, :, 2].any() and S1[2] == 0.0 and not dW[:, 2].any()
    if HW == 1:                                                        # the softmax of one pixel is 1: logit = b + (1 + lambda) s
        np.testing.assert_allclose(logits, np_(b) + (1 + lam) * s[:, :, 0], rtol=1e-12, atol=1e-13)


@pytest.mark.parametrize("act", ACTS)
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "B%d_HW%d_C%d_n%d" % s)
def test_lambda_zero_is_the_linear_head(shape, act):
    B, HW, C, n = shape
    x, sc, sh, W, b, m = _inputs(23, B, HW, C, n, True)
    _, a, _ = _torch_csra(x, sc, sh, W, b, m, 0.0, 2.0, act)
    want = F.linear(a.mean(1), W, b).numpy()
    got = H.csra_reference(x.numpy(), sc.numpy(), sh.numpy(), W.numpy(), b.numpy(), 0.0, 2.0, act, m.numpy())[0]
    assert np.abs(got - want).max() <= 1e-12


def test_large_scores_stay_finite():
    x, sc, sh, W, b, _ = _inputs(29, 2, 9, 8, 3, False)
    x[1, 4, 5] = (1e4 - sh[5]) / sc[5]
    out = H.csra_reference(x.numpy(), sc.numpy(), sh.numpy(), W.numpy(), b.numpy(), 0.3, 2.0) + \
        H.csra_backward_reference(np.ones((2, 3)), x.numpy(), sc.numpy(), sh.numpy(), np.zeros(8), np.ones(8), np.ones(8), W.numpy(), 0.3, 2.0)
    assert all(np.isfinite(t).all() for t in out)


def test_check_head():
    assert H.check_head() == ("linear", 0.1, 1.0) and H.check_head("csra", 0, 2) == ("csra", 0.0, 2.0)
    assert H.check_head("csra", lam="0.25", T=3) == ("csra", 0.25, 3.0)
    for kw in (dict(kind="attention"), dict(kind=None), dict(kind="csra", lam=-0.1), dict(kind="csra", T=0.0), dict(kind="csra", T=-1.0),
               dict(kind="csra", lam=float("nan")), dict(kind="csra", lam=float("inf")), dict(kind="csra", T=float("inf")),
               dict(kind="csra", T=float("nan")), dict(kind="linear", lam="much"), dict(kind="csra", T=None)):
        with pytest.raises(ValueError):
            H.check_head(**kw)


def _small(n=5):
    from chexpert_amd.models import DenseNet
    return DenseNet(32, (2, 2, 2, 2), 64, num_classes=n)


def test_set_head_surface():
    model = _small()
    base, n_params = list(model.state_dict().keys()), len(list(model.parameters()))
    assert model.head_kind == "linear" and model.head_state() == {"kind": "linear", "lam": None, "T": None}
    for kw in (dict(kind="attention"), dict(kind="csra", lam=-1.0), dict(kind="csra", T=0.0), dict(kind="csra", lam=float("nan"))):
        with pytest.raises(ValueError):
            model.set_head(**kw)
        assert model.head_kind == "linear" and not hasattr(model, "head_attn") and list(model.state_dict().keys()) == base
    assert model.set_head("csra", lam=0.3, T=2.0) is model and model.head_kind == "csra"
    assert model.head_attn.dtype == torch.float32 and model.head_attn.tolist() == [pytest.approx(0.3), 2.0]
    assert "head_attn" in dict(model.named_buffers()) and not model.head_attn.requires_grad
    # the keys of the linear head: its checkpoints load, and the other way round
    assert list(model.state_dict().keys()) == base and len(list(model.parameters())) == n_params
    model.load_state_dict(_small().state_dict(), strict=True)
    assert model.head_state() == {"kind": "csra", "lam": pytest.approx(0.3), "T": 2.0}
    dst = _small().load_head_state(model.head_state())
    assert dst.head_kind == "csra" and torch.equal(dst.head_attn, model.head_attn)
    assert _small().load_head_state(None).head_kind == "linear" and _small().load_head_state({}).head_kind == "linear"
    assert model.set_head("csra").head_attn.tolist() == [pytest.approx(0.1), 1.0]
    model.set_head()
    assert model.head_kind == "linear" and not hasattr(model, "head_attn") and list(model.state_dict().keys()) == base
    # the average pool, both ways
    with pytest.raises(ValueError, match="average pool"):
        _small().set_pool("max").set_head("csra")
    m2 = _small().set_head("csra")
    for kind in ("max", "lse", "gem"):
        with pytest.raises(ValueError, match="set_head"):
            m2.set_pool(kind)
    assert m2.set_pool("avg").pool_kind == "avg" and m2.head_kind == "csra" and "pool_p" not in m2.state_dict()
    with pytest.raises(ValueError, match="at most 64"):
        _small(66).set_head("csra")
    assert _small(42).set_head("csra").head_kind == "csra"            # the 3n-wide multiclass head


def test_set_head_is_refused_once_the_engine_has_bound():
    from chexpert_amd.models import Bottleneck, ResNet, construct_model
    for model in (_small(), ResNet(Bottleneck, [1, 1, 1, 1], num_classes=3), construct_model("efficientnet-b0", 3)):
        eng = model._eng()
        model.set_head("csra")                                         # an engine that has not bound yet does not lock the choice
        eng = model._eng()
        assert eng.head_kind() == "csra" and eng._head_path() == "csra"  # (the one name _head_fwd / _head_bwd pick their kernels by)
        eng.flat = torch.zeros(4)                                      # what bind_params leaves behind
        with pytest.raises(RuntimeError, match="before the engine has bound"):
            model.set_head("linear")
        assert model.head_kind == "csra"
        with pytest.raises(ValueError):                                # validation comes first
            model.set_head("attention")
        eng.flat = None
    from chexpert_amd.optim import FusedAdam
    model = _small().set_head("csra")
    FusedAdam(model, lr=1e-3)
    with pytest.raises(RuntimeError, match="before the engine has bound"):
        model.set_head("linear")
    assert model.head_kind == "csra"


def test_paths_that_read_pool_and_classifier_refuse_csra():
    from chexpert_amd import gradcam
    from chexpert_amd.models import DenseNet
    model = _small().set_head("csra")
    x = torch.zeros(2, 3, 64, 64)
    with pytest.raises(NotImplementedError, match="set_head"):
        gradcam.class_cam(model, x)
    with pytest.raises(NotImplementedError, match="set_head"):
        gradcam.hooked_eval_forward(model, x)
    with pytest.raises(NotImplementedError, match="set_head"):
        model.require_avg_pool("grad_cam")
    with pytest.raises(NotImplementedError, match="set_head"):
        DenseNet(12, (2, 2, 2), 24, num_classes=10).set_head("csra")._eng()       # CIFAR DenseNet-BC: the channel-padded twin
    with pytest.raises(NotImplementedError, match="set_head"):
        H.class_maps(_small(), x)                                      # ... and class_maps wants the csra head


def test_entry_points_validate_without_launching():
    from chexpert_amd import _lib, ops
    EINVAL, EALIGN, ESHAPE, EUNSUPPORTED, ESTATROWS = -1, -2, -3, -4, -5
    L = _lib.lib()
    f = [torch.zeros(1 << 14, dtype=torch.float32) for _ in range(6)]
    X, V, O, A, Sc, G = (t.data_ptr() for t in f)
    RELU, SWISH = 1, 2
    assert L.cx_csra_bwd_scratch(2, 4, 16, 5) == 2 * 4 * 16 + 2 * 5 * 16 and L.cx_csra_bwd_scratch(2, 4, 16, 33) == 2 * 4 * 64 + 2 * 33 * 16
    assert L.cx_csra_bwd_scratch(256, 100, 1024, 14) == 256 * 100 * 16 + 128 * 14 * 1024
    assert L.cx_csra_bwd_scratch(2, 4, 16, 65) == EUNSUPPORTED and L.cx_csra_bwd_scratch(0, 4, 16, 5) == ESHAPE
    assert ops.csra_bwd_scratch(2, 4, 16, 5) == 288
    with pytest.raises(RuntimeError):
        ops.csra_bwd_scratch(2, 4, 16, 65)
    for (fwd, bwd), q in (((L.cx_csra_head_fwd, L.cx_csra_head_bwd), 8), ((L.cx_csra_head_fwd_f32, L.cx_csra_head_bwd_f32), 4)):
        fw = lambda x=X, sc=V, sh=V, m=None, W=V, bias=V, lt=V, logits=O, s=O, stat=A, B=2, HW=4, C=16, ldx=16, n=5, act=RELU: \
            fwd(x, sc, sh, m, W, bias, lt, logits, s, stat, B, HW, C, ldx, n, act, None)                  # noqa: E731
        for name in ("x", "sc", "sh", "W", "lt", "logits", "s", "stat"):
            assert fw(**{name: None}) == EINVAL, name
        assert fw(act=0) == EINVAL and fw(act=3) == EINVAL
        assert fw(n=0) == ESHAPE and fw(B=0) == ESHAPE and fw(HW=0) == ESHAPE and fw(C=0, ldx=0) == ESHAPE
        assert fw(C=16 + q // 2, ldx=32) == ESHAPE and fw(ldx=8) == ESHAPE and fw(ldx=16 + q // 2) == ESHAPE
        assert fw(n=65) == EUNSUPPORTED
        assert fw(x=X + 4) == EALIGN
        bw = lambda dl=O, s=O, stat=A, lt=V, x=X, sc=V, sh=V, m=None, mean=V, rstd=V, es=V, W=V, g=G, S1=A, S2=A, dW=O, db=O, scr=Sc, \
            slen=1 << 14, B=2, HW=4, C=16, ldx=16, ldg=16, n=5, act=SWISH, rows=0: \
            bwd(dl, s, stat, lt, x, sc, sh, m, mean, rstd, es, W, g, S1, S2, dW, db, scr, slen, B, HW, C, ldx, ldg, n, act, rows, None)   # noqa: E731
        for name in ("dl", "s", "stat", "lt", "x", "sc", "sh", "mean", "rstd", "es", "W", "g", "S1", "S2", "dW", "scr"):
            assert bw(**{name: None}) == EINVAL, name
        assert bw(act=0) == EINVAL
        assert bw(n=0) == ESHAPE and bw(B=-1) == ESHAPE and bw(HW=0) == ESHAPE and bw(ldx=8) == ESHAPE and bw(ldg=8) == ESHAPE
        assert bw(ldg=16 + q // 2) == ESHAPE
        assert bw(n=65) == EUNSUPPORTED
        assert bw(slen=287) == EUNSUPPORTED and bw(slen=0) == EUNSUPPORTED           # a scratch that is too small is refused
        assert bw(x=X + 8) == EALIGN and bw(g=G + 4) == EALIGN
        assert bw(B=3, rows=2, slen=1 << 14) == ESTATROWS
    assert all(not t.any() for t in f)                                 # nothing ran
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(root, "include", "chexpert_hip.h")).read(), flags=re.S)
    for name, n in (("cx_csra_head_fwd", 17), ("cx_csra_head_bwd", 28), ("cx_csra_head_fwd_f32", 17), ("cx_csra_head_bwd_f32", 28)):
        m = re.search(r"\bint\s+%s\s*\(([^;{]*?)\)\s*;" % name, hdr, flags=re.S)
        assert m and len(_lib.SIGNATURES[name]) == m.group(1).count(",") + 1 == n, name
    assert "csra_head.hip" in open(os.path.join(root, "chexpert_amd", "csrc", "Makefile")).read()
    assert ops.CSRA_MAX_CLASSES == H.MAX_CLASSES == 64


def test_cli_flags():
    from chexpert_amd import cli
    p = cli.build_parser()
    a = p.parse_args([])
    assert (a.head, a.csra_lambda, a.csra_T) == (None, None, None) and cli.resolve_head(a) is None
    a = p.parse_args(["--head", "csra", "--csra_lambda", "0.3", "--csra_T", "2"])
    assert cli.resolve_head(a) == {"kind": "csra", "lam": 0.3, "T": 2.0}
    assert cli.resolve_head(p.parse_args(["--head", "csra"])) == {"kind": "csra", "lam": None, "T": None}
    assert cli.resolve_head(p.parse_args(["--head", "linear"])) == {"kind": "linear", "lam": None, "T": None}
    with pytest.raises(SystemExit):
        p.parse_args(["--head", "attention"])
    for bad in (["--csra_lambda", "0.3"], ["--head", "linear", "--csra_T", "2"], ["--head", "csra", "--csra_lambda", "-1"],
                ["--head", "csra", "--csra_T", "0"], ["--head", "csra", "--csra_T", "nan"]):
        with pytest.raises(ValueError):
            cli.resolve_head(p.parse_args(bad))
    # csra stands on the average pool
    for kind in ("max", "lse", "gem"):
        a = p.parse_args(["--head", "csra", "--pool", kind])
        with pytest.raises(ValueError, match="--head csra .* --pool %s" % kind):
            cli.resolve_head(a, cli.resolve_pool(a))
    a = p.parse_args(["--head", "csra", "--pool", "avg"])
    assert cli.resolve_head(a, cli.resolve_pool(a))["kind"] == "csra"
    # the checkpoint's head; --head linear on a csra checkpoint is refused; linear -> csra is the fine-tuning case
    ck = {"kind": "csra", "lam": 0.25, "T": 3.0}
    assert cli.head_for_checkpoint(None, ck) == ck
    assert cli.head_for_checkpoint({"kind": "csra", "lam": None, "T": None}, ck) == ck
    assert cli.head_for_checkpoint({"kind": "csra", "lam": 0.5, "T": None}, ck) == {"kind": "csra", "lam": 0.5, "T": 3.0}
    assert cli.head_for_checkpoint(None, None) == {"kind": "linear"}
    assert cli.head_for_checkpoint({"kind": "csra", "lam": None, "T": 2.0}, None) == {"kind": "csra", "lam": 0.1, "T": 2.0}
    assert cli.head_for_checkpoint({"kind": "csra", "lam": 0.0, "T": None}, {"kind": "linear", "lam": None, "T": None}) == \
        {"kind": "csra", "lam": 0.0, "T": 1.0}
    with pytest.raises(ValueError, match="--head linear contradicts"):
        cli.head_for_checkpoint({"kind": "linear", "lam": None, "T": None}, ck)


def test_cli_refuses_csra_with_another_pool_before_anything_runs(tmp_path):
    from chexpert_amd import cli
    with pytest.raises((SystemExit, ValueError)):
        cli.main(["--train", "--synthetic", "32", "--head", "csra", "--pool", "max", "--output_dir", str(tmp_path / "o")])
    assert not (tmp_path / "o").exists()
