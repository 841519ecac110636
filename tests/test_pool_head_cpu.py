"""CPU (no GPU): the numpy statements of the pooling heads (chexpert_amd.pooling: pool_reference, pool_backward_reference) against torch
float64 autograd for the four kinds and both activations, GeM's exponent derivative against a central difference, the surface of
FusedNet.set_pool (validation, state_dict keys per kind, the refusal after binding, pool_state), the fine-tuning groups, and the
argument checks of the three entry points of chexpert_amd/csrc/pool_head.hip before any launch."""
import os
import re

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from chexpert_amd import pooling as P

KINDS = ["avg", "max", "lse", "gem"]
ACTS = ["relu", "swish"]


def _inputs(seed, B=3, H=4, W=5, C=6):
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(B, H * W, C, generator=g, dtype=torch.float64)
    sc = torch.rand(C, generator=g, dtype=torch.float64) + 0.5
    sc[1] = -sc[1]                                                     # a negative gamma is legal
    sh = torch.rand(C, generator=g, dtype=torch.float64) - 0.5
    x[:, :, 2] = (-1.0 - sh[2]) / sc[2] - x[:, :, 2].abs()             # one dead channel: z < 0 everywhere
    return x, sc, sh, (B, H, W, C)


def _torch_pool(x, sc, sh, kind, act, r, p, shape):
    """The torch forms: F.adaptive_avg_pool2d / F.adaptive_max_pool2d / torch.logsumexp / the GeM formula on the NCHW activation."""
    B, H, W, C = shape
    z = x * sc + sh
    a = (F.relu(z) if act == "relu" else z * torch.sigmoid(z)).view(B, H, W, C).permute(0, 3, 1, 2)
    if kind == "avg":
        return F.adaptive_avg_pool2d(a, 1).flatten(1)
    if kind == "max":
        return F.adaptive_max_pool2d(a, 1).flatten(1)
    if kind == "lse":
        return (torch.logsumexp(r * a.flatten(2), 2) - np.log(H * W)) / r
    q = p.clamp(1.0, 16.0) if isinstance(p, torch.Tensor) else min(max(p, 1.0), 16.0)
    return a.clamp_min(1e-6).pow(q).flatten(2).mean(2).pow(1.0 / q)


@pytest.mark.parametrize("act", ACTS)
@pytest.mark.parametrize("kind", KINDS)
def test_references_against_torch_autograd(kind, act):
    x, sc, sh, shape = _inputs(11)
    B, H, W, C = shape
    r, p = 7.0, 2.5
    g = torch.Generator().manual_seed(5)
    dpooled = torch.randn(B, C, generator=g, dtype=torch.float64)
    mean, rstd = torch.randn(C, generator=g, dtype=torch.float64), torch.rand(C, generator=g, dtype=torch.float64) + 0.5
    es = torch.randn(C, generator=g, dtype=torch.float64)
    xr = x.clone().requires_grad_(True)
    pt = torch.tensor(p, dtype=torch.float64, requires_grad=True)
    pooled_t = _torch_pool(xr, sc, sh, kind, act, r, pt, shape)
    (pooled_t * dpooled).sum().backward()
    pooled, T = P.pool_reference(x.numpy(), sc.numpy(), sh.numpy(), kind, act, r=r, p=p)
    np.testing.assert_allclose(pooled, pooled_t.detach().numpy(), rtol=1e-12, atol=1e-14)
    assert (T is None) == (kind not in ("lse", "gem"))
    if kind == "lse":                                                  # the offset the backward kernel subtracts: pooled - max
        np.testing.assert_allclose(T, pooled - _torch_pool(x, sc, sh, "max", act, r, p, shape).numpy(), rtol=1e-10, atol=1e-13)
    gout, S1, S2, dp = P.pool_backward_reference(dpooled.numpy(), x.numpy(), sc.numpy(), sh.numpy(), mean.numpy(), rstd.numpy(), es.numpy(),
                                                 kind, act, r=r, p=p)
    dz = xr.grad / sc                                                  # d loss / d z: x.grad = dz * sc
    np.testing.assert_allclose(gout, (dz * es).numpy(), rtol=1e-10, atol=1e-13)
    np.testing.assert_allclose(S1, dz.sum((0, 1)).numpy(), rtol=1e-10, atol=1e-13)
    np.testing.assert_allclose(S2, (dz * (x - mean) * rstd).sum((0, 1)).numpy(), rtol=1e-10, atol=1e-13)
    if kind == "gem":
        np.testing.assert_allclose(dp, pt.grad.item(), rtol=1e-10)
    else:
        assert dp is None
    if act == "relu" or kind == "gem":                                 # the dead channel: nothing flows (swish' is not 0 below 0)
        assert not gout[:, :, 2].any() and S1[2] == 0.0
    if kind == "gem":
        np.testing.assert_allclose(pooled[:, 2], 1e-6, rtol=1e-12)
        assert np.abs(P.pool_p_derivative_reference(x.numpy(), sc.numpy(), sh.numpy(), act, p)[:, 2]).max() < 1e-18


@pytest.mark.parametrize("act", ACTS)
def test_gem_exponent_derivative_against_a_central_difference(act):
    x, sc, sh, _ = _inputs(12)
    a = (x.numpy(), sc.numpy(), sh.numpy())
    for p in (1.5, 3.0, 9.0, 15.5):
        h = 1e-5
        num = (P.pool_reference(*a, "gem", act, p=p + h)[0] - P.pool_reference(*a, "gem", act, p=p - h)[0]) / (2 * h)
        np.testing.assert_allclose(P.pool_p_derivative_reference(*a, act, p), num, rtol=1e-6, atol=1e-9)
    for p in (1.0, 16.0):                                              # clamped: no gradient
        assert not P.pool_p_derivative_reference(*a, act, p).any()


def test_first_maximum_takes_the_gradient_and_large_activations_stay_finite():
    x = np.zeros((1, 4, 2))
    x[0, :, 0] = [1.0, 3.0, 3.0, 2.0]                                  # a tie at pixels 1 and 2
    x[0, :, 1] = [0.5, 1e4, 0.25, 0.125]
    one, zero = np.ones(2), np.zeros(2)
    w = P.pool_weights_reference(x, one, zero, "max")
    assert w[0, :, 0].tolist() == [0.0, 1.0, 0.0, 0.0] and w[0, :, 1].tolist() == [0.0, 1.0, 0.0, 0.0]
    for kind, kw in (("lse", dict(r=10.0)), ("gem", dict(p=16.0)), ("gem", dict(p=3.0))):
        pooled, T = P.pool_reference(x, one, zero, kind, **kw)
        g, S1, S2, dp = P.pool_backward_reference(np.ones((1, 2)), x, one, zero, zero, one, one, kind, **kw)
        assert np.isfinite(pooled).all() and np.isfinite(g).all() and (T is None or np.isfinite(T).all())
        assert 1e4 / 4 <= pooled[0, 1] <= 1e4
    x1 = np.random.RandomState(0).randn(2, 1, 8)                       # HW = 1: every kind returns a
    a = np.maximum(x1[:, 0], 0.0)
    for kind in KINDS:
        want = np.maximum(a, 1e-6) if kind == "gem" else a
        np.testing.assert_allclose(P.pool_reference(x1, np.ones(8), np.zeros(8), kind)[0], want, rtol=1e-12, atol=1e-15)
    with pytest.raises(ValueError):
        P.pool_reference(x, one, zero, "pcam")
    with pytest.raises(ValueError):
        P.pool_reference(x, one, zero, "max", act="gelu")


# ------------------------------------------------------------------------------------------------ the model surface
def _small():
    from chexpert_amd.models import DenseNet
    return DenseNet(32, (2, 2, 2, 2), 64, num_classes=5)


def test_set_pool_validation_and_state_dict_keys():
    model = _small()
    base = list(model.state_dict().keys())
    n_params = len(list(model.parameters()))
    assert model.pool_kind == "avg" and model.pool_state() == {"kind": "avg", "r": None}
    for kw in (dict(kind="pcam"), dict(kind="lse", r=0.0), dict(kind="lse", r=-1.0), dict(kind="lse", r=float("nan")), dict(kind="gem", p=0.5),
               dict(kind="gem", p=16.5), dict(kind="max", p=float("nan")), dict(kind=None), dict(kind="gem", p="three")):
        with pytest.raises(ValueError):
            model.set_pool(**kw)
        assert model.pool_kind == "avg" and list(model.state_dict().keys()) == base
    assert model.set_pool("max") is model and model.pool_kind == "max"
    assert list(model.state_dict().keys()) == base and len(list(model.parameters())) == n_params
    model.set_pool("lse", r=4.0)
    assert sorted(set(model.state_dict().keys()) - set(base)) == ["pool_r"] and len(list(model.parameters())) == n_params
    assert model.pool_r.shape == (1,) and model.pool_r.item() == 4.0 and model.pool_state() == {"kind": "lse", "r": 4.0}
    assert model.pool_param() is model.pool_r
    model.set_pool("gem", p=2.0)
    assert sorted(set(model.state_dict().keys()) - set(base)) == ["pool_p"]
    assert isinstance(model.pool_p, torch.nn.Parameter) and model.pool_p.shape == (1,) and model.pool_p.item() == 2.0
    assert model.pool_param() is model.pool_p and model.pool_state() == {"kind": "gem", "r": None}
    params = list(model.parameters())
    assert len(params) == n_params + 1 and params[-1] is model.pool_p           # the last one: its gradient is final first
    assert [n for n, _ in model.named_parameters()][-1] == "pool_p"
    model.set_pool("gem")
    assert model.pool_p.item() == 3.0
    model.set_pool("lse")
    assert model.pool_r.item() == 10.0
    model.set_pool()
    assert model.pool_kind == "avg" and list(model.state_dict().keys()) == base
    # pool_state / load_pool_state carry the kind (and r) to a fresh model, whose state_dict then takes the stored one
    src = _small().set_pool("lse", r=6.5)
    dst = _small().load_pool_state(src.pool_state())
    dst.load_state_dict(src.state_dict())
    assert dst.pool_kind == "lse" and dst.pool_r.item() == 6.5
    src = _small().set_pool("gem", p=5.0)
    dst = _small().load_pool_state(src.pool_state())
    dst.load_state_dict(src.state_dict())
    assert dst.pool_kind == "gem" and dst.pool_p.item() == 5.0
    assert _small().load_pool_state(None).pool_kind == "avg"


def test_set_pool_is_refused_once_the_engine_has_bound():
    """The engine flag decides (the flat parameter buffer exists), not a forward."""
    from chexpert_amd.models import Bottleneck, ResNet, construct_model
    for model in (_small(), ResNet(Bottleneck, [1, 1, 1, 1], num_classes=3), construct_model("efficientnet-b0", 3)):
        eng = model._eng()
        assert eng.flat is None and not model._pool_bound()
        model.set_pool("gem")                                          # an engine that has not bound yet does not lock the choice
        eng = model._eng()
        eng.flat = torch.zeros(4)                                      # what bind_params leaves behind
        assert model._pool_bound()
        with pytest.raises(RuntimeError, match="before the engine has bound"):
            model.set_pool("max")
        assert model.pool_kind == "gem" and "pool_p" in model.state_dict()
        with pytest.raises(ValueError):                                # validation comes first
            model.set_pool("pcam")
        eng.flat = None
    from chexpert_amd.optim import FusedAdam
    model = _small().set_pool("lse")
    FusedAdam(model, lr=1e-3)                                          # ... and so does a fused optimiser built over the parameters
    with pytest.raises(RuntimeError, match="before the engine has bound"):
        model.set_pool("gem")
    assert model.pool_kind == "lse"


def test_paths_that_assume_the_average_refuse_another_pool():
    from chexpert_amd import gradcam
    from chexpert_amd.models import DenseNet
    model = _small().set_pool("lse")
    x = torch.zeros(2, 3, 64, 64)
    with pytest.raises(NotImplementedError, match="set_pool"):
        gradcam.class_cam(model, x)
    with pytest.raises(NotImplementedError, match="set_pool"):
        gradcam.hooked_eval_forward(model, x)
    with pytest.raises(NotImplementedError, match="set_pool"):
        model.require_avg_pool("grad_cam")
    model.set_pool("avg").require_avg_pool("grad_cam")
    twin = DenseNet(12, (2, 2, 2), 24, num_classes=10).set_pool("max")          # CIFAR DenseNet-BC: the channel-padded twin
    with pytest.raises(NotImplementedError, match="set_pool"):
        twin._eng()
    assert DenseNet(12, (2, 2, 2), 24, num_classes=10).set_pool("avg")._eng() is not None


def test_finetune_groups_put_the_exponent_with_the_head():
    from chexpert_amd import optim as O
    model = _small().set_pool("gem")
    groups = {g["name"]: g for g in O.finetune_groups(model, weight_decay=1e-4, no_decay_norm_bias=True, freeze_backbone=True)}
    ids = lambda name: {id(q) for q in groups[name]["params"]}
    assert id(model.pool_p) in ids("head_no_decay") and groups["head_no_decay"]["weight_decay"] == 0.0
    assert not groups["head_no_decay"]["frozen"] and groups["backbone"]["frozen"]
    assert id(model.pool_p) not in ids("backbone") | ids("backbone_no_decay") | ids("head")
    plain = {g["name"]: g for g in O.finetune_groups(model)}
    assert id(model.pool_p) in {id(q) for q in plain["head"]["params"]}


# ------------------------------------------------------------------------------------------------ the C ABI
def test_entry_points_validate_without_launching():
    """cx_pool_head_fwd / cx_pool_head_bwd / cx_pool_p_grad (and the _f32 twins) check their arguments before any launch."""
    from chexpert_amd import _lib
    EINVAL, EALIGN, ESHAPE, ESTATROWS = -1, -2, -3, -5
    L = _lib.lib()
    f = [torch.zeros(4096, dtype=torch.float32) for _ in range(6)]
    X, V, O, A, Pm, G = (t.data_ptr() for t in f)
    assert all(q % 16 == 0 for q in (X, G))
    MAX, LSE, GEM, RELU, SWISH = 1, 2, 3, 1, 2
    for fwd, bwd in ((L.cx_pool_head_fwd, L.cx_pool_head_bwd), (L.cx_pool_head_fwd_f32, L.cx_pool_head_bwd_f32)):
        fw = lambda x=X, sc=V, sh=V, pooled=O, aux=A, param=Pm, B=2, HW=4, C=16, ldx=16, act=RELU, kind=GEM: \
            fwd(x, sc, sh, pooled, aux, param, B, HW, C, ldx, act, kind, None)
        assert fw(x=None) == EINVAL and fw(sc=None) == EINVAL and fw(sh=None) == EINVAL and fw(pooled=None) == EINVAL
        assert fw(param=None) == EINVAL and fw(param=None, kind=LSE) == EINVAL and fw(aux=None) == EINVAL and fw(aux=None, kind=LSE) == EINVAL
        assert fw(aux=None, param=None, kind=MAX, B=0) == ESHAPE         # (the maximum needs neither)
        assert fw(kind=0) == EINVAL and fw(kind=4) == EINVAL and fw(kind=-1) == EINVAL           # the average has its own kernels
        assert fw(act=0) == EINVAL and fw(act=3) == EINVAL
        assert fw(C=12, ldx=16) == ESHAPE and fw(C=16, ldx=8) == ESHAPE and fw(C=8, ldx=12) == ESHAPE
        assert fw(B=0) == ESHAPE and fw(HW=0) == ESHAPE and fw(C=0, ldx=0) == ESHAPE
        assert fw(x=X + 4) == EALIGN
        bw = lambda dp=O, pooled=O, aux=A, param=Pm, x=X, sc=V, sh=V, mean=V, rstd=V, es=V, g=G, S1=A, S2=A, B=2, HW=4, C=16, ldx=16, ldg=16, \
            act=SWISH, kind=LSE, rows=0: bwd(dp, pooled, aux, param, x, sc, sh, mean, rstd, es, g, S1, S2, B, HW, C, ldx, ldg, act, kind, rows, None)
        for name in ("dp", "pooled", "x", "sc", "sh", "mean", "rstd", "es", "g", "S1", "S2", "param"):
            assert bw(**{name: None}) == EINVAL, name
        assert bw(param=None, kind=GEM) == EINVAL and bw(aux=None) == EINVAL and bw(aux=None, kind=GEM, B=0) == ESHAPE
        assert bw(kind=0) == EINVAL and bw(kind=7) == EINVAL and bw(act=0) == EINVAL and bw(act=-2) == EINVAL
        assert bw(C=20, ldx=24, ldg=24) == ESHAPE and bw(ldx=8) == ESHAPE and bw(ldg=8) == ESHAPE and bw(ldg=20) == ESHAPE
        assert bw(B=-1) == ESHAPE and bw(HW=0) == ESHAPE
        assert bw(x=X + 8) == EALIGN and bw(g=G + 4) == EALIGN
        assert bw(B=3, rows=2) == ESTATROWS and bw(B=3, rows=1, kind=MAX, param=None) == ESTATROWS
    pg = lambda dp=O, pooled=O, aux=A, p=Pm, out=G, B=2, C=16: L.cx_pool_p_grad(dp, pooled, aux, p, out, B, C, None)
    for name in ("dp", "pooled", "aux", "p", "out"):
        assert pg(**{name: None}) == EINVAL, name
    assert pg(B=0) == ESHAPE and pg(C=0) == ESHAPE
    assert all(not t.any() for t in f)                                 # nothing ran
    # declared in the header with the parameters the binding passes, and built from their own source file
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(root, "include", "chexpert_hip.h")).read(), flags=re.S)
    for name, n in (("cx_pool_head_fwd", 13), ("cx_pool_head_bwd", 22), ("cx_pool_p_grad", 8), ("cx_pool_head_fwd_f32", 13),
                    ("cx_pool_head_bwd_f32", 22)):
        m = re.search(r"\bint\s+%s\s*\(([^;{]*?)\)\s*;" % name, hdr, flags=re.S)
        assert m and len(_lib.SIGNATURES[name]) == m.group(1).count(",") + 1 == n
    assert "pool_head.hip" in open(os.path.join(root, "chexpert_amd", "csrc", "Makefile")).read()
    from chexpert_amd import ops
    assert ops.POOL_KINDS == {"avg": 0, "max": 1, "lse": 2, "gem": 3} and (ops.POOL_ACT_RELU, ops.POOL_ACT_SWISH) == (1, 2)


def test_cli_flags():
    from chexpert_amd import cli
    p = cli.build_parser()
    a = p.parse_args([])
    assert (a.pool, a.pool_r, a.pool_p) == (None, None, None)
    a = p.parse_args(["--pool", "gem", "--pool_p", "4.5"])
    assert cli.resolve_pool(a) == {"kind": "gem", "r": 10.0, "p": 4.5}
    assert cli.resolve_pool(p.parse_args(["--pool", "lse", "--pool_r", "5"])) == {"kind": "lse", "r": 5.0, "p": 3.0}
    assert cli.resolve_pool(p.parse_args([])) is None                  # not given: the checkpoint's, or the average
    with pytest.raises(SystemExit):
        p.parse_args(["--pool", "pcam"])
    for bad in (["--pool_r", "5"], ["--pool", "gem", "--pool_r", "5"], ["--pool", "lse", "--pool_p", "2"], ["--pool", "lse", "--pool_r", "0"],
                ["--pool", "gem", "--pool_p", "17"], ["--pool", "max", "--pool_p", "2"]):
        with pytest.raises(ValueError):
            cli.resolve_pool(p.parse_args(bad))
    # a flag that contradicts the checkpoint is refused; an absent flag takes the checkpoint's
    assert cli.pool_for_checkpoint(None, {"kind": "lse", "r": 4.0}) == {"kind": "lse", "r": 4.0}
    assert cli.pool_for_checkpoint({"kind": "lse", "r": 4.0, "p": 3.0}, {"kind": "lse", "r": 4.0})["kind"] == "lse"
    assert cli.pool_for_checkpoint(None, None)["kind"] == "avg"
    with pytest.raises(ValueError, match="--pool"):
        cli.pool_for_checkpoint({"kind": "gem", "r": 10.0, "p": 3.0}, {"kind": "lse", "r": 4.0})
    with pytest.raises(ValueError, match="--pool"):
        cli.pool_for_checkpoint({"kind": "max", "r": 10.0, "p": 3.0}, None)       # a checkpoint from before: the average
