"""GPU: the pooling heads other than the average (chexpert_amd/csrc/pool_head.hip; FusedNet.set_pool).

Kernel level: cx_pool_head_fwd / cx_pool_head_bwd / cx_pool_p_grad and their _f32 twins at the shapes of the head tests of
tests/test_glue_gpu.py, against chexpert_amd.pooling's float64 statements (which tests/test_pool_head_cpu.py holds against torch
autograd), computed from the inputs as stored.  The inputs are sign-safe (every x*sc + sh is at least 1e-2 from 0), carry NaN in
their pitch padding, and have three plants: a dead channel (z < 0 everywhere), an exact tie of the maximum at two pixels of one
column, and -- in the `huge` cases -- one activation of 1e4.  The cases without the 1e4 plant are there because the bounds are
relative to the largest reference magnitude: next to 1e4 they would say little about the other columns.

Bounds (those of tests/test_glue_gpu.py for the average pair): pooled, T, S1, S2 and dp within 1e-4 of the largest reference magnitude;
g element-wise within eps |ref| + 1e-5 max|ref|, eps = 2^-8 (bf16) / 2^-24 (fp32).  Measured maxima: DESIGN.md section 4.43.

Model level: the comparisons with the oracle run in fp32 storage; the bit-for-bit comparisons (autograd route, graph replay, "avg"
against a model that never called set_pool) in bf16 storage, the mode whose weight gradients are reproducible (the fp32 mode adds
its weight-gradient partial sums with fp32 atomics, so two runs of the SAME model differ in their last bits there).  One training step of a small DenseNet, Bottleneck ResNet and efficientnet-b0 against the oracle with the
torch pooling put in from outside, the autograd route, graph replay, FusedAdam on pool_p, the eval-mode input gradient, refusals,
the command line's checkpoint round trip, two ranks, and set_pool("avg") against a model that never called it."""
import json
import math
import os
import time

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from chexpert_amd import pooling as P
from chexpert_amd import synth
from eager_step import _eager_dev_step

pytestmark = pytest.mark.gpu

BF, F32 = torch.bfloat16, torch.float32
STORAGE = [pytest.param(BF, id="bf16"), pytest.param(F32, id="f32")]
SENT = 7.0
NAN = float("nan")
SUM_TOL = 1e-4
CASE = "?"
CX_ESTATROWS = -5
ACT = {"relu": 1, "swish": 2}
KIND = {"max": 1, "lse": 2, "gem": 3}


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    from chexpert_amd import _lib
    _lib.lib()
    return torch.device("cuda:0")


@pytest.fixture(autouse=True)
def _case_id(request):
    global CASE
    CASE = request.node.name


def bf(t):
    return t.to(BF).float()


def stored(t, dt):                     # the values a tensor of storage type dt holds, as fp32
    return bf(t) if dt == BF else t.float()


def rnd(seed, shape, lo=-1.0, hi=1.0):
    g = torch.Generator().manual_seed(seed)
    return torch.rand(shape, generator=g) * (hi - lo) + lo


def mag(seed, shape, lo, hi):          # magnitude in [lo, hi], random sign
    g = torch.Generator().manual_seed(seed)
    v = torch.rand(shape, generator=g) * (hi - lo) + lo
    return v * (torch.randint(0, 2, shape, generator=g).float() * 2 - 1)


def full(dev, shape, dt=F32, v=SENT):
    return torch.full(shape, v, device=dev, dtype=dt)


def pitched(vals, ld, dev, dt, pad=NAN):
    """(rows, C) values -> (rows, ld) device buffer of the storage type; the columns behind C hold `pad` (NaN: an input whose
    padding must not be read)."""
    rows, C = vals.shape
    buf = torch.full((rows, ld), pad, dtype=dt)
    buf[:, :C] = vals.to(dt)
    return buf.to(dev)


def entry(name, dt):
    from chexpert_amd._lib import lib
    return getattr(lib(), name + ("_f32" if dt == F32 else ""))


def last_rows():
    from chexpert_amd._lib import lib
    return lib().cx_last_stat_rows()


def close(got, want, what, rel=SUM_TOL):
    want = torch.as_tensor(want, dtype=torch.float64)
    got = torch.as_tensor(got).double().cpu()
    assert bool(torch.isfinite(got).all()), "%s is not finite" % what
    err = (got - want).abs().max().item() / (want.abs().max().item() + 1e-300)
    print("ERR sum %s %s %.3e" % (CASE, what, err))
    assert err < rel, "%s: rel err %.3e" % (what, err)


def close_elem(got, want, dt, what):
    """|got - ref| <= eps |ref| + 1e-5 max|ref|; prints the largest additive part the elements need, in units of max|ref|."""
    want = torch.as_tensor(want, dtype=torch.float64)
    got = got.double().cpu()
    assert bool(torch.isfinite(got).all()), "%s is not finite" % what
    eps = 2.0 ** -8 if dt == BF else 2.0 ** -24
    d = (got - want).abs_().sub_(want.abs().mul_(eps))
    worst = d.max().item() / (want.abs().max().item() + 1e-300)
    print("ERR elem %s %s %.3e" % (CASE, what, worst))
    assert worst <= 1e-5, "%s: %.3e of max|ref| beyond half an ulp" % (what, worst)


def sign_safe(seed, shape, dt, plant=None):
    """x, sc, sh with x = (z - sh) / sc rounded to the storage type for |z| in [0.05, 2] and |sc| in [0.5, 1.5], both of random sign
    (a negative gamma is legal); `plant(z)` may overwrite entries of z first.  Returns x as stored, sc, sh and z = x*sc + sh in
    float64, whose distance from 0 is asserted: no float64 / fp32 disagreement about a sign is possible."""
    C = shape[-1]
    z = mag(seed, shape, 0.05, 2.0)
    if plant is not None:
        plant(z)
    sc, sh = mag(seed + 1, (C,), 0.5, 1.5), rnd(seed + 2, (C,), -0.5, 0.5)
    x = stored((z - sh) / sc, dt)
    zz = x.double() * sc.double() + sh.double()
    margin = zz.abs().min().item()
    print("MARGIN %s min|x*sc+sh| %.4f, %d of %d gammas negative" % (CASE, margin, int((sc < 0).sum()), C))
    assert margin > 1e-2
    assert C < 16 or bool((sc < 0).any())
    return x, sc, sh, zz


# ------------------------------------------------------------------------------------------------ 1. kernels
SHAPES = [  # B, HW, C, ldx
    (1, 1, 8, 8),                 # HW = 1: every kind returns a
    (3, 25, 128, 192),            # pitched
    (17, 4, 264, 264),            # 561 threads in workgroups of 128
    (2, 100, 2048, 2112),
    (5, 49, 1024, 1024),          # densenet121's head
]
DEAD, TIE, HUGE = 3, 5, 6         # the channels of the plants


def sid(s):
    return "B%d_HW%d_C%d_ld%d" % tuple(s)


def planted(shape, dt, huge):
    """The inputs of one case.  Dead channel: z < 0 at every pixel of every image.  Tie: z = 3 (above every other |z| <= 2) at two
    pixels of channel TIE in every image -- equal z gives equal stored x, so the two activations are equal bit for bit.  huge: one
    z = 1e4 in the last image."""
    B, HW, C, ldx = shape
    tie = (1, HW - 1) if HW >= 3 else None

    def plant(z):
        z[:, :, DEAD] = -z[:, :, DEAD].abs()
        if tie is not None:
            z[:, tie[0], TIE] = z[:, tie[1], TIE] = 3.0
        if huge:
            z[B - 1, HW // 2, HUGE] = 1e4
    x, sc, sh, zz = sign_safe(301, (B, HW, C), dt, plant)
    if tie is not None:
        assert bool((x[:, tie[0], TIE] == x[:, tie[1], TIE]).all())
    return x, sc, sh, zz, tie


@pytest.mark.parametrize("huge", [False, True], ids=["plain", "huge"])
@pytest.mark.parametrize("act", ["relu", "swish"])
@pytest.mark.parametrize("dt", STORAGE)
@pytest.mark.parametrize("shape", SHAPES, ids=sid)
def test_pool_head_kernels(dev, shape, dt, act, huge):
    """Forward, backward (atomic sums with a pitched g; rows mode twice; below B rows) and the exponent's gradient of every kind, with
    r = 10 and p = 3; in the `huge` cases also p = 16 and p = 1, where everything must stay finite and dp must not move."""
    from chexpert_amd._lib import lib, ptr, check, stream_ptr
    B, HW, C, ldx = shape
    x, sc, sh, zz, tie = planted(shape, dt, huge)
    xn, scn, shn = x.double().numpy(), sc.double().numpy(), sh.double().numpy()
    xd, scd, shd = pitched(x.view(-1, C), ldx, dev, dt), sc.to(dev), sh.to(dev)
    dp = mag(306, (B, C), 0.25, 1.0)
    mu, r_, es = rnd(307, (C,), -0.5, 0.5), rnd(308, (C,), 0.5, 2.0), mag(309, (C,), 0.5, 1.5)
    dpd, mud, rd, esd = (t.to(dev) for t in (dp, mu, r_, es))
    fwd, bwd = entry("cx_pool_head_fwd", dt), entry("cx_pool_head_bwd", dt)
    ldg = C + 8
    cases = [("max", None), ("lse", 10.0), ("gem", 3.0)] + ([("gem", 16.0), ("gem", 1.0)] if huge else [])
    for kind, pv in cases:
        tag = kind if pv is None else "%s(%g)" % (kind, pv)
        kw = {"r": pv} if kind == "lse" else {"p": pv} if kind == "gem" else {}
        par = None if pv is None else torch.tensor([pv], device=dev)
        want_p, want_T = P.pool_reference(xn, scn, shn, kind, act, **kw)
        want_g, S1, S2, want_dp = P.pool_backward_reference(dp.double().numpy(), xn, scn, shn, mu.double().numpy(), r_.double().numpy(),
                                                           es.double().numpy(), kind, act, **kw)
        # forward
        pooled, aux = full(dev, (B, C)), full(dev, (B, C))
        check(fwd(ptr(xd), ptr(scd), ptr(shd), ptr(pooled), ptr(aux), ptr(par), B, HW, C, ldx, ACT[act], KIND[kind], stream_ptr()), "cx_pool_head_fwd")
        close(pooled, want_p, "pooled " + tag)
        if kind == "max":
            assert bool((aux == SENT).all()), "the maximum leaves nothing in aux"
        else:
            close(aux, want_T, ("T " if kind == "gem" else "pooled - max ") + tag)
        if HW == 1:                                                 # every kind returns a (GeM: its clamp of a)
            a1 = torch.from_numpy(P.activation(zz.numpy(), act)[0][:, 0])
            close(pooled, a1.clamp_min(1e-6) if kind == "gem" else a1, "pooled = a at HW = 1 " + tag)
        # backward: atomic sums, pitched g
        g, st = full(dev, (B * HW, ldg), dt), torch.zeros(2, C, device=dev)
        args = (ptr(dpd), ptr(pooled), ptr(aux), ptr(par), ptr(xd), ptr(scd), ptr(shd), ptr(mud), ptr(rd), ptr(esd))
        check(bwd(*args, ptr(g), ptr(st[0]), ptr(st[1]), B, HW, C, ldx, ldg, ACT[act], KIND[kind], 0, stream_ptr()), "cx_pool_head_bwd")
        assert bool((g[:, C:] == SENT).all()), "a write into the pitch padding of g"
        gv = g[:, :C].float().view(B, HW, C)
        close_elem(gv, want_g, dt, "g " + tag)
        close(st[0], S1, "S1 atomic " + tag)
        close(st[1], S2, "S2 atomic " + tag)
        if act == "relu" or kind == "gem":                          # the dead channel: nothing flows (swish' is not 0 below 0)
            assert not bool(gv[:, :, DEAD].any()) and float(st[0][DEAD]) == 0.0 and float(st[1][DEAD]) == 0.0
        if kind == "max" and tie is not None:                       # the tie goes to the first pixel
            assert bool((gv[:, tie[0], TIE] != 0).all()) and not bool(gv[:, tie[1], TIE].any())
            assert int((gv != 0).sum()) <= B * C and int((gv[:, :, TIE] != 0).sum()) == B
        # rows mode: exactly B rows, row b = the sums of image b; two calls give equal bits
        outs = []
        for _ in range(2):
            g2, rows = full(dev, (B * HW, ldg), dt), full(dev, (2, B + 3, C))
            check(bwd(*args, ptr(g2), ptr(rows[0]), ptr(rows[1]), B, HW, C, ldx, ldg, ACT[act], KIND[kind], B + 3, stream_ptr()), "cx_pool_head_bwd")
            assert last_rows() == B and bool((rows[:, B:] == SENT).all())
            assert torch.equal(g2, g)
            outs.append(rows[:, :B].clone())
        assert torch.equal(outs[0], outs[1])
        close(outs[0][0].sum(0), S1, "S1 rows " + tag)
        close(outs[0][1].sum(0), S2, "S2 rows " + tag)
        if B > 1:
            g2, rows = full(dev, (B * HW, ldg), dt), full(dev, (2, B, C))
            assert bwd(*args, ptr(g2), ptr(rows[0]), ptr(rows[1]), B, HW, C, ldx, ldg, ACT[act], KIND[kind], B - 1, stream_ptr()) == CX_ESTATROWS
            assert bool((g2 == SENT).all()) and bool((rows == SENT).all())
        # the exponent's gradient: added to what dp holds, in a fixed order; the dead channel adds exactly nothing; clamped: nothing
        if kind == "gem":
            pg = lib().cx_pool_p_grad
            got = []
            for scale_dead in (1.0, 1e6, 1.0):
                d2 = dp.clone()
                d2[:, DEAD] *= scale_dead
                acc = torch.full((1,), 0.25, device=dev)
                check(pg(ptr(d2.to(dev)), ptr(pooled), ptr(aux), ptr(par), ptr(acc), B, C, stream_ptr()), "cx_pool_p_grad")
                got.append(acc.clone())
            assert torch.equal(got[0], got[1]) and torch.equal(got[0], got[2]), "the dead channel moved dp, or two calls differ"
            if pv in (1.0, 16.0):
                assert want_dp == 0.0 and float(got[0]) == 0.25, "clamped p: dp must not move"
            elif HW == 1:                                           # pooled = a': T = ln pooled in every column
                assert abs(want_dp) < 1e-12 and float(got[0]) == 0.25
            else:
                close(got[0] - 0.25, [want_dp], "dp " + tag)


# ------------------------------------------------------------------------------------------------ 2. models
def _rel(a, b):
    return (a.double() - b.double()).abs().max().item() / (b.double().abs().max().item() + 1e-12)


def torch_pool(a, kind, r, p):
    """The torch pooling of an NCHW activation: the oracle's side."""
    if kind == "avg":
        return a.mean((2, 3))
    if kind == "max":
        return F.adaptive_max_pool2d(a, 1).flatten(1)
    if kind == "lse":
        return (torch.logsumexp(r * a.flatten(2), 2) - math.log(a.shape[2] * a.shape[3])) / r
    q = p.clamp(1.0, 16.0)
    return a.clamp_min(1e-6).pow(q).flatten(2).mean(2).pow(1.0 / q)


def _family(net, dev, n_cls=5, seed=21, storage="fp32"):
    """(fused model in `storage` with the state dict loaded, state dict, input size, oracle forward(sd, x, kind, r) with the torch
    pooling applied to the tap in front of the average)."""
    from oracle import nets
    if net == "densenet":
        from chexpert_amd.models import DenseNet
        cfg, S = (2, 2, 2, 2), 64
        sd = synth.fill_state_dict_(nets.zeros_state_dict(nets.densenet_spec(n_cls, block_config=cfg)), seed)
        for k in sd:                       # well-conditioned regime (tests/test_model_gpu.py)
            if k.endswith(".bias") and "classifier" not in k:
                sd[k] = torch.full_like(sd[k], 2.5)
            if k.endswith(".weight") and sd[k].dim() == 1:
                sd[k] = synth.uniform(7, sd[k].shape, 0.8, 1.2)
        model = DenseNet(32, cfg, 64, num_classes=n_cls)
        body = lambda s, xx, taps: nets.densenet_forward(s, xx, cfg, train=True, taps=taps)
        tap, act, fc = "norm5", F.relu, "classifier"
    elif net == "resnet":
        from chexpert_amd.models import Bottleneck, ResNet
        layers, S = (1, 1, 1, 1), 64
        sd = synth.fill_state_dict_(nets.zeros_state_dict(nets.resnet_spec(n_cls, layers=layers)), seed)
        model = ResNet(Bottleneck, list(layers), num_classes=n_cls)
        body = lambda s, xx, taps: nets.resnet_forward(s, xx, layers, train=True, taps=taps)
        tap, act, fc = "layer4", (lambda t: t), "fc"
    else:
        from chexpert_amd.models import construct_model
        from chexpert_amd.models.efficientnet import DropMarker
        name, S = "efficientnet-b0", 224
        sd = synth.fill_state_dict_(nets.zeros_state_dict(nets.efficientnet_spec(name, n_cls)), seed)
        synth.smooth_state_dict_(sd, 1.0)
        model = construct_model(name, n_cls)
        for mod in model.modules():
            if isinstance(mod, DropMarker):
                mod.p = 0.0
        body = lambda s, xx, taps: nets.efficientnet_forward(s, xx, name, train=True, taps=taps)
        tap, act, fc = "head1", (lambda t: t * torch.sigmoid(t)), "head.6"
    model.storage_dtype(storage).load_state_dict(sd, strict=True)

    def forward(s, xx, kind, r):
        taps = {}
        body({k: v for k, v in s.items() if k != "pool_p"}, xx, taps)
        pooled = torch_pool(act(taps[tap]), kind, r, s.get("pool_p"))
        return F.linear(pooled, s[fc + ".weight"], s[fc + ".bias"])
    return model.to(dev), sd, S, forward


@pytest.mark.parametrize("kind", ["max", "lse", "gem"])
@pytest.mark.parametrize("net", ["densenet", "resnet", "efficientnet"])
def test_one_training_step_against_the_oracle(dev, net, kind):
    """Bounds of tests/test_fp32_gpu.py: logits within 1e-3 of the logit scale, loss within 1e-4 relative; for lse and gem every conv
    or linear gradient, and pool_p's, at cos >= 0.9999 and a norm ratio within 1e-3.  For max only logits and loss: an arg-max within
    rounding of a tie flips discontinuously (its gradient is covered at kernel level)."""
    from oracle import step
    model, sd, S, forward = _family(net, dev)
    r, p = 4.0, 2.5
    model.set_pool(kind, r=r, p=p)
    B, n_cls = 4, 5
    x, t = synth.xray_batch(1234, B, S), synth.targets(99, B, n_cls)
    sd_o = {k: v.clone() for k, v in sd.items()}
    if kind == "gem":
        sd_o["pool_p"] = torch.tensor([p])
    loss_o, logits_o, grads_o = step.train_step(lambda s, xx: forward(s, xx, kind, r), sd_o, x, t)
    model.train()
    loss, logits = model.forward_backward(x.to(dev), t.to(dev))
    e = _rel(logits.cpu(), logits_o)
    print("POOL %s %s: train logits rel %.3e, loss %.6f (oracle %.6f)" % (net, kind, e, loss.item(), loss_o.item()))
    assert e < 1e-3
    assert abs(loss.item() - loss_o.item()) < 1e-4 * abs(loss_o.item())
    if kind == "max":
        return
    worst = []
    for k, q in model.named_parameters():
        if q.dim() not in (2, 4) and k != "pool_p":                 # conv and linear weights, and the exponent
            continue
        a, b = q.grad.cpu().double().flatten(), grads_o[k].double().flatten()
        assert b.norm().item() > 0, k
        worst.append((float((a * b).sum() / (a.norm() * b.norm())), abs(float(a.norm() / b.norm()) - 1), k))
    worst.sort()
    ratio = max(worst, key=lambda w: w[1])
    print("POOL %s %s: worst cos %.7f (%s), worst norm ratio - 1 %.3e (%s), %d tensors" % (net, kind, worst[0][0], worst[0][2], ratio[1], ratio[2],
                                                                                            len(worst)))
    if kind == "gem":
        assert any(k == "pool_p" for _, _, k in worst) and float(model.pool_p.grad.abs()) > 0
    assert worst[0][0] >= 0.9999 and ratio[1] <= 1e-3, (worst[:3], ratio)


def _pair(net, dev, kind, **kw):
    a, sd, S, _ = _family(net, dev, storage="bf16")
    b = _family(net, dev, storage="bf16")[0]
    a.set_pool(kind, **kw)
    b.set_pool(kind, **kw)
    return a.train(), b.train(), S


@pytest.mark.parametrize("net,kind", [("densenet", "gem"), ("densenet", "lse"), ("densenet", "max"), ("resnet", "gem"), ("efficientnet", "gem"),
                                      ("efficientnet", "lse")])
def test_fused_step_equals_the_autograd_route(dev, net, kind):
    """forward_backward against model(x) + the BCE + loss.backward(): the same kernels, so loss, logits and every gradient agree bit
    for bit (the comparison of tests/test_multiclass_gpu.py); then the eval-mode step fills a finite, non-zero input gradient."""
    a, b, S = _pair(net, dev, kind)
    B, n = 4, 5
    x, t = synth.xray_batch(2500, B, S).to(dev), synth.targets(2510, B, n).to(dev)
    loss_a, logits_a = a.forward_backward(x, t)
    from chexpert_amd.loss import MaskedBCE
    out = b(x)
    loss_b = MaskedBCE()(out, t)                                    # the loss kernel of the autograd route: the plain step's bits
    loss_b.backward()
    assert torch.equal(logits_a, out.detach()) and torch.equal(loss_a.reshape(()), loss_b.detach())
    ga, gb = dict(a.named_parameters()), dict(b.named_parameters())
    assert list(ga) == list(gb) and (("pool_p" in ga) == (kind == "gem"))
    for k in ga:
        assert torch.equal(ga[k].grad, gb[k].grad), k
    assert max(float(q.grad.abs().max()) for q in ga.values()) > 0
    if kind == "gem":
        assert float(a.pool_p.grad.abs()) > 0
        assert a.pool_p.grad.data_ptr() == a._eng().grad_of(a.pool_p).data_ptr()       # it lives in the flat gradient buffer, at its end
        assert a._eng().off_of[id(a.pool_p)] == max(a._eng().offsets)
    a.zero_grad(set_to_none=True)
    a.eval()
    buf = torch.full((B, 3, S, S), 7.0, device=dev)
    loss_e, _ = a.forward_backward(x, t, input_grad=buf)
    assert math.isfinite(loss_e.item()) and bool(torch.isfinite(buf).all()) and float(buf.abs().max()) > 0 and not bool((buf == 7.0).any())
    xg = x.clone().requires_grad_(True)                             # ... and so does autograd through the eval forward (saliency.py's route)
    b.eval()
    b(xg)[:, 0].sum().backward()
    assert bool(torch.isfinite(xg.grad).all()) and float(xg.grad.abs().max()) > 0


def test_avg_is_untouched_and_refusals(dev):
    """set_pool("avg") against a model that never called it: bit-identical loss, logits and gradients.  class_cam and the hook path
    refuse another pooling; set_pool after the first forward is refused."""
    from chexpert_amd import gradcam
    plain, _, S, _ = _family("densenet", dev, storage="bf16")
    called = _family("densenet", dev, storage="bf16")[0].set_pool("avg")
    x, t = synth.xray_batch(2600, 4, S).to(dev), synth.targets(2610, 4, 5).to(dev)
    la, oa = plain.train().forward_backward(x, t)
    lb, ob = called.train().forward_backward(x, t)
    assert torch.equal(la, lb) and torch.equal(oa, ob)
    assert list(plain.state_dict().keys()) == list(called.state_dict().keys())
    for (k, q), (_, w) in zip(plain.named_parameters(), called.named_parameters()):
        assert torch.equal(q.grad, w.grad), k
    with pytest.raises(RuntimeError, match="before the engine has bound"):
        called.set_pool("max")
    lse = _family("densenet", dev)[0].set_pool("lse")
    with pytest.raises(NotImplementedError, match="set_pool"):
        gradcam.class_cam(lse, x)
    with pytest.raises(NotImplementedError, match="set_pool"):
        gradcam.grad_cam(lse, x)
    lse.eval()
    with torch.no_grad():
        assert bool(torch.isfinite(lse(x)).all())


@pytest.mark.parametrize("kind", ["gem", "lse"])
def test_graphed_step_equals_eager_and_the_exponent_trains(dev, kind):
    """A graph replay equals the eager step bit for bit over three steps; pool_p moves under FusedAdam; pool_r changed in place is seen
    by a replay."""
    from chexpert_amd.graph import GraphedTrainStep
    from chexpert_amd.optim import FusedAdam
    m_e, m_g, S = _pair("densenet", dev, kind, r=4.0)
    B, n = 4, 5
    xs = [synth.xray_batch(2800 + i, B, S).to(dev) for i in range(4)]
    ts = [synth.targets(2810 + i, B, n).to(dev) for i in range(4)]
    opt_e, opt_g = FusedAdam(m_e, lr=1e-2), FusedAdam(m_g, lr=1e-2)
    gs = GraphedTrainStep(m_g, opt_g, xs[0], ts[0])
    flat = lambda m: torch.cat([q.detach().flatten() for q in m.parameters()])                               # noqa: E731
    p0 = m_e.pool_p.item() if kind == "gem" else None
    for i in range(3):
        le = _eager_dev_step(m_e, opt_e, xs[i], ts[i])
        lg, _ = gs.replay(xs[i], ts[i])
        assert torch.equal(le, lg), (i, le.item(), lg.item())
        assert torch.equal(flat(m_e), flat(m_g)), i
        assert torch.equal(m_e._eng().flat_grad, m_g._eng().flat_grad)
    if kind == "gem":
        assert m_e.pool_p.item() != p0 and 1.0 < m_e.pool_p.item() < 16.0 and m_g.pool_p.item() == m_e.pool_p.item()
    else:
        held = m_g.pool_r.data_ptr()
        m_g.pool_r.fill_(9.0)
        m_e.pool_r.fill_(9.0)
        le = _eager_dev_step(m_e, opt_e, xs[3], ts[3])
        lg, logits9 = gs.replay(xs[3], ts[3])
        assert m_g.pool_r.data_ptr() == held and torch.equal(le, lg) and torch.equal(flat(m_e), flat(m_g))
        m_e.pool_r.fill_(4.0)                                         # ... and it matters: the first r gives other logits
        m_e.eval()
        m_g.eval()
        with torch.no_grad():
            assert not torch.equal(m_e(xs[3]), m_g(xs[3]))


# ------------------------------------------------------------------------------------------------ data parallel
def _dp_worker(rank, world, port, out_dir):
    import torch.distributed as dist
    os.environ["MASTER_ADDR"], os.environ["MASTER_PORT"] = "127.0.0.1", str(port)
    dev = torch.device("cuda:%d" % rank)
    torch.cuda.set_device(dev)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    from chexpert_amd.parallel import broadcast_module_state
    model, _, S, _ = _family("densenet", dev)
    model.set_pool("gem").train()
    broadcast_module_state(model)
    x, t = synth.xray_batch(3100 + rank, 4, S).to(dev), synth.targets(3200 + rank, 4, 5).to(dev)
    model.forward_backward(x, t)                     # binds the engine; the single-process gradient of this shard, no reducer yet
    eng = model._eng()
    local = model.pool_p.grad.detach().cpu().clone()
    gathered = [torch.empty_like(local) for _ in range(world)]
    dist.all_gather(gathered, local)
    eng.enable_data_parallel(bucket_bytes=1 << 16)
    model.zero_grad()
    model.forward_backward(x, t)
    torch.cuda.synchronize()
    torch.save({"got": model.pool_p.grad.detach().cpu().clone(), "want": sum(gathered) / world, "local": local},
               os.path.join(out_dir, "rank%d.pt" % rank))
    dist.destroy_process_group()


def test_data_parallel_exponent_gradient_two_ranks(dev, tmp_path):
    """Two ranks, one device each: pool_p.grad after the data-parallel step is the mean of the two single-process gradients."""
    if torch.cuda.device_count() < 2:
        pytest.skip("needs two devices")
    import torch.multiprocessing as mp
    port = 36900 + (os.getpid() % 400)
    ctx = mp.spawn(_dp_worker, args=(2, port, str(tmp_path)), nprocs=2, join=False)
    deadline = time.time() + 300
    try:
        while not ctx.join(timeout=5):
            if time.time() > deadline:
                raise TimeoutError("the ranks ran longer than 300 s")
    finally:
        for p in ctx.processes:
            if p.is_alive():
                p.kill()
                p.join()
    recs = [torch.load(os.path.join(str(tmp_path), "rank%d.pt" % r)) for r in range(2)]
    assert not torch.equal(recs[0]["local"], recs[1]["local"])
    for rec in recs:
        assert abs(float(rec["got"]) - float(rec["want"])) <= 1e-6 * abs(float(rec["want"])), rec
    assert torch.equal(recs[0]["got"], recs[1]["got"])


# ------------------------------------------------------------------------------------------------ command line
_CLI = ["--train", "--synthetic", "32", "--batch_size", "4", "--resize", "64", "--eval_interval", "8", "--log_interval", "1", "--seed", "3",
        "--lr", "0.001", "--fused_optimizer", "--graph"]


def test_cli_checkpoint_round_trip_and_contradiction(dev, tmp_path, capsys):
    """--pool gem trains under --fused_optimizer --graph, the checkpoint stores pool_state, --restore without the flag reads the kind
    from it and continues, a contradicting --pool is refused before load_state_dict, --visualize without --saliency is refused."""
    from chexpert_amd import cli
    out = str(tmp_path / "g")
    model = cli.main(_CLI + ["--pool", "gem", "--pool_p", "4", "--output_dir", out])
    lines = [json.loads(l)["train_loss"] for l in capsys.readouterr().out.splitlines() if l.startswith('{"step"')]
    assert len(lines) == 8 and all(math.isfinite(v) for v in lines), lines
    assert model.pool_kind == "gem" and model.pool_p.item() != 4.0
    ck = os.path.join(out, "checkpoint_latest.pt")
    saved = torch.load(ck, map_location="cpu")
    assert saved["pool_state"] == {"kind": "gem", "r": None} and saved["state_dict"]["pool_p"].shape == (1,)
    model2 = cli.main(_CLI + ["--restore", ck, "--output_dir", str(tmp_path / "r")])
    capsys.readouterr()
    st2 = torch.load(os.path.join(str(tmp_path / "r"), "checkpoint_latest.pt"), map_location="cpu")
    assert model2.pool_kind == "gem" and st2["global_step"] == 16 and st2["pool_state"]["kind"] == "gem"
    for flags in (["--pool", "lse"], ["--pool", "avg"]):
        with pytest.raises(ValueError, match="--pool .* contradicts the checkpoint"):
            cli.main(_CLI + flags + ["--restore", ck, "--output_dir", str(tmp_path / "x")])
    with pytest.raises(ValueError, match="--saliency"):                # the kind comes from the checkpoint: refused before the model is built
        cli.main(["--visualize", "--synthetic", "32", "--batch_size", "4", "--resize", "64", "--restore", ck, "--output_dir", str(tmp_path / "v")])
    with pytest.raises(SystemExit):                                     # ... from the flags: a parser.error
        cli.main(["--visualize", "--pool", "max", "--synthetic", "32", "--resize", "64", "--output_dir", str(tmp_path / "w")])
    with pytest.raises(SystemExit):
        cli.main(["--visualize", "--pool", "max", "--saliency", "grad", "--cam_classes", "0", "--synthetic", "32", "--resize", "64", "--output_dir",
                  str(tmp_path / "w")])
