"""GPU: the class-specific residual attention head (chexpert_amd/csrc/csra_head.hip; FusedNet.set_head("csra")).

Kernel level: cx_csra_head_fwd / cx_csra_head_bwd and their _f32 twins against chexpert_amd.heads' float64 statements (which
tests/test_csra_head_cpu.py holds against torch autograd), computed from the inputs as stored.  The inputs are built as
tests/test_pool_head_gpu.py builds its own: sign-safe (every x*sc + sh is at least 1e-2 from 0), NaN in the pitch padding, a dead channel
(z < 0 everywhere) and -- in the `huge` cases -- one z = 1e4, beside which everything must stay finite.  lambda = 0.3, T = 2; one case
with lambda = 0, which is also held against the linear head.

Bounds (the project's for the average pair, tests/test_glue_gpu.py and tests/test_pool_head_gpu.py): logits, s, S1, S2, dW and db within
1e-4 of the largest reference magnitude; g element-wise within eps |ref| + 1e-5 max|ref|, eps = 2^-8 (bf16) / 2^-24 (fp32).  Measured
maxima: DESIGN.md section 4.45.

Model level: the comparisons with the oracle (torch CSRA applied to the tap) and with the linear head at lambda = 0 run in fp32 storage;
the bit-for-bit comparisons in bf16 storage, the mode whose weight gradients are reproducible."""
import json
import math
import os
import subprocess
import sys

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from chexpert_amd import heads as H
from chexpert_amd import synth
from chexpert_amd.pooling import activation
from eager_step import _eager_dev_step

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BF, F32 = torch.bfloat16, torch.float32
STORAGE = [pytest.param(BF, id="bf16"), pytest.param(F32, id="f32")]
SENT = 7.0
NAN = float("nan")
SUM_TOL = 1e-4
CASE = "?"
CX_EUNSUPPORTED, CX_ESTATROWS = -4, -5
ACT = {"relu": 1, "swish": 2}
LAM, TEMP = 0.3, 2.0


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


def stored(t, dt):                     # the values a tensor of storage type dt holds, as fp32
    return t.to(BF).float() if dt == BF else t.float()


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
SHAPES = [  # B, HW, C, ldx, n, activations, m given
    ((1, 1, 8, 8, 1), ("relu", "swish"), False),                 # HW = 1: the softmax of one pixel is 1
    ((3, 25, 128, 192, 5), ("relu", "swish"), False),            # pitched, NaN in the padding
    ((17, 4, 264, 264, 14), ("relu", "swish"), False),           # ragged C: 66 owners of 4 channels in workgroups of 128
    ((2, 100, 2048, 2112, 42), ("relu", "swish"), False),        # n above one 16- or 32-wide tile, four 512-channel chunks
    ((5, 49, 1024, 1024, 14), ("relu", "swish"), False),         # densenet121's head
    ((2, 144, 1792, 1792, 14), ("swish",), True),                # efficientnet-b4's head with the Dropout mask
]
CASES = [pytest.param(s, a, m, id="B%d_HW%d_C%d_ld%d_n%d_%s%s" % (s + (a, "_m" if m else ""))) for s, acts, m in SHAPES for a in acts]
DEAD, HUGE = 3, 6                 # the channels of the plants


def make_inputs(shape, dt, huge, with_m, dev):
    """The operands of one case, on the host (fp32 as stored; the reference reads these) and on the device."""
    B, HW, C, ldx, n = shape

    def plant(z):
        z[:, :, DEAD] = -z[:, :, DEAD].abs()
        if huge:
            z[B - 1, HW // 2, HUGE] = 1e4
    x, sc, sh, zz = sign_safe(401, (B, HW, C), dt, plant)
    h = {"x": x, "sc": sc, "sh": sh, "W": mag(403, (n, C), 0.02, 0.2), "b": rnd(404, (n,)), "dl": mag(405, (B, n), 0.25, 1.0),
         "mu": rnd(407, (C,), -0.5, 0.5), "r": rnd(408, (C,), 0.5, 2.0), "es": mag(409, (C,), 0.5, 1.5),
         "m": (rnd(410, (B, C), 0.0, 1.0) > 0.2).float() / 0.8 if with_m else None}
    d = {k: (None if v is None else v.to(dev)) for k, v in h.items() if k != "x"}
    d["x"] = pitched(x.view(-1, C), ldx, dev, dt)
    return h, d, zz


def references(h, lam, T, act):
    f = lambda k: None if h[k] is None else h[k].double().numpy()                                        # noqa: E731
    fw = H.csra_reference(f("x"), f("sc"), f("sh"), f("W"), f("b"), lam, T, act, f("m"))
    bw = H.csra_backward_reference(f("dl"), f("x"), f("sc"), f("sh"), f("mu"), f("r"), f("es"), f("W"), lam, T, act, f("m"))
    return fw, bw


def run_kernels(dev, shape, dt, act, huge, with_m, lam, T):
    from chexpert_amd._lib import lib, ptr, check, stream_ptr
    B, HW, C, ldx, n = shape
    h, d, zz = make_inputs(shape, dt, huge, with_m, dev)
    (want_logits, want_s, _, _), (want_g, S1, S2, want_dW, want_db) = references(h, lam, T, act)
    fwd, bwd = entry("cx_csra_head_fwd", dt), entry("cx_csra_head_bwd", dt)
    lt = torch.tensor([lam, T], device=dev)
    # forward
    logits, s, stat = full(dev, (B, n)), full(dev, (B, n, HW)), full(dev, (B, n, 4))
    check(fwd(ptr(d["x"]), ptr(d["sc"]), ptr(d["sh"]), ptr(d["m"]), ptr(d["W"]), ptr(d["b"]), ptr(lt), ptr(logits), ptr(s), ptr(stat), B, HW, C,
              ldx, n, ACT[act], stream_ptr()), "cx_csra_head_fwd")
    close(logits, want_logits, "logits")
    close(s, want_s, "s")
    if HW == 1:                                                     # the softmax of one pixel is 1
        close(logits, h["b"].double().numpy() + (1 + lam) * want_s[:, :, 0], "logits = b + (1 + lambda) s at HW = 1")
    # backward: atomic sums, pitched g, dW and db added to what they hold
    need = lib().cx_csra_bwd_scratch(B, HW, C, n)
    ldg = C + 8
    args = (ptr(d["dl"]), ptr(s), ptr(stat), ptr(lt), ptr(d["x"]), ptr(d["sc"]), ptr(d["sh"]), ptr(d["m"]), ptr(d["mu"]), ptr(d["r"]),
            ptr(d["es"]), ptr(d["W"]))

    def call(g, s1, s2, dW, db, scratch, rows):
        return bwd(*args, ptr(g), ptr(s1), ptr(s2), ptr(dW), ptr(db), ptr(scratch), scratch.numel(), B, HW, C, ldx, ldg, n, ACT[act], rows,
                   stream_ptr())
    g, st, dW, db, scr = full(dev, (B * HW, ldg), dt), torch.zeros(2, C, device=dev), full(dev, (n, C), v=0.5), full(dev, (n,), v=-0.25), \
        full(dev, (need,), v=NAN)
    check(call(g, st[0], st[1], dW, db, scr, 0), "cx_csra_head_bwd")
    assert bool((g[:, C:] == SENT).all()), "a write into the pitch padding of g"
    gv = g[:, :C].float().view(B, HW, C)
    close_elem(gv, want_g, dt, "g")
    close(st[0], S1, "S1 atomic")
    close(st[1], S2, "S2 atomic")
    close(dW.double() - 0.5, want_dW, "dW")
    close(db.double() + 0.25, want_db, "db")
    if act == "relu":                                               # the dead channel: nothing flows
        assert not bool(gv[:, :, DEAD].any()) and float(st[0][DEAD]) == 0.0 and float(st[1][DEAD]) == 0.0
        assert bool((dW[:, DEAD] == 0.5).all())
    # rows mode: exactly B rows, row b = the sums of image b; two calls give equal bits in every output
    outs = []
    for _ in range(2):
        g2, rows, dW2, db2 = full(dev, (B * HW, ldg), dt), full(dev, (2, B + 3, C)), full(dev, (n, C), v=0.5), full(dev, (n,), v=-0.25)
        check(call(g2, rows[0], rows[1], dW2, db2, full(dev, (need + 5,), v=NAN), B + 3), "cx_csra_head_bwd")
        assert last_rows() == B and bool((rows[:, B:] == SENT).all())
        assert torch.equal(g2, g)
        outs.append((rows[:, :B].clone(), dW2, db2))
    assert all(torch.equal(a, b) for a, b in zip(outs[0], outs[1]))
    assert torch.equal(outs[0][1], dW) and torch.equal(outs[0][2], db)
    close(outs[0][0][0].sum(0), S1, "S1 rows")
    close(outs[0][0][1].sum(0), S2, "S2 rows")
    if B > 1:                                                       # too few rows: refused with nothing written
        g2, rows, dW2, db2 = full(dev, (B * HW, ldg), dt), full(dev, (2, B, C)), full(dev, (n, C)), full(dev, (n,))
        scr2 = full(dev, (need,))
        assert call(g2, rows[0], rows[1], dW2, db2, scr2, B - 1) == CX_ESTATROWS
        assert all(bool((t == SENT).all()) for t in (g2, rows, dW2, db2, scr2))
    # a scratch that is too small is refused with nothing written
    g2, dW2 = full(dev, (B * HW, ldg), dt), full(dev, (n, C))
    assert call(g2, st[0], st[1], dW2, db, full(dev, (need - 1,)), 0) == CX_EUNSUPPORTED
    assert bool((g2 == SENT).all()) and bool((dW2 == SENT).all())
    return h, zz, logits


@pytest.mark.parametrize("huge", [False, True], ids=["plain", "huge"])
@pytest.mark.parametrize("dt", STORAGE)
@pytest.mark.parametrize("shape,act,with_m", CASES)
def test_csra_kernels(dev, shape, act, with_m, dt, huge):
    """Forward and backward (atomic sums with a pitched g; rows mode twice; below B rows; a short scratch) at lambda = 0.3, T = 2."""
    run_kernels(dev, shape, dt, act, huge, with_m, LAM, TEMP)


@pytest.mark.parametrize("dt", STORAGE)
def test_csra_kernels_lambda_zero_is_the_linear_head(dev, dt):
    """lambda = 0 at densenet121's head: every check of the case above, and the logits against F.linear on the average."""
    shape = (5, 49, 1024, 1024, 14)
    h, zz, logits = run_kernels(dev, shape, dt, "relu", False, False, 0.0, TEMP)
    a = torch.from_numpy(activation(zz.numpy(), "relu")[0])
    close(logits, F.linear(a.mean(1), h["W"].double(), h["b"].double()), "logits against the linear head")


@pytest.mark.parametrize("dt", STORAGE)
def test_more_than_64_classes_are_unsupported(dev, dt):
    from chexpert_amd._lib import ptr, stream_ptr
    B, HW, C, n = 2, 4, 16, 65
    f = lambda *s: full(dev, s)                                                                          # noqa: E731
    x, g = full(dev, (B * HW, C), dt), full(dev, (B * HW, C), dt)
    v, W, lt = f(C), f(n, C), torch.tensor([LAM, TEMP], device=dev)
    logits, s, stat, dl, dW, db, scr = f(B, n), f(B, n, HW), f(B, n, 4), f(B, n), f(n, C), f(n), f(1 << 16)
    assert entry("cx_csra_head_fwd", dt)(ptr(x), ptr(v), ptr(v), None, ptr(W), ptr(v), ptr(lt), ptr(logits), ptr(s), ptr(stat), B, HW, C, C, n,
                                         1, stream_ptr()) == CX_EUNSUPPORTED
    assert entry("cx_csra_head_bwd", dt)(ptr(dl), ptr(s), ptr(stat), ptr(lt), ptr(x), ptr(v), ptr(v), None, ptr(v), ptr(v), ptr(v), ptr(W), ptr(g),
                                         ptr(v), ptr(v), ptr(dW), ptr(db), ptr(scr), scr.numel(), B, HW, C, C, C, n, 1, 0,
                                         stream_ptr()) == CX_EUNSUPPORTED
    torch.cuda.synchronize()
    assert all(bool((t == SENT).all()) for t in (logits, s, stat, g, dW, db, scr))


# ------------------------------------------------------------------------------------------------ 2. models
def _rel(a, b):
    return (a.double() - b.double()).abs().max().item() / (b.double().abs().max().item() + 1e-12)


def torch_csra(a, W, b, lam, T):
    """The torch CSRA of an NCHW activation: the oracle's side."""
    s = torch.einsum("kc,bchw->bkhw", W, a).flatten(2)
    return b + s.mean(2) + lam * (torch.softmax(T * s, 2) * s).sum(2)


def _family(net, dev, n_cls=5, seed=21, storage="fp32"):
    """(fused model in `storage` with the state dict loaded, state dict, input size, oracle forward(sd, x, lam, T) with the torch CSRA
    applied to the tap in front of the average; lam None: the linear head)."""
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
        body = lambda s, xx, taps: nets.densenet_forward(s, xx, cfg, train=True, taps=taps)              # noqa: E731
        tap, act, fc = "norm5", F.relu, "classifier"
    elif net == "resnet":
        from chexpert_amd.models import Bottleneck, ResNet
        layers, S = (1, 1, 1, 1), 64
        sd = synth.fill_state_dict_(nets.zeros_state_dict(nets.resnet_spec(n_cls, layers=layers)), seed)
        model = ResNet(Bottleneck, list(layers), num_classes=n_cls)
        body = lambda s, xx, taps: nets.resnet_forward(s, xx, layers, train=True, taps=taps)             # noqa: E731
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
        body = lambda s, xx, taps: nets.efficientnet_forward(s, xx, name, train=True, taps=taps)         # noqa: E731
        tap, act, fc = "head1", (lambda t: t * torch.sigmoid(t)), "head.6"
    model.storage_dtype(storage).load_state_dict(sd, strict=True)

    def forward(s, xx, lam, T):
        taps = {}
        body(s, xx, taps)
        return torch_csra(act(taps[tap]), s[fc + ".weight"], s[fc + ".bias"], lam, T)
    return model.to(dev), sd, S, forward


@pytest.mark.parametrize("net", ["densenet", "resnet", "efficientnet"])
def test_one_training_step_against_the_oracle(dev, net):
    """Bounds of tests/test_fp32_gpu.py: logits within 1e-3 of the logit scale, loss within 1e-4 relative, every conv or linear gradient
    at cos >= 0.9999 and a norm ratio within 1e-3."""
    from oracle import step
    model, sd, S, forward = _family(net, dev)
    model.set_head("csra", lam=LAM, T=TEMP)
    B, n_cls = 4, 5
    x, t = synth.xray_batch(1234, B, S), synth.targets(99, B, n_cls)
    loss_o, logits_o, grads_o = step.train_step(lambda s, xx: forward(s, xx, LAM, TEMP), {k: v.clone() for k, v in sd.items()}, x, t)
    model.train()
    loss, logits = model.forward_backward(x.to(dev), t.to(dev))
    e = _rel(logits.cpu(), logits_o)
    print("CSRA %s: train logits rel %.3e, loss %.6f (oracle %.6f)" % (net, e, loss.item(), loss_o.item()))
    assert e < 1e-3
    assert abs(loss.item() - loss_o.item()) < 1e-4 * abs(loss_o.item())
    worst = []
    for k, q in model.named_parameters():
        if q.dim() not in (2, 4):                                   # conv and linear weights
            continue
        a, b = q.grad.cpu().double().flatten(), grads_o[k].double().flatten()
        assert b.norm().item() > 0, k
        worst.append((float((a * b).sum() / (a.norm() * b.norm())), abs(float(a.norm() / b.norm()) - 1), k))
    worst.sort()
    ratio = max(worst, key=lambda w: w[1])
    print("CSRA %s: worst cos %.7f (%s), worst norm ratio - 1 %.3e (%s), %d tensors" % (net, worst[0][0], worst[0][2], ratio[1], ratio[2],
                                                                                       len(worst)))
    assert any(q.dim() == 2 for q in model.parameters())
    assert worst[0][0] >= 0.9999 and ratio[1] <= 1e-3, (worst[:3], ratio)


@pytest.mark.parametrize("net", ["densenet", "resnet", "efficientnet"])
def test_lambda_zero_against_the_linear_head(dev, net):
    """fp32 storage: the csra model at lambda = 0 against the linear-head model with the same weights: logits within 1e-4 of the logit
    scale (the order of the sums differs, so the bits may)."""
    csra, _, S, _ = _family(net, dev)
    lin = _family(net, dev)[0]
    csra.set_head("csra", lam=0.0, T=TEMP)
    x, t = synth.xray_batch(2400, 4, S).to(dev), synth.targets(2410, 4, 5).to(dev)
    for mode in ("train", "eval"):
        getattr(csra, mode)()
        getattr(lin, mode)()
        with torch.no_grad():
            a, b = csra(x), lin(x)
        e = _rel(a, b)
        print("CSRA %s %s: lambda = 0 against the linear head, logits rel %.3e" % (net, mode, e))
        assert e < 1e-4


def _pair(net, dev, **kw):
    a, sd, S, _ = _family(net, dev, storage="bf16")
    b = _family(net, dev, storage="bf16")[0]
    a.set_head("csra", **kw)
    b.set_head("csra", **kw)
    return a.train(), b.train(), S


@pytest.mark.parametrize("net", ["densenet", "resnet", "efficientnet"])
def test_fused_step_equals_the_autograd_route_and_repeats(dev, net):
    """forward_backward against model(x) + the BCE + loss.backward(): the same kernels, so loss, logits and every gradient agree bit
    for bit; the same step twice gives equal gradients; the eval-mode step and autograd through the eval forward fill a finite,
    non-zero input gradient."""
    a, b, S = _pair(net, dev, lam=LAM, T=TEMP)
    if net == "efficientnet":                                      # the Dropout mask in front of the classifier becomes m
        for m_ in (a, b):
            m_.head[5].p = 0.2
    B, n = 4, 5
    x, t = synth.xray_batch(2500, B, S).to(dev), synth.targets(2510, B, n).to(dev)
    loss_a, logits_a = a.forward_backward(x, t)
    from chexpert_amd.loss import MaskedBCE
    out = b(x)
    loss_b = MaskedBCE()(out, t)
    loss_b.backward()
    assert torch.equal(logits_a, out.detach()) and torch.equal(loss_a.reshape(()), loss_b.detach())
    ga, gb = dict(a.named_parameters()), dict(b.named_parameters())
    assert list(ga) == list(gb)
    for k in ga:
        assert torch.equal(ga[k].grad, gb[k].grad), k
    fc = [m_ for m_ in a.modules() if isinstance(m_, torch.nn.Linear)][-1]
    assert float(fc.weight.grad.abs().max()) > 0 and float(fc.bias.grad.abs().max()) > 0
    if net != "efficientnet":                                      # (its masks are drawn per step)
        first = a._eng().flat_grad.clone()
        a.zero_grad()
        a.forward_backward(x, t)
        assert torch.equal(a._eng().flat_grad, first), "two runs of the same step differ"
    a.zero_grad(set_to_none=True)
    a.eval()
    buf = torch.full((B, 3, S, S), 7.0, device=dev)
    loss_e, _ = a.forward_backward(x, t, input_grad=buf)
    assert math.isfinite(loss_e.item()) and bool(torch.isfinite(buf).all()) and float(buf.abs().max()) > 0 and not bool((buf == 7.0).any())
    xg = x.clone().requires_grad_(True)                             # ... and autograd through the eval forward (saliency.py's route)
    b.eval()
    b(xg)[:, 0].sum().backward()
    assert bool(torch.isfinite(xg.grad).all()) and float(xg.grad.abs().max()) > 0


def test_linear_is_untouched_and_refusals(dev):
    """set_head("linear") against a model that never called it: bit-identical loss, logits, gradients and state_dict keys.  The pool
    must be the average, both ways; set_head after the first forward is refused; class_cam and Grad-CAM refuse a csra model."""
    from chexpert_amd import gradcam
    plain, _, S, _ = _family("densenet", dev, storage="bf16")
    called = _family("densenet", dev, storage="bf16")[0].set_head("linear")
    x, t = synth.xray_batch(2600, 4, S).to(dev), synth.targets(2610, 4, 5).to(dev)
    la, oa = plain.train().forward_backward(x, t)
    lb, ob = called.train().forward_backward(x, t)
    assert torch.equal(la, lb) and torch.equal(oa, ob)
    assert list(plain.state_dict().keys()) == list(called.state_dict().keys())
    for (k, q), (_, w) in zip(plain.named_parameters(), called.named_parameters()):
        assert torch.equal(q.grad, w.grad), k
    with pytest.raises(RuntimeError, match="before the engine has bound"):
        called.set_head("csra")
    assert called.head_kind == "linear"
    csra = _family("densenet", dev)[0].set_head("csra")
    assert list(csra.state_dict().keys()) == list(plain.state_dict().keys())
    with pytest.raises(ValueError, match="set_head"):
        csra.set_pool("lse")
    with pytest.raises(ValueError, match="average pool"):
        _family("densenet", dev)[0].set_pool("gem").set_head("csra")
    with pytest.raises(NotImplementedError, match="set_head"):
        gradcam.class_cam(csra, x)
    with pytest.raises(NotImplementedError, match="set_head"):
        gradcam.grad_cam(csra, x)
    csra.eval()
    with torch.no_grad():
        assert bool(torch.isfinite(csra(x)).all())
    with pytest.raises(RuntimeError, match="before the engine has bound"):
        csra.set_head("linear")


@pytest.mark.parametrize("net", ["densenet", "efficientnet"])
def test_class_maps(dev, net):
    model, _, S, _ = _family(net, dev, n_cls=42 if net == "densenet" else 5)          # (42: the 3n-wide multiclass head)
    model.set_head("csra", lam=LAM, T=TEMP).eval()
    n = 42 if net == "densenet" else 5
    x = synth.xray_batch(2700, 3, S).to(dev)
    with torch.no_grad():
        want = model(x)
    scores, attn, logits = H.class_maps(model, x)
    h = S // 32
    assert scores.shape == attn.shape == (3, n, h, h) and logits.shape == (3, n)
    assert torch.equal(logits, want)
    assert float((attn.sum((2, 3)) - 1).abs().max()) < 1e-5 and float(attn.min()) >= 0
    fc = [m_ for m_ in model.modules() if isinstance(m_, torch.nn.Linear)][-1]
    again = fc.bias + scores.mean((2, 3)) + LAM * (attn * scores).sum((2, 3))
    assert _rel(again, want) < 1e-5
    model.train()
    with pytest.raises(RuntimeError, match="eval mode"):
        H.class_maps(model, x)


def test_graphed_step_equals_eager_and_sees_lambda(dev):
    """A graph replay equals the eager step bit for bit over three steps with FusedAdam; head_attn[0] changed in place is seen by the
    next replay."""
    from chexpert_amd.graph import GraphedTrainStep
    from chexpert_amd.optim import FusedAdam
    m_e, m_g, S = _pair("densenet", dev, lam=LAM, T=TEMP)
    B, n = 4, 5
    xs = [synth.xray_batch(2800 + i, B, S).to(dev) for i in range(4)]
    ts = [synth.targets(2810 + i, B, n).to(dev) for i in range(4)]
    opt_e, opt_g = FusedAdam(m_e, lr=1e-2), FusedAdam(m_g, lr=1e-2)
    gs = GraphedTrainStep(m_g, opt_g, xs[0], ts[0])
    flat = lambda m: torch.cat([q.detach().flatten() for q in m.parameters()])                               # noqa: E731
    w0 = m_e.classifier.weight.detach().clone()
    for i in range(3):
        le = _eager_dev_step(m_e, opt_e, xs[i], ts[i])
        lg, _ = gs.replay(xs[i], ts[i])
        assert torch.equal(le, lg), (i, le.item(), lg.item())
        assert torch.equal(flat(m_e), flat(m_g)), i
        assert torch.equal(m_e._eng().flat_grad, m_g._eng().flat_grad)
    assert not torch.equal(m_e.classifier.weight.detach(), w0)
    held = m_g.head_attn.data_ptr()
    m_g.head_attn[0] = 0.9
    m_e.head_attn[0] = 0.9
    le = _eager_dev_step(m_e, opt_e, xs[3], ts[3])
    lg, _ = gs.replay(xs[3], ts[3])
    assert m_g.head_attn.data_ptr() == held and torch.equal(le, lg) and torch.equal(flat(m_e), flat(m_g))
    m_e.head_attn[0] = LAM                                          # ... and it matters: the first lambda gives other logits
    m_e.eval()
    m_g.eval()
    with torch.no_grad():
        assert not torch.equal(m_e(xs[3]), m_g(xs[3]))


# ------------------------------------------------------------------------------------------------ data parallel
_DP_WORKER = r"""
import os, sys, torch, torch.distributed as dist
sys.path.insert(0, %(root)r)
rank, world = int(os.environ["RANK"]), int(os.environ["WORLD_SIZE"])
dist.init_process_group("gloo")
from chexpert_amd.models import DenseNet
from chexpert_amd.parallel import broadcast_module_state
dev = torch.device("cuda:0")
job = torch.load(os.path.join(%(dir)r, "job.pt"))
model = DenseNet(32, (2, 2, 2, 2), 64, num_classes=5)
model.load_state_dict(job["sd"], strict=True)
model = model.to(dev).set_head("csra", lam=job["lam"], T=job["T"]).eval()          # frozen BatchNorm: the shards see the joint batch's network
broadcast_module_state(model)
x, t = job["x"][4 * rank:4 * rank + 4].to(dev), job["t"][4 * rank:4 * rank + 4].to(dev)
model.forward_backward(x, t)                          # binds the engine; no reducer yet
local = model.classifier.weight.grad.detach().cpu().clone()
model._eng().enable_data_parallel(bucket_bytes=1 << 16)
model.zero_grad()
model.forward_backward(x, t)
torch.cuda.synchronize()
torch.save({"w": model.classifier.weight.grad.detach().cpu().clone(), "b": model.classifier.bias.grad.detach().cpu().clone(), "local": local},
           os.path.join(%(dir)r, "rank%%d.pt" %% rank))
dist.destroy_process_group()
"""


def test_data_parallel_classifier_gradient_two_ranks(dev, tmp_path):
    """Two ranks under torch.distributed.run (sharing the device over gloo), eval mode: the classifier's gradient after the data-parallel
    step is the single-process gradient of the joint batch, within the bound of tests/test_dp_gpu.py (cos > 0.999999, rel < 1e-6)."""
    model, sd, S, _ = _family("densenet", dev, storage="bf16")
    model.set_head("csra", lam=LAM, T=TEMP).eval()
    x, t = synth.xray_batch(3100, 8, S), synth.targets(3200, 8, 5)
    model.forward_backward(x.to(dev), t.to(dev))
    want_w, want_b = model.classifier.weight.grad.cpu().double(), model.classifier.bias.grad.cpu().double()
    torch.save({"sd": sd, "x": x, "t": t, "lam": LAM, "T": TEMP}, str(tmp_path / "job.pt"))
    script = tmp_path / "dp_worker.py"
    script.write_text(_DP_WORKER % {"root": ROOT, "dir": str(tmp_path)})
    port = 37300 + (os.getpid() % 400)
    r = subprocess.run([sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node=2", "--master-addr", "127.0.0.1",
                        "--master-port", str(port), str(script)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    recs = [torch.load(str(tmp_path / ("rank%d.pt" % k))) for k in range(2)]
    assert not torch.equal(recs[0]["local"], recs[1]["local"])
    assert torch.equal(recs[0]["w"], recs[1]["w"]) and torch.equal(recs[0]["b"], recs[1]["b"])
    for got, want in ((recs[0]["w"].double(), want_w), (recs[0]["b"].double(), want_b)):
        cos = float((got * want).sum() / (got.norm() * want.norm()))
        rel = float((got - want).norm() / want.norm())
        print("CSRA two ranks: cos %.7f rel %.3e" % (cos, rel))
        assert cos > 0.999999 and rel < 1e-6


# ------------------------------------------------------------------------------------------------ command line
_CLI = ["--train", "--synthetic", "32", "--batch_size", "4", "--resize", "64", "--eval_interval", "8", "--log_interval", "1", "--seed", "3",
        "--lr", "0.001", "--fused_optimizer", "--graph"]


def test_cli_checkpoint_round_trip_contradiction_and_finetuning(dev, tmp_path, capsys):
    """A linear-head run's checkpoint is restored into --head csra (the fine-tuning case) under --fused_optimizer --graph; the csra
    checkpoint stores head_state; --restore without the flag reads the head from it; --head linear is refused; --visualize --cam_classes
    writes the score and attention maps."""
    from chexpert_amd import cli
    lin = str(tmp_path / "lin")
    cli.main(_CLI + ["--output_dir", lin])
    capsys.readouterr()
    ck_lin = os.path.join(lin, "checkpoint_latest.pt")
    assert "head_state" not in torch.load(ck_lin, map_location="cpu")
    out = str(tmp_path / "c")
    model = cli.main(_CLI + ["--head", "csra", "--csra_lambda", "0.3", "--csra_T", "2", "--restore", ck_lin, "--output_dir", out])
    lines = [json.loads(l)["train_loss"] for l in capsys.readouterr().out.splitlines() if l.startswith('{"step"')]
    assert len(lines) == 8 and all(math.isfinite(v) for v in lines), lines
    assert model.head_kind == "csra" and model.head_attn.tolist() == [pytest.approx(0.3), 2.0]
    ck = os.path.join(out, "checkpoint_latest.pt")
    saved = torch.load(ck, map_location="cpu")
    assert saved["head_state"] == {"kind": "csra", "lam": pytest.approx(0.3), "T": 2.0} and saved["global_step"] == 16
    assert list(saved["state_dict"].keys()) == list(torch.load(ck_lin, map_location="cpu")["state_dict"].keys())
    ev = str(tmp_path / "e")
    model2 = cli.main(["--evaluate_single_model", "--synthetic", "32", "--batch_size", "4", "--resize", "64", "--restore", ck, "--output_dir", ev])
    capsys.readouterr()
    assert model2.head_kind == "csra" and model2.head_attn.tolist() == [pytest.approx(0.3), 2.0]
    with pytest.raises(ValueError, match="--head linear contradicts the checkpoint"):
        cli.main(_CLI + ["--head", "linear", "--restore", ck, "--output_dir", str(tmp_path / "x")])
    vdir = str(tmp_path / "v")
    cli.main(["--visualize", "--cam_classes", "0", "2", "--synthetic", "32", "--batch_size", "4", "--resize", "64", "--restore", ck,
              "--output_dir", vdir])
    capsys.readouterr()
    maps = np.load(os.path.join(vdir, "vis", "csra_maps_lowres.npy"))
    assert maps.ndim == 5 and maps.shape[1:] == (2, 2, 2, 2) and np.isfinite(maps).all()
    np.testing.assert_allclose(maps[:, 1].sum((2, 3)), 1.0, atol=1e-5)
    with pytest.raises(ValueError, match="--cam_classes"):             # Grad-CAM alone reads pool + classifier
        cli.main(["--visualize", "--synthetic", "32", "--batch_size", "4", "--resize", "64", "--restore", ck, "--output_dir", str(tmp_path / "w")])
