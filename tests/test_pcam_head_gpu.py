"""GPU: the probabilistic-CAM pooling head (chexpert_amd/csrc/csra_head.hip: cx_pcam_*; FusedNet.set_head("pcam")).

Kernel level: cx_pcam_head_fwd / cx_pcam_head_bwd and their _f32 twins against chexpert_amd.heads' float64 statements (which
tests/test_pcam_head_cpu.py holds against torch autograd), computed from the inputs as stored.  The inputs are built as
tests/test_csra_head_gpu.py builds its own: sign-safe (every x*sc + sh is at least 1e-2 from 0, asserted), NaN in the pitch padding, a
dead channel (z < 0 everywhere) and -- in the `huge` cases -- one z = 1e4, beside which everything must stay finite and within the
same bounds.

Bounds (the project's for the csra and pooling kernels, tests/test_csra_head_gpu.py and tests/test_pool_head_gpu.py): logits, s, S1, S2,
dW and db within 1e-4 of the largest reference magnitude; g element-wise within eps |ref| + 1e-5 max|ref|, eps = 2^-8 (bf16) / 2^-24
(fp32).  Measured maxima: DESIGN.md section 4.46.

Model level: the comparisons with the oracle (a torch PCAM applied to the tap) run in fp32 storage; the bit-for-bit comparisons in bf16
storage, the mode whose weight gradients are reproducible."""
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
SHAPES = [  # (B, HW, C, ldx, n), activation, m given, bias given
    ((1, 1, 8, 8, 1), "relu", False, True),                      # one pixel: logit = b + s
    ((3, 25, 128, 192, 5), "relu", False, True),                 # pitched, NaN in the padding
    ((17, 4, 264, 264, 14), "relu", False, True),                # ragged C; more images than a wave's worth of pixels
    ((2, 65, 16, 16, 17), "relu", False, True),                  # one pixel more than a wave's stride; n in the 32-wide tile
    ((2, 100, 1040, 1048, 42), "relu", False, True),             # n in the 64-wide tile; two 512-channel chunks and a 16-channel tail
    ((2, 144, 64, 64, 5), "swish", True, True),                  # Swish with the mask m
    ((3, 25, 128, 192, 5), "relu", False, False),                # bias = NULL
]
CASES = [pytest.param(s, a, m, b, id="B%d_HW%d_C%d_ld%d_n%d_%s%s%s" % (s + (a, "_m" if m else "", "" if b else "_nobias")))
         for s, a, m, b in SHAPES]
DEAD, HUGE = 3, 6                 # the channels of the plants
R_CASE = (3, 25, 128, 192, 5)     # the case whose r must be far from 0: csra's db = sum dlogit would miss the bound


def make_inputs(shape, dt, huge, with_m, with_b, dev):
    """The operands of one case, on the host (fp32 as stored; the reference reads these) and on the device."""
    B, HW, C, ldx, n = shape

    def plant(z):
        z[:, :, DEAD] = -z[:, :, DEAD].abs()
        if huge:
            z[B - 1, HW // 2, HUGE] = 1e4
    x, sc, sh, zz = sign_safe(401, (B, HW, C), dt, plant)
    h = {"x": x, "sc": sc, "sh": sh, "W": mag(403, (n, C), 0.02, 0.2), "b": rnd(404, (n,)) if with_b else None,
         "dl": mag(405, (B, n), 0.25, 1.0), "mu": rnd(407, (C,), -0.5, 0.5), "r": rnd(408, (C,), 0.5, 2.0), "es": mag(409, (C,), 0.5, 1.5),
         "m": (rnd(410, (B, C), 0.0, 1.0) > 0.2).float() / 0.8 if with_m else None}
    d = {k: (None if v is None else v.to(dev)) for k, v in h.items() if k != "x"}
    d["x"] = pitched(x.view(-1, C), ldx, dev, dt)
    return h, d, zz


def references(h, act):
    f = lambda k: None if h[k] is None else h[k].double().numpy()                                        # noqa: E731
    fw = H.pcam_reference(f("x"), f("sc"), f("sh"), f("W"), f("b"), act, f("m"))
    bw = H.pcam_backward_reference(f("dl"), f("x"), f("sc"), f("sh"), f("mu"), f("r"), f("es"), f("W"), f("b"), act, f("m"))
    logits, s, w, _ = fw
    u = s if h["b"] is None else s + f("b")[None, :, None]
    r = (w * np.exp(-np.logaddexp(0.0, u)) * (u - logits[:, :, None])).sum(2)                             # sum_p w sigma(-u) (u - logit)
    return fw, bw, r


def run_kernels(dev, shape, dt, act, huge, with_m, with_b):
    from chexpert_amd._lib import lib, ptr, check, stream_ptr
    B, HW, C, ldx, n = shape
    h, d, zz = make_inputs(shape, dt, huge, with_m, with_b, dev)
    (want_logits, want_s, _, _), (want_g, S1, S2, want_dW, want_db), r = references(h, act)
    print("R %s max|r| %.3f" % (CASE, np.abs(r).max()))
    fwd, bwd = entry("cx_pcam_head_fwd", dt), entry("cx_pcam_head_bwd", dt)
    # forward
    logits, s, stat = full(dev, (B, n)), full(dev, (B, n, HW)), full(dev, (B, n, 4))
    check(fwd(ptr(d["x"]), ptr(d["sc"]), ptr(d["sh"]), ptr(d["m"]), ptr(d["W"]), ptr(d["b"]), ptr(logits), ptr(s), ptr(stat), B, HW, C, ldx, n,
              ACT[act], stream_ptr()), "cx_pcam_head_fwd")
    close(logits, want_logits, "logits")
    close(s, want_s, "s")
    if HW == 1:                                                     # one pixel: its weight is 1
        close(logits, (0.0 if h["b"] is None else h["b"].double().numpy()) + want_s[:, :, 0], "logits = b + s at HW = 1")
    # the score map is csra's, bit for bit
    lt = torch.tensor([0.3, 2.0], device=dev)
    logits_c, s_c, stat_c = full(dev, (B, n)), full(dev, (B, n, HW)), full(dev, (B, n, 4))
    check(entry("cx_csra_head_fwd", dt)(ptr(d["x"]), ptr(d["sc"]), ptr(d["sh"]), ptr(d["m"]), ptr(d["W"]), ptr(d["b"]), ptr(lt), ptr(logits_c),
                                        ptr(s_c), ptr(stat_c), B, HW, C, ldx, n, ACT[act], stream_ptr()), "cx_csra_head_fwd")
    assert torch.equal(s, s_c), "the score map differs from cx_csra_head_fwd's"
    # backward: atomic sums, pitched g, dW and db added to what they hold
    need = lib().cx_pcam_bwd_scratch(B, HW, C, n)
    assert need == lib().cx_csra_bwd_scratch(B, HW, C, n) + B * n
    ldg = C + 8
    args = (ptr(d["dl"]), ptr(s), ptr(stat), ptr(d["x"]), ptr(d["sc"]), ptr(d["sh"]), ptr(d["m"]), ptr(d["mu"]), ptr(d["r"]), ptr(d["es"]),
            ptr(d["W"]))

    def call(g, s1, s2, dW, db, scratch, rows):
        return bwd(*args, ptr(g), ptr(s1), ptr(s2), ptr(dW), ptr(db), ptr(scratch), scratch.numel(), B, HW, C, ldx, ldg, n, ACT[act], rows,
                   stream_ptr())
    g, st, dW, db, scr = full(dev, (B * HW, ldg), dt), torch.zeros(2, C, device=dev), full(dev, (n, C), v=0.5), full(dev, (n,), v=-0.25), \
        full(dev, (need,), v=NAN)
    check(call(g, st[0], st[1], dW, db, scr, 0), "cx_pcam_head_bwd")
    assert bool((g[:, C:] == SENT).all()), "a write into the pitch padding of g"
    gv = g[:, :C].float().view(B, HW, C)
    close_elem(gv, want_g, dt, "g")
    close(st[0], S1, "S1 atomic")
    close(st[1], S2, "S2 atomic")
    close(dW.double() - 0.5, want_dW, "dW")
    close(db.double() + 0.25, want_db, "db")
    if shape == R_CASE and not huge:                                # the bias gradient is not csra's sum of dlogit
        assert np.abs(r).max() > 0.1
        csra_db = h["dl"].double().sum(0)
        assert (csra_db - torch.as_tensor(want_db)).abs().max().item() / np.abs(want_db).max() > 10 * SUM_TOL
    if act == "relu":                                               # the dead channel: nothing flows
        assert not bool(gv[:, :, DEAD].any()) and float(st[0][DEAD]) == 0.0 and float(st[1][DEAD]) == 0.0
        assert bool((dW[:, DEAD] == 0.5).all())
    # rows mode: exactly B rows, row b = the sums of image b; two calls give equal bits in every output
    outs = []
    for _ in range(2):
        g2, rows, dW2, db2 = full(dev, (B * HW, ldg), dt), full(dev, (2, B + 3, C)), full(dev, (n, C), v=0.5), full(dev, (n,), v=-0.25)
        check(call(g2, rows[0], rows[1], dW2, db2, full(dev, (need + 5,), v=NAN), B + 3), "cx_pcam_head_bwd")
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
    # a scratch that is too small (csra's length among them) is refused with nothing written
    for short in (need - 1, need - B * n):
        g2, dW2, db2, scr2 = full(dev, (B * HW, ldg), dt), full(dev, (n, C)), full(dev, (n,)), full(dev, (short,))
        assert call(g2, st[0], st[1], dW2, db2, scr2, 0) == CX_EUNSUPPORTED
        assert all(bool((t == SENT).all()) for t in (g2, dW2, db2, scr2))


@pytest.mark.parametrize("huge", [False, True], ids=["plain", "huge"])
@pytest.mark.parametrize("dt", STORAGE)
@pytest.mark.parametrize("shape,act,with_m,with_b", CASES)
def test_pcam_kernels(dev, shape, act, with_m, with_b, dt, huge):
    """Forward (and its score map against csra's) and backward (atomic sums with a pitched g; rows mode twice; below B rows; a short
    scratch)."""
    run_kernels(dev, shape, dt, act, huge, with_m, with_b)


@pytest.mark.parametrize("dt", STORAGE)
def test_more_than_64_classes_are_unsupported(dev, dt):
    from chexpert_amd._lib import ptr, stream_ptr
    B, HW, C, n = 2, 4, 16, 65
    f = lambda *s: full(dev, s)                                                                          # noqa: E731
    x, g = full(dev, (B * HW, C), dt), full(dev, (B * HW, C), dt)
    v, W = f(C), f(n, C)
    logits, s, stat, dl, dW, db, scr = f(B, n), f(B, n, HW), f(B, n, 4), f(B, n), f(n, C), f(n), f(1 << 16)
    assert entry("cx_pcam_head_fwd", dt)(ptr(x), ptr(v), ptr(v), None, ptr(W), ptr(v), ptr(logits), ptr(s), ptr(stat), B, HW, C, C, n, 1,
                                         stream_ptr()) == CX_EUNSUPPORTED
    assert entry("cx_pcam_head_bwd", dt)(ptr(dl), ptr(s), ptr(stat), ptr(x), ptr(v), ptr(v), None, ptr(v), ptr(v), ptr(v), ptr(W), ptr(g), ptr(v),
                                         ptr(v), ptr(dW), ptr(db), ptr(scr), scr.numel(), B, HW, C, C, C, n, 1, 0,
                                         stream_ptr()) == CX_EUNSUPPORTED
    torch.cuda.synchronize()
    assert all(bool((t == SENT).all()) for t in (logits, s, stat, g, dW, db, scr))


# ------------------------------------------------------------------------------------------------ 2. models
def _rel(a, b):
    return (a.double() - b.double()).abs().max().item() / (b.double().abs().max().item() + 1e-12)


def torch_pcam(a, W, b):
    """The torch PCAM of an NCHW activation: the oracle's side (the plain quotient of the paper's code)."""
    u = torch.einsum("kc,bchw->bkhw", W, a).flatten(2) + b[None, :, None]
    P = torch.sigmoid(u)
    return ((P / P.sum(2, keepdim=True)) * u).sum(2)


def _family(net, dev, n_cls=5, seed=21, storage="fp32", head_scale=1.0):
    """(fused model in `storage` with the state dict loaded, state dict, input size, oracle forward(sd, x) with the torch PCAM applied
    to the tap in front of the average).  head_scale multiplies the classifier's weight (these networks' scores reach 1e2 to 5e3)."""
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
    sd[fc + ".weight"] = sd[fc + ".weight"] * head_scale
    model.storage_dtype(storage).load_state_dict(sd, strict=True)

    def forward(s, xx):
        taps = {}
        body(s, xx, taps)
        return torch_pcam(act(taps[tap]), s[fc + ".weight"], s[fc + ".bias"])
    return model.to(dev), sd, S, forward


@pytest.mark.parametrize("net", ["densenet", "resnet", "efficientnet"])
def test_one_training_step_against_the_oracle(dev, net):
    """Bounds of tests/test_fp32_gpu.py: logits within 1e-3 of the logit scale, loss within 1e-4 relative, every conv or linear gradient
    at cos >= 0.9999 and a norm ratio within 1e-3."""
    from oracle import step
    model, sd, S, forward = _family(net, dev)
    model.set_head("pcam")
    B, n_cls = 4, 5
    x, t = synth.xray_batch(1234, B, S), synth.targets(99, B, n_cls)
    loss_o, logits_o, grads_o = step.train_step(forward, {k: v.clone() for k, v in sd.items()}, x, t)
    model.train()
    loss, logits = model.forward_backward(x.to(dev), t.to(dev))
    e = _rel(logits.cpu(), logits_o)
    print("PCAM %s: train logits rel %.3e, loss %.6f (oracle %.6f)" % (net, e, loss.item(), loss_o.item()))
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
    print("PCAM %s: worst cos %.7f (%s), worst norm ratio - 1 %.3e (%s), %d tensors" % (net, worst[0][0], worst[0][2], ratio[1], ratio[2],
                                                                                       len(worst)))
    assert any(q.dim() == 2 for q in model.parameters())
    assert worst[0][0] >= 0.9999 and ratio[1] <= 1e-3, (worst[:3], ratio)
    fcb = [k for k, q in model.named_parameters() if q.dim() == 1 and k.endswith(("classifier.bias", "fc.bias", "head.6.bias"))]
    assert len(fcb) == 1                                            # the bias gradient, the term that differs from csra
    a, b = dict(model.named_parameters())[fcb[0]].grad.cpu().double(), grads_o[fcb[0]].double()
    print("PCAM %s: bias gradient rel %.3e" % (net, _rel(a, b)))
    assert _rel(a, b) < 1e-3


def _pair(net, dev):
    a, sd, S, _ = _family(net, dev, storage="bf16")
    b = _family(net, dev, storage="bf16")[0]
    a.set_head("pcam")
    b.set_head("pcam")
    return a.train(), b.train(), S


@pytest.mark.parametrize("net", ["densenet", "resnet", "efficientnet"])
def test_fused_step_equals_the_autograd_route_and_repeats(dev, net):
    """forward_backward against model(x) + the BCE + loss.backward(): the same kernels, so loss, logits and every gradient agree bit
    for bit; the same step twice gives equal gradients; the eval-mode step and autograd through the eval forward fill a finite,
    non-zero input gradient."""
    a, b, S = _pair(net, dev)
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
    must be the average, both ways; set_head after the first forward is refused; class_cam and Grad-CAM refuse a pcam model."""
    from chexpert_amd import gradcam
    plain, _, S, _ = _family("densenet", dev, storage="bf16")
    called = _family("densenet", dev, storage="bf16")[0].set_head("pcam").set_head("linear")
    x, t = synth.xray_batch(2600, 4, S).to(dev), synth.targets(2610, 4, 5).to(dev)
    la, oa = plain.train().forward_backward(x, t)
    lb, ob = called.train().forward_backward(x, t)
    assert torch.equal(la, lb) and torch.equal(oa, ob)
    assert list(plain.state_dict().keys()) == list(called.state_dict().keys())
    for (k, q), (_, w) in zip(plain.named_parameters(), called.named_parameters()):
        assert torch.equal(q.grad, w.grad), k
    with pytest.raises(RuntimeError, match="before the engine has bound"):
        called.set_head("pcam")
    assert called.head_kind == "linear"
    pcam = _family("densenet", dev)[0].set_head("pcam")
    assert list(pcam.state_dict().keys()) == list(plain.state_dict().keys())
    assert [k for k, _ in pcam.named_buffers()] == [k for k, _ in plain.named_buffers()]
    with pytest.raises(ValueError, match="set_head"):
        pcam.set_pool("lse")
    with pytest.raises(ValueError, match="average pool"):
        _family("densenet", dev)[0].set_pool("gem").set_head("pcam")
    with pytest.raises(NotImplementedError, match="set_head"):
        gradcam.class_cam(pcam, x)
    with pytest.raises(NotImplementedError, match="set_head"):
        gradcam.grad_cam(pcam, x)
    pcam.eval()
    with torch.no_grad():
        out = pcam(x)
    assert bool(torch.isfinite(out).all()) and not torch.equal(out, oa)
    with pytest.raises(RuntimeError, match="before the engine has bound"):
        pcam.set_head("linear")


@pytest.mark.parametrize("net", ["densenet", "efficientnet"])
def test_class_maps(dev, net):
    """The classifier's weight is scaled so that the scores stay within a few units, which is asserted as a condition of the test
    (1e-3 < P < 0.98): an fp32 P = sigmoid(u) is 1 from u = 17 on, and logit(P) returns P's rounding 2^-24 times 1 / (1 - P), at most
    3e-6 here.  (The other model tests run the scores as they are, up to 5e3.)"""
    model, _, S, _ = _family(net, dev, n_cls=42 if net == "densenet" else 5, head_scale=1 / 40 if net == "densenet" else 1 / 1500)
    model.set_head("pcam").eval()
    n = 42 if net == "densenet" else 5
    x = synth.xray_batch(2700, 3, S).to(dev)
    with torch.no_grad():
        want = model(x)
    P, w, logits = H.class_maps(model, x)
    h = S // 32
    assert P.shape == w.shape == (3, n, h, h) and logits.shape == (3, n)
    assert torch.equal(logits, want)
    assert float(P.min()) >= 0.0 and float(P.max()) <= 1.0
    assert float((w.sum((2, 3)) - 1).abs().max()) < 1e-5 and float(w.min()) >= 0
    print("PCAM %s class_maps: P in [%.4f, %.4f]" % (net, float(P.min()), float(P.max())))
    assert 1e-3 < float(P.min()) and float(P.max()) < 0.98 and float(P.max() - P.min()) > 0.2
    again = (w * torch.logit(P.double())).sum((2, 3))
    print("PCAM %s class_maps: sum w logit(P) against the logits, rel %.3e" % (net, _rel(again, want)))
    assert _rel(again, want) < 1e-5
    model.train()
    with pytest.raises(RuntimeError, match="eval mode"):
        H.class_maps(model, x)


def test_graphed_step_equals_eager(dev):
    """A graph replay equals the eager step bit for bit over three steps with FusedAdam."""
    from chexpert_amd.graph import GraphedTrainStep
    from chexpert_amd.optim import FusedAdam
    m_e, m_g, S = _pair("densenet", dev)
    B, n = 4, 5
    xs = [synth.xray_batch(2800 + i, B, S).to(dev) for i in range(3)]
    ts = [synth.targets(2810 + i, B, n).to(dev) for i in range(3)]
    opt_e, opt_g = FusedAdam(m_e, lr=1e-2), FusedAdam(m_g, lr=1e-2)
    gs = GraphedTrainStep(m_g, opt_g, xs[0], ts[0])
    flat = lambda m: torch.cat([q.detach().flatten() for q in m.parameters()])                               # noqa: E731
    w0, b0 = m_e.classifier.weight.detach().clone(), m_e.classifier.bias.detach().clone()
    for i in range(3):
        le = _eager_dev_step(m_e, opt_e, xs[i], ts[i])
        lg, _ = gs.replay(xs[i], ts[i])
        assert torch.equal(le, lg), (i, le.item(), lg.item())
        assert torch.equal(flat(m_e), flat(m_g)), i
        assert torch.equal(m_e._eng().flat_grad, m_g._eng().flat_grad)
    assert not torch.equal(m_e.classifier.weight.detach(), w0) and not torch.equal(m_e.classifier.bias.detach(), b0)


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
model = model.to(dev).set_head("pcam").eval()          # frozen BatchNorm: the shards see the joint batch's network
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
    step -- the weight's and the bias's, the term that differs from csra -- is the single-process gradient of the joint batch, within
    the bound of tests/test_dp_gpu.py (cos > 0.999999, rel < 1e-6)."""
    model, sd, S, _ = _family("densenet", dev, storage="bf16")
    model.set_head("pcam").eval()
    x, t = synth.xray_batch(3100, 8, S), synth.targets(3200, 8, 5)
    model.forward_backward(x.to(dev), t.to(dev))
    want_w, want_b = model.classifier.weight.grad.cpu().double(), model.classifier.bias.grad.cpu().double()
    torch.save({"sd": sd, "x": x, "t": t}, str(tmp_path / "job.pt"))
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
        print("PCAM two ranks: cos %.7f rel %.3e" % (cos, rel))
        assert cos > 0.999999 and rel < 1e-6


# ------------------------------------------------------------------------------------------------ command line
_CLI = ["--train", "--synthetic", "8", "--batch_size", "4", "--resize", "64", "--eval_interval", "2", "--log_interval", "1", "--seed", "3",
        "--lr", "0.001", "--fused_optimizer", "--num_workers", "0"]         # two steps; the graphed step has its own test above


def test_cli_checkpoint_round_trip_contradictions_and_visualize(dev, tmp_path, capsys):
    """--head pcam trains and its checkpoint stores head_state; --restore without the flag reads the head from it; --head linear and
    --head csra on it are refused; a linear-head checkpoint restores into --head pcam with one line saying that the function changes;
    --visualize --cam_classes writes the probability and weight maps and one overlay per image."""
    from chexpert_amd import cli
    out = str(tmp_path / "p")
    model = cli.main(_CLI + ["--head", "pcam", "--output_dir", out])
    lines = [json.loads(l)["train_loss"] for l in capsys.readouterr().out.splitlines() if l.startswith('{"step"')]
    assert len(lines) == 2 and all(math.isfinite(v) for v in lines), lines
    assert model.head_kind == "pcam" and not hasattr(model, "head_attn")
    ck = os.path.join(out, "checkpoint_latest.pt")
    saved = torch.load(ck, map_location="cpu")
    assert saved["head_state"] == {"kind": "pcam", "lam": None, "T": None} and saved["global_step"] == 2
    for kind in ("linear", "csra"):
        with pytest.raises(ValueError, match="--head %s contradicts the checkpoint" % kind):
            cli.main(_CLI + ["--head", kind, "--restore", ck, "--output_dir", str(tmp_path / "x")])
    # a linear-head checkpoint with the same keys restores into --head pcam
    lin = str(tmp_path / "lin.pt")
    torch.save({k: v for k, v in saved.items() if k != "head_state"}, lin)
    model3 = cli.main(["--evaluate_single_model", "--synthetic", "32", "--batch_size", "4", "--resize", "64", "--head", "pcam", "--restore", lin,
                       "--num_workers", "0", "--output_dir", str(tmp_path / "f")])
    assert model3.head_kind == "pcam" and "function" in capsys.readouterr().out
    assert list(model3.state_dict().keys()) == list(saved["state_dict"].keys())
    vdir = str(tmp_path / "v")
    model2 = cli.main(["--visualize", "--cam_classes", "0", "2", "--synthetic", "32", "--batch_size", "4", "--resize", "64", "--restore", ck,
                       "--num_workers", "0", "--output_dir", vdir])  # no --head: the checkpoint's
    capsys.readouterr()
    assert model2.head_kind == "pcam"
    maps = np.load(os.path.join(vdir, "vis", "pcam_maps_lowres.npy"))
    assert maps.ndim == 5 and maps.shape[1:] == (2, 2, 2, 2) and np.isfinite(maps).all()
    assert maps[:, 0].min() >= 0.0 and maps[:, 0].max() <= 1.0
    np.testing.assert_allclose(maps[:, 1].sum((2, 3)), 1.0, atol=1e-5)
    pngs = [f for f in os.listdir(os.path.join(vdir, "vis")) if f.startswith("pcam_") and f.endswith(".png")]
    assert len(pngs) == maps.shape[0] and all("_step_%d.png" % saved["global_step"] in f for f in pngs)
    assert not os.path.exists(os.path.join(vdir, "vis", "csra_maps_lowres.npy"))
    with pytest.raises(ValueError, match="--cam_classes"):             # Grad-CAM alone reads pool + classifier
        cli.main(["--visualize", "--synthetic", "32", "--batch_size", "4", "--resize", "64", "--restore", ck, "--output_dir", str(tmp_path / "w")])
