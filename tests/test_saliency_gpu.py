"""GPU: pixel attribution maps (chexpert_amd/saliency.py, csrc/saliency.hip).  Kernel level: cx_sal_points / cx_sal_accumulate /
cx_sal_finish against their numpy statements, bit for bit (the noise term to a few ulp of its logf / sqrtf / cospif).  Network level:
input_gradient, smoothgrad and integrated_gradients on the three fused families against the eval autograd path they are built on
(bit-equal), against the CPU oracle (torch autograd through oracle/nets.py with train=False), the completeness identity, the
contracts of the call (no state moves, no parameter gradient appears or changes) and the --visualize wiring."""
import os

import numpy as np
import pytest
import torch

from chexpert_amd import saliency as S
from chexpert_amd import synth

pytestmark = pytest.mark.gpu

SHAPES = [(8, 8), (7, 9), (1, 5)]          # a row of 3 H W floats: a multiple of four (float4 lanes), odd, shorter than a wave
IMG = [1, 0, 1, 1, 0]                      # R = 5 rows over B = 2 images, out of order
ALPHA = [0.0, 1.0, 0.34375, 1.0 / 3.0, 0.34375]


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    from chexpert_amd import _lib
    _lib.lib()
    return torch.device("cuda:0")


def _rand(seed, *shape):
    return torch.randn(*shape, generator=torch.Generator().manual_seed(seed), dtype=torch.float32)


def _t(a, dev, dtype):
    return torch.tensor(a, dtype=dtype, device=dev)


def _bits(t):
    return t.contiguous().view(torch.int32)


# ------------------------------------------------------------------------------------------------------------ cx_sal_points
@pytest.mark.parametrize("base", ["zero", "const", "full"])
@pytest.mark.parametrize("H,W", SHAPES + [(20, 24)])                   # (20, 24): more than one workgroup per row
def test_points_without_noise_equal_the_statement(dev, H, W, base):
    from chexpert_amd import ops
    x = _rand(1, 2, 3, H, W)
    b = {"zero": (0.0, 0.0, 0.0), "const": (0.25, -15.272206, 1.0 / 3.0), "full": _rand(2, 2, 3, H, W)}[base]
    got = ops.sal_points(x.to(dev), b.to(dev) if base == "full" else b, _t(IMG, dev, torch.int32), _t(ALPHA, dev, torch.float32))
    ref = S.points_reference(x.numpy(), b.numpy() if base == "full" else np.float32(b), IMG, np.float32(ALPHA))
    assert got.shape == (5, 3, H, W) and torch.equal(got.cpu(), torch.from_numpy(ref))
    if base == "zero":
        assert torch.equal(got[1].cpu(), x[0])                          # baseline 0, alpha 1: x exactly


@pytest.mark.parametrize("H,W", SHAPES)
def test_points_with_noise(dev, H, W):
    from chexpert_amd import ops
    x, b = _rand(3, 2, 3, H, W), _rand(4, 2, 3, H, W)
    sigma = [0.5, 4.3]
    img, al, sg = _t(IMG, dev, torch.int32), _t(ALPHA, dev, torch.float32), _t(sigma, dev, torch.float32)
    run = lambda lo, hi: ops.sal_points(x.to(dev), b.to(dev), img[lo:hi].contiguous(), al[lo:hi].contiguous(), sigma=sg, seed=11, first_row=lo)
    got = run(0, 5)
    ref = S.points_reference(x.numpy(), b.numpy(), IMG, np.float32(ALPHA), np.float32(sigma), seed=11)
    err = (got.cpu().double() - torch.from_numpy(ref).double()).abs()
    bound = 1e-5 * torch.tensor(sigma, dtype=torch.float64)[IMG].view(5, 1, 1, 1) + 2.0 ** -23 * torch.from_numpy(ref).double().abs()
    print("noise %dx%d: worst error / bound %.3f" % (H, W, float((err / bound).max())))
    assert bool((err <= bound).all())
    plain = ops.sal_points(x.to(dev), b.to(dev), img, al)
    assert float((got - plain).abs().max()) > 0.1                       # the noise is there
    assert torch.equal(_bits(got), _bits(torch.cat([run(0, 2), run(2, 5)])))      # rows cut into two calls
    assert torch.equal(_bits(got), _bits(run(0, 5)))                    # two runs
    other = ops.sal_points(x.to(dev), b.to(dev), img, al, sigma=sg, seed=12)
    assert not torch.equal(got, other)


def test_points_and_accumulate_grid_stride(dev):
    """A row of more than 2048 x 256 float4: the lanes of a workgroup come round a second time."""
    from chexpert_amd import ops
    H, W = 700, 1000
    x = _rand(5, 1, 3, H, W)
    img, al = _t([0, 0], dev, torch.int32), _t([0.34375, 1.0 / 3.0], dev, torch.float32)
    pts = ops.sal_points(x.to(dev), (0.5, 0.25, -1.0), img, al)
    assert torch.equal(pts.cpu(), torch.from_numpy(S.points_reference(x.numpy(), np.float32((0.5, 0.25, -1.0)), [0, 0], al.cpu().numpy())))
    w = [0.3, 1.7]
    acc = ops.sal_accumulate(pts, img, _t(w, dev, torch.float32), torch.empty(1, 3, H, W, device=dev), accumulate=False)
    assert torch.equal(acc.cpu(), torch.from_numpy(S.accumulate_reference(pts.cpu().numpy(), [0, 0], np.float32(w), 1)))


# ------------------------------------------------------------------------------------------------------------ cx_sal_accumulate
@pytest.mark.parametrize("square", [False, True])
@pytest.mark.parametrize("accumulate", [False, True])
@pytest.mark.parametrize("H,W", SHAPES + [(20, 24)])
def test_accumulate_equals_the_statement(dev, H, W, square, accumulate):
    from chexpert_amd import ops
    g, old = _rand(6, 5, 3, H, W), _rand(7, 2, 3, H, W)
    slot, w = [1, 0, 1, 1, 0], np.float32([0.3, 1.0 / 3.0, 0.7, 0.11, 1.7])
    # the inputs tell a fused multiply-add from the two rounded operations: somewhere fl(a + w t) != fl(a + fl(w t))
    r32 = lambda v: v.float().double()                                                    # (products of two fp32 are exact in double)
    t1, t4 = (r32(g[r].double() ** 2) if square else g[r].double() for r in (1, 4))       # plane 0 folds row 1, then row 4
    a1 = r32((old[0].double() if accumulate else torch.zeros_like(t1)) + r32(float(w[1]) * t1))
    fused, unfused = (a1 + float(w[4]) * t4).float(), (a1 + r32(float(w[4]) * t4)).float()
    assert bool((fused != unfused).any()), "the inputs cannot tell a contracted kernel from the statement"
    acc = old.clone().to(dev)
    ops.sal_accumulate(g.to(dev), _t(slot, dev, torch.int32), torch.from_numpy(w).to(dev), acc, square=square, accumulate=accumulate)
    ref = S.accumulate_reference(g.numpy(), slot, w, 2, square=square, acc=old.numpy() if accumulate else None)
    assert torch.equal(acc.cpu(), torch.from_numpy(ref))


def test_accumulate_skips_slots_outside_the_planes(dev):
    from chexpert_amd import ops
    g = _rand(8, 3, 3, 4, 4)
    acc = torch.full((1, 3, 4, 4), 7.0, device=dev)
    ops.sal_accumulate(g.to(dev), _t([5, 0, -1], dev, torch.int32), _t([1.0, 1.0, 1.0], dev, torch.float32), acc, accumulate=False)
    assert torch.equal(acc[0].cpu(), g[1])


# ------------------------------------------------------------------------------------------------------------ cx_sal_finish
@pytest.mark.parametrize("channels", S.CHANNELS)
@pytest.mark.parametrize("times_input", [False, True])
@pytest.mark.parametrize("H,W", SHAPES + [(4, 33000)])                 # 132 000 pixels: more than 128 workgroups x 256 lanes x 4
def test_finish_equals_the_statement(dev, H, W, channels, times_input):
    from chexpert_amd import ops
    P, img_of = 3, [1, 0, 1]
    acc, x, b = _rand(9, P, 3, H, W), _rand(10, 2, 3, H, W), _rand(11, 2, 3, H, W)
    for base in ((0.25, -15.272206, 1.0 / 3.0), b):
        full = isinstance(base, torch.Tensor)
        run = lambda: ops.sal_finish(acc.to(dev), x.to(dev), base.to(dev) if full else base, _t(img_of, dev, torch.int32),
                                     times_input=times_input, channels=channels, total=True)
        out, tot = run()
        ref, rtot = S.finish_reference(acc.numpy(), x.numpy(), base.numpy() if full else np.float32(base), img_of, times_input, channels)
        assert out.shape == ref.shape and torch.equal(out.cpu(), torch.from_numpy(ref))
        a = S.finish_reference(acc.numpy(), x.numpy(), base.numpy() if full else np.float32(base), img_of, times_input, "none")[0]
        mass = np.abs(a.astype(np.float64)).sum(axis=(1, 2, 3))
        print("finish %dx%d %s: total error / (1e-12 sum|a|) %.3g" % (H, W, channels, float((np.abs(tot.cpu().numpy() - rtot) / (1e-12 * mass)).max())))
        assert tot.dtype == torch.float64 and bool((np.abs(tot.cpu().numpy() - rtot) <= 1e-12 * mass).all())
        out2, tot2 = run()
        assert torch.equal(_bits(out), _bits(out2)) and torch.equal(tot.view(torch.int64), tot2.view(torch.int64))
        assert ops.sal_finish(acc.to(dev), x.to(dev), base.to(dev) if full else base, _t(img_of, dev, torch.int32), times_input=times_input,
                              channels=channels)[1] is None


# ------------------------------------------------------------------------------------------------------------ the networks
def _dense(cfg, S_, n_cls):
    from chexpert_amd.models import DenseNet
    from oracle import nets
    spec = nets.densenet_spec(n_cls, growth=32, block_config=cfg, init_features=64, attn=None, input_hw=(S_, S_))
    return spec, DenseNet(32, cfg, 64, num_classes=n_cls), 2.5, lambda s, x, q=None: nets.densenet_forward(s, x, cfg, train=False, nh=None, q=q)


def _resnet(layers, S_, n_cls):
    from chexpert_amd.models import Bottleneck, ResNet
    from oracle import nets
    return (nets.resnet_spec(n_cls, layers=layers, input_hw=(S_, S_)), ResNet(Bottleneck, list(layers), num_classes=n_cls), 1.0,
            lambda s, x, q=None: nets.resnet_forward(s, x, layers, train=False, q=q))


def _effnet(name, n_cls):
    from chexpert_amd.models import construct_model
    from chexpert_amd.models.efficientnet import DropMarker
    from oracle import nets
    model = construct_model(name, n_cls)
    for mod in model.modules():
        if isinstance(mod, DropMarker):
            mod.p = 0.0
    return nets.efficientnet_spec(name, n_cls), model, 1.0, lambda s, x, q=None: nets.efficientnet_forward(s, x, name, train=False)


NETS = {  # tag -> (builder, B, S)
    "densenet2222_64": (lambda n: _dense((2, 2, 2, 2), 64, n), 2, 64),
    "resnet1111_64": (lambda n: _resnet((1, 1, 1, 1), 64, n), 2, 64),
    "efficientnet-b0_224": (lambda n: _effnet("efficientnet-b0", n), 1, 224),
}
TAGS = list(NETS)
CLASSES = [0, 3]


def _calibrate(model, x):
    """Running statistics in the network's operating range (one train-mode forward at momentum 1 on another batch), then a
    per-BatchNorm jitter, as tests/test_eval_autograd_gpu.py does."""
    bns = [m for m in model.modules() if isinstance(m, torch.nn.BatchNorm2d)]
    moms = [m.momentum for m in bns]
    for m in bns:
        m.momentum = 1.0
    model.train()
    with torch.no_grad():
        model(x)
    for m, mom in zip(bns, moms):
        m.momentum = mom
    with torch.no_grad():
        for i, m in enumerate(bns):
            C = m.num_features
            m.running_mean.add_(synth.uniform(100 + i, (C,), -0.05, 0.05).to(m.running_mean.device) * m.running_var.sqrt())
            m.running_var.mul_(synth.uniform(5000 + i, (C,), 0.9, 1.1).to(m.running_var.device))


_made = {}


def _make(tag, dtype, dev, n_cls=5):
    """(model in eval mode, its state dict on the CPU, the oracle's forward, x on the CPU): built once per (tag, storage type) -- no
    test below leaves a trace in the model."""
    if (tag, dtype) not in _made:
        from oracle import nets
        build, B, S_ = NETS[tag]
        spec, model, bias, fwd = build(n_cls)
        sd = synth.smooth_state_dict_(synth.fill_state_dict_(nets.zeros_state_dict(spec), 21), bias)
        model.load_state_dict(sd, strict=True)
        model = model.storage_dtype(dtype).to(dev)
        _calibrate(model, synth.xray_batch(777, B, S_).to(dev))
        model.eval()
        sd = {k: v.detach().cpu().clone() for k, v in model.state_dict().items()}
        _made[(tag, dtype)] = (model, sd, fwd, synth.xray_batch(1234, B, S_))
    model, sd, fwd, x = _made[(tag, dtype)]
    model.eval()
    model.zero_grad(set_to_none=True)
    return model, sd, fwd, x


def _autograd_dx(model, xd, c):
    xg = xd.clone().requires_grad_(True)
    model(xg)[:, c].sum().backward()
    model.zero_grad(set_to_none=True)
    return xg.grad


def _cmp(got, ref):
    a, b = torch.as_tensor(got).double().flatten().cpu(), torch.as_tensor(ref).double().flatten()
    return float((a * b).sum() / (a.norm() * b.norm())), float(a.norm() / b.norm())


@pytest.mark.parametrize("tag", TAGS)
def test_input_gradient_is_the_eval_autograd_gradient(dev, tag):
    model, _, _, x = _make(tag, "bf16", dev)
    xd = x.to(dev)
    got = S.input_gradient(model, xd, CLASSES)
    assert got.shape == (xd.shape[0], 2, 3) + tuple(xd.shape[2:]) and float(got.abs().max()) > 0
    for k, c in enumerate(CLASSES):
        assert torch.equal(got[:, k], _autograd_dx(model, xd, c)), (tag, c)
    assert torch.equal(S.smoothgrad(model, xd, CLASSES, samples=1, sigma=0.0, channels="none"), got)
    assert torch.equal(S.input_gradient(model, xd, [3], channels="abs")[:, 0], (got[:, 1, 0].abs() + got[:, 1, 1].abs()) + got[:, 1, 2].abs())
    # one class per image: a tensor, and the arg-max of the logits
    with torch.no_grad():
        pred = model(xd).argmax(1)
    per = S.input_gradient(model, xd, pred.cpu())
    assert per.shape[1] == 1 and torch.equal(per, S.input_gradient(model, xd, "pred"))
    for b_ in range(xd.shape[0]):
        if int(pred[b_]) in CLASSES:
            assert torch.equal(per[b_, 0], got[b_, CLASSES.index(int(pred[b_]))])


@pytest.mark.parametrize("tag", TAGS)
def test_integrated_gradients_equal_the_hand_composed_loop(dev, tag):
    """steps = 4, chunk = 3: the rows of cx_sal_points through the public eval autograd path chunk by chunk, the numpy accumulate and
    finish statements on the resulting x.grad -- the orchestration holds to the definitions bit for bit."""
    from chexpert_amd import ops
    model, _, _, x = _make(tag, "bf16", dev)
    xd = x.to(dev)
    B, R = xd.shape[0], 3
    base = ((0.0 - 0.5330) / 0.0349,) * 3
    attr, logits, delta = S.integrated_gradients(model, xd, CLASSES, steps=4, baseline="black", channels="sum", chunk=R)
    alphas, weights = S.path_alphas(4)
    img = np.repeat(np.arange(B), 4).astype(np.int32)
    al, w = np.tile(alphas, B).astype(np.float32), np.tile(weights, B).astype(np.float32)
    for k, c in enumerate(CLASSES):
        acc = None
        for r0 in range(0, len(img), R):
            pts = ops.sal_points(xd, base, torch.from_numpy(img[r0:r0 + R]).to(dev), torch.from_numpy(al[r0:r0 + R]).to(dev))
            g = _autograd_dx(model, pts, c).cpu().numpy()
            acc = S.accumulate_reference(g, img[r0:r0 + R], w[r0:r0 + R], B, acc=acc)
        m, tot = S.finish_reference(acc, x.numpy(), np.float32(base), np.arange(B), True, "sum")
        assert torch.equal(attr[:, k].cpu(), torch.from_numpy(m)), (tag, c)
        with torch.no_grad():
            diff = model(xd)[:, c].double() - model(torch.full_like(xd, base[0]))[:, c].double()
        mass = np.abs(S.finish_reference(acc, x.numpy(), np.float32(base), np.arange(B), True, "none")[0].astype(np.float64)).sum(axis=(1, 2, 3))
        assert bool((np.abs(delta[:, k].cpu().numpy() - (tot - diff.cpu().numpy())) <= 1e-12 * mass).all())


def test_chunking_does_not_change_the_maps_beyond_rounding(dev):
    """Only equal chunking is bit-equal (the engines may pick another kernel for another number of rows); two chunkings agree to the
    project's fp32 figure (cosine >= 0.9999, norm ratio within 1e-3)."""
    for tag in TAGS:
        model, _, _, x = _make(tag, "fp32", dev)
        xd = x.to(dev)
        a = S.integrated_gradients(model, xd, [3], steps=4, channels="none", chunk=3)[0]
        b = S.integrated_gradients(model, xd, [3], steps=4, channels="none", chunk=4 * xd.shape[0])[0]
        cos, nr = _cmp(a, b.cpu())
        print("%s fp32 chunk 3 against one chunk: cos %.8f, norm ratio %.7f, bit-equal %s" % (tag, cos, nr, torch.equal(a, b)))
        assert cos >= 0.9999 and abs(nr - 1) <= 1e-3
        sa = S.smoothgrad(model, xd, [3], samples=4, sigma=0.3, seed=5, chunk=3)
        sb = S.smoothgrad(model, xd, [3], samples=4, sigma=0.3, seed=5)
        cos, nr = _cmp(sa, sb.cpu())
        print("%s fp32 smoothgrad chunk 3 against one chunk: cos %.8f, norm ratio %.7f" % (tag, cos, nr))
        assert cos >= 0.9999 and abs(nr - 1) <= 1e-3


_oracle_ig = {}


def _oracle(tag, dtype, dev, q=None):
    """integrated_gradients_reference over the oracle's eval forward (steps = 8, midpoint, mean-grey baseline), once per case.  The
    plain oracle (q None) is evaluated in float64, so that the reference's own rounding decides nothing: in float32 it does (see
    test_fp32_integrated_gradients_match_the_oracle).  The storage-rounding model q is defined on float32 and stays there."""
    if (tag, dtype) not in _oracle_ig:
        _, sd, fwd, x = _make(tag, dtype, dev)
        if q is None:
            sd, x = {k: (v.double() if v.is_floating_point() else v) for k, v in sd.items()}, x.double()
        f = lambda p: fwd(sd, p, q=q)
        _oracle_ig[(tag, dtype)] = S.integrated_gradients_reference(f, x, CLASSES, steps=8, channels="none")
    return _oracle_ig[(tag, dtype)]


def _check_against_oracle(tag, dtype, dev, cos_min, nr_tol, q=None):
    model, _, _, x = _make(tag, dtype, dev)
    attr_o, logits_o, delta_o = _oracle(tag, dtype, dev, q)
    attr, logits, delta = S.integrated_gradients(model, x.to(dev), CLASSES, steps=8, channels="none")
    bad = []
    for k, c in enumerate(CLASSES):
        cos, nr = _cmp(attr[:, k], attr_o[:, k])
        tot, tot_o = attr[:, k].double().sum((1, 2, 3)).cpu().numpy(), attr_o[:, k].sum(axis=(1, 2, 3))
        rel = float(np.abs(tot / tot_o - 1).max())
        print("%s %s class %d integrated gradients: cos %.6f, norm ratio %.5f, total rel %.2e (total %s, oracle %s), delta %s (oracle %s)"
              % (tag, dtype, c, cos, nr, rel, tot, tot_o, delta[:, k].cpu().numpy(), delta_o[:, k]))
        if cos < cos_min or abs(nr - 1) > nr_tol or (dtype == "fp32" and rel > 1e-3):
            bad.append((c, cos, nr, rel))
    assert not bad, bad


@pytest.mark.parametrize("tag", TAGS)
def test_fp32_integrated_gradients_match_the_oracle(dev, tag):
    """The bounds tests/test_eval_autograd_gpu.py holds x.grad to: the attribution is a positive-weight combination of such gradients
    times a fixed factor.  The oracle's total (the completeness identity's left side) within 1e-3 relative, per image and class.

    The oracle runs in float64 (_oracle).  In float32 its own rounding decides a ReLU kink: at path point alpha = 6.5 / 8 of image 1 of
    resnet1111_64 the unit [199, 1, 4] of the second stage's join has the pre-activation -6.7e-7 in float64 (the layer's rms is 1.4).
    The float32 oracle gives -3.1e-7 when the row is evaluated alone and +5.7e-8, the other side of the kink, when it is one of the
    eight rows of a batch.  The gradient of that row then differs from the float64 oracle's in 1388 input elements by up to 7e-3 of the
    largest, which moves the total of image 1 by 2.8e-4: 2e-6 of the attribution's mass sum|attr| = 140, but 1.08e-3 of class 3's
    total, which is that mass cancelled down to -0.263 (class 0's total is 3.77: 5.1e-5).  The GPU's gradients agree with the float64
    oracle at all eight path points (no element off by more than 1e-4 of the largest), batched or alone, bit-equal between the two.
    Against the float32 oracle (batched) the figures were: densenet2222_64 cos 1.000000, norm ratio 1.00000, total rel <= 1.7e-7;
    efficientnet-b0_224 1.000000, 1.00000, <= 1.4e-5; resnet1111_64 1.000000, 1.00001, 5.1e-5 (class 0) and 1.08e-3 (class 3)."""
    _check_against_oracle(tag, "fp32", dev, 0.9999, 1e-3)


def test_bf16_integrated_gradients_match_the_storage_rounding_oracle(dev):
    from oracle import nets
    _check_against_oracle("densenet2222_64", "bf16", dev, 0.97, 0.05, q=nets.bf16_storage)


@pytest.mark.parametrize("tag", TAGS)
@pytest.mark.parametrize("dtype", ["bf16", "fp32"])
def test_completeness(dev, tag, dtype):
    """logits are those of the plain eval forward, bit for bit; delta is total - (logit(x) - logit(baseline)) with both logits from
    plain eval forwards.  delta itself is printed for m = 4 and m = 32 and held to nothing: the network is piecewise linear and the
    error of the Riemann sum depends on the kinks the path crosses."""
    model, _, _, x = _make(tag, dtype, dev)
    xd = x.to(dev)
    base = torch.full_like(xd, 0.125)
    with torch.no_grad():
        lx, lb = model(xd), model(base)
    for m in (4, 32):
        attr, logits, delta = S.integrated_gradients(model, xd, CLASSES, steps=m, baseline=0.125, channels="none")
        assert torch.equal(logits, lx)
        tot = attr.double().sum((2, 3, 4))
        want = tot - (lx[:, CLASSES].double() - lb[:, CLASSES].double())
        mass = attr.double().abs().sum((2, 3, 4))
        print("%s %s m = %d: delta %s, logit difference %s" % (tag, dtype, m, delta.cpu().numpy(), (lx - lb)[:, CLASSES].cpu().numpy()))
        assert delta.dtype == torch.float64 and bool(((delta - want).abs() <= 1e-12 * mass).all())
    a2, l2, d2 = S.integrated_gradients(model, xd, CLASSES, steps=32, baseline=base, channels="none")       # the same baseline in full
    assert torch.equal(a2, attr) and torch.equal(l2, logits) and torch.equal(d2, delta)


def _state(model):
    return {k: v.clone() for k, v in model.state_dict().items()}


@pytest.mark.parametrize("tag", TAGS)
def test_contracts(dev, tag):
    model, _, _, x = _make(tag, "bf16", dev)
    xd = x.to(dev)
    calls = (lambda: S.input_gradient(model, xd, [3]), lambda: S.smoothgrad(model, xd, [3], samples=2, sigma=0.4),
             lambda: S.integrated_gradients(model, xd, [3], steps=2)[0])
    sd0 = _state(model)
    fired = []
    hooked = model.features.norm5 if hasattr(model, "features") else (model._stages()[-1] if hasattr(model, "_stages") else model.head[1])
    hook = hooked.register_forward_hook(lambda *a: fired.append(1))
    try:
        first = [c() for c in calls]
    finally:
        hook.remove()
    assert not fired and not model.training
    assert all(p.grad is None for p in model.parameters())             # None stays None
    with torch.no_grad():                                               # under an outer no_grad, and a second time: the same bits
        again = [c() for c in calls]
    assert all(torch.equal(_bits(a), _bits(b)) for a, b in zip(first, again))
    model.train()                                                       # from train() state: it is put back, nothing moves
    third = [c() for c in calls]
    assert model.training and all(torch.equal(a, b) for a, b in zip(first, third))
    model.eval()
    sd1 = _state(model)
    assert list(sd0) == list(sd1) and all(torch.equal(sd0[k], sd1[k]) for k in sd0), "running statistics / num_batches_tracked moved"
    # populated gradients (views of the engine's flat buffer after a step) keep their bits
    from oracle import step
    step.bce_sum_mean(model(xd), synth.targets(99, xd.shape[0], 5).to(dev)).backward()
    grads = {k: p.grad.clone() for k, p in model.named_parameters()}
    assert all(g is not None for g in grads.values())
    for c in calls:
        c()
    for k, p in model.named_parameters():
        assert p.grad is not None and torch.equal(_bits(p.grad), _bits(grads[k])), k
    model.zero_grad(set_to_none=True)
    for fn in (S.input_gradient, S.smoothgrad, S.integrated_gradients):
        with pytest.raises(RuntimeError, match="GPU only"):
            fn(model, x, [3])


# ------------------------------------------------------------------------------------------------------------ command line
def test_cli_writes_saliency_maps(dev, tmp_path):
    from chexpert_amd import cli
    cli.main(["--visualize", "--synthetic", "16", "--batch_size", "4", "--resize", "64", "--output_dir", str(tmp_path),
              "--saliency", "ig", "--saliency_steps", "2", "--saliency_classes", "0"])
    d = os.path.join(str(tmp_path), "vis")
    files = sorted(os.listdir(d))
    N = np.load(os.path.join(d, "grad_cam.npy")).shape[0]
    maps, scale = np.load(os.path.join(d, "saliency_ig.npy")), np.load(os.path.join(d, "saliency_ig_scale.npy"))
    assert maps.shape == (N, 1, 64, 64) and maps.dtype == np.float16 and scale.shape == (N, 1) and scale.dtype == np.float32
    assert np.isfinite(maps).all() and (np.abs(maps).max(axis=(2, 3)) == 1.0).all() and (scale > 0).all() and (maps < 0).any()
    assert sum(f.startswith("saliency_ig_synthetic_") and f.endswith(".png") for f in files) == N
    assert sum(f.startswith("vis_") and f.endswith(".png") for f in files) == 5 + 3      # the existing set is what it was
