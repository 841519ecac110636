"""GPU: the squeeze-excite, Swish and DropConnect entry points of effnet.hip, one kernel at a time, against float64 restatements
written here (SELayer / MBConv / drop_connect: models/efficientnet.py:27-131 of the reference).  The restatements are computed
from the inputs as stored (rounded to bf16 for bf16 storage); every kernel runs through its bf16 entry point and its `_f32` twin.

The shapes are chosen for the launch geometry they reach, which is a function of the batch size:
  splits = min(max(1, 1024 / B), HW / 16 + 1) pixel splits of the pool and of the SE-backward reduce,
  CP = C / 8 lanes per pixel row in blocks of CP * (256 / CP) threads, channel slices of se_fwd_kernel, image groups of 16.

Bounds.  Element-wise outputs: |got - ref| <= eps |ref| + 1e-5 max|ref| with eps = 2^-8 (half a bf16 ulp) or 2^-24 (half an fp32
ulp) and 1e-5 for the fp32 evaluation of one fma and one Swish.  fp32 sums and FC results: 1e-4 of the reference's abs-max, the
bar tests/test_dwconv_gpu.py::test_se_backward sets for this arithmetic (measured maxima: DESIGN.md section 4.26).  Every reduction
test also checks its inputs: with the last pixel of the last image left out the reference moves by more than 10 x the tolerance
in that image's most affected channel, so a tail pixel counted twice, or not at all, cannot hide under the bound."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

BF, F32 = torch.bfloat16, torch.float32
STORAGE = [pytest.param(BF, id="bf16"), pytest.param(F32, id="f32")]
SENT = 7.0
SUM_TOL = 1e-4
CASE = "?"


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


def nhwc(t, H, W, dev, dt):            # (B, HW, C) values -> dense NHWC tensor of the storage type on the device
    B, HW, C = t.shape
    return t.view(B, H, W, C).to(dt).to(dev)


def full(dev, shape, dt=F32):
    return torch.full(shape, SENT, device=dev, dtype=dt)


def entry(name, dt):
    from chexpert_amd._lib import lib
    return getattr(lib(), name + ("_f32" if dt == F32 else ""))


def close(got, want, what, rel=SUM_TOL):
    err = (got.double().cpu() - want.double()).abs().max().item() / (want.abs().max().item() + 1e-300)
    print("ERR sum %s %s %.3e" % (CASE, what, err))
    assert err < rel, "%s: rel err %.3e" % (what, err)


def close_elem(got, want, dt, what):
    """|got - ref| <= eps |ref| + 1e-5 max|ref|; prints the largest additive part the elements need, in units of max|ref|."""
    want = want.double()
    eps = 2.0 ** -8 if dt == BF else 2.0 ** -24
    d = (got.double().cpu() - want).abs_().sub_(want.abs().mul_(eps))
    worst = d.max().item() / (want.abs().max().item() + 1e-300)
    print("ERR elem %s %s %.3e" % (CASE, what, worst))
    assert worst <= 1e-5, "%s: %.3e of max|ref| beyond half an ulp" % (what, worst)


def sensitive(ref_row, without_row, ref_max, what, tol=SUM_TOL):
    """Condition on the inputs: ref_row / without_row are the reference of one image (or of the batch sums) with and without
    its last pixel; the most affected channel moves by more than 10 x the tolerance."""
    move = (ref_row.double() - without_row.double()).abs().max().item() / (ref_max + 1e-300)
    print("SENS %s %s %.1f x tol" % (CASE, what, move / tol))
    assert move > 10 * tol, "%s: leaving a pixel out moves the reference by %.2e of its abs-max only" % (what, move)


def swish(z):
    return z * torch.sigmoid(z)


def dswish(z):
    s = torch.sigmoid(z)
    return s * (1 + z * (1 - s))


def act_ref(z, act):
    return z if act == 0 else z.clamp_min(0) if act == 1 else swish(z)


def splits_of(B, HW):
    return min(max(1, 1024 // B), HW // 16 + 1)


SHAPES = [  # B, H, W, C, R
    (4, 16, 16, 40, 10),      # HW 256: 17 splits of 16 pixels, the last split is EMPTY; CP 5: a block of 255 threads
    (3, 7, 7, 40, 10),        # 4 splits of 13, the last has 10 pixels; 51 pixel rows per block > pixels: every lane takes the clamp
    (2, 5, 3, 8, 2),          # 1 split, CP 1
    (8, 31, 31, 24, 6),       # 61 splits of 16, the last split has exactly one pixel
    (2, 33, 33, 16, 4),       # 69 splits > 64: the second level of the q, q + 64, ... row order (se_fwd_kernel, se_bwd_a_kernel)
    (70, 12, 12, 272, 10),    # 10 splits of 15, the last has 9 pixels; se_fwd slices 128, 128, 16; image groups 16 x 4 + 6; R % 4 != 0
    (70, 16, 16, 8, 3),       # the split count is 1024 / B = 14 (HW / 16 + 1 would be 17): 14 splits of 19, the last has 9 pixels
    (2, 4, 4, 2688, 112),     # CP 336 > 256: one pixel row per block
    (1100, 2, 2, 8, 1),       # 1024 / B = 0 -> 1 split; R = 1
]
# 197 splits: cx_rows_reduce takes its four-rows-in-flight loop (rows q + 192 exist), the consumers' in-kernel sums must still give
# its bits.  (At HW = 3136 one pixel is 3e-4 of a mean: under 10 x any 1e-4 bound, so this shape carries no sensitivity condition.)
ORDER_SHAPE = (2, 56, 56, 8, 2)
CP_WIDE = (1, 5, 1, 4104, 0)      # cx_se_act_bwd only: CP 513 > 512 selects the <T, 1, 1024> instantiation
FLAT_BIG = (2, 128, 128, 520, 0)  # flat element-wise kernels only: B HW C / 8 > 8192 x 256, the grid-stride loop runs a second pass


def sid(s):
    return "B%d_%dx%d_C%d" % s[:4] + ("_R%d" % s[4] if s[4] else "")


def se_inputs(B, H, W, C, R, dt):
    """Block input, BatchNorm coefficients and SE parameters (FC weights scaled so that h1 and the logits of s are O(1))."""
    HW = H * W
    x = stored(mag(1, (B, HW, C), 0.5, 2.0), dt)
    sc, sh = rnd(2, (C,), 0.5, 1.5), rnd(3, (C,), -0.5, 0.5)
    w1, b1 = rnd(4, (R, C)) * (2.0 / C ** 0.5), rnd(5, (R,), -0.2, 0.2)
    w2, b2 = rnd(6, (C, R)) * (2.0 / R ** 0.5), rnd(7, (C,), -0.2, 0.2)
    return x, sc, sh, w1, b1, w2, b2


# ------------------------------------------------------------------------------------------------ 1. pool and excitation
@pytest.mark.parametrize("dt", STORAGE)
@pytest.mark.parametrize("shape", SHAPES + [ORDER_SHAPE], ids=sid)
def test_pool_and_excitation(dev, shape, dt):
    """cx_gap_affine_act (three activations; split rows, no rows, rows one float short), cx_se_fwd, cx_gap_se_fwd: pooled, h1, s;
    reproducible with rows, and cx_gap_se_fwd gives the bits of cx_gap_affine_act(rows) + cx_se_fwd."""
    from chexpert_amd import ops
    from chexpert_amd._lib import lib, ptr, check, stream_ptr
    B, H, W, C, R = shape
    HW, n_rows = H * W, splits_of(B, H * W) * B * C
    x, sc, sh, w1, b1, w2, b2 = se_inputs(B, H, W, C, R, dt)
    xd = nhwc(x, H, W, dev, dt)
    scd, shd, w1d, b1d, w2d, b2d = (t.to(dev) for t in (sc, sh, w1, b1, w2, b2))
    z = x.double() * sc.double() + sh.double()
    gap = entry("cx_gap_affine_act", dt)
    for act in (0, 1, 2):
        a = act_ref(z, act)
        want = a.mean(1)
        if shape != ORDER_SHAPE:
            sensitive(want[-1], a[-1, :-1].sum(0) / HW, want.abs().max().item(), "pooled act %d" % act)
        outs = []
        for _ in range(2):                 # split rows: reproducible; the floats behind the announced size are not the kernel's
            pooled, rows = full(dev, (B, C)), full(dev, (n_rows + 64,))
            check(gap(ptr(xd), ptr(scd), ptr(shd), ptr(pooled), B, HW, C, act, ptr(rows), n_rows, stream_ptr()), "cx_gap_affine_act")
            outs.append(pooled)
        assert torch.equal(outs[0], outs[1])
        assert bool((rows[n_rows:] == SENT).all())
        close(outs[0], want, "pooled act %d rows" % act)
        pooled = full(dev, (B, C))         # no rows: atomics
        ops.gap_affine_act(xd, scd, shd, pooled, act=act)
        close(pooled, want, "pooled act %d atomic" % act)
        pooled, rows = full(dev, (B, C)), full(dev, (n_rows,))      # one float short: atomics, the rows stay untouched
        check(gap(ptr(xd), ptr(scd), ptr(shd), ptr(pooled), B, HW, C, act, ptr(rows), n_rows - 1, stream_ptr()), "cx_gap_affine_act")
        close(pooled, want, "pooled act %d short rows" % act)
        assert bool((rows == SENT).all())
    # excitation
    want_p = swish(z).mean(1)
    want_h = want_p @ w1.double().t() + b1.double()
    want_s = torch.sigmoid(swish(want_h) @ w2.double().t() + b2.double())
    pin, h1, s = want_p.float().to(dev), full(dev, (B, R)), full(dev, (B, C))
    check(lib().cx_se_fwd(ptr(pin), ptr(w1d), ptr(b1d), ptr(w2d), ptr(b2d), ptr(h1), ptr(s), B, C, R, stream_ptr()), "cx_se_fwd")
    close(h1, want_h, "h1 se_fwd")
    close(s, want_s, "s se_fwd")
    outs = []
    for _ in range(2):
        pooled, h1, s, rows = full(dev, (B, C)), full(dev, (B, R)), full(dev, (B, C)), full(dev, (n_rows,))
        ops.gap_se_fwd(xd, scd, shd, pooled, w1d, b1d, w2d, b2d, h1, s, act=2, rows=rows)
        outs.append((pooled, h1, s))
    assert all(torch.equal(a_, b_) for a_, b_ in zip(outs[0], outs[1]))
    for got, want, what in zip(outs[0], (want_p, want_h, want_s), ("pooled", "h1", "s")):
        close(got, want, what + " gap_se_fwd rows")
    pooled, h1, s, rows = full(dev, (B, C)), full(dev, (B, R)), full(dev, (B, C)), full(dev, (n_rows,))      # the separate launches
    ops.gap_affine_act(xd, scd, shd, pooled, act=2, rows=rows)
    check(lib().cx_se_fwd(ptr(pooled), ptr(w1d), ptr(b1d), ptr(w2d), ptr(b2d), ptr(h1), ptr(s), B, C, R, stream_ptr()), "cx_se_fwd")
    assert all(torch.equal(a_, b_) for a_, b_ in zip(outs[0], (pooled, h1, s))), "cx_gap_se_fwd differs from the separate launches"
    pooled, h1, s = full(dev, (B, C)), full(dev, (B, R)), full(dev, (B, C))       # no rows: the three-launch atomic form
    ops.gap_se_fwd(xd, scd, shd, pooled, w1d, b1d, w2d, b2d, h1, s, act=2)
    for got, want, what in zip((pooled, h1, s), (want_p, want_h, want_s), ("pooled", "h1", "s")):
        close(got, want, what + " gap_se_fwd atomic")


# ------------------------------------------------------------------------------------------------ 2. Swish x SE scale
@pytest.mark.parametrize("dt", STORAGE)
@pytest.mark.parametrize("shape", SHAPES + [FLAT_BIG], ids=sid)
def test_scale_act_bc(dev, shape, dt):
    """cx_scale_act_bc: u = swish(x*sc + sh) * s[b][c], and without s."""
    from chexpert_amd import ops
    B, H, W, C, _ = shape
    x = stored(mag(11, (B, H * W, C), 0.5, 2.0), dt)
    sc, sh, s = rnd(12, (C,), 0.5, 1.5), rnd(13, (C,), -0.5, 0.5), rnd(14, (B, C), 0.05, 0.95)
    xd, scd, shd, sd = nhwc(x, H, W, dev, dt), sc.to(dev), sh.to(dev), s.to(dev)
    a = swish(x.double() * sc.double() + sh.double())
    for given in (True, False):
        u = full(dev, (B, H, W, C), dt)
        ops.scale_act_bc(xd, scd, shd, sd if given else None, u)
        close_elem(u.view(B, H * W, C).float(), a * s.double()[:, None, :] if given else a, dt, "u" if given else "u without s")


# ------------------------------------------------------------------------------------------------ 3. SE backward
@pytest.mark.parametrize("dt", STORAGE)
@pytest.mark.parametrize("shape", SHAPES + [ORDER_SHAPE], ids=sid)
def test_se_backward_chain(dev, shape, dt):
    """cx_se_bwd_reduce (ds) and cx_se_bwd_fused in its three routes against float64 autograd through pooled -> h1 -> s and
    u = swish(z) * s; route 1 is reproducible and gives the bits of cx_se_bwd_reduce(rows) + cx_se_bwd(slabs)."""
    from chexpert_amd import ops
    from chexpert_amd._lib import lib, ptr, check, stream_ptr
    B, H, W, C, R = shape
    HW, n_rows = H * W, splits_of(B, H * W) * B * C
    x, sc, sh, w1, b1, w2, b2 = se_inputs(B, H, W, C, R, dt)
    du = stored(mag(21, (B, HW, C), 0.25, 1.0), dt)
    p = [t.double().requires_grad_(True) for t in (w1, b1, w2, b2)]
    a = swish(x.double() * sc.double() + sh.double())
    pooled = a.mean(1).requires_grad_(True)
    h1 = pooled @ p[0].t() + p[1]
    s = torch.sigmoid(swish(h1) @ p[2].t() + p[3])
    (a * s[:, None, :] * du.double()).sum().backward()
    want_ds = (a * du.double()).sum(1)
    if shape != ORDER_SHAPE:
        sensitive(want_ds[-1], (a[-1, :-1] * du[-1, :-1].double()).sum(0), want_ds.abs().max().item(), "ds")
    names = ("dW1", "db1", "dW2", "db2")
    init = [rnd(30 + i, t.shape) * t.grad.abs().max().float() for i, t in enumerate(p)]       # the accumulators hold something already
    xd, dud = nhwc(x, H, W, dev, dt), nhwc(du, H, W, dev, dt)
    scd, shd, w1d, w2d = (t.to(dev) for t in (sc, sh, w1, w2))
    sd, h1d, pd = (t.detach().float().to(dev) for t in (s, h1, pooled))
    red, fused = entry("cx_se_bwd_reduce", dt), entry("cx_se_bwd_fused", dt)

    def check_fc(d, dpooled, what):
        for got, i0, t, nm in zip(d, init, p, names):
            close(got.cpu() - i0, t.grad, "%s %s" % (nm, what))
        close(dpooled, pooled.grad, "dpooled " + what)

    outs = []
    for _ in range(2):                     # ds through split rows: reproducible
        ds, rows = full(dev, (B, C)), full(dev, (n_rows + 64,))
        check(red(ptr(dud), ptr(xd), ptr(scd), ptr(shd), ptr(ds), B, HW, C, ptr(rows), n_rows, stream_ptr()), "cx_se_bwd_reduce")
        outs.append(ds)
    assert torch.equal(outs[0], outs[1]) and bool((rows[n_rows:] == SENT).all())
    close(outs[0], want_ds, "ds rows")
    ds_rows = outs[0]
    ds = full(dev, (B, C))
    check(red(ptr(dud), ptr(xd), ptr(scd), ptr(shd), ptr(ds), B, HW, C, None, 0, stream_ptr()), "cx_se_bwd_reduce")
    close(ds, want_ds, "ds atomic")

    def run(rows, ws):
        d, ds, dpooled = [t.clone().to(dev) for t in init], full(dev, (B, C)), full(dev, (B, C))
        check(fused(ptr(dud), ptr(xd), ptr(scd), ptr(shd), ptr(ds), ptr(sd), ptr(h1d), ptr(pd), ptr(w1d), ptr(w2d), ptr(d[0]), ptr(d[1]),
                    ptr(d[2]), ptr(d[3]), ptr(dpooled), B, HW, C, R, ptr(rows), 0 if rows is None else n_rows, ptr(ws),
                    0 if ws is None else ws.numel(), stream_ptr()), "cx_se_bwd_fused")
        return d, ds, dpooled

    scratch = torch.empty(8 << 20, device=dev)
    outs = []
    for _ in range(2):                     # route 1: split rows into the first FC pass, slab workspace
        d, _, dpooled = run(full(dev, (n_rows,)), scratch)
        assert lib().cx_last_slab_floats() > 0
        outs.append(d + [dpooled])
    assert all(torch.equal(a_, b_) for a_, b_ in zip(outs[0], outs[1]))
    check_fc(outs[0][:4], outs[0][4], "route 1")
    d, dpooled = [t.clone().to(dev) for t in init], full(dev, (B, C))       # the separate launches, same workspaces
    check(lib().cx_se_bwd(ptr(ds_rows), ptr(sd), ptr(h1d), ptr(pd), ptr(w1d), ptr(w2d), ptr(d[0]), ptr(d[1]), ptr(d[2]), ptr(d[3]),
                          ptr(dpooled), B, C, R, ptr(scratch), scratch.numel(), stream_ptr()), "cx_se_bwd")
    assert all(torch.equal(a_, b_) for a_, b_ in zip(outs[0], d + [dpooled])), "cx_se_bwd_fused differs from the separate launches"
    # route 2: rows, no slab workspace -- falls back to the one-kernel form and must then have written ds (through the wrapper,
    # whose workspace is the library-wide one: off for this call)
    was = ops.WGRAD_SCRATCH_FLOATS
    ops.set_det_wgrad(False)
    try:
        d, ds, dpooled = [t.clone().to(dev) for t in init], full(dev, (B, C)), full(dev, (B, C))
        ops.se_bwd_fused(dud, xd, scd, shd, ds, sd, h1d, pd, w1d, w2d, d[0], d[1], d[2], d[3], dpooled, rows=full(dev, (n_rows,)))
    finally:
        ops.WGRAD_SCRATCH_FLOATS = was
    assert lib().cx_last_slab_floats() == 0
    assert torch.equal(ds, ds_rows)
    check_fc(d, dpooled, "route 2")
    d, ds, dpooled = run(None, None)       # route 3: neither
    close(ds, want_ds, "ds route 3")
    check_fc(d, dpooled, "route 3")


# ------------------------------------------------------------------------------------------------ 4. Swish / BatchNorm backward glue
def stat_runs(launch, C, dev, want1, want2, dz_of=None):
    """launch(S1, S2, stat_rows) -> the element-wise output or None.  Atomic sums, then 512 and 3 statistic rows: each twice with
    the same bits, 0 < rows written <= rows asked for, the rows add up to the atomic sums."""
    from chexpert_amd._lib import lib
    st = torch.zeros(2, C, device=dev)
    base = launch(st[0], st[1], 0)
    close(st[0], want1, "S1 atomic")
    close(st[1], want2, "S2 atomic")
    for stat_rows in (512, 3):
        outs = []
        for _ in range(2):
            rows = full(dev, (2, stat_rows, C))
            out = launch(rows[0], rows[1], stat_rows)
            n = lib().cx_last_stat_rows()
            assert 0 < n <= stat_rows
            assert bool((rows[:, n:] == SENT).all())
            outs.append(rows[:, :n].clone())
            assert base is None or torch.equal(out, base)
        assert torch.equal(outs[0], outs[1])
        close(outs[0][0].sum(0), want1, "S1 of %d rows" % stat_rows)
        close(outs[0][1].sum(0), want2, "S2 of %d rows" % stat_rows)
        close(outs[0][0].sum(0), st[0].cpu(), "S1 rows against atomics, %d" % stat_rows)
        close(outs[0][1].sum(0), st[1].cpu(), "S2 rows against atomics, %d" % stat_rows)
    return base


def act_bwd_reference(shape, operands, dt):
    """Inputs of cx_se_act_bwd and dz, S1, S2 in float64.  dpooled is of the size HW x gradient, so that dpooled / HW weighs as much
    as du * s; its sign alternates from image to image with magnitudes within 3 % of a per-channel one: a sum over the pixels of an
    image is coherent in dpooled, and only images that cancel leave sums in which one pixel is visible."""
    B, H, W, C, _ = shape
    HW = H * W
    x = stored(mag(41, (B, HW, C), 0.5, 2.0), dt)
    du = stored(mag(42, (B, HW, C), 0.25, 1.0), dt) if operands != "head" else None
    s = rnd(43, (B, C), 0.05, 0.95) if operands == "du_s_dpooled" else None
    dp = None
    if operands != "stem":
        alt = (1.0 - 2.0 * (torch.arange(B) % 2).float())[:, None]
        dp = mag(44, (1, C), 0.25, 1.0) * alt * rnd(49, (B, C), 0.97, 1.03) * (0.5 * HW)
    sc, sh, mu, r = rnd(45, (C,), 0.5, 1.5), rnd(46, (C,), -0.5, 0.5), rnd(47, (C,), -0.5, 0.5), rnd(48, (C,), 0.5, 2.0)
    xx = x.double()
    da = torch.zeros_like(xx)
    if dp is not None:
        da = da + (dp.double() / HW)[:, None, :]
    if du is not None:
        da = da + du.double() * (s.double()[:, None, :] if s is not None else 1.0)
    dz = da * dswish(xx * sc.double() + sh.double())
    t2 = dz * (xx - mu.double()) * r.double()
    S1, S2 = dz.sum((0, 1)), t2.sum((0, 1))
    sensitive(S1, dz.view(-1, C)[:-1].sum(0), S1.abs().max().item(), "S1")
    sensitive(S2, t2.view(-1, C)[:-1].sum(0), S2.abs().max().item(), "S2")
    return x, du, s, dp, sc, sh, mu, r, dz, S1, S2


@pytest.mark.parametrize("dt", STORAGE)
@pytest.mark.parametrize("operands", ["du_s_dpooled", "head", "stem"])
@pytest.mark.parametrize("shape", SHAPES + [CP_WIDE], ids=sid)
def test_se_act_bwd(dev, shape, operands, dt):
    """cx_se_act_bwd: dz = (du * s + dpooled / HW) * swish'(x*sc + sh) with the operand sets of the MBConv block, the head (no du,
    no s) and the stem (du alone); S1 / S2 are sums of the unrounded dz."""
    from chexpert_amd import ops
    B, H, W, C, _ = shape
    HW = H * W
    x, du, s, dp, sc, sh, mu, r, dz, S1, S2 = act_bwd_reference(shape, operands, dt)
    opt = lambda t: None if t is None else t.to(dev)
    xd, dud = nhwc(x, H, W, dev, dt), None if du is None else nhwc(du, H, W, dev, dt)
    scd, shd, mud, rd, sd, dpd = (opt(t) for t in (sc, sh, mu, r, s, dp))

    def launch(s1, s2, stat_rows):
        out = full(dev, (B, H, W, C), dt)
        n = ops.se_act_bwd(dud, xd, scd, shd, mud, rd, sd, dpd, out, s1, s2, stat_rows=stat_rows)
        assert (n is None) == (stat_rows == 0)
        return out

    out = stat_runs(launch, C, dev, S1, S2)
    close_elem(out.view(B, HW, C).float(), dz, dt, "dz")


def bn_lin_reference(shape, dt):
    B, H, W, C, _ = shape
    g, y = stored(mag(51, (B, H * W, C), 0.25, 1.0), dt), stored(mag(52, (B, H * W, C), 0.5, 2.0), dt)
    mu, r = rnd(53, (C,), -0.5, 0.5), rnd(54, (C,), 0.5, 2.0)
    t1 = g.double().view(-1, C)
    t2 = t1 * (y.double().view(-1, C) - mu.double()) * r.double()
    S1, S2 = t1.sum(0), t2.sum(0)
    sensitive(S1, t1[:-1].sum(0), S1.abs().max().item(), "S1")
    sensitive(S2, t2[:-1].sum(0), S2.abs().max().item(), "S2")
    return g, y, mu, r, S1, S2


@pytest.mark.parametrize("dt", STORAGE)
@pytest.mark.parametrize("shape", SHAPES, ids=sid)
def test_bn_lin_bwd_stats(dev, shape, dt):
    """cx_bn_lin_bwd_stats: S1 = sum g, S2 = sum g * (y - mean) * rstd."""
    from chexpert_amd import ops
    B, H, W, C, _ = shape
    g, y, mu, r, S1, S2 = bn_lin_reference(shape, dt)
    gd, yd, mud, rd = nhwc(g, H, W, dev, dt), nhwc(y, H, W, dev, dt), mu.to(dev), r.to(dev)

    def launch(s1, s2, stat_rows):
        n = ops.bn_lin_bwd_stats(gd, yd, mud, rd, s1, s2, stat_rows=stat_rows)
        assert (n is None) == (stat_rows == 0)

    stat_runs(launch, C, dev, S1, S2)


# ------------------------------------------------------------------------------------------------ 5. block output and DropConnect
def sample_scales(B, keep=0.8):        # distinct per image, with a dropped image (0) and a kept one (1 / keep)
    ps = 0.5 + torch.arange(B, dtype=F32) / B
    ps[0] = 0.0
    ps[1] = 1.0 / keep
    return ps


@pytest.mark.parametrize("dt", STORAGE)
@pytest.mark.parametrize("shape", SHAPES + [FLAT_BIG], ids=sid)
def test_affine2_out_and_scale_rows(dev, shape, dt):
    """cx_affine2_out: out = ps[image] * (a*pa + pc) + b*pb with and without b / ps; cx_scale_rows: out = ps[image] * g."""
    from chexpert_amd import ops
    B, H, W, C, _ = shape
    a, b = stored(mag(61, (B, H * W, C), 0.5, 2.0), dt), stored(mag(62, (B, H * W, C), 0.5, 2.0), dt)
    pa, pb, pc = rnd(63, (C,), 0.5, 1.5), rnd(64, (C,), 0.5, 1.5), rnd(65, (C,), -0.5, 0.5)
    ps = sample_scales(B)
    ad, bd = nhwc(a, H, W, dev, dt), nhwc(b, H, W, dev, dt)
    pad, pbd, pcd, psd = (t.to(dev) for t in (pa, pb, pc, ps))
    lin = a.double() * pa.double() + pc.double()
    skip = b.double() * pb.double()
    for with_b in (True, False):
        for with_ps in (True, False):
            out = full(dev, (B, H, W, C), dt)
            ops.affine2_out(ad, bd if with_b else None, pad, pbd if with_b else None, pcd, psd if with_ps else None, out)
            want = lin * ps.double()[:, None, None] if with_ps else lin
            close_elem(out.view(B, H * W, C).float(), want + skip if with_b else want, dt, "out b=%d ps=%d" % (with_b, with_ps))
    out = full(dev, (B, H, W, C), dt)
    ops.scale_rows(ad, psd, out)
    close_elem(out.view(B, H * W, C).float(), a.double() * ps.double()[:, None, None], dt, "scale_rows")


# ------------------------------------------------------------------------------------------------ 6. masks and the head
U64 = (1 << 64) - 1


def mask_ref(n, keep, base, step):
    """splitmix64 of base + step * 1000003 + 0x9E37...15 * (i + 1) (mod 2^64), its top 24 bits as u in [0, 1), u < keep."""
    seed = (base + step * 1000003) & U64
    z = np.uint64(seed) + np.uint64(0x9E3779B97F4A7C15) * np.arange(1, n + 1, dtype=np.uint64)       # uint64 arrays wrap
    z = (z ^ (z >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)
    z = (z ^ (z >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)
    z = z ^ (z >> np.uint64(31))
    u = (z >> np.uint64(40)).astype(np.float32) * np.float32(1.0 / 16777216.0)
    return np.where(u < np.float32(keep), np.float32(1) / np.float32(keep), np.float32(0)).astype(np.float32)


def test_dropout_mask_and_counter(dev):
    """cx_counter_add bumps the device counter; cx_dropout_mask_dev draws the mask of the counter's value, bit for bit the host
    restatement, with a base close to 2^64 (the seed wraps); nothing is written behind n."""
    from chexpert_amd import ops
    base = U64 - 12345
    counter = torch.tensor([11], dtype=torch.int64, device=dev)
    ops.counter_add(counter, 3)
    ops.counter_add(counter, (1 << 33) + 5)
    step = int(counter.item())
    assert step == 11 + 3 + (1 << 33) + 5
    assert (base + step * 1000003) > U64
    for n in (1, 255, 257, 100003):
        for keep in (1.0, 0.8, 0.5):
            buf = full(dev, (n + 64,))
            ops.dropout_mask_dev(buf[:n], keep, base, counter)
            got = buf.cpu().numpy()
            want = mask_ref(n, keep, base, step)
            assert np.array_equal(got[:n].view(np.uint32), want.view(np.uint32)), "mask n=%d keep=%g" % (n, keep)
            assert np.all(got[n:] == SENT)
            kept = got[:n][got[:n] != 0]
            assert np.all(kept == np.float32(1) / np.float32(keep))
            print("MASK n=%d keep=%g kept %d" % (n, keep, kept.size))
            assert kept.size == n if keep == 1.0 else (n < 255 or 0 < kept.size < n)
    ops.counter_add(counter)               # the default increment; another step, another mask
    assert int(counter.item()) == step + 1
    buf = full(dev, (100003,))
    ops.dropout_mask_dev(buf, 0.5, base, counter)
    assert np.array_equal(buf.cpu().numpy(), mask_ref(100003, 0.5, base, step + 1))
    assert not np.array_equal(buf.cpu().numpy(), mask_ref(100003, 0.5, base, step))


def test_mul_f32_in_place(dev):
    """cx_mul_f32 with out = a: one IEEE multiply per element."""
    from chexpert_amd import ops
    for n in (1, 255, 257, 100003):
        a, b = mag(71, (n,), 0.5, 2.0), mag(72, (n,), 0.25, 1.0)
        buf = full(dev, (n + 64,))
        buf[:n] = a.to(dev)
        ad, bd = buf[:n], b.to(dev)
        ops.mul_f32(ad, bd, ad)
        assert torch.equal(buf[:n].cpu(), a * b) and bool((buf[n:] == SENT).all())
        assert torch.equal(bd.cpu(), b)


@pytest.mark.parametrize("N", [1, 5, 14])
@pytest.mark.parametrize("C", [1, 63, 1280, 1793])
def test_linear_fwd(dev, C, N):
    """cx_linear_fwd: y = x W^T (+ bias), the classifier."""
    from chexpert_amd import ops
    B = 3
    x, w, bias = mag(81, (B, C), 0.5, 2.0), rnd(82, (N, C)), rnd(83, (N,))
    xd, wd, bd = x.to(dev), w.to(dev), bias.to(dev)
    want = x.double() @ w.double().t()
    for given in (True, False):
        y = full(dev, (B, N))
        ops.linear_fwd(xd, wd, bd if given else None, y)
        close(y, want + bias.double() if given else want, "y" if given else "y without bias")
