"""GPU: the glue every network runs -- stem pool, head, transition un-pool, residual-join backward, layout conversions, dropout slice,
weight tables and the edges of the BatchNorm coefficient kernels (csrc/elementwise.hip; the 8-channel conversions of csrc/effnet.hip
and cx_f32_to_bf16 of csrc/aaconv.hip) -- one kernel at a time against float64 restatements written here, computed from the inputs
as stored.  Every kernel with an `_f32` twin runs through both entry points (`entry(name, dt)` appends the suffix):
  cx_bnrelu_maxpool_fwd / _bwd, cx_head_fwd, cx_gap_relu_bn_bwd, cx_unpool2_mask, cx_affine2_relu_mask, cx_relu_bwd_stats_mask,
  cx_nchw3_to_nhwc4 / 8, cx_u8_to_nhwc4 / 8, cx_dropout_slice_fwd / _bwd, cx_pack_weights_table  -- each with its _f32 twin --  and
  cx_head_bwd, cx_f32_to_bf16, cx_bf16_to_f32_nchw, cx_affine_to_f32_nchw, cx_gradcam_map, cx_pack_weights, cx_chan_map_table,
  cx_bn_coef, cx_bn_coef_moments, which have none.

The shapes are chosen for the launch geometry they reach: CP = C / 8 lanes per pixel in workgroups of 256 threads, 256 / CP pixels
per workgroup and pass, TA = (256 / CP) * CP active threads where CP does not divide 256, a grid capped by the statistic-row
capacity (the cap is what makes a workgroup take a second pass at these sizes).  Outputs are sentinel-filled with their pitch
padding checked; inputs carry NaN in their pitch padding.

Bounds (those of tests/test_effnet_glue_gpu.py).  Element-wise outputs: |got - ref| <= eps |ref| + 1e-5 max|ref| with eps = 2^-8 /
2^-24; fp32 sums and FC results: 1e-4 of the reference's abs-max; moves and single roundings: torch.equal.  Input conditions,
asserted here: every sign decision fma(x, sc, sh) > 0 has a margin of 1e-2 (so float64 cannot disagree with the fp32 fma), every
sum moves by more than 10 x its tolerance when the last pixel of the last image is left out, the planted max-pool ties exist.
Measured maxima: DESIGN.md section 4.42."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

BF, F32 = torch.bfloat16, torch.float32
STORAGE = [pytest.param(BF, id="bf16"), pytest.param(F32, id="f32")]
SENT = 7.0
NAN = float("nan")
SUM_TOL = 1e-4
CASE = "?"
CX_EINVAL, CX_EALIGN, CX_ESHAPE, CX_ESTATROWS = -1, -2, -3, -5       # include/chexpert_hip.h


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
    """Condition on the inputs: a reference sum with and without the last pixel of the last image; the most affected channel
    moves by more than 10 x the tolerance."""
    move = (ref_row.double() - without_row.double()).abs().max().item() / (ref_max + 1e-300)
    print("SENS %s %s %.1f x tol" % (CASE, what, move / tol))
    assert move > 10 * tol, "%s: leaving a pixel out moves the reference by %.2e of its abs-max only" % (what, move)


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


def stat_runs(launch, k, C, dev, wants, natural, caps, names):
    """launch(stats, stat_rows) -> the element-wise output; stats: k tensors ([C] with stat_rows = 0, [stat_rows][C] else).
    Atomic sums into zeros, then each row capacity twice with the same bits: min(capacity, natural grid) rows written, the rows
    behind them untouched, the written rows add up to the reference."""
    st = torch.zeros(k, C, device=dev)
    base = launch([st[i] for i in range(k)], 0)
    for i in range(k):
        close(st[i], wants[i], names[i] + " atomic")
    for cap in caps:
        outs = []
        for _ in range(2):
            rows = full(dev, (k, cap, C))
            out = launch([rows[i] for i in range(k)], cap)
            n = last_rows()
            assert n == min(cap, natural), "%d rows written, capacity %d, natural grid %d" % (n, cap, natural)
            assert bool((rows[:, n:] == SENT).all())
            outs.append(rows[:, :n].clone())
            assert torch.equal(out, base)
        assert torch.equal(outs[0], outs[1])
        for i in range(k):
            close(outs[0][i].sum(0), wants[i], "%s of %d rows (capacity %d)" % (names[i], n, cap))
    return base


# ------------------------------------------------------------------------------------------------ 1. stem pool
STEM = [
    (1, 2, 2, 8),         # one window, 5 of its 9 taps outside the image, CP 1
    (2, 12, 16, 64),      # 96 pooled pixels at 32 per workgroup: natural grid 3, capacities 2 and 1 make workgroups loop
    (1, 6, 10, 256),      # CP 32, 8 pixels per workgroup: natural grid 2
    (3, 4, 6, 16),        # small general case
    (2, 6, 6, 64),        # 18 pooled pixels at 32 per workgroup: ONE workgroup whatever the capacity (2 included) -- a looping
                          # workgroup needs the 96 or 15 pooled pixels of the second and third shape
]


def sid4(s):
    return "B%d_%dx%d_C%d" % tuple(s)


def window_taps(a, fill):
    """(B,H,W,C) -> (9,B,H/2,W/2,C): tap t = (ky, kx) of the 3x3 stride-2 pad-1 window, `fill` outside the image."""
    B, H, W, C = a.shape
    p = torch.full((B, H + 2, W + 2, C), fill, dtype=a.dtype)
    p[:, 1:-1, 1:-1] = a
    return torch.stack([p[:, t // 3:t // 3 + H:2, t % 3:t % 3 + W:2] for t in range(9)])


def stem_inputs(shape, dt):
    B, H, W, C = shape
    h = C // 2

    def plant(z):
        z[0, 0, 0, :h] = 3.0           # two equal positive maxima in window (0, 0) of image 0: taps 4 and 8, channels below C / 2
        z[0, 1, 1, :h] = 3.0
        z[-1, -1, -1, h:] = 3.5        # the last pixel of the last image wins its window in the other channels: the backward
                                       # sums see it (a pixel that loses its windows gets no gradient at all)
    return sign_safe(101, shape, dt, plant)


@pytest.mark.parametrize("dt", STORAGE)
@pytest.mark.parametrize("shape", STEM, ids=sid4)
def test_stem_pool(dev, shape, dt):
    """cx_bnrelu_maxpool_fwd / _bwd: pooled values, the sums of the stored values, the recorded tap checked by itself (in the
    window, attains the maximum, first in row-major order among the taps that do: the rule of F.max_pool2d), planted ties; the
    backward routed by the recorded tap.  Atomic sums and statistic rows at capacities 512, 2 and 1."""
    from chexpert_amd._lib import ptr, check, stream_ptr
    B, H, W, C = shape
    Ho, Wo, npix = H // 2, W // 2, B * (H // 2) * (W // 2)
    ldy, ldg, ldgx = C + 8, C + 16, C + 24
    natural = -(-npix // (256 // (C // 8)))
    x, sc, sh, zz = stem_inputs(shape, dt)
    xd, scd, shd = x.to(dt).to(dev), sc.to(dev), sh.to(dev)
    # the activation as the kernel forms it: one fp32 fma (x*sc + sh is exact in float64 for these operands, so its rounding to
    # fp32 is the fma's), then max(., 0)
    a32 = zz.float().clamp_min(0)
    t32, t64 = window_taps(a32, -1.0), window_taps(zz.clamp_min(0), -1.0)
    inside = window_taps(torch.ones(shape), 0.0) > 0
    mx32, mx64 = t32.max(0).values, t64.max(0).values
    order = torch.arange(9).view(9, 1, 1, 1, 1)
    first = torch.where(t32 == mx32, order, torch.full_like(order, 99)).min(0).values
    ties = int((((t32 == mx32) & inside).sum(0) >= 2)[mx32 > 0].sum())
    print("TIES %s %d of %d windows have two equal positive maxima" % (CASE, ties, npix * C))
    assert ties >= C // 2 and int(first[0, 0, 0, 0]) == 4 and bool((t32[8, 0, 0, 0, :C // 2] == mx32[0, 0, 0, :C // 2]).all())
    kept = stored(mx32, dt).double().view(npix, C)          # the pooled values as stored
    want_sum, want_sq = kept.sum(0), (kept * kept).sum(0)
    sensitive(want_sum, kept[:-1].sum(0), want_sum.abs().max().item(), "stat_sum")
    sensitive(want_sq, (kept[:-1] ** 2).sum(0), want_sq.abs().max().item(), "stat_sq")
    fwd, bwd = entry("cx_bnrelu_maxpool_fwd", dt), entry("cx_bnrelu_maxpool_bwd", dt)
    state = {}

    def launch_fwd(stats, stat_rows):
        y, am = full(dev, (npix, ldy), dt), full(dev, (npix, C), torch.uint8, 255)
        check(fwd(ptr(xd), ptr(scd), ptr(shd), ptr(y), ptr(am), ptr(stats[0]), ptr(stats[1]), B, H, W, C, ldy, stat_rows, stream_ptr()),
              "cx_bnrelu_maxpool_fwd")
        assert bool((y[:, C:] == SENT).all()), "a write into the pitch padding of y"
        state["y"] = y
        return am

    am_d = stat_runs(launch_fwd, 2, C, dev, (want_sum, want_sq), natural, (512, 2, 1), ("stat_sum", "stat_sq"))
    close_elem(state["y"][:, :C].float(), mx64.view(npix, C), dt, "pooled")
    y = full(dev, (npix, ldy), dt)                          # without statistics
    am2 = full(dev, (npix, C), torch.uint8, 255)
    check(fwd(ptr(xd), ptr(scd), ptr(shd), ptr(y), ptr(am2), None, None, B, H, W, C, ldy, 0, stream_ptr()), "cx_bnrelu_maxpool_fwd")
    assert torch.equal(y, state["y"]) and torch.equal(am2, am_d)
    am = am_d.cpu().view(B, Ho, Wo, C).long()
    assert int(am.max()) <= 8
    assert bool(inside.gather(0, am[None])[0].all()), "a recorded tap outside the image"
    at = t64.gather(0, am[None])[0]
    assert bool(((at - mx64).abs() <= mx64 * 2.0 ** -23).all()), "the recorded tap does not hold the window maximum"
    assert torch.equal(am, first), "not the first tap in row-major order among those that attain the maximum"
    # backward: dY = g*ga + gx*gb + gc goes to the recorded tap and is masked by the ReLU
    g, gx = stored(mag(111, (npix, C), 0.25, 1.0), dt), stored(mag(112, (npix, C), 0.25, 1.0), dt)
    ga, gb, gc = mag(113, (C,), 0.5, 1.5), rnd(114, (C,), -0.3, 0.3), rnd(115, (C,), -0.2, 0.2)
    mu, r = rnd(116, (C,), -0.5, 0.5), rnd(117, (C,), 0.5, 2.0)
    cg = (g.double() * ga.double() + gx.double() * gb.double() + gc.double()).view(B, Ho, Wo, C)
    route = torch.zeros(B, H + 2, W + 2, C, dtype=torch.float64)
    for t in range(9):
        route[:, t // 3:t // 3 + H:2, t % 3:t % 3 + W:2] += torch.where(am == t, cg, torch.zeros((), dtype=torch.float64))
    dz = torch.where(zz > 0, route[:, 1:-1, 1:-1], torch.zeros((), dtype=torch.float64)).reshape(-1, C)
    t2 = dz * (x.double().view(-1, C) - mu.double()) * r.double()
    S1, S2 = dz.sum(0), t2.sum(0)
    sensitive(S1, dz[:-1].sum(0), S1.abs().max().item(), "S1")
    sensitive(S2, t2[:-1].sum(0), S2.abs().max().item(), "S2")
    gd, gxd = pitched(g, ldg, dev, dt), pitched(gx, ldgx, dev, dt)
    gad, gbd, gcd, mud, rd = (t.to(dev) for t in (ga, gb, gc, mu, r))

    def launch_bwd(stats, stat_rows):
        out = full(dev, (B * H * W, C), dt)
        check(bwd(ptr(xd), ptr(scd), ptr(shd), ptr(mud), ptr(rd), ptr(am_d), ptr(gd), ptr(gxd), ptr(gad), ptr(gbd), ptr(gcd), ptr(out),
                  ptr(stats[0]), ptr(stats[1]), B, H, W, C, ldg, ldgx, stat_rows, stream_ptr()), "cx_bnrelu_maxpool_bwd")
        return out

    out = stat_runs(launch_bwd, 2, C, dev, (S1, S2), natural, (512, 2, 1), ("S1", "S2"))
    close_elem(out.float(), dz, dt, "dz")


@pytest.mark.parametrize("dt", STORAGE)
def test_stem_pool_return_codes(dev, dt):
    """C = 24 (3 chunks do not divide 256), odd H, odd W: CX_ESHAPE from both directions, nothing launched (the outputs keep
    their sentinels)."""
    from chexpert_amd._lib import ptr, stream_ptr
    fwd, bwd = entry("cx_bnrelu_maxpool_fwd", dt), entry("cx_bnrelu_maxpool_bwd", dt)
    buf, out = torch.zeros(4096, device=dev, dtype=dt), full(dev, (4096,), dt)
    v, am, st = torch.ones(256, device=dev), torch.zeros(4096, device=dev, dtype=torch.uint8), full(dev, (2, 256))
    for B, H, W, C in ((1, 4, 4, 24), (1, 3, 4, 8), (1, 4, 3, 8)):
        assert fwd(ptr(buf), ptr(v), ptr(v), ptr(out), ptr(am), ptr(st[0]), ptr(st[1]), B, H, W, C, C, 0, stream_ptr()) == CX_ESHAPE
        assert bwd(ptr(buf), ptr(v), ptr(v), ptr(v), ptr(v), ptr(am), ptr(buf), ptr(buf), ptr(v), ptr(v), ptr(v), ptr(out), ptr(st[0]),
                   ptr(st[1]), B, H, W, C, C, C, 0, stream_ptr()) == CX_ESHAPE
    assert fwd(ptr(buf), ptr(v), ptr(v), ptr(out), None, ptr(st[0]), ptr(st[1]), 1, 4, 4, 8, 8, 0, stream_ptr()) == CX_EINVAL
    assert bool((out == SENT).all()) and bool((st == SENT).all())


# ------------------------------------------------------------------------------------------------ 2. head
HEAD = [  # B, HW, C, ldx, n
    (1, 1, 8, 8, 1),
    (3, 25, 128, 192, 5),
    (5, 49, 1024, 1024, 14),      # densenet121's head
    (2, 100, 2048, 2112, 9),      # 9 classes over 4 waves: wave 0 takes three
    (17, 4, 264, 264, 3),         # B C / 8 = 561 threads in workgroups of 128; C % 256 != 0: head_bwd's tail block
]


def hid(s):
    return "B%d_HW%d_C%d_ld%d_n%d" % tuple(s)


@pytest.mark.parametrize("dt", STORAGE)
@pytest.mark.parametrize("shape", HEAD, ids=hid)
def test_head_forward_and_pool_backward(dev, shape, dt):
    """cx_head_fwd: pooled = mean relu(x*sc + sh), logits = pooled W^T (+ bias).  cx_gap_relu_bn_bwd: g = e_scale * dz with
    dz = [x*sc + sh > 0] dpooled / HW, S1 = sum dz, S2 = sum dz (x - mean) rstd; atomic sums with a pitched g, one row per image in
    rows mode, CX_ESTATROWS below B rows."""
    from chexpert_amd._lib import ptr, check, stream_ptr
    B, HW, C, ldx, n = shape
    x, sc, sh, zz = sign_safe(201, (B, HW, C), dt)
    xd, scd, shd = pitched(x.view(-1, C), ldx, dev, dt), sc.to(dev), sh.to(dev)
    w, bias = rnd(204, (n, C)) * (2.0 / C ** 0.5), rnd(205, (n,))
    wd, bd = w.to(dev), bias.to(dev)
    act = zz.clamp_min(0)
    want_p = act.mean(1)
    want_l = want_p @ w.double().t()
    sensitive(want_p[-1], act[-1, :-1].sum(0) / HW, want_p.abs().max().item(), "pooled")
    fwd = entry("cx_head_fwd", dt)
    for given in (True, False):
        pooled, logits = full(dev, (B, C)), full(dev, (B, n))
        check(fwd(ptr(xd), ptr(scd), ptr(shd), ptr(wd), ptr(bd) if given else None, ptr(pooled), ptr(logits), B, HW, C, ldx, n,
                  stream_ptr()), "cx_head_fwd")
        close(pooled, want_p, "pooled")
        close(logits, want_l + bias.double() if given else want_l, "logits" if given else "logits without bias")
    # pool backward
    dp = mag(206, (B, C), 0.25, 1.0)
    mu, r, es = rnd(207, (C,), -0.5, 0.5), rnd(208, (C,), 0.5, 2.0), mag(209, (C,), 0.5, 1.5)
    dpd, mud, rd, esd = (t.to(dev) for t in (dp, mu, r, es))
    dz = torch.where(zz > 0, (dp.double() / HW)[:, None, :], torch.zeros((), dtype=torch.float64))
    t2 = dz * (x.double() - mu.double()) * r.double()
    S1, S2 = dz.sum((0, 1)), t2.sum((0, 1))
    sensitive(S1, dz.view(-1, C)[:-1].sum(0), S1.abs().max().item(), "S1")
    sensitive(S2, t2.view(-1, C)[:-1].sum(0), S2.abs().max().item(), "S2")
    want_g = (dz * es.double()).view(-1, C)
    bwd = entry("cx_gap_relu_bn_bwd", dt)
    ldg = C + 8
    g, st = full(dev, (B * HW, ldg), dt), torch.zeros(2, C, device=dev)                # atomic sums, pitched g
    check(bwd(ptr(dpd), ptr(xd), ptr(scd), ptr(shd), ptr(mud), ptr(rd), ptr(esd), ptr(g), ptr(st[0]), ptr(st[1]), B, HW, C, ldx, ldg, 0,
              stream_ptr()), "cx_gap_relu_bn_bwd")
    assert bool((g[:, C:] == SENT).all()), "a write into the pitch padding of g"
    close_elem(g[:, :C].float(), want_g, dt, "g")
    close(st[0], S1, "S1 atomic")
    close(st[1], S2, "S2 atomic")
    outs = []
    for _ in range(2):                                      # rows mode: exactly B rows, row b = the sums of image b
        g2, rows = full(dev, (B * HW, ldg), dt), full(dev, (2, B + 3, C))
        check(bwd(ptr(dpd), ptr(xd), ptr(scd), ptr(shd), ptr(mud), ptr(rd), ptr(esd), ptr(g2), ptr(rows[0]), ptr(rows[1]), B, HW, C, ldx,
                  ldg, B + 3, stream_ptr()), "cx_gap_relu_bn_bwd")
        assert last_rows() == B and bool((rows[:, B:] == SENT).all())
        assert torch.equal(g2, g)
        outs.append(rows[:, :B].clone())
    assert torch.equal(outs[0], outs[1])
    close(outs[0][0], dz.sum(1), "S1 rows, one per image")
    close(outs[0][1], t2.sum(1), "S2 rows, one per image")
    if B > 1:
        g2, rows = full(dev, (B * HW, ldg), dt), full(dev, (2, B, C))
        assert bwd(ptr(dpd), ptr(xd), ptr(scd), ptr(shd), ptr(mud), ptr(rd), ptr(esd), ptr(g2), ptr(rows[0]), ptr(rows[1]), B, HW, C, ldx,
                   ldg, B - 1, stream_ptr()) == CX_ESTATROWS
        assert bool((g2 == SENT).all()) and bool((rows == SENT).all())


@pytest.mark.parametrize("shape", HEAD, ids=hid)
def test_head_bwd(dev, shape):
    """cx_head_bwd (fp32 operands, no twin): dW += dlogits^T pooled, db += sum_b dlogits, dpooled = dlogits W, from accumulators
    that hold something already; db = None; n > C is refused."""
    from chexpert_amd._lib import lib, ptr, check, stream_ptr
    B, _, C, _, n = shape
    dl, pooled = mag(221, (B, n), 0.25, 1.0), rnd(222, (B, C), 0.0, 1.0)
    w = rnd(223, (n, C)) * (2.0 / C ** 0.5)
    want_dw, want_db, want_dp = dl.double().t() @ pooled.double(), dl.double().sum(0), dl.double() @ w.double()
    # (the sums run over the images here: the last image left out)
    sensitive(want_dw, dl[:-1].double().t() @ pooled[:-1].double(), want_dw.abs().max().item(), "dW")
    sensitive(want_db, dl[:-1].double().sum(0), want_db.abs().max().item(), "db")
    init_w, init_b = rnd(224, (n, C)) * want_dw.abs().max().float(), rnd(225, (n,)) * want_db.abs().max().float()
    dld, pd, wd = dl.to(dev), pooled.to(dev), w.to(dev)
    for with_db in (True, False):
        dw, db, dpo = init_w.clone().to(dev), init_b.clone().to(dev), full(dev, (B, C))
        check(lib().cx_head_bwd(ptr(dld), ptr(pd), ptr(wd), ptr(dw), ptr(db) if with_db else None, ptr(dpo), B, C, n, stream_ptr()),
              "cx_head_bwd")
        close(dw.cpu() - init_w, want_dw, "dW increment")
        close(dpo, want_dp, "dpooled")
        if with_db:
            close(db.cpu() - init_b, want_db, "db increment")
        else:
            assert torch.equal(db.cpu(), init_b)
    dw, dpo = init_w.clone().to(dev), full(dev, (B, C))
    assert lib().cx_head_bwd(ptr(dld), ptr(pd), ptr(wd), ptr(dw), None, ptr(dpo), B, C, C + 1, stream_ptr()) == CX_ESHAPE
    assert torch.equal(dw.cpu(), init_w) and bool((dpo == SENT).all())


# ------------------------------------------------------------------------------------------------ 3. un-pool
UNPOOL = [  # C, (B, H, W): every width at two shapes
    (8, (1, 2, 2)), (8, (2, 8, 6)),
    (256, (2, 8, 6)), (256, (3, 4, 10)),          # 8 pixels per workgroup: natural grids 12 and 15, capacity 3 makes them loop
    (280, (1, 2, 2)), (280, (3, 4, 10)),          # 35 chunks: 7 pixels per workgroup on 245 threads, 11 idle
    (2048, (1, 2, 2)), (2048, (2, 8, 6)),         # one pixel per workgroup
]


@pytest.mark.parametrize("dt", STORAGE)
@pytest.mark.parametrize("C,bhw", UNPOOL, ids=lambda v: str(v).replace(" ", ""))
def test_unpool2_mask(dev, C, bhw, dt):
    """cx_unpool2_mask: g = e_scale * dz, dz = [x*sc + sh > 0] d[pooled pixel] / 4, S1 = sum dz, S2 = sum dz (x - mean) rstd; all three
    pitches wider than C; atomic sums and statistic rows at capacities 512 and 3."""
    from chexpert_amd._lib import ptr, check, stream_ptr
    B, H, W = bhw
    npix = B * H * W
    ldd, ldx, ldg = C + 16, C + 8, C + 24
    natural = min(2048, -(-npix // (256 // (C // 8))))
    x, sc, sh, zz = sign_safe(301, (B, H, W, C), dt)
    d = stored(mag(304, (B, H // 2, W // 2, C), 0.25, 1.0), dt)
    mu, r, es = rnd(305, (C,), -0.5, 0.5), rnd(306, (C,), 0.5, 2.0), mag(307, (C,), 0.5, 1.5)
    up = d.double().repeat_interleave(2, 1).repeat_interleave(2, 2)
    dz = torch.where(zz > 0, 0.25 * up, torch.zeros((), dtype=torch.float64)).view(-1, C)
    t2 = dz * (x.double().view(-1, C) - mu.double()) * r.double()
    S1, S2 = dz.sum(0), t2.sum(0)
    sensitive(S1, dz[:-1].sum(0), S1.abs().max().item(), "S1")
    sensitive(S2, t2[:-1].sum(0), S2.abs().max().item(), "S2")
    dd, xd = pitched(d.view(-1, C), ldd, dev, dt), pitched(x.view(-1, C), ldx, dev, dt)
    scd, shd, mud, rd, esd = (t.to(dev) for t in (sc, sh, mu, r, es))
    fn = entry("cx_unpool2_mask", dt)

    def launch(stats, stat_rows):
        g = full(dev, (npix, ldg), dt)
        check(fn(ptr(dd), ptr(xd), ptr(scd), ptr(shd), ptr(mud), ptr(rd), ptr(esd), ptr(g), ptr(stats[0]), ptr(stats[1]), B, H, W, C, ldd,
                 ldx, ldg, stat_rows, stream_ptr()), "cx_unpool2_mask")
        assert bool((g[:, C:] == SENT).all()), "a write into the pitch padding of g"
        return g

    g = stat_runs(launch, 2, C, dev, (S1, S2), natural, (512, 3), ("S1", "S2"))
    close_elem(g[:, :C].float(), dz * es.double(), dt, "g")


@pytest.mark.parametrize("dt", STORAGE)
def test_unpool2_mask_return_codes(dev, dt):
    from chexpert_amd._lib import ptr, stream_ptr
    fn = entry("cx_unpool2_mask", dt)
    buf, out, v, st = torch.zeros(8 * 2056, device=dev, dtype=dt), full(dev, (8 * 2056,), dt), torch.ones(2056, device=dev), full(dev, (2, 2056))
    for B, H, W, C in ((1, 3, 2, 8), (1, 2, 3, 8), (1, 2, 2, 2056), (1, 2, 2, 12)):
        assert fn(ptr(buf), ptr(buf), ptr(v), ptr(v), ptr(v), ptr(v), ptr(v), ptr(out), ptr(st[0]), ptr(st[1]), B, H, W, C, C, C, C, 0,
                  stream_ptr()) == CX_ESHAPE
    assert bool((out == SENT).all()) and bool((st == SENT).all())


# ------------------------------------------------------------------------------------------------ 4. residual join and its backward
JOIN = [  # rows, C
    (50, 64),         # C % 64 == 0: the blocked side-plane layout
    (333, 256),       # 32 chunks per row, 333 rows: the last workgroup is ragged
    (41, 40),         # C % 64 != 0: row-major side plane; 5 chunks: 255 threads of 256
    (77, 160),        # 20 chunks: 240 threads of 256 (WRN-28-10)
    (9, 2048),        # 256 chunks: a row per workgroup and pass
]


def side_chunk(m, cq, rows, C):
    """Byte of the sign-bit plane that holds the 8 channels of chunk cq of row m (include/chexpert_hip.h): row-major where
    C % 64 != 0, else blocks of 64 channels, [block][row][8 bytes]."""
    return m * (C // 8) + cq if C % 64 else ((cq // 8) * rows + m) * 8 + cq % 8


def decode_signs(mask, rows, C):
    m, cq = torch.arange(rows).view(-1, 1), torch.arange(C // 8).view(1, -1)
    byte = mask[side_chunk(m, cq, rows, C)].long()                      # (rows, C / 8)
    return ((byte[:, :, None] >> torch.arange(8)) & 1).view(rows, C) != 0


@pytest.mark.parametrize("dt", STORAGE)
@pytest.mark.parametrize("rows,C", JOIN, ids=lambda v: str(v))
def test_join_and_its_backward(dev, rows, C, dt):
    """cx_affine2_relu_mask: out = relu(a*pa + b*pb + pc) and its sign bits, against float64.  cx_relu_bwd_stats_mask: dz = [out > 0]
    dout (a select: exact), S1 = sum dz, S2a = sum dz (a - mu_a) r_a, S2b likewise; the sign read from `out` and from the bits, one
    and two bases, atomic sums and statistic rows."""
    from chexpert_amd._lib import ptr, check, stream_ptr
    CP = C // 8
    natural = min(2048, -(-rows * CP // 256))
    z = mag(401, (rows, C), 0.05, 2.0)
    b = stored(mag(402, (rows, C), 0.25, 1.0), dt)
    pa, pb, pc = mag(403, (C,), 0.5, 1.5), mag(404, (C,), 0.5, 1.5), rnd(405, (C,), -0.5, 0.5)
    a = stored((z - b * pb - pc) / pa, dt)
    zz = a.double() * pa.double() + b.double() * pb.double() + pc.double()
    margin = zz.abs().min().item()
    print("MARGIN %s min|a*pa+b*pb+pc| %.4f" % (CASE, margin))
    assert margin > 1e-2 and bool((pa < 0).any()) and bool((pb < 0).any())
    ad, bd, pad, pbd, pcd = a.to(dt).to(dev), b.to(dt).to(dev), pa.to(dev), pb.to(dev), pc.to(dev)
    out, bits = full(dev, (rows, C), dt), full(dev, (rows * CP + 64,), torch.uint8, 0xA5)
    check(entry("cx_affine2_relu_mask", dt)(ptr(ad), ptr(bd), ptr(pad), ptr(pbd), ptr(pcd), ptr(out), ptr(bits), rows, C, stream_ptr()),
          "cx_affine2_relu_mask")
    close_elem(out.float(), zz.clamp_min(0), dt, "out")
    assert bool((bits[rows * CP:] == 0xA5).all())
    on = zz > 0
    assert torch.equal(decode_signs(bits[:rows * CP].cpu(), rows, C), on), "sign bits"
    assert torch.equal(out.cpu() > 0, on)
    out2 = full(dev, (rows, C), dt)                         # without the bit plane
    check(entry("cx_affine2_relu_mask", dt)(ptr(ad), ptr(bd), ptr(pad), ptr(pbd), ptr(pcd), ptr(out2), None, rows, C, stream_ptr()),
          "cx_affine2_relu_mask")
    assert torch.equal(out2, out)
    # backward
    dout = stored(mag(411, (rows, C), 0.25, 1.0), dt)
    mu_a, r_a, mu_b, r_b = rnd(412, (C,), -0.5, 0.5), rnd(413, (C,), 0.5, 2.0), rnd(414, (C,), -0.5, 0.5), rnd(415, (C,), 0.5, 2.0)
    dz = torch.where(on, dout.double(), torch.zeros((), dtype=torch.float64))
    ta, tb = dz * (a.double() - mu_a.double()) * r_a.double(), dz * (b.double() - mu_b.double()) * r_b.double()
    wants = (dz.sum(0), ta.sum(0), tb.sum(0))
    for t, nm in zip((dz, ta, tb), ("S1", "S2a", "S2b")):
        sensitive(t.sum(0), t[:-1].sum(0), t.sum(0).abs().max().item(), nm)
    doutd, mad, rad, mbd, rbd = dout.to(dt).to(dev), mu_a.to(dev), r_a.to(dev), mu_b.to(dev), r_b.to(dev)
    want_dz = dz.to(dt)
    fn = entry("cx_relu_bwd_stats_mask", dt)
    for from_bits in (False, True):
        for two in (False, True):
            k = 3 if two else 2

            def launch(stats, stat_rows):
                o = full(dev, (rows, C), dt)
                check(fn(ptr(doutd), None if from_bits else ptr(out), ptr(bits) if from_bits else None, ptr(ad), ptr(mad), ptr(rad),
                         ptr(bd) if two else None, ptr(mbd) if two else None, ptr(rbd) if two else None, ptr(o), ptr(stats[0]),
                         ptr(stats[1]), ptr(stats[2]) if two else None, rows, C, stat_rows, stream_ptr()), "cx_relu_bwd_stats_mask")
                return o

            what = "%s, %s" % ("bits" if from_bits else "out", "two bases" if two else "one basis")
            o = stat_runs(launch, k, C, dev, wants[:k], natural, (512, 3), tuple(nm + " " + what for nm in ("S1", "S2a", "S2b")[:k]))
            assert torch.equal(o.cpu(), want_dz), "dz is a select of stored values (%s)" % what
    st, o = full(dev, (3, C)), full(dev, (rows, C), dt)          # two bases without a third sum: refused
    assert fn(ptr(doutd), ptr(out), None, ptr(ad), ptr(mad), ptr(rad), ptr(bd), ptr(mbd), ptr(rbd), ptr(o), ptr(st[0]), ptr(st[1]), None,
              rows, C, 0, stream_ptr()) == CX_EINVAL
    assert fn(ptr(doutd), None, None, ptr(ad), ptr(mad), ptr(rad), None, None, None, ptr(o), ptr(st[0]), ptr(st[1]), None,
              rows, C, 0, stream_ptr()) == CX_EINVAL
    assert bool((o == SENT).all()) and bool((st == SENT).all())


# ------------------------------------------------------------------------------------------------ 5. layout conversion and export
IMG = [(2, 7, 9), (3, 17, 19)]        # B H W = 126 (less than a workgroup) and 969 (four workgroups, the last ragged)


@pytest.mark.parametrize("dt", STORAGE)
@pytest.mark.parametrize("width", [4, 8])
@pytest.mark.parametrize("bhw", IMG, ids=lambda v: "%dx%dx%d" % v)
def test_nchw3_to_nhwc(dev, bhw, width, dt):
    """cx_nchw3_to_nhwc4 / cx_nchw3_to_nhwc8: the three channels moved and rounded once, the pad channels exactly zero."""
    from chexpert_amd._lib import ptr, check, stream_ptr
    B, H, W = bhw
    x = mag(501, (B, 3, H, W), 1e-3, 4.0)
    want = torch.zeros(B, H, W, width, dtype=dt)
    want[..., :3] = x.permute(0, 2, 3, 1).to(dt)
    xd, y = x.to(dev), full(dev, (B * H * W * width + 64,), dt)
    check(entry("cx_nchw3_to_nhwc%d" % width, dt)(ptr(xd), ptr(y), B, H, W, stream_ptr()), "cx_nchw3_to_nhwc%d" % width)
    assert torch.equal(y[:want.numel()].cpu().view(want.shape), want)
    assert bool((y[want.numel():] == SENT).all())


def whiten_ref(u, mean, std):
    """float64 value of u * (1 / (255 std)) - mean / std from the two fp32 constants the entry points form."""
    scale = np.float32(1.0) / (np.float32(255.0) * np.float32(std))
    shift = -np.float32(mean) / np.float32(std)
    return u.double() * float(scale) + float(shift)


@pytest.mark.parametrize("dt", STORAGE)
@pytest.mark.parametrize("width", [4, 8])
def test_u8_to_nhwc(dev, width, dt):
    """cx_u8_to_nhwc4 / cx_u8_to_nhwc8 on images holding all 256 byte values, default mean and std: fp32 within one ulp of the float64
    value, bf16 equal to its round-to-nearest-even (no byte value lies within 2^-20 of a rounding boundary: asserted); three equal
    channels, zero pad channels; npix % 16 != 0 is CX_EALIGN for the 16-pixels-per-thread bf16 form."""
    from chexpert_amd._lib import ptr, check, stream_ptr
    mean, std = 0.5330, 0.0349
    fn = entry("cx_u8_to_nhwc%d" % width, dt)
    for npix in (272, 259, 4112, 4099):
        g = torch.Generator().manual_seed(510 + npix)
        u = torch.cat([torch.arange(256), torch.randint(0, 256, (npix - 256,), generator=g)]).to(torch.uint8)
        ref = whiten_ref(u, mean, std)
        ud, y = u.to(dev), full(dev, (npix * width + 64,), dt)
        rc = fn(ptr(ud), ptr(y), npix, mean, std, stream_ptr())
        if dt == BF and width == 4 and npix % 16:
            assert rc == CX_EALIGN and bool((y == SENT).all())
            continue
        check(rc, "cx_u8_to_nhwc%d" % width)
        got = y[:npix * width].cpu().view(npix, width)
        assert bool((y[npix * width:] == SENT).all())
        assert torch.equal(got[:, 1], got[:, 0]) and torch.equal(got[:, 2], got[:, 0]) and bool((got[:, 3:] == 0).all())
        if dt == F32:
            ulp = torch.from_numpy(np.spacing(np.abs(ref.numpy()).astype(np.float32)).astype(np.float64))
            err = ((got[:, 0].double() - ref).abs() / ulp).max().item()
            print("ERR ulp %s npix %d %.3f" % (CASE, npix, err))
            assert err <= 1.0
        else:
            lo = ref.float().to(BF)                              # RNE; the fp32 step in between cannot move it:
            half = torch.ldexp(torch.ones(npix, dtype=torch.float64), torch.frexp(lo.double().abs()).exponent - 9)      # half a bf16 ulp
            near = (((ref - lo.double()).abs() - half).abs() / ref.abs()).min().item()
            print("TIE %s npix %d nearest rounding boundary %.2e away, relative" % (CASE, npix, near))
            assert near > 2.0 ** -20
            assert torch.equal(got[:, 0], lo)


def test_f32_to_bf16(dev):
    """cx_f32_to_bf16 = torch's .to(bfloat16): exact ties in both directions, negative values, signed zeros, infinities, rounding up
    across a binade, NaN (compared by isnan); n = 4096 * 256 + 3 takes the grid-stride loop's second pass."""
    from chexpert_amd._lib import lib, ptr, check, stream_ptr
    special = torch.tensor([1 + 2.0 ** -8, 1 + 3 * 2.0 ** -8, -(1 + 2.0 ** -8), -(1 + 3 * 2.0 ** -8), 0.0, -0.0, float("inf"), -float("inf"),
                            2 - 2.0 ** -9, -(2 - 2.0 ** -9), 255.5, 1 + 2.0 ** -8 + 2.0 ** -20, 1 + 2.0 ** -8 - 2.0 ** -20, NAN, 3.0e38, 1e-30])
    for n in (1, 7, 1023, 4096 * 256 + 3):
        x = mag(520, (n,), 1e-3, 100.0)
        m = min(n, special.numel())
        x[:m] = special[:m]
        if n > 4096 * 256:
            x[-3:] = special[:3]                                 # in the second pass too
        xd, y = x.to(dev), full(dev, (n + 64,), BF)
        check(lib().cx_f32_to_bf16(ptr(xd), ptr(y), n, stream_ptr()), "cx_f32_to_bf16")
        got, want = y[:n].cpu(), x.to(BF)
        nan = torch.isnan(want)
        assert torch.equal(torch.isnan(got), nan)
        assert torch.equal(got.view(torch.int16)[~nan], want.view(torch.int16)[~nan])      # bits: -0 is not +0
        assert bool((y[n:] == SENT).all())
    assert float(special[:2].to(BF)[0]) == 1.0 and float(special[:2].to(BF)[1]) == 1 + 2.0 ** -6      # the ties go to even


@pytest.mark.parametrize("shape", [(2, 3, 5, 8, 16), (3, 7, 9, 40, 48), (1, 2, 2, 520, 528)], ids=lambda s: "B%d_%dx%d_C%d_ld%d" % s)
def test_export_to_f32_nchw(dev, shape):
    """cx_bf16_to_f32_nchw: a move; cx_affine_to_f32_nchw: one fp32 fma (exact in float64 for bf16 x, so its rounding to fp32 is the
    fma's) and an optional ReLU, or a move without scale / shift.  Pitched bf16 input, B H W C not a multiple of 256."""
    from chexpert_amd._lib import lib, ptr, check, stream_ptr
    B, H, W, C, ldx = shape
    x = bf(mag(530, (B, H, W, C), 0.05, 2.0))
    sc, sh = mag(531, (C,), 0.5, 1.5), rnd(532, (C,), -0.5, 0.5)
    xd, scd, shd = pitched(x.view(-1, C), ldx, dev, BF), sc.to(dev), sh.to(dev)
    nchw = lambda t: t.permute(0, 3, 1, 2).contiguous()
    n = x.numel()
    y = full(dev, (n + 64,))
    check(lib().cx_bf16_to_f32_nchw(ptr(xd), ptr(y), B, H, W, C, ldx, stream_ptr()), "cx_bf16_to_f32_nchw")
    assert torch.equal(y[:n].cpu().view(B, C, H, W), nchw(x)) and bool((y[n:] == SENT).all())
    fma = (x.double() * sc.double() + sh.double()).float()
    for relu in (0, 1):
        for affine in (True, False):
            y = full(dev, (n + 64,))
            check(lib().cx_affine_to_f32_nchw(ptr(xd), ptr(scd) if affine else None, ptr(shd) if affine else None, relu, ptr(y), B, H, W, C,
                                              ldx, stream_ptr()), "cx_affine_to_f32_nchw")
            want = fma if affine else x
            assert torch.equal(y[:n].cpu().view(B, C, H, W), nchw(want.clamp_min(0) if relu else want)), "relu %d affine %d" % (relu, affine)
            assert bool((y[n:] == SENT).all())
    assert lib().cx_affine_to_f32_nchw(ptr(xd), ptr(scd), None, 0, ptr(y), B, H, W, C, ldx, stream_ptr()) == CX_EINVAL


@pytest.mark.parametrize("inner_relu", [1, 0])
@pytest.mark.parametrize("C", [8, 512, 520, 1024])
def test_gradcam_map(dev, C, inner_relu):
    """cx_gradcam_map: cam = relu(sum_c w[c] f(x*sc + sh)), f = ReLU or the identity; 520 channels: lane 0 takes a second stride;
    21 pixels: the last workgroup has one of its four waves at work."""
    from chexpert_amd._lib import lib, ptr, check, stream_ptr
    B, HW, ldx = 3, 7, C + 8
    x, sc, sh, zz = sign_safe(540, (B, HW, C), BF)
    w = rnd(543, (C,)) * (2.0 / C ** 0.5)
    f = zz.clamp_min(0) if inner_relu else zz
    pre = f @ w.double()
    want = pre.clamp_min(0)
    assert bool((pre > 0).any()) and bool((pre < 0).any())
    # the sum over channels with the last channel left out: the condition of the reduction tests, for a channel sum
    sensitive(pre, f[..., :-1] @ w.double()[:-1], pre.abs().max().item(), "cam")
    xd, scd, shd, wd, cam = pitched(x.view(-1, C), ldx, dev, BF), sc.to(dev), sh.to(dev), w.to(dev), full(dev, (B * HW + 64,))
    check(lib().cx_gradcam_map(ptr(xd), ptr(scd), ptr(shd), ptr(wd), ptr(cam), B, HW, C, ldx, inner_relu, stream_ptr()), "cx_gradcam_map")
    close(cam[:B * HW], want.view(-1), "cam")
    assert bool((cam[B * HW:] == SENT).all())


# ------------------------------------------------------------------------------------------------ 6. dropout slice
DROP = [  # B, H, W, C, ld, first column of the slice in the wider buffer
    (2, 3, 5, 32, 96, 32),
    (1, 4, 4, 8, 8, 0),
    (3, 2, 2, 280, 288, 8),       # 35 chunks: 245 threads of 256; 420 chunks = 2 workgroups, capacity 1 makes one loop
    (1, 1, 2, 2048, 2048, 0),     # 512 chunks = 2 workgroups
]
BIG_SEED = (1 << 40) + 12345


@pytest.mark.parametrize("dt", STORAGE)
@pytest.mark.parametrize("p", [0.2, 0.5])
@pytest.mark.parametrize("shape", DROP, ids=lambda s: "B%d_%dx%d_C%d_ld%d_at%d" % s)
def test_dropout_slice(dev, shape, p, dt):
    """cx_dropout_slice_fwd: y = keep ? rnd(y * 1/(1-p)) : 0 in place on a channel slice, the keep decisions of oracle.nets.drop_keep
    (seed above 2^32, two layer ids); the neighbouring columns untouched; statistic rows = the sums of the stored result, at
    capacities 512 and 1.  cx_dropout_slice_bwd: g = keep ? (qa g + qb x + qc) / (1-p) : 0 with the same decisions."""
    from chexpert_amd._lib import ptr, check, stream_ptr
    from oracle import nets
    B, H, W, C, ld, c0 = shape
    rows, CP = B * H * W, C // 8
    natural = min(2048, -(-rows * CP // 256))
    seed = torch.tensor([BIG_SEED], dtype=torch.int64, device=dev)
    scale = torch.tensor(np.float32(1.0) / (np.float32(1.0) - np.float32(p)))           # as the entry point forms it
    wide = stored(mag(601, (rows, ld), 0.5, 2.0), dt)
    fwd, bwd = entry("cx_dropout_slice_fwd", dt), entry("cx_dropout_slice_bwd", dt)
    seen = []
    for uid in (3, 17):
        keep = nets.drop_keep(BIG_SEED, uid, (B, H, W, C), float(np.float32(p))).view(rows, C)       # p as the entry point's float holds it
        frac = keep.float().mean().item()
        print("KEEP %s uid %d kept %.3f" % (CASE, uid, frac))
        assert abs(frac - (1 - p)) < 0.2 and not any(torch.equal(keep, k) for k in seen)
        seen.append(keep)
        want = wide.clone()
        want[:, c0:c0 + C] = torch.where(keep, stored(wide[:, c0:c0 + C] * scale, dt), torch.zeros(()))
        kept = want[:, c0:c0 + C].double()
        S1, S2 = kept.sum(0), (kept * kept).sum(0)
        sensitive(S1, kept[:-1].sum(0), S1.abs().max().item(), "S1")
        sensitive(S2, (kept[:-1] ** 2).sum(0), S2.abs().max().item(), "S2")
        for cap in (512, 1):
            outs = []
            for _ in range(2):
                buf, st = wide.to(dt).to(dev), full(dev, (2, cap, C))
                check(fwd(ptr(buf[:, c0:]), ld, rows, C, p, ptr(seed), uid, ptr(st[0]), ptr(st[1]), cap, stream_ptr()), "cx_dropout_slice_fwd")
                n = last_rows()
                assert n == min(cap, natural) and bool((st[:, n:] == SENT).all())
                assert torch.equal(buf.cpu(), want.to(dt)), "slice or its neighbours"
                outs.append(st[:, :n].clone())
            assert torch.equal(outs[0], outs[1])
            close(outs[0][0].sum(0), S1, "S1 of %d rows" % n)
            close(outs[0][1].sum(0), S2, "S2 of %d rows" % n)
        buf = wide.to(dt).to(dev)                               # without statistics
        check(fwd(ptr(buf[:, c0:]), ld, rows, C, p, ptr(seed), uid, None, None, 0, stream_ptr()), "cx_dropout_slice_fwd")
        assert torch.equal(buf.cpu(), want.to(dt))
        # backward
        ldx = C + 8
        x = stored(mag(602, (rows, C), 0.5, 2.0), dt)
        qa, qb, qc = mag(603, (C,), 0.5, 1.5), rnd(604, (C,), -0.3, 0.3), rnd(605, (C,), -0.2, 0.2)
        lin = (qa.double() * wide[:, c0:c0 + C].double() + qb.double() * x.double() + qc.double()) / (1.0 - float(np.float32(p)))
        buf, xd, qad, qbd, qcd = wide.to(dt).to(dev), pitched(x, ldx, dev, dt), qa.to(dev), qb.to(dev), qc.to(dev)
        check(bwd(ptr(buf[:, c0:]), ld, ptr(xd), ldx, ptr(qad), ptr(qbd), ptr(qcd), rows, C, p, ptr(seed), uid, stream_ptr()),
              "cx_dropout_slice_bwd")
        got = buf.cpu()
        close_elem(got[:, c0:c0 + C].float(), torch.where(keep, lin, torch.zeros((), dtype=torch.float64)), dt, "g uid %d" % uid)
        assert bool((got[:, c0:c0 + C][~keep] == 0).all())
        got[:, c0:c0 + C] = 0
        rest = wide.clone()
        rest[:, c0:c0 + C] = 0
        assert torch.equal(got, rest.to(dt)), "the neighbours of the gradient slice"
    buf = wide.to(dt).to(dev)
    for bad in (0.0, 1.0):
        assert fwd(ptr(buf[:, c0:]), ld, rows, C, bad, ptr(seed), 3, None, None, 0, stream_ptr()) == CX_EINVAL
    assert torch.equal(buf.cpu(), wide.to(dt))


# ------------------------------------------------------------------------------------------------ 7. weight tables
def device_table(descs):
    arr = (type(descs[0]) * len(descs))(*descs)
    return torch.frombuffer(bytearray(bytes(arr)), dtype=torch.uint8)


PACK = [  # O, I, kh, kw, transpose, stem
    (32, 24, 1, 1, 0, 0),
    (16, 16, 3, 3, 0, 0),
    (32, 8, 3, 3, 1, 0),
    (5, 7, 3, 3, 0, 0),           # O I = 35: less than one workgroup
    (16, 3, 7, 7, 0, 1),          # the stem
]


def packed_ref(w, transpose, stem, dt):
    """The layouts the kernel comments state.  Plain: [tap][o][i]; transposed: [tap'][i][o] with the taps rotated by 180 degrees;
    stem, bf16: [ky][o][32] with k = 4 (kx + 1) + channel, zero for k < 4 and channel 3; stem, fp32: [49 taps][o][4], channel 3 zero."""
    O, I, kh, kw = w.shape
    taps = kh * kw
    if stem and dt == BF:
        t = torch.zeros(7, O, 8, 4)
        t[:, :, 1:, :3] = w.permute(2, 0, 3, 1)
        return t.reshape(-1).to(dt)
    if stem:
        t = torch.zeros(49, O, 4)
        t[:, :, :3] = w.reshape(O, 3, 49).permute(2, 0, 1)
        return t.reshape(-1)
    v = w.reshape(O, I, taps)
    return (v.flip(2).permute(2, 1, 0) if transpose else v.permute(2, 0, 1)).reshape(-1).to(dt)


@pytest.mark.parametrize("dt", STORAGE)
def test_pack_weights_table(dev, dt):
    """cx_pack_weights_table: five descriptors in one launch at odd offsets with sentinel gaps between the destinations; bf16: the
    bits of cx_pack_weights per tensor and of the permutation written in torch; fp32: the stated layouts, values moved."""
    from chexpert_amd._lib import lib, ptr, check, stream_ptr, CxPackDesc
    ws = [mag(700 + i, (O, I, kh, kw), 1e-3, 2.0) for i, (O, I, kh, kw, _, _) in enumerate(PACK)]
    refs = [packed_ref(w, s[4], s[5], dt) for w, s in zip(ws, PACK)]
    src, dst, descs, so, do = [], [], [], 3, 5
    for w, s, ref in zip(ws, PACK, refs):
        src.append(so)
        dst.append(do)
        descs.append(CxPackDesc(so, do, *s))
        so += w.numel() + 11
        do += ref.numel() + 13
    flat = torch.full((so,), NAN)
    for w, o in zip(ws, src):
        flat[o:o + w.numel()] = w.reshape(-1)
    want = torch.full((do,), SENT, dtype=dt)
    for ref, o in zip(refs, dst):
        want[o:o + ref.numel()] = ref
    flatd, packed, tab = flat.to(dev), full(dev, (do,), dt), device_table(descs).to(dev)
    check(entry("cx_pack_weights_table", dt)(ptr(flatd), ptr(packed), ptr(tab), len(descs), stream_ptr()), "cx_pack_weights_table")
    assert torch.equal(packed.cpu(), want)
    if dt == BF:
        for w, s, ref in zip(ws, PACK, refs):
            wd, one = w.to(dev), full(dev, (ref.numel() + 16,), BF)
            check(lib().cx_pack_weights(ptr(wd), ptr(one), *s, stream_ptr()), "cx_pack_weights")
            assert torch.equal(one[:ref.numel()].cpu(), ref) and bool((one[ref.numel():] == SENT).all())


def chan_pos(j, d):
    if j < d.c0r:
        return j if j < d.split else j + d.shift
    return d.c0p + ((j - d.c0r) // d.k) * d.kp + (j - d.c0r) % d.k


def test_chan_map_table(dev):
    """cx_chan_map_table: a dense-layer descriptor (24 first channels, then layers of growth 12 written 16 wide, 3x3 taps) and one
    with split / shift (an attention transition's [conv | pad | attention] output).  Direction 0 stores and leaves the positions no
    real element maps to untouched; direction 1 stores or adds; 0 then 1 is the identity."""
    from chexpert_amd._lib import lib, ptr, check, stream_ptr, CxChanMapDesc
    descs = [CxChanMapDesc(7, 5, 4, 9, 60, 72, 24, 24, 12, 16, 24, 0),      # real_off, pad_off, O, taps, Ireal, Ipad, c0r, c0p, k, kp, split, shift
             CxChanMapDesc(7 + 4 * 60 * 9 + 3, 5 + 4 * 72 * 9 + 6, 3, 1, 32, 40, 20, 24, 12, 16, 12, 4)]
    n_real, n_pad = descs[1].real_off + 3 * 32 + 9, descs[1].pad_off + 3 * 40 + 9
    real = mag(720, (n_real,), 0.5, 2.0)
    index = torch.full((n_real,), -1, dtype=torch.long)                    # real element -> padded element
    for d in descs:
        for o in range(d.O):
            for j in range(d.Ireal):
                for t in range(d.taps):
                    index[d.real_off + (o * d.Ireal + j) * d.taps + t] = d.pad_off + (o * d.Ipad + chan_pos(j, d)) * d.taps + t
    mapped = index >= 0
    assert int(mapped.sum()) == 4 * 60 * 9 + 3 * 32 and index[mapped].unique().numel() == int(mapped.sum())
    tab = device_table(descs).to(dev)
    fn = lib().cx_chan_map_table
    want_pad = torch.full((n_pad,), SENT)
    want_pad[index[mapped]] = real[mapped]
    reald, padded = real.to(dev), full(dev, (n_pad,))
    check(fn(ptr(reald), ptr(padded), ptr(tab), 2, 0, 0, stream_ptr()), "cx_chan_map_table")
    assert torch.equal(padded.cpu(), want_pad) and torch.equal(reald.cpu(), real)
    assert int((want_pad == SENT).sum()) == n_pad - int(mapped.sum())      # the unmapped positions kept their content
    back = full(dev, (n_real,))                                           # 0 then 1: the identity on the mapped elements
    check(fn(ptr(back), ptr(padded), ptr(tab), 2, 1, 0, stream_ptr()), "cx_chan_map_table")
    assert torch.equal(back.cpu(), torch.where(mapped, real, torch.full((), SENT)))
    pad2 = mag(721, (n_pad,), 0.5, 2.0)
    pad2d = pad2.to(dev)
    for accumulate in (0, 1):
        r2 = real.clone().to(dev)
        check(fn(ptr(r2), ptr(pad2d), ptr(tab), 2, 1, accumulate, stream_ptr()), "cx_chan_map_table")
        want = real.clone()
        want[mapped] = (real[mapped] + pad2[index[mapped]]) if accumulate else pad2[index[mapped]]
        assert torch.equal(r2.cpu(), want), "direction 1, accumulate %d" % accumulate
    assert fn(ptr(reald), ptr(padded), ptr(tab), 2, 2, 0, stream_ptr()) == CX_EINVAL


# ------------------------------------------------------------------------------------------------ 8. BatchNorm coefficient edges
def coef_close(got, want, what, rel):
    err = (got.double().cpu() - want.double()).abs().max().item() / want.abs().max().item()
    print("ERR coef %s %s %.3e" % (CASE, what, err))
    assert err <= rel, "%s: %.3e" % (what, err)


@pytest.mark.parametrize("affine", [True, False], ids=["gamma_beta", "plain"])
@pytest.mark.parametrize("replicas", [63, 64, 65, 257])
def test_bn_coef_edges(dev, replicas, affine):
    """cx_bn_coef at C = 40 (the last 16-channel group is half empty), replicas at the boundaries of the four-in-flight loop of the
    row reduction, row pitch C + 8 (NaN in the padding), a constant channel (the variance clamps at 0: rstd = 1/sqrt(eps)), with
    and without gamma / beta.  Bound: 2e-6 of the abs-max (test_coefficient_kernels_over_many_rows), the constant channel apart --
    its rstd of 316 would otherwise set the scale for all."""
    from chexpert_amd._lib import lib, ptr, check, stream_ptr
    C, ld, const, eps = 40, 48, 21, 1e-5
    n = 4.0 * replicas
    part = torch.full((2, replicas, ld), NAN)
    part[0, :, :C] = rnd(800, (replicas, C), 0.0, 1.0)
    part[1, :, :C] = part[0, :, :C] ** 2 + 5.0
    part[0, :, const], part[1, :, const] = 2.0, 1.0          # four samples of 0.5 per row: sum 2, sum of squares 1, exactly
    gamma, beta = mag(801, (C,), 0.5, 1.5), rnd(802, (C,), -0.5, 0.5)
    rm, rv = rnd(803, (C,)), rnd(804, (C,), 0.5, 1.5)
    S = part[:, :, :C].double().sum(1)
    mean = S[0] / n
    var = (S[1] / n - mean ** 2).clamp_min(0)
    assert var[const].item() == 0.0 and mean[const].item() == 0.5
    rstd = 1 / torch.sqrt(var + eps)
    gm, bt = (gamma.double(), beta.double()) if affine else (torch.ones(C, dtype=torch.float64), torch.zeros(C, dtype=torch.float64))
    pd, rmd, rvd = part.to(dev), rm.clone().to(dev), rv.clone().to(dev)
    gd, btd, out = gamma.to(dev), beta.to(dev), full(dev, (4, C + 8))
    check(lib().cx_bn_coef(ptr(pd[0]), ptr(pd[1]), n, ptr(gd) if affine else None, ptr(btd) if affine else None, eps, 0.1,
                           ptr(rmd), ptr(rvd), ptr(out[0]), ptr(out[1]), ptr(out[2]), ptr(out[3]), C, replicas, ld, stream_ptr()), "cx_bn_coef")
    assert bool((out[:, C:] == SENT).all()), "a write behind channel C"
    rest = torch.arange(C) != const
    for got, want, what in ((out[0, :C], gm * rstd, "scale"), (out[1, :C], bt - mean * gm * rstd, "shift"), (out[2, :C], mean, "mean"),
                            (out[3, :C], rstd, "rstd"), (rmd, 0.9 * rm + 0.1 * mean, "running_mean"),
                            (rvd, 0.9 * rv + 0.1 * var * n / (n - 1), "running_var")):
        coef_close(got[rest], want[rest], what, 2e-6)
        coef_close(got[~rest], want[~rest], what + " of the constant channel", 2e-6)
    assert abs(out[3, const].item() - eps ** -0.5) <= 2e-6 * eps ** -0.5


def test_bn_coef_single_sample(dev):
    """cx_bn_coef with count = 1 (one replica): the variance is 0 up to the rounding of x^2 and clamps, and the running variance
    takes the biased value (there is no n / (n - 1) for one sample)."""
    from chexpert_amd._lib import lib, ptr, check, stream_ptr
    C, eps = 40, 1e-5
    x = mag(810, (C,), 0.5, 2.0)
    sq = x * x
    rm, rv = rnd(811, (C,)), rnd(812, (C,), 0.5, 1.5)
    var = (sq.double() - x.double() ** 2).clamp_min(0)
    rstd = 1 / torch.sqrt(var + eps)
    rmd, rvd, out = rm.clone().to(dev), rv.clone().to(dev), full(dev, (4, C + 8))
    xd, sqd = x.to(dev), sq.to(dev)
    check(lib().cx_bn_coef(ptr(xd), ptr(sqd), 1.0, None, None, eps, 0.1, ptr(rmd), ptr(rvd), ptr(out[0]), ptr(out[1]), ptr(out[2]),
                           ptr(out[3]), C, 1, 0, stream_ptr()), "cx_bn_coef")
    assert bool((out[:, C:] == SENT).all())
    for got, want, what in ((out[0, :C], rstd, "scale"), (out[1, :C], -x.double() * rstd, "shift"), (out[2, :C], x, "mean"),
                            (out[3, :C], rstd, "rstd"), (rmd, 0.9 * rm + 0.1 * x, "running_mean"), (rvd, 0.9 * rv + 0.1 * var, "running_var")):
        coef_close(got, want, what, 2e-6)
    assert float(rvd.max()) < 0.9 * 1.5 + 1e-3              # nothing like an unbiased variance of one sample (a division by 0)


def test_bn_coef_moments_fresh_range(dev):
    """cx_bn_coef_moments at C = 56 with the fresh range [13, 35): it starts and ends inside a 16-channel group and covers the one in
    between; the fourth group has no fresh channel and takes the other path.  Bound: 4e-6 (as above)."""
    from chexpert_amd._lib import lib, ptr, check, stream_ptr
    C, lo, cn, rows, ld, n, eps = 56, 13, 22, 33, 24, 300.0, 1e-5
    gamma, beta = mag(820, (C,), 0.5, 1.5), rnd(821, (C,), -0.5, 0.5)
    rm, rv = rnd(822, (C,)), rnd(823, (C,), 0.5, 1.5)
    m0, r0 = rnd(824, (C,)), rnd(825, (C,), 0.5, 2.0)
    fr = torch.full((2, rows, ld), NAN)
    fr[0, :, :cn] = rnd(826, (rows, cn), 0.0, 1.0)
    fr[1, :, :cn] = fr[0, :, :cn] ** 2 + 3.0
    Sf = fr[:, :, :cn].double().sum(1)
    mf = Sf[0] / n
    vf = Sf[1] / n - mf ** 2
    m_ref, r_ref = m0.double().clone(), r0.double().clone()
    m_ref[lo:lo + cn], r_ref[lo:lo + cn] = mf, 1 / torch.sqrt(vf + eps)
    frd, gd, btd = fr.to(dev), gamma.to(dev), beta.to(dev)
    buf = full(dev, (6, C + 8))
    buf[0, :C], buf[1, :C], buf[2, :C], buf[3, :C] = m0.to(dev), r0.to(dev), rm.to(dev), rv.to(dev)
    check(lib().cx_bn_coef_moments(ptr(buf[0]), ptr(buf[1]), n, ptr(gd), ptr(btd), eps, 0.1, ptr(buf[2]), ptr(buf[3]),
                                   ptr(buf[4]), ptr(buf[5]), C, ptr(frd[0]), ptr(frd[1]), rows, ld, lo, cn, stream_ptr()), "cx_bn_coef_moments")
    assert bool((buf[:, C:] == SENT).all())
    stale = torch.ones(C, dtype=torch.bool)
    stale[lo:lo + cn] = False
    assert torch.equal(buf[0, :C].cpu()[stale], m0[stale]) and torch.equal(buf[1, :C].cpu()[stale], r0[stale])
    g64, b64 = gamma.double(), beta.double()
    for got, want, what in ((buf[0], m_ref, "mean"), (buf[1], r_ref, "rstd"), (buf[4], g64 * r_ref, "scale"),
                            (buf[5], b64 - m_ref * g64 * r_ref, "shift"), (buf[2], 0.9 * rm + 0.1 * m_ref, "running_mean"),
                            (buf[3], 0.9 * rv + 0.1 * (1 / r_ref ** 2 - eps) * n / (n - 1), "running_var")):
        coef_close(got[:C], want, what, 4e-6)
