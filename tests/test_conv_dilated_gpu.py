"""GPU: the generic implicit-GEMM kernels that carry every dilated or grouped 3x3 convolution -- conv_gemm_kernel (csrc/conv_gemm.hip:
forward and input gradient), wgrad_kernel (csrc/conv_wgrad.hip), conv_f32_kernel / wgrad_f32_kernel (csrc/conv_f32.hip) -- through
ops.conv_gemm / ops.conv_wgrad against the CPU float64 references of tests/conv_dilated_cases.py, in both storage types:

  CxConv.dil / CxWgrad.dil by themselves, with stride = 2 and with tstride = 2 (the input gradient of a strided dilated convolution:
  taps two pixels apart on the stride grid), at map borders, on maps smaller than the tap extent, with ragged pixel / channel
  tiles and partial K steps; the per-group launches of a grouped 3x3 on channel slices with their statistic rows side by side at
  the pitch of the whole BatchNorm; impulse and small-integer runs that must match bit for bit.

Every operand is a channel slice of a wider buffer (NaN next to the inputs, a sentinel next to the outputs).  Each check prints an
ERR line (measured error relative to max|want|) before it asserts the bound the project already holds for that output kind."""
import pytest
import torch

import conv_dilated_cases as cd
from conv_dilated_cases import BF16, CASES, EXACT, F32, GROUPED, TOL, cid

pytestmark = pytest.mark.gpu

STORAGE = [pytest.param(BF16, id="bf16"), pytest.param(F32, id="f32")]
SENT = -3.0
XOFF, YOFF = 8, 16                      # first channel of an input / output slice inside its buffer (multiples of 8)


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    from chexpert_amd import _lib
    _lib.lib()
    return torch.device("cuda:0")


@pytest.fixture
def slabs(dev, monkeypatch):
    """slabs(True): the weight-gradient launches that follow leave their partial sums in the slab arena (to be deferred);
    slabs(False): fp32 atomics.  A small arena of this test's own; afterwards the process has the one it had before."""
    from chexpert_amd import ops
    from chexpert_amd._lib import lib
    saved = ops._arenas.pop(dev.index, None)
    lib().cx_wgrad_defer(-1)
    monkeypatch.setattr(ops._WgradArena, "START", 4 << 20)
    monkeypatch.setattr(ops._WgradArena, "MIN_FREE", 1 << 20)

    def mode(on):
        monkeypatch.setattr(ops, "WGRAD_SCRATCH_FLOATS", (16 << 20) if on else 0)
    yield mode
    torch.cuda.synchronize()
    lib().cx_wgrad_defer(-1)
    ops._arenas.pop(dev.index, None)
    if saved is not None:
        ops._arenas[dev.index] = saved


def tdt(dt):
    return torch.bfloat16 if dt == BF16 else torch.float32


def put(t, dt, dev, off, fill, extra=24):
    """NCHW float64 -> (buffer, view): the tensor as channels [off, off + C) of a wider NHWC buffer of the storage type."""
    B, Cc, H, W = t.shape
    buf = torch.full((B, H, W, off + Cc + extra), fill, dtype=tdt(dt), device=dev)
    buf[..., off:off + Cc] = t.permute(0, 2, 3, 1).to(tdt(dt)).to(dev)
    return buf, buf[..., off:off + Cc]


def empty_out(c_shape, dt, dev, off=YOFF, extra=24):
    B, Cc, H, W = c_shape
    buf = torch.full((B, H, W, off + Cc + extra), SENT, dtype=tdt(dt), device=dev)
    return buf, buf[..., off:off + Cc]


def nchw(view):
    return view.double().cpu().permute(0, 3, 1, 2).contiguous()


def outside_untouched(buf, off, Cc):
    """the channels of `buf` next to the slice [off, off + Cc) still hold the sentinel"""
    return bool((buf[..., :off] == SENT).all()) and bool((buf[..., off + Cc:] == SENT).all())


def vec(t, dev):
    return t.float().to(dev)


def pack(w, dt, dev, transpose=False):
    """The forward OIHW weight packed for the storage type: [tap][O][I], or for the input gradient [rotated tap][I][O]."""
    from chexpert_amd import ops
    if dt == BF16:
        return ops.pack_weights(w.float().contiguous().to(dev), transpose=transpose)
    O, I, kh, kw = w.shape                 # the fp32 layout, as test_fp32_gpu.py restates it
    if not transpose:
        return w.float().permute(2, 3, 0, 1).reshape(kh * kw, O, I).contiguous().to(dev)
    return w.float().flip(2, 3).permute(2, 3, 1, 0).reshape(kh * kw, I, O).contiguous().to(dev)


def close(got, want, rel, what, tag):
    err = (got.double() - want).abs().max().item() / (want.abs().max().item() + 1e-300)
    print("ERR %s %s %.3e (bound %.0e)" % (tag, what, err, rel))
    assert err <= rel, "%s %s: rel err %.3e > %.0e" % (tag, what, err, rel)


def fwd_tag(dt, n):
    return "conv_gemm_kernel<%d, " % cd.gemm_bn(n) if dt == BF16 else "conv_f32_kernel<"


def wgrad_tag(dt, n):
    return "wgrad_kernel<%d, %d, " % cd.wgrad_tile(n) if dt == BF16 else "wgrad_f32_kernel<"


def pixel_tiles(c, forward=True):
    m = c.B * (c.Ho * c.Wo if forward else c.H * c.W)
    return (m + 127) // 128               # both kernel families walk 128 output pixels per workgroup


# ------------------------------------------------------------------------------------------------ forward
@pytest.mark.parametrize("dt", STORAGE)
@pytest.mark.parametrize("c", CASES, ids=cid)
def test_forward(dev, c, dt):
    """y = conv(a, w), stride s, pad = dil = d, a = x and a = relu(x*pa + pb); the statistic rows (one per pixel tile) sum to the
    sums of the stored output, rows past the returned count stay 0, nothing is written next to the slice."""
    from chexpert_amd import ops
    d, r, tol = cd.data(c, dt), cd.refs(c, dt), TOL[dt]
    _, xv = put(d.x, dt, dev, XOFF, float("nan"))
    wp = pack(d.w, dt, dev)
    for pro, want in ((0, r.y_plain), (1, r.y_pro)):
        tag = "%s %s fwd pro%d" % (dt, cid(c), pro)
        buf, yv = empty_out(want.shape, dt, dev)
        cap = pixel_tiles(c) + 3
        st = torch.zeros(2, cap, c.N, device=dev)
        kw = dict(prologue=ops.PRO_AFFINE_RELU, pa=vec(d.pa, dev), pb=vec(d.pb, dev)) if pro else {}
        rows = ops.conv_gemm(xv, wp, yv, N=c.N, kh=3, kw=3, stride=c.stride, pad=c.dil, dil=c.dil, stat_sum=st[0], stat_sq=st[1],
                             stat_det=True, stat_replicas=cap, stat_rstride=c.N, **kw)
        assert ops.last_kernel().startswith(fwd_tag(dt, c.N)), ops.last_kernel()
        assert rows == pixel_tiles(c)
        got = nchw(yv)
        close(got, want, tol["y"], "y", tag)
        assert outside_untouched(buf, YOFF, c.N), "wrote outside the slice"
        close(st[0, :rows].double().sum(0).cpu(), got.sum((0, 2, 3)), tol["sums"], "sum", tag)
        close(st[1, :rows].double().sum(0).cpu(), (got * got).sum((0, 2, 3)), tol["sums"], "sum of squares", tag)
        assert (st[:, rows:] == 0).all(), "statistic rows past the returned count"


# ------------------------------------------------------------------------------------------------ input gradient
@pytest.mark.parametrize("dt", STORAGE)
@pytest.mark.parametrize("c", CASES, ids=cid)
def test_input_gradient(dev, c, dt):
    """dx of the same convolution: transposed weights, pad = dil = d, tstride = s.  Stored plainly into a sentinel-filled buffer
    (under stride 2 the pixels off the stride grid must come out as written zeros), then with the BN-backward prologue and the
    mask epilogue accumulating onto an old value, with S1 / S2."""
    from chexpert_amd import ops
    d, r, tol = cd.data(c, dt), cd.refs(c, dt), TOL[dt]
    wt = pack(d.w, dt, dev, transpose=True)
    _, uv = put(d.u, dt, dev, XOFF, float("nan"))
    _, vv = put(d.v, dt, dev, YOFF, float("nan"))
    geo = dict(N=c.K, kh=3, kw=3, pad=c.dil, dil=c.dil, tstride=c.stride)
    # plain store
    tag = "%s %s dgrad store" % (dt, cid(c))
    buf, ov = empty_out(d.x.shape, dt, dev)
    ops.conv_gemm(uv, wt, ov, epilogue=ops.EPI_STORE, **geo)
    assert ops.last_kernel().startswith(fwd_tag(dt, c.K)), ops.last_kernel()
    got = nchw(ov)
    close(got, r.dx_plain, tol["y"], "dx", tag)
    if c.stride == 2:
        assert (got[:, :, 1::2] == 0).all() and (got[:, :, :, 1::2] == 0).all(), "a pixel no tap reaches is not a written zero"
    assert outside_untouched(buf, YOFF, c.K), "wrote outside the slice"
    # BN backward in the prologue, mask epilogue, accumulating
    tag = "%s %s dgrad mask" % (dt, cid(c))
    buf = torch.full((c.B, c.H, c.W, YOFF + c.K + 24), SENT, dtype=tdt(dt), device=dev)
    ov = buf[..., YOFF:YOFF + c.K]
    ov.copy_(d.old.permute(0, 2, 3, 1).to(tdt(dt)))
    _, exv = put(d.ex, dt, dev, XOFF, float("nan"))
    cap = pixel_tiles(c, forward=False) + 3
    st = torch.zeros(2, cap, c.K, device=dev)
    rows = ops.conv_gemm(uv, wt, ov, prologue=ops.PRO_AFFINE2, x2=vv, pa=vec(d.ga, dev), pb=vec(d.gb, dev), pc=vec(d.gc, dev),
                         epilogue=ops.EPI_MASK, ex=exv, e_sc=vec(d.e_sc, dev), e_sh=vec(d.e_sh, dev), e_mu=vec(d.e_mu, dev),
                         e_r=vec(d.e_r, dev), e_scale=vec(d.e_scale, dev), stat_sum=st[0], stat_sq=st[1], stat_det=True,
                         stat_replicas=cap, stat_rstride=c.K, accumulate=True, **geo)
    assert ops.last_kernel().startswith(fwd_tag(dt, c.K)), ops.last_kernel()
    assert rows == pixel_tiles(c, forward=False)
    close(nchw(ov), r.g, tol["g"], "g", tag)
    assert outside_untouched(buf, YOFF, c.K), "wrote outside the slice"
    close(st[0, :rows].double().sum(0).cpu(), r.S1, tol["S"], "S1", tag)
    close(st[1, :rows].double().sum(0).cpu(), r.S2, tol["S"], "S2", tag)
    assert (st[:, rows:] == 0).all(), "statistic rows past the returned count"


# ------------------------------------------------------------------------------------------------ weight gradient
def run_wgrad(ops, dev, slabs, use_slabs, dw, launch, strict=True):
    """One weight-gradient launch (or the launches of all groups) through the slab arena, deferred and flushed, or through atomics.
    strict: the generic kernels, which take the slab path whenever they are offered a workspace."""
    from chexpert_amd._lib import lib
    slabs(use_slabs)
    if use_slabs:
        assert ops.wgrad_defer_begin(dev)
    floats = launch(dw)
    if use_slabs:
        assert not strict or all(f > 0 for f in floats), "the launch did not take the slab path"
        ops.wgrad_defer_flush(dev)
        assert lib().cx_wgrad_defer(0) == 0
    else:
        assert all(f == 0 for f in floats), "the launch did not take the atomic path"
    return dw


@pytest.mark.parametrize("dt", STORAGE)
@pytest.mark.parametrize("c", CASES, ids=cid)
def test_weight_gradient(dev, slabs, c, dt):
    """dW += sum over output pixels of G (x) A at stride s, pad = dil = d: plain operands and (BN backward, BN + ReLU) prologues,
    the library's pixel split and three ranges, partial sums through slabs (deferred) and through atomics."""
    from chexpert_amd import ops
    from chexpert_amd._lib import lib
    d, r, tol = cd.data(c, dt), cd.refs(c, dt), TOL[dt]
    _, gv = put(d.u, dt, dev, XOFF, float("nan"))
    _, g2v = put(d.v, dt, dev, YOFF, float("nan"))
    _, xv = put(d.x, dt, dev, YOFF, float("nan"))
    pros = dict(g_prologue=ops.PRO_AFFINE2, g2=g2v, ga=vec(d.ga, dev), gb=vec(d.gb, dev), gc=vec(d.gc, dev),
                x_prologue=ops.PRO_AFFINE_RELU, pa=vec(d.pa, dev), pb=vec(d.pb, dev))
    dw0 = d.dw0.float()
    for pro, want in ((0, r.dw_plain), (1, r.dw_pro)):
        for splits in (0, 3):
            for use_slabs in (True, False):
                tag = "%s %s wgrad pro%d splits%d %s" % (dt, cid(c), pro, splits, "slabs" if use_slabs else "atomics")

                def launch(dw):
                    ops.conv_wgrad(gv, xv, dw, kh=3, kw=3, stride=c.stride, pad=c.dil, dil=c.dil, splits=splits, **(pros if pro else {}))
                    assert ops.last_kernel().startswith(wgrad_tag(dt, c.N)), ops.last_kernel()
                    return [lib().cx_last_slab_floats()]
                dw = run_wgrad(ops, dev, slabs, use_slabs, dw0.clone().to(dev), launch).cpu()
                close(dw.double() - dw0.double(), want, tol["dw"], "dW", tag)
                if c.dil == 4:               # H = 4: the kernel rows ky = 0 and ky = 2 read only padding
                    assert torch.equal(dw[:, :, [0, 2], :], dw0[:, :, [0, 2], :]), "%s: a tap of padding only is not exactly 0" % tag


# ------------------------------------------------------------------------------------------------ grouped 3x3, one launch per group
@pytest.mark.parametrize("dt", STORAGE)
@pytest.mark.parametrize("c", GROUPED, ids=cid)
def test_grouped_as_the_engine_launches_it(dev, slabs, c, dt):
    """groups = 4: one launch per group on x[..., g*kg:(g+1)*kg] -> y[..., same] with the weights of the group's rows; statistic
    buffers offset by g*kg at the row pitch of the whole width; dw = the group's row range of one OIHW gradient.  Forward, input
    gradient and weight gradient against the groups = 4 float64 reference; the statistic rows of all groups are summed once."""
    from chexpert_amd import ops
    from chexpert_amd._lib import lib
    d, r, tol = cd.data(c, dt), cd.refs(c, dt), TOL[dt]
    Cw, kg, gr = c.K, c.K // c.groups, c.groups
    sl = [slice(g * kg, (g + 1) * kg) for g in range(gr)]
    pa, pb = vec(d.pa, dev), vec(d.pb, dev)
    cap = 64                            # (dil = 1: a tiled kernel with statistic rows of its own may take the call)
    tags = set()
    # forward, BN + ReLU prologue
    tag = "%s %s grouped fwd" % (dt, cid(c))
    _, xv = put(d.x, dt, dev, XOFF, float("nan"))
    buf, yv = empty_out(r.y_pro.shape, dt, dev)
    st = torch.zeros(2, cap * Cw, device=dev)
    for g, s_ in enumerate(sl):
        rows = ops.conv_gemm(xv[..., s_], pack(d.w[s_], dt, dev), yv[..., s_], N=kg, kh=3, kw=3, stride=1, pad=c.dil, dil=c.dil,
                             prologue=ops.PRO_AFFINE_RELU, pa=pa[s_], pb=pb[s_], stat_sum=st[0, g * kg:], stat_sq=st[1, g * kg:],
                             stat_det=True, stat_replicas=cap, stat_rstride=Cw)
        tags.add(ops.last_kernel())
        assert c.dil == 1 or ops.last_kernel().startswith(fwd_tag(dt, kg)), ops.last_kernel()
    got = nchw(yv)
    close(got, r.y_pro, tol["y"], "y", tag)
    assert outside_untouched(buf, YOFF, Cw), "wrote outside the slice"
    st = st.view(2, cap, Cw)
    close(st[0, :rows].double().sum(0).cpu(), got.sum((0, 2, 3)), tol["sums"], "sum", tag)
    close(st[1, :rows].double().sum(0).cpu(), (got * got).sum((0, 2, 3)), tol["sums"], "sum of squares", tag)
    assert (st[:, rows:] == 0).all()
    # input gradient, BN backward prologue + mask epilogue, accumulating
    tag = "%s %s grouped dgrad" % (dt, cid(c))
    _, uv = put(d.u, dt, dev, XOFF, float("nan"))
    _, vv = put(d.v, dt, dev, YOFF, float("nan"))
    _, exv = put(d.ex, dt, dev, XOFF, float("nan"))
    buf = torch.full((c.B, c.H, c.W, YOFF + Cw + 24), SENT, dtype=tdt(dt), device=dev)
    ov = buf[..., YOFF:YOFF + Cw]
    ov.copy_(d.old.permute(0, 2, 3, 1).to(tdt(dt)))
    ga, gb, gc = vec(d.ga, dev), vec(d.gb, dev), vec(d.gc, dev)
    e = {k: vec(getattr(d, k), dev) for k in ("e_sc", "e_sh", "e_mu", "e_r", "e_scale")}
    st = torch.zeros(2, cap * Cw, device=dev)
    for g, s_ in enumerate(sl):
        rows = ops.conv_gemm(uv[..., s_], pack(d.w[s_], dt, dev, transpose=True), ov[..., s_], N=kg, kh=3, kw=3, pad=c.dil, dil=c.dil,
                             tstride=1, prologue=ops.PRO_AFFINE2, x2=vv[..., s_], pa=ga[s_], pb=gb[s_], pc=gc[s_], epilogue=ops.EPI_MASK,
                             ex=exv[..., s_], accumulate=True, stat_sum=st[0, g * kg:], stat_sq=st[1, g * kg:], stat_det=True,
                             stat_replicas=cap, stat_rstride=Cw, **{k: t[s_] for k, t in e.items()})
        tags.add(ops.last_kernel())
        assert c.dil == 1 or ops.last_kernel().startswith(fwd_tag(dt, kg)), ops.last_kernel()
    close(nchw(ov), r.g, tol["g"], "g", tag)
    assert outside_untouched(buf, YOFF, Cw), "wrote outside the slice"
    st = st.view(2, cap, Cw)
    close(st[0, :rows].double().sum(0).cpu(), r.S1, tol["S"], "S1", tag)
    close(st[1, :rows].double().sum(0).cpu(), r.S2, tol["S"], "S2", tag)
    assert (st[:, rows:] == 0).all()
    # weight gradient: the row range of each group of one (C, kg, 3, 3) gradient
    _, xv2 = put(d.x, dt, dev, YOFF, float("nan"))
    dw0 = d.dw0.float()
    for use_slabs in (True, False):
        tag = "%s %s grouped wgrad %s" % (dt, cid(c), "slabs" if use_slabs else "atomics")

        def launch(dw):
            floats = []
            for g, s_ in enumerate(sl):
                ops.conv_wgrad(uv[..., s_], xv2[..., s_], dw[s_], kh=3, kw=3, stride=1, pad=c.dil, dil=c.dil, g_prologue=ops.PRO_AFFINE2,
                               g2=vv[..., s_], ga=ga[s_], gb=gb[s_], gc=gc[s_], x_prologue=ops.PRO_AFFINE_RELU, pa=pa[s_], pb=pb[s_])
                tags.add(ops.last_kernel())
                assert c.dil == 1 or ops.last_kernel().startswith(wgrad_tag(dt, kg)), ops.last_kernel()
                floats.append(lib().cx_last_slab_floats())
            return floats
        dw = run_wgrad(ops, dev, slabs, use_slabs, dw0.clone().to(dev), launch, strict=c.dil > 1).cpu()
        close(dw.double() - dw0.double(), r.dw_pro, tol["dw"], "dW", tag)
    print("KERNELS %s %s %s" % (dt, cid(c), sorted(tags)))


# ------------------------------------------------------------------------------------------------ exact runs
@pytest.mark.parametrize("dt", STORAGE)
@pytest.mark.parametrize("c", EXACT, ids=cid)
def test_impulses_and_small_integers_bit_for_bit(dev, slabs, c, dt):
    """One impulse per image (four corners and the centre, distinct channels) through integer weights that tell every tap apart:
    the forward output and the input gradient equal the reference, which catches a misplaced, mirrored or un-rotated tap
    outright.  The weight gradient of operands from {-2..2}: integer sums below 2^24, exact in any order, slabs or atomics."""
    from chexpert_amd import ops
    from chexpert_amd._lib import lib
    e = cd.exact(c)
    # forward
    _, xv = put(e.x, dt, dev, XOFF, float("nan"))
    buf, yv = empty_out(e.y.shape, dt, dev)
    ops.conv_gemm(xv, pack(e.w, dt, dev), yv, N=c.N, kh=3, kw=3, stride=c.stride, pad=c.dil, dil=c.dil)
    assert ops.last_kernel().startswith(fwd_tag(dt, c.N)), ops.last_kernel()
    assert torch.equal(nchw(yv), e.y), "forward: %d values differ" % (nchw(yv) != e.y).sum().item()
    assert outside_untouched(buf, YOFF, c.N)
    # input gradient of an impulse gradient, stored into a sentinel-filled buffer
    _, uv = put(e.u, dt, dev, XOFF, float("nan"))
    buf, ov = empty_out(e.x.shape, dt, dev)
    ops.conv_gemm(uv, pack(e.w, dt, dev, transpose=True), ov, N=c.K, kh=3, kw=3, pad=c.dil, dil=c.dil, tstride=c.stride)
    assert ops.last_kernel().startswith(fwd_tag(dt, c.K)), ops.last_kernel()
    assert torch.equal(nchw(ov), e.dx), "input gradient: %d values differ" % (nchw(ov) != e.dx).sum().item()
    assert outside_untouched(buf, YOFF, c.K)
    # weight gradient
    _, gv = put(e.gi, dt, dev, XOFF, float("nan"))
    _, xiv = put(e.xi, dt, dev, YOFF, float("nan"))
    for splits in (0, 3):
        for use_slabs in (True, False):
            def launch(dw):
                ops.conv_wgrad(gv, xiv, dw, kh=3, kw=3, stride=c.stride, pad=c.dil, dil=c.dil, splits=splits)
                assert ops.last_kernel().startswith(wgrad_tag(dt, c.N)), ops.last_kernel()
                return [lib().cx_last_slab_floats()]
            dw = run_wgrad(ops, dev, slabs, use_slabs, torch.zeros(c.N, c.K, 3, 3, device=dev), launch).cpu()
            assert torch.equal(dw.double(), e.dw), "dW (splits %d, %s): %d values differ" % (
                splits, "slabs" if use_slabs else "atomics", (dw.double() != e.dw).sum().item())
