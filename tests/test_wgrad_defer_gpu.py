"""GPU: the deferred weight-gradient sums of a backward pass (ops.wgrad_defer_begin / _flush / _abort, ops._WgradArena,
cx_wgrad_defer, cx_dw_reduce_table) on their own.

  1. cx_dw_reduce_table over hand-built descriptor tables against `ordered_sum`, the fp32 restatement of dw_reduce_body's
     association (tests/test_wgrad_defer_cpu.py), bit for bit, with sentinels around every destination.
  2. Every launcher that reaches cx_dw_reduce / cx_dw_reduce_ld: the deferred sums give the bits of the immediate slab mode, and
     both match the reference of the launcher's own kernel test at that test's bound (operands, reference and bound are restated
     from tests/test_kernels_gpu.py, test_dwconv_gpu.py, test_effnet_glue_gpu.py, test_aaconv_gpu.py and test_fp32_gpu.py).
  3. The arena: a launch reports the floats it used and writes nothing past them, the overflow fallback, the repeatable table,
     flush(keep=True), abort, the 1024-descriptor limit.
  4. One training step of each engine with and without deferral: the same bits in every parameter gradient.

Two deferred launches into the SAME dw within one pass are out of scope (the arena paragraph): the engines never do it.
"""
import ctypes as C

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from chexpert_amd import synth
from test_wgrad_defer_cpu import ordered_sum

pytestmark = pytest.mark.gpu

CX_EINVAL = -1
SENT_BITS = 0x7FC0DEAD                 # a quiet NaN no sum produces: whatever adds to it, or stores a number over it, shows
SENT = -12345.0


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    from chexpert_amd import _lib
    _lib.lib()
    return torch.device("cuda:0")


@pytest.fixture
def arena(dev, monkeypatch):
    """Slab workspace on and no arena yet for this device: arena(start, min_free) sizes the one the test's first wgrad_defer_begin
    allocates.  Afterwards deferral is off on both sides and the arena the process had before is back."""
    from chexpert_amd import ops
    from chexpert_amd._lib import lib
    monkeypatch.setattr(ops, "WGRAD_SCRATCH_FLOATS", 16 << 20)
    saved = ops._arenas.pop(dev.index, None)
    lib().cx_wgrad_defer(-1)

    def size(start, min_free):
        monkeypatch.setattr(ops._WgradArena, "START", start)
        monkeypatch.setattr(ops._WgradArena, "MIN_FREE", min_free)
    yield size
    torch.cuda.synchronize()
    lib().cx_wgrad_defer(-1)
    ops._arenas.pop(dev.index, None)
    if saved is not None:
        ops._arenas[dev.index] = saved


def bf(t):
    return t.to(torch.bfloat16).float()


def rnd(seed, shape, lo=-1.0, hi=1.0):
    return synth.uniform(seed, shape, lo, hi)


def trnd(seed, shape, lo=-1.0, hi=1.0):            # the generator of test_dwconv_gpu.py / test_effnet_glue_gpu.py
    g = torch.Generator().manual_seed(seed)
    return torch.rand(shape, generator=g) * (hi - lo) + lo


def nhwc_buf(seed, B, H, W, C, dev, lo=-1.5, hi=1.5):
    """bf16 NHWC buffer on the GPU + its fp32 NCHW value on the CPU."""
    v = bf(rnd(seed, (B, H, W, C), lo, hi))
    return v.to(torch.bfloat16).to(dev), v.permute(0, 3, 1, 2).contiguous()


def swish(z):
    return z * torch.sigmoid(z)


def bits(t):
    return t.contiguous().view(torch.int32)


def same(a, b):
    return torch.equal(bits(a), bits(b))


def close(got, want, rel, what):
    got, want = got.double().cpu(), want.double().cpu()
    scale = want.abs().max().item() + 1e-12
    err = (got - want).abs().max().item()
    print("%s: max err %.3e of scale %.3e (rel %.2e, bound %.0e)" % (what, err, scale, err / scale, rel))
    assert err <= rel * scale, "%s: max err %.3e vs scale %.3e (rel %.2e > %.0e)" % (what, err, scale, err / scale, rel)


def slab_floats():
    from chexpert_amd._lib import lib
    return lib().cx_last_slab_floats()


def up64(n):
    return (n + 63) // 64 * 64


# ------------------------------------------------------------------------------------------------ 1. the table kernel
def _vec_rule(dw_addr, slab_addr, total, cols, dw_ld):
    """cx_dw_reduce_ld's choice of the four-floats-per-lane body."""
    return total % 4 == 0 and dw_addr % 16 == 0 and slab_addr % 16 == 0 and cols % 4 == 0 and dw_ld % 4 == 0


class _Table:
    """Destinations inside one sentinel-filled buffer, slabs in another, the descriptor table as cx_wgrad_defer_take lays it out."""

    def __init__(self, dev, seed):
        self.dev, self.rng = dev, np.random.default_rng(seed)
        self.dst_n, self.slab_n, self.specs = 64, 0, []

    def add(self, total, splits, *, shift=0, cols=0, dw_ld=0, vec):
        """shift: floats by which the destination leaves its 16-byte alignment; cols / dw_ld: a [total / cols][cols] tile that goes
        to rows of pitch dw_ld.  `vec` is what the rule must give for this layout (asserted once the addresses are known)."""
        rows = total // cols if cols else 1
        span = (rows - 1) * dw_ld + cols if cols else total
        off = self.dst_n + shift
        self.dst_n = up64(off + span) + 64                       # at least 64 sentinel floats between two destinations
        soff = self.slab_n
        self.slab_n = up64(soff + splits * total) + 64
        self.specs.append(dict(total=total, splits=splits, cols=cols, dw_ld=dw_ld, vec=vec, off=off, soff=soff, span=span))

    def run(self, picks=None):
        from chexpert_amd import _lib as L
        specs = self.specs if picks is None else [self.specs[i] for i in picks]
        dst0 = np.full(self.dst_n, SENT, np.float32)
        slab = self.rng.uniform(-1.0, 1.0, self.slab_n).astype(np.float32)
        want = dst0.copy()
        for s in specs:
            idx = np.arange(s["total"])
            if s["cols"]:
                idx = idx // s["cols"] * s["dw_ld"] + idx % s["cols"]
            idx = idx + s["off"]
            dst0[idx] = self.rng.uniform(-1.0, 1.0, s["total"]).astype(np.float32)        # a gradient is already there
            want[idx] = ordered_sum(slab[s["soff"]:s["soff"] + s["splits"] * s["total"]].reshape(s["splits"], s["total"]), dst0[idx])
            if s["cols"]:
                assert (want[s["off"]:s["off"] + s["span"]] == SENT).sum() == s["span"] - s["total"]      # the pitch gaps
        dst, slabd = torch.from_numpy(dst0).to(self.dev), torch.from_numpy(slab).to(self.dev)
        arr = (L.CxReduceDesc * len(specs))()
        blocks = 0
        for d, s in zip(arr, specs):
            d.dw, d.slab = dst.data_ptr() + 4 * s["off"], slabd.data_ptr() + 4 * s["soff"]
            assert _vec_rule(d.dw, d.slab, s["total"], s["cols"], s["dw_ld"]) == s["vec"], s
            d.total, d.splits, d.vec, d.cols, d.dw_ld = s["total"], s["splits"], int(s["vec"]), s["cols"], s["dw_ld"]
            d.first_block = blocks                               # cx_wgrad_defer_take: 32 units of 4 floats (vec) or of one per block
            units = s["total"] // 4 if s["vec"] else s["total"]
            blocks += (units + 31) // 32
        tab = torch.frombuffer(bytearray(bytes(arr)), dtype=torch.uint8).to(self.dev)
        L.check(L.lib().cx_dw_reduce_table(L.ptr(tab), len(specs), blocks, L.stream_ptr()), "cx_dw_reduce_table")
        torch.cuda.synchronize()
        return dst.cpu().numpy(), want, [d.first_block for d in arr] + [blocks]


def test_table_sums_equal_the_restatement_bit_for_bit(dev):
    """Nine descriptors in one launch: both bodies, contiguous and column-slice destinations, totals of 1 and 4, partial last
    blocks, splits 1 / 7 / 8 / 9 (empty lanes) / 61, a one-block descriptor between two many-block ones; then n = 1."""
    from chexpert_amd import _lib as L
    t = _Table(dev, 20)
    t.add(4000, 61, vec=True)                              # 1000 units: 32 blocks, the last holds 8 units
    t.add(1, 9, vec=False)                                 # one block between two many-block descriptors; lanes 5..7 empty
    t.add(2052, 1, vec=True)                               # 513 units: 17 blocks, the last holds one unit
    t.add(111, 7, vec=False)                               # total % 4 != 0
    t.add(256, 8, shift=1, vec=False)                      # the destination is one float off its alignment
    t.add(160, 9, cols=32, dw_ld=96, vec=True)             # five rows of a 32-column slice, two blocks
    t.add(210, 1, cols=30, dw_ld=50, vec=False)            # a slice whose width is no multiple of four
    t.add(4, 8, vec=True)
    t.add(1001, 61, vec=False)                             # 32 blocks, the last holds 9 floats
    assert sorted({s["splits"] for s in t.specs}) == [1, 7, 8, 9, 61]
    got, want, first = t.run()
    assert first == [0, 32, 33, 50, 54, 62, 64, 71, 72, 104]
    for s in t.specs:
        sl = slice(s["off"], s["off"] + s["span"])
        assert np.array_equal(got[sl].view(np.int32), want[sl].view(np.int32)), "destination of %s" % s
    assert np.array_equal(got.view(np.int32), want.view(np.int32)), "a sentinel between the destinations changed"
    for pick in (8, 5, 1):                                 # a table of one
        got, want, first = t.run([pick])
        assert np.array_equal(got.view(np.int32), want.view(np.int32)), "n = 1, descriptor %d" % pick
    # what the entry point refuses before it launches
    tab = torch.zeros(64, dtype=torch.uint8, device=dev)
    lib = L.lib()
    assert lib.cx_dw_reduce_table(None, 1, 1, L.stream_ptr()) == CX_EINVAL
    assert lib.cx_dw_reduce_table(L.ptr(tab), 1, 0, L.stream_ptr()) == CX_EINVAL
    assert lib.cx_dw_reduce_table(L.ptr(tab), 1, -3, L.stream_ptr()) == CX_EINVAL
    assert lib.cx_dw_reduce_table(None, 0, 0, L.stream_ptr()) == 0
    torch.cuda.synchronize()


# ------------------------------------------------------------------------------------------------ 2. the producers
class Case:
    """One launcher: launch(dws) adds its weight gradient(s) into the tensors of `dws` (clones of dw0), want[i] is the reference of
    dws[i] - dw0[i] (None: the rest of a wider matrix, which stays as it is), rel the bound of the launcher's own kernel test."""

    def __init__(self, launch, dw0, want, rel, family, unit=None):
        self.launch, self.dw0, self.want, self.rel = launch, dw0, want, rel
        self.family = family                   # what ops.last_kernel() starts with (None: the launcher sets no tag)
        self.unit = unit                       # slab floats per pixel split (None: not a plain splits x total slab)
        self.imm = None                        # the immediate slab mode's result, filled by the first test that needs it


def _conv_case(dev, ksz, K, N, gpro, xpro, B, H, W, family, stride=1, hint=None):
    """test_kernels_gpu.py::test_wgrad: slices of wider buffers, dY = g*ga + g2*gb + gc, A = relu(x*pa + pb), bound 2e-3."""
    from chexpert_amd import ops
    pad = ksz // 2
    Ho, Wo = (H + 2 * pad - ksz) // stride + 1, (W + 2 * pad - ksz) // stride + 1
    gb_, g = nhwc_buf(40, B, Ho, Wo, N + 32, dev)
    g2b, g2 = nhwc_buf(41, B, Ho, Wo, N, dev)
    xb, x = nhwc_buf(42, B, H, W, K + 64, dev)
    ga, gbv, gc = rnd(43, (N,), 0.5, 1.5), rnd(44, (N,), -0.3, 0.3), rnd(45, (N,), -0.2, 0.2)
    pa, pb = rnd(46, (K,), -0.3, 1.5), rnd(47, (K,), -0.5, 0.5)
    cv = lambda t: t.view(1, -1, 1, 1)
    G = bf(g[:, :N] * cv(ga) + g2 * cv(gbv) + cv(gc)) if gpro else g[:, :N]
    A = bf(F.relu(x[:, :K] * cv(pa) + cv(pb))) if xpro else x[:, :K]
    want = torch.nn.grad.conv2d_weight(A, (N, K, ksz, ksz), G, stride=stride, padding=pad)
    dw0 = rnd(48, (N, K, ksz, ksz), -1, 1).to(dev)
    kw = dict(kh=ksz, kw=ksz, stride=stride, pad=pad, g_prologue=gpro, g2=g2b if gpro else None, ga=ga.to(dev), gb=gbv.to(dev),
              gc=gc.to(dev), x_prologue=xpro, pa=pa.to(dev), pb=pb.to(dev), hint=hint)
    return Case(lambda dws: ops.conv_wgrad(gb_[..., :N], xb[..., :K], dws[0], **kw), [dw0], [want], 2e-3, family, unit=N * K * ksz * ksz)


def _pool2_case(dev):
    """test_kernels_gpu.py::test_wgrad_pool2_and_stem, the transition: 48 pooled pixels, two pixel splits."""
    from chexpert_amd import ops
    B, H, W, K, N = 2, 8, 12, 64, 128
    xb, x = nhwc_buf(50, B, H, W, K, dev)
    gb_, g = nhwc_buf(51, B, H // 2, W // 2, N, dev)
    pa, pb = rnd(52, (K,), -0.3, 1.5), rnd(53, (K,), -0.5, 0.5)
    cv = lambda t: t.view(1, -1, 1, 1)
    A = bf(F.avg_pool2d(F.relu(x * cv(pa) + cv(pb)), 2, 2))
    want = torch.nn.grad.conv2d_weight(A, (N, K, 1, 1), g)
    pad_, pbd = pa.to(dev), pb.to(dev)
    dw0 = rnd(56, (N, K, 1, 1), -1, 1).to(dev)
    return Case(lambda dws: ops.conv_wgrad(gb_, xb, dws[0], mode=ops.MODE_POOL2, x_prologue=ops.PRO_AFFINE_RELU, pa=pad_, pb=pbd),
                [dw0], [want], 2e-3, "wgrad_kernel<", unit=N * K)


def _stem_case(dev):
    """test_kernels_gpu.py::test_wgrad_pool2_and_stem, the stem: 384 output pixels, twelve steps of 32."""
    from chexpert_amd import ops
    B, Hs, Ws = 2, 24, 32
    xs = bf(rnd(54, (B, 3, Hs, Ws), -2, 2))
    gsb, gs = nhwc_buf(55, B, Hs // 2, Ws // 2, 64, dev)
    want = torch.nn.grad.conv2d_weight(xs, (64, 3, 7, 7), gs, stride=2, padding=3)
    x4 = ops.nchw3_to_nhwc4(xs.to(dev))
    dw0 = rnd(57, (64, 3, 7, 7), -1, 1).to(dev)
    return Case(lambda dws: ops.conv_wgrad(gsb, x4, dws[0], mode=ops.MODE_STEM), [dw0], [want], 2e-3, "stem_wgrad_kernel<", unit=64 * 147)


def _fused_case(dev, pro, acc, B, H, W, N, family):
    """test_kernels_gpu.py::test_fused_1x1_dgrad_wgrad_equals_separate_kernels, the weight gradient (bound 3e-3)."""
    from chexpert_amd import ops
    K = 128
    ub, u = nhwc_buf(120, B, H, W, K, dev)
    vb, v = nhwc_buf(121, B, H, W, K, dev)
    exb, ex = nhwc_buf(122, B, H, W, N + 8, dev)
    oldb, old = nhwc_buf(123, B, H, W, N + 8, dev)
    w = bf(rnd(124, (K, N, 1, 1), -0.1, 0.1))
    pa, pb, pc = rnd(125, (K,), 0.5, 1.5), rnd(126, (K,), -0.3, 0.3), rnd(127, (K,), -0.2, 0.2)
    e = [rnd(128 + i, (N,), lo, hi) for i, (lo, hi) in enumerate([(-0.3, 1.5), (-0.5, 0.5), (-0.5, 0.5), (0.5, 2.0), (-0.3, 1.5)])]
    cv = lambda t: t.view(1, -1, 1, 1)
    dy = bf(u * cv(pa) + v * cv(pb) + cv(pc)) if pro == 2 else u
    pre = ex[:, :N] * cv(e[0]) + cv(e[1])
    want = torch.nn.grad.conv2d_weight(bf(F.relu(pre)), (K, N, 1, 1), dy)
    wp = ops.pack_weights(w.to(dev), transpose=True)
    ed = [t.to(dev) for t in e]
    kw = dict(prologue=ops.PRO_AFFINE2, x2=vb, pa=pa.to(dev), pb=pb.to(dev), pc=pc.to(dev)) if pro == 2 else {}
    R = 4

    def launch(dws):
        st, g = torch.zeros(2, R, N, device=dev), oldb.clone()
        ops.conv_gemm(ub, wp, g[..., :N], N=N, epilogue=ops.EPI_MASK, ex=exb[..., :N], e_sc=ed[0], e_sh=ed[1], e_mu=ed[2], e_r=ed[3],
                      e_scale=ed[4], stat_sum=st[0], stat_sq=st[1], accumulate=acc, stat_replicas=R, stat_rstride=N, fused_dw=dws[0], **kw)
    return Case(launch, [rnd(133, (K, N, 1, 1), -1, 1).to(dev)], [want], 3e-3, family, unit=K * N)


def _pair_case(dev):
    """test_kernels_gpu.py::test_fused_1x1_backward_of_two_layers_equals_two_passes at (2, 9, 10, 96): three 64-pixel tiles, the
    later layer's gradient a column range of a (128, N + 32) matrix.  The reference is that test's: the single-layer kernel run
    twice, to fp32 summation order (1e-5)."""
    from chexpert_amd import ops
    B, H, W, N, K = 2, 9, 10, 96, 128
    NA = N + 32
    exb, _ = nhwc_buf(500, B, H, W, N + 40, dev)
    oldb, _ = nhwc_buf(501, B, H, W, N + 40, dev)
    lay = []
    for i in range(2):
        n_in = NA if i == 0 else N
        ub, _ = nhwc_buf(510 + i, B, H, W, K, dev)
        vb, _ = nhwc_buf(520 + i, B, H, W, K, dev)
        w = bf(rnd(530 + i, (K, n_in, 1, 1), -0.1, 0.1)).to(dev)
        wp = ops.pack_weights(w, transpose=True)[:N * K]
        vec = lambda s, lo, hi: rnd(s + i, (n_in,), lo, hi).to(dev)[:N].contiguous()
        kw = dict(N=N, epilogue=ops.EPI_MASK, ex=exb[..., :N], e_sc=vec(540, -0.3, 1.5), e_sh=vec(550, -0.5, 0.5), e_mu=vec(560, -0.5, 0.5),
                  e_r=vec(570, 0.5, 2.0), e_scale=vec(580, -0.3, 1.5), accumulate=True, prologue=ops.PRO_AFFINE2, x2=vb,
                  pa=rnd(590 + i, (K,), 0.5, 1.5).to(dev), pb=rnd(600 + i, (K,), -0.3, 0.3).to(dev), pc=rnd(610 + i, (K,), -0.2, 0.2).to(dev))
        lay.append((ub, wp, kw))
    R = 4

    def run(dws, pair):
        g = oldb.clone()
        args = []
        for i in range(2):
            st = torch.zeros(2, R, N, device=dev)
            args.append((lay[i][0], lay[i][1], g[..., :N], dict(lay[i][2], stat_sum=st[0], stat_sq=st[1], stat_replicas=R, stat_rstride=N)))
        if pair:
            ops.conv1x1_bwd_pair(args[0], args[1], dws[0][:, :N], dws[1])
        else:
            for i in range(2):
                ops.conv_gemm(args[i][0], args[i][1], args[i][2], fused_dw=dws[i][:, :N], **args[i][3])
    dw0 = [rnd(620, (K, NA), -1, 1).to(dev), rnd(621, (K, N), -1, 1).to(dev)]
    two = [t.clone() for t in dw0]
    run(two, False)
    want = [a - b for a, b in zip(two, dw0)]                  # (columns N.. of the wider matrix: zero, i.e. untouched)
    return Case(lambda dws: run(dws, True), dw0, want, 1e-5, "pw_bwd2p_kernel<", unit=2 * K * N)


def _batch_case(dev, n=3):
    """test_kernels_gpu.py::test_conv3x3_wgrad_batch_equals_per_layer at (4, 10, 10): bottleneck tensors as slices of wider buffers."""
    from chexpert_amd import ops
    B, H, W = 4, 10, 10
    items, wants, dw0 = [], [], []
    for i in range(n):
        gb_, g = nhwc_buf(300 + i, B, H, W, 32, dev)
        buf = bf(rnd(320 + i, (B, H, W, 160), -1.5, 1.5)).to(torch.bfloat16).to(dev)
        xb = buf[..., 16:144]
        x = xb.float().cpu().permute(0, 3, 1, 2).contiguous()
        pa, pb = rnd(340 + i, (128,), -0.3, 1.5), rnd(360 + i, (128,), -0.5, 0.5)
        cv = lambda t: t.view(1, -1, 1, 1)
        wants.append(torch.nn.grad.conv2d_weight(bf(F.relu(x * cv(pa) + cv(pb))), (32, 128, 3, 3), g, padding=1))
        dw0.append(rnd(380 + i, (32, 128, 3, 3), -1, 1).to(dev))
        items.append((gb_, xb, pa.to(dev), pb.to(dev)))

    def launch(dws):
        assert ops.conv3x3_wgrad_batch([it + (dw,) for it, dw in zip(items, dws)]), "the library declined a dense-layer shape"
    return Case(launch, dw0, wants, 2e-3, "conv3x3_strip_wgrad_batch_kernel<", unit=n * 32 * 128 * 9)


def _aa_case(dev):
    """test_aaconv_gpu.py::test_out_projection_forward_backward, the backward at dv = 8: 126 pixels, two workgroups of 64."""
    from chexpert_amd import ops
    B, H, W, dv = 3, 6, 7, 8
    o = synth.uniform(1, (B, H * W, dv), -1.0, 1.0)
    w = synth.uniform(2, (dv, dv, 1, 1), -0.3, 0.3)
    g, gx = bf(synth.uniform(3, (B, H, W, dv), -1, 1)), bf(synth.uniform(4, (B, H, W, dv), -1, 1))
    ga, gb, gc = synth.uniform(5, (dv,), 0.5, 1.5), synth.uniform(6, (dv,), -0.5, 0.5), synth.uniform(7, (dv,), -0.2, 0.2)
    dY = (g * ga + gx * gb + gc).view(B, H * W, dv)
    want = torch.einsum("bpc,bpd->cd", dY, o).view(dv, dv, 1, 1)
    a = [t.to(dev) for t in (g.to(torch.bfloat16), gx.to(torch.bfloat16), ga, gb, gc, o, w)]
    dO = torch.zeros(B, H * W, dv, device=dev)
    return Case(lambda dws: ops.aa_outproj_bwd(*a, dO, dws[0]), [synth.uniform(8, (dv, dv, 1, 1), -1, 1).to(dev)], [want], 1e-4, None,
                unit=dv * dv)


def _dwconv_case(dev):
    """test_dwconv_gpu.py::test_dwconv_weight_gradient at (3, 1, 5, 10, 10, 72, no activation): the tiled kernel of dwconv.hip."""
    from chexpert_amd import ops
    k, s, B, H, W, Cc = 3, 1, 5, 10, 10, 72
    pad = k // 2
    x = bf(trnd(31, (B, Cc, H, W), -2, 2))
    g, g2 = bf(trnd(32, (B, Cc, H, W))), bf(trnd(33, (B, Cc, H, W)))
    ga, gb, gc = trnd(34, (Cc,), 0.5, 1.5), trnd(35, (Cc,), -0.3, 0.3), trnd(36, (Cc,), -0.2, 0.2)
    cv = lambda t: t.view(1, -1, 1, 1)
    dY = bf(g * cv(ga) + g2 * cv(gb) + cv(gc))
    want = torch.nn.grad.conv2d_weight(x, (Cc, 1, k, k), dY, stride=s, padding=pad, groups=Cc)
    q = lambda t: t.permute(0, 2, 3, 1).contiguous().to(torch.bfloat16).to(dev)
    gq, g2q, xq, t = q(g), q(g2), q(x), [v.to(dev) for v in (ga, gb, gc)]
    return Case(lambda dws: ops.dwconv_wgrad(gq, g2q, t[0], t[1], t[2], xq, None, None, dws[0], k=k, stride=s, pad=pad),
                [trnd(39, (Cc, 1, k, k)).to(dev)], [want], 2e-3, None, unit=Cc * k * k)


def _se_case(dev, B=70, H=16, W=16, Cc=8, R=3):
    """test_effnet_glue_gpu.py::test_se_backward_chain, route 1 (split rows + slabs) at (70, 16, 16, 8, 3), bf16 storage: five
    groups of 16 images, four destinations, float64 autograd, bound 1e-4."""
    from chexpert_amd import ops

    def mag(seed, shape, lo, hi):
        g = torch.Generator().manual_seed(seed)
        v = torch.rand(shape, generator=g) * (hi - lo) + lo
        return v * (torch.randint(0, 2, shape, generator=g).float() * 2 - 1)
    HW = H * W
    n_rows = min(max(1, 1024 // B), HW // 16 + 1) * B * Cc
    x = bf(mag(1, (B, HW, Cc), 0.5, 2.0))
    sc, sh = trnd(2, (Cc,), 0.5, 1.5), trnd(3, (Cc,), -0.5, 0.5)
    w1, b1 = trnd(4, (R, Cc)) * (2.0 / Cc ** 0.5), trnd(5, (R,), -0.2, 0.2)
    w2, b2 = trnd(6, (Cc, R)) * (2.0 / R ** 0.5), trnd(7, (Cc,), -0.2, 0.2)
    du = bf(mag(21, (B, HW, Cc), 0.25, 1.0))
    p = [t.double().requires_grad_(True) for t in (w1, b1, w2, b2)]
    a = swish(x.double() * sc.double() + sh.double())
    pooled = a.mean(1).requires_grad_(True)
    h1 = pooled @ p[0].t() + p[1]
    s = torch.sigmoid(swish(h1) @ p[2].t() + p[3])
    (a * s[:, None, :] * du.double()).sum().backward()
    dw0 = [(trnd(30 + i, t.shape) * t.grad.abs().max().float()).to(dev) for i, t in enumerate(p)]
    xd, dud = (t.view(B, H, W, Cc).to(torch.bfloat16).to(dev) for t in (x, du))
    scd, shd, w1d, w2d = (t.to(dev) for t in (sc, sh, w1, w2))
    sd, h1d, pd = (t.detach().float().to(dev) for t in (s, h1, pooled))

    def launch(dws):
        ds, dpooled = torch.empty(B, Cc, device=dev), torch.empty(B, Cc, device=dev)
        ops.se_bwd_fused(dud, xd, scd, shd, ds, sd, h1d, pd, w1d, w2d, dws[0], dws[1], dws[2], dws[3], dpooled,
                         rows=torch.empty(n_rows, device=dev))
    return Case(launch, dw0, [t.grad for t in p], 1e-4, "se_bwd_a_kernel")


def _f32_case(dev):
    """tests/test_fp32_gpu.py::test_f32_weight_gradient at (1x1, K 96, N 128, both prologues): the fp32 storage mode, 240 pixels in
    15 ranges of 16, float64 reference, bound 1e-5."""
    from chexpert_amd import ops
    B, H, W, K, N = 2, 12, 10, 96, 128
    x, g, g2 = rnd(41, (B, K, H, W), -1.5, 1.5), rnd(42, (B, N, H, W)), rnd(43, (B, N, H, W))
    ga, gb, gc = rnd(44, (N,), 0.5, 1.5), rnd(45, (N,), -0.3, 0.3), rnd(46, (N,), -0.2, 0.2)
    pa, pb = rnd(47, (K,), 0.5, 1.5), rnd(48, (K,), -0.3, 0.3)
    cv = lambda t: t.view(1, -1, 1, 1)
    want = torch.nn.grad.conv2d_weight(F.relu(x * cv(pa) + cv(pb)).double(), (N, K, 1, 1), (g * cv(ga) + g2 * cv(gb) + cv(gc)).double()).float()
    q = lambda t: t.permute(0, 2, 3, 1).contiguous().to(dev)
    gq, xq = q(g), q(x)
    kw = dict(g_prologue=ops.PRO_AFFINE2, g2=q(g2), ga=ga.to(dev), gb=gb.to(dev), gc=gc.to(dev), x_prologue=ops.PRO_AFFINE_RELU,
              pa=pa.to(dev), pb=pb.to(dev))
    return Case(lambda dws: ops.conv_wgrad(gq, xq, dws[0], **kw), [rnd(49, (N, K, 1, 1), -1, 1).to(dev)], [want], 1e-5, "wgrad_f32_kernel<",
                unit=N * K)


def _hint8():
    from chexpert_amd import ops
    return ops.kernel_hint(-1, 8)


BUILDERS = {
    "fused_1x1_wide": lambda d: _fused_case(d, 2, True, 2, 9, 10, 96, "pw_bwd2_kernel<"),           # three 64-pixel tiles
    "fused_1x1_narrow": lambda d: _fused_case(d, 2, True, 2, 9, 10, 24, "pw_bwd_kernel<"),          # N < 32: two 128-pixel tiles
    "pair": _pair_case,
    "strip_3x3": lambda d: _conv_case(d, 3, 128, 32, 2, 1, 3, 9, 7, "conv3x3_strip_wgrad_kernel<"),
    "ring_3x3": lambda d: _conv_case(d, 3, 128, 32, 0, 1, 3, 57, 64, "conv3x3_ring_wgrad_kernel<"),
    "pc_3x3": lambda d: _conv_case(d, 3, 128, 32, 2, 1, 7, 10, 10, "conv3x3_pc_wgrad_kernel<", hint=_hint8()),
    "batch_3x3": _batch_case,
    "pool2": _pool2_case,
    "stem": _stem_case,
    "generic_3x3s2": lambda d: _conv_case(d, 3, 64, 128, 2, 1, 2, 18, 18, "wgrad_kernel<", stride=2),
    "wgrad_mm": lambda d: _conv_case(d, 1, 96, 128, 2, 1, 2, 8, 8, "wgrad_mm_kernel<"),             # 128 pixels: a multiple of 32
    "wgrad3": lambda d: _conv_case(d, 3, 128, 96, 2, 1, 2, 9, 10, "wgrad3_kernel<"),
    "aa_outproj": _aa_case,
    "dwconv": _dwconv_case,
    "se_bwd": _se_case,
    "conv_f32": _f32_case,
    "se_tiny": lambda d: _se_case(d, 2, 5, 3, 8, 2),             # section 3 only: four descriptors for 74 slab floats
    "batch_2": lambda d: _batch_case(d, 2),                      # section 3 only
}
PRODUCERS = [k for k in BUILDERS if k not in ("se_tiny", "batch_2")]
_cases = {}


def case(name, dev):
    """Operands and reference of a launcher, built once for the module and never written to, with the immediate slab mode's result."""
    from chexpert_amd import ops
    c = _cases.get(name)
    if c is None:
        c = _cases[name] = BUILDERS[name](dev)
        a = ops._arenas.get(dev.index)
        assert ops.WGRAD_SCRATCH_FLOATS > 0 and (a is None or not a.active), "build a case before wgrad_defer_begin"
        c.imm = [t.clone() for t in c.dw0]
        c.launch(c.imm)
        c.kernel, c.floats = ops.last_kernel(), slab_floats()
        torch.cuda.synchronize()
    return c


def fresh(c):
    return [t.clone() for t in c.dw0]


@pytest.mark.parametrize("name", PRODUCERS)
def test_deferred_sums_give_the_immediate_slab_bits_and_match_the_reference(dev, arena, name):
    from chexpert_amd import ops
    from chexpert_amd._lib import lib
    arena(16 << 20, 1 << 20)
    c = case(name, dev)
    print("%s: %s, %d slab floats" % (name, c.kernel, c.floats))
    if c.family is not None:
        assert c.kernel.startswith(c.family), c.kernel
    if name == "pool2":
        assert c.kernel.endswith(", 1>"), c.kernel             # MODE_POOL2 of the generic kernel
    if name == "wgrad3":                 # its own sum runs behind the kernel even while deferring
        assert c.floats == 0, "wgrad3 sums at once: it must not report a region a deferring caller would keep"
    else:
        assert c.floats > 0, "the launch fell back to atomics"
        if c.unit:
            assert c.floats % c.unit == 0, "%d reported floats are no whole number of %d-float slabs" % (c.floats, c.unit)
            assert c.floats // c.unit > 1, "one pixel split: nothing to order"
    for got, d0, want in zip(c.imm, c.dw0, c.want):
        close(got - d0, want, c.rel, "%s immediate" % name)
    # deferred, into the same prefill
    dws = fresh(c)
    assert ops.wgrad_defer_begin(dev)
    a = ops._arenas[dev.index]
    c.launch(dws)
    assert c.family is None or ops.last_kernel() == c.kernel
    assert slab_floats() == c.floats and a.off == up64(c.floats) == a.need
    assert lib().cx_wgrad_defer(1) == 1, "the launch left deferral"
    if name == "wgrad3":
        assert all(same(x, y) for x, y in zip(dws, c.imm)), "wgrad3 under deferral: not final after the call"
    else:
        assert all(same(x, y) for x, y in zip(dws, c.dw0)), "a deferred launch added to dw before the flush"
    ops.wgrad_defer_flush(dev)
    assert lib().cx_wgrad_defer(0) == 0, "the flush left deferral on"
    for i, (x, y) in enumerate(zip(dws, c.imm)):
        assert same(x, y), "%s: deferred dw %d differs from the immediate slab mode in %d elements" % (name, i, int((bits(x) != bits(y)).sum()))
    assert len(a.tables) == (0 if name == "wgrad3" else 1)


def test_the_atomic_routes_report_no_slab(dev, arena, monkeypatch):
    """A launch that adds with atomics reports 0 floats -- not the figure of the launch before it -- and a deferring caller's arena
    stays where it is.  The fp32 storage mode's convolution gradient (which kept the previous figure), without a workspace and
    with a region too small for its 15 slabs."""
    from chexpert_amd import ops
    from chexpert_amd._lib import lib
    arena(4096, 1024)
    stem, c = case("stem", dev), case("conv_f32", dev)
    need = 15 * c.unit
    assert c.floats == need > 4096
    # no workspace, no deferral
    stem.launch(fresh(stem))
    assert slab_floats() == stem.floats > 0
    monkeypatch.setattr(ops, "WGRAD_SCRATCH_FLOATS", 0)
    d = fresh(c)
    c.launch(d)
    assert ops.last_kernel() == c.kernel
    assert slab_floats() == 0, "an atomic launch reports the previous launch's slab (%d floats)" % slab_floats()
    close(d[0] - c.dw0[0], c.want[0], c.rel, "fp32 dW through atomics")
    # deferring, with less room than the launch needs: atomics, final at once, nothing recorded
    monkeypatch.setattr(ops, "WGRAD_SCRATCH_FLOATS", 16 << 20)
    stem.launch(fresh(stem))
    assert slab_floats() == stem.floats
    assert ops.wgrad_defer_begin(dev)
    a = ops._arenas[dev.index]
    assert a.buf.numel() == 4096
    d = fresh(c)
    c.launch(d)
    assert slab_floats() == 0 and a.off == 0 and a.need == 0, "the arena advanced by memory nobody used"
    assert lib().cx_wgrad_defer(1) == 1
    close(d[0] - c.dw0[0], c.want[0], c.rel, "fp32 dW through atomics while deferring")
    at_once = d[0].clone()
    ops.wgrad_defer_flush(dev)
    assert same(d[0], at_once) and len(a.tables) == 0


# ------------------------------------------------------------------------------------------------ 3. the arena
def _nan_fill(a):
    a.buf.view(torch.int32).fill_(SENT_BITS)


def _untouched(a, start):
    return bool((a.buf[start:].view(torch.int32) == SENT_BITS).all())


def test_a_launch_writes_nothing_past_the_region_it_reports(dev, arena):
    """A plain launch, the pair launch (two slabs from one region), se_bwd_fused (slabs + partial rows) and the batch launch, one
    after the other in a 1 Mi-float arena filled with a NaN pattern."""
    from chexpert_amd import ops
    arena(1 << 20, 256 << 10)
    seq = [case(n, dev) for n in ("pool2", "pair", "se_bwd", "wgrad_mm", "batch_2")]
    assert ops.wgrad_defer_begin(dev)
    a = ops._arenas[dev.index]
    assert a.buf.numel() == 1 << 20
    _nan_fill(a)
    regions, dws = [], []
    for c in seq:
        before = a.off
        d = fresh(c)
        c.launch(d)
        dws.append(d)
        n = slab_floats()
        assert n == c.floats > 0, "%s: deferred where it should not fall back" % c.kernel
        assert a.off == before + up64(n), "%s: the arena advanced by %d for %d reported floats" % (c.kernel, a.off - before, n)
        torch.cuda.synchronize()
        assert _untouched(a, before + n), "%s wrote past the %d floats it reports" % (c.kernel, n)
        for lo, hi, snap, who in regions:
            assert torch.equal(bits(a.buf[lo:hi]), snap), "%s changed the region of %s" % (c.kernel, who)
        regions.append((before, a.off, bits(a.buf[before:a.off]).clone(), c.kernel))
    ops.wgrad_defer_flush(dev)
    for c, d in zip(seq, dws):
        assert all(same(x, y) for x, y in zip(d, c.imm)), c.kernel
    for lo, hi, snap, who in regions:                           # the table kernel reads the slabs, no more
        assert torch.equal(bits(a.buf[lo:hi]), snap), who
    assert _untouched(a, a.off)


def test_overflow_falls_back_to_the_immediate_sum_and_the_next_pass_fits(dev, arena):
    """Stem launches of 112 896 slab floats into a 1 Mi-float arena that defers while 256 Ki floats are free: the eighth starts
    with 258 304 free and sums at once."""
    from chexpert_amd import ops
    from chexpert_amd._lib import lib
    START, MIN_FREE, n = 1 << 20, 256 << 10, 8
    arena(START, MIN_FREE)
    c = case("stem", dev)
    per = up64(c.floats)
    assert per == 112896 and START - (n - 1) * per < MIN_FREE <= START - (n - 2) * per
    for second in (False, True):
        assert ops.wgrad_defer_begin(dev)
        a = ops._arenas[dev.index]
        if second:
            assert a.buf.numel() >= n * per, "the arena did not grow to what the pass before needed"
            assert a.buf.numel() - (n - 1) * per >= MIN_FREE
            assert len(a.tables) == 0, "tables of the old buffer's addresses survived the reallocation"
        else:
            assert a.buf.numel() == START
        dws = [fresh(c) for _ in range(n)]
        for i, d in enumerate(dws):
            c.launch(d)
            assert slab_floats() == c.floats
            assert lib().cx_wgrad_defer(1) == 1, "launch %d left the C-side switch off" % i
            spilled = not second and i == n - 1
            assert a.off == (i + (0 if spilled else 1)) * per and a.need == (i + 1) * per
            assert same(d[0], c.imm[0] if spilled else c.dw0[0]), "launch %d: %s" % (i, "not final at once" if spilled else "added early")
        ops.wgrad_defer_flush(dev)
        for i, d in enumerate(dws):
            assert same(d[0], c.imm[0]), "pass %d, launch %d: lost or repeated a sum" % (second, i)
        assert len(a.tables) == 1


def test_a_repeated_schedule_reuses_its_table(dev, arena):
    from chexpert_amd import ops
    from chexpert_amd._lib import CxReduceDesc
    arena(1 << 20, 256 << 10)
    seq = [case(n, dev) for n in ("stem", "pair", "wgrad_mm")]
    dws = [fresh(c) for c in seq]

    def one_pass(order):
        for d, c in zip(dws, seq):
            for t, t0 in zip(d, c.dw0):
                t.copy_(t0)
        assert ops.wgrad_defer_begin(dev)
        for i in order:
            seq[i].launch(dws[i])
        ops.wgrad_defer_flush(dev)
        for d, c in zip(dws, seq):
            assert all(same(x, y) for x, y in zip(d, c.imm)), c.kernel
    one_pass((0, 1, 2))
    a = ops._arenas[dev.index]
    keys = list(a.tables)
    assert len(keys) == 1 and len(keys[0]) == 4 * C.sizeof(CxReduceDesc)          # stem, pair a, pair b, wgrad_mm
    held = a.tables[keys[0]]
    one_pass((0, 1, 2))
    assert list(a.tables) == keys and a.tables[keys[0]] is held, "the same schedule uploaded a second table"
    one_pass((2, 0, 1))
    assert len(a.tables) == 2 and keys[0] in a.tables


def test_flush_keep_goes_on_deferring_without_repeating_a_sum(dev, arena):
    from chexpert_amd import ops
    from chexpert_amd._lib import lib
    arena(1 << 20, 256 << 10)
    A, B_, C_ = case("stem", dev), case("pair", dev), case("wgrad_mm", dev)
    da, db, dc = fresh(A), fresh(B_), fresh(C_)
    assert ops.wgrad_defer_begin(dev)
    a = ops._arenas[dev.index]
    A.launch(da)
    B_.launch(db)
    off = a.off
    ops.wgrad_defer_flush(dev, keep=True)
    assert a.active and a.off == off == up64(A.floats) + up64(B_.floats), "flush(keep) gave the slabs of the pass away"
    assert lib().cx_wgrad_defer(1) == 1
    assert all(same(x, y) for x, y in zip(da + db, A.imm + B_.imm)), "not final after flush(keep=True)"
    C_.launch(dc)
    assert a.off == off + up64(C_.floats)
    assert same(dc[0], C_.dw0[0])
    ops.wgrad_defer_flush(dev)
    assert not a.active and lib().cx_wgrad_defer(0) == 0
    assert same(dc[0], C_.imm[0])
    assert all(same(x, y) for x, y in zip(da + db, A.imm + B_.imm)), "the second flush added the first flush's slabs again"


def test_abort_drops_the_recorded_sums(dev, arena):
    from chexpert_amd import ops
    from chexpert_amd._lib import lib
    arena(1 << 20, 256 << 10)
    A, B_ = case("pair", dev), case("wgrad_mm", dev)
    da, db = fresh(A), fresh(B_)
    assert ops.wgrad_defer_begin(dev)
    A.launch(da)
    B_.launch(db)
    ops.wgrad_defer_abort(dev)
    a = ops._arenas[dev.index]
    assert not a.active and lib().cx_wgrad_defer(0) == 0
    ops.wgrad_defer_abort(dev)                               # a second abort, and a flush after it: no-ops
    ops.wgrad_defer_flush(dev)
    assert ops.wgrad_defer_begin(dev)
    d2 = fresh(B_)
    B_.launch(d2)
    ops.wgrad_defer_flush(dev)
    assert same(d2[0], B_.imm[0])
    assert all(same(x, y) for x, y in zip(da + db, A.dw0 + B_.dw0)), "an aborted launch reached its dw"
    # outside deferral the same launch sums at once again
    d3 = fresh(B_)
    B_.launch(d3)
    assert same(d3[0], B_.imm[0])


def test_more_than_1024_recorded_sums_is_an_error(dev, arena):
    """257 se_bwd_fused launches of four descriptors each (74 slab floats per launch)."""
    from chexpert_amd import ops
    from chexpert_amd._lib import lib
    arena(1 << 20, 256 << 10)
    c = case("se_tiny", dev)
    d = fresh(c)
    assert ops.wgrad_defer_begin(dev)
    for _ in range(257):
        c.launch(d)
    with pytest.raises(RuntimeError, match="more than 1024 deferred"):
        ops.wgrad_defer_flush(dev)
    a = ops._arenas[dev.index]
    assert not a.active and lib().cx_wgrad_defer(0) == 0
    assert all(same(x, y) for x, y in zip(d, c.dw0))
    assert ops.wgrad_defer_begin(dev)                        # the next pass starts from an empty list
    for _ in range(256):
        c.launch(d)
    ops.wgrad_defer_flush(dev)
    one = fresh(c)
    assert ops.wgrad_defer_begin(dev)
    c.launch(one)
    ops.wgrad_defer_flush(dev)
    assert all(same(x, y) for x, y in zip(one, c.imm))


# ------------------------------------------------------------------------------------------------ 4. the engines
def _densenet(dev):
    from chexpert_amd.models import DenseNet
    return DenseNet(32, (2, 2, 2, 2), 64, num_classes=5).to(dev).train(), 4, 64


def _resnet(dev):
    from chexpert_amd.models import Bottleneck, ResNet
    return ResNet(Bottleneck, [1, 1, 1, 1], num_classes=5).to(dev).train(), 4, 64


def _effnet(dev):
    from chexpert_amd.models import construct_model
    from chexpert_amd.models.efficientnet import DropMarker
    model = construct_model("efficientnet-b0", 5).to(dev).train()
    for mod in model.modules():
        if isinstance(mod, DropMarker):
            mod.p = 0.0
    return model, 4, 96


def _densenet_fp32(dev):
    from chexpert_amd.models import DenseNet
    from oracle import nets
    cfg = (2, 2, 2, 2)
    sd = synth.fill_state_dict_(nets.zeros_state_dict(nets.densenet_spec(5, block_config=cfg)), 3)
    model = DenseNet(32, cfg, 64, num_classes=5).storage_dtype("fp32")
    model.load_state_dict(sd, strict=True)
    return model.to(dev).train(), 4, 64


@pytest.mark.parametrize("build", [_densenet, _resnet, _effnet, _densenet_fp32], ids=lambda f: f.__name__.strip("_"))
def test_engine_gradients_are_the_same_bits_with_and_without_deferral(dev, arena, monkeypatch, build):
    from chexpert_amd import ops
    torch.manual_seed(21)
    model, B, S = build(dev)
    x, t = synth.xray_batch(700, B, S).to(dev), synth.targets(701, B, 5).to(dev)
    sd = {k: v.clone() for k, v in model.state_dict().items()}

    def step():
        model.load_state_dict(sd)
        model.zero_grad()
        loss, logits = model.forward_backward(x, t)
        return loss.clone(), logits.clone(), {k: p.grad.detach().clone() for k, p in model.named_parameters()}
    begun, begin = [], ops.wgrad_defer_begin
    monkeypatch.setattr(ops, "wgrad_defer_begin", lambda device: begun.append(begin(device)) or begun[-1])
    shipped = step()
    a = ops._arenas.get(dev.index)
    assert begun == [True] and a is not None and not a.active, "the shipped step did not defer"
    assert a.off == a.need > 0 and len(a.tables) >= 1, "a launch of the shipped step fell back to the immediate sum"
    monkeypatch.setattr(type(model._eng()), "_defer_wgrad", lambda self: False)
    plain = step()
    assert begun == [True], "the patched step deferred"
    assert torch.equal(shipped[0], plain[0]) and torch.equal(shipped[1], plain[1])
    for k, g in shipped[2].items():
        assert same(g, plain[2][k]), "%s: %d elements differ" % (k, int((bits(g) != bits(plain[2][k])).sum()))
