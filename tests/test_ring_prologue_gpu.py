"""GPU: the 3x3 ring kernels of the dense layers (csrc/conv3x3_ring.hip) on the small maps, where a workgroup has one or two steps
and the prologue -- the first window of an image requested in one burst with the weights, then staged -- is most of the launch.

Through ops.conv_gemm against the fp32 oracle form, with the comparison and the tolerances of tests/test_kernels_gpu.py
(test_conv3x3_slice_output, test_dgrad_affine2_mask_epilogue, test_dgrad_3x3_dense_side_output_of_the_prologue).  Every case is
launched twice on fresh outputs and the two results are compared bit for bit: a load consumed before it was retired, or a ring
pixel read before anything wrote it, shows as a difference between the runs.

Shapes (H, W):
  10x10   one step per image              20x20   two steps per image           12x10   H != W
  40x40 at B = 1: several steps of one image, spread over workgroups that start inside the image
  B = 1, 2, 3 on the first three: the first window of an image has its top halo row outside the image.
In-loop restart (a workgroup's range crossing an image boundary; launcher: steps_per_wg against steps per image spi):
  B = 257 on 10x10   spi = 1, 256 images or more give a workgroup ceil(B / 256) whole images: 2 steps, the second a restart
  B = 100 on 30x20   spi = 3, 300 steps in ranges of 2: ranges start inside an image and cross into the next one
Restart in two bursts (the two window rows do not fit the chunk slots kept for them):
  forward 7x58 (one-deep pipeline), 6x96 (two column tiles of 48, two-deep pipeline); input gradient 3x130 (one row per step).
"""
import pytest
import torch
import torch.nn.functional as F

from chexpert_amd import synth

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    from chexpert_amd import _lib
    _lib.lib()          # fail loudly if the HIP library is missing
    return torch.device("cuda:0")


def bf(t):
    return t.to(torch.bfloat16).float()


def rnd(seed, shape, lo=-1.0, hi=1.0):
    return synth.uniform(seed, shape, lo, hi)


def nhwc_buf(seed, B, H, W, C, dev, lo=-1.5, hi=1.5):
    """bf16 NHWC buffer on the GPU + its fp32 NCHW value on the CPU."""
    v = bf(rnd(seed, (B, H, W, C), lo, hi))
    return v.to(torch.bfloat16).to(dev), v.permute(0, 3, 1, 2).contiguous()


def to_nchw(t):
    return t.float().cpu().permute(0, 3, 1, 2).contiguous()


def close(got, want, rel=6e-3, what=""):
    scale = want.abs().max().item() + 1e-6
    err = (got - want).abs().max().item()
    print("%s: max err %.3e vs scale %.3e (rel %.2e, bound %.1e)" % (what, err, scale, err / scale, rel))
    assert err <= rel * scale, "%s: max err %.3e vs scale %.3e (rel %.2e)" % (what, err, scale, err / scale)


SMALL = [(B, H, W) for (H, W) in ((10, 10), (20, 20), (12, 10)) for B in (1, 2, 3)] + [(1, 40, 40)]
CROSSING = [(257, 10, 10), (100, 30, 20)]
CAP = 300           # statistic rows: one per workgroup, at most 256


@pytest.mark.parametrize("B,H,W", SMALL + CROSSING + [(1, 7, 58), (1, 6, 96)])
def test_ring_forward_bnrelu_channel_sums(dev, B, H, W):
    """3x3 forward K = 128 -> N = 32 behind BN + ReLU, output a channel slice of a wider buffer, deterministic channel-sum rows."""
    from chexpert_amd import ops
    K, N = 128, 32
    xb, x = nhwc_buf(5, B, H, W, K, dev)
    w = bf(rnd(6, (N, K, 3, 3), -0.1, 0.1))
    pa, pb = rnd(7, (K,), -0.3, 1.5), rnd(8, (K,), -0.5, 0.5)
    a = bf(F.relu(x * pa.view(1, -1, 1, 1) + pb.view(1, -1, 1, 1)))
    want = F.conv2d(a, w, padding=1)
    wp, pad, pbd = ops.pack_weights(w.to(dev)), pa.to(dev), pb.to(dev)
    outs = []
    for _ in range(2):
        buf = torch.full((B, H, W, 96 + N), -3.0, dtype=torch.bfloat16, device=dev)
        st = torch.full((2, CAP, N), float("nan"), device=dev)
        rows = ops.conv_gemm(xb, wp, buf[..., 96:], N=N, kh=3, kw=3, stride=1, pad=1, prologue=ops.PRO_AFFINE_RELU, pa=pad, pb=pbd,
                             stat_sum=st[0], stat_sq=st[1], stat_det=True, stat_replicas=CAP, stat_rstride=N)
        assert ops.lib().cx_last_kernel().decode().startswith("conv3x3_ring_fwd_kernel")
        assert 0 < rows <= 256 and torch.isfinite(st[:, :rows]).all() and torch.isnan(st[:, rows:]).all()
        outs.append((buf.clone(), st[:, :rows].clone()))
    assert torch.equal(outs[0][0], outs[1][0]), "two launches differ in the output"
    assert torch.equal(outs[0][1], outs[1][1]), "two launches differ in the statistic rows"
    buf, st = outs[0]
    got = to_nchw(buf[..., 96:])
    close(got, want, what="y")
    assert (buf[..., :96].float() == -3.0).all(), "wrote outside the channel slice"
    close(st[0].sum(0).cpu(), got.sum((0, 2, 3)), rel=1e-4, what="sum")
    close(st[1].sum(0).cpu(), (got * got).sum((0, 2, 3)), rel=1e-4, what="sumsq")


@pytest.mark.parametrize("B,H,W", SMALL + CROSSING + [(1, 3, 130)])
def test_ring_dgrad_affine2_mask_stats_side_output(dev, B, H, W):
    """3x3 input gradient K = 32 -> N = 128: AFFINE2 prologue on slices of wider buffers, mask epilogue, S1 / S2 rows, and the
    prologue's side output (CxConv.pro_out)."""
    from chexpert_amd import ops
    K, N = 32, 128
    ub, u = nhwc_buf(20, B, H, W, K + 96, dev)            # slices of wider buffers, as in a dense block
    vb, v = nhwc_buf(21, B, H, W, K + 96, dev)
    exb, ex = nhwc_buf(22, B, H, W, N + 32, dev)
    w = bf(rnd(24, (K, N, 3, 3), -0.1, 0.1))              # forward conv weight (O = K, I = N): the input gradient maps K -> N
    pa, pb, pc = rnd(25, (K,), 0.5, 1.5), rnd(26, (K,), -0.3, 0.3), rnd(27, (K,), -0.2, 0.2)
    e_sc, e_sh = rnd(28, (N,), -0.3, 1.5), rnd(29, (N,), -0.5, 0.5)
    e_mu, e_r, e_scale = rnd(30, (N,), -0.5, 0.5), rnd(31, (N,), 0.5, 2.0), rnd(32, (N,), -0.3, 1.5)
    cv = lambda t: t.view(1, -1, 1, 1)
    us, vs = ub[..., 64:64 + K], vb[..., 64:64 + K]
    dy = bf(u[:, 64:64 + K] * cv(pa) + v[:, 64:64 + K] * cv(pb) + cv(pc))
    acc_ref = F.conv_transpose2d(dy, w, padding=1)        # = input gradient of the forward conv
    exs = ex[:, :N]
    dz = torch.where((exs * cv(e_sc) + cv(e_sh)) > 0, acc_ref, torch.zeros(()))
    want = cv(e_scale) * dz
    S1 = dz.sum((0, 2, 3))
    S2 = (dz * (exs - cv(e_mu)) * cv(e_r)).sum((0, 2, 3))
    wp = ops.pack_weights(w.to(dev), transpose=True)
    d = lambda t: t.to(dev)
    coef = dict(pa=d(pa), pb=d(pb), pc=d(pc), e_sc=d(e_sc), e_sh=d(e_sh), e_mu=d(e_mu), e_r=d(e_r), e_scale=d(e_scale))
    outs = []
    for _ in range(2):
        out = torch.full((B, H, W, N + 32), 5.0, dtype=torch.bfloat16, device=dev)
        side = torch.full((B, H, W, K), 7.0, dtype=torch.bfloat16, device=dev)
        st = torch.full((2, CAP, N), float("nan"), device=dev)
        rows = ops.conv_gemm(us, wp, out[..., :N], N=N, kh=3, kw=3, pad=1, prologue=ops.PRO_AFFINE2, x2=vs, epilogue=ops.EPI_MASK,
                             ex=exb[..., :N], stat_sum=st[0], stat_sq=st[1], stat_det=True, stat_replicas=CAP, stat_rstride=N,
                             pro_out=side, **coef)
        assert ops.lib().cx_last_kernel().decode().startswith("conv3x3_ring_dgrad_kernel")
        assert ops.last_pro_out()
        assert 0 < rows <= 256 and torch.isfinite(st[:, :rows]).all() and torch.isnan(st[:, rows:]).all()
        outs.append((out.clone(), side.clone(), st[:, :rows].clone()))
    for k, what in enumerate(("the output", "the side output", "the statistic rows")):
        assert torch.equal(outs[0][k], outs[1][k]), "two launches differ in " + what
    out, side, st = outs[0]
    close(to_nchw(out[..., :N]), want, rel=8e-3, what="g")
    assert (out[..., N:].float() == 5.0).all(), "wrote outside the slice"
    close(st[0].sum(0).cpu(), S1, rel=2e-3, what="S1")
    close(st[1].sum(0).cpu(), S2, rel=2e-3, what="S2")
    cl = lambda t: t.view(1, 1, 1, -1).to(dev)
    want_side = torch.addcmul(torch.addcmul(cl(pc), vs.float(), cl(pb)), us.float(), cl(pa)).to(torch.bfloat16)   # fmaf(u, a, fmaf(v, b, c))
    assert (side.float() - want_side.float()).abs().max().item() <= 2.0 ** -7 * want_side.float().abs().max().item()   # (one bf16 ulp: fma contraction)
    assert (side == want_side).float().mean().item() > 0.99
