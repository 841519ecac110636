"""Case tables and float64 references of the dilated / grouped 3x3 convolution tests (test_conv_dilated_gpu.py runs the kernels,
test_conv_dilated_cpu.py checks this module by itself; not collected: no test_ prefix).  Nothing here needs a GPU.

All convolutions are 3x3 with padding = dilation.  The reference is CPU float64, F.conv2d(a, w, stride=s, padding=d, dilation=d,
groups=g) on operands that hold storage-type values; the input gradient and the weight gradient are torch.autograd.grad of that
same call.  Prologues and epilogues are restated as in test_conv_mm_gpu.py:

    a  = relu(x*pa + pb)                     BN + ReLU of the activation operand (pb > 0 on every channel: a padded tap filled
                                             with relu(pb) where 0 belongs shows on every border pixel)
    dy = u*pa + v*pb + pc                    BN backward of the gradient operand
    dz = where(ex*e_sc + e_sh > 0, acc, 0)   out = e_scale*dz (+ old)    S1 = sum dz    S2 = sum dz*(ex - e_mu)*e_r

A value the bf16 kernels round before the MFMA (a, dy) is rounded to bf16 here too; the fp32 kernels keep it in registers, so the
fp32 reference leaves it in float64.  The mask predicate is evaluated in float64 on storage-type operands: the product is exact
there and the sign of the rounded sum is the sign of the exact one, which is also what the kernels' fp32 fmaf returns."""
import collections
import functools
import types

import torch
import torch.nn.functional as F

from chexpert_amd import synth

BF16, F32 = "bf16", "f32"

# Bounds, relative to max|want|: the bf16 figures of test_conv_mm_gpu.py, the fp32 figures of test_fp32_gpu.py (whose masked
# gradient holds 4e-6).  y: a stored convolution output; g: the masked gradient; S: S1 / S2; sums: the statistic rows against the
# sums of the stored output; dw: the weight gradient.
TOL = {BF16: dict(y=6e-3, g=8e-3, S=2e-3, sums=1e-4, dw=2e-3),
       F32: dict(y=2e-6, g=4e-6, S=5e-5, sums=2e-5, dw=1e-5)}

Case = collections.namedtuple("Case", "B H W K N dil stride Ho Wo groups", defaults=(1,))

# K, N: input / output channels of the forward convolution (the input gradient maps N -> K)
CASES = [
    Case(2, 9, 11, 64, 64, 2, 1, 9, 11),        # BN = 64 tile, 198 pixels = 1.55 pixel tiles
    Case(1, 4, 5, 128, 128, 4, 1, 4, 5),        # map smaller than the 9-pixel tap extent: six of the nine taps are all padding; BN = 128
    Case(3, 7, 6, 40, 32, 2, 1, 7, 6),          # partial last K step (8 of 32), N == 32 tile, wgrad_kernel<32, 128
    Case(2, 13, 10, 72, 200, 2, 2, 7, 5),       # dil with stride, odd height; ragged N (three 64-tiles + 8)
    Case(2, 13, 10, 72, 72, 2, 2, 7, 5),        # ... its twins: one 64-tile + 8,
    Case(2, 13, 10, 72, 104, 2, 2, 7, 5),       # ... and a partial 128-row tile of dW (N % 128 >= 96)
    Case(2, 12, 9, 64, 128, 2, 2, 6, 5),        # the same with an even height (a forward input row the stride grid never reaches)
    Case(2, 8, 8, 32, 96, 3, 1, 8, 8),          # odd dilation: nothing may assume a power of two
]

# the grouped 3x3 of a ResNeXt bottleneck as the engine launches it: one launch per group on channel slices
GROUPED = [
    Case(2, 9, 10, 128, 128, 1, 1, 9, 10, 4),   # 32 channels per group
    Case(2, 9, 10, 128, 128, 2, 1, 9, 10, 4),
    Case(2, 9, 10, 32, 32, 1, 1, 9, 10, 4),     # 8 channels per group: an 8-of-32 K step, 8 valid columns of a 64-wide tile
    Case(2, 9, 10, 32, 32, 2, 1, 9, 10, 4),
]

# exact runs (impulses / small integers): dil = 2 at both strides (odd and even height), dil = 4 on the 4x5 map
EXACT = [
    Case(5, 9, 11, 16, 24, 2, 1, 9, 11),
    Case(5, 13, 10, 16, 24, 2, 2, 7, 5),
    Case(5, 12, 9, 16, 24, 2, 2, 6, 5),
    Case(5, 4, 5, 16, 24, 4, 1, 4, 5),
]
EXACT_CH_IN = (0, 3, 7, 10, 15)                 # the channel of each image's impulse (both parities of c)
EXACT_CH_OUT = (0, 5, 11, 18, 23)


def cid(c):
    return "%dx%dx%d_K%d_N%d_d%d_s%d%s" % (c.B, c.H, c.W, c.K, c.N, c.dil, c.stride, "_g%d" % c.groups if c.groups > 1 else "")


# ---- the library's shape validation (cx_conv_gemm / cx_conv_wgrad, 3x3, pad = dil), restated
def _extent(c):
    return c.dil * 2 + 1


def lib_forward_size(c):
    """(Ho, Wo) cx_conv_gemm demands of a forward launch with stride = c.stride, pad = dil = c.dil, or None if it rejects it."""
    ke = _extent(c)
    if c.H + 2 * c.dil - ke < 0 or c.W + 2 * c.dil - ke < 0:
        return None
    return (c.H + 2 * c.dil - ke) // c.stride + 1, (c.W + 2 * c.dil - ke) // c.stride + 1


def lib_accepts_dgrad(c):
    """cx_conv_gemm's check of the input-gradient launch: operand (Ho, Wo), output (H, W), pad = dil = c.dil, tstride = c.stride."""
    ke, pad = _extent(c), c.dil
    if c.stride > 1:
        fpad = ke - 1 - pad                      # the forward's padding
        if c.stride > 2 or fpad < 0 or c.H + 2 * fpad - ke < 0 or c.W + 2 * fpad - ke < 0:
            return False
        return c.Ho == (c.H + 2 * fpad - ke) // c.stride + 1 and c.Wo == (c.W + 2 * fpad - ke) // c.stride + 1
    return c.H == c.Ho + 2 * pad - ke + 1 and c.W == c.Wo + 2 * pad - ke + 1


def lib_accepts_wgrad(c):
    return (c.Ho, c.Wo) == lib_forward_size(c)


def gemm_bn(n):
    """launch_bn (conv_gemm.hip): the channel tile of conv_gemm_kernel."""
    return 128 if n % 128 == 0 else 32 if n == 32 else 64


def wgrad_tile(n):
    """launch_tile (conv_wgrad.hip): (BNW, BCW) of wgrad_kernel."""
    if n == 32:
        return 32, 128
    return (128, 64) if (n % 128 == 0 or n % 128 >= 96 or n >= 224) else (64, 64)


def untouched_fraction(c):
    """Share of the forward input's pixels that no tap of a 3x3 with pad = dil and this stride reads (their gradient is 0)."""
    if c.stride == 1:
        return 0.0
    hit = lambda n, no: len({o * c.stride - c.dil + k * c.dil for o in range(no) for k in range(3)} & set(range(n)))
    return 1.0 - hit(c.H, c.Ho) * hit(c.W, c.Wo) / float(c.H * c.W)


# ---- operands
def rnd(seed, shape, lo=-1.0, hi=1.0):
    return synth.uniform(seed, shape, lo, hi).double()


def stored(t, dt):
    """float64 tensor of the values a tensor of storage type dt holds."""
    return t.to(torch.bfloat16).double() if dt == BF16 else t.float().double()


def staged(t, dt):
    """a prologue result as the kernel multiplies it: rounded to bf16 by the bf16 kernels, kept in registers by the fp32 ones."""
    return t.to(torch.bfloat16).double() if dt == BF16 else t


def cv(t):
    return t.view(1, -1, 1, 1)


@functools.lru_cache(maxsize=None)
def data(c, dt, seed=0):
    """Operands of a case (float64 tensors of storage-type values, NCHW; coefficient vectors hold fp32 values).  Read only."""
    B, H, W, K, N, Ho, Wo = c.B, c.H, c.W, c.K, c.N, c.Ho, c.Wo
    s = 100 * seed + 7
    d = types.SimpleNamespace()
    d.x = stored(rnd(s + 1, (B, K, H, W), -1.5, 1.5), dt)
    d.w = stored(rnd(s + 2, (N, K // c.groups, 3, 3), -0.1, 0.1), dt)
    d.pa, d.pb = rnd(s + 3, (K,), -0.3, 1.5), rnd(s + 4, (K,), 0.2, 0.5)
    d.u = stored(rnd(s + 5, (B, N, Ho, Wo), -1.5, 1.5), dt)
    d.v = stored(rnd(s + 6, (B, N, Ho, Wo), -1.5, 1.5), dt)
    d.ga, d.gb, d.gc = rnd(s + 7, (N,), 0.5, 1.5), rnd(s + 8, (N,), -0.3, 0.3), rnd(s + 9, (N,), -0.2, 0.2)
    d.ex = stored(rnd(s + 10, (B, K, H, W), -1.5, 1.5), dt)
    d.old = stored(rnd(s + 11, (B, K, H, W), -1.5, 1.5), dt)
    d.e_sc, d.e_sh = rnd(s + 12, (K,), -0.3, 1.5), rnd(s + 13, (K,), -0.5, 0.5)
    d.e_mu, d.e_r, d.e_scale = rnd(s + 14, (K,), -0.5, 0.5), rnd(s + 15, (K,), 0.5, 2.0), rnd(s + 16, (K,), -0.3, 1.5)
    d.dw0 = rnd(s + 17, (N, K // c.groups, 3, 3), -1.0, 1.0)            # what the weight gradient is added to
    return d


def conv_and_grads(c, a, w, dy):
    """y = conv2d(a, w) of the case in float64, and autograd's gradients of that call at the output gradient dy."""
    a, w = a.detach().clone().requires_grad_(), w.detach().clone().requires_grad_()
    y = F.conv2d(a, w, stride=c.stride, padding=c.dil, dilation=c.dil, groups=c.groups)
    assert tuple(y.shape[2:]) == (c.Ho, c.Wo), (tuple(y.shape), c)
    da, dw = torch.autograd.grad(y, (a, w), dy)
    return y.detach(), da, dw


def transposed_input_grad(c, w, dy):
    """The input gradient by a second formula (conv_transpose2d), for the self-consistency check of the CPU test only."""
    op = ((c.H - 1) % c.stride, (c.W - 1) % c.stride)
    return F.conv_transpose2d(dy, w, stride=c.stride, padding=c.dil, output_padding=op, dilation=c.dil, groups=c.groups)


@functools.lru_cache(maxsize=None)
def refs(c, dt, seed=0):
    """Every reference of a case, computed once.  plain: no prologue; pro: a = relu(x*pa + pb), dy = u*ga + v*gb + gc."""
    d = data(c, dt, seed)
    r = types.SimpleNamespace()
    r.a = staged(F.relu(d.x * cv(d.pa) + cv(d.pb)), dt)
    r.dy = staged(d.u * cv(d.ga) + d.v * cv(d.gb) + cv(d.gc), dt)
    r.y_plain, r.dx_plain, r.dw_plain = conv_and_grads(c, d.x, d.w, d.u)
    r.y_pro, r.dx_pro, r.dw_pro = conv_and_grads(c, r.a, d.w, r.dy)
    # mask epilogue on the prologue form of the input gradient, accumulating onto `old`
    r.dz = torch.where(d.ex * cv(d.e_sc) + cv(d.e_sh) > 0, r.dx_pro, torch.zeros((), dtype=torch.float64))
    r.g = cv(d.e_scale) * r.dz + d.old
    r.S1 = r.dz.sum((0, 2, 3))
    r.S2 = (r.dz * (d.ex - cv(d.e_mu)) * cv(d.e_r)).sum((0, 2, 3))
    return r


# ---- exact runs
def corners_and_centre(h, w):
    return [(0, 0), (0, w - 1), (h - 1, 0), (h - 1, w - 1), (h // 2, w // 2)]


def impulses(B, C, h, w, channels):
    t = torch.zeros(B, C, h, w, dtype=torch.float64)
    for b, ((py, px), ch) in enumerate(zip(corners_and_centre(h, w), channels)):
        t[b, ch, py, px] = 1.0
    return t


def integer_weights(N, K):
    """w[n,c,ky,kx] = 1 + 3*ky + kx + 16*(n % 4) + 64*(c % 2): every tap, four output channels and two input channels tell apart;
    integers <= 121, exact in bf16."""
    n, c = torch.arange(N).view(N, 1, 1, 1), torch.arange(K).view(1, K, 1, 1)
    ky, kx = torch.arange(3).view(1, 1, 3, 1), torch.arange(3).view(1, 1, 1, 3)
    return (1 + 3 * ky + kx + 16 * (n % 4) + 64 * (c % 2)).double()


def small_integers(seed, shape):
    g = torch.Generator().manual_seed(seed)
    return torch.randint(-2, 3, shape, generator=g).double()


@functools.lru_cache(maxsize=None)
def exact(c):
    """Operands and float64 references of an exact run: forward and input gradient of impulses through integer weights, weight
    gradient of operands drawn from {-2..2}.  Every value is an integer that bf16 (<= 256) resp. fp32 (< 2^24) holds exactly, so
    the kernels must return these references bit for bit in either storage type and in any summation order."""
    e = types.SimpleNamespace()
    e.x = impulses(c.B, c.K, c.H, c.W, EXACT_CH_IN)
    e.u = impulses(c.B, c.N, c.Ho, c.Wo, EXACT_CH_OUT)
    e.w = integer_weights(c.N, c.K)
    e.y, e.dx, _ = conv_and_grads(c, e.x, e.w, e.u)
    e.xi = small_integers(11, (c.B, c.K, c.H, c.W))
    e.gi = small_integers(12, (c.B, c.N, c.Ho, c.Wo))
    _, _, e.dw = conv_and_grads(c, e.xi, e.w, e.gi)
    e.dw_abs_bound = 4 * c.B * c.Ho * c.Wo          # |g*x| <= 4 over at most B*Ho*Wo terms: the largest partial sum in any order
    return e
