"""Thin tensor-level wrappers over the C ABI (one call = one kernel launch on the current stream).  Every launch of the package goes
through here: `lib()` is named in this module and in `_lib.py` only.

Tensors: activations are torch.bfloat16 NHWC views (B,H,W,C) whose channel pitch may exceed C (a
slice of a dense-block buffer); statistics / coefficient vectors / parameter gradients are fp32.
"""
import os

import torch

from . import _lib as L
from ._lib import (BOOT_MAX_POINTS, BOOT_MAX_TILES, BOOT_MAX_UNITS, BOOT_SENS, BOOT_SPEC, BOOT_TILE, CALIB_MAX_BINS, CALIB_MAX_ITER,
                   CALIB_METHODS, DELONG_MAX_ROWS, DELONG_TILE, DELONG_WG_ENTRIES, EPI_JOIN, EPI_MASK, EPI_STORE, HIER_MAX_LABELS, HIER_MAX_PATH, NTXENT_MAX_D, NTXENT_MAX_N, BARLOW_MAX_D, BARLOW_MAX_N,
                   KNN_MAX_CLASSES, KNN_MAX_D, KNN_MAX_K, KNN_MAX_SPLITS, PROBE_MAX_HISTORY, PROBE_MAX_SPLITS,
                   MODE_CONV, MODE_POOL2, MODE_STEM, PRO_AFFINE2, PRO_AFFINE_RELU, PRO_JOIN, PRO_NONE, CxConv, CxWgrad, check, lib, ptr, require_cuda, stream_ptr)
import ctypes as C


def _nhwc(t):
    """(B,H,W,C) view -> (B,H,W,C,pitch).  bf16 is the fast path; fp32 tensors select the fp32 storage mode (CX_DT_F32)."""
    assert t.dtype in (torch.bfloat16, torch.float32) and t.dim() == 4, "expected a bf16 (or fp32-mode) NHWC tensor"
    B, H, W, Cc = t.shape
    sb, sh, sw, sc = t.stride()
    assert sc == 1 and sh == W * sw and sb == H * sh, "NHWC slice must be dense in (B,H,W) with a channel pitch"
    return B, H, W, Cc, sw


def _dense(t, like=None):
    """_nhwc for a kernel that takes no pitch: (B,H,W,C) of a dense NHWC tensor (of `like`'s shape and storage type)."""
    B, H, W, Cc, ld = _nhwc(t)
    assert ld == Cc, "this kernel takes dense NHWC tensors (no channel pitch)"
    assert like is None or (t.shape == like.shape and t.dtype == like.dtype), "NHWC operands of one launch share shape and storage type"
    return B, H, W, Cc


def _f32(*tensors, n=0):
    """Statistics, coefficients, parameters and their gradients: contiguous fp32 of at least n elements (None: not given)."""
    for t in tensors:
        assert t is None or (t.dtype == torch.float32 and t.is_contiguous() and t.numel() >= n), "expected a contiguous fp32 tensor"


# Workspace of the reproducible weight-gradient sums (CxWgrad.scratch): one slab buffer per (device, stream) -- kernels on one stream
# are serialised, those of two streams are not.  The engines whose statistics
# are deterministic (plain DenseNet / ResNet) switch it on for their backward pass (set_det_wgrad), which makes the whole training
# step bit-reproducible; measured cost +1.3 % on DenseNet121 bs=256 (1.3 GB of slab traffic per step), none on ResNet152.
# CHEXPERT_DET_WGRAD=0 keeps the fp32 atomics everywhere.  A launch whose splits x |dW| exceed the buffer falls back to atomics.
WGRAD_SCRATCH_DEFAULT = 0 if os.environ.get("CHEXPERT_DET_WGRAD", "1") == "0" else 16 << 20
WGRAD_SCRATCH_FLOATS = 0


def set_det_wgrad(on):
    global WGRAD_SCRATCH_FLOATS
    WGRAD_SCRATCH_FLOATS = WGRAD_SCRATCH_DEFAULT if on else 0


_wgrad_scratch = {}


def wgrad_scratch(device):
    if WGRAD_SCRATCH_FLOATS <= 0:
        return None
    key = (device.index, torch.cuda.current_stream(device).cuda_stream)
    t = _wgrad_scratch.get(key)
    if t is None or t.numel() != WGRAD_SCRATCH_FLOATS:
        t = _wgrad_scratch[key] = torch.empty(WGRAD_SCRATCH_FLOATS, dtype=torch.float32, device=device)
    return t


# ---- deferred slab sums (cx_wgrad_defer): one table-driven launch per backward pass instead of one small launch per weight gradient
class _WgradArena:
    """Slab memory of one backward pass: every weight-gradient launch between defer_begin() and defer_flush() gets its own
    region (bump allocation in launch order, so the addresses -- and with them the descriptor table -- repeat from step to step),
    and the ordered sums into dw run in ONE launch at the flush.  The table lives on the device, keyed by its content: a repeated
    schedule uploads nothing (which also makes the flush capturable in a hipGraph after a warm-up step).  The arena grows to what
    a pass needed (DenseNet121 at 256 images: ~2 GB of the 288): a launch that does not fit runs its sum at once, as without
    deferral, and the next pass finds a larger arena."""
    START = int(os.environ.get("CHEXPERT_WGRAD_ARENA_MB", "256")) * (1 << 20) // 4
    MIN_FREE = 16 << 20            # a launch is only deferred while this much is left (what covers every layer, see above)

    def __init__(self, device):
        self.device = device
        self.buf = torch.empty(self.START, dtype=torch.float32, device=device)
        self.off = 0
        self.need = 0
        self.spilled = False           # a launch of the pass found less than MIN_FREE left and ran its sum at once
        self.tables = {}
        self.active = False


_arenas = {}


def _arena(device):
    a = _arenas.get(device.index)
    if a is None:
        a = _arenas[device.index] = _WgradArena(device)
    return a


def wgrad_defer_begin(device):
    """Start deferring the slab sums of this thread's weight-gradient launches (no-op without the slab workspace)."""
    if WGRAD_SCRATCH_FLOATS <= 0:
        return False
    a = _arena(device)
    if a.spilled or a.need > a.buf.numel():          # the previous pass did not fit (a spill can leave need <= numel: MIN_FREE)
        a.buf = None
        a.buf = torch.empty(int(a.need * 1.05) + a.MIN_FREE, dtype=torch.float32, device=device)
        a.tables.clear()
    a.off, a.need, a.spilled, a.active = 0, 0, False, True
    lib().cx_wgrad_defer(1)
    return True


def _wgrad_ws(device):
    """(tensor to hand to the launch as scratch, arena or None, deferred?)."""
    a = _arenas.get(device.index)
    if a is not None and a.active:
        if a.buf.numel() - a.off >= a.MIN_FREE:
            return a.buf[a.off:], a, True
        lib().cx_wgrad_defer(0)                      # this launch sums at once from the per-stream scratch
        a.spilled = True
        return wgrad_scratch(device), a, False
    return wgrad_scratch(device), None, False


def _wgrad_used(a, deferred):
    if a is not None:
        n = (lib().cx_last_slab_floats() + 63) // 64 * 64
        a.need += n
        if deferred:
            a.off += n
        else:
            lib().cx_wgrad_defer(1)


def wgrad_defer_flush(device, keep=False):
    """Add every deferred slab to its dw (one launch on the current stream, which must have been joined with the producers) and
    return to immediate sums -- or, with `keep`, go on deferring (a data-parallel backward flushes before each bucket's
    all-reduce: the gradients of the bucket are then final, the slabs of the later layers keep collecting)."""
    a = _arenas.get(device.index)
    if a is None or not a.active:
        return
    a.active = bool(keep)
    cap = 1024
    arr = (L.CxReduceDesc * cap)()
    blocks = C.c_int64(0)
    n = lib().cx_wgrad_defer_take(arr, cap, C.byref(blocks))
    if not keep:
        lib().cx_wgrad_defer(-1)
    if n < 0:
        raise RuntimeError("more than %d deferred weight-gradient sums" % cap)
    if n == 0:
        return
    key = bytes(memoryview(arr).cast("B")[:n * C.sizeof(L.CxReduceDesc)])
    t = a.tables.get(key)
    if t is None:
        if len(a.tables) > 256:
            a.tables.clear()
        # (an upload from pageable memory: not legal while a hipGraph is being captured -- the tables of a captured step are those
        # of the warm-up steps, every address in them is a persistent buffer)
        t = a.tables[key] = torch.frombuffer(bytearray(key), dtype=torch.uint8).to(device)
    check(lib().cx_dw_reduce_table(ptr(t), n, blocks.value, stream_ptr()), "cx_dw_reduce_table")


def wgrad_defer_abort(device):
    """Leave deferral without running the sums (error paths; no-op after a flush)."""
    a = _arenas.get(device.index)
    if a is not None and a.active:
        a.active = False
        lib().cx_wgrad_defer(-1)


def conv_gemm(x, w_packed, y, *, fused_dw=None, **kw):
    """cx_conv_gemm; with `fused_dw` (fp32 OIHW gradient of the forward 1x1 weight) cx_conv1x1_dgrad_wgrad instead: the input
    gradient with the mask epilogue AND the weight gradient of the same bottleneck convolution in one pass."""
    p = _conv_params(x, w_packed, y, **kw)
    if fused_dw is None:
        check(lib().cx_conv_gemm(C.byref(p), stream_ptr()), "cx_conv_gemm")
    else:
        require_cuda(fused_dw)
        assert x.dtype == torch.bfloat16, "the fused 1x1 input + weight gradient is a bf16 kernel"
        assert fused_dw.dtype == torch.float32
        ws, arena, dfr = _wgrad_ws(fused_dw.device)
        check(lib().cx_conv1x1_dgrad_wgrad_ld_ws(C.byref(p), ptr(fused_dw), _dw_pitch(fused_dw, p.N), ptr(ws),
                                                 0 if ws is None else ws.numel(), stream_ptr()), "cx_conv1x1_dgrad_wgrad_ld_ws")
        _wgrad_used(arena, dfr)
    return lib().cx_last_stat_rows() if p.stat_det else None      # stat_det: rows the consumer has to sum


def _dw_pitch(dw, n):
    """Row pitch of a (128, n[, 1, 1]) fp32 weight gradient that may be a column range of a wider matrix."""
    if dw.dim() == 1:
        assert dw.numel() == 128 * n and dw.is_contiguous()
        return n
    assert dw.shape[0] == 128 and dw.shape[1] == n and dw.numel() == 128 * n and dw.stride(1) == 1 and dw.stride(0) >= n, \
        (tuple(dw.shape), dw.stride())
    return dw.stride(0)


def conv1x1_bwd_pair(a, b, dw_a, dw_b):
    """cx_conv1x1_dgrad_wgrad_pair_ws: the fused 1x1 backward of TWO dense layers in one pass over the channels both read.  `a`
    (the later layer) and `b` are (x, w_packed, y, keywords) as `conv_gemm` takes them; dw_a may be a column range of the later
    layer's wider weight gradient.  Returns the statistic rows each layer wrote (stat_det)."""
    pa = _conv_params(a[0], a[1], a[2], **a[3])
    pb = _conv_params(b[0], b[1], b[2], **b[3])
    require_cuda(dw_a, dw_b)
    assert dw_a.dtype == torch.float32 and dw_b.dtype == torch.float32 and dw_b.is_contiguous()
    ws, arena, dfr = _wgrad_ws(dw_a.device)
    check(lib().cx_conv1x1_dgrad_wgrad_pair_ws(C.byref(pa), C.byref(pb), ptr(dw_a), _dw_pitch(dw_a, pa.N), ptr(dw_b), ptr(ws),
                                               0 if ws is None else ws.numel(), stream_ptr()), "cx_conv1x1_dgrad_wgrad_pair_ws")
    _wgrad_used(arena, dfr)
    return lib().cx_last_stat_rows() if pa.stat_det else None


def last_stat_rows():
    return lib().cx_last_stat_rows()


def last_kernel():
    """The kernel instantiation the most recent conv / weight-gradient call of this thread dispatched to, as rocprofv3 spells it;
    after an attention call (aa_attention_fwd / _weights / _bwd) the family, storage type and template arguments of what ran:
    `aa_row_fwd<3,20>`, `aa_bwd<f32,5>`, `aa_weights<bf16>`, `aa_heads_fwd<bf16,32,16>`."""
    return lib().cx_last_kernel().decode()


def last_pro_out():
    """True when the last conv_gemm of this thread wrote its `pro_out` side tensor (the selected kernel supports it)."""
    return bool(lib().cx_last_pro_out())


def kernel_hint(on=-1, form=-1):
    """CxConv.kernel_hint / CxWgrad.kernel_hint (ABI 10; include/chexpert_hip.h CX_KERNEL_HINT): pins the kernel family (on = 0 the
    generic kernels, 1 the tiled ones) and tile form of ONE call -- tests and micro-benchmarks only; 0 = the library picks."""
    return (0 if on < 0 else on + 1) | ((0 if form < 0 else form + 1) << 8)


KERNEL_HINT = 0          # default hint of the calls made while it is set (tests / scratch benchmarks: `ops.KERNEL_HINT = kernel_hint(1, 3)`)


def _conv_params(x, w_packed, y, *, N, kh=1, kw=1, stride=1, pad=0, mode=MODE_CONV, prologue=PRO_NONE, pa=None, pb=None,
                 pc=None, x2=None, epilogue=EPI_STORE, stat_sum=None, stat_sq=None, ex=None, e_sc=None, e_sh=None,
                 e_mu=None, e_r=None, e_scale=None, accumulate=False, K=None, tstride=1, stat_replicas=1, stat_rstride=0,
                 stat_det=False, pro_out=None, emask=None, x3=None, po_lo=None, po_mask=None, dil=1, hint=None):
    require_cuda(x, w_packed, y)
    p = CxConv()
    p.kernel_hint = KERNEL_HINT if hint is None else hint
    B, H, W, Cx, ldx = _nhwc(x)
    By, Ho, Wo, Cy, ldy = _nhwc(y)
    assert By == B and Cy == N
    p.x, p.w, p.y = ptr(x), ptr(w_packed), ptr(y)
    p.B, p.H, p.W, p.Ho, p.Wo = B, H, W, Ho, Wo
    p.K = (32 if mode == MODE_STEM else Cx) if K is None else K
    p.N = N
    p.ldx, p.ldy = ldx, ldy
    p.kh, p.kw, p.stride, p.pad = kh, kw, stride, pad
    p.prologue, p.mode, p.epilogue, p.accumulate = prologue, mode, epilogue, int(accumulate)
    p.dil = dil
    p.tstride = tstride
    p.pa, p.pb, p.pc = ptr(pa), ptr(pb), ptr(pc)
    if x2 is not None:
        assert x2.shape == x.shape
        p.x2, p.ldx2 = ptr(x2), _nhwc(x2)[4]
    p.stat_sum, p.stat_sq = ptr(stat_sum), ptr(stat_sq)
    p.stat_replicas, p.stat_rstride, p.stat_det = stat_replicas, stat_rstride, int(bool(stat_det))
    p.dtype = 1 if x.dtype == torch.float32 else 0
    for t_ in (w_packed, y, x2, ex):
        assert t_ is None or t_.dtype == x.dtype, "all tensors of one convolution share the storage type"
    if ex is not None:
        assert ex.shape == y.shape
        p.ex, p.ldex = ptr(ex), _nhwc(ex)[4]
    p.e_sc, p.e_sh, p.e_mu, p.e_r, p.e_scale = ptr(e_sc), ptr(e_sh), ptr(e_mu), ptr(e_r), ptr(e_scale)
    if pro_out is not None:              # dense side output of the prologue (CxConv.pro_out); last_pro_out() says whether it was written
        require_cuda(pro_out)
        assert pro_out.dtype == x.dtype and tuple(pro_out.shape) == tuple(x.shape)
        p.pro_out, p.ldpo = ptr(pro_out), _nhwc(pro_out)[4]
    if emask is not None:                # CX_EPI_JOIN: sign bits of the forward join (affine2_relu's mask)
        require_cuda(emask)
        assert emask.dtype == torch.uint8 and emask.is_contiguous() and emask.numel() * 8 == B * Ho * Wo * N
        p.emask = ptr(emask)
    if prologue == PRO_JOIN:             # the residual join of the block below as this conv1's prologue (CxConv.x3 / po_lo / po_mask)
        assert x2 is not None and pro_out is not None and x.is_contiguous() and x2.is_contiguous()
        for t_, n_ in ((x3, x.numel()), (po_lo, x.numel()), (po_mask, x.numel() // 8)):
            if t_ is not None:
                require_cuda(t_)
                assert t_.dtype in (torch.int8, torch.uint8) and t_.is_contiguous() and t_.numel() == n_
        p.x3, p.po_lo, p.po_mask = ptr(x3), ptr(po_lo), ptr(po_mask)
    p._keep = (x, w_packed, y, pa, pb, pc, x2, stat_sum, stat_sq, ex, e_sc, e_sh, e_mu, e_r, e_scale, pro_out, emask, x3, po_lo, po_mask)      # keep the views alive
    return p


def conv_wgrad(g, x, dw, *, kh=1, kw=1, stride=1, pad=0, mode=MODE_CONV, g_prologue=PRO_NONE, g2=None, ga=None, gb=None,
               gc=None, x_prologue=PRO_NONE, pa=None, pb=None, splits=0, K=None, dil=1, hint=None):
    require_cuda(g, x, dw)
    p = CxWgrad()
    p.kernel_hint = KERNEL_HINT if hint is None else hint
    p.dil = dil
    B, Ho, Wo, N, ldg = _nhwc(g)
    Bx, H, W, Cx, ldx = _nhwc(x)
    assert Bx == B and dw.dtype == torch.float32 and dw.is_contiguous()
    p.g, p.x, p.dw = ptr(g), ptr(x), ptr(dw)
    p.B, p.H, p.W, p.Ho, p.Wo = B, H, W, Ho, Wo
    p.K = (32 if mode == MODE_STEM else Cx) if K is None else K
    p.N = N
    p.ldg, p.ldx = ldg, ldx
    if g2 is not None:
        assert g2.shape == g.shape
        p.g2, p.ldg2 = ptr(g2), _nhwc(g2)[4]
    p.ga, p.gb, p.gc, p.pa, p.pb = ptr(ga), ptr(gb), ptr(gc), ptr(pa), ptr(pb)
    p.kh, p.kw, p.stride, p.pad = kh, kw, stride, pad
    p.g_prologue, p.x_prologue, p.mode, p.splits = g_prologue, x_prologue, mode, splits
    p.dtype = 1 if g.dtype == torch.float32 else 0
    assert x.dtype == g.dtype and (g2 is None or g2.dtype == g.dtype)
    ws, arena, dfr = _wgrad_ws(dw.device)
    if ws is not None:
        p.scratch, p.scratch_floats = ptr(ws), ws.numel()
    check(lib().cx_conv_wgrad(C.byref(p), stream_ptr()), "cx_conv_wgrad")
    _wgrad_used(arena, dfr)


def stem_input_grad(dz, y, pa, pb, pc, w, dx, *, stride, pad):
    """cx_stem_input_grad: dx (fp32 NCHW (B,3,H,W), overwritten) = input gradient of the stem convolution w (fp32 (C0,wc,k,k))
    at the gradient g = pa*dz + pb*y + pc (dz, y: (B,Ho,Wo,C0) NHWC in the storage type).  Raises outside the kernel's geometries
    (CX_EUNSUPPORTED): there is no other path."""
    require_cuda(dz, y, pa, pb, pc, w, dx)
    B, Ho, Wo, C0, ldz = _nhwc(dz)
    By, Hy, Wy, Cy, ldy = _nhwc(y)
    assert (By, Hy, Wy, Cy) == (B, Ho, Wo, C0) and y.dtype == dz.dtype
    assert w.dtype == torch.float32 and w.is_contiguous() and w.dim() == 4 and w.shape[0] == C0 and w.shape[2] == w.shape[3]
    assert dx.dtype == torch.float32 and dx.is_contiguous() and dx.dim() == 4 and dx.shape[:2] == (B, 3)
    for t in (pa, pb, pc):
        assert t.dtype == torch.float32 and t.is_contiguous() and t.numel() >= C0
    H, W = dx.shape[2], dx.shape[3]
    check(lib().cx_stem_input_grad(ptr(dz), ptr(y), ptr(pa), ptr(pb), ptr(pc), ptr(w), ptr(dx), ldz, ldy, w.shape[1], B, H, W, Ho, Wo, C0,
                                   w.shape[2], stride, pad, 1 if dz.dtype == torch.float32 else 0, stream_ptr()), "cx_stem_input_grad")
    return dx


def conv3x3_wgrad_batch(items):
    """cx_conv3x3_wgrad_batch: the 3x3 weight gradients of several dense layers of one block in ONE launch.
    items: [(g dense (B,H,W,32) gradient slice, x saved bottleneck tensor (B,H,W,128), pa, pb norm2 scale / shift, dw fp32 OIHW)].
    Returns False when the library declines the shape / workspace (the caller then launches cx_conv_wgrad per layer)."""
    n = len(items)
    if n == 0:
        return True
    g0, x0 = items[0][0], items[0][1]
    if n > L.WGRAD_BATCH_MAX or g0.dtype != torch.bfloat16:
        return False
    p, bt = CxWgrad(), L.CxWgradBatch()
    B, H, W, N, ldg = _nhwc(g0)
    _, _, _, K, ldx = _nhwc(x0)
    p.B, p.H, p.W, p.Ho, p.Wo, p.K, p.N = B, H, W, H, W, K, N
    p.ldg, p.ldx = ldg, ldx
    p.kh, p.kw, p.stride, p.pad = 3, 3, 1, 1
    p.g_prologue, p.x_prologue, p.mode, p.dtype = PRO_NONE, PRO_AFFINE_RELU, MODE_CONV, 0
    for i, (g, x, pa, pb, dw) in enumerate(items):
        require_cuda(g, x, dw)
        assert _nhwc(g) == (B, H, W, N, ldg) and _nhwc(x) == (B, H, W, K, ldx) and g.dtype == x.dtype == torch.bfloat16
        assert dw.dtype == torch.float32 and dw.is_contiguous() and dw.numel() == N * K * 9
        bt.g[i], bt.x[i], bt.pa[i], bt.pb[i], bt.dw[i] = ptr(g), ptr(x), ptr(pa), ptr(pb), ptr(dw)
    bt.n = n
    ws, arena, dfr = _wgrad_ws(g0.device)
    if ws is None:
        return False
    p.scratch, p.scratch_floats = ptr(ws), ws.numel()
    rc = lib().cx_conv3x3_wgrad_batch(C.byref(p), C.byref(bt), stream_ptr())
    if rc == -4:                               # CX_EUNSUPPORTED: nothing was launched
        if arena is not None and not dfr:
            lib().cx_wgrad_defer(1)
        return False
    check(rc, "cx_conv3x3_wgrad_batch")
    _wgrad_used(arena, dfr)
    return True


def pack_weights(w, transpose=False, stem=False, out=None):
    """OIHW fp32 -> packed bf16 (see cx_pack_weights)."""
    require_cuda(w)
    O, I, kh, kw = w.shape
    n = 7 * O * 32 if stem else kh * kw * O * I
    if out is None:
        out = torch.empty(n, dtype=torch.bfloat16, device=w.device)
    assert w.is_contiguous() and w.dtype == torch.float32 and out.numel() >= n
    check(lib().cx_pack_weights(ptr(w), ptr(out), O, I, kh, kw, int(transpose), int(stem), stream_ptr()), "cx_pack_weights")
    return out


def _fn(name, t):
    """C entry point for the storage type of tensor t (bf16 or the fp32 mode)."""
    return getattr(lib(), name + "_f32" if t.dtype == torch.float32 else name)


def pack_weights_table(flat, packed, desc_dev, n_desc):
    if packed.dtype == torch.float32:
        check(lib().cx_pack_weights_table_f32(ptr(flat), ptr(packed), ptr(desc_dev), n_desc, stream_ptr()), "cx_pack_weights_table_f32")
    else:
        check(lib().cx_pack_weights_table(ptr(flat), ptr(packed), ptr(desc_dev), n_desc, stream_ptr()), "cx_pack_weights_table")


def u8_to_nhwc4(x, out=None, mean=0.5330, std=0.0349):
    """uint8 grey images (B,1,H,W) or (B,H,W) -> whitened, channel-expanded (B,H,W,4) bf16 (chexpert.py:70-72 on the GPU)."""
    require_cuda(x)
    assert x.dtype == torch.uint8 and x.is_contiguous()
    if x.dim() == 4:
        assert x.shape[1] == 1
        B, _, H, W = x.shape
    else:
        B, H, W = x.shape
    if out is None:
        out = torch.empty(B, H, W, 4, dtype=torch.bfloat16, device=x.device)
    check(_fn("cx_u8_to_nhwc4", out)(ptr(x), ptr(out), B * H * W, mean, std, stream_ptr()), "cx_u8_to_nhwc4")
    return out


def u8_jitter(x, brightness, contrast, order, out=None):
    """ColorJitter(brightness, contrast) of explore_data.ipynb cell 6 on decoded grey bytes (B,1,H,W) / (B,H,W) uint8, on the GPU;
    brightness / contrast: fp32 (B,) factors, order: int32 (B,), 0 = brightness first."""
    require_cuda(x, brightness, contrast, order)
    assert x.dtype == torch.uint8 and x.is_contiguous() and order.dtype == torch.int32
    B = x.shape[0]
    HW = x.numel() // B
    if out is None:
        out = torch.empty_like(x)
    check(lib().cx_u8_jitter(ptr(x), ptr(out), B, HW, ptr(brightness), ptr(contrast), ptr(order), stream_ptr()), "cx_u8_jitter")
    return out


def u8_affine(x, mat, fill=0, out=None):
    """Random-affine warp of decoded grey bytes (B,1,H,W) / (B,H,W) uint8 on the GPU (cx_u8_affine: bilinear, taps outside the image
    read `fill`); mat: fp32 (B,6) inverse maps in pixel units about the image centre (chexpert_amd.augment.affine_matrices)."""
    require_cuda(x, mat, out)
    assert x.dtype == torch.uint8 and x.is_contiguous() and x.dim() in (3, 4) and (x.dim() == 3 or x.shape[1] == 1)
    B, H, W = x.shape[0], x.shape[-2], x.shape[-1]
    assert mat.dtype == torch.float32 and mat.is_contiguous() and tuple(mat.shape) == (B, 6)
    if out is None:
        out = torch.empty_like(x)
    assert out.dtype == torch.uint8 and out.shape == x.shape and out.is_contiguous()
    check(lib().cx_u8_affine(ptr(x), ptr(out), B, H, W, ptr(mat), int(fill), stream_ptr()), "cx_u8_affine")
    return out


def _plan_i32(v, shape, name):
    assert v.dtype == torch.int32 and v.is_contiguous() and tuple(v.shape) == shape, "%s: int32 %s expected" % (name, shape)


def u8_mix(x, perm, lam_q, box, fill=0, out=None):
    """Mixup / CutMix / random erasing of decoded grey bytes (B,1,H,W) / (B,H,W) uint8 on the GPU (cx_u8_mix, integers throughout):
    inside row b's box (y0 y1 x0 x1, clamped to the image) y = (q*x[b] + (65536 - q)*o + 32768) >> 16 with q = lam_q[b] and
    o = x[perm[b]], or `fill` where perm[b] < 0; outside it y = x[b].  perm, lam_q: int32 (B,), box: int32 (B,4)
    (chexpert_amd.augment.mix_plan / erase_plan).  `out` must not be x."""
    require_cuda(x, perm, lam_q, box, out)
    assert x.dtype == torch.uint8 and x.is_contiguous() and x.dim() in (3, 4) and (x.dim() == 3 or x.shape[1] == 1)
    B, H, W = x.shape[0], x.shape[-2], x.shape[-1]
    _plan_i32(perm, (B,), "perm"), _plan_i32(lam_q, (B,), "lam_q"), _plan_i32(box, (B, 4), "box")
    if out is None:
        out = torch.empty_like(x)
    assert out.dtype == torch.uint8 and out.shape == x.shape and out.is_contiguous()
    check(lib().cx_u8_mix(ptr(x), ptr(out), B, H, W, ptr(perm), ptr(lam_q), ptr(box), int(fill), stream_ptr()), "cx_u8_mix")
    return out


def target_mix(t, perm, tw_q, out=None):
    """The targets that go with u8_mix (cx_target_mix): t fp32 (B, n); out[b] = w*t[b] + (1 - w)*t[perm[b]] with w = tw_q[b] / 65536,
    every product and sum rounded on its own; -1 where either label is < 0 (ignored stays ignored); t[b] where perm[b] < 0 or
    tw_q[b] == 65536.  perm, tw_q: int32 (B,).  `out` must not be t."""
    require_cuda(t, perm, tw_q, out)
    assert t.dtype == torch.float32 and t.is_contiguous() and t.dim() == 2
    B, n = t.shape
    _plan_i32(perm, (B,), "perm"), _plan_i32(tw_q, (B,), "tw_q")
    if out is None:
        out = torch.empty_like(t)
    assert out.dtype == torch.float32 and out.shape == t.shape and out.is_contiguous()
    check(lib().cx_target_mix(ptr(t), ptr(out), B, n, ptr(perm), ptr(tw_q), stream_ptr()), "cx_target_mix")
    return out


def _u8_images(x):
    assert x.dtype == torch.uint8 and x.is_contiguous() and x.dim() in (3, 4) and (x.dim() == 3 or x.shape[1] == 1)
    return x.shape[0], x.shape[-2], x.shape[-1]


def u8_clahe_lut(x, grid, clip_count):
    """Stage 1 of CLAHE (cx_u8_clahe_lut): the (B, GY, GX, 256) uint8 equalisation tables of decoded grey bytes (B,1,H,W) / (B,H,W)
    uint8 on the GPU; grid = (GY, GX), clip_count = the integer clip level per bin (chexpert_amd.augment.clahe_clip_count; 0: none)."""
    require_cuda(x)
    B, H, W = _u8_images(x)
    GY, GX = int(grid[0]), int(grid[1])
    lut = torch.empty(B, max(GY, 0), max(GX, 0), 256, dtype=torch.uint8, device=x.device)
    check(lib().cx_u8_clahe_lut(ptr(x), ptr(lut), B, H, W, GY, GX, int(clip_count), stream_ptr()), "cx_u8_clahe_lut")
    return lut


def u8_clahe_apply(x, lut, out=None):
    """Stage 2 of CLAHE (cx_u8_clahe_apply): every pixel through the bilinear blend of the four tables around it; lut: (B, GY, GX, 256)
    uint8 as u8_clahe_lut returns it.  `out` must not be x."""
    require_cuda(x, lut, out)
    B, H, W = _u8_images(x)
    assert lut.dtype == torch.uint8 and lut.is_contiguous() and lut.dim() == 4 and lut.shape[0] == B and lut.shape[3] == 256
    if out is None:
        out = torch.empty_like(x)
    assert out.dtype == torch.uint8 and out.shape == x.shape and out.is_contiguous()
    check(lib().cx_u8_clahe_apply(ptr(x), ptr(lut), ptr(out), B, H, W, lut.shape[1], lut.shape[2], stream_ptr()), "cx_u8_clahe_apply")
    return out


def u8_clahe(x, grid=(8, 8), clip_limit=2.0, out=None):
    """Contrast-limited adaptive histogram equalisation of decoded grey bytes on the GPU: both stages (two launches).  The structure
    is OpenCV's createCLAHE(clipLimit, tileGridSize); the arithmetic is the integer definition of chexpert_amd/augment.py, not
    bit-equal to OpenCV's float rounding."""
    from .augment import clahe_clip_count
    B, H, W = _u8_images(x)
    GY, GX = int(grid[0]), int(grid[1])
    if GY < 1 or GX < 1 or H % GY or W % GX:
        raise RuntimeError("u8_clahe: grid %s does not divide a %d x %d image (unsupported shape)" % ((GY, GX), H, W))
    return u8_clahe_apply(x, u8_clahe_lut(x, (GY, GX), clahe_clip_count(clip_limit, H // GY, W // GX)), out)


def nchw3_to_nhwc4(x, out=None):
    require_cuda(x)
    B, Cc, H, W = x.shape
    assert Cc == 3 and x.dtype == torch.float32 and x.is_contiguous()
    if out is None:
        out = torch.empty(B, H, W, 4, dtype=torch.bfloat16, device=x.device)
    check(_fn("cx_nchw3_to_nhwc4", out)(ptr(x), ptr(out), B, H, W, stream_ptr()), "cx_nchw3_to_nhwc4")
    return out


def u8_to_nhwc8(x, out, mean=0.5330, std=0.0349):
    """cx_u8_to_nhwc8: uint8 grey images (B,1,H,W) -> whitened (B,H,W,8) in out's storage type (3 equal channels + 5 zeros)."""
    require_cuda(x, out)
    B, H, W, Cc = _dense(out)
    assert x.dtype == torch.uint8 and x.is_contiguous() and tuple(x.shape) == (B, 1, H, W) and Cc == 8
    check(_fn("cx_u8_to_nhwc8", out)(ptr(x), ptr(out), B * H * W, mean, std, stream_ptr()), "cx_u8_to_nhwc8")


def nchw3_to_nhwc8(x, out):
    """cx_nchw3_to_nhwc8: fp32 (B,3,H,W) -> (B,H,W,8) in out's storage type (the 3 channels + 5 zeros)."""
    require_cuda(x, out)
    B, H, W, Cc = _dense(out)
    assert x.dtype == torch.float32 and x.is_contiguous() and tuple(x.shape) == (B, 3, H, W) and Cc == 8
    check(_fn("cx_nchw3_to_nhwc8", out)(ptr(x), ptr(out), B, H, W, stream_ptr()), "cx_nchw3_to_nhwc8")


def chan_map_table(real, padded, table, n_desc, direction, accumulate=0):
    """cx_chan_map_table: copies (direction 0: real -> padded, 1: padded -> real, `accumulate`: added) between the flat fp32 buffers
    of a network and of its channel-padded twin, as the n_desc CxChanMapDesc of `table` (uint8 bytes on the device) say."""
    require_cuda(real, padded, table)
    _f32(real, padded)
    assert table.dtype == torch.uint8 and table.is_contiguous() and table.numel() == n_desc * C.sizeof(L.CxChanMapDesc)
    check(lib().cx_chan_map_table(ptr(real), ptr(padded), ptr(table), n_desc, direction, accumulate, stream_ptr()), "cx_chan_map_table")


def bn_coef(s, q, count, gamma, beta, eps, momentum, rmean, rvar, scale, shift, mean, rstd, Cn=None, replicas=1, rstride=0):
    Cn = Cn if Cn is not None else s.numel()
    check(lib().cx_bn_coef(ptr(s), ptr(q), float(count), ptr(gamma), ptr(beta), eps, momentum, ptr(rmean), ptr(rvar),
                           ptr(scale), ptr(shift), ptr(mean), ptr(rstd), Cn, replicas, rstride, stream_ptr()), "cx_bn_coef")


def bn_coef_moments(mean, rstd, count, gamma, beta, eps, momentum, rmean, rvar, scale, shift, Cn, fresh=None):
    """cx_bn_coef_moments; fresh = (sum, sq, rows, rstride, c_lo, c_n) reduces those channels from deterministic statistic rows first."""
    fs, fq, rows, rstride, c_lo, c_n = fresh if fresh is not None else (None, None, 0, 0, 0, 0)
    check(lib().cx_bn_coef_moments(ptr(mean), ptr(rstd), float(count), ptr(gamma), ptr(beta), eps, momentum, ptr(rmean), ptr(rvar),
                                   ptr(scale), ptr(shift), Cn, ptr(fs), ptr(fq), rows, rstride, c_lo, c_n, stream_ptr()),
          "cx_bn_coef_moments")


def bn_coef_eval(rmean, rvar, gamma, beta, eps, scale, shift, mean, rstd, Cn=None):
    Cn = Cn if Cn is not None else rmean.numel()
    check(lib().cx_bn_coef_eval(ptr(rmean), ptr(rvar), ptr(gamma), ptr(beta), eps, ptr(scale), ptr(shift), ptr(mean),
                                ptr(rstd), Cn, stream_ptr()), "cx_bn_coef_eval")


def bn_bwd_coef(S1, S2, count, gamma, mean, rstd, dgamma, dbeta, A, Bc, pa, pb, pc, Cn, replicas=1, rstride=0, q=None):
    """q = (qa, qb, qc, q_lo, q_n): also emit the slice coefficients (cx_bn_bwd_slice_coef) of channels [q_lo, q_lo + q_n)."""
    qa, qb, qc, q_lo, q_n = q if q is not None else (None, None, None, 0, 0)
    check(lib().cx_bn_bwd_coef(ptr(S1), ptr(S2), float(count), ptr(gamma), ptr(mean), ptr(rstd), ptr(dgamma), ptr(dbeta),
                               ptr(A), ptr(Bc), ptr(pa), ptr(pb), ptr(pc), Cn, replicas, rstride, ptr(qa), ptr(qb), ptr(qc), q_lo, q_n,
                               stream_ptr()), "cx_bn_bwd_coef")


def bn_bwd_coef_eval(S1, S2, mean, rstd, rmean, rvar, gamma, eps, dgamma, dbeta, pa, pb, pc, Cn, replicas=1, rstride=0, q=None):
    """cx_bn_bwd_coef_eval: the frozen (running-statistic) form of bn_bwd_coef.  (mean, rstd) is the basis the producer reduced S2
    against, (rmean, rvar) the BatchNorm's running statistics; q = (qa, qb, qc, q_lo, q_n): also write the identity slice
    coefficients (1, 0, 0) of channels [q_lo, q_lo + q_n)."""
    qa, qb, qc, q_lo, q_n = q if q is not None else (None, None, None, 0, 0)
    check(lib().cx_bn_bwd_coef_eval(ptr(S1), ptr(S2), ptr(mean), ptr(rstd), ptr(rmean), ptr(rvar), ptr(gamma), float(eps), ptr(dgamma),
                                    ptr(dbeta), ptr(pa), ptr(pb), ptr(pc), Cn, replicas, rstride, ptr(qa), ptr(qb), ptr(qc), q_lo, q_n,
                                    stream_ptr()), "cx_bn_bwd_coef_eval")


def bn_bwd_slice_coef(A, Bc, mean, rstd, pa, pb, pc, Cn):
    check(lib().cx_bn_bwd_slice_coef(ptr(A), ptr(Bc), ptr(mean), ptr(rstd), ptr(pa), ptr(pb), ptr(pc), Cn, stream_ptr()),
          "cx_bn_bwd_slice_coef")


def dropout_slice_fwd(y, p, seed, uid, S1=None, S2=None, stat_rows=0):
    """cx_dropout_slice_fwd: dropout in place on the channel slice y (a (B,H,W,C) view of a wider NHWC buffer); returns the statistic
    rows written (S1 / S2 given)."""
    B, H, W, Cc, ld = _nhwc(y)
    require_cuda(y, seed)
    assert seed.dtype == torch.int64
    check(_fn("cx_dropout_slice_fwd", y)(ptr(y), ld, B * H * W, Cc, float(p), ptr(seed), int(uid), ptr(S1), ptr(S2), stat_rows,
                                         stream_ptr()), "cx_dropout_slice_fwd")
    return lib().cx_last_stat_rows() if S1 is not None else None


def dropout_slice_bwd(g, x, qa, qb, qc, p, seed, uid):
    """cx_dropout_slice_bwd: g <- keep ? (qa g + qb x + qc) / (1 - p) : 0 in place on the gradient slice."""
    B, H, W, Cc, ldg = _nhwc(g)
    assert x.shape == g.shape and seed.dtype == torch.int64
    require_cuda(g, x, seed)
    check(_fn("cx_dropout_slice_bwd", g)(ptr(g), ldg, ptr(x), _nhwc(x)[4], ptr(qa), ptr(qb), ptr(qc), B * H * W, Cc, float(p), ptr(seed),
                                         int(uid), stream_ptr()), "cx_dropout_slice_bwd")


def bnrelu_maxpool_fwd(x, scale, shift, y, argmax, stat_sum, stat_sq, stat_rows=0):
    B, H, W, Cc, ldx = _nhwc(x)
    assert ldx == Cc
    ldy = _nhwc(y)[4]
    check(_fn("cx_bnrelu_maxpool_fwd", x)(ptr(x), ptr(scale), ptr(shift), ptr(y), ptr(argmax), ptr(stat_sum), ptr(stat_sq),
                                      B, H, W, Cc, ldy, stat_rows, stream_ptr()), "cx_bnrelu_maxpool_fwd")
    return lib().cx_last_stat_rows() if stat_rows else None


def bnrelu_maxpool_bwd(x, scale, shift, mean, rstd, argmax, g, gx, ga, gb, gc, dz, S1, S2, stat_rows=0):
    B, H, W, Cc, ldx = _nhwc(x)
    assert ldx == Cc and _nhwc(dz)[4] == Cc
    check(_fn("cx_bnrelu_maxpool_bwd", x)(ptr(x), ptr(scale), ptr(shift), ptr(mean), ptr(rstd), ptr(argmax), ptr(g), ptr(gx),
                                      ptr(ga), ptr(gb), ptr(gc), ptr(dz), ptr(S1), ptr(S2), B, H, W, Cc, _nhwc(g)[4],
                                      _nhwc(gx)[4], stat_rows, stream_ptr()), "cx_bnrelu_maxpool_bwd")
    return lib().cx_last_stat_rows() if stat_rows else None


def head_fwd(x, scale, shift, w, bias, pooled, logits):
    B, H, W, Cc, ldx = _nhwc(x)
    check(_fn("cx_head_fwd", x)(ptr(x), ptr(scale), ptr(shift), ptr(w), ptr(bias), ptr(pooled), ptr(logits), B, H * W, Cc, ldx,
                            logits.shape[1], stream_ptr()), "cx_head_fwd")


def bce_fwd_bwd(logits, target, loss, loss_elem, dlogits, grad_scale=1.0):
    B, n = logits.shape
    check(lib().cx_bce_fwd_bwd(ptr(logits), ptr(target), ptr(loss), ptr(loss_elem), ptr(dlogits), grad_scale, B, n,
                               stream_ptr()), "cx_bce_fwd_bwd")


def _loss_operands(logits, target, vectors=(), loss=None, outputs=()):
    """The operands the loss wrappers share (AssertionError): contiguous fp32 (B, n) logits and targets, optional per-class `vectors`
    (n,), an optional one-float `loss` and optional (B, n) `outputs`, every one on the logits' device.  Returns (B, n).  Where
    require_cuda stands beside it is each wrapper's own: it decides which of the two errors a call that earns both gets."""
    assert logits.dim() == 2 and logits.dtype == torch.float32 and logits.is_contiguous()
    B, n = logits.shape
    assert target.dtype == torch.float32 and target.is_contiguous() and tuple(target.shape) == (B, n)
    assert all(v is None or tuple(v.shape) == (n,) for v in vectors)
    assert all(o is None or tuple(o.shape) == (B, n) for o in outputs)
    assert all(t is None or t.device == logits.device for t in (target, loss, *vectors, *outputs))
    _f32(loss, n=1)
    _f32(*vectors, *outputs)
    return B, n


def bce_masked_fwd_bwd(logits, target, pos_weight, loss, loss_elem, dlogits, grad_scale=1.0):
    """bce_fwd_bwd in which a target < 0 is ignored (no loss, no gradient; the divisor stays B) and pos_weight (fp32 (n,), or None)
    weights the positive term per class as torch's BCEWithLogitsLoss(pos_weight) does.  loss, loss_elem and dlogits are optional."""
    require_cuda(logits, target, pos_weight, loss, loss_elem, dlogits)
    B, n = _loss_operands(logits, target, (pos_weight,), loss, (loss_elem, dlogits))
    check(lib().cx_bce_masked_fwd_bwd(ptr(logits), ptr(target), ptr(pos_weight), ptr(loss), ptr(loss_elem), ptr(dlogits), grad_scale,
                                      B, n, stream_ptr()), "cx_bce_masked_fwd_bwd")


def aucm_fwd_bwd(logits, target, prior, aux, margin, loss, loss_class, dlogits, daux, grad_scale=1.0):
    """The AUC min-max-margin loss of the (B, n) logits with its gradients in one launch (cx_aucm_fwd_bwd): prior fp32 (n,) in (0, 1),
    aux fp32 (3, n) = rows a, b, alpha, margin > 0; a target < 0 is ignored, t >= 0.5 is a positive.  loss (1,), loss_class (n,),
    dlogits (B, n) and daux (3, n) are optional; grad_scale multiplies dlogits alone."""
    require_cuda(logits, target, prior, aux, loss, loss_class, dlogits, daux)
    assert prior is not None
    B, n = _loss_operands(logits, target, (prior, loss_class), loss, (dlogits,))
    assert tuple(aux.shape) == (3, n) and (daux is None or tuple(daux.shape) == (3, n))
    assert aux.device == logits.device and (daux is None or daux.device == logits.device)
    _f32(aux, daux)
    check(lib().cx_aucm_fwd_bwd(ptr(logits), ptr(target), ptr(prior), ptr(aux), float(margin), ptr(loss), ptr(loss_class), ptr(dlogits),
                                ptr(daux), grad_scale, B, n, stream_ptr()), "cx_aucm_fwd_bwd")


def aucm_aux_step(aux, daux, lr_aux):
    """a -= lr da, b -= lr db, alpha = max(0, alpha + lr dalpha) on the (3, n) auxiliary scalars of aucm_fwd_bwd; lr_aux is a one-float
    DEVICE tensor, read by the kernel (a captured step sees a changed rate)."""
    require_cuda(aux, daux, lr_aux)
    assert aux.dim() == 2 and aux.shape[0] == 3 and tuple(daux.shape) == tuple(aux.shape) and lr_aux.numel() == 1
    assert daux.device == aux.device and lr_aux.device == aux.device
    _f32(aux, daux, n=aux.numel())
    _f32(lr_aux, n=1)
    check(lib().cx_aucm_aux_step(ptr(aux), ptr(daux), ptr(lr_aux), aux.shape[1], stream_ptr()), "cx_aucm_aux_step")


def asl_fwd_bwd(logits, target, pos_weight, focus, loss, loss_elem, dlogits, grad_scale=1.0):
    """The focal / asymmetric loss of the (B, n) logits with d loss / d logits in one launch (cx_asl_fwd_bwd): focus is a four-float
    DEVICE tensor [gamma+, gamma-, clip, alpha or -1], read by the kernel (a captured step sees a changed value); a target < 0 is
    ignored, pos_weight (fp32 (n,), or None) weights the positive term.  loss (1,), loss_elem and dlogits (B, n) are optional;
    grad_scale multiplies dlogits alone."""
    B, n = _loss_operands(logits, target, (pos_weight,), loss, (loss_elem, dlogits))
    assert focus is not None and tuple(focus.shape) == (4,) and focus.device == logits.device
    _f32(focus)
    require_cuda(logits, target, pos_weight, focus, loss, loss_elem, dlogits)
    check(lib().cx_asl_fwd_bwd(ptr(logits), ptr(target), ptr(pos_weight), ptr(focus), ptr(loss), ptr(loss_elem), ptr(dlogits), grad_scale,
                               B, n, stream_ptr()), "cx_asl_fwd_bwd")


def _mc3_logits(logits):
    """The (B, 3n) logits of the three-way softmax (AssertionError): contiguous fp32, three outputs per finding.  Returns (B, n)."""
    assert logits.dim() == 2 and logits.dtype == torch.float32 and logits.is_contiguous()
    assert logits.shape[0] >= 1 and logits.shape[1] >= 3 and logits.shape[1] % 3 == 0
    return logits.shape[0], logits.shape[1] // 3


def mc3_fwd_bwd(logits, target, class_weight, loss, loss_elem, dlogits, grad_scale=1.0):
    """The three-way softmax cross-entropy of U-MultiClass with d loss / d logits in one launch (cx_mc3_fwd_bwd): logits (B, 3n), finding
    k owning columns 3k (negative), 3k + 1 (positive), 3k + 2 (uncertain); target the (B, n) table, class 2 where t < 0, 1 where
    t >= 0.5, else 0; class_weight fp32 (n, 3) or None.  loss (1,), loss_elem (B, n) and dlogits (B, 3n) are optional; grad_scale
    multiplies dlogits alone."""
    B, n = _mc3_logits(logits)
    assert target.dtype == torch.float32 and target.is_contiguous() and tuple(target.shape) == (B, n)
    assert class_weight is None or tuple(class_weight.shape) == (n, 3)
    assert loss_elem is None or tuple(loss_elem.shape) == (B, n)
    assert dlogits is None or tuple(dlogits.shape) == (B, 3 * n)
    assert all(t is None or t.device == logits.device for t in (target, class_weight, loss, loss_elem, dlogits))
    _f32(loss, n=1)
    _f32(class_weight, loss_elem, dlogits)
    require_cuda(logits, target, class_weight, loss, loss_elem, dlogits)
    check(lib().cx_mc3_fwd_bwd(ptr(logits), ptr(target), ptr(class_weight), ptr(loss), ptr(loss_elem), ptr(dlogits), grad_scale, B, n,
                               stream_ptr()), "cx_mc3_fwd_bwd")


def mc3_collapse(logits, z, p_unc=None):
    """The binary logits of (B, 3n) three-way logits (cx_mc3_collapse): z (B, n) = z1 - z0, whose sigmoid is p1 / (p0 + p1), and, where
    given, p_unc (B, n), the softmax probability of "uncertain".  Returns z."""
    B, n = _mc3_logits(logits)
    assert z is not None and tuple(z.shape) == (B, n) and (p_unc is None or tuple(p_unc.shape) == (B, n))
    assert all(t is None or t.device == logits.device for t in (z, p_unc))
    _f32(z, p_unc)
    require_cuda(logits, z, p_unc)
    check(lib().cx_mc3_collapse(ptr(logits), ptr(z), ptr(p_unc), B, n, stream_ptr()), "cx_mc3_collapse")
    return z


HIER_MODES = {"conditional": 0, "unconditional": 1}          # cx_hier_fwd_bwd's mode


def check_hier_parent(who, parent, n=None):
    """The parent table of the hierarchical loss, checked on the host (ValueError in the name of `who`) and returned as a CPU int32
    vector: at most HIER_MAX_LABELS entries (n of them where n is given), entry k either -1 (a root) or in [0, k) (parents come
    before children, so the table has no cycle), no path -- a node and its ancestors -- longer than HIER_MAX_PATH."""
    try:
        p = torch.as_tensor(parent).detach().cpu().reshape(-1)
        if p.numel() and (p.dtype.is_floating_point or p.dtype == torch.bool) and not bool((p == p.round()).all()):
            raise ValueError
        p = p.to(torch.int64)
    except (TypeError, ValueError, RuntimeError):
        raise ValueError("%s takes a parent table of integers (got %r)" % (who, parent))
    if p.numel() < 1 or p.numel() > HIER_MAX_LABELS or (n is not None and p.numel() != n):
        raise ValueError("%s takes a parent table of %s entries (got %d)"
                         % (who, "1 .. %d" % HIER_MAX_LABELS if n is None else "%d, one per output of the head" % n, p.numel()))
    table, depth = p.tolist(), []
    for k, a in enumerate(table):
        if a < -1 or a >= k:
            raise ValueError("%s: parent[%d] = %d; an entry is -1 (a root) or the index of an EARLIER label" % (who, k, a))
        depth.append(1 if a < 0 else depth[a] + 1)
        if depth[k] > HIER_MAX_PATH:
            raise ValueError("%s: label %d has %d ancestors; a path holds at most %d labels" % (who, k, depth[k] - 1, HIER_MAX_PATH))
    return p.to(torch.int32)


def _hier_parent(who, parent, n, device):
    """The table as the kernels take it: an int32 (n,) tensor on `device` is the caller's to have checked (Loss.set did: its values
    stay on the device); anything on the host -- a list, a CPU tensor -- is checked here and copied over."""
    if isinstance(parent, torch.Tensor) and parent.is_cuda:
        assert parent.dtype == torch.int32 and parent.is_contiguous() and tuple(parent.shape) == (n,) and parent.device == device
        return parent
    p = check_hier_parent(who, parent, n)
    return p if device.type != "cuda" else p.to(device)


def hier_fwd_bwd(logits, target, parent, pos_weight, mode, loss, loss_elem, dlogits, grad_scale=1.0):
    """The hierarchical label loss of the (B, n) logits with d loss / d logits in one launch (cx_hier_fwd_bwd): parent the int32 (n,)
    table ON THE DEVICE, read by the kernel (a captured step sees a table rewritten in place), or a host table, which is checked
    (check_hier_parent) and copied over; mode 0 / 'conditional' or 1 / 'unconditional', passed by value; a target < 0 is ignored,
    pos_weight (fp32 (n,), or None) weights the positive term.  loss (1,), loss_elem and dlogits (B, n) are optional; grad_scale
    multiplies dlogits alone."""
    if isinstance(mode, str):
        mode = HIER_MODES.get(mode)
    if not isinstance(mode, int) or isinstance(mode, bool) or mode not in (0, 1):
        raise ValueError("hier_fwd_bwd takes mode 0 / 'conditional' or 1 / 'unconditional' (got %r)" % (mode,))
    if logits.dim() == 2 and logits.shape[1] > HIER_MAX_LABELS:
        raise ValueError("hier_fwd_bwd takes at most %d labels (got %d)" % (HIER_MAX_LABELS, logits.shape[1]))
    B, n = _loss_operands(logits, target, (pos_weight,), loss, (loss_elem, dlogits))
    assert B >= 1 and n >= 1
    parent = _hier_parent("hier_fwd_bwd", parent, n, logits.device)
    require_cuda(logits, target, parent, pos_weight, loss, loss_elem, dlogits)
    check(lib().cx_hier_fwd_bwd(ptr(logits), ptr(target), ptr(parent), ptr(pos_weight), mode, ptr(loss), ptr(loss_elem), ptr(dlogits),
                                grad_scale, B, n, stream_ptr()), "cx_hier_fwd_bwd")


def hier_collapse(logits, parent, z, p=None):
    """The unconditional logits of (B, n) conditional ones (cx_hier_collapse): a root's z is its logit bit for bit, any other
    z = log P - log(1 - P) of the product P of the sigmoids along its path, so that sigmoid(z) = P; p (optional) = P.  parent as
    in hier_fwd_bwd.  Returns z."""
    assert logits.dim() == 2 and logits.dtype == torch.float32 and logits.is_contiguous() and logits.shape[0] >= 1 and logits.shape[1] >= 1
    B, n = logits.shape
    if n > HIER_MAX_LABELS:
        raise ValueError("hier_collapse takes at most %d labels (got %d)" % (HIER_MAX_LABELS, n))
    assert z is not None and tuple(z.shape) == (B, n) and (p is None or tuple(p.shape) == (B, n))
    assert all(t is None or t.device == logits.device for t in (z, p))
    _f32(z, p)
    parent = _hier_parent("hier_collapse", parent, n, logits.device)
    require_cuda(logits, parent, z, p)
    check(lib().cx_hier_collapse(ptr(logits), ptr(parent), ptr(z), ptr(p), B, n, stream_ptr()), "cx_hier_collapse")
    return z


def ntxent_scratch(N, d):
    """The floats of scratch ntxent_fwd_bwd needs for (N, d) embeddings (cx_ntxent_scratch): N d + 4 N, for the normalised rows, their
    norms, and each row's log-sum-exp, 1 / |P| and loss.  Sizes the loss refuses are a ValueError."""
    N, d = int(N), int(d)
    if not (1 <= N <= NTXENT_MAX_N and 1 <= d <= NTXENT_MAX_D):
        raise ValueError("the contrastive loss takes 1 .. %d rows of 1 .. %d values (got %d x %d)" % (NTXENT_MAX_N, NTXENT_MAX_D, N, d))
    return int(lib().cx_ntxent_scratch(N, d))


def ntxent_fwd_bwd(logits, ids, temperature, loss, loss_elem, dlogits, top1=None, scratch=None, grad_scale=1.0):
    """The NT-Xent / SupCon loss of the (N, d) embeddings with its exact gradient (cx_ntxent_fwd_bwd, three launches; the definition
    stands in include/chexpert_hip.h): ids fp32 (N, 1), integer-valued, rows with the same id >= 0 are each other's positives and a
    row with an id < 0 is out of the batch; temperature a one-float DEVICE tensor, read by the kernels (a captured step sees a changed
    value).  loss (1,), loss_elem (N, 1), dlogits (N, d) and top1 (N,) int32 -- each row's nearest other row -- are optional;
    grad_scale multiplies dlogits alone.  scratch: fp32, at least ntxent_scratch(N, d) floats (None: allocated here, which a graph
    capture must not do -- hold one).  Returns the scratch."""
    assert logits.dim() == 2 and logits.dtype == torch.float32 and logits.is_contiguous()
    N, d = logits.shape
    need = ntxent_scratch(N, d)
    assert ids.dtype == torch.float32 and ids.is_contiguous() and tuple(ids.shape) == (N, 1)
    assert temperature is not None and temperature.numel() == 1
    assert loss_elem is None or tuple(loss_elem.shape) == (N, 1)
    assert dlogits is None or tuple(dlogits.shape) == (N, d)
    assert top1 is None or (top1.dtype == torch.int32 and top1.is_contiguous() and tuple(top1.shape) == (N,))
    if scratch is None:
        scratch = torch.empty(need, dtype=torch.float32, device=logits.device)
    assert scratch.dim() == 1 and scratch.numel() >= need
    assert all(t is None or t.device == logits.device for t in (ids, temperature, loss, loss_elem, dlogits, top1, scratch))
    _f32(loss, temperature, n=1)
    _f32(loss_elem, dlogits)
    _f32(scratch, n=scratch.numel())
    require_cuda(logits, ids, temperature, loss, loss_elem, dlogits, top1, scratch)
    check(lib().cx_ntxent_fwd_bwd(ptr(logits), ptr(ids), ptr(temperature), ptr(loss), ptr(loss_elem), ptr(dlogits), ptr(top1), grad_scale,
                                  ptr(scratch), scratch.numel(), N, d, stream_ptr()), "cx_ntxent_fwd_bwd")
    return scratch


def knn_scratch(Q, M, k, splits=0):
    """The floats of scratch knn_topk needs (cx_knn_scratch): Q x slices x k 64-bit keys, `splits` = 0 being the library's own choice of
    slices.  Sizes the search refuses are a ValueError."""
    Q, M, k, splits = int(Q), int(M), int(k), int(splits)
    if not (Q >= 1 and 1 <= M < 2 ** 31 and 1 <= k <= KNN_MAX_K and 0 <= splits <= KNN_MAX_SPLITS):
        raise ValueError("the search takes Q >= 1 queries, 1 <= M < 2^31 bank rows, 1 <= k <= %d and 0 <= splits <= %d (got Q %d, M %d, k %d, "
                         "splits %d)" % (KNN_MAX_K, KNN_MAX_SPLITS, Q, M, k, splits))
    return int(lib().cx_knn_scratch(Q, M, k, splits))


def knn_normalize(x, y):
    """y = x / max(|x|, 1e-12) per row of the (rows, d) fp32 matrix (cx_knn_normalize), the normalisation of the contrastive loss."""
    assert x.dim() == 2 and y.shape == x.shape
    _f32(x, y)
    require_cuda(x, y)
    rows, d = x.shape
    if not 1 <= d <= KNN_MAX_D:
        raise ValueError("rows of 1 .. %d values (got %d)" % (KNN_MAX_D, d))
    if rows:
        check(lib().cx_knn_normalize(ptr(x), ptr(y), rows, d, stream_ptr()), "cx_knn_normalize")
    return y


def knn_topk(q, bank, k, out_sim, out_idx, q_group=None, bank_group=None, scratch=None, splits=0):
    """The k nearest bank rows of every query by inner product (cx_knn_topk; the order is defined in include/chexpert_hip.h): q (Q, d),
    bank (M, d) fp32; out_sim (Q, k) fp32 and out_idx (Q, k) int32, descending, ties to the lower index, idx -1 / sim -inf where a query
    has fewer than k candidates.  q_group / bank_group int32, both or neither: a bank row of the query's own group (>= 0) is no
    candidate.  scratch: fp32, at least knn_scratch(Q, M, k, splits) floats (None: allocated here).  Returns the scratch."""
    assert q.dim() == 2 and bank.dim() == 2 and q.shape[1] == bank.shape[1]
    (Q, d), M = q.shape, bank.shape[0]
    if not 1 <= d <= KNN_MAX_D:
        raise ValueError("rows of 1 .. %d values (got %d)" % (KNN_MAX_D, d))
    need = knn_scratch(Q, M, k, splits)
    _f32(q, bank, out_sim)
    assert tuple(out_sim.shape) == (Q, k) and tuple(out_idx.shape) == (Q, k) and out_idx.dtype == torch.int32 and out_idx.is_contiguous()
    if (q_group is None) != (bank_group is None):
        raise ValueError("q_group and bank_group are given together or not at all")
    for g, n in ((q_group, Q), (bank_group, M)):
        assert g is None or (g.dtype == torch.int32 and g.is_contiguous() and tuple(g.shape) == (n,))
    if scratch is None:
        scratch = torch.empty(need, dtype=torch.float32, device=q.device)
    _f32(scratch, n=need)
    assert all(t is None or t.device == q.device for t in (bank, out_sim, out_idx, q_group, bank_group, scratch))
    require_cuda(q, bank, out_sim, out_idx, q_group, bank_group, scratch)
    check(lib().cx_knn_topk(ptr(q), ptr(bank), ptr(q_group), ptr(bank_group), ptr(out_sim), ptr(out_idx), ptr(scratch), scratch.numel(),
                            Q, M, d, int(k), int(splits), stream_ptr()), "cx_knn_topk")
    return scratch


def knn_vote(sim, idx, labels, out_score, out_support, inv_T):
    """The weighted vote of each query's neighbours (cx_knn_vote): labels (M, n) fp32 in [0, 1], < 0 = ignored; weights
    exp((s_j - s_0) * inv_T) relative to the nearest neighbour; out_score (Q, n) = num / den, out_support (Q, n) = den, 0.5 / 0 where no
    neighbour has the label."""
    Q, k = sim.shape
    n = labels.shape[1]
    if not (1 <= k <= KNN_MAX_K and 1 <= n <= KNN_MAX_CLASSES and inv_T >= 0):
        raise ValueError("the vote takes 1 <= k <= %d, 1 <= n <= %d and inv_T >= 0 (got k %d, n %d, inv_T %r)"
                         % (KNN_MAX_K, KNN_MAX_CLASSES, k, n, inv_T))
    _f32(sim, labels, out_score, out_support)
    assert idx.dtype == torch.int32 and idx.is_contiguous() and tuple(idx.shape) == (Q, k) and labels.dim() == 2
    assert tuple(out_score.shape) == (Q, n) and tuple(out_support.shape) == (Q, n)
    require_cuda(sim, idx, labels, out_score, out_support)
    if Q:
        check(lib().cx_knn_vote(ptr(sim), ptr(idx), ptr(labels), ptr(out_score), ptr(out_support), float(inv_T), Q, k, n, stream_ptr()),
              "cx_knn_vote")


def probe_scratch(M, d, n, splits=0):
    """The floats of scratch probe_loss_grad and probe_colstats need for a bank of M rows (cx_probe_scratch), `splits` = 0 being the
    library's own choice of slices.  Sizes the kernels refuse are a ValueError."""
    M, d, n, splits = int(M), int(d), int(n), int(splits)
    if not (1 <= M < 2 ** 31 and 1 <= d <= KNN_MAX_D and 1 <= n <= KNN_MAX_CLASSES and 0 <= splits <= PROBE_MAX_SPLITS):
        raise ValueError("the probe takes 1 <= M < 2^31 rows of 1 .. %d features, 1 .. %d classes and 0 <= splits <= %d (got M %d, d %d, "
                         "n %d, splits %d)" % (KNN_MAX_D, KNN_MAX_CLASSES, PROBE_MAX_SPLITS, M, d, n, splits))
    return int(lib().cx_probe_scratch(M, d, n, splits))


def _probe_scratch(scratch, need, like):
    if scratch is None:
        scratch = torch.empty(need + (need & 1), dtype=torch.float32, device=like.device)
    _f32(scratch, n=need)
    assert scratch.device == like.device and scratch.data_ptr() % 8 == 0
    return scratch


def probe_colstats(x, mean, rstd, scratch=None):
    """mean (d,) and rstd (d,) = 1 / max(population std, 1e-6) of the columns of x (M, d) fp32 (cx_probe_colstats): double sums in a
    fixed order, rounded once.  scratch: fp32, at least probe_scratch(M, d, 1) floats (None: allocated here).  Returns the scratch."""
    assert x.dim() == 2
    M, d = x.shape
    need = probe_scratch(M, d, 1)
    _f32(x)
    _f32(mean, rstd, n=d)
    assert mean.numel() == d and rstd.numel() == d and mean.device == x.device and rstd.device == x.device
    scratch = _probe_scratch(scratch, need, x)
    require_cuda(x, mean, rstd, scratch)
    check(lib().cx_probe_colstats(ptr(x), ptr(mean), ptr(rstd), ptr(scratch), scratch.numel(), M, d, stream_ptr()), "cx_probe_colstats")
    return scratch


def probe_standardize(x, mean, rstd, y):
    """y = (x - mean) * rstd per column of the (rows, d) fp32 matrix, two roundings (cx_probe_standardize); y may be x."""
    assert x.dim() == 2 and y.shape == x.shape
    rows, d = x.shape
    if not 1 <= d <= KNN_MAX_D:
        raise ValueError("rows of 1 .. %d values (got %d)" % (KNN_MAX_D, d))
    _f32(x, y)
    _f32(mean, rstd, n=d)
    assert mean.numel() == d and rstd.numel() == d and all(t.device == x.device for t in (mean, rstd, y))
    require_cuda(x, mean, rstd, y)
    if rows:
        check(lib().cx_probe_standardize(ptr(x), ptr(mean), ptr(rstd), ptr(y), rows, d, stream_ptr()), "cx_probe_standardize")
    return y


def _probe_theta(theta, n, d, *same):
    _f32(theta, *same)
    assert tuple(theta.shape) == (n, d + 1), "theta is (n, d + 1): the weights, then the bias"
    assert all(t is None or (tuple(t.shape) == (n, d + 1) and t.device == theta.device) for t in same)


def probe_logits(x, theta, out):
    """out (rows, n) = x w^T + b for theta (n, d + 1) = [w | b] (cx_probe_logits), fp32 on the fp32-input MFMA."""
    assert x.dim() == 2 and theta.dim() == 2
    rows, d = x.shape
    n = theta.shape[0]
    if rows:
        probe_scratch(rows, d, n)                                            # (checks d and n)
    _f32(x, out)
    _probe_theta(theta, n, d)
    assert tuple(out.shape) == (rows, n) and out.device == x.device and theta.device == x.device
    require_cuda(x, theta, out)
    if rows:
        check(lib().cx_probe_logits(ptr(x), ptr(theta), ptr(out), rows, d, n, stream_ptr()), "cx_probe_logits")
    return out


def _probe_flags(t, n, like):
    assert t is None or (t.dtype == torch.int32 and t.is_contiguous() and t.numel() == n and t.device == like.device)


def probe_loss_grad(x, y, theta, loss, grad, count, pos_weight=None, l2=0.0, active=None, scratch=None, splits=0):
    """Loss (n,), gradient (n, d + 1) and count (n, 3) = live rows, sum y, sum (1 - y) of the multi-label logistic regression of
    include/chexpert_hip.h (cx_probe_loss_grad): x (M, d), y (M, n) with < 0 = ignored, theta (n, d + 1), pos_weight (n,) or None, l2 >= 0.
    active (n,) int32 or None: a class whose flag is 0 keeps its previous outputs.  scratch: fp32, at least probe_scratch(M, d, n, splits)
    floats (None: allocated here).  Returns the scratch."""
    assert x.dim() == 2 and y.dim() == 2 and y.shape[0] == x.shape[0]
    (M, d), n = x.shape, y.shape[1]
    need = probe_scratch(M, d, n, splits)
    l2 = float(l2)
    if not (0.0 <= l2 < float("inf")):
        raise ValueError("l2 must be finite and >= 0 (got %r)" % (l2,))
    _f32(x, y)
    _probe_theta(theta, n, d, grad)
    _f32(loss, pos_weight, n=n)
    _f32(count, n=3 * n)
    assert loss.numel() == n and count.numel() == 3 * n and (pos_weight is None or pos_weight.numel() == n)
    _probe_flags(active, n, x)
    scratch = _probe_scratch(scratch, need, x)
    assert all(t is None or t.device == x.device for t in (y, theta, loss, grad, count, pos_weight))
    require_cuda(x, y, theta, loss, grad, count, pos_weight, active, scratch)
    check(lib().cx_probe_loss_grad(ptr(x), ptr(y), ptr(theta), ptr(pos_weight), l2, ptr(active), ptr(loss), ptr(grad), ptr(count),
                                   ptr(scratch), scratch.numel(), M, d, n, int(splits), stream_ptr()), "cx_probe_loss_grad")
    return scratch


def _probe_history(s_hist, y_hist, hist, n, d, like):
    _f32(s_hist, y_hist)
    assert s_hist.dim() == 3 and s_hist.shape == y_hist.shape and s_hist.shape[0] == n and s_hist.shape[2] == d + 1
    m = s_hist.shape[1]
    if not 1 <= m <= PROBE_MAX_HISTORY:
        raise ValueError("a history of 1 .. %d pairs (got %d)" % (PROBE_MAX_HISTORY, m))
    assert hist.dtype == torch.int32 and hist.is_contiguous() and tuple(hist.shape) == (n, 2)
    assert all(t.device == like.device for t in (s_hist, y_hist, hist))
    return m


def probe_lbfgs_direction(grad, s_hist, y_hist, hist, direction, stats, active=None):
    """direction (n, d + 1) = -H grad per class by the L-BFGS two-loop recursion over the pairs in s_hist / y_hist (n, m, d + 1), hist
    (n, 2) int32 = pairs held, next slot (cx_probe_lbfgs_direction); -grad where that does not descend.  stats (n, 4): g . dir, max |g|,
    sum |g|, 1 where the fallback was taken.  active (n,) int32 or None: a class whose flag is 0 keeps its previous outputs."""
    n, d = grad.shape[0], grad.shape[1] - 1
    _probe_theta(grad, n, d, direction)
    m = _probe_history(s_hist, y_hist, hist, n, d, grad)
    _f32(stats, n=4 * n)
    assert stats.numel() == 4 * n and stats.device == grad.device
    _probe_flags(active, n, grad)
    require_cuda(grad, s_hist, y_hist, hist, direction, stats, active)
    check(lib().cx_probe_lbfgs_direction(ptr(grad), ptr(s_hist), ptr(y_hist), ptr(hist), ptr(active), ptr(direction), ptr(stats), n, d, m,
                                         stream_ptr()), "cx_probe_lbfgs_direction")


def probe_lbfgs_advance(theta, grad, direction, t, mode, theta_t, grad_t, s_hist, y_hist, hist, tstats):
    """Per class by mode (n,) int32 (cx_probe_lbfgs_advance): 1 forms the trial point theta_t = theta + t dir; 2 accepts it: the pair
    (theta_t - theta, grad_t - grad) joins the history unless s.y <= 0, then theta = theta_t, grad = grad_t; 3 writes the trial's slope
    and size, tstats (n, 2) = grad_t . dir, max |grad_t|; 0 writes nothing."""
    n, d = theta.shape[0], theta.shape[1] - 1
    _probe_theta(theta, n, d, grad, direction, theta_t, grad_t)
    m = _probe_history(s_hist, y_hist, hist, n, d, theta)
    _f32(t, n=n)
    _f32(tstats, n=2 * n)
    assert t.numel() == n and t.device == theta.device and tstats.numel() == 2 * n and tstats.device == theta.device
    _probe_flags(mode, n, theta)
    assert mode is not None
    require_cuda(theta, grad, direction, t, mode, theta_t, grad_t, s_hist, y_hist, hist, tstats)
    check(lib().cx_probe_lbfgs_advance(ptr(theta), ptr(grad), ptr(direction), ptr(t), ptr(mode), ptr(theta_t), ptr(grad_t), ptr(s_hist),
                                       ptr(y_hist), ptr(hist), ptr(tstats), n, d, m, stream_ptr()), "cx_probe_lbfgs_advance")


def barlow_scratch(N, d):
    """The floats of scratch barlow_fwd_bwd needs for (N, d) embeddings (cx_barlow_scratch; the layout stands in
    include/chexpert_hip.h): the two normalised views, the d x d matrix G, the per-column vectors and the tiles' partial sums.  Sizes
    the loss refuses are a ValueError."""
    N, d = int(N), int(d)
    if not (2 <= N <= BARLOW_MAX_N and 1 <= d <= BARLOW_MAX_D):
        raise ValueError("the Barlow Twins loss takes 2 .. %d rows of 1 .. %d values (got %d x %d)" % (BARLOW_MAX_N, BARLOW_MAX_D, N, d))
    return int(lib().cx_barlow_scratch(N, d))


def barlow_fwd_bwd(logits, ids, lambd, loss, dlogits, stats=None, scratch=None, grad_scale=1.0):
    """The Barlow Twins loss of the (N, d) embeddings with its exact gradient (cx_barlow_fwd_bwd, four launches, the products on the
    fp32-input MFMA; the definition stands in include/chexpert_hip.h): rows p and p + N // 2 are the two views of pair p; ids fp32
    (N, 1) is a mask, a pair with an id < 0 in either row is out of the batch; lambd a one-float DEVICE tensor, read by the kernels (a
    captured step sees a changed value).  loss (1,), dlogits (N, d) and stats (4,) = [on, off, mean_k C_kk, m] are optional;
    grad_scale multiplies dlogits alone.  scratch: fp32, at least barlow_scratch(N, d) floats (None: allocated here, which a graph
    capture must not do -- hold one).  Returns the scratch."""
    assert logits.dim() == 2 and logits.dtype == torch.float32 and logits.is_contiguous()
    N, d = logits.shape
    need = barlow_scratch(N, d)
    assert ids.dtype == torch.float32 and ids.is_contiguous() and tuple(ids.shape) == (N, 1)
    assert lambd is not None and lambd.numel() == 1
    assert dlogits is None or tuple(dlogits.shape) == (N, d)
    assert stats is None or tuple(stats.shape) == (4,)
    if scratch is None:
        scratch = torch.empty(need, dtype=torch.float32, device=logits.device)
    assert scratch.dim() == 1 and scratch.numel() >= need
    assert all(t is None or t.device == logits.device for t in (ids, lambd, loss, dlogits, stats, scratch))
    _f32(loss, lambd, n=1)
    _f32(dlogits)
    _f32(stats, n=4)
    _f32(scratch, n=scratch.numel())
    require_cuda(logits, ids, lambd, loss, dlogits, stats, scratch)
    check(lib().cx_barlow_fwd_bwd(ptr(logits), ptr(ids), ptr(lambd), ptr(loss), ptr(dlogits), ptr(stats), grad_scale, ptr(scratch),
                                  scratch.numel(), N, d, stream_ptr()), "cx_barlow_fwd_bwd")
    return scratch


def softmax_ce_fwd_bwd(logits, target, loss, loss_elem, dlogits, grad_scale=1.0):
    """CrossEntropyLoss forward + gradient in one launch (fp32 logits [B, n], int64 class indices [B])."""
    B, n = logits.shape
    check(lib().cx_softmax_ce_fwd_bwd(ptr(logits), ptr(target), ptr(loss), ptr(loss_elem), ptr(dlogits), grad_scale, B, n,
                                      stream_ptr()), "cx_softmax_ce_fwd_bwd")


def head_bwd(dlogits, pooled, w, dw, db, dpooled):
    B, n = dlogits.shape
    check(lib().cx_head_bwd(ptr(dlogits), ptr(pooled), ptr(w), ptr(dw), ptr(db), ptr(dpooled), B, pooled.shape[1], n,
                            stream_ptr()), "cx_head_bwd")


def gap_relu_bn_bwd(dpooled, x, scale, shift, mean, rstd, e_scale, g, S1, S2, stat_rows=0):
    B, H, W, Cc, ldx = _nhwc(x)
    check(_fn("cx_gap_relu_bn_bwd", x)(ptr(dpooled), ptr(x), ptr(scale), ptr(shift), ptr(mean), ptr(rstd), ptr(e_scale), ptr(g),
                                   ptr(S1), ptr(S2), B, H * W, Cc, ldx, _nhwc(g)[4], stat_rows, stream_ptr()), "cx_gap_relu_bn_bwd")
    return lib().cx_last_stat_rows() if stat_rows else None


# ---- pooling heads other than the average (csrc/pool_head.hip; the definitions: include/chexpert_hip.h, pooling.py)
POOL_KINDS = {"avg": 0, "max": 1, "lse": 2, "gem": 3}       # CX_POOL_*
POOL_ACT_RELU, POOL_ACT_SWISH = 1, 2                        # CX_POOL_ACT_*


def _pool_args(x, pooled, param, act, kind):
    require_cuda(x, pooled, param)
    B, H, W, Cc, ldx = _nhwc(x)
    k = POOL_KINDS[kind] if isinstance(kind, str) else int(kind)
    assert k in (1, 2, 3), "pool_head_*: kind max, lse or gem (the average has its own kernels)"
    assert act in (POOL_ACT_RELU, POOL_ACT_SWISH)
    assert tuple(pooled.shape) == (B, Cc) and pooled.dtype == torch.float32 and pooled.is_contiguous()
    assert (param is None) == (k == 1), "pool_head_*: param is r for lse, p for gem, None for max"
    assert param is None or (param.dtype == torch.float32 and param.numel() == 1)
    return B, H * W, Cc, ldx, k


def pool_head_fwd(x, sc, sh, pooled, aux, param, *, act, kind):
    """cx_pool_head_fwd: pooled (B,C) fp32 = pool_p act(x*sc + sh) over the pixels of an NHWC map, pool = max / lse / gem; aux (B,C)
    receives GeM's T / LSE's offset pooled - max; param: the one-element fp32 tensor r (lse) or p (gem), None for max."""
    B, HW, Cc, ldx, k = _pool_args(x, pooled, param, act, kind)
    assert k == 1 or (aux is not None and aux.shape == pooled.shape and aux.dtype == torch.float32 and aux.is_contiguous())
    check(_fn("cx_pool_head_fwd", x)(ptr(x), ptr(sc), ptr(sh), ptr(pooled), ptr(aux), ptr(param), B, HW, Cc, ldx, act, k, stream_ptr()),
          "cx_pool_head_fwd")


def pool_head_bwd(dpooled, pooled, aux, param, x, sc, sh, mean, rstd, e_scale, g, S1, S2, *, act, kind, stat_rows=0):
    """cx_pool_head_bwd: the backward of pool_head_fwd with the contract of gap_relu_bn_bwd (g = e_scale * dz, S1 / S2; stat_rows > 0:
    one statistic row per image).  Returns the row count in rows mode."""
    B, HW, Cc, ldx, k = _pool_args(x, pooled, param, act, kind)
    assert tuple(dpooled.shape) == (B, Cc) and dpooled.dtype == torch.float32 and dpooled.is_contiguous()
    assert g.dtype == x.dtype and g.shape == x.shape
    check(_fn("cx_pool_head_bwd", x)(ptr(dpooled), ptr(pooled), ptr(aux), ptr(param), ptr(x), ptr(sc), ptr(sh), ptr(mean), ptr(rstd),
                                     ptr(e_scale), ptr(g), ptr(S1), ptr(S2), B, HW, Cc, ldx, _nhwc(g)[4], act, k, stat_rows, stream_ptr()),
          "cx_pool_head_bwd")
    return lib().cx_last_stat_rows() if stat_rows else None


def pool_p_grad(dpooled, pooled, aux, p, dp):
    """cx_pool_p_grad: dp[0] += sum dpooled * pooled * (T - ln pooled) / q (GeM's exponent; 0 where p is clamped), in a fixed order."""
    require_cuda(dpooled, pooled, aux, p, dp)
    B, Cc = pooled.shape
    for t in (dpooled, pooled, aux):
        assert tuple(t.shape) == (B, Cc) and t.dtype == torch.float32 and t.is_contiguous()
    assert p.dtype == dp.dtype == torch.float32 and p.numel() == dp.numel() == 1
    check(lib().cx_pool_p_grad(ptr(dpooled), ptr(pooled), ptr(aux), ptr(p), ptr(dp), B, Cc, stream_ptr()), "cx_pool_p_grad")


# ---- class-specific residual attention head (csrc/csra_head.hip; the definition: include/chexpert_hip.h, heads.py)
CSRA_MAX_CLASSES = 64                                       # CX_CSRA_MAX_CLASSES
CSRA_STAT = 4                                               # floats per (image, class) the forward leaves for the way back


def _map_args(kind, x, m, w, attn, act):
    """The shared argument check of the two heads that pool a per-pixel score map.  Returns (B, HW, C, ldx, n, the [lambda, T] argument of
    the cx_csra_* entry points: cx_pcam_* take none)."""
    assert kind in ("csra", "pcam")
    require_cuda(x, m, w, attn)
    B, H, W, Cc, ldx = _nhwc(x)
    n = w.shape[0]
    assert act in (POOL_ACT_RELU, POOL_ACT_SWISH)
    assert tuple(w.shape) == (n, Cc) and w.dtype == torch.float32 and w.is_contiguous()
    if kind == "csra":
        assert attn.dtype == torch.float32 and attn.numel() == 2 and attn.is_contiguous(), "csra_head_*: attn is the fp32 device tensor [lambda, T]"
    assert m is None or (tuple(m.shape) == (B, Cc) and m.dtype == torch.float32 and m.is_contiguous())
    return B, H * W, Cc, ldx, n, ((ptr(attn),) if kind == "csra" else ())


def map_bwd_scratch(kind, B, HW, Cc, n):
    """cx_<kind>_bwd_scratch: the floats of scratch map_head_bwd needs at this shape (pcam: csra's + B n)."""
    name = "cx_%s_bwd_scratch" % kind
    r = getattr(lib(), name)(B, HW, Cc, n)
    if r < 0:
        check(int(r), name)
    return int(r)


def map_head_fwd(kind, x, sc, sh, m, w, bias, attn, logits, s, stat, *, act):
    """cx_<kind>_head_fwd, kind "csra" or "pcam": s (B,n,HW) fp32 = the classifier w (n,C) at every pixel of act(x*sc + sh) * m (m (B,C)
    fp32 or None); logits (B,n) pooled from it per class; stat (B,n,4) is what the backward reads.
    csra: logits = bias + mean_p s + lambda * softmax_p(T s) . s with attn = [lambda, T] in device memory.
    pcam: logits = sum_p w_p (s_p + bias) with w_p = sigmoid(s_p + bias) / sum_q sigmoid(s_q + bias); attn is not read."""
    B, HW, Cc, ldx, n, lam = _map_args(kind, x, m, w, attn, act)
    for t, shape in ((logits, (B, n)), (s, (B, n, HW)), (stat, (B, n, CSRA_STAT))):
        assert tuple(t.shape) == shape and t.dtype == torch.float32 and t.is_contiguous()
    name = "cx_%s_head_fwd" % kind
    check(_fn(name, x)(ptr(x), ptr(sc), ptr(sh), ptr(m), ptr(w), ptr(bias), *lam, ptr(logits), ptr(s), ptr(stat), B, HW, Cc, ldx, n, act,
                       stream_ptr()), name)


def map_head_bwd(kind, dlogits, s, stat, attn, x, sc, sh, m, mean, rstd, e_scale, w, g, S1, S2, dw, db, scratch, *, act, stat_rows=0):
    """cx_<kind>_head_bwd: the backward of map_head_fwd with the contract of gap_relu_bn_bwd (g = e_scale * dz, S1 / S2; stat_rows > 0:
    one statistic row per image); dw (n,C) and db (n,; or None) are added to, in a fixed order through `scratch` (fp32, at least
    map_bwd_scratch floats).  Returns the row count in rows mode."""
    B, HW, Cc, ldx, n, lam = _map_args(kind, x, m, w, attn, act)
    require_cuda(dlogits, s, stat, g, dw, db, scratch)
    assert tuple(dlogits.shape) == (B, n) and dlogits.dtype == torch.float32 and dlogits.is_contiguous()
    assert g.dtype == x.dtype and g.shape == x.shape
    assert dw.numel() == n * Cc and dw.dtype == torch.float32 and dw.is_contiguous() and (db is None or db.numel() == n)
    assert scratch.dtype == torch.float32 and scratch.is_contiguous()
    name = "cx_%s_head_bwd" % kind
    check(_fn(name, x)(ptr(dlogits), ptr(s), ptr(stat), *lam, ptr(x), ptr(sc), ptr(sh), ptr(m), ptr(mean), ptr(rstd), ptr(e_scale), ptr(w),
                       ptr(g), ptr(S1), ptr(S2), ptr(dw), ptr(db), ptr(scratch), scratch.numel(), B, HW, Cc, ldx, _nhwc(g)[4], n, act,
                       stat_rows, stream_ptr()), name)
    return lib().cx_last_stat_rows() if stat_rows else None


def csra_bwd_scratch(B, HW, Cc, n):
    """cx_csra_bwd_scratch: the floats of scratch csra_head_bwd needs at this shape."""
    return map_bwd_scratch("csra", B, HW, Cc, n)


def csra_head_fwd(x, sc, sh, m, w, bias, attn, logits, s, stat, *, act):
    """map_head_fwd of the csra head."""
    return map_head_fwd("csra", x, sc, sh, m, w, bias, attn, logits, s, stat, act=act)


def csra_head_bwd(dlogits, s, stat, attn, x, sc, sh, m, mean, rstd, e_scale, w, g, S1, S2, dw, db, scratch, *, act, stat_rows=0):
    """map_head_bwd of the csra head."""
    return map_head_bwd("csra", dlogits, s, stat, attn, x, sc, sh, m, mean, rstd, e_scale, w, g, S1, S2, dw, db, scratch, act=act,
                        stat_rows=stat_rows)


# ---- probabilistic-CAM pooling head (csrc/csra_head.hip): the csra operands without [lambda, T]
def pcam_bwd_scratch(B, HW, Cc, n):
    """cx_pcam_bwd_scratch: the floats of scratch pcam_head_bwd needs at this shape (csra_bwd_scratch + B n)."""
    return map_bwd_scratch("pcam", B, HW, Cc, n)


def pcam_head_fwd(x, sc, sh, m, w, bias, logits, s, stat, *, act):
    """map_head_fwd of the pcam head: csra_head_fwd's arguments without attn."""
    return map_head_fwd("pcam", x, sc, sh, m, w, bias, None, logits, s, stat, act=act)


def pcam_head_bwd(dlogits, s, stat, x, sc, sh, m, mean, rstd, e_scale, w, g, S1, S2, dw, db, scratch, *, act, stat_rows=0):
    """map_head_bwd of the pcam head: csra_head_bwd's arguments without attn."""
    return map_head_bwd("pcam", dlogits, s, stat, None, x, sc, sh, m, mean, rstd, e_scale, w, g, S1, S2, dw, db, scratch, act=act,
                        stat_rows=stat_rows)


def unpool2_mask(d, x, sc, sh, mean, rstd, e_scale, g, S1, S2, stat_rows=0):
    B, H, W, Cc, ldx = _nhwc(x)
    check(_fn("cx_unpool2_mask", x)(ptr(d), ptr(x), ptr(sc), ptr(sh), ptr(mean), ptr(rstd), ptr(e_scale), ptr(g), ptr(S1), ptr(S2),
                                B, H, W, Cc, _nhwc(d)[4], ldx, _nhwc(g)[4], stat_rows, stream_ptr()), "cx_unpool2_mask")
    return lib().cx_last_stat_rows() if stat_rows else None


def affine2_inplace(dz, x, pa, pb, pc):
    B, H, W, Cc, ld = _nhwc(dz)
    assert ld == Cc and _nhwc(x)[4] == Cc
    check(lib().cx_affine2_inplace(ptr(dz), ptr(x), ptr(pa), ptr(pb), ptr(pc), B * H * W, Cc, stream_ptr()),
          "cx_affine2_inplace")


def affine2_relu(a, b, pa, pb, pc, out, mask=None):
    """mask (optional, uint8 [rows * C / 8]): the sign bits of `out` for relu_bwd_stats (cx_affine2_relu_mask)."""
    B, H, W, Cc, ld = _nhwc(a)
    assert ld == Cc and _nhwc(b)[4] == Cc and _nhwc(out)[4] == Cc
    assert mask is None or (mask.dtype == torch.uint8 and mask.numel() == B * H * W * Cc // 8)
    check(_fn("cx_affine2_relu_mask", a)(ptr(a), ptr(b), ptr(pa), ptr(pb), ptr(pc), ptr(out), ptr(mask), B * H * W, Cc, stream_ptr()),
          "cx_affine2_relu_mask")


def join_fwd(a, b, b_lo, pa, pb, pc, out, out_lo, mask=None):
    """cx_join_fwd: out = relu(a*pa + (b [+ b_lo])*pb + pc) as hi (bf16 `out`) + lo (int8 `out_lo`) planes + sign bits `mask`."""
    require_cuda(a, b, out)
    B, H, W, Cc, ld = _nhwc(a)
    assert a.dtype == torch.bfloat16 and ld == Cc and _nhwc(b)[4] == Cc and _nhwc(out)[4] == Cc
    n = B * H * W * Cc
    for t_ in (b_lo, out_lo):
        assert t_ is None or (t_.dtype in (torch.int8, torch.uint8) and t_.is_contiguous() and t_.numel() == n)
    assert mask is None or (mask.dtype == torch.uint8 and mask.numel() == n // 8)
    check(lib().cx_join_fwd(ptr(a), ptr(b), ptr(b_lo), ptr(pa), ptr(pb), ptr(pc), ptr(out), ptr(out_lo), ptr(mask), B * H * W, Cc,
                            stream_ptr()), "cx_join_fwd")


def relu_bwd_stats(dout, out, a, mu_a, r_a, b, mu_b, r_b, dz, S1, S2a, S2b, stat_rows=0, mask=None):
    """mask (optional): sign bits written by affine2_relu, read instead of `out`."""
    B, H, W, Cc, ld = _nhwc(dout)
    assert ld == Cc
    check(_fn("cx_relu_bwd_stats_mask", dout)(ptr(dout), ptr(out), ptr(mask), ptr(a), ptr(mu_a), ptr(r_a), ptr(b), ptr(mu_b), ptr(r_b),
                                              ptr(dz), ptr(S1), ptr(S2a), ptr(S2b), B * H * W, Cc, stat_rows, stream_ptr()),
          "cx_relu_bwd_stats_mask")
    return lib().cx_last_stat_rows() if stat_rows else None


def adam_step(p, g, m, v, lr, beta1, beta2, eps, weight_decay, step, grad_scale=1.0):
    check(lib().cx_adam_step(ptr(p), ptr(g), ptr(m), ptr(v), p.numel(), lr, beta1, beta2, eps, weight_decay, step, grad_scale,
                             stream_ptr()), "cx_adam_step")


def sgd_nesterov_step(p, g, buf, lr, momentum, weight_decay, first_step, grad_scale=1.0):
    check(lib().cx_sgd_nesterov_step(ptr(p), ptr(g), ptr(buf), p.numel(), lr, momentum, weight_decay, int(first_step),
                                     grad_scale, stream_ptr()), "cx_sgd_nesterov_step")


def rmsprop_step(p, g, sq, buf, lr, alpha, eps, momentum, weight_decay, grad_scale=1.0):
    check(lib().cx_rmsprop_step(ptr(p), ptr(g), ptr(sq), ptr(buf), p.numel(), lr, alpha, eps, momentum, weight_decay,
                                grad_scale, stream_ptr()), "cx_rmsprop_step")


def adam_step_dev(p, g, m, v, hyper, beta1, beta2, eps, weight_decay, grad_scale=1.0):
    check(lib().cx_adam_step_dev(ptr(p), ptr(g), ptr(m), ptr(v), p.numel(), ptr(hyper), beta1, beta2, eps, weight_decay, grad_scale,
                                 stream_ptr()), "cx_adam_step_dev")


def sgd_nesterov_step_dev(p, g, buf, hyper, momentum, weight_decay, grad_scale=1.0):
    check(lib().cx_sgd_nesterov_step_dev(ptr(p), ptr(g), ptr(buf), p.numel(), ptr(hyper), momentum, weight_decay, grad_scale,
                                         stream_ptr()), "cx_sgd_nesterov_step_dev")


def rmsprop_step_dev(p, g, sq, buf, hyper, alpha, eps, momentum, weight_decay, grad_scale=1.0):
    check(lib().cx_rmsprop_step_dev(ptr(p), ptr(g), ptr(sq), ptr(buf), p.numel(), ptr(hyper), alpha, eps, momentum, weight_decay,
                                    grad_scale, stream_ptr()), "cx_rmsprop_step_dev")


def optim_tick(hyper):
    check(lib().cx_optim_tick(ptr(hyper), stream_ptr()), "cx_optim_tick")


# ---- global-norm clipping, non-finite skip and weight EMA inside the optimiser launch (csrc/optim.hip)
def grad_norm_partials(n):
    """Floats of workspace `grad_norm` needs for n gradients (the grid of its first launch: a function of n alone)."""
    return lib().cx_grad_norm_partials(n)


def grad_norm(g, workspace, clip, grad_scale=1.0, max_norm=0.0, skip_nonfinite=False):
    """clip = float[4] {norm of grad_scale * g, clip coefficient, nonfinite, skipped steps} on the device; two launches, no atomics,
    the same bits on every call.  max_norm <= 0: coefficient 1.  `clip[3]` is a running count: zero `clip` once."""
    require_cuda(g, workspace, clip)
    _f32(g, workspace)
    _f32(clip, n=4)
    check(lib().cx_grad_norm(ptr(g), g.numel(), grad_scale, max_norm, int(bool(skip_nonfinite)), ptr(workspace), workspace.numel(),
                             ptr(clip), stream_ptr()), "cx_grad_norm")


def _optim_tail(clip, ema, ema_decay, ema_warmup, skip_nonfinite, *bufs, n=0):
    """Checks `bufs` (n floats each) and clip; the trailing arguments every `_ex` and `_items` entry point takes."""
    require_cuda(clip, ema, *bufs)
    _f32(ema, *bufs, n=n)
    _f32(clip, n=4)
    return ptr(clip), ptr(ema), (0.0 if ema is None else float(ema_decay)), int(bool(ema_warmup)), int(bool(skip_nonfinite)), stream_ptr()


def adam_step_ex(p, g, m, v, lr, beta1, beta2, eps, weight_decay, step, grad_scale=1.0, clip=None, ema=None, ema_decay=0.0,
                 ema_warmup=True, skip_nonfinite=False):
    tail = _optim_tail(clip, ema, ema_decay, ema_warmup, skip_nonfinite, p, g, m, v, n=p.numel())
    check(lib().cx_adam_step_ex(ptr(p), ptr(g), ptr(m), ptr(v), p.numel(), lr, beta1, beta2, eps, weight_decay, step, grad_scale,
                                *tail), "cx_adam_step_ex")


def sgd_nesterov_step_ex(p, g, buf, lr, momentum, weight_decay, first_step, step, grad_scale=1.0, clip=None, ema=None, ema_decay=0.0,
                         ema_warmup=True, skip_nonfinite=False):
    tail = _optim_tail(clip, ema, ema_decay, ema_warmup, skip_nonfinite, p, g, buf, n=p.numel())
    check(lib().cx_sgd_nesterov_step_ex(ptr(p), ptr(g), ptr(buf), p.numel(), lr, momentum, weight_decay, int(first_step), step,
                                        grad_scale, *tail), "cx_sgd_nesterov_step_ex")


def rmsprop_step_ex(p, g, sq, buf, lr, alpha, eps, momentum, weight_decay, step, grad_scale=1.0, clip=None, ema=None, ema_decay=0.0,
                    ema_warmup=True, skip_nonfinite=False):
    tail = _optim_tail(clip, ema, ema_decay, ema_warmup, skip_nonfinite, p, g, sq, buf, n=p.numel())
    check(lib().cx_rmsprop_step_ex(ptr(p), ptr(g), ptr(sq), ptr(buf), p.numel(), lr, alpha, eps, momentum, weight_decay, step,
                                   grad_scale, *tail), "cx_rmsprop_step_ex")


def adam_step_dev_ex(p, g, m, v, hyper, beta1, beta2, eps, weight_decay, grad_scale=1.0, clip=None, ema=None, ema_decay=0.0,
                     ema_warmup=True, skip_nonfinite=False):
    tail = _optim_tail(clip, ema, ema_decay, ema_warmup, skip_nonfinite, p, g, m, v, n=p.numel())
    check(lib().cx_adam_step_dev_ex(ptr(p), ptr(g), ptr(m), ptr(v), p.numel(), ptr(hyper), beta1, beta2, eps, weight_decay,
                                    grad_scale, *tail), "cx_adam_step_dev_ex")


def sgd_nesterov_step_dev_ex(p, g, buf, hyper, momentum, weight_decay, grad_scale=1.0, clip=None, ema=None, ema_decay=0.0,
                             ema_warmup=True, skip_nonfinite=False):
    tail = _optim_tail(clip, ema, ema_decay, ema_warmup, skip_nonfinite, p, g, buf, n=p.numel())
    check(lib().cx_sgd_nesterov_step_dev_ex(ptr(p), ptr(g), ptr(buf), p.numel(), ptr(hyper), momentum, weight_decay, grad_scale,
                                            *tail), "cx_sgd_nesterov_step_dev_ex")


def rmsprop_step_dev_ex(p, g, sq, buf, hyper, alpha, eps, momentum, weight_decay, grad_scale=1.0, clip=None, ema=None, ema_decay=0.0,
                        ema_warmup=True, skip_nonfinite=False):
    tail = _optim_tail(clip, ema, ema_decay, ema_warmup, skip_nonfinite, p, g, sq, buf, n=p.numel())
    check(lib().cx_rmsprop_step_dev_ex(ptr(p), ptr(g), ptr(sq), ptr(buf), p.numel(), ptr(hyper), alpha, eps, momentum, weight_decay,
                                       grad_scale, *tail), "cx_rmsprop_step_dev_ex")


# ---- parameter groups: per-tensor item table and per-group rows walked by the optimiser kernels (csrc/optim.hip)
def optim_item_vec4():
    """Longest work item of the grouped optimiser kernels, in 16-byte units (a constant of the library)."""
    return lib().cx_optim_item_vec4()


def _group_tables(p, items, groups, *bufs):
    """Checks of one grouped launch; returns (n, items pointer, item count, groups pointer, group count)."""
    n = p.numel()
    require_cuda(p, items, groups, *bufs)
    _f32(p, *bufs, n=n)
    _f32(groups)
    assert items.dtype == torch.int32 and items.is_contiguous() and items.dim() == 2 and items.shape[1] == 4, \
        "items: an int32 tensor (n_items, 4) {start4, len4, group, tensor}"
    assert groups.dim() == 2 and groups.shape[1] == 4, "groups: a float tensor (G, 4) {lr_mult, weight_decay, frozen, t0}"
    return n, ptr(items), items.shape[0], ptr(groups), groups.shape[0]


def grad_norm_items(g, items, groups, partials, group_sq, group_norm, clip, grad_scale=1.0, max_norm=0.0, skip_nonfinite=False):
    """The segmented `grad_norm`: clip = {norm over the groups with frozen == 0, coefficient, nonfinite, skipped}, group_norm[k] the
    norm of every group (frozen ones too).  Two launches, no atomics, the same bits on every call.  partials: n_items floats."""
    n, pi, ni, pg, ng = _group_tables(g, items, groups)
    require_cuda(partials, group_sq, group_norm, clip)
    _f32(partials, n=ni)
    _f32(group_sq, group_norm, n=ng)
    _f32(clip, n=4)
    check(lib().cx_grad_norm_items(ptr(g), n, pi, ni, pg, ng, grad_scale, max_norm, int(bool(skip_nonfinite)), ptr(partials),
                                   ptr(group_sq), ptr(group_norm), ptr(clip), stream_ptr()), "cx_grad_norm_items")


def adam_step_items(p, g, m, v, items, groups, decoupled, beta1, beta2, eps, hyper=None, lr=0.0, step=0, grad_scale=1.0, clip=None,
                    ema=None, ema_decay=0.0, ema_warmup=True, skip_nonfinite=False):
    """Adam over the item table.  hyper (device float[8]) given: lr and the step come from it; else `lr` and the 1-based `step`."""
    n, pi, ni, pg, ng = _group_tables(p, items, groups, g, m, v, ema)
    check(lib().cx_adam_step_items(ptr(p), ptr(g), ptr(m), ptr(v), n, pi, ni, pg, ng, int(bool(decoupled)), ptr(hyper), lr, int(step),
                                   beta1, beta2, eps, grad_scale, *_optim_tail(clip, ema, ema_decay, ema_warmup, skip_nonfinite)),
          "cx_adam_step_items")


def sgd_nesterov_step_items(p, g, buf, items, groups, decoupled, momentum, hyper=None, lr=0.0, step=0, grad_scale=1.0, clip=None,
                            ema=None, ema_decay=0.0, ema_warmup=True, skip_nonfinite=False):
    """SGD with Nesterov momentum over the item table (`buf` starts as zeros: there is no first-step switch)."""
    n, pi, ni, pg, ng = _group_tables(p, items, groups, g, buf, ema)
    check(lib().cx_sgd_nesterov_step_items(ptr(p), ptr(g), ptr(buf), n, pi, ni, pg, ng, int(bool(decoupled)), ptr(hyper), lr, int(step),
                                           momentum, grad_scale, *_optim_tail(clip, ema, ema_decay, ema_warmup, skip_nonfinite)),
          "cx_sgd_nesterov_step_items")


def rmsprop_step_items(p, g, sq, buf, items, groups, decoupled, alpha, eps, momentum, hyper=None, lr=0.0, step=0, grad_scale=1.0,
                       clip=None, ema=None, ema_decay=0.0, ema_warmup=True, skip_nonfinite=False):
    """RMSprop with momentum over the item table."""
    n, pi, ni, pg, ng = _group_tables(p, items, groups, g, sq, buf, ema)
    check(lib().cx_rmsprop_step_items(ptr(p), ptr(g), ptr(sq), ptr(buf), n, pi, ni, pg, ng, int(bool(decoupled)), ptr(hyper), lr,
                                      int(step), alpha, eps, momentum, grad_scale,
                                      *_optim_tail(clip, ema, ema_decay, ema_warmup, skip_nonfinite)), "cx_rmsprop_step_items")


def _trust_tables(ni, tensor_items, partials, trust):
    """Checks of the trust-ratio tables of one launch; returns (tensor_items pointer, n_tensors, part_w pointer, part_u pointer,
    trust pointer).  tensor_items: int32 (T + 1,), the first item of every tensor in increasing order, then n_items."""
    part_w, part_u = partials
    require_cuda(tensor_items, part_w, part_u, trust)
    if tensor_items.dtype != torch.int32 or tensor_items.dim() != 1 or not tensor_items.is_contiguous() or tensor_items.numel() < 2:
        raise ValueError("tensor_items: a contiguous int32 tensor (n_tensors + 1,) with n_tensors >= 1")
    T = tensor_items.numel() - 1
    _f32(part_w, part_u, n=ni)
    _f32(trust, n=4 * T)
    return ptr(tensor_items), T, ptr(part_w), ptr(part_u), ptr(trust)


def lamb_step_items(p, g, m, v, items, groups, decoupled, beta1, beta2, eps, tensor_items, partials, trust, u, trust_clip=False,
                    always_adapt=False, hyper=None, lr=0.0, step=0, grad_scale=1.0, clip=None, ema=None, ema_decay=0.0, ema_warmup=True,
                    skip_nonfinite=False):
    """LAMB over the item table: Adam's moments, the update u stored in `u` (n floats of scratch), trust[k] = {r, |p|, |u|, adapted}
    per tensor (partials: two buffers of n_items floats), then p -= lr_g * r * u.  Three launches."""
    if decoupled:
        raise ValueError("LAMB's weight decay already sits outside the moments: decoupled=True has no meaning")
    if not eps > 0:
        raise ValueError("eps must be > 0 (got %r): it keeps the update of the zero padding at 0" % (eps,))
    n, pi, ni, pg, ng = _group_tables(p, items, groups, g, m, v, u, ema)
    check(lib().cx_lamb_step_items(ptr(p), ptr(g), ptr(m), ptr(v), n, pi, ni, pg, ng, 0, ptr(hyper), lr, int(step), beta1, beta2, eps,
                                   grad_scale, *_optim_tail(clip, ema, ema_decay, ema_warmup, skip_nonfinite)[:-1],
                                   *_trust_tables(ni, tensor_items, partials, trust), ptr(u), int(bool(trust_clip)),
                                   int(bool(always_adapt)), stream_ptr()), "cx_lamb_step_items")


def lars_step_items(p, g, buf, items, groups, decoupled, momentum, tensor_items, partials, trust, coef, eps, trust_clip=False,
                    always_adapt=False, hyper=None, lr=0.0, step=0, grad_scale=1.0, clip=None, ema=None, ema_decay=0.0, ema_warmup=True,
                    skip_nonfinite=False):
    """LARS over the item table (`buf` starts as zeros): trust[k] = {r, |p|, |g|, adapted} per tensor with
    r = coef |p| / (|g| + wd |p| + eps), then SGD with Nesterov momentum on r * (g + wd * p).  Three launches."""
    if decoupled:
        raise ValueError("LARS's weight decay is part of the trust ratio: decoupled=True has no meaning")
    if not coef > 0:
        raise ValueError("the trust coefficient must be > 0 (got %r)" % (coef,))
    if not eps >= 0:
        raise ValueError("eps must be >= 0 (got %r)" % (eps,))
    n, pi, ni, pg, ng = _group_tables(p, items, groups, g, buf, ema)
    check(lib().cx_lars_step_items(ptr(p), ptr(g), ptr(buf), n, pi, ni, pg, ng, 0, ptr(hyper), lr, int(step), momentum, grad_scale,
                                   *_optim_tail(clip, ema, ema_decay, ema_warmup, skip_nonfinite)[:-1],
                                   *_trust_tables(ni, tensor_items, partials, trust), coef, eps, int(bool(trust_clip)),
                                   int(bool(always_adapt)), stream_ptr()), "cx_lars_step_items")


# ---- sharpness-aware minimisation over the same tables (csrc/optim.hip: cx_sam_*_items)
def _items_host(items, items_host):
    """Pointer of the host copy of the item table (None: none), which the library checks against the buffer before it launches."""
    if items_host is None:
        return None
    if items_host.is_cuda or items_host.dtype != torch.int32 or not items_host.is_contiguous() or items_host.shape != items.shape:
        raise ValueError("items_host: a contiguous int32 CPU tensor shaped like items")
    return ptr(items_host)


def sam_norm_items(p, g, items, groups, rho_eps, partials, sam, grad_scale=1.0, adaptive=False, items_host=None):
    """sam = {norm, rho / (norm + eps), nonfinite, 0} with norm = |grad_scale * g * s| over the unfrozen groups, s = 1 or, adaptive,
    |p| elementwise; rho_eps: device float[2] {rho, eps}.  Two launches, no atomics, the same bits on every call.  partials:
    n_items floats."""
    n, pi, ni, pg, ng = _group_tables(g, items, groups, p)
    require_cuda(rho_eps, partials, sam)
    _f32(rho_eps, n=2)
    _f32(partials, n=ni)
    _f32(sam, n=4)
    check(lib().cx_sam_norm_items(ptr(p), ptr(g), n, pi, _items_host(items, items_host), ni, pg, ng, ptr(rho_eps), grad_scale,
                                  int(bool(adaptive)), ptr(partials), ptr(sam), stream_ptr()), "cx_sam_norm_items")


def sam_perturb_items(p, g, backup, items, groups, sam, grad_scale=1.0, adaptive=False, items_host=None):
    """backup = p, then p += sam[1] * s^2 * grad_scale * g on the items of the unfrozen groups; nothing when sam[2] != 0."""
    n, pi, ni, pg, ng = _group_tables(p, items, groups, g, backup)
    require_cuda(sam)
    _f32(sam, n=4)
    check(lib().cx_sam_perturb_items(ptr(p), ptr(g), ptr(backup), n, pi, _items_host(items, items_host), ni, pg, ng, ptr(sam),
                                     grad_scale, int(bool(adaptive)), stream_ptr()), "cx_sam_perturb_items")


def sam_restore_items(p, backup, items, groups, sam, items_host=None):
    """p = backup on the items of the unfrozen groups (a copy); nothing when sam[2] != 0."""
    n, pi, ni, pg, ng = _group_tables(p, items, groups, backup)
    require_cuda(sam)
    _f32(sam, n=4)
    check(lib().cx_sam_restore_items(ptr(p), ptr(backup), n, pi, _items_host(items, items_host), ni, pg, ng, ptr(sam), stream_ptr()),
          "cx_sam_restore_items")


def bf16_to_f32_nchw(x, out=None):
    B, H, W, Cc, ldx = _nhwc(x)
    if out is None:
        out = torch.empty(B, Cc, H, W, dtype=torch.float32, device=x.device)
    check(lib().cx_bf16_to_f32_nchw(ptr(x), ptr(out), B, H, W, Cc, ldx, stream_ptr()), "cx_bf16_to_f32_nchw")
    return out


# ---- attention-augmented convolution pieces (csrc/aaconv.hip)
def aa_attention_fwd(qkv, key_rel_h, key_rel_w, o, lse, nh, dk, dv):
    B, H, W, Cq, ldq = _nhwc(qkv)
    check(_fn("cx_aa_attention_fwd", qkv)(ptr(qkv), ptr(key_rel_h), ptr(key_rel_w), ptr(o), ptr(lse), B, H, W, nh, dk, dv, ldq, stream_ptr()),
          "cx_aa_attention_fwd")


def aa_attention_weights(qkv, key_rel_h, key_rel_w, lse, nh, dk, dv):
    """softmax(logits) (B, nh, HW, HW) fp32 of the forward that produced `qkv` / `lse` (AAConv2d.weights, attn_aug_conv.py:87)."""
    B, H, W, Cq, ldq = _nhwc(qkv)
    out = torch.empty(B, nh, H * W, H * W, dtype=torch.float32, device=qkv.device)
    check(_fn("cx_aa_attention_weights", qkv)(ptr(qkv), ptr(key_rel_h), ptr(key_rel_w), ptr(lse), ptr(out), B, H, W, nh, dk, dv, ldq,
                                        stream_ptr()), "cx_aa_attention_weights")
    return out


def aa_attention_bwd(qkv, key_rel_h, key_rel_w, o, d_o, lse, dqkv, d_rel_h, d_rel_w, nh, dk, dv):
    """With the slab workspace on (set_det_wgrad) the relative-table gradients are summed in workgroup order (reproducible)."""
    B, H, W, Cq, ldq = _nhwc(qkv)
    ws = wgrad_scratch(qkv.device)                 # partial tables are consumed inside the call: the per-stream scratch is enough
    need = ((H * W + 127) // 128) * B * nh * (dk // nh) * (2 * H - 1 + 2 * W - 1)
    if ws is not None and ws.numel() < need:
        ws = _big_scratch(qkv.device, need)
    check(_fn("cx_aa_attention_bwd", qkv)(ptr(qkv), ptr(key_rel_h), ptr(key_rel_w), ptr(o), ptr(d_o), ptr(lse), ptr(dqkv), ptr(d_rel_h),
                                    ptr(d_rel_w), B, H, W, nh, dk, dv, ldq, ptr(ws), 0 if ws is None else ws.numel(), stream_ptr()),
          "cx_aa_attention_bwd")


_big = {}


def _big_scratch(device, floats):
    """A larger per-(device, stream) workspace for the few calls whose partial results exceed the default slab buffer."""
    key = (device.index, torch.cuda.current_stream(device).cuda_stream)
    t = _big.get(key)
    if t is None or t.numel() < floats:
        t = _big[key] = torch.empty(int(floats), dtype=torch.float32, device=device)
    return t


def aa_outproj_fwd(o, w, y, stat_sum, stat_sq, stat_rows=0, stat_rstride=0):
    """stat_rows > 0: deterministic statistic rows (returns the number written), else atomics into stat_sum / stat_sq."""
    B, H, W, dv, ldy = _nhwc(y)
    check(_fn("cx_aa_outproj_fwd", y)(ptr(o), ptr(w), ptr(y), ldy, ptr(stat_sum), ptr(stat_sq), B * H * W, dv, stat_rows, stat_rstride,
                                  stream_ptr()), "cx_aa_outproj_fwd")
    return lib().cx_last_stat_rows() if stat_rows > 0 else None


def aa_outproj_bwd(g, gx, ga, gb, gc, o, w, d_o, dw):
    B, H, W, dv, ldg = _nhwc(g)
    ws, arena, dfr = _wgrad_ws(dw.device)
    check(_fn("cx_aa_outproj_bwd", g)(ptr(g), ldg, ptr(gx), _nhwc(gx)[4], ptr(ga), ptr(gb), ptr(gc), ptr(o), ptr(w), ptr(d_o), ptr(dw),
                                  B * H * W, dv, ptr(ws), 0 if ws is None else ws.numel(), stream_ptr()), "cx_aa_outproj_bwd")
    _wgrad_used(arena, dfr)


def rows_reduce(dst, rows, n_rows, C, rstride, accumulate=True):
    check(lib().cx_rows_reduce(ptr(dst), ptr(rows), n_rows, C, rstride, int(accumulate), stream_ptr()), "cx_rows_reduce")


def copy_stream(src, dst):
    """dst = src through the library's own 16-byte-per-lane copy kernel (the measured stream rate bench.py reports)."""
    require_cuda(src, dst)
    n = src.numel() * src.element_size()
    if dst.numel() * dst.element_size() != n or not (src.is_contiguous() and dst.is_contiguous()):
        raise RuntimeError("copy_stream needs two contiguous buffers of equal size")
    check(lib().cx_copy_stream(ptr(src), ptr(dst), n, stream_ptr()), "cx_copy_stream")


def stats_bc(x, s, q):
    B, H, W, Cc, ldx = _nhwc(x)
    check(_fn("cx_stats_bc", x)(ptr(x), ptr(s), ptr(q), B, H * W, Cc, ldx, stream_ptr()), "cx_stats_bc")


def affine_relu_bc(x, sc, sh, y):
    B, H, W, Cc, ldx = _nhwc(x)
    assert _nhwc(y)[4] == Cc
    check(_fn("cx_affine_relu_bc", x)(ptr(x), ptr(sc), ptr(sh), ptr(y), B, H * W, Cc, ldx, stream_ptr()), "cx_affine_relu_bc")


def in_relu_bwd(da, x, sc, sh, S1, S2, gout):
    B, H, W, Cc, ldx = _nhwc(x)
    assert _nhwc(da)[4] == Cc
    check(_fn("cx_in_relu_bwd", da)(ptr(da), ptr(x), ptr(sc), ptr(sh), ptr(S1), ptr(S2), ptr(gout), B, H * W, Cc, ldx, _nhwc(gout)[4],
                               stream_ptr()), "cx_in_relu_bwd")


def f32_to_bf16(x, y):
    check(lib().cx_f32_to_bf16(ptr(x), ptr(y), x.numel(), stream_ptr()), "cx_f32_to_bf16")


# ---- EfficientNet pieces (csrc/dwconv.hip, csrc/effnet.hip): depthwise convolution, squeeze-excite, Swish glue.  None of these
# kernels takes a pitch: every NHWC operand is dense.  stat_rows > 0: deterministic statistic rows (the count written is returned),
# 0: fp32 atomics into [C] vectors.  rows: the optional row scratch of the per-(image, channel) sums (None: atomics).
def _out_hw(H, W, k, stride, pad):
    return (H + 2 * pad - k) // stride + 1, (W + 2 * pad - k) // stride + 1


def dwconv_fwd(x, w, sc, sh, y, stat_sum, stat_sq, *, k, stride, pad, stat_rows=0):
    """cx_dwconv_fwd: y = depthwise k x k convolution (w fp32 (C,1,k,k)) of swish(x*sc + sh) (sc None: of x) + the sums of y."""
    require_cuda(x, w, y)
    B, H, W, Cc = _dense(x)
    assert _dense(y) == (B, *_out_hw(H, W, k, stride, pad), Cc) and y.dtype == x.dtype
    _f32(sc, sh, stat_sum, stat_sq, n=Cc)
    _f32(w, n=Cc * k * k)
    check(_fn("cx_dwconv_fwd", x)(ptr(x), ptr(w), ptr(sc), ptr(sh), ptr(y), ptr(stat_sum), ptr(stat_sq), B, H, W, Cc, k, stride, pad,
                                  stat_rows, stream_ptr()), "cx_dwconv_fwd")
    return lib().cx_last_stat_rows() if stat_rows else None


def dwconv_dgrad(g, g2, ga, gb, gc, w, x, sc, sh, mean, rstd, dz, S1, S2, *, k, stride, pad, accumulate=False, stat_rows=0):
    """cx_dwconv_dgrad: dY = g*ga + g2*gb + gc; dz (+)= (sum_taps dY w) * swish'(x*sc + sh) with the BatchNorm backward sums S1 / S2
    of dz (sc None: dz is the plain input gradient, no sums)."""
    require_cuda(g, g2, w, x, dz)
    B, H, W, Cc = _dense(x)
    assert _dense(g) == (B, *_out_hw(H, W, k, stride, pad), Cc) and g.dtype == x.dtype
    _dense(g2, g)
    _dense(dz, x)
    _f32(ga, gb, gc, sc, sh, mean, rstd, S1, S2, n=Cc)
    _f32(w, n=Cc * k * k)
    check(_fn("cx_dwconv_dgrad", x)(ptr(g), ptr(g2), ptr(ga), ptr(gb), ptr(gc), ptr(w), ptr(x), ptr(sc), ptr(sh), ptr(mean), ptr(rstd),
                                    ptr(dz), ptr(S1), ptr(S2), B, H, W, Cc, k, stride, pad, int(accumulate), stat_rows, stream_ptr()),
          "cx_dwconv_dgrad")
    return lib().cx_last_stat_rows() if stat_rows else None


def dwconv_wgrad(g, g2, ga, gb, gc, x, sc, sh, dw, *, k, stride, pad):
    """cx_dwconv_wgrad: dw (fp32 (C,1,k,k)) += the depthwise weight gradient at dY = g*ga + g2*gb + gc and the input
    swish(x*sc + sh) (sc None: x), through the slab workspace (reproducible, deferrable) when it is on."""
    require_cuda(g, g2, x, dw)
    B, H, W, Cc = _dense(x)
    assert _dense(g) == (B, *_out_hw(H, W, k, stride, pad), Cc) and g.dtype == x.dtype
    _dense(g2, g)
    _f32(ga, gb, gc, sc, sh, n=Cc)
    _f32(dw, n=Cc * k * k)
    ws, arena, dfr = _wgrad_ws(dw.device)
    check(_fn("cx_dwconv_wgrad", x)(ptr(g), ptr(g2), ptr(ga), ptr(gb), ptr(gc), ptr(x), ptr(sc), ptr(sh), ptr(dw), B, H, W, Cc, k, stride,
                                    pad, ptr(ws), 0 if ws is None else ws.numel(), stream_ptr()), "cx_dwconv_wgrad")
    _wgrad_used(arena, dfr)


def gap_se_fwd(x, sc, sh, pooled, w1, b1, w2, b2, h1, s, *, act=2, rows=None):
    """cx_gap_se_fwd: pooled = mean_hw act(x*sc + sh) (act 0 none / 1 ReLU / 2 Swish), h1 = W1 pooled + b1,
    s = sigmoid(W2 swish(h1) + b2): squeeze + excitation in two launches."""
    require_cuda(x, pooled, w1, w2, h1, s)
    B, H, W, Cc = _dense(x)
    R = h1.shape[1]
    assert tuple(pooled.shape) == tuple(s.shape) == (B, Cc) and tuple(h1.shape) == (B, R)
    _f32(sc, sh, b2, n=Cc)
    _f32(pooled, s, rows, n=B * Cc)
    _f32(w1, w2, n=R * Cc)
    _f32(b1, h1, n=R)
    check(_fn("cx_gap_se_fwd", x)(ptr(x), ptr(sc), ptr(sh), ptr(pooled), ptr(w1), ptr(b1), ptr(w2), ptr(b2), ptr(h1), ptr(s), B, H * W, Cc,
                                  R, act, ptr(rows), 0 if rows is None else rows.numel(), stream_ptr()), "cx_gap_se_fwd")


def scale_act_bc(x, sc, sh, s, u):
    """cx_scale_act_bc: u = swish(x*sc + sh) * s[b][c] (s None: no squeeze-excite scaling)."""
    require_cuda(x, s, u)
    B, H, W, Cc = _dense(x)
    _dense(u, x)
    _f32(sc, sh, n=Cc)
    _f32(s, n=B * Cc)
    check(_fn("cx_scale_act_bc", x)(ptr(x), ptr(sc), ptr(sh), ptr(s), ptr(u), B, H * W, Cc, stream_ptr()), "cx_scale_act_bc")


def gap_affine_act(x, sc, sh, pooled, *, act, rows=None):
    """cx_gap_affine_act: pooled[b][c] = mean_hw act(x*sc + sh) (act as gap_se_fwd)."""
    require_cuda(x, pooled)
    B, H, W, Cc = _dense(x)
    _f32(sc, sh, n=Cc)
    _f32(pooled, rows, n=B * Cc)
    check(_fn("cx_gap_affine_act", x)(ptr(x), ptr(sc), ptr(sh), ptr(pooled), B, H * W, Cc, act, ptr(rows),
                                      0 if rows is None else rows.numel(), stream_ptr()), "cx_gap_affine_act")


def se_bwd_fused(du, x, sc, sh, ds, s, h1, pooled, w1, w2, dw1, db1, dw2, db2, dpooled, *, rows=None):
    """cx_se_bwd_fused: ds[b][c] = sum_hw du * swish(x*sc + sh) and the backward of the two squeeze-excite FCs (their gradients
    added into dw1 / db1 / dw2 / db2 through the slab workspace when it is on; dpooled written)."""
    require_cuda(du, x, ds, s, h1, pooled, w1, w2, dw1, db1, dw2, db2, dpooled)
    B, H, W, Cc = _dense(x)
    _dense(du, x)
    R = h1.shape[1]
    assert tuple(s.shape) == tuple(pooled.shape) == tuple(ds.shape) == tuple(dpooled.shape) == (B, Cc) and tuple(h1.shape) == (B, R)
    _f32(sc, sh, db2, n=Cc)
    _f32(ds, s, pooled, dpooled, rows, n=B * Cc)
    _f32(w1, w2, dw1, dw2, n=R * Cc)
    _f32(h1, db1, n=R)
    ws, arena, dfr = _wgrad_ws(dw1.device)
    check(_fn("cx_se_bwd_fused", x)(ptr(du), ptr(x), ptr(sc), ptr(sh), ptr(ds), ptr(s), ptr(h1), ptr(pooled), ptr(w1), ptr(w2), ptr(dw1),
                                    ptr(db1), ptr(dw2), ptr(db2), ptr(dpooled), B, H * W, Cc, R, ptr(rows),
                                    0 if rows is None else rows.numel(), ptr(ws), 0 if ws is None else ws.numel(), stream_ptr()),
          "cx_se_bwd_fused")
    _wgrad_used(arena, dfr)


def se_act_bwd(du, x, sc, sh, mean, rstd, s, dpooled, dz, S1, S2, stat_rows=0):
    """cx_se_act_bwd: dz = (du*s[b][c] + dpooled[b][c]/HW) * swish'(x*sc + sh) (du or dpooled / s may be None) with the BatchNorm
    backward sums S1 / S2 of dz."""
    require_cuda(du, x, s, dpooled, dz)
    B, H, W, Cc = _dense(x)
    _dense(dz, x)
    if du is not None:
        _dense(du, x)
    _f32(sc, sh, mean, rstd, S1, S2, n=Cc)
    _f32(s, dpooled, n=B * Cc)
    check(_fn("cx_se_act_bwd", x)(ptr(du), ptr(x), ptr(sc), ptr(sh), ptr(mean), ptr(rstd), ptr(s), ptr(dpooled), ptr(dz), ptr(S1), ptr(S2),
                                  B, H * W, Cc, stat_rows, stream_ptr()), "cx_se_act_bwd")
    return lib().cx_last_stat_rows() if stat_rows else None


def bn_lin_bwd_stats(g, y, mean, rstd, S1, S2, stat_rows=0):
    """cx_bn_lin_bwd_stats: the backward sums S1 = sum g, S2 = sum g * (y - mean) * rstd of a BatchNorm without activation."""
    require_cuda(g, y)
    B, H, W, Cc = _dense(g)
    _dense(y, g)
    _f32(mean, rstd, S1, S2, n=Cc)
    check(_fn("cx_bn_lin_bwd_stats", g)(ptr(g), ptr(y), ptr(mean), ptr(rstd), ptr(S1), ptr(S2), B * H * W, Cc, stat_rows, stream_ptr()),
          "cx_bn_lin_bwd_stats")
    return lib().cx_last_stat_rows() if stat_rows else None


def affine2_out(a, b, pa, pb, pc, sample_scale, out):
    """cx_affine2_out: out = s * (a*pa + pc) + b*pb; b (the skip input) and s = sample_scale[image] (DropConnect) may be None."""
    require_cuda(a, b, sample_scale, out)
    B, H, W, Cc = _dense(a)
    _dense(out, a)
    if b is not None:
        _dense(b, a)
    _f32(pa, pb, pc, n=Cc)
    _f32(sample_scale, n=B)
    check(_fn("cx_affine2_out", a)(ptr(a), ptr(b), ptr(pa), ptr(pb), ptr(pc), ptr(sample_scale), H * W, ptr(out), B * H * W, Cc,
                                   stream_ptr()), "cx_affine2_out")


def scale_rows(g, sample_scale, out):
    """cx_scale_rows: out = sample_scale[image] * g: the gradient that enters a DropConnect-ed branch."""
    require_cuda(g, sample_scale, out)
    B, H, W, Cc = _dense(g)
    _dense(out, g)
    _f32(sample_scale, n=B)
    check(_fn("cx_scale_rows", g)(ptr(g), ptr(sample_scale), H * W, ptr(out), B * H * W, Cc, stream_ptr()), "cx_scale_rows")


def dropout_mask_dev(out, keep_prob, base, step):
    """cx_dropout_mask_dev: out[i] in {0, 1/keep_prob}, a counter-based Bernoulli mask whose seed is base + step[0] * 1000003 (step:
    the int64 device counter counter_add bumps)."""
    require_cuda(out, step)
    _f32(out)
    assert step.dtype == torch.int64 and step.numel() == 1
    check(lib().cx_dropout_mask_dev(ptr(out), out.numel(), keep_prob, base, ptr(step), stream_ptr()), "cx_dropout_mask_dev")


def counter_add(counter, inc=1):
    """cx_counter_add: counter[0] += inc on the device (one int64)."""
    require_cuda(counter)
    assert counter.dtype == torch.int64 and counter.numel() == 1
    check(lib().cx_counter_add(ptr(counter), inc, stream_ptr()), "cx_counter_add")


def mul_f32(a, b, out):
    """cx_mul_f32: out = a * b, element-wise on fp32 (out may be a)."""
    require_cuda(a, b, out)
    _f32(a, b, out, n=a.numel())
    check(lib().cx_mul_f32(ptr(a), ptr(b), ptr(out), a.numel(), stream_ptr()), "cx_mul_f32")


def linear_fwd(x, w, bias, y):
    """cx_linear_fwd: y (B,N) = x (B,C) W^T + bias, all fp32 (bias None: no bias)."""
    require_cuda(x, w, bias, y)
    (B, Cc), N = x.shape, y.shape[1]
    assert y.shape[0] == B and tuple(w.shape) == (N, Cc) and (bias is None or bias.numel() == N)
    _f32(x, w, bias, y)
    check(lib().cx_linear_fwd(ptr(x), ptr(w), ptr(bias), ptr(y), B, Cc, N, stream_ptr()), "cx_linear_fwd")


# ---- Grad-CAM (csrc/gradcam.hip) on a bf16 NHWC feature map that may be a channel slice
def affine_to_f32_nchw(x, scale, shift, relu, out):
    """cx_affine_to_f32_nchw: out (B,C,H,W) fp32 = act(x*scale + shift) (scale / shift None: identity; relu: ReLU)."""
    require_cuda(x, scale, shift, out)
    B, H, W, Cc, ldx = _nhwc(x)
    _f32(scale, shift, n=Cc)
    _f32(out)
    assert tuple(out.shape) == (B, Cc, H, W)
    check(_fn("cx_affine_to_f32_nchw", x)(ptr(x), ptr(scale), ptr(shift), int(relu), ptr(out), B, H, W, Cc, ldx, stream_ptr()),
          "cx_affine_to_f32_nchw")


def gradcam_map(x, scale, shift, w, cam, inner_relu):
    """cx_gradcam_map: cam (B,HW) = relu(sum_c w[c] * f(x*scale + shift)), f = ReLU when inner_relu else the identity."""
    require_cuda(x, scale, shift, w, cam)
    B, H, W, Cc, ldx = _nhwc(x)
    _f32(scale, shift, w, n=Cc)
    _f32(cam, n=B * H * W)
    check(_fn("cx_gradcam_map", x)(ptr(x), ptr(scale), ptr(shift), ptr(w), ptr(cam), B, H * W, Cc, ldx, inner_relu, stream_ptr()),
          "cx_gradcam_map")


CAM_ACT_NONE, CAM_ACT_RELU, CAM_ACT_SWISH = 0, 1, 2


def class_cam(x, scale, shift, w, cam, *, act, relu=True, cls=None):
    """cx_class_cam: cam (B,K,H*W) fp32 = post(1/(H*W) * sum_f w[cls(b,k), f] * act(x*scale + shift)), all K classes in one launch that
    reads x once.  x: bf16 or fp32-mode NHWC view (channel pitch allowed); scale / shift: fp32 (C) or both None (identity);
    act: CAM_ACT_*; w: fp32 (n_classes, C) with unit column stride; post = ReLU when `relu`.
    cls: None -- map k is class k, K = n_classes; a list / tuple of K class indices -- the same classes for every image, range-checked
    here (ValueError) before anything is launched; an int32 device tensor (B, K) -- one row of classes per image, NOT checked (that
    would be a host sync): the kernel clamps every entry into [0, n_classes)."""
    require_cuda(x, scale, shift, w, cam)
    B, H, W, Cc, ldx = _nhwc(x)
    assert (scale is None) == (shift is None), "scale and shift come together"
    _f32(scale, shift, n=Cc)
    assert act in (CAM_ACT_NONE, CAM_ACT_RELU, CAM_ACT_SWISH), "act is one of ops.CAM_ACT_*"
    assert w.dtype == torch.float32 and w.dim() == 2 and w.shape[1] == Cc and w.stride(1) == 1, "w: fp32 (n_classes, C) rows"
    n_classes, ldw = w.shape[0], w.stride(0)
    assert cam.dtype == torch.float32 and cam.is_contiguous() and cam.dim() == 3 and cam.shape[0] == B and cam.shape[2] == H * W, \
        "cam: contiguous fp32 (B, K, H*W)"
    K = cam.shape[1]
    if isinstance(cls, (list, tuple)):
        if len(cls) != K or K < 1:
            raise ValueError("class_cam: %d class indices for %d maps per image" % (len(cls), K))
        if not all(isinstance(c, int) and 0 <= c < n_classes for c in cls):
            raise ValueError("class_cam: class indices must be ints in [0, %d) (got %s)" % (n_classes, list(cls)))
        cls = torch.tensor(list(cls), dtype=torch.int32).repeat(B, 1).to(x.device)
    if cls is not None:
        require_cuda(cls)
        assert cls.dtype == torch.int32 and cls.is_contiguous() and tuple(cls.shape) == (B, K), "cls: contiguous int32 (B, K)"
    else:
        assert K == n_classes, "without a class table the maps are those of all n_classes classes"
    check(_fn("cx_class_cam", x)(ptr(x), ptr(scale), ptr(shift), ptr(w), ptr(cls), ptr(cam), B, H * W, Cc, ldx, n_classes, ldw, K,
                                 act, int(bool(relu)), stream_ptr()), "cx_class_cam")


def cam_norm_upsample(cam, out, h, w):
    """cx_cam_norm_upsample: out (B,1,H,W) = the h x w maps cam (B,h*w) scaled to [0, 1] per image and up-sampled bilinearly."""
    require_cuda(cam, out)
    B, _, H, W = out.shape
    assert tuple(cam.shape) == (B, h * w) and out.shape[1] == 1
    _f32(cam, out)
    check(lib().cx_cam_norm_upsample(ptr(cam), ptr(out), B, h, w, H, W, stream_ptr()), "cx_cam_norm_upsample")


# ---- evaluation statistics over per-class entry lists (bootstrap.hip, calib.hip, delong.hip; the header's constants are in _lib.py) ----
def _class_lists(what, counts, order, offs, lens, n_units, per_class=1, min_classes=0):
    """What boot_auc, boot_sweep, boot_calib and delong_place check alike: counts (None: the kernel reads no table) is int32
    (n_rep, >= n_units) on the GPU with unit row stride, order a contiguous int32 device tensor, and class c's per_class lists of
    lens[c] entries from offs[c] lie inside it (ValueError in `what`'s name otherwise).  Returns (ld, n_rep, n_cls, offs, lens): the
    row pitch to pass for counts and the two host sequences as the ctypes arrays the entry points take."""
    require_cuda(counts, order)
    assert counts is None or (counts.dtype == torch.int32 and counts.dim() == 2 and counts.stride(1) == 1 and counts.shape[1] >= n_units), \
        "counts: int32 (n_rep, >= n_units) rows"
    assert order.dtype == torch.int32 and order.dim() == 1 and order.is_contiguous(), "order: contiguous int32"
    offs, lens = [int(v) for v in offs], [int(v) for v in lens]
    n_cls, n_rep = len(lens), 0 if counts is None else counts.shape[0]
    if n_cls < min_classes or len(offs) != n_cls or any(n < 0 or o < 0 or o + per_class * n > order.numel() for o, n in zip(offs, lens)):
        raise ValueError("%s: offsets %s / lengths %s do not fit an order array of %d entries" % (what, offs, lens, order.numel()))
    ld = 0 if counts is None else counts.stride(0) if n_rep > 1 else counts.shape[1]
    return ld, n_rep, n_cls, (C.c_int64 * n_cls)(*offs), (C.c_int32 * n_cls)(*lens)


def boot_counts(n_units, n_rep, seed, first=0, out=None, device="cuda"):
    """cx_boot_counts: rows first .. first + n_rep - 1 of the bootstrap count table as an (n_rep, n_units) int32 tensor on the GPU
    (the kernel's uint32; a count is at most n_units <= 2^24): element [r, u] is the number of the n_units draws of replicate
    first + r that hit unit u.  A row depends on (seed, first + r, n_units) only.  `out`: a contiguous int32 (>= n_rep, n_units)
    tensor whose first n_rep rows are written and returned.  Up to BOOT_MAX_TILES * BOOT_TILE units a workgroup counts a tile of
    BOOT_TILE units in LDS; above that the hits are added in device memory."""
    n_units, n_rep, first = int(n_units), int(n_rep), int(first)
    if out is None:
        out = torch.empty(max(n_rep, 0), max(n_units, 0), dtype=torch.int32, device=device)
    require_cuda(out)
    assert out.dtype == torch.int32 and out.dim() == 2 and out.is_contiguous() and out.shape[0] >= n_rep and out.shape[1] == n_units, \
        "out: contiguous int32 (>= n_rep, n_units)"
    check(lib().cx_boot_counts(ptr(out), out.stride(0) if out.shape[0] else n_units, n_units, first, n_rep, int(seed) & (2 ** 64 - 1),
                               stream_ptr()), "cx_boot_counts")
    return out[:n_rep]


def boot_auc(counts, order, offs, lens, n_units):
    """cx_boot_auc: the integer parts of the weighted AUROC of every (replicate, class).  counts: int32 (n_rep, >= n_units) on the GPU
    with unit row stride, read as uint32 (rows of boot_counts, or any non-negative weights whose row sum is < 2^32); order: int32
    device tensor holding, for class c, the `hi` then the `lo` order of its kept rows (lens[c] entries each, from offs[c]; an entry =
    unit index | label << 31; metrics.bootstrap_plan builds them); offs / lens: host sequences of C ints.  Returns int64 tensors
    (n_rep, C): num2, wpos, wneg with AUROC = num2 / (2 * wpos * wneg); a class with lens[c] == 0 gives zeros."""
    ld, n_rep, n_cls, offs, lens = _class_lists("boot_auc", counts, order, offs, lens, n_units, per_class=2)
    num2 = torch.empty(n_rep, n_cls, dtype=torch.int64, device=counts.device)
    wpos = torch.empty(n_rep, n_cls, dtype=torch.int32, device=counts.device)
    wneg = torch.empty_like(wpos)
    if n_rep == 0:
        return num2, wpos.long(), wneg.long()
    check(lib().cx_boot_auc(ptr(counts), ld, n_rep, ptr(order), offs, lens, n_cls, ptr(num2), ptr(wpos), ptr(wneg), int(n_units),
                            stream_ptr()), "cx_boot_auc")
    return num2, wpos.long() & 0xffffffff, wneg.long() & 0xffffffff      # the kernel's uint32 sums


def boot_sweep(counts, order, offs, lens, n_units, points=()):
    """cx_boot_sweep: the integer parts of the average precision and of fixed operating points of every (replicate, class).  counts: as
    boot_auc takes them; order: int32 device tensor holding, for class c, its kept rows once, descending in score (lens[c] entries from
    offs[c]; an entry = unit index | label << 31 | end of its tie group << 30; metrics.bootstrap_sweep_plan builds them); points: up to
    BOOT_MAX_POINTS pairs (BOOT_SENS or BOOT_SPEC, value in millionths 1 .. 999 999).  Returns int64 tensors apnum, wpos, wneg
    (n_rep, C) and pts (n_rep, C, len(points)): AP = apnum / (wpos * 2^32) with apnum the kernel's uint64 (read it as such: .numpy()
    .view(np.uint64); it passes 2^63 only when wpos does 2^31); sens@ = pts / wpos, spec@ = 1 - pts / wneg."""
    points = [(int(k), int(v)) for k, v in points]
    n_pts = len(points)
    ld, n_rep, n_cls, offs, lens = _class_lists("boot_sweep", counts, order, offs, lens, n_units)
    if n_pts > BOOT_MAX_POINTS or any(k not in (BOOT_SENS, BOOT_SPEC) or not 1 <= v <= 999999 for k, v in points):
        raise ValueError("boot_sweep: at most %d operating points (BOOT_SENS | BOOT_SPEC, 1 .. 999999 millionths), got %s"
                         % (BOOT_MAX_POINTS, points))
    apnum = torch.empty(n_rep, n_cls, dtype=torch.int64, device=counts.device)
    wpos = torch.empty(n_rep, n_cls, dtype=torch.int32, device=counts.device)
    wneg = torch.empty_like(wpos)
    pts = torch.empty(n_rep, n_cls, n_pts, dtype=torch.int32, device=counts.device)
    if n_rep == 0:
        return apnum, wpos.long(), wneg.long(), pts.long()
    check(lib().cx_boot_sweep(ptr(counts), ld, n_rep, ptr(order), offs, lens, n_cls, (C.c_int32 * max(n_pts, 1))(*[k for k, _ in points]),
                              (C.c_int32 * max(n_pts, 1))(*[v for _, v in points]), n_pts, ptr(apnum), ptr(wpos), ptr(wneg),
                              ptr(pts) if n_pts else None, int(n_units), stream_ptr()), "cx_boot_sweep")
    return apnum, wpos.long() & 0xffffffff, wneg.long() & 0xffffffff, pts.long() & 0xffffffff      # the kernel's unsigned values


# ---- calibration (calib.hip; chexpert_amd/calibration.py composes them and states them in numpy) ----
def calib_fit(logits, targets, method="temperature", smooth=False, g_tol=1e-10, max_iter=100):
    """cx_calib_fit: the per-class calibration map u = a z + b of (N, C) logits against (N, C) targets (target < 0: the row is left
    out of the class; positive iff target > 0.5), every class in one launch.  Returns a float64 (C, 8) tensor on the GPU: a, b,
    nll_before, nll_after, gmax, lambda_min, iterations, status (0 converged, 1 iteration cap, 2 degenerate, 3 flat; 2 / 3 return the
    identity).  ValueError before any launch: an unknown method, max_iter outside 1 .. CALIB_MAX_ITER, g_tol negative or NaN."""
    require_cuda(logits, targets)
    if method not in CALIB_METHODS:
        raise ValueError("calib_fit: method %r (one of %s)" % (method, sorted(CALIB_METHODS)))
    if not 1 <= int(max_iter) <= CALIB_MAX_ITER:
        raise ValueError("calib_fit: max_iter must be inside 1 .. %d (got %r)" % (CALIB_MAX_ITER, max_iter))
    if not float(g_tol) >= 0.0:
        raise ValueError("calib_fit: g_tol must be >= 0 (got %r)" % (g_tol,))
    assert logits.dim() == 2 and logits.shape == targets.shape, "logits / targets: (N, C) of one shape"
    n, n_cls = logits.shape
    z, t = logits.float().t().contiguous(), targets.float().t().contiguous()      # class-major (C, N)
    out = torch.tensor([1.0, 0.0, float("nan"), float("nan"), float("nan"), float("nan"), 0.0, 2.0], dtype=torch.float64,
                       device=logits.device).repeat(n_cls, 1)                     # what a class without rows is (N == 0: no launch)
    check(lib().cx_calib_fit(ptr(z), ptr(t), n_cls, n, CALIB_METHODS[method], int(bool(smooth)), float(g_tol), int(max_iter), ptr(out),
                             stream_ptr()), "cx_calib_fit")
    return out


def boot_calib(counts, order, conf, offs, lens, n_units, bins):
    """cx_boot_calib: the integer bin sums behind ECE / MCE / Brier of every (replicate, class).  counts: as boot_auc takes them; order:
    int32 device tensor holding lens[c] entries for class c from offs[c] (an entry = unit index | bin << 24 | label << 31); conf: int32
    device tensor parallel to order, the fixed-point confidences read as uint32 (calibration.calibration_plan builds both); bins: M in
    1 .. CALIB_MAX_BINS.  Returns int64 tensors wsum, wpos, csum (n_rep, C, M) and bnum (n_rep, C); csum and bnum hold the kernel's
    uint64 (read them as such: .numpy().view(np.uint64)).  ValueError before any launch: offsets / lengths that do not fit the order
    array, a conf of another length, bins outside 1 .. CALIB_MAX_BINS."""
    require_cuda(conf)
    assert conf.dtype == torch.int32 and conf.dim() == 1 and conf.is_contiguous(), "conf: contiguous int32"
    bins = int(bins)
    ld, n_rep, n_cls, offs, lens = _class_lists("boot_calib", counts, order, offs, lens, n_units)
    if conf.numel() != order.numel():
        raise ValueError("boot_calib: %d confidences for %d entries" % (conf.numel(), order.numel()))
    if not 1 <= bins <= CALIB_MAX_BINS:
        raise ValueError("boot_calib: %d bins (1 .. %d are supported)" % (bins, CALIB_MAX_BINS))
    wsum = torch.empty(n_rep, n_cls, bins, dtype=torch.int32, device=counts.device)
    wpos = torch.empty_like(wsum)
    csum = torch.empty(n_rep, n_cls, bins, dtype=torch.int64, device=counts.device)
    bnum = torch.empty(n_rep, n_cls, dtype=torch.int64, device=counts.device)
    if n_rep == 0 or n_cls == 0:
        return wsum.long(), wpos.long(), csum, bnum
    check(lib().cx_boot_calib(ptr(counts), ld, n_rep, ptr(order), ptr(conf), offs, lens, n_cls, bins, ptr(wsum), ptr(wpos), ptr(csum),
                              ptr(bnum), int(n_units), stream_ptr()), "cx_boot_calib")
    return wsum.long() & 0xffffffff, wpos.long() & 0xffffffff, csum, bnum      # the kernel's unsigned values


# ---- DeLong / Obuchowski variance of the AUROC (delong.hip; chexpert_amd/metrics.py composes them and states them in numpy) ----
def delong_place(order, offs, lens, n_units, out=None):
    """cx_delong_place: the unit sums of the doubled placements.  order / offs / lens: what boot_auc takes (metrics.bootstrap_plan builds
    them).  Returns an int64 (4 C, n_units) tensor on the GPU, rows 4c .. 4c+3 = (sum of X2 over the unit's positives, their number, sum
    of Y2 over its negatives, their number) of class c; a class with lens[c] == 0 gives zeros.  `out`: an int64 (4 C, >= n_units) tensor
    with unit column stride whose first n_units columns are written (zeroed first) and returned; the columns behind them are left
    untouched.  A workgroup walks DELONG_WG_ENTRIES entries of a list."""
    n_units = int(n_units)
    _, _, n_cls, offs, lens = _class_lists("delong_place", None, order, offs, lens, n_units, per_class=2, min_classes=1)
    if not 1 <= n_units <= BOOT_MAX_UNITS:
        raise ValueError("delong_place: %d units (1 .. 2^24 are supported)" % n_units)
    if out is None:
        out = torch.empty(4 * n_cls, n_units, dtype=torch.int64, device=order.device)
    require_cuda(out)
    assert out.dtype == torch.int64 and out.dim() == 2 and out.shape[0] == 4 * n_cls and out.shape[1] >= n_units and out.stride(1) == 1 \
        and (out.shape[0] == 1 or out.stride(0) >= n_units), "out: int64 (4 C, >= n_units) rows"
    check(lib().cx_delong_place(ptr(order), offs, lens, n_cls, n_units, ptr(out), out.stride(0), stream_ptr()), "cx_delong_place")
    return out[:, :n_units]


def int_gram(z, n_units):
    """cx_delong_gram: g = z[:, :n_units] @ z[:, :n_units].T in int64 arithmetic that wraps mod 2^64.  z: int64 (Q, >= n_units) on the GPU
    with unit column stride, Q in 1 .. DELONG_MAX_ROWS.  Returns an int64 (Q, Q) tensor, symmetric."""
    require_cuda(z)
    n_units = int(n_units)
    assert z.dtype == torch.int64 and z.dim() == 2 and z.stride(1) == 1 and z.shape[1] >= n_units, "z: int64 (Q, >= n_units) rows"
    n_rows = z.shape[0]
    if not 1 <= n_rows <= DELONG_MAX_ROWS:
        raise ValueError("int_gram: %d rows (1 .. %d are supported)" % (n_rows, DELONG_MAX_ROWS))
    if not 1 <= n_units <= BOOT_MAX_UNITS:
        raise ValueError("int_gram: %d units (1 .. 2^24 are supported)" % n_units)
    g = torch.empty(n_rows, n_rows, dtype=torch.int64, device=z.device)
    check(lib().cx_delong_gram(ptr(z), z.stride(0) if n_rows > 1 else z.shape[1], n_rows, n_units, ptr(g), stream_ptr()), "cx_delong_gram")
    return g


# ---- pixel attribution maps (saliency.hip; chexpert_amd/saliency.py composes them and states them in numpy) ----
SAL_MODES = {"none": 0, "sum": 1, "abs": 2, "max": 3}      # CX_SAL_NONE .. CX_SAL_MAX of the header
SAL_PARTIALS = 128                                          # CX_SAL_PARTIALS


def _sal_images(t, what):
    assert t.dtype == torch.float32 and t.is_contiguous() and t.dim() == 4 and t.shape[1] == 3, "%s: contiguous fp32 (.,3,H,W)" % what
    return t.shape[0], t.shape[2], t.shape[3]


def _sal_table(t, dtype, n, what):
    assert t.dtype == dtype and t.is_contiguous() and t.numel() == n, "%s: contiguous %s of %d entries" % (what, dtype, n)


def _sal_base(base, x):
    """(full baseline or None, the three per-channel constants) of a baseline given as a (B,3,H,W) tensor or as three floats."""
    if isinstance(base, torch.Tensor):
        assert base.shape == x.shape, "a full baseline has the input's shape"
        _sal_images(base, "base")
        return base, (0.0, 0.0, 0.0)
    b = tuple(float(v) for v in base)
    assert len(b) == 3, "a constant baseline is three floats, one per channel"
    return None, b


def sal_points(x, base, img, alpha, out=None, *, sigma=None, seed=0, first_row=0):
    """cx_sal_points: out (R,3,H,W) = base[img[r]] + alpha[r] * (x[img[r]] - base[img[r]]) [+ sigma[img[r]] * n(seed, first_row + r, .)],
    every product and sum rounded on its own.  x: fp32 (B,3,H,W); base: a tensor of x's shape or three per-channel floats; img int32 (R,),
    alpha fp32 (R,), sigma None or fp32 (B,), all on the device."""
    require_cuda(x, img, alpha, sigma, out)
    B, H, W = _sal_images(x, "x")
    R = img.numel()
    _sal_table(img, torch.int32, R, "img")
    _sal_table(alpha, torch.float32, R, "alpha")
    if sigma is not None:
        _sal_table(sigma, torch.float32, B, "sigma")
    full, const = _sal_base(base, x)
    require_cuda(full)
    if out is None:
        out = torch.empty(R, 3, H, W, dtype=torch.float32, device=x.device)
    assert _sal_images(out, "out") == (R, H, W)
    check(lib().cx_sal_points(ptr(x), ptr(full), const[0], const[1], const[2], ptr(img), ptr(alpha), ptr(sigma), int(seed) & (2 ** 64 - 1),
                              int(first_row) & (2 ** 64 - 1), ptr(out), B, R, H, W, stream_ptr()), "cx_sal_points")
    return out


def sal_accumulate(g, slot, w, acc, *, square=False, accumulate=True):
    """cx_sal_accumulate: acc (P,3,H,W) = (acc if accumulate else 0) + sum over the rows r with slot[r] == p, in ascending order, of
    w[r] * (g[r]^2 if square else g[r]).  g: fp32 (R,3,H,W); slot int32 (R,), w fp32 (R,) on the device."""
    require_cuda(g, slot, w, acc)
    R, H, W = _sal_images(g, "g")
    P, Ha, Wa = _sal_images(acc, "acc")
    assert (Ha, Wa) == (H, W), "acc and g share H and W"
    _sal_table(slot, torch.int32, R, "slot")
    _sal_table(w, torch.float32, R, "w")
    check(lib().cx_sal_accumulate(ptr(g), ptr(slot), ptr(w), ptr(acc), R, P, H, W, int(bool(square)), int(bool(accumulate)), stream_ptr()),
          "cx_sal_accumulate")
    return acc


def sal_finish(acc, x=None, base=(0.0, 0.0, 0.0), img_of=None, *, times_input=False, channels="none", total=False):
    """cx_sal_finish: a = acc * (x[img_of[p]] - base[img_of[p]]) with times_input, else acc; the map (P,3,H,W) for channels "none",
    else (P,H,W): "sum" (a0 + a1) + a2, "abs" (|a0| + |a1|) + |a2|, "max" the largest |a_c|.  Returns (map, total): total is None, or
    with total=True the float64 (P,) sums of a over each plane."""
    require_cuda(acc, x, img_of)
    if channels not in SAL_MODES:
        raise ValueError("sal_finish: channels is one of %s (got %r)" % (", ".join(SAL_MODES), channels))
    P, H, W = _sal_images(acc, "acc")
    B, full, const = 0, None, (0.0, 0.0, 0.0)
    if times_input:
        B, Hx, Wx = _sal_images(x, "x")
        assert (Hx, Wx) == (H, W), "acc and x share H and W"
        _sal_table(img_of, torch.int32, P, "img_of")
        full, const = _sal_base(base, x)
        require_cuda(full)
    out = torch.empty((P, 3, H, W) if channels == "none" else (P, H, W), dtype=torch.float32, device=acc.device)
    tot = torch.empty(P, dtype=torch.float64, device=acc.device) if total else None
    part = torch.empty(P * SAL_PARTIALS, dtype=torch.float64, device=acc.device) if total else None
    check(lib().cx_sal_finish(ptr(acc), ptr(x) if times_input else None, ptr(full), const[0], const[1], const[2],
                              ptr(img_of) if times_input else None, ptr(out), ptr(tot), ptr(part), P, B, H, W, int(bool(times_input)),
                              SAL_MODES[channels], stream_ptr()), "cx_sal_finish")
    return out, tot
