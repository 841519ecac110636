"""Geometric augmentation of the uint8 image hand-over: the host side of `cx_u8_affine` (chexpert_amd/csrc/augment.hip).

The warp itself is one HIP kernel on the decoded grey bytes (`ops.u8_affine`), between the loader's batch and `--jitter` / the first
kernel of the network; what lives here is the parameter draw (no GPU needed) and the CPU statement of the kernel's definition that
the tests hold it against.  The random step sits BEHIND the loader, so the decoded-image cache (`--cache_decoded`) stays valid.

Convention (kernel, `affine_matrices` and `affine_reference` alike).  mat[b] = (m0 .. m5) is the INVERSE map of image b, row-major
2x3, in pixel units about the image centre: output pixel (i, j) of an (H, W) image samples the source at

    xo = j + 0.5 - W/2              yo = i + 0.5 - H/2
    u  = m0*xo + m1*yo + m2 + W/2 - 0.5
    v  = m3*xo + m4*yo + m5 + H/2 - 0.5
    u0 = floor(u), v0 = floor(v), fu = u - u0, fv = v - v0
    p(r, c) = x[b][r][c] inside the image, else `fill`
    top = p(v0,u0)*(1-fu) + p(v0,u0+1)*fu ;  bot likewise on row v0+1
    y[b][i][j] = uint8(floor(top*(1-fv) + bot*fv + 0.5))

Contrast equalisation (CLAHE: `cx_u8_clahe_lut` + `cx_u8_clahe_apply`, chexpert_amd/csrc/clahe.hip; `ops.u8_clahe`) lives here too:
deterministic preprocessing rather than augmentation, so it runs in every mode, as the first step on the uint8 batch, before the
warp.  Its structure is OpenCV's `createCLAHE(clipLimit, tileGridSize)`, but it is NOT bit-equal to OpenCV, which rounds the tables
and the interpolation in float and anchors on pixel indices: the definition below is integer arithmetic throughout (kernel and
`clahe_reference` agree bit for bit), and tables sit at tile centres with pixel centres at half-integers.

x: uint8 (B, H, W) or (B, 1, H, W); grid (GY, GX), each 1..16, dividing (H, W); tile th = H / GY, tw = W / GX, area = th * tw; clip
limit c >= 0 (`//` is floor division):

    L = 0 if c == 0 else min(area, max(1, floor(c * area / 256)))          clip count (`clahe_clip_count`); 0 = no clipping

    table of tile (b, gy, gx), 256 bytes:
      hist[v] = number of pixels of the tile with value v
      if L > 0:  excess = sum(max(hist[v] - L, 0));  hist[v] = min(hist[v], L);  q, r = divmod(excess, 256)
                 hist[v] += q for every v
                 if r > 0: step = max(1, 256 // r); for v = 0, step, 2*step, ... < 256, while r > 0: hist[v] += 1, r -= 1
      cdf[v] = hist[0] + ... + hist[v];   lut[v] = (cdf[v] * 255 + area // 2) // area

    output pixel (i, j) with value v = x[b][i][j]:
      ay = 2*i + 1 - th;  gy0 = ay // (2*th)  (-1 in the top half tile);  wy = ay - gy0 * 2*th  (in [0, 2*th));  gy1 = gy0 + 1
      then gy0 and gy1 are clamped to [0, GY-1];  ax, gx0, wx, gx1 likewise with j, tw, GX
      num = (2*th - wy) * ((2*tw - wx) * lut[gy0][gx0][v] + wx * lut[gy0][gx1][v])
          +       wy    * ((2*tw - wx) * lut[gy1][gx0][v] + wx * lut[gy1][gx1][v])
      y[b][i][j] = (num + 2*th*tw) // (4*th*tw)

GY = GX = 1 with c = 0 is plain global histogram equalisation.

Sample mixing (Mixup, CutMix, random erasing: `cx_u8_mix` + `cx_target_mix`, chexpert_amd/csrc/mix.hip; `ops.u8_mix`,
`ops.target_mix`) is the LAST step on the uint8 batch: the per-sample transforms above come first and the collated batch is mixed
afterwards, as timm does.  A plan is four int32 arrays, perm (B,), lam_q (B,), box (B, 4) = y0 y1 x0 x1 and tw_q (B,); `mix_plan` and
`erase_plan` draw one, `mix_reference` / `target_mix_reference` state what the kernels make of it (bit for bit, `//`-free integers
and separately rounded fp32):

    p = clamp(perm[b], -1, B-1);  q = clamp(lam_q[b], 0, 65536);  y0, y1 clamped to [0, H];  x0, x1 clamped to [0, W]
    pixel (i, j), a = x[b][i][j]:   outside rows [y0, y1) x columns [x0, x1):  y = a
                                    inside:  o = fill if p < 0 else x[p][i][j];  y = (q*a + (65536 - q)*o + 32768) >> 16
    targets, w_q = clamp(tw_q[b], 0, 65536), w = w_q / 65536 (w and 1 - w exact in fp32):
      p < 0 or w_q == 65536:            out[b][c] = t[b][c]
      else t[b][c] < 0 or t[p][c] < 0:  out[b][c] = -1          (a label the loss ignores stays ignored)
      else:                             out[b][c] = fl(fl(w * t[b][c]) + fl((1 - w) * t[p][c]))

Mixup: box = the image, lam_q = tw_q = round(65536 lambda).  CutMix: a partial box, lam_q = 0, tw_q = the share of the row's own
pixels.  Erasing: perm = -1, lam_q = 0, tw_q = 65536 (labels do not change).
"""
import math

import torch

from . import synth

# --affine defaults of the command line; test-time augmentation (predict --tta) draws from half of these ranges
TRAIN_DEFAULTS = {"degrees": 10.0, "translate": 0.05, "scale": (0.9, 1.1), "shear": 0.0}
TTA_RANGES = {"degrees": 5.0, "translate": 0.025, "scale": (0.95, 1.05), "shear": 0.0}


def step_seed(step, rank=0):
    """Seed of minibatch `step` on data-parallel rank `rank`, built like the one of cli.py's jitter() (step * 7919 + 13 + rank) with
    another offset: a run is reproducible, the ranks draw different transforms, and the warp does not share its numbers with the
    jitter of the same step."""
    return int(step) * 7919 + 4001 + int(rank)


def mix_seed(step, rank=0):
    """step_seed's sibling for the --mixup / --cutmix plan of minibatch `step`: an offset of its own, so the mix shares no numbers
    with the erase, the warp or the jitter of the same step (the offsets stay below the 7919 between two steps)."""
    return int(step) * 7919 + 2003 + int(rank)


def erase_seed(step, rank=0):
    """step_seed's sibling for the --erase_prob plan of minibatch `step`."""
    return int(step) * 7919 + 6007 + int(rank)


def tta_seed_of(tta_seed, draw, batch):
    """Seed of test-time-augmentation draw `draw` (1 .. K-1) of minibatch number `batch`: a function of these three only."""
    return (int(tta_seed) * 8191 + int(draw)) * 1000003 + int(batch)


def affine_matrices(seed, B, H, W, degrees=10.0, translate=0.05, scale=(0.9, 1.1), shear=0.0):
    """(B, 6) fp32 inverse maps in the kernel's convention, drawn like torchvision's RandomAffine: angle uniform in +-degrees,
    translation uniform in +-translate * size per axis (kept fractional: the sampler is bilinear anyway, where torchvision rounds to
    whole pixels), scale uniform in [scale[0], scale[1]], shear along x uniform in +-shear degrees; composed as torchvision's
    _get_inverse_affine_matrix about the image centre (forward map = translate . rotate . shear . scale).  The numbers come from
    synth.uniform(seed, ...): pure functions of the seed.  Zero ranges give the identity exactly."""
    lo, hi = (float(scale[0]), float(scale[1])) if isinstance(scale, (tuple, list)) else (float(scale), float(scale))
    u = synth.uniform(seed, (5, B), 0.0, 1.0, dtype=torch.float64)
    rot = (2.0 * u[0] - 1.0) * math.radians(float(degrees))
    tx = (2.0 * u[1] - 1.0) * float(translate) * W
    ty = (2.0 * u[2] - 1.0) * float(translate) * H
    s = lo + u[3] * (hi - lo)
    sx = (2.0 * u[4] - 1.0) * math.radians(float(shear))
    # rotation . shear without the scale (determinant 1), then its inverse over the scale
    a, c = torch.cos(rot), torch.sin(rot)
    b = -a * torch.tan(sx) - c
    d = -c * torch.tan(sx) + a
    m0, m1, m3, m4 = d / s, -b / s, -c / s, a / s
    m2 = -(m0 * tx + m1 * ty)
    m5 = -(m3 * tx + m4 * ty)
    return (torch.stack([m0, m1, m2, m3, m4, m5], 1) + 0.0).to(torch.float32).contiguous()      # (+ 0.0: no negative zeros)


def affine_reference(img, mat, fill=0, rounded=True):
    """The definition in the module docstring in torch float64 on the CPU: img (B,1,H,W) or (B,H,W) of any real dtype, mat (B,6);
    returns the same shape, uint8 (`rounded`) or the float64 value before `floor(. + 0.5)`.  Used by the tests and by nothing else."""
    shape = img.shape
    H, W = shape[-2], shape[-1]
    x = img.reshape(-1, H, W).double()
    B = x.shape[0]
    m = mat.double().reshape(B, 6, 1, 1)
    xo = (torch.arange(W, dtype=torch.float64) + 0.5 - W / 2.0).view(1, 1, W)
    yo = (torch.arange(H, dtype=torch.float64) + 0.5 - H / 2.0).view(1, H, 1)
    u = m[:, 0] * xo + m[:, 1] * yo + m[:, 2] + W / 2.0 - 0.5
    v = m[:, 3] * xo + m[:, 4] * yo + m[:, 5] + H / 2.0 - 0.5
    u0, v0 = torch.floor(u), torch.floor(v)
    fu, fv = u - u0, v - v0
    bi = torch.arange(B).view(B, 1, 1).expand(B, H, W)

    def p(r, c):
        inside = (r >= 0) & (r < H) & (c >= 0) & (c < W)
        val = x[bi, r.clamp(0, H - 1).long(), c.clamp(0, W - 1).long()]
        return torch.where(inside, val, torch.full_like(val, float(fill)))

    top = p(v0, u0) * (1 - fu) + p(v0, u0 + 1) * fu
    bot = p(v0 + 1, u0) * (1 - fu) + p(v0 + 1, u0 + 1) * fu
    val = top * (1 - fv) + bot * fv
    if not rounded:
        return val.reshape(shape)
    return torch.floor(val + 0.5).clamp(0, 255).to(torch.uint8).reshape(shape)


class RandomAffine:
    """The --affine step of the training loop: warps a uint8 batch on the GPU with matrices drawn from (step, rank)."""

    def __init__(self, degrees, translate, scale, shear, rank, device, fill=0):
        self.ranges = {"degrees": float(degrees), "translate": float(translate), "scale": (float(scale[0]), float(scale[1])),
                       "shear": float(shear)}
        self.rank, self.device, self.fill = rank, device, fill

    def __call__(self, x_u8, step):
        from . import ops
        B, H, W = x_u8.shape[0], x_u8.shape[-2], x_u8.shape[-1]
        mat = affine_matrices(step_seed(step, self.rank), B, H, W, **self.ranges)
        return ops.u8_affine(x_u8, mat.to(self.device), self.fill)


def clahe_clip_count(clip_limit, th, tw):
    """The integer clip level per histogram bin of a th x tw tile for clip limit c (a multiple of the mean bin height area / 256, as
    OpenCV's clipLimit): 0 for c == 0 (no clipping), else min(area, max(1, floor(c * area / 256)))."""
    c, area = float(clip_limit), int(th) * int(tw)
    if not (c >= 0.0 and math.isfinite(c)):
        raise ValueError("the CLAHE clip limit is a finite number >= 0 (got %r)" % (clip_limit,))
    if c == 0.0:
        return 0
    return min(area, max(1, int(math.floor(c * area / 256.0))))


def check_clahe_grid(grid, H, W):
    """(GY, GX) as ints if the grid is one the kernels take for an H x W image, else ValueError with the reason."""
    if len(grid) != 2:
        raise ValueError("the CLAHE grid is two numbers GY GX (got %r)" % (grid,))
    GY, GX = int(grid[0]), int(grid[1])
    if not (1 <= GY <= 16 and 1 <= GX <= 16):
        raise ValueError("the CLAHE grid takes 1..16 tiles per axis (got %d x %d)" % (GY, GX))
    if H % GY or W % GX:
        raise ValueError("the CLAHE grid %d x %d does not divide the %d x %d image" % (GY, GX, H, W))
    if W % 4 or H > 1024 or W > 1024:
        raise ValueError("CLAHE takes images up to 1024 x 1024 whose width is a multiple of 4 (got %d x %d)" % (H, W))
    return GY, GX


def clahe_tables_reference(img, grid, clip_count):
    """The tables of the definition in the module docstring in numpy integers on the CPU, and the redistribution residual r of
    every tile: (lut (B, GY, GX, 256) uint8, r (B, GY, GX) int64; r = 0 where nothing is clipped)."""
    import numpy as np
    x = np.asarray(img.cpu() if isinstance(img, torch.Tensor) else img)
    H, W = x.shape[-2], x.shape[-1]
    GY, GX = check_clahe_grid(grid, H, W)
    x = x.reshape(-1, H, W)
    B, th, tw = x.shape[0], H // GY, W // GX
    area, L = th * tw, int(clip_count)
    if not 0 <= L <= area:
        raise ValueError("clip count %d outside [0, %d]" % (L, area))
    tiles = x.reshape(B, GY, th, GX, tw).transpose(0, 1, 3, 2, 4).reshape(B * GY * GX, area)
    lut = np.empty((B * GY * GX, 256), np.uint8)
    res = np.zeros(B * GY * GX, np.int64)
    for n, tile in enumerate(tiles):
        hist = np.bincount(tile, minlength=256).astype(np.int64)
        if L > 0:
            excess = int(np.maximum(hist - L, 0).sum())
            hist = np.minimum(hist, L)
            q, r = divmod(excess, 256)
            hist += q
            res[n] = r
            if r > 0:
                step = max(1, 256 // r)
                for v in range(0, 256, step):
                    if r == 0:
                        break
                    hist[v] += 1
                    r -= 1
        lut[n] = (np.cumsum(hist) * 255 + area // 2) // area
    return torch.from_numpy(lut.reshape(B, GY, GX, 256)), torch.from_numpy(res.reshape(B, GY, GX))


def clahe_apply_reference(img, lut):
    """The interpolation of the definition in the module docstring in numpy integers on the CPU: img uint8 (B,1,H,W) / (B,H,W),
    lut (B, GY, GX, 256) uint8; returns img's shape, uint8."""
    import numpy as np
    x = np.asarray(img.cpu() if isinstance(img, torch.Tensor) else img)
    t = np.asarray(lut.cpu() if isinstance(lut, torch.Tensor) else lut).astype(np.int64)
    shape, H, W = x.shape, x.shape[-2], x.shape[-1]
    x = x.reshape(-1, H, W)
    B, GY, GX = t.shape[0], t.shape[1], t.shape[2]
    th, tw = H // GY, W // GX

    def axis(n, t_, G):
        a = 2 * np.arange(n, dtype=np.int64) + 1 - t_
        g0 = a // (2 * t_)                                   # floor division: -1 in the first half tile
        w = a - g0 * 2 * t_
        return np.clip(g0, 0, G - 1), np.clip(g0 + 1, 0, G - 1), w

    gy0, gy1, wy = (v.reshape(1, H, 1) for v in axis(H, th, GY))
    gx0, gx1, wx = (v.reshape(1, 1, W) for v in axis(W, tw, GX))
    b = np.arange(B).reshape(B, 1, 1)
    v = x.astype(np.int64)
    num = (2 * th - wy) * ((2 * tw - wx) * t[b, gy0, gx0, v] + wx * t[b, gy0, gx1, v]) \
        + wy * ((2 * tw - wx) * t[b, gy1, gx0, v] + wx * t[b, gy1, gx1, v])
    assert int(num.max()) < 2 ** 31
    return torch.from_numpy(((num + 2 * th * tw) // (4 * th * tw)).astype(np.uint8).reshape(shape))


def clahe_reference(img, grid=(8, 8), clip_limit=2.0, return_lut=False):
    """The definition in the module docstring in numpy integers on the CPU: img uint8 (B,1,H,W) / (B,H,W); returns the same shape,
    uint8, and with `return_lut` the (B, GY, GX, 256) uint8 tables too.  Like OpenCV's createCLAHE in structure, not bit-equal to it
    (integer rounding, tile-centre / pixel-centre anchoring).  Used by the tests and by nothing else."""
    H, W = img.shape[-2], img.shape[-1]
    GY, GX = check_clahe_grid(grid, H, W)
    lut, _ = clahe_tables_reference(img, (GY, GX), clahe_clip_count(clip_limit, H // GY, W // GX))
    out = clahe_apply_reference(img, lut)
    return (out, lut) if return_lut else out


class Clahe:
    """The --clahe step: equalises a uint8 batch on the GPU (ops.u8_clahe: two launches).  No random draw: every mode runs it."""

    def __init__(self, grid=(8, 8), clip_limit=2.0):
        self.grid, self.clip_limit = (int(grid[0]), int(grid[1])), float(clip_limit)
        clahe_clip_count(self.clip_limit, 1, 1)              # (validates the limit)

    def __call__(self, x_u8, out=None):
        from . import ops
        if x_u8.dtype != torch.uint8:
            raise RuntimeError("CLAHE equalises the decoded uint8 images (got %s)" % x_u8.dtype)
        return ops.u8_clahe(x_u8, self.grid, self.clip_limit, out)


# ---- sample mixing: Mixup, CutMix, random erasing ----------------------------------------------------------------------------------
MIX_ONE = 65536              # lambda = 1 in the 16-bit fixed point of lam_q / tw_q
ERASE_FILL = 136             # the dataset mean 0.5330 in grey levels


def _identity_plan(B):
    import numpy as np
    return {"perm": np.arange(B, dtype=np.int32), "lam_q": np.full(B, MIX_ONE, np.int32), "box": np.zeros((B, 4), np.int32),
            "tw_q": np.full(B, MIX_ONE, np.int32)}


def mix_plan(seed, B, H, W, mixup_alpha=0.0, cutmix_alpha=0.0, prob=1.0, switch_prob=0.5, mode="batch"):
    """The Mixup / CutMix plan of one minibatch as int32 numpy arrays {perm (B,), lam_q (B,), box (B,4), tw_q (B,)}, with the
    semantics of timm's `Mixup`: with probability 1 - prob nothing is mixed; with both alphas > 0 CutMix is chosen with probability
    switch_prob; mode "batch" draws once for the minibatch, "elem" once per row.  A pure function of its arguments:
      perm     argsort (stable) of synth.uniform(seed, (B,)); fixed points are allowed (a row mixed with itself is unchanged)
      lambda   Beta(alpha, alpha) from numpy.random.RandomState(seed mod 2^32) (the legacy stream, which NumPy keeps frozen): n draws
               at mixup_alpha where it is > 0, then n at cutmix_alpha where it is > 0 (n = 1 or B)
      u        counters B .. B + 4n - 1 of the same synth.uniform stream, in [0, 1): rows `apply`, `switch`, `cy`, `cx`
      a draw is mixed where u_apply < prob, and is a CutMix where only cutmix_alpha > 0, or both are and u_switch < switch_prob
      Mixup    lam_q = tw_q = floor(65536 lambda + 0.5), box = the image
      CutMix   timm's rand_bbox: r = sqrt(1 - lambda), cut = int(H r) x int(W r) about the centre (int(u_cy H), int(u_cx W)), clipped
               to the image; lam_q = 0; tw_q = ((HW - area) * 131072 + HW) // (2 HW), the share of the row's own pixels rounded half
               up to 16 bits
    B = 0, both alphas 0, prob = 0, or no draw that is mixed give the identity plan (perm = 0..B-1, lam_q = tw_q = 65536, empty boxes)."""
    import numpy as np
    B, H, W = int(B), int(H), int(W)
    ma, ca = float(mixup_alpha), float(cutmix_alpha)
    if mode not in ("batch", "elem"):
        raise ValueError("mix_plan: mode is batch or elem (got %r)" % (mode,))
    if ma < 0 or ca < 0 or not (0.0 <= float(prob) <= 1.0 and 0.0 <= float(switch_prob) <= 1.0):
        raise ValueError("mix_plan: alphas >= 0 and probabilities in [0, 1] (got %r, %r, %r, %r)" % (mixup_alpha, cutmix_alpha, prob, switch_prob))
    plan = _identity_plan(B)
    if B == 0 or (ma == 0 and ca == 0):
        return plan
    n = 1 if mode == "batch" else B
    plan["perm"] = np.argsort(synth.uniform(seed, (B,)).numpy(), kind="stable").astype(np.int32)
    rs = np.random.RandomState(int(seed) % (1 << 32))
    lam_mix = rs.beta(ma, ma, n) if ma > 0 else np.ones(n)
    lam_cut = rs.beta(ca, ca, n) if ca > 0 else np.ones(n)
    u = synth.uniform(seed, (B + 4 * n,), 0.0, 1.0, dtype=torch.float64).numpy()[B:].reshape(4, n)
    apply = u[0] < float(prob)
    if not apply.any():
        return _identity_plan(B)
    cut = np.full(n, ma == 0) if (ma == 0 or ca == 0) else u[1] < float(switch_prob)
    lam_q = np.full(n, MIX_ONE, np.int64)
    tw_q = np.full(n, MIX_ONE, np.int64)
    box = np.zeros((n, 4), np.int64)
    for k in range(n):
        if not apply[k]:
            continue
        if cut[k]:
            r = math.sqrt(max(0.0, 1.0 - float(lam_cut[k])))
            ch, cw = int(H * r), int(W * r)
            cy, cx = int(u[2, k] * H), int(u[3, k] * W)
            y0, y1 = min(max(cy - ch // 2, 0), H), min(max(cy + ch // 2, 0), H)
            x0, x1 = min(max(cx - cw // 2, 0), W), min(max(cx + cw // 2, 0), W)
            area = (y1 - y0) * (x1 - x0)
            box[k] = (y0, y1, x0, x1)
            lam_q[k] = 0
            tw_q[k] = ((H * W - area) * 131072 + H * W) // (2 * H * W)
        else:
            lam_q[k] = tw_q[k] = min(max(int(math.floor(65536.0 * float(lam_mix[k]) + 0.5)), 0), MIX_ONE)
            box[k] = (0, H, 0, W)
    rows = np.zeros(B, np.int64) if n == 1 else np.arange(B)
    plan["lam_q"], plan["tw_q"], plan["box"] = lam_q[rows].astype(np.int32), tw_q[rows].astype(np.int32), box[rows].astype(np.int32)
    return plan


def erase_plan(seed, B, H, W, prob=0.25, area=(0.02, 1.0 / 3.0), aspect=(0.3, 3.3), attempts=10):
    """The random-erasing plan of one minibatch (same arrays as mix_plan), drawn as torchvision's `RandomErasing.get_params`: a row
    is erased where u < prob; then up to `attempts` tries of an area fraction uniform in `area` and an aspect ratio log-uniform in
    `aspect`, h = int(round(sqrt(A r))), w = int(round(sqrt(A / r))) with A the fraction times H W; the first try with h < H and
    w < W is taken, top uniform in [0, H - h], left uniform in [0, W - w] (none fits: the row stays).  The numbers are
    synth.uniform(seed, (B, 1 + 4 * attempts)) in [0, 1).  Erased rows get perm = -1 (the kernel writes `fill`) and their box; the
    others keep perm = b and an empty box; lam_q = 0 and tw_q = 65536 everywhere: labels do not change."""
    import numpy as np
    B, H, W, attempts = int(B), int(H), int(W), int(attempts)
    if not 0.0 <= float(prob) <= 1.0:
        raise ValueError("erase_plan: prob in [0, 1] (got %r)" % (prob,))
    plan = _identity_plan(B)
    plan["lam_q"][:] = 0
    if B == 0 or float(prob) == 0.0:
        return plan
    u = synth.uniform(seed, (B, 1 + 4 * attempts), 0.0, 1.0, dtype=torch.float64).numpy()
    la0, la1 = math.log(float(aspect[0])), math.log(float(aspect[1]))
    for b in range(B):
        if not u[b, 0] < float(prob):
            continue
        for k in range(attempts):
            ua, ur, ut, ul = u[b, 1 + 4 * k:5 + 4 * k]
            A = H * W * (float(area[0]) + ua * (float(area[1]) - float(area[0])))
            r = math.exp(la0 + ur * (la1 - la0))
            h, w = int(round(math.sqrt(A * r))), int(round(math.sqrt(A / r)))
            if not (h < H and w < W):
                continue
            top, left = int(ut * (H - h + 1)), int(ul * (W - w + 1))
            plan["perm"][b] = -1
            plan["box"][b] = (top, top + h, left, left + w)
            break
    return plan


def _np(v):
    import numpy as np
    return np.asarray(v.cpu() if isinstance(v, torch.Tensor) else v)


def mix_reference(x, perm, lam_q, box, fill=0):
    """cx_u8_mix's definition (module docstring) in numpy int64 on the CPU, clamps included: x uint8 (B,1,H,W) / (B,H,W); returns the
    same shape, uint8 (a torch tensor).  Used by the tests and by nothing else."""
    import numpy as np
    xs = _np(x)
    shape, H, W = xs.shape, xs.shape[-2], xs.shape[-1]
    a = xs.reshape(-1, H, W).astype(np.int64)
    B = a.shape[0]
    p = np.clip(_np(perm).astype(np.int64).reshape(B), -1, B - 1)
    q = np.clip(_np(lam_q).astype(np.int64).reshape(B), 0, MIX_ONE).reshape(B, 1, 1)
    bx = _np(box).astype(np.int64).reshape(B, 4)
    y0, y1 = np.clip(bx[:, 0], 0, H).reshape(B, 1, 1), np.clip(bx[:, 1], 0, H).reshape(B, 1, 1)
    x0, x1 = np.clip(bx[:, 2], 0, W).reshape(B, 1, 1), np.clip(bx[:, 3], 0, W).reshape(B, 1, 1)
    i, j = np.arange(H).reshape(1, H, 1), np.arange(W).reshape(1, 1, W)
    inside = (i >= y0) & (i < y1) & (j >= x0) & (j < x1)
    o = np.where((p < 0).reshape(B, 1, 1), np.int64(fill), a[np.maximum(p, 0)])
    m = (q * a + (MIX_ONE - q) * o + 32768) >> 16
    return torch.from_numpy(np.where(inside, m, a).astype(np.uint8).reshape(shape))


def target_mix_reference(t, perm, tw_q):
    """cx_target_mix's definition (module docstring) in numpy float32 on the CPU, every product and sum rounded on its own: t (B, n);
    returns (B, n) float32 (a torch tensor).  Used by the tests and by nothing else."""
    import numpy as np
    tt = _np(t).astype(np.float32)
    B = tt.shape[0]
    p = np.clip(_np(perm).astype(np.int64).reshape(B), -1, B - 1)
    wq = np.clip(_np(tw_q).astype(np.int64).reshape(B), 0, MIX_ONE)
    w = (wq.astype(np.float32) * np.float32(2.0 ** -16)).reshape(B, 1)
    oth = tt[np.maximum(p, 0)]
    blend = (w * tt).astype(np.float32) + ((np.float32(1.0) - w) * oth).astype(np.float32)
    out = np.where((tt < 0) | (oth < 0), np.float32(-1.0), blend.astype(np.float32))
    keep = ((p < 0) | (wq == MIX_ONE)).reshape(B, 1)
    return torch.from_numpy(np.where(keep, tt, out).astype(np.float32))


def _plan_to(plan, device):
    """A plan's four arrays on `device` through ONE copy: int32 views (perm, lam_q, tw_q, box) of a (7 B,) buffer."""
    import numpy as np
    B = len(plan["perm"])
    flat = np.concatenate([plan["perm"], plan["lam_q"], plan["tw_q"], plan["box"].reshape(-1)]).astype(np.int32)
    d = torch.from_numpy(flat).to(device)
    return d[:B], d[B:2 * B], d[2 * B:3 * B], d[3 * B:].view(B, 4)


class SampleMix:
    """The --mixup / --cutmix / --erase_prob step of the training loop, the last one on the uint8 batch: (x_u8, t, step) -> (x, t)
    on the GPU, its plans drawn from (step, rank).  Mixing is ops.u8_mix + ops.target_mix; erasing a second ops.u8_mix (labels do not
    change).  Build it with `make_sample_mix`, which returns None when everything is off."""

    def __init__(self, mixup_alpha=0.0, cutmix_alpha=0.0, prob=1.0, switch_prob=0.5, mode="batch", erase_prob=0.0, erase_fill=ERASE_FILL,
                 rank=0, device=None):
        self.mix = {"mixup_alpha": float(mixup_alpha), "cutmix_alpha": float(cutmix_alpha), "prob": float(prob),
                    "switch_prob": float(switch_prob), "mode": mode}
        self.mixing = (self.mix["mixup_alpha"] > 0 or self.mix["cutmix_alpha"] > 0) and self.mix["prob"] > 0
        self.erase_prob, self.erase_fill = float(erase_prob), int(erase_fill)
        self.rank, self.device = rank, device
        mix_plan(0, 0, 1, 1, **self.mix)                     # (validates the settings)
        erase_plan(0, 0, 1, 1, prob=self.erase_prob)
        if not 0 <= self.erase_fill <= 255:
            raise ValueError("the erase fill is a grey level 0..255 (got %r)" % (erase_fill,))

    def __call__(self, x_u8, t, step):
        from . import ops
        if x_u8.dtype != torch.uint8:
            raise RuntimeError("the sample mix works on the decoded uint8 images (got %s)" % x_u8.dtype)
        B, H, W = x_u8.shape[0], x_u8.shape[-2], x_u8.shape[-1]
        device = x_u8.device if self.device is None else self.device
        if self.mixing:
            perm, lam_q, tw_q, box = _plan_to(mix_plan(mix_seed(step, self.rank), B, H, W, **self.mix), device)
            x_u8 = ops.u8_mix(x_u8, perm, lam_q, box, 0)
            t = ops.target_mix(t, perm, tw_q)
        if self.erase_prob > 0:
            perm, lam_q, _, box = _plan_to(erase_plan(erase_seed(step, self.rank), B, H, W, prob=self.erase_prob), device)
            x_u8 = ops.u8_mix(x_u8, perm, lam_q, box, self.erase_fill)
        return x_u8, t


def make_sample_mix(mixup_alpha=0.0, cutmix_alpha=0.0, prob=1.0, switch_prob=0.5, mode="batch", erase_prob=0.0, erase_fill=ERASE_FILL,
                    rank=0, device=None):
    """A SampleMix, or None with everything off (no alpha > 0 or mix probability 0, and erase probability 0): then nothing is
    launched or allocated."""
    sm = SampleMix(mixup_alpha, cutmix_alpha, prob, switch_prob, mode, erase_prob, erase_fill, rank, device)
    return sm if (sm.mixing or sm.erase_prob > 0) else None


# ------------------------------------------------------------------------------------------------ two views (contrastive pretraining)
def duplicate_views(x_u8):
    """[x; x]: the uint8 minibatch twice, rows i and i + B the same image, ahead of the per-row random steps (RandomAffine, the
    jitter), which draw parameters for each of the 2B rows."""
    return torch.cat([x_u8, x_u8])


def contrastive_ids(rows, groups=None):
    """The (2B, 1) fp32 ids of the contrastive loss for the duplicated minibatch of duplicate_views.  rows: the B dataset indices of
    the minibatch.  groups None (--positive view): the row's position 0 .. B - 1, so the two views of an image are each other's only
    positive.  groups: one integer per value `rows` can take (the index of the image's study or patient, indexed the way `rows` counts: the
    loader's row labels, or positions): the id is that of the image's group, so other
    images of the group in the minibatch are positives too (MedAug).  Ids must be exact in fp32: below 2^24."""
    rows = torch.as_tensor(rows, dtype=torch.int64).reshape(-1)
    if groups is None:
        ids = torch.arange(rows.numel(), dtype=torch.int64)
    else:
        ids = torch.as_tensor(groups, dtype=torch.int64)[rows]
        if ids.numel() and (int(ids.min()) < 0 or int(ids.max()) >= 1 << 24):
            raise ValueError("contrastive_ids takes group indices in [0, 2^24) (got %d .. %d)" % (int(ids.min()), int(ids.max())))
    return torch.cat([ids, ids]).to(torch.float32).reshape(-1, 1)
