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
