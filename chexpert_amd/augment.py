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
