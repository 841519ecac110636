"""CPU (no GPU): the host side of the random-affine augmentation -- the parameter draw of chexpert_amd/augment.py, the float64
statement of cx_u8_affine's definition against torch's grid_sample, and the command-line wiring."""
import math

import torch
import torch.nn.functional as F

from chexpert_amd import augment, synth


def _recover(mat, H, W):
    """(angle, scale, shear, tx, ty) in degrees / pixels from (B,6) inverse maps (inverse of augment.affine_matrices)."""
    m = mat.double()
    a00, a01, m2, a10, a11, m5 = m.unbind(1)
    scale = 1.0 / torch.sqrt(a00 * a11 - a01 * a10)               # rotation . shear has determinant 1
    angle = torch.atan2(-a10, a11)                                # inverse = [[d, -b], [-c, a]] / s with a = cos, c = sin
    shear = torch.atan((a01 + a10) / a11)                         # b = -a tan(sx) - c
    inv = torch.stack([a00, a01, a10, a11], 1).view(-1, 2, 2)
    t = -torch.linalg.solve(inv, torch.stack([m2, m5], 1).unsqueeze(2)).squeeze(2)
    return torch.rad2deg(angle), scale, torch.rad2deg(shear), t[:, 0], t[:, 1]


def test_affine_matrices_deterministic_rank_dependent_and_inside_the_ranges():
    B, H, W = 64, 320, 384
    kw = dict(degrees=15.0, translate=0.05, scale=(0.9, 1.1), shear=5.0)
    a = augment.affine_matrices(augment.step_seed(3, 0), B, H, W, **kw)
    assert a.dtype == torch.float32 and tuple(a.shape) == (B, 6) and a.is_contiguous()
    assert torch.equal(a, augment.affine_matrices(augment.step_seed(3, 0), B, H, W, **kw))
    assert not torch.equal(a, augment.affine_matrices(augment.step_seed(3, 1), B, H, W, **kw))       # another rank
    assert not torch.equal(a, augment.affine_matrices(augment.step_seed(4, 0), B, H, W, **kw))       # another step
    assert augment.step_seed(3, 0) != 3 * 7919 + 13                  # not the jitter's numbers of the same step
    angle, scale, shear, tx, ty = _recover(a, H, W)
    eps = 1e-4                                                       # the matrices are rounded to fp32
    assert angle.abs().max() <= 15 + eps and angle.abs().max() > 7 and angle.min() < 0 < angle.max()
    assert scale.min() >= 0.9 - eps and scale.max() <= 1.1 + eps and scale.max() - scale.min() > 0.1
    assert shear.abs().max() <= 5 + eps and shear.abs().max() > 2
    assert tx.abs().max() <= 0.05 * W + 1e-3 and ty.abs().max() <= 0.05 * H + 1e-3 and tx.abs().max() > 0.02 * W
    # the defaults are the command line's
    d = augment.affine_matrices(5, B, H, W)
    angle, scale, shear, tx, ty = _recover(d, H, W)
    assert angle.abs().max() <= 10 + eps and shear.abs().max() <= eps and scale.min() >= 0.9 - eps and scale.max() <= 1.1 + eps


def test_zero_ranges_give_the_identity_exactly():
    m = augment.affine_matrices(11, 7, 320, 320, degrees=0, translate=0, scale=(1, 1), shear=0)
    assert torch.equal(m, torch.tensor([1.0, 0, 0, 0, 1, 0]).repeat(7, 1))
    assert not torch.signbit(m).any()


def _smooth(H, W):
    """A smooth float image that falls to ~0 at its border (so that the step to the zero padding is small too): gradient
    <= 4 grey levels per pixel, which the test checks."""
    i = torch.arange(H, dtype=torch.float64).view(H, 1)
    j = torch.arange(W, dtype=torch.float64).view(1, W)
    base = min(190.0, 1.8 * min(H, W) / math.pi)
    win = torch.sin(math.pi * (i + 0.5) / H) * torch.sin(math.pi * (j + 0.5) / W)
    return win * base * (0.8 + 0.2 * torch.sin(2 * math.pi * j / 128) * torch.cos(2 * math.pi * i / 160))


def _theta(mat, H, W):
    """The normalised theta of F.affine_grid(align_corners=False) equivalent to pixel-unit, centre-relative inverse maps:
    x_n = 2 xo / W, y_n = 2 yo / H and u = xs_n W / 2 + W/2 - 0.5."""
    m = mat.double()
    return torch.stack([m[:, 0], m[:, 1] * H / W, m[:, 2] * 2 / W, m[:, 3] * W / H, m[:, 4], m[:, 5] * 2 / H], 1).view(-1, 2, 3)


def test_affine_reference_matches_grid_sample_on_a_smooth_image():
    """Pins the convention (pixel centres, centre-relative, inverse map) to torch's bilinear grid_sample with zero padding and
    align_corners=False.  Both sides are exact bilinear forms; grid_sample in fp32 carries a coordinate error of the order
    160 * 2^-24 px, times a gradient <= 4 levels / px: ~4e-5 levels.  The bound 1e-3 leaves room.  In float64 the same
    comparison agrees to 1e-9."""
    for H, W in ((320, 320), (96, 128), (320, 384)):
        B = 6
        img = _smooth(H, W)
        pad = F.pad(img, (1, 1, 1, 1))
        grad = max((pad[:, 1:] - pad[:, :-1]).abs().max().item(), (pad[1:] - pad[:-1]).abs().max().item())
        assert grad <= 4.0, grad                                       # the premise of the bound
        x = img.expand(B, 1, H, W).contiguous()
        mat = augment.affine_matrices(70 + H, B, H, W, degrees=15.0, translate=0.05, scale=(0.9, 1.1), shear=5.0)
        got = augment.affine_reference(x, mat, fill=0, rounded=False)
        assert got.dtype == torch.float64 and got.shape == x.shape
        th = _theta(mat, H, W)
        want64 = F.grid_sample(x, F.affine_grid(th, (B, 1, H, W), align_corners=False), mode="bilinear", padding_mode="zeros",
                               align_corners=False)
        assert (got - want64).abs().max().item() <= 1e-9
        want32 = F.grid_sample(x.float(), F.affine_grid(th.float(), (B, 1, H, W), align_corners=False), mode="bilinear",
                               padding_mode="zeros", align_corners=False)
        err = (got - want32.double()).abs().max().item()
        print("affine_reference vs grid_sample fp32 at %dx%d: max abs diff %.3e, gradient %.2f" % (H, W, err, grad))
        assert err <= 1e-3, err
        assert (got - x).abs().max().item() > 5                        # the image did move


def test_affine_reference_identity_translation_rotation_direction():
    u8 = synth.xray_u8(91, 3, 32)
    B = u8.shape[0]
    ident = torch.tensor([1.0, 0, 0, 0, 1, 0]).repeat(B, 1)
    assert torch.equal(augment.affine_reference(u8, ident, 0), u8)
    assert torch.equal(augment.affine_reference(u8[:, 0], ident, 7), u8[:, 0])             # (B,H,W) form
    # inverse map (1,0,tx, 0,1,ty): output (i, j) reads source (i + ty, j + tx)
    tx, ty = 3, -5
    got = augment.affine_reference(u8, torch.tensor([1.0, 0, tx, 0, 1, ty]).repeat(B, 1), 128)
    want = torch.full_like(u8, 128)
    want[:, :, 5:, :32 - 3] = u8[:, :, :32 - 5, 3:]
    assert torch.equal(got, want)
    # (0,-1,0, 1,0,0): u = S-1-i, v = j, i.e. y[i][j] = x[j][S-1-i] = torch.rot90(x, k=1) (counter-clockwise); pinned here and in
    # tests/test_augment_gpu.py
    rot = augment.affine_reference(u8, torch.tensor([0.0, -1, 0, 1, 0, 0]).repeat(B, 1), 0)
    assert torch.equal(rot, torch.rot90(u8, 1, (-2, -1))) and not torch.equal(rot, torch.rot90(u8, -1, (-2, -1)))
    # half-way between two pixels: the mean, rounded half up
    half = augment.affine_reference(u8, torch.tensor([1.0, 0, 0.5, 0, 1, 0]).repeat(B, 1), 0)
    nxt = torch.cat([u8[..., 1:], torch.zeros_like(u8[..., :1])], -1)
    assert torch.equal(half, ((u8.int() + nxt.int() + 1) // 2).to(torch.uint8))


def test_cli_flags_and_affine_only_when_training():
    from chexpert_amd import cli
    a = cli.build_parser().parse_args([])
    assert (a.affine, a.affine_degrees, a.affine_translate, a.affine_scale, a.affine_shear) == (False, 10.0, 0.05, [0.9, 1.1], 0.0)
    assert (a.affine_degrees, a.affine_translate, tuple(a.affine_scale), a.affine_shear) == \
        tuple(augment.TRAIN_DEFAULTS[k] if k != "scale" else tuple(augment.TRAIN_DEFAULTS[k]) for k in ("degrees", "translate", "scale", "shear"))
    a = cli.build_parser().parse_args(["--train", "--affine", "--affine_degrees", "7", "--affine_translate", "0.1", "--affine_scale", "0.8", "1.2",
                                       "--affine_shear", "3"])
    aug = cli.make_affine(a, 1, torch.device("cpu"))
    assert isinstance(aug, augment.RandomAffine) and aug.rank == 1
    assert aug.ranges == {"degrees": 7.0, "translate": 0.1, "scale": (0.8, 1.2), "shear": 3.0}
    # without --train no augmentation object exists: validation / --evaluate / --visualize never warp
    for argv in (["--affine"], ["--affine", "--evaluate"], ["--affine", "--visualize"], ["--train"], []):
        assert cli.make_affine(cli.build_parser().parse_args(argv), 0, torch.device("cpu")) is None
    # half the training ranges for test-time augmentation, as predict's docstring states
    assert augment.TTA_RANGES == {"degrees": 5.0, "translate": 0.025, "scale": (0.95, 1.05), "shear": 0.0}
    from chexpert_amd import predict
    p = predict.build_parser().parse_args(["a.csv", "b.csv", "--restore_path", "x"])
    assert (p.tta, p.tta_seed) == (1, 0)
    assert predict.build_parser().parse_args(["a.csv", "b.csv", "--restore_path", "x", "--tta", "4"]).tta == 4
    assert augment.tta_seed_of(0, 1, 0) != augment.tta_seed_of(0, 2, 0) != augment.tta_seed_of(0, 1, 1) != augment.tta_seed_of(1, 1, 0)


def test_affine_entry_point_validates_without_launching():
    """cx_u8_affine checks its arguments before any launch (no GPU needed): null pointers, W % 4, sizes above 1024."""
    from chexpert_amd import _lib
    f = _lib.lib().cx_u8_affine
    assert f(None, None, 1, 8, 8, None, 0, None) == -1                  # CX_EINVAL
    buf = torch.zeros(4096, dtype=torch.uint8)
    out = torch.zeros(4096, dtype=torch.uint8)
    mat = torch.zeros(6)
    assert f(buf.data_ptr(), out.data_ptr(), 1, 8, 6, mat.data_ptr(), 0, None) == -3          # CX_ESHAPE: W % 4
    assert f(buf.data_ptr(), out.data_ptr(), 1, 8, 1028, mat.data_ptr(), 0, None) == -3
    assert f(buf.data_ptr(), out.data_ptr(), 1, 1025, 8, mat.data_ptr(), 0, None) == -3
    assert f(buf.data_ptr(), buf.data_ptr(), 1, 8, 8, mat.data_ptr(), 0, None) == -1          # in place is not supported
    assert f(buf.data_ptr(), out.data_ptr(), 1, 8, 8, mat.data_ptr(), 256, None) == -1
