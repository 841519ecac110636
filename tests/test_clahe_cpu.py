"""CPU (no GPU): the integer definition of the CLAHE step (chexpert_amd.augment.clahe_reference, the statement the kernels of
chexpert_amd/csrc/clahe.hip are held to in tests/test_clahe_gpu.py) pinned by properties that can be written down by hand, the
argument checks of the two entry points, and the command-line wiring.  Inputs are structured (ramps, blobs, constant tiles):
white noise has flat tile histograms and exercises neither the clip nor the tables."""
import json

import numpy as np
import pytest
import torch

from chexpert_amd import augment


def _ramp(H, W, lo=100, hi=140):
    """Low-contrast horizontal ramp confined to lo..hi."""
    return np.broadcast_to((lo + (np.arange(W) * (hi - lo + 1)) // W).astype(np.uint8), (H, W)).copy()


def _blobs(H, W, seed=3):
    """The ramp plus Gaussian blobs."""
    rng = np.random.default_rng(seed)
    i, j = np.mgrid[0:H, 0:W].astype(np.float64)
    img = _ramp(H, W, 60, 120).astype(np.float64)
    for _ in range(5):
        ci, cj, s, a = rng.uniform(0, H), rng.uniform(0, W), rng.uniform(2, max(H, W) / 4), rng.uniform(40, 130)
        img += a * np.exp(-((i - ci) ** 2 + (j - cj) ** 2) / (2 * s * s))
    return np.clip(img, 0, 255).astype(np.uint8)


def _batch(H, W):
    rng = np.random.default_rng(H * 1000 + W)
    return np.stack([_ramp(H, W), _blobs(H, W), rng.integers(0, 256, (H, W), dtype=np.uint8)])


def _clipped_hist(tile, L):
    """The histogram after clip and redistribute, restated from the definition."""
    hist = np.bincount(tile.ravel(), minlength=256).astype(np.int64)
    if L > 0:
        excess = int(np.maximum(hist - L, 0).sum())
        hist = np.minimum(hist, L)
        q, r = divmod(excess, 256)
        hist += q
        if r > 0:
            step = max(1, 256 // r)
            for v in range(0, 256, step):
                if r == 0:
                    break
                hist[v] += 1
                r -= 1
    return hist


def test_global_equalisation_matches_a_hand_written_cdf():
    x = _batch(48, 64)
    got, lut = augment.clahe_reference(torch.from_numpy(x), (1, 1), 0.0, return_lut=True)
    assert got.dtype == torch.uint8 and tuple(got.shape) == x.shape and tuple(lut.shape) == (3, 1, 1, 256)
    for b in range(len(x)):
        cdf = np.cumsum(np.bincount(x[b].ravel(), minlength=256))
        table = (cdf * 255 + x[b].size // 2) // x[b].size
        assert np.array_equal(lut[b, 0, 0].numpy(), table)
        assert np.array_equal(got[b].numpy(), table[x[b]])
    # the (B,1,H,W) form
    assert torch.equal(augment.clahe_reference(torch.from_numpy(x[:, None]), (1, 1), 0.0)[:, 0], got)
    assert (got[0].numpy() != x[0]).mean() > 0.5 and got[0].max() == 255      # the low-contrast ramp is stretched to the full range


def test_large_clip_limit_equals_no_clipping():
    x = torch.from_numpy(_batch(32, 48))
    for grid in ((2, 3), (1, 1), (4, 4)):
        area = (32 // grid[0]) * (48 // grid[1])
        assert augment.clahe_clip_count(256.0, 32 // grid[0], 48 // grid[1]) == area       # L >= area: nothing to clip
        o0, l0 = augment.clahe_reference(x, grid, 0.0, return_lut=True)
        o1, l1 = augment.clahe_reference(x, grid, 256.0, return_lut=True)
        o2, l2 = augment.clahe_reference(x, grid, 1e6, return_lut=True)
        assert torch.equal(l0, l1) and torch.equal(l0, l2) and torch.equal(o0, o1) and torch.equal(o0, o2)
        assert not torch.equal(augment.clahe_reference(x, grid, 2.0, return_lut=True)[1], l0)


def test_clipped_histogram_keeps_its_mass_and_tables_are_monotone():
    x = _batch(48, 80)
    th, tw = 16, 16
    seen = set()
    for c in (0.01, 0.5, 2.0, 7.3, 40.0):
        L = augment.clahe_clip_count(c, th, tw)
        lut, res = augment.clahe_tables_reference(torch.from_numpy(x), (3, 5), L)
        lut = lut.numpy().astype(np.int64)
        assert (np.diff(lut, axis=-1) >= 0).all() and (lut[..., 255] == 255).all()
        for b in range(len(x)):
            for gy in range(3):
                for gx in range(5):
                    tile = x[b, gy * th:(gy + 1) * th, gx * tw:(gx + 1) * tw]
                    hist = _clipped_hist(tile, L)
                    assert hist.sum() == th * tw and hist.min() >= 0
                    assert np.array_equal(lut[b, gy, gx], (np.cumsum(hist) * 255 + th * tw // 2) // (th * tw))
                    excess = int(np.maximum(np.bincount(tile.ravel(), minlength=256) - L, 0).sum())
                    assert int(res[b, gy, gx]) == excess % 256
                    seen.add(0 if excess % 256 == 0 else 1 if excess % 256 <= 128 else 2)
    assert seen == {0, 1, 2}                                           # no residual, step >= 2, step == 1


def test_flat_tile_gives_the_rounded_ramp():
    rng = np.random.default_rng(5)
    for th, tw in ((16, 16), (16, 32), (32, 48)):
        area = th * tw
        assert area % 256 == 0
        tiles = [rng.permutation(np.repeat(np.arange(256), area // 256)).reshape(th, tw).astype(np.uint8) for _ in range(4)]
        x = np.block([[tiles[0], tiles[1]], [tiles[2], tiles[3]]])[None]
        want = ((np.arange(256) + 1) * area // 256 * 255 + area // 2) // area
        for c in (0.0, 1.0, 2.0):                                       # a flat histogram sits at area / 256 = the level c = 1 clips at
            lut = augment.clahe_reference(torch.from_numpy(x), (2, 2), c, return_lut=True)[1]
            assert (lut.numpy() == want).all()
        # four equal tables: the interpolation returns the table's value
        assert np.array_equal(augment.clahe_reference(torch.from_numpy(x), (2, 2), 0.0).numpy(), want[x].astype(np.uint8))


def test_constant_image_gives_a_single_value_derived_from_the_redistribution_rule():
    H, W = 48, 64
    for k in (0, 1, 77, 128, 254, 255):
        x = torch.full((2, H, W), k, dtype=torch.uint8)
        for grid in ((1, 1), (2, 2), (3, 4), (12, 16)):
            area = (H // grid[0]) * (W // grid[1])
            for c in (0.0, 0.01, 2.0, 40.0, 300.0):
                L = augment.clahe_clip_count(c, H // grid[0], W // grid[1])
                if L == 0 or L >= area:
                    cdf_k = area                                        # every pixel sits in bin k
                else:                                                   # bin k keeps L; area - L spread: q to every bin, +1 to bins 0, step, ...
                    q, r = divmod(area - L, 256)
                    extra = min(r, k // max(1, 256 // r) + 1) if r else 0
                    cdf_k = L + (k + 1) * q + extra
                want = (cdf_k * 255 + area // 2) // area
                got = augment.clahe_reference(x, grid, c)
                assert (got == want).all(), (k, grid, c, want, got.unique())


def test_mirrored_input_gives_mirrored_output():
    x = torch.from_numpy(_batch(48, 80))
    for grid in ((3, 5), (2, 2), (1, 4), (16, 16)):
        for c in (0.0, 2.0):
            y = augment.clahe_reference(x, grid, c)
            assert torch.equal(augment.clahe_reference(x.flip(-1), grid, c), y.flip(-1))
            assert torch.equal(augment.clahe_reference(x.flip(-2), grid, c), y.flip(-2))


def test_clip_count():
    assert augment.clahe_clip_count(0.0, 40, 40) == 0
    assert augment.clahe_clip_count(1e-9, 40, 40) == 1 and augment.clahe_clip_count(0.01, 16, 16) == 1
    assert augment.clahe_clip_count(2.0, 40, 40) == 12                  # floor(2 * 1600 / 256)
    assert augment.clahe_clip_count(2.0, 16, 16) == 2
    assert augment.clahe_clip_count(1e9, 40, 40) == 1600 and augment.clahe_clip_count(40.0, 4, 4) == 2
    for c in (1e-6, 0.3, 1.0, 5.0, 255.9, 256.0, 1e4):
        for th, tw in ((4, 4), (16, 32), (40, 40), (1024, 1024)):
            assert 1 <= augment.clahe_clip_count(c, th, tw) <= th * tw
    for bad in (-1.0, float("nan"), float("inf")):
        with pytest.raises(ValueError):
            augment.clahe_clip_count(bad, 8, 8)


def test_entry_points_validate_without_launching():
    """cx_u8_clahe_lut / cx_u8_clahe_apply check their arguments before any launch (no GPU needed), as cx_u8_affine does."""
    from chexpert_amd import _lib
    EINVAL, EALIGN, ESHAPE = -1, -2, -3
    lut_f, app_f = _lib.lib().cx_u8_clahe_lut, _lib.lib().cx_u8_clahe_apply
    x = torch.zeros(1 << 16, dtype=torch.uint8)
    y = torch.zeros(1 << 16, dtype=torch.uint8)
    t = torch.zeros(17 * 17 * 256 + 8, dtype=torch.uint8)
    X, Y, T = x.data_ptr(), y.data_ptr(), t.data_ptr()
    assert T % 4 == 0 and Y % 4 == 0
    assert lut_f(None, T, 1, 32, 32, 2, 2, 0, None) == EINVAL and lut_f(X, None, 1, 32, 32, 2, 2, 0, None) == EINVAL
    assert lut_f(X, T, 0, 32, 32, 2, 2, 0, None) == EINVAL
    assert lut_f(X, T, 1, 32, 32, 3, 2, 0, None) == ESHAPE              # H % GY
    assert lut_f(X, T, 1, 32, 32, 2, 5, 0, None) == ESHAPE              # W % GX
    assert lut_f(X, T, 1, 32, 30, 2, 2, 0, None) == ESHAPE              # W % 4
    assert lut_f(X, T, 1, 34, 34, 17, 17, 0, None) == ESHAPE            # a grid of 17
    assert lut_f(X, T, 1, 32, 32, 0, 2, 0, None) == ESHAPE
    assert lut_f(X, T, 1, 1028, 8, 1, 1, 0, None) == ESHAPE and lut_f(X, T, 1, 8, 1028, 1, 1, 0, None) == ESHAPE
    assert lut_f(X, T, 1, 32, 32, 2, 2, -1, None) == EINVAL             # clip count outside [0, area]
    assert lut_f(X, T, 1, 32, 32, 2, 2, 257, None) == EINVAL
    assert lut_f(X, T + 1, 1, 32, 32, 2, 2, 0, None) == EALIGN
    assert app_f(None, T, Y, 1, 32, 32, 2, 2, None) == EINVAL and app_f(X, None, Y, 1, 32, 32, 2, 2, None) == EINVAL
    assert app_f(X, T, None, 1, 32, 32, 2, 2, None) == EINVAL and app_f(X, T, Y, -1, 32, 32, 2, 2, None) == EINVAL
    assert app_f(X, T, X, 1, 32, 32, 2, 2, None) == EINVAL              # in place is not supported
    assert app_f(X, T, Y, 1, 32, 32, 3, 2, None) == ESHAPE and app_f(X, T, Y, 1, 32, 32, 2, 5, None) == ESHAPE
    assert app_f(X, T, Y, 1, 32, 30, 2, 2, None) == ESHAPE and app_f(X, T, Y, 1, 34, 68, 17, 17, None) == ESHAPE
    assert app_f(X, T, Y, 1, 1025, 8, 1, 1, None) == ESHAPE
    assert app_f(X, T, Y + 2, 1, 32, 32, 2, 2, None) == EALIGN and app_f(X, T + 1, Y, 1, 32, 32, 2, 2, None) == EALIGN
    # declared in the header with the parameters the binding passes, and built from its own source file
    import os
    import re
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(root, "include", "chexpert_hip.h")).read(), flags=re.S)
    for name, n in (("cx_u8_clahe_lut", 9), ("cx_u8_clahe_apply", 9)):
        m = re.search(r"\bint\s+%s\s*\(([^;{]*?)\)\s*;" % name, hdr, flags=re.S)
        assert m and len(_lib.SIGNATURES[name]) == m.group(1).count(",") + 1 == n
    assert "clahe.hip" in open(os.path.join(root, "chexpert_amd", "csrc", "Makefile")).read()
    assert _lib.lib().cx_abi_version() == 10                            # additive entry points


def test_reference_rejects_what_the_kernels_reject():
    x = torch.zeros(1, 32, 32, dtype=torch.uint8)
    for grid in ((3, 2), (2, 5), (17, 2), (0, 2)):
        with pytest.raises(ValueError):
            augment.clahe_reference(x, grid, 2.0)
    with pytest.raises(ValueError):
        augment.clahe_reference(torch.zeros(1, 32, 30, dtype=torch.uint8), (2, 2), 2.0)      # W % 4
    with pytest.raises(ValueError):
        augment.clahe_tables_reference(x, (2, 2), 257)


def test_command_line_flags_grid_check_and_config_round_trip(tmp_path):
    from chexpert_amd import cli, predict
    a = cli.parse_args([])
    assert (a.clahe, a.clahe_grid, a.clahe_clip) == (False, [8, 8], 2.0)
    assert cli.make_clahe(a) is None                                   # flag off: no object, nothing launched or allocated
    a = cli.parse_args(["--evaluate", "--clahe", "--clahe_grid", "4", "5", "--clahe_clip", "3.5", "--resize", "80"])
    step = cli.make_clahe(a)
    assert isinstance(step, augment.Clahe) and step.grid == (4, 5) and step.clip_limit == 3.5
    for argv in (["--train", "--clahe"], ["--visualize", "--clahe"], ["--evaluate_ensemble", "--clahe"], ["--clahe"]):
        assert isinstance(cli.make_clahe(cli.parse_args(argv)), augment.Clahe)         # preprocessing: every mode
    # a grid that does not divide the crop size (320 by default, else --resize) is an argument error
    for argv in (["--clahe", "--clahe_grid", "7", "8"], ["--clahe", "--resize", "100"], ["--clahe", "--clahe_grid", "17", "4"],
                 ["--clahe", "--clahe_grid", "0", "4"], ["--clahe", "--clahe_clip", "-1"], ["--clahe", "--resize", "90", "--clahe_grid", "5", "5"]):
        with pytest.raises(SystemExit):
            cli.parse_args(argv)
        with pytest.raises(SystemExit):
            predict.parse_args(["a.csv", "b.csv", "--restore_path", "x"] + argv)
    cli.parse_args(["--resize", "100"])                                 # without --clahe the default grid binds nothing
    # the run's saved config (main() dumps args.__dict__) restores the three values through --load_config
    path = tmp_path / "config.json"
    json.dump(a.__dict__, open(path, "w"), indent=4)
    b = cli.parse_args(["--load_config", str(path)])
    assert (b.clahe, list(b.clahe_grid), b.clahe_clip, b.resize) == (True, [4, 5], 3.5, 80)
    assert cli.make_clahe(b).grid == (4, 5)
    cfg = json.load(open(path))
    cfg["clahe_grid"] = [7, 8]
    json.dump(cfg, open(path, "w"))
    with pytest.raises(SystemExit):                                     # checked after the config is applied
        cli.parse_args(["--load_config", str(path)])
    p = predict.parse_args(["a.csv", "b.csv", "--restore_path", "x"])
    assert (p.clahe, p.clahe_grid, p.clahe_clip) == (False, [8, 8], 2.0)
    p = predict.parse_args(["a.csv", "b.csv", "--restore_path", "x", "--clahe", "--clahe_grid", "4", "4", "--clahe_clip", "0", "--tta", "2"])
    assert (p.clahe, p.clahe_grid, p.clahe_clip, p.tta) == (True, [4, 4], 0.0, 2)
