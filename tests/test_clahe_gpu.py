"""GPU: cx_u8_clahe_lut and cx_u8_clahe_apply (chexpert_amd/csrc/clahe.hip) against the integer statement of their definition
(chexpert_amd.augment.clahe_reference, itself pinned in tests/test_clahe_cpu.py) -- exact equality, the definition has no float in
it -- and the --clahe flag of the command line and of predict."""
import functools
import json
import math

import numpy as np
import pytest
import torch

from chexpert_amd import augment, synth

pytestmark = pytest.mark.gpu

# (H, W, grid): the smallest shapes at which each mechanism can go wrong
SHAPES = [
    (32, 32, (2, 2)),          # area = 256
    (64, 96, (4, 3)),          # non-square tile 16 x 32, odd grid
    (48, 80, (3, 5)),
    (64, 64, (1, 1)),          # global
    (64, 64, (16, 16)),        # 4 x 4 tiles: every occupied bin is clipped at any limit
    (320, 320, (8, 8)),        # the workload's tile, 40 x 40: a 4-pixel lane never straddles two tiles, a 64-wide strip does
    (320, 384, (8, 8)),
    # beyond the listed ones: tiles whose width is no multiple of 4 (the byte path of the table kernel; a lane's four pixels straddle
    # table columns), and a tile higher than the 64 rows one workgroup of the apply kernel takes (a band split into chunks)
    (20, 36, (2, 6)),
    (160, 32, (1, 2)),
]
CLIPS = [0.0, 0.01, 2.0, 40.0]


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    from chexpert_amd import _lib
    _lib.lib()          # fail loudly if the HIP library is missing
    return torch.device("cuda:0")


def _ramp(H, W, lo=100, hi=140):
    return np.broadcast_to((lo + (np.arange(W) * (hi - lo + 1)) // W).astype(np.uint8), (H, W)).copy()


@functools.lru_cache(maxsize=None)
def _images(H, W, grid):
    """One batch per shape, holding every kind of image (so every batch has 6 images, at least as many as a smaller batch would
    need): [0] a low-contrast horizontal ramp confined to 100..140, [1] a ramp plus Gaussian blobs, [2] constant tiles beside noise
    tiles (a checkerboard of the grid), [3] white noise, [4] all 0, [5] all 255."""
    rng = np.random.default_rng(H * 4099 + W * 17 + grid[0])
    th, tw = H // grid[0], W // grid[1]
    i, j = np.mgrid[0:H, 0:W].astype(np.float64)
    blobs = _ramp(H, W, 60, 120).astype(np.float64)
    for _ in range(6):
        ci, cj, s, a = rng.uniform(0, H), rng.uniform(0, W), rng.uniform(2, max(H, W) / 4), rng.uniform(40, 130)
        blobs += a * np.exp(-((i - ci) ** 2 + (j - cj) ** 2) / (2 * s * s))
    noise = rng.integers(0, 256, (H, W), dtype=np.uint8)
    board = ((np.arange(H)[:, None] // th + np.arange(W)[None, :] // tw) % 2).astype(bool)
    if grid == (1, 1):                                                  # one tile: left half constant, right half noise
        board = np.broadcast_to(np.arange(W)[None, :] >= W // 2, (H, W))
    mixed = np.where(board, rng.integers(0, 256, (H, W), dtype=np.uint8), np.uint8(93))
    x = np.stack([_ramp(H, W), np.clip(blobs, 0, 255).astype(np.uint8), mixed.astype(np.uint8), noise,
                  np.zeros((H, W), np.uint8), np.full((H, W), 255, np.uint8)])
    return torch.from_numpy(x).contiguous()


@functools.lru_cache(maxsize=None)
def _reference(case, clip):
    """(x, y, lut, residuals) of SHAPES[case] at clip limit `clip`, computed once on the CPU and shared (never written to)."""
    H, W, grid = SHAPES[case]
    x = _images(H, W, grid)
    L = augment.clahe_clip_count(clip, H // grid[0], W // grid[1])
    lut, res = augment.clahe_tables_reference(x, grid, L)
    y, lut2 = augment.clahe_reference(x, grid, clip, return_lut=True)
    assert torch.equal(lut, lut2)
    return x, y, lut, res


def _where(a, b):
    bad = (a != b).nonzero()
    return "equal" if not len(bad) else "%d differ, first at %s: got %d, want %d" % (len(bad), bad[0].tolist(), a[tuple(bad[0])], b[tuple(bad[0])])


@pytest.mark.parametrize("clip", CLIPS)
@pytest.mark.parametrize("case", range(len(SHAPES)))
def test_tables_apply_and_both_against_the_integer_reference(dev, case, clip):
    from chexpert_amd import ops
    H, W, grid = SHAPES[case]
    x, want, want_lut, _ = _reference(case, clip)
    xd = x.to(dev)
    L = augment.clahe_clip_count(clip, H // grid[0], W // grid[1])
    lut = ops.u8_clahe_lut(xd, grid, L)
    assert lut.dtype == torch.uint8 and tuple(lut.shape) == (x.shape[0], grid[0], grid[1], 256)
    assert torch.equal(lut.cpu(), want_lut), "tables: " + _where(lut.cpu(), want_lut)
    got = ops.u8_clahe_apply(xd, want_lut.to(dev))                      # the stage on its own: fed the reference's tables
    assert torch.equal(got.cpu(), want), "apply: " + _where(got.cpu(), want)
    both = ops.u8_clahe(xd, grid, clip)
    assert both.dtype == torch.uint8 and both.shape == x.shape
    assert torch.equal(both.cpu(), want), "end to end: " + _where(both.cpu(), want)
    assert (want[0] != x[0]).double().mean().item() > 0.5               # the step did something to the low-contrast ramp


def test_the_cases_cover_every_kind_of_redistribution_residual():
    """r = excess % 256 of every tile of every case above, from the reference: r == 0 (nothing left over, or nothing clipped),
    0 < r <= 128 (step >= 2: every step-th bin gets one) and r > 128 (step == 1: the first r bins)."""
    seen = {"zero": 0, "low": 0, "high": 0}
    clipped_tiles = 0
    for case in range(len(SHAPES)):
        for clip in CLIPS:
            x, _, _, res = _reference(case, clip)
            r = res.numpy().ravel()
            seen["zero"] += int((r == 0).sum())
            seen["low"] += int(((r > 0) & (r <= 128)).sum())
            seen["high"] += int((r > 128).sum())
            if clip > 0:
                clipped_tiles += r.size
    print("redistribution residuals over all cases:", seen, "clipped tiles:", clipped_tiles)
    assert seen["zero"] > 0 and seen["low"] > 0 and seen["high"] > 0


def test_boundary_rows_and_columns_and_the_central_cross(dev):
    """32 x 32 at 2 x 2 (tiles 16 x 16), region by region, so that a failure names where the interpolation went wrong: the outer
    th/2 rows and tw/2 columns (both tables clamp to the same tile), and the central cross (where the weights change tile)."""
    from chexpert_amd import ops
    for clip in (0.0, 2.0):
        x, want, lut, _ = _reference(0, clip)
        got = ops.u8_clahe_apply(x.to(dev), lut.to(dev)).cpu()
        regions = {"top rows": (slice(0, 8), slice(None)), "bottom rows": (slice(24, 32), slice(None)),
                   "left columns": (slice(None), slice(0, 8)), "right columns": (slice(None), slice(24, 32)),
                   "horizontal bar of the cross": (slice(14, 18), slice(None)), "vertical bar of the cross": (slice(None), slice(14, 18)),
                   "interior": (slice(8, 24), slice(8, 24))}
        for name, (ri, rj) in regions.items():
            assert torch.equal(got[:, ri, rj], want[:, ri, rj]), "%s (clip %g): %s" % (name, clip, _where(got[:, ri, rj], want[:, ri, rj]))
        # in the corners one table alone decides: the output is that tile's table of the input
        for (ri, rj, gy, gx) in ((slice(0, 8), slice(0, 8), 0, 0), (slice(0, 8), slice(24, 32), 0, 1), (slice(24, 32), slice(0, 8), 1, 0)):
            for b in range(x.shape[0]):
                assert torch.equal(got[b, ri, rj], lut[b, gy, gx][x[b, ri, rj].long()])


def test_run_to_run_identity_out_argument_four_dim_and_unaligned_input(dev):
    from chexpert_amd import ops
    x, want, lut, _ = _reference(5, 2.0)                                # 320 x 320, 8 x 8
    xd = x.to(dev)
    a, b = ops.u8_clahe(xd, (8, 8), 2.0), ops.u8_clahe(xd, (8, 8), 2.0)
    assert torch.equal(a, b) and torch.equal(a.cpu(), want)             # integer LDS adds, one writer per byte
    assert torch.equal(ops.u8_clahe_lut(xd, (8, 8), 12), ops.u8_clahe_lut(xd, (8, 8), 12))
    out = torch.full_like(xd, 200)
    r = ops.u8_clahe(xd, (8, 8), 2.0, out=out)
    assert r is out and torch.equal(out, a)
    r = ops.u8_clahe_apply(xd, lut.to(dev), out=out.fill_(7))
    assert r is out and torch.equal(out, a)
    x4 = xd[:, None].contiguous()                                       # (B, 1, H, W)
    y4 = ops.u8_clahe(x4, (8, 8), 2.0)
    assert y4.shape == x4.shape and torch.equal(y4[:, 0], a)
    # an input that starts at an odd address (the kernels then read it byte by byte)
    buf = torch.zeros(x.numel() + 4, dtype=torch.uint8, device=dev)
    odd = buf[1:1 + x.numel()].view(x.shape)
    odd.copy_(xd)
    assert odd.data_ptr() % 4 == 1 and odd.is_contiguous()
    assert torch.equal(ops.u8_clahe_lut(odd, (8, 8), 12).cpu(), lut) and torch.equal(ops.u8_clahe(odd, (8, 8), 2.0), a)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.u8_clahe(x, (8, 8), 2.0)
    with pytest.raises(RuntimeError, match="unsupported shape"):
        ops.u8_clahe(xd, (7, 8), 2.0)
    with pytest.raises(RuntimeError, match="unsupported shape"):
        ops.u8_clahe_lut(xd, (17, 8), 0)
    with pytest.raises(RuntimeError, match="cx_u8_clahe_apply failed"):
        ops.u8_clahe_apply(xd, lut.to(dev), out=xd)                     # in place


def _losses(text):
    return [json.loads(l)["train_loss"] for l in text.splitlines() if l.startswith('{"step"')]


def test_cli_clahe_trains_evaluates_and_only_runs_when_asked(dev, tmp_path, capsys, monkeypatch):
    """--train --synthetic --clahe --fused_optimizer --graph ends with finite losses, equalising every training AND every evaluation
    batch; --evaluate_single_model --clahe runs on its checkpoint, with the flags restored from the run's config.json; without
    --clahe ops.u8_clahe is never called (the default path gains no launch)."""
    from chexpert_amd import cli, ops
    calls = []
    real = ops.u8_clahe

    def counted(x, grid=(8, 8), clip_limit=2.0, out=None):
        calls.append((tuple(x.shape), tuple(grid), clip_limit))
        assert x.dtype == torch.uint8 and x.is_cuda
        return real(x, grid, clip_limit, out)
    monkeypatch.setattr(ops, "u8_clahe", counted)
    base = ["--train", "--fused_optimizer", "--graph", "--synthetic", "16", "--batch_size", "4", "--resize", "64", "--eval_interval", "4",
            "--log_interval", "1", "--seed", "3"]
    capsys.readouterr()
    cli.main(base + ["--clahe", "--clahe_grid", "4", "4", "--clahe_clip", "3.0", "--output_dir", str(tmp_path / "a")])
    la = _losses(capsys.readouterr().out)
    assert len(la) == 4 and all(math.isfinite(v) for v in la), la
    # 4 training batches; the evaluation at step 4 and the one at the end of the epoch: 1 validation batch of 4 each
    assert calls == [((4, 1, 64, 64), (4, 4), 3.0)] * 6
    cfg = json.load(open(tmp_path / "a" / "config.json"))
    assert (cfg["clahe"], cfg["clahe_grid"], cfg["clahe_clip"]) == (True, [4, 4], 3.0)
    del calls[:]
    cfg.update(train=False, evaluate_single_model=True, restore=str(tmp_path / "a" / "checkpoint_latest.pt"), output_dir=str(tmp_path / "e"))
    json.dump(cfg, open(tmp_path / "eval.json", "w"))
    cli.main(["--load_config", str(tmp_path / "eval.json")])
    assert calls == [((4, 1, 64, 64), (4, 4), 3.0)]
    res = json.load(open(tmp_path / "e" / "eval_results_step_4.json"))
    assert all(math.isfinite(v) for v in res["loss"].values())
    del calls[:]
    capsys.readouterr()
    cli.main(base + ["--output_dir", str(tmp_path / "c")])
    lc = _losses(capsys.readouterr().out)
    assert not calls and len(lc) == 4 and lc[0] != la[0]                # the equalised first batch is another input


def test_first_training_batch_is_jitter_of_affine_of_clahe(dev, tmp_path, monkeypatch):
    """--clahe --affine --jitter: what the network receives for the first minibatch equals jitter(affine(clahe_reference(x))) bit for
    bit -- the existing kernels applied to the reference's bytes with the step's seeds."""
    from chexpert_amd import cli, ops
    from chexpert_amd.models import _fused
    raw, fed = [], []
    real_clahe, real_fb = ops.u8_clahe, _fused.FusedNet.forward_backward

    def clahe(x, grid=(8, 8), clip_limit=2.0, out=None):
        raw.append(x.cpu())
        return real_clahe(x, grid, clip_limit, out)

    def forward_backward(self, x, target, input_grad=None):
        fed.append(x.cpu())
        return real_fb(self, x, target, input_grad)
    monkeypatch.setattr(ops, "u8_clahe", clahe)
    monkeypatch.setattr(_fused.FusedNet, "forward_backward", forward_backward)
    cli.main(["--train", "--fused_optimizer", "--synthetic", "8", "--batch_size", "4", "--resize", "64", "--eval_interval", "100", "--log_interval", "1",
              "--seed", "3", "--clahe", "--affine", "--jitter", "--output_dir", str(tmp_path / "o")])
    assert len(fed) == 2 and fed[0].dtype == torch.uint8
    x0, B = raw[0], 4
    ref = augment.clahe_reference(x0, (8, 8), 2.0)
    assert (ref != x0).double().mean().item() > 0.5
    mat = augment.affine_matrices(augment.step_seed(1, 0), B, 64, 64, **augment.TRAIN_DEFAULTS)
    warped = ops.u8_affine(ref.to(dev), mat.to(dev), 0)
    u = synth.uniform(1 * 7919 + 13, (3, B), 0.0, 1.0)
    want = ops.u8_jitter(warped, (0.75 + 0.5 * u[0]).to(dev), (0.75 + 0.5 * u[1]).to(dev), (u[2] > 0.5).to(torch.int32).to(dev)).cpu()
    assert torch.equal(fed[0], want), _where(fed[0], want)


class _Studies(torch.utils.data.Dataset):
    """What predict() needs of a ChexpertCSV: uint8 items, attr_names, and a Path column for the study names."""
    attr_names = ["Atelectasis", "Cardiomegaly", "Consolidation", "Edema", "Pleural Effusion"]

    def __init__(self, n, size):
        import pandas as pd
        self.x = torch.from_numpy(np.stack([_ramp(size, size, 90 + 5 * i, 150 + 5 * i) for i in range(n)]))[:, None].contiguous()
        self.data = pd.DataFrame({"Path": ["valid/patient%05d/study1/view1_frontal.jpg" % i for i in range(n)]})

    def __len__(self):
        return len(self.x)

    def __getitem__(self, i):
        return self.x[i], torch.zeros(5), i


def test_predict_with_clahe_and_test_time_augmentation(dev):
    """predict(clahe=...) equalises each batch once, before the plain forward and before each draw's warp: with --tta 2 the result is
    the mean of the forward of the equalised batch and the forward of its warp."""
    from chexpert_amd import ops, predict
    from chexpert_amd.models import DenseNet
    torch.manual_seed(0)
    model = DenseNet(32, (2, 2, 2, 2), 64, num_classes=5).to(dev).eval()
    ds, bs = _Studies(5, 64), 3
    step = augment.Clahe((4, 4), 2.0)
    p = predict.predict(model, ds, bs, dev, tta=2, tta_seed=5, clahe=step)
    want = []
    with torch.no_grad():
        for n, k in enumerate(range(0, 5, bs)):
            x = ds.x[k:k + bs]
            eq = augment.clahe_reference(x, (4, 4), 2.0).to(dev)
            assert torch.equal(step(x.to(dev)), eq)
            mat = augment.affine_matrices(augment.tta_seed_of(5, 1, n), len(x), 64, 64, **augment.TTA_RANGES)
            ps = torch.sigmoid(model(eq).float()) + torch.sigmoid(model(ops.u8_affine(eq, mat.to(dev))).float())
            want.append((ps / 2).cpu())
    assert torch.equal(torch.from_numpy(p.values), torch.cat(want))
    plain = predict.predict(model, ds, bs, dev, tta=2, tta_seed=5)
    assert (plain.values != p.values).any()                            # the flag changes the input; without it nothing is equalised
    assert predict.predict(model, ds, bs, dev, tta=2, tta_seed=5, clahe=step).equals(p)
    args = predict.parse_args(["a.csv", "b.csv", "--restore_path", "x", "--resize", "64", "--clahe", "--clahe_grid", "4", "4", "--tta", "2"])
    assert (args.clahe, args.clahe_grid, args.clahe_clip, args.tta) == (True, [4, 4], 2.0, 2)
