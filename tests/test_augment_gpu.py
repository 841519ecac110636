"""GPU: cx_u8_affine (chexpert_amd/csrc/augment.hip) against the float64 statement of its definition
(chexpert_amd.augment.affine_reference, itself pinned to torch's grid_sample in tests/test_augment_cpu.py), the --affine flag of
the command line and test-time augmentation in predict."""
import json

import pytest
import torch

from chexpert_amd import augment, synth

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    from chexpert_amd import _lib
    _lib.lib()          # fail loudly if the HIP library is missing
    return torch.device("cuda:0")


def _noise(seed, B, H, W):
    """(B,1,H,W) uint8 iid U{0..255}: synth.xray_u8's generator at a non-square size."""
    s = max(H, W)
    n = -(-B * H * W // (s * s))
    return synth.xray_u8(seed, n, s).flatten()[:B * H * W].reshape(B, 1, H, W).contiguous()


@pytest.mark.parametrize("H,W", [(96, 96), (320, 320), (320, 384)])
@pytest.mark.parametrize("fill", [0, 128])
def test_kernel_against_the_float64_restatement(dev, H, W, fill):
    """Noise input (the hardest case for rounding: every value is equally likely), RandomAffine at degrees 15, translate 0.05,
    scale 0.9-1.1, shear 5.  The kernel works in fp32, the statement in float64, so a pixel may round the other way where the
    float64 value lies next to x.5:
      * every pixel differs by at most 1 grey level;
      * a pixel may differ only where the float64 value before rounding lies within 2e-2 of a rounding boundary;
      * at most 2e-3 of all pixels differ.
    Origin of the numbers: the definition evaluated in plain fp32 on the CPU against float64 at these inputs and ranges deviates
    by at most 2.2e-3 (96^2) / 7.5e-3 (320^2) grey levels (coordinate rounding times a gradient of up to 255 levels per pixel) and
    rounds 1.6e-4 / 5.0e-4 of the pixels differently, none outside the window; the window is 2.7x that deviation and the cap 4x
    that share, which covers fused multiply-adds contracting differently.  The cap keeps the window from hiding a shifted image:
    a one-pixel shift of noise changes > 99 % of the pixels."""
    from chexpert_amd import ops
    B = 6
    u8 = _noise(400 + H + W, B, H, W) if H != W else synth.xray_u8(400 + H, B, H)
    mat = augment.affine_matrices(900 + H + W + fill, B, H, W, degrees=15.0, translate=0.05, scale=(0.9, 1.1), shear=5.0)
    got = ops.u8_affine(u8.to(dev), mat.to(dev), fill).cpu()
    assert got.shape == u8.shape and got.dtype == torch.uint8
    val = augment.affine_reference(u8, mat, fill, rounded=False)
    want = augment.affine_reference(u8, mat, fill)
    diff = (got.int() - want.int()).abs()
    frac = val + 0.5 - torch.floor(val + 0.5)                          # distance above the boundary x.5 (mod 1)
    near = torch.minimum(frac, 1.0 - frac) <= 2e-2
    share = (diff > 0).double().mean().item()
    outside = int(((diff > 0) & ~near).sum())
    print("u8_affine %dx%d fill %d: max diff %d, share differing %.3e, differing outside the window %d"
          % (H, W, fill, diff.max().item(), share, outside))
    assert diff.max().item() <= 1
    assert outside == 0
    assert share <= 2e-3
    assert (want != u8).double().mean().item() > 0.9                   # the warp did something
    if fill:                                                           # the uncovered corners hold `fill` (noise alone: 1 / 256)
        assert (got == fill).double().mean().item() > 0.01


def test_strong_minification_takes_the_same_definition(dev):
    """Scale 0.2-0.3 (inverse maps that magnify 3-5 x) and +-45 degrees: the source footprint of an output tile is 20 times the tile
    and most samples fall outside the image; same statement, same conditions as above (the sample positions inside the image are of
    the same size, so is the fp32 deviation)."""
    from chexpert_amd import ops
    B, S = 6, 320
    u8 = synth.xray_u8(415, B, S)
    mat = augment.affine_matrices(416, B, S, S, degrees=45.0, translate=0.05, scale=(0.2, 0.3), shear=5.0)
    got = ops.u8_affine(u8.to(dev), mat.to(dev), 50).cpu()
    val = augment.affine_reference(u8, mat, 50, rounded=False)
    diff = (got.int() - augment.affine_reference(u8, mat, 50).int()).abs()
    frac = val + 0.5 - torch.floor(val + 0.5)
    near = torch.minimum(frac, 1.0 - frac) <= 2e-2
    share = (diff > 0).double().mean().item()
    print("u8_affine minifying: max diff %d, share differing %.3e, outside the window %d" % (diff.max().item(), share, int(((diff > 0) & ~near).sum())))
    assert diff.max().item() <= 1 and not ((diff > 0) & ~near).any() and share <= 2e-3
    assert (got == 50).double().mean().item() > 0.5                    # most of the output lies outside the shrunken image


def test_identity_and_integer_translation_bit_for_bit(dev):
    from chexpert_amd import ops
    for H, W in ((96, 96), (320, 384), (50, 68)):                       # the last: partial tiles on both axes
        B = 4
        u8 = _noise(31 + H, B, H, W)
        x = u8.to(dev)
        ident = torch.tensor([1.0, 0, 0, 0, 1, 0]).repeat(B, 1).to(dev)
        assert torch.equal(ops.u8_affine(x, ident, 77).cpu(), u8)
        for tx, ty, fill in ((3, -5, 128), (-17, 9, 0), (0, 40, 255), (W, 0, 9)):
            got = ops.u8_affine(x, torch.tensor([1.0, 0, tx, 0, 1, ty]).repeat(B, 1).to(dev), fill).cpu()
            want = torch.full_like(u8, fill)                            # output (i, j) reads source (i + ty, j + tx)
            i0, i1, j0, j1 = max(0, -ty), min(H, H - ty), max(0, -tx), min(W, W - tx)
            if i1 > i0 and j1 > j0:
                want[:, :, i0:i1, j0:j1] = u8[:, :, i0 + ty:i1 + ty, j0 + tx:j1 + tx]
            assert torch.equal(got, want), (H, W, tx, ty)
            assert torch.equal(want, augment.affine_reference(u8, torch.tensor([1.0, 0, tx, 0, 1, ty]).repeat(B, 1), fill))


def test_rotation_direction(dev):
    """(0,-1,0, 1,0,0) on a square image: u = S-1-i, v = j, every sample on a pixel centre, so y[i][j] = x[j][S-1-i] =
    torch.rot90(x, k=1) bit for bit (derived with affine_reference in tests/test_augment_cpu.py).  A transposed matrix or a forward
    map used as an inverse gives k = -1."""
    from chexpert_amd import ops
    u8 = synth.xray_u8(77, 3, 96)
    rot = torch.tensor([0.0, -1, 0, 1, 0, 0]).repeat(3, 1)
    got = ops.u8_affine(u8.to(dev), rot.to(dev)).cpu()
    assert torch.equal(augment.affine_reference(u8, rot, 0), torch.rot90(u8, 1, (-2, -1)))
    assert torch.equal(got, torch.rot90(u8, 1, (-2, -1)))
    assert not torch.equal(got, torch.rot90(u8, -1, (-2, -1)))


def test_reproducible_out_argument_and_errors(dev):
    from chexpert_amd import ops
    B, S = 5, 128
    u8 = synth.xray_u8(5, B, S).to(dev)
    mat = augment.affine_matrices(6, B, S, S).to(dev)
    a = ops.u8_affine(u8, mat, 3)
    b = ops.u8_affine(u8, mat, 3)
    assert torch.equal(a, b)                                            # one writer per byte, no atomics
    out = torch.full_like(u8, 200)
    r = ops.u8_affine(u8, mat, 3, out=out)
    assert r is out and torch.equal(out, a)
    assert torch.equal(ops.u8_affine(u8[:, 0], mat, 3), a[:, 0])        # (B,H,W) form
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.u8_affine(u8.cpu(), mat.cpu())
    with pytest.raises(RuntimeError, match="unsupported shape"):
        ops.u8_affine(torch.zeros(2, 1, 16, 18, dtype=torch.uint8, device=dev), mat[:2])        # W % 4 != 0
    # matrices that send every sample far outside (or nowhere at all) give `fill` everywhere
    wild = torch.tensor([[1e30, 0, 0, 0, 1, 0], [1, 0, -1e9, 0, 1, 1e9], [float("nan")] * 6, [0, 0, 1e4, 0, 0, 0], [1, 0, 0, 0, 1, float("inf")]])
    assert (ops.u8_affine(u8, wild.to(dev), 42) == 42).all()


def _losses(capsys):
    out = capsys.readouterr().out
    return [json.loads(l)["train_loss"] for l in out.splitlines() if l.startswith('{"step"')]


def test_cli_affine_runs_reproducibly_and_only_when_asked(dev, tmp_path, capsys, monkeypatch):
    """--train --fused_optimizer --graph --affine --jitter: the warp runs eagerly on the uint8 batch in front of the jitter and the
    captured step; the run ends, logs finite losses, and the same command logs the same losses again (seeded draw, deterministic
    engine).  Without --affine ops.u8_affine is never called: the default path is untouched."""
    import math
    from chexpert_amd import cli, ops
    calls = []
    real = ops.u8_affine

    def counted(x, mat, fill=0, out=None):
        calls.append(tuple(x.shape))
        assert x.dtype == torch.uint8 and x.is_cuda
        return real(x, mat, fill, out)
    monkeypatch.setattr(ops, "u8_affine", counted)
    # (--seed: without it the weights are initialised from torch's global generator, which two runs in one process do not share)
    base = ["--train", "--fused_optimizer", "--graph", "--jitter", "--synthetic", "16", "--batch_size", "4", "--resize", "64",
            "--eval_interval", "4", "--log_interval", "1", "--seed", "3"]
    capsys.readouterr()
    cli.main(base + ["--affine", "--output_dir", str(tmp_path / "a")])
    la = _losses(capsys)
    assert len(la) == 4 and all(math.isfinite(v) for v in la), la
    assert calls == [(4, 1, 64, 64)] * 4                                # once per minibatch, never in the evaluation passes
    cli.main(base + ["--affine", "--output_dir", str(tmp_path / "b")])
    assert _losses(capsys) == la
    del calls[:]
    cli.main(base + ["--output_dir", str(tmp_path / "c")])
    lc = _losses(capsys)
    assert not calls and len(lc) == 4
    assert lc[0] != la[0]                                               # the warped first batch is another input
    # a partial last minibatch (18 = 4 x 4 + 2) takes the eager step behind the same warp
    cli.main(base + ["--affine", "--synthetic", "18", "--output_dir", str(tmp_path / "d")])
    lp = _losses(capsys)
    assert calls == [(4, 1, 64, 64)] * 4 + [(2, 1, 64, 64)] and len(lp) == 5 and all(math.isfinite(v) for v in lp)


class _Studies(torch.utils.data.Dataset):
    """What predict() needs of a ChexpertCSV: uint8 items, attr_names, and a Path column for the study names."""
    attr_names = ["Atelectasis", "Cardiomegaly", "Consolidation", "Edema", "Pleural Effusion"]

    def __init__(self, n, size):
        import pandas as pd
        self.x = synth.xray_u8(123, n, size)
        # study 0 has two views
        self.data = pd.DataFrame({"Path": ["valid/patient%05d/study1/view%d_frontal.jpg" % (max(i, 1), i) for i in range(n)]})

    def __len__(self):
        return len(self.x)

    def __getitem__(self, i):
        return self.x[i], torch.zeros(5), i


def test_predict_test_time_augmentation(dev):
    """tta=1 is the plain path bit for bit; tta=4 is the mean over the unwarped forward and three forwards of batches warped by
    ops.u8_affine (held against affine_reference here) with the documented seeds and ranges; two calls agree bit for bit."""
    from chexpert_amd import ops, predict
    from chexpert_amd.models import DenseNet
    torch.manual_seed(0)
    model = DenseNet(32, (2, 2, 2, 2), 64, num_classes=5).to(dev).eval()
    ds, bs = _Studies(8, 64), 3
    with torch.no_grad():
        plain = torch.cat([torch.sigmoid(model(ds.x[k:k + bs].to(dev)).float()).cpu() for k in range(0, 8, bs)])
    p1 = predict.predict(model, ds, bs, dev)
    assert len(p1) == 7 and list(p1.columns) == ds.attr_names
    assert torch.equal(torch.from_numpy(p1.values[1:]), plain[2:])                          # the other studies: one view each
    assert torch.equal(torch.from_numpy(p1.values[0]), torch.maximum(plain[0], plain[1]))   # max over the two views
    assert predict.predict(model, ds, bs, dev, tta=1, tta_seed=9).equals(p1)
    want = []
    with torch.no_grad():
        for n, k in enumerate(range(0, 8, bs)):
            x = ds.x[k:k + bs]
            ps = [torch.sigmoid(model(x.to(dev)).float()).cpu().double()]
            for draw in (1, 2, 3):
                mat = augment.affine_matrices(augment.tta_seed_of(5, draw, n), len(x), 64, 64, degrees=5.0, translate=0.025,
                                              scale=(0.95, 1.05), shear=0.0)
                w = ops.u8_affine(x.to(dev), mat.to(dev))
                ref = augment.affine_reference(x, mat, 0)
                d = (w.cpu().int() - ref.int()).abs()
                assert d.max().item() <= 1 and (d > 0).double().mean().item() <= 2e-3
                ps.append(torch.sigmoid(model(w).float()).cpu().double())
            want.append(torch.stack(ps).mean(0))
    want = torch.cat(want)
    want = torch.cat([torch.maximum(want[0], want[1])[None], want[2:]])
    p4 = predict.predict(model, ds, bs, dev, tta=4, tta_seed=5)
    # the product sums four fp32 probabilities in [0, 1] and divides by 4: within 4 fp32 roundings of the float64 mean
    assert (torch.from_numpy(p4.values).double() - want).abs().max().item() <= 4 * 2.0 ** -24
    assert (p4.values != p1.values).any()
    assert predict.predict(model, ds, bs, dev, tta=4, tta_seed=5).equals(p4)
    assert not predict.predict(model, ds, bs, dev, tta=4, tta_seed=6).equals(p4)
