"""GPU: cx_u8_mix and cx_target_mix (chexpert_amd/csrc/mix.hip) against the numpy statements of their definitions
(chexpert_amd.augment.mix_reference / target_mix_reference, pinned in tests/test_mix_cpu.py), SampleMix, and the --mixup / --cutmix /
--erase_prob flags of the command line.  The definitions are integer / separately rounded fp32, so every comparison is torch.equal:
there is no tolerance to choose."""
import contextlib
import io
import json
import math

import numpy as np
import pytest
import torch

from chexpert_amd import augment, synth

pytestmark = pytest.mark.gpu
ONE = 65536


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


def _dev_plan(dev, *arrays):
    return [torch.from_numpy(np.ascontiguousarray(a, dtype=np.int32)).to(dev) for a in arrays]


def _row_specs(B, H, W):
    """(perm or None = the next row, lam_q, box) of every row case the kernel can take another path on."""
    full = (0, H, 0, W)
    xa, xb = (3, 9) if W < 64 else (37, min(203, W - 1))                 # edges not on multiples of 4 (nor of 16)
    boxes = [(0, 0, 0, 0), (3, 3, 0, W),                                # empty
             (H // 2, H // 2 + 1, W // 2 + 1, W // 2 + 2),              # a single pixel
             (1, H - 2, xa, xb),                                        # unaligned edges
             (0, H // 2, 0, 5), (H - 3, H, W - 5, W),                   # touching the top-left / bottom-right corners
             (0, 1, 0, W), (H - 1, H, 0, W), (0, H, 0, 1), (0, H, W - 1, W)]      # one row / column on each border
    specs = [(None, q, full) for q in (0, 1, 32768, 65535, ONE)]
    specs += [(None, q, bx) for bx in boxes for q in (0, 32768)]
    specs += [("self", 100, full), ("self", 0, (1, H - 2, xa, xb))]     # a fixed point of perm
    specs += [(-1, 0, full), (-1, 0, (1, H - 2, xa, xb)), (-1, 21845, (0, H // 2, 0, 5)), (-9, 0, (H - 3, H, W - 5, W))]   # fill
    specs += [(B + 7, 70000, (-5, H + 9, -3, W + 100)),                 # out of range: clamped to the partner B-1 at lambda = 1 ...
              (B + 7, 12345, (-5, H + 9, -3, W + 100)),                 # ... and at a lambda that reads it
              (None, -4, (H - 2, 2 ** 30, W - 6, 2 ** 30))]
    return specs


@pytest.mark.parametrize("B,H,W", [(5, 12, 20), (4, 50, 68), (4, 320, 320), (2, 1024, 1024)])
def test_kernel_against_the_integer_statement(dev, B, H, W):
    """Noise images; (5, 12, 20): odd batch, smaller than any workgroup, the dword path; (4, 50, 68): partial bands, dword path;
    (4, 320, 320): the 16-byte path, several bands per image; (2, 1024, 1024): the size limit.  The row cases of _row_specs are
    dealt B at a time, with fill 0 and 136 alternating."""
    from chexpert_amd import ops
    u8 = _noise(700 + H + W, B, H, W)
    x = u8.to(dev)
    specs = _row_specs(B, H, W)
    specs += specs[:(-len(specs)) % B]
    changed = 0
    for n, k in enumerate(range(0, len(specs), B)):
        rows = specs[k:k + B]
        perm = [(b + 1) % B if p is None else b if p == "self" else p for b, (p, _, _) in enumerate(rows)]
        lam_q, box, fill = [q for _, q, _ in rows], [bx for _, _, bx in rows], (0, 136)[n % 2]
        got = ops.u8_mix(x, *_dev_plan(dev, perm, lam_q, box), fill).cpu()
        want = augment.mix_reference(u8, np.array(perm), np.array(lam_q), np.array(box), fill)
        assert got.shape == u8.shape and got.dtype == torch.uint8
        assert torch.equal(got, want), (B, H, W, rows)
        changed += int((want != u8).sum())
    assert changed > H * W                                               # the plans did something


@pytest.mark.parametrize("B,H,W", [(3, 8, 32), (2, 64, 80)])
def test_kernel_on_a_dword_aligned_view(dev, B, H, W):
    """W % 16 == 0 but the images start 4 bytes into an allocation: the dword path at a width the 16-byte path would take."""
    from chexpert_amd import ops
    u8 = _noise(9, B, H, W)
    buf = torch.empty(B * H * W + 16, dtype=torch.uint8, device=dev)
    x = buf[4:4 + B * H * W].view(B, 1, H, W)
    x.copy_(u8)
    assert x.data_ptr() % 16 == 4
    perm, lam_q, box = [1, 2, 0][:B] if B == 3 else [1, 0], [30000, 0, 7][:B], [[0, H, 0, W], [1, H - 1, 3, 9], [2, 5, 0, W]][:B]
    got = ops.u8_mix(x, *_dev_plan(dev, perm, lam_q, box), 5).cpu()
    assert torch.equal(got, augment.mix_reference(u8, np.array(perm), np.array(lam_q), np.array(box), 5))


def _targets(seed, B, n):
    """Hard labels with a share of soft (label-smoothed) and ignored (-1) ones."""
    t = synth.targets(seed, B, n)
    u = synth.uniform(seed + 1, (B, n), 0.0, 1.0)
    t = torch.where(u < 0.25, synth.uniform(seed + 2, (B, n), 0.0, 1.0), t)
    return torch.where(u > 0.8, torch.full_like(t, -1.0), t).contiguous()


@pytest.mark.parametrize("B,n", [(5, 5), (256, 14)])
def test_target_mix_against_the_fp32_statement(dev, B, n):
    from chexpert_amd import ops
    t = _targets(40 + B, B, n)
    assert (t < 0).any() and ((t > 0) & (t < 1)).any() and (t == 1).any()
    perm = np.argsort(synth.uniform(41, (B,)).numpy(), kind="stable")
    tw_q = (synth.uniform(42, (B,), 0.0, 1.0).double().numpy() * 65537).astype(np.int64)
    perm[0], tw_q[1], tw_q[2], perm[3], tw_q[3], perm[4], tw_q[4] = -1, ONE, 0, B + 7, 70000, -9, -3
    tw_q[B // 2] = 21845                                                 # w = 1/3 to 16 bits: products that round
    got = ops.target_mix(t.to(dev), *_dev_plan(dev, perm, tw_q)).cpu()
    want = augment.target_mix_reference(t, perm, tw_q)
    assert got.dtype == torch.float32 and torch.equal(got, want)
    assert torch.equal(got[0], t[0]) and torch.equal(got[1], t[1]) and (got != t).any()
    assert ((got == -1) == ((t < 0) | (t[np.clip(perm, 0, B - 1)] < 0)))[5:].all()


def test_target_blend_is_not_contracted(dev):
    """w t + (1 - w) u with separately rounded products: inputs at which a fused multiply-add gives another last bit."""
    from chexpert_amd import ops
    B, n = 64, 14
    t = synth.uniform(50, (B, n), 0.0, 1.0).contiguous()
    perm = np.roll(np.arange(B), 1)
    tw_q = np.full(B, 21845)
    want = augment.target_mix_reference(t, perm, tw_q)
    w = np.float32(21845 * 2.0 ** -16)
    w1 = np.float32(1) - w
    a, o = t.numpy(), t.numpy()[perm]
    # what a contracted build would give: one product kept exact inside a fused multiply-add (float64 holds it exactly)
    fused_a = (np.float64(w) * a.astype(np.float64) + (w1 * o).astype(np.float64)).astype(np.float32)
    fused_o = ((w * a).astype(np.float64) + np.float64(w1) * o.astype(np.float64)).astype(np.float32)
    assert (fused_a != want.numpy()).any() and (fused_o != want.numpy()).any()      # the inputs tell the two apart
    assert torch.equal(ops.target_mix(t.to(dev), *_dev_plan(dev, perm, tw_q)).cpu(), want)


@pytest.mark.parametrize("kw", [{"mixup_alpha": 0.4}, {"cutmix_alpha": 1.0}, {"mixup_alpha": 0.4, "cutmix_alpha": 1.0},
                                {"mixup_alpha": 0.4, "mode": "elem"}, {"cutmix_alpha": 1.0, "mode": "elem"},
                                {"mixup_alpha": 0.4, "cutmix_alpha": 1.0, "mode": "elem"},
                                {"erase_prob": 0.5}, {"cutmix_alpha": 1.0, "mode": "elem", "erase_prob": 0.5, "erase_fill": 7}])
def test_sample_mix_follows_the_plans(dev, kw):
    B, S, n, rank = 6, 64, 5, 1
    u8, t = synth.xray_u8(60, B, S), _targets(61, B, n)
    sm = augment.make_sample_mix(rank=rank, device=dev, **kw)
    mix = {k: v for k, v in kw.items() if not k.startswith("erase")}
    for step in (1, 2, 3):
        x, tt = sm(u8.to(dev), t.to(dev), step)
        wx, wt = u8, t
        if mix:
            p = augment.mix_plan(augment.mix_seed(step, rank), B, S, S, **mix)
            wx = augment.mix_reference(wx, p["perm"], p["lam_q"], p["box"], 0)
            wt = augment.target_mix_reference(wt, p["perm"], p["tw_q"])
        if "erase_prob" in kw:
            e = augment.erase_plan(augment.erase_seed(step, rank), B, S, S, prob=kw["erase_prob"])
            wx = augment.mix_reference(wx, e["perm"], e["lam_q"], e["box"], kw.get("erase_fill", 136))
        assert torch.equal(x.cpu(), wx) and torch.equal(tt.cpu(), wt), (kw, step)
    assert not torch.equal(x.cpu(), u8)


def test_reproducible_out_argument_and_errors(dev):
    from chexpert_amd import ops
    B, S = 5, 128
    u8 = synth.xray_u8(5, B, S).to(dev)
    p = augment.mix_plan(6, B, S, S, 0.4, 1.0, mode="elem")
    perm, lam_q, box, tw_q = _dev_plan(dev, p["perm"], p["lam_q"], p["box"], p["tw_q"])
    a = ops.u8_mix(u8, perm, lam_q, box, 3)
    assert torch.equal(a, ops.u8_mix(u8, perm, lam_q, box, 3))            # one writer per byte, no atomics
    out = torch.full_like(u8, 200)
    r = ops.u8_mix(u8, perm, lam_q, box, 3, out=out)
    assert r is out and torch.equal(out, a)
    assert torch.equal(ops.u8_mix(u8[:, 0], perm, lam_q, box, 3), a[:, 0])      # (B,H,W) form
    t = _targets(7, B, 5).to(dev)
    ta = ops.target_mix(t, perm, tw_q)
    assert torch.equal(ta, ops.target_mix(t, perm, tw_q))
    tout = torch.full_like(t, 9.0)
    assert ops.target_mix(t, perm, tw_q, out=tout) is tout and torch.equal(tout, ta)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.u8_mix(u8.cpu(), perm.cpu(), lam_q.cpu(), box.cpu())
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.target_mix(t.cpu(), perm.cpu(), tw_q.cpu())
    with pytest.raises(RuntimeError, match="unsupported shape"):
        ops.u8_mix(torch.zeros(2, 1, 16, 18, dtype=torch.uint8, device=dev), perm[:2], lam_q[:2], box[:2])       # W % 4 != 0
    with pytest.raises(RuntimeError, match="cx_u8_mix"):
        ops.u8_mix(u8, perm, lam_q, box, out=u8)                          # a partner row may be read after it was written
    with pytest.raises(RuntimeError, match="cx_target_mix"):
        ops.target_mix(t, perm, tw_q, out=t)
    with pytest.raises(RuntimeError, match="cx_u8_mix"):
        ops.u8_mix(u8, perm, lam_q, box, 256)


# ---- the command line ----------------------------------------------------------------------------------------------------------------
BASE = ["--train", "--fused_optimizer", "--graph", "--jitter", "--synthetic", "16", "--batch_size", "4", "--resize", "64",
        "--eval_interval", "4", "--log_interval", "1", "--seed", "3"]
_runs = {}


def _run(tmp_path_factory, extra, again=False):
    """One cli.main(BASE + extra): (train losses, shapes ops.u8_mix saw, how often ops.target_mix ran, whether a model was in eval
    mode during a call -- never).  Cached per command line, so the tests below share the runs; `again` runs it a second time."""
    from chexpert_amd import cli, ops
    key = (tuple(extra), again)
    if key in _runs:
        return _runs[key]
    calls, tcalls = [], []
    real, real_t = ops.u8_mix, ops.target_mix

    def counted(x, perm, lam_q, box, fill=0, out=None):
        calls.append((tuple(x.shape), int(fill)))
        assert x.dtype == torch.uint8 and x.is_cuda
        return real(x, perm, lam_q, box, fill, out)

    def counted_t(t, perm, tw_q, out=None):
        tcalls.append(tuple(t.shape))
        return real_t(t, perm, tw_q, out)
    ops.u8_mix, ops.target_mix = counted, counted_t
    buf = io.StringIO()
    try:
        with contextlib.redirect_stdout(buf):
            cli.main(BASE + list(extra) + ["--output_dir", str(tmp_path_factory.mktemp("mix"))])
    finally:
        ops.u8_mix, ops.target_mix = real, real_t
    losses = [json.loads(l)["train_loss"] for l in buf.getvalue().splitlines() if l.startswith('{"step"')]
    _runs[key] = (losses, calls, tcalls)
    return _runs[key]


@pytest.mark.parametrize("flags,per_batch", [(("--mixup", "0.4"), [0]), (("--cutmix", "1.0"), [0]), (("--erase_prob", "0.5"), [136])])
def test_cli_flag_runs_reproducibly(dev, tmp_path_factory, flags, per_batch):
    """--train --fused_optimizer --graph --jitter with one of the flags: the mix runs eagerly on the uint8 batch behind the jitter and
    in front of the captured step; finite losses, the same losses from the same command, ops.u8_mix once per training minibatch and
    never in the evaluation passes (16 / 4 = 4 minibatches; the evaluations at step 4 and at the end add none)."""
    la, calls, tcalls = _run(tmp_path_factory, flags)
    assert len(la) == 4 and all(math.isfinite(v) for v in la), la
    assert calls == [((4, 1, 64, 64), f) for _ in range(4) for f in per_batch]
    assert tcalls == ([] if flags[0] == "--erase_prob" else [(4, 5)] * 4)      # erasing leaves the labels alone
    lb, calls_b, _ = _run(tmp_path_factory, flags, again=True)
    assert lb == la and calls_b == calls


def test_cli_default_path_is_untouched(dev, tmp_path_factory):
    lc, calls, tcalls = _run(tmp_path_factory, ())
    assert not calls and not tcalls and len(lc) == 4
    lo, calls, tcalls = _run(tmp_path_factory, ("--mixup", "0", "--cutmix", "0", "--erase_prob", "0"))
    assert not calls and not tcalls and lo == lc
    lm = _run(tmp_path_factory, ("--mixup", "0.4"))[0]
    assert lm[0] != lc[0]                                                # the mixed first batch is another input


def test_cli_erasing_on_top_of_a_mix_and_the_partial_last_minibatch(dev, tmp_path_factory):
    """18 = 4 x 4 + 2: the last minibatch of 2 takes the eager step behind the same mix; with erasing on top of a mix ops.u8_mix
    runs twice per minibatch, the mix (fill 0) first."""
    lp, calls, tcalls = _run(tmp_path_factory, ("--mixup", "0.4", "--erase_prob", "0.5", "--synthetic", "18"))
    shapes = [(4, 1, 64, 64)] * 4 + [(2, 1, 64, 64)]
    assert calls == [(s, f) for s in shapes for f in (0, 136)]
    assert tcalls == [(4, 5)] * 4 + [(2, 5)]
    assert len(lp) == 5 and all(math.isfinite(v) for v in lp), lp


def test_cli_ignored_labels_stay_ignored(dev, tmp_path_factory):
    """--uncertain ignore keeps -1 in the targets; under --mixup they meet real labels of the partner row and stay -1, which the
    masked loss skips: finite losses end to end."""
    lu, calls, tcalls = _run(tmp_path_factory, ("--uncertain", "ignore", "--synthetic_uncertain", "0.3", "--mixup", "0.4"))
    assert len(lu) == 4 and all(math.isfinite(v) for v in lu), lu
    assert len(calls) == 4 and len(tcalls) == 4
