"""GPU: the kernels of chexpert_amd/csrc/delong.hip (cx_delong_place, cx_delong_gram) and metrics.delong_auc / delong_auc_diff on top of
them, held to the numpy statement in chexpert_amd/metrics.py.  Everything is integer or bit equality: the host finish is exact, so the
floats of the GPU path equal those of the statement whenever the integers do."""
import json
import os

import numpy as np
import pytest
import torch

from chexpert_amd import metrics as M

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "these tests need the GPU"
    return torch.device("cuda:0")


def _place_case(N, lens, seed):
    """One class per requested length (the other rows of the class ignored), scores with heavy ties; the last two classes keep every
    row: one all positive, one with every score tied."""
    rng = np.random.default_rng(seed)
    C = len(lens) + 2
    s = np.round(rng.normal(size=(N, C)) * 2) / 2
    t = (rng.random((N, C)) < 0.4).astype(np.float64)
    for c, n in enumerate(lens):
        t[rng.permutation(N)[n:], c] = -1.0
    t[:, -2] = 1.0
    s[:, -1] = 0.25
    return s.astype(np.float32), t


def _check_place(dev, plan, n_units, pad=0):
    from chexpert_amd import ops
    want = M.delong_place_reference(plan["order"], plan["offs"], plan["lens"], n_units)
    order = torch.from_numpy(plan["order"]).to(dev)
    if pad:
        out = torch.full((want.shape[0], n_units + pad), -7, dtype=torch.int64, device=dev)
        got = ops.delong_place(order, plan["offs"], plan["lens"], n_units, out=out)
        assert bool((out[:, n_units:] == -7).all())                     # the padding behind the U columns is left untouched
    else:
        got = ops.delong_place(order, plan["offs"], plan["lens"], n_units)
    assert got.dtype == torch.int64 and tuple(got.shape) == want.shape
    assert torch.equal(got.cpu(), torch.from_numpy(want))
    return want


def test_place_equals_the_reference_at_every_boundary(dev):
    from chexpert_amd import ops
    W = ops.DELONG_WG_ENTRIES
    N = 3 * W + 1                                                       # crosses every step boundary of a workgroup's walk
    lens = (1, 63, 64, 65, 257, 0, W - 1, W, W + 1, N)
    s, t = _place_case(N, lens, 3)
    plan = M.bootstrap_plan(s, t)
    assert list(plan["lens"]) == list(lens) + [N, N]
    z = _check_place(dev, plan, N)
    for c in range(len(lens) + 2):                                      # num2 both ways, and the counts
        assert z[4 * c].sum() == z[4 * c + 2].sum() and z[4 * c + 1].sum() + z[4 * c + 3].sum() == plan["lens"][c]
    assert not z[20:24].any()                                           # the class of length 0
    assert z[4 * len(lens) + 3].sum() == 0 and z[4 * len(lens)].sum() == 0          # all rows positive: no negative to be in front of
    # U < N with uneven groups (some of them large), into a table with a pitch above U
    rng = np.random.default_rng(4)
    groups = np.maximum(rng.integers(0, 700, size=N), rng.integers(0, 700, size=N))
    plan = M.bootstrap_plan(s, t, groups)
    assert plan["n_units"] < N
    _check_place(dev, plan, plan["n_units"], pad=5)
    # a unit index above U - 1 is clamped to it
    z = _check_place(dev, plan, plan["n_units"] - 50)
    assert z[-3, -1] + z[-1, -1] == (plan["units"] >= plan["n_units"] - 51).sum() > 51          # (the last class keeps every row)
    # the same bits on every run
    order = torch.from_numpy(plan["order"]).to(dev)
    a, b = (ops.delong_place(order, plan["offs"], plan["lens"], plan["n_units"]) for _ in range(2))
    assert torch.equal(a, b)
    with pytest.raises(ValueError):                                     # lists that do not fit the order array
        ops.delong_place(order[:-1], plan["offs"], plan["lens"], plan["n_units"])


def test_place_70001_rows(dev):
    rng = np.random.default_rng(5)
    N = 70001
    s = (np.round(rng.normal(size=(N, 2)) * 8) / 8).astype(np.float32)
    t = (rng.random((N, 2)) < 0.3).astype(np.float64)
    t[rng.random((N, 2)) < 0.1] = -1.0
    _check_place(dev, M.bootstrap_plan(s, t), N)
    _check_place(dev, M.bootstrap_plan(s, t, rng.integers(0, 20000, size=N)), 20000, pad=3)


@pytest.fixture(scope="module")
def gram_rows():
    rng = np.random.default_rng(6)
    return rng.integers(-(1 << 40), 1 << 40, size=(128, 70001 + 3), dtype=np.int64)     # products of 2^80: the sums wrap


@pytest.mark.parametrize("Q", [4, 12, 128])
def test_gram_equals_the_reference(dev, gram_rows, Q):
    from chexpert_amd import ops
    for U in (1, 63, 64, 65, 1000, 70001):
        z = np.ascontiguousarray(gram_rows[:Q, :U + 3])
        want = M.int_gram_reference(z, U)
        got = ops.int_gram(torch.from_numpy(z).to(dev), U)              # a pitch above U: the columns behind it are not read
        assert got.dtype == torch.int64 and tuple(got.shape) == (Q, Q)
        assert torch.equal(got.cpu(), torch.from_numpy(want)), (Q, U)
        assert torch.equal(got, got.t())
    zt = torch.from_numpy(np.ascontiguousarray(gram_rows[:Q, :1000])).to(dev)
    assert torch.equal(ops.int_gram(zt, 1000), ops.int_gram(zt, 1000))  # the same bits on every run
    with pytest.raises(ValueError):
        ops.int_gram(torch.zeros(129, 4, dtype=torch.int64, device=dev), 4)


def _model_case(dtype, seed):
    g = torch.Generator().manual_seed(seed)
    t = (torch.rand(500, 5, generator=g) < 0.35).float()
    a = (t + torch.randn(500, 5, generator=g)).to(dtype)
    b = (0.7 * t + torch.randn(500, 5, generator=g)).to(dtype)
    t[torch.rand(500, 5, generator=g) < 0.1] = -1.0
    t[:, 4] = torch.where(t[:, 4] > 0.5, torch.zeros(()), t[:, 4])       # class 4 has no positive: NaN in the same places
    groups = np.random.default_rng(seed).integers(0, 180, size=500)
    return a, b, t, groups


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float32])
def test_end_to_end_equals_the_reference_float_for_float(dev, dtype):
    a, b, t, groups = _model_case(dtype, 7)
    for g in (None, groups):
        want = M.delong_auc_reference(a, t, groups=g)
        got = M.delong_auc(a.to(dev), t.to(dev), groups=g, device=dev)
        assert json.dumps(got, sort_keys=True) == json.dumps(want, sort_keys=True)          # repr round-trips: equal bits, equal NaNs
        assert got["method"] == ("delong" if g is None else "obuchowski") and np.isnan(got["aucs"][4]) and got["se"][0] > 0
        assert set(got) == {"aucs", "se", "lo", "hi", "n_pos", "n_neg", "n_units_pos", "n_units_neg", "mean_auc", "alpha", "n_units", "method"}
        want = M.delong_auc_diff_reference(a, b, t, groups=g, alpha=0.1)
        got = M.delong_auc_diff(a.to(dev), b.to(dev), t.to(dev), groups=g, alpha=0.1, device=dev)
        assert json.dumps(got, sort_keys=True) == json.dumps(want, sort_keys=True)
        assert 0.0 < got["p"][0] <= 1.0 and got["degenerate"][0] is False and np.isnan(got["p"][4])
        assert set(got["mean_auc"]) == {"delta", "se", "lo", "hi", "z", "p"}
        again = M.delong_auc_diff(a.to(dev), b.to(dev), t.to(dev), groups=g, alpha=0.1, device=dev)
        assert json.dumps(again, sort_keys=True) == json.dumps(got, sort_keys=True)         # two calls, the same bits
    same = M.delong_auc_diff(a[:, :4].to(dev), a[:, :4].clone().to(dev), t[:, :4].to(dev), device=dev)
    assert all(same["degenerate"].values()) and same["mean_auc"]["delta"] == 0.0 and np.isnan(same["mean_auc"]["p"])


def test_write_delong_writes_the_named_file(dev, tmp_path):
    from chexpert_amd import cli
    a, b, t, groups = _model_case(torch.float32, 8)
    args = cli.parse_args(["--evaluate_single_model", "--delong", "--bootstrap_alpha", "0.1", "--output_dir", str(tmp_path)])
    path = cli.write_delong(args, "eval_results_step_7", a[:, :4], t[:, :4])
    assert path == os.path.join(str(tmp_path), "delong_step_7.json") and os.listdir(tmp_path) == ["delong_step_7.json"]
    got = json.load(open(path))
    want = M.delong_auc_reference(a[:, :4], t[:, :4], alpha=0.1)
    assert got["alpha"] == 0.1 and got["unit"] == "image" and got["method"] == "delong" and "vs_members" not in got
    assert {int(k): v for k, v in got["aucs"].items()} == want["aucs"] and {int(k): v for k, v in got["se"].items()} == want["se"]
    assert got["mean_auc"] == want["mean_auc"]
    # the ensemble: the paired test of the mean logits against every member, keyed by the checkpoint's file name
    mean = torch.stack([a, b], 2).mean(2)[:, :4]
    path = cli.write_delong(args, "eval_results_ensemble", mean, t[:, :4], groups, members={"checkpoint_1.pt": a[:, :4], "checkpoint_2.pt": b[:, :4]})
    got = json.load(open(path))
    assert os.path.basename(path) == "delong_ensemble.json" and got["method"] == "obuchowski" and sorted(got["vs_members"]) == ["checkpoint_1.pt", "checkpoint_2.pt"]
    want = M.delong_auc_diff_reference(mean, b[:, :4], t[:, :4], groups=groups, alpha=0.1)
    assert got["vs_members"]["checkpoint_2.pt"]["mean_auc"] == want["mean_auc"]
    assert {int(k): v for k, v in got["vs_members"]["checkpoint_2.pt"]["p"].items()} == want["p"]
