"""GPU: the kernels of chexpert_amd/csrc/bootstrap.hip (cx_boot_counts, cx_boot_auc) and metrics.bootstrap_auc / bootstrap_auc_diff on top of
them, held to the numpy statement in chexpert_amd/metrics.py.  Everything is integer or bit equality; the one tolerance is the derived
N * 2^-52 between the integer AUROC and metrics.roc_curve / metrics.auc (tests/test_bootstrap_cpu.py derives it)."""
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


def test_counts_equal_the_reference_at_every_tile_boundary(dev):
    from chexpert_amd import ops
    T, K = ops.BOOT_TILE, ops.BOOT_MAX_TILES
    seed = 0x9E3779B97F4A7C15 ^ 12345                                   # != 0, above 2^63: the seed is an unsigned 64-bit value
    # one tile; one below, at and one above the tile; the last size of the LDS form and the first of the device-memory form
    for U in (1, 2, 63, 64, 65, 257, T - 1, T, T + 1, K * T, K * T + 1):
        want = M.bootstrap_counts_reference(U, 3, seed)
        got = ops.boot_counts(U, 3, seed, device=dev)
        assert got.dtype == torch.int32 and tuple(got.shape) == (3, U)
        assert torch.equal(got.cpu(), torch.from_numpy(want.view(np.int32))), U
        assert (want.sum(1) == U).all()
    # a replicate depends on its index, not on the call that computes it
    for U in (257, T + 1, K * T + 1):
        full = ops.boot_counts(U, 8, seed, device=dev)
        assert torch.equal(ops.boot_counts(U, 3, seed, first=5, device=dev), full[5:])
        out = torch.full((4, U), -1, dtype=torch.int32, device=dev)     # into the first rows of a larger table; the rest untouched
        assert torch.equal(ops.boot_counts(U, 3, seed, first=5, out=out), full[5:]) and bool((out[3] == -1).all())
    assert torch.equal(ops.boot_counts(257, 8, seed, device=dev), ops.boot_counts(257, 8, seed, device=dev))
    assert not torch.equal(ops.boot_counts(257, 8, seed + 1, device=dev), ops.boot_counts(257, 8, seed, device=dev))
    with pytest.raises(RuntimeError):
        ops.boot_counts((1 << 24) + 1, 1, 0, out=torch.empty(1, (1 << 24) + 1, dtype=torch.int32, device=dev))


def _scan_case(lens, seed, n_units):
    """Scores with heavy ties, one class per requested length (the other rows of the class ignored), the second class all positive,
    rows grouped into n_units units with several rows per unit."""
    rng = np.random.default_rng(seed)
    N = max(max(lens), 2 * n_units)
    s = np.round(rng.normal(size=(N, len(lens))) * 2) / 2
    s[:, -1] = rng.normal(size=N)                                       # ... and one class without ties
    t = (rng.random((N, len(lens))) < 0.4).astype(np.float64)
    t[:, 1] = 1.0
    for c, n in enumerate(lens):
        t[rng.permutation(N)[n:], c] = -1.0
    groups = rng.permutation(N) % n_units
    return s, t, groups


@pytest.mark.parametrize("lens", [(0, 1, 65, 1000), (63, 64, 129, 257)])
def test_scan_equals_the_reference(dev, lens):
    from chexpert_amd import ops
    U = 300
    s, t, groups = _scan_case(lens, sum(lens), U)
    plan = M.bootstrap_plan(s, t, groups)
    assert tuple(plan["lens"]) == lens and plan["n_units"] == U
    rng = np.random.default_rng(7)
    counts = rng.integers(0, 4001, size=(6, U)).astype(np.uint32)       # hand-made: up to 4000 per unit, a third of them zero
    counts[rng.random((6, U)) < 0.33] = 0
    counts[3] = 4000                                                    # W = 4e6 over 1000 rows, num2 of the order of 1e13
    counts[4] = 1                                                       # the data set itself
    counts[5] = 0
    counts[5, ::7] = 4000
    want = M.bootstrap_scan_reference(counts, plan["order"], plan["offs"], plan["lens"], U)
    if max(lens) == 1000:                                               # the 64-bit sum and the 32-bit carry across steps are exercised
        assert int(want[0].max()) > 1 << 40 and int(want[2].max()) > 1 << 20 and int((want[1] + want[2]).max()) == 4000 * 1000
    got = ops.boot_auc(torch.from_numpy(counts.view(np.int32)).to(dev), torch.from_numpy(plan["order"]).to(dev), plan["offs"], plan["lens"], U)
    for g, w in zip(got, want):
        assert g.dtype == torch.int64 and tuple(g.shape) == (6, len(lens))
        assert torch.equal(g.cpu(), torch.from_numpy(w.astype(np.int64)))
    # the same integers straight from the definition (no prepared orders)
    for g, w in zip(got, M._definition_parts(s, t, plan["units"], counts)):
        assert torch.equal(g.cpu(), torch.from_numpy(w))
    assert bool((got[2][:, 1] == 0).all())                              # the all-positive class: no negative weight, no AUROC
    # the row of ones is the AUROC of compute_metrics
    auc = M._auc_of(*(v.cpu().numpy() for v in got))[4]
    ref = M.compute_metrics(s, t, np.zeros_like(s))["aucs"]
    for c, n in enumerate(lens):
        if np.isnan(ref[c]):
            assert np.isnan(auc[c])
        else:
            assert abs(auc[c] - ref[c]) <= n * 2.0 ** -52, (c, auc[c], ref[c])
    # unit indices past n_units are clamped, never trusted: a smaller n_units reads the last unit's count instead
    small = ops.boot_auc(torch.from_numpy(counts.view(np.int32)).to(dev), torch.from_numpy(plan["order"]).to(dev), plan["offs"], plan["lens"], 200)
    for g, w in zip(small, M.bootstrap_scan_reference(counts, plan["order"], plan["offs"], plan["lens"], 200)):
        assert torch.equal(g.cpu(), torch.from_numpy(w.astype(np.int64)))
    with pytest.raises(ValueError):
        ops.boot_auc(torch.from_numpy(counts.view(np.int32)).to(dev), torch.from_numpy(plan["order"][:-1].copy()).to(dev), plan["offs"], plan["lens"], U)


def test_scan_more_classes_than_one_launch_holds(dev):
    """40 classes: the scan stage passes offsets and lengths as kernel arguments, 32 classes per launch."""
    from chexpert_amd import ops
    rng = np.random.default_rng(40)
    s = np.round(rng.normal(size=(70, 40)) * 2) / 2
    t = (rng.random((70, 40)) < 0.5).astype(np.float64)
    t[rng.random((70, 40)) < 0.2] = -1.0
    plan = M.bootstrap_plan(s, t)
    counts = M.bootstrap_counts_reference(70, 5, 3)
    got = ops.boot_auc(torch.from_numpy(counts.view(np.int32)).to(dev), torch.from_numpy(plan["order"]).to(dev), plan["offs"], plan["lens"], 70)
    for g, w in zip(got, M.bootstrap_scan_reference(counts, plan["order"], plan["offs"], plan["lens"], 70)):
        assert torch.equal(g.cpu(), torch.from_numpy(w.astype(np.int64)))


def _same(a, b):
    assert a.keys() == b.keys()
    for k in a:
        if isinstance(a[k], dict):
            assert a[k].keys() == b[k].keys(), k
            assert np.array_equal(np.array(list(a[k].values()), dtype=np.float64), np.array(list(b[k].values()), dtype=np.float64),
                                  equal_nan=True), k
        elif isinstance(a[k], np.ndarray):
            assert np.array_equal(a[k], b[k], equal_nan=True), k
        else:
            assert a[k] == b[k], k


@pytest.fixture(scope="module")
def e2e():
    rng = np.random.default_rng(234)
    N, C = 234, 5
    t = (rng.random((N, C)) < 0.3).astype(np.float32)
    s = (rng.normal(size=(N, C)) + 1.2 * t).astype(np.float32)
    s[:, 1] = np.round(s[:, 1])                                         # one class with heavy ties
    t[:3, 2], t[3:, 2] = 1.0, 0.0                                       # three positives: some replicates draw none
    t[rng.random((N, C)) < 0.1] = -1.0                                  # 10 % of the labels ignored
    ref = M.bootstrap_auc_reference(s, t, n_boot=200, seed=11, return_replicates=True)
    return s, t, ref


def test_end_to_end_equals_the_reference(dev, e2e):
    s, t, ref = e2e
    got = M.bootstrap_auc(s, t, n_boot=200, seed=11, device=dev, return_replicates=True)
    _same(got, ref)
    assert 0 < ref["n_degenerate"][2] < 200 and np.isnan(got["replicates"][:, 2]).sum() == ref["n_degenerate"][2]
    _same(M.bootstrap_auc(s, t, n_boot=200, seed=11, device=dev, return_replicates=True), got)          # two calls: the same bits
    _same(M.bootstrap_auc(s, t, n_boot=200, seed=11, device=dev, chunk=7, return_replicates=True), got)
    other = M.bootstrap_auc(torch.from_numpy(s), torch.from_numpy(t), n_boot=200, seed=12, device=dev, return_replicates=True)
    assert other["aucs"] == got["aucs"] and not np.array_equal(other["replicates"], got["replicates"], equal_nan=True)
    for c in range(5):
        assert got["n_degenerate"][c] < 200
        assert np.isfinite(got["lo"][c]) and np.isfinite(got["hi"][c]) and got["lo"][c] <= got["hi"][c]
    assert np.isfinite(got["mean_auc"]["lo"]) and got["mean_auc"]["lo"] <= got["mean_auc"]["hi"]
    json.dumps({k: v for k, v in got.items() if k != "replicates"})
    aucs = M.compute_metrics(s, t, np.zeros_like(s))["aucs"]
    for c in range(5):
        assert abs(got["aucs"][c] - aucs[c]) <= 234 * 2.0 ** -52
    # resampling by patient: three images per patient
    groups = np.array(["patient%d" % (i // 3) for i in range(234)])
    _same(M.bootstrap_auc(s, t, n_boot=50, seed=3, groups=groups, device=dev, return_replicates=True),
          M.bootstrap_auc_reference(s, t, n_boot=50, seed=3, groups=groups, return_replicates=True))
    with pytest.raises(RuntimeError):                                   # the GPU or nothing
        M.bootstrap_auc(s, t, n_boot=10, device="cpu")


def test_paired_difference(dev, e2e):
    s, t, _ = e2e
    r = M.bootstrap_auc_diff(s, s, t, n_boot=100, seed=5, device=dev)
    for c in range(5):
        assert (r["delta"][c], r["lo"][c], r["hi"][c], r["p"][c]) == (0.0, 0.0, 0.0, 1.0)
    assert (r["mean_auc"]["delta"], r["mean_auc"]["lo"], r["mean_auc"]["hi"], r["mean_auc"]["p"]) == (0.0, 0.0, 0.0, 1.0)
    s2 = (s + 0.7 * np.random.default_rng(1).normal(size=s.shape)).astype(np.float32)
    _same(M.bootstrap_auc_diff(s, s2, t, n_boot=100, seed=5, device=dev, chunk=33, return_replicates=True),
          M.bootstrap_auc_diff_reference(s, s2, t, n_boot=100, seed=5, return_replicates=True))


def test_cli_writes_the_intervals_and_leaves_the_results_alone(dev, tmp_path, capsys):
    from chexpert_amd import cli
    base = ["--evaluate", "--synthetic", "64", "--batch_size", "4", "--resize", "64", "--seed", "3"]
    cli.main(base + ["--output_dir", str(tmp_path / "a")])
    capsys.readouterr()
    cli.main(base + ["--bootstrap", "50", "--output_dir", str(tmp_path / "b")])
    out = capsys.readouterr().out
    assert sorted(f for f in os.listdir(tmp_path / "a") if f.endswith(".json")) == ["config.json", "eval_results_step_0.json"]
    assert sorted(f for f in os.listdir(tmp_path / "b") if f.endswith(".json")) == ["auc_ci_step_0.json", "config.json", "eval_results_step_0.json"]
    assert open(tmp_path / "a" / "eval_results_step_0.json", "rb").read() == open(tmp_path / "b" / "eval_results_step_0.json", "rb").read()
    ci = json.load(open(tmp_path / "b" / "auc_ci_step_0.json"))
    assert set(ci) == {"aucs", "lo", "hi", "se", "n_degenerate", "mean_auc", "n_boot", "seed", "alpha", "n_units", "unit"}
    assert set(ci["mean_auc"]) == {"point", "lo", "hi", "se"} and set(ci["aucs"]) == {"0", "1", "2", "3", "4"}
    assert (ci["n_boot"], ci["seed"], ci["alpha"], ci["n_units"], ci["unit"]) == (50, 3, 0.05, 12, "image")
    res = json.load(open(tmp_path / "b" / "eval_results_step_0.json"))
    for c in "01234":
        if res["aucs"][c] == res["aucs"][c]:
            assert abs(ci["aucs"][c] - res["aucs"][c]) <= 12 * 2.0 ** -52
    assert "bootstrap intervals" in out and out.count("[") >= 6
