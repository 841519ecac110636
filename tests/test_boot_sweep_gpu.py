"""GPU: the kernel cx_boot_sweep of chexpert_amd/csrc/bootstrap.hip and metrics.bootstrap_metrics / bootstrap_metrics_diff on top of it,
held to the numpy statement in chexpert_amd/metrics.py (bootstrap_sweep_reference, which tests/test_boot_sweep_cpu.py pins to the
definition and to the float curves).  Everything here is integer or bit equality."""
import json
import os

import numpy as np
import pytest
import torch

from chexpert_amd import metrics as M

pytestmark = pytest.mark.gpu

POINTS8 = [(M.BOOT_SENS, 900000), (M.BOOT_SPEC, 900000), (M.BOOT_SENS, 1), (M.BOOT_SPEC, 1), (M.BOOT_SENS, 999999), (M.BOOT_SPEC, 999999),
           (M.BOOT_SENS, 500000), (M.BOOT_SPEC, 123456)]


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "these tests need the GPU"
    return torch.device("cuda:0")


def _sweep_case(lens, seed, n_units):
    """One class per requested length (the other rows of the class ignored), the second class all positive, rows grouped into n_units
    units with several rows per unit.  The scores of a class fall with the position in its sweep, tied in runs of 1, 2 or 3, and the
    positions 60 .. 69 and 250 .. 261 share one score each: a tie group across the 64-lane step and one across the 256-entry block."""
    rng = np.random.default_rng(seed)
    N = max(max(lens), 2 * n_units)
    s = rng.normal(size=(N, len(lens)))
    t = (rng.random((N, len(lens))) < 0.4).astype(np.float64)
    t[:, 1] = 1.0
    for c, n in enumerate(lens):
        rows = rng.permutation(N)
        t[rows[n:], c] = -1.0
        pos = (np.arange(n) // (1 + c % 3)).astype(np.float64)
        for a, b in ((60, 70), (250, 262)):
            pos[a:b] = pos[a] if n > a else 0.0
        s[rows[:n], c] = -pos
    groups = rng.permutation(N) % n_units
    return s, t, groups


def _hand_counts(U):
    rng = np.random.default_rng(7)
    counts = rng.integers(0, 4001, size=(6, U)).astype(np.uint32)       # hand-made: up to 4000 per unit, a third of them zero
    counts[rng.random((6, U)) < 0.33] = 0
    counts[3] = 4000                                                    # W = 4e6 over 1000 rows, apnum of the order of 2^51
    counts[4] = 1                                                       # the data set itself
    counts[5] = 0
    counts[5, ::7] = 4000
    return counts


def _equal(got, want, n_pts):
    for g, w in zip(got, want):
        assert g.dtype == torch.int64 and tuple(g.shape) == w.shape
        assert torch.equal(g.cpu(), torch.from_numpy(w.view(np.int64))), (n_pts, g.cpu().numpy(), w)


@pytest.mark.parametrize("lens", [(0, 1, 65, 1000), (63, 64, 129, 257)])
def test_sweep_equals_the_statement(dev, lens):
    from chexpert_amd import ops
    U = 300
    s, t, groups = _sweep_case(lens, sum(lens), U)
    plan = M.bootstrap_sweep_plan(s, t, groups)
    assert tuple(plan["lens"]) == lens and plan["n_units"] == U
    for c, n in enumerate(lens):                                        # the constructed tie groups do straddle the boundaries
        e = plan["order"][plan["offs"][c]:plan["offs"][c] + n]
        assert n <= 64 or not e[63] & 0x40000000
        assert n <= 256 or not e[255] & 0x40000000
    counts = _hand_counts(U)
    d_counts, d_order = torch.from_numpy(counts.view(np.int32)).to(dev), torch.from_numpy(plan["order"]).to(dev)
    for points in ([], POINTS8[:1], POINTS8):                           # 0, 1 and 8 operating points
        want = M.bootstrap_sweep_reference(counts, plan["order"], plan["offs"], plan["lens"], U, points)
        if max(lens) == 1000:                                           # the 64-bit sum and the 32-bit carries across steps are exercised
            assert int(want[0].max()) > 1 << 50 and int((want[1] + want[2]).max()) == 4000 * 1000
            assert len(points) < 8 or int(want[3].max()) > 1 << 20
        got = ops.boot_sweep(d_counts, d_order, plan["offs"], plan["lens"], U, points)
        assert tuple(got[3].shape) == (6, len(lens), len(points))
        _equal(got, want, len(points))
    # the all-positive class: no negative weight, AP = 1 wherever a positive was drawn
    val = M._sweep_values(("ap",), [], got[0].cpu().numpy().view(np.uint64), got[1].cpu().numpy(), got[2].cpu().numpy(), None)["ap"]
    some = got[1][:, 1].cpu().numpy() > 0
    assert bool((got[2][:, 1] == 0).all()) and some[3] and (val[some, 1] == 1.0).all() and np.isnan(val[~some, 1]).all()
    # unit indices past n_units are clamped, never trusted: a smaller n_units reads the last unit's count instead
    small = ops.boot_sweep(d_counts, d_order, plan["offs"], plan["lens"], 200, POINTS8)
    _equal(small, M.bootstrap_sweep_reference(counts, plan["order"], plan["offs"], plan["lens"], 200, POINTS8), 8)
    assert not torch.equal(small[0], got[0])
    with pytest.raises(ValueError):
        ops.boot_sweep(d_counts, torch.from_numpy(plan["order"][:-1].copy()).to(dev), plan["offs"], plan["lens"], U)
    with pytest.raises(ValueError):
        ops.boot_sweep(d_counts, d_order, plan["offs"], plan["lens"], U, POINTS8 + POINTS8[:1])
    with pytest.raises(ValueError):
        ops.boot_sweep(d_counts, d_order, plan["offs"], plan["lens"], U, [(M.BOOT_SENS, 0)])


def test_sweep_more_classes_than_one_launch_holds(dev):
    """40 classes: offsets and lengths travel as kernel arguments, 32 classes per launch."""
    from chexpert_amd import ops
    rng = np.random.default_rng(40)
    s = np.round(rng.normal(size=(70, 40)) * 2) / 2
    t = (rng.random((70, 40)) < 0.5).astype(np.float64)
    t[rng.random((70, 40)) < 0.2] = -1.0
    plan = M.bootstrap_sweep_plan(s, t)
    counts = M.bootstrap_counts_reference(70, 5, 3)
    got = ops.boot_sweep(torch.from_numpy(counts.view(np.int32)).to(dev), torch.from_numpy(plan["order"]).to(dev), plan["offs"], plan["lens"],
                         70, POINTS8[:3])
    _equal(got, M.bootstrap_sweep_reference(counts, plan["order"], plan["offs"], plan["lens"], 70, POINTS8[:3]), 3)


def _same(a, b):
    assert a.keys() == b.keys()
    for k in a:
        if isinstance(a[k], dict) and any(isinstance(v, dict) for v in a[k].values()):
            _same(a[k], b[k])                                           # {metric: summary}
        elif isinstance(a[k], dict):
            assert a[k].keys() == b[k].keys(), k
            assert np.array_equal(np.array(list(a[k].values()), dtype=np.float64), np.array(list(b[k].values()), dtype=np.float64),
                                  equal_nan=True), k
        elif isinstance(a[k], np.ndarray):
            assert np.array_equal(a[k], b[k], equal_nan=True), k
        else:
            assert a[k] == b[k], k


NAMES = ("auroc", "ap", "sens@0.9", "spec@0.9", "sens@0.5")


@pytest.fixture(scope="module")
def e2e():
    rng = np.random.default_rng(150)
    N, C = 150, 3
    t = (rng.random((N, C)) < 0.3).astype(np.float32)                   # about 45 positives per class: no replicate is degenerate
    s = (rng.normal(size=(N, C)) + 1.2 * t).astype(np.float32)
    s[:, 1] = np.round(s[:, 1])                                         # one class with heavy ties
    t[rng.random((N, C)) < 0.1] = -1.0                                  # 10 % of the labels ignored
    groups = np.array(["patient%d" % (i // 3) for i in range(N)])
    ref = {g is None: M.bootstrap_metrics_reference(s, t, NAMES, n_boot=64, seed=11, groups=g, return_replicates=True) for g in (None, groups)}
    return s, t, groups, ref


@pytest.mark.parametrize("grouped", [False, True])
def test_end_to_end_equals_the_reference(dev, e2e, grouped):
    s, t, groups, ref = e2e
    g, ref = (groups if grouped else None), ref[not grouped]
    got = M.bootstrap_metrics(s, t, NAMES, n_boot=64, seed=11, groups=g, device=dev, return_replicates=True)
    assert list(got) == list(NAMES)
    _same(got, ref)
    for name in NAMES:
        assert got[name]["n_degenerate"] == {0: 0, 1: 0, 2: 0} and got[name]["n_units"] == (50 if grouped else 150)
        assert np.isfinite(got[name]["replicates"]).all() and got[name]["replicates"].shape == (64, 3)
        assert all(got[name]["lo"][c] <= got[name]["hi"][c] for c in range(3))
        json.dumps({k: v for k, v in got[name].items() if k != "replicates"})
    _same(M.bootstrap_metrics(s, t, NAMES, n_boot=64, seed=11, groups=g, device=dev, return_replicates=True), got)       # the same bits
    for chunk in (7, 64):                                                                        # the chunking does not show
        _same(M.bootstrap_metrics(torch.from_numpy(s), torch.from_numpy(t), NAMES, n_boot=64, seed=11, groups=g, device=dev, chunk=chunk,
                                  return_replicates=True), got)
    auc = M.bootstrap_auc(s, t, n_boot=64, seed=11, groups=g, device=dev, return_replicates=True)
    assert set(got["auroc"]) - {"point"} == set(auc) - {"aucs"}
    _same({("aucs" if k == "point" else k): v for k, v in got["auroc"].items()}, auc)
    other = M.bootstrap_metrics(s, t, ("ap",), n_boot=64, seed=12, groups=g, device=dev, return_replicates=True)["ap"]
    assert other["point"] == got["ap"]["point"] and not np.array_equal(other["replicates"], got["ap"]["replicates"])
    with pytest.raises(RuntimeError):                                   # the GPU or nothing
        M.bootstrap_metrics(s, t, ("ap",), n_boot=4, device="cpu")
    with pytest.raises(ValueError):
        M.bootstrap_metrics(s, t, ("sens@1.5",), n_boot=4, device=dev)


def test_paired_difference(dev, e2e):
    s, t, groups, _ = e2e
    r = M.bootstrap_metrics_diff(s, s, t, NAMES, n_boot=64, seed=5, device=dev)
    for m in r.values():
        for c in range(3):
            assert (m["delta"][c], m["lo"][c], m["hi"][c], m["p"][c]) == (0.0, 0.0, 0.0, 1.0)
        assert (m["mean_auc"]["delta"], m["mean_auc"]["lo"], m["mean_auc"]["hi"], m["mean_auc"]["p"]) == (0.0, 0.0, 0.0, 1.0)
    s2 = (s + 0.7 * np.random.default_rng(1).normal(size=s.shape)).astype(np.float32)
    _same(M.bootstrap_metrics_diff(s, s2, t, NAMES, n_boot=64, seed=5, groups=groups, device=dev, chunk=33, return_replicates=True),
          M.bootstrap_metrics_diff_reference(s, s2, t, NAMES, n_boot=64, seed=5, groups=groups, return_replicates=True))


def test_cli_writes_the_metric_intervals_and_leaves_the_auroc_file_alone(dev, tmp_path, capsys, monkeypatch):
    from chexpert_amd import cli
    seen, inner = [], cli.write_metrics_ci

    def spy(args, tag, outputs, targets, groups=None):
        seen.append((np.array(M._as_scores(outputs)), np.array(M._as_scores(targets)), groups))
        return inner(args, tag, outputs, targets, groups)
    monkeypatch.setattr(cli, "write_metrics_ci", spy)
    base = ["--evaluate_single_model", "--synthetic", "64", "--batch_size", "4", "--resize", "64", "--seed", "3", "--bootstrap", "20"]
    cli.main(base + ["--output_dir", str(tmp_path / "a")])
    assert "mean over the classes" not in capsys.readouterr().out
    cli.main(base + ["--bootstrap_metrics", "ap", "sens@0.9", "--output_dir", str(tmp_path / "b")])
    out = capsys.readouterr().out
    assert sorted(f for f in os.listdir(tmp_path / "a") if f.endswith(".json")) == ["auc_ci_step_0.json", "config.json", "eval_results_step_0.json"]
    assert sorted(f for f in os.listdir(tmp_path / "b") if f.endswith(".json")) == ["auc_ci_step_0.json", "config.json", "eval_results_step_0.json",
                                                                                   "metrics_ci_step_0.json"]
    for name in ("auc_ci_step_0.json", "eval_results_step_0.json"):
        assert open(tmp_path / "a" / name, "rb").read() == open(tmp_path / "b" / name, "rb").read()
    assert json.load(open(tmp_path / "b" / "config.json"))["bootstrap_metrics"] == ["ap", "sens@0.9"]
    ci = json.load(open(tmp_path / "b" / "metrics_ci_step_0.json"))
    assert list(ci) == ["ap", "sens@0.9"] and len(seen) == 2 and seen[1][2] is None
    ref = M.bootstrap_metrics_reference(seen[1][0], seen[1][1], ("ap", "sens@0.9"), n_boot=20, seed=3)
    for name in ci:
        assert set(ci[name]) == {"point", "lo", "hi", "se", "n_degenerate", "mean_auc", "n_boot", "seed", "alpha", "n_units", "unit"}
        assert (ci[name]["n_boot"], ci[name]["seed"], ci[name]["alpha"], ci[name]["n_units"], ci[name].pop("unit")) == (20, 3, 0.05, 12, "image")
        _same(ci[name], json.loads(json.dumps(ref[name])))
        assert ("%s, mean over the classes" % name) in out
