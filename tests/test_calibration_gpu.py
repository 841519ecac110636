"""GPU: the kernels of chexpert_amd/csrc/calib.hip.  cx_boot_calib and calibration_metrics are held to the numpy statement in
chexpert_amd/calibration.py bit for bit (integers, then floats formed by one shared function); cx_calib_fit to the reference Newton
iteration within the distance two stopping points of one strictly convex problem can have."""
import json
import os

import numpy as np
import pytest
import torch

from chexpert_amd import calibration as K
from chexpert_amd import metrics as M

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "these tests need the GPU"
    return torch.device("cuda:0")


def _hand_counts(U):
    rng = np.random.default_rng(7)
    counts = rng.integers(0, 4001, size=(6, U)).astype(np.uint32)       # hand-made: up to 4000 per unit, a third of them zero
    counts[rng.random((6, U)) < 0.33] = 0
    counts[3] = 4000                                                    # W = 4e6 over 1000 rows
    counts[4] = 1                                                       # the data set itself
    counts[5] = 0
    counts[5, ::7] = 4000
    return counts


def _case(lens, seed, n_units):
    """One class per requested length (the other rows of the class ignored), the second class all positive, rows grouped into n_units
    units with several rows per unit; logits rounded to two decimals (ties), and +-800 (P = 2^32 - 1 and P = 0) where a class has room."""
    rng = np.random.default_rng(seed)
    N = max(max(lens), 2 * n_units)
    z = np.round(rng.normal(0.0, 2.5, (N, len(lens))), 2).astype(np.float32)
    t = (rng.random((N, len(lens))) < 0.4).astype(np.float32)
    t[:, 1] = 1.0
    for c, n in enumerate(lens):
        rows = rng.permutation(N)
        t[rows[n:], c] = -1.0
        if n >= 2:
            z[rows[0], c], z[rows[1], c] = 800.0, -800.0
    return z, t, rng.permutation(N) % n_units


def _run(dev, plan, counts, n_units=None):
    from chexpert_amd import ops
    U = plan["n_units"] if n_units is None else n_units
    return ops.boot_calib(torch.from_numpy(counts.view(np.int32)).to(dev), torch.from_numpy(plan["order"]).to(dev),
                          torch.from_numpy(plan["conf"].view(np.int32)).to(dev), plan["offs"], plan["lens"], U, plan["bins"])


def _equal(got, want):
    for g, w in zip(got, want):
        assert g.dtype == torch.int64 and tuple(g.shape) == w.shape
        assert torch.equal(g.cpu(), torch.from_numpy(w.view(np.int64))), (g.cpu().numpy(), w)


@pytest.mark.parametrize("binning", K.BINNINGS)
@pytest.mark.parametrize("bins", (1, 15, 64))
@pytest.mark.parametrize("lens", ((0, 1, 63, 64), (65, 129, 257, 1000)))
def test_boot_calib_equals_the_statement(dev, lens, bins, binning):
    U = 300
    z, t, groups = _case(lens, 3, U)
    plan = K.calibration_plan(z, t, groups, None, bins, binning)
    assert plan["n_units"] == U and tuple(plan["lens"]) == lens
    counts = _hand_counts(U)
    want = K.calibration_sums_reference(counts, plan)
    if max(lens) == 1000:                                               # the 64-bit paths are exercised
        assert int(want[3].max()) > 1 << 40 and int(want[0].sum(axis=2).max()) == 4000 * 1000
        assert bins > 1 or int(want[2].max()) > 1 << 50
    got = _run(dev, plan, counts)
    assert tuple(got[0].shape) == (6, len(lens), bins) and tuple(got[3].shape) == (6, len(lens))
    _equal(got, want)
    if min(lens) == 0:                                                  # a class without rows gives zeros
        assert all(int(g[:, 0].abs().sum()) == 0 for g in got)
    assert torch.equal(got[0][:, 1], got[1][:, 1])                      # the all-positive class
    # unit indices past n_units are clamped, never trusted: a smaller n_units reads the last unit's count instead
    small = _run(dev, plan, counts, n_units=U // 2)
    _equal(small, K.calibration_sums_reference(counts, plan, n_units=U // 2))
    assert not torch.equal(small[0], got[0])


def test_boot_calib_more_classes_than_one_launch_holds(dev):
    rng = np.random.default_rng(5)
    z = rng.normal(0.0, 2.0, (70, 40)).astype(np.float32)
    t = (rng.random((70, 40)) < 0.5).astype(np.float32)
    plan = K.calibration_plan(z, t, None, None, 15, "mass")
    counts = _hand_counts(70)
    got = _run(dev, plan, counts)
    _equal(got, K.calibration_sums_reference(counts, plan))
    assert int((got[0].sum(dim=2)[4] == 70).sum()) == 40                # the row of ones: every class weighs its 70 rows


def test_boot_calib_refuses_bad_arguments_before_any_launch(dev, monkeypatch):
    from chexpert_amd import ops
    z, t, groups = _case((5, 9), 1, 8)
    plan = K.calibration_plan(z, t, groups, None, 15, "width")
    counts = torch.ones(2, plan["n_units"], dtype=torch.int32, device=dev)
    order, conf = torch.from_numpy(plan["order"]).to(dev), torch.from_numpy(plan["conf"].view(np.int32)).to(dev)
    monkeypatch.setattr(ops, "lib", lambda: pytest.fail("a refused call reached the library"))
    for bad in (dict(lens=[5, 10]), dict(offs=[0, 6]), dict(offs=[-1, 5]), dict(bins=0), dict(bins=65), dict(conf=conf[:-1])):
        kw = dict(conf=conf, offs=plan["offs"], lens=plan["lens"], bins=15)
        kw.update(bad)
        with pytest.raises(ValueError, match="boot_calib"):
            ops.boot_calib(counts, order, kw["conf"], kw["offs"], kw["lens"], plan["n_units"], kw["bins"])


def _same(a, b):
    assert a.keys() == b.keys()
    for k in a:
        if isinstance(a[k], dict):
            _same(a[k], b[k])
        elif isinstance(a[k], np.ndarray):
            assert np.array_equal(a[k], b[k], equal_nan=True), k
        elif isinstance(a[k], list):
            assert np.array_equal(np.array(a[k], dtype=np.float64), np.array(b[k], dtype=np.float64), equal_nan=True), k
        else:
            assert a[k] == b[k] or (a[k] != a[k] and b[k] != b[k]), k


def test_calibration_metrics_equal_the_reference_on_every_float(dev):
    from chexpert_amd import ops
    z, t, groups = _case((150, 150, 97, 0), 11, 40)
    cal = K.fit_calibration_reference(z, t, "platt", smooth=True)
    for g, c, binning in ((None, None, "width"), (groups, cal, "mass")):
        want = K.calibration_metrics_reference(z, t, c, 15, binning, n_boot=64, seed=9, groups=g, return_replicates=True)
        for chunk in (7, None):
            got = K.calibration_metrics(z, t, c, 15, binning, n_boot=64, seed=9, groups=g, device=dev, chunk=chunk, return_replicates=True)
            _same(got, want)
        assert set(got) == {"ece", "mce", "brier", "reliability", "replicate_weights"} and got["ece"]["replicates"].shape == (64, 4)
        assert np.isnan(got["ece"]["point"][3]) and got["ece"]["n_degenerate"][3] == 64          # the class without rows
        # the counts are those of bootstrap_auc for the same seed: the kept weight of every (replicate, class) is the same
        plan = M.bootstrap_plan(z, t, g)
        U = plan["n_units"]
        _, wpos, wneg = ops.boot_auc(ops.boot_counts(U, 64, 9, device=dev), torch.from_numpy(plan["order"]).to(dev), plan["offs"], plan["lens"], U)
        assert np.array_equal(got["replicate_weights"].astype(np.int64), (wpos + wneg).cpu().numpy())
    points = K.calibration_metrics(z, t, None, 15, "width", device=dev)
    _same(points, K.calibration_metrics_reference(z, t, None, 15, "width"))
    assert set(points["ece"]) == {"point"}
    assert points["reliability"]["bins"] == 15 and len(points["reliability"]["weight"][0]) == 15


def _fit_case(N, C, seed):
    """Well-conditioned classes (lambda_min of the reference's Hessian >= 0.01 is asserted by the caller), some ignored labels, class 1
    all ignored and class 2 all positive."""
    rng = np.random.default_rng(seed)
    scale, shift = 1.0 + 0.5 * (np.arange(C) % 4), -0.3 * (np.arange(C) % 3)
    z = (rng.normal(size=(N, C)) * scale).astype(np.float32)
    p = 1.0 / (1.0 + np.exp(-(0.6 * z.astype(np.float64) + shift)))
    t = (rng.random((N, C)) < p).astype(np.float32)
    t[rng.random((N, C)) < 0.1] = -1.0
    t[:, 1] = -1.0
    t[:, 2] = 1.0
    return z, t


@pytest.mark.parametrize("C", (5, 33))
@pytest.mark.parametrize("N", (64, 255, 256, 257, 1000))
def test_fit_agrees_with_the_reference_iteration(dev, N, C):
    from chexpert_amd import ops
    z, t = _fit_case(N, C, 100 + N + C)
    g_tol = 1e-10
    for method in K.METHODS:
        ref = K.fit_calibration_reference(z, t, method, g_tol=g_tol)
        got = K.fit_calibration(z, t, method, g_tol=g_tol, device=dev)
        assert got["status"] == ref["status"] and ref["status"][1] == 2 and ref["status"][2] == 2 and ref["status"][0] == 0
        assert got["method"] == method and got["smooth"] is False and set(got) == set(ref)
        for c in range(C):
            for name in ("nll_before", "nll_after"):
                a, b = got[name][c], ref[name][c]
                assert (np.isnan(a) and np.isnan(b)) or abs(a - b) <= 1e-12 * N * abs(b), (name, c, a, b)
            if ref["status"][c] == 0:
                assert ref["lambda_min"][c] >= 0.01, (c, ref["lambda_min"][c])
                bound = 4 * g_tol / ref["lambda_min"][c]
                assert abs(got["a"][c] - ref["a"][c]) <= bound and abs(got["b"][c] - ref["b"][c]) <= bound, (c, got["a"][c], ref["a"][c])
                assert got["gmax"][c] <= g_tol and got["nll_after"][c] <= got["nll_before"][c]
            else:
                assert (got["a"][c], got["b"][c]) == (1.0, 0.0)
            if method == "temperature":
                assert got["b"][c] == 0.0
        assert np.isnan(got["nll_before"][1]) and np.isfinite(got["nll_before"][2])
    zt, tt = torch.from_numpy(z).to(dev), torch.from_numpy(t).to(dev)
    one, two = ops.calib_fit(zt, tt, "platt"), ops.calib_fit(zt, tt, "platt")
    assert one.dtype == torch.float64 and tuple(one.shape) == (C, 8)
    assert torch.equal(one.view(torch.int64), two.view(torch.int64))                       # the same bits (NaN included) on every run


def test_fit_statuses_separable_smooth_cap_and_refusals(dev, monkeypatch):
    from chexpert_amd import ops
    zs = np.linspace(-3, 3, 64).astype(np.float32)[:, None]
    ts = (zs > 0).astype(np.float32)
    sep = K.fit_calibration(zs, ts, "platt", device=dev)
    assert sep["status"][0] == 3 and (sep["a"][0], sep["b"][0]) == (1.0, 0.0) and sep["lambda_min"][0] < 1e-8
    assert sep["nll_after"][0] == sep["nll_before"][0]
    smooth, ref = K.fit_calibration(zs, ts, "platt", smooth=True, device=dev), K.fit_calibration_reference(zs, ts, "platt", smooth=True)
    assert smooth["status"][0] == 0 and ref["status"][0] == 0 and ref["lambda_min"][0] >= 0.01
    assert abs(smooth["a"][0] - ref["a"][0]) <= 4e-10 / ref["lambda_min"][0] and abs(smooth["b"][0] - ref["b"][0]) <= 4e-10 / ref["lambda_min"][0]
    z, t = _fit_case(255, 5, 1)
    capped, ref = K.fit_calibration(z, t, "platt", max_iter=1, device=dev), K.fit_calibration_reference(z, t, "platt", max_iter=1)
    assert capped["status"] == ref["status"] == {0: 1, 1: 2, 2: 2, 3: 1, 4: 1} and capped["iterations"][0] == 1
    assert abs(capped["a"][0] - ref["a"][0]) <= 1e-12 and capped["a"][0] != 1.0              # the one step is kept
    empty = ops.calib_fit(torch.zeros(0, 3, device=dev), torch.zeros(0, 3, device=dev))        # N = 0: no launch, every class degenerate
    assert tuple(empty.shape) == (3, 8) and empty[:, 7].tolist() == [2.0] * 3 and empty[:, 0].tolist() == [1.0] * 3
    zt, tt = torch.from_numpy(z).to(dev), torch.from_numpy(t).to(dev)
    monkeypatch.setattr(ops, "lib", lambda: pytest.fail("a refused call reached the library"))
    for bad in (dict(max_iter=0), dict(max_iter=1001), dict(method="isotonic"), dict(g_tol=float("nan"))):
        with pytest.raises(ValueError):
            ops.calib_fit(zt, tt, **bad)
        with pytest.raises(ValueError):
            K.fit_calibration(z, t, device=dev, **bad)


_CLI = ["--evaluate_single_model", "--synthetic", "64", "--batch_size", "4", "--resize", "64", "--seed", "3"]


@pytest.fixture(scope="module")
def fitted_run(dev, tmp_path_factory):
    """One `--calibrate platt --bootstrap 32` evaluation of the tiny synthetic configuration, shared by the two tests below."""
    from chexpert_amd import cli
    out = tmp_path_factory.mktemp("calibrate")
    cli.main(_CLI + ["--calibrate", "platt", "--bootstrap", "32", "--output_dir", str(out)])
    return out


def test_cli_writes_the_calibration_report_and_the_figure(fitted_run):
    out = fitted_run
    files = sorted(os.listdir(out))
    assert "calibration_step_0.json" in files and "reliability_step_0.png" in files and "eval_results_step_0.json" in files
    assert os.path.getsize(out / "reliability_step_0.png") > 2000
    rep = json.load(open(out / "calibration_step_0.json"))
    assert {"fit", "fitted_here", "ece_before", "mce_before", "brier_before", "ece_after", "mce_after", "brier_after", "reliability_before",
            "reliability_after", "unit"} == set(rep) and rep["fitted_here"] is True and rep["fit"]["method"] == "platt"
    for name in ("ece", "mce", "brier"):
        for when in ("before", "after"):
            s = rep["%s_%s" % (name, when)]
            assert s["n_boot"] == 32 and s["n_units"] == sum(rep["reliability_before"]["weight"]["0"]) > 0 and set(s["point"]) == set("01234")
            assert {"lo", "hi", "se", "mean_auc"} <= set(s)
    for c in "01234":
        assert rep["fit"]["status"][c] in (0, 1, 2, 3)
        before = rep["fit"]["nll_before"][c]
        assert before != before or rep["fit"]["nll_after"][c] <= before       # (NaN: a class without a kept row)


def test_cli_applies_a_stored_fit_and_reports_points_without_bootstrap(fitted_run, tmp_path, capsys):
    """--calibration_from on the same evaluation gives the "after" points of the run that fitted the map (the fit survives its json
    round trip bit for bit); without --bootstrap the summaries hold the points only; --calibration_bins alone applies no map."""
    from chexpert_amd import cli
    stored = str(fitted_run / "calibration_step_0.json")
    first = json.load(open(stored))
    cli.main(_CLI + ["--calibration_from", stored, "--output_dir", str(tmp_path / "from")])
    rep = json.load(open(tmp_path / "from" / "calibration_step_0.json"))
    assert rep["fitted_here"] is False
    _same(rep["fit"], first["fit"])
    for name in ("ece", "mce", "brier"):
        for when in ("before", "after"):
            assert set(rep["%s_%s" % (name, when)]) == {"point"}
            _same(rep["%s_%s" % (name, when)]["point"], first["%s_%s" % (name, when)]["point"])
    _same(rep["reliability_after"], first["reliability_after"])                      # (NaN in an empty bin)
    assert os.path.exists(tmp_path / "from" / "reliability_step_0.png")
    cli.main(_CLI + ["--calibration_bins", "10", "--calibration_binning", "mass", "--output_dir", str(tmp_path / "bins")])
    capsys.readouterr()
    rep = json.load(open(tmp_path / "bins" / "calibration_step_0.json"))
    assert rep["fit"] is None and "ece_after" not in rep and rep["reliability_before"]["bins"] == 10
    assert rep["reliability_before"]["binning"] == "mass" and os.path.exists(tmp_path / "bins" / "reliability_step_0.png")
