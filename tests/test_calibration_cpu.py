"""CPU (no GPU): the numpy statements of chexpert_amd/calibration.py -- the plan and sums cx_boot_calib is held to against the
definition in Python integers, the values against plain float64 ECE / Brier, the reference Newton fit against an independent gradient
-- and the host surface around them (command-line flags, the json round trip, predict's probabilities, the figure)."""
import json
import os

import numpy as np
import pytest
import torch

from chexpert_amd import calibration as K


def _case(seed, N=90, C=4, n_units=25):
    """Logits with ties, the extremes P = 0 / P = 2^32 - 1 (logits -800 / +800), some ignored rows, class 2 all ignored and class 3
    all positive; rows grouped into n_units units."""
    rng = np.random.default_rng(seed)
    z = np.round(rng.normal(0.0, 2.0, (N, C)), 1).astype(np.float32)              # one decimal: many equal scores
    t = (rng.random((N, C)) < 0.4).astype(np.float32)
    t[rng.random((N, C)) < 0.15] = -1.0
    z[0, 0], z[1, 0], z[2, 0], z[3, 0] = 800.0, -800.0, 800.0, -800.0
    t[:4, 0] = (1.0, 0.0, 0.0, 1.0)
    t[:, 2] = -1.0
    t[:, 3] = 1.0
    return z, t, rng.permutation(N) % n_units


def _counts(U, seed=5):
    rng = np.random.default_rng(seed)
    counts = rng.integers(0, 4001, size=(5, U)).astype(np.uint32)
    counts[rng.random((5, U)) < 0.33] = 0
    counts[2] = 4000
    counts[3] = 1                                                                 # the data set itself
    counts[4] = 0
    return counts


@pytest.mark.parametrize("binning", K.BINNINGS)
@pytest.mark.parametrize("M", (1, 2, 15, 64))
def test_sums_over_the_plan_equal_the_definition_in_exact_integers(M, binning):
    z, t, groups = _case(1)
    cal = {"a": {0: 0.7, 1: 1.3, 2: 1.0, 3: 2.0}, "b": {0: 0.2, 1: -0.5, 2: 0.0, 3: 0.1}}
    for g, c in ((groups, None), (None, cal)):
        plan = K.calibration_plan(z, t, g, c, M, binning)
        counts = _counts(plan["n_units"])
        got = K.calibration_sums_reference(counts, plan)
        want = K._calibration_definition(z, t, counts, g, c, M, binning)
        for a, b in zip(got, want):
            assert a.dtype == np.uint64 and a.shape == b.shape and (a.astype(object) == b).all()
        # bins ascend along a class's entries (what lets a lane of the kernel add once per bin), the extremes are present
        for cl in range(z.shape[1]):
            e = plan["order"][plan["offs"][cl]:plan["offs"][cl] + plan["lens"][cl]]
            assert (np.diff((e >> 24) & 63) >= 0).all() and (((e >> 24) & 63) < M).all()
        if c is None:
            P0 = plan["conf"][:plan["lens"][0]]
            assert P0.min() == 0 and P0.max() == 2 ** 32 - 1
        assert plan["lens"][2] == 0 and (got[0][:, 2] == 0).all() and (got[3][:, 2] == 0).all()      # the all-ignored class
        assert (got[0][:, 3] == got[1][:, 3]).all()                                                # the all-positive class


def test_edge_values_one_bin_empty_bins_and_nan():
    z, t, groups = _case(2)
    plan = K.calibration_plan(z, t, groups, None, 1, "width")
    sums = K.calibration_sums_reference(_counts(plan["n_units"]), plan)
    v = K._calibration_values(*sums)
    wsum, wpos, csum = (s.astype(np.float64)[:, :, 0] for s in sums[:3])
    with np.errstate(divide="ignore", invalid="ignore"):
        gap = np.abs(wpos / wsum - csum / (wsum * 2.0 ** 32))
    live = wsum > 0
    assert live[3].all() == False and live[3, 0] and not live[:, 2].any() and not live[4].any()
    assert (v["ece"][live] == v["mce"][live]).all()                               # M = 1: ECE == MCE == |frac_pos - mean_conf|
    np.testing.assert_allclose(v["ece"][live], gap[live], rtol=0, atol=1e-12)
    for name in ("ece", "mce", "brier"):                                          # NaN iff W = 0
        assert (np.isnan(v[name]) == ~live).all()
    # all rows in one bin of 64 (logits inside one bin's width), the other 63 empty
    z1 = np.full((10, 1), 0.01, dtype=np.float32) + np.arange(10, dtype=np.float32)[:, None] * 1e-4
    t1 = (np.arange(10) % 2).astype(np.float32)[:, None]
    p1 = K.calibration_plan(z1, t1, None, None, 64, "width")
    s1 = K.calibration_sums_reference(np.ones((1, 10), dtype=np.uint32), p1)
    assert (s1[0][0, 0] > 0).sum() == 1 and int(s1[0][0, 0, 32]) == 10
    v1 = K._calibration_values(*s1)
    assert v1["ece"][0, 0] == v1["mce"][0, 0]
    rel = K.calibration_metrics_reference(z1, t1, bins=64)["reliability"]
    assert rel["weight"][0][32] == 10 and rel["frac_pos"][0][32] == 0.5 and np.isnan(rel["frac_pos"][0][0])
    assert abs(rel["mean_conf"][0][32] - 0.5025) < 1e-3


@pytest.mark.parametrize("M", (2, 7, 15, 64))
def test_mass_binning_keeps_ties_together_and_balances_the_bins(M):
    z, t, _ = _case(3, N=200)
    plan = K.calibration_plan(z, t, None, None, M, "mass")
    for c in (0, 1):
        o, n = int(plan["offs"][c]), int(plan["lens"][c])
        e, P = plan["order"][o:o + n], plan["conf"][o:o + n]
        bins = (e >> 24) & 63
        for p in np.unique(P):
            assert len(set(bins[P == p])) == 1                                    # equal P never splits across bins
        largest_tie = np.unique(P, return_counts=True)[1].max()
        sizes = np.bincount(bins, minlength=M)
        # a tie group of g rows starting in a bin pulls at most g - 1 later rows into it and hands at most g - 1 of its first rows to the
        # bin before, on top of the floor / ceil of n / M: every bin is within the largest tie group of the equal share
        assert sizes.sum() == n and abs(sizes - n / M).max() <= largest_tie
    # without ties (largest tie group 1) the bins differ by at most one row
    z1 = np.random.default_rng(9).permutation(173).astype(np.float32)[:, None] / 20
    p1 = K.calibration_plan(z1, np.ones_like(z1), None, None, M, "mass")
    assert len(np.unique(p1["conf"])) == 173
    sizes = np.bincount((p1["order"] >> 24) & 63, minlength=M)
    assert sizes.sum() == 173 and sizes.max() - sizes.min() <= 1


@pytest.mark.parametrize("binning", K.BINNINGS)
def test_values_agree_with_plain_float64_ece_and_brier(binning):
    """The fixed point loses less than 2^-32 of a row's confidence and the squared residual less than 2^-31, so both values are
    within 2^-31 of the float64 ones computed from p directly (plus a few ulp): 1e-9 is a derived bound, not a measurement."""
    z, t, groups = _case(4)
    M = 15
    plan = K.calibration_plan(z, t, groups, None, M, binning)
    counts = _counts(plan["n_units"])
    v = K._calibration_values(*K.calibration_sums_reference(counts, plan))
    for c in (0, 1, 3):
        keep = t[:, c] >= 0
        p = K._sigmoid64(z[keep, c].astype(np.float64))
        y = (t[keep, c] > 0.5).astype(np.float64)
        bins = K._bins_of(K.fixed_point(p), M, binning)
        for r in range(len(counts)):
            w = counts[r, groups[keep]].astype(np.float64)
            if w.sum() == 0:
                assert np.isnan(v["ece"][r, c]) and np.isnan(v["brier"][r, c])
                continue
            gaps = np.array([abs((w * (y - p))[bins == k].sum()) for k in range(M)])
            sizes = np.array([w[bins == k].sum() for k in range(M)])
            assert abs(v["ece"][r, c] - gaps.sum() / w.sum()) <= 1e-9
            assert abs(v["mce"][r, c] - (gaps[sizes > 0] / sizes[sizes > 0]).max()) <= 1e-9
            assert abs(v["brier"][r, c] - (w * (y - p) ** 2).sum() / w.sum()) <= 1e-9


def _draw(N, C, seed):
    rng = np.random.default_rng(seed)
    z = np.stack([rng.normal(0.0, 1.0 + c, N) for c in range(C)], 1).astype(np.float32)
    p = 1.0 / (1.0 + np.exp(-(0.6 * z.astype(np.float64) - 0.4 * np.arange(C))))
    return z, (rng.random((N, C)) < p).astype(np.float32)


def _gradient(z, t, a, b):
    """The float64 gradient of the mean loss, written independently of calibration._fit_terms (through tanh)."""
    u = a * z.astype(np.float64) + b
    r = 0.5 * (1.0 + np.tanh(0.5 * u)) - t
    return np.mean(r * z.astype(np.float64)), np.mean(r)


@pytest.mark.parametrize("N", (64, 255, 1000))
def test_reference_fit_converges_to_a_stationary_point(N):
    z, t = _draw(N, 5, 11 + N)
    for method in K.METHODS:
        fit = K.fit_calibration_reference(z, t, method)
        assert json.loads(json.dumps(fit))["a"]["0"] == fit["a"][0]               # json-serialisable
        for c in range(5):
            assert fit["status"][c] == 0 and fit["nll_after"][c] <= fit["nll_before"][c] and 1 <= fit["iterations"][c] <= 12
            ga, gb = _gradient(z[:, c], t[:, c], fit["a"][c], fit["b"][c])
            assert abs(ga) <= 10 * 1e-10 and (method == "temperature" or abs(gb) <= 10 * 1e-10)
            assert fit["temperature"][c] == 1.0 / fit["a"][c]
            if method == "temperature":
                assert fit["b"][c] == 0.0                                         # exactly


def test_reference_fit_statuses_and_the_undone_scaling():
    zs = np.linspace(-3, 3, 64).astype(np.float32)[:, None]
    ts = (zs > 0).astype(np.float32)
    sep = K.fit_calibration_reference(zs, ts, "platt")
    assert sep["status"][0] == 3 and sep["a"][0] == 1.0 and sep["b"][0] == 0.0 and sep["lambda_min"][0] < 1e-8
    assert sep["nll_after"][0] == sep["nll_before"][0]
    smooth = K.fit_calibration_reference(zs, ts, "platt", smooth=True)
    assert smooth["status"][0] == 0 and smooth["lambda_min"][0] > 0.01 and smooth["a"][0] > 1.0
    none = K.fit_calibration_reference(zs, np.zeros_like(ts), "platt")            # no positives
    assert none["status"][0] == 2 and none["a"][0] == 1.0 and none["b"][0] == 0.0
    empty = K.fit_calibration_reference(zs, -np.ones_like(ts), "temperature")     # no kept row
    assert empty["status"][0] == 2 and np.isnan(empty["nll_before"][0])
    capped = K.fit_calibration_reference(*_draw(255, 2, 3), "platt", max_iter=1)
    assert set(capped["status"].values()) == {1} and set(capped["iterations"].values()) == {1}
    for bad in (dict(max_iter=0), dict(max_iter=1001), dict(method="isotonic"), dict(g_tol=-1.0)):
        with pytest.raises(ValueError):
            K.fit_calibration_reference(zs, ts, **bad)
    # scaling the logits by 2 is undone: the minimiser in a halves.  Both fits stop within g_tol / lambda_min of their minimiser
    # (the bound of tests/test_calibration_gpu.py), and 2 z is exact in float32
    z, t = _draw(1000, 3, 7)
    for method in K.METHODS:
        one, two = K.fit_calibration_reference(z, t, method), K.fit_calibration_reference(2 * z, t, method)
        for c in range(3):
            bound = 4 * 1e-10 / min(one["lambda_min"][c], two["lambda_min"][c])
            assert abs(two["a"][c] - 0.5 * one["a"][c]) <= bound and abs(two["b"][c] - one["b"][c]) <= bound


def test_cli_flags_parse_and_the_exclusive_pair_errors(tmp_path, capsys):
    from chexpert_amd import cli
    a = cli.parse_args(["--evaluate_single_model", "--calibrate", "platt", "--calibrate_smooth", "--calibration_bins", "20",
                        "--calibration_binning", "mass"])
    assert (a.calibrate, a.calibrate_smooth, a.calibration_bins, a.calibration_binning, a.calibration_from) == ("platt", True, 20, "mass", None)
    d = cli.parse_args(["--evaluate_single_model"])
    assert (d.calibrate, d.calibrate_smooth, d.calibration_bins, d.calibration_binning, d.calibration_from) == (None, False, None, "width", None)
    stored = tmp_path / "calibration_step_0.json"
    fit = K.fit_calibration_reference(*_draw(255, 5, 1), "platt")
    json.dump({"fit": fit}, open(stored, "w"))
    assert cli.parse_args(["--calibration_from", str(stored)]).calibration_from == str(stored)
    for bad in (["--calibrate", "platt", "--calibration_from", str(stored)], ["--calibrate", "isotonic"], ["--calibration_bins", "0"],
                ["--calibration_bins", "65"], ["--calibrate_smooth"], ["--calibration_from", str(tmp_path / "missing.json")],
                ["--calibration_binning", "quantile"]):
        with pytest.raises(SystemExit):
            cli.parse_args(bad)
    capsys.readouterr()
    assert cli.report_name("eval_results_step_5", "calibration") == "calibration_step_5.json"
    assert not cli.report_name("eval_results_ensemble", "reliability", ".png").startswith("eval_results")
    # nothing asked for: nothing computed or written
    assert cli.write_calibration(d, "eval_results_step_0", None, None) is None
    # the json round trip (string class keys) gives the same calibrated logits
    z = _draw(255, 5, 1)[0]
    back = K.load_calibration(str(stored))
    assert set(back["a"]) == {"0", "1", "2", "3", "4"}
    want = z.astype(np.float64) * np.array([fit["a"][c] for c in range(5)]) + np.array([fit["b"][c] for c in range(5)])
    assert np.array_equal(K.apply_calibration(z, fit), want) and np.array_equal(K.apply_calibration(z, back), want)
    got = K.apply_calibration(torch.from_numpy(z), back)
    assert got.dtype == torch.float64 and np.array_equal(got.numpy(), want)
    with pytest.raises(ValueError):
        K.apply_calibration(z[:, :3], fit)
    json.dump({"aucs": {}}, open(tmp_path / "other.json", "w"))
    with pytest.raises(ValueError):
        K.load_calibration(str(tmp_path / "other.json"))


def test_predict_probabilities_identity_is_bit_equal(tmp_path):
    from chexpert_amd import predict
    rng = np.random.default_rng(0)
    z = torch.from_numpy(rng.normal(0, 4, (33, 5)).astype(np.float32))
    plain = predict.probabilities(z)
    assert torch.equal(plain, torch.sigmoid(z))
    identity = K.fit_calibration_reference(np.zeros((4, 5), np.float32), -np.ones((4, 5), np.float32))      # status 2 everywhere
    path = tmp_path / "calibration_identity.json"
    json.dump({"fit": identity}, open(path, "w"))
    assert torch.equal(predict.probabilities(z, K.load_calibration(str(path))), plain)
    assert torch.equal(predict.probabilities(z.bfloat16(), K.load_calibration(str(path))), torch.sigmoid(z.bfloat16().float()))
    fit = dict(identity, a={c: 0.5 for c in range(5)}, b={c: 0.25 for c in range(5)})
    assert torch.equal(predict.probabilities(z, fit), torch.sigmoid(z * 0.5 + 0.25))
    args = predict.parse_args(["in.csv", "out.csv", "--restore_path", "x.pt", "--calibration", str(path)])
    assert args.calibration == str(path) and predict.parse_args(["in.csv", "out.csv", "--restore_path", "x.pt"]).calibration is None
    with pytest.raises(SystemExit):
        predict.parse_args(["in.csv", "out.csv", "--restore_path", "x.pt", "--calibration", str(tmp_path / "missing.json")])


def test_reliability_diagram_writes_a_figure(tmp_path):
    from chexpert_amd import vis
    z, t = _draw(255, 5, 2)
    before = K.calibration_metrics_reference(z, t, bins=10)
    fit = K.fit_calibration_reference(z, t, "platt")
    after = K.calibration_metrics_reference(z, t, fit, bins=10)
    assert set(before) == {"ece", "mce", "brier", "reliability"} and set(before["ece"]) == {"point"}
    names = ["Atelectasis", "Cardiomegaly", "Consolidation", "Edema", "Pleural Effusion"]
    one = vis.reliability_diagram(before["reliability"], names, str(tmp_path / "reliability_a.png"))
    two = vis.reliability_diagram(json.loads(json.dumps(before["reliability"])), names, str(tmp_path / "reliability_b.png"),
                                  after=after["reliability"])
    for path in (one, two):
        assert os.path.getsize(path) > 2000 and open(path, "rb").read(4) == b"\x89PNG"


def test_reference_metrics_summaries_have_the_bootstrap_shape():
    z, t = _draw(64, 3, 4)
    groups = np.arange(64) // 2
    m = K.calibration_metrics_reference(z, t, n_boot=20, seed=3, groups=groups, return_replicates=True)
    for name in ("ece", "mce", "brier"):
        s = m[name]
        assert set(s) == {"point", "lo", "hi", "se", "n_degenerate", "mean_auc", "n_boot", "seed", "alpha", "n_units", "replicates"}
        assert s["n_units"] == 32 and s["replicates"].shape == (20, 3) and all(s["lo"][c] <= s["hi"][c] for c in range(3))
    assert m["replicate_weights"].shape == (20, 3) and (m["replicate_weights"] == 64).all()       # every row kept: W = 2 U
    with pytest.raises(ValueError):
        K.calibration_metrics_reference(z, t, n_boot=-1)
    with pytest.raises(ValueError):
        K.calibration_metrics_reference(z, t, bins=0)
    with pytest.raises(ValueError):
        K.calibration_metrics_reference(z, t, binning="quantile")
