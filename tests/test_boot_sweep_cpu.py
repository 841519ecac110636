"""CPU (no GPU): the integer definition of the bootstrapped average precision and fixed operating points (chexpert_amd.metrics:
bootstrap_sweep_plan, bootstrap_sweep_reference, bootstrap_metrics_reference -- the statement the kernel cx_boot_sweep of
chexpert_amd/csrc/bootstrap.hip is held to in tests/test_boot_sweep_gpu.py) pinned by a second statement straight from the definition, by
metrics.precision_recall_curve / metrics.roc_curve on the materialised resample and by hand-computed values; the argument checks of the
entry point, and the command-line wiring."""
import ctypes
import json
import os
import re

import numpy as np
import pytest

from chexpert_amd import metrics as M

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("ap", "sens@0.9", "spec@0.9", "sens@0.5", "spec@0.123456")


def _case(N, C, seed, ties=True, ignore=0.1):
    rng = np.random.default_rng(seed)
    s = rng.normal(size=(N, C))
    if ties:
        s = np.round(s * 2) / 2                                        # scores rounded to halves: heavy ties
    t = (rng.random((N, C)) < 0.4).astype(np.float64)
    t[rng.random((N, C)) < ignore] = -1.0
    return s, t


def _counts(N, R, seed):
    """Bootstrap rows with a further third of the weights set to zero, a row of ones and a row with one unit only."""
    rng = np.random.default_rng(seed)
    counts = M.bootstrap_counts_reference(N, R, seed)
    counts[rng.random(counts.shape) < 0.33] = 0
    counts[-2] = 1
    counts[-1] = 0
    counts[-1, N // 2] = 3
    return counts


def test_metric_names_are_parsed_strictly():
    names, points = M.parse_boot_metrics(["auroc", "ap", "sens@0.9", "spec@.95", "sens@0.000001", "spec@0.999999", "sens@0.5000"])
    assert names == ("auroc", "ap", "sens@0.9", "spec@.95", "sens@0.000001", "spec@0.999999", "sens@0.5000")
    assert points == [(M.BOOT_SENS, 900000), (M.BOOT_SPEC, 950000), (M.BOOT_SENS, 1), (M.BOOT_SPEC, 999999), (M.BOOT_SENS, 500000)]
    assert M.parse_boot_metrics("ap") == (("ap",), [])
    for bad in (["auc"], ["AP"], ["sens@"], ["sens@0"], ["sens@0.0"], ["sens@1"], ["spec@1.0"], ["sens@1.5"], ["sens@-0.5"],
                ["sens@0.1234567"], ["sens@0.90000000"], ["sens@9e-1"], ["sens@0.9 "], ["sens@0.9\n"], ["sens @0.9"], ["sensitivity@0.9"],
                ["spec@nan"], ["ap", "ap"], ["sens@0.9", "sens@0.9"], [], [3], ["sens@0.%d" % k for k in range(1, 10)]):
        with pytest.raises(ValueError):
            M.parse_boot_metrics(bad)
    assert len(M.parse_boot_metrics(["sens@0.%d" % k for k in range(1, 9)])[1]) == 8 == M.BOOT_MAX_POINTS


def test_plan_lists_every_class_once_descending_with_the_group_ends_marked():
    s, t = _case(90, 3, 5)
    groups = np.arange(90) // 2
    plan = M.bootstrap_sweep_plan(s, t, groups)
    assert plan["n_units"] == 45 and plan["order"].dtype == np.int32 and plan["lens"].dtype == np.int32
    assert np.array_equal(plan["lens"], (t >= 0).sum(0)) and np.array_equal(plan["offs"], np.r_[0, np.cumsum(plan["lens"])[:-1]])
    for c in range(3):
        e = plan["order"][plan["offs"][c]:plan["offs"][c] + plan["lens"][c]]
        keep = np.nonzero(t[:, c] >= 0)[0]
        # the entries are a permutation of the kept rows: recover the rows from the deterministic order inside a tie group
        by = sorted(keep, key=lambda i: (-s[i, c], not t[i, c] > 0.5, i))
        assert np.array_equal(e & 0xffffff, groups[by]) and np.array_equal(e < 0, t[by, c] > 0.5)
        sc = s[by, c]
        assert np.array_equal((e & 0x40000000) != 0, np.r_[sc[1:] != sc[:-1], True])
        assert ((e & 0x3f000000) == 0).all()                               # nothing else above the unit index
    again = M.bootstrap_sweep_plan(s, t, groups)
    assert all(np.array_equal(plan[k], again[k]) for k in ("order", "offs", "lens", "units"))
    empty = M.bootstrap_sweep_plan(s, np.full_like(t, -1.0))
    assert list(empty["lens"]) == [0, 0, 0] and len(empty["order"]) == 0
    with pytest.raises(ValueError):
        M.bootstrap_sweep_plan(np.full((4, 1), np.nan), np.zeros((4, 1)))
    with pytest.raises(ValueError):
        M.bootstrap_sweep_plan(s, t, groups[:-1])


def test_hand_computed_values():
    # scores 3 2 2 1, labels + - + -, weights 1 2 1 3: the curve is (0,0) (1,0) (2,2) (2,5); W+ = 2, W- = 5
    s = np.array([[3.0], [2.0], [2.0], [1.0]])
    t = np.array([[1.0], [0.0], [1.0], [0.0]])
    plan = M.bootstrap_sweep_plan(s, t)
    assert list(plan["order"].view(np.uint32)) == [0xC0000000, 0x80000002, 0x40000001, 0x40000003]
    counts = np.array([[1, 2, 1, 3]], dtype=np.uint32)
    _, points = M.parse_boot_metrics(["sens@0.9", "sens@0.6", "spec@0.5", "spec@0.500001"])
    apnum, wpos, wneg, pts = M.bootstrap_sweep_reference(counts, plan["order"], plan["offs"], plan["lens"], 4, points)
    assert (int(wpos[0, 0]), int(wneg[0, 0])) == (2, 5)
    assert int(apnum[0, 0]) == 1 * (1 << 32) + 1 * ((2 << 32) // 4)                        # precision 1 then 1/2, a step of 1 each
    # sens@0.9: fp * 1e6 <= 1e5 * 5 -> fp = 0 -> tp 1; sens@0.6: fp <= 2 -> tp 2; spec@0.5: tp >= 1 -> fp 0; spec@0.500001: tp >= 2 -> fp 2
    assert [int(v) for v in pts[0, 0]] == [1, 2, 0, 2]
    v = M._sweep_values(("sens@0.9", "sens@0.6", "spec@0.5", "spec@0.500001", "ap"), points, apnum, wpos, wneg, pts)
    assert (v["ap"][0, 0], v["sens@0.9"][0, 0], v["sens@0.6"][0, 0], v["spec@0.5"][0, 0], v["spec@0.500001"][0, 0]) == (0.75, 0.5, 1.0, 1.0, 0.6)
    # the weight 0 on the second positive's unit removes nothing from the static marks: the group (2.0) still ends with (1, 2)
    counts = np.array([[1, 2, 0, 3]], dtype=np.uint32)
    apnum, wpos, wneg, pts = M.bootstrap_sweep_reference(counts, plan["order"], plan["offs"], plan["lens"], 4, points)
    assert int(apnum[0, 0]) == 1 << 32 and [int(v) for v in pts[0, 0]] == [1, 1, 0, 0] and (int(wpos[0, 0]), int(wneg[0, 0])) == (1, 5)
    # a unit index past n_units reads the last unit's count
    a = M.bootstrap_sweep_reference(counts, plan["order"], plan["offs"], plan["lens"], 2, points)
    b = M.bootstrap_sweep_reference(counts[:, [0, 1, 1, 1]], plan["order"], plan["offs"], plan["lens"], 4, points)
    assert all(np.array_equal(x, y) for x, y in zip(a, b))
    for bad in ([(2, 5)], [(0, 0)], [(1, 10 ** 6)], [(0, 5)] * 9):
        with pytest.raises(ValueError):
            M.bootstrap_sweep_reference(counts, plan["order"], plan["offs"], plan["lens"], 4, bad)


@pytest.mark.parametrize("N", [1, 2, 65, 257])
def test_statement_equals_the_definition_in_integers(N):
    s, t = _case(N, 4, N)
    s[:, 3] = 0.25                                                      # one tie group of all rows
    groups = np.random.default_rng(N).permutation(N) % max(1, N // 2)   # several rows per unit
    plan = M.bootstrap_sweep_plan(s, t, groups)
    counts = _counts(plan["n_units"], 6, N)
    _, points = M.parse_boot_metrics(NAMES)
    got = M.bootstrap_sweep_reference(counts, plan["order"], plan["offs"], plan["lens"], plan["n_units"], points)
    want = M._sweep_definition_parts(s, t, plan["units"], counts, points)
    for g, w in zip(got, want):
        assert g.dtype == np.uint64 and g.shape == w.shape and np.array_equal(g.astype(object), w)
    # without operating points the other three outputs are the same
    for g, w in zip(M.bootstrap_sweep_reference(counts, plan["order"], plan["offs"], plan["lens"], plan["n_units"]), got[:3]):
        assert np.array_equal(g, w)


def _float_reference(y, sc, points):
    """AP, sens@ and spec@ of a materialised sample through metrics.precision_recall_curve and metrics.roc_curve.  The operating point is
    picked by the integer condition on the curve's own counts (fpr and tpr times the totals round to them exactly), so that a comparison
    sitting on its boundary cannot fall to the other side in floating point; the VALUE compared is the curve's."""
    p, r, _ = M.precision_recall_curve(y, sc)
    ap = -np.sum(np.diff(r) * p[:-1])                                   # sklearn.average_precision_score's step sum
    fpr, tpr, _ = M.roc_curve(y, sc)
    Wp, Wn = int((y > 0.5).sum()), int((y <= 0.5).sum())
    if Wn == 0:
        return ap, None
    fp, tp = np.rint(fpr * Wn).astype(np.int64), np.rint(tpr * Wp).astype(np.int64)
    out = []
    for kind, ppm in points:
        if kind == M.BOOT_SENS:
            out.append(tpr[fp * 10 ** 6 <= (10 ** 6 - ppm) * Wn].max())
        else:
            out.append(1.0 - fpr[tp * 10 ** 6 >= ppm * Wp].min())
    return ap, out


@pytest.mark.parametrize("N", [1, 2, 65, 257, 1000])
def test_statement_against_the_float_curves_of_the_materialised_resample(N):
    """Bounds.  AP: every floor loses less than 2^-32 of its step's weight (2^-32 in all); the float route sums at most N products of a
    recall step and a precision, each factor and each partial sum <= 1 carrying one rounding of at most 2^-53: N * 2^-52 covers them and
    the two roundings of the integer route.  Operating points: a roc_curve coordinate is one correctly rounded quotient, as is the
    integer route's (1 - x adds one rounding of a value <= 1): far inside N * 2^-52."""
    s, t = _case(N, 3, 1000 + N)
    s[:, 2] = -1.5                                                      # a tie group of all rows
    plan = M.bootstrap_sweep_plan(s, t)
    counts = _counts(N, 8, N)
    names, points = M.parse_boot_metrics(NAMES)
    ints = M.bootstrap_sweep_reference(counts, plan["order"], plan["offs"], plan["lens"], N, points)
    val = M._sweep_values(names, points, *ints)
    seen = 0
    for r in range(len(counts)):
        for c in range(3):
            keep = t[:, c] >= 0
            w = counts[r][keep]
            y, sc = np.repeat(t[keep, c], w), np.repeat(s[keep, c], w)
            Wp, Wn = int((y > 0.5).sum()), int((y <= 0.5).sum())
            assert (int(ints[1][r, c]), int(ints[2][r, c])) == (Wp, Wn)
            if Wp == 0:
                assert all(np.isnan(val[n][r, c]) for n in names)
                continue
            ap, ops_ = _float_reference(y, sc, points)
            assert abs(val["ap"][r, c] - ap) <= 2.0 ** -32 + N * 2.0 ** -52, (r, c, val["ap"][r, c], ap)
            assert val["ap"][r, c] <= ap + N * 2.0 ** -52                                   # the floors only ever lose
            if Wn == 0:
                assert all(np.isnan(val[n][r, c]) for n in names[1:])
                continue
            for n, ref in zip(names[1:], ops_):
                seen += 1
                assert abs(val[n][r, c] - ref) <= N * 2.0 ** -52, (r, c, n, val[n][r, c], ref)
    assert seen > 0 or N <= 2


def test_degenerate_classes():
    N, B = 40, 12
    rng = np.random.default_rng(3)
    s = np.round(rng.normal(size=(N, 4)))
    t = (rng.random((N, 4)) < 0.5).astype(np.float64)
    t[:, 1], t[:, 2], t[:, 3] = 1.0, 0.0, -1.0                          # all positive, all negative, all ignored
    assert list(M.bootstrap_sweep_plan(s, t)["lens"]) == [N, N, N, 0]
    r = M.bootstrap_metrics_reference(s, t, ("auroc", "ap", "sens@0.9", "spec@0.8"), n_boot=B, seed=2, return_replicates=True)
    assert list(r) == ["auroc", "ap", "sens@0.9", "spec@0.8"]
    ap, sens, spec = r["ap"], r["sens@0.9"], r["spec@0.8"]
    assert (ap["replicates"][:, 1] == 1.0).all() and ap["point"][1] == 1.0 and ap["n_degenerate"][1] == 0
    for m in (sens, spec):
        assert np.isnan(m["replicates"][:, 1:]).all() and all(np.isnan(m["point"][c]) and m["n_degenerate"][c] == B for c in (1, 2, 3))
        assert np.isfinite(m["replicates"][:, 0]).all() and m["n_degenerate"][0] == 0
    assert np.isnan(ap["replicates"][:, 2:]).all() and all(np.isnan(ap["point"][c]) and ap["n_degenerate"][c] == B for c in (2, 3))
    assert np.isnan(ap["lo"][3]) and np.isnan(ap["se"][3]) and np.isnan(ap["mean_auc"]["point"])
    for m in r.values():
        assert set(m) == {"point", "lo", "hi", "se", "n_degenerate", "mean_auc", "n_boot", "seed", "alpha", "n_units", "replicates"}
        assert (m["n_boot"], m["seed"], m["alpha"], m["n_units"]) == (B, 2, 0.05, N)
        json.dumps({k: v for k, v in m.items() if k != "replicates"})


def test_consistency_with_the_auroc_bootstrap_and_the_paired_form():
    s, t = _case(150, 3, 33)
    groups = np.arange(150) // 3
    for g in (None, groups):
        a = M.bootstrap_metrics_reference(s, t, ("ap", "auroc", "sens@0.9"), n_boot=30, seed=4, groups=g, alpha=0.1, return_replicates=True)
        b = M.bootstrap_auc_reference(s, t, n_boot=30, seed=4, groups=g, alpha=0.1, return_replicates=True)
        assert list(a) == ["ap", "auroc", "sens@0.9"]
        assert set(a["auroc"]) - {"point"} == set(b) - {"aucs"}
        for k in b:
            x, y = a["auroc"]["point" if k == "aucs" else k], b[k]
            if isinstance(y, dict):
                assert x.keys() == y.keys() and np.array_equal(np.array(list(x.values()), float), np.array(list(y.values()), float), equal_nan=True)
            else:
                assert np.array_equal(x, y, equal_nan=True)
        # the metrics share the replicates' draws: one metric asked for alone gives the same numbers
        alone = M.bootstrap_metrics_reference(s, t, ("sens@0.9",), n_boot=30, seed=4, groups=g, alpha=0.1, return_replicates=True)
        assert np.array_equal(alone["sens@0.9"]["replicates"], a["sens@0.9"]["replicates"], equal_nan=True)
    names = ("auroc", "ap", "sens@0.9", "spec@0.9")
    r = M.bootstrap_metrics_diff_reference(s, s, t, names, n_boot=30, seed=1)
    assert list(r) == list(names)
    for m in r.values():
        for c in range(3):
            assert (m["delta"][c], m["lo"][c], m["hi"][c], m["p"][c]) == (0.0, 0.0, 0.0, 1.0)
        assert (m["mean_auc"]["delta"], m["mean_auc"]["lo"], m["mean_auc"]["hi"], m["mean_auc"]["p"]) == (0.0, 0.0, 0.0, 1.0)
    better = s + 3.0 * (t > 0.5)
    r = M.bootstrap_metrics_diff_reference(better, s, t, names, n_boot=40, seed=1, return_replicates=True)
    a = M.bootstrap_metrics_reference(better, t, names, n_boot=40, seed=1, return_replicates=True)
    b = M.bootstrap_metrics_reference(s, t, names, n_boot=40, seed=1, return_replicates=True)
    for n in names:
        assert np.array_equal(r[n]["replicates"], a[n]["replicates"] - b[n]["replicates"], equal_nan=True)      # paired: the same draws
        assert all(r[n]["delta"][c] > 0 and r[n]["lo"][c] > 0 for c in range(3))
    for bad in ({"n_boot": 0}, {"alpha": 1.0}, {"metrics": ("f1",)}, {"metrics": ("sens@1.0",)}):
        with pytest.raises(ValueError):
            M.bootstrap_metrics_reference(s, t, **bad)


def test_entry_point_validates_without_launching():
    from chexpert_amd import _lib, ops
    EINVAL, EALIGN, ESHAPE = -1, -2, -3
    f = _lib.lib().cx_boot_sweep
    buf = (ctypes.c_uint64 * 64)()
    P = ctypes.addressof(buf)
    assert P % 8 == 0
    offs, lens = (ctypes.c_int64 * 2)(0, 8), (ctypes.c_int32 * 2)(4, 3)
    kinds, ppms = (ctypes.c_int32 * 2)(0, 1), (ctypes.c_int32 * 2)(900000, 1)

    def call(counts=P, ld=8, n_rep=1, order=P, offs=offs, lens=lens, C=2, kinds=kinds, ppms=ppms, n=2, apnum=P, wpos=P, wneg=P, pts=P, U=8):
        return f(counts, ld, n_rep, order, offs, lens, C, kinds, ppms, n, apnum, wpos, wneg, pts, U, None)
    for name in ("counts", "order", "offs", "lens", "apnum", "wpos", "wneg", "kinds", "ppms", "pts"):
        assert call(**{name: None}) == EINVAL, name
    assert call(n_rep=0) == EINVAL and call(C=0) == EINVAL and call(C=-1) == EINVAL
    assert call(lens=(ctypes.c_int32 * 2)(4, -1)) == EINVAL and call(offs=(ctypes.c_int64 * 2)(0, -8)) == EINVAL
    assert call(n=9) == ESHAPE and call(n=-1) == ESHAPE
    for bad in ((0, 0), (0, 1000000), (0, -5), (2, 5), (-1, 5)):
        assert call(kinds=(ctypes.c_int32 * 2)(0, bad[0]), ppms=(ctypes.c_int32 * 2)(5, bad[1])) == EINVAL, bad
    assert call(U=0) == ESHAPE and call(U=(1 << 24) + 1, ld=1 << 25) == ESHAPE and call(ld=7) == ESHAPE
    assert call(apnum=P + 4) == EALIGN and call(order=P + 2) == EALIGN and call(counts=P + 1) == EALIGN and call(wpos=P + 2) == EALIGN
    assert call(wneg=P + 2) == EALIGN and call(pts=P + 2) == EALIGN
    # declared in the header with the parameters the binding passes; the constants ops and metrics export are the header's
    hdr = open(os.path.join(ROOT, "include", "chexpert_hip.h")).read()
    code = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    m = re.search(r"\bint\s+cx_boot_sweep\s*\(([^;{]*?)\)\s*;", code, flags=re.S)
    assert m and len(_lib.SIGNATURES["cx_boot_sweep"]) == m.group(1).count(",") + 1 == 16
    for name, v in (("CX_BOOT_MAX_POINTS", 8), ("CX_BOOT_SENS", 0), ("CX_BOOT_SPEC", 1)):
        assert int(re.search(r"\b%s\s*=\s*(\d+)" % name, code).group(1)) == v
    assert (ops.BOOT_MAX_POINTS, ops.BOOT_SENS, ops.BOOT_SPEC) == (M.BOOT_MAX_POINTS, M.BOOT_SENS, M.BOOT_SPEC) == (8, 0, 1)
    assert _lib.lib().cx_abi_version() == 10                            # an additive entry point


def test_command_line_flags_and_config_round_trip(tmp_path):
    from chexpert_amd import cli
    assert cli.parse_args([]).bootstrap_metrics is None
    a = cli.parse_args(["--evaluate", "--bootstrap", "200", "--bootstrap_metrics", "ap", "sens@0.9", "spec@0.95", "--bootstrap_seed", "9"])
    assert a.bootstrap_metrics == ["ap", "sens@0.9", "spec@0.95"] and (a.bootstrap, a.bootstrap_seed) == (200, 9)
    for argv in (["--bootstrap_metrics", "ap"], ["--bootstrap", "0", "--bootstrap_metrics", "ap"], ["--bootstrap", "10", "--bootstrap_metrics"],
                 ["--bootstrap", "10", "--bootstrap_metrics", "auprc"], ["--bootstrap", "10", "--bootstrap_metrics", "sens@1"],
                 ["--bootstrap", "10", "--bootstrap_metrics", "sens@0.1234567"], ["--bootstrap", "10", "--bootstrap_metrics", "ap", "ap"],
                 ["--bootstrap", "10", "--bootstrap_metrics"] + ["spec@0.%d" % k for k in range(1, 10)]):
        with pytest.raises(SystemExit):
            cli.parse_args(argv)
    path = tmp_path / "config.json"
    json.dump(a.__dict__, open(path, "w"), indent=4)
    b = cli.parse_args(["--load_config", str(path)])
    assert b.bootstrap_metrics == ["ap", "sens@0.9", "spec@0.95"] and b.bootstrap == 200
    cfg = json.load(open(path))
    cfg["bootstrap_metrics"] = ["sens@2"]
    json.dump(cfg, open(path, "w"))
    with pytest.raises(SystemExit):                                     # checked after the config is applied
        cli.parse_args(["--load_config", str(path)])
    cfg["bootstrap_metrics"], cfg["bootstrap"] = ["ap"], 0
    json.dump(cfg, open(path, "w"))
    with pytest.raises(SystemExit):
        cli.parse_args(["--load_config", str(path)])


def test_command_line_file_name_and_nothing_without_the_flag(tmp_path):
    import fnmatch

    from chexpert_amd import cli
    for tag, want in (("eval_results_step_300", "metrics_ci_step_300.json"), ("eval_results_ensemble", "metrics_ci_ensemble.json")):
        assert cli.report_name(tag, "metrics_ci") == want and want != cli.report_name(tag, "auc_ci")
        assert not fnmatch.fnmatch(want, "eval_results*") and not want.startswith("eval_results")      # --plot_roc globs that prefix
    s, t = _case(20, 5, 1)
    # without the option, and without --bootstrap, nothing is computed (no GPU is touched: this test runs without one) or written
    for argv in (["--evaluate"], ["--evaluate", "--bootstrap", "10"]):
        a = cli.parse_args(argv + ["--output_dir", str(tmp_path)])
        assert cli.write_metrics_ci(a, "eval_results_step_0", s, t) is None and os.listdir(tmp_path) == []
