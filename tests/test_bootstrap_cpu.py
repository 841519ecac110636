"""CPU (no GPU): the integer definition of the AUROC bootstrap (chexpert_amd.metrics: bootstrap_counts_reference, bootstrap_scan_reference,
bootstrap_auc_reference -- the statements the kernels of chexpert_amd/csrc/bootstrap.hip are held to in tests/test_bootstrap_gpu.py)
pinned by hand-computed vectors and by metrics.roc_curve / metrics.auc on the materialised resample, the argument checks of the two
entry points, and the command-line wiring."""
import ctypes
import json
import os
import re

import numpy as np
import pytest

from chexpert_amd import metrics as M

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _case(N, C, seed, ties=True, ignore=0.1):
    rng = np.random.default_rng(seed)
    s = rng.normal(size=(N, C))
    if ties:
        s = np.round(s * 2) / 2                                        # scores rounded to 0.5: heavy ties
    t = (rng.random((N, C)) < 0.4).astype(np.float64)
    t[rng.random((N, C)) < ignore] = -1.0
    return s, t


def test_splitmix_vectors_and_draws():
    assert [M.splitmix64(0, k) for k in range(3)] == [0xe220a8397b1dcdaf, 0x6e789e6aa1b965f4, 0x06c45d188009454f]
    assert list(M.bootstrap_draws(5, 0, 7)) + list(M.bootstrap_draws(5, 1, 7)) == [1, 0, 4, 2, 2, 1, 2, 1, 0, 2]
    # the vectorised draws are the Python-int definition, term by term, also where k * U and the seed wrap
    for U, b, seed in ((5, 0, 7), (257, 3, 2 ** 64 - 5), (1000, 2 ** 20, 12345678901234567)):
        want = [((M.splitmix64(seed, b * U + j) >> 32) * U) >> 32 for j in range(U)]
        assert list(M.bootstrap_draws(U, b, seed)) == want


def test_counts_rows_sum_to_u_and_do_not_depend_on_chunking():
    for U in (1, 2, 65, 257):
        c = M.bootstrap_counts_reference(U, 8, 5)
        assert c.dtype == np.uint32 and c.shape == (8, U) and (c.sum(1) == U).all()
        assert np.array_equal(M.bootstrap_counts_reference(U, 3, 5, first=5), c[5:])
        assert np.array_equal(np.concatenate([M.bootstrap_counts_reference(U, 1, 5, first=r) for r in range(8)]), c)
        for r in range(8):
            assert np.array_equal(c[r], np.bincount(M.bootstrap_draws(U, r, 5), minlength=U))
    assert not np.array_equal(M.bootstrap_counts_reference(257, 2, 5), M.bootstrap_counts_reference(257, 2, 6))
    for bad in (0, (1 << 24) + 1):
        with pytest.raises(ValueError):
            M.bootstrap_counts_reference(bad, 1, 0)


@pytest.mark.parametrize("N", [2, 65, 257, 1000])
def test_weighted_auroc_is_the_auroc_of_the_materialised_resample(N):
    """Bound N * 2^-52: roc_curve / auc sum at most N trapezoids of size <= 1, each addition rounding by at most 2^-53 of a partial
    sum <= 1, and every one of the 2 N curve coordinates carries one division's rounding; the integer route has one rounding."""
    s, t = _case(N, 3, N)
    plan = M.bootstrap_plan(s, t)
    counts = M.bootstrap_counts_reference(N, 12, 3)
    num2, wpos, wneg = M.bootstrap_scan_reference(counts, plan["order"], plan["offs"], plan["lens"], N)
    got = M._auc_of(num2, wpos, wneg)
    # the scan over the two prepared orders is the definition (LT_i + LE_i from the sorted rows and their tie groups), in integers
    for a, b in zip((num2, wpos, wneg), M._definition_parts(s, t, plan["units"], counts)):
        assert np.array_equal(a.astype(np.int64), b)
    seen = 0
    for r in range(len(counts)):
        for c in range(3):
            keep = t[:, c] >= 0
            w = counts[r][keep]
            yt, ys = np.repeat(t[keep, c], w), np.repeat(s[keep, c], w)
            ref = M.auc(*M.roc_curve(yt, ys)[:2]) if len(yt) else float("nan")
            assert int(wpos[r, c]) == int((yt > 0.5).sum()) and int(wneg[r, c]) == int((yt <= 0.5).sum())
            if np.isnan(ref):
                assert np.isnan(got[r, c])
            else:
                seen += 1
                assert abs(got[r, c] - ref) <= N * 2.0 ** -52, (r, c, got[r, c], ref)
    assert seen > 0 or N == 2


def test_exact_values_degenerate_classes_and_ignored_rows():
    N = 64
    t = np.zeros((N, 4))
    t[N // 2:, :] = 1.0
    s = np.zeros((N, 4))
    s[:, 1] = np.arange(N)                        # class 1: perfectly separated
    s[:, 2] = -np.arange(N)                       # class 2: perfectly wrong
    t[:, 3] = 1.0                                 # class 3: no negatives
    r = M.bootstrap_auc_reference(s, t, n_boot=40, seed=2, return_replicates=True)
    rep = r["replicates"]
    assert rep.shape == (40, 4) and (rep[:, 0] == 0.5).all() and (rep[:, 1] == 1.0).all() and (rep[:, 2] == 0.0).all()
    assert np.isnan(rep[:, 3]).all() and r["n_degenerate"] == {0: 0, 1: 0, 2: 0, 3: 40}
    assert r["aucs"][0] == 0.5 and r["aucs"][1] == 1.0 and r["aucs"][2] == 0.0 and np.isnan(r["aucs"][3])
    assert (r["lo"][0], r["hi"][0], r["se"][0]) == (0.5, 0.5, 0.0) and np.isnan(r["lo"][3]) and np.isnan(r["se"][3])
    assert np.isnan(r["mean_auc"]["point"]) and np.isnan(r["mean_auc"]["lo"])          # a class is degenerate in every replicate
    json.dumps({k: v for k, v in r.items() if k != "replicates"})
    assert (r["n_boot"], r["seed"], r["alpha"], r["n_units"]) == (40, 2, 0.05, N)
    # rows with target -1 are left out of that class only: the class equals the same class of the data set without those rows'
    # labels, under the SAME draws (the units are the rows of the full table)
    s, t = _case(120, 2, 9, ignore=0.0)
    t2 = t.copy()
    t2[::3, 0] = -1.0
    a = M.bootstrap_auc_reference(s, t2, n_boot=30, seed=4, return_replicates=True)
    b = M.bootstrap_auc_reference(s, t, n_boot=30, seed=4, return_replicates=True)
    assert np.array_equal(a["replicates"][:, 1], b["replicates"][:, 1]) and not np.array_equal(a["replicates"][:, 0], b["replicates"][:, 0])
    counts = M.bootstrap_counts_reference(120, 30, 4)
    keep = t2[:, 0] >= 0
    for rr in range(30):
        w = counts[rr][keep]
        ref = M.auc(*M.roc_curve(np.repeat(t[keep, 0], w), np.repeat(s[keep, 0], w))[:2])
        assert abs(a["replicates"][rr, 0] - ref) <= 120 * 2.0 ** -52
    # the percentiles and the deviation are numpy's over the non-degenerate replicates
    v = a["replicates"][:, 0]
    assert a["lo"][0] == float(np.nanpercentile(v, 2.5)) and a["hi"][0] == float(np.nanpercentile(v, 97.5))
    assert a["se"][0] == float(np.std(v, ddof=1))
    m = a["replicates"].mean(1)
    assert a["mean_auc"]["lo"] == float(np.percentile(m, 2.5)) and a["mean_auc"]["point"] == float(np.mean([a["aucs"][0], a["aucs"][1]]))
    for bad in ({"n_boot": 0}, {"alpha": 0.0}, {"alpha": 1.0}):
        with pytest.raises(ValueError):
            M.bootstrap_auc_reference(s, t, **bad)


def test_groups_duplicated_rows_grouped_give_the_ungrouped_replicates():
    s, t = _case(90, 3, 21)
    a = M.bootstrap_auc_reference(s, t, n_boot=25, seed=6, return_replicates=True)
    ids = np.array(["p%03d/study1" % i for i in range(90)])
    perm = np.random.default_rng(1).permutation(180)
    s2, t2, g2 = np.concatenate([s, s])[perm], np.concatenate([t, t])[perm], np.concatenate([ids, ids])[perm]
    b = M.bootstrap_auc_reference(s2, t2, n_boot=25, seed=6, groups=g2, return_replicates=True)
    assert b["n_units"] == 90 == a["n_units"]
    assert np.array_equal(a["replicates"], b["replicates"], equal_nan=True)      # the same draws, every weight doubled
    assert a["aucs"] == b["aucs"]
    plan = M.bootstrap_plan(s2, t2, g2)
    assert plan["n_units"] == 90 and int(plan["lens"].sum()) == int((t2 >= 0).sum()) and plan["order"].dtype == np.int32
    assert np.array_equal(plan["offs"], np.concatenate([[0], np.cumsum(2 * plan["lens"].astype(np.int64))[:-1]]))
    assert ((plan["order"] & 0x7fffffff) < 90).all()
    with pytest.raises(ValueError):
        M.bootstrap_plan(s2, t2, g2[:-1])
    with pytest.raises(ValueError):
        M.bootstrap_plan(np.full((4, 1), np.nan), np.zeros((4, 1)))


def test_paired_difference_reference():
    s, t = _case(150, 3, 33)
    r = M.bootstrap_auc_diff_reference(s, s, t, n_boot=30, seed=1)
    for c in range(3):
        assert (r["delta"][c], r["lo"][c], r["hi"][c], r["p"][c]) == (0.0, 0.0, 0.0, 1.0)
    assert (r["mean_auc"]["delta"], r["mean_auc"]["lo"], r["mean_auc"]["hi"], r["mean_auc"]["p"]) == (0.0, 0.0, 0.0, 1.0)
    better = s + 3.0 * (t > 0.5)                                        # the positives pushed up: a clearly better model
    r = M.bootstrap_auc_diff_reference(better, s, t, n_boot=99, seed=1, return_replicates=True)
    d = r["replicates"]
    for c in range(3):
        assert r["delta"][c] > 0 and r["lo"][c] > 0 and r["p"][c] == 2.0 * 1.0 / 100.0         # no replicate at or below zero
        assert r["lo"][c] == float(np.percentile(d[:, c], 2.5))
    a = M.bootstrap_auc_reference(better, t, n_boot=99, seed=1, return_replicates=True)["replicates"]
    b = M.bootstrap_auc_reference(s, t, n_boot=99, seed=1, return_replicates=True)["replicates"]
    assert np.array_equal(d, a - b)                                     # paired: the same draws for both models


def test_entry_points_validate_without_launching():
    from chexpert_amd import _lib, ops
    EINVAL, EALIGN, ESHAPE = -1, -2, -3
    cnt_f, auc_f = _lib.lib().cx_boot_counts, _lib.lib().cx_boot_auc
    buf = (ctypes.c_uint64 * 64)()
    P = ctypes.addressof(buf)
    assert P % 8 == 0
    assert cnt_f(None, 8, 8, 0, 1, 0, None) == EINVAL
    assert cnt_f(P, 8, 8, 0, 0, 0, None) == EINVAL and cnt_f(P, 8, 8, -1, 1, 0, None) == EINVAL
    assert cnt_f(P, 8, 0, 0, 1, 0, None) == ESHAPE and cnt_f(P, 1 << 25, (1 << 24) + 1, 0, 1, 0, None) == ESHAPE
    assert cnt_f(P, 7, 8, 0, 1, 0, None) == ESHAPE                      # row pitch below U
    assert cnt_f(P + 2, 8, 8, 0, 1, 0, None) == EALIGN
    offs, lens = (ctypes.c_int64 * 2)(0, 8), (ctypes.c_int32 * 2)(4, 3)

    def auc(counts=P, ld=8, n_rep=1, order=P, offs=offs, lens=lens, C=2, num2=P, wpos=P, wneg=P, U=8):
        return auc_f(counts, ld, n_rep, order, offs, lens, C, num2, wpos, wneg, U, None)
    for name in ("counts", "order", "num2", "wpos", "wneg"):
        assert auc(**{name: None}) == EINVAL
    assert auc(offs=None) == EINVAL and auc(lens=None) == EINVAL
    assert auc(n_rep=0) == EINVAL and auc(C=0) == EINVAL and auc(C=-1) == EINVAL
    assert auc(lens=(ctypes.c_int32 * 2)(4, -1)) == EINVAL and auc(offs=(ctypes.c_int64 * 2)(0, -8)) == EINVAL
    assert auc(U=0) == ESHAPE and auc(U=(1 << 24) + 1, ld=1 << 25) == ESHAPE and auc(ld=7) == ESHAPE
    assert auc(num2=P + 4) == EALIGN and auc(order=P + 2) == EALIGN and auc(counts=P + 1) == EALIGN and auc(wpos=P + 2) == EALIGN
    # declared in the header with the parameters the binding passes, and built from its own source file
    hdr = open(os.path.join(ROOT, "include", "chexpert_hip.h")).read()
    code = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    for name, n in (("cx_boot_counts", 7), ("cx_boot_auc", 12)):
        m = re.search(r"\bint\s+%s\s*\(([^;{]*?)\)\s*;" % name, code, flags=re.S)
        assert m and len(_lib.SIGNATURES[name]) == m.group(1).count(",") + 1 == n
    assert "bootstrap.hip" in open(os.path.join(ROOT, "chexpert_amd", "csrc", "Makefile")).read()
    assert _lib.lib().cx_abi_version() == 10                            # additive entry points
    # the sizes at which the counts stage changes its form, as ops exports them, are the header's
    for name, v in (("CX_BOOT_TILE", ops.BOOT_TILE), ("CX_BOOT_MAX_TILES", ops.BOOT_MAX_TILES)):
        assert int(re.search(r"\b%s\s*=\s*(\d+)" % name, code).group(1)) == v
    assert ops.BOOT_MAX_UNITS == M.BOOT_MAX_UNITS == 1 << 24 and re.search(r"CX_BOOT_MAX_UNITS\s*=\s*1\s*<<\s*24", code)


def test_command_line_flags_and_config_round_trip(tmp_path):
    from chexpert_amd import cli
    a = cli.parse_args([])
    assert (a.bootstrap, a.bootstrap_seed, a.bootstrap_unit, a.bootstrap_alpha) == (0, None, "image", 0.05)
    a = cli.parse_args(["--evaluate", "--bootstrap", "500", "--bootstrap_seed", "9", "--bootstrap_unit", "patient", "--bootstrap_alpha", "0.1"])
    assert (a.bootstrap, a.bootstrap_seed, a.bootstrap_unit, a.bootstrap_alpha) == (500, 9, "patient", 0.1)
    for argv in (["--bootstrap", "-1"], ["--bootstrap", "10", "--bootstrap_alpha", "0"], ["--bootstrap_alpha", "1"],
                 ["--bootstrap_alpha", "nan"], ["--bootstrap_unit", "hospital"], ["--bootstrap", "x"],
                 ["--bootstrap", "10", "--bootstrap_unit", "study", "--synthetic", "64"],
                 ["--bootstrap", "10", "--bootstrap_unit", "patient", "--synthetic", "64"]):
        with pytest.raises(SystemExit):
            cli.parse_args(argv)
    cli.parse_args(["--bootstrap_unit", "study", "--synthetic", "64"])  # without --bootstrap the unit binds nothing
    path = tmp_path / "config.json"
    json.dump(a.__dict__, open(path, "w"), indent=4)
    b = cli.parse_args(["--load_config", str(path)])
    assert (b.bootstrap, b.bootstrap_seed, b.bootstrap_unit, b.bootstrap_alpha) == (500, 9, "patient", 0.1)
    cfg = json.load(open(path))
    cfg["bootstrap_alpha"] = 1.5
    json.dump(cfg, open(path, "w"))
    with pytest.raises(SystemExit):                                     # checked after the config is applied
        cli.parse_args(["--load_config", str(path)])


def test_command_line_file_name_groups_and_nothing_without_the_flag(tmp_path):
    import fnmatch

    import pandas as pd

    from chexpert_amd import cli
    for tag, want in (("eval_results_step_300", "auc_ci_step_300.json"), ("eval_results_ensemble", "auc_ci_ensemble.json")):
        assert cli.report_name(tag, "auc_ci") == want
        assert not fnmatch.fnmatch(want, "eval_results*") and not want.startswith("eval_results")      # --plot_roc globs that prefix
    # --bootstrap 0: nothing is computed (no GPU is touched: this test runs without one) and nothing is written
    a = cli.parse_args(["--evaluate", "--output_dir", str(tmp_path)])
    s, t = _case(20, 5, 1)
    assert cli.write_auc_ci(a, "eval_results_step_0", s, t) is None and os.listdir(tmp_path) == []
    assert cli.bootstrap_groups(a, object()) is None

    class Table:
        data = pd.DataFrame({"Path": ["CheXpert-v1.0-small/valid/patient1/study1/view1_frontal.jpg",
                                      "CheXpert-v1.0-small/valid/patient1/study1/view2_lateral.jpg",
                                      "CheXpert-v1.0-small/valid/patient1/study2/view1_frontal.jpg",
                                      "CheXpert-v1.0-small/valid/patient2/study1/view1_frontal.jpg"]}, index=[3, 5, 6, 9])
    study = cli.bootstrap_groups(cli.parse_args(["--bootstrap", "10", "--bootstrap_unit", "study"]), Table())
    patient = cli.bootstrap_groups(cli.parse_args(["--bootstrap", "10", "--bootstrap_unit", "patient"]), Table())
    assert list(study) == ["CheXpert-v1.0-small/valid/patient1/study1"] * 2 + ["CheXpert-v1.0-small/valid/patient1/study2",
                                                                                "CheXpert-v1.0-small/valid/patient2/study1"]
    assert list(patient) == ["CheXpert-v1.0-small/valid/patient1"] * 3 + ["CheXpert-v1.0-small/valid/patient2"]
    assert M.bootstrap_plan(s[:4], t[:4], study)["n_units"] == 3 and M.bootstrap_plan(s[:4], t[:4], patient)["n_units"] == 2
    a = cli.parse_args(["--bootstrap_unit", "study"])
    a.bootstrap = 10                                                    # (a dataset without paths reached past parse_args)
    with pytest.raises(ValueError, match="file paths"):
        cli.bootstrap_groups(a, object())
