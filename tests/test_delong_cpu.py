"""CPU (no GPU): the DeLong / Obuchowski variance of the AUROC and the paired test (chexpert_amd.metrics: delong_place_reference,
int_gram_reference, delong_auc_reference, delong_auc_diff_reference -- the statements the kernels of chexpert_amd/csrc/delong.hip are held
to in tests/test_delong_gpu.py) pinned by an O(M N) float64 DeLong written from the kernel psi(x, y) = 1, 1/2, 0, by the duplication
identity of the clustered form, by the bootstrap's standard error, the degenerate cases, the overflow guard, the argument checks of
the two entry points, and the command-line wiring."""
import ctypes
import json
import math
import os
import re

import numpy as np
import pytest

from chexpert_amd import metrics as M

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REL = 1e-12          # both sides are float64 sums of < 100 terms of magnitude <= 1 (1e-15 expected): room for the order of operations


def _case(N, C, seed, ignore=0.15):
    rng = np.random.default_rng(seed)
    t = (rng.random((N, C)) < 0.4).astype(np.float64)
    s = np.floor(np.clip(rng.normal(size=(N, C)) + 0.8 * t + 2.0, 0.0, 3.999) * 2.0) / 2.0       # 8 levels: ties abound
    t[rng.random((N, C)) < ignore] = -1.0
    return s, t


def _placements(s, t):
    """theta, V10 (one per positive), V01 (one per negative) of one class from psi(x, y) = 1 (x > y), 1/2 (x = y), 0 (x < y)."""
    pos, neg = s[t > 0.5], s[(t >= 0) & (t <= 0.5)]
    psi = (pos[:, None] > neg[None, :]) + 0.5 * (pos[:, None] == neg[None, :])
    return psi.mean(), psi.mean(1), psi.mean(0)


def _close(a, b):
    return (math.isnan(a) and math.isnan(b)) or abs(a - b) <= REL * max(abs(a), abs(b))


def test_reference_matches_the_brute_force_delong():
    s, t = _case(60, 3, 11)
    r = M.delong_auc_reference(s, t)
    assert r["method"] == "delong" and r["n_units"] == 60 and r["alpha"] == 0.05
    zq, cm = 1.959963984540054, M.compute_metrics(s, t, np.zeros_like(s))
    for c in range(3):
        th, v10, v01 = _placements(s[:, c], t[:, c])
        se = math.sqrt(v10.var(ddof=1) / len(v10) + v01.var(ddof=1) / len(v01))
        assert len(v10) > 5 and len(v01) > 5
        assert _close(r["aucs"][c], th) and _close(r["se"][c], se)
        assert _close(r["lo"][c], max(th - zq * se, 0.0)) and _close(r["hi"][c], min(th + zq * se, 1.0))
        assert (r["n_pos"][c], r["n_neg"][c], r["n_units_pos"][c], r["n_units_neg"][c]) == (len(v10), len(v01), len(v10), len(v01))
        assert _close(r["aucs"][c], cm["aucs"][c])                      # the trapezoid area of the evaluation
    assert _close(r["mean_auc"]["point"], np.mean([r["aucs"][c] for c in range(3)]))
    assert 0.0 < r["mean_auc"]["se"] < max(r["se"].values()) and r["mean_auc"]["lo"] < r["mean_auc"]["point"] < r["mean_auc"]["hi"]
    json.dumps(r)


def test_paired_reference_matches_the_brute_force_covariance():
    sa, t = _case(60, 3, 12)
    sb = np.floor((sa + np.random.default_rng(5).normal(size=sa.shape)) * 2.0) / 2.0
    r = M.delong_auc_diff_reference(sa, sb, t)
    ra, rb = M.delong_auc_reference(sa, t), M.delong_auc_reference(sb, t)
    for c in range(3):
        tha, a10, a01 = _placements(sa[:, c], t[:, c])
        thb, b10, b01 = _placements(sb[:, c], t[:, c])
        S10, S01 = np.cov(np.stack([a10, b10]), ddof=1), np.cov(np.stack([a01, b01]), ddof=1)
        S = S10 / len(a10) + S01 / len(a01)
        var = S[0, 0] + S[1, 1] - 2.0 * S[0, 1]
        z = (tha - thb) / math.sqrt(var)
        assert _close(ra["se"][c], math.sqrt(S[0, 0])) and _close(rb["se"][c], math.sqrt(S[1, 1]))
        assert _close(r["delta"][c], tha - thb) and _close(r["se"][c], math.sqrt(var))
        assert _close(r["z"][c], z) and _close(r["p"][c], math.erfc(abs(z) / math.sqrt(2.0))) and r["degenerate"][c] is False
        assert r["lo"][c] < r["delta"][c] < r["hi"][c]
    assert _close(r["mean_auc"]["delta"], ra["mean_auc"]["point"] - rb["mean_auc"]["point"])
    m = r["mean_auc"]
    assert m["se"] > 0 and _close(m["z"], m["delta"] / m["se"]) and _close(m["p"], math.erfc(abs(m["z"]) / math.sqrt(2.0)))
    json.dumps(r)


def test_duplicated_rows_in_one_group_give_the_ungrouped_errors():
    s, t = _case(60, 3, 13)
    r = M.delong_auc_reference(s, t)
    g = M.delong_auc_reference(np.repeat(s, 3, axis=0), np.repeat(t, 3, axis=0), groups=np.repeat(np.arange(60), 3))
    assert g["method"] == "obuchowski" and g["n_units"] == 60
    for c in range(3):
        assert g["aucs"][c] == r["aucs"][c] and _close(g["se"][c], r["se"][c])
        assert g["n_pos"][c] == 3 * r["n_pos"][c] and g["n_units_pos"][c] == r["n_units_pos"][c]
    assert g["mean_auc"]["point"] == r["mean_auc"]["point"] and _close(g["mean_auc"]["se"], r["mean_auc"]["se"])
    sb = np.roll(s, 7, axis=0) * 0.5 + s * 0.5
    d = M.delong_auc_diff_reference(s, sb, t)
    e = M.delong_auc_diff_reference(np.repeat(s, 3, axis=0), np.repeat(sb, 3, axis=0), np.repeat(t, 3, axis=0), groups=np.repeat(np.arange(60), 3))
    for c in range(3):
        assert e["delta"][c] == d["delta"][c] and _close(e["se"][c], d["se"][c]) and _close(e["p"][c], d["p"][c])


def test_one_group_per_row_is_the_ungrouped_result():
    s, t = _case(60, 3, 14)
    a, b = M.delong_auc_reference(s, t), M.delong_auc_reference(s, t, groups=np.arange(60))
    assert b.pop("method") == "obuchowski" and a.pop("method") == "delong"
    assert json.dumps(a) == json.dumps(b)                               # float for float


def _correlated(N, C, seed, per):
    """score = label + unit effect + noise over units of `per` consecutive rows (positives and negatives inside a unit)."""
    rng = np.random.default_rng(seed)
    t = (rng.random((N, C)) < 0.4).astype(np.float64)
    unit = np.arange(N) // per
    s = t + np.repeat(rng.normal(size=(N // per, C)), per, axis=0) * 0.8 + rng.normal(size=(N, C)) * 0.6
    return s, t, unit


def test_standard_error_agrees_with_the_bootstrap():
    """Measured: se(DeLong) / se(bootstrap, B = 2000) for class 0, class 1 and the mean = 0.9971, 0.9957, 0.9693 without groups and
    1.0158, 1.0112, 1.0093 with units of three rows.  The bootstrap's own Monte-Carlo error is 1 / sqrt(2 B) = 1.6 %, the estimators
    differ by O(1 / N): the ratio is held inside 10 %."""
    s, t, unit = _correlated(600, 2, 21, 3)
    for groups in (None, unit):
        d = M.delong_auc_reference(s, t, groups=groups)
        b = M.bootstrap_auc_reference(s, t, n_boot=2000, seed=3, groups=groups)
        ratios = [d["se"][c] / b["se"][c] for c in range(2)] + [d["mean_auc"]["se"] / b["mean_auc"]["se"]]
        print("delong / bootstrap se, groups=%s: %s" % ("None" if groups is None else "3 rows", ["%.4f" % v for v in ratios]))
        assert all(abs(v - 1.0) < 0.10 for v in ratios), ratios
    # the grouping matters on this data (the unit sums and the S11 term are exercised): the clustered error is another number
    a, g = M.delong_auc_reference(s, t), M.delong_auc_reference(s, t, groups=unit)
    assert all(abs(g["se"][c] / a["se"][c] - 1.0) > 0.02 for c in range(2))


def test_degenerate_classes():
    s, t = _case(40, 3, 15, ignore=0.0)
    t[:, 0] = 0.0                                                       # class 0: no positive
    t[:, 1] = 0.0
    t[5, 1] = 1.0                                                       # class 1: one positive (unit)
    r = M.delong_auc_reference(s, t)
    assert math.isnan(r["aucs"][0]) and math.isnan(r["se"][0]) and math.isnan(r["lo"][0]) and math.isnan(r["hi"][0])
    assert not math.isnan(r["aucs"][1]) and math.isnan(r["se"][1]) and math.isnan(r["lo"][1]) and r["n_units_pos"][1] == 1
    assert not math.isnan(r["se"][2])
    assert all(math.isnan(v) for v in r["mean_auc"].values())          # the rule of _row_mean
    # one positive UNIT of several rows is as degenerate as one positive row
    t[6, 1] = 1.0
    g = np.arange(40)
    g[6] = 5
    r = M.delong_auc_reference(s[:, 1:], t[:, 1:], groups=g)
    assert r["n_pos"][0] == 2 and r["n_units_pos"][0] == 1 and math.isnan(r["se"][0]) and not math.isnan(r["mean_auc"]["point"])
    # identical models: Var(delta) is exactly 0
    s, t = _case(40, 2, 16)
    d = M.delong_auc_diff_reference(s, s.copy(), t)
    for c in range(2):
        assert d["delta"][c] == 0.0 and d["se"][c] == 0.0 and d["degenerate"][c] is True and math.isnan(d["z"][c]) and math.isnan(d["p"][c])
    assert d["mean_auc"]["delta"] == 0.0 and math.isnan(d["mean_auc"]["z"]) and math.isnan(d["mean_auc"]["p"])
    # a single row
    r = M.delong_auc_reference(np.array([[0.3]]), np.array([[1.0]]))
    assert math.isnan(r["aucs"][0]) and math.isnan(r["se"][0]) and math.isnan(r["mean_auc"]["se"]) and r["n_units"] == 1
    d = M.delong_auc_diff_reference(np.array([[0.3]]), np.array([[0.1]]), np.array([[1.0]]))
    assert math.isnan(d["delta"][0]) and math.isnan(d["p"][0]) and d["degenerate"][0] is False
    for bad in (0.0, 1.0, float("nan")):
        with pytest.raises(ValueError, match="alpha"):
            M.delong_auc_reference(s, t, alpha=bad)
    with pytest.raises(ValueError, match="NaN"):                        # bootstrap_plan's input errors
        M.delong_auc_reference(np.full((4, 1), np.nan), np.ones((4, 1)))
    with pytest.raises(ValueError, match="table rows"):
        M.delong_auc_diff_reference(np.zeros((4, 17)), np.zeros((4, 17)), np.ones((4, 17)))


def test_hand_computed_table_and_gram():
    # one class, scores 1 2 2 3 3, labels - + - + -, units 0 0 1 1 2
    s, t = np.array([[1.0], [2.0], [2.0], [3.0], [3.0]]), np.array([[0.0], [1.0], [0.0], [1.0], [0.0]])
    p = M.bootstrap_plan(s, t, groups=[0, 0, 1, 1, 2])
    z = M.delong_place_reference(p["order"], p["offs"], p["lens"], 3)
    # X2: row 1 (score 2): 2 * 1 + 1 = 3; row 3 (score 3): 2 * 2 + 1 = 5.  Y2: row 0: 4; row 2: 2 * 1 + 1 = 3; row 4: 1
    assert z.dtype == np.int64 and z.tolist() == [[3, 5, 0], [1, 1, 0], [4, 3, 1], [1, 1, 1]]
    assert z[0].sum() == z[2].sum() == 8                                # num2; theta = 8 / 12
    g = M.int_gram_reference(z)
    assert g.dtype == np.int64 and g.tolist() == (z.astype(object) @ z.astype(object).T).tolist()
    big = np.array([[1 << 40, 3], [-(1 << 35), 1 << 33]], dtype=np.int64)
    want = [[((int(a) * int(c) + int(b) * int(d) + (1 << 63)) % (1 << 64)) - (1 << 63) for c, d in big] for a, b in big]
    assert M.int_gram_reference(big).tolist() == want                   # wrapping is the definition
    assert M.int_gram_reference(np.concatenate([big, big], 1), 2).tolist() == want


def test_overflow_guard_raises_before_anything_runs():
    N = 40000                                                           # one unit of N rows: 4 N^2 * N^2 >= 2^63 from N = 38968
    s, t = np.arange(N, dtype=np.float64)[:, None] % 17, (np.arange(N) % 3 == 0).astype(np.float64)[:, None]
    with pytest.raises(ValueError, match="overflow"):
        M.delong_auc_reference(s, t, groups=np.zeros(N, dtype=np.int64))
    with pytest.raises(ValueError, match="overflow"):
        M.delong_auc(s, t, groups=np.zeros(N, dtype=np.int64))          # before any launch: no GPU is touched
    M.delong_auc_reference(s[:3000], t[:3000], groups=np.zeros(3000, dtype=np.int64))


def test_entry_points_validate_without_launching():
    from chexpert_amd import _lib, ops
    EINVAL, EALIGN, ESHAPE = -1, -2, -3
    place_f, gram_f = _lib.lib().cx_delong_place, _lib.lib().cx_delong_gram
    buf = (ctypes.c_uint64 * 64)()
    P = ctypes.addressof(buf)
    assert P % 8 == 0
    offs, lens = (ctypes.c_int64 * 2)(0, 8), (ctypes.c_int32 * 2)(4, 3)

    def place(order=P, offs=offs, lens=lens, C=2, U=8, z=P, ldz=8):
        return place_f(order, offs, lens, C, U, z, ldz, None)
    for name in ("order", "offs", "lens", "z"):
        assert place(**{name: None}) == EINVAL
    assert place(C=0) == EINVAL and place(C=-1) == EINVAL
    assert place(lens=(ctypes.c_int32 * 2)(4, -1)) == EINVAL and place(offs=(ctypes.c_int64 * 2)(0, -8)) == EINVAL
    assert place(U=0) == ESHAPE and place(U=(1 << 24) + 1, ldz=1 << 25) == ESHAPE and place(ldz=7) == ESHAPE
    assert place(order=P + 2) == EALIGN and place(z=P + 4) == EALIGN

    def gram(z=P, ldz=8, Q=4, U=8, g=P):
        return gram_f(z, ldz, Q, U, g, None)
    assert gram(z=None) == EINVAL and gram(g=None) == EINVAL
    assert gram(Q=0) == ESHAPE and gram(Q=129) == ESHAPE and gram(U=0) == ESHAPE and gram(U=(1 << 24) + 1, ldz=1 << 25) == ESHAPE
    assert gram(ldz=7) == ESHAPE
    assert gram(z=P + 4) == EALIGN and gram(g=P + 4) == EALIGN
    # declared in the header with the parameters the binding passes, and built from its own source file
    hdr = open(os.path.join(ROOT, "include", "chexpert_hip.h")).read()
    code = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    for name, n in (("cx_delong_place", 8), ("cx_delong_gram", 6)):
        m = re.search(r"\bint\s+%s\s*\(([^;{]*?)\)\s*;" % name, code, flags=re.S)
        assert m and len(_lib.SIGNATURES[name]) == m.group(1).count(",") + 1 == n
    assert "delong.hip" in open(os.path.join(ROOT, "chexpert_amd", "csrc", "Makefile")).read()
    assert _lib.lib().cx_abi_version() == 10                            # additive entry points
    for name, v in (("CX_DELONG_MAX_ROWS", ops.DELONG_MAX_ROWS), ("CX_DELONG_WG_ENTRIES", ops.DELONG_WG_ENTRIES),
                    ("CX_DELONG_TILE", ops.DELONG_TILE)):
        assert int(re.search(r"\b%s\s*=\s*(\d+)" % name, code).group(1)) == v
    assert ops.DELONG_MAX_ROWS == M.DELONG_MAX_ROWS == 4 * 16 * 2


def test_command_line_flag_config_round_trip_and_file_name(tmp_path):
    import fnmatch

    from chexpert_amd import cli
    assert cli.parse_args([]).delong is False
    a = cli.parse_args(["--evaluate_single_model", "--delong", "--bootstrap_unit", "patient", "--bootstrap_alpha", "0.1"])
    assert a.delong is True and a.bootstrap == 0 and a.bootstrap_unit == "patient" and a.bootstrap_alpha == 0.1
    for unit in ("study", "patient"):
        with pytest.raises(SystemExit):                                 # the bootstrap's refusal: synthetic images have no paths
            cli.parse_args(["--delong", "--bootstrap_unit", unit, "--synthetic", "64"])
    cli.parse_args(["--delong", "--synthetic", "64"])
    cli.parse_args(["--bootstrap_unit", "study", "--synthetic", "64"])  # without --delong (or --bootstrap) the unit binds nothing
    path = tmp_path / "config.json"
    json.dump(a.__dict__, open(path, "w"), indent=4)
    b = cli.parse_args(["--load_config", str(path)])
    assert b.delong is True and b.bootstrap_unit == "patient" and b.bootstrap_alpha == 0.1
    for tag, want in (("eval_results_step_300", "delong_step_300.json"), ("eval_results_ensemble", "delong_ensemble.json")):
        assert cli.report_name(tag, "delong") == want
        assert not fnmatch.fnmatch(want, "eval_results*") and not want.startswith("eval_results")      # --plot_roc globs that prefix
    # without --delong: nothing is computed (no GPU is touched: this test runs without one) and nothing is written
    a = cli.parse_args(["--evaluate_single_model", "--output_dir", str(tmp_path / "out")])
    os.makedirs(a.output_dir, exist_ok=True)
    s, t = _case(20, 5, 1)
    assert cli.write_delong(a, "eval_results_step_0", s, t) is None and os.listdir(a.output_dir) == []
    # the units come through the existing bootstrap_groups
    assert cli.bootstrap_groups(cli.parse_args(["--delong"]), object()) is None
