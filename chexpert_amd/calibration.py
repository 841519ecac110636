"""Calibration of the predicted probabilities: Platt / temperature scaling fit, ECE, MCE and Brier score with bootstrap intervals
(chexpert_amd/csrc/calib.hip).

Inputs are those of metrics.py: `outputs` (N, C) raw logits (bf16 / fp16 go through `_as_scores`), `targets` (N, C); a row with
target < 0 is left out of that class, a row is positive iff target > 0.5.

Calibration map, per class c: u = a_c z + b_c, p = sigmoid(u).  method "temperature": b_c = 0, only a_c is fitted and T_c = 1 / a_c
is reported; "platt": both.  The identity is a = 1, b = 0.
Fit objective, per class over its kept rows, in float64 on the float32 logits: the mean of softplus(u) - t u with
softplus(u) = max(u, 0) + log1p(exp(-|u|)); t is the 0 / 1 label or, smooth=True, Platt's targets t+ = (N+ + 1) / (N+ + 2),
t- = 1 / (N- + 2).  Solver: damped Newton from the identity on the gradient g and Hessian H of the mean loss, step
d = (H + 1e-12 I)^-1 g, halved while the loss rises, at most 40 halvings ("rises": the candidate's loss exceeds L (1 + 1e-12) -- a
difference below the rounding of an N-term float64 sum is no rise, so a step at the noise floor is taken whole whatever the order
of the sum); stop when max |g| <= g_tol or after max_iter iterations.
Status per class: 0 converged; 1 iteration cap reached, the parameters are kept; 2 degenerate (no kept row, no positive or no
negative), the identity is returned; 3 flat: the smallest eigenvalue of the mean Hessian at the end is below 1e-8 (separable or
nearly separable data), the identity is returned -- smooth=True is the cure.

Fixed-point probability: P = min(floor(p 2^32), 2^32 - 1) as uint32, p computed on the host in float64 from the map (exp on the
device would not be bit-equal).  Everything after this point is integers.
Bins, M from 1 to 64: binning "width": bin = (P M) >> 32; "mass": the class's kept rows sorted ascending by P, a row whose first
equal-P position is k of n gets bin = (k M) // n (equal-mass bins of the data set itself, ties kept in one bin).  Bins are a
property of the scores alone: they do not move with a replicate.
Per replicate, class and bin, with row weight w = counts[unit(row)]: wsum_b = sum w, wpos_b = sum w over the positives (uint32),
csum_b = sum w P (uint64).  Per replicate and class: bnum = sum w umulhi(d, d), d = 2^32 - 1 - P for a positive and P for a
negative (uint64); W = sum_b wsum_b.
Values (float64, formed on the host by `_calibration_values` from these exact integers, GPU path and reference path alike):
  G_b = |wpos_b 2^32 - csum_b| (uint64, exact);  ECE = float64(sum_b G_b) / (float64(W) 2^32);
  MCE = max over wsum_b > 0 of float64(G_b) / (float64(wsum_b) 2^32);  Brier = float64(bnum) / (float64(W) 2^32), below the exact
  value by less than 2^-31.  All three NaN iff W = 0.
The `*_reference` functions are the numpy statements the kernels are held to; `fit_calibration` and `calibration_metrics` run on the
GPU only.
"""
import numpy as np

from ._lib import CALIB_MAX_BINS as MAX_BINS
from ._lib import CALIB_MAX_ITER as MAX_ITER
from ._lib import CALIB_METHODS
from .resample import _check_boot, _check_inputs, _check_scores, _pack_lists, _replicates, _summarise_metric

METHODS = tuple(CALIB_METHODS)            # ("temperature", "platt")
BINNINGS = ("width", "mass")
_HALVINGS, _RIDGE, _FLAT, _SLACK = 40, 1e-12, 1e-8, 1e-12
_FIT_COLUMNS = ("a", "b", "nll_before", "nll_after", "gmax", "lambda_min", "iterations", "status")


def _check_fit(method, g_tol, max_iter):
    if method not in METHODS:
        raise ValueError("calibration: method %r (one of %s)" % (method, METHODS))
    if not 1 <= int(max_iter) <= MAX_ITER:
        raise ValueError("calibration: max_iter must be inside 1 .. %d (got %r)" % (MAX_ITER, max_iter))
    if not float(g_tol) >= 0.0:
        raise ValueError("calibration: g_tol must be >= 0 (got %r)" % (g_tol,))


def _inputs(outputs, targets, *groups):
    """The checked inputs with the logits in float32: (s, t), or (s, t, units, U) when the rows' groups (or None) are given."""
    s, *rest = _check_inputs(outputs, targets, *groups, "calibration") if groups else _check_scores(outputs, targets, "calibration")
    return (np.asarray(s, dtype=np.float32), *rest)


def _fit_terms(z, t, a, b, full=True):
    """Mean loss (and gradient, Hessian entries) of the map (a, b) on float64 logits z against targets t."""
    u = a * z + b
    e = np.exp(-np.abs(u))
    loss = float(np.mean((np.maximum(u, 0.0) + np.log1p(e)) - t * u))
    if not full:
        return loss
    q = 1.0 / (1.0 + e)
    p, w = np.where(u >= 0.0, q, e * q), e * q * q
    r = p - t
    return loss, float(np.mean(r * z)), float(np.mean(r)), float(np.mean(w * z * z)), float(np.mean(w * z)), float(np.mean(w))


def _fit_class(z, y, platt, smooth, g_tol, max_iter):
    """One class of fit_calibration_reference: the row (a, b, nll_before, nll_after, gmax, lambda_min, iterations, status)."""
    nan = float("nan")
    keep = y >= 0
    z, pos = z[keep].astype(np.float64), y[keep] > 0.5
    n_pos, n_neg = int(pos.sum()), int((~pos).sum())
    if n_pos + n_neg == 0:
        return [1.0, 0.0, nan, nan, nan, nan, 0.0, 2.0]
    t_pos, t_neg = ((n_pos + 1.0) / (n_pos + 2.0), 1.0 / (n_neg + 2.0)) if smooth else (1.0, 0.0)
    t = np.where(pos, t_pos, t_neg)
    a, b, it = 1.0, 0.0, 0
    L, ga, gb, haa, hab, hbb = _fit_terms(z, t, a, b)
    nll0 = L
    if n_pos == 0 or n_neg == 0:
        return [1.0, 0.0, nll0, nll0, nan, nan, 0.0, 2.0]
    while True:
        if not platt:
            gb = 0.0
        gmax = max(abs(ga), abs(gb))
        lmin = 0.5 * (haa + hbb) - np.sqrt(0.25 * (haa - hbb) * (haa - hbb) + hab * hab) if platt else haa
        if gmax <= g_tol:
            status = 0
            break
        if it >= max_iter:
            status = 1
            break
        if platt:
            h00, h11 = haa + _RIDGE, hbb + _RIDGE
            det = h00 * h11 - hab * hab
            da, db = (h11 * ga - hab * gb) / det, (h00 * gb - hab * ga) / det
        else:
            da, db = ga / (haa + _RIDGE), 0.0
        step, halvings = 1.0, 0
        while True:
            ca, cb = a - step * da, b - step * db
            Lc = _fit_terms(z, t, ca, cb, full=False)
            finite = bool(np.isfinite(Lc))
            if finite and Lc <= L + _SLACK * abs(L):
                a, b = ca, cb
                break
            if halvings >= _HALVINGS:
                if finite:
                    a, b = ca, cb
                break
            step, halvings = step * 0.5, halvings + 1
        it += 1
        L, ga, gb, haa, hab, hbb = _fit_terms(z, t, a, b)
    nll1 = L
    if not lmin >= _FLAT:
        status = 3
    if status == 3:
        a, b, nll1 = 1.0, 0.0, nll0
    return [a, b, nll0, nll1, gmax, float(lmin), float(it), float(status)]


def _fit_dict(rows, method, smooth):
    rows = np.asarray(rows, dtype=np.float64).reshape(-1, 8)
    out = {"method": method, "smooth": bool(smooth)}
    for k, name in enumerate(_FIT_COLUMNS):
        out[name] = {c: (int(rows[c, k]) if name in ("iterations", "status") else float(rows[c, k])) for c in range(len(rows))}
    out["temperature"] = {c: (1.0 / out["a"][c] if out["a"][c] != 0.0 else float("inf")) for c in range(len(rows))}
    return out


def fit_calibration_reference(outputs, targets, method="temperature", smooth=False, g_tol=1e-10, max_iter=100):
    """The numpy statement of fit_calibration: the same iteration on the host, float64 numpy sums."""
    _check_fit(method, g_tol, max_iter)
    s, t = _inputs(outputs, targets)
    rows = [_fit_class(s[:, c], t[:, c], method == "platt", bool(smooth), float(g_tol), int(max_iter)) for c in range(s.shape[1])]
    return _fit_dict(rows, method, smooth)


def fit_calibration(outputs, targets, method="temperature", smooth=False, g_tol=1e-10, max_iter=100, device="cuda"):
    """Fits the per-class calibration map on the GPU (cx_calib_fit: every class in one launch; no CPU fallback).  Returns a
    json-serialisable dict, int class keys as in compute_metrics: method, smooth, a, b, temperature (1 / a), nll_before, nll_after
    (mean loss at the identity / at the returned parameters), iterations, status (0 converged, 1 iteration cap, 2 degenerate,
    3 flat; 2 and 3 return the identity), lambda_min, gmax."""
    import torch

    from . import ops
    _check_fit(method, g_tol, max_iter)
    s, t = _inputs(outputs, targets)
    rows = ops.calib_fit(torch.from_numpy(s).to(device), torch.from_numpy(t.astype(np.float32)).to(device), method, smooth, g_tol, max_iter)
    return _fit_dict(rows.cpu().numpy(), method, smooth)


def _map_of(cal, n_cls):
    """(a, b) float64 arrays of C classes from a fit dict (int or str class keys: a json round trip makes them strings); None: identity."""
    if cal is None:
        return np.ones(n_cls), np.zeros(n_cls)

    def column(name):
        d = cal[name]
        if len(d) != n_cls:
            raise ValueError("calibration: the fit holds %d classes, the outputs %d" % (len(d), n_cls))
        return np.array([float(d[c] if c in d else d[str(c)]) for c in range(n_cls)], dtype=np.float64)
    return column("a"), column("b")


def apply_calibration(outputs, cal):
    """The calibrated logits a z + b in float64 (numpy in, numpy out; torch in, torch out on the input's device).  The identity for
    the classes of status 2 / 3 falls out of their a, b."""
    if hasattr(outputs, "detach"):
        import torch
        a, b = _map_of(cal, outputs.shape[-1])
        return outputs.double() * torch.from_numpy(a).to(outputs.device) + torch.from_numpy(b).to(outputs.device)
    z = np.asarray(outputs, dtype=np.float64)
    a, b = _map_of(cal, z.shape[-1])
    return z * a + b


def _sigmoid64(u):
    e = np.exp(-np.abs(u))
    return np.where(u >= 0.0, 1.0 / (1.0 + e), e / (1.0 + e))


def fixed_point(p):
    """P = min(floor(p 2^32), 2^32 - 1) as uint64 values below 2^32 (p float64 inside [0, 1]; p 2^32 is exact)."""
    return np.minimum(np.floor(np.asarray(p, dtype=np.float64) * 2.0 ** 32), 2.0 ** 32 - 1).astype(np.uint64)


def _check_bins(bins, binning):
    if binning not in BINNINGS:
        raise ValueError("calibration: binning %r (one of %s)" % (binning, BINNINGS))
    if not 1 <= int(bins) <= MAX_BINS:
        raise ValueError("calibration: %r bins (1 .. %d are supported)" % (bins, MAX_BINS))
    return int(bins)


def _bins_of(P, M, binning):
    """Bin of every kept row of one class from its fixed-point confidences (uint64 values below 2^32)."""
    if binning == "width":
        return ((P * np.uint64(M)) >> np.uint64(32)).astype(np.int64)
    first = np.searchsorted(np.sort(P), P, side="left").astype(np.int64)       # the first equal-P position in the sorted class
    return (first * M) // max(len(P), 1)


def calibration_plan(outputs, targets, groups=None, cal=None, bins=15, binning="width"):
    """What cx_boot_calib reads, built once per call on the host: for every class the kept rows (target >= 0) ascending in the
    fixed-point confidence P of the map `cal` (None: the identity), so ascending in bin, then in row index.  An entry is the row's
    unit index in bits 0-23, its bin in bits 24-29 and its label (target > 0.5) in bit 31; `conf` holds P in parallel.
    Returns {"order": int32, "conf": uint32, "offs": int64 (C), "lens": int32 (C), "units", "n_units", "bins", "binning"}."""
    M = _check_bins(bins, binning)
    s, t, units, U = _inputs(outputs, targets, groups)
    a, b = _map_of(cal, s.shape[1])
    parts, confs = [], []
    for c in range(s.shape[1]):
        keep = np.nonzero(t[:, c] >= 0)[0]
        P = fixed_point(_sigmoid64(a[c] * s[keep, c].astype(np.float64) + b[c]))
        by = np.lexsort((keep, P))                                # ascending P (and with it bin), then row
        entry = units[keep] | (_bins_of(P, M, binning) << 24) | ((t[keep, c] > 0.5).astype(np.int64) << 31)
        parts.append(entry[by].astype(np.uint32).view(np.int32))
        confs.append(P[by].astype(np.uint32))
    order, offs, lens = _pack_lists(parts)
    return {"order": order, "conf": _pack_lists(confs, np.uint32)[0], "offs": offs, "lens": lens, "units": units, "n_units": U, "bins": M,
            "binning": binning}


def calibration_sums_reference(counts, plan, n_units=None):
    """Statement of cx_boot_calib in uint64 numpy, vectorised over the replicates: (wsum, wpos, csum) (n_rep, C, M) and bnum
    (n_rep, C), all uint64.  Unit indices are clamped to n_units - 1 (default: the plan's) and bins to M - 1, as the kernel does."""
    counts, u64 = np.asarray(counts).astype(np.uint64), np.uint64
    order, conf = np.asarray(plan["order"], dtype=np.int32), np.asarray(plan["conf"]).astype(u64)
    U, M = int(plan["n_units"] if n_units is None else n_units), int(plan["bins"])
    R, C = counts.shape[0], len(plan["lens"])
    wsum, wpos, csum = (np.zeros((R, C, M), dtype=u64) for _ in range(3))
    bnum = np.zeros((R, C), dtype=u64)
    for c in range(C):
        o, n = int(plan["offs"][c]), int(plan["lens"][c])
        e, P = order[o:o + n], conf[o:o + n]
        w = counts[:, np.minimum(e & 0xffffff, U - 1)]
        pos, bins = e < 0, np.minimum((e >> 24) & 63, M - 1)
        d = np.where(pos, u64(0xffffffff) - P, P)
        bnum[:, c] = (w * ((d * d) >> u64(32))).sum(1, dtype=u64)
        for k in range(M):
            sel = bins == k
            wsum[:, c, k] = w[:, sel].sum(1, dtype=u64)
            wpos[:, c, k] = w[:, sel & pos].sum(1, dtype=u64)
            csum[:, c, k] = (w[:, sel] * P[sel]).sum(1, dtype=u64)
    return wsum, wpos, csum, bnum


def _calibration_definition(outputs, targets, counts, groups=None, cal=None, bins=15, binning="width"):
    """(wsum, wpos, csum, bnum) straight from the definition, in Python integers (object arrays): no prepared plan, no sorted order, a
    loop over the rows."""
    M = _check_bins(bins, binning)
    s, t, units, U = _inputs(outputs, targets, groups)
    a, b = _map_of(cal, s.shape[1])
    counts = np.asarray(counts).astype(np.int64)
    R, C = counts.shape[0], s.shape[1]
    wsum, wpos, csum = (np.zeros((R, C, M), dtype=object) for _ in range(3))
    bnum = np.zeros((R, C), dtype=object)
    for c in range(C):
        rows = [i for i in range(s.shape[0]) if t[i, c] >= 0]
        P = [int(v) for v in fixed_point(_sigmoid64(a[c] * s[rows, c].astype(np.float64) + b[c]))]
        if binning == "width":
            where = [(p * M) >> 32 for p in P]
        else:
            ranked = sorted(P)
            where = [(ranked.index(p) * M) // len(P) for p in P]
        for r in range(R):
            for i, p, k in zip(rows, P, where):
                w, pos = int(counts[r, units[i]]), t[i, c] > 0.5
                wsum[r, c, k] += w
                wpos[r, c, k] += w if pos else 0
                csum[r, c, k] += w * p
                d = (2 ** 32 - 1 - p) if pos else p
                bnum[r, c] += w * ((d * d) >> 32)
    return wsum, wpos, csum, bnum


def _u64(a):
    a = np.asarray(a)
    return a.view(np.uint64) if a.dtype == np.int64 else a.astype(np.uint64)      # int64: the kernel's uint64 bits


def _calibration_values(wsum, wpos, csum, bnum):
    """{"ece", "mce", "brier"}: (n_rep, C) float64 from the exact integers (the one place that forms them, for both paths), and
    "weight": W (n_rep, C) uint64.  wpos_b < 2^32, so wpos_b 2^32 and G_b are exact in uint64; sum_b G_b <= W 2^32 fits; every float64
    conversion rounds once and so does every quotient."""
    wsum, wpos, csum, bnum = _u64(wsum), _u64(wpos), _u64(csum), _u64(bnum)
    lhs = wpos << np.uint64(32)
    G = np.where(lhs >= csum, lhs - csum, csum - lhs)
    W = wsum.sum(axis=2, dtype=np.uint64)
    Wf, two32 = W.astype(np.float64), 2.0 ** 32
    live = W > 0
    with np.errstate(divide="ignore", invalid="ignore"):
        den = np.where(live, Wf, 1.0) * two32
        ece = np.where(live, G.sum(axis=2, dtype=np.uint64).astype(np.float64) / den, np.nan)
        brier = np.where(live, bnum.astype(np.float64) / den, np.nan)
        per_bin = np.where(wsum > 0, G.astype(np.float64) / (np.where(wsum > 0, wsum, 1).astype(np.float64) * two32), 0.0)
        mce = np.where(live, per_bin.max(axis=2, initial=0.0), np.nan)
    return {"ece": ece, "mce": mce, "brier": brier, "weight": W}


def _reliability(wsum, wpos, csum, bins, binning):
    """The reliability curve of the point sample (row 0 of the sums): per class and bin the weight, the fraction positive
    wpos_b / wsum_b and the mean confidence csum_b / (wsum_b 2^32); NaN in an empty bin."""
    wsum, wpos, csum = _u64(wsum)[0], _u64(wpos)[0], _u64(csum)[0]
    live = wsum > 0
    den = np.where(live, wsum, 1).astype(np.float64)
    frac = np.where(live, wpos.astype(np.float64) / den, np.nan)
    conf = np.where(live, csum.astype(np.float64) / (den * 2.0 ** 32), np.nan)
    C = wsum.shape[0]
    return {"bins": int(bins), "binning": binning, "weight": {c: [int(v) for v in wsum[c]] for c in range(C)},
            "frac_pos": {c: [float(v) for v in frac[c]] for c in range(C)}, "mean_conf": {c: [float(v) for v in conf[c]] for c in range(C)}}


_VALUES = ("ece", "mce", "brier")
_SUMS = ("wsum", "wpos", "csum", "bnum")


def _calibration_metrics(outputs, targets, cal, bins, binning, n_boot, seed, groups, alpha, return_replicates, device=None, chunk=None,
                         host=False):
    """The body of calibration_metrics and of its numpy statement: the integer sums of the point sample and of every replicate through
    the replicate driver -- from cx_boot_calib on `device`, or, host=True, from calibration_sums_reference -- then the one forming of
    the floats."""
    if int(n_boot) != 0:
        _check_boot(n_boot, alpha)
    plan = calibration_plan(outputs, targets, groups, cal, bins, binning)
    U = plan["n_units"]
    if host:
        def sums(counts):
            return calibration_sums_reference(counts, plan)
    else:
        import torch

        from . import ops
        order = torch.from_numpy(plan["order"]).to(device)
        conf = torch.from_numpy(plan["conf"].view(np.int32)).to(device)

        def sums(counts):
            return (v.cpu().numpy() for v in ops.boot_calib(counts, order, conf, plan["offs"], plan["lens"], U, plan["bins"]))
    point, reps = _replicates(lambda counts: dict(zip(_SUMS, sums(counts))), U, n_boot, seed, device, chunk, host)
    point = [point[name][None] for name in _SUMS]                 # as one-row tables again
    values = _calibration_values(*point)
    if reps is None:
        out = {name: {"point": {c: float(v) for c, v in enumerate(values[name][0])}} for name in _VALUES}
    else:
        rep_values = _calibration_values(*(reps[name] for name in _SUMS))
        out = {name: _summarise_metric(values[name][0], rep_values[name], n_boot, seed, alpha, U, return_replicates) for name in _VALUES}
    out["reliability"] = _reliability(*point[:3], plan["bins"], plan["binning"])
    if return_replicates and reps is not None:
        out["replicate_weights"] = rep_values["weight"]             # W of every (replicate, class)
    return out


def calibration_metrics(outputs, targets, cal=None, bins=15, binning="width", n_boot=0, seed=0, groups=None, alpha=0.05, device="cuda",
                        chunk=None, return_replicates=False):
    """ECE, MCE and Brier score per class of the map `cal` (None: the raw sigmoid) with their percentile bootstrap intervals, on the
    GPU (cx_boot_counts + cx_boot_calib; no CPU fallback).  Returns {"ece": summary, "mce": summary, "brier": summary,
    "reliability": {bins, binning, weight, frac_pos, mean_conf per class and bin, of the point sample}}; a summary is what
    bootstrap_metrics returns per metric.  The point estimate runs through the same kernel with a row of ones; n_boot = 0 returns
    {"point": ...} summaries only.  The replicates use the count table, the chunking and the seeds of bootstrap_auc: for one
    (seed, unit) they are the resamples of the AUROC intervals.  With `cal` given every interval is CONDITIONAL on the fitted
    parameters: the fit is not redrawn per replicate, so the intervals leave the fit's own sampling error out.
    return_replicates: also "replicates" per summary and "replicate_weights", the kept weight W of every (replicate, class)."""
    return _calibration_metrics(outputs, targets, cal, bins, binning, n_boot, seed, groups, alpha, return_replicates, device=device, chunk=chunk)


def calibration_metrics_reference(outputs, targets, cal=None, bins=15, binning="width", n_boot=0, seed=0, groups=None, alpha=0.05,
                                  return_replicates=False):
    """The numpy statement of calibration_metrics (host; for the tests and as the timing yardstick)."""
    return _calibration_metrics(outputs, targets, cal, bins, binning, n_boot, seed, groups, alpha, return_replicates, host=True)


def load_calibration(path):
    """The fit stored in a calibration_<tag>.json (its "fit" entry) or a bare fit dict written with json."""
    import json
    with open(path) as f:
        d = json.load(f)
    d = d.get("fit", d)
    if not isinstance(d, dict) or "a" not in d or "b" not in d:
        raise ValueError("calibration: %s holds no fit (no 'a' / 'b')" % path)
    return d
