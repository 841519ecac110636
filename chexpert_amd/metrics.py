"""Evaluation metrics of the reference (`compute_metrics`, /root/reference/chexpert.py:130-146).

The reference calls sklearn `roc_curve` / `auc` / `precision_recall_curve` per class on raw logits.
Here the ROC / PR curves are built directly (descending score sweep with tie groups collapsed, as
sklearn's `_binary_clf_curve` does) and the AUROC is the trapezoid area.  That part is host-side numpy: it runs once per
evaluation on (N, 5) arrays.

The interval estimates below it run on the GPU: percentile bootstrap intervals of the AUROC (bootstrap.hip, cx_boot_auc) and of
the average precision and fixed operating points (cx_boot_sweep), both over the count tables of resample.py's replicate driver, and
the analytic DeLong / Obuchowski intervals and paired test (delong.hip).  Every GPU function has a `*_reference` twin, the numpy
statement the kernels are held to bit for bit; a pair shares one private body that differs only in where the integers come from.
"""
import math
import re
from fractions import Fraction
from statistics import NormalDist

import numpy as np

from ._lib import BOOT_MAX_POINTS, BOOT_SENS, BOOT_SPEC, DELONG_MAX_ROWS
from .resample import (BOOT_MAX_UNITS, _as_scores, _check_boot, _check_inputs, _pack_lists, _replicates, _summarise_diff,  # noqa: F401
                       _summarise_metric, _units_of, bootstrap_counts_reference, bootstrap_draws, splitmix64)  # (the draws stay in reach here)


def _binary_curve(y_true, score):
    y_true = np.asarray(y_true, dtype=np.float64) > 0.5
    score = np.asarray(score, dtype=np.float64)
    order = np.argsort(-score, kind="mergesort")
    y, s = y_true[order], score[order]
    distinct = np.where(np.diff(s))[0]
    idx = np.r_[distinct, y.size - 1]                 # last index of every tie group
    tps = np.cumsum(y)[idx].astype(np.float64)
    fps = (1 + idx) - tps
    return fps, tps, s[idx]


def roc_curve(y_true, score):
    fps, tps, thr = _binary_curve(y_true, score)
    fps, tps = np.r_[0.0, fps], np.r_[0.0, tps]
    if fps[-1] <= 0 or tps[-1] <= 0:
        nan = np.full(fps.shape, np.nan)
        return (nan if fps[-1] <= 0 else fps / fps[-1]), (nan if tps[-1] <= 0 else tps / tps[-1]), thr
    return fps / fps[-1], tps / tps[-1], thr


_trapz = getattr(np, "trapezoid", None) or np.trapz      # NumPy >= 2.0 / 1.x


def auc(x, y):
    return float(_trapz(y, x)) if not (np.any(np.isnan(x)) or np.any(np.isnan(y))) else float("nan")


def precision_recall_curve(y_true, score):
    fps, tps, thr = _binary_curve(y_true, score)
    precision = tps / np.maximum(tps + fps, 1e-300)
    recall = tps / tps[-1] if tps[-1] > 0 else np.ones_like(tps)
    sl = slice(None, None, -1)
    return np.r_[precision[sl], 1.0], np.r_[recall[sl], 0.0], thr[sl]


def compute_metrics(outputs, targets, losses):
    """Same dictionary layout as chexpert.py:130-146 (lists per class, json-serialisable).  A row whose target is negative (an
    uncertain label kept as -1) is left out of that class's curves and of that class's mean loss."""
    outputs, targets, losses = (np.asarray(t, dtype=np.float64) for t in (outputs, targets, losses))
    if not (targets < 0).any():
        mean_loss = losses.mean(0).tolist()
    else:
        mean_loss = [float(losses[targets[:, i] >= 0, i].mean()) if (targets[:, i] >= 0).any() else float("nan")
                     for i in range(outputs.shape[1])]
    fpr, tpr, aucs, precision, recall = {}, {}, {}, {}, {}
    for i in range(outputs.shape[1]):
        keep = targets[:, i] >= 0
        if len(keep) and not keep.any():                  # a class with every label ignored has no curve
            aucs[i], fpr[i], tpr[i], precision[i], recall[i] = float("nan"), [], [], [], []
            continue
        f, t, _ = roc_curve(targets[keep, i], outputs[keep, i])
        aucs[i] = auc(f, t)
        p, r, _ = precision_recall_curve(targets[keep, i], outputs[keep, i])
        fpr[i], tpr[i], precision[i], recall[i] = f.tolist(), t.tolist(), p.tolist(), r.tolist()
    return {"fpr": fpr, "tpr": tpr, "aucs": aucs, "precision": precision, "recall": recall, "loss": dict(enumerate(mean_loss))}


def mean_auc(metrics):
    v = np.array(list(metrics["aucs"].values()), dtype=np.float64)
    return float(np.nanmean(v)) if np.any(~np.isnan(v)) else float("nan")


# ---- bootstrap confidence intervals of the AUROC (chexpert_amd/csrc/bootstrap.hip) ------------------------------------------------
# Rows are grouped into U resampling units (an image by default, or a study / a patient); replicate b draws U units with replacement
# and weighs every row by the number of times its unit was drawn.  The weighted AUROC is exact in integers:
#   num2 = sum over positives i of w_i * (LT_i + LE_i),  LT_i / LE_i = the negative weight with a score < / <= that of i
#   AUROC = num2 / (2 W+ W-): the trapezoid area of the materialised resample, ties counted half; W+ = 0 or W- = 0: NaN (degenerate)
# The `*_reference` functions are the numpy statement the kernels are held to bit for bit; `bootstrap_auc` itself runs on the GPU only.
# The draws, the count table, the input checks and the replicate loop are resample.py's.
def bootstrap_plan(outputs, targets, groups=None):
    """What cx_boot_auc reads, built once per call on the host (N log N): for every class the kept rows (target >= 0) in two orders,
    both ascending in score (compared in the dtype given): `hi` with the negatives of a tie group before its positives, `lo` with the
    positives first.  An entry is the row's unit index with the label (target > 0.5) in bit 31.
    groups: one hashable id per row (data.extract_patient_ids output works); the units are the distinct ids.  None: every row its own.
    Returns {"order": int32 (for class c: hi then lo, lens[c] entries each, from offs[c]), "offs": int64 (C), "lens": int32 (C),
    "units": int64 (N) unit index of every row, "n_units": U}."""
    s, t, units, U = _check_inputs(outputs, targets, groups, "bootstrap")
    parts = []
    for c in range(s.shape[1]):
        keep = np.nonzero(t[:, c] >= 0)[0]
        pos = t[keep, c] > 0.5
        rank = np.unique(s[keep, c], return_inverse=True)[1].reshape(-1)
        entry = (units[keep] | (pos.astype(np.int64) << 31)).astype(np.uint32).view(np.int32)
        parts.append((entry[np.lexsort((pos, rank))], entry[np.lexsort((~pos, rank))]))
    order, offs, lens = _pack_lists(parts)
    return {"order": order, "offs": offs, "lens": lens, "units": units, "n_units": U}


def bootstrap_scan_reference(counts, order, offs, lens, n_units):
    """Statement of cx_boot_auc in uint64 numpy: (num2, wpos, wneg), each (n_rep, C) uint64, num2 = S(hi) + S(lo) with
    S(order) = sum_t p_t * (sum_{t' < t} q_t'), p / q the count of the entry's unit at a positive / negative entry; unit indices are
    clamped to n_units - 1 as the kernel clamps them."""
    counts = np.asarray(counts).astype(np.uint64)
    order = np.asarray(order, dtype=np.int32)
    R, C = counts.shape[0], len(lens)
    num2, wpos, wneg = (np.zeros((R, C), dtype=np.uint64) for _ in range(3))
    for c in range(C):
        n, o = int(lens[c]), int(offs[c])
        for k in range(2):
            e = order[o + k * n:o + (k + 1) * n]
            w = counts[:, np.minimum(e & 0x7fffffff, n_units - 1)]
            p, q = np.where(e < 0, w, np.uint64(0)), np.where(e < 0, np.uint64(0), w)
            excl = np.cumsum(q, axis=1, dtype=np.uint64) - q
            num2[:, c] += (p * excl).sum(1, dtype=np.uint64)
            if k == 0:
                wpos[:, c], wneg[:, c] = p.sum(1, dtype=np.uint64), q.sum(1, dtype=np.uint64)
    return num2, wpos, wneg


def _definition_parts(s, t, units, counts):
    """(num2, wpos, wneg), each (R, C) int64, straight from the definition (no `hi` / `lo` orders): the rows of a class sorted by score,
    the negative weight accumulated along them, LE_i read at the end and LT_i before the start of row i's tie group."""
    counts = np.asarray(counts).astype(np.int64)
    R, C = counts.shape[0], s.shape[1]
    num2, wpos, wneg = (np.zeros((R, C), dtype=np.int64) for _ in range(3))
    for c in range(C):
        keep = np.nonzero(t[:, c] >= 0)[0]
        if not len(keep):
            continue
        vals, rank = np.unique(s[keep, c], return_inverse=True)
        rank = rank.reshape(-1)
        by = np.argsort(rank, kind="mergesort")
        pos, r = (t[keep, c] > 0.5)[by], rank[by]
        w = counts[:, units[keep][by]]
        cneg = np.concatenate([np.zeros((R, 1), dtype=np.int64), np.cumsum(np.where(pos, 0, w), axis=1)], axis=1)
        start = np.searchsorted(r, np.arange(len(vals)), side="left")      # first sorted row of every tie group
        end = np.searchsorted(r, np.arange(len(vals)), side="right")
        num2[:, c] = (np.where(pos, w, 0) * (cneg[:, start[r]] + cneg[:, end[r]])).sum(1)
        wpos[:, c], wneg[:, c] = np.where(pos, w, 0).sum(1), cneg[:, -1]
    return num2, wpos, wneg


def _auc_of(num2, wpos, wneg):
    """float64 num2 / (2 W+ W-): both operands are exact (below 2^53 for U <= 2^24), so this is the correctly rounded quotient."""
    num2, den = np.asarray(num2).astype(np.float64), 2.0 * np.asarray(wpos).astype(np.float64) * np.asarray(wneg).astype(np.float64)
    with np.errstate(divide="ignore", invalid="ignore"):
        return np.where(den > 0, num2 / np.where(den > 0, den, 1.0), np.nan)


def _aucs(summaries):
    """bootstrap_auc's result from bootstrap_metrics' for ("auroc",): the same numbers with "aucs" in place of "point"."""
    s = summaries["auroc"]
    return {"aucs": s.pop("point"), **s}


def bootstrap_auc(outputs, targets, n_boot=1000, seed=0, groups=None, alpha=0.05, device="cuda", chunk=None, return_replicates=False):
    """AUROC per class with its (1 - alpha) non-parametric percentile bootstrap interval, on the GPU (cx_boot_counts + cx_boot_auc; no
    CPU fallback).  outputs / targets: (N, C) scores and labels as compute_metrics takes them (target < 0: the row is left out of that
    class); groups: one id per row to resample by study or patient instead of by image.  Replicates run in chunks whose count table
    stays under 256 MB (`chunk`: replicates per chunk); the result does not depend on the chunking.  The point estimate goes through
    the same kernel with a row of ones as counts.  Returns a json-serialisable dict, int class keys as in compute_metrics:
      aucs; lo, hi: np.percentile at 100 alpha/2 and 100 (1 - alpha/2) over the non-degenerate replicates; se: their std (ddof 1);
      n_degenerate: replicates without a positive or without a negative; mean_auc: {point, lo, hi, se} of the per-replicate mean over
      the classes (NaN where any class is degenerate); n_boot, seed, alpha, n_units.
    return_replicates: also "replicates", the (n_boot, C) float64 array (not json-serialisable)."""
    return _aucs(_bootstrap_metrics(outputs, targets, ("auroc",), n_boot, seed, groups, alpha, return_replicates, device=device, chunk=chunk))


def bootstrap_auc_reference(outputs, targets, n_boot=1000, seed=0, groups=None, alpha=0.05, return_replicates=False):
    """The numpy statement of bootstrap_auc (host, integers from the definition; for the tests and as the timing yardstick)."""
    return _aucs(_bootstrap_metrics(outputs, targets, ("auroc",), n_boot, seed, groups, alpha, return_replicates, host=True))


def bootstrap_auc_diff(outputs_a, outputs_b, targets, n_boot=1000, seed=0, groups=None, alpha=0.05, device="cuda", chunk=None,
                       return_replicates=False):
    """Paired bootstrap of the AUROC difference of two models on the same rows (one count table, two plans).  Per class and under
    "mean_auc" for the mean over the classes: delta (a - b), lo, hi (percentiles of the replicate differences) and p, two-sided:
    2 min((#{d* <= 0} + 1) / (B' + 1), (#{d* >= 0} + 1) / (B' + 1)) capped at 1, B' = the replicates degenerate in neither model."""
    return _bootstrap_metrics_diff(outputs_a, outputs_b, targets, ("auroc",), n_boot, seed, groups, alpha, return_replicates, device=device,
                                   chunk=chunk)["auroc"]


def bootstrap_auc_diff_reference(outputs_a, outputs_b, targets, n_boot=1000, seed=0, groups=None, alpha=0.05, return_replicates=False):
    """The numpy statement of bootstrap_auc_diff."""
    return _bootstrap_metrics_diff(outputs_a, outputs_b, targets, ("auroc",), n_boot, seed, groups, alpha, return_replicates, host=True)["auroc"]


# ---- bootstrap of the metrics that need the whole threshold sweep (chexpert_amd/csrc/bootstrap.hip, cx_boot_sweep) ----------------
# For one replicate and one class: the kept rows (target >= 0) weigh w = counts[unit(row)], a row is positive iff target > 0.5.  The
# distinct scores are swept from high to low; after tie group g, tp_g / fp_g = the positive / negative weight with a score >= the
# group's, W+ / W- the totals.  The operating points of the resample are (tp_g, fp_g) at the group ends, plus (0, 0); nothing is
# interpolated:
#   AP      = apnum / (W+ 2^32),  apnum = sum_g (tp_g - tp_{g-1}) * floor((tp_g << 32) / (tp_g + fp_g))  (uint64; a term with
#             tp_g = tp_{g-1} is 0 and does not divide): the step sum of sklearn's average_precision_score, below the exact value by
#             less than 2^-32.  NaN iff W+ = 0
#   sens@S  = max{tp_g : fp_g 10^6 <= (10^6 - s) W-} / W+,  s = round(S 10^6): the sensitivity at specificity >= S
#   spec@S  = 1 - min{fp_g : tp_g 10^6 >= s W+} / W-: the specificity at sensitivity >= S.  Both NaN iff W+ = 0 or W- = 0
# A tie group without weight in a replicate repeats the previous (tp, fp), so the group ends are a property of the scores alone.
BOOT_PPM = 10 ** 6
_METRIC_POINT = re.compile(r"(sens|spec)@(\d*\.\d+|\d+)\Z")


def parse_boot_metrics(names):
    """Strict parse of metric names: "auroc", "ap", "sens@S", "spec@S" with S a plain decimal inside (0, 1) of at most 6 decimals.
    Returns (names as a tuple, points): points lists (BOOT_SENS | BOOT_SPEC, s = S in millionths) of the operating points in the order
    named.  ValueError: an unknown or repeated name, an S outside (0, 1) or finer than 10^-6, more than BOOT_MAX_POINTS points, none."""
    if isinstance(names, str):
        names = (names,)
    names, points = tuple(names), []
    if not names:
        raise ValueError("bootstrap: no metric named")
    for name in names:
        if not isinstance(name, str):
            raise ValueError("bootstrap: a metric name is a string (got %r)" % (name,))
        if names.count(name) > 1:
            raise ValueError("bootstrap: metric %r is named twice" % name)
        if name in ("auroc", "ap"):
            continue
        m = _METRIC_POINT.match(name)
        if not m:
            raise ValueError("bootstrap: unknown metric %r (auroc, ap, sens@S, spec@S with S a decimal inside (0, 1))" % name)
        frac = m.group(2).partition(".")[2]
        if len(frac) > 6:
            raise ValueError("bootstrap: %r has more than 6 decimals" % name)
        ppm = int(m.group(2).partition(".")[0] or "0") * BOOT_PPM + int((frac + "000000")[:6])
        if not 1 <= ppm <= BOOT_PPM - 1:
            raise ValueError("bootstrap: %r asks for a value outside (0, 1)" % name)
        points.append((BOOT_SENS if m.group(1) == "sens" else BOOT_SPEC, ppm))
    if len(points) > BOOT_MAX_POINTS:
        raise ValueError("bootstrap: %d operating points (at most %d in one call)" % (len(points), BOOT_MAX_POINTS))
    return names, points


def bootstrap_sweep_plan(outputs, targets, groups=None):
    """What cx_boot_sweep reads, built once per call on the host: for every class the kept rows (target >= 0) ONCE, descending in score
    (compared in the dtype given).  An entry is the row's unit index with the label (target > 0.5) in bit 31 and bit 30 set on the last
    entry of its tie group (free: U <= 2^24).  Inside a tie group the positives come first, then the row index ascends: the order there
    is immaterial, this one makes the plan deterministic.  Returns {"order": int32, "offs": int64 (C), "lens": int32 (C), "units",
    "n_units"} as bootstrap_plan does, with lens[c] entries for class c from offs[c]."""
    s, t, units, U = _check_inputs(outputs, targets, groups, "bootstrap")
    parts = []
    for c in range(s.shape[1]):
        keep = np.nonzero(t[:, c] >= 0)[0]
        pos = t[keep, c] > 0.5
        rank = np.unique(s[keep, c], return_inverse=True)[1].reshape(-1)
        by = np.lexsort((keep, ~pos, -rank))                     # descending score; positives first; ascending row
        entry = units[keep][by] | (pos[by].astype(np.int64) << 31)
        if len(by):
            r = rank[by]
            entry |= np.r_[r[1:] != r[:-1], True].astype(np.int64) << 30
        parts.append(entry.astype(np.uint32).view(np.int32))
    order, offs, lens = _pack_lists(parts)
    return {"order": order, "offs": offs, "lens": lens, "units": units, "n_units": U}


def _check_points(points):
    points = [(int(k), int(v)) for k, v in points]
    if len(points) > BOOT_MAX_POINTS or any(k not in (BOOT_SENS, BOOT_SPEC) or not 1 <= v <= BOOT_PPM - 1 for k, v in points):
        raise ValueError("bootstrap: at most %d operating points (BOOT_SENS | BOOT_SPEC, 1 .. 999999 millionths), got %s"
                         % (BOOT_MAX_POINTS, points))
    return points


def bootstrap_sweep_reference(counts, order, offs, lens, n_units, points=()):
    """Statement of cx_boot_sweep in uint64 numpy, vectorised over the replicates: (apnum, wpos, wneg, pts), (n_rep, C) and
    (n_rep, C, P) uint64.  Unit indices are clamped to n_units - 1 as the kernel clamps them; every comparison is in uint64."""
    counts = np.asarray(counts).astype(np.uint64)
    order = np.asarray(order, dtype=np.int32)
    points = _check_points(points)
    R, C, u64 = counts.shape[0], len(lens), np.uint64
    apnum, wpos, wneg = (np.zeros((R, C), dtype=u64) for _ in range(3))
    pts = np.zeros((R, C, len(points)), dtype=u64)
    for c in range(C):
        e = order[int(offs[c]):int(offs[c]) + int(lens[c])]
        w = counts[:, np.minimum(e & 0x3fffffff, n_units - 1)]
        tp = np.cumsum(np.where(e < 0, w, u64(0)), axis=1, dtype=u64)
        fp = np.cumsum(np.where(e < 0, u64(0), w), axis=1, dtype=u64)
        if len(e):
            wpos[:, c], wneg[:, c] = tp[:, -1], fp[:, -1]
        ends = np.nonzero(e & 0x40000000)[0]
        tp, fp = tp[:, ends], fp[:, ends]                        # the operating points of the resample (without (0, 0))
        step = tp - np.concatenate([np.zeros((R, 1), dtype=u64), tp[:, :-1]], axis=1)
        live = (step > 0) & (tp + fp > 0)
        quot = (tp << u64(32)) // np.where(live, tp + fp, u64(1))
        apnum[:, c] = np.where(live, step * quot, u64(0)).sum(1, dtype=u64)
        for k, (kind, ppm) in enumerate(points):
            if kind == BOOT_SENS:
                ok = fp * u64(BOOT_PPM) <= u64(BOOT_PPM - ppm) * wneg[:, c:c + 1]
                pts[:, c, k] = np.where(ok, tp, u64(0)).max(axis=1, initial=u64(0))               # (0, 0) always qualifies
            else:
                ok = tp * u64(BOOT_PPM) >= u64(ppm) * wpos[:, c:c + 1]
                least = np.where(ok, fp, u64(0xffffffff)).min(axis=1, initial=u64(0xffffffff))
                pts[:, c, k] = np.where(wpos[:, c] == 0, u64(0), least)                           # (0, 0) qualifies iff W+ = 0
    return apnum, wpos, wneg, pts


def _sweep_definition_parts(s, t, units, counts, points=()):
    """(apnum, wpos, wneg, pts) straight from the definition, in Python integers (object arrays): no prepared order, no running sums, no
    group-end marks.  For every distinct score v of a class, tp / fp are the weights of the kept positives / negatives scoring >= v;
    the thresholds whose group has no weight in a replicate are dropped before anything else is formed."""
    counts = np.asarray(counts).astype(np.int64)
    points = _check_points(points)
    R, C = counts.shape[0], s.shape[1]
    apnum, wpos, wneg = (np.zeros((R, C), dtype=object) for _ in range(3))
    pts = np.zeros((R, C, len(points)), dtype=object)
    for c in range(C):
        keep = np.nonzero(t[:, c] >= 0)[0]
        sc, pos = s[keep, c], t[keep, c] > 0.5
        vals = np.unique(sc)[::-1]
        at_least = (sc[None, :] >= vals[:, None]).astype(np.int64)               # (thresholds, rows)
        in_group = (sc[None, :] == vals[:, None]).astype(np.int64)
        for r in range(R):
            w = counts[r, units[keep]]
            tps, fps = at_least @ np.where(pos, w, 0), at_least @ np.where(pos, 0, w)
            present = (in_group @ w) > 0
            curve = [(0, 0)] + [(int(a), int(b)) for a, b in zip(tps[present], fps[present])]
            Wp, Wn = int(np.where(pos, w, 0).sum()), int(np.where(pos, 0, w).sum())
            wpos[r, c], wneg[r, c] = Wp, Wn
            apnum[r, c] = sum((a - a0) * ((a << 32) // (a + b)) for (a0, _), (a, b) in zip(curve[:-1], curve[1:]) if a != a0)
            for k, (kind, ppm) in enumerate(points):
                if kind == BOOT_SENS:
                    pts[r, c, k] = max(a for a, b in curve if b * BOOT_PPM <= (BOOT_PPM - ppm) * Wn)
                else:
                    pts[r, c, k] = min(b for a, b in curve if a * BOOT_PPM >= ppm * Wp)
    return apnum, wpos, wneg, pts


def _sweep_values(names, points, apnum, wpos, wneg, pts):
    """{name: (n_rep, C) float64} of the sweep's metrics from its integers.  float64(apnum) rounds once (apnum may need 64 bits), W+ 2^32
    is exact and the quotient rounds once; the operating points are quotients of exact operands, 1 - x rounds once more."""
    ap = np.asarray(apnum).astype(np.uint64).astype(np.float64)
    p, q = np.asarray(wpos).astype(np.float64), np.asarray(wneg).astype(np.float64)
    both = (p > 0) & (q > 0)
    out, k = {}, 0
    with np.errstate(divide="ignore", invalid="ignore"):
        for name in names:
            if name == "ap":
                out[name] = np.where(p > 0, ap / (np.where(p > 0, p, 1.0) * 2.0 ** 32), np.nan)
            elif name != "auroc":
                v = np.asarray(pts)[:, :, k].astype(np.float64)
                out[name] = np.where(both, v / np.where(both, p, 1.0) if points[k][0] == BOOT_SENS else 1.0 - v / np.where(both, q, 1.0), np.nan)
                k += 1
    return out


def _evaluator(outputs, targets, groups, names, points, device=None, host=False):
    """(evaluate, U) of one model: evaluate(counts) -> {name: (R, C) float64} of the named metrics over a count table.  On the GPU the
    integers come from cx_boot_auc and cx_boot_sweep over the prepared plans; host=True: the AUROC's from the definition
    (`_definition_parts`, no plan) and the sweep's from the numpy statement of the kernel over the plan."""
    auroc = sweep = None                                         # counts -> the integer parts, where the names ask for them
    if "auroc" in names:
        if host:
            s, t = _as_scores(outputs), np.asarray(_as_scores(targets), dtype=np.float64)
            units, U = _units_of(s.shape[0], groups)

            def auroc(counts):
                return _definition_parts(s, t, units, counts)
        else:
            plan = bootstrap_plan(outputs, targets, groups)
            auroc, U = _gpu_parts("boot_auc", plan, device), plan["n_units"]
    if len(names) > ("auroc" in names):
        plan = bootstrap_sweep_plan(outputs, targets, groups)
        U = plan["n_units"]
        if host:
            def sweep(counts):
                return bootstrap_sweep_reference(counts, plan["order"], plan["offs"], plan["lens"], U, points)
        else:
            sweep = _gpu_parts("boot_sweep", plan, device, points)

    def evaluate(counts):
        out = {} if auroc is None else {"auroc": _auc_of(*auroc(counts))}
        if sweep is not None:
            out.update(_sweep_values(names, points, *sweep(counts)))       # (apnum is read as the kernel's uint64 there)
        return out
    return evaluate, U


def _gpu_parts(op, plan, device, *args):
    """counts -> the integer parts that ops.<op> returns for the plan, as numpy arrays; the order array goes to the device once."""
    import torch

    from . import ops
    order = torch.from_numpy(plan["order"]).to(device)
    return lambda counts: (v.cpu().numpy() for v in getattr(ops, op)(counts, order, plan["offs"], plan["lens"], plan["n_units"], *args))


def _bootstrap(models, targets, metrics, n_boot, seed, groups, alpha, device=None, chunk=None, host=False):
    """(names, point, reps, U) of the named metrics of every model over ONE count table per chunk of replicates (the paired
    comparison): point[k, name] (C) and reps[k, name] (n_boot, C) of model k."""
    _check_boot(n_boot, alpha)
    names, points = parse_boot_metrics(metrics)
    evaluators, units = zip(*(_evaluator(o, targets, groups, names, points, device, host) for o in models))
    point, reps = _replicates(lambda counts: {(k, name): v for k, evaluate in enumerate(evaluators) for name, v in evaluate(counts).items()},
                              units[0], n_boot, seed, device, chunk, host)
    return names, point, reps, units[0]


def _bootstrap_metrics(outputs, targets, metrics, n_boot, seed, groups, alpha, return_replicates, **backend):
    names, point, reps, U = _bootstrap([outputs], targets, metrics, n_boot, seed, groups, alpha, **backend)
    return {name: _summarise_metric(point[0, name], reps[0, name], n_boot, seed, alpha, U, return_replicates) for name in names}


def _bootstrap_metrics_diff(outputs_a, outputs_b, targets, metrics, n_boot, seed, groups, alpha, return_replicates, **backend):
    names, point, reps, U = _bootstrap([outputs_a, outputs_b], targets, metrics, n_boot, seed, groups, alpha, **backend)
    return {name: _summarise_diff(point[0, name], point[1, name], reps[0, name], reps[1, name], n_boot, seed, alpha, U, return_replicates)
            for name in names}


def bootstrap_metrics(outputs, targets, metrics=("auroc", "ap"), n_boot=1000, seed=0, groups=None, alpha=0.05, device="cuda", chunk=None,
                      return_replicates=False):
    """Percentile bootstrap intervals of several evaluation metrics over the SAME resamples, on the GPU (cx_boot_counts, cx_boot_auc,
    cx_boot_sweep; no CPU fallback).  metrics: "auroc", "ap" (average precision, the step sum), "sens@S" (sensitivity at specificity
    >= S) and "spec@S" (specificity at sensitivity >= S), S a decimal inside (0, 1) with at most 6 decimals, at most 8 operating
    points in one call.  The other arguments are those of bootstrap_auc.  Returns {name: summary}; a summary has the keys of
    bootstrap_auc's result with "point" in place of "aucs" ("mean_auc" is the metric's mean over the classes), and the "auroc"
    summary carries the numbers of bootstrap_auc with the same arguments, bit for bit."""
    return _bootstrap_metrics(outputs, targets, metrics, n_boot, seed, groups, alpha, return_replicates, device=device, chunk=chunk)


def bootstrap_metrics_reference(outputs, targets, metrics=("auroc", "ap"), n_boot=1000, seed=0, groups=None, alpha=0.05,
                                return_replicates=False):
    """The numpy statement of bootstrap_metrics (host; for the tests and as the timing yardstick)."""
    return _bootstrap_metrics(outputs, targets, metrics, n_boot, seed, groups, alpha, return_replicates, host=True)


def bootstrap_metrics_diff(outputs_a, outputs_b, targets, metrics=("auroc", "ap"), n_boot=1000, seed=0, groups=None, alpha=0.05,
                           device="cuda", chunk=None, return_replicates=False):
    """Paired bootstrap of the difference a - b of every named metric between two models on the same rows (one count table, two plans
    per kernel).  Returns {name: what bootstrap_auc_diff returns for the AUROC}."""
    return _bootstrap_metrics_diff(outputs_a, outputs_b, targets, metrics, n_boot, seed, groups, alpha, return_replicates, device=device,
                                   chunk=chunk)


def bootstrap_metrics_diff_reference(outputs_a, outputs_b, targets, metrics=("auroc", "ap"), n_boot=1000, seed=0, groups=None, alpha=0.05,
                                     return_replicates=False):
    """The numpy statement of bootstrap_metrics_diff."""
    return _bootstrap_metrics_diff(outputs_a, outputs_b, targets, metrics, n_boot, seed, groups, alpha, return_replicates, host=True)


# ---- DeLong / Obuchowski variance of the AUROC and the paired test (chexpert_amd/csrc/delong.hip) ----------------------------------
# One model, one class: the kept rows (target >= 0), M positives (target > 0.5), N negatives, scores compared in the dtype given.
# Doubled placements, ties counted half (integers):
#   a positive i: X2_i = 2 #{neg j : s_j < s_i} + #{neg j : s_j = s_i};  a negative j: Y2_j = 2 #{pos i : s_i > s_j} + #{pos i : s_i = s_j}
#   num2 = sum X2 = sum Y2 (what cx_boot_auc returns for a count row of ones),  theta = num2 / (2 M N)
# Rows are grouped into U units (one row each, or the distinct ids of `groups`).  Per class and unit u four integers -- the table of
# cx_delong_place: X_u (sum of X2 over the unit's positives), m_u (their number), Y_u (sum of Y2 over its negatives), n_u.  With
#   a_u = X_u / (2 N) - m_u theta,  b_u = Y_u / (2 M) - n_u theta,  I10 / I01 / I = the units with m_u > 0 / n_u > 0 / a kept row:
#   S10 = I10 / ((I10 - 1) M) sum a_u^2,  S01 = I01 / ((I01 - 1) N) sum b_u^2,  S11 = I / (I - 1) sum a_u b_u
#   Var(theta) = S10 / M + S01 / N + 2 S11 / (M N)                 (Obuchowski 1997; single-row units: DeLong 1988 exactly)
#   Cov(theta_A, theta_B): the same with the cross products sum aA aB, sum bA bB and sum (aA bB + aB bA) (no factor 2 on the last)
#   Var(delta) = Var_A + Var_B - 2 Cov,  z = delta / sqrt(Var(delta)),  p = erfc(|z| / sqrt 2)
# The mean over the classes (different kept rows per class: DeLong's matrix does not apply) takes the cluster-robust influence form:
#   psi_u^c = a_u^c / M^c + b_u^c / N^c,  psibar_u = mean_c psi_u^c,  Var(mean theta) = U / (U - 1) sum_u psibar_u^2
# which for one class differs from the per-class form only in the finite-sample factors (U / (U - 1) for all three terms instead of
# I10 / (I10 - 1), I01 / (I01 - 1), I / (I - 1)); the paired mean uses psibar_A - psibar_B.
# Where each part is computed: a_u = (M X_u - m_u num2) / (2 M N) and b_u = (N Y_u - n_u num2) / (2 M N) have integer numerators, so every
# sum above is a combination of the raw moment sums G[p][q] = sum_u z[p][u] z[q][u] of the table's rows (cx_delong_gram) with integer
# coefficients.  The host forms these combinations in Python integers, the quotients as exact fractions, and rounds ONCE to float64:
# no float sum is ever formed, so the GPU path and the numpy statement return equal floats whenever their integers agree, and identical
# models give Var(delta) = 0 exactly.
def delong_place_reference(order, offs, lens, n_units):
    """Statement of cx_delong_place in int64 numpy: the (4 C, n_units) table, rows 4c .. 4c+3 = X, m, Y, n of class c, from the `hi` /
    `lo` orders of bootstrap_plan.  In `hi` the negatives in front of a positive are its LE, in `lo` its LT (their sum is X2); for a
    negative Y2 = (M - positives in front in lo) + (M - positives in front in hi).  Unit indices are clamped to n_units - 1."""
    order = np.asarray(order, dtype=np.int32)
    U = int(n_units)
    z = np.zeros((4 * len(lens), U), dtype=np.int64)
    for c in range(len(lens)):
        n, o = int(lens[c]), int(offs[c])
        for k in range(2):
            e = order[o + k * n:o + (k + 1) * n]
            pos = e < 0
            u = np.minimum(e & 0x7fffffff, U - 1).astype(np.int64)
            before = np.cumsum(pos, dtype=np.int64) - pos                  # positives in front of every entry
            neg_before = np.arange(n, dtype=np.int64) - before
            np.add.at(z[4 * c], u[pos], neg_before[pos])
            np.add.at(z[4 * c + 2], u[~pos], int(pos.sum()) - before[~pos])
            if k == 0:
                np.add.at(z[4 * c + 1], u[pos], 1)
                np.add.at(z[4 * c + 3], u[~pos], 1)
    return z


def int_gram_reference(z, n_units=None):
    """Statement of cx_delong_gram: g[p][q] = sum_u z[p][u] z[q][u] mod 2^64 over the first n_units columns, as an int64 (Q, Q) array."""
    z = np.ascontiguousarray(np.asarray(z, dtype=np.int64)[:, :n_units]).view(np.uint64)
    with np.errstate(over="ignore"):
        return np.matmul(z, z.T).view(np.int64)


def _delong_check(alpha):
    if not 0.0 < alpha < 1.0:
        raise ValueError("delong: alpha must be inside (0, 1) (got %r)" % alpha)


def _delong_plans(models, targets, groups):
    """The plans of the models (bootstrap_plan's errors are the input errors) after the checks that come before any launch."""
    plans = [bootstrap_plan(o, targets, groups) for o in models]
    n_cls, U = len(plans[0]["lens"]), plans[0]["n_units"]
    if n_cls < 1:
        raise ValueError("delong: the outputs hold no class")
    if 4 * n_cls * len(plans) > DELONG_MAX_ROWS:
        raise ValueError("delong: %d classes of %d model(s) need %d table rows (at most %d are supported)"
                         % (n_cls, len(plans), 4 * n_cls * len(plans), DELONG_MAX_ROWS))
    # overflow guard: X_u <= 2 L g_u with L = the longest class list and g_u the rows of unit u, so every Gram entry is at most
    # 4 L^2 sum g_u^2; below 2^63 the int64 the kernel returns is the true integer
    g = np.bincount(plans[0]["units"], minlength=U).astype(np.int64)
    longest = int(max(int(v) for v in plans[0]["lens"]))
    if 4 * longest * longest * int(np.dot(g, g)) >= 1 << 63:
        raise ValueError("delong: 4 * %d^2 * sum of squared unit sizes (%d) reaches 2^63: the moment sums would overflow int64"
                         % (longest, int(np.dot(g, g))))
    return plans


def _delong_stats(table, n_models):
    """Per model and class (M, N, num2, I10, I01, I) as Python ints from the (4 C K, U) int64 table, a numpy array or a torch tensor
    on the GPU (only these reductions leave it)."""
    m, n = table[1::4], table[3::4]
    sums, m_on, n_on, any_on = (v.tolist() for v in (table.sum(1), (m > 0).sum(1), (n > 0).sum(1), ((m + n) > 0).sum(1)))
    n_cls = len(m_on) // n_models
    return [[(sums[4 * r + 1], sums[4 * r + 3], sums[4 * r], m_on[r], n_on[r], any_on[r]) for r in range(k * n_cls, (k + 1) * n_cls)]
            for k in range(n_models)]


class _DelongFinish:
    """The exact host finish: stats[k][c] = (M, N, num2, I10, I01, I), G = the (4 C K)^2 moment sums as nested lists of Python ints."""

    def __init__(self, stats, G, n_units):
        self.stats, self.G, self.U, self.C = stats, G, int(n_units), len(stats[0])

    def _q(self, k, c, v, l, d, w):
        """sum_u (v . rows of (k, c))_u (w . rows of (l, d))_u as an integer."""
        G, p0, q0 = self.G, 4 * (k * self.C + c), 4 * (l * self.C + d)
        return sum(v[i] * w[j] * G[p0 + i][q0 + j] for i in range(4) if v[i] for j in range(4) if w[j])

    def _coef(self, k, c):
        """Integer numerators of a_u, b_u (both over 2 M N) and psi_u (over 2 M^2 N^2) on the rows X, m, Y, n."""
        M, N, S = self.stats[k][c][:3]
        return (M, -S, 0, 0), (0, 0, N, -S), (M * N, -N * S, M * N, -M * S)

    def theta(self, k, c):
        M, N, S = self.stats[k][c][:3]
        return Fraction(S, 2 * M * N) if M and N else None

    def cov(self, k, l, c):
        """Cov(theta_k, theta_l) of class c as a Fraction (k == l: the variance); None where it is not defined."""
        M, N, _, I10, I01, I = self.stats[k][c]
        if not (M and N) or I10 < 2 or I01 < 2:
            return None
        (ak, bk, _), (al, bl, _) = self._coef(k, c), self._coef(l, c)
        D = (2 * M * N) ** 2
        s10 = Fraction(I10 * self._q(k, c, ak, l, c, al), (I10 - 1) * M * D)
        s01 = Fraction(I01 * self._q(k, c, bk, l, c, bl), (I01 - 1) * N * D)
        s11 = Fraction(I * (self._q(k, c, ak, l, c, bl) + self._q(l, c, al, k, c, bk)), (I - 1) * D)
        return s10 / M + s01 / N + s11 / (M * N)

    def mean_cov(self, k, l):
        """U / (U - 1) sum_u psibar_k psibar_l as a Fraction; None where a class has no positive or no negative, or U = 1."""
        if self.U < 2 or any(not (st[0] and st[1]) for st in self.stats[k]):
            return None
        tot = Fraction(0)
        for c in range(self.C):
            Mc, Nc = self.stats[k][c][:2]
            wc = self._coef(k, c)[2]
            for d in range(self.C):
                Md, Nd = self.stats[l][d][:2]
                tot += Fraction(self._q(k, c, wc, l, d, self._coef(l, d)[2]), 4 * (Mc * Nc * Md * Nd) ** 2)
        return tot * Fraction(self.U, (self.U - 1) * self.C * self.C)


def _delong_se(var):
    return math.sqrt(float(var)) if var is not None and var >= 0 else float("nan")


def _delong_band(point, se, zq, lo, hi):
    if math.isnan(point) or math.isnan(se):
        return float("nan"), float("nan")
    return min(max(point - zq * se, lo), hi), min(max(point + zq * se, lo), hi)


def _delong_summary(fin, alpha, grouped):
    C, zq = fin.C, NormalDist().inv_cdf(1.0 - alpha / 2.0)
    th = [fin.theta(0, c) for c in range(C)]
    aucs = {c: float(th[c]) if th[c] is not None else float("nan") for c in range(C)}
    se = {c: _delong_se(fin.cov(0, 0, c)) for c in range(C)}
    band = {c: _delong_band(aucs[c], se[c], zq, 0.0, 1.0) for c in range(C)}
    point = float(sum(th) / C) if all(t is not None for t in th) else float("nan")
    mse = _delong_se(fin.mean_cov(0, 0))
    mband = _delong_band(point, mse, zq, 0.0, 1.0)
    st = fin.stats[0]
    return {"aucs": aucs, "se": se, "lo": {c: band[c][0] for c in range(C)}, "hi": {c: band[c][1] for c in range(C)},
            "n_pos": {c: st[c][0] for c in range(C)}, "n_neg": {c: st[c][1] for c in range(C)},
            "n_units_pos": {c: st[c][3] for c in range(C)}, "n_units_neg": {c: st[c][4] for c in range(C)},
            "mean_auc": {"point": point, "se": mse, "lo": mband[0], "hi": mband[1]},
            "alpha": float(alpha), "n_units": fin.U, "method": "obuchowski" if grouped else "delong"}


def _delong_test(delta, var, zq):
    """(delta, se, lo, hi, z, p, degenerate) of one difference: delta a Fraction or None, var its variance as a Fraction or None."""
    nan = float("nan")
    if delta is None:
        return nan, nan, nan, nan, nan, nan, False
    d = float(delta)
    if var is None:
        return d, nan, nan, nan, nan, nan, False
    se = _delong_se(var)
    lo, hi = _delong_band(d, se, zq, -1.0, 1.0)
    if var <= 0:
        return d, se, lo, hi, nan, nan, True
    z = d / se
    return d, se, lo, hi, z, math.erfc(abs(z) / math.sqrt(2.0)), False


def _delong_diff_summary(fin, alpha, grouped):
    C, zq = fin.C, NormalDist().inv_cdf(1.0 - alpha / 2.0)
    rows = []
    for c in range(C):
        ta, tb = fin.theta(0, c), fin.theta(1, c)
        va, vb, cab = fin.cov(0, 0, c), fin.cov(1, 1, c), fin.cov(0, 1, c)
        rows.append(_delong_test(None if ta is None else ta - tb, None if va is None else va + vb - 2 * cab, zq))
    th = [(fin.theta(0, c), fin.theta(1, c)) for c in range(C)]
    ok = all(a is not None for a, _ in th)
    maa, mbb, mab = fin.mean_cov(0, 0), fin.mean_cov(1, 1), fin.mean_cov(0, 1)
    m = _delong_test(sum(a - b for a, b in th) / C if ok else None, None if maa is None else maa + mbb - 2 * mab, zq)
    keys = ("delta", "se", "lo", "hi", "z", "p", "degenerate")
    out = {name: {c: rows[c][i] for c in range(C)} for i, name in enumerate(keys)}
    out["mean_auc"] = dict(zip(keys[:6], m[:6]))
    out.update({"alpha": float(alpha), "n_units": fin.U, "method": "obuchowski" if grouped else "delong"})
    return out


def _delong(summary, models, targets, groups, alpha, device=None, host=False):
    """summary (_delong_summary | _delong_diff_summary) of the exact finish over one stacked table and one Gram matrix of the models:
    through cx_delong_place and cx_delong_gram on `device`, or, host=True, through their numpy statements."""
    _delong_check(alpha)
    plans = _delong_plans(models, targets, groups)
    U, n_cls = plans[0]["n_units"], len(plans[0]["lens"])
    if host:
        table = np.concatenate([delong_place_reference(p["order"], p["offs"], p["lens"], U) for p in plans])
        gram = int_gram_reference(table)
    else:
        import torch

        from . import ops
        table = torch.empty(4 * n_cls * len(plans), U, dtype=torch.int64, device=device)
        for k, p in enumerate(plans):
            ops.delong_place(torch.from_numpy(p["order"]).to(device), p["offs"], p["lens"], U, out=table[4 * n_cls * k:4 * n_cls * (k + 1)])
        gram = ops.int_gram(table, U).cpu()
    return summary(_DelongFinish(_delong_stats(table, len(plans)), gram.tolist(), U), alpha, groups is not None)


def delong_auc(outputs, targets, groups=None, alpha=0.05, device="cuda"):
    """AUROC per class with its analytic standard error and (1 - alpha) normal interval, on the GPU (cx_delong_place + cx_delong_gram;
    no CPU fallback): DeLong's variance (DeLong, DeLong and Clarke-Pearson 1988) for groups=None, Obuchowski's clustered extension
    (1997) with `groups`, one id per row as bootstrap_auc takes them.  Deterministic: no seed, no replicates.  The definitions are in
    the comment above; everything that scales with the rows is integer work on the GPU, the finish is exact on the host.  Returns a
    json-serialisable dict, int class keys: aucs, se, lo, hi (theta -/+ z_{1-alpha/2} se, clipped to [0, 1]; the quantile from
    statistics.NormalDist), n_pos, n_neg, n_units_pos, n_units_neg (M, N, I10, I01); mean_auc: {point, se, lo, hi} of the mean over the
    classes, whose variance is the cluster-robust influence form U / (U - 1) sum_u psibar_u^2 -- it differs from the per-class form only
    in the finite-sample factors; alpha, n_units, method ("delong" | "obuchowski").  A class without a positive or a negative: NaN
    throughout (and the mean with it, as in bootstrap_auc); a class with one positive or one negative unit: se, lo, hi NaN.
    ValueError before any launch: bootstrap_plan's input errors (shapes, NaN scores), more than 32 classes, alpha outside (0, 1), and
    4 max_c(M_c + N_c)^2 sum_u g_u^2 >= 2^63 (g_u the rows of unit u), beyond which the moment sums could overflow."""
    return _delong(_delong_summary, [outputs], targets, groups, alpha, device)


def delong_auc_reference(outputs, targets, groups=None, alpha=0.05):
    """The numpy statement of delong_auc (host: delong_place_reference, int_gram_reference and the same exact finish)."""
    return _delong(_delong_summary, [outputs], targets, groups, alpha, host=True)


def delong_auc_diff(outputs_a, outputs_b, targets, groups=None, alpha=0.05, device="cuda"):
    """DeLong's paired test of the AUROC difference a - b of two models on the same rows (Obuchowski's with `groups`), on the GPU: both
    models' tables stacked, one Gram matrix.  Per class: delta, se, lo, hi (delta -/+ z se, clipped to [-1, 1]), z = delta / se,
    p = erfc(|z| / sqrt 2) and degenerate (Var(delta) <= 0, identical scores for example: z and p are NaN); mean_auc: {delta, se, lo,
    hi, z, p} of the mean over the classes with the influence form of delong_auc on psibar_a - psibar_b; alpha, n_units, method.  At
    most 16 classes; the other errors are those of delong_auc."""
    return _delong(_delong_diff_summary, [outputs_a, outputs_b], targets, groups, alpha, device)


def delong_auc_diff_reference(outputs_a, outputs_b, targets, groups=None, alpha=0.05):
    """The numpy statement of delong_auc_diff."""
    return _delong(_delong_diff_summary, [outputs_a, outputs_b], targets, groups, alpha, host=True)
