"""Evaluation metrics of the reference (`compute_metrics`, /root/reference/chexpert.py:130-146).

The reference calls sklearn `roc_curve` / `auc` / `precision_recall_curve` per class on raw logits.
Here the ROC / PR curves are built directly (descending score sweep with tie groups collapsed, as
sklearn's `_binary_clf_curve` does) and the AUROC is the trapezoid area.  Host-side numpy: this runs once
per evaluation on (N, 5) arrays and is not on the GPU hot path.
"""
import re

import numpy as np


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
_M64 = (1 << 64) - 1
BOOT_MAX_UNITS = 1 << 24
BOOT_TABLE_BYTES = 256 << 20          # budget of the count table: replicates are processed in chunks that stay under it


def splitmix64(seed, k):
    """The draw hash: the splitmix64 finaliser of seed + 0x9E3779B97F4A7C15 * (k + 1) mod 2^64 (what effnet.hip uses for dropout), on
    Python ints."""
    z = (seed + 0x9E3779B97F4A7C15 * (k + 1)) & _M64
    z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & _M64
    z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & _M64
    return z ^ (z >> 31)


def bootstrap_draws(n_units, b, seed):
    """The n_units unit indices replicate b draws: unit = ((splitmix64(seed, b * U + j) >> 32) * U) >> 32, in uint64 numpy arithmetic
    (which wraps mod 2^64 as the definition asks).  The multiply-shift favours some units by at most U / 2^32 in probability."""
    U = int(n_units)
    with np.errstate(over="ignore"):
        k = np.uint64((int(b) * U) & _M64) + np.arange(U, dtype=np.uint64)
        z = np.uint64(int(seed) & _M64) + np.uint64(0x9E3779B97F4A7C15) * (k + np.uint64(1))
        z = (z ^ (z >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)
        z = (z ^ (z >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)
        z = z ^ (z >> np.uint64(31))
        return (((z >> np.uint64(32)) * np.uint64(U)) >> np.uint64(32)).astype(np.int64)


def bootstrap_counts_reference(n_units, n_rep, seed, first=0):
    """Statement of cx_boot_counts: (n_rep, n_units) uint32, row r = how often each unit is drawn by replicate first + r."""
    U = int(n_units)
    if not 1 <= U <= BOOT_MAX_UNITS:
        raise ValueError("bootstrap: %d resampling units (1 .. 2^24 are supported)" % U)
    out = np.zeros((int(n_rep), U), dtype=np.uint32)
    for r in range(int(n_rep)):
        out[r] = np.bincount(bootstrap_draws(U, first + r, seed), minlength=U)
    return out


def _as_scores(a):
    if hasattr(a, "detach"):                    # a torch tensor: numpy has no bfloat16 (the conversion to fp32 keeps its order and ties)
        a = a.detach().cpu()
        a = (a.float() if str(a.dtype) in ("torch.bfloat16", "torch.float16") else a).numpy()
    return np.asarray(a)


def _units_of(n_rows, groups):
    if groups is None:
        return np.arange(n_rows, dtype=np.int64), n_rows
    g = np.asarray(groups)
    if g.shape != (n_rows,):
        raise ValueError("bootstrap: groups holds %s ids for %d rows" % (g.shape, n_rows))
    ids, inv = np.unique(g, return_inverse=True)
    return inv.reshape(-1).astype(np.int64), int(len(ids))


def bootstrap_plan(outputs, targets, groups=None):
    """What cx_boot_auc reads, built once per call on the host (N log N): for every class the kept rows (target >= 0) in two orders,
    both ascending in score (compared in the dtype given): `hi` with the negatives of a tie group before its positives, `lo` with the
    positives first.  An entry is the row's unit index with the label (target > 0.5) in bit 31.
    groups: one hashable id per row (data.extract_patient_ids output works); the units are the distinct ids.  None: every row its own.
    Returns {"order": int32 (for class c: hi then lo, lens[c] entries each, from offs[c]), "offs": int64 (C), "lens": int32 (C),
    "units": int64 (N) unit index of every row, "n_units": U}."""
    s, t = _as_scores(outputs), np.asarray(_as_scores(targets), dtype=np.float64)
    if s.ndim != 2 or s.shape != t.shape:
        raise ValueError("bootstrap: outputs %s and targets %s must be (N, C) arrays of one shape" % (s.shape, t.shape))
    if np.isnan(s).any():
        raise ValueError("bootstrap: the scores hold NaN")
    units, U = _units_of(s.shape[0], groups)
    if not 1 <= U <= BOOT_MAX_UNITS:
        raise ValueError("bootstrap: %d resampling units (1 .. 2^24 are supported)" % U)
    parts, offs, lens, at = [], [], [], 0
    for c in range(s.shape[1]):
        keep = np.nonzero(t[:, c] >= 0)[0]
        pos = t[keep, c] > 0.5
        rank = np.unique(s[keep, c], return_inverse=True)[1].reshape(-1)
        entry = (units[keep] | (pos.astype(np.int64) << 31)).astype(np.uint32).view(np.int32)
        parts += [entry[np.lexsort((pos, rank))], entry[np.lexsort((~pos, rank))]]
        offs.append(at)
        lens.append(len(keep))
        at += 2 * len(keep)
    order = np.concatenate(parts) if parts else np.zeros(0, dtype=np.int32)
    return {"order": order.astype(np.int32), "offs": np.asarray(offs, dtype=np.int64), "lens": np.asarray(lens, dtype=np.int32),
            "units": units, "n_units": U}


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


def _interval(v, alpha):
    """(lo, hi, se, n_degenerate) of one column of replicates: percentiles and the ddof-1 deviation over the non-degenerate ones."""
    ok = v[~np.isnan(v)]
    lo, hi = (float(np.percentile(ok, 100.0 * q)) for q in (alpha / 2, 1 - alpha / 2)) if len(ok) else (float("nan"), float("nan"))
    return lo, hi, float(np.std(ok, ddof=1)) if len(ok) > 1 else float("nan"), int(len(v) - len(ok))


def _row_mean(a):
    """Mean over the classes, NaN where any class is (np.mean propagates it)."""
    return a.mean(axis=1) if a.shape[1] else np.full(a.shape[0], np.nan)


def _summarise(point, rep, n_boot, seed, alpha, n_units, return_replicates):
    C = rep.shape[1]
    cols = [_interval(rep[:, c], alpha) for c in range(C)]
    m = _interval(_row_mean(rep), alpha)
    out = {"aucs": {c: float(point[c]) for c in range(C)}, "lo": {c: cols[c][0] for c in range(C)}, "hi": {c: cols[c][1] for c in range(C)},
           "se": {c: cols[c][2] for c in range(C)}, "n_degenerate": {c: cols[c][3] for c in range(C)},
           "mean_auc": {"point": float(_row_mean(point[None])[0]), "lo": m[0], "hi": m[1], "se": m[2]},
           "n_boot": int(n_boot), "seed": int(seed), "alpha": float(alpha), "n_units": int(n_units)}
    if return_replicates:
        out["replicates"] = rep
    return out


def _p_two_sided(d):
    ok = d[~np.isnan(d)]
    if not len(ok):
        return float("nan")
    return float(min(1.0, 2.0 * min((np.sum(ok <= 0) + 1.0) / (len(ok) + 1.0), (np.sum(ok >= 0) + 1.0) / (len(ok) + 1.0))))


def _summarise_diff(point_a, point_b, rep_a, rep_b, n_boot, seed, alpha, n_units, return_replicates):
    C = rep_a.shape[1]
    d = rep_a - rep_b                                         # NaN where either model's replicate is degenerate
    cols = [_interval(d[:, c], alpha) for c in range(C)]
    dm = _row_mean(rep_a) - _row_mean(rep_b)
    m = _interval(dm, alpha)
    out = {"delta": {c: float(point_a[c] - point_b[c]) for c in range(C)}, "lo": {c: cols[c][0] for c in range(C)},
           "hi": {c: cols[c][1] for c in range(C)}, "p": {c: _p_two_sided(d[:, c]) for c in range(C)},
           "n_degenerate": {c: cols[c][3] for c in range(C)},
           "mean_auc": {"delta": float(_row_mean(point_a[None])[0] - _row_mean(point_b[None])[0]), "lo": m[0], "hi": m[1],
                        "p": _p_two_sided(dm)},
           "n_boot": int(n_boot), "seed": int(seed), "alpha": float(alpha), "n_units": int(n_units)}
    if return_replicates:
        out["replicates"] = d
    return out


def _check_boot(n_boot, alpha):
    if int(n_boot) < 1:
        raise ValueError("bootstrap: n_boot must be >= 1 (got %r)" % n_boot)
    if not 0.0 < alpha < 1.0:
        raise ValueError("bootstrap: alpha must be inside (0, 1) (got %r)" % alpha)


def _replicates_gpu(plans, n_boot, seed, device, chunk):
    """[(point (C), replicates (n_boot, C))] per plan, all plans over ONE count table per chunk of replicates (the paired comparison)."""
    import torch

    from . import ops
    U = plans[0]["n_units"]
    assert all(p["n_units"] == U for p in plans)
    if chunk is None:
        chunk = max(1, BOOT_TABLE_BYTES // (4 * U))
    chunk = max(1, min(int(chunk), int(n_boot)))
    orders = [torch.from_numpy(p["order"]).to(device) for p in plans]
    table = torch.empty(chunk, U, dtype=torch.int32, device=device)
    ones = torch.ones(1, U, dtype=torch.int32, device=device)
    points = [_auc_of(*(v.cpu().numpy() for v in ops.boot_auc(ones, o, p["offs"], p["lens"], U)))[0] for p, o in zip(plans, orders)]
    reps = [[] for _ in plans]
    for first in range(0, int(n_boot), chunk):
        counts = ops.boot_counts(U, min(chunk, int(n_boot) - first), seed, first=first, out=table)
        for k, (p, o) in enumerate(zip(plans, orders)):
            reps[k].append(_auc_of(*(v.cpu().numpy() for v in ops.boot_auc(counts, o, p["offs"], p["lens"], U))))
    return [(pt, np.concatenate(r)) for pt, r in zip(points, reps)]


def _replicates_reference(outputs, targets, groups, n_boot, seed):
    s, t = _as_scores(outputs), np.asarray(_as_scores(targets), dtype=np.float64)
    units, U = _units_of(s.shape[0], groups)
    point = _auc_of(*_definition_parts(s, t, units, np.ones((1, U), dtype=np.int64)))[0]
    reps = []
    for first in range(0, int(n_boot), 64):                       # (chunks only bound the host memory: a row depends on its index alone)
        counts = bootstrap_counts_reference(U, min(64, int(n_boot) - first), seed, first=first)
        reps.append(_auc_of(*_definition_parts(s, t, units, counts)))
    return point, np.concatenate(reps), U


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
    _check_boot(n_boot, alpha)
    plan = bootstrap_plan(outputs, targets, groups)
    (point, rep), = _replicates_gpu([plan], n_boot, seed, device, chunk)
    return _summarise(point, rep, n_boot, seed, alpha, plan["n_units"], return_replicates)


def bootstrap_auc_reference(outputs, targets, n_boot=1000, seed=0, groups=None, alpha=0.05, return_replicates=False):
    """The numpy statement of bootstrap_auc (host, integers from the definition; for the tests and as the timing yardstick)."""
    _check_boot(n_boot, alpha)
    point, rep, U = _replicates_reference(outputs, targets, groups, n_boot, seed)
    return _summarise(point, rep, n_boot, seed, alpha, U, return_replicates)


def bootstrap_auc_diff(outputs_a, outputs_b, targets, n_boot=1000, seed=0, groups=None, alpha=0.05, device="cuda", chunk=None,
                       return_replicates=False):
    """Paired bootstrap of the AUROC difference of two models on the same rows (one count table, two plans).  Per class and under
    "mean_auc" for the mean over the classes: delta (a - b), lo, hi (percentiles of the replicate differences) and p, two-sided:
    2 min((#{d* <= 0} + 1) / (B' + 1), (#{d* >= 0} + 1) / (B' + 1)) capped at 1, B' = the replicates degenerate in neither model."""
    _check_boot(n_boot, alpha)
    pa, pb = bootstrap_plan(outputs_a, targets, groups), bootstrap_plan(outputs_b, targets, groups)
    (point_a, rep_a), (point_b, rep_b) = _replicates_gpu([pa, pb], n_boot, seed, device, chunk)
    return _summarise_diff(point_a, point_b, rep_a, rep_b, n_boot, seed, alpha, pa["n_units"], return_replicates)


def bootstrap_auc_diff_reference(outputs_a, outputs_b, targets, n_boot=1000, seed=0, groups=None, alpha=0.05, return_replicates=False):
    """The numpy statement of bootstrap_auc_diff."""
    _check_boot(n_boot, alpha)
    point_a, rep_a, U = _replicates_reference(outputs_a, targets, groups, n_boot, seed)
    point_b, rep_b, _ = _replicates_reference(outputs_b, targets, groups, n_boot, seed)
    return _summarise_diff(point_a, point_b, rep_a, rep_b, n_boot, seed, alpha, U, return_replicates)


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
BOOT_MAX_POINTS, BOOT_SENS, BOOT_SPEC, BOOT_PPM = 8, 0, 1, 10 ** 6
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
    s, t = _as_scores(outputs), np.asarray(_as_scores(targets), dtype=np.float64)
    if s.ndim != 2 or s.shape != t.shape:
        raise ValueError("bootstrap: outputs %s and targets %s must be (N, C) arrays of one shape" % (s.shape, t.shape))
    if np.isnan(s).any():
        raise ValueError("bootstrap: the scores hold NaN")
    units, U = _units_of(s.shape[0], groups)
    if not 1 <= U <= BOOT_MAX_UNITS:
        raise ValueError("bootstrap: %d resampling units (1 .. 2^24 are supported)" % U)
    parts, offs, lens, at = [], [], [], 0
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
        offs.append(at)
        lens.append(len(keep))
        at += len(keep)
    order = np.concatenate(parts) if parts else np.zeros(0, dtype=np.int32)
    return {"order": order.astype(np.int32), "offs": np.asarray(offs, dtype=np.int64), "lens": np.asarray(lens, dtype=np.int32),
            "units": units, "n_units": U}


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


def _summarise_metric(*args):
    s = _summarise(*args)
    return {"point": s.pop("aucs"), **s}


def _metric_replicates_gpu(models, targets, names, points, n_boot, seed, groups, device, chunk):
    """[{name: (point (C), replicates (n_boot, C))}] per model, every model and every metric over ONE count table per chunk of
    replicates; the point estimate goes through the same kernels with a row of ones."""
    import torch

    from . import ops
    auc = [bootstrap_plan(o, targets, groups) if "auroc" in names else None for o in models]
    swp = [bootstrap_sweep_plan(o, targets, groups) if len(names) > ("auroc" in names) else None for o in models]
    U = (auc[0] or swp[0])["n_units"]
    if chunk is None:
        chunk = max(1, BOOT_TABLE_BYTES // (4 * U))
    chunk = max(1, min(int(chunk), int(n_boot)))
    dev_order = [[None if p is None else torch.from_numpy(p["order"]).to(device) for p in (a, s)] for a, s in zip(auc, swp)]

    def evaluate(counts, k):
        out = {}
        if auc[k] is not None:
            out["auroc"] = _auc_of(*(v.cpu().numpy() for v in ops.boot_auc(counts, dev_order[k][0], auc[k]["offs"], auc[k]["lens"], U)))
        if swp[k] is not None:
            got = ops.boot_sweep(counts, dev_order[k][1], swp[k]["offs"], swp[k]["lens"], U, points)
            apnum, wpos, wneg, pts = (v.cpu().numpy() for v in got)
            out.update(_sweep_values(names, points, apnum.view(np.uint64), wpos, wneg, pts))
        return out

    table = torch.empty(chunk, U, dtype=torch.int32, device=device)
    ones = torch.ones(1, U, dtype=torch.int32, device=device)
    point = [evaluate(ones, k) for k in range(len(models))]
    reps = [{name: [] for name in names} for _ in models]
    for first in range(0, int(n_boot), chunk):
        counts = ops.boot_counts(U, min(chunk, int(n_boot) - first), seed, first=first, out=table)
        for k in range(len(models)):
            for name, v in evaluate(counts, k).items():
                reps[k][name].append(v)
    return [{name: (point[k][name][0], np.concatenate(reps[k][name])) for name in names} for k in range(len(models))], U


def _metric_replicates_reference(outputs, targets, names, points, n_boot, seed, groups):
    """{name: (point, replicates)} on the host: the AUROC as bootstrap_auc_reference forms it, the sweep's metrics through the numpy
    statement of the kernel over the prepared plan."""
    out, U = {}, None
    if "auroc" in names:
        point, rep, U = _replicates_reference(outputs, targets, groups, n_boot, seed)
        out["auroc"] = (point, rep)
    if len(names) > ("auroc" in names):
        plan = bootstrap_sweep_plan(outputs, targets, groups)
        U = plan["n_units"]

        def values(counts):
            return _sweep_values(names, points, *bootstrap_sweep_reference(counts, plan["order"], plan["offs"], plan["lens"], U, points))
        point, reps = values(np.ones((1, U), dtype=np.uint32)), []
        for first in range(0, int(n_boot), 64):
            reps.append(values(bootstrap_counts_reference(U, min(64, int(n_boot) - first), seed, first=first)))
        out.update({name: (point[name][0], np.concatenate([r[name] for r in reps])) for name in point})
    return {name: out[name] for name in names}, U


def bootstrap_metrics(outputs, targets, metrics=("auroc", "ap"), n_boot=1000, seed=0, groups=None, alpha=0.05, device="cuda", chunk=None,
                      return_replicates=False):
    """Percentile bootstrap intervals of several evaluation metrics over the SAME resamples, on the GPU (cx_boot_counts, cx_boot_auc,
    cx_boot_sweep; no CPU fallback).  metrics: "auroc", "ap" (average precision, the step sum), "sens@S" (sensitivity at specificity
    >= S) and "spec@S" (specificity at sensitivity >= S), S a decimal inside (0, 1) with at most 6 decimals, at most 8 operating
    points in one call.  The other arguments are those of bootstrap_auc.  Returns {name: summary}; a summary has the keys of
    bootstrap_auc's result with "point" in place of "aucs" ("mean_auc" is the metric's mean over the classes), and the "auroc"
    summary carries the numbers of bootstrap_auc with the same arguments, bit for bit."""
    _check_boot(n_boot, alpha)
    names, points = parse_boot_metrics(metrics)
    (res,), U = _metric_replicates_gpu([outputs], targets, names, points, n_boot, seed, groups, device, chunk)
    return {name: _summarise_metric(*res[name], n_boot, seed, alpha, U, return_replicates) for name in names}


def bootstrap_metrics_reference(outputs, targets, metrics=("auroc", "ap"), n_boot=1000, seed=0, groups=None, alpha=0.05,
                                return_replicates=False):
    """The numpy statement of bootstrap_metrics (host; for the tests and as the timing yardstick)."""
    _check_boot(n_boot, alpha)
    names, points = parse_boot_metrics(metrics)
    res, U = _metric_replicates_reference(outputs, targets, names, points, n_boot, seed, groups)
    return {name: _summarise_metric(*res[name], n_boot, seed, alpha, U, return_replicates) for name in names}


def bootstrap_metrics_diff(outputs_a, outputs_b, targets, metrics=("auroc", "ap"), n_boot=1000, seed=0, groups=None, alpha=0.05,
                           device="cuda", chunk=None, return_replicates=False):
    """Paired bootstrap of the difference a - b of every named metric between two models on the same rows (one count table, two plans
    per kernel).  Returns {name: what bootstrap_auc_diff returns for the AUROC}."""
    _check_boot(n_boot, alpha)
    names, points = parse_boot_metrics(metrics)
    (a, b), U = _metric_replicates_gpu([outputs_a, outputs_b], targets, names, points, n_boot, seed, groups, device, chunk)
    return {name: _summarise_diff(a[name][0], b[name][0], a[name][1], b[name][1], n_boot, seed, alpha, U, return_replicates)
            for name in names}


def bootstrap_metrics_diff_reference(outputs_a, outputs_b, targets, metrics=("auroc", "ap"), n_boot=1000, seed=0, groups=None, alpha=0.05,
                                     return_replicates=False):
    """The numpy statement of bootstrap_metrics_diff."""
    _check_boot(n_boot, alpha)
    names, points = parse_boot_metrics(metrics)
    a, U = _metric_replicates_reference(outputs_a, targets, names, points, n_boot, seed, groups)
    b, _ = _metric_replicates_reference(outputs_b, targets, names, points, n_boot, seed, groups)
    return {name: _summarise_diff(a[name][0], b[name][0], a[name][1], b[name][1], n_boot, seed, alpha, U, return_replicates)
            for name in names}
