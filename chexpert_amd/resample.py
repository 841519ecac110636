"""The resampling core that metrics.py and calibration.py share: the bootstrap draws and their count table, the input checks, the
packing of per-class lists for the kernels, ONE replicate driver for the GPU path and for the numpy statements, and the summaries.

Rows are grouped into U resampling units (an image by default, or a study / a patient); replicate b draws U units with replacement
and weighs every row by the number of times its unit was drawn.  A statistic is an `evaluate(counts)`
callable over a table of such counts; `_replicates` feeds it the row of ones (the point estimate) and the table chunk by chunk, from
cx_boot_counts on the GPU or from `bootstrap_counts_reference` on the host.
"""
import numpy as np

from ._lib import BOOT_MAX_UNITS

_M64 = (1 << 64) - 1
BOOT_TABLE_BYTES = 256 << 20          # budget of the count table: replicates are processed in chunks that stay under it
_HOST_CHUNK = 64                      # replicates per chunk of the host backend (it only bounds the host memory)


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


def _check_scores(outputs, targets, what):
    """(s, t) of the (N, C) scores in the dtype given and the float64 targets; `what` ("bootstrap" | "calibration") opens the messages."""
    s, t = _as_scores(outputs), np.asarray(_as_scores(targets), dtype=np.float64)
    if s.ndim != 2 or s.shape != t.shape:
        raise ValueError("%s: outputs %s and targets %s must be (N, C) arrays of one shape" % (what, s.shape, t.shape))
    if np.isnan(s).any():
        raise ValueError("%s: the scores hold NaN" % what)
    return s, t


def _check_inputs(outputs, targets, groups, what):
    """(s, t, units, U): `_check_scores`, then the unit index of every row and the number of units, 1 .. 2^24.
    groups: one hashable id per row (data.extract_patient_ids output works); the units are the distinct ids.  None: every row its own."""
    s, t = _check_scores(outputs, targets, what)
    units, U = _units_of(s.shape[0], groups)
    if not 1 <= U <= BOOT_MAX_UNITS:
        raise ValueError("%s: %d resampling units (1 .. 2^24 are supported)" % (what, U))
    return s, t, units, U


def _pack_lists(parts, dtype=np.int32):
    """(order, offs, lens) as the kernels read them, from one list per class or one tuple of equally long lists (`hi`, `lo`) per
    class: order holds them back to back, class c from offs[c] (int64) with lens[c] (int32) entries per list."""
    parts = [p if isinstance(p, tuple) else (p,) for p in parts]
    lens = [len(p[0]) for p in parts]
    offs = np.cumsum([0] + [len(p) * n for p, n in zip(parts, lens)], dtype=np.int64)[:-1]
    order = np.concatenate([a for p in parts for a in p]) if parts else np.zeros(0, dtype=dtype)
    return order.astype(dtype), offs, np.asarray(lens, dtype=np.int32)


def _replicates(evaluate, n_units, n_boot, seed, device=None, chunk=None, host=False):
    """The one replicate loop.  evaluate(counts) -> {key: array with one leading row per row of counts}; counts is an (R, U) table,
    an int32 tensor on `device` from cx_boot_counts or, host=True, the uint32 array of `bootstrap_counts_reference` in chunks of 64.
    Returns (point, reps): point[key] = evaluate's row for a count row of ones, reps[key] = the rows of replicates 0 .. n_boot - 1
    (None for n_boot = 0).  On the GPU the replicates run in chunks whose table stays under BOOT_TABLE_BYTES (`chunk`: replicates per
    chunk); a row depends on (seed, replicate, U) alone, so the result does not depend on the chunking."""
    U, n_boot = int(n_units), int(n_boot)
    if host:
        chunk, ones = _HOST_CHUNK, np.ones((1, U), dtype=np.uint32)

        def draw(first, n):
            return bootstrap_counts_reference(U, n, seed, first=first)
    else:
        import torch

        from . import ops
        if chunk is None:
            chunk = max(1, BOOT_TABLE_BYTES // (4 * U))
        chunk = max(1, min(int(chunk), n_boot))
        ones = torch.ones(1, U, dtype=torch.int32, device=device)
        table = torch.empty(chunk if n_boot else 0, U, dtype=torch.int32, device=device)

        def draw(first, n):
            return ops.boot_counts(U, n, seed, first=first, out=table)
    point = {key: v[0] for key, v in evaluate(ones).items()}
    chunks = [evaluate(draw(first, min(chunk, n_boot - first))) for first in range(0, n_boot, chunk)]
    if len(chunks) < 2:                                           # the usual case on the GPU: one chunk, handed over without a copy
        return point, chunks[0] if chunks else None
    return point, {key: np.concatenate([c[key] for c in chunks]) for key in point}


def _check_boot(n_boot, alpha):
    if int(n_boot) < 1:
        raise ValueError("bootstrap: n_boot must be >= 1 (got %r)" % n_boot)
    if not 0.0 < alpha < 1.0:
        raise ValueError("bootstrap: alpha must be inside (0, 1) (got %r)" % alpha)


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


def _summarise_metric(*args):
    s = _summarise(*args)
    return {"point": s.pop("aucs"), **s}


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
