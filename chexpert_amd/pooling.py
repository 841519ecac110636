"""Global pooling heads of the fused networks: the average, the maximum, log-sum-exp (LSE; Wang et al., ChestX-ray8, CVPR 2017) and the
generalised mean with a learnable exponent (GeM; Radenovic et al., TPAMI 2019), chosen by `FusedNet.set_pool`.

This module states the kernels of csrc/pool_head.hip in numpy float64 (the definitions also stand in include/chexpert_hip.h), the way
saliency.py and calibration.py state theirs.  With a[b, p, c] = act(x[b, p, c] * sc[c] + sh[c]) over the HW pixels p of image b:

  avg   mean_p a                                                          d pooled / d a = 1 / HW
  max   max_p a                                                           1 at the first maximal pixel in ascending p, else 0
  lse   m + log(mean_p exp(r (a - m))) / r,  m = max_p a,  r > 0          exp(r (a - pooled)) / HW
  gem   (mean_p a'^q)^(1/q),  a' = max(a, 1e-6),  q = clamp(p, 1, 16)     a'^(q-1) pooled^(1-q) / HW where a > 1e-6, else 0

and d pooled / d p = pooled (T - ln pooled) / q with T = sum_p a'^q ln a' / sum_p a'^q, 0 where p is clamped (p <= 1 or p >= 16).
The activation's derivative multiplies d pooled / d a: the ReLU mask z > 0, or swish'(z) = s (1 + z (1 - s)), s = sigmoid(z)."""
import numpy as np

KINDS = ("avg", "max", "lse", "gem")
ACTS = ("relu", "swish")
GEM_EPS = 1e-6
P_MIN, P_MAX = 1.0, 16.0
DEFAULT_R, DEFAULT_P = 10.0, 3.0


def check_pool(kind="avg", r=DEFAULT_R, p=DEFAULT_P):
    """Validates the operands of set_pool; returns (kind, r, p) as (str, float, float).  ValueError otherwise."""
    if kind not in KINDS:
        raise ValueError("pool kind must be one of %s (got %r)" % (", ".join(KINDS), kind))
    try:
        r, p = float(r), float(p)
    except (TypeError, ValueError):
        raise ValueError("pool r and p must be numbers (got r=%r, p=%r)" % (r, p))
    if not (np.isfinite(r) and r > 0.0):
        raise ValueError("pool r must be finite and > 0 (got %r)" % (r,))
    if not P_MIN <= p <= P_MAX:
        raise ValueError("pool p must lie in [%g, %g] (got %r)" % (P_MIN, P_MAX, p))
    return kind, r, p


def _sigmoid(z):
    return 0.5 * (1.0 + np.tanh(0.5 * z))


def activation(z, act):
    """(act(z), act'(z)) in float64"""
    z = np.asarray(z, dtype=np.float64)
    if act == "relu":
        return np.maximum(z, 0.0), (z > 0).astype(np.float64)
    if act == "swish":
        s = _sigmoid(z)
        return z * s, s * (1.0 + z * (1.0 - s))
    raise ValueError("act must be relu or swish (got %r)" % (act,))


def _operands(x, sc, sh, act):
    x = np.asarray(x, dtype=np.float64)
    if x.ndim != 3:
        raise ValueError("x is (B, HW, C)")
    z = x * np.asarray(sc, dtype=np.float64) + np.asarray(sh, dtype=np.float64)
    a, da = activation(z, act)
    return x, a, da


def pool_reference(x, sc, sh, kind, act="relu", r=DEFAULT_R, p=DEFAULT_P):
    """x (B, HW, C), sc / sh (C,) -> (pooled (B, C), aux (B, C)), float64; aux is what the forward kernel leaves for the way back:
    T for gem, the offset pooled - m for lse, None otherwise."""
    if kind not in KINDS:
        raise ValueError("unknown pool kind %r" % (kind,))
    _, a, _ = _operands(x, sc, sh, act)
    if kind == "avg":
        return a.mean(1), None
    m = a.max(1)
    if kind == "max":
        return m, None
    if kind == "lse":
        off = np.log(np.exp(r * (a - m[:, None])).mean(1)) / r
        return m + off, off
    q = min(max(float(p), P_MIN), P_MAX)
    ap = np.maximum(a, GEM_EPS)
    mm = np.maximum(m, GEM_EPS)[:, None]
    w = (ap / mm) ** q                                    # relative to the column maximum: no overflow
    pooled = mm[:, 0] * w.mean(1) ** (1.0 / q)
    T = (w * np.log(ap)).sum(1) / w.sum(1)
    return pooled, T


def pool_weights_reference(x, sc, sh, kind, act="relu", r=DEFAULT_R, p=DEFAULT_P):
    """d pooled[b, c] / d a[b, p, c], (B, HW, C) float64."""
    _, a, _ = _operands(x, sc, sh, act)
    B, HW, C = a.shape
    if kind == "avg":
        return np.full_like(a, 1.0 / HW)
    pooled, _ = pool_reference(x, sc, sh, kind, act, r, p)
    if kind == "max":
        w = np.zeros_like(a)
        first = a.argmax(1)                               # numpy returns the first occurrence
        bi, ci = np.meshgrid(np.arange(B), np.arange(C), indexing="ij")
        w[bi, first, ci] = 1.0
        return w
    if kind == "lse":
        return np.exp(r * (a - pooled[:, None])) / HW
    q = min(max(float(p), P_MIN), P_MAX)
    ap = np.maximum(a, GEM_EPS)
    return np.where(a > GEM_EPS, (ap / pooled[:, None]) ** (q - 1.0) / HW, 0.0)


def pool_backward_reference(dpooled, x, sc, sh, mean, rstd, e_scale, kind, act="relu", r=DEFAULT_R, p=DEFAULT_P):
    """The backward kernel's outputs in float64: g (B, HW, C) = e_scale * dz with dz = dpooled * (d pooled / d a) * act'(z),
    S1 (C,) = sum dz, S2 (C,) = sum dz (x - mean) rstd, and dp = sum dpooled * d pooled / d p (gem; None otherwise)."""
    xx, a, da = _operands(x, sc, sh, act)
    dpooled = np.asarray(dpooled, dtype=np.float64)
    dz = dpooled[:, None, :] * pool_weights_reference(x, sc, sh, kind, act, r, p) * da
    t2 = dz * (xx - np.asarray(mean, dtype=np.float64)) * np.asarray(rstd, dtype=np.float64)
    dp = None
    if kind == "gem":
        dp = float((dpooled * pool_p_derivative_reference(x, sc, sh, act, p)).sum())
    return dz * np.asarray(e_scale, dtype=np.float64), dz.sum((0, 1)), t2.sum((0, 1)), dp


def pool_p_derivative_reference(x, sc, sh, act="relu", p=DEFAULT_P):
    """d pooled / d p of gem, (B, C) float64: pooled (T - ln pooled) / q, 0 where p is clamped."""
    pooled, T = pool_reference(x, sc, sh, "gem", act, p=p)
    if not P_MIN < float(p) < P_MAX:
        return np.zeros_like(pooled)
    return pooled * (T - np.log(pooled)) / float(p)
