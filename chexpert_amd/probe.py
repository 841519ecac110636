"""The linear probe of a frozen backbone: logistic regression on its pooled features, fitted on the GPU.

The linear evaluation SimCLR, MoCo and MoCo-CXR report: freeze the network, embed a bank of labelled training images (FusedNet.embed,
knn.embed_dataset), fit one linear classifier per finding on the bank and report the AUROC per finding on the validation set.  On a
fixed bank that is a convex problem -- multi-label L2-regularised logistic regression -- so the fit needs no backward pass through the
network and its result is the optimum itself: deterministic and comparable between checkpoints.

The definition.  X (M, d) fp32; Y (M, n) fp32 in [0, 1], a value < 0 = an ignored label (the convention of knn_vote, MaskedBCE and
--uncertain ignore); theta (n, d + 1) row-major, theta[c, :d] = w_c, theta[c, d] = b_c; pos_weight (n,), default ones; l2 >= 0.  Per
class c over its live rows (y_ic >= 0), N_c = max(their number, 1), z_ic = x_i . w_c + b_c:

    f_c       = (1 / N_c) sum_live [pw_c y softplus(-z) + (1 - y) softplus(z)] + (l2 / 2) |w_c|^2      (the bias is not regularised)
    r_ic      = (pw_c y + 1 - y) sigmoid(z) - pw_c y   (0 for an ignored row)
    df_c/dw_c = (1 / N_c) sum_i r_ic x_i + l2 w_c,      df_c/db_c = (1 / N_c) sum_i r_ic

The classes do not couple: n independent problems in lockstep over one shared pass of the bank (ops.probe_loss_grad, csrc/probe.hip).
A class is DEGENERATE when its live rows hold no positive mass (sum y == 0) or no negative mass (sum (1 - y) == 0) -- no live row is
both: its result is theta_c = 0 with status 2.

Standardisation (the default): mean_k and std_k the population mean and standard deviation of the bank's columns, rstd_k =
1 / max(std_k, 1e-6) (a definition: a dead channel has x - mean = 0 and stays 0); the fit runs on (x - mean) * rstd and is folded back
to raw-feature coordinates on the host in float64, rounded once: W_raw = W * rstd, b_raw = b - W_raw . mean, so that
classifier(embed(x)) gives the probe's logits.

The solver is L-BFGS per class with Armijo backtracking (c1 = 1e-4, the step halved at most 30 times; the first step min(1, 1 / |g|_1),
later ones start at 1).  The sufficient decrease f(theta_t) <= f(theta) + c1 t g . dir is read off the fp32 losses, or, where a step
lowers the loss by less than its last bit, off the trial's slope: f is convex, so f(theta_t) <= f(theta) + t g_t . dir, and
g_t . dir <= c1 g . dir certifies the same inequality.  The solver's vector arithmetic runs in csrc/probe.hip
(ops.probe_lbfgs_direction / probe_lbfgs_advance); the host steers from O(n) numbers per pass.  Status per class: 0 converged
(|g|_inf <= g_tol), 1 max_iter reached, 2 degenerate, 3 the line search was exhausted (the fp32 floor; `gmax` tells how far it got).

`reference_loss_grad`, `reference_optimum` and `reference_colstats` are the definitions in numpy float64 which the tests hold the
kernels and the fit to.
"""
import numpy as np
import torch

from . import ops

U = 2.0 ** -24                    # the unit roundoff of fp32
STD_FLOOR = 1e-6
ARMIJO_C1, MAX_HALVINGS = 1e-4, 30
STATUS = {0: "converged", 1: "max_iter", 2: "degenerate", 3: "line search exhausted"}


# ---- the definitions in numpy float64 ------------------------------------------------------------------------------------------------
def _softplus(z):
    return np.maximum(z, 0.0) + np.log1p(np.exp(-np.abs(z)))


def _sigmoid(z):
    e = np.exp(-np.abs(z))
    return np.where(z >= 0, 1.0, e) / (1.0 + e)


def reference_colstats(X):
    """(mean, std, rstd) of the columns of X in float64: the population statistics and rstd = 1 / max(std, 1e-6)."""
    X = np.asarray(X, dtype=np.float64)
    mean = X.mean(axis=0)
    std = np.sqrt(((X - mean) ** 2).mean(axis=0))
    return mean, std, 1.0 / np.maximum(std, STD_FLOOR)


def degenerate(Y):
    """(n,) bool: the classes whose live labels hold no positive or no negative mass (a class without a live row among them)."""
    Y = np.asarray(Y, dtype=np.float64)
    live = Y >= 0
    return (np.where(live, Y, 0.0).sum(axis=0) == 0) | (np.where(live, 1.0 - Y, 0.0).sum(axis=0) == 0)


def reference_loss_grad(X, Y, theta, pos_weight=None, l2=0.0):
    """(loss (n,), grad (n, d + 1), E_loss (n,), E_grad (n, d + 1)) of the module docstring's definition in float64.  The E are
    first-order bounds on the error of ANY fp32 evaluation of the same formulas (any summation order), u = 2^-24:
      logit     dz  = (d + 2) u (sum_k |x w| + |b|)
      residual  dr  = wgt (dz / 4 + 8 u) + 2 u |pw y|          wgt = pw y + 1 - y; 8 u: one expf (1 ulp), one add, one divide, the weight
      loss term del = wgt dz + 8 u el                           |d softplus| <= 1; log1pf is 2 ulp
      gradient  E   = [(M + 2) u sum_i |r x| + sum_i dr |x|] / N_c + 4 u |l2 w| + 2 u |G|      (the bias column: x = 1, no l2 term)
      loss      E   = [(M + 2) u sum_i el + sum_i del] / N_c + (d + 4) u (l2 / 2) |w|^2 + 2 u |f|."""
    X, Y, theta = np.asarray(X, dtype=np.float64), np.asarray(Y, dtype=np.float64), np.asarray(theta, dtype=np.float64)
    (M, d), n = X.shape, Y.shape[1]
    assert theta.shape == (n, d + 1)
    pw = np.ones(n) if pos_weight is None else np.asarray(pos_weight, dtype=np.float64).reshape(n)
    W, b = theta[:, :d], theta[:, d]
    live = Y >= 0
    N = np.maximum(live.sum(axis=0), 1).astype(np.float64)
    y = np.where(live, Y, 0.0)
    z = X @ W.T + b
    pwy, omy = pw * y, 1.0 - y
    wgt = pwy + omy
    el = np.where(live, pwy * _softplus(-z) + omy * _softplus(z), 0.0)
    r = np.where(live, wgt * _sigmoid(z) - pwy, 0.0)
    ww = (W * W).sum(axis=1)
    loss = el.sum(axis=0) / N + 0.5 * l2 * ww
    grad = np.empty((n, d + 1))
    grad[:, :d] = (r.T @ X) / N[:, None] + l2 * W
    grad[:, d] = r.sum(axis=0) / N
    # the bounds
    aX = np.abs(X)
    dz = (d + 2) * U * (aX @ np.abs(W).T + np.abs(b))
    dr = np.where(live, wgt * (dz / 4 + 8 * U) + 2 * U * np.abs(pwy), 0.0)
    del_ = np.where(live, wgt * dz + 8 * U * el, 0.0)
    E_grad = np.empty((n, d + 1))
    E_grad[:, :d] = ((M + 2) * U * (np.abs(r).T @ aX) + dr.T @ aX) / N[:, None] + 4 * U * np.abs(l2 * W)
    E_grad[:, d] = ((M + 2) * U * np.abs(r).sum(axis=0) + dr.sum(axis=0)) / N
    E_grad += 2 * U * np.abs(grad)
    E_loss = ((M + 2) * U * el.sum(axis=0) + del_.sum(axis=0)) / N + (d + 4) * U * 0.5 * l2 * ww + 2 * U * np.abs(loss)
    return loss, grad, E_loss, E_grad


def reference_optimum(X, Y, pos_weight=None, l2=0.0, tol=1e-13, max_iter=200):
    """theta* (n, d + 1) in float64: damped Newton per class on the (d + 1)^2 Hessian until |g|_inf < tol.  For small d only.  A
    degenerate class is theta = 0.  l2 > 0, or data that is not separable, makes the optimum finite."""
    X, Y = np.asarray(X, dtype=np.float64), np.asarray(Y, dtype=np.float64)
    (M, d), n = X.shape, Y.shape[1]
    pw = np.ones(n) if pos_weight is None else np.asarray(pos_weight, dtype=np.float64).reshape(n)
    X1 = np.concatenate([X, np.ones((M, 1))], axis=1)
    reg = np.full(d + 1, float(l2))
    reg[d] = 0.0
    theta = np.zeros((n, d + 1))
    dead = degenerate(Y)
    for c in range(n):
        if dead[c]:
            continue
        live = Y[:, c] >= 0
        A, y = X1[live], Y[live, c]
        N = max(len(y), 1)
        pwy, omy = pw[c] * y, 1.0 - y
        wgt = pwy + omy

        def f(t):
            z = A @ t
            return (pwy * _softplus(-z) + omy * _softplus(z)).sum() / N + 0.5 * (reg * t * t).sum()

        t = np.zeros(d + 1)
        for _ in range(max_iter):
            z = A @ t
            s = _sigmoid(z)
            g = A.T @ (wgt * s - pwy) / N + reg * t
            if np.abs(g).max() < tol:
                break
            H = (A * (wgt * s * (1.0 - s))[:, None]).T @ A / N + np.diag(reg)
            try:
                step = np.linalg.solve(H, g)
            except np.linalg.LinAlgError:                                  # l2 == 0 and a direction the data does not see
                step = np.linalg.lstsq(H, g, rcond=None)[0]
            f0, gs, a = f(t), g @ step, 1.0
            while a > 1e-12 and f(t - a * step) > f0 - 1e-4 * a * gs:
                a *= 0.5
            t = t - a * step
        theta[c] = t
    return theta


def fold_back(theta, mean, rstd):
    """(W_raw (n, d), b_raw (n,)) in float64 of a theta fitted on (x - mean) * rstd: W_raw = W * rstd, b_raw = b - W_raw . mean."""
    theta, mean, rstd = (np.asarray(v, dtype=np.float64) for v in (theta, mean, rstd))
    W = theta[:, :-1] * rstd
    return W, theta[:, -1] - W @ mean


# ---- the fit on the GPU ------------------------------------------------------------------------------------------------------------
def _prepare(feats, standardize):
    """(the bank the fit runs on, mean, rstd): the standardised copy of feats and its statistics, or feats itself and (None, None)."""
    if feats.dim() != 2 or feats.shape[0] < 1:
        raise ValueError("the bank is (M, d) with M >= 1 (got %s)" % (tuple(feats.shape),))
    X = feats.to(torch.float32).contiguous()
    if not standardize:
        return X, None, None
    d = X.shape[1]
    mean, rstd = torch.empty(d, dtype=torch.float32, device=X.device), torch.empty(d, dtype=torch.float32, device=X.device)
    ops.probe_colstats(X, mean, rstd)
    return ops.probe_standardize(X, mean, rstd, torch.empty_like(X)), mean, rstd


def _solve(X, Y, l2, pos_weight, g_tol, max_iter, history, theta0, splits):
    (M, d), n, dev = X.shape, Y.shape[1], X.device
    f32 = dict(dtype=torch.float32, device=dev)
    i32 = dict(dtype=torch.int32, device=dev)
    if not 1 <= int(history) <= ops.PROBE_MAX_HISTORY:
        raise ValueError("history takes 1 .. %d pairs (got %r)" % (ops.PROBE_MAX_HISTORY, history))
    if not (g_tol >= 0 and max_iter >= 0):
        raise ValueError("g_tol and max_iter are >= 0 (got %r, %r)" % (g_tol, max_iter))
    m = int(history)
    theta = torch.zeros(n, d + 1, **f32)
    if theta0 is not None:
        theta0 = torch.as_tensor(theta0)
        if tuple(theta0.shape) != (n, d + 1):
            raise ValueError("theta0 is (n, d + 1) = (%d, %d) (got %s)" % (n, d + 1, tuple(theta0.shape)))
        theta.copy_(theta0.to(**f32))
    pw = None if pos_weight is None else torch.as_tensor(pos_weight).to(**f32).reshape(-1).contiguous()
    if pw is not None and pw.numel() != n:
        raise ValueError("pos_weight has %d entries for %d classes" % (pw.numel(), n))
    grad, theta_t, grad_t, direction = (torch.zeros(n, d + 1, **f32) for _ in range(4))
    loss, loss_t = torch.zeros(n, **f32), torch.zeros(n, **f32)
    count, count_t, stats, tstats = torch.zeros(n, 3, **f32), torch.zeros(n, 3, **f32), torch.zeros(n, 4, **f32), torch.zeros(n, 2, **f32)
    s_hist, y_hist, hist = torch.zeros(n, m, d + 1, **f32), torch.zeros(n, m, d + 1, **f32), torch.zeros(n, 2, **i32)
    scratch = ops.probe_loss_grad(X, Y, theta, loss, grad, count, pw, l2, None, None, splits)
    passes = 1
    cnt = count.cpu().numpy().astype(np.float64)
    dead = (cnt[:, 0] == 0) | (cnt[:, 1] == 0) | (cnt[:, 2] == 0)
    status = np.where(dead, 2, -1).astype(np.int64)            # -1: still running
    iters = np.zeros(n, dtype=np.int64)
    f = loss.cpu().numpy().astype(np.float64)
    gmax, gd = np.zeros(n), np.zeros(n)
    t, halvings = np.ones(n), np.zeros(n, dtype=np.int64)

    def flags(mask):
        return torch.as_tensor(np.asarray(mask, dtype=np.int32), device=dev)

    def advance(mode):
        ops.probe_lbfgs_advance(theta, grad, direction, torch.as_tensor(t, **f32), flags(mode), theta_t, grad_t, s_hist, y_hist, hist,
                                tstats)

    def new_direction(mask, first):
        """The direction of the classes of `mask` at their (new) theta; those that have converged or used up max_iter retire."""
        ops.probe_lbfgs_direction(grad, s_hist, y_hist, hist, direction, stats, flags(mask))
        st = stats.cpu().numpy().astype(np.float64)
        for c in np.flatnonzero(mask):
            gd[c], gmax[c] = st[c, 0], st[c, 1]
            if gmax[c] <= g_tol:
                status[c] = 0
            elif iters[c] >= max_iter:
                status[c] = 1
            else:
                t[c], halvings[c] = (min(1.0, 1.0 / st[c, 2]) if first else 1.0), 0

    new_direction(status < 0, True)
    while (status < 0).any():
        run = status < 0
        advance(run)
        ops.probe_loss_grad(X, Y, theta_t, loss_t, grad_t, count_t, pw, l2, flags(run), scratch, splits)
        advance(run * 3)
        passes += 1
        ft, slope = loss_t.cpu().numpy().astype(np.float64), tstats.cpu().numpy().astype(np.float64)[:, 0]
        accept = np.zeros(n, dtype=bool)
        for c in np.flatnonzero(run):
            # the sufficient decrease as the fp32 loss shows it, or as the trial's slope certifies it: f is convex, so f(theta_t) <=
            # f(theta) + t g_t . dir <= f(theta) + c1 t g . dir wherever g_t . dir <= c1 g . dir.  Near the optimum a step lowers
            # the loss by less than the loss's last bit and only the second form can see it
            if np.isfinite(ft[c]) and (ft[c] <= f[c] + ARMIJO_C1 * t[c] * gd[c] or slope[c] <= ARMIJO_C1 * gd[c]):
                accept[c] = True
            else:
                t[c], halvings[c] = 0.5 * t[c], halvings[c] + 1
                if halvings[c] > MAX_HALVINGS:
                    status[c] = 3
        if accept.any():
            advance(accept * 2)
            f[accept] = ft[accept]
            iters[accept] += 1
            new_direction(accept, False)
    theta[torch.as_tensor(dead, device=dev)] = 0.0
    f[dead], gmax[dead] = 0.0, 0.0
    return {"theta": theta, "status": status.tolist(), "iterations": iters.tolist(), "passes": passes, "loss": f.tolist(),
            "gmax": gmax.tolist(), "count": cnt.tolist()}


def _finish(res, mean, rstd):
    theta = res["theta"]
    th = theta.cpu().numpy().astype(np.float64)
    if mean is None:
        W, b = th[:, :-1], th[:, -1]
    else:
        W, b = fold_back(th, mean.cpu().numpy(), rstd.cpu().numpy())
    res["W"] = torch.as_tensor(W.astype(np.float32), device=theta.device)
    res["b"] = torch.as_tensor(b.astype(np.float32), device=theta.device)
    res["mean"], res["rstd"] = mean, rstd
    return res


def _labels(labels, M, device):
    Y = torch.as_tensor(labels)
    if Y.dim() != 2 or Y.shape[0] != M:
        raise ValueError("the labels are (M, n) for a bank of %d rows (got %s)" % (M, tuple(Y.shape)))
    return Y.to(device=device, dtype=torch.float32).contiguous()


def _check_l2(l2):
    l2 = float(l2)
    if not (l2 >= 0 and np.isfinite(l2)):
        raise ValueError("l2 must be finite and >= 0 (got %r)" % (l2,))
    return l2


def fit(feats, labels, l2=1e-3, pos_weight=None, standardize=True, g_tol=1e-5, max_iter=200, history=10, theta0=None, splits=0):
    """The probe's fit on the bank feats (M, d) with labels (M, n): a dict with W (n, d) and b (n,) in raw-feature coordinates, theta
    (n, d + 1) in the fitted (standardised) coordinates, mean and rstd (None without standardisation), and per class status,
    iterations, loss, gmax (|g|_inf at the result) and count (live rows, sum y, sum (1 - y)); passes = the passes over the bank.
    theta0: a warm start in the fitted coordinates."""
    l2 = _check_l2(l2)
    X, mean, rstd = _prepare(feats, standardize)
    Y = _labels(labels, X.shape[0], X.device)
    return _finish(_solve(X, Y, l2, pos_weight, g_tol, max_iter, history, theta0, splits), mean, rstd)


def fit_path(feats, labels, l2s, pos_weight=None, standardize=True, g_tol=1e-5, max_iter=200, history=10, splits=0):
    """One fit per value of l2s, in the order given; they are solved in descending order of l2, each warm-started from the one
    before, over one standardised copy of the bank."""
    l2s = [_check_l2(v) for v in l2s]
    X, mean, rstd = _prepare(feats, standardize)
    Y = _labels(labels, X.shape[0], X.device)
    out, theta0 = {}, None
    for i in sorted(range(len(l2s)), key=lambda i: -l2s[i]):
        res = _finish(_solve(X, Y, l2s[i], pos_weight, g_tol, max_iter, history, theta0, splits), mean, rstd)
        out[i], theta0 = res, res["theta"]
    return [out[i] for i in range(len(l2s))]


def predict_logits(feats, fit):
    """(rows, n) fp32: the probe's logits of the features, standardised with the bank's statistics (ops.probe_logits)."""
    X = feats.to(torch.float32).contiguous()
    theta = fit["theta"]
    if fit.get("mean") is not None and X.shape[0]:
        X = ops.probe_standardize(X, fit["mean"], fit["rstd"], torch.empty_like(X))
    return ops.probe_logits(X, theta, torch.empty(X.shape[0], theta.shape[0], dtype=torch.float32, device=X.device))


def load_into(model, fit):
    """Writes the fit's W, b into the model's classifier (the nn.Linear cli.classifier_keys names) through load_state_dict.  A
    classifier of another width -- the projection of a contrastive checkpoint -- is replaced by one of n outputs first (FusedNet.resize_classifier,
    which refuses a model whose parameters a fused optimiser already holds).  Returns the model."""
    from .cli import classifier_keys
    W, b = fit["W"], fit["b"]
    wk, bk = classifier_keys(model)
    lin = model.get_submodule(wk[:-len(".weight")])
    if lin.in_features != W.shape[1]:
        raise ValueError("the fit has %d features, the classifier reads %d" % (W.shape[1], lin.in_features))
    model.resize_classifier(W.shape[0])
    sd = model.state_dict()
    sd[wk], sd[bk] = W.to(sd[wk].dtype), b.to(sd[bk].dtype)
    model.load_state_dict(sd)
    return model


def probe_auc(logits, targets):
    """{class: AUROC} of the probe's logits over the rows whose target is confident (0 or 1)."""
    from .knn import knn_auc
    return knn_auc(logits, torch.ones_like(logits), targets)


@torch.no_grad()
def probe(model, train_ds, valid_ds, l2s, n_bank, batch_size, device, pre=None, max_iter=200, embedded=None):
    """The linear probe of `model`: {"bank", "l2": [...], "fits": [{"l2", "aucs", "mean_auc", "status", "iterations", "passes",
    "train_loss"} ...]} and, under "_fits", the fits themselves (not for a report).  embedded: (bank, labels, queries, targets) where
    the caller has embedded the two sets already (the kNN probe of the same evaluation)."""
    from . import knn
    idx = knn.bank_indices(len(train_ds), n_bank)
    if embedded is None:
        bank, labels = knn.embed_dataset(model, train_ds, idx, batch_size, device, pre)
        q, targets = knn.embed_dataset(model, valid_ds, range(len(valid_ds)), batch_size, device, pre)
    else:
        bank, labels, q, targets = embedded
    fits = fit_path(bank, labels, l2s, max_iter=max_iter)
    out = {"bank": len(idx), "l2": [float(v) for v in l2s], "fits": [], "_fits": fits}
    for l2, res in zip(l2s, fits):
        aucs = probe_auc(predict_logits(q, res), targets)
        out["fits"].append({"l2": float(l2), "aucs": aucs, "mean_auc": knn.mean_auc(aucs), "status": res["status"],
                            "iterations": res["iterations"], "passes": res["passes"], "train_loss": res["loss"]})
    return out
