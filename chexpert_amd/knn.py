"""The kNN probe of a frozen backbone and image retrieval on its pooled features.

The weighted k-nearest-neighbour probe of Wu et al., "Unsupervised Feature Learning via Non-Parametric Instance Discrimination" (CVPR
2018), the monitor SimCLR, MoCo, MoCo-CXR and DINO report next to their loss: embed a bank of labelled training images with the frozen
network (FusedNet.embed), embed the validation images, let each validation image's k nearest bank rows vote with weight exp(s / T), and
report the AUROC per finding.  No training; deterministic.  The search (ops.knn_topk) and the vote (ops.knn_vote) are HIP kernels
(csrc/knn.hip); `reference_topk` and `reference_vote` are their definitions in numpy float64, which the tests hold them to.

The order that defines "nearest": the larger similarity first, the lower bank index among equal similarities (a total order: the
result does not depend on how the kernel tiles or slices the bank); a NaN similarity counts as -inf.  A bank row whose group equals
the query's group (>= 0) is no candidate: the row's own position as the group is leave-one-out, the patient code is patient-disjoint
search.  A query with fewer than k candidates has idx -1 and sim -inf in the tail.
"""
import numpy as np
import torch

from . import ops

METRICS = ("cosine", "dot")


def _check_metric(metric):
    if metric not in METRICS:
        raise ValueError("metric must be one of %s (got %r)" % (", ".join(METRICS), metric))


def _groups(group, n, device, what):
    if group is None:
        return None
    g = torch.as_tensor(group).reshape(-1)
    if g.numel() != n:
        raise ValueError("%s has %d entries for %d rows" % (what, g.numel(), n))
    return g.to(device=device, dtype=torch.int32).contiguous()


def normalize(x):
    """x / max(|x|, 1e-12) per row (ops.knn_normalize), the normalisation of the contrastive loss."""
    x = x.to(torch.float32).contiguous()
    return ops.knn_normalize(x, torch.empty_like(x))


class KnnSearch:
    """knn_topk with its scratch held between calls (one allocation per shape)."""

    def __init__(self):
        self._scratch = None

    def __call__(self, q, bank, k, q_group=None, bank_group=None, metric="cosine", splits=0):
        _check_metric(metric)
        if q.dim() != 2 or bank.dim() != 2 or q.shape[1] != bank.shape[1]:
            raise ValueError("q is (Q, d) and bank (M, d) (got %s and %s)" % (tuple(q.shape), tuple(bank.shape)))
        if (q_group is None) != (bank_group is None):
            raise ValueError("q_group and bank_group are given together or not at all")
        (Q, d), M, k = q.shape, bank.shape[0], int(k)
        need = ops.knn_scratch(max(Q, 1), M, k, splits)                     # (checks M, k and splits)
        sim = torch.empty(Q, k, dtype=torch.float32, device=q.device)
        idx = torch.empty(Q, k, dtype=torch.int32, device=q.device)
        if Q == 0:
            return sim, idx
        q, bank = q.to(torch.float32).contiguous(), bank.to(torch.float32).contiguous()
        if metric == "cosine":
            q, bank = normalize(q), normalize(bank)
        if self._scratch is None or self._scratch.numel() < need or self._scratch.device != q.device:
            self._scratch = torch.empty(need, dtype=torch.float32, device=q.device)
        ops.knn_topk(q, bank, k, sim, idx, _groups(q_group, Q, q.device, "q_group"), _groups(bank_group, M, q.device, "bank_group"),
                     self._scratch, splits)
        return sim, idx


_search = KnnSearch()


def knn_topk(q, bank, k, q_group=None, bank_group=None, metric="cosine", splits=0):
    """(sim (Q, k) fp32, idx (Q, k) int32): each query's k nearest bank rows in the order of the module docstring.  metric "cosine"
    normalises both sides first, "dot" is the plain inner product.  splits: the slices the kernel cuts the bank into (0: its choice;
    the result is the same for every value).  The scratch is held by the module between calls."""
    return _search(q, bank, k, q_group, bank_group, metric, splits)


def knn_vote(sim, idx, labels, T=0.1):
    """(score (Q, n), support (Q, n)) of the weighted vote: w_j = exp((s_j - s_0) / T) over a query's valid neighbours, score = the
    weighted mean of their labels that are not ignored (< 0), support = the weight that voted; 0.5 / 0 where none did.  T = inf is
    the unweighted vote."""
    if not T > 0:
        raise ValueError("the vote's temperature must be > 0 (got %r)" % (T,))
    labels = labels.to(device=sim.device, dtype=torch.float32).contiguous()
    score = torch.empty(sim.shape[0], labels.shape[1], dtype=torch.float32, device=sim.device)
    support = torch.empty_like(score)
    ops.knn_vote(sim.contiguous(), idx.contiguous(), labels, score, support, 0.0 if np.isinf(T) else 1.0 / float(T))
    return score, support


def knn_predict(q, bank, labels, k=200, T=0.1, q_group=None, bank_group=None, metric="cosine", splits=0):
    """The probe's prediction for every query: knn_topk, then knn_vote over the bank's labels (M, n).  k is cut to the bank's size."""
    k = min(int(k), bank.shape[0])
    sim, idx = knn_topk(q, bank, k, q_group, bank_group, metric, splits)
    return knn_vote(sim, idx, labels, T)


def knn_auc(score, support, targets):
    """{class: AUROC} of the probe through metrics.roc_curve / auc, over the rows that had support and whose target is confident (0 or
    1); NaN for a class without such rows of both kinds."""
    from .metrics import auc, roc_curve
    score, support, targets = (np.asarray(torch.as_tensor(v).cpu(), dtype=np.float64) for v in (score, support, targets))
    out = {}
    for c in range(score.shape[1]):
        keep = (support[:, c] > 0) & ((targets[:, c] == 0) | (targets[:, c] == 1))
        if not keep.any():
            out[c] = float("nan")
            continue
        f, t, _ = roc_curve(targets[keep, c], score[keep, c])
        out[c] = auc(f, t)
    return out


def mean_auc(aucs):
    v = np.array(list(aucs.values()), dtype=np.float64)
    return float(np.nanmean(v)) if np.any(~np.isnan(v)) else float("nan")


@torch.no_grad()
def embed_dataset(model, ds, indices, batch_size, device, pre=None):
    """(features (N, C) fp32 on the device, targets (N, n)) of the images `indices` of `ds`, in that order, from model.embed in eval
    mode.  `pre`: the deterministic preprocessing of the uint8 batch on the GPU (--clahe), or None."""
    from .cli import batches
    was_training = model.training
    model.eval()
    feats, tgts = [], []
    try:
        for x, t, _ in batches(ds, list(indices), batch_size, False):
            x = x.to(device)
            feats.append(model.embed(x if pre is None else pre(x)))
            tgts.append(t)
    finally:
        model.train(was_training)
    if not feats:
        raise ValueError("embed_dataset: no images")
    return torch.cat(feats), torch.cat(tgts)


@torch.no_grad()
def retrieve(model, bank, x, k, metric="cosine"):
    """(idx (B, k), sim (B, k)): the bank rows most similar to each image of the uint8 or normalised batch x, by model.embed."""
    was_training = model.training
    model.eval()
    try:
        q = model.embed(x)
    finally:
        model.train(was_training)
    sim, idx = knn_topk(q, bank, k, metric=metric)
    return idx, sim


def bank_indices(n_train, n_bank):
    """The positions of the probe's bank in the training set: all of it for n_bank 0 (or >= its size), else n_bank images at an even
    stride, the same ones every time."""
    if n_bank <= 0 or n_bank >= n_train:
        return list(range(n_train))
    return [int(i * n_train // n_bank) for i in range(n_bank)]


@torch.no_grad()
def probe(model, train_ds, valid_ds, k, T, n_bank, batch_size, device, pre=None, embedded=None):
    """The kNN probe of `model`: {"k", "temperature", "bank", "aucs", "mean_auc"} (k is cut to the bank's size).  embedded: (bank,
    labels, queries, targets) where the caller has embedded the two sets already (the linear probe of the same evaluation)."""
    idx = bank_indices(len(train_ds), n_bank)
    if embedded is None:
        bank, labels = embed_dataset(model, train_ds, idx, batch_size, device, pre)
        q, targets = embed_dataset(model, valid_ds, range(len(valid_ds)), batch_size, device, pre)
    else:
        bank, labels, q, targets = embedded
    k = min(int(k), bank.shape[0])
    score, support = knn_predict(q, bank, labels, k, T)
    aucs = knn_auc(score, support, targets)
    return {"k": k, "temperature": float(T), "bank": len(idx), "aucs": aucs, "mean_auc": mean_auc(aucs)}


# ---- the definitions in numpy float64 ------------------------------------------------------------------------------------------------
def reference_topk(q, bank, k, q_group=None, bank_group=None):
    """(sim (Q, k) float64, idx (Q, k) int64, S (Q, M) float64, A (Q, M) float64): the k nearest rows of every query by the plain inner
    product in float64, in the order of the module docstring, written as a lexsort on (-similarity, index) over the candidates; idx -1
    and sim -inf in the tail of a query with fewer than k candidates.  S is the full similarity matrix and A = sum_k |q_k b_k|, the
    scale of an fp32 summation's error bound."""
    q, bank = np.asarray(q, dtype=np.float64), np.asarray(bank, dtype=np.float64)
    (Q, d), M = q.shape, bank.shape[0]
    if (q_group is None) != (bank_group is None):
        raise ValueError("q_group and bank_group are given together or not at all")
    S = q @ bank.T
    A = np.abs(q) @ np.abs(bank).T
    key = np.where(np.isnan(S), -np.inf, S) + 0.0                              # NaN counts as -inf; -0 is +0
    sim = np.full((Q, k), -np.inf)
    idx = np.full((Q, k), -1, dtype=np.int64)
    rows = np.arange(M)
    for i in range(Q):
        cand = rows
        if q_group is not None and q_group[i] >= 0:
            cand = rows[np.asarray(bank_group) != q_group[i]]
        order = cand[np.lexsort((cand, -key[i, cand]))][:k]                    # primary: -similarity, then the index
        sim[i, :len(order)] = key[i, order]
        idx[i, :len(order)] = order
    return sim, idx, S, A


def reference_vote(sim, idx, labels, inv_T):
    """(score (Q, n), support (Q, n)) in float64: over a query's valid neighbours j (idx >= 0) in list order, s_0 the first of them,
    w_j = exp((s_j - s_0) * inv_T) (1 where inv_T == 0 or s_j == s_0); num_c = sum_j w_j y[idx_j, c] and den_c = sum_j w_j over the
    neighbours whose label c is not ignored (< 0); score = num / den, support = den; den == 0: score 0.5, support 0."""
    sim, idx, labels = np.asarray(sim, dtype=np.float64), np.asarray(idx), np.asarray(labels, dtype=np.float64)
    Q, n = sim.shape[0], labels.shape[1]
    score, support = np.full((Q, n), 0.5), np.zeros((Q, n))
    for i in range(Q):
        valid = np.flatnonzero(idx[i] >= 0)
        if not len(valid):
            continue
        s, y = sim[i, valid], labels[idx[i, valid]]
        with np.errstate(invalid="ignore"):
            w = np.where((inv_T == 0) | (s == s[0]), 1.0, np.exp((s - s[0]) * inv_T))
        for c in range(n):
            use = y[:, c] >= 0
            den = w[use].sum()
            if den > 0:
                score[i, c], support[i, c] = (w[use] * y[use, c]).sum() / den, den
    return score, support
