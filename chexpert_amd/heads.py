"""Heads of the fused networks, chosen by `FusedNet.set_head`: "linear" (activation, global pool, classifier: what the networks always
had), "csra", class-specific residual attention (Zhu & Wu, "Residual Attention: A Simple but Effective Method for Multi-Label
Recognition", ICCV 2021), which applies the classifier at every pixel and then pools the score map per class, and "pcam",
probabilistic-CAM pooling (Ye et al., "Weakly Supervised Lesion Localization With Probabilistic-CAM Pooling", 2020), which pools the
same score map with the per-pixel probabilities as weights.

This module states the kernels of csrc/csra_head.hip in numpy float64 (the definition also stands in include/chexpert_hip.h), the way
pooling.py states those of pool_head.hip.  For image b, with a[b,p,c] = act(x[b,p,c] sc[c] + sh[c]) m[b,c] over the HW pixels p (act: ReLU
or Swish; m: the optional per-(image, channel) multiplier, the EfficientNet head's Dropout mask, absent = 1), W (n, C), b (n,),
lambda >= 0 and T > 0:

  s[b,k,p]   = sum_c W[k,c] a[b,p,c]                    (no bias: the softmax does not see it)
  w[b,k,p]   = softmax over p of T s[b,k,p]             (relative to max_p s: a score of 1e4 stays finite)
  att[b,k]   = sum_p w[b,k,p] s[b,k,p]
  logit[b,k] = b[k] + mean_p s[b,k,p] + lambda att[b,k]

  ds[b,k,p]  = dlogit[b,k] (1/HW + lambda w[b,k,p] (1 + T (s[b,k,p] - att[b,k])))
  da[b,p,c]  = m[b,c] sum_k ds[b,k,p] W[k,c],   dz = da act'(z),   g = e_scale dz,   S1 = sum dz,   S2 = sum dz (x - mean) rstd
  dW[k,c]   += sum_{b,p} ds[b,k,p] a[b,p,c],    db[k] += sum_b dlogit[b,k]

Against the paper's code: the scores are not divided by |W_k| and the bias is kept, so lambda = 0 is exactly the linear head with the
average pool (the same nn.Linear, the same state_dict keys); one head only (no sum over several T); no T = infinity (max) branch.

The pcam head, on the same a, W, b and m, with sigma the logistic function:

  s[b,k,p]   = sum_c W[k,c] a[b,p,c]                         (csra's score map: same kernel, same bits)
  u[b,k,p]   = s[b,k,p] + b[k]                               (b absent = 0)
  w[b,k,p]   = sigma(u[b,k,p]) / sum_q sigma(u[b,k,q])       evaluated as softmax over p of log sigma(u), relative to its maximum
  logit[b,k] = sum_p w[b,k,p] u[b,k,p]                       (= b[k] + sum_p w s, since sum_p w = 1)
  P[b,k,p]   = sigma(u[b,k,p])                               the probability map

  q[b,k,p]   = sigma(-u[b,k,p])                              (1 - sigma(u), formed without cancellation)
  ds[b,k,p]  = dlogit[b,k] w[b,k,p] (1 + q[b,k,p] (u[b,k,p] - logit[b,k]))
  r[b,k]     = sum_p w[b,k,p] q[b,k,p] (u[b,k,p] - logit[b,k])
  db[k]     += sum_b dlogit[b,k] (1 + r[b,k])                (the bias is inside sigma, so db is NOT csra's sum_b dlogit)
  da, dz, g = e_scale dz, S1, S2, dW: csra's lines with this ds

Against the paper's code: one nn.Linear, the network's classifier under its state_dict keys, is shared by all classes' maps; the
gradient flows through the weights w (nothing is detached); no hyper-parameter.  HW = 1 gives logit = b + s; equal scores at every
pixel give logit = u; W = 0 gives logit = b and w = 1/HW; b -> +infinity tends to the linear head with the average pool."""
import numpy as np

from .pooling import activation

KINDS = ("linear", "csra", "pcam")
DEFAULT_LAMBDA, DEFAULT_T = 0.1, 1.0
MAX_CLASSES = 64


def check_head(kind="linear", lam=DEFAULT_LAMBDA, T=DEFAULT_T):
    """Validates the operands of set_head; returns (kind, lam, T) as (str, float, float).  ValueError otherwise.  lam and T belong to
    "csra"; the other kinds validate them and do not use them."""
    if kind not in KINDS:
        raise ValueError("head kind must be one of %s (got %r)" % (", ".join(KINDS), kind))
    try:
        lam, T = float(lam), float(T)
    except (TypeError, ValueError):
        raise ValueError("head lam and T must be numbers (got lam=%r, T=%r)" % (lam, T))
    if not (np.isfinite(lam) and lam >= 0.0):
        raise ValueError("head lam must be finite and >= 0 (got %r)" % (lam,))
    if not (np.isfinite(T) and T > 0.0):
        raise ValueError("head T must be finite and > 0 (got %r)" % (T,))
    return kind, lam, T


def _operands(x, sc, sh, act, m):
    x = np.asarray(x, dtype=np.float64)
    if x.ndim != 3:
        raise ValueError("x is (B, HW, C)")
    z = x * np.asarray(sc, dtype=np.float64) + np.asarray(sh, dtype=np.float64)
    a, da = activation(z, act)
    mm = np.ones((x.shape[0], x.shape[2])) if m is None else np.asarray(m, dtype=np.float64)
    return x, a * mm[:, None, :], da, mm


def csra_reference(x, sc, sh, W, b, lam, T, act="relu", m=None):
    """x (B, HW, C), sc / sh (C,), W (n, C), b (n,) or None, m (B, C) or None -> (logits (B, n), s (B, n, HW), w (B, n, HW), att (B, n)),
    float64."""
    _, a, _, _ = _operands(x, sc, sh, act, m)
    W = np.asarray(W, dtype=np.float64)
    s = np.einsum("kc,bpc->bkp", W, a)
    e = np.exp(T * (s - s.max(2, keepdims=True)))
    w = e / e.sum(2, keepdims=True)
    att = (w * s).sum(2)
    logits = s.mean(2) + lam * att
    if b is not None:
        logits = logits + np.asarray(b, dtype=np.float64)
    return logits, s, w, att


def csra_backward_reference(dlogits, x, sc, sh, mean, rstd, e_scale, W, lam, T, act="relu", m=None):
    """The backward kernel's outputs in float64: g (B, HW, C) = e_scale dz, S1 (C,) = sum dz, S2 (C,) = sum dz (x - mean) rstd, and what
    it adds to the classifier's gradients: dW (n, C), db (n,)."""
    xx, a, dact, mm = _operands(x, sc, sh, act, m)
    W = np.asarray(W, dtype=np.float64)
    dl = np.asarray(dlogits, dtype=np.float64)
    _, s, w, att = csra_reference(x, sc, sh, W, None, lam, T, act, m)
    HW = xx.shape[1]
    ds = dl[:, :, None] * (1.0 / HW + lam * w * (1.0 + T * (s - att[:, :, None])))
    da = np.einsum("bkp,kc->bpc", ds, W) * mm[:, None, :]
    dz = da * dact
    t2 = dz * (xx - np.asarray(mean, dtype=np.float64)) * np.asarray(rstd, dtype=np.float64)
    dW = np.einsum("bkp,bpc->kc", ds, a)
    return dz * np.asarray(e_scale, dtype=np.float64), dz.sum((0, 1)), t2.sum((0, 1)), dW, dl.sum(0)


def _log_sigmoid(u):
    return -np.logaddexp(0.0, -u)


def pcam_reference(x, sc, sh, W, b, act="relu", m=None):
    """x (B, HW, C), sc / sh (C,), W (n, C), b (n,) or None, m (B, C) or None -> (logits (B, n), s (B, n, HW), w (B, n, HW),
    P (B, n, HW)), float64."""
    _, a, _, _ = _operands(x, sc, sh, act, m)
    s = np.einsum("kc,bpc->bkp", np.asarray(W, dtype=np.float64), a)
    u = s if b is None else s + np.asarray(b, dtype=np.float64)[None, :, None]
    L = _log_sigmoid(u)
    e = np.exp(L - L.max(2, keepdims=True))
    w = e / e.sum(2, keepdims=True)
    return (w * u).sum(2), s, w, np.exp(L)


def pcam_backward_reference(dlogits, x, sc, sh, mean, rstd, e_scale, W, b, act="relu", m=None):
    """The backward kernel's outputs in float64: g (B, HW, C) = e_scale dz, S1 (C,) = sum dz, S2 (C,) = sum dz (x - mean) rstd, and what
    it adds to the classifier's gradients: dW (n, C), db (n,)."""
    xx, a, dact, mm = _operands(x, sc, sh, act, m)
    W = np.asarray(W, dtype=np.float64)
    dl = np.asarray(dlogits, dtype=np.float64)
    logits, s, w, _ = pcam_reference(x, sc, sh, W, b, act, m)
    u = s if b is None else s + np.asarray(b, dtype=np.float64)[None, :, None]
    t = np.exp(_log_sigmoid(-u)) * (u - logits[:, :, None])            # q (u - logit)
    ds = dl[:, :, None] * w * (1.0 + t)
    r = (w * t).sum(2)
    da = np.einsum("bkp,kc->bpc", ds, W) * mm[:, None, :]
    dz = da * dact
    t2 = dz * (xx - np.asarray(mean, dtype=np.float64)) * np.asarray(rstd, dtype=np.float64)
    dW = np.einsum("bkp,bpc->kc", ds, a)
    return dz * np.asarray(e_scale, dtype=np.float64), dz.sum((0, 1)), t2.sum((0, 1)), dW, (dl * (1.0 + r)).sum(0)


def _csra_maps(model, s, st):
    """(scores, attention) of the csra head from the forward's score map s (B, n, HW) and its stat rows."""
    import torch
    s = s.clone()
    return s, torch.exp(model.head_attn[1] * (s - st[:, :, 0:1])) * st[:, :, 1:2]


def _pcam_maps(model, s, st):
    """(P, w) of the pcam head from the forward's score map s (B, n, HW) and its stat rows."""
    import torch
    u = s + st[:, :, 3:4]                                              # the kernel's u = s + bias, the same rounding
    wgt = torch.exp(torch.nn.functional.logsigmoid(u) - torch.nn.functional.logsigmoid(st[:, :, 0:1])) * st[:, :, 1:2]
    return torch.sigmoid(u), wgt


def class_maps(model, x):
    """One eval-mode forward of a model with the csra head (set_head("csra")): (scores (B, n, h, w), attention (B, n, h, w), logits (B, n)),
    fp32 tensors on x's device.  scores is the classifier applied at every pixel of the last feature map (without the bias), attention
    its softmax over the pixels at temperature T, which sums to 1 over the pixels of every (image, class); logits equal model(x).
    With the pcam head (set_head("pcam")): (P (B, n, h, w), w (B, n, h, w), logits (B, n)), P = sigmoid(s + bias) the per-class
    probability map in [0, 1] and w = P / sum_p P the pooling weights, which sum to 1 over the pixels; logits equal model(x).
    Under set_loss(kind="hier") the logits are CONDITIONAL ones -- P(finding | its parent is positive) -- and the maps are taken on them
    as they are: a map shows the evidence for a finding given its parent, not for the unconditional probability
    (loss.collapse_hierarchy gives that number, and it has no single map)."""
    import torch
    if getattr(model, "head_kind", "linear") not in ("csra", "pcam"):
        raise NotImplementedError("class_maps reads the score map of the csra or pcam head: this model has set_head(%r)"
                                  % (getattr(model, "head_kind", "linear"),))
    if model.training:
        raise RuntimeError("class_maps runs in eval mode (model.eval())")
    if not x.is_cuda:
        raise RuntimeError("class_maps runs on the GPU only: move the model and the input to cuda")
    with torch.no_grad():
        eng = model._eng()
        ws = eng.forward(x, False)
        B, n = ws.logits.shape
        h, w = ws.head_hw
        a, b = (_pcam_maps if model.head_kind == "pcam" else _csra_maps)(model, ws.head_s, ws.head_stat)
        logits = ws.logits.clone()
        eng.release(ws)
    return a.view(B, n, h, w), b.view(B, n, h, w), logits
