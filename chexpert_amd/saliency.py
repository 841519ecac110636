"""Pixel attribution maps of the fused networks at input resolution, class-specific: the plain input gradient, SmoothGrad (Smilkov et
al. 2017; with `squared`, SmoothGrad^2 of Hooker et al. 2019) and integrated gradients (Sundararajan et al. 2017), next to the
class-independent `grad_cam` and the 10 x 10 `class_cam` of gradcam.py.

The expensive part is the eval-mode forward + backward with dx (DESIGN.md sections 4.23 and 4.24): BatchNorm is frozen at its running
statistics, so the rows of a batch do not influence each other, and all path points or noise samples of an image ride in one batch.
Around it sit three HIP kernels (csrc/saliency.hip):

    cx_sal_points      builds the rows the network is evaluated at: base + alpha * (x - base) [+ sigma * n]
    cx_sal_accumulate  folds the dx of a pass into one sum per image: acc (+)= w * dx (or w * dx^2)
    cx_sal_finish      acc [* (x - base)], reduced over the three channels, and its sum (the completeness identity)

A pass is `eng.forward(points, False, record=True)` then `eng.backward(ws, dl, dx=buf)` with dl one-hot in the class column, inside
`params_untouched`, over at most `chunk` rows; there is one forward per backward and per class (the engines' backward consumes the
workspace).  The `*_reference` functions are the numpy statements the kernels are held to (bit for bit, the noise term to a few ulp),
and `integrated_gradients_reference` / `smoothgrad_reference` compose them around any differentiable torch callable.
"""
import math

import numpy as np
import torch

from . import ops
from .vis import MEAN, STD

RULES = ("midpoint", "trapezoid")
CHANNELS = tuple(ops.SAL_MODES)
CHUNK_PIXELS = 32 * 320 * 320          # default rows per pass: as many as hold this many pixels (32 rows at 320 x 320)
_M64 = (1 << 64) - 1


# ------------------------------------------------------------------------------------------------ numpy statements of the kernels
def _splitmix64(seed, k):
    """metrics.splitmix64 on a uint64 array k (arithmetic mod 2^64)."""
    with np.errstate(over="ignore"):
        z = np.uint64(int(seed) & _M64) + np.uint64(0x9E3779B97F4A7C15) * (k + np.uint64(1))
        z = (z ^ (z >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)
        z = (z ^ (z >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)
        return z ^ (z >> np.uint64(31))


def normal_reference(seed, rows, row_elems, first_row=0):
    """The noise of cx_sal_points: (rows, row_elems) fp32, element [r, e] = n(seed, (first_row + r) * row_elems + e), one standard normal
    per hash z = splitmix64(seed, k): u1 = ((z >> 40) + 1) / 2^24 in (0, 1], u2 = ((z >> 8) & 0xFFFFFF) / 2^24,
    n = sqrt(-2 ln u1) * cos(2 pi u2), here in float64 and rounded once.  |n| <= sqrt(48 ln 2) = 5.77; a row depends on
    (seed, first_row + r) only."""
    with np.errstate(over="ignore"):
        k = (np.uint64(int(first_row) & _M64) + np.arange(int(rows), dtype=np.uint64))[:, None] * np.uint64(int(row_elems)) \
            + np.arange(int(row_elems), dtype=np.uint64)[None, :]
    z = _splitmix64(seed, k)
    u1 = ((z >> np.uint64(40)) + np.uint64(1)).astype(np.float64) * 2.0 ** -24
    u2 = ((z >> np.uint64(8)) & np.uint64(0xFFFFFF)).astype(np.float64) * 2.0 ** -24
    return (np.sqrt(-2.0 * np.log(u1)) * np.cos(2.0 * np.pi * u2)).astype(np.float32)


def _np_base(base, x):
    """The baseline as an array that broadcasts against x (B,3,H,W): a full array, or three per-channel constants."""
    base = np.asarray(base, dtype=x.dtype)
    return base if base.shape == x.shape else base.reshape(1, 3, 1, 1)


def points_reference(x, base, img, alpha, sigma=None, seed=0, first_row=0):
    """Statement of cx_sal_points in x's dtype (fp32: the kernel's bits): out[r] = base[b] + alpha[r] * (x[b] - base[b]), b = img[r],
    plus sigma[b] * n(seed, first_row + r, .) when sigma (B,) is given -- every product and every sum rounded on its own."""
    x = np.asarray(x)
    dt = x.dtype.type
    img = np.asarray(img, dtype=np.int64)
    bb = np.broadcast_to(_np_base(base, x), x.shape)[img]
    d = x[img] - bb
    out = bb + np.asarray(alpha, dtype=dt).reshape(-1, 1, 1, 1) * d
    if sigma is not None:
        n = normal_reference(seed, len(img), x[0].size, first_row).reshape(out.shape).astype(dt)
        out = out + np.asarray(sigma, dtype=dt)[img].reshape(-1, 1, 1, 1) * n
    return out


def accumulate_reference(g, slot, w, planes, square=False, acc=None):
    """Statement of cx_sal_accumulate: acc (planes,3,H,W) starts at `acc` (or 0); for r ascending, acc[slot[r]] += w[r] * (g[r]^2 if
    square else g[r]), each product and sum rounded in g's dtype."""
    g = np.asarray(g)
    dt = g.dtype.type
    out = np.zeros((int(planes),) + g.shape[1:], dtype=g.dtype) if acc is None else np.array(acc, dtype=g.dtype)
    for r in range(len(g)):
        if 0 <= int(slot[r]) < planes:
            t = g[r] * g[r] if square else g[r]
            out[int(slot[r])] = out[int(slot[r])] + dt(w[r]) * t
    return out


def finish_reference(acc, x=None, base=(0.0, 0.0, 0.0), img_of=None, times_input=False, channels="none"):
    """Statement of cx_sal_finish: a = acc * (x[img_of] - base[img_of]) with times_input, else acc; channels "none": a (P,3,H,W), "sum"
    (a0 + a1) + a2, "abs" (|a0| + |a1|) + |a2|, "max" the largest |a_c| (P,H,W).  Returns (map, total): total float64 (P,), the sum of
    a over each plane."""
    a = np.asarray(acc)
    if times_input:
        x = np.asarray(x, dtype=a.dtype)
        img_of = np.asarray(img_of, dtype=np.int64)
        a = a * (x[img_of] - np.broadcast_to(_np_base(base, x), x.shape)[img_of])
    total = a.astype(np.float64).sum(axis=(1, 2, 3))
    if channels == "none":
        return a, total
    if channels == "sum":
        return (a[:, 0] + a[:, 1]) + a[:, 2], total
    m = np.abs(a)
    if channels == "abs":
        return (m[:, 0] + m[:, 1]) + m[:, 2], total
    if channels == "max":
        return np.maximum(np.maximum(m[:, 0], m[:, 1]), m[:, 2]), total
    raise ValueError("channels is one of %s (got %r)" % (", ".join(CHANNELS), channels))


# ------------------------------------------------------------------------------------------------ arguments (host only, no launch)
def path_alphas(steps, rule="midpoint"):
    """(alphas, weights) of the Riemann sum of integrated gradients over the straight path, float64: midpoint -- `steps` points
    (s + 1/2) / steps with weights 1 / steps; trapezoid -- steps + 1 points s / steps with weights 1 / steps, halved at both ends.  The weights sum to 1 exactly."""
    if isinstance(steps, bool) or not isinstance(steps, (int, np.integer)) or steps < 1:
        raise ValueError("steps is an integer >= 1 (got %r)" % (steps,))
    m = int(steps)
    if rule == "midpoint":
        a, w = (np.arange(m, dtype=np.float64) + 0.5) / m, np.full(m, 1.0 / m)
    elif rule == "trapezoid":
        a, w = np.arange(m + 1, dtype=np.float64) / m, np.full(m + 1, 1.0 / m)
        w[0] = w[-1] = 0.5 / m
    else:
        raise ValueError("rule is one of %s (got %r)" % (", ".join(RULES), rule))
    # the middle weight absorbs the rounding of 1 / m (at most an ulp), so that the exact sum of the weights rounds to 1 (math.fsum)
    j = len(w) // 2
    w[j] = 1.0 - math.fsum(np.delete(w, j))
    return a, w


def _baseline(baseline, x):
    """None (0: the dataset mean grey in whitened units), "black", a float, three per-channel floats or a full (B,3,H,W) tensor ->
    three floats, or the tensor."""
    if baseline is None:
        return (0.0, 0.0, 0.0)
    if isinstance(baseline, str):
        if baseline != "black":
            raise ValueError("baseline is None, 'black', a float, three per-channel floats or a (B,3,H,W) tensor (got %r)" % baseline)
        return ((0.0 - MEAN) / STD,) * 3
    if isinstance(baseline, (int, float)) and not isinstance(baseline, bool):
        return (float(baseline),) * 3
    if isinstance(baseline, torch.Tensor) and baseline.dim() == 4:
        if tuple(baseline.shape) != tuple(x.shape):
            raise ValueError("a full baseline has the input's shape %s (got %s)" % (tuple(x.shape), tuple(baseline.shape)))
        return baseline
    vals = baseline.tolist() if isinstance(baseline, (torch.Tensor, np.ndarray)) else list(baseline)
    if len(vals) != 3 or not all(isinstance(v, (int, float)) for v in vals):
        raise ValueError("a per-channel baseline is three floats (got %r)" % (baseline,))
    return tuple(float(v) for v in vals)


def _classes(model, classes, x, who):
    """gradcam._cam_classes (None, a list, a (B,) tensor, "pred") under this module's name, plus the per-image length check."""
    from .gradcam import _cam_classes, cam_source
    try:
        kind, K, payload = _cam_classes(classes, cam_source(model)[1].out_features)
    except ValueError as e:
        raise ValueError(str(e).replace("class_cam", who)) from None
    if kind == "per_image" and payload.numel() != x.shape[0]:
        raise ValueError("%s: %d classes for %d images" % (who, payload.numel(), x.shape[0]))
    return kind, K, payload


def _check_common(x, channels, chunk, who):
    if channels not in CHANNELS:
        raise ValueError("%s: channels is one of %s (got %r)" % (who, ", ".join(CHANNELS), channels))
    if chunk is not None and (isinstance(chunk, bool) or not isinstance(chunk, (int, np.integer)) or chunk < 1):
        raise ValueError("%s: chunk is a number of rows >= 1 (got %r)" % (who, chunk))
    if x.dim() != 4 or x.shape[1] != 3 or not x.dtype.is_floating_point:
        raise ValueError("%s takes a (B,3,H,W) float input (got %s %s)" % (who, tuple(x.shape), x.dtype))


def _on_gpu(x, who):
    if not x.is_cuda:
        raise RuntimeError("%s runs on the GPU only" % who)
    return x.detach().float().contiguous()


# ------------------------------------------------------------------------------------------------ the passes
def _eval_logits(eng, rows):
    ws = eng.forward(rows, False)
    try:
        return ws.logits.clone()
    finally:
        eng.release(ws)


def _maps(eng, x, cls, cls_img, rows, base, *, sigma=None, seed=0, square=False, chunk=None, times_input=False, channels="none",
          total=False):
    """Runs the passes of every requested class.  rows = (img, alpha, w): host arrays of R entries, image-major; cls = (kind, K, payload)
    of _classes; cls_img: the (B,) int64 class of every image for the kinds with one class per image.  Returns (maps (B,K,...),
    totals float64 (B,K) or None)."""
    from .models._fused import params_untouched
    kind, K, payload = cls
    B, _, H, W = x.shape
    dev = x.device
    R = len(rows[0])
    n_max = min(R, int(chunk) if chunk is not None else max(1, CHUNK_PIXELS // (H * W)))
    img = torch.from_numpy(np.asarray(rows[0], dtype=np.int32)).to(dev)
    alpha = torch.from_numpy(np.asarray(rows[1], dtype=np.float32)).to(dev)
    w = torch.from_numpy(np.asarray(rows[2], dtype=np.float32)).to(dev)
    img_of = torch.arange(B, dtype=torch.int32, device=dev)
    pts = torch.empty(n_max, 3, H, W, dtype=torch.float32, device=dev)
    g = torch.empty_like(pts)
    acc = torch.empty(B, 3, H, W, dtype=torch.float32, device=dev)
    row_cls = cls_img[img.long()].view(-1, 1) if cls_img is not None else None
    outs, tots = [], []
    for k in range(K):
        for r0 in range(0, R, n_max):
            n = min(n_max, R - r0)
            ops.sal_points(x, base, img[r0:r0 + n], alpha[r0:r0 + n], pts[:n], sigma=sigma, seed=seed, first_row=r0)
            ws = eng.forward(pts[:n], False, record=True)
            try:
                dl = torch.zeros_like(ws.logits)
                if row_cls is not None:
                    dl.scatter_(1, row_cls[r0:r0 + n], 1.0)
                else:
                    dl[:, k if kind == "all" else payload[k]] = 1.0
                with params_untouched(eng.params, eng.flat_grad):
                    eng.backward(ws, dl, dx=g[:n])
            finally:
                eng.release(ws)
            ops.sal_accumulate(g[:n], img[r0:r0 + n], w[r0:r0 + n], acc, square=square, accumulate=r0 > 0)
        out, tot = ops.sal_finish(acc, x, base, img_of, times_input=times_input, channels=channels, total=total)
        outs.append(out)
        tots.append(tot)
    return torch.stack(outs, 1), (torch.stack(tots, 1) if total else None)


def _image_classes(kind, payload, logits, n_classes, dev):
    """The (B,) int64 class of every image for classes="pred" (argmax on the device, no host sync) or a (B,) tensor (clamped into
    range: indices that live on the device cannot be checked without a sync); None for the kinds that share the classes."""
    if kind == "pred":
        return logits.argmax(1)
    if kind == "per_image":
        return payload.to(device=dev, dtype=torch.int64).clamp(0, n_classes - 1)
    return None


class _Eval:
    """model.eval() for the duration of a call; `training` is put back (nothing else of the model moves: the passes go to the engine
    directly, so registered Grad-CAM hooks never fire and the running statistics are only read)."""

    def __init__(self, model):
        self.model = model

    def __enter__(self):
        self.was_training = self.model.training
        self.model.eval()
        return self.model._eng()

    def __exit__(self, *exc):
        self.model.train(self.was_training)


def _gradient_maps(model, x, cls, samples, sigma, seed, squared, channels, chunk):
    """The mean over `samples` rows per image of the (squared) gradient at x [+ sigma * n]; sigma: None or a (B,) tensor."""
    B = x.shape[0]
    rows = (np.repeat(np.arange(B), samples), np.ones(B * samples), np.full(B * samples, np.float32(1.0) / np.float32(samples)))
    with _Eval(model) as eng:
        logits = _eval_logits(eng, x) if cls[0] == "pred" else None
        cls_img = _image_classes(cls[0], cls[2], logits, model._n_classes(), x.device)
        return _maps(eng, x, cls, cls_img, rows, (0.0, 0.0, 0.0), sigma=sigma, seed=seed, square=squared, chunk=chunk,
                     channels=channels)[0]


@torch.no_grad()
def input_gradient(model, x, classes=None, *, channels="none"):
    """d logit_c / d x of the eval-mode network (frozen BatchNorm) for the requested classes: (B,K,3,H,W) fp32, bit-equal to the x.grad
    of `model(x.requires_grad_())[:, c].sum().backward()` on the same batch (channels other than "none" reduce it as `smoothgrad` does).  classes as for `class_cam`: None -- all; a list of ints;
    a (B,) integer tensor -- one class per image (K = 1); "pred" -- the per-image argmax.  GPU only; the model's state (training flag,
    running statistics, every parameter's .grad) is left as it was, and the call works under torch.no_grad()."""
    who = "input_gradient"
    cls = _classes(model, classes, x, who)
    _check_common(x, channels, None, who)
    return _gradient_maps(model, _on_gpu(x, who), cls, 1, None, 0, False, channels, None)


@torch.no_grad()
def smoothgrad(model, x, classes=None, *, samples=16, sigma=None, noise_level=0.15, seed=0, squared=False, channels="abs", chunk=None):
    """SmoothGrad: the mean over `samples` noisy copies x + sigma * n of d logit_c / d x, or of its square (squared: SmoothGrad^2).
    sigma is in whitened units, a float or a (B,) tensor; None: noise_level / vis.STD, that fraction of the full uint8 range (no
    per-image min / max reduction).  The noise of sample s of image b is n(seed, b * samples + s, .) of `normal_reference`, so the
    maps do not depend on `chunk`, the number of rows per pass (default: as many as hold 32 x 320 x 320 pixels).  channels: how the
    three input channels are reduced -- "none" (B,K,3,H,W), else (B,K,H,W): "sum", "abs" (sum of magnitudes), "max" (largest
    magnitude).  Contracts as for `input_gradient`."""
    who = "smoothgrad"
    cls = _classes(model, classes, x, who)
    _check_common(x, channels, chunk, who)
    if isinstance(samples, bool) or not isinstance(samples, (int, np.integer)) or samples < 1:
        raise ValueError("%s: samples is an integer >= 1 (got %r)" % (who, samples))
    B = x.shape[0]
    if sigma is None:
        if not float(noise_level) >= 0:
            raise ValueError("%s: noise_level is a fraction >= 0 of the uint8 range (got %r)" % (who, noise_level))
        sigma = float(noise_level) / STD
    if isinstance(sigma, torch.Tensor):
        if sigma.dim() != 1 or sigma.numel() != B or not sigma.dtype.is_floating_point:
            raise ValueError("%s: a tensor of sigmas is (B,) floats, one per image" % who)
        sig = sigma.detach().float()
    else:
        if not float(sigma) >= 0:
            raise ValueError("%s: sigma is >= 0 in whitened units (got %r)" % (who, sigma))
        sig = torch.full((B,), float(sigma), dtype=torch.float32)
    x = _on_gpu(x, who)
    return _gradient_maps(model, x, cls, int(samples), sig.to(x.device).contiguous(), int(seed), bool(squared), channels, chunk)


@torch.no_grad()
def integrated_gradients(model, x, classes=None, *, steps=32, rule="midpoint", baseline=None, channels="sum", chunk=None):
    """Integrated gradients along the straight path from the baseline to x: attr = (x - base) * sum_s w_s * d logit_c / d x at
    base + alpha_s * (x - base), with (alpha, w) = path_alphas(steps, rule).  baseline: None -- 0 in whitened units, the dataset mean
    grey; "black" -- (0 - MEAN) / STD; a float; three per-channel floats; a full (B,3,H,W) tensor.  All path points of an image ride in
    one batch, at most `chunk` rows per pass (default: as many as hold 32 x 320 x 320 pixels).

    Returns (attr, logits, delta).  attr: (B,K,H,W) fp32 -- channels "sum" (signed; its pixel sum is the left side of the completeness
    identity), "abs" or "max" -- or (B,K,3,H,W) for "none".  logits (B,n): those of x, bit-equal to the plain eval forward (x and the
    baseline cost one extra eval forward of B rows each).  delta (B,K) float64 = sum(attr) - (logit_k(x) - logit_k(baseline)), the
    completeness gap of the Riemann sum (the sum taken in double over the unreduced attribution).  classes and contracts as for
    `input_gradient`."""
    who = "integrated_gradients"
    cls = _classes(model, classes, x, who)
    _check_common(x, channels, chunk, who)
    alphas, weights = path_alphas(steps, rule)
    base = _baseline(baseline, x)
    x = _on_gpu(x, who)
    B, S = x.shape[0], len(alphas)
    if isinstance(base, torch.Tensor):
        base = base.detach().to(device=x.device, dtype=torch.float32).contiguous()
    rows = (np.repeat(np.arange(B), S), np.tile(alphas, B), np.tile(weights, B))
    with _Eval(model) as eng:
        n_classes = model._n_classes()
        dev = x.device
        # the two ends of the path, as two forwards of B rows: the logits of x are then those of the plain eval forward bit for bit (one
        # forward of 2 B rows would save a launch sequence, but an engine may order its sums by the batch size: the fp32-storage
        # EfficientNet does)
        idx = torch.arange(B, dtype=torch.int32, device=dev)
        logits = _eval_logits(eng, x)
        at_base = _eval_logits(eng, ops.sal_points(x, base, idx, torch.zeros(B, device=dev)))      # base + 0 * (x - base)
        cls_img = _image_classes(cls[0], cls[2], logits, n_classes, dev)
        attr, total = _maps(eng, x, cls, cls_img, rows, base, chunk=chunk, times_input=True, channels=channels, total=True)
        diff = logits.double() - at_base.double()
        if cls_img is not None:
            diff = diff.gather(1, cls_img.view(-1, 1))
        elif cls[0] == "list":
            diff = diff[:, cls[2]]
    return attr, logits, total - diff


# ------------------------------------------------------------------------------------------------ the same around any torch callable
def _ref_classes(classes, n):
    if classes is None:
        return list(range(n))
    classes = [int(c) for c in classes]
    if not classes or not all(0 <= c < n for c in classes):
        raise ValueError("class indices lie in [0, %d) (got %s)" % (n, classes))
    return classes


def _ref_grads(f, pts, classes):
    """d f(pts)[:, c].sum() / d pts for every class c (one forward; f treats its rows independently, as an eval-mode network does)."""
    p = torch.from_numpy(np.ascontiguousarray(pts)).requires_grad_(True)
    with torch.enable_grad():
        out = f(p)
        classes = _ref_classes(classes, out.shape[1])
        return [torch.autograd.grad(out[:, c].sum(), p, retain_graph=True)[0].numpy() for c in classes], classes


def integrated_gradients_reference(f, x, classes=None, *, steps=32, rule="midpoint", baseline=None, channels="sum"):
    """`integrated_gradients` around any differentiable torch callable f: (R,3,H,W) -> (R,n) that treats its rows independently, on
    the CPU in x's dtype: the path points of points_reference, torch autograd for the gradients, the weighted sum and the product
    with x - base in float64.  Returns numpy (attr float64, logits, delta float64), shaped as `integrated_gradients` shapes them."""
    if channels not in CHANNELS:
        raise ValueError("channels is one of %s (got %r)" % (", ".join(CHANNELS), channels))
    xt = torch.as_tensor(x).detach().cpu()
    xn = xt.numpy()
    alphas, weights = path_alphas(steps, rule)
    base = _baseline(baseline, xt)
    base = base.detach().cpu().numpy().astype(xn.dtype) if isinstance(base, torch.Tensor) else np.asarray(base, dtype=xn.dtype)
    B, S = len(xn), len(alphas)
    img = np.repeat(np.arange(B), S)
    grads, classes = _ref_grads(f, points_reference(xn, base, img, np.tile(alphas, B)), classes)
    ends = points_reference(xn, base, np.tile(np.arange(B), 2), np.repeat([1.0, 0.0], B))
    with torch.no_grad():
        both = f(torch.from_numpy(np.ascontiguousarray(ends))).numpy()
    logits, at_base = both[:B], both[B:]
    d = (xn - np.broadcast_to(_np_base(base, xn), xn.shape)).astype(np.float64)
    attr, delta = [], []
    for c, g in zip(classes, grads):
        acc = (g.astype(np.float64).reshape(B, S, *xn.shape[1:]) * weights.reshape(1, S, 1, 1, 1)).sum(1)
        m, tot = finish_reference(acc * d, channels=channels)
        attr.append(m)
        delta.append(tot - (logits[:, c].astype(np.float64) - at_base[:, c].astype(np.float64)))
    return np.stack(attr, 1), logits, np.stack(delta, 1)


def smoothgrad_reference(f, x, classes=None, *, samples=16, sigma=None, noise_level=0.15, seed=0, squared=False, channels="abs"):
    """`smoothgrad` around any differentiable torch callable (see integrated_gradients_reference): the noisy rows of points_reference,
    torch autograd, then accumulate_reference and finish_reference in x's dtype.  Returns the numpy maps."""
    xt = torch.as_tensor(x).detach().cpu()
    xn = xt.numpy()
    B, S = len(xn), int(samples)
    if sigma is None:
        sigma = float(noise_level) / STD
    sig = np.broadcast_to(np.asarray(sigma.detach().cpu() if isinstance(sigma, torch.Tensor) else sigma, dtype=xn.dtype), (B,))
    img = np.repeat(np.arange(B), S)
    grads, _ = _ref_grads(f, points_reference(xn, (0.0, 0.0, 0.0), img, np.ones(B * S), sig, seed), classes)
    w = np.full(B * S, np.float32(1.0) / np.float32(S))
    return np.stack([finish_reference(accumulate_reference(g, img, w, B, square=squared), channels=channels)[0] for g in grads], 1)
