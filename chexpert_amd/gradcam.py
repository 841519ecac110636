"""Grad-CAM for the fused models, computing what /root/reference/chexpert.py:260-303 computes.

As executed by the reference: the legacy backward hook on the classifier
returns the gradient w.r.t. W^T, so after `.mean(1)` the channel weights are
`w[f] = (1/n_cls) * sum_b pooled[b,f]` -- independent of `cls_idx` and shared by the minibatch -- and the
hooked feature map is post-ReLU.  No backward pass is therefore needed: one eval-mode forward through the
HIP engine yields the block-4 buffer, norm5 scale/shift and the pooled features; two small kernels produce
the normalised, bilinearly up-sampled maps.  `hooks` / `cls_idx` are accepted for signature compatibility.
"""
import torch

from . import ops


def _targets(model, eng, ws, dev):
    """(hooked module, final Linear, feature buffer, scale, shift, ReLU'd-in-place-after-the-hook?) of the reference's hook pairs."""
    if hasattr(model, "features"):                               # DenseNet: norm5 output, ReLU'd in place by the model (:514)
        return (model.features.norm5, model.classifier) + eng.norm5_operands(ws) + (True,)
    if hasattr(model, "_stages"):                                # ResNet / WideResNet: output of the last stage (already post-ReLU)
        return model._stages()[-1], model.fc, ws.blk[-1]["out"], None, None, False
    if hasattr(model, "head"):                                   # EfficientNet: head[1] BatchNorm output, before Swish
        S = eng.bn[id(model.head[1])]
        return model.head[1], model.head[-1], ws.yh, eng._v(ws, S.sc), eng._v(ws, S.sh), False
    raise RuntimeError("unknown model family")


def _require_avg(model, what):
    """NotImplementedError naming set_pool for a model that pools with anything but the average."""
    check = getattr(model, "require_avg_pool", None)
    if check is not None:
        check(what)


def hooks_registered(model):
    try:
        eng = model._eng()
    except NotImplementedError:
        return False
    mods = [model.features.norm5, model.classifier] if hasattr(model, "features") else \
        ([model._stages()[-1], model.fc] if hasattr(model, "_stages") else [model.head[1], model.head[-1]])
    return any(len(m._forward_hooks) or len(m._backward_hooks) for m in mods)


class _HookedLinear(torch.autograd.Function):
    """Gives the fused eval forward an autograd edge at the final Linear so that hooks registered on it fire the way the
    reference's grad_cam expects (chexpert.py:268-283): a legacy `register_backward_hook` on nn.Linear receives
    grad_input = (grad_bias, grad_x, grad_W^T)."""

    @staticmethod
    def forward(ctx, anchor, logits, pooled, linear):
        ctx.pooled, ctx.linear = pooled, linear
        return logits.clone()

    @staticmethod
    def backward(ctx, dlogits):
        lin, pooled = ctx.linear, ctx.pooled
        dl = dlogits.contiguous().float()
        dw = torch.zeros_like(lin.weight)
        db = torch.zeros(lin.out_features, device=dl.device)
        dp = torch.empty_like(pooled)
        ops.head_bwd(dl, pooled, lin.weight.detach(), dw, db, dp)
        for hook in list(lin._backward_hooks.values()):
            hook(lin, (db, dp, dw.t()), (dl,))
        return None, None, None, None


def hooked_eval_forward(model, x):
    """Eval forward through the HIP engine that honours `register_forward_hook` on the reference's Grad-CAM targets and
    `register_backward_hook` on the final Linear (chexpert.py:271-272 with the hook pairs of :468, :484, :498), so the
    reference's own `grad_cam(model, x, hooks)` works against the drop-in.  The hooks' arithmetic is that of the average pool: a model
    with another pooling (set_pool) is refused."""
    _require_avg(model, "the Grad-CAM hook path (hooked_eval_forward)")
    eng = model._eng()
    ws = eng.forward(x, False)
    try:
        hooked, lin, buf, sc, sh, relu_after = _targets(model, eng, ws, x.device)
        B, h, w, C = buf.shape
        feat = torch.empty(B, C, h, w, dtype=torch.float32, device=x.device)
        if buf.dtype != torch.bfloat16:
            raise NotImplementedError("hooks are served from the bf16 engine")
        ops.affine_to_f32_nchw(buf, sc, sh, False, feat)
        for hook in list(hooked._forward_hooks.values()):
            hook(hooked, (None,), feat)
        if relu_after:                       # F.relu(features, inplace=True) of the reference mutates the hooked tensor (:514)
            ops.affine_to_f32_nchw(buf, sc, sh, True, feat)
        logits, pooled = ws.logits.clone(), ws.pooled.clone()
    finally:
        eng.release(ws)
    out = _HookedLinear.apply(lin.weight, logits, pooled, lin) if torch.is_grad_enabled() else logits
    for hook in list(lin._forward_hooks.values()):
        hook(lin, (pooled,), out)
    return out


@torch.no_grad()
def grad_cam(model, x, hooks=None, cls_idx=None):
    """Hook targets of the reference: DenseNet `features.norm5` / `classifier` (chexpert.py:468), ResNet `layer4` / `fc`
    (:484, :490), EfficientNet `head[1]` / `head[-1]` (:498).  The map tensor and the pooled input of the final Linear both
    exist in the engine's workspace after one eval forward.  The channel weights here do not depend on the class (module
    docstring); for class-specific maps use `class_cam`.
    Under set_loss(kind="hier") the logits are CONDITIONAL ones -- P(finding | its parent is positive) -- and the maps are taken on them
    as they are: a map shows the evidence for a finding given its parent, not for the unconditional probability
    (loss.collapse_hierarchy gives that number, and it has no single map)."""
    if not x.is_cuda:
        raise RuntimeError("grad_cam runs on the GPU only")
    _require_avg(model, "grad_cam")
    was_training = model.training
    model.eval()
    eng = model._eng()
    ws = eng.forward(x, False)
    try:
        dev = x.device
        if hasattr(model, "features"):                               # DenseNet: relu(norm5(block-4 buffer))
            (buf, sc, sh), inner = eng.norm5_operands(ws), 1
        elif hasattr(model, "_stages"):                              # ResNet: output of the last stage (post-ReLU, no BN in between)
            buf = ws.blk[-1]["out"]
            C_ = buf.shape[3]
            sc, sh, inner = torch.ones(C_, device=dev), torch.zeros(C_, device=dev), 0
        elif hasattr(model, "head"):                                 # EfficientNet: head[1] BatchNorm output, before Swish
            buf = ws.yh
            S = eng.bn[id(model.head[1])]
            sc, sh, inner = eng._v(ws, S.sc), eng._v(ws, S.sh), 0
        else:
            raise RuntimeError("grad_cam: unknown model family")
        B, h, w, C = buf.shape
        n_cls = ws.logits.shape[1]
        wts = (ws.pooled.sum(0) / n_cls).contiguous()
        cam = torch.empty(B, h * w, dtype=torch.float32, device=dev)
        ops.gradcam_map(buf, sc, sh, wts, cam, inner)
        out = torch.empty(B, 1, x.shape[2], x.shape[3], dtype=torch.float32, device=dev)
        ops.cam_norm_upsample(cam, out, h, w)
    finally:
        eng.release(ws)
        model.train(was_training)
    return out


# ---- class-specific maps: Grad-CAM taken at the tensor the network pools globally ("Class maps")
def cam_source(model):
    """(activation code of ops.class_cam, final Linear) of the model's family: the last feature map A that the network averages
    over its pixels is relu(norm5(.)) for DenseNet, the last stage's output as it is for ResNet / WideResNet (already post-ReLU),
    and swish(head[1](.)) for EfficientNet."""
    if hasattr(model, "features"):
        return ops.CAM_ACT_RELU, model.classifier
    if hasattr(model, "_stages"):
        return ops.CAM_ACT_NONE, model.fc
    if hasattr(model, "head"):
        return ops.CAM_ACT_SWISH, model.head[-1]
    raise RuntimeError("class_cam: unknown model family")


def _cam_operands(model, eng, ws):
    """(feature buffer, scale, shift) of A = act(buffer * scale + shift) in the workspace of an eval forward."""
    if hasattr(model, "features"):
        return eng.norm5_operands(ws)
    if hasattr(model, "_stages"):
        return ws.blk[-1]["out"], None, None
    S = eng.bn[id(model.head[1])]
    return ws.yh, eng._v(ws, S.sc), eng._v(ws, S.sh)


def _cam_classes(classes, n_classes):
    """Validates `classes` on the host (no launch): (kind, K, payload)."""
    if classes is None:
        return "all", n_classes, None
    if isinstance(classes, str):
        if classes != "pred":
            raise ValueError("class_cam: classes is None, a list of class indices, a (B,) integer tensor or 'pred' (got %r)" % classes)
        return "pred", 1, None
    if isinstance(classes, torch.Tensor):
        if classes.dim() != 1 or classes.dtype.is_floating_point or classes.dtype == torch.bool:
            raise ValueError("class_cam: a tensor of classes is 1-D and integer, one class per image")
        if not classes.is_cuda and classes.numel() and (int(classes.min()) < 0 or int(classes.max()) >= n_classes):
            raise ValueError("class_cam: class indices must lie in [0, %d)" % n_classes)
        return "per_image", 1, classes
    lst = list(classes)
    if not lst:
        raise ValueError("class_cam: the class list is empty")
    if not all(isinstance(c, int) and not isinstance(c, bool) and 0 <= c < n_classes for c in lst):
        raise ValueError("class_cam: class indices must be ints in [0, %d) (got %s)" % (n_classes, lst))
    return "list", len(lst), lst


@torch.no_grad()
def class_cam(model, x, classes=None, *, relu=True, normalize=True, upsample=True):
    """Class-specific activation maps for all requested classes from ONE eval forward and one kernel launch that reads the final
    feature map once.  With A[b, f, p] the tensor the network pools globally (cam_source) and y = bias + W mean_p A its final Linear,

        M[b, c, p] = (1 / HW) * sum_f W[c, f] * A[b, f, p]

    is Grad-CAM taken at A: alpha[c, f] = mean_p dy_c / dA[f, p] = W[c, f] / HW exactly, so no backward pass is needed, the map is
    relu(M), and y[b, c] = bias[c] + sum_p M[b, c, p] (the CAM identity).  For EfficientNet A is deliberately the POST-Swish tensor
    swish(head[1](.)), not the pre-Swish output of head[1] that the reference's hook (and `grad_cam`) looks at: the post-Swish tensor
    is the last feature map the classifier sees, and only there are the weights exact and class-specific without a backward pass.

    classes: None -- all n_classes; a list / tuple of ints -- the same classes for every image; a 1-D integer tensor of length B --
    one class per image (K = 1); "pred" -- the per-image argmax of the logits, taken on the device without a host sync.  Lists and
    CPU tensors are range-checked (ValueError) before anything is launched; indices that live on the device cannot be checked without
    a sync and are clamped into [0, n_classes) by the kernel.

    Returns (maps, logits).  logits (B, n_classes) are those of this forward.  maps is (B, K, H_in, W_in) fp32 with normalize and
    upsample: every (b, k) map scaled by (t - min) / (max - min + 1e-5), then resized bilinearly with align_corners=True
    (ops.cam_norm_upsample on the (B*K, h*w) rows); normalize without upsample gives the scaled (B, K, h, w) maps; with neither,
    the raw M (relu=False) or relu(M).  relu=False with normalize scales the signed map the same way.  Both storage types, all three
    families; registered Grad-CAM hooks are ignored (the hooked path is never taken); model.training and the running statistics are
    left as they were.

    Under set_loss(kind="hier") logit c is a CONDITIONAL one -- P(finding c | its parent is positive) -- and M is taken on it as it is:
    the map shows the evidence for the finding given its parent, and the CAM identity above holds for that logit, not for the
    unconditional one of loss.collapse_hierarchy."""
    _require_avg(model, "class_cam")          # M is Grad-CAM only when the pool is the mean
    act, lin = cam_source(model)
    kind, K, payload = _cam_classes(classes, lin.out_features)
    if upsample and not normalize:
        raise ValueError("class_cam: upsample=True needs normalize=True (the resize kernel is the normalising one)")
    if not x.is_cuda:
        raise RuntimeError("class_cam runs on the GPU only")
    if kind == "per_image" and payload.numel() != x.shape[0]:
        raise ValueError("class_cam: %d classes for %d images" % (payload.numel(), x.shape[0]))
    was_training = model.training
    model.eval()
    eng = model._eng()
    ws = eng.forward(x, False)
    try:
        dev = x.device
        buf, sc, sh = _cam_operands(model, eng, ws)
        B, h, w, C = buf.shape
        logits = ws.logits.clone()
        W = lin.weight.detach()
        if W.dtype != torch.float32 or W.stride(1) != 1 or W.stride(0) % 4 or W.data_ptr() % 16:
            W = W.float().contiguous().clone()
        cls = payload
        if kind == "pred":
            cls = logits.argmax(1).to(torch.int32).view(B, 1)
        elif kind == "per_image":
            cls = payload.to(device=dev, dtype=torch.int32).contiguous().view(B, 1)
        cam = torch.empty(B, K, h * w, dtype=torch.float32, device=dev)
        ops.class_cam(buf, sc, sh, W, cam, act=act, relu=relu, cls=cls)
        if normalize:
            H_, W_ = (x.shape[2], x.shape[3]) if upsample else (h, w)
            out = torch.empty(B * K, 1, H_, W_, dtype=torch.float32, device=dev)
            ops.cam_norm_upsample(cam.view(B * K, h * w), out, h, w)
            out = out.view(B, K, H_, W_)
        else:
            out = cam.view(B, K, h, w)
    finally:
        eng.release(ws)
        model.train(was_training)
    return out, logits
