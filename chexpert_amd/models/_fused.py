"""What the fused networks (DenseNet, ResNet / WideResNet, EfficientNet) share: the nn.Module surface (FusedNet, with the one
autograd function), the host side of their engines (FusedEngine: flat parameter masters, weight packing, workspaces, the step
protocol of backward) and the coefficient-vector bookkeeping (_Vec, _BN)."""
import contextlib

import torch
import torch.nn as nn

from .. import ops
from .._lib import CxPackDesc
from ..loss import Loss


# --------------------------------------------------------------------------------------------- input gradient (x.grad)
def wants_autograd(model, x):
    """model.forward routes through the autograd function when a train-mode step under grad mode needs a backward: some parameter
    requires a gradient, or the input does (x.grad with every parameter frozen: saliency maps, adversarial examples)."""
    return model.training and torch.is_grad_enabled() and (x.requires_grad or any(p.requires_grad for p in model.parameters()))


def wants_eval_autograd(model, x):
    """The eval-mode twin of wants_autograd: model.forward routes an eval() forward through the autograd function (BatchNorm with
    its running statistics, frozen: saliency maps, integrated gradients, fine-tuning with frozen BatchNorm) when grad mode is on,
    the input or some parameter requires a gradient, and no Grad-CAM hooks are registered (those keep hooked_eval_forward)."""
    if model.training or not torch.is_grad_enabled():
        return False
    if not (x.requires_grad or any(p.requires_grad for p in model.parameters())):
        return False
    from ..gradcam import hooks_registered
    return not hooks_registered(model)


def input_grad_buffer(x_shape, device):
    """fp32 (B, 3, H, W) buffer cx_stem_input_grad writes (every element)."""
    if len(x_shape) != 4 or x_shape[1] != 3:
        raise RuntimeError("the input gradient needs a (B,3,H,W) float input (got %s)" % (tuple(x_shape),))
    return torch.empty(x_shape[0], 3, x_shape[2], x_shape[3], dtype=torch.float32, device=device)


def check_input_grad(buf, x):
    """forward_backward(input_grad=buf): a preallocated fp32 (B,3,H,W) tensor on x's device (shape checks only: no host sync)."""
    if buf.dtype != torch.float32 or not buf.is_contiguous() or buf.device != x.device or tuple(buf.shape) != tuple(x.shape) \
            or x.dim() != 4 or x.shape[1] != 3:
        raise RuntimeError("input_grad must be a contiguous fp32 tensor of the (B,3,H,W) float input's shape on its device")


@contextlib.contextmanager
def params_untouched(params, flat_grad):
    """Backward of a step in which no parameter requires a gradient (only x.grad was asked for): the engine still computes its
    weight gradients into its flat buffer, but afterwards every parameter's .grad is what it was before (None stays None; a .grad
    that views the flat buffer gets its values back)."""
    saved = [p.grad for p in params]
    backup = flat_grad.clone() if any(g is not None for g in saved) else None
    for p in params:
        p.grad = None
    try:
        yield
    finally:
        if backup is not None:
            flat_grad.copy_(backup)
        for p, g in zip(params, saved):
            p.grad = g


AUCM_DATA_PARALLEL = ("the AUC-margin loss (kind='aucm') is not supported data-parallel (world size %d): each rank would update its "
                      "auxiliary scalars a, b, alpha from its own shard, and averaging their gradients needs a collective of its "
                      "own at a new cut of the segmented step, which has not been built -- train on one GPU, or use the "
                      "cross-entropy")


BARLOW_DATA_PARALLEL = ("the Barlow Twins loss (kind='barlow') is not supported data-parallel (world size %d): each rank would normalise and "
                        "correlate its own rows only, and gathering the embeddings across ranks (with the gradient's way back) has not "
                        "been built -- pretrain on one GPU")


NTXENT_DATA_PARALLEL = ("the contrastive loss (kind='ntxent') is not supported data-parallel (world size %d): each rank would contrast "
                        "its own rows only, and gathering the embeddings across ranks (with the gradient's way back) has not been built "
                        "-- pretrain on one GPU")


def check_single_process(reducer, message):
    """Raises RuntimeError(message % world size) when gradients are averaged over more than one rank (`reducer`: the engine's
    GradReducer, or None): the losses that are not a sum over a rank's own elements."""
    world = getattr(reducer, "world", 1) if reducer is not None else 1
    if world > 1:
        raise RuntimeError(message % world)


def check_aucm_single_process(reducer):
    """check_single_process for the AUC-margin loss."""
    check_single_process(reducer, AUCM_DATA_PARALLEL)


# --------------------------------------------------------------------------------------------- module side
class _Fn(torch.autograd.Function):
    """loss.backward() through a fused network: forward runs the engine's training forward -- in eval mode its recording eval
    forward (running statistics, and what backward reads) --, backward its backward pass (in eval mode with frozen BatchNorm).
    `anchor` is a parameter of the network, so that autograd records the call; x.grad is returned when the input needs it."""

    @staticmethod
    def forward(ctx, x, anchor, model):
        eng = model._engine
        ws = eng.forward(x, model.training, record=True)
        ctx.model, ctx.eng, ctx.ws, ctx.x_meta = model, eng, ws, (tuple(x.shape), x.dtype, x.device)
        ctx.eval_mode = not model.training
        return ws.logits.clone()

    @staticmethod
    def backward(ctx, dlogits):
        eng, ws = ctx.eng, ctx.ws
        if ws is None:
            raise RuntimeError("backward through the fused %s can only run once per forward" % type(ctx.model).__name__)
        if ctx.eval_mode and torch.is_grad_enabled():
            raise RuntimeError("double backward (create_graph=True) through the fused %s is not supported: its backward runs as "
                               "HIP kernels outside autograd" % type(ctx.model).__name__)
        shape, dtype, dev = ctx.x_meta
        dx = input_grad_buffer(shape, dev) if ctx.needs_input_grad[0] else None
        frozen = not any(p.requires_grad for p in ctx.model.parameters())
        with params_untouched(eng.params, eng.flat_grad) if frozen else contextlib.nullcontext():
            eng.backward(ws, dlogits.contiguous().float(), dx=dx)
        eng.release(ws)
        ctx.ws = None
        return (dx.to(dtype) if dx is not None else None), None, None


class FusedNet(nn.Module):
    """nn.Module surface of a network whose forward / backward run as one schedule of fused HIP kernels.  A subclass supplies
    `_eng()` (its engine, built lazily into `_engine`) and `_anchor()` (the parameter the autograd function is recorded on)."""

    def __init__(self):
        super().__init__()
        self._nbt_pending = 0            # training forwards not yet counted in the BatchNorms' num_batches_tracked
        self._engine = None
        # set_loss(): plain tensors / flags, not buffers (the state_dict keys stay what they are); read through loss_kind,
        # loss_pos_weight, ... below
        self._loss = Loss()
        self._pool_kind = "avg"          # set_pool(): "gem" adds the parameter pool_p, "lse" the buffer pool_r
        self._pool_locked = False        # a fused optimiser has been built over the parameters
        self._head_kind = "linear"       # set_head(): "csra" adds the buffer head_attn = [lambda, T]; "pcam" adds nothing

    def set_loss(self, ignore_negative=False, pos_weight=None, *, kind="bce", prior=None, margin=1.0, lr_aux=None, gamma=None,
                 alpha=None, gamma_pos=None, gamma_neg=None, clip=None, class_weight=None, parent=None, mode=None, temperature=None,
                 lambd=None):
        """The loss of forward_backward.  ignore_negative: a target < 0 (an uncertain label kept as -1, the U-Ignore policy) adds no
        loss and no gradient; the divisor stays the batch size.  pos_weight: None, or n_classes positive-term weights as in torch's
        BCEWithLogitsLoss(pos_weight).  Either option routes the step through cx_bce_masked_fwd_bwd, which skips every target < 0:
        the weighted loss has no arithmetic for a negative target, so pos_weight implies the skipping, and ignore_negative decides
        between the two kernels only when there are no weights.  set_loss() puts the plain loss back, to which a negative target
        is a number like any other.  The weights live in one fp32 tensor (`loss_pos_weight`), neither buffer nor parameter, so
        state_dict() is what it was.  Returns self.

        Choose the loss BEFORE a step is captured (GraphedTrainStep, SegmentedTrainStep): a captured step replays the kernel and
        the weight storage it was captured with.  What a replay does see is a change of the weights' VALUES -- in place
        (`model.loss_pos_weight.mul_(2)`) or by set_loss(pos_weight=...) with the same number of weights and the same options,
        which copies into the held storage.  A switch between the plain and the masked loss, from no weights to weights or
        back, or to another number of weights (new storage) needs a new capture.

        kind="aucm" replaces the cross-entropy by the AUC min-max-margin loss (Yuan et al., ICCV 2021; cx_aucm_fwd_bwd): a
        squared-hinge surrogate of the per-class AUROC with three auxiliary scalars per class, which forward_backward trains
        beside the network (descent on a and b, ascent on alpha >= 0, rate lr_aux, after the backward pass of a train-mode step).
        prior: n_classes positive rates in (0, 1); margin > 0; lr_aux > 0.  It skips every target < 0 (ignore_negative has nothing
        left to decide), counts a target >= 0.5 as a positive, and cannot be combined with pos_weight (ValueError).  The state is
        plain tensors again: `loss_aux` (3, n) = rows a, b, alpha, zero at first; `loss_prior` (n,); `loss_lr_aux` (one float);
        loss_state() / load_loss_state() carry them to a checkpoint and back.  The storage rule is the one of the weights:
        set_loss(kind="aucm", ...) on a model that already holds the loss for the same number of classes copies prior and lr_aux
        into the held storage and leaves `loss_aux` as trained, so a captured step sees the new values (as it sees
        `model.loss_lr_aux.fill_(r)`); coming from another kind, or with another number of classes, `loss_aux` starts at zero.  A
        change of kind or of the margin (passed by value) needs a new capture.  The data-parallel step is not supported: the
        auxiliary gradients would need a collective of their own (forward_backward raises when the engine averages gradients over
        more than one rank).

        kind="focal" (gamma=2.0, alpha=None) and kind="asl" (gamma_pos=0.0, gamma_neg=4.0, clip=0.05) replace the cross-entropy by
        the focal loss (Lin et al., ICCV 2017) and the asymmetric loss (Ridnik et al., ICCV 2021), one kernel for both
        (cx_asl_fwd_bwd; the definition stands in include/chexpert_hip.h): the cross-entropy term of every element is multiplied by
        (1 - p_t)^gamma, with its own exponent for positives and negatives and the negatives' probability shifted down by clip, below
        which a hard negative adds nothing at all.  The focusing weight is part of the derivative (it is not detached).  gamma,
        gamma_pos, gamma_neg >= 0; clip in [0, 1); alpha None or in (0, 1), the positives' share of the class balance a = alpha t +
        (1 - alpha)(1 - t).  Both kinds skip every target < 0, take soft targets, and accept pos_weight (the held storage above).
        The four numbers live in one fp32 device tensor, `loss_focus` = [gamma+, gamma-, clip, alpha or -1], neither buffer nor
        parameter; a repeated call copies into the held storage.  For a captured step the rule of the weights holds: a change of
        kind, or from no pos_weight to weights or back, needs a new capture; a change of VALUES -- `model.loss_focus[1] = 2`, or
        set_loss with the same kind and new numbers -- is seen by the next replay, so a gamma schedule needs none.  The
        data-parallel step needs nothing new (the sum over elements is averaged over the ranks like the cross-entropy's).  An
        operand out of range, or a keyword of another kind, is a ValueError that changes nothing.

        kind="multiclass" (class_weight=None) is the U-MultiClass policy of the data set's paper (Irvin et al., AAAI 2019), a different
        model rather than a different label table: the head has THREE outputs per finding -- columns 3k, 3k + 1, 3k + 2 are finding
        k's negative, positive and uncertain logit -- and the loss is the softmax cross-entropy over each triple, summed over the
        findings and averaged over the batch (cx_mc3_fwd_bwd; the arithmetic stands in include/chexpert_hip.h).  The target stays the
        (B, n) table: class 2 where t < 0 (an uncertain label kept as -1), 1 where t >= 0.5, else 0; nothing is ignored and there is
        no soft-target form.  The head width must be a multiple of 3; pos_weight and ignore_negative=True are refused.
        class_weight: None, or a finite (n, 3) table > 0 whose entry [k][c] multiplies the terms of finding k with class c; it lives
        in one fp32 tensor, `loss_class_weight`, neither buffer nor parameter, under the storage rule of the weights: a repeated call
        with the same shape copies into the held storage, which a captured step's replay sees (as it sees an in-place change);
        from no weights to weights or back needs a new capture.  Nothing changes per step, and the data-parallel step needs nothing
        new.  At test time loss.collapse_multiclass(logits) gives the binary (B, n) logits z = z_positive - z_negative.

        kind="hier" (parent=, mode="conditional" | "unconditional", pos_weight=None) is the hierarchical label loss over a tree of
        findings (Chen et al., MIDL 2019; the conditional training of Pham et al., 2019; cx_hier_fwd_bwd, whose arithmetic stands in
        include/chexpert_hip.h): every logit is the logit of P(finding | its parent is positive).  parent: one entry per output of
        the head, the index of the finding's parent or -1 for a root, parents before children, no path longer than 8
        (data.CHEXPERT_PARENT for the 14 CheXpert findings); a table of another length is a ValueError.  'conditional' is the masked
        cross-entropy in which an element also drops out where an ancestor's target is not positive (< 0.5, or ignored);
        'unconditional' is the cross-entropy of the product of the sigmoids along the path from the root.  Both skip every target
        < 0 (ignore_negative=True is refused: there is nothing left to decide), take soft targets and accept pos_weight.  The
        table lives in one int32 device tensor, `loss_parent`, under the storage rule of the weights: a repeated call with a table
        of the same length copies into the held storage, which a captured step's replay sees (as it sees an in-place change; such
        a change is the caller's to keep a valid table).  The mode is passed by value, like the margin: a change of mode, like a
        change of kind or from no pos_weight to weights, needs a new capture.  Nothing changes per step; the loss is a sum over
        elements with divisor B, so the data-parallel step reduces it as it does the cross-entropy.  At test time
        loss.collapse_hierarchy(logits, model.loss_parent) gives the unconditional logits; class_cam, Grad-CAM and heads.class_maps
        work on the conditional logits as they are, so their maps show the evidence for a finding GIVEN its parent.

        kind="ntxent" (temperature=0.2) is contrastive pretraining: the head's n outputs are an EMBEDDING (the classifier nn.Linear is
        the projection), the target of forward_backward is an (N, 1) fp32 column of ids, and the loss is NT-Xent / SupCon over the rows
        of the batch (cx_ntxent_fwd_bwd; the definition stands in include/chexpert_hip.h and, in numpy, in loss.reference_ntxent):
        rows with the same id >= 0 are each other's positives, a row with an id < 0 is out of the batch.  pos_weight,
        ignore_negative=True and every other kind's keyword are refused.  The temperature (finite, > 0) lives in one fp32 device
        tensor, `loss_temperature`, under the storage rule of the weights: a repeated call copies into the held storage, and a
        captured step's replay sees that, as it sees `model.loss_temperature.fill_(0.1)`.  The kernels' scratch is held with the loss
        state and sized by the first step of a batch size (a capture's warm-up steps).  Both views of an image pass through the
        network in ONE batch, so BatchNorm's statistics are shared between them, as in SimCLR.  The data-parallel step is refused:
        the negatives would be each rank's own, and gathering embeddings across ranks is a feature of its own.

        kind="barlow" (lambd=0.0051) is Barlow Twins pretraining, the loss that needs neither negatives nor a large batch: the same
        operands as kind="ntxent" -- the head's n <= 1024 outputs are an embedding, the target an (N, 1) fp32 column of ids, rows p and
        p + N // 2 the two views of an image -- but the ids are a mask only (a pair with an id < 0 in either row is out of the batch).
        Both views are batch-normalised over the pairs, and loss = sum_k (1 - C_kk)^2 + lambd sum_{k != l} C_kl^2 over their d x d
        cross-correlation matrix C (cx_barlow_fwd_bwd, csrc/barlow.hip: the products run on the fp32-input MFMA; the definition stands
        in include/chexpert_hip.h and, in numpy, in loss.reference_barlow).  lambd (finite, >= 0) lives in one fp32 device tensor,
        `loss_lambda`, under the storage rule of `loss_temperature`; the scratch is held and sized the same way.  pos_weight,
        ignore_negative=True, temperature and every other kind's keyword are refused; so is the data-parallel step."""
        self._loss.set(next(self.parameters()).device, self._n_classes(), ignore_negative, pos_weight, kind=kind, prior=prior,
                       margin=margin, lr_aux=lr_aux, gamma=gamma, alpha=alpha, gamma_pos=gamma_pos, gamma_neg=gamma_neg, clip=clip,
                       class_weight=class_weight, parent=parent, mode=mode, temperature=temperature, lambd=lambd)
        return self

    # ---- the global pooling in front of the classifier
    def set_pool(self, kind="avg", r=10.0, p=3.0):
        """The global pooling of the head: "avg" (the default: the kernels of the average head, untouched), "max", "lse" (log-sum-exp
        with sharpness r > 0) or "gem" (generalised mean with the trained exponent p in [1, 16]); the definitions stand in
        chexpert_amd/pooling.py.  "gem" registers the parameter `pool_p` (shape (1,), trained with the network: its gradient lives in
        the flat gradient buffer, behind every other parameter's), "lse" registers the buffer `pool_r` (one fp32 value in device
        memory, not trained; a captured step sees `model.pool_r.fill_(5.0)`).  An "avg" or "max" model keeps exactly the state_dict
        keys it had.  Call it BEFORE the engine binds the parameters -- before the first forward, and before a fused optimiser is
        built over the model's parameters --: afterwards it raises RuntimeError.  An invalid kind, r <= 0 or p outside [1, 16] is a
        ValueError that changes nothing.  class_cam, the Grad-CAM hook path and the channel-padded CIFAR DenseNet-BC assume the
        average and refuse another kind.  Returns self."""
        from ..pooling import check_pool
        kind, r, p = check_pool(kind, r, p)
        if kind != "avg" and self._head_kind in ("csra", "pcam"):
            raise ValueError("set_pool(%r): the %s head (set_head) pools its score map itself and stands on the average pool"
                             % (kind, self._head_kind))
        if self._pool_bound():
            raise RuntimeError("set_pool() must be called before the engine has bound the parameters (before the first forward and "
                               "before a fused optimiser is built): the pooling parameter is part of the flat parameter buffer")
        dev = next(self.parameters()).device
        self._parameters.pop("pool_p", None)
        self._buffers.pop("pool_r", None)
        self._pool_kind = kind
        if kind == "gem":
            self.register_parameter("pool_p", nn.Parameter(torch.full((1,), p, dtype=torch.float32, device=dev)))
        elif kind == "lse":
            self.register_buffer("pool_r", torch.full((1,), r, dtype=torch.float32, device=dev))
        return self

    def _pool_bound(self):
        """Whether the parameter list is fixed: the engine has bound the parameters to its flat buffer (the engine flag), or a fused
        optimiser has been built over them."""
        return self._pool_locked or (self._engine is not None and getattr(self._engine, "flat", None) is not None)

    @property
    def pool_kind(self):
        return self._pool_kind

    def pool_param(self):
        """The device tensor the pooling kernels read: r for "lse", p for "gem", None otherwise."""
        return {"lse": self._buffers.get("pool_r"), "gem": self._parameters.get("pool_p")}.get(self._pool_kind)

    def pool_state(self):
        """What a checkpoint keeps beside the state_dict to rebuild the head: {kind, r} (r None unless kind is "lse"; GeM's p is a
        parameter and travels in the state_dict)."""
        return {"kind": self._pool_kind, "r": float(self.pool_r.item()) if self._pool_kind == "lse" else None}

    def load_pool_state(self, d):
        """Restores pool_state() (None or {}: the average) -- before load_state_dict, which then finds `pool_p` / `pool_r`.  Returns
        self."""
        d = d or {}
        kind = d.get("kind", "avg")
        return self.set_pool(kind, r=d["r"]) if kind == "lse" and d.get("r") is not None else self.set_pool(kind)

    def require_avg_pool(self, what):
        """class_cam, the Grad-CAM hooks and the channel-padded twin read the head as an average in front of the classifier."""
        if self._pool_kind != "avg":
            raise NotImplementedError("%s assumes the global average pool: this model pools with set_pool(%r)" % (what, self._pool_kind))
        if self._head_kind != "linear":
            raise NotImplementedError("%s assumes the linear head: this model has set_head(%r) (its maps: heads.class_maps)"
                                      % (what, self._head_kind))

    # ---- the head: activation -> pool -> classifier ("linear"), or the classifier at every pixel, pooled per class ("csra")
    def set_head(self, kind="linear", lam=0.1, T=1.0):
        """The head of the network: "linear" (the default: activation, global pool, classifier; the kernels it always ran, untouched)
        or "csra", class-specific residual attention (Zhu & Wu, ICCV 2021): the classifier is applied at every pixel of the last
        feature map and the score map s is pooled per class, logit = bias + mean_p s + lam * sum_p softmax_p(T s) s; the definition
        stands in chexpert_amd/heads.py.  It is the same nn.Linear under the same state_dict keys, and lam = 0 is the linear head as
        a function, so a checkpoint of a linear-head model loads into a csra model.  "csra" registers the buffer `head_attn`, an fp32
        (2,) device tensor [lam, T] that the kernels read (not trained, not part of the state_dict: head_state() carries it; a
        captured step sees `model.head_attn[0] = 0.2`).  Call it BEFORE the engine binds the parameters -- before the first forward,
        and before a fused optimiser is built --: afterwards it raises RuntimeError.  An invalid kind, lam < 0, T <= 0 or a
        non-finite value is a ValueError that changes nothing, as is "csra" on a model whose set_pool is not the average, or with
        more than 64 outputs.  class_cam, the Grad-CAM hook path and the channel-padded CIFAR DenseNet-BC refuse a csra model;
        heads.class_maps gives its score and attention maps.
        "pcam" is probabilistic-CAM pooling (Ye et al. 2020): the same score map, pooled per class with the per-pixel probabilities
        sigmoid(s + bias) as weights, logit = sum_p w (s + bias), w = sigmoid(s + bias) / sum_p sigmoid(s + bias).  It has no
        hyper-parameter (lam and T are validated and unused), registers no buffer and adds no state_dict key; the ordering rule, the
        average pool, the 64 outputs and the refusals are csra's; a linear checkpoint loads, but the function changes.
        heads.class_maps gives its probability maps and pooling weights.  Returns self."""
        from ..heads import MAX_CLASSES, check_head
        kind, lam, T = check_head(kind, lam, T)
        if kind != "linear" and self._pool_kind != "avg":
            raise ValueError("set_head(%r) stands on the average pool: this model pools with set_pool(%r)" % (kind, self._pool_kind))
        if kind != "linear" and self._n_classes() > MAX_CLASSES:
            raise ValueError("set_head(%r) takes at most %d outputs (this classifier has %d)" % (kind, MAX_CLASSES, self._n_classes()))
        if self._pool_bound():
            raise RuntimeError("set_head() must be called before the engine has bound the parameters (before the first forward and "
                               "before a fused optimiser is built): a bound engine has chosen its head kernels")
        dev = next(self.parameters()).device
        self._buffers.pop("head_attn", None)
        self._non_persistent_buffers_set.discard("head_attn")
        self._head_kind = kind
        if kind == "csra":
            self.register_buffer("head_attn", torch.tensor([lam, T], dtype=torch.float32, device=dev), persistent=False)
        return self

    @property
    def head_kind(self):
        return self._head_kind

    def head_state(self):
        """What a checkpoint keeps beside the state_dict to rebuild the head: {kind, lam, T} (lam and T None unless kind is "csra")."""
        if self._head_kind != "csra":
            return {"kind": self._head_kind, "lam": None, "T": None}
        lam, T = (float(v) for v in self.head_attn.tolist())
        return {"kind": "csra", "lam": lam, "T": T}

    def load_head_state(self, d):
        """Restores head_state() (None or {}: the linear head).  Returns self."""
        d = d or {}
        kind = d.get("kind", "linear")
        if kind == "csra" and d.get("lam") is not None and d.get("T") is not None:
            return self.set_head(kind, lam=d["lam"], T=d["T"])
        return self.set_head(kind)

    def named_parameters(self, prefix="", recurse=True, remove_duplicate=True):
        """nn.Module's order with `pool_p` moved to the end: backward produces the gradients from the end of the flat buffer to its
        start (the head first), and the data-parallel reducer cuts its buckets in that order."""
        held, pp = None, self._parameters.get("pool_p")
        for name, q in super().named_parameters(prefix=prefix, recurse=recurse, remove_duplicate=remove_duplicate):
            if pp is not None and q is pp:
                held = (name, q)
            else:
                yield name, q
        if held is not None:
            yield held

    def _n_classes(self):
        """Width of the final Linear layer (the classifier of every family)."""
        return [m for m in self.modules() if isinstance(m, nn.Linear)][-1].out_features

    def resize_classifier(self, n_out):
        """Replaces the classifier (the last nn.Linear) by a fresh one of n_out outputs on the same device -- a contrastive
        checkpoint's projection becomes a head of one logit per finding (probe.load_into) -- and drops the engine, which is built
        anew over the new parameters at the next forward.  Refused once a fused optimiser holds the parameters.  Returns self."""
        name, old = [(k, m) for k, m in self.named_modules() if isinstance(m, nn.Linear)][-1]
        if old.out_features == n_out:
            return self
        if self._pool_locked:
            raise RuntimeError("resize_classifier: the classifier has %d outputs, %d are asked for, and a fused optimiser holds the "
                               "parameters: build the model anew" % (old.out_features, n_out))
        new = nn.Linear(old.in_features, n_out).to(device=old.weight.device, dtype=old.weight.dtype)
        parent, _, leaf = name.rpartition(".")
        setattr(self.get_submodule(parent) if parent else self, leaf, new)
        object.__setattr__(self, "_engine", None)
        return self

    def loss_state(self):
        """What set_loss(kind=...) holds beyond the model's state_dict, as CPU tensors and floats: {kind, aux, prior, margin, lr_aux}
        (aux, prior and lr_aux are None for kind 'bce').  Kinds 'focal' and 'asl' add `focus`, the four numbers of `loss_focus`, kind
        'multiclass' adds `class_weight` (the (n, 3) table, or None), kind 'hier' adds `parent` (the int32 table) and `mode` (the name).  A
        checkpoint keeps it beside the weights."""
        return self._loss.state()

    def load_loss_state(self, d):
        """Restores loss_state(): for kind 'aucm' the loss is set with the stored prior, margin and rate, and the auxiliary scalars
        are copied in (into the held storage when there is one for this number of classes).  Kind 'bce' leaves the options of
        the cross-entropy (ignore_negative, pos_weight) as they are.  Kinds 'focal' and 'asl' set the loss with the stored `focus`
        (checked like set_loss's operands) and keep the pos_weight the model holds.  Kind 'multiclass' sets the loss with the stored
        `class_weight`.  Kind 'hier' sets the loss with the stored `parent` and `mode` and keeps the pos_weight the model holds.
        Returns self."""
        self._loss.load_state(d, next(self.parameters()).device, self._n_classes())
        return self

    def loss_step_state(self):
        """The tensors beyond parameters and buffers that a train-mode forward_backward changes (a graph capture's warm-up steps
        really run: it puts them back).  The focal and asymmetric losses change nothing per step."""
        return self._loss.step_state()

    def storage_dtype(self, dtype):
        """Storage type of the activations inside the fused schedule: torch.bfloat16 (default: bf16 tensors, fp32 accumulation
        and statistics) or torch.float32 -- the parity mode of north_star ("1e-3 fp32"): the same schedule on fp32 tensors with
        the exact f32 MFMA (csrc/conv_f32.hip).  Parameters are fp32 masters either way.  Returns self."""
        dtype = {"bf16": torch.bfloat16, "fp32": torch.float32}.get(dtype, dtype)
        if dtype not in (torch.bfloat16, torch.float32):
            raise ValueError("storage dtype must be bf16 or fp32")
        object.__setattr__(self, "_storage_dtype", dtype)
        return self

    def state_dict(self, *args, **kwargs):
        if self._nbt_pending:
            for mod in self.modules():
                if isinstance(mod, nn.BatchNorm2d) and mod.num_batches_tracked is not None:
                    mod.num_batches_tracked += self._nbt_pending
            self._nbt_pending = 0
        return super().state_dict(*args, **kwargs)

    def forward(self, x):
        if not x.is_cuda:
            raise RuntimeError("chexpert_amd %s runs on the GPU only (hand-written HIP kernels); there is no CPU fallback -- move "
                               "the model and the input to cuda" % type(self).__name__)
        eng = self._eng()
        if wants_autograd(self, x):
            return _Fn.apply(x, self._anchor(), self)
        if not self.training:
            from ..gradcam import hooked_eval_forward, hooks_registered
            if hooks_registered(self):                     # Grad-CAM hook protocol of the reference (chexpert.py:271-272)
                self.require_avg_pool("the Grad-CAM hook path (hooked_eval_forward)")
                return hooked_eval_forward(self, x)
            if wants_eval_autograd(self, x):               # frozen-BatchNorm backward (saliency, fine-tuning with frozen BN)
                return _Fn.apply(x, self._anchor(), self)
        ws = eng.forward(x, self.training)
        out = ws.logits.clone()
        eng.release(ws)
        return out

    def embed(self, x, return_logits=False):
        """The (B, C) fp32 vector the classifier reads -- the pooled features of one eval-mode forward (a clone of the engine's
        `pooled`, after set_pool's pooling of whichever kind) -- for the kNN probe and retrieval (chexpert_amd.knn).  The launches are
        those of model(x); return_logits=True returns (features, logits) of that one forward, the logits bit for bit model(x)'s.  A
        model in train mode is refused (batch statistics would make a row depend on its batch), as is a csra / pcam head, which has
        no pooled vector."""
        if not x.is_cuda:
            raise RuntimeError("chexpert_amd %s runs on the GPU only (hand-written HIP kernels); there is no CPU fallback -- move "
                               "the model and the input to cuda" % type(self).__name__)
        if self.training:
            raise RuntimeError("embed() needs the model in eval mode: with batch statistics a row's features would depend on its batch "
                               "(call model.eval())")
        if self._head_kind != "linear":
            raise NotImplementedError("embed() needs the linear head: the %s head (set_head) pools per-class score maps and has no pooled "
                                      "feature vector" % self._head_kind)
        eng = self._eng()
        with torch.no_grad():
            ws = eng.forward(x, False)
            feats = ws.pooled.clone()
            logits = ws.logits.clone() if return_logits else None
            eng.release(ws)
        return (feats, logits) if return_logits else feats

    # fused training step (bench / trainer fast path; same arithmetic as chexpert.py:159-163)
    def forward_backward(self, x, target, input_grad=None, track_stats=True):
        """logits = model(x); loss = BCEWithLogits(logits, target).sum(1).mean(0); loss.backward().
        Returns (loss, logits) as device tensors without a host sync.  input_grad: None, or a preallocated fp32 (B,3,H,W) tensor that
        also receives d loss / d x (what x.grad would hold), still without a host sync.  In eval mode this is the frozen-BatchNorm
        step (running statistics, which stay as they are).  After set_loss(...) the loss ignores targets < 0 and / or weights the
        positive term per class (same reduction, same divisor).  After set_loss(kind="aucm", ...) the loss is the AUC-margin loss,
        and a train-mode step ends with the update of its auxiliary scalars (`loss_aux`), from the gradients of this step; the
        eval-mode step computes the gradients and leaves `loss_aux` alone.  After set_loss(kind="focal" | "asl") the loss is the
        focal / asymmetric loss (ops.asl_fwd_bwd), in either mode.  After set_loss(kind="multiclass") the logits are (B, 3n) against
        the (B, n) target and the loss is the three-way softmax cross-entropy per finding (ops.mc3_fwd_bwd), in either mode.  After
        set_loss(kind="hier") the loss is the hierarchical one over the held parent table (ops.hier_fwd_bwd), in either mode.  After
        set_loss(kind="ntxent") the target is the (B, 1) column of ids and the loss the contrastive one over the rows (ops.ntxent_fwd_bwd).
        track_stats=False: a train-mode step computes with batch statistics as always, but writes no BatchNorm running statistic
        and counts no batch (the second pass of optim.FusedSAM); the launches are the same, the coefficient kernels get no running
        buffers."""
        eng = self._eng()
        if input_grad is not None:
            check_input_grad(input_grad, x)
        L = self._loss
        if L.kind == "aucm":
            check_aucm_single_process(eng.reducer)
        if L.kind == "ntxent":
            check_single_process(eng.reducer, NTXENT_DATA_PARALLEL)
        if L.kind == "barlow":
            check_single_process(eng.reducer, BARLOW_DATA_PARALLEL)
        eng.track_stats = bool(track_stats)
        try:
            ws = eng.forward(x, self.training, record=True)
        finally:
            eng.track_stats = True
        B, n = ws.logits.shape
        loss = torch.empty(1, dtype=torch.float32, device=x.device)
        dl = torch.empty(B, n, dtype=torch.float32, device=x.device)
        L.launch(ws.logits, target, loss, None, dl)                            # one launch, whatever set_loss chose
        eng.backward(ws, dl, dx=input_grad)
        if L.kind == "aucm" and self.training:                                 # from this step's gradients; eval leaves them alone
            ops.aucm_aux_step(L.aux, L.daux, L.lr_aux)
        logits = ws.logits.clone()
        eng.release(ws)
        return loss, logits


# what set_loss holds, readable on the model (read-only: set_loss writes; a tensor may be written in place)
for _name in ("kind", "ignore_negative", "pos_weight", "margin", "aux", "prior", "lr_aux", "focus", "class_weight", "parent", "mode", "temperature", "daux"):
    setattr(FusedNet, ("_loss_" if _name == "daux" else "loss_") + _name, property(lambda self, _name=_name: getattr(self._loss, _name)))
FusedNet.loss_lambda = property(lambda self: self._loss.lambd)


# --------------------------------------------------------------------------------------------- engine side
def _up4(n):
    return (n + 3) // 4 * 4


def flatten(tensors, dev):
    """Moves `tensors` into one new zero-padded fp32 buffer on dev, each at a 16-byte aligned offset, and makes every tensor's data
    its view there.  Returns (buffer, offsets in floats)."""
    offs, total = [], 0
    for t in tensors:
        offs.append(total)
        total += _up4(t.numel())
    flat = torch.zeros(total, dtype=torch.float32, device=dev)
    for t, off in zip(tensors, offs):
        flat[off:off + t.numel()].copy_(t.data.reshape(-1))
        t.data = flat[off:off + t.numel()].view(t.shape)
    return flat, offs


class _Vec:
    """Carves fp32 vectors out of one flat tensor (16-byte aligned), from offset `base` on."""

    def __init__(self, base=0):
        self.n = base

    def take(self, n):
        off = self.n
        self.n += _up4(n)
        return (off, n)


class _BN:
    """Vector slots of one BatchNorm: forward coefficients sc / sh / mean / rstd, backward coefficients pa / pb / pc."""

    def __init__(self, V, C):
        self.C = C
        self.sc, self.sh, self.mean, self.rstd = (V.take(C) for _ in range(4))
        self.pa, self.pb, self.pc = (V.take(C) for _ in range(3))

    @staticmethod
    def plan(bns):
        """Slots of every BatchNorm of `bns` in one vector.  Returns ({id(bn): _BN}, the _Vec, for more slots behind them)."""
        V = _Vec()
        return {id(bn): _BN(V, bn.num_features) for bn in bns}, V


class FusedEngine:
    """Host side of a fused network: binds the module's parameters to one flat fp32 buffer (and their gradients to another),
    packs the convolution weights into the kernels' layouts, keeps the activation workspaces, and wraps the network's backward
    schedule (`_backward`) in the step protocol: .grad binding, weight-gradient deferral and the data-parallel reducer."""

    def __init__(self, model):
        self.model = model
        # activation storage type: bf16, or fp32 = the parity mode of north_star ("1e-3 fp32")
        self.dtype = getattr(model, "_storage_dtype", torch.bfloat16)
        self.flat = self.flat_grad = self.device = None
        self.pool = {}
        self.reducer = None          # chexpert_amd.parallel.GradReducer when data-parallel
        # False for the span of one forward (FusedNet.forward_backward(track_stats=False)): a train-mode forward computes with batch
        # statistics, writes no running_mean / running_var and counts no batch
        self.track_stats = True
        self.packed_version = None

    # ---- binding
    def bound(self, dev):
        """Whether the module's parameters still are the views of the flat buffer on dev."""
        if self.flat is None or self.device != dev:
            return False
        params = list(self.model.parameters())
        return len(params) == len(self.offsets) and \
            all(p.data_ptr() == self.flat.data_ptr() + 4 * off for p, off in zip(params, self.offsets))

    def bind_params(self, dev):
        """The fp32 parameter masters become views of one flat buffer, their gradients views of another (grad_views)."""
        m = self.model
        params = list(m.parameters())
        for p in params:
            if p.dtype != torch.float32:
                raise RuntimeError("parameters must be fp32 masters (bf16 is the kernels' storage type)")
        for b in m.buffers():
            if b.device != dev:
                raise RuntimeError("module buffers are on %s, input on %s -- call model.to(device)" % (b.device, dev))
        self.flat, self.offsets = flatten(params, dev)
        self.params = params
        self.flat_grad = torch.zeros_like(self.flat)
        self.grad_views = [self.flat_grad[off:off + p.numel()].view(p.shape) for p, off in zip(params, self.offsets)]
        self.off_of = {id(p): off for p, off in zip(params, self.offsets)}
        self.device = dev
        self.pool = {}

    def plan_packing(self, convs, stem=None, stem_layout=False, stem8=None):
        """Descriptor table of the weight packing (CxPackDesc, one launch packs them all): `stem` in the forward layout only (the
        7x7 stride-2 stem kernel's own layout when stem_layout), then every conv of `convs` in the forward (w_fwd) and transposed
        (w_bwd) layouts -- a grouped conv as one convolution per group --, then the region of `stem8`, a 3-input-channel stem that
        _pack_stem8 pads to 8 channels and packs itself (at stem_off)."""
        descs, cur = [], 0
        self.wf, self.wb = {}, {}

        def add(conv, transpose=False, stem=False):
            nonlocal cur
            O, I, kh, kw = conv.weight.shape
            src = self.off_of[id(conv.weight)]
            gr = getattr(conv, "groups", 1)
            if gr > 1:
                # the filters of group g are rows [g O/G, (g+1) O/G) of the (O, I/G, kh, kw) weight -- contiguous --; the entry is
                # the list of the groups' (offset, size)
                og, n = O // gr, (O // gr) * I * kh * kw
                ent = []
                for g in range(gr):
                    descs.append(CxPackDesc(src + g * n, cur, og, I, kh, kw, int(transpose), 0))
                    ent.append((cur, n))
                    cur += (n + 7) // 8 * 8
                return ent
            n = (49 * O * 4 if self.dtype == torch.float32 else 7 * O * 32) if stem else O * I * kh * kw
            descs.append(CxPackDesc(src, cur, O, I, kh, kw, int(transpose), int(stem)))
            off = cur
            cur += (n + 7) // 8 * 8
            return (off, n)
        if stem is not None:
            self.wf[id(stem)] = add(stem, stem=stem_layout)
        for conv in convs:
            self.wf[id(conv)] = add(conv)
            self.wb[id(conv)] = add(conv, transpose=True)
        if stem8 is not None:
            self.stem_off = cur
            cur += 9 * stem8.out_channels * 8
        self.packed = torch.empty(cur, dtype=self.dtype, device=self.device)
        arr = (CxPackDesc * len(descs))(*descs)
        self.desc_dev = torch.frombuffer(bytearray(bytes(arr)), dtype=torch.uint8).to(self.device)
        self.n_desc = len(descs)
        self.packed_version = None

    def pack(self, train):
        # training: parameters change every step (possibly through the fused optimiser, which does not bump tensor versions) ->
        # always repack (one launch); eval: only when a version moved
        ver = None if train else sum(p._version for p in self.params)
        if ver is not None and ver == self.packed_version:
            return
        ops.pack_weights_table(self.flat, self.packed, self.desc_dev, self.n_desc)
        self._pack_stem8()
        self.packed_version = ver

    def _pack_stem8(self):
        """Packs the stem8 region of plan_packing (networks with a 3-to-8-channel stem)."""

    def w_fwd(self, conv, group=None):
        off, n = self.wf[id(conv)] if group is None else self.wf[id(conv)][group]
        return self.packed[off:off + n]

    def w_bwd(self, conv, group=None):
        off, n = self.wb[id(conv)] if group is None else self.wb[id(conv)][group]
        return self.packed[off:off + n]

    def grad_of(self, p):
        """p's gradient in the flat gradient buffer (1-D view)."""
        off = self.off_of[id(p)]
        return self.flat_grad[off:off + p.numel()]

    @staticmethod
    def recorded(ws, train, record):
        """Marks a forward's workspace: ws.frozen (an eval forward: backward takes the frozen-BatchNorm form) and ws.recorded
        (whether it holds everything backward reads)."""
        ws.frozen = not train
        ws.recorded = train or record

    @staticmethod
    def bn_bwd_coef(ws, bn, S1, S2, count, gamma, mean, rstd, dgamma, dbeta, A, Bc, pa, pb, pc, Cn, replicas=1, rstride=0, q=None, lo=0):
        """Backward coefficients of BatchNorm `bn` over its channels [lo, lo + Cn) (gamma, mean, rstd, dgamma, dbeta, A, Bc already
        sliced by the caller): ops.bn_bwd_coef after a training forward; after an eval forward the frozen form
        (ops.bn_bwd_coef_eval: running statistics, no batch-statistic terms, A / Bc untouched, identity slice coefficients)."""
        if not ws.frozen:
            return ops.bn_bwd_coef(S1, S2, count, gamma, mean, rstd, dgamma, dbeta, A, Bc, pa, pb, pc, Cn, replicas=replicas,
                                   rstride=rstride, q=q)
        ops.bn_bwd_coef_eval(S1, S2, mean, rstd, bn.running_mean[lo:lo + Cn], bn.running_var[lo:lo + Cn], gamma, bn.eps, dgamma,
                             dbeta, pa, pb, pc, Cn, replicas=replicas, rstride=rstride, q=q)

    def _bn_train(self, bn):
        """(gamma, beta, eps, momentum, running mean, running var) of a training BatchNorm as the coefficient kernels take them:
        momentum None counts as 0.1, the running buffers are None when the module tracks none -- or when this forward tracks none
        (`track_stats` off: the second pass of FusedSAM)."""
        track = bn.track_running_stats and self.track_stats
        return (bn.weight, bn.bias, bn.eps, bn.momentum if bn.momentum is not None else 0.1,
                bn.running_mean if track else None, bn.running_var if track else None)

    # ---- BatchNorm coefficients of an engine that keeps its _BN slots in `self.bn` ({id(bn): _BN}) and its statistic rows in
    # ws.slab[0] / ws.slab[1] (ResNet, EfficientNet)
    def _bn_coef(self, ws, bn, count, train, rows=None):
        """Forward coefficients of `bn` (scale, shift, mean, rstd) from the `rows` statistic rows over `count` values per channel
        its producer has just written, with the running-statistic update; eval: from the running statistics."""
        S, v = self.bn[id(bn)], self._v
        if train:
            ops.bn_coef(ws.slab[0], ws.slab[1], count, *self._bn_train(bn), v(ws, S.sc), v(ws, S.sh), v(ws, S.mean), v(ws, S.rstd), S.C,
                        replicas=rows, rstride=S.C)
        else:
            ops.bn_coef_eval(bn.running_mean, bn.running_var, bn.weight, bn.bias, bn.eps, v(ws, S.sc), v(ws, S.sh), v(ws, S.mean),
                             v(ws, S.rstd), S.C)

    def _bn_bwd(self, ws, bn, rows, count, s2=None):
        """Backward coefficients pa / pb / pc of `bn` and its dgamma / dbeta from the `rows` statistic rows of its backward sums S1 /
        S2 over `count` values per channel (s2: the rows of S2 where they are not ws.slab[1]); everything else follows from bn's slot."""
        S, v, G = self.bn[id(bn)], self._v, self.grad_of
        self.bn_bwd_coef(ws, bn, ws.slab[0], ws.slab[1] if s2 is None else s2, count, bn.weight, v(ws, S.mean), v(ws, S.rstd),
                         G(bn.weight), G(bn.bias), None, None, v(ws, S.pa), v(ws, S.pb), v(ws, S.pc), S.C, replicas=rows, rstride=S.C)

    @staticmethod
    def _v(ws, slot, n=None):
        off, m = slot
        return ws.vec[off:off + (m if n is None else n)]

    # ---- operand keywords of the convolutions around a BatchNorm whose record S names its vectors (sc, sh, pa, pb, pc: a _BN,
    # or an engine's own record with these fields); c_: the channel range of a grouped convolution
    @staticmethod
    def _ch(t, c_):
        return t if c_ is None else t[..., c_]

    def _pro_bnrelu(self, ws, S, c_=None):
        """forward: relu(bn_S(.)) of the operand"""
        return dict(prologue=ops.PRO_AFFINE_RELU, pa=self._ch(self._v(ws, S.sc), c_), pb=self._ch(self._v(ws, S.sh), c_))

    def _x_bnrelu(self, ws, S, c_=None):
        """weight gradient: relu(bn_S(.)) of the activation operand"""
        return dict(x_prologue=ops.PRO_AFFINE_RELU, pa=self._ch(self._v(ws, S.sc), c_), pb=self._ch(self._v(ws, S.sh), c_))

    def _pro_bnbwd(self, ws, y, S, c_=None):
        """input gradient: BatchNorm S's backward of the gradient operand, dY = dz * pa + y * pb + pc"""
        ch, v = self._ch, self._v
        return dict(prologue=ops.PRO_AFFINE2, x2=ch(y, c_), pa=ch(v(ws, S.pa), c_), pb=ch(v(ws, S.pb), c_), pc=ch(v(ws, S.pc), c_))

    def _g_bnbwd(self, ws, y, S, c_=None):
        """weight gradient: the same of its gradient operand"""
        ch, v = self._ch, self._v
        return dict(g_prologue=ops.PRO_AFFINE2, g2=ch(y, c_), ga=ch(v(ws, S.pa), c_), gb=ch(v(ws, S.pb), c_), gc=ch(v(ws, S.pc), c_))

    # ---- the classifier head of every engine, from the last feature map x (read as act(x*sc + sh), act an ops.POOL_ACT_*) to ws.logits
    # and back.  FusedNet.set_head / set_pool choose the path (_head_path); the average pool's kernels follow the activation:
    #   ReLU:  head_fwd (pool and classifier in one kernel);   head_bwd, gap_relu_bn_bwd
    #   Swish: gap_affine_act, linear_fwd;                      head_bwd, se_act_bwd
    # another pooling (max / lse / gem) runs pool_head_fwd + linear_fwd and head_bwd, pool_p_grad (gem), pool_head_bwd; a head that
    # pools a per-pixel score map (csra / pcam) runs map_head_fwd in the place of pool + classifier and map_head_bwd in the place of
    # head_bwd + the pool's backward.  Every backward leaves g / S1 / S2 as the average's does.  mask: None, or the (B, C) Dropout
    # mask in front of the classifier (EfficientNet), which a score-map head's kernels apply themselves.
    def pool_kind(self):
        return getattr(self.model, "pool_kind", "avg")

    def head_kind(self):
        return getattr(self.model, "head_kind", "linear")

    def _head_path(self):
        """The head's path by one name: set_head's "csra" / "pcam" (they stand on the average pool), else set_pool's "avg" / "max" /
        "lse" / "gem" in front of the linear classifier."""
        head = self.head_kind()
        return head if head != "linear" else self.pool_kind()

    def _head_fwd(self, ws, x, sc, sh, fc, act, mask=None, rows=None):
        """Fills ws.logits, and ws.pooled where the path has one.  ws.drop (the mask) and ws.fc_in (what the classifier read) stay for
        the way back.  rows: the scratch rows of the Swish average (gap_affine_act)."""
        m, path = self.model, self._head_path()
        ws.drop, ws.fc_in = mask, ws.pooled
        if path in ("csra", "pcam"):
            return self._map_fwd(ws, path, x, sc, sh, mask, fc, act)
        if path == "avg" and act == ops.POOL_ACT_RELU:
            assert mask is None, "head_fwd applies the classifier itself: nothing comes in between"
            return ops.head_fwd(x, sc, sh, fc.weight, fc.bias, ws.pooled, ws.logits)
        if path == "avg":
            ops.gap_affine_act(x, sc, sh, ws.pooled, act=act, rows=rows)
        else:
            # ws.pool_aux: GeM's T, which pool_p_grad reads; LSE's offset, which its backward reads
            if path != "max" and getattr(ws, "pool_aux", None) is None:
                ws.pool_aux = torch.empty_like(ws.pooled)
            ops.pool_head_fwd(x, sc, sh, ws.pooled, ws.pool_aux if path != "max" else None, m.pool_param(), act=act, kind=path)
        if mask is not None:
            ws.pooled_d = torch.empty_like(ws.pooled)
            ops.mul_f32(ws.pooled, mask, ws.pooled_d)
            ws.fc_in = ws.pooled_d
        ops.linear_fwd(ws.fc_in, fc.weight, fc.bias, ws.logits)

    def _head_bwd(self, ws, dlogits, x, sc, sh, mean, rstd, e_scale, g, S1, S2, stat_rows, fc, act, mask, done):
        """The head's backward from dlogits: the classifier's gradients, then g = e_scale * dz and the BatchNorm backward sums S1 / S2
        of dz.  The reducer hears of pool_p first (gem: it is the last parameter of the flat buffer) and of fc.weight after a
        score-map head's backward.  Returns the statistic rows."""
        m, G, path = self.model, self.grad_of, self._head_path()
        db = G(fc.bias) if fc.bias is not None else None
        if path in ("csra", "pcam"):
            return self._map_bwd(ws, path, dlogits, x, sc, sh, mask, mean, rstd, e_scale, g, S1, S2, stat_rows, fc, db, act, done)
        dpooled = torch.empty_like(ws.pooled)
        ops.head_bwd(dlogits, ws.fc_in, fc.weight, G(fc.weight), db, dpooled)
        if mask is not None:
            ops.mul_f32(dpooled, mask, dpooled)
        if path == "avg" and act == ops.POOL_ACT_RELU:
            return ops.gap_relu_bn_bwd(dpooled, x, sc, sh, mean, rstd, e_scale, g, S1, S2, stat_rows)
        if path == "avg":                      # (se_act_bwd takes no e_scale: the Swish head's is 1)
            return ops.se_act_bwd(None, x, sc, sh, mean, rstd, None, dpooled, g, S1, S2, stat_rows)
        if path == "gem":
            ops.pool_p_grad(dpooled, ws.pooled, ws.pool_aux, m.pool_p, G(m.pool_p))
            done(m.pool_p)
        return ops.pool_head_bwd(dpooled, ws.pooled, ws.pool_aux if path != "max" else None, m.pool_param(), x, sc, sh, mean, rstd,
                                 e_scale, g, S1, S2, act=act, kind=path, stat_rows=stat_rows)

    def _map_fwd(self, ws, kind, x, sc, sh, m, fc, act):
        """ws.logits of the csra / pcam head.  ws.head_s (the per-pixel score map) and ws.head_stat stay for the way back and for
        class_maps; ws.head_scratch is allocated by the first backward."""
        B, H, W, _ = x.shape
        n = fc.out_features
        if getattr(ws, "head_s", None) is None:
            ws.head_s = torch.empty(B, n, H * W, dtype=torch.float32, device=self.device)
            ws.head_stat = torch.empty(B, n, ops.CSRA_STAT, dtype=torch.float32, device=self.device)
            ws.head_scratch = None
        ws.head_hw = (H, W)
        ops.map_head_fwd(kind, x, sc, sh, m, fc.weight, fc.bias, self._head_attn(kind), ws.logits, ws.head_s, ws.head_stat, act=act)

    def _map_bwd(self, ws, kind, dlogits, x, sc, sh, m, mean, rstd, e_scale, g, S1, S2, stat_rows, fc, db, act, done):
        """The csra / pcam head's backward: the classifier's gradients are added where head_bwd adds them (pcam's bias gradient is the
        kernel's sum_b dlogit (1 + r)).  Returns the statistic rows."""
        B, H, W, C = x.shape
        if ws.head_scratch is None:
            ws.head_scratch = torch.empty(ops.map_bwd_scratch(kind, B, H * W, C, fc.out_features), dtype=torch.float32, device=self.device)
        rows = ops.map_head_bwd(kind, dlogits, ws.head_s, ws.head_stat, self._head_attn(kind), x, sc, sh, m, mean, rstd, e_scale, fc.weight,
                                g, S1, S2, self.grad_of(fc.weight), db, ws.head_scratch, act=act, stat_rows=stat_rows)
        done(fc.weight)
        return rows

    def _head_attn(self, kind):
        """csra's [lambda, T] in device memory; pcam has none."""
        return self.model.head_attn if kind == "csra" else None

    # ---- workspaces
    def acquire(self, B, H, W):
        lst = self.pool.setdefault((B, H, W), [])
        return lst.pop() if lst else self._new_workspace(B, H, W)

    def release(self, ws):
        lst = self.pool.setdefault(ws.key, [])
        if len(lst) < 2:
            lst.append(ws)

    # ---- backward
    def _defer_wgrad(self):
        """Whether a backward pass defers the ordered slab sums of its weight gradients to one table-driven launch at its end."""
        return True

    def backward(self, ws, dlogits, dx=None):
        """The backward pass of the forward that filled `ws`, from d loss / d logits; dx: None, or an fp32 (B,3,H,W) buffer that also
        receives the input gradient (cx_stem_input_grad).  Gradients accumulate into the parameters' .grad, which are views of
        the flat gradient buffer (bound here when some .grad is None)."""
        if not getattr(ws, "recorded", True):
            raise RuntimeError("this eval forward recorded nothing for a backward: run forward(x, False, record=True)")
        ops.set_det_wgrad(True)                # reproducible weight-gradient sums beside the ordered statistic rows
        # the ordered slab sums run as one table-driven launch at the end of the pass (ops.wgrad_defer_*); a data-parallel run
        # flushes them before each gradient bucket leaves (GradReducer.pre_launch)
        deferred = self._defer_wgrad() and ops.wgrad_defer_begin(self.device)
        try:
            fresh = any(p.grad is None for p in self.params)
            if fresh:
                self.flat_grad.zero_()
            elif not all(p.grad.data_ptr() == gv.data_ptr() for p, gv in zip(self.params, self.grad_views)):
                raise RuntimeError("parameter .grad tensors were replaced; call zero_grad(set_to_none=True) first")
            red = self.reducer
            if red is not None:
                red.begin()
            done = (lambda p: red.ready(self.off_of[id(p)])) if red is not None else (lambda p: None)
            self._backward(ws, dlogits, dx, done)
            if red is not None:
                red.finish()
            if fresh:
                for p, gv in zip(self.params, self.grad_views):
                    p.grad = gv
            if deferred:
                ops.wgrad_defer_flush(self.device)
        finally:
            if deferred:
                ops.wgrad_defer_abort(self.device)

    def _pre_bucket(self):
        # the deferred weight-gradient slab sums (ops.wgrad_defer_*) run before each bucket leaves, so that the bucket is final
        ops.wgrad_defer_flush(self.device, keep=True)

    def enable_data_parallel(self, bucket_bytes=16 << 20, group=None):
        """Average gradients across ranks inside backward (bucketed all-reduce overlapped with the remaining backward kernels).
        Call after the first bind (i.e. after one forward)."""
        from ..parallel import GradReducer
        if self.flat_grad is None:
            raise RuntimeError("bind the engine first (run one forward)")
        self.reducer = GradReducer(self.flat_grad, bucket_bytes, group)
        self.reducer.pre_launch = self._pre_bucket
