"""The loss of a training step, stated once for its two routes.  `Loss` is what `FusedNet.set_loss` holds: the kind, its numbers and
the device tensors the kernels of csrc/loss.hip read, with the one rule that picks the kernel (`Loss.launch`).  The modules below are
the same losses outside the fused step -- `loss = MaskedBCE(w)(model(x), t); loss.backward()` and the element losses of an
evaluation -- over the same `launch`, so the autograd route and the fused step run one kernel and agree bit for bit: MaskedBCE for
the cross-entropy with uncertain-label handling (cx_bce_fwd_bwd / cx_bce_masked_fwd_bwd), AUCMLoss for kind "aucm" (cx_aucm_fwd_bwd),
with its auxiliary scalars as parameters, FocalLoss and AsymmetricLoss for kinds "focal" and "asl" (cx_asl_fwd_bwd),
MultiClassUncertain for kind "multiclass" (cx_mc3_fwd_bwd), the three-way softmax of the U-MultiClass policy, whose logits are (B, 3n)
and which `collapse_multiclass` turns into binary ones (cx_mc3_collapse), HierarchicalBCE for kind "hier" (cx_hier_fwd_bwd), the
conditional / unconditional loss over the findings' tree, whose conditional logits `collapse_hierarchy` turns into unconditional
ones (cx_hier_collapse), NTXentLoss for kind "ntxent" (cx_ntxent_fwd_bwd), the contrastive NT-Xent / SupCon loss of (N, d)
embeddings against an (N, 1) column of ids, the one loss that couples the rows of a batch; `reference_ntxent` states it in float64
numpy and `contrastive_top1` is its accuracy figure, BarlowTwinsLoss for kind "barlow" (cx_barlow_fwd_bwd, csrc/barlow.hip), the
cross-correlation loss of the two views' batch-normalised embeddings, with `reference_barlow` as its float64 statement and
`barlow_terms` as its monitor.  Device tensors only: there is no CPU path (but for the numpy statement)."""
import math

import numpy as np
import torch
import torch.nn as nn

from . import ops

KERNEL = {"bce": "cx_bce_masked_fwd_bwd", "aucm": "cx_aucm_fwd_bwd", "focal": "cx_asl_fwd_bwd", "asl": "cx_asl_fwd_bwd",
          "multiclass": "cx_mc3_fwd_bwd", "hier": "cx_hier_fwd_bwd", "ntxent": "cx_ntxent_fwd_bwd",
          "barlow": "cx_barlow_fwd_bwd"}
WIDTH = {"multiclass": 3}          # logits per target element, where it is not 1


# ------------------------------------------------------------------------------------------------ the range checks, each once
# `who` is the caller as its user wrote it (set_loss(kind='asl'), FocalLoss, ...); a refusal is a ValueError in its name.
def check_focus(who, gamma_pos, gamma_neg, clip, alpha, names=("gamma_pos", "gamma_neg")):
    """The four numbers of the focal / asymmetric loss as the kernel reads them: [gamma+, gamma-, clip, alpha or -1]."""
    try:
        gp, gn, m, al = (float(v) for v in (gamma_pos, gamma_neg, clip, -1.0 if alpha is None else alpha))
    except (TypeError, ValueError):
        raise ValueError("%s takes numbers (got %r)" % (who, (gamma_pos, gamma_neg, clip, alpha)))
    for name, v in zip(names, (gp, gn)):
        if not 0 <= v < float("inf"):
            raise ValueError("%s takes a finite %s >= 0 (got %r)" % (who, name, v))
    if not 0 <= m < 1:
        raise ValueError("%s takes a clip in [0, 1) (got %r)" % (who, m))
    if alpha is not None and not 0 < al < 1:          # (NaN fails it)
        raise ValueError("%s takes alpha None or in (0, 1) (got %r)" % (who, alpha))
    return [gp, gn, m, al]


def check_pos_weight(who, pos_weight, n=None):
    """None, or the positive-term weights as an fp32 vector (on the device they came on): finite, > 0, and n of them where n is given."""
    if pos_weight is None:
        return None
    w = torch.as_tensor(pos_weight, dtype=torch.float32).detach().reshape(-1)
    if (n is not None and w.numel() != n) or not bool(((w > 0) & torch.isfinite(w)).all()):
        raise ValueError("%s takes %sfinite pos_weight > 0 (got %s)" % (who, "" if n is None else "%d " % n, w.tolist()))
    return w


def check_class_weight(who, class_weight, n=None):
    """None, or the weights of the three-way softmax as an fp32 (n, 3) table (on the device they came on), row k = the weights of
    finding k's classes negative, positive, uncertain: finite, > 0, and n rows where n is given."""
    if class_weight is None:
        return None
    w = torch.as_tensor(class_weight, dtype=torch.float32).detach()
    shaped = w.dim() == 2 and w.shape[1] == 3 and w.shape[0] >= 1 and (n is None or w.shape[0] == n)
    if not shaped or not bool(((w > 0) & torch.isfinite(w)).all()):
        raise ValueError("%s takes finite class_weight > 0 of shape (%s, 3) (got shape %s: %s)"
                         % (who, "n" if n is None else n, tuple(w.shape), w.tolist()))
    return w


def check_prior(who, prior, margin, n=None):
    """The class positive rates of the AUC-margin loss as a CPU fp32 vector: in (0, 1), n of them where n is given; margin > 0."""
    if prior is None:
        raise ValueError("%s needs prior: the class positive rates" % who)
    p = torch.as_tensor(prior, dtype=torch.float32).detach().reshape(-1).cpu()
    if p.numel() < 1 or (n is not None and p.numel() != n):
        raise ValueError("%s takes one prior per class%s (got %d)" % (who, "" if n is None else ": %d" % n, p.numel()))
    if not bool(((p > 0) & (p < 1)).all()):
        raise ValueError("%s takes priors in (0, 1) (got %s)" % (who, p.tolist()))
    if not float(margin) > 0:
        raise ValueError("%s takes a margin > 0 (got %r)" % (who, margin))
    return p


def check_hier_mode(who, mode):
    """'conditional' / 'unconditional' (or cx_hier_fwd_bwd's 0 / 1) as the name."""
    names = {v: k for k, v in ops.HIER_MODES.items()}
    if isinstance(mode, str) and mode in ops.HIER_MODES:
        return mode
    if isinstance(mode, int) and not isinstance(mode, bool) and mode in names:
        return names[mode]
    raise ValueError("%s takes mode 'conditional' or 'unconditional' (got %r)" % (who, mode))


def check_temperature(who, temperature):
    """The temperature of the contrastive loss as a float: finite and > 0."""
    try:
        t = float(temperature)
    except (TypeError, ValueError):
        raise ValueError("%s takes a temperature, a number > 0 (got %r)" % (who, temperature))
    if not 0 < t < float("inf"):
        raise ValueError("%s takes a finite temperature > 0 (got %r)" % (who, temperature))
    return t


def check_lambda(who, lambd):
    """The off-diagonal weight of the Barlow Twins loss as a float: finite and >= 0."""
    try:
        v = float(lambd)
    except (TypeError, ValueError):
        raise ValueError("%s takes lambd, a number >= 0 (got %r)" % (who, lambd))
    if not 0 <= v < float("inf"):
        raise ValueError("%s takes a finite lambd >= 0 (got %r)" % (who, lambd))
    return v


# ------------------------------------------------------------------------------------------------ the loss of a step
class Loss:
    """The loss of a step: `kind` ('bce', 'aucm', 'focal', 'asl', 'multiclass', 'hier', 'ntxent', 'barlow'), `ignore_negative`, `margin` (a host float, passed
    by value), `mode` (kind 'hier': 'conditional' or 'unconditional', a host value like the margin, None elsewhere), `parent` (kind
    'hier': the int32 (n,) device table of each label's parent, -1 for a root) and the fp32 device tensors the kernels read -- `pos_weight` (n,), `focus` (4,) = [gamma+, gamma-, clip, alpha or -1],
    `aux` and `daux` (3, n) = rows a, b, alpha and their gradients, `prior` (n,), `lr_aux` (1,), `class_weight` (n, 3) = the weights
    of kind 'multiclass', whose head has 3n outputs, `temperature` (1,) of kind 'ntxent', whose logits are (N, d) embeddings and whose
    target is the (N, 1) column of ids, `lambd` (1,) of kind 'barlow', which takes the same operands --, None where the kind has none.
    Kinds 'ntxent' and 'barlow' also hold the kernels' scratch, sized by the
    first launch that needs it (never under a graph capture: a captured step's warm-up runs have sized it).  Plain
    tensors, neither buffers nor parameters.  Behind them stands held storage (`_held`, by name) that outlives a change of kind: a
    repeated set() with the same sizes copies into it, so a captured step, which replays the storage it was captured with, sees the
    new values.  FusedNet keeps one (set / state / load_state are its set_loss / loss_state / load_loss_state); a loss module makes
    one per call from its own attributes."""

    def __init__(self, kind="bce", ignore_negative=False, margin=1.0, pos_weight=None, focus=None, aux=None, daux=None, prior=None,
                 lr_aux=None, class_weight=None, parent=None, mode=None, temperature=None, lambd=None):
        self.kind, self.ignore_negative, self.margin = kind, ignore_negative, margin
        self.temperature, self.lambd = temperature, lambd
        self.parent, self.mode = parent, mode
        self.pos_weight, self.focus, self.aux, self.daux, self.prior, self.lr_aux = pos_weight, focus, aux, daux, prior, lr_aux
        self.class_weight = class_weight
        self._held = {}

    def launch(self, logits, target, loss, loss_elem, dlogits):
        """The loss (1,), the element losses (B, n) and d loss / d logits (B, n), each where given, in one launch.  The kernel is
        the kind's; for 'bce' the masked one when ignore_negative is set or there are weights (it skips every target < 0: the
        weighted loss has no arithmetic for a negative target), else the plain one, to which a negative target is a number.  Kind
        'multiclass' takes (B, 3n) logits and dlogits beside the (B, n) target and element losses."""
        if self.kind == "ntxent":
            ops.ntxent_fwd_bwd(logits, target, self.temperature, loss, loss_elem, dlogits, None, self._scratch(logits))
        elif self.kind == "barlow":
            if loss_elem is not None:
                raise RuntimeError("the Barlow Twins loss has no element losses")
            ops.barlow_fwd_bwd(logits, target, self.lambd, loss, dlogits, None, self._scratch(logits))
        elif self.kind == "aucm":
            if loss_elem is not None:
                raise RuntimeError("the AUC-margin loss has no element losses")
            ops.aucm_fwd_bwd(logits, target, self.prior, self.aux, self.margin, loss, None, dlogits, self.daux)
        elif self.kind == "multiclass":
            ops.mc3_fwd_bwd(logits, target, self.class_weight, loss, loss_elem, dlogits)
        elif self.kind == "hier":
            ops.hier_fwd_bwd(logits, target, self.parent, self.pos_weight, self.mode, loss, loss_elem, dlogits)
        elif self.kind in ("focal", "asl"):
            ops.asl_fwd_bwd(logits, target, self.pos_weight, self.focus, loss, loss_elem, dlogits)
        elif self.ignore_negative or self.pos_weight is not None:
            ops.bce_masked_fwd_bwd(logits, target, self.pos_weight, loss, loss_elem, dlogits)
        else:
            ops.bce_fwd_bwd(logits, target, loss, loss_elem, dlogits)

    def _scratch(self, logits):
        """The held scratch of kinds 'ntxent' and 'barlow' for these (N, d) embeddings: made on first use and when it is too small or
        on another device, which a stream under capture must not do."""
        barlow = self.kind == "barlow"
        need = (ops.barlow_scratch if barlow else ops.ntxent_scratch)(*logits.shape)
        held = self._held.get("scratch")
        if held is None or held.numel() < need or held.device != logits.device:
            if torch.cuda.is_current_stream_capturing():
                raise RuntimeError("the %s loss would allocate its scratch (%d floats) under a graph capture: run one step of "
                                   "this batch size before capturing" % ("Barlow Twins" if barlow else "contrastive", need))
            held = self._held["scratch"] = torch.empty(need, dtype=torch.float32, device=logits.device)
        return held

    def _hold(self, name, values, dev, keep=False, dtype=torch.float32):
        """`values` copied into the held storage `name`, which is made anew for another shape or another device; with `keep`,
        storage that is already there stays as it is.  None: None (the storage is kept for the next time)."""
        if values is None:
            return None
        v = torch.as_tensor(values, dtype=dtype)
        held = self._held.get(name)
        fresh = held is None or held.shape != v.shape or held.device != dev
        if fresh:
            held = self._held[name] = torch.empty(v.shape, dtype=dtype, device=dev)
        if fresh or not keep:
            held.copy_(v)
        return held

    def _put(self, who, dev, kind, ignore_negative, pos_weight=None, focus=None, prior=None, margin=None, lr_aux=None,
             class_weight=None, parent=None, mode=None, temperature=None, lambd=None):
        """The one place that writes the state, after every check: each field is assigned, to None where `kind` has none, so nothing
        of the previous kind is left over.  `aux` starts at zero coming from another kind and stays as trained coming from 'aucm';
        the margin stays what the last 'aucm' made it."""
        if dev.type != "cuda" and (kind != "bce" or pos_weight is not None):
            raise RuntimeError("%s holds its state on the parameters' device: call model.to(device) first" % who)
        zeros = None if prior is None else torch.zeros(3, prior.numel())
        self.aux = self._hold("aux", zeros, dev, keep=self.kind == "aucm")
        self.daux = self._hold("daux", zeros, dev, keep=True)
        self.pos_weight, self.focus = self._hold("pos_weight", pos_weight, dev), self._hold("focus", focus, dev)
        self.prior, self.lr_aux = self._hold("prior", prior, dev), self._hold("lr_aux", None if lr_aux is None else [lr_aux], dev)
        self.class_weight = self._hold("class_weight", class_weight, dev)
        self.parent, self.mode = self._hold("parent", parent, dev, dtype=torch.int32), mode
        self.temperature = self._hold("temperature", None if temperature is None else [temperature], dev)
        self.lambd = self._hold("lambd", None if lambd is None else [lambd], dev)
        self.kind, self.ignore_negative = kind, ignore_negative
        if margin is not None:
            self.margin = float(margin)

    def set(self, dev, n, ignore_negative=False, pos_weight=None, *, kind="bce", prior=None, margin=1.0, lr_aux=None, gamma=None,
            alpha=None, gamma_pos=None, gamma_neg=None, clip=None, class_weight=None, parent=None, mode=None, temperature=None,
            lambd=None):
        """FusedNet.set_loss for a model whose head has n outputs, with its parameters on dev.  A refused call changes nothing."""
        if kind not in KERNEL:
            raise ValueError("set_loss(kind=...) takes 'bce', 'aucm', 'focal', 'asl', 'multiclass', 'hier', 'ntxent' or 'barlow' (got %r)" % (kind,))
        if kind != "barlow" and lambd is not None:
            raise ValueError("set_loss: lambd belongs to kind='barlow'")
        if kind != "ntxent" and temperature is not None:
            raise ValueError("set_loss: temperature belongs to kind='ntxent'")
        if kind != "hier" and (parent is not None or mode is not None):
            raise ValueError("set_loss: parent and mode belong to kind='hier'")
        if kind != "multiclass" and class_weight is not None:
            raise ValueError("set_loss: class_weight belongs to kind='multiclass'")
        if kind != "aucm" and (prior is not None or lr_aux is not None or margin != 1.0):
            raise ValueError("set_loss: prior, margin and lr_aux belong to kind='aucm'")
        if kind != "focal" and (gamma is not None or alpha is not None):
            raise ValueError("set_loss: gamma and alpha belong to kind='focal'")
        if kind != "asl" and (gamma_pos is not None or gamma_neg is not None or clip is not None):
            raise ValueError("set_loss: gamma_pos, gamma_neg and clip belong to kind='asl'")
        who = "set_loss(kind=%r)" % kind
        if kind == "bce":
            w = None if pos_weight is None else torch.as_tensor(pos_weight, dtype=torch.float32).reshape(-1)
            self._put("set_loss(pos_weight=...)", dev, kind, bool(ignore_negative), w)
        elif kind == "aucm":
            if pos_weight is not None:
                raise ValueError("%s cannot be combined with pos_weight: the class prior is this loss's weighting" % who)
            p = check_prior(who, prior, margin, n)
            if lr_aux is None or not float(lr_aux) > 0:
                raise ValueError("%s needs lr_aux > 0, the rate of the auxiliary scalars (got %r)" % (who, lr_aux))
            self._put(who, dev, kind, True, prior=p, margin=margin, lr_aux=float(lr_aux))
        elif kind == "multiclass":
            if pos_weight is not None or ignore_negative:
                raise ValueError("%s cannot be combined with pos_weight or ignore_negative: an uncertain label is a class of its "
                                 "own there, and class_weight is this loss's weighting" % who)
            if n % 3:
                raise ValueError("%s needs a head of three outputs per finding (negative, positive, uncertain); this head has %d" % (who, n))
            self._put(who, dev, kind, False, class_weight=check_class_weight(who, class_weight, n // 3))
        elif kind == "ntxent":
            if pos_weight is not None or ignore_negative:
                raise ValueError("%s cannot be combined with pos_weight or ignore_negative: its target is a column of ids, of which a "
                                 "negative one takes its row out of the batch" % who)
            if n > ops.NTXENT_MAX_D:
                raise ValueError("%s takes embeddings of at most %d values; this head has %d outputs" % (who, ops.NTXENT_MAX_D, n))
            self._put(who, dev, kind, False, temperature=check_temperature(who, 0.2 if temperature is None else temperature))
        elif kind == "barlow":
            if pos_weight is not None or ignore_negative:
                raise ValueError("%s cannot be combined with pos_weight or ignore_negative: its target is a column of ids, of which a "
                                 "negative one takes its pair out of the batch" % who)
            if n > ops.BARLOW_MAX_D:
                raise ValueError("%s takes embeddings of at most %d values; this head has %d outputs" % (who, ops.BARLOW_MAX_D, n))
            self._put(who, dev, kind, False, lambd=check_lambda(who, 0.0051 if lambd is None else lambd))
        elif kind == "hier":
            if ignore_negative:
                raise ValueError("%s always ignores a target < 0; ignore_negative is the cross-entropy's switch" % who)
            if parent is None:
                raise ValueError("%s needs parent: for each of the head's %d outputs the index of its parent label, -1 for a root" % (who, n))
            table = ops.check_hier_parent(who, parent, n)
            self._put(who, dev, kind, True, check_pos_weight(who, pos_weight, n), parent=table,
                      mode=check_hier_mode(who, "conditional" if mode is None else mode))
        else:
            if kind == "focal":
                g = 2.0 if gamma is None else gamma
                focus = check_focus(who, g, g, 0.0, alpha, ("gamma", "gamma"))
            else:
                focus = check_focus(who, 0.0 if gamma_pos is None else gamma_pos, 4.0 if gamma_neg is None else gamma_neg,
                                    0.05 if clip is None else clip, None)
            self._put(who, dev, kind, True, check_pos_weight(who, pos_weight, n), focus)

    def step_state(self):
        """FusedNet.loss_step_state: the tensors a train-mode step changes."""
        return [self.aux] if self.kind == "aucm" else []

    def state(self):
        """FusedNet.loss_state: CPU tensors and floats."""
        def cpu(t):
            return None if t is None else t.detach().cpu().clone()
        d = {"kind": self.kind, "aux": cpu(self.aux), "prior": cpu(self.prior), "margin": float(self.margin),
             "lr_aux": None if self.lr_aux is None else float(self.lr_aux.item())}
        if self.focus is not None:
            d["focus"] = cpu(self.focus)
        if self.kind == "multiclass":
            d["class_weight"] = cpu(self.class_weight)
        if self.kind == "hier":
            d["parent"], d["mode"] = cpu(self.parent), self.mode
        if self.kind == "ntxent":
            d["temperature"] = float(self.temperature.item())
        if self.kind == "barlow":
            d["lambd"] = float(self.lambd.item())
        return d

    def load_state(self, d, dev, n):
        """FusedNet.load_loss_state."""
        kind = d["kind"]
        if kind in ("focal", "asl"):
            focus = d.get("focus")
            if focus is None or torch.as_tensor(focus).numel() != 4:
                raise ValueError("load_loss_state: kind %r needs focus, four numbers (got %r)" % (kind, focus))
            gp, gn, m, al = torch.as_tensor(focus, dtype=torch.float32).reshape(-1).tolist()
            who = "load_loss_state(kind=%r)" % kind
            focus = check_focus(who, gp, gn, m, None if al < 0 else al)
            self._put(who, dev, kind, True, check_pos_weight(who, self.pos_weight, n), focus)      # (the held weights stay)
        elif kind == "aucm":
            aux = torch.as_tensor(d["aux"], dtype=torch.float32)
            if tuple(aux.shape) != (3, n):
                raise ValueError("load_loss_state: aux must be (3, %d) (got %s)" % (n, tuple(aux.shape)))
            self.set(dev, n, kind="aucm", prior=d["prior"], margin=d["margin"], lr_aux=d["lr_aux"])
            self.aux.copy_(aux)
        elif kind == "multiclass":
            self.set(dev, n, kind="multiclass", class_weight=d.get("class_weight"))
        elif kind == "hier":
            if d.get("parent") is None:
                raise ValueError("load_loss_state: kind 'hier' needs parent, the table of the labels' parents")
            self.set(dev, n, kind="hier", parent=d["parent"], mode=d.get("mode"), pos_weight=self.pos_weight)   # (the held weights stay)
        elif kind == "ntxent":
            if d.get("temperature") is None:
                raise ValueError("load_loss_state: kind 'ntxent' needs temperature")
            self.set(dev, n, kind="ntxent", temperature=d["temperature"])
        elif kind == "barlow":
            if d.get("lambd") is None:
                raise ValueError("load_loss_state: kind 'barlow' needs lambd")
            self.set(dev, n, kind="barlow", lambd=d["lambd"])
        elif kind != "bce":
            raise ValueError("load_loss_state: unknown loss kind %r" % (kind,))
        elif self.kind != "bce":               # (a model that holds the cross-entropy keeps its options)
            self.set(dev, n)


# ------------------------------------------------------------------------------------------------ the autograd route
def _operands(logits, target, who, kind):
    """The contiguous fp32 logits and targets of a loss module: (B, n) both, or (B, 3n) against (B, n) for kind 'multiclass', or (N, d)
    embeddings against an (N, 1) column of ids for kinds 'ntxent' and 'barlow' (which needs N >= 2)."""
    width = WIDTH.get(kind, 1)
    if not logits.is_cuda:
        raise RuntimeError("%s runs on the GPU only (%s); there is no CPU fallback" % (who, KERNEL[kind]))
    if kind in ("ntxent", "barlow"):
        if logits.dim() != 2 or logits.shape[0] < (2 if kind == "barlow" else 1) or logits.shape[1] < 1 or tuple(target.shape) != (logits.shape[0], 1):
            raise RuntimeError("%s takes (N, d) embeddings and an (N, 1) column of ids (got %s and %s)" % (who, tuple(logits.shape), tuple(target.shape)))
        return logits.detach().contiguous().float(), target.detach().contiguous().float()
    if logits.dim() != 2 or logits.shape[1] % width or tuple(target.shape) != (logits.shape[0], logits.shape[1] // width):
        raise RuntimeError("%s takes %s (got %s and %s)" % (who, "(B, n) logits and targets of one shape" if width == 1 else
                                                            "(B, %dn) logits and (B, n) targets" % width, tuple(logits.shape), tuple(target.shape)))
    return logits.detach().contiguous().float(), target.detach().contiguous().float()


class _LossFn(torch.autograd.Function):
    """loss and d loss / d logits in one launch (Loss.launch); backward scales the stored gradient.  `aux`: nothing, or the a, b, alpha
    of an AUCMLoss, which autograd records; their gradients are the three rows of state.daux, from the same launch."""

    @staticmethod
    def forward(ctx, logits, target, state, who, *aux):
        x, t = _operands(logits, target, who, state.kind)
        loss = torch.empty(1, dtype=torch.float32, device=x.device)
        dl = torch.empty_like(x)
        state.launch(x, t, loss, None, dl)
        ctx.save_for_backward(dl, *([state.daux] if aux else []))
        ctx.in_dtype = logits.dtype
        return loss[0]

    @staticmethod
    def backward(ctx, grad_output):
        dl, *daux = ctx.saved_tensors
        grads = ((dl * grad_output).to(ctx.in_dtype), None, None, None)
        if daux:
            # alpha is the dual variable: the saddle point is a minimum in (w, a, b) and a maximum in alpha, so its gradient leaves
            # negated and the optimiser that descends on every parameter ascends on alpha
            grads += (daux[0][0] * grad_output, daux[0][1] * grad_output, -daux[0][2] * grad_output)
        return grads


class _LossModule(nn.Module):
    """What the loss modules share.  A subclass keeps its operands as plain attributes -- moved by hand to the logits' device
    (`.to` of the module leaves them), never in a state_dict -- and states them as a Loss in `_state(device)`."""
    _aux = ()                  # names of the parameters autograd records

    def _on(self, device, *names):
        for name in names:
            t = getattr(self, name)
            if t is not None and t.device != device:
                setattr(self, name, t.to(device))

    def forward(self, logits, target):
        who = type(self).__name__
        _operands(logits, target, who, self.kind)                          # (refuses a CPU tensor before anything is moved)
        return _LossFn.apply(logits, target, self._state(logits), who, *(getattr(self, name) for name in self._aux))

    @torch.no_grad()
    def elementwise(self, logits, target):
        """The (B, n) element losses (0 where ignored, and for a hard negative at or below the clip), outside autograd."""
        x, t = _operands(logits, target, type(self).__name__, self.kind)
        out = torch.empty(t.shape, dtype=torch.float32, device=x.device)
        self._state(x).launch(x, t, None, out, None)
        return out


class MaskedBCE(_LossModule):
    """BCEWithLogitsLoss(pos_weight)(logits, target) summed over the classes and averaged over the batch (chexpert.py:160), in which
    a target < 0 is ignored (no loss, no gradient; the divisor stays the batch size).  The two options select the kernel exactly
    as FusedNet.set_loss does: with ignore_negative or a pos_weight it is cx_bce_masked_fwd_bwd, which skips every target < 0 (the
    weighted loss has no arithmetic for a negative target, so pos_weight implies the skipping); with neither it is the plain
    cx_bce_fwd_bwd, to which a negative target is a number like any other, as it is to torch's BCEWithLogitsLoss."""
    kind = "bce"

    def __init__(self, pos_weight=None, ignore_negative=True):
        super().__init__()
        self.ignore_negative = bool(ignore_negative)
        self.pos_weight = None if pos_weight is None else torch.as_tensor(pos_weight, dtype=torch.float32).reshape(-1)

    @property
    def masked(self):
        return self.ignore_negative or self.pos_weight is not None

    def _state(self, logits):
        self._on(logits.device, "pos_weight")
        return Loss("bce", self.ignore_negative, pos_weight=self.pos_weight)


class AUCMLoss(_LossModule):
    """The AUC min-max-margin loss (Yuan et al., "Large-scale Robust Deep AUC Maximization", ICCV 2021) of (B, n) logits, summed
    over the classes: the loss of FusedNet.set_loss(kind="aucm") for the autograd route, by the same kernel, so `loss.backward()`
    leaves the fused step's d loss / d logits bit for bit.  prior: n class positive rates in (0, 1); margin > 0.  A target < 0 is
    ignored, a target >= 0.5 counts as a positive, the rest as negatives.

    The auxiliary scalars a, b, alpha are nn.Parameters of THIS module (shape (n,), zero at first): hand them to an optimiser
    beside the network's.  The problem is a saddle point -- minimise over the network, a and b, maximise over alpha >= 0 -- so
    backward returns alpha's gradient NEGATED: `alpha.grad` is -d loss / d alpha, and a descending optimiser ascends on alpha.
    Call clamp_() after each optimiser step to keep alpha >= 0 (plain SGD with rate lr_aux followed by clamp_() is the update
    FusedNet.forward_backward makes).  There are no element losses: elementwise() raises."""
    kind, _aux = "aucm", ("a", "b", "alpha")

    def __init__(self, prior, margin=1.0):
        super().__init__()
        self.prior = check_prior("AUCMLoss", prior, margin)
        self.margin = float(margin)
        self.a, self.b, self.alpha = (nn.Parameter(torch.zeros(self.prior.numel())) for _ in range(3))

    def _state(self, logits):
        self._on(logits.device, "prior")
        if self.a.device != logits.device:
            raise RuntimeError("AUCMLoss: a, b and alpha are on %s, the logits on %s -- call loss.to(device)" % (self.a.device, logits.device))
        if logits.shape[1] != self.prior.numel():
            raise RuntimeError("AUCMLoss holds %d classes, the logits have %d" % (self.prior.numel(), logits.shape[1]))
        aux = torch.stack([self.a.detach(), self.b.detach(), self.alpha.detach()]).float().contiguous()
        return Loss("aucm", True, self.margin, prior=self.prior, aux=aux, daux=torch.empty_like(aux))

    @torch.no_grad()
    def clamp_(self):
        """alpha >= 0, after an optimiser step.  Returns self."""
        self.alpha.clamp_(min=0)
        return self

    def elementwise(self, logits, target):
        raise RuntimeError("AUCMLoss has no element losses: it is a function of each class's whole batch column (its positives "
                           "against its negatives), not a sum over elements -- evaluate with MaskedBCE.elementwise or BCEWithLogitsLoss")


class _FocusLoss(_LossModule):
    """What FocalLoss and AsymmetricLoss share: the four numbers [gamma+, gamma-, clip, alpha or -1] the kernel reads from the device
    (`focus`) and the positive-term weights (`pos_weight`)."""

    def __init__(self, focus, pos_weight):
        super().__init__()
        self.focus = torch.tensor(focus, dtype=torch.float32)
        self.pos_weight = check_pos_weight(type(self).__name__, pos_weight)

    def _state(self, logits):
        self._on(logits.device, "focus", "pos_weight")
        return Loss(self.kind, True, pos_weight=self.pos_weight, focus=self.focus)


class FocalLoss(_FocusLoss):
    """The focal loss (Lin et al., "Focal Loss for Dense Object Detection", ICCV 2017) of (B, n) logits: torchvision's
    sigmoid_focal_loss(alpha, gamma) summed over the classes and averaged over the batch, a target < 0 ignored (the divisor stays the
    batch size), soft targets valid, pos_weight on the positive term -- the loss of FusedNet.set_loss(kind="focal") for the autograd
    route, by the same kernel, so `loss.backward()` leaves the fused step's d loss / d logits bit for bit.  gamma >= 0; alpha None
    (no class balance) or in (0, 1).  The focusing weight is differentiated, not detached."""
    kind = "focal"

    def __init__(self, gamma=2.0, alpha=None, pos_weight=None):
        super().__init__(check_focus("FocalLoss", gamma, gamma, 0.0, alpha, ("gamma", "gamma")), pos_weight)


class AsymmetricLoss(_FocusLoss):
    """The asymmetric loss (Ridnik et al., "Asymmetric Loss for Multi-Label Classification", ICCV 2021) of (B, n) logits, timm's
    AsymmetricLossMultiLabel (its blended form for soft targets) summed over the classes and averaged over the batch: positives
    -(1 - p)^gamma_pos log p, negatives -p_m^gamma_neg log(1 - p_m) with p_m = max(p - clip, 0), so a hard negative with p <= clip
    adds no loss and no gradient.  A target < 0 is ignored; pos_weight weights the positive term.  The loss of
    FusedNet.set_loss(kind="asl") for the autograd route, by the same kernel, bit for bit."""
    kind = "asl"

    def __init__(self, gamma_pos=0.0, gamma_neg=4.0, clip=0.05, pos_weight=None):
        super().__init__(check_focus("AsymmetricLoss", gamma_pos, gamma_neg, clip, None), pos_weight)


class MultiClassUncertain(_LossModule):
    """The U-MultiClass policy of the data set's paper (Irvin et al., "CheXpert", AAAI 2019) as a loss: every finding has three logits
    -- negative, positive, uncertain, columns 3k, 3k + 1, 3k + 2 of the (B, 3n) logits -- and the loss is the softmax cross-entropy
    over them, summed over the findings and averaged over the batch.  The (B, n) target is the table the other losses read: class 2
    where t < 0 (an uncertain label kept as -1), 1 where t >= 0.5, else 0; nothing is ignored and there is no soft-target form.
    class_weight: None, or a finite (n, 3) table > 0 whose entry [k][c] multiplies the terms of finding k with class c.  The loss of
    FusedNet.set_loss(kind="multiclass") for the autograd route, by the same kernel, bit for bit.  elementwise() gives the (B, n)
    terms; collapse_multiclass() the binary logits an evaluation reads."""
    kind = "multiclass"

    def __init__(self, class_weight=None):
        super().__init__()
        self.class_weight = check_class_weight("MultiClassUncertain", class_weight)

    def _state(self, logits):
        self._on(logits.device, "class_weight")
        if self.class_weight is not None and logits.shape[1] != 3 * self.class_weight.shape[0]:
            raise RuntimeError("MultiClassUncertain holds %d findings, the logits have %d columns" % (self.class_weight.shape[0], logits.shape[1]))
        return Loss("multiclass", False, class_weight=self.class_weight)


@torch.no_grad()
def collapse_multiclass(logits, return_uncertain=False):
    """The binary logits of (B, 3n) three-way logits (cx_mc3_collapse): z (B, n) = z_positive - z_negative in fp32, so that sigmoid(z)
    is the paper's test-time probability, the softmax over negative and positive with "uncertain" dropped; everything that takes
    (B, n) logits -- evaluation losses, AUROC, bootstrap, calibration, ensembles -- takes z.  return_uncertain: (z, p_unc) with
    p_unc (B, n) the softmax probability of "uncertain"."""
    if not logits.is_cuda:
        raise RuntimeError("collapse_multiclass runs on the GPU only (cx_mc3_collapse); there is no CPU fallback")
    if logits.dim() != 2 or logits.shape[1] == 0 or logits.shape[1] % 3:
        raise RuntimeError("collapse_multiclass takes (B, 3n) logits (got %s)" % (tuple(logits.shape),))
    x = logits.detach().contiguous().float()
    z = torch.empty(x.shape[0], x.shape[1] // 3, dtype=torch.float32, device=x.device)
    p = torch.empty_like(z) if return_uncertain else None
    if x.shape[0]:
        ops.mc3_collapse(x, z, p)
    return (z, p) if return_uncertain else z


class HierarchicalBCE(_LossModule):
    """The hierarchical label loss of (B, n) logits over a tree of findings (Chen et al., "Deep hierarchical multi-label classification
    of chest X-ray images", MIDL 2019; the conditional training of Pham et al., 2019): every logit is the logit of
    P(finding | its parent is positive).  parent: for each finding the index of its parent, -1 for a root, parents before children
    (data.CHEXPERT_PARENT for the 14 CheXpert findings).  mode 'conditional' (HLCP): the masked cross-entropy of each logit, in which
    an element also drops out where an ancestor's target is not positive (< 0.5, or ignored).  mode 'unconditional' (HLUP): the
    cross-entropy of the product of the sigmoids along the path from the root, against the element's own target.  A target < 0 is
    ignored (the divisor stays the batch size), soft targets are valid, pos_weight weights the positive term.  The loss of
    FusedNet.set_loss(kind="hier") for the autograd route, by the same kernel, bit for bit.  elementwise() gives the (B, n) terms;
    collapse_hierarchy() the unconditional logits an evaluation reads."""
    kind = "hier"

    def __init__(self, parent, mode="conditional", pos_weight=None):
        super().__init__()
        self.parent = ops.check_hier_parent("HierarchicalBCE", parent)
        self.mode = check_hier_mode("HierarchicalBCE", mode)
        self.pos_weight = check_pos_weight("HierarchicalBCE", pos_weight, self.parent.numel())

    def _state(self, logits):
        self._on(logits.device, "parent", "pos_weight")
        if logits.shape[1] != self.parent.numel():
            raise RuntimeError("HierarchicalBCE holds %d findings, the logits have %d columns" % (self.parent.numel(), logits.shape[1]))
        return Loss("hier", True, pos_weight=self.pos_weight, parent=self.parent, mode=self.mode)


@torch.no_grad()
def collapse_hierarchy(logits, parent, return_prob=False):
    """The unconditional logits of (B, n) conditional ones (cx_hier_collapse): a root keeps its logit bit for bit, any other finding gets
    z = log P - log(1 - P) with P the product of the sigmoids along its path from the root, so that sigmoid(z) = P; everything that
    takes (B, n) logits -- evaluation losses, AUROC, bootstrap, DeLong, calibration, ensembles -- takes z.  parent: the table of
    HierarchicalBCE (a list, a CPU tensor, or the int32 device tensor a model holds as `loss_parent`).  return_prob: (z, P)."""
    if not logits.is_cuda:
        raise RuntimeError("collapse_hierarchy runs on the GPU only (cx_hier_collapse); there is no CPU fallback")
    if logits.dim() != 2 or logits.shape[1] == 0:
        raise RuntimeError("collapse_hierarchy takes (B, n) logits (got %s)" % (tuple(logits.shape),))
    x = logits.detach().contiguous().float()
    if isinstance(parent, torch.Tensor) and parent.is_cuda:
        parent = parent.to(device=x.device, dtype=torch.int32).contiguous()
    z = torch.empty_like(x)
    p = torch.empty_like(x) if return_prob else None
    if x.shape[0]:
        ops.hier_collapse(x, parent, z, p)
    else:
        ops.check_hier_parent("collapse_hierarchy", parent.cpu() if isinstance(parent, torch.Tensor) else parent, x.shape[1])
    return (z, p) if return_prob else z


# ------------------------------------------------------------------------------------------------ contrastive pretraining
NTXENT_EPS = 1e-12          # the clamp of the normalisation: z = e / max(|e|, eps)


def reference_ntxent(e, ids, temperature, dtype=np.float64):
    """The statement of cx_ntxent_fwd_bwd in numpy, in `dtype` (float64: the reference; float32: the model of the kernel's rounding
    that the tests hold their tolerance against).  e (N, d), ids (N,) or (N, 1), temperature > 0.  With V = {i : ids_i >= 0},
    z_i = e_i / max(|e_i|, 1e-12), s_ij = z_i . z_j / temperature, A(i) = V \\ {i} and P(i) = {j in A(i) : ids_j == ids_i}:
    l_i = -(1 / |P(i)|) sum_{p in P(i)} (s_ip - log sum_{a in A(i)} exp s_ia) for the anchors (the rows of V with a positive), 0 for
    every other row, loss = the mean of l_i over the anchors (0 without one).  Every id occurring twice: SimCLR's NT-Xent; otherwise
    SupCon's L_out.  Returns {"loss": float, "loss_elem": (N,), "grad": (N, d) = d loss / d e through the normalisation,
    "top1": (N,) int64, the a in A(i) with the largest s_ia (the lowest on a tie), -1 outside V or where A(i) is empty, "s": the (N, N)
    similarities with -inf outside A(i), "anchors": the boolean (N,) mask, "p": the (N, N) softmax of s over A(i) in the anchors' rows
    (0 elsewhere), "dS": d (M loss) / d s, row i the part that comes from l_i}."""
    e = np.asarray(e, dtype=dtype)
    g = np.asarray(ids, dtype=np.float64).reshape(-1)
    N, d = e.shape
    tau = dtype(temperature)
    norm = np.sqrt((e * e).sum(1, dtype=dtype))
    den = np.maximum(norm, dtype(NTXENT_EPS))
    V = g >= 0
    z = np.where(V[:, None], e / den[:, None], dtype(0))
    A = V[:, None] & V[None, :] & ~np.eye(N, dtype=bool)
    P = A & (g[:, None] == g[None, :])
    s = np.where(A, (z @ z.T) / tau, -np.inf).astype(dtype)
    nP = P.sum(1)
    nPf = np.maximum(nP, 1).astype(dtype)
    anchors = nP > 0
    M = int(anchors.sum())
    has = A.any(1)
    top1 = np.where(has, np.argmax(np.where(has[:, None], s, 0), axis=1), -1)
    m = np.where(has, np.max(np.where(has[:, None], s, 0), axis=1), dtype(0))
    ex = np.where(A, np.exp(np.where(A, s - m[:, None], 0)), dtype(0)).astype(dtype)
    se = ex.sum(1, dtype=dtype)
    lg = np.log(np.where(has, se, 1)).astype(dtype)
    ps = np.where(P, s - m[:, None], dtype(0)).sum(1, dtype=dtype)
    ell = np.where(anchors, lg - ps / nPf, dtype(0)).astype(dtype)
    p = np.where(anchors[:, None], ex / np.where(has, se, 1)[:, None], dtype(0)).astype(dtype)
    dS = np.where(anchors[:, None], p - P / nPf[:, None], dtype(0)).astype(dtype)
    out = {"loss_elem": ell, "top1": top1.astype(np.int64), "s": s, "anchors": anchors, "p": p, "dS": dS}
    if M == 0:
        out["loss"], out["grad"] = 0.0, np.zeros_like(e)
        return out
    out["loss"] = float(ell.sum(dtype=dtype) / dtype(M))
    dz = ((dS + dS.T) @ z) / (tau * dtype(M))
    above = (norm >= dtype(NTXENT_EPS))[:, None]
    proj = np.where(above, (dz * z).sum(1, dtype=dtype)[:, None] * z, dtype(0))
    out["grad"] = np.where(V[:, None], (dz - proj) / den[:, None], dtype(0)).astype(dtype)
    return out


class NTXentLoss(_LossModule):
    """The contrastive loss of (N, d) embeddings against an (N, 1) column of ids: SimCLR's NT-Xent (Chen et al., ICML 2020) where every
    id occurs exactly twice, SupCon's L_out (Khosla et al., NeurIPS 2020) otherwise; `reference_ntxent` is the definition.  Rows with
    the same id >= 0 are each other's positives, every other row with an id >= 0 is a negative, a row with an id < 0 is out of the
    batch.  The embeddings are normalised inside (z = e / max(|e|, 1e-12)) and the gradient goes back through that.  The loss of
    FusedNet.set_loss(kind="ntxent") for the autograd route, by the same kernels, so `loss.backward()` leaves the fused step's d loss /
    d logits bit for bit.  temperature: a finite number > 0; it lives in a one-float tensor (`temperature`) that may be rewritten in
    place.  elementwise() gives the (N, 1) terms l_i, 0 for a row that is not an anchor."""
    kind = "ntxent"

    def __init__(self, temperature=0.2):
        super().__init__()
        self.temperature = torch.tensor([check_temperature("NTXentLoss", temperature)], dtype=torch.float32)
        self._scratch = None

    def _state(self, logits):
        self._on(logits.device, "temperature")
        state = Loss("ntxent", False, temperature=self.temperature)
        if self._scratch is not None:
            state._held["scratch"] = self._scratch
        self._scratch = state._scratch(logits)               # (the module keeps it from call to call)
        return state


@torch.no_grad()
def contrastive_top1(logits, ids, return_counts=False):
    """The share of anchors -- rows with an id >= 0 that have a positive among the other rows -- whose nearest other row (the largest
    cosine similarity; cx_ntxent_fwd_bwd's top1) is one of their positives: the accuracy figure of contrastive pretraining.  logits
    (N, d) device embeddings, ids (N, 1) or (N,).  A float, NaN without an anchor; return_counts: (hits, anchors) as ints."""
    x, t = _operands(logits, ids.reshape(-1, 1), "contrastive_top1", "ntxent")
    top = torch.empty(x.shape[0], dtype=torch.int32, device=x.device)
    one = torch.ones(1, dtype=torch.float32, device=x.device)              # (the nearest row does not depend on the temperature)
    ops.ntxent_fwd_bwd(x, t, one, None, None, None, top)
    g = t.reshape(-1)
    valid = g >= 0
    same = (g[:, None] == g[None, :]) & valid[:, None] & valid[None, :]
    anchors = (same.sum(1) - valid.long()) > 0
    near = top.long().clamp(min=0)
    hit = anchors & (top >= 0) & (g[near] == g)
    hits, total = int(hit.sum().item()), int(anchors.sum().item())
    if return_counts:
        return hits, total
    return hits / total if total else math.nan


# ------------------------------------------------------------------------------------------------ Barlow Twins pretraining
BARLOW_EPS = 1e-5           # CX_BARLOW_EPS: the epsilon of the batch normalisation


def reference_barlow(e, ids, lambd, dtype=np.float64):
    """The statement of cx_barlow_fwd_bwd in numpy, in `dtype` (float64: the reference; float32: a model of fp32 rounding in another
    summation order than the kernels', which the tests hold their tolerance against).  e (N, d), ids (N,) or (N, 1), lambd >= 0 (used
    as the fp32 value the kernels read).  h = N // 2; row p < h is view A of pair p, row p + h view B, an odd last row belongs to no
    pair; V = {p : ids_p >= 0 and ids_{p+h} >= 0}, m = |V|.  Per view and column over V: mu = mean, v = the biased variance (two
    passes), a^ = (a - mu) / sqrt(v + 1e-5); C = A^T B^ / m; on = sum_k (1 - C_kk)^2, off = sum_{k != l} C_kl^2, loss = on + lambd
    off.  The gradient is the full chain: G_kk = -2 (1 - C_kk), G_kl = 2 lambd C_kl, da^ = b^ G^T / m, db^ = a^ G / m, then
    BatchNorm's backward da = (da^ - mean_p da^ - a^ mean_p (da^ o a^)) / sqrt(v + eps); rows outside V and the odd row are zeros,
    and what they hold (NaN included) is never read.  m < 2: loss 0, gradient 0.  Returns {"loss", "on", "off": floats, "C": (d, d),
    "grad": (N, d), "m": int, "mean_diag": float, "ahat", "bhat": (m, d), "valid": the boolean (h,) mask, "istd": (2, d)}."""
    e = np.asarray(e)
    g = np.asarray(ids, dtype=np.float64).reshape(-1)
    N, d = e.shape
    h = N // 2
    lam = dtype(np.float32(lambd))
    valid = (g[:h] >= 0) & (g[h:2 * h] >= 0)
    m = int(valid.sum())
    out = {"m": m, "valid": valid, "grad": np.zeros((N, d), dtype=dtype)}
    if m < 2:
        out.update(loss=0.0, on=0.0, off=0.0, mean_diag=0.0, C=np.zeros((d, d), dtype=dtype), ahat=np.zeros((m, d), dtype=dtype),
                   bhat=np.zeros((m, d), dtype=dtype), istd=np.zeros((2, d), dtype=dtype))
        return out
    mm, eps = dtype(m), dtype(BARLOW_EPS)

    def normalise(x):
        mu = x.sum(0, dtype=dtype) / mm
        c = x - mu
        v = (c * c).sum(0, dtype=dtype) / mm
        istd = dtype(1) / np.sqrt(v + eps)
        return (c * istd).astype(dtype), istd.astype(dtype)

    a, b = np.asarray(e[:h][valid], dtype=dtype), np.asarray(e[h:2 * h][valid], dtype=dtype)
    ah, ia = normalise(a)
    bh, ib = normalise(b)
    C = ((ah.T @ bh) / mm).astype(dtype)
    eye = np.eye(d, dtype=bool)
    t = dtype(1) - np.diag(C)
    on = (t * t).sum(dtype=dtype)
    off = np.where(eye, dtype(0), C * C).sum(1, dtype=dtype).sum(dtype=dtype)
    G = np.where(eye, dtype(-2) * (dtype(1) - C), dtype(2) * lam * C).astype(dtype)
    dah, dbh = ((bh @ G.T) / mm).astype(dtype), ((ah @ G) / mm).astype(dtype)

    def back(dx, xh, istd):
        return ((dx - dx.sum(0, dtype=dtype) / mm - xh * ((dx * xh).sum(0, dtype=dtype) / mm)) * istd).astype(dtype)

    rows = np.flatnonzero(valid)
    out["grad"][rows] = back(dah, ah, ia)
    out["grad"][rows + h] = back(dbh, bh, ib)
    out.update(loss=float(on + lam * off), on=float(on), off=float(off), mean_diag=float(np.diag(C).sum(dtype=dtype) / dtype(d)), C=C,
               ahat=ah, bhat=bh, istd=np.stack([ia, ib]))
    return out


class BarlowTwinsLoss(_LossModule):
    """The Barlow Twins loss (Zbontar et al., ICML 2021) of (N, d) embeddings whose rows p and p + N // 2 are two views of one image
    (augment.duplicate_views' [x; x] layout), against an (N, 1) column of ids read as a mask (a pair with an id < 0 in either row is out
    of the batch): both views are batch-normalised over the pairs, and their d x d cross-correlation matrix is pushed towards the
    identity, loss = sum_k (1 - C_kk)^2 + lambd sum_{k != l} C_kl^2; `reference_barlow` is the definition.  The loss of
    FusedNet.set_loss(kind="barlow") for the autograd route, by the same kernels, so `loss.backward()` leaves the fused step's d loss /
    d logits bit for bit.  lambd: finite, >= 0; it lives in a one-float tensor (`lambd`) that may be rewritten in place.  There are no
    element losses: elementwise() raises."""
    kind = "barlow"

    def __init__(self, lambd=0.0051):
        super().__init__()
        self.lambd = torch.tensor([check_lambda("BarlowTwinsLoss", lambd)], dtype=torch.float32)
        self._scratch = None

    def _state(self, logits):
        self._on(logits.device, "lambd")
        state = Loss("barlow", False, lambd=self.lambd)
        if self._scratch is not None:
            state._held["scratch"] = self._scratch
        self._scratch = state._scratch(logits)               # (the module keeps it from call to call)
        return state


@torch.no_grad()
def barlow_terms(logits, ids):
    """(on, off, mean_diag, m) of the Barlow Twins loss of these device embeddings (cx_barlow_fwd_bwd's stats): the diagonal term
    sum_k (1 - C_kk)^2, the off-diagonal term sum_{k != l} C_kl^2 without its weight, the mean of the diagonal of C (1 when the two
    views agree in every coordinate) and the pairs in the batch: the monitor of this pretraining, next to contrastive_top1.  logits
    (N, d), ids (N, 1) or (N,).  Floats and an int; zeros where fewer than two pairs are in the batch."""
    x, t = _operands(logits, ids.reshape(-1, 1), "barlow_terms", "barlow")
    stats = torch.empty(4, dtype=torch.float32, device=x.device)
    zero = torch.zeros(1, dtype=torch.float32, device=x.device)               # (the terms do not depend on lambd)
    ops.barlow_fwd_bwd(x, t, zero, None, None, stats)
    on, off, diag, m = stats.tolist()
    return on, off, diag, int(m)
