"""The training loss with uncertain-label handling outside the fused step: `loss = MaskedBCE(w)(model(x), t); loss.backward()` and
the element losses of an evaluation run the arithmetic of `FusedNet.set_loss` (cx_bce_masked_fwd_bwd, csrc/elementwise.hip), so
the autograd route and the fused step agree bit for bit.  AUCMLoss is the same for `FusedNet.set_loss(kind="aucm")`: the AUC
min-max-margin loss (cx_aucm_fwd_bwd, csrc/aucm.hip) with its auxiliary scalars as parameters.  FocalLoss and AsymmetricLoss are
the same for `FusedNet.set_loss(kind="focal" | "asl")` (cx_asl_fwd_bwd, csrc/focal.hip).  Device tensors only: there is no CPU
path."""
import torch
import torch.nn as nn

from . import ops


def _operands(logits, target, who="MaskedBCE", kernel="cx_bce_masked_fwd_bwd"):
    if not logits.is_cuda:
        raise RuntimeError("%s runs on the GPU only (%s); there is no CPU fallback" % (who, kernel))
    if logits.dim() != 2 or tuple(target.shape) != tuple(logits.shape):
        raise RuntimeError("%s takes (B, n) logits and targets of one shape (got %s and %s)" % (who, tuple(logits.shape), tuple(target.shape)))
    return logits.detach().contiguous().float(), target.detach().contiguous().float()


class _MaskedBCEFn(torch.autograd.Function):
    """loss and d loss / d logits in one launch; backward scales the stored gradient."""

    @staticmethod
    def forward(ctx, logits, target, pos_weight, masked):
        x, t = _operands(logits, target)
        loss = torch.empty(1, dtype=torch.float32, device=x.device)
        dl = torch.empty_like(x)
        if masked:
            ops.bce_masked_fwd_bwd(x, t, pos_weight, loss, None, dl)
        else:
            ops.bce_fwd_bwd(x, t, loss, None, dl)
        ctx.save_for_backward(dl)
        ctx.in_dtype = logits.dtype
        return loss[0]

    @staticmethod
    def backward(ctx, grad_output):
        dl, = ctx.saved_tensors
        return (dl * grad_output).to(ctx.in_dtype), None, None, None


class MaskedBCE(nn.Module):
    """BCEWithLogitsLoss(pos_weight)(logits, target) summed over the classes and averaged over the batch (chexpert.py:160), in which
    a target < 0 is ignored (no loss, no gradient; the divisor stays the batch size).  The two options select the kernel exactly
    as FusedNet.set_loss does: with ignore_negative or a pos_weight it is cx_bce_masked_fwd_bwd, which skips every target < 0 (the
    weighted loss has no arithmetic for a negative target, so pos_weight implies the skipping); with neither it is the plain
    cx_bce_fwd_bwd, to which a negative target is a number like any other, as it is to torch's BCEWithLogitsLoss."""

    def __init__(self, pos_weight=None, ignore_negative=True):
        super().__init__()
        self.ignore_negative = bool(ignore_negative)
        # a plain attribute like FusedNet.set_loss's: moved by hand (`.to` of the module leaves it), never in a state_dict
        self.pos_weight = None if pos_weight is None else torch.as_tensor(pos_weight, dtype=torch.float32).reshape(-1)

    @property
    def masked(self):
        return self.ignore_negative or self.pos_weight is not None

    def _weight(self, device):
        if self.pos_weight is not None and self.pos_weight.device != device:
            self.pos_weight = self.pos_weight.to(device)
        return self.pos_weight

    def forward(self, logits, target):
        return _MaskedBCEFn.apply(logits, target, self._weight(logits.device), self.masked)

    @torch.no_grad()
    def elementwise(self, logits, target):
        """The (B, n) element losses (0 where ignored), outside autograd."""
        x, t = _operands(logits, target)
        out = torch.empty_like(x)
        if self.masked:
            ops.bce_masked_fwd_bwd(x, t, self._weight(x.device), None, out, None)
        else:
            ops.bce_fwd_bwd(x, t, None, out, None)
        return out


class _AUCMFn(torch.autograd.Function):
    """loss, d loss / d logits and the three auxiliary gradients in one launch; backward scales the stored gradients."""

    @staticmethod
    def forward(ctx, logits, target, a, b, alpha, prior, margin):
        x, t = _operands(logits, target, "AUCMLoss", "cx_aucm_fwd_bwd")
        aux = torch.stack([a.detach(), b.detach(), alpha.detach()]).float().contiguous()
        loss = torch.empty(1, dtype=torch.float32, device=x.device)
        dl, daux = torch.empty_like(x), torch.empty_like(aux)
        ops.aucm_fwd_bwd(x, t, prior, aux, margin, loss, None, dl, daux)
        ctx.save_for_backward(dl, daux)
        ctx.in_dtype = logits.dtype
        return loss[0]

    @staticmethod
    def backward(ctx, grad_output):
        dl, daux = ctx.saved_tensors
        # alpha is the dual variable: the saddle point is a minimum in (w, a, b) and a maximum in alpha, so its gradient leaves
        # negated and the optimiser that descends on every parameter ascends on alpha
        return (dl * grad_output).to(ctx.in_dtype), None, daux[0] * grad_output, daux[1] * grad_output, -daux[2] * grad_output, None, None


class AUCMLoss(nn.Module):
    """The AUC min-max-margin loss (Yuan et al., "Large-scale Robust Deep AUC Maximization", ICCV 2021) of (B, n) logits, summed
    over the classes: the loss of FusedNet.set_loss(kind="aucm") for the autograd route, by the same kernel, so `loss.backward()`
    leaves the fused step's d loss / d logits bit for bit.  prior: n class positive rates in (0, 1); margin > 0.  A target < 0 is
    ignored, a target >= 0.5 counts as a positive, the rest as negatives.

    The auxiliary scalars a, b, alpha are nn.Parameters of THIS module (shape (n,), zero at first): hand them to an optimiser
    beside the network's.  The problem is a saddle point -- minimise over the network, a and b, maximise over alpha >= 0 -- so
    backward returns alpha's gradient NEGATED: `alpha.grad` is -d loss / d alpha, and a descending optimiser ascends on alpha.
    Call clamp_() after each optimiser step to keep alpha >= 0 (plain SGD with rate lr_aux followed by clamp_() is the update
    FusedNet.forward_backward makes).  There are no element losses: elementwise() raises."""

    def __init__(self, prior, margin=1.0):
        super().__init__()
        p = torch.as_tensor(prior, dtype=torch.float32).detach().reshape(-1).cpu()
        if p.numel() < 1 or not bool(((p > 0) & (p < 1)).all()):
            raise ValueError("AUCMLoss takes class priors in (0, 1) (got %s)" % p.tolist())
        if not float(margin) > 0:
            raise ValueError("AUCMLoss takes a margin > 0 (got %r)" % (margin,))
        self.margin = float(margin)
        self.prior = p                       # a plain attribute, moved by hand like MaskedBCE.pos_weight
        self.a, self.b, self.alpha = (nn.Parameter(torch.zeros(p.numel())) for _ in range(3))

    def forward(self, logits, target):
        if self.prior.device != logits.device:
            self.prior = self.prior.to(logits.device)
        if self.a.device != logits.device:
            raise RuntimeError("AUCMLoss: a, b and alpha are on %s, the logits on %s -- call loss.to(device)" % (self.a.device, logits.device))
        if logits.dim() == 2 and logits.shape[1] != self.prior.numel():
            raise RuntimeError("AUCMLoss holds %d classes, the logits have %d" % (self.prior.numel(), logits.shape[1]))
        return _AUCMFn.apply(logits, target, self.a, self.b, self.alpha, self.prior, self.margin)

    @torch.no_grad()
    def clamp_(self):
        """alpha >= 0, after an optimiser step.  Returns self."""
        self.alpha.clamp_(min=0)
        return self

    def elementwise(self, logits, target):
        raise RuntimeError("AUCMLoss has no element losses: it is a function of each class's whole batch column (its positives "
                           "against its negatives), not a sum over elements -- evaluate with MaskedBCE.elementwise or BCEWithLogitsLoss")


class _FocusFn(torch.autograd.Function):
    """loss and d loss / d logits in one launch (cx_asl_fwd_bwd); backward scales the stored gradient."""

    @staticmethod
    def forward(ctx, logits, target, pos_weight, focus, who):
        x, t = _operands(logits, target, who, "cx_asl_fwd_bwd")
        loss = torch.empty(1, dtype=torch.float32, device=x.device)
        dl = torch.empty_like(x)
        ops.asl_fwd_bwd(x, t, pos_weight, focus, loss, None, dl)
        ctx.save_for_backward(dl)
        ctx.in_dtype = logits.dtype
        return loss[0]

    @staticmethod
    def backward(ctx, grad_output):
        dl, = ctx.saved_tensors
        return (dl * grad_output).to(ctx.in_dtype), None, None, None, None


class _FocusLoss(nn.Module):
    """What FocalLoss and AsymmetricLoss share: the four numbers [gamma+, gamma-, clip, alpha or -1] the kernel reads from the device
    (`focus`, a plain attribute like `pos_weight`, moved by hand), the autograd route and the element losses."""

    def __init__(self, focus, pos_weight):
        super().__init__()
        gp, gn, m, al = (float(v) for v in focus)
        who = type(self).__name__
        if not (0 <= gp < float("inf") and 0 <= gn < float("inf")):
            raise ValueError("%s takes finite exponents >= 0 (got %r, %r)" % (who, gp, gn))
        if not 0 <= m < 1:
            raise ValueError("%s takes a clip in [0, 1) (got %r)" % (who, m))
        self.focus = torch.tensor([gp, gn, m, al], dtype=torch.float32)
        self.pos_weight = None if pos_weight is None else torch.as_tensor(pos_weight, dtype=torch.float32).detach().reshape(-1)
        if self.pos_weight is not None and not bool(((self.pos_weight > 0) & torch.isfinite(self.pos_weight)).all()):
            raise ValueError("%s takes finite pos_weight > 0 (got %s)" % (who, self.pos_weight.tolist()))

    def _held(self, device):
        if self.focus.device != device:
            self.focus = self.focus.to(device)
        if self.pos_weight is not None and self.pos_weight.device != device:
            self.pos_weight = self.pos_weight.to(device)
        return self.pos_weight, self.focus

    def forward(self, logits, target):
        _operands(logits, target, type(self).__name__, "cx_asl_fwd_bwd")      # (refuses a CPU tensor before anything is moved)
        w, focus = self._held(logits.device)
        return _FocusFn.apply(logits, target, w, focus, type(self).__name__)

    @torch.no_grad()
    def elementwise(self, logits, target):
        """The (B, n) element losses (0 where ignored, and for a hard negative at or below the clip), outside autograd."""
        x, t = _operands(logits, target, type(self).__name__, "cx_asl_fwd_bwd")
        w, focus = self._held(x.device)
        out = torch.empty_like(x)
        ops.asl_fwd_bwd(x, t, w, focus, None, out, None)
        return out


class FocalLoss(_FocusLoss):
    """The focal loss (Lin et al., "Focal Loss for Dense Object Detection", ICCV 2017) of (B, n) logits: torchvision's
    sigmoid_focal_loss(alpha, gamma) summed over the classes and averaged over the batch, a target < 0 ignored (the divisor stays the
    batch size), soft targets valid, pos_weight on the positive term -- the loss of FusedNet.set_loss(kind="focal") for the autograd
    route, by the same kernel, so `loss.backward()` leaves the fused step's d loss / d logits bit for bit.  gamma >= 0; alpha None
    (no class balance) or in (0, 1).  The focusing weight is differentiated, not detached."""

    def __init__(self, gamma=2.0, alpha=None, pos_weight=None):
        if alpha is not None and not 0 < float(alpha) < 1:
            raise ValueError("FocalLoss takes alpha None or in (0, 1) (got %r)" % (alpha,))
        super().__init__([gamma, gamma, 0.0, -1.0 if alpha is None else alpha], pos_weight)


class AsymmetricLoss(_FocusLoss):
    """The asymmetric loss (Ridnik et al., "Asymmetric Loss for Multi-Label Classification", ICCV 2021) of (B, n) logits, timm's
    AsymmetricLossMultiLabel (its blended form for soft targets) summed over the classes and averaged over the batch: positives
    -(1 - p)^gamma_pos log p, negatives -p_m^gamma_neg log(1 - p_m) with p_m = max(p - clip, 0), so a hard negative with p <= clip
    adds no loss and no gradient.  A target < 0 is ignored; pos_weight weights the positive term.  The loss of
    FusedNet.set_loss(kind="asl") for the autograd route, by the same kernel, bit for bit."""

    def __init__(self, gamma_pos=0.0, gamma_neg=4.0, clip=0.05, pos_weight=None):
        super().__init__([gamma_pos, gamma_neg, clip, -1.0], pos_weight)
