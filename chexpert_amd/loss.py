"""The training loss with uncertain-label handling outside the fused step: `loss = MaskedBCE(w)(model(x), t); loss.backward()` and
the element losses of an evaluation run the arithmetic of `FusedNet.set_loss` (cx_bce_masked_fwd_bwd, csrc/elementwise.hip), so
the autograd route and the fused step agree bit for bit.  Device tensors only: there is no CPU path."""
import torch
import torch.nn as nn

from . import ops


def _operands(logits, target):
    if not logits.is_cuda:
        raise RuntimeError("MaskedBCE runs on the GPU only (cx_bce_masked_fwd_bwd); there is no CPU fallback")
    if logits.dim() != 2 or tuple(target.shape) != tuple(logits.shape):
        raise RuntimeError("MaskedBCE takes (B, n) logits and targets of one shape (got %s and %s)" % (tuple(logits.shape), tuple(target.shape)))
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
