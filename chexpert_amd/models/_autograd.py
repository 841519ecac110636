"""What the three fused networks' autograd functions share for the input gradient (x.grad)."""
import contextlib

import torch


def wants_autograd(model, x):
    """model.forward routes through the autograd function when a train-mode step under grad mode needs a backward: some parameter
    requires a gradient, or the input does (x.grad with every parameter frozen: saliency maps, adversarial examples)."""
    return model.training and torch.is_grad_enabled() and (x.requires_grad or any(p.requires_grad for p in model.parameters()))


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
