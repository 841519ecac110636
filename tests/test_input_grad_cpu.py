"""CPU: the host side of the input gradient (x.grad) through the fused networks -- the new C ABI entry point is declared and bound
with the header's parameter count, and the routing of model.forward into the autograd functions."""
import os
import re

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_stem_input_grad_is_declared_and_bound():
    from chexpert_amd import _lib
    hdr = open(os.path.join(ROOT, "include", "chexpert_hip.h")).read()
    m = re.search(r"int cx_stem_input_grad\(([^)]*)\);", hdr)
    assert m, "cx_stem_input_grad is not declared in include/chexpert_hip.h"
    assert len(_lib.SIGNATURES["cx_stem_input_grad"]) == len(m.group(1).split(",")) == 21
    assert "stem_dgrad.hip" in open(os.path.join(ROOT, "chexpert_amd", "csrc", "Makefile")).read()


def _nets():
    from chexpert_amd.models import BasicBlock, Bottleneck, DenseNet, ResNet, WideResNet, construct_model
    return [DenseNet(32, (2, 2, 2, 2), 64, num_classes=5), DenseNet(12, (6, 6, 6), 24, num_classes=5),
            ResNet(Bottleneck, [1, 1, 1, 1], num_classes=5), WideResNet(BasicBlock, 16, 4, num_classes=5),
            construct_model("efficientnet-b0", 5)]


@pytest.mark.parametrize("i", range(5))
def test_frozen_model_with_a_requires_grad_input_routes_into_autograd(i):
    from chexpert_amd.models._fused import wants_autograd
    model = _nets()[i].train()
    x = torch.zeros(2, 3, 32, 32)
    assert wants_autograd(model, x)                       # parameters require grad (as before)
    for p in model.parameters():
        p.requires_grad_(False)
    assert not wants_autograd(model, x)                   # all frozen, plain input: the engine's own forward (as before)
    assert wants_autograd(model, x.clone().requires_grad_(True))
    with torch.no_grad():
        assert not wants_autograd(model, x.clone().requires_grad_(True))
    assert not wants_autograd(model.eval(), x.clone().requires_grad_(True))   # eval mode stays as it is


def test_forward_routes_through_wants_autograd():
    import inspect
    from chexpert_amd.models._fused import FusedNet
    assert "wants_autograd(self, x)" in inspect.getsource(FusedNet.forward)
    for net in _nets():                                   # one forward / forward_backward for every network
        assert isinstance(net, FusedNet)
        for name in ("forward", "forward_backward"):
            assert getattr(type(net), name) is getattr(FusedNet, name), (type(net).__name__, name)


@pytest.mark.parametrize("i", range(5))
def test_bind_flattens_fp32_masters(i):
    """eng.bind: every parameter becomes a view of the flat fp32 buffer at a 16-byte aligned offset and keeps its values, the
    gradient views alias the flat gradient buffer, and a parameter that is not fp32 is refused."""
    model = _nets()[i]
    before = [p.detach().clone() for p in model.parameters()]
    eng = model._eng()
    eng.bind(torch.device("cpu"))
    params = list(model.parameters())
    assert len(params) == len(eng.grad_views) == len(before)
    base, gbase = eng.flat.data_ptr(), eng.flat_grad.data_ptr()
    for p, g, b in zip(params, eng.grad_views, before):
        off = p.data_ptr() - base
        assert p.untyped_storage().data_ptr() == eng.flat.untyped_storage().data_ptr() and p.dtype == torch.float32
        assert 0 <= off and off % 16 == 0 and off // 4 + p.numel() <= eng.flat.numel()
        assert torch.equal(p.detach(), b)
        assert g.untyped_storage().data_ptr() == eng.flat_grad.untyped_storage().data_ptr()
        assert g.shape == p.shape and g.data_ptr() - gbase == off
    model = _nets()[i]
    p = next(model.parameters())
    p.data = p.data.to(torch.bfloat16)
    with pytest.raises(RuntimeError, match="fp32"):
        model._eng().bind(torch.device("cpu"))


def test_params_untouched_restores_every_grad():
    from chexpert_amd.models._fused import params_untouched
    flat = torch.arange(6, dtype=torch.float32)
    a, b = torch.nn.Parameter(torch.zeros(2)), torch.nn.Parameter(torch.zeros(4))
    a.grad = flat[:2]                                      # a view of the flat buffer
    with params_untouched([a, b], flat):
        assert a.grad is None and b.grad is None
        flat.fill_(-1.0)                                   # the engine writes its weight gradients
        a.grad, b.grad = flat[:2], flat[2:]
    assert torch.equal(a.grad, torch.tensor([0.0, 1.0])) and b.grad is None


def test_input_grad_buffer_checks():
    from chexpert_amd.models._fused import check_input_grad, input_grad_buffer
    x = torch.zeros(2, 3, 8, 8)
    check_input_grad(torch.zeros(2, 3, 8, 8), x)
    for bad in (torch.zeros(2, 3, 8, 8, dtype=torch.float16), torch.zeros(2, 3, 8, 9), torch.zeros(2, 3, 8, 16)[..., ::2]):
        with pytest.raises(RuntimeError):
            check_input_grad(bad, x)
    assert input_grad_buffer((2, 3, 8, 8), torch.device("cpu")).shape == (2, 3, 8, 8)
    with pytest.raises(RuntimeError):
        input_grad_buffer((2, 1, 8, 8), torch.device("cpu"))
