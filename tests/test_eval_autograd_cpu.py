"""CPU: the host side of autograd through the fused networks in eval mode (frozen BatchNorm) -- the routing predicate of
model.forward and the frozen-statistics coefficient entry point's declaration and binding."""
import inspect
import os
import re

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_bn_bwd_coef_eval_is_declared_and_bound():
    from chexpert_amd import _lib
    hdr = open(os.path.join(ROOT, "include", "chexpert_hip.h")).read()
    m = re.search(r"int cx_bn_bwd_coef_eval\(([^)]*)\);", hdr)
    assert m, "cx_bn_bwd_coef_eval is not declared in include/chexpert_hip.h"
    assert len(_lib.SIGNATURES["cx_bn_bwd_coef_eval"]) == len(m.group(1).split(",")) == 22
    assert "cx_bn_bwd_coef_eval" in open(os.path.join(ROOT, "chexpert_amd", "csrc", "elementwise.hip")).read()


def _nets():
    from chexpert_amd.models import BasicBlock, Bottleneck, DenseNet, ResNet, WideResNet, construct_model
    return [DenseNet(32, (2, 2, 2, 2), 64, num_classes=5), DenseNet(12, (6, 6, 6), 24, num_classes=5),
            ResNet(Bottleneck, [1, 1, 1, 1], num_classes=5), WideResNet(BasicBlock, 16, 4, num_classes=5),
            construct_model("efficientnet-b0", 5)]


@pytest.mark.parametrize("i", range(5))
def test_eval_routing_truth_table(i):
    from chexpert_amd.models._fused import wants_autograd, wants_eval_autograd
    model = _nets()[i].eval()
    x = torch.zeros(2, 3, 32, 32)
    xg = x.clone().requires_grad_(True)
    assert wants_eval_autograd(model, x)                  # eval, grad mode, parameters requiring grad
    assert not wants_autograd(model, x)                   # (the train-mode predicate is unchanged)
    with torch.no_grad():
        assert not wants_eval_autograd(model, x)          # no_grad: the plain eval forward
        assert not wants_eval_autograd(model, xg)
    for p in model.parameters():
        p.requires_grad_(False)
    assert not wants_eval_autograd(model, x)              # all frozen, plain input: the plain eval forward
    assert wants_eval_autograd(model, xg)                 # all frozen, x.requires_grad: x.grad only
    model.train()
    assert not wants_eval_autograd(model, xg)             # train mode: wants_autograd's business
    assert wants_autograd(model, xg)


def test_eval_routing_leaves_grad_cam_hooks_on_their_path():
    from chexpert_amd.models._fused import FusedNet, wants_eval_autograd
    model = _nets()[0].eval()
    x = torch.zeros(2, 3, 32, 32)
    h = model.features.norm5.register_forward_hook(lambda *a: None)
    assert not wants_eval_autograd(model, x)              # Grad-CAM hooks keep hooked_eval_forward
    h.remove()
    assert wants_eval_autograd(model, x)
    src = inspect.getsource(FusedNet.forward)
    assert "wants_autograd(self, x)" in src
    assert src.index("hooks_registered(self)") < src.index("wants_eval_autograd(self, x)")


def test_eval_backward_refuses_an_unrecorded_forward():
    """An eval forward that did not record what backward reads (record=False) cannot be differentiated."""
    from chexpert_amd.models._fused import FusedEngine
    eng = FusedEngine(torch.nn.Linear(2, 2))
    ws = type("WS", (), {})()
    FusedEngine.recorded(ws, False, False)
    assert ws.frozen and not ws.recorded
    with pytest.raises(RuntimeError, match="record"):
        eng.backward(ws, torch.zeros(1, 1))
    FusedEngine.recorded(ws, False, True)
    assert ws.frozen and ws.recorded
    FusedEngine.recorded(ws, True, False)
    assert not ws.frozen and ws.recorded
