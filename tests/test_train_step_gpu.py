"""GPU: optimizer.train_step (optim._Flat.train_step) against the step written out by hand, bit for bit over three steps.  The
captured side -- a graph replay of train_step against the same hand-written step -- is what the graph-against-eager tests of the
loss, head and pooling files check."""
import pytest
import torch

from chexpert_amd import synth
from eager_step import _eager_dev_step

pytestmark = pytest.mark.gpu

B, S, N_CLS = 4, 64, 5


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    from chexpert_amd import _lib
    _lib.lib()
    return torch.device("cuda:0")


def _twin(dev):
    """Two DenseNets with the same weights, in the well-conditioned regime of tests/test_model_gpu.py."""
    from chexpert_amd.models import DenseNet
    from oracle import nets
    cfg = (2, 2, 2, 2)
    sd = synth.fill_state_dict_(nets.zeros_state_dict(nets.densenet_spec(N_CLS, block_config=cfg)), 21)
    for k in sd:
        if k.endswith(".bias") and "classifier" not in k:
            sd[k] = torch.full_like(sd[k], 2.5)
        if k.endswith(".weight") and sd[k].dim() == 1:
            sd[k] = synth.uniform(7, sd[k].shape, 0.8, 1.2)
    out = []
    for _ in range(2):
        m = DenseNet(32, cfg, 64, num_classes=N_CLS)
        m.load_state_dict(sd)
        out.append(m.to(dev).train())
    return out


def _batches(dev):
    return [(synth.xray_batch(4100 + i, B, S).to(dev), synth.targets(4110 + i, B, N_CLS).to(dev)) for i in range(3)]


def _same(m_a, m_b, what):
    flat = lambda m: torch.cat([p.detach().flatten() for p in m.parameters()])                               # noqa: E731
    assert torch.equal(flat(m_a), flat(m_b)), what
    assert torch.equal(m_a._eng().flat_grad, m_b._eng().flat_grad), what


def test_train_step_dev_equals_the_hand_written_device_step(dev):
    from chexpert_amd.optim import FusedAdam
    m_a, m_b = _twin(dev)
    opt_a, opt_b = FusedAdam(m_a, lr=1e-2), FusedAdam(m_b, lr=1e-2)
    w0 = m_a.classifier.weight.detach().clone()
    for i, (x, t) in enumerate(_batches(dev)):
        la, logits = opt_a.train_step(m_a, x, t, dev=True)
        assert m_a._eng().packed_version is None and logits.shape == (B, N_CLS)
        lb = _eager_dev_step(m_b, opt_b, x, t)
        assert torch.equal(la, lb), (i, la.item(), lb.item())
        _same(m_a, m_b, i)
    opt_a.sync_from_device()
    opt_b.sync_from_device()
    assert opt_a.step_count == opt_b.step_count == 3
    assert not torch.equal(m_a.classifier.weight.detach(), w0)


def test_train_step_host_equals_zero_grad_forward_backward_step(dev):
    from chexpert_amd.optim import FusedAdam
    m_a, m_b = _twin(dev)
    opt_a, opt_b = FusedAdam(m_a, lr=1e-2), FusedAdam(m_b, lr=1e-2)
    w0 = m_a.classifier.weight.detach().clone()
    for i, (x, t) in enumerate(_batches(dev)):
        la, _ = opt_a.train_step(m_a, x, t)
        opt_b.zero_grad()
        lb, _ = m_b.forward_backward(x, t)
        opt_b.step()
        assert torch.equal(la, lb), (i, la.item(), lb.item())
        _same(m_a, m_b, i)
    assert opt_a.step_count == opt_b.step_count == 3
    assert not torch.equal(m_a.classifier.weight.detach(), w0)
