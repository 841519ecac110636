"""GPU: the AUC-margin loss -- cx_aucm_fwd_bwd and cx_aucm_aux_step against a float64 torch statement of the definition with
autograd, the autograd route (loss.AUCMLoss), FusedNet.set_loss(kind="aucm") in the fused step, under graph replay, through
loss_state() / load_loss_state(), and the command line.

Tolerances are those of the BCE kernels (tests/test_uncertain_gpu.py): the loss within 1e-5 absolute, gradients within 1e-5 of the
largest reference magnitude."""
import json
import math
import os

import pytest
import torch

from chexpert_amd import synth
from eager_step import _eager_dev_step

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    from chexpert_amd import _lib
    _lib.lib()          # fail loudly if the HIP library is missing
    return torch.device("cuda:0")


def close(got, want, rel, what=""):
    """max|diff| / max|ref| < rel, against a reference that is not trivially small."""
    scale = want.abs().max().item()
    err = (got - want).abs().max().item()
    assert scale > 1e-4, "%s: the reference is trivial (max %.3e)" % (what, scale)
    print("%s: max err %.3e vs scale %.3e (rel %.2e)" % (what, err, scale, err / scale))
    assert err / scale < rel, "%s: max err %.3e vs scale %.3e (rel %.2e)" % (what, err, scale, err / scale)


# ------------------------------------------------------------------------------------------------ float64 oracle (as in test_aucm_cpu.py)
def oracle(logits, t, prior, aux, margin):
    """The definition in float64 with autograd: (loss, per-class terms, d loss / d logits, d loss / d aux (3, n)).  Rows are live
    when t >= 0 and positive when t >= 0.5; a class without a live row adds nothing."""
    x = logits.detach().cpu().double().clone().requires_grad_(True)
    t, p = t.detach().cpu().double(), prior.detach().cpu().double()
    a, b, al = (aux.detach().cpu()[i].double().clone().requires_grad_(True) for i in range(3))
    y = torch.sigmoid(x)
    live = (t >= 0).double()
    P, N = live * (t >= 0.5).double(), live * (t < 0.5).double()
    cnt = live.sum(0)
    L = cnt.clamp(min=1)
    inner = p * (1 - p) * margin + (p * y * N - (1 - p) * y * P).sum(0) / L
    lc = (1 - p) * ((y - a) ** 2 * P).sum(0) / L + p * ((y - b) ** 2 * N).sum(0) / L + 2 * al * inner - p * (1 - p) * al ** 2
    lc = lc * (cnt > 0).double()
    lc.sum().backward()
    return lc.sum().detach(), lc.detach(), x.grad, torch.stack([a.grad, b.grad, al.grad])


def oracle_update(aux, daux, lr):
    """a -= lr da, b -= lr db, alpha = max(0, alpha + lr dalpha), float64."""
    aux, daux = aux.detach().cpu().double(), daux.detach().cpu().double()
    return torch.stack([aux[0] - lr * daux[0], aux[1] - lr * daux[1], (aux[2] + lr * daux[2]).clamp(min=0)])


def _targets(seed, B, n, ignored=0.2):
    t = synth.targets(seed, B, n).clone()
    return torch.where(synth.uniform(seed + 3, (B, n), 0.0, 1.0) < ignored, torch.full_like(t, -1.0), t)


def _operands(seed, B, n):
    logits = synth.uniform(seed, (B, n), -6.0, 6.0)
    prior = synth.uniform(seed + 1, (n,), 0.05, 0.6)
    aux = torch.stack([synth.uniform(seed + 2, (n,), -0.5, 1.5), synth.uniform(seed + 3, (n,), -0.5, 1.5), synth.uniform(seed + 4, (n,), 0.0, 2.0)])
    return logits, prior, aux


def _run(dev, logits, t, prior, aux, margin, grad_scale=1.0):
    from chexpert_amd import ops
    B, n = logits.shape
    out = [torch.full((1,), 7.0, device=dev), torch.full((n,), 7.0, device=dev), torch.full((B, n), 7.0, device=dev), torch.full((3, n), 7.0, device=dev)]
    ops.aucm_fwd_bwd(logits.to(dev), t.to(dev), prior.to(dev), aux.to(dev), margin, out[0], out[1], out[2], out[3], grad_scale)
    return out


_SHAPES = [(1, 1), (3, 1), (7, 3), (64, 5), (257, 14), (1024, 5), (5, 300)]      # the last: more classes than one sweep of 256 columns
_cache = {}


def _shape_case(B, n):
    """Operands and the float64 reference of one shape of the table, computed once."""
    if (B, n) not in _cache:
        seed = 2000 + 10 * B + n
        logits, prior, aux = _operands(seed, B, n)
        t = _targets(seed + 10, B, n, ignored=0.0 if B < 7 else 0.2)
        if (B, n) == (1, 1):
            t[0, 0] = 1.0                                # a single positive, no negative
        if (B, n) == (3, 1):
            t[:, 0] = torch.tensor([1.0, 0.0, 0.0])
        if (B, n) == (7, 3):
            t[:, 1] = -1.0                               # one column wholly ignored
        if (B, n) == (1024, 5):
            t[:, 2] = 1.0                                # a column of only positives
        margin = 1.0 if n != 5 else 0.7
        _cache[(B, n)] = (logits, t, prior, aux, margin, oracle(logits, t, prior, aux, margin))
    return _cache[(B, n)]


@pytest.mark.parametrize("B,n", _SHAPES)
def test_kernel_against_float64(dev, B, n):
    from chexpert_amd import ops
    logits, t, prior, aux, margin, (loss_ref, lc_ref, g_ref, daux_ref) = _shape_case(B, n)
    if B >= 64:
        assert (t < 0).any() and (t == 1).any() and (t == 0).any()
    loss, lc, dl, daux = _run(dev, logits, t, prior, aux, margin)
    print("B=%d n=%d loss %.7f ref %.7f diff %.3e" % (B, n, loss.item(), loss_ref.item(), abs(loss.item() - loss_ref.item())))
    assert abs(loss.item() - loss_ref.item()) < 1e-5
    err_c = (lc.cpu().double() - lc_ref).abs().max().item()
    print("per-class terms: max abs err %.3e" % err_c)
    assert err_c < 1e-5
    close(dl.cpu().double(), g_ref, rel=1e-5, what="dlogits")
    close(daux.cpu().double(), daux_ref, rel=1e-5, what="daux")
    ign = t < 0
    assert bool((dl.cpu()[ign] == 0.0).all())
    # the same bits again, and each output is optional: the others do not move
    again = _run(dev, logits, t, prior, aux, margin)
    assert all(torch.equal(u, v) for u, v in zip((loss, lc, dl, daux), again))
    xd, td, pd, ad = logits.to(dev), t.to(dev), prior.to(dev), aux.to(dev)
    loss2, dl2, daux2 = torch.zeros(1, device=dev), torch.zeros(B, n, device=dev), torch.zeros(3, n, device=dev)
    ops.aucm_fwd_bwd(xd, td, pd, ad, margin, loss2, None, None, None)
    assert torch.equal(loss2, loss)
    ops.aucm_fwd_bwd(xd, td, pd, ad, margin, None, None, dl2, None)
    assert torch.equal(dl2, dl)
    ops.aucm_fwd_bwd(xd, td, pd, ad, margin, None, None, None, daux2)
    assert torch.equal(daux2, daux)
    # grad_scale multiplies dlogits alone
    h = _run(dev, logits, t, prior, aux, margin, grad_scale=0.5)
    assert torch.equal(h[0], loss) and torch.equal(h[1], lc) and torch.equal(h[3], daux)
    close(h[2].cpu().double(), 0.5 * g_ref, rel=1e-5, what="dlogits at grad_scale 0.5")
    assert torch.equal(h[2], dl * 0.5)                                  # (a power of two: exact)
    if (B, n) == (7, 3):
        # the wholly ignored class: no loss, no gradient, and the update leaves its scalars' bits alone
        assert aux[2, 1] > 0 and lc[1].item() == 0.0 and bool((dl[:, 1] == 0).all()) and bool((daux[:, 1] == 0).all())
        assert lc_ref[1].item() == 0.0 and bool((daux_ref[:, 1] == 0).all())
        stepped = ad.clone()
        ops.aucm_aux_step(stepped, daux, torch.full((1,), 0.3, device=dev))
        assert torch.equal(stepped[:, 1], ad[:, 1]) and not torch.equal(stepped[:, 0], ad[:, 0]) and not torch.equal(stepped[:, 2], ad[:, 2])
    if (B, n) == (1, 1):
        assert daux[1, 0].item() == 0.0                                 # no negative: nothing pulls b


def test_soft_labels_fall_on_the_side_they_came_from(dev):
    B, n = 16, 3
    logits, prior, aux = _operands(77, B, n)
    hard = synth.targets(78, B, n)
    soft = torch.where(hard > 0.5, torch.full_like(hard, 0.55), torch.full_like(hard, 0.45))
    soft[0], hard[0] = -1.0, -1.0
    assert (soft == 0.55).any() and (soft == 0.45).any()
    a, b = _run(dev, logits, soft, prior, aux, 1.0), _run(dev, logits, hard, prior, aux, 1.0)
    assert all(torch.equal(u, v) for u, v in zip(a, b))
    loss_ref, _, g_ref, daux_ref = oracle(logits, soft, prior, aux, 1.0)
    assert abs(a[0].item() - loss_ref.item()) < 1e-5
    close(a[2].cpu().double(), g_ref, rel=1e-5, what="dlogits (soft labels)")
    close(a[3].cpu().double(), daux_ref, rel=1e-5, what="daux (soft labels)")


def test_aux_step_against_the_oracle_update(dev):
    """The update is three fp32 operations on numbers of the size of aux and lr * daux: each rounds at 2^-24 of its result, so
    3 * 2^-24 of the largest magnitude involved bounds the error (1e-6 with room)."""
    from chexpert_amd import ops
    n, lr = 14, 0.25
    aux = torch.stack([synth.uniform(90, (n,), -1.0, 1.0), synth.uniform(91, (n,), -1.0, 1.0), synth.uniform(92, (n,), 0.0, 0.5)])
    daux = synth.uniform(93, (3, n), -4.0, 4.0)
    aux[2, 3], daux[2, 3] = 0.0, -1.0                                   # the clamp holds this alpha at 0
    aux[2, 4], daux[2, 4] = 0.0, 2.0                                    # ... and lets this one rise
    want = oracle_update(aux, daux, lr)
    assert (want[2] == 0).sum() >= 2 and want[2, 3] == 0 and want[2, 4] == 0.5
    got, lr_dev = aux.to(dev), torch.full((1,), lr, device=dev)
    ops.aucm_aux_step(got, daux.to(dev), lr_dev)
    close(got.cpu().double(), want, rel=1e-6, what="aux after the step")
    assert got[2, 3].item() == 0.0 and bool((got[2] >= 0).all())
    # the rate is read from the device at launch time
    got2 = aux.to(dev)
    ops.aucm_aux_step(got2, daux.to(dev), lr_dev.fill_(0.5))
    close(got2.cpu().double(), oracle_update(aux, daux, 0.5), rel=1e-6, what="aux after the step at the new rate")
    # from the kernel's own gradients
    logits, t, prior, aux5, margin, (_, _, _, daux_ref) = _shape_case(64, 5)
    _, _, _, d5 = _run(dev, logits, t, prior, aux5, margin)
    a5 = aux5.to(dev)
    ops.aucm_aux_step(a5, d5, torch.full((1,), 0.1, device=dev))
    close(a5.cpu().double(), oracle_update(aux5, d5, 0.1), rel=1e-6, what="aux after the step, kernel gradients")


def test_wrappers_check_their_operands(dev):
    from chexpert_amd import ops
    x, t, p, a = torch.zeros(2, 5, device=dev), torch.zeros(2, 5, device=dev), torch.full((5,), 0.3, device=dev), torch.zeros(3, 5, device=dev)
    loss = torch.zeros(1, device=dev)
    with pytest.raises(RuntimeError):
        ops.aucm_fwd_bwd(x, t, p.cpu(), a, 1.0, loss, None, None, None)
    with pytest.raises(RuntimeError, match="invalid argument"):
        ops.aucm_fwd_bwd(x, t, p, a, 0.0, loss, None, None, None)
    for bad in (dict(t=t.double()), dict(p=p[:4]), dict(a=a[:2]), dict(a=a[:, :4]), dict(x=x.t(), t=t.t())):
        k = dict(dict(x=x, t=t, p=p, a=a), **bad)
        with pytest.raises(AssertionError):
            ops.aucm_fwd_bwd(k["x"], k["t"], k["p"], k["a"], 1.0, loss, None, None, None)
    with pytest.raises(AssertionError):
        ops.aucm_fwd_bwd(x, t, p, a, 1.0, loss, None, torch.zeros(2, 4, device=dev), None)
    with pytest.raises(AssertionError):
        ops.aucm_aux_step(a, a[:2], loss)
    with pytest.raises(RuntimeError):
        ops.aucm_aux_step(a, a.clone(), loss.cpu())


# ------------------------------------------------------------------------------------------------ autograd route
def _criterion(dev, prior, aux, margin):
    from chexpert_amd.loss import AUCMLoss
    crit = AUCMLoss(prior, margin).to(dev)
    with torch.no_grad():
        for p_, row in zip((crit.a, crit.b, crit.alpha), aux):
            p_.copy_(row)
    return crit


def test_autograd_route_is_the_fused_kernel(dev):
    logits, t, prior, aux, margin, (loss_ref, _, g_ref, daux_ref) = _shape_case(64, 5)
    loss, _, dl, daux = _run(dev, logits, t, prior, aux, margin)
    crit = _criterion(dev, prior, aux, margin)
    x = logits.to(dev).requires_grad_(True)
    out = crit(x, t.to(dev))
    assert out.dim() == 0 and torch.equal(out.detach(), loss[0])
    out.backward()
    assert torch.equal(x.grad, dl)
    # the module's parameter gradients: the oracle's, with alpha's negated (a descending optimiser ascends on alpha)
    got = torch.stack([crit.a.grad, crit.b.grad, crit.alpha.grad])
    want = daux_ref * torch.tensor([[1.0], [1.0], [-1.0]], dtype=torch.float64)
    close(got.cpu().double(), want, rel=1e-5, what="parameter gradients")
    assert torch.equal(got, daux * torch.tensor([[1.0], [1.0], [-1.0]], device=dev))
    assert float(crit.alpha.grad.abs().max()) > 0
    # backward scales by the incoming gradient
    crit.zero_grad()
    x2 = logits.to(dev).requires_grad_(True)
    (2.0 * crit(x2, t.to(dev))).backward()
    assert torch.equal(x2.grad, dl * 2.0) and torch.equal(crit.a.grad, daux[0] * 2.0)
    # plain SGD on the module's parameters at rate lr, then clamp_(): the fused step's update
    from chexpert_amd import ops
    lr = 0.3
    opt = torch.optim.SGD(crit.parameters(), lr=lr)
    crit.zero_grad()
    crit(logits.to(dev), t.to(dev)).backward()
    opt.step()
    crit.clamp_()
    stepped = aux.to(dev)
    ops.aucm_aux_step(stepped, daux, torch.full((1,), lr, device=dev))
    close(torch.stack([crit.a, crit.b, crit.alpha]).detach().cpu().double(), stepped.cpu().double(), rel=1e-6, what="SGD + clamp_ against the fused update")


# ------------------------------------------------------------------------------------------------ fused step
def _net(kind, dev, seed=3):
    from chexpert_amd.models import Bottleneck, DenseNet, ResNet, construct_model, densenet121
    torch.manual_seed(seed)
    if kind == "densenet121":
        model, S = densenet121(num_classes=5), 64
    elif kind == "densenet":
        model, S = DenseNet(32, (2, 2, 2, 2), 64, num_classes=5), 64
        for n_, p in model.named_parameters():           # well-conditioned regime (tests/test_model_gpu.py)
            if n_.endswith(".bias") and "classifier" not in n_:
                p.data.fill_(2.5)
    elif kind == "resnet":
        model, S = ResNet(Bottleneck, [1, 1, 1, 1], num_classes=5), 64
    else:
        from chexpert_amd.models.efficientnet import DropMarker
        model, S = construct_model("efficientnet-b0", 5), 96
        for mod in model.modules():                      # no dropout / DropConnect draws
            if isinstance(mod, DropMarker):
                mod.p = 0.0
    return model.to(dev).train(), S


def _twin(kind, dev):
    a, S = _net(kind, dev)
    b, _ = _net(kind, dev)
    b.load_state_dict({k: v.clone() for k, v in a.state_dict().items()})
    return a, b, S


_PRIOR = [0.3, 0.1, 0.05, 0.25, 0.4]


def _mixed_targets(seed, B, dev):
    """(B, 5) targets with an ignored label, and a positive and a negative in every class."""
    t = _targets(seed, B, 5, ignored=0.15)
    t[0], t[1] = 1.0, 0.0
    t[2, 0] = -1.0
    return t.to(dev)


def _update_bound(aux_ref, daux_ref, lr):
    """Error allowed in the updated scalars: the gradient tolerance carried through the rate, plus the update's own fp32 roundings."""
    return lr * 1e-5 * daux_ref.abs().max().item() + 3 * 2.0 ** -24 * max(aux_ref.abs().max().item(), 1.0)


def test_fused_step_densenet_equals_the_autograd_route(dev):
    """densenet121 at 64 x 64, B = 4, five classes."""
    a, b, S = _twin("densenet121", dev)
    assert S == 64 and len(list(a.features.denseblock3.children())) == 24 and a.classifier.out_features == 5
    B, margin, lr = 4, 0.8, 0.2
    x = synth.xray_batch(800, B, S).to(dev)
    t = _mixed_targets(810, B, dev)
    keys = list(a.state_dict().keys())
    assert a.set_loss(kind="aucm", prior=_PRIOR, margin=margin, lr_aux=lr) is a
    assert list(a.state_dict().keys()) == keys and not any("loss" in n for n, _ in a.named_buffers())
    assert a.loss_kind == "aucm" and tuple(a.loss_aux.shape) == (3, 5) and bool((a.loss_aux == 0).all())
    assert torch.equal(a.loss_prior.cpu(), torch.tensor(_PRIOR)) and a.loss_lr_aux.tolist() == [torch.tensor(lr).item()]
    aux0 = torch.stack([synth.uniform(820, (5,), 0.0, 1.0), synth.uniform(821, (5,), 0.0, 1.0), synth.uniform(822, (5,), 0.0, 1.0)])
    a.loss_aux.copy_(aux0)
    loss_a, logits_a = a.forward_backward(x, t)
    ref, _, _, daux_ref = oracle(logits_a, t, a.loss_prior, aux0, margin)
    print("fused loss %.7f, float64 oracle on the returned logits %.7f" % (loss_a.item(), ref.item()))
    assert abs(loss_a.item() - ref.item()) < 1e-5
    # the autograd route on a twin with the same weights: the same bits in every gradient
    crit = _criterion(dev, _PRIOR, aux0, margin)
    out = b(x)
    loss_b = crit(out, t)
    loss_b.backward()
    assert torch.equal(loss_a.reshape(()), loss_b.detach()) and torch.equal(logits_a, out.detach())
    ga, gb = dict(a.named_parameters()), dict(b.named_parameters())
    for k in ga:
        assert torch.equal(ga[k].grad, gb[k].grad), k
    assert torch.equal(a._eng().flat_grad, b._eng().flat_grad)
    assert max(float(p.grad.abs().max()) for p in ga.values()) > 0
    # after the step the scalars are the oracle's update
    want = oracle_update(aux0, daux_ref, lr)
    err = (a.loss_aux.cpu().double() - want).abs().max().item()
    bound = _update_bound(want, daux_ref, lr)
    print("loss_aux after the step: max abs err %.3e (bound %.3e)" % (err, bound))
    assert err <= bound and not torch.equal(a.loss_aux.cpu(), aux0)


@pytest.mark.parametrize("kind", ["resnet", "efficientnet"])
def test_fused_step_loss_value_other_families(dev, kind):
    model, S = _net(kind, dev)
    B = 4
    x = synth.xray_batch(830, B, S).to(dev)
    t = _mixed_targets(840, B, dev)
    model.set_loss(kind="aucm", prior=_PRIOR, margin=1.0, lr_aux=0.1)
    aux0 = torch.stack([synth.uniform(850, (5,), 0.0, 1.0), synth.uniform(851, (5,), 0.0, 1.0), synth.uniform(852, (5,), 0.0, 1.0)])
    model.loss_aux.copy_(aux0)
    loss, logits = model.forward_backward(x, t)
    ref, _, _, _ = oracle(logits, t, model.loss_prior, aux0, 1.0)
    print("%s: fused loss %.7f, float64 oracle %.7f" % (kind, loss.item(), ref.item()))
    assert abs(loss.item() - ref.item()) < 1e-5


def test_eval_mode_step_leaves_the_scalars_alone(dev):
    model, S = _net("densenet", dev)
    x, t = synth.xray_batch(860, 4, S).to(dev), _mixed_targets(870, 4, dev)
    model.set_loss(kind="aucm", prior=_PRIOR, lr_aux=0.5)
    model.forward_backward(x, t)                                        # a train-mode step moves them
    held = model.loss_aux.clone()
    assert float(held.abs().max()) > 0
    model.eval()
    model.zero_grad(set_to_none=True)
    loss, _ = model.forward_backward(x, t)                              # the frozen-BatchNorm step: gradients, no update
    assert torch.equal(model.loss_aux, held) and math.isfinite(loss.item())
    assert float(model.classifier.weight.grad.abs().max()) > 0 and float(model._loss_daux.abs().max()) > 0


def test_default_loss_is_untouched_after_a_visit(dev):
    a, b, S = _twin("densenet", dev)
    x, t = synth.xray_batch(880, 4, S).to(dev), synth.targets(890, 4, 5).to(dev)
    a.set_loss(kind="aucm", prior=_PRIOR, lr_aux=0.1)
    la, _ = a.forward_backward(x, t)
    assert a.set_loss() is a and (a.loss_kind, a.loss_ignore_negative, a.loss_pos_weight, a.loss_aux) == ("bce", False, None, None)
    a.zero_grad(set_to_none=True)
    l1, _ = a.forward_backward(x, t)
    l2, _ = b.forward_backward(x, t)                                    # a model that never heard of it
    assert torch.equal(l1, l2) and not torch.equal(l1, la)
    ga, gb = dict(a.named_parameters()), dict(b.named_parameters())
    for k in ga:
        assert torch.equal(ga[k].grad, gb[k].grad), k
    # coming back from another kind the scalars start at zero again, in the storage held before
    a.set_loss(kind="aucm", prior=_PRIOR, lr_aux=0.1)
    assert bool((a.loss_aux == 0).all())
    with pytest.raises(ValueError):
        a.set_loss(kind="aucm", prior=_PRIOR, lr_aux=0.1, pos_weight=[1.0] * 5)


def test_loss_state_round_trip(dev):
    a, S = _net("densenet", dev)
    xs = [synth.xray_batch(900 + i, 4, S).to(dev) for i in range(3)]
    ts = [_mixed_targets(910 + 10 * i, 4, dev) for i in range(3)]
    a.set_loss(kind="aucm", prior=_PRIOR, margin=0.9, lr_aux=0.3)
    for i in range(2):
        a.zero_grad(set_to_none=True)
        a.forward_backward(xs[i], ts[i])
    st = a.loss_state()
    assert set(st) == {"kind", "aux", "prior", "margin", "lr_aux"} and st["kind"] == "aucm" and st["margin"] == 0.9
    assert isinstance(st["lr_aux"], float) and abs(st["lr_aux"] - 0.3) < 1e-7
    assert not st["aux"].is_cuda and not st["prior"].is_cuda and torch.equal(st["aux"], a.loss_aux.cpu()) and float(st["aux"].abs().max()) > 0
    fresh, _ = _net("densenet", dev, seed=11)                           # other weights until the state_dict arrives
    fresh.load_state_dict({k: v.clone() for k, v in a.state_dict().items()})
    assert fresh.load_loss_state(st) is fresh
    assert fresh.loss_kind == "aucm" and fresh.loss_margin == 0.9 and torch.equal(fresh.loss_aux, a.loss_aux)
    assert torch.equal(fresh.loss_prior, a.loss_prior) and torch.equal(fresh.loss_lr_aux, a.loss_lr_aux)
    a.zero_grad(set_to_none=True)
    la, _ = a.forward_backward(xs[2], ts[2])
    lf, _ = fresh.forward_backward(xs[2], ts[2])
    assert torch.equal(la, lf) and torch.equal(a._eng().flat_grad, fresh._eng().flat_grad) and torch.equal(a.loss_aux, fresh.loss_aux)
    # set_loss on a model that holds the loss keeps the trained scalars and their storage, and copies the new values in
    held, ptr = a.loss_aux.clone(), a.loss_aux.data_ptr()
    a.set_loss(kind="aucm", prior=[0.2] * 5, margin=0.9, lr_aux=0.05)
    assert a.loss_aux.data_ptr() == ptr and torch.equal(a.loss_aux, held) and a.loss_prior.tolist() == torch.tensor([0.2] * 5).tolist()


def test_graphed_step_replays_the_loss_and_its_update(dev):
    from chexpert_amd.graph import GraphedTrainStep
    from chexpert_amd.optim import FusedAdam
    m_e, m_g, S = _twin("densenet", dev)
    B = 4
    xs = [synth.xray_batch(920 + i, B, S).to(dev) for i in range(4)]
    ts = [_mixed_targets(930 + 10 * i, B, dev) for i in range(4)]
    for m in (m_e, m_g):
        m.set_loss(kind="aucm", prior=_PRIOR, margin=1.0, lr_aux=0.1)
    opt_e, opt_g = FusedAdam(m_e, lr=1e-3), FusedAdam(m_g, lr=1e-3)
    gs = GraphedTrainStep(m_g, opt_g, xs[0], ts[0])
    assert bool((m_g.loss_aux == 0).all())                              # the capture's warm-up steps are put back
    flat = lambda m: torch.cat([p.detach().flatten() for p in m.parameters()])
    for i in range(3):
        le = _eager_dev_step(m_e, opt_e, xs[i], ts[i])
        lg, _ = gs.replay(xs[i], ts[i])
        assert torch.equal(le, lg), (i, le.item(), lg.item())
        assert torch.equal(flat(m_e), flat(m_g)), i
        assert torch.equal(m_e.loss_aux, m_g.loss_aux) and float(m_g.loss_aux.abs().max()) > 0, i
    # the rate changes in place: the captured step reads the new value
    before = m_g.loss_aux.clone()
    m_g.loss_lr_aux.fill_(0.5)
    m_e.set_loss(kind="aucm", prior=_PRIOR, margin=1.0, lr_aux=0.5)    # same kind, same n: copied into the held storage
    assert torch.equal(m_e.loss_aux, before)
    le = _eager_dev_step(m_e, opt_e, xs[3], ts[3])
    lg, _ = gs.replay(xs[3], ts[3])
    assert torch.equal(le, lg) and torch.equal(flat(m_e), flat(m_g)) and torch.equal(m_e.loss_aux, m_g.loss_aux)
    d = m_g._loss_daux
    new, old = before[:2] - 0.5 * d[:2], before[:2] - 0.1 * d[:2]
    assert float((m_g.loss_aux[:2] - new).abs().max()) * 100 < float((m_g.loss_aux[:2] - old).abs().max())


# ------------------------------------------------------------------------------------------------ command line
def _losses(capsys):
    out = capsys.readouterr().out
    return [json.loads(l)["train_loss"] for l in out.splitlines() if l.startswith('{"step"')]


_CLI = ["--train", "--batch_size", "4", "--resize", "64", "--log_interval", "1", "--seed", "3", "--loss", "aucm", "--aucm_margin", "0.8",
        "--lr", "0.001"]


def test_cli_graphed_run_checkpoints_and_restores(dev, tmp_path, capsys):
    from chexpert_amd import cli
    base = _CLI + ["--synthetic", "32", "--eval_interval", "8", "--fused_optimizer"]
    capsys.readouterr()
    out = str(tmp_path / "g")
    model = cli.main(base + ["--graph", "--aucm_lr_aux", "0.05", "--output_dir", out])
    lg = _losses(capsys)
    assert len(lg) == 8 and all(math.isfinite(v) for v in lg), lg
    cfg = json.load(open(os.path.join(out, "config.json")))
    ds = cli.SyntheticXrays(32, 64, 5, 7)
    assert cfg["loss"] == "aucm" and cfg["aucm_prior"] is None and cfg["aucm_prior_resolved"] == cli.resolve_aucm_prior(None, ds.targets, 5)
    st = torch.load(os.path.join(out, "checkpoint_latest.pt"), map_location="cpu")["loss_state"]
    assert st["kind"] == "aucm" and st["margin"] == 0.8 and abs(st["lr_aux"] - 0.05) < 1e-7 and float(st["aux"].abs().max()) > 1e-3
    assert torch.equal(st["aux"], model.loss_aux.cpu()) and st["prior"].tolist() == torch.tensor(cfg["aucm_prior_resolved"]).tolist()
    res = json.load(open(os.path.join(out, "eval_results_step_8.json")))
    assert len(res["aucs"]) == 5 and all(math.isfinite(v) for v in res["loss"].values())      # evaluation keeps the BCE element losses
    # --restore continues from the checkpoint's scalars; this run's flags keep the last word on the rate: at a rate of 1e-9 eight
    # more steps leave them where the checkpoint had them (1e-9 * 8 gradients of order 1), which a start from zero would not
    out2 = str(tmp_path / "r")
    model2 = cli.main(base + ["--aucm_lr_aux", "1e-9", "--restore", os.path.join(out, "checkpoint_latest.pt"), "--output_dir", out2])
    lr_ = _losses(capsys)
    assert len(lr_) == 8 and all(math.isfinite(v) for v in lr_), lr_
    assert abs(model2.loss_lr_aux.item() - 1e-9) < 1e-15
    assert float((model2.loss_aux.cpu() - st["aux"]).abs().max()) < 1e-6
    st2 = torch.load(os.path.join(out2, "checkpoint_latest.pt"), map_location="cpu")
    assert st2["global_step"] == 16 and st2["loss_state"]["kind"] == "aucm"


def test_cli_autograd_route(dev, tmp_path, capsys):
    """Without --fused_optimizer the loss module trains its scalars under plain SGD at the auxiliary rate; the checkpoint reads them
    back through the model's loss state."""
    from chexpert_amd import cli
    capsys.readouterr()
    out = str(tmp_path / "e")
    model = cli.main(_CLI + ["--synthetic", "16", "--eval_interval", "4", "--aucm_lr_aux", "0.05", "--output_dir", out])
    le = _losses(capsys)
    assert len(le) == 4 and all(math.isfinite(v) for v in le), le
    st = torch.load(os.path.join(out, "checkpoint_latest.pt"), map_location="cpu")["loss_state"]
    assert st["kind"] == "aucm" and float(st["aux"].abs().max()) > 1e-3 and bool((st["aux"][2] >= 0).all())
    assert torch.equal(st["aux"], model.loss_aux.cpu())
