"""GPU: the U-MultiClass policy -- cx_mc3_fwd_bwd against the float64 oracle (shared with tests/test_multiclass_cpu.py, which checks it
against central differences and F.cross_entropy), its confident elements one by one, cx_mc3_collapse, FusedNet.set_loss(kind="multiclass")
in the fused step against the autograd route, under graph replay and data-parallel, and the command line."""
import json
import math
import os
import time

import pytest
import torch

from chexpert_amd import synth
from eager_step import _eager_dev_step

pytestmark = pytest.mark.gpu

TARGET_OF_CLASS = {0: 0.0, 1: 1.0, 2: -1.0}


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    from chexpert_amd import _lib
    _lib.lib()          # fail loudly if the HIP library is missing
    return torch.device("cuda:0")


def close(got, want, rel, what=""):
    """The bound of tests/test_kernels_gpu.py: max error against the largest reference magnitude."""
    scale = want.abs().max().item() + 1e-6
    err = (got - want).abs().max().item()
    print("%s: max err %.3e vs scale %.3e (rel %.2e)" % (what, err, scale, err / scale))
    assert err <= rel * scale, "%s: max err %.3e vs scale %.3e (rel %.2e)" % (what, err, scale, err / scale)


def _targets(seed, B, n, uncertain=0.25):
    """Hard Bernoulli(0.3) labels, a share `uncertain` of them replaced by -1."""
    t = synth.targets(seed, B, n).clone()
    return torch.where(synth.uniform(seed + 3, (B, n), 0.0, 1.0) < uncertain, torch.full_like(t, -1.0), t)


# ------------------------------------------------------------------------------------------------ float64 oracle (as in test_multiclass_cpu.py)
def classes_of(t):
    """2 where t < 0, 1 where t >= 0.5, else 0."""
    return torch.where(t < 0, 2, torch.where(t >= 0.5, 1, 0))


def _elem64(x, c, w):
    """-log softmax_c of every triple, float64, differentiable: logsumexp(z) - z_c, times w[k][c]."""
    B, n = c.shape
    z = x.view(B, n, 3)
    le = torch.logsumexp(z, 2) - z.gather(2, c[..., None])[..., 0]
    return le if w is None else le * w[torch.arange(n)[None].expand(B, n), c]


def oracle(logits, t, w):
    """(loss, element losses (B, n), d loss / d logits (B, 3n)) by autograd in float64; loss = sum of elements / B."""
    x = logits.double().clone().requires_grad_(True)
    le = _elem64(x, classes_of(t), None if w is None else w.double())
    loss = le.sum() / x.shape[0]
    loss.backward()
    return loss.detach(), le.detach(), x.grad


def confident_case(c, B=64, n=5):
    """Every element's class is c and its logit leads the other two by gaps uniform in [4, 12]; the leading logit itself is uniform in
    +-8, so its magnitude is what a cancelling form loses digits against."""
    zc = synth.uniform(61 + c, (B, n), -8.0, 8.0)
    rest = [zc - synth.uniform(71 + c, (B, n), 4.0, 12.0), zc - synth.uniform(81 + c, (B, n), 4.0, 12.0)]
    z = torch.stack([zc if j == c else rest.pop(0) for j in range(3)], 2)
    return z.reshape(B, 3 * n).contiguous(), torch.full((B, n), TARGET_OF_CLASS[c])


# ------------------------------------------------------------------------------------------------ kernels
def _kernel_case(B, n):
    """Logits uniform in +-8; targets drawn from -1, 0, 1 and the soft values 0.3 (class 0) and 0.7 (class 1), the first elements
    walking through the three classes."""
    seed = 4000 + 10 * B + n
    x = synth.uniform(seed, (B, 3 * n), -8.0, 8.0)
    t = torch.tensor([-1.0, 0.0, 1.0, 0.3, 0.7, -1.0])[synth.uniform(seed + 1, (B, n), 0.0, 6.0).long().clamp(max=5)]
    t.view(-1)[:3] = torch.tensor([0.0, 1.0, -1.0])[:B * n]
    return x, t.contiguous(), synth.uniform(seed + 5, (n, 3), 0.5, 8.0)


@pytest.mark.parametrize("B,n", [(1, 5), (3, 5), (1, 1), (256, 14), (300, 14)])
def test_kernel_against_float64(dev, B, n):
    """|loss - ref| <= 1e-5 max(1, |ref|); loss_elem and dlogits within 1e-5 of the largest reference magnitude (the project's bounds
    for its loss kernels; an fp32 statement of the header sits at 2e-7 of that scale).  300 x 14 is no multiple of the 256 threads
    and takes more than one stride."""
    from chexpert_amd import ops
    x, t, cw = _kernel_case(B, n)
    if B * n >= 3:
        assert set(classes_of(t).flatten().tolist()) == {0, 1, 2}
    xd, td = x.to(dev), t.to(dev)
    got = {}
    for w in (cw, None):
        loss_ref, le_ref, g_ref = oracle(x, t, w)
        wd = None if w is None else w.to(dev)
        loss, le, dl = torch.full((1,), 7.0, device=dev), torch.full((B, n), 7.0, device=dev), torch.full((B, 3 * n), 7.0, device=dev)
        ops.mc3_fwd_bwd(xd, td, wd, loss, le, dl)
        what = "B=%d n=%d %s" % (B, n, "weighted" if w is not None else "unweighted")
        print("%s: loss %.7f ref %.7f diff %.3e" % (what, loss.item(), loss_ref.item(), abs(loss.item() - loss_ref.item())))
        assert bool(torch.isfinite(loss).all()) and bool(torch.isfinite(le).all()) and bool(torch.isfinite(dl).all()), what
        assert abs(loss.item() - loss_ref.item()) <= 1e-5 * max(1.0, abs(loss_ref.item())), what
        close(le.cpu().double(), le_ref, rel=1e-5, what=what + " loss_elem")
        close(dl.cpu().double(), g_ref, rel=1e-5, what=what + " dlogits")
        # each output alone gives the same bits; the others do not move
        loss2, le2, dl2 = torch.zeros(1, device=dev), torch.zeros(B, n, device=dev), torch.zeros(B, 3 * n, device=dev)
        ops.mc3_fwd_bwd(xd, td, wd, loss2, None, None)
        assert torch.equal(loss2, loss)
        ops.mc3_fwd_bwd(xd, td, wd, None, le2, None)
        assert torch.equal(le2, le)
        ops.mc3_fwd_bwd(xd, td, wd, None, None, dl2)
        assert torch.equal(dl2, dl) and torch.equal(loss2, loss) and torch.equal(le2, le)
        # grad_scale multiplies the gradient alone
        ops.mc3_fwd_bwd(xd, td, wd, loss2.zero_(), le2.zero_(), dl2.zero_(), grad_scale=0.5)
        assert torch.equal(loss2, loss) and torch.equal(le2, le) and torch.equal(dl2, dl * 0.5)
        # two calls, equal bits
        loss4, le4, dl4 = torch.ones(1, device=dev), torch.ones(B, n, device=dev), torch.ones(B, 3 * n, device=dev)
        ops.mc3_fwd_bwd(xd, td, wd, loss4, le4, dl4)
        assert torch.equal(loss4, loss) and torch.equal(le4, le) and torch.equal(dl4, dl)
        got[w is None] = (loss, le, dl)
    # a table of ones gives the bits of the call without one, and the weights matter
    loss1, le1, dl1 = torch.zeros(1, device=dev), torch.zeros(B, n, device=dev), torch.zeros(B, 3 * n, device=dev)
    ops.mc3_fwd_bwd(xd, td, torch.ones(n, 3, device=dev), loss1, le1, dl1)
    assert all(torch.equal(a, b) for a, b in zip((loss1, le1, dl1), got[True]))
    assert not torch.equal(got[False][2], got[True][2])


def test_confident_elements_keep_their_digits(dev):
    """The target class's logit leads the other two by gaps uniform in [4, 12], each class taking its turn as the target: loss and the
    three gradients of every element within 2e-5 OF ITS OWN reference value (the bound of the focal loss's test of the same name; the
    fp32 statement costs about ten roundings of 2^-24).  Measured on the MI355X: loss 6.0e-7, gradients 7.3e-7 at worst."""
    from chexpert_amd import ops
    for c in range(3):
        z, t = confident_case(c)
        B, n = t.shape
        _, le_ref, g_ref = oracle(z, t, None)
        assert bool((le_ref > 0).all()) and bool((g_ref != 0).all()) and float(le_ref.max()) < 0.04
        le, dl = torch.zeros(B, n, device=dev), torch.zeros(B, 3 * n, device=dev)
        ops.mc3_fwd_bwd(z.to(dev), t.to(dev), None, None, le, dl)
        rl = ((le.cpu().double() - le_ref).abs() / le_ref.abs()).max().item()
        rg = ((dl.cpu().double() - g_ref).abs() / g_ref.abs()).max().item()
        print("target class %d: max elementwise rel err loss %.3e gradient %.3e (smallest reference loss %.3e)" % (c, rl, rg, le_ref.min().item()))
        assert rl < 2e-5 and rg < 2e-5


@pytest.mark.parametrize("B,n", [(3, 5), (1000, 14)])
def test_collapse(dev, B, n):
    from chexpert_amd import ops
    from chexpert_amd.loss import collapse_multiclass
    x = synth.uniform(4500 + B, (B, 3 * n), -8.0, 8.0)
    xd = x.to(dev)
    z, pu = torch.full((B, n), 7.0, device=dev), torch.full((B, n), 7.0, device=dev)
    assert ops.mc3_collapse(xd, z, pu) is z
    assert torch.equal(z, xd[:, 1::3] - xd[:, 0::3])                  # one fp32 subtraction
    p = torch.softmax(x.double().view(B, n, 3), 2)
    err_p = (torch.sigmoid(z).cpu().double() - p[..., 1] / (p[..., 0] + p[..., 1])).abs().max().item()
    err_u = (pu.cpu().double() - p[..., 2]).abs().max().item()
    print("B=%d n=%d: sigmoid(z) against p1 / (p0 + p1): %.3e; p_unc against the float64 softmax: %.3e" % (B, n, err_p, err_u))
    assert err_p <= 1e-6 and err_u <= 1e-6
    z2 = torch.zeros(B, n, device=dev)
    ops.mc3_collapse(xd, z2)                                           # p_unc is optional
    assert torch.equal(z2, z)
    assert torch.equal(collapse_multiclass(xd), z)
    zz, pp = collapse_multiclass(xd, return_uncertain=True)
    assert torch.equal(zz, z) and torch.equal(pp, pu)
    with pytest.raises(RuntimeError, match="3n"):
        collapse_multiclass(xd[:, :3 * n - 1])


def test_wrappers_check_their_operands(dev):
    from chexpert_amd import ops
    x, t, w, loss = torch.zeros(2, 15, device=dev), torch.zeros(2, 5, device=dev), torch.ones(5, 3, device=dev), torch.zeros(1, device=dev)
    for bad in (dict(logits=x.cpu()), dict(class_weight=w.cpu()), dict(loss=loss.cpu()), dict(target=t.cpu())):      # mixed devices
        args = dict(logits=x, target=t, class_weight=w, loss=loss, loss_elem=None, dlogits=None)
        args.update(bad)
        with pytest.raises((RuntimeError, AssertionError)):
            ops.mc3_fwd_bwd(**args)
    for bad in (dict(target=t.double()), dict(class_weight=torch.ones(4, 3, device=dev)), dict(target=torch.zeros(2, 15, device=dev)),
                dict(dlogits=torch.zeros(2, 5, device=dev)), dict(logits=torch.zeros(2, 14, device=dev))):
        args = dict(logits=x, target=t, class_weight=w, loss=loss, loss_elem=None, dlogits=None)
        args.update(bad)
        with pytest.raises(AssertionError):
            ops.mc3_fwd_bwd(**args)
    with pytest.raises(AssertionError):
        ops.mc3_collapse(x, torch.zeros(2, 15, device=dev))
    with pytest.raises((RuntimeError, AssertionError)):
        ops.mc3_collapse(x, torch.zeros(2, 5))


# ------------------------------------------------------------------------------------------------ fused step
def _net(kind, dev, seed=3, width=15):
    from chexpert_amd.models import DenseNet, construct_model
    torch.manual_seed(seed)
    if kind == "densenet":
        model, S = DenseNet(32, (2, 2, 2, 2), 64, num_classes=width), 64
        for n_, p in model.named_parameters():           # well-conditioned regime (tests/test_model_gpu.py)
            if n_.endswith(".bias") and "classifier" not in n_:
                p.data.fill_(2.5)
    else:
        from chexpert_amd.models.efficientnet import DropMarker
        model, S = construct_model("efficientnet-b0", width), 96
        for mod in model.modules():                      # two passes must see the same network: no dropout / DropConnect draws
            if isinstance(mod, DropMarker):
                mod.p = 0.0
    return model.to(dev).train(), S


def _twin(kind, dev):
    a, S = _net(kind, dev)
    b, _ = _net(kind, dev)
    b.load_state_dict({k: v.clone() for k, v in a.state_dict().items()})
    return a, b, S


@pytest.mark.parametrize("net,weighted", [("densenet", False), ("densenet", True), ("efficientnet", True)])
def test_fused_step_equals_the_autograd_route(dev, net, weighted):
    from chexpert_amd import ops
    from chexpert_amd.loss import MaskedBCE, MultiClassUncertain, collapse_multiclass
    a, b, S = _twin(net, dev)
    B, n = 4, 5
    x = synth.xray_batch(2500, B, S).to(dev)
    t = _targets(2510, B, n).to(dev)
    assert (t < 0).any() and (t == 0).any() and (t == 1).any()
    w = synth.uniform(2520, (n, 3), 0.5, 8.0).to(dev) if weighted else None
    keys = list(a.state_dict().keys())
    assert a.set_loss(kind="multiclass", class_weight=w) is a
    crit = MultiClassUncertain(w)
    assert list(a.state_dict().keys()) == keys and a.loss_step_state() == []      # neither buffer nor parameter; nothing per step
    assert a.loss_kind == "multiclass" and a.loss_ignore_negative is False and a.loss_pos_weight is None and a.loss_focus is None
    if weighted:
        cw = a.loss_class_weight
        assert tuple(cw.shape) == (n, 3) and cw.is_cuda and cw.dtype == torch.float32 and torch.equal(cw, w) and cw.data_ptr() != w.data_ptr()
    else:
        assert a.loss_class_weight is None
    loss_a, logits_a = a.forward_backward(x, t)
    assert tuple(logits_a.shape) == (B, 3 * n)
    out = b(x)
    loss_b = crit(out, t)
    loss_b.backward()
    assert loss_b.dim() == 0 and torch.equal(loss_a.reshape(()), loss_b.detach())
    assert torch.equal(logits_a, out.detach())
    ga, gb = dict(a.named_parameters()), dict(b.named_parameters())
    for k in ga:
        assert torch.equal(ga[k].grad, gb[k].grad), k
    assert max(float(p.grad.abs().max()) for p in ga.values()) > 0
    # the loss is the float64 oracle's, and so are the element losses outside autograd
    ref, le_ref, _ = oracle(logits_a.cpu(), t.cpu(), None if w is None else w.cpu())
    print("%s weighted=%s: fused loss %.7f, float64 oracle %.7f" % (net, weighted, loss_a.item(), ref.item()))
    assert abs(loss_a.item() - ref.item()) <= 1e-5 * max(1.0, abs(ref.item()))
    le = crit.elementwise(out, t)
    assert not le.requires_grad and tuple(le.shape) == (B, n)
    close(le.cpu().double(), le_ref, rel=1e-5, what="elementwise")
    # backward scales by the incoming gradient
    xl = logits_a.clone().requires_grad_(True)
    (3.0 * crit(xl, t)).backward()
    dl = torch.empty_like(logits_a)
    ops.mc3_fwd_bwd(logits_a, t, a.loss_class_weight, None, None, dl)
    assert torch.equal(xl.grad, dl * 3.0)
    # teeth: these are not the gradients of the cross-entropy on the collapsed logits
    zl = logits_a.clone().requires_grad_(True)
    MaskedBCE()(zl[:, 1::3] - zl[:, 0::3], t).backward()
    assert not torch.equal(zl.grad, dl) and torch.equal(collapse_multiclass(logits_a), logits_a[:, 1::3] - logits_a[:, 0::3])
    # the module refuses logits and targets of one shape, which every other loss takes
    with pytest.raises(RuntimeError, match="3n"):
        crit(out, torch.zeros(B, 3 * n, device=dev))
    # the eval-mode (frozen BatchNorm) step fills a finite, non-zero input gradient
    if net == "densenet":
        a.zero_grad(set_to_none=True)
        a.eval()
        buf = torch.full((B, 3, S, S), 7.0, device=dev)
        loss_e, _ = a.forward_backward(x, t, input_grad=buf)
        assert math.isfinite(loss_e.item()) and bool(torch.isfinite(buf).all()) and float(buf.abs().max()) > 0 and not bool((buf == 7.0).any())
        assert float(a.classifier.weight.grad.abs().max()) > 0


def test_set_loss_walk_leaves_nothing_of_the_previous_kind(dev):
    """bce (weights) -> multiclass (weights) -> asl (weights) -> multiclass (none) -> multiclass (weights): after every move the public
    attributes are the new kind's alone, the step's loss and d loss / d logits are those of the matching module on the same logits, bit
    for bit, the held storage of a second visit is that of the first, and loss_state() round-trips."""
    from chexpert_amd.loss import AsymmetricLoss, MaskedBCE, MultiClassUncertain
    model, S = _net("densenet", dev)
    other, _ = _net("densenet", dev)
    B, n = 2, 5
    x = synth.xray_batch(2700, B, S).to(dev)
    t3, t1 = _targets(2710, B, n, 0.3).to(dev), _targets(2720, B, 3 * n, 0.3).to(dev)
    pw, cw = synth.uniform(2730, (3 * n,), 0.5, 8.0), synth.uniform(2740, (n, 3), 0.5, 8.0)
    bce_state = {"kind": "bce", "aux": None, "prior": None, "margin": 1.0, "lr_aux": None}
    assert model.loss_state() == bce_state
    # (kind, set_loss keywords, the module, the target, then what the model must hold: ignore_negative, pos_weight, focus, class_weight)
    walk = [("bce", dict(pos_weight=pw), lambda: MaskedBCE(pw, ignore_negative=False), t1, False, pw, None, None),
            ("multiclass", dict(kind="multiclass", class_weight=cw), lambda: MultiClassUncertain(cw), t3, False, None, None, cw),
            ("asl", dict(kind="asl", pos_weight=pw), lambda: AsymmetricLoss(pos_weight=pw), t1, True, pw, torch.tensor([0.0, 4.0, 0.05, -1.0]), None),
            ("multiclass", dict(kind="multiclass"), lambda: MultiClassUncertain(), t3, False, None, None, None),
            ("multiclass", dict(kind="multiclass", class_weight=2 * cw), lambda: MultiClassUncertain(2 * cw), t3, False, None, None, 2 * cw)]
    eng, seen, ptrs = model._eng(), [], {}
    backward = eng.backward

    def spy(ws, dl, dx=None):                                           # d loss / d logits, as the step hands it to the backward pass
        seen.append(dl.clone())
        return backward(ws, dl, dx=dx)
    eng.backward = spy
    for kind, kw, make, t, ign, w, focus, cweight in walk:
        assert model.set_loss(**kw) is model
        assert (model.loss_kind, model.loss_ignore_negative) == (kind, ign), kw
        assert model.loss_aux is None and model.loss_prior is None and model.loss_lr_aux is None
        for name, want in (("loss_pos_weight", w), ("loss_focus", focus), ("loss_class_weight", cweight)):
            got = getattr(model, name)
            assert (got is None) == (want is None), (kw, name)
            if got is not None:
                assert got.is_cuda and got.dtype == torch.float32 and torch.equal(got.cpu(), want), (kw, name)
                assert ptrs.setdefault(name, got.data_ptr()) == got.data_ptr(), (kw, name)
        st = model.loss_state()
        assert st["kind"] == kind and model.loss_step_state() == [] and ("class_weight" in st) == (kind == "multiclass")
        if kind == "multiclass":                                        # round trip through another model
            assert (st["class_weight"] is None) == (cweight is None) and (cweight is None or (not st["class_weight"].is_cuda and torch.equal(st["class_weight"], cweight)))
            assert other.load_loss_state(st) is other and other.loss_kind == "multiclass"
            st2 = other.loss_state()
            assert st2.keys() == st.keys() and (st2["class_weight"] is None if cweight is None else torch.equal(st2["class_weight"], cweight))
        model.zero_grad(set_to_none=True)
        loss, logits = model.forward_backward(x, t)
        xl = logits.clone().requires_grad_(True)
        lm = make()(xl, t)
        lm.backward()
        assert torch.equal(lm.detach(), loss.reshape(())) and torch.equal(xl.grad, seen[-1]), kw
        assert math.isfinite(loss.item()) and float(seen[-1].abs().max()) > 0
    assert len(seen) == len(walk) and set(ptrs) == {"loss_pos_weight", "loss_focus", "loss_class_weight"}
    with pytest.raises(ValueError):                                     # refused: nothing changes
        model.set_loss(kind="multiclass", class_weight=torch.ones(4, 3))
    assert model.loss_kind == "multiclass" and torch.equal(model.loss_class_weight.cpu(), 2 * cw)
    assert model.set_loss() is model and model.loss_class_weight is None and model.loss_state() == bce_state
    assert other.load_loss_state(bce_state) is other and other.loss_kind == "bce" and other.loss_class_weight is None


def test_graphed_step_equals_eager_and_sees_class_weight_changes(dev):
    from chexpert_amd.graph import GraphedTrainStep
    from chexpert_amd.optim import FusedAdam
    m_e, m_g, S = _twin("densenet", dev)
    B, n = 4, 5
    xs = [synth.xray_batch(2800 + i, B, S).to(dev) for i in range(4)]
    ts = [_targets(2810 + 10 * i, B, n).to(dev) for i in range(4)]
    w = synth.uniform(2820, (n, 3), 0.5, 8.0).to(dev)
    for m in (m_e, m_g):
        m.set_loss(kind="multiclass", class_weight=w)
    opt_e, opt_g = FusedAdam(m_e, lr=1e-3), FusedAdam(m_g, lr=1e-3)
    # captured on a batch WITHOUT uncertain labels: what a replay reads is the target copied in, not the one captured
    gs = GraphedTrainStep(m_g, opt_g, xs[0], synth.targets(2830, B, n).to(dev))
    held = m_g.loss_class_weight.data_ptr()
    flat = lambda m: torch.cat([p.detach().flatten() for p in m.parameters()])                               # noqa: E731
    for i in range(3):
        le = _eager_dev_step(m_e, opt_e, xs[i], ts[i])
        lg, logits = gs.replay(xs[i], ts[i])
        assert tuple(logits.shape) == (B, 3 * n) and torch.equal(le, lg), (i, le.item(), lg.item())
        assert torch.equal(flat(m_e), flat(m_g)), i
        assert torch.equal(m_e._eng().flat_grad, m_g._eng().flat_grad)
    # the weights change in place: the next replay reads the new values and matches an eager step with them
    m_g.loss_class_weight.mul_(2)
    m_e.set_loss(kind="multiclass", class_weight=2 * w)
    assert m_g.loss_class_weight.data_ptr() == held and torch.equal(m_g.loss_class_weight, m_e.loss_class_weight)
    le = _eager_dev_step(m_e, opt_e, xs[3], ts[3])
    lg, logits = gs.replay(xs[3], ts[3])
    assert torch.equal(le, lg) and torch.equal(flat(m_e), flat(m_g))
    # ... and it matters: the same logits under the first weights give another loss
    from chexpert_amd.loss import MultiClassUncertain
    assert MultiClassUncertain(w)(logits, ts[3]).item() != lg.item() == MultiClassUncertain(2 * w)(logits, ts[3]).item()


# ------------------------------------------------------------------------------------------------ data parallel
def _dp_worker(rank, world, port, out_dir):
    import torch.distributed as dist
    os.environ["MASTER_ADDR"], os.environ["MASTER_PORT"] = "127.0.0.1", str(port)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    from chexpert_amd.parallel import broadcast_module_state
    dev = torch.device("cuda:0")
    model, S = _net("densenet", dev)
    broadcast_module_state(model)
    x = synth.xray_batch(3100 + rank, 4, S).to(dev)
    t = _targets(3200 + 10 * rank, 4, 5, 0.3).to(dev)
    model.set_loss(kind="multiclass", class_weight=synth.uniform(9, (5, 3), 0.5, 8.0))
    loss, logits = model.forward_backward(x, t)           # binds the engine; the single-process gradient of this shard, no reducer yet
    eng = model._eng()
    g_local = eng.flat_grad.detach().cpu().clone()
    gathered = [torch.empty_like(g_local) for _ in range(world)]
    dist.all_gather(gathered, g_local)
    want = sum(gathered) / world
    eng.enable_data_parallel(bucket_bytes=1 << 16)
    model.zero_grad()
    model.forward_backward(x, t)
    torch.cuda.synchronize()
    got = eng.flat_grad.detach().cpu().clone()
    both = [torch.empty_like(got) for _ in range(world)]
    dist.all_gather(both, got)
    torch.save({"got": got, "want": want, "local": g_local, "same": bool(torch.equal(both[0], both[1])), "logits": logits.cpu(), "t": t.cpu(),
                "loss": loss.item(), "n_uncertain": int((t < 0).sum()), "n_buckets": len(eng.reducer.ranges)}, os.path.join(out_dir, "rank%d.pt" % rank))
    dist.destroy_process_group()


def _spawn_with_time_limit(fn, args, nprocs, seconds):
    """mp.spawn whose processes are killed when they outlive `seconds` (a hung rank must not outlive its test)."""
    import torch.multiprocessing as mp
    ctx = mp.spawn(fn, args=args, nprocs=nprocs, join=False)
    deadline = time.time() + seconds
    try:
        while not ctx.join(timeout=5):
            if time.time() > deadline:
                raise TimeoutError("the ranks ran longer than %d s" % seconds)
    finally:
        for p in ctx.processes:
            if p.is_alive():
                p.kill()
                p.join()


def test_data_parallel_gradients_two_ranks_one_gpu(dev, tmp_path):
    """Two ranks on one GPU: the gradients the reducer leaves on both ranks are the mean of the two single-process gradients, to the
    1e-6 relative of the masked BCE's data-parallel test.  That mean is the gradient of the joined batch under data-parallel semantics
    -- BatchNorm statistics per rank --, and the loss kernel's own share of the statement holds bit for bit: on the joined logits
    (B = 8) it returns each shard's dlogits at grad_scale 1/2, and the mean of the two losses."""
    from chexpert_amd import ops
    port = 36500 + (os.getpid() % 400)
    _spawn_with_time_limit(_dp_worker, (2, port, str(tmp_path)), 2, 300)
    recs = [torch.load(os.path.join(str(tmp_path), "rank%d.pt" % r)) for r in range(2)]
    assert not torch.equal(recs[0]["local"], recs[1]["local"])
    for r, rec in enumerate(recs):
        assert rec["same"], "ranks ended with different gradients"
        assert rec["n_buckets"] >= 3 and rec["n_uncertain"] >= 2
        g, w = rec["got"].double(), rec["want"].double()
        rel = float((g - w).norm() / w.norm())
        print("rank %d: rel %.3e, %d uncertain labels, %d buckets" % (r, rel, rec["n_uncertain"], rec["n_buckets"]))
        assert rel < 1e-6, rel
    # the joined batch through the loss kernel
    w = synth.uniform(9, (5, 3), 0.5, 8.0).to(dev)
    xj, tj = torch.cat([r["logits"] for r in recs]).to(dev), torch.cat([r["t"] for r in recs]).to(dev)
    lj, dj = torch.zeros(1, device=dev), torch.zeros(8, 15, device=dev)
    ops.mc3_fwd_bwd(xj, tj, w, lj, None, dj)
    halves = []
    for r in recs:
        d = torch.zeros(4, 15, device=dev)
        ops.mc3_fwd_bwd(r["logits"].to(dev), r["t"].to(dev), w, None, None, d, grad_scale=0.5)
        halves.append(d)
    assert torch.equal(dj, torch.cat(halves)) and float(dj.abs().max()) > 0
    assert abs(lj.item() - 0.5 * (recs[0]["loss"] + recs[1]["loss"])) <= 1e-6 * max(1.0, abs(lj.item()))


# ------------------------------------------------------------------------------------------------ predict
class _Studies(torch.utils.data.Dataset):
    """What predict() needs of a ChexpertCSV: uint8 items, attr_names, and a Path column for the study names."""
    attr_names = ["Atelectasis", "Cardiomegaly", "Consolidation", "Edema", "Pleural Effusion"]

    def __init__(self, n, size):
        import pandas as pd
        self.x = synth.xray_u8(123, n, size)
        # study 0 has two views
        self.data = pd.DataFrame({"Path": ["valid/patient%05d/study1/view%d_frontal.jpg" % (max(i, 1), i) for i in range(n)]})

    def __len__(self):
        return len(self.x)

    def __getitem__(self, i):
        return self.x[i], torch.zeros(5), i


def test_predict_collapses_the_three_way_head(dev):
    """predict(collapse=True) on a model with 3n outputs: the probabilities are sigmoid(z1 - z0) of every forward, one column per
    finding, the max over a study's views as always; --tta and a calibration map act on the collapsed logits."""
    from chexpert_amd import predict
    model, S = _net("densenet", dev)
    model.eval()
    ds, bs = _Studies(8, S), 3
    with torch.no_grad():
        out = torch.cat([model(ds.x[k:k + bs].to(dev)).float() for k in range(0, 8, bs)])
    assert tuple(out.shape) == (8, 15)
    plain = torch.sigmoid(out[:, 1::3] - out[:, 0::3]).cpu()
    p1 = predict.predict(model, ds, bs, dev, collapse=True)
    assert len(p1) == 7 and list(p1.columns) == ds.attr_names
    assert torch.equal(torch.from_numpy(p1.values[1:]), plain[2:])                          # the other studies: one view each
    assert torch.equal(torch.from_numpy(p1.values[0]), torch.maximum(plain[0], plain[1]))   # max over the two views
    a, b = synth.uniform(5, (5,), 0.5, 2.0), synth.uniform(6, (5,), -1.0, 1.0)
    cal = {"method": "platt", "a": {c: float(a[c]) for c in range(5)}, "b": {c: float(b[c]) for c in range(5)}}
    pc = predict.predict(model, ds, bs, dev, cal=cal, collapse=True)
    want = torch.sigmoid((out[:, 1::3] - out[:, 0::3]) * a.to(dev) + b.to(dev)).cpu()
    assert torch.equal(torch.from_numpy(pc.values[1:]), want[2:])
    p2 = predict.predict(model, ds, bs, dev, tta=2, tta_seed=5, collapse=True)
    assert tuple(p2.shape) == (7, 5) and not p2.equals(p1) and bool(((p2.values > 0) & (p2.values < 1)).all())
    with pytest.raises(ValueError):                                     # without the collapse the 15 columns meet five names
        predict.predict(model, ds, bs, dev)


# ------------------------------------------------------------------------------------------------ command line
def _losses(capsys):
    out = capsys.readouterr().out
    return [json.loads(l)["train_loss"] for l in out.splitlines() if l.startswith('{"step"')]


_CLI = ["--train", "--synthetic", "32", "--batch_size", "4", "--resize", "64", "--eval_interval", "8", "--log_interval", "1", "--seed", "3",
        "--lr", "0.001"]
_MC = ["--synthetic_uncertain", "0.2", "--uncertain", "multiclass"]
_GRAPH = _MC + ["--fused_optimizer", "--graph"]


@pytest.fixture(scope="module")
def graphed_run(dev, tmp_path_factory):
    """One `--uncertain multiclass --fused_optimizer --graph --bootstrap 50 --calibrate platt` training run, shared by the two tests
    below: (output folder, model, its stdout)."""
    import contextlib
    import io
    from chexpert_amd import cli
    out = str(tmp_path_factory.mktemp("multiclass") / "g")
    buf = io.StringIO()
    with contextlib.redirect_stdout(buf):
        model = cli.main(_CLI + _GRAPH + ["--bootstrap", "50", "--calibrate", "platt", "--output_dir", out])
    return out, model, buf.getvalue()


def test_cli_graphed_run_writes_collapsed_results_and_the_loss_state(graphed_run):
    out, model, text = graphed_run
    lg = [json.loads(l)["train_loss"] for l in text.splitlines() if l.startswith('{"step"')]
    assert len(lg) == 8 and all(math.isfinite(v) for v in lg), lg
    assert model.loss_kind == "multiclass" and model.loss_class_weight is None and model.classifier.out_features == 15
    cfg = json.load(open(os.path.join(out, "config.json")))
    assert cfg["uncertain"] == "multiclass" and cfg["loss"] == "bce" and cfg["n_classes"] == 5
    ck = os.path.join(out, "checkpoint_latest.pt")
    saved = torch.load(ck, map_location="cpu")
    assert saved["loss_state"]["kind"] == "multiclass" and saved["loss_state"]["class_weight"] is None
    assert saved["state_dict"]["classifier.weight"].shape[0] == 15
    # everything behind the forward sees (N, n_classes): the collapsed logits
    res = json.load(open(os.path.join(out, "eval_results_step_8.json")))
    assert len(res["aucs"]) == 5 and len(res["loss"]) == 5 and all(math.isfinite(v) for v in res["loss"].values())
    ci = json.load(open(os.path.join(out, "auc_ci_step_8.json")))
    assert len(ci["aucs"]) == len(ci["lo"]) == len(ci["hi"]) == 5
    cal = json.load(open(os.path.join(out, "calibration_step_8.json")))
    assert cal["fit"]["method"] == "platt" and len(cal["ece_before"]["point"]) == 5 and os.path.isfile(os.path.join(out, "reliability_step_8.png"))


def test_cli_restores_and_refuses_the_other_head(dev, graphed_run, tmp_path, capsys):
    from chexpert_amd import cli
    capsys.readouterr()
    ck = os.path.join(graphed_run[0], "checkpoint_latest.pt")
    # --restore checks the head and continues
    out2 = str(tmp_path / "r")
    model2 = cli.main(_CLI + _GRAPH + ["--restore", ck, "--output_dir", out2])
    lr_ = _losses(capsys)
    assert len(lr_) == 8 and all(math.isfinite(v) for v in lr_), lr_
    st2 = torch.load(os.path.join(out2, "checkpoint_latest.pt"), map_location="cpu")
    assert model2.loss_kind == "multiclass" and st2["global_step"] == 16 and st2["loss_state"]["kind"] == "multiclass"
    # a run of the other head refuses the checkpoint by name, before load_state_dict meets the shapes
    with pytest.raises(ValueError, match="trained with --uncertain multiclass.*without it"):
        cli.main(_CLI + ["--fused_optimizer", "--restore", ck, "--output_dir", str(tmp_path / "x")])
    with pytest.raises(ValueError, match="trained with --uncertain multiclass.*without it"):
        cli.main(["--evaluate_single_model", "--synthetic", "32", "--batch_size", "4", "--resize", "64", "--restore", ck, "--output_dir", str(tmp_path / "y")])


def test_cli_autograd_route_is_the_same_kernel(dev, tmp_path, capsys):
    """Without --fused_optimizer the loss module computes the loss: the first batch's loss line is the fused route's."""
    from chexpert_amd import cli
    capsys.readouterr()
    flags = _MC + ["--synthetic", "16", "--eval_interval", "4", "--erase_prob", "0.3"]
    m1 = cli.main(_CLI + flags + ["--output_dir", str(tmp_path / "e")])
    le = _losses(capsys)
    m2 = cli.main(_CLI + flags + ["--fused_optimizer", "--output_dir", str(tmp_path / "f")])
    lf = _losses(capsys)
    assert len(le) == len(lf) == 4 and all(math.isfinite(v) for v in le + lf) and le[0] == lf[0], (le, lf)
    for m, d in ((m1, "e"), (m2, "f")):
        assert m.loss_kind == "multiclass" and m.classifier.out_features == 15
        assert torch.load(os.path.join(str(tmp_path / d), "checkpoint_latest.pt"), map_location="cpu")["loss_state"]["kind"] == "multiclass"
        assert len(json.load(open(os.path.join(str(tmp_path / d), "eval_results_step_4.json")))["aucs"]) == 5


def test_cli_default_flags_never_reach_the_new_kernels(dev, tmp_path, capsys, monkeypatch):
    from chexpert_amd import cli, ops
    from chexpert_amd.loss import collapse_multiclass

    def refuse(*a, **k):
        raise AssertionError("a cx_mc3 wrapper was reached without --uncertain multiclass")
    monkeypatch.setattr(ops, "mc3_fwd_bwd", refuse)
    monkeypatch.setattr(ops, "mc3_collapse", refuse)
    capsys.readouterr()
    out = str(tmp_path / "p")
    model = cli.main(_CLI[:2] + ["16"] + _CLI[3:] + ["--eval_interval", "4", "--fused_optimizer", "--graph", "--output_dir", out])
    lp = _losses(capsys)
    assert len(lp) == 4 and all(math.isfinite(v) for v in lp), lp
    assert model.loss_kind == "bce" and model.loss_class_weight is None and model.classifier.out_features == 5
    ck = os.path.join(out, "checkpoint_latest.pt")
    assert "loss_state" not in torch.load(ck, map_location="cpu")
    assert json.load(open(os.path.join(out, "config.json")))["uncertain"] == "ones"
    # the patches have teeth: these are the names FusedNet.forward_backward, the loss module and the collapse call
    wide, S = _net("densenet", dev)
    wide.set_loss(kind="multiclass")
    x, t = synth.xray_batch(2900, 4, S).to(dev), _targets(2910, 4, 5).to(dev)
    with pytest.raises(AssertionError, match="was reached"):
        wide.forward_backward(x, t)
    with pytest.raises(AssertionError, match="was reached"):
        collapse_multiclass(torch.zeros(2, 6, device=dev))
    # the reverse refusal: a --uncertain multiclass run does not take the cross-entropy run's checkpoint
    with pytest.raises(ValueError, match="trained without --uncertain multiclass.*with it"):
        cli.main(_CLI + _MC + ["--fused_optimizer", "--restore", ck, "--output_dir", str(tmp_path / "x")])
