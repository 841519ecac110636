"""GPU: the focal / asymmetric loss -- cx_asl_fwd_bwd against the float64 oracle (shared with tests/test_focal_cpu.py, which checks
it against central differences and the restated torchvision / timm formulas), its confident elements one by one, FusedNet.set_loss
(kind="focal" | "asl") in the fused step against the autograd route, under graph replay and data-parallel, and the command line."""
import json
import math
import os
import time

import pytest
import torch
import torch.nn.functional as F

from chexpert_amd import synth
from eager_step import _eager_dev_step

pytestmark = pytest.mark.gpu

# (gamma+, gamma-, clip, alpha); the last set has a fractional exponent below 1 together with a clip: g u^(g-1) u' is inf * 0 there
P_SETS = [(0.0, 0.0, 0.0, None), (2.0, 2.0, 0.0, 0.25), (0.0, 4.0, 0.05, None), (1.0, 4.0, 0.05, None), (0.5, 0.5, 0.2, None)]


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


def _targets(seed, B, n, ignored=0.2, soft=0.15):
    """Hard Bernoulli(0.3) labels, a share `soft` of them replaced by values uniform in [0, 1], a share `ignored` by -1."""
    t = synth.targets(seed, B, n).clone()
    u = synth.uniform(seed + 1, (B, n), 0.0, 1.0)
    t = torch.where(synth.uniform(seed + 2, (B, n), 0.0, 1.0) < soft, u, t)
    return torch.where(synth.uniform(seed + 3, (B, n), 0.0, 1.0) < ignored, torch.full_like(t, -1.0), t)


def _focus(P, dev):
    gp, gn, m, alpha = P
    return torch.tensor([gp, gn, m, -1.0 if alpha is None else alpha], dtype=torch.float32, device=dev)


# ------------------------------------------------------------------------------------------------ float64 oracle (as in test_focal_cpu.py)
def _elem64(x, t, w, P):
    """The definition, float64, differentiable.  Piecewise where the naive statement is inf * 0 (a hard negative at or below the
    clip with an exponent below 1): every `where` masks the OPERAND of log / exp, not only the result, so autograd never multiplies
    a zero by an infinite local derivative."""
    gp, gn, m, alpha = P
    live = t >= 0
    tt = torch.where(live, t, torch.zeros_like(t))
    p, q = torch.sigmoid(x), torch.sigmoid(-x)
    logp, logq = F.logsigmoid(x), F.logsigmoid(-x)
    one, zero = torch.ones_like(x), torch.zeros_like(x)
    above = p > m
    pm = torch.where(above, p - m, zero)
    logpn = logq if m == 0 else torch.where(above, torch.log(torch.where(above, q + m, one)), zero)
    w = one if w is None else w
    C = -(w * tt * logp + (1 - tt) * logpn)
    u = tt * q + (1 - tt) * pm
    g = gp * tt + gn * (1 - tt)
    pos = (u > 0) & (g > 0)
    f = torch.where(g == 0, one, torch.where(pos, torch.exp(g * torch.log(torch.where(pos, u, one))), zero))
    a = one if alpha is None else alpha * tt + (1 - alpha) * (1 - tt)
    return torch.where(live, a * f * C, zero)


def oracle(logits, t, w, P):
    """(loss, element losses, d loss / d logits) by autograd in float64; loss = sum of elements / B."""
    x = logits.double().clone().requires_grad_(True)
    le = _elem64(x, t.double(), None if w is None else w.double(), P)
    loss = le.sum() / x.shape[0]
    loss.backward()
    return loss.detach(), le.detach(), x.grad


# ------------------------------------------------------------------------------------------------ kernel
def _kernel_case(B, n):
    """Logits uniform in +-8, a share of them moved to -10 .. -4 (below every clip of P_SETS as a probability); element (0, 0) is a
    hard negative at -7."""
    seed = 3000 + 10 * B + n
    x = synth.uniform(seed, (B, n), -8.0, 8.0)
    x = torch.where(synth.uniform(seed + 1, (B, n), 0.0, 1.0) < 0.15, synth.uniform(seed + 2, (B, n), -10.0, -4.0), x)
    t = _targets(seed + 10, B, n)
    x[0, 0], t[0, 0] = -7.0, 0.0
    return x, t, synth.uniform(seed + 5, (n,), 0.5, 8.0)


@pytest.mark.parametrize("B,n", [(1, 5), (3, 5), (256, 14), (300, 14)])
def test_kernel_against_float64(dev, B, n):
    """|loss - ref| <= 1e-5 max(1, |ref|); loss_elem and dlogits within 1e-5 of the largest reference magnitude (the bounds of the
    masked BCE's test; an fp32 statement of the definition sits at 1e-7 .. 6e-7 of that scale).  300 x 14 is no multiple of the 256
    threads and takes more than one stride."""
    from chexpert_amd import ops
    x, t, pw = _kernel_case(B, n)
    if B >= 256:
        assert (t < 0).any() and ((t > 0) & (t < 1)).any() and (t == 1).any() and (t == 0).any()
    xd, td = x.to(dev), t.to(dev)
    ign = t < 0
    for P in P_SETS:
        m = P[2]
        below = (t == 0) & (torch.sigmoid(x.double()) <= m)            # hard negatives at or below the clip
        assert m == 0 or bool(below[0, 0])
        for w in (pw, None):
            loss_ref, le_ref, g_ref = oracle(x, t, w, P)
            assert bool(torch.isfinite(g_ref).all()) and bool((g_ref[below] == 0).all()) and bool((le_ref[below] == 0).all())
            wd, fo = None if w is None else w.to(dev), _focus(P, dev)
            loss, le, dl = torch.full((1,), 7.0, device=dev), torch.full((B, n), 7.0, device=dev), torch.full((B, n), 7.0, device=dev)
            ops.asl_fwd_bwd(xd, td, wd, fo, loss, le, dl)
            what = "B=%d n=%d P=%s %s" % (B, n, P, "weighted" if w is not None else "unweighted")
            print("%s: loss %.7f ref %.7f diff %.3e" % (what, loss.item(), loss_ref.item(), abs(loss.item() - loss_ref.item())))
            assert bool(torch.isfinite(loss).all()) and bool(torch.isfinite(le).all()) and bool(torch.isfinite(dl).all()), what
            assert abs(loss.item() - loss_ref.item()) <= 1e-5 * max(1.0, abs(loss_ref.item())), what
            close(le.cpu().double(), le_ref, rel=1e-5, what=what + " loss_elem")
            close(dl.cpu().double(), g_ref, rel=1e-5, what=what + " dlogits")
            assert bool((le.cpu()[ign] == 0.0).all()) and bool((dl.cpu()[ign] == 0.0).all()), what
            assert bool((le.cpu()[below] == 0.0).all()) and bool((dl.cpu()[below] == 0.0).all()), what
            # each output is optional; the others do not move
            loss2, le2, dl2 = torch.zeros(1, device=dev), torch.zeros(B, n, device=dev), torch.zeros(B, n, device=dev)
            ops.asl_fwd_bwd(xd, td, wd, fo, loss2, None, dl2)
            assert torch.equal(loss2, loss) and torch.equal(dl2, dl)
            loss3 = torch.zeros(1, device=dev)
            ops.asl_fwd_bwd(xd, td, wd, fo, loss3, le2, None)
            assert torch.equal(loss3, loss) and torch.equal(le2, le)
            ops.asl_fwd_bwd(xd, td, wd, fo, None, None, dl2.zero_())
            assert torch.equal(dl2, dl)
            # grad_scale multiplies the gradient alone
            ops.asl_fwd_bwd(xd, td, wd, fo, loss2.zero_(), le2.zero_(), dl2, grad_scale=0.5)
            assert torch.equal(loss2, loss) and torch.equal(le2, le) and torch.equal(dl2, dl * 0.5)
            # two calls, equal bits
            loss4, le4, dl4 = torch.ones(1, device=dev), torch.ones(B, n, device=dev), torch.ones(B, n, device=dev)
            ops.asl_fwd_bwd(xd, td, wd, fo, loss4, le4, dl4)
            assert torch.equal(loss4, loss) and torch.equal(le4, le) and torch.equal(dl4, dl)
    # without focusing it is the masked cross-entropy's statement: the two kernels agree to the same bound
    loss_b, le_b, dl_b = torch.zeros(1, device=dev), torch.zeros(B, n, device=dev), torch.zeros(B, n, device=dev)
    ops.bce_masked_fwd_bwd(xd, td, pw.to(dev), loss_b, le_b, dl_b)
    ops.asl_fwd_bwd(xd, td, pw.to(dev), _focus(P_SETS[0], dev), loss, le, dl)
    assert abs(loss.item() - loss_b.item()) <= 1e-5 * max(1.0, abs(loss_b.item()))
    close(le.cpu().double(), le_b.cpu().double(), rel=1e-5, what="loss_elem against cx_bce_masked_fwd_bwd")
    close(dl.cpu().double(), dl_b.cpu().double(), rel=1e-5, what="dlogits against cx_bce_masked_fwd_bwd")


@pytest.mark.parametrize("weighted", [False, True])
def test_all_ignored_batch(dev, weighted):
    from chexpert_amd import ops
    B, n = 7, 5
    logits = synth.uniform(5, (B, n), -8.0, 8.0).to(dev)
    t = torch.full((B, n), -1.0, device=dev)
    w = synth.uniform(6, (n,), 0.5, 8.0).to(dev) if weighted else None
    for P in P_SETS:
        loss, le, dl = torch.full((1,), 7.0, device=dev), torch.full((B, n), 7.0, device=dev), torch.full((B, n), 7.0, device=dev)
        ops.asl_fwd_bwd(logits, t, w, _focus(P, dev), loss, le, dl)
        assert loss.item() == 0.0 and bool((le == 0).all()) and bool((dl == 0).all())


@pytest.mark.parametrize("gamma", [1.0, 2.0, 4.0])
def test_confident_elements_keep_their_digits(dev, gamma):
    """Hard positives at logits 4 .. 10 and the mirrored hard negatives (no clip): loss and gradient of every element within 2e-5 OF
    ITS OWN reference value -- they are tiny against the batch's largest, so the bound relative to that maximum does not see them.
    exp(gamma log u) in fp32 costs about gamma |ln u| 2^-23 <= 5e-6 there, plus a few roundings (an fp32 statement measured 5e-7); the
    cancelling form 1 - sigmoid(x) loses e^x of its digits (1e-3 .. 5e-3 at these logits)."""
    from chexpert_amd import ops
    B, n = 64, 5
    x = synth.uniform(51, (B, n), 4.0, 10.0)
    fo = _focus((gamma, gamma, 0.0, None), dev)
    for xs, t in ((x, torch.ones(B, n)), (-x, torch.zeros(B, n))):
        _, le_ref, g_ref = oracle(xs, t, None, (gamma, gamma, 0.0, None))
        le, dl = torch.zeros(B, n, device=dev), torch.zeros(B, n, device=dev)
        ops.asl_fwd_bwd(xs.to(dev), t.to(dev), None, fo, None, le, dl)
        assert bool((le_ref > 0).all()) and bool((g_ref != 0).all())
        rl = ((le.cpu().double() - le_ref).abs() / le_ref.abs()).max().item()
        rg = ((dl.cpu().double() - g_ref).abs() / g_ref.abs()).max().item()
        print("gamma %g, %s: max elementwise rel err loss %.3e gradient %.3e (smallest reference loss %.3e)"
              % (gamma, "positives" if t[0, 0] == 1 else "negatives", rl, rg, le_ref.min().item()))
        assert rl < 2e-5 and rg < 2e-5


def test_wrapper_checks_its_operands(dev):
    from chexpert_amd import ops
    x, t, w = torch.zeros(2, 5, device=dev), torch.zeros(2, 5, device=dev), torch.ones(5, device=dev)
    fo, loss = _focus(P_SETS[2], dev), torch.zeros(1, device=dev)
    for bad in (dict(logits=x.cpu()), dict(pos_weight=w.cpu()), dict(focus=fo.cpu()), dict(loss=loss.cpu())):      # mixed devices
        args = dict(logits=x, target=t, pos_weight=w, focus=fo, loss=loss, loss_elem=None, dlogits=None)
        args.update(bad)
        with pytest.raises((RuntimeError, AssertionError)):
            ops.asl_fwd_bwd(**args)
    for bad in (dict(target=t.double()), dict(pos_weight=torch.ones(4, device=dev)), dict(logits=x.t(), target=t.t()),
                dict(dlogits=torch.zeros(2, 4, device=dev)), dict(focus=torch.zeros(3, device=dev))):
        args = dict(logits=x, target=t, pos_weight=w, focus=fo, loss=loss, loss_elem=None, dlogits=None)
        args.update(bad)
        with pytest.raises(AssertionError):
            ops.asl_fwd_bwd(**args)


# ------------------------------------------------------------------------------------------------ fused step
def _net(kind, dev, seed=3):
    from chexpert_amd.models import DenseNet, construct_model
    torch.manual_seed(seed)
    if kind == "densenet":
        model, S = DenseNet(32, (2, 2, 2, 2), 64, num_classes=5), 64
        for n_, p in model.named_parameters():           # well-conditioned regime (tests/test_model_gpu.py)
            if n_.endswith(".bias") and "classifier" not in n_:
                p.data.fill_(2.5)
    else:
        from chexpert_amd.models.efficientnet import DropMarker
        model, S = construct_model("efficientnet-b0", 5), 96
        for mod in model.modules():                      # two passes must see the same network: no dropout / DropConnect draws
            if isinstance(mod, DropMarker):
                mod.p = 0.0
    return model.to(dev).train(), S


def _twin(kind, dev):
    a, S = _net(kind, dev)
    b, _ = _net(kind, dev)
    b.load_state_dict({k: v.clone() for k, v in a.state_dict().items()})
    return a, b, S


@pytest.mark.parametrize("net,kind", [("densenet", "asl"), ("densenet", "focal"), ("efficientnet", "asl")])
def test_fused_step_equals_the_autograd_route(dev, net, kind):
    from chexpert_amd import ops
    from chexpert_amd.loss import AsymmetricLoss, FocalLoss, MaskedBCE
    a, b, S = _twin(net, dev)
    B = 4
    x = synth.xray_batch(1500, B, S).to(dev)
    t = _targets(1510, B, 5, ignored=0.25).to(dev)
    assert (t < 0).any() and (t >= 0).any()
    w = synth.uniform(1520, (5,), 0.5, 8.0).to(dev)
    keys = list(a.state_dict().keys())
    if kind == "asl":
        assert a.set_loss(kind="asl", gamma_pos=1.0, gamma_neg=4.0, clip=0.05, pos_weight=w) is a
        crit, P = AsymmetricLoss(1.0, 4.0, 0.05, pos_weight=w), (1.0, 4.0, 0.05, None)
    else:
        assert a.set_loss(kind="focal", gamma=2.0, alpha=0.25, pos_weight=w) is a
        crit, P = FocalLoss(2.0, 0.25, pos_weight=w), (2.0, 2.0, 0.0, 0.25)
    assert list(a.state_dict().keys()) == keys and a.loss_step_state() == []      # neither buffer nor parameter; nothing per step
    assert a.loss_kind == kind and tuple(a.loss_focus.shape) == (4,) and a.loss_focus.is_cuda and a.loss_focus.dtype == torch.float32
    assert torch.equal(a.loss_focus, _focus(P, dev)) and torch.equal(a.loss_pos_weight, w) and a.loss_pos_weight.data_ptr() != w.data_ptr()
    loss_a, logits_a = a.forward_backward(x, t)
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
    ref, le_ref, _ = oracle(logits_a.cpu(), t.cpu(), w.cpu(), P)
    print("%s %s: fused loss %.7f, float64 oracle %.7f" % (net, kind, loss_a.item(), ref.item()))
    assert abs(loss_a.item() - ref.item()) <= 1e-5 * max(1.0, abs(ref.item()))
    le = crit.elementwise(out, t)
    assert not le.requires_grad and tuple(le.shape) == (B, 5)
    close(le.cpu().double(), le_ref, rel=1e-5, what="elementwise")
    # backward scales by the incoming gradient
    xl = logits_a.clone().requires_grad_(True)
    (3.0 * crit(xl, t)).backward()
    dl = torch.empty_like(logits_a)
    ops.asl_fwd_bwd(logits_a, t, w, a.loss_focus, None, None, dl)
    assert torch.equal(xl.grad, dl * 3.0)
    # teeth: these are not the cross-entropy's gradients
    gk = {k: v.grad.clone() for k, v in gb.items()}
    b.zero_grad(set_to_none=True)
    MaskedBCE(w)(b(x), t).backward()
    assert sum(int(not torch.equal(gb[k].grad, gk[k])) for k in gb) > len(gb) // 2
    # loss_state() carries the four numbers; a repeated set_loss keeps the storage a captured step reads
    st = a.loss_state()
    assert st["kind"] == kind and not st["focus"].is_cuda and torch.equal(st["focus"], a.loss_focus.cpu())
    assert b.load_loss_state(st) is b and b.loss_kind == kind and torch.equal(b.loss_focus, a.loss_focus) and b.loss_pos_weight is None
    held, held_w = a.loss_focus.data_ptr(), a.loss_pos_weight.data_ptr()
    if kind == "asl":
        a.set_loss(kind="asl", gamma_neg=2.0, pos_weight=2 * w)
        assert [round(v, 6) for v in a.loss_focus.tolist()] == [0.0, 2.0, 0.05, -1.0]
    else:
        a.set_loss(kind="focal", gamma=1.0, pos_weight=2 * w)
        assert a.loss_focus.tolist() == [1.0, 1.0, 0.0, -1.0]
    assert a.loss_focus.data_ptr() == held and a.loss_pos_weight.data_ptr() == held_w and torch.equal(a.loss_pos_weight, 2 * w)
    with pytest.raises(ValueError):                                     # refused: nothing changes
        a.set_loss(kind=kind, pos_weight=[1.0] * 4)
    assert a.loss_kind == kind and torch.equal(a.loss_pos_weight, 2 * w)
    # set_loss() puts the plain loss back: the step is the one of a model that never heard of it
    assert a.set_loss() is a and (a.loss_kind, a.loss_focus, a.loss_pos_weight, a.loss_ignore_negative) == ("bce", None, None, False)
    assert a.loss_state() == {"kind": "bce", "aux": None, "prior": None, "margin": 1.0, "lr_aux": None}
    b.set_loss()
    a.zero_grad(set_to_none=True)
    b.zero_grad(set_to_none=True)
    t01 = synth.targets(1530, B, 5).to(dev)
    la, _ = a.forward_backward(x, t01)
    lb, _ = b.forward_backward(x, t01)
    assert torch.equal(la, lb)
    for k in ga:
        assert torch.equal(ga[k].grad, gb[k].grad), k


def test_eval_mode_step_with_input_grad(dev):
    """The frozen-BatchNorm step under the asymmetric loss fills the input gradient; it is the autograd route's x.grad."""
    from chexpert_amd.loss import AsymmetricLoss
    a, b, S = _twin("densenet", dev)
    B = 4
    x = synth.xray_batch(1600, B, S).to(dev)
    t = _targets(1610, B, 5, ignored=0.25).to(dev)
    a.set_loss(kind="asl")
    a.eval()
    b.eval()
    buf = torch.full((B, 3, S, S), 7.0, device=dev)
    loss, logits = a.forward_backward(x, t, input_grad=buf)
    assert math.isfinite(loss.item()) and bool(torch.isfinite(buf).all()) and float(buf.abs().max()) > 0 and not bool((buf == 7.0).any())
    assert float(a.classifier.weight.grad.abs().max()) > 0
    xb = x.clone().requires_grad_(True)
    lb = AsymmetricLoss()(b(xb), t)
    lb.backward()
    assert torch.equal(lb.detach(), loss.reshape(())) and torch.equal(xb.grad, buf)


def test_set_loss_walk_leaves_nothing_of_the_previous_kind(dev):
    """set_loss walked across the kinds, twice: plain -> ignore_negative -> pos_weight -> focal(pos_weight) -> aucm -> asl (no
    weights) -> pos_weight only -> plain.  After every move the public attributes are the documented ones (None where the kind
    has none; the margin is passed by value to 'aucm' alone and stays what the last 'aucm' made it), the step's loss and
    d loss / d logits are those of the matching loss module on the same logits, bit for bit, and the held storage of a second visit
    is that of the first."""
    from chexpert_amd.loss import AsymmetricLoss, AUCMLoss, FocalLoss, MaskedBCE
    model, S = _net("densenet", dev)
    B, n = 2, 5
    x = synth.xray_batch(1700, B, S).to(dev)
    t = _targets(1710, B, n, ignored=0.3).to(dev)
    assert (t < 0).any() and (t >= 0).any()
    w1, w2, w3 = (synth.uniform(1720 + i, (n,), 0.5, 8.0) for i in range(3))
    prior = synth.uniform(1730, (n,), 0.1, 0.9)
    zeros = torch.zeros(3, n)
    f32 = lambda *v: torch.tensor(v, dtype=torch.float32)                                                     # noqa: E731
    # (name, set_loss keywords, the loss module, then what the model must hold: ignore_negative, pos_weight, aux, prior, lr_aux, focus)
    walk = [("bce", {}, lambda: MaskedBCE(ignore_negative=False), False, None, None, None, None, None),
            ("bce", dict(ignore_negative=True), lambda: MaskedBCE(), True, None, None, None, None, None),
            ("bce", dict(pos_weight=w1), lambda: MaskedBCE(w1, ignore_negative=False), False, w1, None, None, None, None),
            ("focal", dict(kind="focal", gamma=1.5, alpha=0.25, pos_weight=w2), lambda: FocalLoss(1.5, 0.25, pos_weight=w2),
             True, w2, None, None, None, f32(1.5, 1.5, 0.0, 0.25)),
            ("aucm", dict(kind="aucm", prior=prior, margin=0.7, lr_aux=0.05), lambda: AUCMLoss(prior, 0.7).to(dev),
             True, None, zeros, prior, f32(0.05), None),
            ("asl", dict(kind="asl"), lambda: AsymmetricLoss(), True, None, None, None, None, f32(0.0, 4.0, 0.05, -1.0)),
            ("bce", dict(pos_weight=w3), lambda: MaskedBCE(w3, ignore_negative=False), False, w3, None, None, None, None),
            ("bce", {}, lambda: MaskedBCE(ignore_negative=False), False, None, None, None, None, None)]
    eng, seen, ptrs = model._eng(), [], {}
    backward = eng.backward

    def spy(ws, dl, dx=None):                                           # d loss / d logits, as the step hands it to the backward pass
        seen.append(dl.clone())
        return backward(ws, dl, dx=dx)
    eng.backward = spy
    margin = 1.0
    for visit in range(2):
        for kind, kw, make, ign, w, aux, pr, lr, focus in walk:
            assert model.set_loss(**kw) is model
            margin = kw.get("margin", margin)
            assert (model.loss_kind, model.loss_ignore_negative, model.loss_margin) == (kind, ign, margin), (visit, kw)
            for name, want in (("loss_pos_weight", w), ("loss_aux", aux), ("loss_prior", pr), ("loss_lr_aux", lr), ("loss_focus", focus),
                               ("_loss_daux", aux)):
                got = getattr(model, name)
                assert (got is None) == (want is None), (visit, kw, name)
                if got is not None:
                    assert got.is_cuda and got.dtype == torch.float32 and tuple(got.shape) == tuple(want.shape), (visit, kw, name)
                    assert name == "_loss_daux" or torch.equal(got.cpu(), want), (visit, kw, name)
                    assert ptrs.setdefault(name, got.data_ptr()) == got.data_ptr(), (visit, kw, name)
            assert model.loss_state()["kind"] == kind and model.loss_step_state() == ([model.loss_aux] if kind == "aucm" else [])
            model.zero_grad(set_to_none=True)
            loss, logits = model.forward_backward(x, t)
            crit = make()
            xl = logits.clone().requires_grad_(True)
            lm = crit(xl, t)
            lm.backward()
            assert torch.equal(lm.detach(), loss.reshape(())) and torch.equal(xl.grad, seen[-1]), (visit, kw)
            assert math.isfinite(loss.item()) and float(seen[-1].abs().max()) > 0
            if kind == "aucm":                                          # the train-mode step has moved the scalars: a later kind must not see them
                assert float(model.loss_aux.abs().max()) > 0
    assert len(seen) == 2 * len(walk) and set(ptrs) == {"loss_pos_weight", "loss_aux", "loss_prior", "loss_lr_aux", "loss_focus", "_loss_daux"}


def test_graphed_step_sees_focus_changes_and_ignored_targets(dev):
    from chexpert_amd.graph import GraphedTrainStep
    from chexpert_amd.optim import FusedAdam
    m_e, m_g, S = _twin("densenet", dev)
    B, c = 4, 2
    xs = [synth.xray_batch(1700 + i, B, S).to(dev) for i in range(3)]
    ts = [_targets(1710 + 10 * i, B, 5, ignored=0.25).to(dev) for i in range(3)]
    for t in ts:
        t[:, c] = -1.0                                                  # a whole class ignored
    w = synth.uniform(1720, (5,), 0.5, 8.0).to(dev)
    for m in (m_e, m_g):
        m.set_loss(kind="asl", gamma_pos=0.0, gamma_neg=4.0, clip=0.05, pos_weight=w)
    opt_e, opt_g = FusedAdam(m_e, lr=1e-3), FusedAdam(m_g, lr=1e-3)
    # captured on a batch WITHOUT ignored labels: what a replay reads is the target copied in, not the one captured
    gs = GraphedTrainStep(m_g, opt_g, xs[0], synth.targets(1730, B, 5).to(dev))
    held = m_g.loss_focus.data_ptr()
    flat = lambda m: torch.cat([p.detach().flatten() for p in m.parameters()])
    for i in range(2):
        le = _eager_dev_step(m_e, opt_e, xs[i], ts[i])
        lg, _ = gs.replay(xs[i], ts[i])
        assert torch.equal(le, lg), (i, le.item(), lg.item())
        assert torch.equal(flat(m_e), flat(m_g)), i
        # the ignored class left no gradient contribution: its classifier row is exactly 0, the others are not
        for m in (m_e, m_g):
            gw, gb = m.classifier.weight.grad, m.classifier.bias.grad
            assert bool((gw[c] == 0).all()) and gb[c].item() == 0.0
            assert all(float(gw[k].abs().max()) > 0 and gb[k].item() != 0.0 for k in range(5) if k != c)
        assert torch.equal(m_e._eng().flat_grad, m_g._eng().flat_grad)
    # gamma- changes in place: the next replay reads the new value and matches an eager step at gamma- = 2
    m_g.loss_focus[1] = 2
    m_e.set_loss(kind="asl", gamma_pos=0.0, gamma_neg=2.0, clip=0.05, pos_weight=w)
    assert m_g.loss_focus.data_ptr() == held and torch.equal(m_g.loss_focus, m_e.loss_focus)
    le = _eager_dev_step(m_e, opt_e, xs[2], ts[2])
    lg, _ = gs.replay(xs[2], ts[2])
    assert torch.equal(le, lg) and torch.equal(flat(m_e), flat(m_g))
    # ... and it matters: the same logits under gamma- = 4 give another loss
    from chexpert_amd.loss import AsymmetricLoss
    m_g.eval()
    with torch.no_grad():
        out = m_g(xs[2])
    assert AsymmetricLoss(0.0, 2.0, 0.05, w)(out, ts[2]).item() != AsymmetricLoss(0.0, 4.0, 0.05, w)(out, ts[2]).item()


# ------------------------------------------------------------------------------------------------ data parallel
def _dp_worker(rank, world, port, out_dir):
    import torch.distributed as dist
    os.environ["MASTER_ADDR"], os.environ["MASTER_PORT"] = "127.0.0.1", str(port)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    from chexpert_amd.parallel import broadcast_module_state
    dev = torch.device("cuda:0")
    model, S = _net("densenet", dev)
    broadcast_module_state(model)
    x = synth.xray_batch(2100 + rank, 4, S).to(dev)
    t = _targets(2200 + 10 * rank, 4, 5, ignored=0.3).to(dev)
    t[:, rank] = -1.0                                     # each rank ignores a whole class of its own
    model.set_loss(kind="asl", gamma_pos=1.0, gamma_neg=4.0, clip=0.05, pos_weight=synth.uniform(9, (5,), 0.5, 8.0))
    _, logits = model.forward_backward(x, t)              # binds the engine; the single-process gradient of this shard, no reducer yet
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
                "n_ignored": int((t < 0).sum()), "n_buckets": len(eng.reducer.ranges)}, os.path.join(out_dir, "rank%d.pt" % rank))
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
    """Two ranks on one GPU: the gradients the reducer leaves on both ranks are the mean of the two single-process gradients (each
    shard's own forward_backward without a reducer), to the bound of the masked BCE's data-parallel test.  That mean is the gradient
    of the joined batch under data-parallel semantics -- BatchNorm statistics per rank -- and the loss kernel's own share of the
    statement holds bit for bit: on the joined logits (B = 8) it returns each shard's dlogits at grad_scale 1/2, and the mean of the
    two losses."""
    from chexpert_amd import ops
    port = 36100 + (os.getpid() % 400)
    _spawn_with_time_limit(_dp_worker, (2, port, str(tmp_path)), 2, 300)
    recs = [torch.load(os.path.join(str(tmp_path), "rank%d.pt" % r)) for r in range(2)]
    assert not torch.equal(recs[0]["local"], recs[1]["local"])
    for r, rec in enumerate(recs):
        assert rec["same"], "ranks ended with different gradients"
        assert rec["n_buckets"] >= 3 and rec["n_ignored"] >= 4
        g, w = rec["got"].double(), rec["want"].double()
        rel = float((g - w).norm() / w.norm())
        print("rank %d: rel %.3e, %d ignored labels, %d buckets" % (r, rel, rec["n_ignored"], rec["n_buckets"]))
        assert rel < 1e-6, rel
    # the joined batch through the loss kernel
    w, fo = synth.uniform(9, (5,), 0.5, 8.0).to(dev), _focus((1.0, 4.0, 0.05, None), dev)
    xj, tj = torch.cat([r["logits"] for r in recs]).to(dev), torch.cat([r["t"] for r in recs]).to(dev)
    lj, dj = torch.zeros(1, device=dev), torch.zeros(8, 5, device=dev)
    ops.asl_fwd_bwd(xj, tj, w, fo, lj, None, dj)
    halves, losses = [], []
    for r in recs:
        l, d = torch.zeros(1, device=dev), torch.zeros(4, 5, device=dev)
        ops.asl_fwd_bwd(r["logits"].to(dev), r["t"].to(dev), w, fo, l, None, d, grad_scale=0.5)
        halves.append(d)
        losses.append(l.item())
    assert torch.equal(dj, torch.cat(halves)) and float(dj.abs().max()) > 0
    assert abs(lj.item() - 0.5 * (losses[0] + losses[1])) <= 1e-6 * max(1.0, abs(lj.item()))


# ------------------------------------------------------------------------------------------------ command line
def _losses(capsys):
    out = capsys.readouterr().out
    return [json.loads(l)["train_loss"] for l in out.splitlines() if l.startswith('{"step"')]


_CLI = ["--train", "--synthetic", "32", "--batch_size", "4", "--resize", "64", "--eval_interval", "8", "--log_interval", "1", "--seed", "3",
        "--lr", "0.001"]


def test_cli_graphed_run_with_mixup_checkpoints_and_restores(dev, tmp_path, capsys):
    from chexpert_amd import cli
    capsys.readouterr()
    out = str(tmp_path / "g")
    flags = ["--loss", "asl", "--mixup", "0.2", "--uncertain", "ignore", "--synthetic_uncertain", "0.2", "--fused_optimizer", "--graph"]
    model = cli.main(_CLI + flags + ["--asl_gamma_neg", "3", "--asl_clip", "0.1", "--output_dir", out])
    lg = _losses(capsys)
    assert len(lg) == 8 and all(math.isfinite(v) for v in lg), lg
    assert model.loss_kind == "asl" and model.loss_pos_weight is None
    cfg = json.load(open(os.path.join(out, "config.json")))
    assert cfg["loss"] == "asl" and cfg["asl_gamma_neg"] == 3.0 and cfg["asl_clip"] == 0.1 and cfg["asl_gamma_pos"] is None and cfg["mixup"] == 0.2
    st = torch.load(os.path.join(out, "checkpoint_latest.pt"), map_location="cpu")["loss_state"]
    assert st["kind"] == "asl" and torch.equal(st["focus"], torch.tensor([0.0, 3.0, 0.1, -1.0]))
    res = json.load(open(os.path.join(out, "eval_results_step_8.json")))
    assert len(res["aucs"]) == 5 and all(math.isfinite(v) for v in res["loss"].values())      # evaluation keeps the BCE element losses
    # --restore checks the kind and puts the checkpoint's numbers back (this run's flags are the defaults 0 / 4 / 0.05)
    ck = os.path.join(out, "checkpoint_latest.pt")
    out2 = str(tmp_path / "r")
    model2 = cli.main(_CLI + flags + ["--restore", ck, "--output_dir", out2])
    lr_ = _losses(capsys)
    assert len(lr_) == 8 and all(math.isfinite(v) for v in lr_), lr_
    assert model2.loss_kind == "asl" and torch.equal(model2.loss_focus.cpu(), st["focus"])
    st2 = torch.load(os.path.join(out2, "checkpoint_latest.pt"), map_location="cpu")
    assert st2["global_step"] == 16 and st2["loss_state"]["kind"] == "asl" and torch.equal(st2["loss_state"]["focus"], st["focus"])
    with pytest.raises(ValueError, match="--loss asl.*--loss focal"):
        cli.main(_CLI + ["--loss", "focal", "--fused_optimizer", "--restore", ck, "--output_dir", str(tmp_path / "x")])


def test_cli_autograd_route_is_the_same_kernel(dev, tmp_path, capsys):
    """Without --fused_optimizer the loss module computes the loss: the first batch's loss line is the fused route's."""
    from chexpert_amd import cli
    capsys.readouterr()
    flags = ["--loss", "focal", "--focal_gamma", "1.5", "--focal_alpha", "0.25", "--pos_weight", "auto", "--uncertain", "ignore",
             "--synthetic_uncertain", "0.2", "--synthetic", "16", "--eval_interval", "4"]
    m1 = cli.main(_CLI + flags + ["--output_dir", str(tmp_path / "e")])
    le = _losses(capsys)
    m2 = cli.main(_CLI + flags + ["--fused_optimizer", "--output_dir", str(tmp_path / "f")])
    lf = _losses(capsys)
    assert len(le) == len(lf) == 4 and all(math.isfinite(v) for v in le + lf) and le[0] == lf[0], (le, lf)
    for m in (m1, m2):
        assert m.loss_kind == "focal" and m.loss_focus.tolist() == [1.5, 1.5, 0.0, 0.25] and m.loss_pos_weight is not None
    st = torch.load(os.path.join(str(tmp_path / "e"), "checkpoint_latest.pt"), map_location="cpu")["loss_state"]
    assert st["kind"] == "focal" and st["focus"].tolist() == [1.5, 1.5, 0.0, 0.25]


def test_cli_default_flags_never_reach_the_new_kernel(dev, tmp_path, capsys, monkeypatch):
    from chexpert_amd import cli, ops

    def refuse(*a, **k):
        raise AssertionError("ops.asl_fwd_bwd was reached without --loss focal|asl")
    monkeypatch.setattr(ops, "asl_fwd_bwd", refuse)
    capsys.readouterr()
    out = str(tmp_path / "p")
    model = cli.main(_CLI[:2] + ["16"] + _CLI[3:] + ["--eval_interval", "4", "--fused_optimizer", "--graph", "--output_dir", out])
    lp = _losses(capsys)
    assert len(lp) == 4 and all(math.isfinite(v) for v in lp), lp
    assert model.loss_kind == "bce" and model.loss_focus is None
    assert "loss_state" not in torch.load(os.path.join(out, "checkpoint_latest.pt"), map_location="cpu")
    cfg = json.load(open(os.path.join(out, "config.json")))
    assert cfg["loss"] == "bce" and cfg["focal_gamma"] is None and cfg["asl_clip"] is None
    # the patch has teeth: this is the name FusedNet.forward_backward and the loss modules call
    model.set_loss(kind="asl")
    x, t = synth.xray_batch(1800, 4, 64).to(dev), synth.targets(1810, 4, 5).to(dev)
    with pytest.raises(AssertionError, match="was reached"):
        model.forward_backward(x, t)
