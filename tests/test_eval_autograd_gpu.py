"""GPU: autograd through the fused networks in eval mode (BatchNorm frozen at its running statistics) -- the frozen-statistics
coefficient kernel (cx_bn_bwd_coef_eval) against a closed form, x.grad and every parameter's .grad of every fused network form
against the CPU oracle (torch autograd through oracle/nets.py with train=False), and the contracts of the eval autograd path:
bit-identical logits, no state moves, frozen parameters, forward_backward parity, determinism and the Grad-CAM hook path."""
import pytest
import torch

from chexpert_amd import synth

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    from chexpert_amd import _lib
    _lib.lib()
    return torch.device("cuda:0")


# ------------------------------------------------------------------------------------------------------------ the kernel
@pytest.mark.parametrize("C,R,rstride,with_gamma,q", [(64, 1, 0, True, (0, 64)), (200, 300, 208, True, (40, 96)),
                                                      (37, 70, 37, False, None), (1280, 16, 1280, True, (1248, 32))])
def test_bn_bwd_coef_eval_closed_form(dev, C, R, rstride, with_gamma, q):
    """Random statistic rows (multiples of 1/64: their fp32 sums are exact), a basis (mean, rstd) different from the running
    statistics: dgamma += S2 * r / r_b + r * (mu_b - m) * S1, dbeta += S1, pa = gamma * r (bit-equal to bn_coef_eval's scale),
    pb = pc = 0, slice coefficients (1, 0, 0) inside the range and untouched outside."""
    from chexpert_amd import ops
    rows = max(R, 1)
    pitch = rstride if R > 1 else C
    s1r = (torch.randint(-64, 65, (rows, pitch), generator=torch.Generator().manual_seed(1)).float() / 64)
    s2r = (torch.randint(-64, 65, (rows, pitch), generator=torch.Generator().manual_seed(2)).float() / 64)
    mb, rb = synth.uniform(3, (C,), -1.0, 1.0), synth.uniform(4, (C,), 0.5, 2.0)
    rm, rv = synth.uniform(5, (C,), -1.0, 1.0), synth.uniform(6, (C,), 0.2, 3.0)
    gamma = synth.uniform(7, (C,), 0.5, 1.5) if with_gamma else None
    dg0, db0 = synth.uniform(8, (C,), -1.0, 1.0), synth.uniform(9, (C,), -1.0, 1.0)
    eps = 1e-5
    d = lambda t: None if t is None else t.to(dev)
    dg, db = d(dg0.clone()), d(db0.clone())
    pa, pb, pc = (torch.full((C,), 7.0, device=dev) for _ in range(3))
    qn = q[1] if q else 0
    qv = [torch.full((qn + 4,), 7.0, device=dev) for _ in range(3)]
    ops.bn_bwd_coef_eval(d(s1r), d(s2r), d(mb), d(rb), d(rm), d(rv), d(gamma), eps, dg, db, pa, pb, pc, C, replicas=R, rstride=rstride,
                         q=(qv[0][:qn], qv[1][:qn], qv[2][:qn], q[0], qn) if q else None)
    S1, S2 = s1r[:, :C].double().sum(0), s2r[:, :C].double().sum(0)
    r = 1.0 / torch.sqrt(rv.double() + eps)
    ref_dg = dg0.double() + S2 * r / rb.double() + r * (mb.double() - rm.double()) * S1
    ref_db = db0.double() + S1
    rel = lambda a, b: (a.cpu().double() - b).abs().max().item() / b.abs().max().item()
    print("C %d R %d: dgamma rel %.2e, dbeta rel %.2e" % (C, R, rel(dg, ref_dg), rel(db, ref_db)))
    assert rel(dg, ref_dg) <= 1e-6 and rel(db, ref_db) <= 1e-6
    sc = torch.empty(C, device=dev)
    ops.bn_coef_eval(d(rm), d(rv), d(gamma), None, eps, sc, None, None, None, C)
    assert torch.equal(pa, sc)
    assert not pb.any() and not pc.any()
    if q:
        assert torch.equal(qv[0][:qn], torch.ones(qn, device=dev)) and not qv[1][:qn].any() and not qv[2][:qn].any()
        assert all(bool((t[qn:] == 7.0).all()) for t in qv)
    # basis = the running statistics: dgamma gets exactly S2 (what the ResNet / EfficientNet slots hold in eval mode)
    rstd = torch.empty(C, device=dev)
    ops.bn_coef_eval(d(rm), d(rv), None, None, eps, None, None, None, rstd, C)
    dg2 = d(dg0.clone())
    ops.bn_bwd_coef_eval(d(s1r), d(s2r), d(rm), rstd, d(rm), d(rv), d(gamma), eps, dg2, None, None, None, None, C, replicas=R,
                         rstride=rstride)
    assert torch.equal(dg2, d(dg0) + d(s2r[:, :C].sum(0)))


# ------------------------------------------------------------------------------------------------------------ the networks
ATTN = dict(k=.2, v=.1, nh=8)
WRN_ATTN = dict(k=0.5, v=0.25, nh=4)


def _dense(cfg, S, n_cls, growth=32, init=64, attn=None, drop_rate=0.0):
    from chexpert_amd.models import DenseNet
    from oracle import nets
    spec = nets.densenet_spec(n_cls, growth=growth, block_config=cfg, init_features=init, attn=attn, input_hw=(S, S))
    model = DenseNet(growth, cfg, init, num_classes=n_cls, drop_rate=drop_rate,
                     attn_params=dict(attn, relative=True, input_dims=(S, S)) if attn else None)
    nh = attn["nh"] if attn else None
    return spec, model, 2.5, lambda s, x, q=None: nets.densenet_forward(s, x, cfg, train=False, nh=nh, q=q)


def _resnet(layers, S, n_cls):
    from chexpert_amd.models import Bottleneck, ResNet
    from oracle import nets
    return (nets.resnet_spec(n_cls, layers=layers, input_hw=(S, S)), ResNet(Bottleneck, list(layers), num_classes=n_cls), 1.0,
            lambda s, x, q=None: nets.resnet_forward(s, x, layers, train=False, q=q))


def _wrn(S, n_cls, attn=None):
    from chexpert_amd.models import BasicBlock, WideResNet
    from oracle import nets
    model = WideResNet(BasicBlock, 16, 4, num_classes=n_cls, attn_params=dict(attn, relative=True, input_dims=(S, S)) if attn else None)
    nh = attn["nh"] if attn else None
    return (nets.basic_resnet_spec(n_cls, wide=(16, 4), attn=attn, input_hw=(S, S)), model, 1.0,
            lambda s, x, q=None: nets.basic_resnet_forward(s, x, wide=(16, 4), train=False, nh=nh, q=q))


def _effnet(name, n_cls, drop=False):
    from chexpert_amd.models import construct_model
    from chexpert_amd.models.efficientnet import DropMarker
    from oracle import nets
    model = construct_model(name, n_cls)
    if not drop:
        for mod in model.modules():
            if isinstance(mod, DropMarker):
                mod.p = 0.0
    # (the EfficientNet oracle has no storage-rounding model: q is ignored)
    return nets.efficientnet_spec(name, n_cls), model, 1.0, lambda s, x, q=None: nets.efficientnet_forward(s, x, name, train=False)


NETS = {  # tag -> (builder, B, S)
    "densenet2222_64": (lambda n: _dense((2, 2, 2, 2), 64, n), 4, 64),
    "densenet2222_64_drop": (lambda n: _dense((2, 2, 2, 2), 64, n, drop_rate=0.2), 4, 64),
    "densenet121_320": (lambda n: _dense((6, 12, 24, 16), 320, n), 2, 320),
    "aadensenet6422_64": (lambda n: _dense((6, 4, 2, 2), 64, n, attn=ATTN), 8, 64),
    "resnet1111_64": (lambda n: _resnet((1, 1, 1, 1), 64, n), 4, 64),
    "efficientnet-b0_224": (lambda n: _effnet("efficientnet-b0", n), 2, 224),
    "efficientnet-b0_224_drop": (lambda n: _effnet("efficientnet-b0", n, drop=True), 2, 224),
    "wrn16_4_32": (lambda n: _wrn(32, n), 4, 32),
    "aawrn16_4_32": (lambda n: _wrn(32, n, WRN_ATTN), 8, 32),
    "densenetbc_L40_32": (lambda n: _dense((6, 6, 6), 32, n, growth=12, init=24), 4, 32),
}


def _calibrate(model, x):
    """Running statistics in the network's operating range: one train-mode forward (no_grad) at momentum 1 on another batch,
    then a per-BatchNorm jitter (mean +- 5 %, variance x 0.9 .. 1.1), so that the consumers of a dense-block channel hold different
    running statistics and the frozen backward's basis correction is exercised."""
    bns = [m for m in model.modules() if isinstance(m, torch.nn.BatchNorm2d)]
    moms = [m.momentum for m in bns]
    for m in bns:
        m.momentum = 1.0
    model.train()
    with torch.no_grad():
        model(x)
    for m, mom in zip(bns, moms):
        m.momentum = mom
    with torch.no_grad():
        for i, m in enumerate(bns):
            C = m.num_features
            m.running_mean.add_(synth.uniform(100 + i, (C,), -0.05, 0.05).to(m.running_mean.device) * m.running_var.sqrt())
            m.running_var.mul_(synth.uniform(5000 + i, (C,), 0.9, 1.1).to(m.running_var.device))


def _make(tag, dtype, dev, n_cls=5):
    from oracle import nets
    build, B, S = NETS[tag]
    spec, model, bias, fwd = build(n_cls)
    sd = synth.smooth_state_dict_(synth.fill_state_dict_(nets.zeros_state_dict(spec), 21), bias)
    model.load_state_dict(sd, strict=True)
    model = model.storage_dtype(dtype).to(dev)
    _calibrate(model, synth.xray_batch(777, B, S).to(dev))
    model.eval()
    sd = {k: v.detach().cpu().clone() for k, v in model.state_dict().items()}
    x, t = synth.xray_batch(1234, B, S), synth.targets(99, B, n_cls)
    return model, sd, fwd, x, t


def _oracle(fwd, sd, x, t, q=None):
    """(x.grad, {name: .grad}) of the eval-mode oracle: F.batch_norm with the running statistics, autograd on CPU; q: the oracle's
    storage-rounding model (nets.bf16_storage) or None."""
    from oracle import step
    sd = {k: v.clone() for k, v in sd.items()}
    names = step.trainable(sd)
    for k in names:
        sd[k].requires_grad_(True)
    xr = x.clone().requires_grad_(True)
    loss = step.bce_sum_mean(fwd(sd, xr, q=q), t)
    gs = torch.autograd.grad(loss, [xr] + [sd[k] for k in names])
    return gs[0], dict(zip(names, gs[1:]))


def _eval_step(model, x, t, dev, x_grad=True):
    from oracle import step
    model.zero_grad(set_to_none=True)
    xg = x.to(dev).requires_grad_(x_grad)
    logits = model(xg)
    loss = step.bce_sum_mean(logits, t.to(dev))
    loss.backward()
    grads = {k: (p.grad.clone() if p.grad is not None else None) for k, p in model.named_parameters()}
    return logits.detach(), loss.detach(), grads, (xg.grad.clone() if x_grad else None)


def _cmp(got, ref):
    a, b = got.double().flatten().cpu(), ref.double().flatten()
    cos = float((a * b).sum() / (a.norm() * b.norm()))
    return cos, float(a.norm() / b.norm())


def _check_against_oracle(tag, dtype, dev, cos_min, nr_tol, q=None):
    model, sd, fwd, x, t = _make(tag, dtype, dev)
    _, _, grads, dx = _eval_step(model, x, t, dev)
    dx_o, grads_o = _oracle(fwd, sd, x, t, q)
    bad = []
    cos, nr = _cmp(dx, dx_o)
    print("%s %s eval x.grad: cos %.6f, norm ratio %.5f" % (tag, dtype, cos, nr))
    if cos < cos_min or abs(nr - 1) > nr_tol:
        bad.append(("x", cos, nr))
    gmax = max(g.norm().item() for g in grads_o.values())
    worst = (2.0, 0.0, "")
    for k, g in grads.items():
        assert g is not None, k
        if grads_o[k].norm().item() <= 1e-6 * gmax:           # (no signal to compare: e.g. parameters that only feed zeros)
            continue
        cos, nr = _cmp(g, grads_o[k])
        worst = min(worst, (cos, nr, k))
        if cos < cos_min or abs(nr - 1) > nr_tol:
            bad.append((k, cos, nr))
    print("%s %s eval parameter gradients: worst cos %.6f (norm ratio %.5f) at %s" % (tag, dtype, *worst))
    assert not bad, bad[:8]


@pytest.mark.parametrize("tag", ["densenet2222_64", "densenet121_320", "aadensenet6422_64", "resnet1111_64", "efficientnet-b0_224",
                                 "densenetbc_L40_32"])
def test_fp32_eval_gradients_match_the_fp32_oracle(dev, tag):
    """x.grad and every parameter's .grad (BatchNorm weight / bias included) at the project's fp32 figure."""
    _check_against_oracle(tag, "fp32", dev, 0.9999, 1e-3)


@pytest.mark.parametrize("tag", ["densenet121_320", "aadensenet6422_64", "resnet1111_64", "efficientnet-b0_224", "wrn16_4_32",
                                 "aawrn16_4_32", "densenetbc_L40_32"])
def test_bf16_eval_gradients_smooth_regime(dev, tag):
    """bf16 storage against the oracle's bf16 storage-rounding model (nets.bf16_storage: input, weights, stored activations and
    normalised operands rounded as the kernels store them; not modelled in the attention layers nor in the EfficientNet oracle).
    Against the plain fp32 oracle the frozen-BatchNorm gradients of small-sample parameters (norm gains / biases of the 10x10 maps,
    the attention nets at B = 4) measure the storage rounding itself: cos 0.93-0.99 where the rounding model gives 0.98-0.9999, while
    every fp32-storage case above agrees to cos 1.000000."""
    from oracle import nets
    _check_against_oracle(tag, "bf16", dev, 0.97, 0.05, q=nets.bf16_storage)


@pytest.mark.parametrize("tag", ["densenet2222_64", "aadensenet6422_64", "resnet1111_64", "efficientnet-b0_224", "aawrn16_4_32",
                                 "densenetbc_L40_32"])
def test_eval_autograd_logits_equal_the_plain_eval_forward(dev, tag):
    model, _, _, x, t = _make(tag, "bf16", dev)
    xd = x.to(dev)
    with torch.no_grad():
        plain = model(xd)
    out = model(xd.clone().requires_grad_(True))
    assert out.grad_fn is not None
    assert torch.equal(out.detach(), plain)


def _state(model):
    eng = model._eng()
    eng = getattr(eng, "inner", eng)                      # (the channel-padded twin's engine holds the dropout seed)
    extra = {"nbt_pending": torch.tensor(model._nbt_pending)}
    for name in ("step_dev", "drop_seed"):
        if getattr(eng, name, None) is not None:
            extra[name] = getattr(eng, name).clone()
    return {k: v.clone() for k, v in model.state_dict().items()}, extra


@pytest.mark.parametrize("tag", ["densenet2222_64_drop", "resnet1111_64", "efficientnet-b0_224_drop", "densenetbc_L40_32"])
def test_eval_backward_moves_no_state(dev, tag):
    """After an eval forward + backward the running statistics, num_batches_tracked, the device mask counter and the dropout seed
    are bit-identical, and a following training step gives what the same step gives on an untouched copy."""
    model, _, _, x, t = _make(tag, "bf16", dev)
    copy, _, _, _, _ = _make(tag, "bf16", dev)
    sd0, ex0 = _state(model)
    _eval_step(model, x, t, dev)
    sd1, ex1 = _state(model)
    for k in sd0:
        assert torch.equal(sd0[k], sd1[k]), k
    for k in ex0:
        assert torch.equal(ex0[k], ex1[k]), k
    xd, td = x.to(dev), t.to(dev)
    res = []
    for m in (model, copy):
        m.train()
        m.zero_grad(set_to_none=True)
        loss, logits = m.forward_backward(xd, td)
        res.append((loss, logits, {k: p.grad.clone() for k, p in m.named_parameters()}, m.state_dict()))
    (l0, o0, g0, s0), (l1, o1, g1, s1) = res
    assert torch.equal(l0, l1) and torch.equal(o0, o1)
    for k in g0:
        assert torch.equal(g0[k], g1[k]), k
    for k in s0:
        assert torch.equal(s0[k], s1[k]), k


@pytest.mark.parametrize("tag", ["densenet2222_64", "resnet1111_64", "efficientnet-b0_224", "densenetbc_L40_32"])
def test_eval_frozen_parameters_give_x_grad_only(dev, tag):
    model, _, _, x, t = _make(tag, "bf16", dev)
    _, _, _, dx_u = _eval_step(model, x, t, dev)
    for p in model.parameters():
        p.requires_grad_(False)
    model.zero_grad(set_to_none=True)
    from oracle import step
    xg = x.to(dev).requires_grad_(True)
    step.bce_sum_mean(model(xg), t.to(dev)).backward()
    assert xg.grad is not None and torch.equal(xg.grad, dx_u) and xg.grad.abs().max() > 0
    assert all(p.grad is None for p in model.parameters())
    for p in model.parameters():                          # an existing .grad of a frozen parameter is left as it was
        p.grad = torch.full_like(p, 3.0)
    xg = x.to(dev).requires_grad_(True)
    step.bce_sum_mean(model(xg), t.to(dev)).backward()
    assert torch.equal(xg.grad, dx_u)
    assert all(bool((p.grad == 3.0).all()) for p in model.parameters())


@pytest.mark.parametrize("tag", ["densenet2222_64", "aadensenet6422_64", "resnet1111_64", "efficientnet-b0_224", "wrn16_4_32",
                                 "densenetbc_L40_32"])
def test_eval_forward_backward_matches_module_autograd(dev, tag):
    """forward_backward in eval mode is the frozen-BatchNorm step: loss, logits, parameter gradients and input_grad bit-equal to
    model(x) + backward with the fused loss kernel's logit gradient; two passes are bit-equal (determinism)."""
    from chexpert_amd import ops
    model, _, _, x, t = _make(tag, "bf16", dev)
    xd, td = x.to(dev), t.to(dev)
    runs = []
    for _ in range(2):
        model.zero_grad(set_to_none=True)
        buf = torch.full_like(xd, 7.0)
        loss, logits = model.forward_backward(xd, td, input_grad=buf)
        runs.append((loss, logits, {k: p.grad.clone() for k, p in model.named_parameters()}, buf))
    model.zero_grad(set_to_none=True)
    xg = xd.clone().requires_grad_(True)
    out = model(xg)
    loss_m = torch.empty(1, device=dev)
    dl = torch.empty_like(out)
    ops.bce_fwd_bwd(out.detach(), td, loss_m, None, dl)
    out.backward(dl)
    runs.append((loss_m, out.detach(), {k: p.grad.clone() for k, p in model.named_parameters()}, xg.grad))
    ref = runs[0]
    assert ref[3].abs().max() > 0
    for r in runs[1:]:
        assert torch.equal(r[0], ref[0]) and torch.equal(r[1], ref[1]) and torch.equal(r[3], ref[3])
        for k in ref[2]:
            assert torch.equal(r[2][k], ref[2][k]), k
    assert not model.training


def test_eval_double_backward_raises(dev):
    model, _, _, x, t = _make("densenet2222_64", "bf16", dev)
    from oracle import step
    loss = step.bce_sum_mean(model(x.to(dev).requires_grad_(True)), t.to(dev))
    with pytest.raises(RuntimeError, match="double backward"):
        loss.backward(create_graph=True)


@pytest.mark.parametrize("tag", ["densenet2222_64", "resnet1111_64", "efficientnet-b0_224"])
def test_grad_cam_hooks_keep_the_hooked_path(dev, tag):
    model, _, _, x, t = _make(tag, "bf16", dev)
    target = model.features.norm5 if hasattr(model, "features") else (model._stages()[-1] if hasattr(model, "_stages") else model.head[1])
    seen = []
    h = target.register_forward_hook(lambda mod, inp, out: seen.append(out.shape))
    try:
        out = model(x.to(dev))                            # eval, grad mode on, parameters requiring grad
    finally:
        h.remove()
    assert seen and type(out.grad_fn).__name__.startswith("_HookedLinear")
    with torch.no_grad():
        plain = model(x.to(dev))
    assert torch.equal(out.detach(), plain)
