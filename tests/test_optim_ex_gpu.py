"""GPU: global-norm gradient clipping, non-finite skip and weight EMA inside the optimiser launch (csrc/optim.hip:
cx_grad_norm, cx_*_step_ex, cx_*_step_dev_ex) and their wiring in chexpert_amd.optim, against torch.optim +
torch.nn.utils.clip_grad_norm_ on the CPU and float64 restatements."""
import math

import pytest
import torch

from chexpert_amd import synth

pytestmark = pytest.mark.gpu

KINDS = ["adam", "sgd_nesterov", "rmsprop"]
U = 2.0 ** -24                     # unit round-off of fp32


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    from chexpert_amd import _lib
    _lib.lib()          # fail loudly if the HIP library is missing
    return torch.device("cuda:0")


def rnd(seed, shape, lo=-1.0, hi=1.0):
    return synth.uniform(seed, shape, lo, hi)


def close(got, want, rel, what=""):
    scale = want.abs().max().item() + 1e-6
    err = (got.double() - want.double()).abs().max().item()
    assert err <= rel * scale, "%s: max err %.3e vs scale %.3e (rel %.2e)" % (what, err, scale, err / scale)


def ceil_div(a, b):
    return -(-a // b)


def norm_partials(n):
    """The grid of cx_grad_norm's first launch, restated: one workgroup per 1024 16-byte groups, at most 2048."""
    return 0 if n == 0 else min(2048, max(1, ceil_div(n // 4, 1024)))


def norm_bound(n):
    """Relative bound on the fp32 norm from the summation shape of the two launches: a sum of non-negative terms carries at most
    (number of roundings on the longest path of a term to the result) * 2^-24 of relative error.
    Launch 1, per thread: ceil(range / 256) fused multiply-adds into one of four accumulators, two additions that join the four,
    one more for the scalar tail; then 6 shuffle levels in the wave and 3 additions over the 4 waves.
    Launch 2, per thread: ceil(partials / 256) additions; then the same 6 + 3 fold.
    (The two roundings of (grad_scale * g)^2 and the square root's own are covered: the square root halves the relative error of
    the sum, and the path is always longer than 3.)"""
    blocks = max(1, norm_partials(n))
    per = ceil_div(n // 4, blocks)
    chain1 = ceil_div(per, 256) + 2 + 1
    chain2 = ceil_div(blocks, 256)
    folds = 6 + 3
    return (chain1 + folds + chain2 + folds) * U


def run_norm(ops, g, grad_scale=1.0, max_norm=0.0, skip=False, clip=None):
    ws = torch.zeros(max(1, ops.grad_norm_partials(g.numel())), device=g.device)
    if clip is None:
        clip = torch.zeros(4, device=g.device)
    ops.grad_norm(g, ws, clip, grad_scale, max_norm, skip)
    return clip


_G_BIG = {}


def g_big():
    if "g" not in _G_BIG:                 # one hash fill shared by every size: the cases are prefixes of it
        _G_BIG["g"] = rnd(500, (5000003 + 4,))
    return _G_BIG["g"]


# ------------------------------------------------------------------------------------------------ norm
@pytest.mark.parametrize("grad_scale", [1.0, 0.125])
@pytest.mark.parametrize("n", [1, 3, 255, 10007, 5000003])
def test_grad_norm_values_and_reproducible(dev, n, grad_scale):
    from chexpert_amd import ops
    assert ops.grad_norm_partials(n) == norm_partials(n)
    if n == 5000003:                       # ranges longer than one pass of a workgroup, and n % 4 != 0
        assert ceil_div(n // 4, norm_partials(n)) > 256 and n % 4
    g = g_big()[:n].clone()
    want = (g.double() * grad_scale).norm().item()
    gd = g.to(dev)
    a = run_norm(ops, gd, grad_scale).cpu()
    b = run_norm(ops, gd, grad_scale).cpu()
    err = abs(float(a[0]) - want) / want
    print("n %d scale %g: norm %.9g want %.9g rel err %.3e bound %.3e" % (n, grad_scale, float(a[0]), want, err, norm_bound(n)))
    assert err <= norm_bound(n)
    assert float(a[1]) == 1.0 and float(a[2]) == 0.0 and float(a[3]) == 0.0          # clipping off: coefficient 1
    assert torch.equal(a, b)                                                           # same bits on every call


def test_grad_norm_empty_and_misaligned(dev):
    from chexpert_amd import ops
    c = run_norm(ops, torch.zeros(0, device=dev), max_norm=1.0).cpu()
    assert c.tolist() == [0.0, 1.0, 0.0, 0.0]
    g = torch.ones(1025, device=dev)
    with pytest.raises(RuntimeError, match="16-byte aligned"):
        run_norm(ops, g[1:])                                     # a view offset by one float: refused before any launch
    assert float(run_norm(ops, g[4:]).cpu()[0]) == torch.tensor(1021.0).sqrt().item()      # 16 bytes on: accepted, the sum is exact


# ------------------------------------------------------------------------------------------------ the extended steps
def launch(ops, kind, form, p, g, st, it, lr=1e-2, hyper=None, ex=None, grad_scale=1.0):
    """One step of `kind` through the plain (ex None) or the extended entry point; it = 0-based step; form 'host' or 'dev'."""
    kw = {} if ex is None else ex
    sfx = "" if ex is None else "_ex"
    if form == "dev":
        if kind == "adam":
            getattr(ops, "adam_step_dev" + sfx)(p, g, st[0], st[1], hyper, 0.9, 0.999, 1e-8, 0.0, grad_scale, **kw)
        elif kind == "sgd_nesterov":
            getattr(ops, "sgd_nesterov_step_dev" + sfx)(p, g, st[0], hyper, 0.9, 0.0, grad_scale, **kw)
        else:
            getattr(ops, "rmsprop_step_dev" + sfx)(p, g, st[0], st[1], hyper, 0.99, 1e-3, 0.9, 0.0, grad_scale, **kw)
        ops.optim_tick(hyper)
        return
    if kind == "adam":
        getattr(ops, "adam_step" + sfx)(p, g, st[0], st[1], lr, 0.9, 0.999, 1e-8, 0.0, it + 1, grad_scale, **kw)
    elif kind == "sgd_nesterov":
        step = () if ex is None else (it + 1,)
        getattr(ops, "sgd_nesterov_step" + sfx)(p, g, st[0], lr, 0.9, 0.0, it == 0, *step, grad_scale, **kw)
    else:
        step = () if ex is None else (it + 1,)
        getattr(ops, "rmsprop_step" + sfx)(p, g, st[0], st[1], lr, 0.99, 1e-3, 0.9, 0.0, *step, grad_scale, **kw)


def plain_hyper(dev, lr=1e-2):
    return torch.tensor([lr, 0, 0, 1.0, 0, 0, 0, lr], dtype=torch.float32, device=dev)


# Each of the three checks below runs at n = 10007 (the test of its name) and, as `_small_n`, at n = 3: less than one 16-byte unit
# and less than a wave (the scalar tail of the norm carries the whole sum), and n = 257: one element past a workgroup (a second
# workgroup with a single live lane).  Same bounds.
SMALL_N = [3, 257]


def check_clipping_matches_clip_grad_norm(dev, kind, form, n):
    """Three steps, gradients one vector scaled by 1, 10 and 0.5, max_norm = 2 x the norm of the first: unclipped, clipped, unclipped.
    CPU: clip_grad_norm_(max_norm) then torch.optim's step (oracle.step.make_optimizer)."""
    from chexpert_amd import ops
    from oracle import step as ostep
    p0, g0 = rnd(620, (n,)), rnd(621, (n,))
    max_norm = 2.0 * g0.double().norm().item()
    pc = p0.clone().requires_grad_(True)
    opt, _ = ostep.make_optimizer(kind, [pc], 1e-2)
    p = p0.clone().to(dev)
    st = [torch.zeros(n, device=dev) for _ in range(2)]
    hyper = plain_hyper(dev)
    clip = torch.zeros(4, device=dev)
    ws = torch.zeros(ops.grad_norm_partials(n), device=dev)
    coefs = []
    for it, s in enumerate([1.0, 10.0, 0.5]):
        g = g0 * s
        pc.grad = g.clone()
        torch.nn.utils.clip_grad_norm_([pc], max_norm)
        opt.step()
        gd = g.to(dev)
        ops.grad_norm(gd, ws, clip, 1.0, max_norm, False)
        launch(ops, kind, form, p, gd, st, it, hyper=hyper, ex={"clip": clip})
        c = clip.cpu()
        norm64 = g.double().norm().item()
        coef64 = min(1.0, max_norm / (norm64 + 1e-6))
        coefs.append(float(c[1]))
        assert abs(float(c[0]) - norm64) <= norm_bound(n) * norm64
        assert abs(float(c[1]) - coef64) <= (norm_bound(n) + 3 * U) * coef64, (it, float(c[1]), coef64)
    assert coefs[0] == 1.0 and coefs[1] < 0.21 and coefs[2] == 1.0, coefs
    close(p.cpu(), pc.detach(), rel=2e-6 if form == "host" else 5e-6, what=kind)


@pytest.mark.parametrize("form", ["host", "dev"])
@pytest.mark.parametrize("kind", KINDS)
def test_clipping_matches_clip_grad_norm(dev, kind, form):
    check_clipping_matches_clip_grad_norm(dev, kind, form, 10007)


@pytest.mark.parametrize("n", SMALL_N)
@pytest.mark.parametrize("form", ["host", "dev"])
@pytest.mark.parametrize("kind", KINDS)
def test_clipping_matches_clip_grad_norm_small_n(dev, kind, form, n):
    check_clipping_matches_clip_grad_norm(dev, kind, form, n)


def check_ex_step_without_options_gives_the_plain_bits(dev, kind, form, n):
    from chexpert_amd import ops
    p0 = rnd(630, (n,)).to(dev)
    pa, pb = p0.clone(), p0.clone()
    sa = [torch.zeros(n, device=dev) for _ in range(2)]
    sb = [torch.zeros(n, device=dev) for _ in range(2)]
    ha, hb = plain_hyper(dev), plain_hyper(dev)
    for it in range(3):
        g = rnd(631 + it, (n,)).to(dev)
        launch(ops, kind, form, pa, g, sa, it, hyper=ha, grad_scale=0.5)
        launch(ops, kind, form, pb, g, sb, it, hyper=hb, ex={}, grad_scale=0.5)
        assert torch.equal(pa, pb), (kind, form, it)
        assert torch.equal(sa[0], sb[0]) and torch.equal(sa[1], sb[1]), (kind, form, it)
    assert not torch.equal(pa, p0)


@pytest.mark.parametrize("form", ["host", "dev"])
@pytest.mark.parametrize("kind", KINDS)
def test_ex_step_without_options_gives_the_plain_bits(dev, kind, form):
    check_ex_step_without_options_gives_the_plain_bits(dev, kind, form, 10007)


@pytest.mark.parametrize("n", SMALL_N)
@pytest.mark.parametrize("form", ["host", "dev"])
@pytest.mark.parametrize("kind", KINDS)
def test_ex_step_without_options_gives_the_plain_bits_small_n(dev, kind, form, n):
    check_ex_step_without_options_gives_the_plain_bits(dev, kind, form, n)


def check_ema_follows_the_parameters(dev, kind, warmup, form, n):
    """ema = d * ema + (1 - d) * p_new with the p the device produced at each step, restated in float64."""
    from chexpert_amd import ops
    d0 = 0.9
    p = rnd(640, (n,)).to(dev)
    ema = p.clone()
    want = p.cpu().double()
    st = [torch.zeros(n, device=dev) for _ in range(2)]
    hyper = plain_hyper(dev)
    for it in range(5):
        g = rnd(641 + it, (n,)).to(dev)
        launch(ops, kind, form, p, g, st, it, hyper=hyper, ex={"ema": ema, "ema_decay": d0, "ema_warmup": warmup})
        t = it + 1
        d = min(d0, (1.0 + t) / (10.0 + t)) if warmup else d0
        want = d * want + (1.0 - d) * p.cpu().double()
    close(ema.cpu(), want, rel=1e-6, what="%s ema" % kind)
    assert not torch.equal(ema, p)


@pytest.mark.parametrize("form", ["host", "dev"])
@pytest.mark.parametrize("warmup", [True, False])
@pytest.mark.parametrize("kind", KINDS)
def test_ema_follows_the_parameters(dev, kind, warmup, form):
    check_ema_follows_the_parameters(dev, kind, warmup, form, 10007)


@pytest.mark.parametrize("n", SMALL_N)
@pytest.mark.parametrize("form", ["host", "dev"])
@pytest.mark.parametrize("warmup", [True, False])
@pytest.mark.parametrize("kind", KINDS)
def test_ema_follows_the_parameters_small_n(dev, kind, warmup, form, n):
    check_ema_follows_the_parameters(dev, kind, warmup, form, n)


def lr_after(kind, lr, lr0, step, warm, gamma, ms):
    """cx_optim_tick after minibatch number `step` (chexpert.py:157-165): the scheduler has then been stepped k times."""
    if kind == "adam" or step < warm:
        return lr
    k = step - max(warm, 1) + 1
    if kind == "rmsprop":
        return lr * gamma
    return lr0 * gamma ** sum(k >= m for m in ms)


def ref_step(kind, p, st, g, lr, t):
    """float64 restatement of torch.optim.Adam / SGD(momentum .9, nesterov) / RMSprop(momentum .9, eps 1e-3) at minibatch t."""
    if kind == "adam":
        st[0] = 0.9 * st[0] + 0.1 * g
        st[1] = 0.999 * st[1] + 0.001 * g * g
        return p - lr / (1 - 0.9 ** t) * (st[0] / (st[1].sqrt() / math.sqrt(1 - 0.999 ** t) + 1e-8))
    if kind == "sgd_nesterov":
        st[0] = g.clone() if t == 1 else 0.9 * st[0] + g
        return p - lr * (g + 0.9 * st[0])
    st[0] = 0.99 * st[0] + 0.01 * g * g
    st[1] = 0.9 * st[1] + g / (st[0].sqrt() + 1e-3)
    return p - lr * st[1]


@pytest.mark.parametrize("bad", [float("inf"), float("nan")])
@pytest.mark.parametrize("kind", KINDS)
def test_nonfinite_step_is_skipped_and_still_counted(dev, kind, bad):
    """Step 2 of 4 has one inf (NaN) in g: nothing is written, the step still counts for the schedule and the bias correction."""
    from chexpert_amd import ops
    n, warm, lr0, d0 = 10007, 2, 1e-2, 0.9
    kindc, gamma, ms = {"adam": (0, 1.0, (0, 0)), "sgd_nesterov": (2, 0.1, (2, 4)), "rmsprop": (1, 0.97, (0, 0))}[kind]
    hyper = torch.tensor([lr0, 0, kindc, gamma, warm, ms[0], ms[1], lr0], dtype=torch.float32, device=dev)
    p0 = rnd(650, (n,))
    p = p0.clone().to(dev)
    ema = p.clone()
    st = [torch.zeros(n, device=dev) for _ in range(2)]
    clip = torch.zeros(4, device=dev)
    ws = torch.zeros(ops.grad_norm_partials(n), device=dev)
    ex = {"clip": clip, "ema": ema, "ema_decay": d0, "ema_warmup": True, "skip_nonfinite": True}
    pr, sr, lr = p0.double(), [torch.zeros(n, dtype=torch.float64) for _ in range(2)], lr0
    for it in range(4):
        g = rnd(651 + it, (n,))
        if it == 1:
            g[n // 2] = bad
        gd = g.to(dev)
        before = [t.clone() for t in (p, st[0], st[1], ema)]
        ops.grad_norm(gd, ws, clip, 1.0, 0.0, True)
        launch(ops, kind, "dev", p, gd, st, it, hyper=hyper, ex=ex)
        c = clip.cpu()
        if it == 1:
            for a, b in zip(before, (p, st[0], st[1], ema)):
                assert torch.equal(a, b)                         # bit for bit what step 1 left
            assert float(c[2]) == 1.0 and float(c[3]) == 1.0
        else:
            assert float(c[2]) == 0.0
            pr = ref_step(kind, pr, sr, g.double(), lr, it + 1)      # t = the minibatch count, the skipped one included
        lr = lr_after(kind, lr, lr0, it + 1, warm, gamma, ms)
        h = hyper.cpu()
        assert int(h[1]) == it + 1 and abs(float(h[0]) - lr) <= 1e-6 * lr0, (it, h, lr)
    assert float(clip.cpu()[3]) == 1.0 and int(hyper.cpu()[1]) == 4
    close(p.cpu(), pr, rel=5e-6, what=kind)
    # without skip_nonfinite the same gradient is reported and not counted
    g = rnd(652, (n,))
    g[n // 2] = bad
    c = run_norm(ops, g.to(dev), skip=False).cpu()
    assert float(c[2]) == 1.0 and float(c[3]) == 0.0


# ------------------------------------------------------------------------------------------------ the captured step
def test_graphed_step_with_clip_skip_ema_equals_eager_bits(dev):
    """GraphedTrainStep replays cx_grad_norm + cx_adam_step_dev_ex: three replays equal three eager forward_backward + step_dev +
    tick steps bit for bit (parameters, EMA, clip); then an eval forward under ema_weights()."""
    from chexpert_amd.graph import GraphedTrainStep
    from chexpert_amd.models import DenseNet
    from chexpert_amd.optim import FusedAdam
    cfg, B, S, n_cls = (2, 2, 2, 2), 4, 64, 5
    xs = [synth.xray_batch(300 + i, B, S).to(dev) for i in range(3)]
    ts = [synth.targets(400 + i, B, n_cls).to(dev) for i in range(3)]

    def fresh():
        torch.manual_seed(5)
        m = DenseNet(32, cfg, 64, num_classes=n_cls).to(dev).train()
        for n_, p in m.named_parameters():
            if n_.endswith(".bias") and "classifier" not in n_:
                p.data.fill_(2.5)
        return m

    def eager(max_norm, steps):
        m = fresh()
        opt = None
        for x, t in list(zip(xs, ts))[:steps]:
            m.zero_grad()
            m.forward_backward(x, t)
            if opt is None:
                opt = FusedAdam(m, lr=1e-3, max_grad_norm=max_norm, skip_nonfinite=True, ema_decay=0.9)
            opt.step_dev()
            opt.tick()
        return m, opt
    _, probe = eager(None, 1)
    max_norm = 0.5 * probe.grad_norm()                   # half the first step's norm: the clip is active
    assert max_norm > 0
    m_e, opt_e = eager(max_norm, 3)
    m_g = fresh()
    opt_g = FusedAdam(m_g, lr=1e-3, max_grad_norm=max_norm, skip_nonfinite=True, ema_decay=0.9)
    gs = GraphedTrainStep(m_g, opt_g, xs[0], ts[0])
    for x, t in zip(xs, ts):
        gs.replay(x, t)
    torch.cuda.synchronize()
    assert torch.equal(m_e._eng().flat, m_g._eng().flat)
    assert torch.equal(opt_e._ema, opt_g._ema)
    assert torch.equal(opt_e._clip, opt_g._clip)
    assert float(opt_g._clip.cpu()[1]) < 1.0 and opt_g.skipped_steps() == 0
    assert abs(opt_g.grad_norm() - float(opt_g._clip.cpu()[0])) == 0.0
    # evaluation with the averaged weights
    m_g.eval()
    with torch.no_grad():
        live = m_g(xs[0]).clone()
        with opt_g.ema_weights():
            avg = m_g(xs[0]).clone()
            sd_avg = {k: v.detach().clone() for k, v in m_g.state_dict().items()}
        back = m_g(xs[0]).clone()
        m2 = fresh()
        m2.load_state_dict(sd_avg)
        m2.eval()
        ref = m2(xs[0]).clone()
    assert not torch.equal(avg, live)
    assert torch.equal(avg, ref)
    assert torch.equal(back, live)
    with pytest.raises(RuntimeError):
        with FusedAdam(m2, lr=1e-3).ema_weights():
            pass
