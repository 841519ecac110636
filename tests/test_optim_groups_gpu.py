"""GPU: parameter groups of the fused optimisers (csrc/optim.hip: cx_grad_norm_items, cx_*_step_items) and their wiring in
chexpert_amd.optim, on a synthetic layout of ten tensors (about 30 V floats, V = cx_optim_item_vec4()): against torch.optim built
with the same param_groups on the CPU, the float64 restatement optim.reference_step where torch has no such rule, and bit for bit
where the feature promises bits (partition independence, frozen groups, skipped steps, the captured step, groups=None)."""
import math

import pytest
import torch

from chexpert_amd import synth

pytestmark = pytest.mark.gpu

KINDS = ["adam", "sgd_nesterov", "rmsprop"]
U = 2.0 ** -24                     # unit round-off of fp32
LR = 1e-2
GROUP_HP = [(1.0, 0.0), (0.1, 1e-2), (3.0, 1e-3)]            # (lr_mult, weight_decay) of groups 0, 1, 2


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
    print("%s: max err %.3e vs scale %.3e (rel %.2e, allowed %.1e)" % (what, err, scale, err / scale, rel))
    assert err <= rel * scale, "%s: max err %.3e vs scale %.3e (rel %.2e)" % (what, err, scale, err / scale)


def ceil_div(a, b):
    return -(-a // b)


def synthetic_sizes():
    """Floats per tensor: around one 16-byte unit, odd sizes, one short of / exactly / one float past a whole item (4 V floats) and a
    tensor of four items -- more than one workgroup, items of one partial pass and of V / 256 whole passes."""
    from chexpert_amd import ops
    V = ops.optim_item_vec4()
    return [1, 3, 4, 5, 255, 1021, 4 * V - 4, 4 * V, 4 * V + 1, 12 * V + 7]


_VALUES = {}


def values(seed, sizes):
    """Per-tensor uniform values, filled once per seed and never changed (every user clones)."""
    key = (seed, tuple(sizes))
    if key not in _VALUES:
        _VALUES[key] = [rnd(seed * 100 + k, (n,)) for k, n in enumerate(sizes)]
    return _VALUES[key]


class _Eng:
    packed_version = None


class Net(torch.nn.Module):
    """The synthetic tensors bound to one zero-padded flat buffer on the device, as the engines bind a model's parameters."""

    def __init__(self, sizes, dev, seed=7):
        super().__init__()
        from chexpert_amd.models._fused import flatten
        self.sizes = list(sizes)
        self.w = torch.nn.ParameterList([torch.nn.Parameter(v.clone()) for v in values(seed, sizes)])
        e = self.eng = _Eng()
        e.params = list(self.parameters())
        e.flat, e.offsets = flatten(e.params, dev)
        e.flat_grad = torch.zeros_like(e.flat)
        e.device = dev
        pad = torch.ones(e.flat.numel(), dtype=torch.bool)
        for off, n in zip(e.offsets, sizes):
            pad[off:off + n] = False
        self.pad = pad.to(dev)

    def _eng(self):
        return self.eng

    def set_grad(self, per_tensor):
        g = torch.zeros(self.eng.flat.numel())
        for off, v in zip(self.eng.offsets, per_tensor):
            g[off:off + v.numel()] = v
        self.eng.flat_grad.copy_(g.to(self.eng.flat_grad.device))

    def tensors(self, flat):
        f = flat.detach().cpu()
        return [f[off:off + n] for off, n in zip(self.eng.offsets, self.sizes)]

    def mask(self, group_of, grp):
        """Elements (padding included) of the tensors of group `grp`."""
        m = torch.zeros(self.eng.flat.numel(), dtype=torch.bool)
        for k, (off, n) in enumerate(zip(self.eng.offsets, self.sizes)):
            if group_of[k] == grp:
                m[off:off + ceil_div(n, 4) * 4] = True
        return m.to(self.eng.flat.device)


def group_dicts(net, group_of, rows):
    """`groups` for the optimiser: tensor k in group group_of[k]; group 0 is the default group, dict j is group j + 1."""
    ps = list(net.parameters())
    return [dict(rows[j], params=[p for p, q in zip(ps, group_of) if q == j]) for j in range(1, len(rows))]


def make_fused(kind, net, rows, group_of, decoupled=False, **options):
    """Group 0's (lr_mult 1) weight decay is the constructor's."""
    from chexpert_amd import optim as O
    assert rows[0].get("lr_mult", 1.0) == 1.0 and not rows[0].get("frozen", False)
    kw = dict(weight_decay=rows[0].get("weight_decay", 0.0), decoupled=decoupled, groups=group_dicts(net, group_of, rows), **options)
    if kind == "adam":
        return O.FusedAdam(net, lr=LR, **kw)
    if kind == "sgd_nesterov":
        return O.FusedSGDNesterov(net, lr=LR, **kw)
    return O.FusedRMSprop(net, lr=LR, decay=1.0, **kw)          # (decay 1: the scheduler inside tick() leaves lr alone)


def fused_step(opt, form):
    if form == "host":
        opt.step()
    else:
        opt.step_dev()
        opt.tick()


def torch_optimizer(kind, decoupled, params_by_group, rows):
    pg = [{"params": ps, "lr": LR * r.get("lr_mult", 1.0), "weight_decay": r.get("weight_decay", 0.0)} for ps, r in zip(params_by_group, rows)]
    if kind == "adam":
        return (torch.optim.AdamW if decoupled else torch.optim.Adam)(pg, lr=LR, betas=(0.9, 0.999), eps=1e-8)
    if decoupled:
        return None                                              # torch has no decoupled SGD / RMSprop: the float64 restatement
    if kind == "sgd_nesterov":
        return torch.optim.SGD(pg, lr=LR, momentum=0.9, nesterov=True)
    return torch.optim.RMSprop(pg, lr=LR, alpha=0.99, momentum=0.9, eps=1e-3)


class Reference:
    """torch.optim on the CPU with real param_groups where torch has the rule, else optim.reference_step in float64.  `absent(t)`:
    the groups whose gradients are None at the 1-based step t (they join with their own step count: t0)."""

    def __init__(self, kind, decoupled, sizes, group_of, rows, seed=7, absent=lambda t: ()):
        self.kind, self.decoupled, self.group_of, self.rows, self.absent = kind, decoupled, group_of, rows, absent
        self.ps = [torch.nn.Parameter(v.clone()) for v in values(seed, sizes)]
        by_group = [[p for p, q in zip(self.ps, group_of) if q == j] for j in range(len(rows))]
        self.opt = torch_optimizer(kind, decoupled, by_group, rows)
        if self.opt is None:
            self.p64 = [p.detach().double() for p in self.ps]
            self.st = [[torch.zeros(n, dtype=torch.float64), torch.zeros(n, dtype=torch.float64)] for n in sizes]
        self.t = 0
        self.sat_out = [0] * len(rows)

    def step(self, grads):
        from chexpert_amd.optim import reference_step
        self.t += 1
        gone = set(self.absent(self.t))
        for j in gone:
            self.sat_out[j] += 1
        if self.opt is not None:
            for k, p in enumerate(self.ps):
                p.grad = None if self.group_of[k] in gone else grads[k].clone()
            self.opt.step()
            return
        for k in range(len(self.ps)):
            j = self.group_of[k]
            r = self.rows[j]
            self.p64[k] = reference_step(self.kind, self.p64[k], grads[k], self.st[k], LR, self.t, lr_mult=r.get("lr_mult", 1.0),
                                         weight_decay=r.get("weight_decay", 0.0), frozen=j in gone, t0=self.sat_out[j],
                                         decoupled=self.decoupled)

    def flat(self):
        return torch.cat([p.detach().double() for p in self.ps] if self.opt is not None else self.p64)


def rows3(frozen=None):
    return [{"lr_mult": m, "weight_decay": wd, "frozen": j == frozen} for j, (m, wd) in enumerate(GROUP_HP)]


def round_robin(sizes, n):
    return [k % n for k in range(len(sizes))]


# ------------------------------------------------------------------------------------------------ against torch
@pytest.mark.parametrize("decoupled", [False, True])
@pytest.mark.parametrize("form", ["host", "dev"])
@pytest.mark.parametrize("kind", KINDS)
def test_three_groups_match_torch_param_groups(dev, kind, form, decoupled):
    """Three steps, three groups (lr_mult, weight_decay) = (1, 0), (0.1, 1e-2), (3, 1e-3), L2 and decoupled decay, held to what
    tests/test_optim_ex_gpu.py holds the ungrouped kernels to.  The padding floats stay 0 under every rule."""
    sizes = synthetic_sizes()
    group_of = round_robin(sizes, 3)
    net = Net(sizes, dev)
    opt = make_fused(kind, net, rows3(), group_of, decoupled)
    ref = Reference(kind, decoupled, sizes, group_of, rows3())
    for it in range(3):
        g = values(20 + it, sizes)
        net.set_grad(g)
        fused_step(opt, form)
        ref.step(g)
    close(torch.cat(net.tensors(net.eng.flat)), ref.flat(), rel=2e-6 if form == "host" else 5e-6, what="%s %s decoupled=%s" % (kind, form, decoupled))
    for buf in [net.eng.flat] + opt._state:
        assert not buf[net.pad].any()                                   # padding: p = g = 0 stays 0, states too
    assert opt._state[0][~net.pad].abs().max().item() > 0
    if form == "dev":
        opt.sync_from_device()
    assert opt.step_count == 3


# ------------------------------------------------------------------------------------------------ partition independence
@pytest.mark.parametrize("form", ["host", "dev"])
@pytest.mark.parametrize("kind", KINDS)
def test_the_cut_into_groups_and_items_never_changes_an_element(dev, kind, form):
    """The same hyper-parameters in every group: one group, five groups, and five groups over a table cut at 300 units instead of V
    leave p, every state and the EMA with the same bits after three steps."""
    from chexpert_amd import optim as O
    sizes = synthetic_sizes()
    row = {"lr_mult": 0.5, "weight_decay": 1e-2}
    runs = []
    for n_groups, vec4 in ((1, None), (5, None), (5, 300)):
        net = Net(sizes, dev)
        group_of = round_robin(sizes, n_groups)
        rows = [{"weight_decay": 1e-2}] + [row] * (n_groups - 1) if n_groups > 1 else [{"weight_decay": 1e-2}]
        opt = make_fused(kind, net, rows, group_of, ema_decay=0.9)
        opt._bufs(opt.NSTATE)
        opt.set_group(0, lr_mult=0.5)
        if vec4 is not None:
            items = O.item_table(sizes, group_of, vec4=vec4)
            assert len(items) > opt._items.shape[0]
            opt._items = torch.tensor(items, dtype=torch.int32).to(dev)
        for it in range(3):
            net.set_grad(values(30 + it, sizes))
            fused_step(opt, form)
        runs.append([net.eng.flat.clone()] + [s.clone() for s in opt._state] + [opt._ema.clone()])
    for other in runs[1:]:
        for a, b in zip(runs[0], other):
            assert torch.equal(a, b)
    assert not torch.equal(runs[0][0], runs[0][-1])


# ------------------------------------------------------------------------------------------------ frozen groups
@pytest.mark.parametrize("form", ["host", "dev"])
@pytest.mark.parametrize("kind", KINDS)
def test_frozen_group_keeps_its_bits_then_joins_with_its_own_step_count(dev, kind, form):
    """Group 1 of three is frozen for two steps: its p, states and EMA elements keep their bits while the others move.  Thawed
    through set_group, after five steps everything matches the torch run whose gradients of that group were None for those two
    steps (Adam: bias corrections from the group's own step count, t0 = 2).  Five steps of a few ulp each stay far inside the
    three-step tolerance of the ungrouped kernels (one step's rounding is ~U = 6e-8 of the scale)."""
    sizes = synthetic_sizes()
    group_of = round_robin(sizes, 3)
    net = Net(sizes, dev)
    opt = make_fused(kind, net, rows3(frozen=1), group_of, ema_decay=0.9)
    ref = Reference(kind, False, sizes, group_of, rows3(), absent=lambda t: (1,) if t <= 2 else ())
    frozen = net.mask(group_of, 1)
    opt._bufs(opt.NSTATE)
    before = [b.clone() for b in [net.eng.flat] + opt._state + [opt._ema]]
    for it in range(5):
        if it == 2:
            now = [net.eng.flat] + opt._state + [opt._ema]
            for a, b in zip(before, now):
                assert torch.equal(a[frozen], b[frozen])                       # bit for bit what they were
            assert not torch.equal(before[0][~frozen], now[0][~frozen]) and not torch.equal(before[1][~frozen], now[1][~frozen])
            opt.set_group(1, frozen=False)
            assert opt._gtab[1].tolist() == [pytest.approx(0.1), pytest.approx(1e-2), 0.0, 2.0]
        g = values(40 + it, sizes)
        net.set_grad(g)
        fused_step(opt, form)
        ref.step(g)
    close(torch.cat(net.tensors(net.eng.flat)), ref.flat(), rel=2e-6 if form == "host" else 5e-6, what="%s %s thawed" % (kind, form))
    assert not torch.equal(before[0][frozen], net.eng.flat[frozen])


# ------------------------------------------------------------------------------------------------ the segmented norm
def items_norm_bounds(items, n_groups, frozen):
    """Relative bounds on the fp32 group norms and on the global norm from the summation shape: a sum of non-negative terms carries
    at most (roundings on the longest path of a term to the result) * 2^-24 of relative error.
    Launch 1, per item: ceil(len4 / 256) fused multiply-adds into one of a thread's four accumulators, two additions that join the
    four, then 6 shuffle levels in the wave and 3 additions over the 4 waves.  Launch 2: the chain over the group's items, one
    addition each; for the global norm the chain over the unfrozen groups on top.
    (The two roundings of (grad_scale * g)^2 and the square root's own are covered as in tests/test_optim_ex_gpu.py's norm_bound: the
    square root halves the relative error of the sum, and the path is always longer than 3.)"""
    per_group = []
    for k in range(n_groups):
        mine = [it for it in items if it[2] == k]
        chain1 = max([ceil_div(it[1], 256) for it in mine] or [0]) + 2
        per_group.append((chain1 + 9 + len(mine)) * U)
    live = [k for k in range(n_groups) if k not in frozen]
    return per_group, max(per_group[k] for k in live) + len(live) * U


@pytest.mark.parametrize("grad_scale", [1.0, 0.125])
def test_segmented_norm_values_and_reproducible(dev, grad_scale):
    from chexpert_amd import ops, optim as O
    sizes = synthetic_sizes()
    group_of = round_robin(sizes, 3)
    net = Net(sizes, dev)
    opt = make_fused("adam", net, rows3(frozen=1), group_of, skip_nonfinite=True)
    g = values(50, sizes)
    net.set_grad(g)
    opt._bufs(2)
    items = O.item_table(sizes, group_of)

    def run():
        ops.grad_norm_items(net.eng.flat_grad, opt._items, opt._gtab, opt._gpart, opt._gsq, opt._gnorm, opt._clip, grad_scale, 0.0, True)
        return opt._clip.cpu(), opt._gnorm.cpu(), opt._gsq.cpu()
    a, b = run(), run()
    want_group = [math.sqrt(sum(float((v.double() * grad_scale).pow(2).sum()) for v, q in zip(g, group_of) if q == k)) for k in range(3)]
    want = math.sqrt(want_group[0] ** 2 + want_group[2] ** 2)                   # over the unfrozen groups
    bounds, bound = items_norm_bounds(items, 3, {1})
    for k in range(3):
        err = abs(float(a[1][k]) - want_group[k]) / want_group[k]
        print("group %d scale %g: norm %.9g want %.9g rel err %.3e bound %.3e" % (k, grad_scale, float(a[1][k]), want_group[k], err, bounds[k]))
        assert err <= bounds[k]
    err = abs(float(a[0][0]) - want) / want
    print("global scale %g: norm %.9g want %.9g rel err %.3e bound %.3e" % (grad_scale, float(a[0][0]), want, err, bound))
    assert err <= bound
    assert a[0][1:].tolist() == [1.0, 0.0, 0.0]                                  # clipping off: coefficient 1; finite; none skipped
    for x, y in zip(a, b):
        assert torch.equal(x, y)                                                 # same bits on every call
    # the coefficient of an active clip
    ops.grad_norm_items(net.eng.flat_grad, opt._items, opt._gtab, opt._gpart, opt._gsq, opt._gnorm, opt._clip, grad_scale, 0.5 * want, False)
    c = opt._clip.cpu()
    assert abs(float(c[1]) - 0.5 * want / (want + 1e-6)) <= (bound + 3 * U) * 0.5 and float(c[0]) == float(a[0][0])


@pytest.mark.parametrize("kind", KINDS)
def test_nonfinite_in_a_frozen_group_is_ignored_in_a_live_group_skips_the_step(dev, kind):
    sizes = synthetic_sizes()
    group_of = round_robin(sizes, 3)
    net = Net(sizes, dev)
    opt = make_fused(kind, net, rows3(frozen=1), group_of, skip_nonfinite=True, ema_decay=0.9)
    frozen = net.mask(group_of, 1)
    g = [v.clone() for v in values(60, sizes)]
    g[7][100] = float("inf")                                                     # tensor 7 is in group 1: frozen
    assert group_of[7] == 1 and group_of[6] == 0
    net.set_grad(g)
    opt._bufs(opt.NSTATE)
    before = [b.clone() for b in [net.eng.flat] + opt._state + [opt._ema]]
    fused_step(opt, "dev")
    now = [net.eng.flat] + opt._state + [opt._ema]
    assert opt._clip.cpu()[2:].tolist() == [0.0, 0.0] and opt.skipped_steps() == 0
    assert math.isfinite(opt.grad_norm()) and opt.grad_norm() > 0
    norms = opt.group_grad_norms()
    assert len(norms) == 3 and math.isinf(norms[1]) and math.isfinite(norms[0]) and math.isfinite(norms[2])
    assert not torch.equal(before[0][~frozen], now[0][~frozen])                  # the step proceeded ...
    assert all(torch.equal(a[frozen], b[frozen]) for a, b in zip(before, now))   # ... and the frozen group kept its bits
    assert torch.isfinite(net.eng.flat).all()
    # the same inf in a live group: nothing is written anywhere, one step is counted as skipped
    g = [v.clone() for v in values(60, sizes)]
    g[6][100] = float("inf")
    net.set_grad(g)
    before = [b.clone() for b in now]
    fused_step(opt, "dev")
    assert all(torch.equal(a, b) for a, b in zip(before, [net.eng.flat] + opt._state + [opt._ema]))
    assert opt._clip.cpu()[2:].tolist() == [1.0, 1.0] and opt.skipped_steps() == 1
    opt.sync_from_device()
    assert opt.step_count == 2                                                   # a skipped step is still a minibatch


# ------------------------------------------------------------------------------------------------ clip + EMA + groups
@pytest.mark.parametrize("kind", KINDS)
def test_clip_ema_and_groups_together(dev, kind):
    """Device form, three groups, group 2 frozen, max_norm = half the norm of the unfrozen gradient (the clip is active), EMA with
    warm-up.  CPU: clip_grad_norm_ over the unfrozen parameters, then optim.reference_step and the EMA recurrence in float64."""
    from chexpert_amd.optim import reference_step
    sizes = synthetic_sizes()
    group_of = round_robin(sizes, 3)
    rows = rows3(frozen=2)
    live = [k for k in range(len(sizes)) if group_of[k] != 2]
    g0 = values(70, sizes)
    max_norm = 0.5 * math.sqrt(sum(float(g0[k].double().pow(2).sum()) for k in live))
    net = Net(sizes, dev)
    opt = make_fused(kind, net, rows, group_of, max_grad_norm=max_norm, ema_decay=0.9)
    p64 = [v.double() for v in values(7, sizes)]
    ema64 = [v.clone() for v in p64]
    st = [[torch.zeros(n, dtype=torch.float64), torch.zeros(n, dtype=torch.float64)] for n in sizes]
    for it, scale in enumerate([1.0, 3.0, 0.25]):                                # clipped, clipped harder, not clipped
        g = [v * scale for v in g0]
        net.set_grad(g)
        fused_step(opt, "dev")
        gc = [torch.nn.Parameter(torch.zeros(n)) for n in sizes]
        for k in live:
            gc[k].grad = g[k].clone()
        total = torch.nn.utils.clip_grad_norm_([gc[k] for k in live], max_norm)
        assert abs(opt.grad_norm() - float(total)) <= 1e-5 * float(total)
        assert (float(opt._clip.cpu()[1]) < 1.0) == (scale >= 1.0)
        t = it + 1
        d = min(0.9, (1.0 + t) / (10.0 + t))
        for k in range(len(sizes)):
            r = rows[group_of[k]]
            if r["frozen"]:
                continue
            p64[k] = reference_step(kind, p64[k], gc[k].grad, st[k], LR, t, lr_mult=r["lr_mult"], weight_decay=r["weight_decay"])
            ema64[k] = d * ema64[k] + (1.0 - d) * p64[k]
    close(torch.cat(net.tensors(net.eng.flat)), torch.cat(p64), rel=5e-6, what="%s p" % kind)
    close(torch.cat(net.tensors(opt._ema)), torch.cat(ema64), rel=5e-6, what="%s ema" % kind)
    frozen = net.mask(group_of, 2)
    first = torch.cat([torch.nn.functional.pad(v, (0, -v.numel() % 4)) for v in values(7, sizes)]).to(dev)
    assert torch.equal(net.eng.flat[frozen], first[frozen]) and torch.equal(opt._ema[frozen], first[frozen])
    assert not opt._state[0][frozen].any()


# ------------------------------------------------------------------------------------------------ the captured step
def test_graphed_step_with_a_thaw_between_replays_equals_eager_bits(dev):
    """GraphedTrainStep replays cx_adam_step_items with the backbone frozen; set_group thaws it between two replays without a
    recapture.  Two replays, the thaw, two replays = the same five calls run eagerly (forward_backward + step_dev + tick), bit for
    bit; after the first two only the head's elements of the flat buffer have changed."""
    from chexpert_amd.graph import GraphedTrainStep
    from chexpert_amd.models import DenseNet
    from chexpert_amd.optim import FusedAdam, finetune_groups
    cfg, B, S, n_cls = (2, 2, 2, 2), 4, 64, 5
    xs = [synth.xray_batch(300 + i, B, S).to(dev) for i in range(4)]
    ts = [synth.targets(400 + i, B, n_cls).to(dev) for i in range(4)]

    def fresh():
        torch.manual_seed(5)
        m = DenseNet(32, cfg, 64, num_classes=n_cls).to(dev).train()
        opt = FusedAdam(m, lr=1e-3, groups=finetune_groups(m, freeze_backbone=True, head_lr_mult=10, weight_decay=1e-4,
                                                           no_decay_norm_bias=True))
        return m, opt

    def thaw(opt):
        assert opt.group_names == ["default", "backbone", "backbone_no_decay", "head", "head_no_decay"]
        opt.set_group(1, frozen=False)
        opt.set_group(2, frozen=False)
        assert [r[3] for r in opt._grows] == [0.0, 2.0, 2.0, 0.0, 0.0]           # the steps the backbone sat out

    m_e, opt_e = fresh()
    for i, (x, t) in enumerate(zip(xs, ts)):
        if i == 2:
            thaw(opt_e)
        m_e.zero_grad()
        m_e.forward_backward(x, t)
        opt_e.step_dev()
        opt_e.tick()
    m_g, opt_g = fresh()
    gs = GraphedTrainStep(m_g, opt_g, xs[0], ts[0])
    eng = m_g._eng()
    first = eng.flat.clone()
    head = torch.zeros(eng.flat.numel(), dtype=torch.bool)
    for p in m_g.classifier.parameters():
        head[eng.off_of[id(p)]:eng.off_of[id(p)] + p.numel()] = True
    head = head.to(dev)
    for i, (x, t) in enumerate(zip(xs, ts)):
        if i == 2:
            torch.cuda.synchronize()
            assert torch.equal(eng.flat[~head], first[~head])                     # the backbone has not moved ...
            assert (eng.flat[head] != first[head]).any()                          # ... the head has
            thaw(opt_g)
        gs.replay(x, t)
    torch.cuda.synchronize()
    assert torch.equal(m_e._eng().flat, eng.flat)
    assert all(torch.equal(a, b) for a, b in zip(opt_e._state, opt_g._state))
    assert not torch.equal(eng.flat[~head], first[~head])                         # thawed without recapturing
    opt_g.sync_from_device()
    assert opt_g.step_count == 4


# ------------------------------------------------------------------------------------------------ groups=None
@pytest.mark.parametrize("kind", KINDS)
def test_groups_none_gives_the_bits_of_the_plain_and_ex_entry_points(dev, kind):
    """Without groups the optimisers call what they called before: three steps through the class (with a scalar weight_decay, then
    with the EMA on) equal the same three launches of the plain / _ex entry points, bit for bit."""
    from chexpert_amd import ops, optim as O
    sizes, wd = synthetic_sizes(), 1e-2
    for ema_on in (False, True):
        net = Net(sizes, dev)
        kw = {"ema_decay": 0.9} if ema_on else {}
        opt = {"adam": lambda: O.FusedAdam(net, lr=LR, weight_decay=wd, **kw), "sgd_nesterov": lambda: O.FusedSGDNesterov(net, lr=LR, weight_decay=wd, **kw),
               "rmsprop": lambda: O.FusedRMSprop(net, lr=LR, weight_decay=wd, **kw)}[kind]()
        assert not opt._grouped
        p = net.eng.flat.clone()
        st = [torch.zeros_like(p) for _ in range(2)]
        ema = p.clone()
        ex = {"ema": ema, "ema_decay": 0.9, "ema_warmup": True} if ema_on else None
        sfx = "_ex" if ema_on else ""
        for it in range(3):
            net.set_grad(values(80 + it, sizes))
            g = net.eng.flat_grad
            opt.step()
            step = (it + 1,) if ema_on else ()
            if kind == "adam":
                getattr(ops, "adam_step" + sfx)(p, g, st[0], st[1], LR, 0.9, 0.999, 1e-8, wd, it + 1, 1.0, **(ex or {}))
            elif kind == "sgd_nesterov":
                getattr(ops, "sgd_nesterov_step" + sfx)(p, g, st[0], LR, 0.9, wd, it == 0, *step, 1.0, **(ex or {}))
            else:
                getattr(ops, "rmsprop_step" + sfx)(p, g, st[0], st[1], LR, 0.99, 1e-3, 0.9, wd, *step, 1.0, **(ex or {}))
        assert torch.equal(net.eng.flat, p)
        assert all(torch.equal(a, b) for a, b in zip(opt._state, st))
        assert opt._items is None and opt._gtab is None
        if ema_on:
            assert torch.equal(opt._ema, ema)


# ------------------------------------------------------------------------------------------------ the command line
def test_cli_freezes_the_backbone_then_thaws_it_under_graph(dev, tmp_path):
    """--train --fused_optimizer --graph with the group flags, 16 synthetic images in minibatches of 4: the backbone's rows are
    thawed through set_group right after minibatch 2, the captured step goes on without a recapture, the losses stay finite and
    the logged gradient norm is that of the unfrozen groups."""
    import contextlib
    import io
    import json
    from chexpert_amd import cli, graph, optim as O
    thaws, captures = [], []
    real_set, real_init = O._Flat.set_group, graph.GraphedTrainStep.__init__

    def spy_set(self, i, **kw):
        self.sync_from_device()
        thaws.append((self.step_count, self.group_names[i], kw))
        return real_set(self, i, **kw)

    def spy_init(self, *a, **k):
        captures.append(1)
        return real_init(self, *a, **k)
    O._Flat.set_group, graph.GraphedTrainStep.__init__ = spy_set, spy_init
    buf = io.StringIO()
    try:
        with contextlib.redirect_stdout(buf):
            cli.main(["--train", "--fused_optimizer", "--graph", "--synthetic", "16", "--batch_size", "4", "--resize", "64", "--eval_interval", "100",
                      "--log_interval", "1", "--seed", "3", "--weight_decay", "1e-4", "--no_decay_norm_bias", "--head_lr_mult", "10",
                      "--freeze_backbone_steps", "2", "--clip_grad_norm", "5", "--output_dir", str(tmp_path)])
    finally:
        O._Flat.set_group, graph.GraphedTrainStep.__init__ = real_set, real_init
    lines = [json.loads(l) for l in buf.getvalue().splitlines() if l.startswith('{"step"')]
    assert [l["step"] for l in lines] == [1, 2, 3, 4] and all(math.isfinite(l["train_loss"]) for l in lines), lines
    assert thaws == [(2, "backbone", {"frozen": False}), (2, "backbone_no_decay", {"frozen": False})]
    assert captures == [1]
    norms = [l["grad_norm"] for l in lines]
    assert all(math.isfinite(v) and v > 0 for v in norms)
    assert norms[2] > norms[1]                     # from step 3 on the backbone's gradient counts
