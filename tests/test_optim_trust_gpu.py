"""GPU: the layer-wise trust-ratio optimisers (csrc/optim.hip: cx_lamb_step_items, cx_lars_step_items; chexpert_amd.optim.FusedLAMB,
FusedLARS) on the synthetic ten-tensor layout of tests/test_optim_groups_gpu.py (about 30 V floats, V = cx_optim_item_vec4()): against
the float64 statement optim.reference_trust_step, the ratios against float64 norms with a bound derived from the summation shape, and
bit for bit where the feature promises bits (two runs, the cut into groups, frozen groups, skipped steps, the captured step, the
grouped Adam / SGD steps that share a kernel template with LARS)."""
import math

import pytest
import torch

from chexpert_amd import synth

pytestmark = pytest.mark.gpu

KINDS = ["lamb", "lars"]
U = 2.0 ** -24                     # unit round-off of fp32
LR = 1e-2
COEF = 0.02                        # LARS: large enough for the adapted tensors to move visibly in three steps
GROUP_HP = [(1.0, 0.0), (0.1, 1e-2), (3.0, 1e-3)]            # (lr_mult, weight_decay) of groups 0, 1, 2: group 0 is not adapted


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    from chexpert_amd import _lib
    _lib.lib()          # fail loudly if the HIP library is missing
    return torch.device("cuda:0")


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
    """Per-tensor uniform values in [-1, 1), filled once per seed and never changed (every user clones)."""
    key = (seed, tuple(sizes))
    if key not in _VALUES:
        _VALUES[key] = [synth.uniform(seed * 100 + k, (n,), -1.0, 1.0) for k, n in enumerate(sizes)]
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


def rows3(frozen=None):
    return [{"lr_mult": m, "weight_decay": wd, "frozen": j == frozen} for j, (m, wd) in enumerate(GROUP_HP)]


def round_robin(sizes, n):
    return [k % n for k in range(len(sizes))]


def make_fused(kind, net, rows, group_of, **options):
    """Group 0's (lr_mult 1) weight decay is the constructor's; dict j is group j + 1."""
    from chexpert_amd import optim as O
    assert rows[0].get("lr_mult", 1.0) == 1.0 and not rows[0].get("frozen", False)
    ps = list(net.parameters())
    groups = [dict(rows[j], params=[p for p, q in zip(ps, group_of) if q == j]) for j in range(1, len(rows))]
    kw = dict(weight_decay=rows[0].get("weight_decay", 0.0), groups=groups, **options)
    if kind == "lamb":
        return O.FusedLAMB(net, lr=LR, **kw)
    kw.setdefault("trust_coef", COEF)
    return O.FusedLARS(net, lr=LR, **kw)


def fused_step(opt, form):
    if form == "host":
        opt.step()
    else:
        opt.step_dev()
        opt.tick()


def buffers(net, opt):
    return [net.eng.flat] + opt._state + ([opt._ema] if opt._ema is not None else [])


class Statement:
    """optim.reference_trust_step in float64 over the synthetic tensors.  `absent(t)`: the groups frozen at the 1-based step t (they
    join with their own step count: t0)."""

    def __init__(self, kind, sizes, group_of, rows, seed=7, absent=lambda t: (), **rule):
        self.kind, self.group_of, self.rows, self.absent, self.rule = kind, group_of, rows, absent, rule
        if kind == "lars":
            self.rule.setdefault("trust_coef", COEF)
        self.p = [v.double() for v in values(seed, sizes)]
        self.st = [[torch.zeros(n, dtype=torch.float64), torch.zeros(n, dtype=torch.float64)] for n in sizes]
        self.t = 0
        self.sat_out = [0] * len(rows)
        self.ratios = None

    def step(self, grads, **scales):
        from chexpert_amd.optim import reference_trust_step
        self.t += 1
        gone = set(self.absent(self.t))
        for j in gone:
            self.sat_out[j] += 1
        rows = [[r.get("lr_mult", 1.0), r.get("weight_decay", 0.0), j in gone, self.sat_out[j]] for j, r in enumerate(self.rows)]
        self.p, self.ratios = reference_trust_step(self.kind, self.p, grads, self.st, LR, self.t, rows, self.group_of, **scales, **self.rule)

    def flat(self):
        return torch.cat(self.p)


# ------------------------------------------------------------------------------------------------ against the float64 statement
@pytest.mark.parametrize("always_adapt", [False, True])
@pytest.mark.parametrize("form", ["host", "dev"])
@pytest.mark.parametrize("kind", KINDS)
def test_three_steps_match_the_float64_statement(dev, kind, form, always_adapt):
    """Three steps, three groups (lr_mult, weight_decay) = (1, 0), (0.1, 1e-2), (3, 1e-3): group 0 is exempt from adaptation unless
    always_adapt.  Held to what tests/test_optim_groups_gpu.py holds the grouped kernels to; the ratio's error does not enlarge it
    (an update is lr = 1e-2 of the scale, the ratio is good to a few 1e-6).  The padding floats of p, the states and u stay 0."""
    sizes = synthetic_sizes()
    group_of = round_robin(sizes, 3)
    net = Net(sizes, dev)
    opt = make_fused(kind, net, rows3(), group_of, always_adapt=always_adapt)
    ref = Statement(kind, sizes, group_of, rows3(), always_adapt=always_adapt)
    first = net.eng.flat.clone()
    for it in range(3):
        g = values(20 + it, sizes)
        net.set_grad(g)
        fused_step(opt, form)
        ref.step(g)
    rel = 2e-6 if form == "host" else 5e-6
    got = torch.cat(net.tensors(net.eng.flat))
    close(got, ref.flat(), rel=rel, what="%s %s always_adapt=%s" % (kind, form, always_adapt))
    # the parameters moved: every group by more than the comparison allows, the adapted ones together by far more
    scale = ref.flat().abs().max().item()
    moved = (net.eng.flat - first).abs()
    per_group = [moved[net.mask(group_of, j)].max().item() for j in range(3)]
    print("moved per group: %s (allowed error %.1e)" % (["%.3e" % v for v in per_group], rel * scale))
    assert all(v > 4 * rel * scale for v in per_group)
    assert max(per_group[1:]) > 100 * rel * scale
    for buf in [net.eng.flat] + opt._state + ([opt._u] if opt._u is not None else []):
        assert not buf[net.pad].any()                                   # padding: p = g = 0 stays 0, states and u too
    assert opt._state[0][~net.pad].abs().max().item() > 0
    rows = opt._trust.cpu()
    assert [bool(v) for v in rows[:, 3]] == [always_adapt or GROUP_HP[q][1] != 0 for q in group_of]
    if form == "dev":
        opt.sync_from_device()
    assert opt.step_count == 3


# ------------------------------------------------------------------------------------------------ the ratios themselves
def ratio_bounds(kind, items, k):
    """First-order relative bounds (bound of |p|, bound of |u|, bound of r) for tensor k from the summation shape.  A sum of non-negative
    terms carries at most (roundings on the longest path of a term to the result) * 2^-24 of relative error.
    Launch 1, per item: ceil(len4 / 256) fused multiply-adds into one of a thread's four accumulators (each squares and adds with one
    rounding), two additions that join the four, 6 shuffle levels in the wave and 3 additions over the 4 waves.  Launch 2: one addition
    per item of the tensor.  The square root halves the relative error of the sum and adds its own (HIP documents sqrtf at 1 ulp =
    2 U); the division is allowed 1 ulp too.
    LAMB: r = |p| / |u|: the two norms and the division.  LARS: r = coef |p| / (|g| + wd |p| + eps): coef |p| rounds once; the
    denominator is a sum of non-negative terms, as good as its worst term (|g|, or wd |p| with one more rounding) plus its two
    additions; the fp32 values of coef, wd and eps each differ from the test's doubles by at most U.  Second-order terms: 0.1 %."""
    mine = [it for it in items if it[3] == k]
    path = max(ceil_div(it[1], 256) for it in mine) + 2 + 9 + len(mine)
    b_norm = 0.5 * path * U + 2 * U
    if kind == "lamb":
        b_r = 2 * b_norm + 2 * U
    else:
        b_r = (b_norm + 2 * U) + (b_norm + 2 * U + 2 * U) + 2 * U + U
    return b_norm, b_norm, 1.001 * b_r


@pytest.mark.parametrize("kind", KINDS)
def test_trust_table_against_float64_norms(dev, kind):
    """One step with always_adapt (every tensor adapted); tensor 4 (group 1) has p = 0 and tensor 6 (group 0, no decay) g = 0: both
    give r = 1 exactly.  The norms are those of the fp32 buffers the kernels read (p before the step, the scaled gradient, LAMB's
    stored u), in float64."""
    from chexpert_amd import optim as O
    sizes = synthetic_sizes()
    group_of = round_robin(sizes, 3)
    assert group_of[4] == 1 and group_of[6] == 0
    net = Net(sizes, dev)
    opt = make_fused(kind, net, rows3(), group_of, always_adapt=True)
    off = net.eng.offsets
    net.eng.flat.data[off[4]:off[4] + sizes[4]] = 0.0
    g = [v.clone() for v in values(50, sizes)]
    g[6].zero_()
    net.set_grad(g)
    p_before = net.tensors(net.eng.flat.clone())
    fused_step(opt, "dev")
    rows = opt._trust.cpu().double()
    named = opt.trust_ratios()
    items = O.item_table(sizes, group_of)
    u_after = net.tensors(opt._u) if kind == "lamb" else net.tensors(net.eng.flat_grad)
    for k in range(len(sizes)):
        wd = GROUP_HP[group_of[k]][1]
        wn = math.sqrt(float(p_before[k].double().pow(2).sum()))
        un = math.sqrt(float(u_after[k].double().pow(2).sum()))
        r, got_wn, got_un, adapted = [float(v) for v in rows[k]]
        assert adapted == 1.0
        assert named["w.%d" % k] == (float(opt._trust[k, 0]), float(opt._trust[k, 1]), float(opt._trust[k, 2]))
        if k in (4, 6):
            print("tensor %d: r %.9g |p| %.9g |u| %.9g" % (k, r, got_wn, got_un))
            assert r == 1.0 and (got_wn == 0.0 if k == 4 else got_un == 0.0)
            continue
        b_w, b_u, b_r = ratio_bounds(kind, items, k)
        want = wn / un if kind == "lamb" else COEF * wn / (un + wd * wn + 1e-8)
        errs = (abs(got_wn - wn) / wn, abs(got_un - un) / un, abs(r - want) / want)
        print("tensor %d (%d floats): |p| rel err %.3e (bound %.3e), |u| %.3e (%.3e), r = %.9g rel err %.3e (%.3e)"
              % (k, sizes[k], errs[0], b_w, errs[1], b_u, r, errs[2], b_r))
        assert errs[0] <= b_w and errs[1] <= b_u and errs[2] <= b_r


def test_trust_clip_caps_every_ratio_at_one(dev):
    """LARS with trust_coef 3: ratios around 3 without the clip, none above 1 with it (and the tensors that were above sit at 1)."""
    sizes = synthetic_sizes()
    group_of = round_robin(sizes, 3)
    tables = []
    for clip in (False, True):
        net = Net(sizes, dev)
        opt = make_fused("lars", net, rows3(), group_of, trust_coef=3.0, always_adapt=True, trust_clip=clip)
        net.set_grad(values(51, sizes))
        fused_step(opt, "host")
        tables.append(opt._trust.cpu())
    free, capped = tables
    assert (free[:, 0] > 1.0).any() and (capped[:, 0] <= 1.0).all()
    assert torch.equal(capped[:, 0], free[:, 0].clamp(max=1.0)) and torch.equal(capped[:, 1:], free[:, 1:])


# ------------------------------------------------------------------------------------------------ bits
@pytest.mark.parametrize("form", ["host", "dev"])
@pytest.mark.parametrize("kind", KINDS)
def test_same_bits_on_every_run_and_for_every_cut_into_groups(dev, kind, form):
    """The same hyper-parameters in every group: two runs with one group and a run with five groups leave p, every state, the EMA and
    the trust table with the same bits after three steps.  The group is only a label: the item cuts, and with them every summation
    tree, depend on the shapes alone.  (A table cut at another item length may change the bits of the norms and is not promised.)"""
    sizes = synthetic_sizes()
    row = {"lr_mult": 0.5, "weight_decay": 1e-2}
    runs = []
    for n_groups in (1, 1, 5):
        net = Net(sizes, dev)
        group_of = round_robin(sizes, n_groups)
        rows = [{"weight_decay": 1e-2}] + [row] * (n_groups - 1)
        opt = make_fused(kind, net, rows, group_of, ema_decay=0.9)
        opt._bufs(opt.NSTATE)
        opt.set_group(0, lr_mult=0.5)
        for it in range(3):
            net.set_grad(values(30 + it, sizes))
            fused_step(opt, form)
        runs.append([b.clone() for b in buffers(net, opt)] + [opt._trust.clone()])
    for other in runs[1:]:
        for a, b in zip(runs[0], other):
            assert torch.equal(a, b)
    assert not torch.equal(runs[0][0], runs[0][-2])                     # p has left its average behind: something moved
    assert (runs[0][-1][:, 3] == 1.0).all() and (runs[0][-1][:, 0] != 1.0).any()


# ------------------------------------------------------------------------------------------------ frozen groups
@pytest.mark.parametrize("form", ["host", "dev"])
@pytest.mark.parametrize("kind", KINDS)
def test_frozen_group_keeps_its_bits_then_joins_with_its_own_step_count(dev, kind, form):
    """Group 1 of three is frozen for two steps: its p, states, EMA and u elements keep their bits while the others move, and its trust
    rows read r = 1.  Thawed through set_group, after five steps everything matches the statement with t0 = 2."""
    sizes = synthetic_sizes()
    group_of = round_robin(sizes, 3)
    net = Net(sizes, dev)
    opt = make_fused(kind, net, rows3(frozen=1), group_of, ema_decay=0.9)
    ref = Statement(kind, sizes, group_of, rows3(), absent=lambda t: (1,) if t <= 2 else ())
    frozen = net.mask(group_of, 1)
    opt._bufs(opt.NSTATE)
    if opt._u is not None:
        opt._u.fill_(7.0)                                               # a live item overwrites every float of its u
    held = lambda: buffers(net, opt) + ([opt._u] if opt._u is not None else [])
    before = [b.clone() for b in held()]
    for it in range(5):
        if it == 2:
            now = held()
            for a, b in zip(before, now):
                assert torch.equal(a[frozen], b[frozen])                       # bit for bit what they were
                assert not torch.equal(a[~frozen], b[~frozen])
            rows = opt._trust.cpu()
            for k in range(len(sizes)):
                if group_of[k] == 1:
                    assert rows[k].tolist() == [1.0, 0.0, 0.0, 0.0]
                else:
                    assert rows[k, 1] > 0 and rows[k, 2] > 0
            opt.set_group(1, frozen=False)
            assert opt._gtab[1].tolist() == [pytest.approx(0.1), pytest.approx(1e-2), 0.0, 2.0]
        g = values(40 + it, sizes)
        net.set_grad(g)
        fused_step(opt, form)
        ref.step(g)
    close(torch.cat(net.tensors(net.eng.flat)), ref.flat(), rel=2e-6 if form == "host" else 5e-6, what="%s %s thawed" % (kind, form))
    assert not torch.equal(before[0][frozen], net.eng.flat[frozen])
    assert (opt._trust.cpu()[:, 1] > 0).all()


# ------------------------------------------------------------------------------------------------ non-finite gradients
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
    before = [b.clone() for b in buffers(net, opt)]
    fused_step(opt, "dev")
    now = buffers(net, opt)
    assert opt._clip.cpu()[2:].tolist() == [0.0, 0.0] and opt.skipped_steps() == 0
    assert not torch.equal(before[0][~frozen], now[0][~frozen])                  # the step proceeded ...
    assert all(torch.equal(a[frozen], b[frozen]) for a, b in zip(before, now))   # ... and the frozen group kept its bits
    assert torch.isfinite(net.eng.flat).all() and torch.isfinite(opt._trust).all()
    # the same inf in a live group: nothing is written anywhere, one step is counted as skipped
    g = [v.clone() for v in values(60, sizes)]
    g[6][100] = float("inf")
    net.set_grad(g)
    before = [b.clone() for b in now] + [opt._trust.clone()] + ([opt._u.clone()] if opt._u is not None else [])
    fused_step(opt, "dev")
    after = buffers(net, opt) + [opt._trust] + ([opt._u] if opt._u is not None else [])
    assert all(torch.equal(a, b) for a, b in zip(before, after))
    assert opt._clip.cpu()[2:].tolist() == [1.0, 1.0] and opt.skipped_steps() == 1
    opt.sync_from_device()
    assert opt.step_count == 2                                                   # a skipped step is still a minibatch


# ------------------------------------------------------------------------------------------------ clip + EMA + trust
@pytest.mark.parametrize("kind", KINDS)
def test_clip_ema_and_trust_together(dev, kind):
    """Device form, three groups, group 2 frozen, max_norm = half the norm of the live gradient (the clip is active), EMA with
    warm-up.  CPU: clip_grad_norm_ over the live parameters, then the statement and the EMA recurrence in float64."""
    sizes = synthetic_sizes()
    group_of = round_robin(sizes, 3)
    rows = rows3(frozen=2)
    live = [k for k in range(len(sizes)) if group_of[k] != 2]
    g0 = values(70, sizes)
    max_norm = 0.5 * math.sqrt(sum(float(g0[k].double().pow(2).sum()) for k in live))
    net = Net(sizes, dev)
    opt = make_fused(kind, net, rows, group_of, max_grad_norm=max_norm, ema_decay=0.9)
    ref = Statement(kind, sizes, group_of, rows3(), absent=lambda t: (2,))
    ema64 = [v.clone() for v in ref.p]
    for it, scale in enumerate([1.0, 3.0, 0.25]):                                # clipped, clipped harder, not clipped
        g = [v * scale for v in g0]
        net.set_grad(g)
        fused_step(opt, "dev")
        gc = [torch.nn.Parameter(torch.zeros(n)) for n in sizes]
        for k in range(len(sizes)):
            gc[k].grad = g[k].clone()
        total = torch.nn.utils.clip_grad_norm_([gc[k] for k in live], max_norm)
        assert abs(opt.grad_norm() - float(total)) <= 1e-5 * float(total)
        assert (float(opt._clip.cpu()[1]) < 1.0) == (scale >= 1.0)
        ref.step([q.grad for q in gc])
        t = it + 1
        d = min(0.9, (1.0 + t) / (10.0 + t))
        for k in live:
            ema64[k] = d * ema64[k] + (1.0 - d) * ref.p[k]
    close(torch.cat(net.tensors(net.eng.flat)), ref.flat(), rel=5e-6, what="%s p" % kind)
    close(torch.cat(net.tensors(opt._ema)), torch.cat(ema64), rel=5e-6, what="%s ema" % kind)
    frozen = net.mask(group_of, 2)
    first = torch.cat([torch.nn.functional.pad(v, (0, -v.numel() % 4)) for v in values(7, sizes)]).to(dev)
    assert torch.equal(net.eng.flat[frozen], first[frozen]) and torch.equal(opt._ema[frozen], first[frozen])
    assert not opt._state[0][frozen].any()
    assert not torch.equal(net.eng.flat[~frozen], first[~frozen])


# ------------------------------------------------------------------------------------------------ the captured step
@pytest.mark.parametrize("kind", KINDS)
def test_graphed_step_equals_eager_bits(dev, kind):
    """GraphedTrainStep replays the three launches of the trust-ratio step: four replays = the same four calls run eagerly
    (forward_backward + step_dev + tick), bit for bit in p and the states."""
    from chexpert_amd.graph import GraphedTrainStep
    from chexpert_amd.models import DenseNet
    from chexpert_amd.optim import FusedLAMB, FusedLARS, finetune_groups
    cfg, B, S, n_cls = (2, 2, 2, 2), 4, 64, 5
    xs = [synth.xray_batch(300 + i, B, S).to(dev) for i in range(4)]
    ts = [synth.targets(400 + i, B, n_cls).to(dev) for i in range(4)]

    def fresh():
        torch.manual_seed(5)
        m = DenseNet(32, cfg, 64, num_classes=n_cls).to(dev).train()
        groups = finetune_groups(m, weight_decay=1e-4, no_decay_norm_bias=True)
        opt = FusedLAMB(m, lr=1e-3, groups=groups) if kind == "lamb" else FusedLARS(m, lr=1e-2, trust_coef=COEF, groups=groups)
        return m, opt

    m_e, opt_e = fresh()
    for x, t in zip(xs, ts):
        m_e.zero_grad()
        m_e.forward_backward(x, t)
        opt_e.step_dev()
        opt_e.tick()
    m_g, opt_g = fresh()
    gs = GraphedTrainStep(m_g, opt_g, xs[0], ts[0])
    eng = m_g._eng()
    first = eng.flat.clone()
    assert len(opt_g._state) == opt_g.NSTATE
    for x, t in zip(xs, ts):
        gs.replay(x, t)
    torch.cuda.synchronize()
    assert torch.equal(m_e._eng().flat, eng.flat)
    assert all(torch.equal(a, b) for a, b in zip(opt_e._state, opt_g._state))
    assert torch.equal(opt_e._trust, opt_g._trust)
    assert not torch.equal(eng.flat, first) and torch.isfinite(eng.flat).all()
    ratios = opt_g.trust_ratios()
    assert set(ratios) == {n for n, _ in m_g.named_parameters()}
    adapted = opt_g._trust.cpu()[:, 3] != 0
    assert adapted.any() and not adapted.all()                      # the 1-D parameters are exempt (no_decay_norm_bias)
    opt_g.sync_from_device()
    assert opt_g.step_count == 4


# ------------------------------------------------------------------------------------------------ the command line
@pytest.mark.parametrize("kind", KINDS)
def test_cli_trains_under_graph_and_logs_the_ratios(dev, tmp_path, kind):
    import contextlib
    import io
    import json
    from chexpert_amd import cli, graph, optim as O
    captures, built = [], []
    real_init, real_make = graph.GraphedTrainStep.__init__, cli.trust_optimizer

    def spy_init(self, *a, **k):
        captures.append(1)
        return real_init(self, *a, **k)

    def spy_make(*a, **k):
        out = real_make(*a, **k)
        built.append(out[0])
        return out
    graph.GraphedTrainStep.__init__, cli.trust_optimizer = spy_init, spy_make
    buf = io.StringIO()
    try:
        with contextlib.redirect_stdout(buf):
            cli.main(["--train", "--fused_optimizer", "--graph", "--optimizer", kind, "--weight_decay", "1e-2", "--no_decay_norm_bias",
                      "--clip_grad_norm", "5", "--synthetic", "16", "--batch_size", "4", "--resize", "64", "--eval_interval", "100",
                      "--log_interval", "1", "--seed", "3", "--output_dir", str(tmp_path)])
    finally:
        graph.GraphedTrainStep.__init__, cli.trust_optimizer = real_init, real_make
    lines = [json.loads(l) for l in buf.getvalue().splitlines() if l.startswith('{"step"')]
    assert [l["step"] for l in lines] == [1, 2, 3, 4] and all(math.isfinite(l["train_loss"]) for l in lines), lines
    assert captures == [1]
    assert len(built) == 1 and isinstance(built[0], O.FusedLAMB if kind == "lamb" else O.FusedLARS)
    for l in lines:
        assert math.isfinite(l["trust_min"]) and math.isfinite(l["trust_max"]) and 0 < l["trust_min"] <= l["trust_max"], l
        assert math.isfinite(l["grad_norm"]) and l["grad_norm"] > 0


# ------------------------------------------------------------------------------------------------ untouched paths
@pytest.mark.parametrize("kind", ["adam", "sgd_nesterov"])
def test_grouped_adam_and_sgd_still_give_the_bits_of_their_entry_points(dev, kind):
    """The grouped SGD kernel gained a compile-time TRUST flag for LARS: FusedSGDNesterov and FusedAdam with groups still equal three
    direct launches of ops.*_step_items, bit for bit."""
    from chexpert_amd import ops, optim as O
    sizes = synthetic_sizes()
    group_of = round_robin(sizes, 3)
    net = Net(sizes, dev)
    ps = list(net.parameters())
    groups = [dict(rows3()[j], params=[p for p, q in zip(ps, group_of) if q == j]) for j in (1, 2)]
    opt = O.FusedAdam(net, lr=LR, groups=groups, ema_decay=0.9) if kind == "adam" else O.FusedSGDNesterov(net, lr=LR, groups=groups, ema_decay=0.9)
    p = net.eng.flat.clone()
    st = [torch.zeros_like(p) for _ in range(opt.NSTATE)]
    ema = p.clone()
    for it in range(3):
        net.set_grad(values(80 + it, sizes))
        opt.step()
        tail = dict(lr=LR, step=it + 1, ema=ema, ema_decay=0.9, ema_warmup=True)
        if kind == "adam":
            ops.adam_step_items(p, net.eng.flat_grad, st[0], st[1], opt._items, opt._gtab, False, 0.9, 0.999, 1e-8, **tail)
        else:
            ops.sgd_nesterov_step_items(p, net.eng.flat_grad, st[0], opt._items, opt._gtab, False, 0.9, **tail)
    assert torch.equal(net.eng.flat, p) and torch.equal(opt._ema, ema)
    assert all(torch.equal(a, b) for a, b in zip(opt._state, st))
    assert not torch.equal(p, torch.cat([torch.nn.functional.pad(v, (0, -v.numel() % 4)) for v in values(7, sizes)]).to(dev))
