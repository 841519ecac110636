"""CPU (no GPU): host side of the layer-wise trust-ratio optimisers (chexpert_amd.optim.FusedLAMB / FusedLARS): the float64
statement optim.reference_trust_step, constructor and command-line validation, the state_dict round trip, the tensor_items table,
the argument checks of cx_lamb_step_items / cx_lars_step_items before any launch, and the declarations."""
import math
import os
import re

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LR = 1e-2
BETAS = (0.9, 0.999)


def synthetic_sizes(V):
    """The ten-tensor layout of tests/test_optim_groups_cpu.py."""
    return [1, 3, 4, 5, 255, 1021, 4 * V - 4, 4 * V, 4 * V + 1, 12 * V + 7]


class _Eng:
    packed_version = 0


class Net(torch.nn.Module):
    """Flat tensors bound to one zero-padded buffer, as the engines bind a model's parameters."""

    def __init__(self, sizes):
        super().__init__()
        from chexpert_amd.models._fused import flatten
        self.w = torch.nn.ParameterList([torch.nn.Parameter(torch.arange(float(n)) / n) for n in sizes])
        self.eng = _Eng()
        self.eng.params = list(self.parameters())
        self.eng.flat, self.eng.offsets = flatten(self.eng.params, torch.device("cpu"))
        self.eng.flat_grad = torch.zeros_like(self.eng.flat)

    def _eng(self):
        return self.eng


def zeros_states(sizes):
    return [[torch.zeros(n, dtype=torch.float64), torch.zeros(n, dtype=torch.float64)] for n in sizes]


def norm(v):
    return float(v.double().pow(2).sum().sqrt())


# ---------------------------------------------------------------------------------------- LAMB, stated in float64
ROWS = [[1.0, 0.0, 0.0, 0.0], [0.1, 1e-2, 0.0, 0.0], [3.0, 1e-3, 0.0, 0.0]]         # {lr_mult, weight_decay, frozen, t0}


def lamb_case(seed=3):
    torch.manual_seed(seed)
    sizes = [7, 33, 5, 64, 9, 12]
    group_of = [k % 3 for k in range(len(sizes))]
    ps = [torch.randn(n, dtype=torch.float64) for n in sizes]
    gs = [[torch.randn(n, dtype=torch.float64) for n in sizes] for _ in range(3)]
    return sizes, group_of, ps, gs


def adam_update(g_steps, t, eps):
    """m-hat / (sqrt(v-hat) + eps) after t steps of the gradients g_steps[:t], and sqrt(v-hat)."""
    m = torch.zeros_like(g_steps[0])
    v = torch.zeros_like(g_steps[0])
    for g in g_steps[:t]:
        m = BETAS[0] * m + (1 - BETAS[0]) * g
        v = BETAS[1] * v + (1 - BETAS[1]) * g * g
    s = (v / (1 - BETAS[1] ** t)).sqrt()
    return (m / (1 - BETAS[0] ** t)) / (s + eps), s


@pytest.mark.parametrize("always_adapt", [False, True])
def test_lamb_moves_every_adapted_tensor_by_lr_times_its_norm(always_adapt):
    from chexpert_amd.optim import reference_trust_step
    sizes, group_of, ps, gs = lamb_case()
    st = zeros_states(sizes)
    for t in range(1, 4):
        new, ratios = reference_trust_step("lamb", ps, gs[t - 1], st, LR, t, ROWS, group_of, eps=1e-6, always_adapt=always_adapt)
        for k in range(len(sizes)):
            lr_mult, wd = ROWS[group_of[k]][:2]
            r, wn, un, adapted = ratios[k]
            assert adapted == (wd != 0 or always_adapt)
            assert abs(wn - norm(ps[k])) <= 1e-12 * wn
            if adapted:
                moved = norm(new[k] - ps[k])
                assert abs(moved - LR * lr_mult * wn) <= 1e-12 * LR * lr_mult * wn, (t, k, moved)
                assert abs(r - wn / un) <= 1e-15 * r
            else:
                # r = 1: exactly the bias-corrected Adam statement (the group's decay is 0)
                a, _ = adam_update([g[k] for g in gs], t, 1e-6)
                assert r == 1.0
                assert (new[k] - (ps[k] - LR * lr_mult * a)).abs().max().item() <= 1e-15 * (1 + ps[k].abs().max().item())
        ps = new


def test_lamb_ratio_is_one_for_a_zero_tensor_or_a_zero_update_and_clip_caps_it():
    from chexpert_amd.optim import reference_trust_step
    rows = [[1.0, 1e-2, 0.0, 0.0], [1.0, 0.0, 0.0, 0.0]]
    ps = [torch.zeros(5, dtype=torch.float64), torch.ones(4, dtype=torch.float64), 10.0 * torch.ones(6, dtype=torch.float64)]
    gs = [torch.ones(5, dtype=torch.float64), torch.zeros(4, dtype=torch.float64), torch.ones(6, dtype=torch.float64)]
    group_of = [0, 1, 0]
    new, ratios = reference_trust_step("lamb", ps, gs, zeros_states([5, 4, 6]), LR, 1, rows, group_of, eps=1e-6, always_adapt=True)
    assert ratios[0][0] == 1.0 and ratios[0][1] == 0.0 and ratios[0][3]            # p = 0: the plain update
    assert (new[0] + LR * (1.0 / (1.0 + 1e-6))).abs().max().item() <= 1e-15
    assert ratios[1][0] == 1.0 and ratios[1][2] == 0.0 and torch.equal(new[1], ps[1])      # u = 0 (g = 0, wd = 0): nothing moves
    # |p| = 10 sqrt(6), |u| = (1 / (1 + eps) + 0.1) sqrt(6): r ~ 9.09, capped at 1 under trust_clip
    assert abs(ratios[2][0] - 10.0 / (1.0 / (1.0 + 1e-6) + 0.1)) <= 1e-12
    _, clipped = reference_trust_step("lamb", ps, gs, zeros_states([5, 4, 6]), LR, 1, rows, group_of, eps=1e-6, always_adapt=True,
                                      trust_clip=True)
    assert [c[0] for c in clipped] == [1.0, 1.0, 1.0]
    # a ratio below 1 is left alone by the clip
    small = [0.01 * torch.ones(6, dtype=torch.float64)]
    _, a = reference_trust_step("lamb", small, [torch.ones(6, dtype=torch.float64)], zeros_states([6]), LR, 1, rows, [0], eps=1e-6)
    _, b = reference_trust_step("lamb", small, [torch.ones(6, dtype=torch.float64)], zeros_states([6]), LR, 1, rows, [0], eps=1e-6,
                                trust_clip=True)
    assert a[0][0] < 1.0 and a[0][0] == b[0][0]


def test_lamb_is_invariant_to_the_gradient_scale_up_to_the_eps_term():
    """Every gradient times c = 64 over three steps.  The moments scale with c, so the Adam part a_i = m-hat_i / (s_i + eps),
    s_i = sqrt(v-hat_i), becomes m-hat_i / (s_i + eps / c): elementwise |a'_i - a_i| <= delta |a_i| with
    delta = eps (1 - 1 / c) / (s_i + eps / c) <= eps / min_i s_i.  With u = a + wd p at equal p that is |u' - u| <= delta |a|, and a
    normalised vector moves by at most twice the relative change of its argument, so one step's p differs by at most
    lr_g |p| 2 delta kappa, kappa = |a| / |u|.  A difference d in p going into a step leaves it as at most (1 + L) d with
    L = lr_g (1 + 2 (1 + wd |p| / |u|)) (the factor |p| and the direction of u = a + wd p both depend on p).  Three steps:
    bound = sum_t step_t prod_{later} (1 + L).  Without the trust ratio and the bias-corrected denominator nothing of the kind holds:
    plain SGD's three steps would differ by a factor 64."""
    from chexpert_amd.optim import reference_trust_step
    sizes, group_of, ps0, gs = lamb_case(5)
    eps, c = 1e-6, 64.0
    rows = [[1.0, 1e-2, 0.0, 0.0], [0.1, 1e-2, 0.0, 0.0], [3.0, 1e-3, 0.0, 0.0]]
    runs = []
    for scale in (1.0, c):
        ps, st, trace = [p.clone() for p in ps0], zeros_states(sizes), []
        for t in range(1, 4):
            new, ratios = reference_trust_step("lamb", ps, [scale * g for g in gs[t - 1]], st, LR, t, rows, group_of, eps=eps)
            trace.append((ps, ratios))
            ps = new
        runs.append((ps, trace))
    for k in range(len(sizes)):
        lr_g, wd = LR * rows[group_of[k]][0], rows[group_of[k]][1]
        bound = 0.0
        for t in range(1, 4):
            a, s = adam_update([g[k] for g in gs], t, eps)
            delta = eps / s.min().item()
            _, wn, un, _ = runs[0][1][t - 1][1][k]
            bound = bound * (1.0 + lr_g * (1.0 + 2.0 * (1.0 + wd * wn / un))) + lr_g * wn * 2.0 * delta * norm(a) / un
        diff = norm(runs[0][0][k] - runs[1][0][k])
        moved = norm(runs[0][0][k] - ps0[k])
        print("tensor %d: |p(64 g) - p(g)| = %.3e, bound %.3e, three steps moved p by %.3e" % (k, diff, bound, moved))
        assert diff <= bound
        assert bound < 1e-2 * moved                                        # the bound says something


# ---------------------------------------------------------------------------------------- LARS, stated in float64
def test_lars_matches_a_hand_computed_two_tensor_case():
    """Tensor 0: p = (3, 4), g = (0.6, 0.8), wd = 0.1, coef = 0.1, eps = 0: r = 0.1 * 5 / (1 + 0.5) = 1 / 3,
    g' = (g + 0.1 p) / 3 = (0.3, 0.4), buf = g', p <- p - 0.1 * 1.9 * g' = (2.943, 3.924).  Tensor 1 sits in a group without decay
    (lr_mult 2): not adapted, r = 1, p <- (1, -2) - 0.2 * 1.9 * (0.5, 0.5) = (0.81, -2.19).  A second step with the same gradients:
    tensor 1's buf = 0.9 * 0.5 + 0.5 = 0.95, p <- (0.81, -2.19) - 0.2 * (0.5 + 0.9 * 0.95) = (0.539, -2.461)."""
    from chexpert_amd.optim import reference_trust_step
    ps = [torch.tensor([3.0, 4.0], dtype=torch.float64), torch.tensor([1.0, -2.0], dtype=torch.float64)]
    gs = [torch.tensor([0.6, 0.8], dtype=torch.float64), torch.tensor([0.5, 0.5], dtype=torch.float64)]
    rows = [{"lr_mult": 1.0, "weight_decay": 0.1}, {"lr_mult": 2.0, "weight_decay": 0.0}]
    st = zeros_states([2, 2])
    new, ratios = reference_trust_step("lars", ps, gs, st, 0.1, 1, rows, [0, 1], momentum=0.9, trust_coef=0.1, eps=0.0)
    assert abs(ratios[0][0] - 1.0 / 3.0) <= 1e-15 and ratios[0][1] == 5.0 and abs(ratios[0][2] - 1.0) <= 1e-15 and ratios[0][3]
    assert ratios[1][0] == 1.0 and not ratios[1][3]
    assert (new[0] - torch.tensor([2.943, 3.924], dtype=torch.float64)).abs().max().item() <= 1e-14
    assert (new[1] - torch.tensor([0.81, -2.19], dtype=torch.float64)).abs().max().item() <= 1e-14
    assert (st[0][0] - torch.tensor([0.3, 0.4], dtype=torch.float64)).abs().max().item() <= 1e-15
    new2, _ = reference_trust_step("lars", new, gs, st, 0.1, 2, rows, [0, 1], momentum=0.9, trust_coef=0.1, eps=0.0)
    assert (new2[1] - torch.tensor([0.539, -2.461], dtype=torch.float64)).abs().max().item() <= 1e-14
    # the clip leaves 1/3 alone and caps a ratio above 1
    _, big = reference_trust_step("lars", ps, gs, zeros_states([2, 2]), 0.1, 1, rows, [0, 1], trust_coef=3.0, eps=0.0)
    _, cap = reference_trust_step("lars", ps, gs, zeros_states([2, 2]), 0.1, 1, rows, [0, 1], trust_coef=3.0, eps=0.0, trust_clip=True)
    assert abs(big[0][0] - 10.0) <= 1e-14 and cap[0][0] == 1.0
    # p = 0 or g = 0: r = 1
    zero = [torch.zeros(2, dtype=torch.float64), torch.ones(2, dtype=torch.float64)]
    _, rz = reference_trust_step("lars", zero, [gs[0], torch.zeros(2, dtype=torch.float64)], zeros_states([2, 2]), 0.1, 1, rows, [0, 0],
                                 trust_coef=0.1)
    assert rz[0][0] == 1.0 and rz[1][0] == 1.0 and rz[0][3] and rz[1][3]


def test_lars_with_ratio_one_is_sgd_nesterov():
    """coef = (|g| + wd |p| + eps) / |p| makes r = 1 (to an ulp): three steps equal reference_step("sgd_nesterov") with the same decay."""
    from chexpert_amd.optim import reference_step, reference_trust_step
    torch.manual_seed(9)
    n, wd, eps, lr_mult = 37, 1e-2, 1e-3, 0.5
    p = torch.randn(n, dtype=torch.float64)
    q = p.clone()
    st, st_ref = zeros_states([n]), [torch.zeros(n, dtype=torch.float64), torch.zeros(n, dtype=torch.float64)]
    for t in range(1, 4):
        g = torch.randn(n, dtype=torch.float64)
        coef = (norm(g) + wd * norm(p) + eps) / norm(p)
        (p,), ratios = reference_trust_step("lars", [p], [g], st, LR, t, [[lr_mult, wd, 0.0, 0.0]], [0], trust_coef=coef, eps=eps)
        assert abs(ratios[0][0] - 1.0) <= 4e-16
        q = reference_step("sgd_nesterov", q, g, st_ref, LR, t, lr_mult=lr_mult, weight_decay=wd)
    assert (p - q).abs().max().item() <= 1e-14 * (1 + q.abs().max().item())
    assert (st[0][0] - st_ref[0]).abs().max().item() <= 1e-14


def test_frozen_group_and_t0_in_the_statement():
    from chexpert_amd.optim import reference_trust_step
    sizes, group_of, ps, gs = lamb_case(7)
    rows = [list(r) for r in ROWS]
    rows[1][2] = 1.0
    for kind in ("lamb", "lars"):
        st = zeros_states(sizes)
        new, ratios = reference_trust_step(kind, ps, gs[0], st, LR, 1, rows, group_of)
        for k in range(len(sizes)):
            if group_of[k] == 1:
                assert new[k] is ps[k] and ratios[k] == (1.0, 0.0, 0.0, False) and not st[k][0].any() and not st[k][1].any()
            else:
                assert not torch.equal(new[k], ps[k])
    # t0: LAMB's bias corrections count the group's own steps
    a, _ = reference_trust_step("lamb", ps, gs[0], zeros_states(sizes), LR, 1, ROWS, group_of)
    late = [[r[0], r[1], 0.0, 2.0] for r in ROWS]
    b, _ = reference_trust_step("lamb", ps, gs[0], zeros_states(sizes), LR, 3, late, group_of)
    assert all(torch.equal(x, y) for x, y in zip(a, b))
    with pytest.raises(ValueError, match="kind"):
        reference_trust_step("adam", ps, gs[0], zeros_states(sizes), LR, 1, ROWS, group_of)


# ---------------------------------------------------------------------------------------- constructors, state_dict, tensor_items
def test_constructors_refuse_what_has_no_meaning():
    from chexpert_amd import optim as O
    net = Net([5, 9])
    with pytest.raises(ValueError, match="decoupled"):
        O.FusedLAMB(net, decoupled=True)
    with pytest.raises(ValueError, match="decoupled"):
        O.FusedLARS(net, lr=0.1, decoupled=True)
    for bad in (0.0, -1.0, float("nan")):
        with pytest.raises(ValueError, match="trust_coef"):
            O.FusedLARS(net, lr=0.1, trust_coef=bad)
    with pytest.raises(ValueError, match="eps"):
        O.FusedLAMB(net, eps=0.0)
    with pytest.raises(ValueError, match="max_grad_norm"):
        O.FusedLAMB(net, max_grad_norm=0.0)                         # the shared options are still checked
    lamb = O.FusedLAMB(net)
    lars = O.FusedLARS(net, lr=0.1)
    assert lamb._grouped and lars._grouped                          # groups=None: one default group, the grouped path
    assert lamb.group_names == ["default"] and lamb._grows == [[1.0, 0.0, 0.0, 0.0]]
    assert (lamb.lr, lamb.betas, lamb.eps, lamb.always_adapt, lamb.trust_clip) == (1e-3, (0.9, 0.999), 1e-6, False, False)
    assert (lars.momentum, lars.trust_coef, lars.trust_eps, lars.milestones, lars.gamma) == (0.9, 0.001, 1e-8, (40000, 60000), 0.1)
    assert isinstance(lars, O.FusedSGDNesterov) and lars._sched[0] == 2
    assert (lamb.NSTATE, lamb.KIND, lars.NSTATE, lars.KIND) == (2, "lamb", 1, "lars")
    # what graph.py asks to size the states
    assert hasattr(lamb, "betas") and not hasattr(lars, "betas") and not hasattr(lars, "alpha")
    assert lamb.trust_ratios() == {}


def test_state_dict_round_trip_and_another_kind_is_refused():
    from chexpert_amd import optim as O
    net = Net([5, 9, 12])
    groups = [{"params": [net.w[1]], "lr_mult": 0.1, "weight_decay": 1e-2, "name": "mid"}]
    a = O.FusedLARS(net, lr=0.1, trust_coef=0.02, eps=1e-7, trust_clip=True, always_adapt=True, groups=groups, ema_decay=0.9)
    sd = a.state_dict()
    assert sd["kind"] == "FusedLARS" and sd["trust"] == {"coef": 0.02, "eps": 1e-7, "trust_clip": True, "always_adapt": True}
    assert sd["groups"]["names"] == ["default", "mid"] and not sd["groups"]["decoupled"]
    b = O.FusedLARS(net, lr=0.3, groups=groups, ema_decay=0.9)
    b.load_state_dict(sd)
    assert (b.trust_coef, b.trust_eps, b.trust_clip, b.always_adapt, b.lr) == (0.02, 1e-7, True, True, 0.1)
    assert b.state_dict()["trust"] == sd["trust"]
    lamb = O.FusedLAMB(net, eps=1e-5, groups=groups)
    sd_l = lamb.state_dict()
    assert sd_l["trust"] == {"coef": 1.0, "eps": 1e-5, "trust_clip": False, "always_adapt": False}
    assert not {"u", "partials", "trust_table"} & set(sd_l)         # scratch, partials and the trust table are not state
    c = O.FusedLAMB(net, groups=groups)
    c.load_state_dict(sd_l)
    assert c.eps == 1e-5
    adam_sd = O.FusedAdam(net, groups=groups).state_dict()
    for other in (lamb, a):
        with pytest.raises(RuntimeError, match="FusedAdam"):
            other.load_state_dict(adam_sd)
    with pytest.raises(RuntimeError, match="FusedLARS"):
        O.FusedSGDNesterov(net, lr=0.1, groups=groups).load_state_dict(sd)
    with pytest.raises(RuntimeError, match="FusedLAMB"):
        a.load_state_dict(sd_l)


def test_tensor_items_point_at_each_tensors_first_item():
    from chexpert_amd import ops, optim as O
    V = ops.optim_item_vec4()
    sizes = synthetic_sizes(V)
    group_of = [k % 3 for k in range(len(sizes))]
    items = O.item_table(sizes, group_of)
    starts = O.tensor_items(items, len(sizes))
    assert starts == [0, 1, 2, 3, 4, 5, 6, 7, 8, 10, 14] and starts[-1] == len(items)
    for k in range(len(sizes)):
        assert items[starts[k]][3] == k and (starts[k] == 0 or items[starts[k] - 1][3] == k - 1)
        assert all(it[3] == k for it in items[starts[k]:starts[k + 1]])
    # a tensor without elements owns no item; a table out of tensor order is refused
    assert O.tensor_items(O.item_table([4, 0, 9], [0, 0, 0]), 3) == [0, 1, 1, 2]
    with pytest.raises(ValueError):
        O.tensor_items([(0, 1, 0, 1), (1, 1, 0, 0)], 2)
    with pytest.raises(ValueError):
        O.tensor_items(items, len(sizes) - 1)
    # the optimisers build it beside their states, with the partials, the trust table and (LAMB) the scratch for u
    net = Net(sizes)
    groups = [{"params": [p for k, p in enumerate(net.parameters()) if k % 3 == j]} for j in (1, 2)]
    for o in (O.FusedLAMB(net, groups=groups), O.FusedLARS(net, lr=0.1, groups=groups)):
        o._bufs(o.NSTATE)
        assert o._titems.dtype == torch.int32 and o._titems.tolist() == starts
        assert [t.numel() for t in o._tpart] == [len(items)] * 2 and tuple(o._trust.shape) == (len(sizes), 4)
        assert (o._u is not None) == (o.KIND == "lamb") and len(o._state) == o.NSTATE
        assert o._u is None or (o._u.shape == net.eng.flat.shape and not o._u.any())
        assert set(o.trust_ratios()) == {"w.%d" % k for k in range(len(sizes))}


# ---------------------------------------------------------------------------------------- the command line
def test_cli_flags_are_validated_before_anything_is_built():
    from chexpert_amd import cli
    a = cli.build_parser().parse_args([])
    assert (a.optimizer, a.trust_coef, a.trust_clip, a.always_adapt) == (None, None, False, False)      # the defaults: nothing changes
    assert cli.trust_options(a) == {} and cli.group_options(a) == {} and cli.optimizer_options(a) == {}
    assert cli.fused_optimizer_kwargs(a, None) == {}
    f = cli.build_parser().parse_args(["--fused_optimizer"])
    assert cli.trust_options(f) == {} and cli.fused_optimizer_kwargs(f, None) == {}
    for kind in ("lamb", "lars"):
        with pytest.raises(ValueError, match="--fused_optimizer"):
            cli.main(["--optimizer", kind])                                  # raised before anything touches data or the GPU
        with pytest.raises(ValueError, match="--decoupled_decay cannot be combined with --optimizer %s" % kind):
            cli.main(["--fused_optimizer", "--optimizer", kind, "--weight_decay", "1e-2", "--decoupled_decay"])
    with pytest.raises(ValueError, match="--trust_coef"):
        cli.main(["--fused_optimizer", "--optimizer", "lamb", "--trust_coef", "0.01"])
    for bad in ("0", "-1", "nan"):
        with pytest.raises(ValueError, match="--trust_coef"):
            cli.main(["--fused_optimizer", "--optimizer", "lars", "--trust_coef", bad])
    for argv in (["--trust_coef", "0.01"], ["--trust_clip"], ["--always_adapt"]):
        with pytest.raises(ValueError, match="--optimizer"):
            cli.main(["--fused_optimizer"] + argv)
    with pytest.raises(SystemExit):
        cli.build_parser().parse_args(["--optimizer", "adamw"])
    b = cli.build_parser().parse_args(["--fused_optimizer", "--optimizer", "lars", "--trust_coef", "0.02", "--trust_clip"])
    assert cli.trust_options(b) == {"kind": "lars", "trust_coef": 0.02, "trust_clip": True, "always_adapt": False}
    c = cli.build_parser().parse_args(["--fused_optimizer", "--optimizer", "lamb", "--always_adapt", "--weight_decay", "1e-2",
                                       "--no_decay_norm_bias", "--clip_grad_norm", "5", "--head_lr_mult", "10"])
    assert cli.trust_options(c) == {"kind": "lamb", "trust_clip": False, "always_adapt": True}
    from chexpert_amd import optim as O
    from chexpert_amd.models import DenseNet
    m = DenseNet(32, (2, 2, 2, 2), 64, num_classes=5)
    opt, sched = cli.trust_optimizer(c, m, cli.trust_options(c))
    assert isinstance(opt, O.FusedLAMB) and sched is None and opt.always_adapt and opt.max_grad_norm == 5.0
    assert opt.group_names == ["default", "backbone", "backbone_no_decay", "head", "head_no_decay"]
    assert [r[1] for r in opt._grows] == [1e-2, 1e-2, 0.0, 1e-2, 0.0] and [r[0] for r in opt._grows] == [1.0, 1.0, 1.0, 10.0, 10.0]
    opt, sched = cli.trust_optimizer(b, m, cli.trust_options(b))
    assert isinstance(opt, O.FusedLARS) and sched == "fused" and opt.trust_coef == 0.02 and opt.trust_clip and opt._grouped
    doc = cli.__doc__
    for flag in ("--optimizer lamb|lars", "--trust_coef", "--trust_clip", "--always_adapt"):
        assert flag in doc, flag


# ---------------------------------------------------------------------------------------- argument checks before any launch
def test_ops_wrappers_refuse_bad_arguments_before_any_launch():
    from chexpert_amd import ops
    n = 8
    p, g, m, v, u = (torch.zeros(n) for _ in range(5))
    items = torch.tensor([[0, 2, 0, 0]], dtype=torch.int32)
    groups = torch.tensor([[1.0, 0.0, 0.0, 0.0]])
    ti = torch.tensor([0, 1], dtype=torch.int32)
    parts, trust = (torch.zeros(1), torch.zeros(1)), torch.zeros(1, 4)

    def lamb(decoupled=False, eps=1e-6, **kw):
        return ops.lamb_step_items(p, g, m, v, items, groups, decoupled, 0.9, 0.999, eps, ti, parts, trust, u, lr=1e-3, step=1, **kw)

    def lars(decoupled=False, coef=0.001, eps=1e-8, **kw):
        return ops.lars_step_items(p, g, m, items, groups, decoupled, 0.9, ti, parts, trust, coef, eps, lr=1e-3, step=1, **kw)
    with pytest.raises(ValueError, match="decoupled"):
        lamb(decoupled=True)
    with pytest.raises(ValueError, match="decoupled"):
        lars(decoupled=True)
    with pytest.raises(ValueError, match="eps"):
        lamb(eps=0.0)
    with pytest.raises(ValueError, match="coefficient"):
        lars(coef=0.0)
    with pytest.raises(ValueError, match="eps"):
        lars(eps=-1.0)
    for fn in (lamb, lars):
        with pytest.raises(RuntimeError, match="GPU only"):
            fn()                                                             # host tensors: no CPU fallback, nothing launched
    assert not p.any() and not m.any() and not u.any()


def test_entry_points_validate_before_launching():
    """Argument validation happens before the first of the three launches, so it can be exercised without a GPU."""
    import ctypes
    from chexpert_amd import _lib
    l = _lib.lib()
    buf = (ctypes.c_float * 64)()
    base = ctypes.addressof(buf)
    base += (-base) % 16
    tab = base + 64                                           # 16-byte aligned "tables" in the same host array (never read)
    EINVAL, EALIGN = -1, -2
    tail = (None, None, 0.0, 0, 0)                            # clip, ema, ema_decay, ema_warmup, skip_nonfinite

    def lamb(p=base, g=base, m=base, v=base, n=8, items=tab, ni=1, groups=tab, ng=1, dec=0, hyper=None, step=1, eps=1e-6, tail=tail, ti=tab,
             nt=1, pw=base, pu=base, trust=base, u=base):
        return l.cx_lamb_step_items(p, g, m, v, n, items, ni, groups, ng, dec, hyper, 1e-3, step, 0.9, 0.999, eps, 1.0, *tail, ti, nt, pw, pu,
                                    trust, u, 0, 0, None)

    def lars(p=base, g=base, m=base, n=8, items=tab, ni=1, groups=tab, ng=1, dec=0, hyper=None, step=1, tail=tail, ti=tab, nt=1, pw=base,
             pu=base, trust=base, coef=0.001, eps=1e-8):
        return l.cx_lars_step_items(p, g, m, n, items, ni, groups, ng, dec, hyper, 1e-3, step, 0.9, 1.0, *tail, ti, nt, pw, pu, trust, coef,
                                    eps, 0, 0, None)
    for fn in (lamb, lars):
        assert fn(items=None) == EINVAL and fn(groups=None) == EINVAL          # the checks of the grouped steps ...
        assert fn(ng=0) == EINVAL and fn(ng=257) == EINVAL
        assert fn(ni=0) == EINVAL and fn(n=6) == EINVAL
        assert fn(p=None) == EINVAL and fn(g=None) == EINVAL and fn(m=None) == EINVAL
        assert fn(p=base + 4) == EALIGN and fn(g=base + 4) == EALIGN and fn(m=base + 8) == EALIGN
        assert fn(items=tab + 4) == EALIGN and fn(groups=tab + 8) == EALIGN
        assert fn(step=0) == EINVAL
        assert fn(tail=(None, base, 1.5, 0, 0)) == EINVAL and fn(tail=(None, base + 4, 0.5, 0, 0)) == EALIGN
        assert fn(dec=1) == EINVAL                                             # ... and the trust tables' own
        assert fn(nt=0) == EINVAL and fn(nt=-3) == EINVAL
        assert fn(ti=None) == EINVAL and fn(trust=None) == EINVAL
        assert fn(pw=None) == EINVAL and fn(pu=None) == EINVAL
        assert fn(n=0, ni=0) == 0                                              # nothing to do: no launch
    assert lamb(v=None) == EINVAL and lamb(v=base + 12) == EALIGN
    assert lamb(u=None) == EINVAL and lamb(u=base + 4) == EALIGN
    assert lamb(eps=0.0) == EINVAL
    assert lars(coef=0.0) == EINVAL and lars(coef=-1.0) == EINVAL and lars(eps=-1.0) == EINVAL


def test_header_declares_the_entry_points_and_lib_lists_them():
    from chexpert_amd import _lib
    header = open(os.path.join(ROOT, "include", "chexpert_hip.h")).read()
    for name in ("cx_lamb_step_items", "cx_lars_step_items"):
        m = re.search(r"\bint %s\(([^;]*)\);" % name, header)
        assert m, name
        assert name in _lib.SIGNATURES and len(_lib.SIGNATURES[name]) == m.group(1).count(",") + 1
        assert hasattr(_lib.lib(), name)
    for name in ("lamb_step_items", "lars_step_items"):
        from chexpert_amd import ops
        assert callable(getattr(ops, name))
    assert math.isfinite(_lib.lib().cx_optim_item_vec4())
