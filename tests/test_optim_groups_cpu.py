"""CPU (no GPU): host side of the parameter groups of the fused optimisers: the item table, constructor and command-line validation,
finetune_groups, the state_dict round trip, argument checks of the new entry points before any launch, and the float64 restatement
of the grouped rules (chexpert_amd.optim.reference_step) against torch.optim built with real param_groups."""
import math
import os
import re

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KINDS = ["adam", "sgd_nesterov", "rmsprop"]


def synthetic_sizes(V):
    """Floats per tensor: one short of / exactly / one past a 16-byte unit, odd sizes, one short of / exactly / one float past a
    whole item (V 16-byte units = 4 V floats) and a tensor of four items."""
    return [1, 3, 4, 5, 255, 1021, 4 * V - 4, 4 * V, 4 * V + 1, 12 * V + 7]


class _Eng:
    packed_version = 0


class Net(torch.nn.Module):
    """Ten flat tensors bound to one zero-padded buffer, as the engines bind a model's parameters."""

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


def test_item_table_covers_the_buffer_once_and_keeps_tensors_apart():
    from chexpert_amd import _lib, ops, optim
    V = _lib.lib().cx_optim_item_vec4()
    assert V == ops.optim_item_vec4() and V >= 1
    sizes = synthetic_sizes(V)
    group_of = [k % 3 for k in range(len(sizes))]
    items = optim.item_table(sizes, group_of)
    offs, at = [], 0
    for n in sizes:                                        # _fused.flatten's layout
        offs.append(at)
        at += (n + 3) // 4 * 4
    nxt = 0
    for start4, len4, grp, tensor in items:
        assert start4 == nxt and 1 <= len4 <= V            # in order, no gap, no overlap, none longer than V
        nxt = start4 + len4
        lo, hi = offs[tensor] // 4, (offs[tensor] + sizes[tensor] + 3) // 4
        assert lo <= start4 and start4 + len4 <= hi        # inside ONE tensor (padding included)
        assert grp == group_of[tensor]
    assert 4 * nxt == at
    per_tensor = [sum(1 for it in items if it[3] == k) for k in range(len(sizes))]
    assert per_tensor == [1, 1, 1, 1, 1, 1, 1, 1, 2, 4]
    # each tensor's items are as long as they can be: only its last one is shorter than V
    for k in range(len(sizes)):
        lens = [it[1] for it in items if it[3] == k]
        assert all(v == V for v in lens[:-1]) and sum(lens) == (sizes[k] + 3) // 4
    # a function of shapes and assignment alone; another cut on request
    assert optim.item_table(sizes, group_of) == items
    small = optim.item_table(sizes, group_of, vec4=7)
    assert max(it[1] for it in small) == 7 and sum(it[1] for it in small) == at // 4
    # the optimiser builds the same table beside its states
    net = Net(sizes)
    groups = [{"params": [p for k, p in enumerate(net.parameters()) if k % 3 == j]} for j in (1, 2)]
    o = optim.FusedAdam(net, lr=1e-3, groups=groups)
    o._bufs(2)
    assert o._items.dtype == torch.int32 and o._items.tolist() == [list(it) for it in items]
    assert o._gtab.tolist() == [[1.0, 0.0, 0.0, 0.0]] * 3
    assert o._gpart.numel() == len(items) and o._gsq.numel() == 3 and o._gnorm.numel() == 3


def test_constructor_validation():
    from chexpert_amd.optim import FusedAdam, FusedRMSprop, FusedSGDNesterov
    net = Net([5, 8, 3])
    a, b, c = list(net.parameters())
    stranger = torch.nn.Parameter(torch.zeros(4))
    for cls in (FusedAdam, FusedSGDNesterov, FusedRMSprop):
        with pytest.raises(ValueError, match="twice"):
            cls(net, lr=1e-3, groups=[{"params": [a]}, {"params": [a, b]}])
        with pytest.raises(ValueError, match="not the model's"):
            cls(net, lr=1e-3, groups=[{"params": [stranger]}])
        with pytest.raises(ValueError, match="256"):
            cls(net, lr=1e-3, groups=[{"params": []} for _ in range(256)])
        for bad in (-1.0, float("nan"), float("inf")):
            with pytest.raises(ValueError, match="lr_mult"):
                cls(net, lr=1e-3, groups=[{"params": [a], "lr_mult": bad}])
        with pytest.raises(ValueError):
            cls(net, lr=1e-3, groups=[{"params": [a], "learning_rate": 2.0}])
    o = FusedAdam(net, lr=1e-3, weight_decay=0.5, groups=[{"params": [c], "lr_mult": 0.0}, {"params": [a], "weight_decay": 0.0, "frozen": True}])
    assert o._grows == [[1.0, 0.5, 0.0, 0.0], [0.0, 0.5, 0.0, 0.0], [1.0, 0.0, 1.0, 0.0]]      # the constructor's decay is the default
    assert o._gparams == [["w.1"], ["w.2"], ["w.0"]]                                            # unnamed parameters: group 0
    assert FusedAdam(net, lr=1e-3, groups=[{"params": []} for _ in range(255)])._grouped       # 255 dicts + the default group = 256
    with pytest.raises(ValueError, match="lr_mult"):
        o.set_group(1, lr_mult=-2.0)
    with pytest.raises(RuntimeError, match="groups"):
        FusedAdam(net, lr=1e-3).set_group(0, frozen=True)


def test_set_group_rewrites_the_row_and_counts_the_steps_sat_out():
    from chexpert_amd.optim import FusedAdam
    net = Net([5, 8, 3])
    a, b, c = list(net.parameters())
    o = FusedAdam(net, lr=1e-3, groups=[{"params": [a], "frozen": True}, {"params": [b]}])
    o._bufs(2)
    o.step_count = 2
    o.set_group(1, frozen=False)                            # frozen from the start: t0 = the steps done
    assert o._grows[1] == [1.0, 0.0, 0.0, 2.0] and o._gtab[1].tolist() == [1.0, 0.0, 0.0, 2.0]
    o.set_group(2, lr_mult=0.25, weight_decay=0.125)
    assert o._gtab[2].tolist() == [0.25, 0.125, 0.0, 0.0]
    o.step_count = 5
    o.set_group(1, frozen=True)
    o.step_count = 9
    o.set_group(1, frozen=False)                            # sat out 2 + 4 steps
    assert o._gtab[1].tolist() == [1.0, 0.0, 0.0, 6.0]
    o.set_group(1, frozen=False)                            # no change: nothing counted twice
    assert o._gtab[1].tolist() == [1.0, 0.0, 0.0, 6.0]


def test_finetune_groups_on_the_small_densenet():
    from chexpert_amd.models import DenseNet
    from chexpert_amd.optim import FusedAdam, finetune_groups
    m = DenseNet(32, (2, 2, 2, 2), 64, num_classes=5)
    names = {id(p): n for n, p in m.named_parameters()}
    g = finetune_groups(m)
    assert [d["name"] for d in g] == ["backbone", "head"]
    assert sorted(names[id(p)] for p in g[1]["params"]) == ["classifier.bias", "classifier.weight"]
    assert len(g[0]["params"]) + 2 == len(names)
    assert all(d["lr_mult"] == 1.0 and d["weight_decay"] == 0.0 and d["frozen"] is False for d in g)
    g = finetune_groups(m, weight_decay=1e-4, no_decay_norm_bias=True, head_lr_mult=10.0, backbone_lr_mult=0.5, freeze_backbone=True)
    by = {d["name"]: d for d in g}
    assert list(by) == ["backbone", "backbone_no_decay", "head", "head_no_decay"]
    assert [names[id(p)] for p in by["head"]["params"]] == ["classifier.weight"]
    assert [names[id(p)] for p in by["head_no_decay"]["params"]] == ["classifier.bias"]
    assert all(p.dim() <= 1 for p in by["backbone_no_decay"]["params"]) and all(p.dim() > 1 for p in by["backbone"]["params"])
    assert any("norm" in names[id(p)] for p in by["backbone_no_decay"]["params"])
    assert sum(len(d["params"]) for d in g) == len(names)                       # a partition of the model's parameters
    assert (by["backbone"]["weight_decay"], by["backbone_no_decay"]["weight_decay"], by["head"]["weight_decay"],
            by["head_no_decay"]["weight_decay"]) == (1e-4, 0.0, 1e-4, 0.0)
    assert [d["lr_mult"] for d in g] == [0.5, 0.5, 10.0, 10.0] and [d["frozen"] for d in g] == [True, True, False, False]
    o = FusedAdam(m, lr=1e-3, groups=g)
    assert o.group_names == ["default", "backbone", "backbone_no_decay", "head", "head_no_decay"] and o._gparams[0] == []
    with pytest.raises(ValueError, match="nn.Linear"):
        finetune_groups(torch.nn.Conv2d(3, 3, 1))


def test_state_dict_round_trip_and_refusal_of_another_partition():
    from chexpert_amd.optim import FusedAdam
    net = Net([5, 8, 3])
    a, b, c = list(net.parameters())
    groups = [{"params": [a], "lr_mult": 3.0, "frozen": True, "name": "first"}, {"params": [b], "weight_decay": 0.25}]
    o = FusedAdam(net, lr=1e-3, decoupled=True, groups=groups)
    o._bufs(2)
    o.step_count = 4
    o.set_group(1, frozen=False)
    sd = o.state_dict()
    assert set(sd) == {"kind", "lr", "base_lr", "step_count", "sched_steps", "state", "groups"}
    assert sd["groups"]["rows"] == [[1.0, 0.0, 0.0, 0.0], [3.0, 0.0, 0.0, 4.0], [1.0, 0.25, 0.0, 0.0]]
    assert sd["groups"]["decoupled"] is True and sd["groups"]["params"] == [["w.2"], ["w.0"], ["w.1"]]
    p = FusedAdam(net, lr=1.0, decoupled=True, groups=[{"params": [a], "frozen": True}, {"params": [b]}])
    p._bufs(2)
    p.load_state_dict(sd)
    assert p._grows == sd["groups"]["rows"] and p._gtab.tolist() == sd["groups"]["rows"] and p.step_count == 4
    assert p.state_dict()["groups"] == dict(sd["groups"], names=["default", "group1", "group2"])
    # another partition: refused, naming the parameter that moved
    q = FusedAdam(net, lr=1.0, decoupled=True, groups=[{"params": [a]}, {"params": [c]}])
    with pytest.raises(RuntimeError, match=r"w\.[12] is in group"):
        q.load_state_dict(sd)
    with pytest.raises(RuntimeError, match="decoupled"):
        FusedAdam(net, lr=1.0, groups=[{"params": [a]}, {"params": [b]}]).load_state_dict(sd)
    with pytest.raises(RuntimeError, match="parameter groups"):
        FusedAdam(net, lr=1.0).load_state_dict(sd)
    # a checkpoint written without groups loads, and leaves groups off / as constructed
    plain = FusedAdam(net, lr=1e-3)
    plain._state = [torch.zeros(16), torch.ones(16)]
    sd0 = plain.state_dict()
    r = FusedAdam(net, lr=1.0)
    r.load_state_dict(sd0)
    assert not r._grouped and "groups" not in r.state_dict() and r._items is None
    q.load_state_dict(sd0)
    assert q._grouped and q._grows[1] == [1.0, 0.0, 0.0, 0.0]


def test_groups_none_keeps_the_state_dict_keys_and_the_entry_points(monkeypatch):
    from chexpert_amd import ops
    from chexpert_amd.optim import FusedAdam, FusedRMSprop, FusedSGDNesterov
    net = Net([5, 8, 3])
    calls = []
    for name in dir(ops):
        if name.endswith(("_step", "_step_dev", "_step_ex", "_step_dev_ex", "_step_items")) or name in ("grad_norm", "grad_norm_items"):
            monkeypatch.setattr(ops, name, lambda *a, _n=name, **k: calls.append(_n))
    for cls, kind in ((FusedAdam, "adam"), (FusedSGDNesterov, "sgd_nesterov"), (FusedRMSprop, "rmsprop")):
        o = cls(net, lr=1e-3, weight_decay=0.1)
        assert set(o.state_dict()) == {"kind", "lr", "base_lr", "step_count", "sched_steps", "state"}
        assert not o._grouped and o.wd == 0.1
        del calls[:]
        o.step()
        assert calls == [kind + "_step"] and o._items is None and o._gtab is None
        e = cls(net, lr=1e-3, ema_decay=0.9, max_grad_norm=1.0)
        assert set(e.state_dict()) == {"kind", "lr", "base_lr", "step_count", "sched_steps", "state", "max_grad_norm", "skip_nonfinite",
                                       "ema_decay", "ema_warmup", "skipped", "ema"}
        del calls[:]
        e.step()
        assert calls == ["grad_norm", kind + "_step_ex"]
        for kw in ({"decoupled": True}, {"groups": []}, {"groups": [{"params": list(net.parameters())[:1]}], "skip_nonfinite": True}):
            g = cls(net, lr=1e-3, **kw)
            del calls[:]
            g.step()
            assert calls == (["grad_norm_items"] if "skip_nonfinite" in kw else []) + [kind + "_step_items"] and g.step_count == 1


def test_cli_flags_validation_and_defaults():
    from chexpert_amd import cli
    a = cli.build_parser().parse_args([])
    assert (a.batch_size, a.lr, a.n_epochs, a.log_interval, a.eval_interval, a.lr_decay_factor, a.model, a.fused_optimizer, a.graph) == \
        (16, 1e-4, 1, 50, 300, 0.97, "densenet121", False, False)
    assert (a.weight_decay, a.decoupled_decay, a.no_decay_norm_bias, a.head_lr_mult, a.backbone_lr_mult, a.freeze_backbone_steps) == \
        (None, False, False, None, None, 0)
    assert cli.group_options(a) == {} and cli.optimizer_options(a) == {}
    assert cli.fused_optimizer_kwargs(a, None) == {}                          # the constructors are called as before
    for argv in (["--weight_decay", "1e-4"], ["--decoupled_decay"], ["--no_decay_norm_bias"], ["--head_lr_mult", "10"],
                 ["--backbone_lr_mult", "0.1"], ["--freeze_backbone_steps", "100"], ["--freeze_backbone_steps", "-1"]):
        with pytest.raises(ValueError, match="--fused_optimizer"):
            cli.main(argv)                                                    # raised before anything touches data or the GPU
    for argv, word in ((["--weight_decay", "-1"], "--weight_decay"), (["--weight_decay", "nan"], "--weight_decay"),
                       (["--head_lr_mult", "-3"], "--head_lr_mult"), (["--head_lr_mult", "inf"], "--head_lr_mult"),
                       (["--backbone_lr_mult", "-0.5"], "--backbone_lr_mult"), (["--freeze_backbone_steps", "-2"], "--freeze_backbone_steps"),
                       (["--decoupled_decay"], "--weight_decay"), (["--no_decay_norm_bias", "--weight_decay", "0"], "--weight_decay")):
        with pytest.raises(ValueError, match=word):
            cli.main(["--fused_optimizer"] + argv)
    b = cli.build_parser().parse_args(["--fused_optimizer", "--weight_decay", "1e-4"])
    assert cli.group_options(b) == {"weight_decay": 1e-4, "decoupled": False, "finetune": None, "freeze_steps": 0}
    assert cli.fused_optimizer_kwargs(b, None) == {"weight_decay": 1e-4}      # a scalar decay alone: the plain kernels
    c = cli.build_parser().parse_args(["--fused_optimizer", "--weight_decay", "0.01", "--decoupled_decay", "--no_decay_norm_bias",
                                       "--head_lr_mult", "10", "--freeze_backbone_steps", "-1", "--clip_grad_norm", "2"])
    go = cli.group_options(c)
    assert go == {"weight_decay": 0.01, "decoupled": True, "freeze_steps": -1,
                  "finetune": {"weight_decay": 0.01, "no_decay_norm_bias": True, "head_lr_mult": 10.0, "backbone_lr_mult": 1.0,
                               "freeze_backbone": True}}
    from chexpert_amd.models import DenseNet
    from chexpert_amd.optim import FusedAdam
    m = DenseNet(32, (2, 2, 2, 2), 64, num_classes=5)
    kw = cli.fused_optimizer_kwargs(c, m)
    assert kw["weight_decay"] == 0.01 and kw["decoupled"] is True and kw["max_grad_norm"] == 2.0
    o = FusedAdam(m, lr=1e-3, **kw)
    assert [r[2] for r in o._grows] == [0.0, 1.0, 1.0, 0.0, 0.0] and [r[0] for r in o._grows] == [1.0, 1.0, 1.0, 10.0, 10.0]
    cli.thaw_backbone(o)
    assert [r[2] for r in o._grows] == [0.0] * 5


def test_new_entry_points_validate_before_launching():
    """Argument validation happens before any launch, so it can be exercised without a GPU."""
    import ctypes
    from chexpert_amd import _lib
    l = _lib.lib()
    buf = (ctypes.c_float * 64)()
    base = ctypes.addressof(buf)
    base += (-base) % 16
    tab = base + 64                                           # 16-byte aligned "tables" in the same host array (never read)
    EINVAL, EALIGN = -1, -2
    tail = (None, None, 0.0, 0, 0, None)                      # clip, ema, ema_decay, ema_warmup, skip_nonfinite, stream

    def adam(p=base, g=base, m=base, v=base, n=8, items=tab, ni=1, groups=tab, ng=1, hyper=None, step=1, tail=tail):
        return l.cx_adam_step_items(p, g, m, v, n, items, ni, groups, ng, 0, hyper, 1e-3, step, 0.9, 0.999, 1e-8, 1.0, *tail)

    def sgd(p=base, g=base, b=base, n=8, items=tab, ni=1, groups=tab, ng=1):
        return l.cx_sgd_nesterov_step_items(p, g, b, n, items, ni, groups, ng, 0, None, 1e-3, 1, 0.9, 1.0, *tail)

    def rms(p=base, g=base, s=base, b=base, n=8, items=tab, ni=1, groups=tab, ng=1, mom=0.9):
        return l.cx_rmsprop_step_items(p, g, s, b, n, items, ni, groups, ng, 0, None, 1e-3, 1, 0.99, 1e-3, mom, 1.0, *tail)

    def norm(g=base, n=8, items=tab, ni=1, groups=tab, ng=1, part=base, gsq=base, gnorm=base, clip=base):
        return l.cx_grad_norm_items(g, n, items, ni, groups, ng, 1.0, 0.0, 0, part, gsq, gnorm, clip, None)

    for fn in (adam, sgd, rms, norm):
        assert fn(items=None) == EINVAL and fn(groups=None) == EINVAL          # null tables
        assert fn(ng=0) == EINVAL and fn(ng=257) == EINVAL                     # G outside [1, 256]
        assert fn(ni=0) == EINVAL                                              # n > 0 with no item
        assert fn(n=6) == EINVAL                                               # not whole 16-byte units
        assert fn(g=None) == EINVAL
        assert fn(g=base + 4) == EALIGN and fn(items=tab + 4) == EALIGN and fn(groups=tab + 8) == EALIGN
    for fn in (adam, sgd, rms):
        assert fn(p=None) == EINVAL and fn(p=base + 4) == EALIGN
        assert fn(n=0, ni=0) == 0                                              # nothing to do: no launch
    assert adam(m=None) == EINVAL and adam(v=None) == EINVAL and adam(m=base + 4) == EALIGN and adam(v=base + 12) == EALIGN
    assert adam(step=0) == EINVAL                                              # host form: the step number is 1-based
    assert adam(tail=(None, base, 1.5, 0, 0, None)) == EINVAL                  # EMA decay > 1
    assert adam(tail=(None, base + 4, 0.5, 0, 0, None)) == EALIGN
    assert sgd(b=None) == EINVAL and sgd(b=base + 8) == EALIGN
    assert rms(s=None) == EINVAL and rms(b=None) == EINVAL and rms(b=None, mom=0.0, n=0, ni=0) == 0
    assert norm(clip=None) == EINVAL and norm(part=None) == EINVAL and norm(gsq=None) == EINVAL and norm(gnorm=None) == EINVAL


def test_header_declares_the_entry_points_and_the_makefile_lists_the_source():
    header = open(os.path.join(ROOT, "include", "chexpert_hip.h")).read()
    for name in ("cx_optim_item_vec4", "cx_grad_norm_items", "cx_adam_step_items", "cx_sgd_nesterov_step_items", "cx_rmsprop_step_items"):
        assert re.search(r"\bint %s\(" % name, header), name
    mk = open(os.path.join(ROOT, "chexpert_amd", "csrc", "Makefile")).read()
    srcs = re.search(r"^SRCS = (.*)$", mk, re.M).group(1).split()
    assert "optim.hip" in srcs and "elementwise.hip" in srcs
    assert os.path.exists(os.path.join(ROOT, "chexpert_amd", "csrc", "optim.hip"))


# ---------------------------------------------------------------------------------------- the float64 restatement against torch.optim
GROUP_HP = [(1.0, 0.0), (0.1, 1e-2), (3.0, 1e-3)]           # (lr_mult, weight_decay) of groups 0, 1, 2
LATE = 2                                                    # the group whose gradients are None for the first two steps


def torch_optimizer(kind, decoupled, params_by_group, lr):
    pg = [{"params": ps, "lr": lr * m, "weight_decay": wd} for ps, (m, wd) in zip(params_by_group, GROUP_HP)]
    if kind == "adam":
        return (torch.optim.AdamW if decoupled else torch.optim.Adam)(pg, lr=lr, betas=(0.9, 0.999), eps=1e-8)
    assert not decoupled
    if kind == "sgd_nesterov":
        return torch.optim.SGD(pg, lr=lr, momentum=0.9, nesterov=True)
    return torch.optim.RMSprop(pg, lr=lr, alpha=0.99, momentum=0.9, eps=1e-3)


@pytest.mark.parametrize("kind,decoupled", [("adam", False), ("adam", True), ("sgd_nesterov", False), ("rmsprop", False)])
def test_reference_step_agrees_with_torch_optim_param_groups(kind, decoupled):
    """Five steps in float64, three groups; group 2 has no gradient for the first two (torch then starts its step count, its
    momentum buffer and its moments at step 3: the t0 rule)."""
    from chexpert_amd.optim import reference_step
    torch.manual_seed(11)
    sizes, lr = [7, 33, 5, 64, 9, 12], 1e-2
    group_of = [k % 3 for k in range(len(sizes))]
    ps = [torch.nn.Parameter(torch.randn(n, dtype=torch.float64)) for n in sizes]
    opt = torch_optimizer(kind, decoupled, [[p for p, q in zip(ps, group_of) if q == j] for j in range(3)], lr)
    mine = [p.detach().clone() for p in ps]
    start = [p.detach().clone() for p in ps]
    st = [[torch.zeros(n, dtype=torch.float64), torch.zeros(n, dtype=torch.float64)] for n in sizes]
    for t in range(1, 6):
        gs = [torch.randn(n, dtype=torch.float64) for n in sizes]
        for k, p in enumerate(ps):
            p.grad = None if (group_of[k] == LATE and t <= 2) else gs[k].clone()
        opt.step()
        for k in range(len(sizes)):
            m, wd = GROUP_HP[group_of[k]]
            late = group_of[k] == LATE
            mine[k] = reference_step(kind, mine[k], gs[k], st[k], lr, t, lr_mult=m, weight_decay=wd, frozen=late and t <= 2,
                                     t0=2 if late else 0, decoupled=decoupled)
        if t == 2:                                          # no gradient so far: torch has not touched the late group, nor has the restatement
            for k in range(len(sizes)):
                assert (torch.equal(ps[k].detach(), start[k]) and torch.equal(mine[k], start[k])) == (group_of[k] == LATE)
    for k in range(len(sizes)):
        err = (mine[k] - ps[k].detach()).abs().max().item()
        assert err <= 1e-13 * (1.0 + ps[k].detach().abs().max().item()), (kind, decoupled, k, err)
    assert math.isfinite(sum(float(p.detach().sum()) for p in ps))


def test_reference_step_decoupled_order_and_frozen():
    """Decoupled decay of SGD / RMSprop (torch has none): p <- p (1 - lr_g wd) first, then the rule on the decayed p with no decay."""
    from chexpert_amd.optim import reference_step
    p, g = torch.tensor([2.0, -1.0], dtype=torch.float64), torch.tensor([0.5, 0.25], dtype=torch.float64)
    for kind in KINDS:
        st_a = [torch.zeros(2, dtype=torch.float64) for _ in range(2)]
        st_b = [torch.zeros(2, dtype=torch.float64) for _ in range(2)]
        a = reference_step(kind, p, g, st_a, 0.1, 1, lr_mult=2.0, weight_decay=0.5, decoupled=True)
        b = reference_step(kind, p * (1 - 0.2 * 0.5), g, st_b, 0.2, 1)
        assert torch.equal(a, b) and torch.equal(st_a[0], st_b[0])
        st_c = [torch.ones(2, dtype=torch.float64) for _ in range(2)]
        assert reference_step(kind, p, g, st_c, 0.1, 1, frozen=True) is p and torch.equal(st_c[0], torch.ones(2, dtype=torch.float64))
    with pytest.raises(ValueError):
        reference_step("lion", p, g, [], 0.1, 1)
