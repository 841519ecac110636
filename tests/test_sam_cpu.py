"""CPU (no GPU): host side of sharpness-aware minimisation (chexpert_amd.optim.FusedSAM, csrc/optim.hip: cx_sam_*_items): the float64
statement reference_sam_step, the argument checks of the three entry points before any launch, the wrapper's bookkeeping (tables,
delegation, state_dict) and the command line's refusals."""
import math
import os
import re

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def tensors(seed, sizes, lo=-1.0, hi=1.0):
    g = torch.Generator().manual_seed(seed)
    return [(torch.rand(n, generator=g, dtype=torch.float64) * (hi - lo) + lo) for n in sizes]


SIZES = [7, 33, 5, 64, 9, 12]
GROUP_OF = [k % 3 for k in range(len(SIZES))]
ROWS = [[1.0, 0.0, 0.0, 0.0], [0.1, 1e-2, 0.0, 0.0], [3.0, 1e-3, 0.0, 0.0]]


def rows(frozen=None):
    return [[r[0], r[1], 1.0 if j == frozen else 0.0, r[3]] for j, r in enumerate(ROWS)]


# ------------------------------------------------------------------------------------------------ the float64 statement
@pytest.mark.parametrize("adaptive", [False, True])
def test_rho_zero_is_the_identity(adaptive):
    from chexpert_amd.optim import reference_sam_step
    p, g = tensors(1, SIZES), tensors(2, SIZES)
    out, norm = reference_sam_step(p, g, rows(), GROUP_OF, 0.0, adaptive, 1e-12, 1.0)
    assert all(torch.equal(a, b) for a, b in zip(out, p)) and norm > 0


@pytest.mark.parametrize("grad_scale", [1.0, 1.0 / 128])
def test_sam_moves_the_unfrozen_weights_by_rho(grad_scale):
    """|perturbed - p| = rho * |g| / (|g| + eps) over the unfrozen tensors: rho, up to eps = 1e-12 of the norm -- whatever the
    gradient's scale."""
    from chexpert_amd.optim import reference_sam_step
    p, g = tensors(3, SIZES), tensors(4, SIZES)
    for frozen in (None, 1):
        out, norm = reference_sam_step(p, g, rows(frozen), GROUP_OF, 0.05, False, 1e-12, grad_scale)
        live = [k for k in range(len(SIZES)) if GROUP_OF[k] != frozen]
        moved = math.sqrt(sum(float((out[k] - p[k]).pow(2).sum()) for k in live))
        assert abs(moved - 0.05) <= 1e-10 * 0.05
        want = grad_scale * math.sqrt(sum(float(g[k].pow(2).sum()) for k in live))
        assert abs(norm - want) <= 1e-12 * want


def test_asam_is_invariant_under_rescaling_a_tensor():
    """Tensor 3 times c with its gradient over c (what a rescaling of a layer ahead of a ReLU or a BatchNorm does to the loss
    surface): the norm is unchanged, the perturbation of that tensor scales by c and every other tensor's stays.  SAM has no such
    invariance."""
    from chexpert_amd.optim import reference_sam_step
    p, g, c = tensors(5, SIZES), tensors(6, SIZES), 7.5
    p2 = [v * c if k == 3 else v for k, v in enumerate(p)]
    g2 = [v / c if k == 3 else v for k, v in enumerate(g)]
    a, na = reference_sam_step(p, g, rows(), GROUP_OF, 0.5, True, 1e-12, 1.0)
    b, nb = reference_sam_step(p2, g2, rows(), GROUP_OF, 0.5, True, 1e-12, 1.0)
    assert abs(na - nb) <= 1e-13 * na
    for k in range(len(SIZES)):
        ea, eb = a[k] - p[k], b[k] - p2[k]
        assert ea.abs().max() > 0
        assert (eb - (c if k == 3 else 1.0) * ea).abs().max() <= 1e-12 * eb.abs().max()
    s, ns = reference_sam_step(p, g, rows(), GROUP_OF, 0.5, False, 1e-12, 1.0)
    s2, ns2 = reference_sam_step(p2, g2, rows(), GROUP_OF, 0.5, False, 1e-12, 1.0)
    assert abs(ns - ns2) > 1e-3 * ns


@pytest.mark.parametrize("adaptive", [False, True])
def test_a_frozen_group_is_returned_untouched_and_is_absent_from_the_norm(adaptive):
    from chexpert_amd.optim import reference_sam_step
    p, g = tensors(7, SIZES), tensors(8, SIZES)
    out, norm = reference_sam_step(p, g, rows(frozen=1), GROUP_OF, 0.05, adaptive, 1e-12, 1.0)
    g_inf = [v.clone() for v in g]
    g_inf[1][2] = float("inf")                               # tensor 1 is in the frozen group: nothing reads it
    out2, norm2 = reference_sam_step(p, g_inf, [dict(lr_mult=r[0], weight_decay=r[1], frozen=bool(r[2])) for r in rows(frozen=1)],
                                     GROUP_OF, 0.05, adaptive, 1e-12, 1.0)
    assert norm2 == norm and math.isfinite(norm)
    for k in range(len(SIZES)):
        assert torch.equal(out[k], out2[k])
        if GROUP_OF[k] == 1:
            assert out[k] is p[k]
        else:
            assert not torch.equal(out[k], p[k])
    _, full = reference_sam_step(p, g, rows(), GROUP_OF, 0.05, adaptive, 1e-12, 1.0)
    assert norm < full


def test_a_zero_gradient_gives_a_zero_perturbation():
    from chexpert_amd.optim import reference_sam_step
    p = tensors(9, SIZES)
    out, norm = reference_sam_step(p, [torch.zeros_like(v) for v in p], rows(), GROUP_OF, 0.05, False, 1e-12, 1.0)
    assert norm == 0.0 and all(torch.equal(a, b) for a, b in zip(out, p))


# ------------------------------------------------------------------------------------------------ the entry points
def test_entry_points_validate_before_launching():
    """Argument validation happens before any launch, so it can be exercised without a GPU.  The tables of the kernels live in device
    memory; a host copy of the item table (`items_host`), when given, is checked against the buffer and the group count."""
    import ctypes
    from chexpert_amd import _lib
    l = _lib.lib()
    buf = (ctypes.c_float * 64)()
    base = ctypes.addressof(buf)
    base += (-base) % 16
    tab = base + 64                                           # 16-byte aligned "tables" in the same host array (never read)
    EINVAL, EALIGN = -1, -2
    host = (ctypes.c_uint32 * 8)(0, 1, 0, 0, 1, 1, 1, 1)      # two items of one unit each: units [0, 2), groups 0 and 1
    hp = ctypes.addressof(host)

    def norm(p=base, g=base, n=8, items=tab, ih=None, ni=2, groups=tab, ng=2, hyp=base, adaptive=1, part=base, sam=base):
        return l.cx_sam_norm_items(p, g, n, items, ih, ni, groups, ng, hyp, 1.0, adaptive, part, sam, None)

    def perturb(p=base, g=base, b=base, n=8, items=tab, ih=None, ni=2, groups=tab, ng=2, sam=base, adaptive=0):
        return l.cx_sam_perturb_items(p, g, b, n, items, ih, ni, groups, ng, sam, 1.0, adaptive, None)

    def restore(p=base, b=base, n=8, items=tab, ih=None, ni=2, groups=tab, ng=2, sam=base):
        return l.cx_sam_restore_items(p, b, n, items, ih, ni, groups, ng, sam, None)

    for fn in (norm, perturb, restore):
        assert fn(items=None) == EINVAL and fn(groups=None) == EINVAL          # null tables
        assert fn(sam=None) == EINVAL
        assert fn(ng=0) == EINVAL and fn(ng=257) == EINVAL                     # G outside [1, 256]
        assert fn(ni=0) == EINVAL                                              # n > 0 with no item
        assert fn(n=6) == EINVAL                                               # not whole 16-byte units
        assert fn(n=4, ih=hp) == EINVAL                                        # the second item ends past the buffer
        assert fn(ng=1, ih=hp) == EINVAL                                       # ... or names group 1 of one
        assert fn(items=tab + 4) == EALIGN and fn(groups=tab + 8) == EALIGN
        assert fn(p=base + 4) == EALIGN
    for fn in (perturb, restore):
        assert fn(p=None) == EINVAL and fn(b=None) == EINVAL and fn(b=base + 8) == EALIGN
        assert fn(n=0, ni=0) == 0                                              # nothing to do: no launch
    assert perturb(g=None) == EINVAL and perturb(g=base + 4) == EALIGN
    assert norm(g=None) == EINVAL and norm(part=None) == EINVAL and norm(hyp=None) == EINVAL
    assert norm(p=None) == EINVAL                                              # ASAM reads the weights ...
    assert norm(g=base + 4, adaptive=0) == EALIGN


def test_header_declares_the_entry_points_and_lib_lists_them():
    from chexpert_amd import _lib, ops
    header = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "chexpert_hip.h")).read(), flags=re.S)
    for name in ("cx_sam_norm_items", "cx_sam_perturb_items", "cx_sam_restore_items"):
        m = re.search(r"\bint %s\(([^;]*)\);" % name, header)
        assert m, name
        assert name in _lib.SIGNATURES and len(_lib.SIGNATURES[name]) == m.group(1).count(",") + 1
        assert hasattr(_lib.lib(), name)
        assert callable(getattr(ops, name[3:]))
    mk = open(os.path.join(ROOT, "chexpert_amd", "csrc", "Makefile")).read()
    assert "optim.hip" in re.search(r"^SRCS = (.*)$", mk, re.M).group(1).split()
    assert _lib.lib().cx_abi_version() == 10                                   # additive entry points


# ------------------------------------------------------------------------------------------------ the wrapper
class _Eng:
    packed_version = 0
    reducer = None


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


def test_constructor_validation_and_delegation():
    from chexpert_amd.optim import FusedAdam, FusedSAM
    net = Net([5, 8, 3])
    base = FusedAdam(net, lr=1e-3, max_grad_norm=2.0)
    with pytest.raises(TypeError, match="fused optimiser"):
        FusedSAM(torch.optim.SGD(net.parameters(), lr=0.1))
    with pytest.raises(TypeError):
        FusedSAM(FusedSAM(base))
    for bad in (-0.1, float("nan"), float("inf")):
        with pytest.raises(ValueError, match="rho"):
            FusedSAM(base, rho=bad)
    for bad in (0.0, -1e-12, float("nan")):
        with pytest.raises(ValueError, match="eps"):
            FusedSAM(base, eps=bad)
    s = FusedSAM(base)
    assert (s.rho, s.adaptive, s.eps) == (0.05, False, 1e-12)
    assert s.lr == 1e-3 and s.betas == (0.9, 0.999) and s.max_grad_norm == 2.0 and s.model is net      # read through
    s.lr = 0.5                                                                  # written through
    assert base.lr == 0.5 and "lr" not in vars(s)
    assert s.hyper.__self__ is base and s.tick.__self__ is base and s.grad_norm.__self__ is base
    with pytest.raises(AttributeError):
        s.no_such_attribute
    with pytest.raises(RuntimeError, match="train_step"):
        s.step()
    with pytest.raises(RuntimeError, match="train_step"):
        s.step_dev()
    with pytest.raises(ValueError, match="rho"):
        s.set_rho(-1.0)
    s.set_rho(0.0)
    assert s.rho == 0.0


def test_tables_an_ungrouped_base_gets_group_zero_and_a_grouped_one_shares_its_own():
    from chexpert_amd import optim as O
    net = Net([5, 8, 3, 40])
    s = O.FusedSAM(O.FusedSGDNesterov(net, lr=0.1), rho=0.1)
    s._bufs()
    items = O.item_table([5, 8, 3, 40], [0, 0, 0, 0])
    assert s._sitems.tolist() == [list(it) for it in items] and s._sitems_host.tolist() == s._sitems.tolist()
    assert s._sgtab.tolist() == [[1.0, 0.0, 0.0, 0.0]] and s._tables()[0] is s._sitems
    assert s._backup.shape == net.eng.flat.shape and s._spart.numel() == len(items) and s._sam.numel() == 4
    assert s._rho_dev.tolist() == [pytest.approx(0.1), pytest.approx(1e-12)]
    assert s.base._items is None                                                 # the base stays on its plain kernels
    s.set_rho(0.25)
    assert s._rho_dev.tolist()[0] == 0.25
    a, b, c, d = list(net.parameters())
    g = O.FusedSAM(O.FusedLAMB(net, lr=1e-3, groups=[{"params": [a, c], "frozen": True}]))
    g._bufs()
    it, gt = g._tables()
    assert it is g.base._items and gt is g.base._gtab and g._sitems is None
    assert g._sitems_host.tolist() == g.base._items.tolist() and [r[2] for r in g._sitems_host.tolist()] == [1, 0, 1, 0]
    g.set_group(1, frozen=False)                                                 # the base's: the shared table follows
    assert gt[1].tolist()[2] == 0.0


def test_state_dict_carries_the_base_state_and_the_sam_entry_both_ways():
    from chexpert_amd.optim import FusedAdam, FusedSAM
    net = Net([5, 8, 3])
    plain = FusedAdam(net, lr=1e-3)
    plain._state = [torch.zeros(16), torch.ones(16)]
    plain.step_count = 7
    s = FusedSAM(plain, rho=0.2, adaptive=True, eps=1e-10)
    sd = s.state_dict()
    assert sd["sam"] == {"rho": 0.2, "adaptive": True, "eps": 1e-10}
    assert {k: v for k, v in sd.items() if k not in ("sam", "state")} == {k: v for k, v in plain.state_dict().items() if k != "state"}
    # a SAM checkpoint into a run without SAM: the base reads its own keys
    bare = FusedAdam(net, lr=1.0)
    bare.load_state_dict(sd)
    assert bare.step_count == 7 and bare.lr == 1e-3
    # ... into another SAM run: the entry comes along; a checkpoint without the entry leaves SAM as constructed
    other = FusedSAM(FusedAdam(net, lr=1.0), rho=0.05)
    other.load_state_dict(sd)
    assert (other.rho, other.adaptive, other.eps, other.step_count) == (0.2, True, 1e-10, 7)
    kept = FusedSAM(FusedAdam(net, lr=1.0), rho=0.3)
    kept.load_state_dict(plain.state_dict())
    assert (kept.rho, kept.adaptive, kept.step_count) == (0.3, False, 7)


def test_refusals_that_need_no_gpu():
    from chexpert_amd.optim import FusedAdam, FusedSAM
    net = Net([5, 8, 3])
    s = FusedSAM(FusedAdam(net, lr=1e-3))
    net.loss_kind = "aucm"
    with pytest.raises(RuntimeError, match="aucm"):
        s.first_step()
    with pytest.raises(RuntimeError, match="aucm"):
        s.train_step(net, None, None)
    net.loss_kind = "bce"
    net.eng.reducer = object()
    with pytest.raises(RuntimeError, match="data-parallel"):
        s.train_step(net, None, None)
    net.eng.reducer = None
    with pytest.raises(RuntimeError, match="not the one"):
        s.train_step(Net([4]), None, None)
    net.eval()
    with pytest.raises(RuntimeError, match="training mode"):
        s.train_step(net, None, None)


def test_track_stats_is_an_engine_switch_that_forward_backward_resets():
    """The second pass's switch: off only for the span of one forward, whatever happens inside it."""
    from chexpert_amd.models import DenseNet
    import inspect
    m = DenseNet(32, (2, 2, 2, 2), 64, num_classes=5)
    eng = m._eng()
    assert eng.track_stats is True
    assert inspect.signature(m.forward_backward).parameters["track_stats"].default is True
    bn = torch.nn.BatchNorm2d(4)
    assert eng._bn_train(bn)[4] is bn.running_mean and eng._bn_train(bn)[5] is bn.running_var
    eng.track_stats = False
    assert eng._bn_train(bn)[4:] == (None, None) and eng._bn_train(bn)[:4] == (bn.weight, bn.bias, bn.eps, 0.1)
    eng.track_stats = True
    seen = []

    def forward(x, train, record=False):
        seen.append(eng.track_stats)
        raise RuntimeError("stop here")
    eng.forward = forward
    for want in (False, True):
        with pytest.raises(RuntimeError, match="stop here"):                   # the forward raises ...
            m.forward_backward(torch.zeros(2, 3, 64, 64), torch.zeros(2, 5), track_stats=want)
        assert eng.track_stats is True                                         # ... and the switch is back
    assert seen == [False, True]


# ------------------------------------------------------------------------------------------------ the command line
def test_cli_flags_validation_and_defaults():
    from chexpert_amd import cli
    a = cli.build_parser().parse_args([])
    assert (a.sam_rho, a.sam_adaptive) == (None, False) and cli.sam_options(a) == {}
    with pytest.raises(ValueError, match="--fused_optimizer"):
        cli.main(["--sam_rho", "0.05"])                                        # raised before anything touches data or the GPU
    with pytest.raises(ValueError, match="aucm"):
        cli.main(["--fused_optimizer", "--sam_rho", "0.05", "--loss", "aucm"])
    for bad in ("0", "-0.1", "nan", "inf"):
        with pytest.raises(ValueError, match="--sam_rho"):
            cli.main(["--fused_optimizer", "--sam_rho", bad])
    with pytest.raises(ValueError, match="--sam_rho"):
        cli.main(["--fused_optimizer", "--sam_adaptive"])
    b = cli.build_parser().parse_args(["--fused_optimizer", "--sam_rho", "0.1", "--sam_adaptive"])
    assert cli.sam_options(b) == {"rho": 0.1, "adaptive": True}
    with pytest.raises(ValueError, match="more than one rank"):
        cli.sam_options(b, world=2)
    c = cli.build_parser().parse_args(["--fused_optimizer", "--sam_rho", "0.1", "--optimizer", "lamb", "--loss", "focal"])
    assert cli.sam_options(c) == {"rho": 0.1, "adaptive": False}
