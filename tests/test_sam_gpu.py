"""GPU: sharpness-aware minimisation (csrc/optim.hip: cx_sam_norm_items, cx_sam_perturb_items, cx_sam_restore_items;
chexpert_amd.optim.FusedSAM).  The kernels on the synthetic ten-tensor layout of tests/test_optim_trust_gpu.py (about 24 V floats,
V = cx_optim_item_vec4()): against the float64 statement optim.reference_sam_step with a bound derived from the summation shape, and
bit for bit where the feature promises bits.  The orchestration (train_step, the captured step, the options of the base optimiser)
on the smallest model of each family, held to equal bits: the engines are reproducible run to run."""
import math

import pytest
import torch

from chexpert_amd import synth

pytestmark = pytest.mark.gpu

U = 2.0 ** -24                     # unit round-off of fp32
EPS = 1e-12
RHO = {False: 0.5, True: 2.0}      # large enough for the one-float tensor to move visibly (ASAM's radius is usually ~10x SAM's)
SENTINEL = 7.0


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    from chexpert_amd import _lib
    _lib.lib()          # fail loudly if the HIP library is missing
    return torch.device("cuda:0")


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
    reducer = None


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


def round_robin(sizes, n):
    return [k % n for k in range(len(sizes))]


def make_sam(net, n_groups, adaptive, frozen=None, rho=None):
    """FusedSAM over a grouped FusedSGDNesterov (n_groups >= 2: dict j is group j + 1, round-robin) or an ungrouped one (n_groups = 0:
    FusedSAM's own table); the backup is pre-filled with a sentinel."""
    from chexpert_amd import optim as O
    ps = list(net.parameters())
    group_of = round_robin(net.sizes, max(1, n_groups))
    if n_groups == 0:
        base = O.FusedSGDNesterov(net, lr=1e-2)
    else:
        base = O.FusedSGDNesterov(net, lr=1e-2, groups=[{"params": [p for p, q in zip(ps, group_of) if q == j], "frozen": j == frozen}
                                                         for j in range(1, n_groups)])
    s = O.FusedSAM(base, rho=RHO[adaptive] if rho is None else rho, adaptive=adaptive, eps=EPS)
    s._bufs()
    s._backup.fill_(SENTINEL)
    return s, group_of


def restore(net, s):
    from chexpert_amd import ops
    items, gtab = s._tables()
    ops.sam_restore_items(net.eng.flat, s._backup, items, gtab, s._sam, s._sitems_host)


def norm_bound(items, live, adaptive):
    """First-order relative bound of the norm from the summation shape, the way ratio_bounds of tests/test_optim_trust_gpu.py derives
    LAMB's.  A sum of non-negative terms carries at most (roundings on the longest path of a term to the result) * 2^-24 of relative
    error.  A term: grad_scale = 1 multiplies exactly; ASAM's g * |p| rounds once, which the square doubles.  Launch 1, per item:
    ceil(len4 / 256) fused multiply-adds into one of a thread's four accumulators (each squares and adds with one rounding), two
    additions that join the four, 6 shuffle levels in the wave and 3 additions over the 4 waves.  Launch 2: ceil(n_items / 256)
    additions per thread (frozen items add +0, exactly), then the same 9 levels.  The square root halves the relative error of the sum
    and adds its own (HIP documents sqrtf at 1 ulp = 2 U).  Second-order terms: 0.1 %."""
    mine = [it for it in items if it[3] in live]
    path = max(ceil_div(it[1], 256) for it in mine) + 2 + 9 + ceil_div(len(items), 256) + 9 + (2 if adaptive else 0)
    return 1.001 * (0.5 * path * U + 2 * U)


def move_bound(b_norm, adaptive):
    """Relative bound of one element's perturbation e = scale * s^2 * g: the norm's, the three roundings of scale = rho / (norm + eps)
    (fp32 rho, the sum, the quotient), the product scale * e and, ASAM, p * p and its product with g.  The sum p + e then rounds once
    more: at most 1 ulp of the result whether or not the compiler fuses it -- the comparison allows 2."""
    return 1.001 * (b_norm + (3 + 1 + (2 if adaptive else 0)) * U)


# ------------------------------------------------------------------------------------------------ 1. against the float64 statement
@pytest.mark.parametrize("frozen", [None, 1])
@pytest.mark.parametrize("adaptive", [False, True])
def test_norm_and_perturbation_match_the_float64_statement(dev, adaptive, frozen):
    from chexpert_amd import optim as O
    sizes = synthetic_sizes()
    net = Net(sizes, dev)
    s, group_of = make_sam(net, 3, adaptive, frozen)
    g = values(20, sizes)
    net.set_grad(g)
    p0 = values(7, sizes)
    s.first_step()
    rows = [[1.0, 0.0, float(j == frozen), 0.0] for j in range(3)]
    want, want_norm = O.reference_sam_step(p0, g, rows, group_of, RHO[adaptive], adaptive, EPS, 1.0)
    live = {k for k in range(len(sizes)) if group_of[k] != frozen}
    items = O.item_table(sizes, group_of)
    b_norm = norm_bound(items, live, adaptive)
    got = s._sam.cpu().double()
    err = abs(float(got[0]) - want_norm) / want_norm
    print("norm %.9g (float64 %.9g): rel err %.3e, bound %.3e; nonfinite %g" % (got[0], want_norm, err, b_norm, got[2]))
    assert err <= b_norm and float(got[2]) == 0.0 and float(got[3]) == 0.0
    assert s.perturbation_norm() == float(got[0])
    want_scale = RHO[adaptive] / (want_norm + EPS)
    assert abs(float(got[1]) - want_scale) <= 1.001 * (b_norm + 3 * U) * want_scale
    # the perturbed weights
    after = net.tensors(net.eng.flat)
    maxw = max(float(v.abs().max()) for v in p0)
    b_move = move_bound(b_norm, adaptive)
    for k in range(len(sizes)):
        if k not in live:
            assert torch.equal(after[k], p0[k])
            continue
        e = (want[k] - p0[k].double()).abs().max().item()
        allowed = b_move * e + 2 * 2.0 ** -23 * maxw
        err = (after[k].double() - want[k]).abs().max().item()
        moved = (after[k].double() - p0[k].double()).abs().max().item()
        print("tensor %d (%d floats): max err %.3e, allowed %.3e (bound %.3e x largest step %.3e + 2 ulp of %.4f); moved %.3e"
              % (k, sizes[k], err, allowed, b_move, e, maxw, moved))
        assert err <= allowed
        assert moved > 100 * allowed                                   # the test cannot pass on a no-op
    assert b_move * RHO[adaptive] * max(1.0, maxw) >= max(b_move * (want[k] - p0[k].double()).abs().max().item() for k in live)


# ------------------------------------------------------------------------------------------------ 2. bits
@pytest.mark.parametrize("adaptive", [False, True])
def test_backup_frozen_items_padding_restore_and_reproducibility(dev, adaptive):
    sizes = synthetic_sizes()
    runs = []
    for rep in range(2):
        net = Net(sizes, dev)
        s, group_of = make_sam(net, 3, adaptive, frozen=1)
        net.set_grad(values(21, sizes))
        before = net.eng.flat.clone()
        s.first_step()
        frozen = net.mask(group_of, 1)
        assert net.eng.packed_version is None
        assert torch.equal(s._backup[~frozen], before[~frozen])                        # the weights before, padding included
        assert (s._backup[frozen] == SENTINEL).all()                                   # no byte of a frozen item's backup ...
        assert torch.equal(net.eng.flat[frozen], before[frozen])                       # ... or of its weights written
        assert not net.eng.flat[net.pad].any() and not s._backup[net.pad & ~frozen].any()
        for k, (a, b) in enumerate(zip(net.tensors(net.eng.flat), net.tensors(before))):
            assert torch.equal(a, b) == (group_of[k] == 1), k
        runs.append((net.eng.flat.clone(), s._sam.clone(), s._spart.clone()))
        restore(net, s)
        assert torch.equal(net.eng.flat, before)                                       # a copy: the weights' own bits
        assert (s._backup[frozen] == SENTINEL).all()
    assert all(torch.equal(a, b) for a, b in zip(*runs))


@pytest.mark.parametrize("adaptive", [False, True])
def test_the_cut_into_groups_is_only_a_label(dev, adaptive):
    """The same tensors in FusedSAM's own one-group table, in one group of a grouped base and in three: the item order is the same,
    so the sum is, and every perturbed bit."""
    sizes = synthetic_sizes()
    out = []
    for n_groups in (0, 1, 3):
        net = Net(sizes, dev)
        s, _ = make_sam(net, n_groups, adaptive)
        net.set_grad(values(22, sizes))
        s.first_step()
        out.append((net.eng.flat.clone(), s._sam.clone(), s._backup.clone()))
    for other in out[1:]:
        assert all(torch.equal(a, b) for a, b in zip(out[0], other))
    assert not torch.equal(out[0][0], out[0][2])


# ------------------------------------------------------------------------------------------------ 3. edge values
@pytest.mark.parametrize("adaptive", [False, True])
def test_zero_gradient_leaves_every_bit_and_nothing_is_nan(dev, adaptive):
    sizes = synthetic_sizes()
    net = Net(sizes, dev)
    s, _ = make_sam(net, 3, adaptive)
    before = net.eng.flat.clone()
    s.first_step()                                                                     # flat_grad is all zeros
    sam = s._sam.cpu()
    assert sam[0] == 0.0 and sam[2] == 0.0 and torch.isfinite(sam).all() and sam[1] > 0
    assert torch.equal(net.eng.flat, before) and torch.equal(s._backup, before)


@pytest.mark.parametrize("adaptive", [False, True])
def test_inf_in_a_live_tensor_stops_everything_in_a_frozen_one_is_ignored(dev, adaptive):
    sizes = synthetic_sizes()
    net = Net(sizes, dev)
    s, group_of = make_sam(net, 3, adaptive, frozen=1)
    assert group_of[7] == 1 and group_of[6] == 0
    frozen = net.mask(group_of, 1)
    before = net.eng.flat.clone()
    g = [v.clone() for v in values(23, sizes)]
    g[6][100] = float("inf")                                                           # tensor 6 is live
    net.set_grad(g)
    s.first_step()
    assert float(s._sam.cpu()[2]) == 1.0
    assert torch.equal(net.eng.flat, before) and (s._backup == SENTINEL).all()         # perturb wrote nothing ...
    restore(net, s)
    assert torch.equal(net.eng.flat, before)                                           # ... and restore did not copy the sentinel
    g = [v.clone() for v in values(23, sizes)]
    g[7][100] = float("inf")                                                           # the same inf in the frozen group
    net.set_grad(g)
    s.first_step()
    sam = s._sam.cpu()
    assert sam[2] == 0.0 and torch.isfinite(sam).all() and sam[0] > 0
    assert torch.equal(net.eng.flat[frozen], before[frozen]) and torch.isfinite(net.eng.flat).all()
    for k, (a, b) in enumerate(zip(net.tensors(net.eng.flat), net.tensors(before))):
        assert torch.equal(a, b) == (group_of[k] == 1), k


def test_asam_does_not_move_a_tensor_of_zeros(dev):
    sizes = synthetic_sizes()
    net = Net(sizes, dev)
    off = net.eng.offsets
    net.eng.flat.data[off[5]:off[5] + sizes[5]] = 0.0
    s, _ = make_sam(net, 3, True)
    net.set_grad(values(24, sizes))
    before = net.eng.flat.clone()
    s.first_step()
    for k, (a, b) in enumerate(zip(net.tensors(net.eng.flat), net.tensors(before))):
        assert torch.equal(a, b) == (k == 5), k
    assert torch.isfinite(net.eng.flat).all()


# ------------------------------------------------------------------------------------------------ 4. rho in device memory
@pytest.mark.parametrize("adaptive", [False, True])
def test_set_rho_between_two_calls_scales_the_second(dev, adaptive):
    """rho doubled on the device: scale doubles exactly (a power of two), and so does every element's step up to the rounding of the
    two sums p + e (1 ulp of the result each at most)."""
    sizes = synthetic_sizes()
    net = Net(sizes, dev)
    s, _ = make_sam(net, 3, adaptive, rho=0.25)
    net.set_grad(values(25, sizes))
    before = net.eng.flat.clone()
    s.first_step()
    scale1, p1 = float(s._sam.cpu()[1]), net.eng.flat.clone()
    restore(net, s)
    s.set_rho(0.5)
    s.first_step()
    scale2, p2 = float(s._sam.cpu()[1]), net.eng.flat.clone()
    assert scale2 == 2.0 * scale1 and scale1 > 0
    e1, e2 = (p1.double() - before.double()), (p2.double() - before.double())
    ulp = 2.0 ** -23 * float(p2.abs().max())
    print("largest step %.3e -> %.3e; largest departure from twice the first %.3e (3 ulp = %.3e)"
          % (e1.abs().max(), e2.abs().max(), (e2 - 2 * e1).abs().max(), 3 * ulp))
    assert (e2 - 2 * e1).abs().max().item() <= 3 * ulp and e1.abs().max().item() > 100 * ulp


# ================================================================================================ orchestration
B, N_CLS = 4, 5
SIZE = {"densenet": 64, "resnet": 64, "efficientnet": 64}
FAMILIES = ["densenet", "resnet", "efficientnet"]


def build(family, dev, dtype=torch.float32):
    """The smallest model each family's own GPU tests use, identically initialised on every call."""
    from chexpert_amd import models
    torch.manual_seed(5)
    if family == "densenet":
        m = models.DenseNet(32, (2, 2, 2, 2), 64, num_classes=N_CLS)
    elif family == "resnet":
        m = models.ResNet(models.Bottleneck, [1, 1, 1, 1], num_classes=N_CLS)
    else:
        m = models.construct_model("efficientnet-b0", N_CLS)
    return m.to(dev).storage_dtype(dtype).train()


def base_of(family, m, **kw):
    """One base optimiser per family, so the three kernel families of the plain steps all pass under FusedSAM: Adam with an EMA
    (`_ex`), SGD (plain), RMSprop with parameter groups (`_items`)."""
    from chexpert_amd import optim as O
    if family == "densenet":
        return O.FusedAdam(m, lr=1e-3, ema_decay=0.9, **kw)
    if family == "resnet":
        return O.FusedSGDNesterov(m, lr=1e-2, **kw)
    return O.FusedRMSprop(m, lr=1e-4, groups=O.finetune_groups(m, weight_decay=1e-4, head_lr_mult=10.0), **kw)


def batch(family, dev, i=0):
    return synth.xray_batch(300 + i, B, SIZE[family]).to(dev), synth.targets(400 + i, B, N_CLS).to(dev)


def snapshot(m, opt):
    eng = m._eng()
    out = {"flat": eng.flat.clone(), "state": [t.clone() for t in opt._state], "ema": None if opt._ema is None else opt._ema.clone()}
    out["sd"] = {k: v.clone() for k, v in m.state_dict().items() if "running_" in k or "num_batches" in k}
    return out


_RUNS = {}


def runs(family, dev):
    """Computed once per family and shared: A the SAM step, C the perturbed weights after first_step, B the same step by hand from
    pieces that existed before FusedSAM, P the base optimiser's plain step, Z the SAM step with rho = 0."""
    if family in _RUNS:
        return _RUNS[family]
    from chexpert_amd.optim import FusedSAM
    x, t = batch(family, dev)
    r = {}
    # C
    m = build(family, dev)
    s = FusedSAM(base_of(family, m), rho=0.05)
    s.zero_grad()
    m.forward_backward(x, t)
    r["start"] = None
    s.first_step()
    perturbed = m._eng().flat.clone()
    r["C_backup"] = s._backup.clone()
    # A
    m = build(family, dev)
    s = FusedSAM(base_of(family, m), rho=0.05)
    r["start"] = {k: v.clone() for k, v in m.state_dict().items()}
    loss, logits = s.train_step(m, x, t)
    r["A"] = dict(snapshot(m, s), loss=loss.clone(), logits=logits.clone(), norm=s.perturbation_norm(), step_count=s.step_count)
    # B
    m = build(family, dev)
    opt = base_of(family, m)
    eng = m._eng()
    opt.zero_grad()
    m.forward_backward(x, t)
    original = eng.flat.clone()
    eng.flat.copy_(perturbed)
    eng.packed_version = None
    opt.zero_grad()
    m.forward_backward(x, t)
    eng.flat.copy_(original)
    eng.packed_version = None
    opt.step()
    r["B"] = snapshot(m, opt)
    r["original"], r["perturbed"] = original, perturbed
    # P
    m = build(family, dev)
    opt = base_of(family, m)
    opt.zero_grad()
    loss, logits = m.forward_backward(x, t)
    opt.step()
    r["P"] = dict(snapshot(m, opt), loss=loss.clone(), logits=logits.clone())
    # Z
    m = build(family, dev)
    s = FusedSAM(base_of(family, m), rho=0.05)
    s.set_rho(0.0)
    s.train_step(m, x, t)
    r["Z"] = snapshot(m, s)
    # P2 (EfficientNet): the plain step on the gradient of the SECOND forward of the batch.  Dropout and DropConnect draw their masks
    # from a device counter that advances per forward, so the gradient FusedSAM applies was taken under the second draw
    r["P2"] = None
    if family == "efficientnet":
        m = build(family, dev)
        opt = base_of(family, m)
        for _ in range(2):
            opt.zero_grad()
            m.forward_backward(x, t)
        opt.step()
        r["P2"] = snapshot(m, opt)
    torch.cuda.synchronize()
    _RUNS[family] = r
    return r


def same(a, b):
    return torch.equal(a["flat"], b["flat"]) and all(torch.equal(u, v) for u, v in zip(a["state"], b["state"])) and \
        ((a["ema"] is None and b["ema"] is None) or torch.equal(a["ema"], b["ema"]))


@pytest.mark.parametrize("family", FAMILIES)
def test_train_step_is_the_composition_of_its_pieces(dev, family):
    """5 (and the EMA half of 9).  A = FusedSAM.train_step; B = forward_backward, the perturbed weights of a third run copied in,
    zero_grad, forward_backward, the original weights copied back, the base optimiser's step.  Parameters, optimiser states and (DenseNet:
    the base keeps one) the EMA are bit-equal; the second pass really saw other weights."""
    r = runs(family, dev)
    assert torch.equal(r["C_backup"], r["original"]) and not torch.equal(r["perturbed"], r["original"])
    moved = (r["perturbed"] - r["original"]).double().norm().item()
    print("%s: |perturbed - p| = %.6g (rho 0.05), norm %.6g" % (family, moved, r["A"]["norm"]))
    assert abs(moved - 0.05) <= 1e-4 * 0.05                   # (fp32 sums of ~1e6 elements; test 1 holds the kernels to their bound)
    assert same(r["A"], r["B"])
    assert not torch.equal(r["A"]["flat"], r["original"]) and torch.isfinite(r["A"]["flat"]).all()
    assert not same(r["A"], r["P"])                           # and SAM is not the plain step
    assert r["A"]["step_count"] == 1
    if family == "densenet":
        assert r["A"]["ema"] is not None and not torch.equal(r["A"]["ema"], r["original"])


@pytest.mark.parametrize("family", FAMILIES)
def test_second_pass_leaves_batchnorm_statistics_and_counts_alone(dev, family):
    """6.  After train_step every running_mean, running_var and num_batches_tracked equals that of ONE plain forward_backward on the
    same batch from the same start, and so do the returned loss and logits."""
    r = runs(family, dev)
    a, p = r["A"], r["P"]
    assert a["sd"].keys() == p["sd"].keys() and len(a["sd"]) >= 3
    assert all(torch.equal(a["sd"][k], p["sd"][k]) for k in a["sd"])
    changed = [k for k in a["sd"] if not torch.equal(a["sd"][k], r["start"][k].to(a["sd"][k].device))]
    assert len(changed) == len(a["sd"])                        # every statistic moved once, every count is 1
    assert all(int(v) == 1 for k, v in a["sd"].items() if "num_batches" in k)
    assert torch.equal(a["loss"], p["loss"]) and torch.equal(a["logits"], p["logits"])
    # the by-hand composition ran two tracked forwards: its statistics differ, which is what the switch is for
    assert any(not torch.equal(r["B"]["sd"][k], a["sd"][k]) for k in a["sd"])


@pytest.mark.parametrize("family", FAMILIES)
def test_rho_zero_is_the_plain_step(dev, family):
    """7.  With rho = 0 the SAM step leaves parameters and states bit-equal to the base optimiser's plain step on the same batch.
    EfficientNet's Dropout and DropConnect draw fresh masks in the second pass (their device counter advances per forward), so there
    the plain step to compare with is the one on the batch's second forward; against the first draw's the weights differ."""
    r = runs(family, dev)
    if family == "efficientnet":
        assert same(r["Z"], r["P2"]) and not torch.equal(r["Z"]["flat"], r["P"]["flat"])
    else:
        assert same(r["Z"], r["P"])
    assert all(torch.equal(r["Z"]["sd"][k], r["P"]["sd"][k]) for k in r["P"]["sd"])


def test_captured_step_equals_eager_bits_and_the_plain_graph_is_unchanged(dev):
    """8.  Three replays of GraphedTrainStep over FusedSAM(FusedAdam), rho changed before the third, against three eager
    train_step(dev=True) calls on a twin; constructing the graphed step leaves buffers and parameters as they were; a graph over
    the bare FusedAdam still equals its eager step."""
    from chexpert_amd.graph import GraphedTrainStep
    from chexpert_amd.optim import FusedAdam, FusedSAM
    data = [batch("densenet", dev, i) for i in range(3)]

    def fresh(sam):
        m = build("densenet", dev)
        opt = FusedAdam(m, lr=1e-3)
        return m, (FusedSAM(opt, rho=0.05) if sam else opt)

    for sam in (True, False):
        m_e, o_e = fresh(sam)
        for i, (x, t) in enumerate(data):
            if sam and i == 2:
                o_e.set_rho(0.2)
            if sam:
                o_e.train_step(m_e, x, t, dev=True)
            else:
                m_e.zero_grad()
                m_e.forward_backward(x, t)
                o_e.step_dev()
                o_e.tick()
        m_g, o_g = fresh(sam)
        held = [b.detach().clone() for b in m_g.buffers()]
        params = [p.detach().clone() for p in m_g.parameters()]
        gs = GraphedTrainStep(m_g, o_g, *data[0])
        torch.cuda.synchronize()
        assert all(torch.equal(a, b) for a, b in zip(held, m_g.buffers())) and m_g._nbt_pending == 0
        assert all(torch.equal(a, b) for a, b in zip(params, m_g.parameters()))
        for i, (x, t) in enumerate(data):
            if sam and i == 2:
                o_g.set_rho(0.2)
            gs.replay(x, t)
        torch.cuda.synchronize()
        assert torch.equal(m_e._eng().flat, m_g._eng().flat), sam
        assert all(torch.equal(a, b) for a, b in zip(o_e._state, o_g._state)), sam
        assert torch.equal(o_e.hyper(), o_g.hyper()) and float(o_g.hyper()[1]) == 3.0
        sd_e, sd_g = m_e.state_dict(), m_g.state_dict()
        assert all(torch.equal(sd_e[k], sd_g[k]) for k in sd_e), sam
        if sam:
            assert torch.equal(o_e._sam, o_g._sam) and o_g.perturbation_norm() > 0
            o_g.sync_from_device()
            assert o_g.step_count == 3
            sam_flat = m_g._eng().flat.clone()
        else:
            assert not torch.equal(sam_flat, m_g._eng().flat)


def test_frozen_backbone_rides_along(dev):
    """9.  FusedSAM(FusedLAMB(groups=finetune_groups(freeze_backbone=True))): no byte of the backbone's weights, states or backup is
    touched by a full step, and the head moves."""
    from chexpert_amd.optim import FusedLAMB, FusedSAM, finetune_groups
    m = build("densenet", dev)
    s = FusedSAM(FusedLAMB(m, lr=1e-2, groups=finetune_groups(m, weight_decay=1e-4, freeze_backbone=True)), rho=0.05)
    x, t = batch("densenet", dev)
    m.forward_backward(x, t)                                  # binds the engine
    s._bufs()
    s._backup.fill_(SENTINEL)
    eng = m._eng()
    head = torch.zeros(eng.flat.numel(), dtype=torch.bool)
    head_ids = {id(q) for q in m.classifier.parameters()}
    for q, off in zip(eng.params, eng.offsets):
        if id(q) in head_ids:
            head[off:off + (q.numel() + 3) // 4 * 4] = True
    head = head.to(dev)
    assert 0 < int(head.sum()) < head.numel()
    before = [eng.flat.clone()] + [v.clone() for v in s._state]
    s.train_step(m, x, t)
    after = [eng.flat] + list(s._state)
    for a, b in zip(before, after):
        assert torch.equal(a[~head], b[~head]) and not torch.equal(a[head], b[head])
    assert (s._backup[~head] == SENTINEL).all() and torch.equal(s._backup[head], before[0][head])
    assert s.perturbation_norm() > 0


def test_refusals(dev):
    """10."""
    from chexpert_amd.graph import SegmentedTrainStep
    from chexpert_amd.optim import FusedAdam, FusedSAM
    m = build("densenet", dev)
    s = FusedSAM(FusedAdam(m, lr=1e-3))
    x, t = batch("densenet", dev)
    before = [p.detach().clone() for p in m.parameters()]
    with pytest.raises(RuntimeError, match="FusedSAM"):
        SegmentedTrainStep(m, s, x, t)
    m._eng().reducer = object()
    with pytest.raises(RuntimeError, match="data-parallel"):
        s.train_step(m, x, t)
    m._eng().reducer = None
    m.set_loss(kind="aucm", prior=[0.2] * N_CLS, margin=1.0, lr_aux=0.1)
    with pytest.raises(RuntimeError, match="aucm"):
        s.train_step(m, x, t)
    with pytest.raises(RuntimeError, match="train_step"):
        s.step()
    assert all(torch.equal(a, b) for a, b in zip(before, m.parameters())) and m._nbt_pending == 0


def test_bf16_storage_trains(dev):
    """11."""
    from chexpert_amd.optim import FusedAdam, FusedSAM
    m = build("densenet", dev, torch.bfloat16)
    s = FusedSAM(FusedAdam(m, lr=1e-3), rho=0.05, adaptive=True)
    x, t = batch("densenet", dev)
    before = [p.detach().clone() for p in m.parameters()]
    loss, logits = s.train_step(m, x, t)
    assert math.isfinite(loss.item()) and torch.isfinite(logits).all() and s.perturbation_norm() > 0
    assert all(torch.isfinite(p).all() for p in m.parameters())
    assert sum(not torch.equal(a, b) for a, b in zip(before, m.parameters())) > len(before) // 2


def _cli(argv):
    import contextlib
    import io
    import json
    from chexpert_amd import cli
    buf = io.StringIO()
    with contextlib.redirect_stdout(buf):
        cli.main(argv)
    return [json.loads(l) for l in buf.getvalue().splitlines() if l.startswith('{"step"')]


_CLI = ["--train", "--fused_optimizer", "--batch_size", "4", "--resize", "64", "--eval_interval", "4", "--log_interval", "1", "--seed", "3"]


def test_cli_trains_under_graph_logs_the_norm_and_saves_the_entry(dev, tmp_path):
    """18 images in minibatches of 4: four replays of the captured step, then the partial minibatch through train_step(dev=True) on
    the same device-resident state."""
    import os
    lines = _cli(_CLI + ["--graph", "--sam_rho", "0.05", "--sam_adaptive", "--clip_grad_norm", "5", "--synthetic", "18",
                         "--output_dir", str(tmp_path)])
    assert [l["step"] for l in lines] == [1, 2, 3, 4, 5] and all(math.isfinite(l["train_loss"]) for l in lines), lines
    assert all(math.isfinite(l["sam_norm"]) and l["sam_norm"] > 0 and l["grad_norm"] > 0 for l in lines), lines
    sd = torch.load(os.path.join(str(tmp_path), "optim_checkpoint_latest.pt"))
    assert sd["sam"] == {"rho": 0.05, "adaptive": True, "eps": 1e-12} and sd["kind"] == "FusedAdam" and sd["step_count"] == 4


_LAMB = ["--optimizer", "lamb", "--weight_decay", "1e-2", "--synthetic", "8", "--eval_interval", "2"]


@pytest.fixture(scope="module")
def sam_run(dev, tmp_path_factory):
    """One eager (no --graph) SAM run under LAMB, two minibatches, shared by the two tests below: (output folder, log lines)."""
    out = str(tmp_path_factory.mktemp("sam_run"))
    return out, _cli(_CLI + _LAMB + ["--sam_rho", "0.1", "--output_dir", out])


def test_cli_eager_step_under_lamb(dev, sam_run):
    """Without --graph the step is train_step(dev=False); the base's log entries ride along."""
    import os
    out, lines = sam_run
    assert [l["step"] for l in lines] == [1, 2] and all(l["sam_norm"] > 0 and math.isfinite(l["train_loss"]) for l in lines), lines
    assert all(0 < l["trust_min"] <= l["trust_max"] for l in lines), lines
    sd = torch.load(os.path.join(out, "optim_checkpoint_latest.pt"))
    assert sd["sam"] == {"rho": 0.1, "adaptive": False, "eps": 1e-12} and sd["kind"] == "FusedLAMB" and sd["step_count"] == 2


def test_cli_restore_into_a_run_without_sam_and_back(dev, sam_run, tmp_path):
    """The optimiser checkpoint of a SAM run restores into a run without SAM (the base reads its own keys), and that run's into a SAM
    run again (no `sam` entry: as the flags say)."""
    import os
    b, c = str(tmp_path / "b"), str(tmp_path / "c")
    lines = _cli(_CLI + _LAMB + ["--restore", os.path.join(sam_run[0], "checkpoint_latest.pt"), "--output_dir", b])
    assert [l["step"] for l in lines] == [3, 4] and all("sam_norm" not in l and math.isfinite(l["train_loss"]) for l in lines), lines
    sd = torch.load(os.path.join(b, "optim_checkpoint_latest.pt"))
    assert "sam" not in sd and sd["step_count"] == 4
    lines = _cli(_CLI + _LAMB + ["--sam_rho", "0.2", "--restore", os.path.join(b, "checkpoint_latest.pt"), "--output_dir", c])
    assert [l["step"] for l in lines] == [5, 6] and all(l["sam_norm"] > 0 for l in lines), lines
    sd = torch.load(os.path.join(c, "optim_checkpoint_latest.pt"))
    assert sd["sam"]["rho"] == 0.2 and sd["step_count"] == 6
