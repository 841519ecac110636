"""CPU (no GPU): the host side of the hierarchical label loss -- the float64 oracle of tests/test_hier_gpu.py against central differences
and, for a table of roots, against F.binary_cross_entropy_with_logits; an fp32 torch restatement of the header's arithmetic on confident
elements (beside the pure log-sum-exp form, which loses the small losses); the 14-label table, its tree and the closure of a label
table under it; the two C entry points' declarations and their argument checks before any launch; the wrappers', set_loss's and the
loss module's refusals; the command line's defaults and refusals."""
import math
import os
import re

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from chexpert_amd import synth

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CHEXPERT = [-1, -1, 1, -1, 3, 3, 3, 6, 3, -1, -1, -1, -1, -1]
LN2 = math.log(2.0)


# ------------------------------------------------------------------------------------------------ float64 oracle (as in test_hier_gpu.py)
def paths_of(parent):
    """path(k) for every k: k and its ancestors, root first."""
    out = []
    for k, a in enumerate(parent):
        out.append(([] if a < 0 else out[a]) + [k])
    return out


def log1mexp(u):
    """log(1 - exp(u)) for u < 0: log(-expm1(u)) above -ln 2, log1p(-exp(u)) below; each branch sees only its own arguments, so autograd
    meets no infinity behind the where."""
    hi = u > -LN2
    return torch.where(hi, torch.log(-torch.expm1(torch.where(hi, u, -torch.ones_like(u)))),
                       torch.log1p(-torch.exp(torch.where(hi, -torch.ones_like(u), u))))


def _elem64(x, t, parent, mode, w):
    """The (B, n) element losses in float64, differentiable in x.  mode 0: the cross-entropy of sigmoid(x_k) where t >= 0 and every
    proper ancestor's target is >= 0.5.  mode 1: the cross-entropy of P_k = prod_{path} sigmoid(x_j) where t >= 0; log P_k is a sum of
    logsigmoids.  w: None or (n,) weights of the positive term."""
    B, n = x.shape
    paths = paths_of(parent)
    t = t.double()
    live = t >= 0
    tt = torch.where(live, t, torch.zeros_like(t))
    ww = torch.ones(n, dtype=torch.float64) if w is None else w.double()
    if mode == 0:
        for k, p in enumerate(paths):
            for a in p[:-1]:
                live[:, k] &= t[:, a] >= 0.5
        le = -(ww * tt * F.logsigmoid(x) + (1 - tt) * F.logsigmoid(-x))
    else:
        ls = F.logsigmoid(x)
        u = torch.stack([ls[:, p].sum(1) for p in paths], 1)
        le = -(ww * tt * u + (1 - tt) * log1mexp(u))
    return torch.where(live, le, torch.zeros_like(le))


def oracle(logits, t, parent, mode, w=None):
    """(loss, element losses (B, n), d loss / d logits (B, n)) by autograd in float64; loss = sum of elements / B."""
    x = logits.double().clone().requires_grad_(True)
    le = _elem64(x, t, parent, mode, w)
    loss = le.sum() / x.shape[0]
    loss.backward()
    return loss.detach(), le.detach(), x.grad


def case(seed, B, parent):
    """Logits uniform in +-8, targets from {-1, 0, 1, 0.3, 0.7}, weights in [0.5, 8]."""
    n = len(parent)
    x = synth.uniform(seed, (B, n), -8.0, 8.0)
    t = torch.tensor([-1.0, 0.0, 1.0, 0.3, 0.7])[synth.uniform(seed + 1, (B, n), 0.0, 5.0).long().clamp(max=4)]
    return x, t, synth.uniform(seed + 2, (n,), 0.5, 8.0)


def confident_case(which, B=64, parent=CHEXPERT):
    """0: all logits in [4, 12], t = 1.  1: all in [-12, -4], t = 0 (the smallest loss, a product of three such sigmoids, is about
    5e-15).  2: confident-positive inner nodes (t = 1) over confident-negative leaves (t = 0)."""
    n = len(parent)
    mag = synth.uniform(91 + which, (B, n), 4.0, 12.0)
    if which == 0:
        return mag, torch.ones(B, n)
    if which == 1:
        return -mag, torch.zeros(B, n)
    inner = torch.tensor([k in parent for k in range(n)])
    return torch.where(inner, mag, -mag), inner.float().expand(B, n).contiguous()


# ------------------------------------------------------------------------------------------------ the oracle itself
@pytest.mark.parametrize("mode", [0, 1])
@pytest.mark.parametrize("weighted", [False, True])
def test_oracle_gradients_against_central_differences(mode, weighted):
    """Central differences with h = 1e-6 in float64, the step and the bound (1e-7) of the other losses' oracle tests: truncation
    h^2 f''' / 6 ~ 1e-13, rounding eps |f| / h ~ 1e-8 for a loss of order 100; a wrong term is of order 1e-2 and more."""
    h = 1e-6
    x, t, w = case(7, 6, CHEXPERT)
    x, w = x.double(), (w if weighted else None)
    assert len(set(t.flatten().tolist())) == 5                        # every kind of target: ignored, hard, soft on either side
    _, le, gx = oracle(x, t, CHEXPERT, mode, w)
    assert bool(torch.isfinite(gx).all()) and bool((le >= 0).all()) and float(gx.abs().max()) > 1e-3

    def f(x_):
        return float(_elem64(x_, t, CHEXPERT, mode, w).sum() / x.shape[0])
    worst = 0.0
    for i in range(x.shape[0]):
        for j in range(x.shape[1]):
            e = torch.zeros_like(x)
            e[i, j] = h
            worst = max(worst, abs((f(x + e) - f(x - e)) / (2 * h) - gx[i, j].item()))
    print("mode %d weighted=%s: oracle vs central differences: max abs err %.3e" % (mode, weighted, worst))
    assert worst < 1e-7


@pytest.mark.parametrize("mode", [0, 1])
def test_oracle_of_a_table_of_roots_is_the_masked_cross_entropy(mode):
    x, t, w = case(11, 16, [-1] * 9)
    for pw in (None, w):
        _, le, gx = oracle(x, t, [-1] * 9, mode, pw)
        xr = x.double().clone().requires_grad_(True)
        ref = F.binary_cross_entropy_with_logits(xr, t.double().clamp(min=0), pos_weight=None if pw is None else pw.double(), reduction="none")
        ref = torch.where(t >= 0, ref, torch.zeros_like(ref))
        (ref.sum() / 16).backward()
        assert float((le - ref.detach()).abs().max()) < 1e-12 and float((gx - xr.grad).abs().max()) < 1e-12
        assert bool((le[t < 0] == 0).all()) and bool((gx[t < 0] == 0).all())


def test_oracle_modes_differ_and_a_negative_ancestor_switches_the_child_off():
    x, t, _ = case(13, 32, CHEXPERT)
    _, le0, g0 = oracle(x, t, CHEXPERT, 0)
    _, le1, g1 = oracle(x, t, CHEXPERT, 1)
    roots = [k for k, a in enumerate(CHEXPERT) if a < 0]
    assert float((le0[:, roots] - le1[:, roots]).abs().max()) < 1e-12 and float((le0 - le1).abs().max()) > 1e-2
    off = (t[:, 3] < 0.5) & (t[:, 5] >= 0)                              # Edema under a Lung Opacity that is not positive
    assert bool(off.any()) and bool((le0[off, 5] == 0).all()) and bool((g0[off, 5] == 0).all()) and bool((le1[off, 5] > 0).all())
    # in mode 1 a leaf's term reaches every ancestor: Pneumonia (7) moves Consolidation (6) and Lung Opacity (3)
    only = torch.full_like(t, -1.0)
    only[:, 7] = t[:, 7].clamp(min=0)
    _, _, g = oracle(x, only, CHEXPERT, 1)
    assert bool((g[:, [3, 6, 7]] != 0).all()) and bool((g[:, [0, 1, 2, 4, 5, 8, 9, 10, 11, 12, 13]] == 0).all())


# ------------------------------------------------------------------------------------------------ the header's arithmetic in fp32
def header_fp32(z, t, parent, w=None, pure_lse=False):
    """include/chexpert_hip.h, cx_hier_fwd_bwd, mode 1, restated in torch fp32 on (B, n): (element losses, d(sum of elements)/dz), the
    additions in the header's order.  pure_lse: log(1 - P) by the log-sum-exp of the a_j everywhere, without the log1p branch."""
    z, t = z.float(), t.float()
    B, n = z.shape
    e = torch.log1p(torch.exp(-z.abs()))
    lp, lq = -(torch.clamp(-z, min=0) + e), -(torch.clamp(z, min=0) + e)
    q = 1 / (1 + torch.exp(z))
    le, g = torch.zeros(B, n), torch.zeros(B, n)
    for k, path in enumerate(paths_of(parent)):
        u, a = torch.zeros(B), []
        for j in path:
            a.append(u + lq[:, j])
            u = u + lp[:, j]
        a = torch.stack(a, 1)
        m = a.max(1).values
        s = torch.zeros(B)
        for c in range(a.shape[1]):
            s = s + torch.exp(a[:, c] - m)
        lse = m + torch.log(s)
        l1m = lse if pure_lse else torch.where(u <= -np.float32(LN2), torch.log1p(-torch.exp(u)), lse)
        wk = 1.0 if w is None else w[k].float()
        live, tk = t[:, k] >= 0, t[:, k]
        assert u.dtype == l1m.dtype == torch.float32
        le[:, k] = torch.where(live, -wk * tk * u - (1 - tk) * l1m, torch.zeros(B))
        for j in path:
            g[:, j] = g[:, j] + torch.where(live, (1 - tk) * torch.exp(u + lq[:, j] - l1m) - wk * tk * q[:, j], torch.zeros(B))
    return le, g


def test_header_arithmetic_on_random_logits():
    """The statement on the 14-finding tree, logits in +-8, mixed hard, soft and ignored targets: 1e-5 of the largest reference magnitude,
    the bound of the GPU test (measured: 1.1e-7)."""
    x, t, w = case(17, 64, CHEXPERT)
    for pw in (None, w):
        _, le_ref, g_ref = oracle(x, t, CHEXPERT, 1, pw)
        le, g = header_fp32(x, t, CHEXPERT, pw)
        el = float((le.double() - le_ref).abs().max() / le_ref.abs().max())
        eg = float((g.double() - g_ref * 64).abs().max() / (g_ref * 64).abs().max())
        print("weighted=%s: header form vs float64: loss_elem %.3e gradient %.3e of the largest magnitude" % (pw is not None, el, eg))
        assert el < 1e-5 and eg < 1e-5


def test_header_arithmetic_keeps_confident_elements_and_the_pure_log_sum_exp_does_not():
    """Loss and gradient of every confident element within 2e-5 OF ITS OWN float64 value (measured worst case 2.7e-6, on the small
    losses of case 1); the pure log-sum-exp form loses every digit of a loss of 5e-15: it rounds at the magnitude of 1."""
    for which in range(3):
        z, t = confident_case(which)
        B = z.shape[0]
        _, le_ref, g_ref = oracle(z, t, CHEXPERT, 1)
        g_ref = g_ref * B
        assert bool((le_ref > 0).all()) and bool((g_ref != 0).all())
        if which == 1:
            assert 1e-16 < float(le_ref.min()) < 1e-13
        errs = {}
        for pure in (False, True):
            le, g = header_fp32(z, t, CHEXPERT, pure_lse=pure)
            errs[pure] = (float(((le.double() - le_ref).abs() / le_ref).max()), float(((g.double() - g_ref).abs() / g_ref.abs()).max()))
        print("case %d: header form rel err loss %.3e gradient %.3e; pure log-sum-exp loss %.3e gradient %.3e"
              % (which, errs[False][0], errs[False][1], errs[True][0], errs[True][1]))
        assert errs[False][0] < 2e-5 and errs[False][1] < 2e-5
        if which == 1:
            assert errs[True][0] > 0.5


def test_header_arithmetic_at_the_extremes():
    """+-1e4 on a chain of depth 3: finite, and the closed forms 1e4 - ln(depth) and 1e4 x depth; the factorised gradient
    q_j exp(u - l1m) is 0 * inf there."""
    chain = [-1, 0, 1]
    le, g = header_fp32(torch.full((2, 3), 1e4), torch.zeros(2, 3), chain)
    assert bool(torch.isfinite(le).all()) and bool(torch.isfinite(g).all())
    assert torch.allclose(le[0].double(), torch.tensor([1e4, 1e4 - math.log(2), 1e4 - math.log(3)], dtype=torch.float64), rtol=1e-5)
    # (the exponent u + lq_j - l1m is a difference of numbers of size 1e4, whose fp32 spacing is 1e-3: the gradient carries that)
    assert torch.allclose(g[0].double(), torch.tensor([1 + 1 / 2 + 1 / 3, 1 / 2 + 1 / 3, 1 / 3], dtype=torch.float64), rtol=2e-3)
    le, g = header_fp32(torch.full((2, 3), -1e4), torch.ones(2, 3), chain)
    assert bool(torch.isfinite(le).all()) and bool(torch.isfinite(g).all())
    assert le[0].tolist() == [1e4, 2e4, 3e4] and g[0].tolist() == [-3.0, -2.0, -1.0]
    z = torch.full((1,), 1e4)
    assert not math.isfinite(float((1 / (1 + torch.exp(z))) * torch.exp(torch.zeros(1) - (-z))))      # the form the header rules out


# ------------------------------------------------------------------------------------------------ labels
def test_label_names_tree_and_closure():
    from chexpert_amd import data
    names, par = data.ATTR_NAMES_ALL, data.CHEXPERT_PARENT
    assert par == CHEXPERT and len(names) == len(par) == 14 and set(data.ATTR_NAMES) <= set(names) and data.ATTR_NAMES == data.ChexpertCSV.attr_names
    tree = {names[k]: (None if a < 0 else names[a]) for k, a in enumerate(par)}
    assert tree["Cardiomegaly"] == "Enlarged Cardiomediastinum" and tree["Pneumonia"] == "Consolidation"
    assert all(tree[c] == "Lung Opacity" for c in ("Lung Lesion", "Edema", "Consolidation", "Atelectasis"))
    assert sum(v is None for v in tree.values()) == 8 and all(-1 <= a < k for k, a in enumerate(par))
    lab = np.zeros((6, 14), dtype=np.float32)
    lab[0, 2] = 1.0                        # Cardiomegaly under a blank Enlarged Cardiomediastinum
    lab[1, 7], lab[1, 6], lab[1, 3] = 1.0, -1.0, 0.3     # Pneumonia: Consolidation (ignored) and Lung Opacity (smoothed) become 1
    lab[2, 7], lab[2, 3] = 0.0, 0.0        # a negative child says nothing
    lab[3, 5] = -1.0                       # nor does an ignored one
    lab[4, 8] = 0.7                        # a smoothed positive counts (>= 0.5) ...
    lab[5, 8] = 0.3                        # ... a smoothed negative does not
    got = data.hierarchy_closure(lab, par)
    want = lab.copy()
    want[0, 1] = 1.0
    want[1, 6] = want[1, 3] = 1.0
    want[4, 3] = 1.0
    assert got is not lab and got.dtype == np.float32 and np.array_equal(got, want) and lab[0, 1] == 0.0
    tt = data.hierarchy_closure(torch.from_numpy(lab), par)
    assert isinstance(tt, torch.Tensor) and np.array_equal(tt.numpy(), want)
    assert np.array_equal(data.hierarchy_closure(want, par), want)                           # idempotent
    assert np.array_equal(data.hierarchy_closure(lab[:, :5], [-1] * 5), lab[:, :5])          # roots alone: nothing moves
    for bad in ([-1] * 13, [0] + [-1] * 13, [-1, 2] + [-1] * 12, [-2] + [-1] * 13):
        with pytest.raises(ValueError):
            data.hierarchy_closure(lab, bad)


def test_csv_reads_all_fourteen_labels(tmp_path):
    from chexpert_amd import data
    folder = tmp_path / data.DIR_NAME
    folder.mkdir()
    cols = ["Path", "Sex", "Age", "Frontal/Lateral", "AP/PA"] + data.ATTR_NAMES_ALL
    rows = []
    vals = ["", "0.0", "1.0", "-1.0"]
    for i in range(6):
        rows.append(["%s/train/patient%05d/study1/view1_frontal.jpg" % (data.DIR_NAME, i), "Male", "50", "Frontal", "AP"]
                    + [vals[(i + k) % 4] for k in range(14)])
    for name in ("train.csv", "valid.csv"):
        (folder / name).write_text("\n".join([",".join(cols)] + [",".join(r) for r in rows]) + "\n")
    num = {"": 0.0, "0.0": 0.0, "1.0": 1.0, "-1.0": -1.0}
    raw = np.array([[num[vals[(i + k) % 4]] for k in range(14)] for i in range(6)], dtype=np.float32)
    ds = data.ChexpertCSV(str(tmp_path), "train", labels="all", uncertain="ignore")
    assert ds.attr_names == data.ATTR_NAMES_ALL and tuple(ds.targets.shape) == (6, 14) and np.array_equal(ds.targets.numpy(), raw)
    ones = data.ChexpertCSV(str(tmp_path), "train", labels="all")
    assert np.array_equal(ones.targets.numpy(), np.where(raw < 0, 1.0, raw))
    valid = data.ChexpertCSV(str(tmp_path), "valid", labels="all")
    assert np.array_equal(valid.targets.numpy(), raw)
    five = data.ChexpertCSV(str(tmp_path), "train")                                           # the default is what it was
    cols5 = [data.ATTR_NAMES_ALL.index(a) for a in data.ATTR_NAMES]
    assert five.attr_names == data.ATTR_NAMES and data.ChexpertCSV.attr_names == data.ATTR_NAMES
    assert np.array_equal(five.targets.numpy(), np.where(raw < 0, 1.0, raw)[:, cols5])
    with pytest.raises(ValueError):
        data.ChexpertCSV(str(tmp_path), "train", labels="fourteen")


# ------------------------------------------------------------------------------------------------ library
@pytest.mark.parametrize("name,count", [("cx_hier_fwd_bwd", 12), ("cx_hier_collapse", 7)])
def test_symbols_match_the_header(name, count):
    from chexpert_amd import _lib
    text = open(os.path.join(ROOT, "include", "chexpert_hip.h")).read()
    hdr = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    m = re.search(r"\bint\s+%s\s*\(([^;{]*?)\)\s*;" % name, hdr, flags=re.S)
    assert m, "%s is not declared in include/chexpert_hip.h" % name
    assert len(_lib.SIGNATURES[name]) == m.group(1).count(",") + 1 == count
    assert hasattr(_lib.lib(), name)
    assert _lib.lib().cx_abi_version() == 10                           # additive entry points
    assert name in open(os.path.join(ROOT, "INTEGRATION.md")).read()
    assert int(re.search(r"#define CX_HIER_MAX_LABELS (\d+)", text).group(1)) == _lib.HIER_MAX_LABELS == 64
    assert int(re.search(r"#define CX_HIER_MAX_PATH (\d+)", text).group(1)) == _lib.HIER_MAX_PATH == 8
    from chexpert_amd.loss import KERNEL
    assert KERNEL["hier"] == "cx_hier_fwd_bwd"


def test_entry_points_validate_without_launching():
    """Bad arguments give CX_EINVAL before anything is launched (no GPU here: a launch would fail with a positive HIP error)."""
    from chexpert_amd import _lib
    f, g = _lib.lib().cx_hier_fwd_bwd, _lib.lib().cx_hier_collapse
    x, t, o = (torch.zeros(256) for _ in range(3))
    par = torch.full((256,), -1, dtype=torch.int32)
    X, T, O, P = (v.data_ptr() for v in (x, t, o, par))

    def call(x_=X, t_=T, p_=P, mode=0, B=2, n=5):
        return f(x_, t_, p_, None, mode, O, None, None, 1.0, B, n, None)
    assert call(x_=None) == call(t_=None) == call(p_=None) == -1
    assert call(B=0) == call(B=-2) == call(n=0) == call(n=-1) == call(n=65) == call(B=1 << 26, n=64) == -1
    assert call(mode=2) == call(mode=-1) == call(mode=1, n=65) == -1

    def coll(x_=X, p_=P, z_=O, B=2, n=5):
        return g(x_, p_, z_, None, B, n, None)
    assert coll(x_=None) == coll(p_=None) == coll(z_=None) == -1
    assert coll(B=0) == coll(B=-2) == coll(n=0) == coll(n=-1) == coll(n=65) == coll(B=1 << 26, n=64) == -1


def test_parent_table_check():
    from chexpert_amd import ops
    ok = ops.check_hier_parent("t", CHEXPERT, 14)
    assert ok.dtype == torch.int32 and not ok.is_cuda and ok.tolist() == CHEXPERT
    assert ops.check_hier_parent("t", torch.tensor(CHEXPERT)).tolist() == CHEXPERT
    assert ops.check_hier_parent("t", [-1] + list(range(7))).tolist() == [-1] + list(range(7))       # a chain of 8: the longest path
    assert ops.check_hier_parent("t", [-1] * 64).numel() == 64
    bad = [([-1] * 13, 14), ([-1] * 15, 14), ([], None), ([-1] * 65, None), ([0], None), ([-1, 1], None), ([-1, 2, -1], None),
           ([-2, -1], None), ([-1] + list(range(8)), None), ([-1, 0.5], None), ("ab", None), ([[-1, 0]], 1)]
    for table, n in bad:
        with pytest.raises(ValueError, match="^who"):
            ops.check_hier_parent("who", table, n)
    with pytest.raises(ValueError, match="8 ancestors.*at most 8"):                             # depth 9
        ops.check_hier_parent("who", [-1] + list(range(8)))


def test_ops_wrappers_refuse_before_any_launch():
    from chexpert_amd import ops
    x, t, w, loss = torch.zeros(2, 5), torch.zeros(2, 5), torch.ones(5), torch.zeros(1)
    par = [-1, 0, 1, -1, 3]
    for mode in (0, 1, "conditional", "unconditional"):
        with pytest.raises(RuntimeError, match="GPU only"):            # well-formed, but on the CPU
            ops.hier_fwd_bwd(x, t, par, None, mode, loss, None, None)
    with pytest.raises(RuntimeError, match="GPU only"):
        ops.hier_fwd_bwd(x, t, torch.tensor(par, dtype=torch.int32), w, 1, loss, torch.zeros(2, 5), torch.zeros(2, 5))
    for kw in (dict(parent=[-1] * 4), dict(parent=[-1] * 6), dict(parent=[-1, 1, -1, -1, -1]), dict(parent=[-1, 0, 1, 2, 5]), dict(parent=[0, 0, 0, 0, 0]),
               dict(mode=2), dict(mode="hlcp"), dict(mode=None), dict(mode=True), dict(mode=1.0), dict(mode=[1]), dict(mode={}),
               dict(logits=torch.zeros(2, 65), target=torch.zeros(2, 65), parent=[-1] * 65),
               dict(logits=torch.zeros(1, 9), target=torch.zeros(1, 9), parent=[-1] + list(range(8)))):
        args = dict(logits=x, target=t, parent=par, pos_weight=None, mode=0, loss=loss, loss_elem=None, dlogits=None)
        args.update(kw)
        with pytest.raises(ValueError):
            ops.hier_fwd_bwd(**args)
    for kw in (dict(logits=torch.zeros(10)), dict(target=torch.zeros(2, 4)), dict(target=t.double()), dict(logits=x.double()),
               dict(pos_weight=torch.ones(4)), dict(pos_weight=w.double()), dict(loss=torch.zeros(0)), dict(loss_elem=torch.zeros(2, 4)),
               dict(dlogits=torch.zeros(5, 2)), dict(dlogits=torch.zeros(5, 2).t()), dict(logits=torch.zeros(5, 2).t())):
        args = dict(logits=x, target=t, parent=par, pos_weight=None, mode=0, loss=loss, loss_elem=None, dlogits=None)
        args.update(kw)
        with pytest.raises(AssertionError):
            ops.hier_fwd_bwd(**args)
    z = torch.zeros(2, 5)
    with pytest.raises(RuntimeError, match="GPU only"):
        ops.hier_collapse(x, par, z)
    with pytest.raises(RuntimeError, match="GPU only"):
        ops.hier_collapse(x, par, z, torch.zeros(2, 5))
    for kw in (dict(parent=[-1] * 4), dict(parent=[-1, 1, -1, -1, -1]), dict(logits=torch.zeros(2, 65), z=torch.zeros(2, 65), parent=[-1] * 65)):
        args = dict(logits=x, parent=par, z=z, p=None)
        args.update(kw)
        with pytest.raises(ValueError):
            ops.hier_collapse(**args)
    for kw in (dict(logits=torch.zeros(10)), dict(logits=x.double()), dict(z=None), dict(z=torch.zeros(2, 4)), dict(z=z.double()), dict(p=z.half()),
               dict(p=torch.zeros(2, 4))):
        args = dict(logits=x, parent=par, z=z, p=None)
        args.update(kw)
        with pytest.raises(AssertionError):
            ops.hier_collapse(**args)


# ------------------------------------------------------------------------------------------------ set_loss / the loss module
def _model(width=14):
    from chexpert_amd.models import DenseNet
    return DenseNet(32, (2, 2, 2, 2), 64, num_classes=width)


def test_set_loss_validates_its_arguments():
    model = _model()
    keys = list(model.state_dict().keys())
    before = model.loss_state()
    assert before == {"kind": "bce", "aux": None, "prior": None, "margin": 1.0, "lr_aux": None}      # what it has always been
    assert model.loss_parent is None and model.loss_mode is None and model.loss_step_state() == []
    nan = float("nan")
    P = CHEXPERT
    bad = [dict(kind="hier"), dict(kind="hier", parent=[-1] * 13), dict(kind="hier", parent=[-1] * 15), dict(kind="hier", parent=[-1] * 5),
           dict(kind="hier", parent=[0] + [-1] * 13), dict(kind="hier", parent=[-1, 2] + [-1] * 12), dict(kind="hier", parent=[-1, 1] + [-1] * 12),
           dict(kind="hier", parent=[-3] + [-1] * 13), dict(kind="hier", parent=[-1] + list(range(8)) + [-1] * 5),               # depth 9
           dict(kind="hier", parent=P, mode="hlcp"), dict(kind="hier", parent=P, mode=2), dict(kind="hier", parent=P, ignore_negative=True),
           dict(kind="hier", parent=P, pos_weight=[1.0] * 13), dict(kind="hier", parent=P, pos_weight=[0.0] * 14), dict(kind="hier", parent=P, pos_weight=[nan] * 14),
           # a keyword that belongs to another kind, and this kind's keywords with another kind
           dict(kind="hier", parent=P, class_weight=[[1.0] * 3] * 14), dict(kind="hier", parent=P, prior=[0.1] * 14), dict(kind="hier", parent=P, lr_aux=0.1),
           dict(kind="hier", parent=P, margin=0.5), dict(kind="hier", parent=P, gamma=2.0), dict(kind="hier", parent=P, alpha=0.25),
           dict(kind="hier", parent=P, gamma_pos=0.0), dict(kind="hier", parent=P, gamma_neg=4.0), dict(kind="hier", parent=P, clip=0.05),
           dict(parent=P), dict(mode="conditional"), dict(kind="bce", parent=P), dict(kind="asl", parent=P), dict(kind="focal", mode="unconditional"),
           dict(kind="aucm", prior=[0.1] * 14, lr_aux=0.1, parent=P), dict(kind="multiclass", parent=P), dict(kind="hierarchy", parent=P)]
    for kw in bad:
        with pytest.raises(ValueError):
            model.set_loss(**kw)
    with pytest.raises(ValueError, match="14"):                        # the table's length is the head's width
        model.set_loss(kind="hier", parent=[-1] * 5)
    n65 = _model(65)
    with pytest.raises(ValueError):
        n65.set_loss(kind="hier", parent=[-1] * 65)
    for ok in (dict(kind="hier", parent=P), dict(kind="hier", parent=torch.tensor(P), mode="unconditional"),
               dict(kind="hier", parent=P, mode=1, pos_weight=[2.0] * 14)):
        with pytest.raises(RuntimeError, match="model.to"):           # valid, but the state lives on the device
            model.set_loss(**ok)
    # nothing moved
    assert (model.loss_kind, model.loss_ignore_negative, model.loss_pos_weight, model.loss_parent, model.loss_mode) == ("bce", False, None, None, None)
    assert list(model.state_dict().keys()) == keys and model.loss_state() == before
    for d in ({"kind": "hier"}, {"kind": "hier", "parent": None, "mode": "conditional"}, {"kind": "hier", "parent": torch.tensor([-1] * 5), "mode": "conditional"},
              {"kind": "hier", "parent": torch.tensor(P), "mode": "sideways"}):
        with pytest.raises(ValueError):
            model.load_loss_state(d)
    with pytest.raises(RuntimeError, match="model.to"):
        model.load_loss_state({"kind": "hier", "parent": torch.tensor(P, dtype=torch.int32), "mode": "unconditional"})
    assert model.loss_kind == "bce" and model.loss_parent is None and model.loss_state() == before


def test_loss_module_surface():
    from chexpert_amd.loss import HierarchicalBCE, collapse_hierarchy
    crit = HierarchicalBCE(CHEXPERT)
    assert crit.kind == "hier" and crit.mode == "conditional" and crit.pos_weight is None and not list(crit.parameters()) and not crit.state_dict()
    assert crit.parent.dtype == torch.int32 and crit.parent.tolist() == CHEXPERT
    crit = HierarchicalBCE([-1, 0], mode="unconditional", pos_weight=[1.0, 2.0])
    assert crit.mode == "unconditional" and crit.pos_weight.tolist() == [1.0, 2.0] and HierarchicalBCE([-1, 0], mode=1).mode == "unconditional"
    with pytest.raises(RuntimeError, match="GPU only"):               # device tensors only
        crit(torch.zeros(2, 2), torch.zeros(2, 2))
    with pytest.raises(RuntimeError, match="GPU only"):
        crit.elementwise(torch.zeros(2, 2), torch.zeros(2, 2))
    with pytest.raises(RuntimeError, match="GPU only"):
        collapse_hierarchy(torch.zeros(2, 2), [-1, 0])
    for make in (lambda: HierarchicalBCE([0]), lambda: HierarchicalBCE([-1, 1]), lambda: HierarchicalBCE([]), lambda: HierarchicalBCE([-1] * 65),
                 lambda: HierarchicalBCE([-1] + list(range(8))), lambda: HierarchicalBCE([-1, 0], mode="both"),
                 lambda: HierarchicalBCE([-1, 0], pos_weight=[1.0]), lambda: HierarchicalBCE([-1, 0], pos_weight=[1.0, -1.0])):
        with pytest.raises(ValueError):
            make()


# ------------------------------------------------------------------------------------------------ command line, predict
def test_parser_flags_and_their_defaults():
    from chexpert_amd import cli
    a = cli.build_parser().parse_args([])
    assert a.labels == "competition" and a.loss == "bce" and a.hier_mode is None and a.hier_parents is None and a.no_hier_closure is False
    assert a.n_classes == 5 and cli.hier_options(a) is None
    a = cli.parse_args([])
    assert a.n_classes == 5 and a.labels == "competition" and cli.hier_options(a) is None
    assert cli.parse_args(["--n_classes", "14"]).n_classes == 14 and cli.parse_args(["--n_classes", "3"]).n_classes == 3
    a = cli.parse_args(["--labels", "all"])
    assert a.n_classes == 14 and a.loss == "bce" and cli.hier_options(a) is None and cli.head_width(a) == 14
    assert cli.parse_args(["--labels", "all", "--n_classes", "14"]).n_classes == 14
    with pytest.raises(SystemExit):
        cli.parse_args(["--labels", "all", "--n_classes", "5"])
    a = cli.parse_args(["--labels", "all", "--loss", "hier"])
    assert cli.hier_options(a) == {"parent": CHEXPERT, "mode": None, "closure": True, "explicit": False}       # (no --hier_mode: a restored
    assert cli.hier_mode_of(cli.hier_options(a)) == "conditional"                                               # checkpoint may still say)
    assert cli.focus_options(a) is None and cli.aucm_options(a) is None and cli.multiclass_options(a) is False
    a = cli.parse_args(["--loss", "hier", "--hier_mode", "unconditional", "--hier_parents", "-1", "0", "0", "-1", "3", "--no_hier_closure",
                        "--pos_weight", "auto", "--uncertain", "ignore", "--fused_optimizer", "--graph", "--erase_prob", "0.3", "--bootstrap", "50"])
    assert cli.hier_options(a) == {"parent": [-1, 0, 0, -1, 3], "mode": "unconditional", "closure": False, "explicit": True}
    assert cli.class_names(14, "all")[7] == "Pneumonia" and cli.class_names(14)[7] == "class 7" and cli.class_names(5, "all") == cli.class_names(5)
    assert "--loss hier" in cli.__doc__ and "hier_parents" in cli.build_parser().format_help()
    # a checkpoint's table against the run's
    st = {"kind": "hier", "parent": torch.tensor([-1, 0, 0, -1, 3], dtype=torch.int32), "mode": "unconditional"}
    run = cli.hier_options(a)
    assert cli.hier_for_checkpoint(run, st, "a.pt") is run and cli.hier_for_checkpoint(run, None, "a.pt") is run
    assert cli.hier_for_checkpoint(None, {"kind": "asl"}, "a.pt") is None
    got = cli.hier_for_checkpoint(None, st, "a.pt")
    assert got == {"parent": [-1, 0, 0, -1, 3], "mode": "unconditional", "closure": True, "explicit": False}
    assert cli.hier_for_checkpoint(None, dict(st, closure=False), "a.pt")["closure"] is False
    # a run without --hier_mode continues in the stored mode; one that names another is refused, as another table is
    bare = dict(run, mode=None)
    for stored in ("unconditional", "conditional"):
        got = cli.hier_for_checkpoint(bare, dict(st, mode=stored), "a.pt")
        assert got == dict(run, mode=stored) and cli.hier_mode_of(got) == stored and bare["mode"] is None
    assert cli.hier_mode_of(cli.hier_for_checkpoint(bare, {"kind": "asl"}, "a.pt")) == "conditional"
    with pytest.raises(ValueError, match="a.pt.*--hier_mode conditional.*--hier_mode unconditional"):
        cli.hier_for_checkpoint(run, dict(st, mode="conditional"), "a.pt")
    with pytest.raises(ValueError, match="a.pt.*--loss hier"):
        cli.hier_for_checkpoint(None, st, "a.pt", train=True)
    # the members of an ensemble: all trained with the loss on the run's table, or none
    cli.check_member_hier(run, {"loss_state": st}, "c.pt")
    cli.check_member_hier(None, {"state_dict": {}}, "c.pt")
    cli.check_member_hier(None, {"loss_state": {"kind": "asl"}}, "c.pt")
    for r, ck in ((None, {"loss_state": st}), (run, {"state_dict": {}}), (run, {"loss_state": {"kind": "asl"}})):
        with pytest.raises(ValueError, match="c.pt.*--loss hier"):
            cli.check_member_hier(r, ck, "c.pt")
    with pytest.raises(ValueError, match="--hier_parents"):
        cli.check_member_hier(dict(run, parent=[-1, 0, 1, -1, 3]), {"loss_state": st}, "c.pt")
    other = dict(run, parent=[-1, 0, 1, -1, 3])
    with pytest.raises(ValueError, match=r"a.pt.*\[-1, 0, 0, -1, 3\].*--hier_parents"):
        cli.hier_for_checkpoint(other, st, "a.pt")


def test_command_line_refusals_come_before_anything_runs(tmp_path):
    from chexpert_amd import cli
    out = str(tmp_path / "o")
    base = ["--train", "--synthetic", "16", "--output_dir", out]
    five = ["-1", "0", "0", "-1", "3"]
    refused = [(["--loss", "hier"], "--labels all"), (["--loss", "hier", "--hier_parents", "auto"], "--labels all"),
               (["--loss", "hier", "--labels", "all", "--uncertain", "multiclass"], "multiclass"),
               (["--loss", "hier", "--hier_parents"] + five + ["--uncertain", "multiclass"], "multiclass"),
               (["--loss", "hier", "--labels", "all", "--mixup", "0.2"], "--loss hier.*--mixup"),
               (["--loss", "hier", "--hier_parents"] + five + ["--cutmix", "1.0"], "--loss hier.*--cutmix"),
               (["--loss", "hier", "--hier_parents", "-1", "0", "0"], "--hier_parents.*5"),
               (["--loss", "hier", "--hier_parents", "-1", "0", "0", "-1", "4"], "--hier_parents"),
               (["--loss", "hier", "--hier_parents", "-1", "0", "x", "-1", "3"], "--hier_parents"),
               (["--loss", "hier", "--labels", "all", "--hier_parents"] + five, "--hier_parents.*14"),
               (["--hier_mode", "unconditional"], "--loss hier"), (["--hier_parents"] + five, "--loss hier"), (["--no_hier_closure"], "--loss hier"),
               (["--loss", "asl", "--hier_parents", "auto"], "--loss hier")]
    for extra, why in refused:
        with pytest.raises(ValueError, match=why):
            cli.main(base + extra)
    with pytest.raises(SystemExit):
        cli.main(base + ["--labels", "all", "--n_classes", "5"])
    with pytest.raises(SystemExit):
        cli.main(base + ["--loss", "hier", "--labels", "all", "--hier_mode", "both"])
    assert not os.path.exists(out)                                     # refused before the run wrote anything


def test_predict_reads_the_parent_table_from_the_checkpoint():
    from chexpert_amd import predict
    assert predict.hier_parent_of({"state_dict": {}}) is None and predict.hier_parent_of({"loss_state": {"kind": "asl"}}) is None
    ck = {"loss_state": {"kind": "hier", "parent": torch.tensor(CHEXPERT, dtype=torch.int32), "mode": "conditional"}}
    assert predict.hier_parent_of(ck) == CHEXPERT
    import inspect
    assert inspect.signature(predict.predict).parameters["collapse"].default is False
