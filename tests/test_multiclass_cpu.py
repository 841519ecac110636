"""CPU (no GPU): the host side of the U-MultiClass policy -- the float64 oracle of tests/test_multiclass_gpu.py against central differences
and F.cross_entropy, an fp32 numpy restatement of the header's arithmetic on confident elements (beside the naive form, which loses
them), the two C entry points' declarations and their argument checks before any launch, the wrappers' refusals,
FusedNet.set_loss(kind="multiclass") validation, the loss module's surface, the label table, the command line's refusals and
predict's head-width rule."""
import os
import re

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from chexpert_amd import synth

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TARGET_OF_CLASS = {0: 0.0, 1: 1.0, 2: -1.0}


# ------------------------------------------------------------------------------------------------ float64 oracle (as in test_multiclass_gpu.py)
def classes_of(t):
    """2 where t < 0, 1 where t >= 0.5, else 0."""
    return torch.where(t < 0, 2, torch.where(t >= 0.5, 1, 0))


def _elem64(x, c, w):
    """-log softmax_c of every triple, float64, differentiable: logsumexp(z) - z_c, times w[k][c]."""
    B, n = c.shape
    z = x.view(B, n, 3)
    le = torch.logsumexp(z, 2) - z.gather(2, c[..., None])[..., 0]
    return le if w is None else le * w[torch.arange(n)[None].expand(B, n), c]


def oracle(logits, t, w):
    """(loss, element losses (B, n), d loss / d logits (B, 3n)) by autograd in float64; loss = sum of elements / B."""
    x = logits.double().clone().requires_grad_(True)
    le = _elem64(x, classes_of(t), None if w is None else w.double())
    loss = le.sum() / x.shape[0]
    loss.backward()
    return loss.detach(), le.detach(), x.grad


def confident_case(c, B=64, n=5):
    """Every element's class is c and its logit leads the other two by gaps uniform in [4, 12]; the leading logit itself is uniform in
    +-8, so its magnitude is what a cancelling form loses digits against."""
    zc = synth.uniform(61 + c, (B, n), -8.0, 8.0)
    rest = [zc - synth.uniform(71 + c, (B, n), 4.0, 12.0), zc - synth.uniform(81 + c, (B, n), 4.0, 12.0)]
    z = torch.stack([zc if j == c else rest.pop(0) for j in range(3)], 2)
    return z.reshape(B, 3 * n).contiguous(), torch.full((B, n), TARGET_OF_CLASS[c])


def _case(seed, B, n):
    x = synth.uniform(seed, (B, 3 * n), -8.0, 8.0).double()
    t = torch.tensor([-1.0, 0.0, 1.0, 0.3, 0.5, 0.7])[(synth.uniform(seed + 1, (B, n), 0.0, 6.0)).long().clamp(max=5)]
    w = synth.uniform(seed + 2, (n, 3), 0.5, 8.0).double()
    return x, t, w


def test_classes_of_the_target_table():
    t = torch.tensor([-1.0, -0.25, 0.0, 0.3, 0.49999, 0.5, 0.7, 1.0])
    assert classes_of(t).tolist() == [2, 2, 0, 0, 0, 1, 1, 1]


@pytest.mark.parametrize("weighted", [False, True])
def test_oracle_gradients_against_central_differences(weighted):
    """Central differences with h = 1e-6 in float64, the step and the bound (1e-7) of the focal loss's oracle test: truncation
    h^2 f''' / 6 ~ 1e-13 (the softmax's third derivative is below 1, times a weight below 8) and rounding eps |f| / h ~ 1e-8 for a loss
    of order 100; a wrong term is of order 1e-2 and more."""
    h = 1e-6
    x, t, w = _case(7, 9, 4)
    w = w if weighted else None
    c = classes_of(t)
    assert set(c.flatten().tolist()) == {0, 1, 2}
    _, le, gx = oracle(x, t, w)
    assert bool(torch.isfinite(gx).all()) and bool((le > 0).all()) and float(gx.abs().max()) > 1e-3

    def f(x_):
        return float(_elem64(x_, c, w).sum() / x.shape[0])
    worst = 0.0
    for i in range(x.shape[0]):
        for j in range(x.shape[1]):
            e = torch.zeros_like(x)
            e[i, j] = h
            worst = max(worst, abs((f(x + e) - f(x - e)) / (2 * h) - gx[i, j].item()))
    print("weighted=%s: oracle vs central differences: max abs err %.3e" % (weighted, worst))
    assert worst < 1e-7


def test_oracle_is_torch_cross_entropy_on_the_reshaped_logits():
    x, t, w = _case(11, 16, 5)
    B, n = t.shape
    c = classes_of(t)
    _, le, gx = oracle(x, t, None)
    xr = x.clone().requires_grad_(True)
    ref = F.cross_entropy(xr.view(B * n, 3), c.view(B * n), reduction="none").view(B, n)
    (ref.sum() / B).backward()
    assert float((le - ref.detach()).abs().max()) < 1e-12 and float((gx - xr.grad).abs().max()) < 1e-12
    # weighted: finding k's weights are its own cross-entropy's class weights
    _, le, gx = oracle(x, t, w)
    xr = x.clone().requires_grad_(True)
    ref = torch.stack([F.cross_entropy(xr.view(B, n, 3)[:, k], c[:, k], weight=w[k], reduction="none") for k in range(n)], 1)
    (ref.sum() / B).backward()
    assert float((le - ref.detach()).abs().max()) < 1e-12 and float((gx - xr.grad).abs().max()) < 1e-12


# ------------------------------------------------------------------------------------------------ the header's arithmetic in fp32
def header_fp32(z, c, naive=False):
    """include/chexpert_hip.h, cx_mc3_fwd_bwd, restated in numpy fp32 on (N, 3) logits and (N,) classes: (l, dl/dz).  naive: the forms
    the header rules out, m + log(s) - z_c and e_c / s - 1."""
    z = z.astype(np.float32)
    rows = np.arange(len(z))
    m = z.max(1)
    e = np.exp(z - m[:, None])
    s = (e[:, 0] + e[:, 1]) + e[:, 2]
    r = np.where(c == 0, e[:, 1] + e[:, 2], np.where(c == 1, e[:, 0] + e[:, 2], e[:, 0] + e[:, 1]))
    zc = z[rows, c]
    assert e.dtype == s.dtype == r.dtype == np.float32
    g = e / s[:, None]
    if naive:
        g[rows, c] = e[rows, c] / s - np.float32(1)
        return (m + np.log(s)) - zc, g
    g[rows, c] = -r / s
    return np.where(zc == m, np.log1p(r), (m - zc) + np.log(s)), g


def test_header_arithmetic_keeps_confident_elements_and_the_naive_form_does_not():
    """Loss and the three gradients of every confident element within 2e-5 OF ITS OWN float64 value (about ten roundings of 2^-24);
    the naive form, m + log(s) - z_c with e_c / s - 1, loses them: it rounds at the magnitude of m and of 1."""
    for c in range(3):
        z, t = confident_case(c)
        B, n = t.shape
        _, le_ref, g_ref = oracle(z, t, None)
        g_ref = g_ref * B
        assert bool((le_ref > 0).all()) and bool((g_ref != 0).all()) and float(le_ref.max()) < 0.04
        cls = classes_of(t).reshape(-1).numpy()
        errs = {}
        for naive in (False, True):
            l, g = header_fp32(z.numpy().reshape(B * n, 3), cls, naive)
            rl = np.abs(l.astype(np.float64).reshape(B, n) - le_ref.numpy()) / le_ref.numpy()
            rg = np.abs(g.astype(np.float64).reshape(B, 3 * n) - g_ref.numpy()) / np.abs(g_ref.numpy())
            errs[naive] = (rl.max(), rg.max())
        print("class %d: header form rel err loss %.3e gradient %.3e; naive form loss %.3e gradient %.3e"
              % (c, errs[False][0], errs[False][1], errs[True][0], errs[True][1]))
        assert errs[False][0] < 2e-5 and errs[False][1] < 2e-5
        assert errs[True][0] > 2e-5 and errs[True][1] > 2e-5


# ------------------------------------------------------------------------------------------------ library
@pytest.mark.parametrize("name,count", [("cx_mc3_fwd_bwd", 10), ("cx_mc3_collapse", 6)])
def test_symbols_match_the_header(name, count):
    from chexpert_amd import _lib
    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "chexpert_hip.h")).read(), flags=re.S)
    m = re.search(r"\bint\s+%s\s*\(([^;{]*?)\)\s*;" % name, hdr, flags=re.S)
    assert m, "%s is not declared in include/chexpert_hip.h" % name
    assert len(_lib.SIGNATURES[name]) == m.group(1).count(",") + 1 == count
    assert hasattr(_lib.lib(), name)
    assert _lib.lib().cx_abi_version() == 10                           # additive entry points
    assert name in open(os.path.join(ROOT, "INTEGRATION.md")).read()
    from chexpert_amd.loss import KERNEL
    assert KERNEL["multiclass"] == "cx_mc3_fwd_bwd"


def test_entry_points_validate_without_launching():
    """Bad arguments give CX_EINVAL before anything is launched (no GPU here: a launch would fail with a positive HIP error)."""
    from chexpert_amd import _lib
    f, g = _lib.lib().cx_mc3_fwd_bwd, _lib.lib().cx_mc3_collapse
    x, t, o = (torch.zeros(64) for _ in range(3))
    X, T, O = (v.data_ptr() for v in (x, t, o))

    def call(x_=X, t_=T, B=2, n=5):
        return f(x_, t_, None, O, None, None, 1.0, B, n, None)
    assert call(x_=None) == call(t_=None) == -1
    assert call(B=0) == call(B=-2) == call(n=0) == call(n=-1) == call(B=1 << 20, n=1 << 12) == -1

    def coll(x_=X, z_=O, B=2, n=5):
        return g(x_, z_, None, B, n, None)
    assert coll(x_=None) == coll(z_=None) == -1
    assert coll(B=0) == coll(B=-2) == coll(n=0) == coll(n=-1) == coll(B=1 << 20, n=1 << 12) == -1


def test_ops_wrappers_refuse_before_any_launch():
    from chexpert_amd import ops
    x, t, w, loss = torch.zeros(2, 15), torch.zeros(2, 5), torch.ones(5, 3), torch.zeros(1)
    with pytest.raises(RuntimeError, match="GPU only"):                # well-formed, but on the CPU
        ops.mc3_fwd_bwd(x, t, None, loss, None, None)
    with pytest.raises(RuntimeError, match="GPU only"):
        ops.mc3_fwd_bwd(x, t, w, loss, torch.zeros(2, 5), torch.zeros(2, 15))
    bad = [dict(logits=torch.zeros(30)), dict(logits=torch.zeros(2, 15, 1)), dict(logits=torch.zeros(2, 14)), dict(logits=torch.zeros(2, 5)),
           dict(target=torch.zeros(2, 15)), dict(target=torch.zeros(2, 4)), dict(target=torch.zeros(5, 2)), dict(target=torch.zeros(10)),
           dict(class_weight=torch.ones(4, 3)), dict(class_weight=torch.ones(5, 2)), dict(class_weight=torch.ones(15)), dict(class_weight=torch.ones(3, 5)),
           dict(loss=torch.zeros(0)), dict(loss_elem=torch.zeros(2, 15)), dict(loss_elem=torch.zeros(2, 4)), dict(dlogits=torch.zeros(2, 5)),
           dict(dlogits=torch.zeros(30)), dict(logits=x.double()), dict(target=t.double()), dict(target=t.long()),
           dict(class_weight=w.double()), dict(loss=loss.double()), dict(dlogits=torch.zeros(2, 15).half()),
           dict(logits=torch.zeros(15, 2).t()), dict(target=torch.zeros(5, 2).t()), dict(dlogits=torch.zeros(15, 2).t()),
           dict(class_weight=torch.ones(3, 5).t())]
    for kw in bad:
        args = dict(logits=x, target=t, class_weight=None, loss=loss, loss_elem=None, dlogits=None)
        args.update(kw)
        with pytest.raises(AssertionError):
            ops.mc3_fwd_bwd(**args)
    z = torch.zeros(2, 5)
    with pytest.raises(RuntimeError, match="GPU only"):
        ops.mc3_collapse(x, z)
    with pytest.raises(RuntimeError, match="GPU only"):
        ops.mc3_collapse(x, z, torch.zeros(2, 5))
    for kw in (dict(logits=torch.zeros(2, 14)), dict(logits=torch.zeros(30)), dict(logits=x.double()), dict(logits=torch.zeros(15, 2).t()),
               dict(z=None), dict(z=torch.zeros(2, 15)), dict(z=torch.zeros(2, 4)), dict(z=z.double()), dict(z=torch.zeros(5, 2).t()),
               dict(p_unc=torch.zeros(2, 15)), dict(p_unc=z.half())):
        args = dict(logits=x, z=z, p_unc=None)
        args.update(kw)
        with pytest.raises(AssertionError):
            ops.mc3_collapse(**args)


# ------------------------------------------------------------------------------------------------ set_loss / the loss module
def _model(width=15):
    from chexpert_amd.models import DenseNet
    return DenseNet(32, (2, 2, 2, 2), 64, num_classes=width)


def test_set_loss_validates_its_arguments():
    model = _model()
    keys = list(model.state_dict().keys())
    before = model.loss_state()
    assert before == {"kind": "bce", "aux": None, "prior": None, "margin": 1.0, "lr_aux": None}      # what it has always been
    assert model.loss_class_weight is None and model.loss_step_state() == []
    nan, inf = float("nan"), float("inf")
    ones = [[1.0] * 3] * 5
    bad = [dict(kind="multiclass", pos_weight=[1.0] * 5), dict(kind="multiclass", pos_weight=[1.0] * 15), dict(kind="multiclass", ignore_negative=True),
           dict(kind="multiclass", class_weight=[[1.0] * 3] * 4), dict(kind="multiclass", class_weight=[[1.0] * 2] * 5),
           dict(kind="multiclass", class_weight=[1.0] * 15), dict(kind="multiclass", class_weight=[[1.0] * 5] * 3),
           dict(kind="multiclass", class_weight=[[1.0, 0.0, 1.0]] * 5), dict(kind="multiclass", class_weight=[[1.0, -2.0, 1.0]] * 5),
           dict(kind="multiclass", class_weight=[[1.0, nan, 1.0]] * 5), dict(kind="multiclass", class_weight=[[1.0, inf, 1.0]] * 5),
           # a keyword that belongs to another kind, and this kind's keyword with another kind
           dict(kind="multiclass", gamma=2.0), dict(kind="multiclass", alpha=0.25), dict(kind="multiclass", gamma_pos=0.0),
           dict(kind="multiclass", gamma_neg=4.0), dict(kind="multiclass", clip=0.05), dict(kind="multiclass", prior=[0.1] * 5),
           dict(kind="multiclass", lr_aux=0.1), dict(kind="multiclass", margin=0.5),
           dict(class_weight=ones), dict(kind="bce", class_weight=ones), dict(kind="asl", class_weight=ones), dict(kind="focal", class_weight=ones),
           dict(kind="aucm", prior=[0.1] * 15, lr_aux=0.1, class_weight=ones), dict(kind="multi")]
    for kw in bad:
        with pytest.raises(ValueError):
            model.set_loss(**kw)
    with pytest.raises(TypeError):
        model.set_loss(False, None, "multiclass")                     # keyword-only
    for ok in (dict(kind="multiclass"), dict(kind="multiclass", class_weight=ones), dict(kind="multiclass", class_weight=torch.full((5, 3), 2.0))):
        with pytest.raises(RuntimeError, match="model.to"):           # valid, but the state lives on the device
            model.set_loss(**ok)
    # nothing moved
    assert (model.loss_kind, model.loss_ignore_negative, model.loss_pos_weight, model.loss_class_weight) == ("bce", False, None, None)
    assert list(model.state_dict().keys()) == keys and model.loss_state() == before
    for d in ({"kind": "multiclass", "class_weight": torch.ones(4, 3)}, {"kind": "multiclass", "class_weight": torch.zeros(5, 3)},
              {"kind": "multiclass", "class_weight": torch.ones(15)}):
        with pytest.raises(ValueError):
            model.load_loss_state(d)
    with pytest.raises(RuntimeError, match="model.to"):
        model.load_loss_state({"kind": "multiclass", "class_weight": None})
    assert model.loss_kind == "bce" and model.loss_class_weight is None and model.loss_state() == before
    # a head that is no multiple of three outputs cannot hold the loss
    for width in (5, 14, 16):
        with pytest.raises(ValueError, match="three outputs per finding"):
            _model(width).set_loss(kind="multiclass")


def test_loss_module_surface():
    from chexpert_amd.loss import MultiClassUncertain, collapse_multiclass
    crit = MultiClassUncertain()
    assert crit.kind == "multiclass" and crit.class_weight is None and not list(crit.parameters()) and not crit.state_dict()
    w = MultiClassUncertain(class_weight=[[1.0, 2.0, 3.0], [4.0, 5.0, 6.0]]).class_weight
    assert w.dtype == torch.float32 and w.tolist() == [[1.0, 2.0, 3.0], [4.0, 5.0, 6.0]]
    with pytest.raises(RuntimeError, match="GPU only"):               # device tensors only
        crit(torch.zeros(2, 6), torch.zeros(2, 2))
    with pytest.raises(RuntimeError, match="GPU only"):
        crit.elementwise(torch.zeros(2, 6), torch.zeros(2, 2))
    with pytest.raises(RuntimeError, match="GPU only"):
        collapse_multiclass(torch.zeros(2, 6))
    for make in (lambda: MultiClassUncertain([1.0, 2.0, 3.0]), lambda: MultiClassUncertain([[1.0, 2.0]]), lambda: MultiClassUncertain([[1.0, 0.0, 1.0]]),
                 lambda: MultiClassUncertain([[1.0, -1.0, 1.0]]), lambda: MultiClassUncertain([[1.0, float("nan"), 1.0]]),
                 lambda: MultiClassUncertain(torch.ones(3, 5))):
        with pytest.raises(ValueError):
            make()


# ------------------------------------------------------------------------------------------------ labels, command line, predict
def test_multiclass_label_table_is_the_ignore_table():
    from chexpert_amd import cli, data
    assert "multiclass" in data.UNCERTAIN_POLICIES
    lab = np.array([[-1.0, 0.0, 1.0], [1.0, -1.0, 0.0], [0.0, 0.0, -1.0]], dtype=np.float32)
    got = data.apply_uncertain(lab, "multiclass", seed=3)
    assert got.dtype == np.float32 and np.array_equal(got, data.apply_uncertain(lab, "ignore", seed=3)) and np.array_equal(got, lab)
    assert got is not lab
    a = cli.SyntheticXrays(200, 8, 5, 7, uncertain_frac=0.2, uncertain="multiclass").targets
    assert torch.equal(a, cli.SyntheticXrays(200, 8, 5, 7, uncertain_frac=0.2, uncertain="ignore").targets) and bool((a < 0).any())


def test_parser_flags_and_their_defaults():
    from chexpert_amd import cli
    a = cli.build_parser().parse_args([])
    assert a.uncertain == "ones" and cli.multiclass_options(a) is False and cli.head_width(a) == 5
    a = cli.parse_args(["--uncertain", "multiclass"])
    assert a.loss == "bce" and cli.multiclass_options(a) is True and cli.head_width(a) == 15 and a.n_classes == 5
    assert cli.focus_options(a) is None and cli.aucm_options(a) is None
    a = cli.parse_args(["--uncertain", "multiclass", "--n_classes", "14", "--erase_prob", "0.3", "--fused_optimizer", "--graph",
                        "--bootstrap", "50", "--calibrate", "platt", "--plot_roc"])
    assert cli.multiclass_options(a) is True and cli.head_width(a) == 42
    for p in ("ones", "zeros", "ignore", "ones_lsr", "zeros_lsr"):
        a = cli.parse_args(["--uncertain", p, "--loss", "asl", "--mixup", "0.2", "--pos_weight", "auto"])
        assert cli.multiclass_options(a) is False and cli.head_width(a) == 5
    assert "multiclass" in cli.build_parser().format_help() and "U-MultiClass" in cli.__doc__
    # a checkpoint's head against the run's, both ways
    bce, mc = {"state_dict": {}}, {"state_dict": {}, "loss_state": {"kind": "multiclass", "class_weight": None}}
    asl = {"state_dict": {}, "loss_state": {"kind": "asl"}}
    cli.check_checkpoint_head(bce, False, "a.pt")
    cli.check_checkpoint_head(asl, False, "a.pt")
    cli.check_checkpoint_head(mc, True, "a.pt")
    for ck, run in ((bce, True), (asl, True), (mc, False)):
        with pytest.raises(ValueError, match="a.pt.*--uncertain multiclass"):
            cli.check_checkpoint_head(ck, run, "a.pt")


def test_command_line_refusals_come_before_anything_runs(tmp_path):
    from chexpert_amd import cli
    out = str(tmp_path / "o")
    base = ["--train", "--synthetic", "16", "--output_dir", out, "--uncertain", "multiclass"]
    for extra, flag in ((["--loss", "focal"], "--loss focal"), (["--loss", "asl"], "--loss asl"), (["--loss", "aucm"], "--loss aucm"),
                        (["--pos_weight", "auto"], "--pos_weight"), (["--pos_weight"] + ["1.0"] * 5, "--pos_weight"),
                        (["--mixup", "0.2"], "--mixup"), (["--cutmix", "1.0"], "--cutmix"), (["--mixup", "0.2", "--cutmix", "1.0"], "--mixup"),
                        (["--visualize"], "--visualize"), (["--visualize", "--cam_classes", "0"], "--visualize"),
                        (["--visualize", "--saliency", "grad"], "--visualize")):
        with pytest.raises(ValueError, match="--uncertain multiclass.*%s" % flag):
            cli.main(base + extra)
    with pytest.raises(ValueError, match="--uncertain multiclass.*--visualize"):       # outside training too
        cli.main(["--visualize", "--synthetic", "16", "--output_dir", out, "--uncertain", "multiclass"])
    assert not os.path.exists(out)                                     # refused before the run wrote anything


def test_predict_reads_the_head_width_from_the_checkpoint():
    from chexpert_amd import predict
    for key in ("classifier.weight", "fc.weight"):
        assert predict.head_is_multiclass({key: torch.zeros(5, 8)}, key, 5) is False
        assert predict.head_is_multiclass({key: torch.zeros(15, 8)}, key, 5) is True
        assert predict.head_is_multiclass({key: torch.zeros(42, 8)}, key, 14) is True
        for rows in (10, 14, 16, 45, 1):
            with pytest.raises(ValueError, match=r"ck\.pt.*%d rows.*5 findings.*need 5 .*or 15 " % rows):
                predict.head_is_multiclass({key: torch.zeros(rows, 8)}, key, 5, "ck.pt")
    import inspect
    assert inspect.signature(predict.predict).parameters["collapse"].default is False
