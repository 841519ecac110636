"""CPU (no GPU): the host side of the focal / asymmetric loss -- the float64 oracle of tests/test_focal_gpu.py against central
differences and against the restated torchvision / timm formulas, the C entry point's declaration and its argument checks before any
launch, the wrapper's refusals, FusedNet.set_loss(kind="focal" | "asl") validation, and the command line's refusals."""
import os
import re

import pytest
import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# (gamma+, gamma-, clip, alpha); the last set has a fractional exponent below 1 together with a clip: g u^(g-1) u' is inf * 0 there
P_SETS = [(0.0, 0.0, 0.0, None), (2.0, 2.0, 0.0, 0.25), (0.0, 4.0, 0.05, None), (1.0, 4.0, 0.05, None), (0.5, 0.5, 0.2, None)]


# ------------------------------------------------------------------------------------------------ float64 oracle (as in test_focal_gpu.py)
def _elem64(x, t, w, P):
    """The definition, float64, differentiable.  Piecewise where the naive statement is inf * 0 (a hard negative at or below the
    clip with an exponent below 1): every `where` masks the OPERAND of log / exp, not only the result, so autograd never multiplies
    a zero by an infinite local derivative."""
    gp, gn, m, alpha = P
    live = t >= 0
    tt = torch.where(live, t, torch.zeros_like(t))
    p, q = torch.sigmoid(x), torch.sigmoid(-x)
    logp, logq = F.logsigmoid(x), F.logsigmoid(-x)
    one, zero = torch.ones_like(x), torch.zeros_like(x)
    above = p > m
    pm = torch.where(above, p - m, zero)
    logpn = logq if m == 0 else torch.where(above, torch.log(torch.where(above, q + m, one)), zero)
    w = one if w is None else w
    C = -(w * tt * logp + (1 - tt) * logpn)
    u = tt * q + (1 - tt) * pm
    g = gp * tt + gn * (1 - tt)
    pos = (u > 0) & (g > 0)
    f = torch.where(g == 0, one, torch.where(pos, torch.exp(g * torch.log(torch.where(pos, u, one))), zero))
    a = one if alpha is None else alpha * tt + (1 - alpha) * (1 - tt)
    return torch.where(live, a * f * C, zero)


def oracle(logits, t, w, P):
    """(loss, element losses, d loss / d logits) by autograd in float64; loss = sum of elements / B."""
    x = logits.double().clone().requires_grad_(True)
    le = _elem64(x, t.double(), None if w is None else w.double(), P)
    loss = le.sum() / x.shape[0]
    loss.backward()
    return loss.detach(), le.detach(), x.grad


def _case(seed, B, n, P):
    g = torch.Generator().manual_seed(seed)
    x = torch.rand(B, n, generator=g, dtype=torch.float64) * 12 - 6
    t = (torch.rand(B, n, generator=g) < 0.3).double()
    soft = torch.rand(B, n, generator=g) < 0.2
    t[soft] = torch.rand(B, n, generator=g, dtype=torch.float64)[soft]
    t[torch.rand(B, n, generator=g) < 0.2] = -1.0
    t[0, 0], t[1, 0], t[2, 0] = 0.0, 0.0, 1.0
    x[0, 0] = -5.0                                                      # a hard negative far below every clip in P_SETS
    x[1, 0] = 3.0
    w = torch.rand(n, generator=g, dtype=torch.float64) * 7.5 + 0.5
    return x, t, w


@pytest.mark.parametrize("P", P_SETS)
def test_oracle_gradients_against_central_differences(P):
    """Central differences with h = 1e-6 in float64: truncation h^2 f''' / 6 ~ 1e-12 and rounding eps |f| / h ~ 1e-9 for a loss of
    order 1..10, so 1e-7 leaves two digits of room and still catches any wrong term (those are of order 1e-2 and more).  Towards the
    clip the third derivative grows like g (g-1) (g-2) u^(g-3) (p q)^3 for g < 1; no element with a negative share sits closer to
    it than 1e-3 in probability (asserted), where h^2 / 6 of that is 1e-12 * 0.375 * 3e7 * 0.16^3 / 6 < 1e-8."""
    h = 1e-6
    x, t, w = _case(7, 9, 4, P)
    m = P[2]
    loss, le, gx = oracle(x, t, w, P)
    assert bool(torch.isfinite(gx).all()) and bool(torch.isfinite(le).all()) and float(gx.abs().max()) > 1e-3
    assert bool((gx[t < 0] == 0).all()) and bool((le[t < 0] == 0).all())
    below = (t == 0) & (torch.sigmoid(x) <= m)
    if m > 0:
        assert below[0, 0] and bool((gx[below] == 0).all()) and bool((le[below] == 0).all())      # the hard threshold, finite and exact
        assert float((torch.sigmoid(x) - m).abs()[(t >= 0) & (t < 1)].min()) > 1e-3

    def f(x_):
        return float(_elem64(x_, t, w, P).sum() / x.shape[0])
    worst = 0.0
    for i in range(x.shape[0]):
        for c in range(x.shape[1]):
            e = torch.zeros_like(x)
            e[i, c] = h
            worst = max(worst, abs((f(x + e) - f(x - e)) / (2 * h) - gx[i, c].item()))
    print("P=%s: oracle vs central differences: max abs err %.3e" % (P, worst))
    assert worst < 1e-7


def test_oracle_without_focusing_is_the_cross_entropy():
    x, t, w = _case(11, 16, 5, P_SETS[0])
    live = (t >= 0).double()
    for pw in (None, w):
        _, le, gx = oracle(x, t, pw, P_SETS[0])
        xr = x.clone().requires_grad_(True)
        ref = F.binary_cross_entropy_with_logits(xr, t.clamp(min=0), reduction="none", pos_weight=pw) * live
        (ref.sum() / x.shape[0]).backward()
        assert float((le - ref.detach()).abs().max()) < 1e-12 and float((gx - xr.grad).abs().max()) < 1e-12


def _torchvision_focal(x, t, alpha, gamma):
    """torchvision.ops.sigmoid_focal_loss, reduction 'none', restated (alpha < 0: no class balance)."""
    p = torch.sigmoid(x)
    ce = F.binary_cross_entropy_with_logits(x, t, reduction="none")
    p_t = p * t + (1 - p) * (1 - t)
    loss = ce * ((1 - p_t) ** gamma)
    if alpha >= 0:
        loss = (alpha * t + (1 - alpha) * (1 - t)) * loss
    return loss


def _timm_asl(x, y, gamma_neg, gamma_pos, clip, eps=1e-8):
    """timm.loss.AsymmetricLossMultiLabel.forward restated, element-wise (timm returns minus the sum of this)."""
    xs_pos = torch.sigmoid(x)
    xs_neg = 1 - xs_pos
    if clip is not None and clip > 0:
        xs_neg = (xs_neg + clip).clamp(max=1)
    loss = y * torch.log(xs_pos.clamp(min=eps)) + (1 - y) * torch.log(xs_neg.clamp(min=eps))
    if gamma_neg > 0 or gamma_pos > 0:
        pt = xs_pos * y + xs_neg * (1 - y)
        loss = loss * torch.pow(1 - pt, gamma_pos * y + gamma_neg * (1 - y))
    return -loss


def test_oracle_is_the_torchvision_focal_loss():
    x, t, _ = _case(13, 16, 5, P_SETS[1])
    live = t >= 0
    for gamma, alpha in ((2.0, 0.25), (2.0, None), (1.0, 0.6), (4.0, None), (0.0, 0.25)):
        _, le, _ = oracle(x, t, None, (gamma, gamma, 0.0, alpha))
        ref = _torchvision_focal(x, t.clamp(min=0), -1.0 if alpha is None else alpha, gamma)        # soft targets included
        assert float((le - ref)[live].abs().max()) < 1e-12, (gamma, alpha)


def test_oracle_is_the_timm_asymmetric_loss_on_hard_targets():
    x, t, _ = _case(17, 16, 5, P_SETS[2])
    hard = (t == 0) | (t == 1)
    assert int(hard.sum()) > 30
    for gp, gn, m in ((0.0, 4.0, 0.05), (1.0, 4.0, 0.05), (0.5, 0.5, 0.2), (0.0, 0.0, 0.0), (2.0, 1.0, 0.0)):
        _, le, _ = oracle(x, t, None, (gp, gn, m, None))
        ref = _timm_asl(x, t.clamp(min=0), gn, gp, m)
        assert float((le - ref)[hard].abs().max()) < 1e-12, (gp, gn, m)


# ------------------------------------------------------------------------------------------------ library
def test_asl_symbol_matches_the_header():
    from chexpert_amd import _lib
    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "chexpert_hip.h")).read(), flags=re.S)
    m = re.search(r"\bint\s+cx_asl_fwd_bwd\s*\(([^;{]*?)\)\s*;", hdr, flags=re.S)
    assert m, "cx_asl_fwd_bwd is not declared in include/chexpert_hip.h"
    assert len(_lib.SIGNATURES["cx_asl_fwd_bwd"]) == m.group(1).count(",") + 1 == 11
    assert hasattr(_lib.lib(), "cx_asl_fwd_bwd")
    assert _lib.lib().cx_abi_version() == 10                           # an additive entry point
    mk = open(os.path.join(ROOT, "chexpert_amd", "csrc", "Makefile")).read()
    assert re.search(r"^SRCS\s*=.*\bloss\.hip\b", mk, flags=re.M)
    assert "cx_asl_fwd_bwd" in open(os.path.join(ROOT, "INTEGRATION.md")).read()


def test_entry_point_validates_without_launching():
    """Bad arguments give CX_EINVAL before anything is launched (no GPU here: a launch would fail with a positive HIP error)."""
    from chexpert_amd import _lib
    f = _lib.lib().cx_asl_fwd_bwd
    x, t, fo, o = (torch.zeros(64) for _ in range(4))
    X, T, FO, O = (v.data_ptr() for v in (x, t, fo, o))

    def call(x_=X, t_=T, f_=FO, B=2, n=5):
        return f(x_, t_, None, f_, O, None, None, 1.0, B, n, None)
    assert call(x_=None) == call(t_=None) == call(f_=None) == -1
    assert call(B=0) == call(B=-2) == call(n=0) == call(n=-1) == call(B=1 << 20, n=1 << 12) == -1


def test_ops_wrapper_refuses_before_any_launch():
    from chexpert_amd import ops
    x, t, fo, loss = torch.zeros(2, 5), torch.zeros(2, 5), torch.tensor([0.0, 4.0, 0.05, -1.0]), torch.zeros(1)
    with pytest.raises(RuntimeError, match="GPU only"):                # well-formed, but on the CPU
        ops.asl_fwd_bwd(x, t, None, fo, loss, None, None)
    with pytest.raises(RuntimeError, match="GPU only"):
        ops.asl_fwd_bwd(x, t, torch.ones(5), fo, loss, torch.zeros(2, 5), torch.zeros(2, 5))
    bad = [dict(logits=torch.zeros(10)), dict(logits=torch.zeros(2, 5, 1)), dict(target=torch.zeros(2, 4)), dict(target=torch.zeros(5, 2)),
           dict(pos_weight=torch.ones(4)), dict(pos_weight=torch.ones(1, 5)), dict(focus=torch.zeros(3)), dict(focus=torch.zeros(5)),
           dict(focus=None), dict(loss=torch.zeros(0)), dict(loss_elem=torch.zeros(2, 4)), dict(dlogits=torch.zeros(10)),
           dict(logits=x.double()), dict(target=t.double()), dict(target=t.long()), dict(pos_weight=torch.ones(5).double()),
           dict(focus=fo.double()), dict(loss=loss.double()), dict(dlogits=torch.zeros(2, 5).half()),
           dict(logits=torch.zeros(5, 2).t()), dict(target=torch.zeros(5, 2).t()), dict(dlogits=torch.zeros(5, 2).t())]
    for kw in bad:
        args = dict(logits=x, target=t, pos_weight=None, focus=fo, loss=loss, loss_elem=None, dlogits=None)
        args.update(kw)
        with pytest.raises(AssertionError):
            ops.asl_fwd_bwd(**args)


# ------------------------------------------------------------------------------------------------ set_loss / the loss modules
def _model():
    from chexpert_amd.models import DenseNet
    return DenseNet(32, (2, 2, 2, 2), 64, num_classes=5)


def test_set_loss_validates_its_arguments():
    model = _model()
    keys = list(model.state_dict().keys())
    before = model.loss_state()
    assert before == {"kind": "bce", "aux": None, "prior": None, "margin": 1.0, "lr_aux": None}      # what it has always been
    assert model.loss_focus is None and model.loss_step_state() == []
    nan, inf = float("nan"), float("inf")
    bad = [dict(kind="focal", gamma=-1.0), dict(kind="focal", gamma=nan), dict(kind="focal", gamma=inf), dict(kind="focal", alpha=0.0),
           dict(kind="focal", alpha=1.0), dict(kind="focal", alpha=-0.25), dict(kind="focal", alpha=nan),
           dict(kind="asl", gamma_pos=-0.5), dict(kind="asl", gamma_neg=-1.0), dict(kind="asl", gamma_neg=nan), dict(kind="asl", clip=-0.1),
           dict(kind="asl", clip=1.0), dict(kind="asl", clip=nan),
           dict(kind="focal", pos_weight=[1.0] * 4), dict(kind="asl", pos_weight=[1.0, 1.0, 0.0, 1.0, 1.0]), dict(kind="asl", pos_weight=[1.0, 1.0, -2.0, 1.0, 1.0]),
           dict(kind="asl", pos_weight=[1.0, 1.0, nan, 1.0, 1.0]),
           # a keyword that belongs to another kind
           dict(kind="focal", gamma_neg=4.0), dict(kind="focal", gamma_pos=0.0), dict(kind="focal", clip=0.05), dict(kind="asl", gamma=2.0),
           dict(kind="asl", alpha=0.25), dict(kind="focal", prior=[0.1] * 5), dict(kind="asl", lr_aux=0.1), dict(kind="asl", margin=0.5),
           dict(gamma=2.0), dict(alpha=0.25), dict(clip=0.05), dict(gamma_pos=1.0), dict(kind="bce", gamma_neg=4.0),
           dict(kind="aucm", prior=[0.1] * 5, lr_aux=0.1, gamma=2.0), dict(kind="aucm", prior=[0.1] * 5, lr_aux=0.1, clip=0.05),
           dict(kind="focus")]
    for kw in bad:
        with pytest.raises(ValueError):
            model.set_loss(**kw)
    with pytest.raises(TypeError):
        model.set_loss(False, None, "focal")                          # the new arguments are keyword-only
    for ok in (dict(kind="focal"), dict(kind="focal", gamma=0.0, alpha=0.25), dict(kind="asl"), dict(kind="asl", gamma_pos=1.0, gamma_neg=4.0, clip=0.0),
               dict(kind="asl", pos_weight=[2.0] * 5)):
        with pytest.raises(RuntimeError, match="model.to"):           # valid, but the state lives on the device
            model.set_loss(**ok)
    # nothing moved
    assert (model.loss_kind, model.loss_ignore_negative, model.loss_pos_weight, model.loss_focus) == ("bce", False, None, None)
    assert list(model.state_dict().keys()) == keys and model.loss_state() == before
    assert model.load_loss_state(before) is model and model.loss_kind == "bce"
    for d in ({"kind": "focal"}, {"kind": "asl", "focus": None}, {"kind": "asl", "focus": torch.zeros(3)},
              {"kind": "asl", "focus": torch.tensor([0.0, 4.0, 1.5, -1.0])}, {"kind": "focal", "focus": torch.tensor([-1.0, 2.0, 0.0, -1.0])},
              {"kind": "hinge", "focus": torch.zeros(4)}):
        with pytest.raises(ValueError):
            model.load_loss_state(d)
    assert model.loss_kind == "bce" and model.loss_focus is None


def test_loss_modules_surface():
    from chexpert_amd.loss import AsymmetricLoss, FocalLoss
    f = FocalLoss()
    assert f.focus.tolist() == [2.0, 2.0, 0.0, -1.0] and f.pos_weight is None and not list(f.parameters()) and not f.state_dict()
    assert FocalLoss(gamma=1.5, alpha=0.25).focus.tolist() == [1.5, 1.5, 0.0, 0.25]
    a = AsymmetricLoss()
    assert [round(v, 6) for v in a.focus.tolist()] == [0.0, 4.0, 0.05, -1.0]
    assert AsymmetricLoss(1.0, 2.0, 0.0, pos_weight=[1.0, 2.0]).pos_weight.tolist() == [1.0, 2.0]
    for crit in (f, a):
        with pytest.raises(RuntimeError, match="GPU only"):           # device tensors only
            crit(torch.zeros(2, 3), torch.zeros(2, 3))
        with pytest.raises(RuntimeError, match="GPU only"):
            crit.elementwise(torch.zeros(2, 3), torch.zeros(2, 3))
    for make in (lambda: FocalLoss(gamma=-1.0), lambda: FocalLoss(alpha=0.0), lambda: FocalLoss(alpha=1.0), lambda: FocalLoss(alpha=-1.0),
                 lambda: AsymmetricLoss(gamma_pos=-1.0), lambda: AsymmetricLoss(gamma_neg=float("nan")), lambda: AsymmetricLoss(clip=1.0),
                 lambda: AsymmetricLoss(clip=-0.01), lambda: AsymmetricLoss(pos_weight=[1.0, 0.0]), lambda: FocalLoss(pos_weight=[-1.0])):
        with pytest.raises(ValueError):
            make()


# ------------------------------------------------------------------------------------------------ command line
def test_parser_flags_and_their_defaults():
    from chexpert_amd import cli
    a = cli.build_parser().parse_args([])
    assert (a.loss, a.focal_gamma, a.focal_alpha, a.asl_gamma_pos, a.asl_gamma_neg, a.asl_clip) == ("bce", None, None, None, None, None)
    assert cli.focus_options(a) is None
    a = cli.build_parser().parse_args(["--loss", "focal"])
    assert cli.focus_options(a) == {"kind": "focal", "gamma": 2.0, "alpha": None}
    a = cli.build_parser().parse_args(["--loss", "focal", "--focal_gamma", "1.5", "--focal_alpha", "0.25"])
    assert cli.focus_options(a) == {"kind": "focal", "gamma": 1.5, "alpha": 0.25}
    a = cli.build_parser().parse_args(["--loss", "asl"])
    assert cli.focus_options(a) == {"kind": "asl", "gamma_pos": 0.0, "gamma_neg": 4.0, "clip": 0.05}
    a = cli.build_parser().parse_args(["--loss", "asl", "--asl_gamma_pos", "1", "--asl_gamma_neg", "3", "--asl_clip", "0"])
    assert cli.focus_options(a) == {"kind": "asl", "gamma_pos": 1.0, "gamma_neg": 3.0, "clip": 0.0}
    assert cli.aucm_options(a) is None
    # the sample-mixing flags, refused with --loss aucm, parse with the new losses (soft targets are defined for them)
    for loss in ("asl", "focal"):
        a = cli.parse_args(["--loss", loss, "--mixup", "0.2", "--cutmix", "1.0", "--erase_prob", "0.3", "--uncertain", "ignore", "--pos_weight", "auto"])
        assert a.loss == loss and a.mixup == 0.2 and cli.focus_options(a)["kind"] == loss
    with pytest.raises(SystemExit):
        cli.parse_args(["--loss", "aucm", "--mixup", "0.2"])
    text = cli.build_parser().format_help()
    assert "--focal_gamma" in text and "--asl_clip" in text and "stays the cross-entropy" in " ".join(text.split())
    assert "--loss {focal,asl}" in cli.__doc__


def test_command_line_refusals_come_before_anything_runs(tmp_path, monkeypatch):
    from chexpert_amd import cli
    out = str(tmp_path / "o")
    base = ["--train", "--synthetic", "16", "--output_dir", out]
    for extra in (["--focal_gamma", "-1"], ["--focal_gamma", "nan"], ["--focal_gamma", "inf"], ["--focal_alpha", "0"], ["--focal_alpha", "1"],
                  ["--focal_alpha", "-0.5"], ["--focal_alpha", "nan"]):
        with pytest.raises(ValueError, match="--focal_"):
            cli.main(base + ["--loss", "focal"] + extra)
    for extra in (["--asl_gamma_pos", "-1"], ["--asl_gamma_neg", "-0.5"], ["--asl_gamma_neg", "nan"], ["--asl_clip", "1"], ["--asl_clip", "-0.1"],
                  ["--asl_clip", "nan"]):
        with pytest.raises(ValueError, match="--asl_"):
            cli.main(base + ["--loss", "asl"] + extra)
    # flags of a loss that is not chosen
    for loss in ([], ["--loss", "bce"], ["--loss", "asl"], ["--loss", "aucm"]):
        for extra in (["--focal_gamma", "2"], ["--focal_alpha", "0.25"]):
            with pytest.raises(ValueError, match="--loss focal"):
                cli.main(base + loss + extra)
    for loss in ([], ["--loss", "bce"], ["--loss", "focal"], ["--loss", "aucm"]):
        for extra in (["--asl_gamma_pos", "0"], ["--asl_gamma_neg", "4"], ["--asl_clip", "0.05"]):
            with pytest.raises(ValueError, match="--loss asl"):
                cli.main(base + loss + extra)
    for loss in ("focal", "asl"):
        for extra in (["--aucm_margin", "0.5"], ["--aucm_lr_aux", "0.1"], ["--aucm_prior", "auto"]):
            with pytest.raises(ValueError, match="--loss aucm"):
                cli.main(base + ["--loss", loss] + extra)
    # more than one rank is NOT a refusal for these losses: the options pass where --loss aucm raises
    monkeypatch.setattr(cli.P, "dist_info", lambda: (0, 2, 0))
    with pytest.raises(ValueError, match="--asl_clip"):               # (the next check is reached)
        cli.main(base + ["--loss", "asl", "--asl_clip", "2"])
    assert not os.path.exists(out)                                     # refused before the run wrote anything
