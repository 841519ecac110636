"""CPU (no GPU): the host side of the AUC-margin loss -- the two C entry points' declaration and their argument checks before any
launch, FusedNet.set_loss(kind="aucm") validation, `--aucm_prior auto`, the command line's refusals, the data-parallel refusal, and
the float64 oracle of tests/test_aucm_gpu.py against central finite differences."""
import os
import re

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ------------------------------------------------------------------------------------------------ float64 oracle (as in test_aucm_gpu.py)
def _loss64(x, t, p, a, b, al, margin):
    """The definition, float64, differentiable: rows live when t >= 0, positive when t >= 0.5; a class without a live row adds 0."""
    y = torch.sigmoid(x)
    live = (t >= 0).double()
    P, N = live * (t >= 0.5).double(), live * (t < 0.5).double()
    cnt = live.sum(0)
    L = cnt.clamp(min=1)
    inner = p * (1 - p) * margin + (p * y * N - (1 - p) * y * P).sum(0) / L
    lc = (1 - p) * ((y - a) ** 2 * P).sum(0) / L + p * ((y - b) ** 2 * N).sum(0) / L + 2 * al * inner - p * (1 - p) * al ** 2
    return lc * (cnt > 0).double()


def oracle(logits, t, prior, aux, margin):
    """(loss, per-class terms, d loss / d logits, d loss / d aux (3, n)) by autograd in float64."""
    x = logits.double().clone().requires_grad_(True)
    a, b, al = (aux[i].double().clone().requires_grad_(True) for i in range(3))
    lc = _loss64(x, t.double(), prior.double(), a, b, al, margin)
    lc.sum().backward()
    return lc.sum().detach(), lc.detach(), x.grad, torch.stack([a.grad, b.grad, al.grad])


def _case(seed, B, n):
    g = torch.Generator().manual_seed(seed)
    x = (torch.rand(B, n, generator=g, dtype=torch.float64) * 12 - 6)
    t = (torch.rand(B, n, generator=g) < 0.3).double()
    t[torch.rand(B, n, generator=g) < 0.2] = -1.0
    t[0, 0], t[1, 0] = 0.55, 0.45                                    # soft labels on either side of the split
    prior = torch.rand(n, generator=g, dtype=torch.float64) * 0.5 + 0.05
    aux = torch.rand(3, n, generator=g, dtype=torch.float64) * 2 - 1
    aux[2] = aux[2].abs()
    return x, t, prior, aux


def test_oracle_gradients_against_central_differences():
    """Central differences with h = 1e-6 in float64: truncation h^2 f''' / 6 ~ 1e-13 and rounding eps |f| / h ~ 1e-9 for a loss of
    order 1..10, so 1e-7 leaves two digits of room and still catches any wrong term (those are of order 1e-2 and more)."""
    margin, h = 0.7, 1e-6
    x, t, prior, aux = _case(5, 9, 4)
    t[:, 3] = -1.0                                                      # a class without a live row
    loss, lc, gx, gaux = oracle(x, t, prior, aux, margin)
    assert lc[3].item() == 0.0 and bool((gx[:, 3] == 0).all()) and bool((gaux[:, 3] == 0).all())
    assert bool((gx[t < 0] == 0).all()) and float(gx.abs().max()) > 1e-3 and float(gaux[:, :3].abs().min()) > 1e-4

    def f(x_, aux_):
        return float(_loss64(x_, t, prior, aux_[0], aux_[1], aux_[2], margin).sum())
    worst = 0.0
    for i in range(x.shape[0]):
        for c in range(x.shape[1]):
            e = torch.zeros_like(x)
            e[i, c] = h
            worst = max(worst, abs((f(x + e, aux) - f(x - e, aux)) / (2 * h) - gx[i, c].item()))
    for j in range(3):
        for c in range(x.shape[1]):
            e = torch.zeros_like(aux)
            e[j, c] = h
            worst = max(worst, abs((f(x, aux + e) - f(x, aux - e)) / (2 * h) - gaux[j, c].item()))
    print("oracle vs central differences: max abs err %.3e" % worst)
    assert worst < 1e-7
    # the closed forms of the definition, term by term
    y = torch.sigmoid(x)
    live = (t >= 0).double()
    P, N = live * (t >= 0.5).double(), live * (t < 0.5).double()
    assert P[0, 0] == 1 and N[1, 0] == 1                                # 0.55 is a positive, 0.45 a negative
    has = (live.sum(0) > 0).double()
    L, p, (a, b, al) = live.sum(0).clamp(min=1), prior, aux
    dx = y * (1 - y) / L * (P * (1 - p) * (2 * (y - a) - 2 * al) + N * p * (2 * (y - b) + 2 * al))
    da = -(1 - p) * (2 * (y - a) * P).sum(0) / L * has
    db = -p * (2 * (y - b) * N).sum(0) / L * has
    dal = (2 * (p * (1 - p) * margin + (p * y * N - (1 - p) * y * P).sum(0) / L) - 2 * p * (1 - p) * al) * has
    assert float((dx - gx).abs().max()) < 1e-15 and float((torch.stack([da, db, dal]) - gaux).abs().max()) < 1e-15


# ------------------------------------------------------------------------------------------------ library
def test_aucm_symbols_match_the_header():
    from chexpert_amd import _lib
    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "chexpert_hip.h")).read(), flags=re.S)
    for name, n in (("cx_aucm_fwd_bwd", 13), ("cx_aucm_aux_step", 5)):
        m = re.search(r"\bint\s+%s\s*\(([^;{]*?)\)\s*;" % name, hdr, flags=re.S)
        assert m, "%s is not declared in include/chexpert_hip.h" % name
        assert len(_lib.SIGNATURES[name]) == m.group(1).count(",") + 1 == n
        assert hasattr(_lib.lib(), name)
    assert _lib.lib().cx_abi_version() == 10                           # additive entry points
    mk = open(os.path.join(ROOT, "chexpert_amd", "csrc", "Makefile")).read()
    assert re.search(r"^SRCS\s*=.*\bloss\.hip\b", mk, flags=re.M)


def test_entry_points_validate_without_launching():
    """Bad arguments give CX_EINVAL before anything is launched (no GPU here: a launch would fail with a positive HIP error)."""
    from chexpert_amd import _lib
    f, g = _lib.lib().cx_aucm_fwd_bwd, _lib.lib().cx_aucm_aux_step
    x, t, p, aux, o = (torch.zeros(64) for _ in range(5))
    X, T, P, A, O = (v.data_ptr() for v in (x, t, p, aux, o))

    def call(x_=X, t_=T, p_=P, a_=A, margin=1.0, B=2, n=5):
        return f(x_, t_, p_, a_, margin, O, None, None, None, 1.0, B, n, None)
    assert call(x_=None) == call(t_=None) == call(p_=None) == call(a_=None) == -1
    assert call(B=0) == call(B=-2) == call(n=0) == call(n=-1) == -1
    assert call(margin=0.0) == call(margin=-1.0) == call(margin=float("nan")) == -1
    assert g(None, O, P, 5, None) == g(A, None, P, 5, None) == g(A, O, None, 5, None) == g(A, O, P, 0, None) == -1
    assert _lib.lib().cx_error_string(-1).startswith(b"invalid argument")


def test_ops_wrappers_refuse_cpu_tensors():
    from chexpert_amd import ops
    z = torch.zeros(2, 5)
    with pytest.raises(RuntimeError, match="GPU only"):
        ops.aucm_fwd_bwd(z, z, torch.full((5,), 0.3), torch.zeros(3, 5), 1.0, torch.zeros(1), None, None, None)
    with pytest.raises(RuntimeError, match="GPU only"):
        ops.aucm_aux_step(torch.zeros(3, 5), torch.zeros(3, 5), torch.zeros(1))


# ------------------------------------------------------------------------------------------------ set_loss / the loss module
def _model():
    from chexpert_amd.models import DenseNet
    return DenseNet(32, (2, 2, 2, 2), 64, num_classes=5)


def test_set_loss_validates_its_arguments():
    model = _model()
    keys = list(model.state_dict().keys())
    assert (model.loss_kind, model.loss_aux, model.loss_prior, model.loss_lr_aux) == ("bce", None, None, None)
    ok = dict(kind="aucm", prior=[0.1, 0.2, 0.3, 0.4, 0.5], lr_aux=0.1)
    for bad in (dict(ok, kind="auc"), dict(ok, pos_weight=[1.0] * 5), dict(ok, prior=None), dict(ok, prior=[0.1] * 4),
                dict(ok, prior=[0.1, 0.2, 0.3, 0.4, 0.0]), dict(ok, prior=[0.1, 0.2, 0.3, 0.4, 1.0]), dict(ok, prior=[0.1, 0.2, 0.3, 0.4, float("nan")]),
                dict(ok, lr_aux=None), dict(ok, lr_aux=0.0), dict(ok, lr_aux=-1.0), dict(ok, margin=0.0), dict(ok, margin=-2.0),
                dict(prior=[0.1] * 5), dict(lr_aux=0.1), dict(margin=0.5), dict(kind="bce", prior=[0.1] * 5)):
        with pytest.raises(ValueError):
            model.set_loss(**bad)
    with pytest.raises(TypeError):
        model.set_loss(False, None, "aucm")                           # the new arguments are keyword-only
    with pytest.raises(RuntimeError, match="model.to"):               # valid, but the state lives on the device
        model.set_loss(**ok)
    # nothing moved: the model still holds the plain loss and its state_dict is what it was
    assert (model.loss_kind, model.loss_ignore_negative, model.loss_pos_weight, model.loss_aux) == ("bce", False, None, None)
    assert list(model.state_dict().keys()) == keys
    assert model.loss_state() == {"kind": "bce", "aux": None, "prior": None, "margin": 1.0, "lr_aux": None}
    assert model.load_loss_state(model.loss_state()) is model and model.loss_kind == "bce"
    with pytest.raises(ValueError):
        model.load_loss_state({"kind": "focal"})


def test_loss_module_surface():
    from chexpert_amd.loss import AUCMLoss
    crit = AUCMLoss([0.1, 0.2, 0.3], margin=0.5)
    assert sorted(n for n, _ in crit.named_parameters()) == ["a", "alpha", "b"]
    assert all(tuple(p.shape) == (3,) and bool((p == 0).all()) for p in crit.parameters()) and crit.margin == 0.5
    with torch.no_grad():
        crit.alpha.copy_(torch.tensor([-1.0, 0.0, 2.0]))
    assert crit.clamp_() is crit and crit.alpha.tolist() == [0.0, 0.0, 2.0]
    with pytest.raises(RuntimeError, match="no element losses"):
        crit.elementwise(torch.zeros(2, 3), torch.zeros(2, 3))
    with pytest.raises(RuntimeError, match="GPU only"):               # device tensors only
        crit(torch.zeros(2, 3), torch.zeros(2, 3))
    for bad in ([0.0, 0.5], [0.5, 1.0], []):
        with pytest.raises(ValueError):
            AUCMLoss(bad)
    with pytest.raises(ValueError):
        AUCMLoss([0.5], margin=0.0)


def test_data_parallel_is_refused_with_a_reason():
    from chexpert_amd.models._fused import check_aucm_single_process

    class Reducer:
        def __init__(self, world):
            self.world = world
    check_aucm_single_process(None)
    check_aucm_single_process(Reducer(1))
    with pytest.raises(RuntimeError, match="not supported data-parallel.*world size 2.*collective"):
        check_aucm_single_process(Reducer(2))


# ------------------------------------------------------------------------------------------------ command line
def test_parser_flags_and_prior_auto():
    from chexpert_amd import cli
    a = cli.build_parser().parse_args([])
    assert (a.loss, a.aucm_margin, a.aucm_prior, a.aucm_lr_aux) == ("bce", None, None, None)
    assert cli.aucm_options(a) is None
    a = cli.build_parser().parse_args(["--loss", "aucm", "--aucm_margin", "0.5", "--aucm_prior", "auto", "--aucm_lr_aux", "0.02", "--lr", "0.001"])
    assert (a.loss, a.aucm_margin, a.aucm_prior, a.aucm_lr_aux) == ("aucm", 0.5, ["auto"], 0.02)
    assert cli.aucm_options(a) == {"margin": 0.5, "lr_aux": 0.02}
    a = cli.build_parser().parse_args(["--loss", "aucm", "--lr", "0.003"])
    assert cli.aucm_options(a) == {"margin": 1.0, "lr_aux": 0.003}    # the rate defaults to --lr
    with pytest.raises(SystemExit):
        cli.build_parser().parse_args(["--loss", "hinge"])
    # a hand-made table: -1 is ignored, 0.55 is a positive, 0.45 a negative
    t = torch.tensor([[1.0, 0.0, -1.0, 0.55],
                      [0.0, -1.0, 1.0, 0.45],
                      [0.0, 1.0, 0.0, -1.0],
                      [-1.0, 0.0, 0.0, 0.0],
                      [1.0, 1.0, -1.0, 1.0]])
    #   class 0: 2 / 4    class 1: 2 / 4    class 2: 1 / 3    class 3: 2 positives (0.55, 1) of 4 live
    assert cli.resolve_aucm_prior(["auto"], t, 4) == [0.5, 0.5, 1.0 / 3.0, 0.5]
    assert cli.resolve_aucm_prior(None, t, 4) == cli.resolve_aucm_prior("auto", t, 4) == [0.5, 0.5, 1.0 / 3.0, 0.5]
    assert cli.resolve_aucm_prior(["0.1", "0.2", "0.3", "0.4"], None, 4) == [0.1, 0.2, 0.3, 0.4]


def test_prior_errors_name_the_class():
    from chexpert_amd import cli
    t = torch.tensor([[1.0, 0.0, -1.0, 0.0, 1.0], [0.0, 0.0, -1.0, 1.0, 1.0], [0.0, 0.0, -1.0, 1.0, 0.55]])
    for tt, c in ((t, 1), (t[:, [0, 3, 2, 3, 0]], 2), (t[:, [0, 3, 0, 3, 4]], 4)):      # no positive / no live label / no negative
        with pytest.raises(ValueError, match=r"class %d \(%s\)" % (c, cli.ATTR_NAMES[c])):
            cli.resolve_aucm_prior(["auto"], tt, 5)
    with pytest.raises(ValueError, match=r"class 3 \(Edema\)"):
        cli.resolve_aucm_prior(["0.1", "0.2", "0.3", "1.0", "0.5"], None, 5)
    with pytest.raises(ValueError, match=r"class 0 \(Atelectasis\)"):
        cli.resolve_aucm_prior(["0", "0.2", "0.3", "0.4", "0.5"], None, 5)
    with pytest.raises(ValueError, match=r"class 6 \(class 6\)"):
        cli.resolve_aucm_prior(["0.5"] * 6 + ["1.5"], None, 7)
    for bad in (["0.1", "0.2"], ["auto", "0.1"], ["x"] * 5):
        with pytest.raises(ValueError):
            cli.resolve_aucm_prior(bad, None, 5)


def test_command_line_refusals_come_before_anything_runs(tmp_path, monkeypatch):
    from chexpert_amd import cli
    out = str(tmp_path / "o")
    base = ["--train", "--synthetic", "16", "--output_dir", out]
    with pytest.raises(ValueError, match="--pos_weight"):
        cli.main(base + ["--loss", "aucm", "--pos_weight", "auto"])
    for extra in (["--aucm_margin", "0"], ["--aucm_margin", "-1"], ["--aucm_lr_aux", "0"], ["--aucm_lr_aux", "-0.1"]):
        with pytest.raises(ValueError):
            cli.main(base + ["--loss", "aucm"] + extra)
    for extra in (["--aucm_prior", "auto"], ["--aucm_lr_aux", "0.1"], ["--aucm_margin", "0.5"], ["--aucm_margin", "1.0"]):      # flags of a loss that is not chosen
        with pytest.raises(ValueError, match="--loss aucm"):
            cli.main(base + extra)
    # under torch.distributed.run with more than one rank: refused before the process group is formed
    monkeypatch.setattr(cli.P, "dist_info", lambda: (0, 2, 0))
    with pytest.raises(RuntimeError, match="--loss aucm.*not supported data-parallel.*world size 2"):
        cli.main(base + ["--loss", "aucm"])
    assert not os.path.exists(out)                                     # refused before the run wrote anything
