"""Barlow Twins pretraining on the GPU: cx_barlow_fwd_bwd against the float64 statement (loss.reference_barlow) within the rounding
bound test_barlow_cpu derives, its reproducibility and edge cases, the fused step against the autograd route, the captured step, SAM,
and the command line (--pretrain barlow, --restore, --init_backbone)."""
import json
import math
import os
import shutil

import numpy as np
import pytest
import torch

from chexpert_amd import synth
from eager_step import _eager_dev_step
from test_barlow_cpu import LAMBDAS, LAYOUTS, SHAPES, case, check_against, tolerance

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def dev():
    from chexpert_amd import _lib
    _lib.lib()
    return torch.device("cuda:0")


def run(dev, e, ids, lambd, outputs="lgs", grad_scale=1.0, scratch=None):
    """One call of ops.barlow_fwd_bwd with the outputs named in `outputs` (l loss, g gradient, s stats), each prefilled with a value
    the kernels never write.  Returns them (None where not asked for) as device tensors."""
    from chexpert_amd import ops
    x = torch.tensor(np.array(e, dtype=np.float32)).to(dev).contiguous()
    g = torch.as_tensor(np.asarray(ids), dtype=torch.float32).reshape(-1, 1).to(dev)
    lam = torch.tensor([lambd], dtype=torch.float32, device=dev)
    N, d = x.shape
    loss = torch.full((1,), 777.0, device=dev) if "l" in outputs else None
    grad = torch.full((N, d), 777.0, device=dev) if "g" in outputs else None
    stats = torch.full((4,), 777.0, device=dev) if "s" in outputs else None
    ops.barlow_fwd_bwd(x, g, lam, loss, grad, stats, scratch, grad_scale)
    return loss, grad, stats


def _np(*tensors):
    return [None if t is None else t.cpu().numpy() for t in tensors]


@pytest.mark.parametrize("N,d", SHAPES)
def test_kernel_against_float64(dev, N, d):
    """Loss, stats and every gradient row against the float64 statement within test_barlow_cpu.tolerance (derived there from
    u = 2^-24), at every shared case: both layouts, both lambdas."""
    from chexpert_amd.loss import reference_barlow
    for layout in LAYOUTS:
        e, ids = case(N, d, layout)
        for lambd in LAMBDAS:
            ref = reference_barlow(e, ids, lambd)
            tol = tolerance(e, ids, lambd, ref)
            loss, grad, stats = _np(*run(dev, e, ids, lambd))
            check_against(ref, tol, loss[0], stats, grad, (N, d, lambd, layout))
            if ref["m"] < 2:
                assert loss[0] == 0 and not grad.any() and stats.tolist() == [0, 0, 0, ref["m"]]
    # grad_scale multiplies the gradient alone
    l3, g3, s3 = _np(*run(dev, e, ids, lambd, grad_scale=3.0))
    assert np.array_equal(l3, loss) and np.array_equal(s3, stats)
    assert np.allclose(g3, 3.0 * grad, rtol=4 * 2.0 ** -24, atol=0)


@pytest.mark.parametrize("N,d", [(6, 5), (66, 33), (130, 136), (512, 128)])
def test_two_launches_give_equal_bits_and_each_output_alone_its_own(dev, N, d):
    e, ids = case(N, d, "negative")
    first = run(dev, e, ids, 0.0051)
    again = run(dev, e, ids, 0.0051)
    for a, b in zip(first, again):
        assert torch.equal(a, b)
    for k, name in enumerate("lgs"):
        alone = run(dev, e, ids, 0.0051, outputs=name)
        assert [o is not None for o in alone] == [i == k for i in range(3)]
        assert torch.equal(alone[k], first[k]), name
    pair = run(dev, e, ids, 0.0051, outputs="ls")
    assert torch.equal(pair[0], first[0]) and torch.equal(pair[2], first[2]) and pair[1] is None
    # a caller's scratch, larger than needed and full of NaN, and the wrapper's own give the same bits
    from chexpert_amd import ops
    big = torch.full((ops.barlow_scratch(N, d) + 100,), float("nan"), device=dev)
    held = run(dev, e, ids, 0.0051, scratch=big)
    for a, b in zip(first, held):
        assert torch.equal(a, b)
    assert torch.isnan(big[-100:]).all()


def test_rows_outside_the_batch_touch_nothing(dev):
    e, ids = case(66, 33, "negative")
    h = 33
    pair_out = (ids[:h] < 0) | (ids[h:] < 0)
    out = np.flatnonzero(np.concatenate([pair_out, pair_out]))
    zeroed, poisoned = e.copy(), e.copy()
    zeroed[out] = 0.0
    poisoned[out] = np.nan
    first = run(dev, zeroed, ids, 1.0)
    second = run(dev, poisoned, ids, 1.0)
    for a, b in zip(first, second):
        assert torch.equal(a, b)
    assert torch.isfinite(first[0]).all() and torch.isfinite(first[1]).all() and not first[1][out].any()
    assert first[2][3].item() == int((~pair_out).sum()) and first[1].abs().max() > 0
    # the odd last row is outside every pair
    e13, ids13 = case(13, 7, "full")
    p13 = e13.copy()
    p13[12] = np.nan
    a, b = run(dev, e13, ids13, 1.0), run(dev, p13, ids13, 1.0)
    for x, y in zip(a, b):
        assert torch.equal(x, y)
    assert not a[1][12].any()
    # teeth: a change to a row INSIDE the batch is seen
    inside = zeroed.copy()
    keep = np.flatnonzero(~pair_out)[0]
    inside[keep] = inside[keep] * -37.5 + 4.0
    assert not torch.equal(run(dev, inside, ids, 1.0)[1], first[1])


def test_fewer_than_two_pairs_give_exact_zeros(dev):
    e, _ = case(13, 7, "full")
    for ids, m in ((-np.ones(13), 0), (np.array([0, -1, -1, -1, -1, -1, 0, 1, 2, 3, 4, 5, 9.0]), 1),
                   (np.array([0, 1, 2, 3, 4, 5, -1, -1, -1, -1, -1, -1, 3.0]), 0)):
        loss, grad, stats = _np(*run(dev, e, ids, 1.0))
        assert loss[0] == 0 and not grad.any() and stats.tolist() == [0, 0, 0, m]
    loss, grad, stats = _np(*run(dev, e[:2], np.zeros(2), 1.0))                        # one pair
    assert loss[0] == 0 and not grad.any() and stats.tolist() == [0, 0, 0, 1]
    loss, grad, stats = _np(*run(dev, e[:3], np.zeros(3), 1.0))
    assert loss[0] == 0 and not grad.any() and stats.tolist() == [0, 0, 0, 1]


def test_a_constant_column_stays_finite(dev):
    from chexpert_amd.loss import reference_barlow
    e, ids = case(66, 33, "full")
    const = e.copy()
    const[:, 3] = 2.5
    const[:, 20] = 0.0
    ref = reference_barlow(const, ids, 1.0)
    loss, grad, stats = _np(*run(dev, const, ids, 1.0))
    assert np.isfinite(loss).all() and np.isfinite(grad).all() and np.isfinite(stats).all()
    check_against(ref, tolerance(const, ids, 1.0, ref), loss[0], stats, grad, "constant column")


@pytest.mark.parametrize("scale", [1e4, 1e-6])
def test_extreme_scales_stay_inside_the_bound(dev, scale):
    from chexpert_amd.loss import reference_barlow
    base, ids = case(130, 136, "negative")
    e = (base.astype(np.float64) * scale).astype(np.float32)
    for lambd in LAMBDAS:
        ref = reference_barlow(e, ids, lambd)
        loss, grad, stats = _np(*run(dev, e, ids, lambd))
        assert np.isfinite(loss).all() and np.isfinite(grad).all() and np.abs(grad).max() > 0
        check_against(ref, tolerance(e, ids, lambd, ref), loss[0], stats, grad, ("scale", scale, lambd))


def test_wrapper_refusals(dev):
    from chexpert_amd import ops
    from chexpert_amd.loss import BarlowTwinsLoss, barlow_terms
    x, g, t = torch.zeros(4, 8, device=dev), torch.zeros(4, 1, device=dev), torch.ones(1, device=dev)
    with pytest.raises(AssertionError):
        ops.barlow_fwd_bwd(x, g, t, None, None, scratch=torch.zeros(8, device=dev))
    with pytest.raises(AssertionError):
        ops.barlow_fwd_bwd(x, g, t, None, None, stats=torch.zeros(4, dtype=torch.float64, device=dev))
    with pytest.raises(ValueError):
        ops.barlow_fwd_bwd(torch.zeros(4, 2000, device=dev), g, t, None, None)
    with pytest.raises(ValueError):
        ops.barlow_fwd_bwd(torch.zeros(1, 8, device=dev), torch.zeros(1, 1, device=dev), t, None, None)
    with pytest.raises(RuntimeError, match=r"\(N, 1\) column of ids"):
        BarlowTwinsLoss()(x, torch.zeros(4, 8, device=dev))
    with pytest.raises(AssertionError):                                            # an operand on another device
        ops.barlow_fwd_bwd(x, g, torch.ones(1), None, None)
    with pytest.raises(RuntimeError, match="no element losses"):
        BarlowTwinsLoss().elementwise(x, g)
    e, ids = case(66, 33, "negative")
    on, off, diag, m = barlow_terms(torch.tensor(e, device=dev), torch.tensor(ids, dtype=torch.float32, device=dev))
    stats = run(dev, e, ids, 1.0, outputs="s")[2].tolist()
    assert [on, off, diag, m] == stats and isinstance(m, int)


# ------------------------------------------------------------------------------------------------ the fused step
D = 16


def _net(dev, seed=3, width=D):
    """densenet121 with a 16-wide head (the projection), at the 64 x 64 input of the other loss tests."""
    import torch.nn as nn
    from chexpert_amd.models import densenet121
    torch.manual_seed(seed)
    model = densenet121(pretrained=False)
    model.classifier = nn.Linear(model.classifier.in_features, width)
    return model.to(dev).train(), 64


def _twin(dev):
    a, S = _net(dev)
    b, _ = _net(dev)
    b.load_state_dict({k: v.clone() for k, v in a.state_dict().items()})
    return a, b, S


def _ids(dev, B=8, which=0):
    table = [[0, 1, 2, 3, 0, 1, 2, 3], [0, 1, -1, 3, 0, 1, 2, 3], [5, 6, 7, 8, 5, 6, 7, 8], [0, 1, 2, 3, 0, -1, 2, 3]][which]
    return torch.tensor(table[:B], dtype=torch.float32, device=dev).reshape(-1, 1)


@pytest.mark.parametrize("train", [True, False])
def test_fused_step_equals_the_autograd_route(dev, train):
    from chexpert_amd import ops
    from chexpert_amd.loss import BarlowTwinsLoss, MaskedBCE, reference_barlow
    a, b, S = _twin(dev)
    a.train(train), b.train(train)
    B = 8
    x = synth.xray_batch(5500, B, S).to(dev)
    t = _ids(dev, B, 1)
    keys = list(a.state_dict().keys())
    assert a.set_loss(kind="barlow", lambd=0.05) is a
    crit = BarlowTwinsLoss(0.05)
    assert list(a.state_dict().keys()) == keys and a.loss_step_state() == []
    assert a.loss_kind == "barlow" and a.loss_ignore_negative is False and a.loss_pos_weight is None and a.loss_temperature is None
    lam = a.loss_lambda
    assert lam.is_cuda and tuple(lam.shape) == (1,) and lam.item() == pytest.approx(0.05)
    dx = torch.empty(B, 3, S, S, dtype=torch.float32, device=dev)
    loss_a, logits_a = a.forward_backward(x, t, input_grad=dx)
    assert tuple(logits_a.shape) == (B, D)
    xb = x.clone().requires_grad_(True)
    out = b(xb)
    loss_b = crit(out, t)
    loss_b.backward()
    assert loss_b.dim() == 0 and torch.equal(loss_a.reshape(()), loss_b.detach())
    assert torch.equal(logits_a, out.detach())
    ga, gb = dict(a.named_parameters()), dict(b.named_parameters())
    for k in ga:
        assert torch.equal(ga[k].grad, gb[k].grad), k
    assert max(float(p.grad.abs().max()) for p in ga.values()) > 0
    assert xb.grad is not None and torch.equal(xb.grad, dx) and float(dx.abs().max()) > 0
    # the loss is the float64 statement's on these logits
    ref = reference_barlow(logits_a.cpu().numpy(), t.cpu().numpy(), 0.05)
    tol = tolerance(logits_a.cpu().numpy(), t.cpu().numpy().reshape(-1), 0.05, ref)
    print("train %s: fused loss %.7f, float64 statement %.7f" % (train, loss_a.item(), ref["loss"]))
    assert ref["m"] == 3 and abs(loss_a.item() - ref["loss"]) <= tol["loss"] and ref["loss"] > 0
    # backward scales by the incoming gradient
    xl = logits_a.clone().requires_grad_(True)
    (3.0 * crit(xl, t)).backward()
    dl = torch.empty_like(logits_a)
    ops.barlow_fwd_bwd(logits_a, t, a.loss_lambda, None, dl)
    assert torch.equal(xl.grad, dl * 3.0)
    # teeth: another lambda is another gradient
    other = torch.empty_like(dl)
    ops.barlow_fwd_bwd(logits_a, t, torch.tensor([0.5], device=dev), None, other)
    assert not torch.equal(other, dl)
    with pytest.raises(RuntimeError, match="column of ids"):
        crit(out, t.reshape(-1))
    with pytest.raises(RuntimeError):
        MaskedBCE()(out, t)


def test_set_loss_walk_leaves_nothing_of_the_previous_kind(dev):
    """asl (weights) -> barlow -> barlow (another lambda: the held storage) -> ntxent -> barlow -> hier -> barlow -> bce: after every
    move the public attributes are the new kind's alone, a refused call changes nothing, and loss_state() round-trips."""
    from chexpert_amd.loss import BarlowTwinsLoss
    model, S = _net(dev)
    other, _ = _net(dev)
    pw = synth.uniform(5730, (D,), 0.5, 8.0)
    bce_state = {"kind": "bce", "aux": None, "prior": None, "margin": 1.0, "lr_aux": None}
    model.set_loss(kind="asl", pos_weight=pw)
    assert model.loss_lambda is None and model.loss_focus is not None
    model.set_loss(kind="barlow")
    held = model.loss_lambda.data_ptr()
    assert model.loss_kind == "barlow" and model.loss_lambda.item() == pytest.approx(0.0051)
    for name in ("loss_pos_weight", "loss_focus", "loss_aux", "loss_prior", "loss_lr_aux", "loss_class_weight", "loss_parent", "loss_mode",
                 "loss_temperature"):
        assert getattr(model, name) is None, name
    assert model.loss_ignore_negative is False
    model.set_loss(kind="barlow", lambd=0.02)
    assert model.loss_lambda.data_ptr() == held and model.loss_lambda.item() == pytest.approx(0.02)
    st = model.loss_state()
    assert st["kind"] == "barlow" and st["lambd"] == pytest.approx(0.02) and "focus" not in st and "temperature" not in st
    assert other.load_loss_state(st) is other and other.loss_kind == "barlow" and other.loss_lambda.item() == pytest.approx(0.02)
    assert other.loss_state() == st
    for kw in (dict(kind="barlow", pos_weight=pw), dict(kind="barlow", ignore_negative=True), dict(kind="barlow", lambd=-1.0),
               dict(kind="barlow", temperature=0.2), dict(kind="barlow", gamma=1.0), dict(kind="barlow", parent=[-1] * D),
               dict(kind="asl", lambd=0.3), dict(kind="ntxent", lambd=0.3)):
        with pytest.raises(ValueError):
            model.set_loss(**kw)
        assert model.loss_kind == "barlow" and model.loss_lambda.item() == pytest.approx(0.02) and model.loss_pos_weight is None
    model.set_loss(kind="ntxent", temperature=0.3)
    assert model.loss_lambda is None and model.loss_temperature.item() == pytest.approx(0.3) and "lambd" not in model.loss_state()
    x, t = synth.xray_batch(5700, 8, S).to(dev), _ids(dev)
    model.forward_backward(x, t)                                      # (sizes the contrastive scratch; the next kind sizes its own)
    model.set_loss(kind="barlow", lambd=0.5)
    assert model.loss_lambda.data_ptr() == held and model.loss_temperature is None
    loss, logits = model.forward_backward(x, t)
    assert torch.equal(BarlowTwinsLoss(0.5)(logits, t), loss.reshape(())) and math.isfinite(loss.item()) and loss.item() > 0
    model.set_loss(kind="hier", parent=[-1] * D)
    assert model.loss_lambda is None and model.loss_parent is not None
    model.set_loss(kind="barlow", lambd=0.5)
    assert model.loss_parent is None and model.loss_mode is None
    assert model.set_loss() is model and model.loss_lambda is None and model.loss_state() == bce_state


def test_graphed_step_equals_eager_and_sees_lambda_rewritten_in_place(dev):
    """Three replays of GraphedTrainStep over FusedAdam against three eager train_step(dev=True) calls on a twin, bit for bit; lambda
    rewritten in place before a fourth; the scratch was sized by the warm-up runs, so the capture allocated none."""
    from chexpert_amd.graph import GraphedTrainStep
    from chexpert_amd.loss import BarlowTwinsLoss
    from chexpert_amd.optim import FusedAdam
    m_e, m_g, S = _twin(dev)
    B = 8
    xs = [synth.xray_batch(5800 + i, B, S).to(dev) for i in range(5)]
    ts = [_ids(dev, B, i % 4) for i in range(5)]
    for m in (m_e, m_g):
        m.set_loss(kind="barlow", lambd=0.0051)
    opt_e, opt_g = FusedAdam(m_e, lr=1e-3), FusedAdam(m_g, lr=1e-3)
    gs = GraphedTrainStep(m_g, opt_g, xs[0], ts[2])
    scratch = m_g._loss._held["scratch"]
    held, where = m_g.loss_lambda.data_ptr(), scratch.data_ptr()
    flat = lambda m: torch.cat([p.detach().flatten() for p in m.parameters()])                               # noqa: E731
    for i in range(3):
        le, _ = opt_e.train_step(m_e, xs[i], ts[i], dev=True)
        lg, logits = gs.replay(xs[i], ts[i])
        assert tuple(logits.shape) == (B, D) and torch.equal(le.reshape(-1), lg.reshape(-1)), (i, le.item(), lg.item())
        assert torch.equal(flat(m_e), flat(m_g)), i
        assert torch.equal(m_e._eng().flat_grad, m_g._eng().flat_grad)
    le = _eager_dev_step(m_e, opt_e, xs[3], ts[3])
    lg, _ = gs.replay(xs[3], ts[3])
    assert torch.equal(le.reshape(-1), lg.reshape(-1)) and torch.equal(flat(m_e), flat(m_g))
    # lambda changes in place: the next replay reads it
    m_g.loss_lambda.fill_(0.5)
    m_e.set_loss(kind="barlow", lambd=0.5)
    assert m_g.loss_lambda.data_ptr() == held
    le = _eager_dev_step(m_e, opt_e, xs[4], ts[4])
    lg, logits = gs.replay(xs[4], ts[4])
    assert torch.equal(le.reshape(-1), lg.reshape(-1)) and torch.equal(flat(m_e), flat(m_g))
    assert BarlowTwinsLoss(0.0051)(logits, ts[4]).item() != lg.item() == BarlowTwinsLoss(0.5)(logits, ts[4]).item()
    assert m_g._loss._held["scratch"] is scratch and scratch.data_ptr() == where


def test_a_missing_scratch_under_capture_is_an_error_not_an_allocation(dev, monkeypatch):
    from chexpert_amd.loss import Loss
    state = Loss("barlow", lambd=torch.tensor([0.0051], device=dev))
    z, t = torch.randn(8, D, device=dev), _ids(dev)
    loss, dl = torch.empty(1, device=dev), torch.empty(8, D, device=dev)
    monkeypatch.setattr(torch.cuda, "is_current_stream_capturing", lambda: True)
    with pytest.raises(RuntimeError, match="Barlow Twins loss would allocate its scratch .* under a graph capture"):
        state.launch(z, t, loss, None, dl)
    assert "scratch" not in state._held
    monkeypatch.undo()
    state.launch(z, t, loss, None, dl)                                  # sized outside capture ...
    held = state._held["scratch"]
    monkeypatch.setattr(torch.cuda, "is_current_stream_capturing", lambda: True)
    state.launch(z[:4].contiguous(), t[:4].contiguous(), loss, None, dl[:4])      # ... a step that fits uses it as it is
    assert state._held["scratch"] is held
    with pytest.raises(RuntimeError, match="no element losses"):
        state.launch(z, t, None, torch.empty(8, 1, device=dev), None)


def test_one_sam_step_runs(dev):
    from chexpert_amd.optim import FusedAdam, FusedSAM
    m, S = _net(dev)
    m.set_loss(kind="barlow")
    s = FusedSAM(FusedAdam(m, lr=1e-3), rho=0.05)
    before = torch.cat([p.detach().flatten() for p in m.parameters()]).clone()
    loss, logits = s.train_step(m, synth.xray_batch(5900, 8, S).to(dev), _ids(dev))
    assert math.isfinite(float(loss)) and float(loss) > 0 and tuple(logits.shape) == (8, D)
    after = torch.cat([p.detach().flatten() for p in m.parameters()])
    assert torch.isfinite(after).all() and not torch.equal(before, after)


# ------------------------------------------------------------------------------------------------ the command line
_CLI = ["--train", "--synthetic", "8", "--batch_size", "4", "--resize", "64", "--eval_interval", "2", "--log_interval", "1", "--seed", "3",
        "--lr", "0.001"]
_PRE = ["--pretrain", "barlow", "--proj_dim", "16", "--affine", "--jitter"]


def _lines(text):
    return [json.loads(l) for l in text.splitlines() if l.startswith('{"step"')]


@pytest.fixture(scope="module")
def pretrain_run(dev, tmp_path_factory):
    """One `--pretrain barlow --affine --jitter --fused_optimizer --graph` run of two steps with an evaluation after the second, shared
    by the tests below: (output folder, model, its stdout)."""
    import contextlib
    import io
    from chexpert_amd import cli
    out = str(tmp_path_factory.mktemp("barlow") / "p")
    buf = io.StringIO()
    with contextlib.redirect_stdout(buf):
        model = cli.main(_CLI + _PRE + ["--fused_optimizer", "--graph", "--output_dir", out])
    return out, model, buf.getvalue()


def test_cli_pretraining_writes_the_json_and_the_checkpoint(dev, pretrain_run):
    out, model, text = pretrain_run
    lines = _lines(text)
    assert [l["step"] for l in lines] == [1, 2] and all(math.isfinite(l["train_loss"]) and l["train_loss"] > 0 for l in lines)
    assert all(l["on_diag"] >= 0 and l["off_diag"] >= 0 and "top1" not in l for l in lines)
    assert all(l["train_loss"] == pytest.approx(l["on_diag"] + 0.0051 * l["off_diag"], rel=1e-3, abs=1e-4) for l in lines)
    assert model.loss_kind == "barlow" and model.loss_lambda.item() == pytest.approx(0.0051) and model.classifier.out_features == 16
    res = json.load(open(os.path.join(out, "pretrain_eval_step_2.json")))
    assert res["pretrain"] == "barlow" and res["pairs"] == 4 and res["lambda"] == pytest.approx(0.0051) and set(res["loss"]) == {"barlow"}
    assert math.isfinite(res["loss"]["barlow"]) and res["loss"]["barlow"] > 0
    assert res["loss"]["barlow"] == pytest.approx(res["on_diag"] + res["lambda"] * res["off_diag"], rel=1e-5)
    assert -1.0 <= res["mean_diag"] <= 1.0 + 1e-3
    assert "Evaluate Barlow Twins pretraining @ step 2" in text
    assert not [f for f in os.listdir(out) if f.startswith("eval_results")]          # nothing a --plot_roc would read as AUROCs
    ck = torch.load(os.path.join(out, "checkpoint_latest.pt"), map_location="cpu")
    assert ck["pretrain"] == "barlow" and ck["global_step"] == 2
    assert ck["eval_loss"] == pytest.approx(res["loss"]["barlow"]) and ck["avg_auc"] == -ck["eval_loss"]
    assert ck["loss_state"]["kind"] == "barlow" and ck["loss_state"]["lambd"] == pytest.approx(0.0051)
    assert tuple(ck["state_dict"]["classifier.weight"].shape) == (16, 1024)
    best = torch.load(os.path.join(out, "best_checkpoints", "checkpoint_0.pt"), map_location="cpu")
    assert best["pretrain"] == "barlow" and best["eval_loss"] == ck["eval_loss"]


def test_cli_restore_continues_and_is_refused_into_other_runs(dev, pretrain_run, tmp_path, capsys):
    from chexpert_amd import cli
    out, _, _ = pretrain_run
    path = os.path.join(out, "checkpoint_latest.pt")
    with pytest.raises(ValueError, match="--init_backbone"):
        cli.main(_CLI + ["--fused_optimizer", "--restore", path, "--output_dir", str(tmp_path / "s")])
    with pytest.raises(ValueError, match="one of --pretrain barlow, this run is --pretrain contrastive"):
        cli.main(_CLI + ["--pretrain", "contrastive", "--proj_dim", "16", "--jitter", "--fused_optimizer", "--restore", path,
                         "--output_dir", str(tmp_path / "w")])
    # the stored lambda stays where --barlow_lambda is not given
    ck = torch.load(path, map_location="cpu")
    ck["loss_state"]["lambd"] = 0.02
    torch.save(ck, str(tmp_path / "moved.pt"))
    shutil.copy(os.path.join(out, "optim_checkpoint_latest.pt"), str(tmp_path / "optim_moved.pt"))       # (what --restore reads beside it)
    capsys.readouterr()
    model = cli.main(_CLI + _PRE + ["--fused_optimizer", "--restore", str(tmp_path / "moved.pt"), "--output_dir", str(tmp_path / "c")])
    lines = _lines(capsys.readouterr().out)
    assert [l["step"] for l in lines] == [3, 4] and all(math.isfinite(l["train_loss"]) and "on_diag" in l for l in lines)
    assert model.loss_kind == "barlow" and model.loss_lambda.item() == pytest.approx(0.02)
    assert json.load(open(str(tmp_path / "c" / "pretrain_eval_step_4.json")))["lambda"] == pytest.approx(0.02)


def test_cli_init_backbone_starts_a_supervised_run(dev, pretrain_run, tmp_path, capsys):
    from chexpert_amd import cli
    out, _, _ = pretrain_run
    path = os.path.join(out, "checkpoint_latest.pt")
    capsys.readouterr()
    model = cli.main(_CLI + ["--fused_optimizer", "--init_backbone", path, "--output_dir", str(tmp_path / "f")])
    text = capsys.readouterr().out
    lines = _lines(text)
    assert [l["step"] for l in lines] == [1, 2] and all(math.isfinite(l["train_loss"]) for l in lines) and "on_diag" not in lines[0]
    assert model.loss_kind == "bce" and model.classifier.out_features == 5 and "tensors loaded" in text
    new = torch.load(str(tmp_path / "f" / "checkpoint_latest.pt"), map_location="cpu")
    assert new["global_step"] == 2 and "pretrain" not in new


def test_cli_autograd_route_is_the_same_kernels(dev, pretrain_run, tmp_path, capsys):
    """Without --fused_optimizer the step is model(x) -> BarlowTwinsLoss -> backward() under torch's optimiser: the first minibatch
    (same seed, same views, same initial weights) gives the fused run's loss bit for bit."""
    from chexpert_amd import cli
    _, _, text = pretrain_run
    capsys.readouterr()
    model = cli.main(_CLI + _PRE + ["--barlow_lambda", "0.0051", "--output_dir", str(tmp_path / "a")])
    lines = _lines(capsys.readouterr().out)
    assert [l["step"] for l in lines] == [1, 2] and lines[0]["train_loss"] == _lines(text)[0]["train_loss"]
    assert lines[0]["on_diag"] == _lines(text)[0]["on_diag"] and math.isfinite(lines[1]["train_loss"])
    assert model.loss_kind == "barlow" and os.path.exists(str(tmp_path / "a" / "pretrain_eval_step_2.json"))
