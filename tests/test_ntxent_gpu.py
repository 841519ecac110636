"""Contrastive pretraining on the GPU: cx_ntxent_fwd_bwd against the float64 statement (loss.reference_ntxent) within the rounding
bound test_ntxent_cpu derives, its reproducibility and edge cases, the fused step against the autograd route, the captured step, SAM,
and the command line (--pretrain contrastive, --init_backbone)."""
import json
import math
import os

import numpy as np
import pytest
import torch

from chexpert_amd import synth
from eager_step import _eager_dev_step
from test_ntxent_cpu import LAYOUTS, SHAPES, TAUS, case, check_against, tolerance

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def dev():
    from chexpert_amd import _lib
    _lib.lib()
    return torch.device("cuda:0")


def run(dev, e, ids, tau, outputs="legt", grad_scale=1.0, scratch=None):
    """One call of ops.ntxent_fwd_bwd with the outputs named in `outputs` (l loss, e element losses, g gradient, t top1), each
    prefilled with a value the kernels never write.  Returns them (None where not asked for) as device tensors."""
    from chexpert_amd import ops
    x = torch.as_tensor(e, dtype=torch.float32).to(dev).contiguous()
    g = torch.as_tensor(np.asarray(ids), dtype=torch.float32).reshape(-1, 1).to(dev)
    t = torch.tensor([tau], dtype=torch.float32, device=dev)
    N, d = x.shape
    loss = torch.full((1,), 777.0, device=dev) if "l" in outputs else None
    elem = torch.full((N, 1), 777.0, device=dev) if "e" in outputs else None
    grad = torch.full((N, d), 777.0, device=dev) if "g" in outputs else None
    top = torch.full((N,), 777, dtype=torch.int32, device=dev) if "t" in outputs else None
    ops.ntxent_fwd_bwd(x, g, t, loss, elem, grad, top, scratch, grad_scale)
    return loss, elem, grad, top


def _np(*tensors):
    return [None if t is None else t.cpu().numpy() for t in tensors]


@pytest.mark.parametrize("tau", TAUS)
@pytest.mark.parametrize("N,d", SHAPES)
def test_kernel_against_float64(dev, N, d, tau):
    """Loss, element losses, gradient and nearest row against the float64 statement, for every id layout.  The tolerance is
    test_ntxent_cpu.tolerance: with u = 2^-24, eps_s = (2 d + 9) u / tau on a similarity, eta = 2 eps_s + (ceil(N / 256) + 12) u
    (2 / tau + log N + 1) on an element loss, eta + 4 u (2 / tau + log N) on the loss, and on the 2-norm of gradient row i
    W_i / (|e_i| tau M) (eta + (N + 3 d + 27) u) with W_i the absolute mass of the row's coefficients; top1 is compared on the rows
    whose two best float64 scores differ by more than 2 eps_s (test_ntxent_cpu asserts these are at least 95 % of every case)."""
    from chexpert_amd.loss import reference_ntxent
    for layout in LAYOUTS:
        e, ids = case(N, d, layout)
        ref = reference_ntxent(e, ids, tau)
        tol = tolerance(e, ids, tau, ref)
        loss, elem, grad, top = _np(*run(dev, e, ids, tau))
        worst = check_against(ref, tol, loss[0], elem, grad, top, (N, d, tau, layout))
        print("N %d d %d tau %g %-8s loss %.6f (ref %.6f)  elem err %.2e of %.2e  grad err / tol %.3f"
              % (N, d, tau, layout, loss[0], ref["loss"], worst[0], tol["elem"], worst[1]))
        assert np.all(elem.reshape(-1)[~ref["anchors"]] == 0) and np.all(grad[np.asarray(ids) < 0] == 0)
    # grad_scale multiplies the gradient alone
    l3, e3, g3, _ = run(dev, e, ids, tau, grad_scale=3.0)
    assert np.array_equal(l3.cpu().numpy(), loss) and np.array_equal(e3.cpu().numpy(), elem)
    assert np.allclose(g3.cpu().numpy(), 3.0 * grad, rtol=4 * 2.0 ** -24, atol=0)


@pytest.mark.parametrize("N,d", [(6, 16), (65, 128), (130, 136), (512, 128)])
def test_two_launches_give_equal_bits_and_each_output_alone_its_own(dev, N, d):
    e, ids = case(N, d, "negative")
    first = run(dev, e, ids, 0.05)
    again = run(dev, e, ids, 0.05)
    for a, b in zip(first, again):
        assert torch.equal(a, b)
    for k, name in enumerate("legt"):
        alone = run(dev, e, ids, 0.05, outputs=name)
        assert [o is not None for o in alone] == [i == k for i in range(4)]
        assert torch.equal(alone[k], first[k]), name
    pair = run(dev, e, ids, 0.05, outputs="lt")
    assert torch.equal(pair[0], first[0]) and torch.equal(pair[3], first[3]) and pair[1] is None and pair[2] is None
    # a caller's scratch, larger than needed, and the kernels' own give the same bits
    from chexpert_amd import ops
    big = torch.full((ops.ntxent_scratch(N, d) + 100,), float("nan"), device=dev)
    held = run(dev, e, ids, 0.05, scratch=big)
    for a, b in zip(first, held):
        assert torch.equal(a, b)
    assert torch.isnan(big[-100:]).all()


@pytest.mark.parametrize("scale", [1e4, 1e-20])
def test_small_temperature_with_duplicates_and_extreme_scales(dev, scale):
    """tau = 0.01, every row once more as an exact duplicate (s = 100 at the maximum), embeddings times 1e4 and times 1e-20: finite,
    and the float64 statement's.  At 1e-20 every norm is below the clamp 1e-12: z = e / 1e-12 and the gradient is dz / 1e-12."""
    from chexpert_amd.loss import reference_ntxent
    half, ids_half = case(12, 16, "pairs")
    e = (np.concatenate([half, half]).astype(np.float64) * scale).astype(np.float32)
    ids = np.concatenate([ids_half, ids_half])
    ref = reference_ntxent(e, ids, 0.01)
    tol = tolerance(e, ids, 0.01, ref)
    loss, elem, grad, top = _np(*run(dev, e, ids, 0.01))
    assert np.isfinite(loss).all() and np.isfinite(elem).all() and np.isfinite(grad).all() and ref["loss"] > 0
    check_against(ref, tol, loss[0], elem, grad, top, scale)
    assert np.abs(grad).max() > 0
    if scale < 1:
        assert np.sqrt((e.astype(np.float64) ** 2).sum(1)).max() < 1e-12
    # the duplicate of a row is its nearest row wherever that is decided; it stands 12 rows further on, so rows 12.. find it first
    assert np.array_equal(top[12:][tol["top1"][12:]], np.arange(12)[tol["top1"][12:]])


def test_a_row_outside_the_batch_touches_nothing(dev):
    e, ids = case(65, 128, "negative")
    out = np.flatnonzero(ids < 0)
    first = run(dev, e, ids, 0.05)
    assert not first[2][out].any() and not first[1][out].any() and (first[3][out] == -1).all()
    moved = e.copy()
    moved[out] = moved[out] * -37.5 + 4.0
    second = run(dev, moved, ids, 0.05)
    for a, b in zip(first, second):
        assert torch.equal(a, b)
    # teeth: the same change to a row INSIDE the batch is seen
    inside = e.copy()
    inside[0] = inside[0] * -37.5 + 4.0
    assert not torch.equal(run(dev, inside, ids, 0.05)[2], first[2])


def test_no_anchor_gives_exact_zeros(dev):
    e, _ = case(6, 16, "pairs")
    for ids in (np.arange(6), np.array([-1, -1, -1, -1, -1, -1.0]), np.array([0, -1, -1, -1, -1, -1.0])):
        loss, elem, grad, top = _np(*run(dev, e, ids, 0.2))
        assert loss[0] == 0 and not elem.any() and not grad.any()
        want = -1 if (ids >= 0).sum() < 2 else None
        assert np.all(top == -1) if want == -1 else np.all(top >= 0)
    loss, elem, grad, top = _np(*run(dev, e[:1], np.zeros(1), 0.2))
    assert loss[0] == 0 and not elem.any() and not grad.any() and top.tolist() == [-1]
    loss, elem, grad, top = _np(*run(dev, e[:2], np.zeros(2), 0.2))             # one pair: log 1
    assert loss[0] == 0 and not elem.any() and top.tolist() == [1, 0] and not grad.any()


def test_top1_ties_and_the_accuracy_figure(dev):
    from chexpert_amd.loss import contrastive_top1
    e = np.array([[1.0, 0.0], [0.0, 1.0], [0.0, 1.0], [1.0, 0.0], [1.0, 0.0]], dtype=np.float32)
    ids = np.array([0, 1, 1, 0, 2.0])
    assert run(dev, e, ids, 0.5, outputs="t")[3].tolist() == [3, 2, 1, 0, 0]
    x, g = torch.tensor(e, device=dev), torch.tensor(ids, dtype=torch.float32, device=dev)
    assert contrastive_top1(x, g) == 1.0 and contrastive_top1(x, g.reshape(-1, 1), return_counts=True) == (4, 4)
    swapped = torch.tensor([0, 1, 0, 1, 2.0], device=dev)                          # every nearest row is now a negative
    assert contrastive_top1(x, swapped) == 0.0
    assert math.isnan(contrastive_top1(x, torch.arange(5, dtype=torch.float32, device=dev)))
    big, ids_big = case(130, 136, "negative")
    from chexpert_amd.loss import reference_ntxent
    ref = reference_ntxent(big, ids_big, 1.0)
    decided = tolerance(big, ids_big, 1.0, ref)["top1"]                              # (contrastive_top1 ranks at temperature 1)
    hit = ref["anchors"] & (ids_big[np.maximum(ref["top1"], 0)] == ids_big)
    sure, open_rows = int((hit & decided).sum()), int((ref["anchors"] & ~decided).sum())
    got = contrastive_top1(torch.tensor(big, device=dev), torch.tensor(ids_big, dtype=torch.float32, device=dev), return_counts=True)
    # exact on the rows whose nearest row is decided within the rounding bound; only an undecided anchor may count either way
    assert got[1] == int(ref["anchors"].sum()) and sure <= got[0] <= sure + open_rows and open_rows <= 0.05 * len(ids_big)


def test_wrapper_refusals(dev):
    from chexpert_amd import ops
    from chexpert_amd.loss import NTXentLoss
    x, g, t = torch.zeros(4, 8, device=dev), torch.zeros(4, 1, device=dev), torch.ones(1, device=dev)
    with pytest.raises(AssertionError):
        ops.ntxent_fwd_bwd(x, g, t, None, None, None, scratch=torch.zeros(8, device=dev))
    with pytest.raises(AssertionError):
        ops.ntxent_fwd_bwd(x, g, t, None, None, None, top1=torch.zeros(4, dtype=torch.int64, device=dev))
    with pytest.raises(ValueError):
        ops.ntxent_fwd_bwd(torch.zeros(4, 2000, device=dev), g, t, None, None, None)
    with pytest.raises(RuntimeError, match=r"\(N, 1\) column of ids"):
        NTXentLoss()(x, torch.zeros(4, 8, device=dev))
    with pytest.raises(AssertionError):                                            # an operand on another device
        ops.ntxent_fwd_bwd(x, g, torch.ones(1), None, None, None)


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
    table = [[0, 1, 2, 3, 0, 1, 2, 3], [0, 0, 0, 1, 2, 1, -1, 3], [5, 5, 6, 6, 7, 7, 8, 8], [0, 1, 2, -1, 0, 1, 2, 9]][which]
    return torch.tensor(table[:B], dtype=torch.float32, device=dev).reshape(-1, 1)


@pytest.mark.parametrize("train", [True, False])
def test_fused_step_equals_the_autograd_route(dev, train):
    from chexpert_amd import ops
    from chexpert_amd.loss import MaskedBCE, NTXentLoss, reference_ntxent
    a, b, S = _twin(dev)
    a.train(train), b.train(train)
    B = 8
    x = synth.xray_batch(4500, B, S).to(dev)
    t = _ids(dev, B, 1)
    keys = list(a.state_dict().keys())
    assert a.set_loss(kind="ntxent", temperature=0.1) is a
    crit = NTXentLoss(0.1)
    assert list(a.state_dict().keys()) == keys and a.loss_step_state() == []
    assert a.loss_kind == "ntxent" and a.loss_ignore_negative is False and a.loss_pos_weight is None and a.loss_focus is None
    tau = a.loss_temperature
    assert tau.is_cuda and tuple(tau.shape) == (1,) and tau.item() == pytest.approx(0.1)
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
    # the loss is the float64 statement's on these logits, and so are the element losses outside autograd
    ref = reference_ntxent(logits_a.cpu().numpy(), t.cpu().numpy(), 0.1)
    tol = tolerance(logits_a.cpu().numpy(), t.cpu().numpy().reshape(-1), 0.1, ref)
    print("train %s: fused loss %.7f, float64 statement %.7f" % (train, loss_a.item(), ref["loss"]))
    assert abs(loss_a.item() - ref["loss"]) <= tol["loss"] and ref["loss"] > 0
    le = crit.elementwise(out, t)
    assert not le.requires_grad and tuple(le.shape) == (B, 1)
    assert np.abs(le.cpu().numpy().reshape(-1) - ref["loss_elem"]).max() <= tol["elem"]
    # backward scales by the incoming gradient
    xl = logits_a.clone().requires_grad_(True)
    (3.0 * crit(xl, t)).backward()
    dl = torch.empty_like(logits_a)
    ops.ntxent_fwd_bwd(logits_a, t, a.loss_temperature, None, None, dl)
    assert torch.equal(xl.grad, dl * 3.0)
    # teeth: another temperature is another gradient
    other = torch.empty_like(dl)
    ops.ntxent_fwd_bwd(logits_a, t, torch.tensor([0.2], device=dev), None, None, other)
    assert not torch.equal(other, dl)
    with pytest.raises(RuntimeError, match="column of ids"):
        crit(out, t.reshape(-1))
    with pytest.raises(RuntimeError):
        MaskedBCE()(out, t)


def test_set_loss_walk_leaves_nothing_of_the_previous_kind(dev):
    """asl (weights) -> ntxent -> ntxent (another temperature: the held storage) -> hier -> ntxent -> bce: after every move the public
    attributes are the new kind's alone, a refused call changes nothing, and loss_state() round-trips."""
    model, S = _net(dev)
    other, _ = _net(dev)
    pw = synth.uniform(4730, (D,), 0.5, 8.0)
    bce_state = {"kind": "bce", "aux": None, "prior": None, "margin": 1.0, "lr_aux": None}
    model.set_loss(kind="asl", pos_weight=pw)
    assert model.loss_temperature is None and model.loss_focus is not None
    model.set_loss(kind="ntxent")
    held = model.loss_temperature.data_ptr()
    assert model.loss_kind == "ntxent" and model.loss_temperature.item() == pytest.approx(0.2)
    for name in ("loss_pos_weight", "loss_focus", "loss_aux", "loss_prior", "loss_lr_aux", "loss_class_weight", "loss_parent", "loss_mode"):
        assert getattr(model, name) is None, name
    assert model.loss_ignore_negative is False
    model.set_loss(kind="ntxent", temperature=0.07)
    assert model.loss_temperature.data_ptr() == held and model.loss_temperature.item() == pytest.approx(0.07)
    st = model.loss_state()
    assert st["kind"] == "ntxent" and st["temperature"] == pytest.approx(0.07) and "focus" not in st and "parent" not in st
    assert other.load_loss_state(st) is other and other.loss_kind == "ntxent" and other.loss_temperature.item() == pytest.approx(0.07)
    assert other.loss_state() == st
    for kw in (dict(kind="ntxent", pos_weight=pw), dict(kind="ntxent", ignore_negative=True), dict(kind="ntxent", temperature=0.0),
               dict(kind="ntxent", gamma=1.0), dict(kind="ntxent", parent=[-1] * D), dict(kind="asl", temperature=0.3)):
        with pytest.raises(ValueError):
            model.set_loss(**kw)
        assert model.loss_kind == "ntxent" and model.loss_temperature.item() == pytest.approx(0.07) and model.loss_pos_weight is None
    model.set_loss(kind="hier", parent=[-1] * D)
    assert model.loss_temperature is None and model.loss_parent is not None and "temperature" not in model.loss_state()
    model.set_loss(kind="ntxent", temperature=0.5)
    assert model.loss_temperature.data_ptr() == held and model.loss_parent is None and model.loss_mode is None
    x, t = synth.xray_batch(4700, 8, S).to(dev), _ids(dev)
    loss, logits = model.forward_backward(x, t)
    from chexpert_amd.loss import NTXentLoss
    assert torch.equal(NTXentLoss(0.5)(logits, t), loss.reshape(())) and math.isfinite(loss.item()) and loss.item() > 0
    assert model.set_loss() is model and model.loss_temperature is None and model.loss_state() == bce_state


def test_graphed_step_equals_eager_and_sees_the_temperature_rewritten_in_place(dev):
    """Three replays of GraphedTrainStep over FusedAdam against three eager train_step(dev=True) calls on a twin, bit for bit; the
    temperature rewritten in place before a fourth; the scratch was sized by the warm-up runs, so the capture allocated none."""
    from chexpert_amd.graph import GraphedTrainStep
    from chexpert_amd.loss import NTXentLoss
    from chexpert_amd.optim import FusedAdam
    m_e, m_g, S = _twin(dev)
    B = 8
    xs = [synth.xray_batch(4800 + i, B, S).to(dev) for i in range(5)]
    ts = [_ids(dev, B, i % 4) for i in range(5)]
    for m in (m_e, m_g):
        m.set_loss(kind="ntxent", temperature=0.2)
    opt_e, opt_g = FusedAdam(m_e, lr=1e-3), FusedAdam(m_g, lr=1e-3)
    gs = GraphedTrainStep(m_g, opt_g, xs[0], ts[2])
    scratch = m_g._loss._held["scratch"]
    held, where = m_g.loss_temperature.data_ptr(), scratch.data_ptr()
    flat = lambda m: torch.cat([p.detach().flatten() for p in m.parameters()])                               # noqa: E731
    for i in range(3):
        le, _ = opt_e.train_step(m_e, xs[i], ts[i], dev=True)
        lg, logits = gs.replay(xs[i], ts[i])
        assert tuple(logits.shape) == (B, D) and torch.equal(le.reshape(-1), lg.reshape(-1)), (i, le.item(), lg.item())
        assert torch.equal(flat(m_e), flat(m_g)), i
        assert torch.equal(m_e._eng().flat_grad, m_g._eng().flat_grad)
    # the independent statement of the step agrees as well
    le = _eager_dev_step(m_e, opt_e, xs[3], ts[3])
    lg, _ = gs.replay(xs[3], ts[3])
    assert torch.equal(le.reshape(-1), lg.reshape(-1)) and torch.equal(flat(m_e), flat(m_g))
    # the temperature changes in place: the next replay reads it
    m_g.loss_temperature.fill_(0.05)
    m_e.set_loss(kind="ntxent", temperature=0.05)
    assert m_g.loss_temperature.data_ptr() == held
    le = _eager_dev_step(m_e, opt_e, xs[4], ts[4])
    lg, logits = gs.replay(xs[4], ts[4])
    assert torch.equal(le.reshape(-1), lg.reshape(-1)) and torch.equal(flat(m_e), flat(m_g))
    assert NTXentLoss(0.2)(logits, ts[4]).item() != lg.item() == NTXentLoss(0.05)(logits, ts[4]).item()
    assert m_g._loss._held["scratch"] is scratch and scratch.data_ptr() == where


def test_a_missing_scratch_under_capture_is_an_error_not_an_allocation(dev, monkeypatch):
    from chexpert_amd.loss import Loss
    state = Loss("ntxent", temperature=torch.tensor([0.2], device=dev))
    z, t = torch.randn(8, D, device=dev), _ids(dev)
    loss, dl = torch.empty(1, device=dev), torch.empty(8, D, device=dev)
    monkeypatch.setattr(torch.cuda, "is_current_stream_capturing", lambda: True)
    with pytest.raises(RuntimeError, match="under a graph capture"):
        state.launch(z, t, loss, None, dl)
    assert "scratch" not in state._held
    monkeypatch.undo()
    state.launch(z, t, loss, None, dl)                                  # sized outside capture ...
    held = state._held["scratch"]
    monkeypatch.setattr(torch.cuda, "is_current_stream_capturing", lambda: True)
    state.launch(z[:4].contiguous(), t[:4].contiguous(), loss, None, dl[:4])      # ... a step that fits uses it as it is
    assert state._held["scratch"] is held


def test_one_sam_step_runs(dev):
    from chexpert_amd.optim import FusedAdam, FusedSAM
    m, S = _net(dev)
    m.set_loss(kind="ntxent", temperature=0.2)
    s = FusedSAM(FusedAdam(m, lr=1e-3), rho=0.05)
    before = torch.cat([p.detach().flatten() for p in m.parameters()]).clone()
    loss, logits = s.train_step(m, synth.xray_batch(4900, 8, S).to(dev), _ids(dev))
    assert math.isfinite(float(loss)) and float(loss) > 0 and tuple(logits.shape) == (8, D)
    after = torch.cat([p.detach().flatten() for p in m.parameters()])
    assert torch.isfinite(after).all() and not torch.equal(before, after)


# ------------------------------------------------------------------------------------------------ the command line
_CLI = ["--train", "--synthetic", "8", "--batch_size", "4", "--resize", "64", "--eval_interval", "2", "--log_interval", "1", "--seed", "3",
        "--lr", "0.001"]
_PRE = ["--pretrain", "contrastive", "--proj_dim", "16", "--affine", "--jitter"]


def _lines(text):
    return [json.loads(l) for l in text.splitlines() if l.startswith('{"step"')]


@pytest.fixture(scope="module")
def pretrain_run(dev, tmp_path_factory):
    """One `--pretrain contrastive --affine --jitter --fused_optimizer --graph` run of two steps with an evaluation after the second,
    shared by the tests below: (output folder, model, its stdout)."""
    import contextlib
    import io
    from chexpert_amd import cli
    out = str(tmp_path_factory.mktemp("ntxent") / "p")
    buf = io.StringIO()
    with contextlib.redirect_stdout(buf):
        model = cli.main(_CLI + _PRE + ["--fused_optimizer", "--graph", "--output_dir", out])
    return out, model, buf.getvalue()


def test_cli_pretraining_writes_the_json_and_the_checkpoint(dev, pretrain_run):
    out, model, text = pretrain_run
    lines = _lines(text)
    assert [l["step"] for l in lines] == [1, 2] and all(math.isfinite(l["train_loss"]) and l["train_loss"] > 0 for l in lines)
    assert all(0.0 <= l["top1"] <= 1.0 for l in lines)
    assert model.loss_kind == "ntxent" and model.loss_temperature.item() == pytest.approx(0.2) and model.classifier.out_features == 16
    res = json.load(open(os.path.join(out, "pretrain_eval_step_2.json")))
    assert res["pretrain"] == "contrastive" and res["anchors"] == 8 and 0.0 <= res["top1"] <= 1.0 and res["positive"] == "view"
    assert math.isfinite(res["loss"]["contrastive"]) and res["loss"]["contrastive"] > 0 and res["temperature"] == pytest.approx(0.2)
    assert "Evaluate contrastive pretraining @ step 2" in text
    assert not [f for f in os.listdir(out) if f.startswith("eval_results")]          # nothing a --plot_roc would read as AUROCs
    ck = torch.load(os.path.join(out, "checkpoint_latest.pt"), map_location="cpu")
    assert ck["pretrain"] == "contrastive" and ck["global_step"] == 2
    assert ck["eval_loss"] == pytest.approx(res["loss"]["contrastive"]) and ck["avg_auc"] == -ck["eval_loss"]
    assert ck["loss_state"]["kind"] == "ntxent" and ck["loss_state"]["temperature"] == pytest.approx(0.2) and ck["loss_state"]["positive"] == "view"
    assert tuple(ck["state_dict"]["classifier.weight"].shape) == (16, 1024)
    best = torch.load(os.path.join(out, "best_checkpoints", "checkpoint_0.pt"), map_location="cpu")
    assert best["pretrain"] == "contrastive" and best["eval_loss"] == ck["eval_loss"]


def test_cli_init_backbone_starts_a_supervised_run_from_the_pretrained_backbone(dev, pretrain_run, tmp_path, capsys, monkeypatch):
    from chexpert_amd import cli
    out, _, _ = pretrain_run
    path = os.path.join(out, "checkpoint_latest.pt")
    ck = torch.load(path, map_location="cpu")
    seen = {}
    train = cli.train

    def spy(run):                                                       # the model as the first step finds it
        seen.update({k: v.detach().cpu().clone() for k, v in run.model.state_dict().items()})
        return train(run)
    monkeypatch.setattr(cli, "train", spy)
    capsys.readouterr()
    model = cli.main(_CLI + ["--fused_optimizer", "--init_backbone", path, "--output_dir", str(tmp_path / "f")])
    text = capsys.readouterr().out
    lines = _lines(text)
    assert [l["step"] for l in lines] == [1, 2] and all(math.isfinite(l["train_loss"]) for l in lines) and "top1" not in lines[0]
    assert model.loss_kind == "bce" and model.classifier.out_features == 5
    head = {"classifier.weight", "classifier.bias"}
    assert set(seen) == set(ck["state_dict"]) and head <= set(seen)
    for k, v in ck["state_dict"].items():
        if k not in head:
            assert torch.equal(seen[k], v), k
    assert any(k.endswith("running_mean") for k in seen) and any(k.endswith("num_batches_tracked") for k in seen)
    assert tuple(seen["classifier.weight"].shape) == (5, 1024) and not seen["classifier.bias"].any() and seen["classifier.weight"].abs().max() > 0
    new = torch.load(str(tmp_path / "f" / "checkpoint_latest.pt"), map_location="cpu")
    assert new["global_step"] == 2 and "pretrain" not in new and "tensors loaded" in text
    # a missing backbone tensor is an error that names it
    broken = {k: v for k, v in ck["state_dict"].items() if k != "features.norm5.weight"}
    torch.save(dict(ck, state_dict=broken), str(tmp_path / "broken.pt"))
    with pytest.raises(ValueError, match="features.norm5.weight"):
        cli.main(_CLI + ["--fused_optimizer", "--init_backbone", str(tmp_path / "broken.pt"), "--output_dir", str(tmp_path / "g")])


def test_cli_restore_continues_pretraining_and_is_refused_into_a_supervised_run(dev, pretrain_run, tmp_path, capsys):
    from chexpert_amd import cli
    out, _, _ = pretrain_run
    path = os.path.join(out, "checkpoint_latest.pt")
    with pytest.raises(ValueError, match="--init_backbone"):
        cli.main(_CLI + ["--fused_optimizer", "--restore", path, "--output_dir", str(tmp_path / "s")])
    with pytest.raises(ValueError, match="--proj_dim asks for 32"):
        cli.main(_CLI + ["--pretrain", "contrastive", "--proj_dim", "32", "--jitter", "--fused_optimizer", "--restore", path,
                         "--output_dir", str(tmp_path / "w")])
    capsys.readouterr()
    # the eager fused route continues it; the stored temperature stays where --temperature is not given
    model = cli.main(_CLI + _PRE + ["--fused_optimizer", "--restore", path, "--output_dir", str(tmp_path / "c")])
    lines = _lines(capsys.readouterr().out)
    assert [l["step"] for l in lines] == [3, 4] and all(math.isfinite(l["train_loss"]) and "top1" in l for l in lines)
    assert model.loss_kind == "ntxent" and model.loss_temperature.item() == pytest.approx(0.2)
    assert os.path.exists(str(tmp_path / "c" / "pretrain_eval_step_4.json"))


def test_cli_autograd_route_is_the_same_kernels(dev, pretrain_run, tmp_path, capsys):
    """Without --fused_optimizer the step is model(x) -> NTXentLoss -> backward() under torch's optimiser: the first minibatch (same
    seed, same views, same initial weights) gives the fused run's loss bit for bit."""
    from chexpert_amd import cli
    _, _, text = pretrain_run
    capsys.readouterr()
    model = cli.main(_CLI + _PRE + ["--temperature", "0.2", "--output_dir", str(tmp_path / "a")])
    lines = _lines(capsys.readouterr().out)
    assert [l["step"] for l in lines] == [1, 2] and lines[0]["train_loss"] == _lines(text)[0]["train_loss"]
    assert lines[0]["top1"] == _lines(text)[0]["top1"] and math.isfinite(lines[1]["train_loss"])
    assert model.loss_kind == "ntxent" and os.path.exists(str(tmp_path / "a" / "pretrain_eval_step_2.json"))
