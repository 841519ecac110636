"""GPU: ignored (-1) labels and class-weighted BCE -- cx_bce_masked_fwd_bwd against a float64 torch statement, its bit identity
with cx_bce_fwd_bwd, FusedNet.set_loss in the fused step, under graph replay and data-parallel, and the command line."""
import json
import math
import os
import time

import pytest
import torch
import torch.nn.functional as F

from chexpert_amd import synth
from eager_step import _eager_dev_step

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    from chexpert_amd import _lib
    _lib.lib()          # fail loudly if the HIP library is missing
    return torch.device("cuda:0")


def close(got, want, rel, what=""):
    """The bound of tests/test_kernels_gpu.py: max error against the largest reference magnitude."""
    scale = want.abs().max().item() + 1e-6
    err = (got - want).abs().max().item()
    print("%s: max err %.3e vs scale %.3e (rel %.2e)" % (what, err, scale, err / scale))
    assert err <= rel * scale, "%s: max err %.3e vs scale %.3e (rel %.2e)" % (what, err, scale, err / scale)


def _targets(seed, B, n, ignored=0.2, soft=0.15):
    """Hard Bernoulli(0.3) labels, a share `soft` of them replaced by values uniform in [0, 1], a share `ignored` by -1."""
    t = synth.targets(seed, B, n).clone()
    u = synth.uniform(seed + 1, (B, n), 0.0, 1.0)
    t = torch.where(synth.uniform(seed + 2, (B, n), 0.0, 1.0) < soft, u, t)
    return torch.where(synth.uniform(seed + 3, (B, n), 0.0, 1.0) < ignored, torch.full_like(t, -1.0), t)


def _statement(logits, t, pw):
    """float64: BCEWithLogitsLoss(reduction='none', pos_weight) on clamped targets, times (t >= 0), .sum(1).mean(0); autograd."""
    x = logits.double().requires_grad_(True)
    le = F.binary_cross_entropy_with_logits(x, t.double().clamp(min=0), reduction="none", pos_weight=pw.double()) * (t >= 0).double()
    loss = le.sum(1).mean(0)
    loss.backward()
    return loss.detach(), le.detach(), x.grad


@pytest.mark.parametrize("n", [5, 14])
@pytest.mark.parametrize("B", [1, 3, 256])
def test_masked_bce_kernel_against_float64(dev, B, n):
    from chexpert_amd import ops
    seed = 1000 + 10 * B + n
    logits = synth.uniform(seed, (B, n), -8.0, 8.0)
    pw = synth.uniform(seed + 5, (n,), 0.5, 8.0)
    t = _targets(seed + 10, B, n)
    if B == 256:
        assert (t < 0).any() and ((t > 0) & (t < 1)).any() and (t == 1).any() and (t == 0).any()
    loss_ref, le_ref, g_ref = _statement(logits, t, pw)
    xd, td, pd = logits.to(dev), t.to(dev), pw.to(dev)
    loss, le, dl = torch.full((1,), 7.0, device=dev), torch.full((B, n), 7.0, device=dev), torch.full((B, n), 7.0, device=dev)
    ops.bce_masked_fwd_bwd(xd, td, pd, loss, le, dl)
    print("B=%d n=%d loss %.7f ref %.7f diff %.3e" % (B, n, loss.item(), loss_ref.item(), abs(loss.item() - loss_ref.item())))
    assert abs(loss.item() - loss_ref.item()) < 1e-5
    close(le.cpu().double(), le_ref, rel=1e-5, what="loss_elem")
    close(dl.cpu().double(), g_ref, rel=1e-5, what="dlogits")
    ign = (t < 0)
    assert bool((le.cpu()[ign] == 0.0).all()) and bool((dl.cpu()[ign] == 0.0).all())
    if (~ign).any():
        assert bool((le.cpu()[~ign] > 0).all())
    # each output is optional; the others do not move
    loss2, le2, dl2 = torch.zeros(1, device=dev), torch.zeros(B, n, device=dev), torch.zeros(B, n, device=dev)
    ops.bce_masked_fwd_bwd(xd, td, pd, loss2, None, dl2)
    assert torch.equal(loss2, loss) and torch.equal(dl2, dl)
    loss3 = torch.zeros(1, device=dev)
    ops.bce_masked_fwd_bwd(xd, td, pd, loss3, le2, None)
    assert torch.equal(loss3, loss) and torch.equal(le2, le)
    ops.bce_masked_fwd_bwd(xd, td, pd, None, None, dl2.zero_())
    assert torch.equal(dl2, dl)
    # grad_scale multiplies the gradient alone
    ops.bce_masked_fwd_bwd(xd, td, pd, loss2.zero_(), None, dl2, grad_scale=0.5)
    assert torch.equal(loss2, loss) and torch.equal(dl2, dl * 0.5)
    # without weights the statement holds too (pos_weight = 1), ignored elements included
    loss_ref1, le_ref1, g_ref1 = _statement(logits, t, torch.ones(n))
    ops.bce_masked_fwd_bwd(xd, td, None, loss2, le2, dl2)
    print("unweighted: loss %.7f ref %.7f diff %.3e" % (loss2.item(), loss_ref1.item(), abs(loss2.item() - loss_ref1.item())))
    assert abs(loss2.item() - loss_ref1.item()) < 1e-5
    close(le2.cpu().double(), le_ref1, rel=1e-5, what="loss_elem (no weights)")
    close(dl2.cpu().double(), g_ref1, rel=1e-5, what="dlogits (no weights)")
    assert bool((le2.cpu()[ign] == 0.0).all()) and bool((dl2.cpu()[ign] == 0.0).all())


def test_weighted_gradient_keeps_its_digits_on_confident_positives(dev):
    """Large positive logits on positive targets: d loss / dx = -w (1 - sigmoid(x)) / B is tiny against the largest gradient of a
    batch, so the bound relative to that maximum does not see it.  Held element by element: exp, one add, one divide and three
    multiplies are a few fp32 roundings (6e-8 each), far inside 1e-5 of the element's own value; 1 - 1 / (1 + exp(-x)) instead
    loses e^x of them (three digits left at x = 8)."""
    from chexpert_amd import ops
    B, n = 64, 5
    logits = synth.uniform(41, (B, n), 6.0, 16.0)
    t, pw = torch.ones(B, n), synth.uniform(42, (n,), 0.5, 8.0)
    _, _, g_ref = _statement(logits, t, pw)
    dl = torch.zeros(B, n, device=dev)
    ops.bce_masked_fwd_bwd(logits.to(dev), t.to(dev), pw.to(dev), None, None, dl)
    rel = ((dl.cpu().double() - g_ref).abs() / g_ref.abs()).max().item()
    print("weighted gradient on confident positives: max elementwise rel err %.3e" % rel)
    assert bool((g_ref != 0).all()) and rel < 1e-5


def test_loss_module_options_select_the_kernel(dev):
    """MaskedBCE(ignore_negative=False) without weights is the plain loss (a -1 is a number, as for BCEWithLogitsLoss); with
    ignore_negative, or with weights, a -1 is skipped."""
    from chexpert_amd import ops
    from chexpert_amd.loss import MaskedBCE
    B, n = 6, 5
    x = synth.uniform(43, (B, n), -8.0, 8.0).to(dev)
    t = _targets(44, B, n, ignored=0.4, soft=0.0).to(dev)
    ign = t < 0
    assert ign.any() and (~ign).any()
    loss, le, dl = torch.zeros(1, device=dev), torch.zeros(B, n, device=dev), torch.zeros(B, n, device=dev)
    ops.bce_fwd_bwd(x, t, loss, le, dl)
    plain = MaskedBCE(ignore_negative=False)
    xl = x.clone().requires_grad_(True)
    lp = plain(xl, t)
    lp.backward()
    assert torch.equal(lp.detach(), loss[0]) and torch.equal(xl.grad, dl) and torch.equal(plain.elementwise(x, t), le)
    assert bool((le[ign] != 0).all())
    ones = torch.ones(n, device=dev)
    for crit in (MaskedBCE(), MaskedBCE(ones, ignore_negative=False)):
        assert bool((crit.elementwise(x, t)[ign] == 0).all()) and crit(x, t).item() != lp.item()


@pytest.mark.parametrize("B,n", [(1, 5), (3, 5), (4, 14), (256, 5), (256, 14), (300, 14)])
def test_bit_identity_with_the_plain_kernel(dev, B, n):
    from chexpert_amd import ops
    logits = synth.uniform(50 + B + n, (B, n), -8.0, 8.0).to(dev)
    soft = synth.uniform(60 + B + n, (B, n), 0.0, 1.0)
    for t in (synth.targets(70 + B + n, B, n), torch.where(soft < 0.3, soft, synth.targets(71 + B + n, B, n))):
        t = t.to(dev)
        a = [torch.zeros(1, device=dev), torch.zeros(B, n, device=dev), torch.zeros(B, n, device=dev)]
        b = [torch.ones(1, device=dev), torch.ones(B, n, device=dev), torch.ones(B, n, device=dev)]
        for scale in (1.0, 0.37):
            ops.bce_fwd_bwd(logits, t, a[0], a[1], a[2], scale)
            ops.bce_masked_fwd_bwd(logits, t, None, b[0], b[1], b[2], scale)
            for u, v, what in zip(a, b, ("loss", "loss_elem", "dlogits")):
                assert torch.equal(u, v), what
        # and twice the same bits, weighted too
        w = synth.uniform(3, (n,), 0.5, 8.0).to(dev)
        c = [torch.ones(1, device=dev), torch.ones(B, n, device=dev), torch.ones(B, n, device=dev)]
        ops.bce_masked_fwd_bwd(logits, t, w, b[0], b[1], b[2])
        ops.bce_masked_fwd_bwd(logits, t, w, c[0], c[1], c[2])
        assert all(torch.equal(u, v) for u, v in zip(b, c))


@pytest.mark.parametrize("weighted", [False, True])
def test_all_ignored_batch(dev, weighted):
    from chexpert_amd import ops
    B, n = 7, 5
    logits = synth.uniform(5, (B, n), -8.0, 8.0).to(dev)
    t = torch.full((B, n), -1.0, device=dev)
    w = synth.uniform(6, (n,), 0.5, 8.0).to(dev) if weighted else None
    loss, le, dl = torch.full((1,), 7.0, device=dev), torch.full((B, n), 7.0, device=dev), torch.full((B, n), 7.0, device=dev)
    ops.bce_masked_fwd_bwd(logits, t, w, loss, le, dl)
    assert loss.item() == 0.0 and bool((le == 0).all()) and bool((dl == 0).all())
    assert not torch.isnan(loss).any() and not torch.isnan(dl).any()


def test_wrapper_checks_its_operands(dev):
    from chexpert_amd import ops
    x, t, w = torch.zeros(2, 5, device=dev), torch.zeros(2, 5, device=dev), torch.ones(5, device=dev)
    loss = torch.zeros(1, device=dev)
    with pytest.raises(RuntimeError):
        ops.bce_masked_fwd_bwd(x.cpu(), t, w, loss, None, None)
    with pytest.raises(RuntimeError):
        ops.bce_masked_fwd_bwd(x, t, w.cpu(), loss, None, None)
    with pytest.raises(AssertionError):
        ops.bce_masked_fwd_bwd(x, t.double(), w, loss, None, None)
    with pytest.raises(AssertionError):
        ops.bce_masked_fwd_bwd(x, t, torch.ones(4, device=dev), loss, None, None)
    with pytest.raises(AssertionError):
        ops.bce_masked_fwd_bwd(x.t(), t.t(), w, loss, None, None)
    with pytest.raises(AssertionError):
        ops.bce_masked_fwd_bwd(x, t, w, loss, None, torch.zeros(2, 4, device=dev))


# ------------------------------------------------------------------------------------------------ fused step
def _net(kind, dev, seed=3):
    from chexpert_amd.models import DenseNet, construct_model
    torch.manual_seed(seed)
    if kind == "densenet":
        model, S = DenseNet(32, (2, 2, 2, 2), 64, num_classes=5), 64
        for n_, p in model.named_parameters():           # well-conditioned regime (tests/test_model_gpu.py)
            if n_.endswith(".bias") and "classifier" not in n_:
                p.data.fill_(2.5)
    else:
        from chexpert_amd.models.efficientnet import DropMarker
        model, S = construct_model("efficientnet-b0", 5), 96
        for mod in model.modules():                      # two passes must see the same network: no dropout / DropConnect draws
            if isinstance(mod, DropMarker):
                mod.p = 0.0
    return model.to(dev).train(), S


def _twin(kind, dev):
    a, S = _net(kind, dev)
    b, _ = _net(kind, dev)
    b.load_state_dict({k: v.clone() for k, v in a.state_dict().items()})
    return a, b, S


@pytest.mark.parametrize("kind", ["densenet", "efficientnet"])
def test_fused_step_equals_the_autograd_route(dev, kind):
    from chexpert_amd.loss import MaskedBCE
    a, b, S = _twin(kind, dev)
    B = 4
    x = synth.xray_batch(500, B, S).to(dev)
    t = _targets(510, B, 5, ignored=0.25).to(dev)
    assert (t < 0).any() and (t >= 0).any()
    w = synth.uniform(520, (5,), 0.5, 8.0).to(dev)
    keys = list(a.state_dict().keys())
    assert a.set_loss(ignore_negative=True, pos_weight=w) is a
    assert list(a.state_dict().keys()) == keys                          # neither buffer nor parameter
    assert torch.equal(a.loss_pos_weight, w) and a.loss_pos_weight.data_ptr() != w.data_ptr()
    loss_a, logits_a = a.forward_backward(x, t)
    crit = MaskedBCE(w)
    out = b(x)
    loss_b = crit(out, t)
    loss_b.backward()
    assert loss_b.dim() == 0 and torch.equal(loss_a.reshape(()), loss_b.detach())
    assert torch.equal(logits_a, out.detach())
    ga, gb = dict(a.named_parameters()), dict(b.named_parameters())
    for k in ga:
        assert torch.equal(ga[k].grad, gb[k].grad), k
    assert max(float(p.grad.abs().max()) for p in ga.values()) > 0
    # the loss is the float64 statement's, and the element losses without a graph
    ref, le_ref, _ = _statement(logits_a.cpu(), t.cpu(), w.cpu())
    print("fused loss %.7f, float64 statement %.7f" % (loss_a.item(), ref.item()))
    assert abs(loss_a.item() - ref.item()) < 1e-5
    le = crit.elementwise(out, t)
    assert not le.requires_grad and tuple(le.shape) == (B, 5)
    close(le.cpu().double(), le_ref, rel=1e-5, what="elementwise")
    # backward scales by the incoming gradient
    xl = logits_a.clone().requires_grad_(True)
    (3.0 * crit(xl, t)).backward()
    dl = torch.empty_like(logits_a)
    from chexpert_amd import ops
    ops.bce_masked_fwd_bwd(logits_a, t, w, None, None, dl)
    assert torch.equal(xl.grad, dl * 3.0)
    # set_loss() puts the plain loss back: the step is the one of a model that never heard of it
    a.set_loss()
    a.zero_grad(set_to_none=True)
    b.zero_grad(set_to_none=True)
    t01 = synth.targets(530, B, 5).to(dev)
    la, _ = a.forward_backward(x, t01)
    lb, _ = b.forward_backward(x, t01)
    assert torch.equal(la, lb)
    for k in ga:
        assert torch.equal(ga[k].grad, gb[k].grad), k


def test_ignoring_has_teeth(dev):
    model, S = _net("densenet", dev)
    B, c = 4, 2
    x = synth.xray_batch(600, B, S).to(dev)
    t = synth.targets(610, B, 5).to(dev)
    t[:, c] = -1.0
    others = [k for k in range(5) if k != c]
    model.set_loss(ignore_negative=True)
    model.forward_backward(x, t)
    gw, gb = model.classifier.weight.grad, model.classifier.bias.grad
    assert bool((gw[c] == 0).all()) and gb[c].item() == 0.0
    assert all(float(gw[k].abs().max()) > 0 and gb[k].item() != 0.0 for k in others)
    model.set_loss()                                                    # the plain loss takes -1 for a number
    model.zero_grad(set_to_none=True)
    model.forward_backward(x, t)
    gw, gb = model.classifier.weight.grad, model.classifier.bias.grad
    assert float(gw[c].abs().max()) > 0 and gb[c].item() != 0.0


def test_graphed_step_replays_ignored_targets_and_sees_weight_updates(dev):
    from chexpert_amd.graph import GraphedTrainStep
    from chexpert_amd.optim import FusedAdam
    m_e, m_g, S = _twin("densenet", dev)
    B = 4
    xs = [synth.xray_batch(700 + i, B, S).to(dev) for i in range(3)]
    ts = [_targets(710 + 10 * i, B, 5, ignored=0.25).to(dev) for i in range(3)]
    assert all((t < 0).any() for t in ts)
    w = synth.uniform(720, (5,), 0.5, 8.0).to(dev)
    m_e.set_loss(ignore_negative=True, pos_weight=w)
    m_g.set_loss(ignore_negative=True, pos_weight=w)
    opt_e, opt_g = FusedAdam(m_e, lr=1e-3), FusedAdam(m_g, lr=1e-3)
    # captured on a batch WITHOUT ignored labels: what a replay reads is the target copied in, not the one captured
    gs = GraphedTrainStep(m_g, opt_g, xs[0], synth.targets(730, B, 5).to(dev))
    held = m_g.loss_pos_weight.data_ptr()
    flat = lambda m: torch.cat([p.detach().flatten() for p in m.parameters()])
    for i in range(2):
        le = _eager_dev_step(m_e, opt_e, xs[i], ts[i])
        lg, _ = gs.replay(xs[i], ts[i])
        assert torch.equal(le, lg), (i, le.item(), lg.item())
        assert torch.equal(flat(m_e), flat(m_g)), i
    # the weights change in place: the captured step reads the new values
    m_g.loss_pos_weight.mul_(2)
    m_e.set_loss(ignore_negative=True, pos_weight=2 * w)
    assert m_g.loss_pos_weight.data_ptr() == held and torch.equal(m_g.loss_pos_weight, m_e.loss_pos_weight)
    le = _eager_dev_step(m_e, opt_e, xs[2], ts[2])
    lg, _ = gs.replay(xs[2], ts[2])
    assert torch.equal(le, lg) and torch.equal(flat(m_e), flat(m_g))
    # ... and they matter: the same step under the old weights gives another loss
    m_g.set_loss(ignore_negative=True, pos_weight=w)
    assert m_g.loss_pos_weight.data_ptr() == held                       # set_loss keeps the storage a captured step reads
    m_g.eval()
    with torch.no_grad():
        out = m_g(xs[2])
    from chexpert_amd.loss import MaskedBCE
    assert MaskedBCE(w)(out, ts[2]).item() != MaskedBCE(2 * w)(out, ts[2]).item()


# ------------------------------------------------------------------------------------------------ data parallel
def _dp_worker(rank, world, port, out_dir):
    import torch.distributed as dist
    os.environ["MASTER_ADDR"], os.environ["MASTER_PORT"] = "127.0.0.1", str(port)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    from chexpert_amd.parallel import broadcast_module_state
    dev = torch.device("cuda:0")
    model, S = _net("densenet", dev)
    broadcast_module_state(model)
    x = synth.xray_batch(100 + rank, 4, S).to(dev)
    t = _targets(200 + 10 * rank, 4, 5, ignored=0.3).to(dev)
    t[:, rank] = -1.0                                     # each rank ignores a whole class of its own
    model.set_loss(ignore_negative=True, pos_weight=synth.uniform(9, (5,), 0.5, 8.0))
    model.forward_backward(x, t)                          # binds the engine; local masked gradient, no reducer yet
    eng = model._eng()
    g_local = eng.flat_grad.detach().cpu().clone()
    gathered = [torch.empty_like(g_local) for _ in range(world)]
    dist.all_gather(gathered, g_local)
    want = sum(gathered) / world
    eng.enable_data_parallel(bucket_bytes=1 << 16)
    model.zero_grad()
    model.forward_backward(x, t)
    torch.cuda.synchronize()
    got = eng.flat_grad.detach().cpu().clone()
    both = [torch.empty_like(got) for _ in range(world)]
    dist.all_gather(both, got)
    torch.save({"got": got, "want": want, "local": g_local, "same": bool(torch.equal(both[0], both[1])),
                "n_ignored": int((t < 0).sum()), "n_buckets": len(eng.reducer.ranges)}, os.path.join(out_dir, "rank%d.pt" % rank))
    dist.destroy_process_group()


def _spawn_with_time_limit(fn, args, nprocs, seconds):
    """mp.spawn whose processes are killed when they outlive `seconds` (a hung rank must not outlive its test)."""
    import torch.multiprocessing as mp
    ctx = mp.spawn(fn, args=args, nprocs=nprocs, join=False)
    deadline = time.time() + seconds
    try:
        while not ctx.join(timeout=5):
            if time.time() > deadline:
                raise TimeoutError("the ranks ran longer than %d s" % seconds)
    finally:
        for p in ctx.processes:
            if p.is_alive():
                p.kill()
                p.join()


def test_data_parallel_masked_gradients_two_ranks_one_gpu(dev, tmp_path):
    port = 35500 + (os.getpid() % 400)
    _spawn_with_time_limit(_dp_worker, (2, port, str(tmp_path)), 2, 300)
    recs = [torch.load(os.path.join(str(tmp_path), "rank%d.pt" % r)) for r in range(2)]
    assert not torch.equal(recs[0]["local"], recs[1]["local"])
    for r, rec in enumerate(recs):
        assert rec["same"], "ranks ended with different gradients"
        assert rec["n_buckets"] >= 3 and rec["n_ignored"] >= 4
        g, w = rec["got"].double(), rec["want"].double()
        rel = float((g - w).norm() / w.norm())
        print("rank %d: rel %.3e, %d ignored labels, %d buckets" % (r, rel, rec["n_ignored"], rec["n_buckets"]))
        assert rel < 1e-6, rel


# ------------------------------------------------------------------------------------------------ command line
def _losses(capsys):
    out = capsys.readouterr().out
    return [json.loads(l)["train_loss"] for l in out.splitlines() if l.startswith('{"step"')]


_CLI_BASE = ["--train", "--synthetic", "64", "--fused_optimizer", "--graph", "--batch_size", "4", "--resize", "64", "--eval_interval", "16",
             "--log_interval", "1", "--seed", "3"]

def test_cli_ignore_policy_with_auto_weights_in_the_graphed_step(dev, tmp_path, capsys):
    from chexpert_amd import cli
    capsys.readouterr()
    out = str(tmp_path / "u")
    cli.main(_CLI_BASE + ["--synthetic_uncertain", "0.2", "--uncertain", "ignore", "--pos_weight", "auto", "--output_dir", out])
    lu = _losses(capsys)
    assert len(lu) == 16 and all(math.isfinite(v) for v in lu), lu
    cfg = json.load(open(os.path.join(out, "config.json")))
    assert cfg["uncertain"] == "ignore" and cfg["pos_weight"] == ["auto"] and cfg["synthetic_uncertain"] == 0.2
    ds = cli.SyntheticXrays(64, 64, 5, 7, 0.2, "ignore")
    assert (ds.targets < 0).any()
    want = cli.resolve_pos_weight(["auto"], ds.targets, 5)
    assert cfg["pos_weight_resolved"] == want and len(want) == 5 and all(1 / 16 <= v <= 16 for v in want)
    res = json.load(open(os.path.join(out, "eval_results_step_16.json")))
    assert len(res["aucs"]) == 5 and all(math.isfinite(v) for v in res["loss"].values())
    # the non-fused route under the same flags: the loss module through autograd
    cli.main([a for a in _CLI_BASE if a not in ("--fused_optimizer", "--graph")] +
             ["--synthetic_uncertain", "0.2", "--uncertain", "ignore", "--pos_weight", "auto", "--output_dir", str(tmp_path / "e")])
    le = _losses(capsys)
    assert len(le) == 16 and all(math.isfinite(v) for v in le) and le[0] == lu[0]      # one first batch, one loss kernel


# The loss lines of `--train --synthetic 64 --fused_optimizer --graph --batch_size 4 --resize 64 --eval_interval 16 --log_interval 1
# --seed 3` as the commit before this feature prints them on an MI355X (steps 1 .. 16)
_PARENT_LOSS_LINES = [3.74753, 3.69885, 3.55252, 3.63391, 3.58182, 3.70679, 3.43228, 3.36451, 3.58357, 3.2646, 3.22182, 3.26596,
                      3.35101, 3.28316, 3.36463, 3.04184]


def test_cli_default_flags_never_reach_the_new_kernel(dev, tmp_path, capsys, monkeypatch):
    """Without the three new flags the command is the one it was: it prints the loss lines recorded from the parent commit, every
    loss launch is ops.bce_fwd_bwd with the arguments FusedNet.forward_backward has always passed, cx_bce_masked_fwd_bwd is never
    called, the evaluation keeps torch's element losses, and config.json holds the defaults."""
    from chexpert_amd import cli, ops
    plain, masked = [], []
    real = ops.bce_fwd_bwd

    def counted(logits, target, loss, loss_elem, dlogits, grad_scale=1.0):
        plain.append((tuple(logits.shape), loss_elem is None, grad_scale))
        return real(logits, target, loss, loss_elem, dlogits, grad_scale)
    monkeypatch.setattr(ops, "bce_fwd_bwd", counted)
    monkeypatch.setattr(ops, "bce_masked_fwd_bwd", lambda *a, **k: masked.append(a))
    capsys.readouterr()
    cli.main(_CLI_BASE + ["--output_dir", str(tmp_path / "p")])
    lp = _losses(capsys)
    print("loss lines without the new flags:", lp)
    assert lp == _PARENT_LOSS_LINES
    assert not masked
    assert plain and all(c == ((4, 5), True, 1.0) for c in plain), plain[:3]      # warm-up and capture; replays launch no Python
    cfg = json.load(open(os.path.join(str(tmp_path / "p"), "config.json")))
    assert cfg["uncertain"] == "ones" and cfg["pos_weight"] is None and cfg["synthetic_uncertain"] == 0.0
    assert "pos_weight_resolved" not in cfg
    cli.main(_CLI_BASE + ["--output_dir", str(tmp_path / "q")])
    assert _losses(capsys) == lp and not masked
