"""Contrastive pretraining without a GPU: the float64 statement of the NT-Xent / SupCon loss (loss.reference_ntxent) against an
independent torch statement and its closed forms, the tolerance the GPU tests hold the kernels to (derived here, and met here by a
float32 evaluation of the statement on the GPU tests' inputs), set_loss / NTXentLoss / the C entry point's refusals, the command
line's refusals, the two-view batch and id plan, and the key handling of --init_backbone."""
import math

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from chexpert_amd import loss as L

U = 2.0 ** -24            # the unit roundoff of fp32


# ------------------------------------------------------------------------------------------------ the cases the GPU tests share
SHAPES = [(2, 8), (4, 5), (6, 16), (64, 128), (65, 128), (130, 136), (512, 128)]
TAUS = [0.5, 0.05]
LAYOUTS = ["pairs", "triple", "negative", "one"]


def ids_of(layout, N):
    """pairs: row i and row i + N // 2 are two views (an odd N leaves the last row single); triple: three rows of one id, the rest
    singles; negative: the pairs with every third row taken out (id -1); one: one id for all rows."""
    h = max(N // 2, 1)
    pairs = np.where(np.arange(N) < 2 * h, np.arange(N) % h, N).astype(np.float64)
    if layout == "pairs":
        return pairs
    if layout == "triple":
        return np.concatenate([np.zeros(min(3, N)), np.arange(1, max(N - 3, 0) + 1)]).astype(np.float64)
    if layout == "negative":
        return np.where(np.arange(N) % 3 == 1, -1.0, pairs)
    assert layout == "one"
    return np.zeros(N)


def embeddings(N, d, ids, seed):
    """fp32 embeddings in which rows of one id lie near each other (a common centre plus noise), so the nearest row means something."""
    rng = np.random.default_rng(seed)
    centre, noise = rng.standard_normal((2 * N + 2, d)), rng.standard_normal((N, d))
    return (centre[np.asarray(ids, dtype=np.int64) % (2 * N + 2)] + 0.7 * noise).astype(np.float32)


def case(N, d, layout, seed=None):
    ids = ids_of(layout, N)
    return embeddings(N, d, ids, 1000 * N + d + LAYOUTS.index(layout) if seed is None else seed), ids


def tolerance(e, ids, tau, ref=None):
    """What an fp32 evaluation of the statement may differ from the float64 one by, from rounding alone (u = 2^-24):

      dot products   |e_i| has a relative error of at most (d / 2 + 2) u (a sum of d squares, a square root), a component of z
                     (d / 2 + 3) u, the product of two (d + 6) u; the sum of the d products adds d u sum_k |z_ik z_jk| <= d u.  With
                     the division by tau:  eps_s = (2 d + 9) u / tau  on every s_ij, whatever the order of the sum.
      log-sum-exp    lse and the mean over the positives are 1-Lipschitz in s (sup norm): 2 eps_s on l_i.  Its own arithmetic: s - m
                     (|s - m| <= 2 / tau), expf, a sum of N terms by a tree over at most ceil(N / 256) serial terms and 8 levels,
                     logf, the positives' sum, the divide: `depth` = ceil(N / 256) + 12 roundings on quantities of at most
                     2 / tau + log N + 1.
      =>  eta = 2 eps_s + depth u (2 / tau + log N + 1)        the element losses; the same as a RELATIVE error of exp(s_ij - lse_i)
          loss: eta + 4 u (2 / tau + log N)                    (the mean of the anchors' losses, summed in double)
      gradient       c_ij = dS_ij + dS_ji inherits eta p (p the softmax terms it is made of), the sum over j of c_ij z_j adds at
                     most (N + 3) u sum_j |c_ij| (|z_j| = 1), the step back through the normalisation 3 (d + 8) u.  In the 2-norm of
                     row i, with W_i = sum_j (p_ij + p_ji + |c_ij|) from the float64 statement, M anchors and |e_i| clamped at 1e-12:
                         tol_i = W_i / (|e_i| tau M) * (eta + (N + 3 d + 27) u)
      top1           two candidates whose float64 scores differ by no more than 2 eps_s may change places: such rows are left out.

    Returns {"eps_s", "elem", "loss", "grad" (N,), "top1" (N,) bool: the rows whose nearest row is decided}."""
    N, d = e.shape
    ref = ref or L.reference_ntxent(e, ids, tau)
    eps_s = (2 * d + 9) * U / tau
    logn = math.log(max(N, 2))
    eta = 2 * eps_s + (math.ceil(N / 256) + 12) * U * (2 / tau + logn + 1)
    M = max(int(ref["anchors"].sum()), 1)
    c = ref["dS"] + ref["dS"].T
    W = ref["p"].sum(1) + ref["p"].sum(0) + np.abs(c).sum(1)
    norm = np.maximum(np.sqrt((e.astype(np.float64) ** 2).sum(1)), L.NTXENT_EPS)
    s = np.sort(np.where(np.isfinite(ref["s"]), ref["s"], -np.inf), axis=1)
    with np.errstate(invalid="ignore"):                                            # (a lone candidate has -inf below it: decided)
        decided = np.ones(N, dtype=bool) if N < 2 else ~(s[:, -1] - s[:, -2] <= 2 * eps_s)
    return {"eps_s": eps_s, "elem": eta, "loss": eta + 4 * U * (2 / tau + logn), "grad": W / (norm * tau * M) * (eta + (N + 3 * d + 27) * U),
            "top1": decided & (ref["top1"] >= 0)}


def check_against(ref, tol, loss, elem, grad, top1, what=""):
    """loss, element losses (N,), gradient (N, d) and top1 (N,) as numpy arrays against the float64 statement, within `tol`."""
    assert abs(float(loss) - ref["loss"]) <= tol["loss"], (what, float(loss), ref["loss"], tol["loss"])
    err = np.abs(np.asarray(elem, dtype=np.float64).reshape(-1) - ref["loss_elem"])
    assert err.max() <= tol["elem"], (what, "elem", err.max(), tol["elem"])
    rows = np.sqrt(((np.asarray(grad, dtype=np.float64) - ref["grad"]) ** 2).sum(1))
    assert np.all(rows <= tol["grad"]), (what, "grad", float((rows - tol["grad"]).max()), int(np.argmax(rows - tol["grad"])))
    top1 = np.asarray(top1).reshape(-1)
    assert np.array_equal(top1[tol["top1"]], ref["top1"][tol["top1"]]), (what, "top1")
    assert np.all(top1[ref["top1"] < 0] == -1), (what, "top1 outside V")
    return float(err.max()), float((rows / np.maximum(tol["grad"], 1e-300)).max())


@pytest.mark.parametrize("tau", TAUS)
@pytest.mark.parametrize("N,d", SHAPES)
def test_a_float32_evaluation_stays_inside_the_tolerance(N, d, tau):
    """The GPU tests' inputs and bound: the statement evaluated in float32 numpy (another order of every sum than the kernels') meets
    the float64 one within it, and the nearest row is undecided within the bound for at most 5 % of a case's rows."""
    for layout in LAYOUTS:
        e, ids = case(N, d, layout)
        ref = L.reference_ntxent(e, ids, tau)
        tol = tolerance(e, ids, tau, ref)
        r32 = L.reference_ntxent(e, ids, tau, dtype=np.float32)
        check_against(ref, tol, r32["loss"], r32["loss_elem"], r32["grad"], r32["top1"], (N, d, tau, layout))
        left_out = int(((ref["top1"] >= 0) & ~tol["top1"]).sum())
        assert left_out <= 0.05 * N, (N, d, tau, layout, left_out)
        # the bound is a rounding bound, not slack: far below the quantities it guards
        assert tol["elem"] < 2e-3 and (ref["loss"] == 0 or tol["loss"] < 1e-2 * max(ref["loss"], 0.1))


# ------------------------------------------------------------------------------------------------ the statement
def _simclr_torch(e, tau):
    N = e.shape[0]
    x = torch.tensor(e, dtype=torch.float64, requires_grad=True)
    z = F.normalize(x, dim=1)
    s = (z @ z.T / tau).masked_fill(torch.eye(N, dtype=torch.bool), -math.inf)
    partner = (torch.arange(N) + N // 2) % N
    loss = F.cross_entropy(s, partner)
    loss.backward()
    per_row = F.cross_entropy(s, partner, reduction="none")
    return loss.item(), per_row.detach().numpy(), x.grad.numpy()


def _supcon_torch(e, ids, tau):
    """SupCon's L_out written out: for every anchor the mean over its positives of -log softmax."""
    N = e.shape[0]
    x = torch.tensor(e, dtype=torch.float64, requires_grad=True)
    z = x / x.norm(dim=1, keepdim=True).clamp_min(1e-12)
    terms = []
    for i in range(N):
        if ids[i] < 0:
            continue
        cand = [j for j in range(N) if j != i and ids[j] >= 0]
        pos = [j for j in cand if ids[j] == ids[i]]
        if not pos:
            continue
        s = torch.stack([z[i] @ z[j] for j in cand]) / tau
        logp = s - torch.logsumexp(s, 0)
        terms.append(-torch.stack([logp[cand.index(p)] for p in pos]).mean())
    loss = torch.stack(terms).mean()
    loss.backward()
    return loss.item(), x.grad.numpy()


@pytest.mark.parametrize("d", [1, 5, 16])
@pytest.mark.parametrize("N", [2, 4, 6, 10])
def test_reference_is_simclr_nt_xent_on_pairs(N, d):
    rng = np.random.default_rng(10 * N + d)
    e = rng.standard_normal((N, d))
    ids = np.arange(N) % (N // 2)
    for tau in (0.5, 0.1):
        ref = L.reference_ntxent(e, ids, tau)
        loss, rows, grad = _simclr_torch(e, tau)
        assert abs(ref["loss"] - loss) <= 1e-12 * max(1.0, abs(loss))
        assert np.allclose(ref["loss_elem"], rows, rtol=1e-11, atol=1e-12)
        assert np.allclose(ref["grad"], grad, rtol=1e-9, atol=1e-12)
        # a gradient row is orthogonal to its embedding: the loss does not see the length of e_i
        assert np.all(np.abs((ref["grad"] * e).sum(1)) <= 1e-12 * (np.abs(ref["grad"]) * np.abs(e)).sum(1) + 1e-300)


@pytest.mark.parametrize("d", [1, 5, 16])
@pytest.mark.parametrize("N", [4, 6, 10])
def test_reference_is_supcon_with_several_positives(N, d):
    rng = np.random.default_rng(77 * N + d)
    e = rng.standard_normal((N, d))
    for ids in ([0, 0, 0] + list(range(1, N - 2)), [0, 1] * (N // 2), [0] * N, [0, 0, -1] + [1] * (N - 3)):
        ids = np.array(ids, dtype=np.float64)
        ref = L.reference_ntxent(e, ids, 0.3)
        loss, grad = _supcon_torch(e, ids, 0.3)
        assert abs(ref["loss"] - loss) <= 1e-12 * max(1.0, abs(loss)), ids
        assert np.allclose(ref["grad"], grad, rtol=1e-9, atol=1e-12), ids


def test_closed_forms():
    rng = np.random.default_rng(5)
    # one pair and nothing else: the only candidate is the positive, so the loss is log 1 = 0 and nothing moves
    r = L.reference_ntxent(rng.standard_normal((2, 7)), [3, 3], 0.2)
    assert r["loss"] == 0.0 and not r["grad"].any() and r["top1"].tolist() == [1, 0]
    # all ids distinct: no anchor
    r = L.reference_ntxent(rng.standard_normal((5, 3)), np.arange(5), 0.2)
    assert r["loss"] == 0.0 and not r["grad"].any() and not r["loss_elem"].any() and not r["anchors"].any()
    assert np.all(r["top1"] >= 0)                                                 # (still each other's candidates)
    # a negative id takes its row out: the statement on the remaining rows
    e, ids = rng.standard_normal((7, 4)), np.array([0, 1, -1, 0, 1, -5, 2.0])
    keep = ids >= 0
    r, q = L.reference_ntxent(e, ids, 0.4), L.reference_ntxent(e[keep], ids[keep], 0.4)
    assert r["loss"] == q["loss"] and np.array_equal(r["grad"][keep], q["grad"]) and not r["grad"][~keep].any()
    assert np.array_equal(r["loss_elem"][keep], q["loss_elem"]) and not r["loss_elem"][~keep].any()
    assert np.all(r["top1"][~keep] == -1) and np.array_equal(r["top1"][keep], np.flatnonzero(keep)[q["top1"]])
    # a row of V without a positive (id 2) is a negative for the others: without it the loss changes
    assert L.reference_ntxent(e[:6], ids[:6], 0.4)["loss"] != r["loss"]
    # a single row, and a single row of V among rows that are out
    assert L.reference_ntxent(e[:1], [0], 0.4)["top1"].tolist() == [-1]
    assert L.reference_ntxent(e[:3], [-1, 4, -1], 0.4)["top1"].tolist() == [-1, -1, -1]


def test_top1_ties_go_to_the_lowest_index():
    e = np.array([[1.0, 0.0], [0.0, 1.0], [0.0, 1.0], [1.0, 0.0], [1.0, 0.0]])
    r = L.reference_ntxent(e, [0, 1, 1, 0, 2], 0.5)
    assert r["top1"].tolist() == [3, 2, 1, 0, 0]


def test_the_clamp_of_the_normalisation():
    """Below 1e-12 the embedding is divided by the clamp, and the gradient goes back through that division alone."""
    rng = np.random.default_rng(9)
    e = rng.standard_normal((6, 4)) * 1e-20
    x = torch.tensor(e, dtype=torch.float64, requires_grad=True)
    z = F.normalize(x, dim=1)
    s = (z @ z.T / 0.01).masked_fill(torch.eye(6, dtype=torch.bool), -math.inf)
    F.cross_entropy(s, (torch.arange(6) + 3) % 6).backward()
    r = L.reference_ntxent(e, np.arange(6) % 3, 0.01)
    assert np.isfinite(r["grad"]).all() and np.allclose(r["grad"], x.grad.numpy(), rtol=1e-9, atol=0)


# ------------------------------------------------------------------------------------------------ refusals that need no GPU
def test_set_loss_refuses_without_changing_anything():
    state = L.Loss()
    cpu = torch.device("cpu")
    for kw in (dict(kind="ntxent", pos_weight=[1.0] * 8), dict(kind="ntxent", ignore_negative=True), dict(kind="ntxent", temperature=0.0),
               dict(kind="ntxent", temperature=-1.0), dict(kind="ntxent", temperature=float("nan")), dict(kind="ntxent", temperature=float("inf")),
               dict(kind="ntxent", temperature="warm"), dict(kind="ntxent", gamma=2.0), dict(kind="ntxent", clip=0.1),
               dict(kind="ntxent", prior=[0.5] * 8), dict(kind="ntxent", margin=2.0), dict(kind="ntxent", class_weight=[[1, 1, 1]]),
               dict(kind="ntxent", parent=[-1] * 8), dict(kind="ntxent", mode="conditional"), dict(kind="bce", temperature=0.2),
               dict(kind="focal", temperature=0.2), dict(kind="hier", parent=[-1] * 8, temperature=0.2), dict(kind="simclr")):
        with pytest.raises(ValueError):
            state.set(cpu, 8, **kw)
        assert state.kind == "bce" and state.temperature is None and state._held == {}, kw
    with pytest.raises(ValueError, match="at most 1024"):
        state.set(cpu, 2048, kind="ntxent")
    with pytest.raises(RuntimeError, match="model.to"):                            # the state lives on the parameters' device
        state.set(cpu, 8, kind="ntxent")
    assert state.kind == "bce" and state.temperature is None
    with pytest.raises(ValueError, match="temperature"):
        state.load_state({"kind": "ntxent"}, cpu, 8)


def test_loss_module_and_top1_refuse_what_they_cannot_take():
    for bad in (0.0, -0.1, float("nan"), None, "x"):
        with pytest.raises(ValueError):
            L.NTXentLoss(bad)
    crit = L.NTXentLoss(0.1)
    assert crit.kind == "ntxent" and crit.temperature.tolist() == pytest.approx([0.1]) and list(crit.state_dict()) == []
    with pytest.raises(RuntimeError, match="GPU only"):
        crit(torch.zeros(4, 8), torch.zeros(4, 1))
    with pytest.raises(RuntimeError, match="GPU only"):
        crit.elementwise(torch.zeros(4, 8), torch.zeros(4, 1))
    with pytest.raises(RuntimeError, match="GPU only"):
        L.contrastive_top1(torch.zeros(4, 8), torch.zeros(4))
    assert L.KERNEL["ntxent"] == "cx_ntxent_fwd_bwd"


def test_entry_point_validates_before_any_launch():
    """cx_ntxent_fwd_bwd and cx_ntxent_scratch check their arguments before anything is launched (no GPU needed)."""
    from chexpert_amd import _lib, ops
    EINVAL, ESHAPE = -1, -3
    lib = _lib.lib()
    f = [torch.zeros(4096, dtype=torch.float32) for _ in range(4)]
    E, G, T, S = (t.data_ptr() for t in f)
    call = lambda e=E, g=G, t=T, s=S, floats=4096, N=8, d=16: lib.cx_ntxent_fwd_bwd(e, g, t, None, None, None, None, 1.0, s, floats, N, d, None)   # noqa: E731
    assert call(e=None) == EINVAL and call(g=None) == EINVAL and call(t=None) == EINVAL and call(s=None) == EINVAL
    assert call(N=0) == EINVAL and call(N=-3) == EINVAL and call(d=0) == EINVAL and call(d=-1) == EINVAL
    assert call(floats=8 * 16 + 4 * 8 - 1) == EINVAL and call(floats=0) == EINVAL
    assert call(N=_lib.NTXENT_MAX_N + 1, floats=1 << 40) == ESHAPE and call(d=_lib.NTXENT_MAX_D + 1, floats=1 << 40) == ESHAPE
    assert _lib.NTXENT_MAX_N >= 2048 and _lib.NTXENT_MAX_D >= 512
    assert lib.cx_ntxent_scratch(8, 16) == 8 * 16 + 4 * 8 == ops.ntxent_scratch(8, 16)
    assert lib.cx_ntxent_scratch(2048, 512) == 2048 * 512 + 4 * 2048
    assert lib.cx_ntxent_scratch(0, 16) == 0 and lib.cx_ntxent_scratch(8, 0) == 0 and lib.cx_ntxent_scratch(_lib.NTXENT_MAX_N + 1, 4) == 0
    for N, d in ((0, 4), (4, 0), (_lib.NTXENT_MAX_N + 1, 4), (4, _lib.NTXENT_MAX_D + 1)):
        with pytest.raises(ValueError):
            ops.ntxent_scratch(N, d)
    # the wrapper: host tensors are refused before the library is called
    e, g, t = torch.zeros(4, 8), torch.zeros(4, 1), torch.ones(1)
    with pytest.raises(RuntimeError, match="GPU only"):
        ops.ntxent_fwd_bwd(e, g, t, None, None, None)
    with pytest.raises(AssertionError):
        ops.ntxent_fwd_bwd(e, g.reshape(-1), t, None, None, None)
    with pytest.raises(AssertionError):
        ops.ntxent_fwd_bwd(e, g, t, None, None, None, scratch=torch.zeros(10))


# ------------------------------------------------------------------------------------------------ the command line
_PRE = ["--train", "--synthetic", "16", "--batch_size", "4", "--resize", "64", "--pretrain", "contrastive"]


def test_cli_flag_checks(tmp_path):
    from chexpert_amd import cli
    run = cli.check_flags(_PRE + ["--jitter"])
    assert run.pretrain == {"proj_dim": 128, "temperature": None, "positive": "view"} and cli.head_width(run.args) == 128
    assert cli.temperature_of(run.pretrain) == 0.2 and cli.temperature_of(run.pretrain, {"temperature": 0.07}) == 0.07
    run = cli.check_flags(_PRE + ["--affine", "--proj_dim", "32", "--temperature", "0.5", "--fused_optimizer", "--graph", "--optimizer", "lamb",
                                  "--ema_decay", "0.99", "--sam_rho", "0.05", "--pool", "gem", "--model", "resnet152"])
    assert run.pretrain == {"proj_dim": 32, "temperature": 0.5, "positive": "view"} and cli.head_width(run.args) == 32
    assert cli.temperature_of(run.pretrain, {"temperature": 0.07}) == 0.5
    assert cli.check_flags(["--train", "--synthetic", "16"]).pretrain is None                          # every other run: as before
    assert cli.head_width(cli.check_flags(["--train", "--synthetic", "16"]).args) == 5
    ck = tmp_path / "some.pt"
    ck.write_bytes(b"")
    refused = [([], "--affine or --jitter"),
               (["--jitter", "--mixup", "0.4"], "--mixup"), (["--jitter", "--cutmix", "1.0"], "--cutmix"), (["--affine", "--erase_prob", "0.5"], "--erase_prob"),
               (["--jitter", "--loss", "focal"], "--loss focal"), (["--jitter", "--loss", "hier", "--hier_parents", "-1", "0", "0", "-1", "3"], "--loss hier"),
               (["--jitter", "--uncertain", "multiclass"], "--uncertain multiclass"), (["--jitter", "--head", "csra"], "--head csra"),
               (["--jitter", "--head", "pcam"], "--head pcam"), (["--jitter", "--pos_weight", "auto"], "--pos_weight"),
               (["--jitter", "--evaluate_single_model"], "--evaluate_single_model"), (["--jitter", "--evaluate_ensemble"], "--evaluate_ensemble"),
               (["--jitter", "--visualize"], "--visualize"), (["--jitter", "--plot_roc"], "--plot_roc"),
               (["--jitter", "--proj_dim", "0"], "--proj_dim"), (["--jitter", "--proj_dim", "4096"], "--proj_dim"),
               (["--jitter", "--temperature", "0"], "temperature"), (["--jitter", "--temperature", "-1"], "temperature"),
               (["--jitter", "--positive", "study"], "--positive study"), (["--jitter", "--positive", "patient"], "--positive patient"),
               (["--jitter", "--init_backbone", str(ck), "--restore", str(ck)], "exclusive")]
    for extra, why in refused:
        with pytest.raises(ValueError) as err:
            cli.check_flags(_PRE + extra)
        assert why in str(err.value) and "\n" not in str(err.value), (extra, str(err.value))
    with pytest.raises(ValueError, match="2 x --batch_size"):
        cli.check_flags(["--train", "--synthetic", "16", "--batch_size", "4096", "--pretrain", "contrastive", "--jitter"])
    with pytest.raises(ValueError, match="pass --train"):
        cli.check_flags(["--synthetic", "16", "--pretrain", "contrastive", "--jitter"])
    for flags in (["--proj_dim", "16"], ["--temperature", "0.1"], ["--positive", "view"]):
        with pytest.raises(ValueError, match="belong to --pretrain contrastive"):
            cli.check_flags(["--train", "--synthetic", "16"] + flags)
    with pytest.raises(ValueError, match="pass --train"):
        cli.check_flags(["--evaluate_single_model", "--synthetic", "16", "--init_backbone", str(ck)])
    with pytest.raises(ValueError, match="no file"):
        cli.check_flags(["--train", "--synthetic", "16", "--init_backbone", str(tmp_path / "absent.pt")])
    assert cli.check_flags(["--train", "--synthetic", "16", "--init_backbone", str(ck), "--head", "csra", "--loss", "asl"]).pretrain is None
    assert cli.check_flags(["--train", "--synthetic", "16", "--init_backbone", str(ck), "--pool", "gem", "--loss", "focal"]).pretrain is None


def test_more_than_one_rank_is_refused(monkeypatch):
    from chexpert_amd import cli
    monkeypatch.setattr(cli.P, "dist_info", lambda: (0, 2, 0))
    with pytest.raises(ValueError, match="more than one rank"):
        cli.check_flags(_PRE + ["--jitter"])
    from chexpert_amd.models import _fused
    with pytest.raises(RuntimeError, match="kind='ntxent'.*world size 2"):
        _fused.check_single_process(type("R", (), {"world": 2})(), _fused.NTXENT_DATA_PARALLEL)
    _fused.check_single_process(type("R", (), {"world": 1})(), _fused.NTXENT_DATA_PARALLEL)
    _fused.check_single_process(None, _fused.NTXENT_DATA_PARALLEL)


def test_restore_is_refused_across_pretraining_and_supervised_runs():
    from chexpert_amd import cli
    pre = {"proj_dim": 16, "temperature": None, "positive": "view"}
    sup = {"state_dict": {"classifier.weight": torch.zeros(5, 8)}}
    con = {"pretrain": "contrastive", "state_dict": {"features.w": torch.zeros(4, 3, 3, 3), "classifier.weight": torch.zeros(16, 8), "classifier.bias": torch.zeros(16)}}
    con["state_dict"]["later.table"] = torch.zeros(7, 2)                           # (a 2-D tensor behind the classifier: not its width)
    key = "classifier.weight"
    cli.check_checkpoint_pretrain(sup, None, "a.pt", key)
    cli.check_checkpoint_pretrain(con, pre, "a.pt", key)
    with pytest.raises(ValueError, match="--init_backbone"):
        cli.check_checkpoint_pretrain(con, None, "a.pt", key)
    with pytest.raises(ValueError, match="supervised"):
        cli.check_checkpoint_pretrain(sup, pre, "a.pt", key)
    with pytest.raises(ValueError, match="16 outputs, --proj_dim asks for 32"):
        cli.check_checkpoint_pretrain(con, dict(pre, proj_dim=32), "a.pt", key)


def test_two_view_batch_and_id_plan():
    """[x; x] and the ids for --positive view, study and patient on a made-up list: rows i and i + B are the same image; `view` numbers
    the positions, the others give every row the index of its image's group, so two images of one patient are positives."""
    from chexpert_amd import augment
    x = torch.arange(3 * 1 * 2 * 2, dtype=torch.uint8).reshape(3, 1, 2, 2)
    xx = augment.duplicate_views(x)
    assert xx.dtype == torch.uint8 and tuple(xx.shape) == (6, 1, 2, 2) and torch.equal(xx[:3], x) and torch.equal(xx[3:], x)
    rows = torch.tensor([7, 2, 5])
    ids = augment.contrastive_ids(rows)
    assert ids.dtype == torch.float32 and tuple(ids.shape) == (6, 1) and ids.reshape(-1).tolist() == [0, 1, 2, 0, 1, 2]
    paths = ["p1/s1", "p1/s2", "p2/s1", "p2/s1", "p3/s1", "p1/s1", "p3/s2", "p3/s1"]                 # one per dataset row
    study = np.unique(np.array(paths), return_inverse=True)[1]
    patient = np.unique(np.array([p.rsplit("/", 1)[0] for p in paths]), return_inverse=True)[1]
    assert augment.contrastive_ids(rows, study).reshape(-1).tolist() == [float(study[i]) for i in (7, 2, 5)] * 2
    got = augment.contrastive_ids([7, 4, 6, 0], patient).reshape(-1).tolist()
    assert got == [2, 2, 2, 0, 2, 2, 2, 0]                                                         # three images of patient p3, one of p1
    ref = L.reference_ntxent(np.random.default_rng(0).standard_normal((8, 4)), got, 0.2)
    assert ref["anchors"].all() and ref["p"].shape == (8, 8)
    # the plan is SimCLR's for `view`: every id exactly twice, partner B rows away
    r = L.reference_ntxent(np.random.default_rng(1).standard_normal((6, 4)), ids.reshape(-1).numpy(), 0.2)
    assert r["anchors"].all() and np.array_equal(np.flatnonzero(r["dS"][0] < 0), [3])
    with pytest.raises(ValueError):
        augment.contrastive_ids([0], [1 << 24])
    # the unit derivation is the one behind --bootstrap_unit, and a set without file paths is refused by name
    from chexpert_amd import cli
    assert cli.unit_groups("view", object(), "--positive", "view") is None and cli.unit_groups("image", object()) is None
    with pytest.raises(ValueError, match="--positive patient groups the images by their file paths"):
        cli.unit_groups("patient", object(), "--positive", "view")
    with pytest.raises(ValueError, match="--bootstrap_unit study groups the images by their file paths; this dataset has none \\(use image\\)"):
        cli.unit_groups("study", object())


def test_positive_codes_follow_the_loaders_row_labels():
    """A dataset whose frame kept its csv row labels after a filter (labels 3, 4, 8, 10, 11 at positions 0 .. 4): the training loader
    hands out LABELS (the third item of ds[i]), the evaluation positions; each finds its image's study / patient."""
    import pandas as pd
    from chexpert_amd import augment, cli
    paths = ["d/train/patient1/study1/a.jpg", "d/train/patient2/study1/a.jpg", "d/train/patient1/study2/a.jpg",
             "d/train/patient2/study1/b.jpg", "d/train/patient3/study1/a.jpg"]
    ds = type("DS", (), {})()
    ds.data = pd.DataFrame({"Path": paths}, index=[3, 4, 8, 10, 11])
    assert cli.positive_codes("view", ds) is None and cli.positive_codes("view", ds, by_label=True) is None
    study, patient = cli.positive_codes("study", ds), cli.positive_codes("patient", ds)
    assert study.tolist() == [0, 2, 1, 2, 3] and patient.tolist() == [0, 1, 0, 1, 2]
    table = cli.positive_codes("patient", ds, by_label=True)
    assert table.tolist() == [-1, -1, -1, 0, 1, -1, -1, -1, 0, -1, 1, 2]
    labels = [10, 3, 11, 8]                                                          # a minibatch as the loader yields it
    assert augment.contrastive_ids(labels, table).reshape(-1).tolist() == [1, 0, 2, 0] * 2
    assert augment.contrastive_ids([3, 0, 4, 2], patient).reshape(-1).tolist() == [1, 0, 2, 0] * 2     # the same images by position
    assert augment.contrastive_ids([4, 10], cli.positive_codes("study", ds, by_label=True)).reshape(-1).tolist() == [2, 2, 2, 2]
    with pytest.raises(ValueError):                                                  # a label no image has
        augment.contrastive_ids([5], table)
    with pytest.raises(IndexError):
        augment.contrastive_ids([12], table)


def test_init_backbone_key_handling():
    import torch.nn as nn
    from chexpert_amd import cli

    class Tiny(nn.Module):
        def __init__(self, width):
            super().__init__()
            self.features = nn.Sequential(nn.Conv2d(1, 2, 1), nn.BatchNorm2d(2))
            self.classifier = nn.Linear(2, width)
    torch.manual_seed(0)
    pre, fine = Tiny(16), Tiny(5)
    with torch.no_grad():
        pre.features[1].running_mean.fill_(3.0)
        pre.features[1].num_batches_tracked.fill_(9)
    head = set(cli.classifier_keys(fine))
    assert cli.classifier_keys(fine) == ("classifier.weight", "classifier.bias") and cli.POOL_KEYS == ("pool_p", "pool_r")
    ck = dict(pre.state_dict(), pool_p=torch.full((1,), 2.5))                                      # (a GeM checkpoint into an avg model)
    taken = cli.backbone_state(fine.state_dict(), ck, head, "f.pt")
    assert set(taken) == set(fine.state_dict()) - head and all(taken[k] is ck[k] for k in taken) and "pool_p" not in taken
    assert "features.1.running_mean" in taken and "features.1.num_batches_tracked" in taken
    # the pooling's numbers: taken where both sides hold them in one shape, left alone otherwise (--pool stays free)
    gem = dict(fine.state_dict(), pool_p=torch.full((1,), 3.0))
    assert cli.backbone_state(gem, ck, head, "f.pt")["pool_p"] is ck["pool_p"]
    assert "pool_p" not in cli.backbone_state(gem, pre.state_dict(), head, "f.pt")                 # (an avg checkpoint into a GeM model)
    assert "pool_p" not in cli.backbone_state(gem, dict(ck, pool_p=torch.zeros(2)), head, "f.pt")
    lse = dict(fine.state_dict(), pool_r=torch.full((1,), 10.0))
    assert "pool_r" not in cli.backbone_state(lse, ck, head, "f.pt") and "pool_p" not in cli.backbone_state(lse, ck, head, "f.pt")
    missing = {k: v for k, v in ck.items() if k != "features.1.running_var"}
    with pytest.raises(ValueError, match="no tensor 'features.1.running_var'"):
        cli.backbone_state(fine.state_dict(), missing, head, "f.pt")
    with pytest.raises(ValueError, match="'features.0.weight' has shape \\(4, 1, 1, 1\\) in the checkpoint, \\(2, 1, 1, 1\\)"):
        cli.backbone_state(fine.state_dict(), dict(ck, **{"features.0.weight": torch.zeros(4, 1, 1, 1)}), head, "f.pt")
    with pytest.raises(ValueError, match="no place for the checkpoint's tensor 'features.9.weight'"):
        cli.backbone_state(fine.state_dict(), dict(ck, **{"features.9.weight": torch.zeros(1)}), head, "f.pt")
