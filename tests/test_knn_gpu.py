"""GPU: the exact k-nearest-neighbour search, the vote and the row normalisation of csrc/knn.hip against their numpy float64
definitions (chexpert_amd/knn.py: reference_topk, reference_vote), FusedNet.embed, and the command line's --knn_probe.

Exact cases use values from {-1, 0, 1}: every partial sum is an integer below 2^24, so any fp32 summation order is exact and the
kernel's (similarity, index) lists must equal the definition bit for bit; such inputs are full of ties, which tests the index rule
across tile and slice boundaries.  General cases (unit-norm Gaussian rows) are held to the bound of ANY fp32 summation of d products,
E = (d + 1) 2^-24 sum_k |q_k b_k| per pair: the returned similarities within E of the float64 ones, the list sorted exactly by its own
key, and no row left out beating a row taken by more than the two rows' bounds added."""
import glob
import json
import math
import os

import numpy as np
import pytest
import torch

from chexpert_amd import synth

pytestmark = pytest.mark.gpu

SPLITS = (0, 1, 3, 7)
EXACT = [(1, 1, 1, 1), (3, 5, 3, 5), (17, 300, 16, 7), (33, 1000, 64, 200), (5, 4099, 24, 256), (70, 2500, 8, 64)]
GENERAL = [(17, 300, 130, 7), (33, 1000, 1024, 200), (5, 4099, 2048, 256), (9, 700, 2560, 50)]


@pytest.fixture(scope="module")
def dev():
    from chexpert_amd import _lib
    _lib.lib()
    return torch.device("cuda:0")


def ternary(seed, rows, d):
    return np.random.default_rng(seed).integers(-1, 2, size=(rows, d)).astype(np.float32)


def unit_rows(seed, rows, d):
    x = np.random.default_rng(seed).standard_normal((rows, d))
    return (x / np.linalg.norm(x, axis=1, keepdims=True)).astype(np.float32)


def search(dev, q, bank, k, splits=0, q_group=None, bank_group=None):
    from chexpert_amd import knn
    sim, idx = knn.knn_topk(torch.from_numpy(q).to(dev), torch.from_numpy(bank).to(dev), k,
                            None if q_group is None else torch.as_tensor(q_group), None if bank_group is None else torch.as_tensor(bank_group),
                            metric="dot", splits=splits)
    torch.cuda.synchronize()
    return sim.cpu().numpy(), idx.cpu().numpy()


def assert_exact(got, want):
    (sim, idx), (rsim, ridx) = got, want[:2]
    assert sim.dtype == np.float32 and idx.dtype == np.int32
    assert np.array_equal(idx, ridx), "indices differ at %s" % (np.argwhere(idx != ridx)[:5].tolist(),)
    assert np.array_equal(sim, rsim.astype(np.float32)) and not np.signbit(sim[sim == 0]).any()


_refs = {}


def exact_case(shape):
    """(q, bank, reference) of an exact shape, computed once and shared by the splits."""
    from chexpert_amd import knn
    if shape not in _refs:
        Q, M, d, k = shape
        q, bank = ternary(Q + 31 * d, Q, d), ternary(M + 17 * d, M, d)
        _refs[shape] = (q, bank, knn.reference_topk(q, bank, k))
    return _refs[shape]


@pytest.mark.parametrize("splits", SPLITS)
@pytest.mark.parametrize("shape", EXACT, ids=lambda s: "x".join(map(str, s)))
def test_exact_cases_equal_the_definition_bit_for_bit(dev, shape, splits):
    q, bank, ref = exact_case(shape)
    assert_exact(search(dev, q, bank, shape[3], splits), ref)


@pytest.mark.parametrize("splits", (1, 7))
def test_group_exclusion_leave_one_out_and_patient_groups(dev, splits):
    from chexpert_amd import knn
    Q, M, d, k = 17, 300, 16, 7
    bank = ternary(41, M, d)
    own = np.arange(M, dtype=np.int32)                                       # leave-one-out: q = bank, the group is the row's position
    got = search(dev, bank, bank, k, splits, own, own)
    assert_exact(got, knn.reference_topk(bank, bank, k, own, own))
    assert not (got[1] == own[:, None]).any()
    q, patients = ternary(43, Q, d), np.arange(M, dtype=np.int32) // 4        # patient-disjoint: groups of 4 rows
    qg = (np.arange(Q, dtype=np.int32) * 5) % (M // 4)
    qg[3] = -1                                                                # a negative group excludes nothing
    got = search(dev, q, bank, k, splits, qg, patients)
    assert_exact(got, knn.reference_topk(q, bank, k, qg, patients))
    assert_exact((got[0][3:4], got[1][3:4]), [r[3:4] for r in knn.reference_topk(q, bank, k)[:2]])
    assert not (patients[got[1]] == qg[:, None])[qg >= 0].any()


@pytest.mark.parametrize("splits", (1, 7))
def test_fewer_candidates_than_k_gives_the_tail(dev, splits):
    from chexpert_amd import knn
    q, bank = ternary(47, 17, 16), ternary(53, 300, 16)
    groups = np.minimum(np.arange(300, dtype=np.int32) // 99, 2)             # groups 0, 1 of 99 rows; group 2 of 102
    qg = np.arange(17, dtype=np.int32) % 4 - 1                                # -1 (nothing excluded), 0, 1, 2
    for k in (200, 256):
        sim, idx = search(dev, q, bank, k, splits, qg, groups)
        assert_exact((sim, idx), knn.reference_topk(q, bank, k, qg, groups))
        left = np.array([300, 201, 201, 198])[qg + 1]                         # candidates each query has
        for i in range(17):
            n = min(k, left[i])
            assert (idx[i, :n] >= 0).all() and (idx[i, n:] == -1).all() and np.isneginf(sim[i, n:]).all() and np.isfinite(sim[i, :n]).all()
    sim, idx = search(dev, q[:3], bank[:5], 9, splits)                         # a bank smaller than k
    assert_exact((sim, idx), knn.reference_topk(q[:3], bank[:5], 9))
    assert (idx[:, 5:] == -1).all() and np.isneginf(sim[:, 5:]).all()


def sorted_by_own_key(sim, idx):
    a, b, i, j = sim[:, :-1], sim[:, 1:], idx[:, :-1], idx[:, 1:]
    return bool(((a > b) | ((a == b) & (i < j)) | (j < 0)).all())


_general = {}


def general_case(shape):
    from chexpert_amd import knn
    if shape not in _general:
        Q, M, d, k = shape
        q, bank = unit_rows(Q + d, Q, d), unit_rows(M + d, M, d)
        _, _, S, A = knn.reference_topk(q, bank, 1)
        _general[shape] = (q, bank, S, (d + 1) * 2.0 ** -24 * A)
    return _general[shape]


@pytest.mark.parametrize("shape", GENERAL, ids=lambda s: "x".join(map(str, s)))
def test_general_cases_within_the_fp32_summation_bound(dev, shape):
    Q, M, d, k = shape
    q, bank, S, E = general_case(shape)
    sim, idx = search(dev, q, bank, k)
    assert (idx >= 0).all() and (idx < M).all() and all(len(set(r)) == k for r in idx.tolist())
    err = np.abs(sim.astype(np.float64) - np.take_along_axis(S, idx.astype(np.int64), 1))
    bound = np.take_along_axis(E, idx.astype(np.int64), 1)
    print("shape %s: max |sim - S| %.3e, max of the bound %.3e, largest ratio %.3f" % (shape, err.max(), bound.max(), (err / bound).max()))
    assert (err <= bound).all()
    assert sorted_by_own_key(sim, idx)
    for i in range(Q):
        taken = np.zeros(M, dtype=bool)
        taken[idx[i]] = True
        if taken.all():
            continue
        assert (S[i] - E[i])[~taken].max() <= (S[i] + E[i])[taken].min(), "query %d: a row left out beats a row taken" % i


def test_two_launches_and_every_split_give_equal_bits(dev):
    Q, M, d, k = 33, 1000, 1024, 200
    q, bank, _, _ = general_case((Q, M, d, k))
    first = search(dev, q, bank, k, 1)
    for splits in (1, 7, 0, 3):
        again = search(dev, q, bank, k, splits)
        assert np.array_equal(first[0].view(np.int32), again[0].view(np.int32)) and np.array_equal(first[1], again[1]), splits


def test_nan_counts_as_minus_infinity_and_ops_refusals(dev):
    from chexpert_amd import knn, ops
    q, bank = ternary(3, 4, 8), ternary(5, 200, 8)
    bank[7, 2] = np.nan
    bank[130, 0] = np.nan
    sim, idx = search(dev, q, bank, 200, 3)
    # (0 * NaN is NaN: the two rows are NaN for every query)
    assert np.array_equal(idx[:, -2:], np.tile([7, 130], (4, 1))) and np.isneginf(sim[:, -2:]).all() and np.isfinite(sim[:, :-2]).all()
    t = lambda *s: torch.empty(*s, device=dev)                                                          # noqa: E731
    with pytest.raises(ValueError):
        knn.knn_topk(t(3, 4), t(9, 4), 257)
    with pytest.raises(ValueError):
        knn.knn_topk(t(3, 4), t(9, 4), 0)
    with pytest.raises(ValueError):
        knn.knn_topk(t(3, 4), t(9, 5), 2)
    with pytest.raises(ValueError):
        knn.knn_topk(t(3, 4), t(9, 4), 2, q_group=torch.zeros(3))
    with pytest.raises(ValueError):
        knn.knn_topk(t(3, 4), t(9, 4), 2, metric="l2")
    with pytest.raises(ValueError):
        ops.knn_scratch(3, 9, 2, 257)
    with pytest.raises(RuntimeError, match="GPU only"):
        ops.knn_normalize(torch.zeros(2, 3), torch.zeros(2, 3))


def test_normalize_against_float64(dev):
    from chexpert_amd import knn
    rng = np.random.default_rng(9)
    for rows, d in ((1, 1), (7, 3), (33, 130), (5, 1024), (3, 2560)):
        x = (rng.standard_normal((rows, d)) * 10.0 ** rng.integers(-6, 7, size=(rows, 1))).astype(np.float32)
        if rows > 2:
            x[1] = 0.0                                                         # stays zero
            x[2] = 1e-20                                                       # below the clamp: x / 1e-12
        y = knn.normalize(torch.from_numpy(x).to(dev)).cpu().numpy().astype(np.float64)
        x64 = x.astype(np.float64)
        want = x64 / np.maximum(np.sqrt((x64 * x64).sum(1, keepdims=True)), 1e-12)
        assert np.all(np.abs(y - want) <= 2.0 ** -22 * np.abs(want)), (rows, d)
        if rows > 2:
            assert not y[1].any() and np.allclose(y[2], 1e-8, rtol=2.0 ** -22, atol=0)
    q = knn.normalize(torch.from_numpy(unit_rows(1, 4, 64) * 3).to(dev))       # cosine = dot of the normalised rows
    a = knn.knn_topk(q * 5, q, 4, metric="cosine")
    b = knn.knn_topk(knn.normalize(q * 5), knn.normalize(q), 4, metric="dot")
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1]) and a[1][:, 0].tolist() == [0, 1, 2, 3]


def vote(dev, sim, idx, labels, inv_T):
    from chexpert_amd import ops
    Q, n = sim.shape[0], labels.shape[1]
    score, support = torch.empty(Q, n, device=dev), torch.empty(Q, n, device=dev)
    ops.knn_vote(torch.from_numpy(sim).to(dev), torch.from_numpy(idx).to(dev), torch.from_numpy(labels).to(dev), score, support, inv_T)
    return score.cpu().numpy(), support.cpu().numpy()


@pytest.mark.parametrize("k", (8, 200, 256))
def test_vote_against_the_definition(dev, k):
    """Scores within 1e-6 absolute; the support (weights and sums are double in the kernel, the result is rounded to fp32 once) within
    2^-23 of its size.  The temperatures are fp32 numbers, so that kernel and definition see the same inv_T."""
    from chexpert_amd import knn
    rng = np.random.default_rng(k)
    Q, M, n = 37, 500, 14
    labels = rng.integers(0, 2, size=(M, n)).astype(np.float32)
    labels[rng.random((M, n)) < 0.2] = -1.0                                   # ignored labels
    labels[:, 3] = -1.0                                                       # a class nobody has: den = 0
    labels[:, 5] = rng.random(M).astype(np.float32)                           # soft targets
    sim = -np.sort(-rng.uniform(-1, 1, size=(Q, k)).astype(np.float32), axis=1)
    idx = rng.integers(0, M, size=(Q, k)).astype(np.int32)
    for i in range(0, Q, 3):                                                  # the -1 / -inf tail, down to no neighbour at all
        cut = (i * 7) % (k + 1)
        sim[i, cut:], idx[i, cut:] = -np.inf, -1
    for inv_T in (10.0, float(np.float32(1.0 / 0.07)), 0.0):
        score, support = vote(dev, sim, idx, labels, inv_T)
        rscore, rsupport = knn.reference_vote(sim, idx, labels, inv_T)
        assert np.abs(score - rscore).max() <= 1e-6, (inv_T, np.abs(score - rscore).max())
        assert np.all(np.abs(support - rsupport) <= 2.0 ** -23 * rsupport)
        assert (score[:, 3] == 0.5).all() and (support[:, 3] == 0).all()
        empty = idx[:, 0] < 0
        assert empty.any() and (score[empty] == 0.5).all() and (support[empty] == 0).all()
    hard = np.where(labels < 0, -1.0, np.round(labels)).astype(np.float32)     # inv_T = 0 on 0/1 labels: integer sums, exact
    score, support = vote(dev, sim, idx, hard, 0.0)
    rscore, rsupport = knn.reference_vote(sim, idx, hard, 0.0)
    assert np.array_equal(support, rsupport.astype(np.float32)) and np.array_equal(score, rscore.astype(np.float32))
    again = vote(dev, sim, idx, labels, 10.0)
    assert np.array_equal(again[0], vote(dev, sim, idx, labels, 10.0)[0])


def test_knn_predict_and_auc_end_to_end(dev):
    from chexpert_amd import knn
    bank, q = unit_rows(11, 400, 96), unit_rows(12, 50, 96)
    labels = (np.random.default_rng(13).random((400, 5)) < 0.4).astype(np.float32)
    labels[::7, 2] = -1.0
    score, support = knn.knn_predict(torch.from_numpy(q).to(dev), torch.from_numpy(bank).to(dev), torch.from_numpy(labels), k=20, T=0.1)
    rsim, ridx, _, _ = knn.reference_topk(q, bank, 20)
    rscore, rsupport = knn.reference_vote(rsim, ridx, labels, 10.0)
    assert np.abs(score.cpu().numpy() - rscore).max() <= 2e-5                  # (the similarities' 1e-7 enter the weights through / T)
    targets = (np.random.default_rng(14).random((50, 5)) < 0.5).astype(np.float32)
    aucs = knn.knn_auc(score, support, targets)
    assert set(aucs) == set(range(5)) and all(0.0 <= v <= 1.0 for v in aucs.values())


# ---- the embedding ---------------------------------------------------------------------------------------------------------------------
def small_model(net, dev, storage, n_cls=5):
    from oracle import nets
    if net == "densenet121":
        from chexpert_amd.models import densenet121
        model = densenet121(num_classes=n_cls)
        sd = synth.fill_state_dict_(nets.zeros_state_dict(nets.densenet_spec(n_cls)), 21)
    elif net == "resnet":
        from chexpert_amd.models import Bottleneck, ResNet
        model = ResNet(Bottleneck, [1, 1, 1, 1], num_classes=n_cls)
        sd = synth.fill_state_dict_(nets.zeros_state_dict(nets.resnet_spec(n_cls, layers=(1, 1, 1, 1))), 21)
    else:
        from chexpert_amd.models import construct_model
        model = construct_model("efficientnet-b0", n_cls)
        sd = synth.fill_state_dict_(nets.zeros_state_dict(nets.efficientnet_spec("efficientnet-b0", n_cls)), 21)
        synth.smooth_state_dict_(sd, 1.0)
    model.storage_dtype(storage).load_state_dict(sd, strict=True)
    return model.to(dev).eval()


def last_linear(model):
    return [m for m in model.modules() if isinstance(m, torch.nn.Linear)][-1]


def assert_classifier_reads(feats, fc, logits):
    """classifier(feats) in float64 against the model's logits, within the bound of any fp32 summation of C products and the bias."""
    f, w, b = feats.double().cpu(), fc.weight.detach().double().cpu(), fc.bias.detach().double().cpu()
    bound = (fc.in_features + 2) * 2.0 ** -24 * (f.abs() @ w.abs().T + b.abs())
    assert ((f @ w.T + b - logits.double().cpu()).abs() <= bound).all()


@pytest.mark.parametrize("storage", ["bf16", "fp32"])
@pytest.mark.parametrize("net", ["densenet121", "resnet", "efficientnet-b0"])
def test_embed_is_what_the_classifier_reads(dev, net, storage):
    model = small_model(net, dev, storage)
    x = synth.xray_batch(3, 3, 64).to(dev)
    before = model(x)
    feats, logits = model.embed(x, return_logits=True)
    after = model(x)
    fc = last_linear(model)
    assert feats.dtype == torch.float32 and tuple(feats.shape) == (3, fc.in_features) and torch.isfinite(feats).all()
    assert torch.equal(before, logits) and torch.equal(before, after) and torch.equal(model.embed(x), feats)
    assert_classifier_reads(feats, fc, before)


@pytest.mark.parametrize("kind", ["max", "lse", "gem"])
def test_embed_follows_set_pool(dev, kind):
    from chexpert_amd.models import Bottleneck, ResNet
    from oracle import nets
    model = ResNet(Bottleneck, [1, 1, 1, 1], num_classes=5)
    model.set_pool(kind)
    sd = synth.fill_state_dict_(nets.zeros_state_dict(nets.resnet_spec(5, layers=(1, 1, 1, 1))), 21)
    model.load_state_dict(sd, strict=False)
    model.to(dev).eval()
    x = synth.xray_batch(3, 3, 64).to(dev)
    feats, logits = model.embed(x, return_logits=True)
    fc = last_linear(model)
    assert torch.equal(logits, model(x)) and tuple(feats.shape) == (3, fc.in_features)
    assert_classifier_reads(feats, fc, logits)


def test_embed_refusals(dev):
    from chexpert_amd.models import Bottleneck, ResNet
    x = synth.xray_batch(3, 2, 64).to(dev)
    model = ResNet(Bottleneck, [1, 1, 1, 1], num_classes=5).to(dev)
    model.train()
    with pytest.raises(RuntimeError, match="eval mode"):
        model.embed(x)
    with pytest.raises(RuntimeError, match="GPU only"):
        model.eval().embed(x.cpu())
    for kind in ("csra", "pcam"):
        model = ResNet(Bottleneck, [1, 1, 1, 1], num_classes=5)
        model.set_head(kind)
        with pytest.raises(NotImplementedError, match="%s head" % kind):
            model.to(dev).eval().embed(x)


# ---- the command line ------------------------------------------------------------------------------------------------------------------
_CLI = ["--train", "--synthetic", "8", "--batch_size", "4", "--resize", "64", "--eval_interval", "2", "--log_interval", "1", "--seed", "3",
        "--lr", "0.001"]
_PRE = ["--pretrain", "contrastive", "--proj_dim", "16", "--affine", "--jitter"]


def test_cli_pretraining_reports_the_probe(dev, tmp_path, capsys):
    from chexpert_amd import cli, knn
    out = str(tmp_path / "p")
    model = cli.main(_CLI + _PRE + ["--fused_optimizer", "--knn_probe", "3", "--knn_bank", "0", "--output_dir", out])
    text = capsys.readouterr().out
    res = json.load(open(os.path.join(out, "pretrain_eval_step_2.json")))
    got = res["knn"]
    assert set(got) == {"k", "temperature", "bank", "aucs", "mean_auc"} and (got["k"], got["temperature"], got["bank"]) == (3, 0.1, 8)
    assert "kNN probe @ step 2" in text
    # recomputed through the float64 definitions from the returned model's embeddings
    train_ds, valid_ds = cli.SyntheticXrays(8, 64, 5, 7), cli.SyntheticXrays(4, 64, 5, 11)
    mode = model.training
    bank, labels = knn.embed_dataset(model, train_ds, range(8), 4, dev)
    q, targets = knn.embed_dataset(model, valid_ds, range(4), 4, dev)
    assert tuple(bank.shape) == (8, 1024) and tuple(labels.shape) == (8, 5) and model.training == mode
    unit = lambda v: v / np.maximum(np.linalg.norm(v, axis=1, keepdims=True), 1e-12)                    # noqa: E731
    rsim, ridx, _, _ = knn.reference_topk(unit(q.double().cpu().numpy()), unit(bank.double().cpu().numpy()), 3)
    want = knn.knn_auc(*knn.reference_vote(rsim, ridx, labels.numpy(), 10.0), targets)
    assert np.allclose([got["aucs"][str(c)] for c in range(5)], [want[c] for c in range(5)], rtol=0, atol=1e-12, equal_nan=True)
    m = knn.mean_auc(want)
    assert (math.isnan(m) and math.isnan(got["mean_auc"])) or got["mean_auc"] == pytest.approx(m, abs=1e-12)
    idx, sim = knn.retrieve(model, bank, train_ds[5][0][None].to(dev), 3)     # the image itself is its own nearest neighbour
    assert idx[0, 0].item() == 5 and sim[0, 0].item() == pytest.approx(1.0, abs=1e-5) and model.training == mode
    # the same run without the flag: today's keys
    out2 = str(tmp_path / "q")
    cli.main(_CLI + _PRE + ["--fused_optimizer", "--output_dir", out2])
    plain = json.load(open(os.path.join(out2, "pretrain_eval_step_2.json")))
    assert set(plain) == set(res) - {"knn"} and all(plain[key] == res[key] for key in plain)
    assert "kNN probe" not in capsys.readouterr().out


def test_cli_evaluate_single_model_writes_the_probe(dev, tmp_path, capsys):
    from chexpert_amd import cli
    out = str(tmp_path / "s")
    cli.main(_CLI + ["--fused_optimizer", "--output_dir", out])
    ev = str(tmp_path / "e")
    cli.main(["--evaluate_single_model", "--synthetic", "8", "--batch_size", "4", "--resize", "64", "--restore",
              os.path.join(out, "checkpoint_latest.pt"), "--output_dir", ev, "--knn_probe", "3", "--knn_temperature", "0.07", "--knn_bank", "4"])
    assert "kNN probe @ step 2" in capsys.readouterr().out
    files = glob.glob(os.path.join(ev, "knn_*.json"))
    assert [os.path.basename(f) for f in files] == ["knn_step_2.json"] and os.path.exists(os.path.join(ev, "eval_results_step_2.json"))
    res = json.load(open(files[0]))
    assert (res["k"], res["temperature"], res["bank"]) == (3, 0.07, 4) and set(res["aucs"]) == {str(c) for c in range(5)}
    assert all(math.isnan(v) or 0.0 <= v <= 1.0 for v in res["aucs"].values())
