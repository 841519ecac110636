"""CPU (no GPU): the kNN probe's C ABI (declarations, bindings, validation codes before any launch), the numpy float64 definitions
of the search and the vote (chexpert_amd/knn.py), and the command line's refusals."""
import os
import re

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRY = {"cx_knn_scratch": 4, "cx_knn_normalize": 5, "cx_knn_topk": 14, "cx_knn_vote": 10}


def test_header_makefile_and_bindings_agree():
    from chexpert_amd import _lib, ops
    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "chexpert_hip.h")).read(), flags=re.S)
    for name, n in ENTRY.items():
        m = re.search(r"\b(?:int|long long)\s+%s\s*\(([^;{]*?)\)\s*;" % name, hdr, flags=re.S)
        assert m, "%s is not declared in include/chexpert_hip.h" % name
        assert len(_lib.SIGNATURES[name]) == m.group(1).count(",") + 1 == n, name
        assert hasattr(_lib.lib(), name) and callable(getattr(ops, name[3:]))
        assert name in open(os.path.join(ROOT, "INTEGRATION.md")).read()
    mk = open(os.path.join(ROOT, "chexpert_amd", "csrc", "Makefile")).read()
    assert "knn.hip" in [l for l in mk.splitlines() if l.startswith("SRCS")][0]
    assert _lib.lib().cx_abi_version() == 10                           # additive entry points
    assert _lib.lib().cx_knn_scratch.restype is _lib.C.c_longlong
    for name, v in (("CX_KNN_MAX_K", 256), ("CX_KNN_MAX_D", 4096), ("CX_KNN_MAX_SPLITS", ops.KNN_MAX_SPLITS), ("CX_KNN_MAX_CLASSES", 64)):
        assert int(re.search(r"#define\s+%s\s+(\d+)" % name, hdr).group(1)) == v
    assert (ops.KNN_MAX_K, ops.KNN_MAX_D, ops.KNN_MAX_CLASSES) == (256, 4096, 64)
    # only ops names the library
    src = open(os.path.join(ROOT, "chexpert_amd", "knn.py")).read()
    assert "lib()" not in src and "_lib" not in src


def test_validation_codes_before_any_launch():
    """Every refusal returns before a launch, so it is the same without a GPU.  The pointers are never dereferenced."""
    from chexpert_amd import _lib
    L = _lib.lib()
    EINVAL, EALIGN = -1, -2
    p, Q, M, d, k = 4096, 17, 300, 16, 7

    def topk(q=p, bank=p, qg=None, bg=None, sim=p, idx=p, scratch=p, floats=None, Q=Q, M=M, d=d, k=k, splits=3):
        floats = L.cx_knn_scratch(Q, M, k, splits) if floats is None else floats
        return L.cx_knn_topk(q, bank, qg, bg, sim, idx, scratch, floats, Q, M, d, k, splits, None)
    for kw in ({"q": None}, {"bank": None}, {"sim": None}, {"idx": None}, {"scratch": None, "floats": 1 << 30}):
        assert topk(**kw) == EINVAL, kw
    assert topk(k=0, floats=1 << 30) == EINVAL and topk(k=257, floats=1 << 30) == EINVAL
    assert topk(d=0) == EINVAL and topk(d=4097) == EINVAL
    assert topk(Q=0, floats=1 << 30) == EINVAL and topk(M=0, floats=1 << 30) == EINVAL
    assert topk(splits=-1, floats=1 << 30) == EINVAL and topk(splits=257, floats=1 << 30) == EINVAL
    assert topk(qg=p) == EINVAL and topk(bg=p) == EINVAL                      # one group pointer without the other
    for splits in (0, 1, 3, 7):
        need = L.cx_knn_scratch(Q, M, k, splits)
        assert need >= 2 * Q * k * max(splits, 1) and need % 2 == 0
        assert topk(splits=splits, floats=need - 1) == EINVAL                # a scratch one float too small
    assert L.cx_knn_scratch(Q, M, k, 3) == 2 * Q * 3 * k and L.cx_knn_scratch(Q, M, k, 1) == 2 * Q * k
    assert L.cx_knn_scratch(Q, M, 0, 0) == 0 and L.cx_knn_scratch(Q, M, 257, 0) == 0 and L.cx_knn_scratch(0, M, k, 0) == 0
    assert topk(q=p + 2) == EALIGN and topk(scratch=p + 4) == EALIGN and topk(qg=p + 1, bg=p) == EALIGN
    assert L.cx_knn_normalize(None, p, 3, 4, None) == EINVAL and L.cx_knn_normalize(p, None, 3, 4, None) == EINVAL
    assert L.cx_knn_normalize(p, p, 0, 4, None) == EINVAL and L.cx_knn_normalize(p, p, 3, 4097, None) == EINVAL
    vote = lambda *a: L.cx_knn_vote(*a, None)                                                          # noqa: E731
    assert vote(None, p, p, p, p, 1.0, 3, 5, 5) == EINVAL and vote(p, p, p, p, None, 1.0, 3, 5, 5) == EINVAL
    assert vote(p, p, p, p, p, 1.0, 3, 0, 5) == EINVAL and vote(p, p, p, p, p, 1.0, 3, 257, 5) == EINVAL
    assert vote(p, p, p, p, p, 1.0, 3, 5, 65) == EINVAL and vote(p, p, p, p, p, -1.0, 3, 5, 5) == EINVAL
    assert vote(p, p, p, p, p, float("nan"), 3, 5, 5) == EINVAL


def test_reference_topk_against_brute_force_argsort():
    from chexpert_amd import knn
    rng = np.random.default_rng(5)
    q, bank = rng.standard_normal((9, 12)), rng.standard_normal((57, 12))
    sim, idx, S, A = knn.reference_topk(q, bank, 10)
    want = np.argsort(-(q @ bank.T), axis=1, kind="stable")[:, :10]            # tie-free: any sort gives this order
    assert np.array_equal(idx, want) and np.array_equal(sim, np.take_along_axis(q @ bank.T, want, 1))
    assert np.array_equal(S, q @ bank.T) and np.allclose(A, np.abs(q[:, None, :] * bank[None]).sum(-1), rtol=1e-14, atol=0)
    assert (np.diff(sim, axis=1) < 0).all()
    # patient-disjoint: the rows of the query's group are gone, everything else keeps its order
    qg, bg = np.arange(9) % 3, np.arange(57) % 4
    qg[0] = -1                                                                 # a negative group excludes nothing
    sim_g, idx_g, _, _ = knn.reference_topk(q, bank, 10, qg, bg)
    assert np.array_equal(idx_g[0], idx[0])
    for i in range(1, 9):
        full = np.argsort(-(q[i] @ bank.T), kind="stable")
        assert np.array_equal(idx_g[i], [j for j in full if bg[j] != qg[i]][:10])
    with pytest.raises(ValueError):
        knn.reference_topk(q, bank, 3, qg, None)


def test_reference_topk_ties_exclusion_and_tail_by_hand():
    from chexpert_amd import knn
    bank = np.array([[1.0], [2.0], [1.0], [2.0], [0.0], [np.nan]])
    q = np.array([[1.0], [-1.0]])
    sim, idx, _, _ = knn.reference_topk(q, bank, 6)
    assert idx.tolist() == [[1, 3, 0, 2, 4, 5], [4, 0, 2, 1, 3, 5]]           # equal similarities: the lower index; NaN last (as -inf)
    assert sim[0].tolist() == [2, 2, 1, 1, 0, -np.inf] and sim[1].tolist() == [0, -1, -1, -2, -2, -np.inf]
    assert not np.signbit(sim[1, 0])                                            # -0 is +0
    sim, idx, _, _ = knn.reference_topk(q, bank, 5, q_group=[7, -1], bank_group=[0, 7, 7, 1, 7, 2])
    assert idx.tolist() == [[3, 0, 5, -1, -1], [4, 0, 2, 1, 3]]               # group 7 is absent from query 0, the tail is -1 / -inf
    assert sim[0].tolist() == [2, 1, -np.inf, -np.inf, -np.inf]


def test_reference_vote_by_hand():
    from chexpert_amd import knn
    labels = np.array([[1.0, 0.0, -1.0], [0.0, 1.0, -1.0], [1.0, -1.0, -1.0], [0.25, 0.0, -1.0]])
    sim = np.array([[0.9, 0.8, 0.6, -np.inf], [0.5, 0.5, -np.inf, -np.inf], [-np.inf] * 4])
    idx = np.array([[2, 0, 1, -1], [3, 3, -1, -1], [-1] * 4])
    score, support = knn.reference_vote(sim, idx, labels, 10.0)
    w = np.exp(np.array([0.0, -1.0, -3.0]))                                   # (s - 0.9) * 10
    assert np.allclose(support[0], [w.sum(), w[1] + w[2], 0.0], rtol=1e-15)   # class 1: row 2's label is ignored; class 2: all are
    assert np.allclose(score[0], [(w[0] + w[1]) / w.sum(), w[2] / (w[1] + w[2]), 0.5], rtol=1e-15)
    assert score[1].tolist() == [0.25, 0.0, 0.5] and support[1].tolist() == [2.0, 2.0, 0.0]
    assert score[2].tolist() == [0.5, 0.5, 0.5] and support[2].tolist() == [0.0, 0.0, 0.0]       # no neighbour at all
    score, support = knn.reference_vote(sim, idx, labels, 0.0)                # the unweighted vote
    assert score[0].tolist() == [2 / 3, 0.5, 0.5] and support[0].tolist() == [3.0, 2.0, 0.0]


def test_knn_auc_uses_supported_confident_rows_only():
    from chexpert_amd import knn, metrics
    score = np.array([[0.9], [0.2], [0.7], [0.1], [0.99], [0.0]])
    support = np.array([[1.0], [2.0], [1.0], [1.0], [0.0], [1.0]])
    targets = np.array([[1.0], [0.0], [0.0], [1.0], [0.0], [-1.0]])
    f, t, _ = metrics.roc_curve(targets[:4, 0], score[:4, 0])
    assert knn.knn_auc(score, support, targets) == {0: metrics.auc(f, t)} and knn.knn_auc(score, support, targets)[0] == 0.5
    assert np.isnan(knn.knn_auc(score, np.zeros_like(support), targets)[0]) and np.isnan(knn.mean_auc({0: float("nan")}))
    assert knn.bank_indices(10, 0) == list(range(10)) == knn.bank_indices(10, 12) and knn.bank_indices(10, 4) == [0, 2, 5, 7]


_PRE = ["--train", "--synthetic", "16", "--pretrain", "contrastive", "--jitter"]


def test_cli_flag_checks():
    from chexpert_amd import cli
    assert cli.check_flags(_PRE).knn is None and cli.check_flags(["--train", "--synthetic", "16"]).knn is None
    assert cli.check_flags(_PRE + ["--knn_probe", "200"]).knn == {"k": 200, "temperature": 0.1, "bank": 8192}
    run = cli.check_flags(["--evaluate_single_model", "--synthetic", "16", "--knn_probe", "3", "--knn_temperature", "0.07", "--knn_bank", "0"])
    assert run.knn == {"k": 3, "temperature": 0.07, "bank": 0}
    refused = [(_PRE + ["--knn_probe", "0"], "1 .. 256"), (_PRE + ["--knn_probe", "257"], "1 .. 256"),
               (_PRE + ["--knn_probe", "5", "--knn_temperature", "0"], "--knn_temperature"),
               (_PRE + ["--knn_probe", "5", "--knn_temperature", "-0.1"], "--knn_temperature"),
               (_PRE + ["--knn_probe", "5", "--knn_bank", "-1"], "--knn_bank"),
               (["--evaluate_single_model", "--synthetic", "16", "--knn_probe", "5", "--head", "csra"], "--head csra"),
               (["--evaluate_single_model", "--synthetic", "16", "--knn_probe", "5", "--head", "pcam"], "--head pcam"),
               (["--train", "--synthetic", "16", "--knn_probe", "5"], "--pretrain contrastive or with --evaluate_single_model"),
               (["--train", "--synthetic", "16", "--knn_temperature", "0.1"], "belong to --knn_probe"),
               (["--train", "--synthetic", "16", "--knn_bank", "64"], "belong to --knn_probe")]
    for argv, why in refused:
        with pytest.raises(ValueError) as err:
            cli.check_flags(argv)
        assert why in str(err.value) and "\n" not in str(err.value), (argv, str(err.value))


def test_more_than_one_rank_is_refused(monkeypatch):
    from chexpert_amd import cli
    monkeypatch.setattr(cli.P, "dist_info", lambda: (0, 2, 0))
    with pytest.raises(ValueError, match="--knn_probe cannot be combined with more than one rank"):
        cli.check_flags(["--evaluate_single_model", "--synthetic", "16", "--knn_probe", "5"])
