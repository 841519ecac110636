"""GPU: the linear probe's kernels (csrc/probe.hip) against their numpy float64 definitions (chexpert_amd/probe.py), the L-BFGS fit
against the float64 optimum, and the command line's --linear_probe.

Exact cases.  Logits of X, W from {-1, 0, 1} with an integer bias: every partial sum is an integer below 2^24, so any fp32 summation
order is exact.  The loss and gradient at theta = 0: z = 0, sigmoid = 0.5 exactly, r is a multiple of 0.25 for pos_weight from
{0.5, 1, 2} and labels from {0, 1}; with ternary X every sum is a multiple of 0.25 far below 2^23 of those units, and with a
power-of-two number of live rows per class the one division is exact: the gradient must equal the definition bit for bit for every
`splits`, which catches a dropped or doubled row or column at a tile, slice or tail boundary.

General cases are held to reference_loss_grad's E_loss / E_grad, first-order bounds of ANY fp32 evaluation of the definition
(u = 2^-24; the budget per element is stated there: expf 1 ulp, log1pf 2 ulp, as the ROCm device library documents them)."""
import glob
import json
import math
import os

import numpy as np
import pytest
import torch

from chexpert_amd import synth

pytestmark = pytest.mark.gpu

U = 2.0 ** -24
SPLITS = (0, 1, 3, 7)
EXACT_LOGITS = [(1, 1, 1), (3, 5, 3), (17, 16, 14), (33, 130, 16), (70, 1025, 17), (5, 2560, 64)]
EXACT_GRAD = [(1, 1, 1), (300, 16, 5), (1000, 64, 14), (4099, 24, 17), (2500, 1030, 3)]
GENERAL = [(300, 24, 5), (1000, 130, 14), (257, 1024, 3), (700, 2560, 20)]
FITS = [((300, 24, 5), 1e-3), ((1000, 130, 14), 1e-4), ((257, 1024, 3), 1e-2)]
G_TOL = 1e-5


@pytest.fixture(scope="module")
def dev():
    from chexpert_amd import _lib
    _lib.lib()
    return torch.device("cuda:0")


def ids(s):
    return "x".join(map(str, s))


def gpu(dev, a):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).to(dev)


def loss_grad(dev, X, Y, theta, pw=None, l2=0.0, splits=0, active=None, into=None):
    """(loss, grad, count) as numpy from ops.probe_loss_grad; `into`: the three output tensors to reuse."""
    from chexpert_amd import ops
    n, d = Y.shape[1], X.shape[1]
    if into is None:
        into = (torch.zeros(n, device=dev), torch.zeros(n, d + 1, device=dev), torch.zeros(n, 3, device=dev))
    ops.probe_loss_grad(gpu(dev, X), gpu(dev, Y), gpu(dev, theta), into[0], into[1], into[2], gpu(dev, pw), l2,
                        None if active is None else torch.as_tensor(active, dtype=torch.int32, device=dev), None, splits)
    torch.cuda.synchronize()
    return tuple(t.cpu().numpy() for t in into)


# ---- exact cases ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", EXACT_LOGITS, ids=ids)
def test_logits_exact_cases_equal_the_definition_bit_for_bit(dev, shape):
    from chexpert_amd import ops
    rows, d, n = shape
    rng = np.random.default_rng(rows + 31 * d + n)
    X = rng.integers(-1, 2, size=(rows, d)).astype(np.float32)
    theta = rng.integers(-1, 2, size=(n, d + 1)).astype(np.float32)
    theta[:, d] = rng.integers(-50, 51, size=n)
    out = ops.probe_logits(gpu(dev, X), gpu(dev, theta), torch.full((rows, n), 7.5, device=dev)).cpu().numpy()
    want = X.astype(np.float64) @ theta[:, :d].astype(np.float64).T + theta[:, d]
    assert out.dtype == np.float32 and np.array_equal(out, want.astype(np.float32))


_exact = {}


def exact_case(shape):
    """(X, Y, pos_weight, l2, the float64 reference) of an exact shape, computed once and shared by the splits."""
    from chexpert_amd import probe
    if shape not in _exact:
        M, d, n = shape
        rng = np.random.default_rng(M + 17 * d + n)
        X = rng.integers(-1, 2, size=(M, d)).astype(np.float32)
        Y = np.full((M, n), -1.0, dtype=np.float32)
        top = 1 << (M.bit_length() - 1)                                        # the largest power of two <= M
        for c in range(n):
            live = rng.permutation(M)[:max(1, top >> (c % 3))]                  # another power of two, other rows, per class
            Y[live, c] = rng.integers(0, 2, size=len(live))
        pw = rng.choice([0.5, 1.0, 2.0], size=n).astype(np.float32)
        l2 = 0.37
        _exact[shape] = (X, Y, pw, l2, probe.reference_loss_grad(X, Y, np.zeros((n, d + 1)), pw, l2))
    return _exact[shape]


@pytest.mark.parametrize("splits", SPLITS)
@pytest.mark.parametrize("shape", EXACT_GRAD, ids=ids)
def test_loss_grad_exact_cases_at_zero(dev, shape, splits):
    M, d, n = shape
    X, Y, pw, l2, (rloss, rgrad, E_loss, _) = exact_case(shape)
    loss, grad, count = loss_grad(dev, X, Y, np.zeros((n, d + 1), dtype=np.float32), pw, l2, splits)
    assert np.array_equal(rgrad.astype(np.float32).astype(np.float64), rgrad), "the case is not exactly representable"
    bad = np.argwhere(grad != rgrad.astype(np.float32))
    assert not len(bad), "gradient differs at (class, column) %s" % bad[:5].tolist()
    live = Y >= 0
    assert np.array_equal(count[:, 0], live.sum(0).astype(np.float32))
    assert np.array_equal(count[:, 1], np.where(live, Y, 0).sum(0)) and np.array_equal(count[:, 2], np.where(live, 1 - Y, 0).sum(0))
    assert np.all(np.abs(loss - rloss) <= E_loss), (np.abs(loss - rloss) / E_loss).max()


# ---- general cases -------------------------------------------------------------------------------------------------------------------
_general = {}


def general_case(shape):
    from chexpert_amd import probe
    if shape not in _general:
        M, d, n = shape
        rng = np.random.default_rng(M + d + n)
        X = rng.standard_normal((M, d)).astype(np.float32)
        theta = (rng.standard_normal((n, d + 1)) / math.sqrt(d)).astype(np.float32)
        Y = (rng.random((M, n)) < 0.4).astype(np.float32)
        Y[:, 1 % n] = rng.random(M)                                            # a soft-label class
        Y[rng.random((M, n)) < 0.1] = -1.0
        Y[:, n - 1] = -1.0                                                     # a class entirely ignored
        pw = rng.uniform(0.5, 3.0, size=n).astype(np.float32)
        l2 = 1e-3
        _general[shape] = (X, Y, theta, pw, l2, probe.reference_loss_grad(X, Y, theta, pw, l2))
    return _general[shape]


@pytest.mark.parametrize("shape", GENERAL, ids=ids)
def test_general_cases_within_the_fp32_bounds(dev, shape):
    M, d, n = shape
    X, Y, theta, pw, l2, (rloss, rgrad, E_loss, E_grad) = general_case(shape)
    loss, grad, count = loss_grad(dev, X, Y, theta, pw, l2)
    eg, el = np.abs(grad - rgrad), np.abs(loss - rloss)
    print("shape %s: largest ratio error / bound: gradient %.4f, loss %.4f" % (shape, np.nanmax(eg / np.where(E_grad > 0, E_grad, np.nan)), (el / E_loss).max()))
    assert np.all(eg <= E_grad) and np.all(el <= E_loss)
    live = Y >= 0
    assert np.array_equal(count[:, 0], live.sum(0).astype(np.float32)) and count[n - 1].tolist() == [0, 0, 0]
    pos = np.where(live, Y.astype(np.float64), 0).sum(0)
    assert np.all(np.abs(count[:, 1] - pos) <= (M + 2) * U * pos)
    # logits of the same operands: the bound of any fp32 summation of d products and the bias
    from chexpert_amd import ops
    z = ops.probe_logits(gpu(dev, X), gpu(dev, theta), torch.empty(M, n, device=dev)).cpu().numpy()
    X64, t64 = X.astype(np.float64), theta.astype(np.float64)
    dz = (d + 2) * U * (np.abs(X64) @ np.abs(t64[:, :d]).T + np.abs(t64[:, d]))
    assert np.all(np.abs(z - (X64 @ t64[:, :d].T + t64[:, d])) <= dz)


def test_two_launches_give_equal_bits_and_inactive_classes_keep_theirs(dev):
    shape = (1000, 130, 14)
    X, Y, theta, pw, l2, _ = general_case(shape)
    first = loss_grad(dev, X, Y, theta, pw, l2, 3)
    again = loss_grad(dev, X, Y, theta, pw, l2, 3)
    assert all(np.array_equal(a.view(np.int32), b.view(np.int32)) for a, b in zip(first, again))
    n, d = 14, 130
    active = np.array([1, 0, 1, 1, 0, 0, 1, 1, 1, 0, 1, 1, 0, 1], dtype=np.int32)
    into = (torch.full((n,), -3.25, device=dev), torch.full((n, d + 1), -3.25, device=dev), torch.full((n, 3), -3.25, device=dev))
    got = loss_grad(dev, X, Y, theta, pw, l2, 3, active, into)
    for a, b in zip(got, first):
        assert np.array_equal(a[active == 1].view(np.int32), b[active == 1].view(np.int32))
        assert (a[active == 0] == -3.25).all()
    none = loss_grad(dev, X, Y, theta, pw, l2, 0, np.zeros(n, dtype=np.int32), into)       # nothing active: nothing written
    assert all(np.array_equal(a.view(np.int32), b.view(np.int32)) for a, b in zip(none, got))


def test_ops_refusals(dev):
    from chexpert_amd import ops, probe
    t = lambda *s: torch.zeros(*s, device=dev)                                                          # noqa: E731
    with pytest.raises(ValueError):
        ops.probe_scratch(10, 4097, 3)
    with pytest.raises(ValueError):
        ops.probe_scratch(10, 8, 65)
    with pytest.raises(ValueError):
        ops.probe_scratch(10, 8, 3, 1025)
    with pytest.raises(ValueError):
        ops.probe_loss_grad(t(5, 3), t(5, 2), t(2, 4), t(2), t(2, 4), t(2, 3), l2=-1.0)
    with pytest.raises(AssertionError):
        ops.probe_loss_grad(t(5, 3), t(5, 2), t(2, 3), t(2), t(2, 4), t(2, 3))
    with pytest.raises(RuntimeError, match="GPU only"):
        ops.probe_standardize(torch.zeros(2, 3), torch.zeros(3), torch.zeros(3), torch.zeros(2, 3))
    with pytest.raises(ValueError):
        probe.fit(t(5, 3), t(4, 2))
    with pytest.raises(ValueError):
        probe.fit(t(5, 3), t(5, 2), l2=-1.0)
    with pytest.raises(ValueError):
        probe.fit(t(5, 3), t(5, 2), history=17)


@pytest.mark.parametrize("shape", [(1, 1), (7, 3), (300, 130), (4099, 1024)], ids=ids)
def test_column_statistics_and_standardisation(dev, shape):
    """mean and rstd against the float64 definition within 2^-22 relative (a double-accumulated, once-rounded result, as in
    test_normalize_against_float64); the standardised matrix equals fp32((fp32(x - mean)) * rstd) bit for bit."""
    from chexpert_amd import ops, probe
    M, d = shape
    rng = np.random.default_rng(M + d)
    X = (rng.standard_normal((M, d)) * rng.uniform(0.01, 20, size=d) + rng.uniform(-3, 3, size=d)).astype(np.float32)
    if d >= 3:
        X[:, 1] = 3.25                                                         # a constant column
        X[:, 2] = (1e4 + rng.standard_normal(M)).astype(np.float32)            # a column of magnitude 1e4
    mean, rstd = torch.empty(d, device=dev), torch.empty(d, device=dev)
    ops.probe_colstats(gpu(dev, X), mean, rstd)
    rmean, rstd_dev, rrstd = probe.reference_colstats(X)
    m, r = mean.cpu().numpy(), rstd.cpu().numpy()
    assert np.all(np.abs(m - rmean) <= 2.0 ** -22 * np.abs(rmean)) and np.all(np.abs(r - rrstd) <= 2.0 ** -22 * rrstd)
    Xs = ops.probe_standardize(gpu(dev, X), mean, rstd, torch.empty(M, d, device=dev)).cpu().numpy()
    want = ((X - m).astype(np.float32) * r).astype(np.float32)
    assert np.array_equal(Xs.view(np.int32), want.view(np.int32))
    if d >= 3 or M == 1:
        k = 1 if d >= 3 else 0
        assert r[k] == np.float32(1e6) and not Xs[:, k].any()
    inplace = gpu(dev, X)
    ops.probe_standardize(inplace, mean, rstd, inplace)                         # in place
    assert np.array_equal(inplace.cpu().numpy().view(np.int32), want.view(np.int32))


# ---- the fit ---------------------------------------------------------------------------------------------------------------------------
_fits = {}


def fit_case(dev, case):
    """A planted logistic model on Gaussian features of another scale and offset per column, 10 % ignored labels, one all-ignored
    and one all-negative class appended: (X, Y, the fit, the standardised X the fit ran on as numpy fp32, theta*)."""
    from chexpert_amd import probe
    if case not in _fits:
        (M, d, n), l2 = case
        rng = np.random.default_rng(M + d)
        Z = rng.standard_normal((M, d))
        planted = rng.standard_normal((n, d + 1)) / math.sqrt(d)
        Y = (rng.random((M, n)) < 1 / (1 + np.exp(-2 * (Z @ planted[:, :d].T + planted[:, d])))).astype(np.float32)
        Y[rng.random((M, n)) < 0.1] = -1.0
        Y = np.concatenate([Y, np.full((M, 1), -1.0, np.float32), np.zeros((M, 1), np.float32)], axis=1)
        X = (Z * rng.uniform(0.5, 4, size=d) + rng.uniform(-2, 2, size=d)).astype(np.float32)
        fit = probe.fit(gpu(dev, X), gpu(dev, Y), l2=l2, g_tol=G_TOL)
        Xs = ((X - fit["mean"].cpu().numpy()).astype(np.float32) * fit["rstd"].cpu().numpy()).astype(np.float32)
        _fits[case] = (X, Y, fit, Xs, probe.reference_optimum(Xs, Y, None, l2))
    return _fits[case]


def assert_fit(theta, status, Xs, Y, l2, star, what):
    """The conditions of a converged fit: status 0 on every class with both kinds of labels; the float64 gradient at theta within
    g_tol + its own fp32 bound; by convexity f(theta) - f(theta*) <= |g(theta)|_2 |theta - theta*|_2, up to the loss's bound on both
    evaluations; status 2 and zeros on the degenerate classes."""
    from chexpert_amd import probe
    n = Y.shape[1]
    dead = probe.degenerate(Y)
    assert dead[-2:].all() and not dead[:-2].any()
    assert [status[c] for c in range(n)] == [2 if dead[c] else 0 for c in range(n)], (what, status)
    assert not theta[dead].any()
    loss, grad, E_loss, E_grad = probe.reference_loss_grad(Xs, Y, theta, None, l2)
    live = ~dead
    gmax = np.abs(grad[live]).max(axis=1)
    print("%s: |g64|_inf per class %s (g_tol %g + bound %s)" % (what, gmax, G_TOL, E_grad[live].max(axis=1)))
    assert np.all(gmax <= G_TOL + E_grad[live].max(axis=1))
    if star is not None:
        fstar = probe.reference_loss_grad(Xs, Y, star, None, l2)[0]
        gap = (loss - fstar)[live]
        room = np.linalg.norm(grad[live], axis=1) * np.linalg.norm((theta - star)[live], axis=1) + 2 * E_loss[live]
        assert np.all(gap <= room) and np.all(gap >= -2 * E_loss[live]), (what, gap, room)


@pytest.mark.parametrize("case", FITS, ids=lambda c: ids(c[0]))
def test_fit_reaches_the_float64_optimum(dev, case):
    from chexpert_amd import probe
    X, Y, fit, Xs, star = fit_case(dev, case)
    theta = fit["theta"].cpu().numpy().astype(np.float64)
    print("iterations %s, passes %d, status %s" % (fit["iterations"], fit["passes"], fit["status"]))
    assert_fit(theta, fit["status"], Xs, Y, case[1], star, "fit %s" % (case,))
    assert tuple(fit["W"].shape) == (Y.shape[1], X.shape[1]) and tuple(fit["b"].shape) == (Y.shape[1],)
    assert np.array_equal(np.array(fit["count"])[:, 0], (Y >= 0).sum(0))
    # W, b are theta folded back to raw features in float64, rounded once
    W, b = probe.fold_back(theta, fit["mean"].cpu().numpy(), fit["rstd"].cpu().numpy())
    assert np.array_equal(fit["W"].cpu().numpy(), W.astype(np.float32)) and np.array_equal(fit["b"].cpu().numpy(), b.astype(np.float32))
    # predict_logits(X) = X W_raw^T + b_raw: the logit bound on the standardised operands plus the fold-back's one rounding
    z = probe.predict_logits(gpu(dev, X), fit).cpu().numpy()
    X64, d = X.astype(np.float64), X.shape[1]
    Wr, br = fit["W"].cpu().numpy().astype(np.float64), fit["b"].cpu().numpy().astype(np.float64)
    bound = (d + 2) * U * (np.abs(Xs.astype(np.float64)) @ np.abs(theta[:, :d]).T + np.abs(theta[:, d])) + \
        U * (np.abs(X64) @ np.abs(Wr).T + np.abs(br))
    assert np.all(np.abs(z - (X64 @ Wr.T + br)) <= bound)


def test_two_fits_give_equal_bits_and_the_path_warm_starts(dev):
    from chexpert_amd import probe
    case = FITS[0]
    X, Y, fit, Xs, star = fit_case(dev, case)
    again = probe.fit(gpu(dev, X), gpu(dev, Y), l2=case[1], g_tol=G_TOL)
    assert torch.equal(again["theta"].view(torch.int32), fit["theta"].view(torch.int32)) and torch.equal(again["W"], fit["W"])
    assert again["passes"] == fit["passes"] and again["iterations"] == fit["iterations"] and again["loss"] == fit["loss"]
    path = probe.fit_path(gpu(dev, X), gpu(dev, Y), (1e-2, 1e-3), g_tol=G_TOL)
    assert len(path) == 2
    for res, l2 in zip(path, (1e-2, 1e-3)):
        assert_fit(res["theta"].cpu().numpy().astype(np.float64), res["status"], Xs, Y, l2, probe.reference_optimum(Xs, Y, None, l2),
                   "path l2 %g" % l2)
    print("passes: cold %d, warm %d" % (fit["passes"], path[1]["passes"]))
    assert path[1]["passes"] <= fit["passes"]
    back = probe.fit_path(gpu(dev, X), gpu(dev, Y), (1e-3, 1e-2), g_tol=G_TOL)            # results in the order given, solved descending
    assert torch.equal(back[0]["theta"], path[1]["theta"]) and torch.equal(back[1]["theta"], path[0]["theta"])


def test_fit_without_standardisation(dev):
    """standardize=False on the same data: the raw X of fit_case (another scale, 0.5 .. 4, and offset, -2 .. 2, per column), the
    penalty on the raw weights, the conditions of assert_fit in raw coordinates against reference_optimum of the raw problem."""
    from chexpert_amd import probe
    case = FITS[0]
    X, Y, _, _, _ = fit_case(dev, case)
    fit = probe.fit(gpu(dev, X), gpu(dev, Y), l2=case[1], g_tol=G_TOL, standardize=False)
    print("iterations %s, passes %d, status %s, gmax %s" % (fit["iterations"], fit["passes"], fit["status"], fit["gmax"]))
    assert fit["mean"] is None and fit["rstd"] is None
    theta = fit["theta"].cpu().numpy()
    assert_fit(theta.astype(np.float64), fit["status"], X, Y, case[1], probe.reference_optimum(X, Y, None, case[1]), "raw coordinates")
    assert np.array_equal(fit["W"].cpu().numpy(), theta[:, :-1]) and np.array_equal(fit["b"].cpu().numpy(), theta[:, -1])


# ---- end to end ------------------------------------------------------------------------------------------------------------------------
def small_model(dev, storage, n_cls=5):
    from chexpert_amd.models import densenet121
    from oracle import nets
    model = densenet121(num_classes=n_cls)
    sd = synth.fill_state_dict_(nets.zeros_state_dict(nets.densenet_spec(n_cls)), 21)
    model.storage_dtype(storage).load_state_dict(sd, strict=True)
    return model.to(dev).eval()


def classifier_bound(feats, W, b):
    """The bound of assert_classifier_reads (test_knn_gpu): any fp32 summation of C products and the bias."""
    return (W.shape[1] + 2) * U * (np.abs(feats) @ np.abs(W).T + np.abs(b))


@pytest.mark.parametrize("n", [5, 3], ids=["same_width", "resized"])
@pytest.mark.parametrize("storage", ["bf16", "fp32"])
def test_load_into_makes_the_model_the_probe(dev, storage, n):
    """After load_into, model(x) equals predict_logits(model.embed(x), fit) within the bound of assert_classifier_reads; each of the
    two is also within its own fp32 bound of the float64 value.  n = 5 is the model's width: the live engine's flat buffers must
    see the new values; n = 3 replaces the classifier."""
    from chexpert_amd import probe
    model = small_model(dev, storage)
    x = synth.xray_batch(3, 12, 64).to(dev)
    feats = model.embed(x)
    labels = torch.from_numpy((np.random.default_rng(5).random((12, n)) < 0.5).astype(np.float32))
    fit = probe.fit(feats, labels, l2=1e-2, max_iter=20)
    before = {k: v.clone() for k, v in model.state_dict().items()}
    assert probe.load_into(model, fit) is model
    fc = [m for m in model.modules() if isinstance(m, torch.nn.Linear)][-1]
    assert fc.out_features == n and torch.equal(fc.weight.detach(), fit["W"]) and torch.equal(fc.bias.detach(), fit["b"])
    after = model.state_dict()
    assert all(torch.equal(before[k], after[k]) for k in before if not k.startswith("classifier."))
    assert torch.equal(model.embed(x), feats)
    with torch.no_grad():
        out = model(x).double().cpu().numpy()
    f64 = feats.double().cpu().numpy()
    W, b = fit["W"].double().cpu().numpy(), fit["b"].double().cpu().numpy()
    exact = f64 @ W.T + b
    head = classifier_bound(f64, W, b)
    assert np.all(np.abs(out - exact) <= head)
    theta = fit["theta"].double().cpu().numpy()
    Xs = ((f64 - fit["mean"].double().cpu().numpy()) * fit["rstd"].double().cpu().numpy())
    z = probe.predict_logits(feats, fit).double().cpu().numpy()
    mine = classifier_bound(Xs, theta[:, :-1], theta[:, -1]) + U * (np.abs(f64) @ np.abs(W).T + np.abs(b))
    assert np.all(np.abs(z - exact) <= mine)
    print("largest |model(x) - predict_logits| / bound: %.4f" % (np.abs(z - out) / head).max())
    assert np.all(np.abs(z - out) <= head)


_CLI = ["--synthetic", "8", "--batch_size", "4", "--resize", "64"]
_TRAIN = ["--train", "--eval_interval", "2", "--log_interval", "1", "--seed", "3", "--lr", "0.001", "--fused_optimizer"]


def test_cli_probe_save_and_restore(dev, tmp_path, capsys):
    from chexpert_amd import cli, knn, probe
    out = str(tmp_path / "s")
    cli.main(_CLI + _TRAIN + ["--output_dir", out])
    ev, saved = str(tmp_path / "e"), str(tmp_path / "probe" / "fitted.pt")
    model = cli.main(["--evaluate_single_model"] + _CLI + ["--restore", os.path.join(out, "checkpoint_latest.pt"), "--output_dir", ev,
                                                           "--linear_probe", "--probe_l2", "0.01", "--probe_bank", "0", "--probe_save", saved])
    assert "linear probe @ step 2" in capsys.readouterr().out
    files = glob.glob(os.path.join(ev, "probe_*.json"))
    assert [os.path.basename(f) for f in files] == ["probe_step_2.json"] and os.path.exists(os.path.join(ev, "eval_results_step_2.json"))
    res = json.load(open(files[0]))
    assert set(res) == {"bank", "l2", "fits"} and res["bank"] == 8 and res["l2"] == [0.01] and len(res["fits"]) == 1
    f = res["fits"][0]
    assert set(f) == {"l2", "aucs", "mean_auc", "status", "iterations", "passes", "train_loss"}
    assert set(f["aucs"]) == {str(c) for c in range(5)} and len(f["status"]) == 5 and len(f["train_loss"]) == 5
    # the saved checkpoint: the source's weights and step, the classifier the fit, nothing of the optimiser or the loss
    src, ck = torch.load(os.path.join(out, "checkpoint_latest.pt"), map_location="cpu"), torch.load(saved, map_location="cpu")
    assert ck["global_step"] == src["global_step"] == 2 and "loss_state" not in ck and set(ck["state_dict"]) == set(src["state_dict"])
    wk, bk = cli.classifier_keys(model)
    assert all(torch.equal(ck["state_dict"][k], src["state_dict"][k]) for k in src["state_dict"] if k not in (wk, bk))
    assert tuple(ck["state_dict"][wk].shape) == (5, 1024) and not torch.equal(ck["state_dict"][wk], src["state_dict"][wk])
    # ... is the fit of the bank the command line embedded
    train_ds, valid_ds = cli.SyntheticXrays(8, 64, 5, 7), cli.SyntheticXrays(4, 64, 5, 11)
    bank, labels = knn.embed_dataset(model, train_ds, range(8), 4, dev)
    q, targets = knn.embed_dataset(model, valid_ds, range(4), 4, dev)
    fit = probe.fit(bank, labels, l2=0.01)
    assert torch.equal(fit["W"].cpu(), ck["state_dict"][wk]) and torch.equal(fit["b"].cpu(), ck["state_dict"][bk])
    assert f["status"] == fit["status"] and f["passes"] == fit["passes"]
    # it restores with a plain --evaluate_single_model, whose logits are the probe's within the bound of assert_classifier_reads
    ev2 = str(tmp_path / "e2")
    restored = cli.main(["--evaluate_single_model"] + _CLI + ["--restore", saved, "--output_dir", ev2])
    with torch.no_grad():
        z_model = restored.eval()(torch.stack([valid_ds[i][0] for i in range(4)]).to(dev)).double().cpu().numpy()
    z_probe = probe.predict_logits(q, fit).double().cpu().numpy()
    f64, W, b = q.double().cpu().numpy(), fit["W"].double().cpu().numpy(), fit["b"].double().cpu().numpy()
    bound = classifier_bound(f64, W, b)
    assert np.all(np.abs(z_model - z_probe) <= bound)
    res2 = json.load(open(os.path.join(ev2, "eval_results_step_2.json")))
    assert not glob.glob(os.path.join(ev2, "probe_*.json"))
    for c in range(5):
        a, p = res2["aucs"][str(c)], f["aucs"][str(c)]
        col, margin = np.sort(z_probe[:, c]), 2 * bound[:, c].max()
        if (np.diff(col) > margin).all():                                       # no two scores within the bound: the ranks are the same
            assert (math.isnan(a) and math.isnan(p)) or a == pytest.approx(p, abs=1e-12), (c, a, p)


def test_cli_pretraining_reports_the_linear_probe(dev, tmp_path, capsys):
    from chexpert_amd import cli
    out = str(tmp_path / "p")
    pre = ["--pretrain", "contrastive", "--proj_dim", "16", "--affine", "--jitter"]
    cli.main(_CLI + _TRAIN + pre + ["--linear_probe", "--probe_l2", "0.1", "0.01", "--probe_bank", "0", "--probe_max_iter", "30",
                                    "--knn_probe", "3", "--knn_bank", "0", "--output_dir", out])
    text = capsys.readouterr().out
    res = json.load(open(os.path.join(out, "pretrain_eval_step_2.json")))
    got = res["linear_probe"]
    assert set(got) == {"bank", "l2", "fits"} and got["bank"] == 8 and got["l2"] == [0.1, 0.01] and [f["l2"] for f in got["fits"]] == [0.1, 0.01]
    assert all(set(f["aucs"]) == {str(c) for c in range(5)} and len(f["status"]) == 5 for f in got["fits"])
    assert all(math.isnan(v) or 0.0 <= v <= 1.0 for f in got["fits"] for v in f["aucs"].values())
    lines = text.count("linear probe @ step 2")                              # one line per value of --probe_l2 at every evaluation
    assert lines >= 2 and lines % 2 == 0 and "kNN probe @ step 2" in text and res["knn"]["bank"] == 8
