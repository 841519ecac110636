"""CPU (no GPU, no library): the float64 definitions of the linear probe (chexpert_amd/probe.py) and the command line's checks of
--linear_probe and its flags."""
import argparse

import numpy as np
import pytest

from chexpert_amd import probe


def small_problem(seed=0):
    """7 rows x 3 columns x 2 classes with an ignored label, a soft label and pos_weight != 1."""
    rng = np.random.default_rng(seed)
    X = rng.standard_normal((7, 3))
    Y = (rng.random((7, 2)) < 0.5).astype(np.float64)
    Y[0, 0], Y[1, 0] = 1.0, 0.0                     # both kinds are live in both classes
    Y[2, 1], Y[3, 1] = 1.0, 0.0
    Y[4, 0] = -1.0                                  # ignored
    Y[5, 1] = 0.3                                   # soft
    theta = rng.standard_normal((2, 4)) * 0.4
    return X, Y, theta, np.array([2.0, 0.7])


def test_gradient_against_central_differences_of_its_own_loss():
    X, Y, theta, pw = small_problem()
    l2, h = 0.05, 1e-6
    loss, grad, E_loss, E_grad = probe.reference_loss_grad(X, Y, theta, pw, l2)
    assert loss.shape == (2,) and grad.shape == (2, 4) and (E_loss > 0).all() and (E_grad > 0).all()
    for c in range(2):
        for k in range(4):
            e = np.zeros_like(theta)
            e[c, k] = h
            up, dn = probe.reference_loss_grad(X, Y, theta + e, pw, l2)[0], probe.reference_loss_grad(X, Y, theta - e, pw, l2)[0]
            num = (up - dn) / (2 * h)
            assert abs(num[c] - grad[c, k]) <= 1e-8 * max(1.0, abs(grad[c, k])), (c, k, num[c], grad[c, k])
            assert num[1 - c] == 0.0                                           # the classes do not couple
    # the ignored row is no row of its class: changing its features moves class 1 only
    X2 = X.copy()
    X2[4] += 10.0
    l2_, g2 = probe.reference_loss_grad(X2, Y, theta, pw, l2)[:2]
    assert l2_[0] == loss[0] and np.array_equal(g2[0], grad[0]) and l2_[1] != loss[1]
    # the bias is not regularised: at theta = 0 the loss is log 2 weighted and l2 plays no part
    z = np.zeros_like(theta)
    assert np.array_equal(probe.reference_loss_grad(X, Y, z, pw, 0.0)[1], probe.reference_loss_grad(X, Y, z, pw, 3.0)[1])


def test_reference_optimum_is_a_stationary_point():
    rng = np.random.default_rng(1)
    X = rng.standard_normal((60, 5))
    planted = rng.standard_normal((3, 6))
    Y = (rng.random((60, 3)) < 1 / (1 + np.exp(-(X @ planted[:, :5].T + planted[:, 5])))).astype(np.float64)
    Y[rng.random(Y.shape) < 0.1] = -1.0
    Y[:5, 1] = rng.random(5)
    pw = np.array([1.0, 2.5, 0.5])
    for l2 in (1e-2, 1e-4):
        star = probe.reference_optimum(X, Y, pw, l2)
        loss, grad = probe.reference_loss_grad(X, Y, star, pw, l2)[:2]
        assert np.abs(grad).max() < 1e-12
        other = star + 1e-3 * rng.standard_normal(star.shape)
        assert (probe.reference_loss_grad(X, Y, other, pw, l2)[0] > loss).all()          # strictly convex: the minimum


def test_degenerate_classes_are_reported():
    Y = np.array([[1, 0, -1, 1, 0.0], [0, 0, -1, 1, 0.5], [1, -1, -1, 1, 1.0]], dtype=np.float64)
    # both kinds; all negative; all ignored; all positive; soft labels carry both masses
    assert probe.degenerate(Y).tolist() == [False, True, True, True, False]
    X = np.random.default_rng(2).standard_normal((3, 2))
    star = probe.reference_optimum(X, Y, None, 0.1)
    assert not star[[1, 2, 3]].any() and star[0].any() and star[4].any()
    loss, grad = probe.reference_loss_grad(X, Y, np.zeros((5, 3)), None, 0.1)[:2]
    assert loss[2] == 0.0 and not grad[2].any()                                 # no live row: N_c = 1, nothing summed


def test_fold_back_reproduces_the_standardised_logits():
    rng = np.random.default_rng(3)
    X = rng.standard_normal((40, 6)) * rng.uniform(0.1, 30, size=6) + rng.uniform(-5, 5, size=6)
    X[:, 2] = 4.25                                                              # a dead channel
    mean, std, rstd = probe.reference_colstats(X)
    assert std[2] == 0.0 and rstd[2] == 1e6 and np.allclose(mean, X.mean(0)) and np.allclose(std, X.std(0))
    Xs = (X - mean) * rstd
    assert not Xs[:, 2].any() and np.allclose(Xs.std(0)[[0, 1, 3, 4, 5]], 1.0)
    theta = rng.standard_normal((4, 7))
    W, b = probe.fold_back(theta, mean, rstd)
    want = Xs @ theta[:, :6].T + theta[:, 6]
    got = X @ W.T + b
    scale = np.abs(X) @ np.abs(W).T + np.abs(b)
    assert np.all(np.abs(got - want) <= 16 * 2.0 ** -53 * scale)


def _args(**kw):
    base = dict(linear_probe=False, probe_l2=None, probe_bank=None, probe_max_iter=None, probe_save=None, pretrain=None,
                evaluate_single_model=False, head=None, uncertain="ones", loss="bce")
    base.update(kw)
    return argparse.Namespace(**base)


def test_every_refusal_names_its_flag_without_a_gpu():
    from chexpert_amd import cli
    ok = dict(linear_probe=True, evaluate_single_model=True)
    assert cli.probe_options(_args()) is None
    assert cli.probe_options(_args(**ok)) == {"l2": [1e-3], "bank": 8192, "max_iter": 200, "save": None}
    assert cli.probe_options(_args(linear_probe=True, pretrain="contrastive", probe_l2=[0.1, 0.0], probe_bank=0, probe_max_iter=7)) == \
        {"l2": [0.1, 0.0], "bank": 0, "max_iter": 7, "save": None}
    assert cli.probe_options(_args(probe_l2=[0.5], probe_save="f.pt", **ok))["save"] == "f.pt"
    refused = [
        (dict(probe_l2=[0.1]), "--linear_probe"), (dict(probe_bank=4), "--linear_probe"), (dict(probe_max_iter=4), "--linear_probe"),
        (dict(probe_save="f.pt"), "--linear_probe"),
        (dict(linear_probe=True), "--evaluate_single_model"),
        (dict(head="csra", **ok), "--head csra"), (dict(head="pcam", **ok), "--head pcam"),
        (dict(uncertain="multiclass", **ok), "--uncertain multiclass"), (dict(loss="hier", **ok), "--loss hier"),
        (dict(probe_l2=[0.1, -1e-3], **ok), "--probe_l2"), (dict(probe_l2=[float("nan")], **ok), "--probe_l2"),
        (dict(probe_l2=[float("inf")], **ok), "--probe_l2"),
        (dict(probe_bank=-1, **ok), "--probe_bank"), (dict(probe_max_iter=0, **ok), "--probe_max_iter"),
        (dict(probe_save="f.pt", probe_l2=[0.1, 0.2], **ok), "--probe_save"),
        (dict(probe_save="f.pt", linear_probe=True, pretrain="contrastive"), "--probe_save"),
    ]
    for kw, flag in refused:
        with pytest.raises(ValueError, match=flag):
            cli.probe_options(_args(**kw))
    with pytest.raises(ValueError, match="more than one rank"):
        cli.probe_options(_args(**ok), world=2)
    # the Python entry points refuse what the flags refuse
    with pytest.raises(ValueError, match="l2"):
        probe._check_l2(-1.0)
    with pytest.raises(ValueError, match="l2"):
        probe._check_l2(float("nan"))


def test_the_parser_accepts_the_flags_and_check_flags_resolves_them():
    from chexpert_amd import cli
    a = cli.build_parser().parse_args(["--evaluate_single_model", "--linear_probe", "--probe_l2", "0.01", "0.001", "--probe_bank", "0",
                                       "--probe_max_iter", "50", "--probe_save", "out.pt"])
    assert a.linear_probe and a.probe_l2 == [0.01, 0.001] and a.probe_bank == 0 and a.probe_max_iter == 50 and a.probe_save == "out.pt"
    b = cli.build_parser().parse_args([])
    assert not b.linear_probe and b.probe_l2 is None and b.probe_bank is None and b.probe_max_iter is None and b.probe_save is None
    run = cli.check_flags(["--evaluate_single_model", "--synthetic", "8", "--linear_probe", "--knn_probe", "3"])
    assert run.probe == {"l2": [1e-3], "bank": 8192, "max_iter": 200, "save": None} and run.knn["k"] == 3
    assert cli.check_flags(["--evaluate_single_model", "--synthetic", "8"]).probe is None
    with pytest.raises(ValueError, match="--linear_probe"):
        cli.check_flags(["--evaluate_single_model", "--synthetic", "8", "--probe_l2", "0.1"])
    assert "--linear_probe" in cli.__doc__ and "probe_l2" in cli.build_parser().format_help()
