"""Barlow Twins pretraining without a GPU: the float64 statement of the loss (loss.reference_barlow) against an independent torch
statement, finite differences and its closed forms, the tolerance the GPU tests hold the kernels to (derived here, and met here by a
float32 evaluation of the statement on the GPU tests' inputs), set_loss / BarlowTwinsLoss / the C entry point's refusals, the command
line's refusals and defaults, and the checkpoint kind check."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

from chexpert_amd import loss as L

U = 2.0 ** -24            # the unit roundoff of fp32


# ------------------------------------------------------------------------------------------------ the cases the GPU tests share
SHAPES = [(4, 8), (6, 5), (8, 16), (13, 7), (64, 32), (66, 33), (130, 136), (258, 64), (512, 128), (128, 1024), (4096, 16)]
LAMBDAS = [0.0051, 1.0]
LAYOUTS = ["full", "negative"]
_CASES = {}


def ids_of(layout, N):
    """full: row p and row p + N // 2 carry the id p (an odd last row an id of its own); negative: every third row's id is -1, which
    takes its pair out of the batch."""
    h = N // 2
    ids = np.where(np.arange(N) < 2 * h, np.arange(N) % max(h, 1), N).astype(np.float64)
    return ids if layout == "full" else np.where(np.arange(N) % 3 == 1, -1.0, ids)


def case(N, d, layout):
    """fp32 embeddings of two views: a shared, column-correlated base plus 0.3 noise per view, every column with its own scale
    exp(U(-2, 2)) and an offset of up to 3 of its standard deviations (so a - mu cancels digits), and the ids.  Made once per case."""
    key = (N, d, layout)
    if key not in _CASES:
        rng = np.random.default_rng(7000 * N + 10 * d + LAYOUTS.index(layout))
        h = N // 2
        mix = np.eye(d) + 0.5 * rng.standard_normal((d, d)) / np.sqrt(d)
        base = rng.standard_normal((h, d)) @ mix
        rows = np.concatenate([base + 0.3 * rng.standard_normal((h, d)), base + 0.3 * rng.standard_normal((h, d)),
                               rng.standard_normal((N - 2 * h, d))])
        scale, offset = np.exp(rng.uniform(-2, 2, d)), rng.uniform(-3, 3, d)
        std = np.sqrt(np.diag(mix.T @ mix) + 0.09)
        e = ((rows + offset * std) * scale).astype(np.float32)
        e.setflags(write=False)
        _CASES[key] = (e, ids_of(layout, N))
    return _CASES[key]


def tolerance(e, ids, lambd, ref=None):
    """What an fp32 evaluation of the statement may differ from the float64 one by, from rounding alone (u = 2^-24), whatever the order
    of its sums.  n = m terms enter a column's sums; for view x in {a, b} and column k let A_k = max_p |x_pk|, s_k = sqrt(v_k + eps),
    R_k = A_k / s_k and H_k = max_p |x^_pk| (float64 statement).  First order in u, second-order terms kept where they are cheap, the
    whole multiplied by 1.01 for the rest:

      mean           a sum of n terms and a divide:  |d mu| <= n u A_k,  i.e. n u R_k in units of s_k
      centring       c = a - mu:  |dc| <= |d mu| + u |c|: THE cancellation, in terms of max |a_.k| / sqrt(v_k + eps)
      variance       sum (c + dc)^2: the d mu part of dc is constant over p and sum c = 0, so it enters at second order only;
                     rho_k = (n + 5) u + 1.1 (n u R_k)^2 + 2 u (n u R_k)  relative on v_k + eps (sum, squares, divide, the + eps)
      1 / sqrt       iota_k = 0.51 rho_k + 6 u  (square root and reciprocal, 2.5 ulp allowed for each)
      x^             eps_k = 1.01 n u R_k + H_k (iota_k + 2 u)                                   absolute, on every element of column k
      C_kl           a sum of n products and a divide, with sum_p |a^ b^| <= m (Cauchy-Schwarz; mean a^^2 <= 1):
                     EC_kl = eps^a_k + eps^b_l + eps^a_k eps^b_l + (n + 2) u (1 + eps^a_k) (1 + eps^b_l)
      on             t_k = 1 - C_kk has dt = EC_kk + u |t_k|; sum_k [2 |t_k| dt + dt^2] + (d + 34) u on.  No term passes through more
                     than d + 32 additions in an fp32 evaluation that sums a row and then the rows (numpy) or 16 values in a lane,
                     6 butterfly levels, 4 waves and the tiles in double (the kernels); the rest is the square and the cast
      off            sum_{k != l} [2 |C_kl| EC_kl + EC_kl^2] + (2 d + 34) u off, likewise
      loss           tol_on + lambda tol_off + 2 u loss;     mean_diag: mean_k EC_kk + (d + 34) u mean_k |C_kk|
      G              EG_kk = 2 dt_k;  EG_kl = 2 lambda (EC_kl + 2 u |C_kl|)
      dx^_pk         = sum_l y^_pl G_kl / m (y the other view; for view b the transposed G), a sum of d products:
                     E1_pk = [sum_l (eps^y_l (|G_kl| + EG_kl) + |y^_pl| EG_kl) + (d + 2) u sum_l (|y^_pl| + eps^y_l)(|G_kl| + EG_kl)] / m
                     -- ABSOLUTE, through sum_l |G_kl|: with m = 2 every x^ is +-1 and the gradient is almost pure cancellation
      the two means  mean_p dx^ (0 in exact arithmetic, and in the kernels) as an fp32 sum:  Em_k = mean_p E1_pk + (n + 1) u mean_p |dx^_pk|
                     t_k = mean_p (dx^ o x^)_k, either as that sum, Et = mean_p (E1 |x^| + |dx^| eps + E1 eps) + (n + 2) u mean_p |dx^ x^|,
                     or in its closed form sum_l G_kl C_kl / m, Et = [sum_l (EG |C| + |G| EC + EG EC) + (d + 19) u sum_l (|G| + EG)
                     (|C| + EC)] / m: the larger of the two
      dx_pk          = (dx^ - mean - x^ t) / s_k:
                     E_pk = [E1_pk + Em_k + eps_k |t_k| + (|x^_pk| + eps_k) Et_k + 3 u (|dx^_pk| + |x^_pk t_k|)] / s_k + (iota_k + 2 u) |dx_pk|
                     and the gradient row is held in the 2-norm: tol_p = |E_p.|_2

    Returns {"loss", "on", "off", "mean_diag": floats, "grad": (N,) (0 for a row outside the batch: exact zeros are asked of it)}."""
    e = np.asarray(e)
    N, d = e.shape
    h = N // 2
    ref = ref or L.reference_barlow(e, ids, lambd)
    m = ref["m"]
    out = {"loss": 0.0, "on": 0.0, "off": 0.0, "mean_diag": 0.0, "grad": np.zeros(N)}
    if m < 2:
        return out
    lam = float(np.float32(lambd))
    n, valid, C = m, ref["valid"], ref["C"]
    views = [e[:h][valid].astype(np.float64), e[h:2 * h][valid].astype(np.float64)]
    hats, istd = [ref["ahat"], ref["bhat"]], ref["istd"]
    eps, iota = [], []
    for x, xh, s_inv in zip(views, hats, istd):
        R = np.abs(x).max(0) * s_inv
        rho = (n + 5) * U + 1.1 * (n * U * R) ** 2 + 2 * U * (n * U * R)
        iota.append(0.51 * rho + 6 * U)
        eps.append(1.01 * n * U * R + np.abs(xh).max(0) * (iota[-1] + 2 * U))
    EC = eps[0][:, None] + eps[1][None, :] + eps[0][:, None] * eps[1][None, :] + (n + 2) * U * (1 + eps[0][:, None]) * (1 + eps[1][None, :])
    eye = np.eye(d, dtype=bool)
    t = 1.0 - np.diag(C)
    dt = np.diag(EC) + U * np.abs(t)
    on_terms = (2 * np.abs(t) * dt + dt ** 2).sum()
    out["on"] = 1.01 * (on_terms + (d + 34) * U * (ref["on"] + on_terms))
    off_terms = np.where(eye, 0.0, 2 * np.abs(C) * EC + EC ** 2).sum()
    out["off"] = 1.01 * (off_terms + (2 * d + 34) * U * (ref["off"] + off_terms))
    out["loss"] = out["on"] + lam * out["off"] + 2 * U * abs(ref["loss"])
    out["mean_diag"] = 1.01 * (np.diag(EC).mean() + (d + 34) * U * np.abs(np.diag(C)).mean())
    G = np.where(eye, -2.0 * (1.0 - C), 2.0 * lam * C)
    EG = np.where(eye, 2.0 * dt[:, None], 2.0 * lam * (EC + 2 * U * np.abs(C)))
    rows = np.flatnonzero(valid)
    for view in (0, 1):
        Gv, EGv, Cv, ECv = (G, EG, C, EC) if view == 0 else (G.T, EG.T, C.T, EC.T)       # [own column][the other view's column]
        xh, yh, ex, ey = np.abs(hats[view]), np.abs(hats[1 - view]), eps[view], eps[1 - view]
        GA = np.abs(Gv) + EGv
        dxh = (hats[1 - view] @ Gv.T) / m
        E1 = ((ey[None, :] * GA).sum(1)[None, :] + yh @ EGv.T + (d + 2) * U * ((yh + ey[None, :]) @ GA.T)) / m
        Em = E1.mean(0) + (n + 1) * U * np.abs(dxh).mean(0)
        tk = (Gv * Cv).sum(1) / m
        Et_sum = (E1 * xh + np.abs(dxh) * ex[None, :] + E1 * ex[None, :]).mean(0) + (n + 2) * U * np.abs(dxh * hats[view]).mean(0)
        Et_closed = ((EGv * np.abs(Cv) + np.abs(Gv) * ECv + EGv * ECv).sum(1) + (d + 19) * U * (GA * (np.abs(Cv) + ECv)).sum(1)) / m
        Et = np.maximum(Et_sum, Et_closed)
        dx = ref["grad"][rows + view * h]
        E = (E1 + Em[None, :] + ex[None, :] * np.abs(tk)[None, :] + (xh + ex[None, :]) * Et[None, :]
             + 3 * U * (np.abs(dxh) + xh * np.abs(tk)[None, :])) * istd[view][None, :] + (iota[view] + 2 * U)[None, :] * np.abs(dx)
        out["grad"][rows + view * h] = 1.01 * np.sqrt((E ** 2).sum(1))
    return out


def check_against(ref, tol, loss, stats, grad, what="", grad_scale=1.0):
    """loss, stats (4,) = [on, off, mean_diag, m] and the gradient (N, d) against the float64 statement, within `tol`; each may be
    None.  Rows outside the batch must be exact zeros.  Returns the largest ratio error / tolerance seen."""
    worst = 0.0
    pairs = []
    if loss is not None:
        pairs.append(("loss", float(loss), ref["loss"], tol["loss"]))
    if stats is not None:
        stats = np.asarray(stats, dtype=np.float64).reshape(-1)
        assert stats[3] == ref["m"], (what, "m", stats[3], ref["m"])
        pairs += [(k, stats[i], ref[k], tol[k]) for i, k in enumerate(("on", "off", "mean_diag"))]
    for name, got, want, bound in pairs:
        print("%s %-9s got %.9g want %.9g err %.3e tol %.3e" % (what, name, got, want, abs(got - want), bound))
        assert abs(got - want) <= bound, (what, name, got, want, bound)
        worst = max(worst, abs(got - want) / bound if bound else 0.0)
    if grad is not None:
        grad = np.asarray(grad, dtype=np.float64)
        rows = np.sqrt(((grad - grad_scale * ref["grad"]) ** 2).sum(1))
        bound = grad_scale * tol["grad"] + 2 * U * grad_scale * np.sqrt((ref["grad"] ** 2).sum(1)) * (grad_scale != 1.0)
        out_rows = bound == 0
        ratio = float((rows[~out_rows] / bound[~out_rows]).max()) if (~out_rows).any() else 0.0
        print("%s grad      largest row error / tolerance %.4f, largest row norm %.3e, largest tolerance %.3e"
              % (what, ratio, float(np.sqrt((ref["grad"] ** 2).sum(1)).max()), float(bound.max())))
        assert np.all(rows <= bound), (what, "grad", ratio, int(np.argmax(rows - bound)))
        assert not grad[out_rows].any(), (what, "a row outside the batch has a gradient")
        worst = max(worst, ratio)
    return worst


@pytest.mark.parametrize("N,d", SHAPES)
def test_a_float32_evaluation_stays_inside_the_tolerance(N, d):
    """The GPU tests' inputs and bound: the statement evaluated in float32 numpy (another order of every sum than the kernels') meets
    the float64 one within it at every shared case, and the inputs are what the issue says they are."""
    for layout in LAYOUTS:
        e, ids = case(N, d, layout)
        for lambd in LAMBDAS:
            ref = L.reference_barlow(e, ids, lambd)
            tol = tolerance(e, ids, lambd, ref)
            r32 = L.reference_barlow(e, ids, lambd, dtype=np.float32)
            assert r32["m"] == ref["m"]
            check_against(ref, tol, r32["loss"], [r32["on"], r32["off"], r32["mean_diag"], r32["m"]], r32["grad"], (N, d, lambd, layout))
            if ref["m"] < 2:
                assert layout == "negative" and (N, d) in ((4, 8), (8, 16)) and ref["loss"] == 0 and not ref["grad"].any()
            else:
                assert max(np.abs(ref["ahat"]).max(), np.abs(ref["bhat"]).max()) <= 4.5
                # the bound is a worst-case rounding bound (linear in the pairs: 2048 of them at the row cap), yet below a tenth of
                # the quantity it guards at every case
                assert tol["loss"] < 0.1 * ref["loss"] and ref["loss"] > 0
    assert L.reference_barlow(*case(6, 5, "negative"), 1.0)["m"] == 2 and L.reference_barlow(*case(4, 8, "full"), 1.0)["m"] == 2


# ------------------------------------------------------------------------------------------------ the statement
def _barlow_torch(e, lambd):
    """An independent statement: BatchNorm1d(affine=False) in training mode on each view, a matmul, autograd."""
    x = torch.tensor(np.asarray(e, dtype=np.float64), requires_grad=True)
    h = x.shape[0] // 2
    a = F.batch_norm(x[:h], None, None, training=True, eps=1e-5)
    b = F.batch_norm(x[h:2 * h], None, None, training=True, eps=1e-5)
    c = a.T @ b / h
    on = ((1 - torch.diagonal(c)) ** 2).sum()
    off = (c ** 2).sum() - (torch.diagonal(c) ** 2).sum()
    loss = on + float(np.float32(lambd)) * off
    loss.backward()
    return loss.item(), on.item(), off.item(), c.detach().numpy(), x.grad.numpy()


@pytest.mark.parametrize("N,d", [(4, 3), (6, 5), (12, 5), (13, 7), (40, 16)])
@pytest.mark.parametrize("lambd", [0.0, 0.0051, 1.0])
def test_reference_is_batchnorm_matmul_and_autograd(N, d, lambd):
    rng = np.random.default_rng(N * 100 + d)
    e = rng.standard_normal((N, d)) * np.exp(rng.uniform(-1, 1, d)) + rng.uniform(-2, 2, d)
    ref = L.reference_barlow(e, np.arange(N), lambd)
    loss, on, off, c, grad = _barlow_torch(e[:2 * (N // 2)], lambd)
    assert ref["m"] == N // 2
    assert ref["loss"] == pytest.approx(loss, rel=1e-12) and ref["on"] == pytest.approx(on, rel=1e-12) and ref["off"] == pytest.approx(off, rel=1e-10, abs=1e-14)
    assert np.allclose(ref["C"], c, rtol=0, atol=1e-13)
    assert np.allclose(ref["grad"][:2 * (N // 2)], grad, rtol=1e-9, atol=1e-12 * max(np.abs(grad).max(), 1e-300))
    if N % 2:
        assert not ref["grad"][-1].any()


def test_reference_against_finite_differences():
    rng = np.random.default_rng(5)
    e = rng.standard_normal((12, 5)) + rng.uniform(-1, 1, 5)
    ids = np.arange(12.0) % 6
    ids[2] = -1                                                                         # pair 2 (rows 2 and 8) is out of the batch
    ref = L.reference_barlow(e, ids, 0.3)
    num = np.zeros_like(e)
    for i in range(12):
        for j in range(5):
            hi, lo = e.copy(), e.copy()
            hi[i, j] += 1e-6
            lo[i, j] -= 1e-6
            num[i, j] = (L.reference_barlow(hi, ids, 0.3)["loss"] - L.reference_barlow(lo, ids, 0.3)["loss"]) / 2e-6
    assert ref["m"] == 5 and np.abs(num - ref["grad"]).max() < 1e-8 * max(1.0, np.abs(ref["grad"]).max())
    assert not ref["grad"][2].any() and not ref["grad"][8].any() and np.abs(ref["grad"]).max() > 0


def test_closed_forms():
    """The two facts the kernels use: mean_p da^ = 0 and mean_p (da^ o a^)_k = sum_l G_kl C_kl / m (for view B the column sums), so
    BatchNorm's backward is an epilogue of the product; identical views give C_kk = v / (v + eps) and a zero `on` up to eps."""
    e, ids = case(66, 33, "negative")
    for lambd in LAMBDAS:
        ref = L.reference_barlow(e, ids, lambd)
        m, C, ah, bh = ref["m"], ref["C"], ref["ahat"], ref["bhat"]
        lam = float(np.float32(lambd))
        G = np.where(np.eye(33, dtype=bool), -2 * (1 - C), 2 * lam * C)
        dah, dbh = bh @ G.T / m, ah @ G / m
        assert np.abs(dah.mean(0)).max() < 1e-14 and np.abs(dbh.mean(0)).max() < 1e-14
        assert np.allclose((dah * ah).mean(0), (G * C).sum(1) / m, rtol=0, atol=1e-14)
        assert np.allclose((dbh * bh).mean(0), (G * C).sum(0) / m, rtol=0, atol=1e-14)
        rows = np.flatnonzero(ref["valid"])
        closed_a = (dah - ah * ((G * C).sum(1) / m)) * ref["istd"][0]
        closed_b = (dbh - bh * ((G * C).sum(0) / m)) * ref["istd"][1]
        assert np.allclose(ref["grad"][rows], closed_a, rtol=0, atol=1e-15 * np.abs(closed_a).max() + 1e-18)
        assert np.allclose(ref["grad"][rows + 33], closed_b, rtol=0, atol=1e-15 * np.abs(closed_b).max() + 1e-18)
    x = np.random.default_rng(1).standard_normal((20, 6))
    same = L.reference_barlow(np.concatenate([x, x]), np.arange(40), 0.0051)
    v = x.var(0)
    assert np.allclose(np.diag(same["C"]), v / (v + 1e-5), rtol=1e-12) and same["on"] < 1e-8 and same["mean_diag"] == pytest.approx(1.0, abs=1e-4)


def test_exact_zeros_and_a_constant_column():
    e, _ = case(13, 7, "full")
    for ids in (-np.ones(13), np.array([0, -1, -1, -1, -1, -1, 0, 1, 2, 3, 4, 5, 9.0]), np.array([0, 1, 2, 3, 4, 5, -1, -1, -1, -1, -1, -1, 3.0])):
        ref = L.reference_barlow(e, ids, 1.0)
        assert ref["m"] < 2 and ref["loss"] == 0 and ref["on"] == 0 and ref["off"] == 0 and not ref["grad"].any()
    full = L.reference_barlow(e, np.arange(13), 1.0)
    assert full["m"] == 6 and not full["grad"][12].any() and np.abs(full["grad"][:12]).min() > 0
    poisoned = e.copy()
    poisoned[12] = np.nan                                                               # the odd row is never read
    again = L.reference_barlow(poisoned, np.arange(13), 1.0)
    assert again["loss"] == full["loss"] and np.array_equal(again["grad"], full["grad"])
    const = e.copy()
    const[:, 3] = 2.5
    ref = L.reference_barlow(const, np.arange(13), 1.0)
    assert np.isfinite(ref["grad"]).all() and np.isfinite(ref["loss"]) and ref["C"][3, 3] == 0 and not ref["C"][3].any() and not ref["C"][:, 3].any()


# ------------------------------------------------------------------------------------------------ refusals that need no GPU
def test_set_loss_refuses_without_changing_anything():
    state = L.Loss()
    cpu = torch.device("cpu")
    for kw in (dict(kind="barlow", pos_weight=[1.0] * 8), dict(kind="barlow", ignore_negative=True), dict(kind="barlow", lambd=-0.1),
               dict(kind="barlow", lambd=float("nan")), dict(kind="barlow", lambd=float("inf")), dict(kind="barlow", lambd="x"),
               dict(kind="barlow", temperature=0.2), dict(kind="barlow", gamma=2.0), dict(kind="barlow", clip=0.1),
               dict(kind="barlow", prior=[0.5] * 8), dict(kind="barlow", margin=2.0), dict(kind="barlow", class_weight=[[1, 1, 1]]),
               dict(kind="barlow", parent=[-1] * 8), dict(kind="barlow", mode="conditional"), dict(kind="bce", lambd=0.1),
               dict(kind="ntxent", lambd=0.1), dict(kind="focal", lambd=0.1), dict(kind="twins")):
        with pytest.raises(ValueError):
            state.set(cpu, 8, **kw)
        assert state.kind == "bce" and state.lambd is None and state.temperature is None and state._held == {}, kw
    with pytest.raises(ValueError, match="at most 1024"):
        state.set(cpu, 2048, kind="barlow")
    with pytest.raises(RuntimeError, match="model.to"):                            # the state lives on the parameters' device
        state.set(cpu, 8, kind="barlow")
    assert state.kind == "bce" and state.lambd is None
    with pytest.raises(ValueError, match="lambd"):
        state.load_state({"kind": "barlow"}, cpu, 8)
    assert L.check_lambda("x", 0) == 0.0 and L.check_lambda("x", "0.5") == 0.5


def test_loss_module_and_monitor_refuse_what_they_cannot_take():
    for bad in (-0.1, float("nan"), float("inf"), None, "x"):
        with pytest.raises(ValueError):
            L.BarlowTwinsLoss(bad)
    crit = L.BarlowTwinsLoss()
    assert crit.kind == "barlow" and crit.lambd.tolist() == pytest.approx([0.0051]) and list(crit.state_dict()) == []
    with pytest.raises(RuntimeError, match="GPU only"):
        crit(torch.zeros(4, 8), torch.zeros(4, 1))
    with pytest.raises(RuntimeError, match="GPU only"):
        L.barlow_terms(torch.zeros(4, 8), torch.zeros(4))
    assert L.KERNEL["barlow"] == "cx_barlow_fwd_bwd"


def test_entry_point_validates_before_any_launch():
    """cx_barlow_fwd_bwd and cx_barlow_scratch check their arguments before anything is launched (no GPU needed)."""
    from chexpert_amd import _lib, ops
    EINVAL, ESHAPE = -1, -3
    lib = _lib.lib()
    f = [torch.zeros(4096, dtype=torch.float32) for _ in range(4)]
    E, G, T, S = (t.data_ptr() for t in f)
    need = lib.cx_barlow_scratch(8, 16)
    call = lambda e=E, g=G, t=T, s=S, floats=4096, N=8, d=16: lib.cx_barlow_fwd_bwd(e, g, t, None, None, None, 1.0, s, floats, N, d, None)   # noqa: E731
    assert call(e=None) == EINVAL and call(g=None) == EINVAL and call(t=None) == EINVAL and call(s=None) == EINVAL
    assert call(N=1) == EINVAL and call(N=0) == EINVAL and call(N=-3) == EINVAL and call(d=0) == EINVAL and call(d=-1) == EINVAL
    assert 0 < need <= 4096 and call(floats=need - 1) == EINVAL and call(floats=0) == EINVAL
    assert call(N=_lib.BARLOW_MAX_N + 1, floats=1 << 40) == ESHAPE and call(d=_lib.BARLOW_MAX_D + 1, floats=1 << 40) == ESHAPE
    assert (_lib.BARLOW_MAX_N, _lib.BARLOW_MAX_D) == (4096, 1024)
    # the layout of the header: a^ | b^ | G | four d-vectors | m | the tiles' terms | their row sums | their column sums
    r4 = lambda v: (v + 3) // 4 * 4                                                                                                          # noqa: E731
    for N, d in ((8, 16), (13, 7), (66, 33), (130, 136), (4096, 1024)):
        h, nt = N // 2, (d + 63) // 64
        assert lib.cx_barlow_scratch(N, d) == 2 * r4(h * d) + r4(d * d) + 4 * r4(d) + 4 + 4 * nt * nt + 2 * nt * r4(d) == ops.barlow_scratch(N, d)
    assert lib.cx_barlow_scratch(1, 16) == 0 and lib.cx_barlow_scratch(8, 0) == 0 and lib.cx_barlow_scratch(_lib.BARLOW_MAX_N + 1, 4) == 0
    assert lib.cx_barlow_scratch(4, _lib.BARLOW_MAX_D + 1) == 0
    for N, d in ((1, 4), (4, 0), (_lib.BARLOW_MAX_N + 1, 4), (4, _lib.BARLOW_MAX_D + 1)):
        with pytest.raises(ValueError):
            ops.barlow_scratch(N, d)
    # the wrapper: host tensors are refused before the library is called
    e, g, t = torch.zeros(4, 8), torch.zeros(4, 1), torch.ones(1)
    with pytest.raises(RuntimeError, match="GPU only"):
        ops.barlow_fwd_bwd(e, g, t, None, None)
    with pytest.raises(AssertionError):
        ops.barlow_fwd_bwd(e, g.reshape(-1), t, None, None)
    with pytest.raises(AssertionError):
        ops.barlow_fwd_bwd(e, g, t, None, None, scratch=torch.zeros(10))
    with pytest.raises(AssertionError):
        ops.barlow_fwd_bwd(e, g, t, None, None, stats=torch.zeros(3))


# ------------------------------------------------------------------------------------------------ the command line
_PRE = ["--train", "--synthetic", "16", "--batch_size", "4", "--resize", "64", "--pretrain", "barlow"]


def test_cli_flag_checks(tmp_path):
    from chexpert_amd import cli
    run = cli.check_flags(_PRE + ["--jitter"])
    assert run.pretrain == {"kind": "barlow", "proj_dim": 512, "lambd": None, "positive": "view"} and cli.head_width(run.args) == 512
    assert cli.pretrain_kind(run.pretrain) == "barlow" and cli.pretrain_kind(None) is None
    assert cli.lambda_of(run.pretrain) == 0.0051 and cli.lambda_of(run.pretrain, {"lambd": 0.02}) == 0.02
    run = cli.check_flags(_PRE + ["--affine", "--proj_dim", "32", "--barlow_lambda", "0.01", "--fused_optimizer", "--graph", "--optimizer", "lars",
                                  "--ema_decay", "0.99", "--sam_rho", "0.05", "--pool", "gem", "--model", "resnet152", "--positive", "view"])
    assert run.pretrain == {"kind": "barlow", "proj_dim": 32, "lambd": 0.01, "positive": "view"} and cli.head_width(run.args) == 32
    assert cli.lambda_of(run.pretrain, {"lambd": 0.02}) == 0.01
    # the contrastive run keeps its options and its default width
    con = cli.check_flags(["--train", "--synthetic", "16", "--batch_size", "4", "--pretrain", "contrastive", "--jitter"])
    assert con.pretrain == {"proj_dim": 128, "temperature": None, "positive": "view"} and cli.head_width(con.args) == 128
    assert cli.pretrain_kind(con.pretrain) == "contrastive"
    refused = [([], "--affine or --jitter"), (["--jitter", "--temperature", "0.2"], "--temperature"),
               (["--jitter", "--positive", "study"], "--positive study"), (["--jitter", "--positive", "patient"], "--positive patient"),
               (["--jitter", "--barlow_lambda", "-1"], "lambd"), (["--jitter", "--barlow_lambda", "nan"], "lambd"),
               (["--jitter", "--mixup", "0.4"], "--mixup"), (["--jitter", "--loss", "focal"], "--loss focal"),
               (["--jitter", "--uncertain", "multiclass"], "--uncertain multiclass"), (["--jitter", "--head", "csra"], "--head csra"),
               (["--jitter", "--pos_weight", "auto"], "--pos_weight"), (["--jitter", "--evaluate_single_model"], "--evaluate_single_model"),
               (["--jitter", "--proj_dim", "0"], "--proj_dim"), (["--jitter", "--proj_dim", "2048"], "--proj_dim")]
    for extra, why in refused:
        with pytest.raises(ValueError) as err:
            cli.check_flags(_PRE + extra)
        assert why in str(err.value) and "\n" not in str(err.value), (extra, str(err.value))
    with pytest.raises(ValueError, match="--pretrain barlow sees 2 x --batch_size"):
        cli.check_flags(["--train", "--synthetic", "16", "--batch_size", "4096", "--pretrain", "barlow", "--jitter"])
    with pytest.raises(ValueError, match="--pretrain barlow is a training mode"):
        cli.check_flags(["--synthetic", "16", "--pretrain", "barlow", "--jitter"])
    with pytest.raises(ValueError, match="belongs to --pretrain barlow"):
        cli.check_flags(["--train", "--synthetic", "16", "--barlow_lambda", "0.01"])
    with pytest.raises(ValueError, match="--barlow_lambda"):
        cli.check_flags(["--train", "--synthetic", "16", "--pretrain", "contrastive", "--jitter", "--barlow_lambda", "0.01"])


def test_more_than_one_rank_is_refused(monkeypatch):
    from chexpert_amd import cli
    monkeypatch.setattr(cli.P, "dist_info", lambda: (0, 2, 0))
    with pytest.raises(ValueError, match="--pretrain barlow cannot be combined with more than one rank"):
        cli.check_flags(_PRE + ["--jitter"])
    from chexpert_amd.models import _fused
    with pytest.raises(RuntimeError, match="kind='barlow'.*world size 2"):
        _fused.check_single_process(type("R", (), {"world": 2})(), _fused.BARLOW_DATA_PARALLEL)
    _fused.check_single_process(None, _fused.BARLOW_DATA_PARALLEL)
    assert _fused.BARLOW_DATA_PARALLEL != _fused.NTXENT_DATA_PARALLEL


def test_restore_is_refused_across_the_kinds_of_run():
    from chexpert_amd import cli
    bar = {"kind": "barlow", "proj_dim": 16, "lambd": None, "positive": "view"}
    con = {"proj_dim": 16, "temperature": None, "positive": "view"}
    sd = {"classifier.weight": torch.zeros(16, 8), "classifier.bias": torch.zeros(16)}
    sup = {"state_dict": {"classifier.weight": torch.zeros(5, 8)}}
    ck_bar, ck_con = {"pretrain": "barlow", "state_dict": sd}, {"pretrain": "contrastive", "state_dict": sd}
    key = "classifier.weight"
    cli.check_checkpoint_pretrain(ck_bar, bar, "a.pt", key)
    cli.check_checkpoint_pretrain(ck_con, con, "a.pt", key)
    with pytest.raises(ValueError, match="--pretrain barlow.*--init_backbone"):
        cli.check_checkpoint_pretrain(ck_bar, None, "a.pt", key)
    with pytest.raises(ValueError, match="supervised one; --pretrain barlow continues"):
        cli.check_checkpoint_pretrain(sup, bar, "a.pt", key)
    with pytest.raises(ValueError, match="one of --pretrain barlow, this run is --pretrain contrastive"):
        cli.check_checkpoint_pretrain(ck_bar, con, "a.pt", key)
    with pytest.raises(ValueError, match="one of --pretrain contrastive, this run is --pretrain barlow"):
        cli.check_checkpoint_pretrain(ck_con, bar, "a.pt", key)
    with pytest.raises(ValueError, match="16 outputs, --proj_dim asks for 32"):
        cli.check_checkpoint_pretrain(ck_bar, dict(bar, proj_dim=32), "a.pt", key)
