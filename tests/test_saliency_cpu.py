"""CPU (no GPU): the numpy statements of the pixel-attribution kernels (chexpert_amd.saliency: normal_reference, path_alphas, the
integrated-gradients and SmoothGrad compositions around toy torch callables whose attributions can be written down by hand), the
argument checks of the three entry points of chexpert_amd/csrc/saliency.hip, and the command-line flag checks."""
import math
import os
import re

import numpy as np
import pytest
import torch

from chexpert_amd import saliency as S


# ------------------------------------------------------------------------------------------------ the noise
def test_normal_reference_is_a_function_of_seed_and_index():
    from chexpert_amd import metrics as M
    a, b = S.normal_reference(7, 5, 48), S.normal_reference(7, 5, 48)
    assert a.dtype == np.float32 and a.shape == (5, 48) and np.array_equal(a.view(np.uint32), b.view(np.uint32))
    assert not np.array_equal(a, S.normal_reference(8, 5, 48))
    two = np.concatenate([S.normal_reference(7, 2, 48), S.normal_reference(7, 3, 48, first_row=2)])      # rows cut into two calls
    assert np.array_equal(a.view(np.uint32), two.view(np.uint32))
    assert np.array_equal(S.normal_reference(7, 1, 48, first_row=3)[0], a[3])
    # the hash is metrics.splitmix64, the two uniforms and the Box-Muller cosine branch as the header states them
    for r, e in ((0, 0), (1, 5), (4, 47)):
        z = M.splitmix64(7, r * 48 + e)
        u1, u2 = ((z >> 40) + 1) / 2.0 ** 24, ((z >> 8) & 0xFFFFFF) / 2.0 ** 24
        assert a[r, e] == np.float32(math.sqrt(-2.0 * math.log(u1)) * math.cos(2.0 * math.pi * u2))


def test_normal_reference_moments_and_range():
    N = 1 << 16
    for seed in (0, 123456789):
        n = S.normal_reference(seed, 4, N // 4).astype(np.float64).ravel()
        assert np.isfinite(n).all() and np.abs(n).max() <= 5.8            # u1 >= 2^-24: |n| <= sqrt(48 ln 2) = 5.77
        assert abs(n.mean()) <= 4 / math.sqrt(N)
        assert abs(n.var() - 1) <= 4 * math.sqrt(2 / N)


# ------------------------------------------------------------------------------------------------ the path
def test_path_alphas():
    for m in list(range(1, 66)) + [98, 100, 103, 196, 256]:
        for rule in S.RULES:
            a, w = S.path_alphas(m, rule)
            assert a.dtype == np.float64 and w.dtype == np.float64 and math.fsum(w) == 1.0 and (w > 0).all()
            if rule == "midpoint":
                assert len(a) == m and np.array_equal(a, (np.arange(m) + 0.5) / m)
                np.testing.assert_allclose(w, np.full(m, 1.0 / m), rtol=1e-13, atol=0)
            else:
                assert len(a) == m + 1 and np.array_equal(a, np.arange(m + 1) / m) and a[0] == 0.0 and a[-1] == 1.0
                want = np.full(m + 1, 1.0 / m)
                want[0] = want[-1] = 0.5 / m
                np.testing.assert_allclose(w, want, rtol=1e-13, atol=0)
    assert S.path_alphas(4, "midpoint")[0].tolist() == [0.125, 0.375, 0.625, 0.875] and S.path_alphas(4)[1].tolist() == [0.25] * 4
    assert S.path_alphas(2, "trapezoid")[1].tolist() == [0.25, 0.5, 0.25]
    for bad in (0, -3, 2.5, True, None):
        with pytest.raises(ValueError):
            S.path_alphas(bad)
    with pytest.raises(ValueError):
        S.path_alphas(4, "simpson")


# ------------------------------------------------------------------------------------------------ toy callables
def _toy(B=2, H=3, W=5, n=4, seed=0):
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(B, 3, H, W, generator=g, dtype=torch.float64)
    Wl = torch.randn(n, 3 * H * W, generator=g, dtype=torch.float64)
    bias = torch.randn(n, generator=g, dtype=torch.float64)
    return x, Wl, bias


@pytest.mark.parametrize("baseline", [None, "black", 0.25, (0.5, -1.0, 2.0), "full"])
@pytest.mark.parametrize("rule", S.RULES)
def test_integrated_gradients_of_a_linear_function(baseline, rule):
    x, Wl, bias = _toy()
    f = lambda p: p.flatten(1) @ Wl.t() + bias
    if baseline == "full":
        baseline = torch.randn(x.shape, generator=torch.Generator().manual_seed(9), dtype=torch.float64)
    attr, logits, delta = S.integrated_gradients_reference(f, x, [0, 3], steps=3, rule=rule, baseline=baseline, channels="none")
    assert attr.shape == (2, 2, 3, 3, 5) and logits.shape == (2, 4) and delta.shape == (2, 2)
    assert np.abs(delta).max() <= 1e-6
    base = S._baseline(baseline, x)
    base = base.numpy() if isinstance(base, torch.Tensor) else np.asarray(base).reshape(1, 3, 1, 1)
    for k, c in enumerate((0, 3)):
        np.testing.assert_allclose(attr[:, k], Wl[c].numpy().reshape(1, 3, 3, 5) * (x.numpy() - base), rtol=1e-12, atol=1e-12)
    np.testing.assert_allclose(logits, f(x).numpy(), rtol=0, atol=1e-12)
    summed = S.integrated_gradients_reference(f, x, [0, 3], steps=3, rule=rule, baseline=baseline, channels="sum")[0]
    np.testing.assert_allclose(summed, attr.sum(2), rtol=1e-12, atol=1e-12)


def test_midpoint_rule_is_exact_for_a_quadratic():
    x, Wl, bias = _toy(seed=2)
    Q = torch.randn(4, 45, generator=torch.Generator().manual_seed(5), dtype=torch.float64)
    f = lambda p: (p.flatten(1) @ Wl.t()) ** 2 + (p.flatten(1) ** 2) @ Q.t() + bias       # the gradient is linear along the path
    for m in (1, 4):
        _, _, delta = S.integrated_gradients_reference(f, x, None, steps=m, rule="midpoint", baseline=(0.5, 0.0, -0.5))
        assert delta.shape == (2, 4) and np.abs(delta).max() <= 1e-5
    _, _, coarse = S.integrated_gradients_reference(f, x, None, steps=1, rule="trapezoid")          # the trapezoid is exact as well; a
    assert np.abs(coarse).max() <= 1e-5
    cubic = lambda p: (p.flatten(1) @ Wl.t()) ** 3                                                   # cubic is not: delta shows it
    assert np.abs(S.integrated_gradients_reference(cubic, x, None, steps=2)[2]).max() > 1e-3


def test_smoothgrad_without_noise_is_the_gradient():
    x, Wl, bias = _toy(seed=3)
    x = x.float()
    Wf = Wl.float()
    f = lambda p: torch.tanh(p.flatten(1) @ Wf.t())
    xr = x.clone().requires_grad_(True)
    g = torch.stack([torch.autograd.grad(f(xr)[:, c].sum(), xr)[0] for c in range(4)], 1).numpy()
    for samples in (1, 4):                                               # 4 x (1/4) g: exact in binary
        got = S.smoothgrad_reference(f, x, None, samples=samples, sigma=0.0, channels="none")
        assert got.shape == g.shape and np.array_equal(got, g)
    assert np.array_equal(S.smoothgrad_reference(f, x, [1], samples=1, sigma=0.0, channels="abs")[:, 0], np.abs(g[:, 1]).sum(1))
    assert np.array_equal(S.smoothgrad_reference(f, x, [1], samples=1, sigma=0.0, squared=True, channels="max")[:, 0], (g[:, 1] ** 2).max(1))
    noisy = S.smoothgrad_reference(f, x, [1], samples=3, sigma=0.5, seed=4, channels="none")
    assert not np.array_equal(noisy[:, 0], g[:, 1]) and np.array_equal(noisy, S.smoothgrad_reference(f, x, [1], samples=3, sigma=0.5, seed=4, channels="none"))


def test_kernel_statements_on_a_hand_example():
    x = np.arange(2 * 3 * 1 * 2, dtype=np.float32).reshape(2, 3, 1, 2)
    pts = S.points_reference(x, (1.0, 2.0, 3.0), [1, 0], [0.5, 0.0])
    assert np.array_equal(pts[0].ravel(), [1 + 0.5 * 5, 1 + 0.5 * 6, 2 + 0.5 * 6, 2 + 0.5 * 7, 3 + 0.5 * 7, 3 + 0.5 * 8])
    assert np.array_equal(pts[1].ravel(), [1, 1, 2, 2, 3, 3])
    assert np.array_equal(S.points_reference(x, (0.0, 0.0, 0.0), [0, 1], [1.0, 1.0]), x)
    acc = S.accumulate_reference(x, [1, 1], [2.0, 3.0], 2)
    assert not acc[0].any() and np.array_equal(acc[1], 2 * x[0] + 3 * x[1])
    assert np.array_equal(S.accumulate_reference(x, [0, 5], [1.0, 1.0], 1, square=True, acc=np.ones((1, 3, 1, 2), np.float32))[0], 1 + x[0] ** 2)
    m, tot = S.finish_reference(acc, x, (0.0, 0.0, 0.0), [0, 1], times_input=True, channels="sum")
    assert m.shape == (2, 1, 2) and np.array_equal(m[1], (acc[1] * x[1]).sum(0)) and tot[1] == float((acc[1] * x[1]).sum())
    assert np.array_equal(S.finish_reference(-acc, channels="max")[0][1], acc[1].max(0))


# ------------------------------------------------------------------------------------------------ the C ABI
def test_entry_points_validate_without_launching():
    """cx_sal_points / cx_sal_accumulate / cx_sal_finish check their arguments before any launch (no GPU needed)."""
    from chexpert_amd import _lib
    EINVAL, EALIGN, ESHAPE = -1, -2, -3
    L = _lib.lib()
    pts, accf, fin = L.cx_sal_points, L.cx_sal_accumulate, L.cx_sal_finish
    f = [torch.zeros(4096, dtype=torch.float32) for _ in range(4)]
    i32 = torch.zeros(64, dtype=torch.int32)
    d = torch.zeros(1024, dtype=torch.float64)
    X, Bs, O, G = (t.data_ptr() for t in f)
    I, D = i32.data_ptr(), d.data_ptr()
    assert all(p % 8 == 0 for p in (X, Bs, O, G, I, D))
    p = lambda x=X, base=Bs, img=I, al=G, sg=None, out=O, B=2, R=3, H=4, W=5: pts(x, base, 0.0, 0.0, 0.0, img, al, sg, 1, 0, out, B, R, H, W, None)
    assert p(x=None) == EINVAL and p(img=None) == EINVAL and p(al=None) == EINVAL and p(out=None) == EINVAL
    assert p(B=0) == EINVAL and p(R=0) == EINVAL and p(R=-1) == EINVAL and p(H=0) == EINVAL and p(W=-2) == EINVAL
    assert p(out=X) == EINVAL and p(out=Bs) == EINVAL                   # the output aliases an input
    assert p(R=70000) == ESHAPE and p(H=1 << 15, W=1 << 15) == ESHAPE
    assert p(x=X + 2) == EALIGN and p(out=O + 1) == EALIGN and p(img=I + 2) == EALIGN and p(sg=G + 6) == EALIGN and p(base=Bs + 3) == EALIGN
    a = lambda g=G, slot=I, w=X, acc=O, R=3, P=2, H=4, W=5: accf(g, slot, w, acc, R, P, H, W, 0, 1, None)
    assert a(g=None) == EINVAL and a(slot=None) == EINVAL and a(w=None) == EINVAL and a(acc=None) == EINVAL
    assert a(R=0) == EINVAL and a(P=0) == EINVAL and a(H=0) == EINVAL and a(W=0) == EINVAL and a(acc=G) == EINVAL
    assert a(P=65536) == ESHAPE and a(H=1 << 15, W=1 << 15) == ESHAPE
    assert a(g=G + 1) == EALIGN and a(acc=O + 2) == EALIGN and a(slot=I + 1) == EALIGN and a(w=X + 3) == EALIGN
    q = lambda acc=G, x=X, base=Bs, img_of=I, out=O, tot=None, part=None, P=2, B=2, H=4, W=5, ti=1, mode=1: \
        fin(acc, x, base, 0.0, 0.0, 0.0, img_of, out, tot, part, P, B, H, W, ti, mode, None)
    assert q(acc=None) == EINVAL and q(out=None) == EINVAL and q(x=None) == EINVAL and q(img_of=None) == EINVAL
    assert q(P=0) == EINVAL and q(B=0) == EINVAL and q(H=0) == EINVAL and q(W=0) == EINVAL
    assert q(out=G) == EINVAL and q(out=X) == EINVAL and q(out=Bs) == EINVAL and q(tot=D) == EINVAL      # total without partial
    assert q(mode=4) == ESHAPE and q(mode=-1) == ESHAPE and q(P=70000) == ESHAPE
    assert q(acc=G + 2) == EALIGN and q(out=O + 1) == EALIGN and q(tot=D + 4, part=D + 64) == EALIGN and q(tot=D, part=D + 4) == EALIGN
    # declared in the header with the parameters the binding passes, and built from their own source file
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(root, "include", "chexpert_hip.h")).read(), flags=re.S)
    for name, n in (("cx_sal_points", 16), ("cx_sal_accumulate", 11), ("cx_sal_finish", 17)):
        m = re.search(r"\bint\s+%s\s*\(([^;{]*?)\)\s*;" % name, hdr, flags=re.S)
        assert m and len(_lib.SIGNATURES[name]) == m.group(1).count(",") + 1 == n
    assert "saliency.hip" in open(os.path.join(root, "chexpert_amd", "csrc", "Makefile")).read()
    assert L.cx_abi_version() == 10                                     # additive entry points


# ------------------------------------------------------------------------------------------------ arguments and the command line
def test_public_functions_refuse_bad_arguments_before_anything_runs():
    from chexpert_amd.models import DenseNet
    model = DenseNet(32, (2, 2, 2, 2), 64, num_classes=5)               # on the CPU: nothing below may reach a kernel
    x = torch.zeros(2, 3, 64, 64)
    for bad in ([], [5], [-1], [0.5], "top", torch.zeros(3, dtype=torch.int64), torch.tensor([0, 7])):
        for fn in (S.input_gradient, S.smoothgrad, S.integrated_gradients):
            with pytest.raises(ValueError):
                fn(model, x, bad)
    for kw in (dict(steps=0), dict(steps=2.5), dict(rule="simpson"), dict(baseline="white"), dict(baseline=(1.0, 2.0)),
               dict(baseline=torch.zeros(2, 3, 32, 32)), dict(channels="mean"), dict(chunk=0)):
        with pytest.raises(ValueError):
            S.integrated_gradients(model, x, [0], **kw)
    for kw in (dict(samples=0), dict(sigma=-1.0), dict(sigma=torch.zeros(3)), dict(noise_level=-0.1), dict(channels="l2"), dict(chunk=-4)):
        with pytest.raises(ValueError):
            S.smoothgrad(model, x, [0], **kw)
    with pytest.raises(ValueError):
        S.input_gradient(model, torch.zeros(2, 1, 64, 64), [0])
    for fn in (S.input_gradient, S.smoothgrad, S.integrated_gradients):
        with pytest.raises(RuntimeError, match="GPU only"):
            fn(model, x, [0])
    assert model.training


def test_cli_flag_checks():
    from chexpert_amd import cli
    p = cli.build_parser()
    assert cli.resolve_saliency(p.parse_args(["--visualize"])) is None
    sal = cli.resolve_saliency(p.parse_args(["--visualize", "--saliency", "ig"]))
    assert sal == {"method": "ig", "classes": [0, 1, 2, 3, 4], "steps": 32, "sigma": None, "baseline": "mean", "chunk": None}
    sal = cli.resolve_saliency(p.parse_args(["--visualize", "--saliency", "smoothgrad_sq", "--saliency_classes", "0", "2", "--saliency_sigma", "1.5",
                                             "--saliency_chunk", "8"]))
    assert sal == {"method": "smoothgrad_sq", "classes": [0, 2], "steps": 16, "sigma": 1.5, "baseline": "mean", "chunk": 8}
    assert cli.resolve_saliency(p.parse_args(["--visualize", "--saliency", "ig", "--saliency_classes", "all", "--n_classes", "14",
                                              "--saliency_steps", "7", "--saliency_baseline", "black"]))["classes"] == list(range(14))
    for bad in (["--saliency", "ig"], ["--saliency_steps", "4", "--visualize"], ["--saliency_classes", "0"],
                ["--visualize", "--saliency", "ig", "--saliency_classes", "5"], ["--visualize", "--saliency", "ig", "--saliency_classes", "-1"],
                ["--visualize", "--saliency", "ig", "--saliency_classes", "x"], ["--visualize", "--saliency", "ig", "--saliency_steps", "0"],
                ["--visualize", "--saliency", "smoothgrad", "--saliency_steps", "-2"], ["--visualize", "--saliency", "smoothgrad", "--saliency_sigma", "-1"],
                ["--visualize", "--saliency", "ig", "--saliency_sigma", "1"], ["--visualize", "--saliency", "grad", "--saliency_baseline", "black"],
                ["--visualize", "--saliency", "ig", "--saliency_chunk", "0"]):
        with pytest.raises(ValueError):
            cli.resolve_saliency(p.parse_args(bad))
    with pytest.raises(SystemExit):
        p.parse_args(["--visualize", "--saliency", "lime"])
    with pytest.raises(ValueError, match="--visualize"):               # refused in main's flag checks, before anything is built
        cli.main(["--saliency", "ig", "--synthetic", "4", "--output_dir", "unused"])
    with pytest.raises(ValueError, match="--saliency_steps"):
        cli.main(["--visualize", "--saliency", "ig", "--saliency_steps", "0", "--synthetic", "4", "--output_dir", "unused"])


def test_visualize_saliency_writes_one_figure_per_image(tmp_path):
    from chexpert_amd import vis
    rng = np.random.RandomState(0)
    N, K = 3, 2
    args = (rng.rand(N, 64, 64), (rng.rand(N, 5) < 0.3).astype(np.float32), rng.randn(N, 5))
    idents, names = ["synthetic/%d" % i for i in (4, 7, 9)], ["a", "b", "c", "d", "e"]
    files = vis.visualize_saliency(*args, rng.randn(N, K, 64, 64), idents, names, [3, 0], "ig", str(tmp_path), 12, signed=True)
    files += vis.visualize_saliency(*args, np.zeros((N, K, 64, 64)), idents, names, [3, 0], "grad", str(tmp_path), 12)      # an all-zero map draws
    got = sorted(os.listdir(os.path.join(str(tmp_path), "vis")))
    assert got == sorted("saliency_%s_synthetic_%d_step_12.png" % (m, i) for m in ("ig", "grad") for i in (4, 7, 9))
    assert sorted(os.path.basename(f) for f in files) == got
