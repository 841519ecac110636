"""CPU (no GPU): the host side of sample mixing (chexpert_amd/augment.py: mix_plan, erase_plan, mix_reference, target_mix_reference)
and its command-line flags.  The references are the definitions cx_u8_mix / cx_target_mix (chexpert_amd/csrc/mix.hip) are held to in
tests/test_mix_gpu.py; here they are pinned to independent statements of the same arithmetic."""
import os
import re

import numpy as np
import pytest
import torch

from chexpert_amd import augment, synth

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ONE = 65536


def _noise(seed, B, H, W):
    s = max(H, W)
    n = -(-B * H * W // (s * s))
    return synth.xray_u8(seed, n, s).flatten()[:B * H * W].reshape(B, 1, H, W).contiguous()


def _i32(v):
    return np.asarray(v, dtype=np.int32)


def _full(B, H, W):
    return _i32([[0, H, 0, W]] * B)


def test_reference_against_the_float64_statement():
    """floor(lambda a + (1 - lambda) o + 0.5) in float64 with lambda = q / 65536: products of an integer < 2^8 and a multiple of
    2^-16 <= 1, their sum and the half are all exact in float64, so the two statements agree bit for bit."""
    B, H, W = 5, 12, 20
    x = _noise(3, B, H, W)
    perm = _i32([3, 0, 4, 1, 2])
    lam_q = _i32([0, 1, 32768, 65535, 21845])
    box = _i32([[0, H, 0, W], [2, 9, 3, 9], [0, 5, 0, W], [11, 12, 19, 20], [0, H, 16, 20]])
    got = augment.mix_reference(x, perm, lam_q, box)
    assert got.shape == x.shape and got.dtype == torch.uint8
    a = x[:, 0].numpy().astype(np.float64)
    want = a.copy()
    for b in range(B):
        lam = float(lam_q[b]) / 65536.0
        y0, y1, x0, x1 = box[b]
        o = a[perm[b]]
        want[b, y0:y1, x0:x1] = np.floor(lam * a[b, y0:y1, x0:x1] + (1.0 - lam) * o[y0:y1, x0:x1] + 0.5)
    assert np.array_equal(got[:, 0].numpy(), want.astype(np.uint8))
    assert (got != x).any()
    assert torch.equal(augment.mix_reference(x[:, 0], perm, lam_q, box), got[:, 0])      # (B,H,W) form


def test_reference_identity_partner_and_fill():
    B, H, W = 4, 10, 16
    x = _noise(4, B, H, W)
    perm = _i32([1, 2, 3, 0])
    # lambda = 1, or an empty box, leaves a row unchanged
    assert torch.equal(augment.mix_reference(x, perm, _i32([ONE] * B), _full(B, H, W)), x)
    for empty in ([0, 0, 0, 0], [5, 5, 0, W], [0, H, 7, 7], [6, 2, 0, W], [0, H, 9, 3]):
        assert torch.equal(augment.mix_reference(x, perm, _i32([0] * B), _i32([empty] * B)), x)
    # a full box at q = 0 is the partner row; a fixed point of perm is unchanged at any q
    assert torch.equal(augment.mix_reference(x, perm, _i32([0] * B), _full(B, H, W)), x[torch.from_numpy(perm).long()])
    assert torch.equal(augment.mix_reference(x, _i32([0, 1, 2, 3]), _i32([0, 1, 32768, 65535]), _full(B, H, W)), x)
    # perm = -1 writes `fill` inside the box and nothing else
    for fill in (0, 136):
        got = augment.mix_reference(x, _i32([-1] * B), _i32([0] * B), _i32([[2, 7, 3, 9]] * B), fill)
        want = x.clone()
        want[:, :, 2:7, 3:9] = fill
        assert torch.equal(got, want)


def test_reference_clamps_out_of_range_parameters():
    B, H, W = 4, 10, 16
    x = _noise(5, B, H, W)
    wild = augment.mix_reference(x, _i32([B + 7, -9, 2, 1]), _i32([70000, -5, 100, 0]), _i32([[-3, H + 9, -1, W + 50], [-4, 4, -4, 4], [8, 99, 12, 99], [0, H, 0, W]]), 7)
    tame = augment.mix_reference(x, _i32([B - 1, -1, 2, 1]), _i32([ONE, 0, 100, 0]), _i32([[0, H, 0, W], [0, 4, 0, 4], [8, H, 12, W], [0, H, 0, W]]), 7)
    assert torch.equal(wild, tame)
    assert torch.equal(wild[0], x[0]) and (wild[1, 0, :4, :4] == 7).all() and torch.equal(wild[3], x[1])
    t = torch.tensor([[0.0, 1.0], [1.0, 0.0], [0.5, 0.25], [1.0, 1.0]])
    assert torch.equal(augment.target_mix_reference(t, _i32([B + 7, -9, 2, 1]), _i32([70000, 5, -100, 32768])),
                       augment.target_mix_reference(t, _i32([B - 1, -1, 2, 1]), _i32([ONE, 5, 0, 32768])))


def test_target_reference_rules():
    t = torch.tensor([[1.0, 0.0, -1.0, 0.7, 0.3],
                      [0.0, 1.0, 1.0, -1.0, 0.55],
                      [1.0, 1.0, 0.0, 0.0, -1.0],
                      [0.25, 0.0, 1.0, 1.0, 0.85]])
    perm, tw_q = _i32([1, 0, -1, 2]), _i32([16384, 49152, 100, ONE])
    got = augment.target_mix_reference(t, perm, tw_q)
    assert got.dtype == torch.float32 and got.shape == t.shape
    assert torch.equal(got[2], t[2]) and torch.equal(got[3], t[3])          # p < 0 / w_q = 65536: copied, the -1 included
    f = np.float32
    w0, w1 = f(0.25), f(0.75)
    want0 = [f(w0 * f(1.0)) + f(f(1 - w0) * f(0.0)), f(w0 * f(0.0)) + f(f(1 - w0) * f(1.0)), f(-1.0), f(-1.0),
             f(f(w0 * f(0.3)) + f(f(1 - w0) * f(0.55)))]
    want1 = [f(w1 * f(0.0)) + f(f(1 - w1) * f(1.0)), f(w1 * f(1.0)) + f(f(1 - w1) * f(0.0)), f(-1.0), f(-1.0),
             f(f(w1 * f(0.55)) + f(f(1 - w1) * f(0.3)))]
    assert got[0].tolist() == [float(v) for v in want0]                     # -1 on either side gives -1; soft labels are blended
    assert got[1].tolist() == [float(v) for v in want1]
    assert got[0, 0].item() == 0.25 and got[0, 1].item() == 0.75
    # w = 0 takes the partner's labels (and its ignored ones)
    assert torch.equal(augment.target_mix_reference(t[:2, :2], _i32([1, 0]), _i32([0, 0])), t[[1, 0]][:, :2])


def _check_plan(p, B, H, W):
    assert set(p) == {"perm", "lam_q", "box", "tw_q"}
    assert p["perm"].shape == (B,) and p["lam_q"].shape == (B,) and p["tw_q"].shape == (B,) and p["box"].shape == (B, 4)
    assert all(v.dtype == np.int32 for v in p.values())
    assert ((p["lam_q"] >= 0) & (p["lam_q"] <= ONE)).all() and ((p["tw_q"] >= 0) & (p["tw_q"] <= ONE)).all()
    y0, y1, x0, x1 = p["box"].T
    assert ((0 <= y0) & (y0 <= y1) & (y1 <= H) & (0 <= x0) & (x0 <= x1) & (x1 <= W)).all()


def _is_identity(p, B):
    return (p["perm"] == np.arange(B)).all() and (p["lam_q"] == ONE).all() and (p["tw_q"] == ONE).all() and \
        ((p["box"][:, 1] <= p["box"][:, 0]) | (p["box"][:, 3] <= p["box"][:, 2])).all()


@pytest.mark.parametrize("mode", ["batch", "elem"])
@pytest.mark.parametrize("ma,ca", [(0.4, 0.0), (0.0, 1.0), (0.4, 1.0)])
def test_mix_plan_properties(mode, ma, ca):
    B, H, W = 16, 48, 64
    seen_cut = seen_mix = False
    for seed in range(20, 28):
        p = augment.mix_plan(seed, B, H, W, ma, ca, mode=mode)
        _check_plan(p, B, H, W)
        q = augment.mix_plan(seed, B, H, W, ma, ca, mode=mode)
        assert all(np.array_equal(p[k], q[k]) for k in p)                   # a pure function of the seed
        assert sorted(p["perm"].tolist()) == list(range(B))
        assert np.array_equal(p["perm"], np.argsort(synth.uniform(seed, (B,)).numpy(), kind="stable"))
        if mode == "batch":
            assert len(set(p["lam_q"].tolist())) == 1 and len(set(p["tw_q"].tolist())) == 1 and len({tuple(r) for r in p["box"].tolist()}) == 1
        full = (p["box"] == np.array([0, H, 0, W])).all(1)
        area = (p["box"][:, 1] - p["box"][:, 0]).astype(np.int64) * (p["box"][:, 3] - p["box"][:, 2])
        share = ((H * W - area) * 131072 + H * W) // (2 * H * W)
        mixup = full & (p["tw_q"] == p["lam_q"])                            # a full-image Mixup row (lambda may round to q = 0) ...
        cut = (p["lam_q"] == 0) & (p["tw_q"] == share)                      # ... or a CutMix row (a cut of the whole image is both)
        assert (mixup | cut).all()
        if ca == 0:
            assert mixup.all()
        if ma == 0:
            assert cut.all()
        seen_cut, seen_mix = seen_cut or bool((cut & ~mixup).any()), seen_mix or bool((mixup & ~cut).any())
    assert seen_mix == (ma > 0) and seen_cut == (ca > 0)                    # with both alphas, both kinds occur over 8 seeds
    if mode == "elem" and ca == 0:
        assert len(set(augment.mix_plan(20, B, H, W, ma, ca, mode="elem")["lam_q"].tolist())) > 1


def test_mix_plan_lambda_stream():
    """lambda comes from numpy's frozen legacy stream: RandomState(seed mod 2^32).beta."""
    seed, B = 2 ** 32 + 77, 8
    lam = np.random.RandomState(77).beta(0.4, 0.4, 1)[0]
    p = augment.mix_plan(seed, B, 32, 32, 0.4)
    assert (p["lam_q"] == int(np.floor(65536.0 * lam + 0.5))).all()
    lam = np.random.RandomState(77).beta(0.4, 0.4, B)
    assert np.array_equal(augment.mix_plan(seed, B, 32, 32, 0.4, mode="elem")["lam_q"], np.floor(65536.0 * lam + 0.5).astype(np.int32))


def test_cutmix_target_weight_is_the_counted_share():
    """Two constant images through mix_reference under a CutMix plan: tw_q / 65536 equals the counted share of unchanged pixels to
    2^-17 (it is that share rounded half up to 16 bits)."""
    B, H, W = 16, 48, 64
    x = torch.zeros(B, 1, H, W, dtype=torch.uint8)
    x[1::2] = 255
    for seed in (1, 2, 3):
        p = augment.mix_plan(seed, B, H, W, 0.0, 1.0, mode="elem")
        p["perm"] = (np.arange(B, dtype=np.int32) ^ 1)                      # the partner has the other colour
        y = augment.mix_reference(x, p["perm"], p["lam_q"], p["box"])
        share = (y == x).double().mean(dim=(1, 2, 3)).numpy()
        assert np.abs(p["tw_q"] / 65536.0 - share).max() <= 2.0 ** -17
        assert share.min() < 1.0


def test_identity_plans():
    B, H, W = 6, 32, 32
    assert _is_identity(augment.mix_plan(9, B, H, W), B)                                     # both alphas 0
    assert _is_identity(augment.mix_plan(9, B, H, W, 0.4, 1.0, prob=0.0), B)
    assert _is_identity(augment.mix_plan(9, B, H, W, 0.4, 1.0, prob=0.0, mode="elem"), B)
    e = augment.mix_plan(9, 0, H, W, 0.4)
    assert all(len(v) == 0 for v in e.values())
    # an un-applied draw keeps lam_q = tw_q = 65536: with prob = 0.5 in elem mode both kinds of row occur
    p = augment.mix_plan(9, 16, H, W, 0.4, 0.0, prob=0.5, mode="elem")
    off = p["lam_q"] == ONE
    assert off.any() and (~off).any() and (p["tw_q"][off] == ONE).all()
    x = _noise(6, 16, H, W)
    assert torch.equal(augment.mix_reference(x, p["perm"], p["lam_q"], p["box"])[torch.from_numpy(off)], x[torch.from_numpy(off)])
    for bad in ({"mixup_alpha": -1.0}, {"prob": 1.5}, {"switch_prob": -0.1}, {"mode": "row"}):
        with pytest.raises(ValueError):
            augment.mix_plan(1, 4, 8, 8, **bad)


def test_erase_plan():
    B, H, W = 64, 64, 96
    p = augment.erase_plan(11, B, H, W, prob=0.5)
    _check_plan(p, B, H, W)
    q = augment.erase_plan(11, B, H, W, prob=0.5)
    assert all(np.array_equal(p[k], q[k]) for k in p)
    assert (p["tw_q"] == ONE).all() and (p["lam_q"] == 0).all()             # labels do not change
    erased = p["perm"] < 0
    assert 16 <= erased.sum() <= 48                                         # Binomial(64, 0.5): +-4 sigma
    assert (p["perm"][erased] == -1).all() and (p["perm"][~erased] == np.arange(B)[~erased]).all()
    assert (p["box"][~erased] == 0).all()
    h = (p["box"][erased, 1] - p["box"][erased, 0]).astype(np.float64)
    w = (p["box"][erased, 3] - p["box"][erased, 2]).astype(np.float64)
    assert (h >= 1).all() and (w >= 1).all() and (h < H).all() and (w < W).all()
    # h and w are sqrt(A r) and sqrt(A / r) rounded to integers: each within 0.5 of a pair inside the ranges
    assert ((h + 0.5) * (w + 0.5) >= 0.02 * H * W).all() and ((h - 0.5) * (w - 0.5) <= H * W / 3.0).all()
    assert ((h + 0.5) / (w - 0.5) >= 0.3).all() and ((h - 0.5) / (w + 0.5) <= 3.3).all()
    assert len({tuple(r) for r in p["box"][erased].tolist()}) > 1
    # off, everywhere and nowhere
    assert (augment.erase_plan(11, B, H, W, prob=0.0)["perm"] == np.arange(B)).all()
    assert (augment.erase_plan(11, B, H, W, prob=1.0)["perm"] == -1).all()
    x = _noise(8, 4, 16, 16)
    e = augment.erase_plan(12, 4, 16, 16, prob=1.0)
    y = augment.mix_reference(x, e["perm"], e["lam_q"], e["box"], 136)
    for b in range(4):
        y0, y1, x0, x1 = e["box"][b]
        want = x[b].clone()
        want[:, y0:y1, x0:x1] = 136
        assert torch.equal(y[b], want)
    t = synth.targets(13, 4, 5)
    assert torch.equal(augment.target_mix_reference(t, e["perm"], e["tw_q"]), t)


def test_seeds_of_one_step_differ():
    seeds = [f(s, r) for s in (1, 2, 500) for r in (0, 1, 7) for f in (augment.step_seed, augment.mix_seed, augment.erase_seed)]
    seeds += [s * 7919 + 13 + r for s in (1, 2, 500) for r in (0, 1, 7)]            # the jitter's (cli.py)
    assert len(set(seeds)) == len(seeds)
    p, e = augment.mix_plan(augment.mix_seed(3), 8, 16, 16, 0.4), augment.mix_plan(augment.erase_seed(3), 8, 16, 16, 0.4)
    assert not np.array_equal(p["lam_q"], e["lam_q"])


def test_factory_returns_none_when_everything_is_off():
    assert augment.make_sample_mix() is None
    assert augment.make_sample_mix(0.4, 1.0, prob=0.0) is None
    sm = augment.make_sample_mix(0.4)
    assert isinstance(sm, augment.SampleMix) and sm.mixing and sm.erase_prob == 0 and sm.erase_fill == 136
    sm = augment.make_sample_mix(erase_prob=0.25)
    assert sm is not None and not sm.mixing
    with pytest.raises(ValueError):
        augment.make_sample_mix(-0.1)
    with pytest.raises(ValueError):
        augment.make_sample_mix(erase_prob=0.5, erase_fill=300)


def test_parser_defaults_and_argument_errors(capsys):
    from chexpert_amd import cli
    a = cli.parse_args(["--train"])
    assert (a.mixup, a.cutmix, a.mix_prob, a.mix_switch_prob, a.mix_mode, a.erase_prob, a.erase_fill) == (0.0, 0.0, 1.0, 0.5, "batch", 0.0, 136)
    assert cli.make_mix(a, 0, None) is None                                 # the defaults parse to "off"
    a = cli.parse_args(["--train", "--mixup", "0.4", "--cutmix", "1.0", "--mix_mode", "elem", "--erase_prob", "0.25", "--erase_fill", "0"])
    sm = cli.make_mix(a, 2, None)
    assert sm.mix == {"mixup_alpha": 0.4, "cutmix_alpha": 1.0, "prob": 1.0, "switch_prob": 0.5, "mode": "elem"}
    assert (sm.erase_prob, sm.erase_fill, sm.rank) == (0.25, 0, 2)
    a.train = False
    assert cli.make_mix(a, 0, None) is None                                 # evaluation never mixes
    assert cli.make_mix(cli.parse_args(["--train", "--loss", "aucm", "--erase_prob", "0.5"]), 0, None) is not None
    for argv, word in ((["--mixup", "-0.1"], "--mixup"), (["--cutmix", "-1"], "--cutmix"), (["--mix_prob", "1.5"], "--mix_prob"),
                       (["--mix_prob", "-0.5"], "--mix_prob"), (["--mix_switch_prob", "2"], "--mix_switch_prob"),
                       (["--erase_prob", "1.01"], "--erase_prob"), (["--erase_fill", "256"], "--erase_fill"),
                       (["--mix_mode", "row"], "--mix_mode"),
                       (["--mixup", "0.4", "--loss", "aucm"], "aucm"), (["--cutmix", "1.0", "--loss", "aucm"], "aucm")):
        with pytest.raises(SystemExit) as ei:
            cli.parse_args(["--train"] + argv)
        assert ei.value.code == 2
        assert word in capsys.readouterr().err


def test_binding_header_and_makefile():
    from chexpert_amd import _lib
    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "chexpert_hip.h")).read(), flags=re.S)
    for name, n in (("cx_u8_mix", 10), ("cx_target_mix", 7)):
        m = re.search(r"\bint\s+%s\s*\(([^;{]*?)\)\s*;" % name, hdr, flags=re.S)
        assert m and len(_lib.SIGNATURES[name]) == m.group(1).count(",") + 1 == n
    mk = open(os.path.join(ROOT, "chexpert_amd", "csrc", "Makefile")).read()
    assert "mix.hip" in mk
    rule = [l for l in mk.splitlines() if "-ffp-contract=off" in l and not l.startswith("#")]
    assert rule and all("mix.o" in l and "saliency.o" in l for l in rule)
