"""CPU (no GPU): the host side of the uncertain-label policies -- the five policies of ChexpertCSV on a small csv, the synthetic
uncertain labels, compute_metrics leaving ignored rows out, the command line (flags, `--pos_weight auto`), and the argument
checks of cx_bce_masked_fwd_bwd before any launch."""
import json
import math
import os
import warnings

import numpy as np
import pytest
import torch

from chexpert_amd import cli, data, metrics, synth

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# one row per line: the five findings; "" is a blank.  Every class holds -1, a blank, 0 and 1.
_ROWS = [
    ("-1", "", "0", "1", "-1"),
    ("", "0", "1", "-1", ""),
    ("0", "1", "-1", "", "0"),
    ("1", "-1", "", "0", "1"),
    ("-1", "-1", "-1", "-1", "-1"),
    ("1", "0", "1", "0", "1"),
]


def _write_csv(folder, name, rows):
    os.makedirs(folder, exist_ok=True)
    with open(os.path.join(folder, name), "w") as f:
        f.write("Path,Sex," + ",".join(data.ATTR_NAMES) + "\n")
        for i, r in enumerate(rows):
            f.write("%s/train/patient%05d/study1/view1_frontal.jpg,Male,%s\n" % (data.DIR_NAME, i, ",".join(r)))


@pytest.fixture()
def root(tmp_path):
    folder = os.path.join(str(tmp_path), data.DIR_NAME)
    _write_csv(folder, "train.csv", _ROWS)
    _write_csv(folder, "valid.csv", _ROWS)
    return str(tmp_path)


def _raw():
    """The table as numbers: blank -> nan."""
    return np.array([[float(v) if v else float("nan") for v in r] for r in _ROWS], dtype=np.float32)


def test_five_policies_on_a_small_csv(root):
    raw = _raw()
    unc, blank = raw == -1, np.isnan(raw)
    hard = ~unc & ~blank
    for c in range(raw.shape[1]):                                      # the premise: each class holds -1, a blank, 0 and 1
        assert unc[:, c].any() and blank[:, c].any() and (raw[:, c] == 0).any() and (raw[:, c] == 1).any()
    got = {p: data.ChexpertCSV(root, "train", uncertain=p, seed=3).targets for p in data.UNCERTAIN_POLICIES}
    for p, t in got.items():
        assert t.dtype == torch.float32 and tuple(t.shape) == raw.shape
        t = t.numpy()
        assert np.array_equal(t[hard], raw[hard]), p                   # certain labels stay
        assert (t[blank] == 0).all(), p                                # blanks still go to 0
    assert (got["ones"].numpy()[unc] == 1).all()
    assert (got["zeros"].numpy()[unc] == 0).all()
    assert (got["ignore"].numpy()[unc] == -1).all() and (got["ignore"].numpy()[~unc] >= 0).all()
    lo = got["ones_lsr"].numpy()[unc]
    assert (lo >= 0.55).all() and (lo <= 0.85).all() and len(set(lo.tolist())) > len(lo) // 2
    lz = got["zeros_lsr"].numpy()[unc]
    assert (lz >= 0.0).all() and (lz <= 0.3).all() and len(set(lz.tolist())) > len(lz) // 2
    # the default is U-Ones, byte for byte the labels of the reference's statement (dataset.py:139-142)
    import pandas as pd
    df = pd.read_csv(os.path.join(root, data.DIR_NAME, "train.csv"), keep_default_na=True)
    today = torch.tensor(df[data.ATTR_NAMES].fillna(0).replace(-1, 1).values.astype(np.float32))
    assert torch.equal(data.ChexpertCSV(root, "train").targets, today)
    assert torch.equal(got["ones"], today)
    # reproducible draws: one seed, one table; another seed, another table
    for p in ("ones_lsr", "zeros_lsr"):
        assert torch.equal(data.ChexpertCSV(root, "train", uncertain=p, seed=3).targets, got[p])
        assert not torch.equal(data.ChexpertCSV(root, "train", uncertain=p, seed=4).targets, got[p])
    # a draw belongs to its row of the file: a shorter table reads the same values
    assert torch.equal(data.ChexpertCSV(root, "train", uncertain="ones_lsr", seed=3, mini_data=3).targets, got["ones_lsr"][:3])
    with pytest.raises(ValueError):
        data.ChexpertCSV(root, "train", uncertain="twos")


def test_policies_leave_the_validation_table_alone(root):
    want = data.ChexpertCSV(root, "valid").targets
    assert (want == -1).any()                                          # the file is used as it is (blanks to 0)
    for p in data.UNCERTAIN_POLICIES:
        assert torch.equal(data.ChexpertCSV(root, "valid", uncertain=p, seed=9).targets, want), p


def test_synthetic_uncertain_labels():
    N, C, seed = 4000, 5, 7
    today = synth.targets(seed + 1, N, C)
    assert torch.equal(cli.SyntheticXrays(N, 8, C, seed).targets, today)
    assert torch.equal(cli.SyntheticXrays(N, 8, C, seed, uncertain_frac=0.0, uncertain="ignore").targets, today)
    t = cli.SyntheticXrays(N, 8, C, seed, uncertain_frac=0.2, uncertain="ignore").targets
    share = float((t < 0).float().mean())
    sigma = math.sqrt(0.2 * 0.8 / (N * C))
    print("share of -1 at frac 0.2: %.4f (4 sigma = %.4f)" % (share, 4 * sigma))
    assert abs(share - 0.2) <= 4 * sigma
    assert torch.equal(t[t >= 0], today[t >= 0])                       # the other labels are today's
    # independent of the label draw: the marked share is the same among today's positives and negatives
    for v in (0.0, 1.0):
        sel = today == v
        s = float((t[sel] < 0).float().mean())
        assert abs(s - 0.2) <= 4 * math.sqrt(0.2 * 0.8 / int(sel.sum())), (v, s)
    ones = cli.SyntheticXrays(N, 8, C, seed, uncertain_frac=0.2, uncertain="ones").targets
    assert torch.equal(ones, torch.where(t < 0, torch.ones_like(t), today))
    lsr = cli.SyntheticXrays(N, 8, C, seed, uncertain_frac=0.2, uncertain="zeros_lsr").targets
    assert (lsr[t < 0] >= 0).all() and (lsr[t < 0] <= 0.3).all() and torch.equal(lsr[t >= 0], today[t >= 0])


def test_compute_metrics_leaves_ignored_rows_out():
    N, C = 120, 5
    logits = synth.uniform(31, (N, C), -3, 3).numpy().astype(np.float64)
    tg = synth.targets(32, N, C, p=0.35).numpy().astype(np.float64)
    losses = synth.uniform(33, (N, C), 0.0, 2.0).numpy().astype(np.float64)
    mask = synth.uniform01(34, N * C).reshape(N, C) < 0.25
    masked = tg.copy()
    masked[mask] = -1
    got = metrics.compute_metrics(logits, masked, losses)
    assert set(got) == {"fpr", "tpr", "aucs", "precision", "recall", "loss"}
    for c in range(C):
        keep = ~mask[:, c]
        assert 0 < keep.sum() < N
        want = metrics.compute_metrics(logits[keep][:, c:c + 1], tg[keep][:, c:c + 1], losses[keep][:, c:c + 1])
        for k in ("fpr", "tpr", "aucs", "precision", "recall", "loss"):
            assert got[k][c] == want[k][0], (k, c)
    # a class with every label ignored: no curve, nan, and mean_auc skips it
    masked[:, 2] = -1
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        g2 = metrics.compute_metrics(logits, masked, losses)
    assert np.isnan(g2["aucs"][2]) and np.isnan(g2["loss"][2]) and g2["fpr"][2] == []
    assert g2["aucs"][0] == got["aucs"][0] and not np.isnan(metrics.mean_auc(g2))


def test_compute_metrics_without_negatives_reproduces_the_fixture():
    cases = json.load(open(os.path.join(ROOT, "tests", "golden", "auroc.json")))
    for c in cases.values():
        logits = synth.uniform(c["seed"], (c["n"], c["c"]), -3, 3).numpy().astype(np.float64)
        tg = synth.targets(c["seed"] + 100, c["n"], c["c"], p=0.35).numpy()
        if c["variant"] == 1:
            logits = np.round(logits)
        if c["variant"] == 2:
            tg[:, 1] = 0
            tg[:, 3] = 1
        if c["variant"] == 3:
            logits[:, 0] = 0.25
        losses = synth.uniform(c["seed"] + 200, tg.shape, 0.0, 2.0).numpy()
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")
            m = metrics.compute_metrics(logits, tg, losses)
            # ignored rows added to the table change nothing
            extra = np.full((7, c["c"]), -1.0)
            m2 = metrics.compute_metrics(np.r_[logits, np.zeros((7, c["c"]))], np.r_[tg, extra], np.r_[losses, np.full((7, c["c"]), 9.0)])
        for i, want in enumerate(c["aucs"]):
            assert (np.isnan(m["aucs"][i]) if want is None else abs(m["aucs"][i] - want) < 1e-12)
            assert (np.isnan(m2["aucs"][i]) if want is None else m2["aucs"][i] == m["aucs"][i])
            assert m2["loss"][i] == float(losses.astype(np.float64)[:, i].mean())
        assert abs(metrics.mean_auc(m) - c["nanmean"]) < 1e-12
        assert m["loss"] == dict(enumerate(losses.astype(np.float64).mean(0).tolist()))


def test_parser_flags_and_pos_weight_auto():
    a = cli.build_parser().parse_args([])
    assert (a.uncertain, a.pos_weight, a.synthetic_uncertain) == ("ones", None, 0.0)
    a = cli.build_parser().parse_args(["--uncertain", "ignore", "--pos_weight", "auto", "--synthetic_uncertain", "0.2"])
    assert (a.uncertain, a.pos_weight, a.synthetic_uncertain) == ("ignore", ["auto"], 0.2)
    for p in ("ones", "zeros", "ignore", "ones_lsr", "zeros_lsr"):
        assert cli.build_parser().parse_args(["--uncertain", p]).uncertain == p
    with pytest.raises(SystemExit):
        cli.build_parser().parse_args(["--uncertain", "maybe"])
    a = cli.build_parser().parse_args(["--pos_weight", "1", "2.5", "3", "4", "0.5"])
    assert cli.resolve_pos_weight(a.pos_weight, None, 5) == [1.0, 2.5, 3.0, 4.0, 0.5]
    with pytest.raises(ValueError):
        cli.resolve_pos_weight(["1", "2"], None, 5)
    assert cli.resolve_pos_weight(None, None, 5) is None
    # hand-made table; per class (non-ignored negatives) / (positives), soft labels by value, clamp to [1/16, 16]
    t = torch.tensor([[1.0, 0.0, -1.0, 1.0, 0.0, 0.25],
                      [0.0, 0.0, 1.0, 1.0, 0.0, 0.75],
                      [0.0, -1.0, 0.0, 1.0, 0.0, -1.0],
                      [0.0, 1.0, 0.0, 1.0, -1.0, 0.5]])
    t = torch.cat([t, torch.tensor([[0.0, 0.0, 0.0, 1.0, 0.0, -1.0]]).repeat(36, 1)])          # 40 rows
    w = cli.resolve_pos_weight(["auto"], t, 6)
    #   class 0: 39 negatives / 1 positive -> clamped to 16      class 1: 38 / 1 (one ignored) -> 16
    #   class 2: 38 / 1 -> 16, class 3: 0 / 40 -> clamped to 1/16, class 4: no positive -> 16
    #   class 5: values 0.25, 0.75, 0.5 -> positives 1.5, negatives 1.5 -> 1
    assert w == [16.0, 16.0, 16.0, 1.0 / 16, 16.0, 1.0]
    t2 = torch.tensor([[1.0, 0.0], [0.0, -1.0], [0.0, 1.0], [-1.0, 1.0], [0.0, 0.0]])
    assert cli.resolve_pos_weight(["auto"], t2, 2) == [3.0, 1.0]      # inside the clamp: 3 / 1 and 2 / 2


def test_flag_values_are_checked_before_anything_runs(tmp_path):
    for bad in (["1", "2", "-3", "4", "5"], ["1", "0", "3", "4", "5"], ["1", "nan", "3", "4", "5"], ["1", "inf", "3", "4", "5"]):
        with pytest.raises(ValueError):
            cli.resolve_pos_weight(bad, None, 5)
    out = str(tmp_path / "o")
    for f in ("-0.1", "1.5", "nan"):
        with pytest.raises(ValueError):
            cli.main(["--train", "--synthetic", "16", "--synthetic_uncertain", f, "--output_dir", out])
    with pytest.raises(ValueError):                                    # nothing synthetic to mark
        cli.main(["--train", "--data_path", str(tmp_path), "--synthetic_uncertain", "0.2", "--output_dir", out])
    assert not os.path.exists(out)                                     # refused before the run wrote anything


def test_masked_bce_entry_point_validates_without_launching():
    """cx_bce_masked_fwd_bwd checks its arguments before any launch (no GPU needed): null logits / target, B <= 0, n <= 0."""
    from chexpert_amd import _lib
    f = _lib.lib().cx_bce_masked_fwd_bwd
    x, t, o = torch.zeros(16), torch.zeros(16), torch.zeros(16)
    assert f(None, t.data_ptr(), None, o.data_ptr(), None, None, 1.0, 2, 5, None) == -1          # CX_EINVAL
    assert f(x.data_ptr(), None, None, o.data_ptr(), None, None, 1.0, 2, 5, None) == -1
    assert f(x.data_ptr(), t.data_ptr(), None, o.data_ptr(), None, None, 1.0, 0, 5, None) == -1
    assert f(x.data_ptr(), t.data_ptr(), None, o.data_ptr(), None, None, 1.0, -3, 5, None) == -1
    assert f(x.data_ptr(), t.data_ptr(), None, o.data_ptr(), None, None, 1.0, 2, 0, None) == -1
    assert f(x.data_ptr(), t.data_ptr(), None, o.data_ptr(), None, None, 1.0, 2, -1, None) == -1
    assert _lib.lib().cx_abi_version() == 10                           # an additive entry point


def test_set_loss_is_no_state_and_the_loss_module_has_no_cpu_path():
    from chexpert_amd.loss import MaskedBCE
    from chexpert_amd.models import DenseNet
    model = DenseNet(32, (2, 2, 2, 2), 64, num_classes=5)
    keys = list(model.state_dict().keys())
    assert (model.loss_ignore_negative, model.loss_pos_weight) == (False, None)
    assert model.set_loss(ignore_negative=True) is model and model.loss_ignore_negative and model.loss_pos_weight is None
    assert list(model.state_dict().keys()) == keys and not any("pos_weight" in n for n, _ in model.named_buffers())
    model.set_loss()
    assert (model.loss_ignore_negative, model.loss_pos_weight) == (False, None)
    with pytest.raises(RuntimeError):
        model.set_loss(pos_weight=[1.0] * 5)                           # the weights live on the device: model.to(device) first
    with pytest.raises(RuntimeError):
        MaskedBCE()(torch.zeros(2, 5), torch.zeros(2, 5))              # device tensors only
    with pytest.raises(RuntimeError):
        MaskedBCE().elementwise(torch.zeros(2, 5), torch.zeros(2, 5))
    # the options select the kernel as set_loss does: neither of them -> the plain loss
    assert MaskedBCE().masked and MaskedBCE(ignore_negative=False, pos_weight=[1.0] * 5).masked
    assert not MaskedBCE(ignore_negative=False).masked
