"""CPU (no GPU): host logic, the C-ABI library's exported symbols, state_dict compatibility,
data-parallel gradient bucketing over gloo (world_size 2)."""
import ctypes
import os
import re
import subprocess
import sys

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_library_exports_every_declared_symbol():
    from chexpert_amd import _lib
    hdr = open(os.path.join(ROOT, "include", "chexpert_hip.h")).read()
    declared = set(re.findall(r"\b(cx_[a-z0-9_]+)\s*\(", hdr))
    assert declared, "no declarations found"
    lib = ctypes.CDLL(_lib.LIB_PATH)          # built by __graft_entry__.build(); loads without a GPU
    for name in sorted(declared):
        assert hasattr(lib, name), "libchexpert_hip.so does not export %s" % name
    assert declared == set(_lib.SIGNATURES), (declared ^ set(_lib.SIGNATURES))
    assert _lib.lib().cx_abi_version() == 10
    assert _lib.lib().cx_error_string(-3) == b"unsupported shape"
    # every binding passes exactly the parameters the header declares (a short argtypes list makes ctypes pass the rest as 32-bit
    # ints: truncated device pointers, i.e. a GPU memory fault instead of an error)
    code = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    for m in re.finditer(r"\b(?:int|const char\*)\s+(cx_[a-z0-9_]+)\s*\(([^;{]*?)\)\s*;", code, flags=re.S):
        name, args = m.group(1), m.group(2).strip()
        n = 0 if args in ("", "void") else args.count(",") + 1
        assert len(_lib.SIGNATURES[name]) == n, "%s: header declares %d parameters, the binding passes %d" % (name, n, len(_lib.SIGNATURES[name]))


def test_product_library_never_reads_the_environment():
    """No environment variable can change what the shipped library computes: dispatch / ablation switches exist only in the
    diagnostic builds (`make -C chexpert_amd/csrc diag`, -DCX_DIAG / -DCX_DIAG_TIMING), where `cx_diag_int` / `cx_diag_set` wrap
    the ONE getenv call of the sources."""
    from chexpert_amd import _lib
    und = subprocess.run(["nm", "-D", "--undefined-only", _lib.LIB_PATH], capture_output=True, text=True, check=True).stdout
    assert "getenv" not in und, "libchexpert_hip.so imports getenv"
    # ... and exports no debugging hook: the dbg_* selectors / event taps of earlier ABIs mutated process-wide state (kernel choice is
    # the per-call CxConv.kernel_hint / CxWgrad.kernel_hint field since ABI 10; stamps and event taps exist in -DCX_DIAG builds only)
    defined = subprocess.run(["nm", "-D", "--defined-only", _lib.LIB_PATH], capture_output=True, text=True, check=True).stdout
    dbg = [l.split()[-1] for l in defined.splitlines() if l.split() and l.split()[-1].startswith("dbg_")]
    assert not dbg, "libchexpert_hip.so exports debug hooks: %s" % dbg
    csrc = os.path.join(ROOT, "chexpert_amd", "csrc")
    for f in sorted(os.listdir(csrc)):
        if f.endswith((".hip", ".h")):
            src = open(os.path.join(csrc, f)).read()
            n = len(re.findall(r"\bgetenv\s*\(", src))
            if f == "common.h":           # the two helpers, both inside #ifdef CX_DIAG
                head = src[:src.index("#else")]
                assert n == 2 and head.count("getenv(") == 2 and "#ifdef CX_DIAG" in head
            else:
                assert n == 0, "%s calls getenv directly" % f
            # the timing-only ablations (results wrong) sit behind the second flag
            for name in ("CX_PW_BWD_DBG", "CX_WGRAD_MM_NOSTORE"):
                for m in re.finditer(r'cx_diag_(?:int|set)\("%s"' % name, src):
                    before = src[:m.start()]
                    assert before.rfind("#ifdef CX_DIAG_TIMING") > before.rfind("#endif"), "%s: %s outside CX_DIAG_TIMING" % (f, name)


def test_only_ops_and_the_binding_touch_the_library():
    """`ops.py` is the one tensor-level layer over the C ABI: no other module of the package names `lib` (imported, called or as
    `_lib.lib`), so every launch passes a wrapper's shape / dtype / pitch checks."""
    import ast
    pkg = os.path.join(ROOT, "chexpert_amd")
    seen = []
    for d, _, files in os.walk(pkg):
        for f in sorted(files):
            if not f.endswith(".py"):
                continue
            path = os.path.join(d, f)
            rel = os.path.relpath(path, pkg)
            for node in ast.walk(ast.parse(open(path).read(), path)):
                names = [node.id] if isinstance(node, ast.Name) else [node.attr] if isinstance(node, ast.Attribute) else \
                    [a.name for a in node.names] if isinstance(node, ast.ImportFrom) else []
                if "lib" in names:
                    seen.append(rel)
    assert set(seen) == {"ops.py", "_lib.py"}, "the library is reached outside ops.py / _lib.py: %s" % sorted(set(seen))


def test_validation_codes_without_launching():
    """Argument validation happens before any launch, so it can be exercised without a GPU."""
    from chexpert_amd import _lib
    p = _lib.CxConv()
    assert _lib.lib().cx_conv_gemm(ctypes.byref(p), None) == -1           # CX_EINVAL: null pointers
    w = _lib.CxWgrad()
    assert _lib.lib().cx_conv_wgrad(ctypes.byref(w), None) == -1
    bt = _lib.CxWgradBatch()
    assert _lib.lib().cx_conv3x3_wgrad_batch(ctypes.byref(w), ctypes.byref(bt), None) == -1      # n = 0
    assert ctypes.sizeof(_lib.CxWgradBatch) == 5 * 8 * _lib.WGRAD_BATCH_MAX + 8
    assert ctypes.sizeof(_lib.CxConv) == 15 * 8 + 24 * 4 + 8 + 8 + 8 + 3 * 8 + 8     # ... pro_out, ldpo + pad_, emask (ABI 8), x3, po_lo, po_mask (ABI 9), kernel_hint + pad (ABI 10)
    assert _lib.lib().cx_adam_step(None, None, None, None, 0, 0.0, 0.0, 0.0, 0.0, 0.0, 1, 1.0, None) == -1


def test_state_dict_surface_matches_reference_keys():
    from chexpert_amd.models import DenseNet, densenet121
    from oracle import nets
    m = densenet121(num_classes=5)
    spec = nets.densenet_spec(5)
    sd = m.state_dict()
    assert list(sd.keys()) == list(spec.keys())                    # 727 torchvision keys, reference order
    assert all(tuple(sd[k].shape) == tuple(spec[k]) for k in spec)
    assert sum(p.numel() for p in m.parameters()) == 6958981
    # attribute surface used by chexpert.py:464-468
    assert m.classifier.in_features == 1024
    m.classifier = torch.nn.Linear(m.classifier.in_features, 14)
    assert sum(p.numel() for p in m.parameters()) == 6968206
    assert m.features.norm5.num_features == 1024 and hasattr(m.features, "transition3")
    assert m._get_name() == "DenseNet"
    with pytest.raises(RuntimeError):
        m(torch.zeros(1, 3, 64, 64))                               # CPU tensor: no fallback
    with pytest.raises(RuntimeError):
        m.features.conv0(torch.zeros(1, 3, 64, 64))                # sub-modules only hold parameters


def _no_overlap(spans, vec_size):
    spans = sorted(s for s in spans if s[1] > 0)
    for (a, n), (b, _) in zip(spans, spans[1:]):
        assert a + n <= b
    assert spans[0][0] >= 0 and spans[-1][0] + spans[-1][1] <= vec_size


def test_engine_vector_plan_and_block_geometry():
    from chexpert_amd.models import Bottleneck, DenseNet, ResNet
    from chexpert_amd.models.efficientnet import construct_model
    eng = DenseNet(32, (6, 12, 24, 16), 64, num_classes=5)._eng()
    assert eng.blocks == [(64, 6), (128, 12), (256, 24), (512, 16)] and eng.c_final == 1024
    b0, bn = eng.bwd_zero
    assert 0 <= b0 and b0 + bn <= eng.vec_size
    assert not hasattr(eng, "fwd_zero")                # nothing is zeroed per forward: the statistics are rows of the workspace's slab
    # the layout: every later refactor of the engine is checked by the equality of its call lists, which rests on these offsets
    slots = list(eng.vector_slots())
    assert (len(slots), len([s for s in slots if s[1] > 0])) == (731, 730)
    assert eng.vec_size == 139648 and eng.bwd_zero == (104256, 5632)
    # the zeroed region is the blocks' accumulators A / Bc and nothing else
    assert bn == 2 * sum(c + n * 32 for c, n in eng.blocks)
    assert (b0, b0 + bn) == (eng.plan.blocks[0].A[0], eng.plan.blocks[-1].Bc[0] + eng.plan.blocks[-1].Bc[1])
    # slots never overlap
    _no_overlap(slots, eng.vec_size)
    # ResNet and EfficientNet: seven coefficient slots per BatchNorm and the engine's own behind them, no zeroed region at all
    bn_slots = lambda e: [s for S in e.bn.values() for s in (S.sc, S.sh, S.mean, S.rstd, S.pa, S.pb, S.pc)]
    res = ResNet(Bottleneck, [3, 4, 6, 3], num_classes=5)._eng()
    assert len(res.bn) == 53 and res.vec_size == 239424
    _no_overlap(bn_slots(res) + [s for j in res.join for s in j] + [res.ones, res.zeros] + res.scratch, res.vec_size)
    eff = construct_model("efficientnet-b0", 5)._eng()
    assert len(eff.bn) == 49 and eff.vec_size == 148336
    _no_overlap(bn_slots(eff) + [eff.ones], eff.vec_size)
    for e in (res, eff):
        assert not hasattr(e, "fwd_zero") and not hasattr(e, "bwd_zero")


_DP_WORKER = r"""
import os, sys, torch, torch.distributed as dist
sys.path.insert(0, %r)
from chexpert_amd.parallel import GradReducer
rank, world = int(os.environ["RANK"]), int(os.environ["WORLD_SIZE"])
dist.init_process_group("gloo")
n = 100003
g = torch.arange(n, dtype=torch.float32) * (rank + 1)
red = GradReducer(g, bucket_bytes=40000)
red.begin()
for lo in (90000, 70000, 69000, 30000, 12):       # backward hands ranges over from the end of the buffer
    red.ready(lo)
red.finish()
want = torch.arange(n, dtype=torch.float32) * (sum(range(1, world + 1)) / world)
assert torch.allclose(g, want), (g[:4], want[:4])
covered = sorted(red.ranges)
assert covered[0][0] == 0 and covered[-1][1] == n and all(a[1] == b[0] for a, b in zip(covered, covered[1:]))
assert len(covered) >= 3, covered
dist.destroy_process_group()
print("rank", rank, "ok")
"""


def test_gradient_reducer_world2_gloo(tmp_path):
    script = tmp_path / "dp_worker.py"
    script.write_text(_DP_WORKER % ROOT)
    r = subprocess.run([sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node=2", "--master-addr",
                        "127.0.0.1", "--master-port", "29533", str(script)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    assert r.stdout.count("ok") == 2


def test_product_auroc_matches_sklearn_fixture():
    """chexpert_amd.metrics (product, host-side) against the sklearn outputs recorded through the reference's
    compute_metrics (tests/golden/auroc.json)."""
    import json
    import warnings
    import numpy as np
    from chexpert_amd import metrics, synth
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
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")
            m = metrics.compute_metrics(logits, tg, np.zeros_like(tg))
        for i, want in enumerate(c["aucs"]):
            assert (np.isnan(m["aucs"][i]) if want is None else abs(m["aucs"][i] - want) < 1e-12)
        assert abs(metrics.mean_auc(m) - c["nanmean"]) < 1e-12
        assert set(m) == {"fpr", "tpr", "aucs", "precision", "recall", "loss"}


def test_cli_flags_and_checkpoint_tracker(tmp_path):
    from chexpert_amd import cli
    a = cli.build_parser().parse_args([])
    assert (a.batch_size, a.lr, a.n_epochs, a.log_interval, a.eval_interval, a.lr_decay_factor, a.model) == \
        (16, 1e-4, 1, 50, 300, 0.97, "densenet121")                     # defaults of chexpert.py:29-57
    assert cli.build_parser().parse_args(["--evaluate"]).evaluate_single_model
    # tracker keeps the 3 best by AvgAUC, re-using the evicted record's file id (chexpert.py:106-123)
    import numpy as np
    args = cli.build_parser().parse_args(["--output_dir", str(tmp_path)])
    for step, aucv in enumerate([0.70, 0.80, 0.60, 0.75, 0.90, 0.50], 1):
        args.step = step
        cli.save_checkpoint({"global_step": step, "eval_loss": 1.0, "avg_auc": aucv, "state_dict": {}}, {}, None, args,
                            max_records=3)
    rec = np.loadtxt(os.path.join(str(tmp_path), "checkpoints_tracker.csv"), skiprows=1)
    assert rec[:, 3].tolist() == [0.90, 0.80, 0.75]
    assert sorted(rec[:, 0].astype(int).tolist()) == [0, 1, 2]
    assert sorted(os.listdir(os.path.join(str(tmp_path), "best_checkpoints"))) == ["checkpoint_0.pt", "checkpoint_1.pt", "checkpoint_2.pt"]


_SHARD_WORKER = r"""
import os, sys, torch, torch.distributed as dist
sys.path.insert(0, %r)
from chexpert_amd import parallel as P
rank, world, _ = P.dist_info()
dist.init_process_group("gloo")
# sampler: the two ranks partition one shared permutation, equal counts, different epochs differ
a = P.shard_indices(11, rank, world, seed=3, epoch=0)
both = [None, None]
dist.all_gather_object(both, a)
assert len(both[0]) == len(both[1]) == 5 and not set(both[0]) & set(both[1])
assert P.shard_indices(11, rank, world, seed=3, epoch=1) != a
# sharded evaluation: ragged row blocks come back in rank order on every rank
n = 3 + 2 * rank
t = torch.arange(n * 5, dtype=torch.float32).view(n, 5) + 100 * rank
g = P.gather_rows(t)
want = torch.cat([torch.arange(3 * 5, dtype=torch.float32).view(3, 5), torch.arange(5 * 5, dtype=torch.float32).view(5, 5) + 100])
assert torch.equal(g, want), g
e = P.gather_rows(torch.zeros(0 if rank == 0 else 2, 5))
assert e.shape == (2, 5)
dist.destroy_process_group()
print("rank", rank, "ok")
"""


def test_sampler_shards_and_ragged_gather_world2_gloo(tmp_path):
    """The data-parallel loop of chexpert_amd/cli.py: rank-sharded sampler and the all-gather of the
    (N,5) validation logits, two processes over gloo."""
    script = tmp_path / "shard_worker.py"
    script.write_text(_SHARD_WORKER % ROOT)
    r = subprocess.run([sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node=2", "--master-addr",
                        "127.0.0.1", "--master-port", "29534", str(script)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    assert r.stdout.count("ok") == 2


def test_fused_optimiser_state_dict_round_trip():
    from chexpert_amd.optim import FusedAdam, FusedRMSprop

    class _Eng:
        flat = torch.zeros(10)
        flat_grad = torch.zeros(10)

    class _M:
        def _eng(self):
            return _Eng
    a = FusedAdam(_M(), lr=1e-3)
    a.step_count, a.lr = 7, 5e-4
    a._state = [torch.arange(10.0), torch.arange(10.0) * 2]
    sd = a.state_dict()
    b = FusedAdam(_M(), lr=1.0)
    b.load_state_dict(sd)
    assert (b.step_count, b.lr) == (7, 5e-4)
    _, _, st = b._bufs(2)
    assert torch.equal(st[1], torch.arange(10.0) * 2)
    import pytest
    with pytest.raises(RuntimeError):
        FusedRMSprop(_M(), lr=1.0).load_state_dict(sd)


def test_reference_parameter_counts_and_import_paths():
    """The known answers of the reference's only self-test (attn_aug_conv.py:522-655: parameter counts of the papers) through the
    reference's own import paths (`models.attn_aug_conv`, `models.efficientnet`; chexpert.py:25-26)."""
    from models.attn_aug_conv import BasicBlock, Bottleneck, DenseNet, ResNet, WideResNet
    from models.efficientnet import SCALING_PARAMS, construct_model
    n = lambda m: round(sum(p.numel() for p in m.parameters()) * 1e-6, 1)
    attn = lambda k, v, nh, d: {"k": k, "v": v, "nh": nh, "relative": True, "input_dims": d}
    assert n(DenseNet(12, (16, 16, 16), 24, num_classes=10)) == 0.8                       # :530
    assert n(DenseNet(24, (41, 41, 41), 48, num_classes=10)) == 15.3                      # :537
    assert n(DenseNet(40, (31, 31, 31), 80, num_classes=10)) == 25.6                      # :545
    assert sum(p.numel() for p in DenseNet(32, (6, 12, 24, 16), 64).parameters()) == 7978856
    assert n(WideResNet(BasicBlock, 28, 10, num_classes=100, attn_params=attn(.2, .1, 8, (32, 32)))) == 36.2        # :602
    assert n(ResNet(BasicBlock, [3, 4, 6, 3])) == 21.8                                    # :610
    assert n(ResNet(Bottleneck, [3, 4, 6, 3])) == 25.6                                    # :616
    assert n(ResNet(BasicBlock, [3, 4, 6, 3], attn_params=attn(.25, .25, 8, (224, 224)))) == 20.7                  # :623
    assert n(ResNet(Bottleneck, [3, 4, 6, 3], attn_params=attn(.2, .1, 8, (224, 224)))) == 25.8                    # :629
    for k, want in ((.25, 24.3), (.5, 22.3), (.75, 20.7), (1, 19.4)):                       # :635-653
        assert n(ResNet(Bottleneck, [3, 4, 6, 3], attn_params=attn(k, k, 8, (224, 224)))) == want
    assert set(SCALING_PARAMS) == {"efficientnet-b%d" % i for i in range(8)}
    assert sum(p.numel() for p in construct_model("efficientnet-b0", 5).parameters()) == 4013953
    import pytest
    ResNet(BasicBlock, [2, 2, 2, 2])._eng()                # plain BasicBlocks are on the MI355X schedule ...
    with pytest.raises(NotImplementedError):               # ... the attention-augmented ones constructible only
        ResNet(BasicBlock, [2, 2, 2, 2], attn_params=attn(.25, .25, 8, (224, 224)))._eng()
    d = {"k": .2, "v": .1, "nh": 8, "relative": True, "input_dims": (320, 320)}
    DenseNet(32, (6, 12, 24, 16), 64, attn_params=d)
    assert d["input_dims"] == (320, 320)                   # the reference mutates the caller's dict; the drop-in works on a copy


def test_visualisation_figures_from_maps(tmp_path):
    """chexpert_amd/vis.py (chexpert.py:305-397, dataset.py:50-68): the 'vis' subset selection and the two figure kinds, from given maps."""
    import numpy as np
    from chexpert_amd import synth, vis
    t = torch.tensor([[1, 0, 0], [0, 1, 0], [0, 0, 0], [1, 1, 0], [1, 1, 1], [1, 0, 0], [1, 0, 0], [1, 0, 0]], dtype=torch.float32)
    names, groups = vis.select_vis_subset(t, ["A", "B", "C"])
    assert names == ["A", "B", "C", "No findings", "2 conditions", "Multiple conditions"]
    assert groups == [[0, 5, 6], [1], [], [2], [3], [4]]            # three per category at most, in data order
    n = len(t)
    files = vis.visualize(np.random.rand(n, 48, 48), t.numpy(), np.random.randn(n, 3), np.random.rand(n, 48, 48), ["p%d" % i for i in range(n)],
                          ["A", "B", "C"], (names, groups), str(tmp_path), 7)
    assert len(files) == 6 and all(os.path.getsize(f) > 200 for f in files) and os.path.getsize(files[0]) > 5000
    assert os.path.basename(files[3]) == "vis_No_findings_step_7.png"

    class Layer:
        nh = 2
        weights = torch.softmax(torch.randn(1, 2, 16, 16), -1)
    out = vis.vis_attn(torch.randn(1, 3, 64, 64), ["p0"], [5], [Layer()], str(tmp_path))
    assert [os.path.basename(f) for f in out] == ["attn_image_idx_5_0_layer_0.png"]


def test_csv_dataset_u_ones_resize_center_crop(tmp_path):
    """chexpert_amd/data.py against dataset.py:73-153 and chexpert.py:67-69: U-Ones label processing on the training file only, the
    shorter side resized to --resize, centre crop, grey uint8 out, source-row indices, patient ids, the test-csv mode."""
    import numpy as np
    import pandas as pd
    from PIL import Image
    from chexpert_amd import data
    root = tmp_path / data.DIR_NAME
    rows = []
    for split, n in (("train", 5), ("valid", 3)):
        for i in range(n):
            d = root / split / ("patient%05d" % i) / "study1"
            d.mkdir(parents=True)
            w, h = (390 + 7 * i, 320 + 5 * i) if i % 2 == 0 else (330, 412)
            ramp = (np.add.outer(np.arange(h), np.arange(w)) % 256).astype(np.uint8)     # value = (row + col) mod 256
            Image.fromarray(ramp, "L").save(str(d / "view1_frontal.png"))
            rows.append((split, "%s/%s/patient%05d/study1/view1_frontal.png" % (data.DIR_NAME, split, i)))
    nan = float("nan")
    lab = {"train": [[1, nan, -1, 0, 0], [nan, nan, nan, nan, nan], [-1, -1, 1, 0, 1], [0, 1, 0, 0, 0], [1, 1, 1, 1, 1]],
           "valid": [[1, 0, 0, 0, 0], [0, 0, 0, 0, 0], [0, 1, 1, 0, 0]]}
    for split in ("train", "valid"):
        paths = [p for s_, p in rows if s_ == split]
        df = pd.DataFrame({"Path": paths, "Sex": "F", "Frontal/Lateral": ["Frontal"] * (len(paths) - 1) + ["Lateral"]})
        for j, a in enumerate(data.ATTR_NAMES):
            df[a] = [r[j] for r in lab[split]]
        df.to_csv(str(root / (split + ".csv")), index=False)
    tr = data.ChexpertCSV(str(tmp_path), "train", resize=None)
    assert len(tr) == 5 and tr.targets.tolist() == [[1, 0, 1, 0, 0], [0, 0, 0, 0, 0], [1, 1, 1, 0, 1], [0, 1, 0, 0, 0], [1, 1, 1, 1, 1]]
    x, t, idx = tr[0]
    assert x.dtype == torch.uint8 and tuple(x.shape) == (1, 320, 320) and idx == 0
    # no resize: the centre 320 x 320 of the 390 x 320 ramp starts at column 35, row 0
    assert x[0, 0, 0].item() == 35 and x[0, 10, 5].item() == (10 + 40) % 256
    fr = data.ChexpertCSV(str(tmp_path), "train", resize=None, data_filter={"Frontal/Lateral": "Frontal"})
    assert len(fr) == 4
    va = data.ChexpertCSV(str(tmp_path), "valid", resize=224, mini_data=2)
    x, t, idx = va[1]                                   # 330 x 412 -> shorter side 224, then the centre 224 x 224
    assert tuple(x.shape) == (1, 224, 224) and len(va) == 2 and t.tolist() == [0, 0, 0, 0, 0]
    assert list(data.extract_patient_ids(va, [0, 1])) == ["%s/valid/patient%05d/study1" % (data.DIR_NAME, i) for i in (0, 1)]
    vi = data.ChexpertCSV(str(tmp_path), "vis")
    assert vi.vis_attrs[-3:] == ["No findings", "2 conditions", "Multiple conditions"] and vi.vis_idxs[0] == [0] and vi.vis_idxs[5] == [1]
    csv = tmp_path / "test.csv"
    pd.DataFrame({"Path": [str(tmp_path / p) for _, p in rows[:2]]}).to_csv(str(csv), index=False)
    te = data.ChexpertCSV(str(csv), "test", resize=64)
    assert len(te) == 2 and te[0][1].tolist() == [0, 0, 0, 0, 0] and tuple(te[0][0].shape) == (1, 64, 64)


def test_cifar_harness_host_logic(tmp_path):
    """chexpert_amd.cifar (the reference's models/test_model.py): command line, learning-rate schedules against the torch
    schedulers the reference wraps (:176-199), top-k accuracy (:97-101), augmentation shapes and the pickle reader."""
    import math
    import pickle
    import numpy as np
    from chexpert_amd import cifar
    a = cifar.build_parser().parse_args(["--train", "--lr", "0.1", "wideresnet", "16", "4", "--batch_size", "32"])
    assert (a.model, a.architecture, a.train, a.lr, a.batch_size, a.dataset) == ("wideresnet", [16, 4], True, 0.1, 32, "cifar100")
    # warm-up + cosine against torch's CosineAnnealingLR wrapped the way test_model.py:188-199 wraps it
    nb = 4
    a.lr_warmup_epochs, a.lr_cos_max_epochs = 2, 5
    p = torch.nn.Parameter(torch.zeros(1))
    opt = torch.optim.SGD([p], lr=a.lr)

    class Sched(torch.optim.lr_scheduler.CosineAnnealingLR):
        def __init__(self, warm, *args, **kw):
            self.warm = warm
            super().__init__(*args, **kw)

        def get_lr(self):
            if self.last_epoch < self.warm:
                return [b * self.last_epoch / self.warm for b in self.base_lrs]
            return super().get_lr()
    sched = Sched(a.lr_warmup_epochs * nb, opt, T_max=a.lr_cos_max_epochs * nb)
    import warnings
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        for step in range(1, 19):                     # warm-up, then torch's recursive cosine continuing from the last warm-up value
            opt.step()
            sched.step()
            assert abs(opt.param_groups[0]["lr"] - cifar.lr_at(a, step, nb)) < 1e-9, step
    a.model, a.lr_decay_epochs, a.lr_decay_factor = "efficientnet", 1.0, 0.5

    class Stair(torch.optim.lr_scheduler.ExponentialLR):          # the staircase subclass of test_model.py:176-186 behind the warm-up
        def __init__(self, warm, optimizer, gamma, decay_steps):
            self.warm, self.decay_steps = warm, decay_steps
            super().__init__(optimizer, gamma)

        def get_lr(self):
            if self.last_epoch < self.warm:
                return [b * self.last_epoch / self.warm for b in self.base_lrs]
            if self.last_epoch == 0:
                return self.base_lrs
            return [g["lr"] * self.gamma ** (self.last_epoch // self.decay_steps) for g in self.optimizer.param_groups]
    opt = torch.optim.SGD([p], lr=a.lr)
    sched = Stair(a.lr_warmup_epochs * nb, opt, a.lr_decay_factor, a.lr_decay_epochs * nb)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        for step in range(1, 13):
            opt.step()
            sched.step()
            assert abs(opt.param_groups[0]["lr"] - cifar.lr_at(a, step, nb)) < 1e-12 * a.lr + 1e-15, step
    out = torch.tensor([[0.1, 0.5, 0.2, 0.05, 0.05, 0.1, 0.0], [0.9, 0.0, 0.02, 0.03, 0.01, 0.04, 0.0]])
    assert cifar.accuracy(out, torch.tensor([1, 6]), topk=(1, 5)) == [0.5, 0.5]
    x, y = cifar.synthetic_cifar(6, 10, 3)
    g = torch.Generator().manual_seed(1)
    xa = cifar.augment(x, g)
    assert xa.shape == x.shape and xa.dtype == torch.uint8
    n = cifar.normalise(x)
    assert n.shape == (6, 3, 32, 32) and abs(float(n[0, 0, 0, 0]) - (float(x[0, 0, 0, 0]) / 255 - 125.3 / 255) / (63.0 / 255)) < 1e-5
    d = tmp_path / "cifar-10-batches-py"
    d.mkdir()
    for i in range(1, 6):
        pickle.dump({"data": np.full((2, 3072), i, dtype=np.uint8), "labels": [i, 9 - i]}, open(d / ("data_batch_%d" % i), "wb"))
    xs, ys = cifar.load_cifar("cifar10", str(tmp_path), True)
    assert xs.shape == (10, 3, 32, 32) and ys.tolist() == [1, 8, 2, 7, 3, 6, 4, 5, 5, 4] and int(xs[4, 0, 0, 0]) == 3
    lb = cifar.Batches(xs, ys, 4, shuffle=False, aug=False, seed=0)
    assert len(lb) == 3 and [b[1].tolist() for b in lb][2] == [5, 4]


def test_ring_loader_workers_fill_shared_ring(tmp_path):
    """chexpert_amd/loader.py: worker processes decode into the shared uint8 ring; batches arrive in order, the last one partial
    (the reference's DataLoader keeps it, chexpert.py:76), a pass abandoned half-way does not leak into the next one, and the
    decoded bytes equal the dataset's own __getitem__ (generated JPEG folder with the reference's csv columns)."""
    from chexpert_amd.cli import SyntheticXrays
    from chexpert_amd.data import ChexpertCSV
    from chexpert_amd.loader import RingLoader, make_jpeg_folder
    ds = SyntheticXrays(21, 32, 5, 3)
    ld = RingLoader(ds, 8, num_workers=3, slots=2)
    try:
        assert ld.start_method == "fork"                         # nothing has touched a GPU here: workers are plain forks
        for epoch in range(2):
            idx = list(range(21)) if epoch == 0 else list(range(20, -1, -1))
            got = list(ld.batches(idx))
            assert [b[0].shape[0] for b in got] == [8, 8, 5]
            flat = [i for b in got for i in b[2].tolist()]
            assert flat == idx
            for x, t, ii in got:
                for j, i in enumerate(ii.tolist()):
                    assert torch.equal(x[j], ds[i][0]) and torch.equal(t[j], ds[i][1])
        it = ld.batches(list(range(21)))
        next(it)                                                 # abandon the pass after one batch
        del it
        got = list(ld.batches(list(range(16)), drop_last=True))
        assert [b[2].tolist() for b in got] == [list(range(8)), list(range(8, 16))]
        assert torch.equal(got[1][0][3], ds[11][0])
    finally:
        ld.close()
    make_jpeg_folder(str(tmp_path), n=12, w=78, h=64)
    dj = ChexpertCSV(str(tmp_path), "train", resize=48)
    lj = RingLoader(dj, 5, num_workers=2)
    try:
        for x, t, ii in lj.batches(list(range(12))):
            for j, i in enumerate(ii.tolist()):
                assert torch.equal(x[j], dj[i][0]) and torch.equal(t[j], dj[i][1])
            assert set(t.flatten().tolist()) <= {0.0, 1.0}      # U-Ones: blanks -> 0, uncertain -> 1 (dataset.py:139-142)
    finally:
        lj.close()


def test_dataset_logic_against_reference_fixture(tmp_path):
    """chexpert_amd.data.ChexpertCSV against what the REAL reference's ChexpertSmall produced on the same table
    (tests/golden/dataset.json, written by make_golden.py `dataset`): U-Ones processing with / without a data filter
    (dataset.py:134-153), the vis subset (:50-68), mini_data, test mode (:33-37), item labels / source indices (:73-89),
    extract_patient_ids (:156-160)."""
    import json
    import pandas as pd
    from chexpert_amd.data import ChexpertCSV, DIR_NAME, extract_patient_ids
    rec = json.load(open(os.path.join(ROOT, "tests", "golden", "dataset.json")))
    assert rec["attr_names"] == ChexpertCSV.attr_names
    d = tmp_path / DIR_NAME
    d.mkdir()
    pd.DataFrame(rec["train_rows"], columns=rec["columns"]).to_csv(d / "train.csv", index=False)
    pd.DataFrame(rec["valid_rows"], columns=rec["columns"]).to_csv(d / "valid.csv", index=False)
    for tag, flt in (("plain", None), ("filtered", {"Frontal/Lateral": "Frontal"})):
        want = rec[tag]
        tr = ChexpertCSV(str(tmp_path), "train", data_filter=flt)
        assert [int(i) for i in tr.data.index] == want["train_index"]
        assert tr.targets.tolist() == want["train_labels"]
        for k, (lab, src) in zip((0, 5, len(tr) - 1), want["train_items"]):
            assert tr.targets[k].tolist() == lab and int(tr.data.index[k]) == src
    want = rec["plain"]
    assert len(ChexpertCSV(str(tmp_path), "train", mini_data=7)) == want["mini_len"] == 7
    va = ChexpertCSV(str(tmp_path), "valid")
    assert len(va) == want["valid_len"] and va.targets[:6].tolist() == want["valid_labels_head"]
    vis = ChexpertCSV(str(tmp_path), "vis")
    assert vis.vis_attrs == want["vis_attrs"] and vis.vis_idxs == want["vis_idxs"]
    assert [int(i) for i in vis.data.index] == want["vis_index"]
    assert list(extract_patient_ids(va, [0, 3, 17])) == want["patient_ids"]
    tcsv = tmp_path / "paths.csv"
    pd.DataFrame({"Path": [r[0] for r in rec["valid_rows"][:5]]}).to_csv(tcsv, index=False)
    te = ChexpertCSV(str(tcsv), "test")
    assert len(te) == want["test_len"] and te.targets.tolist() == want["test_labels"]


def test_decoded_image_cache_returns_the_same_bytes_without_decoding_again(tmp_path, monkeypatch):
    """ChexpertCSV.enable_decoded_cache (the reference's transform chain, chexpert.py:67-69, has no random step): the second pass
    over the data hands out the first pass's bytes and never opens a file; worker processes fill and read the one shared table."""
    from chexpert_amd import data, loader
    root = str(tmp_path)
    loader.make_jpeg_folder(root, n=12, w=98, h=80)
    ref = data.ChexpertCSV(root, "train", resize=64)
    want = torch.stack([ref[i][0] for i in range(len(ref))])
    ds = data.ChexpertCSV(root, "train", resize=64)
    assert not ds.enable_decoded_cache(max_bytes=1000) and ds.cache_fill() == 0.0
    assert ds.enable_decoded_cache(max_bytes=1 << 20)
    ld = loader.RingLoader(ds, 5, num_workers=2, slots=2)
    try:
        got = torch.cat([x for x, _, _ in ld.batches(list(range(len(ds))))])
        assert torch.equal(got, want) and ds.cache_fill() == 1.0
        calls = []
        monkeypatch.setattr(data, "resize_center_crop", lambda *a, **k: calls.append(1))      # (in this process)
        assert torch.equal(torch.stack([ds[i][0] for i in range(len(ds))]), want) and not calls
        got2 = torch.cat([x for x, _, _ in ld.batches(list(range(len(ds))))])               # workers: from the table they share
        assert torch.equal(got2, want)
    finally:
        ld.close()


def test_decoded_image_cache_shared_by_the_ranks_of_a_node(tmp_path):
    """node_shared: two dataset objects (two ranks of one node) map ONE table under /dev/shm -- a row decoded through the first is
    served to the second without a decode; the creating process unlinks the files at exit."""
    import glob
    from chexpert_amd import data, loader
    if not os.path.isdir("/dev/shm"):
        pytest.skip("no /dev/shm")
    root = str(tmp_path)
    loader.make_jpeg_folder(root, n=6, w=98, h=80)
    code = r"""
import sys, glob, os
sys.path.insert(0, %r)
import torch
from chexpert_amd import data
a = data.ChexpertCSV(%r, "train", resize=64)
b = data.ChexpertCSV(%r, "train", resize=64)
assert a.enable_decoded_cache(max_bytes=1 << 20, node_shared=True) and b.enable_decoded_cache(max_bytes=1 << 20, node_shared=True)
files = glob.glob("/dev/shm/chexpert_amd_cache_%%d_*" %% os.getuid())
assert sorted(f.rsplit(".", 1)[1] for f in files) == ["have", "owner", "rows"], files
assert all((os.stat(f).st_mode & 0o777) == 0o600 for f in files), [oct(os.stat(f).st_mode) for f in files]
x = [a[i][0].clone() for i in range(3)]
assert b.cache_fill() == 0.5
data.resize_center_crop = None                       # a decode through b would now raise
assert all(torch.equal(b[i][0], x[i]) for i in range(3))
print("SHARED-OK")
""" % (ROOT, root, root)
    r = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "SHARED-OK" in r.stdout, r.stderr[-2000:]
    assert not glob.glob("/dev/shm/chexpert_amd_cache_%d_*" % os.getuid()), "the creating process did not unlink the table"
    # a creator that was killed leaves its files behind with `have` flags nobody may trust: the next run starts the table over
    # (the owner file names a dead pid), and a dataset regenerated in the same folder gets another key (index file size / mtime)
    code2 = r"""
import sys, glob, os, signal
sys.path.insert(0, %r)
from chexpert_amd import data
a = data.ChexpertCSV(%r, "train", resize=64)
assert a.enable_decoded_cache(max_bytes=1 << 20, node_shared=True)
if sys.argv[1] == "die":
    a[0]; a[1]
    assert a.cache_fill() > 0
    os.kill(os.getpid(), signal.SIGKILL)
print("FILL %%.3f" %% a.cache_fill())
""" % (ROOT, root)
    r = subprocess.run([sys.executable, "-c", code2, "die"], capture_output=True, text=True, timeout=300)
    assert r.returncode != 0 and len(glob.glob("/dev/shm/chexpert_amd_cache_%d_*" % os.getuid())) == 3, "the killed creator's files stay"
    r = subprocess.run([sys.executable, "-c", code2, "next"], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "FILL 0.000" in r.stdout, (r.stdout, r.stderr[-1500:])
    assert not glob.glob("/dev/shm/chexpert_amd_cache_%d_*" % os.getuid())


def test_library_and_torch_share_one_hip_runtime():
    """Loading libchexpert_hip.so before torch pulled /opt/rocm's libamdhip64 in beside the copy inside the torch wheel: two HIP
    runtimes in one process, and every launch from the library then failed with "no ROCm-capable device" (build() followed by
    smoke() did that).  `_lib.lib()` imports torch first; a fresh interpreter that loads the library first must map ONE runtime."""
    import subprocess
    import sys
    code = ("import sys; sys.path.insert(0, %r)\n"
            "from chexpert_amd import _lib\n_lib.lib()\nimport torch\n"
            "print(len(set(l.split()[-1] for l in open('/proc/self/maps') if 'libamdhip64' in l)))") % os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    out = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stderr[-800:]
    assert out.stdout.strip().splitlines()[-1] == "1", out.stdout


def test_bench_gpus_n_without_world_size_spawns_the_ranks_as_a_child():
    """`python bench.py --gpus 2` (no WORLD_SIZE): the parent builds the two-rank torch.distributed.run command, runs it as a CHILD
    process and relays its exit code -- without importing torch (so it cannot have initialised HIP: no exec / fork hazards)."""
    code = r"""
import json, os, subprocess, sys
sys.path.insert(0, %r)
os.environ.pop("WORLD_SIZE", None)
calls = []
def fake_call(cmd, **kw):
    calls.append((list(cmd), "torch" in sys.modules, kw.get("env", {}).get("HSA_ENABLE_IPC_MODE_LEGACY")))
    return 7
subprocess.call = fake_call
import bench
sys.argv = ["bench.py", "--gpus", "2", "--steps", "3", "--warmup", "1"]
try:
    bench.main()
    rc = None
except SystemExit as e:
    rc = e.code
print(json.dumps({"rc": rc, "calls": calls, "torch_after": "torch" in sys.modules}))
""" % ROOT
    r = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, check=True)
    import json
    out = json.loads(r.stdout.strip().splitlines()[-1])
    assert out["rc"] == 7, "the child's exit code is the parent's"
    assert len(out["calls"]) == 1
    cmd, torch_loaded, ipc = out["calls"][0]
    assert not torch_loaded and not out["torch_after"], "the launcher parent imported torch"
    assert ipc == "0"
    assert cmd[1:4] == ["-m", "torch.distributed.run", "--nnodes=1"]
    assert cmd[cmd.index("--nproc-per-node") + 1] == "2" and cmd[cmd.index("--master-addr") + 1] == "127.0.0.1"
    assert int(cmd[cmd.index("--master-port") + 1]) > 0
    i = cmd.index(os.path.join(ROOT, "bench.py"))
    assert cmd[i + 1:] == ["--gpus", "2", "--steps", "3", "--warmup", "1"]


def test_bench_dump_outputs_float32_bounded_and_reproducible(tmp_path):
    """bench.py --dump-outputs: loss, logits and the engine's flat buffers as float32 .npy; a buffer above DUMP_MAX_ELEMS becomes
    the same seeded sample on every run, and a dump of the largest model (ResNet152, 58.2 M parameters) stays under 64 MB."""
    import numpy as np
    sys.path.insert(0, ROOT)
    import bench
    bench.torch = torch

    class Model:
        def __init__(self, n):
            self.e = type("Engine", (), {})()
            self.e.flat = torch.arange(n, dtype=torch.float64).float()
            self.e.flat_grad = -self.e.flat

        def _eng(self):
            return self.e

    small, big = 1000, 58172494
    logits = torch.randn(256, 14).to(torch.bfloat16)
    for d, n in (("a", small), ("b", big), ("c", big)):
        bench.dump_outputs(str(tmp_path / d), Model(n), torch.tensor(0.25), logits)
    a = {f[:-4]: np.load(str(tmp_path / "a" / f)) for f in os.listdir(str(tmp_path / "a"))}
    assert sorted(a) == ["grads", "logits", "loss", "params"] and all(v.dtype == np.float32 for v in a.values())
    assert np.array_equal(a["params"], np.arange(small)) and np.array_equal(a["grads"], -np.arange(small))
    assert np.array_equal(a["logits"], logits.float().numpy()) and a["loss"].tolist() == [0.25]
    b, c = ({f: np.load(str(tmp_path / d / f)) for f in os.listdir(str(tmp_path / d))} for d in ("b", "c"))
    assert b["params.npy"].shape == (bench.DUMP_MAX_ELEMS,) and np.all(np.diff(b["params.npy"]) >= 0)
    assert all(np.array_equal(b[f], c[f]) for f in b)
    assert sum(os.path.getsize(str(tmp_path / "b" / f)) for f in b) < 64e6
