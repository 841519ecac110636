"""CPU (no GPU): the host side of the class-specific maps (chexpert_amd.gradcam.class_cam): the two C entry points' declaration,
argument validation before any launch, the family table and the figure writer."""
import os
import re

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _models():
    from chexpert_amd.models import BasicBlock, Bottleneck, DenseNet, ResNet, WideResNet, construct_model
    return {"densenet": DenseNet(32, (2, 2, 2, 2), 64, num_classes=5),
            "resnet": ResNet(Bottleneck, [1, 1, 1, 1], num_classes=5),
            "wideresnet": WideResNet(BasicBlock, 10, 4, num_classes=5),
            "efficientnet": construct_model("efficientnet-b0", 5)}


def test_class_cam_symbols_match_the_header():
    from chexpert_amd import _lib
    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "chexpert_hip.h")).read(), flags=re.S)
    for name in ("cx_class_cam", "cx_class_cam_f32"):
        m = re.search(r"\bint\s+%s\s*\(([^;{]*?)\)\s*;" % name, hdr, flags=re.S)
        assert m, "%s is not declared in include/chexpert_hip.h" % name
        assert len(_lib.SIGNATURES[name]) == m.group(1).count(",") + 1 == 16
    assert _lib.lib().cx_abi_version() == 10                           # additive entry points


def test_entry_point_validates_without_launching():
    """Out-of-range arguments give the "unsupported shape" code before anything is launched (no GPU here: a launch would fail with
    a positive HIP error instead)."""
    from chexpert_amd import _lib
    x, w, cam = torch.zeros(4096), torch.zeros(4096), torch.zeros(4096)
    X, W, CAM = x.data_ptr(), w.data_ptr(), cam.data_ptr()
    for f in (_lib.lib().cx_class_cam, _lib.lib().cx_class_cam_f32):
        ok = dict(B=1, HW=4, C=16, ldx=16, n=5, ldw=16, K=5)

        def call(x_=X, w_=W, cam_=CAM, cls=None, act=0, **kw):
            a = dict(ok, **kw)
            return f(x_, None, None, w_, cls, cam_, a["B"], a["HW"], a["C"], a["ldx"], a["n"], a["ldw"], a["K"], act, 1, None)
        assert call(x_=None) == call(w_=None) == call(cam_=None) == -3
        assert call(K=0) == -3 and call(K=4) == -3                 # without a class table K is n_classes
        assert call(C=12, ldx=16) == -3 and call(ldx=20) == -3 and call(ldx=8) == -3 and call(ldw=8) == -3
        assert call(C=4104, ldx=4104, ldw=4104) == -3              # more than 64 values per lane
        assert call(act=3) == -1
    assert _lib.lib().cx_error_string(-3) == b"unsupported shape"


def test_cam_source_family_table():
    from chexpert_amd import gradcam, ops
    m = _models()
    assert gradcam.cam_source(m["densenet"]) == (ops.CAM_ACT_RELU, m["densenet"].classifier)
    assert gradcam.cam_source(m["resnet"]) == (ops.CAM_ACT_NONE, m["resnet"].fc)
    assert gradcam.cam_source(m["efficientnet"]) == (ops.CAM_ACT_SWISH, m["efficientnet"].head[-1])
    assert gradcam.cam_source(m["wideresnet"]) == (ops.CAM_ACT_NONE, m["wideresnet"].fc)
    assert (ops.CAM_ACT_NONE, ops.CAM_ACT_RELU, ops.CAM_ACT_SWISH) == (0, 1, 2)      # CX_CAM_ACT_* of the header
    with pytest.raises(RuntimeError):
        gradcam.cam_source(torch.nn.Linear(2, 2))


def test_class_cam_rejects_cpu_input_and_bad_class_lists(monkeypatch):
    from chexpert_amd import _lib, gradcam
    model = _models()["densenet"]
    x = torch.zeros(2, 3, 64, 64)
    with pytest.raises(RuntimeError, match="class_cam runs on the GPU only"):
        gradcam.class_cam(model, x)
    with pytest.raises(RuntimeError, match="grad_cam runs on the GPU only"):      # the wording it shares
        gradcam.grad_cam(model, x)

    def no_library():
        raise AssertionError("the library was called")
    monkeypatch.setattr(_lib, "lib", no_library)
    from chexpert_amd import ops
    monkeypatch.setattr(ops, "lib", no_library)
    for bad in ([], [5], [-1], [0, 7], (), [1.0], "top", torch.tensor([0, 5]), torch.tensor([-1, 0]), torch.tensor([0.0, 1.0]),
                torch.zeros(2, 2, dtype=torch.int64)):
        with pytest.raises(ValueError):
            gradcam.class_cam(model, x, bad)
    with pytest.raises(ValueError):
        gradcam.class_cam(model, x, normalize=False, upsample=True)
    assert model.training                                             # nothing ran, nothing was switched


def test_cli_flag_parsing():
    from chexpert_amd import cli
    p = cli.build_parser()
    assert p.parse_args(["--visualize"]).cam_classes is None
    assert cli.resolve_cam_classes(None, 5) is None
    assert cli.resolve_cam_classes(p.parse_args(["--visualize", "--cam_classes"]).cam_classes, 5) == [0, 1, 2, 3, 4]
    assert cli.resolve_cam_classes(p.parse_args(["--visualize", "--cam_classes", "all"]).cam_classes, 14) == list(range(14))
    assert cli.resolve_cam_classes(p.parse_args(["--cam_classes", "0", "2", "--visualize"]).cam_classes, 5) == [0, 2]
    for bad in (["5"], ["-1"], ["x"], ["all", "1"]):
        with pytest.raises(ValueError):
            cli.resolve_cam_classes(bad, 5)
    with pytest.raises(ValueError, match="--visualize"):
        cli.main(["--cam_classes", "0", "--synthetic", "4", "--output_dir", "unused"])


def test_visualize_classes_writes_one_figure_per_image(tmp_path):
    from chexpert_amd import vis
    rng = np.random.RandomState(0)
    N, K = 3, 2
    files = vis.visualize_classes(rng.rand(N, 64, 64), (rng.rand(N, 5) < 0.3).astype(np.float32), rng.randn(N, 5), rng.rand(N, K, 2, 2),
                                  ["synthetic/%d" % i for i in (4, 7, 9)], ["a", "b", "c", "d", "e"], [3, 0], str(tmp_path), 12)
    names = sorted(os.listdir(os.path.join(str(tmp_path), "vis")))
    assert names == ["classcam_synthetic_%d_step_12.png" % i for i in (4, 7, 9)]
    assert sorted(os.path.basename(f) for f in files) == names and not any(n.startswith("vis_") for n in names)
    assert all(os.path.getsize(f) > 0 for f in files)
    with pytest.raises(AssertionError):
        vis.visualize_classes(rng.rand(1, 8, 8), np.zeros((1, 5)), np.zeros((1, 5)), rng.rand(1, 3, 2, 2), ["i"], list("abcde"), [0, 1],
                              str(tmp_path), 0)
