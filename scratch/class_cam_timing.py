"""Kernel times of cx_class_cam against K launches of cx_gradcam_map on the same buffer: the block-4 buffer of densenet121 at 320 x 320,
B = 24 (the 'vis' subset), norm5 scale / shift, K classes.  Run under `rocprofv3 --kernel-trace --stats -- python
scratch/class_cam_timing.py K`: the stats then hold REPS launches of class_cam_kernel and REPS * K of gradcam_map_kernel; the cost of
the K-launch sequence is K times the latter's mean.  Also prints device-event times of both (launch gaps included) as one JSON line."""
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch

from chexpert_amd import ops, synth
from chexpert_amd.models import densenet121

K = int(sys.argv[1]) if len(sys.argv) > 1 else 5
REPS, B, S = 50, 24, 320
dev = torch.device("cuda:0")
model = densenet121()
model.classifier = torch.nn.Linear(model.classifier.in_features, K)
model = model.to(dev).eval()
eng = model._eng()
with torch.no_grad():
    ws = eng.forward(synth.xray_batch(5, B, S).to(dev), False)
buf, sc, sh = eng.norm5_operands(ws)
Bb, h, w, C = buf.shape
W = model.classifier.weight.detach().contiguous().clone()
cam = torch.empty(B, K, h * w, device=dev)
one = torch.empty(B, h * w, device=dev)
rows = [W[k].contiguous() for k in range(K)]


def new():
    ops.class_cam(buf, sc, sh, W, cam, act=ops.CAM_ACT_RELU, relu=True)


def old():
    for k in range(K):
        ops.gradcam_map(buf, sc, sh, rows[k], one, 1)


def timed(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(REPS):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) * 1e3 / REPS


for _ in range(5):
    new()
    old()
torch.cuda.synchronize()
# same arithmetic up to the 1/HW factor and the summation order
old()
ops.gradcam_map(buf, sc, sh, rows[K - 1], one, 1)
err = float((cam[:, K - 1] * (h * w) - one).abs().max() / one.abs().max().clamp(min=1e-30))
t = [(timed(new), timed(old)) for _ in range(3)]          # alternating
print(json.dumps({"shape": [Bb, h, w, C], "pitch": buf.stride(2), "K": K, "reps": REPS, "event_us_class_cam": [round(a, 2) for a, _ in t],
                  "event_us_K_gradcam_map": [round(b, 2) for _, b in t], "rel_diff_vs_gradcam_map": err}))
eng.release(ws)
