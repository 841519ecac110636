"""Times of the AUROC bootstrap at (N, C, B) = (234, 5, 1000) and (20 000, 14, 2000): cx_boot_counts and cx_boot_auc separately (device
events around REPS back-to-back launches after a warm-up, launch gaps included), metrics.bootstrap_auc end to end (host clock, plan and
copies included, ending in the device-to-host copies), and the same work on the host through metrics.bootstrap_auc_reference (the
numpy statement, vectorised over replicates) and through the route of metrics.compute_metrics (one roc_curve + auc per replicate and
class on the np.repeat-materialised resample: timed on HOST_REPS replicates and scaled, marked as such).  The results of the GPU and
of the reference are compared bit for bit at the sizes timed.  Prints one JSON line per shape:
    python scratch/bootstrap_timing.py [out.json]"""
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch

from chexpert_amd import metrics as M
from chexpert_amd import ops

REPS, HOST_REPS = 20, 20
dev = torch.device("cuda:0")


def events(fn):
    for _ in range(3):
        fn()
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(REPS):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) * 1e3 / REPS                            # microseconds per call


def shape(N, C, B):
    rng = np.random.default_rng(N)
    t = (rng.random((N, C)) < 0.3).astype(np.float32)
    s = (rng.normal(size=(N, C)) + t).astype(np.float32)
    t[rng.random((N, C)) < 0.05] = -1.0
    t0 = time.perf_counter()
    plan = M.bootstrap_plan(s, t)
    t_plan = time.perf_counter() - t0
    order = torch.from_numpy(plan["order"]).to(dev)
    table = torch.empty(B, N, dtype=torch.int32, device=dev)
    us_counts = events(lambda: ops.boot_counts(N, B, 1, out=table))
    us_auc = events(lambda: ops.boot_auc(table, order, plan["offs"], plan["lens"], N))
    M.bootstrap_auc(s, t, n_boot=B, seed=1, device=dev)               # warm
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    got = M.bootstrap_auc(s, t, n_boot=B, seed=1, device=dev, return_replicates=True)
    t_gpu = time.perf_counter() - t0
    t0 = time.perf_counter()
    ref = M.bootstrap_auc_reference(s, t, n_boot=B, seed=1, return_replicates=True)
    t_ref = time.perf_counter() - t0
    same = bool(np.array_equal(got["replicates"], ref["replicates"], equal_nan=True)) and got["lo"] == ref["lo"] and got["hi"] == ref["hi"]
    counts = M.bootstrap_counts_reference(N, HOST_REPS, 1)
    t0 = time.perf_counter()
    for r in range(HOST_REPS):
        for c in range(C):
            keep = t[:, c] >= 0
            w = counts[r][keep]
            M.auc(*M.roc_curve(np.repeat(t[keep, c], w), np.repeat(s[keep, c], w))[:2])
    t_roc = (time.perf_counter() - t0) * B / HOST_REPS
    entries = 2 * int(plan["lens"].sum()) * B
    return {"N": N, "C": C, "B": B, "cx_boot_counts_us": round(us_counts, 1), "cx_boot_auc_us": round(us_auc, 1),
            "draws_per_us": round(N * B / us_counts, 1), "order_entries_per_us": round(entries / us_auc, 1),
            "host_plan_ms": round(t_plan * 1e3, 2), "bootstrap_auc_end_to_end_ms": round(t_gpu * 1e3, 2),
            "host_reference_ms": round(t_ref * 1e3, 1), "host_roc_curve_route_ms_scaled_from_%d_replicates" % HOST_REPS: round(t_roc * 1e3, 1),
            "bit_equal_to_reference": same}


lines = [shape(234, 5, 1000), shape(20000, 14, 2000)]
for l in lines:
    print(json.dumps(l), flush=True)
if len(sys.argv) > 1:
    json.dump(lines, open(sys.argv[1], "w"), indent=1)
