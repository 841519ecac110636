"""Times of the threshold sweep of the bootstrap at (N, C, B) = (234, 5, 1000) and (20 000, 14, 2000), by the method of
scratch/bootstrap_timing.py (device events around REPS back-to-back launches after a warm-up, launch gaps included): cx_boot_sweep with
0, 2 and 8 operating points against cx_boot_auc on the same count table, metrics.bootstrap_metrics end to end (host clock, plans and
copies included, ending in the device-to-host copies), and the numpy statement of the kernel on the host
(metrics.bootstrap_sweep_reference over HOST_REPS replicates, scaled to B and marked as such).  The kernel's integers are compared with
the statement's on those replicates at the sizes timed.  Prints one JSON line per shape:
    python scratch/boot_sweep_timing.py [out.json]"""
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch

from chexpert_amd import metrics as M
from chexpert_amd import ops

REPS, HOST_REPS = 20, 32
NAMES = ("auroc", "ap", "sens@0.9", "spec@0.9")
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
    auc_plan = M.bootstrap_plan(s, t)
    t0 = time.perf_counter()
    plan = M.bootstrap_sweep_plan(s, t)
    t_plan = time.perf_counter() - t0
    auc_order, order = torch.from_numpy(auc_plan["order"]).to(dev), torch.from_numpy(plan["order"]).to(dev)
    table = ops.boot_counts(N, B, 1, device=dev)
    _, points = M.parse_boot_metrics(["sens@0.9", "spec@0.9", "sens@0.8", "spec@0.8", "sens@0.95", "spec@0.95", "sens@0.5", "spec@0.5"])
    us_auc = events(lambda: ops.boot_auc(table, auc_order, auc_plan["offs"], auc_plan["lens"], N))
    us = {p: events(lambda: ops.boot_sweep(table, order, plan["offs"], plan["lens"], N, points[:p])) for p in (0, 2, 8)}
    us_auc2 = events(lambda: ops.boot_auc(table, auc_order, auc_plan["offs"], auc_plan["lens"], N))      # again: the spread of the yardstick
    counts = table[:HOST_REPS].cpu().numpy().view(np.uint32)
    t0 = time.perf_counter()
    want = M.bootstrap_sweep_reference(counts, plan["order"], plan["offs"], plan["lens"], N, points)
    t_ref = (time.perf_counter() - t0) * B / HOST_REPS
    got = ops.boot_sweep(table[:HOST_REPS], order, plan["offs"], plan["lens"], N, points)
    same = all(np.array_equal(g.cpu().numpy(), w.view(np.int64)) for g, w in zip(got, want))
    M.bootstrap_metrics(s, t, NAMES, n_boot=B, seed=1, device=dev)    # warm
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    M.bootstrap_metrics(s, t, NAMES, n_boot=B, seed=1, device=dev)
    t_gpu = time.perf_counter() - t0
    entries = int(plan["lens"].sum()) * B
    return {"N": N, "C": C, "B": B, "cx_boot_auc_us": round(us_auc, 1), "cx_boot_auc_again_us": round(us_auc2, 1),
            "cx_boot_sweep_0_points_us": round(us[0], 1), "cx_boot_sweep_2_points_us": round(us[2], 1),
            "cx_boot_sweep_8_points_us": round(us[8], 1), "sweep_2_points_over_auc": round(us[2] / us_auc, 2),
            "sweep_0_points_over_auc": round(us[0] / us_auc, 2), "sweep_8_points_over_auc": round(us[8] / us_auc, 2),
            "entries_per_us_2_points": round(entries / us[2], 1), "host_plan_ms": round(t_plan * 1e3, 2),
            "bootstrap_metrics_%s_end_to_end_ms" % "_".join(NAMES): round(t_gpu * 1e3, 2),
            "host_statement_8_points_ms_scaled_from_%d_replicates" % HOST_REPS: round(t_ref * 1e3, 1), "bit_equal_to_statement": same}


lines = [shape(234, 5, 1000), shape(20000, 14, 2000)]
for l in lines:
    print(json.dumps(l), flush=True)
if len(sys.argv) > 1:
    json.dump(lines, open(sys.argv[1], "w"), indent=1)
