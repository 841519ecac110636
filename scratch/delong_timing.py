"""Times of the DeLong / Obuchowski AUROC test at (N, C, models) = (234, 5, 2), (200 000, 14, 2) with image units and (200 000, 14, 2) with
about 65 000 patient units: cx_delong_place and cx_delong_gram separately (device events around REPS back-to-back calls after a warm-up,
launch gaps included), metrics.delong_auc_diff end to end (host clock, both plans and all copies included, ending in the exact host
finish), and the same call's numpy statement on the host, metrics.delong_auc_diff_reference.  The two results are compared float for
float at the sizes timed.  Prints one JSON line per shape:
    python scratch/delong_timing.py [out.json]"""
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch

from chexpert_amd import metrics as M
from chexpert_amd import ops

REPS = 20
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


def shape(N, C, n_groups=None):
    rng = np.random.default_rng(N)
    t = (rng.random((N, C)) < 0.3).astype(np.float32)
    sa = (rng.normal(size=(N, C)) + t).astype(np.float32)
    sb = (rng.normal(size=(N, C)) + 0.8 * t).astype(np.float32)
    t[rng.random((N, C)) < 0.05] = -1.0
    groups = None if n_groups is None else rng.integers(0, n_groups, size=N)
    t0 = time.perf_counter()
    plans = [M.bootstrap_plan(s, t, groups) for s in (sa, sb)]
    t_plan = time.perf_counter() - t0
    U = plans[0]["n_units"]
    order = torch.from_numpy(plans[0]["order"]).to(dev)
    table = torch.empty(8 * C, U, dtype=torch.int64, device=dev)
    us_place = events(lambda: ops.delong_place(order, plans[0]["offs"], plans[0]["lens"], U, out=table[:4 * C]))
    ops.delong_place(torch.from_numpy(plans[1]["order"]).to(dev), plans[1]["offs"], plans[1]["lens"], U, out=table[4 * C:])
    us_gram = events(lambda: ops.int_gram(table, U))
    M.delong_auc_diff(sa, sb, t, groups=groups, device=dev)           # warm
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    got = M.delong_auc_diff(sa, sb, t, groups=groups, device=dev)
    t_gpu = time.perf_counter() - t0
    t0 = time.perf_counter()
    ref = M.delong_auc_diff_reference(sa, sb, t, groups=groups)
    t_ref = time.perf_counter() - t0
    t0 = time.perf_counter()
    M.int_gram_reference(table.cpu().numpy())
    t_ref_gram = time.perf_counter() - t0
    entries = 2 * int(plans[0]["lens"].sum())
    return {"N": N, "C": C, "models": 2, "n_units": U, "cx_delong_place_us_one_model": round(us_place, 1), "cx_delong_gram_us": round(us_gram, 1),
            "order_entries_per_us": round(entries / us_place, 1), "gram_mac_per_us": round(8 * C * (8 * C + 4) / 2 * U / us_gram, 1),
            "host_plans_ms": round(t_plan * 1e3, 2), "delong_auc_diff_end_to_end_ms": round(t_gpu * 1e3, 2),
            "host_reference_ms": round(t_ref * 1e3, 1), "host_reference_gram_alone_ms": round(t_ref_gram * 1e3, 1),
            "equal_to_reference": json.dumps(got, sort_keys=True) == json.dumps(ref, sort_keys=True)}


lines = [shape(234, 5), shape(200000, 14), shape(200000, 14, 65000)]
for l in lines:
    print(json.dumps(l), flush=True)
if len(sys.argv) > 1:
    json.dump(lines, open(sys.argv[1], "w"), indent=1)
