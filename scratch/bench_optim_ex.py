"""Micro-benchmark of the optimiser launches on the flat fp32 buffers: the plain cx_*_step_dev, cx_grad_norm (two launches) and the
cx_*_step_dev_ex with clip + EMA, at the parameter counts of ResNet152 and DenseNet121, next to cx_copy_stream of the same size.
Every launch is timed by its own pair of events; median and 10th / 90th percentile of `reps` launches after `warm` warm-up launches.

    python scratch/bench_optim_ex.py [--reps 60] [--warm 10] [--out FILE.json]

Algorithmic bytes per element: adam / rmsprop read g, p, two states and write p, two states = 28; sgd_nesterov 20; the norm reads 4;
the EMA adds 8 (one read, one write)."""
import argparse, json, statistics, sys
import torch
sys.path.insert(0, '.')
from chexpert_amd import ops

ap = argparse.ArgumentParser()
ap.add_argument("--reps", type=int, default=60)
ap.add_argument("--warm", type=int, default=10)
ap.add_argument("--out", default=None)
args = ap.parse_args()
dev = torch.device('cuda:0')
SIZES = [("resnet152", 58154053), ("densenet121", 6958981)]
STEP_BYTES = {"adam": 28, "sgd_nesterov": 20, "rmsprop": 28}


def timeit(fn):
    for _ in range(args.warm):
        fn()
    torch.cuda.synchronize()
    ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(args.reps)]
    for a, b in ev:
        a.record()
        fn()
        b.record()
    torch.cuda.synchronize()
    us = sorted(a.elapsed_time(b) * 1e3 for a, b in ev)
    return {"median_us": statistics.median(us), "p10_us": us[len(us) // 10], "p90_us": us[len(us) * 9 // 10], "min_us": us[0]}


rows = []
for name, n in SIZES:
    p, g = torch.randn(n, device=dev) * 0.05, torch.randn(n, device=dev) * 1e-3
    s0, s1, ema = torch.zeros(n, device=dev), torch.zeros(n, device=dev), p.clone()
    hyper = torch.tensor([1e-4, 0, 0, 1.0, 0, 0, 0, 1e-4], dtype=torch.float32, device=dev)
    clip = torch.zeros(4, device=dev)
    ws = torch.zeros(ops.grad_norm_partials(n), device=dev)
    n16 = n // 4 * 4
    copy = timeit(lambda: ops.copy_stream(p[:n16], ema[:n16])) if hasattr(ops, "copy_stream") else None
    ema.copy_(p)
    norm = timeit(lambda: ops.grad_norm(g, ws, clip, 1.0, 1.0, True))
    ex = {"clip": clip, "ema": ema, "ema_decay": 0.999, "ema_warmup": True, "skip_nonfinite": True}
    for kind in ("adam", "sgd_nesterov", "rmsprop"):
        if kind == "adam":
            plain = lambda: ops.adam_step_dev(p, g, s0, s1, hyper, 0.9, 0.999, 1e-8, 0.0)
            exf = lambda: ops.adam_step_dev_ex(p, g, s0, s1, hyper, 0.9, 0.999, 1e-8, 0.0, **ex)
        elif kind == "sgd_nesterov":
            plain = lambda: ops.sgd_nesterov_step_dev(p, g, s0, hyper, 0.9, 0.0)
            exf = lambda: ops.sgd_nesterov_step_dev_ex(p, g, s0, hyper, 0.9, 0.0, **ex)
        else:
            plain = lambda: ops.rmsprop_step_dev(p, g, s0, s1, hyper, 0.99, 1e-3, 0.9, 0.0)
            exf = lambda: ops.rmsprop_step_dev_ex(p, g, s0, s1, hyper, 0.99, 1e-3, 0.9, 0.0, **ex)

        def both():
            ops.grad_norm(g, ws, clip, 1.0, 1.0, True)
            exf()
        r = {"model": name, "n": n, "kind": kind, "plain": timeit(plain), "norm": norm, "ex": timeit(exf), "norm_plus_ex": timeit(both),
             "copy_stream": copy, "bytes_plain": STEP_BYTES[kind] * n, "bytes_norm": 4 * n, "bytes_ex": (STEP_BYTES[kind] + 8) * n}
        tb = lambda b, t: b / t["median_us"] / 1e6
        r["tbps"] = {"plain": tb(r["bytes_plain"], r["plain"]), "norm": tb(r["bytes_norm"], norm), "ex": tb(r["bytes_ex"], r["ex"]),
                     "copy_stream": tb(8 * n16, copy) if copy else None}
        rows.append(r)
        print("%-11s n=%9d %-12s plain %7.1f us (%4.2f TB/s) | norm %6.1f us (%4.2f TB/s) | ex %7.1f us (%4.2f TB/s) | norm+ex %7.1f us "
              "[p10 %.1f p90 %.1f] | copy %s" % (name, n, kind, r["plain"]["median_us"], r["tbps"]["plain"], norm["median_us"], r["tbps"]["norm"],
                                                 r["ex"]["median_us"], r["tbps"]["ex"], r["norm_plus_ex"]["median_us"], r["norm_plus_ex"]["p10_us"],
                                                 r["norm_plus_ex"]["p90_us"], "%.1f us (%.2f TB/s)" % (copy["median_us"], r["tbps"]["copy_stream"]) if copy else "-"),
              flush=True)
    del p, g, s0, s1, ema
if args.out:
    json.dump(rows, open(args.out, "w"), indent=1)
