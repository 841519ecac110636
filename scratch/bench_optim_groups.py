"""Micro-benchmark of the grouped optimiser launches (csrc/optim.hip) on the flat fp32 buffers of DenseNet121 and ResNet152 with
their real tensor lists: cx_grad_norm_items and cx_*_step_items (device form, clip + EMA on) for 1, 3 and 64 groups and a sweep of
the item length, next to the ungrouped cx_*_step_dev, cx_*_step_dev_ex and cx_grad_norm at the same n, measured in the same run
(before and after the grouped launches).  Every launch is timed by its own pair of events; median and 10th / 90th percentile of
`reps` launches after `warm` warm-up launches.

    python scratch/bench_optim_groups.py [--reps 60] [--warm 10] [--vec4 256 512 ...] [--out FILE.txt]

Algorithmic bytes per element: adam / rmsprop read g, p, two states and write p, two states = 28; sgd_nesterov 20; the EMA adds 8;
the norm reads 4.  The grouped passes add 16 bytes per item (and launch 2 of the norm one partial + one group index per item)."""
import argparse, statistics, sys
import torch
sys.path.insert(0, '.')
from chexpert_amd import ops, optim as O

ap = argparse.ArgumentParser()
ap.add_argument("--reps", type=int, default=60)
ap.add_argument("--warm", type=int, default=10)
ap.add_argument("--vec4", type=int, nargs="+", default=[1024, 2048, 4096, 8192])
ap.add_argument("--groups", type=int, nargs="+", default=[1, 3, 64])
ap.add_argument("--models", nargs="+", default=["densenet121", "resnet152"])
ap.add_argument("--out", default=None)
args = ap.parse_args()
dev = torch.device('cuda:0')
STEP_BYTES = {"adam": 28, "sgd_nesterov": 20, "rmsprop": 28}
lines = []


def say(s):
    print(s, flush=True)
    lines.append(s)


def tensor_list(name):
    """Parameter sizes of the model as the command line builds it (5 classes), in the engine's order."""
    from chexpert_amd import models
    m = getattr(models, name)()
    head = "classifier" if hasattr(m, "classifier") else "fc"
    setattr(m, head, torch.nn.Linear(getattr(m, head).in_features, 5))
    return [p.numel() for p in m.parameters()]


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
    return {"median": statistics.median(us), "p10": us[len(us) // 10], "p90": us[len(us) * 9 // 10]}


def fmt(t):
    return "%7.1f [%6.1f %6.1f]" % (t["median"], t["p10"], t["p90"])


for name in args.models:
    sizes = tensor_list(name)
    n = sum((s + 3) // 4 * 4 for s in sizes)
    small = sum(1 for s in sizes if s <= 4096)
    say("== %s: %d tensors (%d of at most 4096 floats), flat n = %d floats; times in us: median [p10 p90]" % (name, len(sizes), small, n))
    p, g = torch.randn(n, device=dev) * 0.05, torch.randn(n, device=dev) * 1e-3
    s0, s1, ema = torch.zeros(n, device=dev), torch.zeros(n, device=dev), p.clone()
    # steps_done = 1: on the very first step the ungrouped SGD kernels do not read the momentum buffer (4 bytes per element less)
    hyper = torch.tensor([1e-4, 1, 0, 1.0, 0, 0, 0, 1e-4], dtype=torch.float32, device=dev)
    clip = torch.zeros(4, device=dev)
    ws = torch.zeros(ops.grad_norm_partials(n), device=dev)
    ex = {"clip": clip, "ema": ema, "ema_decay": 0.999, "ema_warmup": True, "skip_nonfinite": True}

    def parent(kind, which):
        tail = ex if which == "ex" else {}
        sfx = "_dev_ex" if which == "ex" else "_dev"
        if kind == "adam":
            return lambda: getattr(ops, "adam_step" + sfx)(p, g, s0, s1, hyper, 0.9, 0.999, 1e-8, 0.0, **tail)
        if kind == "sgd_nesterov":
            return lambda: getattr(ops, "sgd_nesterov_step" + sfx)(p, g, s0, hyper, 0.9, 0.0, **tail)
        return lambda: getattr(ops, "rmsprop_step" + sfx)(p, g, s0, s1, hyper, 0.99, 1e-3, 0.9, 0.0, **tail)

    def grouped(kind, items, gtab):
        if kind == "adam":
            return lambda: ops.adam_step_items(p, g, s0, s1, items, gtab, False, 0.9, 0.999, 1e-8, hyper=hyper, **ex)
        if kind == "sgd_nesterov":
            return lambda: ops.sgd_nesterov_step_items(p, g, s0, items, gtab, False, 0.9, hyper=hyper, **ex)
        return lambda: ops.rmsprop_step_items(p, g, s0, s1, items, gtab, False, 0.99, 1e-3, 0.9, hyper=hyper, **ex)

    def parents(tag):
        out = {"norm": timeit(lambda: ops.grad_norm(g, ws, clip, 1.0, 1.0, True))}
        say("%-8s %-12s cx_grad_norm          %s  (%4.2f TB/s)" % (tag, "", fmt(out["norm"]), 4 * n / out["norm"]["median"] / 1e6))
        for kind in STEP_BYTES:
            out[kind, "dev"], out[kind, "ex"] = timeit(parent(kind, "dev")), timeit(parent(kind, "ex"))
            say("%-8s %-12s _dev %s  (%4.2f TB/s) | _dev_ex %s  (%4.2f TB/s)"
                % (tag, kind, fmt(out[kind, "dev"]), STEP_BYTES[kind] * n / out[kind, "dev"]["median"] / 1e6, fmt(out[kind, "ex"]),
                   (STEP_BYTES[kind] + 8) * n / out[kind, "ex"]["median"] / 1e6))
        return out

    base = parents("parent")
    for G in args.groups:
        group_of = [k % G for k in range(len(sizes))]
        gtab = torch.tensor([[1.0, 0.0, 0.0, 0.0]] * G, dtype=torch.float32, device=dev)
        gsq, gnorm = torch.zeros(G, device=dev), torch.zeros(G, device=dev)
        for V in args.vec4:
            if V > ops.optim_item_vec4():
                continue                                    # the step kernels cut an item into slots of the library's constant
            table = O.item_table(sizes, group_of, vec4=V)
            assert 4 * (table[-1][0] + table[-1][1]) == n
            items = torch.tensor(table, dtype=torch.int32).to(dev)
            part = torch.zeros(len(table), device=dev)
            tn = timeit(lambda: ops.grad_norm_items(g, items, gtab, part, gsq, gnorm, clip, 1.0, 1.0, True))
            row = "G=%-3d V=%-5d items=%-6d norm %s x%4.2f" % (G, V, len(table), fmt(tn), tn["median"] / base["norm"]["median"])
            for kind in STEP_BYTES:
                t = timeit(grouped(kind, items, gtab))
                b = base[kind, "ex"]
                row += " | %s %s x%4.2f%s" % (kind[:4], fmt(t), t["median"] / b["median"], " in" if b["p10"] <= t["median"] <= b["p90"] else "")
            say(row)
    parents("parent2")
    del p, g, s0, s1, ema
if args.out:
    open(args.out, "w").write("\n".join(lines) + "\n")
