"""Micro-benchmark of the trust-ratio steps (csrc/optim.hip: cx_lamb_step_items, cx_lars_step_items, three launches each) on the flat
fp32 buffers of DenseNet121 and ResNet152 with their real tensor lists, next to the grouped steps they stand on (cx_adam_step_items,
cx_sgd_nesterov_step_items: the kernels of the parent commit, unchanged) on the same item table, measured in the same run, before and
after.  Device form (`hyper`), three groups round-robin with weight decay (every tensor adapted); "plain": no clip, no EMA; "ex":
clip + EMA + skip_nonfinite.  Every call (all its launches) is timed by its own pair of events; median and 10th / 90th percentile of
`reps` calls after `warm` warm-up calls.

    python scratch/bench_optim_trust.py [--reps 60] [--warm 10] [--out FILE.txt]

Algorithmic floats per element: adam_items 7 (reads g, p, m, v; writes p, m, v), lamb 7 in the first launch (reads g, p, m, v; writes
m, v, u) + 3 in the apply (reads p, u; writes p) = 10; sgd_items 5, lars 2 more (the read of g and p for the norms) = 7; the EMA adds 2
to each.  On top: the second launch, one workgroup that adds two partials per item."""
import argparse, statistics, sys
import torch
sys.path.insert(0, '.')
from chexpert_amd import ops, optim as O

ap = argparse.ArgumentParser()
ap.add_argument("--reps", type=int, default=60)
ap.add_argument("--warm", type=int, default=10)
ap.add_argument("--models", nargs="+", default=["densenet121", "resnet152"])
ap.add_argument("--out", default=None)
args = ap.parse_args()
dev = torch.device('cuda:0')
FLOATS = {"adam": 7, "lamb": 10, "sgd": 5, "lars": 7}
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
    G = 3
    group_of = [k % G for k in range(len(sizes))]
    table = O.item_table(sizes, group_of)
    items = torch.tensor(table, dtype=torch.int32).to(dev)
    titems = torch.tensor(O.tensor_items(table, len(sizes)), dtype=torch.int32).to(dev)
    say("== %s: %d tensors, %d items, flat n = %d floats; times in us: median [p10 p90]" % (name, len(sizes), len(table), n))
    # small values, a tiny rate and a weight decay: thousands of timed steps leave every buffer finite
    p, g = torch.randn(n, device=dev) * 0.05, torch.randn(n, device=dev) * 1e-3
    s0, s1, u, ema = torch.zeros(n, device=dev), torch.zeros(n, device=dev), torch.zeros(n, device=dev), p.clone()
    gtab = torch.tensor([[1.0, 1e-4, 0.0, 0.0]] * G, dtype=torch.float32, device=dev)
    hyper = torch.tensor([1e-6, 1, 0, 1.0, 0, 0, 0, 1e-6], dtype=torch.float32, device=dev)
    clip = torch.tensor([1.0, 1.0, 0.0, 0.0], device=dev)
    parts = (torch.zeros(len(table), device=dev), torch.zeros(len(table), device=dev))
    trust = torch.zeros(len(sizes), 4, device=dev)
    tails = {"plain": {}, "ex": {"clip": clip, "ema": ema, "ema_decay": 0.999, "ema_warmup": True, "skip_nonfinite": True}}

    def call(kind, tail):
        if kind == "adam":
            return lambda: ops.adam_step_items(p, g, s0, s1, items, gtab, False, 0.9, 0.999, 1e-8, hyper=hyper, **tail)
        if kind == "lamb":
            return lambda: ops.lamb_step_items(p, g, s0, s1, items, gtab, False, 0.9, 0.999, 1e-6, titems, parts, trust, u, hyper=hyper, **tail)
        if kind == "sgd":
            return lambda: ops.sgd_nesterov_step_items(p, g, s0, items, gtab, False, 0.9, hyper=hyper, **tail)
        return lambda: ops.lars_step_items(p, g, s0, items, gtab, False, 0.9, titems, parts, trust, 0.001, 1e-8, hyper=hyper, **tail)

    for which, tail in tails.items():
        extra = 2 if which == "ex" else 0
        t = {}
        for kind in ("adam", "lamb", "sgd", "lars", "adam", "sgd"):              # the parents once more after the new steps
            tag = kind + ("2" if kind in t else "")
            t[tag] = timeit(call(kind, tail))
            say("%-6s %-6s %s  (%4.2f TB/s of algorithmic traffic)" % (which, tag, fmt(t[tag]), 4 * (FLOATS[kind] + extra) * n / t[tag]["median"] / 1e6))
        for new, old in (("lamb", "adam"), ("lars", "sgd")):
            say("%-6s %s / %s_items: x%4.2f measured, x%4.2f by bytes; + %5.1f us" % (
                which, new, old, t[new]["median"] / t[old]["median"], (FLOATS[new] + extra) / (FLOATS[old] + extra),
                t[new]["median"] - t[old]["median"]))
    assert bool(torch.isfinite(p).all()) and bool(torch.isfinite(trust).all())
    del p, g, s0, s1, u, ema
if args.out:
    open(args.out, "w").write("\n".join(lines) + "\n")
