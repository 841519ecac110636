"""Micro-benchmark of sharpness-aware minimisation (csrc/optim.hip: cx_sam_norm_items, cx_sam_perturb_items, cx_sam_restore_items;
optim.FusedSAM).

Part 1, the kernels: on the flat fp32 buffers of DenseNet121 and ResNet152 with their real tensor lists (one group, nothing frozen),
next to cx_copy_stream moving the SAME number of bytes in the same run: the yardstick is the measured copy rate of the machine, not
the code under test.  Algorithmic bytes: norm 4 n (SAM: reads g) or 8 n (ASAM: reads g and p); perturb 16 n (reads g, p; writes p,
backup); restore 8 n (reads backup; writes p).  Every call (all its launches) is timed by its own pair of events; median and 10th /
90th percentile of `reps` calls after `warm` warm-up calls; the copy is timed before and after the kernels.

Part 2, the step: a graphed step of DenseNet121 (bf16 storage, 320 x 320, batch 256) under FusedSAM(FusedAdam) against the graphed
plain-Adam step (the parent commit's graph: no changed code runs in it) and the graphed forward/backward alone, alternating, in the
same process.  Expectation to confirm or refute: SAM = 2 x (forward + backward) + one optimiser step + the three kernels at roughly
their byte time.

    python scratch/bench_sam.py [--reps 60] [--warm 10] [--steps 30] [--rounds 3] [--skip_step] [--lib OTHER.so] [--out FILE.txt]"""
import argparse, statistics, sys
import torch
sys.path.insert(0, '.')
from chexpert_amd import ops, optim as O, synth

ap = argparse.ArgumentParser()
ap.add_argument("--reps", type=int, default=60)
ap.add_argument("--warm", type=int, default=10)
ap.add_argument("--steps", type=int, default=30)
ap.add_argument("--rounds", type=int, default=3)
ap.add_argument("--batch", type=int, default=256)
ap.add_argument("--size", type=int, default=320)
ap.add_argument("--models", nargs="+", default=["densenet121", "resnet152"])
ap.add_argument("--skip_step", action="store_true")
ap.add_argument("--out", default=None)
ap.add_argument("--lib", default=None, help="another build of libchexpert_hip.so to time (an A/B of two builds in one session)")
args = ap.parse_args()
if args.lib:
    from chexpert_amd import _lib
    _lib.LIB_PATH = args.lib
dev = torch.device('cuda:0')
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


def timeit(fn, reps=None, warm=None):
    for _ in range(args.warm if warm is None else warm):
        fn()
    torch.cuda.synchronize()
    ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(reps or args.reps)]
    for a, b in ev:
        a.record()
        fn()
        b.record()
    torch.cuda.synchronize()
    us = sorted(a.elapsed_time(b) * 1e3 for a, b in ev)
    return {"median": statistics.median(us), "p10": us[len(us) // 10], "p90": us[len(us) * 9 // 10]}


def fmt(t):
    return "%8.1f [%7.1f %7.1f]" % (t["median"], t["p10"], t["p90"])


# ---------------------------------------------------------------------------------------------------------------- part 1
for name in args.models:
    sizes = tensor_list(name)
    n = sum((s + 3) // 4 * 4 for s in sizes)
    table = O.item_table(sizes, [0] * len(sizes))
    items_host = torch.tensor(table, dtype=torch.int32).reshape(-1, 4)
    items = items_host.to(dev)
    say("== %s: %d tensors, %d items, flat n = %d floats (%.1f MB); times in us: median [p10 p90]" % (name, len(sizes), len(table), n, 4 * n / 1e6))
    p, g = torch.randn(n, device=dev) * 0.05, torch.randn(n, device=dev) * 1e-3
    backup, src, dst = torch.zeros(n, device=dev), torch.randn(2 * n, device=dev), torch.zeros(2 * n, device=dev)
    gtab = torch.tensor([[1.0, 0.0, 0.0, 0.0]], dtype=torch.float32, device=dev)
    rho_eps = torch.tensor([0.05, 1e-12], dtype=torch.float32, device=dev)
    part, sam = torch.zeros(len(table), device=dev), torch.zeros(4, device=dev)

    def copy(floats_moved):
        h = floats_moved // 2 // 4 * 4                     # a copy of h floats moves 2 h: reads h, writes h (whole 16-byte units)
        return lambda: ops.copy_stream(src[:h], dst[:h])

    def perturb(adaptive):
        return lambda: ops.sam_perturb_items(p, g, backup, items, gtab, sam, 1.0, adaptive, items_host)

    ops.sam_norm_items(p, g, items, gtab, rho_eps, part, sam, 1.0, False, items_host)
    kernels = [
        ("norm sam", 1, lambda: ops.sam_norm_items(p, g, items, gtab, rho_eps, part, sam, 1.0, False, items_host)),
        ("norm asam", 2, lambda: ops.sam_norm_items(p, g, items, gtab, rho_eps, part, sam, 1.0, True, items_host)),
        ("perturb sam", 4, perturb(False)),
        ("perturb asam", 4, perturb(True)),
        ("restore", 2, lambda: ops.sam_restore_items(p, backup, items, gtab, sam, items_host)),
    ]
    yard = {}
    for floats in (1, 2, 4):
        yard[floats] = timeit(copy(floats * n))
        say("copy_stream  %2d n bytes %s  (%4.2f TB/s)" % (4 * floats, fmt(yard[floats]), 4 * floats * n / yard[floats]["median"] / 1e6))
    for tag, floats, fn in kernels:
        if tag.startswith("perturb"):                      # perturb alone would walk p away: each timed call starts from the restored weights
            # (the restore between two calls is not timed)
            rest = kernels[-1][2]
            for _ in range(args.warm):
                fn(); rest()
            torch.cuda.synchronize()
            ev = []
            for _ in range(args.reps):
                a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                a.record(); fn(); b.record(); rest()
                ev.append((a, b))
            torch.cuda.synchronize()
            us = sorted(a.elapsed_time(b) * 1e3 for a, b in ev)
            t = {"median": statistics.median(us), "p10": us[len(us) // 10], "p90": us[len(us) * 9 // 10]}
        else:
            t = timeit(fn)
        say("%-12s %2d n bytes %s  (%4.2f TB/s of algorithmic traffic; copy_stream of the same bytes %6.1f us: x%4.2f)"
            % (tag, 4 * floats, fmt(t), 4 * floats * n / t["median"] / 1e6, yard[floats]["median"], t["median"] / yard[floats]["median"]))
    for floats in (1, 2, 4):
        t = timeit(copy(floats * n))
        say("copy_stream2 %2d n bytes %s  (%4.2f TB/s)" % (4 * floats, fmt(t), 4 * floats * n / t["median"] / 1e6))
    assert bool(torch.isfinite(p).all()) and float(sam.cpu()[2]) == 0.0
    del p, g, backup, src, dst

# ---------------------------------------------------------------------------------------------------------------- part 2
if not args.skip_step:
    from chexpert_amd.graph import GraphedTrainStep
    from chexpert_amd.models import densenet121
    x = synth.xray_batch(1000, args.batch, args.size).to(dev)
    t = synth.targets(2000, args.batch, 5).to(dev)

    def graphed(kind):
        torch.manual_seed(1)
        m = densenet121(num_classes=5).storage_dtype(torch.bfloat16).to(dev).train()
        opt = None if kind == "fwd_bwd" else O.FusedAdam(m, lr=1e-4)
        if kind in ("sam", "asam"):
            opt = O.FusedSAM(opt, rho=0.05 if kind == "sam" else 0.5, adaptive=kind == "asam")
        return GraphedTrainStep(m, opt, x, t)

    kinds = ["fwd_bwd", "adam", "sam", "asam"]
    steps = {k: graphed(k) for k in kinds}
    say("== graphed DenseNet121 step, bf16 storage, %d x %d, batch %d; ms per step: median [p10 p90] of %d replays after %d, %d rounds alternating"
        % (args.size, args.size, args.batch, args.steps, 5, args.rounds))
    res = {k: [] for k in kinds}
    for r in range(args.rounds):
        for k in kinds:
            tt = timeit(lambda: steps[k].replay(), reps=args.steps, warm=5)
            res[k].append(tt["median"] / 1e3)
            say("round %d %-8s %8.3f [%7.3f %7.3f] ms" % (r, k, tt["median"] / 1e3, tt["p10"] / 1e3, tt["p90"] / 1e3))
    med = {k: statistics.median(v) for k, v in res.items()}
    fb, adam = med["fwd_bwd"], med["adam"]
    say("medians over the rounds: " + ", ".join("%s %.3f ms" % (k, med[k]) for k in kinds))
    say("optimiser step (adam - fwd_bwd): %.3f ms" % (adam - fb))
    for k in ("sam", "asam"):
        say("%-4s - (2 x fwd_bwd + optimiser step) = %.3f ms for the three kernels and whatever else the second pass costs; %s / adam = x%.3f"
            % (k, med[k] - (2 * fb + (adam - fb)), k, med[k] / adam))
    loss = float(steps["sam"].loss.item())
    assert loss == loss
if args.out:
    open(args.out, "w").write("\n".join(lines) + "\n")
