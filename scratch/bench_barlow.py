"""Cost of the Barlow Twins loss: (a) the four launches of cx_barlow_fwd_bwd alone at (N, d) = (512, 128),
(512, 512) and (512, 1024), loss and gradient, captured CALLS times in one hipGraph so that no host enqueue is in the figure (and
cx_bce_fwd_bwd on the step's logits the same way, for the comparison in (b); warm L2 in both), each beside the time its flop count
(3 products of 2 (N / 2) d^2 flops) would take at the 155 TF of the fp32-input MFMA, and (b) the graphed densenet121 bf16 320x320
step at 512 rows with this loss against the same step in the same process with the cross-entropy at the same head width.  The timing
loop is scratch/bench_ntxent.py's: every graph warmed before any is timed, device events around K replays, the graphs taking turns
round after round so that a drift of the box shows in all alike.

  python scratch/bench_barlow.py [--rows 512] [--dim 512] [--steps 5] [--rounds 5] [--out profiles/barlow_bench.txt]"""
import argparse
import json
import os
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def time_replays(graphs, steps, rounds):
    ms = {k: [] for k in graphs}
    for _ in range(rounds):
        for k, g in graphs.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            torch.cuda.synchronize()
            e0.record()
            for _ in range(steps):
                g.replay()
            e1.record()
            torch.cuda.synchronize()
            ms[k].append(e0.elapsed_time(e1) / steps)
    return {k: {"median": sorted(v)[len(v) // 2], "min": min(v), "max": max(v)} for k, v in ms.items()}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=512)
    ap.add_argument("--size", type=int, default=320)
    ap.add_argument("--dim", type=int, default=512)
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--calls", type=int, default=50)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    from chexpert_amd import ops, synth
    from chexpert_amd.graph import GraphedTrainStep
    from chexpert_amd.models import densenet121
    from chexpert_amd.optim import FusedAdam
    dev = torch.device("cuda:0")
    lines = []

    # (a) the kernels alone
    kernels = {}
    for N, d in ((512, 128), (512, 512), (512, 1024)):
        e = synth.uniform(77 + N, (N, d), -1.0, 1.0).to(dev)
        ids = (torch.arange(N) % (N // 2)).float().reshape(-1, 1).to(dev)
        tau = torch.tensor([0.0051], device=dev)
        loss, dl = torch.empty(1, device=dev), torch.empty(N, d, device=dev)
        scratch = torch.empty(ops.barlow_scratch(N, d), device=dev)
        ops.barlow_fwd_bwd(e, ids, tau, loss, dl, None, scratch)
        torch.cuda.synchronize()
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g):
            for _ in range(args.calls):
                ops.barlow_fwd_bwd(e, ids, tau, loss, dl, None, scratch)
        for _ in range(args.warmup):
            g.replay()
        kernels["N=%d d=%d" % (N, d)] = g
    # the cross-entropy the step is compared with below, on the (rows, dim) logits of that step: one workgroup over rows x dim elements
    xb = synth.uniform(78, (args.rows, args.dim), -4.0, 4.0).to(dev)
    tb = synth.targets(79, args.rows, args.dim).to(dev)
    lb, db = torch.empty(1, device=dev), torch.empty_like(xb)
    ops.bce_fwd_bwd(xb, tb, lb, None, db)
    torch.cuda.synchronize()
    gb = torch.cuda.CUDAGraph()
    with torch.cuda.graph(gb):
        for _ in range(args.calls):
            ops.bce_fwd_bwd(xb, tb, lb, None, db)
    for _ in range(args.warmup):
        gb.replay()
    # half a second of replays first, so that no graph is timed on clocks that are still ramping; then the three take turns
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    while time.perf_counter() - t0 < 0.5:
        for g in (gb, *kernels.values()):
            g.replay()
        torch.cuda.synchronize()
    alone = time_replays(dict({"bce": gb}, **kernels), 4, args.rounds)
    bce = alone.pop("bce")
    lines.append("cx_bce_fwd_bwd    B=%d n=%d   loss + gradient, one launch of one workgroup: median %.1f us  (min %.1f, max %.1f; same loop)"
                 % (args.rows, args.dim, 1e3 * bce["median"] / args.calls, 1e3 * bce["min"] / args.calls, 1e3 * bce["max"] / args.calls))
    print(lines[-1], flush=True)
    for k, v in alone.items():
        N, d = (int(p.split("=")[1]) for p in k.split())
        lines.append("cx_barlow_fwd_bwd %-14s loss + gradient, four launches: median %.1f us  (min %.1f, max %.1f; %d calls per graph, "
                     "4 replays x %d rounds); its %.3f GFLOP at 155 TF: %.1f us"
                     % (k, 1e3 * v["median"] / args.calls, 1e3 * v["min"] / args.calls, 1e3 * v["max"] / args.calls, args.calls, args.rounds,
                        3e-9 * N * d * d, 3.0 * N * d * d / 155e12 * 1e6))
        print(lines[-1], flush=True)
    lines.append("(the calls of a graph follow each other on the same operands: L2 is warm, so inside a step, behind the head's kernels, "
                 "either loss may cost more than its figure here)")

    # (b) the step
    x = synth.xray_batch(1000, args.rows, args.size).to(dev)
    targets = {"bce": synth.targets(2000, args.rows, args.dim).to(dev),
               "barlow": (torch.arange(args.rows) % (args.rows // 2)).float().reshape(-1, 1).to(dev)}
    steps = {}
    for kind in ("bce", "barlow"):
        torch.manual_seed(1234)
        model = densenet121()
        model.classifier = torch.nn.Linear(model.classifier.in_features, args.dim)
        model = model.to(dev).train()
        if kind == "barlow":
            model.set_loss(kind="barlow", lambd=0.0051)
        opt = FusedAdam(model, lr=1e-4)
        model.forward_backward(x, targets[kind])
        opt.step()
        g = GraphedTrainStep(model, opt, x, targets[kind])
        for _ in range(args.warmup):
            g.replay()
        torch.cuda.synchronize()
        steps[kind] = g
        print("captured %s" % kind, flush=True)
    res = time_replays(steps, args.steps, args.rounds)
    for k, v in res.items():
        lines.append("densenet121 bf16 %dx%d, %d rows, head width %d, graph replay, loss %-6s: median %.3f ms / step  (min %.3f, max %.3f; "
                     "%d steps x %d rounds interleaved)" % (args.size, args.size, args.rows, args.dim, k, v["median"], v["min"], v["max"],
                                                            args.steps, args.rounds))
        print(lines[-1], flush=True)
    diff = res["barlow"]["median"] - res["bce"]["median"]
    lines.append("difference of the medians: %+.3f ms (%+.2f %% of the step)" % (diff, 100 * diff / res["bce"]["median"]))
    print(lines[-1], flush=True)
    print(json.dumps({"kernels_and_steps": lines}), flush=True)
    if args.out:
        os.makedirs(os.path.dirname(args.out) or ".", exist_ok=True)
        open(args.out, "w").write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
