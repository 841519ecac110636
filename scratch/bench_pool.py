"""Step time of densenet121 (bs = 256, 320x320, bf16) for every pooling of FusedNet.set_pool, beside the average on the same build
(DESIGN.md section 4.43).  The timing loop is bench.py's: the step (zero_grad, forward, loss, backward, FusedAdam) captured once as a
hipGraph and replayed, device events around K replays.  The four models live side by side and take turns, round after round, so that
a drift of the box shows in every kind alike.

  python scratch/bench_pool.py [--batch 256] [--steps 20] [--rounds 5] [--out bench_pool.json]"""
import argparse
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=256)
    ap.add_argument("--size", type=int, default=320)
    ap.add_argument("--classes", type=int, default=5)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    from chexpert_amd import synth
    from chexpert_amd.graph import GraphedTrainStep
    from chexpert_amd.models import densenet121
    from chexpert_amd.optim import FusedAdam
    dev = torch.device("cuda:0")
    x = synth.xray_batch(1000, args.batch, args.size).to(dev)
    t = synth.targets(2000, args.batch, args.classes).to(dev)
    steps = {}
    for kind in ("avg", "max", "lse", "gem"):
        torch.manual_seed(1234)
        model = densenet121()
        model.classifier = torch.nn.Linear(model.classifier.in_features, args.classes)
        model = model.to(dev).set_pool(kind).train()
        opt = FusedAdam(model, lr=1e-4)
        model.forward_backward(x, t)
        opt.step()
        g = GraphedTrainStep(model, opt, x, t)
        for _ in range(args.warmup):
            g.replay()
        torch.cuda.synchronize()
        steps[kind] = g
        print("captured %s" % kind, flush=True)
    ms = {k: [] for k in steps}
    for _ in range(args.rounds):
        for kind, g in steps.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            torch.cuda.synchronize()
            e0.record()
            for _ in range(args.steps):
                g.replay()
            e1.record()
            torch.cuda.synchronize()
            ms[kind].append(e0.elapsed_time(e1) / args.steps)
    res = {"workload": "densenet121 bf16 %dx%d bs=%d, graph replay, %d steps x %d rounds interleaved" % (args.size, args.size, args.batch,
                                                                                                    args.steps, args.rounds),
           "ms_per_step": {k: {"median": sorted(v)[len(v) // 2], "min": min(v), "max": max(v)} for k, v in ms.items()}}
    print(json.dumps(res), flush=True)
    if args.out:
        os.makedirs(os.path.dirname(args.out) or ".", exist_ok=True)
        json.dump(res, open(args.out, "w"), indent=1)


if __name__ == "__main__":
    main()
