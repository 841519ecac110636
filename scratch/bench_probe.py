"""Cost of the linear probe (the linear-probe section): (a) one cx_probe_loss_grad pass (both launches) over banks of
(M, d, n) = (8192, 1024, 14), (223414, 1024, 14) and (8192, 2048, 14) against cx_copy_stream of the bank's bytes in the same process,
the yardstick of DESIGN section 0: device events around CALLS back-to-back calls, the two taking turns round after round so that a
drift of the box shows in both alike; and (b) the wall time of one probe at the default bank of 8192 images on densenet121 bf16
320x320, split into the embedding (32 eval-mode forwards of 256 images, one batch reused: the time does not depend on the pixels) and
the fit (Gaussian features with labels from a planted logistic model: the iteration count depends on the data, it is printed), against
the route of before, --freeze_backbone_steps -1: one epoch of forward_backward + the fused optimiser's step over the same 8192 images.

  python scratch/bench_probe.py [--calls 20] [--rounds 7] [--skip_model] [--out profiles/probe_bench.txt]"""
import argparse
import math
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def timed(fns, calls, rounds):
    """{name: (median, min, max) ms per call}: device events around `calls` calls, the functions taking turns in every round."""
    ms = {k: [] for k in fns}
    for _ in range(rounds):
        for k, fn in fns.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            torch.cuda.synchronize()
            e0.record()
            for _ in range(calls):
                fn()
            e1.record()
            torch.cuda.synchronize()
            ms[k].append(e0.elapsed_time(e1) / calls)
    return {k: (sorted(v)[len(v) // 2], min(v), max(v)) for k, v in ms.items()}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--skip_model", action="store_true")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    from chexpert_amd import ops, probe, synth
    dev = torch.device("cuda:0")
    lines = []

    def say(s):
        lines.append(s)
        print(s, flush=True)

    # (a) the pass alone
    for M, d, n in ((8192, 1024, 14), (223414, 1024, 14), (8192, 2048, 14)):
        g = torch.Generator(device=dev).manual_seed(M + d)
        X = torch.randn(M, d, device=dev, generator=g)
        Y = (torch.rand(M, n, device=dev, generator=g) < 0.3).float()
        theta = torch.randn(n, d + 1, device=dev, generator=g) / math.sqrt(d)
        loss, grad, count = torch.empty(n, device=dev), torch.empty(n, d + 1, device=dev), torch.empty(n, 3, device=dev)
        need = ops.probe_scratch(M, d, n)
        scratch = torch.empty(need + (need & 1), device=dev)
        dst = torch.empty_like(X)
        fns = {"pass": lambda: ops.probe_loss_grad(X, Y, theta, loss, grad, count, None, 1e-3, None, scratch),
               "copy": lambda: ops.copy_stream(X, dst)}
        for fn in fns.values():
            for _ in range(args.warmup):
                fn()
        torch.cuda.synchronize()
        t0 = time.perf_counter()                      # a quarter of a second of both first: no clock still ramping in the figures
        while time.perf_counter() - t0 < 0.25:
            for fn in fns.values():
                fn()
            torch.cuda.synchronize()
        res = timed(fns, args.calls, args.rounds)
        nbytes = X.numel() * 4
        say("(a) M = %d, d = %d, n = %d: bank %.1f MB, scratch %.1f MB; %d calls x %d rounds after %d warm-up calls, the two taking turns"
            % (M, d, n, nbytes / 1e6, need * 4 / 1e6, args.calls, args.rounds, args.warmup))
        p, c = res["pass"], res["copy"]
        say("    cx_probe_loss_grad (2 launches)  median %.3f ms (min %.3f, max %.3f)   bank bytes / time = %.2f TB/s, %.1f TFLOP/s"
            % (p[0], p[1], p[2], nbytes / p[0] / 1e9, 4.0 * M * d * 16 / p[0] / 1e9))
        say("    cx_copy_stream of the bank       median %.3f ms (min %.3f, max %.3f)   %.2f TB/s read (and as much written)"
            % (c[0], c[1], c[2], nbytes / c[0] / 1e9))
        say("    ratio pass / copy %.2f" % (p[0] / c[0]))
        del X, Y, dst, scratch

    if not args.skip_model:
        # (b) one probe at the default bank against one epoch of the frozen-backbone route
        from chexpert_amd.models import densenet121
        from chexpert_amd.optim import FusedAdam
        B, steps, n, M = 256, 32, 14, 8192
        torch.manual_seed(1234)
        model = densenet121(num_classes=n).to(dev)
        x = synth.xray_batch(1000, B, 320).to(dev)
        t = synth.targets(2000, B, n).to(dev)
        model.eval()
        for _ in range(2):
            model.embed(x)
        torch.cuda.synchronize()
        emb = []
        for _ in range(3):
            t0 = time.perf_counter()
            for _ in range(steps + 1):                # the bank, and one batch for the 234 validation images
                f = model.embed(x)
            torch.cuda.synchronize()
            emb.append(time.perf_counter() - t0)
        rng = np.random.default_rng(5)
        Z = rng.standard_normal((M, 1024))
        planted = rng.standard_normal((n, 1025)) / 32.0
        Yb = (rng.random((M, n)) < 1 / (1 + np.exp(-2 * (Z @ planted[:, :1024].T + planted[:, 1024])))).astype(np.float32)
        Xb = torch.from_numpy((Z * rng.uniform(0.5, 4, size=1024) + rng.uniform(0, 2, size=1024)).astype(np.float32)).to(dev)
        Yb = torch.from_numpy(Yb).to(dev)
        probe.fit(Xb, Yb, l2=1e-3)
        torch.cuda.synchronize()
        fits = []
        for _ in range(3):
            t0 = time.perf_counter()
            res = probe.fit(Xb, Yb, l2=1e-3)
            torch.cuda.synchronize()
            fits.append(time.perf_counter() - t0)
        model.train()
        opt = FusedAdam(model, lr=1e-4)
        for _ in range(3):
            model.forward_backward(x, t)
            opt.step()
        torch.cuda.synchronize()
        epochs = []
        for _ in range(3):
            t0 = time.perf_counter()
            for _ in range(steps):
                model.forward_backward(x, t)
                opt.step()
            torch.cuda.synchronize()
            epochs.append(time.perf_counter() - t0)
        med = lambda v: sorted(v)[len(v) // 2]                                                          # noqa: E731
        say("(b) densenet121 bf16 320x320, bank of %d images in batches of %d, %d classes; host clock to a device synchronise, 3 runs each"
            % (M, B, n))
        say("    embedding, %d eval forwards          median %.3f s (min %.3f, max %.3f)" % (steps + 1, med(emb), min(emb), max(emb)))
        say("    fit at l2 0.001 (%d passes, iterations %d .. %d, status %s)   median %.3f s (min %.3f, max %.3f)"
            % (res["passes"], min(res["iterations"]), max(res["iterations"]), "".join(map(str, res["status"])), med(fits), min(fits), max(fits)))
        say("    one epoch of forward_backward + FusedAdam.step, %d steps (the --freeze_backbone_steps -1 route)   median %.3f s (min %.3f, max %.3f)"
            % (steps, med(epochs), min(epochs), max(epochs)))
        say("    one probe = %.2f epochs of that route" % ((med(emb) + med(fits)) / med(epochs)))
    if args.out:
        os.makedirs(os.path.dirname(args.out) or ".", exist_ok=True)
        open(args.out, "w").write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
