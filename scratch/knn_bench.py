"""Cost of the exact kNN search at the workload's own shapes, on unit-norm Gaussian rows:
  (a) the probe            Q = 234, M = 223 414, d = 1024, k = 200   yardstick: one read of the bank (cx_copy_stream of the same bytes)
  (b) the default bank     Q = 234, M = 8192                         the same yardstick
  (c) leave-one-out        Q = M = 20 000, d = 1024, groups = the row's position     yardstick: the fp32 matrix rate (TFLOP/s)
and beside each torch's `(q @ bank.T).topk(k)` in fp32 in the same process, what a user would otherwise write (it stores Q x M floats
and has neither the index rule on ties nor group exclusion).  Every figure: WARMUP untimed launches, then ROUNDS rounds of CALLS launches
between two device events, the candidates taking turns round after round; median, min and max of the rounds.

  python scratch/knn_bench.py [--out profiles/knn_bench.txt] [--cases abc]"""
import argparse
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def time_rounds(fns, calls, rounds, warmup):
    for f in fns.values():
        for _ in range(warmup):
            f()
    torch.cuda.synchronize()
    ms = {k: [] for k in fns}
    for _ in range(rounds):
        for k, f in fns.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(calls):
                f()
            e1.record()
            torch.cuda.synchronize()
            ms[k].append(e0.elapsed_time(e1) / calls)
    return {k: (sorted(v)[len(v) // 2], min(v), max(v)) for k, v in ms.items()}


def unit_rows(seed, rows, d, dev):
    g = torch.Generator(device="cpu").manual_seed(seed)
    x = torch.randn(rows, d, generator=g)
    return (x / x.norm(dim=1, keepdim=True)).to(dev)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--cases", default="abc")
    ap.add_argument("--calls", type=int, default=5)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    from chexpert_amd import ops
    dev = torch.device("cuda:0")
    lines = []

    def say(text):
        lines.append(text)
        print(text, flush=True)
    cases = {"a": ("probe", 234, 223414, 1024, 200, False), "b": ("default bank", 234, 8192, 1024, 200, False),
             "c": ("leave-one-out", 20000, 20000, 1024, 200, True)}
    for name in args.cases:
        label, Q, M, d, k, loo = cases[name]
        bank = unit_rows(100 + M % 97, M, d, dev)
        q = bank if loo else unit_rows(7, Q, d, dev)
        group = torch.arange(M, dtype=torch.int32, device=dev) if loo else None
        sim, idx = torch.empty(Q, k, device=dev), torch.empty(Q, k, dtype=torch.int32, device=dev)
        scratch = torch.empty(ops.knn_scratch(Q, M, k, 0), device=dev)
        slices = scratch.numel() // (2 * Q * k)
        copy_dst = torch.empty_like(bank)
        fns = {"knn": lambda: ops.knn_topk(q, bank, k, sim, idx, group, group, scratch, 0),
               "copy": lambda: ops.copy_stream(bank, copy_dst)}
        calls = args.calls
        if name == "c":                                            # (Q x M fp32 = 1.6 GB for torch; a leave-one-out needs the diagonal masked too)
            def torch_line():
                s = q @ bank.T
                s.fill_diagonal_(float("-inf"))
                return s.topk(k)
            calls = max(1, args.calls // 2)
        else:
            def torch_line():
                return (q @ bank.T).topk(k)
        fns["torch"] = torch_line
        res = time_rounds(fns, calls, args.rounds, args.warmup)
        # agreement of the two answers on this input (ties are absent on Gaussian rows: the sets are equal unless a pair is within rounding)
        ts, ti = torch_line()
        same = float((ti.sort(1).values == idx.long().sort(1).values).float().mean())
        flop, nbytes = 2.0 * Q * M * d, 4.0 * M * d
        fmt = lambda v: "median %.3f ms (min %.3f, max %.3f)" % v                                        # noqa: E731
        say("(%s) %s: Q = %d, M = %d, d = %d, k = %d, %d slices, scratch %.1f MB; %d launches x %d rounds after %d warm-up launches"
            % (name, label, Q, M, d, k, slices, 4e-6 * scratch.numel(), calls, args.rounds, args.warmup))
        say("    cx_knn_topk (search + merge)    %s   %.1f TFLOP/s, bank bytes / time = %.2f TB/s" % (fmt(res["knn"]), 1e-9 * flop / res["knn"][0],
                                                                                                     1e-9 * nbytes / res["knn"][0]))
        say("    cx_copy_stream of the bank      %s   %.2f TB/s read (and as much written)" % (fmt(res["copy"]), 1e-9 * nbytes / res["copy"][0]))
        say("    torch (q @ bank.T).topk(k)      %s   %.1f TFLOP/s; Q x M buffer %.1f MB; share of index entries equal to ours %.6f"
            % (fmt(res["torch"]), 1e-9 * flop / res["torch"][0], 4e-6 * Q * M, same))
        say("    ratio knn / copy %.2f, knn / torch %.2f" % (res["knn"][0] / res["copy"][0], res["knn"][0] / res["torch"][0]))
        del bank, q, copy_dst, scratch, ts, ti
        torch.cuda.empty_cache()
    if args.out:
        os.makedirs(os.path.dirname(args.out) or ".", exist_ok=True)
        open(args.out, "w").write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
