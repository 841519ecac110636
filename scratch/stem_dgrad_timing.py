"""Timing of the stem input gradient (cx_stem_input_grad) alone, and the densenet121 bs=256 training step with and without
forward_backward(input_grad=...), as an interleaved A/B in one process.  Device-event timings; for the per-kernel table run it
under `rocprofv3 --kernel-trace --stats` with --kernel-only.

    python scratch/stem_dgrad_timing.py [--kernel-only] [--iters N]"""
import argparse
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def ev_time(fn, iters):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(iters):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) / iters


def kernel_case(name, B, H, C0, k, pad, iters, dev):
    from chexpert_amd import ops
    Ho = (H + 2 * pad - k) // 2 + 1
    dz = torch.randn(B, Ho, Ho, C0, device=dev).bfloat16()
    y = torch.randn(B, Ho, Ho, C0, device=dev).bfloat16()
    pa, pb, pc = (torch.rand(C0, device=dev) for _ in range(3))
    w = torch.randn(C0, 3, k, k, device=dev) * 0.1
    dx = torch.empty(B, 3, H, H, device=dev)
    run = lambda: ops.stem_input_grad(dz, y, pa, pb, pc, w, dx, stride=2, pad=pad)
    for _ in range(3):
        run()
    ms = ev_time(run, iters)
    nbytes = 2 * dz.numel() * 2 + dx.numel() * 4
    r = dict(case=name, ms=round(ms, 4), GB=round(nbytes / 1e9, 3), GBps=round(nbytes / ms / 1e6, 1))
    print(json.dumps(r))
    return r


def step_ab(iters, rounds, dev):
    from chexpert_amd import synth
    from chexpert_amd.models import densenet121
    B, S, n = 256, 320, 14
    model = densenet121(num_classes=n).to(dev).train()
    x = synth.xray_batch(7, B, S).to(dev)
    t = synth.targets(8, B, n).to(dev)
    buf = torch.empty_like(x)
    plain = lambda: model.forward_backward(x, t)
    with_dx = lambda: model.forward_backward(x, t, input_grad=buf)
    for _ in range(3):
        plain()
        with_dx()
    a, b = [], []
    for _ in range(rounds):                  # interleaved A / B
        model.zero_grad(set_to_none=False)
        a.append(ev_time(plain, iters))
        b.append(ev_time(with_dx, iters))
    r = dict(case="densenet121 bs256 320 step", plain_ms=[round(v, 3) for v in a], input_grad_ms=[round(v, 3) for v in b],
             median_plain=round(sorted(a)[len(a) // 2], 3), median_input_grad=round(sorted(b)[len(b) // 2], 3))
    r["delta_ms"] = round(r["median_input_grad"] - r["median_plain"], 3)
    print(json.dumps(r))
    return r


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--kernel-only", action="store_true")
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=6)
    a = ap.parse_args()
    from chexpert_amd import _lib
    _lib.lib()
    dev = torch.device("cuda:0")
    kernel_case("densenet121 stem 7x7 s2 p3, bf16, 320^2, B=256", 256, 320, 64, 7, 3, a.iters, dev)
    kernel_case("efficientnet-b4 stem 3x3 s2 p1, bf16, 380^2, B=64", 64, 380, 48, 3, 1, a.iters, dev)
    if not a.kernel_only:
        step_ab(max(a.iters // 4, 3), a.rounds, dev)


if __name__ == "__main__":
    main()
