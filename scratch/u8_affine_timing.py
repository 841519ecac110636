"""Timing of the random-affine warp (cx_u8_affine) next to cx_u8_jitter on the same uint8 batch, and the densenet121 bs=256
training step with and without the warp in front, as an interleaved A/B in one process.  Device-event timings; for the per-kernel
table run a training run of the command line with --affine --jitter under `rocprofv3 --kernel-trace --stats`.

    python scratch/u8_affine_timing.py [--kernel-only] [--iters N]"""
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


def kernel_case(B, H, W, iters, dev):
    from chexpert_amd import augment, ops
    x = torch.randint(0, 256, (B, 1, H, W), dtype=torch.uint8, device=dev)
    y = torch.empty_like(x)
    mats = {"default ranges": augment.affine_matrices(1, B, H, W).to(dev),
            "15 deg, shear 5": augment.affine_matrices(1, B, H, W, degrees=15.0, shear=5.0).to(dev),
            "identity": torch.tensor([1.0, 0, 0, 0, 1, 0]).repeat(B, 1).to(dev),
            "scale 0.2-0.3": augment.affine_matrices(1, B, H, W, scale=(0.2, 0.3)).to(dev)}
    r = dict(case="%d x %d x %d uint8" % (B, H, W), MB=round(2 * B * H * W / 1e6, 1))
    for name, m in mats.items():
        run = lambda: ops.u8_affine(x, m, 0, out=y)
        for _ in range(5):
            run()
        r["u8_affine us, " + name] = round(ev_time(run, iters) * 1e3, 2)
    if H * W <= 150 * 1024:
        bf, cf = torch.full((B,), 1.1, device=dev), torch.full((B,), 0.9, device=dev)
        od = torch.zeros(B, dtype=torch.int32, device=dev)
        run = lambda: ops.u8_jitter(x, bf, cf, od, out=y)
        for _ in range(5):
            run()
        r["u8_jitter us"] = round(ev_time(run, iters) * 1e3, 2)
    print(json.dumps(r), flush=True)
    return r


def step_ab(iters, rounds, dev):
    from chexpert_amd import augment, ops, synth
    from chexpert_amd.models import densenet121
    B, S, n = 256, 320, 14
    model = densenet121(num_classes=n).to(dev).train()
    x = torch.randint(0, 256, (B, 1, S, S), dtype=torch.uint8, device=dev)
    t = synth.targets(8, B, n).to(dev)
    y = torch.empty_like(x)
    step = [0]

    def warped():                              # what the training loop does per minibatch: draw on the host, upload, warp, step
        step[0] += 1
        mat = augment.affine_matrices(augment.step_seed(step[0]), B, S, S).to(dev)
        model.forward_backward(ops.u8_affine(x, mat, 0, out=y), t)
    plain = lambda: model.forward_backward(x, t)
    for _ in range(3):
        plain()
        warped()
    a, b = [], []
    for _ in range(rounds):                  # interleaved A / B
        model.zero_grad(set_to_none=False)
        a.append(ev_time(plain, iters))
        b.append(ev_time(warped, iters))
    r = dict(case="densenet121 bs256 320 uint8 step", plain_ms=[round(v, 3) for v in a], affine_ms=[round(v, 3) for v in b],
             median_plain=round(sorted(a)[len(a) // 2], 3), median_affine=round(sorted(b)[len(b) // 2], 3))
    r["delta_ms"] = round(r["median_affine"] - r["median_plain"], 3)
    print(json.dumps(r), flush=True)
    return r


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--kernel-only", action="store_true")
    ap.add_argument("--iters", type=int, default=200)
    ap.add_argument("--rounds", type=int, default=6)
    a = ap.parse_args()
    from chexpert_amd import _lib
    _lib.lib()
    dev = torch.device("cuda:0")
    kernel_case(256, 320, 320, a.iters, dev)
    kernel_case(256, 224, 224, a.iters, dev)
    kernel_case(64, 512, 512, a.iters, dev)
    if not a.kernel_only:
        step_ab(10, a.rounds, dev)


if __name__ == "__main__":
    main()
