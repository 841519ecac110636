"""Timing of the sample mix (cx_u8_mix, cx_target_mix) next to cx_u8_jitter on the same uint8 batch and cx_copy_stream of the same
size, in one process: device events around `--iters` back-to-back launches after a warm-up, `--rounds` rounds with the cases
alternated inside a round, median / min / max over the rounds.  The training step with and without --mixup is read from the command
line's own logged rate (see profiles/u8_mix_kernel_times.txt for the two commands).

    python scratch/u8_mix_timing.py [--iters N] [--rounds R]"""
import argparse
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def ev_time(fn, iters):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(iters):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) / iters * 1e3           # microseconds


def plan_on(dev, p):
    return [torch.from_numpy(np.ascontiguousarray(p[k], dtype=np.int32)).to(dev) for k in ("perm", "lam_q", "box", "tw_q")]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=200)
    ap.add_argument("--rounds", type=int, default=7)
    a = ap.parse_args()
    from chexpert_amd import _lib, augment, ops, synth
    _lib.lib()
    dev = torch.device("cuda:0")
    B, H, W, n = 256, 320, 320, 14
    N = B * H * W
    x = torch.randint(0, 256, (B, 1, H, W), dtype=torch.uint8, device=dev)
    y = torch.empty_like(x)
    # the same bytes 4 bytes into an allocation: not 16-byte aligned, so cx_u8_mix takes its dword path
    xb, yb = (torch.empty(N + 16, dtype=torch.uint8, device=dev) for _ in range(2))
    x4, y4 = xb[4:4 + N].view(B, 1, H, W), yb[4:4 + N].view(B, 1, H, W)
    x4.copy_(x)
    half = torch.empty(N // 2 * 3, dtype=torch.uint8, device=dev)      # 1.5 images' worth: a copy of it moves the mixup's three
    half2 = torch.empty_like(half)
    ident = {"perm": np.arange(B), "lam_q": np.full(B, 65536), "box": np.zeros((B, 4)), "tw_q": np.full(B, 65536)}
    # the first seed whose lambda lies inside [0.1, 0.9]: every pixel is blended
    mixup = next(p for p in (augment.mix_plan(s, B, H, W, 0.4) for s in range(1, 100)) if 6554 <= p["lam_q"][0] <= 58982)
    plans = {"mixup, whole image": mixup,
             "cutmix, mix_plan batch": augment.mix_plan(2, B, H, W, 0.0, 1.0),
             "cutmix, mix_plan elem": augment.mix_plan(2, B, H, W, 0.0, 1.0, mode="elem"),
             "erase, erase_plan p=0.25": augment.erase_plan(3, B, H, W, prob=0.25),
             "identity": ident}
    cases = {}
    for name, p in plans.items():
        perm, lam_q, box, _ = plan_on(dev, p)
        cases["u8_mix 16 B/lane, " + name] = lambda perm=perm, lam_q=lam_q, box=box: ops.u8_mix(x, perm, lam_q, box, 136, out=y)
        if name in ("mixup, whole image", "identity"):
            cases["u8_mix 4 B/lane, " + name] = lambda perm=perm, lam_q=lam_q, box=box: ops.u8_mix(x4, perm, lam_q, box, 136, out=y4)
    bf, cf = torch.full((B,), 1.1, device=dev), torch.full((B,), 0.9, device=dev)
    od = torch.zeros(B, dtype=torch.int32, device=dev)
    cases["u8_jitter"] = lambda: ops.u8_jitter(x, bf, cf, od, out=y)
    cases["copy_stream, 26.2 MB (52.4 MB moved)"] = lambda: ops.copy_stream(x, y)
    cases["copy_stream, 39.3 MB (78.6 MB moved)"] = lambda: ops.copy_stream(half, half2)
    t = synth.targets(4, B, n).to(dev)
    tout = torch.empty_like(t)
    perm, _, _, tw_q = plan_on(dev, mixup)
    cases["target_mix (256, 14)"] = lambda: ops.target_mix(t, perm, tw_q, out=tout)
    share = {k: float(((p["box"][:, 1] - p["box"][:, 0]) * (p["box"][:, 3] - p["box"][:, 2])).mean()) / (H * W) for k, p in plans.items()}
    print(json.dumps({"case": "%d x %d x %d uint8" % (B, H, W), "iters": a.iters, "rounds": a.rounds, "mean box share of the image": share}), flush=True)
    for fn in cases.values():
        for _ in range(10):
            fn()
    times = {k: [] for k in cases}
    for _ in range(a.rounds):
        for k, fn in cases.items():
            times[k].append(ev_time(fn, a.iters))
    for k, v in times.items():
        v = sorted(v)
        print(json.dumps({"case": k, "median us": round(v[len(v) // 2], 2), "min us": round(v[0], 2), "max us": round(v[-1], 2)}), flush=True)


if __name__ == "__main__":
    main()
