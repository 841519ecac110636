"""Timing of the two CLAHE kernels (cx_u8_clahe_lut, cx_u8_clahe_apply) next to cx_u8_jitter on the same uint8 batch and
cx_copy_stream on the same number of bytes: device events around many launches, repeated rounds with the kernels interleaved so
that the spread is visible.  The table kernel's LDS adds depend on the histogram (lanes that hit one bin serialise), so three
contents are timed: white noise (flat histograms), a smooth image (ramp + blobs: a few dozen levels per tile, what a radiograph
looks like) and a constant image (every add of a wave on one bin: the worst case).

    python scratch/u8_clahe_timing.py [--iters N] [--rounds R]"""
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
    return a.elapsed_time(b) / iters


def smooth(B, H, W):
    rng = np.random.default_rng(1)
    i, j = np.mgrid[0:H, 0:W].astype(np.float64)
    out = np.empty((B, 1, H, W), np.uint8)
    for b in range(B):
        img = 60.0 + 60.0 * j / W
        for _ in range(6):
            ci, cj, s, a = rng.uniform(0, H), rng.uniform(0, W), rng.uniform(8, W / 4), rng.uniform(40, 130)
            img = img + a * np.exp(-((i - ci) ** 2 + (j - cj) ** 2) / (2 * s * s))
        out[b, 0] = np.clip(img, 0, 255)
    return torch.from_numpy(out)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=200)
    ap.add_argument("--rounds", type=int, default=5)
    a = ap.parse_args()
    from chexpert_amd import _lib, augment, ops
    _lib.lib()
    dev = torch.device("cuda:0")
    B, H, W, grid, clip = 256, 320, 320, (8, 8), 2.0
    L = augment.clahe_clip_count(clip, H // grid[0], W // grid[1])
    base = smooth(16, H, W)
    contents = {"noise": torch.randint(0, 256, (B, 1, H, W), dtype=torch.uint8),
                "smooth": base.repeat(B // 16, 1, 1, 1).contiguous(),
                "constant": torch.full((B, 1, H, W), 93, dtype=torch.uint8)}
    y = torch.empty(B, 1, H, W, dtype=torch.uint8, device=dev)
    bf, cf = torch.full((B,), 1.1, device=dev), torch.full((B,), 0.9, device=dev)
    od = torch.zeros(B, dtype=torch.int32, device=dev)
    for name, xc in contents.items():
        x = xc.to(dev)
        lut = ops.u8_clahe_lut(x, grid, L)
        # (the table kernel through the library directly: ops.u8_clahe_lut allocates its result)
        lib, ptr, sp = _lib.lib(), _lib.ptr, _lib.stream_ptr
        runs = {"clahe_lut": lambda: lib.cx_u8_clahe_lut(ptr(x), ptr(lut), B, H, W, grid[0], grid[1], L, sp()),
                "clahe_apply": lambda: ops.u8_clahe_apply(x, lut, out=y),
                "u8_jitter": lambda: ops.u8_jitter(x, bf, cf, od, out=y),
                "copy_stream": lambda: ops.copy_stream(x, y)}
        for fn in runs.values():
            for _ in range(5):
                fn()
        t = {k: [] for k in runs}
        for _ in range(a.rounds):                # interleaved
            for k, fn in runs.items():
                t[k].append(round(ev_time(fn, a.iters) * 1e3, 2))
        r = dict(case="%d x %d x %d uint8, grid %s, clip %g (L = %d), %s" % (B, H, W, grid, clip, L, name), MB_read_plus_written=round(2 * B * H * W / 1e6, 1))
        for k, v in t.items():
            r[k + " us (median)"] = sorted(v)[len(v) // 2]
            r[k + " us (rounds)"] = v
        assert torch.equal(ops.u8_clahe(x[:16], grid, clip).cpu(), augment.clahe_reference(xc[:16], grid, clip))
        print(json.dumps(r), flush=True)


if __name__ == "__main__":
    main()
