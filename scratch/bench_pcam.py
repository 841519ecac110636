"""The kernels of the pcam head beside those of the csra head at densenet121's head shape (B = 256, HW = 100, C = 1024, n = 5, bf16;
DESIGN.md section 4.46).  Meant to run under one kernel trace, with no counters:

  rocprofv3 --kernel-trace --stats -d <dir> -- python scratch/bench_pcam.py [--iters 20]

The script launches, `iters` times over, cx_pcam_head_fwd + cx_pcam_head_bwd (rows mode) and then cx_csra_head_fwd + cx_csra_head_bwd on
the same operands; the per-kernel averages (pcam_stat_kernel / pcam_ds_kernel beside csra_stat_kernel / csra_ds_kernel) are read from
the trace's statistics."""
import argparse
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=256)
    ap.add_argument("--hw", type=int, default=10)
    ap.add_argument("--channels", type=int, default=1024)
    ap.add_argument("--classes", type=int, default=5)
    ap.add_argument("--iters", type=int, default=20)
    a = ap.parse_args()
    from chexpert_amd import ops
    dev = torch.device("cuda:0")
    B, h, C, n = a.batch, a.hw, a.channels, a.classes
    g_ = torch.Generator().manual_seed(1)
    r = lambda *s: torch.randn(*s, generator=g_).to(dev)                                                  # noqa: E731
    x = r(B, h, h, C).to(torch.bfloat16)
    g = torch.empty_like(x)
    sc, sh, mean, rstd = r(C).abs() + 0.5, r(C) * 0.1, r(C) * 0.1, r(C).abs() + 0.5
    W, bias, dl = r(n, C) * 0.05, r(n), r(B, n) / B
    attn = torch.tensor([0.3, 2.0], device=dev)
    logits, s, stat = torch.empty(B, n, device=dev), torch.empty(B, n, h * h, device=dev), torch.empty(B, n, ops.CSRA_STAT, device=dev)
    scratch = torch.empty(ops.pcam_bwd_scratch(B, h * h, C, n), device=dev)
    rows = torch.empty(2, B, C, device=dev)
    dW, db = torch.zeros(n, C, device=dev), torch.zeros(n, device=dev)
    for _ in range(a.iters):
        ops.pcam_head_fwd(x, sc, sh, None, W, bias, logits, s, stat, act=ops.POOL_ACT_RELU)
        ops.pcam_head_bwd(dl, s, stat, x, sc, sh, None, mean, rstd, sc, W, g, rows[0], rows[1], dW, db, scratch, act=ops.POOL_ACT_RELU,
                          stat_rows=B)
    for _ in range(a.iters):
        ops.csra_head_fwd(x, sc, sh, None, W, bias, attn, logits, s, stat, act=ops.POOL_ACT_RELU)
        ops.csra_head_bwd(dl, s, stat, attn, x, sc, sh, None, mean, rstd, sc, W, g, rows[0], rows[1], dW, db, scratch, act=ops.POOL_ACT_RELU,
                          stat_rows=B)
    torch.cuda.synchronize()
    print("done: %d iterations at B=%d HW=%d C=%d n=%d" % (a.iters, B, h * h, C, n))


if __name__ == "__main__":
    main()
