"""DESIGN.md section 4.24 measurement (profiles/eval_autograd_densenet121_kernel_stats.txt).  densenet121 bf16 320x320: eval-mode
frozen-BatchNorm forward+backward (forward_backward in eval()) against the training step.
time: interleaved CUDA-event timing of both modes at bs 64 and 256.  prof MODE B: a few steps of one mode (under rocprofv3)."""
import statistics
import sys
sys.path.insert(0, ".")
import torch
from chexpert_amd.models import densenet121

dev = torch.device("cuda:0")


def setup(B):
    torch.manual_seed(0)
    model = densenet121(num_classes=14).to(dev)
    g = torch.Generator(device=dev).manual_seed(1)
    x = torch.randn(B, 3, 320, 320, device=dev, generator=g)
    t = (torch.rand(B, 14, device=dev, generator=g) > 0.5).float()
    return model, x, t


def step(model, x, t, mode):
    model.train(mode == "train")
    model.zero_grad(set_to_none=False)
    return model.forward_backward(x, t)


if sys.argv[1] == "time":
    for B in (64, 256):
        model, x, t = setup(B)
        ms = {"train": [], "eval": []}
        for m in ("train", "eval"):
            for _ in range(3):
                step(model, x, t, m)
        for rep in range(4):
            for m in ("train", "eval"):
                a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                torch.cuda.synchronize()
                a.record()
                for _ in range(10):
                    step(model, x, t, m)
                b.record()
                torch.cuda.synchronize()
                ms[m].append(a.elapsed_time(b) / 10)
        print("bs=%d  train %.2f ms/step (runs %s)  eval frozen-BN fwd+bwd %.2f ms/step (runs %s)" % (
            B, statistics.median(ms["train"]), " ".join("%.2f" % v for v in ms["train"]), statistics.median(ms["eval"]),
            " ".join("%.2f" % v for v in ms["eval"])), flush=True)
        del model, x, t
        torch.cuda.empty_cache()
else:
    mode, B = sys.argv[2], int(sys.argv[3])
    model, x, t = setup(B)
    for _ in range(3):
        step(model, x, t, mode)
    torch.cuda.synchronize()
    print("done", mode, B)
