#!/usr/bin/env python
"""Generate tests/golden/heads.json by running the REAL reference on CPU: networks whose AAConv2d heads are not 20 key channels
(the runtime-width attention kernels, csrc/aaconv_heads.hip).  Same procedure and the same stand-ins as make_golden.py, whose
helpers it imports; run it where make_golden.py runs (the reference does not travel to the GPU box):

    python tests/golden/make_golden_heads.py

  * wrn16_4_heads_32_b8: WRN-16-4 at --attn_k 0.5 --attn_v 0.25 --attn_nh 4 (layer3: dk 128, dv 64 -> heads of 32 / 16), 32x32, B 8;
  * aadensenet_k16_64_b2: DenseNet(32, (6, 4, 2, 2), 64) at k 1.6, v 0.25, 8 heads (transitions 1-2: dk 200, dv 32 -> heads of
    25 / 4), 64x64, B 2.

Only data (seeds and the reference's outputs) is written; no reference source text is stored."""
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

from make_golden import filled_sd, install_standins, run_net  # noqa: E402

from chexpert_amd import synth  # noqa: E402


def main():
    install_standins()
    from models.attn_aug_conv import BasicBlock, DenseNet, WideResNet
    from oracle import nets
    n_cls = 5
    out = {}
    wrn = dict(k=0.5, v=0.25, nh=4)
    dn = dict(k=1.6, v=0.25, nh=8)
    jobs = {
        "wrn16_4_heads_32_b8": lambda: (WideResNet(BasicBlock, 16, 4, num_classes=n_cls, attn_params=dict(wrn, relative=True, input_dims=(32, 32))),
                                        nets.basic_resnet_spec(n_cls, wide=(16, 4), attn=wrn, input_hw=(32, 32)), 8, 32,
                                        lambda s, x, train: nets.basic_resnet_forward(s, x, wide=(16, 4), train=train, nh=4)),
        "aadensenet_k16_64_b2": lambda: (DenseNet(32, (6, 4, 2, 2), 64, num_classes=n_cls, attn_params=dict(dn, relative=True, input_dims=(64, 64))),
                                         nets.densenet_spec(n_cls, block_config=(6, 4, 2, 2), attn=dn, input_hw=(64, 64)), 2, 64,
                                         lambda s, x, train: nets.densenet_forward(s, x, (6, 4, 2, 2), train=train, nh=8)),
    }
    for tag, job in jobs.items():
        model, spec, B, S, fwd = job()
        sd = filled_sd(spec, 21)
        x = synth.xray_batch(1234, B, S)
        t = synth.targets(99, B, n_cls)
        run_net(model, sd, x, t, tag, out, fwd)
        out[tag].update(B=B, S=S, n_classes=n_cls, sd_seed=21, x_seed=1234, t_seed=99)
    json.dump(out, open(os.path.join(HERE, "heads.json"), "w"))


if __name__ == "__main__":
    main()
