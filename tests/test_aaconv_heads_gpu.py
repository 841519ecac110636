"""GPU: the runtime-width attention kernels (csrc/aaconv_heads.hip: head widths dk/nh, dv/nh of 1 .. 64 beside the dkh = 20 kernels)
against the oracle's closed form, and the networks of the reference's CIFAR harness that use them."""
import json
import os

import numpy as np
import pytest
import torch

from chexpert_amd import synth

pytestmark = pytest.mark.gpu
G = os.path.join(os.path.dirname(__file__), "golden")


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    from chexpert_amd import _lib
    _lib.lib()
    return torch.device("cuda:0")


def bf(t):
    return t.to(torch.bfloat16).float()


def close(got, want, rel, what=""):
    scale = want.abs().max().item() + 1e-9
    err = (got - want).abs().max().item()
    assert err <= rel * scale, "%s: max err %.3e vs scale %.3e (rel %.2e)" % (what, err, scale, err / scale)


def _rel(a, b):
    return (a - b).abs().max().item() / (b.abs().max().item() + 1e-12)


def _cos(a, b):
    a, b = a.double().flatten(), b.double().flatten()
    return float((a * b).sum() / (a.norm() * b.norm() + 1e-30)), float(a.norm() / (b.norm() + 1e-30))


def _inputs(nh, dkh, dvh, B, H, W, relative, seed=1):
    dk, dv = nh * dkh, nh * dvh
    Cq = 2 * dk + dv
    qkv = bf(synth.uniform(seed, (B, H, W, Cq), -1.5, 1.5))
    if relative:
        rel_h = synth.uniform(seed + 1, (dkh, 2 * H - 1), -1, 1) + dk ** -0.5
        rel_w = synth.uniform(seed + 2, (dkh, 2 * W - 1), -1, 1) + dk ** -0.5
    else:                                          # relative=False: the models run the kernels with all-zero tables
        rel_h, rel_w = torch.zeros(dkh, 2 * H - 1), torch.zeros(dkh, 2 * W - 1)
    d_o = synth.uniform(seed + 3, (B, H * W, dv), -1, 1)
    return qkv, rel_h, rel_w, d_o


SHAPES = [(8, 32, 8, 2, 16, 16, True),       # WRN-28-10 layer3 at k 0.4, the Bottleneck / DenseNet rows at k 0.5 (dvh 6 in 8)
          (8, 25, 4, 2, 10, 10, True),       # the k = 1.6 DenseNet: head offsets n * 25 not a multiple of 4
          (4, 20, 16, 2, 8, 8, True),        # the old key width with more than 13 value channels
          (4, 32, 16, 2, 8, 8, True),        # WRN-16-4 layer3 at k 0.5, v 0.25, 4 heads
          (2, 64, 40, 1, 12, 20, True),      # widest keys, H != W
          (8, 8, 2, 2, 20, 20, True),        # narrow keys
          (4, 48, 26, 1, 40, 40, True),      # the largest map and dv = 104: LDS beyond 64 KB
          (1, 64, 64, 1, 7, 9, True),        # one head of 64 / 64: the key side in two launches
          (4, 32, 16, 2, 8, 8, False)]       # relative=False


@pytest.mark.parametrize("dtype", ["bf16", "fp32"])
@pytest.mark.parametrize("nh,dkh,dvh,B,H,W,relative", SHAPES)
def test_attention_kernels_match_closed_form(dev, dtype, nh, dkh, dvh, B, H, W, relative):
    from chexpert_amd import ops
    from oracle import aaconv
    dk, dv = nh * dkh, nh * dvh
    Cq = 2 * dk + dv
    qkv, rel_h, rel_w, d_o = _inputs(nh, dkh, dvh, B, H, W, relative)
    t = qkv.permute(0, 3, 1, 2).clone().requires_grad_(True)               # (B,Cq,H,W)
    rh, rw = rel_h.clone().requires_grad_(True), rel_w.clone().requires_grad_(True)
    q = t[:, :dk].reshape(B, nh, dkh, H, W) * dkh ** -0.5
    k = t[:, dk:2 * dk].reshape(B, nh, dkh, H, W)
    v = t[:, 2 * dk:].reshape(B, nh, dvh, H * W)
    P = torch.softmax(aaconv.attention_logits(q, k, rh, rw).reshape(B, nh, H * W, H * W), -1)
    o_ref = torch.einsum("bnqk,bndk->bqnd", P, v).reshape(B, H * W, dv)
    (o_ref * d_o).sum().backward()
    qd = (qkv.to(torch.bfloat16) if dtype == "bf16" else qkv.clone()).to(dev)
    o = torch.zeros(B, H * W, dv, device=dev)
    lse = torch.zeros(B * nh, H * W, device=dev)
    ops.aa_attention_fwd(qd, rel_h.to(dev), rel_w.to(dev), o, lse, nh, dk, dv)
    # the launcher's tag: the runtime-width family, the storage type, the key / value capacities the widths are padded to
    st, KC, VC = ("bf16" if dtype == "bf16" else "f32"), (32 if dkh <= 32 else 64), next(c for c in (8, 16, 32, 64) if dvh <= c)
    assert ops.last_kernel() == "aa_heads_fwd<%s,%d,%d>" % (st, KC, VC), ops.last_kernel()
    close(o.cpu(), o_ref.detach(), 2e-4, "o")
    if H * W <= 400:
        wts = ops.aa_attention_weights(qd, rel_h.to(dev), rel_w.to(dev), lse, nh, dk, dv)
        # (the maps do not depend on the value width: keys of 20 channels take the dkh = 20 kernel whatever dv/nh is)
        assert ops.last_kernel() == ("aa_weights<%s>" % st if dkh == 20 else "aa_heads_weights<%s,%d>" % (st, KC)), ops.last_kernel()
        assert wts.shape == (B, nh, H * W, H * W)
        close(wts.cpu(), P.detach(), 2e-4, "weights")
        assert (wts.sum(-1) - 1).abs().max().item() < 1e-4
    dqkv = torch.full((B, H * W, Cq), 7.0, device=dev)
    drh, drw = torch.zeros_like(rel_h, device=dev), torch.zeros_like(rel_w, device=dev)
    ops.aa_attention_bwd(qd, rel_h.to(dev), rel_w.to(dev), o, d_o.to(dev), lse, dqkv, drh, drw, nh, dk, dv)
    assert ops.last_kernel() == "aa_heads_bwd<%s,%d,%d>" % (st, KC, VC), ops.last_kernel()
    want = t.grad.permute(0, 2, 3, 1).reshape(B, H * W, Cq)
    close(dqkv.cpu()[..., :dk], want[..., :dk], 1e-3, "dq")
    close(dqkv.cpu()[..., dk:2 * dk], want[..., dk:2 * dk], 1e-3, "dk")
    close(dqkv.cpu()[..., 2 * dk:], want[..., 2 * dk:], 1e-3, "dv")
    close(drh.cpu(), rh.grad, 1e-3, "d key_rel_h")
    close(drw.cpu(), rw.grad, 1e-3, "d key_rel_w")


def test_out_of_range_heads_are_rejected(dev):
    from chexpert_amd import ops
    B, H, W = 1, 4, 4
    for nh, dkh, dvh in ((1, 72, 8), (1, 32, 72), (2, 32, 56)):         # dkh > 64, dvh > 64, dv = 112 > 104
        dk, dv = nh * dkh, nh * dvh
        qkv = torch.zeros(B, H, W, 2 * dk + dv, dtype=torch.bfloat16, device=dev)
        o, lse = torch.zeros(B, H * W, dv, device=dev), torch.zeros(B * nh, H * W, device=dev)
        with pytest.raises(RuntimeError):
            ops.aa_attention_fwd(qkv, torch.zeros(dkh, 2 * H - 1, device=dev), torch.zeros(dkh, 2 * W - 1, device=dev), o, lse, nh, dk, dv)


def test_backward_is_bit_reproducible(dev):
    """The relative-table gradients go through per-workgroup slabs summed in workgroup order: two calls, the same bits."""
    from chexpert_amd import ops
    nh, dkh, dvh, B, H, W = 8, 25, 4, 2, 20, 20
    dk, dv = nh * dkh, nh * dvh
    qkv, rel_h, rel_w, d_o = _inputs(nh, dkh, dvh, B, H, W, True, seed=11)
    saved = ops.WGRAD_SCRATCH_FLOATS
    ops.set_det_wgrad(True)
    try:
        qd = qkv.to(torch.bfloat16).to(dev)
        o, lse = torch.zeros(B, H * W, dv, device=dev), torch.zeros(B * nh, H * W, device=dev)
        ops.aa_attention_fwd(qd, rel_h.to(dev), rel_w.to(dev), o, lse, nh, dk, dv)
        res = []
        for _ in range(2):
            dqkv = torch.zeros(B, H * W, 2 * dk + dv, device=dev)
            drh, drw = torch.zeros(dkh, 2 * H - 1, device=dev), torch.zeros(dkh, 2 * W - 1, device=dev)
            ops.aa_attention_bwd(qd, rel_h.to(dev), rel_w.to(dev), o, d_o.to(dev), lse, dqkv, drh, drw, nh, dk, dv)
            res.append((dqkv, drh, drw))
        torch.cuda.synchronize()
        for a, b in zip(*res):
            assert torch.equal(a, b)
    finally:
        ops.WGRAD_SCRATCH_FLOATS = saved


# ---------------------------------------------------------------------------------------------- networks
DN_ATTN = dict(k=1.6, v=0.25, nh=8)
WRN_ATTN = dict(k=0.5, v=0.25, nh=4)


def _smooth(sd, bias):
    for k in sd:
        if k.endswith(".bias") and "classifier" not in k and not k.startswith("fc"):
            sd[k] = torch.full_like(sd[k], bias)
        if k.endswith(".weight") and sd[k].dim() == 1:
            sd[k] = synth.uniform(7, sd[k].shape, 0.8, 1.2)
    return sd


def _densenet(n_cls, S, seed, dev, smooth):
    from chexpert_amd.models import DenseNet
    from oracle import nets
    cfg = (6, 4, 2, 2)
    spec = nets.densenet_spec(n_cls, block_config=cfg, attn=DN_ATTN, input_hw=(S, S))
    sd = synth.fill_state_dict_(nets.zeros_state_dict(spec), seed)
    if smooth:
        _smooth(sd, 2.5)
    model = DenseNet(32, cfg, 64, num_classes=n_cls, attn_params=dict(DN_ATTN, relative=True, input_dims=(S, S)))
    t1 = model.features.transition1.conv
    assert (t1.dk, t1.dv, t1.nh) == (200, 32, 8)
    assert list(model.state_dict().keys()) == list(spec.keys())
    model.load_state_dict(sd, strict=True)
    return model.to(dev), sd


def _wrn(n_cls, S, seed, dev, smooth):
    from chexpert_amd.models import BasicBlock, WideResNet
    from oracle import nets
    spec = nets.basic_resnet_spec(n_cls, wide=(16, 4), attn=WRN_ATTN, input_hw=(S, S))
    sd = synth.fill_state_dict_(nets.zeros_state_dict(spec), seed)
    if smooth:
        _smooth(sd, 1.0)
    model = WideResNet(BasicBlock, 16, 4, num_classes=n_cls, attn_params=dict(WRN_ATTN, relative=True, input_dims=(S, S)))
    aa3 = model.layer3[0].conv1
    assert (aa3.dk, aa3.dv, aa3.nh) == (128, 64, 4)
    assert list(model.state_dict().keys()) == list(spec.keys())
    model.load_state_dict(sd, strict=True)
    return model.to(dev), sd


@pytest.mark.parametrize("dtype", ["fp32", "bf16"])
def test_densenet_with_25_channel_key_heads_matches_oracle(dev, dtype):
    """DenseNet(32, (6, 4, 2, 2), 64) at k 1.6, v 0.25, 8 heads: transitions 1-2 have heads of 25 key / 4 value channels (the new
    kernels), transition 3 heads of 20 / 3 (the dkh = 20 kernels).  fp32 storage: the sharp check; bf16: the bounds of
    test_aaconv_gpu.py's value-head test."""
    from oracle import nets, step
    cfg, B, S, n_cls = (6, 4, 2, 2), 4, 64, 5
    model, sd = _densenet(n_cls, S, 25, dev, smooth=True)
    model = model.storage_dtype(dtype).train()
    x, t = synth.xray_batch(1236, B, S), synth.targets(97, B, n_cls)
    fwd = lambda s_, xx, train=True: nets.densenet_forward(s_, xx, cfg, train=train, nh=8)
    loss_o, logits_o, grads_o = step.train_step(fwd, {k: v.clone() for k, v in sd.items()}, x, t)
    model.zero_grad()
    loss, logits = model.forward_backward(x.to(dev), t.to(dev))
    tol = 1e-4 if dtype == "fp32" else 4e-2
    print("k1.6 densenet %s: logits rel %.3e" % (dtype, _rel(logits.cpu(), logits_o)))
    assert _rel(logits.cpu(), logits_o) < tol, _rel(logits.cpu(), logits_o)
    for k, p in model.named_parameters():
        if "transition" in k and p.dim() > 1:
            c, n = _cos(p.grad.cpu(), grads_o[k])
            assert (c > 0.9999 and abs(n - 1) < 1e-3) if dtype == "fp32" else (c > 0.95 and abs(n - 1) < 0.13), (k, c, n)


def test_wideresnet_16_4_wide_heads_smooth_regime(dev):
    """WRN-16-4 at --attn_k 0.5 --attn_v 0.25 --attn_nh 4 (layer3: heads of 32 / 16), bf16, in the smooth regime against the fp32
    oracle with the bounds of test_resnet_gpu.py's WRN-10-10 attention test; a repeated step bit for bit; the attention maps."""
    from oracle import nets, step
    n_cls, B, S = 5, 8, 32
    model, sd = _wrn(n_cls, S, 21, dev, smooth=True)
    x, t = synth.xray_batch(1234, B, S), synth.targets(99, B, n_cls)
    fwd = lambda s, xx: nets.basic_resnet_forward(s, xx, wide=(16, 4), train=True, nh=4)
    loss_o, logits_o, grads_o = step.train_step(fwd, {k: v.clone() for k, v in sd.items()}, x, t)
    model.train()
    loss, logits = model.forward_backward(x.to(dev), t.to(dev))
    e = _rel(logits.cpu(), logits_o)
    print("aawrn16_4 wide heads smooth: train logits rel %.3e" % e)
    assert e < 2e-2 and abs(loss.item() - loss_o.item()) < 1e-2 * abs(loss_o.item())
    g1 = {k: p.grad.detach().clone() for k, p in model.named_parameters()}
    for k in ("layer3.0.conv1.out_proj.weight", "layer3.0.conv1.key_rel_h", "layer3.0.conv1.key_rel_w", "layer3.0.conv1.in_proj_qkv.weight",
              "layer3.1.conv1.in_proj_qkv.weight", "layer2.0.conv1.out_proj.weight"):
        c, n = _cos(g1[k].cpu(), grads_o[k])
        print("  %s cos %.4f norm ratio %.4f" % (k, c, n))
        assert c > 0.95 and abs(n - 1) < 0.08, (k, c, n)
    for k, g in g1.items():
        assert torch.isfinite(g).all(), k
    model.zero_grad()
    model.forward_backward(x.to(dev), t.to(dev))
    for k, p in model.named_parameters():
        assert torch.equal(p.grad, g1[k]), k
    model.eval()
    with torch.no_grad():
        model(x.to(dev))
        w = model.layer3[0].conv1.weights
    assert w.shape == (8, 4, 64, 64)
    assert (w.sum(-1) - 1).abs().max().item() < 1e-4


def _fixture_step(model, rec, dev):
    n_cls, B, S = rec["n_classes"], rec["B"], rec["S"]
    x, t = synth.xray_batch(rec["x_seed"], B, S), synth.targets(rec["t_seed"], B, n_cls)
    model.train()
    out = model(x.to(dev))
    loss = torch.nn.BCEWithLogitsLoss(reduction="none")(out, t.to(dev)).sum(1).mean(0)
    model.zero_grad()
    loss.backward()
    for k, p in model.named_parameters():
        assert p.grad is not None and torch.isfinite(p.grad).all(), k
    return _rel(out.detach().cpu(), torch.tensor(rec["logits_train"])), loss.item()


def test_wideresnet_16_4_wide_heads_matches_reference_golden_fixture(dev):
    """WRN-16-4 at k 0.5, v 0.25, 4 heads: train logits and loss against the fixture recorded from the real reference
    (tests/golden/make_golden_heads.py), hash-filled weights, bf16 (WideResNet has no fp32 storage mode), with the literal bounds of
    test_resnet_gpu.py's attention fixture test."""
    rec = json.load(open(os.path.join(G, "heads.json")))["wrn16_4_heads_32_b8"]
    model, sd = _wrn(rec["n_classes"], rec["S"], rec["sd_seed"], dev, smooth=False)
    assert sum(p.numel() for p in model.parameters()) == rec["n_params"]
    e, loss = _fixture_step(model, rec, dev)
    print("wrn16_4 heads golden: train logits rel %.3e, loss %.5f (reference %.5f)" % (e, loss, rec["loss"]))
    assert e < 5e-2
    assert abs(loss - rec["loss"]) < 3e-2 * abs(rec["loss"])


def test_densenet_k16_matches_reference_golden_fixture(dev):
    """The k = 1.6 DenseNet (heads of 25 / 4 in transitions 1-2) against the fixture recorded from the real reference at B = 2 with
    hash-filled weights.  fp32 storage mode: the bounds of test_fp32_gpu.py's attention fixture test (train logits 1e-3, loss 1e-4,
    gradient norms 1e-2).  bf16: the loss to the literal 3e-2 of test_resnet_gpu.py's attention fixture test; the train logits
    are not bounded in bf16 here -- at B = 2 the batch statistics of hash-filled weights amplify storage rounding (measured 7.4e-2
    against 1.1e-5 in the fp32 mode; the project's own B = 2 attention DenseNet fixture, dkh = 20, measures 2.1e-2 in bf16 and is
    checked in the fp32 mode only, test_fp32_gpu.py)."""
    rec = json.load(open(os.path.join(G, "heads.json")))["aadensenet_k16_64_b2"]
    model, sd = _densenet(rec["n_classes"], rec["S"], rec["sd_seed"], dev, smooth=False)
    assert sum(p.numel() for p in model.parameters()) == rec["n_params"]
    e, loss = _fixture_step(model.storage_dtype("fp32"), rec, dev)
    gmax = max(r["l2"] for r in rec["grads"].values())
    worst = max((abs(p.grad.double().norm().item() / rec["grads"][k]["l2"] - 1), k) for k, p in model.named_parameters()
                if rec["grads"][k]["l2"] > 1e-4 * gmax)
    print("densenet k1.6 golden fp32: train logits rel %.3e, loss %.6f (reference %.6f), worst gradient l2 %.3e (%s)" % (
        e, loss, rec["loss"], worst[0], worst[1]))
    assert e < 1e-3
    assert abs(loss - rec["loss"]) < 1e-4 * abs(rec["loss"])
    assert worst[0] < 1e-2
    model, sd = _densenet(rec["n_classes"], rec["S"], rec["sd_seed"], dev, smooth=False)
    e, loss = _fixture_step(model, rec, dev)
    print("densenet k1.6 golden bf16: train logits rel %.3e, loss %.5f (reference %.5f)" % (e, loss, rec["loss"]))
    assert abs(loss - rec["loss"]) < 3e-2 * abs(rec["loss"])


def test_cifar_harness_wideresnet_with_wide_heads(dev, tmp_path):
    """The command line of the issue: WRN-16-4 --attn --attn_k 0.5 --attn_v 0.25 --attn_nh 4 trains one epoch, then --vis_attn on the
    checkpoint draws the maps of its four AAConv2d layers."""
    from chexpert_amd import cifar
    out = str(tmp_path / "run")
    attn = ["--attn", "--attn_k", "0.5", "--attn_v", "0.25", "--attn_nh", "4"]
    assert cifar.main(["--train"] + attn + ["--synthetic", "64", "--batch_size", "32", "--n_epochs", "1", "--eval_interval", "1",
                                        "--output_dir", out, "wideresnet", "16", "4"]) == 0
    recs = [json.loads(l) for l in open(os.path.join(out, "log.jsonl"))]
    tr = [r["train_loss"] for r in recs if "train_loss" in r]
    assert tr and all(np.isfinite(tr)), tr
    ckpt = os.path.join(out, "checkpoint.pt")
    assert os.path.exists(ckpt)
    ov = str(tmp_path / "vis")
    assert cifar.main(["--vis_attn", "--restore", ckpt] + attn + ["--synthetic", "16", "--batch_size", "16", "--output_dir", ov, "wideresnet", "16", "4"]) == 0
    pngs = [f for f in os.listdir(ov) if f.startswith("vis_attn_image_")]
    assert len(pngs) == 8 * 4 and os.path.getsize(os.path.join(ov, "vis_attn_image_0_layer_3.png")) > 2000
