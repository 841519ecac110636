"""EfficientNet B0-B7 (compound-scaled MBConv nets) on the gfx950 kernels.

Drop-in surface of /root/reference/models/efficientnet.py: `construct_model(model_name, n_classes)`
(:188-228), the `nn.Sequential` index layout and therefore the `state_dict` keys (`stem.0/1`,
`blocks.S.B.{0..8}`, SE at `.6.1/.6.3` (or `.3.1/.3.3` when expand_ratio == 1), `head.0/1/6`), `model.head[1]`,
`model.head[-1]`, BatchNorm eps 1e-3 / momentum 0.01 (:140, :174-176), class `__name__` = model name (:226).
Reproduced quirks: symmetric `ceil(total/2)` "same" padding (:53-64), SE width from the block INPUT channels
(:82), skip whenever shapes match (:109).

Schedule per MBConv block (NHWC bf16):
  expand 1x1 (implicit GEMM, raw + stats) -> depthwise k x k with bn+Swish applied on load (raw + stats)
  -> SE: global pool of swish(bn(.)), two tiny FCs -> u = swish(bn(y_d)) * s[b][c] (one pass)
  -> project 1x1 (implicit GEMM) -> x_out = bn(y_p) (+ x_in).
DropConnect (efficientnet.py:44-51, :100-101) and the classifier Dropout (:169-171) are applied in train mode: per-image /
per-element keep masks drawn on the GPU by `cx_dropout_mask_dev` from (model.drop_seed, device-side count of training forwards, block) -- reproducible and
independent of torch's RNG; the parity tests feed the drawn masks (`engine.last_masks`) to the oracle.
"""
import math

import torch
import torch.nn as nn
import torch.nn.functional as F

from .. import ops
from ._fused import FusedEngine, FusedNet, _BN
from .densenet import BatchNorm2dParams, Conv2dParams, PoolMarker, _FusedOnly

SCALING_PARAMS = {  # width, depth, resolution, dropout (efficientnet.py:13-21)
    "efficientnet-b0": (1.0, 1.0, 224, 0.2), "efficientnet-b1": (1.0, 1.1, 240, 0.2), "efficientnet-b2": (1.1, 1.2, 260, 0.3),
    "efficientnet-b3": (1.2, 1.4, 300, 0.3), "efficientnet-b4": (1.4, 1.8, 380, 0.4), "efficientnet-b5": (1.6, 2.2, 456, 0.4),
    "efficientnet-b6": (1.8, 2.6, 528, 0.5), "efficientnet-b7": (2.0, 3.1, 600, 0.5)}
_BASE = [(1, 32, 16, 3, 1, 1), (2, 16, 24, 3, 2, 6), (2, 24, 40, 5, 2, 6), (3, 40, 80, 3, 2, 6), (3, 80, 112, 5, 1, 6),
         (4, 112, 192, 5, 2, 6), (1, 192, 320, 3, 1, 6)]     # repeats, in, out, k, stride, expand (:149-155)


class Marker(_FusedOnly, nn.Module):
    pass


class DropMarker(_FusedOnly, nn.Module):
    def __init__(self, p):
        super().__init__()
        self.p = p


class SELayer(nn.Sequential):
    def __init__(self, c, r):
        super().__init__(PoolMarker(), Conv2dParams(c, r, 1), Marker(), Conv2dParams(r, c, 1), Marker())


class MBConvBlock(nn.Sequential):
    def __init__(self, cin, cout, k, stride, expand, se_ratio, drop_rate):
        ce = int(cin * expand)
        mods = []
        if expand != 1:
            mods += [Conv2dParams(cin, ce, 1, bias=False), BatchNorm2dParams(ce), Marker()]
        mods += [Conv2dParams(ce, ce, k, stride, groups=ce, bias=False), BatchNorm2dParams(ce), Marker(),
                 SELayer(ce, max(1, int(cin * se_ratio))), Conv2dParams(ce, cout, 1, bias=False), BatchNorm2dParams(cout)]
        if cin == cout and stride == 1:
            mods += [DropMarker(drop_rate)]
        super().__init__(*mods)
        self.cfg = dict(cin=cin, cout=cout, ce=ce, k=k, stride=stride, expand=expand, skip=(cin == cout and stride == 1))


class MBConvBlockRepeat(nn.Sequential):
    def __init__(self, n, cin, cout, k, stride, expand, se_ratio, drop):
        mods = []
        for i in range(n):
            mods.append(MBConvBlock(cin, cout, k, stride, expand, se_ratio, drop * i / n))
            cin, stride = cout, 1
        super().__init__(*mods)


def _round_filters(f, width, div=8):
    new = max(div, int(f * width + div / 2) // div * div)
    if new < 0.9 * f * width:
        new += div
    return int(new)


def same_pad(h_in, k, stride):
    """PaddedConv2d (:53-64): symmetric ceil(total/2)."""
    h_out = math.ceil(h_in / stride)
    return math.ceil(max((h_out - 1) * stride - h_in + (k - 1) + 1, 0) / 2)


class _Engine(FusedEngine):
    # forward / _backward are drivers over per-block methods (stem, MBConv block, head), as in the DenseNet and ResNet engines
    # (fp32 storage: generic f32-MFMA convolutions, the storage-typed depthwise / squeeze-excite / Swish kernels of csrc/effnet.hip,
    # no tiled fast paths; one owner per squeeze-excite sum)
    def __init__(self, model):
        super().__init__(model)
        self.mb = [b for rep in model.blocks for b in rep]
        self.mb_names = ["blocks.%d.%d" % (si, bi) for si, rep in enumerate(model.blocks) for bi, _ in enumerate(rep)]
        self.last_masks = {}         # name -> mask / keep of the most recent train-mode forward (tests, reproducibility)
        self.n_forward = 0           # forwards so far (ws.step)
        self.step_dev = None         # device-side count of the training forwards: what the Dropout / DropConnect masks are drawn from
        self.bns = [model.stem[1]] + [m for b in self.mb for m in b if isinstance(m, nn.BatchNorm2d)] + [model.head[1]]
        self.bn, rest = _BN.plan(self.bns)
        self.ones = rest.take(max(bn.num_features for bn in self.bns))
        self.vec_size = rest.n

    # ---- binding
    def bind(self, dev):
        if self.bound(dev):
            return
        m = self.model
        self.bind_params(dev)
        self.n_classes = m.head[6].out_features
        # (the 3-channel stem is padded to 8 input channels and packed by _pack_stem8)
        self.plan_packing([mod for b in self.mb + [m.head] for mod in b if isinstance(mod, nn.Conv2d) and mod.groups == 1],
                          stem8=m.stem[0])

    def _pack_stem8(self):
        w8 = F.pad(self.model.stem[0].weight.detach(), (0, 0, 0, 0, 0, 5)).contiguous()       # (O,3,3,3) -> (O,8,3,3)
        if self.dtype == torch.float32:         # [tap][O][I] fp32: a 3 K-element layout copy
            self.packed[self.stem_off:self.stem_off + w8.numel()].copy_(w8.permute(2, 3, 0, 1).reshape(-1))
        else:
            ops.pack_weights(w8, out=self.packed[self.stem_off:])

    # ---- workspace
    def _new_workspace(self, B, H, W):
        dev, bf, f32 = self.device, self.dtype, torch.float32
        e = lambda *s, dtype=bf: torch.empty(*s, dtype=dtype, device=dev)
        m = self.model
        ws = type("WS", (), {})()
        ws.key, ws.B, ws.H, ws.W = (B, H, W), B, H, W
        ws.x8 = e(B, H, W, 8)
        p0 = same_pad(H, 3, 2)
        h, w = (H + 2 * p0 - 3) // 2 + 1, (W + 2 * same_pad(W, 3, 2) - 3) // 2 + 1
        c0 = m.stem[0].out_channels
        ws.stem_pad = p0
        ws.ys, ws.x0 = e(B, h, w, c0), e(B, h, w, c0)
        ws.blk = []
        for b in self.mb:
            c = b.cfg
            pd = same_pad(h, c["k"], c["stride"])
            ho, wo = (h + 2 * pd - c["k"]) // c["stride"] + 1, (w + 2 * pd - c["k"]) // c["stride"] + 1
            se = [mod for mod in b if isinstance(mod, SELayer)][0]
            R = se[1].out_channels
            t = dict(hin=(h, w), hout=(ho, wo), pad=pd, R=R,
                     ye=e(B, h, w, c["ce"]) if c["expand"] != 1 else None, yd=e(B, ho, wo, c["ce"]), u=e(B, ho, wo, c["ce"]),
                     yp=e(B, ho, wo, c["cout"]), out=e(B, ho, wo, c["cout"]),
                     pooled=e(B, c["ce"], dtype=f32), h1=e(B, R, dtype=f32), s=e(B, c["ce"], dtype=f32))
            ws.blk.append(t)
            h, w = ho, wo
        ws.yh = e(B, h, w, 1280)
        ws.hw_last = (h, w)
        ws.pooled = e(B, 1280, dtype=f32)
        ws.logits = e(B, self.n_classes, dtype=f32)
        ws.vec = torch.zeros(self.vec_size, dtype=f32, device=dev)
        ws.slab = torch.empty(2, self.SLAB, dtype=f32, device=dev)
        o, n = self.ones
        ws.vec[o:o + n].fill_(1.0)
        ws.bwd = ws.dw8 = None
        return ws

    SLAB = 1 << 22               # floats per half of the statistic-row scratch
    ROWS = 2048                  # most statistic rows an element-wise / depthwise producer writes

    @staticmethod
    def _parts(b):
        mods = list(b)
        i = 0
        conv_e = bn_e = None
        if b.cfg["expand"] != 1:
            conv_e, bn_e = mods[0], mods[1]
            i = 3
        return conv_e, bn_e, mods[i], mods[i + 1], mods[i + 3], mods[i + 4], mods[i + 5]      # dw, bn_d, se, conv_p, bn_p

    # ---- statistics plumbing: every producer of a BatchNorm's sums writes one row per workgroup into ws.slab[0] / ws.slab[1], at
    # the pitch of the BatchNorm's width, and returns the number of rows; the coefficient kernel that follows (_bn_coef, _bn_bwd)
    # sums them in row order.  Named as in the ResNet engine: keywords of a convolution producer (_sp), (S1, S2, stat_rows) of an
    # element-wise / depthwise producer (_ew).  Between a coefficient launch and the next producer ws.slab[0] is free: the
    # squeeze-excite and pooling kernels keep the split rows of their per-(image, channel) sums there
    def _sp(self, ws, S):
        """Statistics keywords of a convolution that produces BatchNorm S's forward sums (none in an eval forward)."""
        if ws.frozen:
            return dict(stat_sum=None, stat_sq=None)
        return dict(stat_sum=ws.slab[0], stat_sq=ws.slab[1], stat_det=True, stat_replicas=self.SLAB // S.C, stat_rstride=S.C)

    def _ew(self, ws, S, bwd=False):
        """Where an element-wise / depthwise producer leaves BatchNorm S's forward sums (nowhere in an eval forward) or, with `bwd`,
        its backward sums S1 / S2."""
        if ws.frozen and not bwd:
            return None, None, 0
        return ws.slab[0], ws.slab[1], min(self.ROWS, self.SLAB // S.C)

    def _pro_bnbwd(self, ws, y, S):
        """input gradient: BatchNorm S's backward of the gradient operand, dY = dz * pa + y * pb + pc"""
        return dict(prologue=ops.PRO_AFFINE2, x2=y, pa=self._v(ws, S.pa), pb=self._v(ws, S.pb), pc=self._v(ws, S.pc))

    def _g_bnbwd(self, ws, y, S):
        """weight gradient: the same of its gradient operand"""
        return dict(g_prologue=ops.PRO_AFFINE2, g2=y, ga=self._v(ws, S.pa), gb=self._v(ws, S.pb), gc=self._v(ws, S.pc))

    # ---- forward
    def forward(self, x, train, record=False):
        """train: batch statistics, Dropout / DropConnect; eval: running statistics, no masks.  Every forward keeps what backward
        reads (activations and squeeze-excite intermediates), so `record` changes nothing here."""
        u8 = x.dtype == torch.uint8             # decoded grey bytes (B,1,H,W): whitened + expanded on the GPU (cx_u8_to_nhwc8)
        if x.dim() != 4 or x.shape[1] != (1 if u8 else 3):
            raise RuntimeError("expected a (B,3,H,W) float input or a (B,1,H,W) uint8 image")
        B, _, H, W = x.shape
        self.bind(x.device)
        self.pack(train or record)          # (a step that differentiates repacks, as training does: a fused optimiser bumps no version)
        ws = self.acquire(B, H, W)
        self.recorded(ws, train, True)
        self.last_masks = {}
        self.n_forward += 1
        ws.step = self.n_forward
        if train:
            # the masks' step counter lives in device memory and is bumped by a kernel: a captured step (graph.py) draws new
            # Dropout / DropConnect masks at every replay, and the eager step draws the same ones
            if self.step_dev is None or self.step_dev.device != x.device:
                self.step_dev = torch.zeros(1, dtype=torch.int64, device=x.device)
            ops.counter_add(self.step_dev)
        if u8:
            ops.u8_to_nhwc8(x.contiguous(), ws.x8)
        else:
            ops.nchw3_to_nhwc8(x.contiguous().float(), ws.x8)
        xin = self._stem_forward(ws, train)
        for bi in range(len(self.mb)):
            xin = self._mbconv_forward(ws, bi, xin, train)
        self._head_forward(ws, xin, train)
        if train and self.track_stats:
            self.model._nbt_pending += 1
        return ws

    def _stem_forward(self, ws, train):
        """3x3 stride-2 convolution of the 8-channel image, BatchNorm, Swish"""
        m, v = self.model, self._v
        S0, c0 = self.bn[id(m.stem[1])], m.stem[0].out_channels
        rows = ops.conv_gemm(ws.x8, self.packed[self.stem_off:], ws.ys, N=c0, kh=3, kw=3, stride=2, pad=ws.stem_pad, **self._sp(ws, S0))
        self._bn_coef(ws, m.stem[1], ws.ys.numel() // c0, train, rows)
        ops.scale_act_bc(ws.ys, v(ws, S0.sc), v(ws, S0.sh), None, ws.x0)
        return ws.x0

    def _mbconv_forward(self, ws, bi, xin, train):
        """efficientnet.py:76-110: expand 1x1 (unless expand_ratio == 1), depthwise k x k with the expansion's BatchNorm + Swish
        applied on load, squeeze-excite, project 1x1, BatchNorm (+ DropConnect-ed skip).  Returns the block's output."""
        b, t, v = self.mb[bi], ws.blk[bi], self._v
        c, cnt = b.cfg, ws.B * t["hout"][0] * t["hout"][1]
        conv_e, bn_e, dw, bn_d, se, conv_p, bn_p = self._parts(b)
        Sd, Sp = self.bn[id(bn_d)], self.bn[id(bn_p)]
        xdw, sc, sh = xin, None, None
        if conv_e is not None:
            Se = self.bn[id(bn_e)]
            rows = ops.conv_gemm(xin, self.w_fwd(conv_e), t["ye"], N=c["ce"], **self._sp(ws, Se))
            self._bn_coef(ws, bn_e, ws.B * t["hin"][0] * t["hin"][1], train, rows)
            xdw, sc, sh = t["ye"], v(ws, Se.sc), v(ws, Se.sh)
        s1, s2, cap = self._ew(ws, Sd)
        rows = ops.dwconv_fwd(xdw, dw.weight, sc, sh, t["yd"], s1, s2, k=c["k"], stride=c["stride"], pad=t["pad"], stat_rows=cap)
        self._bn_coef(ws, bn_d, cnt, train, rows)
        # squeeze + excite (efficientnet.py:69-73) in two launches: the excitation kernel adds the pool's split rows itself
        sc, sh = v(ws, Sd.sc), v(ws, Sd.sh)
        ops.gap_se_fwd(t["yd"], sc, sh, t["pooled"], se[1].weight, se[1].bias, se[3].weight, se[3].bias, t["h1"], t["s"], rows=ws.slab[0])
        ops.scale_act_bc(t["yd"], sc, sh, t["s"], t["u"])
        rows = ops.conv_gemm(t["u"], self.w_fwd(conv_p), t["yp"], N=c["cout"], **self._sp(ws, Sp))
        self._bn_coef(ws, bn_p, cnt, train, rows)
        # DropConnect (efficientnet.py:44-51, :100-101): train mode only, on blocks with a skip; the per-image mask / keep
        # probability is drawn by cx_dropout_mask_dev from the model's step counter (reproducible, independent of torch's RNG)
        last = list(b)[-1]
        p_dc = last.p if (train and c["skip"] and isinstance(last, DropMarker)) else 0.0
        t["dc"] = None
        if p_dc > 0.0:
            t["dc"] = torch.empty(ws.B, dtype=torch.float32, device=self.device)
            ops.dropout_mask_dev(t["dc"], 1.0 - p_dc, self._seed_base(bi), self.step_dev)
            self.last_masks[self.mb_names[bi]] = t["dc"]
        ops.affine2_out(t["yp"], xin if c["skip"] else None, v(ws, Sp.sc), v(ws, self.ones), v(ws, Sp.sh), t["dc"], t["out"])
        return t["out"]

    def _head_forward(self, ws, xin, train):
        """1x1 convolution to 1280 channels, BatchNorm, the Dropout mask, then the shared head behind Swish"""
        m, v, B = self.model, self._v, ws.B
        Sh = self.bn[id(m.head[1])]
        rows = ops.conv_gemm(xin, self.w_fwd(m.head[0]), ws.yh, N=1280, **self._sp(ws, Sh))
        self._bn_coef(ws, m.head[1], B * ws.hw_last[0] * ws.hw_last[1], train, rows)
        # Dropout in front of the classifier (efficientnet.py:169-171), train mode only: the mask is drawn here, the shared head
        # (FusedEngine._head_fwd) applies it
        p_do = m.head[5].p if train else 0.0
        mask = None
        if p_do > 0.0:
            mask = torch.empty(B, 1280, dtype=torch.float32, device=self.device)
            ops.dropout_mask_dev(mask, 1.0 - p_do, self._seed_base(len(self.mb)), self.step_dev)
            self.last_masks["head"] = mask
        self._head_fwd(ws, ws.yh, v(ws, Sh.sc), v(ws, Sh.sh), m.head[6], ops.POOL_ACT_SWISH, mask, rows=ws.slab[0])

    def _seed_base(self, idx):
        """Host part of the 64-bit seed of the mask of block `idx`: (model seed, block); the kernel adds the device-side count of
        training forwards * 1000003."""
        return (int(self.model.drop_seed) * 0x9E3779B1 + idx * 7919 + 12345) & 0xFFFFFFFFFFFFFFFF

    # ---- backward
    def _alloc_bwd(self, ws):
        if ws.bwd is not None:
            return
        dev, bf, B = self.device, self.dtype, ws.B
        bw = {"g": []}
        shapes = {}
        for t in ws.blk:
            sh = tuple(t["out"].shape)
            if sh not in shapes:
                shapes[sh] = torch.empty(sh, dtype=bf, device=dev)
            bw["g"].append(shapes[sh])
        bw["g0"] = torch.empty_like(ws.x0)
        bw["du"] = torch.empty(max(t["u"].numel() for t in ws.blk), dtype=bf, device=dev)
        bw["dzd"] = torch.empty_like(bw["du"])
        bw["dze"] = torch.empty(max([t["ye"].numel() for t in ws.blk if t["ye"] is not None] + [ws.yh.numel(), ws.ys.numel()]),
                                dtype=bf, device=dev)
        bw["gdc"] = torch.empty(max(t["out"].numel() for t in ws.blk), dtype=bf, device=dev)     # DropConnect-masked gradient
        ws.bwd = bw

    def _backward(self, ws, dlogits, dx, done):
        self._alloc_bwd(ws)
        g = self._head_backward(ws, dlogits, done)
        for bi in range(len(self.mb) - 1, -1, -1):
            g = self._mbconv_backward(ws, bi, g, done)
        self._stem_backward(ws, g, dx)

    def _head_backward(self, ws, dlogits, done):
        """Returns the gradient of the last block's output."""
        m, v, G, B = self.model, self._v, self.grad_of, ws.B
        Sh = self.bn[id(m.head[1])]
        dzh = ws.bwd["dze"][:ws.yh.numel()].view(ws.yh.shape)
        rows = self._head_bwd(ws, dlogits, ws.yh, v(ws, Sh.sc), v(ws, Sh.sh), v(ws, Sh.mean), v(ws, Sh.rstd), v(ws, self.ones, 1280), dzh,
                              *self._ew(ws, Sh, bwd=True), m.head[6], ops.POOL_ACT_SWISH, ws.drop, done)
        self._bn_bwd(ws, m.head[1], rows, B * ws.hw_last[0] * ws.hw_last[1])
        g, xlast = ws.bwd["g"][-1], ws.blk[-1]["out"]
        ops.conv_gemm(dzh, self.w_bwd(m.head[0]), g, N=xlast.shape[3], **self._pro_bnbwd(ws, ws.yh, Sh))
        ops.conv_wgrad(dzh, xlast, G(m.head[0].weight), **self._g_bnbwd(ws, ws.yh, Sh))
        done(m.head[0].weight)
        return g

    def _mbconv_backward(self, ws, bi, g, done):
        """Backward of block bi from the gradient g of its output.  Returns the gradient of its input."""
        b, t, bw, v, G, B = self.mb[bi], ws.blk[bi], ws.bwd, self._v, self.grad_of, ws.B
        c, ce = b.cfg, b.cfg["ce"]
        conv_e, bn_e, dw, bn_d, se, conv_p, bn_p = self._parts(b)
        (hi, wi), (ho, wo) = t["hin"], t["hout"]
        Sd, Sp = self.bn[id(bn_d)], self.bn[id(bn_p)]
        xin = ws.blk[bi - 1]["out"] if bi > 0 else ws.x0
        gin = g if c["skip"] else (bw["g"][bi - 1] if bi > 0 else bw["g0"])       # skip: dx accumulates into g itself
        if t.get("dc") is not None:               # the skip path takes g as it is, the branch sees it through the DropConnect mask
            gb = bw["gdc"][:g.numel()].view(g.shape)
            ops.scale_rows(g, t["dc"], gb)
            g = gb
        rows = ops.bn_lin_bwd_stats(g, t["yp"], v(ws, Sp.mean), v(ws, Sp.rstd), *self._ew(ws, Sp, bwd=True))
        self._bn_bwd(ws, bn_p, rows, B * ho * wo)
        du = bw["du"][:B * ho * wo * ce].view(B, ho, wo, ce)
        dzd = bw["dzd"][:B * ho * wo * ce].view(B, ho, wo, ce)
        ops.conv_gemm(g, self.w_bwd(conv_p), du, N=ce, **self._pro_bnbwd(ws, t["yp"], Sp))
        ops.conv_wgrad(g, t["u"], G(conv_p.weight), **self._g_bnbwd(ws, t["yp"], Sp))
        self._se_backward(ws, bi, du, dzd)
        dY = (dzd, t["yd"], v(ws, Sd.pa), v(ws, Sd.pb), v(ws, Sd.pc))           # gradient of the depthwise output: pa*dzd + pb*yd + pc
        geo = dict(k=c["k"], stride=c["stride"], pad=t["pad"])
        if conv_e is not None:
            Se = self.bn[id(bn_e)]
            dze = bw["dze"][:B * hi * wi * ce].view(B, hi, wi, ce)
            s1, s2, cap = self._ew(ws, Se, bwd=True)
            rows = ops.dwconv_dgrad(*dY, dw.weight, t["ye"], v(ws, Se.sc), v(ws, Se.sh), v(ws, Se.mean), v(ws, Se.rstd), dze, s1, s2,
                                    stat_rows=cap, **geo)
            self._bn_bwd(ws, bn_e, rows, B * hi * wi)       # (before the next producer re-uses the statistic rows)
            ops.dwconv_wgrad(*dY, t["ye"], v(ws, Se.sc), v(ws, Se.sh), G(dw.weight), **geo)
            ops.conv_gemm(dze, self.w_bwd(conv_e), gin, N=c["cin"], accumulate=c["skip"], **self._pro_bnbwd(ws, t["ye"], Se))
            ops.conv_wgrad(dze, xin, G(conv_e.weight), **self._g_bnbwd(ws, t["ye"], Se))
        else:                                     # expand_ratio == 1: the depthwise convolution reads the block input itself
            ops.dwconv_dgrad(*dY, dw.weight, xin, None, None, None, None, gin, None, None, accumulate=c["skip"], **geo)
            ops.dwconv_wgrad(*dY, xin, None, None, G(dw.weight), **geo)
        done(list(b.parameters())[0])
        return gin

    def _se_backward(self, ws, bi, du, dzd):
        """From du, the gradient of u = swish(bn(yd)) * s: the squeeze-excite backward (efficientnet.py:69-73) and dzd, the gradient
        of bn_d's output, with bn_d's coefficients.  ds[b][c] = sum_hw du * swish(bn(yd)) and the two FCs' backward are one call: the
        reduce kernel's split rows go straight into the first FC pass (cx_se_bwd_fused: no launch of their own)."""
        t, v, G = ws.blk[bi], self._v, self.grad_of
        _, _, _, bn_d, se, _, _ = self._parts(self.mb[bi])
        Sd = self.bn[id(bn_d)]
        B, ho, wo, ce = du.shape
        sc, sh = v(ws, Sd.sc), v(ws, Sd.sh)
        ds = torch.empty(B, ce, dtype=torch.float32, device=self.device)
        dpl = torch.empty(B, ce, dtype=torch.float32, device=self.device)
        ops.se_bwd_fused(du, t["yd"], sc, sh, ds, t["s"], t["h1"], t["pooled"], se[1].weight, se[3].weight, G(se[1].weight),
                         G(se[1].bias), G(se[3].weight), G(se[3].bias), dpl, rows=ws.slab[0])
        rows = ops.se_act_bwd(du, t["yd"], sc, sh, v(ws, Sd.mean), v(ws, Sd.rstd), t["s"], dpl, dzd, *self._ew(ws, Sd, bwd=True))
        self._bn_bwd(ws, bn_d, rows, B * ho * wo)

    def _stem_backward(self, ws, g, dx):
        """x0 = swish(bn(ys)) from its gradient g; the stem's weight gradient and, into dx when given, the input gradient"""
        m, v, G = self.model, self._v, self.grad_of
        S0, c0 = self.bn[id(m.stem[1])], m.stem[0].out_channels
        dzs = ws.bwd["dze"][:ws.ys.numel()].view(ws.ys.shape)
        rows = ops.se_act_bwd(g, ws.ys, v(ws, S0.sc), v(ws, S0.sh), v(ws, S0.mean), v(ws, S0.rstd), None, None, dzs,
                              *self._ew(ws, S0, bwd=True))
        self._bn_bwd(ws, m.stem[1], rows, ws.ys.numel() // c0)
        # (persistent: its address is part of the deferred slab-sum table, which must not change from step to step)
        if ws.dw8 is None:
            ws.dw8 = torch.empty(c0, 8, 3, 3, dtype=torch.float32, device=self.device)
        dw8 = ws.dw8.zero_()
        ops.conv_wgrad(dzs, ws.x8, dw8, kh=3, kw=3, stride=2, pad=ws.stem_pad, **self._g_bnbwd(ws, ws.ys, S0))
        ops.wgrad_defer_flush(self.device)       # the stem gradient is read back right here: run the deferred slab sums now
        G(m.stem[0].weight).view(c0, 3, 3, 3).add_(dw8[:, :3])
        if dx is not None:
            ops.stem_input_grad(dzs, ws.ys, v(ws, S0.pa), v(ws, S0.pb), v(ws, S0.pc), m.stem[0].weight, dx, stride=2, pad=ws.stem_pad)


class EfficientNet(FusedNet):
    def __init__(self, model_name, n_classes):
        super().__init__()
        assert model_name in SCALING_PARAMS.keys(), "Invalid model name."
        width, depth, _, dropout = SCALING_PARAMS[model_name]
        c_stem = _round_filters(32, width)
        self.stem = nn.Sequential(Conv2dParams(3, c_stem, 3, 2, bias=False), BatchNorm2dParams(c_stem), Marker())
        reps = []
        for (n, cin, cout, k, s, e) in _BASE:
            reps.append(MBConvBlockRepeat(int(math.ceil(depth * n)), _round_filters(cin, width), _round_filters(cout, width), k, s, e,
                                          0.25, 0.2))
        self.blocks = nn.Sequential(*reps)
        self.head = nn.Sequential(Conv2dParams(_round_filters(320, width), 1280, 1, bias=False), BatchNorm2dParams(1280), Marker(),
                                  PoolMarker(), Marker(), DropMarker(dropout), nn.Linear(1280, n_classes))
        for mod in self.modules():                                   # reset_parameters (:171-183)
            if isinstance(mod, nn.BatchNorm2d):
                mod.eps, mod.momentum = 1e-3, 0.01
            if isinstance(mod, nn.Conv2d):
                nn.init.kaiming_normal_(mod.weight, mode="fan_out", nonlinearity="conv2d")
                if mod.bias is not None:
                    nn.init.constant_(mod.bias, 0)
            if isinstance(mod, nn.Linear):
                nn.init.kaiming_uniform_(mod.weight, a=math.sqrt(5), mode="fan_in", nonlinearity="linear")
                nn.init.constant_(mod.bias, 0)
        self.drop_seed = 0           # seed of the Dropout / DropConnect masks (with the forward counter and the block index)

    def _eng(self):
        if self._engine is None or self._engine.dtype != getattr(self, "_storage_dtype", torch.bfloat16):
            object.__setattr__(self, "_engine", _Engine(self))
        return self._engine

    def _anchor(self):
        return self.head[6].weight


def construct_model(model_name, n_classes):
    """efficientnet.py:188-228: compound scaling of the B0 definition; the instance's class is named after the model."""
    assert model_name in SCALING_PARAMS.keys(), "Invalid model name."
    cls = type(model_name, (EfficientNet,), {})
    return cls(model_name, n_classes)
