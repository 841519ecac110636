"""Bottleneck / BasicBlock ResNet (torchvision-shaped; resnet152 = layers [3, 8, 36, 3]) and the WideResNet of the CIFAR
harness on the gfx950 kernels.

Drop-in surface: constructor signature of /root/reference/models/attn_aug_conv.py:218-220, `Bottleneck` with
stride on conv2 (:159-211), torchvision `state_dict` keys (`conv1`, `bn1`, `layerL.i.{conv1,bn1,conv2,bn2,
conv3,bn3,downsample.0,downsample.1}`, `fc`), `model.layer4`, re-assignable `model.fc`.

Schedule per bottleneck (NHWC bf16, fp32 accumulate / statistics):
  conv1 1x1 (raw, stats)  ->  conv2 3x3 stride s with bn1+ReLU in the operand prologue (raw, stats)
  ->  conv3 1x1 with bn2+ReLU in the prologue (raw, stats)  [-> downsample 1x1 stride s (raw, stats)]
  ->  one residual-join kernel out = relu(bn3(y3) + bn_d(yd) | x).
BatchNorm outputs are never stored; backward uses the two-tensor affine form of BN backward in the
prologues of the input- and weight-gradient kernels, and the input gradient of the strided convs is the
same implicit GEMM walking only the source positions that lie on the stride grid (`tstride`).
"""
import os

import torch
import torch.nn as nn

from .. import ops
from .._lib import check, lib, ptr, stream_ptr
from ._fused import FusedEngine, FusedNet, _BN
from .densenet import AAConv2d, BatchNorm2dParams, Conv2dParams, PoolMarker, ReLUMarker


class Bottleneck(nn.Module):
    expansion = 4

    def __init__(self, inplanes, planes, stride=1, downsample=None, groups=1, base_width=64, dilation=1, norm_layer=None,
                 input_dims=None, attn_params=None):
        super().__init__()
        if norm_layer not in (None, nn.BatchNorm2d):
            raise NotImplementedError("other norm layers than BatchNorm2d are not built")
        if (dilation != 1 or groups != 1) and attn_params is not None:
            raise NotImplementedError("a dilated or grouped AAConv2d is not built (the reference's AA networks have neither)")
        width = int(planes * (base_width / 64.)) * groups         # attn_aug_conv.py:168 (wide_resnet*_2: base_width 128)
        if groups != 1 and (width // groups) % 8:
            # a grouped 3x3 runs as one launch per group on channel slices of the NHWC tensors (the kernels take channel counts
            # that are multiples of 8): resnext101_32x8d and wider fit, resnext50_32x4d's first stage (4 channels per group) does not
            raise NotImplementedError("grouped 3x3 convolutions need a multiple of 8 channels per group (got %d)" % (width // groups))
        self.conv1 = Conv2dParams(inplanes, width, 1, bias=False)
        self.bn1 = BatchNorm2dParams(width)
        if attn_params is None:
            # torchvision conv3x3(width, width, stride, groups, dilation): padding = dilation (attn_aug_conv.py:183)
            self.conv2 = Conv2dParams(width, width, 3, stride, dilation, dilation=dilation, groups=groups, bias=False)
        else:                                   # attn_aug_conv.py:170-183: AAConv2d(width, width, 3, stride, dk, dv, nh, ...)
            nh = attn_params["nh"]
            dk = max(20 * nh, int((attn_params["k"] * width // nh) * nh))
            dv = int((attn_params["v"] * width // nh) * nh)
            dims = (int(attn_params["input_dims"][0] * 16 / planes), int(attn_params["input_dims"][1] * 16 / planes))
            self.conv2 = AAConv2d(width, width, 3, stride, dk, dv, nh, attn_params["relative"], dims)
        self.bn2 = BatchNorm2dParams(width)
        self.conv3 = Conv2dParams(width, planes * 4, 1, bias=False)
        self.bn3 = BatchNorm2dParams(planes * 4)
        self.relu = ReLUMarker(inplace=True)
        self.downsample = downsample
        self.stride = stride

    def forward(self, x):  # pragma: no cover - guard
        raise RuntimeError("chexpert_amd: call the parent ResNet (fused HIP schedule)")


class BasicBlock(nn.Module):
    """Signature and parameters of /root/reference/models/attn_aug_conv.py:107-156 (two 3x3 convolutions; AAConv2d replaces
    conv1 in layers 2-4).  The reference uses it in the CIFAR harness (models/test_model.py).  On the HIP schedule: conv3x3 (or the
    AAConv2d conv branch || attention) raw + stats -> conv3x3 with bn1+ReLU in the prologue -> residual-join kernel."""
    expansion = 1

    def __init__(self, inplanes, planes, stride=1, downsample=None, groups=1, base_width=64, dilation=1, norm_layer=None,
                 input_dims=None, attn_params=None):
        super().__init__()
        if groups != 1 or base_width != 64:
            raise ValueError("BasicBlock only supports groups=1 and base_width=64")
        if dilation > 1:
            raise NotImplementedError("Dilation > 1 not supported in BasicBlock")
        if attn_params is None:
            self.conv1 = Conv2dParams(inplanes, planes, 3, stride, 1, bias=False)
        else:
            nh = attn_params["nh"]
            dk = max(20 * nh, int((attn_params["k"] * planes // nh) * nh))
            dv = int((attn_params["v"] * planes // nh) * nh)
            dims = (int(attn_params["input_dims"][0] * 16 / planes), int(attn_params["input_dims"][1] * 16 / planes))
            self.conv1 = AAConv2d(inplanes, planes, 3, stride, dk, dv, nh, attn_params["relative"], dims)
        self.bn1 = BatchNorm2dParams(planes)
        self.relu = ReLUMarker(inplace=True)
        self.conv2 = Conv2dParams(planes, planes, 3, 1, 1, bias=False)
        self.bn2 = BatchNorm2dParams(planes)
        self.downsample = downsample
        self.stride = stride

    def forward(self, x):  # pragma: no cover - guard
        raise RuntimeError("chexpert_amd: call the parent ResNet / WideResNet (fused HIP schedule)")


class _Engine(FusedEngine):
    SLAB = 1 << 22               # floats per statistic-row scratch (rows x channels of the largest producer)
    EW_ROWS = 2048

    def __init__(self, model):
        super().__init__(model)
        # (deterministic statistics: attention-augmented blocks feed one BatchNorm from two kernels: their statistic rows are reduced
        # per channel range, _aa_fwd; the two input-gradient branches stack their rows, _stacked)
        self.join_fuse = os.environ.get("CHEXPERT_JOIN_FUSE", "1") != "0"      # residual-join backward in the conv1 input gradient's epilogue
        # Bottleneck networks in bf16: the residual stream is kept as two planes (bf16 hi + int8 lo = 16 significant bits, common.h
        # cx_join2) and the forward join of an identity block runs in the prologue of the NEXT block's conv1 (CX_PRO_JOIN)
        self.stream_lo = os.environ.get("CHEXPERT_STREAM_LO", "1") != "0"
        self.fwd_join_fuse = os.environ.get("CHEXPERT_FWD_JOIN_FUSE", "1") != "0"
        # fp32 storage: the same schedule on fp32 tensors through the generic f32-MFMA convolutions (csrc/conv_f32.hip) and the
        # templated element-wise kernels
        if self.dtype != torch.bfloat16 and isinstance(model, WideResNet):
            raise NotImplementedError("the fp32 storage mode covers the ImageNet-stem ResNets (resnet152 / aaresnet152 of "
                                      "chexpert.py:482-494); the 3-channel CIFAR stem is packed for bf16")
        self.blocks = [blk for L in model._stages() for blk in L]
        self.basic = model.block is BasicBlock                 # two 3x3 convolutions per block (attn_aug_conv.py:107-156)
        self.two_plane = self.stream_lo and not (model.block is BasicBlock) and self.dtype == torch.bfloat16
        # Where the stream keeps its lo plane: on every output that feeds an identity join (round 5; 46 of resnet152's 50 joins --
        # the four downsample blocks' outputs start a stage and are rounded once).  Round 4 kept it only through the long stages
        # (layer2 / layer3: 42 joins) and measured 8.3e-3 on the reference fixture's train logits at 128 images; on every identity
        # join it is 6.9e-3 for +0.36 ms of the 54.2 ms step (profiles/r05_resnet_margin.txt): kept, the 1e-2 bound then has 30 %
        # of room instead of 17 %.  The FUSED form (the join in the prologue of the next conv1) stays with the long stages: it does
        # not pay on layer1 (N = 64 on a 256-wide tile) nor layer4 (MFMA-bound) -- scratch/bench_join.py.
        # keep_lo[bi]: block bi's output has a lo plane;  fuse_fwd[bi]: its join runs in the prologue of block bi + 1's conv1.
        n = len(self.blocks)
        stage_len = []
        for L in model._stages():
            stage_len += [len(L)] * len(L)
        ident = [b.downsample is None for b in self.blocks]
        long_id = [ident[i] and stage_len[i] >= 6 for i in range(n)]
        # (CHEXPERT_STREAM_LO_MIN=<blocks>: the stage length from which the lo plane is kept, for measurements -- 1 = on every identity join)
        lo_min = int(os.environ.get("CHEXPERT_STREAM_LO_MIN", "1"))
        lo_id = [ident[i] and stage_len[i] >= lo_min for i in range(n)]
        self.keep_lo = [self.two_plane and i + 1 < n and lo_id[i + 1] for i in range(n)]
        self.fuse_fwd = [self.two_plane and self.fwd_join_fuse and long_id[i] and i + 1 < n for i in range(n)]
        self.cifar = isinstance(model, WideResNet)              # 3x3 stride-1 stem, no max-pool, three stages (:311-404)
        # vector plan: [fwd-zero region | bwd-zero region | rest]
        self.bn, rest, self.fwd_zero, self.bwd_zero = _BN.plan(list(self._all_bns()))
        cmax = 2048
        self.join = [[rest.take(self._last_bn(b).num_features) for _ in range(3)] for b in self.blocks]
        self.ones, self.zeros = rest.take(cmax), rest.take(cmax)
        self.scratch = [rest.take(cmax) for _ in range(2)]
        self.vec_size = rest.n

    @staticmethod
    def _cin(b):
        c1 = b.conv1
        return c1.in_proj_qkv.in_channels if isinstance(c1, AAConv2d) else c1.in_channels

    @staticmethod
    def _last_bn(b):
        return b.bn3 if hasattr(b, "bn3") else b.bn2

    def _all_bns(self):
        m = self.model
        yield m.bn1
        for b in self.blocks:
            yield b.bn1
            yield b.bn2
            if hasattr(b, "bn3"):
                yield b.bn3
            if b.downsample is not None:
                yield b.downsample[1]

    # ---- binding / packing
    def bind(self, dev):
        if self.bound(dev):
            return
        m = self.model
        c_last = self._last_bn(self.blocks[-1]).num_features
        if m.fc.in_features != c_last:
            raise RuntimeError("fc.in_features must match the last stage (%d channels)" % c_last)
        self.bind_params(dev)
        self.n_classes = m.fc.out_features
        # (the CIFAR stem's 3 input channels are padded to 8 for the implicit GEMM: packed by _pack_stem8)
        convs = [mod for mod in m.modules() if isinstance(mod, nn.Conv2d) and mod is not m.conv1]
        if self.cifar:
            self.plan_packing(convs, stem8=m.conv1)
        else:
            self.plan_packing(convs, stem=m.conv1, stem_layout=True)

    def _pack_stem8(self):
        if self.cifar:
            w8 = torch.nn.functional.pad(self.model.conv1.weight.detach(), (0, 0, 0, 0, 0, 5)).contiguous()   # (O,3,3,3) -> (O,8,3,3)
            ops.pack_weights(w8, out=self.packed[self.stem_off:])

    # ---- workspace
    class WS:
        pass

    def _new_workspace(self, B, H, W):
        dev, bf = self.device, self.dtype
        e = lambda *s, dtype=bf: torch.empty(*s, dtype=dtype, device=dev)
        ws = _Engine.WS()
        ws.key, ws.B, ws.H, ws.W = (B, H, W), B, H, W
        if self.cifar:
            c0 = self.model.conv1.out_channels
            ws.x8 = e(B, H, W, 8)
            h, w = H, W
            ws.c0 = e(B, h, w, c0)
            ws.pool0 = e(B, h, w, c0)                  # relu(bn1(c0)): the first stage's input (no max-pool in this stem)
        else:
            ws.x4 = e(B, H, W, 4)
            h, w = H // 2, W // 2
            ws.c0 = e(B, h, w, 64)
            h, w = h // 2, w // 2
            ws.amax = e(B, h, w, 64, dtype=torch.uint8)
            ws.pool0 = e(B, h, w, 64)
        ws.blk = []
        for b in self.blocks:
            p_, s_ = b.bn1.num_features, b.stride
            o_ = self._last_bn(b).num_features            # planes * expansion (4 * width only at base_width 64)
            ho, wo = h // s_, w // s_
            if self.basic:                          # y1 = conv1 output (3x3, stride s), y2 = conv2 output, both on the block's output grid
                t = dict(hin=(h, w), hout=(ho, wo), y1=e(B, ho, wo, p_), y2=e(B, ho, wo, p_),
                         yd=e(B, ho, wo, p_) if b.downsample is not None else None, out=e(B, ho, wo, p_))
            else:
                t = dict(hin=(h, w), hout=(ho, wo), y1=e(B, h, w, p_), y2=e(B, ho, wo, p_), y3=e(B, ho, wo, o_),
                         yd=e(B, ho, wo, o_) if b.downsample is not None else None, out=e(B, ho, wo, o_))
            t["mask"] = e(t["out"].numel() // 8, dtype=torch.uint8)          # sign bits of the join output for its backward
            if self.keep_lo[len(ws.blk)]:
                t["out_lo"] = e(t["out"].numel(), dtype=torch.int8)          # lo plane of the residual stream (read by the next join only)
            aa = b.conv1 if self.basic else b.conv2         # the AAConv2d position: conv1 of a BasicBlock, conv2 of a Bottleneck
            if isinstance(aa, AAConv2d):
                if (ho, wo) != tuple(aa.input_dims):
                    raise RuntimeError("AAConv2d was built for %s feature maps, the input gives %s (relative tables are "
                                       "size-bound, attn_aug_conv.py:38-41)" % (tuple(aa.input_dims), (ho, wo)))
                t["QKV"] = e(B, ho, wo, 2 * aa.dk + aa.dv)
                t["O"] = e(B, ho * wo, aa.dv, dtype=torch.float32)
                t["LSE"] = e(B * aa.nh, ho * wo, dtype=torch.float32)
            ws.blk.append(t)
            h, w = ho, wo
        ws.pooled = torch.empty(B, self.model.fc.in_features, dtype=torch.float32, device=dev)
        ws.slab = torch.empty(3, self.SLAB, dtype=torch.float32, device=dev) if self.det else None
        ws.logits = torch.empty(B, self.n_classes, dtype=torch.float32, device=dev)
        ws.vec = torch.zeros(self.vec_size, dtype=torch.float32, device=dev)
        o, n = self.ones
        ws.vec[o:o + n].fill_(1.0)
        ws.bwd = None
        return ws

    def _sp(self, ws, S, train):
        """Statistics arguments of a producer of BatchNorm S's input."""
        if not train:
            return {}
        if self.det:
            return dict(stat_sum=ws.slab[0], stat_sq=ws.slab[1], stat_det=True, stat_replicas=self.SLAB // S.C, stat_rstride=S.C)
        return dict(stat_sum=self._v(ws, S.sum), stat_sq=self._v(ws, S.sq))

    @staticmethod
    def _stat_slice(kw, c_):
        """statistics keywords of a producer restricted to the channel range c_ of their BatchNorm (grouped convolutions): the
        vectors / row buffers start at the range's first channel, the row pitch stays the BatchNorm's width"""
        kw = dict(kw)
        for k in ("stat_sum", "stat_sq"):
            if kw.get(k) is not None:
                kw[k] = kw[k][c_.start:]
        return kw

    def _bn_coef(self, ws, bn, count, train, rows=None):
        S, v = self.bn[id(bn)], self._v
        if train:
            mom = bn.momentum if bn.momentum is not None else 0.1
            ssum, ssq, reps, rstride = (ws.slab[0], ws.slab[1], rows, S.C) if self.det else (v(ws, S.sum), v(ws, S.sq), 1, 0)
            ops.bn_coef(ssum, ssq, count, bn.weight, bn.bias, bn.eps, mom, bn.running_mean, bn.running_var,
                        v(ws, S.sc), v(ws, S.sh), v(ws, S.mean), v(ws, S.rstd), S.C, replicas=reps, rstride=rstride)
        else:
            ops.bn_coef_eval(bn.running_mean, bn.running_var, bn.weight, bn.bias, bn.eps, v(ws, S.sc), v(ws, S.sh), v(ws, S.mean),
                             v(ws, S.rstd), S.C)

    def _bn_coef_part(self, ws, bn, count, rows, lo, n):
        """_bn_coef for channels [lo, lo + n) of `bn` from `rows` statistic rows of pitch n (deterministic mode: an AAConv2d's
        conv branch and its attention out-projection each produce the rows of their own channel range)."""
        S, v = self.bn[id(bn)], self._v
        mom = bn.momentum if bn.momentum is not None else 0.1
        c = lambda t_: t_[lo:lo + n]
        ops.bn_coef(ws.slab[0], ws.slab[1], count, c(bn.weight), c(bn.bias), bn.eps, mom, c(bn.running_mean), c(bn.running_var),
                    c(v(ws, S.sc)), c(v(ws, S.sh)), c(v(ws, S.mean)), c(v(ws, S.rstd)), n, replicas=rows, rstride=n)

    def _aa_fwd(self, ws, aa, xin, yout, qkv_t, bn, S, stride, count, train, pro):
        """AAConv2d forward (attn_aug_conv.py:65-97) into `yout` = [conv branch | attention], with the statistics of the BatchNorm
        that follows.  Returns True when the coefficients of `bn` have been computed here (deterministic training mode)."""
        v = self._v
        p_ = yout.shape[3]
        cc = p_ - aa.dv
        det = train and self.det
        sub = lambda slot, lo, n: None if slot is None else slot[lo:lo + n]
        st = (lambda s_: v(ws, s_)) if train else (lambda s_: None)
        if det:
            rows = ops.conv_gemm(xin, self.w_fwd(aa.conv), yout[..., :cc], N=cc, kh=3, kw=3, stride=stride, pad=1, stat_sum=ws.slab[0],
                                 stat_sq=ws.slab[1], stat_det=True, stat_replicas=self.SLAB // cc, stat_rstride=cc, **pro)
            self._bn_coef_part(ws, bn, count, rows, 0, cc)
        else:
            ops.conv_gemm(xin, self.w_fwd(aa.conv), yout[..., :cc], N=cc, kh=3, kw=3, stride=stride, pad=1,
                          stat_sum=sub(st(S.sum), 0, cc), stat_sq=sub(st(S.sq), 0, cc), **pro)
        ops.conv_gemm(xin, self.w_fwd(aa.in_proj_qkv), qkv_t["QKV"], N=2 * aa.dk + aa.dv, stride=stride, **pro)
        ops.aa_attention_fwd(qkv_t["QKV"], *aa.rel_tables(), qkv_t["O"], qkv_t["LSE"], aa.nh, aa.dk, aa.dv)
        object.__setattr__(aa, "_last", (qkv_t["QKV"], qkv_t["LSE"]))
        if det:
            rows = ops.aa_outproj_fwd(qkv_t["O"], aa.out_proj.weight, yout[..., cc:], ws.slab[0], ws.slab[1],
                                      stat_rows=min(self.EW_ROWS, self.SLAB // aa.dv), stat_rstride=aa.dv)
            self._bn_coef_part(ws, bn, count, rows, cc, aa.dv)
            return True
        ops.aa_outproj_fwd(qkv_t["O"], aa.out_proj.weight, yout[..., cc:], sub(st(S.sum), cc, aa.dv), sub(st(S.sq), cc, aa.dv))
        return False

    def _stacked(self, ws, kw, rows, C):
        """Mask-epilogue arguments for a SECOND producer of the same backward sums (deterministic mode): its statistic rows go
        behind the `rows` rows of the first one, so one reduction over rows + rows2 adds both."""
        if not self.det:
            return kw
        kw = dict(kw)
        kw.update(stat_sum=ws.slab[0][rows * C:], stat_sq=ws.slab[1][rows * C:], stat_replicas=self.SLAB // C - rows)
        return kw

    # ---- forward
    def forward(self, x, train, record=False):
        """train: batch statistics (and running-statistic updates); eval: running statistics.  record (eval): also keep what
        backward reads -- the join ReLU sign bits, which an eval forward without a backward skips."""
        m, v = self.model, self._v
        u8 = x.dtype == torch.uint8             # decoded grey bytes (B,1,H,W): whitened + expanded on the GPU (cx_u8_to_nhwc4)
        if x.dim() != 4 or x.shape[1] != (1 if u8 else 3):
            raise RuntimeError("expected a (B,3,H,W) float input or a (B,1,H,W) uint8 image")
        B, _, H, W = x.shape
        mult = 4 if self.cifar else 32
        if H % mult or W % mult:
            raise RuntimeError("input height/width must be multiples of %d (got %dx%d)" % (mult, H, W))
        self.bind(x.device)
        self.pack(train or record)          # (a step that differentiates repacks, as training does: a fused optimiser bumps no version)
        ws = self.acquire(B, H, W)
        self.recorded(ws, train, record)
        if train and not self.det:
            z0, zn = self.fwd_zero
            ws.vec[z0:z0 + zn].zero_()
        st = (lambda s: v(ws, s)) if train else (lambda s: None)
        sp = lambda S_: self._sp(ws, S_, train)
        S0 = self.bn[id(m.bn1)]
        if self.cifar:
            # attn_aug_conv.py:341-343, :391-393: 3x3 stride-1 stem, BatchNorm, ReLU -- no max-pool
            if u8:
                raise RuntimeError("the CIFAR stem takes (B,3,H,W) float images")
            c0 = m.conv1.out_channels
            check(lib().cx_nchw3_to_nhwc8(ptr(x.contiguous().float()), ptr(ws.x8), B, H, W, stream_ptr()), "cx_nchw3_to_nhwc8")
            rows = ops.conv_gemm(ws.x8, self.packed[self.stem_off:], ws.c0, N=c0, kh=3, kw=3, stride=1, pad=1, **sp(S0))
            self._bn_coef(ws, m.bn1, B * H * W, train, rows)
            ops.affine2_relu(ws.c0, ws.c0, v(ws, S0.sc), v(ws, self.zeros, c0), v(ws, S0.sh), ws.pool0)
        else:
            if u8:
                ops.u8_to_nhwc4(x.contiguous(), ws.x4)
            else:
                ops.nchw3_to_nhwc4(x.contiguous().float(), ws.x4)
            rows = ops.conv_gemm(ws.x4, self.w_fwd(m.conv1), ws.c0, N=64, mode=ops.MODE_STEM, **sp(S0))
            self._bn_coef(ws, m.bn1, B * (H // 2) * (W // 2), train, rows)
            ops.bnrelu_maxpool_fwd(ws.c0, v(ws, S0.sc), v(ws, S0.sh), ws.pool0, ws.amax, None, None)
        xin, xin_lo, pending = ws.pool0, None, None
        for bi, b in enumerate(self.blocks):
            t = ws.blk[bi]
            s_, p_ = b.stride, b.bn1.num_features
            o_ = self._last_bn(b).num_features
            cin_ = self._cin(b)
            hi, wi = t["hin"]
            ho, wo = t["hout"]
            mk = t["mask"] if ws.recorded else None
            if self.basic:
                # attn_aug_conv.py:135-156: conv3x3(stride) - bn1 - relu - conv3x3 - bn2, + identity | downsample(x), relu
                S1, S2 = self.bn[id(b.bn1)], self.bn[id(b.bn2)]
                coef_done = False
                if isinstance(b.conv1, AAConv2d):
                    # attn_aug_conv.py:124-131, :65-97: the first 3x3 is attention-augmented (conv branch || attention, on the raw input)
                    coef_done = self._aa_fwd(ws, b.conv1, xin, t["y1"], t, b.bn1, S1, s_, B * ho * wo, train, {})
                    rows = None
                else:
                    rows = ops.conv_gemm(xin, self.w_fwd(b.conv1), t["y1"], N=p_, kh=3, kw=3, stride=s_, pad=1, **sp(S1))
                if not coef_done:
                    self._bn_coef(ws, b.bn1, B * ho * wo, train, rows)
                rows = ops.conv_gemm(t["y1"], self.w_fwd(b.conv2), t["y2"], N=p_, kh=3, kw=3, stride=1, pad=1,
                                     prologue=ops.PRO_AFFINE_RELU, pa=v(ws, S1.sc), pb=v(ws, S1.sh), **sp(S2))
                self._bn_coef(ws, b.bn2, B * ho * wo, train, rows)
                ja, jb, jc = (v(ws, sl) for sl in self.join[bi])
                if b.downsample is not None:
                    Sd = self.bn[id(b.downsample[1])]
                    rows = ops.conv_gemm(xin, self.w_fwd(b.downsample[0]), t["yd"], N=p_, stride=s_, **sp(Sd))
                    self._bn_coef(ws, b.downsample[1], B * ho * wo, train, rows)
                    torch.add(v(ws, S2.sh), v(ws, Sd.sh), out=jc)
                    ops.affine2_relu(t["y2"], t["yd"], v(ws, S2.sc), v(ws, Sd.sc), jc, t["out"], mk)
                else:
                    ops.affine2_relu(t["y2"], xin, v(ws, S2.sc), v(ws, self.ones, p_), v(ws, S2.sh), t["out"], mk)
                xin = t["out"]
                continue
            S1, S2, S3 = self.bn[id(b.bn1)], self.bn[id(b.bn2)], self.bn[id(b.bn3)]
            if pending is not None:
                # attn_aug_conv.py:202-211 of the block below + :188 of this one: out = relu(bn3(y3) + identity) is computed in this
                # conv1's prologue (hi plane = its operand) and leaves as hi / lo / sign-bit side outputs -- no pass of its own
                tp, Sp, mkp = pending
                rows = ops.conv_gemm(tp["y3"], self.w_fwd(b.conv1), t["y1"], N=p_, prologue=ops.PRO_JOIN, x2=tp["id_hi"], x3=tp["id_lo"],
                                     pa=v(ws, Sp.sc), pb=v(ws, self.ones, cin_), pc=v(ws, Sp.sh), pro_out=tp["out"], po_lo=tp.get("out_lo"),
                                     po_mask=mkp, **sp(S1))
                pending = None
            else:
                rows = ops.conv_gemm(xin, self.w_fwd(b.conv1), t["y1"], N=p_, **sp(S1))
            self._bn_coef(ws, b.bn1, B * hi * wi, train, rows)
            coef_done = False
            if isinstance(b.conv2, AAConv2d):
                # attn_aug_conv.py:65-97: 3x3 conv branch || multi-head attention over the stride-s grid, concatenated on channels
                coef_done = self._aa_fwd(ws, b.conv2, t["y1"], t["y2"], t, b.bn2, S2, s_, B * ho * wo, train,
                                         dict(prologue=ops.PRO_AFFINE_RELU, pa=v(ws, S1.sc), pb=v(ws, S1.sh)))
                rows = None
            else:
                d_ = b.conv2.dilation[0]              # > 1 under replace_stride_with_dilation: padding = dilation, stride 1
                gr = b.conv2.groups
                if gr == 1:
                    rows = ops.conv_gemm(t["y1"], self.w_fwd(b.conv2), t["y2"], N=p_, kh=3, kw=3, stride=s_, pad=d_, dil=d_,
                                         prologue=ops.PRO_AFFINE_RELU, pa=v(ws, S1.sc), pb=v(ws, S1.sh), **sp(S2))
                else:
                    # conv3x3(width, width, stride, groups, dilation) (attn_aug_conv.py:183): one launch per group on its channel
                    # slice of y1 / y2; the statistic rows of the groups sit side by side at the pitch of the whole BatchNorm
                    kg = p_ // gr
                    for g_ in range(gr):
                        c_ = slice(g_ * kg, (g_ + 1) * kg)
                        rows = ops.conv_gemm(t["y1"][..., c_], self.w_fwd(b.conv2, g_), t["y2"][..., c_], N=kg, kh=3, kw=3, stride=s_,
                                             pad=d_, dil=d_, prologue=ops.PRO_AFFINE_RELU, pa=v(ws, S1.sc)[c_], pb=v(ws, S1.sh)[c_],
                                             **self._stat_slice(sp(S2), c_))
            if not coef_done:
                self._bn_coef(ws, b.bn2, B * ho * wo, train, rows)
            rows = ops.conv_gemm(t["y2"], self.w_fwd(b.conv3), t["y3"], N=o_, prologue=ops.PRO_AFFINE_RELU, pa=v(ws, S2.sc),
                                 pb=v(ws, S2.sh), **sp(S3))
            self._bn_coef(ws, b.bn3, B * ho * wo, train, rows)
            ja, jb, jc = (v(ws, sl) for sl in self.join[bi])
            lo_out = t.get("out_lo")
            if b.downsample is not None:
                Sd = self.bn[id(b.downsample[1])]
                rows = ops.conv_gemm(xin, self.w_fwd(b.downsample[0]), t["yd"], N=o_, stride=s_, **sp(Sd))
                self._bn_coef(ws, b.downsample[1], B * ho * wo, train, rows)
                torch.add(v(ws, S3.sh), v(ws, Sd.sh), out=jc)
                if lo_out is not None:       # both operands are raw convolution outputs; the stream starts here with 16 significant bits
                    ops.join_fwd(t["y3"], t["yd"], None, v(ws, S3.sc), v(ws, Sd.sc), jc, t["out"], lo_out, mk)
                else:
                    ops.affine2_relu(t["y3"], t["yd"], v(ws, S3.sc), v(ws, Sd.sc), jc, t["out"], mk)
            elif self.fuse_fwd[bi] and (o_) % 64 == 0 and t["out"].numel() * 2 < (1 << 32):
                t["id_hi"], t["id_lo"] = xin, xin_lo                           # joined in the prologue of the next block's conv1
                pending = (t, S3, mk)
            elif lo_out is not None or xin_lo is not None:
                ops.join_fwd(t["y3"], xin, xin_lo, v(ws, S3.sc), v(ws, self.ones, o_), v(ws, S3.sh), t["out"], lo_out, mk)
            else:
                ops.affine2_relu(t["y3"], xin, v(ws, S3.sc), v(ws, self.ones, o_), v(ws, S3.sh), t["out"], mk)
            xin, xin_lo = t["out"], lo_out
        ops.head_fwd(xin, v(ws, self.ones), v(ws, self.zeros), m.fc.weight, m.fc.bias, ws.pooled, ws.logits)
        if train:
            m._nbt_pending += 1
        return ws

    # ---- backward
    def _alloc_bwd(self, ws):
        if ws.bwd is not None:
            return
        dev, bf, B = self.device, self.dtype, ws.B
        e = lambda *s: torch.empty(*s, dtype=bf, device=dev)
        bw = {}
        # one gradient buffer per block OUTPUT shape change (identity blocks accumulate in place)
        bw["g"] = [None] * len(self.blocks)
        shapes = {}
        for bi, b in enumerate(self.blocks):
            sh = tuple(ws.blk[bi]["out"].shape)
            if sh not in shapes:
                shapes[sh] = e(*sh)
            bw["g"][bi] = shapes[sh]
        bw["g_in0"] = e(*ws.pool0.shape)
        bw["dz2"] = torch.empty(max(t["y2"].numel() for t in ws.blk), dtype=bf, device=dev)
        bw["dz1"] = torch.empty(max(t["y1"].numel() for t in ws.blk), dtype=bf, device=dev)
        bw["dz0"] = torch.empty_like(ws.c0)
        aa_t = [t for t in ws.blk if "QKV" in t]
        if aa_t:                                 # one set of attention-backward scratch buffers, sized for the largest block
            bw["dO"] = torch.empty(max(t["O"].numel() for t in aa_t), dtype=torch.float32, device=dev)
            bw["dQKV32"] = torch.empty(max(t["QKV"].numel() for t in aa_t), dtype=torch.float32, device=dev)
            bw["dQKV"] = torch.empty(max(t["QKV"].numel() for t in aa_t), dtype=bf, device=dev)
        ws.bwd = bw

    def _defer_wgrad(self):
        return self.det and not self.cifar          # the CIFAR stem keeps immediate sums (read back at once)

    def _backward(self, ws, dlogits, dx, done):
        m, v, G = self.model, self._v, self.grad_of
        B = ws.B
        self._alloc_bwd(ws)
        bw = ws.bwd
        z0, zn = self.bwd_zero
        ws.vec[z0:z0 + zn].zero_()
        det = self.det
        ew = lambda C: min(self.EW_ROWS, self.SLAB // C)

        def msp(S_):         # statistics arguments of a mask-epilogue producer of BatchNorm S_'s backward sums
            if det:
                return dict(stat_sum=ws.slab[0], stat_sq=ws.slab[1], stat_det=True, stat_replicas=self.SLAB // S_.C, stat_rstride=S_.C)
            return dict(stat_sum=v(ws, S_.S1), stat_sq=v(ws, S_.S2))

        def srows(S_, rows, second=None):      # (S1, S2, replicas, rstride) for cx_bn_bwd_coef
            if det:
                return ws.slab[0], (ws.slab[1] if second is None else second), rows, S_.C
            return v(ws, S_.S1), v(ws, S_.S2), 1, 0
        ones = lambda n: v(ws, self.ones, n)
        zeros = lambda n: v(ws, self.zeros, n)
        last = ws.blk[-1]["out"]
        dpooled = torch.empty(B, last.shape[3], dtype=torch.float32, device=self.device)
        ops.head_bwd(dlogits, ws.pooled, m.fc.weight, G(m.fc.weight), G(m.fc.bias) if m.fc.bias is not None else None, dpooled)
        g = bw["g"][-1]
        Cl = last.shape[3]
        ops.gap_relu_bn_bwd(dpooled, last, ones(Cl), zeros(Cl), zeros(Cl), ones(Cl), ones(Cl), g, v(ws, self.scratch[0], Cl),
                            v(ws, self.scratch[1], Cl))
        join_rows = None        # statistic rows of a join backward that ran in the epilogue of the block above (CX_EPI_JOIN)
        for bi in range(len(self.blocks) - 1, -1, -1):
            b, t = self.blocks[bi], ws.blk[bi]
            s_, p_ = b.stride, b.bn1.num_features
            o_ = self._last_bn(b).num_features
            hi, wi = t["hin"]
            ho, wo = t["hout"]
            cin = self._cin(b)
            xin = ws.blk[bi - 1]["out"] if bi > 0 else ws.pool0
            if self.basic:
                self._basic_backward(ws, bi, b, t, xin, msp, srows, ew, done)
                continue
            S1, S2, S3 = self.bn[id(b.bn1)], self.bn[id(b.bn2)], self.bn[id(b.bn3)]
            Sd = self.bn[id(b.downsample[1])] if b.downsample is not None else None
            g = bw["g"][bi]
            # residual join backward: dz = dOut * [out > 0] (in place), statistics for bn3 (and the downsample BN)
            cnt_o, cnt_i = B * ho * wo, B * hi * wi
            if join_rows is not None:
                # the conv1 input gradient of the block above finished dOut and ran this join in its epilogue (CX_EPI_JOIN)
                rows, join_rows = join_rows, None
            elif det:
                rows = ops.relu_bwd_stats(g, t["out"], t["y3"], v(ws, S3.mean), v(ws, S3.rstd), t["yd"], v(ws, Sd.mean) if Sd else None,
                                          v(ws, Sd.rstd) if Sd else None, g, ws.slab[0], ws.slab[1], ws.slab[2] if Sd else None,
                                          stat_rows=ew(S3.C), mask=t["mask"])
            else:
                rows = None
                ops.relu_bwd_stats(g, t["out"], t["y3"], v(ws, S3.mean), v(ws, S3.rstd), t["yd"], v(ws, Sd.mean) if Sd else None,
                                   v(ws, Sd.rstd) if Sd else None, g, v(ws, S3.S1), v(ws, S3.S2), v(ws, Sd.S2) if Sd else None,
                                   mask=t["mask"])
            r3 = srows(S3, rows)
            self.bn_bwd_coef(ws, b.bn3, r3[0], r3[1], cnt_o, b.bn3.weight, v(ws, S3.mean), v(ws, S3.rstd), G(b.bn3.weight),
                             G(b.bn3.bias), None, None, v(ws, S3.pa), v(ws, S3.pb), v(ws, S3.pc), S3.C, replicas=r3[2], rstride=r3[3])
            if Sd is not None and det:       # the downsample BatchNorm shares S1 with bn3: reduce it before the rows are re-used
                bnd = b.downsample[1]
                rd = srows(S3, rows, ws.slab[2])
                self.bn_bwd_coef(ws, bnd, rd[0], rd[1], cnt_o, bnd.weight, v(ws, Sd.mean), v(ws, Sd.rstd), G(bnd.weight), G(bnd.bias),
                                 None, None, v(ws, Sd.pa), v(ws, Sd.pb), v(ws, Sd.pc), Sd.C, replicas=rd[2], rstride=rd[3])
            dz2 = bw["dz2"][:B * ho * wo * p_].view(B, ho, wo, p_)
            rows = ops.conv_gemm(g, self.w_bwd(b.conv3), dz2, N=p_, prologue=ops.PRO_AFFINE2, x2=t["y3"], pa=v(ws, S3.pa),
                                 pb=v(ws, S3.pb), pc=v(ws, S3.pc), epilogue=ops.EPI_MASK, ex=t["y2"], e_sc=v(ws, S2.sc),
                                 e_sh=v(ws, S2.sh), e_mu=v(ws, S2.mean), e_r=v(ws, S2.rstd), e_scale=ones(p_), **msp(S2))
            r2 = srows(S2, rows)
            ops.conv_wgrad(g, t["y2"], G(b.conv3.weight), g_prologue=ops.PRO_AFFINE2, g2=t["y3"], ga=v(ws, S3.pa), gb=v(ws, S3.pb),
                           gc=v(ws, S3.pc), x_prologue=ops.PRO_AFFINE_RELU, pa=v(ws, S2.sc), pb=v(ws, S2.sh))
            self.bn_bwd_coef(ws, b.bn2, r2[0], r2[1], cnt_o, b.bn2.weight, v(ws, S2.mean), v(ws, S2.rstd), G(b.bn2.weight),
                             G(b.bn2.bias), None, None, v(ws, S2.pa), v(ws, S2.pb), v(ws, S2.pc), S2.C, replicas=r2[2], rstride=r2[3])
            dz1 = bw["dz1"][:B * hi * wi * p_].view(B, hi, wi, p_)
            mask1 = dict(epilogue=ops.EPI_MASK, ex=t["y1"], e_sc=v(ws, S1.sc), e_sh=v(ws, S1.sh), e_mu=v(ws, S1.mean),
                         e_r=v(ws, S1.rstd), e_scale=ones(p_), **msp(S1))
            if isinstance(b.conv2, AAConv2d):
                aa = b.conv2
                cc = p_ - aa.dv
                qa, qb, qc = v(ws, S2.pa), v(ws, S2.pb), v(ws, S2.pc)          # BN2 backward as dY2 = dz2*pa + y2*pb + pc
                gs_c, ys_c, gs_a, ys_a = dz2[..., :cc], t["y2"][..., :cc], dz2[..., cc:], t["y2"][..., cc:]
                dO = bw["dO"][:t["O"].numel()].view(t["O"].shape)
                dQ32 = bw["dQKV32"][:t["QKV"].numel()].view(t["QKV"].shape)
                dQ = bw["dQKV"][:t["QKV"].numel()].view(t["QKV"].shape)
                ops.aa_outproj_bwd(gs_a, ys_a, qa[cc:], qb[cc:], qc[cc:], t["O"], aa.out_proj.weight, dO, G(aa.out_proj.weight))
                ops.aa_attention_bwd(t["QKV"], *aa.rel_tables(), t["O"], dO, t["LSE"], dQ32, *aa.rel_grads(G), aa.nh, aa.dk, aa.dv)
                if self.dtype == torch.float32:
                    dQ = dQ32
                else:
                    ops.f32_to_bf16(dQ32, dQ)
                # both branches end in the same bn1 + ReLU mask: the conv branch writes dz1, the attention branch adds to it
                rows = ops.conv_gemm(gs_c, self.w_bwd(aa.conv), dz1, N=p_, kh=3, kw=3, pad=1, tstride=s_, prologue=ops.PRO_AFFINE2, x2=ys_c,
                                     pa=qa[:cc], pb=qb[:cc], pc=qc[:cc], **mask1)
                rows2 = ops.conv_gemm(dQ, self.w_bwd(aa.in_proj_qkv), dz1, N=p_, tstride=s_, accumulate=True,
                                      **self._stacked(ws, mask1, rows or 0, S1.C))
                rows = (rows or 0) + (rows2 or 0) if det else None
                ops.conv_wgrad(gs_c, t["y1"], G(aa.conv.weight), kh=3, kw=3, stride=s_, pad=1, g_prologue=ops.PRO_AFFINE2, g2=ys_c,
                               ga=qa[:cc], gb=qb[:cc], gc=qc[:cc], x_prologue=ops.PRO_AFFINE_RELU, pa=v(ws, S1.sc), pb=v(ws, S1.sh))
                ops.conv_wgrad(dQ, t["y1"], G(aa.in_proj_qkv.weight), stride=s_, x_prologue=ops.PRO_AFFINE_RELU, pa=v(ws, S1.sc),
                               pb=v(ws, S1.sh))
            else:
                d_ = b.conv2.dilation[0]              # (a dilated conv2 has stride 1: its input gradient's padding is d (2d - d))
                gr = b.conv2.groups
                kg = p_ // gr
                for g_ in range(gr):
                    c_ = slice(g_ * kg, (g_ + 1) * kg) if gr > 1 else slice(0, p_)
                    m1 = mask1 if gr == 1 else dict(epilogue=ops.EPI_MASK, ex=t["y1"][..., c_], e_sc=v(ws, S1.sc)[c_], e_sh=v(ws, S1.sh)[c_],
                                                    e_mu=v(ws, S1.mean)[c_], e_r=v(ws, S1.rstd)[c_], e_scale=ones(kg),
                                                    **self._stat_slice(msp(S1), c_))
                    rows = ops.conv_gemm(dz2[..., c_], self.w_bwd(b.conv2, g_ if gr > 1 else None), dz1[..., c_], N=kg, kh=3, kw=3, pad=d_,
                                         dil=d_, tstride=s_, prologue=ops.PRO_AFFINE2, x2=t["y2"][..., c_], pa=v(ws, S2.pa)[c_],
                                         pb=v(ws, S2.pb)[c_], pc=v(ws, S2.pc)[c_], **m1)
                    n_w = kg * kg * 9
                    ops.conv_wgrad(dz2[..., c_], t["y1"][..., c_], G(b.conv2.weight)[g_ * n_w:(g_ + 1) * n_w] if gr > 1 else G(b.conv2.weight),
                                   kh=3, kw=3, stride=s_, pad=d_, dil=d_, g_prologue=ops.PRO_AFFINE2, g2=t["y2"][..., c_],
                                   ga=v(ws, S2.pa)[c_], gb=v(ws, S2.pb)[c_], gc=v(ws, S2.pc)[c_], x_prologue=ops.PRO_AFFINE_RELU,
                                   pa=v(ws, S1.sc)[c_], pb=v(ws, S1.sh)[c_])
            r1 = srows(S1, rows)
            self.bn_bwd_coef(ws, b.bn1, r1[0], r1[1], cnt_i, b.bn1.weight, v(ws, S1.mean), v(ws, S1.rstd), G(b.bn1.weight),
                             G(b.bn1.bias), None, None, v(ws, S1.pa), v(ws, S1.pb), v(ws, S1.pc), S1.C, replicas=r1[2], rstride=r1[3])
            gx = (bw["g"][bi - 1] if bi > 0 else bw["g_in0"]) if Sd is not None or bi == 0 else g
            identity = Sd is None
            if identity and gx is not g:
                gx.copy_(g)                      # first block of layer1 never is an identity block; defensive
            prev = self.blocks[bi - 1] if bi > 0 else None
            if (self.join_fuse and det and identity and prev is not None and prev.downsample is None and cin % 128 == 0
                    and self.dtype == torch.bfloat16):
                # dOut of the block below is complete with this launch (identity path already in gx): its join backward -- ReLU
                # mask from the forward's sign bits, bn3 sums -- runs in the epilogue instead of a pass of its own over gx
                tp, Sp = ws.blk[bi - 1], self.bn[id(prev.bn3)]
                join_rows = ops.conv_gemm(dz1, self.w_bwd(b.conv1), gx, N=cin, prologue=ops.PRO_AFFINE2, x2=t["y1"], pa=v(ws, S1.pa),
                                          pb=v(ws, S1.pb), pc=v(ws, S1.pc), accumulate=True, epilogue=ops.EPI_JOIN, ex=tp["y3"],
                                          e_mu=v(ws, Sp.mean), e_r=v(ws, Sp.rstd), emask=tp["mask"], **msp(Sp))
            else:
                ops.conv_gemm(dz1, self.w_bwd(b.conv1), gx, N=cin, prologue=ops.PRO_AFFINE2, x2=t["y1"], pa=v(ws, S1.pa), pb=v(ws, S1.pb),
                              pc=v(ws, S1.pc), accumulate=identity)
            ops.conv_wgrad(dz1, xin, G(b.conv1.weight), g_prologue=ops.PRO_AFFINE2, g2=t["y1"], ga=v(ws, S1.pa), gb=v(ws, S1.pb),
                           gc=v(ws, S1.pc))
            if Sd is not None:
                bnd, convd = b.downsample[1], b.downsample[0]
                if not det:
                    self.bn_bwd_coef(ws, bnd, v(ws, S3.S1), v(ws, Sd.S2), cnt_o, bnd.weight, v(ws, Sd.mean), v(ws, Sd.rstd), G(bnd.weight),
                                     G(bnd.bias), None, None, v(ws, Sd.pa), v(ws, Sd.pb), v(ws, Sd.pc), Sd.C)
                ops.conv_gemm(g, self.w_bwd(convd), gx, N=cin, tstride=s_, prologue=ops.PRO_AFFINE2, x2=t["yd"], pa=v(ws, Sd.pa),
                              pb=v(ws, Sd.pb), pc=v(ws, Sd.pc), accumulate=True)
                ops.conv_wgrad(g, xin, G(convd.weight), stride=s_, g_prologue=ops.PRO_AFFINE2, g2=t["yd"], ga=v(ws, Sd.pa),
                               gb=v(ws, Sd.pb), gc=v(ws, Sd.pc))
            done(b.conv1.weight)
        # stem
        S0 = self.bn[id(m.bn1)]
        gx = bw["g_in0"]
        if self.cifar:
            c0, cnt0 = m.conv1.out_channels, B * ws.H * ws.W
            if det:
                rows = ops.relu_bwd_stats(gx, ws.pool0, ws.c0, v(ws, S0.mean), v(ws, S0.rstd), None, None, None, bw["dz0"], ws.slab[0],
                                          ws.slab[1], None, stat_rows=ew(c0))
            else:
                rows = None
                ops.relu_bwd_stats(gx, ws.pool0, ws.c0, v(ws, S0.mean), v(ws, S0.rstd), None, None, None, bw["dz0"], v(ws, S0.S1),
                                   v(ws, S0.S2), None)
            r0 = srows(S0, rows)
            self.bn_bwd_coef(ws, m.bn1, r0[0], r0[1], cnt0, m.bn1.weight, v(ws, S0.mean), v(ws, S0.rstd), G(m.bn1.weight), G(m.bn1.bias),
                             None, None, v(ws, S0.pa), v(ws, S0.pb), v(ws, S0.pc), c0, replicas=r0[2], rstride=r0[3])
            dw8 = torch.zeros(c0, 8, 3, 3, dtype=torch.float32, device=self.device)       # 3 input channels padded to 8
            ops.conv_wgrad(bw["dz0"], ws.x8, dw8, kh=3, kw=3, stride=1, pad=1, g_prologue=ops.PRO_AFFINE2, g2=ws.c0, ga=v(ws, S0.pa),
                           gb=v(ws, S0.pb), gc=v(ws, S0.pc))
            G(m.conv1.weight).view(c0, 3, 3, 3).add_(dw8[:, :3])
            if dx is not None:
                ops.stem_input_grad(bw["dz0"], ws.c0, v(ws, S0.pa), v(ws, S0.pb), v(ws, S0.pc), m.conv1.weight, dx, stride=1, pad=1)
        else:
            if det:
                rows = ops.bnrelu_maxpool_bwd(ws.c0, v(ws, S0.sc), v(ws, S0.sh), v(ws, S0.mean), v(ws, S0.rstd), ws.amax, gx, gx, ones(64),
                                              zeros(64), zeros(64), bw["dz0"], ws.slab[0], ws.slab[1], stat_rows=ew(64))
            else:
                rows = None
                ops.bnrelu_maxpool_bwd(ws.c0, v(ws, S0.sc), v(ws, S0.sh), v(ws, S0.mean), v(ws, S0.rstd), ws.amax, gx, gx, ones(64),
                                       zeros(64), zeros(64), bw["dz0"], v(ws, S0.S1), v(ws, S0.S2))
            r0 = srows(S0, rows)
            self.bn_bwd_coef(ws, m.bn1, r0[0], r0[1], B * (ws.H // 2) * (ws.W // 2), m.bn1.weight, v(ws, S0.mean), v(ws, S0.rstd),
                             G(m.bn1.weight), G(m.bn1.bias), None, None, v(ws, S0.pa), v(ws, S0.pb), v(ws, S0.pc), 64, replicas=r0[2],
                             rstride=r0[3])
            ops.conv_wgrad(bw["dz0"], ws.x4, G(m.conv1.weight), mode=ops.MODE_STEM, g_prologue=ops.PRO_AFFINE2, g2=ws.c0,
                           ga=v(ws, S0.pa), gb=v(ws, S0.pb), gc=v(ws, S0.pc))
            if dx is not None:
                ops.stem_input_grad(bw["dz0"], ws.c0, v(ws, S0.pa), v(ws, S0.pb), v(ws, S0.pc), m.conv1.weight, dx, stride=2, pad=3)

    def _basic_backward(self, ws, bi, b, t, xin, msp, srows, ew, done):
        """Backward of one BasicBlock (attn_aug_conv.py:135-156), same conventions as the bottleneck path: the block's output
        gradient is masked in place by the join ReLU, BatchNorm backward rides in the two-tensor prologues of the consumers."""
        v, G, bw, B, det = self._v, self.grad_of, ws.bwd, ws.B, self.det
        s_, p_, cin = b.stride, b.bn1.num_features, self._cin(b)
        ho, wo = t["hout"]
        S1, S2 = self.bn[id(b.bn1)], self.bn[id(b.bn2)]
        Sd = self.bn[id(b.downsample[1])] if b.downsample is not None else None
        g = bw["g"][bi]
        cnt = B * ho * wo
        ones = v(ws, self.ones, p_)
        if det:
            rows = ops.relu_bwd_stats(g, t["out"], t["y2"], v(ws, S2.mean), v(ws, S2.rstd), t["yd"], v(ws, Sd.mean) if Sd else None,
                                      v(ws, Sd.rstd) if Sd else None, g, ws.slab[0], ws.slab[1], ws.slab[2] if Sd else None,
                                      stat_rows=ew(S2.C), mask=t["mask"])
        else:
            rows = None
            ops.relu_bwd_stats(g, t["out"], t["y2"], v(ws, S2.mean), v(ws, S2.rstd), t["yd"], v(ws, Sd.mean) if Sd else None,
                               v(ws, Sd.rstd) if Sd else None, g, v(ws, S2.S1), v(ws, S2.S2), v(ws, Sd.S2) if Sd else None,
                               mask=t["mask"])
        r2 = srows(S2, rows)
        self.bn_bwd_coef(ws, b.bn2, r2[0], r2[1], cnt, b.bn2.weight, v(ws, S2.mean), v(ws, S2.rstd), G(b.bn2.weight), G(b.bn2.bias),
                         None, None, v(ws, S2.pa), v(ws, S2.pb), v(ws, S2.pc), S2.C, replicas=r2[2], rstride=r2[3])
        if Sd is not None:                   # the downsample BatchNorm shares S1 (sum of the masked gradient) with bn2
            bnd = b.downsample[1]
            rd = srows(S2, rows, ws.slab[2]) if det else (v(ws, S2.S1), v(ws, Sd.S2), 1, 0)
            self.bn_bwd_coef(ws, bnd, rd[0], rd[1], cnt, bnd.weight, v(ws, Sd.mean), v(ws, Sd.rstd), G(bnd.weight), G(bnd.bias), None, None,
                             v(ws, Sd.pa), v(ws, Sd.pb), v(ws, Sd.pc), Sd.C, replicas=rd[2], rstride=rd[3])
        dz1 = bw["dz1"][:cnt * p_].view(B, ho, wo, p_)
        rows = ops.conv_gemm(g, self.w_bwd(b.conv2), dz1, N=p_, kh=3, kw=3, pad=1, prologue=ops.PRO_AFFINE2, x2=t["y2"], pa=v(ws, S2.pa),
                             pb=v(ws, S2.pb), pc=v(ws, S2.pc), epilogue=ops.EPI_MASK, ex=t["y1"], e_sc=v(ws, S1.sc), e_sh=v(ws, S1.sh),
                             e_mu=v(ws, S1.mean), e_r=v(ws, S1.rstd), e_scale=ones, **msp(S1))
        r1 = srows(S1, rows)
        ops.conv_wgrad(g, t["y1"], G(b.conv2.weight), kh=3, kw=3, stride=1, pad=1, g_prologue=ops.PRO_AFFINE2, g2=t["y2"],
                       ga=v(ws, S2.pa), gb=v(ws, S2.pb), gc=v(ws, S2.pc), x_prologue=ops.PRO_AFFINE_RELU, pa=v(ws, S1.sc), pb=v(ws, S1.sh))
        self.bn_bwd_coef(ws, b.bn1, r1[0], r1[1], cnt, b.bn1.weight, v(ws, S1.mean), v(ws, S1.rstd), G(b.bn1.weight), G(b.bn1.bias),
                         None, None, v(ws, S1.pa), v(ws, S1.pb), v(ws, S1.pc), S1.C, replicas=r1[2], rstride=r1[3])
        gx = (bw["g"][bi - 1] if bi > 0 else bw["g_in0"]) if Sd is not None or bi == 0 else g
        identity = Sd is None
        if identity and gx is not g:
            gx.copy_(g)
        if isinstance(b.conv1, AAConv2d):
            aa = b.conv1
            cc = p_ - aa.dv
            qa, qb, qc = v(ws, S1.pa), v(ws, S1.pb), v(ws, S1.pc)              # BN1 backward as dY1 = dz1*pa + y1*pb + pc
            gs_c, ys_c, gs_a, ys_a = dz1[..., :cc], t["y1"][..., :cc], dz1[..., cc:], t["y1"][..., cc:]
            dO = bw["dO"][:t["O"].numel()].view(t["O"].shape)
            dQ32 = bw["dQKV32"][:t["QKV"].numel()].view(t["QKV"].shape)
            dQ = bw["dQKV"][:t["QKV"].numel()].view(t["QKV"].shape)
            ops.aa_outproj_bwd(gs_a, ys_a, qa[cc:], qb[cc:], qc[cc:], t["O"], aa.out_proj.weight, dO, G(aa.out_proj.weight))
            ops.aa_attention_bwd(t["QKV"], *aa.rel_tables(), t["O"], dO, t["LSE"], dQ32, *aa.rel_grads(G), aa.nh, aa.dk, aa.dv)
            if self.dtype == torch.float32:
                dQ = dQ32
            else:
                ops.f32_to_bf16(dQ32, dQ)
            ops.conv_gemm(gs_c, self.w_bwd(aa.conv), gx, N=cin, kh=3, kw=3, pad=1, tstride=s_, prologue=ops.PRO_AFFINE2, x2=ys_c,
                          pa=qa[:cc], pb=qb[:cc], pc=qc[:cc], accumulate=identity)
            ops.conv_gemm(dQ, self.w_bwd(aa.in_proj_qkv), gx, N=cin, tstride=s_, accumulate=True)
            ops.conv_wgrad(gs_c, xin, G(aa.conv.weight), kh=3, kw=3, stride=s_, pad=1, g_prologue=ops.PRO_AFFINE2, g2=ys_c, ga=qa[:cc],
                           gb=qb[:cc], gc=qc[:cc])
            ops.conv_wgrad(dQ, xin, G(aa.in_proj_qkv.weight), stride=s_)
        else:
            ops.conv_gemm(dz1, self.w_bwd(b.conv1), gx, N=cin, kh=3, kw=3, pad=1, tstride=s_, prologue=ops.PRO_AFFINE2, x2=t["y1"],
                          pa=v(ws, S1.pa), pb=v(ws, S1.pb), pc=v(ws, S1.pc), accumulate=identity)
            ops.conv_wgrad(dz1, xin, G(b.conv1.weight), kh=3, kw=3, stride=s_, pad=1, g_prologue=ops.PRO_AFFINE2, g2=t["y1"],
                           ga=v(ws, S1.pa), gb=v(ws, S1.pb), gc=v(ws, S1.pc))
        if Sd is not None:
            convd = b.downsample[0]
            ops.conv_gemm(g, self.w_bwd(convd), gx, N=cin, tstride=s_, prologue=ops.PRO_AFFINE2, x2=t["yd"], pa=v(ws, Sd.pa),
                          pb=v(ws, Sd.pb), pc=v(ws, Sd.pc), accumulate=True)
            ops.conv_wgrad(g, xin, G(convd.weight), stride=s_, g_prologue=ops.PRO_AFFINE2, g2=t["yd"], ga=v(ws, Sd.pa), gb=v(ws, Sd.pb),
                           gc=v(ws, Sd.pc))
        done(b.conv1.weight if not isinstance(b.conv1, AAConv2d) else b.conv1.first_param())


class ResNet(FusedNet):
    """Signature of /root/reference/models/attn_aug_conv.py:218-220."""

    def __init__(self, block, layers, num_classes=1000, zero_init_residual=False, groups=1, width_per_group=64,
                 replace_stride_with_dilation=None, norm_layer=None, attn_params=None):
        super().__init__()
        if block not in (Bottleneck, BasicBlock):
            raise NotImplementedError("block must be Bottleneck or BasicBlock")
        self.block = block
        if (groups != 1 or width_per_group != 64) and block is BasicBlock:
            raise ValueError("BasicBlock only supports groups=1 and base_width=64")          # attn_aug_conv.py:114-115
        if groups != 1 and attn_params is not None:
            raise NotImplementedError("grouped attention-augmented networks are not built")
        self.groups = groups
        if replace_stride_with_dilation is None:
            replace_stride_with_dilation = [False, False, False]
        if len(replace_stride_with_dilation) != 3:                                             # attn_aug_conv.py:233-235
            raise ValueError("replace_stride_with_dilation should be None or a 3-element tuple, got {}".format(replace_stride_with_dilation))
        if any(replace_stride_with_dilation) and (block is BasicBlock or attn_params is not None):
            raise NotImplementedError("Dilation > 1 not supported in BasicBlock" if block is BasicBlock else
                                      "dilated attention-augmented networks are not built")
        self.base_width = width_per_group
        self.dilation = 1
        self.inplanes = 64
        self.conv1 = Conv2dParams(3, 64, 7, 2, 3, bias=False)
        self.bn1 = BatchNorm2dParams(64)
        self.relu = ReLUMarker(inplace=True)
        self.maxpool = PoolMarker()
        self.layer1 = self._make_layer(64, layers[0], 1)
        rd = replace_stride_with_dilation
        self.layer2 = self._make_layer(128, layers[1], 2, attn_params, dilate=rd[0])          # attn_aug_conv.py:242-244: layers 2-4 only
        self.layer3 = self._make_layer(256, layers[2], 2, attn_params, dilate=rd[1])
        self.layer4 = self._make_layer(512, layers[3], 2, attn_params, dilate=rd[2])
        self.avgpool = PoolMarker()
        self.fc = nn.Linear(512 * block.expansion, num_classes)
        for mod in self.modules():                      # initialisers of attn_aug_conv.py:248-263
            if isinstance(mod, nn.Conv2d):
                nn.init.kaiming_normal_(mod.weight, mode="fan_out", nonlinearity="relu")
            elif isinstance(mod, nn.BatchNorm2d):
                nn.init.constant_(mod.weight, 1)
                nn.init.constant_(mod.bias, 0)
        if zero_init_residual:
            for mod in self.modules():
                if isinstance(mod, Bottleneck):
                    nn.init.constant_(mod.bn3.weight, 0)
                elif isinstance(mod, BasicBlock):
                    nn.init.constant_(mod.bn2.weight, 0)

    def _eng(self):
        for mod in self.modules():
            if isinstance(mod, AAConv2d):
                mod.check_supported()
        if self._engine is None or self._engine.dtype != getattr(self, "_storage_dtype", torch.bfloat16):
            object.__setattr__(self, "_engine", _Engine(self))
        return self._engine

    def _anchor(self):
        return self.fc.weight

    def _make_layer(self, planes, blocks, stride, attn_params=None, dilate=False):
        block, e = self.block, self.block.expansion
        down = None
        previous_dilation = getattr(self, "dilation", 1)        # attn_aug_conv.py:266-271: the stride becomes a dilation
        if dilate:
            self.dilation = previous_dilation * stride
            stride = 1
        if stride != 1 or self.inplanes != planes * e:
            down = nn.Sequential(Conv2dParams(self.inplanes, planes * e, 1, stride, bias=False), BatchNorm2dParams(planes * e))
        bw = getattr(self, "base_width", 64)
        dl = getattr(self, "dilation", 1)
        gr = getattr(self, "groups", 1)
        layers = [block(self.inplanes, planes, stride, down, groups=gr, base_width=bw, dilation=previous_dilation, attn_params=attn_params)]
        self.inplanes = planes * e
        for _ in range(1, blocks):
            layers.append(block(self.inplanes, planes, groups=gr, base_width=bw, dilation=dl, attn_params=attn_params))
        return nn.Sequential(*layers)

    def _stages(self):
        return (self.layer1, self.layer2, self.layer3, self.layer4)


class WideResNet(FusedNet):
    """Signature and parameters of /root/reference/models/attn_aug_conv.py:311-404 (WRN-d-k on CIFAR: 3x3 stem, three stages of
    BasicBlocks, AAConv2d in stages 2-3).  The network of the CIFAR harness (models/test_model.py), on the same HIP schedule as the
    BasicBlock ResNets (3x3 stem without max-pool); attention head sizes outside the kernels' set raise when the model is run."""

    def __init__(self, block, depth, width, num_classes=100, zero_init_residual=False, groups=1, width_per_group=64,
                 replace_stride_with_dilation=None, norm_layer=None, attn_params=None):
        super().__init__()
        assert (depth - 4) % 6 == 0, "depth should be 6n+4"
        n = (depth - 4) // 6
        if attn_params:                          # the reference rescales (and mutates) the caller's dict, :322-324
            attn_params = dict(attn_params)
            attn_params["input_dims"] = (int(attn_params["input_dims"][0] * width), int(attn_params["input_dims"][1] * width))
        if replace_stride_with_dilation not in (None, [False] * 3, (False,) * 3):
            raise NotImplementedError("dilated variants are not built")
        self.block = block
        self.inplanes = 16
        self.conv1 = Conv2dParams(3, 16, 3, 1, 1, bias=False)
        self.bn1 = BatchNorm2dParams(16)
        self.relu = ReLUMarker(inplace=True)
        self.layer1 = self._make_layer(16 * width, n, 1)
        self.layer2 = self._make_layer(32 * width, n, 2, attn_params)
        self.layer3 = self._make_layer(64 * width, n, 2, attn_params)
        self.avgpool = PoolMarker()
        self.fc = nn.Linear(64 * width, num_classes)
        for mod in self.modules():
            if isinstance(mod, nn.Conv2d):
                nn.init.kaiming_normal_(mod.weight, mode="fan_out", nonlinearity="relu")
            elif isinstance(mod, nn.BatchNorm2d):
                nn.init.constant_(mod.weight, 1)
                nn.init.constant_(mod.bias, 0)
        if zero_init_residual:
            for mod in self.modules():
                if isinstance(mod, BasicBlock):
                    nn.init.constant_(mod.bn2.weight, 0)

    _eng, _anchor, _make_layer = ResNet._eng, ResNet._anchor, ResNet._make_layer

    def _stages(self):
        return (self.layer1, self.layer2, self.layer3)


def resnet152(pretrained=False, **kwargs):
    """torchvision.models.resnet152 stand-in (chexpert.py:24, :482)."""
    if pretrained:
        raise RuntimeError("pretrained ImageNet weights cannot be downloaded here; use load_state_dict()")
    return ResNet(Bottleneck, [3, 8, 36, 3], **kwargs)
