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
    """Host-side schedule.  `forward` drives `_stem_forward` / `_cifar_stem_forward`, then per block `_bottleneck_forward` or
    `_basic_forward` (both end in `_join_forward`, with `_down_forward` for a downsample block), then the head; `_backward` drives
    `_head_backward`, per block `_bottleneck_backward` / `_basic_backward` (both begin with `_join_backward` and share
    `_aa_backward_front`, `_gx` and `_down_backward`), then `_stem_backward` / `_cifar_stem_backward`.  What one block hands to the
    next is passed explicitly: `pending` (a forward join deferred to the next conv1's prologue) and `join_rows` (a join backward
    that ran in the epilogue of the block above)."""
    SLAB = 1 << 22               # floats per statistic-row scratch (rows x channels of the largest producer)
    EW_ROWS = 2048

    def __init__(self, model):
        super().__init__(model)
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
        # keep_lo[bi]: block bi's output has a lo plane -- every output that feeds an identity join (46 of resnet152's 50 joins; the
        # four downsample blocks' outputs start a stage and are rounded once).  Keeping it only through the long stages measured
        # 8.3e-3 on the reference fixture's train logits at 128 images, on every identity join 6.9e-3 for +0.36 ms of the 54.2 ms
        # step (profiles/r05_resnet_margin.txt): the 1e-2 bound then has 30 % of room instead of 17 %.
        # fuse_fwd[bi]: block bi's join runs in the prologue of block bi + 1's conv1.  That form stays with the stages of >= 6
        # blocks: it does not pay on layer1 (N = 64 on a 256-wide tile) nor layer4 (MFMA-bound) -- scratch/bench_join.py.
        n = len(self.blocks)
        stage_len = [len(L) for L in model._stages() for _ in L]
        ident = [b.downsample is None for b in self.blocks]
        self.keep_lo = [self.two_plane and i + 1 < n and ident[i + 1] for i in range(n)]
        self.fuse_fwd = [self.two_plane and self.fwd_join_fuse and ident[i] and stage_len[i] >= 6 and i + 1 < n for i in range(n)]
        self.cifar = isinstance(model, WideResNet)              # 3x3 stride-1 stem, no max-pool, three stages (:311-404)
        self.bn, rest = _BN.plan(list(self._all_bns()))
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
        ws.slab = torch.empty(3, self.SLAB, dtype=torch.float32, device=dev)
        ws.logits = torch.empty(B, self.n_classes, dtype=torch.float32, device=dev)
        ws.vec = torch.zeros(self.vec_size, dtype=torch.float32, device=dev)
        o, n = self.ones
        ws.vec[o:o + n].fill_(1.0)
        ws.bwd = None
        return ws

    # ---- statistics plumbing: every producer of a BatchNorm's sums writes one row per workgroup into ws.slab[0] / ws.slab[1], at
    # the pitch of the BatchNorm's width, and returns the number of rows; the coefficient kernel that follows (_bn_coef, _bn_bwd)
    # sums them in row order.  Named as in the DenseNet engine: keywords of a convolution producer (_sp), (S1, S2, stat_rows) of an
    # element-wise producer (_ew)
    def _sp(self, ws, S, bwd=False, after=0):
        """Statistics keywords of a convolution that produces BatchNorm S's forward sums (none in an eval forward), or with `bwd`
        its backward sums S1 / S2 in a mask epilogue.  after: the rows of a first producer of the same sums -- this one's rows go
        behind them, so one reduction over both adds them."""
        if ws.frozen and not bwd:
            return {}
        return dict(stat_sum=ws.slab[0][after * S.C:], stat_sq=ws.slab[1][after * S.C:], stat_det=True,
                    stat_replicas=self.SLAB // S.C - after, stat_rstride=S.C)

    def _ew(self, ws, S):
        return ws.slab[0], ws.slab[1], min(self.EW_ROWS, self.SLAB // S.C)

    @staticmethod
    def _stat_slice(kw, c_):
        """statistics keywords of a producer restricted to the channel range c_ of their BatchNorm (grouped convolutions): the
        row buffers start at the range's first channel, the row pitch stays the BatchNorm's width"""
        kw = dict(kw)
        for k in ("stat_sum", "stat_sq"):
            if kw.get(k) is not None:
                kw[k] = kw[k][c_.start:]
        return kw

    # ---- BatchNorm in the epilogue of an input-gradient convolution (the prologue keywords are FusedEngine's).  c_: the channel
    # range of one group of a grouped convolution or of an AAConv2d branch (None: all channels)
    def _mask(self, ws, y, S, c_=None, after=0):
        """input gradient: the epilogue that masks with [relu(bn_S(y)) > 0] and produces BatchNorm S's backward sums (_sp)"""
        ch, v = self._ch, self._v
        kw = self._sp(ws, S, bwd=True, after=after)
        return dict(epilogue=ops.EPI_MASK, ex=ch(y, c_), e_sc=ch(v(ws, S.sc), c_), e_sh=ch(v(ws, S.sh), c_), e_mu=ch(v(ws, S.mean), c_),
                    e_r=ch(v(ws, S.rstd), c_), e_scale=v(ws, self.ones, S.C if c_ is None else c_.stop - c_.start),
                    **(kw if c_ is None else self._stat_slice(kw, c_)))

    def _bn_coef_part(self, ws, bn, count, rows, lo, n):
        """_bn_coef for channels [lo, lo + n) of `bn` from `rows` statistic rows of pitch n (an AAConv2d's conv branch and its
        attention out-projection each produce the rows of their own channel range)."""
        S, v = self.bn[id(bn)], self._v
        mom = bn.momentum if bn.momentum is not None else 0.1
        c = lambda t_: t_[lo:lo + n]
        rm, rv = (c(bn.running_mean), c(bn.running_var)) if self.track_stats else (None, None)
        ops.bn_coef(ws.slab[0], ws.slab[1], count, c(bn.weight), c(bn.bias), bn.eps, mom, rm, rv,
                    c(v(ws, S.sc)), c(v(ws, S.sh)), c(v(ws, S.mean)), c(v(ws, S.rstd)), n, replicas=rows, rstride=n)

    # ---- forward
    def _aa_fwd(self, ws, aa, xin, yout, qkv_t, bn, stride, count, pro):
        """AAConv2d forward (attn_aug_conv.py:65-97) into `yout` = [conv branch | attention], and the coefficients of the BatchNorm
        `bn` that follows (training: the statistic rows of the two kernels are reduced per channel range; an eval forward produces
        no statistics)."""
        train = not ws.frozen
        cc = yout.shape[3] - aa.dv
        stat = dict(stat_sum=ws.slab[0], stat_sq=ws.slab[1], stat_det=True, stat_replicas=self.SLAB // cc, stat_rstride=cc) if train \
            else dict(stat_sum=None, stat_sq=None)
        rows = ops.conv_gemm(xin, self.w_fwd(aa.conv), yout[..., :cc], N=cc, kh=3, kw=3, stride=stride, pad=1, **stat, **pro)
        if train:
            self._bn_coef_part(ws, bn, count, rows, 0, cc)
        ops.conv_gemm(xin, self.w_fwd(aa.in_proj_qkv), qkv_t["QKV"], N=2 * aa.dk + aa.dv, stride=stride, **pro)
        ops.aa_attention_fwd(qkv_t["QKV"], *aa.rel_tables(), qkv_t["O"], qkv_t["LSE"], aa.nh, aa.dk, aa.dv)
        object.__setattr__(aa, "_last", (qkv_t["QKV"], qkv_t["LSE"]))
        if train:
            rows = ops.aa_outproj_fwd(qkv_t["O"], aa.out_proj.weight, yout[..., cc:], ws.slab[0], ws.slab[1],
                                      stat_rows=min(self.EW_ROWS, self.SLAB // aa.dv), stat_rstride=aa.dv)
            self._bn_coef_part(ws, bn, count, rows, cc, aa.dv)
        else:
            ops.aa_outproj_fwd(qkv_t["O"], aa.out_proj.weight, yout[..., cc:], None, None)
            self._bn_coef(ws, bn, count, False)

    def forward(self, x, train, record=False):
        """train: batch statistics (and running-statistic updates); eval: running statistics.  record (eval): also keep what
        backward reads -- the join ReLU sign bits, which an eval forward without a backward skips."""
        m = self.model
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
        xin = self._cifar_stem_forward(ws, x) if self.cifar else self._stem_forward(ws, x)
        xin_lo, pending = None, None
        for bi in range(len(self.blocks)):
            if self.basic:
                xin = self._basic_forward(ws, bi, xin)
            else:
                xin, xin_lo, pending = self._bottleneck_forward(ws, bi, xin, xin_lo, pending)
        self._head_forward(ws, xin)
        if train and self.track_stats:
            m._nbt_pending += 1
        return ws

    def _head_forward(self, ws, xin):
        """The shared head (FusedEngine._head_fwd) on the last block's output, which is already activated: ReLU of x * 1 + 0."""
        v = self._v
        self._head_fwd(ws, xin, v(ws, self.ones), v(ws, self.zeros), self.model.fc, ops.POOL_ACT_RELU)

    def _stem_forward(self, ws, x):
        """7x7 stride-2 convolution, BatchNorm + ReLU + 3x3 stride-2 max-pool in one kernel"""
        m, v = self.model, self._v
        S0 = self.bn[id(m.bn1)]
        if x.dtype == torch.uint8:
            ops.u8_to_nhwc4(x.contiguous(), ws.x4)
        else:
            ops.nchw3_to_nhwc4(x.contiguous().float(), ws.x4)
        rows = ops.conv_gemm(ws.x4, self.w_fwd(m.conv1), ws.c0, N=64, mode=ops.MODE_STEM, **self._sp(ws, S0))
        self._bn_coef(ws, m.bn1, ws.B * (ws.H // 2) * (ws.W // 2), not ws.frozen, rows)
        ops.bnrelu_maxpool_fwd(ws.c0, v(ws, S0.sc), v(ws, S0.sh), ws.pool0, ws.amax, None, None)
        return ws.pool0

    def _cifar_stem_forward(self, ws, x):
        """attn_aug_conv.py:341-343, :391-393: 3x3 stride-1 stem, BatchNorm, ReLU -- no max-pool"""
        m, v = self.model, self._v
        if x.dtype == torch.uint8:
            raise RuntimeError("the CIFAR stem takes (B,3,H,W) float images")
        S0, c0 = self.bn[id(m.bn1)], m.conv1.out_channels
        ops.nchw3_to_nhwc8(x.contiguous().float(), ws.x8)
        rows = ops.conv_gemm(ws.x8, self.packed[self.stem_off:], ws.c0, N=c0, kh=3, kw=3, stride=1, pad=1, **self._sp(ws, S0))
        self._bn_coef(ws, m.bn1, ws.B * ws.H * ws.W, not ws.frozen, rows)
        ops.affine2_relu(ws.c0, ws.c0, v(ws, S0.sc), v(ws, self.zeros, c0), v(ws, S0.sh), ws.pool0)
        return ws.pool0

    def _basic_forward(self, ws, bi, xin):
        """attn_aug_conv.py:135-156: conv3x3(stride) - bn1 - relu - conv3x3 - bn2, + identity | downsample(x), relu.  Returns the
        block's output."""
        b, t, train = self.blocks[bi], ws.blk[bi], not ws.frozen
        ho, wo = t["hout"]
        p_, cnt = b.bn1.num_features, ws.B * ho * wo
        S1, S2 = self.bn[id(b.bn1)], self.bn[id(b.bn2)]
        if isinstance(b.conv1, AAConv2d):
            # attn_aug_conv.py:124-131, :65-97: the first 3x3 is attention-augmented (conv branch || attention, on the raw input)
            self._aa_fwd(ws, b.conv1, xin, t["y1"], t, b.bn1, b.stride, cnt, {})
        else:
            rows = ops.conv_gemm(xin, self.w_fwd(b.conv1), t["y1"], N=p_, kh=3, kw=3, stride=b.stride, pad=1, **self._sp(ws, S1))
            self._bn_coef(ws, b.bn1, cnt, train, rows)
        rows = ops.conv_gemm(t["y1"], self.w_fwd(b.conv2), t["y2"], N=p_, kh=3, kw=3, stride=1, pad=1, **self._pro_bnrelu(ws, S1),
                             **self._sp(ws, S2))
        self._bn_coef(ws, b.bn2, cnt, train, rows)
        self._join_forward(ws, bi, xin, None)
        return t["out"]

    def _bottleneck_forward(self, ws, bi, xin, xin_lo, pending):
        """attn_aug_conv.py:186-211 with the stride on conv2.  xin / xin_lo: the planes of the block's input; pending: the join of
        the block below when it was left to this conv1's prologue (_join_forward).  Returns (out, out_lo, pending of this block)."""
        v, b, t, train = self._v, self.blocks[bi], ws.blk[bi], not ws.frozen
        s_, p_ = b.stride, b.bn1.num_features
        (hi, wi), (ho, wo) = t["hin"], t["hout"]
        cnt = ws.B * ho * wo
        S1, S2, S3 = self.bn[id(b.bn1)], self.bn[id(b.bn2)], self.bn[id(b.bn3)]
        if pending is not None:
            # attn_aug_conv.py:202-211 of the block below + :188 of this one: out = relu(bn3(y3) + identity) is computed in this
            # conv1's prologue (hi plane = its operand) and leaves as hi / lo / sign-bit side outputs -- no pass of its own
            tp, Sp, mkp = pending
            rows = ops.conv_gemm(tp["y3"], self.w_fwd(b.conv1), t["y1"], N=p_, prologue=ops.PRO_JOIN, x2=tp["id_hi"], x3=tp["id_lo"],
                                 pa=v(ws, Sp.sc), pb=v(ws, self.ones, self._cin(b)), pc=v(ws, Sp.sh), pro_out=tp["out"],
                                 po_lo=tp.get("out_lo"), po_mask=mkp, **self._sp(ws, S1))
        else:
            rows = ops.conv_gemm(xin, self.w_fwd(b.conv1), t["y1"], N=p_, **self._sp(ws, S1))
        self._bn_coef(ws, b.bn1, ws.B * hi * wi, train, rows)
        if isinstance(b.conv2, AAConv2d):
            # attn_aug_conv.py:65-97: 3x3 conv branch || multi-head attention over the stride-s grid, concatenated on channels
            self._aa_fwd(ws, b.conv2, t["y1"], t["y2"], t, b.bn2, s_, cnt, self._pro_bnrelu(ws, S1))
        else:
            # conv3x3(width, width, stride, groups, dilation) (attn_aug_conv.py:183): one launch per group on its channel slice of
            # y1 / y2; the statistic rows of the groups sit side by side at the pitch of the whole BatchNorm
            # d > 1 under replace_stride_with_dilation: padding = dilation.  The block's own stride stays on conv2, so a dilated conv2
            # can have stride 2 (rd = [True, False, True]: layer3[0] has dilation 2 from layer2 and stride 2 of its own)
            d_, gr = b.conv2.dilation[0], b.conv2.groups
            kg = p_ // gr
            for g_ in range(gr):
                c_, wg = (slice(g_ * kg, (g_ + 1) * kg), g_) if gr > 1 else (None, None)
                kw = self._sp(ws, S2)
                rows = ops.conv_gemm(self._ch(t["y1"], c_), self.w_fwd(b.conv2, wg), self._ch(t["y2"], c_), N=kg, kh=3, kw=3, stride=s_,
                                     pad=d_, dil=d_, **self._pro_bnrelu(ws, S1, c_), **(kw if c_ is None else self._stat_slice(kw, c_)))
            self._bn_coef(ws, b.bn2, cnt, train, rows)
        rows = ops.conv_gemm(t["y2"], self.w_fwd(b.conv3), t["y3"], N=S3.C, **self._pro_bnrelu(ws, S2), **self._sp(ws, S3))
        self._bn_coef(ws, b.bn3, cnt, train, rows)
        return t["out"], t.get("out_lo"), self._join_forward(ws, bi, xin, xin_lo)

    def _down_forward(self, ws, b, t, xin):
        """the 1x1 stride-s convolution of a downsample block and the coefficients of its BatchNorm, whose slot is returned"""
        ho, wo = t["hout"]
        Sd = self.bn[id(b.downsample[1])]
        rows = ops.conv_gemm(xin, self.w_fwd(b.downsample[0]), t["yd"], N=Sd.C, stride=b.stride, **self._sp(ws, Sd))
        self._bn_coef(ws, b.downsample[1], ws.B * ho * wo, not ws.frozen, rows)
        return Sd

    def _join_forward(self, ws, bi, xin, xin_lo):
        """The residual join of block bi, out = relu(bn_last(y) + (bn_d(downsample(x)) | x)), on the last convolution's raw output
        y.  An identity join of fuse_fwd is not computed here: it is returned as `pending` = (t, slot of bn_last, mask) for the next
        block's conv1 (else None).  A lo plane is read / written where the stream has one (keep_lo)."""
        v, b, t = self._v, self.blocks[bi], ws.blk[bi]
        S = self.bn[id(self._last_bn(b))]
        y, ones = t["y2" if self.basic else "y3"], v(ws, self.ones, S.C)
        mk = t["mask"] if ws.recorded else None
        lo_out = t.get("out_lo")
        if b.downsample is not None:
            Sd = self._down_forward(ws, b, t, xin)
            jc = v(ws, self.join[bi][2])
            torch.add(v(ws, S.sh), v(ws, Sd.sh), out=jc)
            if lo_out is not None:       # both operands are raw convolution outputs; the stream starts here with 16 significant bits
                ops.join_fwd(y, t["yd"], None, v(ws, S.sc), v(ws, Sd.sc), jc, t["out"], lo_out, mk)
            else:
                ops.affine2_relu(y, t["yd"], v(ws, S.sc), v(ws, Sd.sc), jc, t["out"], mk)
        elif self.fuse_fwd[bi] and S.C % 64 == 0 and t["out"].numel() * 2 < (1 << 32):
            t["id_hi"], t["id_lo"] = xin, xin_lo
            return t, S, mk
        elif lo_out is not None or xin_lo is not None:
            ops.join_fwd(y, xin, xin_lo, v(ws, S.sc), ones, v(ws, S.sh), t["out"], lo_out, mk)
        else:
            ops.affine2_relu(y, xin, v(ws, S.sc), ones, v(ws, S.sh), t["out"], mk)
        return None

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
        return not self.cifar          # the CIFAR stem keeps immediate sums (read back at once)

    def _backward(self, ws, dlogits, dx, done):
        self._alloc_bwd(ws)
        self._head_backward(ws, dlogits, done)
        join_rows = None        # statistic rows of a join backward that ran in the epilogue of the block above (CX_EPI_JOIN)
        for bi in range(len(self.blocks) - 1, -1, -1):
            if self.basic:
                self._basic_backward(ws, bi, done)
            else:
                join_rows = self._bottleneck_backward(ws, bi, join_rows, done)
        if self.cifar:
            self._cifar_stem_backward(ws, dx)
        else:
            self._stem_backward(ws, dx)

    def _head_backward(self, ws, dlogits, done):
        v = self._v
        last = ws.blk[-1]["out"]
        Cl = last.shape[3]
        ones, zeros = v(ws, self.ones, Cl), v(ws, self.zeros, Cl)
        self._head_bwd(ws, dlogits, last, ones, zeros, zeros, ones, ones, ws.bwd["g"][-1], v(ws, self.scratch[0], Cl),
                       v(ws, self.scratch[1], Cl), 0, self.model.fc, ops.POOL_ACT_RELU, None, done)

    def _join_backward(self, ws, bi, rows=None):
        """Residual join backward of block bi: dz = dOut * [out > 0] in place in the block's gradient buffer g, with the backward
        sums of the last BatchNorm and S2 of the downsample BatchNorm, then their coefficients.  rows: the pass already ran, in the
        epilogue of the block above's conv1 input gradient (CX_EPI_JOIN), and left that many statistic rows."""
        v, b, t, g = self._v, self.blocks[bi], ws.blk[bi], ws.bwd["g"][bi]
        bn = self._last_bn(b)
        S, Sd = self.bn[id(bn)], self.bn[id(b.downsample[1])] if b.downsample is not None else None
        if rows is None:
            s1, s2, n_rows = self._ew(ws, S)
            rows = ops.relu_bwd_stats(g, t["out"], t["y2" if self.basic else "y3"], v(ws, S.mean), v(ws, S.rstd), t["yd"],
                                      v(ws, Sd.mean) if Sd else None, v(ws, Sd.rstd) if Sd else None, g, s1, s2,
                                      ws.slab[2] if Sd else None, stat_rows=n_rows, mask=t["mask"])
        ho, wo = t["hout"]
        self._bn_bwd(ws, bn, rows, ws.B * ho * wo)
        if Sd is not None:
            # the downsample BatchNorm shares S1 with the block's last BatchNorm (the same masked gradient), its S2 rows are
            # ws.slab[2]; its coefficients are taken here, before the next producer re-uses the rows
            self._bn_bwd(ws, b.downsample[1], rows, ws.B * ho * wo, s2=ws.slab[2])

    def _gx(self, ws, bi):
        """Where block bi's input gradient goes, and whether it is added there: an identity block's convolutions accumulate into
        the block's own gradient buffer g (which holds the identity path already), a downsample block writes the buffer of the block
        below."""
        bw, g, identity = ws.bwd, ws.bwd["g"][bi], self.blocks[bi].downsample is None
        gx = (bw["g"][bi - 1] if bi > 0 else bw["g_in0"]) if not identity or bi == 0 else g
        if identity and gx is not g:
            gx.copy_(g)                      # first block of layer1 never is an identity block; defensive
        return gx, identity

    def _aa_backward_front(self, ws, aa, t, dz, y, S):
        """Backward of an AAConv2d's attention branch down to its projection: out-projection (with BatchNorm S's backward of the
        gradient dz of [conv branch | attention] in its prologue), attention, dQKV in the storage type.  Returns dQKV and the
        channel range of the conv branch."""
        v, G, bw = self._v, self.grad_of, ws.bwd
        cc = dz.shape[3] - aa.dv
        dO = bw["dO"][:t["O"].numel()].view(t["O"].shape)
        dQ32 = bw["dQKV32"][:t["QKV"].numel()].view(t["QKV"].shape)
        dQ = bw["dQKV"][:t["QKV"].numel()].view(t["QKV"].shape)
        ops.aa_outproj_bwd(dz[..., cc:], y[..., cc:], v(ws, S.pa)[cc:], v(ws, S.pb)[cc:], v(ws, S.pc)[cc:], t["O"], aa.out_proj.weight, dO,
                           G(aa.out_proj.weight))
        ops.aa_attention_bwd(t["QKV"], *aa.rel_tables(), t["O"], dO, t["LSE"], dQ32, *aa.rel_grads(G), aa.nh, aa.dk, aa.dv)
        if self.dtype == torch.float32:
            dQ = dQ32
        else:
            ops.f32_to_bf16(dQ32, dQ)
        return dQ, slice(0, cc)

    def _down_backward(self, ws, b, t, g, gx, xin):
        """input and weight gradient of a downsample block's 1x1 stride-s convolution, BatchNorm backward in the prologues"""
        Sd, convd = self.bn[id(b.downsample[1])], b.downsample[0]
        ops.conv_gemm(g, self.w_bwd(convd), gx, N=self._cin(b), tstride=b.stride, **self._pro_bnbwd(ws, t["yd"], Sd), accumulate=True)
        ops.conv_wgrad(g, xin, self.grad_of(convd.weight), stride=b.stride, **self._g_bnbwd(ws, t["yd"], Sd))

    def _bottleneck_backward(self, ws, bi, join_rows, done):
        """Backward of one Bottleneck: the block's output gradient is masked in place by the join ReLU, BatchNorm backward rides in
        the two-tensor prologues of the consumers.  join_rows: see _join_backward; returns the same for the block below."""
        G, bw, B = self.grad_of, ws.bwd, ws.B
        b, t = self.blocks[bi], ws.blk[bi]
        p_, cin = b.bn1.num_features, self._cin(b)
        (hi, wi), (ho, wo) = t["hin"], t["hout"]
        xin = ws.blk[bi - 1]["out"] if bi > 0 else ws.pool0
        S1, S2, S3 = self.bn[id(b.bn1)], self.bn[id(b.bn2)], self.bn[id(b.bn3)]
        g = bw["g"][bi]
        self._join_backward(ws, bi, join_rows)
        dz2 = bw["dz2"][:B * ho * wo * p_].view(B, ho, wo, p_)
        rows = ops.conv_gemm(g, self.w_bwd(b.conv3), dz2, N=p_, **self._pro_bnbwd(ws, t["y3"], S3), **self._mask(ws, t["y2"], S2))
        ops.conv_wgrad(g, t["y2"], G(b.conv3.weight), **self._g_bnbwd(ws, t["y3"], S3), **self._x_bnrelu(ws, S2))
        self._bn_bwd(ws, b.bn2, rows, B * ho * wo)
        dz1 = bw["dz1"][:B * hi * wi * p_].view(B, hi, wi, p_)
        rows = self._conv2_backward(ws, b, t, dz2, dz1)
        self._bn_bwd(ws, b.bn1, rows, B * hi * wi)
        gx, identity = self._gx(ws, bi)
        prev = self.blocks[bi - 1] if bi > 0 else None
        join_rows = None
        if (self.join_fuse and identity and prev is not None and prev.downsample is None and cin % 128 == 0
                and self.dtype == torch.bfloat16):
            # dOut of the block below is complete with this launch (identity path already in gx): its join backward -- ReLU
            # mask from the forward's sign bits, bn3 sums -- runs in the epilogue instead of a pass of its own over gx
            tp, Sp = ws.blk[bi - 1], self.bn[id(prev.bn3)]
            join_rows = ops.conv_gemm(dz1, self.w_bwd(b.conv1), gx, N=cin, **self._pro_bnbwd(ws, t["y1"], S1), accumulate=True,
                                      epilogue=ops.EPI_JOIN, ex=tp["y3"], e_mu=self._v(ws, Sp.mean), e_r=self._v(ws, Sp.rstd),
                                      emask=tp["mask"], **self._sp(ws, Sp, bwd=True))
        else:
            ops.conv_gemm(dz1, self.w_bwd(b.conv1), gx, N=cin, **self._pro_bnbwd(ws, t["y1"], S1), accumulate=identity)
        ops.conv_wgrad(dz1, xin, G(b.conv1.weight), **self._g_bnbwd(ws, t["y1"], S1))
        if not identity:
            self._down_backward(ws, b, t, g, gx, xin)
        done(b.conv1.weight)
        return join_rows

    def _conv2_backward(self, ws, b, t, dz2, dz1):
        """Input gradient dz1 (through bn1's ReLU mask, with bn1's backward sums) and weight gradients of a Bottleneck's conv2 from
        dz2: the AAConv2d, or the 3x3 as one launch per group.  Returns the statistic rows."""
        G, s_, p_ = self.grad_of, b.stride, b.bn1.num_features
        S1, S2 = self.bn[id(b.bn1)], self.bn[id(b.bn2)]
        if isinstance(b.conv2, AAConv2d):
            aa = b.conv2
            dQ, c_ = self._aa_backward_front(ws, aa, t, dz2, t["y2"], S2)
            # both branches end in the same bn1 + ReLU mask: the conv branch writes dz1, the attention branch adds to it
            rows = ops.conv_gemm(dz2[..., c_], self.w_bwd(aa.conv), dz1, N=p_, kh=3, kw=3, pad=1, tstride=s_,
                                 **self._pro_bnbwd(ws, t["y2"], S2, c_), **self._mask(ws, t["y1"], S1))
            rows2 = ops.conv_gemm(dQ, self.w_bwd(aa.in_proj_qkv), dz1, N=p_, tstride=s_, accumulate=True,
                                  **self._mask(ws, t["y1"], S1, after=rows or 0))
            ops.conv_wgrad(dz2[..., c_], t["y1"], G(aa.conv.weight), kh=3, kw=3, stride=s_, pad=1, **self._g_bnbwd(ws, t["y2"], S2, c_),
                           **self._x_bnrelu(ws, S1))
            ops.conv_wgrad(dQ, t["y1"], G(aa.in_proj_qkv.weight), stride=s_, **self._x_bnrelu(ws, S1))
            return (rows or 0) + (rows2 or 0)
        # the input gradient's padding is (extent - 1) - forward padding = 2d - d = d at either stride: a dilated conv2 has stride 1
        # or, as layer3[0] under replace_stride_with_dilation = [True, False, True], stride 2 (tstride = 2 with taps d pixels apart)
        d_, gr = b.conv2.dilation[0], b.conv2.groups
        kg, ch = p_ // gr, self._ch
        n_w = kg * kg * 9
        for g_ in range(gr):
            c_, wg = (slice(g_ * kg, (g_ + 1) * kg), g_) if gr > 1 else (None, None)
            rows = ops.conv_gemm(ch(dz2, c_), self.w_bwd(b.conv2, wg), ch(dz1, c_), N=kg, kh=3, kw=3, pad=d_, dil=d_, tstride=s_,
                                 **self._pro_bnbwd(ws, t["y2"], S2, c_), **self._mask(ws, t["y1"], S1, c_))
            ops.conv_wgrad(ch(dz2, c_), ch(t["y1"], c_), G(b.conv2.weight)[g_ * n_w:(g_ + 1) * n_w], kh=3, kw=3, stride=s_, pad=d_, dil=d_,
                           **self._g_bnbwd(ws, t["y2"], S2, c_), **self._x_bnrelu(ws, S1, c_))
        return rows

    def _basic_backward(self, ws, bi, done):
        """Backward of one BasicBlock (attn_aug_conv.py:135-156), same conventions as the bottleneck path."""
        G, bw, B = self.grad_of, ws.bwd, ws.B
        b, t = self.blocks[bi], ws.blk[bi]
        s_, p_, cin = b.stride, b.bn1.num_features, self._cin(b)
        ho, wo = t["hout"]
        xin = ws.blk[bi - 1]["out"] if bi > 0 else ws.pool0
        S1, S2 = self.bn[id(b.bn1)], self.bn[id(b.bn2)]
        g = bw["g"][bi]
        self._join_backward(ws, bi)
        dz1 = bw["dz1"][:B * ho * wo * p_].view(B, ho, wo, p_)
        rows = ops.conv_gemm(g, self.w_bwd(b.conv2), dz1, N=p_, kh=3, kw=3, pad=1, **self._pro_bnbwd(ws, t["y2"], S2),
                             **self._mask(ws, t["y1"], S1))
        ops.conv_wgrad(g, t["y1"], G(b.conv2.weight), kh=3, kw=3, stride=1, pad=1, **self._g_bnbwd(ws, t["y2"], S2), **self._x_bnrelu(ws, S1))
        self._bn_bwd(ws, b.bn1, rows, B * ho * wo)
        gx, identity = self._gx(ws, bi)
        if isinstance(b.conv1, AAConv2d):
            aa = b.conv1
            dQ, c_ = self._aa_backward_front(ws, aa, t, dz1, t["y1"], S1)
            ops.conv_gemm(dz1[..., c_], self.w_bwd(aa.conv), gx, N=cin, kh=3, kw=3, pad=1, tstride=s_, **self._pro_bnbwd(ws, t["y1"], S1, c_),
                          accumulate=identity)
            ops.conv_gemm(dQ, self.w_bwd(aa.in_proj_qkv), gx, N=cin, tstride=s_, accumulate=True)
            ops.conv_wgrad(dz1[..., c_], xin, G(aa.conv.weight), kh=3, kw=3, stride=s_, pad=1, **self._g_bnbwd(ws, t["y1"], S1, c_))
            ops.conv_wgrad(dQ, xin, G(aa.in_proj_qkv.weight), stride=s_)
        else:
            ops.conv_gemm(dz1, self.w_bwd(b.conv1), gx, N=cin, kh=3, kw=3, pad=1, tstride=s_, **self._pro_bnbwd(ws, t["y1"], S1),
                          accumulate=identity)
            ops.conv_wgrad(dz1, xin, G(b.conv1.weight), kh=3, kw=3, stride=s_, pad=1, **self._g_bnbwd(ws, t["y1"], S1))
        if not identity:
            self._down_backward(ws, b, t, g, gx, xin)
        done(b.conv1.weight if not isinstance(b.conv1, AAConv2d) else b.conv1.first_param())

    def _stem_backward(self, ws, dx):
        """max-pool + ReLU + BatchNorm backward in one kernel, weight gradient of the 7x7 convolution, input gradient when asked"""
        m, v, G = self.model, self._v, self.grad_of
        S0, gx, dz0 = self.bn[id(m.bn1)], ws.bwd["g_in0"], ws.bwd["dz0"]
        s1, s2, n_rows = self._ew(ws, S0)
        rows = ops.bnrelu_maxpool_bwd(ws.c0, v(ws, S0.sc), v(ws, S0.sh), v(ws, S0.mean), v(ws, S0.rstd), ws.amax, gx, gx, v(ws, self.ones, 64),
                                      v(ws, self.zeros, 64), v(ws, self.zeros, 64), dz0, s1, s2, stat_rows=n_rows)
        self._bn_bwd(ws, m.bn1, rows, ws.B * (ws.H // 2) * (ws.W // 2))
        ops.conv_wgrad(dz0, ws.x4, G(m.conv1.weight), mode=ops.MODE_STEM, **self._g_bnbwd(ws, ws.c0, S0))
        if dx is not None:
            ops.stem_input_grad(dz0, ws.c0, v(ws, S0.pa), v(ws, S0.pb), v(ws, S0.pc), m.conv1.weight, dx, stride=2, pad=3)

    def _cifar_stem_backward(self, ws, dx):
        m, v, G = self.model, self._v, self.grad_of
        S0, gx, dz0 = self.bn[id(m.bn1)], ws.bwd["g_in0"], ws.bwd["dz0"]
        c0 = m.conv1.out_channels
        s1, s2, n_rows = self._ew(ws, S0)
        rows = ops.relu_bwd_stats(gx, ws.pool0, ws.c0, v(ws, S0.mean), v(ws, S0.rstd), None, None, None, dz0, s1, s2, None, stat_rows=n_rows)
        self._bn_bwd(ws, m.bn1, rows, ws.B * ws.H * ws.W)
        dw8 = torch.zeros(c0, 8, 3, 3, dtype=torch.float32, device=self.device)       # 3 input channels padded to 8
        ops.conv_wgrad(dz0, ws.x8, dw8, kh=3, kw=3, stride=1, pad=1, **self._g_bnbwd(ws, ws.c0, S0))
        G(m.conv1.weight).view(c0, 3, 3, 3).add_(dw8[:, :3])
        if dx is not None:
            ops.stem_input_grad(dz0, ws.c0, v(ws, S0.pa), v(ws, S0.pb), v(ws, S0.pc), m.conv1.weight, dx, stride=1, pad=1)


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
