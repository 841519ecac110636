"""DenseNet (torchvision-shaped) whose forward / backward run on the hand-written gfx950 kernels.

Drop-in surface: constructor signature of
/root/reference/models/attn_aug_conv.py:452-453, torchvision `state_dict` key names and OIHW fp32
shapes, `model.features.norm5`, `model.classifier` (re-assignable), `.train()/.eval()`, autograd through
`loss.backward()`.  What differs is *how* `model(x)` executes: not module by module through ATen, but
as one schedule of fused kernels over NHWC bf16 buffers:

  * each dense block lives in ONE (B,H,W,C_total) buffer; layers write their 32 new channels into a
    slice (the reference's torch.cat never happens);
  * BatchNorm batch statistics of a buffer channel are accumulated once, by the kernel that produces
    the channel; every later norm1 over the concatenation re-uses them (same data => same mean/var),
    only gamma/beta differ;
  * BN + ReLU are applied in the consumer's operand prologue, never stored;
  * transition: avg-pool is applied before the 1x1 conv (they commute), 4x fewer MACs;
  * backward: the -mean(dz) - xhat*mean(dz*xhat) terms of every consumer BatchNorm are linear in x and
    share xhat, so they are accumulated as two per-channel coefficients and applied once by the
    channel's producer; the gradient buffer only receives gamma*rstd*dz contributions.
"""
import os
from collections import OrderedDict

import torch
import torch.nn as nn

from .. import ops
from ._fused import FusedEngine, FusedNet, _Vec, flatten


# --------------------------------------------------------------------------------------------- parameter containers
class _FusedOnly:
    def forward(self, *a, **k):  # pragma: no cover - guard
        raise RuntimeError("chexpert_amd: this sub-module only holds parameters; call the parent model "
                           "(the fused HIP schedule).  There is no module-by-module fallback.")


class Conv2dParams(_FusedOnly, nn.Conv2d):
    pass


class BatchNorm2dParams(_FusedOnly, nn.BatchNorm2d):
    pass


class ReLUMarker(_FusedOnly, nn.ReLU):
    pass


class PoolMarker(_FusedOnly, nn.Module):
    pass


class _DenseLayer(nn.Sequential):
    def __init__(self, cin, growth, bn_size):
        super().__init__()
        self.add_module("norm1", BatchNorm2dParams(cin))
        self.add_module("relu1", ReLUMarker(inplace=True))
        self.add_module("conv1", Conv2dParams(cin, bn_size * growth, 1, 1, bias=False))
        self.add_module("norm2", BatchNorm2dParams(bn_size * growth))
        self.add_module("relu2", ReLUMarker(inplace=True))
        self.add_module("conv2", Conv2dParams(bn_size * growth, growth, 3, 1, 1, bias=False))


class _DenseBlock(nn.Sequential):
    def __init__(self, n_layers, cin, bn_size, growth):
        super().__init__()
        for i in range(n_layers):
            self.add_module("denselayer%d" % (i + 1), _DenseLayer(cin + i * growth, growth, bn_size))


class InstanceNormMarker(_FusedOnly, nn.InstanceNorm2d):
    pass


class AAConv2d(nn.Module):
    """Parameter holder with the constructor / attributes of /root/reference/models/attn_aug_conv.py:19-41
    (`dk`, `dv`, `nh`, `relative`, `conv`, `in_proj_qkv`, `out_proj`, `key_rel_h`, `key_rel_w`).  The arithmetic runs in
    csrc/aaconv.hip + the implicit-GEMM kernels as part of the parent model's fused schedule."""

    def __init__(self, in_channels, out_channels, kernel_size, stride, dk, dv, nh, relative, input_dims, **kwargs):
        super().__init__()
        assert dk % nh == 0, "nh must divide dk"
        assert dv % nh == 0, "nh must divide dv"
        # every configuration of the reference is constructible (parameter shapes, state_dict keys: the parameter-count
        # self-test of attn_aug_conv.py:522-655).  The HIP attention kernels cover head widths dk/nh and dv/nh of 1 .. 64 with
        # dv <= 104 (the out-projection) -- the row kernels for dk/nh = 20, dv/nh <= 13 (what chexpert.py trains; relative=False
        # runs too), the runtime-width kernels of csrc/aaconv_heads.hip for the rest -- and the qkv projection and the convolution
        # branch need multiples of 8 channels (conv_gemm).  Anything else raises when the model is RUN, not when it is built.
        self.dk, self.dv, self.nh, self.relative = dk, dv, nh, relative
        self.out_channels = out_channels
        self.kernel_support = not self.unsupported()
        padding = kwargs.pop("padding", None) or kernel_size // 2
        self.conv = Conv2dParams(in_channels, out_channels - dv, kernel_size, stride, padding, bias=False, **kwargs) \
            if out_channels > dv else None
        self.in_proj_qkv = Conv2dParams(in_channels, 2 * dk + dv, 1, stride, bias=False)
        self.out_proj = Conv2dParams(dv, dv, 1, bias=False)
        H, W = input_dims
        self.input_dims = (H, W)
        if relative:
            self.key_rel_h = nn.Parameter(dk ** -0.5 + torch.randn(dk // nh, 2 * H - 1))
            self.key_rel_w = nn.Parameter(dk ** -0.5 + torch.randn(dk // nh, 2 * W - 1))
        else:
            # relative=False (attn_aug_conv.py:77-78 skipped): the kernels run with all-zero position tables -- the same logits --
            # and their table gradients go to a scratch pair; neither is a parameter or part of the state_dict
            for nm, n in (("h", 2 * H - 1), ("w", 2 * W - 1)):
                self.register_buffer("_rel0_" + nm, torch.zeros(dk // nh, n), persistent=False)
                self.register_buffer("_drel0_" + nm, torch.zeros(dk // nh, n), persistent=False)
        self._last = None        # (qkv, lse) of the most recent forward, set by the parent model's engine

    def unsupported(self, branch_aligned=True):
        """The conditions of the HIP kernels this layer fails, as text ('' when it runs).  branch_aligned=False: the convolution
        branch is padded to a multiple of 8 channels by the caller (the channel-padded CIFAR DenseNet-BC)."""
        dkh, dvh, dk, dv = self.dk // self.nh, self.dv // self.nh, self.dk, self.dv
        why = []
        if not 1 <= dkh <= 64:
            why.append("dk/nh = %d is outside 1 .. 64" % dkh)
        if not 1 <= dvh <= 64:
            why.append("dv/nh = %d is outside 1 .. 64" % dvh)
        if dv > 104:
            why.append("dv = %d is above 104 (the out-projection kernels)" % dv)
        if self.out_channels <= dv:
            why.append("out_channels = %d leaves no convolution branch beside dv = %d" % (self.out_channels, dv))
        if (2 * dk + dv) % 8:
            why.append("2dk+dv = %d qkv channels are not a multiple of 8" % (2 * dk + dv))
        if branch_aligned and self.out_channels > dv and (self.out_channels - dv) % 8:
            why.append("out_channels-dv = %d convolution channels are not a multiple of 8" % (self.out_channels - dv))
        return "; ".join(why)

    def check_supported(self, branch_aligned=True):
        """Raises NotImplementedError naming what unsupported() finds."""
        why = self.unsupported(branch_aligned)
        if why:
            raise NotImplementedError("AAConv2d(dk=%d, dv=%d, nh=%d, relative=%s): %s (the HIP attention kernels cover dk/nh and "
                                      "dv/nh = 1 .. 64 with dv <= 104)" % (self.dk, self.dv, self.nh, self.relative, why))

    def rel_tables(self):
        return (self.key_rel_h, self.key_rel_w) if self.relative else (self._rel0_h, self._rel0_w)

    def rel_grads(self, G):
        """where the kernels add the position tables' gradients (G: parameter -> its view in the flat gradient buffer)"""
        return (G(self.key_rel_h), G(self.key_rel_w)) if self.relative else (self._drel0_h, self._drel0_w)

    def first_param(self):
        """the module's first parameter in named_parameters() order (its own before its children's)"""
        return next(self.parameters())

    def forward(self, x):  # pragma: no cover - guard
        raise RuntimeError("chexpert_amd: AAConv2d only holds parameters; call the parent model (fused HIP schedule)")

    @property
    def weights(self):
        """softmax(logits) of the most recent forward, (B, nh, HW, HW) fp32 -- what the reference stores here on every forward
        (attn_aug_conv.py:87) and `vis_attn` reads as `l.weights.data[b]` (chexpert.py:383).  The training path never builds
        the HW x HW tensor; it is rebuilt on access from the saved q/k and log-sum-exp (82 MB per image at 40x40)."""
        if self._last is None:
            return None
        qkv, lse = self._last
        return ops.aa_attention_weights(qkv, *self.rel_tables(), lse, self.nh, self.dk, self.dv)

    def extra_repr(self):
        return "dk={}, dv={}, nh={}, relative={}".format(self.dk, self.dv, self.nh, self.relative)


class _Transition(nn.Sequential):
    def __init__(self, cin, cout, attn_params=None):
        super().__init__()
        if attn_params is None:
            self.add_module("norm", BatchNorm2dParams(cin))
            self.add_module("relu", ReLUMarker(inplace=True))
            self.add_module("conv", Conv2dParams(cin, cout, 1, 1, bias=False))
            self.add_module("pool", PoolMarker())
        else:                                   # attn_aug_conv.py:416-440: InstanceNorm -> ReLU -> AAConv2d(3x3, stride 2)
            nh = attn_params["nh"]
            dk = max(20 * nh, int((attn_params["k"] * cout // nh) * nh))
            dv = int((attn_params["v"] * cout // nh) * nh)
            dims = (attn_params["input_dims"][0] // 2, attn_params["input_dims"][1] // 2)
            self.add_module("norm", InstanceNormMarker(cin))
            self.add_module("relu", ReLUMarker(inplace=True))
            self.add_module("conv", AAConv2d(cin, cout, 3, 2, dk, dv, nh, attn_params["relative"], dims))


# --------------------------------------------------------------------------------------------- workspace
class _Workspace:
    """Activation buffers + coefficient vectors for one (B,H,W); owned by one in-flight forward."""

    def __init__(self, eng, B, H, W, dev):
        bf, u8 = eng.dtype, torch.uint8         # activation storage type: bf16, or fp32 in the parity mode
        self.key = (B, H, W)
        self.B, self.H, self.W = B, H, W
        g = eng.growth
        e = lambda *s, dtype=bf: torch.empty(*s, dtype=dtype, device=dev)
        if eng.cifar:                       # 5x5 stride-1 stem, no pooling: block 1 works on the input's own grid
            self.x8 = e(B, H, W, 8)
            h, w = H, W
            self.c0 = e(B, h, w, eng.c_init)
            self.dz0 = None
            self.amax = None
        else:
            self.x4 = e(B, H, W, 4)
            h, w = H // 2, W // 2
            self.c0 = e(B, h, w, eng.c_init)
            self.dz0 = None
            h, w = h // 2, w // 2
            self.amax = e(B, h, w, eng.c_init, dtype=u8)
        self.buf, self.gbuf, self.y1, self.hw = [], [], [], []
        for bi, (c_in, n_layers) in enumerate(eng.blocks):
            ct = c_in + n_layers * g
            # (twin of a CIFAR DenseNet-BC: the channels between an attention-augmented transition's output and the padded block
            # entry are written by nobody and must read as zero)
            self.buf.append(torch.zeros(B, h, w, ct, dtype=bf, device=dev) if eng.cifar else e(B, h, w, ct))
            self.gbuf.append(None)
            self.y1.append([e(B, h, w, eng.mid) for _ in range(n_layers)])
            self.hw.append((h, w))
            h, w = h // 2, w // 2
        self.dz2 = None
        self.dpool = None
        self.aa = {}
        f32 = torch.float32
        for bi, (c_in, n_layers) in enumerate(eng.blocks[:-1]):
            aa = getattr(eng.model.features, "transition%d" % (bi + 1)).conv
            if not isinstance(aa, AAConv2d):
                continue
            ct = c_in + n_layers * g
            (hh, wh), (ho, wo) = self.hw[bi], self.hw[bi + 1]
            if (ho, wo) != tuple(aa.input_dims):
                raise RuntimeError("AAConv2d was built for %s feature maps, the input gives %s (relative tables are size-bound, "
                                   "attn_aug_conv.py:38-41)" % (tuple(aa.input_dims), (ho, wo)))
            T = type("AAWs", (), {})()
            T.stat = torch.zeros(2, B * ct, dtype=f32, device=dev)
            T.coef = torch.zeros(2, B * ct, dtype=f32, device=dev)
            T.A = e(B, hh, wh, ct)
            T.QKV = e(B, ho, wo, 2 * aa.dk + aa.dv)
            T.O = torch.empty(B, ho * wo, aa.dv, dtype=f32, device=dev)
            T.LSE = torch.empty(B * aa.nh, ho * wo, dtype=f32, device=dev)
            T.bwd = None
            self.aa[bi] = T
        self.pooled = torch.empty(B, eng.c_final, dtype=torch.float32, device=dev)
        self.logits = torch.empty(B, eng.n_classes, dtype=torch.float32, device=dev)
        self.vec = torch.zeros(eng.vec_size, dtype=torch.float32, device=dev)
        self.ones = torch.ones(max(eng.mid, 64, eng.c_init), dtype=torch.float32, device=dev)
        self.zeros = torch.zeros(max(eng.growth, 8), dtype=torch.float32, device=dev)
        # deterministic statistics (CxConv.stat_det): every producer writes per-workgroup rows into this scratch pair and the
        # coefficient kernel that follows on the same stream sums them in row order
        self.slab = torch.empty(2, eng.SLAB, dtype=torch.float32, device=dev)

    def alloc_backward(self, eng, dev):
        if self.dz0 is not None:
            return
        bf = eng.dtype
        B = self.B
        self.dz0 = torch.empty_like(self.c0)
        self.gbuf = [torch.empty_like(b) for b in self.buf]
        h, w = self.hw[0]
        self.dz2 = [torch.empty(B, h, w, eng.mid, dtype=bf, device=dev) for _ in range(2)]
        # dense copies of the layers' corrected output-gradient slices (CxConv.pro_out of the 3x3 input-gradient kernel, a bf16
        # kernel): one per layer, a block's batched 3x3 weight gradient reads them all after the block's last layer
        self.dyc = None
        if bf == torch.bfloat16:
            self.dyc = [[torch.empty(B, hh, ww, eng.growth, dtype=bf, device=dev) for _ in range(nl)]
                        for (hh, ww), nl in zip(self.hw, eng.model.block_config)]
        if len(self.buf) > 1:
            n = max(self.hw[i + 1][0] * self.hw[i + 1][1] * self.buf[i].shape[3] for i in range(len(self.buf) - 1))
            self.dpool = torch.empty(B * n, dtype=bf, device=dev)
        for bi, T in self.aa.items():
            T.dO = torch.empty_like(T.O)
            T.dQKV32 = torch.empty(T.QKV.shape, dtype=torch.float32, device=dev)
            T.dQKV = torch.empty_like(T.QKV)
            T.dA = torch.empty_like(T.A)
            T.S = torch.zeros_like(T.stat)


# --------------------------------------------------------------------------------------------- engine
class _Slots:
    """A record of named vector slots.  C: the channels of the BatchNorm it serves; such a record carries the field names of a
    `_fused._BN` as far as it has them (sc, sh, mean, rstd, pa, pb, pc), so the operand helpers take either."""

    def __init__(self, C=None, **slots):
        self.C = C
        self.__dict__.update(slots)


class _Engine(FusedEngine):
    """Host-side schedule: issues the kernel sequence of forward and backward on the current stream."""
    SLAB = 1 << 22               # floats per half of the statistic-row scratch (rows x channels of the largest producer)
    EW_ROWS = 2048               # workgroups (= rows) of the element-wise statistic producers

    # ---- statistics plumbing: every producer of a BatchNorm's sums writes one row per workgroup into ws.slab[0] / ws.slab[1], at
    # the pitch of the C channels it produces, and returns the number of rows; the coefficient kernel that follows sums them in row
    # order.  Named as in the ResNet engine: keywords of a convolution producer (_sp), (sum, sq, stat_rows) of an element-wise
    # producer (_ew), (sum, sq, replicas, rstride) for the consumer (_sc).  A forward producer has none in an eval forward (`bwd`: the
    # backward sums S1 / S2, which the frozen backward takes too)
    def _ew_rows(self, C):
        return min(self.EW_ROWS, self.SLAB // C)

    def _sp(self, ws, C, bwd=False):
        if ws.frozen and not bwd:
            return {}
        return dict(stat_sum=ws.slab[0], stat_sq=ws.slab[1], stat_det=True, stat_replicas=self.SLAB // C, stat_rstride=C)

    def _ew(self, ws, C, bwd=False, rows=None):
        if ws.frozen and not bwd:
            return None, None, 0
        return ws.slab[0], ws.slab[1], rows or self._ew_rows(C)

    @staticmethod
    def _sc(ws, C, rows):
        return ws.slab[0], ws.slab[1], rows, C

    def _fresh(self, ws, rows, lo, n):
        """The pending statistic rows of a block buffer's newest channels [lo, lo + n), as cx_bn_coef_moments takes them: the next
        BatchNorm over the buffer reduces them (training forward; None otherwise)."""
        return None if ws.frozen else (ws.slab[0], ws.slab[1], rows, n, lo, n)

    # ---- operand keywords that are DenseNet's own (FusedEngine has those of a BatchNorm record)
    @staticmethod
    def _pro_slice(xs, q):
        """input gradient: the deferred BatchNorm correction of a gradient slice, dY = dy * qa + x * qb + qc (q: _slice_q)"""
        return dict(prologue=ops.PRO_AFFINE2, x2=xs, pa=q[0], pb=q[1], pc=q[2])

    @staticmethod
    def _g_slice(xs, q):
        """weight gradient: the same of its gradient operand"""
        return dict(g_prologue=ops.PRO_AFFINE2, g2=xs, ga=q[0], gb=q[1], gc=q[2])

    def _mask(self, ws, y, S, by_sc=False, c_=None, stat=None):
        """input gradient: the epilogue that masks with [relu(bn_S(y)) > 0] and produces BatchNorm S's backward sums.  The masked
        gradient is scaled by one (conv2's form: norm2, norm0) or, by_sc, by S's scale (conv1's form: a norm1, whose mean / rstd
        are the block's and whose gain the shared xhat terms leave out).  c_: a range of S's channels; stat: the statistics
        keywords, where they are not _sp's (the regions of _pair_backward)."""
        ch, v = self._ch, self._v
        return dict(epilogue=ops.EPI_MASK, ex=ch(y, c_), e_sc=ch(v(ws, S.sc), c_), e_sh=ch(v(ws, S.sh), c_), e_mu=ch(v(ws, S.mean), c_),
                    e_r=ch(v(ws, S.rstd), c_), e_scale=ch(v(ws, S.sc), c_) if by_sc else ws.ones[:S.C],
                    **(self._sp(ws, S.C, bwd=True) if stat is None else stat))

    def __init__(self, model):
        super().__init__(model)
        f = model.features
        self.growth = model.growth_rate
        self.mid = getattr(model, "_mid", None) or model.bn_size * model.growth_rate
        self.c_init = f.conv0.out_channels
        # CIFAR form of the network (attn_aug_conv.py:469-474): 5x5 stride-1 stem without pooling, any number of blocks
        self.cifar = not hasattr(f, "pool0")
        self.blocks = []
        c = self.c_init
        for n_layers in model.block_config:
            self.blocks.append((c, n_layers))
            c = c + n_layers * self.growth
            if len(self.blocks) != len(model.block_config):
                # (the width the next block starts from: c // 2 in the reference's networks; the channel-padded twin of a CIFAR
                # DenseNet-BC rounds it up, and pads between the two branches of an attention-augmented transition)
                c = getattr(f, "denseblock%d" % (len(self.blocks) + 1)).denselayer1.norm1.num_features
        self.c_final = c
        # Statistics are per-workgroup rows summed in a fixed order (bit-identical activations, losses and gradients from run to
        # run).  The AA transitions feed a block's first channels from two kernels -- conv branch and attention out-projection:
        # their statistic rows are reduced one after the other, see _aa_forward.
        self.drop_rate = float(getattr(model, "drop_rate", 0.0))
        self.drop_seed = None        # device int64: the dropout kernels' seed, advanced once per training forward (graph-replayable)
        # two dense layers per fused 1x1 backward pass (_pair_backward): "0" never (default: measured in round 4, the pass saves
        # 20-30 % of the two layers' kernel time but the later layer's 32-channel slice launch, which has to read its dZ a second
        # time, and the two extra small launches per pair give it back -- 27.27 vs 27.22 ms per step, interleaved A/B on one box,
        # profiles/r04_pair_bwd.txt), "1" where the kernels alone gain (see _backward), "all" wherever two layers remain (tests)
        self.pair_bwd = os.environ.get("CHEXPERT_PAIR_BWD", "0")
        self._w2_items = []          # a block's 3x3 weight gradients, collected for one launch (_flush_w2)
        self._plan_vectors()

    # ---- coefficient-vector layout
    def _plan_vectors(self):
        """Carves the coefficient vector into self.plan: .stem (norm0's sc / sh / mean / rstd), .blocks -- per block its channels'
        mean / rstd, the exit norm's (transition norm, norm5) sc / sh, the accumulators A / Bc of the deferred BatchNorm terms, and
        .layers --, per layer .n1 (sc, sh; mean / rstd are the block's, cut to the layer's input channels), .n2 (sc, sh, mean, rstd,
        pa / pb / pc) and the slice triple qa / qb / qc of the layer's output channels; .q and .p: the shared triples of a block's
        first channels and of norm0 (the stem's pa / pb / pc are .p cut to its channels).  No sums live here: they are rows of
        ws.slab.  The takes keep one order, whatever record files them: the layout is [forward coefficients | A / Bc, zeroed
        every backward | backward coefficients]."""
        V, g_, mid, ci = _Vec(), self.growth, self.mid, self.c_init
        self._spans = []

        def take(n):
            self._spans.append(V.take(n))
            return self._spans[-1]
        per_block = lambda n_of, k: [[take(n_of(c, n)) for _ in range(k)] for c, n in self.blocks]
        per_layer = lambda n_of, k: [[[take(n_of(c, i)) for _ in range(k)] for i in range(n)] for c, n in self.blocks]
        ct, cin, mid_, g__ = (lambda c, n: c + n * g_), (lambda c, i: c + i * g_), (lambda c, i: mid), (lambda c, i: g_)
        n0 = [take(ci) for _ in range(4)]
        bmr, n1, n2, nt = per_block(ct, 2), per_layer(cin, 2), per_layer(mid_, 4), per_block(ct, 2)
        b0 = V.n
        AB = per_block(ct, 2)
        self.bwd_zero = (b0, V.n - b0)                                     # the backward accumulates into A / Bc
        # per-layer AFFINE2 vectors (the two-layer pass of _pair_backward holds both its layers' norm2 vectors at once)
        ql, pl = per_layer(g__, 3), per_layer(mid_, 3)
        q = [take(max(mid, ci, max(c for c, _ in self.blocks))) for _ in range(3)]         # slice AFFINE2
        p = [take(max(mid, ci)) for _ in range(3)]                                         # norm2 AFFINE2
        names = lambda keys, *lists: dict(zip(keys.split(), (t for l in lists for t in l)))
        blocks = []
        for bi, (c, n) in enumerate(self.blocks):
            layers = [_Slots(n1=_Slots(cin(c, i), mean=(bmr[bi][0][0], cin(c, i)), rstd=(bmr[bi][1][0], cin(c, i)), **names("sc sh", n1[bi][i])),
                             n2=_Slots(mid, **names("sc sh mean rstd pa pb pc", n2[bi][i], pl[bi][i])),
                             **names("qa qb qc", ql[bi][i])) for i in range(n)]
            blocks.append(_Slots(ct(c, n), layers=layers, **names("mean rstd sc sh A Bc", bmr[bi], nt[bi], AB[bi])))
        stem = _Slots(ci, **names("sc sh mean rstd pa pb pc", n0, [(t[0], ci) for t in p]))
        self.plan = _Slots(stem=stem, blocks=blocks, q=_Slots(**names("qa qb qc", q)), p=_Slots(**names("pa pb pc", p)), dpooled=take(0))
        self.vec_size = V.n

    def vector_slots(self):
        """Every (offset, length) span of the coefficient vector that the plan handed out."""
        return iter(self._spans)

    def norm5_operands(self, ws):
        """(last block buffer, norm5 scale, norm5 shift) of a workspace: relu(buffer * scale + shift) is what the head pools."""
        last = self.plan.blocks[-1]
        return ws.buf[-1], self._v(ws, last.sc), self._v(ws, last.sh)

    # ---- parameter binding
    def bind(self, dev):
        if self.bound(dev):
            return
        m = self.model
        if m.classifier.in_features != self.c_final:
            raise RuntimeError("classifier.in_features must be %d" % self.c_final)
        self.bind_params(dev)
        self.n_classes = m.classifier.out_features
        # packing table: every conv weight, forward layout (+ transposed layout for input gradients)
        f = m.features
        self.plan_packing([mod for mod in f.modules() if isinstance(mod, nn.Conv2d) and mod is not f.conv0], stem=f.conv0,
                          stem_layout=not self.cifar)
        # CIFAR stem: norm0 + relu0 write the first channels of block 1's buffer through a 1x1 identity convolution (BN + ReLU in
        # its prologue, the block's statistic rows from its epilogue); its backward is the same convolution with the mask epilogue
        self.eye = torch.eye(self.c_init, dtype=self.dtype, device=dev).reshape(-1) if self.cifar else None

    def _new_workspace(self, B, H, W):
        return _Workspace(self, B, H, W, self.device)

    def _aa_transition(self, t):
        """The AAConv2d of transition t (the one that feeds block t, 0-based); None for a BatchNorm transition, the stem (t = 0) and
        the head (t = number of blocks)."""
        tr = getattr(self.model.features, "transition%d" % t, None)
        return tr.conv if tr is not None and isinstance(tr.conv, AAConv2d) else None

    def _layer(self, bi, li):
        return getattr(getattr(self.model.features, "denseblock%d" % (bi + 1)), "denselayer%d" % (li + 1))

    @staticmethod
    def _count(buf):
        """values per channel of an NHWC buffer"""
        return buf.shape[0] * buf.shape[1] * buf.shape[2]

    # ---- forward
    def _bn(self, ws, S, bn, count, rows=None):
        """scale / shift / mean / rstd of BatchNorm `bn` into its record S, from the `rows` statistic rows of its input; an eval
        forward takes the running statistics."""
        v = self._v
        out = v(ws, S.sc), v(ws, S.sh), v(ws, S.mean), v(ws, S.rstd), S.C
        if ws.frozen:
            ops.bn_coef_eval(bn.running_mean, bn.running_var, bn.weight, bn.bias, bn.eps, *out)
        else:
            ops.bn_coef(ws.slab[0], ws.slab[1], count, *self._bn_train(bn), *out, replicas=rows, rstride=S.C)

    def _bn_block(self, ws, blk, S, bn, count, fresh):
        """BatchNorm over the first S.C channels of the buffer of block `blk` (S: the .n1 of a dense layer, or blk itself for its
        transition norm / norm5).  Batch moments of a buffer channel exist once (blk.mean / rstd): only the `fresh` channels --
        those the previous launch produced -- are reduced, from their statistic rows."""
        v = self._v
        if ws.frozen:
            return self._bn(ws, S, bn, count)
        ops.bn_coef_moments(v(ws, S.mean), v(ws, S.rstd), count, *self._bn_train(bn), v(ws, S.sc), v(ws, S.sh), S.C, fresh)

    def forward(self, x, train, record=False):
        """train: batch statistics, dropout; eval: running statistics.  Every forward keeps what backward reads (block buffers,
        bottleneck outputs, max-pool arg-max, attention log-sum-exp), so `record` changes nothing here.  An eval forward leaves each
        block's mean / rstd at the running statistics of the block's LAST BatchNorm consumer (transition norm, norm5; the last
        layer's norm1 before an attention transition): the basis of the frozen backward's sums.
        `fresh`, the pending statistic rows of the newest slice (_fresh), goes from each step to the next."""
        u8 = x.dtype == torch.uint8             # decoded grey bytes (B,1,H,W): whitened + expanded on the GPU (cx_u8_to_nhwc4)
        if x.dim() != 4 or x.shape[1] != (1 if u8 else 3):
            raise RuntimeError("expected a (B,3,H,W) float input or a (B,1,H,W) uint8 image")
        B, _, H, W = x.shape
        if self.cifar:
            mult = 1 << (len(self.blocks) - 1)
            if u8 or H % mult or W % mult:
                raise RuntimeError("the CIFAR-stem network takes (B,3,H,W) float images with H, W multiples of %d" % mult)
        elif H % 32 or W % 32:
            raise RuntimeError("input height/width must be multiples of 32 (got %dx%d)" % (H, W))
        self.bind(x.device)
        self.pack(train or record)          # (a step that differentiates repacks, as training does: a fused optimiser bumps no version)
        ws = self.acquire(B, H, W)
        self.recorded(ws, train, True)
        rows = self._cifar_stem_forward(ws, x) if self.cifar else self._stem_forward(ws, x)
        fresh = self._fresh(ws, rows, 0, self.c_init)
        if train and self.drop_rate > 0:
            if self.drop_seed is None:
                rank = torch.distributed.get_rank() if torch.distributed.is_available() and torch.distributed.is_initialized() else 0
                self.drop_seed = torch.tensor([(torch.initial_seed() + (rank << 40)) & 0x7fffffffffffffff], dtype=torch.int64,
                                              device=x.device)
            self.drop_seed.add_(1)
        last = len(self.blocks) - 1
        for bi, (_, n_layers) in enumerate(self.blocks):
            for li in range(n_layers):
                fresh = self._layer_forward(ws, bi, li, fresh)
            if bi == last:
                self._head_forward(ws, bi, fresh)
            elif self._aa_transition(bi + 1) is not None:
                fresh = self._aa_forward(ws, bi, fresh)
            else:
                fresh = self._transition_forward(ws, bi, fresh)
        if train and self.track_stats:
            self.model._nbt_pending += 1
        return ws

    def _stem_forward(self, ws, x):
        """conv0 -> norm0 -> relu0 -> pool0 of the ImageNet form (attn_aug_conv.py:460-465) into block 1's first channels.  Returns
        their statistic rows."""
        f, S, ci = self.model.features, self.plan.stem, self.c_init
        if x.dtype == torch.uint8:
            ops.u8_to_nhwc4(x.contiguous(), ws.x4)
        else:
            ops.nchw3_to_nhwc4(x.contiguous().float(), ws.x4)
        rows = ops.conv_gemm(ws.x4, self.w_fwd(f.conv0), ws.c0, N=ci, mode=ops.MODE_STEM, **self._sp(ws, ci))
        self._bn(ws, S, f.norm0, self._count(ws.c0), rows)
        return ops.bnrelu_maxpool_fwd(ws.c0, self._v(ws, S.sc), self._v(ws, S.sh), ws.buf[0][..., :ci], ws.amax, *self._ew(ws, ci))

    def _cifar_stem_forward(self, ws, x):
        """conv0 (5x5, stride 1, pad 2) -> norm0 -> relu0 of the CIFAR form (attn_aug_conv.py:469-474).  The image is held with 8
        channels (3 + zeros), conv0 runs on the generic implicit GEMM; norm0 + relu0 ride in the prologue of a 1x1 identity
        convolution that writes block 1's first channels.  Returns their statistic rows."""
        f, S, ci = self.model.features, self.plan.stem, self.c_init
        ops.nchw3_to_nhwc8(x.contiguous().float(), ws.x8)
        rows = ops.conv_gemm(ws.x8, self.w_fwd(f.conv0), ws.c0, N=ci, kh=5, kw=5, pad=2, **self._sp(ws, ci))
        self._bn(ws, S, f.norm0, self._count(ws.c0), rows)
        return ops.conv_gemm(ws.c0, self.eye, ws.buf[0][..., :ci], N=ci, **self._pro_bnrelu(ws, S), **self._sp(ws, ci))

    def _layer_forward(self, ws, bi, li, fresh):
        """Dense layer li of block bi: norm1's coefficients, conv1 into the bottleneck buffer, norm2's coefficients, conv2 into the
        layer's slice of the block buffer (and the dropout on it).  Returns the slice's pending statistic rows."""
        blk, layer, g_ = self.plan.blocks[bi], self._layer(bi, li), self.growth
        L = blk.layers[li]
        buf, y1, cin = ws.buf[bi], ws.y1[bi][li], L.n1.C
        cnt = self._count(buf)
        drop = self.drop_rate > 0 and not ws.frozen
        self._bn_block(ws, blk, L.n1, layer.norm1, cnt, fresh)
        rows = ops.conv_gemm(buf[..., :cin], self.w_fwd(layer.conv1), y1, N=self.mid, **self._pro_bnrelu(ws, L.n1), **self._sp(ws, self.mid))
        self._bn(ws, L.n2, layer.norm2, cnt, rows)
        rows = ops.conv_gemm(y1, self.w_fwd(layer.conv2), buf[..., cin:cin + g_], N=g_, kh=3, kw=3, pad=1, **self._pro_bnrelu(ws, L.n2),
                             **({} if drop else self._sp(ws, g_)))
        if drop:
            # dropout on the new slice, in place; its statistic rows are those of the dropped-out values (what every later
            # BatchNorm of the block sees)
            rows = ops.dropout_slice_fwd(buf[..., cin:cin + g_], self.drop_rate, self.drop_seed, bi * 256 + li, *self._ew(ws, g_))
        return self._fresh(ws, rows, cin, g_)

    def _transition_forward(self, ws, bi, fresh):
        """BatchNorm transition after block bi: the norm's coefficients, then ReLU -> 2x2 average pool -> 1x1 convolution (in that
        order: they commute) into the first channels of block bi + 1.  Returns their pending statistic rows."""
        blk, tr = self.plan.blocks[bi], getattr(self.model.features, "transition%d" % (bi + 1))
        cn = self.blocks[bi + 1][0]          # channels the transition produces (half the block's in the reference's networks)
        self._bn_block(ws, blk, blk, tr.norm, self._count(ws.buf[bi]), fresh)
        rows = ops.conv_gemm(ws.buf[bi], self.w_fwd(tr.conv), ws.buf[bi + 1][..., :cn], N=cn, mode=ops.MODE_POOL2,
                             **self._pro_bnrelu(ws, blk), **self._sp(ws, cn))
        return self._fresh(ws, rows, 0, cn)

    def _head_forward(self, ws, bi, fresh):
        """norm5's coefficients, then the shared head (FusedEngine._head_fwd) behind ReLU."""
        m, blk = self.model, self.plan.blocks[bi]
        self._bn_block(ws, blk, blk, m.features.norm5, self._count(ws.buf[bi]), fresh)
        self._head_fwd(ws, ws.buf[bi], self._v(ws, blk.sc), self._v(ws, blk.sh), m.classifier, ops.POOL_ACT_RELU)

    def _aa_forward(self, ws, bi, fresh):
        """InstanceNorm -> ReLU -> AAConv2d(3x3, stride 2) from block buffer bi into the first channels of buffer bi+1.  No BatchNorm
        consumes block bi, whose mean / rstd backward still reads: the moments of its last slice are finished here.  Returns the
        pending statistic rows of the attention channels (a training forward), which the next norm1 reduces."""
        v, blk, nxt, aa = self._v, self.plan.blocks[bi], self.plan.blocks[bi + 1], self._aa_transition(bi + 1)
        buf, nbuf, T = ws.buf[bi], ws.buf[bi + 1], ws.aa[bi]
        B, h, w, ct = buf.shape
        train = not ws.frozen
        none = (None, None, 1e-5, 0.0, None, None)              # no gain, shift or running statistics: moments only
        if train:
            ops.bn_coef_moments(v(ws, blk.mean), v(ws, blk.rstd), B * h * w, *none, None, None, ct, fresh)
        cc = aa.conv.out_channels                               # convolution branch, then the attention channels
        cout = cc + aa.dv                                       # (= ct // 2 in the reference's networks)
        ops.stats_bc(buf, T.stat[0], T.stat[1])                 # one owner per (image, channel): plain stores
        ops.bn_coef(T.stat[0], T.stat[1], h * w, *none, T.coef[0], T.coef[1], None, None, B * ct)
        ops.affine_relu_bc(buf, T.coef[0], T.coef[1], T.A)
        # the block's first channels come from two kernels: the conv branch's rows become moments at once (they share the scratch
        # pair with the out-projection's rows), the attention channels' rows stay pending for the next norm1
        rows = ops.conv_gemm(T.A, self.w_fwd(aa.conv), nbuf[..., :cc], N=cc, kh=3, kw=3, stride=2, pad=1,
                             **(self._sp(ws, cc) if train else dict(stat_sum=None, stat_sq=None)))
        if train:
            ops.bn_coef_moments(v(ws, nxt.mean, cc), v(ws, nxt.rstd, cc), B * (h // 2) * (w // 2), *none, None, None, cc,
                                self._fresh(ws, rows, 0, cc))
        ops.conv_gemm(T.A, self.w_fwd(aa.in_proj_qkv), T.QKV, N=2 * aa.dk + aa.dv, stride=2)
        ops.aa_attention_fwd(T.QKV, *aa.rel_tables(), T.O, T.LSE, aa.nh, aa.dk, aa.dv)
        object.__setattr__(aa, "_last", (T.QKV, T.LSE))
        rows = ops.aa_outproj_fwd(T.O, aa.out_proj.weight, nbuf[..., cc:cout], *self._ew(ws, aa.dv), stat_rstride=aa.dv if train else 0)
        return self._fresh(ws, rows, cc, aa.dv)

    # ---- backward
    def _backward(self, ws, dlogits, dx, done):
        """Head, then the blocks from last to first: a block's layers from last to first, its batched 3x3 weight gradients, its
        entry (transition or stem).  Everything is issued on the current stream.  The weight-gradient kernels only feed the flat
        gradient buffer, but beside the input-gradient chain on a second stream they were no faster (30.37 vs 30.31 ms per step,
        interleaved A/B on one box), and on one stream each 3x3 weight gradient reads the DENSE corrected slice its own layer's
        input-gradient kernel leaves behind (CxConv.pro_out: 30.0 ms)."""
        self._w2_items = []
        ws.alloc_backward(self, self.device)
        z0, zn = self.bwd_zero
        ws.vec[z0:z0 + zn].zero_()
        self._head_backward(ws, dlogits, done)
        # input gradient + weight gradient of conv1 in one pass over dz2 / y1 / the buffer slice (conv1x1_bwd.hip: 6-37 % less kernel
        # time than the two separate kernels, whole step 37.6 vs 39.0 ms): a bf16 kernel for 128 bottleneck channels -- the fp32
        # parity mode and the channel-padded CIFAR twin run the two kernels one after the other
        fused = self.dtype == torch.bfloat16 and self.mid == 128
        k = 0                                # the dz2 buffers alternate (the two-layer pass holds both)
        for bi in range(len(self.blocks) - 1, -1, -1):
            c0, n_layers = self.blocks[bi]
            h, w = ws.hw[bi]
            cnt = ws.B * h * w
            dz2s = [d.view(-1)[:cnt * self.mid].view(ws.B, h, w, self.mid) for d in ws.dz2]
            if self._aa_transition(bi + 1) is not None:
                self._last_slice_coef(ws, bi)
            # a block's 3x3 weight gradients leave the input-gradient chain and run as ONE launch after the block
            # (cx_conv3x3_wgrad_batch) on the maps the strip weight-gradient kernel serves: 40x40 and smaller at 320x320; the 80x80
            # maps keep the ring kernel, layer by layer
            batch_w2 = fused and self.growth == 32 and (w < 56 or h * w < 3136)
            # two layers per pass over the channels both read (cx_conv1x1_dgrad_wgrad_pair_ws), where the x / dX traffic it saves
            # outweighs the second read of the later layer's dZ by its 32-channel slice launch (measured crossover at B = 256:
            # >= 288 shared channels on the 40x40 maps, >= 736 on the 20x20 maps, never on 10x10; scratch/bench_pair.py)
            pair_min = 1 << 30
            if self.pair_bwd != "0" and fused and self.growth == 32 and not self.drop_rate:
                pair_min = 0 if self.pair_bwd == "all" else 288 if cnt >= 300000 else 736 if cnt >= 80000 else 1 << 30
            li = n_layers - 1
            while li >= 0:
                if li >= 1 and c0 + (li - 1) * self.growth >= pair_min:
                    self._pair_backward(ws, bi, li, dz2s[k & 1], dz2s[(k + 1) & 1], batch_w2, done)
                    k, li = k + 2, li - 2
                    continue
                dz2 = dz2s[k & 1]
                self._layer_front(ws, bi, li, dz2, batch_w2)
                self._layer_conv1(ws, bi, li, dz2, fused, done)
                k, li = k + 1, li - 1
            self._flush_w2()
            # the block's first c0 channels were produced by the previous transition (or the stem)
            if self._aa_transition(bi) is not None:
                self._aa_backward(ws, bi, done)
            elif bi > 0:
                self._transition_backward(ws, bi, done)
            elif self.cifar:
                self._cifar_stem_backward(ws, dx)
            else:
                self._stem_backward(ws, dx)

    def _slice_q(self, ws, bi, li):
        """(qa, qb, qc, first channel, channels) of the slice layer li of block bi produced (li = -1: the block's first c0
        channels): emitted by the coefficient kernel of the slice's LAST consumer, whose A / B update completes them."""
        c0, _ = self.blocks[bi]
        Q, n = (self.plan.q, c0) if li < 0 else (self.plan.blocks[bi].layers[li], None)
        return tuple(self._v(ws, t, n) for t in (Q.qa, Q.qb, Q.qc)) + ((0, c0) if li < 0 else (c0 + li * self.growth, self.growth))

    def _norm_bwd(self, ws, bn, S, r, count, acc=None, q=None, c_=None):
        """Backward coefficients of BatchNorm `bn` (record S) and its dgamma / dbeta from the backward sums r = (S1, S2, replicas,
        rstride) over `count` values per channel.  A norm2 / norm0 gets its own pa / pb / pc.  A norm over a block buffer (norm1,
        transition norm, norm5) names the block's record as `acc`: its terms go to the block's accumulators A / Bc, over the
        block's mean / rstd, and q (_slice_q) asks for the coefficients of the slice this norm is the last consumer of.  c_: the
        range of the norm's channels that r covers (_pair_backward)."""
        v, G, M = self._v, self.grad_of, acc or S
        lo, n = (0, S.C) if c_ is None else (c_.start, c_.stop - c_.start)
        ch = lambda t: self._ch(t, c_)
        out = (ch(v(ws, acc.A)), ch(v(ws, acc.Bc)), None, None, None) if acc is not None else \
            (None, None, v(ws, S.pa), v(ws, S.pb), v(ws, S.pc))
        if q is not None and c_ is not None:
            q = q[:3] + (q[3] - lo, q[4])
        self.bn_bwd_coef(ws, bn, r[0], r[1], count, ch(bn.weight), ch(v(ws, M.mean)), ch(v(ws, M.rstd)), ch(G(bn.weight)), ch(G(bn.bias)),
                         *out, n, replicas=r[2], rstride=r[3], q=q, lo=lo)

    def _head_backward(self, ws, dlogits, done):
        """The shared head's backward (FusedEngine._head_bwd) -> norm5, into the last block's gradient buffer."""
        m, v = self.model, self._v
        bi = len(self.blocks) - 1
        blk, ct = self.plan.blocks[bi], self.plan.blocks[bi].C
        if ws.B * ct > self.SLAB:
            raise RuntimeError("batch too large for the statistic-row scratch (B*C = %d > %d)" % (ws.B * ct, self.SLAB))
        rows = self._head_bwd(ws, dlogits, ws.buf[bi], v(ws, blk.sc), v(ws, blk.sh), v(ws, blk.mean), v(ws, blk.rstd), v(ws, blk.sc),
                              ws.gbuf[bi], *self._ew(ws, ct, bwd=True, rows=self.SLAB // ct), m.classifier, ops.POOL_ACT_RELU, None, done)
        self._norm_bwd(ws, m.features.norm5, blk, self._sc(ws, ct, rows), self._count(ws.buf[bi]), acc=blk,
                       q=self._slice_q(ws, bi, self.blocks[bi][1] - 1))

    def _last_slice_coef(self, ws, bi):
        """Block bi feeds an AA transition, which normalises per instance (its backward is complete in cx_in_relu_bwd): no BatchNorm
        consumer follows the block, so nobody has emitted the slice coefficients of its last layer -- A = B = 0 there."""
        blk, g_ = self.plan.blocks[bi], self.growth
        cl = blk.C - g_
        ops.bn_bwd_slice_coef(*(self._v(ws, (t[0] + cl, g_)) for t in (blk.A, blk.Bc, blk.mean, blk.rstd)),
                              *self._slice_q(ws, bi, self.blocks[bi][1] - 1)[:3], g_)

    def _layer_front(self, ws, bi, li, dz2, batch_w2):
        """Layer li of block bi from its gradient slice down to dz2, the gradient at norm2's output: (the dropout backward,) the 3x3
        input gradient with relu2's mask and norm2's sums in its epilogue, the 3x3 weight gradient -- queued for the block's batched
        launch when batch_w2 --, norm2's coefficients pa / pb / pc, which apply norm2's correction to dz2."""
        G, g_ = self.grad_of, self.growth
        layer, n2 = self._layer(bi, li), self.plan.blocks[bi].layers[li].n2
        y1 = ws.y1[bi][li]
        q = self._slice_q(ws, bi, li)                     # written by the previous coefficient launch
        cin = q[3]
        gs, xs = ws.gbuf[bi][..., cin:cin + g_], ws.buf[bi][..., cin:cin + g_]
        if self.drop_rate > 0 and not ws.frozen:         # (eval mode: no dropout in the forward)
            # the slice's deferred BatchNorm correction and the forward's keep decisions, in place on the gradient slice; the
            # kernels below then read it with identity coefficients
            ops.dropout_slice_bwd(gs, xs, *q[:3], self.drop_rate, self.drop_seed, bi * 256 + li)
            q = ws.ones[:g_], ws.zeros[:g_], ws.zeros[:g_]
        dyc = ws.dyc[bi][li] if ws.dyc is not None else None
        rows = ops.conv_gemm(gs, self.w_bwd(layer.conv2), dz2, N=self.mid, kh=3, kw=3, pad=1, pro_out=dyc, **self._pro_slice(xs, q),
                             **self._mask(ws, y1, n2))
        red2 = self._sc(ws, self.mid, rows)
        dw, x_n2 = G(layer.conv2.weight), self._x_bnrelu(ws, n2)
        if dyc is None or not ops.last_pro_out():
            # (fp32 mode, or a kernel without the side output) the slice as it lies in the block buffers, corrected on the fly
            ops.conv_wgrad(gs, y1, dw, kh=3, kw=3, pad=1, **self._g_slice(xs, q), **x_n2)
        elif batch_w2:
            self._w2_items.append(((dyc, y1, x_n2["pa"], x_n2["pb"], dw), x_n2))
        else:
            # the input-gradient kernel left the corrected slice as a dense (M, 32) tensor: the weight gradient reads 64 contiguous
            # bytes per pixel instead of two 64-byte pieces of the block buffers' rows (half of every line wasted)
            ops.conv_wgrad(dyc, y1, dw, kh=3, kw=3, pad=1, **x_n2)
        self._norm_bwd(ws, layer.norm2, n2, red2, self._count(y1))

    def _flush_w2(self):
        """Launch the collected 3x3 weight gradients of the current block (one batched launch per 24 layers; per layer when the
        library declines the shape or the slab workspace)."""
        items, self._w2_items = self._w2_items, []
        for i in range(0, len(items), ops.L.WGRAD_BATCH_MAX):
            part = items[i:i + ops.L.WGRAD_BATCH_MAX]
            if not ops.conv3x3_wgrad_batch([item for item, _ in part]):
                for (dyc, y1, _, _, dw), x_n2 in part:
                    ops.conv_wgrad(dyc, y1, dw, kh=3, kw=3, pad=1, **x_n2)

    def _layer_conv1(self, ws, bi, li, dz2, fused, done):
        """Layer li of block bi from dz2 into the gradient buffer's channels [0, cin): conv1's input gradient with relu1's mask and
        norm1's sums in its epilogue and conv1's weight gradient -- one kernel when `fused`, else two --, norm1's coefficients."""
        G, blk, layer = self.grad_of, self.plan.blocks[bi], self._layer(bi, li)
        L = blk.layers[li]
        y1, cin = ws.y1[bi][li], L.n1.C
        x = ws.buf[bi][..., :cin]
        rows = ops.conv_gemm(dz2, self.w_bwd(layer.conv1), ws.gbuf[bi][..., :cin], N=cin, accumulate=True,
                             fused_dw=G(layer.conv1.weight) if fused else None, **self._pro_bnbwd(ws, y1, L.n2),
                             **self._mask(ws, x, L.n1, by_sc=True))
        if not fused:
            ops.conv_wgrad(dz2, x, G(layer.conv1.weight), **self._g_bnbwd(ws, y1, L.n2), **self._x_bnrelu(ws, L.n1))
        self._norm_bwd(ws, layer.norm1, L.n1, self._sc(ws, cin, rows), self._count(x), acc=blk, q=self._slice_q(ws, bi, li - 1))
        done(layer.norm1.weight)      # every gradient from this layer to the end of the buffer is final

    def _transition_backward(self, ws, bi, done):
        """BatchNorm transition feeding block bi: conv (on the pooled map) -> 2x2 average un-pooling with the ReLU mask and the
        norm's sums -> the norm's coefficients, into the gradient buffer of block bi - 1."""
        v, G, prev = self._v, self.grad_of, self.plan.blocks[bi - 1]
        q = self._slice_q(ws, bi, -1)                         # written by layer 0's norm1 coefficient launch
        c0, cprev = q[4], prev.C
        gs, xs = ws.gbuf[bi][..., :c0], ws.buf[bi][..., :c0]
        B, (h, w) = ws.B, ws.hw[bi]
        tr = getattr(self.model.features, "transition%d" % bi)
        pbuf, pg = ws.buf[bi - 1], ws.gbuf[bi - 1]
        dpool = ws.dpool[:B * h * w * cprev].view(B, h, w, cprev)
        ops.conv_gemm(gs, self.w_bwd(tr.conv), dpool, N=cprev, **self._pro_slice(xs, q))
        rows = ops.unpool2_mask(dpool, pbuf, v(ws, prev.sc), v(ws, prev.sh), v(ws, prev.mean), v(ws, prev.rstd), v(ws, prev.sc), pg,
                                *self._ew(ws, cprev, bwd=True))
        sred = self._sc(ws, cprev, rows)
        ops.conv_wgrad(gs, pbuf, G(tr.conv.weight), mode=ops.MODE_POOL2, **self._g_slice(xs, q), **self._x_bnrelu(ws, prev))
        self._norm_bwd(ws, tr.norm, prev, sred, self._count(pbuf), acc=prev, q=self._slice_q(ws, bi - 1, self.blocks[bi - 1][1] - 1))
        done(tr.norm.weight)

    def _stem_backward(self, ws, dx):
        """ImageNet stem: max-pool / ReLU / norm0 backward in one kernel, norm0's coefficients, conv0's weight (and input) gradient."""
        f, v, G, S, ci = self.model.features, self._v, self.grad_of, self.plan.stem, self.c_init
        gs, xs = ws.gbuf[0][..., :ci], ws.buf[0][..., :ci]
        rows = ops.bnrelu_maxpool_bwd(ws.c0, v(ws, S.sc), v(ws, S.sh), v(ws, S.mean), v(ws, S.rstd), ws.amax, gs, xs,
                                      *self._slice_q(ws, 0, -1)[:3], ws.dz0, *self._ew(ws, ci, bwd=True))
        self._norm_bwd(ws, f.norm0, S, self._sc(ws, ci, rows), self._count(ws.c0))
        ops.conv_wgrad(ws.dz0, ws.x4, G(f.conv0.weight), mode=ops.MODE_STEM, **self._g_bnbwd(ws, ws.c0, S))
        if dx is not None:
            ops.stem_input_grad(ws.dz0, ws.c0, v(ws, S.pa), v(ws, S.pb), v(ws, S.pc), f.conv0.weight, dx, stride=2, pad=3)

    def _cifar_stem_backward(self, ws, dx):
        """Stem of the CIFAR form: relu0 mask + norm0 sums in the mask epilogue of the identity convolution (its two-tensor prologue
        applies the deferred BatchNorm correction to the gradient slice), then conv0's weight (and input) gradient."""
        f, v, G, S, ci = self.model.features, self._v, self.grad_of, self.plan.stem, self.c_init
        gs, xs = ws.gbuf[0][..., :ci], ws.buf[0][..., :ci]
        rows = ops.conv_gemm(gs, self.eye, ws.dz0, N=ci, **self._pro_slice(xs, self._slice_q(ws, 0, -1)), **self._mask(ws, ws.c0, S))
        self._norm_bwd(ws, f.norm0, S, self._sc(ws, ci, rows), self._count(ws.c0))
        ops.conv_wgrad(ws.dz0, ws.x8, G(f.conv0.weight), kh=5, kw=5, pad=2, **self._g_bnbwd(ws, ws.c0, S))
        if dx is not None:
            ops.stem_input_grad(ws.dz0, ws.c0, v(ws, S.pa), v(ws, S.pb), v(ws, S.pc), f.conv0.weight, dx, stride=1, pad=2)

    def _aa_backward(self, ws, bi, done):
        """Backward of the AA transition feeding block bi (from block bi-1); qa/qb/qc apply the deferred BN correction
        to the gradient slice [0, c0) of block bi."""
        G, aa = self.grad_of, self._aa_transition(bi)
        q = self._slice_q(ws, bi, -1)[:3]                     # written by layer 0's norm1 coefficient launch
        buf, gbuf, pbuf, pg, T = ws.buf[bi], ws.gbuf[bi], ws.buf[bi - 1], ws.gbuf[bi - 1], ws.aa[bi - 1]
        cc = aa.conv.out_channels
        c0 = cc + aa.dv                          # (the block's entry width in the reference's networks; the padded twin's is wider)
        Cp = pbuf.shape[3]
        gs_c, xs_c, gs_a, xs_a = gbuf[..., :cc], buf[..., :cc], gbuf[..., cc:c0], buf[..., cc:c0]
        q_c = [t[:cc] for t in q]
        ops.aa_outproj_bwd(gs_a, xs_a, *(t[cc:c0] for t in q), T.O, aa.out_proj.weight, T.dO, G(aa.out_proj.weight))
        ops.aa_attention_bwd(T.QKV, *aa.rel_tables(), T.O, T.dO, T.LSE, T.dQKV32, *aa.rel_grads(G), aa.nh, aa.dk, aa.dv)
        if self.dtype == torch.float32:         # fp32 storage mode: the fp32 gradient is the convolution operand as it is
            T.dQKV = T.dQKV32
        else:
            ops.f32_to_bf16(T.dQKV32, T.dQKV)
        # (the 3x3 branch reaches every pixel and stores; the 1x1 branch only reaches the even-even ones: accumulating, its
        # other parity classes are nothing to do)
        ops.conv_gemm(gs_c, self.w_bwd(aa.conv), T.dA, N=Cp, kh=3, kw=3, pad=1, tstride=2, **self._pro_slice(xs_c, q_c))
        ops.conv_gemm(T.dQKV, self.w_bwd(aa.in_proj_qkv), T.dA, N=Cp, tstride=2, accumulate=True)
        ops.conv_wgrad(T.dQKV, T.A, G(aa.in_proj_qkv.weight), stride=2)
        ops.conv_wgrad(gs_c, T.A, G(aa.conv.weight), kh=3, kw=3, stride=2, pad=1, **self._g_slice(xs_c, q_c))
        ops.in_relu_bwd(T.dA, pbuf, T.coef[0], T.coef[1], T.S[0], T.S[1], pg)       # S: one owner per (image, channel), plain stores
        done(aa.first_param())

    def _pair_backward(self, ws, bi, li, dz2_a, dz2_b, batch_w2, done):
        """Backward of dense layers li (a) and li - 1 (b) of block bi with ONE pass of the fused 1x1 backward over the channels
        [0, cin_b) both read.  Order: a's 3x3 input gradient -> a's 1x1 backward on its 32 newest channels alone (they are layer
        b's output slice: b's gradient depends on them) -> the slice's coefficients -> b's 3x3 input gradient -> the pair pass ->
        both norm1 coefficient launches (a's first: the A / B accumulators then see the same additions in the same order as in
        the layer-by-layer schedule).  Per channel every sum has the same terms as layer by layer, in another fp32 order."""
        v, G, blk = self._v, self.grad_of, self.plan.blocks[bi]
        buf, gbuf, cnt = ws.buf[bi], ws.gbuf[bi], self._count(ws.buf[bi])
        la, lb, La, Lb = self._layer(bi, li), self._layer(bi, li - 1), blk.layers[li], blk.layers[li - 1]
        cin_a, cin_b = La.n1.C, Lb.n1.C

        def conv1_args(l_i, layer, dz2, lo, hi, stat):
            """conv_gemm arguments of the layer's fused 1x1 backward restricted to its input channels [lo, hi)"""
            L = blk.layers[l_i]
            kw = dict(N=hi - lo, accumulate=True, **self._pro_bnbwd(ws, ws.y1[bi][l_i], L.n2),
                      **self._mask(ws, buf, L.n1, by_sc=True, c_=slice(lo, hi), stat=stat))
            return dz2, self.w_bwd(layer.conv1)[lo * self.mid:hi * self.mid], gbuf[..., lo:hi], kw

        def stat_region(n, part, parts):
            """(producer keywords, consumer tuple-maker) for the backward sums of n channels in one of `parts` regions of the rows"""
            per = self.SLAB // parts
            a, b_ = ws.slab[0][part * per:(part + 1) * per], ws.slab[1][part * per:(part + 1) * per]
            return dict(stat_sum=a, stat_sq=b_, stat_det=True, stat_replicas=per // n, stat_rstride=n), lambda rows: (a, b_, rows, n)

        self._layer_front(ws, bi, li, dz2_a, batch_w2)
        # layer a on slice li - 1 alone
        st_kw, st_red = stat_region(self.growth, 0, 1)
        x_, w_, y_, kw_ = conv1_args(li, la, dz2_a, cin_b, cin_a, st_kw)
        rows = ops.conv_gemm(x_, w_, y_, fused_dw=G(la.conv1.weight).view(self.mid, cin_a)[:, cin_b:], **kw_)
        self._norm_bwd(ws, la.norm1, La.n1, st_red(rows), cnt, acc=blk, q=self._slice_q(ws, bi, li - 1), c_=slice(cin_b, cin_a))
        self._layer_front(ws, bi, li - 1, dz2_b, batch_w2)
        # both layers on [0, cin_b)
        sa_kw, sa_red = stat_region(cin_b, 0, 2)
        sb_kw, sb_red = stat_region(cin_b, 1, 2)
        rows = ops.conv1x1_bwd_pair(conv1_args(li, la, dz2_a, 0, cin_b, sa_kw), conv1_args(li - 1, lb, dz2_b, 0, cin_b, sb_kw),
                                    G(la.conv1.weight).view(self.mid, cin_a)[:, :cin_b], G(lb.conv1.weight).view(self.mid, cin_b))
        self._norm_bwd(ws, la.norm1, La.n1, sa_red(rows), cnt, acc=blk, c_=slice(0, cin_b))
        self._norm_bwd(ws, lb.norm1, Lb.n1, sb_red(rows), cnt, acc=blk, q=self._slice_q(ws, bi, li - 2), c_=slice(0, cin_b))
        done(lb.norm1.weight)

    def _pre_bucket(self):
        self._flush_w2()
        super()._pre_bucket()


# --------------------------------------------------------------------------------------------- channel-padded twin
def _up8(n):
    return (n + 7) // 8 * 8


class _TwinNet(nn.Module):
    """The network the kernels run when the real one has widths that are not multiples of 8 (CIFAR DenseNet-BC, growth 12:
    models/test_model.py:306): same topology, every dense layer writes kp = up8(k) channels and every transition up8 of its width;
    the extra channels carry zero weights / BatchNorm gains / shifts, so they stay exactly zero forward and backward.  Only a
    parameter holder for _Engine -- its tensors are filled from the real model's by cx_chan_map_table before every forward."""

    def __init__(self, real):
        super().__init__()
        rf = real.features
        k, kp = real.growth_rate, _up8(real.growth_rate)
        mid, midp = real.bn_size * k, _up8(real.bn_size * k)
        self.growth_rate, self.block_config, self.bn_size, self._mid = kp, real.block_config, real.bn_size, midp
        self.drop_rate = getattr(real, "drop_rate", 0.0)      # (zeros stay zero under dropout: the padding channels are unaffected)
        ci = rf.conv0.out_channels
        nb = len(real.block_config)

        def padc(c, n):
            """padded width of a block's first channels: a multiple of 8 such that the block's full width c + n * kp is a multiple of
            32 (the pooled transition convolution walks its input in 32-channel steps)"""
            c = _up8(c)
            while (c + n * kp) % 32:
                c += 8
            return c
        cip = padc(ci, real.block_config[0])
        f = nn.Sequential()
        kh = rf.conv0.kernel_size[0]
        f.add_module("conv0", Conv2dParams(8, cip, kh, rf.conv0.stride[0], rf.conv0.padding[0], bias=False))
        f.add_module("norm0", BatchNorm2dParams(cip))
        # channel maps (c0r, c0p, k, kp) of every block buffer, and the (real tensor, twin tensor, rows, map) list of the sync tables
        self.maps, self.pairs, self.aa_pairs = [], [], []
        ident = lambda n, npad: (n, npad, 1, 1, n, 0)
        self.pairs += [(rf.conv0.weight, f.conv0.weight, ci, ident(3, 8)), (rf.norm0, f.norm0, None, ident(ci, cip))]
        cr, cp = ci, cip
        split, shift = ci, 0                  # inside a block's first channels: real j >= split sits at j + shift (after an AA transition)
        for bi, n in enumerate(real.block_config):
            m_ = (cr, cp, k, kp, split, shift)
            self.maps.append(m_)
            rblock = getattr(rf, "denseblock%d" % (bi + 1))
            block = nn.Sequential()
            for li in range(n):
                rl = getattr(rblock, "denselayer%d" % (li + 1))
                cinr, cinp = cr + li * k, cp + li * kp
                L = nn.Sequential()
                L.add_module("norm1", BatchNorm2dParams(cinp))
                L.add_module("conv1", Conv2dParams(cinp, midp, 1, 1, bias=False))
                L.add_module("norm2", BatchNorm2dParams(midp))
                L.add_module("conv2", Conv2dParams(midp, kp, 3, 1, 1, bias=False))
                block.add_module("denselayer%d" % (li + 1), L)
                self.pairs += [(rl.norm1, L.norm1, None, m_), (rl.conv1.weight, L.conv1.weight, mid, m_),
                               (rl.norm2, L.norm2, None, ident(mid, midp)), (rl.conv2.weight, L.conv2.weight, k, ident(mid, midp))]
            f.add_module("denseblock%d" % (bi + 1), block)
            ctr, ctp = cr + n * k, cp + n * kp
            if bi != nb - 1 and isinstance(getattr(rf, "transition%d" % (bi + 1)).conv, AAConv2d):
                # attention-augmented transition (attn_aug_conv.py:436-440): InstanceNorm -> ReLU -> AAConv2d(3x3, stride 2).  Its
                # output is [convolution branch | attention channels]: the branch is padded to a multiple of 8, the attention
                # channels follow, the rest up to the next block's entry width reads as zero
                raa = getattr(rf, "transition%d" % (bi + 1)).conv
                ccr, dv = raa.conv.out_channels, raa.dv
                ccp = _up8(ccr)
                cor, cop = ccr + dv, padc(ccp + dv, real.block_config[bi + 1])
                T = nn.Sequential()
                T.add_module("norm", InstanceNormMarker(ctp))
                taa = AAConv2d(ctp, ccp + dv, 3, 2, raa.dk, dv, raa.nh, raa.relative, raa.input_dims)
                T.add_module("conv", taa)
                f.add_module("transition%d" % (bi + 1), T)
                self.pairs += [(raa.conv.weight, taa.conv.weight, ccr, m_), (raa.in_proj_qkv.weight, taa.in_proj_qkv.weight, 2 * raa.dk + dv, m_),
                               (raa.out_proj.weight, taa.out_proj.weight, dv, ident(dv, dv))]
                if raa.relative:
                    for nm in ("key_rel_h", "key_rel_w"):
                        rp, tp = getattr(raa, nm), getattr(taa, nm)
                        self.pairs.append((rp, tp, rp.shape[0], ident(rp.shape[1], tp.shape[1])))
                self.aa_pairs.append((raa, taa))
                cr, cp, split, shift = cor, cop, ccr, ccp - ccr
            elif bi != nb - 1:
                rt = getattr(rf, "transition%d" % (bi + 1))
                cor = rt.conv.out_channels
                cop = padc(cor, real.block_config[bi + 1])
                T = nn.Sequential()
                T.add_module("norm", BatchNorm2dParams(ctp))
                T.add_module("conv", Conv2dParams(ctp, cop, 1, 1, bias=False))
                f.add_module("transition%d" % (bi + 1), T)
                self.pairs += [(rt.norm, T.norm, None, m_), (rt.conv.weight, T.conv.weight, cor, m_)]
                cr, cp, split, shift = cor, cop, cor, 0
            else:
                f.add_module("norm5", BatchNorm2dParams(ctp))
                self.classifier = nn.Linear(ctp, real.classifier.out_features, bias=real.classifier.bias is not None)
                self.pairs += [(rf.norm5, f.norm5, None, m_), (real.classifier.weight, self.classifier.weight, real.classifier.out_features, m_)]
                if real.classifier.bias is not None:
                    nc = real.classifier.out_features
                    self.pairs += [(real.classifier.bias, self.classifier.bias, None, ident(nc, nc))]
        self.features = f
        for t in list(self.parameters()) + [b for b in self.buffers() if b.dtype == torch.float32]:
            t.data.zero_()                        # the padded positions keep these zeros (running_var of a padded channel: 0 + eps)
        self._nbt_pending = 0

    def forward(self, *a, **k):  # pragma: no cover - guard
        raise RuntimeError("parameter holder of the channel-padded schedule")


class _PaddedEngine(FusedEngine):
    """Engine of a network with unaligned widths: binds the REAL parameters to a flat buffer (what optimisers and state_dict see),
    runs the channel-padded twin on an inner _Engine and moves parameters / running statistics / gradients between the two flat
    layouts with one table-driven launch each (cx_chan_map_table)."""

    def __init__(self, model):
        super().__init__(model)
        self.twin = _TwinNet(model)
        object.__setattr__(self.twin, "_storage_dtype", self.dtype)
        self.inner = _Engine(self.twin)
        self.c_final = model.classifier.in_features

    def bind(self, dev):
        if self.bound(dev) and all(b.data_ptr() == self.stat.data_ptr() + 4 * off for b, off in zip(self.rbufs, self.boffs)):
            return
        if self.twin.classifier.weight.device != dev:
            self.twin.to(dev)
        self.inner.bind(dev)
        self.bind_params(dev)
        # running statistics of both networks in flat buffers of their own
        bn_pairs = [(r, t) for r, t, _, _ in self.twin.pairs if isinstance(r, nn.BatchNorm2d)]
        self.rbufs = [b for r, _ in bn_pairs for b in (r.running_mean, r.running_var)]
        tbufs = [b for _, t in bn_pairs for b in (t.running_mean, t.running_var)]
        self.stat, self.boffs = flatten(self.rbufs, dev)
        self.tstat, tboffs = flatten(tbufs, dev)
        in_ = self.inner
        from .._lib import CxChanMapDesc
        pd, sd = [], []
        bi = 0
        for r, t, rows, (c0r, c0p, k, kp, split, shift) in self.twin.pairs:
            if isinstance(r, nn.BatchNorm2d):
                C_r, C_p = r.num_features, t.num_features
                for rp, tp in ((r.weight, t.weight), (r.bias, t.bias)):
                    pd.append(CxChanMapDesc(self.off_of[id(rp)], in_.off_of[id(tp)], 1, 1, C_r, C_p, c0r, c0p, k, kp, split, shift))
                for j in range(2):
                    sd.append(CxChanMapDesc(self.boffs[bi + j], tboffs[bi + j], 1, 1, C_r, C_p, c0r, c0p, k, kp, split, shift))
                bi += 2
            else:
                O_r = r.shape[0]
                I_r = r.shape[1] if r.dim() > 1 else 1
                I_p = t.shape[1] if t.dim() > 1 else 1
                taps = r[0, 0].numel() if r.dim() == 4 else 1
                if r.dim() == 1:                 # classifier bias: one row of O_r channels
                    O_r, I_r, I_p = 1, r.shape[0], t.shape[0]
                if rows is not None and r.dim() > 1:
                    O_r = rows
                pd.append(CxChanMapDesc(self.off_of[id(r)], in_.off_of[id(t)], O_r, taps, I_r, I_p, c0r, c0p, k, kp, split, shift))

        def table(descs):
            arr = (CxChanMapDesc * len(descs))(*descs)
            return torch.frombuffer(bytearray(bytes(arr)), dtype=torch.uint8).to(dev), len(descs)
        self.ptab, self.stab = table(pd), table(sd)
        self.n_classes = self.model.classifier.out_features

    def _map(self, real, padded, tab, direction, accumulate=0):
        ops.chan_map_table(real, padded, tab[0], tab[1], direction, accumulate)

    def forward(self, x, train, record=False):
        self.bind(x.device)
        in_ = self.inner
        self._map(self.flat, in_.flat, self.ptab, 0)              # parameters: real -> padded
        self._map(self.stat, self.tstat, self.stab, 0)            # running statistics
        in_.packed_version = None
        in_.track_stats = self.track_stats
        ws = in_.forward(x, train, record)
        for raa, taa in self.twin.aa_pairs:                       # AAConv2d.weights of the real module (attn_aug_conv.py:87)
            object.__setattr__(raa, "_last", taa._last)
        if train and self.track_stats:
            self._map(self.stat, self.tstat, self.stab, 1)        # updated running statistics: padded -> real
            self.twin._nbt_pending = 0
            self.model._nbt_pending += 1
        return ws

    def backward(self, ws, dlogits, dx=None):
        in_ = self.inner
        in_.flat_grad.zero_()
        for p, gv in zip(in_.params, in_.grad_views):
            p.grad = gv
        fresh = any(p.grad is None for p in self.params)
        if fresh:
            self.flat_grad.zero_()
        in_.backward(ws, dlogits, dx)       # (the twin's conv0 reads the 3 real input channels first: dx is the real one's)
        self._map(self.flat_grad, in_.flat_grad, self.ptab, 1, 1)  # gradients: padded -> real, added
        if fresh:
            for p, gv in zip(self.params, self.grad_views):
                p.grad = gv

    def release(self, ws):
        self.inner.release(ws)

    def enable_data_parallel(self, *a, **k):
        raise NotImplementedError("the channel-padded CIFAR DenseNet-BC schedule is single-device (models/test_model.py has no "
                                  "data-parallel mode)")


# --------------------------------------------------------------------------------------------- module
class DenseNet(FusedNet):
    """Signature of /root/reference/models/attn_aug_conv.py:452-453 (torchvision DenseNet + attn_params)."""

    def __init__(self, growth_rate=32, block_config=(6, 12, 24, 16), num_init_features=64, bn_size=4, drop_rate=0,
                 num_classes=1000, attn_params=None):
        super().__init__()
        if not 0 <= drop_rate < 1:
            raise ValueError("drop_rate must be in [0, 1)")
        # torchvision _DenseLayer: F.dropout(new_features, p=drop_rate, training=self.training) on each layer's 32 new channels
        # (attn_aug_conv.py:479-481 hands drop_rate to _DenseBlock); chexpert.py trains with 0
        self.drop_rate = float(drop_rate)
        self.growth_rate, self.block_config, self.bn_size = growth_rate, tuple(block_config), bn_size
        if attn_params is not None:             # the reference mutates the caller's dict (:468, :493); a copy is used here
            attn_params = dict(attn_params)
        if len(block_config) == 4:              # ImageNet stem (attn_aug_conv.py:459-468): the configuration chexpert.py trains
            self.features = nn.Sequential(OrderedDict([
                ("conv0", Conv2dParams(3, num_init_features, 7, 2, 3, bias=False)),
                ("norm0", BatchNorm2dParams(num_init_features)),
                ("relu0", ReLUMarker(inplace=True)),
                ("pool0", PoolMarker()),
            ]))
            if attn_params is not None:
                attn_params["input_dims"] = (attn_params["input_dims"][0] // 4, attn_params["input_dims"][1] // 4)
        else:                                   # CIFAR stem (:469-474): constructible (models/test_model.py), not on the MI355X path
            self.features = nn.Sequential(OrderedDict([
                ("conv0", Conv2dParams(3, num_init_features, 5, 1, 2, bias=False)),
                ("norm0", BatchNorm2dParams(num_init_features)),
                ("relu0", ReLUMarker(inplace=True)),
            ]))
        c = num_init_features
        self.attn_params = attn_params
        for i, n in enumerate(block_config):
            self.features.add_module("denseblock%d" % (i + 1), _DenseBlock(n, c, bn_size, growth_rate))
            c += n * growth_rate
            if i != len(block_config) - 1:
                self.features.add_module("transition%d" % (i + 1), _Transition(c, c // 2, attn_params))
                c //= 2
            if attn_params is not None:
                attn_params["input_dims"] = (attn_params["input_dims"][0] // 2, attn_params["input_dims"][1] // 2)
        self.features.add_module("norm5", BatchNorm2dParams(c))
        self.classifier = nn.Linear(c, num_classes)
        # initialisers of the reference (attn_aug_conv.py:503-510)
        for mod in self.modules():
            if isinstance(mod, nn.Conv2d):
                nn.init.kaiming_normal_(mod.weight)
            elif isinstance(mod, nn.BatchNorm2d):
                nn.init.constant_(mod.weight, 1)
                nn.init.constant_(mod.bias, 0)
            elif isinstance(mod, nn.Linear):
                nn.init.constant_(mod.bias, 0)

    # the engine is rebuilt lazily (the classifier may be replaced after construction, chexpert.py:464)
    def _eng(self):
        padded = len(self.block_config) != 4 or self.growth_rate % 8 or self.features.conv0.out_channels % 8
        if padded and len(self.block_config) == 4:
            raise NotImplementedError("ImageNet-stem DenseNets need growth and stem widths that are multiples of 8")
        for mod in self.modules():
            if isinstance(mod, AAConv2d):
                mod.check_supported(branch_aligned=not padded)
        if padded:
            self.require_avg_pool("the channel-padded CIFAR DenseNet-BC schedule (_TwinNet)")
        if self._engine is None or self._engine.c_final != self.classifier.in_features or \
                self._engine.dtype != getattr(self, "_storage_dtype", torch.bfloat16):
            object.__setattr__(self, "_engine", _PaddedEngine(self) if padded else _Engine(self))
        return self._engine

    def _anchor(self):
        return self.classifier.weight


def densenet121(pretrained=False, **kwargs):
    """torchvision.models.densenet121 stand-in (chexpert.py:24, :462).  `pretrained` would download
    ImageNet weights in the reference; there is no network here, load a state_dict instead."""
    if pretrained:
        raise RuntimeError("pretrained ImageNet weights cannot be downloaded here; use load_state_dict()")
    return DenseNet(32, (6, 12, 24, 16), 64, **kwargs)
