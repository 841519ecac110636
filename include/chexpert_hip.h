/*
 * chexpert_hip.h -- C ABI of libchexpert_hip.so (gfx950 / MI355X).
 *
 * The reference (kamenbliznashki/chexpert) has no FFI layer: its hot path is the implicit ATen/cuDNN
 * work behind `model(x)`, `loss.backward()` and `optimizer.step()` (chexpert.py:159-164, :204).  This
 * library is what a maintainer binds INSTEAD of those ATen ops (see INTEGRATION.md for the ctypes
 * stub).  Each entry point cites the reference statement whose arithmetic it replaces.
 *
 * Conventions
 *   - plain pointers and sizes only; every pointer is a DEVICE pointer owned by the caller
 *     (no ownership transfer, no allocation inside the library);
 *   - asynchronous on `stream` (a hipStream_t passed as void*; NULL = default stream);
 *   - returns 0 on success, a positive hipError_t from the launch, or a negative CX_E* validation
 *     code; nothing is launched when validation fails;
 *   - activations are NHWC bf16 with an explicit channel pitch (`ld*`, in elements) so a kernel can
 *     read / write a channel slice of a wider dense-block buffer (the reference's torch.cat,
 *     torchvision _DenseLayer.forward, is never materialised);
 *   - statistics, coefficient vectors and gradients of parameters are fp32.
 */
#ifndef CHEXPERT_HIP_H
#define CHEXPERT_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define CX_ABI_VERSION 10

enum { CX_EINVAL = -1, CX_EALIGN = -2, CX_ESHAPE = -3, CX_EUNSUPPORTED = -4, CX_ESTATROWS = -5 };

/* storage type of the activation tensors of a CxConv / CxWgrad: bf16 (the fast path: fp32 accumulation, fp32 statistics) or
 * fp32 (the parity mode of north_star "1e-3 fp32": same schedule, exact f32 MFMA, fp32 packed weights [tap][N][K])        */
enum { CX_DT_BF16 = 0, CX_DT_F32 = 1 };

/* A-operand prologues of the implicit GEMM (fused normalisation, never stored) */
enum {
  CX_PRO_NONE = 0,         /* a = x                                                              */
  CX_PRO_AFFINE_RELU = 1,  /* a = relu(x*pa[c] + pb[c])          BN/IN (scale,shift) + ReLU       */
  CX_PRO_AFFINE2 = 2,      /* a = x*pa[c] + x2*pb[c] + pc[c]     BN backward / deferred correction */
  CX_PRO_JOIN = 3          /* ABI 9, the residual join of the block BELOW as the prologue of a Bottleneck's conv1
                              (attn_aug_conv.py:188-211: `out = relu(bn3(conv3(.)) + identity)` followed by the next block's
                              `conv1(out)`): t = relu(x*pa[c] + (x2 [+ x3]) + pc[c]) with x = conv3's raw output, x2 / x3 = the
                              hi / lo planes of the identity operand (the residual stream, cx_join_fwd), a = bf16(t).  Side
                              outputs, written once (by the first N tile): pro_out = hi plane of t (bf16, pitch ldpo), po_lo =
                              its lo plane (one byte per element; NULL: single-plane output, the sign bits are then those of the
                              rounded tensor as cx_affine2_relu_mask writes them), po_mask = sign bits [t > 0] (one byte per 8
                              channels, bit c%8; NULL in eval mode), both in the side-plane layout of cx_join_fwd.  Bit for bit what cx_join_fwd leaves.  1x1, stride 1, bf16, K % 64 == 0. */
};
/* addressing modes */
enum {
  CX_MODE_CONV = 0,   /* kh x kw taps, stride, zero padding (applied after the prologue)          */
  CX_MODE_POOL2 = 1,  /* 1x1 on the 2x2 average of the prologue output (transition: conv o avgpool
                         commute, attn_aug_conv.py:433-434)                                      */
  CX_MODE_STEM = 2    /* 7x7 stride 2 pad 3 on a (B,H,W,4) bf16 image; 7 row-taps of 8px*4ch      */
};
/* epilogues */
enum {
  CX_EPI_STORE = 0,   /* y = bf16(acc); optional per-channel sum / sum of squares (fp32 atomics)   */
  CX_EPI_MASK = 1,    /* dz = acc * [ex*e_sc + e_sh > 0]; S1 += sum dz; S2 += sum dz*(ex-e_mu)*e_r;
                         y = (accumulate ? y : 0) + e_scale*dz            (ReLU+BN backward)      */
  CX_EPI_JOIN = 2     /* ABI 8, residual join backward folded into the input gradient that completes the join's output
                         gradient (attn_aug_conv.py:202-209: out = relu(bn3(z3) + identity)): t = bf16(y + acc) is the gradient of
                         `out` (y holds the part that arrived through the identity path: accumulate must be set),
                         dz = t * [bit of emask], S1 += sum dz, S2 += sum dz*(ex-e_mu)*e_r with ex = z3 (the join BatchNorm's
                         input), y = dz.  Bit for bit what CX_EPI_STORE + cx_relu_bwd_stats_mask leave in y.  bf16, stride 1. */
};

typedef struct CxConv {
  const void* x;        /* bf16 input (B,H,W,ldx)                                                 */
  const void* x2;       /* second input for CX_PRO_AFFINE2 (same geometry, pitch ldx2) or NULL     */
  const void* w;        /* packed bf16 weights [taps][N][K] (K contiguous), see cx_pack_weights    */
  void* y;              /* bf16 output (B,Ho,Wo,ldy), written at channel 0 of the pointer          */
  const float* pa; const float* pb; const float* pc;          /* prologue vectors [K]             */
  float* stat_sum; float* stat_sq;                             /* [N] or NULL                      */
  const void* ex;       /* CX_EPI_MASK: bf16 tensor (B,Ho,Wo,ldex) the ReLU mask / xhat come from  */
  const float* e_sc; const float* e_sh; const float* e_mu; const float* e_r; const float* e_scale; /* [N] */
  int32_t B, H, W, Ho, Wo;
  int32_t K, N;         /* channels per tap in / out; both multiples of 8                          */
  int32_t ldx, ldx2, ldy, ldex;
  int32_t kh, kw, stride, pad;
  int32_t prologue, mode, epilogue, accumulate;   /* accumulate: y += result (both epilogues)             */
  int32_t tstride;      /* 2: input gradient of a stride-2 conv (x is its output gradient,              */
                        /* stride must be 1, pad = kh-1-forward_pad, weights packed with transpose=1)    */
  int32_t stat_replicas; /* R > 1: workgroup b adds its statistics to replica b % R, replica r of channel */
  int32_t stat_rstride;  /* n lives at stat_sum[r*stat_rstride + n].  Thousands of workgroups adding to   */
                         /* the same N floats serialise at the memory side; the consumer (cx_bn_coef /   */
                         /* cx_bn_bwd_coef) sums the replicas.  0 or 1: a single copy                     */
  int32_t stat_det;      /* != 0: DETERMINISTIC statistics.  No atomics: the launch writes `rows` complete rows   */
                         /* stat_sum[r*stat_rstride + n] (r < rows, every n < N; one writer per element, partial */
                         /* sums combined in a fixed order inside the workgroup), rows <= stat_replicas (the     */
                         /* caller's capacity) or CX_ESTATROWS; cx_last_stat_rows() then returns `rows` and the   */
                         /* consumer sums exactly those rows in row order (cx_bn_coef / cx_bn_bwd_coef with      */
                         /* replicas = rows): bit-identical results from run to run.  No zero-fill is needed      */
  int32_t dtype;         /* CX_DT_BF16 (0) or CX_DT_F32: x, x2, y, ex are fp32, w is fp32 [tap][N][K]; K, N, ld* % 4 */
  /* ABI 7.  Optional side output of the prologue: the transformed input (what the convolution actually consumes, e.g. the     */
  /* dense-layer output gradient after the deferred BatchNorm correction) stored as a dense bf16 (B,H,W,ldpo) tensor, K        */
  /* channels per pixel.  The 3x3 weight gradient of the same layer then reads ONE dense 64-byte row per pixel               */
  /* (g_prologue NONE) instead of two 64-byte pieces of 512..2048-byte rows of the block buffers.  Kernels that cannot        */
  /* write it ignore the field: cx_last_pro_out() says whether the last cx_conv_gemm of this thread did.                     */
  void* pro_out;
  int32_t ldpo;
  int32_t dil;           /* ABI 9 (was a zero pad field).  0 / 1: adjacent taps.  d > 1: taps d pixels apart -- torchvision conv3x3(..., dilation) of a */
                         /* Bottleneck under replace_stride_with_dilation (attn_aug_conv.py:183, :266-271): CX_MODE_CONV, kernel extent           */
                         /* d (kh - 1) + 1 in every shape rule; runs on the generic implicit GEMM (the tiled kernels assume adjacent taps)          */
  /* ABI 8.  CX_EPI_JOIN: the forward join's sign bits as cx_affine2_relu_mask / cx_join_fwd wrote them (side-plane layout, ABI 9): bit n%8 of chunk n/8 = [out[m][n] > 0] */
  const uint8_t* emask;
  /* ABI 9.  CX_PRO_JOIN: lo plane of the identity operand (B,H,W,K) int8 (NULL: x2 is a single-plane bf16 tensor), and the lo /   */
  /* sign-bit side outputs (dense: K bytes resp. K/8 bytes per pixel)                                                            */
  const int8_t* x3;
  int8_t* po_lo;
  uint8_t* po_mask;
  /* ABI 10.  Per-call kernel selection for tests and micro-benchmarks (stateless: replaces the process-wide dbg_* selectors of      */
  /* earlier ABIs).  0: the library picks.  Low byte 1: the generic implicit-GEMM kernels (conv_gemm.hip / conv_wgrad.hip),        */
  /* 2: the tiled kernels (conv_mm.hip / wgrad_mm.hip) where the shape allows.  Second byte f + 1: tile form f (1 = 128 x 128,     */
  /* 2 = 256 x 128 (weight gradient only), 3 = 128 x 256; weight gradient f = 0: the strip kernel for 3x3; f = 5: the activation-   */
  /* stationary 1x1 kernel, conv1x1_xs.hip, or an error; f = 7 / 8: ring / producer-consumer 3x3 forms).  CX_KERNEL_HINT(on, f).     */
  int32_t kernel_hint;
  int32_t pad2_;
} CxConv;
#define CX_KERNEL_HINT(on, form) ((((on) < 0) ? 0 : (on) + 1) | ((((form) < 0) ? 0 : (form) + 1) << 8))

/* Weight gradient of the same convolution:  dW[n][c][ky][kx] += sum_m G[m][n] * A[m@tap][c]
 *   G = dY (prologue NONE or AFFINE2 with vectors ga/gb/gc over N, second tensor g2)
 *   A = the forward A operand (prologue NONE / AFFINE_RELU with pa/pb over K, any mode)          */
typedef struct CxWgrad {
  const void* g; const void* g2;          /* bf16 (B,Ho,Wo,ldg)                                    */
  const void* x;                           /* bf16 forward input (B,H,W,ldx)                        */
  float* dw;                               /* fp32 OIHW gradient, accumulated with atomics          */
  const float* ga; const float* gb; const float* gc;   /* [N]                                       */
  const float* pa; const float* pb;                      /* [K]                                       */
  int32_t B, H, W, Ho, Wo, K, N;
  int32_t ldg, ldg2, ldx;
  int32_t kh, kw, stride, pad;
  int32_t g_prologue, x_prologue, mode;
  int32_t splits;                          /* pixel-range splits (0 = library picks)                */
  int32_t dtype;                           /* CX_DT_BF16 (0) or CX_DT_F32 (g, g2, x fp32)          */
  int32_t dil;                             /* ABI 9 (fills what was alignment padding): as CxConv.dil           */
  /* Optional workspace for a reproducible sum (ABI 4).  The pixel range of a weight gradient is split over workgroups; */
  /* with scratch == NULL (or too small for this launch) the partial tiles are added to dw with fp32 atomics, whose order */
  /* changes from run to run.  With scratch_floats >= splits * |dW| every workgroup plain-stores its partial tile into   */
  /* slab `split` and a second launch on the same stream adds the slabs to dw in split order: bit-identical results.      */
  /* The library picks `splits`; 16 M floats cover every layer of the reference's networks at their benchmark batches.    */
  float* scratch;
  int64_t scratch_floats;
  int32_t kernel_hint;                     /* ABI 10: as CxConv.kernel_hint                                      */
  int32_t pad_;
} CxWgrad;

/* ABI 8.  The 3x3 weight gradients (K = 128 -> N = 32, stride 1, pad 1) of up to CX_WGRAD_BATCH_MAX dense layers of ONE dense block
 * (same B, H, W, pitches) in one launch: torchvision `_DenseLayer.conv2` as restated at attn_aug_conv.py:13, weight gradient of
 * every layer of a `_DenseBlock` (:476-483).  A dense layer's 3x3 weight gradient feeds only the flat gradient buffer, so the
 * launches of a block do not depend on each other once every layer's output-gradient slice exists as a dense tensor
 * (CxConv.pro_out) -- batched they leave the input-gradient chain and share one grid (workgroup = layer x pixel range x 32-channel
 * tile).  `geo` gives the common geometry and prologue (g_prologue NONE, x_prologue AFFINE_RELU), the slab workspace (scratch:
 * n * splits * 36864 floats are used, cx_last_slab_floats() reports them) and dtype; its g / x / dw / pa / pb are ignored.
 * items[i]: g = dense (B,H,W,ldg) gradient slice, x = saved bottleneck tensor (B,H,W,ldx), pa / pb = its norm2 scale / shift [128],
 * dw = fp32 OIHW gradient (32,128,3,3), added in split order (immediately or through cx_wgrad_defer like cx_conv_wgrad).
 * CX_EUNSUPPORTED: shape / workspace outside the kernel's range -- call cx_conv_wgrad per layer instead.                          */
#define CX_WGRAD_BATCH_MAX 24
typedef struct CxWgradBatch {
  const void* g[CX_WGRAD_BATCH_MAX];
  const void* x[CX_WGRAD_BATCH_MAX];
  const float* pa[CX_WGRAD_BATCH_MAX];
  const float* pb[CX_WGRAD_BATCH_MAX];
  float* dw[CX_WGRAD_BATCH_MAX];
  int32_t n, pad_;
} CxWgradBatch;
int cx_conv3x3_wgrad_batch(const CxWgrad* geo, const CxWgradBatch* items, void* stream);

/* ABI 8.  Channel-padded twin (the CIFAR DenseNet-BC of models/test_model.py:306: growth 12, widths 24 + 12 i are not multiples of
 * the kernels' 8-channel vectors).  The network runs on a twin whose dense layers write kp = 16 channels (12 real + 4 that stay
 * zero: zero weights, zero BatchNorm gain and shift) and whose transitions are padded likewise; this entry point moves parameters
 * / running statistics real -> padded (dir 0, store) and gradients / running statistics padded -> real (dir 1; accumulate: add)
 * between two flat fp32 buffers, one descriptor per tensor, ONE launch.  Element (o, j, t) of the real [O][Ireal][taps] tensor is
 * element (o, pos(j), t) of the padded [.][Ipad][taps] one, pos(j) = j (+ shift from `split` on) for j < c0r, else
 * c0p + ((j-c0r)/k)*kp + (j-c0r)%k.                                                                                             */
typedef struct CxChanMapDesc {
  int64_t real_off, pad_off;         /* element offsets into the two flat buffers                                             */
  int32_t O, taps, Ireal, Ipad;      /* rows copied (the padded tensor may have more), kh*kw, channels per row                   */
  int32_t c0r, c0p, k, kp;           /* channel map (k = kp = 1, c0r = Ireal: identity with a wider row)                          */
  int32_t split, shift;              /* inside the first c0r channels: j >= split sits at j + shift (split = c0r, shift = 0: none) --
                                        the output of an attention-augmented transition is [conv branch | pad | attention channels] */
} CxChanMapDesc;
int cx_chan_map_table(float* real_flat, float* padded_flat, const CxChanMapDesc* table_dev, int n_desc, int dir, int accumulate,
                      void* stream);

/* Deferred slab sums (ABI 6).  A training step issues ~120 weight-gradient launches whose partial tiles (CxWgrad.scratch) each
 * need a small ordered sum into dw; one launch per sum puts ~60 of them on the critical stream (6-7 us each on DenseNet121).
 * cx_wgrad_defer(1) switches the calling thread to deferral: every weight-gradient entry point (cx_conv_wgrad,
 * cx_conv1x1_dgrad_wgrad_ws) then only stores its partial tiles -- the caller must hand each launch a scratch region that
 * stays untouched until the sums have run (cx_last_slab_floats() tells how much of it the launch used; 0 = it fell back to atomics)
 * -- and records {dw, slab, total, splits}.  cx_wgrad_defer_take() returns the records (first_block filled in), which the caller
 * copies to the device once per distinct schedule, and cx_dw_reduce_table() adds them all in ONE launch on a stream that has
 * been joined with the producers: every dw element receives exactly the additions, in the order, of its own immediate sum,
 * so results are bit-identical to the immediate form.  cx_wgrad_defer(0) returns to immediate sums and keeps the pending records
 * (a single launch can be taken out of the deferral that way), cx_wgrad_defer(-1) also drops them.                              */
typedef struct CxReduceDesc {
  float* dw; const float* slab;      /* dw[i] += slab[0*total + i] + slab[1*total + i] + ... (fixed association)             */
  int64_t total;                     /* elements of dw                                                                        */
  int32_t splits, vec, first_block, pad_;
  int32_t cols, dw_ld;               /* ABI 9: cols != 0: the slab tile is [total / cols][cols] and goes to dw[r * dw_ld + c] (a column   */
  int64_t pad2_;                     /* range of a wider matrix: a layer's newest 32 input channels, or all but those); 0: contiguous    */
} CxReduceDesc;
int cx_wgrad_defer(int on);                                            /* returns the previous state                          */
int cx_wgrad_defer_take(CxReduceDesc* out_host, int capacity, int64_t* total_blocks);   /* n records, or -n if capacity < n   */
int cx_last_slab_floats(void);
int cx_dw_reduce_table(const CxReduceDesc* table_dev, int n, int64_t total_blocks, void* stream);

int cx_abi_version(void);
int cx_last_pro_out(void);      /* 1: the last cx_conv_gemm of the calling thread wrote CxConv.pro_out */
const char* cx_error_string(int code);
/* name of the kernel instantiation the most recent cx_conv_gemm / cx_conv1x1_dgrad_wgrad* / cx_conv_wgrad call of this thread
 * dispatched to, spelled as rocprofv3 lists it (e.g. "pw_bwd2_kernel<2, true, 0>"; a stride-2 input gradient that runs as up to
 * four parity-class launches carries the suffix " x parity classes").  For measurement tools: valid until the next call.       */
const char* cx_last_kernel(void);
/* rows written by the most recent successful stat_det launch issued from the calling thread */
int cx_last_stat_rows(void);

/* conv forward / input-gradient as one implicit GEMM family.
 * Replaces F.conv2d + F.batch_norm + F.relu (+ torch.cat, avg_pool2d) forward and their autograd
 * input-gradients: torchvision _DenseLayer (norm1-relu1-conv1-norm2-relu2-conv2), _Transition
 * (attn_aug_conv.py:431-434), features.conv0 (:461), Bottleneck convs (:194-203).               */
int cx_conv_gemm(const CxConv* p, void* stream);
/* weight gradient (autograd of the same convs)                                                   */
int cx_conv_wgrad(const CxWgrad* p, void* stream);
/* input gradient of the stem convolution down to the 3-channel image (x.grad through features.conv0 / conv1 / stem[0]):
 * dx[b][c][iy][ix] = sum_{o,ky,kx} w[o][c][ky][kx] * g[b][oy][ox][o], iy = stride*oy - pad + ky, c = 0..2, with
 * g = pa[o]*dz + pb[o]*y + pc[o] (the stem weight gradient's CX_PRO_AFFINE2 prologue).  dz / y: (B,Ho,Wo,>=C0) NHWC, row
 * pitches ldz / ldy, dtype 0 = bf16 (g and w rounded to bf16, fp32 sums), 1 = fp32; w: fp32 master (C0,wc,k,k), the first 3 input
 * channels used; dx: fp32 NCHW (B,3,H,W), overwritten, deterministic (no atomics).  Geometries: k7 s2 p3, k3 s2 p0|p1
 * (bf16: C0 % 8 == 0, C0 <= 64), k3 s1 p1, k5 s1 p2 (C0 <= 128); anything else CX_EUNSUPPORTED.                        */
int cx_stem_input_grad(const void* dz, const void* y, const float* pa, const float* pb, const float* pc, const float* w, float* dx,
                       int ldz, int ldy, int wc, int B, int H, int W, int Ho, int Wo, int C0, int k, int stride, int pad, int dtype,
                       void* stream);

/* Input gradient AND weight gradient of the dense-layer bottleneck 1x1 convolution in one pass over dZ and the activation
 * slice (K = 128 gradient channels, CX_EPI_MASK): p as for cx_conv_gemm (p->ex = the activation slice x, p->e_sc / p->e_sh its
 * BatchNorm scale / shift), and dW[n][c] += sum_m dZ[m][n] * relu(x[m][c]*e_sc[c] + e_sh[c]) into the fp32 OIHW gradient
 * dw (128, N, 1, 1) -- the same result as cx_conv_gemm followed by cx_conv_wgrad with x_prologue = AFFINE_RELU(e_sc, e_sh). */
int cx_conv1x1_dgrad_wgrad(const CxConv* p, float* dw, void* stream);
/* the same with a workspace for the reproducible weight-gradient sum (see CxWgrad.scratch; NULL / 0 = atomics) */
int cx_conv1x1_dgrad_wgrad_ws(const CxConv* p, float* dw, float* scratch, int64_t scratch_floats, void* stream);
/* ABI 9.  The same with dw a column range of a wider fp32 matrix: row n of the (128, p->N) result goes to dw[n * dw_ld + c] (the 32
 * newest input channels of a dense layer's conv1 weight, torchvision `_DenseLayer.conv1` as restated at attn_aug_conv.py:13).     */
int cx_conv1x1_dgrad_wgrad_ld_ws(const CxConv* p, float* dw, int dw_ld, float* scratch, int64_t scratch_floats, void* stream);
/* ABI 9.  TWO dense layers of one dense block in one pass over the block's activation and gradient buffers: a = layer l restricted to
 * the N channels it shares with b = layer l - 1 (its 32 newest channels go through cx_conv1x1_dgrad_wgrad_ld_ws first: layer l - 1's
 * output gradient depends on them).  Both add e_scale * mask * (dZ W) to y[..., :N] (the second layer on top of the first, each sum
 * rounded to bf16 as the separate passes round it: y is bit-identical to them) and accumulate their weight gradients (dw_a: pitch
 * dw_ld_a, dw_b: pitch N) and statistic rows (a->stat_*, b->stat_*: distinct buffers, same geometry); x and the old gradient are read
 * once and the new gradient written once for the pair.  a and b share ex, y, N, B/H/W, ldex, ldy, accumulate, stat_det and
 * stat_replicas (stat_rstride is each layer's own); prologue AFFINE2, epilogue MASK, K = 128 (accumulate = 0: layer a takes the old gradient as zero, layer
 * b adds to layer a's).  scratch: 2 * splits * 128 * N floats for the ordered sums
 * (cx_last_slab_floats() reports what was used), or NULL for atomics.  No reference counterpart (autograd runs the layers one by one). */
int cx_conv1x1_dgrad_wgrad_pair_ws(const CxConv* a, const CxConv* b, float* dw_a, int dw_ld_a, float* dw_b, float* scratch,
                                   int64_t scratch_floats, void* stream);

/* OIHW fp32 -> packed bf16.  transpose=0: [tap][O][I] (forward);  transpose=1: [tap'][I][O] with
 * taps rotated by 180 degrees (input-gradient of a stride-1 conv).  stem=1: (64,3,7,7) -> [ky][O][8*4].  */
int cx_pack_weights(const float* w_oihw, void* packed, int O, int I, int kh, int kw, int transpose, int stem,
                    void* stream);

/* The same for every conv weight of a model in ONE launch: `flat` is the flat fp32 parameter buffer,
 * `table_dev` a DEVICE array of descriptors (element offsets into flat / packed).                  */
typedef struct CxPackDesc {
  int64_t src_off, dst_off;
  int32_t O, I, kh, kw, transpose, stem;
} CxPackDesc;
int cx_pack_weights_table(const float* flat, void* packed, const CxPackDesc* table_dev, int n_desc, void* stream);

/* (B,3,H,W) fp32 NCHW -> (B,H,W,4) bf16 (4th channel zero).  Replaces x.to(device) layout glue
 * ahead of features.conv0 (chexpert.py:159).                                                      */
int cx_nchw3_to_nhwc4(const float* x, void* y, int B, int H, int W, void* stream);
/* uint8 grey image (B,H,W) -> (B,H,W,4) bf16 with the three identical whitened channels ((u/255 - mean)/std) and a zero pad:
 * the reference transform chain `float().div(255)`, `Normalize(mean, std)`, `expand(3,-1,-1)` (chexpert.py:70-72) done on
 * the GPU from the decoded bytes, so the host pipeline ships 1 B per pixel instead of 12.
 * npix = B*H*W must be a multiple of 16.                                                                             */
int cx_u8_to_nhwc4(const uint8_t* x, void* y, size_t npix, float mean, float std, void* stream);

/* BatchNorm training statistics -> (scale, shift) of the consumer + running-stat update
 * (F.batch_norm, momentum semantics of nn.BatchNorm2d incl. unbiased running_var).
 * sum/sq: fp32 [C] over `count` elements.  gamma/beta may be NULL (-> 1, 0: InstanceNorm-like).
 * running_* may be NULL.  Also emits mean / rstd when non-NULL.                                   */
int cx_bn_coef(const float* sum, const float* sq, float count, const float* gamma, const float* beta, float eps,
               float momentum, float* running_mean, float* running_var, float* scale, float* shift, float* mean,
               float* rstd, int C, int replicas, int rstride, void* stream);   /* sum/sq: `replicas` copies, `rstride` floats apart */
/* BatchNorm coefficients from per-channel moments that already exist (a dense-block channel's batch mean / rstd are computed once,
 * by the kernel that produced the channel; every later norm1 over the concatenation -- torchvision _DenseLayer.norm1 -- re-uses
 * them with its own gamma / beta / running buffers).  Channels [c_lo, c_lo + c_n) are reduced first, in row order, from `rows`
 * deterministic statistic rows (CxConv.stat_det) into mean / rstd.                                                             */
int cx_bn_coef_moments(float* mean, float* rstd, float count, const float* gamma, const float* beta, float eps, float momentum,
                       float* running_mean, float* running_var, float* scale, float* shift, int C, const float* sum, const float* sq,
                       int rows, int rstride, int c_lo, int c_n, void* stream);
/* eval mode: scale/shift from running statistics                                                 */
int cx_bn_coef_eval(const float* running_mean, const float* running_var, const float* gamma, const float* beta,
                    float eps, float* scale, float* shift, float* mean, float* rstd, int C, void* stream);

/* Backward bookkeeping of one consumer BatchNorm over buffer channels [0,C):
 *   dgamma += S2, dbeta += S1 (fp32 parameter gradients);
 *   deferred per-channel correction  A[c] += r*gamma*S1/count,  Bc[c] += r*gamma*S2/count
 * (the -mean(dz) - xhat*mean(dz*xhat) terms of BN backward are linear in x and shared by every
 * consumer of a dense-block channel, so they are applied once, by the channel's producer).
 * If pa/pb/pc are non-NULL also emits the AFFINE2 vectors of a SINGLE-consumer BN (norm2):
 *   dY = dz*pa + y*pb + pc.                                                                       */
int cx_bn_bwd_coef(const float* S1, const float* S2, float count, const float* gamma, const float* mean,
                   const float* rstd, float* dgamma, float* dbeta, float* A, float* Bc, float* pa, float* pb,
                   float* pc, int C, int replicas, int rstride,
                   /* optional: the cx_bn_bwd_slice_coef vectors of channels [q_lo, q_lo + q_n) from the A / B this call has just
                      completed (their last consumer), qa/qb/qc of q_n floats, or NULL                                   */
                   float* qa, float* qb, float* qc, int q_lo, int q_n, void* stream);   /* S1/S2 replicated as above */
/* Frozen (eval-mode) form of cx_bn_bwd_coef: BatchNorm with the running statistics m = running_mean, r = 1/sqrt(running_var+eps)
 * has dx = gamma*r*dy and no batch-statistic terms.  S1 = sum dy and S2 = sum dy*(x-mean)*rstd were reduced by the producer
 * against the basis (mean, rstd) it read, which may differ from (m, r) (a dense-block channel's consumers share one basis):
 *   dgamma += S2*(r/rstd) + r*(mean-m)*S1,  dbeta += S1;
 *   pa = gamma*r, pb = pc = 0 (if pa is non-NULL);  qa/qb/qc of channels [q_lo, q_lo+q_n) = 1, 0, 0 (if qa is non-NULL).
 * gamma may be NULL (1).  Deterministic: the rows are summed in a fixed order, no atomics.                                      */
int cx_bn_bwd_coef_eval(const float* S1, const float* S2, const float* mean, const float* rstd, const float* running_mean,
                        const float* running_var, const float* gamma, float eps, float* dgamma, float* dbeta, float* pa, float* pb,
                        float* pc, int C, int replicas, int rstride, float* qa, float* qb, float* qc, int q_lo, int q_n,
                        void* stream);
/* AFFINE2 vectors that apply the deferred correction to a gradient slice:
 *   dY_true = G*1 + x*(-r*Bc) + (mean*r*Bc - A)                                                   */
int cx_bn_bwd_slice_coef(const float* A, const float* Bc, const float* mean, const float* rstd, float* pa,
                         float* pb, float* pc, int C, void* stream);

/* stem: y = maxpool3x3s2p1(relu(x*scale+shift)) into a channel slice + stats of the pooled output
 * (features.norm0/relu0/pool0, attn_aug_conv.py:462-464).  argmax: (B,H/2,W/2,C) uint8 window
 * position (0..8) of the first maximum, kept for the backward pass.                               */
int cx_bnrelu_maxpool_fwd(const void* x, const float* scale, const float* shift, void* y, uint8_t* argmax,
                          float* stat_sum, float* stat_sq, int B, int H, int W, int C, int ldy, int stat_rows, void* stream);
/* backward of the same: routes (corrected) dY to the arg-max, applies the ReLU mask, writes dz (bf16,
 * (B,H,W,C)) and accumulates S1 = sum dz, S2 = sum dz*xhat                                       */
int cx_bnrelu_maxpool_bwd(const void* x, const float* scale, const float* shift, const float* mean,
                          const float* rstd, const uint8_t* argmax, const void* g, const void* gx, const float* ga,
                          const float* gb, const float* gc, void* dz, float* S1, float* S2, int B, int H, int W, int C,
                          int ldg, int ldgx, int stat_rows, void* stream);

/* head: pooled[b][c] = mean_hw relu(x*scale+shift); logits = pooled @ Wt + bias
 * (attn_aug_conv.py:514-516)                                                                      */
int cx_head_fwd(const void* x, const float* scale, const float* shift, const float* w, const float* bias,
                float* pooled, float* logits, int B, int HW, int C, int ldx, int n_classes, void* stream);
/* loss = BCEWithLogits(logits,target).sum(1).mean(0); dlogits = (sigmoid - target)/B * grad_scale
 * (chexpert.py:160, :530)                                                                         */
int cx_bce_fwd_bwd(const float* logits, const float* target, float* loss, float* loss_elem, float* dlogits,
                   float grad_scale, int B, int n_classes, void* stream);
/* cx_bce_fwd_bwd with ignored labels and class weights: the uncertainty policies the reference asks for (dataset.py:119, :141
 * "setup options for uncertain labels") and torch's BCEWithLogitsLoss(pos_weight).  Per element, x = logits[b][c], t = target[b][c],
 * p = pos_weight ? pos_weight[c] : 1:
 *   t < 0   ignored: loss_elem = 0, dlogits = 0, nothing added to loss
 *   else    w = 1 + (p-1) t;  l = (1-t) x + w (log1p(exp(-|x|)) + max(-x, 0));  dl/dx = (1-t) - w (1 - sigmoid(x))
 * loss = sum l / B (the divisor stays the batch size, whatever is ignored: .sum(1).mean(0) over the masked element losses),
 * dlogits = dl/dx / B * grad_scale.  Soft targets in [0,1] are valid.  pos_weight: fp32 [n_classes] on the device, or NULL; with
 * NULL a live element runs cx_bce_fwd_bwd's expressions, so targets without negatives give its loss, loss_elem and dlogits bit for
 * bit.  loss, loss_elem and dlogits are optional.  One workgroup, fixed tree, no atomics: bit-reproducible.  Additive entry point
 * of ABI 10 (no struct changed).                                                                                               */
int cx_bce_masked_fwd_bwd(const float* logits, const float* target, const float* pos_weight, float* loss, float* loss_elem,
                          float* dlogits, float grad_scale, int B, int n_classes, void* stream);
/* AUC min-max-margin loss (Yuan et al., ICCV 2021) with its gradients, one launch (loss.hip).  Per class c, over the batch rows i, with
 * x = logits[i][c], y = sigmoid(x), t = target[i][c], p = prior[c] in (0, 1), m = margin > 0, (a, b, alpha) = aux[0][c], aux[1][c],
 * aux[2][c]; a row is live when t >= 0 (t < 0 is ignored as in cx_bce_masked_fwd_bwd), positive (P) when live and t >= 0.5, negative
 * (N) when live and t < 0.5, L = number of live rows:
 *   inner      = p (1-p) m + sum(p y N - (1-p) y P) / L
 *   loss_c     = (1-p) sum((y-a)^2 P) / L + p sum((y-b)^2 N) / L + 2 alpha inner - p (1-p) alpha^2
 *   dloss/dx_i = y (1-y) / L [P (1-p) (2 (y-a) - 2 alpha) + N p (2 (y-b) + 2 alpha)]              (0 for an ignored row)
 *   dloss/da   = -(1-p) sum(2 (y-a) P) / L,  dloss/db = -p sum(2 (y-b) N) / L,  dloss/dalpha = 2 inner - 2 p (1-p) alpha
 * and loss = sum_c loss_c.  A class without a live row adds nothing: loss_c = 0 and its three auxiliary gradients are 0, so the
 * update below leaves its scalars alone.  prior: fp32 [n_classes]; aux, daux: fp32 (3, n_classes); loss: one float; loss_class:
 * [n_classes] (the loss_c); dlogits: (B, n_classes) = dloss/dx * grad_scale (grad_scale touches nothing else).  loss, loss_class,
 * dlogits and daux may each be NULL.  One workgroup; the per-class sums run in double over a fixed tree, no atomics: bit-reproducible.
 * Any B >= 1 and n_classes >= 1.  CX_EINVAL before anything is launched: NULL logits / target / prior / aux, B < 1, n_classes < 1,
 * margin <= 0.  Additive entry points of ABI 10 (no struct changed).                                                             */
int cx_aucm_fwd_bwd(const float* logits, const float* target, const float* prior, const float* aux, float margin, float* loss,
                    float* loss_class, float* dlogits, float* daux, float grad_scale, int B, int n_classes, void* stream);
/* primal descent on a and b, dual ascent on alpha, from the gradients of the same step: a -= lr da, b -= lr db,
 * alpha = max(0, alpha + lr dalpha), lr = *lr_aux_dev (a device float: a captured step sees a changed rate).                      */
int cx_aucm_aux_step(float* aux, const float* daux, const float* lr_aux_dev, int n_classes, void* stream);
/* Focal loss (Lin et al., ICCV 2017) and asymmetric loss (Ridnik et al., ICCV 2021) with d loss / d logits, one launch (loss.hip).
 * focus: FOUR floats ON THE DEVICE, [gamma+ >= 0, gamma- >= 0, clip m in [0, 1), alpha in (0, 1) or a negative number for "none"];
 * the kernel reads them from memory, so a captured step sees a change made in place.  Per element, x = logits[b][c],
 * t = target[b][c], w = pos_weight ? pos_weight[c] : 1, p = sigmoid(x), q = sigmoid(-x), p_m = max(p - m, 0), p_n = min(q + m, 1):
 *   t < 0   ignored: loss_elem = 0, dlogits = 0, nothing added to loss (as in cx_bce_masked_fwd_bwd)
 *   else    C = -(w t log p + (1-t) log p_n);  u = t q + (1-t) p_m;  g = gamma+ t + gamma- (1-t);  f = g == 0 ? 1 : u^g;
 *           a = alpha < 0 ? 1 : alpha t + (1-alpha)(1-t);  l = a f C
 * loss = sum l / B (the divisor stays the batch size), dlogits = dl/dx / B * grad_scale with the exact derivative (f is not
 * detached; d p_m / dx = p q where p > m, 0 elsewhere).  A hard negative at or below the clip (t == 0, p <= m) gives l = 0 and
 * dl/dx = 0 exactly, whatever gamma- is (u = 0: the derivative of 0^g is taken as 0).  Soft targets in [0, 1] are valid.  gamma+ =
 * gamma- and m = 0 is the focal loss (torchvision's sigmoid_focal_loss summed over the classes and averaged over the batch), all
 * zero and no alpha the (weighted, masked) cross-entropy.  pos_weight: fp32 [n_classes] on the device, or NULL.  loss (one float),
 * loss_elem and dlogits (B, n_classes) may each be NULL.  One workgroup, the sum in double over a fixed tree, no atomics:
 * bit-reproducible.  CX_EINVAL before anything is launched: NULL logits / target / focus, B < 1, n_classes < 1.  The values of
 * focus are the caller's to keep in range.  Additive entry point of ABI 10 (no struct changed).                                  */
int cx_asl_fwd_bwd(const float* logits, const float* target, const float* pos_weight, const float* focus, float* loss,
                   float* loss_elem, float* dlogits, float grad_scale, int B, int n_classes, void* stream);
/* U-MultiClass (Irvin et al., "CheXpert", AAAI 2019): a three-way softmax cross-entropy per finding, with d loss / d logits, one launch
 * (loss.hip).  The head has 3n outputs; finding k of row b owns logits[b][3k + 0] (negative), [3k + 1] (positive) and [3k + 2]
 * (uncertain).  target: the (B, n) fp32 table of the sigmoid losses; the class of element (b, k) is c = 2 if t < 0, 1 if t >= 0.5,
 * else 0.  Nothing is ignored and there is no soft-target form.  Per element, with (z0, z1, z2) its three logits:
 *   m = max(z0, z1, z2);  e_j = expf(z_j - m);  s = (e0 + e1) + e2
 *   r = the sum of the two e_j with j != c, added in index order (never s - e_c)
 *   l = z_c == m ? log1pf(r) : (m - z_c) + logf(s)                                   = -log softmax_c
 *   dl/dz_j = e_j / s for j != c,  -r / s for j == c (never e_c / s - 1)
 * so a confident correct element keeps its digits (elements whose target logit leads by 4 .. 12: within 7e-7 of their float64 values
 * in an fp32 model of this statement, where m + logf(s) - z_c is off by 4e-3 .. 1.3e-2).  class_weight: fp32 (n, 3) on the device,
 * or NULL: l and its three gradients are multiplied by w[k][c]; a table of ones gives the bits of NULL.  loss = sum w l / B (sum over
 * the findings, mean over the batch: the reduction and divisor of cx_bce_fwd_bwd; weights do not change the divisor), loss_elem (B, n)
 * = w l, dlogits (B, 3n) = w dl/dz / B * grad_scale.  loss, loss_elem and dlogits may each be NULL.  One workgroup, the sum in double
 * over a fixed tree, no atomics: bit-reproducible.  CX_EINVAL before anything is launched: NULL logits / target, B < 1, n < 1,
 * B * n > INT_MAX - 256.  Additive entry points of ABI 10 (no struct changed).                                                     */
int cx_mc3_fwd_bwd(const float* logits, const float* target, const float* class_weight, float* loss, float* loss_elem,
                   float* dlogits, float grad_scale, int B, int n, void* stream);
/* The test-time form of those logits: z[b][k] = z1 - z0 (one fp32 subtraction), so that sigmoid(z) = p1 / (p0 + p1), the softmax
 * over the two classes left when "uncertain" is dropped -- everything that takes binary (B, n) logits takes z --, and, where p_unc is
 * given, p_unc[b][k] = e2 / s with m, e, s as above.  One thread per (b, k), no reduction; any B * n <= INT_MAX - 256 (a whole
 * validation table in one call).  CX_EINVAL before anything is launched: NULL logits / z, B < 1, n < 1, the size cap.            */
int cx_mc3_collapse(const float* logits, float* z, float* p_unc, int B, int n, void* stream);
/* Hierarchical label loss (Chen et al., "Deep hierarchical multi-label classification of chest X-ray images", MIDL 2019: HLCP and HLUP;
 * the conditional training of Pham et al., 2019) on the (B, n) logits of a step, with d loss / d logits, one launch (loss.hip).  The
 * labels form a forest: parent[k] == -1 is a root, else 0 <= parent[k] < k (parents come before children); parent is int32 [n] ON THE
 * DEVICE, read by the kernel, so a captured step sees a table rewritten in place.  path(k) is k and its ancestors, root first, at most
 * CX_HIER_MAX_PATH nodes; n <= CX_HIER_MAX_LABELS.  EVERY logit is the logit of the conditional probability P(k | parent(k) positive),
 * in both modes.  target: the (B, n) table of cx_bce_masked_fwd_bwd (t < 0 ignored, soft targets in [0, 1] valid); pos_weight: fp32 [n]
 * on the device, or NULL.
 *   mode 0, conditional: element (b, k) is live iff t >= 0 and the target of every proper ancestor is >= 0.5; a live element is the
 *     element of cx_bce_masked_fwd_bwd (its unweighted or weighted expressions, its fp32 or double sum, its stride and tree), any other
 *     gives loss_elem = 0 and dlogits = 0.  A table of roots gives cx_bce_masked_fwd_bwd's bits in all three outputs.
 *   mode 1, unconditional: the cross-entropy of P_k = prod_{j in path(k)} sigmoid(z_j); element (b, k) is live iff t >= 0 (ancestors'
 *     targets are not read).  Per node, from one e = log1pf(expf(-|z|)):  lp = -(max(-z, 0) + e) = log sigmoid(z),  lq = -(max(z, 0) + e)
 *     = log sigmoid(-z).  Along the path, root first:  u = sum lp_j = log P_k;  a_j = (sum_{i before j} lp_i) + lq_j, the logarithms of
 *     the positive terms of 1 - P = sum_j (prod_{i<j} p_i) q_j.  l1m = log(1 - P_k) = log1pf(-expf(u)) where u <= -ln 2, else
 *     max_j a_j + logf(sum_j expf(a_j - max)): no 1 - P is formed from a rounded P, and a small loss keeps its digits.  With
 *     w = pos_weight ? pos_weight[k] : 1:   l = -w t u - (1 - t) l1m,   dl/dz_j = (1 - t) expf(u + lq_j - l1m) - w t q_j  for every j in
 *     path(k), q_j = 1 / (1 + expf(z_j)) (the exponent form: q_j expf(u - l1m) is 0 * inf at z = +1e4).  dlogits[b][j] is the sum of these
 *     over the k of j's subtree in ascending k, times 1 / B * grad_scale.  A pos_weight of ones gives the bits of NULL.
 * loss = sum l / B (the divisor stays the batch size).  loss (one float), loss_elem and dlogits (B, n) may each be NULL; each alone
 * has the bits it has beside the others.  One workgroup, a fixed tree (the sum in double in mode 1), no atomics: bit-reproducible.
 * CX_EINVAL before anything is launched: NULL logits / target / parent, B < 1, n < 1, n > CX_HIER_MAX_LABELS, a mode other than 0 / 1,
 * B * n > INT_MAX - 256.  The table's VALUES are the caller's to keep in range (it is device memory); for memory safety alone the
 * kernels read an entry outside [-1, k) as a root and cut a path after CX_HIER_MAX_PATH nodes.  Additive entry points of ABI 10.    */
#define CX_HIER_MAX_LABELS 64
#define CX_HIER_MAX_PATH 8
int cx_hier_fwd_bwd(const float* logits, const float* target, const int* parent, const float* pos_weight, int mode, float* loss,
                    float* loss_elem, float* dlogits, float grad_scale, int B, int n, void* stream);
/* The test-time form of those logits: the logit of the UNCONDITIONAL probability.  A root's z is its logit, copied bit for bit; any other
 * z[b][k] = u - l1m with the expressions of mode 1, so that sigmoid(z) = P_k; p (optional) = expf(u).  One thread per (b, k), no
 * reduction; any B (a whole validation table in one call).  CX_EINVAL before anything is launched: NULL logits / parent / z, B < 1,
 * n < 1, n > CX_HIER_MAX_LABELS, B * n > INT_MAX - 256.                                                                             */
int cx_hier_collapse(const float* logits, const int* parent, float* z, float* p, int B, int n, void* stream);
/* NT-Xent / SupCon (Chen et al., "A Simple Framework for Contrastive Learning of Visual Representations", ICML 2020; Khosla et al.,
 * "Supervised Contrastive Learning", NeurIPS 2020, L_out) on the (N, d) embeddings e of a step, with the exact d loss / d e, three launches
 * (loss.hip).  ids: fp32 (N, 1) ON THE DEVICE, integer-valued (exact below 2^24); temperature: one fp32 value ON THE DEVICE, read by the
 * kernels, so a captured step sees it rewritten in place.
 *   V = {i : ids_i >= 0}; a row outside V is neither an anchor nor a negative: its element loss and its gradient row are 0, top1 is -1,
 *     and its embedding reaches no other row's bits.
 *   z_i = e_i / max(|e_i|, 1e-12);  s_ij = z_i . z_j / tau;  for i in V:  A(i) = V \ {i},  P(i) = {j in A(i) : ids_j == ids_i}
 *   anchors: the rows of V with |P(i)| >= 1, M of them.  With m_i = max_{a in A(i)} s_ia:
 *     lse_i = m_i + logf(sum_a expf(s_ia - m_i));   l_i = logf(sum_a expf(s_ia - m_i)) - sum_p (s_ip - m_i) / |P(i)|
 *   loss = sum l_i / M (0 where M == 0, and then every gradient is 0);  loss_elem (N, 1) = l_i (0 for a row that is no anchor)
 *   top1 (N,) int32 = the a in A(i) with the largest s_ia, the lowest such a on a tie; -1 outside V or where A(i) is empty
 *   dS_ij = [i anchor] (expf(s_ij - lse_i) - [j in P(i)] / |P(i)|);   dz_i = sum_{j in A(i)} (dS_ij + dS_ji) z_j / (tau M)
 *   dlogits (N, d) = (dz_i - (dz_i . z_i) z_i) / |e_i| * grad_scale where |e_i| >= 1e-12, dz_i / 1e-12 * grad_scale below the clamp
 * Every id occurring exactly twice is SimCLR's NT-Xent.  fp32 on the VALU; every sum in a fixed order, no atomics: bit-reproducible, and
 * each output alone has the bits it has beside the others.  loss, loss_elem, dlogits and top1 may each be NULL.  scratch: the caller's,
 * cx_ntxent_scratch(N, d) = N d + 4 N floats (z | |e| | lse | 1 / |P| | l), nothing is allocated here.  CX_EINVAL before anything is
 * launched: NULL e / ids / temperature / scratch, N < 1, d < 1, scratch_floats below cx_ntxent_scratch(N, d); CX_ESHAPE: N >
 * CX_NTXENT_MAX_N or d > CX_NTXENT_MAX_D (the row of similarities and two d-vectors live in LDS).  cx_ntxent_scratch returns 0 for sizes
 * the loss refuses.  |e_i|^2 is formed in fp32: embeddings beyond 1e18 overflow it.  Additive entry points of ABI 10.                */
#define CX_NTXENT_MAX_N 4096
#define CX_NTXENT_MAX_D 1024
long long cx_ntxent_scratch(int N, int d);
int cx_ntxent_fwd_bwd(const float* e, const float* ids, const float* temperature, float* loss, float* loss_elem, float* dlogits,
                      int* top1, float grad_scale, float* scratch, long long scratch_floats, int N, int d, void* stream);
/* Barlow Twins (Zbontar et al., "Barlow Twins: Self-Supervised Learning via Redundancy Reduction", ICML 2021) on the (N, d) embeddings e
 * of a step, with the exact d loss / d e through the batch normalisation; four launches (barlow.hip), the three products on the
 * fp32-input MFMA.  ids: fp32 (N, 1) ON THE DEVICE, read as a mask only; lambda: one fp32 value ON THE DEVICE, read by the kernels, so a
 * captured step sees it rewritten in place.
 *   h = N / 2; row p < h is view A of pair p, row p + h view B (the [x; x] layout); with an odd N the last row belongs to no pair.
 *   V = {p < h : ids_p >= 0 and ids_{p+h} >= 0}, m = |V| counted on the device.  A row of a pair outside V, and the odd last row, get a
 *     gradient row of exact zeros, and their embeddings reach no other output's bits, even when they hold NaN.
 *   per view and column k, over p in V:  mu_k = sum a_pk / m;  v_k = sum (a_pk - mu_k)^2 / m (biased, two passes);
 *     a^_pk = (a_pk - mu_k) / sqrt(v_k + CX_BARLOW_EPS), 0 for p outside V;  b^ likewise from view B
 *   C_kl = sum_p a^_pk b^_pl / m;  on = sum_k (1 - C_kk)^2;  off = sum_{k != l} C_kl^2;  loss = on + lambda off (no further scale)
 *   G_kk = -2 (1 - C_kk), G_kl = 2 lambda C_kl (k != l);  da^ = b^ G^T / m;  db^ = a^ G / m
 *   da_p. = (da^_p. - mean_p da^ - a^_p. * mean_p (da^ o a^)) / sqrt(v + eps), db likewise (BatchNorm's backward).  The kernels use the
 *     closed forms mean_p da^ = 0 and mean_p (da^ o a^)_k = sum_l G_kl C_kl / m (for view B the column sums), which hold in exact
 *     arithmetic, so the way back through the normalisation is the epilogue of the product.
 *   dlogits (N, d) = these rows * grad_scale;  stats (4,) = [on, off, mean_k C_kk, m]
 *   m < 2: loss and every gradient are exactly 0, stats = [0, 0, 0, m].  A constant column gives a^ = 0 and C_kk = 0; all stays finite.
 * fp32; every sum in a fixed order (the tiles' shares of on / off / the diagonal are added in tile order in double), no atomics:
 * bit-reproducible, and each output alone has the bits it has beside the others.  loss, dlogits and stats may each be NULL.  scratch: the
 * caller's, nothing is allocated here.  With r4(x) = x rounded up to a multiple of 4, d4 = r4(d), nt = ceil(d / 64) it holds, in floats:
 *   a^ (r4(h d)) | b^ (r4(h d)) | G (r4(d d)) | 1 / sqrt(v + eps) of view A, of view B (d4 each) | sum_l G_kl C_kl (d4) |
 *   sum_k G_kl C_kl (d4) | m (4) | the 64 x 64 tiles' [on, off, sum C_kk, -] (4 nt nt) | the tiles' row sums of G o C (nt d4) | their
 *   column sums (nt d4);  cx_barlow_scratch(N, d) is the total.
 * CX_EINVAL before anything is launched: NULL e / ids / lambda / scratch, N < 2, d < 1, scratch_floats below cx_barlow_scratch(N, d);
 * CX_ESHAPE: N > CX_BARLOW_MAX_N or d > CX_BARLOW_MAX_D (the pair mask lives in LDS; 1024 is the width the head is exercised at).
 * cx_barlow_scratch returns 0 for sizes the loss refuses.  Additive entry points of ABI 10.                                           */
#define CX_BARLOW_MAX_N 4096
#define CX_BARLOW_MAX_D 1024
#define CX_BARLOW_EPS 1e-5f
long long cx_barlow_scratch(int N, int d);
int cx_barlow_fwd_bwd(const float* e, const float* ids, const float* lambda, float* loss, float* dlogits, float* stats, float grad_scale,
                      float* scratch, long long scratch_floats, int N, int d, void* stream);
/* loss = CrossEntropyLoss(logits, target) (mean over the batch of logsumexp - logit[target]);
 * dlogits = (softmax - onehot)/B * grad_scale; loss_elem (optional) = the per-sample terms
 * (models/test_model.py:118, :143, :331: the CIFAR harness criterion)                              */
int cx_softmax_ce_fwd_bwd(const float* logits, const int64_t* target, float* loss, float* loss_elem, float* dlogits,
                          float grad_scale, int B, int n_classes, void* stream);
/* head backward: dW += dlogits^T pooled, db += sum dlogits, dpooled = dlogits @ W;
 * then gradient into the block buffer through GAP + ReLU + norm5 (mask epilogue semantics):
 * dz = dpooled/HW * [x*scale+shift>0]; S1,S2 += ...; g = e_scale*dz (written, not accumulated)   */
int cx_head_bwd(const float* dlogits, const float* pooled, const float* w, float* dw, float* db,
                float* dpooled, int B, int C, int n_classes, void* stream);
int cx_gap_relu_bn_bwd(const float* dpooled, const void* x, const float* scale, const float* shift,
                       const float* mean, const float* rstd, const float* e_scale, void* g, float* S1, float* S2,
                       int B, int HW, int C, int ldx, int ldg, int stat_rows, void* stream);

/* transition backward glue: un-pool (each of the 4 inputs gets d/4), ReLU mask + BN mask epilogue */
int cx_unpool2_mask(const void* d, const void* x, const float* sc, const float* sh, const float* mean,
                    const float* rstd, const float* e_scale, void* g, float* S1, float* S2, int B, int H, int W,
                    int C, int ldd, int ldx, int ldg, int stat_rows, void* stream);

/* residual join of a Bottleneck: out = relu(a*pa + b*pb + pc) (bn3(conv3) + identity | bn_d(downsample),
 * attn_aug_conv.py:202-209); pa/pb/pc fp32 [C]                                                    */
int cx_affine2_relu(const void* a, const void* b, const float* pa, const float* pb, const float* pc, void* out, size_t rows,
                    int C, void* stream);
/* ABI 9.  Dropout on the new feature slice of a dense layer (torchvision `_DenseLayer.forward`: `F.dropout(new_features, p=drop_rate,
 * training=self.training)`; the reference's DenseNet hands drop_rate to torchvision's _DenseBlock, attn_aug_conv.py:453, :479-481), in place on the slice
 * y[m * ld + c], m < rows, c < C (C % 8 == 0): y = keep ? y / (1 - p) : 0, keep = hash(seed[0], uid, m * C + c) >= p * 2^32 (a
 * counter-based hash: nothing is stored, _bwd regenerates the decisions; seed is a DEVICE int64 so that a replayed hipGraph draws
 * new decisions every step).  S1 / S2 (optional): one row per workgroup of the sums / sums of squares of the result over the
 * slice's channels, at most stat_rows rows (cx_last_stat_rows() reports how many) -- they replace the rows the producing convolution
 * wrote.  _bwd, in place on the gradient slice g with the stored (post-dropout) activations x: g = keep ? (qa g + qb x + qc) /
 * (1 - p) : 0, i.e. the deferred BatchNorm correction of the slice with the keep decision on top; the 3x3 input-gradient and weight-
 * gradient kernels then read g with identity coefficients.                                                                          */
int cx_dropout_slice_fwd(void* y, int ld, int64_t rows, int C, float p, const int64_t* seed, uint32_t uid, float* S1, float* S2,
                         int stat_rows, void* stream);
int cx_dropout_slice_fwd_f32(void* y, int ld, int64_t rows, int C, float p, const int64_t* seed, uint32_t uid, float* S1, float* S2,
                             int stat_rows, void* stream);
int cx_dropout_slice_bwd(void* g, int ldg, const void* x, int ldx, const float* qa, const float* qb, const float* qc, int64_t rows, int C,
                         float p, const int64_t* seed, uint32_t uid, void* stream);
int cx_dropout_slice_bwd_f32(void* g, int ldg, const void* x, int ldx, const float* qa, const float* qb, const float* qc, int64_t rows,
                             int C, float p, const int64_t* seed, uint32_t uid, void* stream);
/* its backward: dz = dout * [out > 0]; S1 += sum dz; S2a += sum dz*(a-mu_a)*r_a; S2b += sum dz*(b-mu_b)*r_b
 * (b / S2b optional).  dz may alias dout.                                                         */
int cx_relu_bwd_stats(const void* dout, const void* out, const void* a, const float* mu_a, const float* r_a, const void* b,
                      const float* mu_b, const float* r_b, void* dz, float* S1, float* S2a, float* S2b, size_t rows, int C,
                      int stat_rows, void* stream);
/* ABI 9.  Residual join forward of a Bottleneck (attn_aug_conv.py:202-209: `out += identity; out = relu(out)` behind bn3) with the
 * residual stream kept as TWO planes: t = relu(a*pa[c] + (b [+ b_lo])*pb[c] + pc[c]) per element of (rows, C) bf16 tensors;
 * out = bf16(t) (the tensor every convolution reads), out_lo = the next 8 mantissa bits of t as a signed byte per element (NULL:
 * single-plane output, the cx_affine2_relu_mask form), mask = sign bits, one byte per 8-channel chunk (NULL: not written).  Side-plane
 * layout (lo planes and every sign-bit plane of this library, also cx_affine2_relu_mask / cx_relu_bwd_stats_mask / CxConv.emask):
 * chunk q (channels 8q..8q+7) of row m is chunk number ((q/8)*rows + m)*8 + q%8 where C % 64 == 0 -- blocks of 64 channels, so a
 * convolution k-step writes whole 128-byte lines -- and m*(C/8) + q otherwise.  b_lo = lo plane of b (NULL:
 * b is a single-plane tensor, e.g. the downsample convolution's raw output).  The reference keeps the stream in fp32; rounded to
 * bf16 at each of resnet152's 50 joins it alone costs 1.0e-2 of the train logits' abs-max -- with the lo plane 2^-17 per join.
 * cx_conv_gemm with CX_PRO_JOIN computes the same bits in the prologue of the next block's conv1.                                 */
int cx_join_fwd(const void* a, const void* b, const int8_t* b_lo, const float* pa, const float* pb, const float* pc, void* out,
                int8_t* out_lo, uint8_t* mask, size_t rows, int C, void* stream);
/* ABI 5: the same pair with the sign of `out` kept as one bit per element (mask: uint8 [rows * C / 8], byte i = the 8 channels
 * of chunk i, bit j = out[8 i + j] > 0), written by the forward and read by the backward INSTEAD of `out` (a quarter of the
 * backward's read bytes).  mask == NULL: the forms above.  `out` may be NULL in the backward when mask is given.            */
int cx_affine2_relu_mask(const void* a, const void* b, const float* pa, const float* pb, const float* pc, void* out, uint8_t* mask,
                         size_t rows, int C, void* stream);
int cx_relu_bwd_stats_mask(const void* dout, const void* out, const uint8_t* mask, const void* a, const float* mu_a,
                           const float* r_a, const void* b, const float* mu_b, const float* r_b, void* dz, float* S1, float* S2a,
                           float* S2b, size_t rows, int C, int stat_rows, void* stream);
/* the same two in the fp32 storage mode (a, b, out, dout, dz fp32; north_star "1e-3 fp32" for the ResNets) */
int cx_affine2_relu_mask_f32(const void* a, const void* b, const float* pa, const float* pb, const float* pc, void* out, uint8_t* mask,
                             size_t rows, int C, void* stream);
int cx_relu_bwd_stats_mask_f32(const void* dout, const void* out, const uint8_t* mask, const void* a, const float* mu_a, const float* r_a,
                               const void* b, const float* mu_b, const float* r_b, void* dz, float* S1, float* S2a, float* S2b,
                               size_t rows, int C, int stat_rows, void* stream);

/* dz (B,H,W,C) bf16 -> dY = dz*pa + x*pb + pc in place (BN0 backward ahead of the stem wgrad)      */
int cx_affine2_inplace(void* dz, const void* x, const float* pa, const float* pb, const float* pc, size_t rows,
                       int C, void* stream);

/* fused optimisers on flat fp32 buffers (torch.optim.Adam / SGD(nesterov) / RMSprop(momentum) as
 * wired at chexpert.py:470, :479, :499)                                                           */
int cx_adam_step(float* p, const float* g, float* m, float* v, size_t n, float lr, float beta1, float beta2,
                 float eps, float weight_decay, int step, float grad_scale, void* stream);
int cx_sgd_nesterov_step(float* p, const float* g, float* buf, size_t n, float lr, float momentum,
                         float weight_decay, int first_step, float grad_scale, void* stream);
int cx_rmsprop_step(float* p, const float* g, float* sq, float* buf, size_t n, float lr, float alpha, float eps,
                    float momentum, float weight_decay, float grad_scale, void* stream);

/* The same updates with the learning rate and the step count read from device memory, so a captured hipGraph of the training
 * step (chexpert.py:159-165) can be replayed while both change: hyper = float[8] {lr, steps_done, sched_kind (0 none,
 * 1 ExponentialLR chexpert.py:500, 2 MultiStepLR :480), gamma, lr_warmup_steps (:165), milestone0, milestone1, base_lr}.
 * cx_optim_tick = "step += 1; if step >= lr_warmup_steps: scheduler.step()" (:165).                                            */
int cx_adam_step_dev(float* p, const float* g, float* m, float* v, size_t n, const float* hyper, float beta1, float beta2,
                     float eps, float weight_decay, float grad_scale, void* stream);
int cx_sgd_nesterov_step_dev(float* p, const float* g, float* buf, size_t n, const float* hyper, float momentum,
                             float weight_decay, float grad_scale, void* stream);
int cx_rmsprop_step_dev(float* p, const float* g, float* sq, float* buf, size_t n, const float* hyper, float alpha, float eps,
                        float momentum, float weight_decay, float grad_scale, void* stream);
int cx_optim_tick(float* hyper, void* stream);

/* Global-norm gradient clipping, non-finite skip and weight EMA inside the optimiser launch (optim.hip).
 * cx_grad_norm: two launches, no atomics.  Launch 1: cx_grad_norm_partials(n) workgroups (a function of n alone), each sums
 * (grad_scale * g)^2 over a fixed contiguous range (16-byte loads, n % 4 scalar tail) and plain-stores one partial to `workspace`
 * (>= cx_grad_norm_partials(n) floats).  Launch 2: one workgroup sums the partials in a fixed order and writes
 * clip = float[4] {norm, coef, nonfinite, skipped}: norm = sqrt(sum); coef = min(1, max_norm / (norm + 1e-6))
 * (torch.nn.utils.clip_grad_norm_), 1 when max_norm <= 0; nonfinite = 1 when the sum is inf or NaN; skipped += 1 when nonfinite and
 * skip_nonfinite (the caller zeroes clip once).  g 16-byte aligned (CX_EALIGN), any n; n == 0: norm 0, coef 1.                       */
int cx_grad_norm_partials(size_t n);
int cx_grad_norm(const float* g, size_t n, float grad_scale, float max_norm, int skip_nonfinite, float* workspace,
                 size_t workspace_floats, float* clip, void* stream);
/* The six steps above with: the gradient that enters the update = grad_scale * clip[1] * g (clip null: grad_scale * g); nothing
 * written (p, states, ema keep their bits) when skip_nonfinite and clip[2] != 0; ema (null: none) = d * ema + (1 - d) * p_new in the
 * same pass, d = ema_decay or, with ema_warmup, min(ema_decay, (1 + t) / (10 + t)), t = the 1-based number of this step (`step`,
 * or hyper[1] + 1).  clip and ema null: the call is forwarded to the plain entry point (same kernel, same bits).  cx_optim_tick is unchanged: a skipped step is still a
 * minibatch for the schedule and for Adam's bias correction.                                                                      */
int cx_adam_step_ex(float* p, const float* g, float* m, float* v, size_t n, float lr, float beta1, float beta2, float eps,
                    float weight_decay, int step, float grad_scale, const float* clip, float* ema, float ema_decay, int ema_warmup,
                    int skip_nonfinite, void* stream);
int cx_sgd_nesterov_step_ex(float* p, const float* g, float* buf, size_t n, float lr, float momentum, float weight_decay,
                            int first_step, int step, float grad_scale, const float* clip, float* ema, float ema_decay,
                            int ema_warmup, int skip_nonfinite, void* stream);
int cx_rmsprop_step_ex(float* p, const float* g, float* sq, float* buf, size_t n, float lr, float alpha, float eps, float momentum,
                       float weight_decay, int step, float grad_scale, const float* clip, float* ema, float ema_decay,
                       int ema_warmup, int skip_nonfinite, void* stream);
int cx_adam_step_dev_ex(float* p, const float* g, float* m, float* v, size_t n, const float* hyper, float beta1, float beta2,
                        float eps, float weight_decay, float grad_scale, const float* clip, float* ema, float ema_decay,
                        int ema_warmup, int skip_nonfinite, void* stream);
int cx_sgd_nesterov_step_dev_ex(float* p, const float* g, float* buf, size_t n, const float* hyper, float momentum,
                                float weight_decay, float grad_scale, const float* clip, float* ema, float ema_decay, int ema_warmup,
                                int skip_nonfinite, void* stream);
int cx_rmsprop_step_dev_ex(float* p, const float* g, float* sq, float* buf, size_t n, const float* hyper, float alpha, float eps,
                           float momentum, float weight_decay, float grad_scale, const float* clip, float* ema, float ema_decay,
                           int ema_warmup, int skip_nonfinite, void* stream);

/* Parameter groups for the fused optimisers (optim.hip): per-group learning-rate multiplier, weight decay (L2 or decoupled),
 * frozen groups and a per-group step count.  The flat buffers hold every parameter tensor at a multiple of 4 floats, zero-padded
 * to a multiple of 4 (n % 4 == 0), and are walked through two tables in device memory:
 *   items  = uint32[n_items][4] {start4, len4, group, tensor}: a run of len4 16-byte units from unit start4, all of one tensor,
 *            len4 <= cx_optim_item_vec4() (a constant); items in buffer order, covering every unit exactly once.  The kernels
 *            trust the table: start4 + len4 <= n / 4 and group < n_groups are the caller's to guarantee.
 *   groups = float[n_groups][4] {lr_mult, weight_decay, frozen, t0}, 1 <= n_groups <= 256.  Read by the kernels at every launch,
 *            so a captured hipGraph sees a row rewritten between two replays.
 * cx_grad_norm_items: two launches, no atomics.  Launch 1 plain-stores one partial sum of (grad_scale * g)^2 per item to
 * `partials` (n_items floats).  Launch 2, one workgroup: group_sq[k] = the partials of group k added one by one in item order,
 * group_norm[k] = sqrt(group_sq[k]) (frozen groups too); then the group_sq of the groups with frozen == 0 added in group order give
 * clip = {norm, coef, nonfinite, skipped} exactly as cx_grad_norm defines them.  A non-finite value in a frozen group shows in that
 * group's group_norm only.
 * cx_*_step_items: hyper null -> `lr` and the 1-based `step` are the host's; else lr = hyper[0], step = hyper[1] + 1 (the arguments
 * are ignored).  Per item of group k: frozen != 0 -> skipped, no byte of p, the states or ema written; lr_k = lr * lr_mult;
 * decoupled == 0: g += weight_decay_k * p (the L2 form of the plain steps); decoupled != 0: p <- p * (1 - lr_k * weight_decay_k)
 * first, then the rule without decay (torch.optim.AdamW's order).  Adam's bias corrections use step - t0_k, the group's own step
 * count; SGD and RMSprop do not read t0.  The SGD momentum buffer must start as zeros (momentum * 0 + g is the first step's
 * buffer).  clip / ema / ema_decay / ema_warmup / skip_nonfinite as in the *_ex steps (the EMA's warm-up counts `step`, not
 * step - t0).  Padding floats stay 0 under every rule.
 * CX_EINVAL before any launch: a null pointer (clip and ema may be null; buf of RMSprop when momentum == 0), n_groups outside
 * [1, 256], n % 4 != 0, n_items == 0 with n > 0, step < 1 without hyper, ema_decay outside [0, 1].  CX_EALIGN: a buffer or table
 * that is not 16-byte aligned.                                                                                                     */
int cx_optim_item_vec4(void);
int cx_grad_norm_items(const float* g, size_t n, const uint32_t* items, int n_items, const float* groups, int n_groups,
                       float grad_scale, float max_norm, int skip_nonfinite, float* partials, float* group_sq, float* group_norm,
                       float* clip, void* stream);
int cx_adam_step_items(float* p, const float* g, float* m, float* v, size_t n, const uint32_t* items, int n_items, const float* groups,
                       int n_groups, int decoupled, const float* hyper, float lr, int step, float beta1, float beta2, float eps,
                       float grad_scale, const float* clip, float* ema, float ema_decay, int ema_warmup, int skip_nonfinite,
                       void* stream);
int cx_sgd_nesterov_step_items(float* p, const float* g, float* buf, size_t n, const uint32_t* items, int n_items, const float* groups,
                               int n_groups, int decoupled, const float* hyper, float lr, int step, float momentum, float grad_scale,
                               const float* clip, float* ema, float ema_decay, int ema_warmup, int skip_nonfinite, void* stream);
int cx_rmsprop_step_items(float* p, const float* g, float* sq, float* buf, size_t n, const uint32_t* items, int n_items,
                          const float* groups, int n_groups, int decoupled, const float* hyper, float lr, int step, float alpha, float eps,
                          float momentum, float grad_scale, const float* clip, float* ema, float ema_decay, int ema_warmup,
                          int skip_nonfinite, void* stream);

/* Layer-wise trust ratios over the same tables: LAMB (You et al., ICLR 2020) on Adam's moments, LARS (You, Gitman, Ginsburg 2017) on
 * SGD with Nesterov momentum.  Each call enqueues three launches on `stream`, with no atomics and nothing read on the host.  With
 * g = grad_scale * clip[1] * grad, lr_k = lr * lr_mult_k and t_k = step - t0_k of the tensor's group k:
 *   LAMB  m = b1 m + (1 - b1) g;  v = b2 v + (1 - b2) g^2;  u = (m / (1 - b1^t_k)) / (sqrt(v / (1 - b2^t_k)) + eps) + wd_k p;
 *         r = |p| / |u|;  p -= lr_k r u
 *   LARS  r = coef |p| / (|g| + wd_k |p| + eps);  g' = r (g + wd_k p);  buf = momentum buf + g';  p -= lr_k (g' + momentum buf)
 * r is 1 unless the tensor is adapted (wd_k != 0, or always_adapt != 0) and both norms are > 0; trust_clip != 0: r = min(r, 1).
 * Launch 1, one workgroup per item: part_w[item] = sum p^2, part_u[item] = sum u^2 (LARS: sum g^2); LAMB also writes m, v and the
 * update u (n floats of scratch: the apply reads the stored u, so the norm belongs to the u that is applied).  Launch 2, one
 * workgroup: the partials of tensor k's items tensor_items[k] .. tensor_items[k + 1] - 1 (uint32[n_tensors + 1], the first item of
 * every tensor, then n_items) added one by one in item order give trust[k] = float[4] {r, |p|, |u| (LARS: |g|), adapted}, for the
 * tensors of frozen groups too (r = 1).  Launch 3: the update, with ema as in the *_step_items.  Every summation tree is a function of
 * the item table alone.  An item of a frozen group gets partials of 0 and no other byte written; on a step that skip_nonfinite drops,
 * nothing at all is written.  Padding floats stay 0.
 * CX_EINVAL / CX_EALIGN before any launch as for cx_*_step_items, and CX_EINVAL for decoupled != 0, n_tensors < 1, a null
 * tensor_items / trust / partial buffer / u, eps <= 0 (LAMB), coef <= 0 or eps < 0 (LARS).                                          */
int cx_lamb_step_items(float* p, const float* g, float* m, float* v, size_t n, const uint32_t* items, int n_items, const float* groups,
                       int n_groups, int decoupled, const float* hyper, float lr, int step, float beta1, float beta2, float eps,
                       float grad_scale, const float* clip, float* ema, float ema_decay, int ema_warmup, int skip_nonfinite,
                       const uint32_t* tensor_items, int n_tensors, float* part_w, float* part_u, float* trust, float* u,
                       int trust_clip, int always_adapt, void* stream);
int cx_lars_step_items(float* p, const float* g, float* buf, size_t n, const uint32_t* items, int n_items, const float* groups,
                       int n_groups, int decoupled, const float* hyper, float lr, int step, float momentum, float grad_scale,
                       const float* clip, float* ema, float ema_decay, int ema_warmup, int skip_nonfinite,
                       const uint32_t* tensor_items, int n_tensors, float* part_w, float* part_u, float* trust, float coef, float eps,
                       int trust_clip, int always_adapt, void* stream);

/* Sharpness-aware minimisation (SAM: Foret et al., ICLR 2021; ASAM: Kwon et al., ICML 2021) over the same item table and group rows
 * (optim.hip): the ascent step p <- p + rho * s^2 g / |s g| with g = grad_scale * grad and s = 1 (adaptive == 0) or s = |p|
 * elementwise (adaptive != 0), taken over the groups with frozen == 0.
 * cx_sam_norm_items: two launches, no atomics.  Launch 1 plain-stores one partial sum of (g s)^2 per item to `partials` (n_items
 * floats; 0 for an item of a frozen group, which is not read).  Launch 2, one workgroup, adds the partials in item order in a tree
 * that is a function of n_items alone and writes sam = float[4] {norm, scale = rho / (norm + eps), nonfinite, 0}; rho_eps =
 * float[2] {rho, eps} in DEVICE memory, so a captured hipGraph follows a rho schedule.  norm == 0 gives scale = rho / eps (eps > 0
 * is the caller's to guarantee) and with it a perturbation of 0; an inf or NaN sum sets nonfinite = 1.  p may be null when
 * adaptive == 0.
 * cx_sam_perturb_items: per element of every item of an unfrozen group backup = p, then p = p + scale * s^2 * g (scale = sam[1]).
 * cx_sam_restore_items: p = backup on the same elements (a copy).  Both write nothing at all when sam[2] != 0, and no byte of p or
 * backup of a frozen group.  Padding floats (p = g = 0) stay 0.
 * The kernels skip an item with start4 + len4 > n / 4 or group >= n_groups.  items_host (may be null): a host copy of the table,
 * checked for exactly that before any launch.
 * CX_EINVAL before any launch: a null pointer (items_host aside), n_groups outside [1, 256], n % 4 != 0, n_items == 0 with n > 0,
 * an item of items_host past the buffer or with a group >= n_groups.  CX_EALIGN: a buffer or table that is not 16-byte aligned.    */
int cx_sam_norm_items(const float* p, const float* g, size_t n, const uint32_t* items, const uint32_t* items_host, int n_items,
                      const float* groups, int n_groups, const float* rho_eps, float grad_scale, int adaptive, float* partials,
                      float* sam, void* stream);
int cx_sam_perturb_items(float* p, const float* g, float* backup, size_t n, const uint32_t* items, const uint32_t* items_host,
                         int n_items, const float* groups, int n_groups, const float* sam, float grad_scale, int adaptive,
                         void* stream);
int cx_sam_restore_items(float* p, const float* backup, size_t n, const uint32_t* items, const uint32_t* items_host, int n_items,
                         const float* groups, int n_groups, const float* sam, void* stream);

/* ---- attention-augmented convolution (AAConv2d, models/attn_aug_conv.py:19-100) --------------------
 * qkv: bf16 (B, H*W, ldq) output of in_proj_qkv (channels [q dk | k dk | v dv], head-major), ldq % 4 == 0 and
 * ldq >= 2 dk + dv (the kernels read q and k in chunks of four elements: 8 bytes of bf16, 16 bytes of fp32); CX_ESHAPE otherwise,
 * before any launch.  cx_last_kernel() names the family and instance that ran: aa_row_fwd<DVH,W> / aa_row_bwd<DVH,W>,
 * aa_fwd<bf16|f32,DVH> / aa_bwd<..> / aa_weights<bf16|f32>, aa_heads_fwd<bf16|f32,KC,VC> / aa_heads_bwd<..> / aa_heads_weights<..,KC>.
 * Head widths dkh = dk/nh and dvh = dv/nh of 1 .. 64 with dv <= 104: dkh = 20 with dvh <= 13 runs the row / generic kernels
 * of aaconv.hip + aaconv_row.hip, every other width the runtime-width kernels of aaconv_heads.hip; CX_ESHAPE beyond that, or
 * when a map's relative tables and tiles exceed the LDS of a workgroup (any H, W <= 40 fits).
 * o: fp32 (B, H*W, dv) attention output BEFORE out_proj; lse: fp32 (B*nh, H*W) log-sum-exp of the logits.
 * Logits include the relative terms of rel_to_abs / relative_logits_1d (:43-63) in closed form; the
 * (B,nh,HW,HW) tensors of the reference are never materialised.  The _f32 entry points take fp32 qkv (fp32 storage mode). */
int cx_aa_attention_fwd(const void* qkv, const float* key_rel_h, const float* key_rel_w, float* o, float* lse, int B, int H, int W,
                        int nh, int dk, int dv, int ldq, void* stream);
/* weights: fp32 (B, nh, H*W, H*W) = softmax(logits) rebuilt from the saved lse -- the tensor the reference leaves in
 * AAConv2d.weights after a forward (:87) and vis_attn reads (chexpert.py:383); visualisation only                   */
int cx_aa_attention_weights(const void* qkv, const float* key_rel_h, const float* key_rel_w, const float* lse, float* weights, int B,
                            int H, int W, int nh, int dk, int dv, int ldq, void* stream);
/* dqkv: fp32 (B, H*W, 2dk+dv) fully written; d_rel_h / d_rel_w (dkh, 2H-1 / 2W-1) ACCUMULATED.  With a workspace of
 * ceil(HW/128)*B*nh * dkh*(2H-1 + 2W-1) floats every query-side workgroup stores its partial tables and they are added in
 * workgroup order (bit-reproducible); scratch == NULL or too small: fp32 atomics                                          */
int cx_aa_attention_bwd(const void* qkv, const float* key_rel_h, const float* key_rel_w, const float* o, const float* d_o,
                        const float* lse, float* dqkv, float* d_rel_h, float* d_rel_w, int B, int H, int W, int nh, int dk, int dv,
                        int ldq, float* scratch, int64_t scratch_floats, void* stream);
/* out_proj (dv x dv, :92) forward into a bf16 channel slice (+stats) and its backward (dY = g*ga+gx*gb+gc).
 * stat_rows > 0: deterministic statistic rows as CxConv.stat_det (row r at stat_sum[r*stat_rstride + c], at most stat_rows rows,
 * cx_last_stat_rows() tells how many); 0: one fp32 atomic per channel and workgroup.  The backward's dW partial tiles go
 * through the CxWgrad.scratch protocol (and the deferred sums) when a workspace is given.                                  */
int cx_aa_outproj_fwd(const float* o, const float* w, void* y, int ldy, float* stat_sum, float* stat_sq, size_t npix, int dv,
                      int stat_rows, int stat_rstride, void* stream);
int cx_aa_outproj_bwd(const void* g, int ldg, const void* gx, int ldgx, const float* ga, const float* gb, const float* gc,
                      const float* o, const float* w, float* d_o, float* dw, size_t npix, int dv, float* scratch, int64_t scratch_floats,
                      void* stream);
/* dst[c] (+)= rows[0*rstride + c] + rows[1*rstride + c] + ... in row order (accumulate != 0: added to dst, else assigned)      */
int cx_rows_reduce(float* dst, const float* rows, int n_rows, int C, int rstride, int accumulate, void* stream);
/* InstanceNorm2d + ReLU ahead of the AAConv2d (:438-439): per-(b,c) sums, per-(b,c) affine+ReLU, and the backward.  The sums are
 * plain stores from one owner per (b, c) (no atomics, no zero-fill needed, bit-reproducible)                                 */
int cx_stats_bc(const void* x, float* sum, float* sq, int B, int HW, int C, int ldx, void* stream);
int cx_affine_relu_bc(const void* x, const float* sc, const float* sh, void* y, int B, int HW, int C, int ldx, void* stream);
int cx_in_relu_bwd(const void* da, const void* x, const float* sc, const float* sh, float* S1, float* S2, void* gout, int B, int HW,
                   int C, int ldx, int ldg, void* stream);
/* fp32 storage-mode twins of the AAConv2d entry points (qkv / activations fp32; the per-query VALU kernels, no MFMA row kernels) */
int cx_aa_attention_fwd_f32(const void* qkv, const float* rel_h, const float* rel_w, float* o, float* lse, int B, int H, int W, int nh,
                        int dk, int dv, int ldq, void* stream);
int cx_aa_attention_weights_f32(const void* qkv, const float* rel_h, const float* rel_w, const float* lse, float* weights, int B, int H,
                            int W, int nh, int dk, int dv, int ldq, void* stream);
int cx_aa_attention_bwd_f32(const void* qkv, const float* rel_h, const float* rel_w, const float* o, const float* d_o, const float* lse,
                        float* dqkv, float* d_rel_h, float* d_rel_w, int B, int H, int W, int nh, int dk, int dv, int ldq,
                        float* scratch, int64_t scratch_floats, void* stream);
int cx_stats_bc_f32(const void* x, float* sum, float* sq, int B, int HW, int C, int ldx, void* stream);
int cx_affine_relu_bc_f32(const void* x, const float* sc, const float* sh, void* y, int B, int HW, int C, int ldx, void* stream);
int cx_aa_outproj_fwd_f32(const float* o, const float* w, void* y, int ldy, float* stat_sum, float* stat_sq, size_t npix, int dv,
                      int stat_rows, int stat_rstride, void* stream);
int cx_aa_outproj_bwd_f32(const void* g, int ldg, const void* gx, int ldgx, const float* ga, const float* gb, const float* gc,
                      const float* o, const float* w, float* d_o, float* dw, size_t npix, int dv, float* scratch, int64_t scratch_floats,
                      void* stream);
int cx_in_relu_bwd_f32(const void* da, const void* x, const float* sc, const float* sh, float* S1, float* S2, void* gout, int B, int HW,
                   int C, int ldx, int ldg, void* stream);
int cx_f32_to_bf16(const float* x, void* y, size_t n, void* stream);

/* ---- EfficientNet blocks (models/efficientnet.py:27-131): depthwise conv, squeeze-excitation, Swish glue ----------
 * depthwise k x k conv on (B,H,W,C) bf16, weights fp32 (C,1,k,k); the preceding BatchNorm+Swish is applied on load
 * when sc/sh are given (sc == NULL: raw input).  Output / statistics as cx_conv_gemm.                          */
int cx_nchw3_to_nhwc8(const float* x, void* y, int B, int H, int W, void* stream);
/* uint8 grey image (npix pixels) -> whitened, channel-expanded (.., 8) bf16 for the EfficientNet stem (chexpert.py:70-72 on the GPU) */
int cx_u8_to_nhwc8(const uint8_t* x, void* y, size_t npix, float mean, float std, void* stream);
/* stat_rows (cx_dwconv_fwd / cx_dwconv_dgrad / cx_bn_lin_bwd_stats / cx_se_act_bwd): > 0 = DETERMINISTIC statistic rows with the
 * CxConv.stat_det convention (row r at sum[r * C + c], at most stat_rows rows, cx_last_stat_rows() tells how many; the consumer
 * cx_bn_coef / cx_bn_bwd_coef sums them in row order), 0 = fp32 atomics into [C] vectors the caller zeroed.
 * cx_dwconv_wgrad: scratch / scratch_floats = the CxWgrad.scratch slab protocol (reproducible sums, deferrable), NULL = atomics.
 * cx_gap_affine_act / cx_se_bwd_reduce: scratch of splits * B * C floats (splits <= 1024 / B) = every pixel split plain-stores its
 * partial per-(image, channel) sum and a second launch adds the rows in order; cx_se_bwd: scratch = slab workspace, one slab per
 * group of images for dW1 / db1 / dW2 / db2.  NULL: fp32 atomics.                                                             */
int cx_dwconv_fwd(const void* x, const float* w, const float* sc, const float* sh, void* y, float* stat_sum, float* stat_sq, int B, int H,
                  int W, int C, int k, int stride, int pad, int stat_rows, void* stream);
/* dY = g*ga + g2*gb + gc;  dz = (sum_t dY w) * swish'(x*sc+sh), S1 += dz, S2 += dz*(x-mean)*rstd (sc==NULL: dz = sum) */
int cx_dwconv_dgrad(const void* g, const void* g2, const float* ga, const float* gb, const float* gc, const float* w, const void* x,
                    const float* sc, const float* sh, const float* mean, const float* rstd, void* dz, float* S1, float* S2, int B, int H,
                    int W, int C, int k, int stride, int pad, int accumulate, int stat_rows, void* stream);
int cx_dwconv_wgrad(const void* g, const void* g2, const float* ga, const float* gb, const float* gc, const void* x, const float* sc,
                    const float* sh, float* dw, int B, int H, int W, int C, int k, int stride, int pad, float* scratch,
                    int64_t scratch_floats, void* stream);
/* pooled[b][c] = mean_hw act(x*sc+sh) (act 0 none / 1 relu / 2 swish): SELayer pool (:69), head pool (:162)      */
int cx_gap_affine_act(const void* x, const float* sc, const float* sh, float* pooled, int B, int HW, int C, int act, float* scratch,
                      int64_t scratch_floats, void* stream);
/* SELayer FCs (:70-73): h1 = W1 pooled + b1, s = sigmoid(W2 swish(h1) + b2); and their backward                */
int cx_se_fwd(const float* pooled, const float* w1, const float* b1, const float* w2, const float* b2, float* h1, float* s, int B, int C,
              int R, void* stream);
/* ABI 10.  SELayer squeeze + excitation (:69-73) as TWO launches: cx_gap_affine_act's per-split partial means are added by the
 * excitation kernel itself (in row order: reproducible), which also leaves pooled[b][c] for the backward pass -- the reduce launch
 * between the two is gone (33 launches per EfficientNet-B4 step).  scratch as for cx_gap_affine_act; NULL / too small: the
 * three-launch form with atomics.                                                                                        */
int cx_gap_se_fwd(const void* x, const float* sc, const float* sh, float* pooled, const float* w1, const float* b1, const float* w2,
                  const float* b2, float* h1, float* s, int B, int HW, int C, int R, int act, float* scratch, int64_t scratch_floats,
                  void* stream);
int cx_gap_se_fwd_f32(const void* x, const float* sc, const float* sh, float* pooled, const float* w1, const float* b1, const float* w2,
                      const float* b2, float* h1, float* s, int B, int HW, int C, int R, int act, float* scratch, int64_t scratch_floats,
                      void* stream);
int cx_se_bwd(const float* ds, const float* s, const float* h1, const float* pooled, const float* w1, const float* w2, float* dw1,
              float* db1, float* dw2, float* db2, float* dpooled, int B, int C, int R, float* scratch, int64_t scratch_floats,
              void* stream);
/* ABI 10.  cx_se_bwd_reduce + cx_se_bwd without the reduce launch between them: the split rows of ds[b][c] = sum_hw du * swish(x*sc+sh)
 * (rows_scratch: splits * B * C floats, as for cx_se_bwd_reduce) are added, in row order, by the first FC pass.  `ds` (B x C) is written
 * only when that form cannot run (no row / slab workspace: the four-launch sequence with what workspaces there are).            */
int cx_se_bwd_fused(const void* du, const void* x, const float* sc, const float* sh, float* ds, const float* s, const float* h1,
                    const float* pooled, const float* w1, const float* w2, float* dw1, float* db1, float* dw2, float* db2, float* dpooled,
                    int B, int HW, int C, int R, float* rows_scratch, int64_t rows_floats, float* scratch, int64_t scratch_floats,
                    void* stream);
int cx_se_bwd_fused_f32(const void* du, const void* x, const float* sc, const float* sh, float* ds, const float* s, const float* h1,
                        const float* pooled, const float* w1, const float* w2, float* dw1, float* db1, float* dw2, float* db2, float* dpooled,
                        int B, int HW, int C, int R, float* rows_scratch, int64_t rows_floats, float* scratch, int64_t scratch_floats,
                        void* stream);
/* u = swish(x*sc+sh) * s[b][c] (s NULL: no SE scaling)                                                          */
int cx_scale_act_bc(const void* x, const float* sc, const float* sh, const float* s, void* u, int B, int HW, int C, void* stream);
int cx_se_bwd_reduce(const void* du, const void* x, const float* sc, const float* sh, float* ds, int B, int HW, int C, float* scratch,
                     int64_t scratch_floats, void* stream);
/* dz = (du*s[b][c] + dpooled[b][c]/HW) * swish'(x*sc+sh) + BN backward sums (du or dpooled may be NULL)          */
int cx_se_act_bwd(const void* du, const void* x, const float* sc, const float* sh, const float* mean, const float* rstd, const float* s,
                  const float* dpooled, void* dz, float* S1, float* S2, int B, int HW, int C, int stat_rows, void* stream);
int cx_bn_lin_bwd_stats(const void* g, const void* y, const float* mean, const float* rstd, float* S1, float* S2, size_t rows, int C,
                        int stat_rows, void* stream);
/* out = s*(a*pa + pc) + b*pb (b may be NULL): projection BatchNorm output, DropConnect, skip (:105-110).  sample_scale
 * (optional, one float per image, rows_per_sample rows each) is the DropConnect mask / keep probability (:44-51)     */
int cx_affine2_out(const void* a, const void* b, const float* pa, const float* pb, const float* pc, const float* sample_scale,
                   size_t rows_per_sample, void* out, size_t rows, int C, void* stream);
/* out[row][:] = sample_scale[row / rows_per_sample] * g[row][:]: gradient entering a DropConnect-ed branch            */
int cx_scale_rows(const void* g, const float* sample_scale, size_t rows_per_sample, void* out, size_t rows, int C, void* stream);
/* out[i] in {0, 1/keep_prob}: counter-based (splitmix64 of seed and index) Bernoulli mask for Dropout (:170) and DropConnect */
/* fp32 storage-mode twins of the EfficientNet entry points above (activations fp32; the generic kernels, no tiled fast paths) */
int cx_nchw3_to_nhwc8_f32(const float* x, void* y, int B, int H, int W, void* stream);
int cx_u8_to_nhwc8_f32(const uint8_t* x, void* y, size_t npix, float mean, float std, void* stream);
int cx_dwconv_fwd_f32(const void* x, const float* w, const float* sc, const float* sh, void* y, float* stat_sum, float* stat_sq, int B, int H,
                  int W, int C, int k, int stride, int pad, int stat_rows, void* stream);
int cx_dwconv_dgrad_f32(const void* g, const void* g2, const float* ga, const float* gb, const float* gc, const float* w, const void* x,
                    const float* sc, const float* sh, const float* mean, const float* rstd, void* dz, float* S1, float* S2, int B, int H,
                    int W, int C, int k, int stride, int pad, int accumulate, int stat_rows, void* stream);
int cx_dwconv_wgrad_f32(const void* g, const void* g2, const float* ga, const float* gb, const float* gc, const void* x, const float* sc,
                    const float* sh, float* dw, int B, int H, int W, int C, int k, int stride, int pad, float* scratch,
                    int64_t scratch_floats, void* stream);
int cx_gap_affine_act_f32(const void* x, const float* sc, const float* sh, float* pooled, int B, int HW, int C, int act, float* scratch,
                      int64_t scratch_floats, void* stream);
int cx_scale_act_bc_f32(const void* x, const float* sc, const float* sh, const float* s, void* u, int B, int HW, int C, void* stream);
int cx_bn_lin_bwd_stats_f32(const void* g, const void* y, const float* mean, const float* rstd, float* S1, float* S2, size_t rows, int C,
                        int stat_rows, void* stream);
int cx_se_bwd_reduce_f32(const void* du, const void* x, const float* sc, const float* sh, float* ds, int B, int HW, int C, float* scratch,
                     int64_t scratch_floats, void* stream);
int cx_se_act_bwd_f32(const void* du, const void* x, const float* sc, const float* sh, const float* mean, const float* rstd, const float* s,
                  const float* dpooled, void* dz, float* S1, float* S2, int B, int HW, int C, int stat_rows, void* stream);
int cx_affine2_out_f32(const void* a, const void* b, const float* pa, const float* pb, const float* pc, const float* sample_scale,
                   size_t rows_per_sample, void* out, size_t rows, int C, void* stream);
int cx_scale_rows_f32(const void* g, const float* sample_scale, size_t rows_per_sample, void* out, size_t rows, int C, void* stream);
int cx_dropout_mask(float* out, size_t n, float keep_prob, unsigned long long seed, void* stream);
/* ABI 7: the same mask with seed = base + step[0] * 1000003 assembled on the device, and the one-element counter bump that goes  */
/* with it -- a captured training step (hipGraph) then draws new Dropout / DropConnect masks at every replay                  */
int cx_dropout_mask_dev(float* out, size_t n, float keep_prob, unsigned long long base, const unsigned long long* step, void* stream);
int cx_counter_add(unsigned long long* counter, unsigned long long inc, void* stream);
int cx_mul_f32(const float* a, const float* b, float* out, size_t n, void* stream);
int cx_linear_fwd(const float* x, const float* w, const float* bias, float* y, int B, int C, int N, void* stream);

/* Grad-CAM as the reference code executes it (chexpert.py:260-303):
 * cam[b][p] = relu(sum_c w[c]*f(x*scale+shift)) with class-independent w[c] = mean_b pooled[b][c]*B/n_cls,
 * then per-image (t-min)/(max-min+1e-5) and bilinear upsampling with align_corners=True.
 * inner_relu = 1: f = relu (DenseNet: the hook on features.norm5 ends up holding the in-place ReLU'd tensor, :468);
 * inner_relu = 0: f = identity (ResNet layer4 output, already >= 0, :484; EfficientNet head[1] = BatchNorm output, :498) */
int cx_gradcam_map(const void* x, const float* scale, const float* shift, const float* w, float* cam, int B, int HW, int C,
                   int ldx, int inner_relu, void* stream);
int cx_cam_norm_upsample(const float* cam, float* out, int B, int h, int w, int H, int W, void* stream);

/* Class-specific maps at the tensor the network pools globally, A = act(x*scale + shift), for K classes in one pass over x:
 *   cam[b][k][p] = post((1/HW) * sum_f w[cls(b,k)][f] * A[b][p][f]),   post = relu when `relu` else the identity.
 * With the final Linear y = bias + W mean_p A this is Grad-CAM taken at A (alpha[c][f] = mean_p dy_c/dA[f][p] = W[c][f]/HW exactly, no
 * backward pass), and sum_p of the signed map (relu = 0) is y[b][c] - bias[c].
 *   x      (B, HW, C) NHWC, pixel pitch ldx >= C elements, bf16 (the _f32 twin: fp32); C % 8 == 0, ldx % 8 == 0, C <= 4096
 *   scale / shift   fp32 [C], or both NULL for the identity;   act: CX_CAM_ACT_*
 *   w      fp32 (n_classes, C), 16-byte aligned, row pitch ldw >= C, ldw % 4 == 0
 *   cls    NULL: class k of the map is row k of w and K == n_classes; else int32 (B, K) on the device, the row of w for map (b, k)
 *          (one class list repeated for every image, or one class per image with K = 1).  The library cannot range-check device
 *          memory: an entry outside [0, n_classes) is CLAMPED into the range inside the kernel (callers that hold the indices on the
 *          host check them there).
 *   cam    fp32 (B, K, HW)
 * x is read once whatever K is.  fp32 sums in a fixed order, one writer per element, no atomics: bit-reproducible, and a class gives
 * the same bits wherever it stands in cls.  CX_ESHAPE ("unsupported shape") before anything is launched for NULL x / w / cam, K < 1,
 * C % 8, C > 4096, a bad pitch, or cls == NULL with K != n_classes.  Additive entry points of ABI 10 (no struct changed).        */
enum { CX_CAM_ACT_NONE = 0, CX_CAM_ACT_RELU = 1, CX_CAM_ACT_SWISH = 2 };
int cx_class_cam(const void* x, const float* scale, const float* shift, const float* w, const int* cls, float* cam, int B, int HW, int C,
                 int ldx, int n_classes, int ldw, int K, int act, int relu, void* stream);
int cx_class_cam_f32(const void* x, const float* scale, const float* shift, const float* w, const int* cls, float* cam, int B, int HW,
                     int C, int ldx, int n_classes, int ldw, int K, int act, int relu, void* stream);

/* stat_rows (cx_bnrelu_maxpool_fwd / _bwd, cx_gap_relu_bn_bwd, cx_unpool2_mask, cx_relu_bwd_stats): 0 = the statistics are added to the single
 * copy S1 / S2 [C] with atomics; > 0 = deterministic rows: the launch uses at most stat_rows workgroups (cx_gap_relu_bn_bwd: one row
 * per image, B <= stat_rows) and plain-stores row r at S[r*C + c]; cx_last_stat_rows() gives the row count for the consumer.   */

/* Brightness / contrast jitter of the decoded grey images (B, HW) uint8 on the GPU: the "+ data aug" of the reference's
 * `_data_aug` README rows = ColorJitter(brightness=0.25, contrast=0.25) of explore_data.ipynb cell 6, torchvision tensor
 * semantics on uint8 (y = trunc(clamp(b*x)); y = trunc(clamp(c*x + (1-c)*mean(x)))), per-image factors and order (0 = brightness
 * first) drawn by the caller.  HW % 16 == 0, HW <= 150 KiB (the image is parked in LDS between the two passes).               */
int cx_u8_jitter(const uint8_t* x, uint8_t* y, int B, int HW, const float* brightness, const float* contrast, const int* order,
                 void* stream);
/* Random-affine warp of the decoded grey images x, y: (B, H, W) uint8, distinct buffers (the geometric half of augmentation; the
 * caller draws the matrices).  mat[b] is the INVERSE map of image b (output pixel -> source position), row-major 2x3, in pixel
 * units about the image centre.  fp32 throughout, for output pixel (i, j):
 *   xo = j + 0.5 - W/2, yo = i + 0.5 - H/2
 *   u  = m0*xo + m1*yo + m2 + W/2 - 0.5,  v = m3*xo + m4*yo + m5 + H/2 - 0.5
 *   u0 = floor(u), v0 = floor(v), fu = u - u0, fv = v - v0;  p(r, c) = x[b][r][c] inside the image, else `fill` (0..255)
 *   top = p(v0,u0)*(1-fu) + p(v0,u0+1)*fu, bot likewise on row v0+1;  y[b][i][j] = uint8(floor(top*(1-fv) + bot*fv + 0.5))
 * The identity (1,0,0, 0,1,0) returns x bit for bit.  One writer per output byte, no atomics: bit-reproducible.
 * W % 4 == 0, H and W <= 1024, else CX_ESHAPE; y and mat 4-byte aligned.  Additive entry point of ABI 10 (no struct changed).   */
int cx_u8_affine(const uint8_t* x, uint8_t* y, int B, int H, int W, const float* mat /* device, [B][6] */, int fill, void* stream);
/* Sample mixing of the decoded grey images x, y: (B, H, W) uint8, distinct buffers (mix.hip): Mixup, CutMix and random erasing
 * through one primitive; the caller draws the plan (chexpert_amd/augment.py: mix_plan, erase_plan).  Integer arithmetic throughout.
 * Per row b: p = perm[b] clamped to [-1, B-1], q = lam_q[b] clamped to [0, 65536], the box (y0 y1 x0 x1) clamped to the image: rows
 * [y0, y1), columns [x0, x1).  For pixel (i, j) with a = x[b][i][j]:
 *   outside the box   y[b][i][j] = a
 *   inside the box    o = (p < 0) ? fill : x[p][i][j];   y[b][i][j] = (q*a + (65536 - q)*o + 32768) >> 16
 * i.e. round-half-up of lambda*a + (1 - lambda)*o with lambda = q / 65536 (the sum is below 2^24: exact).  Mixup: box = the whole
 * image, any q.  CutMix: a partial box, q = 0.  Erasing: p = -1, q = 0.  Because of the clamps no load leaves the batch whatever
 * the parameter arrays hold; a row (or band of rows) the box does not touch is copied without reading the partner.  One writer per
 * output byte, no atomics: bit-reproducible.  x == y is CX_EINVAL (a partner row may be read after it was written), as are a null
 * pointer, B, H or W <= 0 and fill outside 0..255.  W % 4 == 0, H and W <= 1024, else CX_ESHAPE; x, y, perm, lam_q and box 4-byte
 * aligned, else CX_EALIGN (16 bytes per lane where W % 16 == 0 and x, y are 16-byte aligned).  Additive entry point of ABI 10.   */
int cx_u8_mix(const uint8_t* x, uint8_t* y, int B, int H, int W, const int* perm /* device, [B] */, const int* lam_q /* device, [B] */,
              const int* box /* device, [B][4]: y0 y1 x0 x1 */, int fill, void* stream);
/* The targets that go with cx_u8_mix: t, out (B, n) fp32, distinct buffers.  Every product and sum is rounded to fp32 on its own
 * (nothing is contracted into a fused multiply-add).  p = perm[b] clamped to [-1, B-1], w_q = tw_q[b] clamped to [0, 65536],
 * w = w_q / 65536 (w and 1 - w are exact in fp32):
 *   p < 0 or w_q == 65536            out[b][c] = t[b][c]
 *   else t[b][c] < 0 or t[p][c] < 0  out[b][c] = -1      (a label the loss ignores stays ignored)
 *   else                             out[b][c] = w * t[b][c] + (1 - w) * t[p][c]
 * CX_EINVAL: a null pointer, out == t, B or n <= 0.  CX_EALIGN: a pointer that is not 4-byte aligned.  Additive entry point of ABI 10. */
int cx_target_mix(const float* t, float* out, int B, int n, const int* perm /* device, [B] */, const int* tw_q /* device, [B] */,
                  void* stream);
/* Contrast-limited adaptive histogram equalisation (CLAHE) of the decoded grey images x: (B, H, W) uint8, in two stages (clahe.hip).
 * The structure is OpenCV's createCLAHE (per-tile clipped histogram -> table, bilinear blend of the four surrounding tables), but
 * NOT bit-equal to it: everything here is integer arithmetic, and tables sit at tile centres with pixel centres at half-integers.
 * Grid (GY, GX), each 1..16, tile th = H / GY by tw = W / GX, area = th * tw.
 * cx_u8_clahe_lut writes lut: (B, GY, GX, 256) uint8.  clip_count L in [0, area] is computed by the caller
 * (L = 0 if c == 0 else min(area, max(1, floor(c * area / 256))) for a clip limit c; 0 = no clipping).  Table of tile (b, gy, gx):
 *   hist[v] = number of pixels of the tile with value v
 *   L > 0:  excess = sum max(hist[v] - L, 0);  hist[v] = min(hist[v], L);  q, r = divmod(excess, 256);  hist[v] += q for every v;
 *           r > 0: step = max(1, 256 / r), and hist[v] += 1 for v = 0, step, 2 step, ... < 256 while r-- > 0
 *   cdf[v] = hist[0] + ... + hist[v];   lut[v] = (cdf[v] * 255 + area / 2) / area
 * cx_u8_clahe_apply writes y (a buffer other than x) from x and the tables.  For pixel (i, j) with value v = x[b][i][j]:
 *   ay = 2 i + 1 - th;  gy0 = floor(ay / (2 th)) (-1 in the top half tile);  wy = ay - gy0 * 2 th;  gy1 = gy0 + 1; both clamped to
 *   [0, GY - 1];  ax, gx0, wx, gx1 likewise with j, tw, GX
 *   num = (2 th - wy) * ((2 tw - wx) * lut[gy0][gx0][v] + wx * lut[gy0][gx1][v])
 *       +       wy    * ((2 tw - wx) * lut[gy1][gx0][v] + wx * lut[gy1][gx1][v])
 *   y[b][i][j] = (num + 2 th tw) / (4 th tw)                                  (num < 2^31 at the size limits)
 * GY = GX = 1 with L = 0 is plain global histogram equalisation.  Integer LDS adds inside a workgroup, nothing added in device
 * memory, one writer per output byte: bit-reproducible.
 * CX_ESHAPE: H % GY, W % GX, W % 4, H or W > 1024, a grid value outside 1..16.  CX_EINVAL: a null pointer, B <= 0, x == y,
 * clip_count outside [0, area].  CX_EALIGN: lut or y not 4-byte aligned (x may have any alignment).  Additive entry points of ABI 10. */
int cx_u8_clahe_lut(const uint8_t* x, uint8_t* lut, int B, int H, int W, int GY, int GX, int clip_count, void* stream);
int cx_u8_clahe_apply(const uint8_t* x, const uint8_t* lut, uint8_t* y, int B, int H, int W, int GY, int GX, void* stream);

/* Non-parametric bootstrap of the AUROC (bootstrap.hip; chexpert_amd/metrics.py: bootstrap_auc, and the numpy statement of both entry
 * points, bootstrap_counts_reference / bootstrap_scan_reference).  Integer arithmetic throughout, held to that statement bit for bit.
 * Rows are grouped into U resampling units (an image, a study, a patient); replicate b draws U units with replacement.  Draw j of
 * replicate b is the splitmix64 finaliser that effnet.hip uses for dropout, scaled by a multiply-shift:
 *   k = b * U + j (uint64);  z = seed + 0x9E3779B97F4A7C15 * (k + 1);  z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9;
 *   z = (z ^ (z >> 27)) * 0x94D049BB133111EB;  z = z ^ (z >> 31);  unit = ((z >> 32) * U) >> 32        (all mod 2^64)
 * (the multiply-shift favours some units by at most U / 2^32 in probability: 0.4 % of 1 / U at U = 2^24, 5e-6 of it at U = 20 000).
 * cx_boot_counts writes rows first .. first + n_rep - 1 of the count table into counts[0 .. n_rep) (row pitch ld >= U dwords):
 * counts[r][u] = number of the U draws of replicate first + r that hit unit u; a row sums to U and depends on (seed, first + r, U)
 * only, not on how the replicates are cut into calls.  U <= CX_BOOT_MAX_TILES * CX_BOOT_TILE: one workgroup per (replicate, tile of
 * CX_BOOT_TILE units) counts in LDS and stores the tile; above, the rows are zeroed and the hits added in device memory.  Integer adds
 * commute: the same bits on every run.
 * cx_boot_auc: for class c the caller lists the kept rows (target >= 0) twice, both times ascending in score: `hi` with the negatives
 * of a tie group before its positives, `lo` with the positives first.  An entry is the row's unit index with the label (1 = positive)
 * in bit 31.  order (device) holds, for class c, hi then lo, len[c] entries each, from order[offs[c]]; offs and len are HOST arrays of C
 * elements, checked here (len[c] may be 0 and differ by class).  With w = counts[r][unit], p = w at a positive entry, q = w at a
 * negative one and S(order) = sum_t p_t * (sum_{t' < t} q_t'):
 *   num2[r][c] = S(hi) + S(lo) = sum over positives i of w_i * (LT_i + LE_i),   LT_i / LE_i = the negative weight with a score < / <= that of i
 *   wpos[r][c] = sum p,  wneg[r][c] = sum q;   AUROC = num2 / (2 * wpos * wneg) (formed by the caller in float64: exact operands below
 *   2^53 for U <= 2^24, so the quotient is correctly rounded), the trapezoid area with ties counted half; wpos == 0 or wneg == 0: no AUROC.
 * Outputs are (n_rep, C) row-major, one writer per element.  Unit indices >= U are CLAMPED to U - 1 inside the kernel, never trusted.
 * Requirement: the sum of a count row is < 2^32 (cx_boot_counts: U).  One wave per (replicate, class); no LDS, no atomics.
 * CX_EINVAL: a null pointer, n_rep < 1, first < 0, C < 1, a negative len[c] or offs[c].  CX_ESHAPE: U outside [1, CX_BOOT_MAX_UNITS],
 * ld < U.  CX_EALIGN: counts / order / wpos / wneg not 4-byte, num2 not 8-byte aligned.  Additive entry points of ABI 10.          */
enum { CX_BOOT_TILE = 8192, CX_BOOT_MAX_TILES = 8, CX_BOOT_MAX_UNITS = 1 << 24 };
int cx_boot_counts(uint32_t* counts, int ld, int U, int first, int n_rep, uint64_t seed, void* stream);
int cx_boot_auc(const uint32_t* counts, int ld, int n_rep, const int32_t* order /* device */, const int64_t* offs /* host, [C] */,
                const int32_t* len /* host, [C] */, int C, uint64_t* num2, uint32_t* wpos, uint32_t* wneg, int U, void* stream);

/* The threshold sweep of the same bootstrap (bootstrap.hip; chexpert_amd/metrics.py: bootstrap_metrics, and the numpy statement
 * bootstrap_sweep_reference, held bit for bit): average precision and fixed operating points of every (replicate, class), in integers.
 * For class c the caller lists the kept rows ONCE, descending in score (metrics.bootstrap_sweep_plan): an entry is the row's unit index
 * with the label in bit 31 and bit 30 set on the LAST entry of its tie group (the order inside a group is immaterial).  order (device)
 * holds len[c] entries for class c from order[offs[c]]; offs and len are HOST arrays.  With w = counts[r][unit], tp_g / fp_g = the
 * positive / negative weight up to and including the marked entry g, tp_0 = fp_0 = 0, W+ / W- the totals:
 *   apnum[r][c] = sum over marked g of (tp_g - tp_{g-1}) * floor((tp_g << 32) / (tp_g + fp_g))      (uint64; a term with tp_g = tp_{g-1} is 0
 *                 and does not divide);  AP = apnum / (W+ * 2^32), the step sum of the precision-recall curve, below the exact value
 *                 by less than 2^-32 (every floor loses less than 2^-32 of its step's weight); W+ = 0: no AP
 *   wpos[r][c] = W+,  wneg[r][c] = W-
 *   pts[r][c][k], for operating point k with s = pt_ppm[k] millionths (1 .. 999 999), over the marked entries and the point (0, 0):
 *     pt_type[k] == CX_BOOT_SENS: max{tp_g : fp_g * 10^6 <= (10^6 - s) * W-}    sensitivity at specificity >= s = pts / W+
 *     pt_type[k] == CX_BOOT_SPEC: min{fp_g : tp_g * 10^6 >= s * W+}              specificity at sensitivity >= s = 1 - pts / W-
 *     (uint64 comparisons; both values need W+ > 0 and W- > 0; the set of the minimum is never empty: the last entry is marked, and
 *     with W+ = 0 the point (0, 0) qualifies).
 * pt_type / pt_ppm are HOST arrays of P <= CX_BOOT_MAX_POINTS entries; P = 0 (pt_type, pt_ppm, pts may then be NULL) computes apnum,
 * wpos and wneg only and reads the entries once instead of twice: W+ and W- of the conditions come from a first pass of the kernel over
 * the same entries, never from the caller.  Outputs are row-major (n_rep, C) and (n_rep, C, P), one writer per element.  Unit indices
 * >= U are CLAMPED to U - 1.  Requirement: the sum of a count row is < 2^32, which also keeps apnum below 2^64.  One wave per
 * (replicate, class); no LDS, no atomics.
 * CX_EINVAL: a null pointer, n_rep < 1, C < 1, a negative len[c] or offs[c], a pt_type that is neither constant, a pt_ppm outside
 * [1, 999 999].  CX_ESHAPE: P outside [0, CX_BOOT_MAX_POINTS], U outside [1, CX_BOOT_MAX_UNITS], ld < U.  CX_EALIGN: counts / order /
 * wpos / wneg / pts not 4-byte, apnum not 8-byte aligned.  Additive entry point of ABI 10.                                          */
enum { CX_BOOT_MAX_POINTS = 8, CX_BOOT_SENS = 0, CX_BOOT_SPEC = 1 };
int cx_boot_sweep(const uint32_t* counts, int ld, int n_rep, const int32_t* order /* device */, const int64_t* offs /* host, [C] */,
                  const int32_t* len /* host, [C] */, int C, const int32_t* pt_type /* host, [P] */, const int32_t* pt_ppm /* host, [P] */,
                  int P, uint64_t* apnum, uint32_t* wpos, uint32_t* wneg, uint32_t* pts, int U, void* stream);

/* Calibration of the predicted probabilities (calib.hip; chexpert_amd/calibration.py: fit_calibration, calibration_metrics, and the
 * numpy statements fit_calibration_reference / calibration_sums_reference).
 * cx_calib_fit fits, for every class c on its own, the map u = a_c z + b_c, p = sigmoid(u) (method CX_CALIB_PLATT; with
 * CX_CALIB_TEMPERATURE b_c = 0 and only a_c = 1 / T_c is fitted).  logits and targets are fp32 (C, N), class-major and contiguous; a
 * row with target < 0 is left out of its class, a row is positive iff target > 0.5.  The objective is the mean over the kept rows of
 * softplus(u) - t u in fp64, softplus(u) = max(u, 0) + log1p(exp(-|u|)), t the 0 / 1 label or, smooth != 0, Platt's targets
 * (N+ + 1) / (N+ + 2) and 1 / (N- + 2).  Damped Newton from the identity (a = 1, b = 0): gradient g and Hessian H of the mean loss,
 * step d = (H + 1e-12 I)^-1 g, the step halved while the loss rises (above L (1 + 1e-12), the rounding of the sum), at most 40
 * halvings; it stops when max |g| <= g_tol or after max_iter iterations.  out is fp64 (C, 8): a, b, nll_before, nll_after, gmax,
 * lambda_min, iterations, status.  status 0: converged; 1: iteration cap, parameters kept; 2: degenerate (no kept row, no positive or
 * no negative), the identity is returned; 3: flat -- the smallest eigenvalue of the last Hessian is below 1e-8 (separable or nearly
 * separable data), the identity is returned (smooth is the cure).  With status 2 / 3 nll_after is the loss of the identity; with
 * status 2 gmax and lambda_min are NaN, and both losses are NaN when no row is kept.  One 256-thread workgroup per class, fp64 sums
 * reduced in one fixed order, no atomics: the same bits on every run.  Every loop is bounded by max_iter.  N == 0 or C == 0 returns 0
 * without launching (out is left untouched).
 * CX_EINVAL before anything is launched: C < 0, N < 0, an unknown method, max_iter outside [1, CX_CALIB_MAX_ITER], g_tol negative or
 * NaN, a null pointer.  CX_EALIGN: logits / targets not 4-byte, out not 8-byte aligned.
 * cx_boot_calib: the bin sums of every (replicate, class) over a count table as cx_boot_sweep reads it (counts, ld, n_rep; the sum of a
 * count row is < 2^32).  order (device) holds len[c] entries for class c from order[offs[c]] (offs, len: HOST arrays): an entry is the
 * row's unit index in bits 0-23, its bin in bits 24-29 and its label in bit 31; conf (device, parallel to order) holds the row's
 * fixed-point confidence P = min(floor(p 2^32), 2^32 - 1).  With w = counts[r][unit], per bin b < M:
 *   wsum[r][c][b] = sum w,  wpos[r][c][b] = sum w over the positives (uint32),  csum[r][c][b] = sum w P (uint64)
 *   bnum[r][c]    = sum w umulhi(d, d),  d = 2^32 - 1 - P at a positive and P at a negative (uint64)
 * so that, formed by the caller in float64 with G_b = |wpos_b 2^32 - csum_b| and W = sum_b wsum_b: ECE = sum_b G_b / (W 2^32),
 * MCE = max over wsum_b > 0 of G_b / (wsum_b 2^32), Brier = bnum / (W 2^32) (below the exact value by less than 2^-31).
 * Outputs are row-major (n_rep, C, M) and (n_rep, C), one writer per element; a class with len[c] == 0 gives zeros.  Unit indices
 * >= U are CLAMPED to U - 1 and bins >= M to M - 1.  The entries may come in any order; listed ascending in bin (calibration_plan)
 * a lane adds to its wave's LDS accumulators once per bin instead of once per entry.  One wave per (replicate, class); integer LDS
 * atomics only (integer adds commute: the same bits on every run).
 * CX_EINVAL: a null pointer, n_rep < 1, C < 1, a negative len[c] or offs[c].  CX_ESHAPE: M outside [1, CX_CALIB_MAX_BINS], U outside
 * [1, CX_BOOT_MAX_UNITS], ld < U.  CX_EALIGN: counts / order / conf / wsum / wpos not 4-byte, csum / bnum not 8-byte aligned.
 * Additive entry points of ABI 10.                                                                                              */
enum { CX_CALIB_TEMPERATURE = 0, CX_CALIB_PLATT = 1, CX_CALIB_MAX_ITER = 1000, CX_CALIB_MAX_BINS = 64 };
int cx_calib_fit(const float* logits, const float* targets, int C, int N, int method, int smooth, double g_tol, int max_iter, double* out,
                 void* stream);
int cx_boot_calib(const uint32_t* counts, int ld, int n_rep, const int32_t* order /* device */, const uint32_t* conf /* device */,
                  const int64_t* offs /* host, [C] */, const int32_t* len /* host, [C] */, int C, int M, uint32_t* wsum, uint32_t* wpos,
                  uint64_t* csum, uint64_t* bnum, int U, void* stream);

/* DeLong / Obuchowski variance of the AUROC (delong.hip; chexpert_amd/metrics.py: delong_auc, delong_auc_diff, and the numpy statement
 * of both entry points, delong_place_reference / int_gram_reference, held bit for bit).  Integer arithmetic throughout.
 * cx_delong_place reads exactly what cx_boot_auc reads (the `hi` then the `lo` order of every class's kept rows, len[c] entries each
 * from order[offs[c]], an entry = unit index in bits 0-30 | label << 31; offs / len are HOST arrays) and writes the unit sums of the
 * doubled placements into z, an int64 table of 4 C rows of pitch ldz >= U (the padding is left untouched; the U columns are zeroed by
 * the entry point itself).  With M the positives of the class, ties counted half:
 *   a positive i:  X2_i = 2 #{neg j : s_j < s_i} + #{neg j : s_j = s_i} = (negatives in front of i in hi) + (those in front in lo)
 *   a negative j:  Y2_j = 2 #{pos i : s_i > s_j} + #{pos i : s_i = s_j} = (M - positives in front in lo) + (M - those in front in hi)
 *   z[4c][u] = sum of X2 over unit u's positives,  z[4c+1][u] = their number,  z[4c+2][u] = sum of Y2 over its negatives,
 *   z[4c+3][u] = their number;  sum_u z[4c] = sum_u z[4c+2] = the num2 of cx_boot_auc for a count row of ones
 * One 1024-thread workgroup per (class, order, chunk of CX_DELONG_WG_ENTRIES entries): a pass over the whole list that counts M and
 * the positives in front of the chunk, then the chunk, whose exclusive prefix count of positives (the negatives in front are the
 * position minus it) comes from wave ballots, an LDS scan of the wave totals and a running carry; every entry is added to its unit's
 * row with 64-bit integer atomics (integer adds commute: the same bits on every run).  No workgroup waits on another.  Unit indices
 * >= U are CLAMPED to U - 1; len[c] may be 0 and may differ by class.
 * CX_EINVAL: a null pointer, C < 1, a negative len[c] or offs[c].  CX_ESHAPE: U outside [1, CX_BOOT_MAX_UNITS], ldz < U.  CX_EALIGN:
 * order not 4-byte, z not 8-byte aligned.
 * cx_delong_gram: g[p][q] = sum_{u < U} z[p][u] * z[q][u] mod 2^64 for the Q rows of z (pitch ldz >= U), g row-major Q x Q, symmetric
 * (p <= q is computed and mirrored); the entry point zeroes g itself.  A workgroup stages tiles of CX_DELONG_TILE units x Q rows in
 * LDS (33 KB at Q = 128), a thread keeps up to three 4 x 4 blocks of g in registers over all the tiles of its workgroup (64-bit
 * multiply-add on the vector ALU) and adds them to g with 64-bit integer atomics at the end.
 * CX_EINVAL: a null pointer.  CX_ESHAPE: Q outside [1, CX_DELONG_MAX_ROWS], U outside [1, CX_BOOT_MAX_UNITS], ldz < U.  CX_EALIGN: z or
 * g not 8-byte aligned.  Additive entry points of ABI 10.                                                                          */
enum { CX_DELONG_MAX_ROWS = 128, CX_DELONG_WG_ENTRIES = 16384, CX_DELONG_TILE = 32 };
int cx_delong_place(const int32_t* order /* device */, const int64_t* offs /* host, [C] */, const int32_t* len /* host, [C] */, int C,
                    int U, int64_t* z, int ldz, void* stream);
int cx_delong_gram(const int64_t* z, int ldz, int Q, int U, int64_t* g, void* stream);

/* Pixel attribution maps (saliency.hip; chexpert_amd/saliency.py: input_gradient, smoothgrad, integrated_gradients, and the numpy
 * statement of the three entry points, points_reference / accumulate_reference / finish_reference): the glue around the eval-mode
 * forward + backward with dx.  fp32 NCHW, N = 3 * H * W floats per row; every product and every sum below is rounded to fp32 on its
 * own (nothing is contracted into a fused multiply-add), so the results are those of the numpy statement bit for bit -- the noise
 * term excepted, whose logf / cospif are the device's.  One writer per output element, no atomics: the same bits on every run.
 * cx_sal_points writes out (R,3,H,W), the rows the network is evaluated at.  With b = img[r] (device table, clamped into [0, B)) and
 * base[b][e] = the full baseline (B,3,H,W), or, base == NULL, the constant base0 / base1 / base2 of e's channel:
 *   d = x[b][e] - base[b][e];   v = base[b][e] + alpha[r] * d;
 *   out[r][e] = v                                                     (sigma == NULL)
 *   out[r][e] = v + sigma[b] * n(seed, (first_row + r) * N + e)       (sigma: device table, one fp32 per image)
 * Baseline 0 and alpha 1 give x exactly.  n(seed, k) is one standard normal per hash, so a row's noise depends on (seed, first_row + r)
 * only and not on how the rows are cut into calls.  With z = the splitmix64 hash of cx_boot_counts above (z = seed + 0x9E37... * (k + 1), ...):
 *   u1 = ((z >> 40) + 1) * 2^-24;   u2 = ((z >> 8) & 0xFFFFFF) * 2^-24;   n = sqrtf(-2 * logf(u1)) * cospif(2 * u2)       (|n| <= 5.77)
 * cx_sal_accumulate folds the input gradients g (R,3,H,W) of a pass into acc (P,3,H,W).  Per element of plane p: a = acc (accumulate
 * != 0) or 0; for r = 0 .. R - 1 in this order, where slot[r] == p: t = g[r] (square == 0) or g[r] * g[r]; a = a + w[r] * t; acc = a.
 * slot (int32) and w (fp32) are device tables of R entries; a slot outside [0, P) belongs to no plane.
 * cx_sal_finish turns the sums into maps.  a[p][c] = acc[p][c] (times_input == 0) or acc[p][c] * (x[b][c] - base[b][c]) with
 * b = img_of[p] (device table, clamped into [0, B)) and the baseline as above.  mode CX_SAL_NONE: out (P,3,H,W) = a; the others give
 * out (P,H,W): CX_SAL_SUM (a0 + a1) + a2, CX_SAL_ABS (|a0| + |a1|) + |a2|, CX_SAL_MAX max(max(|a0|, |a1|), |a2|).  total != NULL:
 * total[p] (double) = the sum of a over the 3 H W elements of plane p (the left side of the completeness identity of integrated
 * gradients), accumulated in double in two fixed stages: CX_SAL_PARTIALS workgroup sums per plane into partial (P * CX_SAL_PARTIALS
 * doubles, the caller's), then their sum in ascending order.
 * Any H, W >= 1 (one float4 per lane where N % 4 == 0 -- finish: H W % 4 == 0 -- and the tensors are 16-byte aligned, one float
 * otherwise).  CX_EINVAL before anything is launched: a null pointer (base, sigma, total always may be null; x, img_of when
 * times_input == 0; partial when total is), B, R, P, H or W <= 0, an output that aliases an input, total without partial.
 * CX_ESHAPE: H * W >= 2^29, R or P > 65535, an unknown mode.  CX_EALIGN: a pointer that is not 4-byte (total, partial: 8-byte) aligned.
 * Additive entry points of ABI 10.                                                                                              */
enum { CX_SAL_NONE = 0, CX_SAL_SUM = 1, CX_SAL_ABS = 2, CX_SAL_MAX = 3, CX_SAL_PARTIALS = 128 };
int cx_sal_points(const float* x, const float* base, float base0, float base1, float base2, const int32_t* img, const float* alpha,
                  const float* sigma, uint64_t seed, uint64_t first_row, float* out, int B, int R, int H, int W, void* stream);
int cx_sal_accumulate(const float* g, const int32_t* slot, const float* w, float* acc, int R, int P, int H, int W, int square,
                      int accumulate, void* stream);
int cx_sal_finish(const float* acc, const float* x, const float* base, float base0, float base1, float base2, const int32_t* img_of,
                  float* out, double* total, double* partial, int P, int B, int H, int W, int times_input, int mode, void* stream);

/* ---- global pooling heads other than the average (csrc/pool_head.hip; numpy statement: chexpert_amd/pooling.py).
 * a[b][p][c] = act(x[b][p][c] * sc[c] + sh[c]) over the HW pixels p of image b; act = CX_POOL_ACT_RELU (DenseNet; ResNet with sc = 1,
 * sh = 0) or CX_POOL_ACT_SWISH (the EfficientNet head).  The average stays with cx_head_fwd / cx_gap_relu_bn_bwd and
 * cx_gap_affine_act / cx_se_act_bwd: CX_POOL_AVG is a name for the callers, these entries refuse it.
 *
 *   kind          pooled[b][c]                                                    d pooled / d a[b][p][c]
 *   CX_POOL_MAX   max_p a                                                         1 at the FIRST maximal pixel in ascending p, else 0
 *   CX_POOL_LSE   m + log(mean_p exp(r (a - m))) / r,  m = max_p a,  r > 0        exp(r (a - pooled)) / HW
 *   CX_POOL_GEM   (mean_p a'^q)^(1/q),  a' = max(a, 1e-6),  q = clamp(p, 1, 16)   a'^(q-1) pooled^(1-q) / HW where a > 1e-6, else 0
 *
 * GeM's exponent is trained: d pooled / d p = pooled (T - ln pooled) / q with T = sum_p a'^q ln a' / sum_p a'^q, and 0 where p is
 * clamped (p <= 1 or p >= 16).  The activation's derivative multiplies d pooled / d a: the ReLU mask x*sc + sh > 0, or swish'.
 * LSE and GeM are computed relative to the column maximum (two walks over the column), so an activation of 1e4 stays finite
 * with r = 10 and with p = 16.  param: the device pointer to r (LSE) or p (GeM), one fp32 value read by the kernel -- a captured step
 * sees an in-place change --, NULL for the maximum.
 *
 * Forward: pooled fp32 (B, C); aux fp32 (B, C) receives T for GeM, for LSE the offset pooled - m = log(mean_p exp(r (a - m))) / r, and
 * is not touched by the maximum (may be NULL then).  No pitch padding of x is read.
 * Backward: the contract of cx_gap_relu_bn_bwd -- dz = dpooled * (d pooled / d a) * act', g = e_scale * dz (storage type, pitch ldg,
 * padding untouched), S1 = sum dz, S2 = sum dz (x - mean) rstd; stat_rows == 0: fp32 atomics into S1 / S2 [C]; stat_rows > 0:
 * exactly one row per image (row b at S[b*C + c], the row count B is what the last-stat-rows query returns, two calls give equal
 * bits), CX_ESTATROWS below B rows with nothing written.  The maximum stores no arg-max: the backward evaluates the same fmaf and
 * activation, which gives the forward's bits, and the first pixel that equals pooled takes the gradient.  LSE forms a - pooled as
 * (a - m) - aux with the column maximum found again: next to a maximum of 1e4 pooled itself is rounded to 1e-3, and r times that
 * would be the gradient's relative error.  GeM's backward does not read aux (the exponent's gradient does).
 * cx_pool_p_grad: dp[0] += sum_{b,c} dpooled pooled (T - ln pooled) / q in a fixed order (one workgroup, no atomics).
 * Checks, before any launch: CX_EINVAL a NULL operand (param and aux where the kind needs them), an unknown kind or act; CX_ESHAPE C % 8, a pitch % 8, a pitch below C, a size <= 0; CX_EALIGN x or g not 16-byte aligned.  Additive entry points of
 * ABI 10.                                                                                                                       */
enum { CX_POOL_AVG = 0, CX_POOL_MAX = 1, CX_POOL_LSE = 2, CX_POOL_GEM = 3 };
enum { CX_POOL_ACT_RELU = 1, CX_POOL_ACT_SWISH = 2 };        /* the codes of cx_gap_affine_act's act */
int cx_pool_head_fwd(const void* x, const float* sc, const float* sh, float* pooled, float* aux, const float* param, int B, int HW,
                     int C, int ldx, int act, int kind, void* stream);
int cx_pool_head_bwd(const float* dpooled, const float* pooled, const float* aux, const float* param, const void* x, const float* sc,
                     const float* sh, const float* mean, const float* rstd, const float* e_scale, void* g, float* S1, float* S2, int B,
                     int HW, int C, int ldx, int ldg, int act, int kind, int stat_rows, void* stream);
int cx_pool_p_grad(const float* dpooled, const float* pooled, const float* aux, const float* p, float* dp, int B, int C, void* stream);
int cx_pool_head_fwd_f32(const void* x, const float* sc, const float* sh, float* pooled, float* aux, const float* param, int B, int HW,
                         int C, int ldx, int act, int kind, void* stream);
int cx_pool_head_bwd_f32(const float* dpooled, const float* pooled, const float* aux, const float* param, const void* x,
                         const float* sc, const float* sh, const float* mean, const float* rstd, const float* e_scale, void* g,
                         float* S1, float* S2, int B, int HW, int C, int ldx, int ldg, int act, int kind, int stat_rows, void* stream);

/* ---- class-specific residual attention head (csrc/csra_head.hip; FusedNet.set_head("csra"); chexpert_amd/heads.py states the same
 * in numpy float64).  The classifier is applied at every pixel and the score map is pooled per class (CSRA; Zhu & Wu, ICCV 2021).
 * For image b, a[b,p,c] = act(x[b,p,c] sc[c] + sh[c]) m[b,c], act = CX_POOL_ACT_RELU or CX_POOL_ACT_SWISH, m the optional
 * per-(image, channel) multiplier (the EfficientNet head's Dropout mask; NULL: 1), W (n, C), bias (n,) or NULL, lam_T = the device
 * pointer to [lambda, T] (lambda >= 0, T > 0; read by the kernels, so a captured step sees a changed value):
 *
 *   s[b,k,p]   = sum_c W[k,c] a[b,p,c]                     (no bias: the softmax does not see it)
 *   w[b,k,p]   = softmax over p of T s[b,k,p]              (relative to max_p s: a score of 1e4 stays finite)
 *   att[b,k]   = sum_p w[b,k,p] s[b,k,p]
 *   logit[b,k] = bias[k] + mean_p s[b,k,p] + lambda att[b,k]
 *
 *   ds[b,k,p]  = dlogit[b,k] (1/HW + lambda w[b,k,p] (1 + T (s[b,k,p] - att[b,k])))
 *   da[b,p,c]  = m[b,c] sum_k ds[b,k,p] W[k,c],   dz = da act'(z),   g = e_scale dz,   S1 = sum dz,   S2 = sum dz (x - mean) rstd
 *   dW[k,c]   += sum_{b,p} ds[b,k,p] a[b,p,c],    db[k] += sum_b dlogit[b,k]
 *
 * lambda = 0 is the average head (cx_head_fwd) as a function; the scores are not divided by |W_k| and the bias is kept, one head,
 * no T = infinity branch.  All sums are fp32 on the VALU: the activated operand is not rounded to bf16.
 *
 * cx_csra_head_fwd: x (B, HW, ldx) in the storage type, padding never read; logits (B, n), s (B, n, HW) fp32 and stat (B, n, 4) fp32
 * = [max_p s, 1 / sum_p exp(T (s - max)), att - max, 0], which the backward reads.
 * cx_csra_head_bwd: the contract of cx_gap_relu_bn_bwd / cx_pool_head_bwd: g in the storage type at pitch ldg, padding untouched;
 * stat_rows == 0: fp32 atomics into S1 / S2 (C each); stat_rows > 0: row b of S1 / S2 = the sums of image b, plain stores,
 * cx_last_stat_rows() returns B, CX_ESTATROWS with nothing written below B rows.  dW (n, C) and db (n,; may be NULL) are ADDED to,
 * like cx_head_bwd's, from per-group partial sums in `scratch` added in a fixed order: no atomics on dW / db, and in rows mode two
 * calls on the same inputs give equal bits in every output.  scratch: scratch_len floats, at least cx_csra_bwd_scratch(B, HW, C, n)
 * (= B HW n' + groups n C with n' = n rounded up to 16 / 32 / 64 and groups <= 128); a smaller one is CX_EUNSUPPORTED (there is no
 * other path).  The contents of scratch are undefined afterwards.
 * Checks, before any launch: CX_EINVAL a NULL operand (m, bias, db may be NULL) or an unknown act; CX_ESHAPE n < 1, a size <= 0, C or
 * a pitch % 8 (bf16 storage) / % 4 (fp32 storage), a pitch below C; CX_EUNSUPPORTED n > CX_CSRA_MAX_CLASSES or the scratch too
 * small; CX_EALIGN x, g or scratch not 16-byte aligned.  Additive entry points of ABI 10.                                       */
#define CX_CSRA_MAX_CLASSES 64
int cx_csra_head_fwd(const void* x, const float* sc, const float* sh, const float* m, const float* W, const float* bias, const float* lam_T,
                     float* logits, float* s, float* stat, int B, int HW, int C, int ldx, int n, int act, void* stream);
int cx_csra_head_bwd(const float* dlogits, const float* s, const float* stat, const float* lam_T, const void* x, const float* sc,
                     const float* sh, const float* m, const float* mean, const float* rstd, const float* e_scale, const float* W, void* g,
                     float* S1, float* S2, float* dW, float* db, float* scratch, long long scratch_len, int B, int HW, int C, int ldx, int ldg,
                     int n, int act, int stat_rows, void* stream);
int cx_csra_head_fwd_f32(const void* x, const float* sc, const float* sh, const float* m, const float* W, const float* bias,
                         const float* lam_T, float* logits, float* s, float* stat, int B, int HW, int C, int ldx, int n, int act, void* stream);
int cx_csra_head_bwd_f32(const float* dlogits, const float* s, const float* stat, const float* lam_T, const void* x, const float* sc,
                         const float* sh, const float* m, const float* mean, const float* rstd, const float* e_scale, const float* W, void* g,
                         float* S1, float* S2, float* dW, float* db, float* scratch, long long scratch_len, int B, int HW, int C, int ldx,
                         int ldg, int n, int act, int stat_rows, void* stream);
long long cx_csra_bwd_scratch(int B, int HW, int C, int n);      /* floats; CX_ESHAPE / CX_EUNSUPPORTED as above */

/* ---- probabilistic-CAM pooling head (csrc/csra_head.hip; FusedNet.set_head("pcam"); chexpert_amd/heads.py states the same in numpy
 * float64).  PCAM (Ye et al., "Weakly Supervised Lesion Localization With Probabilistic-CAM Pooling", 2020): the classifier at every
 * pixel, each per-pixel logit turned into a probability, the map pooled per class with those probabilities as weights.  a, W, bias
 * and m are those of the csra head above; sigma is the logistic function:
 *
 *   s[b,k,p]   = sum_c W[k,c] a[b,p,c]                     (csra's score map: the same kernel, the same bits)
 *   u[b,k,p]   = s[b,k,p] + bias[k]                        (bias NULL: 0)
 *   w[b,k,p]   = sigma(u[b,k,p]) / sum_q sigma(u[b,k,q])   evaluated as softmax over p of log sigma(u), relative to its maximum
 *   logit[b,k] = sum_p w[b,k,p] u[b,k,p]
 *   P[b,k,p]   = sigma(u[b,k,p])                           the probability map
 *
 *   q[b,k,p]   = sigma(-u[b,k,p])
 *   ds[b,k,p]  = dlogit[b,k] w[b,k,p] (1 + q[b,k,p] (u[b,k,p] - logit[b,k]))
 *   r[b,k]     = sum_p w[b,k,p] q[b,k,p] (u[b,k,p] - logit[b,k])
 *   db[k]     += sum_b dlogit[b,k] (1 + r[b,k])            (the bias is inside sigma: not csra's sum_b dlogit)
 *   da, dz, g = e_scale dz, S1, S2, dW: the csra lines with this ds
 *
 * One nn.Linear is shared by all classes' maps, the gradient flows through w, and there is no hyper-parameter, hence no lam_T.
 * sigma(u), sigma(-u) and log sigma(u) are formed from one exp(-|u|); scores of +-1e4 stay finite.
 *
 * cx_pcam_head_fwd: the arguments of cx_csra_head_fwd without lam_T.  stat (B, n, 4) fp32 = [max_p u, 1 / sum_p exp(log sigma(u) -
 * log sigma(max_p u)), logit - max_p u, bias[k]]: relative to the largest u of the row, so that a score of 1e4 beside ordinary ones
 * costs nothing in u - logit = (u - max u) - stat[2] or in w; the bias rides along for the way back, whose argument list has none.
 * cx_pcam_head_bwd: the arguments and the contract of cx_csra_head_bwd without lam_T (g, S1 / S2 atomic or one row per image,
 * CX_ESTATROWS; dW and db ADDED to in a fixed order, no atomics, equal bits over two calls).  scratch: at least
 * cx_pcam_bwd_scratch(B, HW, C, n) = cx_csra_bwd_scratch(B, HW, C, n) + B n floats (the last B n hold dlogit (1 + r)); a shorter one
 * is CX_EUNSUPPORTED with nothing written.  The checks are those of the csra entry points.  Additive entry points of ABI 10.     */
int cx_pcam_head_fwd(const void* x, const float* sc, const float* sh, const float* m, const float* W, const float* bias, float* logits,
                     float* s, float* stat, int B, int HW, int C, int ldx, int n, int act, void* stream);
int cx_pcam_head_bwd(const float* dlogits, const float* s, const float* stat, const void* x, const float* sc, const float* sh, const float* m,
                     const float* mean, const float* rstd, const float* e_scale, const float* W, void* g, float* S1, float* S2, float* dW,
                     float* db, float* scratch, long long scratch_len, int B, int HW, int C, int ldx, int ldg, int n, int act, int stat_rows,
                     void* stream);
int cx_pcam_head_fwd_f32(const void* x, const float* sc, const float* sh, const float* m, const float* W, const float* bias, float* logits,
                         float* s, float* stat, int B, int HW, int C, int ldx, int n, int act, void* stream);
int cx_pcam_head_bwd_f32(const float* dlogits, const float* s, const float* stat, const void* x, const float* sc, const float* sh,
                         const float* m, const float* mean, const float* rstd, const float* e_scale, const float* W, void* g, float* S1,
                         float* S2, float* dW, float* db, float* scratch, long long scratch_len, int B, int HW, int C, int ldx, int ldg, int n,
                         int act, int stat_rows, void* stream);
long long cx_pcam_bwd_scratch(int B, int HW, int C, int n);      /* floats; CX_ESHAPE / CX_EUNSUPPORTED as above */

/* ---- fp32 storage mode (CX_DT_F32): the element-wise kernels of the DenseNet path with fp32 activation tensors (same arguments,
 * `const void*` tensors are fp32, pitches in elements), the fp32 weight table ([tap][O][I] fp32; descriptors with stem = 1 give
 * [49][O][4]) and the fp32 image layouts.  cx_conv_gemm / cx_conv_wgrad take CxConv.dtype / CxWgrad.dtype = CX_DT_F32.          */
int cx_pack_weights_table_f32(const float* flat, float* packed, const CxPackDesc* table_dev, int n_desc, void* stream);
int cx_nchw3_to_nhwc4_f32(const float* x, float* y, int B, int H, int W, void* stream);
int cx_u8_to_nhwc4_f32(const uint8_t* x, float* y, size_t npix, float mean, float std, void* stream);
int cx_bnrelu_maxpool_fwd_f32(const void* x, const float* scale, const float* shift, void* y, uint8_t* argmax,
                          float* stat_sum, float* stat_sq, int B, int H, int W, int C, int ldy, int stat_rows, void* stream);
int cx_bnrelu_maxpool_bwd_f32(const void* x, const float* scale, const float* shift, const float* mean,
                          const float* rstd, const uint8_t* argmax, const void* g, const void* gx, const float* ga,
                          const float* gb, const float* gc, void* dz, float* S1, float* S2, int B, int H, int W, int C,
                          int ldg, int ldgx, int stat_rows, void* stream);
int cx_head_fwd_f32(const void* x, const float* scale, const float* shift, const float* w, const float* bias,
                float* pooled, float* logits, int B, int HW, int C, int ldx, int n_classes, void* stream);
int cx_gap_relu_bn_bwd_f32(const float* dpooled, const void* x, const float* scale, const float* shift,
                       const float* mean, const float* rstd, const float* e_scale, void* g, float* S1, float* S2,
                       int B, int HW, int C, int ldx, int ldg, int stat_rows, void* stream);
int cx_unpool2_mask_f32(const void* d, const void* x, const float* sc, const float* sh, const float* mean,
                    const float* rstd, const float* e_scale, void* g, float* S1, float* S2, int B, int H, int W,
                    int C, int ldd, int ldx, int ldg, int stat_rows, void* stream);

/* utilities */
int cx_fill_f32(float* p, float v, size_t n, void* stream);
/* ABI 9: dst = src as a 16-byte-per-lane grid-stride copy (bytes % 16 == 0, both 16-byte aligned): the measured stream rate of the
 * device that bench.py reports next to the 8 TB/s specification ("a stream-copy micro-benchmark"); no
 * reference counterpart */
int cx_copy_stream(const void* src, void* dst, size_t bytes, void* stream);
/* y (B,C,H,W) fp32 = act(x*scale + shift) of a bf16 NHWC tensor (scale/shift NULL: identity; relu != 0: ReLU): the tensor a
 * forward hook on the reference's hook targets receives (features.norm5 / layer4 / head[1], chexpert.py:468, :484, :498)      */
int cx_affine_to_f32_nchw(const void* x, const float* scale, const float* shift, int relu, float* y, int B, int H, int W, int C,
                          int ldx, void* stream);
int cx_bf16_to_f32_nchw(const void* x, float* y, int B, int H, int W, int C, int ldx, void* stream);

/* ---- exact k-nearest-neighbour search and the weighted vote (csrc/knn.hip): the kNN probe of a frozen backbone (Wu et al., CVPR 2018)
 * and image retrieval on the pooled features.  No reference counterpart.  Additive entry points of ABI 10.
 *
 * The order that defines "nearest".  A (similarity, bank index) pair is one 64-bit key: the high word is the fp32 similarity as an
 * order-preserving unsigned integer (u = the bits; u >= 2^31 ? ~u : u | 2^31; a NaN similarity counts as -inf, -0 as +0), the low
 * word is 0xFFFFFFFF - index.  The result of a query is its k largest keys in descending key order: the larger similarity first, the
 * lower bank index among equal similarities.  The order is total, so the result does not depend on how the bank was tiled or split.
 *
 * cx_knn_normalize: y = x / max(|x|, 1e-12) per row of the (rows, d) fp32 matrix, |x| = sqrtf of the fp32 sum of squares (the
 *   normalisation of the contrastive loss); x == y is allowed.  CX_EINVAL: NULL x / y, rows < 1, d outside [1, CX_KNN_MAX_D].
 * cx_knn_topk: q (Q, d), bank (M, d) fp32 row-major; the similarity is the plain inner product (cosine: normalise both sides first),
 *   in fp32 on the fp32-input MFMA, an fmaf chain over two interleaved halves of d.  q_group (Q,) / bank_group (M,) int32, both or
 *   neither: a bank row whose group equals the query's group, that group >= 0, is no candidate (the group = the row's own position:
 *   leave-one-out; = the patient: patient-disjoint search).  out_sim (Q, k) fp32, out_idx (Q, k) int32; a query with fewer than k
 *   candidates has idx = -1, sim = -inf in the tail.  splits = the slices the bank is cut into (of whole 128-row tiles; a slice past
 *   the bank's end is empty): 0 = chosen here from Q, M and the device's compute units, a positive value forces that many (the
 *   kernel_hint of this entry point).  scratch: the caller's, cx_knn_scratch floats (Q x slices x k keys), 8-byte aligned; nothing
 *   is allocated, nothing is sized by Q x M, no atomics: the same bits on every run and for every value of splits.
 *   CX_EINVAL before any launch: NULL q / bank / out_sim / out_idx / scratch, one group pointer without the other, Q < 1, M < 1,
 *   d outside [1, CX_KNN_MAX_D], k outside [1, CX_KNN_MAX_K], splits outside [0, CX_KNN_MAX_SPLITS], scratch_floats too small.
 *   CX_EALIGN: a pointer that is not 4-byte aligned, a scratch that is not 8-byte aligned.  cx_knn_scratch returns 0 for refused sizes.
 * cx_knn_vote: labels (M, n) fp32, targets in [0, 1], a value < 0 = ignored.  For query q over its valid neighbours j (idx >= 0) in
 *   list order, s_0 the first of them: w_j = exp((s_j - s_0) * inv_T) (1 where inv_T == 0 or s_j == s_0);
 *   num_c = sum_j w_j y[idx_j, c] and den_c = sum_j w_j over the neighbours whose label c is not ignored; out_score (Q, n) = num_c /
 *   den_c, out_support (Q, n) = den_c; den_c == 0: score 0.5, support 0.  Weights and sums in double, in list order, each result
 *   rounded to fp32 once: bit-reproducible.
 *   CX_EINVAL: a NULL pointer, Q < 1, k outside [1, CX_KNN_MAX_K], n outside [1, CX_KNN_MAX_CLASSES], inv_T < 0 or NaN.            */
#define CX_KNN_MAX_K 256
#define CX_KNN_MAX_D 4096
#define CX_KNN_MAX_SPLITS 256
#define CX_KNN_MAX_CLASSES 64
long long cx_knn_scratch(int Q, int M, int k, int splits);
int cx_knn_normalize(const float* x, float* y, int rows, int d, void* stream);
int cx_knn_topk(const float* q, const float* bank, const int* q_group, const int* bank_group, float* out_sim, int* out_idx, float* scratch,
                long long scratch_floats, int Q, int M, int d, int k, int splits, void* stream);
int cx_knn_vote(const float* sim, const int* idx, const float* labels, float* out_score, float* out_support, float inv_T, int Q, int k,
                int n, void* stream);

/* ---- the linear probe (csrc/probe.hip): multi-label L2-regularised logistic regression on a bank of pooled features, the linear
 * evaluation of SimCLR / MoCo / MoCo-CXR, and the vector arithmetic of its L-BFGS solver.  No reference counterpart.  Additive entry
 * points of ABI 10.  The definition in float64 is chexpert_amd/probe.py (reference_loss_grad).
 *
 * x (M, d) fp32; y (M, n) fp32 in [0, 1], a value < 0 = ignored; theta (n, d + 1) fp32 row-major, theta[c, :d] = w_c, theta[c, d] =
 * b_c; pos_weight (n,) or NULL (ones); l2 >= 0.  Per class c over its live rows (N_c = max(their number, 1)), z = x . w_c + b_c:
 *   loss_c = (1 / N_c) sum [pw y softplus(-z) + (1 - y) softplus(z)] + (l2 / 2) |w_c|^2      (the bias is not regularised)
 *   r      = (pw y + 1 - y) sigmoid(z) - pw y;   grad_c[:d] = (1 / N_c) sum r x + l2 w_c;   grad_c[d] = (1 / N_c) sum r
 * cx_probe_scratch: the floats of scratch for a bank of M rows (the larger of what cx_probe_loss_grad and cx_probe_colstats need);
 *   0 for refused sizes: M < 1, d outside [1, CX_KNN_MAX_D], n outside [1, CX_KNN_MAX_CLASSES], splits outside [0, CX_PROBE_MAX_SPLITS].
 * cx_probe_colstats: mean (d,) = the column means of x, rstd (d,) = 1 / max(population standard deviation, 1e-6).  Two passes (the
 *   sum, then the squared distances from the double mean), each accumulated in double: slices of rows first, then the slices in
 *   order; each result rounded to fp32 once.  scratch 8-byte aligned.
 * cx_probe_standardize: y = (x - mean) * rstd, the difference and the product rounded separately; x == y is allowed.
 * cx_probe_logits: out (rows, n) = x w^T + b on v_mfma_f32_16x16x4_f32 (the tile code of cx_probe_loss_grad).
 * cx_probe_loss_grad: loss (n,), grad (n, d + 1), count (n, 3) = live rows, sum y, sum (1 - y) over them.  Two launches: each slice
 *   of the bank leaves its partial sums in the scratch, then the slices are added in slice order, divided by N_c once (fp32) and
 *   l2 w is added by one fma.  active (n,) int32 or NULL: a class whose flag is 0 keeps the previous bits of its loss, grad and count.
 *   splits: 0 = chosen here from M and the device's compute units.  No atomics: the same bits on every run for the same splits;
 *   another splits is another summation order.
 * cx_probe_lbfgs_direction: one workgroup per active class.  dir_c = -H g_c by the two-loop recursion over the class's history of
 *   pairs (s_hist, y_hist: (n, m, d + 1); hist (n, 2) int32: the pairs held and the slot the next one goes to; both zero at the
 *   start), initial scaling s.y / y.y of the newest pair, every dot product a fixed-order reduction; -g_c where that does not
 *   descend.  stats (n, 4): g . dir, max |g|, sum |g|, 1 where the fallback was taken.
 * cx_probe_lbfgs_advance: per class by mode (n,) int32.  1: theta_t = theta + t_c dir_c.  2: the trial is accepted: the pair
 *   (theta_t - theta, grad_t - grad) joins the history unless s.y <= 0, then theta = theta_t and grad = grad_t.  3: tstats (n, 2) =
 *   grad_t . dir_c, max |grad_t|: the trial's slope (f is convex, so f(theta_t) <= f(theta) + t grad_t . dir: a slope that is still
 *   steep enough certifies the sufficient decrease where the fp32 loss cannot resolve it).  0: nothing is written.
 * CX_EINVAL before any launch: a NULL pointer that is not optional, a size outside the limits above, m outside
 *   [1, CX_PROBE_MAX_HISTORY], l2 < 0 or not finite, scratch_floats too small.  CX_EALIGN: a misaligned pointer.                        */
#define CX_PROBE_MAX_SPLITS 1024
#define CX_PROBE_MAX_HISTORY 16
long long cx_probe_scratch(int M, int d, int n, int splits);
int cx_probe_colstats(const float* x, float* mean, float* rstd, float* scratch, long long scratch_floats, int M, int d, void* stream);
int cx_probe_standardize(const float* x, const float* mean, const float* rstd, float* y, long long rows, int d, void* stream);
int cx_probe_logits(const float* x, const float* theta, float* out, int rows, int d, int n, void* stream);
int cx_probe_loss_grad(const float* x, const float* y, const float* theta, const float* pos_weight, float l2, const int* active,
                       float* loss, float* grad, float* count, float* scratch, long long scratch_floats, int M, int d, int n, int splits,
                       void* stream);
int cx_probe_lbfgs_direction(const float* grad, const float* s_hist, const float* y_hist, const int* hist, const int* active, float* dir,
                             float* stats, int n, int d, int m, void* stream);
int cx_probe_lbfgs_advance(float* theta, float* grad, const float* dir, const float* t, const int* mode, float* theta_t,
                           const float* grad_t, float* s_hist, float* y_hist, int* hist, float* tstats, int n, int d, int m, void* stream);

#ifdef __cplusplus
}
#endif
#endif
