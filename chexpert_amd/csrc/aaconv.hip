// Attention-augmented convolution (AAConv2d, /root/reference/models/attn_aug_conv.py:19-100) on gfx950.
//
// The reference materialises the (B, nh, HW, HW) logits, two expanded relative-logit tensors, the softmax
// and its autograd copies (82 MB per image at HW = 1600).  Here nothing of size HW x HW ever exists:
//
//   S[i][j] = q~_i . k_j + rh_i[ky(j)] + rw_i[kx(j)],   rh_i[ky] = q~_i . key_rel_h[:, ky - qy + H - 1],
//                                                        rw_i[kx] = q~_i . key_rel_w[:, kx - qx + W - 1]
//
// (closed form of rel_to_abs / relative_logits_1d, :43-63, :77-86).  One lane owns one query: q~ (dkh = 20
// values) lives in registers, its two relative-logit rows (H + W values) in LDS, keys / values stream
// through LDS tiles and are read as broadcasts, softmax is online (one exp per key).  dkh = 20 and
// dvh in {1,3,6} make the matrix cores pointless here (hard part 3): this is VALU work
// bounded by LDS broadcast reads.  The backward pass recomputes P from the saved log-sum-exp.
#include <type_traits>
#include "common.h"

// aaconv_row.hip: row-streamed kernels for map widths 40 and 20 (which: 0 forward, 1 the whole backward)
int cx_try_aa_row(int which, const void* qkv, const float* rel_h, const float* rel_w, float* o, const float* d_o, float* lse, float* dqkv,
                  float* d_rel_h, float* d_rel_w, float* slab_h, float* slab_w, int B, int H, int W, int nh, int dk, int dv, int ldq,
                  hipStream_t st, bool* handled);
int cx_rows_reduce_add_impl(float* dst, const float* rows, int n_rows, int C, int rstride, hipStream_t st);     // elementwise.hip
// aaconv_heads.hip: the same four operations for head widths 1 <= dk/nh, dv/nh <= 64 (runtime values), dv <= 104
int cx_aa_heads_fwd(int f32, const void* qkv, const float* rel_h, const float* rel_w, float* o, float* lse, int B, int H, int W, int nh,
                    int dk, int dv, int ldq, hipStream_t st);
int cx_aa_heads_weights(int f32, const void* qkv, const float* rel_h, const float* rel_w, const float* lse, float* wts, int B, int H, int W,
                        int nh, int dk, int dv, int ldq, hipStream_t st);
int cx_aa_heads_bwd(int f32, const void* qkv, const float* rel_h, const float* rel_w, const float* o, const float* d_o, const float* lse,
                    float* dqkv, float* d_rel_h, float* d_rel_w, float* slab_h, float* slab_w, int B, int H, int W, int nh, int dk, int dv,
                    int ldq, hipStream_t st);

namespace {

constexpr int AQ = 128;      // queries per workgroup (one per thread)
constexpr int TK = 64;       // keys per LDS tile
constexpr int DKH = 20;      // head dim of q/k for every AA layer of the reference (dk = max(20*nh, ...) = 160, nh = 8)
constexpr int MAXDV = 13;       // dv/nh in {1,2,3,4,6,8}: every AA layer chexpert.py trains, and WRN-28-10's third stage (dv 64 at 8 heads);
                                // 9 and 13: the Densenet-BC transitions of the CIFAR harness at v = 0.7 (models/readme.md:34-38)

struct AAGeo {
  int B, H, W, nh, dk, dv, ldq;     // qkv tensor: (B, H*W, ldq) bf16, channels [q dk | k dk | v dv]
};

// ---------------------------------------------------------------------------------------------- forward
template <typename T, int DVH>
__global__ __launch_bounds__(AQ) void aa_attn_fwd_kernel(const T* __restrict__ qkv, const float* __restrict__ rel_h,
                                                        const float* __restrict__ rel_w, float* __restrict__ o,
                                                        float* __restrict__ lse, const AAGeo g) {
  extern __shared__ __attribute__((aligned(16))) float lds[];
  const int H = g.H, W = g.W, HW = H * W;
  const int LH = 2 * H - 1, LW = 2 * W - 1;
  float* RH = lds;                       // [DKH][LH]
  float* RW = RH + DKH * LH;             // [DKH][LW]
  float* rh = RW + DKH * LW;             // [AQ][H+1]
  float* rw = rh + AQ * (H + 1);         // [AQ][W+1]
  float* Kt = rw + AQ * (W + 1);         // [TK][DKH]
  float* Vt = Kt + TK * DKH;             // [TK][DVH]
  const int tid = threadIdx.x;
  const int bn = blockIdx.y, b = bn / g.nh, n = bn - b * g.nh;
  const int i = blockIdx.x * AQ + tid;
  const bool qvalid = i < HW;
  const int ic = qvalid ? i : HW - 1;
  const int qy = ic / W, qx = ic - qy * W;
  const T* base = qkv + (size_t)b * HW * g.ldq;

  for (int t = tid; t < DKH * LH; t += AQ) RH[t] = rel_h[t];
  for (int t = tid; t < DKH * LW; t += AQ) RW[t] = rel_w[t];
  float q[DKH];
  const float scale = rsqrtf((float)DKH);
  {
    const T* qp = base + (size_t)ic * g.ldq + n * DKH;
#pragma unroll
    for (int d = 0; d < DKH; d += 4) {
      const typename V4<T>::raw v = V4<T>::ld(qp + d);
#pragma unroll
      for (int e = 0; e < 4; ++e) q[d + e] = V4<T>::get(v, e) * scale;
    }
  }
  __syncthreads();
  for (int ky = 0; ky < H; ++ky) {
    float a = 0.f;
#pragma unroll
    for (int d = 0; d < DKH; ++d) a = fmaf(q[d], RH[d * LH + ky - qy + H - 1], a);
    rh[tid * (H + 1) + ky] = a;
  }
  for (int kx = 0; kx < W; ++kx) {
    float a = 0.f;
#pragma unroll
    for (int d = 0; d < DKH; ++d) a = fmaf(q[d], RW[d * LW + kx - qx + W - 1], a);
    rw[tid * (W + 1) + kx] = a;
  }

  float m = -3.0e38f, l = 0.f, acc[DVH];
#pragma unroll
  for (int d = 0; d < DVH; ++d) acc[d] = 0.f;
  const int kofs = g.dk + n * DKH, vofs = 2 * g.dk + n * DVH;
  for (int j0 = 0; j0 < HW; j0 += TK) {
    __syncthreads();
    // stage TK keys (20 bf16 = 5 x 8 B each) and values
    for (int t = tid; t < TK * 5; t += AQ) {
      const int j = t / 5, c = t - j * 5;
      const int jj = min(j0 + j, HW - 1);
      const typename V4<T>::raw v = V4<T>::ld(base + (size_t)jj * g.ldq + kofs + c * 4);
#pragma unroll
      for (int e = 0; e < 4; ++e) Kt[j * DKH + c * 4 + e] = V4<T>::get(v, e);
    }
    for (int t = tid; t < TK * DVH; t += AQ) {
      const int j = t / DVH, d = t - j * DVH;
      const int jj = min(j0 + j, HW - 1);
      Vt[t] = V4<T>::ld1(base + (size_t)jj * g.ldq + vofs + d);
    }
    __syncthreads();
    const int jn = min(TK, HW - j0);
    int ky = j0 / W, kx = j0 - ky * W;
#pragma unroll 4
    for (int j = 0; j < jn; ++j) {
      float s = rh[tid * (H + 1) + ky] + rw[tid * (W + 1) + kx];
      const float4* kp = reinterpret_cast<const float4*>(Kt + j * DKH);
#pragma unroll
      for (int c = 0; c < 5; ++c) {
        const float4 kv = kp[c];
        s = fmaf(q[4 * c], kv.x, fmaf(q[4 * c + 1], kv.y, fmaf(q[4 * c + 2], kv.z, fmaf(q[4 * c + 3], kv.w, s))));
      }
      if (s > m) {
        const float c = __expf(m - s);
        l = fmaf(l, c, 1.f);
#pragma unroll
        for (int d = 0; d < DVH; ++d) acc[d] = fmaf(acc[d], c, Vt[j * DVH + d]);
        m = s;
      } else {
        const float p = __expf(s - m);
        l += p;
#pragma unroll
        for (int d = 0; d < DVH; ++d) acc[d] = fmaf(p, Vt[j * DVH + d], acc[d]);
      }
      if (++kx == W) { kx = 0; ++ky; }
    }
  }
  if (qvalid) {
    const float inv = 1.f / l;
    float* op = o + ((size_t)b * HW + i) * g.dv + n * DVH;
#pragma unroll
    for (int d = 0; d < DVH; ++d) op[d] = acc[d] * inv;
    lse[(size_t)bn * HW + i] = m + __logf(l);
  }
}


// ---------------------------------------------------------------------------------------------- attention maps
// The reference keeps softmax(logits) of the last forward in AAConv2d.weights, (B, nh, HW, HW), for vis_attn
// (chexpert.py:363-383).  The training path never materialises it; this kernel rebuilds it on request from the saved
// log-sum-exp: one lane per query writes its row P[i][:] = exp(S[i][:] - lse[i]).  Visualisation only, not tuned.
template <typename T>
__global__ __launch_bounds__(AQ) void aa_attn_weights_kernel(const T* __restrict__ qkv, const float* __restrict__ rel_h,
                                                            const float* __restrict__ rel_w, const float* __restrict__ lse,
                                                            float* __restrict__ wts, const AAGeo g) {
  extern __shared__ __attribute__((aligned(16))) float lds[];
  const int H = g.H, W = g.W, HW = H * W;
  const int LH = 2 * H - 1, LW = 2 * W - 1;
  float* RH = lds;
  float* RW = RH + DKH * LH;
  float* rh = RW + DKH * LW;
  float* rw = rh + AQ * (H + 1);
  float* Kt = rw + AQ * (W + 1);
  const int tid = threadIdx.x;
  const int bn = blockIdx.y, b = bn / g.nh, n = bn - b * g.nh;
  const int i = blockIdx.x * AQ + tid;
  const bool qvalid = i < HW;
  const int ic = qvalid ? i : HW - 1;
  const int qy = ic / W, qx = ic - qy * W;
  const T* base = qkv + (size_t)b * HW * g.ldq;
  for (int t = tid; t < DKH * LH; t += AQ) RH[t] = rel_h[t];
  for (int t = tid; t < DKH * LW; t += AQ) RW[t] = rel_w[t];
  float q[DKH];
  const float scale = rsqrtf((float)DKH);
  {
    const T* qp = base + (size_t)ic * g.ldq + n * DKH;
#pragma unroll
    for (int d = 0; d < DKH; d += 4) {
      const typename V4<T>::raw v = V4<T>::ld(qp + d);
#pragma unroll
      for (int e = 0; e < 4; ++e) q[d + e] = V4<T>::get(v, e) * scale;
    }
  }
  __syncthreads();
  for (int ky = 0; ky < H; ++ky) {
    float a = 0.f;
#pragma unroll
    for (int d = 0; d < DKH; ++d) a = fmaf(q[d], RH[d * LH + ky - qy + H - 1], a);
    rh[tid * (H + 1) + ky] = a;
  }
  for (int kx = 0; kx < W; ++kx) {
    float a = 0.f;
#pragma unroll
    for (int d = 0; d < DKH; ++d) a = fmaf(q[d], RW[d * LW + kx - qx + W - 1], a);
    rw[tid * (W + 1) + kx] = a;
  }
  const float li = lse[(size_t)bn * HW + ic];
  float* row = wts + ((size_t)bn * HW + ic) * HW;
  const int kofs = g.dk + n * DKH;
  for (int j0 = 0; j0 < HW; j0 += TK) {
    __syncthreads();
    for (int t = tid; t < TK * 5; t += AQ) {
      const int j = t / 5, c = t - j * 5;
      const int jj = min(j0 + j, HW - 1);
      const typename V4<T>::raw v = V4<T>::ld(base + (size_t)jj * g.ldq + kofs + c * 4);
#pragma unroll
      for (int e = 0; e < 4; ++e) Kt[j * DKH + c * 4 + e] = V4<T>::get(v, e);
    }
    __syncthreads();
    const int jn = min(TK, HW - j0);
    int ky = j0 / W, kx = j0 - ky * W;
#pragma unroll 4
    for (int j = 0; j < jn; ++j) {
      float sl = rh[tid * (H + 1) + ky] + rw[tid * (W + 1) + kx];
      const float4* kp = reinterpret_cast<const float4*>(Kt + j * DKH);
#pragma unroll
      for (int c = 0; c < 5; ++c) {
        const float4 kv = kp[c];
        sl = fmaf(q[4 * c], kv.x, fmaf(q[4 * c + 1], kv.y, fmaf(q[4 * c + 2], kv.z, fmaf(q[4 * c + 3], kv.w, sl))));
      }
      if (qvalid) row[j0 + j] = __expf(sl - li);
      if (++kx == W) { kx = 0; ++ky; }
    }
  }
}

// ---------------------------------------------------------------------------------------------- backward
// Pass Q (one lane per query): recompute P from the saved LSE, dS = P (dP - delta), accumulate
//   dq_i = scale * sum_j dS_ij (k_j + RH[:, ky-qy+H-1] + RW[:, kx-qx+W-1])
//   dRH / dRW : sum_{i,j} dS_ij q~_i at the relative offsets (reduced per workgroup in LDS, then atomics)
// Pass K (one lane per key): dk_j = sum_i dS_ij q~_i, dv_j = sum_i P_ij dO_i.
template <typename T, int DVH>
__global__ __launch_bounds__(AQ) void aa_attn_bwd_q_kernel(const T* __restrict__ qkv, const float* __restrict__ rel_h,
                                                          const float* __restrict__ rel_w, const float* __restrict__ o,
                                                          const float* __restrict__ d_o, const float* __restrict__ lse,
                                                          float* __restrict__ dqkv, float* __restrict__ d_rel_h,
                                                          float* __restrict__ d_rel_w, float* __restrict__ slab_h,
                                                          float* __restrict__ slab_w, const AAGeo g) {
  extern __shared__ __attribute__((aligned(16))) float lds[];
  const int H = g.H, W = g.W, HW = H * W;
  const int LH = 2 * H - 1, LW = 2 * W - 1;
  float* RH = lds;
  float* RW = RH + DKH * LH;
  float* rh = RW + DKH * LW;             // [AQ][H+1]  logits rows, later re-used as d(rh)
  float* rw = rh + AQ * (H + 1);
  float* Kt = rw + AQ * (W + 1);
  float* Vt = Kt + TK * DKH;
  float* dRH = Vt + TK * DVH;            // [DKH][LH] workgroup partial
  float* dRW = dRH + DKH * LH;
  const int tid = threadIdx.x;
  const int bn = blockIdx.y, b = bn / g.nh, n = bn - b * g.nh;
  const int i = blockIdx.x * AQ + tid;
  const bool qvalid = i < HW;
  const int ic = qvalid ? i : HW - 1;
  const int qy = ic / W, qx = ic - qy * W;
  const T* base = qkv + (size_t)b * HW * g.ldq;

  for (int t = tid; t < DKH * LH; t += AQ) { RH[t] = rel_h[t]; dRH[t] = 0.f; }
  for (int t = tid; t < DKH * LW; t += AQ) { RW[t] = rel_w[t]; dRW[t] = 0.f; }
  float q[DKH];
  const float scale = rsqrtf((float)DKH);
  {
    const T* qp = base + (size_t)ic * g.ldq + n * DKH;
#pragma unroll
    for (int d = 0; d < DKH; d += 4) {
      const typename V4<T>::raw v = V4<T>::ld(qp + d);
#pragma unroll
      for (int e = 0; e < 4; ++e) q[d + e] = V4<T>::get(v, e) * scale;
    }
  }
  float dO[DVH], delta = 0.f;
  {
    const float* op = o + ((size_t)b * HW + ic) * g.dv + n * DVH;
    const float* dp = d_o + ((size_t)b * HW + ic) * g.dv + n * DVH;
#pragma unroll
    for (int d = 0; d < DVH; ++d) { dO[d] = qvalid ? dp[d] : 0.f; delta = fmaf(dO[d], op[d], delta); }
  }
  const float L = lse[(size_t)bn * HW + ic];
  __syncthreads();
  for (int ky = 0; ky < H; ++ky) {
    float a = 0.f;
#pragma unroll
    for (int d = 0; d < DKH; ++d) a = fmaf(q[d], RH[d * LH + ky - qy + H - 1], a);
    rh[tid * (H + 1) + ky] = a;
  }
  for (int kx = 0; kx < W; ++kx) {
    float a = 0.f;
#pragma unroll
    for (int d = 0; d < DKH; ++d) a = fmaf(q[d], RW[d * LW + kx - qx + W - 1], a);
    rw[tid * (W + 1) + kx] = a;
  }
  // per-query accumulators: dq (through k_j) and the row/column sums of dS (d rh_i[ky], d rw_i[kx]) kept in LDS
  // as a second half of the rh/rw rows would double LDS; instead accumulate d(rw) per kx in registers-free form:
  // d rh_i[ky] is final when the key row ky ends, d rw_i[kx] accumulates over rows in LDS (own row, no conflicts).
  float dq[DKH];
#pragma unroll
  for (int d = 0; d < DKH; ++d) dq[d] = 0.f;
  float* drw = Kt + TK * DKH + TK * DVH + DKH * (LH + LW);      // [AQ][W+1], behind dRW
  float* drh_s = drw + AQ * (W + 1);                            // [AQ][H+1]
  float* Qs = drh_s + AQ * (H + 1);                             // [AQ][DKH+1]
  for (int kx = 0; kx < W; ++kx) drw[tid * (W + 1) + kx] = 0.f;
  for (int ky = 0; ky < H; ++ky) drh_s[tid * (H + 1) + ky] = 0.f;
  const int kofs = g.dk + n * DKH, vofs = 2 * g.dk + n * DVH;
  float drh_run = 0.f;
  for (int j0 = 0; j0 < HW; j0 += TK) {
    __syncthreads();
    for (int t = tid; t < TK * 5; t += AQ) {
      const int j = t / 5, c = t - j * 5;
      const int jj = min(j0 + j, HW - 1);
      const typename V4<T>::raw v = V4<T>::ld(base + (size_t)jj * g.ldq + kofs + c * 4);
#pragma unroll
      for (int e = 0; e < 4; ++e) Kt[j * DKH + c * 4 + e] = V4<T>::get(v, e);
    }
    for (int t = tid; t < TK * DVH; t += AQ) {
      const int j = t / DVH, d = t - j * DVH;
      const int jj = min(j0 + j, HW - 1);
      Vt[t] = V4<T>::ld1(base + (size_t)jj * g.ldq + vofs + d);
    }
    __syncthreads();
    const int jn = min(TK, HW - j0);
    int ky = j0 / W, kx = j0 - ky * W;
#pragma unroll 4
    for (int j = 0; j < jn; ++j) {
      float s = rh[tid * (H + 1) + ky] + rw[tid * (W + 1) + kx];
      const float4* kp = reinterpret_cast<const float4*>(Kt + j * DKH);
      float4 kv[5];
#pragma unroll
      for (int c = 0; c < 5; ++c) {
        kv[c] = kp[c];
        s = fmaf(q[4 * c], kv[c].x, fmaf(q[4 * c + 1], kv[c].y, fmaf(q[4 * c + 2], kv[c].z, fmaf(q[4 * c + 3], kv[c].w, s))));
      }
      const float p = __expf(s - L);
      float dp = 0.f;
#pragma unroll
      for (int d = 0; d < DVH; ++d) dp = fmaf(dO[d], Vt[j * DVH + d], dp);
      const float ds = p * (dp - delta);
#pragma unroll
      for (int c = 0; c < 5; ++c) {
        dq[4 * c] = fmaf(ds, kv[c].x, dq[4 * c]);
        dq[4 * c + 1] = fmaf(ds, kv[c].y, dq[4 * c + 1]);
        dq[4 * c + 2] = fmaf(ds, kv[c].z, dq[4 * c + 2]);
        dq[4 * c + 3] = fmaf(ds, kv[c].w, dq[4 * c + 3]);
      }
      drh_run += ds;
      drw[tid * (W + 1) + kx] += ds;
      if (++kx == W) {
        // key row ky complete: fold d rh_i[ky] into dq and into the workgroup's dRH partial
        if (qvalid) {
          const int r = ky - qy + H - 1;
#pragma unroll
          for (int d = 0; d < DKH; ++d) {
            dq[d] = fmaf(drh_run, RH[d * LH + r], dq[d]);
          }
        }
        drh_s[tid * (H + 1) + ky] = qvalid ? drh_run : 0.f;      // d rh_i[ky]: folded into the table gradient after the key loop
        drh_run = 0.f;
        kx = 0;
        ++ky;
      }
    }
  }
  if (qvalid) {
    for (int kx = 0; kx < W; ++kx) {
      const float dsum = drw[tid * (W + 1) + kx];
      const int r = kx - qx + W - 1;
#pragma unroll
      for (int d = 0; d < DKH; ++d) dq[d] = fmaf(dsum, RW[d * LW + r], dq[d]);
    }
    float* dqp = dqkv + ((size_t)b * HW + i) * (2 * g.dk + g.dv) + n * DKH;
#pragma unroll
    for (int d = 0; d < DKH; ++d) dqp[d] = dq[d] * scale;       // q~ = q * scale
  } else {
    for (int kx = 0; kx < W; ++kx) drw[tid * (W + 1) + kx] = 0.f;
  }
#pragma unroll
  for (int d = 0; d < DKH; ++d) Qs[tid * (DKH + 1) + d] = q[d];
  __syncthreads();
  // table gradients, owner-computes (a fixed order of additions: LDS float atomics from many lanes are not): the thread that owns
  // word (d, r) walks the workgroup's queries; query l meets offset r at key row ky = r - (H-1) + qy_l
  const int i0 = blockIdx.x * AQ;
  for (int t = tid; t < DKH * LH; t += AQ) {
    const int d = t / LH, r = t - d * LH;
    int yq = i0 / W, xq = i0 - yq * W;
    float a = 0.f;
    for (int l = 0; l < AQ; ++l) {
      const int ky = r - (H - 1) + yq;
      if (ky >= 0 && ky < H) a = fmaf(drh_s[l * (H + 1) + ky], Qs[l * (DKH + 1) + d], a);
      if (++xq == W) { xq = 0; ++yq; }
    }
    dRH[t] = a;
  }
  for (int t = tid; t < DKH * LW; t += AQ) {
    const int d = t / LW, r = t - d * LW;
    int xq = i0 % W;
    float a = 0.f;
    for (int l = 0; l < AQ; ++l) {
      const int kx = r - (W - 1) + xq;
      if (kx >= 0 && kx < W) a = fmaf(drw[l * (W + 1) + kx], Qs[l * (DKH + 1) + d], a);
      if (++xq == W) xq = 0;
    }
    dRW[t] = a;
  }
  __syncthreads();
  const size_t wg = (size_t)blockIdx.y * gridDim.x + blockIdx.x;
  for (int t = tid; t < DKH * LH; t += AQ) { if (slab_h) slab_h[wg * (DKH * LH) + t] = dRH[t]; else atomicAdd(&d_rel_h[t], dRH[t]); }
  for (int t = tid; t < DKH * LW; t += AQ) { if (slab_w) slab_w[wg * (DKH * LW) + t] = dRW[t]; else atomicAdd(&d_rel_w[t], dRW[t]); }
}

template <typename T, int DVH>
__global__ __launch_bounds__(AQ) void aa_attn_bwd_k_kernel(const T* __restrict__ qkv, const float* __restrict__ rel_h,
                                                          const float* __restrict__ rel_w, const float* __restrict__ o,
                                                          const float* __restrict__ d_o, const float* __restrict__ lse,
                                                          float* __restrict__ dqkv, const AAGeo g) {
  // one lane per KEY j; queries stream through LDS: q~_i, dO_i, delta_i, lse_i.  S_ij needs the relative terms
  // q~_i . (RH[:, ky-qy+H-1] + RW[:, kx-qx+W-1]): fold them into the key: k'_j(i) is query dependent, so instead
  // use S_ij = q~_i . k_j + rhT_j[qy] + rwT_j[qx] with rhT_j[qy] = q~_i . RH[:, ky-qy+H-1] -- still query dependent.
  // => stage per query tile the two logit rows' entries for THIS key row/column: (rh_i[ky], rw_i[kx]) differ per key,
  // so each lane recomputes the 2 dot products with its own offsets: 2 x 20 FMA extra per pair.
  extern __shared__ __attribute__((aligned(16))) float lds[];
  const int H = g.H, W = g.W, HW = H * W;
  const int LH = 2 * H - 1, LW = 2 * W - 1;
  float* RH = lds;
  float* RW = RH + DKH * LH;
  float* Qt = RW + DKH * LW;             // [TK][DKH] scaled queries
  float* Dt = Qt + TK * DKH;             // [TK][DVH] dO
  float* Et = Dt + TK * DVH;             // [TK][2]   delta, lse
  const int tid = threadIdx.x;
  const int bn = blockIdx.y, b = bn / g.nh, n = bn - b * g.nh;
  const int j = blockIdx.x * AQ + tid;
  const bool kvalid = j < HW;
  const int jc = kvalid ? j : HW - 1;
  const int ky = jc / W, kx = jc - ky * W;
  const T* base = qkv + (size_t)b * HW * g.ldq;
  for (int t = tid; t < DKH * LH; t += AQ) RH[t] = rel_h[t];
  for (int t = tid; t < DKH * LW; t += AQ) RW[t] = rel_w[t];
  float k[DKH], v[DVH], dk[DKH], dv[DVH];
  {
    const T* kp = base + (size_t)jc * g.ldq + g.dk + n * DKH;
#pragma unroll
    for (int d = 0; d < DKH; d += 4) {
      const typename V4<T>::raw u = V4<T>::ld(kp + d);
#pragma unroll
      for (int e = 0; e < 4; ++e) k[d + e] = V4<T>::get(u, e);
    }
#pragma unroll
    for (int d = 0; d < DVH; ++d) v[d] = V4<T>::ld1(base + (size_t)jc * g.ldq + 2 * g.dk + n * DVH + d);
  }
#pragma unroll
  for (int d = 0; d < DKH; ++d) dk[d] = 0.f;
#pragma unroll
  for (int d = 0; d < DVH; ++d) dv[d] = 0.f;
  const float scale = rsqrtf((float)DKH);
  for (int i0 = 0; i0 < HW; i0 += TK) {
    __syncthreads();
    for (int t = tid; t < TK * 5; t += AQ) {
      const int ii = t / 5, c = t - ii * 5;
      const int iq = min(i0 + ii, HW - 1);
      const typename V4<T>::raw u = V4<T>::ld(base + (size_t)iq * g.ldq + n * DKH + c * 4);
#pragma unroll
      for (int e = 0; e < 4; ++e) Qt[ii * DKH + c * 4 + e] = V4<T>::get(u, e) * scale;
    }
    for (int t = tid; t < TK; t += AQ) {
      const int iq = min(i0 + t, HW - 1);
      const bool ok = i0 + t < HW;
      float de = 0.f;
#pragma unroll
      for (int d = 0; d < DVH; ++d) {
        const float dd = ok ? d_o[((size_t)b * HW + iq) * g.dv + n * DVH + d] : 0.f;
        Dt[t * DVH + d] = dd;
        de = fmaf(dd, o[((size_t)b * HW + iq) * g.dv + n * DVH + d], de);
      }
      Et[2 * t] = de;
      Et[2 * t + 1] = ok ? lse[(size_t)bn * HW + iq] : 3.0e38f;      // p = exp(s - inf) = 0 for padding queries
    }
    __syncthreads();
    const int in_ = min(TK, HW - i0);
    int qy = i0 / W, qx = i0 - qy * W;
    for (int ii = 0; ii < in_; ++ii) {
      const float* qp = Qt + ii * DKH;
      const int rhh = ky - qy + H - 1, rww = kx - qx + W - 1;
      float s = 0.f;
#pragma unroll
      for (int d = 0; d < DKH; ++d) s = fmaf(qp[d], k[d] + RH[d * LH + rhh] + RW[d * LW + rww], s);
      const float p = __expf(s - Et[2 * ii + 1]);
      float dp = 0.f;
#pragma unroll
      for (int d = 0; d < DVH; ++d) {
        dp = fmaf(Dt[ii * DVH + d], v[d], dp);
        dv[d] = fmaf(p, Dt[ii * DVH + d], dv[d]);
      }
      const float ds = p * (dp - Et[2 * ii]);
#pragma unroll
      for (int d = 0; d < DKH; ++d) dk[d] = fmaf(ds, qp[d], dk[d]);
      if (++qx == W) { qx = 0; ++qy; }
    }
  }
  if (kvalid) {
    float* dp = dqkv + ((size_t)b * HW + j) * (2 * g.dk + g.dv);
#pragma unroll
    for (int d = 0; d < DKH; ++d) dp[g.dk + n * DKH + d] = dk[d];
#pragma unroll
    for (int d = 0; d < DVH; ++d) dp[2 * g.dk + n * DVH + d] = dv[d];
  }
}

// ---------------------------------------------------------------------------------------------- elementwise glue
// per-(b,c) affine + ReLU (InstanceNorm2d + ReLU ahead of the AAConv2d, attn_aug_conv.py:438-439)
template <typename T>
__global__ void affine_relu_bc_kernel(const T* __restrict__ x, const float* __restrict__ sc, const float* __restrict__ sh,
                                      T* __restrict__ y, int HW, int C, int ldx, size_t total) {
  const int CP = C / 8;
  for (size_t idx = (size_t)blockIdx.x * blockDim.x + threadIdx.x; idx < total; idx += (size_t)gridDim.x * blockDim.x) {
    const int cq = idx % CP;
    const size_t pix = idx / CP;
    const int b = pix / HW;
    typename V8<T>::raw v;
    float o_f[8];
    v = V8<T>::ld(x + pix * ldx + cq * 8);
    const float* s = sc + (size_t)b * C + cq * 8;
    const float* h = sh + (size_t)b * C + cq * 8;
#pragma unroll
    for (int j = 0; j < 8; ++j) o_f[j] = V8<T>::rnd(fmaxf(fmaf(V8<T>::get(v, j), s[j], h[j]), 0.f));
    V8<T>::st(y + idx * 8, o_f);
  }
}

// per-(b,c) sums over the pixels of an image: sum, sum of squares (InstanceNorm statistics).
// Deterministic: a workgroup owns (image b, a group of 8 channel chunks = 64 channels) and ALL pixels of the image -- 32 pixel lanes x
// 8 chunk lanes, four pixels in flight per thread; the 32 pixel-lane partial sums meet in LDS and are added in lane order; one
// plain store per (b, c): no atomics, no zero-fill, the same bits every run.
template <typename F>
__device__ __forceinline__ void bc_fold_store(float (*part)[8][17], const float (&s1)[8], const float (&s2)[8], float* __restrict__ o1,
                                              float* __restrict__ o2, int b, int C, int cbase, F) {
  const int cq = threadIdx.x & 7, rr = threadIdx.x >> 3;
#pragma unroll
  for (int j = 0; j < 8; ++j) { part[rr][cq][j] = s1[j]; part[rr][cq][8 + j] = s2[j]; }
  __syncthreads();
  if (threadIdx.x < 128) {
    const int c8 = threadIdx.x >> 4, k = threadIdx.x & 15;       // chunk lane, (sum | sq) x channel-in-chunk
    float t = 0.f;
#pragma unroll 8
    for (int r = 0; r < 32; ++r) t += part[r][c8][k];
    const int c = cbase + c8 * 8 + (k & 7);
    if (c < C) (k < 8 ? o1 : o2)[(size_t)b * C + c] = t;
  }
}

template <typename T>
__global__ __launch_bounds__(256) void stats_bc_kernel(const T* __restrict__ x, float* __restrict__ sum, float* __restrict__ sq,
                                                       int HW, int C, int ldx) {
  __shared__ float part[32][8][17];
  const int b = blockIdx.y, cbase = blockIdx.x * 64;
  const int cq = threadIdx.x & 7, rr = threadIdx.x >> 3;
  const int c0 = cbase + cq * 8;
  const bool cok = c0 < C;
  const T* xp = x + (size_t)b * HW * ldx + (cok ? c0 : 0);
  float s1[8], s2[8];
#pragma unroll
  for (int j = 0; j < 8; ++j) s1[j] = s2[j] = 0.f;
  int p = rr;
  for (; p + 96 < HW; p += 128) {
    typename V8<T>::raw v[4];
#pragma unroll
    for (int u = 0; u < 4; ++u) v[u] = V8<T>::ld(xp + (size_t)(p + 32 * u) * ldx);
#pragma unroll
    for (int u = 0; u < 4; ++u)
#pragma unroll
      for (int j = 0; j < 8; ++j) { const float f = V8<T>::get(v[u], j); s1[j] += f; s2[j] += f * f; }
  }
  for (; p < HW; p += 32) {
    typename V8<T>::raw v;
    v = V8<T>::ld(xp + (size_t)p * ldx);
#pragma unroll
    for (int j = 0; j < 8; ++j) { const float f = V8<T>::get(v, j); s1[j] += f; s2[j] += f * f; }
  }
  if (!cok) {
#pragma unroll
    for (int j = 0; j < 8; ++j) s1[j] = s2[j] = 0.f;
  }
  bc_fold_store(part, s1, s2, sum, sq, b, C, cbase, 0);
}

// out_proj (dv x dv 1x1 conv, :92) on the fp32 attention output, written as bf16 into the block-buffer slice
// [+ per-channel statistics of the rounded output].  TA = (256 / dv) * dv threads are active: a thread keeps ONE output channel
// (tid % dv) and walks pixels, so its two sums are registers; they meet in LDS and are added in pixel-lane order.  det: the
// workgroup plain-stores its row (stat_sum[row * rstride + c], CxConv.stat_det convention), else one atomic per channel.
template <typename T, int DM>
__global__ __launch_bounds__(256) void aa_outproj_fwd_kernel(const float* __restrict__ o, const float* __restrict__ w, T* __restrict__ y,
                                                             int ldy, float* stat_sum, float* stat_sq, size_t npix, int dv, int TA, int det,
                                                             int rstride) {
  __shared__ float ws[DM * DM];          // DM = 64, or 104 for the 72- / 104-channel out-projections of the CIFAR Densenet-BC at v = 0.7
  __shared__ float st[2][256];
  const int tid = threadIdx.x;
  for (int t = tid; t < dv * dv; t += blockDim.x) ws[t] = w[t];
  __syncthreads();
  const bool active = tid < TA;
  const int c = tid % dv, pl = tid / dv, npl = TA / dv;
  float s1 = 0.f, s2 = 0.f;
  if (active) {
    for (size_t pix = (size_t)blockIdx.x * npl + pl; pix < npix; pix += (size_t)gridDim.x * npl) {
      const float* op = o + pix * dv;
      float a = 0.f;
      for (int d = 0; d < dv; ++d) a = fmaf(ws[c * dv + d], op[d], a);
      const float rv = V8<T>::rnd(a);
      V4<T>::st1(y + pix * ldy + c, rv);
      s1 += rv;
      s2 += rv * rv;
    }
  }
  st[0][tid] = s1;
  st[1][tid] = s2;
  __syncthreads();
  if (stat_sum && tid < dv) {
    float t1 = 0.f, t2 = 0.f;
    for (int l = 0; l < npl; ++l) { t1 += st[0][l * dv + tid]; t2 += st[1][l * dv + tid]; }
    if (det) {
      stat_sum[(size_t)blockIdx.x * rstride + tid] = t1;
      stat_sq[(size_t)blockIdx.x * rstride + tid] = t2;
    } else {
      atomicAdd(&stat_sum[tid], t1);
      atomicAdd(&stat_sq[tid], t2);
    }
  }
}

// backward of out_proj: dO[pix][d] = sum_c dY[pix][c] * W[c][d];  dW[c][d] += sum_pix dY[pix][c] * O[pix][d]
// dY = g*ga + gx*gb + gc (deferred BN correction of the gradient-buffer slice)
template <typename T, int DM, int CH>
__global__ __launch_bounds__(256) void aa_outproj_bwd_kernel(const T* __restrict__ g, int ldg, const T* __restrict__ gx, int ldgx,
                                                             const float* __restrict__ ga, const float* __restrict__ gb,
                                                             const float* __restrict__ gc, const float* __restrict__ o,
                                                             const float* __restrict__ w, float* __restrict__ d_o,
                                                             float* __restrict__ dw, float* __restrict__ slab, size_t npix, int dv) {
  // Two small GEMMs per 64-pixel chunk staged in LDS: dO = dY W (thread per (pixel, d)) and dW += dY^T O (thread per (c, d)
  // pair, which it owns: plain LDS accumulation, no atomics -- a pixel-per-thread outer product sent 64 lanes to the same
  // LDS word dv*dv times per pixel: 2.2 ms per call).
  constexpr int PT = DM + 1;                           // CH pixels per chunk, padded row pitch (dv <= DM): <48, 64> or <64, 32> (64 KB of LDS)
  __shared__ float ws[DM * DM];
  __shared__ float dws[DM * DM];
  __shared__ float dyS[CH * PT];
  __shared__ float oS[CH * PT];
  const int tid = threadIdx.x;
  for (int t = tid; t < dv * dv; t += 256) { ws[t] = w[t]; dws[t] = 0.f; }
  for (size_t p0 = (size_t)blockIdx.x * CH; p0 < npix; p0 += (size_t)gridDim.x * CH) {
    __syncthreads();                                   // previous chunk consumed (first time: ws / dws initialised)
    for (int idx = tid; idx < CH * dv; idx += 256) {
      const int px = idx / dv, c = idx - px * dv;
      const size_t pix = p0 + px;
      const bool ok = pix < npix;
      dyS[px * PT + c] = ok ? fmaf(V4<T>::ld1(g + pix * ldg + c), ga[c], fmaf(V4<T>::ld1(gx + pix * ldgx + c), gb[c], gc[c])) : 0.f;
      oS[px * PT + c] = ok ? o[pix * dv + c] : 0.f;
    }
    __syncthreads();
    for (int idx = tid; idx < CH * dv; idx += 256) {
      const int px = idx / dv, d = idx - px * dv;
      float a = 0.f;
      for (int c = 0; c < dv; ++c) a = fmaf(dyS[px * PT + c], ws[c * dv + d], a);
      if (p0 + px < npix) d_o[(p0 + px) * dv + d] = a;
    }
    for (int pair = tid; pair < dv * dv; pair += 256) {
      const int c = pair / dv, d = pair - c * dv;
      float a = 0.f;
#pragma unroll 8
      for (int px = 0; px < CH; ++px) a = fmaf(dyS[px * PT + c], oS[px * PT + d], a);
      dws[pair] += a;
    }
  }
  __syncthreads();
  for (int t = tid; t < dv * dv; t += 256) dw_out(dw, slab, (size_t)dv * dv, (int)blockIdx.x, t, dws[t]);
}

// The same for 64 < dv <= 104 (Densenet-BC transitions of the CIFAR harness at v = 0.7: dv = 72 / 104): the dv x dv weight-gradient
// sums do not fit LDS beside the weights, so a thread keeps its (c, d) pairs -- pair = tid + 256 i -- in registers.
template <typename T>
__global__ __launch_bounds__(256) void aa_outproj_bwd_big_kernel(const T* __restrict__ g, int ldg, const T* __restrict__ gx, int ldgx,
                                                                 const float* __restrict__ ga, const float* __restrict__ gb,
                                                                 const float* __restrict__ gc, const float* __restrict__ o,
                                                                 const float* __restrict__ w, float* __restrict__ d_o,
                                                                 float* __restrict__ dw, float* __restrict__ slab, size_t npix, int dv) {
  constexpr int DM = 104, CH = 16, PT = DM + 1, NP = (DM * DM + 255) / 256;
  __shared__ float ws[DM * DM];
  __shared__ float dyS[CH * PT];
  __shared__ float oS[CH * PT];
  const int tid = threadIdx.x;
  float acc[NP];
#pragma unroll
  for (int i = 0; i < NP; ++i) acc[i] = 0.f;
  for (int t = tid; t < dv * dv; t += 256) ws[t] = w[t];
  for (size_t p0 = (size_t)blockIdx.x * CH; p0 < npix; p0 += (size_t)gridDim.x * CH) {
    __syncthreads();
    for (int idx = tid; idx < CH * dv; idx += 256) {
      const int px = idx / dv, c = idx - px * dv;
      const size_t pix = p0 + px;
      const bool ok = pix < npix;
      dyS[px * PT + c] = ok ? fmaf(V4<T>::ld1(g + pix * ldg + c), ga[c], fmaf(V4<T>::ld1(gx + pix * ldgx + c), gb[c], gc[c])) : 0.f;
      oS[px * PT + c] = ok ? o[pix * dv + c] : 0.f;
    }
    __syncthreads();
    for (int idx = tid; idx < CH * dv; idx += 256) {
      const int px = idx / dv, d = idx - px * dv;
      float a = 0.f;
      for (int c = 0; c < dv; ++c) a = fmaf(dyS[px * PT + c], ws[c * dv + d], a);
      if (p0 + px < npix) d_o[(p0 + px) * dv + d] = a;
    }
#pragma unroll
    for (int i = 0; i < NP; ++i) {
      const int pair = tid + 256 * i;
      if (pair < dv * dv) {
        const int c = pair / dv, d = pair - c * dv;
        float a = 0.f;
#pragma unroll
        for (int px = 0; px < CH; ++px) a = fmaf(dyS[px * PT + c], oS[px * PT + d], a);
        acc[i] += a;
      }
    }
  }
#pragma unroll
  for (int i = 0; i < NP; ++i) {
    const int pair = tid + 256 * i;
    if (pair < dv * dv) dw_out(dw, slab, (size_t)dv * dv, (int)blockIdx.x, pair, acc[i]);
  }
}

// fp32 (B,HW,C) -> bf16 same shape
__global__ void f32_to_bf16_kernel(const float* __restrict__ x, bf16* __restrict__ y, size_t n) {
  for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (size_t)gridDim.x * blockDim.x) y[i] = f2bf(x[i]);
}

// InstanceNorm + ReLU backward: dz = dA * [a > 0];  dx = r * (dz - mean_hw(dz) - xhat * mean_hw(dz * xhat)) per (b,c)
// pass 1: S1[b][c] = sum dz, S2[b][c] = sum dz*xhat      pass 2: write dx
template <typename T>
__global__ __launch_bounds__(256) void in_relu_bwd_stats_kernel(const T* __restrict__ da, const T* __restrict__ x,
                                                                const float* __restrict__ sc, const float* __restrict__ sh,
                                                                float* __restrict__ S1, float* __restrict__ S2, int HW, int C, int ldx) {
  // same ownership as stats_bc_kernel: (image, 64 channels) per workgroup, every pixel, ordered fold, plain stores
  __shared__ float part[32][8][17];
  const int b = blockIdx.y, cbase = blockIdx.x * 64;
  const int cq = threadIdx.x & 7, rr = threadIdx.x >> 3;
  const int c0 = cbase + cq * 8;
  const bool cok = c0 < C;
  const int cc = cok ? c0 : 0;
  float s1[8], s2[8], fs[8], fh[8];
#pragma unroll
  for (int j = 0; j < 8; ++j) { s1[j] = s2[j] = 0.f; fs[j] = sc[(size_t)b * C + cc + j]; fh[j] = sh[(size_t)b * C + cc + j]; }
  const T* xp = x + (size_t)b * HW * ldx + cc;
  const T* dp = da + (size_t)b * HW * C + cc;
  int p = rr;
  for (; p + 32 < HW; p += 64) {
    typename V8<T>::raw v[2], d[2];
#pragma unroll
    for (int u = 0; u < 2; ++u) {
      v[u] = V8<T>::ld(xp + (size_t)(p + 32 * u) * ldx);
      d[u] = V8<T>::ld(dp + (size_t)(p + 32 * u) * C);
    }
#pragma unroll
    for (int u = 0; u < 2; ++u)
#pragma unroll
      for (int j = 0; j < 8; ++j) {
        const float xh = fmaf(V8<T>::get(v[u], j), fs[j], fh[j]);          // xhat = (x-mean)*rstd
        const float dz = xh > 0.f ? V8<T>::get(d[u], j) : 0.f;
        s1[j] += dz;
        s2[j] += dz * xh;
      }
  }
  for (; p < HW; p += 32) {
    typename V8<T>::raw v, d;
    v = V8<T>::ld(xp + (size_t)p * ldx);
    d = V8<T>::ld(dp + (size_t)p * C);
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      const float xh = fmaf(V8<T>::get(v, j), fs[j], fh[j]);
      const float dz = xh > 0.f ? V8<T>::get(d, j) : 0.f;
      s1[j] += dz;
      s2[j] += dz * xh;
    }
  }
  if (!cok) {
#pragma unroll
    for (int j = 0; j < 8; ++j) s1[j] = s2[j] = 0.f;
  }
  bc_fold_store(part, s1, s2, S1, S2, b, C, cbase, 0);
}

template <typename T>
__global__ void in_relu_bwd_apply_kernel(const T* __restrict__ da, const T* __restrict__ x, const float* __restrict__ sc,
                                         const float* __restrict__ sh, const float* __restrict__ S1, const float* __restrict__ S2,
                                         T* __restrict__ gout, int HW, int C, int ldx, int ldg, size_t total) {
  const int CP = C / 8;
  const float inv = 1.f / HW;
  for (size_t idx = (size_t)blockIdx.x * blockDim.x + threadIdx.x; idx < total; idx += (size_t)gridDim.x * blockDim.x) {
    const int cq = idx % CP;
    const size_t pix = idx / CP;
    const int b = pix / HW;
    typename V8<T>::raw v, d;
    float o_f[8];
    v = V8<T>::ld(x + pix * ldx + cq * 8);
    d = V8<T>::ld(da + pix * C + cq * 8);
    const size_t bc = (size_t)b * C + cq * 8;
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      const float r = sc[bc + j];
      const float xh = fmaf(V8<T>::get(v, j), r, sh[bc + j]);
      const float dz = xh > 0.f ? V8<T>::get(d, j) : 0.f;
      o_f[j] = V8<T>::rnd(r * (dz - S1[bc + j] * inv - xh * S2[bc + j] * inv));
    }
    V8<T>::st(gout + pix * ldg + cq * 8, o_f);
  }
}

inline int grid_for(size_t n, int block, int cap) {
  size_t gsz = (n + block - 1) / block;
  if (gsz > (size_t)cap) gsz = cap;
  if (gsz < 1) gsz = 1;
  return (int)gsz;
}

inline size_t attn_lds_floats(int H, int W, int dvh) { return (size_t)DKH * (2 * H - 1 + 2 * W - 1) + (size_t)AQ * (H + W + 2) + TK * (DKH + dvh); }

// Every dv/nh the generic kernels are instantiated for (1 .. MAXDV).  The forward and the backward launcher expand their dispatch
// switch from this one list, and the backward's case raises the LDS limit of the instance it launches, so the set of instances
// that can be launched and the set that may ask for more than 64 KB are the same set by construction.
#define AA_DVH_LIST(X) X(1) X(2) X(3) X(4) X(5) X(6) X(7) X(8) X(9) X(10) X(11) X(12) X(13)
constexpr size_t AA_LDS_DEFAULT = 64 * 1024;       // dynamic LDS a kernel may ask for without hipFuncSetAttribute
constexpr size_t AA_LDS_BWD_Q = 160 * 1024;        // what the query side of the backward is allowed (the CU's LDS)

template <typename T> constexpr const char* aa_tname() { return std::is_same<T, bf16>::value ? "bf16" : "f32"; }

// the contract every launcher states for qkv: rows of ldq elements holding [q dk | k dk | v dv], read in chunks of four elements
// (8 bytes of bf16, 16 bytes of fp32: V4<T>::ld), so the pitch is a multiple of four elements
inline bool aa_qkv_shape(int B, int H, int W, int nh, int dk, int dv, int ldq) {
  return B > 0 && H > 0 && W > 0 && nh > 0 && dk > 0 && dv >= 0 && dk % nh == 0 && dv % nh == 0 && ldq % 4 == 0 && ldq >= 2 * dk + dv;
}

}  // namespace

// ---- launchers, templated on the storage type (bf16 / the fp32 parity mode)
template <typename T>
static inline const void* as_qkv(const void* p) { return p; }

template <typename T>
int aa_attention_fwd_t(const void* qkv, const float* rel_h, const float* rel_w, float* o, float* lse, int B, int H, int W, int nh,
                        int dk, int dv, int ldq, void* stream) {
  if (!qkv || !rel_h || !rel_w || !o || !lse) return CX_EINVAL;
  if (!aa_qkv_shape(B, H, W, nh, dk, dv, ldq)) return CX_ESHAPE;
  hipStream_t st = as_stream(stream);
  if (dk != nh * DKH || dv / nh > MAXDV)            // other head widths: aaconv_heads.hip (CX_ESHAPE beyond dk/nh, dv/nh <= 64, dv <= 104)
    return cx_aa_heads_fwd(!std::is_same<T, bf16>::value, qkv, rel_h, rel_w, o, lse, B, H, W, nh, dk, dv, ldq, st);
  const int dvh = dv / nh;
  AAGeo g{B, H, W, nh, dk, dv, ldq};
  {
    bool handled = false;
    const int rc = !std::is_same<T, bf16>::value ? 0 : cx_try_aa_row(0, qkv, rel_h, rel_w, o, nullptr, lse, nullptr, nullptr, nullptr, nullptr, nullptr, B, H, W, nh, dk, dv,
                                 ldq, st, &handled);
    if (handled) return rc;
  }
  const size_t smem = attn_lds_floats(H, W, dvh) * 4;
  if (smem > AA_LDS_DEFAULT) return CX_ESHAPE;          // no instance asks for more than the default limit: no attribute to raise
  dim3 grid((H * W + AQ - 1) / AQ, B * nh);
  // (5, 7, 10, 11, 12: value ratios the reference's configurations do not use; generic kernels only)
#define AA_CASE(D)                                                                                                            \
    case D:                                                                                                                   \
      hipLaunchKernelGGL((aa_attn_fwd_kernel<T, D>), grid, dim3(AQ), smem, st, (const T*)qkv, rel_h, rel_w, o, lse, g);       \
      break;
  switch (dvh) {
    AA_DVH_LIST(AA_CASE)
    default: return CX_EUNSUPPORTED;
  }
#undef AA_CASE
  CX_KTAG("aa_fwd<%s,%d>", aa_tname<T>(), dvh);
  return launch_status();
}

template <typename T>
int aa_attention_weights_t(const void* qkv, const float* rel_h, const float* rel_w, const float* lse, float* weights, int B, int H,
                            int W, int nh, int dk, int dv, int ldq, void* stream) {
  if (!qkv || !rel_h || !rel_w || !lse || !weights) return CX_EINVAL;
  if (!aa_qkv_shape(B, H, W, nh, dk, dv, ldq)) return CX_ESHAPE;
  if (dk != nh * DKH)
    return cx_aa_heads_weights(!std::is_same<T, bf16>::value, qkv, rel_h, rel_w, lse, weights, B, H, W, nh, dk, dv, ldq, as_stream(stream));
  AAGeo g{B, H, W, nh, dk, dv, ldq};
  const size_t smem = attn_lds_floats(H, W, 0) * 4;
  if (smem > AA_LDS_DEFAULT) return CX_ESHAPE;
  hipLaunchKernelGGL(aa_attn_weights_kernel<T>, dim3((H * W + AQ - 1) / AQ, B * nh), dim3(AQ), smem, as_stream(stream),
                     (const T*)qkv, rel_h, rel_w, lse, weights, g);
  CX_KTAG("aa_weights<%s>", aa_tname<T>());
  return launch_status();
}

template <typename T>
int aa_attention_bwd_t(const void* qkv, const float* rel_h, const float* rel_w, const float* o, const float* d_o, const float* lse,
                        float* dqkv, float* d_rel_h, float* d_rel_w, int B, int H, int W, int nh, int dk, int dv, int ldq,
                        float* scratch, int64_t scratch_floats, void* stream) {
  if (!qkv || !rel_h || !rel_w || !o || !d_o || !lse || !dqkv || !d_rel_h || !d_rel_w) return CX_EINVAL;
  if (!aa_qkv_shape(B, H, W, nh, dk, dv, ldq)) return CX_ESHAPE;
  hipStream_t st = as_stream(stream);
  // Reproducible relative-table gradients: every query-side workgroup plain-stores its two partial tables into the caller's
  // workspace (one slab per workgroup: 128 queries of one (image, head)) and the slabs are added in workgroup order afterwards.
  // Without (enough) workspace the partial tables are added with fp32 atomics, whose order changes from run to run.
  const int dkh = dk / nh;
  const int TH = dkh * (2 * H - 1), TW = dkh * (2 * W - 1);
  const long long nwg = (long long)((H * W + 127) / 128) * B * nh;        // AQ = AQM = 128 queries per workgroup in every q-side kernel
  float *slab_h = nullptr, *slab_w = nullptr;
  if (scratch && nwg * (TH + TW) <= scratch_floats && nwg < (1ll << 30)) {
    slab_h = scratch;
    slab_w = scratch + nwg * TH;
  }
  if (dk != nh * DKH || dv / nh > MAXDV) {          // other head widths: aaconv_heads.hip, same slab protocol
    if (const int e = cx_aa_heads_bwd(!std::is_same<T, bf16>::value, qkv, rel_h, rel_w, o, d_o, lse, dqkv, d_rel_h, d_rel_w, slab_h, slab_w,
                                      B, H, W, nh, dk, dv, ldq, st)) return e;
    if (slab_h) {
      if (const int e = cx_rows_reduce_add_impl(d_rel_h, slab_h, (int)nwg, TH, TH, st)) return e;
      return cx_rows_reduce_add_impl(d_rel_w, slab_w, (int)nwg, TW, TW, st);
    }
    return 0;
  }
  const int dvh = dv / nh;
  AAGeo g{B, H, W, nh, dk, dv, ldq};
  const size_t smem_q = (attn_lds_floats(H, W, dvh) + (size_t)DKH * (2 * H - 1 + 2 * W - 1) + (size_t)AQ * (W + 1) + (size_t)AQ * (H + 1) +
                         (size_t)AQ * (DKH + 1)) * 4;
  const size_t smem_k = ((size_t)DKH * (2 * H - 1 + 2 * W - 1) + TK * (DKH + dvh + 2)) * 4;
  dim3 grid((H * W + AQ - 1) / AQ, B * nh);
  bool row_q = false;
  {
    const int rc = !std::is_same<T, bf16>::value ? 0 : cx_try_aa_row(1, qkv, rel_h, rel_w, const_cast<float*>(o), d_o, const_cast<float*>(lse), dqkv, d_rel_h, d_rel_w, slab_h,
                                 slab_w, B, H, W, nh, dk, dv, ldq, st, &row_q);
    if (row_q && rc) return rc;          // dq, dk, dv and the table partials all done there
  }
  if (!row_q) {
    if (smem_q > AA_LDS_BWD_Q || smem_k > AA_LDS_DEFAULT) return CX_ESHAPE;
    // smem_q passes the 64 KB default from H + W = 35 on: the case that launches an instance is also what raises that instance's
    // limit, once (a host-side attribute: nothing is queued on the stream)
#define AA_CASE(D)                                                                                                             \
    case D: {                                                                                                                  \
      static const bool attr = ((void)hipFuncSetAttribute(reinterpret_cast<const void*>(&aa_attn_bwd_q_kernel<T, D>),          \
                                                          hipFuncAttributeMaxDynamicSharedMemorySize, (int)AA_LDS_BWD_Q), true); \
      (void)attr;                                                                                                              \
      hipLaunchKernelGGL((aa_attn_bwd_q_kernel<T, D>), grid, dim3(AQ), smem_q, st, (const T*)qkv, rel_h, rel_w, o, d_o, lse, dqkv, \
                         d_rel_h, d_rel_w, slab_h, slab_w, g);                                                                 \
      hipLaunchKernelGGL((aa_attn_bwd_k_kernel<T, D>), grid, dim3(AQ), smem_k, st, (const T*)qkv, rel_h, rel_w, o, d_o, lse, dqkv, g); \
    } break;
    switch (dvh) {
      AA_DVH_LIST(AA_CASE)
      default: return CX_EUNSUPPORTED;
    }
#undef AA_CASE
    CX_KTAG("aa_bwd<%s,%d>", aa_tname<T>(), dvh);
    if (const int e = launch_status()) return e;
  }
  if (slab_h) {
    if (const int e = cx_rows_reduce_add_impl(d_rel_h, slab_h, (int)nwg, TH, TH, st)) return e;
    return cx_rows_reduce_add_impl(d_rel_w, slab_w, (int)nwg, TW, TW, st);
  }
  return 0;
}

template <typename T>
int stats_bc_t(const void* x, float* sum, float* sq, int B, int HW, int C, int ldx, void* stream) {
  if (!x || !sum || !sq || C % 8 || C > 2048 || ldx % 8) return CX_EINVAL;
  hipLaunchKernelGGL(stats_bc_kernel<T>, dim3((C + 63) / 64, B), dim3(256), 0, as_stream(stream), (const T*)x, sum, sq, HW, C, ldx);
  return launch_status();
}

template <typename T>
int affine_relu_bc_t(const void* x, const float* sc, const float* sh, void* y, int B, int HW, int C, int ldx, void* stream) {
  if (!x || !sc || !sh || !y || C % 8 || ldx % 8) return CX_EINVAL;
  const size_t total = (size_t)B * HW * (C / 8);
  hipLaunchKernelGGL(affine_relu_bc_kernel<T>, dim3(grid_for(total, 256, 8192)), dim3(256), 0, as_stream(stream), (const T*)x, sc, sh,
                     (T*)y, HW, C, ldx, total);
  return launch_status();
}

template <typename T>
int aa_outproj_fwd_t(const float* o, const float* w, void* y, int ldy, float* stat_sum, float* stat_sq, size_t npix, int dv,
                      int stat_rows, int stat_rstride, void* stream) {
  if (!o || !w || !y || dv <= 0 || dv > 104) return CX_EINVAL;
  if ((stat_sum == nullptr) != (stat_sq == nullptr)) return CX_EINVAL;
  if (stat_rows > 0 && (!stat_sum || stat_rstride < dv)) return CX_EINVAL;
  const int TA = 256 / dv * dv;
  int grid = grid_for(npix * dv, 256, 2048);
  if (stat_rows > 0) { if (grid > stat_rows) grid = stat_rows; cx_tl_stat_rows = grid; }
  if (dv <= 64)
    hipLaunchKernelGGL((aa_outproj_fwd_kernel<T, 64>), dim3(grid), dim3(256), 0, as_stream(stream), o, w, (T*)y, ldy, stat_sum, stat_sq, npix,
                       dv, TA, stat_rows > 0 ? 1 : 0, stat_rstride);
  else
    hipLaunchKernelGGL((aa_outproj_fwd_kernel<T, 104>), dim3(grid), dim3(256), 0, as_stream(stream), o, w, (T*)y, ldy, stat_sum, stat_sq, npix,
                       dv, TA, stat_rows > 0 ? 1 : 0, stat_rstride);
  return launch_status();
}

template <typename T>
int aa_outproj_bwd_t(const void* g, int ldg, const void* gx, int ldgx, const float* ga, const float* gb, const float* gc,
                      const float* o, const float* w, float* d_o, float* dw, size_t npix, int dv, float* scratch, int64_t scratch_floats,
                      void* stream) {
  if (!g || !gx || !ga || !gb || !gc || !o || !w || !d_o || !dw || dv <= 0 || dv > 104) return CX_EINVAL;
  const int grid = grid_for(npix, 64, 1024);
  float* slab = dw_slab(scratch, scratch_floats, grid, (long long)dv * dv);
  if (dv > 64)
    hipLaunchKernelGGL((aa_outproj_bwd_big_kernel<T>), dim3(grid), dim3(256), 0, as_stream(stream), (const T*)g, ldg, (const T*)gx, ldgx,
                       ga, gb, gc, o, w, d_o, dw, slab, npix, dv);
  else if (dv <= 48)
    hipLaunchKernelGGL((aa_outproj_bwd_kernel<T, 48, 64>), dim3(grid), dim3(256), 0, as_stream(stream), (const T*)g, ldg,
                       (const T*)gx, ldgx, ga, gb, gc, o, w, d_o, dw, slab, npix, dv);
  else
    hipLaunchKernelGGL((aa_outproj_bwd_kernel<T, 64, 32>), dim3(grid), dim3(256), 0, as_stream(stream), (const T*)g, ldg,
                       (const T*)gx, ldgx, ga, gb, gc, o, w, d_o, dw, slab, npix, dv);
  if (const int e = launch_status()) return e;
  return slab ? cx_dw_reduce(dw, slab, (size_t)dv * dv, grid, as_stream(stream)) : 0;
}

template <typename T>
int in_relu_bwd_t(const void* da, const void* x, const float* sc, const float* sh, float* S1, float* S2, void* gout, int B, int HW,
                   int C, int ldx, int ldg, void* stream) {
  if (!da || !x || !sc || !sh || !S1 || !S2 || !gout) return CX_EINVAL;
  if (C % 8 || C > 2048 || ldx % 8 || ldg % 8) return CX_ESHAPE;
  hipStream_t st = as_stream(stream);
  hipLaunchKernelGGL(in_relu_bwd_stats_kernel<T>, dim3((C + 63) / 64, B), dim3(256), 0, st, (const T*)da, (const T*)x, sc, sh, S1, S2,
                     HW, C, ldx);
  const size_t total = (size_t)B * HW * (C / 8);
  hipLaunchKernelGGL(in_relu_bwd_apply_kernel<T>, dim3(grid_for(total, 256, 8192)), dim3(256), 0, st, (const T*)da, (const T*)x, sc,
                     sh, S1, S2, (T*)gout, HW, C, ldx, ldg, total);
  return launch_status();
}

extern "C" {

int cx_aa_attention_fwd(const void* qkv, const float* rel_h, const float* rel_w, float* o, float* lse, int B, int H, int W, int nh,
                        int dk, int dv, int ldq, void* stream) {
  return aa_attention_fwd_t<bf16>(qkv, rel_h, rel_w, o, lse, B, H, W, nh, dk, dv, ldq, stream);
}
int cx_aa_attention_fwd_f32(const void* qkv, const float* rel_h, const float* rel_w, float* o, float* lse, int B, int H, int W, int nh,
                        int dk, int dv, int ldq, void* stream) {
  return aa_attention_fwd_t<float>(qkv, rel_h, rel_w, o, lse, B, H, W, nh, dk, dv, ldq, stream);
}

int cx_aa_attention_weights(const void* qkv, const float* rel_h, const float* rel_w, const float* lse, float* weights, int B, int H,
                            int W, int nh, int dk, int dv, int ldq, void* stream) {
  return aa_attention_weights_t<bf16>(qkv, rel_h, rel_w, lse, weights, B, H, W, nh, dk, dv, ldq, stream);
}
int cx_aa_attention_weights_f32(const void* qkv, const float* rel_h, const float* rel_w, const float* lse, float* weights, int B, int H,
                            int W, int nh, int dk, int dv, int ldq, void* stream) {
  return aa_attention_weights_t<float>(qkv, rel_h, rel_w, lse, weights, B, H, W, nh, dk, dv, ldq, stream);
}

int cx_aa_attention_bwd(const void* qkv, const float* rel_h, const float* rel_w, const float* o, const float* d_o, const float* lse,
                        float* dqkv, float* d_rel_h, float* d_rel_w, int B, int H, int W, int nh, int dk, int dv, int ldq,
                        float* scratch, int64_t scratch_floats, void* stream) {
  return aa_attention_bwd_t<bf16>(qkv, rel_h, rel_w, o, d_o, lse, dqkv, d_rel_h, d_rel_w, B, H, W, nh, dk, dv, ldq, scratch, scratch_floats, stream);
}
int cx_aa_attention_bwd_f32(const void* qkv, const float* rel_h, const float* rel_w, const float* o, const float* d_o, const float* lse,
                        float* dqkv, float* d_rel_h, float* d_rel_w, int B, int H, int W, int nh, int dk, int dv, int ldq,
                        float* scratch, int64_t scratch_floats, void* stream) {
  return aa_attention_bwd_t<float>(qkv, rel_h, rel_w, o, d_o, lse, dqkv, d_rel_h, d_rel_w, B, H, W, nh, dk, dv, ldq, scratch, scratch_floats, stream);
}

int cx_stats_bc(const void* x, float* sum, float* sq, int B, int HW, int C, int ldx, void* stream) {
  return stats_bc_t<bf16>(x, sum, sq, B, HW, C, ldx, stream);
}
int cx_stats_bc_f32(const void* x, float* sum, float* sq, int B, int HW, int C, int ldx, void* stream) {
  return stats_bc_t<float>(x, sum, sq, B, HW, C, ldx, stream);
}

int cx_affine_relu_bc(const void* x, const float* sc, const float* sh, void* y, int B, int HW, int C, int ldx, void* stream) {
  return affine_relu_bc_t<bf16>(x, sc, sh, y, B, HW, C, ldx, stream);
}
int cx_affine_relu_bc_f32(const void* x, const float* sc, const float* sh, void* y, int B, int HW, int C, int ldx, void* stream) {
  return affine_relu_bc_t<float>(x, sc, sh, y, B, HW, C, ldx, stream);
}

int cx_aa_outproj_fwd(const float* o, const float* w, void* y, int ldy, float* stat_sum, float* stat_sq, size_t npix, int dv,
                      int stat_rows, int stat_rstride, void* stream) {
  return aa_outproj_fwd_t<bf16>(o, w, y, ldy, stat_sum, stat_sq, npix, dv, stat_rows, stat_rstride, stream);
}
int cx_aa_outproj_fwd_f32(const float* o, const float* w, void* y, int ldy, float* stat_sum, float* stat_sq, size_t npix, int dv,
                      int stat_rows, int stat_rstride, void* stream) {
  return aa_outproj_fwd_t<float>(o, w, y, ldy, stat_sum, stat_sq, npix, dv, stat_rows, stat_rstride, stream);
}

int cx_aa_outproj_bwd(const void* g, int ldg, const void* gx, int ldgx, const float* ga, const float* gb, const float* gc,
                      const float* o, const float* w, float* d_o, float* dw, size_t npix, int dv, float* scratch, int64_t scratch_floats,
                      void* stream) {
  return aa_outproj_bwd_t<bf16>(g, ldg, gx, ldgx, ga, gb, gc, o, w, d_o, dw, npix, dv, scratch, scratch_floats, stream);
}
int cx_aa_outproj_bwd_f32(const void* g, int ldg, const void* gx, int ldgx, const float* ga, const float* gb, const float* gc,
                      const float* o, const float* w, float* d_o, float* dw, size_t npix, int dv, float* scratch, int64_t scratch_floats,
                      void* stream) {
  return aa_outproj_bwd_t<float>(g, ldg, gx, ldgx, ga, gb, gc, o, w, d_o, dw, npix, dv, scratch, scratch_floats, stream);
}

int cx_f32_to_bf16(const float* x, void* y, size_t n, void* stream) {
  if (!x || !y) return CX_EINVAL;
  hipLaunchKernelGGL(f32_to_bf16_kernel, dim3(grid_for(n, 256, 4096)), dim3(256), 0, as_stream(stream), x, (bf16*)y, n);
  return launch_status();
}

int cx_in_relu_bwd(const void* da, const void* x, const float* sc, const float* sh, float* S1, float* S2, void* gout, int B, int HW,
                   int C, int ldx, int ldg, void* stream) {
  return in_relu_bwd_t<bf16>(da, x, sc, sh, S1, S2, gout, B, HW, C, ldx, ldg, stream);
}
int cx_in_relu_bwd_f32(const void* da, const void* x, const float* sc, const float* sh, float* S1, float* S2, void* gout, int B, int HW,
                   int C, int ldx, int ldg, void* stream) {
  return in_relu_bwd_t<float>(da, x, sc, sh, S1, S2, gout, B, HW, C, ldx, ldg, stream);
}

}  // extern "C"
