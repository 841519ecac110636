// Relative-position attention of AAConv2d (the reference's models/attn_aug_conv.py:43-100) for head widths that are runtime
// values: dkh = dk/nh in 1 .. 64, dvh = dv/nh in 1 .. 64.  aaconv.hip / aaconv_row.hip keep dkh = 20 and dvh <= 13 (every AA
// layer chexpert.py trains); the CIFAR harness of the reference builds others from its --attn_k / --attn_v / --attn_nh
// (WRN-16-4 at k 0.5: dkh 32, dvh 16; the k = 1.6 DenseNet: dkh 25, dvh 4).
//
// Same arithmetic as the generic kernels of aaconv.hip -- one lane per query (per key on the key side), keys / queries stream through
// LDS tiles and are read as broadcasts, online softmax in the forward, P recomputed from the saved log-sum-exp in the backward --
// with the head widths zero-padded to template capacities: KC in {32, 64} key channels, VC in {8, 16, 32, 64} value channels.
// The padded channels hold zeros in registers and LDS, so they add nothing to any sum.  Global reads of a head are element loads:
// at dkh = 25 the head offset n * dkh is not a multiple of 4 and the vector loads of aaconv.hip would be misaligned.
//
// LDS beyond 64 KB (large tables, 40 x 40 maps) is requested per instantiation with hipFuncSetAttribute (at most 160 KB).  The
// query side keeps 128 queries per workgroup, so the slab count of the reproducible table-gradient sums is the one of the
// workspace contract (chexpert_hip.h: ceil(HW/128) * B * nh slabs of dkh * (2H-1 + 2W-1) floats).
#include "common.h"

namespace {

constexpr int HQ = 128;      // queries (query side) or keys (key side) per workgroup, one per lane
constexpr int HT = 64;       // keys (query side) or queries (key side) per LDS tile
constexpr int LDS_MAX = 160 * 1024;

struct HGeo {
  int B, H, W, nh, dk, dv, ldq, dkh, dvh;     // qkv: (B, H*W, ldq), channels [q dk | k dk | v dv], head-major
};

// relative tables [KC][2L-1] with the rows dkh .. KC-1 zero
__device__ __forceinline__ void stage_tables(const float* __restrict__ rel_h, const float* __restrict__ rel_w, float* RH, float* RW, int KC,
                                             const HGeo& g, int LH, int LW, int tid) {
  for (int t = tid; t < KC * LH; t += HQ) RH[t] = t < g.dkh * LH ? rel_h[t] : 0.f;
  for (int t = tid; t < KC * LW; t += HQ) RW[t] = t < g.dkh * LW ? rel_w[t] : 0.f;
}

// one head of one pixel, scaled, zero-padded to the capacity
template <typename T, int C>
__device__ __forceinline__ void load_head(const T* __restrict__ p, int n, float (&x)[C], float scale) {
#pragma unroll
  for (int d = 0; d < C; ++d) x[d] = d < n ? V4<T>::ld1(p + d) * scale : 0.f;
}

// tile [HT][C] of one head's channels for rows r0 .. r0+HT-1 (clamped to HW-1), zero-padded columns
template <typename T, int C>
__device__ __forceinline__ void stage_tile(const T* __restrict__ base, int ldq, int ofs, int n, int r0, int HW, float scale, float* Xt, int tid) {
  for (int t = tid; t < HT * C; t += HQ) {
    const int r = t / C, d = t - r * C;
    const int rr = min(r0 + r, HW - 1);
    Xt[t] = d < n ? V4<T>::ld1(base + (size_t)rr * ldq + ofs + d) * scale : 0.f;
  }
}

// the two relative-logit rows of this lane's query: rh[ky] = q~ . RH[:, ky-qy+H-1], rw[kx] = q~ . RW[:, kx-qx+W-1]
template <int KC>
__device__ __forceinline__ void rel_rows(const float (&q)[KC], const float* RH, const float* RW, float* rh, float* rw, int H, int W,
                                         int qy, int qx) {
  const int LH = 2 * H - 1, LW = 2 * W - 1;
  for (int ky = 0; ky < H; ++ky) {
    float a = 0.f;
#pragma unroll
    for (int d = 0; d < KC; ++d) a = fmaf(q[d], RH[d * LH + ky - qy + H - 1], a);
    rh[ky] = a;
  }
  for (int kx = 0; kx < W; ++kx) {
    float a = 0.f;
#pragma unroll
    for (int d = 0; d < KC; ++d) a = fmaf(q[d], RW[d * LW + kx - qx + W - 1], a);
    rw[kx] = a;
  }
}

template <int KC>
__device__ __forceinline__ float dot_key(const float (&q)[KC], const float* Kr, float s) {
  const float4* kp = reinterpret_cast<const float4*>(Kr);
#pragma unroll
  for (int c = 0; c < KC / 4; ++c) {
    const float4 kv = kp[c];
    s = fmaf(q[4 * c], kv.x, fmaf(q[4 * c + 1], kv.y, fmaf(q[4 * c + 2], kv.z, fmaf(q[4 * c + 3], kv.w, s))));
  }
  return s;
}

// ---------------------------------------------------------------------------------------------- forward (o, lse)
template <typename T, int KC, int VC>
__global__ __launch_bounds__(HQ) void aah_fwd_kernel(const T* __restrict__ qkv, const float* __restrict__ rel_h, const float* __restrict__ rel_w,
                                                     float* __restrict__ o, float* __restrict__ lse, const HGeo g) {
  extern __shared__ __attribute__((aligned(16))) float lds[];
  const int H = g.H, W = g.W, HW = H * W;
  const int LH = 2 * H - 1, LW = 2 * W - 1;
  float* RH = lds;                       // [KC][LH]
  float* RW = RH + KC * LH;              // [KC][LW]
  float* rh = RW + KC * LW;              // [HQ][H+1]
  float* rw = rh + HQ * (H + 1);         // [HQ][W+1]
  float* Kt = rw + HQ * (W + 1);         // [HT][KC]
  float* Vt = Kt + HT * KC;              // [HT][VC]
  const int tid = threadIdx.x;
  const int bn = blockIdx.y, b = bn / g.nh, n = bn - b * g.nh;
  const int i = blockIdx.x * HQ + tid;
  const bool qvalid = i < HW;
  const int ic = qvalid ? i : HW - 1;
  const int qy = ic / W, qx = ic - qy * W;
  const T* base = qkv + (size_t)b * HW * g.ldq;
  const float scale = rsqrtf((float)g.dkh);

  stage_tables(rel_h, rel_w, RH, RW, KC, g, LH, LW, tid);
  float q[KC];
  load_head<T, KC>(base + (size_t)ic * g.ldq + n * g.dkh, g.dkh, q, scale);
  __syncthreads();
  rel_rows<KC>(q, RH, RW, rh + tid * (H + 1), rw + tid * (W + 1), H, W, qy, qx);

  float m = -3.0e38f, l = 0.f, acc[VC];
#pragma unroll
  for (int d = 0; d < VC; ++d) acc[d] = 0.f;
  const int kofs = g.dk + n * g.dkh, vofs = 2 * g.dk + n * g.dvh;
  for (int j0 = 0; j0 < HW; j0 += HT) {
    __syncthreads();
    stage_tile<T, KC>(base, g.ldq, kofs, g.dkh, j0, HW, 1.f, Kt, tid);
    stage_tile<T, VC>(base, g.ldq, vofs, g.dvh, j0, HW, 1.f, Vt, tid);
    __syncthreads();
    const int jn = min(HT, HW - j0);
    int ky = j0 / W, kx = j0 - ky * W;
#pragma unroll 2
    for (int j = 0; j < jn; ++j) {
      const float s = dot_key<KC>(q, Kt + j * KC, rh[tid * (H + 1) + ky] + rw[tid * (W + 1) + kx]);
      const float4* vp = reinterpret_cast<const float4*>(Vt + j * VC);
      if (s > m) {
        const float c = __expf(m - s);
        l = fmaf(l, c, 1.f);
#pragma unroll
        for (int e = 0; e < VC / 4; ++e) {
          const float4 v = vp[e];
          acc[4 * e] = fmaf(acc[4 * e], c, v.x);
          acc[4 * e + 1] = fmaf(acc[4 * e + 1], c, v.y);
          acc[4 * e + 2] = fmaf(acc[4 * e + 2], c, v.z);
          acc[4 * e + 3] = fmaf(acc[4 * e + 3], c, v.w);
        }
        m = s;
      } else {
        const float p = __expf(s - m);
        l += p;
#pragma unroll
        for (int e = 0; e < VC / 4; ++e) {
          const float4 v = vp[e];
          acc[4 * e] = fmaf(p, v.x, acc[4 * e]);
          acc[4 * e + 1] = fmaf(p, v.y, acc[4 * e + 1]);
          acc[4 * e + 2] = fmaf(p, v.z, acc[4 * e + 2]);
          acc[4 * e + 3] = fmaf(p, v.w, acc[4 * e + 3]);
        }
      }
      if (++kx == W) { kx = 0; ++ky; }
    }
  }
  if (qvalid) {
    const float inv = 1.f / l;
    float* op = o + ((size_t)b * HW + i) * g.dv + n * g.dvh;
#pragma unroll
    for (int d = 0; d < VC; ++d)
      if (d < g.dvh) op[d] = acc[d] * inv;
    lse[(size_t)bn * HW + i] = m + __logf(l);
  }
}

// ---------------------------------------------------------------------------------------------- attention maps (AAConv2d.weights)
template <typename T, int KC>
__global__ __launch_bounds__(HQ) void aah_weights_kernel(const T* __restrict__ qkv, const float* __restrict__ rel_h,
                                                         const float* __restrict__ rel_w, const float* __restrict__ lse,
                                                         float* __restrict__ wts, const HGeo g) {
  extern __shared__ __attribute__((aligned(16))) float lds[];
  const int H = g.H, W = g.W, HW = H * W;
  const int LH = 2 * H - 1, LW = 2 * W - 1;
  float* RH = lds;
  float* RW = RH + KC * LH;
  float* rh = RW + KC * LW;
  float* rw = rh + HQ * (H + 1);
  float* Kt = rw + HQ * (W + 1);
  const int tid = threadIdx.x;
  const int bn = blockIdx.y, b = bn / g.nh, n = bn - b * g.nh;
  const int i = blockIdx.x * HQ + tid;
  const bool qvalid = i < HW;
  const int ic = qvalid ? i : HW - 1;
  const int qy = ic / W, qx = ic - qy * W;
  const T* base = qkv + (size_t)b * HW * g.ldq;
  stage_tables(rel_h, rel_w, RH, RW, KC, g, LH, LW, tid);
  float q[KC];
  load_head<T, KC>(base + (size_t)ic * g.ldq + n * g.dkh, g.dkh, q, rsqrtf((float)g.dkh));
  __syncthreads();
  rel_rows<KC>(q, RH, RW, rh + tid * (H + 1), rw + tid * (W + 1), H, W, qy, qx);
  const float li = lse[(size_t)bn * HW + ic];
  float* row = wts + ((size_t)bn * HW + ic) * HW;
  const int kofs = g.dk + n * g.dkh;
  for (int j0 = 0; j0 < HW; j0 += HT) {
    __syncthreads();
    stage_tile<T, KC>(base, g.ldq, kofs, g.dkh, j0, HW, 1.f, Kt, tid);
    __syncthreads();
    const int jn = min(HT, HW - j0);
    int ky = j0 / W, kx = j0 - ky * W;
    for (int j = 0; j < jn; ++j) {
      const float sl = dot_key<KC>(q, Kt + j * KC, rh[tid * (H + 1) + ky] + rw[tid * (W + 1) + kx]);
      if (qvalid) row[j0 + j] = __expf(sl - li);
      if (++kx == W) { kx = 0; ++ky; }
    }
  }
}

// ---------------------------------------------------------------------------------------------- backward, query side
// One lane per query: P from the saved LSE, dS = P (dP - delta), dq_i = scale * sum_j dS_ij (k_j + RH[:, ky-qy+H-1] + RW[:, kx-qx+W-1]);
// the row / column sums of dS (d rh_i[ky], d rw_i[kx]) leave the key loop in LDS and become the workgroup's partial table gradients
// (owner-computes, a fixed order of additions), plain-stored into the caller's slab (or added with atomics without a workspace).
// LDS: [RH][RW][rh -> d rh in place][d rw][ rw | Kt | Vt  ->  Qs after the key loop ]
template <typename T, int KC, int VC>
__host__ __device__ constexpr int bwdq_union_floats(int W) {
  return HQ * (W + 1) + HT * (KC + VC) > HQ * (KC + 1) ? HQ * (W + 1) + HT * (KC + VC) : HQ * (KC + 1);
}

template <typename T, int KC, int VC>
__global__ __launch_bounds__(HQ) void aah_bwd_q_kernel(const T* __restrict__ qkv, const float* __restrict__ rel_h, const float* __restrict__ rel_w,
                                                       const float* __restrict__ o, const float* __restrict__ d_o, const float* __restrict__ lse,
                                                       float* __restrict__ dqkv, float* __restrict__ d_rel_h, float* __restrict__ d_rel_w,
                                                       float* __restrict__ slab_h, float* __restrict__ slab_w, const HGeo g) {
  extern __shared__ __attribute__((aligned(16))) float lds[];
  const int H = g.H, W = g.W, HW = H * W;
  const int LH = 2 * H - 1, LW = 2 * W - 1;
  float* RH = lds;                       // [KC][LH]
  float* RW = RH + KC * LH;              // [KC][LW]
  float* rh = RW + KC * LW;              // [HQ][H+1]  row logits; entry ky becomes d rh_i[ky] once key row ky is done
  float* drw = rh + HQ * (H + 1);        // [HQ][W+1]  d rw_i[kx]
  float* rw = drw + HQ * (W + 1);        // [HQ][W+1]  column logits    } key loop
  float* Kt = rw + HQ * (W + 1);         // [HT][KC]                    }
  float* Vt = Kt + HT * KC;              // [HT][VC]                    }
  float* Qs = rw;                        // [HQ][KC+1] scaled queries, after the key loop
  const int tid = threadIdx.x;
  const int bn = blockIdx.y, b = bn / g.nh, n = bn - b * g.nh;
  const int i = blockIdx.x * HQ + tid;
  const bool qvalid = i < HW;
  const int ic = qvalid ? i : HW - 1;
  const int qy = ic / W, qx = ic - qy * W;
  const T* base = qkv + (size_t)b * HW * g.ldq;
  const float scale = rsqrtf((float)g.dkh);

  stage_tables(rel_h, rel_w, RH, RW, KC, g, LH, LW, tid);
  float q[KC];
  load_head<T, KC>(base + (size_t)ic * g.ldq + n * g.dkh, g.dkh, q, scale);
  float dO[VC], delta = 0.f;
  {
    const float* op = o + ((size_t)b * HW + ic) * g.dv + n * g.dvh;
    const float* dp = d_o + ((size_t)b * HW + ic) * g.dv + n * g.dvh;
#pragma unroll
    for (int d = 0; d < VC; ++d) {
      dO[d] = (qvalid && d < g.dvh) ? dp[d] : 0.f;
      if (d < g.dvh) delta = fmaf(dO[d], op[d], delta);
    }
  }
  const float L = lse[(size_t)bn * HW + ic];
  __syncthreads();
  rel_rows<KC>(q, RH, RW, rh + tid * (H + 1), rw + tid * (W + 1), H, W, qy, qx);
  for (int kx = 0; kx < W; ++kx) drw[tid * (W + 1) + kx] = 0.f;
  float dq[KC];
#pragma unroll
  for (int d = 0; d < KC; ++d) dq[d] = 0.f;
  const int kofs = g.dk + n * g.dkh, vofs = 2 * g.dk + n * g.dvh;
  float drh_run = 0.f;
  for (int j0 = 0; j0 < HW; j0 += HT) {
    __syncthreads();
    stage_tile<T, KC>(base, g.ldq, kofs, g.dkh, j0, HW, 1.f, Kt, tid);
    stage_tile<T, VC>(base, g.ldq, vofs, g.dvh, j0, HW, 1.f, Vt, tid);
    __syncthreads();
    const int jn = min(HT, HW - j0);
    int ky = j0 / W, kx = j0 - ky * W;
    for (int j = 0; j < jn; ++j) {
      const float s = dot_key<KC>(q, Kt + j * KC, rh[tid * (H + 1) + ky] + rw[tid * (W + 1) + kx]);
      const float p = __expf(s - L);
      float dp = 0.f;
      const float4* vp = reinterpret_cast<const float4*>(Vt + j * VC);
#pragma unroll
      for (int e = 0; e < VC / 4; ++e) {
        const float4 v = vp[e];
        dp = fmaf(dO[4 * e], v.x, fmaf(dO[4 * e + 1], v.y, fmaf(dO[4 * e + 2], v.z, fmaf(dO[4 * e + 3], v.w, dp))));
      }
      const float ds = p * (dp - delta);
      const float4* kp = reinterpret_cast<const float4*>(Kt + j * KC);
#pragma unroll
      for (int c = 0; c < KC / 4; ++c) {
        const float4 kv = kp[c];
        dq[4 * c] = fmaf(ds, kv.x, dq[4 * c]);
        dq[4 * c + 1] = fmaf(ds, kv.y, dq[4 * c + 1]);
        dq[4 * c + 2] = fmaf(ds, kv.z, dq[4 * c + 2]);
        dq[4 * c + 3] = fmaf(ds, kv.w, dq[4 * c + 3]);
      }
      drh_run += ds;
      drw[tid * (W + 1) + kx] += ds;
      if (++kx == W) {
        // key row ky complete: fold d rh_i[ky] into dq; its logit slot is not read again and keeps it for the table gradient
        if (qvalid) {
          const int r = ky - qy + H - 1;
#pragma unroll
          for (int d = 0; d < KC; ++d) dq[d] = fmaf(drh_run, RH[d * LH + r], dq[d]);
        }
        rh[tid * (H + 1) + ky] = qvalid ? drh_run : 0.f;
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
      for (int d = 0; d < KC; ++d) dq[d] = fmaf(dsum, RW[d * LW + r], dq[d]);
    }
    float* dqp = dqkv + ((size_t)b * HW + i) * (2 * g.dk + g.dv) + n * g.dkh;
#pragma unroll
    for (int d = 0; d < KC; ++d)
      if (d < g.dkh) dqp[d] = dq[d] * scale;      // q~ = q * scale
  } else {
    for (int kx = 0; kx < W; ++kx) drw[tid * (W + 1) + kx] = 0.f;
  }
  __syncthreads();                       // every lane is done with rw / Kt / Vt: Qs takes their place
#pragma unroll
  for (int d = 0; d < KC; ++d) Qs[tid * (KC + 1) + d] = q[d];
  __syncthreads();
  // table gradients: the thread that owns word (d, r) walks the workgroup's queries in order; query l meets offset r at key row
  // ky = r - (H-1) + qy_l (column kx = r - (W-1) + qx_l)
  const int i0 = blockIdx.x * HQ;
  const size_t wg = (size_t)blockIdx.y * gridDim.x + blockIdx.x;
  const int TH = g.dkh * LH, TW = g.dkh * LW;
  for (int t = tid; t < TH; t += HQ) {
    const int d = t / LH, r = t - d * LH;
    int yq = i0 / W, xq = i0 - yq * W;
    float a = 0.f;
    for (int l = 0; l < HQ; ++l) {
      const int ky = r - (H - 1) + yq;
      if (ky >= 0 && ky < H) a = fmaf(rh[l * (H + 1) + ky], Qs[l * (KC + 1) + d], a);
      if (++xq == W) { xq = 0; ++yq; }
    }
    if (slab_h) slab_h[wg * TH + t] = a; else atomicAdd(&d_rel_h[t], a);
  }
  for (int t = tid; t < TW; t += HQ) {
    const int d = t / LW, r = t - d * LW;
    int xq = i0 % W;
    float a = 0.f;
    for (int l = 0; l < HQ; ++l) {
      const int kx = r - (W - 1) + xq;
      if (kx >= 0 && kx < W) a = fmaf(drw[l * (W + 1) + kx], Qs[l * (KC + 1) + d], a);
      if (++xq == W) xq = 0;
    }
    if (slab_w) slab_w[wg * TW + t] = a; else atomicAdd(&d_rel_w[t], a);
  }
}

// ---------------------------------------------------------------------------------------------- backward, key side
// One lane per key j, queries stream through LDS: dk_j = sum_i dS_ij q~_i, dv_j = sum_i P_ij dO_i.  MODE 0 both; for the widest
// heads (KC + VC > 72) the two sums are separate launches, MODE 1 dk (k, v, dk live) and MODE 2 dv (k, dv live), so that neither
// holds four head-wide arrays in registers.
template <typename T, int KC, int VC, int MODE>
__global__ __launch_bounds__(HQ) void aah_bwd_k_kernel(const T* __restrict__ qkv, const float* __restrict__ rel_h, const float* __restrict__ rel_w,
                                                       const float* __restrict__ o, const float* __restrict__ d_o, const float* __restrict__ lse,
                                                       float* __restrict__ dqkv, const HGeo g) {
  constexpr bool DK = MODE != 2, DV = MODE != 1;
  extern __shared__ __attribute__((aligned(16))) float lds[];
  const int H = g.H, W = g.W, HW = H * W;
  const int LH = 2 * H - 1, LW = 2 * W - 1;
  float* RH = lds;                       // [KC][LH]
  float* RW = RH + KC * LH;              // [KC][LW]
  float* Qt = RW + KC * LW;              // [HT][KC] scaled queries
  float* Dt = Qt + HT * KC;              // [HT][VC] dO
  float* Et = Dt + HT * VC;              // [HT][2]  delta, lse
  const int tid = threadIdx.x;
  const int bn = blockIdx.y, b = bn / g.nh, n = bn - b * g.nh;
  const int j = blockIdx.x * HQ + tid;
  const bool kvalid = j < HW;
  const int jc = kvalid ? j : HW - 1;
  const int ky = jc / W, kx = jc - ky * W;
  const T* base = qkv + (size_t)b * HW * g.ldq;
  const float scale = rsqrtf((float)g.dkh);
  stage_tables(rel_h, rel_w, RH, RW, KC, g, LH, LW, tid);
  float k[KC], v[VC], dk[KC], dv[VC];
  load_head<T, KC>(base + (size_t)jc * g.ldq + g.dk + n * g.dkh, g.dkh, k, 1.f);
  if (DK) load_head<T, VC>(base + (size_t)jc * g.ldq + 2 * g.dk + n * g.dvh, g.dvh, v, 1.f);
#pragma unroll
  for (int d = 0; d < KC; ++d) dk[d] = 0.f;
#pragma unroll
  for (int d = 0; d < VC; ++d) dv[d] = 0.f;
  for (int i0 = 0; i0 < HW; i0 += HT) {
    __syncthreads();
    stage_tile<T, KC>(base, g.ldq, n * g.dkh, g.dkh, i0, HW, scale, Qt, tid);
    for (int t = tid; t < HT; t += HQ) {
      const int iq = min(i0 + t, HW - 1);
      const bool ok = i0 + t < HW;
      const size_t ro = ((size_t)b * HW + iq) * g.dv + n * g.dvh;
      float de = 0.f;
      for (int d = 0; d < VC; ++d) {
        const float dd = (ok && d < g.dvh) ? d_o[ro + d] : 0.f;
        Dt[t * VC + d] = dd;
        if (d < g.dvh) de = fmaf(dd, o[ro + d], de);
      }
      Et[2 * t] = de;
      Et[2 * t + 1] = ok ? lse[(size_t)bn * HW + iq] : 3.0e38f;      // p = exp(s - inf) = 0 for padding queries
    }
    __syncthreads();
    const int in_ = min(HT, HW - i0);
    int qy = i0 / W, qx = i0 - qy * W;
    for (int ii = 0; ii < in_; ++ii) {
      const float* qp = Qt + ii * KC;
      const int rhh = ky - qy + H - 1, rww = kx - qx + W - 1;
      float s = 0.f;
#pragma unroll
      for (int d = 0; d < KC; ++d) s = fmaf(qp[d], k[d] + RH[d * LH + rhh] + RW[d * LW + rww], s);
      const float p = __expf(s - Et[2 * ii + 1]);
      const float4* dp4 = reinterpret_cast<const float4*>(Dt + ii * VC);
      if (DK) {
        float dp = 0.f;
#pragma unroll
        for (int e = 0; e < VC / 4; ++e) {
          const float4 u = dp4[e];
          dp = fmaf(u.x, v[4 * e], fmaf(u.y, v[4 * e + 1], fmaf(u.z, v[4 * e + 2], fmaf(u.w, v[4 * e + 3], dp))));
        }
        const float ds = p * (dp - Et[2 * ii]);
        const float4* q4 = reinterpret_cast<const float4*>(qp);
#pragma unroll
        for (int c = 0; c < KC / 4; ++c) {
          const float4 u = q4[c];
          dk[4 * c] = fmaf(ds, u.x, dk[4 * c]);
          dk[4 * c + 1] = fmaf(ds, u.y, dk[4 * c + 1]);
          dk[4 * c + 2] = fmaf(ds, u.z, dk[4 * c + 2]);
          dk[4 * c + 3] = fmaf(ds, u.w, dk[4 * c + 3]);
        }
      }
      if (DV) {
#pragma unroll
        for (int e = 0; e < VC / 4; ++e) {
          const float4 u = dp4[e];
          dv[4 * e] = fmaf(p, u.x, dv[4 * e]);
          dv[4 * e + 1] = fmaf(p, u.y, dv[4 * e + 1]);
          dv[4 * e + 2] = fmaf(p, u.z, dv[4 * e + 2]);
          dv[4 * e + 3] = fmaf(p, u.w, dv[4 * e + 3]);
        }
      }
      if (++qx == W) { qx = 0; ++qy; }
    }
  }
  if (kvalid) {
    float* dp = dqkv + ((size_t)b * HW + j) * (2 * g.dk + g.dv);
    if (DK) {
#pragma unroll
      for (int d = 0; d < KC; ++d)
        if (d < g.dkh) dp[g.dk + n * g.dkh + d] = dk[d];
    }
    if (DV) {
#pragma unroll
      for (int d = 0; d < VC; ++d)
        if (d < g.dvh) dp[2 * g.dk + n * g.dvh + d] = dv[d];
    }
  }
}

// ---------------------------------------------------------------------------------------------- launchers
inline size_t fwd_floats(int KC, int VC, int H, int W) {
  return (size_t)KC * (2 * H - 1 + 2 * W - 1) + (size_t)HQ * (H + W + 2) + (size_t)HT * (KC + VC);
}
template <int KC, int VC>
inline size_t bwdq_floats(int H, int W) {
  return (size_t)KC * (2 * H - 1 + 2 * W - 1) + (size_t)HQ * (H + 1) + (size_t)HQ * (W + 1) + bwdq_union_floats<float, KC, VC>(W);
}
inline size_t bwdk_floats(int KC, int VC, int H, int W) {
  return (size_t)KC * (2 * H - 1 + 2 * W - 1) + (size_t)HT * (KC + VC + 2);
}

// dynamic LDS above the 64 KB default, once per kernel instantiation (a host-side attribute: nothing is queued on the stream)
template <typename T> constexpr const char* tname() { return std::is_same<T, bf16>::value ? "bf16" : "f32"; }

template <typename K>
inline void allow_lds(K* kern) {
  (void)hipFuncSetAttribute(reinterpret_cast<const void*>(kern), hipFuncAttributeMaxDynamicSharedMemorySize, LDS_MAX);
}

template <typename T, int KC, int VC>
int launch_fwd(const HGeo& g, const T* qkv, const float* rel_h, const float* rel_w, float* o, float* lse, hipStream_t st) {
  static const bool attr = (allow_lds(&aah_fwd_kernel<T, KC, VC>), true);
  (void)attr;
  const size_t smem = fwd_floats(KC, VC, g.H, g.W) * 4;
  if (smem > LDS_MAX) return CX_ESHAPE;
  hipLaunchKernelGGL((aah_fwd_kernel<T, KC, VC>), dim3((g.H * g.W + HQ - 1) / HQ, g.B * g.nh), dim3(HQ), smem, st, qkv, rel_h, rel_w, o, lse, g);
  CX_KTAG("aa_heads_fwd<%s,%d,%d>", tname<T>(), KC, VC);
  return launch_status();
}

template <typename T, int KC>
int launch_weights(const HGeo& g, const T* qkv, const float* rel_h, const float* rel_w, const float* lse, float* wts, hipStream_t st) {
  static const bool attr = (allow_lds(&aah_weights_kernel<T, KC>), true);
  (void)attr;
  const size_t smem = fwd_floats(KC, 0, g.H, g.W) * 4;
  if (smem > LDS_MAX) return CX_ESHAPE;
  hipLaunchKernelGGL((aah_weights_kernel<T, KC>), dim3((g.H * g.W + HQ - 1) / HQ, g.B * g.nh), dim3(HQ), smem, st, qkv, rel_h, rel_w, lse, wts, g);
  CX_KTAG("aa_heads_weights<%s,%d>", tname<T>(), KC);
  return launch_status();
}

template <typename T, int KC, int VC>
int launch_bwd(const HGeo& g, const T* qkv, const float* rel_h, const float* rel_w, const float* o, const float* d_o, const float* lse,
               float* dqkv, float* d_rel_h, float* d_rel_w, float* slab_h, float* slab_w, hipStream_t st) {
  constexpr bool split = KC + VC > 72;
  static const bool attr = (allow_lds(&aah_bwd_q_kernel<T, KC, VC>), allow_lds(&aah_bwd_k_kernel<T, KC, VC, 0>),
                            allow_lds(&aah_bwd_k_kernel<T, KC, VC, 1>), allow_lds(&aah_bwd_k_kernel<T, KC, VC, 2>), true);
  (void)attr;
  const size_t smem_q = bwdq_floats<KC, VC>(g.H, g.W) * 4, smem_k = bwdk_floats(KC, VC, g.H, g.W) * 4;
  if (smem_q > LDS_MAX || smem_k > LDS_MAX) return CX_ESHAPE;
  const dim3 grid((g.H * g.W + HQ - 1) / HQ, g.B * g.nh);
  hipLaunchKernelGGL((aah_bwd_q_kernel<T, KC, VC>), grid, dim3(HQ), smem_q, st, qkv, rel_h, rel_w, o, d_o, lse, dqkv, d_rel_h, d_rel_w,
                     slab_h, slab_w, g);
  if (split) {
    hipLaunchKernelGGL((aah_bwd_k_kernel<T, KC, VC, 1>), grid, dim3(HQ), smem_k, st, qkv, rel_h, rel_w, o, d_o, lse, dqkv, g);
    hipLaunchKernelGGL((aah_bwd_k_kernel<T, KC, VC, 2>), grid, dim3(HQ), smem_k, st, qkv, rel_h, rel_w, o, d_o, lse, dqkv, g);
  } else {
    hipLaunchKernelGGL((aah_bwd_k_kernel<T, KC, VC, 0>), grid, dim3(HQ), smem_k, st, qkv, rel_h, rel_w, o, d_o, lse, dqkv, g);
  }
  CX_KTAG("aa_heads_bwd<%s,%d,%d>", tname<T>(), KC, VC);
  return launch_status();
}

// capacity dispatch: KC = 32 | 64 key channels, VC = 8 | 16 | 32 | 64 value channels
#define AAH_DISPATCH(KCV, VCV, CALL)               \
  if ((KCV) == 32) {                               \
    constexpr int KC = 32;                         \
    switch (VCV) {                                 \
      case 8: { constexpr int VC = 8; CALL; }      \
      case 16: { constexpr int VC = 16; CALL; }    \
      case 32: { constexpr int VC = 32; CALL; }    \
      default: { constexpr int VC = 64; CALL; }    \
    }                                              \
  } else {                                         \
    constexpr int KC = 64;                         \
    switch (VCV) {                                 \
      case 8: { constexpr int VC = 8; CALL; }      \
      case 16: { constexpr int VC = 16; CALL; }    \
      case 32: { constexpr int VC = 32; CALL; }    \
      default: { constexpr int VC = 64; CALL; }    \
    }                                              \
  }

inline int key_cap(int dkh) { return dkh <= 32 ? 32 : 64; }
inline int val_cap(int dvh) { return dvh <= 8 ? 8 : dvh <= 16 ? 16 : dvh <= 32 ? 32 : 64; }

// the shapes these kernels cover (the launchers also bound the LDS of the map size)
inline bool heads_shape(int B, int H, int W, int nh, int dk, int dv, int ldq, bool need_dv) {
  if (B <= 0 || H <= 0 || W <= 0 || nh <= 0 || dk % nh || dv % nh || ldq % 4 || ldq < 2 * dk + dv) return false;
  const int dkh = dk / nh, dvh = dv / nh;
  if (dkh < 1 || dkh > 64) return false;
  return !need_dv || (dvh >= 1 && dvh <= 64 && dv <= 104);
}

template <typename T>
int heads_fwd_t(const void* qkv, const float* rel_h, const float* rel_w, float* o, float* lse, int B, int H, int W, int nh, int dk, int dv,
                int ldq, hipStream_t st) {
  if (!heads_shape(B, H, W, nh, dk, dv, ldq, true)) return CX_ESHAPE;
  const HGeo g{B, H, W, nh, dk, dv, ldq, dk / nh, dv / nh};
  AAH_DISPATCH(key_cap(g.dkh), val_cap(g.dvh), return (launch_fwd<T, KC, VC>(g, (const T*)qkv, rel_h, rel_w, o, lse, st)))
}

template <typename T>
int heads_weights_t(const void* qkv, const float* rel_h, const float* rel_w, const float* lse, float* wts, int B, int H, int W, int nh, int dk,
                    int dv, int ldq, hipStream_t st) {
  if (!heads_shape(B, H, W, nh, dk, dv, ldq, false)) return CX_ESHAPE;
  const HGeo g{B, H, W, nh, dk, dv, ldq, dk / nh, dv / nh};
  return g.dkh <= 32 ? launch_weights<T, 32>(g, (const T*)qkv, rel_h, rel_w, lse, wts, st)
                     : launch_weights<T, 64>(g, (const T*)qkv, rel_h, rel_w, lse, wts, st);
}

template <typename T>
int heads_bwd_t(const void* qkv, const float* rel_h, const float* rel_w, const float* o, const float* d_o, const float* lse, float* dqkv,
                float* d_rel_h, float* d_rel_w, float* slab_h, float* slab_w, int B, int H, int W, int nh, int dk, int dv, int ldq, hipStream_t st) {
  if (!heads_shape(B, H, W, nh, dk, dv, ldq, true)) return CX_ESHAPE;
  const HGeo g{B, H, W, nh, dk, dv, ldq, dk / nh, dv / nh};
  AAH_DISPATCH(key_cap(g.dkh), val_cap(g.dvh),
               return (launch_bwd<T, KC, VC>(g, (const T*)qkv, rel_h, rel_w, o, d_o, lse, dqkv, d_rel_h, d_rel_w, slab_h, slab_w, st)))
}

}  // namespace

// entry points for aaconv.hip's dispatch (f32: the fp32 storage mode); CX_ESHAPE outside 1 <= dkh, dvh <= 64, dv <= 104 or when the
// map's tables and tiles exceed 160 KB of LDS.  slab_h / slab_w: ceil(HW/128) * B * nh partial tables each, or null (atomics).
int cx_aa_heads_fwd(int f32, const void* qkv, const float* rel_h, const float* rel_w, float* o, float* lse, int B, int H, int W, int nh,
                    int dk, int dv, int ldq, hipStream_t st) {
  return f32 ? heads_fwd_t<float>(qkv, rel_h, rel_w, o, lse, B, H, W, nh, dk, dv, ldq, st)
             : heads_fwd_t<bf16>(qkv, rel_h, rel_w, o, lse, B, H, W, nh, dk, dv, ldq, st);
}

int cx_aa_heads_weights(int f32, const void* qkv, const float* rel_h, const float* rel_w, const float* lse, float* wts, int B, int H, int W,
                        int nh, int dk, int dv, int ldq, hipStream_t st) {
  return f32 ? heads_weights_t<float>(qkv, rel_h, rel_w, lse, wts, B, H, W, nh, dk, dv, ldq, st)
             : heads_weights_t<bf16>(qkv, rel_h, rel_w, lse, wts, B, H, W, nh, dk, dv, ldq, st);
}

int cx_aa_heads_bwd(int f32, const void* qkv, const float* rel_h, const float* rel_w, const float* o, const float* d_o, const float* lse,
                    float* dqkv, float* d_rel_h, float* d_rel_w, float* slab_h, float* slab_w, int B, int H, int W, int nh, int dk, int dv,
                    int ldq, hipStream_t st) {
  return f32 ? heads_bwd_t<float>(qkv, rel_h, rel_w, o, d_o, lse, dqkv, d_rel_h, d_rel_w, slab_h, slab_w, B, H, W, nh, dk, dv, ldq, st)
             : heads_bwd_t<bf16>(qkv, rel_h, rel_w, o, d_o, lse, dqkv, d_rel_h, d_rel_w, slab_h, slab_w, B, H, W, nh, dk, dv, ldq, st);
}
