// The Barlow Twins loss over the (N, d) embeddings of a step (include/chexpert_hip.h, cx_barlow_fwd_bwd): the first loss here whose
// arithmetic is matrix-shaped -- three products with d x d or h x d outputs -- and so the first on the fp32-input MFMA
// (v_mfma_f32_32x32x2_f32: bit for bit a k-ordered fmaf chain), with the operand staging of knn.hip / probe.hip: whole-row global
// loads, k-major LDS tiles, the next chunk's loads in flight during the MFMAs.  h = N / 2 pairs, row p is view A and row p + h view B.
//
//   barlow_norm_kernel    a workgroup owns 32 columns of one view: the pair mask and its count m (every workgroup counts for itself:
//                         integers, no order), then mean, biased variance and the normalised column in three passes over the rows;
//                         thread (row group g of 8, column c) adds rows g, g + 8, ... in ascending order, the 8 partials are added in
//                         group order.  A row outside the batch is never loaded and is written as zeros, so it reaches no sum.
//   barlow_corr_kernel    a workgroup (4 waves, 2 x 2) owns a 64 x 64 tile of C = A^T B / m, K = h in chunks of 32 pairs; the
//                         epilogue forms G, writes it, and leaves the tile's share of on, off, sum C_kk (wave butterfly, then the 4
//                         waves in order) and of the row / column sums of G o C (through an LDS image of the tile, ascending index).
//   barlow_finish_kernel  one workgroup: the tiles' shares in tile order, the loss terms in double; loss, stats, and the two vectors
//                         r_k = sum_l G_kl C_kl and c_l = sum_k G_kl C_kl.
//   barlow_grad_kernel    a workgroup owns a 64 x 64 tile of dA^ = B^ G^T / m (blockIdx.z 0) or dB^ = A^ G / m (1), K = d; the
//                         epilogue is BatchNorm's backward in its closed form -- mean_p dA^ = 0, mean_p (dA^ o A^)_k = r_k / m --
//                         times grad_scale, zeros for a row outside the batch and for the odd last row.
// m < 2: the products are skipped and every output is an exact zero.  No atomics, every sum in a fixed order, partial tiles and the
// h and d tails by zero fill and predication: the same bits on every run, and each output alone has the bits it has beside the others.
#include "common.h"
#include <math.h>

namespace {

constexpr int BT_NT = 256, BT_T = 64, BT_KC = 32;
constexpr int BT_PV = BT_T + 4;      // pitch of a tile stored as it lies in memory (k-major rows, 16-byte aligned quads)
constexpr int BT_PT = BT_T + 1;      // pitch of a tile stored transposed, and of the G o C image: 1 (mod 32)
constexpr int BT_NC = 32, BT_NG = 8; // barlow_norm_kernel: columns of a workgroup, row groups
constexpr int BT_MAX_N = CX_BARLOW_MAX_N, BT_MAX_D = CX_BARLOW_MAX_D;
constexpr float BT_EPS = CX_BARLOW_EPS;

struct BtLayout {
  long long a, b, g, istd_a, istd_b, rs, cs, m, tile, rowpart, colpart, total;
  int h, d4, nt;
};
static inline long long bt_r4(const long long x) { return (x + 3) & ~3ll; }
static inline BtLayout bt_layout(const int N, const int d) {
  BtLayout L;
  L.h = N / 2;
  L.d4 = (int)bt_r4(d);
  L.nt = (d + BT_T - 1) / BT_T;
  const long long hd = bt_r4((long long)L.h * d), dd = bt_r4((long long)d * d);
  L.a = 0;
  L.b = hd;
  L.g = 2 * hd;
  L.istd_a = L.g + dd;
  L.istd_b = L.istd_a + L.d4;
  L.rs = L.istd_b + L.d4;
  L.cs = L.rs + L.d4;
  L.m = L.cs + L.d4;
  L.tile = L.m + 4;
  L.rowpart = L.tile + 4ll * L.nt * L.nt;
  L.colpart = L.rowpart + (long long)L.nt * L.d4;
  L.total = L.colpart + (long long)L.nt * L.d4;
  return L;
}

// four consecutive values of one row from column `col` on; zeros past the row's end and for a row that does not exist
template <bool VEC>
__device__ __forceinline__ float4 bt_ld4(const float* __restrict__ base, const int row, const bool row_ok, const int d, const int col) {
  float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
  if (!row_ok || col >= d) return v;
  const float* p = base + (size_t)row * d + col;
  if constexpr (VEC) return *reinterpret_cast<const float4*>(p);          // d % 4 == 0 and 16-byte bases: the whole quad is inside the row
  v.x = p[0];
  if (col + 1 < d) v.y = p[1];
  if (col + 2 < d) v.z = p[2];
  if (col + 3 < d) v.w = p[3];
  return v;
}

__device__ __forceinline__ float bt_wave_sum(float v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
  return v;
}

__global__ __launch_bounds__(BT_NT) void barlow_norm_kernel(const float* __restrict__ e, const float* __restrict__ ids,
                                                            float* __restrict__ ahat, float* __restrict__ bhat,
                                                            float* __restrict__ istd_a, float* __restrict__ istd_b,
                                                            float* __restrict__ m_out, const int h, const int d) {
  __shared__ unsigned char valid[BT_MAX_N / 2];
  __shared__ float red[BT_NG][BT_NC];
  const int tid = threadIdx.x, cl = tid & (BT_NC - 1), rg = tid >> 5, view = blockIdx.y;
  const int c = blockIdx.x * BT_NC + cl;
  const bool c_ok = c < d;
  int m = 0;
  for (int base = 0; base < h; base += BT_NT) {
    const int p = base + tid;
    const bool v = p < h && ids[p] >= 0.f && ids[p + h] >= 0.f;
    if (p < h) valid[p] = v ? 1 : 0;
    m += __syncthreads_count(v);
  }
  if (blockIdx.x == 0 && view == 0 && tid == 0) m_out[0] = (float)m;
  if (m < 2) return;
  const float mf = (float)m;
  const float* const x = e + (size_t)view * h * d;
  float* const y = view ? bhat : ahat;
  float s = 0.f;
  if (c_ok)
    for (int p = rg; p < h; p += BT_NG)
      if (valid[p]) s += x[(size_t)p * d + c];
  red[rg][cl] = s;
  __syncthreads();
  float mu = red[0][cl];
#pragma unroll
  for (int g = 1; g < BT_NG; ++g) mu += red[g][cl];
  mu = mu / mf;
  __syncthreads();
  float q = 0.f;
  if (c_ok)
    for (int p = rg; p < h; p += BT_NG)
      if (valid[p]) {
        const float t = x[(size_t)p * d + c] - mu;
        q = fmaf(t, t, q);
      }
  red[rg][cl] = q;
  __syncthreads();
  float var = red[0][cl];
#pragma unroll
  for (int g = 1; g < BT_NG; ++g) var += red[g][cl];
  var = var / mf;
  const float istd = 1.f / sqrtf(var + BT_EPS);
  if (c_ok) {
    if (rg == 0) (view ? istd_b : istd_a)[c] = istd;
    for (int p = rg; p < h; p += BT_NG) y[(size_t)p * d + c] = valid[p] ? (x[(size_t)p * d + c] - mu) * istd : 0.f;
  }
}

template <bool VEC>
__global__ __launch_bounds__(BT_NT) void barlow_corr_kernel(const float* __restrict__ ahat, const float* __restrict__ bhat,
                                                            const float* __restrict__ lambda, const float* __restrict__ m_in,
                                                            float* __restrict__ G, float* __restrict__ tilepart,
                                                            float* __restrict__ rowpart, float* __restrict__ colpart, const int h,
                                                            const int d, const int d4) {
  __shared__ __align__(16) float aT[BT_KC * BT_PV];     // [pair][k]: the chunk of A^ as it lies in memory
  __shared__ __align__(16) float bT[BT_KC * BT_PV];     // [pair][l]
  __shared__ float gc[BT_T * BT_PT];                    // [k][l]: G o C of the tile
  __shared__ float wred[4][3];
  const float mf = m_in[0];
  if (mf < 2.f) return;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, l31 = lane & 31, hh = lane >> 5, wi = wave >> 1, wj = wave & 1;
  const int tj = blockIdx.x, ti = blockIdx.y, nt = gridDim.x, k0 = ti * BT_T, l0 = tj * BT_T;
  const int nch = (h + BT_KC - 1) / BT_KC;
  const float lam2 = 2.f * lambda[0];
  float4 ra[2], rb[2];
  auto issue = [&](const int ch) {
#pragma unroll
    for (int t = 0; t < 2; ++t) {
      const int f = tid + BT_NT * t, p = ch * BT_KC + (f >> 4), q4 = 4 * (f & 15);
      ra[t] = bt_ld4<VEC>(ahat, p, p < h, d, k0 + q4);
      rb[t] = bt_ld4<VEC>(bhat, p, p < h, d, l0 + q4);
    }
  };
  f32x16 acc0, acc1;
#pragma unroll
  for (int i = 0; i < 16; ++i) { acc0[i] = 0.f; acc1[i] = 0.f; }
  issue(0);
  for (int ch = 0; ch < nch; ++ch) {
    __syncthreads();
#pragma unroll
    for (int t = 0; t < 2; ++t) {
      const int f = tid + BT_NT * t;
      *reinterpret_cast<float4*>(aT + (f >> 4) * BT_PV + 4 * (f & 15)) = ra[t];
      *reinterpret_cast<float4*>(bT + (f >> 4) * BT_PV + 4 * (f & 15)) = rb[t];
    }
    __syncthreads();
    if (ch + 1 < nch) issue(ch + 1);                       // in flight during the MFMAs below
    // D[i = k][j = l] += A[i][kk] B[kk][j]: lane gives A[l31][hh] and B[hh][l31]
#pragma unroll
    for (int s = 0; s < BT_KC / 2; s += 2) {
      const float a0 = aT[(2 * s + hh) * BT_PV + wi * 32 + l31], b0 = bT[(2 * s + hh) * BT_PV + wj * 32 + l31];
      const float a1 = aT[(2 * s + 2 + hh) * BT_PV + wi * 32 + l31], b1 = bT[(2 * s + 2 + hh) * BT_PV + wj * 32 + l31];
      acc0 = __builtin_amdgcn_mfma_f32_32x32x2f32(a0, b0, acc0, 0, 0, 0);
      acc1 = __builtin_amdgcn_mfma_f32_32x32x2f32(a1, b1, acc1, 0, 0, 0);
    }
  }
  // register r of lane (column l31) is row 8 (r >> 2) + 4 hh + (r & 3) of the wave's 32
  float on = 0.f, off = 0.f, dg = 0.f;
  const int jl = wj * 32 + l31, l = l0 + jl;
#pragma unroll
  for (int r = 0; r < 16; ++r) {
    const int il = wi * 32 + 8 * (r >> 2) + 4 * hh + (r & 3), k = k0 + il;
    const bool ok = k < d && l < d;
    const float Cv = (acc0[r] + acc1[r]) / mf;
    float Gv;
    if (k == l) {
      const float t = 1.f - Cv;
      Gv = -2.f * t;
      if (ok) { on = fmaf(t, t, on); dg += Cv; }
    } else {
      Gv = lam2 * Cv;
      if (ok) off = fmaf(Cv, Cv, off);
    }
    if (ok) G[(size_t)k * d + l] = Gv;
    gc[il * BT_PT + jl] = ok ? Gv * Cv : 0.f;
  }
  on = bt_wave_sum(on);
  off = bt_wave_sum(off);
  dg = bt_wave_sum(dg);
  if (lane == 0) { wred[wave][0] = on; wred[wave][1] = off; wred[wave][2] = dg; }
  __syncthreads();
  if (tid < 3) {
    float* const tp = tilepart + 4 * ((size_t)ti * nt + tj);
    tp[tid] = ((wred[0][tid] + wred[1][tid]) + wred[2][tid]) + wred[3][tid];
  }
  if (tid < BT_T) {
    if (k0 + tid < d) {
      float s = 0.f;
#pragma unroll 8
      for (int j = 0; j < BT_T; ++j) s += gc[tid * BT_PT + j];
      rowpart[(size_t)tj * d4 + k0 + tid] = s;
    }
  } else if (tid < 2 * BT_T) {
    const int j = tid - BT_T;
    if (l0 + j < d) {
      float s = 0.f;
#pragma unroll 8
      for (int i = 0; i < BT_T; ++i) s += gc[i * BT_PT + j];
      colpart[(size_t)ti * d4 + l0 + j] = s;
    }
  }
}

__global__ __launch_bounds__(BT_NT) void barlow_finish_kernel(const float* __restrict__ lambda, const float* __restrict__ m_in,
                                                              const float* __restrict__ tilepart, const float* __restrict__ rowpart,
                                                              const float* __restrict__ colpart, float* __restrict__ rs,
                                                              float* __restrict__ cs, float* __restrict__ loss,
                                                              float* __restrict__ stats, const int d, const int d4, const int nt) {
  const int tid = threadIdx.x;
  const float mf = m_in[0];
  if (mf < 2.f) {
    if (tid == 0) {
      if (loss) loss[0] = 0.f;
      if (stats) { stats[0] = 0.f; stats[1] = 0.f; stats[2] = 0.f; stats[3] = mf; }
    }
    return;
  }
  if (tid == 0 && (loss || stats)) {
    double on = 0.0, off = 0.0, dg = 0.0;
    for (int t = 0; t < nt * nt; ++t) {
      on += (double)tilepart[4 * t];
      off += (double)tilepart[4 * t + 1];
      dg += (double)tilepart[4 * t + 2];
    }
    if (loss) loss[0] = (float)(on + (double)lambda[0] * off);
    if (stats) { stats[0] = (float)on; stats[1] = (float)off; stats[2] = (float)(dg / (double)d); stats[3] = mf; }
  }
  for (int k = tid; k < d; k += BT_NT) {
    float r = 0.f, c = 0.f;
    for (int t = 0; t < nt; ++t) {
      r += rowpart[(size_t)t * d4 + k];
      c += colpart[(size_t)t * d4 + k];
    }
    rs[k] = r;
    cs[k] = c;
  }
}

template <bool VEC>
__global__ __launch_bounds__(BT_NT) void barlow_grad_kernel(const float* __restrict__ ahat, const float* __restrict__ bhat,
                                                            const float* __restrict__ G, const float* __restrict__ istd_a,
                                                            const float* __restrict__ istd_b, const float* __restrict__ rs,
                                                            const float* __restrict__ cs, const float* __restrict__ m_in,
                                                            const float* __restrict__ ids, float* __restrict__ dlogits,
                                                            const float grad_scale, const int N, const int h, const int d) {
  __shared__ float aT[BT_KC * BT_PT];       // [kk][pair]: the other view's chunk, transposed
  __shared__ float bT[BT_KC * BT_PT];       // [kk][output column]: G's chunk
  __shared__ unsigned char vrow[BT_T];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, l31 = lane & 31, hh = lane >> 5, wi = wave >> 1, wj = wave & 1;
  const int view = blockIdx.z, c0 = blockIdx.x * BT_T, p0 = blockIdx.y * BT_T;
  const float mf = m_in[0];
  if ((N & 1) && blockIdx.x == 0 && blockIdx.y == 0 && view == 0)       // the odd last row belongs to no pair
    for (int c = tid; c < d; c += BT_NT) dlogits[(size_t)(N - 1) * d + c] = 0.f;
  if (mf < 2.f) {
    for (int i = tid; i < BT_T * BT_T; i += BT_NT) {
      const int p = p0 + (i >> 6), c = c0 + (i & 63);
      if (p < h && c < d) dlogits[((size_t)view * h + p) * d + c] = 0.f;
    }
    return;
  }
  if (tid < BT_T) {
    const int p = p0 + tid;
    vrow[tid] = (p < h && ids[p] >= 0.f && ids[p + h] >= 0.f) ? 1 : 0;
  }
  const float* const other = view ? ahat : bhat;      // dA^ = B^ G^T / m, dB^ = A^ G / m
  const int nch = (d + BT_KC - 1) / BT_KC;
  float4 ra[2], rb[2];
  auto issue = [&](const int ch) {
    const int kk0 = ch * BT_KC;
#pragma unroll
    for (int t = 0; t < 2; ++t) {
      const int f = tid + BT_NT * t;
      const int i = f >> 3, kq = 4 * (f & 7);              // [64 rows][8 quads along kk]
      ra[t] = bt_ld4<VEC>(other, p0 + i, p0 + i < h, d, kk0 + kq);
      if (view == 0) {                                      // B[kk = l][j = k] = G[k][l]: rows of G are output columns
        rb[t] = bt_ld4<VEC>(G, c0 + i, c0 + i < d, d, kk0 + kq);
      } else {                                              // B[kk = k][j = l] = G[k][l]: as it lies in memory
        const int kk = f >> 4, q4 = 4 * (f & 15);           // [32 rows][16 quads along j]
        rb[t] = bt_ld4<VEC>(G, kk0 + kk, kk0 + kk < d, d, c0 + q4);
      }
    }
  };
  f32x16 acc0, acc1;
#pragma unroll
  for (int i = 0; i < 16; ++i) { acc0[i] = 0.f; acc1[i] = 0.f; }
  issue(0);
  for (int ch = 0; ch < nch; ++ch) {
    __syncthreads();
#pragma unroll
    for (int t = 0; t < 2; ++t) {
      const int f = tid + BT_NT * t;
      const int i = f >> 3, kq = 4 * (f & 7);
      aT[(kq + 0) * BT_PT + i] = ra[t].x;
      aT[(kq + 1) * BT_PT + i] = ra[t].y;
      aT[(kq + 2) * BT_PT + i] = ra[t].z;
      aT[(kq + 3) * BT_PT + i] = ra[t].w;
      if (view == 0) {
        bT[(kq + 0) * BT_PT + i] = rb[t].x;
        bT[(kq + 1) * BT_PT + i] = rb[t].y;
        bT[(kq + 2) * BT_PT + i] = rb[t].z;
        bT[(kq + 3) * BT_PT + i] = rb[t].w;
      } else {
        const int kk = f >> 4, q4 = 4 * (f & 15);
        bT[kk * BT_PT + q4 + 0] = rb[t].x;
        bT[kk * BT_PT + q4 + 1] = rb[t].y;
        bT[kk * BT_PT + q4 + 2] = rb[t].z;
        bT[kk * BT_PT + q4 + 3] = rb[t].w;
      }
    }
    __syncthreads();
    if (ch + 1 < nch) issue(ch + 1);                       // in flight during the MFMAs below
#pragma unroll
    for (int s = 0; s < BT_KC / 2; s += 2) {
      const float a0 = aT[(2 * s + hh) * BT_PT + wi * 32 + l31], b0 = bT[(2 * s + hh) * BT_PT + wj * 32 + l31];
      const float a1 = aT[(2 * s + 2 + hh) * BT_PT + wi * 32 + l31], b1 = bT[(2 * s + 2 + hh) * BT_PT + wj * 32 + l31];
      acc0 = __builtin_amdgcn_mfma_f32_32x32x2f32(a0, b0, acc0, 0, 0, 0);
      acc1 = __builtin_amdgcn_mfma_f32_32x32x2f32(a1, b1, acc1, 0, 0, 0);
    }
  }
  const int c = c0 + wj * 32 + l31;
  if (c >= d) return;
  const float* const own = view ? bhat : ahat;
  const float t = (view ? cs : rs)[c] / mf, is = (view ? istd_b : istd_a)[c];
#pragma unroll
  for (int r = 0; r < 16; ++r) {
    const int il = wi * 32 + 8 * (r >> 2) + 4 * hh + (r & 3), p = p0 + il;
    if (p >= h) continue;
    float out = 0.f;
    if (vrow[il]) {
      const float dhat = (acc0[r] + acc1[r]) / mf;
      out = (dhat - own[(size_t)p * d + c] * t) * is * grad_scale;
    }
    dlogits[((size_t)view * h + p) * d + c] = out;
  }
}

}  // namespace

long long cx_barlow_scratch(int N, int d) {
  if (N < 2 || d < 1 || N > BT_MAX_N || d > BT_MAX_D) return 0;
  return bt_layout(N, d).total;
}

int cx_barlow_fwd_bwd(const float* e, const float* ids, const float* lambda, float* loss, float* dlogits, float* stats, float grad_scale,
                      float* scratch, long long scratch_floats, int N, int d, void* stream) {
  if (!e || !ids || !lambda || !scratch || N < 2 || d < 1) return CX_EINVAL;
  if (N > BT_MAX_N || d > BT_MAX_D) return CX_ESHAPE;
  const BtLayout L = bt_layout(N, d);
  if (scratch_floats < L.total) return CX_EINVAL;
  const int h = L.h, nt = L.nt, ht = (h + BT_T - 1) / BT_T;
  float *ahat = scratch + L.a, *bhat = scratch + L.b, *G = scratch + L.g, *istd_a = scratch + L.istd_a, *istd_b = scratch + L.istd_b;
  float *rs = scratch + L.rs, *cs = scratch + L.cs, *m = scratch + L.m, *tilepart = scratch + L.tile;
  float *rowpart = scratch + L.rowpart, *colpart = scratch + L.colpart;
  const bool vec = (d % 4 == 0) && aligned16(scratch);
  hipStream_t st = as_stream(stream);
  hipLaunchKernelGGL(barlow_norm_kernel, dim3((d + BT_NC - 1) / BT_NC, 2), dim3(BT_NT), 0, st, e, ids, ahat, bhat, istd_a, istd_b, m, h, d);
  if (vec)
    hipLaunchKernelGGL(barlow_corr_kernel<true>, dim3(nt, nt), dim3(BT_NT), 0, st, ahat, bhat, lambda, m, G, tilepart, rowpart, colpart, h, d, L.d4);
  else
    hipLaunchKernelGGL(barlow_corr_kernel<false>, dim3(nt, nt), dim3(BT_NT), 0, st, ahat, bhat, lambda, m, G, tilepart, rowpart, colpart, h, d, L.d4);
  hipLaunchKernelGGL(barlow_finish_kernel, dim3(1), dim3(BT_NT), 0, st, lambda, m, tilepart, rowpart, colpart, rs, cs, loss, stats, d, L.d4, nt);
  if (dlogits) {
    if (vec)
      hipLaunchKernelGGL(barlow_grad_kernel<true>, dim3(nt, ht, 2), dim3(BT_NT), 0, st, ahat, bhat, G, istd_a, istd_b, rs, cs, m, ids, dlogits,
                         grad_scale, N, h, d);
    else
      hipLaunchKernelGGL(barlow_grad_kernel<false>, dim3(nt, ht, 2), dim3(BT_NT), 0, st, ahat, bhat, G, istd_a, istd_b, rs, cs, m, ids, dlogits,
                         grad_scale, N, h, d);
  }
  return launch_status();
}
