// HBM-bound glue kernels of the DenseNet hot path: layout conversion, weight packing, BatchNorm
// coefficient bookkeeping, stem pooling, head, loss, un-pooling and the fused optimisers.
// All activation traffic is 16 B per lane along the channel axis (NHWC bf16).
#include <vector>
#include "common.h"

namespace {

// ------------------------------------------------------------------------------------------------
// per-channel statistic reduction shared by the elementwise kernels: each thread owns one 8-channel
// chunk `cq` (constant over its grid-stride loop) and 2x8 partial sums.
__device__ __forceinline__ void block_stats_flush(const float (&s1)[8], const float (&s2)[8], int cq, int C,
                                                  float* lds, float* g1, float* g2, int det) {
  // lds: blockDim.x * 16 floats.  Every thread parks its 2 x 8 partial sums; the threads that own chunk c / 8 (tid % CP == c / 8)
  // are then summed in thread order -- a fixed order -- and the block row is plain-stored (det: row = blockIdx.x of a [grid][C]
  // slab, no atomics) or added to the single copy with one atomic per channel.
  const int CP = C >> 3;
  __syncthreads();
#pragma unroll
  for (int j = 0; j < 8; ++j) {
    lds[threadIdx.x * 16 + j] = s1[j];
    lds[threadIdx.x * 16 + 8 + j] = s2[j];
  }
  __syncthreads();
  for (int c = threadIdx.x; c < C; c += blockDim.x) {
    const int chunk = c >> 3, j = c & 7;
    float a = 0.f, b = 0.f;
    for (int t = chunk; t < (int)blockDim.x; t += CP) {
      a += lds[t * 16 + j];
      b += lds[t * 16 + 8 + j];
    }
    if (det) {
      g1[(size_t)blockIdx.x * C + c] = a;
      g2[(size_t)blockIdx.x * C + c] = b;
    } else {
      atomicAdd(&g1[c], a);
      atomicAdd(&g2[c], b);
    }
  }
}

// ------------------------------------------------------------------------------------------------
// (8-channel vector I/O for both storage types: V8<T> in common.h)

// ------------------------------------------------------------------------------------------------
__global__ void pack_weights_kernel(const float* __restrict__ w, bf16* __restrict__ out, int O, int I, int kh, int kw,
                                    int transpose, int stem) {
  const size_t idx = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (stem) {
    const size_t total = (size_t)7 * O * 32;
    if (idx >= total) return;
    const int k = idx % 32, o = (idx / 32) % O, ky = idx / (32 * (size_t)O);
    const int kx = (k >> 2) - 1, ch = k & 3;
    float v = 0.f;
    if (kx >= 0 && ch < 3) v = w[((size_t)(o * 3 + ch) * 7 + ky) * 7 + kx];
    out[idx] = f2bf(v);
    return;
  }
  const int taps = kh * kw;
  const size_t total = (size_t)taps * O * I;
  if (idx >= total) return;
  if (!transpose) {                  // [tap][o][i]
    const int i = idx % I, o = (idx / I) % O, tap = idx / ((size_t)I * O);
    out[idx] = f2bf(w[((size_t)o * I + i) * taps + tap]);
  } else {                           // [tap'][i][o], taps rotated by 180 degrees
    const int o = idx % O, i = (idx / O) % I, tp = idx / ((size_t)I * O);
    out[idx] = f2bf(w[((size_t)o * I + i) * taps + (taps - 1 - tp)]);
  }
}

// dw[i] += sum over the slabs, in a fixed association (bit-reproducible): eight threads per group of four elements each add a
// contiguous range of slabs in order (four loads in flight), then lane 0 of the eight adds the eight partial sums in order.
// cols / dw_ld (ABI 9): the slab holds a compact [rows][cols] tile that goes to columns of a wider matrix, dw[r * dw_ld + c] (a 32-channel
// column slice of a weight gradient, or its first K' columns: two-layers-per-pass of the fused 1x1 backward); cols == 0: dw is contiguous.
template <bool VEC>
__device__ __forceinline__ void dw_reduce_body(float* __restrict__ dw, const float* __restrict__ slab, size_t total, int splits,
                                               unsigned block, float (*part)[8][4], const int cols = 0, const int dw_ld = 0) {
  constexpr int E = VEC ? 4 : 1;
  const int oi = threadIdx.x >> 3, j = threadIdx.x & 7;
  const size_t i = ((size_t)block * 32 + oi) * E;
  const int per = (splits + 7) >> 3;
  const int s0 = j * per, s1 = (s0 + per < splits) ? s0 + per : splits;
  float a[4] = {0.f, 0.f, 0.f, 0.f};
  if (i < total) {
    for (int s = s0; s < s1; ++s) {
      if (VEC) {
        const float4 b = *reinterpret_cast<const float4*>(slab + (size_t)s * total + i);
        a[0] += b.x; a[1] += b.y; a[2] += b.z; a[3] += b.w;
      } else {
        a[0] += slab[(size_t)s * total + i];
      }
    }
  }
#pragma unroll
  for (int e = 0; e < 4; ++e) part[oi][j][e] = a[e];
  __syncthreads();
  if (j == 0 && i < total) {
    float t[4] = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int k = 0; k < 8; ++k)
#pragma unroll
      for (int e = 0; e < 4; ++e) t[e] += part[oi][k][e];
    size_t di = i;
    if (cols) {                                   // (VEC: cols % 4 == 0, so the four elements stay in one row)
      const size_t r = i / (size_t)cols;
      di = r * (size_t)dw_ld + (i - r * (size_t)cols);
    }
    if (VEC) {
      float4 d = *reinterpret_cast<float4*>(dw + di);
      d.x += t[0]; d.y += t[1]; d.z += t[2]; d.w += t[3];
      *reinterpret_cast<float4*>(dw + di) = d;
    } else {
      dw[di] += t[0];
    }
  }
}

template <bool VEC>
__global__ __launch_bounds__(256) void dw_reduce_kernel(float* __restrict__ dw, const float* __restrict__ slab, size_t total, int splits,
                                                        int cols, int dw_ld) {
  __shared__ float part[32][8][4];
  dw_reduce_body<VEC>(dw, slab, total, splits, blockIdx.x, part, cols, dw_ld);
}

// The same sums for MANY weight gradients in one launch (cx_dw_reduce_table): descriptor d owns blocks [first_block_d,
// first_block_{d+1}); a block finds its descriptor by bisection (uniform per block) and runs the body above, so every dw element
// sees exactly the additions, in exactly the order, of its own cx_dw_reduce launch.
__global__ __launch_bounds__(256) void dw_reduce_table_kernel(const CxReduceDesc* __restrict__ tab, int n) {
  __shared__ float part[32][8][4];
  int lo = 0, hi = n - 1;
  const int b = (int)blockIdx.x;
  while (lo < hi) {
    const int mid = (lo + hi + 1) >> 1;
    if (tab[mid].first_block <= b) lo = mid; else hi = mid - 1;
  }
  const CxReduceDesc d = tab[lo];
  const unsigned block = (unsigned)(b - d.first_block);
  if (d.vec) dw_reduce_body<true>(d.dw, d.slab, (size_t)d.total, d.splits, block, part, d.cols, d.dw_ld);
  else dw_reduce_body<false>(d.dw, d.slab, (size_t)d.total, d.splits, block, part, d.cols, d.dw_ld);
}

// one launch for every conv weight of a model: blockIdx.y = descriptor, blockIdx.x strides over its (output, input) channel pairs.
// A thread owns one pair: it reads the pair's kh*kw taps (contiguous fp32 in OIHW) and writes one bf16 into each tap plane; the
// pairs run in the destination's order (input channel fastest, or output channel fastest in the transposed layout), so a wave
// writes 128 contiguous bytes per tap and reads whole 36-byte runs.  (Element-per-thread in destination order re-fetched every
// source line once per tap: 5.6 GB of reads for ResNet152's 60 M weights.)
__global__ void pack_table_kernel(const float* __restrict__ flat, bf16* __restrict__ packed, const CxPackDesc* __restrict__ table) {
  const CxPackDesc d = table[blockIdx.y];
  const float* w = flat + d.src_off;
  bf16* out = packed + d.dst_off;
  const int O = d.O, I = d.I, taps = d.kh * d.kw;
  if (d.stem) {
    const size_t total = (size_t)7 * O * 32;
    for (size_t idx = (size_t)blockIdx.x * blockDim.x + threadIdx.x; idx < total; idx += (size_t)gridDim.x * blockDim.x) {
      const int k = idx % 32, o = (idx / 32) % O, ky = idx / (32 * (size_t)O);
      const int kx = (k >> 2) - 1, ch = k & 3;
      out[idx] = f2bf((kx >= 0 && ch < 3) ? w[((size_t)(o * 3 + ch) * 7 + ky) * 7 + kx] : 0.f);
    }
    return;
  }
  const size_t pairs = (size_t)O * I;
  for (size_t pidx = (size_t)blockIdx.x * blockDim.x + threadIdx.x; pidx < pairs; pidx += (size_t)gridDim.x * blockDim.x) {
    const int o = d.transpose ? (int)(pidx % O) : (int)(pidx / I);
    const int i = d.transpose ? (int)(pidx / O) : (int)(pidx % I);
    const float* src = w + ((size_t)o * I + i) * taps;
    for (int t = 0; t < taps; ++t) out[(size_t)(d.transpose ? taps - 1 - t : t) * pairs + pidx] = f2bf(src[t]);
  }
}

__global__ void nchw3_to_nhwc4_kernel(const float* __restrict__ x, bf16* __restrict__ y, size_t hw, size_t total) {
  const size_t idx = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (idx >= total) return;
  const size_t b = idx / hw, p = idx - b * hw;
  const float* src = x + b * 3 * hw + p;
  U64 o;
  o.e[0] = f2bf(src[0]);
  o.e[1] = f2bf(src[hw]);
  o.e[2] = f2bf(src[2 * hw]);
  o.e[3] = f2bf(0.f);
  *reinterpret_cast<uint2*>(y + idx * 4) = o.u;
}

__global__ void nchw3_to_nhwc4_f32_kernel(const float* __restrict__ x, float* __restrict__ y, size_t hw, size_t total) {
  const size_t idx = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (idx >= total) return;
  const size_t b = idx / hw, p = idx - b * hw;
  const float* src = x + b * 3 * hw + p;
  *reinterpret_cast<float4*>(y + idx * 4) = make_float4(src[0], src[hw], src[2 * hw], 0.f);
}

__global__ void u8_to_nhwc4_f32_kernel(const uint8_t* __restrict__ x, float* __restrict__ y, float scale, float shift, size_t total) {
  const size_t idx = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (idx >= total) return;
  const float g = fmaf((float)x[idx], scale, shift);
  *reinterpret_cast<float4*>(y + idx * 4) = make_float4(g, g, g, 0.f);
}

// fp32 storage mode: the same table, fp32 output; descriptors with stem = 1 produce [49 taps][O][4] (the stem is a plain 7x7
// convolution over the zero-padded 4-channel image there)
__global__ void pack_table_f32_kernel(const float* __restrict__ flat, float* __restrict__ packed, const CxPackDesc* __restrict__ table) {
  const CxPackDesc d = table[blockIdx.y];
  const float* w = flat + d.src_off;
  float* out = packed + d.dst_off;
  const int O = d.O, I = d.I, taps = d.kh * d.kw;
  const int Ip = d.stem ? 4 : I;
  const size_t total = (size_t)taps * O * Ip;
  for (size_t idx = (size_t)blockIdx.x * blockDim.x + threadIdx.x; idx < total; idx += (size_t)gridDim.x * blockDim.x) {
    float v;
    if (!d.transpose) {
      const int i = idx % Ip, o = (idx / Ip) % O, tap = idx / ((size_t)Ip * O);
      v = i < I ? w[((size_t)o * I + i) * taps + tap] : 0.f;
    } else {
      const int o = idx % O, i = (idx / O) % I, tp = idx / ((size_t)I * O);
      v = w[((size_t)o * I + i) * taps + (taps - 1 - tp)];
    }
    out[idx] = v;
  }
}

// uint8 grey image -> the three identical whitened channels of the reference transform chain, NHWC4 bf16, 16 pixels per thread
__global__ void u8_to_nhwc4_kernel(const uint8_t* __restrict__ x, bf16* __restrict__ y, float scale, float shift, size_t total16) {
  const size_t idx = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (idx >= total16) return;
  const uint4 v = *reinterpret_cast<const uint4*>(x + idx * 16);
  const uint32_t w[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
  for (int q = 0; q < 4; ++q) {
    U128 o0, o1;                                     // 2 x (2 pixels x 4 channels)
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      const bf16 g = f2bf(fmaf((float)((w[q] >> (8 * e)) & 0xffu), scale, shift));
      U128& o = e < 2 ? o0 : o1;
      const int k = (e & 1) * 4;
      o.e[k] = g; o.e[k + 1] = g; o.e[k + 2] = g; o.e[k + 3] = f2bf(0.f);
    }
    *reinterpret_cast<uint4*>(y + (idx * 16 + q * 4) * 4) = o0.u;
    *reinterpret_cast<uint4*>(y + (idx * 16 + q * 4 + 2) * 4) = o1.u;
  }
}

// Row reduction shared by the coefficient kernels: a 1024-thread workgroup owns 16 channels; thread (q, j) sums rows q, q + 64, ...
// of channel j with four loads in flight (added in row order), the 64 partial sums meet in LDS and are added in q order.  The
// order is fixed, so the result does not depend on scheduling.
template <typename T>
__device__ __forceinline__ void reduce_rows16(const float* __restrict__ a, const float* __restrict__ b, int rows, int rstride, int ch,
                                              T (*part)[64][17], T& ta, T& tb) {
  const int j = threadIdx.x & 15, q = threadIdx.x >> 4;
  T sa = 0, sb = 0;
  int r = q;
  for (; r + 192 < rows; r += 256) {
    const float a0 = a[(size_t)r * rstride + ch], a1 = a[(size_t)(r + 64) * rstride + ch];
    const float a2 = a[(size_t)(r + 128) * rstride + ch], a3 = a[(size_t)(r + 192) * rstride + ch];
    const float b0 = b[(size_t)r * rstride + ch], b1 = b[(size_t)(r + 64) * rstride + ch];
    const float b2 = b[(size_t)(r + 128) * rstride + ch], b3 = b[(size_t)(r + 192) * rstride + ch];
    sa += (T)a0; sa += (T)a1; sa += (T)a2; sa += (T)a3;
    sb += (T)b0; sb += (T)b1; sb += (T)b2; sb += (T)b3;
  }
  for (; r < rows; r += 64) {
    sa += (T)a[(size_t)r * rstride + ch];
    sb += (T)b[(size_t)r * rstride + ch];
  }
  part[0][q][j] = sa;
  part[1][q][j] = sb;
  __syncthreads();
  ta = 0; tb = 0;
  if (q == 0) {
#pragma unroll 8
    for (int k = 0; k < 64; ++k) { ta += part[0][k][j]; tb += part[1][k][j]; }
  }
}

// Both coefficient kernels reduce `replicas` rows per channel (16 atomic replicas, or the per-workgroup rows of a
// CxConv.stat_det launch: hundreds to thousands).  A 256-thread workgroup owns 16 channels: thread (q, j) sums rows q, q + 16, ...
// of channel j (64-B row segments per 16 lanes), the 16 partial sums meet in LDS and are added in q order -- a fixed order, so
// the result does not depend on scheduling.
__global__ __launch_bounds__(1024) void bn_coef_kernel(const float* sum, const float* sq, float count, const float* gamma,
                                                       const float* beta, float eps, float momentum, float* rmean, float* rvar,
                                                       float* scale, float* shift, float* mean, float* rstd, int C, int replicas,
                                                       int rstride) {
  __shared__ double part[2][64][17];
  const int j = threadIdx.x & 15, q = threadIdx.x >> 4;
  const int c = blockIdx.x * 16 + j;
  const int cc = c < C ? c : C - 1;
  double ts, tq;
  reduce_rows16<double>(sum, sq, replicas, rstride, cc, part, ts, tq);
  if (q != 0 || c >= C) return;
  const float g = gamma ? gamma[c] : 1.f, b = beta ? beta[c] : 0.f;
  const float rm0 = rmean ? rmean[c] : 0.f, rv0 = rvar ? rvar[c] : 0.f;
  const double m = ts / count;
  double v = tq / count - m * m;
  if (v < 0) v = 0;
  const float r = (float)(1.0 / sqrt(v + (double)eps));
  const float sc = g * r;
  if (scale) scale[c] = sc;
  if (shift) shift[c] = b - (float)m * sc;
  if (mean) mean[c] = (float)m;
  if (rstd) rstd[c] = r;
  if (rmean) rmean[c] = (1.f - momentum) * rm0 + momentum * (float)m;
  if (rvar) rvar[c] = (1.f - momentum) * rv0 + momentum * (float)(count > 1.f ? v * count / (count - 1.0) : v);
}

// BatchNorm coefficients of one layer from per-channel moments that already exist (dense blocks: a channel's batch mean / rstd
// are computed once, when the channel is produced; every later norm1 over the concatenation re-uses them with its own gamma /
// beta / running buffers).  Channels [c_lo, c_lo + c_n) are "fresh": their moments are first reduced from `rows` statistic rows
// (sum / sq at row pitch rstride, element c - c_lo) and written to mean / rstd.
__global__ __launch_bounds__(1024) void bn_coef_moments_kernel(float* mean, float* rstd, float count, const float* gamma,
                                                               const float* beta, float eps, float momentum, float* rmean, float* rvar,
                                                               float* scale, float* shift, int C, const float* sum, const float* sq,
                                                               int rows, int rstride, int c_lo, int c_n) {
  __shared__ double part[2][64][17];
  const int j = threadIdx.x & 15, q = threadIdx.x >> 4;
  const int c = blockIdx.x * 16 + j;
  const int cc = c < C ? c : C - 1;
  // block-uniform: does this group of 16 channels touch the fresh range?
  const int g0 = blockIdx.x * 16;
  const bool any_fresh = c_n > 0 && g0 < c_lo + c_n && g0 + 16 > c_lo;
  float m, r;
  if (any_fresh) {
    const bool fresh = cc >= c_lo && cc < c_lo + c_n;
    double ts, tq;
    reduce_rows16<double>(sum, sq, rows, rstride, fresh ? cc - c_lo : 0, part, ts, tq);
    if (q != 0 || c >= C) return;
    if (fresh) {
      const double md = ts / count;
      double v = tq / count - md * md;
      if (v < 0) v = 0;
      m = (float)md;
      r = (float)(1.0 / sqrt(v + (double)eps));
      mean[c] = m;
      rstd[c] = r;
    } else {
      m = mean[c];
      r = rstd[c];
    }
  } else {
    if (q != 0 || c >= C) return;
    m = mean[c];
    r = rstd[c];
  }
  const float g = gamma ? gamma[c] : 1.f, b = beta ? beta[c] : 0.f;
  const float sc = g * r;
  if (scale) scale[c] = sc;
  if (shift) shift[c] = b - m * sc;
  if (rmean) rmean[c] = (1.f - momentum) * rmean[c] + momentum * m;
  if (rvar) {
    const float v = fmaxf(1.f / (r * r) - eps, 0.f);                 // biased batch variance back from rstd
    rvar[c] = (1.f - momentum) * rvar[c] + momentum * (count > 1.f ? v * count / (count - 1.f) : v);
  }
}

// dst[c] += sum over rows (row order): the tall ordered sum behind per-workgroup partial vectors (attention table gradients,
// EfficientNet per-channel sums)
__global__ __launch_bounds__(1024) void rows_reduce_add_kernel(float* __restrict__ dst, const float* __restrict__ rows, int n_rows, int C,
                                                               int rstride, int assign) {
  __shared__ float part[2][64][17];
  const int j = threadIdx.x & 15, q = threadIdx.x >> 4;
  const int c = blockIdx.x * 16 + j;
  const int cc = c < C ? c : C - 1;
  float s, unused;
  reduce_rows16<float>(rows, rows, n_rows, rstride, cc, part, s, unused);
  if (q != 0 || c >= C) return;
  dst[c] = assign ? s : dst[c] + s;
}

__global__ void bn_coef_eval_kernel(const float* rmean, const float* rvar, const float* gamma, const float* beta,
                                    float eps, float* scale, float* shift, float* mean, float* rstd, int C) {
  const int c = blockIdx.x * blockDim.x + threadIdx.x;
  if (c >= C) return;
  const float r = 1.f / sqrtf(rvar[c] + eps);
  const float g = gamma ? gamma[c] : 1.f, b = beta ? beta[c] : 0.f;
  if (scale) scale[c] = g * r;
  if (shift) shift[c] = b - rmean[c] * g * r;
  if (mean) mean[c] = rmean[c];
  if (rstd) rstd[c] = r;
}

__global__ __launch_bounds__(1024) void bn_bwd_coef_kernel(const float* S1, const float* S2, float count, const float* gamma,
                                                           const float* mean, const float* rstd, float* dgamma, float* dbeta, float* A,
                                                           float* Bc, float* pa, float* pb, float* pc, int C, int replicas, int rstride,
                                                           float* qa, float* qb, float* qc, int q_lo, int q_n) {
  __shared__ float part[2][64][17];
  const int j = threadIdx.x & 15, q = threadIdx.x >> 4;
  const int c = blockIdx.x * 16 + j;
  const int cc = c < C ? c : C - 1;
  float s1, s2;
  reduce_rows16<float>(S1, S2, replicas, rstride, cc, part, s1, s2);
  if (q != 0 || c >= C) return;
  const float g = gamma ? gamma[c] : 1.f, r = rstd[c], mu = mean[c];
  if (dgamma) dgamma[c] += s2;
  if (dbeta) dbeta[c] += s1;
  const float inv = 1.f / count;
  float a_new = 0.f, b_new = 0.f;
  if (A) { a_new = A[c] + r * g * s1 * inv; A[c] = a_new; }
  if (Bc) { b_new = Bc[c] + r * g * s2 * inv; Bc[c] = b_new; }
  if (qa && c >= q_lo && c < q_lo + q_n) {      // cx_bn_bwd_slice_coef for the channels whose A / B are final after this consumer
    const float rb = r * b_new;
    qa[c - q_lo] = 1.f;
    qb[c - q_lo] = -rb;
    qc[c - q_lo] = mu * rb - a_new;
  }
  if (pa) {
    pa[c] = g * r;
    pb[c] = -g * r * r * s2 * inv;
    pc[c] = g * r * (mu * r * s2 - s1) * inv;
  }
}

// Frozen (eval-mode) form of bn_bwd_coef_kernel: y = gamma * (x - m) * r + beta with the running statistics m and
// r = 1 / sqrt(running_var + eps), so dx = gamma * r * dy and there are no batch-statistic terms.  The producer reduced
// S1 = sum dy and S2 = sum dy * (x - mu_b) * r_b against the basis (mu_b, r_b) it read (`mean` / `rstd`), hence
//   dgamma += sum dy * (x - m) * r = S2 * (r / r_b) + r * (mu_b - m) * S1    (exactly S2 when the basis is the running statistics)
//   dbeta  += S1,   pa = gamma * r, pb = pc = 0,   slice coefficients (qa, qb, qc) = (1, 0, 0).
// r is formed as bn_coef_eval_kernel forms it, so pa equals the forward's scale bit for bit.
__global__ __launch_bounds__(1024) void bn_bwd_coef_eval_kernel(const float* S1, const float* S2, const float* mean, const float* rstd,
                                                                const float* rmean, const float* rvar, const float* gamma, float eps,
                                                                float* dgamma, float* dbeta, float* pa, float* pb, float* pc, int C,
                                                                int replicas, int rstride, float* qa, float* qb, float* qc, int q_lo,
                                                                int q_n) {
  __shared__ float part[2][64][17];
  const int j = threadIdx.x & 15, q = threadIdx.x >> 4;
  const int c = blockIdx.x * 16 + j;
  const int cc = c < C ? c : C - 1;
  float s1, s2;
  reduce_rows16<float>(S1, S2, replicas, rstride, cc, part, s1, s2);
  if (q != 0 || c >= C) return;
  const float g = gamma ? gamma[c] : 1.f;
  const float r = 1.f / sqrtf(rvar[c] + eps);
  if (dgamma) dgamma[c] += s2 * (r / rstd[c]) + r * (mean[c] - rmean[c]) * s1;
  if (dbeta) dbeta[c] += s1;
  if (qa && c >= q_lo && c < q_lo + q_n) {
    qa[c - q_lo] = 1.f;
    qb[c - q_lo] = 0.f;
    qc[c - q_lo] = 0.f;
  }
  if (pa) {
    pa[c] = g * r;
    pb[c] = 0.f;
    pc[c] = 0.f;
  }
}

__global__ void bn_bwd_slice_coef_kernel(const float* A, const float* Bc, const float* mean, const float* rstd,
                                         float* pa, float* pb, float* pc, int C) {
  const int c = blockIdx.x * blockDim.x + threadIdx.x;
  if (c >= C) return;
  const float rb = rstd[c] * Bc[c];
  pa[c] = 1.f;
  pb[c] = -rb;
  pc[c] = mean[c] * rb - A[c];
}

// ------------------------------------------------------------------------------------------------
// stem: BN0 + ReLU + maxpool 3x3 s2 p1, arg-max recorded (uint8, window position 0..8)
template <typename T>
__global__ __launch_bounds__(256) void bnrelu_maxpool_fwd_kernel(const T* __restrict__ x, const float* __restrict__ sc,
                                                                 const float* __restrict__ sh, T* __restrict__ y,
                                                                 uint8_t* __restrict__ amax, float* g1, float* g2, int B,
                                                                 int H, int W, int C, int ldy, int det) {
  extern __shared__ float lds[];
  const int CP = C / 8;
  for (int i = threadIdx.x; i < 2 * C; i += blockDim.x) lds[i] = 0.f;
  __syncthreads();
  const int Ho = H / 2, Wo = W / 2;
  const int cq = threadIdx.x % CP;
  float fsc[8], fsh[8], s1[8], s2[8];
#pragma unroll
  for (int j = 0; j < 8; ++j) { fsc[j] = sc[cq * 8 + j]; fsh[j] = sh[cq * 8 + j]; s1[j] = s2[j] = 0.f; }
  const size_t npix = (size_t)B * Ho * Wo;
  const size_t ppb = blockDim.x / CP;
  // (neighbouring image rows share window reads: the remap keeps them on one XCD's L2 instead of eight)
  for (size_t pix = (size_t)xcd_remap(blockIdx.x, gridDim.x) * ppb + threadIdx.x / CP; pix < npix; pix += (size_t)gridDim.x * ppb) {
    const int b = pix / ((size_t)Ho * Wo);
    const int rem = pix - (size_t)b * Ho * Wo;
    const int oy = rem / Wo, ox = rem - oy * Wo;
    float best[8];
    int bi[8];
#pragma unroll
    for (int j = 0; j < 8; ++j) { best[j] = -1.f; bi[j] = 0; }
    // all nine window loads go out first on clamped addresses (a branch around a load serialises them); taps outside the image
    // are masked when compared
    typename V8<T>::raw wv[9];
    bool wok[9];
#pragma unroll
    for (int t = 0; t < 9; ++t) {
      const int iy = 2 * oy - 1 + t / 3, ix = 2 * ox - 1 + t % 3;
      wok[t] = iy >= 0 && iy < H && ix >= 0 && ix < W;
      const int iyc = min(max(iy, 0), H - 1), ixc = min(max(ix, 0), W - 1);
      wv[t] = V8<T>::ld(x + ((size_t)(b * H + iyc) * W + ixc) * C + cq * 8);
    }
#pragma unroll
    for (int t = 0; t < 9; ++t) {
#pragma unroll
      for (int j = 0; j < 8; ++j) {
        const float a = fmaxf(fmaf(V8<T>::get(wv[t], j), fsc[j], fsh[j]), 0.f);
        if (wok[t] && a > best[j]) { best[j] = a; bi[j] = t; }
      }
    }
    uint8_t idx[8];
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      const float rv = V8<T>::rnd(best[j]);
      s1[j] += rv;
      s2[j] += rv * rv;
      idx[j] = (uint8_t)bi[j];
    }
    V8<T>::st(y + pix * ldy + cq * 8, best);
    *reinterpret_cast<uint2*>(amax + pix * C + cq * 8) = *reinterpret_cast<const uint2*>(idx);
  }
  if (g1) block_stats_flush(s1, s2, cq, C, lds, g1, g2, det);
}

template <typename T>
__global__ __launch_bounds__(256) void bnrelu_maxpool_bwd_kernel(
    const T* __restrict__ x, const float* __restrict__ sc, const float* __restrict__ sh, const float* __restrict__ mean,
    const float* __restrict__ rstd, const uint8_t* __restrict__ amax, const T* __restrict__ g, const T* __restrict__ gx,
    const float* __restrict__ ga, const float* __restrict__ gb, const float* __restrict__ gc, T* __restrict__ dz, float* S1,
    float* S2, int B, int H, int W, int C, int ldg, int ldgx, int det) {
  extern __shared__ float lds[];
  const int CP = C / 8;
  for (int i = threadIdx.x; i < 2 * C; i += blockDim.x) lds[i] = 0.f;
  __syncthreads();
  const int Ho = H / 2, Wo = W / 2;
  const int cq = threadIdx.x % CP;
  float fsc[8], fsh[8], fmu[8], fr[8], fa[8], fb[8], fc[8], s1[8], s2[8];
#pragma unroll
  for (int j = 0; j < 8; ++j) {
    const int c = cq * 8 + j;
    fsc[j] = sc[c]; fsh[j] = sh[c]; fmu[j] = mean[c]; fr[j] = rstd[c];
    fa[j] = ga[c]; fb[j] = gb[c]; fc[j] = gc[c];
    s1[j] = s2[j] = 0.f;
  }
  // A thread owns a 2x2 block of input pixels = the pixels (2a+dy, 2b+dx) of pooled position (a, b), 8 channels.  The four
  // windows (a+wy, b+wx) are the only ones that contain any of them: pixel (dy,dx) sits at tap (1+dy-2wy, 1+dx-2wx) of window
  // (wy,wx) when wy <= dy and wx <= dx.  One pass of 12 window loads therefore serves four pixels (a thread per pixel issued
  // 12 loads each, 4x the pooled tensors through L1: the kernel ran at 2.1 TB/s of HBM traffic behind its own address stream).
  const size_t nblk = (size_t)B * Ho * Wo;
  const size_t ppb = blockDim.x / CP;
  for (size_t blk = (size_t)xcd_remap(blockIdx.x, gridDim.x) * ppb + threadIdx.x / CP; blk < nblk; blk += (size_t)gridDim.x * ppb) {
    const int b = blk / ((size_t)Ho * Wo);
    const int rem = blk - (size_t)b * Ho * Wo;
    const int a = rem / Wo, bb = rem - a * Wo;
    uint2 wi[4];
    typename V8<T>::raw wg[4], wx[4], xin[4];
    bool wok[4];
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      const int oy = a + (k >> 1), ox = bb + (k & 1);
      wok[k] = oy < Ho && ox < Wo;
      const int oyc = oy < Ho ? oy : Ho - 1, oxc = ox < Wo ? ox : Wo - 1;
      const size_t op = ((size_t)b * Ho + oyc) * Wo + oxc;
      wi[k] = *reinterpret_cast<const uint2*>(amax + op * C + cq * 8);
      wg[k] = V8<T>::ld(g + op * ldg + cq * 8);
      wx[k] = V8<T>::ld(gx + op * ldgx + cq * 8);
    }
    const size_t p00 = ((size_t)(b * H + 2 * a) * W + 2 * bb);
#pragma unroll
    for (int q = 0; q < 4; ++q) xin[q] = V8<T>::ld(x + (p00 + (size_t)(q >> 1) * W + (q & 1)) * C + cq * 8);
    float acc[4][8];
#pragma unroll
    for (int q = 0; q < 4; ++q)
#pragma unroll
      for (int j = 0; j < 8; ++j) acc[q][j] = 0.f;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      const uint8_t* idx = reinterpret_cast<const uint8_t*>(&wi[k]);
      const int wy = k >> 1, wxx = k & 1;
#pragma unroll
      for (int j = 0; j < 8; ++j) {
        const float cg = wok[k] ? fmaf(V8<T>::get(wg[k], j), fa[j], fmaf(V8<T>::get(wx[k], j), fb[j], fc[j])) : 0.f;
        const int t = idx[j];
#pragma unroll
        for (int q = 0; q < 4; ++q) {
          const int dy = q >> 1, dx = q & 1;
          if (wy <= dy && wxx <= dx) {            // compile-time
            const int tap = (1 + dy - 2 * wy) * 3 + (1 + dx - 2 * wxx);
            acc[q][j] += (t == tap) ? cg : 0.f;
          }
        }
      }
    }
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      float o[8];
#pragma unroll
      for (int j = 0; j < 8; ++j) {
        const float xf = V8<T>::get(xin[q], j);
        const float d = (fmaf(xf, fsc[j], fsh[j]) > 0.f) ? acc[q][j] : 0.f;
        s1[j] += d;
        s2[j] += d * (xf - fmu[j]) * fr[j];
        o[j] = d;
      }
      V8<T>::st(dz + (p00 + (size_t)(q >> 1) * W + (q & 1)) * C + cq * 8, o);
    }
  }
  block_stats_flush(s1, s2, cq, C, lds, S1, S2, det);
}

// ------------------------------------------------------------------------------------------------
// head
template <typename T>
__global__ void gap_bnrelu_kernel(const T* __restrict__ x, const float* __restrict__ sc, const float* __restrict__ sh,
                                  float* __restrict__ pooled, int B, int HW, int C, int ldx) {
  const int CP = C / 8;
  const size_t idx = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (idx >= (size_t)B * CP) return;
  const int b = idx / CP, cq = idx % CP;
  float fsc[8], fsh[8], acc[8];
#pragma unroll
  for (int j = 0; j < 8; ++j) { fsc[j] = sc[cq * 8 + j]; fsh[j] = sh[cq * 8 + j]; acc[j] = 0.f; }
  for (int p = 0; p < HW; ++p) {
    const typename V8<T>::raw v = V8<T>::ld(x + ((size_t)b * HW + p) * ldx + cq * 8);
#pragma unroll
    for (int j = 0; j < 8; ++j) acc[j] += fmaxf(fmaf(V8<T>::get(v, j), fsc[j], fsh[j]), 0.f);
  }
  const float inv = 1.f / HW;
#pragma unroll
  for (int j = 0; j < 8; ++j) pooled[(size_t)b * C + cq * 8 + j] = acc[j] * inv;
}

__global__ void linear_kernel(const float* __restrict__ pooled, const float* __restrict__ w, const float* __restrict__ bias,
                              float* __restrict__ logits, int C, int n_classes) {
  // one block per batch element; wave w handles classes w, w+4, ...
  const int b = blockIdx.x, lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  for (int k = wave; k < n_classes; k += blockDim.x / 64) {
    float acc = 0.f;
    for (int c = lane; c < C; c += 64) acc += pooled[(size_t)b * C + c] * w[(size_t)k * C + c];
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) acc += __shfl_xor(acc, d);
    if (lane == 0) logits[(size_t)b * n_classes + k] = acc + (bias ? bias[k] : 0.f);
  }
}

// grid (C/256, n + B): row y < n computes dW[y][:] (and db[y]), row y >= n computes dpooled[y-n][:]
__global__ void head_bwd_kernel(const float* __restrict__ dlogits, const float* __restrict__ pooled, const float* __restrict__ w,
                                float* dw, float* db, float* __restrict__ dpooled, int B, int C, int n) {
  const int c = blockIdx.x * blockDim.x + threadIdx.x;
  const int y = blockIdx.y;
  if (y < n) {
    if (c < C) {
      float acc = 0.f;
      for (int b = 0; b < B; ++b) acc = fmaf(dlogits[b * n + y], pooled[(size_t)b * C + c], acc);
      dw[(size_t)y * C + c] += acc;
    }
    if (c == 0 && db) {
      float acc = 0.f;
      for (int b = 0; b < B; ++b) acc += dlogits[b * n + y];
      db[y] += acc;
    }
  } else if (c < C) {
    const int b = y - n;
    float acc = 0.f;
    for (int k = 0; k < n; ++k) acc = fmaf(dlogits[b * n + k], w[(size_t)k * C + c], acc);
    dpooled[(size_t)b * C + c] = acc;
  }
}

template <typename T>
__global__ void gap_relu_bn_bwd_kernel(const float* __restrict__ dpooled, const T* __restrict__ x, const float* __restrict__ sc,
                                       const float* __restrict__ sh, const float* __restrict__ mean, const float* __restrict__ rstd,
                                       const float* __restrict__ escale, T* __restrict__ g, float* S1, float* S2, int B, int HW,
                                       int C, int ldx, int ldg, int det) {
  const int CP = C / 8;
  const size_t idx = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (idx >= (size_t)B * CP) return;
  const int b = idx / CP, cq = idx % CP;
  float fsc[8], fsh[8], fmu[8], fr[8], fe[8], dp[8], s1[8], s2[8];
  const float inv = 1.f / HW;
#pragma unroll
  for (int j = 0; j < 8; ++j) {
    const int c = cq * 8 + j;
    fsc[j] = sc[c]; fsh[j] = sh[c]; fmu[j] = mean[c]; fr[j] = rstd[c]; fe[j] = escale[c];
    dp[j] = dpooled[(size_t)b * C + c] * inv;
    s1[j] = s2[j] = 0.f;
  }
  for (int p = 0; p < HW; ++p) {
    const typename V8<T>::raw v = V8<T>::ld(x + ((size_t)b * HW + p) * ldx + cq * 8);
    float o[8];
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      const float xf = V8<T>::get(v, j);
      const float d = (fmaf(xf, fsc[j], fsh[j]) > 0.f) ? dp[j] : 0.f;
      s1[j] += d;
      s2[j] += d * (xf - fmu[j]) * fr[j];
      o[j] = fe[j] * d;
    }
    V8<T>::st(g + ((size_t)b * HW + p) * ldg + cq * 8, o);
  }
#pragma unroll
  for (int j = 0; j < 8; ++j) {
    if (det) {                                  // row = image: B rows of C sums, one writer per element
      S1[(size_t)b * C + cq * 8 + j] = s1[j];
      S2[(size_t)b * C + cq * 8 + j] = s2[j];
    } else {
      atomicAdd(&S1[cq * 8 + j], s1[j]);
      atomicAdd(&S2[cq * 8 + j], s2[j]);
    }
  }
}

// transition backward glue: un-pool + ReLU/BN mask
template <typename T>
__global__ __launch_bounds__(256) void unpool2_mask_kernel(const T* __restrict__ d, const T* __restrict__ x,
                                                           const float* __restrict__ sc, const float* __restrict__ sh,
                                                           const float* __restrict__ mean, const float* __restrict__ rstd,
                                                           const float* __restrict__ escale, T* __restrict__ g, float* S1,
                                                           float* S2, int B, int H, int W, int C, int ldd, int ldx, int ldg, int det) {
  extern __shared__ float lds[];
  const int CP = C / 8;
  for (int i = threadIdx.x; i < 2 * C; i += blockDim.x) lds[i] = 0.f;
  __syncthreads();
  const int cq = threadIdx.x % CP;
  float fsc[8], fsh[8], fmu[8], fr[8], fe[8], s1[8], s2[8];
#pragma unroll
  for (int j = 0; j < 8; ++j) {
    const int c = cq * 8 + j;
    fsc[j] = sc[c]; fsh[j] = sh[c]; fmu[j] = mean[c]; fr[j] = rstd[c]; fe[j] = escale[c];
    s1[j] = s2[j] = 0.f;
  }
  const size_t npix = (size_t)B * H * W;
  const size_t ppb = blockDim.x / CP;
  const int Ho = H / 2, Wo = W / 2;
  // (C / 8 need not divide the workgroup: the trailing blockDim % CP threads idle with zero sums -- the padded widths of the CIFAR
  // DenseNet-BC twin, e.g. 280 channels = 35 chunks, run 245 threads of 256)
  const bool active = threadIdx.x < ppb * CP;
  // (neighbouring image rows share window reads: the remap keeps them on one XCD's L2 instead of eight)
  for (size_t pix = active ? (size_t)xcd_remap(blockIdx.x, gridDim.x) * ppb + threadIdx.x / CP : npix; pix < npix; pix += (size_t)gridDim.x * ppb) {
    const int b = pix / ((size_t)H * W);
    const int rem = pix - (size_t)b * H * W;
    const int iy = rem / W, ix = rem - iy * W;
    const size_t op = ((size_t)b * Ho + (iy >> 1)) * Wo + (ix >> 1);
    const typename V8<T>::raw dv = V8<T>::ld(d + op * ldd + cq * 8);
    const typename V8<T>::raw xv = V8<T>::ld(x + pix * ldx + cq * 8);
    float o[8];
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      const float xf = V8<T>::get(xv, j);
      const float dzv = (fmaf(xf, fsc[j], fsh[j]) > 0.f) ? 0.25f * V8<T>::get(dv, j) : 0.f;
      s1[j] += dzv;
      s2[j] += dzv * (xf - fmu[j]) * fr[j];
      o[j] = fe[j] * dzv;
    }
    V8<T>::st(g + pix * ldg + cq * 8, o);
  }
  block_stats_flush(s1, s2, cq, C, lds, S1, S2, det);
}

__global__ void affine2_inplace_kernel(bf16* __restrict__ dz, const bf16* __restrict__ x, const float* __restrict__ pa,
                                       const float* __restrict__ pb, const float* __restrict__ pc, size_t rows, int C) {
  const int CP = C / 8;
  const size_t total = rows * CP;
  for (size_t idx = (size_t)blockIdx.x * blockDim.x + threadIdx.x; idx < total; idx += (size_t)gridDim.x * blockDim.x) {
    const int cq = idx % CP;
    U128 u, v, o;
    u.u = *reinterpret_cast<const uint4*>(dz + idx * 8);
    v.u = *reinterpret_cast<const uint4*>(x + idx * 8);
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      const int c = cq * 8 + j;
      o.e[j] = f2bf(fmaf(bf2f(u.e[j]), pa[c], fmaf(bf2f(v.e[j]), pb[c], pc[c])));
    }
    *reinterpret_cast<uint4*>(dz + idx * 8) = o.u;
  }
}

// residual join: out = relu(a*pa + b*pb + pc)
// mask (optional): one bit per element, byte idx = chunk of 8 channels, bit j = out[8 idx + j] > 0 -- what the backward of the join
// needs of `out` (relu_bwd_stats_kernel), at 1/16 of its bytes
template <typename T>
__global__ void affine2_relu_kernel(const T* __restrict__ a, const T* __restrict__ b, const float* __restrict__ pa,
                                    const float* __restrict__ pb, const float* __restrict__ pc, T* __restrict__ out,
                                    uint8_t* __restrict__ mask, size_t rows, int C) {
  const int CP = C / 8;
  const size_t total = rows * CP;
  for (size_t idx = (size_t)blockIdx.x * blockDim.x + threadIdx.x; idx < total; idx += (size_t)gridDim.x * blockDim.x) {
    const int cq = idx % CP;
    const typename V8<T>::raw u = V8<T>::ld(a + idx * 8), v = V8<T>::ld(b + idx * 8);
    float o[8];
    unsigned m = 0;
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      const int c = cq * 8 + j;
      o[j] = V8<T>::rnd(fmaxf(fmaf(V8<T>::get(u, j), pa[c], fmaf(V8<T>::get(v, j), pb[c], pc[c])), 0.f));
      m |= (o[j] > 0.f ? 1u : 0u) << j;
    }
    V8<T>::st(out + idx * 8, o);
    if (mask) mask[cx_side_chunk(idx / CP, cq, rows, C)] = (uint8_t)m;
  }
}

// Residual join forward with the two-plane residual stream (common.h, cx_join2): out = relu(a * pa + (b [+ b_lo]) * pb + pc), stored as
// hi (bf16) + lo (int8) + sign bits.  The same arithmetic runs in the prologue of the next block's conv1 (conv_mm.hip, CX_PRO_JOIN);
// this pass is used where no such convolution follows (a downsample block's join, the last block) and by the tests as the yardstick.
template <int V>      // V 8-channel chunks per thread: 2 where C % 64 == 0 (every access 16 bytes wide: hi 2 x 16, lo 16), else 1
__global__ __launch_bounds__(256) void join_fwd_kernel(const uint4* __restrict__ a, const uint4* __restrict__ b, const uint8_t* __restrict__ b_lo,
                                                       const float* __restrict__ pa, const float* __restrict__ pb, const float* __restrict__ pc,
                                                       uint4* __restrict__ out, uint8_t* __restrict__ out_lo, uint8_t* __restrict__ mask,
                                                       size_t rows, int C) {
  const int CP = C / (8 * V);
  const size_t total = rows * CP;
  for (size_t idx = (size_t)blockIdx.x * blockDim.x + threadIdx.x; idx < total; idx += (size_t)gridDim.x * blockDim.x) {
    // V = 2 (C % 64 == 0): threads walk the side planes' order -- 4 threads = the 64 channels of a block, then the next row, then
    // the next block -- so the lo / sign-bit accesses of a wave are ONE contiguous run and the hi accesses whole 128-byte lines
    size_t m;
    int cq;                                                  // first chunk of this thread
    if (V == 2) {
      const size_t blk = idx / (rows * 4), r = idx - blk * (rows * 4);
      m = r >> 2;
      cq = (int)blk * 8 + (int)(r & 3) * 2;
    } else {
      m = idx / CP;
      cq = (int)(idx - m * CP);
    }
    const size_t side = cx_side_chunk(m, cq, rows, C);       // (V = 2: cq is even, the two chunks are neighbours in the blocked layout)
    const size_t hidx = m * (size_t)(C >> 3) + cq;           // chunk index in the row-major hi planes
    uint4 u[V], w[V];
    uint32_t lw[2 * V];
#pragma unroll
    for (int k = 0; k < V; ++k) u[k] = a[hidx + k], w[k] = b[hidx + k];
    if (b_lo) {
      if (V == 2) {
        const uint4 t = *reinterpret_cast<const uint4*>(b_lo + side * 8);
        lw[0] = t.x, lw[1] = t.y, lw[2] = t.z, lw[3] = t.w;
      } else {
        const uint2 t = *reinterpret_cast<const uint2*>(b_lo + side * 8);
        lw[0] = t.x, lw[1] = t.y;
      }
    } else {
#pragma unroll
      for (int k = 0; k < 2 * V; ++k) lw[k] = 0u;
    }
    uint32_t lo[2 * V], mk[V];
    uint4 o[V];
#pragma unroll
    for (int k = 0; k < V; ++k) {
      const int c0 = (cq + k) * 8;
      const uint32_t uw[4] = {u[k].x, u[k].y, u[k].z, u[k].w}, vw[4] = {w[k].x, w[k].y, w[k].z, w[k].w};
      uint32_t ow[4];
      lo[2 * k] = lo[2 * k + 1] = 0u;
      mk[k] = 0u;
#pragma unroll
      for (int j = 0; j < 4; ++j)
        ow[j] = cx_join2(uw[j], vw[j], b_lo != nullptr, lw[2 * k + (j >> 1)], j, pa[c0 + 2 * j], pa[c0 + 2 * j + 1], pb[c0 + 2 * j],
                         pb[c0 + 2 * j + 1], pc[c0 + 2 * j], pc[c0 + 2 * j + 1], out_lo != nullptr, lo[2 * k + (j >> 1)], mk[k]);
      o[k] = make_uint4(ow[0], ow[1], ow[2], ow[3]);
    }
#pragma unroll
    for (int k = 0; k < V; ++k) out[hidx + k] = o[k];
    if (out_lo) {
      if (V == 2) *reinterpret_cast<uint4*>(out_lo + side * 8) = make_uint4(lo[0], lo[1], lo[2], lo[3]);
      else *reinterpret_cast<uint2*>(out_lo + side * 8) = make_uint2(lo[0], lo[1]);
    }
    if (mask) {
      if (V == 2) *reinterpret_cast<uint16_t*>(mask + side) = (uint16_t)(mk[0] | (mk[V - 1] << 8));
      else mask[side] = (uint8_t)mk[0];
    }
  }
}

template <typename T>
__global__ __launch_bounds__(256) void relu_bwd_stats_kernel(const T* __restrict__ dout, const T* __restrict__ out,
                                                             const T* __restrict__ a, const float* __restrict__ mu_a,
                                                             const float* __restrict__ r_a, const T* __restrict__ b,
                                                             const float* __restrict__ mu_b, const float* __restrict__ r_b,
                                                             T* __restrict__ dz, float* S1, float* S2a, float* S2b, size_t rows,
                                                             int C, int det, const uint8_t* __restrict__ mask, int TA) {
  extern __shared__ float lds[];          // [3][C] (atomic mode) / [256][24] (deterministic rows)
  const int CP = C / 8;
  if (!det) {
    for (int i = threadIdx.x; i < 3 * C; i += blockDim.x) lds[i] = 0.f;
  }
  __syncthreads();
  // A thread keeps ONE chunk column cq for the whole grid-stride loop (its means / rstds live in registers): the TA = (256 / CP) * CP
  // leading threads of a workgroup are active, so the stride gridDim.x * T is a multiple of CP for any C % 8 == 0 (C <= 2048) --
  // e.g. the 160 / 320 / 640-wide joins of WRN-28-10 (attn_aug_conv.py:311-404) run 240 threads of 256
  float s1[8], s2[8], s3[8];
  const size_t total = rows * CP;
  const size_t stride = (size_t)gridDim.x * TA;
  const bool active = (int)threadIdx.x < TA;
  size_t idx = active ? (size_t)blockIdx.x * TA + threadIdx.x : total;
  const int cq = active ? (int)(idx % CP) : 0;
#pragma unroll
  for (int j = 0; j < 8; ++j) s1[j] = s2[j] = s3[j] = 0.f;
  float ma[8], ra_[8], mb[8], rb_[8];
#pragma unroll
  for (int j = 0; j < 8; ++j) {
    ma[j] = mu_a[cq * 8 + j]; ra_[j] = r_a[cq * 8 + j];
    mb[j] = b ? mu_b[cq * 8 + j] : 0.f; rb_[j] = b ? r_b[cq * 8 + j] : 0.f;
  }
  for (; idx < total; idx += stride) {
    typename V8<T>::raw o, bv;
    const typename V8<T>::raw g = V8<T>::ld(dout + idx * 8);
    unsigned mk = 0;
    if (mask) mk = mask[cx_side_chunk(idx / CP, cq, rows, C)];      // the forward's sign bits instead of the read of `out`
    else o = V8<T>::ld(out + idx * 8);
    const typename V8<T>::raw av = V8<T>::ld(a + idx * 8);
    if (b) bv = V8<T>::ld(b + idx * 8);
    float d[8];
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      const bool on = mask ? ((mk >> j) & 1u) != 0 : V8<T>::get(o, j) > 0.f;
      const float dzv = on ? V8<T>::get(g, j) : 0.f;
      s1[j] += dzv;
      s2[j] += dzv * (V8<T>::get(av, j) - ma[j]) * ra_[j];
      if (b) s3[j] += dzv * (V8<T>::get(bv, j) - mb[j]) * rb_[j];
      d[j] = dzv;
    }
    V8<T>::st(dz + idx * 8, d);
  }
  if (det) {               // one row per workgroup, partial sums of the threads sharing a chunk folded in thread order
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      lds[threadIdx.x * 24 + j] = s1[j];
      lds[threadIdx.x * 24 + 8 + j] = s2[j];
      lds[threadIdx.x * 24 + 16 + j] = s3[j];
    }
    __syncthreads();
    for (int c = threadIdx.x; c < C; c += blockDim.x) {
      const int chunk = c >> 3, j = c & 7;
      float t1 = 0.f, t2 = 0.f, t3 = 0.f;
      for (int t = chunk; t < TA; t += CP) {
        t1 += lds[t * 24 + j];
        t2 += lds[t * 24 + 8 + j];
        t3 += lds[t * 24 + 16 + j];
      }
      S1[(size_t)blockIdx.x * C + c] = t1;
      S2a[(size_t)blockIdx.x * C + c] = t2;
      if (b) S2b[(size_t)blockIdx.x * C + c] = t3;
    }
    return;
  }
  if (active) {
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      atomicAdd(&lds[cq * 8 + j], s1[j]);
      atomicAdd(&lds[C + cq * 8 + j], s2[j]);
      if (b) atomicAdd(&lds[2 * C + cq * 8 + j], s3[j]);
    }
  }
  __syncthreads();
  for (int c = threadIdx.x; c < C; c += blockDim.x) {
    atomicAdd(&S1[c], lds[c]);
    atomicAdd(&S2a[c], lds[C + c]);
    if (b) atomicAdd(&S2b[c], lds[2 * C + c]);
  }
}

__global__ void fill_kernel(float* p, float v, size_t n) {
  for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (size_t)gridDim.x * blockDim.x) p[i] = v;
}

__global__ void bf16_to_f32_nchw_kernel(const bf16* __restrict__ x, float* __restrict__ y, int HW, int C, int ldx, size_t total) {
  const size_t idx = (size_t)blockIdx.x * blockDim.x + threadIdx.x;     // over (b, c, p) output order
  if (idx >= total) return;
  const int p = idx % HW;
  const int c = (idx / HW) % C;
  const size_t b = idx / ((size_t)HW * C);
  y[idx] = bf2f(x[(b * HW + p) * ldx + c]);
}

// y[b][c][p] = act(x[b][p][c] * sc[c] + sh[c]) as fp32 NCHW: the feature map a forward hook on features.norm5 / layer4 / head[1] sees
__global__ void affine_to_f32_nchw_kernel(const bf16* __restrict__ x, const float* __restrict__ sc, const float* __restrict__ sh,
                                          int relu, float* __restrict__ y, int HW, int C, int ldx, size_t total) {
  const size_t idx = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (idx >= total) return;
  const int p = idx % HW;
  const int c = (idx / HW) % C;
  const size_t b = idx / ((size_t)HW * C);
  float v = bf2f(x[(b * HW + p) * ldx + c]);
  if (sc) v = fmaf(v, sc[c], sh[c]);
  y[idx] = relu ? fmaxf(v, 0.f) : v;
}

// Grad-CAM: cam[b][p] = relu(sum_c w[c] * relu(x[b][p][c]*sc[c]+sh[c]))   (chexpert.py:283-285 as executed)
__global__ void gradcam_map_kernel(const bf16* __restrict__ x, const float* __restrict__ sc, const float* __restrict__ sh,
                                   const float* __restrict__ w, float* __restrict__ cam, size_t npix, int C, int ldx, int inner_relu) {
  const int lane = threadIdx.x & 63;
  const size_t pix = (size_t)blockIdx.x * (blockDim.x / 64) + (threadIdx.x >> 6);
  if (pix >= npix) return;
  float acc = 0.f;
  for (int c = lane * 8; c < C; c += 512) {
    U128 v;
    v.u = *reinterpret_cast<const uint4*>(x + pix * ldx + c);
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      const float f = fmaf(bf2f(v.e[j]), sc[c + j], sh[c + j]);
      acc += w[c + j] * (inner_relu ? fmaxf(f, 0.f) : f);
    }
  }
#pragma unroll
  for (int d = 32; d >= 1; d >>= 1) acc += __shfl_xor(acc, d);
  if (lane == 0) cam[pix] = fmaxf(acc, 0.f);
}

// per image: (t - min) / (max - min + 1e-5), then bilinear upsample with align_corners=True (chexpert.py:289-296)
__global__ void cam_norm_upsample_kernel(const float* __restrict__ cam, float* __restrict__ out, int h, int w, int H, int W) {
  __shared__ float smin[256], smax[256];
  const int b = blockIdx.x;
  const float* c = cam + (size_t)b * h * w;
  float mn = 3.4e38f, mx = -3.4e38f;
  for (int i = threadIdx.x; i < h * w; i += blockDim.x) { mn = fminf(mn, c[i]); mx = fmaxf(mx, c[i]); }
  smin[threadIdx.x] = mn; smax[threadIdx.x] = mx;
  __syncthreads();
  for (int s = blockDim.x / 2; s > 0; s >>= 1) {
    if (threadIdx.x < s) { smin[threadIdx.x] = fminf(smin[threadIdx.x], smin[threadIdx.x + s]); smax[threadIdx.x] = fmaxf(smax[threadIdx.x], smax[threadIdx.x + s]); }
    __syncthreads();
  }
  mn = smin[0]; mx = smax[0];
  const float inv = 1.f / (mx - mn + 1e-5f);
  const float ry = H > 1 ? (float)(h - 1) / (H - 1) : 0.f, rx = W > 1 ? (float)(w - 1) / (W - 1) : 0.f;
  for (int i = threadIdx.x; i < H * W; i += blockDim.x) {
    const int Y = i / W, X = i - Y * W;
    const float fy = Y * ry, fx = X * rx;
    int y0 = (int)fy, x0 = (int)fx;
    if (y0 > h - 1) y0 = h - 1;
    if (x0 > w - 1) x0 = w - 1;
    const int y1 = min(y0 + 1, h - 1), x1 = min(x0 + 1, w - 1);
    const float ly = fy - y0, lx = fx - x0;
    const float v00 = (c[y0 * w + x0] - mn) * inv, v01 = (c[y0 * w + x1] - mn) * inv;
    const float v10 = (c[y1 * w + x0] - mn) * inv, v11 = (c[y1 * w + x1] - mn) * inv;
    out[(size_t)b * H * W + i] = (1.f - ly) * ((1.f - lx) * v00 + lx * v01) + ly * ((1.f - lx) * v10 + lx * v11);
  }
}

// ------------------------------------------------------------------------------------------------
// Brightness / contrast jitter of the decoded grey image on the GPU (the `_data_aug` rows of the reference README are its
// explore_data.ipynb cell 6: ColorJitter(brightness=0.25, contrast=0.25)).  torchvision tensor semantics on uint8:
//   brightness b: y = trunc(clamp(b * x, 0, 255))
//   contrast   c: y = trunc(clamp(c * x + (1 - c) * mean(x), 0, 255)), mean over the image (fp32)
// applied in the order `order[b]` says (0: brightness first).  One workgroup per image; the image lives in LDS between the
// passes (320 x 320 = 100 KB, 380 x 380 = 141 KB), so HBM sees one read and one write.
__global__ __launch_bounds__(1024) void u8_jitter_kernel(const uint8_t* __restrict__ x, uint8_t* __restrict__ y, int HW,
                                                         const float* __restrict__ bfac, const float* __restrict__ cfac,
                                                         const int* __restrict__ order) {
  extern __shared__ __attribute__((aligned(16))) unsigned char img[];      // [HW] image, then 32 floats of reduction scratch
  float* red = reinterpret_cast<float*>(img + HW);
  const int b = blockIdx.x, tid = threadIdx.x;
  const uint8_t* src = x + (size_t)b * HW;
  const float bf_ = bfac[b], cf = cfac[b];
  const bool bright_first = order[b] == 0;
  float sum = 0.f;
  for (int i = tid * 16; i < HW; i += 1024 * 16) {                // HW % 16 == 0
    uint4 v = *reinterpret_cast<const uint4*>(src + i);
    uint32_t w[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      uint32_t o = 0;
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        float p = (float)((w[q] >> (8 * e)) & 0xffu);
        if (bright_first) p = truncf(fminf(fmaxf(bf_ * p, 0.f), 255.f));
        sum += p;
        o |= ((uint32_t)p) << (8 * e);
      }
      w[q] = o;
    }
    *reinterpret_cast<uint4*>(img + i) = make_uint4(w[0], w[1], w[2], w[3]);
  }
  // deterministic block sum: lanes by shuffles, waves in order
#pragma unroll
  for (int d = 32; d >= 1; d >>= 1) sum += __shfl_xor(sum, d);
  if ((tid & 63) == 0) red[tid >> 6] = sum;
  __syncthreads();
  if (tid == 0) {
    float t = 0.f;
    for (int k = 0; k < 16; ++k) t += red[k];
    red[16] = t / (float)HW;
  }
  __syncthreads();
  const float mean = red[16];
  uint8_t* dst = y + (size_t)b * HW;
  for (int i = tid * 16; i < HW; i += 1024 * 16) {
    uint4 v = *reinterpret_cast<const uint4*>(img + i);
    uint32_t w[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      uint32_t o = 0;
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        float p = (float)((w[q] >> (8 * e)) & 0xffu);
        p = truncf(fminf(fmaxf(fmaf(cf, p, (1.f - cf) * mean), 0.f), 255.f));
        if (!bright_first) p = truncf(fminf(fmaxf(bf_ * p, 0.f), 255.f));
        o |= ((uint32_t)p) << (8 * e);
      }
      w[q] = o;
    }
    *reinterpret_cast<uint4*>(dst + i) = make_uint4(w[0], w[1], w[2], w[3]);
  }
}

// ---- dropout on a dense layer's new feature slice (torchvision `_DenseLayer.forward`: F.dropout(new_features, p, training), the
// DenseNet of attn_aug_conv.py:453, :479-481 hands drop_rate to torchvision's _DenseBlock).  The keep decision of element (pixel m, channel c) of layer `uid` is a
// counter-based hash of (seed, uid, m * C + c) -- nothing is stored: backward regenerates it.  (torch's Philox stream cannot be
// reproduced bit for bit outside torch; the tests feed the same decisions to the oracle.)
__device__ __forceinline__ uint32_t drop_mix(uint32_t h) {
  h ^= h >> 16; h *= 0x7feb352du; h ^= h >> 15; h *= 0x846ca68bu; h ^= h >> 16;
  return h;
}
__device__ __forceinline__ bool drop_keep(uint32_t seed_lo, uint32_t seed_hi, uint32_t uid, uint64_t idx, uint32_t thr) {
  uint32_t h = drop_mix((uint32_t)idx * 0x9e3779b1u + seed_lo);
  h = drop_mix(h ^ ((uint32_t)(idx >> 32) * 0x85ebca77u + uid * 0xc2b2ae3du + seed_hi));
  return h >= thr;
}

// forward, in place on the slice y[m * ld + c], c < C: y = keep ? y * scale : 0; one statistic row (sum, sum of squares of the stored
// result) per workgroup.  backward (BWD), in place on the gradient slice: g = keep ? scale * (qa g + qb x + qc) : 0 -- the deferred
// BatchNorm correction of the slice (the AFFINE2 prologue the 3x3 input-gradient kernel would apply) with the keep decision on top.
template <typename T, bool BWD>
__global__ __launch_bounds__(256) void dropout_slice_kernel(T* __restrict__ y, int ld, const T* __restrict__ x, int ldx,
                                                            const float* __restrict__ qa, const float* __restrict__ qb,
                                                            const float* __restrict__ qc, size_t rows, int C, float scale, uint32_t thr,
                                                            const int64_t* __restrict__ seed, uint32_t uid, float* S1, float* S2, int TA) {
  __shared__ float lds[256 * 16];
  const int CP = C / 8;
  const uint64_t sd = (uint64_t)seed[0];
  const uint32_t seed_lo = (uint32_t)sd, seed_hi = (uint32_t)(sd >> 32);
  const size_t total = rows * CP;
  const size_t stride = (size_t)gridDim.x * TA;
  const bool active = (int)threadIdx.x < TA;
  size_t idx = active ? (size_t)blockIdx.x * TA + threadIdx.x : total;
  const int cq = active ? (int)(idx % CP) : 0;
  float s1[8], s2[8], a_[8], b_[8], c_[8];
#pragma unroll
  for (int j = 0; j < 8; ++j) {
    s1[j] = s2[j] = 0.f;
    a_[j] = BWD ? qa[cq * 8 + j] : 0.f; b_[j] = BWD ? qb[cq * 8 + j] : 0.f; c_[j] = BWD ? qc[cq * 8 + j] : 0.f;
  }
  for (; idx < total; idx += stride) {
    const size_t m = idx / CP;
    T* py = y + m * ld + cq * 8;
    const typename V8<T>::raw v = V8<T>::ld(py);
    typename V8<T>::raw xv;
    if (BWD) xv = V8<T>::ld(x + m * ldx + cq * 8);
    float o[8];
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      const bool keep = drop_keep(seed_lo, seed_hi, uid, (uint64_t)m * C + cq * 8 + j, thr);
      float t = V8<T>::get(v, j);
      if (BWD) t = fmaf(a_[j], t, fmaf(b_[j], V8<T>::get(xv, j), c_[j]));
      o[j] = keep ? V8<T>::rnd(t * scale) : 0.f;
      s1[j] += o[j];
      s2[j] = fmaf(o[j], o[j], s2[j]);
    }
    V8<T>::st(py, o);
  }
  if (BWD || !S1) return;
#pragma unroll
  for (int j = 0; j < 8; ++j) {
    lds[threadIdx.x * 16 + j] = s1[j];
    lds[threadIdx.x * 16 + 8 + j] = s2[j];
  }
  __syncthreads();
  for (int c = threadIdx.x; c < C; c += blockDim.x) {       // partial sums of the threads sharing a chunk, folded in thread order
    const int chunk = c >> 3, j = c & 7;
    float t1 = 0.f, t2 = 0.f;
    for (int t = chunk; t < TA; t += CP) {
      t1 += lds[t * 16 + j];
      t2 += lds[t * 16 + 8 + j];
    }
    S1[(size_t)blockIdx.x * C + c] = t1;
    S2[(size_t)blockIdx.x * C + c] = t2;
  }
}

inline int grid_for(size_t n, int block, int cap = 4096) {
  size_t g = (n + block - 1) / block;
  if (g > (size_t)cap) g = cap;
  if (g < 1) g = 1;
  return (int)g;
}

template <typename T, bool BWD>
static int dropout_slice_t(void* y, int ld, const void* x, int ldx, const float* qa, const float* qb, const float* qc, int64_t rows, int C,
                           float p, const int64_t* seed, uint32_t uid, float* S1, float* S2, int stat_rows, void* stream) {
  if (!y || !seed || rows <= 0 || C <= 0 || (C % 8) || C > 2048 || (ld % 8) || ld < C || !(p > 0.f) || !(p < 1.f)) return CX_EINVAL;
  if (BWD && (!x || !qa || !qb || !qc || (ldx % 8) || ldx < C)) return CX_EINVAL;
  if (!BWD && ((S1 == nullptr) != (S2 == nullptr) || (S1 && stat_rows <= 0))) return CX_EINVAL;
  const int CP = C / 8, TA = 256 / CP * CP;
  int grid = grid_for((size_t)rows * CP, 256, 2048);
  if (!BWD && S1) { if (grid > stat_rows) grid = stat_rows; cx_tl_stat_rows = grid; }
  const double t = (double)p * 4294967296.0;
  const uint32_t thr = t >= 4294967295.0 ? 0xffffffffu : (uint32_t)t;
  hipLaunchKernelGGL((dropout_slice_kernel<T, BWD>), dim3(grid), dim3(256), 0, as_stream(stream), (T*)y, ld, (const T*)x, ldx, qa, qb, qc,
                     (size_t)rows, C, 1.f / (1.f - p), thr, seed, uid, S1, S2, TA);
  return launch_status();
}
template <typename T>
int bnrelu_maxpool_fwd_t(const void* x, const float* scale, const float* shift, void* y, uint8_t* argmax, float* stat_sum,
                          float* stat_sq, int B, int H, int W, int C, int ldy, int stat_rows, void* stream) {
  if (!x || !scale || !shift || !y || !argmax) return CX_EINVAL;
  if (C % 8 || C > 256 || 256 % (C / 8) || (H & 1) || (W & 1) || (ldy % 8)) return CX_ESHAPE;
  const size_t npix = (size_t)B * (H / 2) * (W / 2);
  const int ppb = 256 / (C / 8);
  int grid = grid_for(npix, ppb, 2048);
  if (stat_rows > 0 && stat_sum) { if (grid > stat_rows) grid = stat_rows; cx_tl_stat_rows = grid; }
  hipLaunchKernelGGL((bnrelu_maxpool_fwd_kernel<T>), dim3(grid), dim3(256), 256 * 16 * sizeof(float), as_stream(stream),
                     (const T*)x, scale, shift, (T*)y, argmax, stat_sum, stat_sq, B, H, W, C, ldy, stat_rows > 0 ? 1 : 0);
  return launch_status();
}

template <typename T>
int bnrelu_maxpool_bwd_t(const void* x, const float* scale, const float* shift, const float* mean, const float* rstd,
                          const uint8_t* argmax, const void* g, const void* gx, const float* ga, const float* gb, const float* gc,
                          void* dz, float* S1, float* S2, int B, int H, int W, int C, int ldg, int ldgx, int stat_rows, void* stream) {
  if (!x || !scale || !shift || !mean || !rstd || !argmax || !g || !gx || !ga || !gb || !gc || !dz || !S1 || !S2) return CX_EINVAL;
  if (C % 8 || C > 256 || 256 % (C / 8) || (H & 1) || (W & 1) || (ldg % 8) || (ldgx % 8)) return CX_ESHAPE;
  const size_t npix = (size_t)B * (H / 2) * (W / 2);     // 2x2 pixel blocks
  const int ppb = 256 / (C / 8);
  int grid = grid_for(npix, ppb, 2048);
  if (stat_rows > 0) { if (grid > stat_rows) grid = stat_rows; cx_tl_stat_rows = grid; }
  hipLaunchKernelGGL((bnrelu_maxpool_bwd_kernel<T>), dim3(grid), dim3(256), 256 * 16 * sizeof(float), as_stream(stream),
                     (const T*)x, scale, shift, mean, rstd, argmax, (const T*)g, (const T*)gx, ga, gb, gc, (T*)dz, S1,
                     S2, B, H, W, C, ldg, ldgx, stat_rows > 0 ? 1 : 0);
  return launch_status();
}

template <typename T>
int head_fwd_t(const void* x, const float* scale, const float* shift, const float* w, const float* bias, float* pooled,
                float* logits, int B, int HW, int C, int ldx, int n_classes, void* stream) {
  if (!x || !scale || !shift || !w || !pooled || !logits) return CX_EINVAL;
  if (C % 8 || ldx % 8 || n_classes <= 0) return CX_ESHAPE;
  const size_t n = (size_t)B * (C / 8);
  hipLaunchKernelGGL((gap_bnrelu_kernel<T>), dim3((n + 127) / 128), dim3(128), 0, as_stream(stream), (const T*)x, scale, shift, pooled,
                     B, HW, C, ldx);
  hipLaunchKernelGGL(linear_kernel, dim3(B), dim3(256), 0, as_stream(stream), pooled, w, bias, logits, C, n_classes);
  return launch_status();
}

template <typename T>
int gap_relu_bn_bwd_t(const float* dpooled, const void* x, const float* scale, const float* shift, const float* mean,
                       const float* rstd, const float* e_scale, void* g, float* S1, float* S2, int B, int HW, int C, int ldx,
                       int ldg, int stat_rows, void* stream) {
  if (!dpooled || !x || !scale || !shift || !mean || !rstd || !e_scale || !g || !S1 || !S2) return CX_EINVAL;
  if (C % 8 || ldx % 8 || ldg % 8) return CX_ESHAPE;
  const size_t n = (size_t)B * (C / 8);
  if (stat_rows > 0) { if (stat_rows < B) return CX_ESTATROWS; cx_tl_stat_rows = B; }
  hipLaunchKernelGGL((gap_relu_bn_bwd_kernel<T>), dim3((n + 127) / 128), dim3(128), 0, as_stream(stream), dpooled, (const T*)x, scale,
                     shift, mean, rstd, e_scale, (T*)g, S1, S2, B, HW, C, ldx, ldg, stat_rows > 0 ? 1 : 0);
  return launch_status();
}

template <typename T>
int unpool2_mask_t(const void* d, const void* x, const float* sc, const float* sh, const float* mean, const float* rstd,
                    const float* e_scale, void* g, float* S1, float* S2, int B, int H, int W, int C, int ldd, int ldx, int ldg,
                    int stat_rows, void* stream) {
  if (!d || !x || !sc || !sh || !mean || !rstd || !e_scale || !g || !S1 || !S2) return CX_EINVAL;
  if (C % 8 || C > 2048 || (H & 1) || (W & 1) || ldd % 8 || ldx % 8 || ldg % 8) return CX_ESHAPE;
  const size_t npix = (size_t)B * H * W;
  const int ppb = 256 / (C / 8);
  int grid = grid_for(npix, ppb, 2048);
  if (stat_rows > 0) { if (grid > stat_rows) grid = stat_rows; cx_tl_stat_rows = grid; }
  hipLaunchKernelGGL((unpool2_mask_kernel<T>), dim3(grid), dim3(256), 256 * 16 * sizeof(float), as_stream(stream),
                     (const T*)d, (const T*)x, sc, sh, mean, rstd, e_scale, (T*)g, S1, S2, B, H, W, C, ldd, ldx, ldg,
                     stat_rows > 0 ? 1 : 0);
  return launch_status();
}


}  // namespace

// Measurement hook (not part of the ABI): an event handed over by dbg_pre_reduce_event is recorded once, on the stream of the next
// slab reduce, BEFORE that reduce is launched -- so a caller bracketing a weight-gradient entry point with events can time the
// producing kernel alone (bench.py's roofline figure is per kernel, as rocprofv3 reports it).
// Diagnostic builds only (-DCX_DIAG): the product library exports no dbg_* symbol.
#ifdef CX_DIAG
static thread_local hipEvent_t g_pre_reduce_event = nullptr;
static thread_local int g_pre_reduce_taken = 0;
extern "C" void dbg_pre_reduce_event(void* ev) {
  g_pre_reduce_event = (hipEvent_t)ev;
  g_pre_reduce_taken = 0;
}
extern "C" int dbg_pre_reduce_event_taken(void) { return g_pre_reduce_taken; }
#endif

// Deferred slab sums (cx_wgrad_defer): while the calling thread has deferral on, a weight-gradient launch leaves its partial tiles
// in the caller's slab and only records what has to be added; cx_wgrad_defer_take hands the records to the caller, who runs them
// all with ONE cx_dw_reduce_table launch once the producing streams have been joined.
thread_local int cx_tl_slab_floats_v = 0;
namespace {
struct DeferState { bool on = false; std::vector<CxReduceDesc> list; };
thread_local DeferState g_defer;
inline bool reduce_vec(const float* dw, const float* slab, size_t total) { return (total & 3) == 0 && aligned16(dw) && aligned16(slab); }
}

int cx_dw_reduce(float* dw, const float* slab, size_t total, int splits, hipStream_t st) {
  return cx_dw_reduce_ld(dw, slab, total, splits, 0, 0, st);
}

int cx_dw_reduce_ld(float* dw, const float* slab, size_t total, int splits, int cols, int dw_ld, hipStream_t st) {
  if (!dw || !slab || total == 0 || splits <= 0 || cols < 0 || (cols && (dw_ld < cols || total % (size_t)cols))) return CX_EINVAL;
  if (cols == dw_ld) cols = dw_ld = 0;            // contiguous after all
  const bool vec = reduce_vec(dw, slab, total) && (cols % 4) == 0 && (dw_ld % 4) == 0;
  if (g_defer.on) {
    CxReduceDesc d;
    d.dw = dw; d.slab = slab; d.total = (int64_t)total; d.splits = splits;
    d.vec = vec ? 1 : 0;
    d.first_block = 0;
    d.cols = cols; d.dw_ld = dw_ld; d.pad_ = 0; d.pad2_ = 0;
    g_defer.list.push_back(d);
    return 0;
  }
#ifdef CX_DIAG
  if (g_pre_reduce_event) {
    (void)hipEventRecord(g_pre_reduce_event, st);
    g_pre_reduce_event = nullptr;
    g_pre_reduce_taken = 1;
  }
#endif
  if (vec) {
    const size_t n4 = total / 4;
    hipLaunchKernelGGL(dw_reduce_kernel<true>, dim3((unsigned)((n4 + 31) / 32)), dim3(256), 0, st, dw, slab, total, splits, cols, dw_ld);
  } else {
    hipLaunchKernelGGL(dw_reduce_kernel<false>, dim3((unsigned)((total + 31) / 32)), dim3(256), 0, st, dw, slab, total, splits, cols, dw_ld);
  }
  return launch_status();
}

template <typename T>
static int affine2_relu_mask_t(const void* a, const void* b, const float* pa, const float* pb, const float* pc, void* out, uint8_t* mask,
                               size_t rows, int C, void* stream) {
  if (!a || !b || !pa || !pb || !pc || !out || C % 8) return CX_EINVAL;
  hipLaunchKernelGGL(affine2_relu_kernel<T>, dim3(grid_for(rows * (C / 8), 256, 8192)), dim3(256), 0, as_stream(stream), (const T*)a,
                     (const T*)b, pa, pb, pc, (T*)out, mask, rows, C);
  return launch_status();
}
template <typename T>
static int relu_bwd_stats_mask_t(const void* dout, const void* out, const uint8_t* mask, const void* a, const float* mu_a, const float* r_a,
                                 const void* b, const float* mu_b, const float* r_b, void* dz, float* S1, float* S2a, float* S2b,
                                 size_t rows, int C, int stat_rows, void* stream) {
  if (!dout || (!out && !mask) || !a || !mu_a || !r_a || !dz || !S1 || !S2a) return CX_EINVAL;
  if (b && (!mu_b || !r_b || !S2b)) return CX_EINVAL;
  if (C % 8 || C > 2048) return CX_ESHAPE;
  const int T_ = 256 / (C / 8) * (C / 8);          // active threads per workgroup (see the kernel)
  int grid = grid_for(rows * (C / 8), 256, 2048);
  if (stat_rows > 0) { if (grid > stat_rows) grid = stat_rows; cx_tl_stat_rows = grid; }
  const size_t lds_bytes = (stat_rows > 0 ? (size_t)256 * 24 : (size_t)3 * C) * sizeof(float);
  hipLaunchKernelGGL(relu_bwd_stats_kernel<T>, dim3(grid), dim3(256), lds_bytes,
                     as_stream(stream), (const T*)dout, (const T*)out, (const T*)a, mu_a, r_a, (const T*)b, mu_b, r_b,
                     (T*)dz, S1, S2a, S2b, rows, C, stat_rows > 0 ? 1 : 0, mask, T_);
  return launch_status();
}
int cx_rows_reduce_add_impl(float* dst, const float* rows, int n_rows, int C, int rstride, hipStream_t st) {
  if (!dst || !rows || n_rows <= 0 || C <= 0 || rstride < C) return CX_EINVAL;
  hipLaunchKernelGGL(rows_reduce_add_kernel, dim3((C + 15) / 16), dim3(1024), 0, st, dst, rows, n_rows, C, rstride, 0);
  return launch_status();
}

extern "C" {

int cx_rows_reduce(float* dst, const float* rows, int n_rows, int C, int rstride, int accumulate, void* stream) {
  if (!dst || !rows || n_rows <= 0 || C <= 0 || rstride < C) return CX_EINVAL;
  hipLaunchKernelGGL(rows_reduce_add_kernel, dim3((C + 15) / 16), dim3(1024), 0, as_stream(stream), dst, rows, n_rows, C, rstride,
                     accumulate ? 0 : 1);
  return launch_status();
}

int cx_wgrad_defer(int on) {
  const int was = g_defer.on ? 1 : 0;
  g_defer.on = on > 0;
  if (on < 0) g_defer.list.clear();
  return was;
}

int cx_wgrad_defer_take(CxReduceDesc* out, int capacity, int64_t* total_blocks) {
  const int n = (int)g_defer.list.size();
  if (!out || n > capacity) return -n;
  int64_t blocks = 0;
  for (int i = 0; i < n; ++i) {
    CxReduceDesc d = g_defer.list[i];
    if (blocks >= (1ll << 31) - (1 << 24)) return CX_ESHAPE;
    d.first_block = (int32_t)blocks;
    const int64_t units = d.vec ? d.total / 4 : d.total;
    blocks += (units + 31) / 32;
    out[i] = d;
  }
  if (total_blocks) *total_blocks = blocks;
  g_defer.list.clear();
  return n;
}

int cx_last_slab_floats(void) { return cx_tl_slab_floats_v; }

int cx_dw_reduce_table(const CxReduceDesc* table_dev, int n, int64_t total_blocks, void* stream) {
  if (n == 0) return 0;
  if (!table_dev || n < 0 || total_blocks <= 0 || total_blocks >= (1ll << 31)) return CX_EINVAL;
  hipLaunchKernelGGL(dw_reduce_table_kernel, dim3((unsigned)total_blocks), dim3(256), 0, as_stream(stream), table_dev, n);
  return launch_status();
}

int cx_abi_version(void) { return CX_ABI_VERSION; }

const char* cx_error_string(int code) {
  switch (code) {
    case 0: return "ok";
    case CX_EINVAL: return "invalid argument (null pointer or inconsistent options)";
    case CX_EALIGN: return "pointer or pitch not 16-byte aligned";
    case CX_ESHAPE: return "unsupported shape";
    case CX_EUNSUPPORTED: return "unsupported prologue/epilogue/mode combination";
    case CX_ESTATROWS: return "stat_det: the launch needs more statistic rows than stat_replicas (capacity) provides";
    default: return code > 0 ? hipGetErrorString((hipError_t)code) : "unknown";
  }
}

int cx_pack_weights(const float* w, void* packed, int O, int I, int kh, int kw, int transpose, int stem, void* stream) {
  if (!w || !packed || O <= 0 || I <= 0) return CX_EINVAL;
  if (stem && (I != 3 || kh != 7 || kw != 7)) return CX_ESHAPE;
  const size_t total = stem ? (size_t)7 * O * 32 : (size_t)kh * kw * O * I;
  hipLaunchKernelGGL(pack_weights_kernel, dim3((total + 255) / 256), dim3(256), 0, as_stream(stream), w, (bf16*)packed, O, I, kh,
                     kw, transpose, stem);
  return launch_status();
}

int cx_pack_weights_table(const float* flat, void* packed, const CxPackDesc* table_dev, int n_desc, void* stream) {
  if (!flat || !packed || !table_dev || n_desc <= 0) return CX_EINVAL;
  // (grid.x = 128 blocks per descriptor: with 16 the 2.4 M-element 3x3 tensors of ResNet152's layer4 were each walked by 16 workgroups
  // and set the launch's time, 0.58 ms per step; blocks beyond a small tensor's pairs leave at once)
  hipLaunchKernelGGL(pack_table_kernel, dim3(128, n_desc), dim3(256), 0, as_stream(stream), flat, (bf16*)packed, table_dev);
  return launch_status();
}

// Channel-padded twin of a network whose widths are not multiples of 8 (the CIFAR DenseNet-BC of models/test_model.py:306: growth
// 12).  Element (o, j, t) of a real OIHW tensor lives at (o, pos(j), t) of the padded one, pos(j) = j for j < c0r (a block's first
// channels; j + shift from j = split on: an attention-augmented transition writes its convolution branch, padded, then its
// attention channels), else c0p + ((j - c0r) / k) * kp + (j - c0r) % k (dense layer (j - c0r) / k writes kp >= k channels).  dir 0: real ->
// padded (store; positions no real element maps to keep their zeros), dir 1: padded -> real (add: gradients; or store).
__global__ void chan_map_table_kernel(float* __restrict__ real, float* __restrict__ padded, const CxChanMapDesc* __restrict__ table,
                                      int dir, int accumulate) {
  const CxChanMapDesc d = table[blockIdx.x];
  float* r = real + d.real_off;
  float* q = padded + d.pad_off;
  const int total = d.O * d.Ireal * d.taps;
  for (int idx = threadIdx.x; idx < total; idx += blockDim.x) {
    const int t = idx % d.taps, j = (idx / d.taps) % d.Ireal, o = idx / (d.taps * d.Ireal);
    const int pj = j < d.c0r ? (j < d.split ? j : j + d.shift) : d.c0p + ((j - d.c0r) / d.k) * d.kp + (j - d.c0r) % d.k;
    const size_t pi = ((size_t)o * d.Ipad + pj) * d.taps + t;
    if (dir == 0) q[pi] = r[idx];
    else r[idx] = accumulate ? r[idx] + q[pi] : q[pi];
  }
}

int cx_chan_map_table(float* real_flat, float* padded_flat, const CxChanMapDesc* table_dev, int n_desc, int dir, int accumulate,
                      void* stream) {
  if (!real_flat || !padded_flat || !table_dev || n_desc <= 0 || dir < 0 || dir > 1) return CX_EINVAL;
  hipLaunchKernelGGL(chan_map_table_kernel, dim3(n_desc), dim3(256), 0, as_stream(stream), real_flat, padded_flat, table_dev, dir,
                     accumulate);
  return launch_status();
}

int cx_nchw3_to_nhwc4(const float* x, void* y, int B, int H, int W, void* stream) {
  if (!x || !y || B <= 0 || H <= 0 || W <= 0) return CX_EINVAL;
  const size_t hw = (size_t)H * W, total = hw * B;
  hipLaunchKernelGGL(nchw3_to_nhwc4_kernel, dim3((total + 255) / 256), dim3(256), 0, as_stream(stream), x, (bf16*)y, hw, total);
  return launch_status();
}

int cx_pack_weights_table_f32(const float* flat, float* packed, const CxPackDesc* table_dev, int n_desc, void* stream) {
  if (!flat || !packed || !table_dev || n_desc <= 0) return CX_EINVAL;
  hipLaunchKernelGGL(pack_table_f32_kernel, dim3(16, n_desc), dim3(256), 0, as_stream(stream), flat, packed, table_dev);
  return launch_status();
}

int cx_nchw3_to_nhwc4_f32(const float* x, float* y, int B, int H, int W, void* stream) {
  if (!x || !y || B <= 0 || H <= 0 || W <= 0) return CX_EINVAL;
  const size_t hw = (size_t)H * W, total = hw * B;
  hipLaunchKernelGGL(nchw3_to_nhwc4_f32_kernel, dim3((total + 255) / 256), dim3(256), 0, as_stream(stream), x, y, hw, total);
  return launch_status();
}

int cx_u8_to_nhwc4_f32(const uint8_t* x, float* y, size_t npix, float mean, float std, void* stream) {
  if (!x || !y || std <= 0.f) return CX_EINVAL;
  hipLaunchKernelGGL(u8_to_nhwc4_f32_kernel, dim3((npix + 255) / 256), dim3(256), 0, as_stream(stream), x, y, 1.f / (255.f * std),
                     -mean / std, npix);
  return launch_status();
}

int cx_u8_jitter(const uint8_t* x, uint8_t* y, int B, int HW, const float* brightness, const float* contrast, const int* order,
                 void* stream) {
  if (!x || !y || !brightness || !contrast || !order || B <= 0 || HW <= 0) return CX_EINVAL;
  if ((HW % 16) || !aligned16(x) || !aligned16(y)) return CX_EALIGN;
  if (HW > 150 * 1024) return CX_ESHAPE;                       // the image is parked in LDS between the two passes
  static bool attr = false;
  if (!attr) {
    (void)hipFuncSetAttribute(reinterpret_cast<const void*>(&u8_jitter_kernel), hipFuncAttributeMaxDynamicSharedMemorySize, 150 * 1024 + 128);
    attr = true;
  }
  hipLaunchKernelGGL(u8_jitter_kernel, dim3(B), dim3(1024), (size_t)HW + 128, as_stream(stream), x, y, HW, brightness, contrast, order);
  return launch_status();
}

int cx_u8_to_nhwc4(const uint8_t* x, void* y, size_t npix, float mean, float std, void* stream) {
  if (!x || !y || std <= 0.f) return CX_EINVAL;
  if ((npix % 16) || !aligned16(x) || !aligned16(y)) return CX_EALIGN;
  const size_t total16 = npix / 16;
  // ((u/255) - mean) / std = u * (1/(255 std)) - mean/std
  hipLaunchKernelGGL(u8_to_nhwc4_kernel, dim3((total16 + 255) / 256), dim3(256), 0, as_stream(stream), x, (bf16*)y,
                     1.f / (255.f * std), -mean / std, total16);
  return launch_status();
}

int cx_bn_coef(const float* sum, const float* sq, float count, const float* gamma, const float* beta, float eps, float momentum,
               float* running_mean, float* running_var, float* scale, float* shift, float* mean, float* rstd, int C,
               int replicas, int rstride, void* stream) {
  if (!sum || !sq || C <= 0 || count <= 0) return CX_EINVAL;
  if (replicas < 1) replicas = 1;
  if (replicas > 1 && rstride < C) return CX_EINVAL;
  hipLaunchKernelGGL(bn_coef_kernel, dim3((C + 15) / 16), dim3(1024), 0, as_stream(stream), sum, sq, count, gamma, beta, eps,
                     momentum, running_mean, running_var, scale, shift, mean, rstd, C, replicas, rstride);
  return launch_status();
}

int cx_bn_coef_moments(float* mean, float* rstd, float count, const float* gamma, const float* beta, float eps, float momentum,
                       float* running_mean, float* running_var, float* scale, float* shift, int C, const float* sum, const float* sq,
                       int rows, int rstride, int c_lo, int c_n, void* stream) {
  if (!mean || !rstd || C <= 0 || count <= 0) return CX_EINVAL;
  if (c_n > 0 && (!sum || !sq || rows < 1 || rstride < c_n || c_lo < 0 || c_lo + c_n > C)) return CX_EINVAL;
  hipLaunchKernelGGL(bn_coef_moments_kernel, dim3((C + 15) / 16), dim3(1024), 0, as_stream(stream), mean, rstd, count, gamma, beta, eps,
                     momentum, running_mean, running_var, scale, shift, C, sum, sq, rows, rstride, c_lo, c_n);
  return launch_status();
}

int cx_bn_coef_eval(const float* rm, const float* rv, const float* gamma, const float* beta, float eps, float* scale,
                    float* shift, float* mean, float* rstd, int C, void* stream) {
  if (!rm || !rv || C <= 0) return CX_EINVAL;
  hipLaunchKernelGGL(bn_coef_eval_kernel, dim3((C + 255) / 256), dim3(256), 0, as_stream(stream), rm, rv, gamma, beta, eps,
                     scale, shift, mean, rstd, C);
  return launch_status();
}

int cx_bn_bwd_coef(const float* S1, const float* S2, float count, const float* gamma, const float* mean, const float* rstd,
                   float* dgamma, float* dbeta, float* A, float* Bc, float* pa, float* pb, float* pc, int C, int replicas,
                   int rstride, float* qa, float* qb, float* qc, int q_lo, int q_n, void* stream) {
  if (!S1 || !S2 || !mean || !rstd || C <= 0 || count <= 0) return CX_EINVAL;
  if (qa && (!qb || !qc || !A || !Bc || q_lo < 0 || q_n <= 0 || q_lo + q_n > C)) return CX_EINVAL;
  if (replicas < 1) replicas = 1;
  if (replicas > 1 && rstride < C) return CX_EINVAL;
  if (pa && (!pb || !pc)) return CX_EINVAL;
  hipLaunchKernelGGL(bn_bwd_coef_kernel, dim3((C + 15) / 16), dim3(1024), 0, as_stream(stream), S1, S2, count, gamma, mean,
                     rstd, dgamma, dbeta, A, Bc, pa, pb, pc, C, replicas, rstride, qa, qb, qc, q_lo, q_n);
  return launch_status();
}

int cx_bn_bwd_coef_eval(const float* S1, const float* S2, const float* mean, const float* rstd, const float* running_mean,
                        const float* running_var, const float* gamma, float eps, float* dgamma, float* dbeta, float* pa, float* pb,
                        float* pc, int C, int replicas, int rstride, float* qa, float* qb, float* qc, int q_lo, int q_n, void* stream) {
  if (!S1 || !S2 || !mean || !rstd || !running_mean || !running_var || C <= 0) return CX_EINVAL;
  if (qa && (!qb || !qc || q_lo < 0 || q_n <= 0 || q_lo + q_n > C)) return CX_EINVAL;
  if (replicas < 1) replicas = 1;
  if (replicas > 1 && rstride < C) return CX_EINVAL;
  if (pa && (!pb || !pc)) return CX_EINVAL;
  hipLaunchKernelGGL(bn_bwd_coef_eval_kernel, dim3((C + 15) / 16), dim3(1024), 0, as_stream(stream), S1, S2, mean, rstd, running_mean,
                     running_var, gamma, eps, dgamma, dbeta, pa, pb, pc, C, replicas, rstride, qa, qb, qc, q_lo, q_n);
  return launch_status();
}

int cx_bn_bwd_slice_coef(const float* A, const float* Bc, const float* mean, const float* rstd, float* pa, float* pb, float* pc,
                         int C, void* stream) {
  if (!A || !Bc || !mean || !rstd || !pa || !pb || !pc || C <= 0) return CX_EINVAL;
  hipLaunchKernelGGL(bn_bwd_slice_coef_kernel, dim3((C + 255) / 256), dim3(256), 0, as_stream(stream), A, Bc, mean, rstd, pa, pb,
                     pc, C);
  return launch_status();
}

int cx_dropout_slice_fwd(void* y, int ld, int64_t rows, int C, float p, const int64_t* seed, uint32_t uid, float* S1, float* S2, int stat_rows, void* stream) {
  return dropout_slice_t<bf16, false>(y, ld, nullptr, 0, nullptr, nullptr, nullptr, rows, C, p, seed, uid, S1, S2, stat_rows, stream);
}
int cx_dropout_slice_fwd_f32(void* y, int ld, int64_t rows, int C, float p, const int64_t* seed, uint32_t uid, float* S1, float* S2, int stat_rows, void* stream) {
  return dropout_slice_t<float, false>(y, ld, nullptr, 0, nullptr, nullptr, nullptr, rows, C, p, seed, uid, S1, S2, stat_rows, stream);
}
int cx_dropout_slice_bwd(void* g, int ldg, const void* x, int ldx, const float* qa, const float* qb, const float* qc, int64_t rows, int C, float p, const int64_t* seed, uint32_t uid, void* stream) {
  return dropout_slice_t<bf16, true>(g, ldg, x, ldx, qa, qb, qc, rows, C, p, seed, uid, nullptr, nullptr, 0, stream);
}
int cx_dropout_slice_bwd_f32(void* g, int ldg, const void* x, int ldx, const float* qa, const float* qb, const float* qc, int64_t rows, int C, float p, const int64_t* seed, uint32_t uid, void* stream) {
  return dropout_slice_t<float, true>(g, ldg, x, ldx, qa, qb, qc, rows, C, p, seed, uid, nullptr, nullptr, 0, stream);
}

int cx_bnrelu_maxpool_fwd(const void* x, const float* scale, const float* shift, void* y, uint8_t* argmax, float* stat_sum, float* stat_sq, int B, int H, int W, int C, int ldy, int stat_rows, void* stream) {
  return bnrelu_maxpool_fwd_t<bf16>(x, scale, shift, y, argmax, stat_sum, stat_sq, B, H, W, C, ldy, stat_rows, stream);
}
int cx_bnrelu_maxpool_fwd_f32(const void* x, const float* scale, const float* shift, void* y, uint8_t* argmax, float* stat_sum, float* stat_sq, int B, int H, int W, int C, int ldy, int stat_rows, void* stream) {
  return bnrelu_maxpool_fwd_t<float>(x, scale, shift, y, argmax, stat_sum, stat_sq, B, H, W, C, ldy, stat_rows, stream);
}

int cx_bnrelu_maxpool_bwd(const void* x, const float* scale, const float* shift, const float* mean, const float* rstd, const uint8_t* argmax, const void* g, const void* gx, const float* ga, const float* gb, const float* gc, void* dz, float* S1, float* S2, int B, int H, int W, int C, int ldg, int ldgx, int stat_rows, void* stream) {
  return bnrelu_maxpool_bwd_t<bf16>(x, scale, shift, mean, rstd, argmax, g, gx, ga, gb, gc, dz, S1, S2, B, H, W, C, ldg, ldgx, stat_rows, stream);
}
int cx_bnrelu_maxpool_bwd_f32(const void* x, const float* scale, const float* shift, const float* mean, const float* rstd, const uint8_t* argmax, const void* g, const void* gx, const float* ga, const float* gb, const float* gc, void* dz, float* S1, float* S2, int B, int H, int W, int C, int ldg, int ldgx, int stat_rows, void* stream) {
  return bnrelu_maxpool_bwd_t<float>(x, scale, shift, mean, rstd, argmax, g, gx, ga, gb, gc, dz, S1, S2, B, H, W, C, ldg, ldgx, stat_rows, stream);
}

int cx_head_fwd(const void* x, const float* scale, const float* shift, const float* w, const float* bias, float* pooled, float* logits, int B, int HW, int C, int ldx, int n_classes, void* stream) {
  return head_fwd_t<bf16>(x, scale, shift, w, bias, pooled, logits, B, HW, C, ldx, n_classes, stream);
}
int cx_head_fwd_f32(const void* x, const float* scale, const float* shift, const float* w, const float* bias, float* pooled, float* logits, int B, int HW, int C, int ldx, int n_classes, void* stream) {
  return head_fwd_t<float>(x, scale, shift, w, bias, pooled, logits, B, HW, C, ldx, n_classes, stream);
}

int cx_head_bwd(const float* dlogits, const float* pooled, const float* w, float* dw, float* db, float* dpooled, int B, int C,
                int n_classes, void* stream) {
  if (!dlogits || !pooled || !w || !dw || !dpooled) return CX_EINVAL;
  if (n_classes > C) return CX_ESHAPE;
  hipLaunchKernelGGL(head_bwd_kernel, dim3((C + 255) / 256, n_classes + B), dim3(256), 0, as_stream(stream), dlogits, pooled, w, dw, db,
                     dpooled, B, C, n_classes);
  return launch_status();
}

int cx_gap_relu_bn_bwd(const float* dpooled, const void* x, const float* scale, const float* shift, const float* mean, const float* rstd, const float* e_scale, void* g, float* S1, float* S2, int B, int HW, int C, int ldx, int ldg, int stat_rows, void* stream) {
  return gap_relu_bn_bwd_t<bf16>(dpooled, x, scale, shift, mean, rstd, e_scale, g, S1, S2, B, HW, C, ldx, ldg, stat_rows, stream);
}
int cx_gap_relu_bn_bwd_f32(const float* dpooled, const void* x, const float* scale, const float* shift, const float* mean, const float* rstd, const float* e_scale, void* g, float* S1, float* S2, int B, int HW, int C, int ldx, int ldg, int stat_rows, void* stream) {
  return gap_relu_bn_bwd_t<float>(dpooled, x, scale, shift, mean, rstd, e_scale, g, S1, S2, B, HW, C, ldx, ldg, stat_rows, stream);
}

int cx_unpool2_mask(const void* d, const void* x, const float* sc, const float* sh, const float* mean, const float* rstd, const float* e_scale, void* g, float* S1, float* S2, int B, int H, int W, int C, int ldd, int ldx, int ldg, int stat_rows, void* stream) {
  return unpool2_mask_t<bf16>(d, x, sc, sh, mean, rstd, e_scale, g, S1, S2, B, H, W, C, ldd, ldx, ldg, stat_rows, stream);
}
int cx_unpool2_mask_f32(const void* d, const void* x, const float* sc, const float* sh, const float* mean, const float* rstd, const float* e_scale, void* g, float* S1, float* S2, int B, int H, int W, int C, int ldd, int ldx, int ldg, int stat_rows, void* stream) {
  return unpool2_mask_t<float>(d, x, sc, sh, mean, rstd, e_scale, g, S1, S2, B, H, W, C, ldd, ldx, ldg, stat_rows, stream);
}

int cx_affine2_inplace(void* dz, const void* x, const float* pa, const float* pb, const float* pc, size_t rows, int C, void* stream) {
  if (!dz || !x || !pa || !pb || !pc || C % 8) return CX_EINVAL;
  hipLaunchKernelGGL(affine2_inplace_kernel, dim3(grid_for(rows * (C / 8), 256, 8192)), dim3(256), 0, as_stream(stream), (bf16*)dz,
                     (const bf16*)x, pa, pb, pc, rows, C);
  return launch_status();
}

int cx_affine2_relu_mask(const void* a, const void* b, const float* pa, const float* pb, const float* pc, void* out, uint8_t* mask,
                         size_t rows, int C, void* stream) {
  return affine2_relu_mask_t<bf16>(a, b, pa, pb, pc, out, mask, rows, C, stream);
}
int cx_affine2_relu_mask_f32(const void* a, const void* b, const float* pa, const float* pb, const float* pc, void* out, uint8_t* mask,
                             size_t rows, int C, void* stream) {
  return affine2_relu_mask_t<float>(a, b, pa, pb, pc, out, mask, rows, C, stream);
}

int cx_join_fwd(const void* a, const void* b, const int8_t* b_lo, const float* pa, const float* pb, const float* pc, void* out, int8_t* out_lo,
                uint8_t* mask, size_t rows, int C, void* stream) {
  if (!a || !b || !pa || !pb || !pc || !out || C <= 0 || (C % 8)) return CX_EINVAL;
  if (!aligned16(a) || !aligned16(b) || !aligned16(out) || (((uintptr_t)b_lo) & 7) || (((uintptr_t)out_lo) & 7)) return CX_EALIGN;
  if (rows == 0) return 0;
  if (C % 64 == 0)
    hipLaunchKernelGGL(join_fwd_kernel<2>, dim3(grid_for(rows * (C / 16), 256, 8192)), dim3(256), 0, as_stream(stream), (const uint4*)a,
                       (const uint4*)b, (const uint8_t*)b_lo, pa, pb, pc, (uint4*)out, (uint8_t*)out_lo, mask, rows, C);
  else
    hipLaunchKernelGGL(join_fwd_kernel<1>, dim3(grid_for(rows * (C / 8), 256, 8192)), dim3(256), 0, as_stream(stream), (const uint4*)a,
                       (const uint4*)b, (const uint8_t*)b_lo, pa, pb, pc, (uint4*)out, (uint8_t*)out_lo, mask, rows, C);
  return launch_status();
}

int cx_affine2_relu(const void* a, const void* b, const float* pa, const float* pb, const float* pc, void* out, size_t rows, int C,
                    void* stream) {
  return cx_affine2_relu_mask(a, b, pa, pb, pc, out, nullptr, rows, C, stream);
}

int cx_relu_bwd_stats(const void* dout, const void* out, const void* a, const float* mu_a, const float* r_a, const void* b,
                      const float* mu_b, const float* r_b, void* dz, float* S1, float* S2a, float* S2b, size_t rows, int C,
                      int stat_rows, void* stream) {
  return cx_relu_bwd_stats_mask(dout, out, nullptr, a, mu_a, r_a, b, mu_b, r_b, dz, S1, S2a, S2b, rows, C, stat_rows, stream);
}

int cx_relu_bwd_stats_mask(const void* dout, const void* out, const uint8_t* mask, const void* a, const float* mu_a, const float* r_a,
                           const void* b, const float* mu_b, const float* r_b, void* dz, float* S1, float* S2a, float* S2b, size_t rows,
                           int C, int stat_rows, void* stream) {
  return relu_bwd_stats_mask_t<bf16>(dout, out, mask, a, mu_a, r_a, b, mu_b, r_b, dz, S1, S2a, S2b, rows, C, stat_rows, stream);
}
int cx_relu_bwd_stats_mask_f32(const void* dout, const void* out, const uint8_t* mask, const void* a, const float* mu_a, const float* r_a,
                               const void* b, const float* mu_b, const float* r_b, void* dz, float* S1, float* S2a, float* S2b,
                               size_t rows, int C, int stat_rows, void* stream) {
  return relu_bwd_stats_mask_t<float>(dout, out, mask, a, mu_a, r_a, b, mu_b, r_b, dz, S1, S2a, S2b, rows, C, stat_rows, stream);
}

int cx_gradcam_map(const void* x, const float* scale, const float* shift, const float* w, float* cam, int B, int HW, int C, int ldx,
                   int inner_relu, void* stream) {
  if (!x || !scale || !shift || !w || !cam || C % 8 || ldx % 8) return CX_EINVAL;
  const size_t npix = (size_t)B * HW;
  hipLaunchKernelGGL(gradcam_map_kernel, dim3((npix + 3) / 4), dim3(256), 0, as_stream(stream), (const bf16*)x, scale, shift, w, cam, npix,
                     C, ldx, inner_relu);
  return launch_status();
}

int cx_cam_norm_upsample(const float* cam, float* out, int B, int h, int w, int H, int W, void* stream) {
  if (!cam || !out || B <= 0 || h <= 0 || w <= 0 || H <= 0 || W <= 0) return CX_EINVAL;
  hipLaunchKernelGGL(cam_norm_upsample_kernel, dim3(B), dim3(256), 0, as_stream(stream), cam, out, h, w, H, W);
  return launch_status();
}

// The yardstick next to the 8 TB/s specification: a 16-byte-per-lane copy.  Form chosen by measurement (scratch/copybench.hip,
// profiles/r04_copybench.txt; 1 GiB read + 1 GiB written): a workgroup moves contiguous 16 KB pieces (four loads in flight per
// thread), pieces dealt round-robin over >= 4096 workgroups, non-temporal loads and stores: 6.0-6.2 TB/s, against 4.5-5.1 TB/s for
// the grid-stride form, 5.3-5.8 without the non-temporal hint and 4.9 for hipMemcpyAsync (MI355X_MICROARCH.md quotes 6.29 TB/s).
namespace {
__global__ __launch_bounds__(256) void copy_stream_kernel(const cx_u32x4* __restrict__ src, cx_u32x4* __restrict__ dst, size_t n16) {
  constexpr size_t PIECE = 4 * 256;
  const size_t whole = n16 / PIECE * PIECE;
  for (size_t base = (size_t)blockIdx.x * PIECE; base < whole; base += (size_t)gridDim.x * PIECE) {
    const cx_u32x4* s = src + base + threadIdx.x;
    cx_u32x4* d = dst + base + threadIdx.x;
    const cx_u32x4 a = __builtin_nontemporal_load(s), b = __builtin_nontemporal_load(s + 256);
    const cx_u32x4 c = __builtin_nontemporal_load(s + 512), e = __builtin_nontemporal_load(s + 768);
    __builtin_nontemporal_store(a, d);
    __builtin_nontemporal_store(b, d + 256);
    __builtin_nontemporal_store(c, d + 512);
    __builtin_nontemporal_store(e, d + 768);
  }
  for (size_t i = whole + (size_t)blockIdx.x * 256 + threadIdx.x; i < n16; i += (size_t)gridDim.x * 256) dst[i] = src[i];
}
}  // namespace

int cx_copy_stream(const void* src, void* dst, size_t bytes, void* stream) {
  if (!src || !dst || (bytes % 16) || !aligned16(src) || !aligned16(dst)) return CX_EINVAL;
  if (bytes == 0) return 0;
  const size_t pieces = (bytes / 16 + 1023) / 1024;
  hipLaunchKernelGGL(copy_stream_kernel, dim3((unsigned)(pieces < 16384 ? pieces : 16384)), dim3(256), 0, as_stream(stream),
                     (const cx_u32x4*)src, (cx_u32x4*)dst, bytes / 16);
  return launch_status();
}

int cx_fill_f32(float* p, float v, size_t n, void* stream) {
  if (!p) return CX_EINVAL;
  hipLaunchKernelGGL(fill_kernel, dim3(grid_for(n, 256, 2048)), dim3(256), 0, as_stream(stream), p, v, n);
  return launch_status();
}

int cx_affine_to_f32_nchw(const void* x, const float* scale, const float* shift, int relu, float* y, int B, int H, int W, int C, int ldx,
                          void* stream) {
  if (!x || !y || ((scale == nullptr) != (shift == nullptr))) return CX_EINVAL;
  const size_t total = (size_t)B * H * W * C;
  hipLaunchKernelGGL(affine_to_f32_nchw_kernel, dim3((total + 255) / 256), dim3(256), 0, as_stream(stream), (const bf16*)x, scale, shift,
                     relu, y, H * W, C, ldx, total);
  return launch_status();
}

int cx_bf16_to_f32_nchw(const void* x, float* y, int B, int H, int W, int C, int ldx, void* stream) {
  if (!x || !y) return CX_EINVAL;
  const size_t total = (size_t)B * H * W * C;
  hipLaunchKernelGGL(bf16_to_f32_nchw_kernel, dim3((total + 255) / 256), dim3(256), 0, as_stream(stream), (const bf16*)x, y, H * W, C,
                     ldx, total);
  return launch_status();
}

}  // extern "C"
