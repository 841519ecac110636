// The linear probe of a frozen backbone (include/chexpert_hip.h, cx_probe_*): multi-label L2-regularised logistic regression on a
// bank of pooled features, n independent convex problems over one shared pass of the bank, and the vector arithmetic of its L-BFGS
// solver.  The definition is chexpert_amd/probe.py (reference_loss_grad, numpy float64).
//
//   probe_pass_kernel    a workgroup (4 waves) owns one slice of the bank's rows and walks it in tiles of 64 rows, wave w rows
//                        16 w .. 16 w + 15.  Logits: D[class][row] on v_mfma_f32_16x16x4_f32, the classes on the 16-wide side; the
//                        four k of one instruction are the columns c0 + 4 q + j of lane quarter q, so a lane's operands are ONE
//                        16-byte load of its row (j = 0..3 feed four instructions; a dot product does not care in which order its
//                        terms are taken as long as both operands agree); the loads of four such chunks are issued before their
//                        MFMAs.  Residual and loss terms in registers (expf / log1pf),
//                        the residuals transposed through LDS, then R^T X for the same 64 rows on the same MFMA: the rows are the
//                        k side, a wave owns column tiles of 16 and keeps their sums in registers over the whole slice; the tile
//                        of X is read again (it was read microseconds earlier and sits in L2).  Column d of the gradient is the
//                        bias: the B operand there is 1.  A panel of 2048 / (class tiles) columns per workgroup; wider matrices
//                        take one workgroup per panel (blockIdx.y), each forming the logits again.
//   probe_finish_kernel  adds the slices in slice order, one fp32 division by N_c, one fused add of l2 w; the loss likewise.
// No atomics, partial tiles by zero fill and predication, a caller's scratch: the same bits on every run for the same `splits`.
// A class whose active flag is 0 costs no MFMA where its whole class tile is idle, and never a store.
#include "common.h"
#include <math.h>

namespace {

constexpr int PB_NT = 256, PB_TR = 64;
constexpr int PB_KB = 4;                                       // chunks of 16 columns whose loads are in flight together
constexpr int PB_ACC = 32;                                     // 16 x 16 gradient tiles a wave accumulates (128 registers)
constexpr int PB_MAX_D = CX_KNN_MAX_D, PB_MAX_N = CX_KNN_MAX_CLASSES, PB_MAX_SPLITS = CX_PROBE_MAX_SPLITS, PB_MAX_HIST = CX_PROBE_MAX_HISTORY;
constexpr int PB_STAT_SLICES = 256;
constexpr float PB_STD_FLOOR = 1e-6f;

static inline bool aligned_to(const void* p, const uintptr_t a) { return (((uintptr_t)p) & (a - 1)) == 0; }

// four consecutive values of one row (pitch floats apart) from column `col` on; zeros from column `lim` on and for a row that is not there
template <bool VEC>
__device__ __forceinline__ float4 pb_ld4(const float* __restrict__ base, const long long row, const bool ok, const int pitch, const int lim,
                                         const int col) {
  float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
  if (!ok || col >= lim) return v;
  const float* p = base + (size_t)row * pitch + col;
  if constexpr (VEC) return *reinterpret_cast<const float4*>(p);          // pitch == lim, lim % 4 == 0 and a 16-byte base
  v.x = p[0];
  if (col + 1 < lim) v.y = p[1];
  if (col + 2 < lim) v.z = p[2];
  if (col + 3 < lim) v.w = p[3];
  return v;
}

// the sum of v over the workgroup's 256 threads in a fixed order; every thread calls it
__device__ __forceinline__ float pb_block_sum(float v, float* __restrict__ red, const int tid) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
  __syncthreads();
  if ((tid & 63) == 0) red[tid >> 6] = v;
  __syncthreads();
  return ((red[0] + red[1]) + red[2]) + red[3];
}
__device__ __forceinline__ float pb_block_max(float v, float* __restrict__ red, const int tid) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v = fmaxf(v, __shfl_xor(v, o));
  __syncthreads();
  if ((tid & 63) == 0) red[tid >> 6] = v;
  __syncthreads();
  return fmaxf(fmaxf(red[0], red[1]), fmaxf(red[2], red[3]));
}

// z[ct][j] = x_row . w_class for class 16 ct + 4 (lane >> 4) + j and the row of lane & 15 (no bias).  wok: this lane's A-operand class
// 16 ct + (lane & 15) exists and is active; ton: some class of the tile is (uniform)
template <int N16, bool VEC>
__device__ __forceinline__ void pb_tile_logits(const float* __restrict__ x, const long long row, const bool row_ok, const int d,
                                               const float* __restrict__ theta, const bool (&wok)[N16], const bool (&ton)[N16],
                                               const int l15, const int lq, f32x4 (&z)[N16]) {
  f32x4 z0[N16], z1[N16];
#pragma unroll
  for (int ct = 0; ct < N16; ++ct)
#pragma unroll
    for (int j = 0; j < 4; ++j) { z0[ct][j] = 0.f; z1[ct][j] = 0.f; }
  // PB_KB chunks of 16 columns at a time: all their loads are issued first, then their MFMAs, in the order of the columns (a
  // chunk past d loads zeros and is skipped), so a load's latency is covered by the chunks before it
  for (int c0 = 0; c0 < d; c0 += 16 * PB_KB) {
    float4 xv[PB_KB], wv[N16][PB_KB];
#pragma unroll
    for (int u = 0; u < PB_KB; ++u) {
      const int col = c0 + 16 * u + 4 * lq;
      xv[u] = pb_ld4<VEC>(x, row, row_ok, d, d, col);
#pragma unroll
      for (int ct = 0; ct < N16; ++ct) wv[ct][u] = pb_ld4<false>(theta, 16 * ct + l15, wok[ct] && ton[ct], d + 1, d, col);
    }
#pragma unroll
    for (int u = 0; u < PB_KB; ++u) {
      if (c0 + 16 * u >= d) break;
#pragma unroll
      for (int ct = 0; ct < N16; ++ct) {
        if (!ton[ct]) continue;
        z0[ct] = __builtin_amdgcn_mfma_f32_16x16x4f32(wv[ct][u].x, xv[u].x, z0[ct], 0, 0, 0);
        z1[ct] = __builtin_amdgcn_mfma_f32_16x16x4f32(wv[ct][u].y, xv[u].y, z1[ct], 0, 0, 0);
        z0[ct] = __builtin_amdgcn_mfma_f32_16x16x4f32(wv[ct][u].z, xv[u].z, z0[ct], 0, 0, 0);
        z1[ct] = __builtin_amdgcn_mfma_f32_16x16x4f32(wv[ct][u].w, xv[u].w, z1[ct], 0, 0, 0);
      }
    }
  }
#pragma unroll
  for (int ct = 0; ct < N16; ++ct) z[ct] = z0[ct] + z1[ct];
}

// the residual r = (pw y + 1 - y) sigmoid(z) - pw y and the loss term pw y softplus(-z) + (1 - y) softplus(z) of one live label
__device__ __forceinline__ void pb_residual(const float z, const float y, const float pw, float& r, float& el) {
  const float pwy = pw * y, omy = 1.f - y, wgt = pwy + omy;
  const float e = expf(-fabsf(z));                      // in (0, 1]
  const float s = (z >= 0.f ? 1.f : e) / (1.f + e);
  r = fmaf(wgt, s, -pwy);
  const float L = log1pf(e);
  el = pwy * (fmaxf(-z, 0.f) + L) + omy * (fmaxf(z, 0.f) + L);
}

template <int N16>
__device__ __forceinline__ void pb_class_flags(const int* __restrict__ active, const int n, const int l15, bool (&wok)[N16], bool (&ton)[N16]) {
#pragma unroll
  for (int ct = 0; ct < N16; ++ct) {
    const int c = 16 * ct + l15;
    wok[ct] = c < n && (!active || active[c] != 0);
    ton[ct] = __builtin_amdgcn_readfirstlane(__ballot(wok[ct]) != 0ull ? 1 : 0) != 0;       // uniform, and known to be
  }
}

template <int N16, bool VEC>
__global__ __launch_bounds__(PB_NT) void probe_logits_kernel(const float* __restrict__ x, const float* __restrict__ theta,
                                                             float* __restrict__ out, const int rows, const int d, const int n) {
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, l15 = lane & 15, lq = lane >> 4;
  bool wok[N16], ton[N16];
  pb_class_flags<N16>(nullptr, n, l15, wok, ton);
  const long long row = (long long)blockIdx.x * PB_TR + 16 * wave + l15;
  if ((long long)blockIdx.x * PB_TR + 16 * wave >= rows) return;
  f32x4 z[N16];
  pb_tile_logits<N16, VEC>(x, row, row < rows, d, theta, wok, ton, l15, lq, z);
  if (row >= rows) return;
#pragma unroll
  for (int ct = 0; ct < N16; ++ct)
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const int c = 16 * ct + 4 * lq + j;
      if (c < n) out[(size_t)row * n + c] = z[ct][j] + theta[(size_t)c * (d + 1) + d];
    }
}

template <int N16, bool VEC>
__global__ __launch_bounds__(PB_NT) void probe_pass_kernel(const float* __restrict__ x, const float* __restrict__ y,
                                                           const float* __restrict__ theta, const float* __restrict__ pos_weight,
                                                           const int* __restrict__ active, float* __restrict__ part,
                                                           float* __restrict__ lpart, const int M, const int d, const int n,
                                                           const long long rows_per_slice) {
  constexpr int CT = PB_ACC / N16;                     // column tiles of a wave
  constexpr int DP = CT * 4 * 16;                      // columns of a panel
  constexpr int NC = N16 * 16;
  __shared__ float rT[PB_TR][NC + 1];                  // the tile's residuals [row][class]
  __shared__ float red[4][NC][4];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, l15 = lane & 15, lq = lane >> 4;
  const int slice = blockIdx.x, D1 = d + 1;
  const int pcol = blockIdx.y * DP;
  const long long r0 = min((long long)M, (long long)slice * rows_per_slice), r1 = min((long long)M, r0 + rows_per_slice);

  bool wok[N16], ton[N16];
  pb_class_flags<N16>(active, n, l15, wok, ton);
  // the classes of this lane's logits: 16 ct + 4 lq + j
  bool dok[N16][4];
  float bias[N16][4], pw[N16][4], lsum[N16][4], pos[N16][4], neg[N16][4];
  int cnt[N16][4];                                     // live rows: an integer, exact for any M < 2^31
#pragma unroll
  for (int ct = 0; ct < N16; ++ct)
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const int c = 16 * ct + 4 * lq + j;
      dok[ct][j] = c < n && (!active || active[c] != 0);
      bias[ct][j] = dok[ct][j] ? theta[(size_t)c * D1 + d] : 0.f;
      pw[ct][j] = (dok[ct][j] && pos_weight) ? pos_weight[c] : 1.f;
      lsum[ct][j] = 0.f; cnt[ct][j] = 0; pos[ct][j] = 0.f; neg[ct][j] = 0.f;
    }
  f32x4 acc[N16][CT];
#pragma unroll
  for (int ct = 0; ct < N16; ++ct)
#pragma unroll
    for (int t = 0; t < CT; ++t)
#pragma unroll
      for (int j = 0; j < 4; ++j) acc[ct][t][j] = 0.f;

  for (long long rb = r0; rb < r1; rb += PB_TR) {
    // logits, residuals and loss terms of this wave's 16 rows
    const long long row = rb + 16 * wave + l15;
    const bool row_ok = row < r1;
    f32x4 z[N16];
    if (rb + 16 * wave < r1) {
      pb_tile_logits<N16, VEC>(x, row, row_ok, d, theta, wok, ton, l15, lq, z);
    } else {
#pragma unroll
      for (int ct = 0; ct < N16; ++ct)
#pragma unroll
        for (int j = 0; j < 4; ++j) z[ct][j] = 0.f;
    }
#pragma unroll
    for (int ct = 0; ct < N16; ++ct)
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        float r = 0.f;
        if (row_ok && dok[ct][j]) {
          const float yv = y[(size_t)row * n + 16 * ct + 4 * lq + j];
          if (yv >= 0.f) {
            float el;
            pb_residual(z[ct][j] + bias[ct][j], yv, pw[ct][j], r, el);
            lsum[ct][j] += el;
            cnt[ct][j] += 1;
            pos[ct][j] += yv;
            neg[ct][j] += 1.f - yv;
          }
        }
        rT[16 * wave + l15][16 * ct + 4 * lq + j] = r;
      }
    __syncthreads();
    // G[class][column] += sum over the tile's rows of R[class][row] X[row][column]; column d is the bias (X = 1)
    const int nsteps = (int)min((long long)PB_TR / 4, ((r1 - rb + 15) / 16) * 4);
#pragma unroll
    for (int t = 0; t < CT; ++t) {
      const int col0 = pcol + (t * 4 + wave) * 16;
      if (col0 >= D1) continue;
      const int col = col0 + l15;
      for (int st0 = 0; st0 < nsteps; st0 += 4) {          // (nsteps is a multiple of 4) four loads, then their MFMAs
        float b[4];
#pragma unroll
        for (int u = 0; u < 4; ++u) {
          const int rk = 4 * (st0 + u) + lq;
          b[u] = col == d ? 1.f : 0.f;
          if (col < d && rb + rk < r1) b[u] = x[(size_t)(rb + rk) * d + col];
        }
#pragma unroll
        for (int u = 0; u < 4; ++u) {
          const int rk = 4 * (st0 + u) + lq;
#pragma unroll
          for (int ct = 0; ct < N16; ++ct) {
            if (!ton[ct]) continue;
            acc[ct][t] = __builtin_amdgcn_mfma_f32_16x16x4f32(rT[rk][16 * ct + l15], b[u], acc[ct][t], 0, 0, 0);
          }
        }
      }
    }
    __syncthreads();
  }

  // the slice's partial gradient: register j of a lane is class 16 ct + 4 lq + j, column col0 + l15
#pragma unroll
  for (int t = 0; t < CT; ++t) {
    const int col = pcol + (t * 4 + wave) * 16 + l15;
    if (col >= D1) continue;
#pragma unroll
    for (int ct = 0; ct < N16; ++ct)
#pragma unroll
      for (int j = 0; j < 4; ++j)
        if (dok[ct][j]) part[((size_t)slice * n + 16 * ct + 4 * lq + j) * D1 + col] = acc[ct][t][j];
  }
  if (blockIdx.y != 0) return;
  // loss, live rows, positive and negative mass: over the 16 rows of a wave, then the waves in order
#pragma unroll
  for (int ct = 0; ct < N16; ++ct)
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      float v0 = lsum[ct][j], v2 = pos[ct][j], v3 = neg[ct][j];
      int v1 = cnt[ct][j];
#pragma unroll
      for (int o = 8; o > 0; o >>= 1) {
        v0 += __shfl_xor(v0, o);
        v1 += __shfl_xor(v1, o);
        v2 += __shfl_xor(v2, o);
        v3 += __shfl_xor(v3, o);
      }
      if (l15 == 0) {
        float* const r = red[wave][16 * ct + 4 * lq + j];
        r[0] = v0; r[1] = __int_as_float(v1); r[2] = v2; r[3] = v3;
      }
    }
  __syncthreads();
  for (int i = tid; i < NC * 4; i += PB_NT) {
    const int c = i >> 2, q = i & 3;
    if (c >= n || (active && active[c] == 0)) continue;
    float v = ((red[0][c][q] + red[1][c][q]) + red[2][c][q]) + red[3][c][q];
    if (q == 1)                                        // the count travels as the bits of an int
      v = __int_as_float(__float_as_int(red[0][c][1]) + __float_as_int(red[1][c][1]) + __float_as_int(red[2][c][1]) +
                         __float_as_int(red[3][c][1]));
    lpart[((size_t)slice * 4 + q) * n + c] = v;
  }
}

// grid (n, column blocks of 256): the slices in order, / N_c, + l2 w; block y == 0 also gives the loss and the counts
__global__ __launch_bounds__(PB_NT) void probe_finish_kernel(const float* __restrict__ part, const float* __restrict__ lpart,
                                                             const float* __restrict__ theta, const int* __restrict__ active,
                                                             const float l2, float* __restrict__ loss, float* __restrict__ grad,
                                                             float* __restrict__ count, const int d, const int n, const int S) {
  __shared__ float red[4];
  const int c = blockIdx.x, tid = threadIdx.x, D1 = d + 1;
  if (active && active[c] == 0) return;
  double live = 0.0;
  for (int s = 0; s < S; ++s) live += (double)__float_as_int(lpart[((size_t)s * 4 + 1) * n + c]);
  const float Nc = (float)(live < 1.0 ? 1.0 : live);
  const int col = blockIdx.y * PB_NT + tid;
  if (col < D1) {
    float g = 0.f;
    for (int s = 0; s < S; ++s) g += part[((size_t)s * n + c) * D1 + col];
    g = g / Nc;
    if (col < d) g = fmaf(l2, theta[(size_t)c * D1 + col], g);
    grad[(size_t)c * D1 + col] = g;
  }
  if (blockIdx.y != 0) return;
  float ww = 0.f;
  for (int k = tid; k < d; k += PB_NT) {
    const float w = theta[(size_t)c * D1 + k];
    ww = fmaf(w, w, ww);
  }
  ww = pb_block_sum(ww, red, tid);
  if (tid == 0) {
    float ls = 0.f;
    double p = 0.0, q = 0.0;
    for (int s = 0; s < S; ++s) {
      ls += lpart[((size_t)s * 4 + 0) * n + c];
      p += (double)lpart[((size_t)s * 4 + 2) * n + c];
      q += (double)lpart[((size_t)s * 4 + 3) * n + c];
    }
    loss[c] = fmaf(0.5f * l2, ww, ls / Nc);
    count[3 * c + 0] = (float)live;
    count[3 * c + 1] = (float)p;
    count[3 * c + 2] = (float)q;
  }
}

// ---- column statistics: double sums, slices of rows first, then the slices in order ---------------------------------------------------
// pass 0: sum of x; pass 1: sum of (x - mean)^2 with the double mean
__global__ __launch_bounds__(PB_NT) void probe_stat_part_kernel(const float* __restrict__ x, const double* __restrict__ mean,
                                                                double* __restrict__ part, const int M, const int d,
                                                                const long long rows_per_slice) {
  const int col = blockIdx.x * PB_NT + threadIdx.x, slice = blockIdx.y;
  if (col >= d) return;
  const long long r0 = min((long long)M, (long long)slice * rows_per_slice), r1 = min((long long)M, r0 + rows_per_slice);
  double acc = 0.0;
  if (mean) {
    const double mu = mean[col];
    for (long long r = r0; r < r1; ++r) {
      const double v = (double)x[(size_t)r * d + col] - mu;
      acc += v * v;
    }
  } else {
    for (long long r = r0; r < r1; ++r) acc += (double)x[(size_t)r * d + col];
  }
  part[(size_t)slice * d + col] = acc;
}
__global__ __launch_bounds__(PB_NT) void probe_stat_finish_kernel(const double* __restrict__ part, double* __restrict__ mean_d,
                                                                  float* __restrict__ mean, float* __restrict__ rstd, const int M,
                                                                  const int d, const int S) {
  const int col = blockIdx.x * PB_NT + threadIdx.x;
  if (col >= d) return;
  double acc = 0.0;
  for (int s = 0; s < S; ++s) acc += part[(size_t)s * d + col];
  acc /= (double)M;
  if (mean) {
    mean_d[col] = acc;
    mean[col] = (float)acc;
  } else {
    const double sd = sqrt(acc);
    rstd[col] = (float)(1.0 / (sd > (double)PB_STD_FLOOR ? sd : (double)PB_STD_FLOOR));
  }
}
// y = (x - mean) * rstd: a difference and a product, each rounded once (there is no product-sum here for the compiler to fuse)
__global__ __launch_bounds__(PB_NT) void probe_standardize_kernel(const float* x, const float* __restrict__ mean,
                                                                  const float* __restrict__ rstd, float* y, const long long total,
                                                                  const int d) {
  for (long long i = (long long)blockIdx.x * PB_NT + threadIdx.x; i < total; i += (long long)gridDim.x * PB_NT) {
    const int k = (int)(i % d);
    const float df = x[i] - mean[k];
    y[i] = df * rstd[k];
  }
}

// ---- the solver's vector arithmetic: one workgroup per class ---------------------------------------------------------------------------
// hist[2 c] = pairs held (<= m), hist[2 c + 1] = the slot the next pair goes to; pair j of class c at (c m + j) D1
__global__ __launch_bounds__(PB_NT) void probe_direction_kernel(const float* __restrict__ grad, const float* __restrict__ sh,
                                                                const float* __restrict__ yh, const int* __restrict__ hist,
                                                                const int* __restrict__ active, float* __restrict__ dir,
                                                                float* __restrict__ stats, const int m, const int D1) {
  __shared__ float q[PB_MAX_D + 1];
  __shared__ float red[4];
  __shared__ float alpha[PB_MAX_HIST], sy[PB_MAX_HIST];
  const int c = blockIdx.x, tid = threadIdx.x;
  if (active && active[c] == 0) return;
  const float* const g = grad + (size_t)c * D1;
  const int held = hist[2 * c], head = hist[2 * c + 1];
  float gmax = 0.f, g1 = 0.f;
  for (int k = tid; k < D1; k += PB_NT) {
    const float v = g[k];
    q[k] = v;
    gmax = fmaxf(gmax, fabsf(v));
    g1 += fabsf(v);
  }
  gmax = pb_block_max(gmax, red, tid);
  g1 = pb_block_sum(g1, red, tid);
  float gamma = 1.f;
  for (int i = 0; i < held; ++i) {                     // newest first
    const int j = (head - 1 - i + 2 * m) % m;
    const float* const s = sh + ((size_t)c * m + j) * D1;
    const float* const yy = yh + ((size_t)c * m + j) * D1;
    float a = 0.f, b = 0.f, e = 0.f;
    for (int k = tid; k < D1; k += PB_NT) {
      a = fmaf(s[k], yy[k], a);
      b = fmaf(s[k], q[k], b);
      e = fmaf(yy[k], yy[k], e);
    }
    a = pb_block_sum(a, red, tid);
    b = pb_block_sum(b, red, tid);
    if (i == 0) {
      e = pb_block_sum(e, red, tid);
      gamma = a / e;
    }
    const float al = b / a;
    if (tid == 0) { alpha[i] = al; sy[i] = a; }
    for (int k = tid; k < D1; k += PB_NT) q[k] = fmaf(-al, yy[k], q[k]);
  }
  __syncthreads();
  for (int k = tid; k < D1; k += PB_NT) q[k] *= gamma;
  for (int i = held - 1; i >= 0; --i) {
    const int j = (head - 1 - i + 2 * m) % m;
    const float* const s = sh + ((size_t)c * m + j) * D1;
    const float* const yy = yh + ((size_t)c * m + j) * D1;
    float b = 0.f;
    for (int k = tid; k < D1; k += PB_NT) b = fmaf(yy[k], q[k], b);
    b = pb_block_sum(b, red, tid);
    const float co = alpha[i] - b / sy[i];
    for (int k = tid; k < D1; k += PB_NT) q[k] = fmaf(co, s[k], q[k]);
  }
  float gd = 0.f, gg = 0.f;
  for (int k = tid; k < D1; k += PB_NT) {
    gd = fmaf(g[k], -q[k], gd);
    gg = fmaf(g[k], g[k], gg);
  }
  gd = pb_block_sum(gd, red, tid);
  gg = pb_block_sum(gg, red, tid);
  const bool descends = gd < 0.f && gd > -INFINITY;     // false for NaN too
  for (int k = tid; k < D1; k += PB_NT) dir[(size_t)c * D1 + k] = descends ? -q[k] : -g[k];
  if (tid == 0) {
    stats[4 * c + 0] = descends ? gd : -gg;
    stats[4 * c + 1] = gmax;
    stats[4 * c + 2] = g1;
    stats[4 * c + 3] = descends ? 0.f : 1.f;
  }
}

// mode[c] 1: theta_t = theta + t dir.  2: the trial is accepted: the pair (theta_t - theta, grad_t - grad) joins the history unless
// s.y <= 0, then theta = theta_t and grad = grad_t.  3: the trial's slope and size, tstats[2 c] = grad_t . dir, tstats[2 c + 1] =
// max |grad_t| (by convexity f(theta_t) <= f(theta) + grad_t . (theta_t - theta): a slope that is still steep enough certifies the
// sufficient decrease where the fp32 loss cannot resolve it).  0: nothing is written
__global__ __launch_bounds__(PB_NT) void probe_advance_kernel(float* __restrict__ theta, float* __restrict__ grad,
                                                              const float* __restrict__ dir, const float* __restrict__ t,
                                                              const int* __restrict__ mode, float* __restrict__ theta_t,
                                                              const float* __restrict__ grad_t, float* __restrict__ sh,
                                                              float* __restrict__ yh, int* __restrict__ hist,
                                                              float* __restrict__ tstats, const int m, const int D1) {
  __shared__ float red[4];
  const int c = blockIdx.x, tid = threadIdx.x, md = mode[c];
  const size_t o = (size_t)c * D1;
  if (md == 3) {
    float a = 0.f, mx = 0.f;
    for (int k = tid; k < D1; k += PB_NT) {
      a = fmaf(grad_t[o + k], dir[o + k], a);
      mx = fmaxf(mx, fabsf(grad_t[o + k]));
    }
    a = pb_block_sum(a, red, tid);
    mx = pb_block_max(mx, red, tid);
    if (tid == 0) {
      tstats[2 * c] = a;
      tstats[2 * c + 1] = mx;
    }
  } else if (md == 1) {
    const float tc = t[c];
    for (int k = tid; k < D1; k += PB_NT) theta_t[o + k] = fmaf(tc, dir[o + k], theta[o + k]);
  } else if (md == 2) {
    float a = 0.f;
    for (int k = tid; k < D1; k += PB_NT) a = fmaf(theta_t[o + k] - theta[o + k], grad_t[o + k] - grad[o + k], a);
    a = pb_block_sum(a, red, tid);
    const int held = hist[2 * c], head = hist[2 * c + 1];
    const bool push = a > 0.f;
    float* const s = sh + ((size_t)c * m + head) * D1;
    float* const yy = yh + ((size_t)c * m + head) * D1;
    for (int k = tid; k < D1; k += PB_NT) {
      const float tn = theta_t[o + k], gn = grad_t[o + k];
      if (push) {
        s[k] = tn - theta[o + k];
        yy[k] = gn - grad[o + k];
      }
      theta[o + k] = tn;
      grad[o + k] = gn;
    }
    __syncthreads();
    if (tid == 0 && push) {
      hist[2 * c] = held < m ? held + 1 : m;
      hist[2 * c + 1] = (head + 1) % m;
    }
  }
}

int pb_cus() {
  static const int cus = [] {
    int dev = 0, n = 0;
    if (hipGetDevice(&dev) != hipSuccess || hipDeviceGetAttribute(&n, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess || n < 1) {
      (void)hipGetLastError();
      n = 256;
    }
    return n;
  }();
  return cus;
}
// the slices of a pass: the caller's, or one per compute unit with at least one whole tile of rows each
int pb_splits(const int M, const int splits) {
  if (splits > 0) return splits;
  const long long tiles = ((long long)M + PB_TR - 1) / PB_TR;
  long long s = tiles < pb_cus() ? tiles : pb_cus();
  return (int)(s < 1 ? 1 : s > PB_MAX_SPLITS ? PB_MAX_SPLITS : s);
}
int pb_stat_slices(const int M) {
  const long long s = ((long long)M + 31) / 32;
  return (int)(s < PB_STAT_SLICES ? s : PB_STAT_SLICES);
}
bool pb_sizes_ok(const int M, const int d, const int n, const int splits) {
  return M >= 1 && d >= 1 && d <= PB_MAX_D && n >= 1 && n <= PB_MAX_N && splits >= 0 && splits <= PB_MAX_SPLITS;
}

template <int N16>
void pb_launch_pass(const bool vec, const dim3 grid, hipStream_t st, const float* x, const float* y, const float* theta, const float* pw,
                    const int* active, float* part, float* lpart, int M, int d, int n, long long rps) {
  if (vec)
    hipLaunchKernelGGL((probe_pass_kernel<N16, true>), grid, dim3(PB_NT), 0, st, x, y, theta, pw, active, part, lpart, M, d, n, rps);
  else
    hipLaunchKernelGGL((probe_pass_kernel<N16, false>), grid, dim3(PB_NT), 0, st, x, y, theta, pw, active, part, lpart, M, d, n, rps);
}
template <int N16>
void pb_launch_logits(const bool vec, const dim3 grid, hipStream_t st, const float* x, const float* theta, float* out, int rows, int d,
                      int n) {
  if (vec)
    hipLaunchKernelGGL((probe_logits_kernel<N16, true>), grid, dim3(PB_NT), 0, st, x, theta, out, rows, d, n);
  else
    hipLaunchKernelGGL((probe_logits_kernel<N16, false>), grid, dim3(PB_NT), 0, st, x, theta, out, rows, d, n);
}

}  // namespace

long long cx_probe_scratch(int M, int d, int n, int splits) {
  if (!pb_sizes_ok(M, d, n, splits)) return 0;
  const long long pass = (long long)pb_splits(M, splits) * ((long long)n * (d + 1) + 4ll * n);
  const long long stat = 2ll * (pb_stat_slices(M) + 1) * d;
  return pass > stat ? pass : stat;
}

int cx_probe_colstats(const float* x, float* mean, float* rstd, float* scratch, long long scratch_floats, int M, int d, void* stream) {
  if (!x || !mean || !rstd || !scratch || M < 1 || d < 1 || d > PB_MAX_D) return CX_EINVAL;
  const int S = pb_stat_slices(M);
  if (scratch_floats < 2ll * (S + 1) * d) return CX_EINVAL;
  if (!aligned_to(x, 4) || !aligned_to(mean, 4) || !aligned_to(rstd, 4) || !aligned_to(scratch, 8)) return CX_EALIGN;
  double* const part = reinterpret_cast<double*>(scratch);
  double* const mean_d = part + (size_t)S * d;
  const long long rps = ((long long)M + S - 1) / S;
  const dim3 grid((d + PB_NT - 1) / PB_NT, S), fin((d + PB_NT - 1) / PB_NT);
  hipStream_t st = as_stream(stream);
  hipLaunchKernelGGL(probe_stat_part_kernel, grid, dim3(PB_NT), 0, st, x, (const double*)nullptr, part, M, d, rps);
  hipLaunchKernelGGL(probe_stat_finish_kernel, fin, dim3(PB_NT), 0, st, (const double*)part, mean_d, mean, (float*)nullptr, M, d, S);
  hipLaunchKernelGGL(probe_stat_part_kernel, grid, dim3(PB_NT), 0, st, x, (const double*)mean_d, part, M, d, rps);
  hipLaunchKernelGGL(probe_stat_finish_kernel, fin, dim3(PB_NT), 0, st, (const double*)part, mean_d, (float*)nullptr, rstd, M, d, S);
  return launch_status();
}

int cx_probe_standardize(const float* x, const float* mean, const float* rstd, float* y, long long rows, int d, void* stream) {
  if (!x || !mean || !rstd || !y || rows < 1 || d < 1 || d > PB_MAX_D) return CX_EINVAL;
  if (!aligned_to(x, 4) || !aligned_to(mean, 4) || !aligned_to(rstd, 4) || !aligned_to(y, 4)) return CX_EALIGN;
  const long long total = rows * d, blocks = (total + PB_NT - 1) / PB_NT;
  hipLaunchKernelGGL(probe_standardize_kernel, dim3((unsigned)(blocks < 65536 ? blocks : 65536)), dim3(PB_NT), 0, as_stream(stream), x, mean,
                     rstd, y, total, d);
  return launch_status();
}

int cx_probe_logits(const float* x, const float* theta, float* out, int rows, int d, int n, void* stream) {
  if (!x || !theta || !out || !pb_sizes_ok(rows, d, n, 0)) return CX_EINVAL;
  if (!aligned_to(x, 4) || !aligned_to(theta, 4) || !aligned_to(out, 4)) return CX_EALIGN;
  const bool vec = (d % 4 == 0) && aligned16(x);
  const dim3 grid((unsigned)(((long long)rows + PB_TR - 1) / PB_TR));
  hipStream_t st = as_stream(stream);
  if (n <= 16) pb_launch_logits<1>(vec, grid, st, x, theta, out, rows, d, n);
  else if (n <= 32) pb_launch_logits<2>(vec, grid, st, x, theta, out, rows, d, n);
  else pb_launch_logits<4>(vec, grid, st, x, theta, out, rows, d, n);
  return launch_status();
}

int cx_probe_loss_grad(const float* x, const float* y, const float* theta, const float* pos_weight, float l2, const int* active,
                       float* loss, float* grad, float* count, float* scratch, long long scratch_floats, int M, int d, int n, int splits,
                       void* stream) {
  if (!x || !y || !theta || !loss || !grad || !count || !scratch || !pb_sizes_ok(M, d, n, splits) || !(l2 >= 0.f) || !(l2 < INFINITY))
    return CX_EINVAL;
  const int S = pb_splits(M, splits);
  if (scratch_floats < (long long)S * ((long long)n * (d + 1) + 4ll * n)) return CX_EINVAL;
  if (!aligned_to(x, 4) || !aligned_to(y, 4) || !aligned_to(theta, 4) || !aligned_to(pos_weight, 4) || !aligned_to(active, 4) ||
      !aligned_to(loss, 4) || !aligned_to(grad, 4) || !aligned_to(count, 4) || !aligned_to(scratch, 4))
    return CX_EALIGN;
  const int D1 = d + 1, n16 = n <= 16 ? 1 : n <= 32 ? 2 : 4, dp = (PB_ACC / n16) * 64;
  const long long t16 = ((long long)M + 15) / 16, rps = ((t16 + S - 1) / S) * 16;
  float* const part = scratch;
  float* const lpart = scratch + (size_t)S * n * D1;
  const bool vec = (d % 4 == 0) && aligned16(x);
  const dim3 grid(S, (D1 + dp - 1) / dp);
  hipStream_t st = as_stream(stream);
  if (n16 == 1) pb_launch_pass<1>(vec, grid, st, x, y, theta, pos_weight, active, part, lpart, M, d, n, rps);
  else if (n16 == 2) pb_launch_pass<2>(vec, grid, st, x, y, theta, pos_weight, active, part, lpart, M, d, n, rps);
  else pb_launch_pass<4>(vec, grid, st, x, y, theta, pos_weight, active, part, lpart, M, d, n, rps);
  hipLaunchKernelGGL(probe_finish_kernel, dim3(n, (D1 + PB_NT - 1) / PB_NT), dim3(PB_NT), 0, st, (const float*)part, (const float*)lpart,
                     theta, active, l2, loss, grad, count, d, n, S);
  return launch_status();
}

int cx_probe_lbfgs_direction(const float* grad, const float* s_hist, const float* y_hist, const int* hist, const int* active, float* dir,
                             float* stats, int n, int d, int m, void* stream) {
  if (!grad || !s_hist || !y_hist || !hist || !dir || !stats || n < 1 || n > PB_MAX_N || d < 1 || d > PB_MAX_D || m < 1 || m > PB_MAX_HIST)
    return CX_EINVAL;
  hipLaunchKernelGGL(probe_direction_kernel, dim3(n), dim3(PB_NT), 0, as_stream(stream), grad, s_hist, y_hist, hist, active, dir, stats, m,
                     d + 1);
  return launch_status();
}

int cx_probe_lbfgs_advance(float* theta, float* grad, const float* dir, const float* t, const int* mode, float* theta_t,
                           const float* grad_t, float* s_hist, float* y_hist, int* hist, float* tstats, int n, int d, int m, void* stream) {
  if (!theta || !grad || !dir || !t || !mode || !theta_t || !grad_t || !s_hist || !y_hist || !hist || !tstats || n < 1 || n > PB_MAX_N || d < 1 ||
      d > PB_MAX_D || m < 1 || m > PB_MAX_HIST)
    return CX_EINVAL;
  hipLaunchKernelGGL(probe_advance_kernel, dim3(n), dim3(PB_NT), 0, as_stream(stream), theta, grad, dir, t, mode, theta_t, grad_t, s_hist,
                     y_hist, hist, tstats, m, d + 1);
  return launch_status();
}
