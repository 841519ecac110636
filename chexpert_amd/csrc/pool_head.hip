// Global pooling heads other than the average: max, log-sum-exp (LSE) and generalised mean (GeM) over the HW pixels of the last
// feature map, with the activation in front (ReLU of DenseNet / ResNet, Swish of EfficientNet) applied on load.  The definitions
// stand in include/chexpert_hip.h beside the entry points; chexpert_amd/pooling.py restates them in numpy.
//
// Mapping: that of the average kernels (gap_bnrelu_kernel / gap_relu_bn_bwd_kernel of elementwise.hip): one thread per (image,
// 8 channels) walks the column of HW pixels with one 16-byte access per pixel (bf16; two in the fp32 mode).  LSE and GeM are computed
// relative to the column maximum, so the forward walks the column twice (the second walk hits the cache: a column is HW lines).
// The pass is memory-bound; every sum of one (image, channel) is formed by one thread in ascending pixel order, so the results
// are reproducible, and the backward's per-image statistic rows have one writer per element.
#include <math.h>
#include "common.h"

namespace {

constexpr float GEM_EPS = 1e-6f;
constexpr int PH_THREADS = 128;              // workgroup of the two column kernels (the bound keeps their ~140 registers out of scratch)

__device__ __forceinline__ float ph_sigmoid(float z) { return 1.f / (1.f + expf(-z)); }

// a = act(z), act: CX_POOL_ACT_RELU or CX_POOL_ACT_SWISH.  The forward and the backward call this one function on the same fmaf, so
// the max backward finds the pooled value again bit for bit.
__device__ __forceinline__ float ph_act(float z, int act) { return act == CX_POOL_ACT_SWISH ? z * ph_sigmoid(z) : fmaxf(z, 0.f); }

__device__ __forceinline__ float ph_dact(float z, int act) {
  if (act == CX_POOL_ACT_SWISH) {
    const float s = ph_sigmoid(z);
    return s * (1.f + z * (1.f - s));
  }
  return z > 0.f ? 1.f : 0.f;
}

__device__ __forceinline__ float ph_q(const float* param) { return fminf(fmaxf(*param, 1.f), 16.f); }

template <typename T>
__global__ __launch_bounds__(PH_THREADS) void pool_head_fwd_kernel(const T* __restrict__ x, const float* __restrict__ sc, const float* __restrict__ sh,
                                     float* __restrict__ pooled, float* __restrict__ aux, const float* __restrict__ param, int B,
                                     int HW, int C, int ldx, int act, int kind) {
  const int CP = C / 8;
  const size_t idx = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (idx >= (size_t)B * CP) return;
  const int b = idx / CP, cq = idx % CP;
  const T* col = x + (size_t)b * HW * ldx + cq * 8;
  float fsc[8], fsh[8], m[8];
#pragma unroll
  for (int j = 0; j < 8; ++j) { fsc[j] = sc[cq * 8 + j]; fsh[j] = sh[cq * 8 + j]; m[j] = -INFINITY; }
  for (int p = 0; p < HW; ++p) {
    const typename V8<T>::raw v = V8<T>::ld(col + (size_t)p * ldx);
#pragma unroll
    for (int j = 0; j < 8; ++j) m[j] = fmaxf(m[j], ph_act(fmaf(V8<T>::get(v, j), fsc[j], fsh[j]), act));
  }
  float* out = pooled + (size_t)b * C + cq * 8;
  if (kind == CX_POOL_MAX) {
#pragma unroll
    for (int j = 0; j < 8; ++j) out[j] = m[j];
    return;
  }
  float s[8], t[8];
#pragma unroll
  for (int j = 0; j < 8; ++j) s[j] = t[j] = 0.f;
  if (kind == CX_POOL_LSE) {
    const float r = *param;
    for (int p = 0; p < HW; ++p) {
      const typename V8<T>::raw v = V8<T>::ld(col + (size_t)p * ldx);
#pragma unroll
      for (int j = 0; j < 8; ++j) s[j] += expf(r * (ph_act(fmaf(V8<T>::get(v, j), fsc[j], fsh[j]), act) - m[j]));
    }
    // aux = pooled - m, the offset the backward subtracts from a - m: next to a large maximum pooled itself has no digits left
    // for it (1e4 - 0.46 is rounded to 1e-3, and r times that error would be the relative error of the gradient)
    float* ax = aux + (size_t)b * C + cq * 8;
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      const float off = logf(s[j] / (float)HW) / r;
      out[j] = m[j] + off;
      ax[j] = off;
    }
    return;
  }
  // GeM relative to m' = max(m, eps): s = sum (a'/m')^q, t = sum (a'/m')^q ln(a'/m'); pooled = m' (s/HW)^(1/q), T = ln m' + t/s.
  // A column that is clamped everywhere gives s = HW and t = 0 exactly: pooled = eps and T = ln pooled bit for bit.
  const float q = ph_q(param);
  float mm[8];
#pragma unroll
  for (int j = 0; j < 8; ++j) mm[j] = fmaxf(m[j], GEM_EPS);
  for (int p = 0; p < HW; ++p) {
    const typename V8<T>::raw v = V8<T>::ld(col + (size_t)p * ldx);
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      const float a = fmaxf(ph_act(fmaf(V8<T>::get(v, j), fsc[j], fsh[j]), act), GEM_EPS);
      // (a'/m')^q as exp(q ln(a'/m')), one logarithm for the power and for T.  The rounding of the logarithm costs the power a
      // relative q |ln| 2^-24, which its own size weighs: w q |ln(a'/m')| is at most 1/e.  A ratio of 1 gives exactly 1.
      const float l = logf(a / mm[j]);                     // <= 0
      const float w = expf(q * l);
      s[j] += w;
      t[j] += w * l;
    }
  }
  float* ax = aux + (size_t)b * C + cq * 8;
#pragma unroll
  for (int j = 0; j < 8; ++j) {
    out[j] = mm[j] * expf(logf(s[j] / (float)HW) / q);        // (s / HW, not s * (1 / HW): a clamped column gives exactly 1)
    ax[j] = logf(mm[j]) + t[j] / s[j];
  }
}

template <typename T>
__global__ __launch_bounds__(PH_THREADS) void pool_head_bwd_kernel(const float* __restrict__ dpooled, const float* __restrict__ pooled,
                                     const float* __restrict__ aux, const float* __restrict__ param, const T* __restrict__ x, const float* __restrict__ sc,
                                     const float* __restrict__ sh, const float* __restrict__ mean, const float* __restrict__ rstd,
                                     const float* __restrict__ escale, T* __restrict__ g, float* S1, float* S2, int B, int HW, int C,
                                     int ldx, int ldg, int act, int kind, int det) {
  const int CP = C / 8;
  const size_t idx = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (idx >= (size_t)B * CP) return;
  const int b = idx / CP, cq = idx % CP;
  float fsc[8], fsh[8], fmu[8], fr[8], fe[8], dp[8], pl[8], s1[8], s2[8];
  float m[8], off[8];                          // lse: the column maximum (found again here) and pooled - m (the forward's aux)
  unsigned open = 0xffu;                       // max: bit j is set while channel j's first maximal pixel has not been met
  const float inv = 1.f / HW;
  const float par = kind == CX_POOL_LSE ? *param : kind == CX_POOL_GEM ? ph_q(param) : 0.f;
#pragma unroll
  for (int j = 0; j < 8; ++j) {
    const int c = cq * 8 + j;
    fsc[j] = sc[c]; fsh[j] = sh[c]; fmu[j] = mean[c]; fr[j] = rstd[c]; fe[j] = escale[c];
    dp[j] = dpooled[(size_t)b * C + c];
    pl[j] = pooled[(size_t)b * C + c];
    s1[j] = s2[j] = 0.f;
    m[j] = -INFINITY;
    off[j] = kind == CX_POOL_LSE ? aux[(size_t)b * C + c] : 0.f;
  }
  if (kind == CX_POOL_LSE) {
    for (int p = 0; p < HW; ++p) {
      const typename V8<T>::raw v = V8<T>::ld(x + ((size_t)b * HW + p) * ldx + cq * 8);
#pragma unroll
      for (int j = 0; j < 8; ++j) m[j] = fmaxf(m[j], ph_act(fmaf(V8<T>::get(v, j), fsc[j], fsh[j]), act));
    }
  }
  for (int p = 0; p < HW; ++p) {
    const typename V8<T>::raw v = V8<T>::ld(x + ((size_t)b * HW + p) * ldx + cq * 8);
    float o[8];
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      const float xf = V8<T>::get(v, j);
      const float z = fmaf(xf, fsc[j], fsh[j]);
      const float a = ph_act(z, act);
      float w;                                 // d pooled / d a
      if (kind == CX_POOL_MAX) {
        const bool hit = ((open >> j) & 1u) && a == pl[j];
        w = hit ? 1.f : 0.f;
        if (hit) open &= ~(1u << j);
      } else if (kind == CX_POOL_LSE) {
        w = expf(par * ((a - m[j]) - off[j])) * inv;      // exp(r (a - pooled)) / HW with a - pooled = (a - m) - (pooled - m)
      } else {
        w = a > GEM_EPS ? expf((par - 1.f) * logf(a / pl[j])) * inv : 0.f;      // (a / pooled)^(q - 1) / HW; q = 1 gives 1 / HW
      }
      const float d = dp[j] * w * ph_dact(z, act);
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

// dp += sum_{b,c} dpooled pooled (T - ln pooled) / q, 0 where p is clamped.  One workgroup: thread i adds the elements i, i + 1024,
// ... in ascending order, the 1024 partial sums are added by a fixed tree.
constexpr int PG_THREADS = 1024;

__global__ __launch_bounds__(PG_THREADS) void pool_p_grad_kernel(const float* __restrict__ dpooled, const float* __restrict__ pooled,
                                                                 const float* __restrict__ aux, const float* __restrict__ p,
                                                                 float* dp, size_t n) {
  __shared__ float part[PG_THREADS];
  float acc = 0.f;
  for (size_t i = threadIdx.x; i < n; i += PG_THREADS) acc += dpooled[i] * pooled[i] * (aux[i] - logf(pooled[i]));
  part[threadIdx.x] = acc;
  __syncthreads();
  for (int w = PG_THREADS / 2; w >= 1; w >>= 1) {
    if ((int)threadIdx.x < w) part[threadIdx.x] += part[threadIdx.x + w];
    __syncthreads();
  }
  if (threadIdx.x == 0) {
    const float pv = *p;
    if (pv > 1.f && pv < 16.f) dp[0] += part[0] / pv;
  }
}

bool known(int act, int kind) {
  return (act == CX_POOL_ACT_RELU || act == CX_POOL_ACT_SWISH) && (kind == CX_POOL_MAX || kind == CX_POOL_LSE || kind == CX_POOL_GEM);
}

template <typename T>
int pool_head_fwd_t(const void* x, const float* sc, const float* sh, float* pooled, float* aux, const float* param, int B, int HW,
                    int C, int ldx, int act, int kind, void* stream) {
  if (!x || !sc || !sh || !pooled || !known(act, kind)) return CX_EINVAL;
  if (kind != CX_POOL_MAX && (!param || !aux)) return CX_EINVAL;
  if (B <= 0 || HW <= 0 || C <= 0 || C % 8 || ldx % 8 || ldx < C) return CX_ESHAPE;
  if (!aligned16(x)) return CX_EALIGN;
  const size_t n = (size_t)B * (C / 8);
  hipLaunchKernelGGL((pool_head_fwd_kernel<T>), dim3((n + PH_THREADS - 1) / PH_THREADS), dim3(PH_THREADS), 0, as_stream(stream), (const T*)x, sc, sh, pooled, aux,
                     param, B, HW, C, ldx, act, kind);
  return launch_status();
}

template <typename T>
int pool_head_bwd_t(const float* dpooled, const float* pooled, const float* aux, const float* param, const void* x, const float* sc,
                    const float* sh, const float* mean, const float* rstd, const float* e_scale, void* g, float* S1, float* S2, int B,
                    int HW, int C, int ldx, int ldg, int act, int kind, int stat_rows, void* stream) {
  if (!dpooled || !pooled || !x || !sc || !sh || !mean || !rstd || !e_scale || !g || !S1 || !S2 || !known(act, kind)) return CX_EINVAL;
  if (kind != CX_POOL_MAX && !param) return CX_EINVAL;
  if (kind == CX_POOL_LSE && !aux) return CX_EINVAL;
  if (B <= 0 || HW <= 0 || C <= 0 || C % 8 || ldx % 8 || ldg % 8 || ldx < C || ldg < C) return CX_ESHAPE;
  if (!aligned16(x) || !aligned16(g)) return CX_EALIGN;
  const size_t n = (size_t)B * (C / 8);
  if (stat_rows > 0) { if (stat_rows < B) return CX_ESTATROWS; cx_tl_stat_rows = B; }
  hipLaunchKernelGGL((pool_head_bwd_kernel<T>), dim3((n + PH_THREADS - 1) / PH_THREADS), dim3(PH_THREADS), 0, as_stream(stream), dpooled, pooled, aux, param,
                     (const T*)x, sc, sh, mean, rstd, e_scale, (T*)g, S1, S2, B, HW, C, ldx, ldg, act, kind, stat_rows > 0 ? 1 : 0);
  return launch_status();
}

}  // namespace

extern "C" {

int cx_pool_head_fwd(const void* x, const float* sc, const float* sh, float* pooled, float* aux, const float* param, int B, int HW,
                     int C, int ldx, int act, int kind, void* stream) {
  return pool_head_fwd_t<bf16>(x, sc, sh, pooled, aux, param, B, HW, C, ldx, act, kind, stream);
}
int cx_pool_head_fwd_f32(const void* x, const float* sc, const float* sh, float* pooled, float* aux, const float* param, int B, int HW,
                         int C, int ldx, int act, int kind, void* stream) {
  return pool_head_fwd_t<float>(x, sc, sh, pooled, aux, param, B, HW, C, ldx, act, kind, stream);
}
int cx_pool_head_bwd(const float* dpooled, const float* pooled, const float* aux, const float* param, const void* x, const float* sc,
                     const float* sh, const float* mean, const float* rstd, const float* e_scale, void* g, float* S1, float* S2, int B,
                     int HW, int C, int ldx, int ldg, int act, int kind, int stat_rows, void* stream) {
  return pool_head_bwd_t<bf16>(dpooled, pooled, aux, param, x, sc, sh, mean, rstd, e_scale, g, S1, S2, B, HW, C, ldx, ldg, act, kind,
                               stat_rows, stream);
}
int cx_pool_head_bwd_f32(const float* dpooled, const float* pooled, const float* aux, const float* param, const void* x, const float* sc,
                         const float* sh, const float* mean, const float* rstd, const float* e_scale, void* g, float* S1, float* S2,
                         int B, int HW, int C, int ldx, int ldg, int act, int kind, int stat_rows, void* stream) {
  return pool_head_bwd_t<float>(dpooled, pooled, aux, param, x, sc, sh, mean, rstd, e_scale, g, S1, S2, B, HW, C, ldx, ldg, act, kind,
                                stat_rows, stream);
}
int cx_pool_p_grad(const float* dpooled, const float* pooled, const float* aux, const float* p, float* dp, int B, int C, void* stream) {
  if (!dpooled || !pooled || !aux || !p || !dp) return CX_EINVAL;
  if (B <= 0 || C <= 0) return CX_ESHAPE;
  hipLaunchKernelGGL(pool_p_grad_kernel, dim3(1), dim3(PG_THREADS), 0, as_stream(stream), dpooled, pooled, aux, p, dp, (size_t)B * C);
  return launch_status();
}

}  // extern "C"
