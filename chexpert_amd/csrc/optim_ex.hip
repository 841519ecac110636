// Global-norm gradient clipping, non-finite skip and weight EMA inside the optimiser launch (flat fp32 buffers).
//
//   cx_grad_norm      two launches, no atomics: per-workgroup partial sums of (grad_scale * g)^2 over fixed contiguous ranges, then ONE
//                     workgroup that sums the partials and writes clip[4] = {norm, coef, nonfinite, skipped} to device memory
//   cx_*_step[_dev]_ex the updates of elementwise.hip with the gradient multiplied by clip[1], nothing written at all when clip[2] says
//                     the gradient was not finite and skipping is on, and ema = d * ema + (1 - d) * p_new written by the thread that
//                     computed p_new; with clip and ema both null the call IS the plain entry point (its kernel, its bits)
//
// Nothing here reads a gradient on the host, so a captured hipGraph of the training step replays all of it.
#include <math.h>
#include "common.h"

namespace {

constexpr int GN_THREADS = 256;          // 4 waves
constexpr int GN_MAX_BLOCKS = 2048;      // 256 CUs x 8 workgroups
constexpr int GN_MIN_VEC = 1024;         // 16-byte loads per workgroup before a second workgroup is worth its launch (16 KB)

// The grid is a function of n alone (never of the device or of occupancy), so the summation tree, and with it every bit of the
// norm, is the same on every run and on every rank of a data-parallel job.
inline int gn_blocks(size_t n) {
  if (n == 0) return 0;
  const size_t b = ((n >> 2) + GN_MIN_VEC - 1) / GN_MIN_VEC;
  return (int)(b < 1 ? 1 : b > (size_t)GN_MAX_BLOCKS ? (size_t)GN_MAX_BLOCKS : b);
}

// wave fold (6 shuffle levels, lane 0 ends with the sum of the wave), then the 4 wave sums in wave order; valid in thread 0
__device__ __forceinline__ float gn_block_fold(float v) {
  __shared__ float wave_sum[GN_THREADS / 64];
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) v += __shfl_down(v, off, 64);
  if ((threadIdx.x & 63) == 0) wave_sum[threadIdx.x >> 6] = v;
  __syncthreads();
  return ((wave_sum[0] + wave_sum[1]) + wave_sum[2]) + wave_sum[3];
}

// Launch 1.  Workgroup b owns the 16-byte groups [b * per, min((b + 1) * per, n / 4)), per = ceil((n / 4) / gridDim.x); thread t
// takes groups t, t + 256, ... of that range (coalesced: a wave reads 1 KiB per instruction) into four accumulators, one per
// component.  The n % 4 trailing floats go to threads 0..2 of the last workgroup.  g is read with plain loads: the step that
// follows reads it again, out of the caches where it still fits.
__global__ __launch_bounds__(GN_THREADS) void grad_sq_partial_kernel(const float* __restrict__ g, size_t n, float gscale,
                                                                      float* __restrict__ part) {
  const size_t n4 = n >> 2;
  const size_t per = (n4 + gridDim.x - 1) / gridDim.x;
  const size_t lo = (size_t)blockIdx.x * per;
  const size_t hi = lo + per < n4 ? lo + per : n4;
  const f32x4* __restrict__ g4 = reinterpret_cast<const f32x4*>(g);
  float a0 = 0.f, a1 = 0.f, a2 = 0.f, a3 = 0.f;
#pragma unroll 4
  for (size_t i = lo + threadIdx.x; i < hi; i += GN_THREADS) {
    const f32x4 v = g4[i];
    const float x0 = v[0] * gscale, x1 = v[1] * gscale, x2 = v[2] * gscale, x3 = v[3] * gscale;
    a0 = fmaf(x0, x0, a0);
    a1 = fmaf(x1, x1, a1);
    a2 = fmaf(x2, x2, a2);
    a3 = fmaf(x3, x3, a3);
  }
  float acc = (a0 + a1) + (a2 + a3);
  if (blockIdx.x == gridDim.x - 1 && threadIdx.x < (n & 3)) {
    const float x = g[(n4 << 2) + threadIdx.x] * gscale;
    acc = fmaf(x, x, acc);
  }
  const float s = gn_block_fold(acc);
  if (threadIdx.x == 0) part[blockIdx.x] = s;
}

// Launch 2: one workgroup.  Thread t sums partials [t * per, (t + 1) * per) in index order (per = ceil(nparts / 256) <= 8), the 256
// sums are folded as above.  clip = {norm, coef, nonfinite, skipped}: coef is torch.nn.utils.clip_grad_norm_'s
// clamp(max_norm / (norm + 1e-6), max = 1) (1 when max_norm <= 0: clipping off, the norm is still reported); `skipped` counts the
// steps that the *_ex kernels will drop (a float: exact up to 2^24).
__global__ __launch_bounds__(GN_THREADS) void grad_norm_final_kernel(const float* __restrict__ part, int nparts, float max_norm,
                                                                      int skip_nonfinite, float* __restrict__ clip) {
  const int per = (nparts + GN_THREADS - 1) / GN_THREADS;
  const int lo = threadIdx.x * per;
  const int hi = lo + per < nparts ? lo + per : nparts;
  float acc = 0.f;
  for (int i = lo; i < hi; ++i) acc += part[i];
  const float sum = gn_block_fold(acc);
  if (threadIdx.x != 0) return;
  const float norm = sqrtf(sum);
  const bool nonfinite = !(sum < INFINITY);                 // inf or NaN (the sum of squares is never negative)
  float coef = 1.f;
  if (max_norm > 0.f) {
    const float c = max_norm / (norm + 1e-6f);
    coef = c > 1.f ? 1.f : c;                               // NaN stays NaN, as torch.clamp leaves it
  }
  clip[0] = norm;
  clip[1] = coef;
  clip[2] = nonfinite ? 1.f : 0.f;
  if (nonfinite && skip_nonfinite) clip[3] += 1.f;
}

// ---- the extended steps ---------------------------------------------------------------------------------------------------------
// One kernel per optimiser serves the host-lr and the device-hyper form: `hyper` null -> lr and the 1-based step number are the
// host's arguments (and Adam's bias corrections the host's powf, as in cx_adam_step).  The update expressions are those of
// adam_kernel / sgd_nesterov_kernel / rmsprop_kernel and their _dev forms, term by term, with gs = grad_scale * clip[1] in the
// place of grad_scale (clip null: gs = grad_scale * 1).  Same expressions is not same bits: under -ffp-contract=fast the compiler
// fuses b1 * m + (1 - b1) * g and its like into one rounding here, while in adam_kernel it packs the products two by two
// (v_pk_mul_f32) and adds them unfused -- a last-bit difference per step, inside what both kernels are tested to against
// torch.optim.  That is why the entry points below hand a call without clip and without ema to the plain entry point.
struct ExTail {
  const float* clip;
  float* ema;
  float ema_decay;
  int ema_warmup;
  int skip_nonfinite;
};

struct AdamRule {
  float *m, *v;
  float b1, b2, eps, wd, bc1, bc2_sqrt, lr;
  __device__ __forceinline__ void prepare(const float* hyper) {
    if (hyper) {
      const float step = hyper[1] + 1.f;
      lr = hyper[0];
      bc1 = 1.f - powf(b1, step);
      bc2_sqrt = sqrtf(1.f - powf(b2, step));
    }
  }
  __device__ __forceinline__ float update(size_t i, float gi, const float pi) const {
    if (wd != 0.f) gi += wd * pi;
    const float mi = b1 * m[i] + (1.f - b1) * gi;
    const float vi = b2 * v[i] + (1.f - b2) * gi * gi;
    m[i] = mi;
    v[i] = vi;
    const float denom = sqrtf(vi) / bc2_sqrt + eps;
    return pi - (lr / bc1) * (mi / denom);
  }
};

struct SgdRule {
  float* buf;
  float mom, wd, lr;
  int first;
  __device__ __forceinline__ void prepare(const float* hyper) {
    if (hyper) {
      lr = hyper[0];
      first = hyper[1] == 0.f;
    }
  }
  __device__ __forceinline__ float update(size_t i, float gi, const float pi) const {
    if (wd != 0.f) gi += wd * pi;
    const float bi = first ? gi : mom * buf[i] + gi;
    buf[i] = bi;
    return pi - lr * (gi + mom * bi);
  }
};

struct RmsRule {
  float *sq, *buf;
  float alpha, eps, mom, wd, lr;
  __device__ __forceinline__ void prepare(const float* hyper) {
    if (hyper) lr = hyper[0];
  }
  __device__ __forceinline__ float update(size_t i, float gi, const float pi) const {
    if (wd != 0.f) gi += wd * pi;
    const float si = alpha * sq[i] + (1.f - alpha) * gi * gi;
    sq[i] = si;
    const float avg = sqrtf(si) + eps;
    if (mom > 0.f) {
      const float bi = mom * buf[i] + gi / avg;
      buf[i] = bi;
      return pi - lr * bi;
    }
    return pi - lr * gi / avg;
  }
};

template <class Rule>
__global__ __launch_bounds__(256) void step_ex_kernel(Rule r, float* __restrict__ p, const float* __restrict__ g, size_t n,
                                                       const float* __restrict__ hyper, int step, float gscale, ExTail x) {
  if (x.clip && x.skip_nonfinite && x.clip[2] != 0.f) return;        // the whole grid takes the same side: nothing is written
  r.prepare(hyper);
  const float gs = gscale * (x.clip ? x.clip[1] : 1.f);
  float d = x.ema_decay;
  if (x.ema && x.ema_warmup) {
    const float t = hyper ? hyper[1] + 1.f : (float)step;
    d = fminf(d, (1.f + t) / (10.f + t));
  }
  const float omd = 1.f - d;
  for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (size_t)gridDim.x * blockDim.x) {
    const float e = x.ema ? x.ema[i] : 0.f;                          // ahead of the stores: every load of the element is in flight at once
    const float pn = r.update(i, g[i] * gs, p[i]);
    p[i] = pn;
    if (x.ema) x.ema[i] = d * e + omd * pn;
  }
}

inline int step_grid(size_t n) {
  const size_t b = (n + 255) / 256;
  return (int)(b < 1 ? 1 : b > 2048 ? 2048 : b);
}

template <class Rule>
int launch_step_ex(const Rule& r, float* p, const float* g, size_t n, const float* hyper, int step, float gscale, const float* clip,
                   float* ema, float ema_decay, int ema_warmup, int skip_nonfinite, void* stream) {
  if (ema && !(ema_decay >= 0.f && ema_decay <= 1.f)) return CX_EINVAL;
  if (!hyper && step < 1) return CX_EINVAL;
  const ExTail x = {clip, ema, ema_decay, ema_warmup, skip_nonfinite};
  hipLaunchKernelGGL(step_ex_kernel<Rule>, dim3(step_grid(n)), dim3(256), 0, as_stream(stream), r, p, g, n, hyper, step, gscale, x);
  return launch_status();
}

}  // namespace

extern "C" {

int cx_grad_norm_partials(size_t n) { return gn_blocks(n); }

int cx_grad_norm(const float* g, size_t n, float grad_scale, float max_norm, int skip_nonfinite, float* workspace,
                 size_t workspace_floats, float* clip, void* stream) {
  if (!clip || (n && (!g || !workspace))) return CX_EINVAL;
  const int blocks = gn_blocks(n);
  if (workspace_floats < (size_t)blocks) return CX_EINVAL;
  if (n && !aligned16(g)) return CX_EALIGN;
  if (blocks)
    hipLaunchKernelGGL(grad_sq_partial_kernel, dim3(blocks), dim3(GN_THREADS), 0, as_stream(stream), g, n, grad_scale, workspace);
  hipLaunchKernelGGL(grad_norm_final_kernel, dim3(1), dim3(GN_THREADS), 0, as_stream(stream), workspace, blocks, max_norm,
                     skip_nonfinite, clip);
  return launch_status();
}

int cx_adam_step_ex(float* p, const float* g, float* m, float* v, size_t n, float lr, float beta1, float beta2, float eps,
                    float weight_decay, int step, float grad_scale, const float* clip, float* ema, float ema_decay, int ema_warmup,
                    int skip_nonfinite, void* stream) {
  if (!clip && !ema) return cx_adam_step(p, g, m, v, n, lr, beta1, beta2, eps, weight_decay, step, grad_scale, stream);
  if (!p || !g || !m || !v || step < 1) return CX_EINVAL;
  const float bc1 = 1.f - powf(beta1, (float)step);
  const float bc2s = sqrtf(1.f - powf(beta2, (float)step));
  const AdamRule r = {m, v, beta1, beta2, eps, weight_decay, bc1, bc2s, lr};
  return launch_step_ex(r, p, g, n, nullptr, step, grad_scale, clip, ema, ema_decay, ema_warmup, skip_nonfinite, stream);
}

int cx_adam_step_dev_ex(float* p, const float* g, float* m, float* v, size_t n, const float* hyper, float beta1, float beta2,
                        float eps, float weight_decay, float grad_scale, const float* clip, float* ema, float ema_decay,
                        int ema_warmup, int skip_nonfinite, void* stream) {
  if (!clip && !ema) return cx_adam_step_dev(p, g, m, v, n, hyper, beta1, beta2, eps, weight_decay, grad_scale, stream);
  if (!p || !g || !m || !v || !hyper) return CX_EINVAL;
  const AdamRule r = {m, v, beta1, beta2, eps, weight_decay, 1.f, 1.f, 0.f};
  return launch_step_ex(r, p, g, n, hyper, 0, grad_scale, clip, ema, ema_decay, ema_warmup, skip_nonfinite, stream);
}

int cx_sgd_nesterov_step_ex(float* p, const float* g, float* buf, size_t n, float lr, float momentum, float weight_decay,
                            int first_step, int step, float grad_scale, const float* clip, float* ema, float ema_decay,
                            int ema_warmup, int skip_nonfinite, void* stream) {
  if (!clip && !ema) return cx_sgd_nesterov_step(p, g, buf, n, lr, momentum, weight_decay, first_step, grad_scale, stream);
  if (!p || !g || !buf) return CX_EINVAL;
  const SgdRule r = {buf, momentum, weight_decay, lr, first_step};
  return launch_step_ex(r, p, g, n, nullptr, step, grad_scale, clip, ema, ema_decay, ema_warmup, skip_nonfinite, stream);
}

int cx_sgd_nesterov_step_dev_ex(float* p, const float* g, float* buf, size_t n, const float* hyper, float momentum,
                                float weight_decay, float grad_scale, const float* clip, float* ema, float ema_decay, int ema_warmup,
                                int skip_nonfinite, void* stream) {
  if (!clip && !ema) return cx_sgd_nesterov_step_dev(p, g, buf, n, hyper, momentum, weight_decay, grad_scale, stream);
  if (!p || !g || !buf || !hyper) return CX_EINVAL;
  const SgdRule r = {buf, momentum, weight_decay, 0.f, 0};
  return launch_step_ex(r, p, g, n, hyper, 0, grad_scale, clip, ema, ema_decay, ema_warmup, skip_nonfinite, stream);
}

int cx_rmsprop_step_ex(float* p, const float* g, float* sq, float* buf, size_t n, float lr, float alpha, float eps, float momentum,
                       float weight_decay, int step, float grad_scale, const float* clip, float* ema, float ema_decay,
                       int ema_warmup, int skip_nonfinite, void* stream) {
  if (!clip && !ema) return cx_rmsprop_step(p, g, sq, buf, n, lr, alpha, eps, momentum, weight_decay, grad_scale, stream);
  if (!p || !g || !sq || (momentum > 0.f && !buf)) return CX_EINVAL;
  const RmsRule r = {sq, buf, alpha, eps, momentum, weight_decay, lr};
  return launch_step_ex(r, p, g, n, nullptr, step, grad_scale, clip, ema, ema_decay, ema_warmup, skip_nonfinite, stream);
}

int cx_rmsprop_step_dev_ex(float* p, const float* g, float* sq, float* buf, size_t n, const float* hyper, float alpha, float eps,
                           float momentum, float weight_decay, float grad_scale, const float* clip, float* ema, float ema_decay,
                           int ema_warmup, int skip_nonfinite, void* stream) {
  if (!clip && !ema) return cx_rmsprop_step_dev(p, g, sq, buf, n, hyper, alpha, eps, momentum, weight_decay, grad_scale, stream);
  if (!p || !g || !sq || !hyper || (momentum > 0.f && !buf)) return CX_EINVAL;
  const RmsRule r = {sq, buf, alpha, eps, momentum, weight_decay, 0.f};
  return launch_step_ex(r, p, g, n, hyper, 0, grad_scale, clip, ema, ema_decay, ema_warmup, skip_nonfinite, stream);
}

}  // extern "C"
