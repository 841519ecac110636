// Pixel attribution maps (chexpert_amd/saliency.py: input_gradient, smoothgrad, integrated_gradients): the glue around the eval-mode
// forward + backward with dx.  BatchNorm is frozen in eval mode, so the rows of a batch do not influence each other and all path
// points / noise samples of an image ride in one batch.  Three entry points (include/chexpert_hip.h states their arithmetic; the numpy
// statements `*_reference` of saliency.py are what the tests hold them to, bit for bit except for the noise term):
//   cx_sal_points      the rows the network is evaluated at: base + alpha * (x - base) [+ sigma * n(seed, index)]
//   cx_sal_accumulate  acc[slot[r]] (+)= w[r] * g[r] (or g[r]^2), rows in ascending order
//   cx_sal_finish      acc [* (x - base)], reduced over the three channels, and its sum per plane (the completeness identity)
// fp32 NCHW throughout (the float interface of the models and of cx_stem_input_grad).  One writer per output element, no atomics:
// the same bits on every run.  All three are streams: one float4 per lane where a row (3 H W floats) is a multiple of four floats
// and every pointer is 16-byte aligned (then H W % 4 == 0 too, so a float4 never straddles a channel), one float per lane otherwise.
// Every statement below is a separate, rounded fp32 operation: the Makefile compiles this file with -ffp-contract=off.  Under the
// -ffp-contract=fast of the other files the backend fuses a * b + c into one rounding whatever the source says (__fmul_rn / __fadd_rn
// are plain * and + in this toolchain's headers, and a contract(off) pragma does not reach the target-wide option);
// tests/test_saliency_gpu.py holds inputs that tell the two apart.
// Measured at (32, 3, 320, 320) against cx_copy_stream on the same bytes: DESIGN.md section 4.33.
#include "common.h"

namespace {

constexpr int SAL_PARTIALS = CX_SAL_PARTIALS;      // workgroups (= partial sums of `total`) per plane of cx_sal_finish

__device__ __forceinline__ float sal_mul(const float a, const float b) { return a * b; }
__device__ __forceinline__ float sal_add(const float a, const float b) { return a + b; }
__device__ __forceinline__ float sal_sub(const float a, const float b) { return a - b; }

// one standard normal per hash (Box-Muller, the cosine branch only, so that a draw depends on (seed, k) alone)
__device__ __forceinline__ float sal_normal(const uint64_t seed, const uint64_t k) {
  uint64_t z = seed + 0x9E3779B97F4A7C15ull * (k + 1ull);              // splitmix64, as boot_draw / the dropout masks
  z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
  z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
  z ^= z >> 31;
  const float u1 = (float)((uint32_t)(z >> 40) + 1u) * 0x1p-24f;       // in (0, 1]: exact (at most 2^24)
  const float u2 = (float)((uint32_t)(z >> 8) & 0xFFFFFFu) * 0x1p-24f; // in [0, 1): exact
  return sal_mul(sqrtf(sal_mul(-2.f, logf(u1))), cospif(sal_mul(2.f, u2)));
}

template <int V> struct Vec;
template <> struct Vec<4> {
  typedef float4 T;
  static __device__ __forceinline__ float get(const T& v, int j) { return j == 0 ? v.x : j == 1 ? v.y : j == 2 ? v.z : v.w; }
  static __device__ __forceinline__ T make(const float (&a)[4]) { return make_float4(a[0], a[1], a[2], a[3]); }
  static __device__ __forceinline__ T splat(float a) { return make_float4(a, a, a, a); }
};
template <> struct Vec<1> {
  typedef float T;
  static __device__ __forceinline__ float get(const T& v, int) { return v; }
  static __device__ __forceinline__ T make(const float (&a)[1]) { return a[0]; }
  static __device__ __forceinline__ T splat(float a) { return a; }
};

// ---- cx_sal_points: grid (chunks of a row, R) ---------------------------------------------------------------------------------------
// img[r] is clamped into [0, B): a table on the device is never trusted with an address.  NOISE is a template parameter: left to a
// run-time test the compiler turns the branch into a select and the hash, logf and cospif run for every element of a noise-free row.
template <int V, bool NOISE>
__global__ __launch_bounds__(256) void sal_points_kernel(const float* __restrict__ x, const float* __restrict__ base, float b0, float b1,
                                                         float b2, const int32_t* __restrict__ img, const float* __restrict__ alpha,
                                                         const float* __restrict__ sigma, uint64_t seed, uint64_t first_row,
                                                         float* __restrict__ out, int B, int HW) {
  typedef typename Vec<V>::T T;
  const int N = 3 * HW, nv = N / V;
  const int r = blockIdx.y;
  const int b = min(max(img[r], 0), B - 1);
  const float al = alpha[r];
  const float sg = NOISE ? sigma[b] : 0.f;
  const uint64_t k0 = (first_row + (uint64_t)r) * (uint64_t)N;
  const T* xr = reinterpret_cast<const T*>(x + (size_t)b * N);
  const T* br = base ? reinterpret_cast<const T*>(base + (size_t)b * N) : nullptr;
  T* outr = reinterpret_cast<T*>(out + (size_t)r * N);
  for (int i = blockIdx.x * 256 + threadIdx.x; i < nv; i += gridDim.x * 256) {
    const int e = i * V;
    const T xv = xr[i];
    const int c = e / HW;                                        // (V == 4: H W % 4 == 0, the four elements share the channel)
    const T bv = br ? br[i] : Vec<V>::splat(c == 0 ? b0 : c == 1 ? b1 : b2);
    float o[V];
#pragma unroll
    for (int j = 0; j < V; ++j) {
      const float bb = Vec<V>::get(bv, j);
      const float d = sal_sub(Vec<V>::get(xv, j), bb);
      float v = sal_add(bb, sal_mul(al, d));
      if (NOISE) v = sal_add(v, sal_mul(sg, sal_normal(seed, k0 + (uint64_t)(e + j))));
      o[j] = v;
    }
    outr[i] = Vec<V>::make(o);
  }
}

// ---- cx_sal_accumulate: grid (chunks of a plane, P) ---------------------------------------------------------------------------------
// A lane owns its elements of plane p and walks the rows in ascending order; slot[r] is wave-uniform, so a row of another plane costs
// one scalar compare.  Four rows' loads are issued before the first is consumed.  A slot outside [0, P) matches no plane.
template <int V>
__global__ __launch_bounds__(256) void sal_accumulate_kernel(const float* __restrict__ g, const int32_t* __restrict__ slot,
                                                             const float* __restrict__ w, float* __restrict__ acc, int R, int N, int square,
                                                             int accumulate) {
  typedef typename Vec<V>::T T;
  const int nv = N / V;
  const int p = blockIdx.y;
  T* accp = reinterpret_cast<T*>(acc + (size_t)p * N);
  for (int i = blockIdx.x * 256 + threadIdx.x; i < nv; i += gridDim.x * 256) {
    float a[V];
    {
      const T old = accumulate ? accp[i] : Vec<V>::splat(0.f);
#pragma unroll
      for (int j = 0; j < V; ++j) a[j] = Vec<V>::get(old, j);
    }
    for (int r0 = 0; r0 < R; r0 += 4) {
      T v[4];
      bool m[4];
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        m[q] = r0 + q < R && slot[r0 + q] == p;
        if (m[q]) v[q] = reinterpret_cast<const T*>(g + (size_t)(r0 + q) * N)[i];
      }
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        if (!m[q]) continue;
        const float wr = w[r0 + q];
#pragma unroll
        for (int j = 0; j < V; ++j) {
          const float gv = Vec<V>::get(v[q], j);
          const float t = square ? sal_mul(gv, gv) : gv;
          a[j] = sal_add(a[j], sal_mul(wr, t));
        }
      }
    }
    accp[i] = Vec<V>::make(a);
  }
}

// ---- cx_sal_finish: grid (SAL_PARTIALS, P) ------------------------------------------------------------------------------------------
// A lane owns V pixels of plane p in all three channels.  `total`: every lane sums its a values in double in the order it meets
// them, the 64 lanes of a wave through a fixed shuffle tree, the four waves in wave order through LDS: partial[p][workgroup]; the second
// launch adds the SAL_PARTIALS partials of a plane in ascending order.
template <int V>
__global__ __launch_bounds__(256) void sal_finish_kernel(const float* __restrict__ acc, const float* __restrict__ x,
                                                         const float* __restrict__ base, float b0, float b1, float b2,
                                                         const int32_t* __restrict__ img_of, float* __restrict__ out,
                                                         double* __restrict__ partial, int B, int HW, int times_input, int mode) {
  typedef typename Vec<V>::T T;
  __shared__ double wsum[4];
  const int nv = HW / V;
  const int p = blockIdx.y;
  const size_t N = (size_t)3 * HW;
  const int b = times_input ? min(max(img_of[p], 0), B - 1) : 0;
  const float bc[3] = {b0, b1, b2};
  double tot = 0.0;
  for (int i = blockIdx.x * 256 + threadIdx.x; i < nv; i += gridDim.x * 256) {
    float a[3][V];
#pragma unroll
    for (int c = 0; c < 3; ++c) {
      const T av = reinterpret_cast<const T*>(acc + p * N + (size_t)c * HW)[i];
      if (times_input) {                                         // uniform
        const T xv = reinterpret_cast<const T*>(x + b * N + (size_t)c * HW)[i];
        const T bv = base ? reinterpret_cast<const T*>(base + b * N + (size_t)c * HW)[i] : Vec<V>::splat(bc[c]);
#pragma unroll
        for (int j = 0; j < V; ++j) a[c][j] = sal_mul(Vec<V>::get(av, j), sal_sub(Vec<V>::get(xv, j), Vec<V>::get(bv, j)));
      } else {
#pragma unroll
        for (int j = 0; j < V; ++j) a[c][j] = Vec<V>::get(av, j);
      }
    }
#pragma unroll
    for (int j = 0; j < V; ++j) {
      tot += (double)a[0][j];
      tot += (double)a[1][j];
      tot += (double)a[2][j];
    }
    if (mode == CX_SAL_NONE) {
#pragma unroll
      for (int c = 0; c < 3; ++c) reinterpret_cast<T*>(out + p * N + (size_t)c * HW)[i] = Vec<V>::make(a[c]);
    } else {
      float o[V];
#pragma unroll
      for (int j = 0; j < V; ++j) {
        if (mode == CX_SAL_SUM)
          o[j] = sal_add(sal_add(a[0][j], a[1][j]), a[2][j]);
        else if (mode == CX_SAL_ABS)
          o[j] = sal_add(sal_add(fabsf(a[0][j]), fabsf(a[1][j])), fabsf(a[2][j]));
        else
          o[j] = fmaxf(fmaxf(fabsf(a[0][j]), fabsf(a[1][j])), fabsf(a[2][j]));
      }
      reinterpret_cast<T*>(out + (size_t)p * HW)[i] = Vec<V>::make(o);
    }
  }
  if (!partial) return;                                          // uniform
#pragma unroll
  for (int d = 32; d >= 1; d >>= 1) tot += __shfl_down(tot, d, 64);
  if ((threadIdx.x & 63) == 0) wsum[threadIdx.x >> 6] = tot;
  __syncthreads();
  if (threadIdx.x == 0) partial[(size_t)p * SAL_PARTIALS + blockIdx.x] = ((wsum[0] + wsum[1]) + wsum[2]) + wsum[3];
}

__global__ __launch_bounds__(64) void sal_total_kernel(const double* __restrict__ partial, double* __restrict__ total, int P) {
  const int p = blockIdx.x * 64 + threadIdx.x;
  if (p >= P) return;
  double s = 0.0;
  for (int k = 0; k < SAL_PARTIALS; ++k) s += partial[(size_t)p * SAL_PARTIALS + k];
  total[p] = s;
}

inline bool al4(const void* p) { return (((uintptr_t)p) & 3) == 0; }
inline bool al16(const void* p) { return (((uintptr_t)p) & 15) == 0; }      // (a null pointer counts as aligned)
// H W < 2^29 keeps 3 H W (+ the stride of a grid-stride loop) inside an int
inline bool sal_shape_ok(int H, int W, long long rows) { return (long long)H * W < (1ll << 29) && rows <= 65535; }
inline unsigned sal_blocks(int nv) { return (unsigned)min((nv + 255) / 256, 2048); }

}  // namespace

int cx_sal_points(const float* x, const float* base, float base0, float base1, float base2, const int32_t* img, const float* alpha,
                  const float* sigma, uint64_t seed, uint64_t first_row, float* out, int B, int R, int H, int W, void* stream) {
  if (!x || !img || !alpha || !out || B <= 0 || R <= 0 || H <= 0 || W <= 0 || out == x || out == base) return CX_EINVAL;
  if (!sal_shape_ok(H, W, R)) return CX_ESHAPE;
  if (!al4(x) || !al4(base) || !al4(img) || !al4(alpha) || !al4(sigma) || !al4(out)) return CX_EALIGN;
  const int HW = H * W, N = 3 * HW;
  const bool wide = N % 4 == 0 && al16(x) && al16(base) && al16(out);
  const dim3 grid(sal_blocks(wide ? N / 4 : N), (unsigned)R);
  auto kern = wide ? (sigma ? sal_points_kernel<4, true> : sal_points_kernel<4, false>)
                   : (sigma ? sal_points_kernel<1, true> : sal_points_kernel<1, false>);
  hipLaunchKernelGGL(kern, grid, dim3(256), 0, as_stream(stream), x, base, base0, base1, base2, img, alpha, sigma, seed, first_row, out, B, HW);
  return launch_status();
}

int cx_sal_accumulate(const float* g, const int32_t* slot, const float* w, float* acc, int R, int P, int H, int W, int square,
                      int accumulate, void* stream) {
  if (!g || !slot || !w || !acc || R <= 0 || P <= 0 || H <= 0 || W <= 0 || (const float*)acc == g) return CX_EINVAL;
  if (!sal_shape_ok(H, W, P)) return CX_ESHAPE;
  if (!al4(g) || !al4(slot) || !al4(w) || !al4(acc)) return CX_EALIGN;
  const int N = 3 * H * W;
  const bool wide = N % 4 == 0 && al16(g) && al16(acc);
  const dim3 grid(sal_blocks(wide ? N / 4 : N), (unsigned)P);
  if (wide)
    hipLaunchKernelGGL(sal_accumulate_kernel<4>, grid, dim3(256), 0, as_stream(stream), g, slot, w, acc, R, N, square, accumulate);
  else
    hipLaunchKernelGGL(sal_accumulate_kernel<1>, grid, dim3(256), 0, as_stream(stream), g, slot, w, acc, R, N, square, accumulate);
  return launch_status();
}

int cx_sal_finish(const float* acc, const float* x, const float* base, float base0, float base1, float base2, const int32_t* img_of,
                  float* out, double* total, double* partial, int P, int B, int H, int W, int times_input, int mode, void* stream) {
  if (!acc || !out || P <= 0 || H <= 0 || W <= 0 || (const float*)out == acc) return CX_EINVAL;
  if (times_input && (!x || !img_of || B <= 0 || (const float*)out == x || (const float*)out == base)) return CX_EINVAL;
  if (total && !partial) return CX_EINVAL;
  if (mode < CX_SAL_NONE || mode > CX_SAL_MAX || !sal_shape_ok(H, W, P)) return CX_ESHAPE;
  if (!al4(acc) || !al4(x) || !al4(base) || !al4(img_of) || !al4(out) || (((uintptr_t)total) & 7) || (((uintptr_t)partial) & 7)) return CX_EALIGN;
  if (!times_input) x = base = nullptr, img_of = nullptr;
  const int HW = H * W;
  const bool wide = HW % 4 == 0 && al16(acc) && al16(x) && al16(base) && al16(out);
  const dim3 grid((unsigned)SAL_PARTIALS, (unsigned)P);
  double* part = total ? partial : nullptr;
  if (wide)
    hipLaunchKernelGGL(sal_finish_kernel<4>, grid, dim3(256), 0, as_stream(stream), acc, x, base, base0, base1, base2, img_of, out, part, B,
                       HW, times_input, mode);
  else
    hipLaunchKernelGGL(sal_finish_kernel<1>, grid, dim3(256), 0, as_stream(stream), acc, x, base, base0, base1, base2, img_of, out, part, B,
                       HW, times_input, mode);
  if (total) hipLaunchKernelGGL(sal_total_kernel, dim3((unsigned)((P + 63) / 64)), dim3(64), 0, as_stream(stream), partial, total, P);
  return launch_status();
}
