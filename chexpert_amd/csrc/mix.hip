// Sample-mixing regularisation of the decoded grey images on the GPU: Mixup (Zhang et al., ICLR 2018), CutMix (Yun et al., ICCV 2019)
// and random erasing / Cutout (Zhong et al., AAAI 2020) through ONE primitive, the last step on the uint8 batch in front of the
// network (after cx_u8_clahe, cx_u8_affine and cx_u8_jitter: per-sample transforms first, then the collated batch is mixed), and
// the blend of the targets that goes with it.  The caller draws the plan (chexpert_amd/augment.py: mix_plan, erase_plan); the numpy
// statements mix_reference / target_mix_reference are what the tests hold the two kernels to, bit for bit.
//
// cx_u8_mix, integers throughout.  Per row b: p = perm[b] clamped to [-1, B-1], q = lam_q[b] clamped to [0, 65536], the box clamped
// to the image (rows [y0, y1), columns [x0, x1)).  Pixel (i, j) with a = x[b][i][j]: outside the box y = a; inside it
// o = (p < 0) ? fill : x[p][i][j] and y = (q*a + (65536 - q)*o + 32768) >> 16 -- round-half-up of lambda*a + (1 - lambda)*o with
// lambda = q / 65536; the sum stays below 2^24, so it is exact.  Mixup: box = the image, any q.  CutMix: a partial box, q = 0.
// Erasing: p = -1, q = 0.
// A stream: one lane = V consecutive bytes of the image (V = 16 where W % 16 == 0 and both images are 16-byte aligned, else 4: a
// lane's bytes share the row), one workgroup = MIX_U * 256 consecutive lanes' worth of one image, i.e. a band of whole and partial
// rows, so the row parameters are uniform per workgroup (scalar loads) and every access is a contiguous run of the image.  A band
// that no pixel of the row's box falls into, a row with q = 65536 and a row mixed with itself (p = b) are straight copies: the
// partner is not loaded.  Elsewhere a lane loads its partner bytes only where its own bytes meet the box.  Because of the clamps
// no load leaves the batch whatever the parameter arrays hold.  One writer per byte, no atomics: the same bits on every run.
//
// cx_target_mix, fp32, every product and sum rounded on its own (the Makefile compiles this file with -ffp-contract=off, as
// saliency.hip: the tree-wide -ffp-contract=fast would fuse w*t + (1-w)*u into one rounding).  p and w_q clamped as above,
// w = w_q / 65536 (w and 1 - w are exact in fp32).  p < 0 or w_q == 65536: out = t[b][c].  Else t[b][c] < 0 or t[p][c] < 0: out = -1
// (a label the loss ignores stays ignored: blending it with a real label would fabricate one).  Else out = w*t[b][c] + (1-w)*t[p][c].
// Measured times: DESIGN.md section 4.34.
#include "common.h"

namespace {

constexpr int MIX_U = 2;      // vectors per lane: both loads of a lane (and of its partner) are issued before the arithmetic

__device__ __forceinline__ uint32_t mix_dword(const uint32_t a, const uint32_t o, const int j, const int x0, const int x1, const uint32_t q) {
  uint32_t r = 0;
#pragma unroll
  for (int e = 0; e < 4; ++e) {
    const uint32_t av = (a >> (8 * e)) & 255u, ov = (o >> (8 * e)) & 255u;
    const uint32_t m = (q * av + (65536u - q) * ov + 32768u) >> 16;
    r |= ((j + e >= x0 && j + e < x1) ? m : av) << (8 * e);
  }
  return r;
}

template <int V> struct MixVec;
template <> struct MixVec<4> {
  typedef uint32_t T;
  static __device__ __forceinline__ T splat(uint32_t v) { return v; }
  static __device__ __forceinline__ T mix(const T a, const T o, int j, int x0, int x1, uint32_t q) { return mix_dword(a, o, j, x0, x1, q); }
};
template <> struct MixVec<16> {
  typedef uint4 T;
  static __device__ __forceinline__ T splat(uint32_t v) { return make_uint4(v, v, v, v); }
  static __device__ __forceinline__ T mix(const T a, const T o, int j, int x0, int x1, uint32_t q) {
    return make_uint4(mix_dword(a.x, o.x, j, x0, x1, q), mix_dword(a.y, o.y, j + 4, x0, x1, q), mix_dword(a.z, o.z, j + 8, x0, x1, q),
                      mix_dword(a.w, o.w, j + 12, x0, x1, q));
  }
};

// grid: B * chunks workgroups; workgroup (b, c) owns vectors [c * 256 * MIX_U, (c + 1) * 256 * MIX_U) of image b (nv = H * W / V each)
template <int V>
__global__ __launch_bounds__(256) void u8_mix_kernel(const uint8_t* __restrict__ x, uint8_t* __restrict__ y, int B, int H, int W,
                                                     const int* __restrict__ perm, const int* __restrict__ lam_q,
                                                     const int* __restrict__ box, uint32_t fill4, int chunks) {
  typedef typename MixVec<V>::T T;
  const int b = blockIdx.x / chunks, c = blockIdx.x - b * chunks;
  const int wv = W / V, nv = H * wv;
  const int p = min(max(perm[b], -1), B - 1);
  const uint32_t q = (uint32_t)min(max(lam_q[b], 0), 65536);
  const int y0 = min(max(box[4 * b], 0), H), y1 = min(max(box[4 * b + 1], 0), H);
  const int x0 = min(max(box[4 * b + 2], 0), W), x1 = min(max(box[4 * b + 3], 0), W);
  const T* src = reinterpret_cast<const T*>(x + (size_t)b * H * W);
  T* dst = reinterpret_cast<T*>(y + (size_t)b * H * W);
  const int v0 = c * (256 * MIX_U), vend = min(v0 + 256 * MIX_U, nv);
  int v[MIX_U];
  T a[MIX_U];
#pragma unroll
  for (int k = 0; k < MIX_U; ++k) {
    v[k] = v0 + k * 256 + (int)threadIdx.x;
    if (v[k] < nv) a[k] = src[v[k]];
  }
  // the rows of this band: [v0 / wv, (vend - 1) / wv]; nothing of the box inside, lambda = 1 or the row is its own partner: a copy
  const bool touched = q != 65536u && p != b && x1 > x0 && y0 <= (vend - 1) / wv && y1 > v0 / wv;      // (uniform)
  if (!touched) {
#pragma unroll
    for (int k = 0; k < MIX_U; ++k)
      if (v[k] < nv) dst[v[k]] = a[k];
    return;
  }
  const T* other = p < 0 ? nullptr : reinterpret_cast<const T*>(x + (size_t)p * H * W);
  int j[MIX_U];
  bool in[MIX_U];
  T o[MIX_U];
#pragma unroll
  for (int k = 0; k < MIX_U; ++k) {
    const int i = v[k] / wv;
    j[k] = (v[k] - i * wv) * V;
    in[k] = v[k] < nv && i >= y0 && i < y1 && j[k] < x1 && j[k] + V > x0;      // some byte of the vector lies in the box
    o[k] = MixVec<V>::splat(fill4);
    if (in[k] && other) o[k] = other[v[k]];
  }
#pragma unroll
  for (int k = 0; k < MIX_U; ++k)
    if (v[k] < nv) dst[v[k]] = in[k] ? MixVec<V>::mix(a[k], o[k], j[k], x0, x1, q) : a[k];
}

__global__ __launch_bounds__(256) void target_mix_kernel(const float* __restrict__ t, float* __restrict__ out, int B, int n,
                                                         const int* __restrict__ perm, const int* __restrict__ tw_q) {
  const int e = blockIdx.x * 256 + threadIdx.x;
  if (e >= B * n) return;
  const int b = e / n, c = e - b * n;
  const int p = min(max(perm[b], -1), B - 1), wq = min(max(tw_q[b], 0), 65536);
  const float own = t[e];
  float r = own;
  if (p >= 0 && wq != 65536) {
    const float oth = t[(size_t)p * n + c];
    const float w = (float)wq * 0x1p-16f, w1 = 1.f - w;                 // both exact
    const float m0 = w * own, m1 = w1 * oth;                            // (no contraction in this file: two products, one sum)
    r = (own < 0.f || oth < 0.f) ? -1.f : m0 + m1;
  }
  out[e] = r;
}

inline bool al4(const void* p) { return (((uintptr_t)p) & 3) == 0; }

}  // namespace

int cx_u8_mix(const uint8_t* x, uint8_t* y, int B, int H, int W, const int* perm, const int* lam_q, const int* box, int fill,
              void* stream) {
  if (!x || !y || !perm || !lam_q || !box || x == y || B <= 0 || H <= 0 || W <= 0 || fill < 0 || fill > 255) return CX_EINVAL;
  if ((W % 4) || W > 1024 || H > 1024) return CX_ESHAPE;
  if (!al4(x) || !al4(y) || !al4(perm) || !al4(lam_q) || !al4(box)) return CX_EALIGN;      // one dword (or four) per lane, both ways
  const bool wide = W % 16 == 0 && aligned16(x) && aligned16(y);
  const int nv = H * (W / (wide ? 16 : 4));
  const int chunks = (nv + 256 * MIX_U - 1) / (256 * MIX_U);
  if ((long long)B * chunks >= (1ll << 31) / 8) return CX_ESHAPE;       // (image offsets are 64-bit: B * H * W itself may exceed 2^31)
  const uint32_t fill4 = (uint32_t)fill * 0x01010101u;
  if (wide)
    hipLaunchKernelGGL(u8_mix_kernel<16>, dim3((unsigned)(B * chunks)), dim3(256), 0, as_stream(stream), x, y, B, H, W, perm, lam_q, box,
                       fill4, chunks);
  else
    hipLaunchKernelGGL(u8_mix_kernel<4>, dim3((unsigned)(B * chunks)), dim3(256), 0, as_stream(stream), x, y, B, H, W, perm, lam_q, box,
                       fill4, chunks);
  return launch_status();
}

int cx_target_mix(const float* t, float* out, int B, int n, const int* perm, const int* tw_q, void* stream) {
  if (!t || !out || !perm || !tw_q || out == t || B <= 0 || n <= 0) return CX_EINVAL;
  if ((long long)B * n >= (1ll << 31) - 256) return CX_ESHAPE;
  if (!al4(t) || !al4(out) || !al4(perm) || !al4(tw_q)) return CX_EALIGN;
  hipLaunchKernelGGL(target_mix_kernel, dim3((unsigned)((B * n + 255) / 256)), dim3(256), 0, as_stream(stream), t, out, B, n, perm, tw_q);
  return launch_status();
}
