// Input gradient of the stem convolution (cx_stem_input_grad): the gradient that reaches the 3-channel image through
// features.conv0 / conv1 / stem[0] of the reference nets, for x.grad in training mode.
//
//   dx[b, c, iy, ix] = sum_{o, ky, kx} W[o, c, ky, kx] * g[b, oy, ox, o],   iy = s*oy - pad + ky (same for x),  c = 0..2
//   g = pa[o] * dz + pb[o] * y + pc[o]          (the PRO_AFFINE2 prologue of the stem's weight gradient: dz = gradient at the
//                                                 stem BatchNorm's output side, y = the stored convolution output)
//
// dz / y are NHWC (B, Ho, Wo, >= C0) in the engine's storage type; W is the fp32 master (C0, wc, k, k) (wc >= 3: the first three
// input channels are the image's); dx is fp32 NCHW (B, 3, H, W), every element written (no accumulation, no atomics: each
// element has ONE owning lane and a fixed summation order, so the result is bit-reproducible).
//
// Two kernels:
//  * stem_dgrad_s2_kernel (bf16 storage, stride 2, k = 7 / pad 3 or k = 3 / pad 0 | 1, C0 a multiple of 8 up to 64): depth-to-space
//    over 2x2 input cells.  The four pixels (2cy+py, 2cx+px) of a cell receive gradient only from the R x R window of g rows /
//    columns cy + dmin .. cy + dmin + R - 1 (R = 4, dmin = -1 for 7x7 pad 3; R = 2 for 3x3), so the operation is an implicit
//    GEMM with M = cells, N = 16 = 4 parities x (3 channels + 1 zero), K = R*R x C0 (padded to 32 | 64) on
//    v_mfma_f32_16x16x32_bf16.  The weights, re-laid out with zeros for impossible taps ([R*R][K/8][16][8] bf16, 32 KB for the
//    7x7 stem), sit in LDS for the whole workgroup.  A workgroup owns 64 cells of a cell row (one 16-cell M tile per wave) and
//    walks down CH cell rows; each step adds ONE new g row (a stride-2 cell row moves the window by one output row) to an
//    R-row ring in LDS, formed once from dz, y and the coefficients, so every g element is formed once per workgroup and read
//    by up to R*R cells from LDS.
//  * stem_dgrad_generic_kernel (fp32 storage at every geometry above, and the stride-1 CIFAR stems -- 3x3 pad 1, 5x5 pad 2 -- in
//    either storage type; C0 up to 128): one lane per input pixel, VALU, taps in (ky, kx) order, channels ascending.
//
// Rounding (the kernel test mirrors it): in bf16 storage g is rounded to bf16 exactly as the stem weight-gradient prologue rounds
// its operand -- bf16(fmaf(dz, pa, fmaf(y, pb, pc))), RNE -- and W to bf16 (RNE of the fp32 master); products and sums are fp32.
// In fp32 storage everything is fp32 (g = fmaf(dz, pa, fmaf(y, pb, pc)), no rounding of W), VALU fmaf chains.
// Anything else returns CX_EUNSUPPORTED: there is no silent fall-back.
#include "common.h"

namespace {

// ------------------------------------------------------------------------------------------------ stride-2 MFMA form (bf16)
constexpr int SD_CW = 64;                 // cells per workgroup row (4 waves x 16)
constexpr int SD_CH = 32;                 // cell rows per workgroup

typedef __attribute__((ext_vector_type(4))) float sd_f32x4;

template <int R, int NKC>                 // R: window width (4 | 2); NKC: 32-channel K chunks per window position (C0 <= 32 NKC)
struct SdLayout {
  static constexpr int TW = SD_CW + R - 1;                  // g pixels of one ring row
  static constexpr int PP = NKC * 64 + 16;                  // bytes per g pixel (+16: conflict-free ds_read_b128 across lanes)
  static constexpr int ROW = TW * PP;
  static constexpr int RING = R * ROW;
  static constexpr int WB = R * R * NKC * 4 * 16 * 16;      // weight fragments: [R*R][NKC*4 k-groups][16 n][8 bf16]
  static constexpr int STG = 4 * 6 * 32 * 4;                // per-wave output staging [3 c][2 py][32 ix] fp32
  static constexpr int COEF = 3 * 64 * 4;
  static constexpr int BYTES = RING + WB + STG + COEF;
  static constexpr int CPP = NKC * 4;                       // 16-B chunks (8 channels) of one g pixel
  static constexpr int CHUNKS = TW * CPP;                   // ... and of one g row
  static constexpr int SLOTS = (CHUNKS + 255) / 256;
};

template <int R, int NKC>
__global__ __launch_bounds__(256, 2) void stem_dgrad_s2_kernel(const bf16* __restrict__ dz, const bf16* __restrict__ y,
                                                                const float* __restrict__ pa, const float* __restrict__ pb,
                                                                const float* __restrict__ pc, const float* __restrict__ w,
                                                                float* __restrict__ dx, const int ldz, const int ldy, const int wc,
                                                                const int H, const int W, const int Ho, const int Wo, const int C0,
                                                                const int k, const int pad, const int dmin) {
  using L = SdLayout<R, NKC>;
  extern __shared__ __attribute__((aligned(16))) char smem[];
  char* ring = smem;
  char* wl = smem + L::RING;
  float* stg = reinterpret_cast<float*>(wl + L::WB);
  float* coef = stg + L::STG / 4;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int b = blockIdx.z;
  const int cx0 = blockIdx.x * SD_CW, cy0 = blockIdx.y * SD_CH;
  const int ncy = (H + 1) >> 1;
  const int nsteps = min(SD_CH, ncy - cy0);

  // weights -> [wy][wx][kg][n][8] bf16; n = py*8 + px*4 + c, k = kg*8 + j = input channel o of the convolution's output
  for (int e = tid; e < L::WB / 2; e += 256) {
    const int j = e & 7, n = (e >> 3) & 15, kg = (e >> 7) % (NKC * 4), pos = (e >> 7) / (NKC * 4);
    const int wy = pos / R, wx = pos - wy * R;
    const int py = n >> 3, px = (n >> 2) & 1, c = n & 3, o = kg * 8 + j;
    const int ky = py + pad - 2 * (dmin + wy), kx = px + pad - 2 * (dmin + wx);
    float v = 0.f;
    if (c < 3 && o < C0 && ky >= 0 && ky < k && kx >= 0 && kx < k) v = w[((size_t)(o * wc + c) * k + ky) * k + kx];
    reinterpret_cast<bf16*>(wl)[e] = f2bf(v);
  }
  if (tid < 64) {
    coef[tid] = tid < C0 ? pa[tid] : 0.f;
    coef[64 + tid] = tid < C0 ? pb[tid] : 0.f;
    coef[128 + tid] = tid < C0 ? pc[tid] : 0.f;
  }
  __syncthreads();

  // one g row: chunk ci = t * CPP + q (pixel t of the row, channels 8q .. 8q+7)
  uint4 rz[L::SLOTS], ry[L::SLOTS];
  bool rv[L::SLOTS];
  auto load_row = [&](int oy) {
#pragma unroll
    for (int i = 0; i < L::SLOTS; ++i) {
      const int ci = tid + 256 * i;
      const int t = ci / L::CPP, q = ci - t * L::CPP;
      const int ox = cx0 + dmin + t;
      rv[i] = ci < L::CHUNKS && q * 8 < C0 && oy >= 0 && oy < Ho && ox >= 0 && ox < Wo;
      if (rv[i]) {
        const size_t pix = ((size_t)b * Ho + oy) * Wo + ox;
        rz[i] = *reinterpret_cast<const uint4*>(dz + pix * ldz + q * 8);
        ry[i] = *reinterpret_cast<const uint4*>(y + pix * ldy + q * 8);
      }
    }
  };
  auto store_row = [&](int oy) {
    char* row = ring + ((oy - dmin - cy0 + R) % R) * L::ROW;      // ring slot of g row oy (oy - dmin - cy0 >= -R + 1)
#pragma unroll
    for (int i = 0; i < L::SLOTS; ++i) {
      const int ci = tid + 256 * i;
      if (ci < L::CHUNKS) {
        const int t = ci / L::CPP, q = ci - t * L::CPP;
        const uint4 o = rv[i] ? cx_affine2_8(rz[i], ry[i], coef + q * 8, coef + 64 + q * 8, coef + 128 + q * 8) : make_uint4(0, 0, 0, 0);
        *reinterpret_cast<uint4*>(row + t * L::PP + q * 16) = o;
      }
    }
  };

  // prime the ring with the first R - 1 rows of the window of cell row cy0
  for (int r = 0; r < R - 1; ++r) {
    load_row(cy0 + dmin + r);
    store_row(cy0 + dmin + r);
  }
  if (nsteps > 0) load_row(cy0 + dmin + R - 1);

  const bool wave_live = cx0 + wave * 16 < ((W + 1) >> 1);
  const int arow = wave * 16 + (lane & 15), kq = lane >> 4;
  float* wst = stg + wave * 192;
  for (int s = 0; s < nsteps; ++s) {
    const int cy = cy0 + s;
    store_row(cy + dmin + R - 1);              // the newest row of this step's window (its slot held row cy + dmin - 1)
    __syncthreads();
    if (s + 1 < nsteps) load_row(cy + dmin + R);
    sd_f32x4 acc = {0.f, 0.f, 0.f, 0.f};
    if (wave_live) {
#pragma unroll
      for (int wy = 0; wy < R; ++wy) {
        const char* row = ring + ((cy + wy - cy0 + R) % R) * L::ROW;   // g row cy + dmin + wy
#pragma unroll
        for (int wx = 0; wx < R; ++wx)
#pragma unroll
          for (int kc = 0; kc < NKC; ++kc) {
            const bf16x8 af = *reinterpret_cast<const bf16x8*>(row + (arow + wx) * L::PP + kc * 64 + kq * 16);
            const bf16x8 bfr = *reinterpret_cast<const bf16x8*>(wl + (((wy * R + wx) * NKC + kc) * 4 + kq) * 256 + (lane & 15) * 16);
            acc = __builtin_amdgcn_mfma_f32_16x16x32_bf16(af, bfr, acc, 0, 0, 0);
          }
      }
      // D: column n = lane & 15 = (py, px, c), rows 4 kq + r = cells -> staging [c][py][2 cell + px]
      const int n = lane & 15, py = n >> 3, px = (n >> 2) & 1, c = n & 3;
      if (c < 3) {
#pragma unroll
        for (int r = 0; r < 4; ++r) wst[(c * 2 + py) * 32 + 2 * (kq * 4 + r) + px] = acc[r];
      }
    }
    __syncthreads();
    if (wave_live) {
      const int ixb = 2 * (cx0 + wave * 16);
#pragma unroll
      for (int i = 0; i < 3; ++i) {
        const int e = lane + 64 * i;
        const int cp = e >> 5, xi = e & 31;
        const int c = cp >> 1, iy = 2 * cy + (cp & 1), ix = ixb + xi;
        if (iy < H && ix < W) dx[(((size_t)b * 3 + c) * H + iy) * W + ix] = wst[e];
      }
    }
  }
}

template <int R, int NKC>
int launch_s2(const bf16* dz, const bf16* y, const float* pa, const float* pb, const float* pc, const float* w, float* dx, int ldz,
              int ldy, int wc, int B, int H, int W, int Ho, int Wo, int C0, int k, int pad, int dmin, hipStream_t st) {
  using L = SdLayout<R, NKC>;
  const dim3 grid((((W + 1) >> 1) + SD_CW - 1) / SD_CW, (((H + 1) >> 1) + SD_CH - 1) / SD_CH, B);
  static const bool attr = hipFuncSetAttribute(reinterpret_cast<const void*>(&stem_dgrad_s2_kernel<R, NKC>),
                                                hipFuncAttributeMaxDynamicSharedMemorySize, L::BYTES) == hipSuccess;
  if (!attr) return CX_EUNSUPPORTED;
  CX_KTAG("stem_dgrad_s2_kernel<%d, %d>", R, NKC);
  hipLaunchKernelGGL((stem_dgrad_s2_kernel<R, NKC>), grid, dim3(256), L::BYTES, st, dz, y, pa, pb, pc, w, dx, ldz, ldy, wc, H, W, Ho,
                     Wo, C0, k, pad, dmin);
  return launch_status();
}

// ------------------------------------------------------------------------------------------------ generic VALU form
constexpr int SG_CMAX = 128;

template <typename T>
__device__ __forceinline__ float sg_ld(const T* p) { return (float)*p; }

template <typename T>
__global__ __launch_bounds__(256) void stem_dgrad_generic_kernel(const T* __restrict__ dz, const T* __restrict__ y,
                                                                 const float* __restrict__ pa, const float* __restrict__ pb,
                                                                 const float* __restrict__ pc, const float* __restrict__ w,
                                                                 float* __restrict__ dx, const int ldz, const int ldy, const int wc,
                                                                 const int B, const int H, const int W, const int Ho, const int Wo,
                                                                 const int C0, const int k, const int stride, const int pad) {
  constexpr bool RND = sizeof(T) == 2;       // bf16 storage: g and W rounded to bf16
  extern __shared__ __attribute__((aligned(16))) char smem[];
  float* wl = reinterpret_cast<float*>(smem);                    // [ky][kx][c][o]
  float* co = wl + k * k * 3 * C0;                              // pa, pb, pc
  for (int e = threadIdx.x; e < k * k * 3 * C0; e += 256) {
    const int o = e % C0, c = (e / C0) % 3, tap = e / (3 * C0);
    const float v = w[((size_t)(o * wc + c) * k) * k + tap];
    wl[e] = RND ? bf2f(f2bf(v)) : v;
  }
  for (int e = threadIdx.x; e < C0; e += 256) {
    co[e] = pa[e];
    co[C0 + e] = pb[e];
    co[2 * C0 + e] = pc[e];
  }
  __syncthreads();
  const size_t pix = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (pix >= (size_t)B * H * W) return;
  const int ix = (int)(pix % W), iy = (int)((pix / W) % H), b = (int)(pix / ((size_t)W * H));
  float a0 = 0.f, a1 = 0.f, a2 = 0.f;
  for (int ky = 0; ky < k; ++ky) {
    const int ty = iy + pad - ky;
    if (ty < 0 || ty % stride) continue;
    const int oy = ty / stride;
    if (oy >= Ho) continue;
    for (int kx = 0; kx < k; ++kx) {
      const int tx = ix + pad - kx;
      if (tx < 0 || tx % stride) continue;
      const int ox = tx / stride;
      if (ox >= Wo) continue;
      const size_t op = ((size_t)b * Ho + oy) * Wo + ox;
      const T* zp = dz + op * ldz;
      const T* yp = y + op * ldy;
      const float* wt = wl + (ky * k + kx) * 3 * C0;
      for (int o = 0; o < C0; ++o) {
        float g = fmaf(sg_ld(zp + o), co[o], fmaf(sg_ld(yp + o), co[C0 + o], co[2 * C0 + o]));
        if (RND) g = bf2f(f2bf(g));
        a0 = fmaf(wt[o], g, a0);
        a1 = fmaf(wt[C0 + o], g, a1);
        a2 = fmaf(wt[2 * C0 + o], g, a2);
      }
    }
  }
  const size_t plane = (size_t)H * W, base = (size_t)b * 3 * plane + (size_t)iy * W + ix;
  dx[base] = a0;
  dx[base + plane] = a1;
  dx[base + 2 * plane] = a2;
}

template <typename T>
int launch_generic(const void* dz, const void* y, const float* pa, const float* pb, const float* pc, const float* w, float* dx, int ldz,
                   int ldy, int wc, int B, int H, int W, int Ho, int Wo, int C0, int k, int stride, int pad, hipStream_t st) {
  const size_t n = (size_t)B * H * W;
  const size_t smem = ((size_t)k * k * 3 * C0 + 3 * C0) * sizeof(float);
  static const bool attr = hipFuncSetAttribute(reinterpret_cast<const void*>(&stem_dgrad_generic_kernel<T>),
                                                hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024) == hipSuccess;
  if (!attr) return CX_EUNSUPPORTED;
  CX_KTAG("stem_dgrad_generic_kernel<%s>", sizeof(T) == 2 ? "bf16" : "float");
  hipLaunchKernelGGL((stem_dgrad_generic_kernel<T>), dim3((unsigned)((n + 255) / 256)), dim3(256), smem, st,
                     reinterpret_cast<const T*>(dz), reinterpret_cast<const T*>(y), pa, pb, pc, w, dx, ldz, ldy, wc, B, H, W, Ho, Wo, C0,
                     k, stride, pad);
  return launch_status();
}

}  // namespace

extern "C" int cx_stem_input_grad(const void* dz, const void* y, const float* pa, const float* pb, const float* pc, const float* w,
                                  float* dx, int ldz, int ldy, int wc, int B, int H, int W, int Ho, int Wo, int C0, int k, int stride,
                                  int pad, int dtype, void* stream) {
  if (!dz || !y || !pa || !pb || !pc || !w || !dx) return CX_EINVAL;
  if (B <= 0 || H <= 0 || W <= 0 || Ho <= 0 || Wo <= 0 || C0 <= 0 || wc < 3 || ldz < C0 || ldy < C0) return CX_EINVAL;
  if (dtype != 0 && dtype != 1) return CX_EUNSUPPORTED;
  // the stem geometries of the three engines: 7x7 s2 p3 (ImageNet DenseNet / ResNet), 3x3 s2 p0 | p1 (EfficientNet same_pad),
  // 3x3 s1 p1 (WideResNet / BasicBlock CIFAR stem), 5x5 s1 p2 (CIFAR DenseNet-BC)
  const bool s2 = stride == 2 && ((k == 7 && pad == 3) || (k == 3 && (pad == 0 || pad == 1)));
  const bool s1 = stride == 1 && ((k == 3 && pad == 1) || (k == 5 && pad == 2));
  if (!s2 && !s1) return CX_EUNSUPPORTED;
  if ((H + 2 * pad - k) / stride + 1 != Ho || (W + 2 * pad - k) / stride + 1 != Wo) return CX_ESHAPE;
  hipStream_t st = as_stream(stream);
  if (dtype == 0 && s2) {
    if (C0 > 64 || C0 % 8) return CX_EUNSUPPORTED;
    if (ldz % 8 || ldy % 8 || !aligned16(dz) || !aligned16(y)) return CX_EALIGN;
    const bf16* z = reinterpret_cast<const bf16*>(dz);
    const bf16* yy = reinterpret_cast<const bf16*>(y);
    if (k == 7)
      return C0 <= 32 ? launch_s2<4, 1>(z, yy, pa, pb, pc, w, dx, ldz, ldy, wc, B, H, W, Ho, Wo, C0, k, pad, -1, st)
                      : launch_s2<4, 2>(z, yy, pa, pb, pc, w, dx, ldz, ldy, wc, B, H, W, Ho, Wo, C0, k, pad, -1, st);
    const int dmin = pad == 1 ? 0 : -1;      // window start: 3x3 pad 1 -> rows cy, cy+1; pad 0 -> cy-1, cy
    return C0 <= 32 ? launch_s2<2, 1>(z, yy, pa, pb, pc, w, dx, ldz, ldy, wc, B, H, W, Ho, Wo, C0, k, pad, dmin, st)
                    : launch_s2<2, 2>(z, yy, pa, pb, pc, w, dx, ldz, ldy, wc, B, H, W, Ho, Wo, C0, k, pad, dmin, st);
  }
  if (C0 > SG_CMAX) return CX_EUNSUPPORTED;
  return dtype == 0 ? launch_generic<bf16>(dz, y, pa, pb, pc, w, dx, ldz, ldy, wc, B, H, W, Ho, Wo, C0, k, stride, pad, st)
                    : launch_generic<float>(dz, y, pa, pb, pc, w, dx, ldz, ldy, wc, B, H, W, Ho, Wo, C0, k, stride, pad, st);
}
