// Class activation maps of the final feature map, all requested classes in one pass (include/chexpert_hip.h, cx_class_cam):
//   cam[b][k][p] = post((1/HW) * sum_f w[cls(b,k)][f] * act(x[b][p][f] * scale[f] + shift[f]))
// The feature map is the only operand of any size and is read once whatever K is: one wave per pixel loads the pixel's channels
// (16 B of bf16 per lane and sweep of 512 channels, every sweep requested before the first is consumed), applies the affine and the
// activation once and keeps the result in registers (C <= 4096: at most 64 values per lane).  The classes are then looped over
// against rows of w, four rows in flight per step.  w (n_classes x C fp32: 20-56 KB for the CheXpert heads) is shared by every pixel
// and read with 32 contiguous bytes per lane; it stays in L2 (4 MiB per XCD) and mostly in the 32 KiB L1 of the CU, whose four
// waves walk the same rows at the same time.  Staging it in LDS would save nothing (each wave needs every row once per pixel either
// way) and would tie K * C to the LDS size.
// Sums are fp32 in a fixed order -- per lane the channels in ascending order, then the xor-shuffle tree -- and every output element
// has one writer: two calls give the same bits, and a class gives the same bits wherever it stands in the class table.
#include "common.h"

namespace {

constexpr int KU = 4;      // class rows in flight per step of the class loop

// accurate forms (expf and an IEEE division, <= 2^-22 relative): the maps are checked against float64 term by term
__device__ __forceinline__ float cam_act(const float z, const int act) {
  return act == CX_CAM_ACT_SWISH ? z / (1.f + expf(-z)) : (act == CX_CAM_ACT_RELU ? fmaxf(z, 0.f) : z);
}

template <typename T, int NS>
__global__ __launch_bounds__(256) void class_cam_kernel(const T* __restrict__ x, const float* __restrict__ sc, const float* __restrict__ sh,
                                                        const float* __restrict__ w, const int* __restrict__ cls, float* __restrict__ cam,
                                                        size_t npix, int HW, int C, int ldx, int n_classes, int ldw, int K, int act,
                                                        int relu, float inv_hw) {
  const int lane = threadIdx.x & 63;
  const size_t pix = (size_t)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (pix >= npix) return;                                  // the same for all lanes of a wave
  typename V8<T>::raw v[NS];
#pragma unroll
  for (int s = 0; s < NS; ++s) {
    const int c = s * 512 + lane * 8;
    v[s] = V8<T>::ld(x + pix * ldx + (c < C ? c : 0));      // lanes past C re-read chunk 0 (in bounds) and drop it below
  }
  float a[NS][8];
#pragma unroll
  for (int s = 0; s < NS; ++s) {
    const int c = s * 512 + lane * 8;
    const bool in = c < C;
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      float z = V8<T>::get(v[s], j);
      if (sc) z = fmaf(z, sc[in ? c + j : 0], sh[in ? c + j : 0]);
      a[s][j] = in ? cam_act(z, act) : 0.f;
    }
  }
  const size_t b = pix / HW;
  const int p = (int)(pix - b * HW);
  for (int k0 = 0; k0 < K; k0 += KU) {
    const float* wr[KU];
    float acc[KU];
#pragma unroll
    for (int u = 0; u < KU; ++u) {
      const int k = min(k0 + u, K - 1);                     // past the end: class K-1 again, not stored
      int row = k;
      if (cls) row = min(max(cls[b * K + k], 0), n_classes - 1);      // device-side indices are clamped, never trusted
      wr[u] = w + (size_t)row * ldw;
      acc[u] = 0.f;
    }
#pragma unroll
    for (int s = 0; s < NS; ++s) {
      const int c = s * 512 + lane * 8;
      if (c < C) {
#pragma unroll
        for (int u = 0; u < KU; ++u) {
          const f32x4 w0 = *reinterpret_cast<const f32x4*>(wr[u] + c);
          const f32x4 w1 = *reinterpret_cast<const f32x4*>(wr[u] + c + 4);
#pragma unroll
          for (int j = 0; j < 4; ++j) acc[u] = fmaf(w0[j], a[s][j], acc[u]);
#pragma unroll
          for (int j = 0; j < 4; ++j) acc[u] = fmaf(w1[j], a[s][4 + j], acc[u]);
        }
      }
    }
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) {
#pragma unroll
      for (int u = 0; u < KU; ++u) acc[u] += __shfl_xor(acc[u], d);
    }
    if (lane == 0) {
#pragma unroll
      for (int u = 0; u < KU; ++u) {
        if (k0 + u < K) {
          const float t = acc[u] * inv_hw;
          cam[(b * K + (k0 + u)) * HW + p] = relu ? fmaxf(t, 0.f) : t;
        }
      }
    }
  }
}

template <typename T>
int class_cam_launch(const void* x, const float* scale, const float* shift, const float* w, const int* cls, float* cam, int B, int HW,
                     int C, int ldx, int n_classes, int ldw, int K, int act, int relu, void* stream) {
  if (!x || !w || !cam || B < 1 || HW < 1 || K < 1 || n_classes < 1 || C < 8 || C % 8 || C > 4096 || ldx % 8 || ldx < C || ldw % 4 ||
      ldw < C || (!cls && K != n_classes))
    return CX_ESHAPE;
  if ((scale == nullptr) != (shift == nullptr) || act < CX_CAM_ACT_NONE || act > CX_CAM_ACT_SWISH) return CX_EINVAL;
  if (!aligned16(x) || !aligned16(w)) return CX_EALIGN;
  const size_t npix = (size_t)B * HW;
  if ((npix + 3) / 4 > 0x7fffffffull) return CX_ESHAPE;
  const dim3 grid((unsigned)((npix + 3) / 4)), block(256);
  const float inv_hw = 1.f / (float)HW;
#define CX_CAM_CASE(NS)                                                                                                              \
  if (C <= NS * 512) {                                                                                                               \
    hipLaunchKernelGGL((class_cam_kernel<T, NS>), grid, block, 0, as_stream(stream), (const T*)x, scale, shift, w, cls, cam, npix, HW, \
                       C, ldx, n_classes, ldw, K, act, relu, inv_hw);                                                                \
    return launch_status();                                                                                                          \
  }
  CX_CAM_CASE(1)
  CX_CAM_CASE(2)
  CX_CAM_CASE(4)
  CX_CAM_CASE(8)
#undef CX_CAM_CASE
  return CX_ESHAPE;
}

}  // namespace

int cx_class_cam(const void* x, const float* scale, const float* shift, const float* w, const int* cls, float* cam, int B, int HW, int C,
                 int ldx, int n_classes, int ldw, int K, int act, int relu, void* stream) {
  return class_cam_launch<bf16>(x, scale, shift, w, cls, cam, B, HW, C, ldx, n_classes, ldw, K, act, relu, stream);
}

int cx_class_cam_f32(const void* x, const float* scale, const float* shift, const float* w, const int* cls, float* cam, int B, int HW,
                     int C, int ldx, int n_classes, int ldw, int K, int act, int relu, void* stream) {
  return class_cam_launch<float>(x, scale, shift, w, cls, cam, B, HW, C, ldx, n_classes, ldw, K, act, relu, stream);
}
