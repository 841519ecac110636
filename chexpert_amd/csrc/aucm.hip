// AUC min-max-margin loss (Yuan et al., "Large-scale Robust Deep AUC Maximization", ICCV 2021) on the (B, n) logits of a training
// step, with the gradients of the logits and of the three auxiliary scalars per class (include/chexpert_hip.h, cx_aucm_fwd_bwd),
// and the primal-descent / dual-ascent update of those scalars (cx_aucm_aux_step).
//
// One workgroup, like the BCE kernels it stands beside: the operand is B x n floats (256 x 14 at the largest), so the launch is
// latency, not throughput, and one workgroup keeps every sum in a fixed order without a second launch or an atomic.
// Thread (r, c) = (tid / CW, tid % CW), CW the power of two that covers min(n, 256): column c is a class, the 256 / CW threads of a
// column stride over the rows.  The work is five sums per class -- (y-a)^2 and (y-a) over the positives, (y-b)^2 and (y-b) over the
// negatives, and p y N - (1-p) y P over both -- plus the count of live rows.  They run in double, for the reason the weighted BCE
// gives: 1e3 terms of order 1 added in fp32 round at 1e-4, which is the whole loss tolerance.  Each column is folded by a fixed
// tree over r through LDS; the thread r = 0 then holds the class's totals, writes its loss term and auxiliary gradients and leaves
// the row count in LDS for the second pass, in which the same threads write d loss / d logits (it needs L, so it cannot be fused
// into the first).  Classes beyond CW (n > 256) are taken in further sweeps of the same code.  The class terms are added to the
// loss by thread 0 in class order.  No atomics anywhere: two runs give the same bits.
#include "common.h"

namespace {

constexpr int NT = 256;       // workgroup width
constexpr int NSUM = 5;       // double sums per class

__device__ __forceinline__ void aucm_sigmoid(const float x, float& y, float& omy) {
  y = 1.f / (1.f + expf(-x));
  omy = 1.f / (1.f + expf(x));        // 1 - y = sigmoid(-x), without the cancellation
}

__global__ __launch_bounds__(NT) void aucm_kernel(const float* __restrict__ logits, const float* __restrict__ target,
                                                  const float* __restrict__ prior, const float* __restrict__ aux, float margin,
                                                  float* loss, float* loss_class, float* dlogits, float* daux, float grad_scale, int B,
                                                  int n, int CW) {
  __shared__ double red[NSUM][NT];
  __shared__ int cnt[NT];
  __shared__ double cls[NT];           // loss terms of this sweep's classes
  const int tid = threadIdx.x, c = tid % CW, r = tid / CW, R = NT / CW;
  double total = 0.0;                  // thread 0: the loss so far
  for (int c0 = 0; c0 < n; c0 += CW) {
    const int k = c0 + c;
    const bool on = k < n;
    double p = 0.5, a = 0.0, b = 0.0, al = 0.0;
    if (on) { p = prior[k]; a = aux[k]; b = aux[n + k]; al = aux[2 * n + k]; }
    double s[NSUM] = {0.0, 0.0, 0.0, 0.0, 0.0};
    int live = 0;
    if (on) {
      for (int i = r; i < B; i += R) {
        const float t = target[(size_t)i * n + k];
        if (t >= 0.f) {
          float yf, omy;
          aucm_sigmoid(logits[(size_t)i * n + k], yf, omy);
          const double y = yf;
          ++live;
          if (t >= 0.5f) {
            const double d = y - a;
            s[0] += d * d;
            s[1] += d;
            s[4] -= (1.0 - p) * y;
          } else {
            const double d = y - b;
            s[2] += d * d;
            s[3] += d;
            s[4] += p * y;
          }
        }
      }
    }
#pragma unroll
    for (int j = 0; j < NSUM; ++j) red[j][tid] = s[j];
    cnt[tid] = live;
    __syncthreads();
    for (int h = R / 2; h > 0; h >>= 1) {
      if (r < h) {
#pragma unroll
        for (int j = 0; j < NSUM; ++j) red[j][tid] += red[j][tid + h * CW];
        cnt[tid] += cnt[tid + h * CW];
      }
      __syncthreads();
    }
    if (r == 0) {
      double lc = 0.0;
      if (on) {
        const int nl = cnt[c];
        double da = 0.0, db = 0.0, dal = 0.0;
        if (nl > 0) {                  // a class without a live row adds nothing and moves nothing
          const double L = nl, q = p * (1.0 - p), inner = q * margin + red[4][c] / L;
          lc = ((1.0 - p) * red[0][c] + p * red[2][c]) / L + 2.0 * al * inner - q * al * al;
          da = -(1.0 - p) * 2.0 * red[1][c] / L;
          db = -p * 2.0 * red[3][c] / L;
          dal = 2.0 * inner - 2.0 * q * al;
        }
        if (loss_class) loss_class[k] = (float)lc;
        if (daux) { daux[k] = (float)da; daux[n + k] = (float)db; daux[2 * n + k] = (float)dal; }
      }
      cls[c] = lc;
    }
    __syncthreads();
    if (tid == 0)
      for (int j = 0; j < CW && c0 + j < n; ++j) total += cls[j];
    if (dlogits && on) {
      const int nl = cnt[c];
      const float invL = nl > 0 ? 1.f / (float)nl : 0.f;
      const float pf = (float)p, af = (float)a, bf = (float)b, alf = (float)al;
      for (int i = r; i < B; i += R) {
        const float t = target[(size_t)i * n + k];
        float d = 0.f;
        if (t >= 0.f) {
          float y, omy;
          aucm_sigmoid(logits[(size_t)i * n + k], y, omy);
          const float g = t >= 0.5f ? (1.f - pf) * (2.f * (y - af) - 2.f * alf) : pf * (2.f * (y - bf) + 2.f * alf);
          d = y * omy * invL * g * grad_scale;
        }
        dlogits[(size_t)i * n + k] = d;
      }
    }
    __syncthreads();                   // red / cnt / cls are rewritten by the next sweep
  }
  if (tid == 0 && loss) *loss = (float)total;
}

__global__ void aucm_aux_step_kernel(float* __restrict__ aux, const float* __restrict__ daux, const float* __restrict__ lr_aux, int n) {
  const int k = blockIdx.x * blockDim.x + threadIdx.x;
  if (k >= n) return;
  const float lr = *lr_aux;
  aux[k] = aux[k] - lr * daux[k];
  aux[n + k] = aux[n + k] - lr * daux[n + k];
  aux[2 * n + k] = fmaxf(aux[2 * n + k] + lr * daux[2 * n + k], 0.f);
}

}  // namespace

int cx_aucm_fwd_bwd(const float* logits, const float* target, const float* prior, const float* aux, float margin, float* loss,
                    float* loss_class, float* dlogits, float* daux, float grad_scale, int B, int n_classes, void* stream) {
  if (!logits || !target || !prior || !aux || B < 1 || n_classes < 1 || !(margin > 0.f)) return CX_EINVAL;
  int CW = 1;
  while (CW < n_classes && CW < NT) CW <<= 1;
  hipLaunchKernelGGL(aucm_kernel, dim3(1), dim3(NT), 0, as_stream(stream), logits, target, prior, aux, margin, loss, loss_class, dlogits,
                     daux, grad_scale, B, n_classes, CW);
  return launch_status();
}

int cx_aucm_aux_step(float* aux, const float* daux, const float* lr_aux_dev, int n_classes, void* stream) {
  if (!aux || !daux || !lr_aux_dev || n_classes < 1) return CX_EINVAL;
  hipLaunchKernelGGL(aucm_aux_step_kernel, dim3((n_classes + NT - 1) / NT), dim3(NT), 0, as_stream(stream), aux, daux, lr_aux_dev,
                     n_classes);
  return launch_status();
}
