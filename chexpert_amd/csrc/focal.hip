// Focal loss (Lin et al., ICCV 2017) and asymmetric loss (Ridnik et al., "Asymmetric Loss for Multi-Label Classification", ICCV 2021)
// on the (B, n) logits of a training step, with d loss / d logits, in one launch (include/chexpert_hip.h, cx_asl_fwd_bwd).  One
// kernel serves both: the focal loss is the asymmetric one with equal exponents and no clip.
//
// The shape is bce_masked_kernel's (elementwise.hip): one workgroup, a grid-stride loop over the B x n elements, a fixed tree over
// LDS, no atomics, every output optional.  The sum runs in double, for the reason the weighted BCE gives.  The four
// hyper-parameters are READ FROM MEMORY (focus[4] = gamma+, gamma-, clip, alpha or a negative number for "no alpha"), so a captured
// step sees a change made in place.
//
// Numerics.  With e = log1p(exp(-|x|)):  softplus(x) = max(x, 0) + e = -log q  and  softplus(-x) = max(-x, 0) + e = -log p, so
// neither logarithm is taken of a rounded probability; q = 1 / (1 + exp(x)) is never 1 - p.  The focusing weight u^g is
// exp(g log u), and log u is one of those softplus values wherever u is p or q themselves (hard targets without a clip, hard
// positives always): q^g of a confident positive is exp(-g softplus(x)), to a relative error of g |ln q| 2^-24.  With a clip m > 0 the
// shifted negative probability p_n = min(q + m, 1) is at least m; its logarithm is log1p(-(p - m)) while p - m < 1/2 (p - m is
// exact near the clip, so the loss keeps its relative accuracy as it goes to 0 there) and log(q + m) beyond.
//
// The clip is stated piecewise.  A hard negative at or below it (u = 0) gives loss 0 and gradient 0 exactly; the product
// g u^(g-1) u' is never formed (it is inf * 0 there for g < 1).  Above the clip u > 0 and g u^(g-1) u' = g f u' / u is finite.
#include "common.h"

#include <climits>

namespace {

constexpr int NT = 256;       // workgroup width

__global__ __launch_bounds__(NT) void asl_kernel(const float* __restrict__ logits, const float* __restrict__ target,
                                                 const float* __restrict__ pos_weight, const float* __restrict__ focus, float* loss,
                                                 float* loss_elem, float* dlogits, float grad_scale, int B, int n) {
  __shared__ double red[NT];
  const float gp = focus[0], gn = focus[1], m = focus[2], alpha = focus[3];
  const float invB = 1.f / B;
  double acc = 0.0;
  for (int i = threadIdx.x; i < B * n; i += NT) {
    const float x = logits[i], t = target[i];
    float l = 0.f, d = 0.f;
    if (t >= 0.f) {
      const float w = pos_weight ? pos_weight[i % n] : 1.f;
      const float e = log1pf(expf(-fabsf(x)));
      const float sp = fmaxf(x, 0.f) + e, sn = fmaxf(-x, 0.f) + e;      // -log q, -log p
      const float p = 1.f / (1.f + expf(-x)), q = 1.f / (1.f + expf(x));
      const float omt = 1.f - t;
      const bool above = p > m;                                          // p_m = p - m there, 0 (and constant) elsewhere
      const float pm = above ? p - m : 0.f;
      float lpn, dneg;                                                   // log p_n;  d(-log p_n)/dx = p q / p_n above the clip
      if (m == 0.f) {
        lpn = -sp;
        dneg = p;
      } else if (above) {
        lpn = pm < 0.5f ? log1pf(-pm) : logf(q + m);
        dneg = p * q / fminf(q + m, 1.f);
      } else {
        lpn = 0.f;
        dneg = 0.f;
      }
      const float C = w * t * sn - omt * lpn;
      const float dC = omt * dneg - w * t * q;
      const float u = t * q + omt * pm;                                  // 1 - p_t;  u' = p q ((1 - t) [p > m] - t)
      const float g = gp * t + gn * omt;
      float f = 1.f, df = 0.f;
      if (g != 0.f) {
        if (u > 0.f) {
          float lu, ratio;                                               // log u, u' / u
          if (t == 1.f) {
            lu = -sp;
            ratio = -p;
          } else if (t == 0.f && m == 0.f) {
            lu = -sn;
            ratio = q;
          } else {
            lu = logf(u);
            ratio = p * q * ((above ? omt : 0.f) - t) / u;
          }
          f = expf(g * lu);
          df = g * f * ratio;
        } else {
          f = 0.f;                                                       // 0^g, g > 0: the hard threshold; its derivative is taken as 0
        }
      }
      const float a = alpha < 0.f ? 1.f : alpha * t + (1.f - alpha) * omt;
      l = a * f * C;
      d = a * (df * C + f * dC) * invB * grad_scale;
    }
    acc += l;
    if (loss_elem) loss_elem[i] = l;
    if (dlogits) dlogits[i] = d;
  }
  red[threadIdx.x] = acc;
  __syncthreads();
  for (int s = NT / 2; s > 0; s >>= 1) {
    if (threadIdx.x < s) red[threadIdx.x] += red[threadIdx.x + s];
    __syncthreads();
  }
  if (threadIdx.x == 0 && loss) *loss = (float)(red[0] / B);
}

}  // namespace

int cx_asl_fwd_bwd(const float* logits, const float* target, const float* pos_weight, const float* focus, float* loss, float* loss_elem,
                   float* dlogits, float grad_scale, int B, int n_classes, void* stream) {
  if (!logits || !target || !focus || B < 1 || n_classes < 1 || (long long)B * n_classes > INT_MAX - NT) return CX_EINVAL;
  hipLaunchKernelGGL(asl_kernel, dim3(1), dim3(NT), 0, as_stream(stream), logits, target, pos_weight, focus, loss, loss_elem, dlogits,
                     grad_scale, B, n_classes);
  return launch_status();
}
