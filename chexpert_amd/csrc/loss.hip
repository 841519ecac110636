// The training losses on the (B, n) logits of a step, each with d loss / d logits in one launch of ONE workgroup: the operand is
// B x n floats (256 x 14 at the largest), so the launch is latency, not throughput, and one workgroup keeps every sum in a fixed
// order without a second launch or an atomic.  Three families:
//
//   cx_bce_fwd_bwd, cx_bce_masked_fwd_bwd, cx_asl_fwd_bwd   sums over elements: one skeleton (elem_loss_kernel) over a per-element
//                                                           term, four terms (plain, masked and weighted BCE, focal / asymmetric)
//   cx_mc3_fwd_bwd, cx_mc3_collapse                         the same sum over elements of THREE logits each (U-MultiClass), in the
//                                                           skeleton's sibling mc3_loss_kernel; the collapse to binary logits
//   cx_hier_fwd_bwd, cx_hier_collapse                       the findings as a forest: the masked BCE under positive ancestors, or the
//                                                           cross-entropy of the product of sigmoids along a path; the collapse
//   cx_softmax_ce_fwd_bwd                                   one wave per sample, its own final sum
//   cx_aucm_fwd_bwd, cx_aucm_aux_step                       a function of each class's whole batch column: column trees, two passes
//   cx_ntxent_fwd_bwd                                       the contrastive loss on (N, d) embeddings, which couples the rows: the one
//                                                           exception to the single workgroup, three launches of a workgroup per row
#include "common.h"

#include <climits>

namespace {

constexpr int NT = 256;       // workgroup width

// sigmoid(x) and 1 - sigmoid(x) = sigmoid(-x), the second without the cancellation
__device__ __forceinline__ void sigmoid_pair(const float x, float& p, float& q) {
  p = 1.f / (1.f + expf(-x));
  q = 1.f / (1.f + expf(x));
}

// ---- the element-wise terms -----------------------------------------------------------------------------------------------------
// A term holds what a launch fixes (the per-class weights, the focus numbers, read from memory once per thread), names the type its
// sum runs in (Acc) and states the arithmetic of one element: (x, t, class index k) -> the loss l and d = d loss / d x, the latter
// already times invB * grad_scale.  mean() is the final divide of the folded sum.  The expressions of a term are its own: two terms
// that look alike do not share a rounded sub-expression.

// BCEWithLogitsLoss summed over the classes and averaged over the batch.  A negative target is a number like any other.
struct BceTerm {
  using Acc = float;
  __device__ BceTerm(const float*, const float*) {}
  __device__ __forceinline__ void operator()(float x, float t, int k, float invB, float grad_scale, float& l, float& d) const {
    l = fmaxf(x, 0.f) - x * t + log1pf(expf(-fabsf(x)));
    d = (1.f / (1.f + expf(-x)) - t) * invB * grad_scale;
  }
  __device__ static float mean(float sum, int B, float invB) { return sum * invB; }
};

// BceTerm with ignored elements (target < 0: no loss, no gradient; the divisor stays B) and, in WeightedBceTerm, a per-class positive
// weight (torch's BCEWithLogitsLoss(pos_weight)).  One workgroup, fixed tree, no atomics.  Unweighted, a live element runs
// BceTerm's expressions and the sum its fp32 tree, so targets without negatives give cx_bce_fwd_bwd's bits.  Weighted, the sum runs
// in double: weights up to 16 on logits of +-8 take the batch sum of 256 x 14 elements past 1e4, where an fp32 add rounds to 5e-4.
struct MaskedBceTerm : BceTerm {
  using BceTerm::BceTerm;
  __device__ __forceinline__ void operator()(float x, float t, int k, float invB, float grad_scale, float& l, float& d) const {
    l = d = 0.f;
    if (t >= 0.f) BceTerm::operator()(x, t, k, invB, grad_scale, l, d);
  }
};

struct WeightedBceTerm {
  using Acc = double;
  const float* __restrict__ pos_weight;
  __device__ WeightedBceTerm(const float* pos_weight, const float*) : pos_weight(pos_weight) {}
  __device__ __forceinline__ void operator()(float x, float t, int k, float invB, float grad_scale, float& l, float& d) const {
    l = d = 0.f;
    if (t >= 0.f) {
      const float w = 1.f + (pos_weight[k] - 1.f) * t;
      l = (1.f - t) * x + w * (log1pf(expf(-fabsf(x))) + fmaxf(-x, 0.f));
      float p, q;
      sigmoid_pair(x, p, q);
      d = ((1.f - t) - w * q) * invB * grad_scale;
    }
  }
  __device__ static float mean(double sum, int B, float invB) { return (float)(sum / B); }
};

// Focal loss (Lin et al., ICCV 2017) and asymmetric loss (Ridnik et al., "Asymmetric Loss for Multi-Label Classification", ICCV 2021)
// on the (B, n) logits of a training step, with d loss / d logits, in one launch (include/chexpert_hip.h, cx_asl_fwd_bwd).  One
// term serves both: the focal loss is the asymmetric one with equal exponents and no clip.
//
// The shape is the masked BCE's (elem_loss_kernel): one workgroup, a grid-stride loop over the B x n elements, a fixed tree over
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
struct AslTerm {
  using Acc = double;
  const float* __restrict__ pos_weight;
  float gp, gn, m, alpha;
  __device__ AslTerm(const float* pos_weight, const float* focus)
      : pos_weight(pos_weight), gp(focus[0]), gn(focus[1]), m(focus[2]), alpha(focus[3]) {}
  __device__ __forceinline__ void operator()(float x, float t, int k, float invB, float grad_scale, float& l, float& d) const {
    l = d = 0.f;
    if (t >= 0.f) {
      const float w = pos_weight ? pos_weight[k] : 1.f;
      const float e = log1pf(expf(-fabsf(x)));
      const float sp = fmaxf(x, 0.f) + e, sn = fmaxf(-x, 0.f) + e;      // -log q, -log p
      float p, q;
      sigmoid_pair(x, p, q);
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
  }
  __device__ static float mean(double sum, int B, float invB) { return (float)(sum / B); }
};

// ---- the element-wise skeleton --------------------------------------------------------------------------------------------------
// One workgroup: thread t takes elements t, t + 256, ... of the B x n, adds their losses in Term::Acc, and the 256 sums are folded
// by a fixed tree over LDS.  loss (one float), loss_elem and dlogits (B x n) are each written when given.  The stride and the tree
// are stated on blockDim.x (256 at every launch), not on NT: with the constant the compiler unrolls the tree and packs the two
// products of the weighted BCE's loss into one v_pk_mul_f32 ahead of the contraction, which costs that loss its fused multiply-add
// (a last-bit change of loss and loss_elem on soft targets).
template <typename Term>
__global__ __launch_bounds__(NT) void elem_loss_kernel(const float* __restrict__ logits, const float* __restrict__ target,
                                                       const float* __restrict__ pos_weight, const float* __restrict__ focus,
                                                       float* loss, float* loss_elem, float* dlogits, float grad_scale, int B, int n) {
  using Acc = typename Term::Acc;
  __shared__ Acc red[NT];
  const Term term(pos_weight, focus);
  const float invB = 1.f / B;
  Acc acc = 0;
  for (int i = threadIdx.x; i < B * n; i += blockDim.x) {
    float l, d;
    term(logits[i], target[i], i % n, invB, grad_scale, l, d);
    acc += l;
    if (loss_elem) loss_elem[i] = l;
    if (dlogits) dlogits[i] = d;
  }
  red[threadIdx.x] = acc;
  __syncthreads();
  for (int s = blockDim.x / 2; s > 0; s >>= 1) {
    if (threadIdx.x < s) red[threadIdx.x] += red[threadIdx.x + s];
    __syncthreads();
  }
  if (threadIdx.x == 0 && loss) *loss = Term::mean(red[0], B, invB);
}

template <typename Term>
int launch_elem_loss(const float* logits, const float* target, const float* pos_weight, const float* focus, float* loss,
                     float* loss_elem, float* dlogits, float grad_scale, int B, int n, void* stream) {
  hipLaunchKernelGGL(elem_loss_kernel<Term>, dim3(1), dim3(NT), 0, as_stream(stream), logits, target, pos_weight, focus, loss, loss_elem,
                     dlogits, grad_scale, B, n);
  return launch_status();
}

// ---- three-way softmax over every finding (U-MultiClass) -----------------------------------------------------------------------
// The U-MultiClass policy of the data set's paper (Irvin et al., "CheXpert", AAAI 2019): every finding owns three logits -- negative,
// positive, uncertain -- and the loss is the softmax cross-entropy over them (include/chexpert_hip.h, cx_mc3_fwd_bwd).  Finding k of
// row b reads logits[b][3k .. 3k+2]; its class comes from the (B, n) target table the sigmoid losses read: 2 where t < 0, 1 where
// t >= 0.5 (the "positive" of aucm_kernel), else 0.  Nothing is ignored.
//
// Numerics.  m = max z, e_j = exp(z_j - m), s = (e0 + e1) + e2, and r = the sum of the two exponentials that are not the target's, in
// index order.  Where the target's logit is the maximum (e_c = 1, s = 1 + r) the loss is log1p(r), else (m - z_c) + log(s); the
// target's gradient is -r / s, never e_c / s - 1, and r is never s - e_c: a confident correct element (r ~ 1e-4) keeps every digit
// where m + log(s) - z_c keeps three.
__device__ __forceinline__ int mc3_class(const float t) { return t < 0.f ? 2 : (t >= 0.5f ? 1 : 0); }

__device__ __forceinline__ void mc3_softmax(const float z0, const float z1, const float z2, float& m, float& e0, float& e1, float& e2,
                                            float& s) {
  m = fmaxf(fmaxf(z0, z1), z2);
  e0 = expf(z0 - m);
  e1 = expf(z1 - m);
  e2 = expf(z2 - m);
  s = (e0 + e1) + e2;
}

// The sibling of elem_loss_kernel for an element of three logits: one workgroup, thread t takes triples t, t + 256, ... of the B x n,
// the sum in double (class weights take it where the weighted BCE's goes), the same fixed tree over LDS, stride and tree stated on
// blockDim.x.  class_weight: (n, 3) or null; the term and its three gradients are multiplied by w[k][c], with 1.f where there is no
// table, so a table of ones gives the bits of the call without one.
__global__ __launch_bounds__(NT) void mc3_loss_kernel(const float* __restrict__ logits, const float* __restrict__ target,
                                                      const float* __restrict__ class_weight, float* loss, float* loss_elem,
                                                      float* dlogits, float grad_scale, int B, int n) {
  __shared__ double red[NT];
  const float invB = 1.f / B;
  double acc = 0;
  for (int i = threadIdx.x; i < B * n; i += blockDim.x) {
    const size_t o = (size_t)i * 3;
    const float z0 = logits[o], z1 = logits[o + 1], z2 = logits[o + 2];
    const int c = mc3_class(target[i]);
    const float w = class_weight ? class_weight[(i % n) * 3 + c] : 1.f;
    float m, e0, e1, e2, s;
    mc3_softmax(z0, z1, z2, m, e0, e1, e2, s);
    const float zc = c == 0 ? z0 : (c == 1 ? z1 : z2);
    const float r = c == 0 ? e1 + e2 : (c == 1 ? e0 + e2 : e0 + e1);
    const float l = w * (zc == m ? log1pf(r) : (m - zc) + logf(s));
    acc += l;
    if (loss_elem) loss_elem[i] = l;
    if (dlogits) {
      dlogits[o] = w * ((c == 0 ? -r : e0) / s) * invB * grad_scale;
      dlogits[o + 1] = w * ((c == 1 ? -r : e1) / s) * invB * grad_scale;
      dlogits[o + 2] = w * ((c == 2 ? -r : e2) / s) * invB * grad_scale;
    }
  }
  red[threadIdx.x] = acc;
  __syncthreads();
  for (int h = blockDim.x / 2; h > 0; h >>= 1) {
    if (threadIdx.x < h) red[threadIdx.x] += red[threadIdx.x + h];
    __syncthreads();
  }
  if (threadIdx.x == 0 && loss) *loss = (float)(red[0] / B);
}

// What the three logits of a finding become at test time: z = z1 - z0, whose sigmoid is p1 / (p0 + p1), the softmax over the two
// classes that are left when "uncertain" is dropped, and p_unc = e2 / s.  One thread per (b, k), no reduction.
__global__ __launch_bounds__(NT) void mc3_collapse_kernel(const float* __restrict__ logits, float* __restrict__ z,
                                                          float* __restrict__ p_unc, long long total) {
  const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= total) return;
  const float z0 = logits[i * 3], z1 = logits[i * 3 + 1], z2 = logits[i * 3 + 2];
  z[i] = z1 - z0;
  if (p_unc) {
    float m, e0, e1, e2, s;
    mc3_softmax(z0, z1, z2, m, e0, e1, e2, s);
    p_unc[i] = e2 / s;
  }
}

// ---- hierarchical labels --------------------------------------------------------------------------------------------------------
// The findings as a forest (include/chexpert_hip.h, cx_hier_fwd_bwd): parent[k] is -1 for a root, else an index below k, and every
// logit is the logit of P(k | parent(k) positive).  Two losses over it (Chen et al., MIDL 2019): the conditional one (mode 0) is the
// masked BCE with one more reason to skip an element -- an ancestor whose target is not positive --, the unconditional one (mode 1)
// the cross-entropy of the product of the sigmoids along the path.  Both are sums over the B x n elements, so both keep the element
// skeleton: one workgroup, thread t takes elements t, t + 256, ..., the fixed tree over LDS, stride and tree stated on blockDim.x.
//
// A path is held as a 64-bit mask (n <= 64): bit j of anc[k] says that j is k or one of its ancestors.  Parents come before children,
// so the set bits in ascending order ARE the path, root first.  The masks are built once per workgroup, into LDS, by the one walk up
// the table there is (hier_stage_masks).  The table is device memory whose values the host entry cannot see, so that walk is safe by
// itself: an entry outside [-1, k) is read as a root and a path is cut after HPATH nodes.  No index leaves the row, whatever the
// table holds.
constexpr int HMAXN = CX_HIER_MAX_LABELS, HPATH = CX_HIER_MAX_PATH;
constexpr float LN2 = 0.693147180559945f;
typedef unsigned long long hmask;

// anc[k] for k < n; desc[j] (where given) = the k whose path holds j, j itself among them.  Ends in a barrier.
__device__ __forceinline__ void hier_stage_masks(const int* __restrict__ parent, hmask* anc, hmask* desc, const int n) {
  for (int k = threadIdx.x; k < n; k += blockDim.x) {
    hmask m = 0;
    int node = k;
#pragma unroll
    for (int s = 0; s < HPATH; ++s) {
      if (node >= 0) {
        m |= 1ull << node;
        const int p = parent[node];
        node = (p >= 0 && p < node) ? p : -1;
      }
    }
    anc[k] = m;
  }
  __syncthreads();
  if (desc) {
    for (int j = threadIdx.x; j < n; j += blockDim.x) {
      hmask m = 0;
      for (int k = j; k < n; ++k) m |= ((anc[k] >> j) & 1ull) << k;
      desc[j] = m;
    }
    __syncthreads();
  }
}

__device__ __forceinline__ int hier_pop(hmask& m) {       // the lowest set bit's index, which leaves the mask
  const int b = __ffsll((long long)m) - 1;
  m &= m - 1;
  return b;
}

// log sigmoid(z) and log sigmoid(-z) from one e, as AslTerm takes its two softplus values
__device__ __forceinline__ void log_sigmoid_pair(const float z, float& lp, float& lq) {
  const float e = log1pf(expf(-fabsf(z)));
  lp = -(fmaxf(-z, 0.f) + e);
  lq = -(fmaxf(z, 0.f) + e);
}

// u = log P and l1m = log(1 - P) of the product of sigmoids along the path `path` (a mask), root first; logs(node, lp, lq) gives a
// node's pair.  The a_j = (sum of the lp before j) + lq_j are formed twice, by the same additions, rather than kept.
template <typename Logs>
__device__ __forceinline__ void hier_log_probs(const hmask path, Logs logs, float& u, float& l1m) {
  float m = -INFINITY;
  u = 0.f;
  for (hmask rest = path; rest;) {
    float lp, lq;
    logs(hier_pop(rest), lp, lq);
    m = fmaxf(m, u + lq);
    u += lp;
  }
  if (u <= -LN2) {
    l1m = log1pf(-expf(u));
  } else {
    float sum = 0.f, pre = 0.f;
    for (hmask rest = path; rest;) {
      float lp, lq;
      logs(hier_pop(rest), lp, lq);
      sum += expf((pre + lq) - m);
      pre += lp;
    }
    l1m = m + logf(sum);
  }
}

// mode 0: Term is MaskedBceTerm or WeightedBceTerm, and the kernel is elem_loss_kernel but for the ancestors' targets
template <typename Term>
__global__ __launch_bounds__(NT) void hier_cond_kernel(const float* __restrict__ logits, const float* __restrict__ target,
                                                       const int* __restrict__ parent, const float* __restrict__ pos_weight, float* loss,
                                                       float* loss_elem, float* dlogits, float grad_scale, int B, int n) {
  using Acc = typename Term::Acc;
  __shared__ Acc red[NT];
  __shared__ hmask anc[HMAXN];
  hier_stage_masks(parent, anc, nullptr, n);
  const Term term(pos_weight, nullptr);
  const float invB = 1.f / B;
  Acc acc = 0;
  for (int i = threadIdx.x; i < B * n; i += blockDim.x) {
    const int k = i % n;
    bool live = true;
    for (hmask above = anc[k] & ~(1ull << k); above;) live = target[i - k + hier_pop(above)] >= 0.5f && live;
    float l = 0.f, d = 0.f;
    if (live) term(logits[i], target[i], k, invB, grad_scale, l, d);
    acc += l;
    if (loss_elem) loss_elem[i] = l;
    if (dlogits) dlogits[i] = d;
  }
  red[threadIdx.x] = acc;
  __syncthreads();
  for (int s = blockDim.x / 2; s > 0; s >>= 1) {
    if (threadIdx.x < s) red[threadIdx.x] += red[threadIdx.x + s];
    __syncthreads();
  }
  if (threadIdx.x == 0 && loss) *loss = Term::mean(red[0], B, invB);
}

// mode 1.  A term of element (b, k) reaches every logit on k's path, so the thread of element (b, j) gathers: it adds the terms of
// the live k of j's subtree (desc[j]) in ascending k, and k = j itself gives the element's loss.  What the gathering threads share
// goes through LDS, one round of 256 elements at a time: the window is the whole rows those elements lie in (at most 256 + 2n
// elements), and its logits, targets and lp / lq (phase A) and u / l1m (phase B) are each read or computed once, by whichever
// thread the window's stride gives them to; a row that two rounds share is computed in both, to the same bits.  The gather itself
// (phase C) reads LDS alone.  Nothing depends on which outputs were asked for.
constexpr int HWIN = NT + 2 * HMAXN;

__global__ __launch_bounds__(NT) void hier_uncond_kernel(const float* __restrict__ logits, const float* __restrict__ target,
                                                         const int* __restrict__ parent, const float* __restrict__ pos_weight, float* loss,
                                                         float* loss_elem, float* dlogits, float grad_scale, int B, int n) {
  __shared__ double red[NT];
  __shared__ hmask anc[HMAXN], desc[HMAXN];
  __shared__ float s_z[HWIN], s_t[HWIN], s_lp[HWIN], s_lq[HWIN], s_u[HWIN], s_l1m[HWIN], s_w[HMAXN];
  for (int k = threadIdx.x; k < n; k += blockDim.x) s_w[k] = pos_weight ? pos_weight[k] : 1.f;
  hier_stage_masks(parent, anc, desc, n);
  const float invB = 1.f / B;
  const int total = B * n;
  double acc = 0;
  for (int base = 0; base < total; base += blockDim.x) {
    const int last = min(base + (int)blockDim.x, total) - 1;        // this round's elements: base .. last
    const int w0 = base / n * n, wlen = (last / n + 1) * n - w0;    // its window: whole rows, wlen < blockDim.x + 2n
    for (int e = threadIdx.x; e < wlen; e += blockDim.x) {
      const float z = logits[w0 + e];
      s_z[e] = z;
      s_t[e] = target[w0 + e];
      log_sigmoid_pair(z, s_lp[e], s_lq[e]);
    }
    __syncthreads();
    for (int e = threadIdx.x; e < wlen; e += blockDim.x) {
      const int k = e % n, r = e - k;
      float u, l1m;
      hier_log_probs(anc[k], [&](int node, float& lp, float& lq) { lp = s_lp[r + node]; lq = s_lq[r + node]; }, u, l1m);
      s_u[e] = u;
      s_l1m[e] = l1m;
    }
    __syncthreads();
    const int i = base + threadIdx.x;
    if (i < total) {
      const int e = i - w0, j = e % n, r = e - j;
      const float lqj = s_lq[e], qj = 1.f / (1.f + expf(s_z[e]));
      float l = 0.f, g = 0.f;
      for (hmask sub = desc[j]; sub;) {
        const int k = hier_pop(sub);
        const float t = s_t[r + k];
        if (t >= 0.f) {
          const float u = s_u[r + k], l1m = s_l1m[r + k];
          const float w = s_w[k];
          const float omt = 1.f - t;
          if (k == j) l = -w * t * u - omt * l1m;
          g += omt * expf(u + lqj - l1m) - w * t * qj;
        }
      }
      acc += l;
      if (loss_elem) loss_elem[i] = l;
      if (dlogits) dlogits[i] = g * invB * grad_scale;
    }
    __syncthreads();                   // the window is rewritten by the next round
  }
  red[threadIdx.x] = acc;
  __syncthreads();
  for (int h = blockDim.x / 2; h > 0; h >>= 1) {
    if (threadIdx.x < h) red[threadIdx.x] += red[threadIdx.x + h];
    __syncthreads();
  }
  if (threadIdx.x == 0 && loss) *loss = (float)(red[0] / B);
}

// One thread per (b, k), no reduction; each workgroup stages the masks for itself.
__global__ __launch_bounds__(NT) void hier_collapse_kernel(const float* __restrict__ logits, const int* __restrict__ parent,
                                                           float* __restrict__ z, float* __restrict__ p, long long total, int n) {
  __shared__ hmask anc[HMAXN];
  hier_stage_masks(parent, anc, nullptr, n);
  const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= total) return;
  const int k = (int)(i % n);
  const float* row = logits + (i - k);
  float u, l1m;
  hier_log_probs(anc[k], [&](int node, float& lp, float& lq) { log_sigmoid_pair(row[node], lp, lq); }, u, l1m);
  z[i] = anc[k] == 1ull << k ? logits[i] : u - l1m;
  if (p) p[i] = expf(u);
}

// ---- softmax cross-entropy ------------------------------------------------------------------------------------------------------
// one wave per sample: row maximum and sum of exponentials by DPP-free shuffles, loss = mean_b (logsumexp - logit[target]);
// the per-sample terms are summed by ONE workgroup in sample order (bit-reproducible)
__global__ void softmax_ce_kernel(const float* __restrict__ logits, const long long* __restrict__ target, float* loss, float* loss_elem,
                                  float* dlogits, float grad_scale, int B, int n) {
  __shared__ float red[256];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, nw = blockDim.x >> 6;
  const float invB = 1.f / B;
  float acc = 0.f;                                       // lane 0 of each wave: its samples' losses
  for (int b = wave; b < B; b += nw) {
    const float* row = logits + (size_t)b * n;
    float m = -INFINITY;
    for (int i = lane; i < n; i += 64) m = fmaxf(m, row[i]);
    for (int o = 32; o > 0; o >>= 1) m = fmaxf(m, __shfl_xor(m, o));
    float se = 0.f;
    for (int i = lane; i < n; i += 64) se += expf(row[i] - m);
    for (int o = 32; o > 0; o >>= 1) se += __shfl_xor(se, o);
    const int t = (int)target[b];
    const float l = (t >= 0 && t < n) ? m + logf(se) - row[t] : 0.f;
    if (lane == 0) {
      acc += l;
      if (loss_elem) loss_elem[b] = l;
    }
    if (dlogits) {
      const float inv = 1.f / se;
      // a target outside [0, n) contributes no loss and no gradient (nn.CrossEntropyLoss raises on it; the host wrapper checks the
      // target tensor's type and placement, its values stay on the device)
      const float live = (t >= 0 && t < n) ? invB * grad_scale : 0.f;
      for (int i = lane; i < n; i += 64) dlogits[(size_t)b * n + i] = (expf(row[i] - m) * inv - (i == t ? 1.f : 0.f)) * live;
    }
  }
  red[threadIdx.x] = lane == 0 ? acc : 0.f;
  __syncthreads();
  if (threadIdx.x == 0 && loss) {
    float s = 0.f;
    for (int w = 0; w < nw; ++w) s += red[w * 64];
    *loss = s * invB;
  }
}

// ---- AUC margin -----------------------------------------------------------------------------------------------------------------
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
constexpr int NSUM = 5;       // double sums per class

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
          sigmoid_pair(logits[(size_t)i * n + k], yf, omy);
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
          sigmoid_pair(logits[(size_t)i * n + k], y, omy);
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

// ---- NT-Xent / SupCon -----------------------------------------------------------------------------------------------------------
// The contrastive loss over the (N, d) embeddings of a step (include/chexpert_hip.h, cx_ntxent_fwd_bwd): the one loss here that
// couples the ROWS of a batch.  Row i with id g_i >= 0 is in the batch (V); its positives P(i) are the other rows of V with its id,
// its candidates A(i) all other rows of V; l_i = lse_i - mean_{p in P(i)} s_ip over the rows with a positive (the anchors), with
// s_ij = z_i . z_j / tau and z = e / max(|e|, 1e-12).  N is a few hundred, so the N x N similarities are some ten MFLOP: fp32 on the
// VALU, and never stored -- three launches over the caller's scratch of N d + 4 N floats (z | norm | lse | 1/|P| | l):
//   ntx_norm_kernel   one wave per row: |e_i|, z_i (zeros for a row outside V, so that it cannot reach another row's sums)
//   ntx_row_kernel    one workgroup per row i: the row s_i. into LDS (one wave per j, d split over its lanes), then row maximum and
//                     top-1, sum of exponentials relative to the maximum, |P(i)| and the positives' sum; writes lse_i, 1/|P(i)|, l_i
//   ntx_grad_kernel   one workgroup per row i: the anchor count M and (workgroup 0) the loss = sum l / M in double; the coefficients
//                     c_j = dS_ij + dS_ji into LDS, dS_ij = [i anchor](exp(s_ij - lse_i) - [j in P(i)] / |P(i)|) and dS_ji the same
//                     from s_ij (s is symmetric, and ntx_wave_dot gives s_ij = s_ji bit for bit), lse_j and |P(j)|;
//                     dz_i = sum_j c_j z_j / (tau M) with consecutive threads on consecutive k; the step back through the normalisation
// Every sum has a fixed order (a lane's ascending k, a xor butterfly, trees over LDS, ascending j): no atomics, the same bits on every
// run, and no output depends on which others were asked for.  tau is read from memory: a captured step sees it rewritten in place.
constexpr int NTX_MAX_N = CX_NTXENT_MAX_N, NTX_MAX_D = CX_NTXENT_MAX_D, NTX_WAVES = NT / 64;
constexpr float NTX_EPS = 1e-12f;

// a . b by one wave: lane l adds k = l, l + 64, ... in ascending k, then a xor butterfly, after which every lane holds the sum.  The
// products and the additions commute, so the value is the same with a and b exchanged.
__device__ __forceinline__ float ntx_wave_dot(const float* a, const float* __restrict__ b, const int d, const int lane) {
  float acc = 0.f;
  for (int k = lane; k < d; k += 64) acc = fmaf(a[k], b[k], acc);
  for (int o = 32; o > 0; o >>= 1) acc += __shfl_xor(acc, o);
  return acc;
}

__global__ __launch_bounds__(NT) void ntx_norm_kernel(const float* __restrict__ e, const float* __restrict__ ids, float* __restrict__ z,
                                                      float* __restrict__ nrm, int N, int d) {
  const int lane = threadIdx.x & 63, row = blockIdx.x * NTX_WAVES + (threadIdx.x >> 6);
  if (row >= N) return;
  const float* er = e + (size_t)row * d;
  const float n = sqrtf(ntx_wave_dot(er, er, d, lane));
  const float den = fmaxf(n, NTX_EPS);
  const bool in = ids[row] >= 0.f;
  for (int k = lane; k < d; k += 64) z[(size_t)row * d + k] = in ? er[k] / den : 0.f;
  if (lane == 0) nrm[row] = n;
}

__global__ __launch_bounds__(NT) void ntx_row_kernel(const float* __restrict__ z, const float* __restrict__ ids,
                                                     const float* __restrict__ temperature, float* __restrict__ lse,
                                                     float* __restrict__ invp, float* __restrict__ ell, float* __restrict__ loss_elem,
                                                     int* __restrict__ top1, int N, int d) {
  __shared__ float zi[NTX_MAX_D], srow[NTX_MAX_N], red_a[NT], red_b[NT];
  __shared__ int red_i[NT];
  const int i = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const float gi = ids[i];
  bool live = gi >= 0.f;
  if (live) {                                     // (the branch is the workgroup's: gi is one value)
    for (int k = tid; k < d; k += NT) zi[k] = z[(size_t)i * d + k];
    __syncthreads();
    const float tau = *temperature;
    for (int j = wave; j < N; j += NTX_WAVES) {
      const float dot = ntx_wave_dot(zi, z + (size_t)j * d, d, lane);
      if (lane == 0) srow[j] = (j != i && ids[j] >= 0.f) ? dot / tau : -INFINITY;
    }
    __syncthreads();
    float best = -INFINITY;                       // the row maximum and where it stands first; INT_MAX: nowhere yet
    int bj = INT_MAX;
    for (int j = tid; j < N; j += NT) {
      const float s = srow[j];
      if (s > best) { best = s; bj = j; }
    }
    red_a[tid] = best;
    red_i[tid] = bj;
    __syncthreads();
    for (int h = NT / 2; h > 0; h >>= 1) {
      if (tid < h) {
        const float v = red_a[tid + h];
        const int q = red_i[tid + h];
        if (v > red_a[tid] || (v == red_a[tid] && q < red_i[tid])) { red_a[tid] = v; red_i[tid] = q; }
      }
      __syncthreads();
    }
    const float m = red_a[0];
    const int top = red_i[0];
    __syncthreads();
    live = top != INT_MAX;                        // A(i) is empty: the only row of V
    if (live) {
      float se = 0.f, ps = 0.f;
      int cnt = 0;
      for (int j = tid; j < N; j += NT) {
        const float s = srow[j];
        se += expf(s - m);                        // (a row outside A(i) stands at -inf: 0)
        if (j != i && ids[j] == gi) { ps += s - m; ++cnt; }
      }
      red_a[tid] = se;
      red_b[tid] = ps;
      red_i[tid] = cnt;
      __syncthreads();
      for (int h = NT / 2; h > 0; h >>= 1) {
        if (tid < h) { red_a[tid] += red_a[tid + h]; red_b[tid] += red_b[tid + h]; red_i[tid] += red_i[tid + h]; }
        __syncthreads();
      }
      if (tid == 0) {
        const float lg = logf(red_a[0]);
        const int P = red_i[0];
        const float l = P > 0 ? lg - red_b[0] / (float)P : 0.f;       // lse_i - mean s_ip, both relative to the maximum
        lse[i] = m + lg;
        invp[i] = P > 0 ? 1.f / (float)P : 0.f;
        ell[i] = l;
        if (loss_elem) loss_elem[i] = l;
        if (top1) top1[i] = top;
      }
    }
  }
  if (!live && tid == 0) {
    lse[i] = 0.f;
    invp[i] = 0.f;
    ell[i] = 0.f;
    if (loss_elem) loss_elem[i] = 0.f;
    if (top1) top1[i] = -1;
  }
}

__global__ __launch_bounds__(NT) void ntx_grad_kernel(const float* __restrict__ z, const float* __restrict__ nrm,
                                                      const float* __restrict__ ids, const float* __restrict__ temperature,
                                                      const float* __restrict__ lse, const float* __restrict__ invp,
                                                      const float* __restrict__ ell, float* __restrict__ loss,
                                                      float* __restrict__ dlogits, float grad_scale, int N, int d) {
  __shared__ float zi[NTX_MAX_D], dzs[NTX_MAX_D], crow[NTX_MAX_N], part[NT];
  __shared__ double red_d[NT];
  __shared__ int red_i[NT];
  const int i = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  int cnt = 0;                                    // the anchors: every workgroup counts them for itself
  double sum = 0.0;
  for (int j = tid; j < N; j += NT) {
    cnt += invp[j] > 0.f ? 1 : 0;
    sum += ell[j];
  }
  red_i[tid] = cnt;
  red_d[tid] = sum;
  __syncthreads();
  for (int h = NT / 2; h > 0; h >>= 1) {
    if (tid < h) { red_i[tid] += red_i[tid + h]; red_d[tid] += red_d[tid + h]; }
    __syncthreads();
  }
  const int M = red_i[0];
  if (i == 0 && tid == 0 && loss) *loss = M > 0 ? (float)(red_d[0] / M) : 0.f;
  if (!dlogits) return;
  const float gi = ids[i];
  if (!(gi >= 0.f) || M == 0) {                   // outside V, or a batch without an anchor: exactly 0
    for (int k = tid; k < d; k += NT) dlogits[(size_t)i * d + k] = 0.f;
    return;
  }
  for (int k = tid; k < d; k += NT) zi[k] = z[(size_t)i * d + k];
  __syncthreads();
  const float tau = *temperature, lse_i = lse[i], invp_i = invp[i];
  for (int j = wave; j < N; j += NTX_WAVES) {
    const float dot = ntx_wave_dot(zi, z + (size_t)j * d, d, lane);
    if (lane == 0) {
      float c = 0.f;
      if (j != i && ids[j] >= 0.f) {
        const float s = dot / tau, pos = ids[j] == gi ? 1.f : 0.f, invp_j = invp[j];
        if (invp_i > 0.f) c += expf(s - lse_i) - pos * invp_i;
        if (invp_j > 0.f) c += expf(s - lse[j]) - pos * invp_j;
      }
      crow[j] = c;
    }
  }
  __syncthreads();
  // dz_i: KW consecutive k at a time, the rows j dealt out to the NT / KW thread groups and the groups' sums added in group order
  int KW = 64;
  while (KW < d && KW < NT) KW <<= 1;
  const int G = NT / KW, grp = tid / KW, c = tid % KW;
  const float scale = 1.f / (tau * (float)M);
  for (int k0 = 0; k0 < d; k0 += KW) {
    const int k = k0 + c;
    float acc = 0.f;
    if (k < d) {
#pragma unroll 8
      for (int j = grp; j < N; j += G) acc = fmaf(crow[j], z[(size_t)j * d + k], acc);
    }
    part[tid] = acc;
    __syncthreads();
    if (grp == 0 && k < d) {
      float t = part[c];
      for (int h = 1; h < G; ++h) t += part[c + h * KW];
      dzs[k] = t * scale;
    }
    __syncthreads();
  }
  // back through z = e / max(|e|, eps): (dz - (dz . z) z) / |e| above the clamp, dz / eps below it
  double dp = 0.0;
  for (int k = tid; k < d; k += NT) dp += (double)dzs[k] * zi[k];
  red_d[tid] = dp;
  __syncthreads();
  for (int h = NT / 2; h > 0; h >>= 1) {
    if (tid < h) red_d[tid] += red_d[tid + h];
    __syncthreads();
  }
  const float n = nrm[i], den = fmaxf(n, NTX_EPS), proj = n >= NTX_EPS ? (float)red_d[0] : 0.f;
  for (int k = tid; k < d; k += NT) dlogits[(size_t)i * d + k] = (dzs[k] - proj * zi[k]) / den * grad_scale;
}

}  // namespace

long long cx_ntxent_scratch(int N, int d) {
  if (N < 1 || d < 1 || N > NTX_MAX_N || d > NTX_MAX_D) return 0;
  return (long long)N * d + 4ll * N;
}

int cx_ntxent_fwd_bwd(const float* e, const float* ids, const float* temperature, float* loss, float* loss_elem, float* dlogits,
                      int* top1, float grad_scale, float* scratch, long long scratch_floats, int N, int d, void* stream) {
  if (!e || !ids || !temperature || !scratch || N < 1 || d < 1) return CX_EINVAL;
  if (N > NTX_MAX_N || d > NTX_MAX_D) return CX_ESHAPE;
  if (scratch_floats < cx_ntxent_scratch(N, d)) return CX_EINVAL;
  float *z = scratch, *nrm = z + (size_t)N * d, *lse = nrm + N, *invp = lse + N, *ell = invp + N;
  hipLaunchKernelGGL(ntx_norm_kernel, dim3((N + NTX_WAVES - 1) / NTX_WAVES), dim3(NT), 0, as_stream(stream), e, ids, z, nrm, N, d);
  hipLaunchKernelGGL(ntx_row_kernel, dim3(N), dim3(NT), 0, as_stream(stream), z, ids, temperature, lse, invp, ell, loss_elem, top1, N, d);
  if (loss || dlogits)
    hipLaunchKernelGGL(ntx_grad_kernel, dim3(dlogits ? N : 1), dim3(NT), 0, as_stream(stream), z, nrm, ids, temperature, lse, invp, ell,
                       loss, dlogits, grad_scale, N, d);
  return launch_status();
}

int cx_bce_fwd_bwd(const float* logits, const float* target, float* loss, float* loss_elem, float* dlogits, float grad_scale,
                   int B, int n_classes, void* stream) {
  if (!logits || !target || B <= 0 || n_classes <= 0) return CX_EINVAL;
  return launch_elem_loss<BceTerm>(logits, target, nullptr, nullptr, loss, loss_elem, dlogits, grad_scale, B, n_classes, stream);
}

int cx_bce_masked_fwd_bwd(const float* logits, const float* target, const float* pos_weight, float* loss, float* loss_elem,
                          float* dlogits, float grad_scale, int B, int n_classes, void* stream) {
  if (!logits || !target || B <= 0 || n_classes <= 0) return CX_EINVAL;
  return (pos_weight ? launch_elem_loss<WeightedBceTerm> : launch_elem_loss<MaskedBceTerm>)(
      logits, target, pos_weight, nullptr, loss, loss_elem, dlogits, grad_scale, B, n_classes, stream);
}

int cx_asl_fwd_bwd(const float* logits, const float* target, const float* pos_weight, const float* focus, float* loss, float* loss_elem,
                   float* dlogits, float grad_scale, int B, int n_classes, void* stream) {
  if (!logits || !target || !focus || B < 1 || n_classes < 1 || (long long)B * n_classes > INT_MAX - NT) return CX_EINVAL;
  return launch_elem_loss<AslTerm>(logits, target, pos_weight, focus, loss, loss_elem, dlogits, grad_scale, B, n_classes, stream);
}

int cx_mc3_fwd_bwd(const float* logits, const float* target, const float* class_weight, float* loss, float* loss_elem, float* dlogits,
                   float grad_scale, int B, int n, void* stream) {
  if (!logits || !target || B < 1 || n < 1 || (long long)B * n > INT_MAX - NT) return CX_EINVAL;
  hipLaunchKernelGGL(mc3_loss_kernel, dim3(1), dim3(NT), 0, as_stream(stream), logits, target, class_weight, loss, loss_elem, dlogits,
                     grad_scale, B, n);
  return launch_status();
}

int cx_mc3_collapse(const float* logits, float* z, float* p_unc, int B, int n, void* stream) {
  if (!logits || !z || B < 1 || n < 1 || (long long)B * n > INT_MAX - NT) return CX_EINVAL;
  const long long total = (long long)B * n;
  hipLaunchKernelGGL(mc3_collapse_kernel, dim3((unsigned)((total + NT - 1) / NT)), dim3(NT), 0, as_stream(stream), logits, z, p_unc, total);
  return launch_status();
}

int cx_hier_fwd_bwd(const float* logits, const float* target, const int* parent, const float* pos_weight, int mode, float* loss,
                    float* loss_elem, float* dlogits, float grad_scale, int B, int n, void* stream) {
  if (!logits || !target || !parent || B < 1 || n < 1 || n > HMAXN || (mode != 0 && mode != 1) || (long long)B * n > INT_MAX - NT)
    return CX_EINVAL;
  auto kernel = mode == 1 ? hier_uncond_kernel : (pos_weight ? hier_cond_kernel<WeightedBceTerm> : hier_cond_kernel<MaskedBceTerm>);
  hipLaunchKernelGGL(kernel, dim3(1), dim3(NT), 0, as_stream(stream), logits, target, parent, pos_weight, loss, loss_elem, dlogits,
                     grad_scale, B, n);
  return launch_status();
}

int cx_hier_collapse(const float* logits, const int* parent, float* z, float* p, int B, int n, void* stream) {
  if (!logits || !parent || !z || B < 1 || n < 1 || n > HMAXN || (long long)B * n > INT_MAX - NT) return CX_EINVAL;
  const long long total = (long long)B * n;
  hipLaunchKernelGGL(hier_collapse_kernel, dim3((unsigned)((total + NT - 1) / NT)), dim3(NT), 0, as_stream(stream), logits, parent, z, p,
                     total, n);
  return launch_status();
}

int cx_softmax_ce_fwd_bwd(const float* logits, const int64_t* target, float* loss, float* loss_elem, float* dlogits, float grad_scale,
                          int B, int n_classes, void* stream) {
  if (!logits || !target || B <= 0 || n_classes <= 0) return CX_EINVAL;
  hipLaunchKernelGGL(softmax_ce_kernel, dim3(1), dim3(256), 0, as_stream(stream), logits, (const long long*)target, loss, loss_elem,
                     dlogits, grad_scale, B, n_classes);
  return launch_status();
}

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
