// Parameter groups for the fused optimisers: per-group learning-rate multiplier, weight decay (L2 or decoupled), frozen groups and a
// per-group step count, on the engine's flat fp32 buffers.
//
// The flat buffers hold every parameter tensor at an offset that is a multiple of 4 floats, zero-padded to a multiple of 4.  The
// kernels here walk a table of work items instead of the flat index range:
//
//   item  = uint32[4] {start4, len4, group, tensor}   a run of len4 16-byte units from unit start4, all of ONE tensor
//                                                      (len4 <= cx_optim_item_vec4(); items in buffer order, covering every unit once)
//   group = float[4]  {lr_mult, weight_decay, frozen, t0}   one row per group, 1 <= G <= 256, in DEVICE memory: a captured hipGraph
//                                                      of the training step sees a row that was rewritten between two replays
//
//   cx_grad_norm_items  the segmented form of cx_grad_norm: one partial per item, then ONE workgroup that sums the partials per group
//                       in item order, the unfrozen groups in group order, and writes clip[4] as cx_grad_norm does.  No atomics.
//   cx_*_step_items     one kernel template over the three update rules; a workgroup takes slices of items, reads the item's group
//                       row once per slice and streams it with 16-byte loads and stores; an item of a frozen group is skipped: no
//                       byte written
//
// The cut into items never changes what is computed for an element: every element sees the same expressions on the same values
// whatever item it falls in (tests/test_optim_groups_gpu.py: one group against five, bit for bit).
#include <math.h>
#include "common.h"

namespace {

constexpr int OG_THREADS = 256;          // 4 waves; one pass of a workgroup covers 256 16-byte units (4 KiB of each buffer)
constexpr int OG_MAX_BLOCKS = 2048;      // 256 CUs x 8 workgroups
// Longest item, in 16-byte units.  A constant: the table (and with it the summation tree of the norm) is a function of the parameter
// shapes and the group assignment alone, never of the device or of occupancy.  Chosen from profiles/optim_groups_bench.txt: the
// second launch of the norm adds the partials one by one, so its time grows with the number of items and wants them long ...
constexpr int OG_ITEM_VEC4 = 8192;
// ... while the steps want many small pieces to spread over the workgroups (DenseNet121 is 530 items of this length), so a step
// hands out slices of items: OG_SLOT_VEC4 units (16 KiB of each buffer), OG_ITEM_VEC4 / OG_SLOT_VEC4 slots per item.
constexpr int OG_SLOT_VEC4 = 1024;
constexpr int OG_SLOTS = OG_ITEM_VEC4 / OG_SLOT_VEC4;
constexpr int OG_MAX_GROUPS = 256;

inline int og_blocks(long long work) { return work < 1 ? 1 : work > OG_MAX_BLOCKS ? OG_MAX_BLOCKS : (int)work; }

struct Item {
  uint32_t start4, len4, group, tensor;
};

// ---- the norm -------------------------------------------------------------------------------------------------------------------
// Launch 1.  Workgroup b takes items b, b + gridDim.x, ...; thread t takes units t, t + 256, ... of the item into four accumulators,
// one per component (fused multiply-adds), joins them as (a0 + a1) + (a2 + a3), then the wave fold (6 shuffle levels) and the 4 wave
// sums in wave order: the arithmetic of grad_sq_partial_kernel (optim_ex.hip) on one item.  One plain store per item.
__global__ __launch_bounds__(OG_THREADS) void item_sq_partial_kernel(const float* __restrict__ g, const Item* __restrict__ items,
                                                                      int n_items, float gscale, float* __restrict__ part) {
  __shared__ float wave_sum[OG_THREADS / 64];
  const f32x4* __restrict__ g4 = reinterpret_cast<const f32x4*>(g);
  for (int it = blockIdx.x; it < n_items; it += gridDim.x) {
    const Item item = items[it];
    const size_t lo = item.start4, hi = lo + item.len4;
    float a0 = 0.f, a1 = 0.f, a2 = 0.f, a3 = 0.f;
#pragma unroll 4
    for (size_t i = lo + threadIdx.x; i < hi; i += OG_THREADS) {
      const f32x4 v = g4[i];
      const float x0 = v[0] * gscale, x1 = v[1] * gscale, x2 = v[2] * gscale, x3 = v[3] * gscale;
      a0 = fmaf(x0, x0, a0);
      a1 = fmaf(x1, x1, a1);
      a2 = fmaf(x2, x2, a2);
      a3 = fmaf(x3, x3, a3);
    }
    float v = (a0 + a1) + (a2 + a3);
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) v += __shfl_down(v, off, 64);
    if ((threadIdx.x & 63) == 0) wave_sum[threadIdx.x >> 6] = v;
    __syncthreads();
    if (threadIdx.x == 0) part[it] = ((wave_sum[0] + wave_sum[1]) + wave_sum[2]) + wave_sum[3];
    __syncthreads();                                       // wave_sum is written again for the next item
  }
}

// Launch 2: one workgroup.  Thread q < G owns group q: it adds the partials of the group's items one by one in item order, writes
// group_sq[q] and group_norm[q] -- for a frozen group too.  The items pass through LDS 256 at a time; every thread reads the same
// four (group, partial) pairs per step (16-byte broadcasts) and adds either the partial or +0 (exact: the sum is never negative), so
// the only instruction on the dependent chain is the addition itself.  Thread 0 then adds group_sq of the groups with frozen == 0
// in group order and writes clip = {norm, coef, nonfinite, skipped} as grad_norm_final_kernel defines them.  A partial of another
// group is selected away, never multiplied by zero: an inf or NaN in a frozen group reaches that group's group_norm and nothing else.
__global__ __launch_bounds__(OG_THREADS) void group_norm_final_kernel(const float* __restrict__ part, const Item* __restrict__ items,
                                                                       int n_items, const float* __restrict__ groups, int n_groups,
                                                                       float max_norm, int skip_nonfinite, float* __restrict__ group_sq,
                                                                       float* __restrict__ group_norm, float* __restrict__ clip) {
  __shared__ __attribute__((aligned(16))) float s_part[OG_THREADS];
  __shared__ __attribute__((aligned(16))) uint32_t s_group[OG_THREADS];
  __shared__ float s_sq[OG_MAX_GROUPS];
  const uint32_t q = threadIdx.x;
  float acc = 0.f;
  for (int base = 0; base < n_items; base += OG_THREADS) {
    const int cnt = n_items - base < OG_THREADS ? n_items - base : OG_THREADS;
    const bool have = (int)threadIdx.x < cnt;
    s_part[threadIdx.x] = have ? part[base + threadIdx.x] : 0.f;
    s_group[threadIdx.x] = have ? items[base + threadIdx.x].group : 0xffffffffu;      // matches no group
    __syncthreads();
    if (q < (uint32_t)n_groups) {
#pragma unroll 4
      for (int j = 0; j < cnt; j += 4) {
        const uint4 gq = *reinterpret_cast<const uint4*>(&s_group[j]);
        const f32x4 pv = *reinterpret_cast<const f32x4*>(&s_part[j]);
        acc += gq.x == q ? pv[0] : 0.f;
        acc += gq.y == q ? pv[1] : 0.f;
        acc += gq.z == q ? pv[2] : 0.f;
        acc += gq.w == q ? pv[3] : 0.f;
      }
    }
    __syncthreads();
  }
  if (q < (uint32_t)n_groups) {
    s_sq[q] = acc;
    group_sq[q] = acc;
    group_norm[q] = sqrtf(acc);
  }
  __syncthreads();
  if (threadIdx.x != 0) return;
  float sum = 0.f;
  for (int k = 0; k < n_groups; ++k)
    if (groups[4 * k + 2] == 0.f) sum += s_sq[k];
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

// ---- the steps ------------------------------------------------------------------------------------------------------------------
// A rule holds its state pointers and the constants of the optimiser; begin() takes what the group row fixes (lr_g = lr * lr_mult,
// the group's own 1-based step t_g = t - t0), update() is the expression of the *_ex rules (optim_ex.hip) on values in registers.
struct GTail {
  const float* clip;
  float* ema;
  float ema_decay;
  int ema_warmup;
  int skip_nonfinite;
};

struct AdamItems {
  float *s0, *s1;                 // m, v
  float b1, b2, eps;
  float step_size, bc2_sqrt;
  static constexpr bool two = true;
  __device__ __forceinline__ void begin(float lr_g, float t_g) {
    step_size = lr_g / (1.f - powf(b1, t_g));
    bc2_sqrt = sqrtf(1.f - powf(b2, t_g));
  }
  __device__ __forceinline__ float update(float gi, float pi, float& mi, float& vi) const {
    mi = b1 * mi + (1.f - b1) * gi;
    vi = b2 * vi + (1.f - b2) * gi * gi;
    const float denom = sqrtf(vi) / bc2_sqrt + eps;
    return pi - step_size * (mi / denom);
  }
};

// (no `first step' switch: the momentum buffer starts as zeros and a frozen item never writes it, so momentum * 0 + g IS g on the
// first step of a group, whenever that is)
struct SgdItems {
  float *s0, *s1;                 // buf, unused
  float mom;
  float lr_g;
  static constexpr bool two = false;
  __device__ __forceinline__ void begin(float lr, float) { lr_g = lr; }
  __device__ __forceinline__ float update(float gi, float pi, float& bi, float&) const {
    bi = mom * bi + gi;
    return pi - lr_g * (gi + mom * bi);
  }
};

struct RmsItems {
  float *s0, *s1;                 // sq, buf
  float alpha, eps, mom;
  float lr_g;
  static constexpr bool two = true;
  __device__ __forceinline__ void begin(float lr, float) { lr_g = lr; }
  __device__ __forceinline__ float update(float gi, float pi, float& si, float& bi) const {
    si = alpha * si + (1.f - alpha) * gi * gi;
    const float avg = sqrtf(si) + eps;
    if (mom > 0.f) {
      bi = mom * bi + gi / avg;
      return pi - lr_g * bi;
    }
    return pi - lr_g * gi / avg;
  }
};

// `hyper` null: lr and the 1-based step number are the host's arguments; else hyper[0] and hyper[1] + 1 (cx_optim_tick's table).
template <class Rule>
__global__ __launch_bounds__(OG_THREADS) void step_items_kernel(Rule r, float* __restrict__ p, const float* __restrict__ g,
                                                                 const Item* __restrict__ items, int n_items,
                                                                 const float* __restrict__ groups, int decoupled,
                                                                 const float* __restrict__ hyper, float lr, int step, float gscale,
                                                                 GTail x) {
  if (x.clip && x.skip_nonfinite && x.clip[2] != 0.f) return;        // the whole grid takes the same side: nothing is written
  const float t = hyper ? hyper[1] + 1.f : (float)step;
  if (hyper) lr = hyper[0];
  const float gs = gscale * (x.clip ? x.clip[1] : 1.f);
  float d = x.ema_decay;
  if (x.ema && x.ema_warmup) d = fminf(d, (1.f + t) / (10.f + t));
  const float omd = 1.f - d;
  f32x4* __restrict__ p4 = reinterpret_cast<f32x4*>(p);
  const f32x4* __restrict__ g4 = reinterpret_cast<const f32x4*>(g);
  f32x4* s04 = reinterpret_cast<f32x4*>(r.s0);
  f32x4* s14 = reinterpret_cast<f32x4*>(r.s1);
  f32x4* e4 = reinterpret_cast<f32x4*>(x.ema);
  const bool has_s1 = Rule::two && r.s1 != nullptr;
  // slot s = slice s / n_items of item s % n_items (slice-major: with the slice as the fast index a grid of 2048 = 256 * OG_SLOTS
  // workgroups would give workgroup b the slice b % OG_SLOTS of every item it meets, and the short items have only slice 0 --
  // measured 4x slower); a slice past the end of a short item is empty
  for (long long s = blockIdx.x; s < (long long)n_items * OG_SLOTS; s += gridDim.x) {
    const Item item = items[s % n_items];
    const uint32_t first = (uint32_t)(s / n_items) * OG_SLOT_VEC4;
    if (first >= item.len4) continue;
    const float* __restrict__ row = groups + 4 * (size_t)item.group;
    const float lr_mult = row[0], wd = row[1], frozen = row[2], t0 = row[3];
    if (frozen != 0.f) continue;                                     // uniform over the workgroup
    const float lr_g = lr * lr_mult;
    r.begin(lr_g, t - t0);
    const float keep = 1.f - lr_g * wd;                              // decoupled: p <- p * (1 - lr_g * wd_g), then the rule without decay
    const float l2 = decoupled ? 0.f : wd;
    const uint32_t last = first + OG_SLOT_VEC4 < item.len4 ? first + OG_SLOT_VEC4 : item.len4;
    const size_t lo = (size_t)item.start4 + first, hi = (size_t)item.start4 + last;
    for (size_t i = lo + threadIdx.x; i < hi; i += OG_THREADS) {
      // every load of the unit ahead of its stores
      const f32x4 gv = g4[i];
      f32x4 pv = p4[i];
      f32x4 av = s04[i];
      f32x4 bv = has_s1 ? s14[i] : f32x4{0.f, 0.f, 0.f, 0.f};
      f32x4 ev = e4 ? e4[i] : f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
      for (int c = 0; c < 4; ++c) {
        float pi = pv[c], gi = gv[c] * gs;
        if (decoupled)
          pi = pi * keep;
        else if (l2 != 0.f)
          gi += l2 * pi;
        float a = av[c], b = bv[c];
        const float pn = r.update(gi, pi, a, b);
        av[c] = a;
        bv[c] = b;
        pv[c] = pn;
        ev[c] = d * ev[c] + omd * pn;
      }
      p4[i] = pv;
      s04[i] = av;
      if (has_s1) s14[i] = bv;
      if (e4) e4[i] = ev;
    }
  }
}

int check_tables(size_t n, const void* items, int n_items, const void* groups, int n_groups) {
  if (!items || !groups || n_items < 0) return CX_EINVAL;
  if (n_groups < 1 || n_groups > OG_MAX_GROUPS) return CX_EINVAL;
  if ((n & 3) != 0) return CX_EINVAL;                       // the flat buffers are whole 16-byte units
  if (n > 0 && n_items == 0) return CX_EINVAL;
  if (!aligned16(items) || !aligned16(groups)) return CX_EALIGN;
  return 0;
}

template <class Rule>
int launch_step_items(const Rule& r, float* p, const float* g, size_t n, const uint32_t* items, int n_items, const float* groups,
                      int n_groups, int decoupled, const float* hyper, float lr, int step, float gscale, const float* clip, float* ema,
                      float ema_decay, int ema_warmup, int skip_nonfinite, void* stream) {
  if (!p || !g || !r.s0) return CX_EINVAL;
  if (const int e = check_tables(n, items, n_items, groups, n_groups)) return e;
  if (ema && !(ema_decay >= 0.f && ema_decay <= 1.f)) return CX_EINVAL;
  if (!hyper && step < 1) return CX_EINVAL;
  if (!aligned16(p) || !aligned16(g) || !aligned16(r.s0) || !aligned16(r.s1) || !aligned16(ema)) return CX_EALIGN;
  if (n == 0) return 0;
  const GTail x = {clip, ema, ema_decay, ema_warmup, skip_nonfinite};
  hipLaunchKernelGGL(step_items_kernel<Rule>, dim3(og_blocks((long long)n_items * OG_SLOTS)), dim3(OG_THREADS), 0, as_stream(stream), r, p, g,
                     reinterpret_cast<const Item*>(items), n_items, groups, decoupled ? 1 : 0, hyper, lr, step, gscale, x);
  return launch_status();
}

}  // namespace

extern "C" {

int cx_optim_item_vec4(void) { return OG_ITEM_VEC4; }

int cx_grad_norm_items(const float* g, size_t n, const uint32_t* items, int n_items, const float* groups, int n_groups,
                       float grad_scale, float max_norm, int skip_nonfinite, float* partials, float* group_sq, float* group_norm,
                       float* clip, void* stream) {
  if (!clip || !group_sq || !group_norm || (n && (!g || !partials))) return CX_EINVAL;
  if (const int e = check_tables(n, items, n_items, groups, n_groups)) return e;
  if (n && !aligned16(g)) return CX_EALIGN;
  const Item* tab = reinterpret_cast<const Item*>(items);
  if (n == 0) n_items = 0;
  if (n_items)
    hipLaunchKernelGGL(item_sq_partial_kernel, dim3(og_blocks(n_items)), dim3(OG_THREADS), 0, as_stream(stream), g, tab, n_items,
                       grad_scale, partials);
  hipLaunchKernelGGL(group_norm_final_kernel, dim3(1), dim3(OG_THREADS), 0, as_stream(stream), partials, tab, n_items, groups, n_groups,
                     max_norm, skip_nonfinite, group_sq, group_norm, clip);
  return launch_status();
}

int cx_adam_step_items(float* p, const float* g, float* m, float* v, size_t n, const uint32_t* items, int n_items, const float* groups,
                       int n_groups, int decoupled, const float* hyper, float lr, int step, float beta1, float beta2, float eps,
                       float grad_scale, const float* clip, float* ema, float ema_decay, int ema_warmup, int skip_nonfinite,
                       void* stream) {
  if (!v) return CX_EINVAL;
  const AdamItems r = {m, v, beta1, beta2, eps, 0.f, 1.f};
  return launch_step_items(r, p, g, n, items, n_items, groups, n_groups, decoupled, hyper, lr, step, grad_scale, clip, ema, ema_decay,
                           ema_warmup, skip_nonfinite, stream);
}

int cx_sgd_nesterov_step_items(float* p, const float* g, float* buf, size_t n, const uint32_t* items, int n_items, const float* groups,
                               int n_groups, int decoupled, const float* hyper, float lr, int step, float momentum, float grad_scale,
                               const float* clip, float* ema, float ema_decay, int ema_warmup, int skip_nonfinite, void* stream) {
  const SgdItems r = {buf, nullptr, momentum, 0.f};
  return launch_step_items(r, p, g, n, items, n_items, groups, n_groups, decoupled, hyper, lr, step, grad_scale, clip, ema, ema_decay,
                           ema_warmup, skip_nonfinite, stream);
}

int cx_rmsprop_step_items(float* p, const float* g, float* sq, float* buf, size_t n, const uint32_t* items, int n_items,
                          const float* groups, int n_groups, int decoupled, const float* hyper, float lr, int step, float alpha, float eps,
                          float momentum, float grad_scale, const float* clip, float* ema, float ema_decay, int ema_warmup,
                          int skip_nonfinite, void* stream) {
  if (momentum > 0.f && !buf) return CX_EINVAL;
  const RmsItems r = {sq, buf, alpha, eps, momentum, 0.f};
  return launch_step_items(r, p, g, n, items, n_items, groups, n_groups, decoupled, hyper, lr, step, grad_scale, clip, ema, ema_decay,
                           ema_warmup, skip_nonfinite, stream);
}

}  // extern "C"
