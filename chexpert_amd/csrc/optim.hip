// The fused optimisers over the engine's flat fp32 buffers: Adam, SGD with Nesterov momentum and RMSprop, each update rule stated
// once, in three kernel families.
//
//   cx_*_step[_dev]       the plain one-kernel update.  `_dev`: the learning rate and the step count live in device memory
//                         (hyper = {lr, steps_done, sched_kind, gamma, warmup_steps, milestone0, milestone1, base_lr}), so a captured
//                         hipGraph can be replayed while both change; cx_optim_tick advances them
//   cx_grad_norm          two launches, no atomics: per-workgroup partial sums of (grad_scale * g)^2 over fixed contiguous ranges, then
//                         ONE workgroup that sums the partials and writes clip[4] = {norm, coef, nonfinite, skipped} to device memory
//   cx_*_step[_dev]_ex    the plain update with the gradient multiplied by clip[1], nothing written at all when clip[2] says the
//                         gradient was not finite and skipping is on, and ema = d * ema + (1 - d) * p_new written by the thread that
//                         computed p_new; with clip and ema both null the call IS the plain entry point (its kernel, its bits)
//   cx_grad_norm_items    the segmented form of cx_grad_norm: one partial per item, then ONE workgroup that sums the partials per group
//                         in item order, the unfrozen groups in group order, and writes clip[4] as cx_grad_norm does.  No atomics.
//   cx_*_step_items       parameter groups (per-group learning-rate multiplier, weight decay (L2 or decoupled), frozen groups, a
//                         per-group step count): a workgroup takes slices of items, reads the item's group row once per slice and
//                         streams it with 16-byte loads and stores; an item of a frozen group is skipped: no byte written
//   cx_lamb_step_items    the grouped steps with a per-tensor trust ratio |p| / |update| (LAMB on Adam, LARS on SGD-Nesterov): per-item
//   cx_lars_step_items    partial sums, ONE workgroup that adds them per tensor in item order, then the update (three launches)
//   cx_sam_*_items        sharpness-aware minimisation around any of the steps: the norm of the (ASAM: weight-scaled) gradient in two
//                         launches, the ascent step with a backup of the weights, the copy back
//
// The grouped kernels walk a table of work items instead of the flat index range.  The flat buffers hold every parameter tensor at
// an offset that is a multiple of 4 floats, zero-padded to a multiple of 4:
//
//   item  = uint32[4] {start4, len4, group, tensor}   a run of len4 16-byte units from unit start4, all of ONE tensor
//                                                      (len4 <= cx_optim_item_vec4(); items in buffer order, covering every unit once)
//   group = float[4]  {lr_mult, weight_decay, frozen, t0}   one row per group, 1 <= G <= 256, in DEVICE memory: a captured hipGraph
//                                                      of the training step sees a row that was rewritten between two replays
//
// The cut into items never changes what is computed for an element: every element sees the same expressions on the same values
// whatever item it falls in (tests/test_optim_groups_gpu.py: one group against five, bit for bit).
//
// Nothing here reads a gradient on the host, so a captured hipGraph of the training step replays all of it.
#include <math.h>
#include "common.h"

namespace {

constexpr int THREADS = 256;             // 4 waves; one pass of a workgroup covers 256 16-byte units (4 KiB of each buffer)
constexpr int MAX_BLOCKS = 2048;         // 256 CUs x 8 workgroups
constexpr int GN_MIN_VEC = 1024;         // 16-byte loads per workgroup before a second workgroup is worth its launch (16 KB)
// Longest item, in 16-byte units.  A constant: the table (and with it the summation tree of the norm) is a function of the parameter
// shapes and the group assignment alone, never of the device or of occupancy.  Chosen from profiles/optim_groups_bench.txt: the
// second launch of the norm adds the partials one by one, so its time grows with the number of items and wants them long ...
constexpr int OG_ITEM_VEC4 = 8192;
// ... while the steps want many small pieces to spread over the workgroups (DenseNet121 is 530 items of this length), so a step
// hands out slices of items: OG_SLOT_VEC4 units (16 KiB of each buffer), OG_ITEM_VEC4 / OG_SLOT_VEC4 slots per item.
constexpr int OG_SLOT_VEC4 = 1024;
constexpr int OG_SLOTS = OG_ITEM_VEC4 / OG_SLOT_VEC4;
constexpr int OG_MAX_GROUPS = 256;

struct Item {
  uint32_t start4, len4, group, tensor;
};

inline int blocks_for(long long work) { return work < 1 ? 1 : work > MAX_BLOCKS ? MAX_BLOCKS : (int)work; }

// The grid of cx_grad_norm is a function of n alone (never of the device or of occupancy), so the summation tree, and with it every
// bit of the norm, is the same on every run and on every rank of a data-parallel job.
inline int gn_blocks(size_t n) { return n == 0 ? 0 : blocks_for((long long)(((n >> 2) + GN_MIN_VEC - 1) / GN_MIN_VEC)); }

// ---- the norms ------------------------------------------------------------------------------------------------------------------
// Thread t takes the 16-byte units lo + t, lo + t + 256, ... < hi of g into four accumulators, one per component (fused
// multiply-adds), and joins them as (a0 + a1) + (a2 + a3).  Coalesced: a wave reads 1 KiB per instruction.  g is read with plain
// loads: the step that follows reads it again, out of the caches where it still fits.
__device__ __forceinline__ float sq_units(const float* __restrict__ g, size_t lo, size_t hi, float gscale) {
  const f32x4* __restrict__ g4 = reinterpret_cast<const f32x4*>(g);
  float a0 = 0.f, a1 = 0.f, a2 = 0.f, a3 = 0.f;
#pragma unroll 4
  for (size_t i = lo + threadIdx.x; i < hi; i += THREADS) {
    const f32x4 v = g4[i];
    const float x0 = v[0] * gscale, x1 = v[1] * gscale, x2 = v[2] * gscale, x3 = v[3] * gscale;
    a0 = fmaf(x0, x0, a0);
    a1 = fmaf(x1, x1, a1);
    a2 = fmaf(x2, x2, a2);
    a3 = fmaf(x3, x3, a3);
  }
  return (a0 + a1) + (a2 + a3);
}

// wave fold (6 shuffle levels, lane 0 ends with the sum of the wave), then the 4 wave sums in wave order; valid in thread 0.  A
// caller that folds again puts a __syncthreads() between the two: wave_sum is written anew.
__device__ __forceinline__ float block_fold(float v) {
  __shared__ float wave_sum[THREADS / 64];
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) v += __shfl_down(v, off, 64);
  if ((threadIdx.x & 63) == 0) wave_sum[threadIdx.x >> 6] = v;
  __syncthreads();
  return ((wave_sum[0] + wave_sum[1]) + wave_sum[2]) + wave_sum[3];
}

// One thread, the sum of squares in hand.  clip = {norm, coef, nonfinite, skipped}: coef is torch.nn.utils.clip_grad_norm_'s
// clamp(max_norm / (norm + 1e-6), max = 1) (1 when max_norm <= 0: clipping off, the norm is still reported); `skipped` counts the
// steps that the kernels below will drop (a float: exact up to 2^24).
__device__ __forceinline__ void write_clip(float sum, float max_norm, int skip_nonfinite, float* __restrict__ clip) {
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

// cx_grad_norm, launch 1.  Workgroup b owns the 16-byte units [b * per, min((b + 1) * per, n / 4)), per = ceil((n / 4) / gridDim.x).
// The n % 4 trailing floats go to threads 0..2 of the last workgroup.
__global__ __launch_bounds__(THREADS) void grad_sq_partial_kernel(const float* __restrict__ g, size_t n, float gscale,
                                                                   float* __restrict__ part) {
  const size_t n4 = n >> 2;
  const size_t per = (n4 + gridDim.x - 1) / gridDim.x;
  const size_t lo = (size_t)blockIdx.x * per;
  const size_t hi = lo + per < n4 ? lo + per : n4;
  float acc = sq_units(g, lo, hi, gscale);
  if (blockIdx.x == gridDim.x - 1 && threadIdx.x < (n & 3)) {
    const float x = g[(n4 << 2) + threadIdx.x] * gscale;
    acc = fmaf(x, x, acc);
  }
  const float s = block_fold(acc);
  if (threadIdx.x == 0) part[blockIdx.x] = s;
}

// cx_grad_norm, launch 2: one workgroup.  Thread t sums partials [t * per, (t + 1) * per) in index order (per = ceil(nparts / 256)
// <= 8), the 256 sums are folded as above.
__global__ __launch_bounds__(THREADS) void grad_norm_final_kernel(const float* __restrict__ part, int nparts, float max_norm,
                                                                   int skip_nonfinite, float* __restrict__ clip) {
  const int per = (nparts + THREADS - 1) / THREADS;
  const int lo = threadIdx.x * per;
  const int hi = lo + per < nparts ? lo + per : nparts;
  float acc = 0.f;
  for (int i = lo; i < hi; ++i) acc += part[i];
  const float sum = block_fold(acc);
  if (threadIdx.x == 0) write_clip(sum, max_norm, skip_nonfinite, clip);
}

// cx_grad_norm_items, launch 1.  Workgroup b takes items b, b + gridDim.x, ...; the units of an item are summed and folded as a
// range of grad_sq_partial_kernel is.  One plain store per item.
__global__ __launch_bounds__(THREADS) void item_sq_partial_kernel(const float* __restrict__ g, const Item* __restrict__ items,
                                                                   int n_items, float gscale, float* __restrict__ part) {
  for (int it = blockIdx.x; it < n_items; it += gridDim.x) {
    const Item item = items[it];
    const float s = block_fold(sq_units(g, item.start4, (size_t)item.start4 + item.len4, gscale));
    if (threadIdx.x == 0) part[it] = s;
    __syncthreads();
  }
}

// cx_grad_norm_items, launch 2: one workgroup.  Thread q < G owns group q: it adds the partials of the group's items one by one in
// item order, writes group_sq[q] and group_norm[q] -- for a frozen group too.  The items pass through LDS 256 at a time; every thread
// reads the same four (group, partial) pairs per step (16-byte broadcasts) and adds either the partial or +0 (exact: the sum is never
// negative), so the only instruction on the dependent chain is the addition itself.  Thread 0 then adds group_sq of the groups with
// frozen == 0 in group order.  A partial of another group is selected away, never multiplied by zero: an inf or NaN in a frozen
// group reaches that group's group_norm and nothing else.
__global__ __launch_bounds__(THREADS) void group_norm_final_kernel(const float* __restrict__ part, const Item* __restrict__ items,
                                                                    int n_items, const float* __restrict__ groups, int n_groups,
                                                                    float max_norm, int skip_nonfinite, float* __restrict__ group_sq,
                                                                    float* __restrict__ group_norm, float* __restrict__ clip) {
  __shared__ __attribute__((aligned(16))) float s_part[THREADS];
  __shared__ __attribute__((aligned(16))) uint32_t s_group[THREADS];
  __shared__ float s_sq[OG_MAX_GROUPS];
  const uint32_t q = threadIdx.x;
  float acc = 0.f;
  for (int base = 0; base < n_items; base += THREADS) {
    const int cnt = n_items - base < THREADS ? n_items - base : THREADS;
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
  write_clip(sum, max_norm, skip_nonfinite, clip);
}

// ---- the update rules -----------------------------------------------------------------------------------------------------------
// A rule holds its state pointers (s0, s1) and the constants of the optimiser.  begin(lr, t) takes what a launch, or a group row,
// fixes: the learning rate and the 1-based step number; update() is the rule on values in registers, the gradient already scaled
// and decayed; has_s0() / has_s1() say whether the step reads a state at all (SGD's first step does not read buf, RMSprop
// without momentum never touches its buf).
struct AdamRule {
  float *s0, *s1;                 // m, v
  float b1, b2, eps;
  float bc1, bc2_sqrt;            // host_bc: the bias corrections are the host's powf (cx_adam_step[_ex]); else begin() computes them
  bool host_bc;
  float step_size;
  __device__ __forceinline__ bool has_s0() const { return true; }
  __device__ __forceinline__ bool has_s1() const { return true; }
  __device__ __forceinline__ void begin(float lr, float t) {
    if (!host_bc) {
      bc1 = 1.f - powf(b1, t);
      bc2_sqrt = sqrtf(1.f - powf(b2, t));
    }
    step_size = lr / bc1;
  }
  __device__ __forceinline__ float update(float gi, float pi, float& mi, float& vi) const {
    mi = b1 * mi + (1.f - b1) * gi;
    vi = b2 * vi + (1.f - b2) * gi * gi;
    const float denom = sqrtf(vi) / bc2_sqrt + eps;
    return pi - step_size * (mi / denom);
  }
};

struct SgdRule {
  float *s0, *s1;                 // buf, unused
  float mom;
  // The flat steps: 1 on the first step (buf is not read: it becomes g), 0 after it, -1: the first step is t == 1 (`hyper` form).
  // The grouped steps: 0 always.  There the momentum buffer starts as zeros and a frozen item never writes it, so momentum * 0 + g
  // IS g on the first step of a group, whenever that is.
  int first;
  float lr;
  __device__ __forceinline__ bool has_s0() const { return !first; }
  __device__ __forceinline__ bool has_s1() const { return false; }
  __device__ __forceinline__ void begin(float lr_, float t) {
    lr = lr_;
    if (first < 0) first = t == 1.f;
  }
  __device__ __forceinline__ float update(float gi, float pi, float& bi, float&) const {
    bi = first ? gi : mom * bi + gi;
    return pi - lr * (gi + mom * bi);
  }
};

struct RmsRule {
  float *s0, *s1;                 // sq, buf (may be null when mom == 0)
  float alpha, eps, mom;
  float lr;
  __device__ __forceinline__ bool has_s0() const { return true; }
  __device__ __forceinline__ bool has_s1() const { return mom > 0.f; }
  __device__ __forceinline__ void begin(float lr_, float) { lr = lr_; }
  __device__ __forceinline__ float update(float gi, float pi, float& si, float& bi) const {
    si = alpha * si + (1.f - alpha) * gi * gi;
    const float avg = sqrtf(si) + eps;
    if (mom > 0.f) {
      bi = mom * bi + gi / avg;
      return pi - lr * bi;
    }
    return pi - lr * gi / avg;
  }
};

// Weight decay ahead of the rule.  L2: g += wd * p.  Decoupled: p <- p * keep, keep = 1 - lr * wd, and the rule without decay
// (torch.optim.AdamW's order).
__device__ __forceinline__ void decay(float& gi, float& pi, bool decoupled, float wd, float keep) {
  if (decoupled)
    pi = pi * keep;
  else if (wd != 0.f)
    gi += wd * pi;
}

// ---- clip, skip and EMA: what the *_ex and the grouped steps share --------------------------------------------------------------
struct Tail {
  const float* clip;
  float* ema;
  float ema_decay;
  int ema_warmup;
  int skip_nonfinite;
};

// What a launch fixes before its loop.  `hyper` null: lr and the 1-based step number t are the host's arguments; else hyper[0] and
// hyper[1] + 1 (cx_optim_tick's table).  gs = grad_scale * clip[1] (clip null: grad_scale * 1); d = the EMA's decay at step t.
struct Launch {
  float lr, t, gs, d, omd;
};

// false: clip[2] says the gradient was not finite and skipping is on.  The whole grid takes the same side: nothing is written.
__device__ __forceinline__ bool begin_launch(const Tail& x, const float* __restrict__ hyper, float lr, int step, float gscale,
                                             Launch& q) {
  if (x.clip && x.skip_nonfinite && x.clip[2] != 0.f) return false;
  q.lr = hyper ? hyper[0] : lr;
  q.t = hyper ? hyper[1] + 1.f : (float)step;
  q.gs = gscale * (x.clip ? x.clip[1] : 1.f);
  q.d = x.ema_decay;
  if (x.ema && x.ema_warmup) q.d = fminf(q.d, (1.f + q.t) / (10.f + q.t));
  q.omd = 1.f - q.d;
  return true;
}

// CX_EINVAL / CX_EALIGN before any launch.  units16: the kernel moves ema in 16-byte units.
int check_tail(const float* hyper, int step, const float* ema, float ema_decay, bool units16) {
  if (ema && !(ema_decay >= 0.f && ema_decay <= 1.f)) return CX_EINVAL;
  if (!hyper && step < 1) return CX_EINVAL;
  if (units16 && !aligned16(ema)) return CX_EALIGN;
  return 0;
}

// ---- the flat steps -------------------------------------------------------------------------------------------------------------
// Adam and SGD (RMSprop: below).  One kernel per rule and per TAIL serves the host-lr and the `hyper` form.  TAIL false is the plain step: no clip, no skip, no EMA
// (x is not read).  Same source is not same bits: under -ffp-contract=fast what the compiler fuses into one rounding and what it
// packs two by two (v_pk_mul_f32) and adds unfused differs between the two instantiations, which is why the
// *_ex entry points hand a call without clip and without ema to the plain kernel.
template <class Rule, bool TAIL>
__global__ __launch_bounds__(THREADS) void step_kernel(Rule r, float* __restrict__ p, const float* __restrict__ g, size_t n,
                                                        const float* __restrict__ hyper, float lr, int step, float wd, float gscale,
                                                        Tail x_) {
  const Tail x = TAIL ? x_ : Tail{nullptr, nullptr, 0.f, 0, 0};
  Launch q;
  if (!begin_launch(x, hyper, lr, step, gscale, q)) return;
  r.begin(q.lr, q.t);
  const bool has_s1 = r.has_s1();
  for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (size_t)gridDim.x * blockDim.x) {
    const float e = x.ema ? x.ema[i] : 0.f;                          // ahead of the stores: every load of the element is in flight at once
    float gi = g[i] * q.gs, pi = p[i];
    decay(gi, pi, false, wd, 1.f);
    // a state that is not read gets a placeholder, which update() ignores.  For s0 it is gi and not a constant: that keeps the
    // decay above in the block that feeds this choice, where the compiler packs g * gs with wd * p and adds them unfused, as these
    // kernels always have (with 0.f here it fuses wd * p into the sum: another last bit whenever wd != 0)
    float a = r.has_s0() ? r.s0[i] : gi, b = has_s1 ? r.s1[i] : 0.f;
    const float pn = r.update(gi, pi, a, b);
    r.s0[i] = a;
    if (has_s1) r.s1[i] = b;
    p[i] = pn;
    if (x.ema) x.ema[i] = q.d * e + q.omd * pn;
  }
}

// clip and ema both null: the plain kernel (and `step`, which only the tail reads, goes unchecked)
template <class Rule>
int launch_step(const Rule& r, float* p, const float* g, size_t n, const float* hyper, float lr, int step, float wd, float gscale,
                const Tail& x, void* stream) {
  const dim3 grid(blocks_for((long long)((n + THREADS - 1) / THREADS)));
  if (!x.clip && !x.ema) {
    hipLaunchKernelGGL((step_kernel<Rule, false>), grid, dim3(THREADS), 0, as_stream(stream), r, p, g, n, hyper, lr, step, wd, gscale, x);
    return launch_status();
  }
  if (const int e = check_tail(hyper, step, x.ema, x.ema_decay, false)) return e;
  hipLaunchKernelGGL((step_kernel<Rule, true>), grid, dim3(THREADS), 0, as_stream(stream), r, p, g, n, hyper, lr, step, wd, gscale, x);
  return launch_status();
}

// ---- the flat RMSprop steps -----------------------------------------------------------------------------------------------------
// Stated separately from step_kernel, on memory: buf is read after sq is stored (and not at all without momentum).  With every load
// of the element ahead of its stores, as step_kernel has them, the same bits came 4 % slower at ResNet152's size
// (profiles/optim_refactor_bench.txt).  RmsRule::update is this rule on registers, for the grouped steps.
__device__ __forceinline__ float rmsprop_flat(float* sq, float* buf, size_t i, float gi, const float pi, float lr, float alpha,
                                              float eps, float mom, float wd) {
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

// plain: `hyper` null or not are two kernels, as they always were
__global__ void rmsprop_kernel(float* __restrict__ p, const float* __restrict__ g, float* __restrict__ sq, float* __restrict__ buf,
                               size_t n, float lr, float alpha, float eps, float mom, float wd, float gscale) {
  for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (size_t)gridDim.x * blockDim.x)
    p[i] = rmsprop_flat(sq, buf, i, g[i] * gscale, p[i], lr, alpha, eps, mom, wd);
}
__global__ void rmsprop_dev_kernel(float* __restrict__ p, const float* __restrict__ g, float* __restrict__ sq, float* __restrict__ buf,
                                   size_t n, const float* __restrict__ hyper, float alpha, float eps, float mom, float wd, float gscale) {
  const float lr = hyper[0];
  for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (size_t)gridDim.x * blockDim.x)
    p[i] = rmsprop_flat(sq, buf, i, g[i] * gscale, p[i], lr, alpha, eps, mom, wd);
}
// clip, skip and EMA
__global__ __launch_bounds__(THREADS) void rmsprop_ex_kernel(float* __restrict__ p, const float* __restrict__ g, float* sq, float* buf,
                                                              size_t n, const float* __restrict__ hyper, float lr, int step, float alpha,
                                                              float eps, float mom, float wd, float gscale, Tail x) {
  Launch q;
  if (!begin_launch(x, hyper, lr, step, gscale, q)) return;
  for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (size_t)gridDim.x * blockDim.x) {
    const float e = x.ema ? x.ema[i] : 0.f;
    const float pn = rmsprop_flat(sq, buf, i, g[i] * q.gs, p[i], q.lr, alpha, eps, mom, wd);
    p[i] = pn;
    if (x.ema) x.ema[i] = q.d * e + q.omd * pn;
  }
}

int launch_rmsprop(float* p, const float* g, float* sq, float* buf, size_t n, const float* hyper, float lr, int step, float alpha,
                   float eps, float mom, float wd, float gscale, const Tail& x, void* stream) {
  const dim3 grid(blocks_for((long long)((n + THREADS - 1) / THREADS)));
  if (x.clip || x.ema) {
    if (const int e = check_tail(hyper, step, x.ema, x.ema_decay, false)) return e;
    hipLaunchKernelGGL(rmsprop_ex_kernel, grid, dim3(THREADS), 0, as_stream(stream), p, g, sq, buf, n, hyper, lr, step, alpha, eps, mom,
                       wd, gscale, x);
  } else if (hyper) {
    hipLaunchKernelGGL(rmsprop_dev_kernel, grid, dim3(THREADS), 0, as_stream(stream), p, g, sq, buf, n, hyper, alpha, eps, mom, wd, gscale);
  } else {
    hipLaunchKernelGGL(rmsprop_kernel, grid, dim3(THREADS), 0, as_stream(stream), p, g, sq, buf, n, lr, alpha, eps, mom, wd, gscale);
  }
  return launch_status();
}

// ---- the grouped steps ----------------------------------------------------------------------------------------------------------
// begin() takes what the group row fixes: lr_g = lr * lr_mult and the group's own 1-based step t_g = t - t0.
// TRUST (cx_lars_step_items): the decayed gradient is multiplied by trust[item.tensor].r ahead of update(); `trust` is not read
// otherwise, and the TRUST = false instantiations are the kernels they were before the flag existed.
template <class Rule, bool TRUST = false>
__global__ __launch_bounds__(THREADS) void step_items_kernel(Rule r, float* __restrict__ p, const float* __restrict__ g,
                                                              const Item* __restrict__ items, int n_items,
                                                              const float* __restrict__ groups, int decoupled,
                                                              const float* __restrict__ hyper, float lr, int step, float gscale,
                                                              Tail x, const float* __restrict__ trust, uint32_t n_tensors) {
  Launch q;
  if (!begin_launch(x, hyper, lr, step, gscale, q)) return;
  f32x4* __restrict__ p4 = reinterpret_cast<f32x4*>(p);
  const f32x4* __restrict__ g4 = reinterpret_cast<const f32x4*>(g);
  f32x4* s04 = reinterpret_cast<f32x4*>(r.s0);
  f32x4* s14 = reinterpret_cast<f32x4*>(r.s1);
  f32x4* e4 = reinterpret_cast<f32x4*>(x.ema);
  const bool has_s1 = r.has_s1();
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
    const float lr_g = q.lr * lr_mult;
    r.begin(lr_g, q.t - t0);
    const float keep = 1.f - lr_g * wd;
    float ratio = 1.f;
    if constexpr (TRUST) {
      if (item.tensor >= n_tensors) continue;                        // a table that names no row of `trust`: nothing is read or written
      ratio = trust[4 * (size_t)item.tensor];
    }
    const uint32_t last = first + OG_SLOT_VEC4 < item.len4 ? first + OG_SLOT_VEC4 : item.len4;
    const size_t lo = (size_t)item.start4 + first, hi = (size_t)item.start4 + last;
    for (size_t i = lo + threadIdx.x; i < hi; i += THREADS) {
      // every load of the unit ahead of its stores
      const f32x4 gv = g4[i];
      f32x4 pv = p4[i];
      f32x4 av = s04[i];
      f32x4 bv = has_s1 ? s14[i] : f32x4{0.f, 0.f, 0.f, 0.f};
      f32x4 ev = e4 ? e4[i] : f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
      for (int c = 0; c < 4; ++c) {
        float gi = gv[c] * q.gs, pi = pv[c];
        float a = av[c], b = bv[c];
        decay(gi, pi, decoupled, wd, keep);
        if constexpr (TRUST) gi *= ratio;
        const float pn = r.update(gi, pi, a, b);
        av[c] = a;
        bv[c] = b;
        pv[c] = pn;
        ev[c] = q.d * ev[c] + q.omd * pn;
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

// CX_EINVAL / CX_EALIGN of a grouped step, before any launch (s0, s1: the rule's state pointers)
int check_step_items(const float* p, const float* g, const float* s0, const float* s1, size_t n, const uint32_t* items, int n_items,
                     const float* groups, int n_groups, const float* hyper, int step, const Tail& x) {
  if (!p || !g || !s0) return CX_EINVAL;
  if (const int e = check_tables(n, items, n_items, groups, n_groups)) return e;
  if (const int e = check_tail(hyper, step, x.ema, x.ema_decay, true)) return e;
  if (!aligned16(p) || !aligned16(g) || !aligned16(s0) || !aligned16(s1)) return CX_EALIGN;
  return 0;
}

template <class Rule>
int launch_step_items(const Rule& r, float* p, const float* g, size_t n, const uint32_t* items, int n_items, const float* groups,
                      int n_groups, int decoupled, const float* hyper, float lr, int step, float gscale, const Tail& x, void* stream) {
  if (const int e = check_step_items(p, g, r.s0, r.s1, n, items, n_items, groups, n_groups, hyper, step, x)) return e;
  if (n == 0) return 0;
  hipLaunchKernelGGL((step_items_kernel<Rule, false>), dim3(blocks_for((long long)n_items * OG_SLOTS)), dim3(THREADS), 0,
                     as_stream(stream), r, p, g, reinterpret_cast<const Item*>(items), n_items, groups, decoupled ? 1 : 0, hyper, lr,
                     step, gscale, x, (const float*)nullptr, 0u);
  return launch_status();
}

// ---- layer-wise trust ratios: LAMB and LARS -------------------------------------------------------------------------------------
// Three launches on one stream, no atomics, nothing read on the host:
//
//   1. trust_partial_kernel  one workgroup per item: part_w[item] = sum p^2, part_u[item] = sum u^2.  LARS: u is the scaled
//                            gradient g = grad_scale * clip[1] * grad.  LAMB: the Adam moments are advanced here (m, v written) and
//                            u = (m / (1 - b1^t_g)) / (sqrt(v) / sqrt(1 - b2^t_g) + eps) + wd * p is stored in a scratch buffer
//   2. trust_ratio_kernel    ONE workgroup, thread k, k + 256, ... owns tensor k: it adds the partials of the tensor's items
//                            tensor_items[k] .. tensor_items[k + 1] - 1 one by one in item order and writes
//                            trust[k] = {r, |p|, |u|, adapted}
//   3. the apply             LAMB: p -= lr_g * r * u from the STORED u (a second kernel compiling the expression of u may round it
//                            differently: the norm would then belong to another u than the one applied); LARS:
//                            step_items_kernel<SgdRule, true>
//
// Every summation tree is a function of the item table alone.  An item of a frozen group writes partials of 0 and nothing else;
// on a skipped step (begin_launch) none of the three kernels writes anything.  The zero padding of the flat layout adds 0 to both
// sums and stays 0: p = g = m = v = 0 gives u = 0 / (0 + eps) + wd * 0 = 0 (eps > 0).
struct TrustArgs {
  const uint32_t* tensor_items;     // uint32[n_tensors + 1]: the first item of every tensor, then n_items
  int n_tensors;
  float *part_w, *part_u;           // n_items floats each
  float* trust;                     // float[4] per tensor
  float coef, eps;                  // LARS
  int clip, always_adapt;
};

// the four-accumulator sums of sq_units for one 16-byte unit
__device__ __forceinline__ void sq_acc(const f32x4& v, float (&a)[4]) {
#pragma unroll
  for (int c = 0; c < 4; ++c) a[c] = fmaf(v[c], v[c], a[c]);
}

template <bool LAMB>
__global__ __launch_bounds__(THREADS) void trust_partial_kernel(AdamRule r, const float* __restrict__ p, const float* __restrict__ g,
                                                                 float* __restrict__ u, const Item* __restrict__ items, int n_items,
                                                                 const float* __restrict__ groups, const float* __restrict__ hyper,
                                                                 float lr, int step, float gscale, Tail x,
                                                                 float* __restrict__ part_w, float* __restrict__ part_u) {
  Launch q;
  if (!begin_launch(x, hyper, lr, step, gscale, q)) return;
  const f32x4* __restrict__ p4 = reinterpret_cast<const f32x4*>(p);
  const f32x4* __restrict__ g4 = reinterpret_cast<const f32x4*>(g);
  f32x4* __restrict__ m4 = reinterpret_cast<f32x4*>(r.s0);
  f32x4* __restrict__ v4 = reinterpret_cast<f32x4*>(r.s1);
  f32x4* __restrict__ u4 = reinterpret_cast<f32x4*>(u);
  for (int it = blockIdx.x; it < n_items; it += gridDim.x) {
    const Item item = items[it];
    const float* __restrict__ row = groups + 4 * (size_t)item.group;
    const float wd = row[1], frozen = row[2], t0 = row[3];
    if (frozen != 0.f) {                                             // uniform over the workgroup
      if (threadIdx.x == 0) {
        part_w[it] = 0.f;
        part_u[it] = 0.f;
      }
      continue;
    }
    // the reciprocals of the bias corrections, once per item: one division and one square root per element are left.  DenseNet121's
    // 212 whole items are fewer than the CUs, so a CU mostly runs ONE workgroup here and the launch is bound by the arithmetic of
    // its four waves, not by memory (profiles/optim_trust_bench.txt)
    float inv_bc1 = 1.f, inv_bc2_sqrt = 1.f;
    if constexpr (LAMB) {
      inv_bc1 = 1.f / (1.f - powf(r.b1, q.t - t0));
      inv_bc2_sqrt = 1.f / sqrtf(1.f - powf(r.b2, q.t - t0));
    }
    float aw[4] = {0.f, 0.f, 0.f, 0.f}, au[4] = {0.f, 0.f, 0.f, 0.f};
    const size_t lo = item.start4, hi = (size_t)item.start4 + item.len4;
#pragma unroll 2
    for (size_t i = lo + threadIdx.x; i < hi; i += THREADS) {
      // every load of the unit ahead of its stores
      f32x4 gv = g4[i];
      const f32x4 pv = p4[i];
      if constexpr (LAMB) {
        f32x4 mv = m4[i];
        f32x4 vv = v4[i];
        f32x4 uv;
#pragma unroll
        for (int c = 0; c < 4; ++c) {
          const float gi = gv[c] * q.gs;
          mv[c] = r.b1 * mv[c] + (1.f - r.b1) * gi;
          vv[c] = r.b2 * vv[c] + (1.f - r.b2) * gi * gi;
          uv[c] = (mv[c] * inv_bc1) / (sqrtf(vv[c]) * inv_bc2_sqrt + r.eps) + wd * pv[c];
        }
        m4[i] = mv;
        v4[i] = vv;
        u4[i] = uv;
        sq_acc(uv, au);
      } else {
#pragma unroll
        for (int c = 0; c < 4; ++c) gv[c] *= q.gs;
        sq_acc(gv, au);
      }
      sq_acc(pv, aw);
    }
    const float sw = block_fold((aw[0] + aw[1]) + (aw[2] + aw[3]));
    __syncthreads();
    const float su = block_fold((au[0] + au[1]) + (au[2] + au[3]));
    if (threadIdx.x == 0) {
      part_w[it] = sw;
      part_u[it] = su;
    }
    __syncthreads();
  }
}

template <bool LAMB>
__global__ __launch_bounds__(THREADS) void trust_ratio_kernel(const Item* __restrict__ items, int n_items,
                                                               const float* __restrict__ groups, int n_groups, Tail x, TrustArgs a) {
  if (x.clip && x.skip_nonfinite && x.clip[2] != 0.f) return;       // begin_launch's test: a skipped step writes nothing
  for (int k = threadIdx.x; k < a.n_tensors; k += THREADS) {
    uint32_t first = a.tensor_items[k], last = a.tensor_items[k + 1];
    if (last > (uint32_t)n_items) last = (uint32_t)n_items;
    float sw = 0.f, su = 0.f;
    for (uint32_t it = first; it < last; ++it) {
      sw += a.part_w[it];
      su += a.part_u[it];
    }
    const float wn = sqrtf(sw), un = sqrtf(su);
    float ratio = 1.f, adapted = 0.f;
    if (first < last) {
      const uint32_t grp = items[first].group;
      const float wd = grp < (uint32_t)n_groups ? groups[4 * (size_t)grp + 1] : 0.f;
      const bool frozen = grp < (uint32_t)n_groups && groups[4 * (size_t)grp + 2] != 0.f;
      if (!frozen && (wd != 0.f || a.always_adapt)) {
        adapted = 1.f;
        if (wn > 0.f && un > 0.f) {
          ratio = LAMB ? wn / un : a.coef * wn / (un + wd * wn + a.eps);
          if (a.clip) ratio = fminf(ratio, 1.f);
        }
      }
    }
    float* __restrict__ out = a.trust + 4 * (size_t)k;
    out[0] = ratio;
    out[1] = wn;
    out[2] = un;
    out[3] = adapted;
  }
}

// The LAMB apply: step_items_kernel's slots over p, the stored u and the EMA.
__global__ __launch_bounds__(THREADS) void lamb_apply_kernel(float* __restrict__ p, const float* __restrict__ u,
                                                              const Item* __restrict__ items, int n_items,
                                                              const float* __restrict__ groups, const float* __restrict__ hyper,
                                                              float lr, int step, float gscale, Tail x,
                                                              const float* __restrict__ trust, uint32_t n_tensors) {
  Launch q;
  if (!begin_launch(x, hyper, lr, step, gscale, q)) return;
  f32x4* __restrict__ p4 = reinterpret_cast<f32x4*>(p);
  const f32x4* __restrict__ u4 = reinterpret_cast<const f32x4*>(u);
  f32x4* e4 = reinterpret_cast<f32x4*>(x.ema);
  for (long long s = blockIdx.x; s < (long long)n_items * OG_SLOTS; s += gridDim.x) {
    const Item item = items[s % n_items];
    const uint32_t first = (uint32_t)(s / n_items) * OG_SLOT_VEC4;
    if (first >= item.len4 || item.tensor >= n_tensors) continue;
    const float* __restrict__ row = groups + 4 * (size_t)item.group;
    if (row[2] != 0.f) continue;                                     // frozen: uniform over the workgroup
    const float scale = q.lr * row[0] * trust[4 * (size_t)item.tensor];
    const uint32_t last = first + OG_SLOT_VEC4 < item.len4 ? first + OG_SLOT_VEC4 : item.len4;
    const size_t lo = (size_t)item.start4 + first, hi = (size_t)item.start4 + last;
    for (size_t i = lo + threadIdx.x; i < hi; i += THREADS) {
      const f32x4 uv = u4[i];
      f32x4 pv = p4[i];
      f32x4 ev = e4 ? e4[i] : f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
      for (int c = 0; c < 4; ++c) {
        pv[c] = pv[c] - scale * uv[c];
        ev[c] = q.d * ev[c] + q.omd * pv[c];
      }
      p4[i] = pv;
      if (e4) e4[i] = ev;
    }
  }
}

int check_trust(const TrustArgs& a, size_t n, bool lars) {
  if (!a.tensor_items || a.n_tensors < 1 || !a.trust) return CX_EINVAL;
  if (n && (!a.part_w || !a.part_u)) return CX_EINVAL;
  if (lars ? !(a.coef > 0.f && a.eps >= 0.f) : !(a.eps > 0.f)) return CX_EINVAL;
  return 0;
}

// ---- sharpness-aware minimisation: SAM and ASAM around any of the steps above ---------------------------------------------------
// The ascent step p <- p + rho * s^2 g / |s g| of Foret et al. (s = 1) and Kwon et al. (s = |p|, elementwise), g = grad_scale * grad,
// over the item table and the group rows of the grouped steps.  Nothing is read on the host and rho lives in device memory, so a
// captured step replays all of it under a rho schedule:
//
//   cx_sam_norm_items     launch 1: one partial per item of sum (g s)^2, summed and folded as item_sq_partial_kernel sums an item; an
//                         item of a frozen group is not read and gets the partial 0.  Launch 2, ONE workgroup: thread t adds the
//                         partials [t * per, (t + 1) * per) in item order (per = ceil(n_items / 256)), the 256 sums are folded as
//                         everywhere here, and thread 0 writes sam[4] = {norm, scale = rho / (norm + eps), nonfinite, 0}.  The tree is
//                         a function of the item table alone: a frozen item adds +0 (exact), the group is otherwise only a label
//   cx_sam_perturb_items  backup = p, p = p + scale * s^2 * g over the slots of the unfrozen items; nothing when sam[2] != 0
//   cx_sam_restore_items  p = backup over the same slots (a copy: the weights come back with their own bits); nothing when sam[2] != 0
//
// The tables live in device memory, so the host cannot see them: every kernel skips an item whose units end past n / 4 or whose
// group is >= n_groups (no byte read or written), and a caller that passes a host copy of the table has it checked before any launch.
__device__ __forceinline__ bool sam_item_ok(const Item& item, size_t n4, int n_groups) {
  return (size_t)item.start4 + item.len4 <= n4 && item.group < (uint32_t)n_groups;
}

template <bool ADAPTIVE>
__global__ __launch_bounds__(THREADS) void sam_sq_partial_kernel(const float* __restrict__ p, const float* __restrict__ g, size_t n4,
                                                                  const Item* __restrict__ items, int n_items,
                                                                  const float* __restrict__ groups, int n_groups, float gscale,
                                                                  float* __restrict__ part) {
  const f32x4* __restrict__ p4 = reinterpret_cast<const f32x4*>(p);
  const f32x4* __restrict__ g4 = reinterpret_cast<const f32x4*>(g);
  for (int it = blockIdx.x; it < n_items; it += gridDim.x) {
    const Item item = items[it];
    if (!sam_item_ok(item, n4, n_groups) || groups[4 * (size_t)item.group + 2] != 0.f) {      // uniform over the workgroup
      if (threadIdx.x == 0) part[it] = 0.f;
      continue;
    }
    float a[4] = {0.f, 0.f, 0.f, 0.f};
    const size_t lo = item.start4, hi = (size_t)item.start4 + item.len4;
#pragma unroll 4
    for (size_t i = lo + threadIdx.x; i < hi; i += THREADS) {
      f32x4 gv = g4[i];
      if constexpr (ADAPTIVE) {
        const f32x4 pv = p4[i];
#pragma unroll
        for (int c = 0; c < 4; ++c) gv[c] = gv[c] * gscale * fabsf(pv[c]);
      } else {
#pragma unroll
        for (int c = 0; c < 4; ++c) gv[c] *= gscale;
      }
      sq_acc(gv, a);
    }
    const float s = block_fold((a[0] + a[1]) + (a[2] + a[3]));
    if (threadIdx.x == 0) part[it] = s;
    __syncthreads();
  }
}

__global__ __launch_bounds__(THREADS) void sam_norm_final_kernel(const float* __restrict__ part, int n_items,
                                                                  const float* __restrict__ rho_eps, float* __restrict__ sam) {
  const int per = (n_items + THREADS - 1) / THREADS;
  const int lo = threadIdx.x * per;
  const int hi = lo + per < n_items ? lo + per : n_items;
  float acc = 0.f;
  for (int i = lo; i < hi; ++i) acc += part[i];
  const float sum = block_fold(acc);
  if (threadIdx.x != 0) return;
  const float norm = sqrtf(sum);
  sam[0] = norm;
  sam[1] = rho_eps[0] / (norm + rho_eps[1]);
  sam[2] = !(sum < INFINITY) ? 1.f : 0.f;                   // inf or NaN (the sum of squares is never negative)
  sam[3] = 0.f;
}

// step_items_kernel's slots over p, g and the backup.  RESTORE: p = backup, g is not read.
template <bool ADAPTIVE, bool RESTORE>
__global__ __launch_bounds__(THREADS) void sam_move_kernel(float* __restrict__ p, const float* __restrict__ g, float* __restrict__ backup,
                                                            size_t n4, const Item* __restrict__ items, int n_items,
                                                            const float* __restrict__ groups, int n_groups,
                                                            const float* __restrict__ sam, float gscale) {
  if (sam[2] != 0.f) return;                                 // the whole grid takes the same side: nothing is written
  const float scale = sam[1];
  f32x4* __restrict__ p4 = reinterpret_cast<f32x4*>(p);
  const f32x4* __restrict__ g4 = reinterpret_cast<const f32x4*>(g);
  f32x4* __restrict__ b4 = reinterpret_cast<f32x4*>(backup);
  for (long long s = blockIdx.x; s < (long long)n_items * OG_SLOTS; s += gridDim.x) {
    const Item item = items[s % n_items];
    const uint32_t first = (uint32_t)(s / n_items) * OG_SLOT_VEC4;
    if (first >= item.len4 || !sam_item_ok(item, n4, n_groups)) continue;
    if (groups[4 * (size_t)item.group + 2] != 0.f) continue;          // frozen: uniform over the workgroup
    const uint32_t last = first + OG_SLOT_VEC4 < item.len4 ? first + OG_SLOT_VEC4 : item.len4;
    const size_t lo = (size_t)item.start4 + first, hi = (size_t)item.start4 + last;
#pragma unroll 2
    for (size_t i = lo + threadIdx.x; i < hi; i += THREADS) {
      if constexpr (RESTORE) {
        p4[i] = b4[i];
      } else {
        const f32x4 gv = g4[i];
        f32x4 pv = p4[i];
        b4[i] = pv;
#pragma unroll
        for (int c = 0; c < 4; ++c) {
          const float e = ADAPTIVE ? (pv[c] * pv[c]) * (gv[c] * gscale) : gv[c] * gscale;
          pv[c] = pv[c] + scale * e;
        }
        p4[i] = pv;
      }
    }
  }
}

// CX_EINVAL / CX_EALIGN of the three SAM entry points, before any launch.  items_host (may be null): a host copy of the table
int check_sam(size_t n, const uint32_t* items, const uint32_t* items_host, int n_items, const float* groups, int n_groups) {
  if (const int e = check_tables(n, items, n_items, groups, n_groups)) return e;
  if (items_host) {
    const size_t n4 = n >> 2;
    for (int it = 0; it < n_items; ++it) {
      const uint32_t* q = items_host + 4 * (size_t)it;
      if ((size_t)q[0] + q[1] > n4 || q[2] >= (uint32_t)n_groups) return CX_EINVAL;
    }
  }
  return 0;
}

// ---- cx_optim_tick applies the reference's schedulers (chexpert.py:165: stepped once per minibatch from lr_warmup_steps on; :480
// MultiStepLR, :500 ExponentialLR)
__global__ void optim_tick_kernel(float* hyper) {
  if (threadIdx.x != 0 || blockIdx.x != 0) return;
  const float step = hyper[1] + 1.f;
  hyper[1] = step;
  const int kind = (int)hyper[2];
  // chexpert.py:157-165: `args.step += 1` opens the minibatch, `if scheduler and args.step >= args.lr_warmup_steps:
  // scheduler.step()` closes it -> after minibatch number `step` the scheduler has been stepped k times
  const float warm = hyper[4];
  if (step < warm) return;
  const float k = step - fmaxf(warm, 1.f) + 1.f;
  if (kind == 1) hyper[0] *= hyper[3];                                                   // ExponentialLR
  if (kind == 2) hyper[0] = hyper[7] * powf(hyper[3], (k >= hyper[5] ? 1.f : 0.f) + (k >= hyper[6] ? 1.f : 0.f));   // MultiStepLR
}

}  // namespace


extern "C" {

int cx_optim_tick(float* hyper, void* stream) {
  if (!hyper) return CX_EINVAL;
  hipLaunchKernelGGL(optim_tick_kernel, dim3(1), dim3(64), 0, as_stream(stream), hyper);
  return launch_status();
}

int cx_grad_norm_partials(size_t n) { return gn_blocks(n); }

int cx_grad_norm(const float* g, size_t n, float grad_scale, float max_norm, int skip_nonfinite, float* workspace,
                 size_t workspace_floats, float* clip, void* stream) {
  if (!clip || (n && (!g || !workspace))) return CX_EINVAL;
  const int blocks = gn_blocks(n);
  if (workspace_floats < (size_t)blocks) return CX_EINVAL;
  if (n && !aligned16(g)) return CX_EALIGN;
  if (blocks)
    hipLaunchKernelGGL(grad_sq_partial_kernel, dim3(blocks), dim3(THREADS), 0, as_stream(stream), g, n, grad_scale, workspace);
  hipLaunchKernelGGL(grad_norm_final_kernel, dim3(1), dim3(THREADS), 0, as_stream(stream), workspace, blocks, max_norm, skip_nonfinite,
                     clip);
  return launch_status();
}

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
    hipLaunchKernelGGL(item_sq_partial_kernel, dim3(blocks_for(n_items)), dim3(THREADS), 0, as_stream(stream), g, tab, n_items, grad_scale,
                       partials);
  hipLaunchKernelGGL(group_norm_final_kernel, dim3(1), dim3(THREADS), 0, as_stream(stream), partials, tab, n_items, groups, n_groups,
                     max_norm, skip_nonfinite, group_sq, group_norm, clip);
  return launch_status();
}

// ---- Adam.  The host-lr form takes its bias corrections from the host's powf.
int cx_adam_step_ex(float* p, const float* g, float* m, float* v, size_t n, float lr, float beta1, float beta2, float eps,
                    float weight_decay, int step, float grad_scale, const float* clip, float* ema, float ema_decay, int ema_warmup,
                    int skip_nonfinite, void* stream) {
  if (!p || !g || !m || !v || step < 1) return CX_EINVAL;
  const float bc1 = 1.f - powf(beta1, (float)step);
  const float bc2s = sqrtf(1.f - powf(beta2, (float)step));
  const AdamRule r = {m, v, beta1, beta2, eps, bc1, bc2s, true, 0.f};
  return launch_step(r, p, g, n, nullptr, lr, step, weight_decay, grad_scale, {clip, ema, ema_decay, ema_warmup, skip_nonfinite}, stream);
}

int cx_adam_step(float* p, const float* g, float* m, float* v, size_t n, float lr, float beta1, float beta2, float eps,
                 float weight_decay, int step, float grad_scale, void* stream) {
  return cx_adam_step_ex(p, g, m, v, n, lr, beta1, beta2, eps, weight_decay, step, grad_scale, nullptr, nullptr, 0.f, 0, 0, stream);
}

int cx_adam_step_dev_ex(float* p, const float* g, float* m, float* v, size_t n, const float* hyper, float beta1, float beta2,
                        float eps, float weight_decay, float grad_scale, const float* clip, float* ema, float ema_decay,
                        int ema_warmup, int skip_nonfinite, void* stream) {
  if (!p || !g || !m || !v || !hyper) return CX_EINVAL;
  const AdamRule r = {m, v, beta1, beta2, eps, 1.f, 1.f, false, 0.f};
  return launch_step(r, p, g, n, hyper, 0.f, 0, weight_decay, grad_scale, {clip, ema, ema_decay, ema_warmup, skip_nonfinite}, stream);
}

int cx_adam_step_dev(float* p, const float* g, float* m, float* v, size_t n, const float* hyper, float beta1, float beta2, float eps,
                     float weight_decay, float grad_scale, void* stream) {
  return cx_adam_step_dev_ex(p, g, m, v, n, hyper, beta1, beta2, eps, weight_decay, grad_scale, nullptr, nullptr, 0.f, 0, 0, stream);
}

int cx_adam_step_items(float* p, const float* g, float* m, float* v, size_t n, const uint32_t* items, int n_items, const float* groups,
                       int n_groups, int decoupled, const float* hyper, float lr, int step, float beta1, float beta2, float eps,
                       float grad_scale, const float* clip, float* ema, float ema_decay, int ema_warmup, int skip_nonfinite,
                       void* stream) {
  if (!v) return CX_EINVAL;
  const AdamRule r = {m, v, beta1, beta2, eps, 1.f, 1.f, false, 0.f};
  return launch_step_items(r, p, g, n, items, n_items, groups, n_groups, decoupled, hyper, lr, step, grad_scale,
                           {clip, ema, ema_decay, ema_warmup, skip_nonfinite}, stream);
}

// ---- SGD with Nesterov momentum
int cx_sgd_nesterov_step_ex(float* p, const float* g, float* buf, size_t n, float lr, float momentum, float weight_decay,
                            int first_step, int step, float grad_scale, const float* clip, float* ema, float ema_decay,
                            int ema_warmup, int skip_nonfinite, void* stream) {
  if (!p || !g || !buf) return CX_EINVAL;
  const SgdRule r = {buf, nullptr, momentum, first_step ? 1 : 0, 0.f};
  return launch_step(r, p, g, n, nullptr, lr, step, weight_decay, grad_scale, {clip, ema, ema_decay, ema_warmup, skip_nonfinite}, stream);
}

int cx_sgd_nesterov_step(float* p, const float* g, float* buf, size_t n, float lr, float momentum, float weight_decay,
                         int first_step, float grad_scale, void* stream) {
  return cx_sgd_nesterov_step_ex(p, g, buf, n, lr, momentum, weight_decay, first_step, 0, grad_scale, nullptr, nullptr, 0.f, 0, 0, stream);
}

int cx_sgd_nesterov_step_dev_ex(float* p, const float* g, float* buf, size_t n, const float* hyper, float momentum,
                                float weight_decay, float grad_scale, const float* clip, float* ema, float ema_decay, int ema_warmup,
                                int skip_nonfinite, void* stream) {
  if (!p || !g || !buf || !hyper) return CX_EINVAL;
  const SgdRule r = {buf, nullptr, momentum, -1, 0.f};
  return launch_step(r, p, g, n, hyper, 0.f, 0, weight_decay, grad_scale, {clip, ema, ema_decay, ema_warmup, skip_nonfinite}, stream);
}

int cx_sgd_nesterov_step_dev(float* p, const float* g, float* buf, size_t n, const float* hyper, float momentum, float weight_decay,
                             float grad_scale, void* stream) {
  return cx_sgd_nesterov_step_dev_ex(p, g, buf, n, hyper, momentum, weight_decay, grad_scale, nullptr, nullptr, 0.f, 0, 0, stream);
}

int cx_sgd_nesterov_step_items(float* p, const float* g, float* buf, size_t n, const uint32_t* items, int n_items, const float* groups,
                               int n_groups, int decoupled, const float* hyper, float lr, int step, float momentum, float grad_scale,
                               const float* clip, float* ema, float ema_decay, int ema_warmup, int skip_nonfinite, void* stream) {
  const SgdRule r = {buf, nullptr, momentum, 0, 0.f};
  return launch_step_items(r, p, g, n, items, n_items, groups, n_groups, decoupled, hyper, lr, step, grad_scale,
                           {clip, ema, ema_decay, ema_warmup, skip_nonfinite}, stream);
}

// ---- LAMB and LARS: the grouped Adam / SGD argument lists plus the trust tables.  Everything is validated before the first of the
// three launches.  `decoupled` is refused: LAMB's decay already sits outside the moments, LARS's is part of the ratio.
int cx_lamb_step_items(float* p, const float* g, float* m, float* v, size_t n, const uint32_t* items, int n_items, const float* groups,
                       int n_groups, int decoupled, const float* hyper, float lr, int step, float beta1, float beta2, float eps,
                       float grad_scale, const float* clip, float* ema, float ema_decay, int ema_warmup, int skip_nonfinite,
                       const uint32_t* tensor_items, int n_tensors, float* part_w, float* part_u, float* trust, float* u,
                       int trust_clip, int always_adapt, void* stream) {
  if (!v || decoupled || (n && !u)) return CX_EINVAL;
  const Tail x = {clip, ema, ema_decay, ema_warmup, skip_nonfinite};
  const TrustArgs a = {tensor_items, n_tensors, part_w, part_u, trust, 0.f, eps, trust_clip ? 1 : 0, always_adapt ? 1 : 0};
  if (const int e = check_step_items(p, g, m, v, n, items, n_items, groups, n_groups, hyper, step, x)) return e;
  if (const int e = check_trust(a, n, false)) return e;
  if (!aligned16(u)) return CX_EALIGN;
  if (n == 0) return 0;
  const AdamRule r = {m, v, beta1, beta2, eps, 1.f, 1.f, false, 0.f};
  const Item* tab = reinterpret_cast<const Item*>(items);
  hipLaunchKernelGGL(trust_partial_kernel<true>, dim3(blocks_for(n_items)), dim3(THREADS), 0, as_stream(stream), r, p, g, u, tab, n_items,
                     groups, hyper, lr, step, grad_scale, x, part_w, part_u);
  hipLaunchKernelGGL(trust_ratio_kernel<true>, dim3(1), dim3(THREADS), 0, as_stream(stream), tab, n_items, groups, n_groups, x, a);
  hipLaunchKernelGGL(lamb_apply_kernel, dim3(blocks_for((long long)n_items * OG_SLOTS)), dim3(THREADS), 0, as_stream(stream), p, u, tab,
                     n_items, groups, hyper, lr, step, grad_scale, x, trust, (uint32_t)n_tensors);
  return launch_status();
}

int cx_lars_step_items(float* p, const float* g, float* buf, size_t n, const uint32_t* items, int n_items, const float* groups,
                       int n_groups, int decoupled, const float* hyper, float lr, int step, float momentum, float grad_scale,
                       const float* clip, float* ema, float ema_decay, int ema_warmup, int skip_nonfinite,
                       const uint32_t* tensor_items, int n_tensors, float* part_w, float* part_u, float* trust, float coef, float eps,
                       int trust_clip, int always_adapt, void* stream) {
  if (decoupled) return CX_EINVAL;
  const Tail x = {clip, ema, ema_decay, ema_warmup, skip_nonfinite};
  const TrustArgs a = {tensor_items, n_tensors, part_w, part_u, trust, coef, eps, trust_clip ? 1 : 0, always_adapt ? 1 : 0};
  if (const int e = check_step_items(p, g, buf, nullptr, n, items, n_items, groups, n_groups, hyper, step, x)) return e;
  if (const int e = check_trust(a, n, true)) return e;
  if (n == 0) return 0;
  const SgdRule r = {buf, nullptr, momentum, 0, 0.f};
  const AdamRule none = {nullptr, nullptr, 0.f, 0.f, 0.f, 1.f, 1.f, false, 0.f};
  const Item* tab = reinterpret_cast<const Item*>(items);
  hipLaunchKernelGGL(trust_partial_kernel<false>, dim3(blocks_for(n_items)), dim3(THREADS), 0, as_stream(stream), none, p, g,
                     (float*)nullptr, tab, n_items, groups, hyper, lr, step, grad_scale, x, part_w, part_u);
  hipLaunchKernelGGL(trust_ratio_kernel<false>, dim3(1), dim3(THREADS), 0, as_stream(stream), tab, n_items, groups, n_groups, x, a);
  hipLaunchKernelGGL((step_items_kernel<SgdRule, true>), dim3(blocks_for((long long)n_items * OG_SLOTS)), dim3(THREADS), 0,
                     as_stream(stream), r, p, g, tab, n_items, groups, 0, hyper, lr, step, grad_scale, x, (const float*)trust,
                     (uint32_t)n_tensors);
  return launch_status();
}

// ---- SAM / ASAM.  Everything is validated before the first launch; p of the norm may be null when adaptive == 0 (it is not read).
int cx_sam_norm_items(const float* p, const float* g, size_t n, const uint32_t* items, const uint32_t* items_host, int n_items,
                      const float* groups, int n_groups, const float* rho_eps, float grad_scale, int adaptive, float* partials,
                      float* sam, void* stream) {
  if (!sam || !rho_eps || (n && (!g || !partials || (adaptive && !p)))) return CX_EINVAL;
  if (const int e = check_sam(n, items, items_host, n_items, groups, n_groups)) return e;
  if (n && (!aligned16(g) || (adaptive && !aligned16(p)))) return CX_EALIGN;
  const Item* tab = reinterpret_cast<const Item*>(items);
  if (n == 0) n_items = 0;
  if (n_items) {
    const dim3 grid(blocks_for(n_items));
    if (adaptive)
      hipLaunchKernelGGL(sam_sq_partial_kernel<true>, grid, dim3(THREADS), 0, as_stream(stream), p, g, n >> 2, tab, n_items, groups,
                         n_groups, grad_scale, partials);
    else
      hipLaunchKernelGGL(sam_sq_partial_kernel<false>, grid, dim3(THREADS), 0, as_stream(stream), p, g, n >> 2, tab, n_items, groups,
                         n_groups, grad_scale, partials);
  }
  hipLaunchKernelGGL(sam_norm_final_kernel, dim3(1), dim3(THREADS), 0, as_stream(stream), partials, n_items, rho_eps, sam);
  return launch_status();
}

int cx_sam_perturb_items(float* p, const float* g, float* backup, size_t n, const uint32_t* items, const uint32_t* items_host,
                         int n_items, const float* groups, int n_groups, const float* sam, float grad_scale, int adaptive,
                         void* stream) {
  if (!p || !g || !backup || !sam) return CX_EINVAL;
  if (const int e = check_sam(n, items, items_host, n_items, groups, n_groups)) return e;
  if (!aligned16(p) || !aligned16(g) || !aligned16(backup)) return CX_EALIGN;
  if (n == 0) return 0;
  const Item* tab = reinterpret_cast<const Item*>(items);
  const dim3 grid(blocks_for((long long)n_items * OG_SLOTS));
  if (adaptive)
    hipLaunchKernelGGL((sam_move_kernel<true, false>), grid, dim3(THREADS), 0, as_stream(stream), p, g, backup, n >> 2, tab, n_items,
                       groups, n_groups, sam, grad_scale);
  else
    hipLaunchKernelGGL((sam_move_kernel<false, false>), grid, dim3(THREADS), 0, as_stream(stream), p, g, backup, n >> 2, tab, n_items,
                       groups, n_groups, sam, grad_scale);
  return launch_status();
}

int cx_sam_restore_items(float* p, const float* backup, size_t n, const uint32_t* items, const uint32_t* items_host, int n_items,
                         const float* groups, int n_groups, const float* sam, void* stream) {
  if (!p || !backup || !sam) return CX_EINVAL;
  if (const int e = check_sam(n, items, items_host, n_items, groups, n_groups)) return e;
  if (!aligned16(p) || !aligned16(backup)) return CX_EALIGN;
  if (n == 0) return 0;
  hipLaunchKernelGGL((sam_move_kernel<false, true>), dim3(blocks_for((long long)n_items * OG_SLOTS)), dim3(THREADS), 0,
                     as_stream(stream), p, (const float*)nullptr, const_cast<float*>(backup), n >> 2,
                     reinterpret_cast<const Item*>(items), n_items, groups, n_groups, sam, 0.f);
  return launch_status();
}

// ---- RMSprop.  momentum == 0: buf is never touched and may be null.
int cx_rmsprop_step_ex(float* p, const float* g, float* sq, float* buf, size_t n, float lr, float alpha, float eps, float momentum,
                       float weight_decay, int step, float grad_scale, const float* clip, float* ema, float ema_decay,
                       int ema_warmup, int skip_nonfinite, void* stream) {
  if (!p || !g || !sq || (momentum > 0.f && !buf)) return CX_EINVAL;
  return launch_rmsprop(p, g, sq, buf, n, nullptr, lr, step, alpha, eps, momentum, weight_decay, grad_scale,
                        {clip, ema, ema_decay, ema_warmup, skip_nonfinite}, stream);
}

int cx_rmsprop_step(float* p, const float* g, float* sq, float* buf, size_t n, float lr, float alpha, float eps, float momentum,
                    float weight_decay, float grad_scale, void* stream) {
  return cx_rmsprop_step_ex(p, g, sq, buf, n, lr, alpha, eps, momentum, weight_decay, 0, grad_scale, nullptr, nullptr, 0.f, 0, 0, stream);
}

int cx_rmsprop_step_dev_ex(float* p, const float* g, float* sq, float* buf, size_t n, const float* hyper, float alpha, float eps,
                           float momentum, float weight_decay, float grad_scale, const float* clip, float* ema, float ema_decay,
                           int ema_warmup, int skip_nonfinite, void* stream) {
  if (!p || !g || !sq || !hyper || (momentum > 0.f && !buf)) return CX_EINVAL;
  return launch_rmsprop(p, g, sq, buf, n, hyper, 0.f, 0, alpha, eps, momentum, weight_decay, grad_scale,
                        {clip, ema, ema_decay, ema_warmup, skip_nonfinite}, stream);
}

int cx_rmsprop_step_dev(float* p, const float* g, float* sq, float* buf, size_t n, const float* hyper, float alpha, float eps,
                        float momentum, float weight_decay, float grad_scale, void* stream) {
  return cx_rmsprop_step_dev_ex(p, g, sq, buf, n, hyper, alpha, eps, momentum, weight_decay, grad_scale, nullptr, nullptr, 0.f, 0, 0, stream);
}

int cx_rmsprop_step_items(float* p, const float* g, float* sq, float* buf, size_t n, const uint32_t* items, int n_items,
                          const float* groups, int n_groups, int decoupled, const float* hyper, float lr, int step, float alpha, float eps,
                          float momentum, float grad_scale, const float* clip, float* ema, float ema_decay, int ema_warmup,
                          int skip_nonfinite, void* stream) {
  if (momentum > 0.f && !buf) return CX_EINVAL;
  const RmsRule r = {sq, buf, alpha, eps, momentum, 0.f};
  return launch_step_items(r, p, g, n, items, n_items, groups, n_groups, decoupled, hyper, lr, step, grad_scale,
                           {clip, ema, ema_decay, ema_warmup, skip_nonfinite}, stream);
}

}  // extern "C"
