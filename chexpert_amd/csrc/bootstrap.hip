// Non-parametric bootstrap of the AUROC on the GPU (include/chexpert_hip.h, cx_boot_counts / cx_boot_auc; chexpert_amd/metrics.py states
// both in numpy and the tests hold the kernels to that statement bit for bit).  Everything is integer arithmetic:
//   counts[b][u] = number of the U draws of replicate b that hit unit u, draw j of replicate b being the splitmix64 hash of
//                  (seed, b * U + j) scaled to [0, U) by a multiply-shift
//   num2[b][c]   = S(hi order) + S(lo order),  S = sum_t p_t * (sum_{t' < t} q_t'),  p / q = the weight counts[b][unit] of entry t where
//                  the entry is a positive / a negative: twice the numerator of the weighted trapezoid AUROC, ties counted half
// Two entry points, one per stage, so that each can be held on its own and a paired comparison can run two plans over one table.
// A third, cx_boot_sweep, reads the same table for the metrics that need the whole threshold sweep (average precision, sensitivity at
// a required specificity and the reverse); its definitions and its own header comment are further down, above boot_sweep_kernel.
// What is read how often: the order arrays (8 B per kept row and class) once per replicate, coalesced, L2-resident after the first
// replicates (20 000 rows x 14 classes: 2.2 MB); the count row of the replicate (4 U bytes) gathered 2 C times, from L1 / L2; the table
// itself is written once and read from L2 or HBM once per (class, order) -- it is the one operand of any size, which is why the host
// caps it (metrics.bootstrap_auc: 256 MB per chunk of replicates).
// Bounds: the hash (about 20 64-bit integer operations per draw) bounds the counts stage; the scan stage is bound by the gather and the
// six cross-lane adds per 64 entries, not by bytes.  Measured at 20 000 rows x 14 classes x 2000 replicates:
// counts 104 us, scan 4.3 ms; at 234 x 5 x 1000: 9 us and 35 us (launch latency).
// Same bits every run: the only unordered operation is the integer add of the counts stage (LDS atomics, or device-memory atomics for
// very large U), and integer adds commute -- the project's rule is about the order of FLOAT sums, of which this file has none.  Every
// output element of the scan stage has exactly one writer.
#include "resample.h"

namespace {

constexpr int BOOT_TILE = CX_BOOT_TILE;            // units per workgroup of the LDS form: 32 KB of counters, 4 workgroups per CU
constexpr int BOOT_MAX_TILES = CX_BOOT_MAX_TILES;  // more tiles than this per replicate: the device-memory form (a tile re-hashes all U draws)
constexpr int BOOT_MAX_U = CX_BOOT_MAX_UNITS;

__device__ __forceinline__ uint32_t boot_draw(const uint64_t seed, const uint64_t k, const uint32_t U) {
  uint64_t z = seed + 0x9E3779B97F4A7C15ull * (k + 1ull);
  z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
  z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
  z ^= z >> 31;
  return __umulhi((uint32_t)(z >> 32), U);                   // in [0, U)
}

// ---- stage 1, LDS form: one workgroup per (replicate, tile of BOOT_TILE units) -------------------------------------------------------
// The tile's counters live in LDS; all 256 threads hash the U draws of the replicate (thread t the draws t, t + 256, ...) and add the
// hits that fall inside the tile; the tile is then stored with plain dword stores.  U <= BOOT_TILE is one workgroup per replicate and
// every draw is hashed once; above it every tile hashes all the draws again, which the host side bounds at BOOT_MAX_TILES.
__global__ __launch_bounds__(256) void boot_counts_lds_kernel(uint32_t* __restrict__ counts, int ld, int U, int first, int tiles,
                                                              uint64_t seed) {
  __shared__ uint32_t cnt[BOOT_TILE];
  const int tid = threadIdx.x;
  const int rep = blockIdx.x / tiles, tile = blockIdx.x - rep * tiles;
  const int u0 = tile * BOOT_TILE, nu = min(BOOT_TILE, U - u0);                // nu >= 1
  for (int u = tid; u < nu; u += 256) cnt[u] = 0u;
  __syncthreads();
  const uint64_t k0 = (uint64_t)(first + rep) * (uint64_t)U;
  for (int j = tid; j < U; j += 256) {
    const uint32_t u = boot_draw(seed, k0 + (uint64_t)j, (uint32_t)U) - (uint32_t)u0;      // wraps below the tile: then >= nu as well
    if (u < (uint32_t)nu) atomicAdd(&cnt[u], 1u);
  }
  __syncthreads();
  uint32_t* row = counts + (size_t)rep * ld + u0;
  for (int u = tid; u < nu; u += 256) row[u] = cnt[u];
}

// ---- stage 1, device-memory form (U > BOOT_MAX_TILES * BOOT_TILE): the rows are zeroed by a first launch, then every draw is hashed
// once and added where it lands (integer atomics execute in L2).
__global__ __launch_bounds__(256) void boot_zero_kernel(uint32_t* __restrict__ counts, int ld, int U, int chunks) {
  const int rep = blockIdx.x / chunks, chunk = blockIdx.x - rep * chunks;
  const int u = chunk * 256 + threadIdx.x;
  if (u < U) counts[(size_t)rep * ld + u] = 0u;
}

__global__ __launch_bounds__(256) void boot_counts_global_kernel(uint32_t* __restrict__ counts, int ld, int U, int first, int chunks,
                                                                 uint64_t seed) {
  const int rep = blockIdx.x / chunks, chunk = blockIdx.x - rep * chunks;
  const int j = chunk * 256 + threadIdx.x;
  if (j >= U) return;
  const uint32_t u = boot_draw(seed, (uint64_t)(first + rep) * (uint64_t)U + (uint64_t)j, (uint32_t)U);      // < U <= ld
  atomicAdd(&counts[(size_t)rep * ld + u], 1u);
}

// ---- stage 2: one wave per (replicate, class), both orders side by side ---------------------------------------------------------------
// A step is 64 entries of each order, one per lane, read coalesced; BOOT_STEPS steps' entries and the count-row gathers behind them
// are requested before the first scan consumes any.  Per step and order: an inclusive wave scan of q in uint32 (wave_scan_add of
// resample.h), the exclusive prefix plus the running carry times p added to the lane's uint64 sum, and the carry advanced by the
// step's total (lane 63, wave-uniform).  The two orders are independent chains, which is what lets one wave own the output element:
// one writer, no LDS, no barrier.
constexpr int BOOT_STEPS = 4;

__global__ __launch_bounds__(256) void boot_auc_kernel(const uint32_t* __restrict__ counts, int ld, int n_rep,
                                                       const int32_t* __restrict__ order, const ClassLists plan, int c0, int cn, int C,
                                                       uint64_t* __restrict__ num2, uint32_t* __restrict__ wpos,
                                                       uint32_t* __restrict__ wneg, int U) {
  const int lane = threadIdx.x & 63;
  const long long item = (long long)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (item >= (long long)n_rep * cn) return;                     // the same for all lanes of a wave; no barrier follows
  const int rep = (int)(item / cn), cl = (int)(item - (long long)rep * cn);
  const int n = plan.len[cl];
  const int32_t* __restrict__ hi = order + plan.offs[cl];
  const int32_t* __restrict__ lo = hi + n;
  const uint32_t* __restrict__ row = counts + (size_t)rep * ld;
  uint64_t acc = 0;
  uint32_t carry_hi = 0, carry_lo = 0, sp = 0;                   // carries: negative weight before this step; sp: positive weight, per lane
  for (int t0 = 0; t0 < n; t0 += 64 * BOOT_STEPS) {
    int32_t eh[BOOT_STEPS], el[BOOT_STEPS];
#pragma unroll
    for (int s = 0; s < BOOT_STEPS; ++s) {
      const int t = t0 + s * 64 + lane;
      const int tc = min(t, n - 1);                              // past the end: the last entry again (in bounds), dropped below
      eh[s] = hi[tc], el[s] = lo[tc];
    }
    uint32_t wh[BOOT_STEPS], wl[BOOT_STEPS];
#pragma unroll
    for (int s = 0; s < BOOT_STEPS; ++s) {                       // unit indices are clamped, never trusted
      wh[s] = row[min(eh[s] & 0x7fffffff, U - 1)];
      wl[s] = row[min(el[s] & 0x7fffffff, U - 1)];
    }
#pragma unroll
    for (int s = 0; s < BOOT_STEPS; ++s) {
      const bool in = t0 + s * 64 + lane < n;
      const uint32_t a = in ? wh[s] : 0u, b = in ? wl[s] : 0u;
      const uint32_t ph = eh[s] < 0 ? a : 0u, qh = eh[s] < 0 ? 0u : a;       // bit 31 = the label
      const uint32_t pl = el[s] < 0 ? b : 0u, ql = el[s] < 0 ? 0u : b;
      const uint32_t ih = wave_scan_add(qh), il = wave_scan_add(ql);
      acc += (uint64_t)ph * (uint64_t)(carry_hi + ih - qh) + (uint64_t)pl * (uint64_t)(carry_lo + il - ql);
      carry_hi += (uint32_t)__builtin_amdgcn_readlane((int)ih, 63);
      carry_lo += (uint32_t)__builtin_amdgcn_readlane((int)il, 63);
      sp += ph;
    }
  }
  // wave_sum_u64 of acc written out, interleaved with the sum of sp: as two loops the compiler schedules this kernel differently
#pragma unroll
  for (int d = 32; d >= 1; d >>= 1) {
    acc += ((uint64_t)(uint32_t)__shfl_xor((int)(acc >> 32), d) << 32) | (uint64_t)(uint32_t)__shfl_xor((int)(uint32_t)acc, d);
    sp += (uint32_t)__shfl_xor((int)sp, d);
  }
  if (lane == 0) {
    const size_t o = (size_t)rep * C + c0 + cl;
    num2[o] = acc, wpos[o] = sp, wneg[o] = carry_hi;
  }
}

// ---- stage 2b: the threshold sweep (cx_boot_sweep): average precision and fixed operating points of every (replicate, class) ---------
// The class's kept rows are listed ONCE, descending in score; an entry carries the label in bit 31 and, in bit 30, the mark "last entry
// of its tie group" (a property of the scores, prepared once: a group without weight in a replicate repeats the previous (tp, fp),
// adds nothing to the sum and cannot move a max or a min).  The wave shape is that of boot_auc_kernel: steps of 64 entries, BOOT_STEPS
// steps' loads and count-row gathers requested ahead, unit indices clamped to U - 1.  Per step: two inclusive scans (positive and
// negative weight) plus their carries give (tp, fp) at every lane; the tp of the previous group end is the exclusive max-scan of
// `mark ? tp : 0` (tp never decreases) joined with a wave-uniform carry; a marked lane whose tp moved adds
// (tp - prev) * floor((tp << 32) / (tp + fp)) to its uint64 sum; every operating point keeps a running max of tp / min of fp over the
// marked lanes that meet its integer condition.
// W+ and W- of the conditions are only known at the end of a sweep.  They come from a FIRST PASS over the same entries (loads and
// gathers, two adds per entry, no scan), not from the wpos / wneg that cx_boot_auc returns: the entry point then trusts nothing but
// its own operands (a caller's totals from another plan, another table or another n_units would silently move every threshold), the
// entries are L2-resident, and the pass is skipped when no operating point is asked for (the average precision needs no total).
// One wave owns the output elements of its (replicate, class): one writer, no LDS, no atomics, no float arithmetic in any result (the
// quotient is estimated in fp64 and corrected in integers, so the value is the integer floor whatever the estimate's rounding).
// Measured at 20 000 rows x 14 classes x 2000 replicates: 5.07 ms without operating points, 9.67 ms with two,
// 10.08 ms with eight, against 4.30 ms of cx_boot_auc on the same table; at 234 x 5 x 1000: 43 - 52 us (launch latency).  The first pass
// costs as much as the sweep, and six more operating points 4 %: the bound is the two dependent memory latencies per block of
// 64 * BOOT_STEPS entries (the entries, then the gather behind them), as in boot_auc_kernel, not the quotient.
constexpr int BOOT_POINTS = CX_BOOT_MAX_POINTS;
constexpr uint64_t BOOT_PPM = 1000000ull;

struct BootSweepPlan {
  ClassLists lists;               // first: the argument layout of the kernel is that of the lists with the points behind them
  int n_pts;
  int spec[BOOT_POINTS];          // 0: sens@ (max tp under fp * 1e6 <= (1e6 - ppm) * W-), 1: spec@ (min fp under tp * 1e6 >= ppm * W+)
  int ppm[BOOT_POINTS];
};

// floor((tp << 32) / den) for 1 <= den, tp <= den: the dividend is exact in fp64 (32 significant bits) and the quotient is <= 2^32, so
// the correctly rounded fp64 quotient is within 2^-21 of the true one and its integer part is the floor or one above it (one below is
// corrected as well, should the division ever be less than correctly rounded).
__device__ __forceinline__ uint64_t boot_quot32(const uint32_t tp, const uint32_t den) {
  const uint64_t a = (uint64_t)tp << 32;
  uint64_t q = (uint64_t)((double)a / (double)den);
  const int64_t r = (int64_t)(a - q * (uint64_t)den);
  if (r < 0) q -= 1ull;
  else if (r >= (int64_t)den) q += 1ull;
  return q;
}

__global__ __launch_bounds__(256) void boot_sweep_kernel(const uint32_t* __restrict__ counts, int ld, int n_rep,
                                                         const int32_t* __restrict__ order, const BootSweepPlan plan, int c0, int cn, int C,
                                                         uint64_t* __restrict__ apnum, uint32_t* __restrict__ wpos,
                                                         uint32_t* __restrict__ wneg, uint32_t* __restrict__ pts, int U) {
  const int lane = threadIdx.x & 63;
  const long long item = (long long)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (item >= (long long)n_rep * cn) return;                     // the same for all lanes of a wave; no barrier follows
  const int rep = (int)(item / cn), cl = (int)(item - (long long)rep * cn);
  const int n = plan.lists.len[cl], P = plan.n_pts;
  const int32_t* __restrict__ ent = order + plan.lists.offs[cl];
  const uint32_t* __restrict__ row = counts + (size_t)rep * ld;
  // first pass (only with operating points): the totals the conditions compare against
  uint32_t Wp = 0, Wn = 0;
  if (P > 0) {
    for (int t0 = 0; t0 < n; t0 += 64 * BOOT_STEPS) {
      int32_t e[BOOT_STEPS];
#pragma unroll
      for (int s = 0; s < BOOT_STEPS; ++s) e[s] = ent[min(t0 + s * 64 + lane, n - 1)];
      uint32_t w[BOOT_STEPS];
#pragma unroll
      for (int s = 0; s < BOOT_STEPS; ++s) w[s] = row[min(e[s] & 0x3fffffff, U - 1)];
#pragma unroll
      for (int s = 0; s < BOOT_STEPS; ++s) {
        const uint32_t a = t0 + s * 64 + lane < n ? w[s] : 0u;
        Wp += e[s] < 0 ? a : 0u, Wn += e[s] < 0 ? 0u : a;
      }
    }
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) Wp += (uint32_t)__shfl_xor((int)Wp, d), Wn += (uint32_t)__shfl_xor((int)Wn, d);
    Wp = (uint32_t)__builtin_amdgcn_readfirstlane((int)Wp), Wn = (uint32_t)__builtin_amdgcn_readfirstlane((int)Wn);
  }
  uint64_t rhs[BOOT_POINTS];
  uint32_t best[BOOT_POINTS];
#pragma unroll
  for (int k = 0; k < BOOT_POINTS; ++k) {                        // the point (0, 0) of the curve: meets every sens@ condition, a spec@ one iff W+ = 0
    rhs[k] = plan.spec[k] ? (uint64_t)plan.ppm[k] * Wp : (BOOT_PPM - (uint64_t)plan.ppm[k]) * Wn;
    best[k] = plan.spec[k] && Wp != 0u ? 0xffffffffu : 0u;
  }
  uint64_t acc = 0;
  uint32_t carry_p = 0, carry_q = 0, carry_prev = 0;             // weight before this step; tp of the last group end before this step
  for (int t0 = 0; t0 < n; t0 += 64 * BOOT_STEPS) {
    int32_t e[BOOT_STEPS];
#pragma unroll
    for (int s = 0; s < BOOT_STEPS; ++s) e[s] = ent[min(t0 + s * 64 + lane, n - 1)];      // past the end: the last entry again, dropped below
    uint32_t w[BOOT_STEPS];
#pragma unroll
    for (int s = 0; s < BOOT_STEPS; ++s) w[s] = row[min(e[s] & 0x3fffffff, U - 1)];       // unit indices are clamped, never trusted
#pragma unroll
    for (int s = 0; s < BOOT_STEPS; ++s) {
      const bool in = t0 + s * 64 + lane < n;
      const uint32_t a = in ? w[s] : 0u;
      const uint32_t p = e[s] < 0 ? a : 0u, q = e[s] < 0 ? 0u : a;                       // bit 31 = the label
      const uint32_t ip = wave_scan_add(p), iq = wave_scan_add(q);
      const uint32_t tp = carry_p + ip, fp = carry_q + iq;
      const bool mark = in && (e[s] & 0x40000000);                                       // bit 30 = the end of a tie group
      const uint32_t m = mark ? tp : 0u;
      const uint32_t x = wave_xscan_max(m);
      const uint32_t prev = max(carry_prev, x);
      if (mark && tp != prev) {                                  // a step of the precision-recall curve: the one place that divides
        const uint32_t den = tp + fp;
        if (den != 0u) acc += (uint64_t)(tp - prev) * boot_quot32(tp, den);
      }
      if (P > 0) {
        const uint64_t lt = (uint64_t)tp * BOOT_PPM, lf = (uint64_t)fp * BOOT_PPM;
#pragma unroll
        for (int k = 0; k < BOOT_POINTS; ++k) {
          if (k < P) {
            if (plan.spec[k]) best[k] = mark && lt >= rhs[k] ? min(best[k], fp) : best[k];
            else best[k] = mark && lf <= rhs[k] ? max(best[k], tp) : best[k];
          }
        }
      }
      carry_p += (uint32_t)__builtin_amdgcn_readlane((int)ip, 63);
      carry_q += (uint32_t)__builtin_amdgcn_readlane((int)iq, 63);
      carry_prev = max(carry_prev, (uint32_t)__builtin_amdgcn_readlane((int)max(x, m), 63));
    }
  }
  acc = wave_sum_u64(acc);
#pragma unroll
  for (int k = 0; k < BOOT_POINTS; ++k) {
    if (k < P) {
#pragma unroll
      for (int d = 32; d >= 1; d >>= 1) {
        const uint32_t o = (uint32_t)__shfl_xor((int)best[k], d);
        best[k] = plan.spec[k] ? min(best[k], o) : max(best[k], o);
      }
    }
  }
  if (lane == 0) {
    const size_t o = (size_t)rep * C + c0 + cl;
    apnum[o] = acc, wpos[o] = carry_p, wneg[o] = carry_q;
#pragma unroll
    for (int k = 0; k < BOOT_POINTS; ++k)
      if (k < P) pts[o * P + k] = best[k];
  }
}

}  // namespace

int cx_boot_counts(uint32_t* counts, int ld, int U, int first, int n_rep, uint64_t seed, void* stream) {
  if (!counts || n_rep < 1 || first < 0) return CX_EINVAL;
  if (U < 1 || U > BOOT_MAX_U || ld < U) return CX_ESHAPE;
  if (((uintptr_t)counts) & 3) return CX_EALIGN;
  if ((long long)first + n_rep > 0x7fffffffll) return CX_EINVAL;
  const int tiles = (U + BOOT_TILE - 1) / BOOT_TILE;
  if (tiles <= BOOT_MAX_TILES) {
    if ((long long)n_rep * tiles > 0x7fffffffll) return CX_ESHAPE;
    hipLaunchKernelGGL(boot_counts_lds_kernel, dim3((unsigned)(n_rep * tiles)), dim3(256), 0, as_stream(stream), counts, ld, U, first,
                       tiles, seed);
    return launch_status();
  }
  const int chunks = (U + 255) / 256;
  if ((long long)n_rep * chunks > 0x7fffffffll) return CX_ESHAPE;
  hipLaunchKernelGGL(boot_zero_kernel, dim3((unsigned)(n_rep * chunks)), dim3(256), 0, as_stream(stream), counts, ld, U, chunks);
  hipLaunchKernelGGL(boot_counts_global_kernel, dim3((unsigned)(n_rep * chunks)), dim3(256), 0, as_stream(stream), counts, ld, U, first,
                     chunks, seed);
  return launch_status();
}

int cx_boot_auc(const uint32_t* counts, int ld, int n_rep, const int32_t* order, const int64_t* offs, const int32_t* len, int C,
                uint64_t* num2, uint32_t* wpos, uint32_t* wneg, int U, void* stream) {
  if (!counts || !order || !offs || !len || !num2 || !wpos || !wneg || n_rep < 1 || C < 1) return CX_EINVAL;
  if (const int rc = check_class_lists(U, ld, offs, len, C)) return rc;
  if ((((uintptr_t)counts) & 3) || (((uintptr_t)order) & 3) || (((uintptr_t)num2) & 7) || (((uintptr_t)wpos) & 3) || (((uintptr_t)wneg) & 3))
    return CX_EALIGN;
  if (((long long)n_rep * CX_LIST_CLASSES + 3) / 4 > 0x7fffffffll) return CX_ESHAPE;
  ClassLists plan;
  return for_class_groups(offs, len, C, plan, [&](int c0, int cn) {
    const long long waves = (long long)n_rep * cn;
    hipLaunchKernelGGL(boot_auc_kernel, dim3((unsigned)((waves + 3) / 4)), dim3(256), 0, as_stream(stream), counts, ld, n_rep, order, plan,
                       c0, cn, C, num2, wpos, wneg, U);
  });
}

int cx_boot_sweep(const uint32_t* counts, int ld, int n_rep, const int32_t* order, const int64_t* offs, const int32_t* len, int C,
                  const int32_t* pt_type, const int32_t* pt_ppm, int P, uint64_t* apnum, uint32_t* wpos, uint32_t* wneg, uint32_t* pts,
                  int U, void* stream) {
  if (!counts || !order || !offs || !len || !apnum || !wpos || !wneg || n_rep < 1 || C < 1) return CX_EINVAL;
  if (P < 0 || P > BOOT_POINTS) return CX_ESHAPE;
  if (P > 0 && (!pt_type || !pt_ppm || !pts)) return CX_EINVAL;
  if (const int rc = check_class_lists(U, ld, offs, len, C)) return rc;
  for (int k = 0; k < P; ++k)
    if ((pt_type[k] != CX_BOOT_SENS && pt_type[k] != CX_BOOT_SPEC) || pt_ppm[k] < 1 || pt_ppm[k] > 999999) return CX_EINVAL;
  if ((((uintptr_t)counts) & 3) || (((uintptr_t)order) & 3) || (((uintptr_t)apnum) & 7) || (((uintptr_t)wpos) & 3) || (((uintptr_t)wneg) & 3) ||
      (P > 0 && (((uintptr_t)pts) & 3)))
    return CX_EALIGN;
  if (((long long)n_rep * CX_LIST_CLASSES + 3) / 4 > 0x7fffffffll) return CX_ESHAPE;
  BootSweepPlan plan;
  plan.n_pts = P;
  for (int k = 0; k < BOOT_POINTS; ++k) plan.spec[k] = k < P ? (pt_type[k] == CX_BOOT_SPEC) : 0, plan.ppm[k] = k < P ? pt_ppm[k] : 1;
  return for_class_groups(offs, len, C, plan.lists, [&](int c0, int cn) {
    const long long waves = (long long)n_rep * cn;
    hipLaunchKernelGGL(boot_sweep_kernel, dim3((unsigned)((waves + 3) / 4)), dim3(256), 0, as_stream(stream), counts, ld, n_rep, order,
                       plan, c0, cn, C, apnum, wpos, wneg, pts, U);
  });
}
