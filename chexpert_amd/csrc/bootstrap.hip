// Non-parametric bootstrap of the AUROC on the GPU (include/chexpert_hip.h, cx_boot_counts / cx_boot_auc; chexpert_amd/metrics.py states
// both in numpy and the tests hold the kernels to that statement bit for bit).  Everything is integer arithmetic:
//   counts[b][u] = number of the U draws of replicate b that hit unit u, draw j of replicate b being the splitmix64 hash of
//                  (seed, b * U + j) scaled to [0, U) by a multiply-shift
//   num2[b][c]   = S(hi order) + S(lo order),  S = sum_t p_t * (sum_{t' < t} q_t'),  p / q = the weight counts[b][unit] of entry t where
//                  the entry is a positive / a negative: twice the numerator of the weighted trapezoid AUROC, ties counted half
// Two entry points, one per stage, so that each can be held on its own and a paired comparison can run two plans over one table.
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
#include "common.h"

namespace {

constexpr int BOOT_TILE = CX_BOOT_TILE;            // units per workgroup of the LDS form: 32 KB of counters, 4 workgroups per CU
constexpr int BOOT_MAX_TILES = CX_BOOT_MAX_TILES;  // more tiles than this per replicate: the device-memory form (a tile re-hashes all U draws)
constexpr int BOOT_MAX_U = CX_BOOT_MAX_UNITS;
constexpr int BOOT_CLASSES = 32;          // classes per launch of the scan stage (offsets and lengths travel as kernel arguments)

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
// are requested before the first scan consumes any.  Per step and order: an inclusive wave scan of q in uint32 (DPP: four shifts inside
// the rows of 16 lanes, then lane 15 of a row to the next row and lane 31 to the upper half), the exclusive prefix plus the running
// carry times p added to the lane's uint64 sum, and the carry advanced by the step's total (lane 63, wave-uniform).  The two orders are
// independent chains, which is what lets one wave own the output element: one writer, no LDS, no barrier.
__device__ __forceinline__ uint32_t boot_wave_scan(uint32_t v) {
#define BOOT_DPP(ctrl, rows) v += (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, ctrl, rows, 0xf, false)
  BOOT_DPP(0x111, 0xf);       // row_shr:1
  BOOT_DPP(0x112, 0xf);       // row_shr:2
  BOOT_DPP(0x114, 0xf);       // row_shr:4
  BOOT_DPP(0x118, 0xf);       // row_shr:8
  BOOT_DPP(0x142, 0xa);       // row_bcast:15 into rows 1 and 3
  BOOT_DPP(0x143, 0xc);       // row_bcast:31 into rows 2 and 3
#undef BOOT_DPP
  return v;
}

struct BootPlan {
  long long offs[BOOT_CLASSES];
  int len[BOOT_CLASSES];
};

constexpr int BOOT_STEPS = 4;

__global__ __launch_bounds__(256) void boot_auc_kernel(const uint32_t* __restrict__ counts, int ld, int n_rep,
                                                       const int32_t* __restrict__ order, const BootPlan plan, int c0, int cn, int C,
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
      const uint32_t ih = boot_wave_scan(qh), il = boot_wave_scan(ql);
      acc += (uint64_t)ph * (uint64_t)(carry_hi + ih - qh) + (uint64_t)pl * (uint64_t)(carry_lo + il - ql);
      carry_hi += (uint32_t)__builtin_amdgcn_readlane((int)ih, 63);
      carry_lo += (uint32_t)__builtin_amdgcn_readlane((int)il, 63);
      sp += ph;
    }
  }
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
  if (U < 1 || U > BOOT_MAX_U || ld < U) return CX_ESHAPE;
  for (int c = 0; c < C; ++c)
    if (len[c] < 0 || offs[c] < 0) return CX_EINVAL;
  if ((((uintptr_t)counts) & 3) || (((uintptr_t)order) & 3) || (((uintptr_t)num2) & 7) || (((uintptr_t)wpos) & 3) || (((uintptr_t)wneg) & 3))
    return CX_EALIGN;
  if (((long long)n_rep * BOOT_CLASSES + 3) / 4 > 0x7fffffffll) return CX_ESHAPE;
  for (int c0 = 0; c0 < C; c0 += BOOT_CLASSES) {
    const int cn = min(BOOT_CLASSES, C - c0);
    BootPlan plan;
    for (int c = 0; c < BOOT_CLASSES; ++c) plan.offs[c] = c < cn ? (long long)offs[c0 + c] : 0ll, plan.len[c] = c < cn ? len[c0 + c] : 0;
    const long long waves = (long long)n_rep * cn;
    hipLaunchKernelGGL(boot_auc_kernel, dim3((unsigned)((waves + 3) / 4)), dim3(256), 0, as_stream(stream), counts, ld, n_rep, order, plan,
                       c0, cn, C, num2, wpos, wneg, U);
    const int rc = launch_status();
    if (rc) return rc;
  }
  return 0;
}
