// DeLong / Obuchowski variance of the AUROC on the GPU (include/chexpert_hip.h, cx_delong_place / cx_delong_gram; chexpert_amd/metrics.py
// states both in numpy and the tests hold the kernels to that statement bit for bit).  Everything is integer arithmetic:
//   place: z[4c .. 4c+3][u] = (sum of X2 over the positives of unit u, their number, sum of Y2 over its negatives, their number) of class
//          c, X2 / Y2 the doubled placements (ties counted half) read off the `hi` / `lo` orders of metrics.bootstrap_plan
//   gram:  g[p][q] = sum_u z[p][u] * z[q][u] mod 2^64, the raw moment sums from which the host forms every variance and covariance in
//          exact integers before it divides once
// What is read how often: the order arrays (8 B per kept row and class) twice (the count of the positives, then the scan), coalesced;
// the table z is written by one 64-bit atomic per entry and order plus one per entry for the counts, and read once by the Gram stage.
// Bounds: the placement stage is bound by latency, not by bytes: every workgroup counts the positives of its whole list (one coalesced
// pass, L2-resident) before it walks its own CX_DELONG_WG_ENTRIES entries (per step one load, one ballot, two barriers, the atomics);
// the Gram stage by the 64-bit multiply-add on the vector ALU (four 32-bit multiplies each; MFMA has no such type): Q (Q + 4) / 2 of
// them per unit.
// Measured at 200 000 rows x 14 classes, two models stacked for the Gram stage (Q = 112): placements 395 us per
// model, Gram 656 us (2.0e12 multiply-adds per second); at 234 x 5: 23 us and 17 us (launch latency).
// Same bits every run: the only unordered operations are integer adds (device-memory atomics), and integer adds commute -- the
// project's rule is about the order of FLOAT sums, of which this file has none.  No workgroup waits on another.
#include "resample.h"

namespace {

typedef unsigned long long u64;

constexpr int DL_THREADS = 1024;
constexpr int DL_WAVES = DL_THREADS / 64;
constexpr int DL_STEPS = 4;                            // entries per thread and step of the walk
constexpr int DL_STEP_ENTRIES = DL_THREADS * DL_STEPS;
constexpr int DL_CHUNK = CX_DELONG_WG_ENTRIES;         // entries of a list that one workgroup walks
static_assert(DL_CHUNK % DL_STEP_ENTRIES == 0, "a workgroup walks whole steps");
static_assert(DL_STEPS * DL_WAVES == 64, "one lane per wave total in the scan of the totals");
constexpr int DL_MAX_U = CX_BOOT_MAX_UNITS;

// rows x cols elements of a table of pitch ld, grid-stride (the padding behind the columns is not touched)
__global__ __launch_bounds__(256) void delong_zero_kernel(u64* __restrict__ p, long long ld, int cols, long long total) {
  for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < total; i += (long long)gridDim.x * 256) {
    const long long r = i / cols;
    p[r * ld + (i - r * cols)] = 0ull;
  }
}

// ---- placements: one workgroup per (class, order, chunk of DL_CHUNK entries) ---------------------------------------------------------
// Pass 1 reads the whole list and counts its positives M and those in front of the workgroup's chunk: that is the chunk's carry, so
// no workgroup waits for another and nothing is handed over (the lists are L2-resident; the pass is one coalesced read).  Pass 2 walks
// the chunk in steps of DL_STEP_ENTRIES entries, thread t the entries t, t + 1024, ... of the step: the number of positives in front of
// an entry is the carry, plus the totals of the waves in front of it within the step (64 totals in LDS, scanned by every wave on its
// own: no second hand-over), plus the ballot bits below its lane.  The negatives in front are the position minus that.
__global__ __launch_bounds__(DL_THREADS) void delong_place_kernel(const int32_t* __restrict__ order, const ClassLists plan, int c0,
                                                                  u64* __restrict__ z, long long ldz, int U) {
  __shared__ uint32_t tot[DL_STEPS * DL_WAVES];
  __shared__ uint32_t red[2 * DL_WAVES];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int cl = blockIdx.y >> 1, k = blockIdx.y & 1;            // k = 0: the hi order (it also counts the rows), 1: lo
  const long long n = plan.len[cl];
  const long long start = (long long)blockIdx.x * DL_CHUNK;
  if (start >= n) return;                                        // the same for the whole workgroup (n == 0 included); no barrier before this
  const long long end = min(n, start + DL_CHUNK);
  const int32_t* __restrict__ ent = order + plan.offs[cl] + (long long)k * n;
  uint32_t cnt = 0, front = 0;
#pragma unroll 4
  for (long long t = tid; t < n; t += DL_THREADS) {
    const uint32_t pos = ent[t] < 0 ? 1u : 0u;                   // bit 31 = the label
    cnt += pos, front += t < start ? pos : 0u;
  }
#pragma unroll
  for (int d = 32; d >= 1; d >>= 1) cnt += (uint32_t)__shfl_xor((int)cnt, d), front += (uint32_t)__shfl_xor((int)front, d);
  if (lane == 0) red[wave] = cnt, red[DL_WAVES + wave] = front;
  __syncthreads();
  uint32_t M = 0, carry = 0;                                     // carry: positives before this step
#pragma unroll
  for (int w = 0; w < DL_WAVES; ++w) M += red[w], carry += red[DL_WAVES + w];
  u64* __restrict__ X = z + (long long)(4 * (c0 + cl)) * ldz;
  u64* __restrict__ mm = X + ldz;
  u64* __restrict__ Y = mm + ldz;
  u64* __restrict__ nn = Y + ldz;
  for (long long t0 = start; t0 < end; t0 += DL_STEP_ENTRIES) {
    int32_t e[DL_STEPS];
    uint32_t pre[DL_STEPS];
#pragma unroll
    for (int s = 0; s < DL_STEPS; ++s) {
      const long long t = t0 + s * DL_THREADS + tid;
      e[s] = ent[t < end ? t : end - 1];                         // past the end: the chunk's last entry again (in bounds), dropped below
    }
#pragma unroll
    for (int s = 0; s < DL_STEPS; ++s) {
      const bool pos = t0 + s * DL_THREADS + tid < end && e[s] < 0;
      const u64 b = __ballot(pos);
      pre[s] = (uint32_t)__popcll(b & ((1ull << lane) - 1ull));
      if (lane == 0) tot[s * DL_WAVES + wave] = (uint32_t)__popcll(b);
    }
    __syncthreads();
    const uint32_t v = tot[lane];
    uint32_t incl = v;
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
      const uint32_t o = (uint32_t)__shfl_up((int)incl, d);
      if (lane >= d) incl += o;
    }
    const uint32_t excl = incl - v;
    const uint32_t step_total = (uint32_t)__shfl((int)incl, 63);
#pragma unroll
    for (int s = 0; s < DL_STEPS; ++s) {
      const uint32_t before = (uint32_t)__shfl((int)excl, s * DL_WAVES + wave);     // every lane takes part
      const long long t = t0 + s * DL_THREADS + tid;
      if (t < end) {
        const uint32_t pb = carry + before + pre[s];             // positives in front of entry t
        const int u = min(e[s] & 0x7fffffff, U - 1);             // unit indices are clamped, never trusted
        if (e[s] < 0) {
          atomicAdd(&X[u], (u64)((uint32_t)t - pb));             // the negatives in front
          if (k == 0) atomicAdd(&mm[u], 1ull);
        } else {
          atomicAdd(&Y[u], (u64)(M - pb));                       // the positives behind
          if (k == 0) atomicAdd(&nn[u], 1ull);
        }
      }
    }
    carry += step_total;
    __syncthreads();                                             // tot is written again by the next step
  }
}

// ---- Gram matrix of the rows: a workgroup owns the tiles blockIdx.x, blockIdx.x + gridDim.x, ... of DG_TILE units -------------------
// The tile is staged transposed, lds[unit][row] with an odd pitch, so that the four rows of a block are adjacent.  The upper triangle of
// g is cut into 4 x 4 blocks (at most 528 for Q = 128); a thread owns the blocks tid, tid + 256, tid + 512 and keeps their 16 sums in
// registers over all its workgroup's tiles, then adds them to g (and to the mirrored element) with one atomic each.
constexpr int DG_TILE = CX_DELONG_TILE;
constexpr int DG_MAXQ = CX_DELONG_MAX_ROWS;
constexpr int DG_BLOCKS = 3;                           // 4 x 4 blocks per thread
static_assert((DG_MAXQ / 4) * (DG_MAXQ / 4 + 1) / 2 <= DG_BLOCKS * 256, "every block of the upper triangle has an owner");
constexpr int DG_MAX_GRID = 1024;

__global__ __launch_bounds__(256) void delong_gram_kernel(const u64* __restrict__ z, long long ldz, int Q, int U, u64* __restrict__ g,
                                                          int tiles) {
  __shared__ u64 lds[DG_TILE * (DG_MAXQ + 1)];
  const int tid = threadIdx.x;
  const int nb = (Q + 3) >> 2, QP = nb * 4 + 1, npairs = nb * (nb + 1) / 2;
  int bp[DG_BLOCKS], bq[DG_BLOCKS];
#pragma unroll
  for (int k = 0; k < DG_BLOCKS; ++k) {
    int rem = k * 256 + tid, p = 0;
    if (rem >= npairs) rem = 0;                                  // no block: computed nowhere (guarded below), the indices stay in bounds
    while (rem >= nb - p) rem -= nb - p, ++p;                    // row p of the triangle holds nb - p blocks; at most nb turns
    bp[k] = p, bq[k] = p + rem;
  }
  u64 acc[DG_BLOCKS][16];
#pragma unroll
  for (int k = 0; k < DG_BLOCKS; ++k)
#pragma unroll
    for (int i = 0; i < 16; ++i) acc[k][i] = 0ull;
  for (int tile = blockIdx.x; tile < tiles; tile += gridDim.x) {
    const int u0 = tile * DG_TILE;
    __syncthreads();                                             // the previous tile has been consumed
    for (int idx = tid; idx < nb * 4 * DG_TILE; idx += 256) {
      const int q = idx / DG_TILE, j = idx - q * DG_TILE;
      lds[j * QP + q] = q < Q && u0 + j < U ? z[(long long)q * ldz + u0 + j] : 0ull;      // rows past Q and units past U: zeros
    }
    __syncthreads();
#pragma unroll
    for (int k = 0; k < DG_BLOCKS; ++k) {
      if (k * 256 + tid < npairs) {
        const u64* __restrict__ ra = lds + 4 * bp[k];
        const u64* __restrict__ rb = lds + 4 * bq[k];
        for (int j = 0; j < DG_TILE; ++j) {
          u64 a[4], b[4];
#pragma unroll
          for (int i = 0; i < 4; ++i) a[i] = ra[j * QP + i], b[i] = rb[j * QP + i];
#pragma unroll
          for (int i = 0; i < 4; ++i)
#pragma unroll
            for (int jj = 0; jj < 4; ++jj) acc[k][i * 4 + jj] += a[i] * b[jj];
        }
      }
    }
  }
#pragma unroll
  for (int k = 0; k < DG_BLOCKS; ++k) {
    if (k * 256 + tid < npairs) {
#pragma unroll
      for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int jj = 0; jj < 4; ++jj) {
          const int p = 4 * bp[k] + i, q = 4 * bq[k] + jj;
          if (p < Q && q < Q) {
            atomicAdd(&g[p * Q + q], acc[k][i * 4 + jj]);
            if (bp[k] != bq[k]) atomicAdd(&g[q * Q + p], acc[k][i * 4 + jj]);      // a diagonal block holds both halves itself
          }
        }
    }
  }
}

}  // namespace

int cx_delong_place(const int32_t* order, const int64_t* offs, const int32_t* len, int C, int U, int64_t* z, int ldz, void* stream) {
  if (!order || !offs || !len || !z || C < 1) return CX_EINVAL;
  if (const int rc = check_class_lists(U, ldz, offs, len, C)) return rc;
  if ((((uintptr_t)order) & 3) || (((uintptr_t)z) & 7)) return CX_EALIGN;
  const long long total = 4ll * C * U;
  const unsigned zgrid = (unsigned)((total + 255) / 256 < 4096 ? (total + 255) / 256 : 4096);
  hipLaunchKernelGGL(delong_zero_kernel, dim3(zgrid), dim3(256), 0, as_stream(stream), (u64*)z, (long long)ldz, U, total);
  int rc = launch_status();
  if (rc) return rc;
  ClassLists plan;
  return for_class_groups(offs, len, C, plan, [&](int c0, int cn) {
    int longest = 0;
    for (int c = 0; c < cn; ++c) longest = max(longest, plan.len[c]);
    if (longest == 0) return;                                    // nothing to add: the rows stay zero
    const unsigned chunks = (unsigned)(((long long)longest + DL_CHUNK - 1) / DL_CHUNK);
    hipLaunchKernelGGL(delong_place_kernel, dim3(chunks, (unsigned)(2 * cn)), dim3(DL_THREADS), 0, as_stream(stream), order, plan, c0,
                       (u64*)z, (long long)ldz, U);
  });
}

int cx_delong_gram(const int64_t* z, int ldz, int Q, int U, int64_t* g, void* stream) {
  if (!z || !g) return CX_EINVAL;
  if (Q < 1 || Q > DG_MAXQ || U < 1 || U > DL_MAX_U || ldz < U) return CX_ESHAPE;
  if ((((uintptr_t)z) & 7) || (((uintptr_t)g) & 7)) return CX_EALIGN;
  const long long total = (long long)Q * Q;
  hipLaunchKernelGGL(delong_zero_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, as_stream(stream), (u64*)g, (long long)Q, Q,
                     total);
  int rc = launch_status();
  if (rc) return rc;
  const int tiles = (U + DG_TILE - 1) / DG_TILE;
  hipLaunchKernelGGL(delong_gram_kernel, dim3((unsigned)min(tiles, DG_MAX_GRID)), dim3(256), 0, as_stream(stream), (const u64*)z,
                     (long long)ldz, Q, U, (u64*)g, tiles);
  return launch_status();
}
