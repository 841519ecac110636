// Exact k-nearest-neighbour search and the weighted vote on pooled features (include/chexpert_hip.h, cx_knn_*): the kNN probe of a
// frozen backbone and image retrieval.  The Q x M similarity matrix is never stored.
//
// The order.  A (similarity, bank index) pair is ONE 64-bit key: the high word the fp32 similarity as an order-preserving unsigned
// integer (NaN counts as -inf, -0 as +0), the low word 0xFFFFFFFF - index.  A query's result is its k largest keys, descending:
// larger similarity first, the lower index on a tie.  The order is total and a key is never 0 (the high word of -inf is 0x007FFFFF),
// so 0 marks an empty slot and the result does not depend on the tiling, the slicing or the order in which candidates arrive.
//
//   knn_topk_kernel    a workgroup (4 waves) owns 32 queries and one slice of the bank.  Per 128 bank rows: q and bank chunks of 32
//                      columns go through LDS (whole 128-byte row segments from memory, stored k-major so that the operand reads of
//                      the fp32-input MFMA are conflict-free; the next chunk's loads are in flight during the MFMAs), each wave forms a
//                      32 rows x 32 queries tile on v_mfma_f32_32x32x2_f32 (two accumulators over alternate k pairs) and leaves it in
//                      LDS.  Then wave w takes queries 8 w .. 8 w + 7: the 128 keys are compared with the query's k-th key (one ballot
//                      per 64), and only the survivors are inserted into the query's sorted list (LDS, 32 x k keys), by the whole
//                      wave: position = the count of larger keys, the tail moves down one slot.  The slice's list goes to the scratch.
//   knn_merge_kernel   one wave per query: the slices' lists are sorted, so k rounds of "largest head" (lane = slice) give the result.
// No atomics, nothing sized by Q x M, partial tiles and the d tail by zero fill and predication: the same bits on every run.
#include "common.h"
#include <math.h>

namespace {

typedef unsigned long long u64;
constexpr int KNN_NT = 256, KNN_TQ = 32, KNN_TB = 128, KNN_KC = 32;
constexpr int KNN_SB = KNN_TB + 1, KNN_SQ = KNN_TQ + 1;      // k-major staging pitches: 1 (mod 32), the transposing stores are conflict-free
constexpr int KNN_SS = KNN_TB + 4;                           // pitch of the similarity tile [query][bank row], 16-byte rows
constexpr int KNN_MAX_K = CX_KNN_MAX_K, KNN_MAX_D = CX_KNN_MAX_D, KNN_MAX_SPLITS = CX_KNN_MAX_SPLITS, KNN_MAX_CLASSES = CX_KNN_MAX_CLASSES;
constexpr float KNN_EPS = 1e-12f;

static inline size_t knn_lds_bytes(int k) {
  return (size_t)KNN_TQ * k * sizeof(u64) + sizeof(float) * (KNN_KC * KNN_SB + KNN_KC * KNN_SQ + KNN_TQ * KNN_SS);
}

__device__ __forceinline__ uint32_t knn_ord(const float s) {
  uint32_t u = __float_as_uint(s);
  if (s != s) u = 0xff800000u;                  // NaN counts as -inf
  if (u == 0x80000000u) u = 0u;                 // -0 == +0
  return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}
__device__ __forceinline__ float knn_unord(const uint32_t o) { return __uint_as_float((o & 0x80000000u) ? (o & 0x7fffffffu) : ~o); }
__device__ __forceinline__ u64 knn_key(const float s, const uint32_t idx) { return ((u64)knn_ord(s) << 32) | (u64)(0xffffffffu - idx); }
__device__ __forceinline__ u64 knn_shfl(const u64 v, const int src) {
  const uint32_t lo = __shfl((int)(uint32_t)v, src), hi = __shfl((int)(uint32_t)(v >> 32), src);
  return ((u64)hi << 32) | lo;
}
__device__ __forceinline__ u64 knn_shfl_xor(const u64 v, const int o) {
  const uint32_t lo = __shfl_xor((int)(uint32_t)v, o), hi = __shfl_xor((int)(uint32_t)(v >> 32), o);
  return ((u64)hi << 32) | lo;
}
// orders one wave's LDS accesses: every lane's reads before it stand before every lane's writes after it
__device__ __forceinline__ void knn_wave_sync() {
  __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
  __builtin_amdgcn_wave_barrier();
}

// four consecutive values of one row from column `col` on; zeros past the row's end and for a row that does not exist
template <bool VEC>
__device__ __forceinline__ float4 knn_ld4(const float* __restrict__ base, const long long row, const bool row_ok, const int d, const int col) {
  float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
  if (!row_ok || col >= d) return v;
  const float* p = base + (size_t)row * d + col;
  if constexpr (VEC) return *reinterpret_cast<const float4*>(p);          // d % 4 == 0 and 16-byte bases: the whole quad is inside the row
  v.x = p[0];
  if (col + 1 < d) v.y = p[1];
  if (col + 2 < d) v.z = p[2];
  if (col + 3 < d) v.w = p[3];
  return v;
}

// `key` (larger than L[k - 1]) into the descending list L of k keys, by one whole wave: lane l owns the slots l, l + 64, ...
__device__ __forceinline__ void knn_insert(u64* __restrict__ L, const int k, const u64 key, const int lane) {
  u64 prev[4];
  int pos = 0;
#pragma unroll
  for (int t = 0; t < 4; ++t) {
    const int e = lane + 64 * t;
    const bool in = e < k;
    const u64 cur = in ? L[e] : 0ull;
    prev[t] = (in && e > 0) ? L[e - 1] : 0ull;
    pos += __popcll(__ballot(in && cur > key));
  }
  knn_wave_sync();
#pragma unroll
  for (int t = 0; t < 4; ++t) {
    const int e = lane + 64 * t;
    if (e < k && e >= pos) L[e] = e == pos ? key : prev[t];
  }
  knn_wave_sync();
}

template <bool VEC>
__global__ __launch_bounds__(KNN_NT) void knn_topk_kernel(const float* __restrict__ q, const float* __restrict__ bank,
                                                          const int* __restrict__ q_group, const int* __restrict__ bank_group,
                                                          u64* __restrict__ part, const int Q, const int M, const int d, const int k,
                                                          const int splits, const long long tiles_per_slice, const int qtiles) {
  extern __shared__ __align__(16) unsigned char knn_smem[];
  u64* const list = reinterpret_cast<u64*>(knn_smem);                       // [TQ][k]
  float* const bT = reinterpret_cast<float*>(list + (size_t)KNN_TQ * k);    // [KC][SB]: bank chunk, k-major
  float* const qT = bT + KNN_KC * KNN_SB;                                   // [KC][SQ]: query chunk, k-major
  float* const simT = qT + KNN_KC * KNN_SQ;                                 // [TQ][SS]: the tile's similarities
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, l31 = lane & 31, h = lane >> 5;
  const int slice = blockIdx.y, nch = (d + KNN_KC - 1) / KNN_KC;
  const long long tiles = ((long long)M + KNN_TB - 1) / KNN_TB;
  const long long t0 = min(tiles, (long long)slice * tiles_per_slice), t1 = min(tiles, t0 + tiles_per_slice);
  const long long rend = min((long long)M, t1 * KNN_TB);
  // staging coordinates: quad f = tid + 256 i of a [rows][8 quads] chunk -> row f >> 3, columns 4 (f & 7) ..
  const int sm = tid & 7, sr = tid >> 3;

  for (int qt = blockIdx.x; qt < qtiles; qt += gridDim.x) {
    const long long qbase = (long long)qt * KNN_TQ;
    for (int i = tid; i < KNN_TQ * k; i += KNN_NT) list[i] = 0ull;
    float4 rb[4], rq;
    auto issue = [&](const long long tile, const int ch) {
      const int col = ch * KNN_KC + 4 * sm;
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        const long long row = tile * KNN_TB + sr + 32 * i;
        rb[i] = knn_ld4<VEC>(bank, row, row < rend, d, col);
      }
      rq = knn_ld4<VEC>(q, qbase + sr, qbase + sr < Q, d, col);
    };
    long long tile = t0;
    int ch = 0;
    if (tile < t1) issue(tile, 0);
    f32x16 acc0, acc1;
    while (tile < t1) {
      __syncthreads();
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        const int r = sr + 32 * i;
        bT[(4 * sm + 0) * KNN_SB + r] = rb[i].x;
        bT[(4 * sm + 1) * KNN_SB + r] = rb[i].y;
        bT[(4 * sm + 2) * KNN_SB + r] = rb[i].z;
        bT[(4 * sm + 3) * KNN_SB + r] = rb[i].w;
      }
      qT[(4 * sm + 0) * KNN_SQ + sr] = rq.x;
      qT[(4 * sm + 1) * KNN_SQ + sr] = rq.y;
      qT[(4 * sm + 2) * KNN_SQ + sr] = rq.z;
      qT[(4 * sm + 3) * KNN_SQ + sr] = rq.w;
      __syncthreads();
      const bool last = ch == nch - 1;
      const long long ntile = last ? tile + 1 : tile;
      const int nchk = last ? 0 : ch + 1;
      if (ntile < t1) issue(ntile, nchk);                       // in flight during the MFMAs below
      if (ch == 0) {
#pragma unroll
        for (int i = 0; i < 16; ++i) { acc0[i] = 0.f; acc1[i] = 0.f; }
      }
      // D[i = bank row][j = query] += A[i][kk] B[kk][j]: lane l gives A[l & 31][l >> 5] and B[l >> 5][l & 31]
#pragma unroll
      for (int kk = 0; kk < KNN_KC / 2; kk += 2) {
        const float a0 = bT[(2 * kk + h) * KNN_SB + wave * 32 + l31], b0 = qT[(2 * kk + h) * KNN_SQ + l31];
        const float a1 = bT[(2 * kk + 2 + h) * KNN_SB + wave * 32 + l31], b1 = qT[(2 * kk + 2 + h) * KNN_SQ + l31];
        acc0 = __builtin_amdgcn_mfma_f32_32x32x2f32(a0, b0, acc0, 0, 0, 0);
        acc1 = __builtin_amdgcn_mfma_f32_32x32x2f32(a1, b1, acc1, 0, 0, 0);
      }
      if (last) {
        // register 4 g + j of lane (column = query l31) is bank row 8 g + 4 h + j of the wave's 32
#pragma unroll
        for (int g = 0; g < 4; ++g)
          *reinterpret_cast<float4*>(simT + l31 * KNN_SS + wave * 32 + 8 * g + 4 * h) =
              make_float4(acc0[4 * g] + acc1[4 * g], acc0[4 * g + 1] + acc1[4 * g + 1], acc0[4 * g + 2] + acc1[4 * g + 2],
                          acc0[4 * g + 3] + acc1[4 * g + 3]);
        __syncthreads();
        // selection: this wave's 8 queries against the tile's 128 rows (lane: rows lane and lane + 64)
        const long long g0 = tile * KNN_TB + lane, g1 = g0 + 64;
        const bool ok0 = g0 < rend, ok1 = g1 < rend;
        const int bg0 = (bank_group && ok0) ? bank_group[g0] : -1, bg1 = (bank_group && ok1) ? bank_group[g1] : -1;
        for (int qi = wave * 8; qi < wave * 8 + 8; ++qi) {
          if (qbase + qi >= Q) break;
          const int gq = q_group ? q_group[qbase + qi] : -1;
          u64* const L = list + (size_t)qi * k;
          u64 thr = L[k - 1];
          const float s0 = simT[qi * KNN_SS + lane], s1 = simT[qi * KNN_SS + lane + 64];
          const u64 key0 = (ok0 && !(gq >= 0 && bg0 == gq)) ? knn_key(s0, (uint32_t)g0) : 0ull;
          const u64 key1 = (ok1 && !(gq >= 0 && bg1 == gq)) ? knn_key(s1, (uint32_t)g1) : 0ull;
#pragma unroll
          for (int half = 0; half < 2; ++half) {
            const u64 key = half ? key1 : key0;
            u64 mask = __ballot(key > thr);
            while (mask) {
              const int src = __ffsll((long long)mask) - 1;
              mask &= mask - 1;
              const u64 cand = knn_shfl(key, src);
              if (cand > thr) {
                knn_insert(L, k, cand, lane);
                thr = L[k - 1];
              }
            }
          }
        }
      }
      tile = ntile;
      ch = nchk;
    }
    __syncthreads();
    for (int i = tid; i < KNN_TQ * k; i += KNN_NT) {
      const int qi = i / k, e = i - qi * k;
      if (qbase + qi < Q) part[((size_t)(qbase + qi) * splits + slice) * k + e] = list[i];
    }
    __syncthreads();
  }
}

// one wave per query: the `splits` descending lists of k keys -> the k largest, as (similarity, index)
__global__ __launch_bounds__(64) void knn_merge_kernel(const u64* __restrict__ part, float* __restrict__ out_sim, int* __restrict__ out_idx,
                                                       const int Q, const int k, const int splits) {
  const int lane = threadIdx.x;
  for (int qg = blockIdx.x; qg < Q; qg += gridDim.x) {
    const u64* const P = part + (size_t)qg * splits * k;
    int head[4];
    u64 hk[4];
#pragma unroll
    for (int t = 0; t < 4; ++t) {
      const int s = lane + 64 * t;
      head[t] = 0;
      hk[t] = s < splits ? P[(size_t)s * k] : 0ull;
    }
    u64 mine = 0ull;                                   // result e sits on lane e & 63 until 64 are complete
    for (int e = 0; e < k; ++e) {
      u64 best = 0ull;
#pragma unroll
      for (int t = 0; t < 4; ++t) best = hk[t] > best ? hk[t] : best;
      u64 m = best;
#pragma unroll
      for (int o = 32; o > 0; o >>= 1) {
        const u64 other = knn_shfl_xor(m, o);
        m = other > m ? other : m;
      }
      if (lane == (e & 63)) mine = m;
      if (m != 0ull && best == m) {                    // non-empty keys are distinct: one lane, one of its heads
#pragma unroll
        for (int t = 0; t < 4; ++t)
          if (hk[t] == m) {
            const int s = lane + 64 * t;
            ++head[t];
            hk[t] = head[t] < k ? P[(size_t)s * k + head[t]] : 0ull;
          }
      }
      if ((e & 63) == 63 || e == k - 1) {
        const int o = (e & ~63) + lane;
        if (o <= e) {
          out_sim[(size_t)qg * k + o] = mine ? knn_unord((uint32_t)(mine >> 32)) : -INFINITY;
          out_idx[(size_t)qg * k + o] = mine ? (int)(0xffffffffu - (uint32_t)mine) : -1;
        }
        mine = 0ull;
      }
    }
  }
}

// y = x / max(|x|, 1e-12) per row, one wave per row: lane l adds the squares of k = l, l + 64, ... in ascending k, then a xor butterfly
__global__ __launch_bounds__(KNN_NT) void knn_normalize_kernel(const float* x, float* y, const int rows,
                                                               const int d) {
  const int lane = threadIdx.x & 63;
  const long long row = (long long)blockIdx.x * (KNN_NT / 64) + (threadIdx.x >> 6);
  if (row >= rows) return;
  const float* xr = x + (size_t)row * d;
  float acc = 0.f;
  for (int k = lane; k < d; k += 64) acc = fmaf(xr[k], xr[k], acc);
  for (int o = 32; o > 0; o >>= 1) acc += __shfl_xor(acc, o);
  const float den = fmaxf(sqrtf(acc), KNN_EPS);
  for (int k = lane; k < d; k += 64) y[(size_t)row * d + k] = xr[k] / den;
}

// one workgroup of 64 per query: the weights once per neighbour (double), then thread c = class c sums them in list order (double);
// the two results are rounded to fp32 once
__global__ __launch_bounds__(64) void knn_vote_kernel(const float* __restrict__ sim, const int* __restrict__ idx,
                                                      const float* __restrict__ labels, float* __restrict__ out_score,
                                                      float* __restrict__ out_support, const float inv_T, const int Q, const int k,
                                                      const int n) {
  __shared__ double w_s[KNN_MAX_K];
  __shared__ float s_s[KNN_MAX_K];
  __shared__ int i_s[KNN_MAX_K];
  const int c = threadIdx.x;
  for (int qg = blockIdx.x; qg < Q; qg += gridDim.x) {
    __syncthreads();
    for (int j = c; j < k; j += 64) {
      i_s[j] = idx[(size_t)qg * k + j];
      s_s[j] = sim[(size_t)qg * k + j];
    }
    __syncthreads();
    float s0 = 0.f;                                    // the similarity of the first valid neighbour
    for (int j = 0; j < k; ++j)
      if (i_s[j] >= 0) { s0 = s_s[j]; break; }
    for (int j = c; j < k; j += 64) {
      const float s = s_s[j];
      w_s[j] = (inv_T == 0.f || s == s0) ? 1.0 : exp(((double)s - (double)s0) * (double)inv_T);
    }
    __syncthreads();
    if (c < n) {
      double num = 0.0, den = 0.0;
      for (int j = 0; j < k; ++j) {
        const int r = i_s[j];
        if (r < 0) continue;
        const float yv = labels[(size_t)r * n + c];
        if (yv >= 0.f) {
          num += w_s[j] * (double)yv;
          den += w_s[j];
        }
      }
      out_score[(size_t)qg * n + c] = den > 0.0 ? (float)(num / den) : 0.5f;
      out_support[(size_t)qg * n + c] = den > 0.0 ? (float)den : 0.f;
    }
  }
}

// compute units of the current device (256 where none answers: the sizes are then still validated without a GPU)
int knn_cus() {
  static const int cus = [] {
    int dev = 0, n = 0;
    if (hipGetDevice(&dev) != hipSuccess || hipDeviceGetAttribute(&n, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess || n < 1) {
      (void)hipGetLastError();
      n = 256;
    }
    return n;
  }();
  return cus;
}

// the slices of a search: the caller's, or enough (query tile, slice) workgroups for two per compute unit, each slice at least 8 tiles
int knn_splits(const int Q, const int M, const int splits) {
  if (splits > 0) return splits;
  const long long qtiles = ((long long)Q + KNN_TQ - 1) / KNN_TQ, tiles = ((long long)M + KNN_TB - 1) / KNN_TB;
  long long s = (2ll * knn_cus() + qtiles - 1) / qtiles;
  s = s < tiles / 8 ? s : tiles / 8;
  return (int)(s < 1 ? 1 : s > KNN_MAX_SPLITS ? KNN_MAX_SPLITS : s);
}

bool knn_sizes_ok(const int Q, const int M, const int k, const int splits) {
  return Q >= 1 && M >= 1 && k >= 1 && k <= KNN_MAX_K && splits >= 0 && splits <= KNN_MAX_SPLITS;
}
static inline bool aligned_to(const void* p, const uintptr_t a) { return (((uintptr_t)p) & (a - 1)) == 0; }

}  // namespace

long long cx_knn_scratch(int Q, int M, int k, int splits) {
  if (!knn_sizes_ok(Q, M, k, splits)) return 0;
  return 2ll * Q * knn_splits(Q, M, splits) * k;
}

int cx_knn_normalize(const float* x, float* y, int rows, int d, void* stream) {
  if (!x || !y || rows < 1 || d < 1 || d > KNN_MAX_D) return CX_EINVAL;
  if (!aligned_to(x, 4) || !aligned_to(y, 4)) return CX_EALIGN;
  const long long blocks = ((long long)rows + KNN_NT / 64 - 1) / (KNN_NT / 64);
  hipLaunchKernelGGL(knn_normalize_kernel, dim3((unsigned)blocks), dim3(KNN_NT), 0, as_stream(stream), x, y, rows, d);
  return launch_status();
}

int cx_knn_topk(const float* q, const float* bank, const int* q_group, const int* bank_group, float* out_sim, int* out_idx, float* scratch,
                long long scratch_floats, int Q, int M, int d, int k, int splits, void* stream) {
  if (!q || !bank || !out_sim || !out_idx || !scratch || (q_group == nullptr) != (bank_group == nullptr)) return CX_EINVAL;
  if (!knn_sizes_ok(Q, M, k, splits) || d < 1 || d > KNN_MAX_D) return CX_EINVAL;
  if (scratch_floats < cx_knn_scratch(Q, M, k, splits)) return CX_EINVAL;
  if (!aligned_to(q, 4) || !aligned_to(bank, 4) || !aligned_to(out_sim, 4) || !aligned_to(out_idx, 4) || !aligned_to(q_group, 4) ||
      !aligned_to(bank_group, 4) || !aligned_to(scratch, 8))
    return CX_EALIGN;
  const int S = knn_splits(Q, M, splits);
  const long long tiles = ((long long)M + KNN_TB - 1) / KNN_TB, tps = (tiles + S - 1) / S;
  const long long qtiles = ((long long)Q + KNN_TQ - 1) / KNN_TQ;
  const int gx = (int)(qtiles < 65536 ? qtiles : 65536);
  const size_t lds = knn_lds_bytes(k);
  const bool vec = (d % 4 == 0) && aligned16(q) && aligned16(bank);
  u64* part = reinterpret_cast<u64*>(scratch);
  static const bool attr = ((void)hipFuncSetAttribute(reinterpret_cast<const void*>(&knn_topk_kernel<true>),
                                                      hipFuncAttributeMaxDynamicSharedMemorySize, (int)knn_lds_bytes(KNN_MAX_K)),
                            (void)hipFuncSetAttribute(reinterpret_cast<const void*>(&knn_topk_kernel<false>),
                                                      hipFuncAttributeMaxDynamicSharedMemorySize, (int)knn_lds_bytes(KNN_MAX_K)),
                            true);
  (void)attr;
  if (vec)
    hipLaunchKernelGGL(knn_topk_kernel<true>, dim3(gx, S), dim3(KNN_NT), lds, as_stream(stream), q, bank, q_group, bank_group, part, Q, M, d,
                       k, S, tps, (int)qtiles);
  else
    hipLaunchKernelGGL(knn_topk_kernel<false>, dim3(gx, S), dim3(KNN_NT), lds, as_stream(stream), q, bank, q_group, bank_group, part, Q, M, d,
                       k, S, tps, (int)qtiles);
  hipLaunchKernelGGL(knn_merge_kernel, dim3(Q < (1 << 20) ? Q : (1 << 20)), dim3(64), 0, as_stream(stream), part, out_sim, out_idx, Q, k, S);
  return launch_status();
}

int cx_knn_vote(const float* sim, const int* idx, const float* labels, float* out_score, float* out_support, float inv_T, int Q, int k,
                int n, void* stream) {
  if (!sim || !idx || !labels || !out_score || !out_support || Q < 1 || k < 1 || k > KNN_MAX_K || n < 1 || n > KNN_MAX_CLASSES ||
      !(inv_T >= 0.f))
    return CX_EINVAL;
  hipLaunchKernelGGL(knn_vote_kernel, dim3(Q < (1 << 20) ? Q : (1 << 20)), dim3(64), 0, as_stream(stream), sim, idx, labels, out_score,
                     out_support, inv_T, Q, k, n);
  return launch_status();
}
