// Forward of the dense-layer bottleneck 1x1 convolution, K <= 256 input channels (round 4):
//   Y[m][0:128] = relu(X[m][0:K]*scale + shift) . W^T   (+ per-channel sum / sum of squares of the values as stored)
// torchvision `_DenseLayer.norm1 -> relu1 -> conv1` as restated at models/attn_aug_conv.py:13 (forward).
//
// Every global access covers a whole row.  The layer is a stream (K <= 256 against 128 outputs), and the shape of the accesses
// sets its speed: feeding the MFMA's B operand straight from global memory (a lane loads 16 bytes of ITS pixel, so one
// wave-instruction touches 16-byte pieces of 32 different pixels, every 128-byte line is completed by four instructions, and the
// stores are 32-byte pieces likewise) is a fragmentary shape.  Measured (scratch/segbench.hip, profiles/r04_segbench.txt), a bare
// stream in that shape runs at 3.3-4.2 TB/s against 4.9-5.0 TB/s when a wave-instruction covers whole rows -- and a kernel built
// that way sat at 3.2 TB/s.  So here a workgroup (512 threads, one per CU) walks 64-pixel tiles; the tile's
// activations are requested two tiles ahead in the staging shape (consecutive lanes = consecutive 16-byte chunks of a pixel row),
// normalised on the way into a double-buffered LDS image, multiplied from there (weights resident in LDS), and the output tile goes
// back through LDS to leave as whole 256-byte rows.  Two barriers per tile; statistics as per-lane registers reduced once per
// workgroup (deterministic rows).
#include <type_traits>
#include "common.h"

namespace {

constexpr int NO = 128;                 // output channels (bn_size * growth_rate)
constexpr int BM = 64;                  // pixels per tile
constexpr int NT = 512;
constexpr int OP = NO * 2 + 16;         // out-tile pitch (bytes)
typedef uint32_t f2_u32x4 __attribute__((ext_vector_type(4)));

template <int CTRL>
__device__ __forceinline__ float dpp_add(float v) {
  return v + __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(v), CTRL, 0xF, 0xF, true));
}
__device__ __forceinline__ float half_sum(float v) {      // sum over the 32 lanes of each wave half
  v = dpp_add<0xB1>(v);
  v = dpp_add<0x4E>(v);
  v = dpp_add<0x141>(v);
  v = dpp_add<0x140>(v);
  return v + __shfl_xor(v, 16);
}

// KT = K / 32 (a compile-time K: the multiply loop is fully unrolled and its LDS fragment reads run ahead of the MFMAs -- with a
// run-time trip count every MFMA waited for its own two reads and the K = 224 layer took 2.6 times the K = 64 one for 1.8 times the
// bytes); NCH = 16-byte chunks of a tile per thread = ceil(64 * (K / 8) / 512): 1 (K = 32, 64) .. 4 (K = 256)
template <int PRO, int KT>
__global__ __launch_bounds__(NT, 1) void pw_fwd2_kernel(const CxConv p, const int M, const int m_tiles, const int tiles_per_wg) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  constexpr int K = KT * 32, cpr = K >> 3;                       // chunks per row
  constexpr int xp = K * 2 + 16;                                 // X / W tile pitch in bytes
  constexpr int NCH = (BM * cpr + NT - 1) / NT;
  float* coef = reinterpret_cast<float*>(smem);                  // [2][K]
  char* Wt = smem + 2 * K * 4;                                   // [128][xp]
  char* Xl = Wt + NO * xp;                                       // [2][64][xp]
  char* Ol = Xl + 2 * BM * xp;                                   // [64][OP]

  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int lrow = lane & 31, lh = lane >> 5;
  const int pw = wave & 1, cq = wave >> 1;                       // this wave's 32 pixels x 32 output channels
  const bf16* __restrict__ X = reinterpret_cast<const bf16*>(p.x);
  const bf16* __restrict__ Wp = reinterpret_cast<const bf16*>(p.w);
  bf16* __restrict__ Y = reinterpret_cast<bf16*>(p.y);

  const int t0 = blockIdx.x * tiles_per_wg;
  const int t1 = min(m_tiles, t0 + tiles_per_wg);

  if (PRO == CX_PRO_AFFINE_RELU) {
    for (int i = tid; i < K; i += NT) {
      coef[i] = p.pa[i];
      coef[K + i] = p.pb[i];
    }
  }
  for (int i = tid; i < NO * cpr; i += NT) {                     // weights [128][K] -> LDS
    const int n = i / cpr, c = i - n * cpr;
    *reinterpret_cast<uint4*>(Wt + n * xp + c * 16) = *reinterpret_cast<const uint4*>(Wp + (size_t)n * K + c * 8);
  }

  // staging slots of this thread: chunk id tid + 512 i -> (row, chunk); the same for every tile
  int srow[NCH], sch[NCH];
  bool sok[NCH];
#pragma unroll
  for (int i = 0; i < NCH; ++i) {
    const int cid = tid + NT * i;
    sok[i] = cid < BM * cpr;
    const int c = sok[i] ? cid : 0;
    srow[i] = c / cpr;
    sch[i] = c - srow[i] * cpr;
  }
  f2_u32x4 xa[NCH], xb[NCH];
  auto request = [&](int mt, f2_u32x4 (&xr)[NCH]) __attribute__((always_inline)) {
    const int mtc = mt < t1 ? mt : t1 - 1;                       // clamped: the loads are unconditional
#pragma unroll
    for (int i = 0; i < NCH; ++i) {
      const int m = mtc * BM + srow[i];
      const int mc = m < M ? m : M - 1;
      xr[i] = *reinterpret_cast<const f2_u32x4*>(X + (size_t)mc * p.ldx + sch[i] * 8);   // (non-temporal loads / stores here: no change, A/B)
    }
  };
  request(t0, xa);
  request(t0 + 1, xb);

  float s1[2][8], s2[2][8];
#pragma unroll
  for (int cc = 0; cc < 2; ++cc)
#pragma unroll
    for (int e = 0; e < 8; ++e) s1[cc][e] = s2[cc][e] = 0.f;
  const bool want_stats = p.stat_sum != nullptr;
  // output rows this thread stores: 16-byte chunk q of rows r0 and r0 + 32
  const int q = tid & 15, r0 = tid >> 4;
  __syncthreads();                                               // coefficients and weights visible

  auto tile = [&](const int mt, auto SelC, f2_u32x4 (&xr)[NCH]) __attribute__((always_inline)) {
    constexpr int SEL = decltype(SelC)::value;
    const int m0 = mt * BM;
    const bool tvalid = mt < t1;
    char* Xb = Xl + SEL * (BM * xp);
    // ---- this tile's activations (in registers since two tiles ago) -> LDS, BN + ReLU applied
#pragma unroll
    for (int i = 0; i < NCH; ++i) {
      if (sok[i]) {
        uint4 v = make_uint4(xr[i][0], xr[i][1], xr[i][2], xr[i][3]);
        if (PRO == CX_PRO_AFFINE_RELU) {
          const float* sc = coef + sch[i] * 8;
          v = cx_affine_relu8(v, sc, sc + K);
        }
        const unsigned keep = (tvalid && m0 + srow[i] < M) ? 0xffffffffu : 0u;   // rows past the end: zero (they add nothing to the sums)
        v.x &= keep; v.y &= keep; v.z &= keep; v.w &= keep;
        *reinterpret_cast<uint4*>(Xb + srow[i] * xp + sch[i] * 16) = v;
      }
    }
    request(mt + 2, xr);                          // the tile after next, into the set just handed over
    __syncthreads();                              // tile visible; the out tile of the previous tile has been stored
    // ---- D[channel][pixel] = W . X^T over K
    f32x16 acc;
#pragma unroll
    for (int r = 0; r < 16; ++r) acc[r] = 0.f;
    {
      const char* Ab = Xb + (pw * 32 + lrow) * xp + lh * 16;
      const char* Wb = Wt + (cq * 32 + lrow) * xp + lh * 16;
#pragma unroll
      for (int kk = 0; kk < K / 16; ++kk) {
        const bf16x8 af = *reinterpret_cast<const bf16x8*>(Ab + kk * 32);
        const bf16x8 wf = *reinterpret_cast<const bf16x8*>(Wb + kk * 32);
        acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(wf, af, acc, 0, 0, 0);
      }
    }
    // ---- accumulators -> bf16 rows of the out tile (lane = pixel, 8 consecutive channels after the swap) + channel sums
    const bool mv = tvalid && m0 + pw * 32 + lrow < M;
#pragma unroll
    for (int cc = 0; cc < 2; ++cc) {
      float t[8];
#pragma unroll
      for (int r4 = 0; r4 < 4; ++r4) {
        const auto sw = __builtin_amdgcn_permlane32_swap(__float_as_uint(acc[8 * cc + r4]), __float_as_uint(acc[8 * cc + 4 + r4]), false, false);
        t[r4] = __uint_as_float(sw[0]);
        t[4 + r4] = __uint_as_float(sw[1]);
      }
      const uint4 o = cx_pack8_stats(t, mv, want_stats, s1[cc], s2[cc]);
      *reinterpret_cast<uint4*>(Ol + (pw * 32 + lrow) * OP + (cq * 32 + 8 * (2 * cc + lh)) * 2) = o;
    }
    __syncthreads();                              // out tile complete; every wave is done with this X image
    // ---- the tile leaves as whole rows
#pragma unroll
    for (int i = 0; i < 2; ++i) {
      const int row = r0 + 32 * i;
      const uint4 o = *reinterpret_cast<const uint4*>(Ol + row * OP + q * 16);
      if (tvalid && m0 + row < M) *reinterpret_cast<uint4*>(Y + (size_t)(m0 + row) * p.ldy + q * 8) = o;
    }
  };

  const int n_pairs = (t1 - t0 + 1) >> 1;
  for (int pr = 0; pr < n_pairs; ++pr) {
    tile(t0 + 2 * pr, std::integral_constant<int, 0>{}, xa);
    tile(t0 + 2 * pr + 1, std::integral_constant<int, 1>{}, xb);
  }

  if (want_stats) {
    __syncthreads();                                             // (the last tile's row stores read Ol; Xl is free)
    float* scratch = reinterpret_cast<float*>(Xl);               // 8 waves x 2 x 128 floats = 8 KB <= one X image (K >= 32)
    wg_stat_begin<8>(scratch, NO, tid, NT);
    float t1v = 0.f, t2v = 0.f;
#pragma unroll
    for (int cc = 0; cc < 2; ++cc)
#pragma unroll
      for (int e = 0; e < 8; ++e) {
        const float a = half_sum(s1[cc][e]);
        const float b = half_sum(s2[cc][e]);
        if (lrow == 8 * cc + e) { t1v = a; t2v = b; }
      }
    if (lrow < 16) {
      const int n = cq * 32 + 8 * (2 * (lrow >> 3) + lh) + (lrow & 7);
      wg_stat_put(scratch, NO, wave, n, t1v, t2v);
    }
    wg_stat_end<8>(scratch, NO, tid, NT, p.stat_sum, p.stat_sq, p.stat_det, (int)blockIdx.x, p.stat_replicas, p.stat_rstride, 0, p.N);
  }
}

template <int PRO, int KT>
int launch_fwd2(const CxConv& p, hipStream_t st) {
  const long long M = (long long)p.B * p.Ho * p.Wo;
  const int m_tiles = (int)((M + BM - 1) / BM);
  int grid = m_tiles < 256 ? m_tiles : 256;              // one workgroup per CU, each walks a contiguous range of tiles
  const int tpw = (m_tiles + grid - 1) / grid;
  grid = (m_tiles + tpw - 1) / tpw;
  constexpr int xp = KT * 64 + 16;
  constexpr size_t smem = (size_t)2 * KT * 32 * 4 + (size_t)NO * xp + (size_t)2 * BM * xp + (size_t)BM * OP;
  static_assert(smem <= 160 * 1024, "LDS");
  static bool attr_set = false;
  if (!attr_set) {
    (void)hipFuncSetAttribute(reinterpret_cast<const void*>(&pw_fwd2_kernel<PRO, KT>), hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024);
    attr_set = true;
  }
  if (const int e = stat_rows_check(p, grid)) return e;
  CX_KTAG("pw_fwd2_kernel<%d, %d>", PRO, KT);
  hipLaunchKernelGGL((pw_fwd2_kernel<PRO, KT>), dim3(grid), dim3(NT), smem, st, p, (int)M, m_tiles, tpw);
  return launch_status();
}

template <int PRO>
int launch_fwd2_n(const CxConv& p, hipStream_t st) {
  switch (p.K / 32) {
    case 1: return launch_fwd2<PRO, 1>(p, st);
    case 2: return launch_fwd2<PRO, 2>(p, st);
    case 3: return launch_fwd2<PRO, 3>(p, st);
    case 4: return launch_fwd2<PRO, 4>(p, st);
    case 5: return launch_fwd2<PRO, 5>(p, st);
    case 6: return launch_fwd2<PRO, 6>(p, st);
    case 7: return launch_fwd2<PRO, 7>(p, st);
    default: return launch_fwd2<PRO, 8>(p, st);
  }
}



}  // namespace

// Called by cx_conv_gemm after its argument validation; *handled = false leaves the call to the kernels tried after this one.
int cx_try_pw_fwd2(const CxConv& p, hipStream_t st, bool* handled) {
  *handled = false;
  if (p.mode != CX_MODE_CONV || p.kh != 1 || p.kw != 1 || p.stride != 1 || p.pad != 0 || p.tstride > 1) return 0;
  // (K > 256 in the same design, K walked in 128-channel chunks, was measured in three forms and not kept: profiles/r04_pw_fwd3_rejected.txt)
  if (p.epilogue != CX_EPI_STORE || p.accumulate || p.N != NO || (p.K % 32) || p.K < 32 || p.K > 256) return 0;
  if (p.prologue != CX_PRO_AFFINE_RELU && p.prologue != CX_PRO_NONE) return 0;
  if (p.dtype != CX_DT_BF16) return 0;
  *handled = true;
  return p.prologue == CX_PRO_AFFINE_RELU ? launch_fwd2_n<CX_PRO_AFFINE_RELU>(p, st) : launch_fwd2_n<CX_PRO_NONE>(p, st);
}
