// Calibration of the predicted probabilities (include/chexpert_hip.h, cx_calib_fit / cx_boot_calib; chexpert_amd/calibration.py states
// both in numpy).  Two entry points:
//   cx_calib_fit   fits the per-class map u = a z + b (Platt scaling; b = 0: temperature scaling) by a damped Newton iteration on the
//                  mean logistic loss, every class in ONE launch and with no host round trip: one 256-thread workgroup per class.
//   cx_boot_calib  the bin sums behind ECE / MCE / Brier of every (replicate, class) over a bootstrap count table, in integers, held
//                  to calibration.calibration_sums_reference bit for bit.
// cx_calib_fit.  A pass strides the class's N rows (thread t the rows t, t + 256, ...) with fp64 partial sums: the loss, two gradient
// and three Hessian entries (the loss alone while a step is being halved).  The partials are reduced in ONE fixed order -- an xor
// butterfly inside the wave (32, 16, ... 1: every lane ends with the same sum), then the four waves through LDS in wave order -- so the
// result is the same bits on every run; there are no atomics.  Thread 0 then solves the 2x2 system and writes the next point and the
// continue / stop decision to LDS; every thread reads the decision from LDS behind the barrier, so every branch around a
// __syncthreads is workgroup-uniform.  The pass loop is bounded by max_iter * 42 + 2 (a full pass and at most 41 loss passes per
// iteration, one first pass), max_iter validated on the host to 1 .. 1000: the kernel terminates whatever the data.
// It is latency-bound on C workgroups (C = 5 .. 14 of 256 CUs) and that is accepted: the fit runs once per evaluation.  A pass costs
// one exp and one log1p in fp64 per row.  Measured on the MI355X (device events around ops.calib_fit, which
// also transposes the operands): 65 us at 234 rows x 5 classes and 575 us at 20 000 x 14, five iterations (six full passes and
// five loss passes) either way, temperature and Platt alike; the numpy statement takes 1.1 ms and 19 ms on the host.
// cx_boot_calib.  One wave per (replicate, class), the wave shape of boot_sweep_kernel: steps of 64 entries read coalesced with their
// fixed-point confidences, CALIB_STEPS steps' entries and the count-row gathers behind them requested before the first is consumed,
// unit indices clamped to U - 1 and bins to M - 1.  Bound, as the sweep: the two dependent memory latencies per block of steps (the
// entries, then the gather), not bytes.
// How a wave folds its lanes into the M bins: integer LDS accumulators per wave (uint32 weight, uint32 positive weight, uint64
// weight x confidence; 1 KB per wave), fed by RUN-LENGTH sums in registers.  calibration_plan lists a class ascending in confidence,
// so ascending in bin; lane l reads the entries l, l + 64, ... and therefore meets its bins in ascending order: it keeps the sums of
// its current bin in registers and adds them to the LDS slot (ds_add_u32 / ds_add_u64) only when the bin changes, at most M times per
// lane instead of once per entry.  The alternative -- segmented wave sums over the sorted plan -- needs three scans and a
// segment-end select per step where this needs three adds; an unsorted plan is still summed correctly (more flushes, same integers).
// Measured at M = 15 the flushes do not show: a plan shuffled inside every class (a flush at almost every entry) takes 5.41 ms where
// the sorted one takes 5.40 -- the gather is the bound.  The run-length form is kept for small M, where all 64 lanes of a step would
// otherwise add to one LDS address; it costs one compare per entry.
// Integer adds commute, so the LDS atomics give the same bits every run -- the project's rule is about the order of FLOAT sums, of
// which cx_boot_calib has none.  Every output element has one writer (lane b of the wave stores bin b).
// Measured (device events around ops.boot_calib, M = 15, beside cx_boot_sweep without operating points in the
// same process, alternating): 5.40 ms against 5.36 ms at 20 000 rows x 14 classes x 2000 replicates (equal-mass bins: 5.39 ms), 41 us
// against 44 us at 234 x 5 x 1000 (launch latency).  The numpy statement: 13 ms for the 1000 replicates of the small shape, 155 ms per
// 128 replicates of the large one.
#include "resample.h"

namespace {

// ---- cx_calib_fit -----------------------------------------------------------------------------------------------------------------
constexpr int FIT_HALVINGS = 40;
constexpr double FIT_RIDGE = 1e-12;       // H + 1e-12 I
constexpr double FIT_FLAT = 1e-8;         // smallest eigenvalue below this: status 3
constexpr double FIT_SLACK = 1e-12;       // a candidate loss "rises" when it exceeds L (1 + 1e-12): above the rounding of an N-term sum

enum { FIT_FULL = 0, FIT_LOSS = 1, FIT_DONE = 2 };

__device__ __forceinline__ double fit_wave_sum(double v) {
#pragma unroll
  for (int d = 32; d >= 1; d >>= 1) v += __shfl_xor(v, d);
  return v;
}

__global__ __launch_bounds__(256) void calib_fit_kernel(const float* __restrict__ logits, const float* __restrict__ targets, int N,
                                                        int platt, int smooth, double g_tol, int max_iter, double* __restrict__ out) {
  __shared__ double red[4][6];
  __shared__ double s_a, s_b;            // the point the next pass evaluates
  __shared__ double s_tp, s_tn;          // the targets of a positive / a negative
  __shared__ int s_mode;
  __shared__ unsigned s_cnt[4][2];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const float* __restrict__ z = logits + (size_t)blockIdx.x * N;
  const float* __restrict__ y = targets + (size_t)blockIdx.x * N;
  double* __restrict__ o = out + (size_t)blockIdx.x * 8;

  // kept positives and negatives (integers)
  unsigned np = 0, nn = 0;
  for (int i = tid; i < N; i += 256) {
    const float t = y[i];
    if (t >= 0.f) {
      if (t > 0.5f) ++np;
      else ++nn;
    }
  }
#pragma unroll
  for (int d = 32; d >= 1; d >>= 1) np += (unsigned)__shfl_xor((int)np, d), nn += (unsigned)__shfl_xor((int)nn, d);
  if (lane == 0) s_cnt[wave][0] = np, s_cnt[wave][1] = nn;
  __syncthreads();
  if (tid == 0) {
    np = s_cnt[0][0] + s_cnt[1][0] + s_cnt[2][0] + s_cnt[3][0];
    nn = s_cnt[0][1] + s_cnt[1][1] + s_cnt[2][1] + s_cnt[3][1];
    s_cnt[0][0] = np, s_cnt[0][1] = nn;
    s_tp = smooth ? ((double)np + 1.0) / ((double)np + 2.0) : 1.0;
    s_tn = smooth ? 1.0 / ((double)nn + 2.0) : 0.0;
    s_a = 1.0, s_b = 0.0;
    s_mode = FIT_FULL;
  }
  __syncthreads();
  np = s_cnt[0][0], nn = s_cnt[0][1];                            // workgroup-uniform: read from LDS behind the barrier
  const double tpos = s_tp, tneg = s_tn;
  const double inv_n = 1.0 / (double)(np + nn);                  // inf for an empty class: only the loss of the identity uses it
  const bool degenerate = np == 0u || nn == 0u;

  // thread 0's iteration state (registers; the other threads carry dead copies)
  double a = 1.0, b = 0.0, L = 0.0, da = 0.0, db = 0.0, step = 1.0, nll0 = 0.0, gmax = 0.0, lmin = 0.0;
  int it = 0, halvings = 0, status = 0;

  const long long max_pass = (long long)max_iter * (FIT_HALVINGS + 2) + 2;
  for (long long pass = 0; pass < max_pass; ++pass) {
    const int mode = s_mode;                                     // uniform: written by thread 0 before the last barrier
    if (mode == FIT_DONE) break;
    const double pa = s_a, pb = s_b;
    double sl = 0.0, ga = 0.0, gb = 0.0, haa = 0.0, hab = 0.0, hbb = 0.0;
    for (int i = tid; i < N; i += 256) {
      const float tf = y[i];
      if (!(tf >= 0.f)) continue;
      const double x = (double)z[i], t = tf > 0.5f ? tpos : tneg;
      const double u = pa * x + pb;
      const double e = exp(-fabs(u));
      sl += (fmax(u, 0.0) + log1p(e)) - t * u;
      if (mode == FIT_FULL) {
        const double q = 1.0 / (1.0 + e);
        const double p = u >= 0.0 ? q : e * q;                   // sigmoid(u)
        const double w = e * q * q;                              // p (1 - p)
        const double r = p - t;
        ga += r * x, gb += r;
        haa += w * x * x, hab += w * x, hbb += w;
      }
    }
    sl = fit_wave_sum(sl);
    if (mode == FIT_FULL) ga = fit_wave_sum(ga), gb = fit_wave_sum(gb), haa = fit_wave_sum(haa), hab = fit_wave_sum(hab), hbb = fit_wave_sum(hbb);
    if (lane == 0) red[wave][0] = sl, red[wave][1] = ga, red[wave][2] = gb, red[wave][3] = haa, red[wave][4] = hab, red[wave][5] = hbb;
    __syncthreads();
    if (tid == 0) {
      double v[6];
#pragma unroll
      for (int k = 0; k < 6; ++k) v[k] = (((red[0][k] + red[1][k]) + red[2][k]) + red[3][k]) * inv_n;
      int next = FIT_FULL;
      if (mode == FIT_FULL) {
        L = v[0];
        if (pass == 0) nll0 = L;
        if (!platt) v[2] = 0.0;
        gmax = fmax(fabs(v[1]), fabs(v[2]));
        if (platt) lmin = 0.5 * (v[3] + v[5]) - sqrt(0.25 * (v[3] - v[5]) * (v[3] - v[5]) + v[4] * v[4]);
        else lmin = v[3];
        if (degenerate) status = 2, next = FIT_DONE;
        else if (gmax <= g_tol) status = 0, next = FIT_DONE;
        else if (it >= max_iter) status = 1, next = FIT_DONE;
        else {
          if (platt) {
            const double h00 = v[3] + FIT_RIDGE, h11 = v[5] + FIT_RIDGE, h01 = v[4];
            const double det = h00 * h11 - h01 * h01;
            da = (h11 * v[1] - h01 * v[2]) / det, db = (h00 * v[2] - h01 * v[1]) / det;
          } else {
            da = v[1] / (v[3] + FIT_RIDGE), db = 0.0;
          }
          step = 1.0, halvings = 0;
          s_a = a - da, s_b = b - db;
          next = FIT_LOSS;
        }
      } else {                                                   // the loss of a candidate
        const double Lc = v[0];
        const bool finite = Lc - Lc == 0.0;
        if (finite && Lc <= L + FIT_SLACK * fabs(L)) {
          a = s_a, b = s_b, ++it;                                // accepted; the full pass at the new point follows
        } else if (halvings >= FIT_HALVINGS) {
          if (finite) a = s_a, b = s_b;                          // the last, 2^-40, step is taken; a non-finite one is not
          ++it;
          s_a = a, s_b = b;
        } else {
          step *= 0.5, ++halvings;
          s_a = a - step * da, s_b = b - step * db;
          next = FIT_LOSS;
        }
      }
      s_mode = next;
    }
    __syncthreads();
  }
  if (tid == 0) {
    double nll1 = L;
    if (status == 2) gmax = lmin = __builtin_nan("");
    else if (!(lmin >= FIT_FLAT)) status = 3;
    if (status >= 2) a = 1.0, b = 0.0, nll1 = nll0;               // the identity is returned, with its loss
    if (np + nn == 0u) nll0 = nll1 = __builtin_nan("");
    o[0] = a, o[1] = b, o[2] = nll0, o[3] = nll1, o[4] = gmax, o[5] = lmin, o[6] = (double)it, o[7] = (double)status;
  }
}

// ---- cx_boot_calib ----------------------------------------------------------------------------------------------------------------
constexpr int CALIB_STEPS = 4;
constexpr int CALIB_BINS = CX_CALIB_MAX_BINS;

__global__ __launch_bounds__(256) void boot_calib_kernel(const uint32_t* __restrict__ counts, int ld, int n_rep,
                                                         const int32_t* __restrict__ order, const uint32_t* __restrict__ conf,
                                                         const ClassLists plan, int c0, int cn, int C, int M, uint32_t* __restrict__ wsum,
                                                         uint32_t* __restrict__ wpos, uint64_t* __restrict__ csum,
                                                         uint64_t* __restrict__ bnum, int U) {
  __shared__ unsigned long long s_c[4][CALIB_BINS];
  __shared__ uint32_t s_w[4][CALIB_BINS], s_p[4][CALIB_BINS];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const long long item = (long long)blockIdx.x * 4 + wave;
  const bool active = item < (long long)n_rep * cn;              // the same for all lanes of a wave; an idle wave still meets the barriers
  const int rep = active ? (int)(item / cn) : 0, cl = active ? (int)(item - (long long)rep * cn) : 0;
  const int n = active ? plan.len[cl] : 0;
  const int32_t* __restrict__ ent = order + plan.offs[cl];
  const uint32_t* __restrict__ cf = conf + plan.offs[cl];
  const uint32_t* __restrict__ row = counts + (size_t)rep * ld;
  s_c[wave][lane] = 0ull, s_w[wave][lane] = 0u, s_p[wave][lane] = 0u;      // CALIB_BINS == 64: one slot per lane
  __syncthreads();
  uint64_t bn = 0, rc = 0;                                       // Brier numerator; the run's weight x confidence
  uint32_t rw = 0, rp = 0;                                       // the run's weight and positive weight
  int cur = 0;
  for (int t0 = 0; t0 < n; t0 += 64 * CALIB_STEPS) {
    int32_t e[CALIB_STEPS];
    uint32_t P[CALIB_STEPS], w[CALIB_STEPS];
#pragma unroll
    for (int s = 0; s < CALIB_STEPS; ++s) {
      const int tc = min(t0 + s * 64 + lane, n - 1);             // past the end: the last entry again (in bounds), weighed 0 below
      e[s] = ent[tc], P[s] = cf[tc];
    }
#pragma unroll
    for (int s = 0; s < CALIB_STEPS; ++s) w[s] = row[min(e[s] & 0xffffff, U - 1)];       // unit indices are clamped, never trusted
#pragma unroll
    for (int s = 0; s < CALIB_STEPS; ++s) {
      const uint32_t a = t0 + s * 64 + lane < n ? w[s] : 0u;
      const bool pos = e[s] < 0;                                 // bit 31 = the label
      const int bin = min((e[s] >> 24) & 63, M - 1);
      if (bin != cur) {
        if (rw != 0u) atomicAdd(&s_w[wave][cur], rw), atomicAdd(&s_p[wave][cur], rp), atomicAdd(&s_c[wave][cur], (unsigned long long)rc);
        cur = bin, rw = 0u, rp = 0u, rc = 0ull;
      }
      rw += a, rp += pos ? a : 0u, rc += (uint64_t)a * (uint64_t)P[s];
      const uint32_t d = pos ? 0xffffffffu - P[s] : P[s];
      bn += (uint64_t)a * (uint64_t)__umulhi(d, d);
    }
  }
  if (rw != 0u) atomicAdd(&s_w[wave][cur], rw), atomicAdd(&s_p[wave][cur], rp), atomicAdd(&s_c[wave][cur], (unsigned long long)rc);
  bn = wave_sum_u64(bn);
  __syncthreads();
  if (active) {
    const size_t o = (size_t)rep * C + c0 + cl;
    if (lane < M) wsum[o * M + lane] = s_w[wave][lane], wpos[o * M + lane] = s_p[wave][lane], csum[o * M + lane] = s_c[wave][lane];
    if (lane == 0) bnum[o] = bn;
  }
}

}  // namespace

int cx_calib_fit(const float* logits, const float* targets, int C, int N, int method, int smooth, double g_tol, int max_iter, double* out,
                 void* stream) {
  if (C < 0 || N < 0 || (method != CX_CALIB_TEMPERATURE && method != CX_CALIB_PLATT) || max_iter < 1 || max_iter > CX_CALIB_MAX_ITER ||
      !(g_tol >= 0.0))
    return CX_EINVAL;
  if (C == 0 || N == 0) return 0;
  if (!logits || !targets || !out) return CX_EINVAL;
  if ((((uintptr_t)logits) & 3) || (((uintptr_t)targets) & 3) || (((uintptr_t)out) & 7)) return CX_EALIGN;
  hipLaunchKernelGGL(calib_fit_kernel, dim3((unsigned)C), dim3(256), 0, as_stream(stream), logits, targets, N,
                     method == CX_CALIB_PLATT ? 1 : 0, smooth ? 1 : 0, g_tol, max_iter, out);
  return launch_status();
}

int cx_boot_calib(const uint32_t* counts, int ld, int n_rep, const int32_t* order, const uint32_t* conf, const int64_t* offs,
                  const int32_t* len, int C, int M, uint32_t* wsum, uint32_t* wpos, uint64_t* csum, uint64_t* bnum, int U, void* stream) {
  if (!counts || !order || !conf || !offs || !len || !wsum || !wpos || !csum || !bnum || n_rep < 1 || C < 1) return CX_EINVAL;
  if (M < 1 || M > CALIB_BINS) return CX_ESHAPE;
  if (const int rc = check_class_lists(U, ld, offs, len, C)) return rc;
  if ((((uintptr_t)counts) & 3) || (((uintptr_t)order) & 3) || (((uintptr_t)conf) & 3) || (((uintptr_t)wsum) & 3) || (((uintptr_t)wpos) & 3) ||
      (((uintptr_t)csum) & 7) || (((uintptr_t)bnum) & 7))
    return CX_EALIGN;
  if (((long long)n_rep * CX_LIST_CLASSES + 3) / 4 > 0x7fffffffll) return CX_ESHAPE;
  ClassLists plan;
  return for_class_groups(offs, len, C, plan, [&](int c0, int cn) {
    const long long waves = (long long)n_rep * cn;
    hipLaunchKernelGGL(boot_calib_kernel, dim3((unsigned)((waves + 3) / 4)), dim3(256), 0, as_stream(stream), counts, ld, n_rep, order,
                       conf, plan, c0, cn, C, M, wsum, wpos, csum, bnum, U);
  });
}
