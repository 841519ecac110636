// Class-specific residual attention head (CSRA; Zhu & Wu, ICCV 2021): the classifier applied at every pixel of the last feature map,
// the score map pooled per class by its mean plus lambda times a softmax-weighted mean.  The definition stands in
// include/chexpert_hip.h beside the entry points; chexpert_amd/heads.py restates it in numpy.
//
// Forward, two launches.  csra_score_kernel: s[b,k,p] = sum_c W[k,c] a[b,p,c], a skinny GEMM in fp32 on the VALU (the activated operand
// is NOT rounded to bf16: the average head sums it in fp32, and lambda = 0 is that head).  A wave owns 4 pixel rows, a lane 8 channels
// of a 512-channel chunk; the 16 x 512 tile of W comes through LDS; a lane adds its channels in ascending order, the 64 lanes are
// added by an xor butterfly: a fixed order.  csra_stat_kernel: one wave per (image, class) finds max_p s, the softmax sums relative to
// it and the logit.  What it leaves for the way back is relative to the maximum as well (attoff = att - max): beside a score of 1e4
// the rounding of att itself would cost 1e-3 of s - att.
//
// Backward, three launches.  csra_ds_kernel writes ds (B*HW, NT) into the caller's scratch, NT = n rounded up to 16 / 32 / 64, zero
// behind n.  csra_bwd_kernel: one thread per CH channels (CH * NT = 64) of a group of images walks their pixels once: x is read once,
// g written once, W's columns and the weight-gradient partial sums live in registers, ds is the same address for the whole wave.
// Every sum of one (image, channel) is formed by one thread in ascending pixel order; the weight gradient leaves as one partial per
// group of images, which csra_reduce_kernel adds in ascending group order (and db in ascending image order): no atomics on dW / db,
// two calls give equal bits.
//
// Probabilistic-CAM pooling head (PCAM; Ye et al. 2020), FusedNet.set_head("pcam"): the same score map, pooled per class with the
// per-pixel probabilities sigmoid(s + bias) as weights.  Forward: csra_score_kernel as it is, then pcam_stat_kernel, one wave per
// (image, class).  Backward: pcam_ds_kernel, one workgroup per image, writes ds and dl_eff = dlogit (1 + r) (the bias sits inside
// the sigmoid, so db is not the sum of dlogit), then csra_bwd_kernel and csra_reduce_kernel unchanged, the reduce reading dl_eff.  What the stat kernel leaves is
// relative to the row's largest u = s + bias, as csra's is to max_p s.
#include <limits.h>
#include <math.h>
#include "common.h"

namespace {

constexpr int CS_KT = 16;                    // classes per tile of the score kernel
constexpr int CS_PT = 4;                     // pixel rows per wave
constexpr int CS_WAVES = 8;
constexpr int CS_CK = 512;                   // channels per chunk: 64 lanes x 8
constexpr int CS_THREADS = CS_WAVES * 64;
constexpr int CS_STAT = 4;                   // floats per (image, class): max_p s, 1 / sum exp, att - max, unused
constexpr int CS_GROUPS = 128;               // at most this many weight-gradient partials

__device__ __forceinline__ float cs_sigmoid(float z) { return 1.f / (1.f + expf(-z)); }
__device__ __forceinline__ float cs_act(float z, int act) { return act == CX_POOL_ACT_SWISH ? z * cs_sigmoid(z) : fmaxf(z, 0.f); }
__device__ __forceinline__ float cs_dact(float z, int act) {
  if (act == CX_POOL_ACT_SWISH) {
    const float s = cs_sigmoid(z);
    return s * (1.f + z * (1.f - s));
  }
  return z > 0.f ? 1.f : 0.f;
}

__device__ __forceinline__ float cs_wave_sum(float v) {
#pragma unroll
  for (int o = 32; o >= 1; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}
__device__ __forceinline__ float cs_wave_max(float v) {
#pragma unroll
  for (int o = 32; o >= 1; o >>= 1) v = fmaxf(v, __shfl_xor(v, o, 64));
  return v;
}

// CH consecutive channels of the storage type
template <typename T, int CH> struct __attribute__((aligned(sizeof(T) * CH))) VC { T e[CH]; };
__device__ __forceinline__ float cs_f(bf16 v) { return bf2f(v); }
__device__ __forceinline__ float cs_f(float v) { return v; }
__device__ __forceinline__ void cs_set(bf16& d, float v) { d = f2bf(v); }
__device__ __forceinline__ void cs_set(float& d, float v) { d = v; }

template <typename T>
__global__ __launch_bounds__(CS_THREADS) void csra_score_kernel(const T* __restrict__ x, const float* __restrict__ sc, const float* __restrict__ sh,
                                                                const float* __restrict__ m, const float* __restrict__ W, float* __restrict__ s,
                                                                size_t rows, int HW, int C, int ldx, int n, int act) {
  __shared__ float wl[CS_KT][CS_CK];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const size_t row0 = ((size_t)blockIdx.x * CS_WAVES + wave) * CS_PT;
  for (int k0 = 0; k0 < n; k0 += CS_KT) {
    float acc[CS_PT][CS_KT];
#pragma unroll
    for (int r = 0; r < CS_PT; ++r)
#pragma unroll
      for (int kk = 0; kk < CS_KT; ++kk) acc[r][kk] = 0.f;
    for (int c0 = 0; c0 < C; c0 += CS_CK) {
      __syncthreads();                                       // the tile before this one has been consumed
      for (int i = threadIdx.x; i < CS_KT * CS_CK; i += CS_THREADS) {
        const int kk = i / CS_CK, cc = i % CS_CK;
        wl[kk][cc] = (k0 + kk < n && c0 + cc < C) ? W[(size_t)(k0 + kk) * C + c0 + cc] : 0.f;
      }
      __syncthreads();
      const int c = c0 + lane * 8;
      const int nv = C - c < 8 ? C - c : 8;                 // 8, 4 (fp32 storage: C % 4 == 0) or <= 0
      if (nv <= 0) continue;                                 // (the barriers above are outside this branch)
      float fsc[8], fsh[8], a[CS_PT][8];
#pragma unroll
      for (int j = 0; j < 8; ++j) { fsc[j] = j < nv ? sc[c + j] : 0.f; fsh[j] = j < nv ? sh[c + j] : 0.f; }
#pragma unroll
      for (int r = 0; r < CS_PT; ++r) {
#pragma unroll
        for (int j = 0; j < 8; ++j) a[r][j] = 0.f;
        const size_t row = row0 + r;
        if (row >= rows) continue;
        const T* px = x + row * ldx + c;
        const float* pm = m ? m + (row / HW) * C + c : nullptr;
        const VC<T, 4> lo = *reinterpret_cast<const VC<T, 4>*>(px);
#pragma unroll
        for (int j = 0; j < 4; ++j) a[r][j] = cs_act(fmaf(cs_f(lo.e[j]), fsc[j], fsh[j]), act) * (pm ? pm[j] : 1.f);
        if (nv == 8) {
          const VC<T, 4> hi = *reinterpret_cast<const VC<T, 4>*>(px + 4);
#pragma unroll
          for (int j = 0; j < 4; ++j) a[r][4 + j] = cs_act(fmaf(cs_f(hi.e[j]), fsc[4 + j], fsh[4 + j]), act) * (pm ? pm[4 + j] : 1.f);
        }
      }
#pragma unroll
      for (int kk = 0; kk < CS_KT; ++kk) {
        float w[8];
#pragma unroll
        for (int j = 0; j < 8; ++j) w[j] = wl[kk][lane * 8 + j];
#pragma unroll
        for (int r = 0; r < CS_PT; ++r)
#pragma unroll
          for (int j = 0; j < 8; ++j) acc[r][kk] = fmaf(w[j], a[r][j], acc[r][kk]);
      }
    }
    float out = 0.f;                                          // lane r * KT + kk keeps the sum of (row r, class k0 + kk)
#pragma unroll
    for (int r = 0; r < CS_PT; ++r)
#pragma unroll
      for (int kk = 0; kk < CS_KT; ++kk) {
        const float v = cs_wave_sum(acc[r][kk]);
        if (lane == r * CS_KT + kk) out = v;
      }
    const size_t row = row0 + lane / CS_KT;
    const int k = k0 + lane % CS_KT;
    if (row < rows && k < n) s[((row / HW) * n + k) * HW + row % HW] = out;
  }
}

__global__ __launch_bounds__(256) void csra_stat_kernel(const float* __restrict__ s, const float* __restrict__ bias, const float* __restrict__ lt,
                                                        float* __restrict__ logits, float* __restrict__ stat, size_t BN, int n, int HW) {
  const int lane = threadIdx.x & 63;
  const size_t idx = (size_t)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (idx >= BN) return;                                      // (whole waves leave; no barrier below)
  const float* row = s + idx * HW;
  float mx = -INFINITY;
  for (int p = lane; p < HW; p += 64) mx = fmaxf(mx, row[p]);
  mx = cs_wave_max(mx);
  const float lam = lt[0], T = lt[1];
  float z = 0.f, t = 0.f, sm = 0.f;
  for (int p = lane; p < HW; p += 64) {
    const float d = row[p] - mx, e = expf(T * d);
    z += e;
    t += e * d;
    sm += row[p];
  }
  z = cs_wave_sum(z);
  t = cs_wave_sum(t);
  sm = cs_wave_sum(sm);
  if (lane == 0) {
    const float off = t / z;                                  // att - max <= 0
    logits[idx] = (bias ? bias[idx % n] : 0.f) + sm / (float)HW + lam * (mx + off);
    float* st = stat + idx * CS_STAT;
    st[0] = mx; st[1] = 1.f / z; st[2] = off; st[3] = 0.f;
  }
}

// ds[(b HW + p) NT + k] = dlogit[b,k] (1/HW + lambda w (1 + T (s - att))), 0 for k >= n
__global__ __launch_bounds__(256) void csra_ds_kernel(const float* __restrict__ dl, const float* __restrict__ s, const float* __restrict__ stat,
                                                      const float* __restrict__ lt, float* __restrict__ ds, size_t total, int n, int HW, int NT) {
  const size_t idx = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (idx >= total) return;
  const int k = idx % NT;
  const size_t bp = idx / NT, b = bp / HW, p = bp % HW;
  float v = 0.f;
  if (k < n) {
    const float lam = lt[0], T = lt[1];
    const size_t bk = b * n + k;
    const float* st = stat + bk * CS_STAT;
    const float d = s[bk * HW + p] - st[0];
    const float w = expf(T * d) * st[1];
    v = dl[bk] * (1.f / (float)HW + lam * w * (1.f + T * (d - st[2])));
  }
  ds[idx] = v;
}

template <typename T, int NT, int CH>
__global__ __launch_bounds__(256) void csra_bwd_kernel(const float* __restrict__ ds, const T* __restrict__ x, const float* __restrict__ sc,
                                                       const float* __restrict__ sh, const float* __restrict__ m, const float* __restrict__ mean,
                                                       const float* __restrict__ rstd, const float* __restrict__ escale, const float* __restrict__ W,
                                                       T* __restrict__ g, float* S1, float* S2, float* __restrict__ part, int B, int HW, int C,
                                                       int ldx, int ldg, int n, int act, int det, int GB) {
  const int c = (blockIdx.x * blockDim.x + threadIdx.x) * CH;
  if (c >= C) return;                                         // (no barrier in this kernel)
  const int grp = blockIdx.y, b0 = grp * GB, b1 = b0 + GB < B ? b0 + GB : B;
  float w[NT][CH], acc[NT][CH], fsc[CH], fsh[CH], fmu[CH], fr[CH], fe[CH];
#pragma unroll
  for (int k = 0; k < NT; ++k)
#pragma unroll
    for (int j = 0; j < CH; ++j) { w[k][j] = k < n ? W[(size_t)k * C + c + j] : 0.f; acc[k][j] = 0.f; }
#pragma unroll
  for (int j = 0; j < CH; ++j) { fsc[j] = sc[c + j]; fsh[j] = sh[c + j]; fmu[j] = mean[c + j]; fr[j] = rstd[c + j]; fe[j] = escale[c + j]; }
  for (int b = b0; b < b1; ++b) {
    float fm[CH], s1[CH], s2[CH];
#pragma unroll
    for (int j = 0; j < CH; ++j) { fm[j] = m ? m[(size_t)b * C + c + j] : 1.f; s1[j] = s2[j] = 0.f; }
    for (int p = 0; p < HW; ++p) {
      const size_t row = (size_t)b * HW + p;
      const float* d = ds + row * NT;                         // one address for the whole workgroup
      const VC<T, CH> v = *reinterpret_cast<const VC<T, CH>*>(x + row * ldx + c);
      float xf[CH], a[CH], da[CH], dac[CH];
#pragma unroll
      for (int j = 0; j < CH; ++j) {
        xf[j] = cs_f(v.e[j]);
        const float z = fmaf(xf[j], fsc[j], fsh[j]);
        a[j] = cs_act(z, act) * fm[j];
        dac[j] = cs_dact(z, act) * fm[j];
        da[j] = 0.f;
      }
#pragma unroll
      for (int k = 0; k < NT; ++k) {
        const float dk = d[k];
#pragma unroll
        for (int j = 0; j < CH; ++j) {
          da[j] = fmaf(dk, w[k][j], da[j]);
          acc[k][j] = fmaf(dk, a[j], acc[k][j]);
        }
      }
      VC<T, CH> o;
#pragma unroll
      for (int j = 0; j < CH; ++j) {
        const float dz = da[j] * dac[j];
        s1[j] += dz;
        s2[j] += dz * (xf[j] - fmu[j]) * fr[j];
        cs_set(o.e[j], fe[j] * dz);
      }
      *reinterpret_cast<VC<T, CH>*>(g + row * ldg + c) = o;
    }
#pragma unroll
    for (int j = 0; j < CH; ++j) {
      if (det) {                                              // row = image: B rows of C sums, one writer per element
        S1[(size_t)b * C + c + j] = s1[j];
        S2[(size_t)b * C + c + j] = s2[j];
      } else {
        atomicAdd(&S1[c + j], s1[j]);
        atomicAdd(&S2[c + j], s2[j]);
      }
    }
  }
#pragma unroll
  for (int k = 0; k < NT; ++k)
    if (k < n) {
#pragma unroll
      for (int j = 0; j < CH; ++j) part[((size_t)grp * n + k) * C + c + j] = acc[k][j];
    }
}

// dW[i] += sum over the groups in ascending order, db[k] += sum over the images in ascending order
__global__ __launch_bounds__(256) void csra_reduce_kernel(const float* __restrict__ part, const float* __restrict__ dl, float* dW, float* db,
                                                          int groups, int B, int n, size_t nC) {
  const size_t idx = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (idx < nC) {
    float v = 0.f;
    for (int gq = 0; gq < groups; ++gq) v += part[(size_t)gq * nC + idx];
    dW[idx] += v;
  } else if (db && idx < nC + n) {
    const int k = idx - nC;
    float v = 0.f;
    for (int b = 0; b < B; ++b) v += dl[(size_t)b * n + k];
    db[k] += v;
  }
}

// sigmoid(u), sigmoid(-u) and log sigmoid(u) from one exp(-|u|): nothing cancels and nothing overflows
struct PcSig { float p, q, l; };
__device__ __forceinline__ PcSig pc_sig(float u) {
  const float t = expf(-fabsf(u)), inv = 1.f / (1.f + t), hi = inv, lo = t * inv;
  PcSig r;
  r.p = u >= 0.f ? hi : lo;
  r.q = u >= 0.f ? lo : hi;
  r.l = fminf(u, 0.f) - log1pf(t);
  return r;
}

// One wave per (image, class).  u = s + bias, L = log sigmoid(u), w = exp(L - max L) / sum, logit = sum w u.  stat = [max_p u,
// 1 / sum_p exp(L - max L), logit - max u, bias]: relative to the largest u of the row (L is monotone in u, so max L = L(max u), which
// the way back recomputes from stat[0]); the bias rides along because the way back has the csra argument list, which has none.
__global__ __launch_bounds__(256) void pcam_stat_kernel(const float* __restrict__ s, const float* __restrict__ bias, float* __restrict__ logits,
                                                        float* __restrict__ stat, size_t BN, int n, int HW) {
  const int lane = threadIdx.x & 63;
  const size_t idx = (size_t)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (idx >= BN) return;                                      // (whole waves leave; no barrier below)
  const float* row = s + idx * HW;
  const float bk = bias ? bias[idx % n] : 0.f;
  float mx = -INFINITY;
  for (int p = lane; p < HW; p += 64) mx = fmaxf(mx, row[p] + bk);
  mx = cs_wave_max(mx);
  const float lmx = pc_sig(mx).l;
  float z = 0.f, t = 0.f;
  for (int p = lane; p < HW; p += 64) {
    const float u = row[p] + bk, e = expf(pc_sig(u).l - lmx);
    z += e;
    t += e * (u - mx);
  }
  z = cs_wave_sum(z);
  t = cs_wave_sum(t);
  if (lane == 0) {
    const float off = t / z;                                  // logit - max u <= 0
    logits[idx] = mx + off;
    float* st = stat + idx * CS_STAT;
    st[0] = mx; st[1] = 1.f / z; st[2] = off; st[3] = bk;
  }
}

// One workgroup per image.  ds[(b HW + p) NT + k] = dlogit[b,k] w (1 + q (u - logit)), q = sigmoid(-u), 0 for k >= n, and
// dl_eff[b,k] = dlogit[b,k] (1 + r), r = sum_p w q (u - logit).  A thread keeps one class (256 % NT == 0) and walks its pixels in
// ascending order; the 256 / NT partial sums of a class are added in ascending thread order: a fixed order, no atomics.
__global__ __launch_bounds__(256) void pcam_ds_kernel(const float* __restrict__ dl, const float* __restrict__ s, const float* __restrict__ stat,
                                                      float* __restrict__ ds, float* __restrict__ dleff, int n, int HW, int NT) {
  __shared__ float red[256];
  const size_t b = blockIdx.x;
  const int k = threadIdx.x % NT, per = 256 / NT;
  float r = 0.f;
  if (k < n) {
    const size_t bk = b * n + k;
    const float* st = stat + bk * CS_STAT;
    const float mx = st[0], rz = st[1], off = st[2], bias = st[3], d = dl[bk], lmx = pc_sig(mx).l;
    for (int p = threadIdx.x / NT; p < HW; p += per) {
      const float u = s[bk * HW + p] + bias;
      const PcSig g = pc_sig(u);
      const float w = expf(g.l - lmx) * rz, t = g.q * ((u - mx) - off);
      r = fmaf(w, t, r);
      ds[(b * HW + p) * NT + k] = d * w * (1.f + t);
    }
  } else {
    for (int p = threadIdx.x / NT; p < HW; p += per) ds[(b * HW + p) * NT + k] = 0.f;
  }
  red[threadIdx.x] = r;
  __syncthreads();                                            // (every thread of the workgroup arrives)
  if (threadIdx.x < n) {
    float v = 0.f;
    for (int j = 0; j < per; ++j) v += red[j * NT + threadIdx.x];
    dleff[b * n + threadIdx.x] = dl[b * n + threadIdx.x] * (1.f + v);
  }
}

bool known_act(int act) { return act == CX_POOL_ACT_RELU || act == CX_POOL_ACT_SWISH; }
template <typename T> bool shape_ok(int B, int HW, int C, int ld) {
  const int q = sizeof(T) == 2 ? 8 : 4;
  return B > 0 && HW > 0 && C > 0 && C % q == 0 && ld % q == 0 && ld >= C;
}
int nt_of(int n) { return n <= 16 ? 16 : n <= 32 ? 32 : 64; }
int group_size(int B) { return (B + CS_GROUPS - 1) / CS_GROUPS; }

enum Head { CSRA, PCAM };                                     // pcam: no [lambda, T]; its backward keeps dl_eff (B n) behind the partials

long long scratch_floats(Head head, int B, int HW, int C, int n) {
  const int GB = group_size(B), groups = (B + GB - 1) / GB;
  return (long long)B * HW * nt_of(n) + (long long)groups * n * C + (head == PCAM ? (long long)B * n : 0);
}

long long bwd_scratch(Head head, int B, int HW, int C, int n) {
  if (B <= 0 || HW <= 0 || C <= 0 || n < 1) return CX_ESHAPE;
  if (n > CX_CSRA_MAX_CLASSES) return CX_EUNSUPPORTED;
  return scratch_floats(head, B, HW, C, n);
}

template <typename T>
int head_fwd_t(Head head, const void* x, const float* sc, const float* sh, const float* m, const float* W, const float* bias,
               const float* lam_T, float* logits, float* s, float* stat, int B, int HW, int C, int ldx, int n, int act, void* stream) {
  if (!x || !sc || !sh || !W || (head == CSRA && !lam_T) || !logits || !s || !stat || !known_act(act)) return CX_EINVAL;
  if (n < 1 || !shape_ok<T>(B, HW, C, ldx)) return CX_ESHAPE;
  if (n > CX_CSRA_MAX_CLASSES) return CX_EUNSUPPORTED;
  if (!aligned16(x)) return CX_EALIGN;
  const size_t rows = (size_t)B * HW, per = CS_WAVES * CS_PT, BN = (size_t)B * n;
  hipLaunchKernelGGL((csra_score_kernel<T>), dim3((rows + per - 1) / per), dim3(CS_THREADS), 0, as_stream(stream), (const T*)x, sc, sh, m, W, s,
                     rows, HW, C, ldx, n, act);
  if (head == CSRA)
    hipLaunchKernelGGL(csra_stat_kernel, dim3((BN + 3) / 4), dim3(256), 0, as_stream(stream), s, bias, lam_T, logits, stat, BN, n, HW);
  else
    hipLaunchKernelGGL(pcam_stat_kernel, dim3((BN + 3) / 4), dim3(256), 0, as_stream(stream), s, bias, logits, stat, BN, n, HW);
  return launch_status();
}

template <typename T, int NT, int CH>
void launch_bwd(const float* ds, const void* x, const float* sc, const float* sh, const float* m, const float* mean, const float* rstd,
                const float* e_scale, const float* W, void* g, float* S1, float* S2, float* part, int B, int HW, int C, int ldx, int ldg, int n,
                int act, int det, int GB, int groups, hipStream_t st) {
  const int owners = C / CH, threads = owners >= 256 ? 256 : (owners + 63) / 64 * 64;
  hipLaunchKernelGGL((csra_bwd_kernel<T, NT, CH>), dim3((owners + threads - 1) / threads, groups), dim3(threads), 0, st, ds, (const T*)x, sc, sh,
                     m, mean, rstd, e_scale, W, (T*)g, S1, S2, part, B, HW, C, ldx, ldg, n, act, det, GB);
}

// scratch = ds | the weight-gradient partials (| pcam: dl_eff (B n), which feeds the bias gradient in the place of dlogits)
template <typename T>
int head_bwd_t(Head head, const float* dlogits, const float* s, const float* stat, const float* lam_T, const void* x, const float* sc,
               const float* sh, const float* m, const float* mean, const float* rstd, const float* e_scale, const float* W, void* g, float* S1,
               float* S2, float* dW, float* db, float* scratch, long long scratch_len, int B, int HW, int C, int ldx, int ldg, int n, int act,
               int stat_rows, void* stream) {
  if (!dlogits || !s || !stat || (head == CSRA && !lam_T) || !x || !sc || !sh || !mean || !rstd || !e_scale || !W || !g || !S1 || !S2 || !dW ||
      !scratch || !known_act(act))
    return CX_EINVAL;
  if (n < 1 || !shape_ok<T>(B, HW, C, ldx) || !shape_ok<T>(B, HW, C, ldg)) return CX_ESHAPE;
  if (n > CX_CSRA_MAX_CLASSES) return CX_EUNSUPPORTED;
  if (scratch_len < scratch_floats(head, B, HW, C, n)) return CX_EUNSUPPORTED;   // refused, no other path
  if (!aligned16(x) || !aligned16(g) || !aligned16(scratch)) return CX_EALIGN;
  if (stat_rows > 0) { if (stat_rows < B) return CX_ESTATROWS; cx_tl_stat_rows = B; }
  const int NT = nt_of(n), GB = group_size(B), groups = (B + GB - 1) / GB, det = stat_rows > 0 ? 1 : 0;
  const size_t total = (size_t)B * HW * NT, nC = (size_t)n * C;
  float* ds = scratch;
  float* part = scratch + total;
  float* dleff = scratch + scratch_floats(CSRA, B, HW, C, n);
  hipStream_t st = as_stream(stream);
  if (head == CSRA)
    hipLaunchKernelGGL(csra_ds_kernel, dim3((total + 255) / 256), dim3(256), 0, st, dlogits, s, stat, lam_T, ds, total, n, HW, NT);
  else
    hipLaunchKernelGGL(pcam_ds_kernel, dim3(B), dim3(256), 0, st, dlogits, s, stat, ds, dleff, n, HW, NT);
  if (NT == 16)
    launch_bwd<T, 16, 4>(ds, x, sc, sh, m, mean, rstd, e_scale, W, g, S1, S2, part, B, HW, C, ldx, ldg, n, act, det, GB, groups, st);
  else if (NT == 32)
    launch_bwd<T, 32, 2>(ds, x, sc, sh, m, mean, rstd, e_scale, W, g, S1, S2, part, B, HW, C, ldx, ldg, n, act, det, GB, groups, st);
  else
    launch_bwd<T, 64, 1>(ds, x, sc, sh, m, mean, rstd, e_scale, W, g, S1, S2, part, B, HW, C, ldx, ldg, n, act, det, GB, groups, st);
  hipLaunchKernelGGL(csra_reduce_kernel, dim3((nC + n + 255) / 256), dim3(256), 0, st, part, head == CSRA ? dlogits : dleff, dW, db, groups, B,
                     n, nC);
  return launch_status();
}

}  // namespace

extern "C" {

int cx_csra_head_fwd(const void* x, const float* sc, const float* sh, const float* m, const float* W, const float* bias, const float* lam_T,
                     float* logits, float* s, float* stat, int B, int HW, int C, int ldx, int n, int act, void* stream) {
  return head_fwd_t<bf16>(CSRA, x, sc, sh, m, W, bias, lam_T, logits, s, stat, B, HW, C, ldx, n, act, stream);
}
int cx_csra_head_fwd_f32(const void* x, const float* sc, const float* sh, const float* m, const float* W, const float* bias, const float* lam_T,
                         float* logits, float* s, float* stat, int B, int HW, int C, int ldx, int n, int act, void* stream) {
  return head_fwd_t<float>(CSRA, x, sc, sh, m, W, bias, lam_T, logits, s, stat, B, HW, C, ldx, n, act, stream);
}
int cx_csra_head_bwd(const float* dlogits, const float* s, const float* stat, const float* lam_T, const void* x, const float* sc, const float* sh,
                     const float* m, const float* mean, const float* rstd, const float* e_scale, const float* W, void* g, float* S1, float* S2,
                     float* dW, float* db, float* scratch, long long scratch_len, int B, int HW, int C, int ldx, int ldg, int n, int act,
                     int stat_rows, void* stream) {
  return head_bwd_t<bf16>(CSRA, dlogits, s, stat, lam_T, x, sc, sh, m, mean, rstd, e_scale, W, g, S1, S2, dW, db, scratch, scratch_len, B, HW, C, ldx,
                          ldg, n, act, stat_rows, stream);
}
int cx_csra_head_bwd_f32(const float* dlogits, const float* s, const float* stat, const float* lam_T, const void* x, const float* sc,
                         const float* sh, const float* m, const float* mean, const float* rstd, const float* e_scale, const float* W, void* g,
                         float* S1, float* S2, float* dW, float* db, float* scratch, long long scratch_len, int B, int HW, int C, int ldx, int ldg,
                         int n, int act, int stat_rows, void* stream) {
  return head_bwd_t<float>(CSRA, dlogits, s, stat, lam_T, x, sc, sh, m, mean, rstd, e_scale, W, g, S1, S2, dW, db, scratch, scratch_len, B, HW, C, ldx,
                           ldg, n, act, stat_rows, stream);
}
long long cx_csra_bwd_scratch(int B, int HW, int C, int n) {
  return bwd_scratch(CSRA, B, HW, C, n);
}

int cx_pcam_head_fwd(const void* x, const float* sc, const float* sh, const float* m, const float* W, const float* bias, float* logits,
                     float* s, float* stat, int B, int HW, int C, int ldx, int n, int act, void* stream) {
  return head_fwd_t<bf16>(PCAM, x, sc, sh, m, W, bias, nullptr, logits, s, stat, B, HW, C, ldx, n, act, stream);
}
int cx_pcam_head_fwd_f32(const void* x, const float* sc, const float* sh, const float* m, const float* W, const float* bias, float* logits,
                         float* s, float* stat, int B, int HW, int C, int ldx, int n, int act, void* stream) {
  return head_fwd_t<float>(PCAM, x, sc, sh, m, W, bias, nullptr, logits, s, stat, B, HW, C, ldx, n, act, stream);
}
int cx_pcam_head_bwd(const float* dlogits, const float* s, const float* stat, const void* x, const float* sc, const float* sh, const float* m,
                     const float* mean, const float* rstd, const float* e_scale, const float* W, void* g, float* S1, float* S2, float* dW,
                     float* db, float* scratch, long long scratch_len, int B, int HW, int C, int ldx, int ldg, int n, int act, int stat_rows,
                     void* stream) {
  return head_bwd_t<bf16>(PCAM, dlogits, s, stat, nullptr, x, sc, sh, m, mean, rstd, e_scale, W, g, S1, S2, dW, db, scratch, scratch_len, B, HW, C, ldx, ldg, n,
                          act, stat_rows, stream);
}
int cx_pcam_head_bwd_f32(const float* dlogits, const float* s, const float* stat, const void* x, const float* sc, const float* sh,
                         const float* m, const float* mean, const float* rstd, const float* e_scale, const float* W, void* g, float* S1,
                         float* S2, float* dW, float* db, float* scratch, long long scratch_len, int B, int HW, int C, int ldx, int ldg, int n,
                         int act, int stat_rows, void* stream) {
  return head_bwd_t<float>(PCAM, dlogits, s, stat, nullptr, x, sc, sh, m, mean, rstd, e_scale, W, g, S1, S2, dW, db, scratch, scratch_len, B, HW, C, ldx, ldg,
                           n, act, stat_rows, stream);
}
long long cx_pcam_bwd_scratch(int B, int HW, int C, int n) {
  return bwd_scratch(PCAM, B, HW, C, n);
}

}  // extern "C"
