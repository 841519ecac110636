// What bootstrap.hip, calib.hip and delong.hip share: the per-class entry lists as a kernel argument, the host loop that launches a
// kernel once per group of classes, the host check of the list arguments, and the wave-wide scans and sums of their kernels.
#pragma once
#include "common.h"

// ---- per-class entry lists ---------------------------------------------------------------------------------------------------------
// A statistic reads, for class c, len[c] entries of an order array from offs[c].  The offsets and lengths travel as kernel arguments,
// CX_LIST_CLASSES classes per launch.
constexpr int CX_LIST_CLASSES = 32;

struct ClassLists {
  long long offs[CX_LIST_CLASSES];
  int len[CX_LIST_CLASSES];
};

// The list arguments of an entry point: U units in 1 .. CX_BOOT_MAX_UNITS under a row pitch ld, no negative offset or length.
static inline int check_class_lists(int U, int ld, const int64_t* offs, const int32_t* len, int C) {
  if (U < 1 || U > CX_BOOT_MAX_UNITS || ld < U) return CX_ESHAPE;
  for (int c = 0; c < C; ++c)
    if (len[c] < 0 || offs[c] < 0) return CX_EINVAL;
  return 0;
}

// For every group of CX_LIST_CLASSES classes: fills `lists` (unused slots: offset 0, length 0) and calls launch(c0, cn) with the
// group's first class and its size, then reads the launch status.  Returns the first non-zero status.
template <class Launch>
static inline int for_class_groups(const int64_t* offs, const int32_t* len, int C, ClassLists& lists, Launch launch) {
  for (int c0 = 0; c0 < C; c0 += CX_LIST_CLASSES) {
    const int cn = min(CX_LIST_CLASSES, C - c0);
    for (int c = 0; c < CX_LIST_CLASSES; ++c) lists.offs[c] = c < cn ? (long long)offs[c0 + c] : 0ll, lists.len[c] = c < cn ? len[c0 + c] : 0;
    launch(c0, cn);
    const int rc = launch_status();
    if (rc) return rc;
  }
  return 0;
}

// ---- wave helpers (64 lanes) -------------------------------------------------------------------------------------------------------
// Scans in uint32 by DPP: four shifts inside the rows of 16 lanes, then lane 15 of a row to the next row and lane 31 to the upper
// half.  A lane without a source takes 0, the identity of both operations.
struct WaveAdd {
  __device__ __forceinline__ uint32_t operator()(uint32_t a, uint32_t b) const { return a + b; }
};
struct WaveMax {
  __device__ __forceinline__ uint32_t operator()(uint32_t a, uint32_t b) const { return max(a, b); }
};

template <class Op>
__device__ __forceinline__ uint32_t wave_scan_dpp(uint32_t v) {
  const Op op;
#define CX_SCAN_DPP(ctrl, rows) v = op(v, (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, ctrl, rows, 0xf, false))
  CX_SCAN_DPP(0x111, 0xf);    // row_shr:1
  CX_SCAN_DPP(0x112, 0xf);    // row_shr:2
  CX_SCAN_DPP(0x114, 0xf);    // row_shr:4
  CX_SCAN_DPP(0x118, 0xf);    // row_shr:8
  CX_SCAN_DPP(0x142, 0xa);    // row_bcast:15 into rows 1 and 3
  CX_SCAN_DPP(0x143, 0xc);    // row_bcast:31 into rows 2 and 3
#undef CX_SCAN_DPP
  return v;
}

__device__ __forceinline__ uint32_t wave_scan_add(uint32_t v) { return wave_scan_dpp<WaveAdd>(v); }      // inclusive

__device__ __forceinline__ uint32_t wave_xscan_max(uint32_t v) {                                         // exclusive, identity 0
  v = (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x138, 0xf, 0xf, false);      // wave_shr:1 (lane 0 takes the identity)
  return wave_scan_dpp<WaveMax>(v);
}

// The uint64 sum over the wave by an xor butterfly, the value moved as two 32-bit halves: every lane ends with the sum.
__device__ __forceinline__ uint64_t wave_sum_u64(uint64_t v) {
#pragma unroll
  for (int d = 32; d >= 1; d >>= 1)
    v += ((uint64_t)(uint32_t)__shfl_xor((int)(v >> 32), d) << 32) | (uint64_t)(uint32_t)__shfl_xor((int)(uint32_t)v, d);
  return v;
}
