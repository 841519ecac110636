// Contrast-limited adaptive histogram equalisation (CLAHE) of the decoded grey images on the GPU: the deterministic preprocessing
// step in front of cx_u8_affine / cx_u8_jitter / the first kernel of the network.  It runs behind the loader, so the decoded-image
// cache does not depend on its settings.  The definition is integer arithmetic throughout (include/chexpert_hip.h and
// chexpert_amd/augment.py state it; the tests hold the kernels to it bit for bit):
//   table of tile (b, gy, gx): histogram of the th x tw tile, clipped at L with the excess spread over the 256 bins (OpenCV's rule),
//                              cdf, lut[v] = (cdf[v] * 255 + area / 2) / area
//   pixel (i, j):              bilinear blend of the four tables whose tile centres surround the pixel centre, rounded half up
// Two entry points, one per stage, so that each can be held on its own.
// Measured at 256 x 320^2, grid 8 x 8, clip 2.0: tables 28 us on noise, 41 us on smooth content, 105 us on a
// constant image (the LDS adds of a wave serialise on one bin); apply 35 us whatever the content; cx_u8_jitter on the same bytes 18.5 us.
#include "common.h"

// ---- stage 1: one 256-byte table per tile ---------------------------------------------------------------------------------------
// One workgroup (4 waves) per tile.  Each wave counts into a histogram of its own in LDS (integer LDS adds: a sum of ones does not
// depend on the order the adds arrive in, so the result is the same bits on every run; nothing is added in device memory).  Tile rows
// are read as dwords where the tile's columns and the image allow it (tw % 4 == 0, x 4-byte aligned), else byte by byte.  After the
// barrier thread v owns bin v: sum of the four histograms, clip, redistribute (the residual loop in closed form: bin v gets one more
// iff v % step == 0 and v / step < r), a 256-wide inclusive scan (shuffles inside a wave, the three wave totals through LDS), and one
// byte store.
__device__ __forceinline__ int clahe_wave_scan(int v, const int lane) {      // inclusive prefix sum over the 64 lanes
#pragma unroll
  for (int d = 1; d < 64; d <<= 1) {
    const int u = __shfl_up(v, d, 64);
    if (lane >= d) v += u;
  }
  return v;
}

__global__ __launch_bounds__(256) void u8_clahe_lut_kernel(const uint8_t* __restrict__ x, uint8_t* __restrict__ lut, int H, int W, int GY,
                                                           int GX, int th, int tw, int clip, int wide) {
  __shared__ uint32_t hist[4][256];
  __shared__ int part[2][4];
  const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
  const int tiles = GY * GX;
  const int b = blockIdx.x / tiles, t = blockIdx.x - b * tiles;
  const int gy = t / GX, gx = t - gy * GX;
#pragma unroll
  for (int w = 0; w < 4; ++w) hist[w][tid] = 0u;
  __syncthreads();
  const uint8_t* src = x + ((size_t)b * H + (size_t)gy * th) * W + (size_t)gx * tw;      // rows gy*th .. +th, columns gx*tw .. +tw: inside
  uint32_t* h = hist[wave];
  if (wide) {
    const int dpr = tw >> 2, nd = th * dpr;
    for (int idx = tid; idx < nd; idx += 256) {
      const int r = idx / dpr, c = idx - r * dpr;
      const uint32_t p = *reinterpret_cast<const uint32_t*>(src + (size_t)r * W + c * 4);
      atomicAdd(&h[p & 255u], 1u);
      atomicAdd(&h[(p >> 8) & 255u], 1u);
      atomicAdd(&h[(p >> 16) & 255u], 1u);
      atomicAdd(&h[p >> 24], 1u);
    }
  } else {
    const int np = th * tw;
    for (int idx = tid; idx < np; idx += 256) {
      const int r = idx / tw, c = idx - r * tw;
      atomicAdd(&h[src[(size_t)r * W + c]], 1u);
    }
  }
  __syncthreads();
  int n = (int)(hist[0][tid] + hist[1][tid] + hist[2][tid] + hist[3][tid]);
  if (clip > 0) {                                                // uniform
    const int over = max(n - clip, 0);
    n = min(n, clip);
    const int s = clahe_wave_scan(over, lane);
    if (lane == 63) part[0][wave] = s;
    __syncthreads();
    const int excess = part[0][0] + part[0][1] + part[0][2] + part[0][3];
    const int q = excess >> 8, r = excess & 255;
    n += q;
    if (r > 0) {
      const int step = max(1, 256 / r);
      const int k = tid / step;
      if (k * step == tid && k < r) n += 1;
    }
  }
  int cdf = clahe_wave_scan(n, lane);
  if (lane == 63) part[1][wave] = cdf;
  __syncthreads();
  for (int w = 0; w < wave; ++w) cdf += part[1][w];              // (wave is uniform per wave: no divergence inside it)
  const int area = th * tw;                                      // cdf <= area <= 2^20: cdf * 255 + area / 2 < 2^31
  lut[(size_t)blockIdx.x * 256 + tid] = (uint8_t)((uint32_t)(cdf * 255 + (area >> 1)) / (uint32_t)area);
}

int cx_u8_clahe_lut(const uint8_t* x, uint8_t* lut, int B, int H, int W, int GY, int GX, int clip_count, void* stream) {
  if (!x || !lut || B <= 0 || H <= 0 || W <= 0) return CX_EINVAL;
  if (GY < 1 || GY > 16 || GX < 1 || GX > 16 || (W % 4) || W > 1024 || H > 1024 || (H % GY) || (W % GX)) return CX_ESHAPE;
  const int th = H / GY, tw = W / GX;
  if (clip_count < 0 || clip_count > th * tw) return CX_EINVAL;
  if (((uintptr_t)lut) & 3) return CX_EALIGN;                                // (the apply stage reads the tables as dwords)
  if ((long long)B * GY * GX >= (1ll << 31) / 8) return CX_ESHAPE;
  const int wide = (tw % 4 == 0) && ((((uintptr_t)x) & 3) == 0);              // W % 4 == 0: every row of every image is then aligned too
  hipLaunchKernelGGL(u8_clahe_lut_kernel, dim3((unsigned)(B * GY * GX)), dim3(256), 0, as_stream(stream), x, lut, H, W, GY, GX, th, tw,
                     clip_count, wide);
  return launch_status();
}

// ---- stage 2: the four-table bilinear look-up -----------------------------------------------------------------------------------
// Image rows fall into GY + 1 bands: band k holds the rows whose upper table row is gy0 = k - 1 (rows [((2k-1) th) / 2, ((2k+1) th) / 2)
// clamped to the image; the first and the last band are half a tile high and clamp both table rows to the same tile row).  One
// workgroup = up to CLAHE_ROWS rows of one band of one image, all columns.  It stages the band's two table rows in LDS, interleaved
// as 16-bit pairs (upper table | lower table << 8) so that a pixel costs two LDS reads instead of four: 2 * GX * 256 bytes, 4 KB at
// GX = 8.  One lane = 4 adjacent pixels = one dword store, as in u8_affine_kernel; a lane keeps its column for the whole band, so the
// column quantities (the two table columns and the weight of each of its four pixels) are computed once, and a row costs no division
// but the rounding one, which is a float estimate corrected by at most one (the quotient is <= 255, so the estimate is off by less
// than one).
constexpr int CLAHE_ROWS = 64;

__global__ __launch_bounds__(256) void u8_clahe_apply_kernel(const uint8_t* __restrict__ x, const uint8_t* __restrict__ lut,
                                                             uint8_t* __restrict__ y, int H, int W, int GY, int GX, int th, int tw, int chunks,
                                                             int xwide) {
  __shared__ uint16_t tab[16 * 256];
  const int tid = threadIdx.x;
  const int per_image = (GY + 1) * chunks;
  const int b = blockIdx.x / per_image, rest = blockIdx.x - b * per_image;
  const int k = rest / chunks, chunk = rest - k * chunks;
  const int band0 = max(((2 * k - 1) * th) / 2, 0), band1 = min(((2 * k + 1) * th) / 2, H);      // (2k - 1) th < 0 only for k = 0
  const int i0 = band0 + chunk * CLAHE_ROWS, i1 = min(i0 + CLAHE_ROWS, band1);
  if (i0 >= i1) return;                                          // uniform: an empty chunk (before the barrier, for every thread)
  const int gy0 = min(max(k - 1, 0), GY - 1), gy1 = min(k, GY - 1);
  const uint32_t* top = reinterpret_cast<const uint32_t*>(lut + ((size_t)b * GY + gy0) * GX * 256);
  const uint32_t* bot = reinterpret_cast<const uint32_t*>(lut + ((size_t)b * GY + gy1) * GX * 256);
  for (int d = tid; d < GX * 64; d += 256) {
    const uint32_t a = top[d], c = bot[d];
    uint2 o;
    o.x = (a & 255u) | ((c & 255u) << 8) | (((a >> 8) & 255u) << 16) | (((c >> 8) & 255u) << 24);
    o.y = ((a >> 16) & 255u) | (((c >> 16) & 255u) << 8) | ((a >> 24) << 16) | ((c >> 24) << 24);
    *reinterpret_cast<uint2*>(&tab[d * 4]) = o;
  }
  __syncthreads();
  const int lpr = W >> 2, rpp = 256 / lpr;                       // lanes per row (<= 256), rows per pass (>= 1)
  const int rsub = tid / lpr, col = tid - rsub * lpr;
  if (rsub >= rpp) return;                                       // (no barrier follows)
  const int tw2 = 2 * tw, th2 = 2 * th;
  // pixel j = 4 col + e: ax = 2j + 1 - tw, gx0 = floor(ax / 2tw), wx = ax - gx0 * 2tw
  int o0[4], o1[4], wx[4];
  {
    const int ax = 8 * col + 1 - tw;                             // >= 1 - tw: ax + 2tw > 0
    int g = (ax + tw2) / tw2 - 1, w = ax - g * tw2;
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      o0[e] = min(max(g, 0), GX - 1) * 256, o1[e] = min(max(g + 1, 0), GX - 1) * 256, wx[e] = w;
      w += 2;
      if (w >= tw2) w -= tw2, ++g;
    }
  }
  const uint32_t den = (uint32_t)(4 * th * tw), half = den >> 1;                 // num <= 255 * den < 2^31 at th, tw <= 1024
  const float rden = 1.f / (float)den;
  for (int i = i0 + rsub; i < i1; i += rpp) {
    const int wy = 2 * i + 1 - th - (k - 1) * th2;               // in [0, 2th)
    const size_t off = ((size_t)b * H + i) * W + 4 * col;
    uint32_t p;
    if (xwide)
      p = *reinterpret_cast<const uint32_t*>(x + off);
    else
      p = (uint32_t)x[off] | ((uint32_t)x[off + 1] << 8) | ((uint32_t)x[off + 2] << 16) | ((uint32_t)x[off + 3] << 24);
    uint32_t out = 0;
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      const uint32_t v = (p >> (8 * e)) & 255u;
      const uint32_t l = tab[o0[e] + v], r = tab[o1[e] + v];
      const uint32_t t0 = (uint32_t)(tw2 - wx[e]) * (l & 255u) + (uint32_t)wx[e] * (r & 255u);
      const uint32_t t1 = (uint32_t)(tw2 - wx[e]) * (l >> 8) + (uint32_t)wx[e] * (r >> 8);
      const uint32_t num = (uint32_t)(th2 - wy) * t0 + (uint32_t)wy * t1 + half;
      int q = (int)((float)num * rden);
      const int rem = (int)num - q * (int)den;
      q += rem >= (int)den ? 1 : (rem < 0 ? -1 : 0);
      out |= (uint32_t)q << (8 * e);
    }
    *reinterpret_cast<uint32_t*>(y + off) = out;
  }
}

int cx_u8_clahe_apply(const uint8_t* x, const uint8_t* lut, uint8_t* y, int B, int H, int W, int GY, int GX, void* stream) {
  if (!x || !lut || !y || x == y || B <= 0 || H <= 0 || W <= 0) return CX_EINVAL;
  if (GY < 1 || GY > 16 || GX < 1 || GX > 16 || (W % 4) || W > 1024 || H > 1024 || (H % GY) || (W % GX)) return CX_ESHAPE;
  if ((((uintptr_t)y) & 3) || (((uintptr_t)lut) & 3)) return CX_EALIGN;       // one dword store per lane, dword reads of the tables
  const int th = H / GY, tw = W / GX;
  const int chunks = (th + CLAHE_ROWS - 1) / CLAHE_ROWS;
  if ((long long)B * (GY + 1) * chunks >= (1ll << 31) / 8) return CX_ESHAPE;
  const int xwide = (((uintptr_t)x) & 3) == 0;
  hipLaunchKernelGGL(u8_clahe_apply_kernel, dim3((unsigned)(B * (GY + 1) * chunks)), dim3(256), 0, as_stream(stream), x, lut, y, H, W, GY, GX,
                     th, tw, chunks, xwide);
  return launch_status();
}
