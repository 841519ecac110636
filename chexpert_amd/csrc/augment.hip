// Geometric augmentation of the decoded grey images on the GPU: the random affine warp (rotation, scale, translation, shear) that
// sits between the loader's uint8 batch and cx_u8_jitter / the first kernel of the network.  The loader's decoded cache stays valid
// because the random step runs behind it.
#include "common.h"

// y[b][i][j] = bilinear sample of x[b] at the source position the INVERSE map mat[b] (row-major 2x3, pixel units about the image
// centre) gives for output pixel (i, j); taps outside the image read `fill`.  fp32 throughout:
//   xo = j + 0.5 - W/2, yo = i + 0.5 - H/2
//   u  = m0*xo + m1*yo + m2 + W/2 - 0.5,  v = m3*xo + m4*yo + m5 + H/2 - 0.5
//   u0 = floor(u), v0 = floor(v), fu = u - u0, fv = v - v0
//   top = p(v0,u0)*(1-fu) + p(v0,u0+1)*fu, bot likewise on row v0+1;  y = uint8(floor(top*(1-fv) + bot*fv + 0.5))
// One workgroup = a 64 x 16 output tile of one image (its source footprint under a rotation of a few degrees is a compact patch of
// the 100 KB image, which stays in L2); one lane = 4 adjacent output pixels, stored as one dword.  The six matrix entries are
// uniform per workgroup (scalar loads); the source addresses are per lane.  A tap's address is clamped into the image and its
// value replaced by `fill` where the tap lies outside, so no load leaves the image whatever the matrix holds; the 16 byte loads
// of a lane are issued together, ahead of the arithmetic that consumes them.
// Measured at 256 x 320^2 (52 MB): 49 us for the identity, 90 us at the default ranges (+-10 degrees), against 19 us for
// cx_u8_jitter on the same bytes -- the same instructions, so the difference is the access pattern: under a rotation the 64 lanes of
// one load instruction touch several times as many cache lines.  Staging the tile's source footprint in LDS first (dword loads, taps
// as LDS byte reads) was built and measured too: 59 us / 98 us, no gain where it matters.
constexpr int AFF_TW = 64, AFF_TH = 16;      // output tile: 16 lanes x 4 pixels wide, 16 rows

__global__ __launch_bounds__(256) void u8_affine_kernel(const uint8_t* __restrict__ x, uint8_t* __restrict__ y, int H, int W,
                                                        const float* __restrict__ mat, float fill, int tiles_x, int tiles) {
  const int b = blockIdx.x / tiles, t = blockIdx.x - b * tiles;
  const int ty = t / tiles_x, tx = t - ty * tiles_x;
  const int j0 = tx * AFF_TW + (threadIdx.x & 15) * 4, i = ty * AFF_TH + (threadIdx.x >> 4);
  if (i >= H || j0 >= W) return;               // W % 4 == 0: a lane's four pixels are inside together
  const float* m = mat + b * 6;
  const float m0 = m[0], m1 = m[1], m2 = m[2], m3 = m[3], m4 = m[4], m5 = m[5];
  const float cx = 0.5f * (float)W, cy = 0.5f * (float)H;
  const uint8_t* src = x + (size_t)b * H * W;
  const float yo = (float)i + 0.5f - cy;
  const float ru = fmaf(m1, yo, m2), rv = fmaf(m4, yo, m5);
  float fu[4], fv[4];
  int u0[4], v0[4];
  uint32_t q[4][4];
#pragma unroll
  for (int e = 0; e < 4; ++e) {
    const float xo = (float)(j0 + e) + 0.5f - cx;
    float u = fmaf(m0, xo, ru) + (cx - 0.5f), v = fmaf(m3, xo, rv) + (cy - 0.5f);
    // beyond one pixel outside the image every tap reads `fill`: clamping there keeps floor() inside the int range (NaN -> -2)
    u = fminf(fmaxf(u, -2.f), (float)W + 1.f);
    v = fminf(fmaxf(v, -2.f), (float)H + 1.f);
    const float uf = floorf(u), vf = floorf(v);
    fu[e] = u - uf, fv[e] = v - vf, u0[e] = (int)uf, v0[e] = (int)vf;
    const int ul = min(max(u0[e], 0), W - 1), ur = min(max(u0[e] + 1, 0), W - 1);
    const uint8_t* r0 = src + min(max(v0[e], 0), H - 1) * W;
    const uint8_t* r1 = src + min(max(v0[e] + 1, 0), H - 1) * W;
    q[e][0] = r0[ul], q[e][1] = r0[ur], q[e][2] = r1[ul], q[e][3] = r1[ur];
  }
  uint32_t out = 0;
#pragma unroll
  for (int e = 0; e < 4; ++e) {
    const bool cl = u0[e] >= 0 && u0[e] < W, cr = u0[e] + 1 >= 0 && u0[e] + 1 < W, rt = v0[e] >= 0 && v0[e] < H, rb = v0[e] + 1 >= 0 && v0[e] + 1 < H;
    const float p00 = (rt && cl) ? (float)q[e][0] : fill, p01 = (rt && cr) ? (float)q[e][1] : fill;
    const float p10 = (rb && cl) ? (float)q[e][2] : fill, p11 = (rb && cr) ? (float)q[e][3] : fill;
    const float top = p00 * (1.f - fu[e]) + p01 * fu[e], bot = p10 * (1.f - fu[e]) + p11 * fu[e];
    const float val = floorf(top * (1.f - fv[e]) + bot * fv[e] + 0.5f);
    out |= (uint32_t)fminf(fmaxf(val, 0.f), 255.f) << (8 * e);
  }
  *reinterpret_cast<uint32_t*>(y + ((size_t)b * H + i) * W + j0) = out;
}

int cx_u8_affine(const uint8_t* x, uint8_t* y, int B, int H, int W, const float* mat, int fill, void* stream) {
  if (!x || !y || !mat || x == y || B <= 0 || H <= 0 || W <= 0 || fill < 0 || fill > 255) return CX_EINVAL;
  if ((W % 4) || W > 1024 || H > 1024) return CX_ESHAPE;
  if ((((uintptr_t)y) & 3) || (((uintptr_t)mat) & 3)) return CX_EALIGN;      // one dword store per lane
  const int tiles_x = (W + AFF_TW - 1) / AFF_TW, tiles = tiles_x * ((H + AFF_TH - 1) / AFF_TH);
  if ((long long)B * tiles >= (1ll << 31) / 8) return CX_ESHAPE;              // (image offsets are 64-bit: B * H * W itself may exceed 2^31)
  hipLaunchKernelGGL(u8_affine_kernel, dim3((unsigned)(B * tiles)), dim3(256), 0, as_stream(stream), x, y, H, W, mat, (float)fill,
                     tiles_x, tiles);
  return launch_status();
}
