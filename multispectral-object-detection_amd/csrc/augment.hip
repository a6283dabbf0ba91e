// Batch assembly for the augmented RGB + IR training loader: ONE launch writes the uint8 [B, 6, H, W] batch (cft_augment_batch_u8,
// include/cft_hip.h, where the raster is defined) from a device-resident table with one row per output image and a [B, 2, 3, 256]
// block of HSV look-up tables.  Per output pixel: undo the flips, map through the inverse affine of cv2.warpAffine (1/32 pixel, four
// taps), fetch each tap from the mosaic canvas - which is never materialised: a tap inside one of the at most four tiles is computed
// on the fly from the original with the INTER_LINEAR arithmetic of resize_common.h - blend with integer weights, apply the HSV
// round trip through the image's look-up tables, store RGB planes 0-2 and IR planes 3-5.
//
// Launch shape: the grid is (groups of 1024 output pixels, B); one thread produces 4 consecutive pixels of one row for both streams
// and stores one dword per plane.  The workgroup keeps its image's 1.5 KB of look-up tables in LDS.  Sources are read straight from
// global memory: under rotation and scale the footprint of a row of output pixels is irregular, and the originals of one item are a
// few MB, so L2 serves the re-reads.  No atomics, no inline assembly; every output byte is written once by one thread.
//
// The tile lookup and the resize taps of a canvas pixel are the same for both streams and all channels and are computed once.
// Everything that decides a byte is integer arithmetic or a singly rounded float operation: contraction is off for the whole file.
#include "cft_common.h"
#include "resize_common.h"
#include <cmath>

#pragma clang fp contract(off)

#define AUG_THREADS 256
#define AUG_BORDER 114
#define AUG_COEF_LIMIT 1048576.0       // |inverse-affine coefficient| < 2^20: with sides <= 2^14 a coordinate in 1/1024 pixel is below 2^46

// Where one canvas pixel comes from: nothing (border) or one tile, with the resize weights of its four source pixels.
struct AugTap {
  int tile;                            // -1: border
  CftLinearTap tx, ty;
  bool copy;
};

__device__ __forceinline__ int aug_clampi(int v, int lo, int hi) { return v < lo ? lo : (v > hi ? hi : v); }

__device__ __forceinline__ void aug_locate(const cft_aug_desc_t& d, long cy, long cx, AugTap& t, int& y0, int& y1, int& x0, int& x1) {
  t.tile = -1;
  if (cy < 0 || cx < 0 || cy >= d.canvas_h || cx >= d.canvas_w) return;
  for (int k = 0; k < 4; ++k) {
    if (k >= d.ntiles) break;
    const cft_aug_tile_t& q = d.tile[k];
    if (cy < q.y1 || cy >= q.y2 || cx < q.x1 || cx >= q.x2) continue;
    const int ry = aug_clampi((int)cy - q.padh, 0, q.h - 1), rx = aug_clampi((int)cx - q.padw, 0, q.w - 1);
    t.tile = k;
    t.copy = q.h == q.h0 && q.w == q.w0;
    if (t.copy) {
      y0 = y1 = ry; x0 = x1 = rx;
    } else {
      t.ty = cft_linear_tap_y(ry, cft_linear_scale(q.h, q.h0), q.h0);
      t.tx = cft_linear_tap_x(rx, cft_linear_scale(q.w, q.w0), q.w0);
      y0 = aug_clampi(t.ty.s0, 0, q.h0 - 1); y1 = aug_clampi(t.ty.s1, 0, q.h0 - 1);
      x0 = aug_clampi(t.tx.s0, 0, q.w0 - 1); x1 = aug_clampi(t.tx.s1, 0, q.w0 - 1);
    }
    return;
  }
}

// The three channels of one canvas pixel of one stream.
__device__ __forceinline__ void aug_fetch(const cft_aug_desc_t& d, const AugTap& t, int y0, int y1, int x0, int x1, int s, int v[3]) {
  if (t.tile < 0) { v[0] = v[1] = v[2] = AUG_BORDER; return; }
  const cft_aug_tile_t& q = d.tile[t.tile];
  const unsigned char* src = s ? q.src_ir : q.src_rgb;
  const long stride = s ? q.stride_ir : q.stride_rgb;
  const unsigned char* r0 = src + (long)y0 * stride;
  if (t.copy) {
    const unsigned char* p = r0 + 3L * x0;
    v[0] = p[0]; v[1] = p[1]; v[2] = p[2];
    return;
  }
  const unsigned char* r1 = src + (long)y1 * stride;
#pragma unroll
  for (int c = 0; c < 3; ++c)
    v[c] = cft_linear_blend(r0[3L * x0 + c], r0[3L * x1 + c], r1[3L * x0 + c], r1[3L * x1 + c], t.tx, t.ty);
}

// cv2's two division tables of the 8-bit BGR -> HSV path, entry i: rint((255 << 12) / i) and rint((180 << 12) / (6 i)), entry 0 = 0.
__device__ __forceinline__ int aug_sdiv(int i) { return i ? (int)rint((double)(255 << 12) / (double)i) : 0; }
__device__ __forceinline__ int aug_hdiv(int i) { return i ? (int)rint((double)(180 << 12) / (6.0 * (double)i)) : 0; }

__device__ __forceinline__ int aug_u8(float t) {
  const int q = cft_cv_round(255.f * t);
  return q < 0 ? 0 : (q > 255 ? 255 : q);
}

// (r, g, b) -> 8-bit HSV -> the three look-up tables -> (r, g, b); lut points at this stream's [3][256] bytes in LDS, sdiv / hdiv at
// the workgroup's copies of the two division tables.
__device__ __forceinline__ void aug_hsv(const unsigned char* lut, const int* sdiv, const int* hdiv, int& r, int& g, int& b) {
  const int v = max(r, max(g, b)), mn = min(r, min(g, b)), diff = v - mn;
  const int s = (diff * sdiv[v] + 2048) >> 12;
  const int hh = v == r ? g - b : (v == g ? b - r + 2 * diff : r - g + 4 * diff);
  int h = (hh * hdiv[diff] + 2048) >> 12;
  if (h < 0) h += 180;
  const int h2 = lut[h & 255], s2 = lut[256 + aug_clampi(s, 0, 255)], v2 = lut[512 + v];
  const float sf = __fdiv_rn((float)s2, 255.f), vf = __fdiv_rn((float)v2, 255.f), hf = __fdiv_rn((float)h2, 30.f);
  const float kf = floorf(hf);
  const float f = hf - kf;
  const int k = (int)kf % 6;
  const float t0 = vf, t1 = vf * (1.f - sf), t2 = vf * (1.f - sf * f), t3 = vf * (1.f - sf * (1.f - f));
  float fb, fg, fr;
  switch (k) {
    case 0: fb = t1; fg = t3; fr = t0; break;
    case 1: fb = t1; fg = t0; fr = t2; break;
    case 2: fb = t3; fg = t0; fr = t1; break;
    case 3: fb = t0; fg = t2; fr = t1; break;
    case 4: fb = t0; fg = t1; fr = t3; break;
    default: fb = t2; fg = t1; fr = t0; break;
  }
  r = aug_u8(fr); g = aug_u8(fg); b = aug_u8(fb);
}

__global__ void __launch_bounds__(AUG_THREADS) augment_batch_u8_kernel(const cft_aug_desc_t* __restrict__ desc, const unsigned char* __restrict__ luts,
                                                                       unsigned char* __restrict__ dst, int H, int W) {
  __shared__ unsigned int lut_w[2 * 3 * 256 / 4];
  __shared__ int sdiv[256], hdiv[256];
  __shared__ cft_aug_desc_t d;                                  // uniform over the workgroup
  const int b = blockIdx.y;
  {
    const unsigned int* gl = reinterpret_cast<const unsigned int*>(luts + (long)b * 1536);    // 1536 b: dword aligned when luts is
    for (int i = threadIdx.x; i < 384; i += AUG_THREADS) lut_w[i] = gl[i];
    for (int i = threadIdx.x; i < 256; i += AUG_THREADS) { sdiv[i] = aug_sdiv(i); hdiv[i] = aug_hdiv(i); }
    const unsigned int* gd = reinterpret_cast<const unsigned int*>(desc + b);
    unsigned int* ld = reinterpret_cast<unsigned int*>(&d);
    for (int i = threadIdx.x; i < (int)(sizeof(cft_aug_desc_t) / 4); i += AUG_THREADS) ld[i] = gd[i];
  }
  __syncthreads();
  const unsigned char* lut = reinterpret_cast<const unsigned char*>(lut_w);

  const int gpr = W >> 2;                                       // 4-pixel groups per row
  const long g = (long)blockIdx.x * AUG_THREADS + threadIdx.x;
  if (g >= (long)gpr * H) return;
  const int oy = (int)(g / gpr), ox = (int)(g % gpr) * 4;
  const int fy_ = (d.flip & CFT_AUG_FLIPUD) ? H - 1 - oy : oy;

  long yX = 0, yY = 0;
  if (d.warp) {
    yX = __double2ll_rn((d.inv[1] * (double)fy_ + d.inv[2]) * 1024.0);
    yY = __double2ll_rn((d.inv[4] * (double)fy_ + d.inv[5]) * 1024.0);
  }

  unsigned int out[6] = {0u, 0u, 0u, 0u, 0u, 0u};
#pragma unroll 1
  for (int j = 0; j < 4; ++j) {
    const int fx_ = (d.flip & CFT_AUG_FLIPLR) ? W - 1 - (ox + j) : ox + j;
    int px[6];
    if (!d.warp) {
      AugTap t; int y0 = 0, y1 = 0, x0 = 0, x1 = 0;
      aug_locate(d, fy_, fx_, t, y0, y1, x0, x1);
      aug_fetch(d, t, y0, y1, x0, x1, 0, px);
      aug_fetch(d, t, y0, y1, x0, x1, 1, px + 3);
    } else {
      const long X = (__double2ll_rn(d.inv[0] * (double)fx_ * 1024.0) + yX + 16) >> 5;
      const long Y = (__double2ll_rn(d.inv[3] * (double)fx_ * 1024.0) + yY + 16) >> 5;
      const long sx = X >> 5, sy = Y >> 5;
      const int fx = (int)(X & 31), fy = (int)(Y & 31);
      const int w4[4] = {(32 - fx) * (32 - fy), fx * (32 - fy), (32 - fx) * fy, fx * fy};
      int acc[6] = {0, 0, 0, 0, 0, 0};
#pragma unroll 1
      for (int k = 0; k < 4; ++k) {
        if (w4[k] == 0) continue;                               // a tap of weight 0 decides nothing
        AugTap t; int y0 = 0, y1 = 0, x0 = 0, x1 = 0;
        aug_locate(d, sy + (k >> 1), sx + (k & 1), t, y0, y1, x0, x1);
        int v[6];
        aug_fetch(d, t, y0, y1, x0, x1, 0, v);
        aug_fetch(d, t, y0, y1, x0, x1, 1, v + 3);
#pragma unroll
        for (int c = 0; c < 6; ++c) acc[c] += w4[k] * v[c];
      }
#pragma unroll
      for (int c = 0; c < 6; ++c) px[c] = (acc[c] + 512) >> 10;
    }
    aug_hsv(lut, sdiv, hdiv, px[0], px[1], px[2]);
    aug_hsv(lut + 768, sdiv, hdiv, px[3], px[4], px[5]);
#pragma unroll
    for (int c = 0; c < 6; ++c) out[c] |= (unsigned int)px[c] << (8 * j);
  }
  unsigned char* base = dst + ((long)b * 6 * H + oy) * (long)W + ox;
#pragma unroll
  for (int c = 0; c < 6; ++c)
    *reinterpret_cast<unsigned int*>(base + (long)c * H * W) = out[c];
}

extern "C" int cft_augment_batch_u8(const void* desc_dev, const void* desc_host, const unsigned char* luts, int B, unsigned char* dst,
                                    int dst_h, int dst_w, void* stream) {
  static_assert(sizeof(cft_aug_desc_t) == CFT_AUG_DESC_BYTES && sizeof(cft_aug_tile_t) == CFT_AUG_TILE_BYTES, "cft_aug_desc_t layout");
  CFT_REQUIRE(desc_dev && desc_host && luts && dst, "cft_augment_batch_u8: null pointer");
  CFT_REQUIRE(((uintptr_t)desc_dev & 7) == 0 && ((uintptr_t)desc_host & 7) == 0 && ((uintptr_t)luts & 3) == 0, "cft_augment_batch_u8: misaligned table or look-up tables");
  CFT_REQUIRE(B > 0 && B <= 65535, "cft_augment_batch_u8: batch size out of range (1..65535)");
  CFT_REQUIRE(dst_h > 0 && dst_w > 0 && dst_h <= CFT_AUG_MAX_SIDE && dst_w <= CFT_AUG_MAX_SIDE, "cft_augment_batch_u8: output size out of range");
  CFT_REQUIRE(dst_w % 4 == 0 && ((uintptr_t)dst & 3) == 0, "cft_augment_batch_u8: dst and dst_w must be multiples of 4");
  const cft_aug_desc_t* rows = static_cast<const cft_aug_desc_t*>(desc_host);
  for (int b = 0; b < B; ++b) {
    const cft_aug_desc_t& d = rows[b];
    CFT_REQUIRE(d.ntiles == 1 || d.ntiles == 4, "cft_augment_batch_u8: a row has 1 or 4 tiles");
    CFT_REQUIRE(d.warp == 0 || d.warp == 1, "cft_augment_batch_u8: bad warp flag");
    CFT_REQUIRE((d.flip & ~(CFT_AUG_FLIPLR | CFT_AUG_FLIPUD)) == 0, "cft_augment_batch_u8: bad flip bits");
    CFT_REQUIRE(d.canvas_h > 0 && d.canvas_w > 0 && d.canvas_h <= CFT_AUG_MAX_SIDE && d.canvas_w <= CFT_AUG_MAX_SIDE, "cft_augment_batch_u8: canvas size out of range");
    if (d.warp) {
      for (int i = 0; i < 6; ++i)
        CFT_REQUIRE(std::isfinite(d.inv[i]) && std::fabs(d.inv[i]) < AUG_COEF_LIMIT, "cft_augment_batch_u8: inverse-affine coefficient not finite or too large");
    } else {
      CFT_REQUIRE(d.canvas_h == dst_h && d.canvas_w == dst_w, "cft_augment_batch_u8: without a warp the canvas is the output");
    }
    for (int k = 0; k < d.ntiles; ++k) {
      const cft_aug_tile_t& q = d.tile[k];
      CFT_REQUIRE(q.src_rgb && q.src_ir, "cft_augment_batch_u8: null source pointer in the table");
      CFT_REQUIRE(q.h0 > 0 && q.w0 > 0 && q.h > 0 && q.w > 0 && q.h0 <= CFT_AUG_MAX_SIDE && q.w0 <= CFT_AUG_MAX_SIDE && q.h <= CFT_AUG_MAX_SIDE && q.w <= CFT_AUG_MAX_SIDE,
                  "cft_augment_batch_u8: image size out of range (a resize the linear taps cannot index)");
      CFT_REQUIRE(q.stride_rgb >= 3L * q.w0 && q.stride_ir >= 3L * q.w0, "cft_augment_batch_u8: bad source row stride");
      CFT_REQUIRE(q.x1 >= 0 && q.y1 >= 0 && q.x1 <= q.x2 && q.y1 <= q.y2 && q.x2 <= d.canvas_w && q.y2 <= d.canvas_h, "cft_augment_batch_u8: a tile rectangle lies outside the canvas");
      if (q.x1 < q.x2 && q.y1 < q.y2)
        CFT_REQUIRE((long)q.x1 - q.padw >= 0 && (long)q.y1 - q.padh >= 0 && (long)q.x2 - q.padw <= q.w && (long)q.y2 - q.padh <= q.h,
                    "cft_augment_batch_u8: a tile rectangle minus its pad lies outside the resized image");
      for (int j = 0; j < k; ++j) {
        const cft_aug_tile_t& p = d.tile[j];
        const bool apart = q.x1 >= q.x2 || q.y1 >= q.y2 || p.x1 >= p.x2 || p.y1 >= p.y2 || q.x2 <= p.x1 || p.x2 <= q.x1 || q.y2 <= p.y1 || p.y2 <= q.y1;
        CFT_REQUIRE(apart, "cft_augment_batch_u8: two tile rectangles overlap");
      }
    }
  }
  const long groups = (long)(dst_w / 4) * dst_h;
  hipLaunchKernelGGL(augment_batch_u8_kernel, dim3((unsigned)((groups + AUG_THREADS - 1) / AUG_THREADS), B), dim3(AUG_THREADS), 0, as_stream(stream),
                     static_cast<const cft_aug_desc_t*>(desc_dev), luts, dst, dst_h, dst_w);
  return cft_check_launch("augment_batch_u8_kernel");
}
