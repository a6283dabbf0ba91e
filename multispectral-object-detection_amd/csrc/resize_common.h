// cv2.resize(INTER_LINEAR) for 8-bit images as device functions, shared by cft_letterbox_u8 (pointwise.hip) and cft_pair_batch_u8
// (dataset.hip); below them the INTER_AREA tables (dataset.hip, mosaic.hip).  OpenCV's published 8-bit bilinear path (resize.cpp, INTER_RESIZE_COEF_BITS = 11): source coordinate
// f = (float)((d + 0.5) * scale - 0.5) with scale = 1 / (dst / src) in double, coefficients rounded to 1/2048, horizontal pass in int,
// vertical pass (((b0 * (r0 >> 4)) >> 16) + ((b1 * (r1 >> 4)) >> 16) + 2) >> 2.  The numpy restatement is oracle/letterbox_oracle.py.
#pragma once
#include <hip/hip_runtime.h>

__device__ __forceinline__ int cft_cv_round(float v) { return __float2int_rn(v); }   // cvRound: nearest, ties to even

__device__ __forceinline__ double cft_linear_scale(int dsize, int ssize) { return 1.0 / ((double)dsize / (double)ssize); }

struct CftLinearTap { int s0, s1, c0, c1; };      // the two source indices and their weights in 1/2048

// columns: an index outside the image is clamped and its fraction dropped
__device__ __forceinline__ CftLinearTap cft_linear_tap_x(int d, double scale, int ssize) {
  float f = (float)(((double)d + 0.5) * scale - 0.5);
  int s = (int)floorf(f);
  f -= (float)s;
  if (s < 0) { f = 0.f; s = 0; }
  if (s >= ssize - 1) { f = 0.f; s = ssize - 1; }
  CftLinearTap t;
  t.s0 = s;
  t.s1 = s + 1 > ssize - 1 ? ssize - 1 : s + 1;
  t.c0 = cft_cv_round((1.f - f) * 2048.f);
  t.c1 = cft_cv_round(f * 2048.f);
  return t;
}

// rows: cv2 clamps by index (sy0 = clip(sy), sy1 = clip(sy + 1)) and keeps the fractional weights
__device__ __forceinline__ CftLinearTap cft_linear_tap_y(int d, double scale, int ssize) {
  float f = (float)(((double)d + 0.5) * scale - 0.5);
  const int s = (int)floorf(f);
  f -= (float)s;
  CftLinearTap t;
  t.s0 = s < 0 ? 0 : (s > ssize - 1 ? ssize - 1 : s);
  t.s1 = s + 1 < 0 ? 0 : (s + 1 > ssize - 1 ? ssize - 1 : s + 1);
  t.c0 = cft_cv_round((1.f - f) * 2048.f);
  t.c1 = cft_cv_round(f * 2048.f);
  return t;
}

// p<row><col>: the four source values of one channel
__device__ __forceinline__ int cft_linear_blend(int p00, int p01, int p10, int p11, const CftLinearTap& tx, const CftLinearTap& ty) {
  const int h0 = p00 * tx.c0 + p01 * tx.c1;
  const int h1 = p10 * tx.c0 + p11 * tx.c1;
  const int v = (((ty.c0 * (h0 >> 4)) >> 16) + ((ty.c1 * (h1 >> 4)) >> 16) + 2) >> 2;
  return v < 0 ? 0 : (v > 255 ? 255 : v);
}

// ---- cv2.resize(INTER_AREA) for 8-bit images: shared by cft_pair_batch_u8 (dataset.hip) and cft_mosaic_area (mosaic.hip) ----
// One axis of computeResizeAreaTab for output index d: source cells [c0, c0 + n) with weight w_first for the first, w_last for the
// last and w_mid between (n == 1: w_first).  Cell boundaries d * ssize / dsize are exact in integers; the covered fractions and
// cv2's 1e-3 cut-off for a sliver of a cell are evaluated in double, the weights are float as cv2's DecimateAlpha.
struct AreaTab { int c0, n; float w_first, w_mid, w_last; };

__device__ __forceinline__ AreaTab area_tab(int d, int ssize, int dsize) {
  const double scale = (double)ssize / (double)dsize;
  const long lo = (long)d * ssize, hi = (long)(d + 1) * ssize;         // fsx1 = lo / dsize, fsx2 = hi / dsize
  int s1 = (int)((lo + dsize - 1) / dsize);                            // ceil(fsx1)
  int s2 = (int)(hi / dsize);                                          // floor(fsx2)
  s2 = s2 < ssize - 1 ? s2 : ssize - 1;
  s1 = s1 < s2 ? s1 : s2;
  const double cell = scale < (double)ssize - (double)lo / dsize ? scale : (double)ssize - (double)lo / dsize;
  const double head = (double)((long)s1 * dsize - lo) / dsize;         // s1 - fsx1
  const double tail = (double)(hi - (long)s2 * dsize) / dsize;         // fsx2 - s2
  const bool has_head = head > 1e-3, has_tail = tail > 1e-3;
  const float wh = (float)(head / cell), wm = (float)(1.0 / cell);
  const double t1 = tail < 1.0 ? tail : 1.0;
  const float wt = (float)((t1 < cell ? t1 : cell) / cell);
  AreaTab t;
  t.c0 = has_head ? s1 - 1 : s1;
  t.n = (has_head ? 1 : 0) + (s2 - s1) + (has_tail ? 1 : 0);
  t.w_mid = wm;
  t.w_first = has_head ? wh : (s2 > s1 ? wm : wt);
  t.w_last = has_tail ? wt : (s2 > s1 ? wm : wh);
  return t;
}
__device__ __forceinline__ float area_weight(const AreaTab& t, int i) { return i == 0 ? t.w_first : (i == t.n - 1 ? t.w_last : t.w_mid); }
