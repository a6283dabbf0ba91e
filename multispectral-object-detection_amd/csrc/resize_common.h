// cv2.resize(INTER_LINEAR) for 8-bit images as device functions, shared by cft_letterbox_u8 (pointwise.hip) and cft_pair_batch_u8
// (dataset.hip).  OpenCV's published 8-bit bilinear path (resize.cpp, INTER_RESIZE_COEF_BITS = 11): source coordinate
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
