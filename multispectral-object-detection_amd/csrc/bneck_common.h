// Launch parameters of the fused Bottleneck kernels (bottleneck.hip).
#pragma once
#include "cft_common.h"

struct Bneck128Params {
  const unsigned char* x;
  const unsigned char* w1;   // [128][kpad1]
  const unsigned char* w2;   // [128][kpad2], k = (kh*3 + kw)*128 + ci
  const unsigned char* w2s;  // the same weights as 36 stage images of 8 KiB (cft_bottleneck_pack_w2), or null
  const float* b1;
  const float* b2;
  unsigned char* y;
  int ldx, xoff, ldy, yoff, kpad1, kpad2;
  int H, W, tiles_x, tiles_y, ntiles, shortcut;
  uint32_t m_tiles, m_tiles_x;   // bneck_magic(tiles_x * tiles_y), bneck_magic(tiles_x): the kernels divide tile ids without a divider
};

// floor(2^32 / d) for the mul-hi division below (d >= 1; d = 1 saturates)
static inline uint32_t bneck_magic(int d) { return d <= 1 ? 0xffffffffu : (uint32_t)((1ull << 32) / (unsigned)d); }
// n / d and the remainder for 0 <= n < 2^31 with m = bneck_magic(d): the mul-hi estimate is the quotient or one less
// (n (2^32 / d - m) < 2^31), so one correction step makes it exact.  Wave-uniform operands stay on the scalar unit.
__device__ __forceinline__ int bneck_divmod(int n, int d, uint32_t m, int& rem) {
  int q = (int)__umulhi((uint32_t)n, m);
  int r = n - q * d;
  if (r >= d) { ++q; r -= d; }
  rem = r;
  return q;
}
