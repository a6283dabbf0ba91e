// What the JPEG decoder (jpeg.hip) and the JPEG encoder (jpeg_encode.hip) share, each thing once: the geometry of a file, the layout
// of its coefficients, the guard of a table row's geometry, and the shape of the DCT kernels' workgroups.  include/cft_hip.h defines
// the subset and the arithmetic.  The host functions here keep the host half's contract: plain C++, nothing allocated, no global written.
#pragma once
#include "cft_common.h"
#include <string.h>

// ------------------------------------------------------------------------------------------------ host
// natural-order index of the k-th coefficient in zigzag order
static const unsigned char JPEG_ZIGZAG[64] = {0, 1, 8, 16, 9, 2, 3, 10, 17, 24, 32, 25, 18, 11, 4, 5, 12, 19, 26, 33, 40, 48, 41, 34, 27, 20, 13, 6, 7, 14, 21, 28,
                                              35, 42, 49, 56, 57, 50, 43, 36, 29, 22, 15, 23, 30, 37, 44, 51, 58, 59, 52, 45, 38, 31, 39, 46, 53, 60, 61, 54, 47, 55, 62, 63};

// The sampling subset: one component 1x1; three with chroma 1x1 and luma (hmax x vmax) 1x1, 2x1 or 2x2.
static inline bool jpeg_sampling_ok(int ncomp, int hmax, int vmax) {
  if (ncomp == 1) return hmax == 1 && vmax == 1;
  return ncomp == 3 && ((hmax == 1 && vmax == 1) || (hmax == 2 && vmax == 1) || (hmax == 2 && vmax == 2));
}

// The geometry of a file of the subset, every field of I (restart_interval 0): the MCU-padded block grid bw x bh and the downsampled
// size cw x ch per component, the coefficient and plane counts.  False, with I untouched, for sides or sampling outside the subset.
static inline bool jpeg_geometry(int width, int height, int ncomp, int hmax, int vmax, cft_jpeg_info_t& I) {
  if (width < 1 || height < 1 || width > CFT_JPEG_MAX_SIDE || height > CFT_JPEG_MAX_SIDE || !jpeg_sampling_ok(ncomp, hmax, vmax)) return false;
  memset(&I, 0, sizeof I);
  I.width = width; I.height = height; I.ncomp = ncomp; I.hmax = hmax; I.vmax = vmax;
  I.mcus_x = (width + 8 * hmax - 1) / (8 * hmax);
  I.mcus_y = (height + 8 * vmax - 1) / (8 * vmax);
  long blocks = 0;
  for (int c = 0; c < ncomp; ++c) {
    I.hs[c] = c ? 1 : hmax; I.vs[c] = c ? 1 : vmax;
    I.bw[c] = I.mcus_x * I.hs[c]; I.bh[c] = I.mcus_y * I.vs[c];
    I.cw[c] = (width * I.hs[c] + hmax - 1) / hmax; I.ch[c] = (height * I.vs[c] + vmax - 1) / vmax;
    blocks += (long)I.bw[c] * I.bh[c];
  }
  I.ncoef = 64 * blocks;
  I.plane_bytes = 64 * blocks;
  return true;
}

// The geometry guard of one table row `d` (cft_jpeg_desc_t or cft_jpeg_enc_desc_t: the fields have the same names) inside the entry
// point `who`, a string literal: CFT_EINVAL unless the sizes and the sampling are in the subset and bw / bh are the grid of that
// geometry; `blocks` receives the row's block count.
#define JPEG_REQUIRE_GEOMETRY(who, d, blocks)                                                                                                  \
  do {                                                                                                                                         \
    CFT_REQUIRE((d).width >= 1 && (d).height >= 1 && (d).width <= CFT_JPEG_MAX_SIDE && (d).height <= CFT_JPEG_MAX_SIDE,                         \
                who ": image size out of range");                                                                                              \
    CFT_REQUIRE((d).ncomp == 1 || (d).ncomp == 3, who ": 1 or 3 components");                                                                  \
    cft_jpeg_info_t geometry_;                                                                                                                 \
    CFT_REQUIRE(jpeg_geometry((d).width, (d).height, (d).ncomp, (d).hmax, (d).vmax, geometry_),                                                \
                who ": sampling outside 1x1 (one component) and luma 1x1, 2x1, 2x2");                                                          \
    CFT_REQUIRE(memcmp((d).bw, geometry_.bw, sizeof geometry_.bw) == 0 && memcmp((d).bh, geometry_.bh, sizeof geometry_.bh) == 0,               \
                who ": block grid does not belong to this size and sampling");                                                                 \
    (blocks) = geometry_.ncoef / 64;                                                                                                           \
  } while (0)

// The coefficient layout: component after component, the blocks of a component in raster order of its padded grid, natural order
// within a block.  base[c] is where component c starts, jpeg_block_at the address of block (gy, gx) of component c in `coef` (the
// sum is taken in this order so that coef + base[c] stays out of the callers' block loops).
static inline void jpeg_comp_bases(const cft_jpeg_info_t& I, long base[3]) {
  base[0] = 0;
  base[1] = 64L * I.bw[0] * I.bh[0];
  base[2] = base[1] + 64L * I.bw[1] * I.bh[1];                       // bw, bh of an absent component are 0
}
template <class T>
static inline T* jpeg_block_at(T* coef, const cft_jpeg_info_t& I, const long base[3], int c, int gy, int gx) {
  return coef + base[c] + 64 * ((long)gy * I.bw[c] + gx);
}

// True when none of the four bytes of w is 0xFF: the bit reader and the bit writer then move the dword as it is.
static inline bool jpeg_no_ff(uint32_t w) {
  const uint32_t x = ~w;                                             // a zero byte of x is a 0xFF byte of w
  return ((x - 0x01010101u) & ~x & 0x80808080u) == 0;
}

// ------------------------------------------------------------------------------------------------ device
// Both DCT kernels: 8 lanes per 8x8 block, 32 blocks per workgroup, a block transposed through LDS at a stride of 64 + 8 dwords (the
// 64 lanes of a wave hit 64 different banks on the column accesses, and a lane moves its row as two 16-byte words).
#define JPEG_THREADS 256
#define JPEG_WG_BLOCKS (JPEG_THREADS / 8)
#define JPEG_LDS_STRIDE 72

// libjpeg's FIX(x) at CONST_BITS 13, the constants of jpeg_idct_islow and jpeg_fdct_islow
constexpr int FIX_0_298631336 = 2446, FIX_0_390180644 = 3196, FIX_0_541196100 = 4433, FIX_0_765366865 = 6270;
constexpr int FIX_0_899976223 = 7373, FIX_1_175875602 = 9633, FIX_1_501321110 = 12299, FIX_1_847759065 = 15137;
constexpr int FIX_1_961570560 = 16069, FIX_2_053119869 = 16819, FIX_2_562915447 = 20995, FIX_3_072711026 = 25172;

__device__ __forceinline__ int jpeg_u8(int v) { return v < 0 ? 0 : (v > 255 ? 255 : v); }

// Which block of image d these 8 lanes work on: `blk` in the coefficient layout, that is block `rel` of component `c`, which
// `before` blocks of earlier components precede; `local` within the workgroup, `lane` within the block.  Not active: past the image.
struct JpegBlock {
  long blk, rel, before;
  int c, local, lane;
  bool active;
};

template <class Row>
__device__ __forceinline__ JpegBlock jpeg_locate(const Row& d) {
  const int nb0 = d.bw[0] * d.bh[0], nb1 = d.ncomp == 3 ? d.bw[1] * d.bh[1] : 0, nb2 = d.ncomp == 3 ? d.bw[2] * d.bh[2] : 0;
  JpegBlock b;
  b.local = threadIdx.x >> 3; b.lane = threadIdx.x & 7;
  b.blk = (long)blockIdx.x * JPEG_WG_BLOCKS + b.local;
  b.active = b.blk < (long)nb0 + nb1 + nb2;
  b.c = 0; b.rel = b.blk; b.before = 0;
  if (b.active && b.rel >= nb0) {
    b.rel -= nb0; b.before = nb0; b.c = 1;
    if (b.rel >= nb1) { b.rel -= nb1; b.before += nb1; b.c = 2; }
  }
  return b;
}
