// Baseline JPEG encoding in two halves, the decoder's (jpeg.hip) in the other direction; include/cft_hip.h defines the arithmetic, and
// jpeg_common.h holds what the two share (geometry, coefficient layout, row guard, zigzag order, DCT constants, workgroup shape).
//
// Host half (cft_jpeg_layout, cft_jpeg_quality_tables, cft_jpeg_write_bound, cft_jpeg_write): geometry, tables, headers and Huffman
// coding, plain C++ without a HIP call.  Re-entrant: the code tables are built on the caller's stack, nothing is allocated, no global
// is written (not even cft_last_error's text).  The writer keeps 64 bits, emits four bytes at a time while they hold no 0xFF and fit,
// and checks every other byte against the capacity.
//
// Device half (cft_jpeg_encode_coef): one launch for a whole batch, grid (work of the largest image, image).
//   jpeg_fdct_kernel   8 lanes per 8x8 block, 32 blocks per workgroup: a lane gathers one row of its block from the source (colour
//                      conversion and the h2v1 / h2v2 box filter on the way, every index clamped), transforms it, the block is transposed
//                      through LDS (JPEG_LDS_STRIDE), the lane transforms and quantises one column, a second transpose gives it the
//                      8 coefficients of one row, stored as one 16-byte word.
// No atomics, no inline assembly, no plane workspace; every coefficient is written once by one thread.  All arithmetic is integer.
#include "jpeg_common.h"

// ------------------------------------------------------------------------------------------------ host half
namespace {

// ITU T.81 Annex K: table K.1 (luminance), K.2 (chrominance), natural order
const unsigned char ENC_BASE_Q[2][64] = {
    {16, 11, 10, 16, 24, 40, 51, 61, 12, 12, 14, 19, 26, 58, 60, 55, 14, 13, 16, 24, 40, 57, 69, 56, 14, 17, 22, 29, 51, 87, 80, 62,
     18, 22, 37, 56, 68, 109, 103, 77, 24, 35, 55, 64, 81, 104, 113, 92, 49, 64, 78, 87, 103, 121, 120, 101, 72, 92, 95, 98, 112, 100, 103, 99},
    {17, 18, 24, 47, 99, 99, 99, 99, 18, 21, 26, 66, 99, 99, 99, 99, 24, 26, 56, 99, 99, 99, 99, 99, 47, 66, 99, 99, 99, 99, 99, 99,
     99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99}};

// Annex K tables K.3 - K.6: code counts per length 1..16, then the symbols
const unsigned char ENC_DC_COUNTS[2][16] = {{0, 1, 5, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0, 0, 0}, {0, 3, 1, 1, 1, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0}};
const unsigned char ENC_DC_VALS[12] = {0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11};
const unsigned char ENC_AC_COUNTS[2][16] = {{0, 2, 1, 3, 3, 2, 4, 3, 5, 5, 4, 4, 0, 0, 1, 0x7d}, {0, 2, 1, 2, 4, 4, 3, 4, 7, 5, 4, 4, 0, 1, 2, 0x77}};
const unsigned char ENC_AC_VALS[2][162] = {
    {0x01, 0x02, 0x03, 0x00, 0x04, 0x11, 0x05, 0x12, 0x21, 0x31, 0x41, 0x06, 0x13, 0x51, 0x61, 0x07, 0x22, 0x71, 0x14, 0x32, 0x81, 0x91, 0xa1, 0x08, 0x23, 0x42, 0xb1,
     0xc1, 0x15, 0x52, 0xd1, 0xf0, 0x24, 0x33, 0x62, 0x72, 0x82, 0x09, 0x0a, 0x16, 0x17, 0x18, 0x19, 0x1a, 0x25, 0x26, 0x27, 0x28, 0x29, 0x2a, 0x34, 0x35, 0x36, 0x37,
     0x38, 0x39, 0x3a, 0x43, 0x44, 0x45, 0x46, 0x47, 0x48, 0x49, 0x4a, 0x53, 0x54, 0x55, 0x56, 0x57, 0x58, 0x59, 0x5a, 0x63, 0x64, 0x65, 0x66, 0x67, 0x68, 0x69, 0x6a,
     0x73, 0x74, 0x75, 0x76, 0x77, 0x78, 0x79, 0x7a, 0x83, 0x84, 0x85, 0x86, 0x87, 0x88, 0x89, 0x8a, 0x92, 0x93, 0x94, 0x95, 0x96, 0x97, 0x98, 0x99, 0x9a, 0xa2, 0xa3,
     0xa4, 0xa5, 0xa6, 0xa7, 0xa8, 0xa9, 0xaa, 0xb2, 0xb3, 0xb4, 0xb5, 0xb6, 0xb7, 0xb8, 0xb9, 0xba, 0xc2, 0xc3, 0xc4, 0xc5, 0xc6, 0xc7, 0xc8, 0xc9, 0xca, 0xd2, 0xd3,
     0xd4, 0xd5, 0xd6, 0xd7, 0xd8, 0xd9, 0xda, 0xe1, 0xe2, 0xe3, 0xe4, 0xe5, 0xe6, 0xe7, 0xe8, 0xe9, 0xea, 0xf1, 0xf2, 0xf3, 0xf4, 0xf5, 0xf6, 0xf7, 0xf8, 0xf9, 0xfa},
    {0x00, 0x01, 0x02, 0x03, 0x11, 0x04, 0x05, 0x21, 0x31, 0x06, 0x12, 0x41, 0x51, 0x07, 0x61, 0x71, 0x13, 0x22, 0x32, 0x81, 0x08, 0x14, 0x42, 0x91, 0xa1, 0xb1, 0xc1,
     0x09, 0x23, 0x33, 0x52, 0xf0, 0x15, 0x62, 0x72, 0xd1, 0x0a, 0x16, 0x24, 0x34, 0xe1, 0x25, 0xf1, 0x17, 0x18, 0x19, 0x1a, 0x26, 0x27, 0x28, 0x29, 0x2a, 0x35, 0x36,
     0x37, 0x38, 0x39, 0x3a, 0x43, 0x44, 0x45, 0x46, 0x47, 0x48, 0x49, 0x4a, 0x53, 0x54, 0x55, 0x56, 0x57, 0x58, 0x59, 0x5a, 0x63, 0x64, 0x65, 0x66, 0x67, 0x68, 0x69,
     0x6a, 0x73, 0x74, 0x75, 0x76, 0x77, 0x78, 0x79, 0x7a, 0x82, 0x83, 0x84, 0x85, 0x86, 0x87, 0x88, 0x89, 0x8a, 0x92, 0x93, 0x94, 0x95, 0x96, 0x97, 0x98, 0x99, 0x9a,
     0xa2, 0xa3, 0xa4, 0xa5, 0xa6, 0xa7, 0xa8, 0xa9, 0xaa, 0xb2, 0xb3, 0xb4, 0xb5, 0xb6, 0xb7, 0xb8, 0xb9, 0xba, 0xc2, 0xc3, 0xc4, 0xc5, 0xc6, 0xc7, 0xc8, 0xc9, 0xca,
     0xd2, 0xd3, 0xd4, 0xd5, 0xd6, 0xd7, 0xd8, 0xd9, 0xda, 0xe2, 0xe3, 0xe4, 0xe5, 0xe6, 0xe7, 0xe8, 0xe9, 0xea, 0xf2, 0xf3, 0xf4, 0xf5, 0xf6, 0xf7, 0xf8, 0xf9, 0xfa}};

#define ENC_BLOCK_BOUND 416            // bytes one block can take: (63 * (16 + 10) + 11 + 11) bits, rounded up, every byte stuffed

struct EncCode {
  uint16_t code[256];
  unsigned char len[256];              // 0 = the table has no code for this symbol
};

void enc_make_code(EncCode& c, const unsigned char* counts, const unsigned char* vals) {
  memset(&c, 0, sizeof c);
  int code = 0, k = 0;
  for (int len = 1; len <= 16; ++len) {
    for (int i = 0; i < counts[len - 1]; ++i, ++k, ++code) { c.code[vals[k]] = (uint16_t)code; c.len[vals[k]] = (unsigned char)len; }
    code <<= 1;
  }
}

// true when `info` is what jpeg_geometry gives for its own first five fields
bool enc_info_ok(const cft_jpeg_info_t* info) {
  cft_jpeg_info_t I;
  return jpeg_geometry(info->width, info->height, info->ncomp, info->hmax, info->vmax, I) && memcmp(&I, info, sizeof I) == 0;
}

long enc_header_bytes(int ncomp) {
  const int tables = ncomp == 3 ? 2 : 1;
  return 2 + 18 + 69L * tables + (10 + 3 * ncomp) + tables * (33L + 183L) + (8 + 2 * ncomp);
}

struct EncOut {
  unsigned char* p;
  unsigned char* end;
  uint64_t acc;                        // the pending bits, in the low `bits` bits
  int bits;
  bool full;
};

inline void enc_byte(EncOut& o, unsigned v) {
  if (o.p < o.end) *o.p++ = (unsigned char)v; else o.full = true;
}

inline void enc_bytes(EncOut& o, const unsigned char* src, int n) {
  for (int i = 0; i < n; ++i) enc_byte(o, src[i]);
}

// n <= 26 bits at a time; the accumulator is drained to below 32 bits whenever it reaches 32
inline void enc_put(EncOut& o, unsigned v, int n) {
  o.acc = (o.acc << n) | v;
  o.bits += n;
  if (o.bits < 32) return;
  const int rest = o.bits - 32;
  const uint32_t w = (uint32_t)(o.acc >> rest);
  if (jpeg_no_ff(w) && o.end - o.p >= 4) {
    o.p[0] = (unsigned char)(w >> 24); o.p[1] = (unsigned char)(w >> 16); o.p[2] = (unsigned char)(w >> 8); o.p[3] = (unsigned char)w;
    o.p += 4;
  } else {
    for (int s = 24; s >= 0; s -= 8) {
      const unsigned b = (w >> s) & 255u;
      enc_byte(o, b);
      if (b == 0xFF) enc_byte(o, 0);
    }
  }
  o.bits = rest;
  o.acc &= (1ull << rest) - 1;
}

inline void enc_flush(EncOut& o) {                                 // whole bytes, then the last one padded with 1-bits
  while (o.bits >= 8) {
    const unsigned b = (unsigned)(o.acc >> (o.bits - 8)) & 255u;
    enc_byte(o, b);
    if (b == 0xFF) enc_byte(o, 0);
    o.bits -= 8;
  }
  if (o.bits) {
    const unsigned b = (((unsigned)o.acc << (8 - o.bits)) | ((1u << (8 - o.bits)) - 1)) & 255u;
    enc_byte(o, b);
    if (b == 0xFF) enc_byte(o, 0);
    o.bits = 0;
  }
  o.acc = 0;
}

inline int enc_category(int v) {
  const unsigned a = (unsigned)(v < 0 ? -v : v);
  return a ? 32 - __builtin_clz(a) : 0;
}

inline void enc_segment(EncOut& o, int marker, const unsigned char* body, int n) {
  enc_byte(o, 0xFF); enc_byte(o, (unsigned)marker);
  enc_byte(o, (unsigned)((n + 2) >> 8)); enc_byte(o, (unsigned)((n + 2) & 255));
  enc_bytes(o, body, n);
}

}  // namespace

extern "C" int cft_jpeg_layout(int width, int height, int ncomp, int hmax, int vmax, cft_jpeg_info_t* info) {
  if (!info) return CFT_EINVAL;
  cft_jpeg_info_t I;
  if (!jpeg_geometry(width, height, ncomp, hmax, vmax, I)) return CFT_EINVAL;
  *info = I;
  return CFT_OK;
}

extern "C" int cft_jpeg_quality_tables(int quality, unsigned short* qtab) {
  if (!qtab || quality < 1 || quality > 100) return CFT_EINVAL;
  const int scale = quality < 50 ? 5000 / quality : 200 - 2 * quality;
  for (int c = 0; c < 3; ++c)
    for (int i = 0; i < 64; ++i) {
      const int q = (ENC_BASE_Q[c ? 1 : 0][i] * scale + 50) / 100;
      qtab[c * 64 + i] = (unsigned short)(q < 1 ? 1 : (q > 255 ? 255 : q));
    }
  return CFT_OK;
}

extern "C" int cft_jpeg_write_bound(const cft_jpeg_info_t* info, long* bound) {
  if (bound) *bound = -1;
  if (!info || !bound || !enc_info_ok(info)) return CFT_EINVAL;
  *bound = enc_header_bytes(info->ncomp) + (long)ENC_BLOCK_BOUND * (info->ncoef / 64) + 2;
  return CFT_OK;
}

extern "C" int cft_jpeg_write(const short* coef, const unsigned short* qtab, const cft_jpeg_info_t* info, unsigned char* out, long cap, long* nbytes) {
  if (nbytes) *nbytes = 0;
  if (!coef || !qtab || !info || !out || !nbytes || cap < 0) return CFT_EINVAL;
  if (!enc_info_ok(info)) return CFT_EINVAL;
  const cft_jpeg_info_t& I = *info;
  for (int c = 0; c < I.ncomp; ++c)
    for (int i = 0; i < 64; ++i) {
      if (qtab[c * 64 + i] < 1 || qtab[c * 64 + i] > 255) return CFT_EINVAL;
      if (c == 2 && qtab[128 + i] != qtab[64 + i]) return CFT_EINVAL;   // the file carries one chrominance table
    }
  EncOut o = {out, out + cap, 0, 0, false};
  unsigned char seg[200];
  enc_byte(o, 0xFF); enc_byte(o, 0xD8);
  const unsigned char jfif[14] = {'J', 'F', 'I', 'F', 0, 1, 1, 0, 0, 1, 0, 1, 0, 0};
  enc_segment(o, 0xE0, jfif, 14);
  const int tables = I.ncomp == 3 ? 2 : 1;
  for (int t = 0; t < tables; ++t) {
    seg[0] = (unsigned char)t;
    for (int i = 0; i < 64; ++i) seg[1 + i] = (unsigned char)qtab[t * 64 + JPEG_ZIGZAG[i]];
    enc_segment(o, 0xDB, seg, 65);
  }
  seg[0] = 8;
  seg[1] = (unsigned char)(I.height >> 8); seg[2] = (unsigned char)(I.height & 255);
  seg[3] = (unsigned char)(I.width >> 8); seg[4] = (unsigned char)(I.width & 255);
  seg[5] = (unsigned char)I.ncomp;
  for (int c = 0; c < I.ncomp; ++c) {
    seg[6 + 3 * c] = (unsigned char)(c + 1);
    seg[7 + 3 * c] = (unsigned char)((I.hs[c] << 4) | I.vs[c]);
    seg[8 + 3 * c] = (unsigned char)(c ? 1 : 0);
  }
  enc_segment(o, 0xC0, seg, 6 + 3 * I.ncomp);
  EncCode dc[2], ac[2];
  for (int t = 0; t < tables; ++t) {
    enc_make_code(dc[t], ENC_DC_COUNTS[t], ENC_DC_VALS);
    enc_make_code(ac[t], ENC_AC_COUNTS[t], ENC_AC_VALS[t]);
    seg[0] = (unsigned char)t;
    memcpy(seg + 1, ENC_DC_COUNTS[t], 16); memcpy(seg + 17, ENC_DC_VALS, 12);
    enc_segment(o, 0xC4, seg, 29);
    seg[0] = (unsigned char)(0x10 | t);
    memcpy(seg + 1, ENC_AC_COUNTS[t], 16); memcpy(seg + 17, ENC_AC_VALS[t], 162);
    enc_segment(o, 0xC4, seg, 179);
  }
  seg[0] = (unsigned char)I.ncomp;
  for (int c = 0; c < I.ncomp; ++c) { seg[1 + 2 * c] = (unsigned char)(c + 1); seg[2 + 2 * c] = (unsigned char)(c ? 0x11 : 0x00); }
  seg[1 + 2 * I.ncomp] = 0; seg[2 + 2 * I.ncomp] = 63; seg[3 + 2 * I.ncomp] = 0;
  enc_segment(o, 0xDA, seg, 4 + 2 * I.ncomp);
  if (o.full) return CFT_JPEG_SHORT_BUFFER;

  long base[3];
  jpeg_comp_bases(I, base);
  int real_bw[3], real_bh[3];
  for (int c = 0; c < 3; ++c) { real_bw[c] = (I.cw[c] + 7) / 8; real_bh[c] = (I.ch[c] + 7) / 8; }   // 0 for an absent component
  int pred[3] = {0, 0, 0};
  for (int my = 0; my < I.mcus_y; ++my) {
    for (int mx = 0; mx < I.mcus_x; ++mx) {
      for (int c = 0; c < I.ncomp; ++c) {
        const EncCode& hd = dc[c ? 1 : 0];
        const EncCode& ha = ac[c ? 1 : 0];
        for (int by = 0; by < I.vs[c]; ++by) {
          for (int bx = 0; bx < I.hs[c]; ++bx) {
            const int gy = my * I.vs[c] + by, gx = mx * I.hs[c] + bx;
            if (gy >= real_bh[c] || gx >= real_bw[c]) {                 // dummy block: the previous DC again, no AC
              enc_put(o, hd.code[0], hd.len[0]);
              enc_put(o, ha.code[0], ha.len[0]);
              continue;
            }
            const short* blk = jpeg_block_at(coef, I, base, c, gy, gx);
            const int diff = (int)blk[0] - pred[c];
            pred[c] = blk[0];
            int s = enc_category(diff);
            if (s > 11) return CFT_JPEG_UNSUPPORTED;
            enc_put(o, hd.code[s], hd.len[s]);
            if (s) enc_put(o, (unsigned)(diff < 0 ? diff - 1 : diff) & ((1u << s) - 1), s);
            uint64_t nz = 0;                                          // bit k: the k-th coefficient in zigzag order is not zero
#pragma unroll
            for (int k = 1; k < 64; ++k) nz |= (uint64_t)(blk[JPEG_ZIGZAG[k]] != 0) << k;
            int prev = 0;
            while (nz) {
              const int k = __builtin_ctzll(nz);
              nz &= nz - 1;
              int run = k - prev - 1;
              prev = k;
              while (run > 15) { enc_put(o, ha.code[0xF0], ha.len[0xF0]); run -= 16; }
              const int v = blk[JPEG_ZIGZAG[k]];
              s = enc_category(v);
              if (s > 10) return CFT_JPEG_UNSUPPORTED;
              const int rs = (run << 4) | s;
              enc_put(o, ((unsigned)ha.code[rs] << s) | ((unsigned)(v < 0 ? v - 1 : v) & ((1u << s) - 1)), ha.len[rs] + s);
            }
            if (prev != 63) enc_put(o, ha.code[0], ha.len[0]);
            if (o.full) return CFT_JPEG_SHORT_BUFFER;
          }
        }
      }
    }
  }
  enc_flush(o);
  enc_byte(o, 0xFF); enc_byte(o, 0xD9);
  if (o.full) return CFT_JPEG_SHORT_BUFFER;
  *nbytes = (long)(o.p - out);
  return CFT_OK;
}

// ------------------------------------------------------------------------------------------------ device half
#define ENC_DESCALE(x, n) (((x) + (1 << ((n) - 1))) >> (n))

// jpeg_fdct_islow's one-dimensional butterfly on v[0..7], in place: the row pass (PASS1) scales up by PASS1_BITS, the column pass
// removes it again.  Even part, odd part: the published order of operations.
template <bool PASS1>
__device__ __forceinline__ void enc_fdct_1d(int v[8]) {
  const int t0 = v[0] + v[7], t7 = v[0] - v[7], t1 = v[1] + v[6], t6 = v[1] - v[6];
  const int t2 = v[2] + v[5], t5 = v[2] - v[5], t3 = v[3] + v[4], t4 = v[3] - v[4];
  const int t10 = t0 + t3, t13 = t0 - t3, t11 = t1 + t2, t12 = t1 - t2;
  constexpr int N = PASS1 ? 11 : 15;
  if (PASS1) { v[0] = (t10 + t11) * 4; v[4] = (t10 - t11) * 4; }
  else       { v[0] = ENC_DESCALE(t10 + t11, 2); v[4] = ENC_DESCALE(t10 - t11, 2); }
  int z1 = (t12 + t13) * FIX_0_541196100;
  v[2] = ENC_DESCALE(z1 + t13 * FIX_0_765366865, N);
  v[6] = ENC_DESCALE(z1 - t12 * FIX_1_847759065, N);
  z1 = t4 + t7;
  int z2 = t5 + t6, z3 = t4 + t6, z4 = t5 + t7;
  const int z5 = (z3 + z4) * FIX_1_175875602;
  const int a4 = t4 * FIX_0_298631336, a5 = t5 * FIX_2_053119869, a6 = t6 * FIX_3_072711026, a7 = t7 * FIX_1_501321110;
  z1 *= -FIX_0_899976223; z2 *= -FIX_2_562915447;
  z3 = z3 * -FIX_1_961570560 + z5; z4 = z4 * -FIX_0_390180644 + z5;
  v[7] = ENC_DESCALE(a4 + z1 + z3, N);
  v[5] = ENC_DESCALE(a5 + z2 + z4, N);
  v[3] = ENC_DESCALE(a6 + z2 + z3, N);
  v[1] = ENC_DESCALE(a7 + z1 + z4, N);
}

// One component value of each of NP consecutive pixels x0 .. x0 + NP - 1 of an RGB row (x clamped to width - 1):
// (kr R + kg G + kb B + kadd) >> 16.  Whole dwords when the span lies inside the row and starts on a 4-byte boundary.
template <int NP>
__device__ __forceinline__ void enc_row_rgb(const unsigned char* __restrict__ row, int x0, int width, int kr, int kg, int kb, int kadd, int* out) {
  const unsigned char* p = row + 3L * x0;
  if (x0 + NP <= width && ((uintptr_t)p & 3) == 0) {
    unsigned int w[3 * NP / 4];
#pragma unroll
    for (int i = 0; i < 3 * NP / 4; ++i) w[i] = reinterpret_cast<const unsigned int*>(p)[i];
#pragma unroll
    for (int j = 0; j < NP; ++j) {
      const int r = (int)((w[(3 * j) >> 2] >> (8 * ((3 * j) & 3))) & 255u);
      const int g = (int)((w[(3 * j + 1) >> 2] >> (8 * ((3 * j + 1) & 3))) & 255u);
      const int b = (int)((w[(3 * j + 2) >> 2] >> (8 * ((3 * j + 2) & 3))) & 255u);
      out[j] = (kr * r + kg * g + kb * b + kadd) >> 16;
    }
  } else {
#pragma unroll
    for (int j = 0; j < NP; ++j) {
      const unsigned char* q = row + 3L * min(x0 + j, width - 1);
      out[j] = (kr * (int)q[0] + kg * (int)q[1] + kb * (int)q[2] + kadd) >> 16;
    }
  }
}

__global__ void __launch_bounds__(JPEG_THREADS) jpeg_fdct_kernel(const cft_jpeg_enc_desc_t* __restrict__ table) {
  __shared__ __attribute__((aligned(16))) int tile[2][JPEG_WG_BLOCKS * JPEG_LDS_STRIDE];
  const cft_jpeg_enc_desc_t& d = table[blockIdx.y];                // uniform over the workgroup
  const int W = d.width, H = d.height;
  const JpegBlock b = jpeg_locate(d);
  const int c = b.c, local = b.local, lane = b.lane;
  const long blk = b.blk, rel = b.rel;
  const bool active = b.active;
  const int bw = active ? d.bw[c] : 1;
  const int by = (int)(rel / bw), bx = (int)(rel % bw);
  const int fx = c ? d.hmax : 1, fy = c ? d.vmax : 1;              // how much this component is downsampled
  const int cw = (W + fx - 1) / fx, ch = (H + fy - 1) / fy;
  const bool real = active && bx < (cw + 7) / 8 && by < (ch + 7) / 8;
  int v[8];
  int* t0 = tile[0] + local * JPEG_LDS_STRIDE;
  int* t1 = tile[1] + local * JPEG_LDS_STRIDE;
  if (real) {
    const int sy = min(by * 8 + lane, ch - 1);                     // rows past ch repeat the last downsampled row
    if (d.ncomp == 1) {
      const unsigned char* row = d.src + (long)sy * d.src_stride;
#pragma unroll
      for (int j = 0; j < 8; ++j) v[j] = (int)row[min(bx * 8 + j, W - 1)] - 128;
    } else {
      const int kr = c == 0 ? 19595 : (c == 1 ? -11059 : 32768);
      const int kg = c == 0 ? 38470 : (c == 1 ? -21709 : -27439);
      const int kb = c == 0 ? 7471 : (c == 1 ? 32768 : -5329);
      const int kadd = c == 0 ? 32768 : (128 << 16) + 32767;
      if (fx == 1) {
        enc_row_rgb<8>(d.src + (long)sy * d.src_stride, bx * 8, W, kr, kg, kb, kadd, v);
#pragma unroll
        for (int j = 0; j < 8; ++j) v[j] -= 128;
      } else {
        int s[16];
        enc_row_rgb<16>(d.src + (long)min(fy * sy, H - 1) * d.src_stride, bx * 16, W, kr, kg, kb, kadd, s);
        if (fy == 1) {
#pragma unroll
          for (int j = 0; j < 8; ++j) v[j] = ((s[2 * j] + s[2 * j + 1] + (j & 1)) >> 1) - 128;
        } else {
          int u[16];
          enc_row_rgb<16>(d.src + (long)min(2 * sy + 1, H - 1) * d.src_stride, bx * 16, W, kr, kg, kb, kadd, u);
#pragma unroll
          for (int j = 0; j < 8; ++j) v[j] = ((s[2 * j] + s[2 * j + 1] + u[2 * j] + u[2 * j + 1] + 1 + (j & 1)) >> 2) - 128;
        }
      }
    }
    enc_fdct_1d<true>(v);                                          // row `lane`
    *reinterpret_cast<int4*>(t0 + lane * 8) = make_int4(v[0], v[1], v[2], v[3]);
    *reinterpret_cast<int4*>(t0 + lane * 8 + 4) = make_int4(v[4], v[5], v[6], v[7]);
  }
  __syncthreads();
  if (real) {
#pragma unroll
    for (int r = 0; r < 8; ++r) v[r] = t0[r * 8 + lane];
    enc_fdct_1d<false>(v);                                         // column `lane`
    const unsigned short* q = d.qtab + c * 64 + lane;
#pragma unroll
    for (int r = 0; r < 8; ++r) {
      const unsigned int div = max((unsigned int)q[r * 8], 1u) << 3;
      const unsigned int a = (unsigned int)(v[r] < 0 ? -v[r] : v[r]);
      const int m = (int)((a + (div >> 1)) / div);
      t1[r * 8 + lane] = v[r] < 0 ? -m : m;
    }
  }
  __syncthreads();
  if (!active) return;
  uint4 out = make_uint4(0u, 0u, 0u, 0u);                          // a dummy block is 64 zeros
  if (real) {
    const int4 lo = *reinterpret_cast<const int4*>(t1 + lane * 8);
    const int4 hi = *reinterpret_cast<const int4*>(t1 + lane * 8 + 4);
    out.x = ((unsigned)lo.x & 0xFFFFu) | ((unsigned)lo.y << 16);
    out.y = ((unsigned)lo.z & 0xFFFFu) | ((unsigned)lo.w << 16);
    out.z = ((unsigned)hi.x & 0xFFFFu) | ((unsigned)hi.y << 16);
    out.w = ((unsigned)hi.z & 0xFFFFu) | ((unsigned)hi.w << 16);
  }
  *reinterpret_cast<uint4*>(d.coef + blk * 64 + lane * 8) = out;
}

extern "C" int cft_jpeg_encode_coef(const void* table_dev, const void* table_host, int n, void* stream) {
  static_assert(sizeof(cft_jpeg_enc_desc_t) == CFT_JPEG_ENC_DESC_BYTES, "cft_jpeg_enc_desc_t layout");
  CFT_REQUIRE(table_dev && table_host, "cft_jpeg_encode_coef: null pointer");
  CFT_REQUIRE(((uintptr_t)table_dev & 7) == 0 && ((uintptr_t)table_host & 7) == 0, "cft_jpeg_encode_coef: misaligned table");
  CFT_REQUIRE(n > 0 && n <= 65535, "cft_jpeg_encode_coef: image count out of range (1..65535)");
  const cft_jpeg_enc_desc_t* rows = static_cast<const cft_jpeg_enc_desc_t*>(table_host);
  long max_blocks = 0;
  for (int i = 0; i < n; ++i) {
    const cft_jpeg_enc_desc_t& d = rows[i];
    CFT_REQUIRE(d.src && d.qtab && d.qtab_host && d.coef, "cft_jpeg_encode_coef: null pointer in the table");
    CFT_REQUIRE(((uintptr_t)d.qtab & 1) == 0 && ((uintptr_t)d.qtab_host & 1) == 0, "cft_jpeg_encode_coef: misaligned tables");
    CFT_REQUIRE(((uintptr_t)d.coef & 15) == 0, "cft_jpeg_encode_coef: coefficients not 16-byte aligned");
    long blocks;
    JPEG_REQUIRE_GEOMETRY("cft_jpeg_encode_coef", d, blocks);
    CFT_REQUIRE(d.src_stride >= (long)d.ncomp * d.width, "cft_jpeg_encode_coef: bad source row stride");
    for (int k = 0; k < 64 * d.ncomp; ++k)
      CFT_REQUIRE(d.qtab_host[k] >= 1 && d.qtab_host[k] <= 255, "cft_jpeg_encode_coef: quantisation table entry outside 1..255");
    max_blocks = blocks > max_blocks ? blocks : max_blocks;
  }
  hipLaunchKernelGGL(jpeg_fdct_kernel, dim3((unsigned)((max_blocks + JPEG_WG_BLOCKS - 1) / JPEG_WG_BLOCKS), n), dim3(JPEG_THREADS), 0, as_stream(stream),
                     static_cast<const cft_jpeg_enc_desc_t*>(table_dev));
  return cft_check_launch("jpeg_fdct_kernel");
}
