// Baseline JPEG decoding in two halves (include/cft_hip.h, where the subset and the arithmetic are defined).  What the decoder shares
// with the encoder (jpeg_encode.hip) is in jpeg_common.h: the geometry of a file, the coefficient layout, the geometry guard of a table
// row, the zigzag order, the DCT constants and the workgroup shape of the DCT kernels.
//
// Host half (cft_jpeg_info, cft_jpeg_entropy): marker parsing and Huffman decoding, plain C++ without a HIP call.  It is re-entrant: the
// parse state lives on the caller's stack, nothing is allocated, no global is written (not even cft_last_error's text), so a pool of
// threads can decode files side by side.  Every read is checked against nbytes and every write lands inside the sizes cft_jpeg_info
// reported, whatever the bytes are.  The bit reader keeps 64 bits, refills four bytes at a time while they hold no 0xFF, and a
// 9-bit table resolves the short Huffman codes; longer ones walk the canonical code ranges.
//
// Device half (cft_jpeg_decode_u8): two launches for a whole batch, grid (work of the largest image, image).
//   jpeg_idct_kernel   8 lanes per 8x8 block, 32 blocks per workgroup: a lane dequantises and transforms one column, the block is
//                      transposed through LDS (JPEG_LDS_STRIDE), the lane transforms one row and stores its 8 bytes as one 8-byte
//                      word into the component's plane.
//   jpeg_colour_kernel one thread per 4 consecutive pixels of a row: luma as one dword, chroma through the h2v1 / h2v2 triangle taps
//                      with every neighbour index clamped to the component's downsampled size, YCbCr -> RGB, 12 bytes out.
// No atomics, no inline assembly; every plane byte and every output byte is written once by one thread.  All arithmetic is integer.
#include "jpeg_common.h"

// ------------------------------------------------------------------------------------------------ host half
namespace {

#define JPG_LUT_BITS 9

struct JpgHuff {
  uint16_t lut[1 << JPG_LUT_BITS];     // (length << 8) | symbol of the code that starts these 9 bits, 0 = longer than 9 bits or none
  int mincode[17], maxcode[17];        // per length 1..16; maxcode -1 = no code of that length
  int first[17];                       // index in vals of the first symbol of that length
  unsigned char vals[256];
  bool defined;
};

struct JpgParse {
  cft_jpeg_info_t info;
  uint16_t q[4][64];                   // natural order
  bool qdef[4];
  JpgHuff dc[4], ac[4];
  int tq[3], td[3], ta[3];
  long scan;                           // offset of the first entropy-coded byte
};

inline int jpg_be16(const unsigned char* p) { return (p[0] << 8) | p[1]; }

bool jpg_build_huff(JpgHuff& h, const unsigned char* counts, const unsigned char* syms, int nsyms) {
  memset(h.lut, 0, sizeof h.lut);
  int code = 0, k = 0;
  for (int len = 1; len <= 16; ++len) {
    const int cnt = counts[len - 1];
    h.first[len] = k;
    h.mincode[len] = code;
    h.maxcode[len] = cnt ? code + cnt - 1 : -1;
    for (int i = 0; i < cnt; ++i, ++code, ++k) {
      if (k >= nsyms || code >= (1 << len)) return false;
      h.vals[k] = syms[k];
      if (len <= JPG_LUT_BITS) {
        const int lo = code << (JPG_LUT_BITS - len), n = 1 << (JPG_LUT_BITS - len);
        for (int j = 0; j < n; ++j) h.lut[lo + j] = (uint16_t)((len << 8) | syms[k]);
      }
    }
    code <<= 1;
  }
  h.defined = true;
  return true;
}

// Markers from SOI up to and including SOS.  CFT_OK or CFT_JPEG_UNSUPPORTED.
int jpg_parse(const unsigned char* d, long n, JpgParse& P) {
  memset(&P.info, 0, sizeof P.info);
  for (int i = 0; i < 4; ++i) { P.qdef[i] = false; P.dc[i].defined = false; P.ac[i].defined = false; }
  if (n < 4 || d[0] != 0xFF || d[1] != 0xD8) return CFT_JPEG_UNSUPPORTED;
  long pos = 2;
  bool sof = false, jfif = false, adobe = false;
  int adobe_transform = -1, comp_id[3] = {0, 0, 0}, nc = 0, restart = 0;
  cft_jpeg_info_t& I = P.info;
  for (;;) {
    if (pos + 2 > n || d[pos] != 0xFF) return CFT_JPEG_UNSUPPORTED;
    while (pos < n && d[pos] == 0xFF) ++pos;                       // fill bytes
    if (pos >= n) return CFT_JPEG_UNSUPPORTED;
    const int m = d[pos++];
    if (pos + 2 > n) return CFT_JPEG_UNSUPPORTED;
    const long len = jpg_be16(d + pos);
    if (len < 2 || pos + len > n) return CFT_JPEG_UNSUPPORTED;
    const unsigned char* seg = d + pos + 2;
    long sl = len - 2;
    if (m == 0xC0) {                                               // SOF0
      if (sof || sl < 6) return CFT_JPEG_UNSUPPORTED;
      const int prec = seg[0], H = jpg_be16(seg + 1), W = jpg_be16(seg + 3);
      nc = seg[5];
      if (prec != 8 || H < 1 || W < 1 || H > CFT_JPEG_MAX_SIDE || W > CFT_JPEG_MAX_SIDE || (nc != 1 && nc != 3) || sl != 6 + 3 * nc) return CFT_JPEG_UNSUPPORTED;
      for (int c = 0; c < nc; ++c) {
        comp_id[c] = seg[6 + 3 * c];
        I.hs[c] = seg[7 + 3 * c] >> 4; I.vs[c] = seg[7 + 3 * c] & 15;
        P.tq[c] = seg[8 + 3 * c];
        if (P.tq[c] > 3) return CFT_JPEG_UNSUPPORTED;
      }
      I.width = W; I.height = H; I.ncomp = nc;
      sof = true;
    } else if (m == 0xC4) {                                        // DHT
      while (sl > 0) {
        if (sl < 17) return CFT_JPEG_UNSUPPORTED;
        const int tc = seg[0] >> 4, th = seg[0] & 15;
        int total = 0;
        for (int i = 0; i < 16; ++i) total += seg[1 + i];
        if (tc > 1 || th > 3 || total > 256 || sl < 17 + total) return CFT_JPEG_UNSUPPORTED;
        if (!jpg_build_huff(tc ? P.ac[th] : P.dc[th], seg + 1, seg + 17, total)) return CFT_JPEG_UNSUPPORTED;
        seg += 17 + total; sl -= 17 + total;
      }
    } else if (m == 0xDB) {                                        // DQT
      while (sl > 0) {
        const int pq = seg[0] >> 4, t = seg[0] & 15;
        if (pq != 0 || t > 3 || sl < 65) return CFT_JPEG_UNSUPPORTED;
        for (int i = 0; i < 64; ++i) P.q[t][JPEG_ZIGZAG[i]] = seg[1 + i];
        P.qdef[t] = true;
        seg += 65; sl -= 65;
      }
    } else if (m == 0xDD) {                                        // DRI
      if (sl != 2) return CFT_JPEG_UNSUPPORTED;
      restart = jpg_be16(seg);
    } else if (m == 0xE0) {
      if (sl >= 5 && memcmp(seg, "JFIF", 5) == 0) jfif = true;
    } else if (m == 0xEE) {
      if (sl >= 12 && memcmp(seg, "Adobe", 5) == 0) { adobe = true; adobe_transform = seg[11]; }
    } else if (m == 0xDA) {                                        // SOS
      if (!sof || sl != 4 + 2 * nc || seg[0] != nc) return CFT_JPEG_UNSUPPORTED;
      for (int c = 0; c < nc; ++c) {
        if (seg[1 + 2 * c] != comp_id[c]) return CFT_JPEG_UNSUPPORTED;
        P.td[c] = seg[2 + 2 * c] >> 4; P.ta[c] = seg[2 + 2 * c] & 15;
        if (P.td[c] > 3 || P.ta[c] > 3 || !P.dc[P.td[c]].defined || !P.ac[P.ta[c]].defined || !P.qdef[P.tq[c]]) return CFT_JPEG_UNSUPPORTED;
      }
      if (seg[1 + 2 * nc] != 0 || seg[2 + 2 * nc] != 63 || seg[3 + 2 * nc] != 0) return CFT_JPEG_UNSUPPORTED;
      P.scan = pos + len;
      break;
    } else if ((m >= 0xE1 && m <= 0xEF) || m == 0xFE) {
      // other APPn, COM: skipped
    } else {
      return CFT_JPEG_UNSUPPORTED;                                  // other SOFs, DAC, DNL, DHP, EXP, RSTn, EOI, TEM, reserved
    }
    pos += len;
  }
  // colour space: what libjpeg would convert from must be YCbCr (or one grey component)
  if (adobe && nc == 3 && adobe_transform != 1) return CFT_JPEG_UNSUPPORTED;
  if (nc == 3 && !jfif && !adobe && comp_id[0] == 'R' && comp_id[1] == 'G' && comp_id[2] == 'B') return CFT_JPEG_UNSUPPORTED;
  // sampling: chroma 1x1 and a luma sampling of the subset; the rest of the info follows from these five numbers
  for (int c = 1; c < nc; ++c)
    if (I.hs[c] != 1 || I.vs[c] != 1) return CFT_JPEG_UNSUPPORTED;
  if (!jpeg_geometry(I.width, I.height, nc, I.hs[0], I.vs[0], I)) return CFT_JPEG_UNSUPPORTED;
  I.restart_interval = restart;
  if (nc == 3 && I.hmax == 2 && I.cw[1] <= 2 && !(I.cw[1] == 1 && (I.vmax == 1 || I.ch[1] == 1))) return CFT_JPEG_UNSUPPORTED;   // libjpeg replicates here
  return CFT_OK;
}

struct JpgBits {
  const unsigned char* p;
  const unsigned char* end;
  uint64_t buf;                        // the next bits, most significant first
  int bits;                            // how many of them are real
  bool marker;                         // a marker (or the end of the bytes) stops the feed
};

inline void jpg_refill(JpgBits& b) {
  if (b.bits <= 32 && !b.marker && b.end - b.p >= 4) {
    const uint32_t w = ((uint32_t)b.p[0] << 24) | ((uint32_t)b.p[1] << 16) | ((uint32_t)b.p[2] << 8) | b.p[3];
    if (jpeg_no_ff(w)) {
      b.buf |= (uint64_t)w << (32 - b.bits);
      b.bits += 32; b.p += 4;
      return;
    }
  }
  while (b.bits <= 56 && !b.marker) {
    if (b.p >= b.end) { b.marker = true; break; }
    const unsigned v = *b.p;
    if (v == 0xFF) {
      if (b.end - b.p < 2 || b.p[1] != 0) { b.marker = true; break; }
      b.p += 2;                                                    // a stuffed 0xFF 0x00
    } else {
      ++b.p;
    }
    b.buf |= (uint64_t)v << (56 - b.bits);
    b.bits += 8;
  }
}

inline void jpg_consume(JpgBits& b, int n) { b.buf <<= n; b.bits -= n; }

// One Huffman symbol, -1 when the bits run out or match no code.
inline int jpg_symbol(JpgBits& b, const JpgHuff& h) {
  if (b.bits < 16) jpg_refill(b);
  const unsigned e = h.lut[b.buf >> (64 - JPG_LUT_BITS)];
  if (e) {
    const int len = e >> 8;
    if (len > b.bits) return -1;
    jpg_consume(b, len);
    return e & 255;
  }
  for (int len = JPG_LUT_BITS + 1; len <= 16; ++len) {
    if (len > b.bits) return -1;
    const int code = (int)(b.buf >> (64 - len));
    if (h.maxcode[len] >= 0 && code >= h.mincode[len] && code <= h.maxcode[len]) {
      jpg_consume(b, len);
      return h.vals[h.first[len] + code - h.mincode[len]];
    }
  }
  return -1;
}

// s extra bits (1..16) as the signed value they stand for; false when the bits run out.
inline bool jpg_receive(JpgBits& b, int s, int& v) {
  if (b.bits < s) { jpg_refill(b); if (b.bits < s) return false; }
  v = (int)(b.buf >> (64 - s));
  jpg_consume(b, s);
  if (v < (1 << (s - 1))) v -= (1 << s) - 1;
  return true;
}

inline bool jpg_fits(int v, int q) {
  const int a = v < 0 ? -v : v;
  return a <= 32767 && a * q <= 32767;
}

// Byte-align at the end of an interval or of the scan and take the marker `want` (after optional fill bytes).
inline bool jpg_take_marker(JpgBits& b, int want) {
  if (b.bits >= 8) return false;                                   // whole bytes nobody decoded
  b.buf = 0; b.bits = 0; b.marker = false;
  if (b.end - b.p < 2 || b.p[0] != 0xFF) return false;
  while (b.end - b.p >= 2 && b.p[1] == 0xFF) ++b.p;
  if (b.end - b.p < 2 || b.p[1] != want) return false;
  b.p += 2;
  return true;
}

}  // namespace

extern "C" int cft_jpeg_info(const unsigned char* bytes, long nbytes, cft_jpeg_info_t* info) {
  static_assert(sizeof(cft_jpeg_info_t) == CFT_JPEG_INFO_BYTES, "cft_jpeg_info_t layout");
  if (!bytes || !info || nbytes < 1) return CFT_EINVAL;
  JpgParse P;
  const int st = jpg_parse(bytes, nbytes, P);
  if (st != CFT_OK) return st;
  *info = P.info;
  return CFT_OK;
}

extern "C" int cft_jpeg_entropy(const unsigned char* bytes, long nbytes, short* coef, unsigned short* qtab, const cft_jpeg_info_t* info) {
  if (!bytes || !coef || !qtab || !info || nbytes < 1) return CFT_EINVAL;
  JpgParse P;
  const int st = jpg_parse(bytes, nbytes, P);
  if (st != CFT_OK) return st;
  const cft_jpeg_info_t& I = P.info;
  if (memcmp(&I, info, sizeof I) != 0) return CFT_EINVAL;           // the buffers were sized for another file
  memset(coef, 0, (size_t)I.ncoef * sizeof(short));
  memset(qtab, 0, CFT_JPEG_QTAB_BYTES);
  for (int c = 0; c < I.ncomp; ++c)
    for (int i = 0; i < 64; ++i) qtab[c * 64 + i] = P.q[P.tq[c]][i];
  long base[3];
  jpeg_comp_bases(I, base);
  JpgBits b = {bytes + P.scan, bytes + nbytes, 0, 0, false};
  int pred[3] = {0, 0, 0};
  int left = I.restart_interval, rst = 0;
  for (int my = 0; my < I.mcus_y; ++my) {
    for (int mx = 0; mx < I.mcus_x; ++mx) {
      if (I.restart_interval && left == 0) {
        if (!jpg_take_marker(b, 0xD0 + (rst & 7))) return CFT_JPEG_UNSUPPORTED;
        ++rst; left = I.restart_interval;
        pred[0] = pred[1] = pred[2] = 0;
      }
      for (int c = 0; c < I.ncomp; ++c) {
        const JpgHuff& hd = P.dc[P.td[c]];
        const JpgHuff& ha = P.ac[P.ta[c]];
        const uint16_t* q = P.q[P.tq[c]];
        for (int by = 0; by < I.vs[c]; ++by) {
          for (int bx = 0; bx < I.hs[c]; ++bx) {
            short* blk = jpeg_block_at(coef, I, base, c, my * I.vs[c] + by, mx * I.hs[c] + bx);
            int s = jpg_symbol(b, hd);
            if (s < 0 || s > 11) return CFT_JPEG_UNSUPPORTED;
            if (s) {
              int diff;
              if (!jpg_receive(b, s, diff)) return CFT_JPEG_UNSUPPORTED;
              pred[c] += diff;
            }
            if (!jpg_fits(pred[c], q[0])) return CFT_JPEG_UNSUPPORTED;
            blk[0] = (short)pred[c];
            for (int k = 1; k < 64; ++k) {
              const int rs = jpg_symbol(b, ha);
              if (rs < 0) return CFT_JPEG_UNSUPPORTED;
              const int r = rs >> 4;
              s = rs & 15;
              if (s == 0) {
                if (r != 15) break;                                // end of block
                k += 15;
                continue;
              }
              k += r;
              if (k > 63) return CFT_JPEG_UNSUPPORTED;
              int v;
              if (!jpg_receive(b, s, v)) return CFT_JPEG_UNSUPPORTED;
              const int nat = JPEG_ZIGZAG[k];
              if (!jpg_fits(v, q[nat])) return CFT_JPEG_UNSUPPORTED;
              blk[nat] = (short)v;
            }
          }
        }
      }
      --left;
    }
  }
  if (!jpg_take_marker(b, 0xD9)) return CFT_JPEG_UNSUPPORTED;       // EOI: a second scan, a DNL or a cut file are not in the subset
  return CFT_OK;
}

// ------------------------------------------------------------------------------------------------ device half
// jpeg_idct_islow's one-dimensional butterfly on v[0..7], in place, results descaled by `shift`.  Even part, odd part, recombination:
// the published order of operations.  In the first pass tmp0 / tmp1 carry CONST_BITS, as every product does.
__device__ __forceinline__ void jpg_idct_1d(int v[8], const int shift) {
  int z1 = (v[2] + v[6]) * FIX_0_541196100;
  const int e2 = z1 + v[6] * -FIX_1_847759065;
  const int e3 = z1 + v[2] * FIX_0_765366865;
  const int e0 = (v[0] + v[4]) << 13;
  const int e1 = (v[0] - v[4]) << 13;
  const int t10 = e0 + e3, t13 = e0 - e3, t11 = e1 + e2, t12 = e1 - e2;
  int t0 = v[7], t1 = v[5], t2 = v[3], t3 = v[1];
  z1 = t0 + t3;
  int z2 = t1 + t2, z3 = t0 + t2, z4 = t1 + t3;
  const int z5 = (z3 + z4) * FIX_1_175875602;
  t0 *= FIX_0_298631336; t1 *= FIX_2_053119869; t2 *= FIX_3_072711026; t3 *= FIX_1_501321110;
  z1 *= -FIX_0_899976223; z2 *= -FIX_2_562915447; z3 *= -FIX_1_961570560; z4 *= -FIX_0_390180644;
  z3 += z5; z4 += z5;
  t0 += z1 + z3; t1 += z2 + z4; t2 += z2 + z3; t3 += z1 + z4;
  const int r = 1 << (shift - 1);
  v[0] = (t10 + t3 + r) >> shift; v[7] = (t10 - t3 + r) >> shift;
  v[1] = (t11 + t2 + r) >> shift; v[6] = (t11 - t2 + r) >> shift;
  v[2] = (t12 + t1 + r) >> shift; v[5] = (t12 - t1 + r) >> shift;
  v[3] = (t13 + t0 + r) >> shift; v[4] = (t13 - t0 + r) >> shift;
}

__device__ __forceinline__ int jpg_clampi(int v, int lo, int hi) { return v < lo ? lo : (v > hi ? hi : v); }

__global__ void __launch_bounds__(JPEG_THREADS) jpeg_idct_kernel(const cft_jpeg_desc_t* __restrict__ table, unsigned char* __restrict__ ws) {
  __shared__ __attribute__((aligned(16))) int tile[JPEG_WG_BLOCKS * JPEG_LDS_STRIDE];
  const cft_jpeg_desc_t& d = table[blockIdx.y];                    // uniform over the workgroup
  const JpegBlock b = jpeg_locate(d);
  const int c = b.c, local = b.local, lane = b.lane;
  const long blk = b.blk, rel = b.rel, before = b.before;
  const bool active = b.active;
  int v[8];
  int* t = tile + local * JPEG_LDS_STRIDE;
  if (active) {
    const short* src = d.coef + blk * 64 + lane;
    const unsigned short* q = d.qtab + c * 64 + lane;
#pragma unroll
    for (int r = 0; r < 8; ++r) v[r] = (int)src[r * 8] * (int)q[r * 8];
    jpg_idct_1d(v, 11);                                            // column `lane`
#pragma unroll
    for (int r = 0; r < 8; ++r) t[r * 8 + lane] = v[r];
  }
  __syncthreads();
  if (!active) return;
#pragma unroll
  for (int j = 0; j < 8; ++j) v[j] = t[lane * 8 + j];
  jpg_idct_1d(v, 18);                                              // row `lane`
  uint2 out;
  out.x = (unsigned)jpeg_u8(v[0] + 128) | ((unsigned)jpeg_u8(v[1] + 128) << 8) | ((unsigned)jpeg_u8(v[2] + 128) << 16) | ((unsigned)jpeg_u8(v[3] + 128) << 24);
  out.y = (unsigned)jpeg_u8(v[4] + 128) | ((unsigned)jpeg_u8(v[5] + 128) << 8) | ((unsigned)jpeg_u8(v[6] + 128) << 16) | ((unsigned)jpeg_u8(v[7] + 128) << 24);
  const int bw = d.bw[c];
  const long by = rel / bw, bx = rel % bw;
  unsigned char* dst = ws + d.plane_off + 64 * before + (by * 8 + lane) * (8L * bw) + bx * 8;
  *reinterpret_cast<uint2*>(dst) = out;
}

__global__ void __launch_bounds__(JPEG_THREADS) jpeg_colour_kernel(const cft_jpeg_desc_t* __restrict__ table, const unsigned char* __restrict__ ws) {
  const cft_jpeg_desc_t& d = table[blockIdx.y];
  const int W = d.width, H = d.height;
  const int gpr = (W + 3) >> 2;                                    // 4-pixel groups per row
  const long g = (long)blockIdx.x * JPEG_THREADS + threadIdx.x;
  if (g >= (long)gpr * H) return;
  const int y = (int)(g / gpr), x0 = (int)(g % gpr) * 4;
  const unsigned char* p0 = ws + d.plane_off;
  const unsigned int yw = *reinterpret_cast<const unsigned int*>(p0 + (long)y * (8L * d.bw[0]) + x0);   // inside the padded plane
  int cb[4], cr[4];
  if (d.ncomp == 3) {
    const unsigned char* pc[2];
    pc[0] = p0 + 64L * d.bw[0] * d.bh[0];
    pc[1] = pc[0] + 64L * d.bw[1] * d.bh[1];
    const long s1 = 8L * d.bw[1];
    const int cw = (W + d.hmax - 1) / d.hmax, ch = (H + d.vmax - 1) / d.vmax;
#pragma unroll
    for (int k = 0; k < 2; ++k) {
      int* o = k ? cr : cb;
      if (d.hmax == 1) {
        const unsigned int w = *reinterpret_cast<const unsigned int*>(pc[k] + (long)y * s1 + x0);
#pragma unroll
        for (int j = 0; j < 4; ++j) o[j] = (int)((w >> (8 * j)) & 255u);
      } else {
        const int i0 = x0 >> 1;
        const int ix[4] = {jpg_clampi(i0 - 1, 0, cw - 1), jpg_clampi(i0, 0, cw - 1), jpg_clampi(i0 + 1, 0, cw - 1), jpg_clampi(i0 + 2, 0, cw - 1)};
        if (d.vmax == 1) {
          const unsigned char* row = pc[k] + (long)jpg_clampi(y, 0, ch - 1) * s1;
          const int a = row[ix[0]], b = row[ix[1]], c = row[ix[2]], e = row[ix[3]];
          o[0] = (3 * b + a + 1) >> 2; o[1] = (3 * b + c + 2) >> 2;
          o[2] = (3 * c + b + 1) >> 2; o[3] = (3 * c + e + 2) >> 2;
        } else {
          const int cy = jpg_clampi(y >> 1, 0, ch - 1), ny = jpg_clampi((y & 1) ? cy + 1 : cy - 1, 0, ch - 1);
          const unsigned char* row = pc[k] + (long)cy * s1;
          const unsigned char* nbr = pc[k] + (long)ny * s1;
          int s[4];
#pragma unroll
          for (int j = 0; j < 4; ++j) s[j] = 3 * row[ix[j]] + nbr[ix[j]];
          o[0] = (3 * s[1] + s[0] + 8) >> 4; o[1] = (3 * s[1] + s[2] + 7) >> 4;
          o[2] = (3 * s[2] + s[1] + 8) >> 4; o[3] = (3 * s[2] + s[3] + 7) >> 4;
        }
      }
    }
  }
  unsigned int o[3] = {0u, 0u, 0u};                                // the 12 bytes r g b r g b ... of the four pixels
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    const int Y = (int)((yw >> (8 * j)) & 255u);
    int rgb[3] = {Y, Y, Y};
    if (d.ncomp == 3) {
      const int u = cb[j] - 128, w = cr[j] - 128;
      rgb[0] = jpeg_u8(Y + ((91881 * w + 32768) >> 16));
      rgb[1] = jpeg_u8(Y + ((-22554 * u - 46802 * w + 32768) >> 16));
      rgb[2] = jpeg_u8(Y + ((116130 * u + 32768) >> 16));
    }
#pragma unroll
    for (int k = 0; k < 3; ++k) o[(3 * j + k) >> 2] |= (unsigned)rgb[k] << (8 * ((3 * j + k) & 3));
  }
  unsigned char* dst = d.dst + (long)y * d.dst_stride + 3L * x0;
  if (x0 + 4 <= W && ((uintptr_t)dst & 3) == 0) {
    unsigned int* q = reinterpret_cast<unsigned int*>(dst);
    q[0] = o[0]; q[1] = o[1]; q[2] = o[2];
  } else {
    const int n = 3 * min(4, W - x0);
#pragma unroll
    for (int j = 0; j < 12; ++j)
      if (j < n) dst[j] = (unsigned char)(o[j >> 2] >> (8 * (j & 3)));
  }
}

extern "C" int cft_jpeg_decode_u8(const void* table_dev, const void* table_host, int n, void* workspace, long workspace_bytes, void* stream) {
  static_assert(sizeof(cft_jpeg_desc_t) == CFT_JPEG_DESC_BYTES, "cft_jpeg_desc_t layout");
  CFT_REQUIRE(table_dev && table_host && workspace, "cft_jpeg_decode_u8: null pointer");
  CFT_REQUIRE(((uintptr_t)table_dev & 7) == 0 && ((uintptr_t)table_host & 7) == 0 && ((uintptr_t)workspace & 15) == 0, "cft_jpeg_decode_u8: misaligned table or workspace");
  CFT_REQUIRE(n > 0 && n <= 65535, "cft_jpeg_decode_u8: image count out of range (1..65535)");
  CFT_REQUIRE(workspace_bytes > 0, "cft_jpeg_decode_u8: empty workspace");
  const cft_jpeg_desc_t* rows = static_cast<const cft_jpeg_desc_t*>(table_host);
  long max_blocks = 0, max_groups = 0, prev_end = 0;
  for (int i = 0; i < n; ++i) {
    const cft_jpeg_desc_t& d = rows[i];
    CFT_REQUIRE(d.coef && d.qtab && d.dst, "cft_jpeg_decode_u8: null pointer in the table");
    CFT_REQUIRE(((uintptr_t)d.coef & 1) == 0 && ((uintptr_t)d.qtab & 1) == 0, "cft_jpeg_decode_u8: misaligned coefficients or tables");
    long blocks;
    JPEG_REQUIRE_GEOMETRY("cft_jpeg_decode_u8", d, blocks);
    CFT_REQUIRE(d.dst_stride >= 3L * d.width, "cft_jpeg_decode_u8: bad destination row stride");
    CFT_REQUIRE(d.plane_off >= 0 && (d.plane_off & 15) == 0, "cft_jpeg_decode_u8: plane offset negative or not a multiple of 16");
    CFT_REQUIRE(d.plane_off >= prev_end, "cft_jpeg_decode_u8: plane ranges overlap or do not ascend");
    CFT_REQUIRE(d.plane_off <= workspace_bytes && 64 * blocks <= workspace_bytes - d.plane_off, "cft_jpeg_decode_u8: planes outside the workspace");
    prev_end = d.plane_off + 64 * blocks;
    const long groups = (long)((d.width + 3) / 4) * d.height;
    max_blocks = blocks > max_blocks ? blocks : max_blocks;
    max_groups = groups > max_groups ? groups : max_groups;
  }
  const cft_jpeg_desc_t* dev = static_cast<const cft_jpeg_desc_t*>(table_dev);
  hipLaunchKernelGGL(jpeg_idct_kernel, dim3((unsigned)((max_blocks + JPEG_WG_BLOCKS - 1) / JPEG_WG_BLOCKS), n), dim3(JPEG_THREADS), 0, as_stream(stream),
                     dev, static_cast<unsigned char*>(workspace));
  int st = cft_check_launch("jpeg_idct_kernel");
  if (st != CFT_OK) return st;
  hipLaunchKernelGGL(jpeg_colour_kernel, dim3((unsigned)((max_groups + JPEG_THREADS - 1) / JPEG_THREADS), n), dim3(JPEG_THREADS), 0, as_stream(stream),
                     dev, static_cast<const unsigned char*>(workspace));
  return cft_check_launch("jpeg_colour_kernel");
}
