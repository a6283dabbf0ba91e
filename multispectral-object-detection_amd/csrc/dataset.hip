// Batch assembly for the non-augmented RGB + IR dataloader: ONE launch writes the uint8 [B, 6, H, W] batch (cft_pair_batch_u8,
// include/cft_hip.h) from a device-resident table with one row per image pair.  Per pair: the resize of load_image_rgb_ir
// (reference utils/datasets.py:1361-1367; copy / cv2 INTER_LINEAR / cv2 INTER_AREA), the grey letterbox border (:1205-1207) and
// HWC -> CHW with the stream packing of :1274-1279.
//
// Launch shape: the grid is (tiles, B); one 256-thread workgroup owns one TH x TW tile of the letterbox of one pair (TH * TW = 1024,
// TW <= 256 picked per launch so that the source span of a tile fits the LDS budget).  The workgroup first copies the source span
// of its tile into LDS, row by row with dword loads (byte loads only for the unaligned head and tail of a row: the source stride
// need not be a multiple of 4), then every thread produces 4 consecutive pixels of one row for the three channels and writes one
// dword per plane, so a row of a tile is a contiguous run of TW bytes in each of the three planes.  The byte traffic is what bounds
// it: every source byte is read from HBM once per tile that needs it, every destination byte is written once.
//
// The INTER_AREA arithmetic restates OpenCV's published path (modules/imgproc/src/resize.cpp: computeResizeAreaTab, ResizeArea_,
// ResizeAreaFast_); the float64 numpy restatement it is tested against is tests/dataset_ref.py.  cv2 itself is "parity unpinned",
// as for INTER_LINEAR (pointwise.hip).
#include "cft_common.h"
#include "resize_common.h"

#define PAIR_THREADS 256
#define PAIR_TILE_PIXELS 1024          // TH * TW
#define PAIR_LDS_BUDGET (64 * 1024)    // bytes of source span per workgroup: two workgroups per CU at the worst, a 4 x 256 tile reduced 4x
// CFT_PAIR_MAX_REDUCTION (cft_hip.h): INTER_AREA source pixels per output pixel and axis; what a tile's span in LDS admits, and it bounds the fp32 error (see below)

// AreaTab / area_tab / area_weight (one axis of computeResizeAreaTab) are in resize_common.h, shared with cft_mosaic_area.

// The source span [s0, s1) that the output range [r0, r1) of one axis reads.
__device__ __forceinline__ void source_span(int mode, int r0, int r1, int ssize, int dsize, bool rows, int& s0, int& s1) {
  if (mode == CFT_PAIR_COPY) { s0 = r0; s1 = r1; return; }
  if (mode == CFT_PAIR_AREA) {
    s0 = (int)((long)r0 * ssize / dsize);
    const long e = ((long)r1 * ssize + dsize - 1) / dsize;
    s1 = e < ssize ? (int)e : ssize;
    return;
  }
  const double scale = cft_linear_scale(dsize, ssize);
  const CftLinearTap a = rows ? cft_linear_tap_y(r0, scale, ssize) : cft_linear_tap_x(r0, scale, ssize);
  const CftLinearTap b = rows ? cft_linear_tap_y(r1 - 1, scale, ssize) : cft_linear_tap_x(r1 - 1, scale, ssize);
  s0 = a.s0; s1 = b.s1 + 1;
}

__global__ void __launch_bounds__(PAIR_THREADS) pair_batch_u8_kernel(const cft_pair_desc_t* __restrict__ desc, unsigned char* __restrict__ dst,
                                                                     int H, int W, int TH, int TW, int tiles_x, int color, int lds_bytes) {
  extern __shared__ unsigned int lds_w[];
  const unsigned char* lds = reinterpret_cast<const unsigned char*>(lds_w);
  const cft_pair_desc_t d = desc[blockIdx.y];                  // uniform over the workgroup
  const int oy0 = (blockIdx.x / tiles_x) * TH, ox0 = (blockIdx.x % tiles_x) * TW;
  const int gpr = TW >> 2;                                     // 4-pixel groups per tile row; TH * gpr == PAIR_THREADS
  const int oy = oy0 + (int)threadIdx.x / gpr, ox = ox0 + ((int)threadIdx.x % gpr) * 4;

  // the part of the tile that the resized image covers, in resized-image coordinates
  int ry0 = oy0 - d.top, ry1 = (oy0 + TH < H ? oy0 + TH : H) - d.top;
  int rx0 = ox0 - d.left, rx1 = (ox0 + TW < W ? ox0 + TW : W) - d.left;
  ry0 = ry0 > 0 ? ry0 : 0; ry1 = ry1 < d.h ? ry1 : d.h;
  rx0 = rx0 > 0 ? rx0 : 0; rx1 = rx1 < d.w ? rx1 : d.w;
  const bool covered = ry0 < ry1 && rx0 < rx1;

  int ys0 = 0, ys1 = 0, xs0 = 0, xs1 = 0;
  if (covered) {
    source_span(d.mode, ry0, ry1, d.h0, d.h, true, ys0, ys1);
    source_span(d.mode, rx0, rx1, d.w0, d.w, false, xs0, xs1);
  }
  const int nbytes = (xs1 - xs0) * 3;                          // source bytes per staged row
  const int pdw = (nbytes + 3 + 3) >> 2;                       // LDS row pitch in dwords: the row plus up to 3 bytes of misalignment
  int nrows = ys1 - ys0;
  if ((long)nrows * pdw * 4 > lds_bytes) nrows = pdw > 0 ? lds_bytes / (pdw * 4) : 0;      // never: the launcher sizes lds_bytes for the widest span
  const int ncols = xs1 - xs0;
  const bool int_area = d.mode == CFT_PAIR_AREA && d.w0 % d.w == 0 && d.h0 % d.h == 0;
  const bool inside_row = oy < H && oy - d.top >= 0 && oy - d.top < d.h;

  // the tables of this thread's row and of its 4 columns: the same for both streams, built once
  const int ry = oy - d.top;
  const bool frac_area = d.mode == CFT_PAIR_AREA && !int_area;
  AreaTab taby = {}, tabx[4] = {};
  CftLinearTap lty = {};
  if (inside_row && covered && ox < W) {
    if (d.mode == CFT_PAIR_LINEAR) lty = cft_linear_tap_y(ry, cft_linear_scale(d.h, d.h0), d.h0);
    if (frac_area) {
      taby = area_tab(ry, d.h0, d.h);
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const int rx = ox + j - d.left;
        if (rx >= 0 && rx < d.w) tabx[j] = area_tab(rx, d.w0, d.w);
      }
    }
  }

  for (int s = 0; s < 2; ++s) {
    const unsigned char* src = s ? d.src_ir : d.src_rgb;
    const long stride = s ? d.stride_ir : d.stride_rgb;
    if (s) __syncthreads();                                    // the first stream's span has been consumed
    for (int i = threadIdx.x; i < nrows * pdw; i += PAIR_THREADS) {
      const int r = i / pdw, k = i - r * pdw;
      const unsigned char* lo = src + (long)(ys0 + r) * stride + (long)xs0 * 3;
      const unsigned char* hi = lo + nbytes;
      const unsigned char* a = lo - ((uintptr_t)lo & 3) + 4L * k;        // aligned dword k of the row
      unsigned int v = 0;
      if (a >= lo && a + 4 <= hi) {
        v = *reinterpret_cast<const unsigned int*>(a);
      } else {
#pragma unroll
        for (int b = 0; b < 4; ++b)
          if (a + b >= lo && a + b < hi) v |= (unsigned int)a[b] << (8 * b);
      }
      lds_w[i] = v;
    }
    __syncthreads();
    if (oy >= H || ox >= W) continue;                          // (W % 4 == 0: a group is inside or outside as a whole)

    // LDS byte of source pixel (y, x), channel c; indices are clamped to the staged span
    auto row_base = [&](int y) {
      int r = y - ys0;
      r = r < 0 ? 0 : (r > nrows - 1 ? nrows - 1 : r);
      const unsigned int mis = (unsigned int)((uintptr_t)(src + (long)(ys0 + r) * stride + (long)xs0 * 3) & 3);
      return r * pdw * 4 + (int)mis;
    };
    auto col_off = [&](int x) {
      int c = x - xs0;
      c = c < 0 ? 0 : (c > ncols - 1 ? ncols - 1 : c);
      return c * 3;
    };

    unsigned int out[3] = {0u, 0u, 0u};
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const int rx = ox + j - d.left;
      int v[3] = {color, color, color};
      if (inside_row && covered && nrows > 0 && rx >= 0 && rx < d.w) {
        if (d.mode == CFT_PAIR_COPY) {
          const int o = row_base(ry) + col_off(rx);
          v[0] = lds[o]; v[1] = lds[o + 1]; v[2] = lds[o + 2];
        } else if (d.mode == CFT_PAIR_LINEAR) {
          const CftLinearTap tx = cft_linear_tap_x(rx, cft_linear_scale(d.w, d.w0), d.w0);
          const int b0 = row_base(lty.s0), b1 = row_base(lty.s1), c0 = col_off(tx.s0), c1 = col_off(tx.s1);
#pragma unroll
          for (int c = 0; c < 3; ++c)
            v[c] = cft_linear_blend(lds[b0 + c0 + c], lds[b0 + c1 + c], lds[b1 + c0 + c], lds[b1 + c1 + c], tx, lty);
        } else if (int_area) {
          const int ix = d.w0 / d.w, iy = d.h0 / d.h;
          int sum[3] = {0, 0, 0};
          for (int yy = 0; yy < iy; ++yy) {
            const int b = row_base(ry * iy + yy);
            for (int xx = 0; xx < ix; ++xx) {
              const int o = b + col_off(rx * ix + xx);
              sum[0] += lds[o]; sum[1] += lds[o + 1]; sum[2] += lds[o + 2];
            }
          }
          const int n = ix * iy;
#pragma unroll
          for (int c = 0; c < 3; ++c) v[c] = (2 * sum[c] + n) / (2 * n);       // the exact mean, halves rounded up
        } else {
          // fp32, fixed order: the weighted columns of one source row, then that row into the pixel.  A product or a partial sum is
          // <= 255, so each rounding is off by <= 2^-17; a row sum takes <= 2 (CFT_PAIR_MAX_REDUCTION + 2) of them, the weighted rows (weights
          // summing to 1) pass that on once and add as many of their own: <= 24 * 2^-17 = 0.19 * 2^-10 from the real-number value, inside
          // the 2^-10 band around a tie in which alone a pixel may round the other way.
          const AreaTab& tx = tabx[j];
          float acc[3] = {0.f, 0.f, 0.f};
          for (int yy = 0; yy < taby.n; ++yy) {
            const int b = row_base(taby.c0 + yy);
            float hs[3] = {0.f, 0.f, 0.f};
            for (int xx = 0; xx < tx.n; ++xx) {
              const int o = b + col_off(tx.c0 + xx);
              const float wx = area_weight(tx, xx);
              hs[0] += wx * (float)lds[o]; hs[1] += wx * (float)lds[o + 1]; hs[2] += wx * (float)lds[o + 2];
            }
            const float wy = area_weight(taby, yy);
            acc[0] += wy * hs[0]; acc[1] += wy * hs[1]; acc[2] += wy * hs[2];
          }
#pragma unroll
          for (int c = 0; c < 3; ++c) {
            const int q = cft_cv_round(acc[c]);
            v[c] = q < 0 ? 0 : (q > 255 ? 255 : q);
          }
        }
      }
#pragma unroll
      for (int c = 0; c < 3; ++c) out[c] |= (unsigned int)v[c] << (8 * j);
    }
    unsigned char* base = dst + (((long)blockIdx.y * 6 + s * 3) * H + oy) * (long)W + ox;
#pragma unroll
    for (int c = 0; c < 3; ++c)
      *reinterpret_cast<unsigned int*>(base + (long)(d.flip ? 2 - c : c) * H * W) = out[c];
  }
}

// Upper bound of the LDS bytes that one TH x TW tile of this pair stages (the kernel's source_span, bounded per axis).
static long pair_span_bytes(const cft_pair_desc_t& d, int TH, int TW) {
  long rows, cols;
  if (d.mode == CFT_PAIR_AREA) {
    rows = ((long)TH * d.h0 + d.h - 1) / d.h + 2;
    cols = ((long)TW * d.w0 + d.w - 1) / d.w + 2;
  } else {                                      // copy, or an enlargement: at most one source pixel per output pixel, plus the second tap
    rows = TH + 2;
    cols = TW + 2;
  }
  rows = rows < d.h0 ? rows : d.h0;
  cols = cols < d.w0 ? cols : d.w0;
  return rows * (((cols * 3 + 3 + 3) >> 2) * 4);
}

extern "C" int cft_pair_batch_u8(const void* desc_dev, const void* desc_host, int B, unsigned char* dst, int dst_h, int dst_w, int color, void* stream) {
  static_assert(sizeof(cft_pair_desc_t) == CFT_PAIR_DESC_BYTES, "cft_pair_desc_t layout");
  CFT_REQUIRE(desc_dev && desc_host && dst, "cft_pair_batch_u8: null pointer");
  CFT_REQUIRE(B > 0 && B <= 65535, "cft_pair_batch_u8: batch size out of range (1..65535)");
  CFT_REQUIRE(dst_h > 0 && dst_w > 0 && dst_w % 4 == 0 && ((uintptr_t)dst & 3) == 0, "cft_pair_batch_u8: dst and dst_w must be multiples of 4");
  CFT_REQUIRE((long)dst_h * dst_w < (1L << 31) / 8, "cft_pair_batch_u8: letterbox too large");
  CFT_REQUIRE(color >= 0 && color <= 255, "cft_pair_batch_u8: border value out of range");
  const cft_pair_desc_t* rows = static_cast<const cft_pair_desc_t*>(desc_host);
  for (int b = 0; b < B; ++b) {
    const cft_pair_desc_t& d = rows[b];
    CFT_REQUIRE(d.src_rgb && d.src_ir, "cft_pair_batch_u8: null source pointer in the table");
    CFT_REQUIRE(d.h0 > 0 && d.w0 > 0 && d.h > 0 && d.w > 0 && d.w0 <= (1 << 24) && d.h0 <= (1 << 24), "cft_pair_batch_u8: bad image size in the table");
    CFT_REQUIRE(d.stride_rgb >= 3L * d.w0 && d.stride_ir >= 3L * d.w0, "cft_pair_batch_u8: bad source row stride");
    CFT_REQUIRE(d.top >= 0 && d.left >= 0 && (long)d.top + d.h <= dst_h && (long)d.left + d.w <= dst_w, "cft_pair_batch_u8: a resized image does not fit the letterbox");
    CFT_REQUIRE(d.flip == 0 || d.flip == 1, "cft_pair_batch_u8: bad channel-order flag");
    if (d.mode == CFT_PAIR_COPY) CFT_REQUIRE(d.h == d.h0 && d.w == d.w0, "cft_pair_batch_u8: copy mode with a resized size");
    else if (d.mode == CFT_PAIR_LINEAR) CFT_REQUIRE(d.h >= d.h0 && d.w >= d.w0, "cft_pair_batch_u8: linear mode is the enlarging resize");
    else if (d.mode == CFT_PAIR_AREA)
      CFT_REQUIRE(d.h <= d.h0 && d.w <= d.w0 && (long)d.h * CFT_PAIR_MAX_REDUCTION >= d.h0 && (long)d.w * CFT_PAIR_MAX_REDUCTION >= d.w0,
                  "cft_pair_batch_u8: area mode reduces by 1x to 4x per axis");
    else CFT_REQUIRE(false, "cft_pair_batch_u8: unknown resize mode");
  }
  // the widest tile whose source span fits the LDS budget for every pair
  int TW = 0;
  long lds = 0;
  for (int tw = 256; tw >= 16 && !TW; tw >>= 1) {
    long need = 0;
    for (int b = 0; b < B; ++b) {
      const long n = pair_span_bytes(rows[b], PAIR_TILE_PIXELS / tw, tw);
      need = n > need ? n : need;
    }
    if (need <= PAIR_LDS_BUDGET) { TW = tw; lds = need; }
  }
  CFT_REQUIRE(TW, "cft_pair_batch_u8: no tile shape fits the LDS budget");
  const int TH = PAIR_TILE_PIXELS / TW;
  const int tiles_x = (dst_w + TW - 1) / TW, tiles_y = (dst_h + TH - 1) / TH;
  cft_allow_lds<pair_batch_u8_kernel>(PAIR_LDS_BUDGET);
  hipLaunchKernelGGL(pair_batch_u8_kernel, dim3(tiles_x * tiles_y, B), dim3(PAIR_THREADS), (size_t)lds, as_stream(stream),
                     static_cast<const cft_pair_desc_t*>(desc_dev), dst, dst_h, dst_w, TH, TW, tiles_x, color, (int)lds);
  return cft_check_launch("pair_batch_u8_kernel");
}
