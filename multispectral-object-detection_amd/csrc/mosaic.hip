// plot_images of the reference (utils/plots.py:128-203) on the device (include/cft_hip.h):
//   cft_mosaic_compose  the first bs images of a batch into the ns x ns grid, un-normalised (x 255 when image 0 is <= 1), resized, as uint8;
//   cft_mosaic_slots    the targets of every cell as the slot table cft_detect_render reads (output_to_target fused in for the NMS form);
//   cft_mosaic_finish   file names and cell borders, after the boxes;
//   cft_mosaic_area     the final INTER_AREA reduction, the arithmetic of cft_pair_batch_u8.
// One thread writes one pixel or one slot; the only atomics are integer (the maximum's key, the flag word): every result is the same
// run to run.  cv2's float resize, lines and font are "parity unpinned": the raster is the one defined in the header.
#include "cft_common.h"
#include "resize_common.h"

constexpr int MOSAIC_THREADS = 256;

// ------------------------------------------------------------------------------------------------------------------ area
// Compiled like pair_batch_u8_kernel (dataset.hip), i.e. BEFORE the contract(off) pragma below: the fp32 accumulation is the same
// expression under the same contraction rule, so the two kernels agree bit for bit.  One thread per output pixel, the source read
// from global memory (a mosaic is reduced once per saved file; the pair kernel's LDS staging would buy nothing here).
__global__ void __launch_bounds__(MOSAIC_THREADS) mosaic_area_kernel(const unsigned char* __restrict__ src, long src_stride, int sh, int sw,
                                                                     unsigned char* __restrict__ dst, long dst_stride, int dh, int dw) {
  const long p = (long)blockIdx.x * MOSAIC_THREADS + threadIdx.x;
  if (p >= (long)dh * dw) return;
  const int oy = (int)(p / dw), ox = (int)(p - (long)oy * dw);
  int v[3];
  if (sw % dw == 0 && sh % dh == 0) {
    const int ix = sw / dw, iy = sh / dh;
    int sum[3] = {0, 0, 0};
    for (int yy = 0; yy < iy; ++yy) {
      const unsigned char* row = src + (long)(oy * iy + yy) * src_stride + (long)ox * ix * 3;
      for (int xx = 0; xx < ix; ++xx) {
        sum[0] += row[xx * 3]; sum[1] += row[xx * 3 + 1]; sum[2] += row[xx * 3 + 2];
      }
    }
    const int n = ix * iy;
#pragma unroll
    for (int c = 0; c < 3; ++c) v[c] = (2 * sum[c] + n) / (2 * n);       // the exact mean, halves rounded up
  } else {
    const AreaTab taby = area_tab(oy, sh, dh), tx = area_tab(ox, sw, dw);
    float acc[3] = {0.f, 0.f, 0.f};
    for (int yy = 0; yy < taby.n; ++yy) {
      int y = taby.c0 + yy;
      y = y < 0 ? 0 : (y > sh - 1 ? sh - 1 : y);
      const unsigned char* row = src + (long)y * src_stride;
      float hs[3] = {0.f, 0.f, 0.f};
      for (int xx = 0; xx < tx.n; ++xx) {
        int x = tx.c0 + xx;
        x = x < 0 ? 0 : (x > sw - 1 ? sw - 1 : x);
        const unsigned char* o = row + (long)x * 3;
        const float wx = area_weight(tx, xx);
        hs[0] += wx * (float)o[0]; hs[1] += wx * (float)o[1]; hs[2] += wx * (float)o[2];
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
  unsigned char* o = dst + (long)oy * dst_stride + (long)ox * 3;
  o[0] = (unsigned char)v[0]; o[1] = (unsigned char)v[1]; o[2] = (unsigned char)v[2];
}

extern "C" int cft_mosaic_area(const unsigned char* src, long src_stride, int sh, int sw, unsigned char* dst, long dst_stride, int dh, int dw,
                               void* stream) {
  CFT_REQUIRE(src && dst, "cft_mosaic_area: null pointer");
  CFT_REQUIRE(sh > 0 && sw > 0 && dh > 0 && dw > 0 && sh <= (1 << 24) && sw <= (1 << 24), "cft_mosaic_area: bad size");
  CFT_REQUIRE(dh <= sh && dw <= sw, "cft_mosaic_area: the area resize only reduces");
  CFT_REQUIRE((long)dh * CFT_PAIR_MAX_REDUCTION >= sh && (long)dw * CFT_PAIR_MAX_REDUCTION >= sw, "cft_mosaic_area: reduces by 1x to 4x per axis");
  CFT_REQUIRE(src_stride >= 3L * sw && dst_stride >= 3L * dw && src_stride <= (1L << 40) && dst_stride <= (1L << 40), "cft_mosaic_area: bad row stride");
  CFT_REQUIRE((long)dh * dw < (1L << 31), "cft_mosaic_area: image too large");
  const unsigned char *s0 = src, *s1 = src + (sh - 1) * src_stride + 3L * sw, *d0 = dst, *d1 = dst + (dh - 1) * dst_stride + 3L * dw;
  CFT_REQUIRE(s1 <= d0 || d1 <= s0, "cft_mosaic_area: src and dst overlap");
  const long n = (long)dh * dw;
  hipLaunchKernelGGL(mosaic_area_kernel, dim3((unsigned)((n + MOSAIC_THREADS - 1) / MOSAIC_THREADS)), dim3(MOSAIC_THREADS), 0, as_stream(stream), src,
                     src_stride, sh, sw, dst, dst_stride, dh, dw);
  return cft_check_launch("mosaic_area_kernel");
}

#include "metrics_common.h"      // block_excl_scan, MATCH_THREADS

#pragma clang fp contract(off)   // from here on float arithmetic restates numpy's: separate roundings, no fused multiply-adds

static_assert(MATCH_THREADS == MOSAIC_THREADS, "the slot kernel uses the 256-thread block scan");
constexpr int BOX_WORDS = 16;
constexpr int MOSAIC_MAX_SIDE = 1 << 15;          // cell and mosaic sides; keeps every pixel index an int

// ------------------------------------------------------------------------------------------------------------------ compose
// A key that orders like the float it encodes (a NaN is the largest), for atomicMax on unsigned.
__device__ __forceinline__ unsigned int float_key(float v) {
  if (!(v == v)) return 0xffffffffu;
  const unsigned int u = __float_as_uint(v);
  return (u >> 31) ? ~u : (u | 0x80000000u);
}
constexpr unsigned int KEY_ONE = 0x3f800000u | 0x80000000u;      // float_key(1.0f)

__device__ __forceinline__ float load_elem(const void* p, int dtype, long i) {
  if (dtype == CFT_MOSAIC_U8) return (float)static_cast<const unsigned char*>(p)[i];
  if (dtype == CFT_MOSAIC_F16) return (float)static_cast<const f16_t*>(p)[i];
  return static_cast<const float*>(p)[i];
}

// np.max(images[0]) (utils/plots.py:137): all C channels of image 0, as an ordered key
__global__ void __launch_bounds__(MOSAIC_THREADS) mosaic_max_kernel(const void* __restrict__ img, int dtype, int C, int H, int W, long sc, long sh,
                                                                    long sw, unsigned int* __restrict__ key) {
  __shared__ unsigned int s_k[MOSAIC_THREADS];
  const long n = (long)C * H * W;
  unsigned int k = 0;
  for (long e = (long)blockIdx.x * MOSAIC_THREADS + threadIdx.x; e < n; e += (long)gridDim.x * MOSAIC_THREADS) {
    const int c = (int)(e / ((long)H * W));
    const long r = e - (long)c * H * W;
    const int y = (int)(r / W), x = (int)(r - (long)y * W);
    const unsigned int q = float_key(load_elem(img, dtype, c * sc + y * sh + x * sw));
    k = q > k ? q : k;
  }
  s_k[threadIdx.x] = k;
  __syncthreads();
  for (int o = MOSAIC_THREADS / 2; o > 0; o >>= 1) {
    if ((int)threadIdx.x < o) s_k[threadIdx.x] = s_k[threadIdx.x] > s_k[threadIdx.x + o] ? s_k[threadIdx.x] : s_k[threadIdx.x + o];
    __syncthreads();
  }
  if (threadIdx.x == 0) atomicMax(key, s_k[0]);
}

struct FloatTap { int s0, s1; float a0, a1; };

// OpenCV's float convention for one axis of the bilinear resize (header): indices clamped, the fraction kept
__device__ __forceinline__ FloatTap float_tap(int d, double scale, int ssize) {
  const float f = (float)(((double)d + 0.5) * scale - 0.5);
  const int s = (int)floorf(f);
  FloatTap t;
  t.a1 = f - (float)s;
  t.a0 = 1.f - t.a1;
  t.s0 = s < 0 ? 0 : (s > ssize - 1 ? ssize - 1 : s);
  t.s1 = s + 1 < 0 ? 0 : (s + 1 > ssize - 1 ? ssize - 1 : s + 1);
  return t;
}

__device__ __forceinline__ unsigned char to_u8(float v) {       // clamp to [0, 255], truncate toward zero; a NaN gives 0
  if (!(v > 0.f)) return 0;
  return v >= 255.f ? 255 : (unsigned char)(int)v;
}

struct ComposeArgs {
  const void* img;
  unsigned char* mosaic;
  const unsigned int* key;
  long sb, sc, sh, sw, mstride;
  int dtype, H, W, c0, bs, ns, h, w, resize;
};

__global__ void __launch_bounds__(MOSAIC_THREADS) mosaic_compose_kernel(ComposeArgs a) {
  const int MW = a.ns * a.w, MH = a.ns * a.h;
  const long p = (long)blockIdx.x * MOSAIC_THREADS + threadIdx.x;
  if (p >= (long)MH * MW) return;
  const int y = (int)(p / MW), x = (int)(p - (long)y * MW);
  unsigned char* o = a.mosaic + (long)y * a.mstride + (long)x * 3;
  const int cx = x / a.w, cy = y / a.h, i = cx * a.ns + cy;       // column-major cells
  if (i >= a.bs) {
    o[0] = 255; o[1] = 255; o[2] = 255;
    return;
  }
  const float factor = *a.key <= KEY_ONE ? 255.f : 1.f;
  const int lx = x - cx * a.w, ly = y - cy * a.h;
  const long base = (long)i * a.sb + (long)a.c0 * a.sc;
  if (!a.resize) {
#pragma unroll
    for (int c = 0; c < 3; ++c) o[c] = to_u8(load_elem(a.img, a.dtype, base + c * a.sc + ly * a.sh + lx * a.sw) * factor);
    return;
  }
  const FloatTap tx = float_tap(lx, cft_linear_scale(a.w, a.W), a.W), ty = float_tap(ly, cft_linear_scale(a.h, a.H), a.H);
#pragma unroll
  for (int c = 0; c < 3; ++c) {
    const long b0 = base + c * a.sc + ty.s0 * a.sh, b1 = base + c * a.sc + ty.s1 * a.sh;
    const float p00 = load_elem(a.img, a.dtype, b0 + tx.s0 * a.sw) * factor, p01 = load_elem(a.img, a.dtype, b0 + tx.s1 * a.sw) * factor;
    const float p10 = load_elem(a.img, a.dtype, b1 + tx.s0 * a.sw) * factor, p11 = load_elem(a.img, a.dtype, b1 + tx.s1 * a.sw) * factor;
    const float r0 = tx.a0 * p00 + tx.a1 * p01;
    const float r1 = tx.a0 * p10 + tx.a1 * p11;
    o[c] = to_u8(ty.a0 * r0 + ty.a1 * r1);
  }
}

extern "C" int cft_mosaic_compose(const void* img, int dtype, int B, int C, int H, int W, long sb, long sc, long sh, long sw, int c0, int bs, int ns,
                                  int h, int w, int resize, unsigned char* mosaic, long mstride, int* maxkey, void* stream) {
  CFT_REQUIRE(img && mosaic && maxkey, "cft_mosaic_compose: null pointer");
  CFT_REQUIRE(dtype == CFT_MOSAIC_U8 || dtype == CFT_MOSAIC_F16 || dtype == CFT_MOSAIC_F32, "cft_mosaic_compose: dtype must be uint8, fp16 or fp32");
  CFT_REQUIRE(B > 0 && C >= 3 && C <= 65535 && H > 0 && W > 0 && H <= MOSAIC_MAX_SIDE && W <= MOSAIC_MAX_SIDE, "cft_mosaic_compose: bad batch shape");
  CFT_REQUIRE(c0 >= 0 && c0 + 3 <= C, "cft_mosaic_compose: channels [c0, c0 + 3) are outside the batch");
  CFT_REQUIRE(bs > 0 && bs <= B && ns > 0 && ns <= 256 && (long)ns * ns >= bs && (long)(ns - 1) * (ns - 1) < bs, "cft_mosaic_compose: ns must be ceil(sqrt(bs)), bs in [1, B]");
  CFT_REQUIRE(h > 0 && w > 0 && h <= H && w <= W, "cft_mosaic_compose: the cell is larger than the image");
  CFT_REQUIRE(resize ? true : (h == H && w == W), "cft_mosaic_compose: without a resize the cell is the image");
  CFT_REQUIRE((long)ns * h <= MOSAIC_MAX_SIDE && (long)ns * w <= MOSAIC_MAX_SIDE, "cft_mosaic_compose: mosaic too large");
  CFT_REQUIRE(mstride >= 3L * ns * w && mstride <= (1L << 40), "cft_mosaic_compose: bad mosaic row stride");
  CFT_REQUIRE(((size_t)maxkey & 3) == 0, "cft_mosaic_compose: maxkey must be 4-byte aligned");
  const long lim = 1L << 40;
  CFT_REQUIRE(sb >= 0 && sc >= 0 && sh >= 0 && sw >= 0 && sb < lim && sc < lim && sh < lim && sw < lim, "cft_mosaic_compose: strides must be in [0, 2^40)");
  CFT_REQUIRE((B - 1) * sb + (C - 1) * sc + (H - 1) * sh + (W - 1) * sw < (1L << 46), "cft_mosaic_compose: batch too large");
  hipStream_t st = as_stream(stream);
  if (hipMemsetAsync(maxkey, 0, 4, st) != hipSuccess) {
    cft_set_error("cft_mosaic_compose: hipMemsetAsync failed");
    return CFT_EINVAL;
  }
  const long n0 = (long)C * H * W;
  long blocks = (n0 + MOSAIC_THREADS * 8L - 1) / (MOSAIC_THREADS * 8L);
  blocks = blocks > 1024 ? 1024 : blocks;
  hipLaunchKernelGGL(mosaic_max_kernel, dim3((unsigned)blocks), dim3(MOSAIC_THREADS), 0, st, img, dtype, C, H, W, sc, sh, sw, (unsigned int*)maxkey);
  int rc = cft_check_launch("mosaic_max_kernel");
  if (rc != CFT_OK) return rc;
  ComposeArgs a;
  a.img = img; a.mosaic = mosaic; a.key = (const unsigned int*)maxkey;
  a.sb = sb; a.sc = sc; a.sh = sh; a.sw = sw; a.mstride = mstride;
  a.dtype = dtype; a.H = H; a.W = W; a.c0 = c0; a.bs = bs; a.ns = ns; a.h = h; a.w = w; a.resize = resize;
  const long n = (long)ns * h * ns * w;
  hipLaunchKernelGGL(mosaic_compose_kernel, dim3((unsigned)((n + MOSAIC_THREADS - 1) / MOSAIC_THREADS)), dim3(MOSAIC_THREADS), 0, st, a);
  return cft_check_launch("mosaic_compose_kernel");
}

// ------------------------------------------------------------------------------------------------------------------ slots
// '%.1f' % conf as tenths: round(v * 10) of the double's exact value v = m * 2^-s, ties to even, in integers (10 m < 2^57).
// Saturates at 10; a negative value, zero or a NaN gives 0.
__device__ __forceinline__ int conf_tenths(double conf) {
  unsigned long long u;
  __builtin_memcpy(&u, &conf, 8);
  if (u >> 63) return 0;
  const int ex = (int)(u >> 52);
  const unsigned long long frac = u & ((1ull << 52) - 1ull);
  if (ex == 2047) return frac ? 0 : 10;              // NaN : +inf
  if (ex >= 1023 + 1) return 10;                     // >= 2
  const unsigned long long m = ex ? (frac | (1ull << 52)) : frac;
  const int s = 1075 - (ex ? ex : 1);                // v = m * 2^-s, s in [52, 1074]
  if (s > 62) return 0;                              // v < 2^-9
  const unsigned long long p = m * 10ull, half = 1ull << (s - 1);
  unsigned long long q = p >> s;
  const unsigned long long rem = p & ((1ull << s) - 1ull);
  if (rem > half || (rem == half && (q & 1ull))) ++q;
  return q > 10ull ? 10 : (int)q;
}

template <typename T> struct Target { T cls, x, y, w, h, conf; };

// int() / .astype('int') for the values met here: truncation toward zero; NaN -> 0, saturating far outside any image
template <typename T> __device__ __forceinline__ int trunc_int(T v) {
  if (!(v == v)) return 0;
  return v <= (T)-1073741824 ? -1073741824 : (v >= (T)1073741824 ? 1073741824 : (int)v);
}
template <typename T> __device__ __forceinline__ int trunc_cls(T v) {
  return (v > (T)-1073741824 && v < (T)1073741824) ? (int)v : -1;      // a NaN or a value no class table holds: -1
}

struct SlotArgs {
  const void* rows;
  const float* dets;
  const int* counts;
  int* slots;
  int* flag;
  double sf;
  int nt, cols, max_det, cap, nc, h, w;
};

// Row j of image i.  FORM 0: rows of T; FORM 1: the padded NMS output (T = double), xyxy2xywh in float32 first.
template <typename T, int FORM>
__device__ __forceinline__ bool load_target(const SlotArgs& a, int i, int j, Target<T>& t) {
  if (FORM == 0) {
    const T* r = static_cast<const T*>(a.rows) + (long)j * a.cols;
    if (!(r[0] == (T)i)) return false;
    t.cls = r[1]; t.x = r[2]; t.y = r[3]; t.w = r[4]; t.h = r[5];
    t.conf = a.cols == 7 ? r[6] : (T)1;
  } else {
    const float* d = a.dets + ((long)i * a.max_det + j) * 6;
    const float cx = (d[0] + d[2]) / 2.f, cy = (d[1] + d[3]) / 2.f, w = d[2] - d[0], h = d[3] - d[1];
    t.cls = (T)d[5]; t.x = (T)cx; t.y = (T)cy; t.w = (T)w; t.h = (T)h; t.conf = (T)d[4];
  }
  return true;
}

template <typename T, int FORM>
__global__ void __launch_bounds__(MATCH_THREADS) mosaic_slots_kernel(SlotArgs a) {
  __shared__ T s_max[MATCH_THREADS];
  __shared__ int s_cnt[MATCH_THREADS], s_drawn[MATCH_THREADS], s_nan[MATCH_THREADS];
  __shared__ int s_w[MATCH_THREADS / 64];
  const int i = blockIdx.x, tid = threadIdx.x;
  const bool has_conf = FORM == 1 || a.cols == 7;
  int n = a.nt;
  if (FORM == 1) {
    n = a.counts[i];
    n = n < 0 ? 0 : (n > a.max_det ? a.max_det : n);
  }
  // pass 1: the image's box maximum (boxes.max(), :173), its number of boxes and of drawn targets
  T mx = (T)0;
  int cnt = 0, drawn = 0, nan = 0, bad = 0;
  for (int j = tid; j < n; j += MATCH_THREADS) {
    Target<T> t;
    if (!load_target<T, FORM>(a, i, j, t)) continue;
    const T x1 = t.x - t.w / (T)2, y1 = t.y - t.h / (T)2, x2 = t.x + t.w / (T)2, y2 = t.y + t.h / (T)2;      // xywh2xyxy
    if (!(x1 == x1) || !(y1 == y1) || !(x2 == x2) || !(y2 == y2)) nan = 1;
    T m = x1 > y1 ? x1 : y1;
    m = x2 > m ? x2 : m;
    m = y2 > m ? y2 : m;
    mx = (cnt == 0 || m > mx) ? m : mx;
    ++cnt;
    const int c = trunc_cls(t.cls);
    if (c < 0 || c >= a.nc) bad = 1;
    else if (!has_conf || t.conf > (T)0.25) ++drawn;
  }
  if (bad) atomicOr(a.flag, CFT_MOSAIC_BAD_CLASS);
  s_max[tid] = mx; s_cnt[tid] = cnt; s_drawn[tid] = drawn; s_nan[tid] = nan;
  __syncthreads();
  for (int o = MATCH_THREADS / 2; o > 0; o >>= 1) {
    if (tid < o) {
      if (s_cnt[tid + o] > 0 && (s_cnt[tid] == 0 || s_max[tid + o] > s_max[tid])) s_max[tid] = s_max[tid + o];
      s_cnt[tid] += s_cnt[tid + o]; s_drawn[tid] += s_drawn[tid + o]; s_nan[tid] |= s_nan[tid + o];
    }
    __syncthreads();
  }
  const int D = s_drawn[0];
  const bool normalised = s_cnt[0] > 0 && !s_nan[0] && s_max[0] <= (T)1.01;
  const T sf = (T)a.sf, fw = (T)a.w, fh = (T)a.h;
  const bool scale = !normalised && a.sf < 1.0;
  if (tid == 0 && D > a.cap) atomicOr(a.flag, CFT_MOSAIC_OVERFLOW);
  int4* S = reinterpret_cast<int4*>(a.slots + (long)i * a.cap * BOX_WORDS);
  const int4 z = make_int4(0, 0, 0, 0);
  for (int s = (D < a.cap ? D : a.cap) + tid; s < a.cap; s += MATCH_THREADS) {
    int4* o = S + (long)s * (BOX_WORDS / 4);
    o[0] = z; o[1] = z; o[2] = z; o[3] = z;
  }
  // pass 2: drawn target k of D (target order) goes to slot D - 1 - k: the last drawn ends on top
  int total = 0;
  for (int j0 = 0; j0 < n; j0 += MATCH_THREADS) {             // uniform trip count
    const int j = j0 + tid;
    Target<T> t;
    int c = -1, draw = 0;
    if (j < n && load_target<T, FORM>(a, i, j, t)) {
      c = trunc_cls(t.cls);
      draw = c >= 0 && c < a.nc && (!has_conf || t.conf > (T)0.25);
    }
    int chunk;
    const int k = total + block_excl_scan(draw, s_w, &chunk);
    total += chunk;
    const int s = D - 1 - k;
    if (!draw || s >= a.cap) continue;
    T x1 = t.x - t.w / (T)2, y1 = t.y - t.h / (T)2, x2 = t.x + t.w / (T)2, y2 = t.y + t.h / (T)2;
    if (normalised) { x1 = x1 * fw; x2 = x2 * fw; y1 = y1 * fh; y2 = y2 * fh; }
    else if (scale) { x1 = x1 * sf; y1 = y1 * sf; x2 = x2 * sf; y2 = y2 * sf; }
    int4* o = S + (long)s * (BOX_WORDS / 4);
    o[0] = make_int4(trunc_int(x1), trunc_int(y1), trunc_int(x2), trunc_int(y2));
    o[1] = make_int4(c, has_conf ? conf_tenths((double)t.conf) : 0, 1, 0);
    o[2] = z; o[3] = z;
  }
}

extern "C" int cft_mosaic_slots(const void* rows, int nt, int cols, int f64, const float* dets, const int* counts, int B, int max_det, int bs, int cap,
                                int nc, int h, int w, const double* sf, int* slots, int* flag, void* stream) {
  CFT_REQUIRE(slots && flag && sf, "cft_mosaic_slots: null pointer");
  CFT_REQUIRE((rows != nullptr) != (dets != nullptr), "cft_mosaic_slots: give rows or dets, not both");
  CFT_REQUIRE(bs > 0 && bs <= 65535 && cap > 0 && (long)bs * cap < (1L << 31) / BOX_WORDS, "cft_mosaic_slots: bad slot table shape");
  CFT_REQUIRE(((size_t)slots & 15) == 0 && ((size_t)flag & 3) == 0, "cft_mosaic_slots: slots must be 16-byte aligned, flag 4-byte");
  CFT_REQUIRE(nc >= 1 && nc <= 32767, "cft_mosaic_slots: nc must be in [1, 32767]");
  CFT_REQUIRE(h > 0 && w > 0 && h <= MOSAIC_MAX_SIDE && w <= MOSAIC_MAX_SIDE, "cft_mosaic_slots: bad cell size");
  CFT_REQUIRE(*sf > 0.0 && *sf < 1e30, "cft_mosaic_slots: the scale factor must be positive and finite");
  SlotArgs a;
  a.rows = rows; a.dets = dets; a.counts = counts; a.slots = slots; a.flag = flag; a.sf = *sf;
  a.nt = nt; a.cols = cols; a.max_det = max_det; a.cap = cap; a.nc = nc; a.h = h; a.w = w;
  if (rows) {
    CFT_REQUIRE(nt > 0 && nt < (1 << 27), "cft_mosaic_slots: nt must be in [1, 2^27)");
    CFT_REQUIRE(cols == 6 || cols == 7, "cft_mosaic_slots: rows have 6 or 7 columns");
    CFT_REQUIRE(((size_t)rows & (f64 ? 7 : 3)) == 0, "cft_mosaic_slots: rows are misaligned");
    if (f64) hipLaunchKernelGGL((mosaic_slots_kernel<double, 0>), dim3(bs), dim3(MATCH_THREADS), 0, as_stream(stream), a);
    else hipLaunchKernelGGL((mosaic_slots_kernel<float, 0>), dim3(bs), dim3(MATCH_THREADS), 0, as_stream(stream), a);
  } else {
    CFT_REQUIRE(counts, "cft_mosaic_slots: dets need counts");
    CFT_REQUIRE(B >= bs && max_det > 0 && (long)B * max_det < (1L << 27), "cft_mosaic_slots: bad dets shape");
    CFT_REQUIRE(((size_t)dets & 3) == 0 && ((size_t)counts & 3) == 0, "cft_mosaic_slots: dets / counts are misaligned");
    a.cols = 7;
    hipLaunchKernelGGL((mosaic_slots_kernel<double, 1>), dim3(bs), dim3(MATCH_THREADS), 0, as_stream(stream), a);
  }
  return cft_check_launch("mosaic_slots_kernel");
}

// ------------------------------------------------------------------------------------------------------------------ finish
struct FinishArgs {
  unsigned char* img_rgb;
  unsigned char* img_ir;
  const unsigned char* codes;
  const int* name_len;
  const unsigned char* atlas;
  long stride_rgb, stride_ir;
  int bs, ns, h, w, gh, gw;
};

__global__ void __launch_bounds__(MOSAIC_THREADS) mosaic_finish_kernel(FinishArgs a) {
  const int MW = a.ns * a.w, MH = a.ns * a.h;
  const long p = (long)blockIdx.x * MOSAIC_THREADS + threadIdx.x;
  if (p >= (long)MH * MW) return;
  const int y = (int)(p / MW), x = (int)(p - (long)y * MW);
  // the occupied cells whose border rectangle [bx - 1, bx + w + 1] x [by - 1, by + h + 1] holds this pixel
  const int c_lo = x - a.w - 1 > 0 ? (x - 2) / a.w : 0, c_hi = (x + 1) / a.w < a.ns - 1 ? (x + 1) / a.w : a.ns - 1;
  const int r_lo = y - a.h - 1 > 0 ? (y - 2) / a.h : 0, r_hi = (y + 1) / a.h < a.ns - 1 ? (y + 1) / a.h : a.ns - 1;
  int value = -1;
  for (int c = c_lo; c <= c_hi && value < 0; ++c)
    for (int r = r_lo; r <= r_hi; ++r) {
      if (c * a.ns + r >= a.bs) continue;
      const int bx = c * a.w, by = r * a.h;
      if (x < bx - 1 || x > bx + a.w + 1 || y < by - 1 || y > by + a.h + 1) continue;
      if (x >= bx + 2 && x <= bx + a.w - 2 && y >= by + 2 && y <= by + a.h - 2) continue;
      value = 255;
      break;
    }
  if (value < 0 && a.codes) {                                   // the file name of the pixel's own cell
    const int c = x / a.w, r = y / a.h, i = c * a.ns + r;
    if (i < a.bs) {
      int n = a.name_len[i];
      n = n < 0 ? 0 : (n > CFT_MOSAIC_NAME_CHARS ? CFT_MOSAIC_NAME_CHARS : n);
      const int dx = x - c * a.w - 5, dy = y - r * a.h - 5;
      if (dx >= 0 && dy >= 0 && dy < a.gh && dx < n * a.gw) {
        const int k = dx / a.gw, u = dx - k * a.gw;
        int code = a.codes[(long)i * CFT_MOSAIC_NAME_CHARS + k];
        code = (code < 32 || code > 127) ? 0 : code - 32;
        if (a.atlas[((long)code * a.gh + dy) * a.gw + u] >= 128) value = 220;
      }
    }
  }
  if (value < 0) return;
  unsigned char* o = a.img_rgb + (long)y * a.stride_rgb + (long)x * 3;
  o[0] = (unsigned char)value; o[1] = (unsigned char)value; o[2] = (unsigned char)value;
  if (a.img_ir) {
    o = a.img_ir + (long)y * a.stride_ir + (long)x * 3;
    o[0] = (unsigned char)value; o[1] = (unsigned char)value; o[2] = (unsigned char)value;
  }
}

extern "C" int cft_mosaic_finish(unsigned char* img_rgb, unsigned char* img_ir, long stride_rgb, long stride_ir, int bs, int ns, int h, int w,
                                 const unsigned char* codes, const int* name_len, const unsigned char* atlas, int gh, int gw, void* stream) {
  CFT_REQUIRE(img_rgb, "cft_mosaic_finish: null pointer");
  CFT_REQUIRE(bs > 0 && ns > 0 && ns <= 256 && (long)ns * ns >= bs && (long)(ns - 1) * (ns - 1) < bs, "cft_mosaic_finish: ns must be ceil(sqrt(bs))");
  CFT_REQUIRE(h > 0 && w > 0 && (long)ns * h <= MOSAIC_MAX_SIDE && (long)ns * w <= MOSAIC_MAX_SIDE, "cft_mosaic_finish: bad cell size");
  CFT_REQUIRE(stride_rgb >= 3L * ns * w && stride_rgb <= (1L << 40), "cft_mosaic_finish: bad row stride");
  CFT_REQUIRE(!img_ir || (stride_ir >= 3L * ns * w && stride_ir <= (1L << 40)), "cft_mosaic_finish: bad row stride of the second mosaic");
  if (codes) {
    CFT_REQUIRE(name_len && atlas, "cft_mosaic_finish: file names need name_len and atlas");
    CFT_REQUIRE(((size_t)name_len & 3) == 0, "cft_mosaic_finish: name_len is misaligned");
    CFT_REQUIRE(gh >= 1 && gh <= 64 && gw >= 1 && gw <= 64, "cft_mosaic_finish: glyph size must be in [1, 64]");
  } else {
    gh = 1; gw = 1;
  }
  FinishArgs a;
  a.img_rgb = img_rgb; a.img_ir = img_ir; a.codes = codes; a.name_len = name_len; a.atlas = atlas;
  a.stride_rgb = stride_rgb; a.stride_ir = stride_ir; a.bs = bs; a.ns = ns; a.h = h; a.w = w; a.gh = gh; a.gw = gw;
  const long n = (long)ns * h * ns * w;
  hipLaunchKernelGGL(mosaic_finish_kernel, dim3((unsigned)((n + MOSAIC_THREADS - 1) / MOSAIC_THREADS)), dim3(MOSAIC_THREADS), 0, as_stream(stream), a);
  return cft_check_launch("mosaic_finish_kernel");
}
