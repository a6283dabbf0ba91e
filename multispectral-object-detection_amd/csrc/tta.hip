// Test-time augmentation of the single-stream model (reference models/yolo.py:113-128, utils/torch_utils.py:247-257), include/cft_hip.h:
//   cft_tta_view   one augmented view of an image batch: optional left-right flip, bilinear resize (torch's align_corners=False
//                  arithmetic in float32), right / bottom padding with 0.447, as fp32 NCHW - what the reference hands to forward_once;
//   cft_tta_merge  the three views' predictions into one tensor: boxes de-scaled, the flipped view's x mirrored back, rows concatenated.
// A thread writes TTA_PX neighbouring pixels of one output row (view) or one element (merge).  No atomics, no LDS, no inline assembly;
// every output element is written once, by one thread: two runs give the same bits.
#include "cft_common.h"

#pragma clang fp contract(off)   // the float arithmetic restates torch's CPU expressions: separate roundings, no fused multiply-adds

constexpr int TTA_THREADS = 256;
constexpr int TTA_PX = 4;                 // output pixels of a row per thread
constexpr int TTA_MAX_SIDE = 1 << 15;

__device__ __forceinline__ float tta_load(const void* p, int dtype, long i) {
  if (dtype == CFT_TTA_U8) return __fdiv_rn((float)static_cast<const unsigned char*>(p)[i], 255.f);
  if (dtype == CFT_TTA_F16) return (float)static_cast<const f16_t*>(p)[i];
  return static_cast<const float*>(p)[i];
}

struct TtaTap { int i0, i1; float w0, w1; };

// one axis of torch's bilinear resize with align_corners=False: scale = in / out; src = max(scale * (dst + 0.5) - 0.5, 0);
// i0 = min(floor(src), in - 1); i1 = min(i0 + 1, in - 1); w1 = src - i0 clamped to [0, 1]; w0 = 1 - w1
__device__ __forceinline__ TtaTap tta_tap(int dst, float scale, int in) {
  float src = scale * ((float)dst + 0.5f) - 0.5f;
  src = src < 0.f ? 0.f : src;
  int i0 = (int)floorf(src);
  i0 = i0 > in - 1 ? in - 1 : i0;
  float lam = src - (float)i0;
  lam = lam < 0.f ? 0.f : (lam > 1.f ? 1.f : lam);
  TtaTap t;
  t.i0 = i0;
  t.i1 = i0 + 1 > in - 1 ? in - 1 : i0 + 1;
  t.w1 = lam;
  t.w0 = 1.f - lam;
  return t;
}

struct ViewArgs {
  const void* img;
  float* out;
  long sb, sc, sh, sw;
  float scale_h, scale_w;
  int dtype, B, H, W, hs, ws, Ho, Wo, flip;
};

__global__ void __launch_bounds__(TTA_THREADS) tta_view_kernel(ViewArgs a) {
  const int groups = (a.Wo + TTA_PX - 1) / TTA_PX;
  const long t = (long)blockIdx.x * TTA_THREADS + threadIdx.x;
  if (t >= (long)a.B * 3 * a.Ho * groups) return;
  const int g = (int)(t % groups);
  const long row = t / groups;                       // (b * 3 + c) * Ho + y
  const int y = (int)(row % a.Ho);
  const long bc = row / a.Ho;
  const int c = (int)(bc % 3), b = (int)(bc / 3);
  float* o = a.out + row * a.Wo;
  const int x0 = g * TTA_PX;
  float v[TTA_PX];
  if (y >= a.hs) {
#pragma unroll
    for (int k = 0; k < TTA_PX; ++k) v[k] = 0.447f;
  } else {
    const TtaTap ty = tta_tap(y, a.scale_h, a.H);
    const long r0 = b * a.sb + c * a.sc + ty.i0 * a.sh, r1 = b * a.sb + c * a.sc + ty.i1 * a.sh;
#pragma unroll
    for (int k = 0; k < TTA_PX; ++k) {
      const int x = x0 + k;
      if (x >= a.ws) {                               // padding, and the lanes past the row's end (not stored)
        v[k] = 0.447f;
        continue;
      }
      const TtaTap tx = tta_tap(x, a.scale_w, a.W);
      const int xa = a.flip ? a.W - 1 - tx.i0 : tx.i0, xb = a.flip ? a.W - 1 - tx.i1 : tx.i1;     // the taps of the mirrored image
      const float p00 = tta_load(a.img, a.dtype, r0 + xa * a.sw), p01 = tta_load(a.img, a.dtype, r0 + xb * a.sw);
      const float p10 = tta_load(a.img, a.dtype, r1 + xa * a.sw), p11 = tta_load(a.img, a.dtype, r1 + xb * a.sw);
      const float h0 = p00 * tx.w0 + p01 * tx.w1;
      const float h1 = p10 * tx.w0 + p11 * tx.w1;
      v[k] = h0 * ty.w0 + h1 * ty.w1;
    }
  }
  if (a.Wo % TTA_PX == 0) {
    *reinterpret_cast<float4*>(o + x0) = make_float4(v[0], v[1], v[2], v[3]);
  } else {
#pragma unroll
    for (int k = 0; k < TTA_PX; ++k)
      if (x0 + k < a.Wo) o[x0 + k] = v[k];
  }
}

static_assert(TTA_PX == 4, "the view kernel stores a float4");

// the sizes of utils/torch_utils.py:252-256 in the doubles Python uses: int(side * ratio) and ceil(side * ratio / gs) * gs
static inline int tta_scaled(int side, double ratio) { return (int)((double)side * ratio); }
static inline long tta_padded(int side, double ratio, int gs) {
  const double q = (double)side * ratio / (double)gs;
  long c = (long)q;
  if ((double)c < q) ++c;
  return c * gs;
}

extern "C" int cft_tta_view(const void* img, int dtype, int B, int H, int W, long sb, long sc, long sh, long sw, const double* ratio, int gs,
                            int flip, float* out, int Ho, int Wo, void* stream) {
  CFT_REQUIRE(img && out && ratio, "cft_tta_view: null pointer");
  CFT_REQUIRE(dtype == CFT_TTA_U8 || dtype == CFT_TTA_F16 || dtype == CFT_TTA_F32, "cft_tta_view: dtype must be uint8, fp16 or fp32");
  CFT_REQUIRE(((size_t)img & (dtype == CFT_TTA_F32 ? 3 : dtype == CFT_TTA_F16 ? 1 : 0)) == 0, "cft_tta_view: img is misaligned");
  CFT_REQUIRE(((size_t)out & 15) == 0, "cft_tta_view: out must be 16-byte aligned");
  CFT_REQUIRE(B > 0 && B <= 65535 && H > 0 && W > 0 && H <= TTA_MAX_SIDE && W <= TTA_MAX_SIDE, "cft_tta_view: bad batch shape");
  CFT_REQUIRE(*ratio > 0.0 && *ratio <= 1.0, "cft_tta_view: ratio must be in (0, 1]");
  CFT_REQUIRE(gs >= 1 && gs <= TTA_MAX_SIDE, "cft_tta_view: gs must be in [1, 32768]");
  CFT_REQUIRE(flip == 0 || flip == 1, "cft_tta_view: flip is 0 or 1");
  const int hs = tta_scaled(H, *ratio), ws = tta_scaled(W, *ratio);
  CFT_REQUIRE(hs >= 1 && ws >= 1, "cft_tta_view: the scaled image is empty");
  CFT_REQUIRE(tta_padded(H, *ratio, gs) == Ho && tta_padded(W, *ratio, gs) == Wo, "cft_tta_view: out is not [B, 3, ceil(H r / gs) gs, ceil(W r / gs) gs]");
  CFT_REQUIRE(Ho >= hs && Wo >= ws && Ho <= TTA_MAX_SIDE && Wo <= TTA_MAX_SIDE, "cft_tta_view: bad output size");
  const long lim = 1L << 40;
  CFT_REQUIRE(sb >= 0 && sc >= 0 && sh >= 0 && sw >= 0 && sb < lim && sc < lim && sh < lim && sw < lim, "cft_tta_view: strides must be in [0, 2^40)");
  CFT_REQUIRE((B - 1) * sb + 2 * sc + (H - 1) * sh + (W - 1) * sw < (1L << 46), "cft_tta_view: batch too large");
  const long threads = (long)B * 3 * Ho * ((Wo + TTA_PX - 1) / TTA_PX);
  CFT_REQUIRE((threads + TTA_THREADS - 1) / TTA_THREADS < (1L << 31), "cft_tta_view: batch too large");
  ViewArgs a;
  a.img = img; a.out = out; a.sb = sb; a.sc = sc; a.sh = sh; a.sw = sw;
  a.scale_h = (float)H / (float)hs; a.scale_w = (float)W / (float)ws;
  a.dtype = dtype; a.B = B; a.H = H; a.W = W; a.hs = hs; a.ws = ws; a.Ho = Ho; a.Wo = Wo; a.flip = flip;
  hipLaunchKernelGGL(tta_view_kernel, dim3((unsigned)((threads + TTA_THREADS - 1) / TTA_THREADS)), dim3(TTA_THREADS), 0, as_stream(stream), a);
  return cft_check_launch("tta_view_kernel");
}

struct MergeArgs {
  const float *y0, *y1, *y2;
  float* out;
  float s0, s1, s2, img_w;
  int n0, n1, n2, flip_mask, B, no, total;
};

__global__ void __launch_bounds__(TTA_THREADS) tta_merge_kernel(MergeArgs a) {
  const long e = (long)blockIdx.x * TTA_THREADS + threadIdx.x;
  if (e >= (long)a.B * a.total * a.no) return;
  const int col = (int)(e % a.no);
  const long row = e / a.no;
  int r = (int)(row % a.total);
  const int b = (int)(row / a.total);
  int v = 0;
  if (r >= a.n0) { r -= a.n0; v = 1; }
  if (v == 1 && r >= a.n1) { r -= a.n1; v = 2; }
  const float* y = v == 0 ? a.y0 : (v == 1 ? a.y1 : a.y2);
  const int nv = v == 0 ? a.n0 : (v == 1 ? a.n1 : a.n2);
  const float sv = v == 0 ? a.s0 : (v == 1 ? a.s1 : a.s2);
  float x = y[((long)b * nv + r) * a.no + col];
  if (col < 4) {
    x = __fdiv_rn(x, sv);                                  // yi[..., :4] /= si
    if (col == 0 && ((a.flip_mask >> v) & 1)) x = a.img_w - x;       // yi[..., 0] = img_w - yi[..., 0]
  }
  a.out[e] = x;
}

extern "C" int cft_tta_merge(const float* y0, const float* y1, const float* y2, int B, int n0, int n1, int n2, int no, float s0, float s1, float s2,
                             int flip_mask, float img_w, float* out, int total, void* stream) {
  CFT_REQUIRE(y0 && y1 && y2 && out, "cft_tta_merge: null pointer");
  CFT_REQUIRE((((size_t)y0 | (size_t)y1 | (size_t)y2 | (size_t)out) & 3) == 0, "cft_tta_merge: pointers must be 4-byte aligned");
  CFT_REQUIRE(B > 0 && B <= 65535 && no >= 5 && no <= 65535, "cft_tta_merge: bad batch size or row width");
  CFT_REQUIRE(n0 > 0 && n1 > 0 && n2 > 0 && n0 < (1 << 28) && n1 < (1 << 28) && n2 < (1 << 28), "cft_tta_merge: bad row count");
  CFT_REQUIRE((long)n0 + n1 + n2 == total, "cft_tta_merge: the views' row counts do not add up to the output's");
  CFT_REQUIRE(s0 > 0.f && s0 <= 1.f && s1 > 0.f && s1 <= 1.f && s2 > 0.f && s2 <= 1.f, "cft_tta_merge: ratio must be in (0, 1]");
  CFT_REQUIRE(flip_mask >= 0 && flip_mask < 8, "cft_tta_merge: flip_mask has one bit per view");
  CFT_REQUIRE(img_w >= 1.f && img_w <= (float)TTA_MAX_SIDE, "cft_tta_merge: bad image width");
  const long n = (long)B * total * no;
  CFT_REQUIRE((n + TTA_THREADS - 1) / TTA_THREADS < (1L << 31), "cft_tta_merge: tensor too large");
  const float* lo = out;
  const float* hi = out + n;
  const float* ys[3] = {y0, y1, y2};
  const int ns[3] = {n0, n1, n2};
  for (int v = 0; v < 3; ++v)
    CFT_REQUIRE(ys[v] + (long)B * ns[v] * no <= lo || hi <= ys[v], "cft_tta_merge: an input overlaps the output");
  MergeArgs a;
  a.y0 = y0; a.y1 = y1; a.y2 = y2; a.out = out;
  a.s0 = s0; a.s1 = s1; a.s2 = s2; a.img_w = img_w;
  a.n0 = n0; a.n1 = n1; a.n2 = n2;
  a.flip_mask = flip_mask; a.B = B; a.no = no; a.total = total;
  hipLaunchKernelGGL(tta_merge_kernel, dim3((unsigned)((n + TTA_THREADS - 1) / TTA_THREADS)), dim3(TTA_THREADS), 0, as_stream(stream), a);
  return cft_check_launch("tta_merge_kernel");
}
