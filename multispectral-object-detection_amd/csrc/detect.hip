// The device stage of detect_twostream.py between non_max_suppression and the files it writes (include/cft_hip.h):
//   cft_detect_boxes   what the loop of :129-153 computes about each detection: the rounded box, class, the two digits of the
//                      confidence, the save_one_box rectangle, the save_txt box and the per-image class counts;
//   cft_detect_render  plot_one_box for a whole batch, both streams, in place, one launch.
// The box transforms are those of cft_eval_match (metrics_common.h).  Integer atomics only; the render kernel writes each covered
// pixel once from one thread: every result is the same run to run.
#include "metrics_common.h"

#pragma clang fp contract(off)   // the reference's float ops are separate roundings: no fused multiply-adds here

constexpr int BOX_WORDS = 16;
enum { DETECT_BAD_CLASS = 1 };

// f'{conf:.2f}' as hundredths: round(v * 100) of the float's exact value v = m * 2^e, ties to even, in integers (100 m < 2^31).
// Saturates at 100; a negative value, zero or a NaN gives 0.
__device__ __forceinline__ int conf_hundredths(float conf) {
  unsigned int u;
  __builtin_memcpy(&u, &conf, 4);
  if (u >> 31) return 0;
  const int ex = (int)(u >> 23);
  if (ex == 255) return (u & 0x7fffffu) ? 0 : 100;   // NaN : +inf
  if (ex >= 127 + 1) return 100;                     // >= 2
  const unsigned long long m = ex ? ((u & 0x7fffffu) | 0x800000u) : (u & 0x7fffffu);
  const int s = 150 - (ex ? ex : 1);                 // v = m * 2^-s, s in [23, 149]
  if (s > 40) return 0;                              // v < 2^-17
  const unsigned long long p = m * 100ull, half = 1ull << (s - 1);
  unsigned long long q = p >> s;
  const unsigned long long rem = p & ((1ull << s) - 1ull);
  if (rem > half || (rem == half && (q & 1ull))) ++q;
  return q > 100ull ? 100 : (int)q;
}

// float -> integer as .long() does for the values met here (truncation toward zero); NaN -> 0, saturating far outside any image
__device__ __forceinline__ int trunc_coord(float v) {
  if (!(v == v)) return 0;
  return v <= -1073741824.f ? -1073741824 : (v >= 1073741824.f ? 1073741824 : (int)v);
}
__device__ __forceinline__ int clampi(int v, int lo, int hi) { return v < lo ? lo : (v > hi ? hi : v); }

// One workgroup per image: zero the image's class counts, then one thread per detection slot.
__global__ void __launch_bounds__(MATCH_THREADS) detect_boxes_kernel(const float* __restrict__ dets, const int* __restrict__ counts, int max_det,
                                                                     const float* __restrict__ geom, int nc, float crop_gain, float crop_pad,
                                                                     int square, int4* __restrict__ out, int* __restrict__ hist,
                                                                     int* __restrict__ flag) {
  const int b = blockIdx.x, tid = threadIdx.x;
  int* H = hist + (long)b * nc;
  for (int c = tid; c < nc; c += MATCH_THREADS) H[c] = 0;
  __threadfence();
  __syncthreads();
  int n = counts[b];
  n = n < 0 ? 0 : (n > max_det ? max_det : n);
  const Geom g = load_geom(geom, b);
  for (int r = tid; r < max_det; r += MATCH_THREADS) {
    int4* o = out + ((long)b * max_det + r) * (BOX_WORDS / 4);
    if (r >= n) {
      const int4 z = make_int4(0, 0, 0, 0);
      o[0] = z; o[1] = z; o[2] = z; o[3] = z;
      continue;
    }
    const float* d = dets + ((long)b * max_det + r) * 6;
    const float4 p = scale_box(d[0], d[1], d[2], d[3], g);
    const float x1 = rintf(p.x), y1 = rintf(p.y), x2 = rintf(p.z), y2 = rintf(p.w);      // torch.round: half to even
    const int cls = trunc_class(d[5]);
    if (cls >= 0 && cls < nc) atomicAdd(&H[cls], 1);
    else atomicOr(flag, DETECT_BAD_CLASS);
    const float cx = (x1 + x2) / 2.f, cy = (y1 + y2) / 2.f, w = x2 - x1, h = y2 - y1;   // xyxy2xywh
    // save_one_box: b[:, 2:] * gain + pad, xywh2xyxy, .long(), clip_coords
    float cw = w, ch = h;
    if (square) { cw = fmaxf(w, h); ch = cw; }
    cw = cw * crop_gain + crop_pad;
    ch = ch * crop_gain + crop_pad;
    const int w0 = trunc_coord(g.w0), h0 = trunc_coord(g.h0);
    const int bx1 = clampi(trunc_coord(cx - cw / 2.f), 0, w0), by1 = clampi(trunc_coord(cy - ch / 2.f), 0, h0);
    const int bx2 = clampi(trunc_coord(cx + cw / 2.f), 0, w0), by2 = clampi(trunc_coord(cy + ch / 2.f), 0, h0);
    o[0] = make_int4(trunc_coord(x1), trunc_coord(y1), trunc_coord(x2), trunc_coord(y2));
    o[1] = make_int4(cls, conf_hundredths(d[4]), 1, __float_as_int(d[4]));
    o[2] = make_int4(bx1, by1, bx2, by2);
    o[3] = make_int4(__float_as_int(cx / g.w0), __float_as_int(cy / g.h0), __float_as_int(w / g.w0), __float_as_int(h / g.h0));
  }
}

extern "C" int cft_detect_boxes(const float* dets, const int* counts, int B, int max_det, const float* geom, int nc, float crop_gain, float crop_pad,
                                int square, int* out, int* hist, int* flag, void* stream) {
  CFT_REQUIRE(dets && counts && geom && out && hist && flag, "cft_detect_boxes: null pointer");
  CFT_REQUIRE(B > 0 && B <= 65535 && max_det > 0 && (long)B * max_det < (1L << 31) / BOX_WORDS, "cft_detect_boxes: bad shape");
  CFT_REQUIRE(nc >= 1 && nc <= 32767, "cft_detect_boxes: nc must be in [1, 32767]");
  CFT_REQUIRE(((size_t)out & 15) == 0, "cft_detect_boxes: out must be 16-byte aligned");
  CFT_REQUIRE(crop_gain == crop_gain && crop_pad == crop_pad, "cft_detect_boxes: crop gain / pad is NaN");
  hipLaunchKernelGGL(detect_boxes_kernel, dim3(B), dim3(MATCH_THREADS), 0, as_stream(stream), dets, counts, max_det, geom, nc, crop_gain, crop_pad,
                     square, (int4*)out, hist, flag);
  return cft_check_launch("detect_boxes_kernel");
}

// ---------------------------------------------------------------------------------------------------------------- render
constexpr int RENDER_TW = 64, RENDER_TH = 16;       // one workgroup owns a 64 x 16 pixel tile of one image (both streams)
constexpr int RENDER_LDS_BOXES = 320;               // boxes touching a tile kept in LDS; a tile with more reads the box buffer itself
constexpr int RENDER_MAX_COORD = 1 << 24;

struct RenderArgs {
  const cft_render_desc_t* desc;
  const int* boxes;
  const unsigned char* colors;
  const unsigned char* names;
  const int* name_len;
  const unsigned char* atlas;
  int max_det, nc, text_color, t, flags, name_ld, gh, gw;
};

// characters of the confidence suffix: ' d.dd', or ' d.d' with CFT_RENDER_CONF1
__device__ __forceinline__ int render_conf_chars(int flags) { return (flags & CFT_RENDER_CONF1) ? 4 : 5; }

// What the raster needs of one slot: the box, class, hundredths and the label's length in characters (0: no label).
struct RenderBox { int x1, y1, x2, y2, cls, hund, n, pad; };

__device__ __forceinline__ bool load_render_box(const RenderArgs& a, const int* slot, RenderBox& e) {
  const int4 p = *reinterpret_cast<const int4*>(slot);
  const int4 q = *reinterpret_cast<const int4*>(slot + 4);
  if (q.z == 0 || q.x < 0 || q.x >= a.nc) return false;
  const int lo = (a.flags & CFT_RENDER_SIGNED) ? -RENDER_MAX_COORD : 0;
  e.x1 = clampi(p.x, lo, RENDER_MAX_COORD); e.y1 = clampi(p.y, lo, RENDER_MAX_COORD);
  e.x2 = clampi(p.z, lo, RENDER_MAX_COORD); e.y2 = clampi(p.w, lo, RENDER_MAX_COORD);
  e.cls = q.x;
  e.hund = clampi(q.y, 0, (a.flags & CFT_RENDER_CONF1) ? 10 : 100);      // tenths with CFT_RENDER_CONF1
  e.n = 0;
  e.pad = 0;
  if (a.flags & CFT_RENDER_LABELS) {
    e.n = clampi(a.name_len[q.x], 0, a.name_ld);
    if (a.flags & CFT_RENDER_CONF) e.n += render_conf_chars(a.flags);
  }
  return true;
}

// The rectangle outside of which the slot draws nothing: outline and label background (inclusive).
__device__ __forceinline__ void render_extent(const RenderBox& e, int t, int m, int gh, int gw, int& X0, int& Y0, int& X1, int& Y1) {
  const int a = t / 2;
  X0 = e.x1 - a; Y0 = e.y1 - a; X1 = e.x2 + a; Y1 = e.y2 + a;
  if (e.n > 0) {
    const int lx = e.x1 + e.n * gw * m, ly = e.y1 - gh * m - 3;
    X1 = X1 > lx ? X1 : lx;
    Y0 = Y0 < ly ? Y0 : ly;
  }
}

// 0: the slot does not cover pixel (px, py); 1: class colour; 2: text colour.  Text over background over outline.
__device__ __forceinline__ int render_cover(const RenderArgs& a, const RenderBox& e, int m, int px, int py) {
  const int cw = a.gw * m, chh = a.gh * m;
  if (e.n > 0 && px >= e.x1 && px <= e.x1 + e.n * cw && py >= e.y1 - chh - 3 && py <= e.y1) {
    const int top = e.y1 - 1 - chh, dx = px - e.x1, dy = py - top;
    if (dy >= 0 && dy < chh && dx < e.n * cw) {
      const int k = dx / cw, u = (dx - k * cw) / m, v = dy / m;
      const int len = e.n - ((a.flags & CFT_RENDER_CONF) ? render_conf_chars(a.flags) : 0);
      int code;
      if (k < len) {
        code = a.names[(long)e.cls * a.name_ld + k];
      } else if (a.flags & CFT_RENDER_CONF1) {
        const int j = k - len;
        code = j == 0 ? ' ' : (j == 1 ? '0' + e.hund / 10 : (j == 2 ? '.' : '0' + e.hund % 10));
      } else {
        const int j = k - len;
        code = j == 0 ? ' ' : (j == 1 ? '0' + e.hund / 100 : (j == 2 ? '.' : (j == 3 ? '0' + (e.hund / 10) % 10 : '0' + e.hund % 10)));
      }
      code = (code < 32 || code > 127) ? 0 : code - 32;
      if (a.atlas[((long)code * a.gh + v) * a.gw + u] >= 128) return 2;
    }
    return 1;
  }
  const int h = a.t / 2;
  if (px < e.x1 - h || px > e.x2 + h || py < e.y1 - h || py > e.y2 + h) return 0;
  const int i = a.t - h;
  if (px >= e.x1 + i && px <= e.x2 - i && py >= e.y1 + i && py <= e.y2 - i) return 0;
  return 1;
}

__global__ void __launch_bounds__(MATCH_THREADS) detect_render_kernel(RenderArgs a) {
  __shared__ RenderBox s_box[RENDER_LDS_BOXES];
  __shared__ int s_w[MATCH_THREADS / 64];
  const int b = blockIdx.y, tid = threadIdx.x;
  const cft_render_desc_t d = a.desc[b];                         // uniform over the workgroup
  const int tiles_x = (d.w0 + RENDER_TW - 1) / RENDER_TW, tiles_y = (d.h0 + RENDER_TH - 1) / RENDER_TH;
  if ((long)blockIdx.x >= (long)tiles_x * tiles_y) return;        // the grid is sized for the largest image of the batch
  const int tx0 = ((int)blockIdx.x % tiles_x) * RENDER_TW, ty0 = ((int)blockIdx.x / tiles_x) * RENDER_TH;
  const int tx1 = (tx0 + RENDER_TW < d.w0 ? tx0 + RENDER_TW : d.w0) - 1, ty1 = (ty0 + RENDER_TH < d.h0 ? ty0 + RENDER_TH : d.h0) - 1;
  const int m = (a.t + 1) / 3 > 1 ? (a.t + 1) / 3 : 1;
  const int* B0 = a.boxes + (long)b * a.max_det * BOX_WORDS;

  // the slots that touch this tile, compacted in row order
  int total = 0;
  for (int r0 = 0; r0 < a.max_det; r0 += MATCH_THREADS) {         // uniform trip count
    const int r = r0 + tid;
    RenderBox e;
    int touch = 0;
    if (r < a.max_det && load_render_box(a, B0 + (long)r * BOX_WORDS, e)) {
      int X0, Y0, X1, Y1;
      render_extent(e, a.t, m, a.gh, a.gw, X0, Y0, X1, Y1);
      touch = X0 <= tx1 && X1 >= tx0 && Y0 <= ty1 && Y1 >= ty0;
    }
    int chunk;
    const int pos = total + block_excl_scan(touch, s_w, &chunk);
    if (touch && pos < RENDER_LDS_BOXES) s_box[pos] = e;
    total += chunk;
  }
  if (total == 0) return;                                          // uniform: nothing is drawn in this tile
  __syncthreads();
  const bool in_lds = total <= RENDER_LDS_BOXES;
  const int nlist = in_lds ? total : a.max_det;

  for (int i = tid; i < RENDER_TW * RENDER_TH; i += MATCH_THREADS) {
    const int px = tx0 + i % RENDER_TW, py = ty0 + i / RENDER_TW;
    if (px > tx1 || py > ty1) continue;
    int hit = 0, cls = 0;
    for (int k = 0; k < nlist && !hit; ++k) {
      RenderBox e;
      if (in_lds) e = s_box[k];
      else if (!load_render_box(a, B0 + (long)k * BOX_WORDS, e)) continue;
      hit = render_cover(a, e, m, px, py);
      cls = e.cls;
    }
    if (!hit) continue;
    unsigned char c0, c1, c2;
    if (hit == 2) {
      c0 = (unsigned char)(a.text_color & 255); c1 = (unsigned char)((a.text_color >> 8) & 255); c2 = (unsigned char)((a.text_color >> 16) & 255);
    } else {
      const unsigned char* c = a.colors + (long)cls * 3;
      c0 = c[0]; c1 = c[1]; c2 = c[2];
    }
    unsigned char* o = d.img_rgb + (long)py * d.stride_rgb + (long)px * 3;
    o[0] = c0; o[1] = c1; o[2] = c2;
    if (d.img_ir) {
      o = d.img_ir + (long)py * d.stride_ir + (long)px * 3;
      o[0] = c0; o[1] = c1; o[2] = c2;
    }
  }
}

extern "C" int cft_detect_render(const void* desc_dev, const void* desc_host, int B, const int* boxes, int max_det, const unsigned char* colors, int nc,
                                 int text_color, int thickness, int flags, const unsigned char* names, const int* name_len, int name_ld,
                                 const unsigned char* atlas, int gh, int gw, void* stream) {
  static_assert(sizeof(cft_render_desc_t) == CFT_RENDER_DESC_BYTES, "cft_render_desc_t layout");
  static_assert(sizeof(RenderBox) == 32, "RenderBox layout");
  CFT_REQUIRE(desc_dev && desc_host && boxes && colors, "cft_detect_render: null pointer");
  CFT_REQUIRE(B > 0 && B <= 65535 && max_det > 0 && (long)B * max_det < (1L << 31) / BOX_WORDS, "cft_detect_render: bad shape");
  CFT_REQUIRE(((size_t)boxes & 15) == 0, "cft_detect_render: boxes must be 16-byte aligned");
  CFT_REQUIRE(nc >= 1 && nc <= 32767, "cft_detect_render: nc must be in [1, 32767]");
  CFT_REQUIRE(thickness >= 1 && thickness <= 64, "cft_detect_render: thickness must be in [1, 64]");
  CFT_REQUIRE((flags & ~(CFT_RENDER_LABELS | CFT_RENDER_CONF | CFT_RENDER_CONF1 | CFT_RENDER_SIGNED)) == 0, "cft_detect_render: unknown flag");
  CFT_REQUIRE(!(flags & CFT_RENDER_CONF) || (flags & CFT_RENDER_LABELS), "cft_detect_render: the conf flag needs the labels flag");
  CFT_REQUIRE(!(flags & CFT_RENDER_CONF1) || (flags & CFT_RENDER_CONF), "cft_detect_render: the tenths flag needs the conf flag");
  CFT_REQUIRE(text_color >= 0 && text_color <= 0xffffff, "cft_detect_render: text colour is three bytes");
  if (flags & CFT_RENDER_LABELS) {
    CFT_REQUIRE(names && name_len && atlas, "cft_detect_render: labels need names, name_len and atlas");
    CFT_REQUIRE(name_ld >= 1 && name_ld <= CFT_RENDER_MAX_NAME, "cft_detect_render: name_ld must be in [1, 32]");
    CFT_REQUIRE(gh >= 1 && gh <= 64 && gw >= 1 && gw <= 64, "cft_detect_render: glyph size must be in [1, 64]");
  } else {
    name_ld = 1; gh = 1; gw = 1;
  }
  const cft_render_desc_t* rows = static_cast<const cft_render_desc_t*>(desc_host);
  long tiles = 0;
  for (int b = 0; b < B; ++b) {
    const cft_render_desc_t& d = rows[b];
    CFT_REQUIRE(d.img_rgb, "cft_detect_render: null image pointer in the table");
    CFT_REQUIRE(d.h0 > 0 && d.w0 > 0 && d.h0 <= RENDER_MAX_COORD && d.w0 <= RENDER_MAX_COORD, "cft_detect_render: bad image size in the table");
    CFT_REQUIRE(d.stride_rgb >= 3L * d.w0 && (!d.img_ir || d.stride_ir >= 3L * d.w0), "cft_detect_render: bad row stride in the table");
    CFT_REQUIRE(d.stride_rgb <= (1L << 40) && d.stride_ir <= (1L << 40), "cft_detect_render: bad row stride in the table");
    CFT_REQUIRE(d.pad0 == 0 && d.pad1 == 0, "cft_detect_render: the table's padding words must be 0");
    const long tx = (d.w0 + RENDER_TW - 1) / RENDER_TW, ty = (d.h0 + RENDER_TH - 1) / RENDER_TH;
    tiles = tx * ty > tiles ? tx * ty : tiles;
  }
  CFT_REQUIRE(tiles < (1L << 31), "cft_detect_render: image too large");
  RenderArgs a;
  a.desc = static_cast<const cft_render_desc_t*>(desc_dev);
  a.boxes = boxes; a.colors = colors; a.names = names; a.name_len = name_len; a.atlas = atlas;
  a.max_det = max_det; a.nc = nc; a.text_color = text_color; a.t = thickness; a.flags = flags; a.name_ld = name_ld; a.gh = gh; a.gw = gw;
  hipLaunchKernelGGL(detect_render_kernel, dim3((unsigned)tiles, B), dim3(MATCH_THREADS), 0, as_stream(stream), a);
  return cft_check_launch("detect_render_kernel");
}
