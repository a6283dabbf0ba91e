// Shared by metrics.hip (cft_eval_match, cft_eval_ap) and confusion.hip (cft_eval_confusion, cft_eval_export): the grouped-label
// workspace, the float32 box transforms of the reference in ATen's operation order, box_iou and the block scan.  Include after
// `#pragma clang fp contract(off)`: the reference's float ops are separate roundings.
#pragma once
#include "cft_common.h"

#pragma clang fp contract(off)

constexpr int MATCH_THREADS = 256;
constexpr int MATCH_LDS_LABELS = 1024;      // labels of one image kept in LDS; more are read from the workspace

// Workspace of cft_eval_match: grouped label records (box, class, winner row) and per-image label ranges.
struct MatchWs {
  float4* box;   // [nt] native-space xyxy
  int* cls;      // [nt] class (-1: not an integer class; never matches)
  int* win;      // [nt] lowest row that claims the label (global-memory path only)
  int* off;      // [B] first grouped label of each image
  int* cnt;      // [B] labels of each image
};
static inline size_t align256(size_t x) { return (x + 255) & ~(size_t)255; }
static inline size_t match_ws_layout(int B, int nt, char* base, MatchWs* w) {
  size_t o = 0;
  const size_t n = nt > 0 ? (size_t)nt : 1;
  if (w) w->box = (float4*)(base + o);
  o = align256(o + n * 16);
  if (w) w->cls = (int*)(base + o);
  o = align256(o + n * 4);
  if (w) w->win = (int*)(base + o);
  o = align256(o + n * 4);
  if (w) w->off = (int*)(base + o);
  o = align256(o + (size_t)B * 4);
  if (w) w->cnt = (int*)(base + o);
  o = align256(o + (size_t)B * 4);
  return o;
}

// targets[:, 0] as an image index: exactly an integer in [0, B), else the label belongs to no image (test.py:136 compares with ==)
__device__ __forceinline__ int label_image(float v, int B) {
  if (!(v >= 0.f) || !(v < (float)B)) return -1;
  const int b = (int)v;
  return (float)b == v ? b : -1;
}

struct Geom { float h0, w0, gain, padw, padh; };

// scale_coords (utils/general.py:353-366) + clip_coords (:369-374) on one xyxy box, float32 like ATen
__device__ __forceinline__ float4 scale_box(float x1, float y1, float x2, float y2, const Geom& g) {
  x1 = x1 - g.padw; x2 = x2 - g.padw;
  y1 = y1 - g.padh; y2 = y2 - g.padh;
  x1 = x1 / g.gain; y1 = y1 / g.gain; x2 = x2 / g.gain; y2 = y2 / g.gain;
  x1 = fminf(fmaxf(x1, 0.f), g.w0); x2 = fminf(fmaxf(x2, 0.f), g.w0);
  y1 = fminf(fmaxf(y1, 0.f), g.h0); y2 = fminf(fmaxf(y2, 0.f), g.h0);
  return make_float4(x1, y1, x2, y2);
}

__device__ __forceinline__ Geom load_geom(const float* geom, int b) {
  const float* g = geom + (long)b * 5;
  Geom r;
  r.h0 = g[0]; r.w0 = g[1]; r.gain = g[2]; r.padw = g[3]; r.padh = g[4];
  return r;
}

// Block-wide exclusive prefix sum of one int per thread (MATCH_THREADS threads); returns the block total through *total.
__device__ __forceinline__ int block_excl_scan(int v, int* s_w, int* total) {
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  int x = v;
#pragma unroll
  for (int o = 1; o < 64; o <<= 1) {
    const int y = __shfl_up(x, o);
    if (lane >= o) x += y;
  }
  if (lane == 63) s_w[wave] = x;
  __syncthreads();
  int before = 0, all = 0;
  for (int w = 0; w < MATCH_THREADS / 64; ++w) {
    const int c = s_w[w];
    if (w < wave) before += c;
    all += c;
  }
  __syncthreads();
  *total = all;
  return before + x - v;
}

// How eval_group_kernel reads a label row: GROUP_NATIVE = columns 2..5 are native-space xyxy already (no transform);
// GROUP_TRUNC_CLS = the class is the value truncated toward zero (`.int()`, utils/metrics.py:130) instead of an exact integer.
enum { GROUP_NATIVE = 1, GROUP_TRUNC_CLS = 2 };

// float class -> int as torch's .int() (truncation toward zero); -1 for a NaN or a value an int cannot hold
__device__ __forceinline__ int trunc_class(float cf) {
  return (cf > -2147483648.f && cf < 2147483520.f) ? (int)cf : -1;
}

// box_iou (utils/general.py:422-444) of one prediction with one label, float32: inter / (area1 + area2 - inter)
__device__ __forceinline__ float box_iou1(const float4& p, float pa, const float4& t) {
  const float iw = fmaxf(fminf(p.z, t.z) - fmaxf(p.x, t.x), 0.f);
  const float ih = fmaxf(fminf(p.w, t.w) - fmaxf(p.y, t.y), 0.f);
  const float inter = iw * ih;
  const float ta = (t.z - t.x) * (t.w - t.y);
  return inter / (pa + ta - inter);
}

// The grouping launch (eval_group_kernel, metrics.hip): labels of image b, in target order, to [off[b], off[b] + cnt[b]) of the workspace.
int eval_group_launch(const float* targets, int nt, int B, float img_h, float img_w, const float* geom, MatchWs ws, int* label_hist, int nc,
                      int* tcls, int* nl, int mode, unsigned long long* key, hipStream_t stream);
