// Shared by metrics.hip (cft_eval_match, cft_eval_ap), confusion.hip (cft_eval_confusion, cft_eval_export) and curves.hip
// (cft_eval_curves): the grouped-label workspace, the float32 box transforms of the reference in ATen's operation order, box_iou, the
// block scan, and (at the end) what the two walks over the sorted statistics share.  Include after
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

// ---------------------------------------------------------------------------------------------------------------------
// Shared by cft_eval_ap (metrics.hip) and cft_eval_curves (curves.hip): the sort workspace, the np.interp rule and the F1 argmax.
// ---------------------------------------------------------------------------------------------------------------------
constexpr int SORT_THREADS = 256;
constexpr int SORT_ITEMS = 16;
constexpr int SORT_TILE = SORT_THREADS * SORT_ITEMS;      // elements per workgroup of one radix pass
constexpr int CURVE_THREADS = 256;
static_assert(CURVE_THREADS == MATCH_THREADS, "ap_curve_kernel uses block_excl_scan");
constexpr int NPX = 1000;                                 // np.linspace(0, 1, 1000) (utils/metrics.py:40)

struct ApWs {
  unsigned* key[2];
  int* idx[2];
  unsigned* hist;     // [256 * nblk] per-pass digit counts, digit-major, scanned in place
  int* seg;           // [2 * (nc + 1)] start / end of each class in the sorted order
  double* pcurve;     // [nc, NPX]
  double* rcurve;     // [nc, NPX]
};
static inline int sort_blocks(long n) { return (int)((n + SORT_TILE - 1) / SORT_TILE); }
static inline size_t ap_ws_layout(long n, int nc, char* base, ApWs* w) {
  size_t o = 0;
  const size_t nn = n > 0 ? (size_t)n : 1;
  for (int i = 0; i < 2; ++i) {
    if (w) w->key[i] = (unsigned*)(base + o);
    o = align256(o + nn * 4);
    if (w) w->idx[i] = (int*)(base + o);
    o = align256(o + nn * 4);
  }
  if (w) w->hist = (unsigned*)(base + o);
  o = align256(o + (size_t)256 * (sort_blocks(n) > 0 ? sort_blocks(n) : 1) * 4);
  if (w) w->seg = (int*)(base + o);
  o = align256(o + (size_t)2 * (nc + 1) * 4);
  if (w) w->pcurve = (double*)(base + o);
  o = align256(o + (size_t)nc * NPX * 8);
  if (w) w->rcurve = (double*)(base + o);
  o = align256(o + (size_t)nc * NPX * 8);
  return o;
}

// The sort of cft_eval_ap (kernels in metrics.hip): fills w.idx[*cur] with the stable order by (class ascending, conf descending; ties in
// insertion order) and w.seg with each labelled class's range in it; detections of classes without labels sort last.  n == 0 only
// clears seg.  Launches only: no allocation, no synchronisation.  Arguments are the caller's to check.
int eval_sort_launch(const float* conf, const int* pcls, long n, const int* label_hist, int nc, const ApWs& w, int* cur, hipStream_t stream);

// np.interp between two nodes (numpy's rule: j = last node with xp[j] <= x; an exact hit gives fp[j], else slope*(x - xp[j]) + fp[j],
// retried from the right node if that is NaN)
__device__ __forceinline__ double np_interp_seg(double x, double xa, double ya, double xb, double yb) {
  if (x == xa) return ya;
  const double slope = (yb - ya) / (xb - xa);
  double v = slope * (x - xa) + ya;
  if (v != v) {
    v = slope * (x - xb) + yb;
    if (v != v && ya == yb) v = ya;
  }
  return v;
}

// first index q of the ascending grid g[0..len) with g[q] >= v (upper = false) or g[q] > v (upper = true)
__device__ __forceinline__ int grid_bound(const double* g, int len, double v, bool upper) {
  int lo = 0, hi = len;
  while (lo < hi) {
    const int mid = (lo + hi) >> 1;
    if (upper ? (g[mid] <= v) : (g[mid] < v)) lo = mid + 1; else hi = mid;
  }
  return lo;
}

// The index of f1.mean(0).argmax() (utils/metrics.py:70, :77) by one workgroup of 1024 threads: f1 = 2 p r / (p + r + 1e-16) over the
// classes with labels, rows summed in class order as numpy does, first index on ties, a NaN wins as in np.argmax.  s_v / s_i hold 16
// values, *s_best receives the index; every thread returns it.
__device__ __forceinline__ int f1_best_index(const int* __restrict__ label_hist, int nc, const double* __restrict__ pcurve,
                                             const double* __restrict__ rcurve, double* s_v, int* s_i, int* s_best) {
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  double m = 0.0;
  int mi = -1;
  if (tid < NPX) {
    double sum = 0.0;
    int u = 0;
    bool first = true;
    for (int c = 0; c < nc; ++c) {
      if (label_hist[c] <= 0) continue;
      const double p = pcurve[(long)c * NPX + tid], r = rcurve[(long)c * NPX + tid];
      const double f = 2.0 * p * r / (p + r + 1e-16);
      sum = first ? f : sum + f;
      first = false;
      ++u;
    }
    m = sum / (double)u;
    mi = tid;
  }
  auto better = [](double a, int ai, double b, int bi) {
    if (ai < 0) return false;
    if (bi < 0) return true;
    if (b != b) return a != a && ai < bi;
    if (a != a) return true;
    return a > b || (a == b && ai < bi);
  };
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    const double v2 = __shfl_xor(m, o);
    const int i2 = __shfl_xor(mi, o);
    if (better(v2, i2, m, mi)) { m = v2; mi = i2; }
  }
  if (lane == 0) { s_v[wave] = m; s_i[wave] = mi; }
  __syncthreads();
  if (tid == 0) {
    double bv = s_v[0];
    int bi = s_i[0];
    for (int w = 1; w < 16; ++w)
      if (better(s_v[w], s_i[w], bv, bi)) { bv = s_v[w]; bi = s_i[w]; }
    *s_best = bi < 0 ? 0 : bi;
  }
  __syncthreads();
  return *s_best;
}
