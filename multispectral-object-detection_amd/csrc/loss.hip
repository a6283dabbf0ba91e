// The reference's ComputeLoss (utils/loss.py:88-216) and its gradient with respect to the head outputs, on the GPU:
//   cft_loss_forward   build_targets, the matched entries (CIoU, class BCE), the dense objectness BCE, the scalars;
//   cft_loss_backward  dL/dp_i of every level given the upstream gradient of the scalar (a device pointer).
// build_targets' decisions are the reference's float32 decisions bit for bit (same operations, same order, correctly
// rounded division, torch's remainder); the losses and gradients are computed in float64 from the float32 inputs.
// Candidate lists are compacted with prefix scans, never with atomics, so their order is the reference's.  No float
// atomics anywhere, no allocation, no host synchronisation: both entry points can be captured in a graph, and every
// result is the same run to run.
#include "cft_common.h"

#pragma clang fp contract(off)   // the reference's float ops are separate roundings: no fused multiply-adds here

constexpr int LOSS_MAX_NL = 5;
constexpr int LOSS_THREADS = 256;
constexpr int PAIR_ITEMS = 4;                                  // consecutive (anchor, target) pairs per thread
constexpr int PAIR_TILE = LOSS_THREADS * PAIR_ITEMS;
constexpr int OBJ_ITEMS = 16;
constexpr int OBJ_TILE = LOSS_THREADS * OBJ_ITEMS;             // cells per workgroup of the dense objectness pass
constexpr int SCAN_THREADS_L = 1024;
constexpr int LSORT_ITEMS = 16;
constexpr int LSORT_TILE = LOSS_THREADS * LSORT_ITEMS;

enum { HYP_BOX, HYP_OBJ, HYP_CLS, HYP_CLS_PW, HYP_OBJ_PW, HYP_ANCHOR_T, HYP_FL_GAMMA, HYP_CP, HYP_CN, HYP_GR, HYP_N };

// error bits ORed into the caller's flag
constexpr int LOSS_ERR_IMAGE = 1;     // a target whose image index is outside [0, B) passed the anchor test (it is skipped)
constexpr int LOSS_ERR_CLASS = 2;     // nc > 1 and a target whose class is outside [0, nc) passed the anchor test (it is skipped)

struct LossArgs {
  const float* p[LOSS_MAX_NL];
  int ny[LOSS_MAX_NL], nx[LOSS_MAX_NL];
  int cells[LOSS_MAX_NL];             // B * na * ny * nx
  int nl, B, na, nc, no, nt;
  int cap;                            // 5 * na * nt candidate slots per level
  int npb;                            // pair workgroups per level
  int nbc;                            // candidate workgroups per level (cap / LOSS_THREADS)
  int nbo;                            // objectness workgroups per level (largest level)
  float anchor_t;
  double box, obj, cls, cls_pw, obj_pw, fl_gamma, cp, cn, gr;
};

struct LossGrads { float* g[LOSS_MAX_NL]; };   // dL/dp_l of every level (kernel argument, indexed like LossArgs::p)

struct LossWs {
  int* cell;          // [nl][cap] flattened (b, a, gj, gi) of each candidate
  int* cls;           // [nl][cap]
  float4* tbox;       // [nl][cap] (gxy - gij, gwh)
  float* tobj;        // [nl][cap] the objectness target the candidate would write
  unsigned* key[2];   // [nl][cap] sort keys (cell) and payloads (candidate index) of the backward's stable sort
  int* idx[2];
  int* win;           // [sum cells] last candidate (largest index) per cell, -1 = none
  int* blk;           // [nl][5][npb] per-workgroup candidate counts, offset-major; scanned in place into bases
  int* n;             // [nl] candidates per level
  double* part_box;   // [nl][nbc]
  double* part_cls;   // [nl][nbc]
  double* part_obj;   // [nl][nbo]
  double* bal_used;   // [nl] the balance the forward used (autobalance updates balance itself)
  unsigned* hist;     // [nl][256 * nbs] radix digit counts
  long win_off[LOSS_MAX_NL];
};

static inline size_t lalign(size_t x) { return (x + 255) & ~(size_t)255; }
static inline int lsort_blocks(int cap) { return (cap + LSORT_TILE - 1) / LSORT_TILE; }

static inline size_t loss_ws_layout(const LossArgs& A, char* base, LossWs* w) {
  size_t o = 0;
  const size_t cap = (size_t)(A.cap > 0 ? A.cap : 1) * A.nl;
  auto take = [&](size_t bytes) { char* r = base ? base + o : nullptr; o = lalign(o + bytes); return r; };
  char* cell = take(cap * 4);
  char* cls = take(cap * 4);
  char* tbox = take(cap * 16);
  char* tobj = take(cap * 4);
  char* k0 = take(cap * 4);
  char* k1 = take(cap * 4);
  char* i0 = take(cap * 4);
  char* i1 = take(cap * 4);
  size_t ncell = 0;
  long woff[LOSS_MAX_NL];
  for (int l = 0; l < A.nl; ++l) { woff[l] = (long)ncell; ncell += (size_t)A.cells[l]; }
  char* win = take(ncell * 4);
  char* blk = take((size_t)A.nl * 5 * A.npb * 4);
  char* n = take((size_t)A.nl * 4);
  char* pb = take((size_t)A.nl * A.nbc * 8);
  char* pc = take((size_t)A.nl * A.nbc * 8);
  char* po = take((size_t)A.nl * A.nbo * 8);
  char* bu = take((size_t)A.nl * 8);
  const int nbs = lsort_blocks(A.cap > 0 ? A.cap : 1);
  char* hist = take((size_t)A.nl * 256 * nbs * 4);
  if (w) {
    w->cell = (int*)cell; w->cls = (int*)cls; w->tbox = (float4*)tbox; w->tobj = (float*)tobj;
    w->key[0] = (unsigned*)k0; w->key[1] = (unsigned*)k1; w->idx[0] = (int*)i0; w->idx[1] = (int*)i1;
    w->win = (int*)win; w->blk = (int*)blk; w->n = (int*)n;
    w->part_box = (double*)pb; w->part_cls = (double*)pc; w->part_obj = (double*)po; w->bal_used = (double*)bu;
    w->hist = (unsigned*)hist;
    for (int l = 0; l < A.nl; ++l) w->win_off[l] = woff[l];
  }
  return o;
}

// ---------------------------------------------------------------------------------------------------------------------
// block-wide helpers (fixed orders: deterministic)
// ---------------------------------------------------------------------------------------------------------------------
template <typename T, int NT>
__device__ __forceinline__ T block_scan_excl(T v, T* s_w, T* total) {
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  T x = v;
#pragma unroll
  for (int o = 1; o < 64; o <<= 1) {
    const T y = __shfl_up(x, o);
    if (lane >= o) x += y;
  }
  if (lane == 63) s_w[wave] = x;
  __syncthreads();
  T before = 0, all = 0;
#pragma unroll
  for (int w = 0; w < NT / 64; ++w) {
    const T c = s_w[w];
    if (w < wave) before += c;
    all += c;
  }
  __syncthreads();
  *total = all;
  return before + x - v;
}

// sum of one double per thread, in a fixed tree order; the result is valid in thread 0
__device__ __forceinline__ double block_sum(double v, double* s_w) {
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_down(v, o);
  if (lane == 0) s_w[wave] = v;
  __syncthreads();
  double s = 0.0;
  if (tid == 0)
    for (int w = 0; w < LOSS_THREADS / 64; ++w) s += s_w[w];
  __syncthreads();
  return s;
}

// ---------------------------------------------------------------------------------------------------------------------
// (a) build_targets (utils/loss.py:166-216)
// ---------------------------------------------------------------------------------------------------------------------
// torch.remainder(v, 1.) for float32: fmod, then shifted into [0, 1) when negative (ATen's rule)
__device__ __forceinline__ float rem1(float v) {
  float m = fmodf(v, 1.f);
  if (m != 0.f && m < 0.f) m += 1.f;
  return m;
}

// float -> long truncation of .long(), bounded first so that out-of-range values stay defined (they are clamped later anyway)
__device__ __forceinline__ int trunc_i(float v) {
  v = fminf(fmaxf(v, -1.0e9f), 1.0e9f);
  return (int)v;
}

struct PairT { float x, y, w, h; int b, c; };

// Offsets of build_targets, offset-major: [0,0], [1,0], [0,1], [-1,0], [0,-1] times g = 0.5
__device__ __forceinline__ float off_x(int o) { return o == 1 ? 0.5f : (o == 3 ? -0.5f : 0.f); }
__device__ __forceinline__ float off_y(int o) { return o == 2 ? 0.5f : (o == 4 ? -0.5f : 0.f); }

// 5-bit mask of the offsets that keep pair q = a * nt + t on level l (0: the pair is filtered out)
__device__ __forceinline__ int pair_mask(const LossArgs& A, int l, int q, const float* __restrict__ targets,
                                         const float* __restrict__ anchors, int* __restrict__ err, PairT* pt) {
  const int a = q / A.nt, t = q - a * A.nt;
  const float* tg = targets + (long)t * 6;
  const float gx = (float)A.nx[l], gy = (float)A.ny[l];
  // t = targets * gain (gain = 1, 1, nx, ny, nx, ny, 1)
  const float x = tg[2] * gx, y = tg[3] * gy, w = tg[4] * gx, h = tg[5] * gy;
  const float aw = anchors[(l * A.na + a) * 2], ah = anchors[(l * A.na + a) * 2 + 1];
  // r = wh / anchor; max(r, 1 / r).max(2) < anchor_t   (NaN compares false either way)
  const float r0 = __fdiv_rn(w, aw), r1 = __fdiv_rn(h, ah);
  const float i0 = __fdiv_rn(1.f, r0), i1 = __fdiv_rn(1.f, r1);
  const float m0 = (r0 != r0 || i0 != i0) ? r0 + i0 : fmaxf(r0, i0);
  const float m1 = (r1 != r1 || i1 != i1) ? r1 + i1 : fmaxf(r1, i1);
  const float mm = (m0 != m0 || m1 != m1) ? m0 + m1 : fmaxf(m0, m1);
  if (!(mm < A.anchor_t)) return 0;
  const float bf = tg[0], cf = tg[1];
  if (!(bf > -1.f && bf < (float)A.B)) { atomicOr(err, LOSS_ERR_IMAGE); return 0; }
  if (A.nc > 1 && !(cf > -1.f && cf < (float)A.nc)) { atomicOr(err, LOSS_ERR_CLASS); return 0; }
  const float xi = gx - x, yi = gy - y;          // gxi = gain[[2, 3]] - gxy
  int mask = 1;
  mask |= (rem1(x) < 0.5f && x > 1.f) ? 2 : 0;
  mask |= (rem1(y) < 0.5f && y > 1.f) ? 4 : 0;
  mask |= (rem1(xi) < 0.5f && xi > 1.f) ? 8 : 0;
  mask |= (rem1(yi) < 0.5f && yi > 1.f) ? 16 : 0;
  pt->x = x; pt->y = y; pt->w = w; pt->h = h;
  pt->b = (int)bf;
  pt->c = A.nc > 1 ? (int)cf : 0;
  return mask;
}

__global__ void __launch_bounds__(LOSS_THREADS) loss_init_kernel(LossArgs A, LossWs w) {
  const int l = blockIdx.y;
  int* win = w.win + w.win_off[l];
  for (long i = (long)blockIdx.x * LOSS_THREADS + threadIdx.x; i < A.cells[l]; i += (long)gridDim.x * LOSS_THREADS) win[i] = -1;
}

// packed per-offset counts: 12 bits per offset (a workgroup keeps at most PAIR_TILE = 1024 candidates of one offset)
__device__ __forceinline__ unsigned long long pack_mask(int m) {
  unsigned long long v = 0;
#pragma unroll
  for (int o = 0; o < 5; ++o) v += (unsigned long long)((m >> o) & 1) << (12 * o);
  return v;
}

__global__ void __launch_bounds__(LOSS_THREADS) loss_count_kernel(LossArgs A, const float* __restrict__ targets, const float* __restrict__ anchors,
                                                                  LossWs w, int* __restrict__ err) {
  __shared__ unsigned long long s_w[LOSS_THREADS / 64];
  const int l = blockIdx.y, blk = blockIdx.x, npairs = A.na * A.nt;
  unsigned long long cnt = 0;
  const int q0 = blk * PAIR_TILE + threadIdx.x * PAIR_ITEMS;
  for (int k = 0; k < PAIR_ITEMS; ++k) {
    const int q = q0 + k;
    if (q >= npairs) break;
    PairT pt;
    cnt += pack_mask(pair_mask(A, l, q, targets, anchors, err, &pt));
  }
  unsigned long long tot;
  block_scan_excl<unsigned long long, LOSS_THREADS>(cnt, s_w, &tot);
  if (threadIdx.x < 5) w.blk[((long)l * 5 + threadIdx.x) * A.npb + blk] = (int)((tot >> (12 * threadIdx.x)) & 4095u);
}

// exclusive scan of the 5 * npb offset-major counts of each level, in place; n[l] = the level's candidate count
__global__ void __launch_bounds__(SCAN_THREADS_L) loss_scan_kernel(LossArgs A, LossWs w) {
  __shared__ int s_w[SCAN_THREADS_L / 64];
  const int l = blockIdx.x, m = 5 * A.npb, tid = threadIdx.x;
  if (A.nt == 0) {                          // no pairs: the counts were never written
    if (tid == 0) w.n[l] = 0;
    return;
  }
  int* h = w.blk + (long)l * m;
  const int per = (m + SCAN_THREADS_L - 1) / SCAN_THREADS_L;
  const int a = tid * per, e = min(a + per, m);
  int s = 0;
  for (int i = a; i < e; ++i) s += h[i];
  int tot;
  int run = block_scan_excl<int, SCAN_THREADS_L>(s, s_w, &tot);
  for (int i = a; i < e; ++i) { const int v = h[i]; h[i] = run; run += v; }
  if (tid == 0) w.n[l] = tot;
}

// writes the candidates in the reference's order (offset-major, then anchor-major pairs); the winner map gets the
// largest candidate index per cell (integer atomicMax: the last writer of tobj[b, a, gj, gi] in candidate order)
__global__ void __launch_bounds__(LOSS_THREADS) loss_scatter_kernel(LossArgs A, const float* __restrict__ targets, const float* __restrict__ anchors,
                                                                    LossWs w, int* __restrict__ err) {
  __shared__ unsigned long long s_w[LOSS_THREADS / 64];
  const int l = blockIdx.y, blk = blockIdx.x, npairs = A.na * A.nt;
  int masks[PAIR_ITEMS];
  PairT pts[PAIR_ITEMS];
  unsigned long long cnt = 0;
  const int q0 = blk * PAIR_TILE + threadIdx.x * PAIR_ITEMS;
#pragma unroll
  for (int k = 0; k < PAIR_ITEMS; ++k) {
    const int q = q0 + k;
    masks[k] = q < npairs ? pair_mask(A, l, q, targets, anchors, err, &pts[k]) : 0;
    cnt += pack_mask(masks[k]);
  }
  unsigned long long tot;
  const unsigned long long before = block_scan_excl<unsigned long long, LOSS_THREADS>(cnt, s_w, &tot);
  const long cbase = (long)l * A.cap;
  int* win = w.win + w.win_off[l];
  const int nx = A.nx[l], ny = A.ny[l];
#pragma unroll
  for (int o = 0; o < 5; ++o) {
    int pos = w.blk[((long)l * 5 + o) * A.npb + blk] + (int)((before >> (12 * o)) & 4095u);
    const float ox = off_x(o), oy = off_y(o);
#pragma unroll
    for (int k = 0; k < PAIR_ITEMS; ++k) {
      if (!((masks[k] >> o) & 1)) continue;
      const PairT& p = pts[k];
      const int a = (q0 + k) / A.nt;
      // gij = (gxy - offsets).long(); indices clamped in place, so tbox (gxy - gij) sees the clamped gij as in the reference
      int gi = trunc_i(p.x - ox), gj = trunc_i(p.y - oy);
      gi = min(max(gi, 0), nx - 1);
      gj = min(max(gj, 0), ny - 1);
      const int cell = ((p.b * A.na + a) * ny + gj) * nx + gi;
      w.cell[cbase + pos] = cell;
      w.cls[cbase + pos] = p.c;
      w.tbox[cbase + pos] = make_float4(p.x - (float)gi, p.y - (float)gj, p.w, p.h);
      atomicMax(&win[cell], pos);
      ++pos;
    }
  }
}

// ---------------------------------------------------------------------------------------------------------------------
// (b) per-candidate terms, float64
// ---------------------------------------------------------------------------------------------------------------------
__device__ __forceinline__ double sigm(double x) { return 1.0 / (1.0 + exp(-x)); }

// nn.BCEWithLogitsLoss(pos_weight=pw), optionally wrapped in FocalLoss(gamma, alpha = 0.25); value and d/dx
__device__ __forceinline__ void bce_focal(double x, double y, double pw, double gamma, double* val, double* grad) {
  const double lw = 1.0 + (pw - 1.0) * y;
  const double sp = fmax(-x, 0.0) + log1p(exp(-fabs(x)));     // softplus(-x)
  const double L = (1.0 - y) * x + lw * sp;
  const double p = sigm(x);
  const double dL = (1.0 - y) - lw * (1.0 - p);
  if (gamma > 0.0) {
    const double pt = y * p + (1.0 - y) * (1.0 - p);
    const double af = y * 0.25 + (1.0 - y) * 0.75;
    const double q = 1.0 - pt;
    const double mf = pow(q, gamma);
    const double dq = -(2.0 * y - 1.0) * p * (1.0 - p);        // d(1 - p_t)/dx
    const double dmf = q > 0.0 ? gamma * pow(q, gamma - 1.0) * dq : 0.0;
    if (val) *val = L * af * mf;
    if (grad) *grad = af * (dL * mf + L * dmf);
  } else {
    if (val) *val = L;
    if (grad) *grad = dL;
  }
}

// d min(a, b) / da as torch's minimum backward (ties split the gradient); dmax likewise
__device__ __forceinline__ double dmin_a(double a, double b) { return a < b ? 1.0 : (a == b ? 0.5 : 0.0); }
__device__ __forceinline__ double dmax_a(double a, double b) { return a > b ? 1.0 : (a == b ? 0.5 : 0.0); }

// CIoU of bbox_iou(pbox, tbox, x1y1x2y2=False, CIoU=True, eps=1e-7) from the raw logits ps[0..3]; optionally the gradient
// of G * ciou with respect to the logits (alpha constant, as under the reference's no_grad)
__device__ __forceinline__ double ciou_logits(const float* ps, float4 tb, double aw, double ah, double G, double* g4) {
  const double eps = 1e-7;
  const double sx = sigm(ps[0]), sy = sigm(ps[1]), sw = sigm(ps[2]), sh = sigm(ps[3]);
  const double px = sx * 2.0 - 0.5, py = sy * 2.0 - 0.5;
  const double pw = (sw * 2.0) * (sw * 2.0) * aw, ph = (sh * 2.0) * (sh * 2.0) * ah;
  const double a_x1 = px - pw / 2, a_x2 = px + pw / 2, a_y1 = py - ph / 2, a_y2 = py + ph / 2;
  const double tx = tb.x, ty = tb.y, tw = tb.z, th = tb.w;
  const double b_x1 = tx - tw / 2, b_x2 = tx + tw / 2, b_y1 = ty - th / 2, b_y2 = ty + th / 2;
  const double iw0 = fmin(a_x2, b_x2) - fmax(a_x1, b_x1), ih0 = fmin(a_y2, b_y2) - fmax(a_y1, b_y1);
  const double iw = fmax(iw0, 0.0), ih = fmax(ih0, 0.0);
  const double inter = iw * ih;
  const double w1 = a_x2 - a_x1, h1 = a_y2 - a_y1 + eps;
  const double w2 = b_x2 - b_x1, h2 = b_y2 - b_y1 + eps;
  const double uni = w1 * h1 + w2 * h2 - inter + eps;
  const double iou = inter / uni;
  const double cw = fmax(a_x2, b_x2) - fmin(a_x1, b_x1), ch = fmax(a_y2, b_y2) - fmin(a_y1, b_y1);
  const double c2 = cw * cw + ch * ch + eps;
  const double dx = b_x1 + b_x2 - a_x1 - a_x2, dy = b_y1 + b_y2 - a_y1 - a_y2;
  const double rho2 = (dx * dx + dy * dy) / 4;
  const double kk = 4.0 / (3.141592653589793 * 3.141592653589793);
  const double dA = atan(w2 / h2) - atan(w1 / h1);
  const double v = kk * dA * dA;
  const double alpha = v / (v - iou + (1.0 + eps));
  const double ciou = iou - (rho2 / c2 + v * alpha);
  if (g4) {
    double gx1 = 0, gx2 = 0, gy1 = 0, gy2 = 0, gw1 = 0, gh1 = 0;
    const double g_iou = G, g_rc = -G, g_v = -G * alpha;
    // rho2 / c2
    const double g_rho2 = g_rc / c2, g_c2 = -g_rc * rho2 / (c2 * c2);
    const double g_cw = g_c2 * 2 * cw, g_ch = g_c2 * 2 * ch;
    gx2 += g_cw * dmax_a(a_x2, b_x2); gx1 -= g_cw * dmin_a(a_x1, b_x1);
    gy2 += g_ch * dmax_a(a_y2, b_y2); gy1 -= g_ch * dmin_a(a_y1, b_y1);
    const double g_dx = g_rho2 * dx / 2, g_dy = g_rho2 * dy / 2;
    gx1 -= g_dx; gx2 -= g_dx; gy1 -= g_dy; gy2 -= g_dy;
    // v = k (atan(w2 / h2) - atan(w1 / h1))^2
    const double q = w1 / h1;
    const double g_q = g_v * kk * 2 * dA * (-1.0) / (1.0 + q * q);
    gw1 += g_q / h1; gh1 -= g_q * w1 / (h1 * h1);
    // iou = inter / union
    double g_inter = g_iou / uni;
    const double g_uni = -g_iou * inter / (uni * uni);
    gw1 += g_uni * h1; gh1 += g_uni * w1; g_inter -= g_uni;
    const double g_iw = iw0 >= 0.0 ? g_inter * ih : 0.0, g_ih = ih0 >= 0.0 ? g_inter * iw : 0.0;
    gx2 += g_iw * dmin_a(a_x2, b_x2); gx1 -= g_iw * dmax_a(a_x1, b_x1);
    gy2 += g_ih * dmin_a(a_y2, b_y2); gy1 -= g_ih * dmax_a(a_y1, b_y1);
    gx2 += gw1; gx1 -= gw1; gy2 += gh1; gy1 -= gh1;
    const double g_px = gx1 + gx2, g_py = gy1 + gy2;
    const double g_pw = (gx2 - gx1) / 2, g_ph = (gy2 - gy1) / 2;
    g4[0] = g_px * 2.0 * sx * (1.0 - sx);
    g4[1] = g_py * 2.0 * sy * (1.0 - sy);
    g4[2] = g_pw * aw * 8.0 * sw * sw * (1.0 - sw);
    g4[3] = g_ph * ah * 8.0 * sh * sh * (1.0 - sh);
  }
  return ciou;
}

__device__ __forceinline__ void level_anchor(const LossArgs& A, const float* anchors, int l, int cell, double* aw, double* ah) {
  const int a = (cell / (A.ny[l] * A.nx[l])) % A.na;
  *aw = anchors[(l * A.na + a) * 2];
  *ah = anchors[(l * A.na + a) * 2 + 1];
}

__global__ void __launch_bounds__(LOSS_THREADS) loss_match_kernel(LossArgs A, const float* __restrict__ anchors, LossWs w) {
  __shared__ double s_w[LOSS_THREADS / 64];
  const int l = blockIdx.y, c = blockIdx.x * LOSS_THREADS + threadIdx.x;
  const long cb = (long)l * A.cap;
  double sb = 0.0, sc = 0.0;
  if (c < w.n[l]) {
    const int cell = w.cell[cb + c];
    const float* ps = A.p[l] + (long)cell * A.no;
    double aw, ah;
    level_anchor(A, anchors, l, cell, &aw, &ah);
    const double ciou = ciou_logits(ps, w.tbox[cb + c], aw, ah, 0.0, nullptr);
    sb = 1.0 - ciou;
    // tobj = (1 - gr) + gr * iou.detach().clamp(0), stored in float32 as the reference's tobj tensor
    const float iouf = (float)ciou;
    w.tobj[cb + c] = (float)((1.0 - A.gr) + A.gr * (double)fmaxf(iouf, 0.f));
    if (A.nc > 1) {
      const int k = w.cls[cb + c];
      for (int j = 0; j < A.nc; ++j) {
        double v;
        bce_focal(ps[5 + j], j == k ? A.cp : A.cn, A.cls_pw, A.fl_gamma, &v, nullptr);
        sc += v;
      }
    }
  }
  const double tb = block_sum(sb, s_w);
  const double tc = block_sum(sc, s_w);
  if (threadIdx.x == 0) { w.part_box[(long)l * A.nbc + blockIdx.x] = tb; w.part_cls[(long)l * A.nbc + blockIdx.x] = tc; }
}

// ---------------------------------------------------------------------------------------------------------------------
// (d) dense objectness BCE, tobj read through the winner map
// ---------------------------------------------------------------------------------------------------------------------
__device__ __forceinline__ double cell_tobj(const LossWs& w, const int* win, long cb, int cell) {
  const int k = win[cell];
  return k >= 0 ? (double)w.tobj[cb + k] : 0.0;
}

__global__ void __launch_bounds__(LOSS_THREADS) loss_obj_kernel(LossArgs A, LossWs w) {
  __shared__ double s_w[LOSS_THREADS / 64];
  const int l = blockIdx.y, blk = blockIdx.x;
  const int cells = A.cells[l];
  const int nb = (cells + OBJ_TILE - 1) / OBJ_TILE;
  if (blk >= nb) {
    if (threadIdx.x == 0) w.part_obj[(long)l * A.nbo + blk] = 0.0;
    return;
  }
  const int* win = w.win + w.win_off[l];
  const long cb = (long)l * A.cap;
  const float* p = A.p[l];
  double s = 0.0;
  for (int k = 0; k < OBJ_ITEMS; ++k) {
    const int e = blk * OBJ_TILE + k * LOSS_THREADS + threadIdx.x;
    if (e >= cells) break;
    double v;
    bce_focal(p[(long)e * A.no + 4], cell_tobj(w, win, cb, e), A.obj_pw, A.fl_gamma, &v, nullptr);
    s += v;
  }
  const double t = block_sum(s, s_w);
  if (threadIdx.x == 0) w.part_obj[(long)l * A.nbo + blk] = t;
}

// ---------------------------------------------------------------------------------------------------------------------
// (e) the scalars
// ---------------------------------------------------------------------------------------------------------------------
__device__ double sum_parts(const double* v, int n, double* s_w) {
  double s = 0.0;
  for (int i = threadIdx.x; i < n; i += LOSS_THREADS) s += v[i];
  return block_sum(s, s_w);
}

__global__ void __launch_bounds__(LOSS_THREADS) loss_finish_kernel(LossArgs A, LossWs w, double* __restrict__ balance, int autobalance, int ssi,
                                                                   float* __restrict__ loss_out, float* __restrict__ items) {
  __shared__ double s_w[LOSS_THREADS / 64];
  double lbox = 0.0, lobj = 0.0, lcls = 0.0;
  for (int l = 0; l < A.nl; ++l) {
    const double sb = sum_parts(w.part_box + (long)l * A.nbc, A.nbc, s_w);
    const double sc = sum_parts(w.part_cls + (long)l * A.nbc, A.nbc, s_w);
    const double so = sum_parts(w.part_obj + (long)l * A.nbo, (A.cells[l] + OBJ_TILE - 1) / OBJ_TILE, s_w);
    if (threadIdx.x == 0) {
      const int n = w.n[l];
      if (n) {
        lbox += sb / n;
        if (A.nc > 1) lcls += sc / ((double)n * A.nc);
      }
      const double obji = so / A.cells[l];
      const double b = balance[l];
      w.bal_used[l] = b;
      lobj += obji * b;
      if (autobalance) balance[l] = b * 0.9999 + 0.0001 / obji;
    }
  }
  if (threadIdx.x == 0) {
    if (autobalance) {
      const double d = balance[ssi];
      for (int l = 0; l < A.nl; ++l) balance[l] = balance[l] / d;
    }
    lbox *= A.box; lobj *= A.obj; lcls *= A.cls;
    const double loss = lbox + lobj + lcls;
    loss_out[0] = (float)(loss * A.B);
    items[0] = (float)lbox; items[1] = (float)lobj; items[2] = (float)lcls; items[3] = (float)loss;
  }
}

// ---------------------------------------------------------------------------------------------------------------------
// (f) backward
// ---------------------------------------------------------------------------------------------------------------------
// dense pass: every element of dL/dp_l, zero except the objectness channel
__global__ void __launch_bounds__(LOSS_THREADS) loss_grad_dense_kernel(LossArgs A, LossWs w, const float* __restrict__ gout, LossGrads G) {
  const int l = blockIdx.y;
  float* g = G.g[l];
  const long total = (long)A.cells[l] * A.no;
  const long e0 = (long)blockIdx.x * LOSS_THREADS + threadIdx.x;
  if (e0 >= total) return;
  const double scale = (double)gout[0] * A.B * A.obj * w.bal_used[l] / A.cells[l];
  const int* win = w.win + w.win_off[l];
  const long cb = (long)l * A.cap;
  for (long e = e0; e < total; e += (long)gridDim.x * LOSS_THREADS) {
    const int ch = (int)(e % A.no);
    float v = 0.f;
    if (ch == 4) {
      const int cell = (int)(e / A.no);
      double d;
      bce_focal(A.p[l][e], cell_tobj(w, win, cb, cell), A.obj_pw, A.fl_gamma, nullptr, &d);
      v = (float)(d * scale);
    }
    g[e] = v;
  }
}

__global__ void __launch_bounds__(LOSS_THREADS) lsort_init_kernel(LossArgs A, LossWs w) {
  const int l = blockIdx.y, c = blockIdx.x * LOSS_THREADS + threadIdx.x;
  if (c >= w.n[l]) return;
  const long cb = (long)l * A.cap;
  w.key[0][cb + c] = (unsigned)w.cell[cb + c];
  w.idx[0][cb + c] = c;
}

__global__ void __launch_bounds__(LOSS_THREADS) lsort_hist_kernel(LossArgs A, LossWs w, int cur, int shift, int nbs) {
  __shared__ unsigned s_h[256];
  const int tid = threadIdx.x, blk = blockIdx.x, l = blockIdx.y;
  s_h[tid] = 0u;
  __syncthreads();
  const int n = w.n[l];
  const unsigned* key = w.key[cur] + (long)l * A.cap;
  const int base = blk * LSORT_TILE;
  for (int k = 0; k < LSORT_ITEMS; ++k) {
    const int i = base + k * LOSS_THREADS + tid;
    if (i < n) atomicAdd(&s_h[(key[i] >> shift) & 255u], 1u);     // integer counts: deterministic
  }
  __syncthreads();
  w.hist[(long)l * 256 * nbs + (long)tid * nbs + blk] = s_h[tid];
}

__global__ void __launch_bounds__(SCAN_THREADS_L) lsort_scan_kernel(LossWs w, int nbs) {
  __shared__ unsigned s_w[SCAN_THREADS_L / 64];
  const int l = blockIdx.x, m = 256 * nbs, tid = threadIdx.x;
  unsigned* h = w.hist + (long)l * m;
  const int per = (m + SCAN_THREADS_L - 1) / SCAN_THREADS_L;
  const int a = tid * per, e = min(a + per, m);
  unsigned s = 0u;
  for (int i = a; i < e; ++i) s += h[i];
  unsigned tot;
  unsigned run = block_scan_excl<unsigned, SCAN_THREADS_L>(s, s_w, &tot);
  for (int i = a; i < e; ++i) { const unsigned v = h[i]; h[i] = run; run += v; }
}

// stable scatter of one 8-bit digit (ballot ranks within a wave, LDS counts across waves, tiles in order)
__global__ void __launch_bounds__(LOSS_THREADS) lsort_scatter_kernel(LossArgs A, LossWs w, int cur, int shift, int nbs) {
  constexpr int NW = LOSS_THREADS / 64;
  __shared__ unsigned s_base[256];
  __shared__ unsigned s_wc[NW][256];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, blk = blockIdx.x, l = blockIdx.y;
  const int n = w.n[l];
  const int base = blk * LSORT_TILE;
  if (base >= n) return;                    // whole workgroup: no barrier below is skipped by part of it
  const long cb = (long)l * A.cap;
  const unsigned* key_in = w.key[cur] + cb;
  const int* idx_in = w.idx[cur] + cb;
  unsigned* key_out = w.key[cur ^ 1] + cb;
  int* idx_out = w.idx[cur ^ 1] + cb;
  s_base[tid] = w.hist[(long)l * 256 * nbs + (long)tid * nbs + blk];
  const unsigned long long lt = (1ull << lane) - 1ull;
  for (int k = 0; k < LSORT_ITEMS; ++k) {
    const int i = base + k * LOSS_THREADS + tid;
    const bool valid = i < n;
    const unsigned key = valid ? key_in[i] : 0u;
    const unsigned d = (key >> shift) & 255u;
    unsigned long long peers = __ballot(valid);
#pragma unroll
    for (int bit = 0; bit < 8; ++bit) {
      const bool set = (d >> bit) & 1u;
      const unsigned long long bal = __ballot(set);
      peers &= set ? bal : ~bal;
    }
    const unsigned rank = (unsigned)__popcll(peers & lt);
#pragma unroll
    for (int ww = 0; ww < NW; ++ww) s_wc[ww][tid] = 0u;
    __syncthreads();
    if (valid && rank == 0u) s_wc[wave][d] = (unsigned)__popcll(peers);
    __syncthreads();
    {
      unsigned run = s_base[tid];
#pragma unroll
      for (int ww = 0; ww < NW; ++ww) { const unsigned c = s_wc[ww][tid]; s_wc[ww][tid] = run; run += c; }
      s_base[tid] = run;
    }
    __syncthreads();
    if (valid) {
      const unsigned dst = s_wc[wave][d] + rank;
      key_out[dst] = key;
      idx_out[dst] = idx_in[i];
    }
    __syncthreads();
  }
}

// matched cells: the sorted candidates of one cell form a segment (candidate order kept by the stable sort); its first
// position sums the gradients of the segment in that order and writes them (the reference's gather pi[b, a, gj, gi]
// accumulates duplicates).  Box and class channels are two kernels, each with few live scalars (no register spills).
// Returns the segment's cell, or -1 when position s does not start a segment.
__device__ __forceinline__ int segment_head(const unsigned* key, int s, int n) {
  if (s >= n) return -1;
  const unsigned cell = key[s];
  return (s > 0 && key[s - 1] == cell) ? -1 : (int)cell;
}

__global__ void __launch_bounds__(LOSS_THREADS) loss_grad_box_kernel(LossArgs A, const float* __restrict__ anchors, LossWs w, int cur,
                                                                     const float* __restrict__ gout, LossGrads G) {
  const int l = blockIdx.y, s = blockIdx.x * LOSS_THREADS + threadIdx.x;
  const int n = w.n[l];
  const long cb = (long)l * A.cap;
  const unsigned* key = w.key[cur] + cb;
  const int cell = segment_head(key, s, n);
  if (cell < 0) return;
  int e = s + 1;
  while (e < n && key[e] == (unsigned)cell) ++e;
  const int* idx = w.idx[cur] + cb;
  const float4* tbox = w.tbox + cb;
  const float* ps = A.p[l] + (long)cell * A.no;
  double aw, ah;
  level_anchor(A, anchors, l, cell, &aw, &ah);
  double acc[4] = {0.0, 0.0, 0.0, 0.0};                   // sum of d ciou / d logits, in candidate order
  for (int f = s; f < e; ++f) {
    double g4c[4];
    ciou_logits(ps, tbox[idx[f]], aw, ah, 1.0, g4c);
#pragma unroll
    for (int k = 0; k < 4; ++k) acc[k] += g4c[k];
  }
  const double gbox = -(double)gout[0] * A.B * A.box / n;        // d loss / d ciou of one candidate
  float* g = G.g[l] + (long)cell * A.no;
#pragma unroll
  for (int k = 0; k < 4; ++k) g[k] = (float)(acc[k] * gbox);
}

// class channels (nc > 1): per channel, the segment's candidates of that class take the cp target, the others cn
__global__ void __launch_bounds__(LOSS_THREADS) loss_grad_cls_kernel(LossArgs A, LossWs w, int cur, const float* __restrict__ gout, LossGrads G) {
  const int l = blockIdx.y, s = blockIdx.x * LOSS_THREADS + threadIdx.x;
  const int n = w.n[l];
  const long cb = (long)l * A.cap;
  const unsigned* key = w.key[cur] + cb;
  const int cell = segment_head(key, s, n);
  if (cell < 0) return;
  int e = s + 1;
  while (e < n && key[e] == (unsigned)cell) ++e;
  const int* idx = w.idx[cur] + cb;
  const int* cls = w.cls + cb;
  const float* ps = A.p[l] + (long)cell * A.no + 5;
  float* g = G.g[l] + (long)cell * A.no + 5;
  const double gcls = (double)gout[0] * A.B * A.cls / ((double)n * A.nc);
  for (int j = 0; j < A.nc; ++j) {
    double dn, dp;
    bce_focal(ps[j], A.cn, A.cls_pw, A.fl_gamma, nullptr, &dn);
    bce_focal(ps[j], A.cp, A.cls_pw, A.fl_gamma, nullptr, &dp);
    double a = 0.0;
    for (int f = s; f < e; ++f) a += cls[idx[f]] == j ? dp : dn;
    g[j] = (float)(a * gcls);
  }
}

// ---------------------------------------------------------------------------------------------------------------------
// entry points
// ---------------------------------------------------------------------------------------------------------------------
static int loss_args(int nl, const float* const* p, int B, int na, const int* ny, const int* nx, int nc, int nt, const double* hyp,
                     LossArgs* A) {
  CFT_REQUIRE(nl >= 1 && nl <= LOSS_MAX_NL, "cft_loss: nl must be in [1, 5]");
  CFT_REQUIRE(B >= 1 && na >= 1 && nc >= 1 && nc <= 65535, "cft_loss: bad B / na / nc");
  CFT_REQUIRE(nt >= 0 && (long)5 * na * nt < (1L << 30), "cft_loss: 5 * na * nt must be < 2^30");
  CFT_REQUIRE(ny && nx && hyp, "cft_loss: null pointer");
  *A = LossArgs{};
  A->nl = nl; A->B = B; A->na = na; A->nc = nc; A->no = nc + 5; A->nt = nt;
  int maxcells = 0;
  for (int l = 0; l < nl; ++l) {
    CFT_REQUIRE(ny[l] >= 1 && nx[l] >= 1, "cft_loss: empty level");
    const long cells = (long)B * na * ny[l] * nx[l];
    CFT_REQUIRE(cells * (nc + 5) < (1L << 31), "cft_loss: a level has 2^31 elements or more");
    A->p[l] = p ? p[l] : nullptr;
    A->ny[l] = ny[l]; A->nx[l] = nx[l]; A->cells[l] = (int)cells;
    maxcells = std::max(maxcells, (int)cells);
  }
  A->cap = 5 * na * nt;
  A->npb = std::max(1, (na * nt + PAIR_TILE - 1) / PAIR_TILE);
  A->nbc = std::max(1, (A->cap + LOSS_THREADS - 1) / LOSS_THREADS);
  A->nbo = (maxcells + OBJ_TILE - 1) / OBJ_TILE;
  A->anchor_t = (float)hyp[HYP_ANCHOR_T];
  A->box = hyp[HYP_BOX]; A->obj = hyp[HYP_OBJ]; A->cls = hyp[HYP_CLS];
  A->cls_pw = hyp[HYP_CLS_PW]; A->obj_pw = hyp[HYP_OBJ_PW]; A->fl_gamma = hyp[HYP_FL_GAMMA];
  A->cp = (double)(float)hyp[HYP_CP]; A->cn = (double)(float)hyp[HYP_CN];     // torch.full_like / index_put in float32
  A->gr = hyp[HYP_GR];
  return CFT_OK;
}

extern "C" long cft_loss_workspace_bytes(int nl, int B, int na, const int* ny, const int* nx, int nc, int nt) {
  static const double hyp0[HYP_N] = {};
  LossArgs A;
  if (loss_args(nl, nullptr, B, na, ny, nx, nc, nt, hyp0, &A) != CFT_OK) return -1;
  return (long)loss_ws_layout(A, nullptr, nullptr);
}

extern "C" int cft_loss_forward(int nl, const float* const* p, int B, int na, const int* ny, const int* nx, int nc, const float* targets, int nt,
                                const float* anchors, const double* hyp, double* balance, int autobalance, int ssi, void* workspace,
                                long workspace_bytes, float* loss, float* items, int* err, void* stream) {
  LossArgs A;
  int rc = loss_args(nl, p, B, na, ny, nx, nc, nt, hyp, &A);
  if (rc != CFT_OK) return rc;
  CFT_REQUIRE(p && anchors && balance && workspace && loss && items && err && (nt == 0 || targets), "cft_loss_forward: null pointer");
  for (int l = 0; l < nl; ++l) CFT_REQUIRE(p[l], "cft_loss_forward: null level pointer");
  CFT_REQUIRE(ssi >= 0 && ssi < nl, "cft_loss_forward: ssi out of range");
  CFT_REQUIRE(workspace_bytes >= (long)loss_ws_layout(A, nullptr, nullptr), "cft_loss_forward: workspace too small (see cft_loss_workspace_bytes)");
  CFT_REQUIRE(((size_t)workspace & 255) == 0, "cft_loss_forward: workspace must be 256-byte aligned");
  hipStream_t st = as_stream(stream);
  LossWs w;
  loss_ws_layout(A, (char*)workspace, &w);
  int maxcells = 0;
  for (int l = 0; l < nl; ++l) maxcells = std::max(maxcells, A.cells[l]);
  const int gfill = std::min(2048, (maxcells + LOSS_THREADS - 1) / LOSS_THREADS);
  hipLaunchKernelGGL(loss_init_kernel, dim3(gfill, nl), dim3(LOSS_THREADS), 0, st, A, w);
  if ((rc = cft_check_launch("loss_init_kernel")) != CFT_OK) return rc;
  if (nt > 0) {
    hipLaunchKernelGGL(loss_count_kernel, dim3(A.npb, nl), dim3(LOSS_THREADS), 0, st, A, targets, anchors, w, err);
    if ((rc = cft_check_launch("loss_count_kernel")) != CFT_OK) return rc;
  }
  hipLaunchKernelGGL(loss_scan_kernel, dim3(nl), dim3(SCAN_THREADS_L), 0, st, A, w);   // nt = 0: blk is never read, n = 0 below
  if ((rc = cft_check_launch("loss_scan_kernel")) != CFT_OK) return rc;
  if (nt > 0) {
    hipLaunchKernelGGL(loss_scatter_kernel, dim3(A.npb, nl), dim3(LOSS_THREADS), 0, st, A, targets, anchors, w, err);
    if ((rc = cft_check_launch("loss_scatter_kernel")) != CFT_OK) return rc;
  }
  hipLaunchKernelGGL(loss_match_kernel, dim3(A.nbc, nl), dim3(LOSS_THREADS), 0, st, A, anchors, w);
  if ((rc = cft_check_launch("loss_match_kernel")) != CFT_OK) return rc;
  hipLaunchKernelGGL(loss_obj_kernel, dim3(A.nbo, nl), dim3(LOSS_THREADS), 0, st, A, w);
  if ((rc = cft_check_launch("loss_obj_kernel")) != CFT_OK) return rc;
  hipLaunchKernelGGL(loss_finish_kernel, dim3(1), dim3(LOSS_THREADS), 0, st, A, w, balance, autobalance, ssi, loss, items);
  return cft_check_launch("loss_finish_kernel");
}

extern "C" int cft_loss_backward(int nl, const float* const* p, int B, int na, const int* ny, const int* nx, int nc, int nt, const float* anchors,
                                 const double* hyp, const float* grad_loss, float* const* grad, void* workspace, long workspace_bytes,
                                 void* stream) {
  LossArgs A;
  int rc = loss_args(nl, p, B, na, ny, nx, nc, nt, hyp, &A);
  if (rc != CFT_OK) return rc;
  CFT_REQUIRE(p && anchors && grad_loss && grad && workspace, "cft_loss_backward: null pointer");
  for (int l = 0; l < nl; ++l) CFT_REQUIRE(p[l] && grad[l], "cft_loss_backward: null level pointer");
  CFT_REQUIRE(workspace_bytes >= (long)loss_ws_layout(A, nullptr, nullptr), "cft_loss_backward: workspace too small (see cft_loss_workspace_bytes)");
  CFT_REQUIRE(((size_t)workspace & 255) == 0, "cft_loss_backward: workspace must be 256-byte aligned");
  hipStream_t st = as_stream(stream);
  LossWs w;
  loss_ws_layout(A, (char*)workspace, &w);
  LossGrads g = {};
  long maxel = 0;
  int maxcells = 0;
  for (int l = 0; l < nl; ++l) {
    g.g[l] = grad[l];
    maxel = std::max(maxel, (long)A.cells[l] * A.no);
    maxcells = std::max(maxcells, A.cells[l]);
  }
  const int gd = (int)std::min<long>(65536, (maxel + LOSS_THREADS - 1) / LOSS_THREADS);
  hipLaunchKernelGGL(loss_grad_dense_kernel, dim3(gd, nl), dim3(LOSS_THREADS), 0, st, A, w, grad_loss, g);
  if ((rc = cft_check_launch("loss_grad_dense_kernel")) != CFT_OK) return rc;
  if (nt == 0) return CFT_OK;
  // stable LSD radix sort of each level's candidates by cell, over as many 8-bit digits as the largest cell index needs
  const int nbs = lsort_blocks(A.cap);
  hipLaunchKernelGGL(lsort_init_kernel, dim3(A.nbc, nl), dim3(LOSS_THREADS), 0, st, A, w);
  if ((rc = cft_check_launch("lsort_init_kernel")) != CFT_OK) return rc;
  int cur = 0;
  for (int shift = 0; shift < 32 && ((unsigned)(maxcells - 1) >> shift) > 0u; shift += 8) {
    hipLaunchKernelGGL(lsort_hist_kernel, dim3(nbs, nl), dim3(LOSS_THREADS), 0, st, A, w, cur, shift, nbs);
    if ((rc = cft_check_launch("lsort_hist_kernel")) != CFT_OK) return rc;
    hipLaunchKernelGGL(lsort_scan_kernel, dim3(nl), dim3(SCAN_THREADS_L), 0, st, w, nbs);
    if ((rc = cft_check_launch("lsort_scan_kernel")) != CFT_OK) return rc;
    hipLaunchKernelGGL(lsort_scatter_kernel, dim3(nbs, nl), dim3(LOSS_THREADS), 0, st, A, w, cur, shift, nbs);
    if ((rc = cft_check_launch("lsort_scatter_kernel")) != CFT_OK) return rc;
    cur ^= 1;
  }
  hipLaunchKernelGGL(loss_grad_box_kernel, dim3(A.nbc, nl), dim3(LOSS_THREADS), 0, st, A, anchors, w, cur, grad_loss, g);
  if ((rc = cft_check_launch("loss_grad_box_kernel")) != CFT_OK) return rc;
  if (nc == 1) return CFT_OK;
  hipLaunchKernelGGL(loss_grad_cls_kernel, dim3(A.nbc, nl), dim3(LOSS_THREADS), 0, st, A, w, cur, grad_loss, g);
  return cft_check_launch("loss_grad_cls_kernel");
}

// byte offsets into the workspace of the candidate lists the last forward left there (build_targets' output, for inspection):
// out[0] cell int [nl][cap], out[1] class int [nl][cap], out[2] tbox float4 [nl][cap], out[3] counts int [nl]; returns cap
extern "C" long cft_loss_workspace_offsets(int nl, int B, int na, const int* ny, const int* nx, int nc, int nt, long* out) {
  static const double hyp0[HYP_N] = {};
  LossArgs A;
  if (!out || loss_args(nl, nullptr, B, na, ny, nx, nc, nt, hyp0, &A) != CFT_OK) return -1;
  alignas(256) static char probe[1];      // any base: only differences are used
  LossWs w;
  loss_ws_layout(A, probe, &w);
  out[0] = (long)((char*)w.cell - probe);
  out[1] = (long)((char*)w.cls - probe);
  out[2] = (long)((char*)w.tbox - probe);
  out[3] = (long)((char*)w.n - probe);
  return A.cap;
}
