// mAP statistics of the reference's test.py on the GPU (the step after batched NMS):
//   cft_eval_match  the per-image matching of detections to labels (test.py:132-218), one workgroup per image;
//   cft_eval_ap     ap_per_class (utils/metrics.py:18-108) over all accumulated statistics;
// (cft_eval_confusion and cft_eval_export are in confusion.hip; what both files share is in metrics_common.h.)
// Every rule follows the reference line by line; the numerics are float32 where the reference computes on tensors
// (box transforms, IoU) and float64 where it computes in numpy (curves, AP).  No float atomics anywhere: every
// result is the same run to run.
#include "metrics_common.h"

#pragma clang fp contract(off)   // the reference's float ops are separate roundings: no fused multiply-adds here

constexpr int EVAL_MAX_IOU = 16;
struct IouV { float v[EVAL_MAX_IOU]; };

// ---------------------------------------------------------------------------------------------------------------------
// (a) matching
// ---------------------------------------------------------------------------------------------------------------------
// Stable grouping of the labels by image (one workgroup per image): image b's labels keep their order in `targets` and
// land at [off[b], off[b] + cnt[b]) of the workspace, transformed to native-space xyxy (test.py:136, :201-202).  Also adds the
// image's labels to the class histogram (slot nc counts labels whose class is not an integer in [0, nc)).  `key` (optional)
// is the per-label selection word of cft_eval_confusion, cleared here.
__global__ void __launch_bounds__(MATCH_THREADS) eval_group_kernel(const float* __restrict__ targets, int nt, int B, float img_h, float img_w,
                                                                   const float* __restrict__ geom, MatchWs ws, int* __restrict__ label_hist,
                                                                   int nc, int* __restrict__ tcls_out, int* __restrict__ nl_out, int mode,
                                                                   unsigned long long* __restrict__ key) {
  __shared__ int s_w[MATCH_THREADS / 64];
  const int b = blockIdx.x, tid = threadIdx.x;
  int before = 0, mine = 0;
  for (int i = tid; i < nt; i += MATCH_THREADS) {
    const int im = label_image(targets[(long)i * 6], B);
    before += (im >= 0 && im < b) ? 1 : 0;
    mine += im == b ? 1 : 0;
  }
  int tb, tm;
  block_excl_scan(before, s_w, &tb);
  block_excl_scan(mine, s_w, &tm);
  if (tid == 0) { ws.off[b] = tb; ws.cnt[b] = tm; if (nl_out) nl_out[b] = tm; }
  const Geom g = (mode & GROUP_NATIVE) ? Geom{0.f, 0.f, 1.f, 0.f, 0.f} : load_geom(geom, b);
  int run = 0;
  for (int i0 = 0; i0 < nt; i0 += MATCH_THREADS) {
    const int i = i0 + tid;
    const bool own = i < nt && label_image(targets[(long)i * 6], B) == b;
    int tot;
    const int rank = block_excl_scan(own ? 1 : 0, s_w, &tot);
    if (own) {
      const float* t = targets + (long)i * 6;
      const int pos = tb + run + rank;
      // targets[:, 2:] *= [W, H, W, H] (test.py:125), xywh2xyxy (utils/general.py:299-306), scale_coords
      if (mode & GROUP_NATIVE) {
        ws.box[pos] = make_float4(t[2], t[3], t[4], t[5]);
      } else {
        const float x = t[2] * img_w, y = t[3] * img_h, w = t[4] * img_w, h = t[5] * img_h;
        ws.box[pos] = scale_box(x - w / 2.f, y - h / 2.f, x + w / 2.f, y + h / 2.f, g);
      }
      const float cf = t[1];
      const int c = (mode & GROUP_TRUNC_CLS) ? trunc_class(cf) : ((cf >= 0.f && cf < 2147483520.f && (float)(int)cf == cf) ? (int)cf : -1);
      if (key) key[pos] = 0ull;
      ws.cls[pos] = c;
      ws.win[pos] = 0x7fffffff;
      if (tcls_out) tcls_out[pos] = c;
      if (label_hist) atomicAdd(&label_hist[(c >= 0 && c < nc) ? c : nc], 1);     // integer counts: deterministic
    }
    run += tot;
  }
}

// Best label of the prediction's class (test.py:207 `box_iou(...).max(1)`): first index on ties, a NaN wins like torch.max.
__device__ __forceinline__ void best_label(const float4& p, int pc, int nl, const float4* lbox, const int* lcls, float* best_iou, int* best) {
  const float pa = (p.z - p.x) * (p.w - p.y);
  float bi = 0.f;
  int bl = -1;
  for (int l = 0; l < nl; ++l) {
    if (lcls[l] != pc) continue;
    const float v = box_iou1(p, pa, lbox[l]);
    if (bl < 0 || !(v <= bi)) {
      bi = v; bl = l;
      if (v != v) break;
    }
  }
  *best_iou = bi;
  *best = bl;
}

// One workgroup per image.  Per class with labels each prediction takes its best label if that IoU > iouv[0] and no earlier row
// (test.py:211 walks rows in order) took the same label; a prediction whose best label is taken stays unmatched (the reference
// does not fall back to its second best).  Classes are independent (a label has one class), and `len(detected) == nl` (:217)
// only fires when every label is taken already.  So "row r takes label l" <=> r is the lowest qualifying row whose best is l:
// an integer atomicMin per label, then every row checks whether it won.
__global__ void __launch_bounds__(MATCH_THREADS) eval_match_kernel(const float* __restrict__ dets, const int* __restrict__ counts, int max_det,
                                                                   const float* __restrict__ geom, IouV iouv, int niou, int single_cls,
                                                                   MatchWs ws, unsigned char* __restrict__ correct, unsigned short* __restrict__ tp_bits,
                                                                   float* __restrict__ conf_out, int* __restrict__ pcls_out) {
  __shared__ float4 s_box[MATCH_LDS_LABELS];
  __shared__ int s_cls[MATCH_LDS_LABELS], s_win[MATCH_LDS_LABELS];
  const int b = blockIdx.x, tid = threadIdx.x;
  const int nl = ws.cnt[b], l0 = ws.off[b];
  int n = counts[b];
  n = n < 0 ? 0 : (n > max_det ? max_det : n);
  const bool in_lds = nl <= MATCH_LDS_LABELS;
  const float4* lbox = in_lds ? s_box : ws.box + l0;
  const int* lcls = in_lds ? s_cls : ws.cls + l0;
  int* lwin = in_lds ? s_win : ws.win + l0;
  if (in_lds) {
    for (int l = tid; l < nl; l += MATCH_THREADS) { s_box[l] = ws.box[l0 + l]; s_cls[l] = ws.cls[l0 + l]; s_win[l] = 0x7fffffff; }
  }
  __syncthreads();
  const Geom g = load_geom(geom, b);
  const float* D = dets + (long)b * max_det * 6;
  const float thr0 = iouv.v[0];
  for (int r = tid; r < n; r += MATCH_THREADS) {
    const float* d = D + (long)r * 6;
    const int pc = single_cls ? 0 : (int)d[5];
    const float4 p = scale_box(d[0], d[1], d[2], d[3], g);     // predn (test.py:148-149)
    float bi;
    int bl;
    best_label(p, pc, nl, lbox, lcls, &bi, &bl);
    if (bl >= 0 && bi > thr0) atomicMin(&lwin[bl], r);
  }
  __syncthreads();
  __threadfence_block();
  for (int r = tid; r < max_det; r += MATCH_THREADS) {
    const long o = (long)b * max_det + r;
    unsigned bits = 0u;
    float cf = 0.f;
    int pc = -1;
    if (r < n) {
      const float* d = D + (long)r * 6;
      pc = single_cls ? 0 : (int)d[5];
      cf = d[4];
      const float4 p = scale_box(d[0], d[1], d[2], d[3], g);
      float bi;
      int bl;
      best_label(p, pc, nl, lbox, lcls, &bi, &bl);
      if (bl >= 0 && bi > thr0 && lwin[bl] == r)
        for (int k = 0; k < niou; ++k) bits |= (bi > iouv.v[k] ? 1u : 0u) << k;     // correct[pi[j]] = ious[j] > iouv (:214)
    }
    tp_bits[o] = (unsigned short)bits;
    if (conf_out) conf_out[o] = cf;
    if (pcls_out) pcls_out[o] = pc;
    if (correct)
      for (int k = 0; k < niou; ++k) correct[o * niou + k] = (unsigned char)((bits >> k) & 1u);
  }
}

int eval_group_launch(const float* targets, int nt, int B, float img_h, float img_w, const float* geom, MatchWs ws, int* label_hist, int nc,
                      int* tcls, int* nl, int mode, unsigned long long* key, hipStream_t stream) {
  hipLaunchKernelGGL(eval_group_kernel, dim3(B), dim3(MATCH_THREADS), 0, stream, targets, nt, B, img_h, img_w, geom, ws, label_hist, nc, tcls, nl,
                     mode, key);
  return cft_check_launch("eval_group_kernel");
}

extern "C" long cft_eval_match_workspace_bytes(int B, int nt) {
  if (B <= 0 || nt < 0) return -1;
  return (long)match_ws_layout(B, nt, nullptr, nullptr);
}

extern "C" int cft_eval_match(const float* dets, const int* counts, int B, int max_det, const float* targets, int nt, int img_h, int img_w,
                              const float* geom, const float* iouv_host, int niou, int single_cls, void* workspace, long workspace_bytes,
                              unsigned char* correct, unsigned short* tp_bits, float* conf, int* pcls, int* label_hist, int nc,
                              int* tcls, int* nl, void* stream) {
  CFT_REQUIRE(dets && counts && geom && iouv_host && workspace && tp_bits, "cft_eval_match: null pointer");
  CFT_REQUIRE(B > 0 && max_det > 0 && nt >= 0 && (nt == 0 || targets) && img_h > 0 && img_w > 0, "cft_eval_match: bad shape");
  CFT_REQUIRE(niou >= 1 && niou <= EVAL_MAX_IOU, "cft_eval_match: niou must be in [1, 16]");
  CFT_REQUIRE((long)B * max_det < (1L << 31) && (long)nt * 6 < (1L << 31), "cft_eval_match: too many detections or labels");
  CFT_REQUIRE(label_hist == nullptr || nc >= 0, "cft_eval_match: bad nc");
  CFT_REQUIRE(workspace_bytes >= (long)match_ws_layout(B, nt, nullptr, nullptr), "cft_eval_match: workspace too small (see cft_eval_match_workspace_bytes)");
  CFT_REQUIRE(((size_t)workspace & 255) == 0, "cft_eval_match: workspace must be 256-byte aligned");
  IouV iv;
  for (int k = 0; k < EVAL_MAX_IOU; ++k) iv.v[k] = k < niou ? iouv_host[k] : 2.f;
  MatchWs w;
  match_ws_layout(B, nt, (char*)workspace, &w);
  int st = eval_group_launch(targets, nt, B, (float)img_h, (float)img_w, geom, w, label_hist, nc, tcls, nl, 0, nullptr, as_stream(stream));
  if (st != CFT_OK) return st;
  hipLaunchKernelGGL(eval_match_kernel, dim3(B), dim3(MATCH_THREADS), 0, as_stream(stream), dets, counts, max_det, geom, iv, niou, single_cls, w,
                     correct, tp_bits, conf, pcls);
  return cft_check_launch("eval_match_kernel");
}

// ---------------------------------------------------------------------------------------------------------------------
// (b) ap_per_class
// ---------------------------------------------------------------------------------------------------------------------
constexpr int SCAN_THREADS = 1024;
constexpr int NX = 101;                                   // np.linspace(0, 1, 101) (utils/metrics.py:97)

// conf -> key whose ascending order is descending conf (-0.0 folded onto +0.0, as np.argsort(-conf) sees them equal)
__device__ __forceinline__ unsigned conf_key_desc(float c) {
  unsigned u = __float_as_uint(c);
  if (u == 0x80000000u) u = 0u;
  const unsigned asc = (u & 0x80000000u) ? ~u : (u | 0x80000000u);
  return ~asc;
}

__global__ void __launch_bounds__(SORT_THREADS) ap_init_kernel(const float* __restrict__ conf, int n, unsigned* __restrict__ key, int* __restrict__ idx,
                                                               int* __restrict__ seg, int nseg) {
  const int i = blockIdx.x * SORT_THREADS + threadIdx.x;
  if (i < n) { key[i] = conf_key_desc(conf[i]); idx[i] = i; }
  if (i < nseg) seg[i] = 0;
}

// class of the element in sorted position i (the payload idx): its class if it has labels, else nc (dropped, sorts last)
__global__ void __launch_bounds__(SORT_THREADS) ap_classkey_kernel(const int* __restrict__ pcls, const int* __restrict__ label_hist, int nc, int n,
                                                                   const int* __restrict__ idx, unsigned* __restrict__ key) {
  const int i = blockIdx.x * SORT_THREADS + threadIdx.x;
  if (i >= n) return;
  const int c = pcls[idx[i]];
  key[i] = (c >= 0 && c < nc && label_hist[c] > 0) ? (unsigned)c : (unsigned)nc;
}

__global__ void __launch_bounds__(SORT_THREADS) radix_hist_kernel(const unsigned* __restrict__ key, int n, int shift, int nblk, unsigned* __restrict__ hist) {
  __shared__ unsigned s_h[256];
  const int tid = threadIdx.x, blk = blockIdx.x;
  s_h[tid] = 0u;
  __syncthreads();
  const long base = (long)blk * SORT_TILE;
  for (int k = 0; k < SORT_ITEMS; ++k) {
    const long i = base + (long)k * SORT_THREADS + tid;
    if (i < n) atomicAdd(&s_h[(key[i] >> shift) & 255u], 1u);
  }
  __syncthreads();
  hist[(long)tid * nblk + blk] = s_h[tid];
}

// Exclusive scan of the m = 256 * nblk digit-major counts, in place, by one workgroup.
__global__ void __launch_bounds__(SCAN_THREADS) radix_scan_kernel(unsigned* __restrict__ hist, int m) {
  __shared__ unsigned s_part[SCAN_THREADS];
  const int tid = threadIdx.x;
  const int per = (m + SCAN_THREADS - 1) / SCAN_THREADS;
  const int a = tid * per, e = min(a + per, m);
  unsigned s = 0u;
  for (int i = a; i < e; ++i) s += hist[i];
  s_part[tid] = s;
  __syncthreads();
  if (tid == 0) {
    unsigned run = 0u;
    for (int t = 0; t < SCAN_THREADS; ++t) { const unsigned v = s_part[t]; s_part[t] = run; run += v; }
  }
  __syncthreads();
  unsigned run = s_part[tid];
  for (int i = a; i < e; ++i) { const unsigned v = hist[i]; hist[i] = run; run += v; }
}

// Stable scatter of one 8-bit digit: the tile is walked in order, 256 elements at a time; within a wave an element's rank among
// equal digits comes from ballots (peers = lanes with the same digit), waves are ordered through LDS counts.
__global__ void __launch_bounds__(SORT_THREADS) radix_scatter_kernel(const unsigned* __restrict__ key_in, const int* __restrict__ idx_in,
                                                                     unsigned* __restrict__ key_out, int* __restrict__ idx_out, int n, int shift,
                                                                     int nblk, const unsigned* __restrict__ hist) {
  constexpr int NW = SORT_THREADS / 64;
  __shared__ unsigned s_base[256];
  __shared__ unsigned s_wc[NW][256];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, blk = blockIdx.x;
  s_base[tid] = hist[(long)tid * nblk + blk];
  const unsigned long long lt = (1ull << lane) - 1ull;
  const long base = (long)blk * SORT_TILE;
  for (int k = 0; k < SORT_ITEMS; ++k) {
    const long i = base + (long)k * SORT_THREADS + tid;
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
    for (int w = 0; w < NW; ++w) s_wc[w][tid] = 0u;
    __syncthreads();
    if (valid && rank == 0u) s_wc[wave][d] = (unsigned)__popcll(peers);
    __syncthreads();
    {
      unsigned run = s_base[tid];
#pragma unroll
      for (int w = 0; w < NW; ++w) { const unsigned c = s_wc[w][tid]; s_wc[w][tid] = run; run += c; }
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

// seg[2c] / seg[2c+1] = start / end of class c in the sorted order (left 0 / 0 for a class without predictions)
__global__ void __launch_bounds__(SORT_THREADS) ap_segments_kernel(const unsigned* __restrict__ key, int n, int nc, int* __restrict__ seg) {
  const int i = blockIdx.x * SORT_THREADS + threadIdx.x;
  if (i >= n) return;
  const unsigned c = key[i];
  if (c >= (unsigned)nc) return;
  if (i == 0 || key[i - 1] != c) seg[2 * c] = i;
  if (i == n - 1 || key[i + 1] != c) seg[2 * c + 1] = i + 1;
}

// numpy's add.reduce of a contiguous float64 vector of 9 <= len <= 128 elements: the first element plus the pairwise sum (eight
// accumulators, then the remainder in order) of the rest.  Reads LDS.
__device__ double np_sum_small(const double* a, int len) {
  const double* b = a + 1;
  const int m = len - 1;
  double r0 = b[0], r1 = b[1], r2 = b[2], r3 = b[3], r4 = b[4], r5 = b[5], r6 = b[6], r7 = b[7];
  int i = 8;
  for (; i < m - (m % 8); i += 8) {
    r0 += b[i]; r1 += b[i + 1]; r2 += b[i + 2]; r3 += b[i + 3];
    r4 += b[i + 4]; r5 += b[i + 5]; r6 += b[i + 6]; r7 += b[i + 7];
  }
  double res = ((r0 + r1) + (r2 + r3)) + ((r4 + r5) + (r6 + r7));
  for (; i < m; ++i) res += b[i];
  return a[0] + res;
}

// One workgroup per (class c, IoU column j) of a class with labels (utils/metrics.py:42-66, compute_ap :74-101).  The class's
// predictions are walked from the last (lowest conf) to the first, 256 at a time: exact integer TP counts from the end, the
// precision envelope of compute_ap (a reverse running max) as a running max, and every node of mrec writes the values of the
// 101-point np.interp that fall between it and the next node.  Column 0 also writes the p / r curves at the 1000 px points
// (np.interp(-px, -conf, .), :57 and :61) the same way.
__global__ void __launch_bounds__(CURVE_THREADS) ap_curve_kernel(const unsigned short* __restrict__ tp_bits, const float* __restrict__ conf,
                                                                 const int* __restrict__ idx, const int* __restrict__ seg,
                                                                 const int* __restrict__ label_hist, int niou, const double* __restrict__ px_g,
                                                                 const double* __restrict__ x_g, double* __restrict__ pcurve, double* __restrict__ rcurve,
                                                                 double* __restrict__ ap_out, double* __restrict__ ntp_out) {
  __shared__ double s_px[NPX], s_x[NX], s_y[NX];
  __shared__ int s_w[CURVE_THREADS / 64];
  __shared__ double s_max[CURVE_THREADS], s_rec[CURVE_THREADS], s_env[CURVE_THREADS], s_prec[CURVE_THREADS], s_cf[CURVE_THREADS];
  __shared__ double s_carry[4];     // recall (mrec), envelope, precision, conf of the node after the current chunk
  const int c = blockIdx.x, j = blockIdx.y, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int nl = label_hist[c];
  const bool curves = j == 0;
  if (nl <= 0) {                                    // not a class of np.unique(target_cls): no row
    if (tid == 0) { ap_out[(long)c * niou + j] = 0.0; if (curves) ntp_out[c] = 0.0; }
    return;
  }
  const int s = seg[2 * c], np_ = seg[2 * c + 1] - s;
  double* P = pcurve + (long)c * NPX;
  double* R = rcurve + (long)c * NPX;
  if (np_ <= 0) {                                   // labels but no predictions: rows of zeros (:47-48)
    if (tid == 0) { ap_out[(long)c * niou + j] = 0.0; if (curves) ntp_out[c] = 0.0; }
    if (curves) for (int i = tid; i < NPX; i += CURVE_THREADS) { P[i] = 0.0; R[i] = 0.0; }
    return;
  }
  for (int i = tid; i < NPX; i += CURVE_THREADS) s_px[i] = px_g[i];
  for (int i = tid; i < NX; i += CURVE_THREADS) s_x[i] = x_g[i];
  // total TP of column j in the class
  int cnt = 0;
  for (int k = tid; k < np_; k += CURVE_THREADS) cnt += (tp_bits[idx[s + k]] >> j) & 1;
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) cnt += __shfl_xor(cnt, o);
  if (lane == 0) s_w[wave] = cnt;
  __syncthreads();
  int T = 0;
  for (int w = 0; w < CURVE_THREADS / 64; ++w) T += s_w[w];
  const double denom = (double)nl + 1e-16;           // n_l + 1e-16 (:55)
  if (tid == 0) {                                    // compute_ap's end sentinel: mrec = recall[-1] + 0.01, mpre = 0 (:88-89)
    s_carry[0] = (double)T / denom + 0.01;
    s_carry[1] = 0.0;
    s_carry[2] = 0.0;
    s_carry[3] = 0.0;
    if (curves) ntp_out[c] = (double)T;
  }
  __syncthreads();
  int after = 0;                                     // TPs at positions after the current chunk
  for (int hi = np_; hi > 0; hi -= CURVE_THREADS) {
    const int k = hi - 1 - tid;                      // thread 0 holds the last element of the chunk
    const bool valid = k >= 0;
    const int i0 = valid ? idx[s + k] : 0;
    const unsigned bit = valid ? ((tp_bits[i0] >> j) & 1u) : 0u;
    const double cf = valid ? (double)conf[i0] : 0.0;
    int tot;
    const int excl = block_excl_scan((int)bit, s_w, &tot);
    const int tpc = T - (after + excl);              // tp.cumsum(0) at k, an exact integer
    const double rec = (double)tpc / denom;
    const double prec = (double)tpc / (double)(k + 1);   // tpc / (tpc + fpc) with fpc = (1 - tp).cumsum(0) = k + 1 - tpc
    // running max of the precision from the chunk's end (thread 0) down to this element, then with everything after the chunk
    s_max[tid] = valid ? prec : 0.0;
    __syncthreads();
    for (int o = 1; o < CURVE_THREADS; o <<= 1) {
      const double v = tid >= o ? s_max[tid - o] : 0.0;
      __syncthreads();
      if (tid >= o) s_max[tid] = fmax(s_max[tid], v);
      __syncthreads();
    }
    const double env = fmax(s_max[tid], s_carry[1]);
    s_rec[tid] = rec; s_env[tid] = env; s_prec[tid] = prec; s_cf[tid] = cf;
    __syncthreads();
    // the next node: element k + 1 (thread tid - 1), or the node carried from after the chunk
    const double nrec = tid == 0 ? s_carry[0] : s_rec[tid - 1];
    const double nenv = tid == 0 ? s_carry[1] : s_env[tid - 1];
    const double nprec = tid == 0 ? s_carry[2] : s_prec[tid - 1];
    const double ncf = tid == 0 ? s_carry[3] : s_cf[tid - 1];
    const bool last = k == np_ - 1;
    if (valid) {
      // compute_ap: this element's mrec node owns the grid points in [mrec, next mrec)
      const int qa = grid_bound(s_x, NX, rec, false), qb = grid_bound(s_x, NX, nrec, false);
      for (int q = qa; q < qb; ++q) s_y[q] = np_interp_seg(s_x[q], rec, env, nrec, nenv);
      if (last)                                      // the end sentinel owns the rest: mpre there is 0
        for (int q = qb; q < NX; ++q) s_y[q] = 0.0;
      if (curves) {
        // p / r at px (xp = -conf ascending, x = -px): element k owns conf[k+1] < px <= conf[k]; the last one owns px <= conf[k]
        const int ia = last ? 0 : grid_bound(s_px, NPX, ncf, true), ib = grid_bound(s_px, NPX, cf, true);
        for (int i = ia; i < ib; ++i) {
          if (last) { R[i] = rec; P[i] = prec; continue; }
          const double xq = -s_px[i];
          R[i] = np_interp_seg(xq, -cf, rec, -ncf, nrec);
          P[i] = np_interp_seg(xq, -cf, prec, -ncf, nprec);
        }
      }
    }
    __syncthreads();
    const int first = hi - CURVE_THREADS >= 0 ? CURVE_THREADS - 1 : hi - 1;     // the thread holding the chunk's lowest k
    if (tid == first) { s_carry[0] = rec; s_carry[1] = env; s_carry[2] = prec; s_carry[3] = cf; }
    after += tot;
    __syncthreads();
  }
  // compute_ap's start sentinel (mrec = 0, mpre = max(1, ...) = 1) owns [0, recall[0])
  if (tid == 0) {
    const int qb = grid_bound(s_x, NX, s_carry[0], false);
    for (int q = 0; q < qb; ++q) s_y[q] = np_interp_seg(s_x[q], 0.0, 1.0, s_carry[0], s_carry[1]);
  }
  if (curves) {                                      // px above the highest conf: np.interp's left values, r = 0 and p = 1
    const int ia = grid_bound(s_px, NPX, s_carry[3], true);
    for (int i = ia + tid; i < NPX; i += CURVE_THREADS) { R[i] = 0.0; P[i] = 1.0; }
  }
  __syncthreads();
  // np.trapz(y, x) = add.reduce(diff(x) * (y[1:] + y[:-1]) / 2.0) (:98)
  if (tid < NX - 1) s_max[tid] = (s_x[tid + 1] - s_x[tid]) * (s_y[tid + 1] + s_y[tid]) / 2.0;
  __syncthreads();
  if (tid == 0) ap_out[(long)c * niou + j] = np_sum_small(s_max, NX - 1);
}

// f1 = 2 p r / (p + r + 1e-16) over the classes with labels, the argmax of its mean over classes (numpy: rows summed in class
// order, first index on ties), and p, r, f1 at that index (utils/metrics.py:69-79).  One workgroup of 1024 threads.
__global__ void __launch_bounds__(1024) ap_f1_kernel(const int* __restrict__ label_hist, int nc, const double* __restrict__ pcurve,
                                                     const double* __restrict__ rcurve, double* __restrict__ p_out, double* __restrict__ r_out,
                                                     double* __restrict__ f1_out) {
  __shared__ double s_v[16];
  __shared__ int s_i[16];
  __shared__ int s_best;
  const int tid = threadIdx.x;
  const int i = f1_best_index(label_hist, nc, pcurve, rcurve, s_v, s_i, &s_best);
  for (int c = tid; c < nc; c += 1024) {
    if (label_hist[c] <= 0) { p_out[c] = 0.0; r_out[c] = 0.0; f1_out[c] = 0.0; continue; }
    const double p = pcurve[(long)c * NPX + i], r = rcurve[(long)c * NPX + i];
    p_out[c] = p; r_out[c] = r; f1_out[c] = 2.0 * p * r / (p + r + 1e-16);
  }
}

extern "C" long cft_eval_ap_workspace_bytes(long n, int nc) {
  if (n < 0 || nc <= 0) return -1;
  return (long)ap_ws_layout(n, nc, nullptr, nullptr);
}

// The sort of cft_eval_ap, also run by cft_eval_curves (curves.hip); the contract is at its declaration in metrics_common.h.
int eval_sort_launch(const float* conf, const int* pcls, long n, const int* label_hist, int nc, const ApWs& w, int* cur_out, hipStream_t st) {
  const int nn = (int)n, nblk = sort_blocks(n), nseg = 2 * (nc + 1);
  const int gi = (int)((std::max<long>(n, nseg) + SORT_THREADS - 1) / SORT_THREADS);
  int cur = 0;
  hipLaunchKernelGGL(ap_init_kernel, dim3(gi), dim3(SORT_THREADS), 0, st, conf, nn, w.key[0], w.idx[0], w.seg, nseg);
  int rc = cft_check_launch("ap_init_kernel");
  if (rc != CFT_OK) return rc;
  // stable LSD radix sort: four 8-bit passes over the conf key (descending conf), then the class (ascending), so each class's
  // predictions end up contiguous, by descending conf, ties in insertion order
  auto pass = [&](int shift) -> int {
    hipLaunchKernelGGL(radix_hist_kernel, dim3(nblk), dim3(SORT_THREADS), 0, st, w.key[cur], nn, shift, nblk, w.hist);
    int r = cft_check_launch("radix_hist_kernel");
    if (r != CFT_OK) return r;
    hipLaunchKernelGGL(radix_scan_kernel, dim3(1), dim3(SCAN_THREADS), 0, st, w.hist, 256 * nblk);
    r = cft_check_launch("radix_scan_kernel");
    if (r != CFT_OK) return r;
    hipLaunchKernelGGL(radix_scatter_kernel, dim3(nblk), dim3(SORT_THREADS), 0, st, w.key[cur], w.idx[cur], w.key[cur ^ 1], w.idx[cur ^ 1], nn, shift,
                       nblk, w.hist);
    cur ^= 1;
    return cft_check_launch("radix_scatter_kernel");
  };
  if (n > 0) {
    for (int shift = 0; shift < 32; shift += 8)
      if ((rc = pass(shift)) != CFT_OK) return rc;
    hipLaunchKernelGGL(ap_classkey_kernel, dim3(nblk * SORT_ITEMS), dim3(SORT_THREADS), 0, st, pcls, label_hist, nc, nn, w.idx[cur], w.key[cur]);
    if ((rc = cft_check_launch("ap_classkey_kernel")) != CFT_OK) return rc;
    for (int shift = 0; shift < 16 && (nc >> shift) > 0; shift += 8)
      if ((rc = pass(shift)) != CFT_OK) return rc;
    hipLaunchKernelGGL(ap_segments_kernel, dim3(nblk * SORT_ITEMS), dim3(SORT_THREADS), 0, st, w.key[cur], nn, nc, w.seg);
    if ((rc = cft_check_launch("ap_segments_kernel")) != CFT_OK) return rc;
  }
  *cur_out = cur;
  return CFT_OK;
}

extern "C" int cft_eval_ap(const unsigned short* tp_bits, const float* conf, const int* pcls, long n, int niou, const int* label_hist, int nc,
                           const double* px, const double* x, void* workspace, long workspace_bytes, double* out, void* stream) {
  CFT_REQUIRE(label_hist && px && x && workspace && out, "cft_eval_ap: null pointer");
  CFT_REQUIRE(n >= 0 && n < (1L << 30) && (n == 0 || (tp_bits && conf && pcls)), "cft_eval_ap: bad n (0 <= n < 2^30)");
  CFT_REQUIRE(niou >= 1 && niou <= EVAL_MAX_IOU, "cft_eval_ap: niou must be in [1, 16]");
  CFT_REQUIRE(nc >= 1 && nc <= 65535, "cft_eval_ap: nc must be in [1, 65535]");
  CFT_REQUIRE(workspace_bytes >= (long)ap_ws_layout(n, nc, nullptr, nullptr), "cft_eval_ap: workspace too small (see cft_eval_ap_workspace_bytes)");
  CFT_REQUIRE(((size_t)workspace & 255) == 0, "cft_eval_ap: workspace must be 256-byte aligned");
  hipStream_t st = as_stream(stream);
  ApWs w;
  ap_ws_layout(n, nc, (char*)workspace, &w);
  int cur = 0;
  int rc = eval_sort_launch(conf, pcls, n, label_hist, nc, w, &cur, st);
  if (rc != CFT_OK) return rc;
  // out = [p nc | r nc | f1 nc | ntp nc | ap nc * niou]
  double* p_out = out;
  double* r_out = out + nc;
  double* f1_out = out + 2L * nc;
  double* ntp_out = out + 3L * nc;
  double* ap_out = out + 4L * nc;
  hipLaunchKernelGGL(ap_curve_kernel, dim3(nc, niou), dim3(CURVE_THREADS), 0, st, tp_bits, conf, w.idx[cur], w.seg, label_hist, niou, px, x, w.pcurve,
                     w.rcurve, ap_out, ntp_out);
  if ((rc = cft_check_launch("ap_curve_kernel")) != CFT_OK) return rc;
  hipLaunchKernelGGL(ap_f1_kernel, dim3(1), dim3(1024), 0, st, label_hist, nc, w.pcurve, w.rcurve, p_out, r_out, f1_out);
  return cft_check_launch("ap_f1_kernel");
}
