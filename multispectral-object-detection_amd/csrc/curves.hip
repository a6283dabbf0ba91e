// The curves of a validation run on the GPU, over the statistics that cft_eval_match accumulated:
//   cft_eval_curves  p / r / f1 at the 1000 px points for every class (utils/metrics.py:57, :61, :70: what `test.py --plots` draws as
//                    P_curve, R_curve and F1_curve), the PR curve np.interp(px, mrec, mpre) at IoU 0.5 (:67, PR_curve), the index of
//                    f1.mean(0).argmax() (:77), and the miss rate at every value of an FPPI grid (the MR-FPPI curve behind the
//                    log-average miss rate; include/cft_hip.h defines it, the reference ships no code for it).
// The sort is cft_eval_ap's (eval_sort_launch, metrics.hip); the walk is the one of ap_curve_kernel: each class's predictions from
// the last (lowest conf) to the first, 256 at a time, exact integer TP counts, and every element writes the grid points it owns.
// Plain loads and stores, no atomics; every output element is written exactly once, so two runs give the same bits.
#include "metrics_common.h"

#pragma clang fp contract(off)   // numpy's float64 ops are separate roundings: no fused multiply-adds here

constexpr int CURVES_MAX_GRID = 4096;

// One workgroup per class.  Element k (0 = highest conf) of a class with n_l labels has tpc = TPs of IoU column 0 among the first
// k + 1, fpc = k + 1 - tpc, recall tpc / (n_l + 1e-16), precision tpc / (k + 1), fppi fpc / n_images and miss 1 - recall.
//   p, r   : element k owns the px with conf[k+1] < px <= conf[k] (np.interp(-px, -conf, .)); the last one owns px <= conf[k];
//            px above conf[0] take np.interp's left values r = 0, p = 1.
//   py     : mrec / mpre of compute_ap (:93-97): element k's mrec node owns the px in [recall[k], next mrec); the end sentinel
//            (recall[-1] + 0.01, 0) owns the rest with value 0, the start sentinel (0, 1) owns [0, recall[0]).
//   mr     : element k owns the grid values in [fppi[k], fppi[k+1]), the last one up to +inf, the sentinel (fppi -1, miss 1) those
//            below fppi[0].
// A class without labels gets rows of zeros; one with labels and no predictions zeros in p / r / py and ones in mr.
__global__ void __launch_bounds__(CURVE_THREADS) curves_walk_kernel(const unsigned short* __restrict__ tp_bits, const float* __restrict__ conf,
                                                                    const int* __restrict__ idx, const int* __restrict__ seg,
                                                                    const int* __restrict__ label_hist, int n_images,
                                                                    const double* __restrict__ px_g, const double* __restrict__ grid, int ng,
                                                                    double* __restrict__ pcurve, double* __restrict__ rcurve,
                                                                    double* __restrict__ pycurve, double* __restrict__ mr) {
  __shared__ double s_px[NPX];
  __shared__ int s_w[CURVE_THREADS / 64];
  __shared__ double s_max[CURVE_THREADS], s_rec[CURVE_THREADS], s_env[CURVE_THREADS], s_prec[CURVE_THREADS], s_cf[CURVE_THREADS];
  __shared__ int s_fpc[CURVE_THREADS];
  __shared__ double s_carry[4];     // recall (mrec), envelope, precision, conf of the node after the current chunk
  __shared__ int s_carry_fpc;       // FP count of the element after the current chunk
  const int c = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int nl = label_hist[c];
  double* P = pcurve + (long)c * NPX;
  double* R = rcurve + (long)c * NPX;
  double* PY = pycurve + (long)c * NPX;
  double* M = mr + (long)c * ng;
  const int s = seg[2 * c], np_ = nl > 0 ? seg[2 * c + 1] - s : 0;
  if (np_ <= 0) {
    const double m = nl > 0 ? 1.0 : 0.0;              // labels and no predictions: every label is missed at every FPPI
    for (int i = tid; i < NPX; i += CURVE_THREADS) { P[i] = 0.0; R[i] = 0.0; PY[i] = 0.0; }
    for (int g = tid; g < ng; g += CURVE_THREADS) M[g] = m;
    return;
  }
  for (int i = tid; i < NPX; i += CURVE_THREADS) s_px[i] = px_g[i];
  // total TP of column 0 in the class
  int cnt = 0;
  for (int k = tid; k < np_; k += CURVE_THREADS) cnt += tp_bits[idx[s + k]] & 1;
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) cnt += __shfl_xor(cnt, o);
  if (lane == 0) s_w[wave] = cnt;
  __syncthreads();
  int T = 0;
  for (int w = 0; w < CURVE_THREADS / 64; ++w) T += s_w[w];
  const double denom = (double)nl + 1e-16;           // n_l + 1e-16 (:56)
  const double nimg = (double)n_images;
  if (tid == 0) {                                    // compute_ap's end sentinel: mrec = recall[-1] + 0.01, mpre = 0 (:93-94)
    s_carry[0] = (double)T / denom + 0.01;
    s_carry[1] = 0.0;
    s_carry[2] = 0.0;
    s_carry[3] = 0.0;
    s_carry_fpc = 0;
  }
  __syncthreads();
  int after = 0;                                     // TPs at positions after the current chunk
  for (int hi = np_; hi > 0; hi -= CURVE_THREADS) {
    const int k = hi - 1 - tid;                      // thread 0 holds the last element of the chunk
    const bool valid = k >= 0;
    const int i0 = valid ? idx[s + k] : 0;
    const unsigned bit = valid ? (tp_bits[i0] & 1u) : 0u;
    const double cf = valid ? (double)conf[i0] : 0.0;
    int tot;
    const int excl = block_excl_scan((int)bit, s_w, &tot);
    const int tpc = T - (after + excl);              // tp.cumsum(0) at k, an exact integer
    const int fpc = k + 1 - tpc;                     // (1 - tp).cumsum(0) at k
    const double rec = (double)tpc / denom;
    const double prec = (double)tpc / (double)(k + 1);
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
    s_rec[tid] = rec; s_env[tid] = env; s_prec[tid] = prec; s_cf[tid] = cf; s_fpc[tid] = fpc;
    __syncthreads();
    // the next node: element k + 1 (thread tid - 1), or the node carried from after the chunk
    const double nrec = tid == 0 ? s_carry[0] : s_rec[tid - 1];
    const double nenv = tid == 0 ? s_carry[1] : s_env[tid - 1];
    const double nprec = tid == 0 ? s_carry[2] : s_prec[tid - 1];
    const double ncf = tid == 0 ? s_carry[3] : s_cf[tid - 1];
    const int nfpc = tid == 0 ? s_carry_fpc : s_fpc[tid - 1];
    const bool last = k == np_ - 1;
    if (valid) {
      // PR curve: this element's mrec node owns the px in [mrec, next mrec)
      const int qa = grid_bound(s_px, NPX, rec, false), qb = grid_bound(s_px, NPX, nrec, false);
      for (int q = qa; q < qb; ++q) PY[q] = np_interp_seg(s_px[q], rec, env, nrec, nenv);
      if (last)                                      // the end sentinel owns the rest: mpre there is 0
        for (int q = qb; q < NPX; ++q) PY[q] = 0.0;
      // p / r at px (xp = -conf ascending, x = -px)
      const int ia = last ? 0 : grid_bound(s_px, NPX, ncf, true), ib = grid_bound(s_px, NPX, cf, true);
      for (int i = ia; i < ib; ++i) {
        if (last) { R[i] = rec; P[i] = prec; continue; }
        const double xq = -s_px[i];
        R[i] = np_interp_seg(xq, -cf, rec, -ncf, nrec);
        P[i] = np_interp_seg(xq, -cf, prec, -ncf, nprec);
      }
      // miss rate: the grid values in [fppi[k], fppi[k+1]), one division and one subtraction each
      const int ga = grid_bound(grid, ng, (double)fpc / nimg, false);
      const int gb = last ? ng : grid_bound(grid, ng, (double)nfpc / nimg, false);
      const double miss = 1.0 - rec;
      for (int g = ga; g < gb; ++g) M[g] = miss;
    }
    __syncthreads();
    const int first = hi - CURVE_THREADS >= 0 ? CURVE_THREADS - 1 : hi - 1;     // the thread holding the chunk's lowest k
    if (tid == first) { s_carry[0] = rec; s_carry[1] = env; s_carry[2] = prec; s_carry[3] = cf; s_carry_fpc = fpc; }
    after += tot;
    __syncthreads();
  }
  // compute_ap's start sentinel (mrec = 0, mpre = max(1, ...) = 1) owns [0, recall[0])
  const int qb = grid_bound(s_px, NPX, s_carry[0], false);
  for (int q = tid; q < qb; q += CURVE_THREADS) PY[q] = np_interp_seg(s_px[q], 0.0, 1.0, s_carry[0], s_carry[1]);
  // px above the highest conf: np.interp's left values, r = 0 and p = 1
  const int ia = grid_bound(s_px, NPX, s_carry[3], true);
  for (int i = ia + tid; i < NPX; i += CURVE_THREADS) { R[i] = 0.0; P[i] = 1.0; }
  // grid values below the first fppi: the sentinel's miss rate 1
  const int gb = grid_bound(grid, ng, (double)s_carry_fpc / nimg, false);
  for (int g = tid; g < gb; g += CURVE_THREADS) M[g] = 1.0;
}

// f1 = 2 p r / (p + r + 1e-16) at every px point (rows of classes without labels are zero) and the index of its class mean's
// argmax, by the rule cft_eval_ap uses (f1_best_index).  One workgroup of 1024 threads.
__global__ void __launch_bounds__(1024) curves_f1_kernel(const int* __restrict__ label_hist, int nc, const double* __restrict__ pcurve,
                                                         const double* __restrict__ rcurve, double* __restrict__ f1curve, int* __restrict__ best) {
  __shared__ double s_v[16];
  __shared__ int s_i[16];
  __shared__ int s_best;
  const int tid = threadIdx.x;
  const int i = f1_best_index(label_hist, nc, pcurve, rcurve, s_v, s_i, &s_best);
  if (tid == 0) *best = i;
  if (tid >= NPX) return;
  for (int c = 0; c < nc; ++c) {
    const long o = (long)c * NPX + tid;
    const double p = pcurve[o], r = rcurve[o];
    f1curve[o] = label_hist[c] > 0 ? 2.0 * p * r / (p + r + 1e-16) : 0.0;
  }
}

extern "C" int cft_eval_curves_workspace_bytes(long n, int nc, long* bytes) {
  CFT_REQUIRE(bytes, "cft_eval_curves_workspace_bytes: null pointer");
  CFT_REQUIRE(n >= 0 && n < (1L << 30) && nc >= 1 && nc <= 65535, "cft_eval_curves_workspace_bytes: bad n or nc");
  *bytes = (long)ap_ws_layout(n, nc, nullptr, nullptr);
  return CFT_OK;
}

extern "C" int cft_eval_curves(const unsigned short* tp_bits, const float* conf, const int* pcls, long n, const int* label_hist, int nc,
                               int n_images, const double* px, const double* fppi_grid, const double* fppi_grid_host, int ng, void* workspace,
                               long workspace_bytes, double* pcurve, double* rcurve, double* f1curve, double* pycurve, double* mr, int* best,
                               void* stream) {
  CFT_REQUIRE(label_hist && px && fppi_grid && fppi_grid_host && workspace, "cft_eval_curves: null pointer");
  CFT_REQUIRE(pcurve && rcurve && f1curve && pycurve && mr && best, "cft_eval_curves: null output");
  CFT_REQUIRE(n >= 0 && n < (1L << 30) && (n == 0 || (tp_bits && conf && pcls)), "cft_eval_curves: bad n (0 <= n < 2^30)");
  CFT_REQUIRE(nc >= 1 && nc <= 65535, "cft_eval_curves: nc must be in [1, 65535]");
  CFT_REQUIRE(n_images >= 1, "cft_eval_curves: n_images must be >= 1");
  CFT_REQUIRE(ng >= 1 && ng <= CURVES_MAX_GRID, "cft_eval_curves: the FPPI grid must have 1 to 4096 values");
  CFT_REQUIRE((((size_t)px | (size_t)fppi_grid | (size_t)fppi_grid_host | (size_t)pcurve | (size_t)rcurve | (size_t)f1curve | (size_t)pycurve |
                (size_t)mr) & 7) == 0, "cft_eval_curves: float64 arrays must be 8-byte aligned");
  CFT_REQUIRE(((size_t)label_hist & 3) == 0 && ((size_t)best & 3) == 0 && ((size_t)conf & 3) == 0 && ((size_t)pcls & 3) == 0 &&
              ((size_t)tp_bits & 1) == 0, "cft_eval_curves: misaligned integer or float32 array");
  for (int g = 0; g < ng; ++g) {
    const double v = fppi_grid_host[g];
    CFT_REQUIRE(v == v && v - v == 0.0, "cft_eval_curves: the FPPI grid must be finite");
    CFT_REQUIRE(g == 0 || fppi_grid_host[g - 1] <= v, "cft_eval_curves: the FPPI grid must be non-decreasing");
  }
  CFT_REQUIRE(workspace_bytes >= (long)ap_ws_layout(n, nc, nullptr, nullptr),
              "cft_eval_curves: workspace too small (see cft_eval_curves_workspace_bytes)");
  CFT_REQUIRE(((size_t)workspace & 255) == 0, "cft_eval_curves: workspace must be 256-byte aligned");
  hipStream_t st = as_stream(stream);
  ApWs w;
  ap_ws_layout(n, nc, (char*)workspace, &w);
  int cur = 0;
  int rc = eval_sort_launch(conf, pcls, n, label_hist, nc, w, &cur, st);
  if (rc != CFT_OK) return rc;
  hipLaunchKernelGGL(curves_walk_kernel, dim3(nc), dim3(CURVE_THREADS), 0, st, tp_bits, conf, w.idx[cur], w.seg, label_hist, n_images, px,
                     fppi_grid, ng, pcurve, rcurve, pycurve, mr);
  if ((rc = cft_check_launch("curves_walk_kernel")) != CFT_OK) return rc;
  hipLaunchKernelGGL(curves_f1_kernel, dim3(1), dim3(1024), 0, st, label_hist, nc, pcurve, rcurve, f1curve, best);
  return cft_check_launch("curves_f1_kernel");
}
