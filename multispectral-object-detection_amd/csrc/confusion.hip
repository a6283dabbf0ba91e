// What test.py computes besides its mAP statistics, on the GPU (the last step of SURVEY.md section 8f's evaluation row):
//   cft_eval_confusion  ConfusionMatrix.process_batch (utils/metrics.py:119-157) for a whole batch, one workgroup per image;
//   cft_eval_export     the box values of test.py's save_txt (:152-158) and save_json (:173-182) for every detection slot.
// The grouping of the labels by image, the box transforms and box_iou are those of cft_eval_match (metrics_common.h).  Integer
// atomics only: every result is the same run to run.
#include "metrics_common.h"

#pragma clang fp contract(off)   // the reference's float ops are separate roundings: no fused multiply-adds here

// Workspace of cft_eval_confusion: the grouped labels of cft_eval_match, one selection word per label and one chosen label per
// detection slot.
struct ConfWs {
  MatchWs m;
  unsigned long long* key;   // [nt] (IoU bits << 32) | ~row of the best detection that kept the label; 0 = none
  int* sel;                  // [B * max_det] label kept by the detection; -1 none; -2 not a filtered detection
};
static inline size_t conf_ws_layout(int B, int nt, int max_det, char* base, ConfWs* w) {
  size_t o = match_ws_layout(B, nt, base, w ? &w->m : nullptr);
  const size_t n = nt > 0 ? (size_t)nt : 1;
  if (w) w->key = (unsigned long long*)(base + o);
  o = align256(o + n * 8);
  if (w) w->sel = (int*)(base + o);
  o = align256(o + (size_t)B * max_det * 4);
  return o;
}

enum { CONF_BAD_LABEL_CLASS = 1, CONF_BAD_DET_CLASS = 2 };

// ConfusionMatrix.process_batch (utils/metrics.py:119-157) of image b = blockIdx.x, fed as test.py:193-194 feeds it:
//  * only an image with labels and NMS detections is processed (test.py:140-143 `continue`s without detections, :186 `if nl`);
//  * detections are filtered by conf > conf_thres (:129, strict), classes are .int() truncations (:130-131), the detection
//    class is 0 with single_cls (test.py:146-147);
//  * candidate pairs have box_iou > iou_thres (:132-134, strict; a NaN IoU is no candidate).  The two argsort / np.unique
//    passes (:138-141) leave, for each detection, its highest-IoU label, and then, for each label, its highest-IoU detection
//    among those that kept it.  Class plays no part;
//  * a matched label counts at [detection class, label class] (:150), any other label at [nc, label class] (:152); a filtered
//    detection in no match counts at [its class, nc] only when the image has a match at all (`if n:`, :154-157).
// numpy's argsort is not stable, so the reference leaves exactly equal IoUs open.  Here: the lowest label index wins for a
// detection, then the lowest detection row wins for a label.  Selection is a 64-bit integer atomicMax per label on
// (IoU bits, inverted row): IoUs are positive floats, whose bit patterns order like their values.  Counts are int64 atomicAdds.
// A class outside [0, nc) is not counted; it sets a bit of *flag.  A matched label whose detection has such a class is dropped
// altogether (it is NOT moved to the background row: it was matched), and the match still counts for `if n:`, so the image's
// leftover detections are counted.  The Python side raises on the flag, so such a matrix is never handed out as a result.
__global__ void __launch_bounds__(MATCH_THREADS) eval_confusion_kernel(const float* __restrict__ dets, const int* __restrict__ counts, int max_det,
                                                                       const float* __restrict__ geom, float conf_thres, float iou_thres,
                                                                       int single_cls, int native, int nc, ConfWs ws,
                                                                       unsigned long long* __restrict__ matrix, int* __restrict__ flag) {
  __shared__ float4 s_box[MATCH_LDS_LABELS];
  __shared__ int s_nmatch;
  const int b = blockIdx.x, tid = threadIdx.x;
  const int nl = ws.m.cnt[b], l0 = ws.m.off[b];
  int n = counts[b];
  n = n < 0 ? 0 : (n > max_det ? max_det : n);
  if (nl == 0 || n == 0) return;                       // uniform over the workgroup
  const bool in_lds = nl <= MATCH_LDS_LABELS;
  const float4* lbox = in_lds ? s_box : ws.m.box + l0;
  if (in_lds)
    for (int l = tid; l < nl; l += MATCH_THREADS) s_box[l] = ws.m.box[l0 + l];
  if (tid == 0) s_nmatch = 0;
  __syncthreads();
  const Geom g = native ? Geom{0.f, 0.f, 1.f, 0.f, 0.f} : load_geom(geom, b);
  const float* D = dets + (long)b * max_det * 6;
  unsigned long long* key = ws.key + l0;
  int* sel = ws.sel + (long)b * max_det;
  const long stride = (long)nc + 1;
  // each filtered detection keeps its highest-IoU label (lowest index on ties) and bids for it
  for (int r = tid; r < n; r += MATCH_THREADS) {
    const float* d = D + (long)r * 6;
    int bl = -2;
    if (d[4] > conf_thres) {
      const float4 p = native ? make_float4(d[0], d[1], d[2], d[3]) : scale_box(d[0], d[1], d[2], d[3], g);
      const float pa = (p.z - p.x) * (p.w - p.y);
      float bi = 0.f;
      bl = -1;
      for (int l = 0; l < nl; ++l) {
        const float v = box_iou1(p, pa, lbox[l]);
        if (v > iou_thres && (bl < 0 || v > bi)) { bi = v; bl = l; }
      }
      if (bl >= 0 && bi > 0.f)
        atomicMax(&key[bl], ((unsigned long long)__float_as_uint(bi) << 32) | (unsigned long long)(0xffffffffu - (unsigned)r));
    }
    sel[r] = bl;
  }
  __syncthreads();
  // labels: matched -> [class of its detection, class of the label], else [nc, class of the label]
  for (int l = tid; l < nl; l += MATCH_THREADS) {
    const unsigned long long k = __hip_atomic_load(&key[l], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    const int gc = ws.m.cls[l0 + l];
    long row = nc;
    if (k != 0ull) {
      atomicAdd(&s_nmatch, 1);
      const int r = (int)(0xffffffffu - (unsigned)(k & 0xffffffffull));
      const int dc = single_cls ? 0 : trunc_class(D[(long)r * 6 + 5]);
      if (dc < 0 || dc >= nc) { atomicOr(flag, CONF_BAD_DET_CLASS); continue; }
      row = dc;
    }
    if (gc < 0 || gc >= nc) { atomicOr(flag, CONF_BAD_LABEL_CLASS); continue; }
    atomicAdd(&matrix[row * stride + gc], 1ull);
  }
  __syncthreads();
  if (s_nmatch == 0) return;                           // `if n:` (:154): without a match the detections are not counted
  for (int r = tid; r < n; r += MATCH_THREADS) {       // the thread that wrote sel[r] reads it
    const int bl = sel[r];
    if (bl == -2) continue;
    if (bl >= 0) {
      const unsigned long long k = __hip_atomic_load(&key[bl], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      if ((int)(0xffffffffu - (unsigned)(k & 0xffffffffull)) == r) continue;     // this detection is its label's match
    }
    const int dc = single_cls ? 0 : trunc_class(D[(long)r * 6 + 5]);
    if (dc < 0 || dc >= nc) { atomicOr(flag, CONF_BAD_DET_CLASS); continue; }
    atomicAdd(&matrix[(long)dc * stride + nc], 1ull);
  }
}

extern "C" int cft_eval_confusion_workspace_bytes(int B, int nt, int max_det, long* bytes) {
  CFT_REQUIRE(bytes, "cft_eval_confusion_workspace_bytes: null pointer");
  CFT_REQUIRE(B > 0 && nt >= 0 && max_det > 0, "cft_eval_confusion_workspace_bytes: bad shape");
  *bytes = (long)conf_ws_layout(B, nt, max_det, nullptr, nullptr);
  return CFT_OK;
}

extern "C" int cft_eval_confusion(const float* dets, const int* counts, int B, int max_det, const float* targets, int nt, int img_h, int img_w,
                                  const float* geom, float conf_thres, float iou_thres, int single_cls, int native, int nc, void* workspace,
                                  long workspace_bytes, long long* matrix, int* flag, void* stream) {
  CFT_REQUIRE(dets && counts && workspace && matrix && flag && (native || geom), "cft_eval_confusion: null pointer");
  CFT_REQUIRE(B > 0 && max_det > 0 && nt >= 0 && (nt == 0 || targets) && (native || (img_h > 0 && img_w > 0)), "cft_eval_confusion: bad shape");
  CFT_REQUIRE((long)B * max_det < (1L << 31) && (long)nt * 6 < (1L << 31), "cft_eval_confusion: too many detections or labels");
  CFT_REQUIRE(nc >= 1 && nc <= 32767, "cft_eval_confusion: nc must be in [1, 32767]");
  CFT_REQUIRE(iou_thres >= 0.f, "cft_eval_confusion: iou_thres must be >= 0");
  CFT_REQUIRE(workspace_bytes >= (long)conf_ws_layout(B, nt, max_det, nullptr, nullptr),
              "cft_eval_confusion: workspace too small (see cft_eval_confusion_workspace_bytes)");
  CFT_REQUIRE(((size_t)workspace & 255) == 0, "cft_eval_confusion: workspace must be 256-byte aligned");
  ConfWs w;
  conf_ws_layout(B, nt, max_det, (char*)workspace, &w);
  int st = eval_group_launch(targets, nt, B, (float)img_h, (float)img_w, geom, w.m, nullptr, nc, nullptr, nullptr,
                             GROUP_TRUNC_CLS | (native ? GROUP_NATIVE : 0), w.key, as_stream(stream));
  if (st != CFT_OK) return st;
  hipLaunchKernelGGL(eval_confusion_kernel, dim3(B), dim3(MATCH_THREADS), 0, as_stream(stream), dets, counts, max_det, geom, conf_thres, iou_thres,
                     single_cls, native, nc, w, (unsigned long long*)matrix, flag);
  return cft_check_launch("eval_confusion_kernel");
}

constexpr int EXPORT_FLOATS = 16;

// One thread per detection slot: [x1 y1 x2 y2 | conf cls valid 0 | x y w h / (w0 h0 w0 h0) | left top w h], float32, each value one
// rounding per operation in the reference's order: predn = scale_coords(pred) (test.py:148-149); xyxy2xywh (utils/general.py:289-296:
// (x1 + x2) / 2, x2 - x1) divided by gn (test.py:153-155); the JSON box is the centre minus half the size (test.py:176-177).
// cls is 0 with single_cls (test.py:146-147); slots r >= counts[b] are zero (valid = 0).
__global__ void __launch_bounds__(MATCH_THREADS) eval_export_kernel(const float* __restrict__ dets, const int* __restrict__ counts, int B, int max_det,
                                                                    const float* __restrict__ geom, int single_cls, float4* __restrict__ out) {
  const long i = (long)blockIdx.x * MATCH_THREADS + threadIdx.x;
  if (i >= (long)B * max_det) return;
  const int b = (int)(i / max_det), r = (int)(i % max_det);
  float4* o = out + i * (EXPORT_FLOATS / 4);
  int n = counts[b];
  n = n < 0 ? 0 : (n > max_det ? max_det : n);
  if (r >= n) {
    const float4 z = make_float4(0.f, 0.f, 0.f, 0.f);
    o[0] = z; o[1] = z; o[2] = z; o[3] = z;
    return;
  }
  const float* d = dets + i * 6;
  const Geom g = load_geom(geom, b);
  const float4 p = scale_box(d[0], d[1], d[2], d[3], g);
  const float cx = (p.x + p.z) / 2.f, cy = (p.y + p.w) / 2.f, w = p.z - p.x, h = p.w - p.y;
  o[0] = p;
  o[1] = make_float4(d[4], single_cls ? 0.f : d[5], 1.f, 0.f);
  o[2] = make_float4(cx / g.w0, cy / g.h0, w / g.w0, h / g.h0);
  o[3] = make_float4(cx - w / 2.f, cy - h / 2.f, w, h);
}

extern "C" int cft_eval_export(const float* dets, const int* counts, int B, int max_det, const float* geom, int single_cls, float* out, void* stream) {
  CFT_REQUIRE(dets && counts && geom && out, "cft_eval_export: null pointer");
  CFT_REQUIRE(B > 0 && max_det > 0 && (long)B * max_det < (1L << 31), "cft_eval_export: bad shape");
  CFT_REQUIRE(((size_t)out & 15) == 0, "cft_eval_export: out must be 16-byte aligned");
  const long n = (long)B * max_det;
  hipLaunchKernelGGL(eval_export_kernel, dim3((unsigned)((n + MATCH_THREADS - 1) / MATCH_THREADS)), dim3(MATCH_THREADS), 0, as_stream(stream), dets,
                     counts, B, max_det, geom, single_cls, (float4*)out);
  return cft_check_launch("eval_export_kernel");
}
