// The second half of a training step: torch.optim.SGD's update (train.py:560-563, :769) and ModelEMA.update
// (utils/torch_utils.py:289-299), each as ONE launch over every tensor (include/cft_hip.h has the contract).
//
// Both kernels stream: 20 bytes per element for the step (read p, g, b; write p, b), 12 for the EMA (read e, m; write e), no reuse,
// so the design is only about keeping HBM busy: 256-thread workgroups, a grid-stride over the work table capped at 2 048
// workgroups (8 per CU), 16-byte loads and stores wherever a chunk is full and aligned, all loads of a pass issued before the
// first store.  Plain C++ loads and stores only - no atomics, no LDS, no inline assembly; every element belongs to one thread.
//
// torch.optim.Adam / AdamW (train.py:558, the --adam switch) is the same walk with two more streams: 28 bytes per element (read p, g,
// m, v; write p, m, v).  Its step counters live on the device, one float per tensor, because only the device knows whether GradScaler
// skipped a step: adam_prepare_kernel (one thread per tensor) advances them and writes the two bias-correction coefficients of each
// tensor, adam_step_kernel, launched behind it on the same stream, reads those.  No kernel reads what another workgroup of the same
// launch writes.  Rounding rule of one element (contraction off; an fma only where it is written; sqrtf and / correctly rounded):
//   g0  = grad_scale ? g * (float)(1.0 / (double)*grad_scale) : g
//   Adam  (L2), wd != 0:        g1 = fma(wd, p, g0);  p0 = p
//   AdamW (decoupled), wd != 0: p0 = p * decay;       g1 = g0
//   m1  = fma(w1, g1 - m, m)                           w1 = (float)(1 - beta1)
//   v1  = fma(w2 * g1, g1, b2 * v)                     w2 = (float)(1 - beta2), b2 = (float)beta2
//   den = sqrtf(v1) / bc2_sqrt + eps                   bc2_sqrt = (float)sqrt(1 - beta2^step)
//   p  <- p0 + (-step_size * m1) / den;  m <- m1;  v <- v1        step_size = (float)(lr / (1 - beta1^step))
// the order of operations of torch's single-tensor path (lerp_, mul_().addcmul_(), addcdiv_).
#include "cft_common.h"
#include <math.h>

namespace {

constexpr int kThreads = 256;

struct SgdHyper {                    // by value in the kernel arguments: 128 bytes
  float lr[CFT_OPTIM_MAX_GROUPS], momentum[CFT_OPTIM_MAX_GROUPS], wd[CFT_OPTIM_MAX_GROUPS];
  int nesterov[CFT_OPTIM_MAX_GROUPS];
};

struct SgdCoef { float lr, momentum, wd, inv_scale; bool nesterov, scale; };

// one element; every a + s * b is one fma (the contract of cft_sgd_step)
__device__ __forceinline__ void sgd_element(float& p, float g, float& b, const SgdCoef& c) {
  const float g0 = c.scale ? g * c.inv_scale : g;
  const float g1 = c.wd != 0.0f ? __builtin_fmaf(c.wd, p, g0) : g0;
  const float b1 = c.momentum != 0.0f ? __builtin_fmaf(c.momentum, b, g1) : g1;
  const float d = c.nesterov ? __builtin_fmaf(c.momentum, b1, g1) : b1;
  p = __builtin_fmaf(-c.lr, d, p);
  b = b1;
}

// The tensor pointers come out of the table, so the compiler knows no address space for them and would emit flat accesses; every one
// of them is device memory: say so and get global loads and stores.
typedef __attribute__((address_space(1))) float gfloat;
typedef __attribute__((address_space(1))) f32x4_t gfloat4;
__device__ __forceinline__ gfloat* as_global(const float* a) { return (gfloat*)(uintptr_t)a; }

__device__ __forceinline__ bool aligned16(const void* a) { return (reinterpret_cast<uintptr_t>(a) & 15u) == 0; }

__global__ void __launch_bounds__(kThreads)
sgd_step_kernel(const cft_sgd_seg_t* __restrict__ segs, const cft_optim_work_t* __restrict__ work, long nwork, int chunk,
                SgdHyper h, const float* __restrict__ grad_scale, const float* __restrict__ found_inf) {
  if (found_inf != nullptr && *found_inf != 0.0f) return;        // the step GradScaler skips: nothing is written
  SgdCoef c;
  c.scale = grad_scale != nullptr;
  c.inv_scale = c.scale ? (float)(1.0 / (double)*grad_scale) : 1.0f;
  for (long w = blockIdx.x; w < nwork; w += gridDim.x) {
    const cft_optim_work_t wk = work[w];
    const cft_sgd_seg_t s = segs[wk.seg];
    const int gi = (int)s.group;
    c.lr = h.lr[gi]; c.momentum = h.momentum[gi]; c.wd = h.wd[gi]; c.nesterov = h.nesterov[gi] != 0;
    const bool has_b = c.momentum != 0.0f;
    const long rem = s.n - wk.start;
    const int cnt = rem < (long)chunk ? (int)rem : chunk;
    gfloat* __restrict__ p = as_global(s.p) + wk.start;
    const gfloat* __restrict__ g = as_global(s.g) + wk.start;
    gfloat* __restrict__ b = has_b ? as_global(s.buf) + wk.start : nullptr;
    if (cnt == chunk && aligned16((const void*)(uintptr_t)p) && aligned16((const void*)(uintptr_t)g) && (!has_b || aligned16((const void*)(uintptr_t)b))) {
      for (int i = threadIdx.x * 4; i < chunk; i += kThreads * 4) {        // chunk % 1024 == 0: no tail
        f32x4_t pv = *reinterpret_cast<const gfloat4*>(p + i);
        const f32x4_t gv = *reinterpret_cast<const gfloat4*>(g + i);
        f32x4_t bv = has_b ? *reinterpret_cast<const gfloat4*>(b + i) : f32x4_t{0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int k = 0; k < 4; ++k) {
          float pk = pv[k], bk = bv[k];
          sgd_element(pk, gv[k], bk, c);
          pv[k] = pk; bv[k] = bk;
        }
        *reinterpret_cast<gfloat4*>(p + i) = pv;
        if (has_b) *reinterpret_cast<gfloat4*>(b + i) = bv;
      }
    } else {
      for (int i = threadIdx.x; i < cnt; i += kThreads) {
        float pv = p[i], bv = has_b ? b[i] : 0.0f;
        sgd_element(pv, g[i], bv, c);
        p[i] = pv;
        if (has_b) b[i] = bv;
      }
    }
  }
}

__global__ void __launch_bounds__(kThreads)
ema_update_kernel(const cft_ema_seg_t* __restrict__ segs, const cft_optim_work_t* __restrict__ work, long nwork, int chunk,
                  float d, float one_minus_d) {
  for (long w = blockIdx.x; w < nwork; w += gridDim.x) {
    const cft_optim_work_t wk = work[w];
    const cft_ema_seg_t s = segs[wk.seg];
    const long rem = s.n - wk.start;
    const int cnt = rem < (long)chunk ? (int)rem : chunk;
    gfloat* __restrict__ e = as_global(s.e) + wk.start;
    const gfloat* __restrict__ m = as_global(s.m) + wk.start;
    if (cnt == chunk && aligned16((const void*)(uintptr_t)e) && aligned16((const void*)(uintptr_t)m)) {
      for (int i = threadIdx.x * 4; i < chunk; i += kThreads * 4) {
        f32x4_t ev = *reinterpret_cast<const gfloat4*>(e + i);
        const f32x4_t mv = *reinterpret_cast<const gfloat4*>(m + i);
#pragma unroll
        for (int k = 0; k < 4; ++k) ev[k] = __builtin_fmaf(one_minus_d, mv[k], d * ev[k]);
        *reinterpret_cast<gfloat4*>(e + i) = ev;
      }
    } else {
      for (int i = threadIdx.x; i < cnt; i += kThreads) e[i] = __builtin_fmaf(one_minus_d, m[i], d * e[i]);
    }
  }
}

struct AdamHyper {                   // by value in the kernel arguments: 224 bytes
  float w1[CFT_OPTIM_MAX_GROUPS], b2[CFT_OPTIM_MAX_GROUPS], w2[CFT_OPTIM_MAX_GROUPS], eps[CFT_OPTIM_MAX_GROUPS], wd[CFT_OPTIM_MAX_GROUPS],
      decay[CFT_OPTIM_MAX_GROUPS];
  int decoupled[CFT_OPTIM_MAX_GROUPS];
};

struct AdamPrepare {                 // by value in the kernel arguments: 192 bytes
  double lr[CFT_OPTIM_MAX_GROUPS], beta1[CFT_OPTIM_MAX_GROUPS], beta2[CFT_OPTIM_MAX_GROUPS];
};

struct AdamCoef { float w1, b2, w2, eps, wd, decay, inv_scale, step_size, bc2_sqrt; bool decoupled, scale; };

// one element, by the rounding rule above
__device__ __forceinline__ void adam_element(float& p, float g, float& m, float& v, const AdamCoef& c) {
#pragma clang fp contract(off)
  const float g0 = c.scale ? g * c.inv_scale : g;
  float g1 = g0, p0 = p;
  if (c.wd != 0.0f) {
    if (c.decoupled) p0 = p * c.decay;
    else g1 = __builtin_fmaf(c.wd, p, g0);
  }
  const float m1 = __builtin_fmaf(c.w1, g1 - m, m);
  const float v1 = __builtin_fmaf(c.w2 * g1, g1, c.b2 * v);
  const float den = __builtin_sqrtf(v1) / c.bc2_sqrt + c.eps;
  p = p0 + (-c.step_size * m1) / den;
  m = m1;
  v = v1;
}

// One thread per tensor: count the step and form the tensor's two coefficients in double, as torch does with Python floats.
__global__ void __launch_bounds__(kThreads)
adam_prepare_kernel(const cft_adam_seg_t* __restrict__ segs, int nseg, AdamPrepare h, float* __restrict__ coef,
                    const float* __restrict__ found_inf) {
  if (found_inf != nullptr && *found_inf != 0.0f) return;        // a skipped step is not counted
  const int i = blockIdx.x * kThreads + threadIdx.x;
  if (i >= nseg) return;
  const cft_adam_seg_t s = segs[i];
  const int gi = (int)s.group;
  gfloat* __restrict__ step = as_global(s.step);
  const float count = *step + 1.0f;
  *step = count;
  const double bc1 = 1.0 - pow(h.beta1[gi], (double)count);
  const double bc2 = 1.0 - pow(h.beta2[gi], (double)count);
  gfloat* __restrict__ out = as_global(coef) + 2 * (long)i;
  out[0] = (float)(h.lr[gi] / bc1);
  out[1] = (float)sqrt(bc2);
}

__global__ void __launch_bounds__(kThreads)
adam_step_kernel(const cft_adam_seg_t* __restrict__ segs, const cft_optim_work_t* __restrict__ work, long nwork, int chunk,
                 AdamHyper h, const float* __restrict__ coef, const float* __restrict__ grad_scale, const float* __restrict__ found_inf) {
  if (found_inf != nullptr && *found_inf != 0.0f) return;        // the step GradScaler skips: nothing is written
  AdamCoef c;
  c.scale = grad_scale != nullptr;
  c.inv_scale = c.scale ? (float)(1.0 / (double)*grad_scale) : 1.0f;
  for (long w = blockIdx.x; w < nwork; w += gridDim.x) {
    const cft_optim_work_t wk = work[w];
    const cft_adam_seg_t s = segs[wk.seg];
    const int gi = (int)s.group;
    c.w1 = h.w1[gi]; c.b2 = h.b2[gi]; c.w2 = h.w2[gi]; c.eps = h.eps[gi]; c.wd = h.wd[gi]; c.decay = h.decay[gi];
    c.decoupled = h.decoupled[gi] != 0;
    const gfloat* __restrict__ co = as_global(coef) + 2 * (long)wk.seg;
    c.step_size = co[0]; c.bc2_sqrt = co[1];
    const long rem = s.n - wk.start;
    const int cnt = rem < (long)chunk ? (int)rem : chunk;
    gfloat* __restrict__ p = as_global(s.p) + wk.start;
    const gfloat* __restrict__ g = as_global(s.g) + wk.start;
    gfloat* __restrict__ m = as_global(s.m) + wk.start;
    gfloat* __restrict__ v = as_global(s.v) + wk.start;
    if (cnt == chunk && aligned16((const void*)(uintptr_t)p) && aligned16((const void*)(uintptr_t)g) && aligned16((const void*)(uintptr_t)m) &&
        aligned16((const void*)(uintptr_t)v)) {
      for (int i = threadIdx.x * 4; i < chunk; i += kThreads * 4) {        // chunk % 1024 == 0: no tail
        f32x4_t pv = *reinterpret_cast<const gfloat4*>(p + i);
        const f32x4_t gv = *reinterpret_cast<const gfloat4*>(g + i);
        f32x4_t mv = *reinterpret_cast<const gfloat4*>(m + i);
        f32x4_t vv = *reinterpret_cast<const gfloat4*>(v + i);
#pragma unroll
        for (int k = 0; k < 4; ++k) {
          float pk = pv[k], mk = mv[k], vk = vv[k];
          adam_element(pk, gv[k], mk, vk, c);
          pv[k] = pk; mv[k] = mk; vv[k] = vk;
        }
        *reinterpret_cast<gfloat4*>(p + i) = pv;
        *reinterpret_cast<gfloat4*>(m + i) = mv;
        *reinterpret_cast<gfloat4*>(v + i) = vv;
      }
    } else {
      for (int i = threadIdx.x; i < cnt; i += kThreads) {
        float pv = p[i], mv = m[i], vv = v[i];
        adam_element(pv, g[i], mv, vv, c);
        p[i] = pv;
        m[i] = mv;
        v[i] = vv;
      }
    }
  }
}

bool word_aligned(const void* a) { return (reinterpret_cast<uintptr_t>(a) & 3u) == 0; }

// The canonical cut: the chunks of segment 0 in order, then segment 1's, ...; n[i] = element count of segment i (>= 0, checked by
// the caller).  Returns nullptr when the work rows are exactly that, else what is wrong.
template <typename Seg>
const char* check_work(const Seg* segs, int nseg, const cft_optim_work_t* work, long nwork, int chunk) {
  long w = 0;
  for (int i = 0; i < nseg; ++i) {
    for (long start = 0; start < segs[i].n; start += chunk, ++w) {
      if (w >= nwork) return "fewer work rows than the segments have chunks";
      if (work[w].seg != i || work[w].start != start || work[w].pad != 0) return "a work row is not the next chunk of its segment";
    }
  }
  return w == nwork ? nullptr : "more work rows than the segments have chunks";
}

int check_common(const char* who, const void* table_dev, const void* table_host, int nseg, long nwork, int chunk, int max_blocks) {
  char buf[160];
  const char* bad = nullptr;
  if (table_dev == nullptr || table_host == nullptr) bad = "null table";
  else if (nseg < 0 || nwork < 0) bad = "negative segment or work count";
  else if (nseg > (1 << 24) || nwork > (1L << 31)) bad = "table too large";
  else if (chunk < 1024 || chunk > (1 << 20) || chunk % 1024 != 0) bad = "chunk must be a multiple of 1024 in [1024, 2^20]";
  else if (max_blocks < 0 || max_blocks > 65536) bad = "max_blocks outside [0, 65536]";
  else if ((reinterpret_cast<uintptr_t>(table_dev) & 7u) != 0 || (reinterpret_cast<uintptr_t>(table_host) & 7u) != 0) bad = "table not 8-byte aligned";
  if (bad == nullptr) return CFT_OK;
  snprintf(buf, sizeof(buf), "%s: %s", who, bad);
  cft_set_error(buf);
  return CFT_EINVAL;
}

int fail_work(const char* who, const char* what) {
  char buf[200];
  snprintf(buf, sizeof(buf), "%s: %s", who, what);
  cft_set_error(buf);
  return CFT_EINVAL;
}

int fail(const char* who, const char* what, int row) {
  char buf[200];
  snprintf(buf, sizeof(buf), "%s: segment %d: %s", who, row, what);
  cft_set_error(buf);
  return CFT_EINVAL;
}

int blocks_for(long nwork, int max_blocks) {
  const long cap = max_blocks > 0 ? max_blocks : CFT_OPTIM_MAX_BLOCKS;
  return (int)(nwork < cap ? nwork : cap);
}

}  // namespace

static_assert(sizeof(cft_sgd_seg_t) == CFT_SGD_SEG_BYTES && sizeof(cft_ema_seg_t) == CFT_EMA_SEG_BYTES &&
              sizeof(cft_adam_seg_t) == CFT_ADAM_SEG_BYTES && sizeof(cft_optim_work_t) == CFT_OPTIM_WORK_BYTES,
              "table row sizes are part of the ABI");

extern "C" int cft_sgd_step(const void* table_dev, const void* table_host, int nseg, long nwork, int chunk, int max_blocks,
                            const float* hyper_host, int ngroups, const float* grad_scale, const float* found_inf, void* stream) {
  const int st = check_common("cft_sgd_step", table_dev, table_host, nseg, nwork, chunk, max_blocks);
  if (st != CFT_OK) return st;
  CFT_REQUIRE(hyper_host != nullptr, "cft_sgd_step: null hyper-parameter array");
  CFT_REQUIRE(ngroups >= 1 && ngroups <= CFT_OPTIM_MAX_GROUPS, "cft_sgd_step: 1 to 8 param groups");
  CFT_REQUIRE(word_aligned(grad_scale) && word_aligned(found_inf), "cft_sgd_step: grad_scale / found_inf not 4-byte aligned");
  SgdHyper h = {};
  for (int j = 0; j < ngroups; ++j) {
    h.lr[j] = hyper_host[4 * j]; h.momentum[j] = hyper_host[4 * j + 1]; h.wd[j] = hyper_host[4 * j + 2];
    const float nest = hyper_host[4 * j + 3];
    CFT_REQUIRE(nest == 0.0f || nest == 1.0f, "cft_sgd_step: the nesterov flag is 0 or 1");
    CFT_REQUIRE(!(h.lr[j] != h.lr[j]) && !(h.momentum[j] != h.momentum[j]) && !(h.wd[j] != h.wd[j]), "cft_sgd_step: NaN hyper-parameter");
    CFT_REQUIRE(nest == 0.0f || h.momentum[j] != 0.0f, "cft_sgd_step: nesterov needs a momentum");
    h.nesterov[j] = nest != 0.0f;
  }
  const cft_sgd_seg_t* segs = static_cast<const cft_sgd_seg_t*>(table_host);
  for (int i = 0; i < nseg; ++i) {
    const cft_sgd_seg_t& s = segs[i];
    if (s.n < 0) return fail("cft_sgd_step", "negative element count", i);
    if (s.group < 0 || s.group >= ngroups) return fail("cft_sgd_step", "group index out of range", i);
    if (s.p == nullptr || s.g == nullptr) return fail("cft_sgd_step", "null parameter or gradient", i);
    if (s.buf == nullptr && h.momentum[s.group] != 0.0f) return fail("cft_sgd_step", "no momentum buffer in a group with momentum", i);
    if (!word_aligned(s.p) || !word_aligned(s.g) || !word_aligned(s.buf)) return fail("cft_sgd_step", "pointer not 4-byte aligned", i);
  }
  const cft_optim_work_t* work = reinterpret_cast<const cft_optim_work_t*>(segs + nseg);
  if (const char* bad = check_work(segs, nseg, work, nwork, chunk)) return fail_work("cft_sgd_step", bad);
  if (nwork == 0) return CFT_OK;
  const cft_sgd_seg_t* dsegs = static_cast<const cft_sgd_seg_t*>(table_dev);
  hipLaunchKernelGGL(sgd_step_kernel, dim3(blocks_for(nwork, max_blocks)), dim3(kThreads), 0, as_stream(stream), dsegs,
                     reinterpret_cast<const cft_optim_work_t*>(dsegs + nseg), nwork, chunk, h, grad_scale, found_inf);
  return cft_check_launch("sgd_step_kernel");
}

extern "C" int cft_ema_update(const void* table_dev, const void* table_host, int nseg, long nwork, int chunk, int max_blocks,
                              float d, float one_minus_d, void* stream) {
  const int st = check_common("cft_ema_update", table_dev, table_host, nseg, nwork, chunk, max_blocks);
  if (st != CFT_OK) return st;
  CFT_REQUIRE(!(d != d) && !(one_minus_d != one_minus_d), "cft_ema_update: NaN decay");
  const cft_ema_seg_t* segs = static_cast<const cft_ema_seg_t*>(table_host);
  for (int i = 0; i < nseg; ++i) {
    const cft_ema_seg_t& s = segs[i];
    if (s.n < 0) return fail("cft_ema_update", "negative element count", i);
    if (s.e == nullptr || s.m == nullptr) return fail("cft_ema_update", "null tensor", i);
    if (!word_aligned(s.e) || !word_aligned(s.m)) return fail("cft_ema_update", "pointer not 4-byte aligned", i);
  }
  const cft_optim_work_t* work = reinterpret_cast<const cft_optim_work_t*>(segs + nseg);
  if (const char* bad = check_work(segs, nseg, work, nwork, chunk)) return fail_work("cft_ema_update", bad);
  if (nwork == 0) return CFT_OK;
  const cft_ema_seg_t* dsegs = static_cast<const cft_ema_seg_t*>(table_dev);
  hipLaunchKernelGGL(ema_update_kernel, dim3(blocks_for(nwork, max_blocks)), dim3(kThreads), 0, as_stream(stream), dsegs,
                     reinterpret_cast<const cft_optim_work_t*>(dsegs + nseg), nwork, chunk, d, one_minus_d);
  return cft_check_launch("ema_update_kernel");
}

extern "C" int cft_adam_step(const void* table_dev, const void* table_host, int nseg, long nwork, int chunk, int max_blocks,
                             const double* hyper_host, int ngroups, float* coef, const float* grad_scale, const float* found_inf,
                             void* stream) {
  const int st = check_common("cft_adam_step", table_dev, table_host, nseg, nwork, chunk, max_blocks);
  if (st != CFT_OK) return st;
  CFT_REQUIRE(hyper_host != nullptr, "cft_adam_step: null hyper-parameter array");
  CFT_REQUIRE(ngroups >= 1 && ngroups <= CFT_OPTIM_MAX_GROUPS, "cft_adam_step: 1 to 8 param groups");
  CFT_REQUIRE(coef != nullptr && (reinterpret_cast<uintptr_t>(coef) & 7u) == 0, "cft_adam_step: coef null or not 8-byte aligned");
  CFT_REQUIRE(word_aligned(grad_scale) && word_aligned(found_inf), "cft_adam_step: grad_scale / found_inf not 4-byte aligned");
  AdamHyper h = {};
  AdamPrepare hp = {};
  for (int j = 0; j < ngroups; ++j) {
    const double lr = hyper_host[6 * j], beta1 = hyper_host[6 * j + 1], beta2 = hyper_host[6 * j + 2], eps = hyper_host[6 * j + 3],
                 wd = hyper_host[6 * j + 4], flag = hyper_host[6 * j + 5];
    CFT_REQUIRE(!(lr != lr) && !(beta1 != beta1) && !(beta2 != beta2) && !(eps != eps) && !(wd != wd) && !(flag != flag),
                "cft_adam_step: NaN hyper-parameter");
    CFT_REQUIRE(lr >= 0.0 && eps >= 0.0 && wd >= 0.0, "cft_adam_step: lr, eps and weight_decay are >= 0");
    CFT_REQUIRE(beta1 >= 0.0 && beta1 < 1.0 && beta2 >= 0.0 && beta2 < 1.0, "cft_adam_step: betas are in [0, 1)");
    CFT_REQUIRE(flag == 0.0 || flag == 1.0, "cft_adam_step: the decoupled flag is 0 or 1");
    hp.lr[j] = lr; hp.beta1[j] = beta1; hp.beta2[j] = beta2;
    h.w1[j] = (float)(1.0 - beta1); h.b2[j] = (float)beta2; h.w2[j] = (float)(1.0 - beta2); h.eps[j] = (float)eps; h.wd[j] = (float)wd;
    h.decay[j] = (float)(1.0 - lr * wd);
    h.decoupled[j] = flag != 0.0;
  }
  const cft_adam_seg_t* segs = static_cast<const cft_adam_seg_t*>(table_host);
  for (int i = 0; i < nseg; ++i) {
    const cft_adam_seg_t& s = segs[i];
    if (s.n < 0) return fail("cft_adam_step", "negative element count", i);
    if (s.group < 0 || s.group >= ngroups) return fail("cft_adam_step", "group index out of range", i);
    if (s.p == nullptr || s.g == nullptr) return fail("cft_adam_step", "null parameter or gradient", i);
    if (s.m == nullptr || s.v == nullptr || s.step == nullptr) return fail("cft_adam_step", "null moment or step counter", i);
    if (!word_aligned(s.p) || !word_aligned(s.g) || !word_aligned(s.m) || !word_aligned(s.v) || !word_aligned(s.step))
      return fail("cft_adam_step", "pointer not 4-byte aligned", i);
  }
  const cft_optim_work_t* work = reinterpret_cast<const cft_optim_work_t*>(segs + nseg);
  if (const char* bad = check_work(segs, nseg, work, nwork, chunk)) return fail_work("cft_adam_step", bad);
  if (nwork == 0) return CFT_OK;
  const cft_adam_seg_t* dsegs = static_cast<const cft_adam_seg_t*>(table_dev);
  hipLaunchKernelGGL(adam_prepare_kernel, dim3((nseg + kThreads - 1) / kThreads), dim3(kThreads), 0, as_stream(stream), dsegs, nseg, hp,
                     coef, found_inf);
  const int sp = cft_check_launch("adam_prepare_kernel");
  if (sp != CFT_OK) return sp;
  hipLaunchKernelGGL(adam_step_kernel, dim3(blocks_for(nwork, max_blocks)), dim3(kThreads), 0, as_stream(stream), dsegs,
                     reinterpret_cast<const cft_optim_work_t*>(dsegs + nseg), nwork, chunk, h, (const float*)coef, grad_scale, found_inf);
  return cft_check_launch("adam_step_kernel");
}
