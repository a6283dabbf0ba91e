// The second half of a training step: torch.optim.SGD's update (train.py:560-563, :769), torch.optim.Adam / AdamW (train.py:558, the
// --adam switch) and ModelEMA.update (utils/torch_utils.py:289-299), each as ONE launch over every tensor (include/cft_hip.h has
// the contract).
//
// The three kernels are one walk (walk_rows) over the work table; they differ in their streams and in the rule of one element:
//   sgd_step_kernel    p, g, b      20 bytes per element (read p, g, b; write p, b; no b in a group without momentum)
//   ema_update_kernel  e, m         12 (read e, m; write e)
//   adam_step_kernel   p, g, m, v   28 (read p, g, m, v; write p, m, v)
// They stream, no reuse, so the design is only about keeping HBM busy: 256-thread workgroups, a grid-stride over the work table
// capped at 2 048 workgroups (8 per CU), 16-byte loads and stores wherever a chunk is full and aligned, all loads of a pass issued
// before the first store.  Plain C++ loads and stores only - no atomics, no LDS, no inline assembly; every element belongs to one
// thread.  The entry points share their host side in the same way (with_table): the checks of the table, then the launch.
//
// Adam's step counters live on the device, one float per tensor, because only the device knows whether GradScaler
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

__device__ __forceinline__ bool aligned16(const gfloat* a) { return ((uintptr_t)a & 15u) == 0; }

// The walk of all three kernels: a workgroup takes work rows grid-stride; elements [start, start + chunk) of the row's segment move
// through `rule` as 16-byte words when the chunk is full and every stream that is present is 16-byte aligned, else as dwords.
//   N         streams of a segment;  bit s of Written: stream s is stored back;  bit s of Optional: stream s may be absent (null:
//             it reads as 0 and is never stored) - compile-time masks, so a stream that is always there costs no test
//   row(wk, a)  fills a[0 .. N) with the segment's base pointers, sets the coefficients of `rule`, returns the segment's n
//   rule(x)     one element: x[0 .. N) in, the written ones out
template <int N, unsigned Written, unsigned Optional, typename Row, typename Rule>
__device__ __forceinline__ void walk_rows(const cft_optim_work_t* __restrict__ work, long nwork, int chunk, Row row, Rule rule) {
  static_assert((Optional & 1u) == 0, "stream 0 is always there");
  for (long w = blockIdx.x; w < nwork; w += gridDim.x) {
    const cft_optim_work_t wk = work[w];
    const float* base[N];
    const long rem = row(wk, base) - wk.start;
    const int cnt = rem < (long)chunk ? (int)rem : chunk;
    gfloat* a[N];
    bool has[N], wide = cnt == chunk;
#pragma unroll
    for (int s = 0; s < N; ++s) {
      has[s] = !(Optional >> s & 1) || base[s] != nullptr;
      a[s] = has[s] ? as_global(base[s]) + wk.start : nullptr;
      wide = wide && aligned16(a[s]);
    }
    if (wide) {
      for (int i = threadIdx.x * 4; i < chunk; i += kThreads * 4) {        // chunk % 1024 == 0: no tail
        f32x4_t v[N];
#pragma unroll
        for (int s = 0; s < N; ++s) v[s] = has[s] ? *reinterpret_cast<const gfloat4*>(a[s] + i) : f32x4_t{0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int k = 0; k < 4; ++k) {
          float x[N];
#pragma unroll
          for (int s = 0; s < N; ++s) x[s] = v[s][k];
          rule(x);
#pragma unroll
          for (int s = 0; s < N; ++s)
            if (Written >> s & 1) v[s][k] = x[s];
        }
#pragma unroll
        for (int s = 0; s < N; ++s)
          if ((Written >> s & 1) && has[s]) *reinterpret_cast<gfloat4*>(a[s] + i) = v[s];
      }
    } else {
      for (int i = threadIdx.x; i < cnt; i += kThreads) {
        // An absent stream reads stream 0 again and drops the value: no branch between the loads.  With one, the compiler split
        // this loop in two and then kept the third 16-byte load of the loop above waiting for the stores of the pass before it.
        float x[N];
#pragma unroll
        for (int s = 0; s < N; ++s) {
          const float t = (has[s] ? a[s] : a[0])[i];
          x[s] = has[s] ? t : 0.0f;
        }
        rule(x);
#pragma unroll
        for (int s = 0; s < N; ++s)
          if ((Written >> s & 1) && has[s]) a[s][i] = x[s];
      }
    }
  }
}

__global__ void __launch_bounds__(kThreads)
sgd_step_kernel(const cft_sgd_seg_t* __restrict__ segs, const cft_optim_work_t* __restrict__ work, long nwork, int chunk,
                SgdHyper h, const float* __restrict__ grad_scale, const float* __restrict__ found_inf) {
  if (found_inf != nullptr && *found_inf != 0.0f) return;        // the step GradScaler skips: nothing is written
  SgdCoef c;
  c.scale = grad_scale != nullptr;
  c.inv_scale = c.scale ? (float)(1.0 / (double)*grad_scale) : 1.0f;
  walk_rows<3, 0b101, 0b100>(
      work, nwork, chunk,
      [&](const cft_optim_work_t& wk, const float* (&a)[3]) {
        const cft_sgd_seg_t s = segs[wk.seg];
        const int gi = (int)s.group;
        c.lr = h.lr[gi]; c.momentum = h.momentum[gi]; c.wd = h.wd[gi]; c.nesterov = h.nesterov[gi] != 0;
        a[0] = s.p; a[1] = s.g; a[2] = c.momentum != 0.0f ? s.buf : nullptr;
        return s.n;
      },
      [&](float (&x)[3]) { sgd_element(x[0], x[1], x[2], c); });
}

__global__ void __launch_bounds__(kThreads)
ema_update_kernel(const cft_ema_seg_t* __restrict__ segs, const cft_optim_work_t* __restrict__ work, long nwork, int chunk,
                  float d, float one_minus_d) {
  walk_rows<2, 0b01, 0>(
      work, nwork, chunk,
      [&](const cft_optim_work_t& wk, const float* (&a)[2]) {
        const cft_ema_seg_t s = segs[wk.seg];
        a[0] = s.e; a[1] = s.m;
        return s.n;
      },
      [&](float (&x)[2]) { x[0] = __builtin_fmaf(one_minus_d, x[1], d * x[0]); });
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
  walk_rows<4, 0b1101, 0>(
      work, nwork, chunk,
      [&](const cft_optim_work_t& wk, const float* (&a)[4]) {
        const cft_adam_seg_t s = segs[wk.seg];
        const int gi = (int)s.group;
        c.w1 = h.w1[gi]; c.b2 = h.b2[gi]; c.w2 = h.w2[gi]; c.eps = h.eps[gi]; c.wd = h.wd[gi]; c.decay = h.decay[gi];
        c.decoupled = h.decoupled[gi] != 0;
        const gfloat* __restrict__ co = as_global(coef) + 2 * (long)wk.seg;
        c.step_size = co[0]; c.bc2_sqrt = co[1];
        a[0] = s.p; a[1] = s.g; a[2] = s.m; a[3] = s.v;
        return s.n;
      },
      [&](float (&x)[4]) { adam_element(x[0], x[1], x[2], x[3], c); });
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

int fail(const char* who, const char* what, int row = -1) {
  char buf[200];
  if (row < 0) snprintf(buf, sizeof(buf), "%s: %s", who, what);
  else snprintf(buf, sizeof(buf), "%s: segment %d: %s", who, row, what);
  cft_set_error(buf);
  return CFT_EINVAL;
}

int blocks_for(long nwork, int max_blocks) {
  const long cap = max_blocks > 0 ? max_blocks : CFT_OPTIM_MAX_BLOCKS;
  return (int)(nwork < cap ? nwork : cap);
}

// The host side of all three entry points, in the order in which the checks fire: the table arguments, hyper() (the entry's own
// arguments: a status, its message set), every segment row (n, then row(s): what is wrong with it or nullptr), the work rows; then
// launch(segs, work, blocks) on the device copy of the table, unless there is no work.
template <typename Seg, typename Hyper, typename Row, typename Launch>
int with_table(const char* who, const void* table_dev, const void* table_host, int nseg, long nwork, int chunk, int max_blocks,
               Hyper hyper, Row row, Launch launch) {
  if (table_dev == nullptr || table_host == nullptr) return fail(who, "null table");
  if (nseg < 0 || nwork < 0) return fail(who, "negative segment or work count");
  if (nseg > (1 << 24) || nwork > (1L << 31)) return fail(who, "table too large");
  if (chunk < 1024 || chunk > (1 << 20) || chunk % 1024 != 0) return fail(who, "chunk must be a multiple of 1024 in [1024, 2^20]");
  if (max_blocks < 0 || max_blocks > 65536) return fail(who, "max_blocks outside [0, 65536]");
  if ((reinterpret_cast<uintptr_t>(table_dev) & 7u) != 0 || (reinterpret_cast<uintptr_t>(table_host) & 7u) != 0) return fail(who, "table not 8-byte aligned");
  const int st = hyper();
  if (st != CFT_OK) return st;
  const Seg* segs = static_cast<const Seg*>(table_host);
  for (int i = 0; i < nseg; ++i) {
    if (segs[i].n < 0) return fail(who, "negative element count", i);
    if (const char* bad = row(segs[i])) return fail(who, bad, i);
  }
  if (const char* bad = check_work(segs, nseg, reinterpret_cast<const cft_optim_work_t*>(segs + nseg), nwork, chunk)) return fail(who, bad);
  if (nwork == 0) return CFT_OK;
  const Seg* dsegs = static_cast<const Seg*>(table_dev);
  return launch(dsegs, reinterpret_cast<const cft_optim_work_t*>(dsegs + nseg), blocks_for(nwork, max_blocks));
}

}  // namespace

static_assert(sizeof(cft_sgd_seg_t) == CFT_SGD_SEG_BYTES && sizeof(cft_ema_seg_t) == CFT_EMA_SEG_BYTES &&
              sizeof(cft_adam_seg_t) == CFT_ADAM_SEG_BYTES && sizeof(cft_optim_work_t) == CFT_OPTIM_WORK_BYTES,
              "table row sizes are part of the ABI");

extern "C" int cft_sgd_step(const void* table_dev, const void* table_host, int nseg, long nwork, int chunk, int max_blocks,
                            const float* hyper_host, int ngroups, const float* grad_scale, const float* found_inf, void* stream) {
  SgdHyper h = {};
  return with_table<cft_sgd_seg_t>(
      "cft_sgd_step", table_dev, table_host, nseg, nwork, chunk, max_blocks,
      [&]() -> int {
        CFT_REQUIRE(hyper_host != nullptr, "cft_sgd_step: null hyper-parameter array");
        CFT_REQUIRE(ngroups >= 1 && ngroups <= CFT_OPTIM_MAX_GROUPS, "cft_sgd_step: 1 to 8 param groups");
        CFT_REQUIRE(word_aligned(grad_scale) && word_aligned(found_inf), "cft_sgd_step: grad_scale / found_inf not 4-byte aligned");
        for (int j = 0; j < ngroups; ++j) {
          h.lr[j] = hyper_host[4 * j]; h.momentum[j] = hyper_host[4 * j + 1]; h.wd[j] = hyper_host[4 * j + 2];
          const float nest = hyper_host[4 * j + 3];
          CFT_REQUIRE(nest == 0.0f || nest == 1.0f, "cft_sgd_step: the nesterov flag is 0 or 1");
          CFT_REQUIRE(!(h.lr[j] != h.lr[j]) && !(h.momentum[j] != h.momentum[j]) && !(h.wd[j] != h.wd[j]), "cft_sgd_step: NaN hyper-parameter");
          CFT_REQUIRE(nest == 0.0f || h.momentum[j] != 0.0f, "cft_sgd_step: nesterov needs a momentum");
          h.nesterov[j] = nest != 0.0f;
        }
        return CFT_OK;
      },
      [&](const cft_sgd_seg_t& s) -> const char* {
        if (s.group < 0 || s.group >= ngroups) return "group index out of range";
        if (s.p == nullptr || s.g == nullptr) return "null parameter or gradient";
        if (s.buf == nullptr && h.momentum[s.group] != 0.0f) return "no momentum buffer in a group with momentum";
        if (!word_aligned(s.p) || !word_aligned(s.g) || !word_aligned(s.buf)) return "pointer not 4-byte aligned";
        return nullptr;
      },
      [&](const cft_sgd_seg_t* segs, const cft_optim_work_t* work, int blocks) {
        hipLaunchKernelGGL(sgd_step_kernel, dim3(blocks), dim3(kThreads), 0, as_stream(stream), segs, work, nwork, chunk, h, grad_scale,
                           found_inf);
        return cft_check_launch("sgd_step_kernel");
      });
}

extern "C" int cft_ema_update(const void* table_dev, const void* table_host, int nseg, long nwork, int chunk, int max_blocks,
                              float d, float one_minus_d, void* stream) {
  return with_table<cft_ema_seg_t>(
      "cft_ema_update", table_dev, table_host, nseg, nwork, chunk, max_blocks,
      [&]() -> int {
        CFT_REQUIRE(!(d != d) && !(one_minus_d != one_minus_d), "cft_ema_update: NaN decay");
        return CFT_OK;
      },
      [&](const cft_ema_seg_t& s) -> const char* {
        if (s.e == nullptr || s.m == nullptr) return "null tensor";
        if (!word_aligned(s.e) || !word_aligned(s.m)) return "pointer not 4-byte aligned";
        return nullptr;
      },
      [&](const cft_ema_seg_t* segs, const cft_optim_work_t* work, int blocks) {
        hipLaunchKernelGGL(ema_update_kernel, dim3(blocks), dim3(kThreads), 0, as_stream(stream), segs, work, nwork, chunk, d, one_minus_d);
        return cft_check_launch("ema_update_kernel");
      });
}

extern "C" int cft_adam_step(const void* table_dev, const void* table_host, int nseg, long nwork, int chunk, int max_blocks,
                             const double* hyper_host, int ngroups, float* coef, const float* grad_scale, const float* found_inf,
                             void* stream) {
  AdamHyper h = {};
  AdamPrepare hp = {};
  return with_table<cft_adam_seg_t>(
      "cft_adam_step", table_dev, table_host, nseg, nwork, chunk, max_blocks,
      [&]() -> int {
        CFT_REQUIRE(hyper_host != nullptr, "cft_adam_step: null hyper-parameter array");
        CFT_REQUIRE(ngroups >= 1 && ngroups <= CFT_OPTIM_MAX_GROUPS, "cft_adam_step: 1 to 8 param groups");
        CFT_REQUIRE(coef != nullptr && (reinterpret_cast<uintptr_t>(coef) & 7u) == 0, "cft_adam_step: coef null or not 8-byte aligned");
        CFT_REQUIRE(word_aligned(grad_scale) && word_aligned(found_inf), "cft_adam_step: grad_scale / found_inf not 4-byte aligned");
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
        return CFT_OK;
      },
      [&](const cft_adam_seg_t& s) -> const char* {
        if (s.group < 0 || s.group >= ngroups) return "group index out of range";
        if (s.p == nullptr || s.g == nullptr) return "null parameter or gradient";
        if (s.m == nullptr || s.v == nullptr || s.step == nullptr) return "null moment or step counter";
        if (!word_aligned(s.p) || !word_aligned(s.g) || !word_aligned(s.m) || !word_aligned(s.v) || !word_aligned(s.step))
          return "pointer not 4-byte aligned";
        return nullptr;
      },
      [&](const cft_adam_seg_t* segs, const cft_optim_work_t* work, int blocks) {
        hipLaunchKernelGGL(adam_prepare_kernel, dim3((nseg + kThreads - 1) / kThreads), dim3(kThreads), 0, as_stream(stream), segs, nseg, hp,
                           coef, found_inf);
        const int sp = cft_check_launch("adam_prepare_kernel");
        if (sp != CFT_OK) return sp;
        hipLaunchKernelGGL(adam_step_kernel, dim3(blocks), dim3(kThreads), 0, as_stream(stream), segs, work, nwork, chunk, h,
                           (const float*)coef, grad_scale, found_inf);
        return cft_check_launch("adam_step_kernel");
      });
}
