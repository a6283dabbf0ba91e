// utils/autoanchor.py of the reference on the GPU (train.py:220-221 runs it before the first step):
//   cft_anchor_metric   the ratio metric of check_anchors (:32-38) and kmean_anchors' print_results (:123-142): counts and sums;
//   cft_anchor_kmeans   scipy.cluster.vq.kmeans(obs, k, iter) as kmean_anchors calls it (:166), every restart on the device;
//   cft_anchor_evolve   the genetic loop of kmean_anchors (:185-199), the accept decision kept on the device.
// Every sum is either an integer sum (order-independent) or a float64 tree over a fixed partition: two runs give the same bits.
// No float atomics, no allocation, no synchronisation.
#include "cft_common.h"
#include <math.h>

#pragma clang fp contract(off)   // numpy's and scipy's a * b + c are two roundings: no fused multiply-adds here

typedef unsigned long long u64;

constexpr int AA_THREADS = 256;          // metric / fitness workgroup
constexpr int AA_WAVES = AA_THREADS / 64;
constexpr int AA_MAX_BLOCKS = 1024;
constexpr int AA_MAX_NA = 64;            // anchors (codes) per call
constexpr long AA_MAX_N = 1L << 24;      // labels per call: n * 2^29 stays exact in float64, counts stay exact in float32
constexpr int KM_THREADS = 1024;         // the one k-means workgroup
constexpr int KM_WAVES = KM_THREADS / 64;
constexpr int KM_MAX_ITERS = 100000;     // per restart; scipy has no cap, this one only bounds a run on non-finite input
constexpr double KM_THRESH = 1e-5;       // scipy's default thresh, which kmean_anchors leaves alone

// Fixed point.  A float32 in [2^-6, 1] is a multiple of 2^-29, so x * 2^29 is an integer: sums of terms above thr >= 2^-6 are exact
// integer sums.  An arbitrary x in [0, 1] is split into floor(x * 2^29) and the remainder in units of 2^-61, which holds every
// x >= 2^-38 exactly (smaller ones lose less than 2^-61 each, rounded toward zero).
constexpr float AA_SCALE = 536870912.0f;     // 2^29
constexpr float AA_SCALE_LO = 4294967296.0f; // 2^32

static inline size_t aa_align256(size_t x) { return (x + 255) & ~(size_t)255; }

// x = min over the two dims of min(r, 1 / r), r = wh / k: IEEE float32 divisions, as torch computes it on a CPU
__device__ __forceinline__ float ratio_metric(float2 p, float2 k) {
  const float r0 = p.x / k.x, r1 = p.y / k.y;
  return fminf(fminf(r0, 1.0f / r0), fminf(r1, 1.0f / r1));
}

__device__ __forceinline__ void split_add(float x, u64& hi, u64& lo) {
  const float s = x * AA_SCALE, fl = floorf(s);
  hi += (u64)fl;
  lo += (u64)((s - fl) * AA_SCALE_LO);
}

// Adds every workgroup total v[i] into out[i] with one integer atomic per value.
template <int V>
__device__ __forceinline__ void block_add_u64(u64 (&v)[V], u64* __restrict__ out) {
  __shared__ u64 s[V][AA_WAVES];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
#pragma unroll
  for (int i = 0; i < V; ++i) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) v[i] += __shfl_down(v[i], off);
    if (lane == 0) s[i][wave] = v[i];
  }
  __syncthreads();
  if (threadIdx.x < V) {
    u64 t = 0;
#pragma unroll
    for (int w = 0; w < AA_WAVES; ++w) t += s[threadIdx.x][w];
    if (t) atomicAdd(&out[threadIdx.x], t);
  }
}

// out[8] (accumulated into; the entry point zeroes it):
//   0 sum_i [best_i > thr]   1 sum_ij [x_ij > thr]
//   2, 3 sum x (units 2^-29, 2^-61)   4, 5 sum best (same units)   6 sum x[x > thr] (2^-29)   7 sum best[best > thr] (2^-29)
__global__ void __launch_bounds__(AA_THREADS) anchor_metric_kernel(const float2* __restrict__ wh, long n, const float* __restrict__ k, int na,
                                                                   float thr, u64* __restrict__ out) {
  __shared__ float2 s_k[AA_MAX_NA];
  const int tid = threadIdx.x;
  if (tid < na) s_k[tid] = make_float2(k[2 * tid], k[2 * tid + 1]);
  __syncthreads();
  u64 acc[8] = {0, 0, 0, 0, 0, 0, 0, 0};
  for (long i = (long)blockIdx.x * AA_THREADS + tid; i < n; i += (long)gridDim.x * AA_THREADS) {
    const float2 p = wh[i];
    float best = 0.f;
    for (int j = 0; j < na; ++j) {
      const float x = ratio_metric(p, s_k[j]);
      best = j == 0 ? x : fmaxf(best, x);
      split_add(x, acc[2], acc[3]);
      if (x > thr) { acc[1] += 1; acc[6] += (u64)(x * AA_SCALE); }
    }
    split_add(best, acc[4], acc[5]);
    if (best > thr) { acc[0] += 1; acc[7] += (u64)(best * AA_SCALE); }
  }
  block_add_u64<8>(acc, out);
}

extern "C" int cft_anchor_metric(const float* wh, long n, const float* k, int na, float thr, unsigned long long* out, void* stream) {
  CFT_REQUIRE(wh && k && out, "cft_anchor_metric: null pointer");
  CFT_REQUIRE(n >= 1 && n < AA_MAX_N, "cft_anchor_metric: n must be in [1, 2^24)");
  CFT_REQUIRE(na >= 1 && na <= AA_MAX_NA, "cft_anchor_metric: na must be in [1, 64]");
  CFT_REQUIRE(thr >= 0.015625f && thr <= 1.0f, "cft_anchor_metric: thr = 1 / anchor_t must be in [1/64, 1] (the exact sums need it)");
  CFT_REQUIRE(((size_t)wh & 7) == 0 && ((size_t)out & 7) == 0, "cft_anchor_metric: wh and out must be 8-byte aligned");
  if (hipMemsetAsync(out, 0, 8 * sizeof(u64), as_stream(stream)) != hipSuccess) return cft_check_launch("cft_anchor_metric: memset");
  const long blocks = (n + AA_THREADS - 1) / AA_THREADS;
  hipLaunchKernelGGL(anchor_metric_kernel, dim3((unsigned)(blocks < AA_MAX_BLOCKS ? blocks : AA_MAX_BLOCKS)), dim3(AA_THREADS), 0, as_stream(stream),
                     (const float2*)wh, n, k, na, thr, (u64*)out);
  return cft_check_launch("anchor_metric_kernel");
}

// ---- the genetic loop -------------------------------------------------------------------------------------------------------
// One launch per generation (and one for the fitness of the starting anchors), back to back on the stream.  Every workgroup forms
// the candidate kg = max(k * v, 2.0) in float64 (one multiplication), rounds it to float32 and adds its labels' fitness terms
// best * 2^29 (best > thr) into the generation's 64-bit integer; the workgroup that draws the last ticket forms
// fg = (float)((double)S / (2^29 * n)), accepts when fg > f (float32, strict) and then writes k and f for the next launch.
// Nobody waits for anybody: the last workgroup is whichever finishes last.
__global__ void __launch_bounds__(AA_THREADS) anchor_evolve_kernel(const float2* __restrict__ wh, long n, int na, float thr,
                                                                   const double* __restrict__ v, double* __restrict__ k, float* __restrict__ f,
                                                                   int* __restrict__ flag, float* __restrict__ fg_out, u64* __restrict__ S,
                                                                   unsigned int* __restrict__ ticket) {
  __shared__ float s_k[2 * AA_MAX_NA];
  __shared__ double s_kg[2 * AA_MAX_NA];
  __shared__ int s_accept;
  const int tid = threadIdx.x;
  if (tid < 2 * na) {
    double kg = k[tid];
    if (v) {
      kg = kg * v[tid];
      kg = fmax(kg, 2.0);
    }
    s_kg[tid] = kg;
    s_k[tid] = (float)kg;
  }
  if (tid == 0) s_accept = 0;
  __syncthreads();
  u64 acc[1] = {0};
  for (long i = (long)blockIdx.x * AA_THREADS + tid; i < n; i += (long)gridDim.x * AA_THREADS) {
    const float2 p = wh[i];
    float best = 0.f;
    for (int j = 0; j < na; ++j) {
      const float x = ratio_metric(p, make_float2(s_k[2 * j], s_k[2 * j + 1]));
      best = j == 0 ? x : fmaxf(best, x);
    }
    if (best > thr) acc[0] += (u64)(best * AA_SCALE);
  }
  block_add_u64<1>(acc, S);
  if (tid == 0) {
    __threadfence();                                   // this workgroup's sum and its reads of k come before its ticket
    const unsigned int t = atomicAdd(ticket, 1u);
    if (t == gridDim.x - 1) {
      __threadfence();
      const u64 total = __hip_atomic_load(S, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      const float fg = (float)((double)total / ((double)AA_SCALE * (double)n));
      if (!v) {
        f[0] = fg;
      } else {
        const int accept = fg > f[0];
        *flag = accept;
        *fg_out = fg;
        if (accept) f[0] = fg;
        s_accept = accept;
      }
    }
  }
  __syncthreads();
  if (s_accept && tid < 2 * na) k[tid] = s_kg[tid];
}

extern "C" int cft_anchor_evolve_workspace_bytes(int gen, long* bytes) {
  CFT_REQUIRE(bytes, "cft_anchor_evolve_workspace_bytes: null pointer");
  CFT_REQUIRE(gen >= 0 && gen <= (1 << 20), "cft_anchor_evolve_workspace_bytes: gen must be in [0, 2^20]");
  *bytes = (long)(aa_align256((size_t)(gen + 1) * 8) + aa_align256((size_t)(gen + 1) * 4));
  return CFT_OK;
}

extern "C" int cft_anchor_evolve(const float* wh, long n, int na, float thr, const double* v, int gen, double* k, float* f, int* flags,
                                 float* fg, void* workspace, long workspace_bytes, void* stream) {
  CFT_REQUIRE(wh && k && f && workspace && (gen == 0 || (v && flags && fg)), "cft_anchor_evolve: null pointer");
  CFT_REQUIRE(n >= 1 && n < AA_MAX_N, "cft_anchor_evolve: n must be in [1, 2^24)");
  CFT_REQUIRE(na >= 1 && na <= AA_MAX_NA, "cft_anchor_evolve: na must be in [1, 64]");
  CFT_REQUIRE(gen >= 0 && gen <= (1 << 20), "cft_anchor_evolve: gen must be in [0, 2^20]");
  CFT_REQUIRE(thr >= 0.015625f && thr <= 1.0f, "cft_anchor_evolve: thr = 1 / anchor_t must be in [1/64, 1] (the exact fitness needs it)");
  CFT_REQUIRE(((size_t)wh & 7) == 0 && ((size_t)workspace & 255) == 0, "cft_anchor_evolve: wh must be 8-byte, workspace 256-byte aligned");
  const size_t s_bytes = aa_align256((size_t)(gen + 1) * 8), need = s_bytes + aa_align256((size_t)(gen + 1) * 4);
  CFT_REQUIRE(workspace_bytes >= (long)need, "cft_anchor_evolve: workspace too small (see cft_anchor_evolve_workspace_bytes)");
  u64* S = (u64*)workspace;
  unsigned int* ticket = (unsigned int*)((char*)workspace + s_bytes);
  if (hipMemsetAsync(workspace, 0, need, as_stream(stream)) != hipSuccess) return cft_check_launch("cft_anchor_evolve: memset");
  const long nb = (n + AA_THREADS - 1) / AA_THREADS;
  const dim3 grid((unsigned)(nb < AA_MAX_BLOCKS ? nb : AA_MAX_BLOCKS));
  hipLaunchKernelGGL(anchor_evolve_kernel, grid, dim3(AA_THREADS), 0, as_stream(stream), (const float2*)wh, n, na, thr, (const double*)nullptr, k,
                     f, (int*)nullptr, (float*)nullptr, S, ticket);
  for (int g = 0; g < gen; ++g)
    hipLaunchKernelGGL(anchor_evolve_kernel, grid, dim3(AA_THREADS), 0, as_stream(stream), (const float2*)wh, n, na, thr, v + (size_t)g * 2 * na,
                       k, f, flags + g, fg + g, S + 1 + g, ticket + 1 + g);
  return cft_check_launch("anchor_evolve_kernel");
}

// ---- scipy.cluster.vq.kmeans -----------------------------------------------------------------------------------------------
// Sum of one double per thread over the workgroup, the same tree every time: 6 shuffle steps in each wave, then the 16 wave
// totals in order.  Every thread gets the total.
__device__ __forceinline__ double km_block_sum(double v, double* s_red) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) v += __shfl_down(v, off);
  if (lane == 0) s_red[wave] = v;
  __syncthreads();
  if (threadIdx.x == 0) {
    double t = 0.0;
    for (int w = 0; w < KM_WAVES; ++w) t += s_red[w];
    s_red[KM_WAVES] = t;
  }
  __syncthreads();
  const double t = s_red[KM_WAVES];
  __syncthreads();
  return t;
}

// One workgroup runs every restart: scipy's loop has no iteration bound, so its length is only known on the device.
//  _kpoints: the book starts as obs[idx[r, :]] (the host drew idx);  _vq.vq (nfeat < 5): squared distances d0 * d0 + d1 * d1 in
//  float64, the first strictly smallest wins, the distance is its square root;  the mean distance;  update_cluster_means: sum of
//  the members / their number, codes without members dropped (order kept);  stop when |previous mean - this mean| <= 1e-5,
//  the first previous mean being infinity;  the book of the restart with the strictly lowest last mean distance wins.
// Thread t owns the observations t, t + 1024, ...: it adds them in that order, and the workgroup adds the threads in a tree.
__global__ void __launch_bounds__(KM_THREADS) anchor_kmeans_kernel(const double2* __restrict__ obs, int n, int k, const int* __restrict__ idx,
                                                                   int iters, int* __restrict__ code,
                                                                   double* __restrict__ book_out, double* __restrict__ dist_out,
                                                                   int* __restrict__ info) {
  __shared__ double s_book[2 * AA_MAX_NA];
  __shared__ double s_new[2 * AA_MAX_NA];
  __shared__ int s_has[AA_MAX_NA];
  __shared__ double s_part[AA_MAX_NA][KM_WAVES][3];
  __shared__ double s_red[KM_WAVES + 1];
  __shared__ int s_kc;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  double best_dist = INFINITY;
  int total_it = 0, capped = 0;
  for (int r = 0; r < iters; ++r) {
    if (tid < k) {
      int first = idx[r * k + tid];
      first = first < 0 ? 0 : (first >= n ? n - 1 : first);      // the host draws them in [0, n)
      const double2 o = obs[first];
      s_book[2 * tid] = o.x;
      s_book[2 * tid + 1] = o.y;
    }
    __syncthreads();
    int kc = k;
    double prev = INFINITY, avg = INFINITY;
    for (int it = 0;; ++it) {
      double dsum = 0.0;
      for (int i = tid; i < n; i += KM_THREADS) {
        const double2 o = obs[i];
        double low = INFINITY;
        int c = -1;
        for (int j = 0; j < kc; ++j) {
          const double d0 = s_book[2 * j] - o.x, d1 = s_book[2 * j + 1] - o.y;
          double ds = d0 * d0;
          ds = ds + d1 * d1;
          if (ds < low) { low = ds; c = j; }
        }
        code[i] = c;
        dsum += sqrt(low);
      }
      avg = km_block_sum(dsum, s_red) / (double)n;
      for (int j = 0; j < kc; ++j) {
        double sx = 0.0, sy = 0.0, cnt = 0.0;
        for (int i = tid; i < n; i += KM_THREADS)     // code[i] was written by this thread
          if (code[i] == j) {
            const double2 o = obs[i];
            sx += o.x;
            sy += o.y;
            cnt += 1.0;
          }
#pragma unroll
        for (int off = 32; off > 0; off >>= 1) {
          sx += __shfl_down(sx, off);
          sy += __shfl_down(sy, off);
          cnt += __shfl_down(cnt, off);
        }
        if (lane == 0) {
          s_part[j][wave][0] = sx;
          s_part[j][wave][1] = sy;
          s_part[j][wave][2] = cnt;
        }
      }
      __syncthreads();
      if (tid < kc) {
        double sx = 0.0, sy = 0.0, cnt = 0.0;
        for (int w = 0; w < KM_WAVES; ++w) {
          sx += s_part[tid][w][0];
          sy += s_part[tid][w][1];
          cnt += s_part[tid][w][2];
        }
        s_has[tid] = cnt > 0.0;
        s_new[2 * tid] = sx / cnt;
        s_new[2 * tid + 1] = sy / cnt;
      }
      __syncthreads();
      if (tid == 0) {
        int m = 0;
        for (int j = 0; j < kc; ++j)
          if (s_has[j]) {
            s_book[2 * m] = s_new[2 * j];
            s_book[2 * m + 1] = s_new[2 * j + 1];
            ++m;
          }
        s_kc = m;
      }
      __syncthreads();
      kc = s_kc;
      ++total_it;
      const double diff = fabs(prev - avg);
      prev = avg;
      if (!(diff > KM_THRESH)) break;                     // uniform: every thread holds the same avg
      if (it + 1 >= KM_MAX_ITERS) { capped = 1; break; }
    }
    if (avg < best_dist) {
      best_dist = avg;
      if (tid < 2 * kc) book_out[tid] = s_book[tid];
      if (tid == 0) { info[0] = kc; info[1] = r; }
    }
    __syncthreads();
  }
  if (tid == 0) {
    dist_out[0] = best_dist;
    info[2] = total_it;
    info[3] = capped;
  }
}

extern "C" int cft_anchor_kmeans_workspace_bytes(long n, long* bytes) {
  CFT_REQUIRE(bytes, "cft_anchor_kmeans_workspace_bytes: null pointer");
  CFT_REQUIRE(n >= 1 && n < AA_MAX_N, "cft_anchor_kmeans_workspace_bytes: n must be in [1, 2^24)");
  *bytes = (long)aa_align256((size_t)n * 4);
  return CFT_OK;
}

extern "C" int cft_anchor_kmeans(const double* obs, long n, int k, const int* idx, int iters, void* workspace, long workspace_bytes,
                                 double* book, double* dist, int* info, void* stream) {
  CFT_REQUIRE(obs && idx && workspace && book && dist && info, "cft_anchor_kmeans: null pointer");
  CFT_REQUIRE(n >= 1 && n < AA_MAX_N, "cft_anchor_kmeans: n must be in [1, 2^24)");
  CFT_REQUIRE(k >= 1 && k <= AA_MAX_NA && k <= n, "cft_anchor_kmeans: k must be in [1, min(64, n)]");
  CFT_REQUIRE(iters >= 1 && iters <= 4096, "cft_anchor_kmeans: iter must be in [1, 4096]");
  CFT_REQUIRE(((size_t)obs & 15) == 0 && ((size_t)workspace & 255) == 0, "cft_anchor_kmeans: obs must be 16-byte, workspace 256-byte aligned");
  CFT_REQUIRE(workspace_bytes >= (long)aa_align256((size_t)n * 4), "cft_anchor_kmeans: workspace too small (see cft_anchor_kmeans_workspace_bytes)");
  if (hipMemsetAsync(info, 0, 4 * sizeof(int), as_stream(stream)) != hipSuccess) return cft_check_launch("cft_anchor_kmeans: memset");
  hipLaunchKernelGGL(anchor_kmeans_kernel, dim3(1), dim3(KM_THREADS), 0, as_stream(stream), (const double2*)obs, (int)n, k, idx, iters,
                     (int*)workspace, book, dist, info);
  return cft_check_launch("anchor_kmeans_kernel");
}
