// Multi-head self-attention of the CFT block over ANY token count T (1 <= T <= 2048) for gfx950:
// O = softmax(Q K^T / sqrt(dk)) V per (image, head), flash-style (reference models/common.py:491-510 on a
// vert_anchors x horz_anchors grid, T = 2 * va * ha).  attention.hip keeps the T = 128 kernel that holds the whole
// score tile in registers; this one streams the keys in tiles of 64 and never forms more than a 64-key slice of S.
//
// Work split: one 256-thread workgroup per (image, head, query block); wave w owns QW = 16 * QT queries (QT = 2 for
// dkp <= 128, 1 above, so that Q, the O accumulators and one score slice fit the register file without spills).
// Q fragments are loaded once into registers.  Per 64-key tile the workgroup stages K (row-major, rows padded by 16 B:
// consecutive rows start in different banks) and V^T (head column-major, the same padding) in LDS, then each wave
//   S^T = K Q^T  : K fragments (row operand) from LDS, Q fragments (column operand) from registers; a lane holds,
//                  for ONE query (its column), 4 consecutive keys of each of the 4 key sub-tiles;
//   softmax      : online - per query, tile max in-lane over 16 values + two xor-shuffles; running max / sum updated;
//   O^T += V^T P^T: the lane's exponentials ARE its column-operand fragment (see attention.hip), V^T rows from LDS.
// Tail keys (k >= T) are staged as zero rows and their scores set to -inf; tail queries read row T-1 and are not stored.
//
// Numerics (what tests/test_gpu_cft_anchor_grid.py models in float64), per query row, tiles j = 0, 1, ...:
//   s_k   = fp32(q . k_k) * fp32(1/sqrt(dk))                     (fp32 MFMA accumulation over dkp)
//   m_j   = max(m_{j-1}, max_{k in tile j} s_k),  m_{-1} = -inf
//   e_k   = __expf(s_k - m_j)                                     (fp32, unrounded)
//   alpha = __expf(m_{j-1} - m_j)                                 (0 for the first tile)
//   l_j   = l_{j-1} * alpha + sum_{k in tile j} e_k               (fp32; the UNROUNDED, undropped exponentials)
//   p_k   = RNE_dtype(e_k * keep_k * fp32(1/(1-p)))               (the only rounding of P; keep_k = 1 at inference)
//   O_j   = O_{j-1} * alpha + sum_{k in tile j} p_k v_k           (rescale first, then the fp32 MFMA accumulation)
//   out   = RNE_dtype(O_last * fp32(1 / l_last))                  (one rounding of the output)
// At T = 128 and a single 64-key tile this is the existing kernel's arithmetic up to the split of the key sum.
// Dropout (training): keep_k = cft_hash32(seed, ((b * heads + h) * T + q) * T + k) >= thresh, the index in 64 bits;
// at T = 128 it is the index attention_kernel uses.
#include "cft_common.h"

template <typename T, int QT, int CT>   // CT = dkp / 16 exactly: every register array has a compile-time extent
__global__ void __launch_bounds__(256) attention_tokens_kernel(const unsigned char* __restrict__ qkv, unsigned char* __restrict__ out,
                                                               int T_tok, int heads, int dkp, float scale, uint32_t drop_thresh,
                                                               float inv_keep, unsigned long long seed) {
  constexpr int GE = Elem<T>::GE;
  constexpr int ES = (int)sizeof(T);
  constexpr int KB = 64;                   // keys per tile
  constexpr int KT = GE / 4;               // 16-key sub-tiles per MFMA k chunk (bf16/f16: 2, f32: 1)
  constexpr int NCH = 4 / KT;              // k chunks per tile
  constexpr int QW = 16 * QT;              // queries per wave
  constexpr int KSTEPS = CT * 16 / (4 * GE);  // MFMA k-steps over the head width
  constexpr int PS_B = KB * ES + 16;       // V^T row stride in bytes
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  const int KS_B = dkp * ES + 16;          // K row stride in bytes
  unsigned char* sK = smem;                // [KB][KS_B]
  unsigned char* sVT = smem + KB * KS_B;   // [dkp][PS_B]

  const int bh = blockIdx.x, b = bh / heads, head = bh - b * heads;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int lrow = lane & 15, lgrp = lane >> 4;
  const int G = dkp / GE;                  // granules per head row
  const long ldq_b = (long)3 * heads * dkp * ES;
  const long ldo_b = (long)heads * dkp * ES;
  const unsigned char* qbase = qkv + (long)b * T_tok * ldq_b + (long)head * dkp * ES;
  const unsigned char* kbase = qbase + (long)heads * dkp * ES;
  const unsigned char* vbase = kbase + (long)heads * dkp * ES;
  const int q0 = blockIdx.y * (4 * QW) + wave * QW;

  // ---- Q fragments -> registers (tail queries read the last row; they are never stored) ----
  gran_t qf[QT][KSTEPS];
#pragma unroll
  for (int i = 0; i < QT; ++i) {
    int row = q0 + i * 16 + lrow;
    row = row < T_tok ? row : T_tok - 1;
#pragma unroll
    for (int ks = 0; ks < KSTEPS; ++ks) qf[i][ks] = *reinterpret_cast<const gran_t*>(qbase + (long)row * ldq_b + (ks * 4 + lgrp) * 16);
  }

  float m_run[QT], l_run[QT];
  f32x4_t o[QT][CT];
#pragma unroll
  for (int i = 0; i < QT; ++i) {
    m_run[i] = -INFINITY;
    l_run[i] = 0.f;
#pragma unroll
    for (int j = 0; j < CT; ++j) o[i][j] = f32x4_t{0.f, 0.f, 0.f, 0.f};
  }

  for (int k0 = 0; k0 < T_tok; k0 += KB) {
    // ---- stage K and V^T of keys [k0, k0 + 64); keys >= T as zero rows ----
    __syncthreads();                       // the previous tile is consumed
    for (int i = tid; i < KB * G; i += 256) {
      const int t = i / G, kg = i - t * G;
      const bool live = k0 + t < T_tok;
      const long src = (long)(k0 + t) * ldq_b + kg * 16;
      const gran_t gk = live ? *reinterpret_cast<const gran_t*>(kbase + src) : gran_t{0u, 0u, 0u, 0u};
      const gran_t gv = live ? *reinterpret_cast<const gran_t*>(vbase + src) : gran_t{0u, 0u, 0u, 0u};
      *reinterpret_cast<gran_t*>(sK + t * KS_B + kg * 16) = gk;
      if constexpr (ES == 2) {
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          *reinterpret_cast<uint16_t*>(sVT + (kg * GE + 2 * e) * PS_B + t * 2) = (uint16_t)(gv[e] & 0xffffu);
          *reinterpret_cast<uint16_t*>(sVT + (kg * GE + 2 * e + 1) * PS_B + t * 2) = (uint16_t)(gv[e] >> 16);
        }
      } else {
#pragma unroll
        for (int e = 0; e < 4; ++e) *reinterpret_cast<uint32_t*>(sVT + (kg * GE + e) * PS_B + t * 4) = gv[e];
      }
    }
    __syncthreads();

    // ---- S^T = K Q^T: s[i][j][e] = score(query q0 + i*16 + lrow, key k0 + j*16 + lgrp*4 + e) ----
    f32x4_t s[QT][4];
#pragma unroll
    for (int i = 0; i < QT; ++i)
#pragma unroll
      for (int j = 0; j < 4; ++j) s[i][j] = f32x4_t{0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int ks = 0; ks < KSTEPS; ++ks) {
      const int kg = ks * 4 + lgrp;
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const gran_t kf = *reinterpret_cast<const gran_t*>(sK + (j * 16 + lrow) * KS_B + kg * 16);
#pragma unroll
        for (int i = 0; i < QT; ++i) s[i][j] = mma_granule<T>(kf, qf[i][ks], s[i][j]);
      }
    }

    // ---- online softmax over this tile ----
    const bool tail = k0 + KB > T_tok;
    gran_t pf[QT][NCH];
#pragma unroll
    for (int i = 0; i < QT; ++i) {
      float mx = -INFINITY;
#pragma unroll
      for (int j = 0; j < 4; ++j)
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          float v = s[i][j][e] * scale;
          if (tail && k0 + j * 16 + lgrp * 4 + e >= T_tok) v = -INFINITY;
          s[i][j][e] = v;
          mx = fmaxf(mx, v);
        }
      mx = fmaxf(mx, __shfl_xor(mx, 16));
      mx = fmaxf(mx, __shfl_xor(mx, 32));
      const float m_new = fmaxf(m_run[i], mx);        // finite: every tile holds at least one live key
      const float alpha = __expf(m_run[i] - m_new);   // exp(-inf) = 0 on the first tile
      m_run[i] = m_new;
      float sum = 0.f;
#pragma unroll
      for (int j = 0; j < 4; ++j)
#pragma unroll
        for (int e = 0; e < 4; ++e) { const float pv = __expf(s[i][j][e] - m_new); s[i][j][e] = pv; sum += pv; }
      sum += __shfl_xor(sum, 16);
      sum += __shfl_xor(sum, 32);
      l_run[i] = l_run[i] * alpha + sum;
#pragma unroll
      for (int j = 0; j < CT; ++j)
#pragma unroll
        for (int e = 0; e < 4; ++e) o[i][j][e] *= alpha;
      if (drop_thresh != 0u) {   // training: attn_drop on the probabilities; the normaliser is linear (see attention.hip)
        const unsigned long long qrow = ((unsigned long long)bh * T_tok + (unsigned long long)(q0 + i * 16 + lrow)) * (unsigned long long)T_tok;
        uint32_t keep = 0u;        // bit 4j + e: key k0 + j*16 + lgrp*4 + e kept (a rolled loop: 16 inlined hashes cost registers)
#pragma unroll 1
        for (int n = 0; n < 16; ++n)
          keep |= (cft_hash32(seed, qrow + (unsigned long long)(k0 + (n >> 2) * 16 + lgrp * 4 + (n & 3))) >= drop_thresh ? 1u : 0u) << n;
#pragma unroll
        for (int j = 0; j < 4; ++j)
#pragma unroll
          for (int e = 0; e < 4; ++e) s[i][j][e] = (keep >> (4 * j + e)) & 1u ? s[i][j][e] * inv_keep : 0.0f;
      }
#pragma unroll
      for (int c = 0; c < NCH; ++c) {
        if constexpr (ES == 2) {
          typedef Elem<typename Half16<T>::type> E16;
          pf[i][c] = gran_t{E16::pack2(s[i][2 * c][0], s[i][2 * c][1]), E16::pack2(s[i][2 * c][2], s[i][2 * c][3]),
                            E16::pack2(s[i][2 * c + 1][0], s[i][2 * c + 1][1]), E16::pack2(s[i][2 * c + 1][2], s[i][2 * c + 1][3])};
        } else {
          pf[i][c] = gran_t{__float_as_uint(s[i][c][0]), __float_as_uint(s[i][c][1]), __float_as_uint(s[i][c][2]), __float_as_uint(s[i][c][3])};
        }
      }
    }

    // ---- O^T += V^T P^T ----
#pragma unroll
    for (int c = 0; c < NCH; ++c) {
#pragma unroll
      for (int j = 0; j < CT; ++j) {
        const unsigned char* vrow = sVT + (j * 16 + lrow) * PS_B;
        gran_t vf;
        if constexpr (ES == 2) {   // keys (2c)*16 + lgrp*4 .. +3 and (2c+1)*16 + lgrp*4 .. +3: the slots of pf[.][c]
          const uint2 lo = *reinterpret_cast<const uint2*>(vrow + ((2 * c) * 16 + lgrp * 4) * 2);
          const uint2 hi = *reinterpret_cast<const uint2*>(vrow + ((2 * c + 1) * 16 + lgrp * 4) * 2);
          vf = gran_t{lo.x, lo.y, hi.x, hi.y};
        } else {
          vf = *reinterpret_cast<const gran_t*>(vrow + (c * 16 + lgrp * 4) * 4);
        }
#pragma unroll
        for (int i = 0; i < QT; ++i) o[i][j] = mma_granule<T>(vf, pf[i][c], o[i][j]);
      }
    }
  }

  // ---- out = O / l: o[i][j][e] = O(query q0 + i*16 + lrow, head column j*16 + lgrp*4 + e) ----
#pragma unroll
  for (int i = 0; i < QT; ++i) {
    const int row = q0 + i * 16 + lrow;
    if (row >= T_tok) continue;
    const float inv_sum = 1.0f / l_run[i];
#pragma unroll
    for (int j = 0; j < CT; ++j) {
      {
        float v[4];
#pragma unroll
        for (int e = 0; e < 4; ++e) v[e] = o[i][j][e] * inv_sum;
        unsigned char* dst = out + ((long)b * T_tok + row) * ldo_b + ((long)head * dkp + j * 16 + lgrp * 4) * ES;
        if constexpr (ES == 2) {
          typedef Elem<typename Half16<T>::type> E16;
          *reinterpret_cast<uint2*>(dst) = uint2{E16::pack2(v[0], v[1]), E16::pack2(v[2], v[3])};
        } else {
          *reinterpret_cast<f32x4_t*>(dst) = f32x4_t{v[0], v[1], v[2], v[3]};
        }
      }
    }
  }
}

template <typename T, int QT, int CT>
static void launch_attention_tokens(const void* qkv, void* out, int B, int T_tok, int heads, int dkp, float scale, uint32_t thresh,
                                    float inv_keep, unsigned long long seed, size_t smem, hipStream_t stream) {
  cft_allow_lds<&attention_tokens_kernel<T, QT, CT>>(160 * 1024);
  const int qblk = 4 * 16 * QT;
  hipLaunchKernelGGL((attention_tokens_kernel<T, QT, CT>), dim3(B * heads, (T_tok + qblk - 1) / qblk), dim3(256), smem, stream,
                     (const unsigned char*)qkv, (unsigned char*)out, T_tok, heads, dkp, scale, thresh, inv_keep, seed);
}

extern "C" int cft_attention_tokens(const void* qkv, void* out, int B, int T, int heads, int dk, int dkp,
                                    int dtype, float attn_pdrop, unsigned long long seed, void* stream) {
  CFT_REQUIRE(qkv && out, "cft_attention_tokens: null pointer");
  CFT_REQUIRE(attn_pdrop >= 0.0f && attn_pdrop < 1.0f, "cft_attention_tokens: attn_pdrop must be in [0, 1) (0 = inference)");
  CFT_REQUIRE(cft_is_dtype(dtype), "cft_attention_tokens: bad dtype");
  CFT_REQUIRE(T >= 1 && T <= 2048, "cft_attention_tokens: T must be in [1, 2048]");
  const int es = cft_elem_size(dtype);
  const int kstep = es == 2 ? 32 : 16;
  CFT_REQUIRE(B > 0 && heads > 0 && dk > 0 && dkp >= dk && dkp % kstep == 0 && dkp <= 256,
              "cft_attention_tokens: dkp must be a multiple of 32 (bf16, f16) / 16 (f32), >= dk, <= 256");
  CFT_REQUIRE((long)B * heads < (1L << 31), "cft_attention_tokens: too many (image, head) pairs");
  const size_t smem = (size_t)64 * (dkp * es + 16) + (size_t)dkp * (64 * es + 16);
  CFT_REQUIRE(smem <= 160 * 1024, "cft_attention_tokens: head too wide for LDS");
  const float scale = 1.0f / sqrtf((float)dk);
  const uint32_t thresh = (uint32_t)((double)attn_pdrop * 4294967296.0);
  const float inv_keep = 1.0f / (1.0f - attn_pdrop);
  const hipStream_t st = as_stream(stream);
#define ATT_TOK_CASE(T_, ct_)                                                                                          \
  case ct_:                                                                                                            \
    launch_attention_tokens<T_, (ct_ <= 8 ? 2 : 1), ct_>(qkv, out, B, T, heads, dkp, scale, thresh, inv_keep, seed, smem, st); \
    break;
  if (es == 2) {
    CFT_DISPATCH_DTYPE(dtype, T_, if constexpr (sizeof(T_) == 2) {
      switch (dkp / 16) { ATT_TOK_CASE(T_, 2) ATT_TOK_CASE(T_, 4) ATT_TOK_CASE(T_, 6) ATT_TOK_CASE(T_, 8) ATT_TOK_CASE(T_, 10)
                          ATT_TOK_CASE(T_, 12) ATT_TOK_CASE(T_, 14) ATT_TOK_CASE(T_, 16) }
    });
  } else {
    switch (dkp / 16) { ATT_TOK_CASE(float, 1) ATT_TOK_CASE(float, 2) ATT_TOK_CASE(float, 3) ATT_TOK_CASE(float, 4) ATT_TOK_CASE(float, 5)
                        ATT_TOK_CASE(float, 6) ATT_TOK_CASE(float, 7) ATT_TOK_CASE(float, 8) ATT_TOK_CASE(float, 9) ATT_TOK_CASE(float, 10)
                        ATT_TOK_CASE(float, 11) ATT_TOK_CASE(float, 12) ATT_TOK_CASE(float, 13) ATT_TOK_CASE(float, 14) ATT_TOK_CASE(float, 15)
                        ATT_TOK_CASE(float, 16) }
  }
#undef ATT_TOK_CASE
  return cft_check_launch("attention_tokens_kernel");
}
