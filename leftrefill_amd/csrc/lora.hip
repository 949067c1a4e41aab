// LoRA on the attention / GEGLU Linears: the three skinny products of the unmerged (training) route and the fp32 merge of the
// sampling route.  r = padded rank (32 | 64, the host pads the factors with zeros), X / dY are the wide [M, K | N] activations.
//
//   lr_lora_down   T[M, r]  = alpha * X[M, K] . A[r, K]^T       forward T = x down^T;  backward dT = scale * dY up  (A = up^T)
//   lr_lora_up     Y[M, N] (+)= T[M, r] . U[N, r]^T             forward y += T (scale up)^T;  backward dx += dT (down^T)^T
//   lr_lora_wgrad  D[r, C]  = alpha * P[M, r]^T . Q[M, C]       d up^T = scale * T^T dY;  d down = dT^T X     (fp32, split over M)
//   lr_lora_merge  W_eff    = W + alpha * B[N, R] . A[R, K]     fp32 VALU, any 1 <= R <= 64
//   lr_lora_*_drop the same three products with the LoRA dropout mask of the [M, N] branch regenerated in the kernel (Philox-4x32-10,
//                  one call per 4 consecutive logical columns of a row; leftrefill_amd/lora_dropout.py states it): on up's epilogue,
//                  on down's wide operand as it is loaded, on wgrad's Q chunks before they are staged.  A mask only zeroes; 1 / (1 - p)
//                  is an fp32 scalar.  Compile-time flag DROP: the unmasked instances carry none of it.
//
// down / up are read-bound streams of the wide operand: every MFMA operand (16x16x32, 8 consecutive k per lane) is ONE 16-byte global
// load of a row of X, T or a factor -- no LDS.  The product is formed transposed (factor rows on the accumulator's row index) so that a
// lane owns 4 consecutive columns of one output row (8-byte stores).
// wgrad contracts over the ROW index of both operands: the natural [32 rows][cols] tiles are staged in LDS as they lie in memory and the
// k-major fragments are gathered with ds_read_b64_tr_b16 (as attention_bwd.hip does for Q^T / dO^T): no transposed copies.  M is split
// over blockIdx.y into fp32 partials, summed in split order by a second launch: no atomics, bit-identical from run to run.
#include "common.h"
#include <cmath>

#define LORA_THREADS 256

template <typename T>
__device__ __forceinline__ vec8<T> lora_zero8() {
  return __builtin_bit_cast(vec8<T>, make_uint4(0u, 0u, 0u, 0u));
}

// ---- the dropout mask ---------------------------------------------------------------------------------------------------
// keep(row, col) = philox4x32_10((row, col >> 2, stream, draw), (seed lo, seed hi))[col & 3] >= thr, col the LOGICAL output feature
// (colgrp maps a packed group of 4 columns to its logical group; NULL = identity)
struct lora_mask {
  uint32_t k0, k1, stream, draw, thr;
  float inv_keep;
  const int32_t* colgrp;
};

// bit i: column 4 grp + i of `row` is kept.  10 rounds of 2 x (v_mul_hi_u32, v_mul_lo_u32); the Weyl key sequence is lane-uniform
__device__ __forceinline__ uint32_t lora_keep4(const lora_mask& mk, uint32_t row, uint32_t grp) {
  uint32_t c0 = row, c1 = grp, c2 = mk.stream, c3 = mk.draw, k0 = mk.k0, k1 = mk.k1;
#pragma unroll
  for (int r = 0; r < 10; ++r) {
    const uint32_t hi0 = __umulhi(0xD2511F53u, c0), lo0 = 0xD2511F53u * c0;
    const uint32_t hi1 = __umulhi(0xCD9E8D57u, c2), lo1 = 0xCD9E8D57u * c2;
    c0 = hi1 ^ c1 ^ k0;
    c1 = lo1;
    c2 = hi0 ^ c3 ^ k1;
    c3 = lo0;
    k0 += 0x9E3779B9u;
    k1 += 0xBB67AE85u;
  }
  return (uint32_t)(c0 >= mk.thr) | ((uint32_t)(c1 >= mk.thr) << 1) | ((uint32_t)(c2 >= mk.thr) << 2) | ((uint32_t)(c3 >= mk.thr) << 3);
}

__device__ __forceinline__ uint32_t lora_grp(const lora_mask& mk, uint32_t g) { return mk.colgrp ? (uint32_t)mk.colgrp[g] : g; }

// 2 kept-bits -> the AND mask of the 32-bit word that holds the two 16-bit elements
__device__ __forceinline__ uint32_t lora_pair(uint32_t b) { return ((b & 1u) ? 0xffffu : 0u) | ((b & 2u) ? 0xffff0000u : 0u); }

// 8 consecutive columns col .. col + 7 (col % 8 == 0) of `row`, masked-out elements set to +0: two Philox calls
__device__ __forceinline__ uint4 lora_mask8(uint4 v, const lora_mask& mk, uint32_t row, uint32_t col) {
  const uint32_t b0 = lora_keep4(mk, row, lora_grp(mk, col >> 2)), b1 = lora_keep4(mk, row, lora_grp(mk, (col >> 2) + 1));
  v.x &= lora_pair(b0);
  v.y &= lora_pair(b0 >> 2);
  v.z &= lora_pair(b1);
  v.w &= lora_pair(b1 >> 2);
  return v;
}

// ---- T = alpha X A^T ---------------------------------------------------------------------------------------------------
// one wave = 16 rows of X against all NR * 16 factor rows; accumulator (reg, lane): T[m0 + (lane & 15)][16 j + 4 (lane >> 4) + reg]
// DROP: x is masked as it is loaded, at its own (row, column)
template <typename T, int NR, bool DROP>
__global__ __launch_bounds__(LORA_THREADS) void lora_down_kernel(const T* __restrict__ x, int ldx, const T* __restrict__ a, int lda,
                                                                 T* __restrict__ t, int ldt, int M, int K, float alpha, lora_mask mk) {
  const int lane = threadIdx.x & 63;
  const int w = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int m0 = (blockIdx.x * 4 + w) * 16;
  if (m0 >= M) return;      // (wave-uniform)
  const int mrow = m0 + (lane & 15), kq = (lane >> 4) * 8;
  const T* xp = x + (size_t)min(mrow, M - 1) * ldx + kq;
  const T* ap = a + (size_t)(lane & 15) * lda + kq;
  f32x4 acc[NR];
#pragma unroll
  for (int j = 0; j < NR; ++j) acc[j] = (f32x4){0.f, 0.f, 0.f, 0.f};
  const int kfull = K & ~31;
  for (int k0 = 0; k0 < kfull; k0 += 32) {
    vec8<T> xf = *reinterpret_cast<const vec8<T>*>(xp + k0);
    if constexpr (DROP) xf = __builtin_bit_cast(vec8<T>, lora_mask8(__builtin_bit_cast(uint4, xf), mk, min(mrow, M - 1), k0 + kq));
#pragma unroll
    for (int j = 0; j < NR; ++j)
      acc[j] = lr_mfma16(*reinterpret_cast<const vec8<T>*>(ap + (size_t)j * 16 * lda + k0), xf, acc[j]);
  }
  if (kfull < K) {      // K % 8 == 0: a lane's 8 columns are all inside K or all outside
    const bool in = kfull + kq < K;
    vec8<T> xf = in ? *reinterpret_cast<const vec8<T>*>(xp + kfull) : lora_zero8<T>();
    if constexpr (DROP) {
      if (in) xf = __builtin_bit_cast(vec8<T>, lora_mask8(__builtin_bit_cast(uint4, xf), mk, min(mrow, M - 1), kfull + kq));
    }
#pragma unroll
    for (int j = 0; j < NR; ++j) {
      const vec8<T> af = in ? *reinterpret_cast<const vec8<T>*>(ap + (size_t)j * 16 * lda + kfull) : lora_zero8<T>();
      acc[j] = lr_mfma16(af, xf, acc[j]);
    }
  }
  if (mrow < M) {
    T* tp = t + (size_t)mrow * ldt + 4 * (lane >> 4);
#pragma unroll
    for (int j = 0; j < NR; ++j) {
      vec4<T> o;
#pragma unroll
      for (int i = 0; i < 4; ++i) o[i] = (T)(acc[j][i] * alpha);
      *reinterpret_cast<vec4<T>*>(tp + j * 16) = o;
    }
  }
}

// ---- Y (+)= T U^T -------------------------------------------------------------------------------------------------------
// one wave = 16 rows of T (held in registers) against 256 columns of Y, 16 at a time; accumulator (reg, lane):
// Y[m0 + (lane & 15)][n0 + 4 (lane >> 4) + reg]
#define LORA_UP_COLS 256
// DROP: the mask sits in the epilogue -- a kept element takes inv_keep * acc, a dropped one keeps y's bits (accumulate) or is +0
template <typename T, int KS, bool DROP>
__global__ __launch_bounds__(LORA_THREADS) void lora_up_kernel(const T* __restrict__ t, int ldt, const T* __restrict__ u, int ldu,
                                                               T* __restrict__ y, int ldy, int M, int N, int accumulate, lora_mask mk) {
  const int lane = threadIdx.x & 63;
  const int w = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int m0 = (blockIdx.x * 4 + w) * 16;
  if (m0 >= M) return;      // (wave-uniform)
  const int mrow = m0 + (lane & 15), kq = (lane >> 4) * 8;
  vec8<T> tf[KS];
#pragma unroll
  for (int s = 0; s < KS; ++s) tf[s] = *reinterpret_cast<const vec8<T>*>(t + (size_t)min(mrow, M - 1) * ldt + s * 32 + kq);
  const int nb = blockIdx.y * LORA_UP_COLS, ne = min(N, nb + LORA_UP_COLS);
  for (int n0 = nb; n0 < ne; n0 += 16) {
    const T* up = u + (size_t)min(n0 + (lane & 15), N - 1) * ldu + kq;
    f32x4 acc = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int s = 0; s < KS; ++s) acc = lr_mfma16(*reinterpret_cast<const vec8<T>*>(up + s * 32), tf[s], acc);
    const int nn = n0 + 4 * (lane >> 4);      // N % 8 == 0: the lane's 4 columns are all inside N or all outside
    if (mrow < M && nn < N) {
      T* yp = y + (size_t)mrow * ldy + nn;
      if constexpr (DROP) {
        // fp32 product, fp32 sum and the 16-bit rounding stay three roundings, as the unmasked path's add + convert: contracted into one
        // mixed-precision fma (v_fma_mixlo_f16) the sum would round once, and inv_keep = 1 would not give the unmasked kernel's bits
#pragma clang fp contract(off)
        const uint32_t kb = lora_keep4(mk, mrow, lora_grp(mk, nn >> 2));
        vec4<T> o = __builtin_bit_cast(vec4<T>, make_uint2(0u, 0u));
        float base[4] = {0.f, 0.f, 0.f, 0.f};
        if (accumulate) {
          o = *reinterpret_cast<const vec4<T>*>(yp);
#pragma unroll
          for (int i = 0; i < 4; ++i) base[i] = (float)o[i];
        }
#pragma unroll
        for (int i = 0; i < 4; ++i)
          if ((kb >> i) & 1u) o[i] = (T)(acc[i] * mk.inv_keep + base[i]);
        *reinterpret_cast<vec4<T>*>(yp) = o;
        continue;
      }
      if (accumulate) {
        const vec4<T> old = *reinterpret_cast<const vec4<T>*>(yp);
#pragma unroll
        for (int i = 0; i < 4; ++i) acc[i] += (float)old[i];
      }
      vec4<T> o;
#pragma unroll
      for (int i = 0; i < 4; ++i) o[i] = (T)acc[i];
      *reinterpret_cast<vec4<T>*>(yp) = o;
    }
  }
}

// ---- D = alpha P^T Q ----------------------------------------------------------------------------------------------------
#define LORA_WG_COLS 128      // columns of Q per block (4 waves x 32)
#define LORA_WG_ROWS 32       // rows of P / Q per step = one MFMA k
#define LORA_WG_QS (LORA_WG_COLS * 2 + 16)      // LDS row strides in bytes: 16 B of padding keep the 4 rows of a transpose read off the same banks

template <typename T>
__device__ __forceinline__ vec8<T> lora_frag_tr(const char* tile, int stride, int col0, int lane) {
  typedef short s16x4 __attribute__((ext_vector_type(4)));
  typedef __attribute__((address_space(3))) s16x4* lds_s16x4_t;
  // 16-lane group g gathers rows 8 g .. 8 g + 7 (two [4 rows][16 columns] blocks): lane 4 q + p of the group addresses row q, columns
  // 4 p .. 4 p + 3, and receives column (lane & 15) of the four rows
  const int g = lane >> 4, q = (lane & 15) >> 2, p = lane & 3;
  const char* a = tile + (8 * g + q) * stride + (col0 + 4 * p) * 2;
  const vec4<T> va = __builtin_bit_cast(vec4<T>, __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_s16x4_t)a));
  const vec4<T> vb = __builtin_bit_cast(vec4<T>, __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_s16x4_t)(a + 4 * stride)));
  vec8<T> f;
  f[0] = va[0]; f[1] = va[1]; f[2] = va[2]; f[3] = va[3];
  f[4] = vb[0]; f[5] = vb[1]; f[6] = vb[2]; f[7] = vb[3];
  return f;
}

// grid (ceil(C / 128), splits); block (x, y) writes ws[y][NR * 16][C] columns 128 x .. : accumulator (reg, lane) of (i, ct) is
// r = 16 i + 4 (lane >> 4) + reg, c = c0 + 32 w + 16 ct + (lane & 15)
// DROP: the chunks of Q are masked before they are staged, at their own (row, column)
template <typename T, int NR, bool DROP>
__global__ __launch_bounds__(LORA_THREADS) void lora_wgrad_kernel(const T* __restrict__ p, int ldp, const T* __restrict__ q, int ldq,
                                                                  float* __restrict__ ws, int M, int C, int rows_per_split, lora_mask mk) {
  constexpr int RP = NR * 16, PS = RP * 2 + 16, PCH = RP / 8;      // PCH: 16-byte chunks of a P row
  __shared__ __attribute__((aligned(16))) char sp[LORA_WG_ROWS * PS];
  __shared__ __attribute__((aligned(16))) char sq[LORA_WG_ROWS * LORA_WG_QS];
  const int t = threadIdx.x, lane = t & 63;
  const int w = __builtin_amdgcn_readfirstlane(t >> 6);
  const int c0 = blockIdx.x * LORA_WG_COLS;
  const int mbeg = blockIdx.y * rows_per_split, mend = min(M, mbeg + rows_per_split);
  const uint4 z4 = make_uint4(0u, 0u, 0u, 0u);
  // staging: Q tile = 32 rows x 16 chunks (threads take chunks t and t + 256), P tile = 32 rows x PCH chunks (threads t < 32 PCH)
  const int qrow = t >> 4, qch = t & 15;
  const int prow = t / PCH, pch = t % PCH;
  const bool qcol_in = c0 + qch * 8 < C;      // C % 8 == 0: a chunk is all inside C or all outside
  uint4 gq0, gq1, gp;
  auto load = [&](int m) {
    const int r0 = m + qrow, r1 = m + 16 + qrow;
    gq0 = (qcol_in && r0 < mend) ? *reinterpret_cast<const uint4*>(q + (size_t)r0 * ldq + c0 + qch * 8) : z4;
    gq1 = (qcol_in && r1 < mend) ? *reinterpret_cast<const uint4*>(q + (size_t)r1 * ldq + c0 + qch * 8) : z4;
    if constexpr (DROP) {
      if (qcol_in && r0 < mend) gq0 = lora_mask8(gq0, mk, r0, c0 + qch * 8);
      if (qcol_in && r1 < mend) gq1 = lora_mask8(gq1, mk, r1, c0 + qch * 8);
    }
    gp = (prow < LORA_WG_ROWS && m + prow < mend) ? *reinterpret_cast<const uint4*>(p + (size_t)(m + prow) * ldp + pch * 8) : z4;
  };
  f32x4 acc[NR][2];
#pragma unroll
  for (int i = 0; i < NR; ++i)
#pragma unroll
    for (int ct = 0; ct < 2; ++ct) acc[i][ct] = (f32x4){0.f, 0.f, 0.f, 0.f};
  if (mbeg < mend) load(mbeg);
  for (int m = mbeg; m < mend; m += LORA_WG_ROWS) {
    __syncthreads();      // the previous step's reads are done
    *reinterpret_cast<uint4*>(sq + qrow * LORA_WG_QS + qch * 16) = gq0;
    *reinterpret_cast<uint4*>(sq + (qrow + 16) * LORA_WG_QS + qch * 16) = gq1;
    if (prow < LORA_WG_ROWS) *reinterpret_cast<uint4*>(sp + prow * PS + pch * 16) = gp;
    __syncthreads();
    if (m + LORA_WG_ROWS < mend) load(m + LORA_WG_ROWS);      // next tile's loads fly under this tile's MFMAs
    vec8<T> qf[2];
#pragma unroll
    for (int ct = 0; ct < 2; ++ct) qf[ct] = lora_frag_tr<T>(sq, LORA_WG_QS, w * 32 + ct * 16, lane);
#pragma unroll
    for (int i = 0; i < NR; ++i) {
      const vec8<T> pf = lora_frag_tr<T>(sp, PS, i * 16, lane);
#pragma unroll
      for (int ct = 0; ct < 2; ++ct) acc[i][ct] = lr_mfma16(pf, qf[ct], acc[i][ct]);
    }
  }
  float* wp = ws + (size_t)blockIdx.y * RP * C;
#pragma unroll
  for (int ct = 0; ct < 2; ++ct) {
    const int c = c0 + w * 32 + ct * 16 + (lane & 15);
    if (c < C) {
#pragma unroll
      for (int i = 0; i < NR; ++i)
#pragma unroll
        for (int r = 0; r < 4; ++r) wp[(size_t)(i * 16 + 4 * (lane >> 4) + r) * C + c] = acc[i][ct][r];
    }
  }
}

// D[r][c .. c + 3] = alpha * sum over the splits in order; one thread per 4 columns
__global__ void lora_wgrad_reduce_kernel(const float* __restrict__ ws, float* __restrict__ d, int ldd, int RP, int C, int splits, float alpha) {
  const long long id = blockIdx.x * (long long)blockDim.x + threadIdx.x;
  const int c4 = C / 4;
  if (id >= (long long)RP * c4) return;
  const int r = (int)(id / c4), c = (int)(id % c4) * 4;
  const float* src = ws + (size_t)r * C + c;
  f32x4 a = {0.f, 0.f, 0.f, 0.f};
  for (int s = 0; s < splits; ++s) a += *reinterpret_cast<const f32x4*>(src + (size_t)s * RP * C);
  *reinterpret_cast<f32x4*>(d + (size_t)r * ldd + c) = a * alpha;
}

// ---- W_eff = W + alpha B A (fp32) ---------------------------------------------------------------------------------------
__global__ void lora_merge_kernel(const float* __restrict__ wt, const float* __restrict__ b, const float* __restrict__ a,
                                  float* __restrict__ out, int N, int K, int R, float alpha) {
  const long long id = blockIdx.x * (long long)blockDim.x + threadIdx.x;
  const int k4 = K / 4;
  if (id >= (long long)N * k4) return;
  const int n = (int)(id / k4), k = (int)(id % k4) * 4;
  f32x4 acc = {0.f, 0.f, 0.f, 0.f};
  for (int r = 0; r < R; ++r) {
    const float bv = b[(size_t)n * R + r];
    const f32x4 av = *reinterpret_cast<const f32x4*>(a + (size_t)r * K + k);
#pragma unroll
    for (int i = 0; i < 4; ++i) acc[i] = fmaf(bv, av[i], acc[i]);
  }
  const f32x4 w4 = *reinterpret_cast<const f32x4*>(wt + (size_t)n * K + k);
  f32x4 o;
#pragma unroll
  for (int i = 0; i < 4; ++i) o[i] = acc[i] == 0.f ? w4[i] : fmaf(alpha, acc[i], w4[i]);      // a zero low-rank term leaves W's bits (-0.0 too)
  *reinterpret_cast<f32x4*>(out + (size_t)n * K + k) = o;
}

// ---- host ---------------------------------------------------------------------------------------------------------------
static inline bool lora_rank_ok(int R) { return R == 32 || R == 64; }
static inline bool lora_al16(const void* p) { return ((uintptr_t)p & 15) == 0; }

// the descriptor of a masked launch, checked: 1 / (1 - p) must go with the threshold floor(p 2^32) (LR_E_ARG otherwise)
static int lora_mask_of(const lr_lora_drop* d, lora_mask* mk) {
  if (!d) return LR_E_ARG;
  if (!(d->inv_keep >= 1.f) || !std::isfinite(d->inv_keep)) return LR_E_ARG;
  const double keep = 1.0 - (double)d->threshold / 4294967296.0;
  if (std::fabs((double)d->inv_keep * keep - 1.0) > 1e-3) return LR_E_ARG;
  if ((uintptr_t)d->colgrp & 3) return LR_E_ALIGN;
  *mk = lora_mask{(uint32_t)(d->seed & 0xffffffffull), (uint32_t)(d->seed >> 32), d->stream, d->draw, d->threshold, d->inv_keep, d->colgrp};
  return 0;
}

template <typename T, bool DROP>
static int lora_down_t(const lr_half* x, int ldx, const lr_half* a, int lda, lr_half* t, int ldt, int M, int K, int R, float alpha,
                       const lr_lora_drop* drop, lr_stream_t s) {
  if (!x || !a || !t || M <= 0 || K <= 0 || ldx < K || lda < K || ldt < R) return LR_E_ARG;
  if (!lora_rank_ok(R)) return LR_E_UNSUPPORTED;
  if (K % 8 || ldx % 8 || lda % 8 || ldt % 8 || !lora_al16(x) || !lora_al16(a) || !lora_al16(t)) return LR_E_ALIGN;
  lora_mask mk = {};
  if (DROP) {
    const int rc = lora_mask_of(drop, &mk);
    if (rc) return rc;
  }
  const dim3 grid((M + 63) / 64), block(LORA_THREADS);
  hipStream_t st = (hipStream_t)s;
  if (R == 32) hipLaunchKernelGGL((lora_down_kernel<T, 2, DROP>), grid, block, 0, st, (const T*)x, ldx, (const T*)a, lda, (T*)t, ldt, M, K, alpha, mk);
  else hipLaunchKernelGGL((lora_down_kernel<T, 4, DROP>), grid, block, 0, st, (const T*)x, ldx, (const T*)a, lda, (T*)t, ldt, M, K, alpha, mk);
  return lr_launch_status();
}

template <typename T, bool DROP>
static int lora_up_t(const lr_half* t, int ldt, const lr_half* u, int ldu, lr_half* y, int ldy, int M, int N, int R, int accumulate,
                     const lr_lora_drop* drop, lr_stream_t s) {
  if (!t || !u || !y || M <= 0 || N <= 0 || ldt < R || ldu < R || ldy < N) return LR_E_ARG;
  if (!lora_rank_ok(R)) return LR_E_UNSUPPORTED;
  if (N % 8 || ldt % 8 || ldu % 8 || ldy % 8 || !lora_al16(t) || !lora_al16(u) || !lora_al16(y)) return LR_E_ALIGN;
  lora_mask mk = {};
  if (DROP) {
    const int rc = lora_mask_of(drop, &mk);
    if (rc) return rc;
  }
  const dim3 grid((M + 63) / 64, (N + LORA_UP_COLS - 1) / LORA_UP_COLS), block(LORA_THREADS);
  hipStream_t st = (hipStream_t)s;
  if (R == 32) hipLaunchKernelGGL((lora_up_kernel<T, 1, DROP>), grid, block, 0, st, (const T*)t, ldt, (const T*)u, ldu, (T*)y, ldy, M, N, accumulate, mk);
  else hipLaunchKernelGGL((lora_up_kernel<T, 2, DROP>), grid, block, 0, st, (const T*)t, ldt, (const T*)u, ldu, (T*)y, ldy, M, N, accumulate, mk);
  return lr_launch_status();
}

// how M is split: a pure function of the shape (the sum order is fixed).  About 1024 blocks in all, at least one 32-row step each.
static void lora_wgrad_plan(int M, int C, int* splits, int* rows_per_split) {
  const int ncb = (C + LORA_WG_COLS - 1) / LORA_WG_COLS;
  const int steps = (M + LORA_WG_ROWS - 1) / LORA_WG_ROWS;
  int want = 1024 / ncb;
  if (want < 1) want = 1;
  if (want > 512) want = 512;
  if (want > steps) want = steps;
  const int per = (steps + want - 1) / want;
  *rows_per_split = per * LORA_WG_ROWS;
  *splits = (steps + per - 1) / per;
}

extern "C" int64_t lr_lora_wgrad_workspace_bytes(int M, int R, int C) {
  if (M <= 0 || C <= 0 || !lora_rank_ok(R)) return LR_E_ARG;
  int splits, rows;
  lora_wgrad_plan(M, C, &splits, &rows);
  return (int64_t)splits * R * C * (int64_t)sizeof(float);
}

template <typename T, bool DROP>
static int lora_wgrad_t(const lr_half* p, int ldp, const lr_half* q, int ldq, float* d, int ldd, int M, int R, int C, float alpha,
                        void* workspace, int64_t workspace_bytes, const lr_lora_drop* drop, lr_stream_t s) {
  if (!p || !q || !d || !workspace || M <= 0 || C <= 0 || ldp < R || ldq < C || ldd < C) return LR_E_ARG;
  if (!lora_rank_ok(R)) return LR_E_UNSUPPORTED;
  if (C % 8 || ldp % 8 || ldq % 8 || ldd % 4 || !lora_al16(p) || !lora_al16(q) || !lora_al16(d) || !lora_al16(workspace)) return LR_E_ALIGN;
  int splits, rows;
  lora_wgrad_plan(M, C, &splits, &rows);
  if (workspace_bytes < (int64_t)splits * R * C * (int64_t)sizeof(float)) return LR_E_ARG;
  lora_mask mk = {};
  if (DROP) {
    const int rc = lora_mask_of(drop, &mk);
    if (rc) return rc;
  }
  const dim3 grid((C + LORA_WG_COLS - 1) / LORA_WG_COLS, splits), block(LORA_THREADS);
  hipStream_t st = (hipStream_t)s;
  float* ws = (float*)workspace;
  if (R == 32) hipLaunchKernelGGL((lora_wgrad_kernel<T, 2, DROP>), grid, block, 0, st, (const T*)p, ldp, (const T*)q, ldq, ws, M, C, rows, mk);
  else hipLaunchKernelGGL((lora_wgrad_kernel<T, 4, DROP>), grid, block, 0, st, (const T*)p, ldp, (const T*)q, ldq, ws, M, C, rows, mk);
  int rc = lr_launch_status();
  if (rc) return rc;
  const long long total = (long long)R * (C / 4);
  hipLaunchKernelGGL(lora_wgrad_reduce_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, st, ws, d, ldd, R, C, splits, alpha);
  return lr_launch_status();
}

extern "C" int lr_lora_merge_f32(const float* w, const float* b, const float* a, float* w_eff, int N, int K, int R, float alpha,
                                 lr_stream_t s) {
  if (!w || !b || !a || !w_eff || N <= 0 || K <= 0) return LR_E_ARG;
  if (R < 1 || R > 64) return LR_E_UNSUPPORTED;
  if (K % 4 || !lora_al16(w) || !lora_al16(a) || !lora_al16(w_eff) || ((uintptr_t)b & 3)) return LR_E_ALIGN;
  const long long total = (long long)N * (K / 4);
  hipLaunchKernelGGL(lora_merge_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, (hipStream_t)s, w, b, a, w_eff, N, K, R, alpha);
  return lr_launch_status();
}

// ---- C ABI: fp16 and bf16 forms, unmasked and masked ------------------------------------------------------------------------
LR_ABI_PAIR(lr_lora_down_f16, lr_lora_down_bf16, (const lr_half* x, int ldx, const lr_half* a, int lda, lr_half* t, int ldt, int M, int K, int R, float alpha, lr_stream_t s), lora_down_t<T, false>(x, ldx, a, lda, t, ldt, M, K, R, alpha, nullptr, s))
LR_ABI_PAIR(lr_lora_up_f16, lr_lora_up_bf16, (const lr_half* t, int ldt, const lr_half* u, int ldu, lr_half* y, int ldy, int M, int N, int R, int accumulate, lr_stream_t s), lora_up_t<T, false>(t, ldt, u, ldu, y, ldy, M, N, R, accumulate, nullptr, s))
LR_ABI_PAIR(lr_lora_wgrad_f16, lr_lora_wgrad_bf16, (const lr_half* p, int ldp, const lr_half* q, int ldq, float* d, int ldd, int M, int R, int C, float alpha, void* workspace, int64_t workspace_bytes, lr_stream_t s), lora_wgrad_t<T, false>(p, ldp, q, ldq, d, ldd, M, R, C, alpha, workspace, workspace_bytes, nullptr, s))
LR_ABI_PAIR(lr_lora_down_drop_f16, lr_lora_down_drop_bf16, (const lr_half* x, int ldx, const lr_half* a, int lda, lr_half* t, int ldt, int M, int K, int R, float alpha, const lr_lora_drop* drop, lr_stream_t s), lora_down_t<T, true>(x, ldx, a, lda, t, ldt, M, K, R, alpha, drop, s))
LR_ABI_PAIR(lr_lora_up_drop_f16, lr_lora_up_drop_bf16, (const lr_half* t, int ldt, const lr_half* u, int ldu, lr_half* y, int ldy, int M, int N, int R, int accumulate, const lr_lora_drop* drop, lr_stream_t s), lora_up_t<T, true>(t, ldt, u, ldu, y, ldy, M, N, R, accumulate, drop, s))
LR_ABI_PAIR(lr_lora_wgrad_drop_f16, lr_lora_wgrad_drop_bf16, (const lr_half* p, int ldp, const lr_half* q, int ldq, float* d, int ldd, int M, int R, int C, float alpha, void* workspace, int64_t workspace_bytes, const lr_lora_drop* drop, lr_stream_t s), lora_wgrad_t<T, true>(p, ldp, q, ldq, d, ldd, M, R, C, alpha, workspace, workspace_bytes, drop, s))
