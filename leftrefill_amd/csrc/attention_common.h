// Shared by the attention forward (attention.hip) and the attention-map probe (attention_probe.hip): tile sizes, the K-tile
// LDS-DMA staging and the online softmax of one 32-query block.  d_head = 64.
#pragma once
#include "common.h"

#define ATT_THREADS 256
#define ATT_QB 256
#define ATT_KB 64

typedef float f32x2 __attribute__((ext_vector_type(2)));
typedef const __attribute__((address_space(1))) void* gptr_t;
typedef __attribute__((address_space(3))) void* lptr_t;

// Online softmax of one 32-query block of a wave over one 64-key tile: S^T accumulators -> P^T (16-bit, the PV B operand), running
// max / sum, deferred rescale of O (only when some row's max grew by more than 2^8: P stays <= 256).  One query per lane; the
// partner lane ^ 32 holds the other half of the keys.
// FOLD = false: sacc holds raw q.k, m_run the raw running max (starts at -inf), p = exp2(c (s - m)).
// FOLD = true : Q was pre-multiplied by c = scale log2(e) and the accumulators were INITIALISED with -m_run (`minit`, the C operand of
//               the first QK^T MFMA), so sacc already is the exp2 argument: no per-element multiply-subtract (64 of the ~185
//               non-transcendental VALU instructions of a tile; the kernel is VALU-bound at d_head = 64).  m_run starts at 0 and the
//               first tile always takes the rescale path (sets m_run to the tile's row max).  Q's extra fp16 rounding moves a logit
//               by <= 2^-12 relative per term -- far inside the fp16 rounding of P; the training forward (log-sum-exp output for the
//               backward, which recomputes P from unscaled q, k) keeps FOLD = false.
// NDB = 32-row blocks of the second product's output per query block: 2 (O^T, d_head = 64) or 1 (the probe's cols^T P^T).
template <typename T, bool FOLD, int NDB = 2>
__device__ __forceinline__ void softmax_block(f32x16 (&sacc)[2], f32x16 (&oacc)[NDB], vec8<T> (&pf)[2][2], float& m_run, float& l_run,
                                              f32x16& minit, const float c, const bool first) {
  float mx = sacc[0][0];
#pragma unroll
  for (int kb = 0; kb < 2; ++kb)
#pragma unroll
    for (int r = 0; r < 16; ++r) mx = fmaxf(mx, sacc[kb][r]);
  {  // max across the two half-waves with one VALU lane swap (v_permlane32_swap) instead of an LDS round trip
    const unsigned u = __builtin_bit_cast(unsigned, mx);
    const auto sw = __builtin_amdgcn_permlane32_swap(u, u, false, false);
    mx = fmaxf(__builtin_bit_cast(float, (unsigned)sw[0]), __builtin_bit_cast(float, (unsigned)sw[1]));
  }
  if constexpr (FOLD) {
    if (first || !__all(mx <= 8.0f)) {
      const float d = first ? mx : fmaxf(mx, 0.f);
      const float alpha = first ? 1.f : __builtin_amdgcn_exp2f(-d);
      m_run += d;
      l_run *= alpha;
#pragma unroll
      for (int db = 0; db < NDB; ++db)
#pragma unroll
        for (int r = 0; r < 16; ++r) oacc[db][r] *= alpha;
#pragma unroll
      for (int kb = 0; kb < 2; ++kb)
#pragma unroll
        for (int r = 0; r < 16; ++r) sacc[kb][r] -= d;
#pragma unroll
      for (int r = 0; r < 16; ++r) minit[r] = -m_run;
    }
    float ps = 0.f;
#pragma unroll
    for (int kb = 0; kb < 2; ++kb)
#pragma unroll
      for (int r = 0; r < 16; r += 2) {
        const float p0 = __builtin_amdgcn_exp2f(sacc[kb][r]), p1 = __builtin_amdgcn_exp2f(sacc[kb][r + 1]);
        ps += p0 + p1;
        pf[kb][r >> 3][r & 7] = (T)p0;
        pf[kb][r >> 3][(r & 7) + 1] = (T)p1;
      }
    l_run += ps;
  } else {
    if (!__all((mx - m_run) * c <= 8.0f)) {
      const float m_new = fmaxf(m_run, mx);
      const float alpha = __builtin_amdgcn_exp2f((m_run - m_new) * c);
      m_run = m_new;
      l_run *= alpha;
#pragma unroll
      for (int db = 0; db < NDB; ++db)
#pragma unroll
        for (int r = 0; r < 16; ++r) oacc[db][r] *= alpha;
    }
    // packed fp32 math (v_pk_fma_f32 / v_pk_add_f32: two values per VALU issue) for the exp2 argument and the row sum
    const f32x2 c2 = {c, c};
    const f32x2 mc2 = {m_run * c, m_run * c};
    f32x2 ps2 = {0.f, 0.f};
#pragma unroll
    for (int kb = 0; kb < 2; ++kb)
#pragma unroll
      for (int r = 0; r < 16; r += 2) {
        const f32x2 sv = {sacc[kb][r], sacc[kb][r + 1]};
        const f32x2 a = __builtin_elementwise_fma(sv, c2, -mc2);
        const f32x2 pv = {__builtin_amdgcn_exp2f(a[0]), __builtin_amdgcn_exp2f(a[1])};
        ps2 += pv;
        pf[kb][r >> 3][r & 7] = (T)pv[0];
        pf[kb][r >> 3][(r & 7) + 1] = (T)pv[1];
      }
    l_run += ps2[0] + ps2[1];
  }
}

// Q^T fragment of a query row, pre-multiplied by c when the scale is folded into the operand (softmax_block<FOLD = true>)
template <typename T, bool FOLD>
__device__ __forceinline__ vec8<T> load_q(const T* p, const float c) {
  vec8<T> q = *reinterpret_cast<const vec8<T>*>(p);
  if constexpr (FOLD) {
#pragma unroll
    for (int i = 0; i < 8; ++i) q[i] = (T)((float)q[i] * c);
  }
  return q;
}


// K tile -> LDS: [64 keys][64 d], 128-byte rows, 16-byte LDS-DMA with the source-side XOR swizzle (slot = chunk ^ ((row >> 1) & 7)).
// 64 rows x 8 chunks = 512 x 16 B for a block of four waves: wave w, instr i covers rows (i*4 + w)*8 .. +8.  Keys past Nkv read zeros.
template <typename T>
__device__ __forceinline__ void attn_stage_k(char* Ks, const T* kp, const int ldk, const int Nkv, const int tile, const int w,
                                             const int lane, const T* zero) {
#pragma unroll
  for (int i = 0; i < 2; ++i) {
    const int rbase = (i * 4 + w) * 8;
    const int row = rbase + (lane >> 3);
    const int key = tile * ATT_KB + row;
    const int chunk = (lane & 7) ^ ((row >> 1) & 7);
    const T* g = key < Nkv ? kp + (size_t)key * ldk + chunk * 8 : zero;
    __builtin_amdgcn_global_load_lds((gptr_t)g, (lptr_t)(Ks + rbase * 128), 16, 0, 0);
  }
}
