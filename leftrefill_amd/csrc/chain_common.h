// Helpers shared by the register-chained fused blocks -- xattn_block.hip, xattn_block640.hip, ffn_block.hip, stin_block.hip and
// rowlin.hip.  One design: a wave keeps 16 (or 2 x 16) rows as B operands of swapped 16x16x32 MFMAs, weights stream through a 3-slot LDS
// ring, and the accumulators of one product are handed on as the B operand of the next.  Stated here once, for the kernels that
// take them (xattn_block640, ffn_block, stin_block): the row load, the LayerNorm of operand rows, the ring's lane addressing and fragment
// reader, bias staging and the XCD remap; GroupNorm-on-load tables (stin_block, rowlin); the cross-attention pair's parameter block and
// host fill.  xattn_block.hip and rowlin.hip keep their own device code (see their headers).
#pragma once
#include "common.h"

typedef __attribute__((address_space(3))) void* lptr_t;

template <int N> __device__ __forceinline__ void xa_wait_vmcnt() { asm volatile("s_waitcnt vmcnt(%0)" ::"n"(N) : "memory"); }

// reductions over the four lanes (fr, fq = 0..3) that share a row
__device__ __forceinline__ float xa_row4_sum(float v) {
#if defined(__HIP_DEVICE_COMPILE__)
  const unsigned u = __builtin_bit_cast(unsigned, v);
  const auto a = __builtin_amdgcn_permlane16_swap(u, u, false, false);
  v = __builtin_bit_cast(float, (unsigned)a[0]) + __builtin_bit_cast(float, (unsigned)a[1]);
  const unsigned u2 = __builtin_bit_cast(unsigned, v);
  const auto b = __builtin_amdgcn_permlane32_swap(u2, u2, false, false);
  v = __builtin_bit_cast(float, (unsigned)b[0]) + __builtin_bit_cast(float, (unsigned)b[1]);
#endif
  return v;
}
__device__ __forceinline__ float xa_row4_max(float v) {
#if defined(__HIP_DEVICE_COMPILE__)
  const unsigned u = __builtin_bit_cast(unsigned, v);
  const auto a = __builtin_amdgcn_permlane16_swap(u, u, false, false);
  v = fmaxf(__builtin_bit_cast(float, (unsigned)a[0]), __builtin_bit_cast(float, (unsigned)a[1]));
  const unsigned u2 = __builtin_bit_cast(unsigned, v);
  const auto b = __builtin_amdgcn_permlane32_swap(u2, u2, false, false);
  v = fmaxf(__builtin_bit_cast(float, (unsigned)b[0]), __builtin_bit_cast(float, (unsigned)b[1]));
#endif
  return v;
}

template <typename T>
__device__ __forceinline__ vec8<T> xa_pack(const f32x4& a, const f32x4& b) {
  vec8<T> r;
#pragma unroll
  for (int i = 0; i < 4; ++i) { r[i] = (T)a[i]; r[4 + i] = (T)b[i]; }
  return r;
}

// Two swapped-form accumulator tiles (A = columns 16 j .., B = columns 16 (j + 1) .. of the same 16 rows; lane (fr, fq) holds columns
// 4 fq .. + 3 of row fr in each) -> after the exchange the lane owns EIGHT consecutive columns of row fr: columns
// 16 (j + (fq & 1)) + 8 (fq >> 1) .. + 7, in (a[0..3], b[0..3]) (the register epilogue of gemm_common.h: one 16-byte store per lane).
__device__ __forceinline__ void xa_swap_rows16(f32x4& a, f32x4& b) {
#if defined(__HIP_DEVICE_COMPILE__)
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    const float ar = a[r], br = b[r];
    const auto s = __builtin_amdgcn_permlane16_swap(__builtin_bit_cast(unsigned, ar), __builtin_bit_cast(unsigned, br), false, false);
    a[r] = __builtin_bit_cast(float, (unsigned)s[0]);
    b[r] = __builtin_bit_cast(float, (unsigned)s[1]);
  }
#endif
}

// GroupNorm(32, affine) of a row-resident kernel's INPUT rows: per-channel scale / shift of sample n from the producer's per-group (sum,
// sumsq) partials gp [samples][chunks][32][2] -> LDS tables tabA / tabB [C].  Arithmetic of gn_apply_kernel (norm.hip), operation for
// operation -- chunk sums in fp64 by four lanes per group in the same order, mean / rstd rounded to fp32, a = rstd * gamma, b = beta - mean * a
// -- so `(T)fmaf(x, a, b)` on the rows equals what lr_groupnorm_apply_n would have written.  Block-wide (>= 128 threads); two barriers.
__device__ __forceinline__ void xa_gn_tables(const float* gp, int nchunks, int n, int HW, int C, const float* gamma, const float* beta,
                                             float eps, float* tabA, float* tabB, float* s_mr /* [64] */, int t, int nthreads) {
#if defined(__HIP_DEVICE_COMPILE__)
  const int Cg = C / 32;
  if (t < 128) {
    const int g = t >> 2, sub = t & 3;
    double s = 0.0, q = 0.0;
    const float* ps = gp + ((size_t)n * nchunks * 32 + g) * 2;
#pragma unroll 4
    for (int c = sub; c < nchunks; c += 4) { s += (double)ps[c * 64]; q += (double)ps[c * 64 + 1]; }
#pragma unroll
    for (int sh = 2; sh > 0; sh >>= 1) { s += __shfl_xor(s, sh, 64); q += __shfl_xor(q, sh, 64); }
    if (sub == 0) {
      const double cnt = (double)HW * (double)Cg;
      const double mean = s / cnt;
      double var = q / cnt - mean * mean;
      if (var < 0.0) var = 0.0;
      s_mr[g] = (float)mean;
      s_mr[32 + g] = (float)(1.0 / sqrt(var + (double)eps));
    }
  }
  __syncthreads();
  for (int c = t; c < C; c += nthreads) {
    const int g = c / Cg;
    const float a = s_mr[32 + g] * gamma[c];
    tabA[c] = a;
    tabB[c] = beta[c] - s_mr[g] * a;
  }
  __syncthreads();
#endif
}

// ---- operand rows ------------------------------------------------------------------------------------------------------------------
// One 16-row set in B-operand form: lane (fr, fq) holds x[row0 + fr][64 t5 + 32 u + 8 fq .. + 7]; rowptr = that row + 8 fq.  The four
// fq lanes of a row read 64 consecutive bytes, and the matching weight fragment of lane group fq is chunk 4 u + fq of sub-tile t5 --
// consecutive chunks across fq, which keeps the fragment's ds_read_b128 conflict-free (with chunk 2 fq + u every read took two LDS passes).
template <typename T, int KL>
__device__ __forceinline__ void xa_load_rows(vec8<T> (&xf)[KL][2], const T* rowptr) {
#if defined(__HIP_DEVICE_COMPILE__)
#pragma unroll
  for (int t5 = 0; t5 < KL; ++t5)
#pragma unroll
    for (int u = 0; u < 2; ++u) xf[t5][u] = *reinterpret_cast<const vec8<T>*>(rowptr + 64 * t5 + 32 * u);
#endif
}

// Two-pass LayerNorm of one row set in registers (C = 64 KL; gamma / beta are folded into the weights that follow).  TOUCH: an opaque
// touch between the passes makes each pass convert the 16-bit values again -- it keeps hipcc from holding the converted floats of a row
// set across the passes, which spilled 15 registers in stin_block.hip.  Callers with two row sets fence between them (sched_barrier).
template <typename T, int KL, bool TOUCH>
__device__ __forceinline__ void xa_layernorm_rows(vec8<T> (&xf)[KL][2], float eps) {
#if defined(__HIP_DEVICE_COMPILE__)
  constexpr int C = 64 * KL;
  float s = 0.f;
#pragma unroll
  for (int t5 = 0; t5 < KL; ++t5)
#pragma unroll
    for (int u = 0; u < 2; ++u)
#pragma unroll
      for (int i = 0; i < 8; ++i) s += (float)xf[t5][u][i];
  const float mean = xa_row4_sum(s) * (1.0f / C);
  if constexpr (TOUCH) {
#pragma unroll
    for (int t5 = 0; t5 < KL; ++t5)
#pragma unroll
      for (int u = 0; u < 2; ++u) asm volatile("" : "+v"(xf[t5][u]));
  }
  float q2 = 0.f;
#pragma unroll
  for (int t5 = 0; t5 < KL; ++t5)
#pragma unroll
    for (int u = 0; u < 2; ++u)
#pragma unroll
      for (int i = 0; i < 8; ++i) { const float d = (float)xf[t5][u][i] - mean; q2 = fmaf(d, d, q2); }
  const float rstd = rsqrtf(xa_row4_sum(q2) * (1.0f / C) + eps);
  const float nmr = -mean * rstd;
  if constexpr (TOUCH) {
#pragma unroll
    for (int t5 = 0; t5 < KL; ++t5)
#pragma unroll
      for (int u = 0; u < 2; ++u) asm volatile("" : "+v"(xf[t5][u]));
  }
#pragma unroll
  for (int t5 = 0; t5 < KL; ++t5)
#pragma unroll
    for (int u = 0; u < 2; ++u)
#pragma unroll
      for (int i = 0; i < 8; ++i) xf[t5][u][i] = (T)fmaf((float)xf[t5][u][i], rstd, nmr);
#endif
}

// ---- weight ring -------------------------------------------------------------------------------------------------------------------
// A ring slot holds 128-byte rows (64 k of one weight row).  An LDS-DMA instruction writes lane l's 16 bytes to (base + 16 l): the
// destination is linear, so the bank swizzle is applied on the SOURCE side.  The 64 lanes of wave w fill rows 8 w .. + 7 of a group of
// rows (lrow = 8 w + (lane >> 3)), and lane slot (lane & 7) of row r fetches chunk (lane & 7) ^ ((r >> 1) & 7): chunk c of row r lands
// in 16-byte slot c ^ ((r >> 1) & 7).  The swizzle uses bits 1 .. 3 of the row only, so it is the same for every row r + 16 i a piece
// places this lane's data in.  A fragment reader's rows are fr + a multiple of 16: its swizzle is the lane constant sw = (fr >> 1) & 7.
constexpr unsigned XA_OOB = 0x80000000u;      // buffer offset past every descriptor's range: the DMA writes zeros
__device__ __forceinline__ int xa_ring_row(int w, int lane) { return w * 8 + (lane >> 3); }
__device__ __forceinline__ int xa_ring_chunk(int lane, int lrow) { return (lane & 7) ^ ((lrow >> 1) & 7); }
template <typename T>
struct XaFrag {      // frag(base, row, chunk): A-operand fragment = chunk `chunk` of row `row` (fr + a multiple of 16) of the sub-tile at base
  int sw;
  __device__ __forceinline__ explicit XaFrag(int fr) : sw((fr >> 1) & 7) {}
  __device__ __forceinline__ vec8<T> operator()(const char* base, int row, int chunk) const {
    return *reinterpret_cast<const vec8<T>*>(base + row * 128 + ((chunk ^ sw) << 4));
  }
};

// Bias rows -> LDS behind the ring, segment after segment (lengths in floats, multiples of 4; a zero-length segment is skipped): the
// main loops issue no register loads, which would drain the LDS-DMA queue.
struct XaBiasSeg { const float* src; int n; };
template <int NTHREADS, int NSEG>
__device__ __forceinline__ void xa_stage_bias(float* par, const XaBiasSeg (&seg)[NSEG], int t) {
#if defined(__HIP_DEVICE_COMPILE__)
  int total = 0;
#pragma unroll
  for (int k = 0; k < NSEG; ++k) total += seg[k].n / 4;
  for (int i0 = 0; i0 < total; i0 += NTHREADS) {
    const int i = i0 + t;
    if (i < total) {
      const float* src = seg[0].src + 4 * i;
      int first = 0;
#pragma unroll
      for (int k = 1; k < NSEG; ++k) {
        first += seg[k - 1].n / 4;
        if (i >= first) src = seg[k].src + 4 * (i - first);
      }
      *reinterpret_cast<f32x4*>(par + 4 * i) = *reinterpret_cast<const f32x4*>(src);
    }
  }
#endif
}

// XCD-aware bijective remap of a linear block id: consecutive row blocks (one sample's K / V, one weight stream) stay on one XCD's L2
__device__ __forceinline__ int xa_xcd_remap(int bid, int nblocks) {
  const int q = nblocks >> 3, r = nblocks & 7, xcd = bid & 7;
  return (xcd < r ? xcd * (q + 1) : r * (q + 1) + (xcd - r) * q) + (bid >> 3);
}

// ---- the cross-attention pair (xattn_block.hip: C = 320, 128-row blocks; xattn_block640.hip: C = 640, 64-row blocks) ---------------------
struct XattnParams {
  const void* x; const void* wq; const float* bq; const void* k; const void* vt; const void* wo; const float* bo;
  void* out; float* st_out;
  const void* pre_a; const void* pre_w; const float* pre_b;      // PRE: x1 = pre_a pre_w^T + pre_b + x runs in front (xattn_block.hip)
  int M, HW, Lc, ldk, nblocks;
  float eps, c;               // c = scale * log2(e)
  unsigned k_bytes, vt_bytes;
#ifdef LR_XATTN_TRACE
  unsigned long long* trace;   // developer build only: shader-clock stamps [block][8 waves][24] (tools/trace_xattn.py)
#endif
};
// xattn_block640.hip: the C = 640 / 10-head instance of lr_xattn_block_f16 (64-row blocks, 4 waves); arguments already checked
int lr_xattn640_launch(const lr_xattn_args* a, int bf16_, lr_stream_t s);

// checked arguments -> parameter block for `rows`-row blocks; LR_E_UNSUPPORTED where K or the V^T pack exceed a 31-bit buffer range
static inline int xattn_fill_params(XattnParams& P, const lr_xattn_args* a, int rows, int heads) {
  const int B = a->M / a->HW;
  const int64_t kb = (int64_t)B * a->Lc * a->ldk * 2, vb = (int64_t)B * heads * 2 * 64 * 128;
  if (kb >= ((int64_t)1 << 31) || vb >= ((int64_t)1 << 31)) return LR_E_UNSUPPORTED;
  P.x = a->x; P.wq = a->wq; P.bq = a->bq; P.k = a->k; P.vt = a->vt; P.wo = a->wo; P.bo = a->bo; P.out = a->out;
  P.st_out = a->stats_out;
  P.pre_a = a->pre_a; P.pre_w = a->pre_w; P.pre_b = a->pre_b;
  P.M = a->M; P.HW = a->HW; P.Lc = a->Lc; P.ldk = a->ldk; P.nblocks = a->M / rows;
  P.eps = a->ln_eps; P.c = a->scale * 1.44269504088896340736f;
  P.k_bytes = (unsigned)kb; P.vt_bytes = (unsigned)vb;
#ifdef LR_XATTN_TRACE
  P.trace = nullptr;
#endif
  return 0;
}
