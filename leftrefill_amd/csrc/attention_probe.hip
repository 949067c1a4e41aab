// Attention-map probe: where the softmax mass of a self-attention goes, without materialising the L x L matrix.
//
//   out[b, i, c] = beta * out[b, i, c] + alpha * (1/heads) * sum_h sum_j softmax_j(scale * q_h[b,i,:] . k_h[b,j,:]) * cols[j, c]
//
// i.e. attention with a tiny V (`cols`, <= 8 columns) that every sample and head shares, averaged over the heads.  It is a
// sibling of attention_kernel (attention.hip) and shares its first product, its K-tile staging and its online softmax
// (attention_common.h, FOLD = true: the map is built from the same P values the sampler's attention multiplies into V):
//
// * block = 4 waves = 128 queries of one sample (one 32-query block per wave); the block keeps its queries for ALL heads: per head
//   it streams the K sequence in 64-key tiles, S^T = K Q^T (8 x mfma 32x32x16) -> online softmax in registers ->
//   C^T += cols^T P^T (4 x mfma 32x32x16: ONE 32-row output block, rows >= ncols are zero), normalises by that head's row sum
//   and adds the head terms in head order in fp32.  No atomics, no workspace: a query's result is produced by one lane in a
//   fixed order, so two runs agree bit for bit.
// * cols^T tile in LDS: [32 rows][64 keys], 136-byte pitch (the V^T image of attention_kernel<VM = 0>); rows 8 .. 31 are zeroed
//   once, rows 0 .. 7 are refilled per tile through registers (16-bit loads, one key per thread and two columns per wave).
//   Keys past Nkv and columns past ncols are written as zeros, so a masked P = 0 never meets a stray NaN.
// * accumulator row c = (r & 3) + 8 (r >> 2) + 4 hi: columns 0 .. 3 are registers 0 .. 3 of the lower half-wave, columns 4 .. 7
//   registers 0 .. 3 of the upper one; the other twelve registers only ever hold zeros.
#include "attention_common.h"

#include <type_traits>

#define CT_PITCH 136                       // bytes per cols^T row (64 keys * 2 B + 8 pad)
#define PROBE_QB 128                       // queries per block
#define PROBE_MAX_COLS 8

template <typename T>
struct ProbeParams {
  const T* q; const T* k; const T* cols; float* out;
  int ldq, ldk, ldc, ncols, heads, Nq, Nkv, nqt;
  float c;        // scale * log2(e)
  float alpha_h;  // alpha / heads
  float beta;
};

template <typename T>
__global__ __launch_bounds__(ATT_THREADS) void attention_probe_kernel(const ProbeParams<T> P) {
  __shared__ __attribute__((aligned(16))) char smem[2 * ATT_KB * 128 + 2 * 32 * CT_PITCH];
  char* Ksm = smem;
  char* Csm = smem + 2 * ATT_KB * 128;

  const int t = threadIdx.x, lane = t & 63;
  const int w = __builtin_amdgcn_readfirstlane(t >> 6);
  const int qt = blockIdx.x % P.nqt, b = blockIdx.x / P.nqt;
  const T* zero = reinterpret_cast<const T*>(lr_zero_page);
  const unsigned short* colp = reinterpret_cast<const unsigned short*>(P.cols);

  const int ql = lane & 31, hi = lane >> 5;
  const int qrow = qt * PROBE_QB + w * 32 + ql;
  const int qc = min(qrow, P.Nq - 1);
  const int ntiles = (P.Nkv + ATT_KB - 1) / ATT_KB;
  const int nfull = P.Nkv / ATT_KB;

  // rows 8 .. 31 of both cols^T buffers stay zero for the whole kernel (made visible by the first barrier below)
  for (int i = t; i < 2 * 24 * (CT_PITCH / 4); i += ATT_THREADS) {
    const int buf = i / (24 * (CT_PITCH / 4)), j = i % (24 * (CT_PITCH / 4));
    *reinterpret_cast<unsigned*>(Csm + buf * (32 * CT_PITCH) + 8 * CT_PITCH + j * 4) = 0u;
  }

  // cols^T staging through registers: thread owns key t & 63 and columns 2 w, 2 w + 1
  const int ckey = lane, cc = 2 * w;
  auto load_c = [&](int tile, unsigned short& c0, unsigned short& c1) {
    const int key = tile * ATT_KB + ckey;
    const bool in = key < P.Nkv;
    c0 = in && cc < P.ncols ? colp[(size_t)key * P.ldc + cc] : (unsigned short)0;
    c1 = in && cc + 1 < P.ncols ? colp[(size_t)key * P.ldc + cc + 1] : (unsigned short)0;
  };
  auto write_c = [&](int buf, const unsigned short c0, const unsigned short c1) {
    char* Cs = Csm + buf * (32 * CT_PITCH);
    *reinterpret_cast<unsigned short*>(Cs + cc * CT_PITCH + ckey * 2) = c0;
    *reinterpret_cast<unsigned short*>(Cs + (cc + 1) * CT_PITCH + ckey * 2) = c1;
  };

  const f32x16 zero16 = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
  float total[4] = {0.f, 0.f, 0.f, 0.f};      // sum over heads of the normalised columns 4 hi .. 4 hi + 3 of this lane's query

  for (int h = 0; h < P.heads; ++h) {
    const T* qp = P.q + (size_t)b * P.Nq * P.ldq + h * 64;
    const T* kp = P.k + (size_t)b * P.Nkv * P.ldk + h * 64;
    vec8<T> qf[4];      // Q^T fragments: B-operand of mfma(K, Q^T): lane holds Q[q][s*16 + hi*8 .. +8], pre-multiplied by c
#pragma unroll
    for (int s4 = 0; s4 < 4; ++s4) qf[s4] = load_q<T, true>(qp + (size_t)qc * P.ldq + s4 * 16 + hi * 8, P.c);

    f32x16 cacc[1] = {zero16};
    f32x16 minit = zero16;
    float m_run = 0.f, l_run = 0.f;

    // every wave has passed the barrier that ends the previous head's last tile: both buffers are free
    attn_stage_k<T>(Ksm, kp, P.ldk, P.Nkv, 0, w, lane, zero);
    {
      unsigned short c0, c1;
      load_c(0, c0, c1);
      write_c(0, c0, c1);
    }
    __syncthreads();

    auto process_tile = [&](int tile, auto tail_tag) {
      constexpr bool TAIL = decltype(tail_tag)::value;
      const int cur = tile & 1;
      const bool more = tile + 1 < ntiles;
      unsigned short nc0 = 0, nc1 = 0;
      if (more) {
        attn_stage_k<T>(Ksm + (cur ^ 1) * (ATT_KB * 128), kp, P.ldk, P.Nkv, tile + 1, w, lane, zero);
        load_c(tile + 1, nc0, nc1);
      }
      const char* Ks = Ksm + cur * (ATT_KB * 128);
      const char* Cs = Csm + cur * (32 * CT_PITCH);

      // ---- S^T[key][q] = sum_d K[key][d] Q[q][d], as in attention_kernel
      f32x16 sacc[2];
#pragma unroll
      for (int s4 = 0; s4 < 4; ++s4)
#pragma unroll
        for (int kb = 0; kb < 2; ++kb) {
          const int row = kb * 32 + ql;
          const int kc = s4 * 2 + hi;
          const vec8<T> kf = *reinterpret_cast<const vec8<T>*>(Ks + row * 128 + ((kc ^ ((row >> 1) & 7)) << 4));
          sacc[kb] = lr_mfma32(kf, qf[s4], s4 == 0 ? minit : sacc[kb]);
        }
      // ---- mask the tail tile: accumulator reg r of block kb is key kb*32 + (r&3) + 8*(r>>2) + 4*hi
      if constexpr (TAIL) {
#pragma unroll
        for (int kb = 0; kb < 2; ++kb)
#pragma unroll
          for (int r = 0; r < 16; ++r) {
            const int key = tile * ATT_KB + kb * 32 + (r & 3) + 8 * (r >> 2) + 4 * hi;
            if (key >= P.Nkv) sacc[kb][r] = -INFINITY;
          }
      }
      vec8<T> pf[2][2];
      softmax_block<T, true, 1>(sacc, cacc, pf, m_run, l_run, minit, P.c, tile == 0);

      // ---- C^T[c][q] += sum_key cols^T[c][key] P^T[key][q]; k-slot (hi*8 + jj) of MFMA (kb, tt) is key
      //      kb*32 + 16*tt + 4*hi + jj (jj < 4) and kb*32 + 16*tt + 8 + 4*hi + (jj - 4) (jj >= 4)
#pragma unroll
      for (int kb = 0; kb < 2; ++kb)
#pragma unroll
        for (int tt = 0; tt < 2; ++tt) {
          const int key0 = kb * 32 + 16 * tt + 4 * hi;
          const vec4<T> va = *reinterpret_cast<const vec4<T>*>(Cs + ql * CT_PITCH + key0 * 2);
          const vec4<T> vb = *reinterpret_cast<const vec4<T>*>(Cs + ql * CT_PITCH + (key0 + 8) * 2);
          vec8<T> cf;
          cf[0] = va[0]; cf[1] = va[1]; cf[2] = va[2]; cf[3] = va[3];
          cf[4] = vb[0]; cf[5] = vb[1]; cf[6] = vb[2]; cf[7] = vb[3];
          cacc[0] = lr_mfma32(cf, pf[kb][tt], cacc[0]);
        }
      if (more) write_c(cur ^ 1, nc0, nc1);
      __syncthreads();
    };
    for (int tile = 0; tile < nfull; ++tile) process_tile(tile, std::false_type{});
    if (nfull < ntiles) process_tile(nfull, std::true_type{});

    // ---- this head's term: C^T / l, the row sum of the query being the sum of its two half-waves
    float lt = l_run;
    {
      const unsigned u = __builtin_bit_cast(unsigned, lt);
      const auto sw = __builtin_amdgcn_permlane32_swap(u, u, false, false);
      lt = __builtin_bit_cast(float, (unsigned)sw[0]) + __builtin_bit_cast(float, (unsigned)sw[1]);
    }
    const float inv = 1.0f / lt;
#pragma unroll
    for (int r = 0; r < 4; ++r) total[r] += cacc[0][r] * inv;
  }

  if (qrow < P.Nq) {
    float* op = P.out + ((size_t)b * P.Nq + qrow) * P.ncols;
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int c = 4 * hi + r;
      if (c < P.ncols) {
        float v = P.alpha_h * total[r];
        if (P.beta != 0.f) v = fmaf(P.beta, op[c], v);      // beta == 0: out is never read (it may be uninitialised)
        op[c] = v;
      }
    }
  }
}

template <typename T>
static int lr_attention_probe_t(const lr_half* q, int ldq, const lr_half* k, int ldk, const lr_half* cols, int ldc, int ncols,
                                float* out, int B, int heads, int Nq, int Nkv, float scale, float alpha, float beta, lr_stream_t s) {
  if (!q || !k || !cols || !out || B <= 0 || heads <= 0 || Nq <= 0 || Nkv <= 0) return LR_E_ARG;
  if (ncols < 1 || ncols > PROBE_MAX_COLS || ldc < ncols) return LR_E_ARG;
  if (ldq % 8 || ldk % 8) return LR_E_ALIGN;
  if (((uintptr_t)q | (uintptr_t)k) & 15) return LR_E_ALIGN;
  if (((uintptr_t)cols & 1) || ((uintptr_t)out & 3)) return LR_E_ALIGN;
  ProbeParams<T> P;
  P.q = (const T*)q; P.k = (const T*)k; P.cols = (const T*)cols; P.out = out;
  P.ldq = ldq; P.ldk = ldk; P.ldc = ldc; P.ncols = ncols;
  P.heads = heads; P.Nq = Nq; P.Nkv = Nkv;
  P.nqt = (Nq + PROBE_QB - 1) / PROBE_QB;
  P.c = scale * 1.44269504088896340736f;
  P.alpha_h = alpha / (float)heads;
  P.beta = beta;
  const long long nblocks = (long long)P.nqt * B;
  if (nblocks > 0x7fffffffLL) return LR_E_UNSUPPORTED;
  hipLaunchKernelGGL(attention_probe_kernel<T>, dim3((unsigned)nblocks), dim3(ATT_THREADS), 0, (hipStream_t)s, P);
  return lr_launch_status();
}

LR_ABI_PAIR(lr_attention_probe_f16, lr_attention_probe_bf16, (const lr_half* q, int ldq, const lr_half* k, int ldk, const lr_half* cols, int ldc, int ncols, float* out, int B, int heads, int Nq, int Nkv, float scale, float alpha, float beta, lr_stream_t s), lr_attention_probe_t<T>(q, ldq, k, ldk, cols, ldc, ncols, out, B, heads, Nq, Nkv, scale, alpha, beta, s))
