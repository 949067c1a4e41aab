// Streaming kernels at the edges of the UNet step: layout converters, timestep embedding, the time-MLP
// (small-M linear), the re-arranged multi-view token gather/scatter and the fused CFG + DDIM update.
// All are HBM/launch bound; every global access is vectorised and coalesced.
#include "common.h"
#include <type_traits>

// ---------------------------------------------------------------------------------------------------------------
// NCHW fp32 -> NHWC fp16 (channel-padded).  One thread per (pixel, octet of output channels): the reads of one
// channel plane are coalesced across the 64 lanes of a wave (consecutive pixels), the 16-byte writes land in the
// pixel's row.  Cpad is a multiple of 8.
// ---------------------------------------------------------------------------------------------------------------
template <typename T>
__global__ void nchw_to_nhwc_kernel(const float* __restrict__ x1, int C1, const float* __restrict__ x2, int C2,
                                    T* __restrict__ y, int Cpad, int HW, long long total) {
  const int nOct = Cpad >> 3;
  for (long long idx = blockIdx.x * (long long)blockDim.x + threadIdx.x; idx < total;
       idx += (long long)gridDim.x * blockDim.x) {
    // idx = (n * nOct + o) * HW + p   (pixel fastest => coalesced plane reads)
    const int p = (int)(idx % HW);
    const long long q = idx / HW;
    const int o = (int)(q % nOct);
    const long long n = q / nOct;
    float f[8];
#pragma unroll
    for (int i = 0; i < 8; ++i) {
      const int c = o * 8 + i;
      float v = 0.f;
      if (c < C1) v = x1[((size_t)n * C1 + c) * HW + p];
      else if (c < C1 + C2) v = x2[((size_t)n * C2 + (c - C1)) * HW + p];
      f[i] = v;
    }
    *reinterpret_cast<uint4*>(y + ((size_t)n * HW + p) * Cpad + o * 8) = lr_pack8<T>(f);
  }
}

template <typename OutT, typename T>
__global__ void nhwc_to_nchw_kernel(const T* __restrict__ y, int Cstride, int C, OutT* __restrict__ out, int HW,
                                    long long total) {
  for (long long idx = blockIdx.x * (long long)blockDim.x + threadIdx.x; idx < total;
       idx += (long long)gridDim.x * blockDim.x) {
    const int p = (int)(idx % HW);
    const long long q = idx / HW;
    const int c = (int)(q % C);
    const long long n = q / C;
    out[idx] = (OutT)(float)y[((size_t)n * HW + p) * Cstride + c];
  }
}

// ---------------------------------------------------------------------------------------------------------------
// timestep_embedding (util.py:154-174): out[n][0:half] = cos(t * f_j), out[n][half:] = sin(t * f_j),
// f_j = exp(-ln(10000) * j / half), all in fp32 with the exact libm-class functions (t up to 999 rad: no fast-math).
// TT = int64_t (discrete-time samplers) or float (continuous-time samplers: DPM-Solver feeds t = 949.05, ...); an
// integer-valued float t gives the same bytes as the int64 entry.
// ---------------------------------------------------------------------------------------------------------------
template <typename TT, typename T>
__global__ void timestep_embedding_kernel(const TT* __restrict__ t, int N, int dim, T* __restrict__ out) {
  const int half = dim >> 1;
  const int idx = blockIdx.x * blockDim.x + threadIdx.x;
  if (idx >= N * half) return;
  const int n = idx / half, j = idx % half;
  const float freq = expf(-logf(10000.0f) * (float)j / (float)half);
  const float a = (float)t[n] * freq;
  out[(size_t)n * dim + j] = (T)cosf(a);
  out[(size_t)n * dim + half + j] = (T)sinf(a);
  if ((dim & 1) && j == 0) out[(size_t)n * dim + dim - 1] = (T)0.f;
}

// ---------------------------------------------------------------------------------------------------------------
// Small-M linear: out[m][n] = act_out(sum_k act_in(a[m][k]) w[n][k] + b[n]), M <= 16.  Weight-streaming bound:
// each wave owns output columns n, lanes split K in 16-byte pieces (coalesced 1 KiB per wave load), the (tiny)
// activation matrix is staged once per block in LDS with act_in applied.
// ---------------------------------------------------------------------------------------------------------------
template <int MMAX, typename T>
__global__ void linear_small_m_kernel(const T* __restrict__ a, int lda, const T* __restrict__ w,
                                      const float* __restrict__ bias, T* __restrict__ out, int ldo, int M, int N,
                                      int K, int act_in, int act_out, int cols_per_wave) {
  extern __shared__ __attribute__((aligned(16))) char smem_raw[];
  T* s_a = reinterpret_cast<T*>(smem_raw);  // [MMAX][K]
  const int t = threadIdx.x;
  const int K8 = K >> 3;
  if ((lda & 7) == 0 && (((uintptr_t)a) & 15) == 0) {      // 16-byte loads (round 6: the scalar staging loop was most of a batch-16 launch)
    for (int idx = t; idx < MMAX * K8; idx += blockDim.x) {
      const int m = idx / K8, k = (idx - m * K8) * 8;
      float v[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
      if (m < M) {
        lr_unpack8<T>(*reinterpret_cast<const uint4*>(a + (size_t)m * lda + k), v);
        if (act_in) {
#pragma unroll
          for (int i = 0; i < 8; ++i) v[i] = lr_silu(v[i]);
        }
      }
      *reinterpret_cast<uint4*>(s_a + m * K + k) = lr_pack8<T>(v);
    }
  } else {
    for (int idx = t; idx < MMAX * K; idx += blockDim.x) {
      const int m = idx / K, k = idx % K;
      float v = 0.f;
      if (m < M) {
        v = (float)a[(size_t)m * lda + k];
        if (act_in) v = lr_silu(v);
      }
      s_a[idx] = (T)v;
    }
  }
  __syncthreads();
  const int lane = t & 63, wave = t >> 6;
  const int nwaves = blockDim.x >> 6;
  const int n_begin = (blockIdx.x * nwaves + wave) * cols_per_wave;
  for (int n = n_begin; n < min(N, n_begin + cols_per_wave); ++n) {
    float acc[MMAX];
#pragma unroll
    for (int m = 0; m < MMAX; ++m) acc[m] = 0.f;
    for (int k = lane * 8; k < K; k += 64 * 8) {
      float wf[8];
      lr_unpack8<T>(*reinterpret_cast<const uint4*>(w + (size_t)n * K + k), wf);
#pragma unroll
      for (int m = 0; m < MMAX; ++m) {
        float af[8];
        lr_unpack8<T>(*reinterpret_cast<const uint4*>(s_a + m * K + k), af);
#pragma unroll
        for (int i = 0; i < 8; ++i) acc[m] = fmaf(af[i], wf[i], acc[m]);
      }
    }
#pragma unroll
    for (int m = 0; m < MMAX; ++m) acc[m] = lr_wave_sum(acc[m]);
    if (lane < M) {
      float v = 0.f;
#pragma unroll
      for (int m = 0; m < MMAX; ++m) if (m == lane) v = acc[m];
      if (bias) v += bias[n];
      if (act_out) v = lr_silu(v);
      out[(size_t)lane * ldo + n] = (T)v;
    }
  }
}

// ---------------------------------------------------------------------------------------------------------------
// Multi-view token re-arrangement, concat_target=True (multiview_attention.py:440-446 / 456-460).
// canvases x [b*v][s rows][2s cols][C]; sequence seq [b][(v+1)][s][s][C] = [target(from canvas 0), ref_0..ref_{v-1}].
// ---------------------------------------------------------------------------------------------------------------
// SUM = true is the backward of mv_scatter: the target slot collects the right halves of ALL canvases (fp32 sum).
template <bool SUM, typename T>
__global__ void mv_gather_kernel(const uint4* __restrict__ x, uint4* __restrict__ seq, int b, int v, int s, int C8,
                                 long long total) {
  for (long long idx = blockIdx.x * (long long)blockDim.x + threadIdx.x; idx < total;
       idx += (long long)gridDim.x * blockDim.x) {
    const int c = (int)(idx % C8);
    long long q = idx / C8;
    const int col = (int)(q % s); q /= s;
    const int row = (int)(q % s); q /= s;
    const int j = (int)(q % (v + 1));
    const long long bi = q / (v + 1);
    const int canvas = j == 0 ? 0 : j - 1;
    const int scol = j == 0 ? s + col : col;
    if (SUM && j == 0) {
      float acc[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
      for (int cv = 0; cv < v; ++cv) {
        float f[8];
        lr_unpack8<T>(x[((((size_t)bi * v + cv) * s + row) * (2 * s) + scol) * C8 + c], f);
#pragma unroll
        for (int i = 0; i < 8; ++i) acc[i] += f[i];
      }
      seq[idx] = lr_pack8<T>(acc);
    } else {
      seq[idx] = x[((((size_t)bi * v + canvas) * s + row) * (2 * s) + scol) * C8 + c];
    }
  }
}

// ZERO = true is the backward of mv_gather: only canvas 0 contributed its right half, the others receive zero there.
template <bool ZERO>
__global__ void mv_scatter_kernel(const uint4* __restrict__ seq, uint4* __restrict__ x, int b, int v, int s, int C8,
                                  long long total) {
  for (long long idx = blockIdx.x * (long long)blockDim.x + threadIdx.x; idx < total;
       idx += (long long)gridDim.x * blockDim.x) {
    const int c = (int)(idx % C8);
    long long q = idx / C8;
    const int col = (int)(q % (2 * s)); q /= (2 * s);
    const int row = (int)(q % s); q /= s;
    const int canvas = (int)(q % v);
    const long long bi = q / v;
    const int j = col >= s ? 0 : canvas + 1;
    const int scol = col >= s ? col - s : col;
    if (ZERO && col >= s && canvas != 0) x[idx] = make_uint4(0, 0, 0, 0);
    else x[idx] = seq[((((size_t)bi * (v + 1) + j) * s + row) * s + scol) * C8 + c];
  }
}

// ---------------------------------------------------------------------------------------------------------------
// Row copies with optional index tables (lr_row_copy): the glue of the canvas-sharded multi-view block -- packing rows + their
// LayerNorm statistics into one message, unpacking a received message into sequence order / this rank's own rows, writing the
// canvas back -- as ONE launch of up to four jobs instead of a dozen torch slice / cat / copy kernels.  8-byte granules.
// ---------------------------------------------------------------------------------------------------------------
struct RowCopyJobs { lr_row_copy_job j[4]; };
__global__ void row_copy_kernel(const RowCopyJobs J) {
  const lr_row_copy_job& jb = J.j[blockIdx.y];
  const int g8 = jb.row_bytes >> 3;                       // 8-byte granules per row
  const long long total = (long long)jb.n_rows * g8;
  for (long long idx = blockIdx.x * (long long)blockDim.x + threadIdx.x; idx < total; idx += (long long)gridDim.x * blockDim.x) {
    const int r = (int)(idx / g8), g = (int)(idx - (long long)r * g8);
    const long long sr = jb.src_idx ? jb.src_idx[r] : r, dr = jb.dst_idx ? jb.dst_idx[r] : r;
    const uint2 v = *reinterpret_cast<const uint2*>((const char*)jb.src + sr * jb.src_pitch + jb.src_off + (long long)g * 8);
    *reinterpret_cast<uint2*>((char*)jb.dst + dr * jb.dst_pitch + jb.dst_off + (long long)g * 8) = v;
  }
}

// ---------------------------------------------------------------------------------------------------------------
// Fused sampler updates (DDIM, PLMS, DPM-Solver++, DDIM inversion, three-way DDIM: CFG combine + update of the fp32 state; ancestral
// DDPM: posterior step of one eps), one pass.
// sampler_step_kernel owns the grid-stride loop and the loads of the eps slabs; a Step (below) holds its fp32 streams and scalars
// and loads, updates and stores the V elements of one thread (an optional stream is loaded where it is used, so each Step compiles
// to the code of a hand-written kernel).  V = 4: 16-byte fp32 / 8-byte 16-bit accesses (numel % 4 == 0, aligned buffers), V = 1: scalar.
// Every Step but DdimStep keeps the reference's order of operations op by op (no contraction into fma), so the fp32 result
// matches torch's eager evaluation of the same expression.
// ---------------------------------------------------------------------------------------------------------------
template <int V>
__device__ __forceinline__ void ld_f32(const float* __restrict__ p, long long i, float (&v)[V]) {
  if constexpr (V == 4) {
    const float4 q = *reinterpret_cast<const float4*>(p + i);
    v[0] = q.x; v[1] = q.y; v[2] = q.z; v[3] = q.w;
  } else {
    v[0] = p[i];
  }
}

template <int V>
__device__ __forceinline__ void st_f32(float* __restrict__ p, long long i, const float (&v)[V]) {
  if constexpr (V == 4) *reinterpret_cast<float4*>(p + i) = make_float4(v[0], v[1], v[2], v[3]);
  else p[i] = v[0];
}

template <int V, typename EpsT>
__device__ __forceinline__ void ld_eps(const EpsT* __restrict__ p, long long i, float (&v)[V]) {
  if constexpr (V == 4 && sizeof(EpsT) == 2) {
    const uint2 q = *reinterpret_cast<const uint2*>(p + i);
    const EpsT* h = reinterpret_cast<const EpsT*>(&q);
#pragma unroll
    for (int k = 0; k < 4; ++k) v[k] = (float)h[k];
  } else if constexpr (V == 4) {
    ld_f32<4>(reinterpret_cast<const float*>(p), i, v);
  } else {
    v[0] = (float)p[i];
  }
}

// A Step has NE eps slabs (eps [NE numel]: uncond, cond, ...), its fp32 streams of numel elements each -- in[] (in[0] = x) and
// out[]; a null pointer is an absent optional stream --, MAX_V (4, or 1 for a step that stays one element per thread) and
// apply<EpsT, T>(i, e): load the V elements at i of its inputs, map them and e to the outputs, store those.
template <int V, typename EpsT, typename T, typename Step>
__global__ void sampler_step_kernel(long long numel, const EpsT* __restrict__ eps, const Step s) {
  const long long groups = numel / V;
  for (long long g = blockIdx.x * (long long)blockDim.x + threadIdx.x; g < groups; g += (long long)gridDim.x * blockDim.x) {
    const long long i = g * V;
    float e[Step::NE][V];
#pragma unroll
    for (int j = 0; j < Step::NE; ++j) ld_eps<V, EpsT>(eps, j * numel + i, e[j]);
    s.template apply<EpsT, T>(i, e);
  }
}

// pred_x0 = (x - sqrt_1m_at e) / sqrt_at, x_prev = sqrt_aprev pred_x0 + dir_coef e + sigma noise: the coefficients of the DDIM
// update, formed in fp32 with sqrtf in the reference's order -- its schedule values are 0-dim / [b,1,1,1] fp32 tensors
// (ddim.py:359-381, :623-645; plms.py:204-223 with sigma = 0).
struct DdimCoefs { float sqrt_at, sqrt_1m_at, sqrt_aprev, dir_coef, sigma; };

static inline DdimCoefs ddim_coefs(float a_t, float a_prev, float sigma_t, float sqrt_one_minus_at) {
  return {sqrtf(a_t), sqrt_one_minus_at, sqrtf(a_prev), sqrtf(1.0f - a_prev - sigma_t * sigma_t), sigma_t};
}

// CFG combine + DDIM update (ddim.py:343-381), fp32 state, one element per thread.
// This step is deliberately compiled with the default floating-point contraction ON, while the steps after it are contract(off):
// x - sqrt_1m_at e, sqrt_aprev p0 + dir_coef e and + sigma noise are fused multiply-adds here (and so is the fp32-eps combine,
// which is why this step does not call cfg_combine), and they round differently from the separate multiply and add.  Every
// sample the default DDIM sampler has produced so far carries this rounding; the golden test of this step allows 2e-6, so it
// would NOT notice a switch to contract(off), a reordered expression or a call to cfg_combine.  Keep all three as they are.
struct DdimStep {
  static constexpr int NE = 2, MAX_V = 1;
  const float* in[2];      // x, noise (optional)
  float* out[2];           // x_prev, pred_x0
  float scale;
  DdimCoefs c;
  template <typename EpsT, typename T, int V>
  __device__ __forceinline__ void apply(long long i, const float (&e)[NE][V]) const {
    static_assert(V == 1);
    const float eu = e[0][0], ec = e[1][0];
    float ee;
    if constexpr (sizeof(EpsT) == 2) {
      // the reference's CFG combine runs in fp16 (model output dtype under autocast, ddim.py:343)
      const T d = (T)(ec - eu);
      const T sd = (T)(scale * (float)d);
      ee = (float)(T)(eu + (float)sd);
    } else {
      ee = eu + scale * (ec - eu);
    }
    const float xv = in[0][i];
    const float p0 = (xv - c.sqrt_1m_at * ee) / c.sqrt_at;
    float xp = c.sqrt_aprev * p0 + c.dir_coef * ee;
    if (in[1]) xp += c.sigma * in[1][i];
    out[1][i] = p0;
    out[0][i] = xp;
  }
};

// e = e_u + s (e_c - e_u), rounded in the eps dtype exactly as DdimStep does
template <typename EpsT, typename T>
__device__ __forceinline__ float cfg_combine(float eu, float ec, float scale) {
#pragma clang fp contract(off)
  if constexpr (sizeof(EpsT) == 2) {
    const T d = (T)(ec - eu);
    const T sd = (T)(scale * (float)d);
    return (float)(T)(eu + (float)sd);
  } else {
    return eu + scale * (ec - eu);
  }
}

// PLMS (pseudo linear multistep, sigma = 0): e' = (w0 e + w1 h1 + w2 h2 + w3 h3) / div over the n_hist newest history
// entries, then pred_x0 = (x - sqrt(1 - a_t) e') / sqrt(a_t), x_prev = sqrt(a_prev) pred_x0 + sqrt(1 - a_prev) e'.
struct PlmsStep {
  static constexpr int NE = 2, MAX_V = 4;
  const float* in[4];      // x, then the n_hist newest history entries (the rest null)
  float* out[3];           // e (optional): this evaluation's combined eps; x_prev; pred_x0
  int n_hist;
  float scale, w[4], div;
  DdimCoefs c;
  template <typename EpsT, typename T, int V>
  __device__ __forceinline__ void apply(long long i, const float (&e)[NE][V]) const {
#pragma clang fp contract(off)
    float xv[V], h1[V], h2[V], h3[V], ee[V], p0[V], xp[V];
    ld_f32<V>(in[0], i, xv);
    if (n_hist > 0) ld_f32<V>(in[1], i, h1);
    if (n_hist > 1) ld_f32<V>(in[2], i, h2);
    if (n_hist > 2) ld_f32<V>(in[3], i, h3);
#pragma unroll
    for (int k = 0; k < V; ++k) {
      ee[k] = cfg_combine<EpsT, T>(e[0][k], e[1][k], scale);
      float acc = w[0] * ee[k];                         // integer weights, left to right, then ONE division (plms.py:225-241)
      if (n_hist > 0) acc = acc + w[1] * h1[k];
      if (n_hist > 1) acc = acc + w[2] * h2[k];
      if (n_hist > 2) acc = acc + w[3] * h3[k];
      const float ep = acc / div;
      p0[k] = (xv[k] - c.sqrt_1m_at * ep) / c.sqrt_at;
      xp[k] = c.sqrt_aprev * p0[k] + c.dir_coef * ep;
    }
    if (out[0]) st_f32<V>(out[0], i, ee);
    st_f32<V>(out[2], i, p0);
    st_f32<V>(out[1], i, xp);
  }
};

// DPM-Solver++ multistep (data prediction, solver_type 'dpm_solver'): m0 = (x - sigma_s e) / alpha_s, then
//   order 1: x_t = ratio x - c m0,                     c = alpha_t expm1(-h)
//   order 2: x_t = ratio x - c m0 - c_half D,          c = alpha_t (e^-h - 1), c_half = 0.5 c, D = inv_r0 (m0 - m1)
struct DpmppStep {
  static constexpr int NE = 2, MAX_V = 4;
  const float* in[2];      // x, m1 = the previous step's x0 (null: order 1)
  float* out[2];           // m0 = this step's x0, x_t
  float scale, sigma_s, alpha_s, ratio, c, c_half, inv_r0;
  template <typename EpsT, typename T, int V>
  __device__ __forceinline__ void apply(long long i, const float (&e)[NE][V]) const {
#pragma clang fp contract(off)
    float xv[V], m1[V], m0[V], xt[V];
    ld_f32<V>(in[0], i, xv);
    if (in[1]) ld_f32<V>(in[1], i, m1);
#pragma unroll
    for (int k = 0; k < V; ++k) {
      const float ee = cfg_combine<EpsT, T>(e[0][k], e[1][k], scale);
      m0[k] = (xv[k] - sigma_s * ee) / alpha_s;
      float v = ratio * xv[k] - c * m0[k];
      if (in[1]) {
        const float D = inv_r0 * (m0[k] - m1[k]);
        v = v - c_half * D;
      }
      xt[k] = v;
    }
    st_f32<V>(out[0], i, m0);
    st_f32<V>(out[1], i, xt);
  }
};

// DDIM inversion (DDIMSampler.encode, ddim.py:411-421): x_next = c1 x + c2 e.  c1, c2 are 0-dim float64 tensors in the
// reference, cast to the dtype of the tensor they multiply: with fp16 / bf16 eps, c2 is rounded to that dtype and so is the
// product c2 e; c1 x and the sum are fp32.
struct DdimInvStep {
  static constexpr int NE = 2, MAX_V = 4;
  const float* in[1];      // x
  float* out[1];           // x_next
  float scale, c1, c2;
  template <typename EpsT, typename T, int V>
  __device__ __forceinline__ void apply(long long i, const float (&e)[NE][V]) const {
#pragma clang fp contract(off)
    float xv[V], xn[V];
    ld_f32<V>(in[0], i, xv);
#pragma unroll
    for (int k = 0; k < V; ++k) {
      const float ee = cfg_combine<EpsT, T>(e[0][k], e[1][k], scale);
      const float a = c1 * xv[k];
      float b;
      if constexpr (sizeof(EpsT) == 2) b = (float)(T)((float)(T)c2 * ee);
      else b = c2 * ee;
      xn[k] = a + b;
    }
    st_f32<V>(out[0], i, xn);
  }
};

// Three-way guidance of StructureDDIMSampler.p_sample_ddim_guide (ddim.py:605-607), eps [3 numel] = uncond, cond, cond_simple:
// e = e_u + s ((w e_c + (1 - w) e_s) - e_u), every operation rounded in the eps dtype; then the DDIM update of ddim.py:623-647
// (pred_x0 = (x - sqrt(1 - a_t) e) / sqrt(a_t), x_prev = sqrt(a_prev) pred_x0 + dir_coef e + sigma noise) in fp32.
// The fp32 product of an fp32 scalar and a 16-bit value, as a value: torch rounds it to fp32 first, then to the 16-bit dtype.
// Without the empty asm the compiler fuses multiply + narrowing into one v_fma_mix (a single rounding to 16 bits), which differs
// from the reference in the last 16-bit place whenever the scalar is not exactly representable in a few bits (w = 0.7).
__device__ __forceinline__ float f32_rounded(float v) {
  asm volatile("" : "+v"(v));
  return v;
}

template <typename EpsT, typename T>
__device__ __forceinline__ float cfg3_combine(float eu, float ec, float es, float scale, float w, float w1m) {
#pragma clang fp contract(off)
  if constexpr (sizeof(EpsT) == 2) {
    const T a = (T)f32_rounded(w * ec);
    const T b = (T)f32_rounded(w1m * es);
    const T m = (T)((float)a + (float)b);
    const T d = (T)((float)m - eu);
    const T sd = (T)f32_rounded(scale * (float)d);
    return (float)(T)(eu + (float)sd);
  } else {
    return eu + scale * ((w * ec + w1m * es) - eu);
  }
}

struct DdimCfg3Step {
  static constexpr int NE = 3, MAX_V = 4;
  const float* in[2];      // x, noise (optional)
  float* out[2];           // x_prev, pred_x0
  float scale, w, w1m;
  DdimCoefs c;
  template <typename EpsT, typename T, int V>
  __device__ __forceinline__ void apply(long long i, const float (&e)[NE][V]) const {
#pragma clang fp contract(off)
    float xv[V], nz[V], p0[V], xp[V];
    ld_f32<V>(in[0], i, xv);
    if (in[1]) ld_f32<V>(in[1], i, nz);
#pragma unroll
    for (int k = 0; k < V; ++k) {
      const float ee = cfg3_combine<EpsT, T>(e[0][k], e[1][k], e[2][k], scale, w, w1m);
      p0[k] = (xv[k] - c.sqrt_1m_at * ee) / c.sqrt_at;
      float v = c.sqrt_aprev * p0[k] + c.dir_coef * ee;
      if (in[1]) v = v + c.sigma * nz[k];
      xp[k] = v;
    }
    st_f32<V>(out[1], i, p0);
    st_f32<V>(out[0], i, xp);
  }
};

// Ancestral DDPM posterior step (LatentDiffusion.p_sample after the model call, ddpm.py:950-960, 986-997): one eps slab, no guidance.
//   x_recon = recip x - recipm1 e, clamped to [-1, 1] if clip;  mean = coef1 x_recon + coef2 x;  x_prev = mean + sigma noise
// sigma = nonzero(t) exp(0.5 logvar_clipped[t]) from the host (noise null: sigma == 0, x_prev is exactly the mean).  With a known
// region (in[2..4] set; p_sample_loop, ddpm.py:1093-1095) the same pass blends: x_prev = (sa x0 + s1ma qnoise) m + (1 - m) x_prev.
struct DdpmStep {
  static constexpr int NE = 1, MAX_V = 4;
  const float* in[5];      // x, noise (optional), then all or none of: known x0, its q_sample noise, mask
  float* out[2];           // x_prev, x_recon (optional)
  long long mask_chw, mask_hw;   // mask_hw > 0: mask [B][hw] broadcast over the channels of x [B][chw / hw][hw]; 0: mask shaped like x
  int clip;
  float recip, recipm1, coef1, coef2, sigma, sa, s1ma;
  template <typename EpsT, typename T, int V>
  __device__ __forceinline__ void apply(long long i, const float (&e)[NE][V]) const {
#pragma clang fp contract(off)
    float xv[V], nz[V], k0[V], kn[V], xr[V], xp[V];
    ld_f32<V>(in[0], i, xv);
    if (in[1]) ld_f32<V>(in[1], i, nz);
    if (in[4]) {
      ld_f32<V>(in[2], i, k0);
      ld_f32<V>(in[3], i, kn);
    }
#pragma unroll
    for (int k = 0; k < V; ++k) {
      float r = recip * xv[k] - recipm1 * e[0][k];
      if (clip) r = r < -1.0f ? -1.0f : (r > 1.0f ? 1.0f : r);      // NaN passes through, as in torch.clamp
      xr[k] = r;
      float v = coef1 * r + coef2 * xv[k];
      if (in[1]) v = v + sigma * nz[k];
      if (in[4]) {
        const long long j = i + k;
        const float m = in[4][mask_hw > 0 ? (j / mask_chw) * mask_hw + j % mask_hw : j];
        const float orig = sa * k0[k] + s1ma * kn[k];
        v = orig * m + (1.0f - m) * v;
      }
      xp[k] = v;
    }
    if (out[1]) st_f32<V>(out[1], i, xr);
    st_f32<V>(out[0], i, xp);
  }
};

// DDIMSampler.stochastic_encode (ddim.py:436-449): out = sa[b] x0 + s1ma[b] noise, sample b = blockIdx.y; the coefficient pairs
// are kernel arguments (at most LR_Q_SAMPLE_MAX_B samples per launch).
struct QSampleCoefs { float sa[LR_Q_SAMPLE_MAX_B]; float s1ma[LR_Q_SAMPLE_MAX_B]; };

template <int V>
__global__ void ddim_q_sample_kernel(const float* __restrict__ x0, const float* __restrict__ noise, float* __restrict__ out,
                                     long long per_sample, const QSampleCoefs C) {
#pragma clang fp contract(off)
  const long long base = (long long)blockIdx.y * per_sample;
  const float sa = C.sa[blockIdx.y], s1ma = C.s1ma[blockIdx.y];
  const long long groups = per_sample / V;
  for (long long g = blockIdx.x * (long long)blockDim.x + threadIdx.x; g < groups; g += (long long)gridDim.x * blockDim.x) {
    const long long i = base + g * V;
    float xv[V], nv[V], o[V];
    ld_f32<V>(x0, i, xv);
    ld_f32<V>(noise, i, nv);
#pragma unroll
    for (int k = 0; k < V; ++k) o[k] = sa * xv[k] + s1ma * nv[k];
    st_f32<V>(out, i, o);
  }
}

static inline bool aligned16(const void* p) { return p == nullptr || ((uintptr_t)p & 15) == 0; }

template <typename P, size_t N>
static inline bool aligned16(P* const (&ptrs)[N]) {      // every pointer of a list (null: an absent stream)
  for (P* p : ptrs)
    if (!aligned16(p)) return false;
  return true;
}

static inline int grid_for(long long total, int block, int cap = 4096) {
  long long g = (total + block - 1) / block;
  if (g > cap) g = cap;
  if (g < 1) g = 1;
  return (int)g;
}

extern "C" int lr_abi_version(void) { return 30; }

#ifdef LR_DEV_VARIANTS
// developer build only: name -> value table behind LR_DEV (common.h); set through lr_dev_set by the Python front end
#include <map>
#include <mutex>
#include <string>
static std::map<std::string, int>& lr_dev_table() { static std::map<std::string, int> t; return t; }
static std::mutex lr_dev_mutex;
extern "C" int lr_dev_set(const char* name, int value) {
  if (!name) return LR_E_ARG;
  std::lock_guard<std::mutex> g(lr_dev_mutex);
  lr_dev_table()[name] = value;
  return 0;
}
extern "C" int lr_dev_unset(const char* name) {
  if (!name) return LR_E_ARG;
  std::lock_guard<std::mutex> g(lr_dev_mutex);
  lr_dev_table().erase(name);
  return 0;
}
int lr_dev_get(const char* name, int dflt) {
  std::lock_guard<std::mutex> g(lr_dev_mutex);
  const auto it = lr_dev_table().find(name);
  return it == lr_dev_table().end() ? dflt : it->second;
}
#endif

template <typename T>
static int lr_nchw_f32_to_nhwc_t(const float* x1, int C1, const float* x2, int C2, lr_half* y, int Cpad, int N,
                                       int H, int W, lr_stream_t s) {
  if (!x1 || !y || N <= 0 || H <= 0 || W <= 0 || C1 <= 0) return LR_E_ARG;
  if (!x2) C2 = 0;
  if (Cpad % 8 || Cpad < C1 + C2) return LR_E_ALIGN;
  const long long total = (long long)N * (Cpad / 8) * H * W;
  hipLaunchKernelGGL(nchw_to_nhwc_kernel<T>, dim3(grid_for(total, 256)), dim3(256), 0, (hipStream_t)s, x1, C1, x2, C2,
                     (T*)y, Cpad, H * W, total);
  return lr_launch_status();
}

template <typename T>
static int lr_nhwc_f16_to_nchw_t(const lr_half* y, int Cstride, int C, void* out, int out_is_f32, int N, int H, int W,
                                   lr_stream_t s) {
  if (!y || !out || N <= 0 || C <= 0 || C > Cstride) return LR_E_ARG;
  const long long total = (long long)N * C * H * W;
  if (out_is_f32)
    hipLaunchKernelGGL((nhwc_to_nchw_kernel<float, T>), dim3(grid_for(total, 256)), dim3(256), 0, (hipStream_t)s,
                       (const T*)y, Cstride, C, (float*)out, H * W, total);
  else
    hipLaunchKernelGGL((nhwc_to_nchw_kernel<T, T>), dim3(grid_for(total, 256)), dim3(256), 0, (hipStream_t)s,
                       (const T*)y, Cstride, C, (T*)out, H * W, total);
  return lr_launch_status();
}

template <typename TT, typename T>
static int lr_timestep_embedding_t(const TT* t, int N, int dim, lr_half* out, lr_stream_t s) {
  if (!t || !out || N <= 0 || dim < 2) return LR_E_ARG;
  const int total = N * (dim / 2);
  hipLaunchKernelGGL((timestep_embedding_kernel<TT, T>), dim3((total + 255) / 256), dim3(256), 0, (hipStream_t)s, t, N, dim,
                     (T*)out);
  return lr_launch_status();
}

template <typename T>
static int lr_linear_small_m_t(const lr_half* a, int lda, const lr_half* w, const float* bias, lr_half* out, int ldo,
                                 int M, int N, int K, int act_in, int act_out, lr_stream_t s) {
  if (!a || !w || !out || M <= 0 || N <= 0 || K <= 0) return LR_E_ARG;
  if (M > 16) return LR_E_UNSUPPORTED;
  if (K % 8) return LR_E_ALIGN;
  // columns per wave: every block stages the M activation rows once, so wide layers take more columns per block (about two blocks per
  // CU); a column's arithmetic does not depend on it (one lane-strided K loop + one wave sum per column): same bits for every value
  const int waves = 4;
  int cpw = (N + waves * 512 - 1) / (waves * 512);
  if (cpw < 4) cpw = 4;
  if (cpw > 32) cpw = 32;
  dim3 grid((N + cpw * waves - 1) / (cpw * waves)), block(64 * waves);
  hipStream_t st = (hipStream_t)s;
  if (M <= 4)
    hipLaunchKernelGGL((linear_small_m_kernel<4, T>), grid, block, 4 * K * sizeof(T), st, (const T*)a, lda,
                       (const T*)w, bias, (T*)out, ldo, M, N, K, act_in, act_out, cpw);
  else if (M <= 8)
    hipLaunchKernelGGL((linear_small_m_kernel<8, T>), grid, block, 8 * K * sizeof(T), st, (const T*)a, lda,
                       (const T*)w, bias, (T*)out, ldo, M, N, K, act_in, act_out, cpw);
  else
    hipLaunchKernelGGL((linear_small_m_kernel<16, T>), grid, block, 16 * K * sizeof(T), st, (const T*)a, lda,
                       (const T*)w, bias, (T*)out, ldo, M, N, K, act_in, act_out, cpw);
  return lr_launch_status();
}

template <typename T>
static int lr_mv_gather_t(const lr_half* x, lr_half* seq, int b, int v, int s, int C, lr_stream_t st) {
  if (!x || !seq || b <= 0 || v <= 0 || s <= 0) return LR_E_ARG;
  if (C % 8) return LR_E_ALIGN;
  const long long total = (long long)b * (v + 1) * s * s * (C / 8);
  hipLaunchKernelGGL((mv_gather_kernel<false, T>), dim3(grid_for(total, 256)), dim3(256), 0, (hipStream_t)st, (const uint4*)x,
                     (uint4*)seq, b, v, s, C / 8, total);
  return lr_launch_status();
}

template <typename T>
static int lr_mv_scatter_t(const lr_half* seq, lr_half* x, int b, int v, int s, int C, lr_stream_t st) {
  if (!x || !seq || b <= 0 || v <= 0 || s <= 0) return LR_E_ARG;
  if (C % 8) return LR_E_ALIGN;
  const long long total = (long long)b * v * s * 2 * s * (C / 8);
  hipLaunchKernelGGL(mv_scatter_kernel<false>, dim3(grid_for(total, 256)), dim3(256), 0, (hipStream_t)st, (const uint4*)seq,
                     (uint4*)x, b, v, s, C / 8, total);
  return lr_launch_status();
}

// The one launch of the sampler steps: V = 4 where the step allows it, numel % 4 == 0, every fp32 stream is 16-byte aligned and
// eps 16-byte (fp32) / 8-byte (16-bit) aligned, else V = 1; EpsT = float or the 16-bit type T of the entry point.
template <typename T, typename Step>
static int launch_sampler_step(const Step& st, const void* eps, int eps_is_f32, int64_t numel, lr_stream_t s) {
  const bool vec = Step::MAX_V == 4 && numel % 4 == 0 && aligned16(st.in) && aligned16(st.out) &&
                   ((uintptr_t)eps & (eps_is_f32 ? 15 : 7)) == 0;
  auto launch = [&](auto v, auto* e) {      // v: std::integral_constant<int, V>, e: const EpsT*
    constexpr int V = decltype(v)::value;
    using EpsT = std::remove_cv_t<std::remove_pointer_t<decltype(e)>>;
    hipLaunchKernelGGL((sampler_step_kernel<V, EpsT, T, Step>), dim3(grid_for(numel / V, 256)), dim3(256), 0, (hipStream_t)s,
                       (long long)numel, e, st);
  };
  auto with_eps = [&](auto* e) {
    if constexpr (Step::MAX_V == 4) {
      if (vec) return launch(std::integral_constant<int, 4>{}, e);
    }
    launch(std::integral_constant<int, 1>{}, e);
  };
  if (eps_is_f32) with_eps((const float*)eps);
  else with_eps((const T*)eps);
  return lr_launch_status();
}

template <typename T>
static int lr_ddim_cfg_step_t(const float* x, const void* eps, int eps_is_f32, const float* noise, float* x_prev,
                                float* pred_x0, int64_t numel, float cfg_scale, float a_t, float a_prev, float sigma_t,
                                float sqrt_one_minus_at, lr_stream_t s) {
  if (!x || !eps || !x_prev || !pred_x0 || numel <= 0) return LR_E_ARG;
  const DdimStep st{{x, noise}, {x_prev, pred_x0}, cfg_scale, ddim_coefs(a_t, a_prev, sigma_t, sqrt_one_minus_at)};
  return launch_sampler_step<T>(st, eps, eps_is_f32, numel, s);
}

template <typename T>
static int lr_plms_cfg_step_t(const float* x, const void* eps, int eps_is_f32, const float* const* hist, int n_hist,
                              const float* weights, float divisor, float* e_out, float* x_prev, float* pred_x0, int64_t numel,
                              float cfg_scale, float a_t, float a_prev, float sqrt_one_minus_at, lr_stream_t s) {
  if (!x || !eps || !x_prev || !pred_x0 || !weights || numel <= 0 || n_hist < 0 || n_hist > 3 || divisor == 0.f) return LR_E_ARG;
  if (n_hist > 0 && !hist) return LR_E_ARG;
  PlmsStep st{{x, nullptr, nullptr, nullptr}, {e_out, x_prev, pred_x0}, n_hist, cfg_scale, {weights[0], 0.f, 0.f, 0.f}, divisor,
              ddim_coefs(a_t, a_prev, 0.0f, sqrt_one_minus_at)};
  for (int k = 0; k < n_hist; ++k) {
    if (!hist[k]) return LR_E_ARG;
    st.in[k + 1] = hist[k];
    st.w[k + 1] = weights[k + 1];
  }
  return launch_sampler_step<T>(st, eps, eps_is_f32, numel, s);
}

template <typename T>
static int lr_dpmpp_cfg_step_t(const float* x, const void* eps, int eps_is_f32, const float* x0_prev, float* x0_out, float* x_next,
                               int64_t numel, float cfg_scale, float sigma_s, float alpha_s, float ratio, float c, float c_half,
                               float inv_r0, lr_stream_t s) {
  if (!x || !eps || !x0_out || !x_next || numel <= 0 || alpha_s == 0.f) return LR_E_ARG;
  const DpmppStep st{{x, x0_prev}, {x0_out, x_next}, cfg_scale, sigma_s, alpha_s, ratio, c, c_half, inv_r0};
  return launch_sampler_step<T>(st, eps, eps_is_f32, numel, s);
}

template <typename T>
static int lr_ddim_inv_cfg_step_t(const float* x, const void* eps, int eps_is_f32, float* x_next, int64_t numel, float cfg_scale,
                                  float c1, float c2, lr_stream_t s) {
  if (!x || !eps || !x_next || numel <= 0) return LR_E_ARG;
  const DdimInvStep st{{x}, {x_next}, cfg_scale, c1, c2};
  return launch_sampler_step<T>(st, eps, eps_is_f32, numel, s);
}

template <typename T>
static int lr_ddim_cfg3_step_t(const float* x, const void* eps, int eps_is_f32, const float* noise, float* x_prev, float* pred_x0,
                               int64_t numel, float cfg_scale, float cond_weight, float one_minus_cond_weight, float a_t,
                               float a_prev, float sigma_t, float sqrt_one_minus_at, lr_stream_t s) {
  if (!x || !eps || !x_prev || !pred_x0 || numel <= 0) return LR_E_ARG;
  const DdimCfg3Step st{{x, noise}, {x_prev, pred_x0}, cfg_scale, cond_weight, one_minus_cond_weight,
                        ddim_coefs(a_t, a_prev, sigma_t, sqrt_one_minus_at)};
  return launch_sampler_step<T>(st, eps, eps_is_f32, numel, s);
}

template <typename T>
static int lr_ddpm_step_t(const float* x, const void* eps, int eps_is_f32, const float* noise, const float* known_x0,
                          const float* known_noise, const float* mask, int64_t mask_chw, int64_t mask_hw, int clip_denoised,
                          float* x_prev, float* x0_out, int64_t numel, float sqrt_recip_ac, float sqrt_recipm1_ac, float coef1,
                          float coef2, float sigma, float sqrt_ac, float sqrt_one_minus_ac, lr_stream_t s) {
  if (!x || !eps || !x_prev || numel <= 0 || (!noise && sigma != 0.f)) return LR_E_ARG;
  if (mask) {      // known-region blend: all three streams, and a mask that tiles x exactly
    if (!known_x0 || !known_noise || mask_hw < 0) return LR_E_ARG;
    if (mask_hw > 0 && (mask_chw <= 0 || mask_chw % mask_hw || numel % mask_chw)) return LR_E_ARG;
  } else if (known_x0 || known_noise) {
    return LR_E_ARG;
  }
  const DdpmStep st{{x, sigma != 0.f ? noise : nullptr, known_x0, known_noise, mask}, {x_prev, x0_out}, (long long)mask_chw,
                    (long long)mask_hw, clip_denoised, sqrt_recip_ac, sqrt_recipm1_ac, coef1, coef2, sigma, sqrt_ac,
                    sqrt_one_minus_ac};
  return launch_sampler_step<T>(st, eps, eps_is_f32, numel, s);
}

extern "C" int lr_ddim_q_sample(const float* x0, const float* noise, float* out, int B, int64_t per_sample, const float* sa,
                                const float* s1ma, lr_stream_t s) {
  if (!x0 || !noise || !out || !sa || !s1ma || B <= 0 || B > LR_Q_SAMPLE_MAX_B || per_sample <= 0) return LR_E_ARG;
  QSampleCoefs C{};
  for (int b = 0; b < B; ++b) {
    C.sa[b] = sa[b];
    C.s1ma[b] = s1ma[b];
  }
  const bool vec = per_sample % 4 == 0 && aligned16(x0) && aligned16(noise) && aligned16(out);
  const int V = vec ? 4 : 1;
  dim3 grid(grid_for(per_sample / V, 256, (4096 + B - 1) / B), B), block(256);
  if (vec) hipLaunchKernelGGL(ddim_q_sample_kernel<4>, grid, block, 0, (hipStream_t)s, x0, noise, out, (long long)per_sample, C);
  else hipLaunchKernelGGL(ddim_q_sample_kernel<1>, grid, block, 0, (hipStream_t)s, x0, noise, out, (long long)per_sample, C);
  return lr_launch_status();
}

// =====================================================================================================================
// Backward helpers (training with frozen weights)
// =====================================================================================================================
// GEGLU backward.  pre [M][2H]: the projection (+bias) in the packed layout of lr_gemm_conv_f16 (16-column groups
// [u16 | g16 | u16 | g16 ...]); dy [M][H];  dpre (same layout as pre): du = dy * gelu(g), dg = dy * u * gelu'(g),
// gelu'(g) = Phi(g) + g * phi(g)  (erf form, attention.py:56-58).  One thread per 8 output columns.
template <typename T>
__global__ void geglu_bwd_kernel(const T* __restrict__ pre, const T* __restrict__ dy, T* __restrict__ dpre, long long total,
                                 int H) {
  const int cpr = H >> 3;      // 8-column chunks per row of dy
  for (long long id = blockIdx.x * (long long)blockDim.x + threadIdx.x; id < total; id += (long long)gridDim.x * blockDim.x) {
    const long long m = id / cpr;
    const int c = (int)(id - m * cpr) * 8;            // first output column of this chunk
    const int pc = (c >> 4) * 32 + (c & 15);          // packed column of u; g sits 16 columns later
    float u[8], g[8], d[8], du[8], dg[8];
    lr_unpack8<T>(*reinterpret_cast<const uint4*>(pre + m * 2 * H + pc), u);
    lr_unpack8<T>(*reinterpret_cast<const uint4*>(pre + m * 2 * H + pc + 16), g);
    lr_unpack8<T>(*reinterpret_cast<const uint4*>(dy + m * H + c), d);
#pragma unroll
    for (int i = 0; i < 8; i += 2) {      // two values per instruction stream (packed fp32), Phi from the forward's own formula
      const f32x2_t gg = {g[i], g[i + 1]}, dd = {d[i], d[i + 1]}, uu = {u[i], u[i + 1]};
      const f32x2_t ph = lr_phi_mhalf2(gg);                                                    // Phi(g) - 0.5
      const f32x2_t q = gg * gg * -0.72134752044448170368f;                                    // -g^2 / 2 in log2 units
      const f32x2_t pdf = (f32x2_t){__builtin_amdgcn_exp2f(q[0]), __builtin_amdgcn_exp2f(q[1])} * 0.3989422804014327f;
      const f32x2_t gelu = __builtin_elementwise_fma(gg, ph, gg * 0.5f);                       // == lr_gelu_erf2(g)
      const f32x2_t dgel = __builtin_elementwise_fma(gg, pdf, ph + 0.5f);                      // Phi + g phi
      const f32x2_t a = dd * gelu, b = dd * uu * dgel;
      du[i] = a[0]; du[i + 1] = a[1];
      dg[i] = b[0]; dg[i + 1] = b[1];
    }
    *reinterpret_cast<uint4*>(dpre + m * 2 * H + pc) = lr_pack8<T>(du);
    *reinterpret_cast<uint4*>(dpre + m * 2 * H + pc + 16) = lr_pack8<T>(dg);
  }
}

// GEGLU forward from the stored projection (training keeps `pre` for the backward instead of recomputing the GEMM):
// out[m][c] = u * gelu_erf(g), same packed layout of pre as above.
template <typename T>
__global__ void geglu_fwd_kernel(const T* __restrict__ pre, T* __restrict__ out, long long total, int H) {
  const int cpr = H >> 3;
  for (long long id = blockIdx.x * (long long)blockDim.x + threadIdx.x; id < total; id += (long long)gridDim.x * blockDim.x) {
    const long long m = id / cpr;
    const int c = (int)(id - m * cpr) * 8;
    const int pc = (c >> 4) * 32 + (c & 15);
    float u[8], g[8], o[8];
    lr_unpack8<T>(*reinterpret_cast<const uint4*>(pre + m * 2 * H + pc), u);
    lr_unpack8<T>(*reinterpret_cast<const uint4*>(pre + m * 2 * H + pc + 16), g);
#pragma unroll
    for (int i = 0; i < 8; i += 2) {      // (packed pairs: same formula, same bits as the scalar form)
      const f32x2_t ge = lr_gelu_erf2((f32x2_t){g[i], g[i + 1]});
      o[i] = u[i] * ge[0];
      o[i + 1] = u[i + 1] * ge[1];
    }
    *reinterpret_cast<uint4*>(out + m * H + c) = lr_pack8<T>(o);
  }
}

template <typename T>
static int lr_geglu_fwd_t(const lr_half* pre, lr_half* out, int M, int H, lr_stream_t s) {
  if (!pre || !out || M <= 0 || H <= 0) return LR_E_ARG;
  if (H % 16) return LR_E_ALIGN;
  const long long total = (long long)M * (H / 8);
  long long blocks = (total + 255) / 256;
  if (blocks > 65536) blocks = 65536;
  hipLaunchKernelGGL(geglu_fwd_kernel<T>, dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)s, (const T*)pre, (T*)out, total, H);
  return lr_launch_status();
}

template <typename T>
static int lr_geglu_bwd_t(const lr_half* pre, const lr_half* dy, lr_half* dpre, int M, int H, lr_stream_t s) {
  if (!pre || !dy || !dpre || M <= 0 || H <= 0) return LR_E_ARG;
  if (H % 16) return LR_E_ALIGN;
  const long long total = (long long)M * (H / 8);
  long long blocks = (total + 255) / 256;
  if (blocks > 65536) blocks = 65536;
  hipLaunchKernelGGL(geglu_bwd_kernel<T>, dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)s, (const T*)pre, (const T*)dy,
                     (T*)dpre, total, H);
  return lr_launch_status();
}

// Plain erf-GELU (the text tower's MLP, nn.GELU) for training: the GEMM runs without its GELU epilogue and keeps `pre` for the
// backward.  pre / y / dy / dpre are n contiguous elements, n % 8 == 0; one thread per 8 of them.
//   fwd: y = gelu(pre)                         (lr_gelu_erf2: the fused epilogue's formula, same bits)
//   bwd: dpre = dy * (Phi(pre) + pre phi(pre))  (Phi from the forward's own formula, as in geglu_bwd_kernel)
template <typename T, bool BWD>
__global__ void gelu_kernel(const T* __restrict__ pre, const T* __restrict__ dy, T* __restrict__ out, long long total) {
  for (long long id = blockIdx.x * (long long)blockDim.x + threadIdx.x; id < total; id += (long long)gridDim.x * blockDim.x) {
    float x[8], d[8], o[8];
    lr_unpack8<T>(*reinterpret_cast<const uint4*>(pre + id * 8), x);
    if constexpr (BWD) lr_unpack8<T>(*reinterpret_cast<const uint4*>(dy + id * 8), d);
#pragma unroll
    for (int i = 0; i < 8; i += 2) {
      const f32x2_t xx = {x[i], x[i + 1]};
      f32x2_t r;
      if constexpr (BWD) {
        const f32x2_t ph = lr_phi_mhalf2(xx);                                                   // Phi(x) - 0.5
        const f32x2_t q = xx * xx * -0.72134752044448170368f;                                   // -x^2 / 2 in log2 units
        const f32x2_t pdf = (f32x2_t){__builtin_amdgcn_exp2f(q[0]), __builtin_amdgcn_exp2f(q[1])} * 0.3989422804014327f;
        r = (f32x2_t){d[i], d[i + 1]} * __builtin_elementwise_fma(xx, pdf, ph + 0.5f);        // dy (Phi + x phi)
      } else {
        r = lr_gelu_erf2(xx);
      }
      o[i] = r[0];
      o[i + 1] = r[1];
    }
    *reinterpret_cast<uint4*>(out + id * 8) = lr_pack8<T>(o);
  }
}

template <typename T, bool BWD>
static int lr_gelu_t(const lr_half* pre, const lr_half* dy, lr_half* out, long long n, lr_stream_t s) {
  if (!pre || !out || (BWD && !dy) || n <= 0) return LR_E_ARG;
  if (n % 8 || (((uintptr_t)pre | (uintptr_t)dy | (uintptr_t)out) & 15)) return LR_E_ALIGN;
  const long long total = n / 8;
  long long blocks = (total + 255) / 256;
  if (blocks > 65536) blocks = 65536;
  hipLaunchKernelGGL((gelu_kernel<T, BWD>), dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)s, (const T*)pre, (const T*)dy, (T*)out,
                     total);
  return lr_launch_status();
}

// Backward of the nearest-2x upsample in front of a conv (Upsample.forward, openaimodel.py:115): the four fine pixels
// of a coarse pixel add up.  x [N][2H][2W][C] -> y [N][H][W][C].
template <typename T>
__global__ void sumpool2x2_kernel(const T* __restrict__ x, T* __restrict__ y, long long total, int H, int W, int C) {
  const int cpr = C >> 3;
  for (long long id = blockIdx.x * (long long)blockDim.x + threadIdx.x; id < total; id += (long long)gridDim.x * blockDim.x) {
    const int c = (int)(id % cpr) * 8;
    long long pix = id / cpr;
    const int xw = (int)(pix % W);
    pix /= W;
    const int yh = (int)(pix % H);
    const long long n = pix / H;
    const T* src = x + ((n * 2 * H + 2 * yh) * 2 * W + 2 * xw) * (long long)C + c;
    float a[8], acc[8];
    lr_unpack8<T>(*reinterpret_cast<const uint4*>(src), acc);
    lr_unpack8<T>(*reinterpret_cast<const uint4*>(src + C), a);
#pragma unroll
    for (int i = 0; i < 8; ++i) acc[i] += a[i];
    lr_unpack8<T>(*reinterpret_cast<const uint4*>(src + 2LL * W * C), a);
#pragma unroll
    for (int i = 0; i < 8; ++i) acc[i] += a[i];
    lr_unpack8<T>(*reinterpret_cast<const uint4*>(src + 2LL * W * C + C), a);
#pragma unroll
    for (int i = 0; i < 8; ++i) acc[i] += a[i];
    *reinterpret_cast<uint4*>(y + ((n * H + yh) * W + xw) * (long long)C + c) = lr_pack8<T>(acc);
  }
}

template <typename T>
static int lr_sumpool2x2_t(const lr_half* x, lr_half* y, int N, int H, int W, int C, lr_stream_t s) {
  if (!x || !y || N <= 0 || H <= 0 || W <= 0) return LR_E_ARG;
  if (C % 8) return LR_E_ALIGN;
  const long long total = (long long)N * H * W * (C / 8);
  long long blocks = (total + 255) / 256;
  if (blocks > 65536) blocks = 65536;
  hipLaunchKernelGGL(sumpool2x2_kernel<T>, dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)s, (const T*)x, (T*)y, total, H, W, C);
  return lr_launch_status();
}

// Backward of the multi-view re-arrangement (same shapes as lr_mv_gather / lr_mv_scatter, roles of x and seq swapped)
template <typename T>
static int lr_mv_gather_bwd_t(const lr_half* dseq, lr_half* dx, int b, int v, int s, int C, lr_stream_t st) {
  if (!dx || !dseq || b <= 0 || v <= 0 || s <= 0) return LR_E_ARG;
  if (C % 8) return LR_E_ALIGN;
  const long long total = (long long)b * v * s * 2 * s * (C / 8);
  hipLaunchKernelGGL(mv_scatter_kernel<true>, dim3(grid_for(total, 256)), dim3(256), 0, (hipStream_t)st, (const uint4*)dseq,
                     (uint4*)dx, b, v, s, C / 8, total);
  return lr_launch_status();
}

template <typename T>
static int lr_mv_scatter_bwd_t(const lr_half* dx, lr_half* dseq, int b, int v, int s, int C, lr_stream_t st) {
  if (!dx || !dseq || b <= 0 || v <= 0 || s <= 0) return LR_E_ARG;
  if (C % 8) return LR_E_ALIGN;
  const long long total = (long long)b * (v + 1) * s * s * (C / 8);
  hipLaunchKernelGGL((mv_gather_kernel<true, T>), dim3(grid_for(total, 256)), dim3(256), 0, (hipStream_t)st, (const uint4*)dx,
                     (uint4*)dseq, b, v, s, C / 8, total);
  return lr_launch_status();
}

// ---- C ABI: every entry point in its fp16 and bf16 form -------------------------------------------------------------
LR_ABI_PAIR(lr_nchw_f32_to_nhwc_f16, lr_nchw_f32_to_nhwc_bf16, (const float* x1, int C1, const float* x2, int C2, lr_half* y, int Cpad, int N, int H, int W, lr_stream_t s), lr_nchw_f32_to_nhwc_t<T>(x1, C1, x2, C2, y, Cpad, N, H, W, s))
LR_ABI_PAIR(lr_nhwc_f16_to_nchw, lr_nhwc_f16_to_nchw_bf16, (const lr_half* y, int Cstride, int C, void* out, int out_is_f32, int N, int H, int W, lr_stream_t s), lr_nhwc_f16_to_nchw_t<T>(y, Cstride, C, out, out_is_f32, N, H, W, s))
LR_ABI_PAIR(lr_timestep_embedding, lr_timestep_embedding_bf16, (const int64_t* t, int N, int dim, lr_half* out, lr_stream_t s), lr_timestep_embedding_t<int64_t, T>(t, N, dim, out, s))
LR_ABI_PAIR(lr_timestep_embedding_f32, lr_timestep_embedding_f32_bf16, (const float* t, int N, int dim, lr_half* out, lr_stream_t s), lr_timestep_embedding_t<float, T>(t, N, dim, out, s))
LR_ABI_PAIR(lr_linear_small_m, lr_linear_small_m_bf16, (const lr_half* a, int lda, const lr_half* w, const float* bias, lr_half* out, int ldo, int M, int N, int K, int act_in, int act_out, lr_stream_t s), lr_linear_small_m_t<T>(a, lda, w, bias, out, ldo, M, N, K, act_in, act_out, s))
LR_ABI_PAIR(lr_mv_gather, lr_mv_gather_bf16, (const lr_half* x, lr_half* seq, int b, int v, int s, int C, lr_stream_t st), lr_mv_gather_t<T>(x, seq, b, v, s, C, st))
LR_ABI_PAIR(lr_mv_scatter, lr_mv_scatter_bf16, (const lr_half* seq, lr_half* x, int b, int v, int s, int C, lr_stream_t st), lr_mv_scatter_t<T>(seq, x, b, v, s, C, st))
LR_ABI_PAIR(lr_ddim_cfg_step, lr_ddim_cfg_step_bf16, (const float* x, const void* eps, int eps_is_f32, const float* noise, float* x_prev, float* pred_x0, int64_t numel, float cfg_scale, float a_t, float a_prev, float sigma_t, float sqrt_one_minus_at, lr_stream_t s), lr_ddim_cfg_step_t<T>(x, eps, eps_is_f32, noise, x_prev, pred_x0, numel, cfg_scale, a_t, a_prev, sigma_t, sqrt_one_minus_at, s))
LR_ABI_PAIR(lr_plms_cfg_step, lr_plms_cfg_step_bf16, (const float* x, const void* eps, int eps_is_f32, const float* const* hist, int n_hist, const float* weights, float divisor, float* e_out, float* x_prev, float* pred_x0, int64_t numel, float cfg_scale, float a_t, float a_prev, float sqrt_one_minus_at, lr_stream_t s), lr_plms_cfg_step_t<T>(x, eps, eps_is_f32, hist, n_hist, weights, divisor, e_out, x_prev, pred_x0, numel, cfg_scale, a_t, a_prev, sqrt_one_minus_at, s))
LR_ABI_PAIR(lr_dpmpp_cfg_step, lr_dpmpp_cfg_step_bf16, (const float* x, const void* eps, int eps_is_f32, const float* x0_prev, float* x0_out, float* x_next, int64_t numel, float cfg_scale, float sigma_s, float alpha_s, float ratio, float c, float c_half, float inv_r0, lr_stream_t s), lr_dpmpp_cfg_step_t<T>(x, eps, eps_is_f32, x0_prev, x0_out, x_next, numel, cfg_scale, sigma_s, alpha_s, ratio, c, c_half, inv_r0, s))
LR_ABI_PAIR(lr_ddim_inv_cfg_step, lr_ddim_inv_cfg_step_bf16, (const float* x, const void* eps, int eps_is_f32, float* x_next, int64_t numel, float cfg_scale, float c1, float c2, lr_stream_t s), lr_ddim_inv_cfg_step_t<T>(x, eps, eps_is_f32, x_next, numel, cfg_scale, c1, c2, s))
LR_ABI_PAIR(lr_ddim_cfg3_step, lr_ddim_cfg3_step_bf16, (const float* x, const void* eps, int eps_is_f32, const float* noise, float* x_prev, float* pred_x0, int64_t numel, float cfg_scale, float cond_weight, float one_minus_cond_weight, float a_t, float a_prev, float sigma_t, float sqrt_one_minus_at, lr_stream_t s), lr_ddim_cfg3_step_t<T>(x, eps, eps_is_f32, noise, x_prev, pred_x0, numel, cfg_scale, cond_weight, one_minus_cond_weight, a_t, a_prev, sigma_t, sqrt_one_minus_at, s))
LR_ABI_PAIR(lr_ddpm_step, lr_ddpm_step_bf16, (const float* x, const void* eps, int eps_is_f32, const float* noise, const float* known_x0, const float* known_noise, const float* mask, int64_t mask_chw, int64_t mask_hw, int clip_denoised, float* x_prev, float* x0_out, int64_t numel, float sqrt_recip_ac, float sqrt_recipm1_ac, float coef1, float coef2, float sigma, float sqrt_ac, float sqrt_one_minus_ac, lr_stream_t s), lr_ddpm_step_t<T>(x, eps, eps_is_f32, noise, known_x0, known_noise, mask, mask_chw, mask_hw, clip_denoised, x_prev, x0_out, numel, sqrt_recip_ac, sqrt_recipm1_ac, coef1, coef2, sigma, sqrt_ac, sqrt_one_minus_ac, s))
LR_ABI_PAIR(lr_geglu_fwd, lr_geglu_fwd_bf16, (const lr_half* pre, lr_half* out, int M, int H, lr_stream_t s), lr_geglu_fwd_t<T>(pre, out, M, H, s))
LR_ABI_PAIR(lr_geglu_bwd, lr_geglu_bwd_bf16, (const lr_half* pre, const lr_half* dy, lr_half* dpre, int M, int H, lr_stream_t s), lr_geglu_bwd_t<T>(pre, dy, dpre, M, H, s))
LR_ABI_PAIR(lr_gelu_fwd_f16, lr_gelu_fwd_bf16, (const lr_half* pre, lr_half* y, int64_t n, lr_stream_t s), lr_gelu_t<T, false>(pre, nullptr, y, n, s))
LR_ABI_PAIR(lr_gelu_bwd_f16, lr_gelu_bwd_bf16, (const lr_half* pre, const lr_half* dy, lr_half* dpre, int64_t n, lr_stream_t s), lr_gelu_t<T, true>(pre, dy, dpre, n, s))
LR_ABI_PAIR(lr_sumpool2x2, lr_sumpool2x2_bf16, (const lr_half* x, lr_half* y, int N, int H, int W, int C, lr_stream_t s), lr_sumpool2x2_t<T>(x, y, N, H, W, C, s))
LR_ABI_PAIR(lr_mv_gather_bwd, lr_mv_gather_bwd_bf16, (const lr_half* dseq, lr_half* dx, int b, int v, int s, int C, lr_stream_t st), lr_mv_gather_bwd_t<T>(dseq, dx, b, v, s, C, st))
LR_ABI_PAIR(lr_mv_scatter_bwd, lr_mv_scatter_bwd_bf16, (const lr_half* dx, lr_half* dseq, int b, int v, int s, int C, lr_stream_t st), lr_mv_scatter_bwd_t<T>(dx, dseq, b, v, s, C, st))
extern "C" int lr_row_copy(const lr_row_copy_job* jobs, int n_jobs, lr_stream_t st) {
  if (!jobs || n_jobs < 1 || n_jobs > 4) return LR_E_ARG;
  RowCopyJobs J;
  long long mx = 0;
  for (int i = 0; i < n_jobs; ++i) {
    const lr_row_copy_job& jb = jobs[i];
    if (!jb.src || !jb.dst || jb.n_rows < 0 || jb.row_bytes <= 0) return LR_E_ARG;
    if ((jb.row_bytes | jb.src_pitch | jb.dst_pitch | jb.src_off | jb.dst_off | (int64_t)(uintptr_t)jb.src | (int64_t)(uintptr_t)jb.dst) & 7) return LR_E_ALIGN;
    J.j[i] = jb;
    const long long t_ = (long long)jb.n_rows * (jb.row_bytes >> 3);
    if (t_ > mx) mx = t_;
  }
  if (mx == 0) return 0;
  hipLaunchKernelGGL(row_copy_kernel, dim3(grid_for(mx, 256), n_jobs), dim3(256), 0, (hipStream_t)st, J);
  return lr_launch_status();
}

