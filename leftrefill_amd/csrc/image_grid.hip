// The training logger's tail on the device (include/leftrefill_hip.h: lr_image_grid, lr_token_drift).
//
// lr_image_grid: ONE launch writes the finished uint8 HWC canvas of up to LR_GRID_MAX_SOURCES image batches -- the per-key
// `make_grid(nrow=1, padding=2)` columns, clamp, (x + 1) / 2, * 255, truncation -- padding pixels included, straight from the sources'
// own memory through their element strides (an NHWC view and an NCHW tensor meet in one launch; nothing is copied first and nothing is
// memset).  The canvas is treated as one flat byte array: up to three bytes in front of the first 4-byte-aligned address and behind the
// last are byte stores, everything between is one dword store per thread, so a dword may span two pixels, two sources or two rows (a
// row is 3 Wc bytes, in general no multiple of 4).  A thread walks its four bytes with carries (channel -> pixel -> row); each byte
// finds its source by its canvas column in the by-value table.  Adjacent lanes read adjacent elements along w (stride 1 for NCHW, 3 with
// the channels between for an NHWC view): the reads coalesce on the fastest-varying stride of either layout.
// Every output byte is written exactly once by plain stores: capturable, bitwise reproducible.
//
// lr_token_drift: one wave per token; lane l adds its elements in index order, the 64 lane sums meet in a butterfly (a fixed order),
// and the same pass refreshes the snapshot.
//
// The 8-bit conversion must round exactly like the reference's separate fp32 operations: no fused multiply-add here.
#include "common.h"

#pragma clang fp contract(off)

#define IG_THREADS 256
#define IG_PAD 2      // make_grid's padding

struct GridSources { lr_grid_source s[LR_GRID_MAX_SOURCES]; };

__device__ __forceinline__ float ig_load(const lr_grid_source& s, long long at) {
  if (s.kind == LR_EVAL_PRED_F32) return reinterpret_cast<const float*>(s.ptr)[at];
  if (s.kind == LR_EVAL_PRED_F16) return (float)reinterpret_cast<const f16*>(s.ptr)[at];
  return (float)reinterpret_cast<const bf16*>(s.ptr)[at];
}

// the byte of canvas row `row`, canvas column `px`, channel `ch`
__device__ __forceinline__ unsigned ig_byte(const GridSources& S, int n_sources, int N, int H, int clamp, int rescale, int row, int px,
                                            int ch) {
  float v = 0.f;      // pad_value
  const int pad = N == 1 ? 0 : IG_PAD;
  const int rr = row - pad, cell = H + pad;
  const int k = rr >= 0 ? rr / cell : -1;
  const int y = rr - k * cell;
  if (k >= 0 && k < N && y < H) {
    for (int i = 0; i < n_sources; ++i) {
      const lr_grid_source& s = S.s[i];
      const int x = px - s.col - pad;
      if (x >= 0 && x < s.W) {
        v = ig_load(s, (long long)k * s.stride_n + (long long)(s.C == 1 ? 0 : ch) * s.stride_c + (long long)y * s.stride_h +
                           (long long)x * s.stride_w);
        if (clamp) v = fminf(fmaxf(v, -1.f), 1.f);
        break;
      }
    }
  }
  if (rescale) v = (v + 1.f) / 2.f;
  v = v * 255.f;
  return (unsigned)min(max((int)v, 0), 255);      // truncation; what lies outside 0 .. 255 (clamp off) saturates
}

__global__ __launch_bounds__(IG_THREADS) void image_grid_kernel(const GridSources S, int n_sources, int N, int H, int clamp, int rescale,
                                                                uint8_t* __restrict__ out, int Wc, int head, int n_dwords, int total) {
  const int t = blockIdx.x * IG_THREADS + threadIdx.x;
  const int row_bytes = 3 * Wc;
  if (t < n_dwords) {
    const int b0 = head + 4 * t;
    int row = b0 / row_bytes;
    const int rem = b0 - row * row_bytes;
    int px = rem / 3, ch = rem - px * 3;
    unsigned word = 0;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      word |= ig_byte(S, n_sources, N, H, clamp, rescale, row, px, ch) << (8 * j);
      if (++ch == 3) {
        ch = 0;
        if (++px == Wc) {
          px = 0;
          ++row;
        }
      }
    }
    *reinterpret_cast<unsigned*>(out + b0) = word;
  } else {
    // the ragged ends: `head` bytes in front of the first aligned dword, the rest behind the last
    const int e = t - n_dwords;
    const int b = e < head ? e : 4 * n_dwords + e;
    if (b < total) {
      const int row = b / row_bytes, rem = b - row * row_bytes;
      const int px = rem / 3;
      out[b] = (uint8_t)ig_byte(S, n_sources, N, H, clamp, rescale, row, px, rem - px * 3);
    }
  }
}

extern "C" int lr_image_grid(const lr_grid_source* sources, int n_sources, int N, int H, int clamp, int rescale, uint8_t* out, int Wc,
                             lr_stream_t s) {
  if (!sources || !out || n_sources < 1 || n_sources > LR_GRID_MAX_SOURCES || N < 1 || H < 1 || Wc < 1) return LR_E_ARG;
  const int pad = N == 1 ? 0 : IG_PAD;
  GridSources S;
  for (int i = 0; i < n_sources; ++i) {
    const lr_grid_source& a = sources[i];
    if (!a.ptr || a.kind < LR_EVAL_PRED_F32 || a.kind > LR_EVAL_PRED_BF16 || (a.C != 1 && a.C != 3) || a.W < 1) return LR_E_ARG;
    if (a.col < 0 || (long long)a.col + a.W + 2 * pad > Wc) return LR_E_ARG;                    // leaves the canvas
    for (int j = 0; j < i; ++j)                                                                 // overlaps an earlier source's columns
      if (a.col < sources[j].col + sources[j].W + 2 * pad && sources[j].col < a.col + a.W + 2 * pad) return LR_E_ARG;
    S.s[i] = a;
  }
  const long long Hc = N == 1 ? H : (long long)N * (H + pad) + pad;
  const long long total = Hc * 3 * Wc;
  if (total > 0x7fffffffLL - 8) return LR_E_ARG;
  int head = (int)((4 - ((uintptr_t)out & 3)) & 3);
  if (head > total) head = (int)total;
  const int n_dwords = (int)((total - head) / 4);
  const long long threads = (long long)n_dwords + (total - 4LL * n_dwords);
  const unsigned blocks = (unsigned)((threads + IG_THREADS - 1) / IG_THREADS);
  hipLaunchKernelGGL(image_grid_kernel, dim3(blocks), dim3(IG_THREADS), 0, (hipStream_t)s, S, n_sources, N, H, clamp != 0, rescale != 0, out,
                     Wc, head, n_dwords, (int)total);
  return lr_launch_status();
}

// ---- token drift -------------------------------------------------------------------------------------------------------------------------
template <bool VEC>
__global__ __launch_bounds__(64) void token_drift_kernel(float* __restrict__ old_, const float* __restrict__ new_, int D,
                                                         float* __restrict__ out) {
  const int t = blockIdx.x, lane = threadIdx.x;
  float* o = old_ + (size_t)t * D;
  const float* n = new_ + (size_t)t * D;
  float acc = 0.f;
  if constexpr (VEC) {
    for (int i = lane; i < D / 4; i += 64) {
      const float4 a = reinterpret_cast<const float4*>(o)[i], b = reinterpret_cast<const float4*>(n)[i];
      const float d0 = a.x - b.x, d1 = a.y - b.y, d2 = a.z - b.z, d3 = a.w - b.w;
      acc += d0 * d0;
      acc += d1 * d1;
      acc += d2 * d2;
      acc += d3 * d3;
      reinterpret_cast<float4*>(o)[i] = b;
    }
  } else {
    for (int i = lane; i < D; i += 64) {
      const float b = n[i], d = o[i] - b;
      acc += d * d;
      o[i] = b;
    }
  }
  acc = lr_wave_sum(acc);
  if (lane == 0) out[t] = sqrtf(acc);
}

extern "C" int lr_token_drift(float* old_, const float* new_, int T, int D, float* out, lr_stream_t s) {
  if (!old_ || !new_ || !out || T < 1 || D < 1) return LR_E_ARG;
  if (old_ == new_) return LR_E_ARG;      // the snapshot is written while the tokens are read
  const bool vec = D % 4 == 0 && ((((uintptr_t)old_) | ((uintptr_t)new_)) & 15) == 0;
  if (vec)
    hipLaunchKernelGGL(token_drift_kernel<true>, dim3(T), dim3(64), 0, (hipStream_t)s, old_, new_, D, out);
  else
    hipLaunchKernelGGL(token_drift_kernel<false>, dim3(T), dim3(64), 0, (hipStream_t)s, old_, new_, D, out);
  return lr_launch_status();
}
