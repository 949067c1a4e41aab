// FID features on the device (include/leftrefill_hip.h: lr_fid_input, lr_fid_run, lr_fid_head, lr_fid_accumulate): the pool3 features of
// the Inception network of pytorch-fid as fp16 NHWC activations, and the float64 sums the Frechet distance is computed from.
//
//   input       uint8 NHWC, or an NCHW image in [-1, 1] (optionally composited with the origin under a mask, as eval_metrics.hip forms
//               it) truncated to 8 bits; / 255, bilinear to out x out (align_corners = False, no antialiasing), 2 x - 1, fp16 NHWC with
//               four channels (the fourth is zero)
//   run         an interpreter over a host table of int32 rows (LR_FID_*): one launch per row, a convolution or a pool.  Every row is
//               checked against the arena, the weight blob and the bias blob BEFORE the first launch.
//   head        mean over the final map, fp32 [B][C], pixels added in index order
//   accumulate  sum[D] += sum_r f_r, gram[D][D] += sum_r f_r f_r^T in float64: one thread per output element, rows added in order
// No atomics, no host synchronisation, no allocation, nothing read back; every sum has a fixed order, an image's rows never meet
// another image's: bitwise reproducible and independent of the rest of the batch.
//
// One convolution kernel serves all 94 layers.  Rows are output pixels, K is tap-major / channel-minor (wt [Cout][Kpad], Kpad = kh kw
// Cin rounded up to 64 with zero weights).  A loader lane fetches 8 consecutive K of one pixel (16 bytes) and works out the tap of
// ITS eight: the stored channel count is a multiple of 8, so a fetch never straddles a tap, whatever the K step does (48 and 80 need
// no padding this way; the image's 3 channels are stored as 4 and fetched 4 at a time).  K past the last tap reads as zero.
// M is small (9800 rows at 35 x 35, 512 at 8 x 8 for eight images), so the workgroup tile is 32 pixels x 64 channels x 64 K -- 80
// workgroups on the 8 x 8 map's 320-channel layers, where a 64-pixel tile would leave 40 -- in a 2-stage static LDS ring (27 KB):
// the global loads of step k + 1 are in flight while the 16x16x32 fp16 MFMAs of step k run, one barrier per step.  The weights are
// the A operand, so a lane ends up with four consecutive channels of one pixel: bias, ReLU, one 8-byte store into the channel range
// [c0, c0 + Cout) of a destination with its own channel stride -- a block's concat never exists as a copy.  Cout is guarded at the
// tile edge (weight rows past Cout load as zero and are not stored).
#include "common.h"

#pragma clang fp contract(off)

#define FI_BM 32
#define FI_BN 64
#define FI_BK 64
#define FI_LD (FI_BK + 8)      // 144-byte rows: 16-byte aligned fragments, rows spread over the banks
#define FI_THREADS 256
#define FI_ST 64               // statistics tile: 64 x 64 elements of the Gram matrix per workgroup
#define FI_SR 16               // feature rows staged per step

struct fi_conv {
  const f16* in;      // pixel (0, 0, 0), first channel read
  const f16* wt;      // [Cout][Kpad]
  const float* bias;
  f16* out;           // pixel (0, 0, 0), channel c0
  int B, Hin, Win, Cin, ldin, Hout, Wout, Cout, ldout, kh, kw, stride, ph, pw, Kpad;
};

template <bool C4>
__global__ __launch_bounds__(FI_THREADS) void fid_conv_kernel(const fi_conv c) {
  __shared__ __attribute__((aligned(16))) f16 sa[2][FI_BM][FI_LD];
  __shared__ __attribute__((aligned(16))) f16 sb[2][FI_BN][FI_LD];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int M = c.B * c.Hout * c.Wout;
  const int m0 = blockIdx.x * FI_BM, n0 = blockIdx.y * FI_BN;

  // loader roles: pixels -- row tid / 8, 8 consecutive K (16 bytes); weights -- row tid / 4, 16 consecutive K (32 bytes)
  const int arow = tid >> 3, ak = (tid & 7) * 8;
  const int brow = tid >> 2, bk = (tid & 3) * 16;
  const bool a_ok = m0 + arow < M, b_ok = n0 + brow < c.Cout;
  int iy0 = 0, ix0 = 0;
  const f16* abase = c.in;
  if (a_ok) {
    const int am = m0 + arow, hw = c.Hout * c.Wout;
    const int img = am / hw, rem = am - img * hw;
    const int oy = rem / c.Wout, ox = rem - oy * c.Wout;
    iy0 = oy * c.stride - c.ph;
    ix0 = ox * c.stride - c.pw;
    abase += (size_t)img * c.Hin * c.Win * c.ldin;
  }
  const f16* wrow = c.wt + (size_t)(b_ok ? n0 + brow : 0) * c.Kpad + bk;
  const int Kreal = c.kh * c.kw * c.Cin;
  uint4 ra, rb[2];

  // the source address of K index k of this lane's pixel, or null for a tap outside the image / past the last tap
  auto tap_ptr = [&](int k) -> const f16* {
    if (!a_ok || k >= Kreal) return nullptr;
    const int tap = k / c.Cin, ch = k - tap * c.Cin;
    const int ky = tap / c.kw, kx = tap - ky * c.kw;
    const int iy = iy0 + ky, ix = ix0 + kx;
    if (iy < 0 || iy >= c.Hin || ix < 0 || ix >= c.Win) return nullptr;
    return abase + ((size_t)iy * c.Win + ix) * c.ldin + ch;
  };
  auto fetch = [&](int kk) {
    rb[0] = rb[1] = make_uint4(0u, 0u, 0u, 0u);
    if (b_ok) {
      const uint4* wp = reinterpret_cast<const uint4*>(wrow + (size_t)kk * FI_BK);
      rb[0] = wp[0];
      rb[1] = wp[1];
    }
    const int k = kk * FI_BK + ak;
    ra = make_uint4(0u, 0u, 0u, 0u);
    if (C4) {      // four stored channels per tap: two taps per 16 bytes
      const f16* p0 = tap_ptr(k);
      const f16* p1 = tap_ptr(k + 4);
      if (p0) {
        const uint2 v = *reinterpret_cast<const uint2*>(p0);
        ra.x = v.x;
        ra.y = v.y;
      }
      if (p1) {
        const uint2 v = *reinterpret_cast<const uint2*>(p1);
        ra.z = v.x;
        ra.w = v.y;
      }
    } else {
      const f16* p = tap_ptr(k);
      if (p) ra = *reinterpret_cast<const uint4*>(p);
    }
  };
  auto stash = [&](int buf) {
    *reinterpret_cast<uint4*>(&sa[buf][arow][ak]) = ra;
    uint4* pb = reinterpret_cast<uint4*>(&sb[buf][brow][bk]);
    pb[0] = rb[0];
    pb[1] = rb[1];
  };

  // compute role: wave w owns channels 16 w .. 16 w + 15 of the tile and all 32 pixels = 2 MFMA tiles
  f32x4_t acc[2];
#pragma unroll
  for (int i = 0; i < 2; ++i) acc[i] = (f32x4_t){0.f, 0.f, 0.f, 0.f};

  const int KT = c.Kpad / FI_BK;
  fetch(0);
  stash(0);
  __syncthreads();
  for (int kk = 0; kk < KT; ++kk) {
    const int buf = kk & 1;
    if (kk + 1 < KT) fetch(kk + 1);
#pragma unroll
    for (int ks = 0; ks < FI_BK / 32; ++ks) {
      const int kof = ks * 32 + (lane >> 4) * 8;
      const f16x8 wf = *reinterpret_cast<const f16x8*>(&sb[buf][16 * wave + (lane & 15)][kof]);
#pragma unroll
      for (int i = 0; i < 2; ++i) {
        const f16x8 xf = *reinterpret_cast<const f16x8*>(&sa[buf][16 * i + (lane & 15)][kof]);
        acc[i] = lr_mfma16(wf, xf, acc[i]);
      }
    }
    if (kk + 1 < KT) stash(buf ^ 1);      // last read before the barrier that ended step kk - 1
    __syncthreads();
  }

  // epilogue: D[channel][pixel] -- column (pixel) on lane & 15, rows (channels) 4 (lane >> 4) .. + 3 in the four registers
  const int ch = n0 + 16 * wave + (lane >> 4) * 4;
  if (ch >= c.Cout) return;      // Cout % 4 == 0: a group of four is inside or outside as a whole
  const float4 b = *reinterpret_cast<const float4*>(c.bias + ch);
#pragma unroll
  for (int i = 0; i < 2; ++i) {
    const int p = m0 + 16 * i + (lane & 15);
    if (p >= M) continue;
    f16x4 h;
    h[0] = (f16)fmaxf(acc[i][0] + b.x, 0.f);
    h[1] = (f16)fmaxf(acc[i][1] + b.y, 0.f);
    h[2] = (f16)fmaxf(acc[i][2] + b.z, 0.f);
    h[3] = (f16)fmaxf(acc[i][3] + b.w, 0.f);
    *reinterpret_cast<f16x4*>(c.out + (size_t)p * c.ldout + ch) = h;
  }
}

struct fi_pool {
  const f16* in;
  f16* out;
  int B, Hin, Win, C, ldin, Hout, Wout, ldout, op;
};

// The three 3 x 3 pools, NHWC fp16, one thread per 8 channels of an output pixel.  LR_FID_OP_MAXPOOL_S2: stride 2, floor, no padding;
// LR_FID_OP_MAXPOOL_S1: stride 1, pad 1, taps outside the image are skipped (-inf, never 0); LR_FID_OP_AVGPOOL_S1: stride 1, pad 1,
// fp32 sum of the taps inside the image in (dy, dx) order, divided by their number.
__global__ __launch_bounds__(FI_THREADS) void fid_pool_kernel(const fi_pool a) {
  const int c8n = a.C / 8;
  const long long total = (long long)a.B * a.Hout * a.Wout * c8n;
  const long long idx = (long long)blockIdx.x * FI_THREADS + threadIdx.x;
  if (idx >= total) return;
  const int c8 = (int)(idx % c8n);
  long long pix = idx / c8n;
  const int px = (int)(pix % a.Wout);
  pix /= a.Wout;
  const int py = (int)(pix % a.Hout), b = (int)(pix / a.Hout);
  const bool avg = a.op == LR_FID_OP_AVGPOOL_S1;
  const int st = a.op == LR_FID_OP_MAXPOOL_S2 ? 2 : 1, pad = a.op == LR_FID_OP_MAXPOOL_S2 ? 0 : 1;
  float v[8];
#pragma unroll
  for (int q = 0; q < 8; ++q) v[q] = avg ? 0.f : -INFINITY;
  int cnt = 0;
  for (int dy = 0; dy < 3; ++dy) {
    const int iy = py * st + dy - pad;
    if (iy < 0 || iy >= a.Hin) continue;
    for (int dx = 0; dx < 3; ++dx) {
      const int ix = px * st + dx - pad;
      if (ix < 0 || ix >= a.Win) continue;
      const uint4 u = *reinterpret_cast<const uint4*>(a.in + (((size_t)b * a.Hin + iy) * a.Win + ix) * a.ldin + c8 * 8);
      float f[8];
      lr_unpack8<f16>(u, f);
#pragma unroll
      for (int q = 0; q < 8; ++q) v[q] = avg ? v[q] + f[q] : fmaxf(v[q], f[q]);
      ++cnt;
    }
  }
  if (avg) {
    const float d = (float)cnt;
#pragma unroll
    for (int q = 0; q < 8; ++q) v[q] = v[q] / d;
  }
  *reinterpret_cast<uint4*>(a.out + (((size_t)b * a.Hout + py) * a.Wout + px) * a.ldout + c8 * 8) = lr_pack8<f16>(v);
}

// mean over the HW pixels of the final map: one thread per (image, channel), pixels in index order, fp32
__global__ __launch_bounds__(FI_THREADS) void fid_head_kernel(const f16* __restrict__ in, int B, int HW, int C, int ld, float* __restrict__ out) {
  const int idx = blockIdx.x * FI_THREADS + threadIdx.x;
  if (idx >= B * C) return;
  const int b = idx / C, ch = idx - b * C;
  const f16* p = in + (size_t)b * HW * ld + ch;
  float s = 0.f;
  for (int i = 0; i < HW; ++i) s += (float)p[(size_t)i * ld];
  out[idx] = s / (float)HW;
}

struct fi_input {
  const void* src;
  const float* origin;
  const float* mask;
  int N, H, W, x0, Wc, out;
  f16* dst;
};

// the 8-bit value of channel ch of source pixel (y, x0 + x) of image n, as a float in 0 .. 255
template <typename T>
__device__ __forceinline__ float fi_byte(const fi_input& a, int n, int ch, int y, int x) {
  if constexpr (sizeof(T) == 1) {
    return (float)((const uint8_t*)a.src)[(((size_t)n * a.H + y) * a.W + a.x0 + x) * 3 + ch];
  } else {
    const size_t plane = (size_t)a.H * a.W, row = (size_t)y * a.W + (size_t)(a.x0 + x);
    const size_t at = ((size_t)n * 3 + ch) * plane + row;
    float v = (float)((const T*)a.src)[at];
    if (a.mask) {      // the composite of eval_metrics.hip, same order of operations
      const float m = a.mask[(size_t)n * plane + row];
      v = v * m + a.origin[at] * (1.f - m);
    }
    return (float)(uint8_t)((fminf(fmaxf(v, -1.f), 1.f) + 1.f) / 2.f * 255.f);
  }
}

// One thread per output pixel: source coordinate max(0, (d + 0.5) in / out - 0.5), upper index clamped to the last pixel.  The bytes
// are exact; the coordinate and the blend are float64, because 2 v - 1 cancels around mid-grey and the stored fp16 is finer there than
// fp32 arithmetic on values near 1 (and than an fp32 coordinate near 512) can follow.  715 k pixels per batch of eight: nothing to save.
template <typename T>
__global__ __launch_bounds__(FI_THREADS) void fid_input_kernel(const fi_input a) {
  const long long idx = (long long)blockIdx.x * FI_THREADS + threadIdx.x;
  if (idx >= (long long)a.N * a.out * a.out) return;
  const int ox = (int)(idx % a.out);
  const long long t = idx / a.out;
  const int oy = (int)(t % a.out), n = (int)(t / a.out);
  const double sy = fmax(((double)oy + 0.5) * ((double)a.H / (double)a.out) - 0.5, 0.0);
  const double sx = fmax(((double)ox + 0.5) * ((double)a.Wc / (double)a.out) - 0.5, 0.0);
  const int y0 = min((int)sy, a.H - 1), x0 = min((int)sx, a.Wc - 1);
  const int y1 = min(y0 + 1, a.H - 1), x1 = min(x0 + 1, a.Wc - 1);
  const double ly = sy - (double)y0, lx = sx - (double)x0;
  f16x4 h;
#pragma unroll
  for (int ch = 0; ch < 3; ++ch) {
    const double p00 = (double)fi_byte<T>(a, n, ch, y0, x0) / 255.0, p01 = (double)fi_byte<T>(a, n, ch, y0, x1) / 255.0;
    const double p10 = (double)fi_byte<T>(a, n, ch, y1, x0) / 255.0, p11 = (double)fi_byte<T>(a, n, ch, y1, x1) / 255.0;
    const double v = (1.0 - ly) * ((1.0 - lx) * p00 + lx * p01) + ly * ((1.0 - lx) * p10 + lx * p11);
    h[ch] = (f16)(float)(2.0 * v - 1.0);
  }
  h[3] = (f16)0.f;
  *reinterpret_cast<f16x4*>(a.dst + (size_t)idx * 4) = h;
}

// Workgroup (bj, bi) owns gram[64 bi .. + 63][64 bj .. + 63], thread (ty, tx) a 4 x 4 patch of it; the bj == 0 column also owns
// sum[64 bi .. + 63].  Feature rows are staged 16 at a time and added in row order; a product of two fp32 values is exact in fp64.
__global__ __launch_bounds__(FI_THREADS) void fid_stats_kernel(const float* __restrict__ f, int n, int D, double* __restrict__ sum,
                                                                double* __restrict__ gram) {
  __shared__ float fi[FI_SR][FI_ST], fj[FI_SR][FI_ST];
  const int tid = threadIdx.x, ty = tid >> 4, tx = tid & 15;
  const int i0 = blockIdx.y * FI_ST, j0 = blockIdx.x * FI_ST;
  double g[4][4];
#pragma unroll
  for (int a = 0; a < 4; ++a)
#pragma unroll
    for (int b = 0; b < 4; ++b) g[a][b] = gram[(size_t)(i0 + 4 * ty + a) * D + j0 + 4 * tx + b];
  const bool sums = blockIdx.x == 0 && tid < FI_ST;
  double s = sums ? sum[i0 + tid] : 0.0;
  for (int r0 = 0; r0 < n; r0 += FI_SR) {
    const int rows = min(FI_SR, n - r0);
    for (int e = tid; e < FI_SR * FI_ST; e += FI_THREADS) {
      const int r = e / FI_ST, col = e - r * FI_ST;
      fi[r][col] = r < rows ? f[(size_t)(r0 + r) * D + i0 + col] : 0.f;
      fj[r][col] = r < rows ? f[(size_t)(r0 + r) * D + j0 + col] : 0.f;
    }
    __syncthreads();
    for (int r = 0; r < rows; ++r) {
#pragma unroll
      for (int a = 0; a < 4; ++a)
#pragma unroll
        for (int b = 0; b < 4; ++b) g[a][b] += (double)fi[r][4 * ty + a] * (double)fj[r][4 * tx + b];
      if (sums) s += (double)fi[r][tid];
    }
    __syncthreads();
  }
#pragma unroll
  for (int a = 0; a < 4; ++a)
#pragma unroll
    for (int b = 0; b < 4; ++b) gram[(size_t)(i0 + 4 * ty + a) * D + j0 + 4 * tx + b] = g[a][b];
  if (sums) sum[i0 + tid] = s;
}

// ---- host side: argument checks, the interpreter ----
static inline void fi_count(int* launches) {
  if (launches) ++*launches;
}

extern "C" int lr_fid_input(const void* src, int kind, const float* origin, const float* mask, int N, int H, int W, int x0, int Wc,
                            lr_half* dst, int out, int* launches, lr_stream_t s) {
  if (!src || !dst || kind < LR_EVAL_PRED_F32 || kind > LR_FID_SRC_U8) return LR_E_ARG;
  if (N <= 0 || H <= 0 || W <= 0 || out <= 0 || x0 < 0 || Wc <= 0 || x0 > W - Wc) return LR_E_ARG;
  if (mask && (!origin || kind == LR_FID_SRC_U8)) return LR_E_ARG;
  if ((int64_t)N * out * out > 0x7fffffff || (int64_t)N * H * W > 0x7fffffff / 3) return LR_E_ARG;
  if ((uintptr_t)dst & 7) return LR_E_ALIGN;
  const fi_input a = {src, origin, mask, N, H, W, x0, Wc, out, (f16*)dst};
  const unsigned grid = (unsigned)(((long long)N * out * out + FI_THREADS - 1) / FI_THREADS);
  hipStream_t st = (hipStream_t)s;
  if (kind == LR_FID_SRC_U8)
    fid_input_kernel<uint8_t><<<grid, FI_THREADS, 0, st>>>(a);
  else if (kind == LR_EVAL_PRED_F32)
    fid_input_kernel<float><<<grid, FI_THREADS, 0, st>>>(a);
  else if (kind == LR_EVAL_PRED_F16)
    fid_input_kernel<f16><<<grid, FI_THREADS, 0, st>>>(a);
  else
    fid_input_kernel<bf16><<<grid, FI_THREADS, 0, st>>>(a);
  fi_count(launches);
  return lr_launch_status();
}

// one row against the arena (halves), the weight blob (halves) and the bias blob (floats); 0 or LR_E_ARG
static int fi_check_row(const int32_t* r, int B, int64_t arena_halfs, int64_t wt_halfs, int64_t bias_floats) {
  for (int i = 0; i < LR_FID_ROW_WORDS; ++i)
    if (r[i] < 0) return LR_E_ARG;
  const int op = r[LR_FID_OP];
  if (op < LR_FID_OP_CONV || op > LR_FID_OP_AVGPOOL_S1) return LR_E_ARG;
  const int Hin = r[LR_FID_HIN], Win = r[LR_FID_WIN], Cin = r[LR_FID_CIN], Hout = r[LR_FID_HOUT], Wout = r[LR_FID_WOUT], Cout = r[LR_FID_COUT];
  if (Hin < 1 || Win < 1 || Cin < 1 || Hout < 1 || Wout < 1 || Cout < 1) return LR_E_ARG;
  const int g = (op == LR_FID_OP_CONV && Cin == 4) ? 4 : 8;      // halves per source fetch
  if (Cin % g || r[LR_FID_SRC_LD] % g || r[LR_FID_SRC_C0] % g || r[LR_FID_SRC_OFF] % 8) return LR_E_ARG;
  if ((int64_t)r[LR_FID_SRC_C0] + Cin > r[LR_FID_SRC_LD]) return LR_E_ARG;
  const int gd = op == LR_FID_OP_CONV ? 4 : 8;                   // halves per store
  if (Cout % gd || r[LR_FID_DST_LD] % gd || r[LR_FID_DST_C0] % gd || r[LR_FID_DST_OFF] % 8) return LR_E_ARG;
  if ((int64_t)r[LR_FID_DST_C0] + Cout > r[LR_FID_DST_LD]) return LR_E_ARG;
  if (((int64_t)r[LR_FID_SRC_OFF] + (int64_t)Hin * Win * r[LR_FID_SRC_LD]) * B > arena_halfs) return LR_E_ARG;
  if (((int64_t)r[LR_FID_DST_OFF] + (int64_t)Hout * Wout * r[LR_FID_DST_LD]) * B > arena_halfs) return LR_E_ARG;
  if ((int64_t)B * Hout * Wout > 0x7fffffff - FI_BM || (int64_t)B * Hin * Win * r[LR_FID_SRC_LD] > 0x7fffffffffffLL) return LR_E_ARG;
  int kh = 3, kw = 3, stride = 1, ph = 1, pw = 1;
  if (op == LR_FID_OP_CONV) {
    kh = r[LR_FID_KH], kw = r[LR_FID_KW], stride = r[LR_FID_STRIDE], ph = r[LR_FID_PH], pw = r[LR_FID_PW];
    const bool shape = (kh == kw && (kh == 1 || kh == 3 || kh == 5)) || (kh == 1 && (kw == 7 || kw == 3)) || (kw == 1 && (kh == 7 || kh == 3));
    if (!shape || stride < 1 || stride > 2 || ph >= kh || pw >= kw) return LR_E_ARG;
    const int64_t K = (int64_t)kh * kw * Cin, Kpad = r[LR_FID_KPAD];
    if (Kpad % FI_BK || Kpad < K || Kpad >= K + FI_BK) return LR_E_ARG;
    if (r[LR_FID_W_OFF] % 8 || (int64_t)r[LR_FID_W_OFF] + (int64_t)Cout * Kpad > wt_halfs) return LR_E_ARG;
    if (r[LR_FID_B_OFF] % 4 || (int64_t)r[LR_FID_B_OFF] + Cout > bias_floats) return LR_E_ARG;
  } else {
    if (Cin != Cout) return LR_E_ARG;
    if (op == LR_FID_OP_MAXPOOL_S2) stride = 2, ph = pw = 0;
  }
  if (Hin + 2 * ph < kh || Win + 2 * pw < kw) return LR_E_ARG;
  if (Hout != (Hin + 2 * ph - kh) / stride + 1 || Wout != (Win + 2 * pw - kw) / stride + 1) return LR_E_ARG;
  return 0;
}

extern "C" int lr_fid_run(const int32_t* program, int n_rows, int B, lr_half* arena, int64_t arena_halfs, const lr_half* wt,
                          int64_t wt_halfs, const float* bias, int64_t bias_floats, int* launches, lr_stream_t s) {
  if (!program || !arena || n_rows < 1 || B < 1 || B > 32767 || arena_halfs < 1 || wt_halfs < 0 || bias_floats < 0) return LR_E_ARG;
  bool conv = false;
  for (int i = 0; i < n_rows; ++i) {
    const int rc = fi_check_row(program + (size_t)i * LR_FID_ROW_WORDS, B, arena_halfs, wt_halfs, bias_floats);
    if (rc) return rc;
    conv |= program[(size_t)i * LR_FID_ROW_WORDS + LR_FID_OP] == LR_FID_OP_CONV;
  }
  if (conv && (!wt || !bias)) return LR_E_ARG;
  if (((uintptr_t)arena | (uintptr_t)wt | (uintptr_t)bias) & 15) return LR_E_ALIGN;

  hipStream_t st = (hipStream_t)s;
  f16* base = (f16*)arena;
  for (int i = 0; i < n_rows; ++i) {
    const int32_t* r = program + (size_t)i * LR_FID_ROW_WORDS;
    const f16* in = base + (size_t)r[LR_FID_SRC_OFF] * B + r[LR_FID_SRC_C0];
    f16* out = base + (size_t)r[LR_FID_DST_OFF] * B + r[LR_FID_DST_C0];
    if (r[LR_FID_OP] == LR_FID_OP_CONV) {
      const fi_conv c = {in, (const f16*)wt + r[LR_FID_W_OFF], bias + r[LR_FID_B_OFF], out, B, r[LR_FID_HIN], r[LR_FID_WIN], r[LR_FID_CIN],
                         r[LR_FID_SRC_LD], r[LR_FID_HOUT], r[LR_FID_WOUT], r[LR_FID_COUT], r[LR_FID_DST_LD], r[LR_FID_KH], r[LR_FID_KW],
                         r[LR_FID_STRIDE], r[LR_FID_PH], r[LR_FID_PW], r[LR_FID_KPAD]};
      const int M = B * c.Hout * c.Wout;
      const dim3 grid((unsigned)((M + FI_BM - 1) / FI_BM), (unsigned)((c.Cout + FI_BN - 1) / FI_BN));
      if (c.Cin == 4)
        fid_conv_kernel<true><<<grid, FI_THREADS, 0, st>>>(c);
      else
        fid_conv_kernel<false><<<grid, FI_THREADS, 0, st>>>(c);
    } else {
      const fi_pool p = {in, out, B, r[LR_FID_HIN], r[LR_FID_WIN], r[LR_FID_CIN], r[LR_FID_SRC_LD], r[LR_FID_HOUT], r[LR_FID_WOUT],
                         r[LR_FID_DST_LD], r[LR_FID_OP]};
      const long long total = (long long)B * p.Hout * p.Wout * (p.C / 8);
      fid_pool_kernel<<<(unsigned)((total + FI_THREADS - 1) / FI_THREADS), FI_THREADS, 0, st>>>(p);
    }
    fi_count(launches);
    const int rc = lr_launch_status();
    if (rc) return rc;
  }
  return 0;
}

extern "C" int lr_fid_head(const lr_half* src, int B, int HW, int C, int ld, float* out, int* launches, lr_stream_t s) {
  if (!src || !out || B < 1 || HW < 1 || C < 1 || ld < C || (int64_t)B * C > 0x7fffffff) return LR_E_ARG;
  fid_head_kernel<<<(unsigned)((B * C + FI_THREADS - 1) / FI_THREADS), FI_THREADS, 0, (hipStream_t)s>>>((const f16*)src, B, HW, C, ld, out);
  fi_count(launches);
  return lr_launch_status();
}

extern "C" int lr_fid_accumulate(const float* feats, int n, int D, double* sum, double* gram, int* launches, lr_stream_t s) {
  if (!feats || !sum || !gram || n < 1 || D < FI_ST || D % FI_ST || D > 65535 * FI_ST) return LR_E_ARG;
  if (((uintptr_t)sum | (uintptr_t)gram) & 7) return LR_E_ALIGN;
  fid_stats_kernel<<<dim3(D / FI_ST, D / FI_ST), FI_THREADS, 0, (hipStream_t)s>>>(feats, n, D, sum, gram);
  fi_count(launches);
  return lr_launch_status();
}
