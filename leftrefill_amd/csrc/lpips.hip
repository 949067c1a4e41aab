// LPIPS(alex) of a decoded prediction on the device (include/leftrefill_hip.h: lr_lpips_alex): the five ReLU stages of AlexNet's
// `features` as implicit-GEMM convolutions on the matrix cores, and the learned distance on their outputs.
//
// The 2N images of a call -- N composited predictions, then the N origins -- run as ONE batch through every launch:
//   conv 1          the scored image is formed in the gather: fp32 composite pred m + origin (1 - m), columns [x0, x0 + Wc), r x r area
//                   mean (the order of operations of eval_metrics.hip), (x - shift) / scale, rounded to fp16; it is never written to
//                   memory.  A tap outside the scored image is 0 in the NORMALISED space, as the padding of the torch convolution is.
//   pool, conv 2    MaxPool(3, 2) of stage 1 as its own small kernel, then 5 x 5 on 64 channels
//   pool, conv 3    MaxPool(3, 2) of stage 2, then 3 x 3 on 192 channels
//   conv 4, conv 5  3 x 3 on 384 / 256 channels
//   head x 5        per stage and pixel: na = fa / (|fa| + 1e-10), nb likewise, sum_c lin_c (na_c - nb_c)^2 in fp32 -- one wave per
//                   pixel, the normalised features live in registers only; a workgroup adds its 64 pixels in fp64 into its own slot
//   finish          one wave per sample: slots of a stage in a fixed order (fp64), / pixels of the stage, stages 1..5 in turn
// LPIPS_LAUNCHES = 13 launches whatever N and whatever the image size.  No atomics, no host synchronisation, no allocation: every sum
// has a fixed order, a sample's rows never meet another sample's, so the result is bitwise reproducible and does not depend on the
// rest of the batch.
//
// One convolution kernel serves all five stages.  Rows are output pixels, K is tap-major / channel-minor (wt [Cout][Kpad], Kpad a
// multiple of 64: conv 1 pads 363 -> 384 with zero weights), the workgroup tile is 64 pixels x 64 channels x 64 K in a 2-stage LDS ring
// (static, 36 KB: no MaxDynamicSharedMemorySize to get wrong): the global loads of step k + 1 are in flight while the 16x16x32 fp16
// MFMAs of step k run, one barrier per step.  The weights are the A operand, so a lane ends up with four consecutive channels of one
// pixel: bias, ReLU and one 8-byte NHWC store.  Every channel count is a multiple of 64, so a K step never straddles two taps.
// M is small (129 k rows at stage 1, 7.7 k at stages 3-5 for N = 4 at 512 x 512): this is a scoring tail, not the step.
#include "common.h"

#pragma clang fp contract(off)

#define LP_BM 64
#define LP_BN 64
#define LP_BK 64
#define LP_LD (LP_BK + 8)      // 144-byte rows: 16-byte aligned fragments, rows spread over the banks
#define LP_THREADS 256
#define LP_HEAD_PIX LR_LPIPS_HEAD_PIXELS
#define LP_STAGES 5

struct lp_conv {
  const f16* in;      // NHWC [B][Hin][Win][Cin] (stages 2-5)
  const f16* wt;      // [Cout][Kpad]
  const float* bias;
  f16* out;           // NHWC [B][Hout][Wout][Cout]
  int B, Hin, Win, Cin, Hout, Wout, Cout, ks, stride, pad, Kpad;
};

struct lp_image {
  const void* pred;
  const float* origin;
  const float* mask;
  int N, H, W, x0, r, Ho, Wo;
};

__constant__ float lp_shift[3] = {-0.030f, -0.088f, -0.188f};
__constant__ float lp_scale[3] = {0.458f, 0.448f, 0.450f};

// one pixel of the scored image of batch entry `img` (img < N: composited prediction; else origin), channel ch
template <typename T>
__device__ __forceinline__ float lp_pixel(const lp_image& im, int img, int ch, int y, int x) {
  const bool is_pred = img < im.N;
  const int n = is_pred ? img : img - im.N;
  const size_t plane = (size_t)im.H * im.W;
  const T* pred = (const T*)im.pred;
  float acc = 0.f;
  for (int dy = 0; dy < im.r; ++dy) {
    const size_t row = (size_t)(y * im.r + dy) * im.W + (size_t)(im.x0 + x * im.r);
    for (int dx = 0; dx < im.r; ++dx) {
      const size_t at = ((size_t)n * 3 + ch) * plane + row + dx;
      const float ov = im.origin[at];
      if (is_pred) {
        const float pv = (float)pred[at];
        if (im.mask) {
          const float m = im.mask[(size_t)n * plane + row + dx];
          acc += pv * m + ov * (1.f - m);
        } else {
          acc += pv;
        }
      } else {
        acc += ov;
      }
    }
  }
  if (im.r > 1) {
    const float fr = (float)im.r;
    acc = acc / fr / fr;
  }
  return acc;
}

template <typename T, bool IMAGE>
__global__ __launch_bounds__(LP_THREADS) void lpips_conv_kernel(const lp_conv c, const lp_image im) {
  __shared__ __attribute__((aligned(16))) f16 sa[2][LP_BM][LP_LD];
  __shared__ __attribute__((aligned(16))) f16 sb[2][LP_BN][LP_LD];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const long long M = (long long)c.B * c.Hout * c.Wout;
  const long long m0 = (long long)blockIdx.x * LP_BM;
  const int n0 = blockIdx.y * LP_BN;

  // loader role: row tid / 4 of either tile, 16 consecutive K (32 bytes) of it
  const int lrow = tid >> 2, lk = (tid & 3) * 16;
  const long long lm = m0 + lrow;
  const bool lm_ok = lm < M;
  int img = 0, oy = 0, ox = 0;
  if (lm_ok) {
    const int hw = c.Hout * c.Wout;
    img = (int)(lm / hw);
    const int rem = (int)(lm - (long long)img * hw);
    oy = rem / c.Wout;
    ox = rem - oy * c.Wout;
  }
  const f16* wrow = c.wt + (size_t)(n0 + lrow) * c.Kpad + lk;      // Cout % 64 == 0: every row of the tile exists
  uint4 ra[2], rb[2];

  auto fetch = [&](int kk) {
    const uint4* wp = reinterpret_cast<const uint4*>(wrow + (size_t)kk * LP_BK);
    rb[0] = wp[0];
    rb[1] = wp[1];
    if (IMAGE) {
      f16 v[16];
#pragma unroll
      for (int j = 0; j < 16; ++j) {
        const int k = kk * LP_BK + lk + j;
        float x = 0.f;
        if (lm_ok && k < c.ks * c.ks * 3) {
          const int tap = k / 3, ch = k - tap * 3;
          const int ky = tap / c.ks, kx = tap - ky * c.ks;
          const int iy = oy * c.stride + ky - c.pad, ix = ox * c.stride + kx - c.pad;
          if (iy >= 0 && iy < im.Ho && ix >= 0 && ix < im.Wo) x = (lp_pixel<T>(im, img, ch, iy, ix) - lp_shift[ch]) / lp_scale[ch];
        }
        v[j] = (f16)x;
      }
      ra[0] = __builtin_bit_cast(uint4, *reinterpret_cast<f16x8*>(&v[0]));
      ra[1] = __builtin_bit_cast(uint4, *reinterpret_cast<f16x8*>(&v[8]));
    } else {
      const int k = kk * LP_BK;
      const int tap = k / c.Cin, c0 = k - tap * c.Cin;
      const int ky = tap / c.ks, kx = tap - ky * c.ks;
      const int iy = oy * c.stride + ky - c.pad, ix = ox * c.stride + kx - c.pad;
      ra[0] = ra[1] = make_uint4(0u, 0u, 0u, 0u);
      if (lm_ok && iy >= 0 && iy < c.Hin && ix >= 0 && ix < c.Win) {
        const uint4* ap = reinterpret_cast<const uint4*>(c.in + (((size_t)img * c.Hin + iy) * c.Win + ix) * c.Cin + c0 + lk);
        ra[0] = ap[0];
        ra[1] = ap[1];
      }
    }
  };
  auto stash = [&](int buf) {
    uint4* pa = reinterpret_cast<uint4*>(&sa[buf][lrow][lk]);
    uint4* pb = reinterpret_cast<uint4*>(&sb[buf][lrow][lk]);
    pa[0] = ra[0];
    pa[1] = ra[1];
    pb[0] = rb[0];
    pb[1] = rb[1];
  };

  // compute role: wave (wm, wn) owns 32 pixels x 32 channels = 2 x 2 MFMA tiles
  const int wm = wave & 1, wn = wave >> 1;
  f32x4_t acc[2][2];
#pragma unroll
  for (int j = 0; j < 2; ++j)
#pragma unroll
    for (int i = 0; i < 2; ++i) acc[j][i] = (f32x4_t){0.f, 0.f, 0.f, 0.f};

  const int KT = c.Kpad / LP_BK;
  fetch(0);
  stash(0);
  __syncthreads();
  for (int kk = 0; kk < KT; ++kk) {
    const int buf = kk & 1;
    if (kk + 1 < KT) fetch(kk + 1);
#pragma unroll
    for (int ks = 0; ks < LP_BK / 32; ++ks) {
      const int kof = ks * 32 + (lane >> 4) * 8;
      f16x8 xf[2], wf[2];
#pragma unroll
      for (int i = 0; i < 2; ++i) xf[i] = *reinterpret_cast<const f16x8*>(&sa[buf][32 * wm + 16 * i + (lane & 15)][kof]);
#pragma unroll
      for (int j = 0; j < 2; ++j) wf[j] = *reinterpret_cast<const f16x8*>(&sb[buf][32 * wn + 16 * j + (lane & 15)][kof]);
#pragma unroll
      for (int j = 0; j < 2; ++j)
#pragma unroll
        for (int i = 0; i < 2; ++i) acc[j][i] = lr_mfma16(wf[j], xf[i], acc[j][i]);
    }
    if (kk + 1 < KT) stash(buf ^ 1);      // last read before the barrier that ended step kk - 1
    __syncthreads();
  }

  // epilogue: D[channel][pixel] -- column (pixel) on lane & 15, rows (channels) 4 (lane >> 4) .. + 3 in the four registers
#pragma unroll
  for (int i = 0; i < 2; ++i) {
    const long long p = m0 + 32 * wm + 16 * i + (lane & 15);
    if (p >= M) continue;
#pragma unroll
    for (int j = 0; j < 2; ++j) {
      const int ch = n0 + 32 * wn + 16 * j + (lane >> 4) * 4;
      const float4 b = *reinterpret_cast<const float4*>(c.bias + ch);
      f16x4 h;
      h[0] = (f16)fmaxf(acc[j][i][0] + b.x, 0.f);
      h[1] = (f16)fmaxf(acc[j][i][1] + b.y, 0.f);
      h[2] = (f16)fmaxf(acc[j][i][2] + b.z, 0.f);
      h[3] = (f16)fmaxf(acc[j][i][3] + b.w, 0.f);
      *reinterpret_cast<f16x4*>(c.out + (size_t)p * c.Cout + ch) = h;
    }
  }
}

// MaxPool2d(3, 2), floor mode, no padding, NHWC fp16; one thread per 8 channels of an output pixel
__global__ __launch_bounds__(LP_THREADS) void lpips_pool_kernel(const f16* __restrict__ in, f16* __restrict__ out, int B, int H, int W,
                                                                int Hp, int Wp, int C) {
  const long long total = (long long)B * Hp * Wp * (C / 8);
  const long long idx = (long long)blockIdx.x * LP_THREADS + threadIdx.x;
  if (idx >= total) return;
  const int c8 = (int)(idx % (C / 8));
  long long pix = idx / (C / 8);
  const int px = (int)(pix % Wp);
  pix /= Wp;
  const int py = (int)(pix % Hp), b = (int)(pix / Hp);
  float mx[8];
#pragma unroll
  for (int q = 0; q < 8; ++q) mx[q] = -INFINITY;
#pragma unroll
  for (int dy = 0; dy < 3; ++dy)
#pragma unroll
    for (int dx = 0; dx < 3; ++dx) {      // 2 py + 2 <= H - 1 by Hp = (H - 3) / 2 + 1
      const uint4 u = *reinterpret_cast<const uint4*>(in + (((size_t)b * H + 2 * py + dy) * W + 2 * px + dx) * C + c8 * 8);
      float f[8];
      lr_unpack8<f16>(u, f);
#pragma unroll
      for (int q = 0; q < 8; ++q) mx[q] = fmaxf(mx[q], f[q]);
    }
  *reinterpret_cast<uint4*>(out + (((size_t)b * Hp + py) * Wp + px) * C + c8 * 8) = lr_pack8<f16>(mx);
}

__device__ __forceinline__ double lp_wave_sum(double v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}

// The distance of one stage.  act [2N][P][C]: sample n's prediction features at image n, its origin's at image n + N.
// Workgroup (x, n) scores pixels 64 x .. 64 x + 63 of sample n, wave w the 16 from 64 x + 16 w on, in turn.
__global__ __launch_bounds__(LP_THREADS) void lpips_head_kernel(const f16* __restrict__ act, const float* __restrict__ lin, int N, int P,
                                                                int C, double* __restrict__ slots) {
  __shared__ double red[LP_THREADS / 64];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int n = blockIdx.y;
  float w[3][2];
#pragma unroll
  for (int it = 0; it < 3; ++it) {
    const int ch = it * 128 + lane * 2;
    w[it][0] = ch < C ? lin[ch] : 0.f;
    w[it][1] = ch < C ? lin[ch + 1] : 0.f;
  }
  double total = 0.0;
  for (int q = 0; q < LP_HEAD_PIX / 4; ++q) {
    const int pix = blockIdx.x * LP_HEAD_PIX + wave * (LP_HEAD_PIX / 4) + q;
    if (pix >= P) break;      // wave-uniform
    const f16* fa = act + ((size_t)n * P + pix) * C;
    const f16* fb = act + ((size_t)(n + N) * P + pix) * C;
    float a[3][2], b[3][2];
    float sa2 = 0.f, sb2 = 0.f;
#pragma unroll
    for (int it = 0; it < 3; ++it) {
      const int ch = it * 128 + lane * 2;
      a[it][0] = a[it][1] = b[it][0] = b[it][1] = 0.f;
      if (ch < C) {
        const f16x2 ha = *reinterpret_cast<const f16x2*>(fa + ch), hb = *reinterpret_cast<const f16x2*>(fb + ch);
        a[it][0] = (float)ha[0];
        a[it][1] = (float)ha[1];
        b[it][0] = (float)hb[0];
        b[it][1] = (float)hb[1];
      }
      sa2 += a[it][0] * a[it][0];
      sa2 += a[it][1] * a[it][1];
      sb2 += b[it][0] * b[it][0];
      sb2 += b[it][1] * b[it][1];
    }
    const float na = sqrtf(lr_wave_sum(sa2)) + 1e-10f, nb = sqrtf(lr_wave_sum(sb2)) + 1e-10f;
    float s = 0.f;
#pragma unroll
    for (int it = 0; it < 3; ++it)
#pragma unroll
      for (int e = 0; e < 2; ++e) {
        const float d = a[it][e] / na - b[it][e] / nb;
        s += w[it][e] * (d * d);
      }
    total += (double)lr_wave_sum(s);      // the butterfly leaves the same bits on every lane
  }
  if (lane == 0) red[wave] = total;
  __syncthreads();
  if (threadIdx.x == 0) slots[(size_t)n * gridDim.x + blockIdx.x] = ((red[0] + red[1]) + red[2]) + red[3];
}

struct lp_finish {
  int slots[LP_STAGES];      // workgroups per sample of each stage's head launch
  int pixels[LP_STAGES];
};

// one wave per sample: a stage's slots l, l + 64, ... on lane l, the lanes in a butterfly, the stages in turn
__global__ __launch_bounds__(64) void lpips_finish_kernel(const double* __restrict__ slots, const lp_finish f, int N, float* __restrict__ out) {
  const int n = blockIdx.x, lane = threadIdx.x;
  double total = 0.0;
  size_t base = 0;
#pragma unroll
  for (int k = 0; k < LP_STAGES; ++k) {
    double t = 0.0;
    for (int i = lane; i < f.slots[k]; i += 64) t += slots[base + (size_t)n * f.slots[k] + i];
    total += lp_wave_sum(t) / (double)f.pixels[k];
    base += (size_t)N * f.slots[k];
  }
  if (lane == 0) out[n] = (float)total;
}

// ---- host side: stage geometry, workspace layout, argument checks, the 13 launches ----
static const int LP_CIN[LP_STAGES] = {3, 64, 192, 384, 256};
static const int LP_COUT[LP_STAGES] = {64, 192, 384, 256, 256};
static const int LP_KS[LP_STAGES] = {11, 5, 3, 3, 3};

struct lp_plan {
  int Ho, Wo;
  int h[LP_STAGES], w[LP_STAGES];      // stage outputs
  int hp[2], wp[2];                    // the pooled maps in front of conv 2 and conv 3
  int64_t act[LP_STAGES], pool[2], slots, total;      // byte offsets into the workspace
  lp_finish fin;
};

static inline int64_t lp_align(int64_t v) { return (v + 255) & ~(int64_t)255; }

static int lp_make_plan(int N, int H, int Wc, int r, lp_plan* p) {
  if (N <= 0 || N > 32767 || H <= 0 || Wc <= 0 || r < 1 || r > LR_EVAL_MAX_R) return LR_E_ARG;
  if (H % r || Wc % r) return LR_E_ARG;
  p->Ho = H / r;
  p->Wo = Wc / r;
  if (p->Ho < LR_LPIPS_MIN_SIDE || p->Wo < LR_LPIPS_MIN_SIDE) return LR_E_ARG;      // a stage would be empty
  p->h[0] = (p->Ho - 7) / 4 + 1;      // 11 x 11, stride 4, pad 2
  p->w[0] = (p->Wo - 7) / 4 + 1;
  p->hp[0] = (p->h[0] - 3) / 2 + 1;
  p->wp[0] = (p->w[0] - 3) / 2 + 1;
  p->h[1] = p->hp[0];
  p->w[1] = p->wp[0];
  p->hp[1] = (p->h[1] - 3) / 2 + 1;
  p->wp[1] = (p->w[1] - 3) / 2 + 1;
  for (int k = 2; k < LP_STAGES; ++k) {
    p->h[k] = p->hp[1];
    p->w[k] = p->wp[1];
  }
  if ((int64_t)2 * N * p->h[0] * p->w[0] > 0x7fffffff - LP_BM) return LR_E_ARG;
  int64_t at = 0;
  for (int k = 0; k < LP_STAGES; ++k) {
    p->act[k] = at;
    at += lp_align((int64_t)2 * N * p->h[k] * p->w[k] * LP_COUT[k] * 2);
  }
  for (int k = 0; k < 2; ++k) {
    p->pool[k] = at;
    at += lp_align((int64_t)2 * N * p->hp[k] * p->wp[k] * LP_COUT[k] * 2);
  }
  p->slots = at;
  int64_t nslots = 0;
  for (int k = 0; k < LP_STAGES; ++k) {
    p->fin.pixels[k] = p->h[k] * p->w[k];
    p->fin.slots[k] = (p->fin.pixels[k] + LP_HEAD_PIX - 1) / LP_HEAD_PIX;
    nslots += (int64_t)N * p->fin.slots[k];
  }
  at += lp_align(nslots * 8);
  p->total = at;
  return 0;
}

extern "C" int64_t lr_lpips_workspace_bytes(int N, int H, int Wc, int r) {
  lp_plan p;
  const int rc = lp_make_plan(N, H, Wc, r, &p);
  return rc ? (int64_t)rc : p.total;
}

extern "C" int lr_lpips_alex(const lr_lpips_args* a, lr_stream_t s) {
  if (!a || !a->pred || !a->origin || !a->workspace || !a->out) return LR_E_ARG;
  if (a->pred_kind < LR_EVAL_PRED_F32 || a->pred_kind > LR_EVAL_PRED_BF16) return LR_E_ARG;
  if (a->W <= 0 || a->x0 < 0 || a->Wc <= 0 || a->x0 > a->W - a->Wc) return LR_E_ARG;
  lp_plan p;
  int rc = lp_make_plan(a->N, a->H, a->Wc, a->r, &p);
  if (rc) return rc;
  if (a->workspace_bytes < p.total) return LR_E_ARG;
  uintptr_t al = (uintptr_t)a->workspace & 255;
  for (int k = 0; k < LP_STAGES; ++k) {
    if (!a->wt[k] || !a->bias[k] || !a->lin[k]) return LR_E_ARG;
    al |= ((uintptr_t)a->wt[k] | (uintptr_t)a->bias[k]) & 15;
  }
  if (al) return LR_E_ALIGN;

  hipStream_t st = (hipStream_t)s;
  char* ws = (char*)a->workspace;
  const int B = 2 * a->N;
  lp_image im = {a->pred, a->origin, a->mask, a->N, a->H, a->W, a->x0, a->r, p.Ho, p.Wo};
  for (int k = 0; k < LP_STAGES; ++k) {
    const f16* in = nullptr;
    int Hin = p.Ho, Win = p.Wo;
    if (k == 1 || k == 2) {      // MaxPool(3, 2) in front of conv 2 and conv 3
      const long long total = (long long)B * p.hp[k - 1] * p.wp[k - 1] * (LP_COUT[k - 1] / 8);
      lpips_pool_kernel<<<(unsigned)((total + LP_THREADS - 1) / LP_THREADS), LP_THREADS, 0, st>>>(
          (const f16*)(ws + p.act[k - 1]), (f16*)(ws + p.pool[k - 1]), B, p.h[k - 1], p.w[k - 1], p.hp[k - 1], p.wp[k - 1], LP_COUT[k - 1]);
      if ((rc = lr_launch_status())) return rc;
      in = (const f16*)(ws + p.pool[k - 1]);
    } else if (k > 2) {
      in = (const f16*)(ws + p.act[k - 1]);
    }
    if (k > 0) {
      Hin = p.h[k];      // every later convolution keeps the size of its input
      Win = p.w[k];
    }
    const int kk = LP_KS[k] * LP_KS[k] * LP_CIN[k];
    lp_conv c = {in, (const f16*)a->wt[k], a->bias[k], (f16*)(ws + p.act[k]), B, Hin, Win, LP_CIN[k], p.h[k], p.w[k], LP_COUT[k],
                 LP_KS[k], k == 0 ? 4 : 1, LP_KS[k] / 2 - (k == 0 ? 3 : 0), (kk + LP_BK - 1) / LP_BK * LP_BK};
    const long long M = (long long)B * p.h[k] * p.w[k];
    const dim3 grid((unsigned)((M + LP_BM - 1) / LP_BM), LP_COUT[k] / LP_BN);
    if (k > 0)
      lpips_conv_kernel<float, false><<<grid, LP_THREADS, 0, st>>>(c, im);
    else if (a->pred_kind == LR_EVAL_PRED_F32)
      lpips_conv_kernel<float, true><<<grid, LP_THREADS, 0, st>>>(c, im);
    else if (a->pred_kind == LR_EVAL_PRED_F16)
      lpips_conv_kernel<f16, true><<<grid, LP_THREADS, 0, st>>>(c, im);
    else
      lpips_conv_kernel<bf16, true><<<grid, LP_THREADS, 0, st>>>(c, im);
    if ((rc = lr_launch_status())) return rc;
  }
  double* slots = (double*)(ws + p.slots);
  size_t base = 0;
  for (int k = 0; k < LP_STAGES; ++k) {
    lpips_head_kernel<<<dim3(p.fin.slots[k], a->N), LP_THREADS, 0, st>>>((const f16*)(ws + p.act[k]), a->lin[k], a->N, p.fin.pixels[k],
                                                                          LP_COUT[k], slots + base);
    if ((rc = lr_launch_status())) return rc;
    base += (size_t)a->N * p.fin.slots[k];
  }
  lpips_finish_kernel<<<a->N, 64, 0, st>>>(slots, p.fin, a->N, a->out);
  return lr_launch_status();
}
