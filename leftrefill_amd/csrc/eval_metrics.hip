// Scoring of a decoded prediction on the device: composite, crop, area down-sampling, squared error, luma, 7x7 SSIM, the finite check
// and the 8-bit image of the evaluation harness in one pass over the prediction (include/leftrefill_hip.h: lr_eval_metrics).
//
// Launch 1: one workgroup per 32 x 64 tile of the scored (cropped, down-sampled) image plus a 3-pixel halo.  Phase A streams the halo
// tile once: fp32 composite p = pred m + origin (1 - m), the r x r area mean of p and of origin, the tile's own squared error, finite
// count and uint8 pixels, and the luma of both images -- CENTRED at 0.5 -- into two fp32 LDS planes (2 x 38 x 70 x 4 B = 21 KB, seven
// workgroups per CU by LDS).  Phase B is the separable 7 x 7 box filter straight out of LDS: a thread owns one column and eight rows,
// forms the five horizontal 7-tap sums (a, b, aa, bb, ab) of each of its 14 halo rows once and keeps the last seven in registers, so
// the vertical sum is 7 register adds.  The box sums and the SSIM quotient are fp64: var = E[x^2] - E[x]^2 on a nearly flat image
// cancels most of an fp32 sum (centring alone leaves 1.3e-5 of SSIM there), the kernel is bound by the 7 MB it reads per 512 x 1024
// sample, and the fp64 vector rate of gfx950 hides ~100 operations per pixel behind that.  Only windows that lie fully inside the
// scored image count (skimage crops (win - 1) / 2 pixels off the border before the mean).
// Every workgroup writes its sums to its own slot; launch 2 adds a sample's slots in a fixed order in fp64.  No atomics anywhere: two
// runs on the same input agree bit for bit.
//
// The composite and the 8-bit conversion must round exactly like the harness' separate torch operations: no fused multiply-add here.
#include "common.h"

#pragma clang fp contract(off)

#define EM_TH LR_EVAL_TILE_H
#define EM_TW LR_EVAL_TILE_W
#define EM_R 3                     // (7 - 1) / 2
#define EM_HH (EM_TH + 2 * EM_R)   // 38 halo rows
#define EM_HW (EM_TW + 2 * EM_R)   // 70 halo columns
#define EM_THREADS 256
#define EM_ROWS (EM_TH / (EM_THREADS / EM_TW))   // 8 output rows per thread
static_assert(EM_TW == 64 && EM_THREADS / EM_TW * EM_ROWS == EM_TH, "phase B: one wave per 8-row band, one lane per column");

__device__ __forceinline__ double em_wave_sum(double v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}

// fp64 -> two floats (value = hi + lo to 48 bits): the partials buffer of the C ABI is float
__device__ __forceinline__ void em_split(double d, float& hi, float& lo) {
  hi = (float)d;
  lo = (float)(d - (double)hi);
}

template <typename T>
__global__ __launch_bounds__(EM_THREADS) void eval_metrics_tile_kernel(
    const T* __restrict__ pred, const float* __restrict__ origin, const float* __restrict__ mask, int H, int W, int x0, int r, int Ho,
    int Wo, float* __restrict__ partials, uint8_t* __restrict__ rgb8) {
  __shared__ float la[EM_HH][EM_HW], lb[EM_HH][EM_HW];
  __shared__ double red[3][EM_THREADS / 64];
  const int tid = threadIdx.x;
  const int n = blockIdx.z;
  const int ty0 = blockIdx.y * EM_TH, tx0 = blockIdx.x * EM_TW;
  const size_t plane = (size_t)H * W;
  const float fr = (float)r;
  double sq = 0.0, nonfinite = 0.0;

  // ---- phase A: halo tile -> luma planes; own pixels -> squared error, finite count, uint8 ----
  for (int idx = tid; idx < EM_HH * EM_HW; idx += EM_THREADS) {
    const int hy = idx / EM_HW, hx = idx - hy * EM_HW;
    const int gy = ty0 + hy - EM_R, gx = tx0 + hx - EM_R;
    float a = 0.f, b = 0.f;
    if (gy >= 0 && gy < Ho && gx >= 0 && gx < Wo) {
      const bool own = hy >= EM_R && hy < EM_R + EM_TH && hx >= EM_R && hx < EM_R + EM_TW;
      float p[3] = {0.f, 0.f, 0.f}, o[3] = {0.f, 0.f, 0.f};
      int bad = 0;
      for (int dy = 0; dy < r; ++dy) {
        const size_t row = (size_t)(gy * r + dy) * W + (size_t)(x0 + gx * r);
        for (int dx = 0; dx < r; ++dx) {
          const float m = mask ? mask[(size_t)n * plane + row + dx] : 1.f;
#pragma unroll
          for (int c = 0; c < 3; ++c) {
            const size_t at = ((size_t)n * 3 + c) * plane + row + dx;
            const float pv = (float)pred[at], ov = origin[at];
            bad += !isfinite(pv);
            p[c] += mask ? pv * m + ov * (1.f - m) : pv;      // row-major fp32 sum, as F.interpolate(mode='area') adds them
            o[c] += ov;
          }
        }
      }
      if (r > 1) {
#pragma unroll
        for (int c = 0; c < 3; ++c) {
          p[c] = p[c] / fr / fr;
          o[c] = o[c] / fr / fr;
        }
      }
      a = 0.2989f * ((p[0] + 1.f) / 2.f) + 0.587f * ((p[1] + 1.f) / 2.f) + 0.114f * ((p[2] + 1.f) / 2.f) - 0.5f;
      b = 0.2989f * ((o[0] + 1.f) / 2.f) + 0.587f * ((o[1] + 1.f) / 2.f) + 0.114f * ((o[2] + 1.f) / 2.f) - 0.5f;
      if (own) {
        nonfinite += (double)bad;
#pragma unroll
        for (int c = 0; c < 3; ++c) {
          const double d = 0.5 * ((double)p[c] - (double)o[c]);      // (p + 1) / 2 - (o + 1) / 2 without the fp32 rounding of the shift
          sq += d * d;
        }
        if (rgb8) {
          uint8_t* px = rgb8 + (((size_t)n * Ho + gy) * Wo + gx) * 3;
#pragma unroll
          for (int c = 0; c < 3; ++c) px[c] = (uint8_t)((fminf(fmaxf(p[c], -1.f), 1.f) + 1.f) / 2.f * 255.f);
        }
      }
    }
    la[hy][hx] = a;      // outside the image: 0, read only by windows that do not count
    lb[hy][hx] = b;
  }
  __syncthreads();

  // ---- phase B: 7 x 7 box sums and SSIM of column `col`, output rows band * 8 .. + 7 ----
  const int col = tid & 63, band = tid >> 6;
  const int gx = tx0 + col;
  const bool col_ok = gx >= EM_R && gx < Wo - EM_R;
  double ss = 0.0;
  double hs[7][5];
#pragma unroll
  for (int i = 0; i < EM_ROWS + 6; ++i) {
    const int hy = band * EM_ROWS + i;
    double s[5] = {0.0, 0.0, 0.0, 0.0, 0.0};
#pragma unroll
    for (int k = 0; k < 7; ++k) {
      const double a = (double)la[hy][col + k], b = (double)lb[hy][col + k];
      s[0] += a;
      s[1] += b;
      s[2] += a * a;
      s[3] += b * b;
      s[4] += a * b;
    }
#pragma unroll
    for (int q = 0; q < 5; ++q) hs[i % 7][q] = s[q];
    if (i >= 6) {
      const int gy = ty0 + band * EM_ROWS + (i - 6);
      if (col_ok && gy >= EM_R && gy < Ho - EM_R) {
        double v[5];
#pragma unroll
        for (int q = 0; q < 5; ++q) v[q] = ((((((hs[(i + 1) % 7][q] + hs[(i + 2) % 7][q]) + hs[(i + 3) % 7][q]) + hs[(i + 4) % 7][q]) +
                                              hs[(i + 5) % 7][q]) + hs[(i + 6) % 7][q]) + hs[i % 7][q]) / 49.0;
        const double cov = 49.0 / 48.0, c1 = (0.01 * 2.0) * (0.01 * 2.0), c2 = (0.03 * 2.0) * (0.03 * 2.0);
        const double ua = v[0] + 0.5, ub = v[1] + 0.5;                  // the means carry the centre back; (co)variances are shift-free
        const double va = cov * (v[2] - v[0] * v[0]), vb = cov * (v[3] - v[1] * v[1]), vab = cov * (v[4] - v[0] * v[1]);
        ss += ((2.0 * ua * ub + c1) * (2.0 * vab + c2)) / ((ua * ua + ub * ub + c1) * (va + vb + c2));
      }
    }
  }

  // ---- the workgroup's sums, fixed order: lanes by butterfly, waves 0..3 in turn ----
  sq = em_wave_sum(sq);
  ss = em_wave_sum(ss);
  nonfinite = em_wave_sum(nonfinite);
  if ((tid & 63) == 0) {
    red[0][tid >> 6] = sq;
    red[1][tid >> 6] = ss;
    red[2][tid >> 6] = nonfinite;
  }
  __syncthreads();
  if (tid == 0) {
    double t[3];
#pragma unroll
    for (int q = 0; q < 3; ++q) t[q] = ((red[q][0] + red[q][1]) + red[q][2]) + red[q][3];
    float4 lo4, hi4;
    em_split(t[0], lo4.x, lo4.y);
    em_split(t[1], lo4.z, lo4.w);
    em_split(t[2], hi4.x, hi4.y);
    hi4.z = hi4.w = 0.f;
    float4* slot = reinterpret_cast<float4*>(partials + (((size_t)n * gridDim.y + blockIdx.y) * gridDim.x + blockIdx.x) * LR_EVAL_SLOT_FLOATS);
    slot[0] = lo4;
    slot[1] = hi4;
  }
}

// Launch 2: one wave per sample.  Lane l adds slots l, l + 64, ... in that order, the 64 lane sums meet in a butterfly: a fixed order.
__global__ __launch_bounds__(64) void eval_metrics_finish_kernel(const float* __restrict__ partials, int slots, int Ho, int Wo,
                                                                 float* __restrict__ out) {
  const int n = blockIdx.x, lane = threadIdx.x;
  double t[3] = {0.0, 0.0, 0.0};
  for (int i = lane; i < slots; i += 64) {
    const float4* slot = reinterpret_cast<const float4*>(partials + ((size_t)n * slots + i) * LR_EVAL_SLOT_FLOATS);
    const float4 lo4 = slot[0], hi4 = slot[1];
    t[0] += (double)lo4.x + (double)lo4.y;
    t[1] += (double)lo4.z + (double)lo4.w;
    t[2] += (double)hi4.x + (double)hi4.y;
  }
#pragma unroll
  for (int q = 0; q < 3; ++q) t[q] = em_wave_sum(t[q]);
  if (lane == 0) {
    const double mse = t[0] / (3.0 * (double)Ho * (double)Wo);
    float4 res;
    res.x = (float)mse;
    res.y = (float)(10.0 * log10(1.0 / mse));      // mse == 0 -> +inf, as psnr01
    res.z = (float)(t[1] / ((double)(Ho - 2 * EM_R) * (double)(Wo - 2 * EM_R)));
    res.w = (float)t[2];
    reinterpret_cast<float4*>(out)[n] = res;
  }
}

extern "C" int lr_eval_metrics(const void* pred, int pred_kind, const float* origin, const float* mask, int N, int H, int W, int x0,
                               int Wc, int r, float* partials, float* out, uint8_t* rgb8, lr_stream_t s) {
  if (!pred || !origin || !partials || !out || N <= 0 || N > 65535 || H <= 0 || W <= 0) return LR_E_ARG;
  if (pred_kind < LR_EVAL_PRED_F32 || pred_kind > LR_EVAL_PRED_BF16) return LR_E_ARG;
  if (r < 1 || r > LR_EVAL_MAX_R || x0 < 0 || Wc <= 0 || x0 > W - Wc) return LR_E_ARG;
  if (H % r || Wc % r) return LR_E_ARG;
  const int Ho = H / r, Wo = Wc / r;
  if (Ho < 2 * EM_R + 1 || Wo < 2 * EM_R + 1) return LR_E_ARG;      // no 7 x 7 window fits
  if ((((uintptr_t)partials) | ((uintptr_t)out)) & 15) return LR_E_ALIGN;
  const dim3 grid((Wo + EM_TW - 1) / EM_TW, (Ho + EM_TH - 1) / EM_TH, N);
  if (grid.y > 65535) return LR_E_ARG;
  hipStream_t st = (hipStream_t)s;
  if (pred_kind == LR_EVAL_PRED_F32)
    eval_metrics_tile_kernel<float><<<grid, EM_THREADS, 0, st>>>((const float*)pred, origin, mask, H, W, x0, r, Ho, Wo, partials, rgb8);
  else if (pred_kind == LR_EVAL_PRED_F16)
    eval_metrics_tile_kernel<f16><<<grid, EM_THREADS, 0, st>>>((const f16*)pred, origin, mask, H, W, x0, r, Ho, Wo, partials, rgb8);
  else
    eval_metrics_tile_kernel<bf16><<<grid, EM_THREADS, 0, st>>>((const bf16*)pred, origin, mask, H, W, x0, r, Ho, Wo, partials, rgb8);
  int rc = lr_launch_status();
  if (rc) return rc;
  eval_metrics_finish_kernel<<<N, 64, 0, st>>>(partials, (int)(grid.x * grid.y), Ho, Wo, out);
  return lr_launch_status();
}
