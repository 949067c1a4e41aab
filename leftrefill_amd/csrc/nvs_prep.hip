// Novel-view-synthesis batch assembly on the device: raw RGBA renders -> the batch contract (image, masked_image, mask) of the
// [cond | target] canvas in one launch (include/leftrefill_hip.h: lr_nvs_prep).  Arithmetic of leftrefill_amd/nvsprep.py: composite on
// white, the 8-bit resize (copy, 2 x 2 box, or 11-bit fixed-point bilinear), v / 127.5 - 1; the mask from the target render's own alpha
// -- area-tap occupancy, elliptic dilation -- OR-ed with a stroke plane, or all ones, or a grey file plane.  Everything up to the final
// float mapping is integer arithmetic, so the result equals the numpy statement bit for bit.
//
// One workgroup owns (sample, tile, band of NV_BAND output rows).  A thread forms whole output pixels: a render is RGBA at a
// 16-byte-aligned offset, so a pixel is one 4-byte load and the two pixels a 2 x 2 box needs from a row one 8-byte load.  For the
// target tile of an alpha job the workgroup first builds the occupancy of its rows plus the element's halo (k / 2 rows above,
// k - 1 - k / 2 below, clipped) as bit-rows in LDS: a wave takes 64 consecutive columns and one __ballot gives their word.  The
// dilation of pixel (i, j) is then, per element row e, "any bit of row i + e - r in columns [j + lo[e] - c, j + hi[e] - 1 - c]":
// the span is at most 32 columns, so one or two masked words.  The spans come from the job record; no square root here.
#include "common.h"

#pragma clang fp contract(off)

#define NV_THREADS 256
#define NV_BAND 8
#define NV_WORDS ((LR_NVS_MAX_SIZE + 63) / 64)
#define NV_ROWS (NV_BAND + LR_NVS_MAX_DILATE - 1)

struct nv_axis { int s0, s1, a0, a1; };

// the fixed-point bilinear's taps and coefficients of destination index d on an axis of n source cells
__device__ __forceinline__ nv_axis nv_linear(int d, int n, int S) {
  const double scale = (double)n / (double)S;
  float f = (float)(((double)d + 0.5) * scale - 0.5);
  int s = (int)floorf(f);
  f -= (float)s;
  if (s < 0) { s = 0; f = 0.0f; }
  if (s >= n - 1) { s = n - 1; f = 0.0f; }
  nv_axis a;
  a.s0 = s;
  a.s1 = min(s + 1, n - 1);
  a.a0 = (int)rintf((1.0f - f) * 2048.0f);
  a.a1 = (int)rintf(f * 2048.0f);
  return a;
}

// first and last source cell of the INTER_AREA tap set of destination index d (a run; the sliver threshold is OpenCV's)
__device__ __forceinline__ void nv_area(int d, int n, int S, int& first, int& last) {
  const double scale = (double)n / (double)S;
  const double f1 = (double)d * scale, f2 = f1 + scale;
  int s1 = (int)ceil(f1);
  const int s2 = min((int)floor(f2), n - 1);
  s1 = min(s1, s2);
  first = max(((double)s1 - f1 > 1e-3) ? s1 - 1 : s1, 0);
  last = min((f2 - (double)s2 > 1e-3) ? s2 : s2 - 1, n - 1);
}

__device__ __forceinline__ uint32_t nv_white(uint32_t px) { return (px >> 24) == 0 ? 0x00ffffffu : px; }
__device__ __forceinline__ int nv_ch(uint32_t px, int c) { return (int)((px >> (8 * c)) & 255u); }

// any bit of the row in columns [a, b], 0 <= a <= b < S, b - a < 64
__device__ __forceinline__ bool nv_any(const unsigned long long* row, int a, int b) {
  const int wa = a >> 6, wb = b >> 6;
  const unsigned long long ma = ~0ull << (a & 63), mb = ~0ull >> (63 - (b & 63));
  if (wa == wb) return (row[wa] & ma & mb) != 0ull;
  return ((row[wa] & ma) | (row[wb] & mb)) != 0ull;
}

__global__ __launch_bounds__(NV_THREADS) void nvs_prep_kernel(const uint8_t* __restrict__ arena, const lr_nvs_job* __restrict__ jobs, int S,
                                                              float* __restrict__ image, float* __restrict__ masked,
                                                              float* __restrict__ mask) {
  __shared__ unsigned long long occ[NV_ROWS * NV_WORDS];
  const lr_nvs_job* jp = jobs + blockIdx.z;
  const int tile = blockIdx.y, tid = threadIdx.x;
  const int i0 = blockIdx.x * NV_BAND, i1 = min(S, i0 + NV_BAND);
  const int h = tile ? jp->target_h : jp->cond_h, w = tile ? jp->target_w : jp->cond_w;
  const int64_t off = tile ? jp->target_off : jp->cond_off;
  const int mode = jp->mode, k = jp->k, r = k / 2, sample = jp->sample;
  const bool ref_white = (jp->flags & LR_NVS_REF_WHITE) != 0;
  const int64_t plane_off = jp->plane_off;
  const int words = (S + 63) >> 6;
  const bool dilating = tile == 1 && mode == LR_NVS_MODE_ALPHA;      // uniform over the workgroup
  int y_lo = 0;

  if (dilating) {
    y_lo = max(0, i0 - r);
    const int y_hi = min(S - 1, i1 - 1 + (k - 1 - r));
    const int nrows = y_hi - y_lo + 1;      // <= NV_ROWS
    const int wave = tid >> 6, lane = tid & 63;
    for (int q = wave; q < nrows * words; q += NV_THREADS / 64) {      // bounds uniform over the wave: every lane votes
      const int y = y_lo + q / words, wq = q % words, j = wq * 64 + lane;
      bool o = false;
      if (j < S) {
        int ra, rb, ca, cb;
        nv_area(y, h, S, ra, rb);
        nv_area(j, w, S, ca, cb);
        for (int sy = ra; sy <= rb && !o; ++sy) {
          const uint8_t* a = arena + off + ((int64_t)sy * w + ca) * 4 + 3;
          for (int sx = ca; sx <= cb; ++sx, a += 4)
            if (*a) { o = true; break; }
        }
      }
      const unsigned long long word = __ballot(o);
      if (lane == 0) occ[(y - y_lo) * NV_WORDS + wq] = word;
    }
    __syncthreads();
  }

  const int path = (h == S && w == S) ? 0 : ((h == 2 * S && w == 2 * S) ? 1 : 2);
  const uint32_t* src = reinterpret_cast<const uint32_t*>(arena + off);
  for (int i = i0; i < i1; ++i) {
    const nv_axis ay = nv_linear(i, h, S);
    for (int j = tid; j < S; j += NV_THREADS) {
      int v[3];
      if (path == 0) {
        const uint32_t p = nv_white(src[(int64_t)i * w + j]);
#pragma unroll
        for (int c = 0; c < 3; ++c) v[c] = nv_ch(p, c);
      } else if (path == 1) {      // rows 2 i and 2 i + 1, columns 2 j and 2 j + 1: 8-byte aligned pairs
        const uint2 t = *reinterpret_cast<const uint2*>(src + (int64_t)(2 * i) * w + 2 * j);
        const uint2 b = *reinterpret_cast<const uint2*>(src + (int64_t)(2 * i + 1) * w + 2 * j);
        const uint32_t p00 = nv_white(t.x), p01 = nv_white(t.y), p10 = nv_white(b.x), p11 = nv_white(b.y);
#pragma unroll
        for (int c = 0; c < 3; ++c) v[c] = (nv_ch(p00, c) + nv_ch(p01, c) + nv_ch(p10, c) + nv_ch(p11, c) + 2) >> 2;
      } else {
        const nv_axis ax = nv_linear(j, w, S);
        const uint32_t p00 = nv_white(src[(int64_t)ay.s0 * w + ax.s0]), p01 = nv_white(src[(int64_t)ay.s0 * w + ax.s1]);
        const uint32_t p10 = nv_white(src[(int64_t)ay.s1 * w + ax.s0]), p11 = nv_white(src[(int64_t)ay.s1 * w + ax.s1]);
#pragma unroll
        for (int c = 0; c < 3; ++c) {
          const int r0 = nv_ch(p00, c) * ax.a0 + nv_ch(p01, c) * ax.a1, r1 = nv_ch(p10, c) * ax.a0 + nv_ch(p11, c) * ax.a1;
          v[c] = (((ay.a0 * (r0 >> 4)) >> 16) + ((ay.a1 * (r1 >> 4)) >> 16) + 2) >> 2;
        }
      }

      float m = 0.0f;
      if (tile == 1) {
        if (mode == LR_NVS_MODE_ONES) {
          m = 1.0f;
        } else if (mode == LR_NVS_MODE_FILE) {
          m = (float)((double)arena[plane_off + (int64_t)i * S + j] / 255.0);
        } else {
          bool bit = plane_off >= 0 && arena[plane_off + (int64_t)i * S + j] > 0;
          for (int e = 0; e < k && !bit; ++e) {
            const int y = i + e - r;
            if (y < 0 || y >= S) continue;
            const int a = max(j + (int)jp->lo[e] - r, 0), b = min(j + (int)jp->hi[e] - 1 - r, S - 1);
            if (a <= b) bit = nv_any(occ + (y - y_lo) * NV_WORDS, a, b);
          }
          m = bit ? 1.0f : 0.0f;
        }
      }
      const float keep = m < 0.5f ? 1.0f : 0.0f;
      const size_t px = ((size_t)sample * S + i) * ((size_t)2 * S) + (size_t)tile * S + j;
#pragma unroll
      for (int c = 0; c < 3; ++c) {
        const float f = (float)v[c] / 127.5f - 1.0f;
        image[px * 3 + c] = f;
        masked[px * 3 + c] = ((tile == 1 && ref_white) ? 1.0f : f) * keep;
      }
      mask[px] = m;
    }
  }
}

// what the kernel will index, checked on the host copy of the table before anything is launched
static int nv_check_render(int64_t off, int h, int w, int64_t arena_bytes, int S) {
  if (off < 0 || h <= 0 || w <= 0) return LR_E_ARG;
  if (off & 15) return LR_E_ALIGN;
  if (off > arena_bytes || (int64_t)h * w > (arena_bytes - off) / 4) return LR_E_ARG;
  if (h < S || w < S) return LR_E_UNSUPPORTED;      // enlarging: another filter
  return 0;
}

static int nv_check_job(const lr_nvs_job& jb, int64_t arena_bytes, int S, int B) {
  if (jb.sample < 0 || jb.sample >= B) return LR_E_ARG;
  if (jb.mode != LR_NVS_MODE_ALPHA && jb.mode != LR_NVS_MODE_ONES && jb.mode != LR_NVS_MODE_FILE) return LR_E_ARG;
  int rc = nv_check_render(jb.cond_off, jb.cond_h, jb.cond_w, arena_bytes, S);
  if (rc) return rc;
  rc = nv_check_render(jb.target_off, jb.target_h, jb.target_w, arena_bytes, S);
  if (rc) return rc;
  if (jb.plane_off >= 0) {
    if (jb.plane_off & 15) return LR_E_ALIGN;
    if (jb.plane_off > arena_bytes || (int64_t)S * S > arena_bytes - jb.plane_off) return LR_E_ARG;
  } else if (jb.mode == LR_NVS_MODE_FILE) {
    return LR_E_ARG;
  }
  if (jb.mode == LR_NVS_MODE_ALPHA) {
    if (jb.k < 1) return LR_E_ARG;
    if (jb.k > LR_NVS_MAX_DILATE) return LR_E_UNSUPPORTED;
    for (int e = 0; e < jb.k; ++e)
      if (jb.lo[e] >= jb.hi[e] || jb.hi[e] > jb.k) return LR_E_ARG;
  }
  return 0;
}

extern "C" int lr_nvs_prep(const uint8_t* arena, int64_t arena_bytes, const lr_nvs_job* jobs, const lr_nvs_job* jobs_host, int B, int S,
                           float* image, float* masked_image, float* mask, lr_stream_t s) {
  if (!arena || !jobs || !jobs_host || !image || !masked_image || !mask) return LR_E_ARG;
  if (B <= 0 || B > 65535 || S <= 0 || arena_bytes <= 0) return LR_E_ARG;
  if (S > LR_NVS_MAX_SIZE) return LR_E_UNSUPPORTED;
  if ((((uintptr_t)arena) & 15) || (arena_bytes & 15)) return LR_E_ALIGN;
  for (int i = 0; i < B; ++i) {
    const int rc = nv_check_job(jobs_host[i], arena_bytes, S, B);
    if (rc) return rc;
  }
  const dim3 grid((S + NV_BAND - 1) / NV_BAND, 2, B);
  nvs_prep_kernel<<<grid, NV_THREADS, 0, (hipStream_t)s>>>(arena, jobs, S, image, masked_image, mask);
  return lr_launch_status();
}
