// Pillow's 8-bit resampler and the inpainting canvas of the one-call route on the device (include/leftrefill_hip.h: lr_pil_resize,
// lr_refill_canvas).  Replaces the host image work of the reference's ref_inpainting_gradio.py: `Image.resize(..., BICUBIC)` of source,
// reference (168-169) and result (207), `BILINEAR` of the mask (170), `> 0 -> 255`, `pad_image` (142-145), the [reference | source]
// stitch (184-188), `convert("L")`, the 0.5 threshold, `/ 127.5 - 1` and `image * (mask < 0.5)` of make_batch_sd (54-79).
//
// Arithmetic of leftrefill_amd/refill.py (pil_coeffs, resample_axis, prepare_numpy), which restates Pillow's Resample.c and is pinned
// against Pillow itself.  The host computes, per axis, lo[n_out], cnt[n_out] and the 22-bit fixed-point rows kk[n_out][ksize] in double
// arithmetic; a pass is out[i] = clamp((2^21 + sum_{j < cnt[i]} kk[i][j] in[lo[i] + j]) >> 22, 0, 255) per channel with an arithmetic
// shift.  sum |kk| < 1.4 * 2^22 for both filters, so 255 * sum |kk| + 2^21 < 2^31: 32-bit accumulation.  Everything up to the canvas'
// float mapping is integer arithmetic, so the result equals the numpy statement -- and Pillow -- bit for bit.
//
// Launch 1, horizontal pass: a workgroup owns (job, band of PR_BAND source rows), a thread an output column: it walks the column's
// coefficient row once, each coefficient held in a register across the band's rows (PR_BAND x c accumulators).  Sources are packed at
// any byte offset and a pixel is 3 bytes, so this pass reads bytes.  Launch 2, vertical pass or copy: a workgroup owns (job, band of
// output rows); a row is a flat run of wd c bytes and the coefficient row of an output row is uniform over the workgroup (scalar
// loads), so a thread owns four consecutive bytes -- one dword load per tap, one dword store -- when base and pitch are 4-byte
// aligned, else single bytes.  Launch- and latency-bound like lr_nvs_prep; not tuned.
#include "common.h"

#pragma clang fp contract(off)

#define PR_THREADS 256
#define PR_BAND 8
#define PR_MAX_SIDE (1 << 20)
#define PR_HALF (1 << 21)

__device__ __forceinline__ int pr_clip8(int acc) { return min(max(acc >> 22, 0), 255); }

template <int C>
__device__ __forceinline__ void pr_horizontal(const uint8_t* __restrict__ in, uint8_t* __restrict__ out, const int32_t* __restrict__ tab,
                                              int ws, int wd, int ksize, int y0, int rows) {
  const int32_t *lo = tab, *cnt = tab + wd, *kk = tab + 2 * (int64_t)wd;
  const int64_t pitch = (int64_t)ws * C;
  for (int x = threadIdx.x; x < wd; x += PR_THREADS) {
    const int l = lo[x], n = cnt[x];
    const int32_t* k = kk + (int64_t)x * ksize;
    int acc[PR_BAND][C];
#pragma unroll
    for (int r = 0; r < PR_BAND; ++r)
#pragma unroll
      for (int c = 0; c < C; ++c) acc[r][c] = PR_HALF;
    const uint8_t* p = in + (int64_t)y0 * pitch + (int64_t)l * C;
    for (int j = 0; j < n; ++j, p += C) {
      const int kj = k[j];
#pragma unroll
      for (int r = 0; r < PR_BAND; ++r)
        if (r < rows) {
#pragma unroll
          for (int c = 0; c < C; ++c) acc[r][c] += kj * (int)p[r * pitch + c];
        }
    }
#pragma unroll
    for (int r = 0; r < PR_BAND; ++r)
      if (r < rows) {
        uint8_t* o = out + ((int64_t)(y0 + r) * wd + x) * C;
#pragma unroll
        for (int c = 0; c < C; ++c) o[c] = (uint8_t)pr_clip8(acc[r][c]);
      }
  }
}

__global__ __launch_bounds__(PR_THREADS) void pil_horizontal_kernel(const uint8_t* __restrict__ src, const int32_t* __restrict__ tables,
                                                                    uint8_t* __restrict__ work, uint8_t* __restrict__ dst,
                                                                    const lr_pil_job* __restrict__ jobs) {
  const lr_pil_job jb = jobs[blockIdx.y];
  const int y0 = blockIdx.x * PR_BAND;
  if (jb.h_ksize <= 0 || y0 >= jb.hs) return;      // uniform over the workgroup
  const int rows = min(PR_BAND, jb.hs - y0);
  const uint8_t* in = src + jb.src_off;
  uint8_t* out = jb.v_ksize > 0 ? work + jb.tmp_off : dst + jb.dst_off;
  const int32_t* tab = tables + jb.h_off;
  if (jb.c == 3)
    pr_horizontal<3>(in, out, tab, jb.ws, jb.wd, jb.h_ksize, y0, rows);
  else
    pr_horizontal<1>(in, out, tab, jb.ws, jb.wd, jb.h_ksize, y0, rows);
}

// rows y0 .. y0 + rows - 1 of the output; nb bytes per row on both sides.  ksize == 0: the copy.
template <typename U>
__device__ __forceinline__ void pr_vertical(const uint8_t* __restrict__ in, uint8_t* __restrict__ out, const int32_t* __restrict__ tab,
                                            int hd, int nb, int ksize, int y0, int rows) {
  constexpr int B = (int)sizeof(U);
  const int units = nb / B;      // B == 4 only when nb % 4 == 0
  const int32_t *lo = tab, *cnt = tab + hd, *kk = tab + 2 * (int64_t)hd;
  for (int y = y0; y < y0 + rows; ++y) {
    U* row_out = reinterpret_cast<U*>(out + (int64_t)y * nb);
    if (ksize == 0) {
      const U* row_in = reinterpret_cast<const U*>(in + (int64_t)y * nb);
      for (int u = threadIdx.x; u < units; u += PR_THREADS) row_out[u] = row_in[u];
      continue;
    }
    const int l = lo[y], n = cnt[y];
    const int32_t* k = kk + (int64_t)y * ksize;
    for (int u = threadIdx.x; u < units; u += PR_THREADS) {
      int acc[B];
#pragma unroll
      for (int q = 0; q < B; ++q) acc[q] = PR_HALF;
      const U* p = reinterpret_cast<const U*>(in + (int64_t)l * nb) + u;
      for (int j = 0; j < n; ++j, p += units) {
        const int kj = k[j];
        const uint32_t v = (uint32_t)*p;
#pragma unroll
        for (int q = 0; q < B; ++q) acc[q] += kj * (int)((v >> (8 * q)) & 255u);
      }
      uint32_t packed = 0;
#pragma unroll
      for (int q = 0; q < B; ++q) packed |= (uint32_t)pr_clip8(acc[q]) << (8 * q);
      row_out[u] = (U)packed;
    }
  }
}

__global__ __launch_bounds__(PR_THREADS) void pil_vertical_kernel(const uint8_t* __restrict__ src, const int32_t* __restrict__ tables,
                                                                  const uint8_t* __restrict__ work, uint8_t* __restrict__ dst,
                                                                  const lr_pil_job* __restrict__ jobs) {
  const lr_pil_job jb = jobs[blockIdx.y];
  const int y0 = blockIdx.x * PR_BAND;
  if ((jb.h_ksize > 0 && jb.v_ksize <= 0) || y0 >= jb.hd) return;      // launch 1 finished this job; uniform over the workgroup
  const int rows = min(PR_BAND, jb.hd - y0);
  const uint8_t* in = jb.h_ksize > 0 ? work + jb.tmp_off : src + jb.src_off;
  uint8_t* out = dst + jb.dst_off;
  const int32_t* tab = tables + jb.v_off;
  const int nb = jb.wd * jb.c;
  if (((reinterpret_cast<uintptr_t>(in) | reinterpret_cast<uintptr_t>(out) | (uintptr_t)nb) & 3) == 0)
    pr_vertical<uint32_t>(in, out, tab, jb.hd, nb, jb.v_ksize, y0, rows);
  else
    pr_vertical<uint8_t>(in, out, tab, jb.hd, nb, jb.v_ksize, y0, rows);
}

// one pass' table rows, on the host copy: inside the arena, and every row inside the axis
static int pr_check_axis(const int32_t* th, int64_t words, int64_t off, int n_in, int n_out, int ksize) {
  if (ksize > LR_PIL_MAX_KSIZE) return LR_E_UNSUPPORTED;
  if (off < 0 || off > words || (int64_t)n_out * (2 + (int64_t)ksize) > words - off) return LR_E_ARG;
  const int32_t *lo = th + off, *cnt = lo + n_out;
  for (int i = 0; i < n_out; ++i)
    if (lo[i] < 0 || cnt[i] < 0 || cnt[i] > ksize || lo[i] > n_in - cnt[i]) return LR_E_ARG;
  return 0;
}

static bool pr_window(int64_t off, int64_t bytes, int64_t have) { return off >= 0 && off <= have && bytes <= have - off; }

static int pr_check_job(const lr_pil_job& jb, const int32_t* th, int64_t words, int64_t src_bytes, int64_t work_bytes, int64_t dst_bytes) {
  if (jb.c != 1 && jb.c != 3) return LR_E_ARG;
  if (jb.hs <= 0 || jb.ws <= 0 || jb.hd <= 0 || jb.wd <= 0) return LR_E_ARG;
  if (jb.hs > PR_MAX_SIDE || jb.ws > PR_MAX_SIDE || jb.hd > PR_MAX_SIDE || jb.wd > PR_MAX_SIDE) return LR_E_ARG;
  if (jb.h_ksize < 0 || jb.v_ksize < 0) return LR_E_ARG;
  if (jb.h_ksize > LR_PIL_MAX_KSIZE || jb.v_ksize > LR_PIL_MAX_KSIZE) return LR_E_UNSUPPORTED;
  if (jb.h_ksize == 0 && jb.wd != jb.ws) return LR_E_ARG;
  if (jb.v_ksize == 0 && jb.hd != jb.hs) return LR_E_ARG;
  if (!pr_window(jb.src_off, (int64_t)jb.hs * jb.ws * jb.c, src_bytes)) return LR_E_ARG;
  if (!pr_window(jb.dst_off, (int64_t)jb.hd * jb.wd * jb.c, dst_bytes)) return LR_E_ARG;
  if (jb.h_ksize > 0 && jb.v_ksize > 0 && !pr_window(jb.tmp_off, (int64_t)jb.hs * jb.wd * jb.c, work_bytes)) return LR_E_ARG;
  if (jb.h_ksize > 0) {
    const int rc = pr_check_axis(th, words, jb.h_off, jb.ws, jb.wd, jb.h_ksize);
    if (rc) return rc;
  }
  if (jb.v_ksize > 0) {
    const int rc = pr_check_axis(th, words, jb.v_off, jb.hs, jb.hd, jb.v_ksize);
    if (rc) return rc;
  }
  return 0;
}

extern "C" int lr_pil_resize(const uint8_t* src, int64_t src_bytes, const int32_t* tables, const int32_t* tables_host, int64_t table_words,
                             uint8_t* work, int64_t work_bytes, uint8_t* dst, int64_t dst_bytes, const lr_pil_job* jobs,
                             const lr_pil_job* jobs_host, int n_jobs, lr_stream_t s) {
  if (!src || !tables || !tables_host || !work || !dst || !jobs || !jobs_host) return LR_E_ARG;
  if (n_jobs < 1 || n_jobs > 65535 || src_bytes <= 0 || table_words < 0 || work_bytes < 0 || dst_bytes <= 0) return LR_E_ARG;
  if ((((uintptr_t)src) & 15) || (((uintptr_t)tables) & 3) || (((uintptr_t)tables_host) & 3) || (((uintptr_t)jobs) & 7) ||
      (((uintptr_t)jobs_host) & 7))
    return LR_E_ALIGN;
  int bands_h = 0, bands_v = 0;
  for (int i = 0; i < n_jobs; ++i) {
    const lr_pil_job& jb = jobs_host[i];
    const int rc = pr_check_job(jb, tables_host, table_words, src_bytes, work_bytes, dst_bytes);
    if (rc) return rc;
    if (jb.h_ksize > 0) bands_h = max(bands_h, (jb.hs + PR_BAND - 1) / PR_BAND);
    if (jb.h_ksize == 0 || jb.v_ksize > 0) bands_v = max(bands_v, (jb.hd + PR_BAND - 1) / PR_BAND);
  }
  if (bands_h) {
    pil_horizontal_kernel<<<dim3(bands_h, n_jobs), PR_THREADS, 0, (hipStream_t)s>>>(src, tables, work, dst, jobs);
    const int rc = lr_launch_status();
    if (rc) return rc;
  }
  if (bands_v) pil_vertical_kernel<<<dim3(bands_v, n_jobs), PR_THREADS, 0, (hipStream_t)s>>>(src, tables, work, dst, jobs);
  return lr_launch_status();
}

__global__ __launch_bounds__(PR_THREADS) void refill_canvas_kernel(const uint8_t* __restrict__ ref, const uint8_t* __restrict__ src,
                                                                   const uint8_t* __restrict__ mask, int Sh, int Sw, int H, int W, int n,
                                                                   float* __restrict__ image, float* __restrict__ masked,
                                                                   float* __restrict__ mask_out) {
  const int x = blockIdx.x * PR_THREADS + threadIdx.x, y = blockIdx.y, p = blockIdx.z;
  if (x >= 2 * W) return;
  const bool left = x < W;
  const int xs = min(left ? x : x - W, Sw - 1), ys = min(y, Sh - 1);      // the edge pad
  const size_t at = (((size_t)p * Sh + ys) * Sw + xs) * 3;
  const uint8_t* px = (left ? ref : src) + at;
  float m = 0.0f;
  if (!left) {
    const int r = mask[at] > 0 ? 255 : 0, g = mask[at + 1] > 0 ? 255 : 0, b = mask[at + 2] > 0 ? 255 : 0;
    m = ((19595 * r + 38470 * g + 7471 * b + 32768) >> 16) >= 128 ? 1.0f : 0.0f;
  }
  const float keep = m < 0.5f ? 1.0f : 0.0f;
  float f[3];
#pragma unroll
  for (int c = 0; c < 3; ++c) f[c] = (float)px[c] / 127.5f - 1.0f;
  const size_t plane = (size_t)H * 2 * W, cell = (size_t)y * 2 * W + x;
  for (int k = 0; k < n; ++k) {
    const size_t sample = (size_t)p * n + k;
#pragma unroll
    for (int c = 0; c < 3; ++c) {
      image[(sample * 3 + c) * plane + cell] = f[c];
      masked[(sample * 3 + c) * plane + cell] = f[c] * keep;
    }
    mask_out[sample * plane + cell] = m;
  }
}

extern "C" int lr_refill_canvas(const uint8_t* ref, const uint8_t* src, const uint8_t* mask, int P, int Sh, int Sw, int H, int W, int n,
                                float* image, float* masked_image, float* mask_out, lr_stream_t s) {
  if (!ref || !src || !mask || !image || !masked_image || !mask_out) return LR_E_ARG;
  if (P < 1 || P > 65535 || H < 1 || H > 65535 || W < 1 || W > PR_MAX_SIDE || n < 1) return LR_E_ARG;
  if (Sh < 1 || Sw < 1 || Sh > H || Sw > W) return LR_E_ARG;
  const dim3 grid((2 * W + PR_THREADS - 1) / PR_THREADS, H, P);
  refill_canvas_kernel<<<grid, PR_THREADS, 0, (hipStream_t)s>>>(ref, src, mask, Sh, Sw, H, W, n, image, masked_image, mask_out);
  return lr_launch_status();
}
