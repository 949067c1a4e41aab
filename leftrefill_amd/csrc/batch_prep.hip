// Batch assembly on the device: raw decoded uint8 images and masks -> the batch contract (image, masked_image, mask) in one launch
// (include/leftrefill_hip.h: lr_batch_prep).  Arithmetic of dropin/dataloaders/test_dataset.py (resize_area, resize_nearest) and of the
// single-image training dataset: area shrink of the cropped window only, rint to uint8, v / 127.5 - 1; nearest masks, thresholded.
//
// One workgroup owns (tile, band of output rows).  It streams the source rows the band covers ONCE: a row's window (the columns the
// crop needs) goes to LDS with 16-byte loads from the 16-byte-aligned window around it -- the arena packs images tightly, so a row
// starts at any byte -- and every thread forms the horizontal coverage sums of its (column, channel) values from LDS bytes.  When
// shrinking, a source row overlaps at most two output rows, so the vertical pass is two fp64 accumulators per value: the current
// output row and the next one; a finished row is divided by its weight sums, rounded and stored.  Two LDS row buffers, one barrier
// per source row.  The coverage weights are the expressions of `_area_weights` in fp64 (lo = i r, hi = (i + 1) r, r = n_src / n_dst),
// so a weight here is the weight there; the sums are ordered differently, which can only move a value that sits within ~1e-12 of a
// rounding tie.  The kernel is bound by the bytes it reads and the floats it writes; fp64 costs nothing next to that.
#include "common.h"

#pragma clang fp contract(off)

#define BP_THREADS 256
#define BP_VPT ((3 * LR_PREP_MAX_SIZE + BP_THREADS - 1) / BP_THREADS)   // (column, channel) values per thread
static_assert(LR_PREP_ROW_BYTES % 16 == 0, "row buffers are uint4");

// coverage of source cell [s, s + 1) by destination cell i = [i r, (i + 1) r): `max(0.0, min(hi, j + 1) - max(lo, j))`
__device__ __forceinline__ double bp_cov(int i, int s, double r) {
  const double lo = (double)i * r, hi = (double)(i + 1) * r;
  return fmax(0.0, fmin(hi, (double)(s + 1)) - fmax(lo, (double)s));
}

// resize_nearest: source index min(int(dst * (src / size)), src - 1)
__device__ __forceinline__ int bp_nearest(int d, int src, int S) {
  return min((int)((double)d * ((double)src / (double)S)), src - 1);
}

__device__ __forceinline__ bool bp_mask_at(const uint8_t* __restrict__ arena, const lr_prep_job& jb, int S, int i, int j) {
  const int jm = (jb.flags & LR_PREP_FLIP_MASK) ? S - 1 - j : j;
  if (jb.outpaint_col >= 0) return jm >= jb.outpaint_col;
  if (jb.flags & LR_PREP_ZERO_MASK) return false;
  int v = 0;
#pragma unroll
  for (int q = 0; q < 2; ++q)
    if (jb.mask_off[q] >= 0)
      v += arena[jb.mask_off[q] + (int64_t)bp_nearest(i, jb.mask_h[q], S) * jb.mask_w[q] + bp_nearest(jm, jb.mask_w[q], S)];
  return min(v, 255) > 127;
}

__global__ __launch_bounds__(BP_THREADS) void batch_prep_kernel(const uint8_t* __restrict__ arena, const lr_prep_job* __restrict__ jobs,
                                                                int S, int tiles, int band, float* __restrict__ image,
                                                                float* __restrict__ masked, float* __restrict__ mask) {
  __shared__ uint4 rowbuf[2][LR_PREP_ROW_BYTES / 16];
  const lr_prep_job jb = jobs[blockIdx.y];
  if (jb.flags & LR_PREP_HOST) return;      // the host writes this tile
  const int tid = threadIdx.x;
  const int i0 = blockIdx.x * band, i1 = min(S, i0 + band);
  const int nval = 3 * S;
  const double ry = (double)jb.img_h / (double)jb.rh, rx = (double)jb.img_w / (double)jb.rw;
  // the source columns the crop window covers, and the source rows this band covers
  const int xa = (int)floor((double)jb.x0 * rx), xb = min(jb.img_w, (int)ceil((double)(jb.x0 + S) * rx));
  const int win_bytes = (xb - xa) * 3;
  const int s_begin = (int)floor((double)(jb.y0 + i0) * ry), s_end = min(jb.img_h, (int)ceil((double)(jb.y0 + i1) * ry));

  // per value: resized column, its source columns and the sum of their coverage
  int col[BP_VPT], xs0[BP_VPT], xs1[BP_VPT];
  double wx[BP_VPT], a0[BP_VPT], a1[BP_VPT];
#pragma unroll
  for (int k = 0; k < BP_VPT; ++k) {
    const int idx = tid + k * BP_THREADS, j = idx / 3;
    a0[k] = a1[k] = 0.0;
    wx[k] = 1.0;
    col[k] = xs0[k] = xs1[k] = 0;
    if (idx < nval) {
      col[k] = jb.x0 + ((jb.flags & LR_PREP_FLIP_IMAGE) ? S - 1 - j : j);
      xs0[k] = (int)floor((double)col[k] * rx);
      xs1[k] = min(jb.img_w, (int)ceil((double)(col[k] + 1) * rx));
      double w = 0.0;
      for (int x = xs0[k]; x < xs1[k]; ++x) w += bp_cov(col[k], x, rx);
      wx[k] = w;
    }
  }

  // source row s -> rowbuf[b]: the 16-byte-aligned window around its bytes; returns where the row's first byte landed
  auto stage = [&](int s, int b) -> int {
    const int64_t first = jb.img_off + ((int64_t)s * jb.img_w + xa) * 3;
    const int64_t base = first & ~(int64_t)15;
    const int n16 = (int)((first + win_bytes + 15 - base) >> 4);
    const uint4* src = reinterpret_cast<const uint4*>(arena + base);
    for (int q = tid; q < n16; q += BP_THREADS) rowbuf[b][q] = src[q];
    return (int)(first - base);
  };

  auto finish = [&](int i, const double* acc, double wy) {
#pragma unroll
    for (int k = 0; k < BP_VPT; ++k) {
      const int idx = tid + k * BP_THREADS;
      if (idx >= nval) continue;
      const int j = idx / 3, c = idx - 3 * j;
      const double q = fmin(fmax(rint(acc[k] / (wy * wx[k])), 0.0), 255.0);
      const float f = (float)q / 127.5f - 1.0f;
      const bool m = bp_mask_at(arena, jb, S, i, j);
      const size_t px = ((size_t)jb.sample * S + i) * ((size_t)tiles * S) + (size_t)jb.tile * S + j;
      image[px * 3 + c] = f;
      masked[px * 3 + c] = f * (m ? 0.0f : 1.0f);
      if (c == 0) mask[px] = m ? 1.0f : 0.0f;
    }
  };

  int cur = jb.y0 + i0;                 // resized row being accumulated in a0; a1 collects what a shared source row gives cur + 1
  const int end = jb.y0 + i1;
  double wy0 = 0.0, wy1 = 0.0;
  int buf = 0;
  int shift = s_begin < s_end ? stage(s_begin, 0) : 0;
  __syncthreads();
  for (int s = s_begin; s < s_end; ++s) {
    int shift_next = 0;
    if (s + 1 < s_end) shift_next = stage(s + 1, buf ^ 1);
    const uint8_t* row = reinterpret_cast<const uint8_t*>(rowbuf[buf]) + shift;
    const bool done = (double)(cur + 1) * ry <= (double)(s + 1) || s + 1 == s_end;
    const double w0 = bp_cov(cur, s, ry);
    const double w1 = (done && cur + 1 < end) ? bp_cov(cur + 1, s, ry) : 0.0;
#pragma unroll
    for (int k = 0; k < BP_VPT; ++k) {
      if (tid + k * BP_THREADS >= nval) continue;
      const int c = (tid + k * BP_THREADS) % 3;
      double h = 0.0;
      for (int x = xs0[k]; x < xs1[k]; ++x) h += bp_cov(col[k], x, rx) * (double)row[(x - xa) * 3 + c];
      a0[k] += w0 * h;
      a1[k] += w1 * h;
    }
    wy0 += w0;
    wy1 += w1;
    if (done && cur < end) {
      finish(cur - jb.y0, a0, wy0);
#pragma unroll
      for (int k = 0; k < BP_VPT; ++k) {
        a0[k] = a1[k];
        a1[k] = 0.0;
      }
      wy0 = wy1;
      wy1 = 0.0;
      ++cur;
    }
    __syncthreads();
    buf ^= 1;
    shift = shift_next;
  }
}

// what the kernel will index, checked on the host copy of the table before anything is launched
static int bp_check_job(const lr_prep_job& jb, int64_t arena_bytes, int S, int tiles, int B) {
  if (jb.sample < 0 || jb.sample >= B || jb.tile < 0 || jb.tile >= tiles) return LR_E_ARG;
  if (jb.flags & LR_PREP_HOST) return 0;
  if (jb.img_h <= 0 || jb.img_w <= 0 || jb.img_off < 0 || jb.img_off > arena_bytes ||
      (int64_t)jb.img_h * jb.img_w > (arena_bytes - jb.img_off) / 3)
    return LR_E_ARG;
  if (jb.rh < S || jb.rw < S || jb.y0 < 0 || jb.x0 < 0 || jb.y0 > jb.rh - S || jb.x0 > jb.rw - S) return LR_E_ARG;
  if (jb.rh > jb.img_h || jb.rw > jb.img_w) return LR_E_UNSUPPORTED;      // enlarging: the host's job
  const double rx = (double)jb.img_w / (double)jb.rw;
  const int xa = (int)floor((double)jb.x0 * rx), xb = jb.img_w < (int)ceil((double)(jb.x0 + S) * rx) ? jb.img_w : (int)ceil((double)(jb.x0 + S) * rx);
  if ((int64_t)(xb - xa) * 3 + 30 > LR_PREP_ROW_BYTES) return LR_E_UNSUPPORTED;
  if (jb.outpaint_col < 0 && !(jb.flags & LR_PREP_ZERO_MASK) && jb.mask_off[0] < 0) return LR_E_ARG;
  for (int q = 0; q < 2; ++q) {
    if (jb.mask_off[q] < 0) continue;
    if (jb.mask_h[q] <= 0 || jb.mask_w[q] <= 0 || jb.mask_off[q] > arena_bytes ||
        (int64_t)jb.mask_h[q] * jb.mask_w[q] > arena_bytes - jb.mask_off[q])
      return LR_E_ARG;
  }
  return 0;
}

extern "C" int lr_batch_prep(const uint8_t* arena, int64_t arena_bytes, const lr_prep_job* jobs, const lr_prep_job* jobs_host, int n_jobs,
                             int S, int tiles, int B, float* image, float* masked_image, float* mask, lr_stream_t s) {
  if (!arena || !jobs || !jobs_host || !image || !masked_image || !mask) return LR_E_ARG;
  if (n_jobs <= 0 || n_jobs > 65535 || S <= 0 || S > LR_PREP_MAX_SIZE || tiles <= 0 || B <= 0 || arena_bytes <= 0) return LR_E_ARG;
  if ((((uintptr_t)arena) & 15) || (arena_bytes & 15)) return LR_E_ALIGN;      // the aligned row windows stay inside the arena
  for (int i = 0; i < n_jobs; ++i) {
    const int rc = bp_check_job(jobs_host[i], arena_bytes, S, tiles, B);
    if (rc) return rc;
  }
  // bands: enough workgroups to fill the chip, at least two output rows each so that a shared source row is read twice at most
  int band = (int)((int64_t)n_jobs * S / 1024);
  band = band < 2 ? 2 : (band > 8 ? 8 : band);
  const dim3 grid((S + band - 1) / band, n_jobs);
  batch_prep_kernel<<<grid, BP_THREADS, 0, (hipStream_t)s>>>(arena, jobs, S, tiles, band, image, masked_image, mask);
  return lr_launch_status();
}
