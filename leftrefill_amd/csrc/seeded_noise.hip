// Seeded sampling noise: standard normals that are a pure function of (the sample's key, what the draw is for, the step, the element).
// leftrefill_amd/noise.py states it in float64 (normal_numpy); this file regenerates it in fp32:
//
//   element i of sample b, g = i >> 2:
//     w0..w3 = philox4x32_10(counter = (g, sub_b, step, stream), key = (seed_b & 0xffffffff, seed_b >> 32))
//     u(w)   = ((w >> 9) + 0.5) 2^-23 = (2 (w >> 9) + 1) 2^-24          in (0, 1), 24 significant bits: exact in fp32
//     pair p in {0, 1}:  r = sqrt(-2 ln u(w[2p])),  z[4g + 2p] = r cos(2 pi u(w[2p+1])),  z[4g + 2p + 1] = r sin(2 pi u(w[2p+1]))
//
// One Philox call per four outputs; a thread owns whole groups of four (grid-stride over B * ceil(per_sample / 4) groups, 64-bit
// indices).  A group that lies wholly inside a 16-byte aligned row leaves as ONE 16-byte store; a row's tail (per_sample % 4) and the
// rows of an unaligned `out + b per_sample` leave as scalar stores of the same four values -- the arithmetic does not know which.
// logf, sqrtf and sincospif are HIP's accurate forms (no __-prefixed intrinsic); the argument of sincospif, 2 u = (2 (w >> 9) + 1) 2^-23,
// is exact, so there is no range reduction error.  Philox is written out here as csrc/lora.hip writes it (that file is not touched).
#include "common.h"
#include <cmath>

#define NOISE_THREADS 256

struct noise_words {
  uint32_t w[4];
};

// 10 rounds of 2 x (v_mul_hi_u32, v_mul_lo_u32); the Weyl key sequence
__device__ __forceinline__ noise_words noise_philox(uint32_t c0, uint32_t c1, uint32_t c2, uint32_t c3, uint32_t k0, uint32_t k1) {
#pragma unroll
  for (int r = 0; r < 10; ++r) {
    const uint32_t hi0 = __umulhi(0xD2511F53u, c0), lo0 = 0xD2511F53u * c0;
    const uint32_t hi1 = __umulhi(0xCD9E8D57u, c2), lo1 = 0xCD9E8D57u * c2;
    c0 = hi1 ^ c1 ^ k0;
    c1 = lo1;
    c2 = hi0 ^ c3 ^ k1;
    c3 = lo0;
    k0 += 0x9E3779B9u;
    k1 += 0xBB67AE85u;
  }
  return noise_words{{c0, c1, c2, c3}};
}

// Box-Muller on one pair of words.  (2 k + 1) < 2^24 converts exactly; the two scalings are by powers of two.
__device__ __forceinline__ void noise_pair(uint32_t wa, uint32_t wb, float& z0, float& z1) {
  const float u1 = (float)(2u * (wa >> 9) + 1u) * 0x1p-24f;
  const float two_u2 = (float)(2u * (wb >> 9) + 1u) * 0x1p-23f;
  const float r = sqrtf(-2.0f * logf(u1));
  float sn, cs;
  sincospif(two_u2, &sn, &cs);
  z0 = r * cs;
  z1 = r * sn;
}

__global__ __launch_bounds__(NOISE_THREADS) void seeded_normal_kernel(const int64_t* __restrict__ keys, long long per_sample,
                                                                       long long groups, long long total, uint32_t stream, uint32_t step,
                                                                       float* __restrict__ out) {
  const long long stride = (long long)gridDim.x * NOISE_THREADS;
  for (long long idx = (long long)blockIdx.x * NOISE_THREADS + threadIdx.x; idx < total; idx += stride) {
    const long long b = idx / groups, g = idx - b * groups;      // g < 2^32 (checked by the launcher)
    const unsigned long long seed = (unsigned long long)keys[2 * b];
    const uint32_t sub = (uint32_t)keys[2 * b + 1];
    const noise_words ph = noise_philox((uint32_t)g, sub, step, stream, (uint32_t)seed, (uint32_t)(seed >> 32));
    float z[4];
    noise_pair(ph.w[0], ph.w[1], z[0], z[1]);
    noise_pair(ph.w[2], ph.w[3], z[2], z[3]);
    float* row = out + b * per_sample;
    const long long i0 = 4 * g;
    if (((reinterpret_cast<uintptr_t>(row) & 15) == 0) && i0 + 4 <= per_sample) {
      *reinterpret_cast<float4*>(row + i0) = make_float4(z[0], z[1], z[2], z[3]);
    } else {
#pragma unroll
      for (int j = 0; j < 4; ++j)
        if (i0 + j < per_sample) row[i0 + j] = z[j];
    }
  }
}

extern "C" int lr_seeded_normal(const int64_t* keys, int B, int64_t per_sample, int32_t stream, int32_t step, float* out, lr_stream_t s) {
  if (!keys || !out || B <= 0 || per_sample <= 0 || per_sample / 4 >= (1LL << 32)) return LR_E_ARG;
  if (reinterpret_cast<uintptr_t>(out) & 3) return LR_E_ALIGN;
  const long long groups = (per_sample + 3) / 4, total = groups * B;
  const long long blocks = (total + NOISE_THREADS - 1) / NOISE_THREADS;
  dim3 grid((unsigned)(blocks < 8192 ? blocks : 8192)), block(NOISE_THREADS);
  hipLaunchKernelGGL(seeded_normal_kernel, grid, block, 0, (hipStream_t)s, keys, (long long)per_sample, groups, total, (uint32_t)stream,
                     (uint32_t)step, out);
  return lr_launch_status();
}
