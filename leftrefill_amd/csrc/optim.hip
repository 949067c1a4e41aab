// The optimizer tail of a mixed-precision training step on the device (include/leftrefill_hip.h: lr_amp_adamw_step): gradient
// unscale + non-finite scan, the loss-scale update of torch.amp.GradScaler and the AdamW update of torch.optim.AdamW over a table of
// tensors, with no host read-back -- the skip decision never leaves the device, so the whole training step is capturable.
//
// Three launches, whatever the number of tensors:
//   1. scan:   every workgroup walks every tensor of the table grid-strided, sums (g / scale)^2 and counts non-finite values, and
//              writes its two sums to its own slot.
//   2. decide: one wave adds the slots in a fixed order, takes the skip decision, advances the scaler and the three counters, and
//              leaves this step's constants (1 / scale, step size and decay of every group) in the state block.
//   3. apply:  the same walk as the scan; returns at once when the step is skipped, so parameters and moments keep their bits.
// Nothing is accumulated with atomics: a thread adds its own elements in index order, lanes meet in a butterfly, waves and workgroups
// are added in index order -- two runs on the same input agree bit for bit.
//
// The update restates torch's single-tensor AdamW one rounding at a time (mul by 1 - lr wd; lerp; mul + addcmul; sqrt / sqrt(bc2) + eps;
// addcdiv), so contraction into fused multiply-adds is switched off.  The bias corrections are formed in fp64 like torch's Python
// floats and rounded to fp32 once.
#include "common.h"

#pragma clang fp contract(off)

#define OPT_THREADS 256

struct opt_step_consts {      // written by the decide kernel behind the public words of the state block
  float step_size;            // lr / (1 - beta1^t)
  float decay;                // 1 - lr * weight_decay
  float bc2_sqrt;             // sqrt(1 - beta2^t)
  float lr;
};
static_assert(sizeof(opt_step_consts) == 16 && LR_OPT_STATE_WORDS * 4 == 64 + LR_OPT_MAX_GROUPS * 16, "state block layout");

__device__ __forceinline__ float opt_load(const void* g, int kind, int64_t i) {
  if (kind == LR_OPT_GRAD_F32) return ((const float*)g)[i];
  if (kind == LR_OPT_GRAD_F16) return (float)((const f16*)g)[i];
  return (float)((const bf16*)g)[i];
}

__global__ __launch_bounds__(OPT_THREADS) void amp_scan_kernel(const lr_optim_tensor* __restrict__ tensors, int n_tensors,
                                                               const int* __restrict__ state, float* __restrict__ partials) {
  __shared__ double red[2][OPT_THREADS / 64];
  const float inv_scale = (float)(1.0 / (double)__int_as_float(state[LR_OPT_SCALE]));
  const int64_t stride = (int64_t)gridDim.x * OPT_THREADS;
  double sq = 0.0, bad = 0.0;
  for (int t = 0; t < n_tensors; ++t) {
    const lr_optim_tensor d = tensors[t];
    for (int64_t i = (int64_t)blockIdx.x * OPT_THREADS + threadIdx.x; i < d.numel; i += stride) {
      const float raw = opt_load(d.grad, d.grad_kind, i);      // the finite check is on the scaled value, as torch's unscale_
      const float g = raw * inv_scale;
      if (isfinite(raw)) sq += (double)g * (double)g;
      else bad += 1.0;
    }
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    sq += __shfl_xor(sq, o, 64);
    bad += __shfl_xor(bad, o, 64);
  }
  if ((threadIdx.x & 63) == 0) {
    red[0][threadIdx.x >> 6] = sq;
    red[1][threadIdx.x >> 6] = bad;
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    const double s = ((red[0][0] + red[0][1]) + red[0][2]) + red[0][3];
    const double b = ((red[1][0] + red[1][1]) + red[1][2]) + red[1][3];
    const float hi = (float)s;
    float4 slot = {hi, (float)(s - (double)hi), (float)b, 0.f};
    reinterpret_cast<float4*>(partials)[blockIdx.x] = slot;
  }
}

__global__ __launch_bounds__(64) void amp_decide_kernel(const float* __restrict__ partials, int slots,
                                                        const lr_optim_group* __restrict__ groups, int n_groups, int* __restrict__ state,
                                                        float growth, float backoff, int growth_interval) {
  const int lane = threadIdx.x;
  double sq = 0.0, bad = 0.0;
  for (int i = lane; i < slots; i += 64) {
    const float4 s = reinterpret_cast<const float4*>(partials)[i];
    sq += (double)s.x + (double)s.y;
    bad += (double)s.z;
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    sq += __shfl_xor(sq, o, 64);
    bad += __shfl_xor(bad, o, 64);
  }
  const int found = bad > 0.0;
  const float scale = __int_as_float(state[LR_OPT_SCALE]);
  const int sched = state[LR_OPT_SCHED_STEPS];
  const int applied = state[LR_OPT_APPLIED_STEPS] + (found ? 0 : 1);
  // this step's constants of group `lane`: the lr index advances every call, the bias-correction step only when the update is applied
  if (lane < n_groups) {
    const lr_optim_group g = groups[lane];
    const int at = sched < g.lr_len ? sched : g.lr_len - 1;      // past the end of the table: its last value
    const float lr = g.lr_len > 0 ? g.lr_table[at] : 0.f;
    const double bc1 = 1.0 - pow(g.beta1, (double)applied), bc2 = 1.0 - pow(g.beta2, (double)applied);
    opt_step_consts c;
    c.step_size = (float)((double)lr / bc1);
    c.decay = (float)(1.0 - (double)lr * g.weight_decay);
    c.bc2_sqrt = (float)sqrt(bc2);
    c.lr = lr;
    reinterpret_cast<opt_step_consts*>(state + LR_OPT_CONSTS)[lane] = c;
  }
  if (lane == 0) {
    // torch.amp.GradScaler.update (_amp_update_scale_): back off on a non-finite gradient, else count towards the next growth
    float new_scale = scale;
    int tracker = state[LR_OPT_GROWTH_TRACKER];
    if (growth_interval > 0) {
      if (found) {
        new_scale = scale * backoff;
        tracker = 0;
      } else if (++tracker == growth_interval) {
        const float grown = scale * growth;
        if (isfinite(grown)) new_scale = grown;
        tracker = 0;
      }
    }
    state[LR_OPT_SCALE] = __float_as_int(new_scale);
    state[LR_OPT_GROWTH_TRACKER] = tracker;
    state[LR_OPT_FOUND_INF] = found;
    state[LR_OPT_APPLIED_STEPS] = applied;
    state[LR_OPT_SCHED_STEPS] = sched + 1;
    state[LR_OPT_SKIPPED] += found;
    state[LR_OPT_GRAD_NORM] = __float_as_int((float)sqrt(sq));      // of the finite unscaled values
    state[LR_OPT_INV_SCALE] = __float_as_int((float)(1.0 / (double)scale));
    state[LR_OPT_LR_INDEX] = sched;
  }
}

__global__ __launch_bounds__(OPT_THREADS) void amp_apply_kernel(const lr_optim_tensor* __restrict__ tensors, int n_tensors,
                                                                const lr_optim_group* __restrict__ groups, int n_groups,
                                                                const int* __restrict__ state) {
  if (state[LR_OPT_FOUND_INF]) return;
  const float inv_scale = __int_as_float(state[LR_OPT_INV_SCALE]);
  const int64_t stride = (int64_t)gridDim.x * OPT_THREADS;
  for (int t = 0; t < n_tensors; ++t) {
    const lr_optim_tensor d = tensors[t];
    if (d.group < 0 || d.group >= n_groups) continue;
    const lr_optim_group g = groups[d.group];
    const opt_step_consts c = reinterpret_cast<const opt_step_consts*>(state + LR_OPT_CONSTS)[d.group];
    const float w1 = (float)(1.0 - g.beta1), w2 = (float)(1.0 - g.beta2), beta2 = (float)g.beta2, eps = (float)g.eps;
    for (int64_t i = (int64_t)blockIdx.x * OPT_THREADS + threadIdx.x; i < d.numel; i += stride) {
      const float grad = opt_load(d.grad, d.grad_kind, i) * inv_scale;
      float p = d.param[i], m = d.exp_avg[i], v = d.exp_avg_sq[i];
      p = p * c.decay;
      m = m + w1 * (grad - m);
      v = v * beta2 + (w2 * grad) * grad;
      const float denom = sqrtf(v) / c.bc2_sqrt + eps;
      p = p + (-c.step_size * m) / denom;
      d.param[i] = p;
      d.exp_avg[i] = m;
      d.exp_avg_sq[i] = v;
    }
  }
}

extern "C" int lr_amp_adamw_step(const lr_optim_tensor* tensors, int n_tensors, const lr_optim_group* groups, int n_groups, void* state,
                                 float* partials, int blocks, float growth_factor, float backoff_factor, int growth_interval,
                                 int* launches, lr_stream_t s) {
  if (!tensors || !groups || !state || !partials || n_tensors <= 0 || n_groups <= 0 || n_groups > LR_OPT_MAX_GROUPS) return LR_E_ARG;
  if (blocks <= 0 || blocks > LR_OPT_MAX_BLOCKS || growth_interval < 0) return LR_E_ARG;
  if (growth_interval > 0 && !(growth_factor > 1.f && backoff_factor > 0.f && backoff_factor < 1.f)) return LR_E_ARG;
  if ((((uintptr_t)partials) | ((uintptr_t)state) | ((uintptr_t)tensors) | ((uintptr_t)groups)) & 15) return LR_E_ALIGN;
  hipStream_t st = (hipStream_t)s;
  int* st_words = (int*)state;
  amp_scan_kernel<<<blocks, OPT_THREADS, 0, st>>>(tensors, n_tensors, st_words, partials);
  int rc = lr_launch_status();
  if (rc) return rc;
  if (launches) ++*launches;
  amp_decide_kernel<<<1, 64, 0, st>>>(partials, blocks, groups, n_groups, st_words, growth_factor, backoff_factor, growth_interval);
  rc = lr_launch_status();
  if (rc) return rc;
  if (launches) ++*launches;
  amp_apply_kernel<<<blocks, OPT_THREADS, 0, st>>>(tensors, n_tensors, groups, n_groups, st_words);
  rc = lr_launch_status();
  if (rc) return rc;
  if (launches) ++*launches;
  return 0;
}
