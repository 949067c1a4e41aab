#!/usr/bin/env python
"""LPIPS tail of the evaluation harness at the configs[1] scoring shape (N = 4, 512 x 1024 canvas, right half scored, fp16 prediction):
wall time per batch of

  eager  : what tools/run_inpainting.py does without --device_lpips -- evalglue.compose_prediction (composite, crop) on the device, then
           the eager fp32 `LPIPSAlex` one sample at a time with its `float()` read-back per sample, as validation_result calls it;
  device : one `DeviceLPIPS.score` call (lr_lpips_alex: 13 launches, the composite formed in the first convolution) + one read-back.

Both routes run in this process on the same inputs and the same seeded weights (no pretrained weights ship), alternating; medians of
device-synchronised host-clock times after warm-up; the mean shader clock over the timed loops is recorded.  Also: the time of the
lr_lpips_alex call alone (device events around back-to-back calls on a preallocated workspace), the TFLOP/s that is of the 58 GFLOP
the five convolutions need at this shape, and a per-kernel split from the torch profiler.

    python tools/bench_lpips.py [--reps 20] [--out profiles/lpips_bench.json]
"""
import argparse
import ctypes
import json
import os
import statistics
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import bench  # noqa: E402  (HwSampler: shader clock / power while the timed loops run)
from leftrefill_amd import _lib, evalglue, ops  # noqa: E402


def seeded_state_dict(seed=0):
    """The weights of tests/test_lpips_cpu.py: conv N(0, 2 / fan_in), bias 0.1 N(0, 1), lin U(0, 4 / C)."""
    g = torch.Generator().manual_seed(seed)
    sd = {}
    for i, ((ci, co, k, _, _), fi) in enumerate(zip(evalglue.LPIPSAlex.CONVS, evalglue.LPIPSAlex.FEATURE_INDEX)):
        sd[f"features.{fi}.weight"] = torch.randn(co, ci, k, k, generator=g) * (2.0 / (ci * k * k)) ** 0.5
        sd[f"features.{fi}.bias"] = 0.1 * torch.randn(co, generator=g)
        sd[f"lin{i}.model.1.weight"] = torch.rand(1, co, 1, 1, generator=g) * (4.0 / co)
    return sd


def conv_flops(n_images, Ho, Wo):
    return sum(2 * n_images * h * w * co * ci * k * k for (h, w), (ci, co, k, _, _) in zip(ops.lpips_stage_sizes(Ho, Wo), ops.LPIPS_CONVS))


def eager_route(fn, out, mask_nhwc):
    pred, origin = evalglue.compose_prediction(out, mask_nhwc, 512, 512)
    return [float(fn(pred[i:i + 1].float(), origin[i:i + 1].float())) for i in range(pred.shape[0])]


def device_route(fn, out, mask_nhwc):
    return fn.score(out, mask_nhwc, test_size=512, metric_size=512).tolist()


def wall(fn, *args):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    res = fn(*args)
    torch.cuda.synchronize()
    return time.perf_counter() - t0, res


def kernel_time(fn, pred, origin, mask, x0, calls=20, rounds=5):
    """ms per lr_lpips_alex call (all 13 launches), device events around `calls` back-to-back calls, median of `rounds`."""
    lib = _lib.load()
    packed = fn.packed()
    N, _, H, W = pred.shape
    Wc = W - x0
    need = lib.lr_lpips_workspace_bytes(N, H, Wc, 1)
    ws = torch.empty(need, device=pred.device, dtype=torch.uint8)
    res = torch.empty(N, device=pred.device)
    a = _lib.LpipsArgs()
    a.pred, a.pred_kind, a.origin, a.mask = pred.data_ptr(), ops.EVAL_PRED_KIND[pred.dtype], origin.data_ptr(), mask.data_ptr()
    a.N, a.H, a.W, a.x0, a.Wc, a.r = N, H, W, x0, Wc, 1
    for k in range(5):
        a.wt[k], a.bias[k], a.lin[k] = packed["wt"][k].data_ptr(), packed["bias"][k].data_ptr(), packed["lin"][k].data_ptr()
    a.workspace, a.workspace_bytes, a.out = ws.data_ptr(), need, res.data_ptr()
    st = torch.cuda.current_stream().cuda_stream
    call = lambda: _lib.check(lib.lr_lpips_alex(ctypes.byref(a), st), "lpips_alex")
    for _ in range(5):
        call()
    ms = []
    for _ in range(rounds):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(calls):
            call()
        e1.record()
        e1.synchronize()
        ms.append(e0.elapsed_time(e1) / calls)
    t = statistics.median(ms)
    flops = conv_flops(2 * N, H, Wc)
    doc = {"ms_per_call": round(t, 5), "launches_per_call": ops.LPIPS_LAUNCHES, "conv_gflop_per_call": round(flops / 1e9, 2),
           "tflops": round(flops / t / 1e9, 2), "workspace_mib": round(need / 2 ** 20, 1), "all_ms": [round(v, 5) for v in ms]}
    try:      # per-kernel split, device time summed over the 13 launches of ten calls
        from torch.profiler import ProfilerActivity, profile
        with profile(activities=[ProfilerActivity.CUDA]) as prof:
            for _ in range(10):
                call()
            torch.cuda.synchronize()
        split = {}
        for ev in prof.key_averages():
            dev_us = getattr(ev, "device_time_total", None) or getattr(ev, "cuda_time_total", 0)
            if "lpips_" in ev.key and dev_us:
                split[ev.key[:96]] = {"launches_per_call": ev.count / 10, "us_per_call": round(dev_us / 10, 2)}
        doc["per_kernel"] = split
    except Exception as e:      # the profiler is a convenience here, not the measurement
        doc["per_kernel"] = f"profiler unavailable: {e}"
    return doc


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", type=str, default=os.path.join(ROOT, "profiles", "lpips_bench.json"))
    a = ap.parse_args()
    assert torch.cuda.is_available(), "this benchmark needs the MI355X: a CPU run says nothing about it"
    dev = torch.device("cuda:0")
    B, H, W = 4, 512, 1024
    g = torch.Generator().manual_seed(0)
    image = torch.rand(B, H, W, 3, generator=g) * 2 - 1                                   # the batch contract: NHWC
    mask = torch.zeros(B, H, W, 1)
    mask[:, :, W // 2:] = (torch.rand(B, H // 32, H // 32, 1, generator=g) < 0.5).float().repeat_interleave(32, 1).repeat_interleave(32, 2)
    pred = (image.permute(0, 3, 1, 2) + 0.1 * torch.randn(B, 3, H, W, generator=g)).clamp(-1, 1).half().contiguous()
    out = {"pred": pred.to(dev), "origin_image": image.to(dev).permute(0, 3, 1, 2)}
    mask = mask.to(dev)
    sd = seeded_state_dict()
    eager_fn = evalglue.LPIPSAlex().load_weights(sd).to(dev)
    device_fn = evalglue.DeviceLPIPS().load_weights(sd).to(dev)
    for _ in range(a.warmup):
        e_res, d_res = eager_route(eager_fn, out, mask), device_route(device_fn, out, mask)
    agree = {"eager": e_res, "device": d_res, "max_abs_diff": max(abs(x - y) for x, y in zip(e_res, d_res))}
    hw = bench.HwSampler(dev).start()
    t_eager, t_dev = [], []
    for _ in range(a.reps):                      # alternating: clock / host-load drift hits both routes alike
        t_eager.append(wall(eager_route, eager_fn, out, mask)[0])
        t_dev.append(wall(device_route, device_fn, out, mask)[0])
    kern = kernel_time(device_fn, out["pred"], out["origin_image"].contiguous(), mask.permute(0, 3, 1, 2).contiguous(), W // 2)
    hw_stats = hw.stop()
    ms = lambda ts: {"ms_per_batch": round(1e3 * statistics.median(ts), 4), "ms_per_batch_min": round(1e3 * min(ts), 4),
                     "ms_per_batch_max": round(1e3 * max(ts), 4)}
    doc = {"config": f"configs[1] LPIPS tail: N={B}, canvas {H}x{W}, right half scored, fp16 prediction, origin_image an NHWC view, "
                     "metric_size == test_size; seeded weights (none ship)",
           "timing": f"median of {a.reps} device-synchronised host-clock times per route after {a.warmup} warm-ups, routes alternating in "
                     "one process; each includes its read-back(s)",
           "gpu": torch.cuda.get_device_name(0), "host_cpus": len(os.sched_getaffinity(0)),
           "eager_route": ms(t_eager), "device_route": ms(t_dev),
           "eager_over_device": round(statistics.median(t_eager) / statistics.median(t_dev), 2),
           "routes_agree": agree, "kernel": kern,
           "sclk_mhz_mean": hw_stats.get("sclk_mhz_mean"), "power_w_mean": hw_stats.get("power_w_mean"),
           "hw_sampler": hw_stats.get("hw_sampler")}
    print(json.dumps(doc))
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(doc, f, indent=1)
        f.write("\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
