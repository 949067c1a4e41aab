#!/usr/bin/env python
"""The training image logger's tail at configs[4] logging shapes (N = 4 images of 3 x 256 x 512; `masked_image` and `origin_image` as
NHWC views, `pred` NCHW fp32; T = 73 prompt tokens x 1024): wall time per logging call of

  host   : the reference's route (inpainting_ldm/logger.py) -- every logged tensor to the host as fp32, clamp, make_grid per key,
           rescale, transposes, concatenation, 8-bit conversion (leftrefill_amd.imagelog.grid_numpy after `.float().cpu().numpy()`),
           and per token `sqrt(sum(d**2)).item()` with the re-clone of the snapshot;
  device : InpaintingLogger's device route -- one lr_image_grid launch into a persistent uint8 canvas and its one read-back, one
           lr_token_drift launch, nothing else read back.

JPEG encoding and the file write are the same bytes on both routes and are left out.  Both routes run in this process on the same
inputs, alternating; medians of device-synchronised host-clock times after warm-up.  Also: the two kernels alone (device events around
back-to-back calls on preallocated buffers) with the bytes they have to move, and one training step of `bench.py --workload train` timed
in the same process for scale.  Nothing is asserted about the times.

    python tools/bench_image_log.py [--reps 20] [--out profiles/image_log_bench.json]
"""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import bench  # noqa: E402  (train_bench: the step the logger runs between; HwSampler)
from leftrefill_amd import imagelog, ops  # noqa: E402

N, H, W, T, D = 4, 256, 512, 73, 1024


def host_route(images, old, weight):
    """reference logger.py:88-98 + 43-67 up to the array handed to PIL, and 118-123."""
    canvas = imagelog.grid_numpy({k: v[:N].detach().float().cpu().numpy() for k, v in images.items()}, max_images=N)
    drift = [torch.sqrt(torch.sum((old[j] - weight[j]) ** 2)).item() for j in range(T)]
    return canvas, drift, weight.clone()


def wall(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    res = fn()
    torch.cuda.synchronize()
    return time.perf_counter() - t0, res


def event_ms(call, calls=50, rounds=5):
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
    return statistics.median(ms), [round(v, 5) for v in ms]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--no_train_step", action="store_true", help="skip the training step timed for scale")
    ap.add_argument("--out", type=str, default=os.path.join(ROOT, "profiles", "image_log_bench.json"))
    a = ap.parse_args()
    assert torch.cuda.is_available(), "this benchmark needs the MI355X: a CPU run says nothing about it"
    dev = torch.device("cuda:0")
    import leftrefill_amd.dropin as dropin
    dropin.install()
    from inpainting_ldm.logger import InpaintingLogger
    g = torch.Generator().manual_seed(0)
    image = (torch.rand(N, H, W, 3, generator=g) * 2 - 1).to(dev)                      # the batch contract: NHWC
    masked = image * (torch.rand(N, H, W, 1, generator=g) < 0.5).to(dev)
    pred = (image.permute(0, 3, 1, 2) + 0.1 * torch.randn(N, 3, H, W, generator=g).to(dev)).contiguous()
    images = {"masked_image": masked.permute(0, 3, 1, 2), "origin_image": image.permute(0, 3, 1, 2), "pred": pred}
    weight = 0.02 * torch.randn(T, D, generator=g).to(dev)
    old = [(weight + 1e-3 * torch.randn(T, D, generator=g).to(dev)).contiguous() for _ in range(2)]      # one snapshot per route
    logger = InpaintingLogger(max_images=N)
    logger.special_tokens, logger.special_token_embeddings_old = [f"<t{j}>" for j in range(T)], old[1]
    sink = type("Sink", (), {"log": lambda self, name, value, **kw: None})()

    def device_route():
        canvas = logger.canvas(images)
        logger._log_drift(sink, weight)
        return canvas

    for _ in range(a.warmup):
        h_res, d_res = host_route(images, old[0], weight), device_route()
    agree = {"canvas_bytes_equal": bool(np.array_equal(h_res[0], d_res)), "canvas_shape": list(d_res.shape)}
    hw = bench.HwSampler(dev).start()
    t_host, t_dev = [], []
    for _ in range(a.reps):                      # alternating: clock / host-load drift hits both routes alike
        t_host.append(wall(lambda: host_route(images, old[0], weight))[0])
        t_dev.append(wall(device_route)[0])
    sources = imagelog.sources_of(images, max_images=N)
    canvas = torch.empty(*d_res.shape, device=dev, dtype=torch.uint8)
    drift = torch.empty(T, device=dev)
    grid_ms, grid_all = event_ms(lambda: ops.image_grid(sources, N, H, out=canvas))
    drift_ms, drift_all = event_ms(lambda: ops.token_drift(old[1], weight, out=drift))
    grid_bytes = 3 * N * 3 * H * W * 4 + canvas.numel()            # three fp32 sources read, the canvas written
    drift_bytes = 3 * T * D * 4 + 4 * T                            # old and new read, old written, out written
    hw_stats = hw.stop()
    step = None
    if not a.no_train_step:
        args = argparse.Namespace(steps=10, warmup=3, task="refill", dtype="f16", train_graph=False, recompute=False)
        step = bench.train_bench(args, 0, 1, dev)
    ms = lambda ts: {"ms_per_call": round(1e3 * statistics.median(ts), 4), "ms_per_call_min": round(1e3 * min(ts), 4),
                     "ms_per_call_max": round(1e3 * max(ts), 4)}
    doc = {"config": f"configs[4] logging shapes: N={N} images of 3x{H}x{W}, keys masked_image / origin_image (NHWC views) and pred (NCHW "
                     f"fp32), canvas {list(d_res.shape)}; token drift of {T} x {D} fp32",
           "timing": f"median of {a.reps} device-synchronised host-clock times per route after {a.warmup} warm-ups, routes alternating in "
                     "one process; each includes its read-back; JPEG encoding excluded on both; launches go through the Python wrappers",
           "gpu": torch.cuda.get_device_name(0), "host_cpus": len(os.sched_getaffinity(0)),
           "host_route": ms(t_host), "device_route": ms(t_dev),
           "host_over_device": round(statistics.median(t_host) / statistics.median(t_dev), 2),
           "routes_agree": agree,
           "kernel": {"image_grid": {"ms_per_call": round(grid_ms, 5), "bytes_per_call": grid_bytes, "gb_per_s": round(grid_bytes / grid_ms / 1e6, 1),
                                     "all_ms": grid_all},
                      "token_drift": {"ms_per_call": round(drift_ms, 5), "bytes_per_call": drift_bytes,
                                      "gb_per_s": round(drift_bytes / drift_ms / 1e6, 1), "all_ms": drift_all},
                      "note": "device events around 50 back-to-back calls through the Python wrappers, median of 5 rounds: at these sizes the "
                              "figure is launch-rate bound, not a bandwidth measurement"},
           "train_step_for_scale": None if step is None else {"ms_per_step": round(step["ms_per_step"], 3), "workload": step["config"]["workload"]},
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
