#!/usr/bin/env python
"""Scoring tail of the evaluation harness at configs[1] shapes (B = 4, 512 x 1024 canvas, right half scored): wall time per batch of

  host   : what tools/run_inpainting.py does without --device_metrics (and did before the kernel existed) -- finite check,
           evalglue.compose_prediction, psnr01, per-image rgb_to_gray01 + ssim_gray (float64 scipy on the CPU), the fp32 read-back and
           uint8 conversion for the PNG;
  device : evalglue.device_metrics(want_rgb8=True) (one lr_eval_metrics call) + the read-back of the [3, B] results and the uint8 image.

PNG encoding and the file write are the same bytes on both routes and are left out.  Both routes run in this process on the same
inputs, alternating; medians of device-synchronised host-clock times after warm-up.  Also: the kernel's own time (device events
around back-to-back calls on preallocated buffers) and the bytes it has to move over that time.

    python tools/bench_eval_metrics.py [--reps 20] [--out profiles/eval_metrics_bench.json]
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

import bench  # noqa: E402  (HwSampler: shader clock / power while the timed loops run)
from leftrefill_amd import _lib, evalglue, ops  # noqa: E402


def host_route(out, mask_nhwc):
    """tools/run_inpainting.py, the scoring lines of its batch loop, up to the uint8 arrays handed to PIL."""
    if not torch.isfinite(out["pred"]).all():
        raise RuntimeError("non-finite prediction")
    pred, origin = evalglue.compose_prediction(out, mask_nhwc, 512, 512)
    psnrs = evalglue.psnr01(pred, origin).tolist()
    ssims = [evalglue.ssim_gray(evalglue.rgb_to_gray01(pred[j]), evalglue.rgb_to_gray01(origin[j])) for j in range(pred.shape[0])]
    p01 = (pred.float().clamp(-1, 1) + 1) / 2
    arrs = [(p01[j].permute(1, 2, 0).cpu().numpy() * 255).astype(np.uint8) for j in range(p01.shape[0])]
    return psnrs, ssims, arrs


def device_route(out, mask_nhwc):
    m = evalglue.device_metrics(out, mask_nhwc, test_size=512, metric_size=512, want_rgb8=True)
    psnrs, ssims, bad = torch.stack([m["psnr"], m["ssim"], m["nonfinite"]]).tolist()
    if sum(bad):
        raise RuntimeError("non-finite prediction")
    return psnrs, ssims, list(m["rgb8"].cpu().numpy())


def wall(fn, *args):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    res = fn(*args)
    torch.cuda.synchronize()
    return time.perf_counter() - t0, res


def kernel_time(pred, origin, mask, x0, want_rgb8, calls=50, rounds=5):
    """ms per lr_eval_metrics call (both launches), device events around `calls` back-to-back calls, median of `rounds`."""
    lib = _lib.load()
    N, _, H, W = pred.shape
    Wc = W - x0
    slots = N * (-(-H // ops.EVAL_TILE_H)) * (-(-Wc // ops.EVAL_TILE_W))
    partials = torch.empty(slots * ops.EVAL_SLOT_FLOATS, device=pred.device)
    res = torch.empty(N, 4, device=pred.device)
    rgb8 = torch.empty(N, H, Wc, 3, device=pred.device, dtype=torch.uint8) if want_rgb8 else None
    st = torch.cuda.current_stream().cuda_stream

    def call():
        _lib.check(lib.lr_eval_metrics(pred.data_ptr(), ops.EVAL_PRED_KIND[pred.dtype], origin.data_ptr(), mask.data_ptr(), N, H, W, x0,
                                       Wc, 1, partials.data_ptr(), res.data_ptr(), 0 if rgb8 is None else rgb8.data_ptr(), st), "eval_metrics")

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
    moved = N * H * Wc * (3 * (pred.element_size() + 4) + 4 + (3 if want_rgb8 else 0))      # pred + origin + mask read, uint8 written
    t = statistics.median(ms)
    return {"ms_per_call": round(t, 5), "bytes_per_call": moved, "gb_per_s": round(moved / t / 1e6, 1), "all_ms": [round(v, 5) for v in ms]}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", type=str, default=os.path.join(ROOT, "profiles", "eval_metrics_bench.json"))
    a = ap.parse_args()
    assert torch.cuda.is_available(), "this benchmark needs the MI355X: a CPU run says nothing about it"
    dev = torch.device("cuda:0")
    B, H, W = 4, 512, 1024
    g = torch.Generator().manual_seed(0)
    image = torch.rand(B, H, W, 3, generator=g) * 2 - 1                                   # the batch contract: NHWC
    mask = torch.zeros(B, H, W, 1)
    mask[:, :, W // 2:] = (torch.rand(B, H // 32, H // 32, 1, generator=g) < 0.5).float().repeat_interleave(32, 1).repeat_interleave(32, 2)
    pred = (image.permute(0, 3, 1, 2) + 0.1 * torch.randn(B, 3, H, W, generator=g)).contiguous()
    # as log_images returns them: pred fp32 NCHW from the VAE decoder, origin_image a permuted view of the NHWC batch
    out = {"pred": pred.to(dev), "origin_image": image.to(dev).permute(0, 3, 1, 2)}
    mask = mask.to(dev)
    for _ in range(a.warmup):
        h_res, d_res = host_route(out, mask), device_route(out, mask)
    agree = {"max_abs_psnr_diff_db": float(np.max(np.abs(np.array(h_res[0]) - np.array(d_res[0])))),
             "max_abs_ssim_diff": float(np.max(np.abs(np.array(h_res[1]) - np.array(d_res[1])))),
             "png_bytes_equal": all(np.array_equal(x, y) for x, y in zip(h_res[2], d_res[2]))}
    hw = bench.HwSampler(dev).start()
    t_host, t_dev = [], []
    for _ in range(a.reps):                      # alternating: clock / host-load drift hits both routes alike
        t_host.append(wall(host_route, out, mask)[0])
        t_dev.append(wall(device_route, out, mask)[0])
    origin_c, mask_c = out["origin_image"].contiguous(), mask.permute(0, 3, 1, 2).contiguous()
    kern = {"pred_fp32_rgb8": kernel_time(out["pred"], origin_c, mask_c, W // 2, True),
            "pred_fp16": kernel_time(out["pred"].half(), origin_c, mask_c, W // 2, False)}
    hw_stats = hw.stop()
    ms = lambda ts: {"ms_per_batch": round(1e3 * statistics.median(ts), 4), "ms_per_batch_min": round(1e3 * min(ts), 4),
                     "ms_per_batch_max": round(1e3 * max(ts), 4)}
    doc = {"config": f"configs[1] scoring tail: B={B}, canvas {H}x{W}, right half scored, fp32 prediction from the VAE decoder, "
                     "origin_image an NHWC view, metric_size == test_size",
           "timing": f"median of {a.reps} device-synchronised host-clock times per route after {a.warmup} warm-ups, routes alternating in "
                     "one process; each includes its read-back; PNG encoding excluded on both",
           "gpu": torch.cuda.get_device_name(0), "host_cpus": len(os.sched_getaffinity(0)),
           "host_route": ms(t_host), "device_route": ms(t_dev),
           "host_over_device": round(statistics.median(t_host) / statistics.median(t_dev), 2),
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
