#!/usr/bin/env python
"""FID tail of the evaluation harness at the configs[1] scoring shape (N = 4, 512 x 1024 canvas, right half scored, fp16 prediction):
wall time per batch of

  host   : `fid.HostFID.update` -- torch composite, crop and 8-bit mapping, F.interpolate to 299 x 299, the eager fp32 `FIDInception` on
           the 2N images on the device, the features read back and added to float64 sums in numpy;
  device : `fid.DeviceFID.update` -- two lr_fid_input launches (the composite and the 8-bit mapping inside them), lr_fid_run over
           FID_PROGRAM on the 2N images, lr_fid_head, two lr_fid_accumulate launches; nothing read back.

Both routes run in this process on the same inputs and the same seeded weights (no pretrained weights ship), alternating; medians of
device-synchronised host-clock times after warm-up; the mean shader clock over the timed loops is recorded.  Also: the time of the
network alone (lr_fid_run + lr_fid_head on a filled arena, device events around back-to-back calls), its launch count as the library
counts it, the TFLOP/s that is of the convolutions' FLOPs, and one `compute()` per route.  No threshold is asserted anywhere.

    python tools/bench_fid.py [--reps 10] [--out profiles/fid_bench.json]
"""
import argparse
import json
import os
import statistics
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import bench  # noqa: E402  (HwSampler: shader clock / power while the timed loops run)
from leftrefill_amd import fid, ops  # noqa: E402


def conv_flops(n_images):
    """FLOPs of the 94 convolutions on their real channel counts (the padding of the stored layout is not counted)."""
    P = fid.FID_PROGRAM[fid.FID_PROGRAM[:, fid.W_OP] == fid.OP_CONV]
    return n_images * sum(2 * int(r[fid.W_HOUT]) * int(r[fid.W_WOUT]) * o["cin"] * o["cout"] * o["kh"] * o["kw"] for r, o in zip(P, fid.CONVS))


def wall(fn, *args):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    res = fn(*args)
    torch.cuda.synchronize()
    return time.perf_counter() - t0, res


def network_time(packed, B, dev, calls=5, rounds=5):
    """ms per pass of the network alone on B images: lr_fid_run over FID_PROGRAM + lr_fid_head, device events around `calls` passes."""
    L = fid.FID_LAYOUT
    arena = torch.zeros(B * L["arena_halfs"], device=dev, dtype=torch.float16)
    u8 = torch.randint(0, 256, (B, 512, 512, 3), device=dev, dtype=torch.uint8, generator=torch.Generator(device=dev).manual_seed(0))
    at = L["input_off"] * B
    ops.fid_input(u8, arena[at:at + B * fid.SIZE * fid.SIZE * 4], fid.SIZE)
    feats = torch.empty(B, L["output_c"], device=dev)

    def call():
        ops.fid_run(fid.FID_PROGRAM, B, arena, packed["wt"], packed["bias"])
        ops.fid_head(arena[L["output_off"] * B:], B, L["output_hw"], L["output_c"], L["output_c"], feats)

    before = ops.FID_LAUNCHES.value
    call()
    launches = ops.FID_LAUNCHES.value - before
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
    flops = conv_flops(B)
    doc = {"images": B, "ms_per_pass": round(t, 4), "launches_per_pass": launches, "conv_gflop_per_pass": round(flops / 1e9, 2),
           "tflops": round(flops / t / 1e9, 2), "arena_mib": round(arena.numel() * 2 / 2 ** 20, 1), "all_ms": [round(v, 4) for v in ms]}
    try:      # per-kernel split, device time summed over the launches of three passes
        from torch.profiler import ProfilerActivity, profile
        with profile(activities=[ProfilerActivity.CUDA]) as prof:
            for _ in range(3):
                call()
            torch.cuda.synchronize()
        split = {}
        for ev in prof.key_averages():
            dev_us = getattr(ev, "device_time_total", None) or getattr(ev, "cuda_time_total", 0)
            if "fid_" in ev.key and dev_us:
                split[ev.key[:96]] = {"launches_per_pass": ev.count / 3, "us_per_pass": round(dev_us / 3, 2)}
        doc["per_kernel"] = split
    except Exception as e:      # the profiler is a convenience here, not the measurement
        doc["per_kernel"] = f"profiler unavailable: {e}"
    return doc


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--out", type=str, default=os.path.join(ROOT, "profiles", "fid_bench.json"))
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
    sd = fid.seeded_state_dict(0)
    host_fn, device_fn = fid.HostFID().load_weights(sd).to(dev), fid.DeviceFID().load_weights(sd).to(dev)
    for _ in range(a.warmup):
        host_fn.update(out, mask)
        device_fn.update(out, mask)
    hw = bench.HwSampler(dev).start()
    t_host, t_dev = [], []
    for _ in range(a.reps):                      # alternating: clock / host-load drift hits both routes alike
        t_host.append(wall(host_fn.update, out, mask)[0])
        t_dev.append(wall(device_fn.update, out, mask)[0])
    t_compute = {"host_ms": round(1e3 * wall(host_fn.compute)[0], 1), "device_ms": round(1e3 * wall(device_fn.compute)[0], 1)}
    net = network_time(device_fn.packed(), 2 * B, dev)
    hw_stats = hw.stop()
    mu_h, mu_d = host_fn.pred_stats.sums()[0], device_fn.pred_stats.sums()[0]
    ms = lambda ts: {"ms_per_batch": round(1e3 * statistics.median(ts), 4), "ms_per_batch_min": round(1e3 * min(ts), 4),
                     "ms_per_batch_max": round(1e3 * max(ts), 4)}
    doc = {"config": f"configs[1] FID tail: N={B}, canvas {H}x{W}, right half scored, fp16 prediction, origin_image an NHWC view; "
                     f"{2 * B} images of 299 x 299 per batch; seeded weights (none ship)",
           "timing": f"median of {a.reps} device-synchronised host-clock times per route after {a.warmup} warm-ups, routes alternating in "
                     "one process; the host route includes its read-back of the features, the device route reads nothing back",
           "gpu": torch.cuda.get_device_name(0), "host_cpus": len(os.sched_getaffinity(0)),
           "host_route": ms(t_host), "device_route": ms(t_dev),
           "host_over_device": round(statistics.median(t_host) / statistics.median(t_dev), 2),
           "feature_sum_rel_l2_between_routes": float(((mu_h - mu_d) ** 2).sum() ** 0.5 / (mu_h ** 2).sum() ** 0.5),
           "compute_once_per_evaluation": t_compute, "network": net,
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
