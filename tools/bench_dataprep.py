#!/usr/bin/env python
"""Batch assembly from photo-sized sources (synthetic 1200 x 1600 uint8 images, 600 x 800 masks, the training dataset's plans):

  host   : `dataprep.run_plan_numpy` per sample, as `InpaintingDataset(raw=False)` runs it inside a loader worker -- timed per sample
           in this process (1 worker) and through a DataLoader with 8 workers (8 samples in flight); a batch costs batch / workers
           samples.  A sample takes seconds (two dense float64 einsums), so a few samples are timed, not whole batches.
  device : `collate_raw` (pack: host, one process), the two host-to-device copies (arena + job table, page-locked), one
           `lr_batch_prep` launch -- `DevicePrep.__call__` end to end, and its three parts on their own.

Decoding is the same work on both routes and is left out: sources are held in memory.  Routes alternate in one process.  The kernel's
time is device events around back-to-back calls -- "hot" on one arena and one set of outputs (largely served by the 256 MiB Infinity
Cache at these sizes) and "cold" rotating through 768 MB of copies, the figure held against the HBM peak; its bytes are the source rows
and columns the plans cover, the mask sources and the fp32 outputs, counted from the job table.  Host per-batch figures are the
per-sample timings times the batch size (a few samples are timed, not whole batches).  The training step (bench.py's
`--workload train --task refill`, batch 16) is timed in the same process; "fed" rates are DERIVED from the measured pieces: a route feeds min(step rate, what its workers can supply), the device
route's copy and kernel queue in front of the step on the same stream.

    python tools/bench_dataprep.py [--out profiles/dataprep_bench.json]
"""
import argparse
import json
import os
import random
import statistics
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import bench  # noqa: E402  (train_bench: the step the loader feeds; HwSampler)
from leftrefill_amd import _lib, dataprep  # noqa: E402

HBM_PEAK = 8.0e12      # bytes / s, the MI355X specification
L3_ROTATE = 768 << 20  # bytes of distinct buffers the "cold" kernel timing cycles through: three times the 256 MiB Infinity Cache


class Sources(torch.utils.data.Dataset):
    """Decoded sources held in memory, planned like InpaintingDataset(mode='train'): (plan, raw) or the finished sample."""

    def __init__(self, n, size, raw, seed=0):
        rng = np.random.RandomState(seed)
        self.images = [rng.randint(0, 256, (1200, 1600, 3), dtype=np.uint8) for _ in range(min(n, 4))]
        self.masks = [(rng.rand(600, 800) < 0.5).astype(np.uint8) * 255 for _ in range(2)]
        self.n, self.size, self.raw = n, size, raw

    def __len__(self):
        return self.n

    def __getitem__(self, i):
        random.seed(i)
        img = self.images[i % len(self.images)]
        resize = dataprep.plan_resize_train(img.shape[0], img.shape[1], self.size)
        picks = dataprep.plan_mask_train(1, 1)
        raw = [img] + [self.masks[k] for k in range(len(picks))]
        flip, mask_flip = dataprep.plan_flips()
        tile = dataprep.plan_tile(0, flip=flip, masks=range(1, len(raw)), mask_flip=mask_flip, **resize)
        plan = dict(img_size=self.size, tiles=[tile], txt="p")
        return (plan, raw) if self.raw else dataprep.run_plan_numpy(plan, raw)


def host_ms_per_sample(size, workers, samples):
    ds = Sources(samples, size, raw=False)
    if workers == 0:
        t0 = time.perf_counter()
        for i in range(samples):
            ds[i]
        return 1e3 * (time.perf_counter() - t0) / samples
    loader = torch.utils.data.DataLoader(ds, batch_size=1, num_workers=workers, prefetch_factor=1)
    t0 = time.perf_counter()      # includes starting the workers: tens of ms next to seconds per sample
    for _ in loader:
        pass
    return 1e3 * (time.perf_counter() - t0) / samples      # wall time per sample with `workers` samples in flight


def moved_bytes(batch, size):
    read = written = 0
    for job in dataprep.job_table(batch):
        ry, rx = job["img_h"] / job["rh"], job["img_w"] / job["rw"]
        rows = min(int(job["img_h"]), int(np.ceil((job["y0"] + size) * ry))) - int(np.floor(job["y0"] * ry))
        cols = min(int(job["img_w"]), int(np.ceil((job["x0"] + size) * rx))) - int(np.floor(job["x0"] * rx))
        read += rows * cols * 3 + size * size * int((job["mask_off"] >= 0).sum())
        written += size * size * 7 * 4
    return read, written


def device_route(size, batch_size, reps, dev):
    ds = Sources(batch_size, size, raw=True)
    items = [ds[i] for i in range(batch_size)]
    prep = dataprep.DevicePrep(size, 1, dev)
    lib = _lib.load()
    batch = dataprep.collate_raw(items)
    out = prep(batch)
    torch.cuda.synchronize()
    # the kernel's results at this size against the host route on the first sample (ties may differ by one level: counted)
    host = dataprep.run_plan_numpy(*items[0])
    diff = (out["image"][0].cpu().numpy() != host["image"])
    agree = {"mask_equal": bool(np.array_equal(out["mask"][0].cpu().numpy(), host["mask"])), "image_values_differing": int(diff.sum()),
             "max_abs_diff_levels": float(np.abs(out["image"][0].cpu().numpy() - host["image"]).max() * 127.5)}
    # the kernel alone, two ways: "hot" re-runs one arena and one set of outputs, which at these sizes (28 - 220 MB per batch) the 256 MiB
    # Infinity Cache largely serves; "cold" rotates through copies of the arena and of the outputs that add up to L3_ROTATE bytes, so a
    # buffer comes round again only after more than the cache has streamed past -- the figure to hold against the HBM peak
    n_arena = batch["arena"].numel()
    per_set = n_arena + 7 * 4 * batch_size * size * size
    sets = [(prep.arena[:n_arena].clone(), torch.empty_like(prep.image), torch.empty_like(prep.masked_image), torch.empty_like(prep.mask))
            for _ in range(max(2, -(-L3_ROTATE // per_set)))]
    pack, whole, copy, kern, cold = [], [], [], [], []
    st = torch.cuda.current_stream().cuda_stream

    def launch(arena, image, masked, mask):
        _lib.check(lib.lr_batch_prep(arena.data_ptr(), n_arena, prep.jobs.data_ptr(), batch["jobs"].data_ptr(), batch_size, size, 1, batch_size,
                                     image.data_ptr(), masked.data_ptr(), mask.data_ptr(), st), "batch_prep")

    for _ in range(reps):
        t0 = time.perf_counter()
        batch = dataprep.collate_raw(items)
        pack.append(time.perf_counter() - t0)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        prep(batch)
        torch.cuda.synchronize()
        whole.append(time.perf_counter() - t0)
        e = [torch.cuda.Event(enable_timing=True) for _ in range(4)]
        e[0].record()
        for _ in range(5):
            prep.arena[:n_arena].copy_(batch["arena"], non_blocking=True)
            prep.jobs[:batch["jobs"].numel()].copy_(batch["jobs"], non_blocking=True)
        e[1].record()
        for _ in range(20):
            launch(prep.arena, prep.image, prep.masked_image, prep.mask)
        e[2].record()
        for k in range(2 * len(sets)):
            launch(*sets[k % len(sets)])
        e[3].record()
        e[3].synchronize()
        copy.append(e[0].elapsed_time(e[1]) / 5)
        kern.append(e[1].elapsed_time(e[2]) / 20)
        cold.append(e[2].elapsed_time(e[3]) / (2 * len(sets)))
    read, written = moved_bytes(batch, size)
    k_ms, c_ms = statistics.median(kern), statistics.median(cold)
    return {"pack_ms": round(1e3 * statistics.median(pack), 3), "copy_ms": round(statistics.median(copy), 3), "kernel_ms_hot": round(k_ms, 4), "kernel_ms_cold": round(c_ms, 4), "cold_rotation_sets": len(sets),
            "call_ms": round(1e3 * statistics.median(whole), 3), "arena_bytes": batch["arena"].numel(),
            "kernel_bytes_read": read, "kernel_bytes_written": written, "kernel_gb_per_s_hot": round((read + written) / k_ms / 1e6, 1),
            "kernel_gb_per_s_cold": round((read + written) / c_ms / 1e6, 1),
            "kernel_cold_fraction_of_hbm_peak": round((read + written) / (c_ms * 1e-3) / HBM_PEAK, 4), "agrees_with_host": agree,
            "kernel_ms_hot_all": [round(v, 4) for v in kern], "kernel_ms_cold_all": [round(v, 4) for v in cold]}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--host_samples", type=int, default=2, help="samples timed per size on the 1-worker host route")
    ap.add_argument("--no_step", action="store_true", help="skip timing the training step")
    ap.add_argument("--out", type=str, default=os.path.join(ROOT, "profiles", "dataprep_bench.json"))
    a = ap.parse_args()
    assert torch.cuda.is_available(), "this benchmark needs the MI355X: a CPU run says nothing about it"
    dev = torch.device("cuda:0")
    hw = bench.HwSampler(dev).start()
    doc = {"config": "synthetic 1200x1600 sources, 600x800 masks, InpaintingDataset's training plans (both resize branches, flips), "
                     "one tile per sample; decoding excluded on both routes",
           "timing": "host: wall time per sample of run_plan_numpy, in-process (1 worker) and through a DataLoader with 8 workers; device: "
                     f"medians of {a.reps} reps -- collate_raw (pack), device events around 5 arena + table copies, around 20 back-to-back "
                     "lr_batch_prep calls on one buffer set (hot: Infinity Cache) and around calls rotating through 768 MB of buffer sets "
                     "(cold), DevicePrep.__call__ synchronised (call); routes alternate per size; host per-batch = per-sample x batch",
           "gpu": torch.cuda.get_device_name(0), "host_cpus": len(os.sched_getaffinity(0)), "sizes": {}}
    for size in (256, 512):
        entry = {"host_ms_per_sample_1_worker": round(host_ms_per_sample(size, 0, a.host_samples), 1)}
        for b in (16, 4):      # alternating: a device measurement between the host ones
            entry[f"device_batch_{b}"] = device_route(size, b, a.reps, dev)
        entry["host_ms_per_sample_8_workers"] = round(host_ms_per_sample(size, 8, 8), 1)
        for b in (16, 4):
            entry[f"host_ms_per_batch_{b}"] = {"1_worker": round(b * entry["host_ms_per_sample_1_worker"], 1),
                                               "8_workers": round(b * entry["host_ms_per_sample_8_workers"], 1)}
        doc["sizes"][str(size)] = entry
    if not a.no_step:
        args = argparse.Namespace(steps=10, warmup=3, task="refill", dtype="f16", train_graph=False, recompute=False)
        step = bench.train_bench(args, 0, 1, dev)
        step_ms, bt = step["ms_per_step"], 16
        fed = {"step_ms_batch_16": round(step_ms, 3), "step_samples_per_s": round(1e3 * bt / step_ms, 1)}
        for size in ("256", "512"):
            e = doc["sizes"][size]
            d = e["device_batch_16"]
            fed[size] = {
                "host_1_worker": round(min(1e3 * bt / step_ms, 1e3 / e["host_ms_per_sample_1_worker"]), 2),
                "host_8_workers": round(min(1e3 * bt / step_ms, 1e3 / e["host_ms_per_sample_8_workers"]), 2),
                "device_1_packer": round(1e3 * bt / max(step_ms + d["copy_ms"] + d["kernel_ms_cold"], d["pack_ms"]), 1),
                "device_8_packers": round(1e3 * bt / max(step_ms + d["copy_ms"] + d["kernel_ms_cold"], d["pack_ms"] / 8), 1)}
        fed["note"] = ("derived, samples/s: min(step rate, supply rate); the device route adds its copy and kernel to the step and is "
                       "supplied by collate_raw in 1 or 8 workers; decoding, which both routes need, is not counted")
        doc["training_step_fed"] = fed
    hw_stats = hw.stop()
    doc.update({"sclk_mhz_mean": hw_stats.get("sclk_mhz_mean"), "power_w_mean": hw_stats.get("power_w_mean")})
    print(json.dumps(doc))
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(doc, f, indent=1)
        f.write("\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
