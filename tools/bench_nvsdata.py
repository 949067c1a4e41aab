#!/usr/bin/env python
"""Objaverse NVS batch assembly at the training shape (batch 16 of synthetic 512 x 512 RGBA renders, S = 256: the 2 x 2 box, dilation
sizes 10-25, stroke planes; the plans of `NVS_OBJDataset`'s training branch with the shipped data section):

  host   : `nvsprep.run_nvs_plan_numpy` per sample in this process, and wall time per sample through a DataLoader with 8 workers.
  device : `collate_nvs_raw` (pack: host, one process), the arena + job-table copies between device events, `NVSDevicePrep.__call__`
           synchronised (copies + the one lr_nvs_prep launch), and the launch alone -- re-run on one arena (hot: the bytes fit the
           Infinity Cache) and rotating through more than 256 MiB of distinct arenas and outputs (cold).

Decoding and planning (the stroke plane's PIL drawing included) are the same work on both routes and are left out: renders and
planes are held in memory.  The routes alternate in one process, `--rounds` times.  The training step (bench.py's `--workload train`,
task nvs) is timed in the same process unless --no_step.

    python tools/bench_nvsdata.py [--out profiles/nvsdata_bench.json]
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

import bench  # noqa: E402  (train_bench: the step the loader feeds)
from leftrefill_amd import _lib, nvsprep  # noqa: E402

SIDE, SIZE, BATCH, SETS = 512, 256, 16, 6


class Renders(torch.utils.data.Dataset):
    """Renders held in memory: item i is (plan, raw) or the finished item, an object of about a third of the frame, k = 10 + i % 16."""

    def __init__(self, n, raw, seed=0):
        rng = np.random.RandomState(seed)
        self.n, self.raw, self.views, self.planes = n, raw, [], []
        yy, xx = np.mgrid[:SIDE, :SIDE]
        for v in range(4):
            rgba = rng.randint(0, 256, (SIDE, SIDE, 4), dtype=np.uint8)
            cy, cx = rng.randint(180, 330, size=2)
            rgba[:, :, 3] *= ((yy - cy) ** 2 + (xx - cx) ** 2 < 150 ** 2).astype(np.uint8)
            self.views.append(rgba)
            plane = np.zeros((SIZE, SIZE), np.uint8)
            plane[rng.randint(0, 200):, rng.randint(0, 200):][:40, :120] = 1
            self.planes.append(plane)

    def __len__(self):
        return self.n

    def __getitem__(self, i):
        plan = dict(img_size=SIZE, mode="alpha", k=10 + i % 16, plane=2, ref_white=False, rel_pose=[0.1, 0.2, 0.3, 0.4], txt="p")
        raw = [self.views[i % 4], self.views[(i + 1) % 4], self.planes[i % 4]]
        return (plan, raw) if self.raw else nvsprep.run_nvs_plan_numpy(plan, raw)


def through_workers(n, workers):
    loader = torch.utils.data.DataLoader(Renders(n, raw=False), batch_size=1, num_workers=workers, prefetch_factor=1)
    t0 = time.perf_counter()      # includes starting the workers
    for _ in loader:
        pass
    return 1e3 * (time.perf_counter() - t0) / n


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=3, help="host samples / device repetitions, alternating this often")
    ap.add_argument("--reps", type=int, default=5, help="device repetitions per round")
    ap.add_argument("--no_step", action="store_true", help="skip timing the training step")
    ap.add_argument("--out", type=str, default=os.path.join(ROOT, "profiles", "nvsdata_bench.json"))
    a = ap.parse_args()
    assert torch.cuda.is_available(), "this benchmark needs the MI355X: a CPU run says nothing about it"
    dev = torch.device("cuda:0")
    lib = _lib.load()
    ds = Renders(BATCH, raw=True)
    items = [ds[i] for i in range(BATCH)]
    prep = nvsprep.NVSDevicePrep(SIZE, dev)
    out = prep(nvsprep.collate_nvs_raw(items))      # warm-up: buffers, module load
    torch.cuda.synchronize()
    first = nvsprep.run_nvs_plan_numpy(*items[0])
    agree = all(out[k][0].cpu().numpy().tobytes() == first[k].tobytes() for k in ("image", "masked_image", "mask"))
    st = torch.cuda.current_stream().cuda_stream
    batch = nvsprep.collate_nvs_raw(items)
    n_bytes = batch["arena"].numel()
    sets = [(torch.empty(n_bytes, dtype=torch.uint8, device=dev).copy_(batch["arena"]), torch.empty(BATCH, SIZE, 2 * SIZE, 3, device=dev),
             torch.empty(BATCH, SIZE, 2 * SIZE, 3, device=dev), torch.empty(BATCH, SIZE, 2 * SIZE, 1, device=dev)) for _ in range(SETS)]
    set_bytes = n_bytes + 7 * 4 * BATCH * SIZE * 2 * SIZE
    assert SETS * set_bytes > 256 * 2 ** 20, "the rotation must exceed the Infinity Cache"

    def launch(arena, image, masked, mask):
        _lib.check(lib.lr_nvs_prep(arena.data_ptr(), n_bytes, prep.jobs.data_ptr(), batch["jobs"].data_ptr(), BATCH, SIZE, image.data_ptr(),
                                   masked.data_ptr(), mask.data_ptr(), st), "nvs_prep")

    def events(fn, n):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for i in range(n):
            fn(i)
        e1.record()
        e1.synchronize()
        return e0.elapsed_time(e1) / n

    host, workers, pack, copy, call, hot, cold = [], [], [], [], [], [], []
    for r in range(a.rounds):
        for i in range(2):
            t0 = time.perf_counter()
            nvsprep.run_nvs_plan_numpy(*items[(2 * r + i) % BATCH])
            host.append(1e3 * (time.perf_counter() - t0))
        workers.append(through_workers(2 * BATCH, 8))
        for _ in range(a.reps):
            t0 = time.perf_counter()
            batch = nvsprep.collate_nvs_raw(items)
            pack.append(1e3 * (time.perf_counter() - t0))
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            prep(batch)
            torch.cuda.synchronize()
            call.append(1e3 * (time.perf_counter() - t0))
            copy.append(events(lambda i: (prep.arena[:n_bytes].copy_(batch["arena"], non_blocking=True),
                                          prep.jobs[:batch["jobs"].numel()].copy_(batch["jobs"], non_blocking=True)), 5))
            hot.append(events(lambda i: launch(*sets[0]), 20))
            cold.append(events(lambda i: launch(*sets[i % SETS]), 4 * SETS))
    med = statistics.median
    doc = {"config": f"batch {BATCH}, synthetic {SIDE}x{SIDE} RGBA renders, S = {SIZE} (2 x 2 box), alpha mode with k = 10 .. 25 and a stroke "
                     "plane; decoding and planning excluded on both routes",
           "timing": f"one process, {a.rounds} rounds of two host samples, one 8-worker pass over {2 * BATCH} samples, then {a.reps} device "
                     "repetitions; medians; copy / kernel: device events around 5 copies, 20 launches on one buffer set (hot: Infinity "
                     f"Cache) and {4 * SETS} launches rotating through {SETS} buffer sets of {set_bytes / 2 ** 20:.0f} MiB (cold)",
           "gpu": torch.cuda.get_device_name(0), "host_cpus": len(os.sched_getaffinity(0)),
           "host_ms_per_sample": round(med(host), 2), "host_ms_per_sample_all": [round(v, 2) for v in host],
           "host_ms_per_sample_8_workers": round(med(workers), 2), "host_ms_per_sample_8_workers_all": [round(v, 2) for v in workers],
           "device_pack_ms": round(med(pack), 3), "device_copy_ms": round(med(copy), 3), "device_call_ms": round(med(call), 3),
           "device_call_ms_all": [round(v, 3) for v in call], "device_kernel_ms_hot": round(med(hot), 4),
           "device_kernel_ms_cold": round(med(cold), 4), "arena_bytes": int(n_bytes), "bytes_per_launch": int(set_bytes),
           "cold_gb_per_s": round(set_bytes / med(cold) / 1e6, 1), "agrees_with_host_bit_for_bit": bool(agree)}
    if not a.no_step:
        args = argparse.Namespace(steps=10, warmup=3, task="nvs", dtype="f16", train_graph=False, recompute=False)
        step = bench.train_bench(args, 0, 1, dev)
        doc["training_step_ms"] = round(step["ms_per_step"], 3)
        doc["training_step_note"] = "bench.py --workload train --task nvs at its own batch size, same process"
    print(json.dumps(doc))
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(doc, f, indent=1)
        f.write("\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
