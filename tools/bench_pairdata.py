#!/usr/bin/env python
"""Image-pair batch assembly at the training shape (S = 512, batch 8, synthetic 1200 x 1600 sources, two tiles per sample, the plans
of `InpaintingCrossViewDataset`: both resize branches, random / match / view masks, per-half flips):

  host   : `dataprep.run_plan_numpy` per sample, in this process, as a loader worker runs it with raw=False.  A sample takes seconds
           (four dense float64 einsums), so single samples are timed, not batches; a batch costs batch / workers samples.
  device : `collate_raw` (pack), and `DevicePrep.__call__` synchronised (arena + job-table copy and the one lr_batch_prep launch), and
           the launch alone between device events.
  match  : `dataprep.plan_match_mask` alone (pickle load, point selection, PIL polyline on the 256 grid) -- host work on both routes.

Decoding is the same work on both routes and is left out: sources are held in memory.  The routes alternate in one process: one host
sample, then the device repetitions, `--rounds` times.  The training step (bench.py's `--workload train --task refill`) is timed in
the same run unless --no_step.

    python tools/bench_pairdata.py [--out profiles/pairdata_bench.json]
"""
import argparse
import json
import os
import pickle
import random
import statistics
import sys
import tempfile
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import bench  # noqa: E402  (train_bench: the step the loader feeds)
from leftrefill_amd import _lib, dataprep  # noqa: E402

SIZE, BATCH = 512, 8


def write_matches(root, n, seed=0):
    """n match files of 400 points in 832-pixel coordinates, as the matcher writes them."""
    rng = np.random.RandomState(seed)
    for idx in range(n):
        res = dict(mkpts0=rng.uniform(5, 827, (400, 2)).astype(np.float32), mkpts1=rng.uniform(5, 827, (400, 2)).astype(np.float32),
                   scores=rng.uniform(0.85, 1.0, 400).astype(np.float32))
        with open(os.path.join(root, f"{idx:08d}.pkl"), "wb") as f:
            pickle.dump(res, f)


class Pairs:
    """Decoded sources held in memory, planned like InpaintingCrossViewDataset(mode='train', flip=True, view_mask_rate=0.5,
    match_mask=True, match_mask_rate=0.25): item i is (plan, raw), seeded by i."""

    def __init__(self, match_path, seed=0):
        rng = np.random.RandomState(seed)
        self.images = [rng.randint(0, 256, (1200, 1600, 3), dtype=np.uint8) for _ in range(4)]
        self.masks = [(rng.rand(600, 800) < 0.5).astype(np.uint8) * 255 for _ in range(2)]
        self.match_path = match_path

    def __getitem__(self, i):
        random.seed(i)
        np.random.seed(i)
        raw = [self.images[i % 4], self.images[(i + 1) % 4]]
        resizes, crops = [], []
        for img in raw:
            r = dataprep.plan_resize_train(img.shape[0], img.shape[1], SIZE)
            resizes.append(r)
            crops.append(None if (r["rh"], r["rw"]) == (SIZE, SIZE) else dict(w_start=r["x0"], h_start=r["y0"], w=r["rw"], h=r["rh"]))
        order = (1, 0) if random.random() < 0.5 else (0, 1)
        kw = [dict(zero_mask=True), dict(zero_mask=True)]
        if random.random() < 0.5:
            matched = dataprep.plan_match_mask(self.match_path, i % BATCH, "left" if order[0] == 1 else "right", crops[1], crops[0]) \
                if random.random() < 0.25 else None
            if matched is not None:
                raw.append(matched[1])
                kw[0 if matched[0] else 1] = dict(masks=[2])
            else:
                picks = dataprep.plan_mask_train(1, 1)
                raw.extend(self.masks[:len(picks)])
                kw[0 if random.random() < 0.5 else 1] = dict(masks=list(range(2, 2 + len(picks))))
        else:
            kw[0 if random.random() < 0.5 else 1] = dict(outpaint_col=0)
        flips = [random.random() < 0.5, random.random() < 0.5]
        tiles = [dataprep.plan_tile(order[k], flip=flips[k], mask_flip=flips[k], **resizes[order[k]], **kw[k]) for k in (0, 1)]
        return dict(img_size=SIZE, tiles=tiles, txt="p"), raw


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=2, help="host sample / device repetitions, alternating this often")
    ap.add_argument("--reps", type=int, default=5, help="device repetitions per round")
    ap.add_argument("--no_step", action="store_true", help="skip timing the training step")
    ap.add_argument("--out", type=str, default=os.path.join(ROOT, "profiles", "pairdata_bench.json"))
    a = ap.parse_args()
    assert torch.cuda.is_available(), "this benchmark needs the MI355X: a CPU run says nothing about it"
    dev = torch.device("cuda:0")
    lib = _lib.load()
    host, pack, call, kern, match = [], [], [], [], []
    with tempfile.TemporaryDirectory() as root:
        write_matches(root, BATCH)
        ds = Pairs(root)
        items = [ds[i] for i in range(BATCH)]
        prep = dataprep.DevicePrep(SIZE, 2, dev)
        out = prep(dataprep.collate_raw(items))      # warm-up: buffers, module load
        torch.cuda.synchronize()
        first = dataprep.run_plan_numpy(*items[0])
        diff = out["image"][0].cpu().numpy() != first["image"]
        agree = {"mask_equal": bool(np.array_equal(out["mask"][0].cpu().numpy(), first["mask"])), "image_values_differing": int(diff.sum()),
                 "image_values": int(diff.size)}      # random sources are not de-tied: a tie may round the other way, by one level
        st = torch.cuda.current_stream().cuda_stream
        for r in range(a.rounds):
            t0 = time.perf_counter()
            dataprep.run_plan_numpy(*items[(r + 1) % BATCH])
            host.append(1e3 * (time.perf_counter() - t0))
            for _ in range(a.reps):
                t0 = time.perf_counter()
                batch = dataprep.collate_raw(items)
                pack.append(1e3 * (time.perf_counter() - t0))
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                prep(batch)
                torch.cuda.synchronize()
                call.append(1e3 * (time.perf_counter() - t0))
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                for _ in range(10):
                    _lib.check(lib.lr_batch_prep(prep.arena.data_ptr(), batch["arena"].numel(), prep.jobs.data_ptr(), batch["jobs"].data_ptr(),
                                                 2 * BATCH, SIZE, 2, BATCH, prep.image.data_ptr(), prep.masked_image.data_ptr(),
                                                 prep.mask.data_ptr(), st), "batch_prep")
                e1.record()
                e1.synchronize()
                kern.append(e0.elapsed_time(e1) / 10)
            for idx in range(BATCH):
                random.seed(idx)
                np.random.seed(idx)
                t0 = time.perf_counter()
                done = dataprep.plan_match_mask(root, idx, "right", None, None)
                if done is not None:
                    match.append(1e3 * (time.perf_counter() - t0))
    med = statistics.median
    doc = {"config": f"S = {SIZE}, batch {BATCH}, two tiles per sample, synthetic 1200x1600 sources, 600x800 masks, 400-point match files; "
                     "InpaintingCrossViewDataset's training plans; decoding excluded on both routes",
           "timing": f"wall clock, one process, {a.rounds} rounds of one host sample then {a.reps} device repetitions; medians; "
                     "kernel: device events around 10 back-to-back launches on one buffer set (hot: Infinity Cache)",
           "gpu": torch.cuda.get_device_name(0), "host_cpus": len(os.sched_getaffinity(0)),
           "host_ms_per_sample": round(med(host), 1), "host_ms_per_sample_all": [round(v, 1) for v in host],
           "host_ms_per_batch_derived": {"1_worker": round(BATCH * med(host), 1), "8_workers": round(BATCH * med(host) / 8, 1),
                                         "note": "per-sample time x batch / workers; whole host batches were not timed"},
           "device_pack_ms": round(med(pack), 3), "device_call_ms": round(med(call), 3), "device_kernel_ms_hot": round(med(kern), 4),
           "device_call_ms_all": [round(v, 3) for v in call], "arena_bytes": int(batch["arena"].numel()),
           "match_mask_plan_ms": round(med(match), 3), "match_mask_plans_timed": len(match), "agrees_with_host": agree}
    if not a.no_step:
        args = argparse.Namespace(steps=10, warmup=3, task="refill", dtype="f16", train_graph=False, recompute=False)
        step = bench.train_bench(args, 0, 1, dev)
        doc["training_step_ms"] = round(step["ms_per_step"], 3)
        doc["training_step_note"] = "bench.py --workload train --task refill at its own batch size, same process"
    print(json.dumps(doc))
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(doc, f, indent=1)
        f.write("\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
