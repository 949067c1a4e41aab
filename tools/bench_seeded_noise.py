"""What a seeded draw costs next to torch.randn, at the sampler's noise shapes (no threshold; a measurement, not a claim).

    python tools/bench_seeded_noise.py [--iters 200] [--out profiles/seeded_noise_bench.json]

Shapes: [8, 4, 64, 128] (BASELINE configs[1]: batch 8 latents of 64 x 128) and [1, 4, 64, 128].  Routes, alternating call by call in one
process after a warm-up of both, each call between two device events on the current stream:
    torch_randn       torch.randn(shape, device=...)            (allocates its result, like noise_like)
    seeded_normal     SeededNoise.normal(STEP, k, shape[1:])    (allocates its result; one lr_seeded_normal launch)
    seeded_normal_out the same into a preallocated tensor        (the launch and its host path alone)
Reported: the median of the per-call device-event times in microseconds and the bytes written.  Prints one JSON line and writes it to --out."""
import argparse
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

SHAPES = ((8, 4, 64, 128), (1, 4, 64, 128))


def measure(shape, iters, device):
    from leftrefill_amd import noise as N
    sn = N.SeededNoise(list(range(shape[0])), device=device)
    out = torch.empty(shape, device=device)
    step = [0]

    def seeded():
        step[0] += 1
        return sn.normal(N.STEP, step[0], shape[1:])

    def seeded_out():
        step[0] += 1
        return sn.normal(N.STEP, step[0], shape[1:], out=out)

    fns = {"torch_randn": lambda: torch.randn(shape, device=device), "seeded_normal": seeded, "seeded_normal_out": seeded_out}
    for f in fns.values():
        for _ in range(10):
            f()
    torch.cuda.synchronize()
    times = {k: [] for k in fns}
    for _ in range(iters):
        for k, f in fns.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            f()
            e1.record()
            e1.synchronize()
            times[k].append(1e3 * e0.elapsed_time(e1))
    res = {k + "_us": round(statistics.median(v), 2) for k, v in times.items()}
    res.update({k + "_us_min": round(min(v), 2) for k, v in times.items()})
    res["bytes"] = 4 * out.numel()
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=200)
    ap.add_argument("--out", type=str, default=os.path.join(ROOT, "profiles", "seeded_noise_bench.json"))
    a = ap.parse_args()
    device = torch.device("cuda:0")
    res = {"x".join(str(d) for d in s): measure(s, a.iters, device) for s in SHAPES}
    line = json.dumps({"gpu": torch.cuda.get_device_name(0), "iters": a.iters, "timing": "device events around one call, routes alternating, medians",
                       "shapes": res})
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
