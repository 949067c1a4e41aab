"""Sampler throughput at BASELINE configs[1] shapes: DDIM-50 (the bench.py metric's sampler), PLMS-50, DPM-Solver++(2M)-20,
StructureDDIMSampler-50 (Tm = 25: 25 three-way evaluations at batch 3B, then 25 two-way at 2B; Tm = 0: three-way throughout, the
cost of one batch-3B evaluation) and DDIM encode-25 + decode-25 (an inversion round trip at S = 50).

    python tools/bench_samplers.py [--reps 3] [--out FILE]

Same model and batch as bench.py (B = 4, latent 64x128, CFG 2.5, the full-size UNet with bench.py's random weights, built by
bench.build_model / bench.synthetic_batch).  One warm-up sampling per sampler, then `reps` rounds in which the three samplers
alternate; each sampling is timed with the host clock around device-synchronised work.  Prints one JSON line: per sampler the
steps, UNet evaluations per sampling, seconds per batch (median), images/s and ms per UNet evaluation."""
import argparse
import json
import os
import statistics
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

import bench  # noqa: E402

# (sampler, steps, UNet evaluations); structure-N: StructureDDIMSampler with Tm = N, encode+decode: N steps each way at S = 50
SAMPLERS = [("ddim", 50, 50), ("plms", 50, 51), ("dpm_solver", 20, 20), ("structure-25", 50, 50), ("structure-0", 50, 50),
            ("encode+decode", 25, 50)]
COND_WEIGHT = 0.7


def run(model, batch, B, sampler, steps):
    c_concat, c_cross, uc_cross, x_T = batch
    cond = {"c_concat": [c_concat], "c_crossattn": [c_cross]}
    uc = {"c_concat": [c_concat], "c_crossattn": [uc_cross]}
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    if sampler.startswith("structure-"):
        from ldm.models.diffusion.ddim import StructureDDIMSampler
        cs = {"c_concat": [c_concat], "c_crossattn": [c_cross.flip(0).contiguous()]}     # a context that differs from cond's
        out, _ = StructureDDIMSampler(model).sample(steps, B, tuple(x_T.shape[1:]), cond, verbose=False, eta=0.0, x_T=x_T,
                                                    unconditional_guidance_scale=bench.CFG, unconditional_conditioning=uc,
                                                    Tm=int(sampler.split("-")[1]) * steps // 50, cond_simple=cs,
                                                    cond_weight=COND_WEIGHT)
    elif sampler == "encode+decode":
        from ldm.models.diffusion.ddim import DDIMSampler
        s = DDIMSampler(model)
        s.make_schedule(2 * steps, ddim_eta=0.0, verbose=False)
        z, _ = s.encode(x_T, cond, steps, unconditional_guidance_scale=bench.CFG, unconditional_conditioning=uc)
        out = s.decode(z, cond, steps, unconditional_guidance_scale=bench.CFG, unconditional_conditioning=uc)
    else:
        out, _ = model.sample_log(cond=cond, batch_size=B, ddim=True, ddim_steps=steps, eta=0.0,
                                  unconditional_guidance_scale=bench.CFG, unconditional_conditioning=uc, x_T=x_T, sampler=sampler)
    torch.cuda.synchronize()
    return time.perf_counter() - t0, out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--steps-scale", type=float, default=1.0, help="multiply every step count (quick runs, e.g. a kernel trace)")
    ap.add_argument("--only", type=str, default=None, help="run one sampler only")
    ap.add_argument("--out", type=str, default=None)
    a = ap.parse_args()
    device = torch.device("cuda:0")
    B, h, w = 4, 64, 128
    model = bench.build_model(device)
    batch = bench.synthetic_batch(B, h, w, device, 1234)
    todo = [(s, max(2, int(round(n * a.steps_scale))), e) for s, n, e in SAMPLERS if a.only in (None, s)]
    times = {s: [] for s, _, _ in todo}
    with torch.no_grad():
        for s, n, _ in todo:
            run(model, batch, B, s, n)                               # warm-up: graph capture, embedding rows, allocator
        for _ in range(a.reps):
            for s, n, _ in todo:
                times[s].append(run(model, batch, B, s, n)[0])
    res = {}
    for s, n, _ in todo:
        evals = n + 1 if s == "plms" else (2 * n if s == "encode+decode" else n)
        sec = statistics.median(times[s])
        res[s] = {"steps": n, "unet_evals": evals, "s_per_batch": round(sec, 4), "images_per_s": round(B / sec, 3),
                  "ms_per_eval": round(1e3 * sec / evals, 3), "all_s": [round(t, 4) for t in times[s]]}
    if "ddim" in res:
        for s in res:
            res[s]["ms_per_eval_vs_ddim"] = round(res[s]["ms_per_eval"] / res["ddim"]["ms_per_eval"], 4)
            res[s]["images_per_s_vs_ddim"] = round(res[s]["images_per_s"] / res["ddim"]["images_per_s"], 3)
    # every structure-0 evaluation is one batch-3B UNet call (no shared prefix), every DDIM one a batch-2B call (shared prefix on)
    ratio3 = (round(res["structure-0"]["ms_per_eval"] / res["ddim"]["ms_per_eval"], 4) if "ddim" in res and "structure-0" in res
              else None)
    line = json.dumps({"config": "configs[1]: B=4, latent 64x128, cfg 2.5, full UNet (bench.py weights)", "reps": a.reps,
                       "gpu": torch.cuda.get_device_name(0), "samplers": res,
                       "eval_3B_vs_2B": ratio3})
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
