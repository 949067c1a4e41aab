"""Sampler throughput at BASELINE configs[1] shapes: DDIM-50 (the bench.py metric's sampler), PLMS-50, DPM-Solver++(2M)-20,
StructureDDIMSampler-50 (Tm = 25: 25 three-way evaluations at batch 3B, then 25 two-way at 2B; Tm = 0: three-way throughout, the
cost of one batch-3B evaluation), DDIM encode-25 + decode-25 (an inversion round trip at S = 50) and the ancestral DDPM chain over
the full schedule (ddpm-1000: `LatentDiffusion.sample`, UNet batch B, no guidance).

    python tools/bench_samplers.py [--reps 3] [--only SAMPLER] [--torch-update] [--out FILE]

With the ddpm-1000 row the line also carries `ddpm_split`: ms per step of the chain next to the B = 4 scale-1 UNet step of the same
run (the floor), the update alone and the rest (host gap).  --torch-update adds the same chain with the update done by the
reference's eager torch expression (predict_start_from_noise, clamp_, q_posterior, nonzero mask, exp) instead of lr_ddpm_step --
a switch of this tool, not of the library: what code ported from the reference would run.

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
            ("encode+decode", 25, 50), ("ddpm-1000", 1000, 1000)]
COND_WEIGHT = 0.7


def torch_posterior_step(self, x, eps, t_host, noise, clip_denoised, return_x0, known=None):
    """LatentDiffusion._posterior_step as the reference's eager expression (ddpm.py:950-960, 986-997) on device tables."""
    assert known is None
    t = torch.full((x.shape[0],), int(t_host), device=x.device, dtype=torch.long)
    x_recon = self.predict_start_from_noise(x, t=t, noise=eps)
    if clip_denoised:
        x_recon.clamp_(-1., 1.)
    model_mean, _, model_log_variance = self.q_posterior(x_start=x_recon, x_t=x, t=t)
    nonzero_mask = (1 - (t == 0).float()).reshape(x.shape[0], *((1,) * (len(x.shape) - 1)))
    return model_mean + nonzero_mask * (0.5 * model_log_variance).exp() * noise, (x_recon if return_x0 else None)


class torch_update:
    """While active, the ancestral chain of `model` updates with torch_posterior_step."""

    def __init__(self, model, on=True):
        self.model, self.on = model, on

    def __enter__(self):
        if self.on:
            import types
            self.model._posterior_step = types.MethodType(torch_posterior_step, self.model)

    def __exit__(self, *exc):
        if self.on:
            del self.model._posterior_step


def ddpm_split(model, batch, B, n=100):
    """ms per call, device-synchronised host clock over n back-to-back calls: the captured UNet step at batch B (host-named
    timestep, as the chain calls it) and each of the two updates alone."""
    from ldm.models.diffusion.ddim import CFGModelEval
    c_concat, c_cross, _, x_T = batch
    cond = {"c_concat": [c_concat], "c_crossattn": [c_cross]}
    ev = CFGModelEval()
    ev.model = model
    ev._prepare_timesteps(range(n))
    ts = [torch.full((B,), i, device=x_T.device, dtype=torch.long) for i in range(n)]
    noise = torch.randn_like(x_T)

    def timed(f):
        for i in range(3):
            f(i)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for i in range(n):
            f(i)
        torch.cuda.synchronize()
        return 1e3 * (time.perf_counter() - t0) / n

    def unet(i):
        with ev._step_hint(i):
            return model.apply_model(x_T, ts[i], cond)

    eps = unet(1).clone()
    out = {"unet_step_ms": round(timed(unet), 4), "calls": n}
    out["hip_update_ms"] = round(timed(lambda i: model._posterior_step(x_T, eps, max(i, 1), noise, True, False)), 4)
    with torch_update(model):
        out["torch_update_ms"] = round(timed(lambda i: model._posterior_step(x_T, eps, max(i, 1), noise, True, False)), 4)
    return out


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
    elif sampler.startswith("ddpm-"):
        # the chain is as long as the model's schedule; a shorter one (--steps-scale) runs its last `steps` timesteps
        out, _ = model.sample_log(cond=cond, batch_size=B, ddim=False, ddim_steps=None, sampler="ddpm", x_T=x_T,
                                  timesteps=steps)
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
    ap.add_argument("--torch-update", action="store_true",
                    help="also run ddpm-1000 with the eager torch update instead of lr_ddpm_step (row ddpm-1000-torch-update)")
    ap.add_argument("--out", type=str, default=None)
    a = ap.parse_args()
    device = torch.device("cuda:0")
    B, h, w = 4, 64, 128
    model = bench.build_model(device)
    batch = bench.synthetic_batch(B, h, w, device, 1234)
    todo = [(s, max(2, int(round(n * a.steps_scale))), e) for s, n, e in SAMPLERS if a.only in (None, s)]
    if a.torch_update:
        todo += [(s + "-torch-update", n, e) for s, n, e in todo if s.startswith("ddpm-")]
    times = {s: [] for s, _, _ in todo}
    base = lambda s: s[:-len("-torch-update")] if s.endswith("-torch-update") else s
    hw = bench.HwSampler(device).start()
    with torch.no_grad():
        for s, n, _ in todo:
            with torch_update(model, s != base(s)):
                run(model, batch, B, base(s), n)                     # warm-up: graph capture, embedding rows, allocator
        for _ in range(a.reps):
            for s, n, _ in todo:
                with torch_update(model, s != base(s)):
                    times[s].append(run(model, batch, B, base(s), n)[0])
        split = ddpm_split(model, batch, B) if any(s.startswith("ddpm-") for s, _, _ in todo) else None
    hw_stats = hw.stop()
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
    if split is not None:
        # per step of the chain: the UNet step and the update as measured alone, the rest is host work between launches
        for s in res:
            if s.startswith("ddpm-"):
                upd = split["torch_update_ms" if s.endswith("-torch-update") else "hip_update_ms"]
                split[s] = {"ms_per_step": res[s]["ms_per_eval"], "unet_replay_ms": split["unet_step_ms"], "update_ms": upd,
                            "host_gap_ms": round(res[s]["ms_per_eval"] - split["unet_step_ms"] - upd, 4),
                            "vs_unet_step": round(res[s]["ms_per_eval"] / split["unet_step_ms"], 4)}
    line = json.dumps({"config": "configs[1]: B=4, latent 64x128, cfg 2.5, full UNet (bench.py weights); ddpm: UNet batch 4, no cfg",
                       "reps": a.reps, "gpu": torch.cuda.get_device_name(0), "samplers": res,
                       "eval_3B_vs_2B": ratio3, "ddpm_split": split,
                       "sclk_mhz_mean": hw_stats.get("sclk_mhz_mean"), "power_w_mean": hw_stats.get("power_w_mean"),
                       "hw_sampler": hw_stats.get("hw_sampler")})
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
