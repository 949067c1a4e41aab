"""What recording reference-attention maps costs, at BASELINE configs[1] shapes (B = 4, UNet batch 8 under CFG 2.5, latent 64 x 128,
50 DDIM steps; the full UNet with bench.py's random weights).

    python tools/bench_attn_probe.py [--reps 3] [--steps 50] [--out profiles/attn_probe_bench.json]

Routes, alternated in one process (`reps` rounds after one warm-up sampling each; a sampling is timed with the host clock around
device-synchronised work and divided by its steps):
    captured        the default: one hipGraph replay per step (CFG shared prefix on)
    eager           the same launches issued from Python (`eager_only`), what a probe runs on top of
    probe_all       eager under AttentionProbe(unet): all 16 self-attention layers recorded
    probe_small     eager under AttentionProbe(unet, layers = those with 128, 512 or 2048 tokens)
and the probe kernel alone (3 columns) next to lr_attention_f16 on the same fused q|k|v projection at 8192 x 8192 tokens, 5 heads,
batch 8 (device events over `--kernel-iters` alternating launches).  Prints one JSON line and writes it to --out."""
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

SMALL_TOKENS = (128, 512, 2048)


def sampling(model, batch, B, steps, route, layers=None):
    """Seconds of one DDIM sampling by `route`; also the probe (or None)."""
    from leftrefill_amd.attnprobe import AttentionProbe
    c_concat, c_cross, uc_cross, x_T = batch
    cond = {"c_concat": [c_concat], "c_crossattn": [c_cross]}
    uc = {"c_concat": [c_concat], "c_crossattn": [uc_cross]}
    unet = model.model.diffusion_model
    kw = dict(cond=cond, batch_size=B, ddim=True, ddim_steps=steps, eta=0.0, unconditional_guidance_scale=bench.CFG,
              unconditional_conditioning=uc, x_T=x_T)
    probe = None
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    if route == "captured":
        model.sample_log(**kw)
    elif route == "eager":
        prev = getattr(unet, "eager_only", False)
        unet.eager_only = True
        try:
            model.sample_log(**kw)
        finally:
            unet.eager_only = prev
    else:
        with AttentionProbe(unet, layers=layers) as probe:
            model.sample_log(**kw)
    torch.cuda.synchronize()
    return time.perf_counter() - t0, probe


def kernel_alone(iters, device):
    """us per launch of ops.attention_probe (3 canvas columns) and of ops.attention_qkv on one q|k|v projection, alternating."""
    from leftrefill_amd import ops
    from leftrefill_amd.attnprobe import canvas_columns
    B, heads, h, w = 8, 5, 64, 128
    L, C = h * w, heads * 64
    qkv = torch.randn(B * L, 3 * C, device=device, dtype=torch.float16)
    cols = canvas_columns(h, w, torch.float16, device)
    out = torch.zeros(B, L, 3, device=device)
    scale = 64 ** -0.5
    fns = {"attention_probe_us": lambda: ops.attention_probe(qkv[:, :C], qkv[:, C:2 * C], cols, B, heads, L, L, scale, out=out, beta=1.0),
           "attention_us": lambda: ops.attention_qkv(qkv, B, heads, L, scale)}
    for f in fns.values():
        for _ in range(3):
            f()
    times = {k: [] for k in fns}
    for _ in range(iters):
        for k, f in fns.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            f()
            e1.record()
            e1.synchronize()
            times[k].append(1e3 * e0.elapsed_time(e1))
    res = {k: round(statistics.median(v), 1) for k, v in times.items()}
    res.update(shape=f"B {B}, {heads} heads, {L} x {L} tokens, d_head 64, f16", iters=iters,
               probe_vs_attention=round(res["attention_probe_us"] / res["attention_us"], 4))
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--steps", type=int, default=50)
    ap.add_argument("--kernel-iters", type=int, default=30)
    ap.add_argument("--out", type=str, default=os.path.join(ROOT, "profiles", "attn_probe_bench.json"))
    a = ap.parse_args()
    device = torch.device("cuda:0")
    B, h, w = 4, 64, 128
    model = bench.build_model(device)
    batch = bench.synthetic_batch(B, h, w, device, 1234)
    with torch.no_grad():
        _, probe = sampling(model, batch, B, a.steps, "probe_all")                 # warm-up, and the layer table
        tokens = {l: probe.canvas_of(l)[0] * probe.canvas_of(l)[1] for l in probe.recorded}
        small = [l for l, n in tokens.items() if n in SMALL_TOKENS]
        routes = [("captured", None), ("eager", None), ("probe_all", None), ("probe_small", small)]
        for r, layers in routes[:2] + routes[3:]:
            sampling(model, batch, B, a.steps, r if layers is None else "probe", layers)      # warm-up: graph capture, allocator
        times = {r: [] for r, _ in routes}
        for _ in range(a.reps):
            for r, layers in routes:
                times[r].append(sampling(model, batch, B, a.steps, r, layers)[0])
        kern = kernel_alone(a.kernel_iters, device)
    ms = {r: round(1e3 * statistics.median(t) / a.steps, 3) for r, t in times.items()}
    line = json.dumps({"config": f"configs[1]: B={B}, UNet batch {2 * B}, latent {h}x{w}, cfg {bench.CFG}, DDIM {a.steps}, full UNet (bench.py weights)",
                       "gpu": torch.cuda.get_device_name(0), "reps": a.reps, "ms_per_step": ms,
                       "all_s": {r: [round(x, 4) for x in t] for r, t in times.items()},
                       "probe_all_over_eager_ms": round(ms["probe_all"] - ms["eager"], 3),
                       "probe_small_over_eager_ms": round(ms["probe_small"] - ms["eager"], 3),
                       "layers": {"tokens": tokens, "small": small}, "kernel_alone": kern})
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
