"""LoRA on the UNet: what it costs (-> profiles/lora_bench.json; no threshold is asserted anywhere).

    python -m tools.bench_lora [--steps 6] [--rounds 3] [--out profiles/lora_bench.json]
    python -m tools.bench_lora --dropout 0.1 [--out profiles/lora_dropout_bench.json]      # LoRA dropout: see main_dropout

In ONE process, routes alternating (the repo's rule for A/B numbers):
  * the configs[4] training step (NVSLDM.p_losses, batch 16 at canvas 256x512 = latent 32x64, bf16): prompt tokens only (the factors frozen:
    the merged packing, i.e. the launches of the un-injected model) against prompt tokens + r = 16 LoRA factors (unmerged route, HIP factor
    gradients), with the peak memory of both;
  * the three MFMA kernels alone at the largest layer shapes of that step (level 0: 32768 rows, GEGLU projection 320 -> 2560) against the
    bytes they must move -- operands, outputs and workspaces built before the timed loop, so a timed call is the launch(es) only;
  * the re-merge (lr_lora_merge_f32 + re-packing the SpatialTransformers' records) after a training step: sync, a no-grad forward whose
    packing is stale, sync, minus the same (eager) forward right after it;
  * the merged sampling step against the un-injected model's (the same launches).
"""
import argparse
import json
import os
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)


def _time(fn, n):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(n):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / n * 1e3


def _event_ms(fn):
    """One call between two device events."""
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1)


def _median(v):
    return sorted(v)[len(v) // 2]


def main_dropout(a):
    """--dropout P (-> profiles/lora_dropout_bench.json; no threshold): what the Philox masks inside the LoRA kernels cost.  In ONE
    process, routes alternating call by call, medians of device-event timings:
      * each masked kernel (lr_lora_*_drop) against its unmasked form at the shapes of profiles/lora_bench.json, plain and with the GEGLU
        column-group table;
      * the configs[4] LoRA training step (as above) at p = 0 against p = P."""
    import bench
    from leftrefill_amd import lora_dropout, ops, packing
    dev = torch.device("cuda:0")
    P = a.dropout
    res = {"rank": a.rank, "dtype": "bf16", "batch": 16, "latent": [32, 64], "p": P}
    M, K, N, R = 16 * 32 * 64, 320, 2560, ops.lora_pad_rank(a.rank)
    dt = torch.bfloat16
    x, y = torch.randn(M, K, device=dev).to(dt), torch.randn(M, N, device=dev).to(dt)
    t = torch.randn(M, R, device=dev).to(dt)
    up = torch.randn(N, R, device=dev).to(dt)
    up_t, t_out = up.t().contiguous(), torch.empty(M, R, device=dev, dtype=dt)
    d_out, ws = torch.empty(R, N, device=dev), ops.lora_wgrad_workspace(M, R, N, dev)
    tab = torch.from_numpy(lora_dropout.colgrp_of(packing.geglu_perm(N // 2).numpy())).to(dev)
    drops = {"unmasked": None, "masked": ops.LoraDrop(1234, 3, 7, P), "masked, GEGLU table": ops.LoraDrop(1234, 3, 7, P, colgrp=tab)}
    kernels = {"down [32768 x 2560] -> r (dT)": (lambda d: ops.lora_down(y, up_t, out=t_out, drop=d), 2 * (M * N + M * R + R * N)),
               "up r -> [32768 x 2560] accumulate": (lambda d: ops.lora_up(t, up, out=y, accumulate=True, drop=d), 2 * (2 * M * N + M * R + R * N)),
               "wgrad [32768 x r]^T [32768 x 2560] (+ reduce)": (lambda d: ops.lora_wgrad(t, y, out=d_out, workspace=ws, drop=d),
                                                                2 * (M * N + M * R * (N // 128)) + 4 * R * N + 2 * ws.numel() * 4)}
    kern = {}
    for name, (fn, nbytes) in kernels.items():
        ms = {k: [] for k in drops}
        for k, d in drops.items():
            fn(d)
        for _ in range(30):
            for k, d in drops.items():
                ms[k].append(_event_ms(lambda: fn(d)))
        kern[name] = {k: {"ms": _median(v), "GB_per_s": nbytes / _median(v) / 1e6} for k, v in ms.items()}
        kern[name]["bytes"] = nbytes
    res["kernels"] = kern
    del x, y, t, t_out, ws

    model = bench.build_model(dev, "nvs").train()
    model.lora_cfg = {"do_lora": True, "lora_type": "default", "lora_rank": a.rank, "lora_scale": 1.0, "lora_dropout": P}
    model.set_lora()
    model = model.to(dev).train()
    unet = model.model.diffusion_model
    unet.compute_dtype = torch.bfloat16
    layers = [m_ for m_ in unet.modules() if hasattr(m_, "lora_up")]
    factors = [p for n, p in unet.named_parameters() if ".lora_" in n]
    with torch.no_grad():
        for n, p in unet.named_parameters():
            if ".lora_up." in n:
                p.normal_(std=0.01)
    for p in model.parameters():
        p.requires_grad_(False)
    for p in factors:
        p.requires_grad_(True)
    g = torch.Generator(device=dev).manual_seed(1)
    Bt, h, w = 16, 32, 64
    ctx = torch.randn(Bt, 77, 1024, device=dev, generator=g)
    c_concat, x_start = torch.randn(Bt, 5, h, w, device=dev, generator=g), torch.randn(Bt, 4, h, w, device=dev, generator=g)
    from leftrefill_amd.optim import AmpAdamW
    opt = AmpAdamW([{"params": factors, "lr": 1e-4, "weight_decay": 0.01}], lr=1e-4, weight_decay=0.01, init_scale=1.0, growth_interval=0)

    def step(p):
        for m_ in layers:
            m_.dropout.p = p
        ts = torch.randint(0, 1000, (Bt,), device=dev, generator=g)
        noise = torch.randn(Bt, 4, h, w, device=dev, generator=g)
        loss, _ = model.p_losses(x_start, {"c_concat": [c_concat], "c_crossattn": [ctx]}, ts, noise=noise)
        opt.scale(loss).backward()
        opt.step()
        opt.zero_grad()

    times = {0.0: [], P: []}
    for p in times:
        step(p)
    for _ in range(a.rounds * a.steps):
        for p in times:
            times[p].append(_event_ms(lambda: step(p)))
    res["train_step_ms"] = {f"p={k:g}": {"median": _median(v), "all": v} for k, v in times.items()}
    print(json.dumps(res))
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=6)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--rank", type=int, default=16)
    ap.add_argument("--dropout", type=float, default=None, help="measure the masked kernels and the training step at this LoRA dropout rate")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if a.dropout is not None:
        a.out = a.out or os.path.join(ROOT, "profiles", "lora_dropout_bench.json")
        return main_dropout(a)
    a.out = a.out or os.path.join(ROOT, "profiles", "lora_bench.json")
    import bench
    from leftrefill_amd import ops
    dev = torch.device("cuda:0")
    res = {"rank": a.rank, "dtype": "bf16", "batch": 16, "latent": [32, 64]}

    # ---- the three MFMA kernels alone ------------------------------------------------------------------------------------------------
    M, K, N, R = 16 * 32 * 64, 320, 2560, ops.lora_pad_rank(a.rank)
    dt = torch.bfloat16
    x, y = torch.randn(M, K, device=dev).to(dt), torch.randn(M, N, device=dev).to(dt)
    t = torch.randn(M, R, device=dev).to(dt)
    down, up = torch.randn(R, K, device=dev).to(dt), torch.randn(N, R, device=dev).to(dt)
    kern = {}
    up_t, t_out = up.t().contiguous(), torch.empty(M, R, device=dev, dtype=dt)
    d_out, ws = torch.empty(R, N, device=dev), ops.lora_wgrad_workspace(M, R, N, dev)
    for name, fn, nbytes in (("down [32768 x 320] -> r", lambda: ops.lora_down(x, down, out=t_out), 2 * (M * K + M * R + R * K)),
                             ("down [32768 x 2560] -> r (dT)", lambda: ops.lora_down(y, up_t, out=t_out), 2 * (M * N + M * R + R * N)),
                             ("up r -> [32768 x 2560] accumulate", lambda: ops.lora_up(t, up, out=y, accumulate=True), 2 * (2 * M * N + M * R + R * N)),
                             ("wgrad [32768 x r]^T [32768 x 2560] (+ reduce)", lambda: ops.lora_wgrad(t, y, out=d_out, workspace=ws),
                              2 * (M * N + M * R * (N // 128)) + 4 * R * N + 2 * ws.numel() * 4)):
        fn()
        ms = _time(fn, 20)
        kern[name] = {"ms": ms, "bytes": nbytes, "GB_per_s": nbytes / ms / 1e6}
    res["kernels"] = kern
    del x, y, t, t_out, ws

    # ---- training step: prompt only vs prompt + LoRA factors ---------------------------------------------------------------------------
    model = bench.build_model(dev, "nvs").train()
    model.lora_cfg = {"do_lora": True, "lora_type": "default", "lora_rank": a.rank, "lora_scale": 1.0}
    model.set_lora()
    model = model.to(dev)
    unet = model.model.diffusion_model
    unet.compute_dtype = torch.bfloat16
    factors = [p for n, p in unet.named_parameters() if ".lora_" in n]
    with torch.no_grad():      # nonzero up factors: the down gradients are not trivially zero
        for n, p in unet.named_parameters():
            if ".lora_up." in n:
                p.normal_(std=0.01)
    for p in model.parameters():
        p.requires_grad_(False)
    g = torch.Generator(device=dev).manual_seed(1)
    tokens = torch.nn.Parameter(0.02 * torch.randn(73, 1024, device=dev, generator=g))
    Bt, h, w = 16, 32, 64
    base_ctx = torch.randn(Bt, 77, 1024, device=dev, generator=g)
    c_concat, x_start = torch.randn(Bt, 5, h, w, device=dev, generator=g), torch.randn(Bt, 4, h, w, device=dev, generator=g)
    # the trainer's optimizer (AmpAdamW in its bf16 mode: scale 1, no growth), the factors in a group of their own as configure_optimizers builds it
    from leftrefill_amd.optim import AmpAdamW
    amp = dict(lr=1e-4, weight_decay=0.01, init_scale=1.0, growth_interval=0)
    opts = {"prompt": AmpAdamW([{"params": [tokens]}], **amp),
            "lora": AmpAdamW([{"params": [tokens]}, {"params": factors, "lr": 1e-4, "weight_decay": 0.01}], **amp)}

    def step(route):
        for p in factors:
            p.requires_grad_(route == "lora")
        ctx = torch.cat([base_ctx[:, :1], base_ctx[:, 1:74] + tokens, base_ctx[:, 74:]], dim=1)
        ts = torch.randint(0, 1000, (Bt,), device=dev, generator=g)
        noise = torch.randn(Bt, 4, h, w, device=dev, generator=g)
        loss, _ = model.p_losses(x_start, {"c_concat": [c_concat], "c_crossattn": [ctx]}, ts, noise=noise)
        opts[route].scale(loss).backward()
        opts[route].step()
        opts[route].zero_grad()

    times, peaks = {"prompt": [], "lora": []}, {}
    for _ in range(a.rounds):
        for route in ("prompt", "lora"):
            step(route)                                   # after a switch: re-merge / first-use work stays out of the timing
            torch.cuda.synchronize()
            torch.cuda.reset_peak_memory_stats()
            times[route].append(_time(lambda: step(route), a.steps))
            peaks[route] = max(peaks.get(route, 0), torch.cuda.max_memory_allocated())
    res["train_step_ms"] = {k: {"median": sorted(v)[len(v) // 2], "all": v} for k, v in times.items()}
    res["train_peak_GB"] = {k: v / 2 ** 30 for k, v in peaks.items()}

    # ---- re-merge, and the merged sampling step against the un-injected model's --------------------------------------------------------
    for p in factors:
        p.requires_grad_(False)
    model.eval()
    xs, tt = torch.randn(2, 9, 64, 128, device=dev, generator=g), torch.tensor([501, 501], device=dev)
    cs = torch.randn(2, 77, 1024, device=dev, generator=g)
    merges = []
    unet.use_hip_graph = False                            # eager steps here: a re-merge also drops the captured graphs, whose re-capture is not its cost
    with torch.no_grad():
        unet(xs, tt, context=cs)
        for _ in range(3):
            unet._plan["root"]["merged_stale"] = True
            stale = _time(lambda: unet(xs, tt, context=cs), 1)      # re-merge + one eager step
            fresh = _time(lambda: unet(xs, tt, context=cs), 1)      # one eager step on the packing it just built
            merges.append(stale - fresh)
    unet.use_hip_graph = True
    res["remerge_ms"] = {"median": sorted(merges)[1], "all": merges}
    plain = bench.build_model(dev, "nvs").eval().model.diffusion_model
    plain.compute_dtype = torch.bfloat16
    samp = {"merged": [], "uninjected": []}
    with torch.no_grad():
        for m_ in (unet, plain):
            for _ in range(3):
                m_(xs, tt, context=cs)
        for _ in range(a.rounds):
            samp["merged"].append(_time(lambda: unet(xs, tt, context=cs), 10))
            samp["uninjected"].append(_time(lambda: plain(xs, tt, context=cs), 10))
    res["sampling_step_ms"] = {k: {"median": sorted(v)[len(v) // 2], "all": v} for k, v in samp.items()}
    print(json.dumps(res))
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
