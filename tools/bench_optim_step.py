#!/usr/bin/env python
"""Optimizer tail of a mixed-precision training step, two routes interleaved in one process on one GPU:

    hip   -- AmpAdamW.step(): lr_amp_adamw_step, three launches, no read-back
    torch -- GradScaler.unscale_ / step / update around torch.optim.AdamW(capturable=True) (the sync-free torch route)

at two parameter sets: the prompt tokens of BASELINE configs[4] (73 x 1024) and the NVS set (tokens + pose MLP + refinement network
and its gate).  Each pair times `--iters` back-to-back steps of one route, then of the other; the median over `--pairs` pairs is
recorded with the device name and the clocks read while the timed loops run.

It then records the whole fp16 training step at BASELINE configs[4] shapes, again interleaved: the eager step with torch AdamW and the
host-side loss scaler (what `bench.py --workload train` runs in fp16) against forward + HIP backward + AmpAdamW replayed as one hipGraph,
and the JSON line of `bench.py --workload train` itself from a child process on the same box.

    python tools/bench_optim_step.py [--pairs 7] [--iters 200] [--out profiles/optim_step_bench.json]
"""
import argparse
import json
import os
import statistics
import subprocess
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def param_sets(dev):
    import leftrefill_amd.dropin as dropin
    dropin.install()
    from inpainting_ldm.NVS_ldm import refinement_network
    from ldm.modules.encoders.NVS_modules import RelPosModel
    torch.manual_seed(0)
    tokens = lambda: [torch.nn.Parameter(0.02 * torch.randn(73, 1024, device=dev))]
    nvs = tokens() + list(RelPosModel(input_ch=4, out_ch=1024).to(dev).parameters()) + list(refinement_network(320).to(dev).parameters())
    nvs.append(torch.nn.Parameter(torch.zeros((), device=dev)))
    return {"prompt_tokens": tokens(), "nvs_pose_refinement": nvs}


def time_route(step, iters):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(iters):
        step()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / iters * 1e6


def sample_clocks():
    """Start a clock query now; call the result after the timed region to collect it (the query runs while the GPU is busy)."""
    try:
        proc = subprocess.Popen(["rocm-smi", "--showclocks"], stdout=subprocess.PIPE, stderr=subprocess.DEVNULL, text=True)
    except OSError as e:
        return lambda: f"not read: {e}"

    def collect():
        try:
            out = proc.communicate(timeout=30)[0]
        except subprocess.TimeoutExpired:
            proc.kill()
            return "not read: query timed out"
        return [l.strip() for l in out.splitlines() if "sclk" in l or "mclk" in l][:4]
    return collect


def whole_step(dev, pairs, iters):
    """One fp16 prompt-tuning step at BASELINE configs[4] shapes (batch 16 at 256x512, tokens 73 x 1024), two routes interleaved:
    eager  -- what `bench.py --workload train` runs in fp16: torch AdamW, the loss scale and the isfinite read-back on the host
    graph  -- forward, HIP backward and AmpAdamW.step() replayed as ONE hipGraph (the skip decision stays on the device)."""
    import bench
    from leftrefill_amd.optim import AmpAdamW
    Bt, h, w = 16, 32, 64
    model = bench.build_model(dev, "single").train()
    model.model.diffusion_model.compute_dtype = torch.float16
    for p in model.parameters():
        p.requires_grad_(False)
    g = torch.Generator(device=dev).manual_seed(1099)
    base_ctx = torch.randn(Bt, 77, 1024, device=dev, generator=g)
    c_concat = torch.randn(Bt, 5, h, w, device=dev, generator=g)
    x_start = torch.randn(Bt, 4, h, w, device=dev, generator=g)
    t_buf = torch.zeros(Bt, device=dev, dtype=torch.long)
    noise_buf = torch.zeros(Bt, 4, h, w, device=dev)

    def draw():
        t_buf.copy_(torch.randint(0, 1000, (Bt,), device=dev, generator=g))
        noise_buf.copy_(torch.randn(Bt, 4, h, w, device=dev, generator=g))

    def loss_of(tokens):
        ctx = torch.cat([base_ctx[:, :1], base_ctx[:, 1:74] + tokens, base_ctx[:, 74:]], dim=1)
        return model.p_losses(x_start, {"c_concat": [c_concat], "c_crossattn": [ctx]}, t_buf, noise=noise_buf)[0]

    tok_e = torch.nn.Parameter(0.02 * torch.randn(73, 1024, device=dev, generator=g))
    tok_g = torch.nn.Parameter(tok_e.detach().clone())
    topt = torch.optim.AdamW([tok_e], lr=1e-4)
    scaler = {"scale": 2.0 ** 14, "good": 0}

    def eager():
        draw()
        (loss_of(tok_e) * scaler["scale"]).backward()
        if not bool(torch.isfinite(tok_e.grad).all()):
            scaler["scale"], scaler["good"] = scaler["scale"] * 0.5, 0
        else:
            tok_e.grad /= scaler["scale"]
            topt.step()
            scaler["good"] += 1
            if scaler["good"] % 200 == 0:
                scaler["scale"] *= 2.0
        topt.zero_grad(set_to_none=True)

    hip = AmpAdamW([tok_g], lr=1e-4, init_scale=2.0 ** 14, growth_interval=200)

    def body():
        hip.scale(loss_of(tok_g)).backward()
        hip.step()
        hip.zero_grad()

    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        for _ in range(3):
            draw()
            body()
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        body()

    def replay():
        draw()
        graph.replay()

    for _ in range(3):
        eager()
        replay()
    clocks = sample_clocks()
    rows = [(time_route(eager, iters), time_route(replay, iters)) for _ in range(pairs)]
    e, r = statistics.median(p[0] for p in rows), statistics.median(p[1] for p in rows)
    state = hip.amp_state()
    print(f"whole fp16 step: eager (host scaler) {e / 1e3:.2f} ms, one hipGraph with AmpAdamW {r / 1e3:.2f} ms ({e / r:.3f}x)", flush=True)
    return {"shape": "batch 16 at 256x512 (latent 32x64), tokens 73 x 1024, fp16", "unit": "us per training step", "iters": iters,
            "eager_host_scaler_us": e, "graph_amp_adamw_us": r, "eager_over_graph": e / r, "pairs_us": rows, "clocks_during": clocks(),
            "graph_route_state": {k: state[k] for k in ("scale", "skipped", "applied_steps", "sched_steps")}}


def bench_train_line():
    """`bench.py --workload train` (the eager fp16 step as the bench itself measures it) in a fresh child process."""
    p = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--workload", "train", "--steps", "20", "--warmup", "5"],
                       capture_output=True, text=True, timeout=600, cwd=ROOT)
    lines = [l for l in p.stdout.splitlines() if l.startswith("{")]
    return json.loads(lines[-1]) if p.returncode == 0 and lines else {"error": p.stderr[-500:]}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--pairs", type=int, default=7)
    ap.add_argument("--iters", type=int, default=200)
    ap.add_argument("--step-iters", type=int, default=10, help="training steps per timed run of the whole-step comparison")
    ap.add_argument("--no-whole-step", action="store_true")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "optim_step_bench.json"))
    a = ap.parse_args()
    from leftrefill_amd.optim import AmpAdamW
    dev = torch.device("cuda:0")
    rec = {"device": torch.cuda.get_device_name(0), "pairs": a.pairs, "iters": a.iters, "unit": "us per optimizer tail", "sets": {}}
    rec["note"] = ("wall time of back-to-back steps, host included: both tails are launch-bound at these sizes (3 launches through ctypes "
                   "against torch's ~20), so the ratios are launch counts and host overhead, not device time")
    for name, ps in param_sets(dev).items():
        ref = [torch.nn.Parameter(p.detach().clone()) for p in ps]
        grads = [torch.randn_like(p) * 64.0 for p in ps]
        for p, r, g in zip(ps, ref, grads):
            p.grad, r.grad = g.clone(), g.clone()
        hip = AmpAdamW(ps, lr=1e-4)
        topt = torch.optim.AdamW(ref, lr=1e-4, capturable=True)
        scaler = torch.amp.GradScaler("cuda")
        scaler.scale(torch.zeros((), device=dev))

        def torch_step():
            scaler.unscale_(topt)
            scaler.step(topt)
            scaler.update()

        for _ in range(10):
            hip.step()
            torch_step()
        clocks = sample_clocks()
        pairs = [(time_route(hip.step, a.iters), time_route(torch_step, a.iters)) for _ in range(a.pairs)]
        h, t = statistics.median(p[0] for p in pairs), statistics.median(p[1] for p in pairs)
        rec["sets"][name] = {"tensors": len(ps), "elements": sum(p.numel() for p in ps), "hip_us": h, "torch_us": t, "torch_over_hip": t / h,
                             "pairs_us": pairs, "clocks_during": clocks()}
        print(f"{name}: {len(ps)} tensors, {rec['sets'][name]['elements']} elements: hip {h:.1f} us, torch {t:.1f} us ({t / h:.2f}x)", flush=True)
    if not a.no_whole_step:
        rec["whole_fp16_step"] = whole_step(dev, max(5, a.pairs), a.step_iters)
        rec["bench_py_workload_train"] = bench_train_line()
    with open(a.out, "w") as f:
        json.dump(rec, f, indent=1)
    print(json.dumps({"out": a.out, **{k: v["torch_over_hip"] for k, v in rec["sets"].items()}}))


if __name__ == "__main__":
    main()
