"""One prompt-tuning optimisation step at configs[4] shapes with and without the OpenCLIP text tower in the gradient path.

    python tools/bench_prompt_tuning.py [--steps 10] [--warmup 3] [--out profiles/prompt_tuning_bench.json] [--only C]

Per-GPU batch 16, canvas 256x512 (latent 32x64), NVS task model (what `bench.py --workload train` runs), bf16 UNet, AdamW on the 73 learned
token rows, loss scale 2^14, synthetic weights.  The tower is ViT-H-text sized: width 1024, 16 heads, 24 pre-LN blocks, MLP 4096, causal
mask, 77 tokens, "penultimate" (23 blocks run), frozen; tokens 1..73 of every prompt are the learned rows.
  (A) no tower: the learned rows are added into a fixed context (bench.py --workload train);
  (B) the tower on the eager PyTorch modules under bf16 autocast (the encoder's fallback when `use_hip_backward` is off);
  (C) the tower on the HIP kernels, bf16 (text_engine's differentiable path, `use_hip_backward = True`).
After a warm-up of every variant the timed steps alternate A, B, C in the same process, each timed between device synchronisations.  The
tower's own forward + input-gradient backward is timed the same way for (B) and (C).  --only C runs (C) alone (the profiler run).
"""
import argparse
import json
import os
import statistics
import sys
import time

import torch
import torch.nn as nn

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

B, H_LAT, W_LAT, CTX, WIDTH, HEADS, LAYERS, N_TOK = 16, 32, 64, 77, 1024, 16, 24, 73
RUN_BLOCKS = LAYERS - 1      # penultimate


def tower_flops(batch=B, n=CTX, d=WIDTH, blocks=RUN_BLOCKS):
    """FLOP of the tower from the shapes: the four linears are 12 d^2 MAC per token per block; QK^T and PV are 2 n d MAC per token per
    block counted dense (the causal kernels skip only whole tiles above the diagonal).  Input-gradient backward: one dgrad GEMM per
    linear (= the forward's linear FLOP) and 2.5x the attention forward (recomputed S, dV, dP, dQ, dK)."""
    tok = batch * n
    lin = 2 * 12 * d * d * tok * blocks
    att = 2 * 2 * n * d * tok * blocks
    return {"forward": lin + att, "backward_input_grad": lin + 2.5 * att, "linear_per_token_per_block": 2 * 12 * d * d}


class Tower(nn.Module):
    """open_clip's text transformer surface (oracle/clip_stub.py blocks: nn.MultiheadAttention, GELU MLP) at ViT-H-text size."""

    def __init__(self):
        super().__init__()
        from oracle.clip_stub import ResidualAttentionBlock
        self.transformer = nn.Module()
        self.transformer.resblocks = nn.ModuleList([ResidualAttentionBlock(WIDTH, HEADS) for _ in range(LAYERS)])
        self.positional_embedding = nn.Parameter(0.01 * torch.randn(CTX, WIDTH))
        self.ln_final = nn.LayerNorm(WIDTH)
        self.register_buffer("attn_mask", torch.full((CTX, CTX), float("-inf")).triu_(1), persistent=False)

    def eager(self, x):      # the eager branch of Refill_modules.PromptCLIPEmbedder.encode_with_transformer
        x = (x + self.positional_embedding).permute(1, 0, 2)
        for r in self.transformer.resblocks[:RUN_BLOCKS]:
            x = r(x, attn_mask=self.attn_mask)
        return self.ln_final(x.permute(1, 0, 2))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--only", default=None, choices=["A", "B", "C"])
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import bench
    from leftrefill_amd import text_engine
    dev = torch.device("cuda:0")
    torch.manual_seed(0)
    model = bench.build_model(dev, "nvs").train()
    model.model.diffusion_model.compute_dtype = torch.bfloat16
    for p in model.parameters():
        p.requires_grad_(False)
    tower = Tower().to(dev).eval()
    for p in tower.parameters():
        p.requires_grad_(False)
    packed = text_engine.PackedTextTower(tower, layer_idx=1, compute_dtype=torch.bfloat16)
    g = torch.Generator(device=dev).manual_seed(1099)
    tokens = nn.Parameter(0.02 * torch.randn(N_TOK, WIDTH, device=dev, generator=g))
    opt = torch.optim.AdamW([tokens], lr=1e-4)
    base = torch.randn(B, CTX, WIDTH, device=dev, generator=g)          # token embeddings (A: the fixed context)
    c_concat = torch.randn(B, 5, H_LAT, W_LAT, device=dev, generator=g)
    x_start = torch.randn(B, 4, H_LAT, W_LAT, device=dev, generator=g)
    dz = torch.randn(B, CTX, WIDTH, device=dev, generator=g)
    scale = 2.0 ** 14

    def spliced():
        return torch.cat([base[:, :1], tokens.expand(B, -1, -1), base[:, 1 + N_TOK:]], dim=1)

    def context(v):
        if v == "A":
            return torch.cat([base[:, :1], base[:, 1:1 + N_TOK] + tokens, base[:, 1 + N_TOK:]], dim=1)
        if v == "B":
            with torch.autocast("cuda", dtype=torch.bfloat16):
                return tower.eager(spliced()).float()
        return text_engine.encode_with_transformer(spliced(), packed)

    def step(v):
        t = torch.randint(0, 1000, (B,), device=dev, generator=g)
        noise = torch.randn(B, 4, H_LAT, W_LAT, device=dev, generator=g)
        loss, _ = model.p_losses(x_start, {"c_concat": [c_concat], "c_crossattn": [context(v)]}, t, noise=noise)
        (loss * scale).backward()
        tokens.grad /= scale
        opt.step()
        opt.zero_grad(set_to_none=True)

    def tower_only(v):
        context(v).backward(dz)
        tokens.grad = None

    def timed(fn, v):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn(v)
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3

    variants = [a.only] if a.only else ["A", "B", "C"]
    for v in variants:
        for _ in range(a.warmup):
            step(v)
            if v != "A":
                tower_only(v)
    torch.cuda.synchronize()
    ms = {v: [] for v in variants}
    tms = {v: [] for v in variants if v != "A"}
    for _ in range(a.steps):
        for v in variants:      # alternating: clock / thermal drift hits every variant alike
            ms[v].append(timed(step, v))
            if v != "A":
                tms[v].append(timed(tower_only, v))
    fl = tower_flops()
    res = {"config": {"workload": "configs[4] prompt tuning: NVS task model p_losses, per-GPU batch 16, canvas 256x512 (latent 32x64), "
                                  "bf16, AdamW on 73 x 1024 learned rows, loss scale 2^14, synthetic weights",
                      "tower": f"width {WIDTH}, {HEADS} heads, {LAYERS} blocks, penultimate ({RUN_BLOCKS} run), MLP {4 * WIDTH}, {CTX} tokens, "
                               "frozen (input gradients only)",
                      "variants": {"A": "no tower (bench.py --workload train)", "B": "eager PyTorch tower under bf16 autocast",
                                   "C": "HIP tower, bf16 (use_hip_backward)"},
                      "steps": a.steps, "warmup": a.warmup, "timing": "median per-step wall time between torch.cuda.synchronize(), "
                                                                        "variants alternating in one process"},
           "tower_tflop": {"forward": fl["forward"] / 1e12, "backward_input_grad": fl["backward_input_grad"] / 1e12,
                           "linear_mflop_per_token_per_block": fl["linear_per_token_per_block"] / 1e6},
           "variants": {}}
    for v in variants:
        med = statistics.median(ms[v])
        r = {"ms_per_step": med, "ms_per_step_min": min(ms[v]), "samples_per_s": B / med * 1e3}
        if v != "A":
            tm = statistics.median(tms[v])
            r["tower_fwd_bwd_ms"] = tm
            r["tower_tflop_per_s"] = (fl["forward"] + fl["backward_input_grad"]) / (tm * 1e-3) / 1e12
        res["variants"][v] = r
    if "A" in ms:
        for v in ("B", "C"):
            if v in ms:
                res["variants"][v]["tower_share_of_step"] = 1.0 - res["variants"]["A"]["ms_per_step"] / res["variants"][v]["ms_per_step"]
    if "B" in ms and "C" in ms:
        res["step_speedup_C_over_B"] = res["variants"]["B"]["ms_per_step"] / res["variants"]["C"]["ms_per_step"]
        res["tower_speedup_C_over_B"] = res["variants"]["B"]["tower_fwd_bwd_ms"] / res["variants"]["C"]["tower_fwd_bwd_ms"]
    print(json.dumps(res))
    if a.out:
        with open(a.out, "w") as f:
            f.write(json.dumps(res, indent=1) + "\n")


if __name__ == "__main__":
    main()
