#!/usr/bin/env python
"""Timing of the one-call inpainting route's image work (leftrefill_amd/refill.py) on both routes, and of the sampling between them.

    python tools/bench_refill.py [--size 512 --steps 50 --rounds 5 --no_sampling]      # -> profiles/refill_bench.json

Inputs: synthetic 3000 x 4000 source, mask and reference, `size` 512; decoding is excluded (the arrays are made in memory).
`prepare` + `finish` are timed on the host route (Pillow resizes + numpy, results uploaded / the prediction read back) and on the
device route (lr_pil_resize, lr_refill_canvas, lr_eval_metrics), alternating in one process; of the device route, packing the arena
and tables, the copies and the launches are timed separately.  `finish` gets a fixed random prediction.  The sampling between them
(conditioning, `steps` DDIM steps at guidance 2.5, the VAE decode) is timed on the synthetic model of the GPU tests (oracle MID UNet,
the open_clip stand-in), which only says how small the image work is beside it.  No threshold is asserted.
"""
import argparse
import json
import os
import statistics
import sys
import tempfile
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from leftrefill_amd import refill as R  # noqa: E402


def inputs(h=3000, w=4000, seed=0):
    rng = np.random.RandomState(seed)
    small = rng.randint(0, 256, (h // 8, w // 8, 3), dtype=np.uint8)
    source = np.ascontiguousarray(np.repeat(np.repeat(small, 8, axis=0), 8, axis=1))
    source[::3, ::5] ^= 0x55
    reference = np.ascontiguousarray(source[::-1, ::-1])
    mask = np.zeros((h, w, 3), np.uint8)
    mask[h // 4:h // 2, w // 5:w // 2] = 255
    mask[h // 2:h // 2 + 40, :] = 255
    return source, mask, reference


def synthetic_model(size):
    """The model of tests/test_gpu_refill.py: oracle MID UNet, a small VAE, the prompt embedder on the open_clip stand-in."""
    import yaml
    from oracle import clip_stub, golden_spec as G
    sys.modules.setdefault("open_clip", clip_stub)
    import leftrefill_amd.dropin as dropin
    dropin.install()
    from inpainting_ldm.model import create_model
    dd = dict(double_z=True, z_channels=4, resolution=size, in_channels=3, out_ch=3, ch=64, ch_mult=[1, 2, 4, 4], num_res_blocks=1,
              attn_resolutions=[], dropout=0.0)
    model = {"target": "inpainting_ldm.ref_inpainting_ldm.RefInpaintLDM", "params": dict(
        linear_start=0.00085, linear_end=0.0120, timesteps=1000, first_stage_key="image", cond_stage_key="txt", channels=4,
        cond_stage_trainable=True, conditioning_key="hybrid", scale_factor=0.18215,
        data_config={"img_size": size, "repeat_sp_token": 4, "sp_token": "<special-token>"},
        unet_config={"target": "ldm.modules.diffusionmodules.openaimodel.UNetModel", "params": G.CONFIGS["MID"].kwargs()},
        first_stage_config={"target": "ldm.models.autoencoder.AutoencoderKL",
                            "params": {"ddconfig": dd, "embed_dim": 4, "lossconfig": {"target": "torch.nn.Identity"}}},
        cond_stage_config={"target": "ldm.modules.encoders.Refill_modules.PromptCLIPEmbedder",
                           "params": dict(freeze=True, layer="penultimate", special_tokens=["repeat_4_<special-token>"],
                                          init_text=["reference on the left target on the right"])})}
    with tempfile.TemporaryDirectory() as d:
        path = os.path.join(d, "model_config.yaml")
        with open(path, "w") as f:
            yaml.safe_dump({"model": model}, f)
        m = create_model(path)
    sd = {"model.diffusion_model." + k: v for k, v in G.unet_state("MID").items()}
    m.load_state_dict(sd, strict=False)
    return m.to("cuda").eval()


def ms(fn, sync=True):
    if sync:
        torch.cuda.synchronize()
    t = time.perf_counter()
    out = fn()
    if sync:
        torch.cuda.synchronize()
    return (time.perf_counter() - t) * 1e3, out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--size", type=int, default=512)
    ap.add_argument("--steps", type=int, default=50)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--no_sampling", action="store_true")
    ap.add_argument("--out", type=str, default=os.path.join(ROOT, "profiles", "refill_bench.json"))
    a = ap.parse_args()
    dev = torch.device("cuda")
    source, mask, reference = inputs()
    p = R.plan(source.shape[:2], a.size)
    H, W = p["H"], p["W"]
    pred = torch.from_numpy(np.random.RandomState(1).rand(1, 3, H, 2 * W).astype(np.float32) * 2.4 - 1.2).to(dev).half()

    def host_prepare():
        parts = R.prepare_numpy(source, mask, reference, a.size, 1, resize=R.resize_pil)
        return tuple(torch.from_numpy(x).to(dev) for x in parts)

    def host_finish(image, m):
        return R.finish_numpy(pred.float().cpu().numpy(), image.cpu().numpy(), m.cpu().numpy(), p["out_wh"], resize=R.resize_pil)

    def dev_prepare(timing=None):
        return R.prepare_device([source], [mask], [reference], a.size, 1, dev, timing)

    def dev_finish(image, m, timing=None):
        return R.finish_device(pred, image, m, [p["out_wh"]], timing)

    # warm-up and agreement
    hi = host_prepare()
    di = dev_prepare()
    agree = all(torch.equal(x, y) for x, y in zip(hi, di))
    agree = agree and np.array_equal(host_finish(hi[0], hi[2])[0], dev_finish(di[0], di[2])[0])
    rows = dict(host_prepare_ms=[], host_finish_ms=[], device_prepare_ms=[], device_finish_ms=[], device_pack_ms=[], device_copy_ms=[],
                device_launch_ms=[])
    for _ in range(a.rounds):      # alternating, one process
        t, hi = ms(host_prepare)
        rows["host_prepare_ms"].append(t)
        rows["host_finish_ms"].append(ms(lambda: host_finish(hi[0], hi[2]))[0])
        t, di = ms(dev_prepare)
        rows["device_prepare_ms"].append(t)
        rows["device_finish_ms"].append(ms(lambda: dev_finish(di[0], di[2]))[0])
        timing = {}
        t1, di = ms(lambda: dev_prepare(timing))
        t2, _ = ms(lambda: dev_finish(di[0], di[2], timing))
        rows["device_pack_ms"].append(timing["pack"] * 1e3)
        rows["device_copy_ms"].append(timing["copy"] * 1e3)
        rows["device_launch_ms"].append(t1 + t2 - (timing["pack"] + timing["copy"]) * 1e3)      # launches, the 8-bit read-back included
    result = {
        "config": f"one pair, synthetic 3000 x 4000 source, mask and reference, size {a.size} (canvas {H} x {2 * W}), result "
                  f"{p['out_wh'][0]} x {p['out_wh'][1]}; decoding excluded on both routes",
        "timing": f"one process, {a.rounds} rounds alternating host and device route, wall clock around synchronised calls, medians; "
                  "pack / copy / launch: a separate device call per round with a synchronisation after the copies "
                  "(launch = the rest of the call: kernels, allocations, the result's read-back)",
        "gpu": torch.cuda.get_device_name(0), "host_cpus": os.cpu_count(),
        "agrees_with_host_bit_for_bit": bool(agree),
        "arena_bytes": int(source.nbytes + mask.nbytes + reference.nbytes),
    }
    for k, v in rows.items():
        result[k] = round(statistics.median(v), 3)
        result[k + "_all"] = [round(x, 3) for x in v]
    if not a.no_sampling:
        model = synthetic_model(a.size)
        with torch.no_grad(), torch.autocast("cuda"):
            run = lambda steps: R.sample_latents(model, di[0], di[1], di[2], R.prompt(4), steps, 2.5, [0], 1)
            run(2)      # warm-up: plans, buffers
            result["sampling_ms"] = round(ms(lambda: run(a.steps))[0], 1)
        result["sampling_note"] = f"conditioning + {a.steps} DDIM steps at guidance 2.5 + decode, synthetic model (oracle MID UNet), same process"
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(result, f, indent=1)
        f.write("\n")
    print(json.dumps(result))


if __name__ == "__main__":
    main()
