#!/usr/bin/env python
"""Reference-guided inpainting of one photo from the command line: `predict` of the reference's ref_inpainting_gradio.py (148-211)
without the UI, through `leftrefill_amd.refill.refill`.

    python tools/refill.py --model_path check_points/ref_guided_inpainting --source photo.png --mask mask.png --reference ref.png \
        --out outputs [--steps 50 --scale 2.5 --seed 0 --num_samples 1 --size 512] [--host_prep] [--attn_maps DIR]

The model is loaded the way tools/run_inpainting.py loads it: create_model(model_config.yaml), the newest ckpts/epoch=*.ckpt, then
--pretrained when the model saves its prompt only.  The mask is white where the source is to be filled.  Writes out_00.png ...
out_{num_samples - 1}.png of size (int(size / ratio), size) into --out.  The resizes, the canvas and the 8-bit tail run as HIP kernels;
--host_prep runs them on the host with Pillow and numpy instead and writes the same bytes.  The seed fixes the start code and
torch's generators (the VAE posterior sample and the eta = 1 noise draw from those).  --seeded_noise: every draw of sample j comes
from the key (seed, j) of leftrefill_amd/noise.py instead (`refill(noise="seeded")`): the result depends on the inputs and the seed alone.
--attn_maps DIR: also writes, per output image XX and self-attention layer YY of the UNet, attn_XX_lYY.png (viridis over [0, 1] of how
much each target token attends to the reference, nearest-resized to the result's size) and corr_XX_lYY.npy ([h, w / 2, 2] float32: the
reference-half token (x, y) each target token looks at; leftrefill_amd.attnprobe).
"""
import argparse
import glob
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def write_attn_maps(out_dir, images, attn, size):
    """attn_XX_lYY.png / corr_XX_lYY.npy for every output image XX and layer YY (see the module docstring).  The maps cover the padded
    target half of the canvas; the result shows its top-left size x size pixels, so the maps are cut to that share first."""
    import numpy as np
    import torch.nn.functional as F
    from matplotlib import cm
    from PIL import Image
    os.makedirs(out_dir, exist_ok=True)
    side = max(2, -(-size // 64)) * 64      # leftrefill_amd.refill.plan
    for l, (mass, corr) in enumerate(zip(attn["mass"], attn["correspondence"])):
        kh, kw = max(1, round(mass.shape[1] * size / side)), max(1, round(mass.shape[2] * size / side))
        mass, corr = mass[:, :kh, :kw], corr[:, :kh, :kw]
        for i, im in enumerate(images):
            m = F.interpolate(mass[i:i + 1, None].float(), size=[im.size[1], im.size[0]], mode="nearest")[0, 0].clamp(0, 1).cpu().numpy()
            Image.fromarray((cm.viridis(m)[:, :, :3] * 255).astype(np.uint8)).save(os.path.join(out_dir, f"attn_{i:02d}_l{l:02d}.png"))
            np.save(os.path.join(out_dir, f"corr_{i:02d}_l{l:02d}.npy"), corr[i].float().cpu().numpy())


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--model_path", type=str, required=True)
    ap.add_argument("--source", type=str, required=True)
    ap.add_argument("--mask", type=str, required=True)
    ap.add_argument("--reference", type=str, required=True)
    ap.add_argument("--out", type=str, default="outputs")
    ap.add_argument("--steps", type=int, default=50)
    ap.add_argument("--scale", type=float, default=2.5)
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--num_samples", type=int, default=1)
    ap.add_argument("--size", type=int, default=512)
    ap.add_argument("--host_prep", action="store_true", help="image work on the host with Pillow and numpy (the yardstick route)")
    ap.add_argument("--pretrained", type=str, default="pretrained_models/512-inpainting-ema.ckpt")
    ap.add_argument("--seeded_noise", action="store_true", help="per-sample seeded noise for every draw (refill(noise='seeded'))")
    ap.add_argument("--attn_maps", type=str, default=None, help="directory for the reference-attention maps (attn_XX_lYY.png, corr_XX_lYY.npy)")
    a = ap.parse_args()

    import torch
    from PIL import Image

    import leftrefill_amd.dropin as dropin
    dropin.install()
    from inpainting_ldm.model import create_model, load_state_dict
    from leftrefill_amd.refill import refill

    model = create_model(os.path.join(a.model_path, "model_config.yaml")).cpu()
    ckpts = sorted(glob.glob(os.path.join(a.model_path, "ckpts", "epoch=*.ckpt")), key=os.path.getmtime)
    if ckpts:
        print(model.load_state_dict(load_state_dict(ckpts[-1]), strict=False))
    if getattr(model, "save_prompt_only", False) and os.path.exists(a.pretrained):
        print(model.load_state_dict(load_state_dict(a.pretrained), strict=False))
    model = model.to("cuda").eval()
    torch.manual_seed(a.seed)
    images = refill(model, Image.open(a.source), Image.open(a.mask), Image.open(a.reference), steps=a.steps, scale=a.scale, seed=a.seed,
                    num_samples=a.num_samples, size=a.size, device_prep=not a.host_prep, return_attn=a.attn_maps is not None,
                    noise="seeded" if a.seeded_noise else "torch")
    if a.attn_maps is not None:
        images, attn = images
        write_attn_maps(a.attn_maps, images, attn, a.size)
    os.makedirs(a.out, exist_ok=True)
    for i, im in enumerate(images):
        path = os.path.join(a.out, f"out_{i:02d}.png")
        im.save(path)
        print(path, im.size)


if __name__ == "__main__":
    main()
