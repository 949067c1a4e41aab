#!/usr/bin/env python
"""Evaluation harness with the CLI and call sequence of the reference's test_inpainting.py (56-205), against the drop-in API.

    python tools/run_inpainting.py --model_path check_points/ref_guided_inpainting --cfg 2.5 --eta 1.0 [--test_path DIR]

Call sequence reproduced (reference line numbers): create_model(model_config.yaml).cpu() (82) -> load newest
ckpts/epoch=*.ckpt, then pretrained_models/512-inpainting-ema.ckpt when `save_prompt_only` (84-97) -> .to("cuda").eval()
(102-103) -> no_grad + autocast (126) -> model.log_images(batch, N, unconditional_guidance_scale=cfg, ddim_eta=eta) (141)
-> pred*mask + origin*(1-mask) (146-147) -> keep the right half (148-150) -> PSNR on (x+1)/2 (158), SSIM on the luma (160-162)
-> PNG (168-190).  LPIPS (159): `--lpips_weights alexnet-owt.pth,lpips_alex.pth` (torchvision's AlexNet + the lpips package's
v0.1 linear layers, or one state dict of `lpips.LPIPS(net='alex')`) feeds `evalglue.LPIPSAlex`; without the files (none ship:
no network) the metric is reported as not computed.

--test_path DIR is read through `dataloaders.test_dataset.TestInpaintingDataset` (drop-in of the reference loader: pair
directories with source / target / mask files) and torch's DataLoader, exactly like the reference (118-120).  Without it
(no dataset ships with the reference) `--synthetic N` builds N batches with the same batch contract
(dataloaders/test_dataset.py:91-105): image [B,512,1024,3] in [-1,1] (left reference | right target), mask [B,512,1024,1]
(left half 0), masked_image = image*(mask<0.5), txt = "<special-token0> ... <special-token49>".

--multiview: the call sequence of the reference's test_multiview_inpainting.py (77-233) for the multi-view task model
(inpainting_ldm.multiview_ref_inpainting_ldm.RefInpaintLDM over MultiViewUnetModel): 5-D batches [B, v, H, W, 3], log_images samples all
(b v) canvases jointly and returns the target view; the mask of canvas 0 of every sample pastes the known pixels back, a
[reference | target] canvas keeps its target half (`evalglue.compose_prediction_multiview`, reference 141-170).  --test_path DIR is read
through `leftrefill_amd.dropin.dataloaders.inpainting_crossview_dataset.InpaintingMultiViewDataset` in `val` mode, built as the reference builds
it (test_multiview_inpainting.py:111-114: folders named by a number with target / source / source_1.. and mask.png; `test_limit`
482); without it the mode runs on `--synthetic N` batches with that batch contract: one prompt list per view, txt[view][batch].

--device_metrics: PSNR, SSIM, the finite check and the PNG's bytes come from one HIP kernel pass per batch
(`evalglue.device_metrics*`, read back once) in place of the eager composite / crop / interpolate / psnr01 launches, the fp32
read-backs and the per-image float64 scipy SSIM on the host; printed lines, metric file and PNG names are the same.  It needs an
integer --test_size / --metric_size ratio.

--device_prep (with --test_path): the loader only decodes; area resize, the [source | target] canvas, the mask (thresholded at > 127: a
{0, 255} mask file gives the same mask) and the [-1, 1] mapping of a batch are one launch of csrc/batch_prep.hip -- under --multiview
all B x V canvases of a batch in that one launch.

--device_lpips (with --device_metrics and --lpips_weights): the LPIPS line comes from `evalglue.DeviceLPIPS.score*` -- the HIP AlexNet
of csrc/lpips.hip on the whole batch, the composite formed inside its first convolution -- and joins the batch's one read-back; the
torch composite and the per-sample eager module are not run.  Same printed lines and metric file.

--fid_weights FILE (a state dict of pytorch-fid's / torchvision's Inception network; none ships): a final `FID:` line in the printout
and the metric file -- the Frechet Inception Distance between the composited predictions and the originals, both as the 8-bit images the
reference writes to disk "for fid metric" (`leftrefill_amd.fid`, parity-unpinned).  --device_fid routes the network and the float64
statistics through the HIP kernels of csrc/inception.hip (`fid.DeviceFID`); without it `fid.HostFID` runs the eager network in fp32.
Without --fid_weights nothing changes.

--seeded_noise [--seed N]: every random draw of an item -- the posterior sample of its masked-image encoding, its start code, the noise
of every sampler step -- comes from the item's own key (N, dataset index of the item) of leftrefill_amd/noise.py (under --multiview one
key per canvas: sub = index * views + view) instead of torch's global generators, so the images and the printed metrics do not depend
on --batch_size or on what ran before, up to the UNet's batch-dependent kernel plans.  Without it nothing changes.
"""
import argparse
import glob
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def synthetic_batches(n, batch_size, size, sp_token="<special-token>", repeat=50, seed=0):
    g = torch.Generator().manual_seed(seed)
    txt = " ".join(f"{sp_token[:-1]}{i}>" for i in range(repeat))
    for _ in range(n):
        img = torch.rand(batch_size, size, 2 * size, 3, generator=g) * 2 - 1
        mask = torch.zeros(batch_size, size, 2 * size, 1)
        blocks = (torch.rand(batch_size, size // 32, size // 32, 1, generator=g) < 0.5).float()
        mask[:, :, size:, :] = blocks.repeat_interleave(32, 1).repeat_interleave(32, 2)
        yield {"image": img, "mask": mask, "masked_image": img * (mask < 0.5), "txt": [txt] * batch_size}


def synthetic_mv_batches(n, batch_size, size, views, concat, view_token_len, sp_token="<special-token>", repeat=50, seed=0):
    """Multi-view batches: `views` canvases per sample; concat_target: canvas i = [reference_i | target] (size x 2 size), the mask marks a
    block pattern inside the target half; otherwise square views, view 0 is the (masked) target."""
    g = torch.Generator().manual_seed(seed)
    base = " ".join(f"{sp_token[:-1]}{i}>" for i in range(repeat))
    txt = [[base + " " + " ".join(f"<view_direct-{j}-{l}" for l in range(view_token_len))] * batch_size for j in range(views)]
    wc = 2 * size if concat else size
    for _ in range(n):
        img = torch.rand(batch_size, views, size, wc, 3, generator=g) * 2 - 1
        if concat:
            img[:, :, :, size:] = img[:, :1, :, size:]        # every canvas carries the same target on its right half
        mask = torch.zeros(batch_size, views, size, wc, 1)
        blocks = (torch.rand(batch_size, size // 32, size // 32, 1, generator=g) < 0.5).float()
        blocks[:, 0, 0] = 1.0                                 # never an empty mask (a tiny --test_size has only a few blocks)
        blocks = blocks.repeat_interleave(32, 1).repeat_interleave(32, 2)
        if concat:
            mask[:, :, :, size:, :] = blocks[:, None]
        else:
            mask[:, 0] = blocks
        yield {"image": img, "mask": mask, "masked_image": img * (mask < 0.5), "txt": [list(t) for t in txt]}


def dataset_batches(path, batch_size, size, model, device_prep=False):
    """The reference's loader + DataLoader (test_inpainting.py:118-120), through the subclass that adds the `raw` keyword (its default
    items are that loader's).  device_prep: items are (plan, raw) and the [source | target] canvases of a batch are assembled by one
    HIP kernel launch (leftrefill_amd/dataprep.py)."""
    from dataloaders.raw_pairs import TestInpaintingDataset
    from leftrefill_amd import rawbatch
    cond_cfg = getattr(model, "cond_cfg", None) or {}
    data_cfg = dict(getattr(model, "data_cfg", None) or {})
    data_cfg.pop("img_size", None)
    ds = TestInpaintingDataset(path, img_size=size, deep_prompt=cond_cfg.get("deep_prompt", False), raw=device_prep, **data_cfg)
    return rawbatch.loader(ds, device_prep, "cuda", batch_size=batch_size, shuffle=False)


def multiview_batches(path, batch_size, size, model, device_prep=False):
    """The reference's multi-view loader + DataLoader (test_multiview_inpainting.py:111-114); device_prep as in `dataset_batches`, with
    one tile per view, or two under concat_target."""
    from leftrefill_amd import rawbatch
    from leftrefill_amd.dropin.dataloaders.inpainting_crossview_dataset import InpaintingMultiViewDataset
    data_cfg = dict(getattr(model, "data_cfg", None) or {}, test_limit=482)
    data_cfg.pop("img_size", None)
    ds = InpaintingMultiViewDataset(path, img_size=size, pair_path=None, mask_path=path, mode="val", raw=device_prep,
                                    deep_prompt=(getattr(model, "cond_cfg", None) or {}).get("deep_prompt", False), **data_cfg)
    bad = [p for p in ds.pairs if not (os.path.basename(p).isdigit() and glob.glob(os.path.join(p, "target.*")))]
    if bad or not len(ds):      # refused, not skipped: a wrong folder must not score a subset
        raise SystemExit(f"--multiview --test_path {path}: {len(bad)} of {len(ds)} entries are no multi-view folders (named by a number, "
                         f"holding target / source / source_1.. images and mask.png), e.g. {bad[:1]}; without a dataset, --synthetic N "
                         "builds batches of the same contract")
    return rawbatch.loader(ds, device_prep, "cuda", batch_size=batch_size, shuffle=False)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--model_path", type=str, required=True)
    ap.add_argument("--batch_size", type=int, default=1)
    ap.add_argument("--test_path", type=str, default=None)
    ap.add_argument("--cfg", type=float, default=2.5)
    ap.add_argument("--test_size", type=int, default=512)
    ap.add_argument("--metric_size", type=int, default=512)
    ap.add_argument("--eta", type=float, default=1.0)
    ap.add_argument("--output_path", type=str, default="outputs")
    ap.add_argument("--metric_output", type=str, default="metric_outputs")
    ap.add_argument("--ngpu", type=int, default=1)       # parsed but unused, like the reference (62, 99)
    ap.add_argument("--fp16", action="store_true")       # idem (63)
    ap.add_argument("--sampler", type=str, default="ddim", choices=["ddim", "plms", "dpm_solver", "ddpm"],
                    help="plms needs --eta 0; dpm_solver ignores eta (reference dpm_solver/sampler.py); ddpm: ancestral, full "
                         "schedule, needs a guidance scale of 1")
    ap.add_argument("--steps", type=int, default=50, help="sampler steps (the reference's log_images default: 50)")
    ap.add_argument("--synthetic", type=int, default=0)
    ap.add_argument("--pretrained", type=str, default="pretrained_models/512-inpainting-ema.ckpt")
    ap.add_argument("--lpips_weights", type=str, default=None, help="comma-separated state-dict files for LPIPS(alex)")
    ap.add_argument("--multiview", action="store_true", help="multi-view task model: the call sequence of test_multiview_inpainting.py")
    ap.add_argument("--device_metrics", action="store_true", help="score on the device: PSNR / SSIM / finite check / PNG bytes from one HIP kernel")
    ap.add_argument("--device_prep", action="store_true", help="assemble the --test_path batches on the device from raw decoded images")
    ap.add_argument("--device_lpips", action="store_true", help="LPIPS from the HIP kernels (needs --device_metrics and --lpips_weights)")
    ap.add_argument("--fid_weights", type=str, default=None, help="state-dict file of the FID Inception network: adds the FID line")
    ap.add_argument("--device_fid", action="store_true", help="FID features and statistics from the HIP kernels (needs --fid_weights)")
    ap.add_argument("--seeded_noise", action="store_true", help="per-item seeded noise: results do not depend on --batch_size")
    ap.add_argument("--seed", type=int, default=0, help="the seed of --seeded_noise; an item's key is (seed, its dataset index)")
    a = ap.parse_args()
    if a.device_fid and not a.fid_weights:
        raise SystemExit("--device_fid requires --fid_weights")
    if a.device_lpips and not (a.device_metrics and a.lpips_weights):
        raise SystemExit("--device_lpips requires --device_metrics and --lpips_weights")

    import leftrefill_amd.dropin as dropin
    dropin.install()
    from inpainting_ldm.model import create_model, load_state_dict
    from leftrefill_amd import evalglue

    model = create_model(os.path.join(a.model_path, "model_config.yaml")).cpu()
    ckpts = sorted(glob.glob(os.path.join(a.model_path, "ckpts", "epoch=*.ckpt")), key=os.path.getmtime)
    if ckpts:
        print(model.load_state_dict(load_state_dict(ckpts[-1]), strict=False))
    if getattr(model, "save_prompt_only", False) and os.path.exists(a.pretrained):
        print(model.load_state_dict(load_state_dict(a.pretrained), strict=False))
    model = model.to("cuda").eval()
    os.makedirs(a.output_path, exist_ok=True)
    if a.multiview and a.test_path:
        batches = multiview_batches(a.test_path, a.batch_size, a.test_size, model, a.device_prep)
    elif a.multiview:
        concat = bool(getattr(model, "concat_target", False))
        views = model.view_num - 1 if concat else model.view_num
        vlen = int((getattr(model, "cond_cfg", None) or {}).get("view_token_len", 0)) if (getattr(model, "cond_cfg", None) or {}).get("view_prompt", True) else 0
        dc = getattr(model, "data_cfg", None) or {}
        batches = synthetic_mv_batches(max(1, a.synthetic), a.batch_size, a.test_size, views, concat, vlen,
                                       sp_token=dc.get("sp_token", "<special-token>"), repeat=int(dc.get("repeat_sp_token", 50)))
    else:
        batches = dataset_batches(a.test_path, a.batch_size, a.test_size, model, a.device_prep) if a.test_path else \
            synthetic_batches(max(1, a.synthetic), a.batch_size, a.test_size)
    global_view_num = 0
    lpips_fn = None
    if a.lpips_weights:
        lpips_fn = (evalglue.DeviceLPIPS if a.device_lpips else evalglue.LPIPSAlex)().load_weights(*[torch.load(f, map_location="cpu") for f in a.lpips_weights.split(",")]).cuda()
    fid_fn = None
    if a.fid_weights:
        from leftrefill_amd import fid
        fid_fn = (fid.DeviceFID if a.device_fid else fid.HostFID)().load_weights(torch.load(a.fid_weights, map_location="cpu")).cuda()

    def fid_update(out, mask, view_num):      # one more pass over what the batch's metrics scored; nothing is read back here
        with torch.autocast("cuda", enabled=False):
            if a.multiview:
                fid_fn.update_multiview(out, mask, a.batch_size, view_num)
            else:
                fid_fn.update(out, mask)

    psnrs, ssims, lpipss = [], [], []
    items_seen = 0
    with torch.no_grad(), torch.autocast("cuda"):
        for bi, batch in enumerate(batches):
            batch = {k: (v.cuda() if torch.is_tensor(v) else v) for k, v in batch.items()}
            seeded = {}
            if a.seeded_noise:      # one key per canvas, named by the item's place in the dataset (the loaders do not shuffle)
                from leftrefill_amd.noise import SeededNoise
                img = batch["image"]
                per_item = img.shape[1] if img.dim() == 5 else 1
                subs = [(items_seen + j) * per_item + v_ for j in range(img.shape[0]) for v_ in range(per_item)]
                seeded = {"seeds": SeededNoise([a.seed] * len(subs), subs=subs, device=img.device)}
                items_seen += img.shape[0]
            out = model.log_images(batch, batch["image"].shape[0], unconditional_guidance_scale=a.cfg, ddim_eta=a.eta,
                                       ddim_steps=a.steps, **({} if a.sampler == "ddim" else {"sampler": a.sampler}), **seeded)
            if a.device_metrics:
                if a.multiview:
                    m, global_view_num = evalglue.device_metrics_multiview(out, batch["mask"], a.batch_size, global_view_num, a.test_size,
                                                                           a.metric_size, want_rgb8=True)
                else:
                    m = evalglue.device_metrics(out, batch["mask"], test_size=a.test_size, metric_size=a.metric_size, want_rgb8=True)
                if fid_fn is not None:
                    fid_update(out, batch["mask"], global_view_num)
                rows = [m["psnr"], m["ssim"], m["nonfinite"]]
                if a.device_lpips:      # one more kernel call on the same tensors, one more row of the same read-back
                    if a.multiview:
                        rows.append(lpips_fn.score_multiview(out, batch["mask"], a.batch_size, global_view_num, a.test_size, a.metric_size)[0])
                    else:
                        rows.append(lpips_fn.score(out, batch["mask"], test_size=a.test_size, metric_size=a.metric_size))
                psnr_b, ssim_b, bad_b, *lp_b = torch.stack(rows).tolist()      # the batch's one read-back
                if lp_b:
                    lpipss.extend(lp_b[0])
                if sum(bad_b):
                    scored = m["rgb8"].numel() * (a.test_size // a.metric_size if a.metric_size < a.test_size else 1) ** 2
                    print(f"WARNING: {100 * sum(bad_b) / scored:.2f} % of the decoded prediction is not finite (batch {bi})")
                psnrs.extend(psnr_b)
                ssims.extend(ssim_b)
                if lpips_fn is not None and not a.device_lpips:      # the eager module gets the torch composite
                    if a.multiview:
                        pred, origin, _ = evalglue.compose_prediction_multiview(out, batch["mask"], a.batch_size, global_view_num,
                                                                                a.test_size, a.metric_size)
                    else:
                        pred, origin = evalglue.compose_prediction(out, batch["mask"], a.test_size, a.metric_size)
                    with torch.autocast("cuda", enabled=False):
                        lpipss.extend(lpips_fn(pred.float(), origin.float()).flatten().tolist())
                try:
                    from PIL import Image
                    for j, arr in enumerate(m["rgb8"].cpu().numpy()):
                        Image.fromarray(arr).save(os.path.join(a.output_path, f"{bi:04d}_{j}.png"))
                except ImportError:
                    pass
                continue
            if not torch.isfinite(out["pred"]).all():
                bad = (~torch.isfinite(out["pred"])).float().mean().item()
                print(f"WARNING: {100 * bad:.2f} % of the decoded prediction is not finite (batch {bi})")
            if a.multiview:      # batch["mask"] was flattened to (b v) canvases by log_images, like the reference (100-105)
                pred, origin, global_view_num = evalglue.compose_prediction_multiview(out, batch["mask"], a.batch_size, global_view_num,
                                                                                      a.test_size, a.metric_size)
            else:
                pred, origin = evalglue.compose_prediction(out, batch["mask"], a.test_size, a.metric_size)
            if fid_fn is not None:
                fid_update(out, batch["mask"], global_view_num)
            psnrs.extend(evalglue.psnr01(pred, origin).tolist())
            if lpips_fn is not None:
                with torch.autocast("cuda", enabled=False):
                    lpipss.extend(lpips_fn(pred.float(), origin.float()).flatten().tolist())   # LPIPS takes [-1, 1] (159)
            for j in range(pred.shape[0]):
                ssims.append(evalglue.ssim_gray(evalglue.rgb_to_gray01(pred[j]), evalglue.rgb_to_gray01(origin[j])))
            p01 = (pred.float().clamp(-1, 1) + 1) / 2
            try:
                from PIL import Image
                for j in range(p01.shape[0]):
                    arr = (p01[j].permute(1, 2, 0).cpu().numpy() * 255).astype(np.uint8)
                    Image.fromarray(arr).save(os.path.join(a.output_path, f"{bi:04d}_{j}.png"))
            except ImportError:
                pass
    print(f"PSNR: {float(np.mean(psnrs)):.3f} over {len(psnrs)} images")
    print(f"SSIM: {float(np.mean(ssims)):.4f}")
    lp = f"{float(np.mean(lpipss)):.4f}" if lpipss else "not computed (no --lpips_weights)"
    print(f"LPIPS: {lp}")
    fid_line = f"FID: {fid_fn.compute():.4f}\n" if fid_fn is not None else ""
    print(fid_line, end="")
    os.makedirs(a.metric_output, exist_ok=True)
    with open(os.path.join(a.metric_output, os.path.basename(os.path.normpath(a.model_path)) + ".txt"), "w") as f:
        f.write(f"PSNR: {float(np.mean(psnrs)):.4f}\nSSIM: {float(np.mean(ssims)):.4f}\nLPIPS: {lp}\n" + fid_line)


if __name__ == "__main__":
    main()
