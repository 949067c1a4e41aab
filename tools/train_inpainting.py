#!/usr/bin/env python
"""Prompt tuning from the command line: the flags and the flow of the reference's train_inpainting.py on leftrefill_amd.trainer.Trainer.

    python tools/train_inpainting.py --config_file configs/training.yaml --exp_name my_run --fp16 --synthetic 200
    python tools/train_inpainting.py --config_file ... --exp_name my_run --fp16 --dataset mypkg.data:TrainSet

The training config names `model_config`, `resume_path` (backbone weights), `optim_cfg`, `max_steps`, `accumulate_grad_batches`
and `batch_size`, as the reference's check_points/*/training_config.yaml does.  Checkpoints go to
<save_path>/<exp_name>/ckpts/last.ckpt; --restore continues from it (the default when it exists, unless --no_restore).

Data: --dataset crossview builds what the shipped prompt tokens were trained on: `leftrefill_amd.dropin.dataloaders.inpainting_crossview_dataset.
InpaintingCrossViewDataset` over the config's `image_path` (the image dictionary), `train_pair` and `train_mask_path` and the model's
data section ([reference | target] canvases, view masks, matching-based masks, ...), drawn by `BalancedRandomSampler`
(`n_sample_per_scene` pairs of every scene per epoch, this rank's share; the trainer's epoch hook reseeds it) -- the model's own
`train_dataloader` / `val_dataloader`, as in the reference.  --dataset inpainting builds the `dataloaders.inpainting_dataset.
InpaintingDataset` drop-in (the reference's single-image training set) from the config's `image_path` and `train_mask_path` (the
irregular and the segmentation mask list) and the model's data section; --dataset module:Class builds `Class(**data_cfg)`;
--synthetic N trains on N generated batches with the evaluation harness' batch contract (tools/run_inpainting.py).
--dataset objaverse builds the Objaverse novel-view dataset (`leftrefill_amd.dropin.dataloaders.obj_nvs_dataset.NVS_OBJDataset`) for an
`NVSLDM` model config from the training config's `datapath`, `train_list`, `val_list` and `batch_size` and the model's data section --
the model's own `train_dataloader` / `val_dataloader`; with --device_prep a batch of raw RGBA renders is finished by one
`lr_nvs_prep` launch (leftrefill_amd/nvsprep.py, csrc/nvs_prep.hip).
--device_prep (with --dataset inpainting | crossview | objaverse): the loader's workers only decode and plan; resize, crop, flips, masks and the
[-1, 1] mapping of a whole batch are one HIP kernel launch (leftrefill_amd/dataprep.py, csrc/batch_prep.hip).
--val (with --dataset inpainting | crossview | objaverse): the `val`-mode dataset over `val_image_path` / `val_mask_path` (objaverse: `val_list`;`test_limit` images,
batches of `val_batch_size`, default 4; `test_limit` from the model's data section, else the training config) is validated every
`val_check_interval` steps (a fraction: of an epoch) and its metrics printed.  With --synthetic N, --val scores the first generated batch.
The reference's callbacks (train_inpainting.py:93-138) come from the training config: `logger_freq` adds the image logger
(`inpainting_ldm.logger.InpaintingLogger`: a JPEG grid masked_image | origin_image | pred of the current batch every `logger_freq`
batches under <save_path>/<exp_name>/samples/train/, sampled at the model's `cfg`, and the drift of every learned token; --no_image_log
leaves it out), `save_top_k` adds `leftrefill_amd.trainer.ModelCheckpoint` on `val/<monitor>` (`monitor`, default lpips; `monitor_mode`,
default min) writing ckpts/epoch={e}-step={s}.ckpt next to last.ckpt; either adds the learning-rate monitor.  Without these keys nothing
changes.
"""
import argparse
import importlib
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def record_draws(sampler):
    """Every epoch's indices as the sampler hands them out from now on, one list per epoch, appended to the returned list."""
    epochs, draw = [], type(sampler).__iter__

    class Recording(type(sampler)):
        def __iter__(self):
            epochs.append(list(draw(self)))
            return iter(epochs[-1])

    sampler.__class__ = Recording
    return epochs


def model_loaders(config, model, device_prep, val, workers, device, items):
    """(training batches, validation batches or None) from the model's own train_dataloader / val_dataloader (reference
    ref_inpainting_ldm.py:99-117, NVS_ldm.py:348-372); with device_prep they collate raw decoded images and the dataset's own device
    prep finishes the batches on `device` (leftrefill_amd/rawbatch.py).  items: what a validation item is called in a message."""
    loaders = [model.train_dataloader(raw=device_prep, num_workers=workers, device=device), None]
    if val:
        val_bs = int(config.get("val_batch_size", 4))
        loaders[1] = model.val_dataloader(raw=device_prep, num_workers=min(4, workers), batch_size=val_bs, device=device)
        if len(loaders[1]) == 0:      # drop_last (as the reference has it) would leave no batch and validation nothing to average
            raise SystemExit(f"--val: {len(loaders[1].dataset)} validation {items} are fewer than val_batch_size = {val_bs}")
    return loaders


def inpainting_loaders(config, model, batch_size, device_prep, val, workers, device):
    """(training batches, validation batches or None) of the single-image dataset, as the reference's train_dataloader builds it
    (ref_inpainting_ldm.py:109-111); with device_prep the loaders collate raw bytes and a DevicePrep per loader finishes the batches."""
    from dataloaders.inpainting_dataset import InpaintingDataset
    from leftrefill_amd import rawbatch
    data_cfg = dict(model.data_cfg)      # the reference's model configs carry `test_limit` here (ref_inpainting_ldm.py:109-117 pass it on)
    test_limit = int(data_cfg.pop("test_limit", config.get("test_limit", 200)))
    common = dict(img_size=int(model.img_size), raw=device_prep, test_limit=test_limit, **data_cfg)
    train = InpaintingDataset(image_list=config["image_path"], mask_path=list(config["train_mask_path"]), mode="train", **common)
    loaders = [rawbatch.loader(train, device_prep, device, batch_size=batch_size, shuffle=True, drop_last=True, num_workers=workers), None]
    if val:
        held = InpaintingDataset(image_list=config["val_image_path"], mask_path=config["val_mask_path"], mode="val", **common)
        val_bs = int(config.get("val_batch_size", 4))
        if len(held) < val_bs:      # drop_last (as the reference has it) would leave no batch and validation nothing to average
            raise SystemExit(f"--val: {len(held)} validation images are fewer than val_batch_size = {val_bs}")
        loaders[1] = rawbatch.loader(held, device_prep, device, batch_size=val_bs, shuffle=False, drop_last=True, num_workers=workers)
    return loaders


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--config_file", type=str, required=True)
    ap.add_argument("--exp_name", type=str, required=True)
    ap.add_argument("--save_path", type=str, default="./check_points")
    ap.add_argument("--ngpu", type=int, default=1)
    ap.add_argument("--fp16", action="store_true")
    ap.add_argument("--bf16", action="store_true", help="bfloat16 compute, no loss scale")
    ap.add_argument("--restore", action="store_true")
    ap.add_argument("--no_restore", action="store_true")
    ap.add_argument("--synthetic", type=int, default=0, help="train on N generated batches")
    ap.add_argument("--dataset", type=str, default=None, help="`crossview`, `inpainting`, `objaverse`, or module:Class of a map-style training dataset")
    ap.add_argument("--device_prep", action="store_true", help="assemble batches on the device from raw decoded images (--dataset inpainting | crossview | objaverse)")
    ap.add_argument("--val", action="store_true", help="validate on the config's val_image_path / val_mask_path, or val_list (--dataset inpainting | crossview | objaverse)")
    ap.add_argument("--num_workers", type=int, default=8, help="loader workers, at most 8")
    ap.add_argument("--seed", type=int, default=None, help="seed python's, numpy's and torch's generators")
    ap.add_argument("--log_every_n_steps", type=int, default=50)
    ap.add_argument("--loss_file", type=str, default=None, help="write every step's loss as a JSON list when the run ends")
    ap.add_argument("--index_file", type=str, default=None, help="write the sampler's indices, one list per epoch, as JSON when the run ends (--dataset crossview)")
    ap.add_argument("--hip_graph", action="store_true", help="replay the whole step as one hipGraph (fixed shapes)")
    ap.add_argument("--no_image_log", action="store_true", help="no sample grids even when the config has logger_freq")
    a = ap.parse_args()
    if (a.device_prep or (a.val and not a.synthetic)) and a.dataset not in ("inpainting", "crossview", "objaverse"):
        raise SystemExit("--device_prep and --val need --dataset inpainting, --dataset crossview or --dataset objaverse")
    if a.seed is not None:
        import random
        import numpy as np
        random.seed(a.seed)
        np.random.seed(a.seed)
        torch.manual_seed(a.seed)

    import leftrefill_amd.dropin as dropin
    dropin.install()
    from inpainting_ldm.model import create_model, load_config, load_state_dict
    from leftrefill_amd.trainer import LearningRateMonitor, ModelCheckpoint, Trainer
    from tools.run_inpainting import synthetic_batches

    rank = int(os.environ.get("LOCAL_RANK", 0))
    if a.ngpu > 1:
        torch.distributed.init_process_group("nccl")
    torch.cuda.set_device(rank)
    config = load_config(a.config_file)
    model = create_model(config["model_config"])
    if config.get("resume_path"):
        print(model.load_state_dict(load_state_dict(config["resume_path"]), strict=False))
    if hasattr(model, "lora_cfg"):      # after the base weights, before the optimizer (reference train_inpainting.py:71-72)
        model.set_lora()
    model.cfg, model.optim_cfg, model.world_size = config, config["optim_cfg"], a.ngpu
    model = model.to(f"cuda:{rank}")

    root = os.path.join(a.save_path, a.exp_name)
    last = os.path.join(root, "ckpts", "last.ckpt")
    resume = last if (a.restore or not a.no_restore) and os.path.exists(last) else None
    if a.restore and resume is None:
        raise FileNotFoundError(last)
    bs = int(config.get("batch_size", 1))
    # the reference's callbacks (train_inpainting.py:93-138), each behind its own config key: a config without them runs as before
    callbacks = []
    if "logger_freq" in config and not a.no_image_log:
        from inpainting_ldm.logger import InpaintingLogger
        callbacks.append(InpaintingLogger(batch_frequency=config["logger_freq"], save_dir=f"{a.exp_name}/samples",
                                          log_images_kwargs={"return_attn": config.get("return_attn", False),
                                                             "unconditional_guidance_scale": model.data_cfg["cfg"]}))
    if "save_top_k" in config:
        callbacks.append(ModelCheckpoint(f"{a.save_path}/{a.exp_name}/ckpts", config["save_top_k"], f"val/{config.get('monitor', 'lpips')}",
                                         config.get("monitor_mode", "min")))
    if callbacks:
        callbacks.append(LearningRateMonitor())
    trainer = Trainer(max_steps=int(config["max_steps"]), accumulate_grad_batches=int(config.get("accumulate_grad_batches") or 1),
                      log_every_n_steps=a.log_every_n_steps, precision=16 if a.fp16 else ("bf16" if a.bf16 else 32), default_root_dir=root,
                      resume_from_checkpoint=resume, hip_graph=a.hip_graph, local_rank=rank, callbacks=callbacks)
    trainer.logger.save_dir = a.save_path      # the reference's logger directory: samples land in <save_path>/<exp_name>/samples/<split>
    model.trainer = trainer      # the model's loaders read their rank here
    val_data = None
    workers = min(8, max(0, a.num_workers))
    if a.dataset == "crossview":      # the sampler takes rank and replica count from the model
        model.cfg = dict(config, cross_view_inpainting=True)
        data, val_data = model_loaders(config, model, a.device_prep, a.val, workers, f"cuda:{rank}", "pairs")
    elif a.dataset == "objaverse":      # over the config's `datapath`, `train_list`, `val_list` and `batch_size`
        if not hasattr(model, "_objaverse"):
            raise SystemExit("--dataset objaverse needs a model config whose target is inpainting_ldm.NVS_ldm.NVSLDM")
        data, val_data = model_loaders(config, model, a.device_prep, a.val, workers, f"cuda:{rank}", "objects")
    elif a.dataset == "inpainting":
        data, val_data = inpainting_loaders(config, model, bs, a.device_prep, a.val, workers, f"cuda:{rank}")
    elif a.dataset:
        mod, cls = a.dataset.split(":")
        data = torch.utils.data.DataLoader(getattr(importlib.import_module(mod), cls)(**dict(model.data_cfg)), batch_size=bs, shuffle=True,
                                           num_workers=8, drop_last=True)
    elif a.synthetic:
        data = list(synthetic_batches(a.synthetic, bs, int(model.img_size), seed=rank))
        if a.val:      # no held-out set to generate: the first generated batch is scored
            val_data = data[:1]
    else:
        raise SystemExit("give --synthetic N, --dataset crossview, --dataset inpainting, --dataset objaverse or --dataset module:Class")
    drawn = record_draws(data.sampler) if a.index_file and a.dataset == "crossview" else None
    if val_data is not None:
        every = config.get("val_check_interval", 1.0)
        trainer.val_check_interval = max(1, int(every * len(data))) if isinstance(every, float) else int(every)
    trainer.fit(model, data, val_data)
    if a.loss_file and rank == 0:
        import json
        with open(a.loss_file, "w") as f:
            json.dump(torch.stack(trainer.loss_history).tolist(), f)      # one read-back, after the run
    if drawn is not None and rank == 0:
        import json
        with open(a.index_file, "w") as f:
            json.dump(drawn, f)
    print("saved", last)


if __name__ == "__main__":
    main()
