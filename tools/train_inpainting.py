#!/usr/bin/env python
"""Prompt tuning from the command line: the flags and the flow of the reference's train_inpainting.py on leftrefill_amd.trainer.Trainer.

    python tools/train_inpainting.py --config_file configs/training.yaml --exp_name my_run --fp16 --synthetic 200
    python tools/train_inpainting.py --config_file ... --exp_name my_run --fp16 --dataset mypkg.data:TrainSet

The training config names `model_config`, `resume_path` (backbone weights), `optim_cfg`, `max_steps`, `accumulate_grad_batches`
and `batch_size`, as the reference's check_points/*/training_config.yaml does.  Validation needs the reference's validation
datasets, which are not part of this build: the CLI runs none (`val_check_interval` is ignored) and writes `last.ckpt` at the end.  Checkpoints go to
<save_path>/<exp_name>/ckpts/last.ckpt; --restore continues from it (the default when it exists, unless --no_restore).

The training datasets are not part of this build: --synthetic N trains on N generated batches with the evaluation harness' batch
contract (tools/run_inpainting.py), --dataset module:Class on `Class(**data_cfg)` through torch's DataLoader.
"""
import argparse
import importlib
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


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
    ap.add_argument("--dataset", type=str, default=None, help="module:Class of a map-style training dataset")
    ap.add_argument("--hip_graph", action="store_true", help="replay the whole step as one hipGraph (fixed shapes)")
    a = ap.parse_args()

    import leftrefill_amd.dropin as dropin
    dropin.install()
    from inpainting_ldm.model import create_model, load_config, load_state_dict
    from leftrefill_amd.trainer import Trainer
    from tools.run_inpainting import synthetic_batches

    rank = int(os.environ.get("LOCAL_RANK", 0))
    if a.ngpu > 1:
        torch.distributed.init_process_group("nccl")
    torch.cuda.set_device(rank)
    config = load_config(a.config_file)
    model = create_model(config["model_config"])
    if config.get("resume_path"):
        print(model.load_state_dict(load_state_dict(config["resume_path"]), strict=False))
    model.cfg, model.optim_cfg, model.world_size = config, config["optim_cfg"], a.ngpu
    model = model.to(f"cuda:{rank}")

    root = os.path.join(a.save_path, a.exp_name)
    last = os.path.join(root, "ckpts", "last.ckpt")
    resume = last if (a.restore or not a.no_restore) and os.path.exists(last) else None
    if a.restore and resume is None:
        raise FileNotFoundError(last)
    bs = int(config.get("batch_size", 1))
    if a.dataset:
        mod, cls = a.dataset.split(":")
        data = torch.utils.data.DataLoader(getattr(importlib.import_module(mod), cls)(**dict(model.data_cfg)), batch_size=bs, shuffle=True,
                                           num_workers=8, drop_last=True)
    elif a.synthetic:
        data = list(synthetic_batches(a.synthetic, bs, int(model.img_size), seed=rank))
    else:
        raise SystemExit("give --synthetic N or --dataset module:Class (the reference's training datasets are not part of this build)")
    trainer = Trainer(max_steps=int(config["max_steps"]), accumulate_grad_batches=int(config.get("accumulate_grad_batches") or 1),
                      val_check_interval=None, precision=16 if a.fp16 else ("bf16" if a.bf16 else 32), default_root_dir=root,
                      resume_from_checkpoint=resume, hip_graph=a.hip_graph, local_rank=rank)
    trainer.fit(model, data)
    print("saved", last)


if __name__ == "__main__":
    main()
