"""`inpainting_ldm.ref_inpainting_ldm.RefInpaintLDM` -- the inference entry points of LeftRefill on the MI355X build.

Reproduces `log_images` / `sample_log` / `get_unconditional_conditioning` (reference
inpainting_ldm/ref_inpainting_ldm.py:30-81) and the attributes callers read (`cond_cfg`, `data_cfg`, `world_size`,
`loss_fn_alex`, `save_prompt_only`, test_inpainting.py:95-110), and the validation hooks `validation_step` /
`validation_epoch_end` (119-157): PSNR / SSIM of the pasted right half come from one HIP kernel (evalglue.device_metrics), LPIPS from
`loss_fn_alex` when one is set; the optimizer and checkpoint hooks (83-96, 164-173) over leftrefill_amd.optim; and the dataloaders
(99-117) with the epoch hook (159-161).  `train_dataloader` / `val_dataloader` take `raw=True` for loaders that collate raw decoded
images and `device=` for the dataset's own `DevicePrep` to finish them there (`rawbatch.loader`; tools/train_inpainting.py --device_prep).

Stated deviation: `on_train_epoch_start` sets the sampler's epoch on every rank.  The reference does so only for world_size == 1,
against its own comment ("we have to set epoch manually if using ddp"); under DDP its ranks would repeat epoch 0's draw for ever.
"""
import torch

from leftrefill_amd import evalglue, rawbatch

from ldm.models.diffusion.ddim import DDIMSampler
from ldm.models.diffusion.ddpm import LatentInpaintDiffusion


def make_sampler(name, model):
    """"ddim" | "plms" | "dpm_solver" -> the drop-in sampler of that name over `model`.  ("ddpm", the ancestral sampler, is not a
    sampler object: it lives on the model -- `LatentDiffusion.sample` -- and `RefInpaintLDM.sample_log` routes to it.)"""
    if name == "ddim":
        return DDIMSampler(model)
    if name == "plms":
        from ldm.models.diffusion.plms import PLMSSampler
        return PLMSSampler(model)
    if name == "dpm_solver":
        from ldm.models.diffusion.dpm_solver import DPMSolverSampler
        return DPMSolverSampler(model)
    if name == "ddpm":
        raise ValueError("'ddpm' is the model's own ancestral sampler (model.sample / sample_log(sampler='ddpm')), not a sampler class")
    raise ValueError(f"unknown sampler {name!r}: 'ddim', 'plms', 'dpm_solver' or 'ddpm'")


def _ddpm_has_no_guidance(scale):
    raise ValueError(f"sampler 'ddpm' (ancestral) has no classifier-free guidance: unconditional_guidance_scale={scale!r} would be "
                     "dropped; use 1.0, or one of the guided samplers 'ddim', 'plms', 'dpm_solver'")


class RefInpaintLDM(LatentInpaintDiffusion):
    def __init__(self, *args, **kwargs):
        data_cfg = kwargs.pop('data_config', None)
        save_prompt_only = kwargs.pop('save_prompt_only', False)
        cond_cfg = kwargs.get('cond_stage_config')
        super().__init__(*args, **kwargs)
        self.loss_fn_alex = None
        self.cfg = None
        self.optim_cfg = None
        self.data_cfg = dict(data_cfg) if data_cfg is not None else {}
        self.cond_cfg = dict(cond_cfg.get('params', {}) or {}) if isinstance(cond_cfg, dict) else {}
        self.world_size = 1
        self.image_text_pair = False
        self.img_size = self.data_cfg.pop('img_size', 256)
        self.save_prompt_only = save_prompt_only

    @torch.no_grad()
    def get_unconditional_conditioning(self, N):
        if self.cond_cfg.get('deep_prompt', False):
            return self.get_learned_conditioning([[""] * N] * self.cond_cfg['cross_attn_layers'])
        return self.get_learned_conditioning([""] * N)

    @torch.no_grad()
    def log_images(self, batch, N=4, ddim_steps=50, ddim_eta=0.0, unconditional_guidance_scale=9.0, sampler="ddim", return_attn=False,
                   seeds=None, **kwargs):
        """sampler: "ddim" (the reference's), "plms" or "dpm_solver"; ddim_steps is the step count of any of them.  "ddpm": the
        ancestral sampler over the full schedule (ddim_steps is ignored), which has no guidance -- unconditional_guidance_scale must
        be 1 (or 0: the empty-prompt condition).  return_attn (the reference's keyword, passed from the config's `return_attn`; DDIM
        only): adds log["att_scores"], the sampler's per-layer reference-attention maps (DDIMSampler.ddim_sampling).
        seeds: None, or one key per sample of the batch (the samplers' `seeds=`): the posterior sample of the masked-image encoding and
        every draw of the sampler are then that sample's own seeded draws (leftrefill_amd/noise.py)."""
        if return_attn and sampler != "ddim":
            raise NotImplementedError(f"log_images: return_attn is served by the DDIM sampler, not {sampler!r} (wrap the call in a "
                                      "leftrefill_amd.attnprobe.AttentionProbe instead)")
        attn = {"return_attn": True} if return_attn else {}
        if seeds is not None:
            from leftrefill_amd.noise import shard_seeds
            attn["seeds"] = shard_seeds(seeds, 0, min(N, batch[self.first_stage_key].shape[0]))
        if sampler == "ddpm" and unconditional_guidance_scale not in (0.0, 1.0):
            _ddpm_has_no_guidance(unconditional_guidance_scale)
        use_ddim = ddim_steps is not None
        log = dict()
        z, c = self.get_input(batch, self.first_stage_key, bs=N, **({} if seeds is None else {"seeds": attn["seeds"]}))
        c_concat, c_crossattn = c["c_concat"][0][:N], c["c_crossattn"][0][:N]
        N = min(z.shape[0], N)
        log["masked_image"] = batch['masked_image'].permute(0, 3, 1, 2)
        log["origin_image"] = batch['image'].permute(0, 3, 1, 2)
        if unconditional_guidance_scale > 1.0:
            uc_full = {"c_concat": [c_concat], "c_crossattn": [self.get_unconditional_conditioning(N)]}
            out = self.sample_log(cond={"c_concat": [c_concat], "c_crossattn": [c_crossattn]}, batch_size=N,
                                  ddim=use_ddim, ddim_steps=ddim_steps, eta=ddim_eta,
                                  unconditional_guidance_scale=unconditional_guidance_scale,
                                  unconditional_conditioning=uc_full, sampler=sampler, **attn)
        elif unconditional_guidance_scale == 0.0:
            uc_cross = self.get_unconditional_conditioning(N)
            out = self.sample_log(cond={"c_concat": [c_concat], "c_crossattn": [uc_cross]}, batch_size=N,
                                  ddim=use_ddim, ddim_steps=ddim_steps, eta=ddim_eta, sampler=sampler, **attn)
        else:
            out = self.sample_log(cond={"c_concat": [c_concat], "c_crossattn": [c_crossattn]}, batch_size=N,
                                  ddim=use_ddim, ddim_steps=ddim_steps, eta=ddim_eta, sampler=sampler, **attn)
        log["pred"] = self.decode_first_stage(out[0])
        if return_attn:
            log["att_scores"] = out[2]
        return log

    @torch.no_grad()
    def sample_log(self, cond, batch_size, ddim, ddim_steps, sampler="ddim", **kwargs):
        _, _, h, w = cond["c_concat"][0].shape
        if sampler == "ddpm":
            scale = kwargs.pop("unconditional_guidance_scale", 1.)
            kwargs.pop("unconditional_conditioning", None)
            if scale != 1.:
                _ddpm_has_no_guidance(scale)
            kwargs.pop("eta", None)      # a DDIM knob; the ancestral chain has its own variance
            return self.sample(cond=cond, batch_size=batch_size, return_intermediates=True, verbose=False,
                               shape=(batch_size, self.channels, h, w), **kwargs)
        sampler = make_sampler(sampler, self)
        shape = (self.channels, h, w)   # latent size comes from c_concat (reference 77-79)
        return sampler.sample(ddim_steps, batch_size, shape, cond, verbose=False, **kwargs)

    @torch.no_grad()
    def validation_step(self, batch, batch_idx):
        """reference 119-146: sample the batch at guidance scale data_cfg['cfg'], paste the known pixels back, keep columns w//2:,
        mean PSNR / SSIM (/ LPIPS) over the batch as Python floats."""
        N = batch['image'].shape[0]
        log = self.log_images(batch, N=N, unconditional_guidance_scale=self.data_cfg['cfg'])
        metrics = evalglue.device_metrics(log, batch['mask'], right_half=True)

        def lpips_pair():
            mask = batch['mask'].permute(0, 3, 1, 2).float()
            pred, origin = log['pred'].float(), log['origin_image'].float()
            w = origin.shape[3]
            return (pred * mask + origin * (1 - mask))[:, :, :, w // 2:], origin[:, :, :, w // 2:]

        return evalglue.validation_result(self, metrics, lpips_pair, lambda fn: fn.score(log, batch['mask'], right_half=True))

    def validation_epoch_end(self, outputs):
        return evalglue.validation_epoch_mean(self, outputs)

    # ---- data: the loaders of reference 99-117 and the epoch hook of 159-161 ------------------------------------------------------------------
    def train_dataloader(self, raw=False, num_workers=8, device=None):
        """raw=True: the loader hands out `dataprep.collate_raw` batches; with a device, a `dataprep.DevicePrep` there finishes them
        (`rawbatch.loader`)."""
        if self.cfg.get('cross_view_inpainting'):
            from leftrefill_amd.dropin.dataloaders.inpainting_crossview_dataset import BalancedRandomSampler, InpaintingCrossViewDataset
            train_dataset = InpaintingCrossViewDataset(image_path=self.cfg['image_path'], pair_path=self.cfg['train_pair'],
                                                       mask_path=self.cfg['train_mask_path'], mode='train', img_size=self.img_size,
                                                       deep_prompt=self.cond_cfg.get('deep_prompt', False), raw=raw, **self.data_cfg)
            sampler = BalancedRandomSampler(train_dataset.image_dict, train_dataset.pairs,
                                            n_sample_per_scene=self.cfg['n_sample_per_scene'],
                                            rank=self.local_rank, num_replicas=self.world_size)
            return rawbatch.loader(train_dataset, raw, device, batch_size=self.cfg['batch_size'], sampler=sampler, num_workers=num_workers)
        from dataloaders.inpainting_dataset import InpaintingDataset
        train_dataset = InpaintingDataset(image_list=self.cfg['image_path'], mask_path=self.cfg['train_mask_path'],
                                          annotation=self.cfg.get('annotation'), mode='train', img_size=self.img_size, raw=raw, **self.data_cfg)
        return rawbatch.loader(train_dataset, raw, device, batch_size=self.cfg['batch_size'], shuffle=True, num_workers=num_workers)

    def val_dataloader(self, raw=False, num_workers=4, batch_size=4, device=None):
        from leftrefill_amd.dropin.dataloaders.inpainting_crossview_dataset import InpaintingCrossViewDataset
        data_cfg = dict(self.data_cfg)
        if 'test_limit' in self.cfg:      # the reference's model configs carry it in their data section; a training config may too
            data_cfg.setdefault('test_limit', self.cfg['test_limit'])
        val_dataset = InpaintingCrossViewDataset(image_path=self.cfg['val_image_path'], pair_path=None,
                                                 mask_path=self.cfg['val_mask_path'], mode='val', img_size=self.img_size,
                                                 deep_prompt=self.cond_cfg.get('deep_prompt', False), raw=raw, **data_cfg)
        return rawbatch.loader(val_dataset, raw, device, batch_size=batch_size, shuffle=False, drop_last=True, num_workers=num_workers)

    def on_train_epoch_start(self):
        if self.cfg and self.cfg.get('cross_view_inpainting'):      # on every rank (the reference: only without DDP, see above)
            sampler = getattr(getattr(self.trainer, "train_dataloader", None), "sampler", None)
            if hasattr(sampler, "set_epoch"):
                sampler.set_epoch(self.current_epoch)

    # ---- training: the optimizer owns the learned prompt tokens only (reference 83-96), a checkpoint keeps only them (164-173) ----------
    def configure_optimizers(self):
        from leftrefill_amd.optim import configure_prompt_optimizer
        return configure_prompt_optimizer(self, [{"params": list(self.cond_stage_model.special_embeddings.parameters())}])

    def on_save_checkpoint(self, checkpoint):
        if self.save_prompt_only:      # everything of the prompt encoder except its frozen CLIP tower (`cond_stage_model.model.`)
            from leftrefill_amd.optim import keep_keys
            keep_keys(checkpoint, lambda k: k.startswith("cond_stage_model") and not k.startswith("cond_stage_model.model."))
