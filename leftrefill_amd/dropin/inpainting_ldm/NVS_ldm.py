"""`inpainting_ldm.NVS_ldm` -- the novel-view-synthesis task model (reference inpainting_ldm/NVS_ldm.py; BASELINE configs[4] trains it:
configs/nvs_training_config.yaml) on the MI355X build.

`NVSUnetModel` (reference 22-104) is the UNet with two input-side additions, both index arithmetic around the same HIP blocks:
  * `c_input` (64-68): a tensor added to the output of the first input block (whole canvas, or only its right half) -- the output
    of the optional input-refinement network;
  * `use_sep` (25-32, 57-60, 70-99): a learned separator column `sep_token[str(C)]` is inserted between the left and the right half
    before every block that does not end in a Down / Upsample (canvas width W -> W + 1) and cut out again after it.
`NVSLDM` (107-298): conditioning glue (get_input with the refinement branch, unconditional prompts incl. deep prompts), `log_images`,
`log_multi_cond_images` (K conditionings through DDIMSampler.ddim_multi_sampling) and `sample_log`; the parameter groups its
optimizer owns (`trainable_parameters`, reference 314-337); `validation_step` / `validation_epoch_end` (374-412): the right half of
the RAW prediction (no paste: "whole image test", 380-381) scored by the HIP metrics kernel (evalglue.device_metrics).  
`train_dataloader` / `val_dataloader` (348-372) build the Objaverse dataset (dropin dataloaders/obj_nvs_dataset.py; the DTU branches
raise: the reference tree ships no such modules) and `on_train_batch_end` (299-306) is the mask warm-up.  `set_lora` (154-168) injects LoRA
layers into the UNet's attention / GEGLU Linears (inpainting_ldm/lora.py, `lora_type: 'default'`) and `configure_optimizers` gives the factors
a parameter group of their own (`lr_lora`, `wd_lora`).  The progress-bar hook (308-312) stays out of scope.  The shipped configs use the plain UNetModel with `use_sep: False` and no refinement; the
class is kept a drop-in for checkpoints / configs that turn them on.
"""
import torch
import torch.nn as nn

from leftrefill_amd import engine, evalglue, rawbatch
from ldm.models.diffusion.ddim import DDIMSampler
from ldm.models.diffusion.ddpm import LatentInpaintDiffusion
from ldm.modules.diffusionmodules.openaimodel import UNetModel
from ldm.modules.diffusionmodules.util import GroupNorm32, conv_nd

SEP_CHANNELS = (9, 320, 640, 1280, 2560, 1920, 960)      # widths a block input can have in the SD2 UNet (reference 27)


class NVSUnetModel(UNetModel):
    def __init__(self, *args, **kwargs):
        self.use_sep = kwargs.pop("use_sep", False)
        super().__init__(*args, **kwargs)
        self.sep_token = None
        if self.use_sep:
            self.sep_token = nn.ParameterDict({str(ch): nn.Parameter(torch.randn(ch), requires_grad=True) for ch in SEP_CHANNELS})
            self.eager_only = True        # block shapes change inside the step: no captured graph for this variant

    def _needs_autograd(self, context, c_input=None):
        # the separator tokens are trainable parameters of the UNet itself: their gradient needs the autograd path too
        sep_grad = self.use_sep and any(p.requires_grad for p in self.sep_token.values())
        return super()._needs_autograd(context, c_input) or (torch.is_grad_enabled() and sep_grad)

    def _block_in(self, act, steps):
        """[left | right] -> [left | sep | right] for blocks that do not end in a Down / Upsample (57-60, 85-88)."""
        if not self.use_sep or steps[-1][0] in ("down", "up"):
            return act, None
        N, H, W = act.N, act.H, act.W
        tok = act.materialize().reshape(N, H, W, -1)
        C = tok.shape[-1]
        key = str(self.in_channels) if C not in SEP_CHANNELS and str(self.in_channels) in self.sep_token else str(C)
        sep = self.sep_token[key].to(tok.dtype)
        if sep.numel() < C:               # the 9 input channels are zero-padded to the kernels' 64
            sep = torch.cat([sep, sep.new_zeros(C - sep.numel())])
        col = sep.reshape(1, 1, 1, C).expand(N, H, 1, C)
        tok = torch.cat([tok[:, :, :W // 2], col, tok[:, :, W // 2:]], dim=2)
        return engine.Act(tok.reshape(N * H * (W + 1), C).contiguous(), N, H, W + 1), W

    def _block_out(self, act, W):
        if W is None:
            return act
        N, H = act.N, act.H
        tok = act.materialize().reshape(N, H, act.W, -1)
        tok = torch.cat([tok[:, :, :W // 2], tok[:, :, act.W - W // 2:]], dim=2)
        return engine.Act(tok.reshape(N * H * W, -1).contiguous(), N, H, W)


def refinement_network(model_channels):
    """Input-refinement side network (reference 124-143): masked image + sub-pixel mask at image resolution -> a model_channels map
    at latent resolution; a handful of small convolutions per batch, run once per sampling (host PyTorch code like the VAE glue)."""
    return nn.Sequential(conv_nd(2, 4, 32, 3, padding=1), nn.SiLU(),
                         conv_nd(2, 32, 64, 3, padding=1, stride=2), GroupNorm32(16, 64), nn.SiLU(),
                         conv_nd(2, 64, 64, 3, padding=1), GroupNorm32(16, 64), nn.SiLU(),
                         conv_nd(2, 64, 128, 3, padding=1, stride=2), GroupNorm32(32, 128), nn.SiLU(),
                         conv_nd(2, 128, 128, 3, padding=1), GroupNorm32(32, 128), nn.SiLU(),
                         conv_nd(2, 128, 256, 3, padding=1, stride=2), GroupNorm32(32, 256), nn.SiLU(),
                         conv_nd(2, 256, model_channels, 3, padding=1), GroupNorm32(32, model_channels), nn.SiLU())


class NVSLDM(LatentInpaintDiffusion):
    def __init__(self, *args, **kwargs):
        data_cfg = kwargs.pop("data_config", None)
        self_save_prompt_only = kwargs.pop("save_prompt_only", False)
        refinement = kwargs.pop("refinement_config", None) or {"use_input_refinement": False, "only_masked_refine": False}
        lora = kwargs.pop("lora", None) or {"do_lora": False}
        cond_cfg = kwargs.get("cond_stage_config")
        super().__init__(*args, **kwargs)
        self.loss_fn_alex = None
        self.cfg = None
        self.optim_cfg = None
        self.data_cfg = dict(data_cfg) if data_cfg is not None else {}
        self.cond_cfg = dict(cond_cfg.get("params", {}) or {}) if isinstance(cond_cfg, dict) else {}
        self.world_size = 1
        self.image_text_pair = False
        self.img_size = self.data_cfg.pop("img_size", 256)
        self.mask_steps = 0
        self.warmup_mask_steps = self.data_cfg.get("warmup_mask_steps", 0)
        self.complete_mask_rate = self.data_cfg.get("complete_mask_rate", 0)
        self.save_prompt_only = self_save_prompt_only
        self.refinement_config = dict(refinement)
        self.lora_cfg = dict(lora)
        self.unet_lora_params = None
        self.refinement_model = self.refinement_alpha = None
        if self.refinement_config.get("use_input_refinement"):
            self.refinement_model = refinement_network(kwargs["unet_config"]["params"]["model_channels"])
            self.refinement_alpha = nn.Parameter(torch.tensor(0, dtype=torch.float32), requires_grad=True)

    def set_lora(self):
        """reference 154-168: inject the LoRA layers the `lora:` block asks for; called once the base weights are loaded and before the
        optimizer is built (tools/train_inpainting.py)."""
        self.unet_lora_params = None
        if not self.lora_cfg.get("do_lora"):
            return
        from .lora import inject_trainable_lora, inject_trainable_lora_extended
        kind = self.lora_cfg.get("lora_type", "default")
        kw = dict(r=self.lora_cfg["lora_rank"], scale=self.lora_cfg.get("lora_scale", 1.0))
        if kind == "default":
            # `lora_dropout` (optional, default 0): the reference's inject_trainable_lora(dropout_p=...) -- Philox masks inside the HIP
            # LoRA kernels, one stream per injected layer (inpainting_ldm/lora.py)
            self.unet_lora_params, _ = inject_trainable_lora(self.model.diffusion_model, verbose=False,
                                                             dropout_p=float(self.lora_cfg.get("lora_dropout", 0.0)), **kw)
        elif kind == "extended":
            inject_trainable_lora_extended(self.model.diffusion_model, **kw)      # (NotImplementedError naming the reason)
        else:
            raise NotImplementedError("Not implemented LoRA")

    def get_input(self, batch, k, cond_key=None, bs=None, return_first_stage_outputs=False, force_c_encode=True):
        x, c = super().get_input(batch, k, cond_key, bs, return_first_stage_outputs, force_c_encode)
        c["c_input"] = None
        if self.refinement_config.get("use_input_refinement"):
            masked_key, mask_key = (("clean_masked_image", "clean_mask") if self.refinement_config.get("only_masked_refine", False)
                                    else ("masked_image", "subpixel_mask"))
            to_nchw = lambda t: t.permute(0, 3, 1, 2).to(self.device).contiguous().float()      # 'b h w c -> b c h w'
            inp = torch.cat([to_nchw(batch[masked_key]), to_nchw(batch[mask_key])], dim=1)
            if bs is not None:
                inp = inp[:bs]
            c["c_input"] = self.refinement_model(inp) * self.refinement_alpha
        return x, c

    @torch.no_grad()
    def get_unconditional_conditioning(self, N):
        if self.cond_cfg.get("deep_prompt", False):
            return self.get_learned_conditioning([[""] * N] * self.cond_cfg["cross_attn_layers"])
        return self.get_learned_conditioning([""] * N)

    def _cond_pair(self, batch, N):
        """(cond, uncond) dicts of one batch for classifier-free guidance: same c_concat / c_input, empty prompts (247-262)."""
        z, c = self.get_input(batch, self.first_stage_key, bs=N)
        n = min(z.shape[0], N)
        c_full = {"c_concat": [c["c_concat"][0][:N]], "c_crossattn": [c["c_crossattn"][0][:N]]}
        uc_full = {"c_concat": [c_full["c_concat"][0]], "c_crossattn": [self.get_unconditional_conditioning(n)]}
        if c.get("c_input") is not None:
            c_full["c_input"] = c["c_input"][:N]
            uc_full["c_input"] = c_full["c_input"].clone()
        return n, c_full, uc_full

    @torch.no_grad()
    def log_images(self, batch, N=4, ddim_steps=50, ddim_eta=0.0, unconditional_guidance_scale=9.0, return_attn=False, **kwargs):
        """return_attn: adds log["att_scores"] (DDIMSampler.ddim_sampling); the separator-token UNet itself is refused by the
        attention probe, so this serves NVS models on the plain single-view UNet."""
        log = {"masked_image": batch["masked_image"].permute(0, 3, 1, 2), "origin_image": batch["image"].permute(0, 3, 1, 2)}
        n, c_full, uc_full = self._cond_pair(batch, N)
        attn = {"return_attn": True} if return_attn else {}
        if unconditional_guidance_scale > 1.0:
            out = self.sample_log(cond=c_full, batch_size=n, ddim=ddim_steps is not None, ddim_steps=ddim_steps, eta=ddim_eta,
                                  unconditional_guidance_scale=unconditional_guidance_scale, unconditional_conditioning=uc_full, **attn)
        else:      # (the reference drops c_input on this branch, 274-276)
            out = self.sample_log(cond={k: c_full[k] for k in ("c_concat", "c_crossattn")}, batch_size=n,
                                  ddim=ddim_steps is not None, ddim_steps=ddim_steps, eta=ddim_eta, **attn)
        log["pred"] = self.decode_first_stage(out[0])
        if return_attn:
            log["att_scores"] = out[2]
        return log

    @torch.no_grad()
    def log_multi_cond_images(self, batch, N=4, ddim_steps=50, ddim_eta=0.0, unconditional_guidance_scale=9.0, **kwargs):
        """`batch` = list of K batches (K reference views of the same targets): the K conditionings are denoised side by side and
        share their right half after every step (DDIMSampler.ddim_multi_sampling; reference 283-319)."""
        assert isinstance(batch, list)
        log = {"masked_image": batch[0]["masked_image"].permute(0, 3, 1, 2), "origin_image": batch[0]["image"].permute(0, 3, 1, 2)}
        conds, unconds, n = [], [], N
        for b_ in batch:
            n, c_full, uc_full = self._cond_pair(b_, N)
            conds.append(c_full)
            unconds.append(uc_full)
        samples, _ = self.sample_log(cond=conds, batch_size=n, ddim=ddim_steps is not None, ddim_steps=ddim_steps, eta=ddim_eta,
                                     unconditional_guidance_scale=unconditional_guidance_scale, unconditional_conditioning=unconds)
        log["pred"] = self.decode_first_stage(samples)
        return log

    @torch.no_grad()
    def sample_log(self, cond, batch_size, ddim, ddim_steps, **kwargs):
        first = cond[0] if isinstance(cond, list) else cond
        _, _, h, w = first["c_concat"][0].shape
        return DDIMSampler(self).sample(ddim_steps, batch_size, (self.channels, h, w), cond, verbose=False, **kwargs)

    def trainable_parameters(self):
        """What the reference's optimizer owns besides an optional full-UNet group (configure_optimizers, 314-337): the learned
        prompt tokens, the pose MLP, the refinement network and the separator tokens' owner decides on those itself."""
        params = list(self.cond_stage_model.special_embeddings.parameters())
        if getattr(self.cond_stage_model, "rel_pos_model", None) is not None:
            params.extend(self.cond_stage_model.rel_pos_model.parameters())
        if self.refinement_model is not None and self.refinement_alpha is not None:
            params.extend(self.refinement_model.parameters())
            params.append(self.refinement_alpha)
        return params

    @torch.no_grad()
    def validation_step(self, batch, batch_idx):
        """reference 374-401: columns w//2: of the prediction as sampled -- the mask is not pasted -- against the same columns of the
        image; mean PSNR / SSIM (/ LPIPS) over the batch as Python floats."""
        N = batch["image"].shape[0]
        log = self.log_images(batch, N=N, unconditional_guidance_scale=self.data_cfg["cfg"])
        metrics = evalglue.device_metrics(log, None, compose=False, right_half=True)

        def lpips_pair():
            w = log["origin_image"].shape[3]
            return log["pred"].float()[:, :, :, w // 2:], log["origin_image"].float()[:, :, :, w // 2:]

        return evalglue.validation_result(self, metrics, lpips_pair, lambda fn: fn.score(log, None, compose=False, right_half=True))

    def validation_epoch_end(self, outputs):
        return evalglue.validation_epoch_mean(self, outputs)

    # ---- data (reference 299-306, 348-372) ----------------------------------------------------------------------------------------------
    def _objaverse(self, listfile, mode, raw):
        if not self.data_cfg.get("obj_dataset"):
            raise NotImplementedError("the DTU novel-view datasets (data_config.obj_dataset: False) are no part of the reference tree; "
                                      "this build has the Objaverse dataset only")
        from leftrefill_amd.dropin.dataloaders.obj_nvs_dataset import NVS_OBJDataset
        return NVS_OBJDataset(datapath=self.cfg["datapath"], listfile=self.cfg[listfile], mode=mode, img_size=self.img_size, raw=raw,
                              **self.data_cfg)

    def train_dataloader(self, raw=False, num_workers=8, device=None):
        """raw=True: the loader hands out `nvsprep.collate_nvs_raw` batches; with a device, an `nvsprep.NVSDevicePrep` there finishes
        them (`rawbatch.loader`)."""
        return rawbatch.loader(self._objaverse("train_list", "train", raw), raw, device, batch_size=self.cfg["batch_size"], shuffle=True,
                               num_workers=num_workers)

    def val_dataloader(self, raw=False, num_workers=4, batch_size=4, device=None):
        return rawbatch.loader(self._objaverse("val_list", "val", raw), raw, device, batch_size=batch_size, shuffle=False, drop_last=True,
                               num_workers=num_workers)

    def on_train_batch_end(self, *args, **kwargs):
        """The mask warm-up (reference 299-306): over `warmup_mask_steps` steps the training dataset's `complete_mask_rate` rises
        linearly from its configured value to 1.  The dataset is the one reached through `trainer.train_dataloader`; loader workers
        hold copies of it and see the new rate when they are re-created -- at the next epoch --, as in the reference."""
        hook = getattr(super(), "on_train_batch_end", None)
        if hook is not None:
            hook(*args, **kwargs)
        if self.warmup_mask_steps > 0 and self.mask_steps <= self.warmup_mask_steps:
            dataset = self.trainer.train_dataloader.dataset
            dataset.complete_mask_rate = min(1.0, self.complete_mask_rate +
                                             (self.mask_steps / self.warmup_mask_steps * (1.0 - self.complete_mask_rate)))
            self.mask_steps += 1

    # ---- training (reference 314-345, 418-435) -------------------------------------------------------------------------------------------
    def configure_optimizers(self):
        """One group: prompt tokens (+ pose MLP, + refinement network and its gate where configured), on AmpAdamW."""
        from leftrefill_amd.optim import configure_prompt_optimizer
        if self.optim_cfg.get("all_trainable", False):
            raise NotImplementedError("all_trainable: this build computes no weight gradients of the UNet (its backward stops at the "
                                      "activations and the context)")
        groups = [{"params": self.trainable_parameters(), "lr": self.optim_cfg["learning_rate"]}]
        if self.unet_lora_params is not None:      # reference 333-335: the factors' own learning rate and weight decay
            import itertools
            if getattr(getattr(self, "trainer", None), "hip_graph", False):
                raise NotImplementedError("Trainer(hip_graph=True) with trainable LoRA factors: the factor-gradient kernels' workspaces "
                                          "are allocated per call, the captured training step is not validated with them")
            self.unet_lora_params = [list(g_) for g_ in self.unet_lora_params]      # (the reference's generators: walked once, kept)
            params = list(itertools.chain(*self.unet_lora_params))
            # the only weight gradients of this build are those of the factors of LoRA layers injected into THIS model's UNet
            # (set_lora): any other parameter in the group would sit in the optimizer and never receive a gradient
            injected = {id(p_) for m_ in self.model.diffusion_model.modules() if hasattr(m_, "lora_down") and hasattr(m_, "lora_up")
                        for p_ in (m_.lora_up.weight, m_.lora_down.weight)}
            if not params or any(id(p_) not in injected for p_ in params):
                raise NotImplementedError("LoRA parameter group: this build computes weight gradients only for the factors of the LoRA "
                                          "layers that set_lora() injected into this model's UNet; the group holds other parameters")
            groups.append({"params": params, "lr": self.optim_cfg["lr_lora"], "weight_decay": self.optim_cfg["wd_lora"]})
        return configure_prompt_optimizer(self, groups)

    LORA_DROPOUT_KEY = "lora_dropout_state"      # checkpoint key of the UNet's (seed, draw): a resumed run continues the mask sequence

    def on_load_checkpoint(self, checkpoint):
        from .lora import lora_dropout_state
        state = lora_dropout_state(self.model.diffusion_model)
        if state is not None and self.LORA_DROPOUT_KEY in checkpoint:      # (a checkpoint without the key loads as before)
            state.load_state_dict(checkpoint[self.LORA_DROPOUT_KEY])

    def on_save_checkpoint(self, checkpoint):
        from .lora import lora_dropout_state
        state = lora_dropout_state(self.model.diffusion_model)
        if state is not None:
            checkpoint[self.LORA_DROPOUT_KEY] = state.state_dict()
        if self.save_prompt_only:
            from leftrefill_amd.optim import keep_keys

            def keep(k):      # the prompt encoder without its CLIP tower, the refinement network, LoRA factors, the separator token
                return ((k.startswith("cond_stage_model") and not k.startswith("cond_stage_model.model.")) or k.startswith("refinement_")
                        or "lora_down" in k or "lora_up" in k or "sep_token" in k)

            keep_keys(checkpoint, keep)
