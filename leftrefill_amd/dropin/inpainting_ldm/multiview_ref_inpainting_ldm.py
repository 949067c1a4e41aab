"""`inpainting_ldm.multiview_ref_inpainting_ldm.RefInpaintLDM` -- multi-view task model (configs/multiview_ref_inpainting.yaml:2).

Inference entry points of the reference class (inpainting_ldm/multiview_ref_inpainting_ldm.py): the extra constructor
kwargs `view_mode / view_num / concat_target / reduced_loss` (33-36), `get_input` flattening `[b, v, h, w, c]` batches
to `(b v)` canvases (99-111) and `log_images` (113-180), which samples all `(b v)` canvases jointly (the views meet in
MultiViewUnetModel's re-arranged self-attention) and returns the target view plus the references:
  concat_target: canvases are [ref_i | target]; pred / origin / masked = right half of canvas 0, reference = left halves;
  otherwise    : view 0 is the target, views 1.. are the references.
Training objective `p_losses` (38-91): the single-reference objective per canvas, of which only view 0 of every sample counts.
`validation_step` (225-263): the target view pasted with the mask of canvas 0 of every sample, scored by the HIP metrics kernel
(evalglue.device_metrics_multiview); `validation_epoch_end` is the single-view model's.
"""
import torch

from leftrefill_amd import evalglue

from inpainting_ldm.ref_inpainting_ldm import RefInpaintLDM as _SingleViewLDM
from ldm.modules.diffusionmodules.util import extract_into_tensor
from ldm.util import default


class RefInpaintLDM(_SingleViewLDM):
    def __init__(self, *args, **kwargs):
        mv = (kwargs.get('view_mode', False), kwargs.get('view_num', 4), kwargs.get('concat_target', False),
              kwargs.get('reduced_loss', True))
        super().__init__(*args, **kwargs)       # DDPM.__init__ swallows the extra keys, as in the reference
        self.view_mode, self.view_num, self.concat_target, self.reduced_loss = mv

    def p_losses(self, x_start, cond, t, noise=None):
        """reference 38-91: per-canvas MSE, logvar[t] weighting and the vlb term, then '(b v) -> b v' and view 0 only."""
        noise = default(noise, lambda: torch.randn_like(x_start))
        x_noisy = self.q_sample(x_start=x_start, t=t, noise=noise)
        model_output = self.apply_model(x_noisy, t, cond)
        prefix = 'train' if self.training else 'val'
        if self.parameterization == "x0":
            target = x_start
        elif self.parameterization == "eps":
            target = noise
        else:      # "v" (DDPM.get_v of the reference): sqrt(a_t) noise - sqrt(1 - a_t) x0
            target = (extract_into_tensor(self.sqrt_alphas_cumprod, t, x_start.shape) * noise -
                      extract_into_tensor(self.sqrt_one_minus_alphas_cumprod, t, x_start.shape) * x_start)
        v = self.view_num - 1 if self.concat_target else self.view_num

        def view0(per_canvas):      # '(b v) -> b v', [:, 0]
            return per_canvas.reshape(-1, v)[:, 0]

        loss_dict = {}
        loss_simple = self.get_loss(model_output, target, mean=False).mean([1, 2, 3])
        loss_dict[f'{prefix}/loss_simple'] = view0(loss_simple).mean()
        logvar_t = self.logvar[t].to(self.device)
        loss = loss_simple / torch.exp(logvar_t) + logvar_t
        if self.learn_logvar:
            raise NotImplementedError("learn_logvar is not supported by the multi-view objective (as in the reference)")
        loss = self.l_simple_weight * view0(loss).mean()
        loss_vlb = self.get_loss(model_output, target, mean=False).mean(dim=(1, 2, 3))
        loss_vlb = view0(self.lvlb_weights[t] * loss_vlb).mean()
        loss_dict[f'{prefix}/loss_vlb'] = loss_vlb
        loss = loss + self.original_elbo_weight * loss_vlb
        loss_dict[f'{prefix}/loss'] = loss
        return loss, loss_dict

    def get_input(self, batch, k, cond_key=None, bs=None, return_first_stage_outputs=False, force_c_encode=True, seeds=None):
        if batch['image'].dim() == 5:            # [b, v, h, w, c] -> (b v) canvases, in place like the reference (100-104)
            for key in ('image', 'masked_image', 'mask'):
                t = batch[key]
                batch[key] = t.reshape(t.shape[0] * t.shape[1], *t.shape[2:])
        return super().get_input(batch, k, cond_key=cond_key, bs=bs,
                                 return_first_stage_outputs=return_first_stage_outputs, force_c_encode=force_c_encode, seeds=seeds)

    @torch.no_grad()
    def log_images(self, batch, N=4, ddim_steps=50, ddim_eta=0.0, unconditional_guidance_scale=9.0, seeds=None, **kwargs):
        """seeds: None, or one key per CANVAS, (b v) of them in the batch's order (the samplers' `seeds=`): the posterior sample of
        the masked-image encoding and every draw of the sampler are then that canvas's own seeded draws."""
        img = batch['image']
        sd = {} if seeds is None else {"seeds": seeds}
        N = img.shape[0] * img.shape[1] if img.dim() == 5 else img.shape[0]      # every canvas of every sample (114-117)
        v = self.view_num - 1 if self.concat_target else self.view_num
        use_ddim = ddim_steps is not None
        z, c = self.get_input(batch, self.first_stage_key, bs=N, **sd)
        c_concat, c_crossattn = c["c_concat"][0][:N], c["c_crossattn"][0][:N]
        N = min(z.shape[0], N)
        if unconditional_guidance_scale > 1.0:
            uc_full = {"c_concat": [c_concat], "c_crossattn": [self.get_unconditional_conditioning(N)]}
            samples, _ = self.sample_log(cond={"c_concat": [c_concat], "c_crossattn": [c_crossattn]}, batch_size=N,
                                         ddim=use_ddim, ddim_steps=ddim_steps, eta=ddim_eta,
                                         unconditional_guidance_scale=unconditional_guidance_scale,
                                         unconditional_conditioning=uc_full, **sd)
        elif unconditional_guidance_scale == 0.0:
            uc_cross = self.get_unconditional_conditioning(N)
            samples, _ = self.sample_log(cond={"c_concat": [c_concat], "c_crossattn": [uc_cross]}, batch_size=N,
                                         ddim=use_ddim, ddim_steps=ddim_steps, eta=ddim_eta, **sd)
        else:
            samples, _ = self.sample_log(cond={"c_concat": [c_concat], "c_crossattn": [c_crossattn]}, batch_size=N,
                                         ddim=use_ddim, ddim_steps=ddim_steps, eta=ddim_eta, **sd)
        pred = self.decode_first_stage(samples)

        def by_view(t):      # '(b v) c h w -> b v c h w'
            return t.reshape(t.shape[0] // v, v, *t.shape[1:])

        masked = by_view(batch['masked_image'].permute(0, 3, 1, 2))
        origin = by_view(batch['image'].permute(0, 3, 1, 2))
        pred = by_view(pred)
        log = dict()
        if self.concat_target:
            cut = pred.shape[3]          # the reference splits the width at pred.shape[3] (= H: square halves), 163-166
            log["reference"] = masked[:, :, :, :, 0:cut]
            log["masked_image"] = masked[:, 0, :, :, cut:]
            log["origin_image"] = origin[:, 0, :, :, cut:]
            log["pred"] = pred[:, 0, :, :, cut:]
        else:
            log["reference"] = masked[:, 1:]
            log["masked_image"] = masked[:, 0]
            log["origin_image"] = origin[:, 0]
            log["pred"] = pred[:, 0]
        return log

    @torch.no_grad()
    def validation_step(self, batch, batch_idx):
        """reference 225-263: every canvas of every sample is sampled, the target view is pasted with the mask of canvas 0 (its target
        half under concat_target) and scored whole."""
        img = batch['image']
        N = img.shape[0] * img.shape[1] if img.dim() == 5 else img.shape[0]
        log = self.log_images(batch, N=N, unconditional_guidance_scale=self.data_cfg['cfg'])
        v = self.view_num - 1 if self.concat_target else self.view_num
        flat = batch['mask']                     # [(b v), H, W, 1]: log_images flattened it in place, like the reference
        metrics, _ = evalglue.device_metrics_multiview(log, flat, flat.shape[0] // v)

        def lpips_pair():
            mask = flat.float().permute(0, 3, 1, 2)
            mask = mask.reshape(mask.shape[0] // v, v, *mask.shape[1:])[:, 0]
            if self.concat_target:
                mask = mask[:, :, :, mask.shape[2]:]
            pred, origin = log['pred'].float(), log['origin_image'].float()
            return pred * mask + origin * (1 - mask), origin

        return evalglue.validation_result(self, metrics, lpips_pair, lambda fn: fn.score_multiview(log, flat, flat.shape[0] // v)[0])
