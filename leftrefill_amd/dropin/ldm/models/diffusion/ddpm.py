"""`ldm.models.diffusion.ddpm` -- inference-side host glue for the MI355X build.

Keeps the reference's class names, constructor kwargs and attributes that the sampler / callers read
(reference ldm/models/diffusion/ddpm.py: DDPM 46-535, LatentDiffusion 538-1324, DiffusionWrapper 1327-1371,
LatentFinetuneDiffusion 1512-1651, LatentInpaintDiffusion 1654-1701), minus the PyTorch-Lightning trainer hooks,
EMA, logging and the unused upscale/depth variants (out of scope).

The ancestral DDPM sampler lives here as in the reference (`LatentDiffusion.sample` / `p_sample_loop` / `p_sample` /
`progressive_denoising` / `sample_log`, 937-1136): per timestep one replay of the captured UNet step and one lr_ddpm_step launch.

On the hot path only `apply_model` -> `DiffusionWrapper.forward` ('hybrid': channel-concat of the noisy latent with
[mask | masked-image latent], cross-attention context) -> `UNetModel.forward` is exercised; VAE encode/decode and the
prompt encoder stay PyTorch-ROCm host code as the north star prescribes.
"""
import contextlib

import numpy as np
import torch
import torch.nn as nn

from leftrefill_amd import ops
from ldm.models.diffusion.ddim import CFGModelEval, DDIMSampler
from ldm.modules.diffusionmodules.util import extract_into_tensor, make_beta_schedule, noise_like
from leftrefill_amd import noise as lrn
from ldm.modules.distributions.distributions import DiagonalGaussianDistribution
from ldm.util import default, exists, instantiate_from_config


def disabled_train(self, mode=True):
    return self


class DiffusionWrapper(nn.Module):
    """Conditioning router (reference 1327-1371).  state-dict prefix: `model.diffusion_model.*`."""

    def __init__(self, diff_model_config, conditioning_key):
        super().__init__()
        self.sequential_cross_attn = diff_model_config.pop("sequential_crossattn", False)
        self.diffusion_model = instantiate_from_config(diff_model_config)
        self.conditioning_key = conditioning_key
        assert self.conditioning_key in [None, 'concat', 'crossattn', 'hybrid', 'adm', 'hybrid-adm', 'crossattn-adm',
                                         'hybrid-refine']

    def forward(self, x, t, c_concat: list = None, c_crossattn: list = None, c_adm=None, c_input=None):
        key = self.conditioning_key
        if key is None:
            raise NotImplementedError("unconditional UNet is not a LeftRefill configuration")
        if key == 'concat':
            raise NotImplementedError("LeftRefill's UNet always has a cross-attention context")
        if key == 'crossattn':
            cc = torch.cat(c_crossattn, 1)
            return self.diffusion_model(x, t, context=cc)
        if key == 'hybrid':
            # channel order [noisy z 0-3 | mask 4 | masked-image latent 5-8] (reference 1348-1351, 1662, 1679-1690)
            xc = torch.cat([x] + c_concat, dim=1)
            # a single context tensor is passed through as-is (torch.cat would copy it every step and defeat the
            # UNet's per-context K/V cache); the value is identical
            cc = c_crossattn[0] if len(c_crossattn) == 1 else torch.cat(c_crossattn, 1)
            if c_input is not None:      # NVS input refinement (reference 1355, inpainting_ldm/NVS_ldm.py:64-68)
                return self.diffusion_model(xc, t, context=cc, c_input=c_input)
            return self.diffusion_model(xc, t, context=cc)
        raise NotImplementedError(f"conditioning_key {key!r} is not used by the inpainting path")


class DDPM(nn.Module):
    """Noise schedule buffers (reference register_schedule 149-203) + the attributes DDIMSampler reads."""

    def __init__(self, unet_config, timesteps=1000, beta_schedule="linear", loss_type="l2", ckpt_path=None,
                 ignore_keys=(), load_only_unet=False, monitor="val/loss", use_ema=True, first_stage_key="image",
                 image_size=256, channels=3, log_every_t=100, clip_denoised=True, linear_start=1e-4, linear_end=2e-2,
                 cosine_s=8e-3, given_betas=None, original_elbo_weight=0., v_posterior=0., l_simple_weight=1.,
                 conditioning_key=None, parameterization="eps", scheduler_config=None, use_positional_encodings=False,
                 learn_logvar=False, logvar_init=0., make_it_fit=False, ucg_training=None, reset_ema=False,
                 reset_num_ema_updates=False, **ignored):
        super().__init__()
        assert parameterization in ["eps", "x0", "v"]
        self.parameterization = parameterization
        self.cond_stage_model = None
        self.clip_denoised = clip_denoised
        self.log_every_t = log_every_t
        self.first_stage_key = first_stage_key
        self.image_size = image_size
        self.channels = channels
        self.use_positional_encodings = use_positional_encodings
        self.model = DiffusionWrapper(unet_config, conditioning_key)
        self.use_ema = False  # every LeftRefill config sets use_ema: False
        self.use_scheduler = scheduler_config is not None
        self.ucg_training = ucg_training or {}
        self.ucg_prng = np.random.RandomState()
        self.trainer = None      # leftrefill_amd.trainer.Trainer sets itself here and serves global_step / local_rank / log
        self.loss_scale = None
        self.v_posterior = v_posterior
        self.original_elbo_weight = original_elbo_weight
        self.l_simple_weight = l_simple_weight
        self.loss_type = loss_type
        self.learn_logvar = learn_logvar
        self.register_schedule(given_betas=given_betas, beta_schedule=beta_schedule, timesteps=timesteps,
                               linear_start=linear_start, linear_end=linear_end, cosine_s=cosine_s)
        logvar = torch.full(fill_value=float(logvar_init), size=(self.num_timesteps,))     # reference 129-134
        if learn_logvar:
            self.logvar = nn.Parameter(logvar, requires_grad=True)
        else:
            self.register_buffer('logvar', logvar)

    @property
    def device(self):
        return self.betas.device

    def register_schedule(self, given_betas=None, beta_schedule="linear", timesteps=1000, linear_start=1e-4,
                          linear_end=2e-2, cosine_s=8e-3):
        betas = given_betas if exists(given_betas) else make_beta_schedule(beta_schedule, timesteps, linear_start,
                                                                           linear_end, cosine_s)
        betas = np.asarray(betas, dtype=np.float64)
        ac = np.cumprod(1. - betas, axis=0)
        ac_prev = np.append(1., ac[:-1])
        self.num_timesteps = int(betas.shape[0])
        self.linear_start, self.linear_end = linear_start, linear_end
        f32 = lambda a: torch.tensor(a, dtype=torch.float32)
        for name, val in (("betas", betas), ("alphas_cumprod", ac), ("alphas_cumprod_prev", ac_prev),
                          ("sqrt_alphas_cumprod", np.sqrt(ac)), ("sqrt_one_minus_alphas_cumprod", np.sqrt(1. - ac)),
                          ("log_one_minus_alphas_cumprod", np.log(1. - ac)),
                          ("sqrt_recip_alphas_cumprod", np.sqrt(1. / ac)),
                          ("sqrt_recipm1_alphas_cumprod", np.sqrt(1. / ac - 1))):
            self.register_buffer(name, f32(val))
        # variational-bound weights of the training loss (reference 176-203), eps-parameterisation
        alphas = 1. - betas
        post_var = (1 - self.v_posterior) * betas * (1. - ac_prev) / (1. - ac) + self.v_posterior * betas
        self.register_buffer("posterior_variance", f32(post_var))
        # the posterior tables of the ancestral sampler (reference 185-189), float64 -> fp32.  Non-persistent: state_dict() keeps the
        # keys it had before these tables existed, so checkpoints written by this package keep loading strictly; a reference
        # checkpoint that carries the three keys goes through the tolerant loader, and the values are functions of betas anyway.
        for name, val in (("posterior_log_variance_clipped", np.log(np.maximum(post_var, 1e-20))),
                          ("posterior_mean_coef1", betas * np.sqrt(ac_prev) / (1. - ac)),
                          ("posterior_mean_coef2", (1. - ac_prev) * np.sqrt(alphas) / (1. - ac))):
            self.register_buffer(name, f32(val), persistent=False)
        self._ddpm_host_tables = None
        if self.parameterization == "eps":
            lvlb = self.betas ** 2 / (2 * self.posterior_variance * f32(alphas) * (1 - self.alphas_cumprod))
        elif self.parameterization == "x0":
            lvlb = 0.5 * torch.sqrt(f32(ac)) / (2. * 1 - f32(ac))
        else:
            lvlb = torch.ones_like(self.betas)
        lvlb[0] = lvlb[1]
        self.register_buffer("lvlb_weights", lvlb, persistent=False)

    def get_loss(self, pred, target, mean=True):
        """reference 378-391 (under the reference's autocast the fp16 prediction is promoted to fp32 here)"""
        pred = pred.to(target.dtype)
        if self.loss_type == 'l1':
            loss = (target - pred).abs()
            return loss.mean() if mean else loss
        if self.loss_type == 'l2':
            return torch.nn.functional.mse_loss(target, pred, reduction='mean' if mean else 'none')
        raise NotImplementedError(f"unknown loss type '{self.loss_type}'")

    def q_sample(self, x_start, t, noise=None):
        noise = default(noise, lambda: torch.randn_like(x_start))
        return (extract_into_tensor(self.sqrt_alphas_cumprod, t, x_start.shape) * x_start +
                extract_into_tensor(self.sqrt_one_minus_alphas_cumprod, t, x_start.shape) * noise)

    def q_mean_variance(self, x_start, t):
        """q(x_t | x_0): (mean, variance, log_variance) (reference 283-293)"""
        mean = extract_into_tensor(self.sqrt_alphas_cumprod, t, x_start.shape) * x_start
        variance = extract_into_tensor(1.0 - self.alphas_cumprod, t, x_start.shape)
        log_variance = extract_into_tensor(self.log_one_minus_alphas_cumprod, t, x_start.shape)
        return mean, variance, log_variance

    def predict_start_from_noise(self, x_t, t, noise):
        """reference 295-299"""
        return (extract_into_tensor(self.sqrt_recip_alphas_cumprod, t, x_t.shape) * x_t -
                extract_into_tensor(self.sqrt_recipm1_alphas_cumprod, t, x_t.shape) * noise)

    def q_posterior(self, x_start, x_t, t):
        """q(x_{t-1} | x_t, x_0): (mean, variance, log_variance_clipped) (reference 315-322)"""
        posterior_mean = (extract_into_tensor(self.posterior_mean_coef1, t, x_t.shape) * x_start +
                          extract_into_tensor(self.posterior_mean_coef2, t, x_t.shape) * x_t)
        posterior_variance = extract_into_tensor(self.posterior_variance, t, x_t.shape)
        posterior_log_variance_clipped = extract_into_tensor(self.posterior_log_variance_clipped, t, x_t.shape)
        return posterior_mean, posterior_variance, posterior_log_variance_clipped

    def p_sample_loop(self, *args, **kwargs):
        raise NotImplementedError("DDPM.p_sample_loop (unconditional) is not supported by this build: the UNet always has a "
                                  "context; use LatentDiffusion.p_sample_loop / sample")

    def sample(self, *args, **kwargs):
        raise NotImplementedError("DDPM.sample (unconditional) is not supported by this build: the UNet always has a context; "
                                  "use LatentDiffusion.sample")

    # ---- what PyTorch-Lightning gives a LightningModule, served by leftrefill_amd.trainer.Trainer ---------------------------------
    @property
    def global_step(self):
        return getattr(self.trainer, "global_step", 0)

    @property
    def current_epoch(self):
        return getattr(self.trainer, "current_epoch", 0)

    @property
    def local_rank(self):
        return getattr(self.trainer, "local_rank", 0)

    def optimizers(self):
        return self.trainer.optimizer

    def _log(self, name, value, **kw):      # `self.log` exists only while a trainer serves it (it installs log / log_dict on the module)
        log = getattr(self, "log", None)
        if log is not None:
            log(name, value, **kw)

    # ---- training hooks (reference 438-482) ------------------------------------------------------------------------------------------
    def shared_step(self, batch):
        return self(self.get_input(batch, self.first_stage_key))

    def training_step(self, batch, batch_idx):
        for k, ucg in self.ucg_training.items():      # unconditional-guidance training: blank entry i of key k with probability p
            p, val = ucg["p"], ("" if ucg["val"] is None else ucg["val"])
            for i in range(len(batch[k])):
                if self.ucg_prng.choice(2, p=[1 - p, p]):
                    batch[k][i] = val
        loss, loss_dict = self.shared_step(batch)
        for k, v in loss_dict.items():
            self._log(k, v, prog_bar=True, logger=True, on_step=True, on_epoch=True)
        self._log("global_step", self.global_step, prog_bar=True, logger=True, on_step=True, on_epoch=False)
        if self.use_scheduler:
            self._log("lr_abs", self.optimizers().param_groups[0]["lr"], prog_bar=True, logger=True, on_step=True, on_epoch=False)
        self.loss_dict = loss_dict
        return loss

    def on_train_batch_end(self, *args, **kwargs):
        # None unless precision 16; the scale stays a device scalar: reading it here would put a host sync back into every step
        get_scale = getattr(self.trainer, "loss_scale_after_step", None)
        if get_scale is not None:
            self.loss_scale = get_scale()

    def get_input(self, batch, k):
        x = batch[k]
        if x.dim() == 3:
            x = x[..., None]
        return x.permute(0, 3, 1, 2).to(memory_format=torch.contiguous_format).float()   # 'b h w c -> b c h w'


class LatentDiffusion(DDPM):
    def __init__(self, first_stage_config, cond_stage_config, num_timesteps_cond=None, cond_stage_key="image",
                 cond_stage_trainable=False, concat_mode=True, cond_stage_forward=None, conditioning_key=None,
                 scale_factor=1.0, scale_by_std=False, force_null_conditioning=False, *args, **kwargs):
        self.force_null_conditioning = force_null_conditioning
        self.num_timesteps_cond = default(num_timesteps_cond, 1)
        self.scale_by_std = scale_by_std
        if conditioning_key is None:
            conditioning_key = 'concat' if concat_mode else 'crossattn'
        if cond_stage_config == '__is_unconditional__' and not force_null_conditioning:
            conditioning_key = None
        kwargs.pop("ckpt_path", None)
        kwargs.pop("ignore_keys", None)
        super().__init__(conditioning_key=conditioning_key, *args, **kwargs)
        self.concat_mode = concat_mode
        self.cond_stage_trainable = cond_stage_trainable
        self.cond_stage_key = cond_stage_key
        self.scale_factor = scale_factor
        self.cond_stage_forward = cond_stage_forward
        self.first_stage_model = instantiate_from_config(first_stage_config)
        if self.first_stage_model is not None:
            self.first_stage_model.eval()
            self.first_stage_model.train = disabled_train
            for p in self.first_stage_model.parameters():
                p.requires_grad = False
        if cond_stage_config == "__is_first_stage__":
            self.cond_stage_model = self.first_stage_model
        elif cond_stage_config == "__is_unconditional__":
            self.cond_stage_model = None
        else:
            self.cond_stage_model = instantiate_from_config(cond_stage_config)

    # ---- first stage (KL-VAE; PyTorch-ROCm host code) -----------------------------------------------------------
    def get_first_stage_encoding(self, encoder_posterior, noise=None):
        """noise: a ready standard-normal tensor for the posterior sample (DiagonalGaussianDistribution.sample), or None."""
        if isinstance(encoder_posterior, DiagonalGaussianDistribution):
            z = encoder_posterior.sample(noise=noise)
        elif isinstance(encoder_posterior, torch.Tensor):
            z = encoder_posterior
        else:
            raise NotImplementedError(f"encoder_posterior of type '{type(encoder_posterior)}' not yet implemented")
        return self.scale_factor * z

    @torch.no_grad()
    def encode_first_stage(self, x):
        return self.first_stage_model.encode(x)

    @torch.no_grad()
    def decode_first_stage(self, z, predict_cids=False, force_not_quantize=False):
        return self.first_stage_model.decode(1. / self.scale_factor * z)

    def get_learned_conditioning(self, c):
        m = self.cond_stage_model
        if self.cond_stage_forward is None:
            if hasattr(m, 'encode') and callable(m.encode):
                c = m.encode(c)
                if isinstance(c, DiagonalGaussianDistribution):
                    c = c.mode()
            else:
                c = m(c)
        else:
            c = getattr(m, self.cond_stage_forward)(c)
        return c

    def get_input(self, batch, k, return_first_stage_outputs=False, force_c_encode=False, cond_key=None,
                  return_original_cond=False, bs=None, return_x=False):
        x = super().get_input(batch, k)
        if bs is not None:
            x = x[:bs]
        x = x.to(self.device)
        z = self.get_first_stage_encoding(self.encode_first_stage(x)).detach()
        c, xc = None, None
        if self.model.conditioning_key is not None and not self.force_null_conditioning:
            cond_key = default(cond_key, self.cond_stage_key)
            if cond_key == self.first_stage_key:
                xc = x
            elif cond_key in ('caption', 'coordinates_bbox', 'txt'):
                xc = batch[cond_key]
            elif cond_key == "txt+rel_pose":
                xc = [batch['txt'], batch['rel_pose'].to(self.device)]
            else:
                xc = super().get_input(batch, cond_key).to(self.device)
            if not self.cond_stage_trainable or force_c_encode:
                c = self.get_learned_conditioning(xc if isinstance(xc, (dict, list)) else xc.to(self.device))
            else:
                c = xc
            if bs is not None:
                c = c[:bs]
        out = [z, c]
        if return_first_stage_outputs:
            out.extend([x, self.decode_first_stage(z)])
        if return_x:
            out.append(x)
        if return_original_cond:
            out.append(xc)
        return out

    # ---- the hot path ---------------------------------------------------------------------------------------------
    def apply_model(self, x_noisy, t, cond, return_ids=False):
        """reference 865-880: dict cond (hybrid) is passed through; otherwise wrapped by the conditioning key."""
        if not isinstance(cond, dict):
            if not isinstance(cond, list):
                cond = [cond]
            cond = {('c_concat' if self.model.conditioning_key == 'concat' else 'c_crossattn'): cond}
        out = self.model(x_noisy, t, **cond)
        if isinstance(out, tuple) and not return_ids:
            return out[0]
        return out

    # ---- ancestral DDPM sampling (reference 937-1136) -------------------------------------------------------------------------
    # Per step: one model evaluation at batch B (a replay of the captured UNet step, the one a scale-1 DDIM run of the same batch
    # and conditioning uses) and ONE lr_ddpm_step launch, which also does the known-region blend of a masked run.  The loops step
    # the whole batch at one timestep they know on the host, so nothing is read back from the device; a direct p_sample call
    # reads its `t` back once and issues one launch per run of equal t.
    def _ddpm_unsupported(self, who, **flags):
        bad = [k for k, v in flags.items() if v]
        if bad:
            raise NotImplementedError(f"{who}: {' / '.join(bad)} is not supported by this build (eps-parameterisation, no score "
                                      "corrector, no quantisation of the denoised latent, no shortened conditioning schedule)")
        if self.parameterization != "eps":
            raise NotImplementedError(f"{who}: parameterization {self.parameterization!r} is not supported by this build "
                                      "(LeftRefill samples in the eps-parameterisation)")

    def _ddpm_tables(self):
        """The fp32 tables the posterior step reads, on the host: one download per model (and per schedule), not per step.
        std = exp(0.5 logvar) is formed in fp32 in the reference's order, (0.5 * v).exp() on an fp32 value."""
        tab = self._ddpm_host_tables
        if tab is None or tab["src"] is not self.posterior_log_variance_clipped:
            host = lambda b: b.detach().to(torch.float32).cpu()
            lv = host(self.posterior_log_variance_clipped)
            tab = {"src": self.posterior_log_variance_clipped,
                   "recip": host(self.sqrt_recip_alphas_cumprod).tolist(), "recipm1": host(self.sqrt_recipm1_alphas_cumprod).tolist(),
                   "coef1": host(self.posterior_mean_coef1).tolist(), "coef2": host(self.posterior_mean_coef2).tolist(),
                   "std": (0.5 * lv).exp().tolist(), "sa": host(self.sqrt_alphas_cumprod).tolist(),
                   "s1ma": host(self.sqrt_one_minus_alphas_cumprod).tolist()}
            self._ddpm_host_tables = tab
        return tab

    def _model_eval(self):
        """The samplers' machinery around one model evaluation (precomputed embedding rows, host-named timestep), over this model."""
        ev = CFGModelEval()
        ev.model = self
        return ev

    def _posterior_step(self, x, eps, t_host, noise, clip_denoised, return_x0, known=None):
        tab = self._ddpm_tables()
        i = int(t_host)
        if known is not None:
            known = (known[0], known[1], known[2], tab["sa"][i], tab["s1ma"][i])
        return ops.ddpm_step(x, eps.contiguous(), noise, tab["recip"][i], tab["recipm1"][i], tab["coef1"][i], tab["coef2"][i],
                             0.0 if i == 0 else tab["std"][i], clip_denoised=clip_denoised, return_x0=return_x0, known=known)

    def _p_sample(self, ev, x, c, t, t_host, clip_denoised=False, repeat_noise=False, return_x0=False, temperature=1.,
                  noise_dropout=0., known=None, seeded=None):
        """One ancestral step.  t_host: the timestep every entry of `t` holds, as a host integer (the loops), or None (read `t`
        back).  known: None or (x0, mask) -- the blend with q_sample(x0, t) of the masked loops, whose randn_like is drawn AFTER
        the step's own noise, as in the reference.  seeded: None, or (SeededNoise, loop counter): the step's noise and the known
        region's are then the STEP and KNOWN draws of every sample's key (leftrefill_amd/noise.py) and no generator is touched."""
        x = x.float().contiguous()
        with ev._step_hint(t_host):
            eps = self.apply_model(x, t, c)
        if seeded is None:
            noise = noise_like(x.shape, x.device, repeat_noise)      # drawn every step like the reference (986), also at t == 0
        else:
            sn, k = seeded
            noise = (sn.row0() if repeat_noise else sn).normal(lrn.STEP, k, x.shape[1:])
        if temperature != 1.:
            noise = noise * temperature
        if noise_dropout > 0.:
            noise = torch.nn.functional.dropout(noise, p=noise_dropout)
        if known is not None:
            x0, mask = known
            q_noise = torch.randn_like(x0).float() if seeded is None else seeded[0].normal(lrn.KNOWN, seeded[1], x0.shape[1:])
            known = (x0.float().contiguous(), q_noise, mask.to(device=x.device, dtype=torch.float32).contiguous())
        if t_host is not None:
            return self._posterior_step(x, eps, t_host, noise, clip_denoised, return_x0, known)
        assert known is None
        ts = [int(v) for v in t.tolist()]
        assert len(ts) == x.shape[0], "one timestep per sample"
        eps = eps.contiguous()
        prev, rec, b0 = [], [], 0
        while b0 < len(ts):          # one launch per run of equal t
            b1 = b0 + 1
            while b1 < len(ts) and ts[b1] == ts[b0]:
                b1 += 1
            xp, xr = self._posterior_step(x[b0:b1], eps[b0:b1], ts[b0], noise[b0:b1].contiguous(), clip_denoised, return_x0)
            prev.append(xp)
            rec.append(xr)
            b0 = b1
        one = len(prev) == 1
        return (prev[0] if one else torch.cat(prev)), ((rec[0] if one else torch.cat(rec)) if return_x0 else None)

    def p_mean_variance(self, x, c, t, clip_denoised: bool, return_codebook_ids=False, quantize_denoised=False, return_x0=False,
                        score_corrector=None, corrector_kwargs=None):
        """(model_mean, posterior_variance, posterior_log_variance[, x_recon]) in plain torch (reference 937-966); the sampling
        loops do not come through here -- their step is the fused kernel of `p_sample`."""
        self._ddpm_unsupported("LatentDiffusion.p_mean_variance", return_codebook_ids=return_codebook_ids,
                               quantize_denoised=quantize_denoised, score_corrector=score_corrector is not None)
        model_out = self.apply_model(x, t, c)
        x_recon = self.predict_start_from_noise(x, t=t, noise=model_out)
        if clip_denoised:
            x_recon.clamp_(-1., 1.)
        model_mean, posterior_variance, posterior_log_variance = self.q_posterior(x_start=x_recon, x_t=x, t=t)
        if return_x0:
            return model_mean, posterior_variance, posterior_log_variance, x_recon
        return model_mean, posterior_variance, posterior_log_variance

    @torch.no_grad()
    def p_sample(self, x, c, t, clip_denoised=False, repeat_noise=False, return_codebook_ids=False, quantize_denoised=False,
                 return_x0=False, temperature=1., noise_dropout=0., score_corrector=None, corrector_kwargs=None):
        """x_{t-1} ~ p(x_{t-1} | x_t) (reference 969-997): model call + one lr_ddpm_step per run of equal `t` (read back once here;
        the loops name their timestep on the host instead).  Returns x_prev, or (x_prev, x0) with return_x0.
        Inside `with model.seeded_noise(seeds, step=k):` the noise is the STEP draw at loop counter k of every sample's key."""
        self._ddpm_unsupported("LatentDiffusion.p_sample", return_codebook_ids=return_codebook_ids,
                               quantize_denoised=quantize_denoised, score_corrector=score_corrector is not None)
        seeds, step = self._seeded
        sn = lrn.as_seeded(seeds, x.shape[0], x.device)
        x_prev, x0 = self._p_sample(self._model_eval(), x, c, t, None, clip_denoised, repeat_noise, return_x0, temperature,
                                    noise_dropout, seeded=None if sn is None else (sn, int(step)))
        return (x_prev, x0) if return_x0 else x_prev

    @staticmethod
    def _slice_cond(cond, batch_size):
        if cond is None:
            return None
        if isinstance(cond, dict):
            return {key: cond[key][:batch_size] if not isinstance(cond[key], list) else [x[:batch_size] for x in cond[key]]
                    for key in cond}
        return [c[:batch_size] for c in cond] if isinstance(cond, list) else cond[:batch_size]

    # The reference's signatures of the ancestral sampler are kept name for name (p_sample, p_sample_loop and progressive_denoising take
    # no **kwargs), so the samples' keys reach them through the model: `sample(..., seeds=...)` / `sample_log(ddim=False, seeds=...)`
    # set them for the call, and a direct call of a loop or of p_sample is wrapped in `with model.seeded_noise(seeds):`.
    _seeded = (None, 0)

    @contextlib.contextmanager
    def seeded_noise(self, seeds, step=0):
        """While active, p_sample_loop / progressive_denoising / p_sample of this model draw from the samples' keys instead of torch's
        global generator.  seeds: None (the reference's draws), or one key per sample -- B ints, an integer tensor [B] or [B, 2] of
        (seed, sub) rows, or a leftrefill_amd.noise.SeededNoise.  The loops draw the start code (x_T None), every step's noise and the
        known region's q_sample noise (streams START, STEP, KNOWN at step = the loop counter); step names the draw of a direct p_sample."""
        prev = self._seeded
        self._seeded = (seeds, int(step))
        try:
            yield self
        finally:
            self._seeded = prev

    def _start_code(self, shape, device, x_T):
        """(x_T, SeededNoise | None); when the caller gives no x_T it is torch.randn, or the START draw of every sample's key."""
        sn = lrn.as_seeded(self._seeded[0], shape[0], device)
        if x_T is None:
            x_T = torch.randn(shape, device=device) if sn is None else sn.normal(lrn.START, 0, shape[1:])
        return x_T, sn

    def _ancestral_chain(self, who, cond, img, timesteps, step_kwargs, mask, x0, quantize_denoised, score_corrector=None, sn=None):
        """Generator over the chain timesteps-1 .. 0: yields (i, img, x0_partial) after each step.  sn: the samples' keys (SeededNoise)
        or None; the draws of the k-th step executed are named by the loop counter k = timesteps - 1 - i."""
        self._ddpm_unsupported(who, quantize_denoised=quantize_denoised, score_corrector=score_corrector is not None,
                               shorten_cond_schedule=getattr(self, "shorten_cond_schedule", False))
        b = img.shape[0]
        known = None
        if mask is not None:
            assert x0 is not None
            known = (x0, mask)
        ev = self._model_eval()
        ev._prepare_cfg_inputs(cond, None, 1.)
        ev._prepare_timesteps(range(timesteps))
        for i in reversed(range(0, timesteps)):
            ts = torch.full((b,), i, device=img.device, dtype=torch.long)
            img, x0_partial = self._p_sample(ev, img, cond, ts, i, known=known, seeded=None if sn is None else (sn, timesteps - 1 - i),
                                             **step_kwargs(i))
            yield i, img, x0_partial

    @torch.no_grad()
    def progressive_denoising(self, cond, shape, verbose=True, callback=None, quantize_denoised=False, img_callback=None,
                              mask=None, x0=None, temperature=1., noise_dropout=0., score_corrector=None, corrector_kwargs=None,
                              batch_size=None, x_T=None, start_T=None, log_every_t=None):
        """The chain with the x0 predictions as intermediates (reference 1000-1053).  Returns (img, intermediates).
        Seeded draws: inside `with model.seeded_noise(seeds):`."""
        if not log_every_t:
            log_every_t = self.log_every_t
        timesteps = self.num_timesteps
        if batch_size is not None:
            shape = [batch_size] + list(shape)
        else:
            batch_size = shape[0]
        img, sn = self._start_code(shape, self.device, x_T)
        intermediates = []
        cond = self._slice_cond(cond, batch_size)
        if start_T is not None:
            timesteps = min(timesteps, start_T)
        if type(temperature) == float:
            temperature = [temperature] * timesteps
        kw = lambda i: dict(clip_denoised=self.clip_denoised, return_x0=True, temperature=temperature[i],
                            noise_dropout=noise_dropout)
        for i, img, x0_partial in self._ancestral_chain("LatentDiffusion.progressive_denoising", cond, img, timesteps, kw, mask, x0,
                                                        quantize_denoised, score_corrector, sn=sn):
            if i % log_every_t == 0 or i == timesteps - 1:
                intermediates.append(x0_partial)
            if callback:
                callback(i)
            if img_callback:
                img_callback(img, i)
        return img, intermediates

    @torch.no_grad()
    def p_sample_loop(self, cond, shape, return_intermediates=False, x_T=None, verbose=True, callback=None, timesteps=None,
                      quantize_denoised=False, mask=None, x0=None, img_callback=None, start_T=None, log_every_t=None):
        """The ancestral chain from x_T over `timesteps` (default: all) steps (reference 1056-1104).
        Seeded draws: `sample(..., seeds=...)`, or inside `with model.seeded_noise(seeds):`."""
        if not log_every_t:
            log_every_t = self.log_every_t
        img, sn = self._start_code(shape, self.betas.device, x_T)
        intermediates = [img]
        if timesteps is None:
            timesteps = self.num_timesteps
        if start_T is not None:
            timesteps = min(timesteps, start_T)
        if mask is not None:
            assert x0 is not None
            assert x0.shape[2:3] == mask.shape[2:3], "mask and x0 differ in height (the reference's check, 1081)"
        kw = lambda i: dict(clip_denoised=self.clip_denoised)
        for i, img, _ in self._ancestral_chain("LatentDiffusion.p_sample_loop", cond, img, timesteps, kw, mask, x0,
                                               quantize_denoised, sn=sn):
            if i % log_every_t == 0 or i == timesteps - 1:
                intermediates.append(img)
            if callback:
                callback(i)
            if img_callback:
                img_callback(img, i)
        if return_intermediates:
            return img, intermediates
        return img

    @torch.no_grad()
    def sample(self, cond, batch_size=16, return_intermediates=False, x_T=None, verbose=True, timesteps=None,
               quantize_denoised=False, mask=None, x0=None, shape=None, **kwargs):
        """reference 1107-1122.  seeds= (through **kwargs): one key per sample, see `seeded_noise`; None = the reference's draws."""
        if shape is None:
            shape = (batch_size, self.channels, self.image_size, self.image_size)
        cond = self._slice_cond(cond, batch_size)
        with self.seeded_noise(kwargs.get("seeds", self._seeded[0])):
            return self.p_sample_loop(cond, shape, return_intermediates=return_intermediates, x_T=x_T, verbose=verbose,
                                      timesteps=timesteps, quantize_denoised=quantize_denoised, mask=mask, x0=x0)

    @torch.no_grad()
    def sample_log(self, cond, batch_size, ddim, ddim_steps, **kwargs):
        """reference 1125-1136"""
        if ddim:
            ddim_sampler = DDIMSampler(self)
            shape = (self.channels, self.image_size, self.image_size)
            samples, intermediates = ddim_sampler.sample(ddim_steps, batch_size, shape, cond, verbose=False, **kwargs)
        else:
            samples, intermediates = self.sample(cond=cond, batch_size=batch_size, return_intermediates=True, **kwargs)
        return samples, intermediates


    # ---- training objective (reference 849-863, 900-935); the UNet backward runs on the HIP kernels (train_ops) ----------
    def shared_step(self, batch, **kwargs):
        x, c = self.get_input(batch, self.first_stage_key)
        return self(x, c)

    def forward(self, x, c, *args, **kwargs):
        t = torch.randint(0, self.num_timesteps, (x.shape[0],), device=self.device).long()
        assert self.model.conditioning_key is None or c is not None
        return self.p_losses(x, c, t, *args, **kwargs)

    def p_losses(self, x_start, cond, t, noise=None):
        noise = default(noise, lambda: torch.randn_like(x_start))
        x_noisy = self.q_sample(x_start=x_start, t=t, noise=noise)
        model_output = self.apply_model(x_noisy, t, cond)
        prefix = 'train' if self.training else 'val'
        if self.parameterization == "x0":
            target = x_start
        elif self.parameterization == "eps":
            target = noise
        else:
            raise NotImplementedError("v-parameterisation is not used by LeftRefill")
        loss_dict = {}
        loss_simple = self.get_loss(model_output, target, mean=False).mean([1, 2, 3])
        loss_dict[f'{prefix}/loss_simple'] = loss_simple.mean()
        logvar_t = self.logvar[t].to(self.device)
        loss = loss_simple / torch.exp(logvar_t) + logvar_t
        if self.learn_logvar:
            loss_dict[f'{prefix}/loss_gamma'] = loss.mean()
            loss_dict['logvar'] = self.logvar.data.mean()
        loss = self.l_simple_weight * loss.mean()
        loss_vlb = self.get_loss(model_output, target, mean=False).mean(dim=(1, 2, 3))
        loss_vlb = (self.lvlb_weights[t] * loss_vlb).mean()
        loss_dict[f'{prefix}/loss_vlb'] = loss_vlb
        loss = loss + self.original_elbo_weight * loss_vlb
        loss_dict[f'{prefix}/loss'] = loss
        return loss, loss_dict


class LatentFinetuneDiffusion(LatentDiffusion):
    """Keeps `concat_keys` / `finetune_keys` (reference 1512-1548); checkpoint surgery for widened input convs is a
    training-time concern and not reproduced."""

    def __init__(self, concat_keys: tuple, finetune_keys=("model.diffusion_model.input_blocks.0.0.weight",
                                                          "model_ema.diffusion_modelinput_blocks00weight"),
                 keep_finetune_dims=4, c_concat_log_start=None, c_concat_log_end=None, *args, **kwargs):
        super().__init__(*args, **kwargs)
        self.finetune_keys = finetune_keys
        self.concat_keys = concat_keys
        self.keep_dims = keep_finetune_dims
        self.c_concat_log_start = c_concat_log_start
        self.c_concat_log_end = c_concat_log_end


class LatentInpaintDiffusion(LatentFinetuneDiffusion):
    """Mask + masked-image concat conditioning, text via cross-attention (reference 1654-1701)."""

    def __init__(self, concat_keys=("mask", "masked_image"), masked_image_key="masked_image", *args, **kwargs):
        super().__init__(concat_keys, *args, **kwargs)
        self.masked_image_key = masked_image_key
        assert self.masked_image_key in concat_keys

    def get_input(self, batch, k, cond_key=None, bs=None, return_first_stage_outputs=False, force_c_encode=True, seeds=None):
        """seeds: None, or one key per sample (as in DDIMSampler.sample): the posterior sample of the masked-image encoding -- the only
        posterior sample the sampling reads -- is then the POSTERIOR draw of every sample's key instead of the reference's re-seeded
        host draw, whose value for a sample depends on the sample's place in the batch."""
        z, c, x, xrec, xc = super().get_input(batch, self.first_stage_key, return_first_stage_outputs=True,
                                              force_c_encode=force_c_encode, return_original_cond=True, bs=bs)
        assert exists(self.concat_keys)
        c_cat = []
        for ck in self.concat_keys:
            cc = batch[ck].permute(0, 3, 1, 2).to(memory_format=torch.contiguous_format).float()
            if bs is not None:
                cc = cc[:bs]
            cc = cc.to(self.device)
            if ck != self.masked_image_key:
                cc = torch.nn.functional.interpolate(cc, size=z.shape[-2:])      # mask: nearest to latent size
            else:
                posterior = self.encode_first_stage(cc)
                sn = lrn.as_seeded(seeds, cc.shape[0], cc.device) if isinstance(posterior, DiagonalGaussianDistribution) else None
                noise = None if sn is None else sn.normal(lrn.POSTERIOR, 0, posterior.mean.shape[1:])
                cc = self.get_first_stage_encoding(posterior, noise=noise)  # VAE(masked image) * scale_factor
            c_cat.append(cc)
        all_conds = {"c_concat": [torch.cat(c_cat, dim=1)], "c_crossattn": [c]}
        if return_first_stage_outputs:
            return z, all_conds, x, xrec, xc
        return z, all_conds
