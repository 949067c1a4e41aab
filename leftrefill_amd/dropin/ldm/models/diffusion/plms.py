"""`ldm.models.diffusion.plms.PLMSSampler` for the MI355X build (sampling only).

Same constructor / `make_schedule` / `sample` / `plms_sampling` / `p_sample_plms` surface as the reference
(ldm/models/diffusion/plms.py:11-243) for the paths LeftRefill uses: eps-parameterisation, uniform discretisation, eta = 0,
dict or tensor conditioning, classifier-free guidance with the unconditional batch FIRST (the reference's own sampler
concatenates the conditioning with torch.cat and cannot take LeftRefill's dict-of-lists conditioning).

Pseudo linear multistep (Liu et al. 2022): the eps of step i is a fixed combination of this evaluation's eps and the eps of the
up to three previous steps; the very first step is a two-evaluation improved-Euler step.  Each model evaluation is one replay of
the captured UNet step (shared with DDIMSampler, ddim.CFGModelEval) followed by ONE fused HIP update (lr_plms_cfg_step: CFG
combine + multistep combination + pred_x0 / x_prev), with the schedule on the host -- no device->host sync in the loop.
"""
import numpy as np
import torch

from leftrefill_amd import noise as lrn
from leftrefill_amd import ops
from ldm.models.diffusion.ddim import CFGModelEval, DDIMSampler
from ldm.modules.diffusionmodules.util import noise_like

# (weights of [e, h1, h2, h3], divisor) by the number of history entries; h1 is the newest
PLMS_WEIGHTS = {0: ((1,), 1), 1: ((3, -1), 2), 2: ((23, -16, 5), 12), 3: ((55, -59, 37, -9), 24)}
# second evaluation of the first (improved-Euler) step: (e_next + e) / 2
EULER_WEIGHTS = ((1, 1), 2)


def _unsupported(what):
    raise NotImplementedError(f"PLMSSampler: {what} is not supported by this build (eps-parameterisation, uniform steps, "
                              "eta = 0, dict or tensor conditioning on one rank); DDIMSampler covers it")


class PLMSSampler(CFGModelEval):
    def __init__(self, model, schedule="linear", **kwargs):
        super().__init__()
        self.model = model
        self.ddpm_num_timesteps = model.num_timesteps
        self.schedule = schedule

    def register_buffer(self, name, attr):
        setattr(self, name, attr)

    def make_schedule(self, ddim_num_steps, ddim_discretize="uniform", ddim_eta=0., verbose=True):
        if ddim_eta != 0:
            raise ValueError('ddim_eta must be 0 for PLMS')
        # the DDIM tables of the same steps (reference plms.py:27-50 builds them with the same helpers as ddim.py)
        DDIMSampler.make_schedule(self, ddim_num_steps, ddim_discretize=ddim_discretize, ddim_eta=0., verbose=verbose)

    @torch.no_grad()
    def sample(self, S, batch_size, shape, conditioning=None, callback=None, normals_sequence=None, img_callback=None,
               quantize_x0=False, eta=0., mask=None, x0=None, temperature=1., noise_dropout=0., score_corrector=None,
               corrector_kwargs=None, verbose=True, x_T=None, log_every_t=100, unconditional_guidance_scale=1.,
               unconditional_conditioning=None, dynamic_threshold=None, seeds=None, **kwargs):
        """seeds: None, or one key per sample as in DDIMSampler.sample -- the start code (x_T None) is then the START draw of every
        sample's key.  PLMS is deterministic afterwards; its discarded draws stay discarded (noise_like, the global generator)."""
        if isinstance(conditioning, list):
            _unsupported("list conditioning (the multi-conditioning NVS sampler)")
        self._warn_conditioning_count(conditioning, batch_size)
        self.make_schedule(ddim_num_steps=S, ddim_eta=eta, verbose=verbose)
        C, H, W = shape
        return self.plms_sampling(conditioning, (batch_size, C, H, W), callback=callback, img_callback=img_callback,
                                  quantize_denoised=quantize_x0, mask=mask, x0=x0, ddim_use_original_steps=False,
                                  noise_dropout=noise_dropout, temperature=temperature, score_corrector=score_corrector,
                                  corrector_kwargs=corrector_kwargs, x_T=x_T, log_every_t=log_every_t,
                                  unconditional_guidance_scale=unconditional_guidance_scale,
                                  unconditional_conditioning=unconditional_conditioning, dynamic_threshold=dynamic_threshold,
                                  seeds=seeds)

    def _check(self, use_original_steps=False, quantize_denoised=False, noise_dropout=0., score_corrector=None,
               dynamic_threshold=None, unconditional_conditioning=None, scale=1.):
        if use_original_steps:
            _unsupported("use_original_steps")
        if score_corrector is not None:
            _unsupported("score_corrector")
        if dynamic_threshold is not None:
            _unsupported("dynamic_threshold")
        if quantize_denoised or noise_dropout > 0.:
            _unsupported("quantize_denoised / noise_dropout")
        if self.model.parameterization != "eps":
            _unsupported(f"parameterization {self.model.parameterization!r}")
        if unconditional_conditioning is not None and scale != 1.:
            from leftrefill_amd import dist as lrd
            if lrd.split_cfg_active():
                _unsupported("split classifier-free guidance across ranks")

    @torch.no_grad()
    def plms_sampling(self, cond, shape, x_T=None, ddim_use_original_steps=False, callback=None, timesteps=None,
                      quantize_denoised=False, mask=None, x0=None, img_callback=None, log_every_t=100, temperature=1.,
                      noise_dropout=0., score_corrector=None, corrector_kwargs=None, unconditional_guidance_scale=1.,
                      unconditional_conditioning=None, dynamic_threshold=None, seeds=None):
        self._check(ddim_use_original_steps, quantize_denoised, noise_dropout, score_corrector, dynamic_threshold,
                    unconditional_conditioning, unconditional_guidance_scale)
        if isinstance(cond, list):
            _unsupported("list conditioning (the multi-conditioning NVS sampler)")
        device = self.model.betas.device
        b = shape[0]
        if x_T is None:
            img = DDIMSampler._start_code(lrn.as_seeded(seeds, b, device), shape, device)
        else:
            img = x_T.to(device=device, dtype=torch.float32)
        steps = self.ddim_timesteps
        if timesteps is not None:
            end = int(min(timesteps / steps.shape[0], 1) * steps.shape[0]) - 1
            steps = steps[:end]
        intermediates = {'x_inter': [img], 'pred_x0': [img]}
        time_range = np.flip(steps)
        total_steps = steps.shape[0]
        self._prepare_cfg_inputs(cond, unconditional_conditioning, unconditional_guidance_scale)
        self._prepare_timesteps(time_range)           # every t_next is one of them as well
        old_eps = []                                  # CFG-combined eps of the previous steps (fp32), oldest first
        try:
            for i, step in enumerate(time_range):
                index = total_steps - i - 1
                step_next = int(time_range[min(i + 1, len(time_range) - 1)])
                ts = torch.full((b,), int(step), device=device, dtype=torch.long)
                ts_next = torch.full((b,), step_next, device=device, dtype=torch.long)
                if mask is not None:
                    assert x0 is not None
                    img = self.model.q_sample(x0, ts) * mask + (1. - mask) * img
                img, pred_x0, e_t = self.p_sample_plms(img, cond, ts, index=index, temperature=temperature,
                                                       unconditional_guidance_scale=unconditional_guidance_scale,
                                                       unconditional_conditioning=unconditional_conditioning,
                                                       old_eps=old_eps, t_next=ts_next, t_host=int(step),
                                                       t_next_host=step_next)
                old_eps.append(e_t)
                if len(old_eps) > 3:
                    old_eps.pop(0)
                if callback:
                    callback(i)
                if img_callback:
                    img_callback(pred_x0, i)
                if index % log_every_t == 0 or index == total_steps - 1:
                    intermediates['x_inter'].append(img)
                    intermediates['pred_x0'].append(pred_x0)
        finally:
            self._cfg_cache = None
        return img, intermediates

    def _eval(self, x, c, t, t_host, uc, scale):
        with self._step_hint(t_host):
            return self._cfg_eps(x, c, t, uc, scale)

    @torch.no_grad()
    def p_sample_plms(self, x, c, t, index, repeat_noise=False, use_original_steps=False, quantize_denoised=False,
                      temperature=1., noise_dropout=0., score_corrector=None, corrector_kwargs=None,
                      unconditional_guidance_scale=1., unconditional_conditioning=None, old_eps=None, t_next=None,
                      dynamic_threshold=None, t_host=None, t_next_host=None, **kwargs):
        """Returns (x_prev, pred_x0, e_t): e_t is this step's CFG-combined eps (fp32), the history entry of the next steps.
        t_host / t_next_host: the timesteps of `t` / `t_next` as host integers (None = unknown; only the embedding rows differ)."""
        scale = float(unconditional_guidance_scale)
        self._check(use_original_steps, quantize_denoised, noise_dropout, score_corrector, dynamic_threshold,
                    unconditional_conditioning, scale)
        old_eps = [] if old_eps is None else old_eps
        x = x.float().contiguous()
        device = x.device
        a_t, a_prev = self.ddim_alphas[index], self.ddim_alphas_prev[index]
        s1 = self.ddim_sqrt_one_minus_alphas[index]
        eps, sc = self._eval(x, c, t, t_host, unconditional_conditioning, scale)
        # sigma = 0, but the reference draws its (zero-weighted) noise once per x_prev it forms (plms.py:218): a seeded caller's
        # later random numbers stay where they were
        noise_like(x.shape, device, repeat_noise)
        hist = [h.contiguous() for h in reversed(old_eps[-3:])]            # newest first
        if not hist:
            # improved Euler: x' from e_t, then e_t' = (e_t + e(x', t_next)) / 2 from the same x (plms.py:225-229)
            w, d = PLMS_WEIGHTS[0]
            x_mid, _, e_t = ops.plms_cfg_step(x, eps, [], w, d, sc, a_t, a_prev, s1)
            eps2, sc2 = self._eval(x_mid, c, t_next, t_next_host, unconditional_conditioning, scale)
            noise_like(x.shape, device, repeat_noise)
            w, d = EULER_WEIGHTS
            x_prev, pred_x0, _ = ops.plms_cfg_step(x, eps2, [e_t], w, d, sc2, a_t, a_prev, s1, write_e=False)
            return x_prev, pred_x0, e_t
        w, d = PLMS_WEIGHTS[len(hist)]
        x_prev, pred_x0, e_t = ops.plms_cfg_step(x, eps, hist, w, d, sc, a_t, a_prev, s1)
        return x_prev, pred_x0, e_t
