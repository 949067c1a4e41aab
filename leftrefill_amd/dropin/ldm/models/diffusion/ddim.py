"""`ldm.models.diffusion.ddim.DDIMSampler` for the MI355X build (sampling only).

Same constructor / `sample` / `ddim_sampling` / `p_sample_ddim` / `make_schedule` surface as the reference
(ldm/models/diffusion/ddim.py:11-386) for the paths LeftRefill uses (eps-parameterisation, uniform discretisation,
dict conditioning, classifier-free guidance with the unconditional batch FIRST).

Differences by design (results identical):
  * schedule tables stay on the HOST as float64/fp32 numpy -- the reference builds four `torch.full(...)` from 0-dim
    device tensors per step (ddim.py:359-362), i.e. four device->host syncs per step;
  * the CFG combine + x0 prediction + x_{t-1} update (ddim.py:343-381, ~15 elementwise kernels) is ONE HIP kernel
    (lr_ddim_cfg_step); the UNet step itself is one hipGraph replay.

Also served: `encode` (DDIM inversion, one lr_ddim_inv_cfg_step per evaluation), `stochastic_encode` (lr_ddim_q_sample), `decode`
(ddim.py:389-470) and LeftRefill's `StructureDDIMSampler` (ddim.py:474-647: three-way guidance over [uncond; cond; cond_simple]
for index >= Tm, one lr_ddim_cfg3_step per evaluation, then two-way guidance with cond_simple).  All of them accept dict
conditioning as well as tensors.
"""
import contextlib

import numpy as np
import torch

from leftrefill_amd import ops
from ldm.modules.diffusionmodules.util import make_ddim_sampling_parameters, make_ddim_timesteps, noise_like
from leftrefill_amd import noise as lrn


def _unsupported(who, what):
    raise NotImplementedError(f"{who}: {what} is not supported by this build (eps-parameterisation, uniform DDIM steps, dict or "
                              "tensor conditioning)")


def _cat_cond(parts):
    """torch.cat of conditionings along the batch, in order: dict (of tensors or lists of tensors) or tensor."""
    c = parts[-1]
    if isinstance(c, dict):
        return {k: ([torch.cat([p[k][i] for p in parts]) for i in range(len(c[k]))] if isinstance(c[k], list)
                    else torch.cat([p[k] for p in parts])) for k in c}
    if isinstance(c, torch.Tensor):
        return torch.cat(parts)
    raise NotImplementedError(f"conditioning of type {type(c).__name__} is not supported by this build (dict or tensor)")


class CFGModelEval(object):
    """What every sampler of this package does around one model evaluation (DDIM, PLMS, DPM-Solver++): the [uncond; cond]
    batch built once per sampling, the CFG shared-prefix flag, the embedding rows of every timestep of the sampling computed up
    front and each step's timestep named to the UNet on the host -- so each evaluation is one replay of the same captured step."""

    def _unet(self):
        return getattr(getattr(self.model, "model", None), "diffusion_model", None)

    def _prepare_timesteps(self, steps):
        """The schedule is known before the first step: the UNet computes the embedding rows of all its timesteps in one go
        (UNetModel.prepare_timesteps) and each step names its timestep on the host (`_step_hint`)."""
        unet = self._unet()
        if hasattr(unet, "prepare_timesteps"):
            unet.prepare_timesteps(int(s_) for s_ in steps)

    @contextlib.contextmanager
    def _step_hint(self, step):
        """The model evaluations inside the `with` block run with their host timestep named to the UNet; the name is always cleared
        on the way out.  step: an int, or the exact fp32 value of a continuous time (a python float); None = unknown."""
        unet = self._unet()
        named = hasattr(unet, "prepare_timesteps")
        if named:
            unet._t_host = None if step is None else (step if isinstance(step, float) else int(step))
        try:
            yield
        finally:
            if named:
                unet._t_host = None

    @staticmethod
    def _warn_conditioning_count(conditioning, batch_size, dict_only=False):
        """The reference samplers' notice when the first conditioning entry does not have batch_size rows (DDIM looks at dict
        conditioning only)."""
        if conditioning is None or (dict_only and not isinstance(conditioning, dict)):
            return
        c0 = conditioning[list(conditioning.keys())[0]] if isinstance(conditioning, dict) else conditioning
        while isinstance(c0, list):
            c0 = c0[0]
        if c0.shape[0] != batch_size:
            print(f"Warning: Got {c0.shape[0]} conditionings but batch-size is {batch_size}")

    # the conditioning is constant over the loop: build the [uncond; cond] batch once instead of 50 torch.cat calls
    def _prepare_cfg_inputs(self, c, uc, scale):
        self._cfg_cache = None
        self._cfg_shared = False
        if uc is None or scale == 1. or not isinstance(c, dict):
            return
        c_in = {}
        for k in c:
            if isinstance(c[k], list):
                c_in[k] = [torch.cat([uc[k][i], c[k][i]]) for i in range(len(c[k]))]
            else:
                c_in[k] = torch.cat([uc[k], c[k]])
        self._cfg_cache = (id(c), id(uc), c_in)
        # the two halves of the CFG batch differ only in the cross-attention context when every other conditioning tensor
        # is the same for uncond and cond: checked once per sampling, lets the UNet share the context-free prefix
        import os
        self._cfg_shared = os.environ.get("LEFTREFILL_CFG_SHARED_PREFIX", "1") != "0" and all(
            all(torch.equal(u_, c_) for u_, c_ in zip(uc[k], c[k])) if isinstance(c[k], list) else torch.equal(uc[k], c[k])
            for k in c if k != "c_crossattn")

    def _cfg_eps(self, x, c, t, unconditional_conditioning, scale):
        """One model evaluation on the [uncond; cond] batch (one UNet call, uncond half first, ddim.py:317-342) -> (eps [2B, ...]
        contiguous, the guidance scale to combine it with).  Without an unconditional pass (or at scale 1) the single output is
        returned twice with scale 1.0, so e_u + 1.0 (e_c - e_u) = e.  Split-CFG across ranks is the caller's business."""
        if unconditional_conditioning is None or scale == 1.:
            e = self.model.apply_model(x, t, c)
            return torch.cat([e, e]).contiguous(), 1.0      # degenerate CFG: e_u = e_c = e  ->  e_t = e
        cache = getattr(self, "_cfg_cache", None)
        if cache is not None and cache[0] == id(c) and cache[1] == id(unconditional_conditioning):
            c_in = cache[2]
        elif isinstance(c, torch.Tensor):          # plain-tensor conditioning (apply_model wraps it by the conditioning key)
            c_in = torch.cat([unconditional_conditioning, c])
        else:
            assert isinstance(c, dict) and isinstance(unconditional_conditioning, dict)
            c_in = {k: ([torch.cat([unconditional_conditioning[k][i], c[k][i]]) for i in range(len(c[k]))]
                        if isinstance(c[k], list) else torch.cat([unconditional_conditioning[k], c[k]]))
                    for k in c}
        x_in = torch.cat([x] * 2)
        t_in = torch.cat([t] * 2)
        unet = self._unet()
        shared = (cache is not None and c_in is cache[2] and getattr(self, "_cfg_shared", False)
                  and hasattr(unet, "cfg_shared_prefix"))
        if shared:
            unet.cfg_shared_prefix = True
        try:
            eps = self.model.apply_model(x_in, t_in, c_in)   # [2B, 4, h, w], uncond half first (ddim.py:317-342)
        finally:
            if shared:
                unet.cfg_shared_prefix = False
        return eps.contiguous(), scale

    # three-way guidance of StructureDDIMSampler: the [uncond; cond; cond_simple] batch, built once per sampling like the CFG pair
    def _prepare_cfg3_inputs(self, c, c_simple, uc, scale):
        self._cfg3_cache = None
        if uc is None or scale == 1. or c_simple is None:
            return
        self._cfg3_cache = (id(c), id(c_simple), id(uc), _cat_cond([uc, c, c_simple]))

    def _cfg3_eps(self, x, c, c_simple, t, uc):
        """One model evaluation on the [uncond; cond; cond_simple] batch (one UNet call at 3B, ddim.py:587-604) -> eps [3B, ...]
        contiguous.  No shared prefix: the three thirds are not two equal halves (the flag stays two-way only)."""
        cache = getattr(self, "_cfg3_cache", None)
        if cache is not None and cache[:3] == (id(c), id(c_simple), id(uc)):
            c_in = cache[3]
        else:
            c_in = _cat_cond([uc, c, c_simple])
        eps = self.model.apply_model(torch.cat([x] * 3), torch.cat([t] * 3), c_in)
        return eps.contiguous()


class DDIMSampler(CFGModelEval):
    def __init__(self, model, schedule="linear", **kwargs):
        super().__init__()
        self.model = model
        self.ddpm_num_timesteps = model.num_timesteps
        self.schedule = schedule

    def register_buffer(self, name, attr):
        setattr(self, name, attr)

    def make_schedule(self, ddim_num_steps, ddim_discretize="uniform", ddim_eta=0., verbose=True):
        self.ddim_timesteps = make_ddim_timesteps(ddim_discretize, ddim_num_steps, self.ddpm_num_timesteps,
                                                  verbose=verbose)
        ac = self.model.alphas_cumprod
        assert ac.shape[0] == self.ddpm_num_timesteps, 'alphas have to be defined for each timestep'
        ac32 = ac.detach().to(torch.float32).cpu().numpy()
        self.alphas_cumprod = ac32
        sigmas, alphas, alphas_prev = make_ddim_sampling_parameters(ac32, self.ddim_timesteps, ddim_eta, verbose=verbose)
        self.ddim_sigmas = sigmas
        self.ddim_alphas = alphas
        self.ddim_alphas_prev = alphas_prev
        # sqrt(1 - a_t) is formed in fp32 by the reference (np.sqrt of an fp32 tensor, ddim.py:47)
        a32 = ac32[self.ddim_timesteps]
        self.ddim_sqrt_one_minus_alphas = np.sqrt(np.float32(1) - a32).astype(np.float64)

    @torch.no_grad()
    def sample(self, S, batch_size, shape, conditioning=None, callback=None, normals_sequence=None, img_callback=None,
               quantize_x0=False, eta=0., mask=None, x0=None, temperature=1., noise_dropout=0., score_corrector=None,
               corrector_kwargs=None, verbose=True, x_T=None, log_every_t=100, unconditional_guidance_scale=1.,
               unconditional_conditioning=None, dynamic_threshold=None, ucg_schedule=None, return_attn=False, seeds=None, **kwargs):
        """return_attn: also return `att_scores` (reference ddim.py:139-141), see `ddim_sampling`.
        seeds: None (every draw comes from torch's global generator, as in the reference), or one key per sample -- B ints, an integer
        tensor [B] or [B, 2] of (seed, sub) rows, or a leftrefill_amd.noise.SeededNoise: the start code (x_T None), the noise of every
        step and the q_sample noise of the masked loop are then that sample's own seeded draws (streams START, STEP, KNOWN of
        leftrefill_amd/noise.py at step = the loop counter), the same whatever else is in the batch, and no generator is touched."""
        self._warn_conditioning_count(conditioning, batch_size, dict_only=True)
        if quantize_x0 or score_corrector is not None or dynamic_threshold is not None or noise_dropout > 0.:
            raise NotImplementedError("quantize_x0 / score_corrector / dynamic_threshold / noise_dropout are unused")
        self.make_schedule(ddim_num_steps=S, ddim_eta=eta, verbose=verbose)
        C, H, W = shape
        if isinstance(conditioning, list) and return_attn:
            _unsupported("DDIMSampler", "return_attn with list conditioning (ddim_multi_sampling)")
        if isinstance(conditioning, list):       # NVS consistency sampler (ddim.py:103-120)
            if seeds is not None:
                _unsupported("DDIMSampler", "seeds with list conditioning (ddim_multi_sampling)")
            return self.ddim_multi_sampling(conditioning, (batch_size, C, H, W), callback=callback, temperature=temperature,
                                            x_T=x_T, unconditional_guidance_scale=unconditional_guidance_scale,
                                            unconditional_conditioning=unconditional_conditioning,
                                            ucg_schedule=ucg_schedule)
        return self.ddim_sampling(conditioning, (batch_size, C, H, W), callback=callback, img_callback=img_callback,
                                  mask=mask, x0=x0, temperature=temperature, x_T=x_T, log_every_t=log_every_t,
                                  unconditional_guidance_scale=unconditional_guidance_scale,
                                  unconditional_conditioning=unconditional_conditioning, ucg_schedule=ucg_schedule,
                                  return_attn=return_attn, seeds=seeds)

    @torch.no_grad()
    def ddim_sampling(self, cond, shape, x_T=None, callback=None, timesteps=None, mask=None, x0=None,
                      img_callback=None, log_every_t=100, temperature=1., unconditional_guidance_scale=1.,
                      unconditional_conditioning=None, ucg_schedule=None, return_attn=False, seeds=None, **kwargs):
        """seeds: as in `sample`.
        return_attn: returns (samples, intermediates, att_scores) as the reference does (ddim.py:298-300).  att_scores: a list over
        the UNet's self-attention layers (execution order) of fp32 [b, h_l, w_l] device tensors -- the step mean of the head-averaged
        attention mass every query puts on the reference (left) half of the canvas, recorded by a leftrefill_amd.attnprobe.AttentionProbe
        around the loop (the UNet then runs its eager route) and, under guidance, folded like the reference's scores:
        a_uncond + scale (a_cond - a_uncond) (ddim.py:338-340; once after the step mean, which equals the per-step fold at a constant
        scale -- hence no ucg_schedule)."""
        probe = contextlib.nullcontext()
        if return_attn:
            if ucg_schedule is not None:
                _unsupported("DDIMSampler", "return_attn together with ucg_schedule (the maps are folded once, at one guidance scale)")
            from leftrefill_amd.attnprobe import AttentionProbe
            probe = AttentionProbe(self._unet())
        with probe:
            img, intermediates = self._ddim_loop(cond, shape, x_T, callback, timesteps, mask, x0, img_callback, log_every_t, temperature,
                                                 unconditional_guidance_scale, unconditional_conditioning, ucg_schedule, seeds)
        if return_attn:
            return img, intermediates, self._att_scores(probe, shape[0], unconditional_guidance_scale, unconditional_conditioning)
        return img, intermediates

    @staticmethod
    def _att_scores(probe, b, scale, unconditional_conditioning):
        """The probe's per-layer reference-mass maps as the reference's `att_scores`; the [uncond; cond] halves of a guided batch
        (uncond first, `_prepare_cfg_inputs`) are folded with fold_cfg."""
        from leftrefill_amd.attnprobe import fold_cfg
        guided = unconditional_conditioning is not None and float(scale) != 1.
        maps = []
        for l in probe.recorded:
            m = probe.mass(l)
            assert m.shape[0] == (2 * b if guided else b), f"layer {l}: {m.shape[0]} maps for batch {b}"
            maps.append(fold_cfg(m[:b], m[b:], float(scale)) if guided else m)
        return maps

    @staticmethod
    def _start_code(sn, shape, device):
        """x_T when the caller gives none: torch.randn, or the START draw of every sample's key."""
        return torch.randn(shape, device=device) if sn is None else sn.normal(lrn.START, 0, shape[1:])

    @staticmethod
    def _known_noise(sn, i, x0):
        """The q_sample noise of the known region at loop counter i: None (q_sample draws randn_like) or the KNOWN draw."""
        return None if sn is None else sn.normal(lrn.KNOWN, i, x0.shape[1:])

    @staticmethod
    def _step_noise(shape, device, repeat_noise, seeds, step):
        """The noise of one step: noise_like, or the STEP draw at loop counter `step` (row 0's key for every row under repeat_noise)."""
        if seeds is None:
            return noise_like(shape, device, repeat_noise)
        sn = lrn.as_seeded(seeds, shape[0], device)
        return (sn.row0() if repeat_noise else sn).normal(lrn.STEP, 0 if step is None else step, shape[1:])

    def _ddim_loop(self, cond, shape, x_T, callback, timesteps, mask, x0, img_callback, log_every_t, temperature,
                   unconditional_guidance_scale, unconditional_conditioning, ucg_schedule, seeds=None):
        device = self.model.betas.device
        b = shape[0]
        sn = lrn.as_seeded(seeds, b, device)
        img = self._start_code(sn, shape, device) if x_T is None else x_T.to(device=device, dtype=torch.float32)
        steps = self.ddim_timesteps
        if timesteps is not None:
            end = int(min(timesteps / steps.shape[0], 1) * steps.shape[0]) - 1
            steps = steps[:end]
        intermediates = {'x_inter': [img], 'pred_x0': [img]}
        time_range = np.flip(steps)
        total_steps = steps.shape[0]
        self._prepare_cfg_inputs(cond, unconditional_conditioning, unconditional_guidance_scale)
        self._prepare_timesteps(time_range)
        for i, step in enumerate(time_range):
            index = total_steps - i - 1          # bit-identical step indexing (ddim.py:254)
            ts = torch.full((b,), int(step), device=device, dtype=torch.long)
            if mask is not None:
                assert x0 is not None
                img = self.model.q_sample(x0, ts, noise=self._known_noise(sn, i, x0)) * mask + (1. - mask) * img
            if ucg_schedule is not None:
                unconditional_guidance_scale = ucg_schedule[i]
            # t_host: the timestep of `ts` as a host integer -- p_sample_ddim names it to the UNet around its own model calls
            img, pred_x0 = self.p_sample_ddim(img, cond, ts, index=index, temperature=temperature,
                                              unconditional_guidance_scale=unconditional_guidance_scale,
                                              unconditional_conditioning=unconditional_conditioning, t_host=int(step),
                                              seeds=sn, step=i)
            if callback:
                callback(i)
            if img_callback:
                img_callback(pred_x0, i)
            if index % log_every_t == 0 or index == total_steps - 1:
                intermediates['x_inter'].append(img)
                intermediates['pred_x0'].append(pred_x0)
        self._cfg_cache = None
        return img, intermediates

    @torch.no_grad()
    def ddim_multi_sampling(self, cond, shape, x_T=None, callback=None, timesteps=None, temperature=1.,
                            unconditional_guidance_scale=1., unconditional_conditioning=None, ucg_schedule=None,
                            **kwargs):
        """K conditionings denoised side by side; after every step the right half of ONE of them -- chosen with python's
        `random.shuffle`, consuming the RNG exactly like the reference -- replaces the right half of all K states
        (reference ddim.py:147-222).  Returns (img[0], {})."""
        import random
        device = self.model.betas.device
        b = shape[0]
        K = len(cond)
        if x_T is None:
            first = torch.randn(shape, device=device)       # the reference aliases ONE randn tensor K times (ddim.py:160)
            img = [first] * K
        else:
            img = [x.to(device=device, dtype=torch.float32) for x in x_T]
        ucs = unconditional_conditioning if unconditional_conditioning is not None else [None] * K
        steps = self.ddim_timesteps
        if timesteps is not None:
            end = int(min(timesteps / steps.shape[0], 1) * steps.shape[0]) - 1
            steps = steps[:end]
        total_steps = steps.shape[0]
        self._prepare_timesteps(steps)
        for i, step in enumerate(np.flip(steps)):
            index = total_steps - i - 1
            ts = torch.full((b,), int(step), device=device, dtype=torch.long)
            if ucg_schedule is not None:
                unconditional_guidance_scale = ucg_schedule[i]
            new_img = []
            for img_, cond_, uc_ in zip(img, cond, ucs):
                x_prev, _ = self.p_sample_ddim(img_, cond_, ts, index=index, temperature=temperature,
                                               unconditional_guidance_scale=unconditional_guidance_scale,
                                               unconditional_conditioning=uc_, t_host=int(step))
                new_img.append(x_prev)
            order = list(range(K))
            random.shuffle(order)                 # same RNG consumption and same pick as shuffling the K tensors
            half = new_img[0].shape[-1] // 2
            right = new_img[order[0]][..., half:].clone()
            for x_ in new_img:
                x_[..., half:] = right
            img = new_img
            if callback:
                callback(i)
        return img[0], {}

    @torch.no_grad()
    def p_sample_ddim(self, x, c, t, index, repeat_noise=False, use_original_steps=False, quantize_denoised=False,
                      temperature=1., noise_dropout=0., score_corrector=None, corrector_kwargs=None,
                      unconditional_guidance_scale=1., unconditional_conditioning=None, dynamic_threshold=None,
                      t_host=None, seeds=None, step=None, **kwargs):
        """t_host: the timestep every entry of `t` holds, as a host integer (the sampling loops pass it; None = unknown).  It is named
        to the UNet only around this method's own apply_model calls (precomputed embedding rows, UNetModel.prepare_timesteps).
        seeds, step: the samples' keys (as in `sample`) and the loop counter that names this step's seeded noise; None = noise_like."""
        with self._step_hint(t_host):
            return self._p_sample_ddim(x, c, t, index, repeat_noise, use_original_steps, quantize_denoised, temperature, noise_dropout,
                                       score_corrector, corrector_kwargs, unconditional_guidance_scale, unconditional_conditioning,
                                       dynamic_threshold, seeds, step)

    def _p_sample_ddim(self, x, c, t, index, repeat_noise=False, use_original_steps=False, quantize_denoised=False,
                       temperature=1., noise_dropout=0., score_corrector=None, corrector_kwargs=None,
                       unconditional_guidance_scale=1., unconditional_conditioning=None, dynamic_threshold=None, seeds=None, step=None):
        if use_original_steps or quantize_denoised or score_corrector is not None or dynamic_threshold is not None:
            raise NotImplementedError
        if self.model.parameterization != "eps":
            raise NotImplementedError("LeftRefill samples in the eps-parameterisation")
        x = x.float().contiguous()
        device = x.device
        scale = float(unconditional_guidance_scale)
        if unconditional_conditioning is not None and scale != 1.:
            from leftrefill_amd import dist as lrd
            if lrd.split_cfg_active():
                # cond / uncond passes on two ranks (or, without a process group, one after the other): batch B each, one
                # all-gather of the eps halves per step -- leftrefill_amd/dist.py.  (The [uncond; cond] batch is not built here.)
                # The ranks of a pair must hold the same x and draw the same DDIM noise: the caller seeds them identically
                # (bench.py: seed 1234 + rank // 2), or passes both the same `seeds`.
                role = lrd.split_cfg_role()
                if role is None:
                    # one process runs both passes: each gets its own captured step (graph slot), so the per-context K / V cache
                    # of a slot sees ONE context and is not recomputed twice per DDIM step
                    unet = getattr(getattr(self.model, "model", None), "diffusion_model", None)
                    halves = []
                    for slot, cc in enumerate((unconditional_conditioning, c)):
                        if unet is not None:
                            unet._graph_slot = slot
                        try:
                            halves.append(self.model.apply_model(x, t, cc))
                        finally:
                            if unet is not None:
                                unet._graph_slot = 0
                    eps = torch.cat(halves)
                else:
                    eps = lrd.cfg_exchange(self.model.apply_model(x, t, unconditional_conditioning if role == 0 else c))
                noise = self._step_noise(x.shape, device, repeat_noise, seeds, step)
                sigma = float(self.ddim_sigmas[index])
                return ops.ddim_cfg_step(x, eps.contiguous(), noise, scale, self.ddim_alphas[index], self.ddim_alphas_prev[index],
                                         sigma * float(temperature), self.ddim_sqrt_one_minus_alphas[index])
        eps, scale = self._cfg_eps(x, c, t, unconditional_conditioning, scale)
        # randn is drawn every step like the reference (ddim.py:378), also when sigma_t == 0
        noise = self._step_noise(x.shape, device, repeat_noise, seeds, step)
        sigma = float(self.ddim_sigmas[index])
        x_prev, pred_x0 = ops.ddim_cfg_step(x, eps, noise, scale, self.ddim_alphas[index], self.ddim_alphas_prev[index],
                                            sigma * float(temperature), self.ddim_sqrt_one_minus_alphas[index])
        return x_prev, pred_x0

    def _check_extras(self, who, use_original_steps=False, unconditional_conditioning=None, scale=1.):
        if use_original_steps:
            _unsupported(who, "use_original_steps")
        if self.model.parameterization != "eps":
            _unsupported(who, f"parameterization {self.model.parameterization!r}")
        if unconditional_conditioning is not None and scale != 1.:
            from leftrefill_amd import dist as lrd
            if lrd.split_cfg_active():
                _unsupported(who, "split classifier-free guidance across ranks")

    def encode_coefficients(self, num_steps):
        """(c1, c2) of the first num_steps inversion steps, float64: the reference's 0-dim results (ddim.py:398-400, 417-419), formed in
        its dtype chain -- alphas_next = ddim_alphas (fp32), alphas = torch.tensor(ddim_alphas_prev) (float64).  The kernel applies
        them to fp32 tensors, i.e. rounded to fp32."""
        an = torch.from_numpy(np.asarray(self.ddim_alphas[:num_steps], dtype=np.float32))
        a = torch.tensor(self.ddim_alphas_prev[:num_steps])
        c1 = np.empty(num_steps, dtype=np.float64)
        c2 = np.empty(num_steps, dtype=np.float64)
        for i in range(num_steps):
            c1[i] = (an[i] / a[i]).sqrt().item()
            c2[i] = (an[i].sqrt() * ((1 / an[i] - 1).sqrt() - (1 / a[i] - 1).sqrt())).item()
        return c1, c2

    @torch.no_grad()
    def encode(self, x0, c, t_enc, use_original_steps=False, return_intermediates=None, unconditional_guidance_scale=1.0,
               unconditional_conditioning=None, callback=None):
        """Deterministic DDIM inversion over the first t_enc DDIM steps (ddim.py:389-433): x_next = c1 x + c2 e per step, with
        classifier-free guidance when unconditional_guidance_scale != 1.  Returns (x_next, {'x_encoded', 'intermediate_steps'
        [, 'intermediates']}) with the reference's intermediate-selection rule.

        The model is fed t = i, the LOOP INDEX 0..t_enc-1 (ddim.py:407), not ddim_timesteps[i]: an upstream quirk that this drop-in
        reproduces so that it computes what the reference computes.  Each evaluation is one replay of the captured UNet step
        (the graph DDIM captured, for the same batch and conditioning) and one lr_ddim_inv_cfg_step."""
        scale = float(unconditional_guidance_scale)
        self._check_extras("DDIMSampler.encode", use_original_steps, unconditional_conditioning, scale)
        num_reference_steps = self.ddim_timesteps.shape[0]
        assert t_enc <= num_reference_steps
        num_steps = t_enc
        c1, c2 = self.encode_coefficients(num_steps)
        uc = None
        if scale != 1.:
            assert unconditional_conditioning is not None
            uc = unconditional_conditioning
        x_next = x0
        intermediates = []
        inter_steps = []
        self._prepare_cfg_inputs(c, uc, scale)
        self._prepare_timesteps(range(num_steps))
        try:
            for i in range(num_steps):
                t = torch.full((x0.shape[0],), i, device=x0.device, dtype=torch.long)
                x_in = x_next.float().contiguous()
                with self._step_hint(i):
                    eps, sc = self._cfg_eps(x_in, c, t, uc, scale)
                x_next = ops.ddim_inv_cfg_step(x_in, eps, sc, c1[i], c2[i])
                if return_intermediates and i % (num_steps // return_intermediates) == 0 and i < num_steps - 1:
                    intermediates.append(x_next)
                    inter_steps.append(i)
                elif return_intermediates and i >= num_steps - 2:
                    intermediates.append(x_next)
                    inter_steps.append(i)
                if callback:
                    callback(i)
        finally:
            self._cfg_cache = None
        out = {'x_encoded': x_next, 'intermediate_steps': inter_steps}
        if return_intermediates:
            out.update({'intermediates': intermediates})
        return x_next, out

    def q_sample_coefficients(self, t):
        """(sqrt(ddim_alphas)[t], ddim_sqrt_one_minus_alphas[t]) per sample as fp32 numpy -- what extract_into_tensor gathers in
        stochastic_encode (ddim.py:444-449).  t: DDIM step indices (tensor or sequence); a device tensor is read back once."""
        idx = np.asarray(t.tolist() if isinstance(t, torch.Tensor) else t, dtype=np.int64).reshape(-1)
        sa = np.sqrt(np.asarray(self.ddim_alphas, dtype=np.float32))[idx]
        s1ma = np.asarray(self.ddim_sqrt_one_minus_alphas, dtype=np.float32)[idx]
        return sa, s1ma

    @torch.no_grad()
    def stochastic_encode(self, x0, t, use_original_steps=False, noise=None, seeds=None):
        """Re-noise a clean latent to DDIM step t[b] of each sample (ddim.py:436-449): sqrt(a_t) x0 + sqrt(1 - a_t) noise, one
        lr_ddim_q_sample launch.  noise=None draws randn_like(x0) like the reference, or with `seeds` (as in `sample`) the ENCODE draw
        of every sample's key."""
        if use_original_steps:
            _unsupported("DDIMSampler.stochastic_encode", "use_original_steps")
        sa, s1ma = self.q_sample_coefficients(t)
        assert sa.shape[0] == x0.shape[0], "one DDIM step index per sample"
        if noise is None and seeds is not None:
            noise = lrn.as_seeded(seeds, x0.shape[0], x0.device).normal(lrn.ENCODE, 0, x0.shape[1:])
        if noise is None:
            noise = torch.randn_like(x0)
        return ops.ddim_q_sample(x0.float(), noise.float(), sa, s1ma)

    @torch.no_grad()
    def decode(self, x_latent, cond, t_start, unconditional_guidance_scale=1.0, unconditional_conditioning=None,
               use_original_steps=False, callback=None):
        """Denoise from DDIM step t_start (ddim.py:452-470): p_sample_ddim over ddim_timesteps[:t_start], newest first -- the same
        per-step work as ddim_sampling (precomputed embedding rows, [uncond; cond] batch built once, one graph replay)."""
        self._check_extras("DDIMSampler.decode", use_original_steps)
        steps = self.ddim_timesteps[:t_start]
        time_range = np.flip(steps)
        total_steps = steps.shape[0]
        x_dec = x_latent
        self._prepare_cfg_inputs(cond, unconditional_conditioning, unconditional_guidance_scale)
        self._prepare_timesteps(time_range)
        try:
            for i, step in enumerate(time_range):
                index = total_steps - i - 1
                ts = torch.full((x_latent.shape[0],), int(step), device=x_latent.device, dtype=torch.long)
                x_dec, _ = self.p_sample_ddim(x_dec, cond, ts, index=index,
                                              unconditional_guidance_scale=unconditional_guidance_scale,
                                              unconditional_conditioning=unconditional_conditioning, t_host=int(step))
                if callback:
                    callback(i)
        finally:
            self._cfg_cache = None
        return x_dec


class StructureDDIMSampler(DDIMSampler):
    """LeftRefill's guided sampler (reference ddim.py:474-647): for DDIM index >= Tm a three-way guidance over
    [uncond; cond; cond_simple], e = e_u + s ((w e_c + (1 - w) e_s) - e_u) (ddim.py:607) -- one UNet call at batch 3B (its own
    captured step) and one lr_ddim_cfg3_step; below Tm ordinary DDIM with cond_simple and a copy of the unconditional
    conditioning.  `mask_dir` is accepted and unused, as in the reference (its only use is commented out)."""

    def __init__(self, model, schedule="linear", **kwargs):
        super().__init__(model, schedule, **kwargs)

    @torch.no_grad()
    def sample(self, S, batch_size, shape, conditioning=None, callback=None, normals_sequence=None, img_callback=None,
               quantize_x0=False, eta=0., mask=None, x0=None, temperature=1., noise_dropout=0., score_corrector=None,
               corrector_kwargs=None, verbose=True, x_T=None, log_every_t=100, unconditional_guidance_scale=1.,
               unconditional_conditioning=None, dynamic_threshold=None, ucg_schedule=None, Tm=None, cond_simple=None,
               cond_weight=None, mask_dir='right', seeds=None, **kwargs):
        if isinstance(conditioning, list):       # the reference routes list conditioning to ddim_multi_sampling (no Tm)
            return super().sample(S, batch_size, shape, conditioning=conditioning, callback=callback, img_callback=img_callback,
                                  quantize_x0=quantize_x0, eta=eta, mask=mask, x0=x0, temperature=temperature,
                                  noise_dropout=noise_dropout, score_corrector=score_corrector, verbose=verbose, x_T=x_T,
                                  log_every_t=log_every_t, unconditional_guidance_scale=unconditional_guidance_scale,
                                  unconditional_conditioning=unconditional_conditioning, dynamic_threshold=dynamic_threshold,
                                  ucg_schedule=ucg_schedule, seeds=seeds)
        self._warn_conditioning_count(conditioning, batch_size, dict_only=True)
        self.make_schedule(ddim_num_steps=S, ddim_eta=eta, verbose=verbose)
        C, H, W = shape
        return self.ddim_sampling(conditioning, (batch_size, C, H, W), callback=callback, img_callback=img_callback,
                                  quantize_denoised=quantize_x0, mask=mask, x0=x0, ddim_use_original_steps=False,
                                  noise_dropout=noise_dropout, temperature=temperature, score_corrector=score_corrector,
                                  corrector_kwargs=corrector_kwargs, x_T=x_T, log_every_t=log_every_t,
                                  unconditional_guidance_scale=unconditional_guidance_scale,
                                  unconditional_conditioning=unconditional_conditioning, dynamic_threshold=dynamic_threshold,
                                  ucg_schedule=ucg_schedule, Tm=Tm, cond_simple=cond_simple, cond_weight=cond_weight,
                                  mask_dir=mask_dir, seeds=seeds, **kwargs)

    def _check_guide(self, use_original_steps=False, quantize_denoised=False, noise_dropout=0., score_corrector=None,
                     dynamic_threshold=None, return_attn=False):
        who = "StructureDDIMSampler"
        if return_attn:
            _unsupported(who, "return_attn (the reference's path reads an undefined att_score)")
        if quantize_denoised or noise_dropout > 0. or score_corrector is not None or dynamic_threshold is not None:
            _unsupported(who, "quantize_denoised / noise_dropout / score_corrector / dynamic_threshold")
        self._check_extras(who, use_original_steps)

    @torch.no_grad()
    def ddim_sampling(self, cond, shape, x_T=None, ddim_use_original_steps=False, callback=None, timesteps=None,
                      quantize_denoised=False, mask=None, x0=None, img_callback=None, log_every_t=100, temperature=1.,
                      noise_dropout=0., score_corrector=None, corrector_kwargs=None, unconditional_guidance_scale=1.,
                      unconditional_conditioning=None, dynamic_threshold=None, ucg_schedule=None, Tm=None, cond_simple=None,
                      cond_weight=None, mask_dir='right', seeds=None, **kwargs):
        """seeds: as in DDIMSampler.sample (start code, step noise of both phases, known-region noise)."""
        self._check_guide(ddim_use_original_steps, quantize_denoised, noise_dropout, score_corrector, dynamic_threshold,
                          kwargs.get('return_attn', False))
        if Tm is None or cond_simple is None or cond_weight is None:
            raise ValueError("StructureDDIMSampler needs Tm, cond_simple and cond_weight")
        import copy
        device = self.model.betas.device
        b = shape[0]
        sn = lrn.as_seeded(seeds, b, device)
        img = self._start_code(sn, shape, device) if x_T is None else x_T.to(device=device, dtype=torch.float32)
        steps = self.ddim_timesteps
        if timesteps is not None:
            end = int(min(timesteps / steps.shape[0], 1) * steps.shape[0]) - 1
            steps = steps[:end]
        intermediates = {'x_inter': [img], 'pred_x0': [img]}
        time_range = np.flip(steps)
        total_steps = steps.shape[0]
        # the second phase runs on its own copies of cond_simple and of the unconditional conditioning (ddim.py:517-518)
        new_cond_simple = copy.deepcopy(cond_simple)
        new_uc = copy.deepcopy(unconditional_conditioning)
        scale = unconditional_guidance_scale
        self._prepare_cfg3_inputs(cond, cond_simple, unconditional_conditioning, scale)
        self._prepare_cfg_inputs(new_cond_simple, new_uc, scale)
        self._prepare_timesteps(time_range)
        try:
            for i, step in enumerate(time_range):
                index = total_steps - i - 1
                ts = torch.full((b,), int(step), device=device, dtype=torch.long)
                if mask is not None:
                    assert x0 is not None
                    img = self.model.q_sample(x0, ts, noise=self._known_noise(sn, i, x0)) * mask + (1. - mask) * img
                if ucg_schedule is not None:
                    assert len(ucg_schedule) == len(time_range)
                    scale = ucg_schedule[i]
                if index >= Tm:
                    img, pred_x0 = self.p_sample_ddim_guide(img, cond, cond_simple, cond_weight, ts, index=index,
                                                            temperature=temperature, unconditional_guidance_scale=scale,
                                                            unconditional_conditioning=unconditional_conditioning,
                                                            t_host=int(step), seeds=sn, step=i)
                else:
                    img, pred_x0 = self.p_sample_ddim(img, new_cond_simple, ts, index=index, temperature=temperature,
                                                      unconditional_guidance_scale=scale, unconditional_conditioning=new_uc,
                                                      t_host=int(step), seeds=sn, step=i)
                if callback:
                    callback(i)
                if img_callback:
                    img_callback(pred_x0, i)
                if index % log_every_t == 0 or index == total_steps - 1:
                    intermediates['x_inter'].append(img)
                    intermediates['pred_x0'].append(pred_x0)
        finally:
            self._cfg_cache = None
            self._cfg3_cache = None
        return img, intermediates

    @torch.no_grad()
    def p_sample_ddim_guide(self, x, c, c_simple, c_weight, t, index, repeat_noise=False, use_original_steps=False,
                            quantize_denoised=False, temperature=1., noise_dropout=0., score_corrector=None,
                            corrector_kwargs=None, unconditional_guidance_scale=1., unconditional_conditioning=None,
                            dynamic_threshold=None, t_host=None, seeds=None, step=None, **kwargs):
        """One three-way guided DDIM step (ddim.py:579-647).  Without an unconditional pass (or at scale 1) the model sees c alone
        (ddim.py:585-586) and the step is lr_ddim_cfg_step's.  t_host, seeds, step: as in p_sample_ddim."""
        self._check_guide(use_original_steps, quantize_denoised, noise_dropout, score_corrector, dynamic_threshold,
                          kwargs.get('return_attn', False))
        x = x.float().contiguous()
        scale = float(unconditional_guidance_scale)
        three = unconditional_conditioning is not None and scale != 1.
        if three:
            self._check_extras("StructureDDIMSampler", False, unconditional_conditioning, scale)
        with self._step_hint(t_host):
            if three:
                eps = self._cfg3_eps(x, c, c_simple, t, unconditional_conditioning)
            else:
                eps, _ = self._cfg_eps(x, c, t, None, 1.)
        noise = self._step_noise(x.shape, x.device, repeat_noise, seeds, step)      # drawn every step like the reference (ddim.py:643)
        sigma = float(self.ddim_sigmas[index]) * float(temperature)
        a_t, a_prev, s1 = self.ddim_alphas[index], self.ddim_alphas_prev[index], self.ddim_sqrt_one_minus_alphas[index]
        if not three:
            return ops.ddim_cfg_step(x, eps, noise, 1.0, a_t, a_prev, sigma, s1)
        return ops.ddim_cfg3_step(x, eps, noise, scale, c_weight, a_t, a_prev, sigma, s1)
