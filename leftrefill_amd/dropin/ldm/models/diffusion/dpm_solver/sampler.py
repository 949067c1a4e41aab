"""`ldm.models.diffusion.dpm_solver.sampler.DPMSolverSampler` for the MI355X build (sampling only).

The reference's fixed configuration (ldm/models/diffusion/dpm_solver/sampler.py): DPM-Solver++ (data prediction, Lu et al.
2022), multistep, order 2, time-uniform steps, lower order at the end when steps < 15, no thresholding; `sample` returns
(x, None).  Differences by design (results equal the reference's):
  * dict-of-lists conditioning (LeftRefill's {"c_concat": [...], "c_crossattn": [...]}) works -- the reference concatenates the
    conditioning with torch.cat and cannot take it; the [uncond; cond] batch is built once per sampling;
  * the UNet is fed the reference's continuous fp32 times (999.0, 899.1, ...) and embeds them exactly (lr_timestep_embedding_f32);
  * per step: one replay of the captured UNet step (the same graph DDIM uses) and ONE fused HIP update (lr_dpmpp_cfg_step: CFG
    combine + data prediction + multistep update); every schedule scalar is computed on the host once per sampling.
"""
import torch

from leftrefill_amd import noise as lrn
from leftrefill_amd import ops
from ldm.models.diffusion.ddim import CFGModelEval, DDIMSampler
from .dpm_solver import NoiseScheduleVP, multistep_plan

MODEL_TYPES = {"eps": "noise", "v": "v"}
_PLANS = {}           # (alphas_cumprod bytes, S, lower_order_final) -> multistep_plan

SUPPORTED = "method='multistep', order=2, skip_type='time_uniform', no thresholding, eps-parameterisation"


def _unsupported(what):
    raise NotImplementedError(f"DPMSolverSampler: {what} is not supported by this build ({SUPPORTED}; dict or tensor "
                              "conditioning on one rank)")


class DPMSolverSampler(CFGModelEval):
    def __init__(self, model, **kwargs):
        super().__init__()
        self.model = model
        self.register_buffer('alphas_cumprod', model.alphas_cumprod.detach().to(torch.float32).cpu())

    def register_buffer(self, name, attr):
        setattr(self, name, attr)

    def schedule(self, S, lower_order_final=True):
        """Host tables of an S-step sampling (dpm_solver.multistep_plan): the model times and the per-step scalars.  A few hundred
        small CPU ops: computed once per (schedule, S) and reused by later samplings."""
        key = (self.alphas_cumprod.numpy().tobytes(), int(S), bool(lower_order_final))
        plan = _PLANS.get(key)
        if plan is None:
            ns = NoiseScheduleVP('discrete', alphas_cumprod=self.alphas_cumprod)
            plan = _PLANS[key] = multistep_plan(ns, S, order=2, lower_order_final=lower_order_final)
        return plan

    @torch.no_grad()
    def sample(self, S, batch_size, shape, conditioning=None, callback=None, normals_sequence=None, img_callback=None,
               quantize_x0=False, eta=0., mask=None, x0=None, temperature=1., noise_dropout=0., score_corrector=None,
               corrector_kwargs=None, verbose=True, x_T=None, log_every_t=100, unconditional_guidance_scale=1.,
               unconditional_conditioning=None, method="multistep", order=2, skip_type="time_uniform",
               thresholding=False, lower_order_final=True, dynamic_threshold=None, use_original_steps=False, seeds=None, **kwargs):
        """seeds: None, or one key per sample as in DDIMSampler.sample -- the start code (x_T None) is then the START draw of every
        sample's key; the solver is deterministic afterwards."""
        if method != "multistep":
            _unsupported(f"method {method!r}")
        if order != 2:
            _unsupported(f"order {order}")
        if skip_type != "time_uniform":
            _unsupported(f"skip_type {skip_type!r}")
        if thresholding or dynamic_threshold is not None:
            _unsupported("thresholding")
        if score_corrector is not None:
            _unsupported("score_corrector")
        if use_original_steps:
            _unsupported("use_original_steps")
        if mask is not None:
            _unsupported("mask / x0 blending")
        if self.model.parameterization != "eps":
            _unsupported(f"parameterization {self.model.parameterization!r}")
        if isinstance(conditioning, list):
            _unsupported("list conditioning (the multi-conditioning NVS sampler)")
        scale = float(unconditional_guidance_scale)
        if unconditional_conditioning is not None and scale != 1.:
            from leftrefill_amd import dist as lrd
            if lrd.split_cfg_active():
                _unsupported("split classifier-free guidance across ranks")
        self._warn_conditioning_count(conditioning, batch_size)
        C, H, W = shape
        device = self.model.betas.device
        if x_T is None:
            x = DDIMSampler._start_code(lrn.as_seeded(seeds, batch_size, device), (batch_size, C, H, W), device)
        else:
            x = x_T.to(device=device, dtype=torch.float32)
        x = x.contiguous()
        plan = self.schedule(S, lower_order_final=lower_order_final)
        t_model = [float(v) for v in plan["t_model"]]           # exact fp32 values as python floats
        self._prepare_cfg_inputs(conditioning, unconditional_conditioning, scale)
        unet = self._unet()
        if hasattr(unet, "prepare_timesteps"):
            unet.prepare_timesteps(t_model)
        x0_prev = None
        try:
            for k in range(S):
                t = torch.full((batch_size,), t_model[k], device=device, dtype=torch.float32)
                with self._step_hint(t_model[k]):
                    eps, sc = self._cfg_eps(x, conditioning, t, unconditional_conditioning, scale)
                second = plan["order"][k] == 2
                x, x0 = ops.dpmpp_cfg_step(x, eps, x0_prev if second else None, sc, plan["sigma_s"][k], plan["alpha_s"][k],
                                           plan["ratio"][k], plan["c"][k], plan["c_half"][k] if second else 0.0,
                                           plan["inv_r0"][k] if second else 0.0)
                x0_prev = x0
        finally:
            self._cfg_cache = None
        return x.to(device), None
