"""The host side of the ancestral DDPM sampler against the real reference (tests/golden/ddpm_ancestral.npz, made by
tools/make_golden_ddpm.py): signatures, the posterior tables bit for bit, the plain-torch building blocks, the state-dict keys, the
guidance-scale refusal of sampler="ddpm", and the declaration / binding of the ABI 30 symbols.  The step kernel has no CPU path:
the loops' bookkeeping is pinned on the GPU (tests/test_gpu_ddpm.py)."""
import inspect
import os
import re

import numpy as np
import pytest
import torch

from oracle import golden_spec as G

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
H, W = 8, 16
FN_T = (0, 1, 500, 999)
TABLES = ("posterior_log_variance_clipped", "posterior_mean_coef1", "posterior_mean_coef2", "sqrt_recip_alphas_cumprod",
          "sqrt_recipm1_alphas_cumprod")
# state_dict() of a LatentInpaintDiffusion outside the UNet, as it was before the posterior tables existed
SCHEDULE_KEYS = ['betas', 'alphas_cumprod', 'alphas_cumprod_prev', 'sqrt_alphas_cumprod', 'sqrt_one_minus_alphas_cumprod',
                 'log_one_minus_alphas_cumprod', 'sqrt_recip_alphas_cumprod', 'sqrt_recipm1_alphas_cumprod', 'posterior_variance',
                 'logvar']


def _ddpm():
    import leftrefill_amd.dropin as dropin
    dropin.install()
    import ldm.models.diffusion.ddpm as ddpm
    return ddpm


def _model(timesteps=1000, cls="LatentInpaintDiffusion"):
    ddpm = _ddpm()
    cfg = G.CONFIGS["SMALL"]
    return getattr(ddpm, cls)(first_stage_config={"target": "torch.nn.Identity"}, cond_stage_config={"target": "torch.nn.Identity"},
                              unet_config={"target": "ldm.modules.diffusionmodules.openaimodel.UNetModel", "params": cfg.kwargs()},
                              conditioning_key="hybrid", scale_factor=0.18215, linear_start=0.00085, linear_end=0.0120,
                              timesteps=timesteps, channels=4)


def test_signatures_equal_the_reference(golden):
    g = golden("ddpm_ancestral")
    ddpm = _ddpm()
    sigs = [k for k in g.files if k.startswith("sig.")]
    assert len(sigs) == 9
    for k in sigs:
        _, cls, meth = k.split(".")
        names = [p for p in inspect.signature(getattr(getattr(ddpm, cls), meth)).parameters if p != "self"]
        assert names == [str(n) for n in g[k]], k


def test_reference_defaults_of_the_loops():
    L = _ddpm().LatentDiffusion
    d = lambda meth: {k: p.default for k, p in inspect.signature(getattr(L, meth)).parameters.items()
                      if p.default is not inspect.Parameter.empty}
    assert d("p_sample") == dict(clip_denoised=False, repeat_noise=False, return_codebook_ids=False, quantize_denoised=False,
                                 return_x0=False, temperature=1., noise_dropout=0., score_corrector=None, corrector_kwargs=None)
    assert d("sample") == dict(batch_size=16, return_intermediates=False, x_T=None, verbose=True, timesteps=None,
                               quantize_denoised=False, mask=None, x0=None, shape=None)
    assert d("p_sample_loop") == dict(return_intermediates=False, x_T=None, verbose=True, callback=None, timesteps=None,
                                      quantize_denoised=False, mask=None, x0=None, img_callback=None, start_T=None,
                                      log_every_t=None)


@pytest.mark.parametrize("T_", [1000, 50])
def test_posterior_tables_bit_for_bit(golden, T_):
    g = golden("ddpm_ancestral")
    m = _model(T_)
    for name in TABLES:
        v = getattr(m, name)
        assert v.dtype == torch.float32
        assert np.array_equal(v.numpy(), g[f"tab_T{T_}.{name}"]), name


def test_building_blocks_against_the_reference(golden):
    g = golden("ddpm_ancestral")
    m = _model()
    t = torch.tensor(FN_T, dtype=torch.long)
    shape = (len(FN_T), 4, H, W)
    x_start, x_t, noise = G.T("ddpm_fn.x_start", shape), G.T("ddpm_fn.x_t", shape), G.T("ddpm_fn.noise", shape)
    for k, v in zip(("mean", "variance", "log_variance"), m.q_posterior(x_start, x_t, t)):
        np.testing.assert_allclose(v.numpy(), g["fn.q_posterior." + k], rtol=1e-6, atol=0)
    for k, v in zip(("mean", "variance", "log_variance"), m.q_mean_variance(x_start, t)):
        np.testing.assert_allclose(v.numpy(), g["fn.q_mean_variance." + k], rtol=1e-6, atol=0)
    np.testing.assert_allclose(m.predict_start_from_noise(x_t, t, noise).numpy(), g["fn.predict_start_from_noise"], rtol=1e-6,
                               atol=0)


def test_state_dict_keys_are_unchanged():
    """The three posterior tables are non-persistent: a checkpoint written by this package before they existed loads strictly."""
    m = _model()
    keys = list(m.state_dict())
    unet = [k for k in keys if k.startswith("model.diffusion_model.")]
    assert [k for k in keys if k not in unet] == SCHEDULE_KEYS
    assert {k[len("model.diffusion_model."):] for k in unet} == set(G.unet_state("SMALL"))
    sd = {k: v.clone() for k, v in m.state_dict().items()}
    assert not any("posterior_log_variance_clipped" in k or "posterior_mean_coef" in k for k in sd)
    _model().load_state_dict(sd, strict=True)
    for name in TABLES:
        assert hasattr(m, name)


def test_ddpm_sampler_refuses_a_guidance_scale():
    import leftrefill_amd.dropin as dropin
    dropin.install()
    from inpainting_ldm.ref_inpainting_ldm import RefInpaintLDM, make_sampler
    cfg = G.CONFIGS["SMALL"]
    m = RefInpaintLDM(first_stage_config={"target": "torch.nn.Identity"}, cond_stage_config={"target": "torch.nn.Identity"},
                      unet_config={"target": "ldm.modules.diffusionmodules.openaimodel.UNetModel", "params": cfg.kwargs()},
                      conditioning_key="hybrid", scale_factor=0.18215, linear_start=0.00085, linear_end=0.0120, timesteps=1000,
                      channels=4, data_config={"img_size": 64})
    batch = {"image": torch.zeros(1, 64, 128, 3), "masked_image": torch.zeros(1, 64, 128, 3), "mask": torch.zeros(1, 64, 128, 1),
             "txt": [""]}
    with pytest.raises(ValueError, match="ddim.*plms.*dpm_solver"):
        m.log_images(batch, 1, sampler="ddpm", unconditional_guidance_scale=2.5)
    cond = {"c_concat": [torch.zeros(1, 5, H, W)], "c_crossattn": [torch.zeros(1, 77, cfg.context_dim)]}
    with pytest.raises(ValueError, match="ddim.*plms.*dpm_solver"):
        m.sample_log(cond=cond, batch_size=1, ddim=False, ddim_steps=None, sampler="ddpm", unconditional_guidance_scale=2.5,
                     unconditional_conditioning=cond)
    with pytest.raises(ValueError):
        make_sampler("ddpm", m)


def test_out_of_scope_options_raise():
    m = _model()
    x = torch.zeros(1, 4, H, W)
    t = torch.zeros(1, dtype=torch.long)
    for kw in (dict(quantize_denoised=True), dict(return_codebook_ids=True), dict(score_corrector=object())):
        with pytest.raises(NotImplementedError, match="not supported by this build"):
            m.p_sample(x, None, t, **kw)
    with pytest.raises(NotImplementedError, match="not supported by this build"):
        m.p_sample_loop(None, (1, 4, H, W), quantize_denoised=True)
    ddpm = _ddpm()
    with pytest.raises(NotImplementedError, match="unconditional"):
        ddpm.DDPM.sample(m)


def test_abi_30_symbols_are_declared_and_bound():
    import abi_helpers as abi
    from leftrefill_amd import _lib
    header = abi.header().text
    with open(os.path.join(ROOT, "leftrefill_amd", "csrc", "elementwise.hip")) as f:
        src = f.read()
    assert _lib.ABI_VERSION == 30
    assert re.search(r"lr_abi_version\(void\)\s*\{\s*return 30;", src)
    assert "lr_ddpm_step" in _lib.BF16_TWINS
    for p, ct in zip(abi.c_params("lr_ddpm_step"), _lib.SIGNATURES["lr_ddpm_step"]):
        want = (_lib.c_void_p if "*" in p or "lr_stream_t" in p else _lib.c_int64 if "int64_t" in p else
                _lib.c_float if p.startswith("float") else _lib.c_int)
        assert ct is want, (p, ct)
    assert "ddpm.py:" in header[header.index("ancestral DDPM posterior step"):header.index("int lr_ddpm_step(")]
