"""DDIM encode / stochastic_encode / decode and StructureDDIMSampler, host side (no GPU): the public surface against the reference's
parameter names, the host coefficient tables against the real reference's (tests/golden/ddim_extras.npz, made by
tools/make_golden_ddim_extras.py) and the options this build rejects."""
import inspect

import numpy as np
import pytest
import torch

from oracle import ddim_ref


def _install():
    import leftrefill_amd.dropin as dropin
    dropin.install()


class _Model:
    """What the samplers read from a LatentDiffusion before the first model call."""

    def __init__(self, parameterization="eps"):
        self.num_timesteps = 1000
        self.alphas_cumprod = torch.from_numpy(ddim_ref.alphas_cumprod())
        self.betas = torch.zeros(1000)
        self.parameterization = parameterization

    def apply_model(self, *a, **k):
        raise AssertionError("the model must not be called")


SIGNATURES = [("DDIMSampler", "encode"), ("DDIMSampler", "stochastic_encode"), ("DDIMSampler", "decode"),
              ("StructureDDIMSampler", "__init__"), ("StructureDDIMSampler", "ddim_sampling"),
              ("StructureDDIMSampler", "p_sample_ddim_guide")]


@pytest.mark.parametrize("cls,meth", SIGNATURES, ids=[f"{c}.{m}" for c, m in SIGNATURES])
def test_public_surface_has_the_reference_parameter_names(golden, cls, meth):
    _install()
    import ldm.models.diffusion.ddim as ddim
    assert ddim.__file__.startswith(__import__("leftrefill_amd.dropin", fromlist=["ROOT"]).ROOT)
    ref = [str(n) for n in golden("ddim_extras")[f"sig.{cls}.{meth}"]]
    ours = list(inspect.signature(getattr(getattr(ddim, cls), meth)).parameters)
    ours = [p for p in ours if p != "self"]
    assert [p for p in ours if p in ref] == ref, (ours, ref)
    assert issubclass(ddim.StructureDDIMSampler, ddim.DDIMSampler)


@pytest.mark.parametrize("t_enc", [10, 50])
def test_encode_coefficients_match_reference_bit_for_bit(golden, t_enc):
    _install()
    from ldm.models.diffusion.ddim import DDIMSampler
    s = DDIMSampler(_Model())
    s.make_schedule(50, ddim_eta=0.0, verbose=False)
    c1, c2 = s.encode_coefficients(t_enc)
    g = golden("ddim_extras")
    assert c1.dtype == np.float64 and c2.dtype == np.float64
    assert np.array_equal(c1, g[f"enc_coef_S50_t{t_enc}.c1"])
    assert np.array_equal(c2, g[f"enc_coef_S50_t{t_enc}.c2"])


def test_stochastic_encode_coefficients_match_reference_bit_for_bit(golden):
    _install()
    from ldm.models.diffusion.ddim import DDIMSampler
    s = DDIMSampler(_Model())
    s.make_schedule(50, ddim_eta=0.0, verbose=False)
    g = golden("ddim_extras")
    for t in (torch.from_numpy(g["qs_S50.t"]), list(g["qs_S50.t"])):
        sa, s1ma = s.q_sample_coefficients(t)
        assert sa.dtype == np.float32 and s1ma.dtype == np.float32
        assert np.array_equal(sa.view(np.int32), g["qs_S50.sa"].view(np.int32))
        assert np.array_equal(s1ma.view(np.int32), g["qs_S50.s1ma"].view(np.int32))


def test_trajectory_timestep_feeds_match_reference(golden):
    """encode feeds the loop index 0..t_enc-1 (the reference's quirk), decode the DDIM timesteps below t_start, newest first,
    and the structure sampler runs three-way (batch 3B) for index >= Tm, then two-way (2B)."""
    g = golden("ddim_extras")
    assert list(g["enc_s1.t_seq"]) == list(range(10)) == list(g["enc_s25.t_seq"])
    assert list(g["enc_s25.intermediate_steps"]) == [0, 3, 6, 8, 9]
    _install()
    from ldm.models.diffusion.ddim import DDIMSampler
    s = DDIMSampler(_Model())
    s.make_schedule(50, ddim_eta=0.0, verbose=False)
    assert list(g["sdec.t_seq"]) == [int(v) for v in np.flip(s.ddim_timesteps[:10])]
    for case, B in (("struct_b1", 1), ("struct_b2", 2)):
        assert list(g[case + ".batch_seq"]) == [3 * B] * 5 + [2 * B] * 5


def test_unsupported_options_raise():
    _install()
    from ldm.models.diffusion.ddim import DDIMSampler, StructureDDIMSampler
    s = DDIMSampler(_Model())
    s.make_schedule(10, ddim_eta=0.0, verbose=False)
    x = torch.zeros(1, 4, 8, 16)
    c = torch.zeros(1, 77, 8)
    with pytest.raises(NotImplementedError, match="use_original_steps"):
        s.encode(x, c, 3, use_original_steps=True)
    with pytest.raises(NotImplementedError, match="use_original_steps"):
        s.stochastic_encode(x, torch.tensor([3]), use_original_steps=True)
    with pytest.raises(NotImplementedError, match="use_original_steps"):
        s.decode(x, c, 3, use_original_steps=True)
    v = DDIMSampler(_Model("v"))
    v.make_schedule(10, ddim_eta=0.0, verbose=False)
    with pytest.raises(NotImplementedError, match="parameterization"):
        v.encode(x, c, 3)
    st = StructureDDIMSampler(_Model())
    kw = dict(verbose=False, Tm=5, cond_simple=c, cond_weight=0.7, x_T=x)
    with pytest.raises(NotImplementedError, match="return_attn"):
        st.sample(10, 1, (4, 8, 16), conditioning=c, return_attn=True, **kw)
    with pytest.raises(NotImplementedError, match="use_original_steps"):
        st.make_schedule(10, ddim_eta=0.0, verbose=False)
        st.ddim_sampling(c, (1, 4, 8, 16), ddim_use_original_steps=True, Tm=5, cond_simple=c, cond_weight=0.7, x_T=x)
    with pytest.raises(NotImplementedError, match="parameterization"):
        StructureDDIMSampler(_Model("v")).sample(10, 1, (4, 8, 16), conditioning=c, **kw)
    t = torch.full((1,), 901)
    with pytest.raises(NotImplementedError, match="use_original_steps"):
        st.p_sample_ddim_guide(x, c, c, 0.7, t, 9, use_original_steps=True)
    with pytest.raises(ValueError, match="Tm"):
        st.sample(10, 1, (4, 8, 16), conditioning=c, verbose=False, x_T=x)


def test_three_way_split_cfg_raises(monkeypatch):
    _install()
    from leftrefill_amd import dist as lrd
    from ldm.models.diffusion.ddim import DDIMSampler, StructureDDIMSampler
    monkeypatch.setattr(lrd, "split_cfg_active", lambda: True)
    c = {"c_concat": [torch.zeros(1, 5, 8, 16)], "c_crossattn": [torch.zeros(1, 77, 8)]}
    x = torch.zeros(1, 4, 8, 16)
    st = StructureDDIMSampler(_Model())
    with pytest.raises(NotImplementedError, match="split"):
        st.sample(10, 1, (4, 8, 16), conditioning=c, unconditional_conditioning=c, unconditional_guidance_scale=2.5, verbose=False,
                  Tm=5, cond_simple=c, cond_weight=0.7, x_T=x)
    s = DDIMSampler(_Model())
    s.make_schedule(10, ddim_eta=0.0, verbose=False)
    with pytest.raises(NotImplementedError, match="split"):
        s.encode(x, c, 3, unconditional_guidance_scale=2.5, unconditional_conditioning=c)
