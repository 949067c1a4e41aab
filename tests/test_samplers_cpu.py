"""PLMS and DPM-Solver++ drop-in samplers, host side (no GPU): importability after install(), step indexing and the DPM-Solver++
time grid / per-step scalars against the real reference's (tests/golden/samplers.npz, tools/make_golden_samplers.py)."""
import numpy as np
import pytest
import torch

from oracle import ddim_ref


def _install():
    import leftrefill_amd.dropin as dropin
    dropin.install()


class _Model:
    """What the samplers read from a LatentDiffusion before the first model call."""

    def __init__(self):
        ac = torch.from_numpy(ddim_ref.alphas_cumprod())
        self.num_timesteps = 1000
        self.alphas_cumprod = ac
        self.betas = torch.zeros(1000)
        self.parameterization = "eps"

    def apply_model(self, *a, **k):
        raise AssertionError("the model must not be called")


def test_new_samplers_import_after_install():
    _install()
    from ldm.models.diffusion.plms import PLMSSampler
    from ldm.models.diffusion.dpm_solver import DPMSolverSampler
    from ldm.models.diffusion.dpm_solver.sampler import DPMSolverSampler as D2
    assert D2 is DPMSolverSampler
    import ldm.models.diffusion.plms as m
    assert m.__file__.startswith(__import__("leftrefill_amd.dropin", fromlist=["ROOT"]).ROOT)
    assert PLMSSampler is not None


@pytest.mark.parametrize("case", ["plms_s10", "plms_s10_b2"])
def test_plms_timestep_sequence_matches_reference(golden, case):
    """Timesteps fed to the model, in order: each step's t, plus t_next for the second pass of the first step (plms.py:148)."""
    _install()
    from ldm.models.diffusion.plms import PLMSSampler
    s = PLMSSampler(_Model())
    s.make_schedule(10, ddim_eta=0.0, verbose=False)
    time_range = np.flip(s.ddim_timesteps)
    seq = []
    for i, step in enumerate(time_range):
        seq.append(int(step))
        if i == 0:
            seq.append(int(time_range[min(i + 1, len(time_range) - 1)]))
    g = golden("samplers")
    assert seq == list(g[case + ".t_seq"])
    assert len(seq) == int(g[case + ".noise_calls"])        # one noise draw per x_prev formed, like the evaluations


@pytest.mark.parametrize("S", [10, 20, 25])
def test_dpm_time_grid_and_scalars_match_reference(golden, S):
    _install()
    from ldm.models.diffusion.dpm_solver import DPMSolverSampler
    plan = DPMSolverSampler(_Model()).schedule(S)
    g = golden("samplers")
    tag = f"dpm_sched_S{S}"
    t_ref = g[tag + ".t_seq"]
    assert plan["t_model"].dtype == np.float32 and np.array_equal(plan["t_model"].view(np.int32), t_ref.view(np.int32))
    assert list(plan["order"]) == list(g[tag + ".order"])
    for k in ("sigma_s", "alpha_s", "ratio", "c", "inv_r0"):
        ulp = np.abs(plan[k].view(np.int32).astype(np.int64) - g[f"{tag}.{k}"].view(np.int32).astype(np.int64))
        assert ulp.max() <= 2, (k, ulp.max())
    np.testing.assert_array_equal(plan["c_half"], (np.float32(0.5) * plan["c"]).astype(np.float32))


def test_dpm_trajectory_t_seq_is_the_schedule(golden):
    _install()
    from ldm.models.diffusion.dpm_solver import DPMSolverSampler
    g = golden("samplers")
    for case, S in (("dpm_s10", 10), ("dpm_s20", 20)):
        plan = DPMSolverSampler(_Model()).schedule(S)
        assert np.array_equal(plan["t_model"].view(np.int32), g[case + ".t_seq"].view(np.int32))


def test_plms_rejects_eta_and_unsupported_options():
    _install()
    from ldm.models.diffusion.plms import PLMSSampler
    s = PLMSSampler(_Model())
    with pytest.raises(ValueError):
        s.make_schedule(10, ddim_eta=0.5, verbose=False)
    with pytest.raises(ValueError):
        s.sample(10, 1, (4, 8, 16), conditioning=torch.zeros(1, 77, 8), eta=1.0, verbose=False)
    s.make_schedule(10, ddim_eta=0.0, verbose=False)
    x = torch.zeros(1, 4, 8, 16)
    t = torch.full((1,), 901)
    for kw in ({"use_original_steps": True}, {"score_corrector": object()}, {"dynamic_threshold": 1.0}):
        with pytest.raises(NotImplementedError):
            s.p_sample_plms(x, torch.zeros(1, 77, 8), t, 9, old_eps=[], t_next=t, **kw)
    with pytest.raises(NotImplementedError, match="list conditioning"):
        s.sample(10, 1, (4, 8, 16), conditioning=[{"c_crossattn": [torch.zeros(1, 77, 8)]}], verbose=False)


def test_dpm_rejects_unsupported_options():
    _install()
    from ldm.models.diffusion.dpm_solver import DPMSolverSampler
    from ldm.models.diffusion.dpm_solver.dpm_solver import NoiseScheduleVP
    s = DPMSolverSampler(_Model())
    c = torch.zeros(1, 77, 8)
    for kw in ({"method": "singlestep"}, {"method": "adaptive"}, {"order": 3}, {"skip_type": "logSNR"},
               {"thresholding": True}, {"dynamic_threshold": 1.0}, {"score_corrector": object()},
               {"use_original_steps": True}):
        with pytest.raises(NotImplementedError, match="multistep"):
            s.sample(10, 1, (4, 8, 16), conditioning=c, verbose=False, **kw)
    with pytest.raises(NotImplementedError, match="list conditioning"):
        s.sample(10, 1, (4, 8, 16), conditioning=[{"c_crossattn": [c]}], verbose=False)
    with pytest.raises(NotImplementedError):
        NoiseScheduleVP("linear")


def test_split_cfg_raises(monkeypatch):
    _install()
    from leftrefill_amd import dist as lrd
    from ldm.models.diffusion.plms import PLMSSampler
    from ldm.models.diffusion.dpm_solver import DPMSolverSampler
    monkeypatch.setattr(lrd, "split_cfg_active", lambda: True)
    c = {"c_concat": [torch.zeros(1, 5, 8, 16)], "c_crossattn": [torch.zeros(1, 77, 8)]}
    with pytest.raises(NotImplementedError, match="split"):
        DPMSolverSampler(_Model()).sample(10, 1, (4, 8, 16), conditioning=c, unconditional_conditioning=c,
                                          unconditional_guidance_scale=2.5, verbose=False)
    with pytest.raises(NotImplementedError, match="split"):
        PLMSSampler(_Model()).sample(10, 1, (4, 8, 16), conditioning=c, unconditional_conditioning=c,
                                     unconditional_guidance_scale=2.5, verbose=False)
