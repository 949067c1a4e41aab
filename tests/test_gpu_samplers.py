"""GPU parity of the PLMS and DPM-Solver++ drop-in samplers (tests/golden/samplers.npz, made by tools/make_golden_samplers.py from the
real reference on the CPU): the fused update kernels against single reference steps, the fp32 timestep embedding against the int64
one, the UNet at fractional timesteps against the fp32 oracle, and whole trajectories through RefInpaintLDM (MID UNet, 8x16
latents) against the reference's -- step indexing bit-exact, latents within the drift of a CPU fp16-autocast emulation."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from oracle import ddim_ref, golden_spec as G, unet_ref  # noqa: E402

B_STEP, H, W = 2, 8, 16
SCALE = G.CFG_SCALE


def dev():
    return torch.device("cuda:0")


def _install():
    import leftrefill_amd.dropin as dropin
    dropin.install()


_cache = {}


def model():
    if "m" not in _cache:
        _install()
        from inpainting_ldm.ref_inpainting_ldm import RefInpaintLDM
        cfg = G.CONFIGS[G.TRAJ_CONFIG]
        m = RefInpaintLDM(first_stage_config={"target": "torch.nn.Identity"}, cond_stage_config={"target": "torch.nn.Identity"},
                          unet_config={"target": "ldm.modules.diffusionmodules.openaimodel.UNetModel", "params": cfg.kwargs()},
                          conditioning_key="hybrid", scale_factor=0.18215, linear_start=0.00085, linear_end=0.0120,
                          timesteps=1000, channels=4, data_config={"img_size": 256})
        m.model.diffusion_model.load_state_dict(G.unet_state(G.TRAJ_CONFIG), strict=True)
        _cache["m"] = (m.to(dev()).eval(), cfg)
    return _cache["m"]


def _close(out, ref, name):
    out = out.float().cpu()
    err = (out - ref).abs().max().item()
    print(f"[{name}] max_abs {err:.3e}")
    torch.testing.assert_close(out, ref, rtol=2e-6, atol=2e-6)


# ---- step kernels against single reference steps ------------------------------------------------------------------------------
@pytest.mark.parametrize("case,S,index,n_hist", [("plms_step_h0", 50, 30, 0), ("plms_step_h1", 50, 29, 1), ("plms_step_h2", 50, 28, 2),
                                                 ("plms_step_h3", 50, 17, 3)])
def test_plms_step_kernel(golden, case, S, index, n_hist):
    _install()
    from leftrefill_amd import ops
    g = golden("samplers")
    tabs = ddim_ref.ddim_tables(S, 0.0)
    a_t, a_prev, s1 = tabs["alphas"][index], tabs["alphas_prev"][index], tabs["sqrt_one_minus_alphas"][index]
    x = G.T(case + ".x", (B_STEP, 4, H, W)).to(dev())
    e = G.T(case + ".e", (2 * B_STEP, 4, H, W)).to(dev())
    hist = [G.T(f"{case}.h{j + 1}", (B_STEP, 4, H, W)).to(dev()) for j in range(n_hist)]
    if n_hist == 0:       # two-pass improved Euler: the second evaluation comes from x_mid, the update from x
        from ldm.models.diffusion.plms import EULER_WEIGHTS, PLMS_WEIGHTS
        _, _, e_t = ops.plms_cfg_step(x, e, [], *PLMS_WEIGHTS[0], SCALE, a_t, a_prev, s1)
        e2 = G.T(case + ".e2", (2 * B_STEP, 4, H, W)).to(dev())
        x_prev, p0, none = ops.plms_cfg_step(x, e2, [e_t], *EULER_WEIGHTS, SCALE, a_t, a_prev, s1, write_e=False)
        assert none is None
    else:
        from ldm.models.diffusion.plms import PLMS_WEIGHTS
        x_prev, p0, e_t = ops.plms_cfg_step(x, e, hist, *PLMS_WEIGHTS[n_hist], SCALE, a_t, a_prev, s1)
    _close(e_t, torch.from_numpy(g[case + ".e_t"]), case + " e_t")
    _close(p0, torch.from_numpy(g[case + ".pred_x0"]), case + " pred_x0")
    _close(x_prev, torch.from_numpy(g[case + ".x_prev"]), case + " x_prev")


@pytest.mark.parametrize("case,S,k,order", [("dpm_step_o1", 20, 1, 1), ("dpm_step_o2", 20, 7, 2)])
def test_dpmpp_step_kernel(golden, case, S, k, order):
    _install()
    from leftrefill_amd import ops
    from ldm.models.diffusion.dpm_solver.dpm_solver import NoiseScheduleVP, multistep_plan
    g = golden("samplers")
    plan = multistep_plan(NoiseScheduleVP("discrete", alphas_cumprod=torch.from_numpy(ddim_ref.alphas_cumprod())), S)
    i = k - 1
    assert plan["order"][i] == order
    x = G.T(case + ".x", (B_STEP, 4, H, W)).to(dev())
    e = G.T(case + ".e", (2 * B_STEP, 4, H, W)).to(dev())
    m1 = G.T(case + ".m1", (B_STEP, 4, H, W)).to(dev()) if order == 2 else None
    x_next, x0 = ops.dpmpp_cfg_step(x, e, m1, SCALE, plan["sigma_s"][i], plan["alpha_s"][i], plan["ratio"][i], plan["c"][i],
                                    plan["c_half"][i], plan["inv_r0"][i])
    _close(x0, torch.from_numpy(g[case + ".x0"]), case + " x0")
    _close(x_next, torch.from_numpy(g[case + ".x_next"]), case + " x_next")


def test_step_kernels_vector_and_scalar_paths():
    """numel % 4 == 0 takes the 16-byte path, any other numel the scalar one: both give the eps-dtype CFG combine bit for bit and
    the data prediction of the DPM-Solver++ update, for fp32, fp16 and bf16 eps."""
    from leftrefill_amd import ops
    for n in (4 * 128, 4 * 127 + 3):
        x = G.T("vs.x", (n,)).to(dev())
        for dt in (torch.float32, torch.float16, torch.bfloat16):
            e = G.T("vs.e", (2 * n,)).to(dev()).to(dt)
            h = [G.T(f"vs.h{j}", (n,)).to(dev()) for j in range(3)]
            _, _, e_t = ops.plms_cfg_step(x, e, h, (55, -59, 37, -9), 24, SCALE, 0.5, 0.6, 0.7)
            assert torch.equal(e_t.cpu(), _cfg_cpu(e.cpu(), dt)), (n, dt)
            _, m0 = ops.dpmpp_cfg_step(x, e, h[0], SCALE, 0.9, 0.4, 0.8, -0.3, -0.15, 1.7)
            ref_m0 = (x.cpu() - 0.9 * _cfg_cpu(e.cpu(), dt)) / 0.4
            torch.testing.assert_close(m0.cpu(), ref_m0, rtol=1e-6, atol=1e-5)


def _cfg_cpu(e, dt):
    eu, ec = e.float().chunk(2)
    if dt == torch.float32:
        return eu + SCALE * (ec - eu)
    d = (ec - eu).to(dt).float()
    return (eu + (SCALE * d).to(dt).float()).to(dt).float()


# ---- fp32 timestep embedding ---------------------------------------------------------------------------------------------
def test_timestep_embedding_f32_matches_int64_bytes():
    from leftrefill_amd import ops
    t = torch.arange(0, 1000, device=dev())
    for dt in (torch.float16, torch.bfloat16):
        for dim in (320, 64):
            a = ops.timestep_embedding(t, dim, dt)
            b = ops.timestep_embedding(t.float(), dim, dt)
            assert torch.equal(a.view(torch.int16), b.view(torch.int16))
    tf = torch.tensor([999.0, 949.05, 899.1, 0.25], device=dev())
    ref = unet_ref.timestep_embedding(tf.cpu(), 320)
    out = ops.timestep_embedding(tf, 320).float().cpu()
    torch.testing.assert_close(out, ref.half().float(), rtol=0, atol=2e-3)
    assert not torch.equal(out, ops.timestep_embedding(tf.long(), 320).float().cpu())


def test_unet_at_fractional_timesteps():
    """The UNet embeds a float timestep at its value (no truncation): against the fp32 oracle at those times, as accurate as the
    reference's own fp16-autocast numerics (the whole-UNet criterion of test_gpu_unet.assert_unet_row)."""
    m, cfg = model()
    unet = m.model.diffusion_model
    sd = G.unet_state(G.TRAJ_CONFIG)
    x, _, ctx = G.unet_inputs("unet_frac", cfg, 2, 16, 32, [0, 0])
    t = torch.tensor([949.5498, 499.7], dtype=torch.float32)
    with torch.no_grad():
        y = unet(x.to(dev()), t.to(dev()), ctx.to(dev())).float().cpu()
        ref = unet_ref.unet_forward(sd, cfg, x, t, ctx)
        emul = unet_ref.unet_forward(sd, cfg, x, t, ctx, mode="autocast16").float()
    rel = ((y - ref).norm() / ref.norm()).item()
    rel_e = ((emul - ref).norm() / ref.norm()).item()
    mx, mx_e = (y - ref).abs().max().item(), (emul - ref).abs().max().item()
    print(f"[unet frac t] rel_l2 {rel:.3e} max_abs {mx:.3e} | autocast16 emulation rel_l2 {rel_e:.3e} max_abs {mx_e:.3e}")
    assert rel <= min(rel_e, 4e-3), (rel, rel_e)
    assert mx <= max(2.0 * mx_e, 5e-3), (mx, mx_e)


# ---- whole trajectories --------------------------------------------------------------------------------------------------------
def _emul_eps(sd, cfg, x, t, c_concat, c_cross, uc_cross):
    """CFG eps of the reference's hybrid model under fp16 autocast (oracle emulation), combined in fp16, returned in fp32."""
    B = x.shape[0]
    xc = torch.cat([torch.cat([x] * 2), torch.cat([c_concat] * 2)], dim=1)
    e = unet_ref.unet_forward(sd, cfg, xc, torch.cat([t] * 2), torch.cat([uc_cross, c_cross]), mode="autocast16")
    e_u, e_c = e[:B], e[B:]
    return (e_u + SCALE * (e_c - e_u)).float()


def _emul_plms(sd, cfg, S, x, c_concat, c_cross, uc_cross):
    """PLMS (pseudo linear multistep, eta = 0) from the maths: improved Euler first, then Adams-Bashforth of order 2, 3, 4 on eps."""
    tabs = ddim_ref.ddim_tables(S, 0.0)
    tr = np.flip(tabs["timesteps"])
    f = lambda v: torch.tensor(float(np.float32(v)), dtype=torch.float32)
    B = x.shape[0]

    def upd(x_, e_, idx):
        a_t, a_prev, s1 = f(tabs["alphas"][idx]), f(tabs["alphas_prev"][idx]), f(tabs["sqrt_one_minus_alphas"][idx])
        p0 = (x_ - s1 * e_) / a_t.sqrt()
        return a_prev.sqrt() * p0 + (1. - a_prev).sqrt() * e_

    old = []
    for i, step in enumerate(tr):
        idx = S - i - 1
        e = _emul_eps(sd, cfg, x, torch.full((B,), int(step)), c_concat, c_cross, uc_cross)
        if not old:
            e2 = _emul_eps(sd, cfg, upd(x, e, idx), torch.full((B,), int(tr[min(i + 1, S - 1)])), c_concat, c_cross, uc_cross)
            ep = (e + e2) / 2
        elif len(old) == 1:
            ep = (3 * e - old[-1]) / 2
        elif len(old) == 2:
            ep = (23 * e - 16 * old[-1] + 5 * old[-2]) / 12
        else:
            ep = (55 * e - 59 * old[-1] + 37 * old[-2] - 9 * old[-3]) / 24
        x = upd(x, ep, idx)
        old = (old + [e])[-3:]
    return x


def _emul_dpm(sd, cfg, S, x, c_concat, c_cross, uc_cross):
    """Multistep DPM-Solver++(2M) from the maths: data prediction m = (x - sigma_s e) / alpha_s, first-order step first (and last
    when S < 15), second order in between with D = (m_k - m_{k-1}) / r0."""
    _install()
    from ldm.models.diffusion.dpm_solver.dpm_solver import NoiseScheduleVP, multistep_plan
    p = multistep_plan(NoiseScheduleVP("discrete", alphas_cumprod=torch.from_numpy(ddim_ref.alphas_cumprod())), S)
    f = lambda k, i: torch.tensor(p[k][i], dtype=torch.float32)
    B = x.shape[0]
    m_prev = None
    for i in range(S):
        e = _emul_eps(sd, cfg, x, torch.full((B,), float(p["t_model"][i]), dtype=torch.float32), c_concat, c_cross, uc_cross)
        m = (x - f("sigma_s", i) * e) / f("alpha_s", i)
        if p["order"][i] == 1:
            x = f("ratio", i) * x - f("c", i) * m
        else:
            x = f("ratio", i) * x - f("c", i) * m - f("c_half", i) * (f("inv_r0", i) * (m - m_prev))
        m_prev = m
    return x


TRAJ = [("plms_s10", "plms", 10, 1), ("plms_s10_b2", "plms", 10, 2), ("dpm_s10", "dpm_solver", 10, 1), ("dpm_s20", "dpm_solver", 20, 1)]


@pytest.mark.parametrize("case,sampler,S,B", TRAJ, ids=[c[0] for c in TRAJ])
def test_trajectory(golden, case, sampler, S, B):
    m, cfg = model()
    g = golden("samplers")
    x_T = G.T(case + ".x_T", (B, 4, H, W))
    c_concat = G.T(case + ".c_concat", (B, 5, H, W))
    c_cross = G.T(case + ".c_cross", (B, 77, cfg.context_dim))
    uc_cross = G.T(case + ".uc_cross", (B, 77, cfg.context_dim))
    import ldm.models.diffusion.plms as plms_mod
    calls = {"noise": 0}
    orig_noise = plms_mod.noise_like

    def noise_like(shape, device, repeat=False):
        calls["noise"] += 1
        return orig_noise(shape, device, repeat)

    t_seq = []
    orig_apply = m.apply_model

    def spy(x, t, c, **kw):
        t_seq.append(t[0].item())
        assert x.shape[0] == 2 * B and torch.all(t == t[0])
        assert t.is_floating_point() == (sampler == "dpm_solver")
        return orig_apply(x, t, c, **kw)

    plms_mod.noise_like = noise_like
    m.apply_model = spy
    try:
        cond = {"c_concat": [c_concat.to(dev())], "c_crossattn": [c_cross.to(dev())]}
        uc = {"c_concat": cond["c_concat"], "c_crossattn": [uc_cross.to(dev())]}
        samples, inter = m.sample_log(cond=cond, batch_size=B, ddim=True, ddim_steps=S, eta=0.0, x_T=x_T.to(dev()),
                                      unconditional_guidance_scale=SCALE, unconditional_conditioning=uc, sampler=sampler)
    finally:
        plms_mod.noise_like = orig_noise
        m.apply_model = orig_apply
    ref_t = g[case + ".t_seq"]
    if sampler == "plms":
        assert t_seq == [int(v) for v in ref_t], "PLMS step indexing must be bit-identical"
        assert calls["noise"] == int(g[case + ".noise_calls"])
        assert len(inter["x_inter"]) == g[case + ".x_inter"].shape[0] == len(inter["pred_x0"])
    else:
        assert inter is None
        assert np.array_equal(np.asarray(t_seq, dtype=np.float32).view(np.int32), ref_t.view(np.int32)), "DPM times must be bit-identical"
    sd = G.unet_state(G.TRAJ_CONFIG)
    emul_fn = _emul_plms if sampler == "plms" else _emul_dpm
    with torch.no_grad():
        emul = emul_fn(sd, cfg, S, x_T.clone(), c_concat, c_cross, uc_cross)
    ref = torch.from_numpy(g[case + ".samples"])
    err = (samples.float().cpu() - ref)
    rel = (err.norm() / ref.norm()).item()
    rel_e = ((emul - ref).norm() / ref.norm()).item()
    print(f"[traj {case}] max_abs {err.abs().max().item():.3e} rel_l2 {rel:.3e} | autocast16 emulation rel_l2 {rel_e:.3e} "
          f"| scale {ref.abs().max().item():.2f}")
    assert torch.isfinite(samples).all()
    assert rel <= max(2.0 * rel_e, 5e-3), (rel, rel_e)


def test_dpm_deterministic_and_replays_the_ddim_graph():
    m, cfg = model()
    unet = m.model.diffusion_model
    B = 2
    x_T = G.T("dpmdet.x_T", (B, 4, H, W)).to(dev())
    cond = {"c_concat": [G.T("dpmdet.cc", (B, 5, H, W)).to(dev())], "c_crossattn": [G.T("dpmdet.c", (B, 77, cfg.context_dim)).to(dev())]}
    uc = {"c_concat": cond["c_concat"], "c_crossattn": [G.T("dpmdet.uc", (B, 77, cfg.context_dim)).to(dev())]}
    unet._graphs.clear()
    kw = dict(cond=cond, batch_size=B, ddim=True, ddim_steps=5, eta=0.0, x_T=x_T, unconditional_guidance_scale=SCALE,
              unconditional_conditioning=uc)
    m.sample_log(**kw)
    keys = set(unet._graphs)
    assert len(keys) == 1
    outs = [m.sample_log(sampler="dpm_solver", **kw)[0] for _ in range(2)]
    assert torch.equal(outs[0], outs[1])
    assert set(unet._graphs) == keys, "a DPM-Solver step must replay the graph DDIM captured"
    # the fractional times' rows were precomputed, keyed by their fp32 values
    assert any(isinstance(k, float) and k != int(k) for k in unet._emb_table)
    p = [m.sample_log(sampler="plms", **kw)[0] for _ in range(2)]
    assert torch.equal(p[0], p[1]) and set(unet._graphs) == keys
    assert unet._t_host is None
