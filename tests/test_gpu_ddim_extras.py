"""GPU parity of DDIM encode / stochastic_encode / decode and StructureDDIMSampler (tests/golden/ddim_extras.npz, made by
tools/make_golden_ddim_extras.py from the real reference on the CPU): the ABI 28 step kernels against single reference steps and
their bf16 twins against the same formula in torch, whole trajectories through RefInpaintLDM (MID UNet, 8x16 latents) against the
reference's within the drift of a CPU fp16-autocast emulation, graph reuse and determinism."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from oracle import ddim_ref, golden_spec as G, unet_ref  # noqa: E402

B_STEP, H, W = 2, 8, 16
SCALE = G.CFG_SCALE
TM, CW = 5, 0.7


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


class _Sched:
    """What the samplers read from a LatentDiffusion for their host tables."""
    num_timesteps = 1000
    alphas_cumprod = torch.from_numpy(ddim_ref.alphas_cumprod())
    parameterization = "eps"


def _sampler(cls_name, S, m=None):
    _install()
    import ldm.models.diffusion.ddim as ddim
    s = getattr(ddim, cls_name)(m if m is not None else _Sched())
    s.make_schedule(S, ddim_eta=0.0, verbose=False)
    return s


def _within_ulp(out, ref, name, n=1):
    out = out.float().cpu().contiguous().numpy()
    ref = np.ascontiguousarray(ref, dtype=np.float32)
    d = np.abs(out.view(np.int32).astype(np.int64) - ref.view(np.int32).astype(np.int64))
    print(f"[{name}] max ulp {d.max()}")
    assert d.max() <= n, (name, d.max())


# ---- step kernels against single reference steps ------------------------------------------------------------------------------
@pytest.mark.parametrize("dt", [torch.float16, torch.float32], ids=["f16", "f32"])
def test_inv_step_kernel(golden, dt):
    from leftrefill_amd import ops
    g = golden("ddim_extras")
    c1, c2 = _sampler("DDIMSampler", 50).encode_coefficients(31)
    x = G.T("inv_step.x", (B_STEP, 4, H, W)).to(dev())
    e = G.T("inv_step.e", (2 * B_STEP, 4, H, W)).to(dev()).to(dt)
    x_next = ops.ddim_inv_cfg_step(x, e, SCALE, c1[30], c2[30])
    tag = "f16" if dt == torch.float16 else "f32"
    _within_ulp(x_next, g[f"inv_step.{tag}.x_next"], "inv " + tag)


@pytest.mark.parametrize("dt", [torch.float16, torch.float32], ids=["f16", "f32"])
def test_cfg3_step_kernel(golden, dt):
    from leftrefill_amd import ops
    g = golden("ddim_extras")
    s = _sampler("StructureDDIMSampler", 50)
    k = 30
    x = G.T("cfg3_step.x", (B_STEP, 4, H, W)).to(dev())
    e = G.T("cfg3_step.e", (3 * B_STEP, 4, H, W)).to(dev()).to(dt)
    x_prev, p0 = ops.ddim_cfg3_step(x, e, None, SCALE, CW, s.ddim_alphas[k], s.ddim_alphas_prev[k], 0.0,
                                    s.ddim_sqrt_one_minus_alphas[k])
    tag = "f16" if dt == torch.float16 else "f32"
    _within_ulp(p0, g[f"cfg3_step.{tag}.pred_x0"], "cfg3 pred_x0 " + tag)
    _within_ulp(x_prev, g[f"cfg3_step.{tag}.x_prev"], "cfg3 x_prev " + tag)


def _r(v, dt):
    return v.to(dt).float() if dt != torch.float32 else v


def _inv_cpu(x, e, c1, c2, dt):
    eu, ec = e.float().chunk(2)
    ee = _r(eu + _r(SCALE * _r(ec - eu, dt), dt), dt)
    c2_ = torch.tensor(float(c2), dtype=torch.float64).to(dt).float() if dt != torch.float32 else torch.tensor(np.float32(c2))
    return torch.tensor(np.float32(c1)) * x + _r(c2_ * ee, dt)


def _cfg3_cpu(x, e, a_t, a_prev, s1, dt):
    eu, ec, es = e.float().chunk(3)
    if dt == torch.float32:
        ee = eu + SCALE * ((CW * ec + (1 - CW) * es) - eu)
    else:
        m = _r(_r(CW * ec, dt) + _r((1 - CW) * es, dt), dt)
        ee = _r(eu + _r(SCALE * _r(m - eu, dt), dt), dt)
    f = lambda v: torch.tensor(np.float32(v))
    p0 = (x - f(s1) * ee) / f(a_t).sqrt()
    return f(a_prev).sqrt() * p0 + (1.0 - f(a_prev)).sqrt() * ee, p0


def test_twins_and_vector_scalar_paths():
    """fp32, fp16 and bf16 eps on the 16-byte path (numel % 4 == 0) and the scalar one: the same formula run in torch on the CPU,
    every eps-dtype rounding included (the bf16 twins round the combine and c2 e to bf16)."""
    from leftrefill_amd import ops
    s = _sampler("StructureDDIMSampler", 50)
    c1, c2 = s.encode_coefficients(31)
    k = 30
    a_t, a_prev, s1 = s.ddim_alphas[k], s.ddim_alphas_prev[k], s.ddim_sqrt_one_minus_alphas[k]
    for n in (4 * 128, 4 * 127 + 3):
        x = G.T("tw.x", (n,)).to(dev())
        for dt in (torch.float32, torch.float16, torch.bfloat16):
            e2 = G.T("tw.e2", (2 * n,)).to(dev()).to(dt)
            e3 = G.T("tw.e3", (3 * n,)).to(dev()).to(dt)
            xn = ops.ddim_inv_cfg_step(x, e2, SCALE, c1[k], c2[k])
            _within_ulp(xn, _inv_cpu(x.cpu(), e2.cpu(), c1[k], c2[k], dt).numpy(), f"inv n={n} {dt}")
            xp, p0 = ops.ddim_cfg3_step(x, e3, None, SCALE, CW, a_t, a_prev, 0.0, s1)
            rxp, rp0 = _cfg3_cpu(x.cpu(), e3.cpu(), a_t, a_prev, s1, dt)
            _within_ulp(p0, rp0.numpy(), f"cfg3 pred_x0 n={n} {dt}")
            _within_ulp(xp, rxp.numpy(), f"cfg3 x_prev n={n} {dt}")


def test_q_sample_kernel(golden):
    """Bit-exact against the reference's pairs applied in torch, on both paths, and past the per-launch batch bound."""
    from leftrefill_amd import ops
    g = golden("ddim_extras")
    s = _sampler("DDIMSampler", 50)
    for B, per in ((4, 4 * H * W), (4, 3 * 5 * 7), (ops.Q_SAMPLE_MAX_B + 9, 4 * 4 * 4)):
        t = (list(g["qs_S50.t"]) * B)[:B]
        sa, s1ma = s.q_sample_coefficients(torch.tensor(t, device=dev()))
        if B == 4:
            assert np.array_equal(sa, g["qs_S50.sa"]) and np.array_equal(s1ma, g["qs_S50.s1ma"])
        x0 = G.T("qs.x0", (B, per)).to(dev())
        nz = G.T("qs.n", (B, per)).to(dev())
        out = ops.ddim_q_sample(x0, nz, sa, s1ma)
        ref = torch.from_numpy(sa)[:, None] * x0.cpu() + torch.from_numpy(s1ma)[:, None] * nz.cpu()
        assert torch.equal(out.cpu(), ref), (B, per)


# ---- whole trajectories --------------------------------------------------------------------------------------------------------
def _emul_eps(sd, cfg, x, t, c_concat, ctxs, combine):
    """Model outputs of the reference's hybrid model under fp16 autocast (oracle emulation) on the batch [x] * len(ctxs) with the
    contexts in that order, combined by `combine` in fp16, returned in fp32."""
    n = len(ctxs)
    xc = torch.cat([torch.cat([x] * n), torch.cat([c_concat] * n)], dim=1)
    e = unet_ref.unet_forward(sd, cfg, xc, torch.cat([t] * n), torch.cat(ctxs), mode="autocast16")
    return combine(*e.chunk(n)).float()


def _ddim_upd(x, e, tabs, idx):
    f = lambda v: torch.tensor(float(np.float32(v)), dtype=torch.float32)
    a_t, a_prev, s1 = f(tabs["alphas"][idx]), f(tabs["alphas_prev"][idx]), f(tabs["sqrt_one_minus_alphas"][idx])
    p0 = (x - s1 * e) / a_t.sqrt()
    return a_prev.sqrt() * p0 + (1. - a_prev).sqrt() * e


def _cfg2(eu, ec):
    return eu + SCALE * (ec - eu)


def _cfg3(eu, ec, es):
    return eu + SCALE * ((CW * ec + (1 - CW) * es) - eu)


def _check(out, ref, emul, name):
    ref = torch.from_numpy(ref)
    err = out.float().cpu() - ref
    rel = (err.norm() / ref.norm()).item()
    rel_e = ((emul - ref).norm() / ref.norm()).item()
    print(f"[traj {name}] max_abs {err.abs().max().item():.3e} rel_l2 {rel:.3e} | autocast16 emulation rel_l2 {rel_e:.3e} "
          f"| scale {ref.abs().max().item():.2f}")
    assert torch.isfinite(out).all()
    assert rel <= max(2.0 * rel_e, 5e-3), (rel, rel_e)


def _conds(case, B, cfg, *names):
    cc = G.T(case + ".c_concat", (B, 5, H, W))
    return cc, [G.T(f"{case}.{n}", (B, 77, cfg.context_dim)) for n in names]


def _d(cc, ctx):
    return {"c_concat": [cc.to(dev())], "c_crossattn": [ctx.to(dev())]}


@pytest.mark.parametrize("case,scale,n_inter", [("enc_s1", 1.0, None), ("enc_s25", SCALE, 3)])
def test_encode_trajectory(golden, case, scale, n_inter):
    m, cfg = model()
    g = golden("ddim_extras")
    B, t_enc = 1, 10
    x0 = G.T(case + ".x0", (B, 4, H, W))
    cc, (c, uc) = _conds(case, B, cfg, "c_cross", "uc_cross")
    s = _sampler("DDIMSampler", 50, m)
    t_seq = []
    orig_apply = m.apply_model

    def spy(x, t, cond, **kw):
        t_seq.append(t[0].item())
        return orig_apply(x, t, cond, **kw)

    m.apply_model = spy
    try:
        x_enc, info = s.encode(x0.to(dev()), _d(cc, c), t_enc, return_intermediates=n_inter, unconditional_guidance_scale=scale,
                               unconditional_conditioning=_d(cc, uc) if scale != 1.0 else None)
    finally:
        m.apply_model = orig_apply
    assert t_seq == [int(v) for v in g[case + ".t_seq"]], "encode feeds the loop index (ddim.py:407)"
    assert info["intermediate_steps"] == [int(v) for v in g[case + ".intermediate_steps"]]
    assert info["x_encoded"] is x_enc and ("intermediates" in info) == bool(n_inter)
    sd = G.unet_state(G.TRAJ_CONFIG)
    c1, c2 = s.encode_coefficients(t_enc)
    f = lambda v: torch.tensor(float(np.float32(v)))
    x = x0.clone()
    with torch.no_grad():
        for i in range(t_enc):
            t = torch.full((B,), i)
            e = (_emul_eps(sd, cfg, x, t, cc, [c], lambda e_: e_) if scale == 1.0 else
                 _emul_eps(sd, cfg, x, t, cc, [uc, c], _cfg2))
            x = f(c1[i]) * x + f(c2[i]) * e
    _check(x_enc, g[case + ".x_enc"], x, case)


def test_stochastic_encode_then_decode(golden):
    m, cfg = model()
    g = golden("ddim_extras")
    case, B, t_start = "sdec", 1, 10
    x0 = G.T(case + ".x0", (B, 4, H, W)).to(dev())
    noise = G.T(case + ".noise", (B, 4, H, W)).to(dev())
    cc, (c, uc) = _conds(case, B, cfg, "c_cross", "uc_cross")
    s = _sampler("DDIMSampler", 50, m)
    z = s.stochastic_encode(x0, torch.full((B,), t_start, device=dev(), dtype=torch.long), noise=noise)
    _within_ulp(z, g[case + ".z"], "stochastic_encode")
    x_dec = s.decode(z, _d(cc, c), t_start, unconditional_guidance_scale=SCALE, unconditional_conditioning=_d(cc, uc))
    sd = G.unet_state(G.TRAJ_CONFIG)
    tabs = ddim_ref.ddim_tables(50, 0.0)
    x = torch.from_numpy(g[case + ".z"]).clone()
    with torch.no_grad():
        for i, step in enumerate(np.flip(tabs["timesteps"][:t_start])):
            x = _ddim_upd(x, _emul_eps(sd, cfg, x, torch.full((B,), int(step)), cc, [uc, c], _cfg2), tabs, t_start - i - 1)
    _check(x_dec, g[case + ".x_dec"], x, case)


@pytest.mark.parametrize("case,B", [("struct_b1", 1), ("struct_b2", 2)])
def test_structure_trajectory(golden, case, B):
    m, cfg = model()
    g = golden("ddim_extras")
    S = 10
    x_T = G.T(case + ".x_T", (B, 4, H, W))
    cc, (c, cs, uc) = _conds(case, B, cfg, "c_cross", "cs_cross", "uc_cross")
    s = _sampler("StructureDDIMSampler", S, m)
    batches = []
    orig_apply = m.apply_model

    def spy(x, t, cond, **kw):
        batches.append(x.shape[0])
        return orig_apply(x, t, cond, **kw)

    m.apply_model = spy
    try:
        samples, inter = s.sample(S, B, (4, H, W), _d(cc, c), verbose=False, eta=0.0, x_T=x_T.to(dev()),
                                  unconditional_guidance_scale=SCALE, unconditional_conditioning=_d(cc, uc), Tm=TM,
                                  cond_simple=_d(cc, cs), cond_weight=CW, mask_dir="right")
    finally:
        m.apply_model = orig_apply
    assert batches == [int(v) for v in g[case + ".batch_seq"]]
    assert len(inter["x_inter"]) == g[case + ".x_inter"].shape[0]
    sd = G.unet_state(G.TRAJ_CONFIG)
    tabs = ddim_ref.ddim_tables(S, 0.0)
    x = x_T.clone()
    with torch.no_grad():
        for i, step in enumerate(np.flip(tabs["timesteps"])):
            idx = S - i - 1
            t = torch.full((B,), int(step))
            e = (_emul_eps(sd, cfg, x, t, cc, [uc, c, cs], _cfg3) if idx >= TM else _emul_eps(sd, cfg, x, t, cc, [uc, cs], _cfg2))
            x = _ddim_upd(x, e, tabs, idx)
    _check(samples, g[case + ".samples"], x, case)


def test_replays_the_ddim_graph_and_is_deterministic():
    """encode and decode replay the step DDIM captured; the three-way phase adds exactly one capture (batch 3B, no shared prefix)
    and its two-way phase replays DDIM's; every run is bit-reproducible."""
    m, cfg = model()
    unet = m.model.diffusion_model
    B = 2
    x_T = G.T("dxdet.x_T", (B, 4, H, W)).to(dev())
    x0 = G.T("dxdet.x0", (B, 4, H, W)).to(dev())
    noise = G.T("dxdet.n", (B, 4, H, W)).to(dev())
    cc = G.T("dxdet.cc", (B, 5, H, W))
    cond = _d(cc, G.T("dxdet.c", (B, 77, cfg.context_dim)))
    cs = _d(cc, G.T("dxdet.cs", (B, 77, cfg.context_dim)))
    uc = {"c_concat": cond["c_concat"], "c_crossattn": [G.T("dxdet.uc", (B, 77, cfg.context_dim)).to(dev())]}
    unet._graphs.clear()
    m.sample_log(cond=cond, batch_size=B, ddim=True, ddim_steps=5, eta=0.0, x_T=x_T, unconditional_guidance_scale=SCALE,
                 unconditional_conditioning=uc)
    keys = set(unet._graphs)
    assert len(keys) == 1
    s = _sampler("DDIMSampler", 50, m)
    enc = [s.encode(x0, cond, 6, unconditional_guidance_scale=SCALE, unconditional_conditioning=uc)[0] for _ in range(2)]
    assert torch.equal(enc[0], enc[1])
    assert set(unet._graphs) == keys, "an encode step must replay the graph DDIM captured"
    z = [s.stochastic_encode(x0, torch.full((B,), 6, device=dev(), dtype=torch.long), noise=noise) for _ in range(2)]
    assert torch.equal(z[0], z[1])
    dec = [s.decode(z[0], cond, 6, unconditional_guidance_scale=SCALE, unconditional_conditioning=uc) for _ in range(2)]
    assert torch.equal(dec[0], dec[1]) and set(unet._graphs) == keys
    st = _sampler("StructureDDIMSampler", 6, m)
    kw = dict(verbose=False, eta=0.0, x_T=x_T, unconditional_guidance_scale=SCALE, unconditional_conditioning=uc, Tm=3,
              cond_simple=cs, cond_weight=CW)
    outs = [st.sample(6, B, (4, H, W), cond, **kw)[0] for _ in range(2)]
    assert torch.equal(outs[0], outs[1])
    new = set(unet._graphs) - keys
    assert keys <= set(unet._graphs) and len(new) == 1, (keys, set(unet._graphs))
    (k,) = new
    assert k[0][0] == 3 * B and k[4] is False
    assert unet._t_host is None and st._cfg3_cache is None and st._cfg_cache is None
