"""GPU parity of the ancestral DDPM sampler (tests/golden/ddpm_ancestral.npz, made by tools/make_golden_ddpm.py from the real
reference on the CPU): the ABI 30 posterior-step kernel against single reference p_sample steps and against the same formula in
torch, whole chains through the drop-in LatentDiffusion (TRAJ_CONFIG UNet, 8x16 latents) against the reference's within the drift
of a CPU fp16-autocast emulation, the loops' bookkeeping, the known-region blend, graph reuse and determinism, and
RefInpaintLDM.log_images(sampler="ddpm") end to end."""
import os
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from oracle import golden_spec as G, unet_ref, weights  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
B_STEP, B_TRAJ, H, W = 2, 2, 8, 16
STEP_T = (0, 1, 500, 999)
PROG_START_T = 30
PROG_TEMPERATURE = [1.0 - 0.01 * i for i in range(PROG_START_T)]


def dev():
    return torch.device("cuda:0")


def _install():
    import leftrefill_amd.dropin as dropin
    dropin.install()


_cache = {}


def model(timesteps=1000):
    if timesteps not in _cache:
        _install()
        from inpainting_ldm.ref_inpainting_ldm import RefInpaintLDM
        cfg = G.CONFIGS[G.TRAJ_CONFIG]
        m = RefInpaintLDM(first_stage_config={"target": "torch.nn.Identity"}, cond_stage_config={"target": "torch.nn.Identity"},
                          unet_config={"target": "ldm.modules.diffusionmodules.openaimodel.UNetModel", "params": cfg.kwargs()},
                          conditioning_key="hybrid", scale_factor=0.18215, linear_start=0.00085, linear_end=0.0120,
                          timesteps=timesteps, channels=4, log_every_t=10, data_config={"img_size": 256})
        m.model.diffusion_model.load_state_dict(G.unet_state(G.TRAJ_CONFIG), strict=True)
        _cache[timesteps] = (m.to(dev()).eval(), cfg)
    return _cache[timesteps]


def _within_ulp(out, ref, name, n=1):
    out = out.float().cpu().contiguous().numpy()
    ref = np.ascontiguousarray(ref, dtype=np.float32)
    d = np.abs(out.view(np.int32).astype(np.int64) - ref.view(np.int32).astype(np.int64))
    print(f"[{name}] max ulp {d.max()}")
    assert d.max() <= n, (name, d.max())


# ---- the step on the CPU, op by op in fp32 as the reference evaluates it ----------------------------------------------------------
class _Tab:
    """The reference's fp32 tables (golden) as 0-dim fp32 tensors per timestep."""

    def __init__(self, g, T_=1000):
        self.t = {k: torch.from_numpy(g[f"tab_T{T_}.{k}"]) for k in ("posterior_log_variance_clipped", "posterior_mean_coef1",
                                                                     "posterior_mean_coef2", "sqrt_recip_alphas_cumprod",
                                                                     "sqrt_recipm1_alphas_cumprod")}

    def coefs(self, t):
        """(sqrt_recip, sqrt_recipm1, coef1, coef2, sigma) host floats for ops.ddpm_step"""
        v = self.t
        std = (0.5 * v["posterior_log_variance_clipped"][t]).exp()
        return (v["sqrt_recip_alphas_cumprod"][t].item(), v["sqrt_recipm1_alphas_cumprod"][t].item(),
                v["posterior_mean_coef1"][t].item(), v["posterior_mean_coef2"][t].item(), 0.0 if t == 0 else std.item())


def _step_cpu(x, e, noise, coefs, clip):
    """x, noise fp32, e any float dtype (widened to fp32 as type promotion does in the reference) -> (x_prev, x_recon)"""
    recip, recipm1, c1, c2, sigma = [torch.tensor(v, dtype=torch.float32) for v in coefs]
    xr = recip * x - recipm1 * e.float()
    if clip:
        xr = xr.clamp(-1., 1.)
    mean = c1 * xr + c2 * x
    return (mean if float(sigma) == 0.0 else mean + sigma * noise), xr


# ---- the kernel against single reference steps --------------------------------------------------------------------------------
@pytest.mark.parametrize("clip", [False, True], ids=["noclip", "clip"])
@pytest.mark.parametrize("t", STEP_T)
@pytest.mark.parametrize("dt", [torch.float16, torch.float32], ids=["f16", "f32"])
def test_step_kernel_against_reference_steps(golden, dt, t, clip):
    from leftrefill_amd import ops
    g = golden("ddpm_ancestral")
    tab = _Tab(g)
    x = G.T("ddpm_step.x", (B_STEP, 4, H, W))
    e = G.T("ddpm_step.e", (B_STEP, 4, H, W)).to(dt)
    nz = G.T("ddpm_step.noise.0", (B_STEP, 4, H, W))
    x_prev, x0 = ops.ddpm_step(x.to(dev()), e.to(dev()), nz.to(dev()), *tab.coefs(t), clip_denoised=clip, return_x0=True)
    tag = "f16" if dt == torch.float16 else "f32"
    _within_ulp(x0, g[f"step.t{t}.clip{int(clip)}.{tag}.x0"], f"x0 t={t} clip={clip} {tag}")
    _within_ulp(x_prev, g[f"step.t{t}.clip{int(clip)}.{tag}.x_prev"], f"x_prev t={t} clip={clip} {tag}")
    rp, rx0 = _step_cpu(x, e, nz, tab.coefs(t), clip)
    _within_ulp(x0, rx0.numpy(), f"x0 vs torch t={t} clip={clip} {tag}")
    _within_ulp(x_prev, rp.numpy(), f"x_prev vs torch t={t} clip={clip} {tag}")
    if clip:
        assert x0.abs().max().item() <= 1.0
        if t == 999:
            assert (rx0.abs() == 1.0).any(), "the clamp must bite in this case"
    if t == 0:      # no noise at t == 0: exactly the posterior mean
        mean, _ = _step_cpu(x, e, None, tab.coefs(0), clip)
        assert torch.equal(x_prev.cpu(), mean)
    only_prev, none = ops.ddpm_step(x.to(dev()), e.to(dev()), nz.to(dev()), *tab.coefs(t), clip_denoised=clip)
    assert none is None and torch.equal(only_prev, x_prev)


def test_twins_and_vector_scalar_paths(golden):
    """fp32, fp16 and bf16 eps on the 16-byte path (numel % 4 == 0, aligned), on the scalar one by an odd numel and by a misaligned
    view: the same bits on every path, within 1 ulp of torch with eps rounded the same way; on fp32 eps the two twins agree."""
    from leftrefill_amd import ops
    tab = _Tab(golden("ddpm_ancestral"))
    co = tab.coefs(500)
    for clip in (False, True):
        for dt in (torch.float32, torch.float16, torch.bfloat16):
            n = 4 * 128
            x, nz, e = G.T("dtw.x", (n,)), G.T("dtw.n", (n,)), G.T("dtw.e", (n,)).to(dt)
            rp, rx0 = _step_cpu(x, e, nz, co, clip)
            xp, x0 = ops.ddpm_step(x.to(dev()), e.to(dev()), nz.to(dev()), *co, clip_denoised=clip, return_x0=True)
            _within_ulp(xp, rp.numpy(), f"x_prev {dt} clip={clip}")
            _within_ulp(x0, rx0.numpy(), f"x0 {dt} clip={clip}")
            # misaligned views of the same data: the launcher must fall back to one element per thread, same bits
            pad = lambda v: torch.cat([v[:1], v]).to(dev())[1:]
            xm, nm, em = pad(x), pad(nz), pad(e)
            assert xm.data_ptr() % 16 != 0 and xm.is_contiguous()
            xp_s, x0_s = ops.ddpm_step(xm, em, nm, *co, clip_denoised=clip, return_x0=True)
            assert torch.equal(xp_s, xp) and torch.equal(x0_s, x0)
            # odd numel: scalar path; its first elements see the same data
            n2 = 4 * 127 + 3
            xp_o, x0_o = ops.ddpm_step(x[:n2].to(dev()), e[:n2].to(dev()), nz[:n2].to(dev()), *co, clip_denoised=clip, return_x0=True)
            assert torch.equal(xp_o, xp[:n2]) and torch.equal(x0_o, x0[:n2])
            if dt == torch.float32:
                pick = ops._eps16
                ops._eps16 = lambda eps: torch.bfloat16
                try:
                    xp_b, x0_b = ops.ddpm_step(x.to(dev()), e.to(dev()), nz.to(dev()), *co, clip_denoised=clip, return_x0=True)
                finally:
                    ops._eps16 = pick
                assert torch.equal(xp_b, xp) and torch.equal(x0_b, x0)


def test_known_region_blend_in_the_step(golden):
    """The blend folded into the step equals the reference's expression on the step's own output, for a [B,1,H,W] mask and for the
    same mask at full size, on both paths."""
    from leftrefill_amd import ops
    tab = _Tab(golden("ddpm_ancestral"))
    co = tab.coefs(500)
    sa, s1ma = 0.6171875, 0.78515625
    for shape in ((2, 4, H, W), (2, 3, 5, 7)):
        x, nz, e = G.T("dbl.x", shape), G.T("dbl.n", shape), G.T("dbl.e", shape).half()
        x0, qn = G.T("dbl.x0", shape), G.T("dbl.qn", shape)
        mask = (G.T("dbl.m", (shape[0], 1) + shape[2:]) > 0).float()
        mask[0, 0, 0, 0] = 0.25      # a soft entry: (1 - m) is not 0 or 1
        rp, _ = _step_cpu(x, e, nz, co, True)
        ref = (torch.tensor(sa) * x0 + torch.tensor(s1ma) * qn) * mask + (1. - mask) * rp
        d = lambda v: v.to(dev())
        for mk in (mask, mask.expand(shape).contiguous()):
            out, _ = ops.ddpm_step(d(x), d(e), d(nz), *co, clip_denoised=True, known=(d(x0), d(qn), d(mk), sa, s1ma))
            _within_ulp(out, ref.numpy(), f"blend {shape} mask {tuple(mk.shape)}")


@pytest.mark.parametrize("dt", [torch.float16, torch.float32], ids=["f16", "f32"])
def test_p_sample_with_a_timestep_per_sample(golden, dt):
    """A direct p_sample call whose samples sit at different timesteps, temperature != 1, fixed model output."""
    m, _ = model()
    g = golden("ddpm_ancestral")
    ts = [int(v) for v in g["mixed.t"]]
    shape = (len(ts), 4, H, W)
    x, e = G.T("ddpm_mixed.x", shape).to(dev()), G.T("ddpm_mixed.e", shape).to(dev()).to(dt)
    import ldm.models.diffusion.ddpm as ddpm_mod
    orig_noise, orig_apply = ddpm_mod.noise_like, m.apply_model
    ddpm_mod.noise_like = lambda shape_, device, repeat=False: G.T("ddpm_mixed.noise.0", tuple(shape_)).to(device)
    m.apply_model = lambda x_, t_, c_, **kw: e
    try:
        x_prev, x0 = m.p_sample(x, None, torch.tensor(ts, device=dev()), clip_denoised=True, return_x0=True,
                                temperature=float(g["mixed.temperature"]))
        alone = m.p_sample(x, None, torch.tensor(ts, device=dev()), clip_denoised=True, temperature=float(g["mixed.temperature"]))
    finally:
        ddpm_mod.noise_like, m.apply_model = orig_noise, orig_apply
    tag = "f16" if dt == torch.float16 else "f32"
    _within_ulp(x0, g[f"mixed.{tag}.x0"], "mixed x0 " + tag)
    _within_ulp(x_prev, g[f"mixed.{tag}.x_prev"], "mixed x_prev " + tag)
    assert torch.is_tensor(alone) and torch.equal(alone, x_prev)


# ---- whole chains ------------------------------------------------------------------------------------------------------------------
def _check(out, ref, emul, name):
    ref = torch.from_numpy(ref)
    err = out.float().cpu() - ref
    rel = (err.norm() / ref.norm()).item()
    rel_e = ((emul - ref).norm() / ref.norm()).item()
    print(f"[traj {name}] max_abs {err.abs().max().item():.3e} rel_l2 {rel:.3e} | autocast16 emulation rel_l2 {rel_e:.3e} "
          f"| scale {ref.abs().max().item():.2f}")
    assert torch.isfinite(out).all()
    assert rel <= max(2.0 * rel_e, 5e-3), (rel, rel_e)


class _Injected:
    """While active: the k-th noise_like call of the drop-in's ddpm module returns T('<case>.noise.<k>'), the k-th torch.randn_like
    T('<case>.qnoise.<k>'); the model's apply_model records the timestep it is given."""

    def __init__(self, m, case):
        self.m, self.case, self.n, self.q, self.t_seq = m, case, 0, 0, []

    def __enter__(self):
        import ldm.models.diffusion.ddpm as ddpm_mod
        self.mod = ddpm_mod
        self._nl, self._rl, self._am = ddpm_mod.noise_like, torch.randn_like, self.m.apply_model

        def noise_like(shape, device, repeat=False):
            self.n += 1
            return G.T(f"{self.case}.noise.{self.n - 1}", tuple(shape)).to(device)

        def randn_like(x, **kw):
            self.q += 1
            return G.T(f"{self.case}.qnoise.{self.q - 1}", tuple(x.shape)).to(x.device)

        def apply_model(x, t, c, **kw):
            assert x.shape[0] == t.shape[0]
            self.t_seq.append(t)
            return self._am(x, t, c, **kw)

        ddpm_mod.noise_like, torch.randn_like, self.m.apply_model = noise_like, randn_like, apply_model
        return self

    def __exit__(self, *exc):
        self.mod.noise_like, torch.randn_like, self.m.apply_model = self._nl, self._rl, self._am

    def timesteps(self):
        assert all(bool((t == t[0]).all()) for t in self.t_seq)
        return [int(t[0].item()) for t in self.t_seq]


def _emulate(m, cfg, case, x_T, cc, ctx, n_steps, clip, temperature=None, known=None):
    """The same chain on the CPU: the oracle's fp16-autocast emulation of the UNet, the step in fp32 torch with the model's own
    tables.  Yields (i, img, x0_partial)."""
    sd = G.unet_state(G.TRAJ_CONFIG)
    tb = {k: getattr(m, k).detach().float().cpu() for k in ("sqrt_recip_alphas_cumprod", "sqrt_recipm1_alphas_cumprod",
                                                            "posterior_mean_coef1", "posterior_mean_coef2",
                                                            "posterior_log_variance_clipped", "sqrt_alphas_cumprod",
                                                            "sqrt_one_minus_alphas_cumprod")}
    x = x_T.clone()
    B = x.shape[0]
    with torch.no_grad():
        for k, i in enumerate(reversed(range(n_steps))):
            e = unet_ref.unet_forward(sd, cfg, torch.cat([x, cc], dim=1), torch.full((B,), i), ctx, mode="autocast16").float()
            nz = G.T(f"{case}.noise.{k}", tuple(x.shape))
            if temperature is not None:
                nz = nz * temperature[i]
            std = (0.5 * tb["posterior_log_variance_clipped"][i]).exp()
            co = (tb["sqrt_recip_alphas_cumprod"][i].item(), tb["sqrt_recipm1_alphas_cumprod"][i].item(),
                  tb["posterior_mean_coef1"][i].item(), tb["posterior_mean_coef2"][i].item(), 0.0 if i == 0 else std.item())
            x, xr = _step_cpu(x, e, nz, co, clip)
            if known is not None:
                x0, mask = known
                q = tb["sqrt_alphas_cumprod"][i] * x0 + tb["sqrt_one_minus_alphas_cumprod"][i] * G.T(f"{case}.qnoise.{k}", tuple(x.shape))
                x = q * mask + (1. - mask) * x
            yield i, x, xr


def _traj_inputs(case, cfg):
    B = B_TRAJ
    cc, ctx = G.T(case + ".c_concat", (B, 5, H, W)), G.T(case + ".c_cross", (B, 77, cfg.context_dim))
    return G.T(case + ".x_T", (B, 4, H, W)), cc, ctx, {"c_concat": [cc.to(dev())], "c_crossattn": [ctx.to(dev())]}


def _mask():
    mask = torch.zeros(B_TRAJ, 1, H, W)
    mask[..., : W // 2] = 1.
    return mask


def _run_case(case, m, cfg, full_mask=False):
    """-> (img, intermediates, callback args, img_callback args, timesteps seen, noise draws, logged emulation, emulated final)"""
    B = B_TRAJ
    shape = (B, 4, H, W)
    x_T, cc, ctx, cond = _traj_inputs(case, cfg)
    cb, icb = [], []
    icb_f = lambda im, i: icb.append(i)
    known = None
    with _Injected(m, case) as inj:
        if case == "ddpm_full50":
            n, log, pick = 50, 10, 1
            img, inter = m.sample(cond, batch_size=B, return_intermediates=True, x_T=x_T.to(dev()), verbose=False, shape=shape)
        elif case == "ddpm_t40":
            n, log, pick = 40, 10, 1
            img, inter = m.p_sample_loop(cond, shape, return_intermediates=True, x_T=x_T.to(dev()), verbose=False,
                                         callback=cb.append, img_callback=icb_f, timesteps=40)
        elif case == "ddpm_start25":
            n, log, pick = 25, 7, 1
            img, inter = m.p_sample_loop(cond, shape, return_intermediates=True, x_T=x_T.to(dev()), verbose=False,
                                         callback=cb.append, img_callback=icb_f, start_T=25, log_every_t=7)
        elif case == "ddpm_prog30":
            n, log, pick = PROG_START_T, 10, 2
            img, inter = m.progressive_denoising(cond, (4, H, W), verbose=False, callback=cb.append, img_callback=icb_f,
                                                 temperature=PROG_TEMPERATURE, batch_size=B, x_T=x_T.to(dev()),
                                                 start_T=PROG_START_T, log_every_t=10)
        else:
            assert case == "ddpm_masked50"
            n, log, pick = 50, 10, 1
            known = (G.T(case + ".x0", shape), _mask())
            mk = known[1].expand(shape).contiguous() if full_mask else known[1]
            img, inter = m.sample(cond, batch_size=B, return_intermediates=True, x_T=x_T.to(dev()), verbose=False,
                                  mask=mk.to(dev()), x0=known[0].to(dev()), shape=shape)
        t_seq = inj.timesteps()
    emul_inter = [] if case == "ddpm_prog30" else [x_T]
    last = None
    for i, *vals in _emulate(m, cfg, case, x_T, cc, ctx, n, True, PROG_TEMPERATURE if case == "ddpm_prog30" else None, known):
        last = vals[0]
        if i % log == 0 or i == n - 1:
            emul_inter.append(vals[pick - 1])
    return img, inter, cb, icb, t_seq, (inj.n, inj.q), emul_inter, last


@pytest.mark.parametrize("case,T_", [("ddpm_full50", 50), ("ddpm_t40", 1000), ("ddpm_start25", 1000), ("ddpm_prog30", 1000),
                                     ("ddpm_masked50", 50)])
def test_trajectory(golden, case, T_):
    m, cfg = model(T_)
    g = golden("ddpm_ancestral")
    img, inter, cb, icb, t_seq, draws, emul_inter, emul = _run_case(case, m, cfg)
    assert t_seq == [int(v) for v in g[case + ".t_seq"]]
    assert cb == [int(v) for v in g[case + ".cb_seq"]] and icb == [int(v) for v in g[case + ".img_cb_seq"]]
    assert list(draws) == [int(v) for v in g[case + ".n_noise"]], "noise_like every step, q_sample's randn_like only with a mask"
    ref_inter = g[case + ".intermediates"]
    assert len(inter) == ref_inter.shape[0] == len(emul_inter)
    assert m.model.diffusion_model._t_host is None
    if case != "ddpm_prog30":
        assert torch.equal(inter[0].cpu(), G.T(case + ".x_T", (B_TRAJ, 4, H, W))) and inter[-1] is img
    for k, (o, e) in enumerate(zip(inter, emul_inter)):
        _check(o, ref_inter[k], e, f"{case} intermediate {k}")
    _check(img, g[case + ".samples"], emul, case)
    if case == "ddpm_masked50":
        # the last step (t = 0) inside the known region: q_sample(x0, 0) with the LAST injected q-noise
        x0 = G.T(case + ".x0", (B_TRAJ, 4, H, W))
        q = m.sqrt_alphas_cumprod[0].cpu() * x0 + m.sqrt_one_minus_alphas_cumprod[0].cpu() * G.T(f"{case}.qnoise.49", tuple(x0.shape))
        half = W // 2
        _within_ulp(img[..., :half], q[..., :half].contiguous().numpy(), "known region of the last step")
        ref = torch.from_numpy(g[case + ".samples"])
        _within_ulp(img[..., :half], ref[..., :half].contiguous().numpy(), "known region against the reference")
        full = _run_case(case, m, cfg, full_mask=True)[0]
        assert torch.equal(full, img), "a full-size mask and its [B,1,H,W] form give the same bits"


def test_deterministic_and_device_noise():
    m, cfg = model()
    case = "ddpm_t40"
    x_T, _, _, cond = _traj_inputs(case, cfg)
    shape = tuple(x_T.shape)
    outs = []
    for _ in range(2):
        with _Injected(m, case):
            outs.append(m.p_sample_loop(cond, shape, x_T=x_T.to(dev()), verbose=False, timesteps=12))
    assert torch.is_tensor(outs[0]) and torch.equal(outs[0], outs[1])
    drawn = []
    for _ in range(2):
        torch.manual_seed(77)
        drawn.append(m.sample(cond, batch_size=B_TRAJ, verbose=False, timesteps=12, shape=shape))
    assert drawn[0].is_cuda and torch.equal(drawn[0], drawn[1]) and not torch.equal(drawn[0], outs[0])
    torch.manual_seed(78)
    assert not torch.equal(m.sample(cond, batch_size=B_TRAJ, verbose=False, timesteps=12, shape=shape), drawn[0])


def test_replays_one_captured_step_shared_with_ddim():
    m, cfg = model()
    unet = m.model.diffusion_model
    case = "ddpm_t40"
    x_T, _, _, cond = _traj_inputs(case, cfg)
    shape = tuple(x_T.shape)
    unet._graphs.clear()
    m.p_sample_loop(cond, shape, x_T=x_T.to(dev()), verbose=False, timesteps=8)
    keys = set(unet._graphs)
    assert len(keys) == 1
    (k,) = keys
    assert k[0][0] == B_TRAJ
    m.progressive_denoising(cond, shape[1:], verbose=False, batch_size=B_TRAJ, x_T=x_T.to(dev()), start_T=8)
    assert set(unet._graphs) == keys, "a second chain replays the captured step"
    from ldm.models.diffusion.ddim import DDIMSampler
    DDIMSampler(m).sample(5, B_TRAJ, shape[1:], cond, verbose=False, eta=0.0, x_T=x_T.to(dev()))
    assert set(unet._graphs) == keys, "a scale-1 DDIM run of the same batch and conditioning replays the same entry"
    assert unet._t_host is None


# ---- the task model end to end ---------------------------------------------------------------------------------------------------
def _write_config(path, size):
    import yaml
    cfg = G.CONFIGS["MID"]
    dd = dict(double_z=True, z_channels=4, resolution=size, in_channels=3, out_ch=3, ch=64, ch_mult=[1, 2, 4, 4],
              num_res_blocks=1, attn_resolutions=[], dropout=0.0)
    model_ = {"target": "inpainting_ldm.ref_inpainting_ldm.RefInpaintLDM", "params": dict(
        linear_start=0.00085, linear_end=0.0120, timesteps=1000, first_stage_key="image", cond_stage_key="txt", channels=4,
        cond_stage_trainable=True, conditioning_key="hybrid", scale_factor=0.18215,
        data_config={"img_size": size, "repeat_sp_token": 4, "sp_token": "<special-token>"},
        unet_config={"target": "ldm.modules.diffusionmodules.openaimodel.UNetModel", "params": cfg.kwargs()},
        first_stage_config={"target": "ldm.models.autoencoder.AutoencoderKL",
                            "params": {"ddconfig": dd, "embed_dim": 4, "lossconfig": {"target": "torch.nn.Identity"}}},
        cond_stage_config={"target": "ldm.modules.encoders.Refill_modules.PromptCLIPEmbedder",
                           "params": dict(freeze=True, layer="penultimate", special_tokens=["repeat_4_<special-token>"],
                                          init_text=["reference on the left target on the right"])})}
    with open(path, "w") as f:
        yaml.safe_dump({"model": model_}, f)


def test_log_images_with_the_ddpm_sampler(tmp_path):
    size, N = 64, 2
    _write_config(str(tmp_path / "model_config.yaml"), size)
    stub = tmp_path / "stubs"
    stub.mkdir()
    (stub / "open_clip.py").write_text("from oracle.clip_stub import *  # noqa: F401,F403  (test stand-in for the absent package)\n")
    _install()
    sys.path.insert(0, str(stub))
    try:
        from inpainting_ldm.model import create_model
        m = create_model(str(tmp_path / "model_config.yaml"))
    finally:
        sys.path.remove(str(stub))
    sd = dict(m.state_dict())
    for k, v in m.state_dict().items():
        if k.startswith("first_stage_model."):
            sd[k] = torch.from_numpy(weights.fill_like("vae2." + k[len("first_stage_model."):], v.shape)).to(v.dtype)
    for k, v in G.unet_state("MID").items():
        sd["model.diffusion_model." + k] = v
    m.load_state_dict(sd, strict=True)
    m = m.to(dev()).eval()
    g_ = torch.Generator().manual_seed(3)
    img = torch.rand(N, size, 2 * size, 3, generator=g_) * 2 - 1
    mask = torch.zeros(N, size, 2 * size, 1)
    mask[:, 16:48, size + 16:size + 48] = 1.
    txt = " ".join(f"<special-token{i}>" for i in range(4))
    batch = {"image": img.to(dev()), "mask": mask.to(dev()), "masked_image": (img * (mask < 0.5)).to(dev()), "txt": [txt] * N}
    with torch.no_grad(), torch.autocast("cuda"):
        torch.manual_seed(11)
        log = m.log_images(batch, N, sampler="ddpm", unconditional_guidance_scale=1.0)
        torch.manual_seed(11)
        z, c = m.get_input(batch, m.first_stage_key, bs=N)
        cond = {"c_concat": [c["c_concat"][0][:N]], "c_crossattn": [c["c_crossattn"][0][:N]]}
        samples = m.sample(cond, batch_size=N, verbose=False, shape=(N, m.channels) + tuple(cond["c_concat"][0].shape[2:]))
        pred = m.decode_first_stage(samples)
        with pytest.raises(ValueError, match="ddim.*plms.*dpm_solver"):
            m.log_images(batch, N, sampler="ddpm", unconditional_guidance_scale=2.5)
    assert log["pred"].shape == (N, 3, size, 2 * size) and torch.isfinite(log["pred"]).all()
    assert torch.equal(log["pred"], pred)
