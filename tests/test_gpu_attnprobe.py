"""GPU: the attention-map probe -- lr_attention_probe_f16 / _bf16 against leftrefill_amd.attnprobe.probe_reference (float64 on the same
16-bit operands), its launch properties, and the wiring: AttentionProbe around the UNet, DDIMSampler(return_attn=True), log_images,
the logger's panels and refill(return_attn=True).

Tolerances are the project's attention tolerances (tests/test_gpu_ops.py test_attention: rtol 2e-3, atol 2e-3 for unit-scale V;
tests/test_gpu_bf16.py test_attention_bf16: rtol 1.6e-2, atol 1.6e-2), the absolute part scaled by the column's largest value:
|out - ref| <= A max|col_c| + R |ref|."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from oracle import golden_spec as G  # noqa: E402
from leftrefill_amd import attnprobe as AP  # noqa: E402
from tests.test_gpu_refill import STEPS, synthetic  # noqa: E402, F401  (`synthetic` is that module's fixture)

TOL = {torch.float16: (2e-3, 2e-3), torch.bfloat16: (1.6e-2, 1.6e-2)}      # dtype -> (A, R)
SCALE = 64 ** -0.5


def dev():
    assert torch.cuda.is_available(), "GPU tests need a MI355X"
    return torch.device("cuda:0")


def check(name, out, ref, cols, dtype):
    """|out - ref| <= A max|col_c| + R |ref| per element; prints the measured maxima first."""
    A, R = TOL[dtype]
    out, ref = out.double().cpu(), ref.double().cpu()
    cmax = cols.double().abs().amax(dim=0).cpu()
    err = (out - ref).abs()
    tol = A * cmax + R * ref.abs()
    print(f"[{name}] max_abs_err {err.max().item():.3e} max err/tol {(err / tol.clamp_min(1e-30)).max().item():.3f} "
          f"max|col| {cmax.max().item():.3g} viol {(err > tol).sum().item()}/{err.numel()}")
    assert torch.isfinite(out).all(), name
    assert (err <= tol).all(), f"{name}: {(err > tol).sum().item()} elements outside A={A} R={R}; max err {err.max().item():.3e}"


def operands(B, heads, Nq, Nkv, ncols, dtype, seed, ldc=None):
    """q, k (column slices of a fused q|k|v projection when Nq == Nkv) and random probe columns on the device."""
    from leftrefill_amd import ops  # noqa: F401
    g = torch.Generator().manual_seed(seed)
    C = heads * 64
    if Nq == Nkv:
        qkv = torch.randn(B * Nq, 3 * C, generator=g).to(dtype).to(dev())
        q, k = qkv[:, :C], qkv[:, C:2 * C]
    else:
        q = torch.randn(B * Nq, C, generator=g).to(dtype).to(dev())
        k = torch.randn(B * Nkv, C, generator=g).to(dtype).to(dev())
    cols = torch.randn(Nkv, ldc or ncols, generator=g).to(dtype).to(dev())[:, :ncols]
    return q, k, cols


# (B, heads, Nq, Nkv, ncols): the deepest level; one partial tile; two key tiles on fused strided slices; query and key tails with
# Nq != Nkv, all eight columns and ldc > ncols; several query blocks and many heads
SHAPES = [(2, 1, 2, 2, 1), (1, 5, 32, 32, 3), (2, 5, 128, 128, 3), (1, 2, 200, 333, 8), (1, 10, 512, 512, 3)]


@pytest.mark.parametrize("dtype", [torch.float16, torch.bfloat16], ids=["f16", "bf16"])
@pytest.mark.parametrize("B,heads,Nq,Nkv,ncols", SHAPES)
def test_probe_kernel_matches_the_reference(B, heads, Nq, Nkv, ncols, dtype):
    from leftrefill_amd import ops
    q, k, cols = operands(B, heads, Nq, Nkv, ncols, dtype, seed=Nq + ncols, ldc=12 if ncols == 8 else None)
    assert (cols.stride(0) > ncols) == (ncols == 8)
    out = ops.attention_probe(q, k, cols, B, heads, Nq, Nkv, SCALE)
    assert out.shape == (B, Nq, ncols) and out.dtype == torch.float32
    check(f"probe B{B} h{heads} {Nq}x{Nkv} c{ncols} {dtype}", out, AP.probe_reference(q, k, cols, B, heads, Nq, Nkv, SCALE), cols, dtype)


@pytest.mark.parametrize("dtype", [torch.float16, torch.bfloat16], ids=["f16", "bf16"])
def test_probe_kernel_running_max_jumps(dtype):
    """As test_attention_online_softmax_rescale: a key of the last tile and one of tile 1 match single queries strongly."""
    from leftrefill_amd import ops
    N = 512
    q, k, cols = operands(1, 1, N, N, 3, dtype, seed=11)
    q, k = q.contiguous(), k.contiguous()
    k[450] = (q[7].float() * 6.0).to(dtype)
    k[70] = (q[300].float() * 4.0).to(dtype)
    out = ops.attention_probe(q, k, cols, 1, 1, N, N, SCALE)
    ref = AP.probe_reference(q, k, cols, 1, 1, N, N, SCALE)
    check(f"probe spike {dtype}", out, ref, cols, dtype)
    assert (ref[0, 7].cpu() - cols[450].double().cpu()).abs().max() < 1e-6      # the spike owns query 7's row


def test_probe_kernel_properties():
    from leftrefill_amd import ops
    dtype = torch.float16
    B, heads, N = 2, 5, 128
    q, k, _ = operands(B, heads, N, N, 3, dtype, seed=21)
    A, R = TOL[dtype]
    # an all-ones column: every row of the softmax sums to 1
    ones = torch.ones(N, 1, device=dev(), dtype=dtype)
    o1 = ops.attention_probe(q, k, ones, B, heads, N, N, SCALE)
    print(f"[probe ones] max|out - 1| {(o1 - 1).abs().max().item():.3e}")
    assert ((o1 - 1).abs() <= A + R).all()
    # the canvas columns of an 8 x 16 canvas: mass in [0, 1], coordinates inside the reference half (x <= 7, y <= 7)
    cc = AP.canvas_columns(8, 16, dtype, dev())
    raw = ops.attention_probe(q, k, cc, B, heads, N, N, SCALE).double()
    t0, t1 = A + R * raw[..., 0].abs(), 7 * A + R * raw[..., 1].abs()
    print(f"[probe canvas] mass {raw[..., 0].min().item():.4f} .. {raw[..., 0].max().item():.4f}  x {(raw[..., 1] / raw[..., 0]).min().item():.3f} .. "
          f"{(raw[..., 1] / raw[..., 0]).max().item():.3f}  y {(raw[..., 2] / raw[..., 0]).min().item():.3f} .. {(raw[..., 2] / raw[..., 0]).max().item():.3f}")
    assert (raw[..., 0] >= -t0).all() and (raw[..., 0] <= 1 + t0).all()
    for c in (1, 2):
        assert (raw[..., c] >= -t1).all() and (raw[..., c] <= 7 * raw[..., 0] + t1 + 7 * t0).all()
    check("probe canvas 8x16", raw, AP.probe_reference(q, k, cc, B, heads, N, N, SCALE), cc, dtype)
    # beta = 0 never reads out
    cols = torch.randn(N, 3, generator=torch.Generator().manual_seed(22)).to(dtype).to(dev())
    nan = torch.full((B, N, 3), float("nan"), device=dev())
    one = ops.attention_probe(q, k, cols, B, heads, N, N, SCALE, out=nan, alpha=1.0, beta=0.0)
    assert one is nan and torch.isfinite(one).all()
    # two identical launches agree bit for bit; alpha / beta accumulate exactly
    again = ops.attention_probe(q, k, cols, B, heads, N, N, SCALE)
    assert torch.equal(one, again)
    acc = torch.zeros(B, N, 3, device=dev())
    for _ in range(2):
        ops.attention_probe(q, k, cols, B, heads, N, N, SCALE, out=acc, alpha=0.5, beta=1.0)
    assert torch.equal(acc, one)


def test_probe_kernel_refuses_bad_arguments():
    from leftrefill_amd import _lib
    lib = _lib.load()
    B, heads, N = 1, 1, 32
    buf = torch.zeros(N + 1, 80, device=dev(), dtype=torch.float16)
    cols = torch.ones(N, 8, device=dev(), dtype=torch.float16)
    out = torch.zeros(B, N, 8, device=dev())
    s = torch.cuda.current_stream().cuda_stream

    def call(q=buf.data_ptr(), ldq=80, k=buf.data_ptr(), ldk=80, c=cols.data_ptr(), ldc=8, ncols=3, o=out.data_ptr(), Nq=N, Nkv=N):
        return lib.lr_attention_probe_f16(q, ldq, k, ldk, c, ldc, ncols, o, B, heads, Nq, Nkv, SCALE, 1.0, 0.0, s)

    assert call() == 0
    assert call(ncols=0) == -1 and call(ncols=9) == -1 and call(ncols=8, ldc=4) == -1
    assert call(q=0) == -1 and call(o=0) == -1 and call(Nq=0) == -1 and call(Nkv=0) == -1
    assert call(q=buf.data_ptr() + 2) == -2 and call(k=buf.data_ptr() + 8) == -2      # pointers off the 16-byte grid
    assert call(ldq=76) == -2 and call(ldk=84) == -2                                  # row strides that are no multiple of 8
    assert call(o=out.data_ptr() + 2) == -2
    torch.cuda.synchronize()
    # only the valid call wrote: its [B, N, 3] result (q = k = 0: a uniform softmax over an all-ones column sums to exactly 1)
    assert (out.flatten()[:B * N * 3] == 1).all() and (out.flatten()[B * N * 3:] == 0).all()


# ---- wiring: the TRAJ_CONFIG model of tests/test_gpu_sampler.py, latent 8 x 16, B = 2 ----------------------------------------------------
def _model():
    from tests.test_gpu_sampler import model
    return model(dev())


def _cond(cfg, B=2, h=8, w=16):
    d = dev()
    cond = {"c_concat": [G.T("ap.cc", (B, 5, h, w)).to(d)], "c_crossattn": [G.T("ap.c", (B, 77, cfg.context_dim)).to(d)]}
    uc = {"c_concat": cond["c_concat"], "c_crossattn": [G.T("ap.uc", (B, 77, cfg.context_dim)).to(d)]}
    return cond, uc, G.T("ap.x_T", (B, 4, h, w)).to(d)


def test_probe_records_what_the_attention_kernel_sees(monkeypatch):
    from leftrefill_amd import ops
    m, cfg = _model()
    unet = m.model.diffusion_model
    B, h, w = 2, 8, 16
    d = dev()
    x = G.T("ap.x", (B, 9, h, w)).to(d)
    t = torch.tensor([501, 501], device=d)
    ctx = G.T("ap.ctx", (B, 77, cfg.context_dim)).to(d)
    calls = []
    orig = ops.attention_qkv

    def spy(qkv, B_, heads, L, scale):
        calls.append((qkv.clone(), B_, heads, L, scale))
        return orig(qkv, B_, heads, L, scale)

    monkeypatch.setattr(ops, "attention_qkv", spy)
    with torch.no_grad(), AP.AttentionProbe(unet) as probe:
        unet(x, t, ctx)
    assert probe.steps == 1 and len(calls) >= 2
    assert probe.num_layers == len(calls) and probe.recorded == list(range(len(calls)))
    sizes = set()
    for l, (qkv, B_, heads, L, scale) in enumerate(calls):
        C = heads * 64
        raw = probe.raw(l)
        hl, wl = raw.shape[1:3]
        assert B_ == B and raw.shape == (B, hl, wl, 3) and hl * wl == L and wl == 2 * hl, (l, raw.shape, L)
        cols = AP.canvas_columns(hl, wl, qkv.dtype, d)
        ref = AP.probe_reference(qkv[:, :C], qkv[:, C:2 * C], cols, B, heads, L, L, scale)
        check(f"probe layer {l} ({hl}x{wl}, {heads} heads)", raw.reshape(B, L, 3), ref, cols, qkv.dtype)
        sizes.add(L)
    assert min(sizes) == 2 and max(sizes) == h * w      # from the deepest level's two tokens to the full canvas
    # a layer selection records only those layers and counts all of them
    n = len(calls)
    with torch.no_grad(), AP.AttentionProbe(unet, layers=[1]) as some:
        unet(x, t, ctx)
    assert some.recorded == [1] and some.num_layers == n and torch.equal(some.raw(1), probe.raw(1))


@pytest.fixture(scope="module")
def runs():
    """One 5-step DDIM sampling (scale 2.5, fixed x_T, eta 0) of the TRAJ model by every route under test."""
    import ldm.models.diffusion.ddim as ddim_mod
    m, cfg = _model()
    unet = m.model.diffusion_model
    cond, uc, x_T = _cond(cfg)
    kw = dict(cond=cond, batch_size=2, ddim=True, ddim_steps=5, eta=0.0, x_T=x_T, unconditional_conditioning=uc)
    r = {"m": m}
    r["captured"], _ = m.sample_log(unconditional_guidance_scale=2.5, **kw)
    unet.eager_only = True
    try:
        r["eager"], _ = m.sample_log(unconditional_guidance_scale=2.5, **kw)
    finally:
        del unet.eager_only
    with AP.AttentionProbe(unet) as probe:
        r["probed"], _ = m.sample_log(unconditional_guidance_scale=2.5, **kw)
    r["probe"] = probe
    r["attn"] = m.sample_log(unconditional_guidance_scale=2.5, return_attn=True, **kw)
    r["attn1"] = m.sample_log(unconditional_guidance_scale=1.0, return_attn=True, **kw)
    assert ddim_mod.DDIMSampler is not None
    return r


def test_sampling_under_a_probe_is_the_eager_sampling(runs):
    from leftrefill_amd import engine
    assert engine.PROBE is None
    assert runs["probe"].steps == 5
    d = (runs["probed"] - runs["captured"]).abs().max().item()
    print(f"[probe ddim] max|probed - captured| = {d:.3e} (captured step with the CFG shared prefix; scale {runs['captured'].abs().max().item():.2f})")
    assert torch.equal(runs["probed"], runs["eager"])


def test_sample_return_attn(runs):
    B, h, w = 2, 8, 16
    probe = runs["probe"]
    assert len(runs["attn"]) == 3
    samples, inter, att = runs["attn"]
    assert torch.equal(samples, runs["probed"]) and set(inter) == {"x_inter", "pred_x0"}
    assert len(att) == len(probe.recorded) == probe.num_layers
    for l, a in enumerate(att):
        raw = probe.raw(l)[..., 0]
        assert raw.shape[0] == 2 * B      # [uncond; cond]
        assert a.is_cuda and a.dtype == torch.float32 and a.shape == (B,) + tuple(raw.shape[1:])
        want = AP.fold_cfg(raw[:B] / probe.steps, raw[B:] / probe.steps, 2.5)
        assert (a - want).abs().max().item() <= 1e-6, l
    assert att[0].shape == (B, h, w)
    A, R = TOL[torch.float16]
    _, _, att1 = runs["attn1"]
    lo, hi = min(a.min().item() for a in att1), max(a.max().item() for a in att1)
    print(f"[return_attn scale 1] maps in {lo:.4f} .. {hi:.4f}")
    assert len(att1) == len(att) and all(a.shape[0] == B for a in att1)
    assert lo >= -(A + R) and hi <= 1 + A + R


def test_refusals(runs):
    import ldm.models.diffusion.ddim as ddim_mod
    from leftrefill_amd import engine
    m = runs["m"]
    unet = m.model.diffusion_model
    cond, uc, x_T = _cond(G.CONFIGS[G.TRAJ_CONFIG])
    with pytest.raises(NotImplementedError, match="ucg_schedule"):
        ddim_mod.DDIMSampler(m).sample(5, 2, (4, 8, 16), cond, verbose=False, x_T=x_T, unconditional_guidance_scale=2.5,
                                       unconditional_conditioning=uc, ucg_schedule=[2.5] * 5, return_attn=True)
    x = G.T("ap.x", (2, 9, 8, 16)).to(dev())
    ctx = G.T("ap.ctx", (2, 77, G.CONFIGS[G.TRAJ_CONFIG].context_dim)).to(dev())
    with pytest.raises(NotImplementedError, match="grad-enabled"):
        with torch.enable_grad(), AP.AttentionProbe(unet):
            unet(x, torch.tensor([5, 5], device=dev()), ctx)
    assert engine.PROBE is None
    from ldm.modules.diffusionmodules.multiview_unet import MultiViewUnetModel
    mv = MultiViewUnetModel(**G.mv_config(3, True).kwargs()).to(dev()).eval()
    with pytest.raises(NotImplementedError, match="multi-view"):
        with AP.AttentionProbe(mv):
            pass
    assert engine.PROBE is None
    engine.MV_SHARDED = True
    try:
        with pytest.raises(NotImplementedError, match="MV_SHARDED"):
            with AP.AttentionProbe(unet):
                pass
    finally:
        engine.MV_SHARDED = False


def test_log_images_return_attn_and_the_logger_panels(tmp_path):
    """log_images(return_attn=True): today's keys and values plus `att_scores`; the logger appends one viridis panel per map."""
    pytest.importorskip("matplotlib")
    import leftrefill_amd.dropin as dropin
    dropin.install()
    from inpainting_ldm.logger import InpaintingLogger
    from inpainting_ldm.ref_inpainting_ldm import RefInpaintLDM
    from oracle import weights
    d = dev()
    cfg = G.CONFIGS[G.TRAJ_CONFIG]
    dd = dict(double_z=True, z_channels=4, resolution=64, in_channels=3, out_ch=3, ch=64, ch_mult=[1, 2, 4, 4],
              num_res_blocks=1, attn_resolutions=[], dropout=0.0)
    m = RefInpaintLDM(first_stage_config={"target": "ldm.models.autoencoder.AutoencoderKL",
                                          "params": {"ddconfig": dd, "embed_dim": 4, "lossconfig": {"target": "torch.nn.Identity"}}},
                      cond_stage_config={"target": "torch.nn.Identity"},
                      unet_config={"target": "ldm.modules.diffusionmodules.openaimodel.UNetModel", "params": cfg.kwargs()},
                      conditioning_key="hybrid", scale_factor=0.18215, linear_start=0.00085, linear_end=0.0120,
                      timesteps=1000, channels=4, first_stage_key="image", cond_stage_key="txt",
                      cond_stage_trainable=True, data_config={"img_size": 64})
    m.model.diffusion_model.load_state_dict(G.unet_state(G.TRAJ_CONFIG), strict=True)
    m.first_stage_model.load_state_dict({k: torch.from_numpy(weights.fill_like("vae2." + k, v.shape))
                                         for k, v in m.first_stage_model.state_dict().items()})
    B, S = 2, 64
    ctx_c, ctx_u = G.T("e2e.c", (B, 77, cfg.context_dim)), G.T("e2e.u", (B, 77, cfg.context_dim))

    class Prompt(torch.nn.Module):
        def encode(self, txt):
            return (ctx_u if txt[0] == "" else ctx_c).to(d)

    m.cond_stage_model = Prompt()
    m = m.to(d).eval()
    img = G.T("e2e.img", (B, S, 2 * S, 3), "unit")
    mask = torch.zeros(B, S, 2 * S, 1)
    mask[:, 16:48, S + 8:S + 40] = 1.0
    batch = {"image": img.to(d), "mask": mask.to(d), "masked_image": (img * (mask < 0.5)).to(d), "txt": ["p"] * B}
    kw = dict(ddim_steps=5, ddim_eta=0.0, unconditional_guidance_scale=2.5)
    unet = m.model.diffusion_model

    def run(**extra):
        torch.manual_seed(7)      # the start noise and the VAE posterior sample
        return m.log_images(batch, B, **kw, **extra)

    plain = run()
    unet.eager_only = True
    try:
        eager = run()
    finally:
        del unet.eager_only
    out = run(return_attn=True)
    assert set(plain) == {"masked_image", "origin_image", "pred"} and set(out) == set(plain) | {"att_scores"}
    for k in ("masked_image", "origin_image"):
        assert torch.equal(out[k], plain[k])
    print(f"[log_images return_attn] max|pred - captured pred| = {(out['pred'].float() - plain['pred'].float()).abs().max().item():.3e}")
    assert torch.equal(out["pred"], eager["pred"])
    att = out["att_scores"]
    assert len(att) >= 2 and att[0].shape == (B, S // 8, 2 * S // 8) and all(a.is_cuda and a.shape[0] == B for a in att)
    # the logger: the image keys by the device route, the panels appended on the right
    lg = InpaintingLogger(batch_frequency=1, max_images=2, save_dir="s")
    canvas, full = lg.canvas(plain), lg.canvas(out)
    pw = 2 * S + 4
    assert full.shape == (canvas.shape[0], canvas.shape[1] + len(att) * pw, 3) and np.array_equal(full[:, :canvas.shape[1]], canvas)
    assert full[:, canvas.shape[1]:].reshape(-1, 3).std(axis=0).max() > 0      # (not one flat colour)
    lg.log_local(str(tmp_path), "train", out, 3, 0, 0)
    from PIL import Image
    im = Image.open(str(tmp_path / "s" / "train" / "gs-000003_e-000000_b-000000.jpg"))
    assert im.size == (full.shape[1], full.shape[0])


def test_refill_return_attn(synthetic, tmp_path):  # noqa: F811
    from PIL import Image
    from leftrefill_amd import refill as R
    root, _, _, model = synthetic
    source, mask, reference = (Image.open(str(root / (n + ".png"))) for n in ("source", "mask", "reference"))
    kw = dict(steps=STEPS, scale=2.5, num_samples=2, size=64, seed=0)
    torch.manual_seed(0)
    plain = R.refill(model, source, mask, reference, **kw)
    torch.manual_seed(0)
    images, attn = R.refill(model, source, mask, reference, return_attn=True, **kw)
    assert len(images) == len(plain) == 2
    assert all(np.array_equal(np.asarray(a), np.asarray(b)) for a, b in zip(images, plain))
    assert set(attn) == {"mass", "correspondence"} and len(attn["mass"]) == len(attn["correspondence"]) >= 2
    A, R_ = TOL[torch.float16]
    for l, (ms, co) in enumerate(zip(attn["mass"], attn["correspondence"])):
        N, h, w2 = ms.shape
        assert ms.is_cuda and co.is_cuda and N == 2 and co.shape == (N, h, w2, 2), l
        assert (ms >= -(A + R_)).all() and (ms <= 1 + A + R_).all(), l
        assert torch.isfinite(co[ms > 0]).all(), l
    pl = R.plan((96, 70), 64)      # size 64 pads to a 128 x 256 canvas: the maps cover the padded target half
    assert attn["mass"][0].shape == (2, pl["H"] // 8, pl["W"] // 8) == (2, 16, 16)
    # tools/refill.py --attn_maps: one viridis PNG of the result's size and one correspondence array per image and layer
    pytest.importorskip("matplotlib")
    import importlib.util
    import os
    spec = importlib.util.spec_from_file_location("refill_tool", os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools", "refill.py"))
    tool = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(tool)
    tool.write_attn_maps(str(tmp_path / "maps"), images, attn, 64)
    L = len(attn["mass"])
    assert sorted(os.listdir(str(tmp_path / "maps"))) == sorted([f"attn_{i:02d}_l{l:02d}.png" for i in range(2) for l in range(L)] +
                                                                [f"corr_{i:02d}_l{l:02d}.npy" for i in range(2) for l in range(L)])
    assert Image.open(str(tmp_path / "maps" / "attn_01_l00.png")).size == images[1].size
    corr = np.load(str(tmp_path / "maps" / "corr_00_l00.npy"))
    assert corr.shape == (8, 8, 2) and corr.dtype == np.float32      # the unpadded 64 x 64 target: 8 x 8 tokens
    assert np.array_equal(corr, attn["correspondence"][0][0, :8, :8].cpu().numpy(), equal_nan=True)
