"""GPU: seeded sampling noise -- lr_seeded_normal (csrc/seeded_noise.hip) against the float64 statement (leftrefill_amd/noise.py), its
bitwise properties device against device, its moments and refusals; the samplers' `seeds=` keyword on an element-wise stub model, bit for
bit; `refill(noise="seeded")` on the synthetic model of tests/test_gpu_refill.py (constructed here the same way).

The parity bound, |z_dev - z_f64| <= K 2^-24 max(r, 1) with r = sqrt(-2 ln u1) of the element and z_f64 the statement BEFORE its rounding:

  Write e = 2^-24.  An error of a ulps of a fp32 value v is at most 2 a e |v| (ulp(v) <= 2^-23 |v|).  Both uniforms and the argument
  2 u2 of sincospif are exact in fp32 (24 significant bits), so every error below is a function's own.
    L = -2 logf(u1)        logf within a_log ulp: relative error of L <= 2 a_log e (the factor -2 is exact)
    r = sqrtf(L)           halves the relative error of L and adds a_sqrt ulp: relative error of r <= (a_log + 2 a_sqrt) e
    c = cospi / sinpi      within a_sc ulp, |c| <= 1: absolute error <= 2 a_sc e
    z = r * c              one rounding: <= e |z| <= e r
  so |z_dev - z_f64| <= r e (a_log + 2 a_sqrt + 2 a_sc + 1), and max(r, 1) >= r covers r < 1 as well.
  Values used: a_log = 2, a_sqrt = 1, a_sc = 1.  Read from: the "maximum ULP difference" column of the single-precision table of the
  HIP math API reference (ROCm documentation, "HIP math API"), which lists 1 for sqrtf and for sincospif and no more than 2 for logf;
  the table is not vendored in this tree, so these are the figures as noted when the test was written, taken at the larger value
  where there was doubt (sqrtf is moreover the correctly rounded form under hipcc's default
  -fhip-fp32-correctly-rounded-divide-sqrt, i.e. 0.5).  That gives 2 + 2 + 2 + 1 = 7 <= K = 8; with 1 ulp for logf it is 6.  (The
  issue's estimate of about 4.5 counts a ulp as 1.5 e on average; the bound here counts it at its largest, 2 e.)  K was fixed from
  these numbers before the kernel ran; the measured maximum is printed, and written to profiles/seeded_noise_parity.json when
  LEFTREFILL_WRITE_PROFILES is set -- it plays no part in K, and a measurement above K would be a finding."""
import json
import os
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import seeded_noise_helpers as H  # noqa: E402
from leftrefill_amd import noise as N  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
K = 8.0
PER_SAMPLE = (1, 3, 4, 5, 1023, 4 * 8 * 16)


def dev():
    return torch.device("cuda:0")


def _draw(keys, stream, step, per, offset=0):
    """keys: [(seed, sub)] -> the device draw [B, per] written at `offset` floats past a 16-byte aligned base."""
    from leftrefill_amd import ops
    B = len(keys)
    sn = N.SeededNoise([k[0] for k in keys], subs=[k[1] for k in keys], device=dev())
    buf = torch.full((B * per + 8,), 7.0, device=dev())
    assert buf.data_ptr() % 16 == 0
    out = buf[offset:offset + B * per].view(B, per)
    ops.seeded_normal(sn.keys, stream, step, out)
    torch.cuda.synchronize()
    assert bool((buf[:offset] == 7.0).all()) and bool((buf[offset + B * per:] == 7.0).all()), "a store outside the output"
    return out


# ---- kernel against the statement ------------------------------------------------------------------------------------------------------
def test_kernel_against_the_statement():
    worst, rows = 0.0, []
    for per in PER_SAMPLE:
        for B in (1, 3):
            for offset in (0, 1):
                for k0 in range(0, len(H.KEYS), B):
                    keys = [H.KEYS[(k0 + b) % len(H.KEYS)] for b in range(B)]
                    for stream, step in {(k[2], k[3]) for k in keys}:
                        rows_here = [k for k in keys]
                        got = _draw([(k[0], k[1]) for k in rows_here], stream, step, per, offset).double().cpu().numpy()
                        for b, k in enumerate(rows_here):
                            z, r = N.normal_parts(k[0], k[1], stream, step, per)
                            ratio = float((np.abs(got[b] - z) / (2.0 ** -24 * np.maximum(r, 1.0))).max())
                            worst = max(worst, ratio)
                            rows.append(dict(per_sample=per, B=B, offset=offset, seed=k[0], sub=k[1], stream=stream, step=step, err_over_unit=ratio))
                            assert ratio <= K, (per, B, offset, k, stream, step, ratio)
    # a long draw of every key, so that the measured maximum means something
    got = _draw([(k[0], k[1]) for k in H.KEYS], N.STEP, 49, 2 ** 16).double().cpu().numpy()
    for b, k in enumerate(H.KEYS):
        z, r = N.normal_parts(k[0], k[1], N.STEP, 49, 2 ** 16)
        ratio = float((np.abs(got[b] - z) / (2.0 ** -24 * np.maximum(r, 1.0))).max())
        worst = max(worst, ratio)
        rows.append(dict(per_sample=2 ** 16, B=len(H.KEYS), offset=0, seed=k[0], sub=k[1], stream=N.STEP, step=49, err_over_unit=ratio))
        assert ratio <= K, (k, ratio)
    print(f"[seeded noise parity] max |z_dev - z_f64| / (2^-24 max(r, 1)) = {worst:.3f} over {len(rows)} rows (bound K = {K})")
    if os.environ.get("LEFTREFILL_WRITE_PROFILES"):
        out_dir = os.environ.get("LEFTREFILL_PROFILE_DIR") or os.path.join(ROOT, "profiles")
        with open(os.path.join(out_dir, "seeded_noise_parity.json"), "w") as f:
            json.dump(dict(unit="2^-24 max(r, 1)", K=K, measured_max=worst, rows=rows), f, indent=1)


# ---- bitwise, device against device ----------------------------------------------------------------------------------------------------
def test_bitwise_properties():
    keys = [(3, 0), (2 ** 40 + 7, 3), (9, 1)]
    for per in (5, 1023, 512):
        a = _draw(keys, N.STEP, 2, per)
        assert torch.equal(a, _draw(keys, N.STEP, 2, per))                                  # two runs
        assert torch.equal(a[2:], _draw(keys[2:], N.STEP, 2, per))                          # row 2 of B = 3 == the key alone
        assert torch.equal(a, _draw(keys, N.STEP, 2, per, offset=1))                        # 16-byte stores == scalar stores
        assert torch.equal(a[1, :4], _draw(keys[1:2], N.STEP, 2, 4)[0])                     # element i does not depend on per_sample
        for other in (_draw(keys, N.STEP, 3, per), _draw(keys, N.KNOWN, 2, per)):           # step / stream change every group
            full = per // 4 * 4
            same = (a[:, :full].reshape(3, -1, 4) == other[:, :full].reshape(3, -1, 4)).all(dim=2)
            assert not bool(same.any())
    # SeededNoise on the device: one launch, any per-sample shape, the same values; keys above 2^63 and as tensors
    sn = N.SeededNoise([k[0] for k in keys], subs=[k[1] for k in keys], device=dev())
    z = sn.normal(N.STEP, 2, (4, 8, 16))
    assert z.shape == (3, 4, 8, 16) and torch.equal(z.reshape(3, -1), _draw(keys, N.STEP, 2, 512))
    assert torch.equal(sn.shard(1, 3).normal(N.STEP, 2, (512,)), z.reshape(3, -1)[1:])
    assert torch.equal(sn.row0().normal(N.STEP, 2, (512,)), z.reshape(3, -1)[:1].expand(3, 512))
    assert torch.equal(N.SeededNoise(sn.keys).normal(N.STEP, 2, (512,)), z.reshape(3, -1))
    big = 2 ** 64 - 5
    got = N.SeededNoise([big], device=dev()).normal(N.START, 0, (64,))[0].double().cpu().numpy()
    zz, r = N.normal_parts(big, 0, N.START, 0, 64)
    assert (np.abs(got - zz) <= K * 2.0 ** -24 * np.maximum(r, 1.0)).all()


def test_offsets_past_2_31_elements():
    """B = 2 rows of 2^30 + 5 elements: the second row starts 2^30 + 5 floats in (unaligned: scalar stores), its end lies past 2^31
    elements and 2^33 bytes -- every index is 64-bit.  Only the ends of the rows are compared; nothing is written past the output."""
    from leftrefill_amd import ops
    per, keys = 2 ** 30 + 5, [(3, 0), (2 ** 40 + 7, 3)]
    sn = N.SeededNoise([k[0] for k in keys], subs=[k[1] for k in keys], device=dev())
    buf = torch.empty(2 * per + 4, device=dev())
    buf[-4:] = 7.0
    out = ops.seeded_normal(sn.keys, N.STEP, 1, buf[:2 * per].view(2, per))
    torch.cuda.synchronize()
    assert bool((buf[-4:] == 7.0).all())
    for b, (seed, sub) in enumerate(keys):
        for first, n in ((0, 9), (2 ** 29 - 3, 9), (per - 9, 9)):
            z, r = N.normal_parts(seed, sub, N.STEP, 1, n, first=first)
            got = out[b, first:first + n].double().cpu().numpy()
            assert (np.abs(got - z) <= K * 2.0 ** -24 * np.maximum(r, 1.0)).all(), (b, first)
    del out, buf
    torch.cuda.empty_cache()


# ---- moments ---------------------------------------------------------------------------------------------------------------------------
def test_moments_of_one_device_draw():
    """The five keys differ in (stream, step) as well, so each is its own launch of 2^20 values."""
    zs = [_draw([(s, u)], st, k, H.N_MOMENTS)[0].cpu().numpy() for s, u, st, k in H.KEYS]
    H.check_moments(zs, "device")


# ---- refusals --------------------------------------------------------------------------------------------------------------------------
def test_refusals_launch_nothing():
    from leftrefill_amd import _lib
    lib = _lib.load()
    keys = N.SeededNoise([1, 2], device=dev()).keys
    out = torch.full((2, 64), 7.0, device=dev())
    st = torch.cuda.current_stream().cuda_stream
    call = lambda k, B, per, o: lib.lr_seeded_normal(k, B, per, N.STEP, 0, o, st)
    assert call(0, 2, 64, out.data_ptr()) == -1 and call(keys.data_ptr(), 2, 64, 0) == -1
    assert call(keys.data_ptr(), 0, 64, out.data_ptr()) == -1 and call(keys.data_ptr(), -1, 64, out.data_ptr()) == -1
    assert call(keys.data_ptr(), 2, 0, out.data_ptr()) == -1 and call(keys.data_ptr(), 2, -4, out.data_ptr()) == -1
    assert call(keys.data_ptr(), 1, 4 * 2 ** 32, out.data_ptr()) == -1 and call(keys.data_ptr(), 1, 2 ** 40, out.data_ptr()) == -1
    assert call(keys.data_ptr(), 2, 32, out.data_ptr() + 2) == -2
    torch.cuda.synchronize()
    assert bool((out == 7.0).all())
    assert call(keys.data_ptr(), 2, 64, out.data_ptr()) == 0      # the same arguments untouched are served
    torch.cuda.synchronize()
    assert not bool((out == 7.0).any())


# ---- samplers, bitwise -----------------------------------------------------------------------------------------------------------------
SEEDS, ONE = [3, 5, 9], 1          # the batch, and the row sampled alone
S, ETA, SCALE = 4, 1.0, 2.5


@pytest.fixture(scope="module")
def stub():
    return H.stub_model(dev())


def _rows(seeds, stream):
    return torch.stack([H.keyed(s, stream) for s in seeds]).to(dev())


def _inputs(seeds):
    """Conditioning, unconditional conditioning, simple conditioning, clean latent: functions of each sample's seed; one mask for all."""
    mask = torch.zeros(1, 1, 8, 16, device=dev())
    mask[..., :, :7] = 1.0
    return dict(c=_rows(seeds, 100), uc=_rows(seeds, 101), cs=_rows(seeds, 102), x0=_rows(seeds, 103), mask=mask.expand(len(seeds), 1, 8, 16).contiguous())


class _RngUntouched:
    def __enter__(self):
        self.cpu, self.cuda = torch.get_rng_state(), torch.cuda.get_rng_state(dev())

    def __exit__(self, *exc):
        if exc[0] is None:
            assert torch.equal(self.cpu, torch.get_rng_state()) and torch.equal(self.cuda, torch.cuda.get_rng_state(dev()))


def _ddim(stub, rows, masked=False, **kw):
    """rows: the seeds that name the batch's inputs; kw may carry `seeds=` or `x_T=`."""
    from ldm.models.diffusion.ddim import DDIMSampler
    i = _inputs(rows)
    extra = dict(mask=i["mask"], x0=i["x0"]) if masked else {}
    out, _ = DDIMSampler(stub).sample(S, len(rows), H.LATENT, i["c"], verbose=False, eta=ETA, unconditional_guidance_scale=SCALE,
                                      unconditional_conditioning=i["uc"], **extra, **kw)
    return out


def _structure(stub, seeds, masked=False):
    from ldm.models.diffusion.ddim import StructureDDIMSampler
    i = _inputs(seeds)
    extra = dict(mask=i["mask"], x0=i["x0"]) if masked else {}
    out, _ = StructureDDIMSampler(stub).sample(S, len(seeds), H.LATENT, i["c"], verbose=False, eta=ETA, unconditional_guidance_scale=SCALE,
                                               unconditional_conditioning=i["uc"], Tm=2, cond_simple=i["cs"], cond_weight=0.6, seeds=seeds,
                                               **extra)
    return out


def _ddpm(stub, rows, masked=False, **kw):
    i = _inputs(rows)
    extra = dict(mask=i["mask"], x0=i["x0"]) if masked else {}
    # LatentDiffusion.sample -> p_sample_loop: the ancestral loops keep the reference's parameter lists, `seeds` travels through **kwargs
    return stub.sample(i["c"], batch_size=len(rows), shape=(len(rows),) + H.LATENT, timesteps=S, verbose=False, **extra, **kw)


def _encode(stub, seeds, t):
    from ldm.models.diffusion.ddim import DDIMSampler
    s = DDIMSampler(stub)
    s.make_schedule(S, ddim_eta=ETA, verbose=False)
    return s.stochastic_encode(_inputs(seeds)["x0"], t, seeds=seeds)


@pytest.mark.parametrize("name", ["ddim", "ddim_masked", "structure", "structure_masked", "ddpm", "ddpm_known", "stochastic_encode"])
def test_a_sample_does_not_depend_on_its_batch(stub, name):
    """sample(seeds=[3, 5, 9])[1] == sample(seeds=[5])[0], bit for bit, and no generator moves."""
    run = {"ddim": lambda s: _ddim(stub, s, seeds=s), "ddim_masked": lambda s: _ddim(stub, s, masked=True, seeds=s),
           "structure": lambda s: _structure(stub, s), "structure_masked": lambda s: _structure(stub, s, masked=True),
           "ddpm": lambda s: _ddpm(stub, s, seeds=s), "ddpm_known": lambda s: _ddpm(stub, s, masked=True, seeds=s),
           "stochastic_encode": lambda s: _encode(stub, s, [1, 2, 3] if len(s) == 3 else [2])}[name]
    with _RngUntouched():
        batch, alone = run(SEEDS), run(SEEDS[ONE:ONE + 1])
    assert batch.shape == (3,) + H.LATENT and torch.isfinite(batch).all()
    assert torch.equal(batch[ONE], alone[0])
    assert not torch.equal(batch[0], batch[ONE]) and not torch.equal(batch[2], batch[ONE])
    # the forms of `seeds`: a [B] tensor and a SeededNoise give the same draws; another sub-sample number gives others
    if name == "ddim":
        assert torch.equal(_ddim(stub, SEEDS, seeds=torch.tensor(SEEDS)), batch)
        assert torch.equal(_ddim(stub, SEEDS, seeds=N.SeededNoise(SEEDS, device=dev())), batch)
        assert not torch.equal(_ddim(stub, SEEDS, seeds=N.SeededNoise(SEEDS, subs=[0, 1, 0]))[ONE], batch[ONE])
        with pytest.raises(ValueError, match="2 keys for a batch of 3"):
            _ddim(stub, SEEDS, seeds=[1, 2])
    if name == "ddpm_known":      # a direct call of the loop, and of the chain with its x0 predictions, inside the context manager
        i = _inputs(SEEDS)
        with stub.seeded_noise(SEEDS):
            direct = stub.p_sample_loop(i["c"], (3,) + H.LATENT, timesteps=S, verbose=False, mask=i["mask"], x0=i["x0"])
            prog, _ = stub.progressive_denoising(i["c"], (3,) + H.LATENT, verbose=False, mask=i["mask"], x0=i["x0"], start_T=S)
        assert stub._seeded == (None, 0) and torch.equal(direct, batch) and torch.equal(prog, batch)


class _NoiseLike:
    """While active: the k-th noise_like call of module `mod` returns noises[k]."""

    def __init__(self, mod, noises):
        self.mod, self.noises, self.k = mod, noises, 0

    def __enter__(self):
        self.orig = self.mod.noise_like

        def noise_like(shape, device, repeat=False):
            self.k += 1
            assert tuple(shape) == tuple(self.noises[self.k - 1].shape)
            return self.noises[self.k - 1]

        self.mod.noise_like = noise_like
        return self

    def __exit__(self, *exc):
        self.mod.noise_like = self.orig


def test_seeds_route_is_the_existing_route_fed_the_same_noise(stub):
    """The existing DDIM route driven with x_T and per-step noise from SeededNoise (through a monkeypatched noise_like) gives the `seeds=`
    result bit for bit: the plumbing adds nothing to the arithmetic."""
    import ldm.models.diffusion.ddim as ddim_mod
    sn = N.SeededNoise(SEEDS, device=dev())
    with _NoiseLike(ddim_mod, [sn.normal(N.STEP, k, H.LATENT) for k in range(S)]) as inj:
        fed = _ddim(stub, SEEDS, x_T=sn.normal(N.START, 0, H.LATENT))
    assert inj.k == S
    assert torch.equal(fed, _ddim(stub, SEEDS, seeds=SEEDS))


def test_without_seeds_the_global_generator_draws_as_before(stub):
    """seeds=None: the start code and then one noise_like per step come from torch's generator in the parent commit's call order (DDIM);
    for the ancestral loop with a known region: the start code, then per step noise_like and the randn_like of the known region."""
    import ldm.models.diffusion.ddim as ddim_mod
    import ldm.models.diffusion.ddpm as ddpm_mod
    shape = (3,) + H.LATENT
    torch.manual_seed(7)
    x_T = torch.randn(shape, device=dev())
    noises = [torch.randn(shape, device=dev()) for _ in range(S)]
    with _NoiseLike(ddim_mod, noises):
        want = _ddim(stub, SEEDS, x_T=x_T)
    torch.manual_seed(7)
    assert torch.equal(_ddim(stub, SEEDS), want)
    # DDPM with a known region, restated in torch from the drawn tensors
    i = _inputs(SEEDS)
    torch.manual_seed(7)
    x_T = torch.randn(shape, device=dev())
    draws = [(torch.randn(shape, device=dev()), torch.randn_like(i["x0"])) for _ in range(S)]
    orig = torch.randn_like
    k = [0]

    def randn_like(x, **kw):
        k[0] += 1
        return draws[k[0] - 1][1]

    torch.randn_like = randn_like
    try:
        with _NoiseLike(ddpm_mod, [d[0] for d in draws]):
            want = _ddpm(stub, SEEDS, masked=True, x_T=x_T)
    finally:
        torch.randn_like = orig
    assert k[0] == S
    torch.manual_seed(7)
    assert torch.equal(_ddpm(stub, SEEDS, masked=True), want)


def test_plms_and_dpm_take_the_start_code_from_the_keys(stub):
    from ldm.models.diffusion.dpm_solver.sampler import DPMSolverSampler
    from ldm.models.diffusion.plms import PLMSSampler
    i3, i1 = _inputs(SEEDS), _inputs(SEEDS[ONE:ONE + 1])
    start = N.SeededNoise(SEEDS, device=dev()).normal(N.START, 0, H.LATENT)
    for cls in (PLMSSampler, DPMSolverSampler):
        kw = dict(verbose=False, unconditional_guidance_scale=SCALE)
        a, _ = cls(stub).sample(S, 3, H.LATENT, i3["c"], unconditional_conditioning=i3["uc"], seeds=SEEDS, **kw)
        b, _ = cls(stub).sample(S, 1, H.LATENT, i1["c"], unconditional_conditioning=i1["uc"], seeds=SEEDS[ONE:ONE + 1], **kw)
        c, _ = cls(stub).sample(S, 3, H.LATENT, i3["c"], unconditional_conditioning=i3["uc"], x_T=start, **kw)
        assert torch.equal(a[ONE], b[0]) and torch.equal(a, c), cls.__name__


def test_repeat_noise_uses_row_zero(stub):
    from ldm.models.diffusion.ddim import DDIMSampler
    i = _inputs(SEEDS)
    s = DDIMSampler(stub)
    s.make_schedule(S, ddim_eta=ETA, verbose=False)
    x = torch.zeros((3,) + H.LATENT, device=dev())
    c0 = i["c"][:1].expand(3, -1, -1, -1).contiguous()
    t = torch.full((3,), int(s.ddim_timesteps[2]), device=dev(), dtype=torch.long)
    out, _ = s.p_sample_ddim(x, c0, t, index=2, repeat_noise=True, seeds=SEEDS, step=1)
    assert torch.equal(out[0], out[1]) and torch.equal(out[0], out[2])
    alone, _ = s.p_sample_ddim(x[:1], c0[:1], t[:1], index=2, seeds=SEEDS[:1], step=1)
    assert torch.equal(out[0], alone[0])


# ---- refill on the synthetic model of tests/test_gpu_refill.py --------------------------------------------------------------------------
def _write_config(path, size):
    import yaml
    from oracle import golden_spec as G
    cfg = G.CONFIGS["MID"]
    dd = dict(double_z=True, z_channels=4, resolution=size, in_channels=3, out_ch=3, ch=64, ch_mult=[1, 2, 4, 4],
              num_res_blocks=1, attn_resolutions=[], dropout=0.0)
    model = {"target": "inpainting_ldm.ref_inpainting_ldm.RefInpaintLDM", "params": dict(
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
        yaml.safe_dump({"model": model}, f)


def _pair(hs, ws, hr, wr, seed):
    rng = np.random.RandomState(seed)
    source = rng.randint(0, 256, (hs, ws, 3), dtype=np.uint8)
    reference = rng.randint(0, 256, (hr, wr, 3), dtype=np.uint8)
    mask = np.zeros((hs, ws, 3), np.uint8)
    mask[hs // 4:hs // 2, ws // 5:ws // 2] = 255
    mask[hs // 2:hs // 2 + 3, :] = 255
    return source, mask, reference


@pytest.fixture(scope="module")
def synthetic(tmp_path_factory):
    from oracle import golden_spec as G, weights
    root = tmp_path_factory.mktemp("seeded_refill")
    stub_dir = root / "stubs"
    stub_dir.mkdir()
    _write_config(str(root / "model_config.yaml"), 64)
    (stub_dir / "open_clip.py").write_text("from oracle.clip_stub import *  # noqa: F401,F403  (test stand-in for the absent package)\n")
    import leftrefill_amd.dropin as dropin
    dropin.install()
    sys.path.insert(0, str(stub_dir))
    try:
        from inpainting_ldm.model import create_model
        model = create_model(str(root / "model_config.yaml"))
    finally:
        sys.path.remove(str(stub_dir))
    sd = dict(model.state_dict())
    for k, v in model.state_dict().items():
        if k.startswith("first_stage_model."):
            sd[k] = torch.from_numpy(weights.fill_like("vae2." + k[len("first_stage_model."):], v.shape)).to(v.dtype)
    for k, v in G.unet_state("MID").items():
        sd["model.diffusion_model." + k] = v
    model.load_state_dict(sd, strict=False)
    return root, stub_dir, model.to("cuda").eval()


def _bytes(groups):
    return [np.asarray(im) for g in groups for im in g]


def test_refill_seeded_depends_on_the_inputs_and_the_seed_alone(synthetic):
    from leftrefill_amd import refill as R
    synthetic = synthetic[2]
    a, b = _pair(96, 70, 50, 120, 1), _pair(50, 120, 96, 70, 2)
    args = ([a[0], b[0]], [a[1], b[1]], [a[2], b[2]])
    kw = dict(steps=4, scale=2.5, num_samples=2, size=64, noise="seeded", seed=[3, 5])
    torch.manual_seed(1)
    first = R.refill(synthetic, *args, **kw)
    torch.randn(1000)
    torch.randn(1000, device="cuda")
    np.random.randn(10)
    second = R.refill(synthetic, *args, **kw)
    assert [[im.size for im in g] for g in first] == [[(46, 64)] * 2, [(153, 64)] * 2]
    assert all(np.array_equal(x, y) for x, y in zip(_bytes(first), _bytes(second)))
    assert not np.array_equal(_bytes(first)[0], _bytes(first)[1])      # sub-samples 0 and 1 of one seed differ
    with pytest.raises(ValueError, match="'torch' or 'seeded'"):
        R.refill(synthetic, *args, **dict(kw, noise="philox"))


def _sample_latents_before(model, image, masked_image, mask, txt, steps, scale, seeds, num_samples):
    """`sample_latents` as it stood before the `noise` argument, restated: the call order that noise="torch" must keep."""
    import torch.nn.functional as F
    from ldm.models.diffusion.ddim import DDIMSampler
    n, _, hh, w2 = image.shape
    h, w = hh // 8, w2 // 8
    batch = {"image": image, "masked_image": masked_image, "mask": mask}
    c = model.cond_stage_model.encode([txt] * n)
    c_cat = []
    for ck in model.concat_keys:
        cc = batch[ck].float()
        if ck != model.masked_image_key:
            cc = F.interpolate(cc, size=(h, w))
        else:
            cc = model.get_first_stage_encoding(model.encode_first_stage(cc))
        c_cat.append(cc)
    c_cat = torch.cat(c_cat, dim=1)
    cond = {"c_concat": [c_cat], "c_crossattn": [c]}
    uc_full = {"c_concat": [c_cat], "c_crossattn": [model.get_unconditional_conditioning(n)]}
    start = np.concatenate([np.random.RandomState(s).randn(num_samples, 4, h, w) for s in seeds], axis=0)
    start = torch.from_numpy(start).to(device=image.device, dtype=torch.float32)
    samples, _ = DDIMSampler(model).sample(steps, n, [model.channels, h, w], cond, verbose=False, eta=1.0, unconditional_guidance_scale=scale,
                                           unconditional_conditioning=uc_full, x_T=start)
    return model.decode_first_stage(samples)


def test_refill_torch_noise_is_what_it_was(synthetic):
    from leftrefill_amd import refill as R
    synthetic = synthetic[2]
    a = _pair(96, 70, 50, 120, 1)
    txt = R.prompt(4, "<special-token>")
    with torch.no_grad(), torch.autocast("cuda"):
        image, masked_image, mask = R.prepare_device([a[0]], [a[1]], [a[2]], 64, 2, torch.device("cuda"))
        torch.manual_seed(11)
        want = _sample_latents_before(synthetic, image, masked_image, mask, txt, 4, 2.5, [0], 2)
        torch.manual_seed(11)
        got = R.sample_latents(synthetic, image, masked_image, mask, txt, 4, 2.5, [0], 2, noise="torch")
        torch.manual_seed(11)
        default = R.sample_latents(synthetic, image, masked_image, mask, txt, 4, 2.5, [0], 2)
    assert torch.equal(got, want) and torch.equal(default, want)
    import inspect
    assert inspect.signature(R.refill).parameters["noise"].default == "torch"


# ---- the evaluation route: log_images(seeds=) and tools/run_inpainting.py --seeded_noise -----------------------------------------------
def _eval_batch(B, size=64):
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    try:
        import run_inpainting
    finally:
        sys.path.remove(os.path.join(ROOT, "tools"))
    batch = next(run_inpainting.synthetic_batches(1, B, size, repeat=4))
    return run_inpainting, {k: (v.cuda() if torch.is_tensor(v) else v) for k, v in batch.items()}


def test_log_images_with_seeds_ignores_the_generators(synthetic):
    model = synthetic[2]
    _, batch = _eval_batch(2)
    kw = dict(unconditional_guidance_scale=2.5, ddim_eta=1.0, ddim_steps=4)
    with torch.no_grad(), torch.autocast("cuda"):
        torch.manual_seed(1)
        a = model.log_images(dict(batch), 2, seeds=N.SeededNoise([5, 5], subs=[0, 1], device=dev()), **kw)["pred"]
        torch.randn(100, device="cuda")
        b = model.log_images(dict(batch), 2, seeds=N.SeededNoise([5, 5], subs=[0, 1], device=dev()), **kw)["pred"]
        c = model.log_images(dict(batch), 2, seeds=N.SeededNoise([5, 5], subs=[0, 2], device=dev()), **kw)["pred"]
    assert torch.isfinite(a).all() and torch.equal(a, b)
    assert not torch.equal(a[1], c[1])      # another sub-sample number: another image


def test_harness_takes_seeded_noise(synthetic, tmp_path, monkeypatch, capsys):
    """tools/run_inpainting.py --seeded_noise --seed 5, in process, on two synthetic batches of two items: the keys are (5, dataset index)."""
    root, stub_dir, _ = synthetic
    run_inpainting, _ = _eval_batch(1)
    keys = []
    from leftrefill_amd import noise as noise_mod
    real = noise_mod.SeededNoise

    class Recording(real):
        def __init__(self, seeds, subs=None, device=None):
            super().__init__(seeds, subs=subs, device=device)
            if subs is not None and not torch.is_tensor(seeds):
                keys.append(self.host_keys())

    monkeypatch.setattr(noise_mod, "SeededNoise", Recording)
    monkeypatch.syspath_prepend(str(stub_dir))
    monkeypatch.chdir(tmp_path)
    monkeypatch.setattr(sys, "argv", ["run_inpainting.py", "--model_path", str(root), "--synthetic", "2", "--batch_size", "2", "--test_size", "64",
                                      "--metric_size", "64", "--steps", "4", "--seeded_noise", "--seed", "5", "--device_metrics"])
    run_inpainting.main()
    out = capsys.readouterr().out
    assert "over 4 images" in out and "WARNING" not in out, out[-1500:]
    assert keys == [[(5, 0), (5, 1)], [(5, 2), (5, 3)]]
    assert sorted(os.listdir(str(tmp_path / "outputs"))) == ["0000_0.png", "0000_1.png", "0001_0.png", "0001_1.png"]
