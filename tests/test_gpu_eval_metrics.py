"""lr_eval_metrics (csrc/eval_metrics.hip) on the MI355X against `evalglue.metrics_reference`, the float64 CPU statement of the same
computation, on the same stored inputs; its exact cases, its determinism, and the device route of tools/run_inpainting.py and of
`validation_step` end to end.

Tolerance of the parity cases is measured, not fixed in advance: the FLOOR of an image family is the largest difference between a plain
fp32 restatement of the formulas on the CPU (`_fp32_restatement`: F.avg_pool2d box sums of the luma centred at 0.5, fp32 throughout,
fp32 results) and `metrics_reference` over that family's cases; the kernel gets 4 x that floor (its summation order differs), capped
at 1e-4 in SSIM and 1e-3 dB in PSNR -- the harness prints SSIM to 4 decimals and PSNR to 3.  Floors and observed maxima of the last run
on an MI355X (profiles/eval_metrics_parity.json):
    family   SSIM floor  tolerance  kernel max   PSNR floor (dB)  tolerance  kernel max (dB)
    noise    1.4e-7      5.7e-7     2.8e-8       2.9e-6           1.2e-5     1.8e-6
    ramp     2.2e-7      8.7e-7     3.0e-8       4.5e-6           1.8e-5     4.1e-6
    flat     2.5e-6      1.0e-5     3.0e-8       1.2e-5           4.6e-5     5.1e-6
The kernel's box sums and SSIM quotient are fp64 over the fp32 centred luma, so what remains is the rounding of its fp32 results
(SSIM near 1: 3e-8; a PSNR of 32 .. 64 dB: 1.9e-6, 64 .. 128 dB: 3.8e-6)."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

from oracle import golden_spec as G, weights  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SSIM_CAP, PSNR_CAP = 1e-4, 1e-3
DEV = "cuda"


def _family(name, n, h, w, seed):
    """(pred, origin) [n,3,h,w] fp32 in [-1, 1].  noise: uniform noise plus noise; ramp: a smooth ramp plus small noise; flat: 0.8 plus
    2e-3 noise -- nearly flat, the bad case for an fp32 variance."""
    g = torch.Generator().manual_seed(seed)
    if name == "noise":
        origin = torch.rand(n, 3, h, w, generator=g) * 2 - 1
        pred = origin + 0.05 * torch.randn(n, 3, h, w, generator=g)
    elif name == "ramp":
        yy, xx = torch.meshgrid(torch.linspace(-0.9, 0.9, h), torch.linspace(-0.9, 0.9, w), indexing="ij")
        base = torch.stack([xx, yy, 0.5 * (xx + yy)])[None].expand(n, 3, h, w)
        origin = base + 0.01 * torch.randn(n, 3, h, w, generator=g)
        pred = origin + 0.005 * torch.randn(n, 3, h, w, generator=g)
    else:
        origin = 0.8 + 2e-3 * torch.randn(n, 3, h, w, generator=g)
        pred = origin + 1e-3 * torch.randn(n, 3, h, w, generator=g)
    return pred.clamp(-1, 1).contiguous(), origin.clamp(-1, 1).contiguous()


def _block_mask(n, h, w, seed, cell=8):
    g = torch.Generator().manual_seed(1000 + seed)
    blocks = (torch.rand(n, 1, -(-h // cell), -(-w // cell), generator=g) < 0.5).float()
    return blocks.repeat_interleave(cell, 2).repeat_interleave(cell, 3)[:, :, :h, :w].contiguous()


def _fp32_restatement(pred, origin, mask, x0, Wc, r):
    """The same formulas in plain fp32 torch on the CPU: the floor of what fp32 arithmetic gives on these inputs."""
    p, o = pred.float(), origin.float()
    if mask is not None:
        p = p * mask + o * (1 - mask)
    p, o = p[:, :, :, x0:x0 + Wc], o[:, :, :, x0:x0 + Wc]
    if r > 1:
        size = (p.shape[2] // r, p.shape[3] // r)
        p, o = F.interpolate(p, size=size, mode="area"), F.interpolate(o, size=size, mode="area")
    p01, o01 = (p + 1) / 2, (o + 1) / 2
    psnr = 10.0 * torch.log10(1.0 / ((p01 - o01) ** 2).flatten(1).mean(1))
    a = 0.2989 * p01[:, 0] + 0.587 * p01[:, 1] + 0.114 * p01[:, 2] - 0.5
    b = 0.2989 * o01[:, 0] + 0.587 * o01[:, 1] + 0.114 * o01[:, 2] - 0.5
    box = lambda x: F.avg_pool2d(x[:, None], 7, 1)[:, 0]      # the windows that lie fully inside
    ca, cb = box(a), box(b)
    cov = 49.0 / 48.0
    va, vb, vab = cov * (box(a * a) - ca * ca), cov * (box(b * b) - cb * cb), cov * (box(a * b) - ca * cb)
    ua, ub = ca + 0.5, cb + 0.5
    c1, c2 = (0.01 * 2.0) ** 2, (0.03 * 2.0) ** 2
    s = ((2 * ua * ub + c1) * (2 * vab + c2)) / ((ua * ua + ub * ub + c1) * (va + vb + c2))
    assert psnr.dtype == s.dtype == torch.float32
    return psnr.double(), s.flatten(1).mean(1).double()


# (id, n, h, w, right_half, r, masked, pred dtype)
CASES = [
    ("512x1024_right_f16", 4, 512, 1024, True, 1, True, torch.float16),
    ("512x1024_right_bf16", 4, 512, 1024, True, 1, True, torch.bfloat16),
    ("512x1024_right_f32", 4, 512, 1024, True, 1, True, torch.float32),
    ("512x512_whole", 2, 512, 512, False, 1, True, torch.float32),
    ("r2", 2, 512, 1024, True, 2, True, torch.float32),
    ("r4", 2, 512, 1024, True, 4, True, torch.float16),
    ("no_mask", 2, 512, 1024, True, 1, False, torch.float32),
    ("40x80_right", 2, 40, 80, True, 1, True, torch.float32),
    ("33x66_right", 2, 33, 66, True, 1, True, torch.float16),
    ("narrower_than_a_tile", 2, 48, 20, False, 1, True, torch.float32),
]
FAMILIES = ("noise", "ramp", "flat")


def _case_inputs(family, case, seed):
    _, n, h, w, right, r, masked, dtype = case
    pred, origin = _family(family, n, h, w, seed)
    pred = pred.to(dtype)                                     # the stored prediction: both sides read these values
    mask = _block_mask(n, h, w, seed) if masked else None
    x0 = w // 2 if right else 0
    return pred, origin, mask, x0, w - x0, r


@pytest.mark.parametrize("family", FAMILIES)
def test_kernel_against_metrics_reference(family):
    """Item 5 of the issue: every case of CASES for one image family; prints each figure before it asserts and merges the family's
    floors / maxima into profiles/eval_metrics_parity.json when LEFTREFILL_WRITE_PROFILES is set."""
    from leftrefill_amd import evalglue, ops
    rows = []
    for ci, case in enumerate(CASES):
        pred, origin, mask, x0, Wc, r = _case_inputs(family, case, seed=10 * ci + FAMILIES.index(family))
        mse_r, psnr_r, ssim_r = evalglue.metrics_reference(pred, origin, mask, x0, Wc, r)
        psnr_f, ssim_f = _fp32_restatement(pred, origin, mask, x0, Wc, r)
        out, _ = ops.eval_metrics(pred.to(DEV), origin.to(DEV), None if mask is None else mask.to(DEV), x0=x0, Wc=Wc, r=r)
        out = out.cpu().double()
        row = dict(case=case[0], ssim=float(ssim_r.mean()), psnr=float(psnr_r.mean()),
                   ssim_floor=float((ssim_f - ssim_r).abs().max()), psnr_floor=float((psnr_f - psnr_r).abs().max()),
                   ssim_err=float((out[:, 2] - ssim_r).abs().max()), psnr_err=float((out[:, 1] - psnr_r).abs().max()),
                   mse_rel_err=float(((out[:, 0] - mse_r) / mse_r).abs().max()), nonfinite=float(out[:, 3].sum()))
        print(family, json.dumps(row))
        rows.append(row)
    ssim_floor, psnr_floor = max(r_["ssim_floor"] for r_ in rows), max(r_["psnr_floor"] for r_ in rows)
    ssim_tol, psnr_tol = min(4 * ssim_floor, SSIM_CAP), min(4 * psnr_floor, PSNR_CAP)
    ssim_max, psnr_max = max(r_["ssim_err"] for r_ in rows), max(r_["psnr_err"] for r_ in rows)
    summary = dict(ssim_floor=ssim_floor, ssim_tolerance=ssim_tol, ssim_kernel_max=ssim_max, psnr_floor_db=psnr_floor,
                   psnr_tolerance_db=psnr_tol, psnr_kernel_max_db=psnr_max, cases=rows)
    print(family, "SUMMARY", json.dumps({k: v for k, v in summary.items() if k != "cases"}))
    if os.environ.get("LEFTREFILL_WRITE_PROFILES"):
        path = os.path.join(os.environ["LEFTREFILL_WRITE_PROFILES"], "eval_metrics_parity.json")
        doc = json.load(open(path)) if os.path.exists(path) else {}
        doc[family] = summary
        with open(path, "w") as f:
            json.dump(doc, f, indent=1)
    assert all(r_["nonfinite"] == 0 for r_ in rows)
    assert ssim_max <= ssim_tol, (ssim_max, ssim_tol)
    assert psnr_max <= psnr_tol, (psnr_max, psnr_tol)


def test_exact_cases():
    """Item 6: identical images, known pixels, planted NaN / inf, the uint8 image bit for bit."""
    from leftrefill_amd import ops
    pred, origin = _family("noise", 2, 96, 200, seed=5)
    mask = _block_mask(2, 96, 200, seed=5)
    d = lambda t: t.to(DEV)
    # pred == origin: ssim == 1.0 exactly, psnr == inf (as psnr01), mse == 0
    out, _ = ops.eval_metrics(d(origin), d(origin), d(mask), x0=100, r=1)
    assert torch.equal(out[:, 2].cpu(), torch.ones(2)) and torch.isinf(out[:, 1]).all() and (out[:, 1] > 0).all()
    assert torch.equal(out[:, 0].cpu(), torch.zeros(2))
    out, _ = ops.eval_metrics(d(origin), d(origin), None, x0=0, r=2)
    assert torch.equal(out[:, 2].cpu(), torch.ones(2)) and torch.isinf(out[:, 1]).all()
    # known pixels (mask 0) contribute exactly zero squared error, whatever the prediction says there
    out, _ = ops.eval_metrics(d(pred), d(origin), d(torch.zeros_like(mask)), x0=100)
    assert torch.equal(out[:, 0].cpu(), torch.zeros(2))
    half = torch.zeros_like(mask)
    half[:, :, :, 150:] = 1.0
    wild = pred.clone()
    wild[:, :, :, :150] = 1e3                                  # only under mask 0
    a, _ = ops.eval_metrics(d(pred), d(origin), d(half), x0=100)
    b, _ = ops.eval_metrics(d(wild), d(origin), d(half), x0=100)
    assert torch.equal(a, b)
    # planted NaN / inf in the scored columns are counted exactly, per sample; those left of x0 are not read
    bad = pred.clone()
    bad[0, 0, 3, 120] = float("nan")
    bad[0, 2, 95, 199] = float("inf")
    bad[1, 1, 0, 100] = float("-inf")
    bad[1, 1, 50, 99] = float("nan")
    out, _ = ops.eval_metrics(d(bad.half()), d(origin), d(mask), x0=100)
    assert out[:, 3].tolist() == [2.0, 1.0]
    # uint8 image: bit-equal to the torch expression on the fp32 composite
    for dtype in (torch.float32, torch.float16):
        p = (pred * 1.3).to(dtype)                             # some values beyond [-1, 1]: the clamp matters
        soft = mask * 0.75                                     # a non-binary mask: the composite rounds
        _, rgb = ops.eval_metrics(d(p), d(origin), d(soft), x0=100, want_rgb8=True)
        comp = (d(p).float() * d(soft) + d(origin) * (1 - d(soft)))[:, :, :, 100:]
        want = ((comp.clamp(-1, 1) + 1) / 2 * 255).to(torch.uint8).permute(0, 2, 3, 1)
        assert rgb.dtype == torch.uint8 and rgb.shape == (2, 96, 100, 3)
        assert torch.equal(rgb, want)
    # down-sampled: the same expression on F.interpolate(mode='area') of the composite (a power-of-two mean is exact in any order)
    _, rgb = ops.eval_metrics(d(pred), d(origin), d(mask), x0=100, r=2, want_rgb8=True)
    comp = F.interpolate((d(pred) * d(mask) + d(origin) * (1 - d(mask)))[:, :, :, 100:], size=(48, 50), mode="area")
    want = ((comp.clamp(-1, 1) + 1) / 2 * 255).to(torch.uint8).permute(0, 2, 3, 1)
    assert rgb.shape == (2, 48, 50, 3)
    assert (rgb.int() - want.int()).abs().max() <= 1           # the order of the four fp32 additions may differ by one rounding
    # argument errors are errors, not silence
    with pytest.raises(ValueError):
        ops.eval_metrics(d(pred), d(origin), d(mask), x0=100, r=3)
    with pytest.raises(RuntimeError, match="bad argument"):
        ops.eval_metrics(d(pred[:, :, :6]), d(origin[:, :, :6]), None)      # no 7 x 7 window fits


def test_determinism_and_graph_capture():
    """Item 7: two launches agree bit for bit; the call captures into a graph and the replay equals eager."""
    from leftrefill_amd import ops
    pred, origin = _family("noise", 4, 512, 1024, seed=9)
    mask = _block_mask(4, 512, 1024, seed=9)
    p, o, m = pred.half().to(DEV), origin.to(DEV), mask.to(DEV)
    a, rgb_a = ops.eval_metrics(p, o, m, x0=512, want_rgb8=True)
    b, rgb_b = ops.eval_metrics(p, o, m, x0=512, want_rgb8=True)
    assert torch.equal(a, b) and torch.equal(rgb_a, rgb_b)
    torch.cuda.synchronize()
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        ops.eval_metrics(p, o, m, x0=512, want_rgb8=True)      # warm-up on the side stream
    torch.cuda.current_stream().wait_stream(s)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        c, rgb_c = ops.eval_metrics(p, o, m, x0=512, want_rgb8=True)
    c.zero_()
    g.replay()
    torch.cuda.synchronize()
    assert torch.equal(a, c) and torch.equal(rgb_a, rgb_c)


# ---- item 8: end to end on the tiny model of tests/test_gpu_harness.py (helper copied from there) ------------------------------
def _write_config(path, size):
    import yaml
    cfg = G.CONFIGS["MID"]
    dd = dict(double_z=True, z_channels=4, resolution=size, in_channels=3, out_ch=3, ch=64, ch_mult=[1, 2, 4, 4],
              num_res_blocks=1, attn_resolutions=[], dropout=0.0)
    model = {"target": "inpainting_ldm.ref_inpainting_ldm.RefInpaintLDM", "params": dict(
        linear_start=0.00085, linear_end=0.0120, timesteps=1000, first_stage_key="image", cond_stage_key="txt", channels=4,
        cond_stage_trainable=True, conditioning_key="hybrid", scale_factor=0.18215,
        data_config={"img_size": size, "repeat_sp_token": 4, "sp_token": "<special-token>", "cfg": 2.5},
        unet_config={"target": "ldm.modules.diffusionmodules.openaimodel.UNetModel", "params": cfg.kwargs()},
        first_stage_config={"target": "ldm.models.autoencoder.AutoencoderKL",
                            "params": {"ddconfig": dd, "embed_dim": 4, "lossconfig": {"target": "torch.nn.Identity"}}},
        cond_stage_config={"target": "ldm.modules.encoders.Refill_modules.PromptCLIPEmbedder",
                           "params": dict(freeze=True, layer="penultimate", special_tokens=["repeat_4_<special-token>"],
                                          init_text=["reference on the left target on the right"])})}
    with open(path, "w") as f:
        yaml.safe_dump({"model": model}, f)


VALIDATION_DRIVER = '''
import glob, json, os, sys
import torch
sys.path.insert(0, os.path.join({root!r}, "tools"))
import run_inpainting as R
import leftrefill_amd.dropin as dropin
dropin.install()
from inpainting_ldm.model import create_model, load_state_dict
mdir = {mdir!r}
model = create_model(os.path.join(mdir, "model_config.yaml")).cpu()
model.load_state_dict(load_state_dict(glob.glob(os.path.join(mdir, "ckpts", "epoch=*.ckpt"))[0]), strict=False)
model = model.to("cuda").eval()
batch = next(iter(R.synthetic_batches(1, 2, {size})))
batch = {{k: (v.cuda() if torch.is_tensor(v) else v) for k, v in batch.items()}}
with torch.no_grad(), torch.autocast("cuda"):
    res = model.validation_step(batch, 0)
print("VALIDATION " + json.dumps(res))
print("EPOCH " + json.dumps(model.validation_epoch_end([res, res])))
'''


def test_script_device_route_and_validation_step_end_to_end(tmp_path):
    """tools/run_inpainting.py --synthetic 1 with and without --device_metrics in fresh child processes (same default seed): the PSNR /
    SSIM lines agree within the caps of item 5 plus the rounding of the printed digits, the PNG files are byte-identical; validation_step
    on that model (data_cfg['cfg'] = 2.5, eta 0, 50 steps: log_images' defaults) returns the script's per-batch means."""
    size = 64
    mdir = tmp_path / "synthetic_model"
    (mdir / "ckpts").mkdir(parents=True)
    _write_config(str(mdir / "model_config.yaml"), size)
    stub = tmp_path / "stubs"
    stub.mkdir()
    (stub / "open_clip.py").write_text("from oracle.clip_stub import *  # noqa: F401,F403  (test stand-in for the absent package)\n")
    import leftrefill_amd.dropin as dropin
    dropin.install()
    sys.path.insert(0, str(stub))
    try:
        from inpainting_ldm.model import create_model
        model = create_model(str(mdir / "model_config.yaml"))
    finally:
        sys.path.remove(str(stub))
    sd = dict(model.state_dict())
    for k, v in model.state_dict().items():
        if k.startswith("first_stage_model."):
            sd[k] = torch.from_numpy(weights.fill_like("vae2." + k[len("first_stage_model."):], v.shape)).to(v.dtype)
    for k, v in G.unet_state("MID").items():
        sd["model.diffusion_model." + k] = v
    torch.save({"state_dict": sd}, str(mdir / "ckpts" / "epoch=3.ckpt"))
    env = dict(os.environ, PYTHONPATH=os.pathsep.join([str(stub), ROOT, os.environ.get("PYTHONPATH", "")]))
    runs = {}
    for route in ("host", "device"):
        out_dir, met_dir = tmp_path / ("out_" + route), tmp_path / ("metrics_" + route)
        cmd = [sys.executable, os.path.join(ROOT, "tools", "run_inpainting.py"), "--model_path", str(mdir), "--synthetic", "1",
               "--test_size", str(size), "--metric_size", str(size), "--batch_size", "2", "--cfg", "2.5", "--eta", "0.0",
               "--output_path", str(out_dir), "--metric_output", str(met_dir)] + (["--device_metrics"] if route == "device" else [])
        r = subprocess.run(cmd, capture_output=True, text=True, cwd=str(tmp_path), env=env, timeout=900)
        assert r.returncode == 0, r.stdout[-1500:] + r.stderr[-3000:]
        assert "WARNING" not in r.stdout, r.stdout[-1500:]
        lines = {ln.split(":")[0]: ln for ln in r.stdout.splitlines() if ln.startswith(("PSNR:", "SSIM:", "LPIPS:"))}
        assert "over 2 images" in lines["PSNR"] and lines["LPIPS"].startswith("LPIPS: not computed")
        pngs = {f: (out_dir / f).read_bytes() for f in sorted(os.listdir(str(out_dir)))}
        runs[route] = dict(psnr=float(lines["PSNR"].split()[1]), ssim=float(lines["SSIM"].split()[1]), pngs=pngs,
                           metric=(met_dir / "synthetic_model.txt").read_text())
        print(route, lines["PSNR"], lines["SSIM"])
    assert sorted(runs["host"]["pngs"]) == sorted(runs["device"]["pngs"]) == ["0000_0.png", "0000_1.png"]
    assert runs["host"]["pngs"] == runs["device"]["pngs"]                       # byte-identical files
    assert abs(runs["host"]["psnr"] - runs["device"]["psnr"]) <= PSNR_CAP + 1e-3      # + one unit of the last printed digit
    assert abs(runs["host"]["ssim"] - runs["device"]["ssim"]) <= SSIM_CAP + 1e-4
    assert runs["host"]["metric"].split("\n")[2] == runs["device"]["metric"].split("\n")[2]
    driver = tmp_path / "validation_driver.py"
    driver.write_text(VALIDATION_DRIVER.format(root=ROOT, mdir=str(mdir), size=size))
    r = subprocess.run([sys.executable, str(driver)], capture_output=True, text=True, cwd=str(tmp_path), env=env, timeout=900)
    assert r.returncode == 0, r.stdout[-1500:] + r.stderr[-3000:]
    res = json.loads([ln for ln in r.stdout.splitlines() if ln.startswith("VALIDATION ")][0][len("VALIDATION "):])
    print("validation_step", res)
    assert set(res) == {"psnr", "ssim"}                                          # no loss_fn_alex: no 'lpips'
    assert abs(res["psnr"] - runs["device"]["psnr"]) <= 5e-4 + PSNR_CAP          # the script prints 3 / 4 decimals
    assert abs(res["ssim"] - runs["device"]["ssim"]) <= 5e-5 + SSIM_CAP
    epoch = json.loads([ln for ln in r.stdout.splitlines() if ln.startswith("EPOCH ")][0][len("EPOCH "):])
    assert epoch == res
