"""GPU: the one-call inpainting route (leftrefill_amd/refill.py) -- lr_pil_resize against Pillow byte for byte, lr_refill_canvas and the
lr_eval_metrics tail against the numpy statement bit for bit, the refusals, `refill(...)` on both routes and tools/refill.py, on the
synthetic model of tests/test_gpu_harness.py (config and state-dict helpers restated here; oracle/clip_stub.py stands in for open_clip)."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch
from PIL import Image

pytestmark = pytest.mark.gpu

from oracle import golden_spec as G, weights  # noqa: E402
from leftrefill_amd import refill as R  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
# (h, w) -> (H, W): enlarging, shrinking, one axis equal (a skipped pass), identity (the copy), a tiny source, both axes mixed
CASES = [((37, 53), (64, 64)), ((96, 70), (64, 64)), ((64, 64), (91, 64)), ((64, 64), (33, 64)), ((200, 300), (64, 64)),
         ((64, 64), (64, 64)), ((5, 7), (64, 64)), ((301, 199), (128, 128)), ((64, 128), (512, 200)), ((64, 64), (64, 40))]


def _pil(a, wh, f):
    a = a[:, :, 0] if a.shape[2] == 1 else a
    out = np.asarray(Image.fromarray(a).resize(wh, resample=getattr(Image.Resampling, f.upper())))
    return out.reshape(wh[1], wh[0], -1)


def test_pil_resize_mixed_batch_equals_pil():
    rng = np.random.RandomState(0)
    sources, sizes, filters = [], [], []
    for i, ((h, w), (H, W)) in enumerate(CASES):
        for f in ("bicubic", "bilinear"):
            c = 3 if (i + len(sources)) % 2 == 0 else 1      # channel counts alternate, so odd byte offsets follow
            a = rng.randint(0, 256, (h, w, c), dtype=np.uint8)
            if i % 3 == 0:
                a[::2, ::2] = 0
                a[1::2, 1::2] = 255      # hard edges: the bicubic overshoot meets both clamps
            sources.append(a)
            sizes.append((W, H))
            filters.append(f)
    table = R.ResizeTable()
    for a, wh, f in zip(sources, sizes, filters):
        table.add(0, a.shape, wh, f)
    jobs = table.arrays()[1]
    h, v = jobs["h_ksize"] > 0, jobs["v_ksize"] > 0
    assert (h & v).any() and (~h & v).any() and (h & ~v).any() and (~h & ~v).any()      # both passes, either skipped, the copy
    outs = R.device_resize(sources, sizes, filters, torch.device("cuda"))
    torch.cuda.synchronize()
    for a, wh, f, o in zip(sources, sizes, filters, outs):
        want = _pil(a, wh, f)
        got = o.cpu().numpy()
        assert got.shape == want.shape and np.array_equal(got, want), (a.shape, wh, f, int(np.abs(got.astype(int) - want).max()))


def test_pil_resize_takes_device_sources():
    a = np.random.RandomState(1).randint(0, 256, (3, 128, 128, 3), dtype=np.uint8)
    sizes = [(46, 64), (153, 64), (128, 128)]
    outs = R.device_resize(torch.from_numpy(a).cuda(), sizes, ["bicubic"] * 3, torch.device("cuda"))
    for img, wh, o in zip(a, sizes, outs):
        assert np.array_equal(o.cpu().numpy(), _pil(img, wh, "bicubic"))


def test_a_refused_job_is_resized_on_the_host_and_copied():
    rng = np.random.RandomState(3)
    sources = [rng.randint(0, 256, (16500, 2, 3), dtype=np.uint8), rng.randint(0, 256, (37, 53, 3), dtype=np.uint8)]
    sizes = [(2, 64), (64, 64)]
    assert R.refused(sources[0].shape, sizes[0], "bicubic") and not R.refused(sources[1].shape, sizes[1], "bicubic")
    outs = R.device_resize(sources, sizes, ["bicubic"] * 2, torch.device("cuda"))
    for a, wh, o in zip(sources, sizes, outs):
        assert np.array_equal(o.cpu().numpy(), _pil(a, wh, "bicubic"))


def _pair(hs, ws, hr, wr, seed):
    rng = np.random.RandomState(seed)
    source = rng.randint(0, 256, (hs, ws, 3), dtype=np.uint8)
    reference = rng.randint(0, 256, (hr, wr, 3), dtype=np.uint8)
    mask = np.zeros((hs, ws, 3), np.uint8)
    mask[hs // 4:hs // 2, ws // 5:ws // 2] = 255      # strokes
    mask[hs // 2:hs // 2 + 3, :] = 255
    mask[hs - 5, ws - 7] = (0, 0, 200)                # a coloured pixel: every channel > 0 -> 255 first, then a luma below 128
    mask[3, 4] = (0, 90, 0)
    return source, mask, reference


@pytest.mark.parametrize("size", [64, 128], ids=["size64_pads_to_128", "size128_no_pad"])
def test_prepare_equals_prepare_numpy(size):
    pairs = [_pair(96, 70, 50, 120, 1), _pair(50, 120, 96, 70, 2)]      # P = 2 pairs of different source sizes
    n = 2
    got = R.prepare_device([p[0] for p in pairs], [p[1] for p in pairs], [p[2] for p in pairs], size, n, torch.device("cuda"))
    want = [R.prepare_numpy(s, m, r, size, n) for s, m, r in pairs]
    H = 128
    for k, name in enumerate(("image", "masked_image", "mask")):
        w = np.concatenate([p[k] for p in want], axis=0)
        g = got[k].cpu().numpy()
        assert g.shape == w.shape == (2 * n, 1 if k == 2 else 3, H, 2 * H) and g.dtype == np.float32
        assert np.array_equal(g.view(np.uint32), w.view(np.uint32)), name      # bit for bit
    m = got[2].cpu().numpy()
    assert not m[:, :, :, :H].any() and 0 < m[:, :, :, H:].mean() < 1
    # one pair alone gives the same canvases
    one = R.prepare_device([pairs[1][0]], [pairs[1][1]], [pairs[1][2]], size, n, torch.device("cuda"))
    assert all(torch.equal(one[k], got[k][n:]) for k in range(3))


def _raw_call(lib, args, **over):
    src, tables, tables_host, jobs, jobs_host, n_jobs, work, dst = args
    a = dict(src=src.data_ptr(), src_bytes=src.numel(), tables=tables.data_ptr(), tables_host=tables_host.data_ptr(),
             words=tables.numel(), work=work.data_ptr(), work_bytes=work.numel(), dst=dst.data_ptr(), dst_bytes=dst.numel(),
             jobs=jobs.data_ptr(), jobs_host=jobs_host.data_ptr(), n_jobs=n_jobs)
    a.update(over)
    return lib.lr_pil_resize(a["src"], a["src_bytes"], a["tables"], a["tables_host"], a["words"], a["work"], a["work_bytes"], a["dst"],
                             a["dst_bytes"], a["jobs"], a["jobs_host"], a["n_jobs"], torch.cuda.current_stream().cuda_stream)


def _packed(sources, sizes, filters):
    from leftrefill_amd import rawbatch
    arena, table = rawbatch.Arena(1), R.ResizeTable()
    for a, wh, f in zip(sources, sizes, filters):
        table.add(arena.add(a), a.shape, wh, f)
    tables, jobs = table.arrays()
    tables_host, jobs_host = torch.from_numpy(tables), rawbatch.table_tensor(jobs, False)
    src = arena.tensor(False).cuda()
    work = torch.empty(max(16, table.work_bytes), dtype=torch.uint8, device="cuda")
    dst = torch.full((max(16, table.dst_bytes),), 0xAB, dtype=torch.uint8, device="cuda")
    return src, tables_host.cuda(), tables_host, jobs_host.cuda(), jobs_host, len(jobs), work, dst


def test_refusals_come_before_any_launch():
    from leftrefill_amd import _lib
    lib = _lib.load()
    rng = np.random.RandomState(2)
    good = [rng.randint(0, 256, (96, 70, 3), dtype=np.uint8), rng.randint(0, 256, (40, 40, 1), dtype=np.uint8)]
    sizes, filters = [(64, 64), (40, 40)], ["bicubic", "bilinear"]

    def untouched(dst):
        torch.cuda.synchronize()
        return bool((dst == 0xAB).all())

    # a job over the ksize cap (16500 -> 64 under bicubic: ksize 1033 > 1025), after a job that is fine
    long = rng.randint(0, 256, (16500, 1, 1), dtype=np.uint8)
    args = _packed(good + [long], sizes + [(1, 64)], filters + ["bicubic"])
    assert args[4].numpy().view(R.JOB_DTYPE)["v_ksize"][2] == 1033
    assert _raw_call(lib, args) == -3 and untouched(args[-1])
    args = _packed(good, sizes, filters)
    assert _raw_call(lib, args, work=0) == -1 and untouched(args[-1])                                           # a null pointer
    assert _raw_call(lib, args, src=args[0].data_ptr() + 1, src_bytes=args[0].numel() - 1) == -2 and untouched(args[-1])   # misaligned arena
    assert _raw_call(lib, args, src_bytes=96 * 70 * 3 + 40 * 40 - 1) == -1 and untouched(args[-1])              # a window past the arena
    assert _raw_call(lib, args, dst_bytes=64 * 64 * 3 + 40 * 40 - 1) == -1 and untouched(args[-1])
    assert _raw_call(lib, args, n_jobs=0) == -1 and _raw_call(lib, args, n_jobs=65536) == -1 and untouched(args[-1])
    bad_rows = args[2].clone()
    bad_rows[int(args[4].numpy().view(R.JOB_DTYPE)["h_off"][0])] = 70      # lo[0] + cnt[0] > n_in, in the host copy the check reads
    assert _raw_call(lib, args, tables_host=bad_rows.data_ptr()) == -1 and untouched(args[-1])
    # the same arguments untouched are served
    assert _raw_call(lib, args) == 0
    torch.cuda.synchronize()
    dst = args[-1].cpu().numpy()
    assert np.array_equal(dst[:64 * 64 * 3].reshape(64, 64, 3), _pil(good[0], (64, 64), "bicubic"))
    assert np.array_equal(dst[64 * 64 * 3:64 * 64 * 3 + 1600].reshape(40, 40, 1), good[1])


def test_refill_canvas_refuses_bad_sizes():
    from leftrefill_amd import _lib
    lib = _lib.load()
    u = torch.zeros(1, 64, 64, 3, dtype=torch.uint8, device="cuda")
    f = torch.full((1, 3, 128, 256), 7.0, device="cuda")
    m = torch.full((1, 1, 128, 256), 7.0, device="cuda")
    st = torch.cuda.current_stream().cuda_stream
    assert lib.lr_refill_canvas(u.data_ptr(), u.data_ptr(), u.data_ptr(), 1, 64, 64, 32, 128, 1, f.data_ptr(), f.data_ptr(), m.data_ptr(), st) == -1
    assert lib.lr_refill_canvas(u.data_ptr(), u.data_ptr(), 0, 1, 64, 64, 128, 128, 1, f.data_ptr(), f.data_ptr(), m.data_ptr(), st) == -1
    assert lib.lr_refill_canvas(u.data_ptr(), u.data_ptr(), u.data_ptr(), 0, 64, 64, 128, 128, 1, f.data_ptr(), f.data_ptr(), m.data_ptr(), st) == -1
    torch.cuda.synchronize()
    assert bool((f == 7.0).all()) and bool((m == 7.0).all())


@pytest.mark.parametrize("dtype", [torch.float16, torch.float32], ids=["fp16", "fp32"])
def test_finish_equals_finish_numpy(dtype):
    rng = np.random.RandomState(4)
    H = W = 128
    pairs = [_pair(96, 70, 50, 120, 1), _pair(50, 120, 96, 70, 2)]
    image, _, mask = R.prepare_device([p[0] for p in pairs], [p[1] for p in pairs], [p[2] for p in pairs], 64, 1, torch.device("cuda"))
    pred = torch.from_numpy(rng.rand(2, 3, H, 2 * W).astype(np.float32) * 3 - 1.5).cuda().to(dtype)      # values outside [-1, 1]
    out_whs = [R.plan(p[0].shape[:2], 64)["out_wh"] for p in pairs]
    assert out_whs == [(46, 64), (153, 64)]
    got = R.finish_device(pred, image, mask, out_whs)
    for i, wh in enumerate(out_whs):
        want = R.finish_numpy(pred[i:i + 1].float().cpu().numpy(), image[i:i + 1].cpu().numpy(), mask[i:i + 1].cpu().numpy(), wh)[0]
        assert got[i].shape == want.shape == (wh[1], wh[0], 3) and np.array_equal(got[i], want)
        full = R.finish_numpy(pred[i:i + 1].float().cpu().numpy(), image[i:i + 1].cpu().numpy(), mask[i:i + 1].cpu().numpy(), (W, H))[0]
        assert full.min() == 0 and full.max() == 255      # the 8-bit composite, before the resize averages it, meets both clamps


# ---- the synthetic model of tests/test_gpu_harness.py ---------------------------------------------------------------------------------

def _write_config(path, size):
    import yaml
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


@pytest.fixture(scope="module")
def synthetic(tmp_path_factory):
    """(root, model directory, stub directory, the model on the GPU): a config, a checkpoint of deterministic fills under ckpts/epoch=3.ckpt
    and, under root, three PNGs: a 96 x 70 source, its mask, a 50 x 120 reference."""
    root = tmp_path_factory.mktemp("refill")
    mdir, stub = root / "synthetic_model", root / "stubs"
    (mdir / "ckpts").mkdir(parents=True)
    stub.mkdir()
    _write_config(str(mdir / "model_config.yaml"), 64)
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
    model.load_state_dict(sd, strict=False)
    source, mask, reference = _pair(96, 70, 50, 120, 1)
    for name, arr in (("source", source), ("mask", mask), ("reference", reference)):
        Image.fromarray(arr).save(str(root / (name + ".png")))
    return root, mdir, stub, model.to("cuda").eval()


# DDIM's uniform schedule takes a step count that divides the 1000 training timesteps: 3 gives the stride 333 and a fourth timestep 1000,
# past the table, here as in the reference (ldm/modules/diffusionmodules/util.py make_ddim_timesteps).  4 is the smallest count above it.
STEPS = 4


def _bytes(images):
    return [np.asarray(im) for im in images]


def test_refill_end_to_end_routes_agree(synthetic):
    root, _, _, model = synthetic
    source, mask, reference = (Image.open(str(root / (n + ".png"))) for n in ("source", "mask", "reference"))
    kw = dict(steps=STEPS, scale=2.5, num_samples=2, size=64)
    torch.manual_seed(0)
    dev = R.refill(model, source, mask, reference, seed=0, device_prep=True, **kw)
    torch.manual_seed(0)
    host = R.refill(model, source, mask, reference, seed=0, device_prep=False, **kw)
    assert len(dev) == len(host) == 2 and all(im.size == (int(64 / (96 / 70)), 64) == (46, 64) for im in dev + host)
    assert all(np.array_equal(a, b) for a, b in zip(_bytes(dev), _bytes(host)))
    assert not np.array_equal(*_bytes(dev))      # the two samples differ
    torch.manual_seed(0)
    other = R.refill(model, source, mask, reference, seed=1, device_prep=True, **kw)
    assert not np.array_equal(_bytes(other)[0], _bytes(dev)[0])


def test_refill_takes_a_batch_of_pairs(synthetic):
    root, _, _, model = synthetic
    a = _pair(96, 70, 50, 120, 1)
    b = _pair(50, 120, 96, 70, 2)
    torch.manual_seed(0)
    out = R.refill(model, [a[0], b[0]], [a[1], b[1]], [a[2], b[2]], steps=2, seed=[0, 5], num_samples=1, size=64)
    assert [[im.size for im in g] for g in out] == [[(46, 64)], [(153, 64)]]
    with pytest.raises(AssertionError, match="one per pair"):
        R.refill(model, [a[0], b[0]], [a[1], b[1]], [a[2], b[2]], steps=2, seed=[0], size=64)


def test_refill_tool_writes_the_pngs(synthetic, tmp_path):
    root, mdir, stub, _ = synthetic
    env = dict(os.environ, PYTHONPATH=os.pathsep.join([str(stub), ROOT, os.environ.get("PYTHONPATH", "")]))
    outs = {}
    for route, extra in (("device", []), ("host", ["--host_prep"])):
        out = tmp_path / route
        r = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "refill.py"), "--model_path", str(mdir), "--source",
                            str(root / "source.png"), "--mask", str(root / "mask.png"), "--reference", str(root / "reference.png"),
                            "--out", str(out), "--steps", str(STEPS), "--scale", "2.5", "--seed", "0", "--num_samples", "2", "--size", "64"] + extra,
                           capture_output=True, text=True, cwd=str(tmp_path), env=env, timeout=600)
        assert r.returncode == 0, r.stdout[-1500:] + r.stderr[-3000:]
        assert sorted(os.listdir(str(out))) == ["out_00.png", "out_01.png"]
        outs[route] = [np.asarray(Image.open(str(out / f))) for f in sorted(os.listdir(str(out)))]
        assert all(a.shape == (64, 46, 3) for a in outs[route])
    assert all(np.array_equal(a, b) for a, b in zip(outs["device"], outs["host"]))
