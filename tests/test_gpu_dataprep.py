"""lr_batch_prep (csrc/batch_prep.hip) through `dataprep.collate_raw` + `dataprep.DevicePrep` on the MI355X against a float64 numpy
composition written here from `_area_weights` / `resize_area` / `resize_nearest` of dataloaders/test_dataset.py (not the code under
test), and `tools/train_inpainting.py --dataset inpainting --device_prep --val` end to end.

Pass conditions: `mask` bit-equal; `image` bit-equal except where the yardstick's float64 value before rounding lies within 1e-6 of a
half-integer, where it may differ by one uint8 level; `masked_image` bit-equal to image * (mask < 0.5) of the kernel's own outputs.
The kernel's coverage weights are the yardstick's expressions; only the order of the sums differs (~1e-13 of a level), so away from
a tie both round alike.  Inputs are seeded and, for the integer ratios where an average of 6 pixels ties once in 6, nudged by one
level until the yardstick has no tie at all (`_detie`); every case asserts that the yardstick's ties stay below 1 % of its outputs."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import leftrefill_amd.dropin as dropin

dropin.install()
from dataloaders.test_dataset import _area_weights, resize_nearest  # noqa: E402
from leftrefill_amd import dataprep  # noqa: E402

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
S = 8
TIE = 1e-6


# ---- the yardstick ------------------------------------------------------------------------------------------------------------------
def _area_f64(img, rh, rw):
    """resize_area before its rounding, for a rectangular target: rows first, then columns, normalised coverage weights.  optimize=True
    hands the two contractions to BLAS (0.5 s in place of 6.5 s at 1203 x 1601): the same operands, another order of the sums, which moves
    a value by ~1e-13 of a level -- far inside the tie window."""
    h, w = img.shape[:2]
    if (h, w) == (rh, rw):
        return img.astype(np.float64)
    out = np.einsum("ih,hwc->iwc", _area_weights(h, rh), img.astype(np.float64), optimize=True)
    return np.einsum("jw,iwc->ijc", _area_weights(w, rw), out, optimize=True)


def _yard_tile(tile, raw, size):
    """(float64 window before rounding [S, S, 3], mask {0, 1} float32 [S, S, 1])."""
    pre = _area_f64(raw[tile["image"]], tile["rh"], tile["rw"])[tile["y0"]:tile["y0"] + size, tile["x0"]:tile["x0"] + size]
    if tile["outpaint_col"] >= 0:
        mask = np.zeros((size, size), np.float32)
        mask[:, tile["outpaint_col"]:] = 1
    elif tile["zero_mask"]:
        mask = np.zeros((size, size), np.float32)
    else:
        total = sum(resize_nearest(raw[m], size).astype(np.int64) for m in tile["masks"])
        mask = (np.clip(total, 0, 255) > 127).astype(np.float32)
    if tile["flip"]:
        pre = pre[:, ::-1]
    if tile["mask_flip"]:
        mask = mask[:, ::-1]
    return pre, mask[:, :, None]


def _yard(plan, raw):
    tiles = [_yard_tile(t, raw, plan["img_size"]) for t in plan["tiles"]]
    return np.concatenate([t[0] for t in tiles], axis=1), np.concatenate([t[1] for t in tiles], axis=1)


def _near_tie(pre):
    return np.abs(pre - np.floor(pre) - 0.5) <= TIE


def _detie(img, *targets):
    """Flip the low bit of one source pixel under every output that ties at one of the target sizes (rh, rw), until none does at any
    (deterministic)."""
    img = img.copy()
    h, w = img.shape[:2]
    for _ in range(20):
        clean = True
        for rh, rw in targets:
            for i, j, c in np.argwhere(_near_tie(_area_f64(img, rh, rw))):
                img[int(i * h / rh), int(j * w / rw), c] ^= 1
                clean = False
        if clean:
            return img
    raise AssertionError("ties left")


def _check(got, plan, raw, what=""):
    """One sample of the device batch (dict of CPU tensors [S, T S, .]) against the yardstick."""
    pre, mask = _yard(plan, raw)
    ties = _near_tie(pre)
    assert ties.mean() < 0.01, (what, "the yardstick itself ties in", ties.mean())
    ref8 = np.clip(np.rint(pre), 0, 255)
    ref = ref8.astype(np.uint8).astype(np.float32) / 127.5 - 1.0
    image, gmask, masked = got["image"].numpy(), got["mask"].numpy(), got["masked_image"].numpy()
    assert image.dtype == np.float32 and image.shape == ref.shape and gmask.shape == mask.shape
    assert np.array_equal(gmask, mask), (what, "mask", int((gmask != mask).sum()))
    differ = image != ref
    print(f"{what}: {int(differ.sum())} of {differ.size} image values differ, {int(ties.sum())} yardstick ties")
    assert not (differ & ~ties).any(), (what, "differs away from a tie", np.argwhere(differ & ~ties)[:4], image[differ & ~ties][:4], ref[differ & ~ties][:4])
    got8 = np.rint((image.astype(np.float64) + 1.0) * 127.5)
    assert (np.abs(got8 - ref8)[differ] == 1).all(), (what, "more than one level at a tie")
    assert masked.tobytes() == (image * (gmask < 0.5)).tobytes(), (what, "masked_image")


def _run(items, prep=None, tiles=1, size=S):
    prep = prep or dataprep.DevicePrep(size, tiles, "cuda:0")
    batch = dataprep.collate_raw(items)
    out = prep(batch)
    torch.cuda.synchronize()
    return {k: (v.cpu() if torch.is_tensor(v) else v) for k, v in out.items()}, batch


def _sample(out, b):
    return {k: out[k][b] for k in ("image", "mask", "masked_image")}


# ---- the cases at S = 8 -----------------------------------------------------------------------------------------------------------------
def _cases():
    rng = np.random.RandomState(20)
    u8 = lambda *shape: rng.randint(0, 256, shape, dtype=np.uint8)
    images = {      # name -> (source, resize / crop decisions)
        "identity_8x8": (u8(8, 8, 3), dict(rh=8, rw=8)),
        "integer_16x24": (_detie(u8(16, 24, 3), (8, 8)), dict(rh=8, rw=8)),
        "fractional_19x23": (u8(19, 23, 3), dict(rh=8, rw=8)),
        "crop_11x29_at_0": (u8(11, 29, 3), dict(rh=8, rw=21, x0=0)),       # long side int(29 * (8 / 11)) = 21
        "crop_11x29_at_13": (u8(11, 29, 3), dict(rh=8, rw=21, x0=13)),
        "crop_29x11_at_5": (u8(29, 11, 3), dict(rh=21, rw=8, y0=5)),
        "crop_29x11_at_13": (u8(29, 11, 3), dict(rh=21, rw=8, y0=13)),
    }
    edge = np.array([0, 127, 128, 255], dtype=np.uint8)
    m127 = rng.choice(np.array([127, 128], dtype=np.uint8), size=(8, 8))
    masks = {       # name -> (mask sources, outpainting column)
        "nearest_enlarging_5x7": ([rng.choice(edge, size=(5, 7))], -1),
        "nearest_shrinking_40x33": ([rng.choice(edge, size=(40, 33))], -1),
        "threshold_127_128": ([m127], -1),
        "sum_clipped": ([rng.choice(np.array([0, 100, 127, 200, 255], dtype=np.uint8), size=(12, 9)),
                         rng.choice(np.array([0, 1, 28, 100, 255], dtype=np.uint8), size=(7, 10))], -1),
        "outpaint_2": ([], 2),
        "outpaint_6": ([], 6),
    }
    cases = {}
    for ii, (iname, (img, where)) in enumerate(images.items()):
        for mi, (mname, (sources, col)) in enumerate(masks.items()):
            flip, mask_flip = bool((ii + mi) & 1), bool((ii + mi) & 2)      # every image and every mask kind meets all four combinations
            raw = [img] + sources
            tile = dataprep.plan_tile(0, flip=flip, masks=range(1, len(raw)), mask_flip=mask_flip, outpaint_col=col, **where)
            cases[f"{iname}-{mname}-flip{int(flip)}{int(mask_flip)}"] = (dict(img_size=S, tiles=[tile], txt="p"), raw)
    return cases


CASES = _cases()


@pytest.fixture(scope="module")
def device_cases():
    """Every S = 8 case as one batch: one arena (odd sizes, unaligned offsets), one launch."""
    out, batch = _run(list(CASES.values()))
    return out, batch


def test_case_table_covers_the_flip_combinations():
    """Image flip on and off, the mask flip independent of it: under every image case and every mask kind."""
    for part in (0, 1):
        for kind in {name.split("-")[part] for name in CASES}:
            assert {name[-2:] for name in CASES if name.split("-")[part] == kind} == {"00", "01", "10", "11"}, kind


@pytest.mark.parametrize("name", sorted(CASES))
def test_image_and_mask_cases(device_cases, name):
    out, batch = device_cases
    b = list(CASES).index(name)
    assert not batch["host"] and out["txt"] == ["p"] * len(CASES)
    _check(_sample(out, b), *CASES[name], what=name)


def test_the_sum_of_two_masks_clips_and_the_threshold_sits_between_127_and_128(device_cases):
    out, _ = device_cases
    name = next(n for n in CASES if n.startswith("identity_8x8-threshold_127_128"))
    plan, raw = CASES[name]
    m = (raw[1] == 128).astype(np.float32)
    m = m[:, ::-1] if plan["tiles"][0]["mask_flip"] else m
    assert np.array_equal(out["mask"][list(CASES).index(name)].numpy()[:, :, 0], m) and 0 < m.sum() < 64
    name = next(n for n in CASES if n.startswith("identity_8x8-sum_clipped"))
    plan, raw = CASES[name]
    a, b = resize_nearest(raw[1], S).astype(int), resize_nearest(raw[2], S).astype(int)
    total = a + b
    assert (total > 255).any() and ((total > 127) & (a <= 127) & (b <= 127)).any()      # the fixture needs the clip and the sum
    m = (total > 127).astype(np.float32)
    m = m[:, ::-1] if plan["tiles"][0]["mask_flip"] else m
    assert np.array_equal(out["mask"][list(CASES).index(name)].numpy()[:, :, 0], m)


def test_three_sources_of_odd_sizes_share_one_arena():
    rng = np.random.RandomState(7)
    items = []
    for h, w, mh, mw in ((19, 23, 5, 7), (9, 13, 11, 3), (17, 8, 9, 9)):
        raw = [rng.randint(0, 256, (h, w, 3), dtype=np.uint8), rng.choice(np.array([0, 255], dtype=np.uint8), size=(mh, mw))]
        items.append((dict(img_size=S, tiles=[dataprep.plan_tile(0, S, S, masks=[1])], txt="t"), raw))
    out, batch = _run(items)
    jobs = dataprep.job_table(batch)
    assert [int(j["img_off"]) for j in jobs] == [0, 19 * 23 * 3 + 35, 19 * 23 * 3 + 35 + 9 * 13 * 3 + 33]
    assert {int(j["img_off"]) % 16 for j in jobs} != {0} and {int(j["mask_off"][0]) % 4 for j in jobs} != {0}
    for b, (plan, raw) in enumerate(items):
        _check(_sample(out, b), plan, raw, what=f"arena sample {b}")


def test_two_tile_canvas_with_the_zero_left_mask():
    rng = np.random.RandomState(9)
    items = []
    for (h, w), (h2, w2) in (((19, 23), (16, 24)), ((8, 8), (21, 9))):
        raw = [rng.randint(0, 256, (h, w, 3), dtype=np.uint8), _detie(rng.randint(0, 256, (h2, w2, 3), dtype=np.uint8), (S, S)),
               rng.choice(np.array([0, 255], dtype=np.uint8), size=(13, 10))]
        tiles = [dataprep.plan_tile(0, S, S, zero_mask=True), dataprep.plan_tile(1, S, S, masks=[2])]
        items.append((dict(img_size=S, tiles=tiles, txt="t"), raw))
    out, _ = _run(items, tiles=2)
    assert out["image"].shape == (2, S, 2 * S, 3) and out["mask"].shape == (2, S, 2 * S, 1)
    for b, (plan, raw) in enumerate(items):
        _check(_sample(out, b), plan, raw, what=f"canvas {b}")
        assert not out["mask"][b, :, :S].any() and out["mask"][b, :, S:].any()
        host = dataprep.run_plan_numpy(plan, raw)      # the host route gives the same canvas (no ties in these inputs)
        assert np.array_equal(host["mask"], out["mask"][b].numpy())


def test_photo_sized_source_many_blocks_and_bands():
    rng = np.random.RandomState(11)
    size = 512
    img = rng.randint(0, 256, (1203, 1601, 3), dtype=np.uint8)
    raw = [img, (rng.rand(300, 411) < 0.5).astype(np.uint8) * 255]
    plan = dict(img_size=size, tiles=[dataprep.plan_tile(0, size, size, flip=True, masks=[1])], txt="t")
    out, _ = _run([(plan, raw)], size=size)
    _check(_sample(out, 0), plan, raw, what="1203x1601 -> 512")
    # and the crop branch of the same source: short side to 512, long side int(1601 * (512 / 1203)) = 681, window at column 100
    plan = dict(img_size=size, tiles=[dataprep.plan_tile(0, size, 681, x0=100, masks=[1], mask_flip=True)], txt="t")
    out, _ = _run([(plan, raw)], size=size)
    _check(_sample(out, 0), plan, raw, what="1203x1601 -> 512x681, crop at 100")


def test_enlarging_sample_takes_the_host_route_and_buffers_are_reused():
    rng = np.random.RandomState(13)
    mk = lambda h, w: [rng.randint(0, 256, (h, w, 3), dtype=np.uint8), rng.choice(np.array([0, 255], dtype=np.uint8), size=(9, 9))]
    plan = lambda: dict(img_size=S, tiles=[dataprep.plan_tile(0, S, S, masks=[1])], txt="t")
    items = [(plan(), mk(19, 23)), (plan(), mk(6, 20)), (plan(), mk(11, 29))]      # the second is 6 rows high: enlarging
    prep = dataprep.DevicePrep(S, 1, "cuda:0")
    with pytest.warns(UserWarning, match="on the host"):
        out, batch = _run(items, prep)
    assert [h[0] for h in batch["host"]] == [1] and dataprep.job_table(batch)[1]["flags"] == dataprep.HOST
    host = dataprep.run_plan_numpy(*items[1])
    for k in ("image", "mask", "masked_image"):
        assert out[k][1].numpy().tobytes() == host[k].tobytes(), k
    for b in (0, 2):
        _check(_sample(out, b), *items[b], what=f"beside the host sample {b}")
    ptrs = [t.data_ptr() for t in (prep.arena, prep.jobs, prep.image, prep.masked_image, prep.mask)]
    out2, _ = _run(items[2:], prep)      # a smaller batch: nothing is reallocated
    assert ptrs == [t.data_ptr() for t in (prep.arena, prep.jobs, prep.image, prep.masked_image, prep.mask)]
    assert out2["image"].shape[0] == 1
    _check(_sample(out2, 0), *items[2], what="second call")


def test_bad_tables_are_refused_before_the_launch():
    from leftrefill_amd import _lib
    lib = _lib.load()
    rng = np.random.RandomState(1)
    raw = [rng.randint(0, 256, (19, 23, 3), dtype=np.uint8)]
    item = (dict(img_size=S, tiles=[dataprep.plan_tile(0, S, S, zero_mask=True)], txt="t"), raw)
    batch = dataprep.collate_raw([item])
    arena, out = batch["arena"].cuda(), torch.zeros(3, S, S, 3, device="cuda:0")
    st = torch.cuda.current_stream().cuda_stream

    def call(mutate):
        table = batch["jobs"].clone()
        mutate(table.numpy().view(dataprep.JOB_DTYPE)[0])
        dev = table.cuda()
        return lib.lr_batch_prep(arena.data_ptr(), arena.numel(), dev.data_ptr(), table.data_ptr(), 1, S, 1, 1, out[0].data_ptr(),
                                 out[1].data_ptr(), out[2].data_ptr(), st)

    def setf(field, value):
        return lambda job: job.__setitem__(field, value)

    assert call(lambda job: None) == 0
    assert call(setf("img_off", arena.numel())) == -1 and call(setf("img_h", 40)) == -1      # past the arena
    assert call(setf("x0", 1)) == -1 and call(setf("sample", 1)) == -1 and call(setf("tile", 1)) == -1
    assert call(setf("rh", 20)) == -3                                                        # enlarging: LR_E_UNSUPPORTED
    assert call(setf("flags", 0)) == -1                                                      # no mask of any kind
    torch.cuda.synchronize()


def test_evaluation_loader_device_route_equals_its_default_batches(tmp_path):
    """tools/run_inpainting.py's `dataset_batches(..., device_prep=True)` -- `dataloaders.raw_pairs` + collate_raw + DevicePrep, two tiles
    per sample -- against the batches of its default route on pair directories with {0, 255} masks and tie-free images."""
    from types import SimpleNamespace
    from PIL import Image
    from tools.run_inpainting import dataset_batches
    rng = np.random.RandomState(23)
    for i, (h, w) in enumerate([(19, 23), (16, 24), (31, 9)]):
        d = tmp_path / f"pair_{i}"
        d.mkdir()
        for stem in ("source", "target"):
            Image.fromarray(_detie(rng.randint(0, 256, (h, w, 3), dtype=np.uint8), (S, S))).save(str(d / f"{stem}.png"))
        m = (rng.rand(h + 3, w + 2) < 0.5).astype(np.uint8) * 255
        Image.fromarray(np.stack([m] * 3, -1)).save(str(d / "mask.png"))
    model = SimpleNamespace(cond_cfg={}, data_cfg={"repeat_sp_token": 2, "sp_token": "<special-token>"})
    host = list(dataset_batches(str(tmp_path), 2, S, model))
    device = [{k: (v.cpu().clone() if torch.is_tensor(v) else v) for k, v in b.items()}
              for b in dataset_batches(str(tmp_path), 2, S, model, device_prep=True)]
    assert len(host) == len(device) == 2 and device[0]["image"].shape == (2, S, 2 * S, 3) and device[1]["image"].shape[0] == 1
    for a, b in zip(host, device):
        assert a["txt"] == b["txt"]
        for k in ("image", "mask", "masked_image"):
            assert a[k].dtype == b[k].dtype and a[k].numpy().tobytes() == b[k].numpy().tobytes(), k


# ---- the training CLI end to end ---------------------------------------------------------------------------------------------------------
def test_train_cli_on_a_folder_of_images_with_device_prep_and_validation(tmp_path):
    """tools/train_inpainting.py --dataset inpainting --device_prep --val on the synthetic tiny model of test_gpu_harness.py and 6 small
    PNGs: 2 steps, a validation with printed metrics, ckpts/last.ckpt; the same command without --device_prep starts from the same
    loss -- bit for bit, since the fixture has no value near a rounding tie (asserted here for both resize branches)."""
    import yaml
    from PIL import Image
    from test_gpu_harness import _write_config
    from oracle import golden_spec as G, weights
    size = 64
    _write_config(str(tmp_path / "model_config.yaml"), size)
    with open(str(tmp_path / "model_config.yaml")) as f:
        cfg = yaml.safe_load(f)
    cfg["model"]["params"]["data_config"]["cfg"] = 2.5
    cfg["model"]["params"]["data_config"]["test_limit"] = 2      # where the reference's model configs keep it
    cfg["model"]["params"]["save_prompt_only"] = True
    with open(str(tmp_path / "model_config.yaml"), "w") as f:
        yaml.safe_dump(cfg, f)
    stub = tmp_path / "stubs"
    stub.mkdir()
    (stub / "open_clip.py").write_text("from oracle.clip_stub import *  # noqa: F401,F403  (test stand-in for the absent package)\n")
    sys.path.insert(0, str(stub))
    try:
        from inpainting_ldm.model import create_model
        model = create_model(str(tmp_path / "model_config.yaml"))
    finally:
        sys.path.remove(str(stub))
    sd = dict(model.state_dict())
    for k, v in model.state_dict().items():
        if k.startswith("first_stage_model."):
            sd[k] = torch.from_numpy(weights.fill_like("vae2." + k[len("first_stage_model."):], v.shape)).to(v.dtype)
    for k, v in G.unet_state("MID").items():
        sd["model.diffusion_model." + k] = v
    torch.save({"state_dict": sd}, str(tmp_path / "backbone.ckpt"))
    rng = np.random.RandomState(17)
    (tmp_path / "images").mkdir()
    (tmp_path / "masks").mkdir()
    names = {"irregular": [], "segment": []}
    for i, (h, w) in enumerate([(97, 131), (131, 97), (150, 101), (83, 140), (120, 120), (99, 177)]):
        long_side = max(size, int(max(h, w) * (size / min(h, w))))
        branches = ((size, size), (size, long_side) if h < w else (long_side, size))
        img = _detie(rng.randint(0, 256, (h, w, 3), dtype=np.uint8), *branches)
        assert not any(_near_tie(_area_f64(img, rh, rw)).any() for rh, rw in branches)
        Image.fromarray(img).save(str(tmp_path / "images" / f"im_{i}.png"))
        m = np.zeros((50 + 7 * i, 61), np.uint8)
        m[5 + 3 * i:35 + 3 * i, 28:58] = 255      # in the right half: validation_step scores columns w // 2 onwards
        Image.fromarray(m).save(str(tmp_path / "masks" / f"m_{i}.png"))
        names["irregular" if i % 2 else "segment"].append(str(tmp_path / "masks" / f"m_{i}.png"))
    for kind, paths in names.items():
        (tmp_path / f"{kind}.txt").write_text("\n".join(paths) + "\n")
    train_cfg = dict(model_config=str(tmp_path / "model_config.yaml"), resume_path=str(tmp_path / "backbone.ckpt"), max_steps=2, batch_size=2,
                     optim_cfg=dict(learning_rate=1e-3, weight_decay=0.01, lr_scheduler="cosine", eta_min=0.01),
                     image_path=str(tmp_path / "images"), train_mask_path=[str(tmp_path / "irregular.txt"), str(tmp_path / "segment.txt")],
                     val_image_path=str(tmp_path / "images"), val_mask_path=str(tmp_path / "masks"), val_batch_size=2,
                     val_check_interval=2)
    with open(str(tmp_path / "training.yaml"), "w") as f:
        yaml.safe_dump(train_cfg, f)
    env = dict(os.environ, PYTHONPATH=os.pathsep.join([str(stub), ROOT, os.environ.get("PYTHONPATH", "")]))
    losses = {}
    for route, extra in (("device", ["--device_prep", "--val"]), ("host", ["--val"])):
        cmd = [sys.executable, os.path.join(ROOT, "tools", "train_inpainting.py"), "--config_file", str(tmp_path / "training.yaml"),
               "--exp_name", route, "--save_path", str(tmp_path / "runs"), "--fp16", "--dataset", "inpainting", "--seed", "3", "--num_workers",
               "2", "--log_every_n_steps", "1", "--loss_file", str(tmp_path / f"{route}.json")] + extra
        r = subprocess.run(cmd, capture_output=True, text=True, cwd=str(tmp_path), env=env, timeout=600)
        assert r.returncode == 0, r.stdout[-1500:] + r.stderr[-3000:]
        print(r.stdout[-600:])
        assert "step 2: loss" in r.stdout and os.path.exists(str(tmp_path / "runs" / route / "ckpts" / "last.ckpt"))
        with open(str(tmp_path / f"{route}.json")) as f:
            losses[route] = json.load(f)
        lines = {ln.split()[0]: float(ln.split()[1]) for ln in r.stdout.splitlines() if ln.startswith(("psnr ", "ssim "))}      # the validation's means
        assert "Steps:" in r.stdout and np.isfinite(lines["psnr"]) and 3.0 < lines["psnr"] < 60.0 and -1.0 <= lines["ssim"] <= 1.0
    assert len(losses["device"]) == len(losses["host"]) == 2 and np.isfinite(losses["device"]).all()
    assert losses["device"][0] == losses["host"][0], losses
