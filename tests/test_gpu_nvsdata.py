"""The Objaverse NVS batches on the MI355X: `collate_nvs_raw` + `NVSDevicePrep` (one lr_nvs_prep launch per batch) against the items the
REFERENCE's dataset returned (tests/golden/nvs_dataset.npz, see test_nvsdata_cpu.py) and against the numpy statement
(nvsprep.run_nvs_plan_numpy) at the smallest shapes where the kernel can go wrong, bit for bit -- the arithmetic is integer up to the
final float mapping, so there is no tolerance anywhere; the entry's refusals; and the training CLI end to end with and without
--device_prep."""
import functools
import json
import os
import sys

import numpy as np
import pytest
import torch

import leftrefill_amd.dropin as dropin

dropin.install()
from leftrefill_amd import _lib, nvsprep  # noqa: E402
from rawdata_helpers import KEYS, device_batch, same_bits as _same_bits  # noqa: E402
from test_nvsdata_cpu import Fixture  # noqa: E402
from tools import make_golden_nvs_dataset as G  # noqa: E402

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
S = G.S
KS = (1, 2, 8, 25, 32)


@pytest.fixture(scope="module")
def fixture(tmp_path_factory):
    return Fixture(tmp_path_factory.mktemp("nvs_tree"))


_device = functools.partial(device_batch, nvsprep.collate_nvs_raw)


@pytest.mark.parametrize("name", sorted(G.SETTINGS))
def test_batches_equal_the_references_items(fixture, name):
    want, _ = fixture.golden(name)
    items, *_ = fixture.run(name, raw=True)
    prep = nvsprep.NVSDevicePrep(S)
    for bs in (1, 5):
        for at in range(0, len(items), bs):
            chunk = items[at:at + bs]
            out = _device(prep, chunk)
            assert out["image"].shape == (len(chunk), S, 2 * S, 3) and out["mask"].shape == (len(chunk), S, 2 * S, 1)
            assert out["rel_pose"].shape == (len(chunk), 4)
            for b in range(len(chunk)):
                _same_bits({k: out[k][b] for k in KEYS}, want[at + b], f"{name}[{at + b}] in batches of {bs}")
                assert np.array_equal(out["rel_pose"][b].numpy(), want[at + b]["rel_pose"])
                assert out["txt"][b] == want[at + b]["txt"] if isinstance(want[at + b]["txt"], str) else \
                    [t[b] for t in out["txt"]] == want[at + b]["txt"]
    ptrs = [t.data_ptr() for t in (prep.arena, prep.jobs, prep.image, prep.masked_image, prep.mask)]
    _device(prep, items[:1])      # a smaller batch: the buffers are reused
    assert ptrs == [t.data_ptr() for t in (prep.arena, prep.jobs, prep.image, prep.masked_image, prep.mask)]


# ---- the kernel against the numpy statement -------------------------------------------------------------------------------------------
def _render(rng, h, w, pattern):
    """An RGBA render of noise (also under alpha 0) whose alpha is set in: single corner pixels, one border line, or a blob."""
    rgba = rng.randint(0, 256, (h, w, 4), dtype=np.uint8)
    alpha = np.zeros((h, w), np.uint8)
    if pattern == "corners":
        alpha[[0, 0, h - 1, h - 1], [0, w - 1, 0, w - 1]] = [1, 255, 7, 128]
    elif pattern == "corner":
        alpha[h - 1, w - 1] = 1
    elif pattern == "top":
        alpha[0, :] = 200
    elif pattern == "bottom":
        alpha[h - 1, :] = 1
    elif pattern == "left":
        alpha[:, 0] = 255
    elif pattern == "right":
        alpha[:, w - 1] = 3
    elif pattern == "blob":
        alpha[h // 3:h // 2, w // 4:w // 2 + 3] = rng.randint(1, 256, (h // 2 - h // 3, w // 2 + 3 - w // 4))
        alpha[h - 3, 2] = 9
    elif pattern == "noise":
        alpha[:] = rng.randint(0, 256, (h, w)) * (rng.rand(h, w) < 0.7)
    rgba[:, :, 3] = alpha
    return rgba


def _plan(size, mode="alpha", k=0, plane=None, ref_white=False):
    return dict(img_size=size, mode=mode, k=k, plane=plane, ref_white=ref_white, rel_pose=[0.1, 0.2, 0.3, 0.4], txt="x")


def _check(items, size, what):
    prep = nvsprep.NVSDevicePrep(size)
    out = _device(prep, items)
    for b, (plan, raw) in enumerate(items):
        _same_bits({k: out[k][b] for k in KEYS}, nvsprep.run_nvs_plan_numpy(plan, raw), f"{what}[{b}] {plan['mode']} k={plan['k']}")


# the 2 x 2 box, the general path with both axes non-integer, the copy, a size that is no multiple of the band of 8 rows (box and
# general), and two sizes whose bit-rows span 64-bit words with a partly filled last word (2 and 3 words)
SHAPES = [(32, 32, 16), (30, 26, 12), (16, 16, 16), (40, 40, 20), (47, 33, 20), (160, 160, 80), (260, 260, 130)]


@pytest.mark.parametrize("h,w,size", SHAPES, ids=[f"{h}x{w}_to_{s}" for h, w, s in SHAPES])
def test_kernel_equals_the_numpy_statement(h, w, size):
    """Every element size with alpha in single corner pixels and along each border, and a blob; the cond render differs in shape class
    from the target where the target is square (a general-path cond beside a box-path target)."""
    rng = np.random.RandomState(h * 1000 + size)
    items = []
    for k in KS:
        for pattern in ("corners", "corner", "top", "bottom", "left", "right", "blob"):
            cond = _render(rng, h + 3, w + 5, "noise") if h == w and pattern in ("corners", "blob") else _render(rng, h, w, "noise")
            items.append((_plan(size, k=k), [cond, _render(rng, h, w, pattern)]))
    _check(items, size, f"{h}x{w}->{size}")


def test_ones_strokes_file_planes_and_the_white_right_half():
    h, w, size = 47, 33, 20
    rng = np.random.RandomState(7)
    strokes = (rng.rand(size, size) < 0.1).astype(np.uint8)
    grey = rng.choice(np.array([0, 1, 126, 127, 128, 129, 254, 255], np.uint8), size=(size, size))
    items = []
    for white in (False, True):
        pair = lambda pattern: [_render(rng, h, w, "noise"), _render(rng, h, w, pattern)]      # noqa: E731
        items.append((_plan(size, "ones", ref_white=white), pair("empty")))                         # the empty-alpha case
        items.append((_plan(size, "alpha", k=5, plane=2, ref_white=white), pair("blob") + [strokes]))
        items.append((_plan(size, "alpha", k=8, plane=2, ref_white=white), pair("empty") + [strokes]))      # strokes alone
        items.append((_plan(size, "alpha", k=8, ref_white=white), pair("noise")))
        items.append((_plan(size, "file", plane=2, ref_white=white), pair("blob") + [grey]))
    _check(items, size, "modes")
    mask = nvsprep.run_nvs_plan_numpy(*items[4])["mask"]
    assert 0 < (mask < 0.5).sum() < mask.size and len(np.unique(mask)) == 8      # the grey levels are not thresholded
    out = _device(nvsprep.NVSDevicePrep(size), [items[4]])
    kept = out["masked_image"][0].numpy()[:, size:][grey == 127]
    assert (out["masked_image"][0].numpy()[:, size:][grey == 128] == 0).all() and (kept != 0).all()


def test_a_smaller_batch_reuses_every_buffer():
    """NVSDevicePrep's side of test_gpu_dataprep.py's buffer test: three samples, one per resize path (32 x 32: the box, 16 x 16: the
    copy, 23 x 19: the bilinear), mode alpha with k = 3 and a stroke plane on one of them; then one sample through the same object."""
    size = 16
    rng = np.random.RandomState(17)
    strokes = (rng.rand(size, size) < 0.1).astype(np.uint8)
    items = [(_plan(size, k=3), [_render(rng, 32, 32, "noise"), _render(rng, 32, 32, "blob")]),
             (_plan(size, k=3, plane=2), [_render(rng, 16, 16, "noise"), _render(rng, 16, 16, "corners"), strokes]),
             (_plan(size, k=3), [_render(rng, 23, 19, "noise"), _render(rng, 23, 19, "blob")])]
    prep = nvsprep.NVSDevicePrep(size)
    buffers = lambda: [getattr(prep, n).data_ptr() for n in ("arena", "jobs", "image", "masked_image", "mask", "rel_pose")]  # noqa: E731
    out = _device(prep, items)
    assert out["image"].shape == (3, size, 2 * size, 3) and out["rel_pose"].shape == (3, 4)
    for b, item in enumerate(items):
        _same_bits({k: out[k][b] for k in KEYS}, nvsprep.run_nvs_plan_numpy(*item), f"first call [{b}]")
    ptrs = buffers()
    out = _device(prep, items[2:])      # a smaller batch: nothing is reallocated
    assert ptrs == buffers()
    assert out["image"].shape[0] == out["rel_pose"].shape[0] == 1
    _same_bits({k: out[k][0] for k in KEYS}, nvsprep.run_nvs_plan_numpy(*items[2]), "second call")


def _raw_call(batch, size, mutate):
    """lr_nvs_prep on a batch whose host AND device table went through `mutate`; (return code, outputs untouched)."""
    lib = _lib.load()
    jobs = nvsprep.job_table(batch).copy()
    mutate(jobs)
    table = torch.from_numpy(jobs.view(np.uint8).reshape(-1).copy())
    arena, table_dev = batch["arena"].cuda(), table.cuda()
    B = batch["batch"]
    outs = [torch.full((B, size, 2 * size, c), -7.0, device="cuda") for c in (3, 3, 1)]
    rc = lib.lr_nvs_prep(arena.data_ptr(), arena.numel(), table_dev.data_ptr(), table.data_ptr(), B, size, outs[0].data_ptr(),
                         outs[1].data_ptr(), outs[2].data_ptr(), torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    return rc, all(bool((o == -7.0).all()) for o in outs)


def test_the_entry_refuses_before_any_launch():
    rng = np.random.RandomState(9)
    size = 16
    items = [(_plan(size, k=8), [_render(rng, 32, 32, "noise"), _render(rng, 32, 32, "blob")]) for _ in range(2)]
    batch = nvsprep.collate_nvs_raw(items)
    assert _raw_call(batch, size, lambda j: None) == (0, False)      # the table as collated is taken
    E_ARG, E_ALIGN, E_UNSUPPORTED = -1, -2, -3

    def set_(field, value, at=1):
        def mutate(jobs):
            jobs[field][at] = value
        return mutate

    assert _raw_call(batch, size, set_("k", 33)) == (E_UNSUPPORTED, True)
    assert _raw_call(batch, size, set_("target_h", size - 1)) == (E_UNSUPPORTED, True)      # an enlarging job
    assert _raw_call(batch, size, set_("cond_w", size - 1, at=0)) == (E_UNSUPPORTED, True)
    assert _raw_call(batch, size, set_("cond_off", int(nvsprep.job_table(batch)["cond_off"][1]) + 4)) == (E_ALIGN, True)
    assert _raw_call(batch, size, set_("plane_off", 8)) == (E_ALIGN, True)
    assert _raw_call(batch, size, set_("k", 0)) == (E_ARG, True)
    assert _raw_call(batch, size, set_("target_h", 10 ** 6)) == (E_ARG, True)      # past the arena
    assert _raw_call(batch, size, set_("sample", 2)) == (E_ARG, True)
    assert _raw_call(batch, size, set_("mode", 2)) == (E_ARG, True)      # a file job without a plane

    def bad_span(jobs):
        jobs["hi"][1][3] = 9      # hi > k
    assert _raw_call(batch, size, bad_span) == (E_ARG, True)
    with pytest.raises(RuntimeError):      # through the Python layer an error code is an exception
        nvsprep.NVSDevicePrep(size)(nvsprep.collate_nvs_raw([(_plan(size, k=33), items[0][1])]))
    with pytest.raises(NotImplementedError):
        nvsprep.collate_nvs_raw([(_plan(40, k=3), items[0][1])])


# ---- the CLI end to end -----------------------------------------------------------------------------------------------------------------
SIZE = 64      # the tiny model's canvas side


def _write_nvs_config(path, size):
    import yaml
    from oracle import golden_spec as GS
    dd = dict(double_z=True, z_channels=4, resolution=size, in_channels=3, out_ch=3, ch=64, ch_mult=[1, 2, 4, 4],
              num_res_blocks=1, attn_resolutions=[], dropout=0.0)
    data = dict(img_size=size, repeat_sp_token=4, sp_token="<special-token>", cfg=2.5, obj_dataset=True, warping_based=False, nviews=G.NVIEWS,
                dilate_size=[3, 9], pts_size=[3, 6], width_range=[32, 96], mask_enlarge=[0.05, 0.2], complete_mask_rate=0.0, warmup_mask_steps=2)
    model = {"target": "inpainting_ldm.NVS_ldm.NVSLDM", "params": dict(
        linear_start=0.00085, linear_end=0.0120, timesteps=1000, first_stage_key="image", cond_stage_key="txt", channels=4,
        cond_stage_trainable=True, conditioning_key="hybrid", scale_factor=0.18215, save_prompt_only=True, data_config=data,
        unet_config={"target": "ldm.modules.diffusionmodules.openaimodel.UNetModel", "params": GS.CONFIGS["MID"].kwargs()},
        first_stage_config={"target": "ldm.models.autoencoder.AutoencoderKL",
                            "params": {"ddconfig": dd, "embed_dim": 4, "lossconfig": {"target": "torch.nn.Identity"}}},
        cond_stage_config={"target": "ldm.modules.encoders.NVS_modules.NVSCLIPEmbedder",
                           "params": dict(freeze=False, layer="penultimate", cfg_rate=0.15, special_tokens=["repeat_4_<special-token>"],
                                          init_text=["reference on the left target on the right"])})}
    with open(path, "w") as f:
        yaml.safe_dump({"model": model}, f)


def test_train_cli_on_objaverse_renders_with_and_without_device_prep(fixture, tmp_path):
    """tools/train_inpainting.py --dataset objaverse --val on a tiny NVSLDM: three steps of two objects, then a validation of four.
    The tree is the fixture's with every render doubled (128 x 128: the box; 96 x 80: the bilinear; 64 x 64: the copy; one object
    without alpha).  Seeded and without loader workers, the host and the device route draw the same plans and the arithmetic is
    integer, so losses and validation metrics are equal bit for bit."""
    import yaml
    from oracle import golden_spec as GS
    from test_gpu_pairdata import _child, _state_dict, _stub_and_env
    big = {k: fixture.fx[k] for k in fixture.fx.files}
    for k, v in big.items():
        if v.ndim == 3 and v.shape[2] == 4:
            big[k] = np.kron(v, np.ones((2, 2, 1), np.uint8))
    tree = tmp_path / "tree"
    G.write_tree(str(tree), big)
    _write_nvs_config(str(tmp_path / "model_config.yaml"), SIZE)
    stub, env = _stub_and_env(tmp_path)
    torch.save({"state_dict": _state_dict(str(tmp_path / "model_config.yaml"), stub, GS.unet_state("MID"))}, str(tmp_path / "backbone.ckpt"))
    train_cfg = dict(model_config=str(tmp_path / "model_config.yaml"), resume_path=str(tmp_path / "backbone.ckpt"), max_steps=3, batch_size=2,
                     optim_cfg=dict(learning_rate=1e-3, weight_decay=0.01, lr_scheduler="cosine", eta_min=0.01),
                     datapath=str(tree / "objects"), train_list=str(tree / "train.txt"), val_list=str(tree / "val.txt"),
                     val_batch_size=4, val_check_interval=3)
    with open(str(tmp_path / "training.yaml"), "w") as f:
        yaml.safe_dump(train_cfg, f)
    runs = {}
    for route, extra in (("device", ["--device_prep"]), ("host", [])):
        cmd = [sys.executable, os.path.join(ROOT, "tools", "train_inpainting.py"), "--config_file", str(tmp_path / "training.yaml"),
               "--exp_name", route, "--save_path", str(tmp_path / "runs"), "--fp16", "--dataset", "objaverse", "--val", "--seed", "3",
               "--num_workers", "0", "--log_every_n_steps", "1", "--loss_file", str(tmp_path / f"{route}.json")] + extra
        stdout = _child(cmd, tmp_path, env, 600)
        print(stdout[-600:])
        assert "step 3: loss" in stdout and os.path.exists(str(tmp_path / "runs" / route / "ckpts" / "last.ckpt"))
        with open(str(tmp_path / f"{route}.json")) as f:
            losses = json.load(f)
        metrics = [ln for ln in stdout.splitlines() if ln.startswith(("psnr ", "ssim "))]
        assert len(losses) == 3 and np.isfinite(losses).all() and len(metrics) == 2 and np.isfinite([float(m.split()[1]) for m in metrics]).all()
        runs[route] = (losses, metrics)
    assert runs["device"][0] == runs["host"][0], "losses"
    assert runs["device"][1] == runs["host"][1], "validation metrics"
