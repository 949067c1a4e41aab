"""The image-pair and multi-view batches on the MI355X: `collate_raw` + `DevicePrep` (one lr_batch_prep launch per batch) against the
items the REFERENCE's datasets returned (tests/golden/pair_datasets.npz, see test_pairdata_cpu.py), bit for bit -- the fixture has no
area average within 1e-6 of a rounding tie (asserted on the CPU), so there is no tie allowance here -- and the two CLIs end to end with
and without --device_prep.  These are the first cases to drive the kernel with windows and flips on both tiles at once, a mask on the
left tile, a 256 x 256 mask source shrunk to S = 32, outpaint_col = 0 and B·V samples in one launch."""
import functools
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import leftrefill_amd.dropin as dropin

dropin.install()
from leftrefill_amd import dataprep  # noqa: E402
from rawdata_helpers import KEYS, device_batch, same_bits as _same_bits  # noqa: E402
from test_pairdata_cpu import Fixture  # noqa: E402
from tools import make_golden_pair_datasets as G  # noqa: E402

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
S = G.S


@pytest.fixture(scope="module")
def fixture(tmp_path_factory):
    return Fixture(tmp_path_factory.mktemp("pair_tree"))


_device = functools.partial(device_batch, dataprep.collate_raw)


@pytest.mark.parametrize("name", sorted(G.SETTINGS))
def test_crossview_batches_equal_the_references_items(fixture, name):
    want, _ = fixture.golden(name)
    items, *_ = fixture.run(name, raw=True)
    prep = dataprep.DevicePrep(S, tiles=2)
    for bs in (1, 5):
        for at in range(0, len(items), bs):
            chunk = items[at:at + bs]
            out = _device(prep, chunk)
            assert out["image"].shape == (len(chunk), S, 2 * S, 3) and out["mask"].shape == (len(chunk), S, 2 * S, 1)
            for b in range(len(chunk)):
                _same_bits({k: out[k][b] for k in KEYS}, want[at + b], f"{name}[{at + b}] in batches of {bs}")
                assert out["txt"][b] == want[at + b]["txt"] if isinstance(want[at + b]["txt"], str) else \
                    [t[b] for t in out["txt"]] == want[at + b]["txt"]
    assert not prep.warned      # nothing took the host route


def test_the_recorded_sequences_drive_the_new_kernel_regimes(fixture):
    """What the comparisons above covered, read off the job tables: both tiles windowed and flipped at once, a mask on the left tile,
    a 256 x 256 mask source, outpaint_col = 0 -- each with the flip flags set and clear."""
    seen = set()
    for name in G.SETTINGS:
        items, *_ = fixture.run(name, raw=True)
        jobs = dataprep.job_table(dataprep.collate_raw(items, pin=False))
        for left, right in zip(jobs[0::2], jobs[1::2]):
            both = dataprep.FLIP_IMAGE | dataprep.FLIP_MASK
            if all((j["rh"], j["rw"]) != (S, S) and j["y0"] + j["x0"] > 0 for j in (left, right)):
                seen.add("windows on both tiles")
            if left["flags"] & both == both and right["flags"] & both == both:
                seen.add("flips on both tiles")
            if left["mask_off"][0] >= 0:
                seen.add("mask on the left tile")
            for j in (left, right):
                if (j["mask_h"][0], j["mask_w"][0]) == (256, 256):
                    seen.add("256 mask flipped" if j["flags"] & dataprep.FLIP_MASK else "256 mask")
                if j["outpaint_col"] == 0:
                    seen.add("view mask flipped" if j["flags"] & dataprep.FLIP_MASK else "view mask")
                if j["mask_off"][1] >= 0:
                    seen.add("two mask sources")
    assert seen == {"windows on both tiles", "flips on both tiles", "mask on the left tile", "256 mask", "256 mask flipped", "view mask",
                    "view mask flipped", "two mask sources"}, seen


@pytest.mark.parametrize("name", sorted(G.MV_SETTINGS))
def test_multiview_batches_equal_the_references_items(fixture, name):
    want, _ = fixture.golden(name)
    items, *_ = fixture.run(name, raw=True)
    kwargs = fixture.spec["mv_settings"][name][0]
    tiles, views = (2, kwargs["view_num"] - 1) if kwargs.get("concat_target") else (1, kwargs["view_num"])
    prep = dataprep.DevicePrep(S, tiles=tiles)
    out = _device(prep, items)
    assert out["image"].shape == (len(items), views, S, tiles * S, 3) and out["mask"].shape == (len(items), views, S, tiles * S, 1)
    assert out["idx"].tolist() == fixture.fx[f"{name}/idx"].tolist()
    for b in range(len(items)):
        _same_bits({k: out[k][b] for k in KEYS}, want[b], f"{name}[{b}]")
        assert [t[b] for t in out["txt"]] == want[b]["txt"]
    ptrs = [t.data_ptr() for t in (prep.arena, prep.jobs, prep.image, prep.masked_image, prep.mask)]
    out = _device(prep, items[-1:])      # a smaller batch: the buffers are reused
    assert ptrs == [t.data_ptr() for t in (prep.arena, prep.jobs, prep.image, prep.masked_image, prep.mask)]
    assert out["image"].shape[:2] == (1, views)
    _same_bits({k: out[k][0] for k in KEYS}, want[len(items) - 1], f"{name} second call")


def test_an_enlarging_sample_alone_takes_the_host_route(fixture):
    """A pair batch and a multi-view batch, each mixing a device sample with one whose source is smaller than S."""
    rng = np.random.RandomState(3)
    small = rng.randint(0, 256, (20, 45, 3), dtype=np.uint8)
    want, _ = fixture.golden("val")
    items, *_ = fixture.run("val", raw=True)
    plan, raw = items[0]
    enlarging = (dict(plan, tiles=[dict(plan["tiles"][0], flip=True), plan["tiles"][1]]), [small] + raw[1:])
    prep = dataprep.DevicePrep(S, tiles=2)
    with pytest.warns(UserWarning, match="on the host"):
        batch = dataprep.collate_raw([items[1], enlarging, items[2]])
        out = prep(batch)
    assert [h[0] for h in batch["host"]] == [1] and (dataprep.job_table(batch)["flags"][2:4] == dataprep.HOST).all()
    host = dataprep.run_plan_numpy(*enlarging)
    for k in KEYS:
        assert out[k][1].cpu().numpy().tobytes() == host[k].tobytes(), k
    for b, n in ((0, 1), (2, 2)):
        _same_bits({k: out[k][b].cpu() for k in KEYS}, want[n], f"beside the host sample {b}")
    want, _ = fixture.golden("mv_concat_v3")
    items, *_ = fixture.run("mv_concat_v3", raw=True)
    plan, raw = items[1]
    enlarging = (plan, [raw[0], small] + raw[2:])      # the first reference view is the small image
    prep = dataprep.DevicePrep(S, tiles=2)
    batch = dataprep.collate_raw([enlarging, items[0]])
    with pytest.warns(UserWarning, match="on the host"):
        out = prep(batch)
    assert [h[0] for h in batch["host"]] == [0] and out["image"].shape == (2, 2, S, 2 * S, 3)
    host = dataprep.run_plan_numpy(*enlarging)
    for k in KEYS:
        assert out[k][0].cpu().numpy().tobytes() == host[k].tobytes(), k
    _same_bits({k: out[k][1].cpu() for k in KEYS}, want[0], "beside the multi-view host sample")


# ---- the CLIs end to end ---------------------------------------------------------------------------------------------------------------
SIZE = 64      # the tiny models' canvas side


def _tree_at_64(root, fx):
    """The fixture's tree with every image doubled (all sides >= 64, so nothing enlarges at S = 64) and de-tied again at the sizes a
    64-pixel plan asks for, and a mask.png in every multi-view folder (the evaluation CLI reads masks from the folders only)."""
    rng = np.random.RandomState(64)
    big = {k: fx[k] for k in fx.files}
    for k in fx.files:
        if k.startswith("pool_"):
            big[k] = G.detie(np.kron(fx[k], np.ones((2, 2, 1), np.uint8)), rng, SIZE)
            assert not any(G.near_tie(G._area_f64(big[k], rh, rw)).any() for rh, rw in G.plan_sizes(*big[k].shape[:2], SIZE))
    layout = json.loads(str(fx["layout"]))
    layout["png"]["mv/12/mask.png"] = "segment_1"
    big["layout"] = np.array(json.dumps(layout))
    G.write_tree(str(root), big)


def _stub_and_env(tmp_path):
    stub = tmp_path / "stubs"
    stub.mkdir()
    (stub / "open_clip.py").write_text("from oracle.clip_stub import *  # noqa: F401,F403  (test stand-in for the absent package)\n")
    return stub, dict(os.environ, PYTHONPATH=os.pathsep.join([str(stub), ROOT, os.environ.get("PYTHONPATH", "")]))


def _state_dict(config_file, stub, unet_state):
    from oracle import weights
    sys.path.insert(0, str(stub))
    try:
        from inpainting_ldm.model import create_model
        model = create_model(config_file)
    finally:
        sys.path.remove(str(stub))
    sd = dict(model.state_dict())
    for k, v in model.state_dict().items():
        if k.startswith("first_stage_model."):
            sd[k] = torch.from_numpy(weights.fill_like("vae2." + k[len("first_stage_model."):], v.shape)).to(v.dtype)
    for k, v in unet_state.items():
        sd["model.diffusion_model." + k] = v
    return sd


def _child(cmd, tmp_path, env, limit):
    """One fresh child process under its own time limit; a failure ends the test."""
    r = subprocess.run(cmd, capture_output=True, text=True, cwd=str(tmp_path), env=env, timeout=limit)
    assert r.returncode == 0, r.stdout[-1500:] + r.stderr[-3000:]
    return r.stdout


def test_train_cli_on_image_pairs_with_and_without_device_prep(fixture, tmp_path):
    """tools/train_inpainting.py --dataset crossview --val on the tiny model of test_gpu_harness.py: three steps of three pairs -- one
    epoch of the sampler's six and the first batch of the next -- then a validation.  Seeded and without loader workers, the host and
    the device route draw the same plans; the tree is tie-free, so losses and validation metrics are equal bit for bit.  The indices
    drawn are the reference sampler's epoch 0 and epoch 1 orders."""
    import yaml
    from test_gpu_harness import _write_config
    from oracle import golden_spec as GS
    tree = tmp_path / "tree"
    _tree_at_64(tree, fixture.fx)
    _write_config(str(tmp_path / "model_config.yaml"), SIZE)
    with open(str(tmp_path / "model_config.yaml")) as f:
        cfg = yaml.safe_load(f)
    cfg["model"]["params"]["data_config"].update(cfg=2.5, test_limit=4, flip=True, view_mask_rate=0.5, match_mask=True, match_mask_rate=0.5,
                                                 match_path=str(tree / "match"))
    cfg["model"]["params"]["save_prompt_only"] = True
    with open(str(tmp_path / "model_config.yaml"), "w") as f:
        yaml.safe_dump(cfg, f)
    stub, env = _stub_and_env(tmp_path)
    torch.save({"state_dict": _state_dict(str(tmp_path / "model_config.yaml"), stub, GS.unet_state("MID"))}, str(tmp_path / "backbone.ckpt"))
    train_cfg = dict(model_config=str(tmp_path / "model_config.yaml"), resume_path=str(tmp_path / "backbone.ckpt"), max_steps=3, batch_size=3,
                     optim_cfg=dict(learning_rate=1e-3, weight_decay=0.01, lr_scheduler="cosine", eta_min=0.01),
                     image_path=str(tree / "image_dict.pkl"), train_pair=str(tree / "pairs.pkl"), n_sample_per_scene=3,
                     train_mask_path=[str(tree / "irregular.txt"), str(tree / "segment.txt")], val_image_path=str(tree / "val"),
                     val_mask_path=str(tree / "val_masks"), val_batch_size=4, val_check_interval=3)
    with open(str(tmp_path / "training.yaml"), "w") as f:
        yaml.safe_dump(train_cfg, f)
    runs = {}
    for route, extra in (("device", ["--device_prep"]), ("host", [])):
        cmd = [sys.executable, os.path.join(ROOT, "tools", "train_inpainting.py"), "--config_file", str(tmp_path / "training.yaml"),
               "--exp_name", route, "--save_path", str(tmp_path / "runs"), "--fp16", "--dataset", "crossview", "--val", "--seed", "3",
               "--num_workers", "0", "--log_every_n_steps", "1", "--loss_file", str(tmp_path / f"{route}.json"), "--index_file",
               str(tmp_path / f"{route}_indices.json")] + extra
        stdout = _child(cmd, tmp_path, env, 600)
        print(stdout[-600:])
        assert "step 3: loss" in stdout and "Steps:" in stdout and os.path.exists(str(tmp_path / "runs" / route / "ckpts" / "last.ckpt"))
        with open(str(tmp_path / f"{route}.json")) as f:
            losses = json.load(f)
        with open(str(tmp_path / f"{route}_indices.json")) as f:
            indices = json.load(f)
        metrics = [ln for ln in stdout.splitlines() if ln.startswith(("psnr ", "ssim "))]
        assert len(losses) == 3 and np.isfinite(losses).all() and len(metrics) == 2 and np.isfinite([float(m.split()[1]) for m in metrics]).all()
        runs[route] = (losses, metrics, indices)
    assert runs["device"][0] == runs["host"][0], "losses"
    assert runs["device"][1] == runs["host"][1], "validation metrics"
    order = fixture.fx["sampler/0_1"]
    for route in runs:      # the second epoch's batches follow the sampler's epoch-1 order (after epoch 0: the shuffles are in place)
        assert runs[route][2] == [order[0].tolist(), order[1].tolist()], route


def test_evaluation_cli_on_multiview_folders_with_and_without_device_prep(fixture, tmp_path):
    """tools/run_inpainting.py --multiview --test_path on the two multi-view folders, [reference | target] canvases of a three-view
    model: the same metric lines from the host loader and from the 5-D device route."""
    from test_gpu_harness import _write_mv_config
    from oracle import unet_ref, weights
    tree = tmp_path / "tree"
    _tree_at_64(tree, fixture.fx)
    mdir = tmp_path / "synthetic_mv_model"
    (mdir / "ckpts").mkdir(parents=True)
    cfg = _write_mv_config(str(mdir / "model_config.yaml"), SIZE, 3, True)
    stub, env = _stub_and_env(tmp_path)
    unet = weights.fill_state_dict(unet_ref.param_shapes(cfg), prefix="unet.MV.")
    torch.save({"state_dict": _state_dict(str(mdir / "model_config.yaml"), stub, unet)}, str(mdir / "ckpts" / "epoch=1.ckpt"))
    lines = {}
    for route, extra in (("device", ["--device_prep"]), ("host", [])):
        cmd = [sys.executable, os.path.join(ROOT, "tools", "run_inpainting.py"), "--multiview", "--model_path", str(mdir), "--test_path",
               str(tree / "mv"), "--test_size", str(SIZE), "--metric_size", "32", "--batch_size", "2", "--cfg", "2.5", "--eta", "1.0",
               "--output_path", str(tmp_path / f"out_{route}"), "--metric_output", str(tmp_path / f"metrics_{route}")] + extra
        stdout = _child(cmd, tmp_path, env, 600)
        assert "WARNING" not in stdout, stdout[-1500:]
        lines[route] = [ln for ln in stdout.splitlines() if ln.startswith(("PSNR:", "SSIM:", "LPIPS:"))]
        print(lines[route])
        assert len(lines[route]) == 3 and "over 2 images" in lines[route][0] and 3.0 < float(lines[route][0].split()[1]) < 60.0
    assert lines["device"] == lines["host"]
