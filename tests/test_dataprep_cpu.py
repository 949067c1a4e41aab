"""The host side of device batch assembly (no GPU): the `dataloaders.inpainting_dataset.InpaintingDataset` drop-in -- plans, the order
and number of its random draws, prompts -- `dataprep.run_plan_numpy`, `dataprep.collate_raw`'s arena and job table, and the `raw`
keyword of `TestInpaintingDataset`.  Fixtures are tiny PNGs written into tmp_path."""
import os
import random

import numpy as np
import pytest

import leftrefill_amd.dropin as dropin

dropin.install()
from dataloaders.inpainting_dataset import InpaintingDataset  # noqa: E402
from dataloaders.raw_pairs import TestInpaintingDataset as RawTestInpaintingDataset  # noqa: E402
from dataloaders.test_dataset import TestInpaintingDataset, resize_area, resize_nearest  # noqa: E402
from leftrefill_amd import _lib, build, dataprep  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
S = 8
TOKENS = dict(left_token="left", right_token="right", task_token="viewpoints", real_token="scene")


@pytest.fixture(scope="module")
def data(tmp_path_factory):
    """6 images of mixed shapes (two smaller than S on one side: enlarging), 3 irregular and 2 segmentation masks, list files."""
    from PIL import Image
    root = tmp_path_factory.mktemp("dataprep")
    rng = np.random.RandomState(3)
    (root / "images").mkdir()
    for i, (h, w) in enumerate([(11, 29), (29, 11), (16, 24), (19, 23), (6, 20), (8, 8)]):
        Image.fromarray(rng.randint(0, 256, (h, w, 3), dtype=np.uint8)).save(str(root / "images" / f"im_{i}.png"))
    lists = {}
    for kind, shapes in (("irregular", [(5, 7), (40, 33), (8, 8)]), ("segment", [(12, 9), (8, 8)])):
        (root / kind).mkdir()
        names = []
        for i, (h, w) in enumerate(shapes):
            Image.fromarray(rng.choice(np.array([0, 127, 128, 255], dtype=np.uint8), size=(h, w))).save(str(root / kind / f"m_{i}.png"))
            names.append(str(root / kind / f"m_{i}.png"))
        lists[kind] = str(root / f"{kind}.txt")
        with open(lists[kind], "w") as f:
            f.write("\n".join(names) + "\n")
    with open(str(root / "images.txt"), "w") as f:
        f.write("\n".join(f"im_{i}.png" for i in range(6)) + "\n")
    return dict(root=str(root), images=str(root / "images"), image_txt=str(root / "images.txt"),
                train_masks=[lists["irregular"], lists["segment"]], mask_dir=str(root / "irregular"))


def _train(data, **kw):
    kw.setdefault("repeat_sp_token", 3)
    kw.setdefault("sp_token", "<special-token>")
    return InpaintingDataset(data["images"], mask_path=data["train_masks"], mode="train", img_size=S, **kw)


def _seed(seed):
    random.seed(seed)
    np.random.seed(seed)


def _same(a, b):
    assert a["txt"] == b["txt"]
    for k in ("image", "masked_image", "mask"):
        assert a[k].dtype == b[k].dtype == np.float32 and a[k].shape == b[k].shape and a[k].tobytes() == b[k].tobytes(), k


def _seed_for(data, want, **kw):
    """A seed under which item 0's plan satisfies `want` (searched, so the branches are forced by seeding)."""
    ds = _train(data, raw=True, **kw)
    for seed in range(200):
        _seed(seed)
        plan, raw = ds[0]
        if want(plan["tiles"][0], raw):
            return seed
    raise AssertionError("no seed below 200 reaches the branch")


BRANCHES = {
    "irregular": lambda t, raw: len(t["masks"]) == 1 and raw[1].shape in ((5, 7), (40, 33)),
    "segment": lambda t, raw: len(t["masks"]) == 1 and raw[1].shape == (12, 9),
    "both": lambda t, raw: len(t["masks"]) == 2,
    "direct_resize": lambda t, raw: (t["rh"], t["rw"]) == (S, S),
    "resize_and_crop": lambda t, raw: t["rw"] > S and t["x0"] > 0,
    "both_flips": lambda t, raw: t["flip"] and t["mask_flip"],
}


@pytest.mark.parametrize("branch", sorted(BRANCHES))
def test_finished_sample_is_the_plan_run_on_the_host(data, branch):
    seed = _seed_for(data, BRANCHES[branch])
    for idx in range(6):      # every image shape, the enlarging ones included
        _seed(seed)
        done = _train(data)[idx]
        _seed(seed)
        plan, raw = _train(data, raw=True)[idx]
        _same(done, dataprep.run_plan_numpy(plan, raw))
        assert done["image"].shape == (S, S, 3) and done["mask"].shape == (S, S, 1)
        assert set(np.unique(done["mask"])) <= {0.0, 1.0} and np.array_equal(done["masked_image"], done["image"] * (done["mask"] < 0.5))
        assert all(a.dtype == np.uint8 for a in raw) and all(isinstance(v, (int, bool, list)) for v in plan["tiles"][0].values())


def test_outpainting_val_and_test_modes(data):
    _seed(4)
    done = _train(data, outpainting=True)[2]
    _seed(4)
    plan, raw = _train(data, outpainting=True, raw=True)[2]
    _same(done, dataprep.run_plan_numpy(plan, raw))
    tile = plan["tiles"][0]
    col = tile["outpaint_col"]
    assert len(raw) == 1 and not tile["masks"] and 2 <= col <= 6      # int((0.25 .. 0.75) * 8)
    want = np.zeros((S, S), np.float32)
    want[:, col:] = 1
    assert np.array_equal(done["mask"][:, :, 0], want[:, ::-1] if tile["mask_flip"] else want)
    for mode in ("val", "test"):
        kw = dict(mask_path=data["mask_dir"], mode=mode, img_size=S, test_limit=3, token_map=TOKENS)
        ds, ds_raw = InpaintingDataset(data["images"], **kw), InpaintingDataset(data["images"], raw=True, **kw)
        assert len(ds) == (3 if mode == "val" else 6)      # val: every (6 // 3)-th image, masks strided alike (3 // 3 = 1)
        for idx in range(len(ds)):
            plan, raw = ds_raw[idx]
            _same(ds[idx], dataprep.run_plan_numpy(plan, raw))
            t = plan["tiles"][0]
            assert (t["rh"], t["rw"], t["y0"], t["x0"], t["flip"], t["mask_flip"]) == (S, S, 0, 0, False, False)
            assert ds[idx]["txt"] == "Both left and right images show the scene with different viewpoints."
        if mode == "test":      # the bicubic resize happened on the host: the plan is the identity
            assert all(ds_raw[i][1][0].shape == (S, S, 3) for i in range(6))
    # the validation sample is the yardstick's: area resize, nearest mask thresholded at > 127
    from PIL import Image
    val = InpaintingDataset(data["images"], mask_path=data["mask_dir"], mode="val", img_size=S, test_limit=6, token_map=TOKENS)
    img = np.asarray(Image.open(os.path.join(data["images"], "im_2.png")).convert("RGB"))
    m = np.asarray(Image.open(os.path.join(data["mask_dir"], "m_2.png")).convert("L"))
    assert np.array_equal(val[2]["image"], resize_area(img, S).astype(np.float32) / 127.5 - 1.0)
    assert np.array_equal(val[2]["mask"][:, :, 0], (resize_nearest(m, S) > 127).astype(np.float32))
    # a list file with root_path reads the same images as the folder
    listed = InpaintingDataset(data["image_txt"], root_path=data["images"], mask_path=data["mask_dir"], mode="val", img_size=S,
                               test_limit=6, token_map=TOKENS)
    _same(listed[3], val[3])


def _draws(monkeypatch, ds, idx):
    """The generator calls of one item, in order: (name, arguments)."""
    calls = []

    def counting(mod, name, label):
        real = getattr(mod, name)

        def wrapper(*a, **k):
            calls.append((label, a[:2] if label == "randint" else ()))
            return real(*a, **k)
        monkeypatch.setattr(mod, name, wrapper)

    counting(random, "random", "random")
    counting(random, "randint", "randint")
    counting(np.random, "random", "np.random")
    counting(np.random, "choice", "np.choice")
    item = ds[idx]
    monkeypatch.undo()
    return calls, item


def test_draws_follow_the_reference_order_and_count(data, monkeypatch):
    """reference inpainting_dataset.py: resize branch (70), crop column then row (81-82), mask branch (90) and indices (92 | 96 | 100-101),
    image flip (176), mask flip (178), template (145)."""
    seen = set()
    for seed in range(40):
        # the reference's sequence replayed by hand from the same seed: item 0 is 11 x 29 -> resized 8 x 21 in the crop branch;
        # 3 irregular and 2 segmentation masks
        random.seed(seed)
        want = [("random", ())]
        crop = not random.random() < 0.5
        if crop:
            want += [("randint", (0, 21 - S)), ("randint", (0, 0))]
            random.randint(0, 21 - S), random.randint(0, 0)
        want += [("random", ())]
        rdv = random.random()
        if rdv < 0.4:
            want += [("randint", (0, 2))]                              # one irregular mask
        elif rdv < 0.8:
            want += [("randint", (0, 1))]                              # one segmentation mask
        else:
            want += [("randint", (0, 1)), ("randint", (0, 2))]         # segmentation, then irregular
        want += [("random", ()), ("random", ()), ("np.choice", ())]
        _seed(seed)
        ds = _train(data, raw=True, repeat_sp_token=0, token_map=TOKENS)
        calls, (plan, raw) = _draws(monkeypatch, ds, 0)
        tile = plan["tiles"][0]
        assert calls == want, (seed, calls)
        assert ((tile["rh"], tile["rw"]) == (8, 21)) == crop and len(tile["masks"]) == (1 if rdv < 0.8 else 2)
        irregular, segment = ((5, 7), (40, 33), (8, 8)), ((12, 9), (8, 8))      # the list each mask was read from
        if rdv < 0.4:
            assert raw[1].shape in irregular
        else:
            assert raw[1].shape in segment and (rdv < 0.8 or raw[2].shape in irregular)
        seen.add((crop, 0 if rdv < 0.4 else 1 if rdv < 0.8 else 2))
    assert seen == {(c, k) for c in (False, True) for k in (0, 1, 2)}
    # outpainting: one np.random.random in place of the mask draws; flip=False: no flip draws; a repeated token: no template draw
    _seed(0)
    calls, _ = _draws(monkeypatch, _train(data, raw=True, outpainting=True, flip=False), 5)
    assert [c[0] for c in calls if c[0] != "randint"] == ["random", "np.random"]
    # val / test: nothing is drawn
    ds = InpaintingDataset(data["images"], mask_path=data["mask_dir"], mode="val", img_size=S, test_limit=6, token_map=TOKENS)
    assert _draws(monkeypatch, ds, 1)[0] == []


def test_seeded_picks_are_the_reference_formulas(data):
    """The same seed, the reference's expressions written out: branch thresholds 0.5 / 0.4 / 0.8 / 0.5 / 0.5 and the long side."""
    for seed in range(12):
        _seed(seed)
        plan, raw = _train(data, raw=True)[1]      # 29 x 11: h >= w
        tile = plan["tiles"][0]
        random.seed(seed)
        if random.random() < 0.5:
            want = (S, S, 0, 0)
        else:
            long_side = max(S, int(29 * (S / 11)))
            x0 = random.randint(0, 0)
            want = (long_side, S, random.randint(0, long_side - S), x0)
        assert (tile["rh"], tile["rw"], tile["y0"], tile["x0"]) == want
        assert len(tile["masks"]) == (1 if random.random() < 0.8 else 2)


def test_collate_raw_job_table(data):
    crop = _seed_for(data, BRANCHES["resize_and_crop"])
    both = _seed_for(data, BRANCHES["both"])
    ds = _train(data, raw=True)
    _seed(crop)
    a = ds[0]
    _seed(both)
    b = ds[3]
    _seed(both)
    c = ds[4]                                      # 6 x 20: smaller than S on one side -> the host route
    out = _train(data, raw=True, outpainting=True)
    _seed(1)
    d = out[2]
    batch = dataprep.collate_raw([a, b, c, d], pin=False)
    jobs = dataprep.job_table(batch)
    assert (batch["batch"], batch["tiles"], batch["img_size"]) == (4, 1, S) and len(jobs) == 4
    assert batch["txt"] == [a[0]["txt"]] * 4 and batch["arena"].numel() % 16 == 0
    arena = batch["arena"].numpy()
    off = 0
    for i, (plan, raw) in enumerate([a, b, c, d]):
        job, tile = jobs[i], plan["tiles"][0]
        assert (job["sample"], job["tile"]) == (i, 0)
        if i == 2:
            assert job["flags"] == dataprep.HOST and [h[0] for h in batch["host"]] == [2]
            continue
        assert job["img_off"] == off and (job["img_h"], job["img_w"]) == raw[0].shape[:2]
        assert np.array_equal(arena[off:off + raw[0].size], raw[0].reshape(-1))
        off += raw[0].size
        assert (job["rh"], job["rw"], job["y0"], job["x0"]) == (tile["rh"], tile["rw"], tile["y0"], tile["x0"])
        assert job["flags"] == dataprep.FLIP_IMAGE * tile["flip"] + dataprep.FLIP_MASK * tile["mask_flip"]
        assert job["outpaint_col"] == tile["outpaint_col"]
        for q in range(2):
            if q < len(tile["masks"]):
                m = raw[tile["masks"][q]]
                assert job["mask_off"][q] == off and (job["mask_h"][q], job["mask_w"][q]) == m.shape
                assert np.array_equal(arena[off:off + m.size], m.reshape(-1))
                off += m.size
            else:
                assert job["mask_off"][q] == -1
    assert jobs[3]["outpaint_col"] >= 2 and len(d[0]["tiles"][0]["masks"]) == 0
    assert len({int(j["img_off"]) % 4 for j in jobs if j["flags"] != dataprep.HOST}) > 1      # tightly packed: unaligned offsets
    assert off <= batch["arena"].numel() < off + 16


def test_prompts(data):
    ds = _train(data, repeat_sp_token=0, token_map=TOKENS)
    assert ds.templates() == [
        "Both left and right images show the scene with different viewpoints.",
        "The scene remains the same in both the left and right images, but the viewpoints are different.",
        "The left and right images depict identical scene, but from different viewpoints.",
        "The painting depicts the scene, but from two different viewpoints; one from the left and one from the right.",
        "Both figures capture the same scene, but the left one and the right one are taken from different viewpoints.",
        "The two drawings show the scene, but one is from the left side and the other is from the right side, and they are from different viewpoints",
        "Both pictures depict the same scene, but the left image and the right image are captured with different viewpoints."]
    np.random.seed(0)
    got = {ds.get_prompt() for _ in range(200)}
    assert got == set(ds.templates()) and all(type(p) is str for p in got)
    assert _train(data).get_prompt() == "<special-token0> <special-token1> <special-token2>"
    deep = _train(data, repeat_sp_token=2, deep_prompt=True).get_prompt()
    assert len(deep) == 16 and deep[0] == "<special-token0-layer0> <special-token1-layer0>"
    assert deep[15] == "<special-token0-layer15> <special-token1-layer15>"


def test_test_dataset_raw_keyword_keeps_the_default(tmp_path):
    from PIL import Image
    rng = np.random.RandomState(1)
    for i, (h, w) in enumerate([(16, 24), (19, 23)]):
        d = tmp_path / f"pair_{i}"
        d.mkdir()
        for stem in ("source", "target"):
            Image.fromarray(rng.randint(0, 256, (h, w, 3), dtype=np.uint8)).save(str(d / f"{stem}.png"))
        m = (rng.rand(h, w) < 0.5).astype(np.uint8) * 255
        Image.fromarray(np.stack([m] * 3, -1)).save(str(d / "mask.png"))
    plain = TestInpaintingDataset(str(tmp_path), img_size=S)      # dataloaders.test_dataset itself, which knows no `raw`
    omitted, explicit = RawTestInpaintingDataset(str(tmp_path), img_size=S), RawTestInpaintingDataset(str(tmp_path), img_size=S, raw=False)
    raw = RawTestInpaintingDataset(str(tmp_path), img_size=S, raw=True)
    for i in range(2):
        _same(plain[i], explicit[i])
        _same(plain[i], omitted[i])
        plan, arrays = raw[i]
        assert len(plan["tiles"]) == 2 and plan["tiles"][0]["zero_mask"] and plan["tiles"][1]["masks"] == [2]
        _same(plain[i], dataprep.run_plan_numpy(plan, arrays))      # a {0, 255} mask: the threshold changes nothing
        assert plain[i]["image"].shape == (S, 2 * S, 3) and not plain[i]["mask"][:, :S].any()
    batch = dataprep.collate_raw([raw[0], raw[1]], pin=False)
    jobs = dataprep.job_table(batch)
    assert [(int(j["sample"]), int(j["tile"]), int(j["flags"])) for j in jobs] == [(0, 0, 4), (0, 1, 0), (1, 0, 4), (1, 1, 0)]


def test_cli_loaders_take_test_limit_from_the_model_data_section(data):
    """The reference's model configs carry `test_limit` in data_config, which the CLI hands to the dataset with the rest of it."""
    from types import SimpleNamespace
    from tools.train_inpainting import inpainting_loaders
    model = SimpleNamespace(img_size=S, data_cfg={"repeat_sp_token": 2, "sp_token": "<special-token>", "cfg": 2.5, "test_limit": 3})
    config = dict(image_path=data["images"], train_mask_path=data["train_masks"], val_image_path=data["images"],
                  val_mask_path=data["mask_dir"], val_batch_size=2, test_limit=6)
    for device_prep in (False, True):
        train, val = inpainting_loaders(config, model, 2, device_prep, True, 0, "cpu")
        held = (val.loader if device_prep else val).dataset
        assert len(held) == 3 and held.raw == device_prep and len(train) == 3      # data_config's 3 wins over the training config's 6
    assert inpainting_loaders(config, model, 2, False, False, 0, "cpu")[1] is None
    model.data_cfg.pop("test_limit")
    assert len(inpainting_loaders(config, model, 2, False, True, 0, "cpu")[1].dataset) == 6      # the training config's, when it is the only one
    with pytest.raises(SystemExit, match="val_batch_size"):
        inpainting_loaders(dict(config, val_batch_size=8), model, 2, False, True, 0, "cpu")


def test_collate_raw_refuses_finished_samples(data):
    _seed(0)
    with pytest.raises(TypeError, match="raw=True"):
        dataprep.collate_raw([_train(data)[0]], pin=False)


def test_binding_and_declaration():
    import abi_helpers as abi
    assert len(abi.c_params("lr_batch_prep")) == 12
    assert "batch_prep.hip" in build.SOURCES and _lib.ABI_VERSION == 30
    for name, value in (("FLIP_IMAGE", 1), ("FLIP_MASK", 2), ("ZERO_MASK", 4), ("HOST", 8), ("MAX_SIZE", 512), ("ROW_BYTES", 24576)):
        assert abi.define(f"LR_PREP_{name}") == value and getattr(dataprep, name) == value
