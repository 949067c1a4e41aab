"""The image-pair datasets (dropin dataloaders/inpainting_crossview_dataset.py) and the multi-view collate against
tests/golden/pair_datasets.npz, which the REFERENCE's own classes wrote (tools/make_golden_pair_datasets.py: reference control flow
over a functional cv2 stand-in that resizes with this project's `resize_area_hw` / `resize_nearest`).  Both sides resize with the
same functions, so every comparison here is exact: image, masked_image as float32, mask, txt, and the generators' next values after
each seeded sequence (the draw count).  The tree is rebuilt from the fixture's arrays; nothing here reads the reference."""
import json
import os
import pickle
import random

import numpy as np
import pytest

import leftrefill_amd.dropin as dropin

dropin.install()
from leftrefill_amd import dataprep  # noqa: E402
from leftrefill_amd.dropin.dataloaders.inpainting_crossview_dataset import BalancedRandomSampler  # noqa: E402
from leftrefill_amd.dropin.dataloaders.inpainting_crossview_dataset import InpaintingCrossViewDataset, InpaintingMultiViewDataset  # noqa: E402
from tools import make_golden_pair_datasets as G  # noqa: E402

S = G.S
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "pair_datasets.npz")


class Fixture:
    """The loaded file, its tree written under `root`, and the recorded settings."""

    def __init__(self, root):
        self.root, self.fx = str(root), np.load(GOLDEN)
        G.write_tree(self.root, self.fx)
        self.spec = json.loads(str(self.fx["spec"]))

    def golden(self, name):
        items = G.unpack_items(self.fx[f"{name}/levels"], self.fx[f"{name}/mask_bits"], self.fx[f"{name}/txt"])
        return items, tuple(self.fx[f"{name}/next"])

    def run(self, name, **extra):
        """The recorded sequence of a setting through the drop-in: (items, next random.random(), next np.random.random())."""
        multi = name in self.spec["mv_settings"]
        kwargs, seed, indices = self.spec["mv_settings" if multi else "settings"][name]
        cls = InpaintingMultiViewDataset if multi else InpaintingCrossViewDataset
        return G.run_sequence(cls, dict(kwargs, **extra), seed, indices, self.root)


@pytest.fixture(scope="module")
def fixture(tmp_path_factory):
    return Fixture(tmp_path_factory.mktemp("pair_tree"))


def same_item(got, want, what):
    for k in ("image", "masked_image", "mask"):
        assert got[k].dtype == np.float32 and got[k].shape == want[k].shape, (what, k, got[k].dtype, got[k].shape)
        assert np.array_equal(got[k], want[k]), (what, k, int((got[k] != want[k]).sum()))
    txt = [str(t) for t in got["txt"]] if isinstance(got["txt"], (list, tuple)) else str(got["txt"])
    assert txt == want["txt"], (what, txt, want["txt"])


def test_the_drop_in_name_is_this_module_unless_another_tree_brings_its_own(tmp_path, monkeypatch):
    """`dataloaders.inpainting_crossview_dataset` after install(): this build's classes when no other `dataloaders` directory on sys.path
    holds such a module; that directory's module when one does (it was never shadowed), while the full name stays this build's."""
    import importlib
    import sys

    def forget():
        for name in [n for n in sys.modules if n == "dataloaders" or n.startswith("dataloaders.")]:
            monkeypatch.delitem(sys.modules, name)

    name = "inpainting_crossview_dataset"
    monkeypatch.setattr(sys, "path", [p for p in sys.path if not os.path.isfile(os.path.join(p or os.getcwd(), "dataloaders", name + ".py"))])
    forget()
    root = dropin.install()
    mod = importlib.import_module("dataloaders." + name)
    assert mod.__file__.startswith(root) and "raw" in mod.InpaintingCrossViewDataset.__init__.__code__.co_varnames
    other = tmp_path / "tree" / "dataloaders"
    other.mkdir(parents=True)
    (other / (name + ".py")).write_text("MARK = 'their own'\n")
    monkeypatch.syspath_prepend(str(tmp_path / "tree"))
    forget()
    dropin.install()
    assert importlib.import_module("dataloaders." + name).MARK == "their own"
    assert importlib.import_module("leftrefill_amd.dropin.dataloaders." + name).InpaintingCrossViewDataset is InpaintingCrossViewDataset
    forget()


def test_the_fixture_reaches_every_branch_of_the_reference():
    spec = json.loads(str(np.load(GOLDEN)["spec"]))
    assert set(spec["branch_tally"]) == set(G.BRANCH_LINES.values()) and min(spec["branch_tally"].values()) > 0
    assert os.path.getsize(GOLDEN) < 700 * 1024


@pytest.mark.parametrize("name", sorted(G.SETTINGS))
def test_crossview_items_are_the_references(fixture, name):
    want, nxt = fixture.golden(name)
    got, *got_next = fixture.run(name)
    assert len(got) == len(want)
    for n, (g, w) in enumerate(zip(got, want)):
        same_item(g, w, f"{name}[{n}]")
    assert tuple(got_next) == nxt, "the sequence drew another number of values than the reference"


@pytest.mark.parametrize("name", sorted(G.SETTINGS))
def test_raw_items_execute_to_the_same_samples_and_are_tie_free(fixture, name):
    """raw=True gives (plan, raw) whose host execution is the finished item; no area average any recorded plan takes lies within 1e-6
    of a rounding tie, so the device tests can compare exactly."""
    want, nxt = fixture.golden(name)
    got, *got_next = fixture.run(name, raw=True)
    assert tuple(got_next) == nxt
    for n, ((plan, raw), w) in enumerate(zip(got, want)):
        assert len(plan["tiles"]) == 2 and all(r.dtype == np.uint8 for r in raw)
        same_item(dataprep.run_plan_numpy(plan, raw), w, f"{name}[{n}] raw")
        for tile in plan["tiles"]:
            src = raw[tile["image"]]
            assert tile["rh"] <= src.shape[0] and tile["rw"] <= src.shape[1], "a fixture sample enlarges its source"
            assert (tile["rh"], tile["rw"]) in G.plan_sizes(*src.shape[:2])
            assert not G.near_tie(G._area_f64(src, tile["rh"], tile["rw"])).any(), (name, n, tile)
            assert tile["flip"] == tile["mask_flip"]      # a half's image and mask flip together


def test_plans_say_what_the_items_show(fixture):
    """View masks are outpaint_col = 0 beside a zero_mask tile; a match mask is a 256 x 256 plane of {0, 255} on one tile."""
    got, *_ = fixture.run("only_mask_image", raw=True)
    for plan, raw in got:
        cols = sorted(t["outpaint_col"] for t in plan["tiles"])
        assert cols == [-1, 0] and next(t for t in plan["tiles"] if t["outpaint_col"] < 0)["zero_mask"] and len(raw) == 2
        target_tile = next(k for k, t in enumerate(plan["tiles"]) if t["image"] == 1)
        assert plan["tiles"][target_tile]["outpaint_col"] == 0      # the target's half is the masked one
    got, *_ = fixture.run("match_right", raw=True)
    planes = [raw[2] for plan, raw in got if raw[2].shape == (256, 256)]
    assert len(planes) >= 3 and all(set(np.unique(p)) == {0, 255} for p in planes)
    kinds = fixture.spec["match_kinds"]
    for i, (plan, raw) in zip(fixture.spec["settings"]["match_right"][2], got):
        assert [t["image"] for t in plan["tiles"]] == [0, 1]      # constant_place: source left, target right
        matched = raw[2].shape == (256, 256)
        if matched:      # ... and the match mask on the right
            assert plan["tiles"][0]["zero_mask"] and plan["tiles"][1]["masks"] == [2]
        if kinds[str(i)] in ("missing", "few", "flat", "corners"):      # the None returns fall back to the random masks
            assert not matched, (i, kinds[str(i)])


def test_match_mask_without_a_file_draws_nothing(fixture):
    random.seed(5)
    state = random.getstate()
    assert dataprep.plan_match_mask(os.path.join(fixture.root, "match"), 2, "left", None, None) is None
    assert random.getstate() == state


def test_val_from_two_list_files_and_padding_and_raw_refusals(fixture):
    root = fixture.root
    pairs = [os.path.join(root, "val", f"pair_{i}") for i in range(4)]
    with open(os.path.join(root, "normal.txt"), "w") as f:
        f.write("".join(p + "\n" for p in pairs[:3]))
    with open(os.path.join(root, "special.txt"), "w") as f:
        f.write(pairs[3] + "\n")
    kw = dict(pair_path=None, mask_path=os.path.join(root, "val_masks"), mode="val", img_size=S, token_map=G.TOKEN_MAP)
    ds = InpaintingCrossViewDataset([os.path.join(root, "normal.txt"), os.path.join(root, "special.txt")], test_limit=3, **kw)
    assert ds.pairs == [pairs[3], pairs[0], pairs[1]]      # every special pair, then normal ones up to test_limit
    want, _ = fixture.golden("val")
    same_item(ds[1], want[0], "list-file val")      # pair_0 carries its own mask.png: independent of its index
    few = InpaintingCrossViewDataset(os.path.join(root, "val"), test_limit=150, **kw)      # fewer pairs than test_limit: stride 1
    assert len(few) == 4
    padded = InpaintingCrossViewDataset(os.path.join(root, "val"), test_limit=4, no_padding=False, **kw)[0]
    assert padded["image"].shape == (2 * S, 2 * S, 3) and padded["mask"].shape == (2 * S, 2 * S, 1) and padded["image"].dtype == np.float32
    assert np.array_equal(padded["image"][S // 2:S + S // 2], want[0]["image"]) and (padded["image"][:S // 2] == -1).all()
    assert not padded["mask"][:S // 2].any() and not padded["mask"][S + S // 2:].any()
    with pytest.raises(ValueError, match="S rows"):
        InpaintingCrossViewDataset(os.path.join(root, "val"), test_limit=4, no_padding=False, raw=True, **kw)


# ---- the sampler ----------------------------------------------------------------------------------------------------------------------
def _sampler_inputs(root):
    with open(os.path.join(root, "image_dict.pkl"), "rb") as f:
        image_dict = pickle.load(f)
    with open(os.path.join(root, "pairs.pkl"), "rb") as f:
        return image_dict, pickle.load(f)


def test_sampler_orders_follow_the_reference_through_three_epochs(fixture):
    image_dict, pairs = _sampler_inputs(fixture.root)
    n = fixture.spec["n_sample_per_scene"]
    for rank, replicas in fixture.spec["sampler_splits"]:
        sampler = BalancedRandomSampler(image_dict, pairs, n_sample_per_scene=n, rank=rank, num_replicas=replicas)
        want = fixture.fx[f"sampler/{rank}_{replicas}"]
        assert len(sampler) == want.shape[1]
        for epoch in range(3):
            sampler.set_epoch(epoch)
            assert list(sampler) == want[epoch].tolist(), (rank, replicas, epoch)
    assert fixture.fx["sampler/1_4"].shape[1] == 1      # 6 samples over 4 replicas: ceil((6 - 4) / 4), the reference's arithmetic
    # the per-scene lists are shuffled in place: epoch 2 alone is not epoch 2 after 0 and 1
    fresh = BalancedRandomSampler(image_dict, pairs, n_sample_per_scene=n)
    fresh.set_epoch(2)
    assert list(fresh) != fixture.fx["sampler/0_1"][2].tolist()


def test_sampler_refusals(fixture):
    image_dict, pairs = _sampler_inputs(fixture.root)
    with pytest.raises(ValueError, match="n_sample_per_scene"):
        BalancedRandomSampler(image_dict, pairs, n_sample_per_scene=5)      # the smaller scene has 4 pairs
    with pytest.raises(ValueError, match="rank"):
        BalancedRandomSampler(image_dict, pairs, n_sample_per_scene=2, rank=2, num_replicas=2)


# ---- multi-view -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(G.MV_SETTINGS))
def test_multiview_val_items_are_the_references(fixture, name):
    want, nxt = fixture.golden(name)
    kwargs = fixture.spec["mv_settings"][name][0]
    views = kwargs["view_num"] - 1 if kwargs.get("concat_target") else kwargs["view_num"]
    for extra in ({}, {"raw": True}):
        got, *got_next = fixture.run(name, **extra)
        assert tuple(got_next) == nxt
        for n, (g, w) in enumerate(zip(got, want)):
            if extra:
                assert len(g[0]["views"]) == views
                g = dataprep.run_plan_numpy(*g)
            assert g["image"].shape == (views, S, 2 * S if kwargs.get("concat_target") else S, 3)
            same_item(g, w, f"{name}[{n}]")
            assert g["idx"] == int(fixture.fx[f"{name}/idx"][n])
            if kwargs.get("concat_target"):
                assert not g["mask"][:, :, :S].any() and g["mask"][:, :, S:].any()
            else:
                assert not g["mask"][1:].any() and g["mask"][0].any()
    assert sorted(fixture.fx["mv_plain_v4/idx"].tolist()) == [3, 12]


def test_multiview_train_mode_raises():
    with pytest.raises(NotImplementedError, match="766.*721|721.*766"):
        InpaintingMultiViewDataset("nowhere", "nowhere", ["a", "b"], mode="train")


# ---- the collate ----------------------------------------------------------------------------------------------------------------------
def test_collate_of_pair_items(fixture):
    got, *_ = fixture.run("mixed", raw=True)
    items = got[:5]
    batch = dataprep.collate_raw(items, pin=False)
    jobs = dataprep.job_table(batch)
    assert (batch["batch"], batch["tiles"], batch["img_size"]) == (5, 2, S) and "views" not in batch and not batch["host"] and len(jobs) == 10
    arena, off = batch["arena"].numpy(), 0
    for b, (plan, raw) in enumerate(items):
        used = sorted({t["image"] for t in plan["tiles"]} | {m for t in plan["tiles"] for m in t["masks"]
                                                             if t["outpaint_col"] < 0 and not t["zero_mask"]})
        where = {}
        for t, tile in enumerate(plan["tiles"]):
            job = jobs[2 * b + t]
            assert (job["sample"], job["tile"]) == (b, t)
            want_flags = dataprep.FLIP_IMAGE * tile["flip"] + dataprep.FLIP_MASK * tile["mask_flip"] + dataprep.ZERO_MASK * tile["zero_mask"]
            assert job["flags"] == want_flags and job["outpaint_col"] == tile["outpaint_col"]
            assert [job[k] for k in ("rh", "rw", "y0", "x0")] == [tile[k] for k in ("rh", "rw", "y0", "x0")]
            where.setdefault(tile["image"], int(job["img_off"]))
            assert where[tile["image"]] == int(job["img_off"])
            src = raw[tile["image"]]
            assert np.array_equal(arena[job["img_off"]:job["img_off"] + src.size], src.reshape(-1))
            if tile["outpaint_col"] < 0 and not tile["zero_mask"]:
                for q, m in enumerate(tile["masks"]):
                    where.setdefault(m, int(job["mask_off"][q]))
                    assert np.array_equal(arena[job["mask_off"][q]:job["mask_off"][q] + raw[m].size], raw[m].reshape(-1))
                    assert (job["mask_h"][q], job["mask_w"][q]) == raw[m].shape
            else:
                assert (job["mask_off"] == -1).all()
        assert sorted(where) == used                                  # every source the sample uses, once ...
        first_use = list(where)                                       # ... tightly packed in the order the tiles first name them
        assert [where[i] for i in first_use] == [off + sum(raw[i].size for i in first_use[:k]) for k in range(len(first_use))]
        off += sum(raw[i].size for i in used)
    views = [j for j in jobs if j["outpaint_col"] == 0]
    assert views and all(not (j["flags"] & dataprep.ZERO_MASK) for j in views)      # `mixed` has whole-view masks among its first five


def test_collate_of_multiview_items(fixture):
    for name, views, tiles in (("mv_plain_v4", 4, 1), ("mv_concat_v4_shuffled", 3, 2)):
        items, *_ = fixture.run(name, raw=True)
        batch = dataprep.collate_raw(items, pin=False)
        jobs = dataprep.job_table(batch)
        assert (batch["batch"], batch["views"], batch["tiles"]) == (2, views, tiles) and len(jobs) == 2 * views * tiles
        assert batch["idx"].tolist() == fixture.fx[f"{name}/idx"].tolist()
        assert jobs["sample"].tolist() == [n for n in range(2 * views) for _ in range(tiles)]
        assert jobs["tile"].tolist() == list(range(tiles)) * (2 * views)
        assert len(batch["txt"]) == views and len(batch["txt"][0]) == 2      # txt[view][sample], as the DataLoader collates lists
        for b, (plan, raw) in enumerate(items):
            mine = jobs[b * views * tiles:(b + 1) * views * tiles]
            target_offs = {int(j["img_off"]) for j, t in zip(mine, [t for c in plan["views"] for t in c]) if t["image"] == 0}
            assert len(target_offs) == 1                                   # the target, shown by every canvas, is placed once
            assert len({int(j["img_off"]) for j in mine}) == views if tiles == 1 else views + 1
            masked = [j for j in mine if not j["flags"] & dataprep.ZERO_MASK]
            assert len(masked) == (1 if tiles == 1 else views) and all(int(j["img_off"]) in target_offs for j in masked)
            assert len({int(j["mask_off"][0]) for j in masked}) == 1
        assert int(jobs[-1]["img_off"]) < batch["arena"].numel()
    pair_item = fixture.run("val", raw=True)[0][0]
    with pytest.raises(AssertionError, match="one canvas shape"):
        dataprep.collate_raw([items[0], pair_item], pin=False)
