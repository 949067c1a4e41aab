"""The Objaverse NVS dataset (dropin dataloaders/obj_nvs_dataset.py) and the numpy statement of its arithmetic (leftrefill_amd/nvsprep.py)
against tests/golden/nvs_dataset.npz, which the REFERENCE's own class wrote (tools/make_golden_nvs_dataset.py: reference control flow
over a functional cv2 stand-in that dispatches to nvsprep's restatements of the four OpenCV primitives).  Both sides use the same
primitives, so every comparison here is exact: image, masked_image, mask, rel_pose, txt, and the generators' next values after each
seeded sequence (the draw count).  What is pinned is the control flow, the draws, the composite and the composition; the primitives
are pinned against their literal statements below, not against OpenCV.  The tree is rebuilt from the fixture's arrays; nothing here
reads the reference."""
import json
import os

import numpy as np
import pytest
import torch

import leftrefill_amd.dropin as dropin

dropin.install()
from leftrefill_amd import nvsprep  # noqa: E402
from leftrefill_amd.dropin.dataloaders.obj_nvs_dataset import NVS_OBJDataset  # noqa: E402
from tools import make_golden_nvs_dataset as G  # noqa: E402

S = G.S
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "nvs_dataset.npz")


class Fixture:
    """The loaded file, its tree written under `root`, and the recorded settings."""

    def __init__(self, root):
        self.root, self.fx = str(root), np.load(GOLDEN)
        G.write_tree(self.root, self.fx)
        self.spec = json.loads(str(self.fx["spec"]))

    def golden(self, name):
        kwargs = self.spec["settings"][name][0]
        items = G.unpack_items(*(self.fx[f"{name}/{k}"] for k in ("levels", "mask_levels", "rel_pose", "txt")), G.ref_white(kwargs))
        return items, tuple(self.fx[f"{name}/next"])

    def run(self, name, **extra):
        """The recorded sequence of a setting through the drop-in: (items, next random.random(), next np.random.random())."""
        kwargs, seed, indices = self.spec["settings"][name]
        return G.run_sequence(NVS_OBJDataset, kwargs, seed, indices, self.root, **extra)


@pytest.fixture(scope="module")
def fixture(tmp_path_factory):
    return Fixture(tmp_path_factory.mktemp("nvs_tree"))


def same_item(got, want, what):
    for k in ("image", "masked_image", "mask"):
        assert got[k].dtype == np.float32 and got[k].shape == want[k].shape, (what, k, got[k].dtype, got[k].shape)
        assert got[k].tobytes() == want[k].tobytes(), (what, k, int((got[k] != want[k]).sum()))
    assert got["rel_pose"].dtype == torch.float32 and np.array_equal(got["rel_pose"].numpy(), want["rel_pose"]), what
    txt = [str(t) for t in got["txt"]] if isinstance(got["txt"], (list, tuple)) else str(got["txt"])
    assert txt == want["txt"], (what, txt, want["txt"])


def test_the_fixture_reaches_every_branch_of_the_reference():
    fx = np.load(GOLDEN)
    spec = json.loads(str(fx["spec"]))
    assert set(spec["branch_tally"]) == set(G.BRANCH_LINES.values()) and min(spec["branch_tally"].values()) > 0
    assert os.path.getsize(GOLDEN) < os.path.getsize(os.path.join(ROOT, "tests", "golden", "pair_datasets.npz"))
    want = G.make_inputs()      # the inputs regenerate from the seed
    assert all(np.array_equal(fx[k], v) for k, v in want.items())


@pytest.mark.parametrize("name", sorted(G.SETTINGS))
def test_items_are_the_references(fixture, name):
    want, nxt = fixture.golden(name)
    got, *got_next = fixture.run(name)
    assert len(got) == len(want)
    for n, (g, w) in enumerate(zip(got, want)):
        same_item(g, w, f"{name}[{n}]")
    assert tuple(got_next) == nxt, "the sequence drew another number of values than the reference"


@pytest.mark.parametrize("name", sorted(G.SETTINGS))
def test_raw_plans_execute_to_the_same_items(fixture, name):
    want, nxt = fixture.golden(name)
    got, *got_next = fixture.run(name, raw=True)
    assert tuple(got_next) == nxt
    for n, ((plan, raw), w) in enumerate(zip(got, want)):
        assert set(plan) == {"img_size", "mode", "k", "plane", "ref_white", "rel_pose", "txt"} and plan["mode"] in nvsprep.MODES
        assert all(r.dtype == np.uint8 for r in raw) and raw[0].shape[2] == raw[1].shape[2] == 4 and len(plan["rel_pose"]) == 4
        assert (plan["plane"] is None) == (len(raw) == 2) and (plan["plane"] is None or raw[2].shape == (S, S))
        if plan["mode"] == "alpha":
            assert set(np.unique(raw[2])) <= {0, 1}
        same_item(nvsprep.run_nvs_plan_numpy(plan, raw), w, f"{name}[{n}]")


def test_the_recorded_plans_cover_every_mode(fixture):
    seen = set()
    for name in G.SETTINGS:
        for plan, raw in fixture.run(name, raw=True)[0]:
            path = {(S, S): "copy", (2 * S, 2 * S): "box"}.get(raw[1].shape[:2], "bilinear")
            seen.add((plan["mode"], plan["ref_white"]))
            seen.add(path)
            if plan["mode"] == "alpha":
                seen.add("k even" if plan["k"] % 2 == 0 else "k odd")
    assert seen >= {("alpha", False), ("alpha", True), ("ones", False), ("ones", True), ("file", False), ("file", True), "copy", "box",
                    "bilinear", "k even", "k odd"}, seen


def test_the_composite_needs_no_arithmetic():
    x = np.arange(256, dtype=np.uint8)
    assert np.array_equal(((x / 255.) * 255.).astype(np.uint8), x)
    rgba = np.random.RandomState(0).randint(0, 256, (9, 7, 4), dtype=np.uint8)
    rgba[::2, ::3, 3] = 0
    ref = rgba / 255.      # the reference's statement, channel order aside
    ref[ref[:, :, -1] == 0.] = [1., 1., 1., 1.]
    assert np.array_equal(nvsprep.composite_white(rgba), (ref[:, :, :3] * 255.).astype(np.uint8))
    for v in range(256):      # the file mask: the float32 of the double quotient is the float32 quotient
        assert np.float32(v / 255.) == np.float32(v) / np.float32(255)


def test_ellipse_spans_against_the_literal_tables():
    assert nvsprep.ellipse_spans(8).tolist() == [[4, 5], [1, 8], [1, 8], [0, 8], [0, 8], [0, 8], [1, 8], [1, 8]]
    assert nvsprep.ellipse_spans(5).tolist() == [[2, 3], [0, 5], [0, 5], [0, 5], [2, 3]]
    assert nvsprep.ellipse_spans(1).tolist() == [[0, 1]] and nvsprep.ellipse_spans(2).tolist() == [[1, 2], [0, 2]]
    for k in range(1, nvsprep.MAX_DILATE + 1):
        sp = nvsprep.ellipse_spans(k)
        assert (sp[:, 0] < sp[:, 1]).all() and (sp[:, 1] <= k).all() and sp[k // 2].tolist() == [0, k]


def test_resize_linear_against_literal_values():
    rng = np.random.RandomState(1)
    img = rng.randint(0, 256, (8, 8, 3), dtype=np.uint8)
    assert np.array_equal(nvsprep.resize_linear_u8(img, 8), img)
    box = nvsprep.resize_linear_u8(img, 4)
    v = img.astype(np.int64)
    assert box[1, 2, 0] == (v[2, 4, 0] + v[2, 5, 0] + v[3, 4, 0] + v[3, 5, 0] + 2) >> 2
    # 6 -> 4 on one axis: scale 1.5, f = (d + 0.5) 1.5 - 0.5 = 0.25, 1.75, 3.25, 4.75 -> taps (0, 1), (1, 2), (3, 4), (4, 5)
    s0, s1, a0, a1 = nvsprep.linear_taps(6, 4)
    assert s0.tolist() == [0, 1, 3, 4] and s1.tolist() == [1, 2, 4, 5] and a0.tolist() == [1536, 512, 1536, 512] and a1.tolist() == [512, 1536, 512, 1536]
    s0, s1, a0, a1 = nvsprep.linear_taps(5, 4)
    assert (a0 + a1 == 2048).all() and s1.max() == 4
    flat = np.full((6, 5, 3), 200, np.uint8)      # a constant image stays constant through the fixed-point passes
    assert (nvsprep.resize_linear_u8(flat, 4) == 200).all()
    col = np.zeros((6, 6, 3), np.uint8)
    col[:, 1] = 255      # by hand: R = 255 * 512 = 130560 in every row; ((1536 * (R >> 4)) >> 16) + ((512 * (R >> 4)) >> 16) = 191 + 63; (254 + 2) >> 2 = 64
    assert nvsprep.resize_linear_u8(col, 4)[0, 0, 0] == 64
    with pytest.raises(NotImplementedError):
        nvsprep.resize_linear_u8(img, 9)


def test_occupancy_taps():
    for n, s in ((64, 32), (32, 32), (96, 32)):      # integer scales: the exact block
        first, last = nvsprep.area_taps(n, s)
        assert first.tolist() == [d * (n // s) for d in range(s)] and last.tolist() == [(d + 1) * (n // s) - 1 for d in range(s)]
    first, last = nvsprep.area_taps(48, 32)      # scale 1.5: cells [0, 1], [1, 2], [3, 4], [4, 5], ...
    assert first[:4].tolist() == [0, 1, 3, 4] and last[:4].tolist() == [1, 2, 4, 5]
    for n, s in ((48, 32), (40, 32), (30, 12), (26, 12), (100, 7)):      # every source cell is under some tap; runs are ordered
        first, last = nvsprep.area_taps(n, s)
        assert first[0] == 0 and last[-1] == n - 1 and (first <= last).all() and (first[1:] <= last[:-1] + 1).all()
    alpha = np.zeros((48, 40), np.uint8)
    alpha[47, 39] = 1
    occ = nvsprep.occupancy(alpha, 32)
    assert occ.sum() == 1 and occ[31, 31]
    rows, cols = nvsprep.alpha_lines(alpha, 32)
    assert np.array_equal(rows, occ.any(axis=1)) and np.array_equal(cols, occ.any(axis=0))


@pytest.mark.parametrize("k", [1, 2, 3, 8, 25, 32])
def test_the_box_formula_against_a_brute_force_dilation(k):
    rng = np.random.RandomState(k)
    sp = nvsprep.ellipse_spans(k)
    for trial in range(12):
        H, W = rng.randint(20, 41, size=2)
        m = np.zeros((H, W), bool)
        if trial < 4:      # single pixels in the corners and on the borders
            m[[0, H - 1, 0, H // 2][trial], [0, W - 1, W - 1, 0][trial]] = True
        else:
            m[rng.randint(0, H, 3), rng.randint(0, W, 3)] = True
        brute = np.zeros((H, W), bool)      # the definition, pixel by pixel
        for y in range(H):
            for x in range(W):
                for e in range(k):
                    yy = y + e - k // 2
                    if 0 <= yy < H and m[yy, max(0, x + sp[e, 0] - k // 2):max(0, x + sp[e, 1] - k // 2)].any():
                        brute[y, x] = True
        assert np.array_equal(nvsprep.dilate(m, k), brute)
        ys, xs = np.where(brute)
        assert nvsprep.dilated_box(m.any(axis=1), m.any(axis=0), k) == (ys.min(), ys.max(), xs.min(), xs.max())


def test_a_render_smaller_than_img_size_is_refused(fixture):
    kwargs = dict(G.resolve(fixture.spec["settings"]["train_enlarge"][0], fixture.root), img_size=40)
    ds = NVS_OBJDataset(**kwargs)
    assert ds[0]["image"].shape == (40, 80, 3)      # 64 x 64 renders
    with pytest.raises(NotImplementedError):
        ds[2]      # 32 x 32 renders
    with pytest.raises(NotImplementedError):
        NVS_OBJDataset(raw=True, **dict(kwargs, img_size=44))[1]      # 48 x 40: narrower only


def test_a_one_pixel_box_raises_as_the_reference_does(tmp_path):
    from PIL import Image
    rgba = np.zeros((16, 16, 4), np.uint8)
    rgba[5, 5, 3] = 255
    os.makedirs(str(tmp_path / "o"))
    for v in range(2):
        Image.fromarray(rgba).save(str(tmp_path / "o" / f"{v:03d}.png"))
        np.save(str(tmp_path / "o" / f"{v:03d}.npy"), np.eye(3, 4))
    (tmp_path / "list.txt").write_text("o\n")
    ds = NVS_OBJDataset(str(tmp_path), str(tmp_path / "list.txt"), img_size=16, nviews=2, dilate_size=[1, 1], **G.SP)
    with pytest.raises(ValueError, match="low >= high"):
        ds[0]


def test_collate_nvs_raw(fixture):
    items, *_ = fixture.run("train_enlarge", raw=True)
    batch = nvsprep.collate_nvs_raw(items, pin=False)
    jobs = nvsprep.job_table(batch)
    assert batch["batch"] == len(items) == len(jobs) and batch["img_size"] == S and batch["arena"].numel() % 16 == 0
    assert batch["rel_pose"].shape == (len(items), 4) and batch["rel_pose"].dtype == torch.float32
    assert list(batch["txt"]) == [p["txt"] for p, _ in items]
    arena = batch["arena"].numpy()
    for b, (plan, raw) in enumerate(items):
        jb = jobs[b]
        assert jb["sample"] == b and jb["mode"] == nvsprep.MODES[plan["mode"]] and jb["flags"] == 0
        for name, arr in (("cond", raw[0]), ("target", raw[1])):
            o = int(jb[name + "_off"])
            assert o % 16 == 0 and (jb[name + "_h"], jb[name + "_w"]) == arr.shape[:2] and np.array_equal(arena[o:o + arr.size], arr.reshape(-1))
        if plan["mode"] == "alpha":
            o = int(jb["plane_off"])
            assert o % 16 == 0 and np.array_equal(arena[o:o + S * S], raw[2].reshape(-1)) and jb["k"] == plan["k"]
            assert np.array_equal(np.stack([jb["lo"][:plan["k"]], jb["hi"][:plan["k"]]], axis=1), nvsprep.ellipse_spans(plan["k"]))
        else:
            assert jb["plane_off"] == -1 and jb["k"] == 0
    with pytest.raises(TypeError, match="raw=True"):
        nvsprep.collate_nvs_raw([fixture.run("val_complete")[0][0]])


def test_header_binding_and_source_list_agree_on_the_new_symbol():
    import abi_helpers as abi
    from leftrefill_amd import _lib, build
    assert len(abi.c_params("lr_nvs_prep")) == 10
    assert "nvs_prep.hip" in build.SOURCES and _lib.ABI_VERSION == 30
    assert "lr_abi_version(void) { return 30; }" in open(os.path.join(ROOT, "leftrefill_amd", "csrc", "elementwise.hip")).read()
    for name, value in (("MODE_ALPHA", nvsprep.ALPHA), ("MODE_ONES", nvsprep.ONES), ("MODE_FILE", nvsprep.FILE), ("REF_WHITE", nvsprep.REF_WHITE),
                        ("MAX_SIZE", nvsprep.MAX_SIZE), ("MAX_DILATE", nvsprep.MAX_DILATE)):
        assert abi.define(f"LR_NVS_{name}") == value, name


def test_the_drop_in_name_steps_aside_for_another_trees_module(tmp_path, monkeypatch):
    import importlib
    import sys

    def forget():
        for name in [n for n in sys.modules if n == "dataloaders" or n.startswith("dataloaders.")]:
            monkeypatch.delitem(sys.modules, name)

    name = "obj_nvs_dataset"
    monkeypatch.setattr(sys, "path", [p for p in sys.path if not os.path.isfile(os.path.join(p or os.getcwd(), "dataloaders", name + ".py"))])
    forget()
    root = dropin.install()
    mod = importlib.import_module("dataloaders." + name)
    assert mod.__file__.startswith(root) and "raw" in mod.NVS_OBJDataset.__init__.__code__.co_varnames
    other = tmp_path / "tree" / "dataloaders"
    other.mkdir(parents=True)
    (other / (name + ".py")).write_text("MARK = 'their own'\n")
    monkeypatch.syspath_prepend(str(tmp_path / "tree"))
    forget()
    dropin.install()
    assert importlib.import_module("dataloaders." + name).MARK == "their own"
    assert importlib.import_module("leftrefill_amd.dropin.dataloaders." + name).NVS_OBJDataset is NVS_OBJDataset
    forget()


def test_nvsldm_loaders_and_mask_warmup(fixture):
    """NVSLDM.train_dataloader / val_dataloader (reference NVS_ldm.py:348-372) build the dataset from cfg and data_cfg; the DTU branches
    raise; on_train_batch_end ramps the dataset's complete_mask_rate over warmup_mask_steps (299-306)."""
    from types import SimpleNamespace
    from inpainting_ldm.NVS_ldm import NVSLDM
    m = NVSLDM.__new__(NVSLDM)
    torch.nn.Module.__init__(m)
    m.cfg = dict(datapath=os.path.join(fixture.root, "objects"), train_list=os.path.join(fixture.root, "train.txt"),
                 val_list=os.path.join(fixture.root, "val.txt"), batch_size=2)
    m.data_cfg = dict(obj_dataset=True, warping_based=False, nviews=G.NVIEWS, pts_size=[3, 6], width_range=[32, 96], dilate_size=[3, 9],
                      complete_mask_rate=0.2, warmup_mask_steps=4, cfg=2.5, **G.SP)
    m.img_size, m.mask_steps, m.warmup_mask_steps, m.complete_mask_rate = S, 0, 4, 0.2
    train = m.train_dataloader(num_workers=0)
    assert isinstance(train.dataset, NVS_OBJDataset) and train.dataset.mode == "train" and train.batch_size == 2 and not train.dataset.raw
    batch = next(iter(train))
    assert batch["image"].shape == (2, S, 2 * S, 3) and batch["rel_pose"].shape == (2, 4) and batch["mask"].dtype == torch.float32
    val = m.val_dataloader(num_workers=0, batch_size=4)
    assert val.dataset.mode == "val" and val.drop_last and len(val) == 1 and next(iter(val))["image"].shape == (4, S, 2 * S, 3)
    raw = m.train_dataloader(raw=True, num_workers=0)
    assert raw.dataset.raw and raw.collate_fn is nvsprep.collate_nvs_raw and next(iter(raw))["arena"].dtype == torch.uint8
    m.trainer = SimpleNamespace(train_dataloader=train)
    rates = []
    for _ in range(7):
        m.on_train_batch_end()
        rates.append(train.dataset.complete_mask_rate)
    assert rates[:5] == [0.2, 0.2 + 0.25 * 0.8, 0.2 + 0.5 * 0.8, 0.2 + 0.75 * 0.8, 1.0] and rates[5:] == [1.0, 1.0] and m.mask_steps == 5
    m.data_cfg["obj_dataset"] = False
    with pytest.raises(NotImplementedError):
        m.train_dataloader()
    with pytest.raises(NotImplementedError):
        m.val_dataloader()
