"""tests/golden/pair_datasets.npz: the reference's image-pair datasets and sampler, run by the reference's own control flow.  CPU only.

    python tools/make_golden_pair_datasets.py --reference DIR

The reference's dataloaders/inpainting_crossview_dataset.py imports OpenCV, which is absent here.  This tool puts a small functional
stand-in into sys.modules["cv2"] -- `imread` through PIL, `cvtColor` reversing the channels, `resize` dispatching to this project's
`resize_area_hw` / `resize_nearest` -- and imports the reference module by path.  So the draw order and count, every branch decision,
the match-mask geometry and its PIL rasterisation, left / right placement, flips and sampler orders in the file are the reference's;
only the OpenCV primitives are restated.

It builds a small seeded tree in a temporary directory (`write_tree`, which the tests use to rebuild it from the file): two scenes
of PNG images of mixed shapes, all at least S = 32 on both sides and free of rounding ties at every size a plan can ask for;
irregular and segmentation masks with their list files; match pickles of every kind (`MATCH_KINDS`); val pair folders with and without
mask.png; multi-view folders.  Recorded: the input arrays and the layout; for each of SETTINGS the finished items of a seeded
sequence and the next random.random() / np.random.random() after it (which pins the draw count); sampler orders of epochs 0, 1, 2
iterated in sequence for SAMPLER_SPLITS; multi-view val items for MV_SETTINGS; the tally of reference branches hit (asserted
complete: `BRANCH_LINES`).

An item is stored as uint8 levels and packed mask bits; the tool asserts that this loses nothing: image == levels / 127.5 - 1 in
float32, mask in {0, 1}, masked_image == image * (mask < 0.5) (`unpack_items` restores them with those expressions).
"""
import argparse
import json
import os
import pickle
import sys
import tempfile
import types

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from tools.golden_common import branch_tally, import_reference, resolve, run_sequence  # noqa: E402, F401  (the tests reach them as G.*)
OUT = os.path.join(ROOT, "tests", "golden", "pair_datasets.npz")
S = 32
TOKEN_MAP = dict(left_token="<left>", right_token="<right>", task_token="<views>", real_token="<scene>")
SP = dict(repeat_sp_token=3, sp_token="<special-token>")

# (h, w) of the image pool; the scene of the nine training images; (source, target) of the training pairs, index = match file number
POOL = [(40, 57), (61, 44), (33, 70), (52, 52), (47, 96), (130, 64), (36, 41), (75, 50), (44, 44), (58, 83), (32, 49), (66, 39)]
SCENES = ["0001"] * 5 + ["0002"] * 4
PAIRS = [(0, 1), (1, 2), (2, 3), (3, 4), (4, 0), (5, 6), (6, 7), (7, 8), (8, 5)]
MATCH_KINDS = {0: "spread", 1: "compact", 2: "missing", 3: "few", 4: "flat", 5: "corners", 6: "spread", 7: "compact", 8: "spread"}
TRAIN = dict(image_path="@image_dict.pkl", pair_path="@pairs.pkl", mask_path=["@irregular.txt", "@segment.txt"], mode="train", img_size=S)
SETTINGS = {      # name -> (constructor keywords, seed, item indices)
    "mixed": (dict(TRAIN, flip=True, view_mask_rate=0.5, match_mask=True, match_mask_rate=0.6, match_path="@match", token_map=TOKEN_MAP),
              11, list(range(9)) * 2),
    "match_right": (dict(TRAIN, constant_place=True, view_mask_rate=0.0, match_mask=True, match_mask_rate=1.0, match_path="@match", **SP),
                    12, list(range(9))),
    "match_any": (dict(TRAIN, view_mask_rate=0.0, match_mask=True, match_mask_rate=1.0, match_path="@match", flip=True, **SP),
                  13, [0, 1, 6, 7, 8, 0, 1, 6]),
    "only_mask_image": (dict(TRAIN, only_mask_image=True, flip=True, **SP), 14, [0, 3, 5, 8, 2, 6]),
    "random_masks": (dict(TRAIN, view_mask_rate=0.0, flip=True, deep_prompt=True, **SP), 15, [1, 2, 4, 6, 7, 3, 0, 5]),
    "val": (dict(image_path="@val", pair_path=None, mask_path="@val_masks", mode="val", img_size=S, test_limit=4, token_map=TOKEN_MAP),
            16, [0, 1, 2, 3]),
}
SAMPLER_SPLITS = [(0, 1), (0, 2), (1, 2), (1, 4), (2, 4)]      # (rank, num_replicas); 2 scenes x 3 = 6 samples: 4 does not divide them
N_SAMPLE_PER_SCENE = 3
MV = dict(image_path="@mv", pair_path=None, mask_path="@val_masks", mode="val", img_size=S, test_limit=2, view_token_len=2, **SP)
MV_SETTINGS = {
    "mv_plain_v4": (dict(MV, view_num=4), 21, [0, 1]),
    "mv_concat_v3": (dict(MV, view_num=3, concat_target=True), 22, [0, 1]),
    "mv_concat_v4_shuffled": (dict(MV, view_num=4, concat_target=True, source_shuffle=True), 23, [0, 1]),
    "mv_plain_v2": (dict(MV, view_num=2), 24, [1]),
}
# reference line -> branch name: every one must be executed by the recorded sequences
BRANCH_LINES = {104: "match: no file", 135: "match: no crop record", 137: "match: crop record", 148: "match: fewer than 10 points",
                159: "match: zero area", 165: "match: window (rate < 1)", 175: "match: all points (rate >= 1)",
                178: "match: fewer than 10 picked", 194: "match: left", 196: "match: right", 203: "mask: irregular", 207: "mask: segment",
                211: "mask: sum", 225: "mask: left", 227: "mask: right", 312: "placement: target left", 315: "placement: target right",
                322: "only_mask_image: left", 324: "only_mask_image: right", 333: "view mask: left", 335: "view mask: right",
                351: "flip: left half", 355: "flip: right half", 338: "val: the pair's mask.png", 340: "val: cycled mask list"}


# ---- the tree -----------------------------------------------------------------------------------------------------------------------
def _area_f64(img, rh, rw):
    from leftrefill_amd.dropin.dataloaders.test_dataset import _area_weights
    h, w = img.shape[:2]
    if (h, w) == (rh, rw):
        return img.astype(np.float64)
    out = np.einsum("ih,hwc->iwc", _area_weights(h, rh), img.astype(np.float64))
    return np.einsum("jw,iwc->ijc", _area_weights(w, rw), out)


def plan_sizes(h, w, size=S):
    """The (rh, rw) a training plan can ask of an h x w image: the direct resize and the crop branch."""
    return [(size, size), (size, max(size, int(w * (size / h)))) if h < w else (max(size, int(h * (size / w))), size)]


def near_tie(pre, eps=1e-6):
    return np.abs(pre - np.floor(pre) - 0.5) <= eps


def detie(img, rng, size=S):
    """Flip the low bit of a source pixel under every output within 1e-6 of a rounding tie, at both sizes, until none is.  The pixel is
    drawn among those the output covers: a fixed choice can trade a tie at one size for one at the other for ever."""
    img = img.copy()
    h, w = img.shape[:2]
    for _ in range(200):
        clean = True
        for rh, rw in plan_sizes(h, w, size):
            for i, j, c in np.argwhere(near_tie(_area_f64(img, rh, rw))):
                y = rng.randint(int(i * h / rh), min(h, int(np.ceil((i + 1) * h / rh))))
                x = rng.randint(int(j * w / rw), min(w, int(np.ceil((j + 1) * w / rw))))
                img[y, x, c] ^= 1
                clean = False
        if clean:
            return img
    raise AssertionError("ties left")


def make_inputs():
    """Arrays and layout of the tree, seeded."""
    rng = np.random.RandomState(2024)
    fx = {}
    for k, (h, w) in enumerate(POOL):
        fx[f"pool_{k}"] = detie(rng.randint(0, 256, (h, w, 3), dtype=np.uint8), rng)
    levels = np.array([0, 0, 0, 100, 127, 128, 200, 255, 255, 255], dtype=np.uint8)
    for kind, shapes in (("irregular", [(45, 50), (64, 40), (20, 27)]), ("segment", [(33, 33), (70, 91), (25, 60)]),
                         ("valmask", [(48, 48), (37, 59)])):
        for k, (h, w) in enumerate(shapes):      # blocky, so the nearest gather sees runs; a few grey levels around the threshold
            coarse = rng.choice(levels, size=(-(-h // 6), -(-w // 6)))
            fx[f"{kind}_{k}"] = np.kron(coarse, np.ones((6, 6), np.uint8))[:h, :w].copy()
    png = {f"scenes/{SCENES[k]}/imgs/{k}.png": f"pool_{k}" for k in range(len(SCENES))}
    lists = {}
    for kind in ("irregular", "segment"):
        names = [f"masks/{kind}_{k}.png" for k in range(3)]
        png.update({n: f"{kind}_{k}" for k, n in enumerate(names)})
        lists[f"{kind}.txt"] = names[::-1]      # unsorted in the file: the datasets sort by file name
    for k in range(2):
        png[f"val_masks/m{k}.png"] = f"valmask_{k}"
    for i, (s, t) in enumerate([(9, 10), (10, 11), (11, 3), (0, 9)]):      # val pairs; the even ones carry their own mask
        png[f"val/pair_{i}/source.png"], png[f"val/pair_{i}/target.png"] = f"pool_{s}", f"pool_{t}"
        if i % 2 == 0:
            png[f"val/pair_{i}/mask.png"] = f"segment_{i // 2}"
    for name, own, members in (("3", True, (9, 10, 11, 6, 8)), ("12", False, (1, 3, 0, 7, 2))):      # multi-view folders, named by number
        for stem, k in zip(("target", "source", "source_1", "source_2", "source_3"), members):
            png[f"mv/{name}/{stem}.png"] = f"pool_{k}"
        if own:
            png[f"mv/{name}/mask.png"] = "irregular_0"
    pkl = {}
    for idx, kind in MATCH_KINDS.items():
        if kind == "missing":
            continue
        n = 80
        if kind == "compact":
            p0, p1 = rng.uniform(300, 600, (n, 2)), rng.uniform(280, 560, (n, 2))
        elif kind == "corners":
            corner = np.repeat(np.array([[10, 10], [820, 10], [10, 820], [820, 820]], dtype=np.float64), 6, axis=0)
            p0, p1 = corner + rng.uniform(0, 8, corner.shape), corner + rng.uniform(0, 8, corner.shape)
        else:
            p0, p1 = rng.uniform(5, 827, (n, 2)), rng.uniform(5, 827, (n, 2))
        scores = rng.uniform(0.85, 1.0, len(p0))
        if kind == "few":
            scores[6:] = rng.uniform(0.1, 0.5, len(p0) - 6)
            scores[0] = 1.0
        if kind == "flat":
            p0[:, 0], p1[:, 0] = 400.0, 300.0
        fx[f"match_{idx}_mkpts0"], fx[f"match_{idx}_mkpts1"] = p0.astype(np.float32), p1.astype(np.float32)
        fx[f"match_{idx}_scores"] = scores.astype(np.float32)
        pkl[f"match/{idx:08d}.pkl"] = f"match_{idx}"
    fx["layout"] = np.array(json.dumps(dict(png=png, lists=lists, pkl=pkl, pairs=PAIRS,
                                            image_dict={str(k): f"scenes/{SCENES[k]}/imgs/{k}.png" for k in range(len(SCENES))})))
    return fx


def write_tree(root, fx):
    """Write the tree the arrays and the `layout` of `fx` (the tool's inputs, or the loaded fixture) describe under `root`."""
    from PIL import Image
    layout = json.loads(str(fx["layout"]))
    for rel, key in layout["png"].items():
        os.makedirs(os.path.dirname(os.path.join(root, rel)), exist_ok=True)
        Image.fromarray(np.asarray(fx[key])).save(os.path.join(root, rel))
    for rel, key in layout["pkl"].items():
        os.makedirs(os.path.dirname(os.path.join(root, rel)), exist_ok=True)
        with open(os.path.join(root, rel), "wb") as f:
            pickle.dump({k: np.asarray(fx[f"{key}_{k}"]) for k in ("mkpts0", "mkpts1", "scores")}, f)
    for rel, names in layout["lists"].items():
        with open(os.path.join(root, rel), "w") as f:
            f.write("".join(os.path.join(root, n) + "\n" for n in names))
    with open(os.path.join(root, "image_dict.pkl"), "wb") as f:
        pickle.dump({int(k): os.path.join(root, v) for k, v in layout["image_dict"].items()}, f)
    with open(os.path.join(root, "pairs.pkl"), "wb") as f:
        pickle.dump([dict(source=s, target=t) for s, t in layout["pairs"]], f)


# ---- items <-> arrays ---------------------------------------------------------------------------------------------------------------
def pack_items(items):
    """uint8 levels, packed mask bits and JSON prompts of finished items, after asserting that this loses nothing."""
    levels, bits = [], []
    for it in items:
        image, mask, masked = np.asarray(it["image"]), np.asarray(it["mask"]), np.asarray(it["masked_image"])
        u8 = np.rint((image.astype(np.float64) + 1.0) * 127.5).astype(np.uint8)
        f32 = u8.astype(np.float32) / 127.5 - 1.0
        assert np.array_equal(f32, image) and np.array_equal(image.astype(np.float32), image), "image is not levels / 127.5 - 1 in float32"
        assert np.isin(mask, (0.0, 1.0)).all() and np.array_equal(masked, f32 * (mask < 0.5)), "mask / masked_image"
        levels.append(u8)
        bits.append(np.packbits(mask.astype(np.uint8).reshape(-1)))
    txt = [[str(t) for t in it["txt"]] if isinstance(it["txt"], (list, tuple)) else str(it["txt"]) for it in items]
    return np.stack(levels), np.stack(bits), json.dumps(txt)


def unpack_items(levels, bits, txt):
    """The float32 items `pack_items` stored: image = levels / 127.5 - 1, mask from its bits, masked_image = image * (mask < 0.5)."""
    items = []
    for u8, b, t in zip(levels, bits, json.loads(str(txt))):
        image = u8.astype(np.float32) / 127.5 - 1.0
        mask = np.unpackbits(b)[:u8[..., 0].size].reshape(u8.shape[:-1] + (1,)).astype(np.float32)
        items.append(dict(image=image, mask=mask, masked_image=image * (mask < 0.5), txt=t))
    return items


# ---- the reference ------------------------------------------------------------------------------------------------------------------
def cv2_standin():
    from PIL import Image
    from leftrefill_amd.dataprep import resize_area_hw
    from leftrefill_amd.dropin.dataloaders.test_dataset import resize_nearest
    cv2 = types.ModuleType("cv2")
    cv2.IMREAD_GRAYSCALE, cv2.IMREAD_COLOR, cv2.COLOR_BGR2RGB, cv2.INTER_NEAREST, cv2.INTER_AREA = 0, 1, 4, 0, 3

    def imread(path, flag=1):
        if flag == cv2.IMREAD_GRAYSCALE:
            return np.array(Image.open(path).convert("L"))
        return np.array(Image.open(path).convert("RGB"))[:, :, ::-1].copy()      # BGR

    def resize(img, dsize, interpolation=None):
        w, h = dsize
        if interpolation == cv2.INTER_AREA:
            return resize_area_hw(img, h, w)
        assert interpolation == cv2.INTER_NEAREST and w == h
        return resize_nearest(img, w)

    cv2.imread, cv2.resize, cv2.cvtColor = imread, resize, lambda img, code: img[:, :, ::-1].copy()
    return cv2


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reference", default=os.environ.get("LEFTREFILL_REFERENCE"), help="checkout of the reference project")
    ap.add_argument("--out", default=OUT)
    a = ap.parse_args()
    if not a.reference:
        raise SystemExit("give --reference DIR (or LEFTREFILL_REFERENCE)")
    ref, ref_file = import_reference(a.reference, "inpainting_crossview_dataset", cv2_standin())
    fx = make_inputs()
    out = dict(fx)
    with tempfile.TemporaryDirectory() as root:
        write_tree(root, fx)
        with branch_tally(ref_file, BRANCH_LINES) as tally:
            for name, (kwargs, seed, indices) in SETTINGS.items():
                items, nxt, np_nxt = run_sequence(ref.InpaintingCrossViewDataset, kwargs, seed, indices, root)
                assert all(it["image"].shape == (S, 2 * S, 3) and it["image"].dtype == np.float32 for it in items)
                out[f"{name}/levels"], out[f"{name}/mask_bits"], out[f"{name}/txt"] = pack_items(items)
                out[f"{name}/next"] = np.array([nxt, np_nxt])
        for name, (kwargs, seed, indices) in MV_SETTINGS.items():
            items, nxt, np_nxt = run_sequence(ref.InpaintingMultiViewDataset, kwargs, seed, indices, root)
            out[f"{name}/levels"], out[f"{name}/mask_bits"], out[f"{name}/txt"] = pack_items(items)
            out[f"{name}/idx"] = np.array([it["idx"] for it in items])
            out[f"{name}/next"] = np.array([nxt, np_nxt])
        with open(os.path.join(root, "image_dict.pkl"), "rb") as f:
            image_dict = pickle.load(f)
        with open(os.path.join(root, "pairs.pkl"), "rb") as f:
            pairs = pickle.load(f)
        for rank, replicas in SAMPLER_SPLITS:
            sampler = ref.BalancedRandomSampler(image_dict, pairs, n_sample_per_scene=N_SAMPLE_PER_SCENE, rank=rank, num_replicas=replicas)
            orders = []
            for epoch in range(3):
                sampler.set_epoch(epoch)
                orders.append(list(sampler))
            out[f"sampler/{rank}_{replicas}"] = np.array(orders)
    missed = [name for name, n in tally.items() if n == 0]
    assert not missed, f"branches the sequences never took: {missed}"
    spec = dict(settings=SETTINGS, mv_settings=MV_SETTINGS, sampler_splits=SAMPLER_SPLITS, n_sample_per_scene=N_SAMPLE_PER_SCENE,
                match_kinds={str(k): v for k, v in MATCH_KINDS.items()}, branch_tally=tally)
    out["spec"] = np.array(json.dumps(spec))
    np.savez_compressed(a.out, **out)
    print(json.dumps(tally, indent=1))
    print(f"wrote {a.out}: {os.path.getsize(a.out) / 1024:.0f} KiB")


if __name__ == "__main__":
    main()
