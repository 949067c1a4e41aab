"""Batch assembly from raw decoded images: the per-sample decisions as a plan of plain scalars, its execution on the host in numpy
(`run_plan_numpy`, the yardstick) and on the device (`collate_raw` + `DevicePrep`: one arena copy, one job-table copy, one
`lr_batch_prep` launch per batch, csrc/batch_prep.hip).  The arena packer, the buffer policy, the uploads and the loader wiring are
rawbatch.py's, shared with nvsprep.py.

A plan is `{"img_size": S, "tiles": [tile, ...], "txt": prompt}`; the canvas is `len(tiles)` tiles of S x S side by side (the
single-image training sample has one, the evaluation canvas [source | target] two).  A tile is

    image         index of the uint8 [h, w, 3] source in the sample's `raw` list
    rh, rw        size the source is area-resized to;  y0, x0: origin of the S x S window kept of that
    flip          left-right flip of the window
    masks         indices of up to two uint8 [h, w] mask sources in `raw` (nearest-resized to S, summed, clipped, 1 where > 127)
    mask_flip     left-right flip of the mask, independent of `flip`
    outpaint_col  >= 0: the mask is 1 from this column on (no mask source);  zero_mask: the mask is all zero

The device takes shrinking and identity resizes; a tile that enlarges its source on either axis (INTER_AREA is a different filter
there, and `resize_area` states only its own formula for it) or whose window is wider than the kernel's row buffer sends its whole
sample through `run_plan_numpy`, and `DevicePrep` copies the finished sample in (it warns once).

A multi-view plan carries several canvases instead: `{"img_size": S, "views": [[tile, ...], ...], "txt": prompts, "idx": n}`, every
view a canvas of the same number of tiles over the sample's one `raw` list.  `collate_raw` flattens a batch of them to B·V samples of
the job table (a source is still placed once per sample) and `DevicePrep` returns [B, V, S, T·S, C] views of its buffers.

Two masks are summed as integers and clipped to 255 -- what `np.clip(m1 + m2, 0, 255)` says.  (On uint8 arrays numpy wraps that
sum before the clip; masks of {0, 255} give the same result either way after the `> 127` threshold.)
"""
import ctypes
import math
import os
import pickle
import random
import warnings

import numpy as np
import torch

from . import _lib, rawbatch
from .rawbatch import DevicePrepLoader  # noqa: F401  (its home is rawbatch; importable from here as before)
from .dropin.dataloaders.test_dataset import _area_weights, resize_nearest

FLIP_IMAGE, FLIP_MASK, ZERO_MASK, HOST = 1, 2, 4, 8      # LR_PREP_* of include/leftrefill_hip.h
MAX_SIZE, ROW_BYTES = 512, 24576                         # LR_PREP_MAX_SIZE, LR_PREP_ROW_BYTES
JOB_DTYPE = np.dtype(_lib.PrepJob)                       # numpy image of struct lr_prep_job
assert JOB_DTYPE.itemsize == ctypes.sizeof(_lib.PrepJob) == 80


# ---- plans: decisions only, no pixel work -----------------------------------------------------------------------------------------
def plan_tile(image, rh, rw, y0=0, x0=0, flip=False, masks=(), mask_flip=False, outpaint_col=-1, zero_mask=False):
    return dict(image=int(image), rh=int(rh), rw=int(rw), y0=int(y0), x0=int(x0), flip=bool(flip), masks=[int(m) for m in masks],
                mask_flip=bool(mask_flip), outpaint_col=int(outpaint_col), zero_mask=bool(zero_mask))


def plan_resize_train(h, w, size):
    """The training resize (reference dataloaders/inpainting_dataset.py:68-83): with probability 1/2 straight to size x size, else the
    short side to `size`, the long side to max(size, int(long * (size / short))) and a random size x size window.  Draws:
    random.random, then -- second branch only -- random.randint for the window's column, then for its row."""
    if random.random() < 0.5:
        return dict(rh=size, rw=size, y0=0, x0=0)
    if h < w:
        rh, rw = size, max(size, int(w * (size / h)))
    else:
        rh, rw = max(size, int(h * (size / w))), size
    x0 = random.randint(0, rw - size)
    y0 = random.randint(0, rh - size)
    return dict(rh=rh, rw=rw, y0=y0, x0=x0)


def plan_mask_train(n_irregular, n_segment):
    """Which mask files (reference 88-106): `(irregular indices, segment indices)` in the order they are summed.  Draws:
    random.random, then one random.randint (irregular below 0.4, segment below 0.8) or two (segment, then irregular)."""
    rdv = random.random()
    if rdv < 0.4:
        return [("irregular", random.randint(0, n_irregular - 1))]
    if rdv < 0.8:
        return [("segment", random.randint(0, n_segment - 1))]
    first = ("segment", random.randint(0, n_segment - 1))
    return [first, ("irregular", random.randint(0, n_irregular - 1))]


def plan_outpaint_col(size, min_rate, max_rate):
    """First masked column of the outpainting mask (reference 113-118).  Draws: np.random.random."""
    return int((np.random.random() * (max_rate - min_rate) + min_rate) * size)


def plan_flips():
    """(image flip, mask flip) (reference 175-179).  Draws: random.random twice."""
    flip = random.random() < 0.5
    return flip, random.random() < 0.5


def plan_match_mask(match_path, idx, target_pos, target_crop, source_crop, constant_place=False):
    """The matching-based mask (reference dataloaders/inpainting_crossview_dataset.py:100-198): a closed polyline with round joints
    through matched keypoints of the masked view.  `<match_path>/<idx:08d>.pkl` holds `mkpts0` (target), `mkpts1` (source) and `scores`
    in 832-pixel coordinates; a crop record is `dict(w_start, h_start, w, h)` of the crop branch, None for the direct resize.
    Returns `(mask_left, plane)`, the plane uint8 [256, 256] of {0, 255} (the reference draws 1 and never thresholds: the same mask
    after `> 127`), or None -- no file (before any draw), fewer than 10 good points, a degenerate box, fewer than 10 picked points.
    Draws: random.randint(15, 30); random.random for the side unless constant_place (then the right side); random.random for the
    area; under rate < 1 two np.random.randint for the window; np.random.permutation; np.random.randint for the width."""
    from PIL import Image, ImageDraw
    pkl_name = os.path.join(match_path, str(idx).zfill(8) + ".pkl")
    if not os.path.exists(pkl_name):
        return None
    with open(pkl_name, "rb") as f:
        res = pickle.load(f)
    min_width, max_width, min_area_rate, max_area_rate, min_num, match_size, grid = 35, 70, 0.2, 0.5, 10, 832, 256
    num_vertex = random.randint(15, 30)
    mask_left = (1.0 if constant_place else random.random()) < 0.5
    target_side = (target_pos == "left") == mask_left      # the masked half shows the target
    crop = target_crop if target_side else source_crop
    pts = res["mkpts0" if target_side else "mkpts1"][np.where(res["scores"] > res["scores"].max() * 0.8)]
    if crop is None:
        pts = pts / match_size * grid
    else:      # follow the crop: to the resized image, minus the window's origin, then short side -> 256
        pts = pts / match_size
        pts[:, 0] *= crop["w"]
        pts[:, 1] *= crop["h"]
        pts[:, 0] -= crop["w_start"]
        pts[:, 1] -= crop["h_start"]
        pts /= min(crop["w"], crop["h"]) / grid
        pts = pts[(pts[:, 0] >= 0) * (pts[:, 1] >= 0) * (pts[:, 0] < grid) * (pts[:, 1] < grid)]
    if len(pts) < min_num:
        return None
    x_min, x_max, y_min, y_max = pts[:, 0].min(), pts[:, 0].max(), pts[:, 1].min(), pts[:, 1].max()
    good_w, good_h = x_max - x_min, y_max - y_min
    good_area = good_w * good_h
    if good_area == 0:
        return None
    rate = grid * grid * (min_area_rate + (max_area_rate - min_area_rate) * random.random()) / good_area
    rate_1d = math.sqrt(rate)
    if rate < 1:      # a window of that share of the points' box
        a, b = good_w * rate_1d, good_h * rate_1d
        x_start = x_min + np.random.randint(0, good_w - a + 1)
        y_start = y_min + np.random.randint(0, good_h - b + 1)
        temp = pts[np.where(pts[:, 0] > x_start)]
        temp = temp[np.where(temp[:, 0] < x_start + a)]
        temp = temp[np.where(temp[:, 1] > y_start)]
        temp = temp[np.where(temp[:, 1] < y_start + b)]
        picked = np.random.permutation(temp)
    else:
        picked = np.random.permutation(pts)
    if picked.shape[0] < min_num:
        return None
    picked = picked[:num_vertex]
    width = np.random.randint(min_width, max_width)
    plane = Image.new("L", (grid, grid), 0)
    draw = ImageDraw.Draw(plane)
    draw.line(np.append(picked, picked[:1], axis=0), fill=255, width=width)
    for v in picked:
        draw.ellipse((v[0] - width // 2, v[1] - width // 2, v[0] + width // 2, v[1] + width // 2), fill=255)
    return mask_left, np.asarray(plane, np.uint8)


def tile_needs_host(tile, raw, size):
    """True when lr_batch_prep does not take the tile: it enlarges its source, or its window is wider than the kernel's row buffer."""
    h, w = raw[tile["image"]].shape[:2]
    if size > MAX_SIZE or tile["rh"] > h or tile["rw"] > w:
        return True
    rx = w / tile["rw"]
    xa, xb = int(np.floor(tile["x0"] * rx)), min(w, int(np.ceil((tile["x0"] + size) * rx)))
    return (xb - xa) * 3 + 30 > ROW_BYTES


# ---- the host route ---------------------------------------------------------------------------------------------------------------
def resize_area_hw(img, rh, rw):
    """`resize_area` of dataloaders/test_dataset.py for a rectangular target: uint8 [h, w, c] -> uint8 [rh, rw, c], rows first."""
    h, w = img.shape[:2]
    if (h, w) == (rh, rw):
        return img
    out = np.einsum("ih,hwc->iwc", _area_weights(h, rh), img.astype(np.float64))
    out = np.einsum("jw,iwc->ijc", _area_weights(w, rw), out)
    return np.clip(np.rint(out), 0, 255).astype(np.uint8)


def run_tile_numpy(tile, raw, size):
    """One tile on the host: (image float32 [S, S, 3] in [-1, 1], mask float32 [S, S, 1] in {0, 1})."""
    img = resize_area_hw(raw[tile["image"]], tile["rh"], tile["rw"])
    img = img[tile["y0"]:tile["y0"] + size, tile["x0"]:tile["x0"] + size, :]
    if tile["outpaint_col"] >= 0:
        mask = np.zeros((size, size), dtype=np.uint8)
        mask[:, tile["outpaint_col"]:] = 255
    elif tile["zero_mask"]:
        mask = np.zeros((size, size), dtype=np.uint8)
    else:
        total = sum(resize_nearest(raw[m], size).astype(np.int32) for m in tile["masks"])
        mask = (np.clip(total, 0, 255) > 127).astype(np.uint8) * 255
    mask = mask.astype(np.float32) / 255.0
    if tile["flip"]:
        img = img[:, ::-1].copy()
    if tile["mask_flip"]:
        mask = mask[:, ::-1].copy()
    return img.astype(np.float32) / 127.5 - 1.0, mask[:, :, None]


def run_plan_numpy(plan, raw):
    """Execute a plan on the host: the finished sample `dict(image, txt, masked_image, mask)` of the batch contract; a multi-view plan
    gives [V, S, T S, C] arrays and carries its `idx` along."""
    if "views" in plan:
        views = [run_plan_numpy(dict(img_size=plan["img_size"], tiles=tiles, txt=None), raw) for tiles in plan["views"]]
        out = {k: np.stack([v[k] for v in views]) for k in ("image", "masked_image", "mask")}
        return dict(image=out["image"], txt=plan["txt"], masked_image=out["masked_image"], mask=out["mask"], idx=plan["idx"])
    done = [run_tile_numpy(t, raw, plan["img_size"]) for t in plan["tiles"]]
    image = done[0][0] if len(done) == 1 else np.concatenate([d[0] for d in done], axis=1)
    mask = done[0][1] if len(done) == 1 else np.concatenate([d[1] for d in done], axis=1)
    return dict(image=image, txt=plan["txt"], masked_image=image * (mask < 0.5), mask=mask)


def plan_canvases(plan):
    """The canvases of a plan as lists of tiles: its views, or its one canvas."""
    return plan["views"] if "views" in plan else [plan["tiles"]]


# ---- the device route -------------------------------------------------------------------------------------------------------------
def collate_raw(items, pin=None):
    """DataLoader collate_fn for `raw=True` datasets: a list of (plan, raw) -> one byte arena holding every source once, tightly packed
    (so offsets are unaligned), and the lr_prep_job table, one job per tile.  A sample with a tile the kernel does not take is marked
    LR_PREP_HOST and carried along in `host`; `txt` is collated as the DataLoader would.  Multi-view plans (`views`) become B·V samples
    of the table, sample b's view v at index b V + v, over sample b's one set of sources; the batch then carries `views` = V and `idx`.
    pin: keep arena and table in page-locked memory (default: `rawbatch.default_pin`)."""
    from torch.utils.data import default_collate
    pin = rawbatch.default_pin(pin)
    if not all(isinstance(it, tuple) and len(it) == 2 and isinstance(it[0], dict) and ("tiles" in it[0] or "views" in it[0]) for it in items):
        raise TypeError("collate_raw takes (plan, raw) items: build the dataset with raw=True (dataloaders.inpainting_dataset."
                        "InpaintingDataset, dataloaders.raw_pairs.TestInpaintingDataset, dataloaders.inpainting_crossview_dataset's "
                        "two); dataloaders.test_dataset's own class has no raw mode")
    first = plan_canvases(items[0][0])
    size, views, tiles, multi = items[0][0]["img_size"], len(first), len(first[0]), "views" in items[0][0]
    jobs = np.zeros(len(items) * views * tiles, dtype=JOB_DTYPE)
    jobs["mask_off"] = -1
    jobs["outpaint_col"] = -1
    arena, host = rawbatch.Arena(1), []
    for b, (plan, raw) in enumerate(items):
        canvases = plan_canvases(plan)
        assert plan["img_size"] == size and ("views" in plan) == multi and len(canvases) == views and \
            all(len(c) == tiles for c in canvases), "one canvas shape per batch"
        on_host = any(tile_needs_host(t, raw, size) for c in canvases for t in c)
        if on_host:
            host.append((b, plan, raw))
        where = {}      # a source is placed once per sample

        def place(i):
            if i not in where:
                where[i] = arena.add(raw[i])
            return where[i]

        for v, canvas in enumerate(canvases):
            for t, tile in enumerate(canvas):
                job = jobs[(b * views + v) * tiles + t]
                job["sample"], job["tile"] = b * views + v, t
                if on_host:
                    job["flags"] = HOST
                    continue
                img = raw[tile["image"]]
                assert img.ndim == 3 and img.shape[2] == 3, "image sources are [h, w, 3]"
                job["img_off"], job["img_h"], job["img_w"] = place(tile["image"]), img.shape[0], img.shape[1]
                for k in ("rh", "rw", "y0", "x0", "outpaint_col"):
                    job[k] = tile[k]
                job["flags"] = FLIP_IMAGE * tile["flip"] + FLIP_MASK * tile["mask_flip"] + ZERO_MASK * tile["zero_mask"]
                if tile["outpaint_col"] < 0 and not tile["zero_mask"]:
                    assert 1 <= len(tile["masks"]) <= 2, "one or two mask sources"
                    for q, m in enumerate(tile["masks"]):
                        assert raw[m].ndim == 2, "mask sources are [h, w]"
                        job["mask_off"][q], job["mask_h"][q], job["mask_w"][q] = place(m), raw[m].shape[0], raw[m].shape[1]
    out = dict(arena=arena.tensor(pin), jobs=rawbatch.table_tensor(jobs, pin), img_size=size, tiles=tiles, batch=len(items), host=host,
               txt=default_collate([plan["txt"] for plan, _ in items]))
    if multi:
        out.update(views=views, idx=default_collate([plan["idx"] for plan, _ in items]))
    return out


def job_table(batch):
    """The lr_prep_job records of a collated batch as a numpy structured array (a view)."""
    return batch["jobs"].numpy().view(JOB_DTYPE)


class DevicePrep(rawbatch.DevicePrepBase):
    """collate_raw's batch -> `dict(image, masked_image, mask, txt)` on the device by one lr_batch_prep launch (buffers and views:
    `rawbatch.DevicePrepBase`); a sample marked LR_PREP_HOST is prepared by `run_plan_numpy` and copied in; a multi-view batch comes
    back as [B, V, ...] views with its `idx`."""
    entry = "lr_batch_prep"

    def __init__(self, img_size, tiles=1, device="cuda"):
        super().__init__(img_size, tiles, device)
        self.warned = False

    def dims(self, N):
        return N * self.tiles, self.img_size, self.tiles, N

    def finish(self, batch, out):
        V = batch.get("views")
        for b, plan, raw in batch["host"]:
            if not self.warned:
                self.warned = True
                warnings.warn("DevicePrep: a sample enlarges its source (or is wider than the kernel's row buffer) and is prepared "
                              "on the host; further such samples are routed silently")
            done = run_plan_numpy(plan, raw)
            for k in ("image", "masked_image", "mask"):
                src = torch.from_numpy(np.ascontiguousarray(done[k]))
                (out[k][b] if V is None else out[k][b * V:(b + 1) * V]).copy_(src)
        if V is not None:
            for k in ("image", "masked_image", "mask"):
                out[k] = out[k].view(-1, V, *out[k].shape[1:])
            out["idx"] = batch["idx"]
        return out
