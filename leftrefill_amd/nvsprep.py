"""Novel-view-synthesis batches from raw RGBA renders: the arithmetic of the Objaverse dataset (reference dataloaders/obj_nvs_dataset.py
109-189) stated once in numpy -- the host route and the yardstick --, its plan, and the device route (`collate_nvs_raw` +
`NVSDevicePrep`: one arena copy, one job-table copy, one `lr_nvs_prep` launch per batch, csrc/nvs_prep.hip; the arena packer, the
buffer policy, the uploads and the loader wiring are rawbatch.py's, shared with dataprep.py).

The reference leans on four OpenCV primitives.  OpenCV is absent here, so they are RESTATED below and these statements are the
definition; they are not pinned against OpenCV itself:

    resize_linear_u8   cv2.resize(uint8 image, (S, S)), default INTER_LINEAR: copy at equal size, the 2 x 2 box
                       (a + b + c + d + 2) >> 2 at exactly half size (OpenCV's fast path; the shipped 512 -> 256), else the legacy
                       fixed-point bilinear with 11-bit coefficients
    occupancy          cv2.resize(alpha > 0, (S, S), INTER_AREA) > 0: any set source cell under the area table's taps, sliver
                       threshold 1e-3 included
    ellipse_spans      cv2.getStructuringElement(MORPH_ELLIPSE, (k, k)) as one [lo, hi) column span per row
    dilate             cv2.dilate with that element, anchor at (k // 2, k // 2), positions outside the image ignored

The composite needs no arithmetic: `((x / 255.) * 255.).astype(uint8) == x` for every byte (tests/test_nvsdata_cpu.py asserts it),
so a pixel of alpha 0 becomes white and every other pixel keeps its RGB bytes.

A plan is `dict(img_size, mode, k, plane, ref_white, rel_pose, txt)` over `raw = [cond RGBA, target RGBA (, plane)]`:
    mode "alpha"  mask = dilate(occupancy(target alpha), k) | (plane > 0), plane the S x S stroke plane of {0, 1} or None
    mode "ones"   mask = 1
    mode "file"   mask = float32(plane / 255.), not thresholded (plane: channel 0 of the fixed mask file)
    ref_white     masked_image = [cond | white] * (mask < 0.5) instead of image * (mask < 0.5)
The canvas is [cond | target]; the cond half of the mask is 0.  The mask is float32 in every mode (in the reference the alpha
route's is float64 by accident of `/ 255.`; the values are the same).
"""
import ctypes

import numpy as np
import torch

from . import _lib, rawbatch

ALPHA, ONES, FILE = 0, 1, 2                  # LR_NVS_MODE_* of include/leftrefill_hip.h
REF_WHITE = 1                                # LR_NVS_REF_WHITE
MAX_SIZE, MAX_DILATE = 512, 32               # LR_NVS_MAX_SIZE, LR_NVS_MAX_DILATE
MODES = {"alpha": ALPHA, "ones": ONES, "file": FILE}
JOB_DTYPE = np.dtype(_lib.NvsJob)            # numpy image of struct lr_nvs_job
assert JOB_DTYPE.itemsize == ctypes.sizeof(_lib.NvsJob) == 120


# ---- the arithmetic -----------------------------------------------------------------------------------------------------------------
def composite_white(rgba):
    """uint8 [h, w, 4] RGBA -> uint8 [h, w, 3] RGB on white: alpha 0 becomes 255, every other pixel keeps its bytes."""
    out = rgba[:, :, :3].copy()
    out[rgba[:, :, 3] == 0] = 255
    return out


def linear_taps(n, S):
    """Per destination index of an axis of n source cells: (s0, s1, a0, a1) of the fixed-point bilinear, int32 [S] each."""
    scale = n / S
    f = ((np.arange(S, dtype=np.float64) + 0.5) * scale - 0.5).astype(np.float32)
    s = np.floor(f).astype(np.int32)
    f = f - s.astype(np.float32)
    low, high = s < 0, s >= n - 1
    s = np.where(low, 0, np.where(high, n - 1, s)).astype(np.int32)
    f = np.where(low | high, np.float32(0), f).astype(np.float32)
    a0 = np.rint((np.float32(1) - f) * np.float32(2048)).astype(np.int32)
    a1 = np.rint(f * np.float32(2048)).astype(np.int32)
    return s, np.minimum(s + 1, n - 1).astype(np.int32), a0, a1


def resize_linear_u8(img, S):
    """uint8 [h, w, 3] -> uint8 [S, S, 3] (module docstring); h >= S and w >= S."""
    h, w = img.shape[:2]
    if h < S or w < S:
        raise NotImplementedError(f"a {h} x {w} render is smaller than img_size = {S}: enlarging is not stated here")
    if (h, w) == (S, S):
        return img.copy()
    v = img.astype(np.int32)
    if h == 2 * S and w == 2 * S:
        return ((v[0::2, 0::2] + v[0::2, 1::2] + v[1::2, 0::2] + v[1::2, 1::2] + 2) >> 2).astype(np.uint8)
    x0, x1, a0, a1 = linear_taps(w, S)
    y0, y1, b0, b1 = linear_taps(h, S)
    rows = v[:, x0] * a0[None, :, None] + v[:, x1] * a1[None, :, None]      # [h, S, 3] int32
    out = (((b0[:, None, None] * (rows[y0] >> 4)) >> 16) + ((b1[:, None, None] * (rows[y1] >> 4)) >> 16) + 2) >> 2
    return out.astype(np.uint8)


def area_taps(n, S):
    """Per destination index of an axis of n source cells: the first and the last source cell of its INTER_AREA tap set (a run)."""
    scale = n / S
    first, last = np.empty(S, np.int64), np.empty(S, np.int64)
    for d in range(S):
        f1 = d * scale
        f2 = f1 + scale
        s1, s2 = int(np.ceil(f1)), min(int(np.floor(f2)), n - 1)
        s1 = min(s1, s2)
        first[d] = s1 - 1 if s1 - f1 > 1e-3 else s1
        last[d] = s2 if f2 - s2 > 1e-3 else s2 - 1
    return first, last


def shrink_any(line, S):
    """bool [n] -> bool [S]: any set cell under each destination index's taps."""
    first, last = area_taps(len(line), S)
    return np.array([line[a:b + 1].any() for a, b in zip(first, last)])


def occupancy(alpha, S):
    """uint8 [h, w] alpha -> bool [S, S]: `cv2.resize(alpha > 0, (S, S), INTER_AREA) > 0`."""
    h, w = alpha.shape
    if h < S or w < S:
        raise NotImplementedError(f"a {h} x {w} render is smaller than img_size = {S}: enlarging is not stated here")
    set_ = alpha > 0
    rf, rl = area_taps(h, S)
    cf, cl = area_taps(w, S)
    rows = np.stack([set_[a:b + 1].any(axis=0) for a, b in zip(rf, rl)])            # [S, w]
    return np.stack([rows[:, a:b + 1].any(axis=1) for a, b in zip(cf, cl)], axis=1)


def ellipse_spans(k):
    """The elliptic k x k element as int [k, 2]: row e has ones in columns [lo, hi)."""
    r = c = k // 2
    inv = 1.0 / (r * r) if r else 0.0
    spans = np.empty((k, 2), np.int64)
    for e in range(k):
        dy = e - r
        dx = int(np.rint(c * np.sqrt((r * r - dy * dy) * inv))) if abs(dy) <= r else 0
        spans[e] = max(c - dx, 0), min(c + dx + 1, k)
    return spans


def dilate(mask, k):
    """bool [H, W] -> bool [H, W]: dst(y, x) = OR over the element's (e, j) of src(y + e - r, x + j - c)."""
    H, W = mask.shape
    r = c = k // 2
    out = np.zeros((H, W), bool)
    for e, (lo, hi) in enumerate(ellipse_spans(k)):
        for j in range(lo, hi):
            dy, dx = e - r, j - c      # out[y, x] |= mask[y + dy, x + dx]
            ya, yb, xa, xb = max(0, -dy), min(H, H - dy), max(0, -dx), min(W, W - dx)
            if ya < yb and xa < xb:
                out[ya:yb, xa:xb] |= mask[ya + dy:yb + dy, xa + dx:xb + dx]
    return out


def dilated_box(rows, cols, k):
    """Bounding box (h_min, h_max, w_min, w_max) of `dilate(m, k)` from m's row and column occupancy (bool [S] each, not all clear):
    a set cell at y reaches y - (k - 1 - r) .. y + r.  No plane is formed."""
    r = k // 2
    ys, xs = np.flatnonzero(rows), np.flatnonzero(cols)
    return (max(0, ys[0] - (k - 1 - r)), min(len(rows) - 1, ys[-1] + r), max(0, xs[0] - (k - 1 - r)), min(len(cols) - 1, xs[-1] + r))


def alpha_lines(alpha, S):
    """Row and column occupancy (bool [S] each) of `occupancy(alpha, S)` without forming it: the taps cover every source cell, so a
    shrunk row is occupied iff one of its source rows is."""
    h, w = alpha.shape
    if h < S or w < S:
        raise NotImplementedError(f"a {h} x {w} render is smaller than img_size = {S}: enlarging is not stated here")
    set_ = alpha > 0
    return shrink_any(set_.any(axis=1), S), shrink_any(set_.any(axis=0), S)


# ---- the host route -----------------------------------------------------------------------------------------------------------------
def run_nvs_plan_numpy(plan, raw):
    """Execute a plan on the host: the finished item `dict(image, masked_image, mask, rel_pose, txt)`."""
    S = plan["img_size"]
    cond = resize_linear_u8(composite_white(raw[0]), S)
    target = resize_linear_u8(composite_white(raw[1]), S)
    if plan["mode"] == "ones":
        mask = np.ones((S, S), dtype=np.float32)
    elif plan["mode"] == "file":
        mask = (raw[plan["plane"]] / 255).astype(np.float32)
    else:
        bits = dilate(occupancy(raw[1][:, :, 3], S), plan["k"])
        if plan["plane"] is not None:
            bits = bits | (raw[plan["plane"]] > 0)
        mask = bits.astype(np.float32)
    image = np.concatenate([cond, target], axis=1).astype(np.float32) / 127.5 - 1.0
    mask = np.concatenate([np.zeros_like(mask), mask], axis=1)[:, :, None]
    if plan["ref_white"]:
        masked = (np.concatenate([cond, np.ones_like(cond) * 255], axis=1).astype(np.float32) / 127.5 - 1.0) * (mask < 0.5)
    else:
        masked = image * (mask < 0.5)
    return dict(image=image, masked_image=masked, mask=mask, rel_pose=torch.tensor(plan["rel_pose"], dtype=torch.float32), txt=plan["txt"])


# ---- the device route ---------------------------------------------------------------------------------------------------------------
def collate_nvs_raw(items, pin=None):
    """DataLoader collate_fn for `NVS_OBJDataset(raw=True)`: a list of (plan, raw) -> one byte arena holding every render and plane at a
    16-byte-aligned offset, the lr_nvs_job table (one job per sample, the element's spans of `ellipse_spans(k)` included), `txt`
    collated as the DataLoader would and `rel_pose` float32 [B, 4].  pin: as `dataprep.collate_raw`."""
    from torch.utils.data import default_collate
    pin = rawbatch.default_pin(pin)
    if not all(isinstance(it, tuple) and len(it) == 2 and isinstance(it[0], dict) and "mode" in it[0] for it in items):
        raise TypeError("collate_nvs_raw takes (plan, raw) items: build dataloaders.obj_nvs_dataset.NVS_OBJDataset with raw=True")
    size = items[0][0]["img_size"]
    jobs = np.zeros(len(items), dtype=JOB_DTYPE)
    jobs["plane_off"] = -1
    arena = rawbatch.Arena(16)
    for b, (plan, raw) in enumerate(items):
        assert plan["img_size"] == size, "one canvas shape per batch"
        job = jobs[b]
        job["sample"], job["mode"], job["flags"] = b, MODES[plan["mode"]], REF_WHITE * bool(plan["ref_white"])
        for name, arr in (("cond", raw[0]), ("target", raw[1])):
            assert arr.dtype == np.uint8 and arr.ndim == 3 and arr.shape[2] == 4, "renders are uint8 [h, w, 4]"
            if arr.shape[0] < size or arr.shape[1] < size:
                raise NotImplementedError(f"a {arr.shape[0]} x {arr.shape[1]} render is smaller than img_size = {size}")
            job[name + "_off"], job[name + "_h"], job[name + "_w"] = arena.add(arr), arr.shape[0], arr.shape[1]
        if plan["plane"] is not None:
            arr = raw[plan["plane"]]
            assert arr.dtype == np.uint8 and arr.shape == (size, size), "the plane is uint8 [S, S]"
            job["plane_off"] = arena.add(arr)
        if plan["mode"] == "alpha":
            job["k"] = plan["k"]
            if 1 <= plan["k"] <= MAX_DILATE:      # a larger element is the entry's to refuse
                spans = ellipse_spans(plan["k"])
                job["lo"][:plan["k"]], job["hi"][:plan["k"]] = spans[:, 0], spans[:, 1]
    return dict(arena=arena.tensor(pin), jobs=rawbatch.table_tensor(jobs, pin), img_size=size, batch=len(items),
                txt=default_collate([plan["txt"] for plan, _ in items]),
                rel_pose=torch.tensor([plan["rel_pose"] for plan, _ in items], dtype=torch.float32).reshape(len(items), 4))


def job_table(batch):
    """The lr_nvs_job records of a collated batch as a numpy structured array (a view)."""
    return batch["jobs"].numpy().view(JOB_DTYPE)


class NVSDevicePrep(rawbatch.DevicePrepBase):
    """collate_nvs_raw's batch -> `dict(image, masked_image, mask, rel_pose, txt)` on the device by one lr_nvs_prep launch (buffers and
    views: `rawbatch.DevicePrepBase`); the canvas is the two tiles [cond | target], and `rel_pose` has a grow-only buffer of its own."""
    entry = "lr_nvs_prep"

    def __init__(self, img_size, device="cuda"):
        super().__init__(img_size, 2, device)
        self.rel_pose = None

    def allocate(self, N):
        super().allocate(N)
        self.rel_pose = torch.empty(N, 4, device=self.device)

    def dims(self, N):
        return N, self.img_size

    def finish(self, batch, out):
        out["rel_pose"] = self.rel_pose[:batch["batch"]].copy_(batch["rel_pose"], non_blocking=True)
        return out
