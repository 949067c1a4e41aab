"""`dataloaders.obj_nvs_dataset` (reference dataloaders/obj_nvs_dataset.py): the Objaverse novel-view-synthesis dataset `NVSLDM` is
trained and validated on.

`NVS_OBJDataset`: an object is a folder of `%03d.png` RGBA renders with their `%03d.npy` camera matrices; an item is the
[cond | target] canvas of two of its views.  Item contract: image [S, 2S, 3] float32 in [-1, 1], mask [S, 2S, 1] float32 (0 on the
cond half), masked_image = image * (mask < 0.5) (with `use_ref_mask` in val mode: [cond | white] * (mask < 0.5)), rel_pose float32
[4], txt.  Every item is first a PLAN (leftrefill_amd/nvsprep.py); the reference's random decisions come from the same generators in
the same order and number, also where their result is discarded: `random.sample` for the two views (train mode); in the training-mask
branch `random.random` against `complete_mask_rate`, `random.randint` for the dilation size (before the empty-mask test),
`random.random` for the enlargement (only where `mask_enlarge` is a range), `random.randint` for the number of stroke points,
`np.random.randint` for their columns, their rows and the stroke width; `np.random.choice` for the prompt template (train mode
without `sp_token`).  The bounding box those draws need comes from the row and column occupancy of the shrunk alpha
(`nvsprep.dilated_box`): no dilated plane is formed on the host.  Where the reference raises, this does too: a one-pixel box hands
`np.random.randint` low == high.  `raw=False` (default) executes the plan on the host and returns the finished item; `raw=True`
returns `(plan, raw)` for `nvsprep.collate_nvs_raw` and the device kernel.

Resolution: `leftrefill_amd.dropin.dataloaders.obj_nvs_dataset` is always this module, and this project's tools and models import it
by that name.  As `dataloaders.obj_nvs_dataset` (after `dropin.install()`) it is this module too -- unless another `dataloaders`
directory on sys.path holds a module of that name: a reference tree's own module then keeps the name (end of the import block).

Stated deviations: decoding is PIL's and the four OpenCV primitives are the numpy restatements of leftrefill_amd/nvsprep.py (OpenCV
is absent here; they are not pinned against it); the mask is float32 in every mode (the reference's alpha route leaves it float64
by accident of `/ 255.`; same values); a render smaller than `img_size` raises NotImplementedError (INTER_AREA enlarging is a
different filter); a render must be RGBA (`cv2.imread(IMREAD_UNCHANGED)` of another PNG would hand the reference another channel
count) and a fixed mask file S x S (the reference fails on another size when it concatenates).
"""
import math
import os
import random

import numpy as np
import torch
from torch.utils.data import Dataset

from leftrefill_amd import nvsprep

from .inpainting_dataset import InpaintingDataset

if __name__ == "dataloaders.obj_nvs_dataset":      # imported as the drop-in: another tree's module of this name wins
    import importlib.util
    import sys
    for _d in sys.modules["dataloaders"].__path__:
        _f = os.path.join(_d, "obj_nvs_dataset.py")
        if os.path.isfile(_f) and not os.path.samefile(_f, __file__):
            _spec = importlib.util.spec_from_file_location(__name__, _f)
            sys.modules[__name__] = importlib.util.module_from_spec(_spec)      # the import system hands out what sys.modules holds
            _spec.loader.exec_module(sys.modules[__name__])
            break


def _read_rgba(path):
    from PIL import Image
    return np.array(Image.open(path).convert("RGBA"))


def _read_blue(path):
    """Channel 0 of `cv2.imread(path)` (BGR)."""
    from PIL import Image
    return np.ascontiguousarray(np.array(Image.open(path).convert("RGB"))[:, :, 2])


class NVS_OBJDataset(Dataset):
    templates = InpaintingDataset.templates
    get_prompt = InpaintingDataset.get_prompt

    def __init__(self, datapath, listfile, mode="train", img_size=512, nviews=12, token_map=None, test_limit=150, dilate_size=[8, 20],
                 pts_size=[15, 30], mask_enlarge=[0.0, 0.0], mask_file_path=None, mask_type="fix", width_range=[60, 120],
                 complete_mask_rate=0.0, use_ref_mask=False, raw=False, **kwargs):
        self.datapath, self.listfile, self.mode, self.nviews, self.img_size, self.token_map = datapath, listfile, mode, nviews, img_size, token_map
        self.repeat_sp_token = kwargs.get("repeat_sp_token", 0)      # > 0: the prompt is the same token repeated
        self.sp_token = kwargs.get("sp_token", None)
        self.deep_prompt = kwargs.get("deep_prompt", False)
        self.cross_attn_layers = 16
        self.test_limit, self.dilate_size, self.pts_size, self.mask_type = test_limit, dilate_size, pts_size, mask_type
        self.obj_mask_path = kwargs.get("obj_mask_path", None)
        self.complete_mask_rate, self.width_range, self.mask_enlarge, self.use_ref_mask = complete_mask_rate, width_range, mask_enlarge, use_ref_mask
        self.raw = raw
        with open(self.listfile, "r") as f:
            self.metas = [os.path.join(self.datapath, line.strip()) for line in f.readlines()]
        if self.mode == "val" and self.test_limit < len(self.metas):
            self.metas = self.metas[::len(self.metas) // self.test_limit]
        self.mask_file_path = mask_file_path
        if self.mask_file_path is not None:
            print("Using masks from", self.mask_file_path)

    def __len__(self):
        return len(self.metas)

    collate_raw = staticmethod(nvsprep.collate_nvs_raw)      # collate_fn of the raw=True items (rawbatch.loader)

    def device_prep(self, device="cuda"):
        """What finishes the collated raw batches on the device: [cond | target]."""
        return nvsprep.NVSDevicePrep(self.img_size, device)

    def cartesian_to_spherical(self, xyz):
        xy = xyz[:, 0] ** 2 + xyz[:, 1] ** 2
        z = np.sqrt(xy + xyz[:, 2] ** 2)
        theta = np.arctan2(np.sqrt(xy), xyz[:, 2])      # elevation from the Z axis down
        azimuth = np.arctan2(xyz[:, 1], xyz[:, 0])
        return np.array([theta, azimuth, z])

    def get_T(self, target_RT, cond_RT):
        R, T = target_RT[:3, :3], target_RT[:, -1]
        T_target = -R.T @ T
        R, T = cond_RT[:3, :3], cond_RT[:, -1]
        T_cond = -R.T @ T
        theta_cond, azimuth_cond, z_cond = self.cartesian_to_spherical(T_cond[None, :])
        theta_target, azimuth_target, z_target = self.cartesian_to_spherical(T_target[None, :])
        d_theta = theta_target - theta_cond
        d_azimuth = (azimuth_target - azimuth_cond) % (2 * math.pi)
        d_z = z_target - z_cond
        return torch.tensor([d_theta.item(), math.sin(d_azimuth.item()), math.cos(d_azimuth.item()), d_z.item()])

    def plan_strokes(self, rows, cols, k):
        """The stroke plane over the dilated mask's box (reference 152-176): uint8 [S, S] of {0, 1}."""
        from PIL import Image, ImageDraw
        S = self.img_size
        h_min, h_max, w_min, w_max = nvsprep.dilated_box(rows, cols, k)
        if self.mask_enlarge[1] > self.mask_enlarge[0]:
            enlarge_rate = random.random() * (self.mask_enlarge[1] - self.mask_enlarge[0]) + self.mask_enlarge[0]
            max_diff = max(h_max - h_min, w_max - w_min) * enlarge_rate
            h_min, h_max = np.clip(h_min - max_diff, 0, S - 1), np.clip(h_max + max_diff, 0, S - 1)
            w_min, w_max = np.clip(w_min - max_diff, 0, S - 1), np.clip(w_max + max_diff, 0, S - 1)
        pts_size = random.randint(self.pts_size[0], self.pts_size[1])
        random_x = np.random.randint(w_min, w_max, size=pts_size)
        random_y = np.random.randint(h_min, h_max, size=pts_size)
        random_pts = np.stack([random_x, random_y], axis=1)
        plane = Image.new("L", (S, S), 0)
        width = np.random.randint(self.width_range[0] * (S / 512), self.width_range[1] * (S / 512))
        draw = ImageDraw.Draw(plane)
        pts = np.append(random_pts, random_pts[:1], axis=0).astype(np.float32)      # float32: Pillow reads the buffer as floats
        draw.line(pts, fill=1, width=width)
        for v in pts:
            draw.ellipse((v[0] - width // 2, v[1] - width // 2, v[0] + width // 2, v[1] + width // 2), fill=1)
        return np.asarray(plane, np.uint8).copy()

    def plan(self, idx):
        """(plan, raw) of item idx: every decision and draw, no pixel work beyond the alpha's row and column occupancy."""
        S, filename = self.img_size, self.metas[idx]
        if self.mode == "train":
            index_target, index_cond = random.sample(range(self.nviews), 2)
        else:
            index_target, index_cond = 0, 2
        target = _read_rgba(os.path.join(filename, "%03d.png" % index_target))
        cond = _read_rgba(os.path.join(filename, "%03d.png" % index_cond))
        for im in (target, cond):
            if im.shape[0] < S or im.shape[1] < S:
                raise NotImplementedError(f"a {im.shape[0]} x {im.shape[1]} render is smaller than img_size = {S}: enlarging is not stated here")
        raw, mode, k, plane = [cond, target], "alpha", 0, None
        if self.mask_file_path is not None and self.mode != "train" and self.mask_type == "fix":
            index_mask = index_cond if self.use_ref_mask else index_target
            raw.append(_read_blue(os.path.join(self.mask_file_path, filename.split("/")[-1], "%03d.png" % index_mask)))
            assert raw[2].shape == (S, S), f"the fixed mask is {raw[2].shape}, not {S} x {S}"
            mode, plane = "file", 2
        elif self.mode != "train" and self.mask_type == "complete":
            mode = "ones"
        elif random.random() < self.complete_mask_rate:
            mode = "ones"
        else:
            k = random.randint(self.dilate_size[0], self.dilate_size[1])
            rows, cols = nvsprep.alpha_lines(target[:, :, 3], S)
            if not rows.any():      # no alpha anywhere: the dilated mask sums to 0
                mode = "ones"
            else:
                raw.append(self.plan_strokes(rows, cols, k))
                plane = 2
        target_RT = np.load(os.path.join(filename, "%03d.npy" % index_target))
        cond_RT = np.load(os.path.join(filename, "%03d.npy" % index_cond))
        rel_pose = self.get_T(target_RT, cond_RT).tolist()
        plan = dict(img_size=S, mode=mode, k=int(k) if mode == "alpha" else 0, plane=plane,
                    ref_white=bool(self.mode != "train" and self.use_ref_mask), rel_pose=rel_pose, txt=self.get_prompt())
        return plan, raw

    def __getitem__(self, idx):
        plan, raw = self.plan(idx)
        return (plan, raw) if self.raw else nvsprep.run_nvs_plan_numpy(plan, raw)
