"""`dataloaders.inpainting_dataset.InpaintingDataset` (reference dataloaders/inpainting_dataset.py:11-189), the single-image training /
validation / test dataset: one image per item, masked by an irregular mask, a segmentation mask, their sum (`train`), an
outpainting band (`outpainting=True`) or a fixed mask cycled from `mask_path` (`val`, `test`).

Batch contract (181-189): image [S, S, 3] float32 in [-1, 1], mask [S, S, 1] in {0, 1}, masked_image = image * (mask < 0.5), txt.

Every item is first a PLAN (leftrefill_amd/dataprep.py): the reference's random decisions, drawn from the same generators in the same
order and number -- resize branch, crop offsets (column, then row), mask branch and indices, image flip, mask flip, prompt template --
so a seeded run picks what the reference picks.  `raw=False` (default) executes the plan on the host and returns the finished sample;
`raw=True` returns `(plan, raw)`, the plan plus the decoded uint8 arrays, for `dataprep.collate_raw` and the device kernel.

The reference decodes and resizes with OpenCV (absent here); this loader decodes with PIL -- `convert("RGB")` is the BGR -> RGB
conversion of 158-160, `convert("L")` the luma of `cv2.imread(..., IMREAD_GRAYSCALE)` (the same bytes for a grey file) -- and resizes
with the numpy restatements of dataloaders/test_dataset.py.  `test` mode's PIL bicubic resize (154-156) stays on the host; its plan is
the identity.  `val` strides by `len // test_limit` like the reference, but by at least 1 (the reference fails on fewer files than
`test_limit`).
"""
import os
from glob import glob

import numpy as np
from torch.utils.data import Dataset

from leftrefill_amd import dataprep

from .test_dataset import _read_rgb


def _read_grey(path):
    from PIL import Image
    return np.asarray(Image.open(path).convert("L"))


def _read_lines(path):
    with open(path) as f:
        return [ln.strip() for ln in f.readlines()]


def _by_name(paths):
    return sorted(paths, key=lambda p: p.split("/")[-1])


class InpaintingDataset(Dataset):
    def __init__(self, image_list, mask_path=None, mode="train", img_size=512, token_map=None, test_limit=200, flip=True,
                 outpainting=False, outpainting_min_rate=0.25, outpainting_max_rate=0.75, root_path=None, raw=False, **kwargs):
        if image_list.endswith(".txt"):
            self.image_list = _read_lines(image_list)
            if root_path is not None:
                self.image_list = [os.path.join(root_path, im) for im in self.image_list]
        else:
            self.image_list = _by_name(glob(image_list + "/*"))
        self.mask_path, self.mode, self.img_size, self.token_map, self.raw = mask_path, mode, img_size, token_map, raw
        self.repeat_sp_token = kwargs.get("repeat_sp_token", 0)   # > 0: the prompt is the special token repeated that often
        self.sp_token = kwargs.get("sp_token", None)
        self.deep_prompt = kwargs.get("deep_prompt", False)
        self.cross_attn_layers = 16
        self.flip, self.outpainting = flip, outpainting
        self.outpainting_min_rate, self.outpainting_max_rate = outpainting_min_rate, outpainting_max_rate
        if mode == "train":       # irregular and segmentation masks, one list file each
            self.irregular_mask_list = _by_name(_read_lines(mask_path[0]))
            self.segment_mask_list = _by_name(_read_lines(mask_path[1]))
        elif mask_path.endswith(".txt"):
            self.mask_list = _read_lines(mask_path)
        else:
            self.mask_list = _by_name(glob(mask_path + "/*"))
        if mode == "val":
            self.image_list = self.image_list[::max(1, len(self.image_list) // test_limit)]
            self.mask_list = self.mask_list[::max(1, len(self.mask_list) // test_limit)]

    def __len__(self):
        return len(self.image_list)

    collate_raw = staticmethod(dataprep.collate_raw)      # collate_fn of the raw=True items (rawbatch.loader)

    def device_prep(self, device="cuda"):
        """What finishes the collated raw batches on the device: one tile per canvas."""
        return dataprep.DevicePrep(self.img_size, 1, device)

    def templates(self):
        t = self.token_map
        left, right, task, real = t["left_token"], t["right_token"], t["task_token"], t["real_token"]
        return [f"Both {left} and {right} images show the {real} with different {task}.",
                f"The {real} remains the same in both the {left} and {right} images, but the {task} are different.",
                f"The {left} and {right} images depict identical {real}, but from different {task}.",
                f"The painting depicts the {real}, but from two different {task}; one from the {left} and one from the {right}.",
                f"Both figures capture the same {real}, but the {left} one and the {right} one are taken from different {task}.",
                f"The two drawings show the {real}, but one is from the {left} side and the other is from the {right} side, and they are from different {task}",
                f"Both pictures depict the same {real}, but the {left} image and the {right} image are captured with different {task}."]

    def get_prompt(self):
        if self.repeat_sp_token > 0 and self.sp_token is not None:
            text = " ".join(self.sp_token.replace(">", f"{i}>") for i in range(self.repeat_sp_token))
            if self.deep_prompt:        # one prompt per cross-attention layer
                return [text.replace(">", f"-layer{layer}>") for layer in range(self.cross_attn_layers)]
            return text
        templates = self.templates()      # only used for cross-view inpainting
        if self.mode == "train":
            return str(np.random.choice(templates, size=1)[0])
        return templates[0]

    def plan(self, idx):
        """(plan, raw) of item idx: decode, then decide -- no pixel work beyond the decode (and `test` mode's bicubic resize)."""
        S, path = self.img_size, self.image_list[idx]
        if self.mode == "test":
            from PIL import Image
            img = np.array(Image.open(path).convert("RGB").resize((S, S), resample=Image.BICUBIC).convert("RGB"))
        else:
            img = _read_rgb(path)
        raw = [img]
        h, w = img.shape[:2]
        resize = dataprep.plan_resize_train(h, w, S) if self.mode == "train" else dict(rh=S, rw=S, y0=0, x0=0)
        masks, col = [], -1
        if self.mode != "train":
            raw.append(_read_grey(self.mask_list[idx % len(self.mask_list)]))
            masks = [1]
        elif self.outpainting:
            col = dataprep.plan_outpaint_col(S, self.outpainting_min_rate, self.outpainting_max_rate)
        else:
            lists = {"irregular": self.irregular_mask_list, "segment": self.segment_mask_list}
            for kind, i in dataprep.plan_mask_train(len(self.irregular_mask_list), len(self.segment_mask_list)):
                raw.append(_read_grey(lists[kind][i]))
                masks.append(len(raw) - 1)
        flip, mask_flip = dataprep.plan_flips() if self.flip and self.mode == "train" else (False, False)
        tile = dataprep.plan_tile(0, flip=flip, masks=masks, mask_flip=mask_flip, outpaint_col=col, **resize)
        return dict(img_size=S, tiles=[tile], txt=self.get_prompt()), raw

    def __getitem__(self, idx):
        plan, raw = self.plan(idx)
        return (plan, raw) if self.raw else dataprep.run_plan_numpy(plan, raw)
