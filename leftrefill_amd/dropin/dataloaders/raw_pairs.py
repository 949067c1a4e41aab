"""`TestInpaintingDataset` with the `raw` keyword of `dataloaders.inpainting_dataset.InpaintingDataset`: the evaluation loader of
dataloaders/test_dataset.py, unchanged, plus `raw=True`, under which an item is `(plan, raw)` -- the decoded source, target and mask
plane and a two-tile plan ([source | target], the left mask all zero) for `leftrefill_amd.dataprep.collate_raw` / `DevicePrep`, which
assemble the batch's canvases on the device.  `raw=False` (default) is the parent's item, byte for byte.

The parent divides its mask by 255 without a threshold; the plan thresholds at > 127 like the training set (a {0, 255} mask file: the
same mask).
"""
import os

from leftrefill_amd import dataprep

from . import test_dataset


class TestInpaintingDataset(test_dataset.TestInpaintingDataset):
    __test__ = False      # not a pytest class
    collate_raw = staticmethod(dataprep.collate_raw)      # collate_fn of the raw=True items (rawbatch.loader)

    def __init__(self, root_path, img_size=256, token_map=None, mask_path=None, raw=False, **kwargs):
        super().__init__(root_path, img_size=img_size, token_map=token_map, mask_path=mask_path, **kwargs)
        self.raw = raw

    def device_prep(self, device="cuda"):
        """What finishes the collated raw batches on the device: [source | target], two tiles per canvas."""
        return dataprep.DevicePrep(self.img_size, 2, device)

    def __getitem__(self, idx):
        if not self.raw:
            return super().__getitem__(idx)
        pair = self.pairs[idx]

        def pick(stem):
            p = f"{pair}/{stem}.jpg"
            return p if os.path.exists(p) else p.replace(".jpg", ".png")

        mask_file = f"{pair}/mask.png" if self.mask_list is None else self.mask_list[idx % len(self.mask_list)]
        s = self.img_size
        tiles = [dataprep.plan_tile(0, s, s, zero_mask=True), dataprep.plan_tile(1, s, s, masks=[2])]
        raw = [test_dataset._read_rgb(pick("source")), test_dataset._read_rgb(pick("target")),
               test_dataset._read_rgb(mask_file)[:, :, 2]]       # cv2.imread(...)[:, :, 0] is the BLUE plane of the file
        return dict(img_size=s, tiles=tiles, txt=self.get_prompt()), raw
