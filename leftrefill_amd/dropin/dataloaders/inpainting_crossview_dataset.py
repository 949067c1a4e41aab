"""`dataloaders.inpainting_crossview_dataset` (reference dataloaders/inpainting_crossview_dataset.py): the image-pair datasets the
prompt tokens are trained and evaluated on, and the scene-balanced sampler.

`InpaintingCrossViewDataset` (18-371): one [source | target] or [target | source] canvas per pair.  Item contract: image [S, 2S, 3]
float32 in [-1, 1], mask [S, 2S, 1] in {0, 1}, masked_image = image * (mask < 0.5), txt.  Every item is first a PLAN of two tiles
(leftrefill_amd/dataprep.py); the reference's random decisions come from the same generators in the same order and number: resize
branch and window of the source, then of the target (`plan_resize_train`); the placement draw (taken in every mode); the view-mask
decision and its side; `load_mask`'s short-circuited match-mask draw and `plan_match_mask`; `get_inpainting_mask` (the sum branch
takes the segment index before the irregular one), then its side; one flip draw per half, which flips that half's image and mask
together (both flip flags of the tile); the prompt template.  A whole-view mask is `outpaint_col=0` on that tile, the other tile is
`zero_mask`.  `raw=False` (default) executes the plan on the host and returns the finished sample; `raw=True` returns `(plan, raw)`
for `dataprep.collate_raw` and the device kernel.

`InpaintingMultiViewDataset` (374-766), `mode="val"`: view 0 is the masked target, views 1.. the references; `concat_target=True`
puts the target on the right of every [reference_i | target] canvas and the mask only there.  Items are float32 for both settings
(the reference's concatenated arrays are float64 by accident of `np.zeros`; the values are the same).  `mode="train"` raises
NotImplementedError: in the reference it cannot return an item.

`BalancedRandomSampler` (771-839): `n_sample_per_scene` pairs of every scene per epoch; `__iter__` reseeds Python's generator with
the epoch and shuffles the per-scene lists IN PLACE, so the order of epoch e depends on the epochs iterated before it -- kept.

Resolution: `leftrefill_amd.dropin.dataloaders.inpainting_crossview_dataset` is always this module, and this project's tools and models
import it by that name.  As `dataloaders.inpainting_crossview_dataset` (after `dropin.install()`) it is this module too -- unless another
`dataloaders` directory on sys.path holds a module of that name, which the drop-in package has never shadowed and still does not: a
reference tree's own module then keeps the name (see the end of the import block below).

Stated deviations: decoding is PIL's and the resizes are the numpy restatements of dataloaders/test_dataset.py (the reference uses
OpenCV, absent here); val mode strides by max(1, len // test_limit) (the reference divides by zero on fewer pairs than
`test_limit`); the two-list-file form of `image_path` is taken before the directory test (the reference hands the list to
os.path.isdir, which raises); `no_padding=False` is served on the host route only; the sampler prints no progress bar.
"""
import collections
import math
import os
import pickle
import random
from glob import glob

import numpy as np
from torch.utils.data import Dataset, Sampler

from leftrefill_amd import dataprep

from .inpainting_dataset import InpaintingDataset, _by_name, _read_grey, _read_lines
from .test_dataset import _read_rgb

if __name__ == "dataloaders.inpainting_crossview_dataset":      # imported as the drop-in: another tree's module of this name wins
    import importlib.util
    import sys
    for _d in sys.modules["dataloaders"].__path__:
        _f = os.path.join(_d, "inpainting_crossview_dataset.py")
        if os.path.isfile(_f) and not os.path.samefile(_f, __file__):
            _spec = importlib.util.spec_from_file_location(__name__, _f)
            sys.modules[__name__] = importlib.util.module_from_spec(_spec)      # the import system hands out what sys.modules holds
            _spec.loader.exec_module(sys.modules[__name__])
            break


def _val_pairs(image_path, test_limit):
    """Pair directories of the val / test modes: a directory of them, strided to about `test_limit`, or two list files (normal,
    special): every special pair, then normal ones up to `test_limit`."""
    if isinstance(image_path, (list, tuple)):
        files = _read_lines(image_path[1])
        files.extend(_read_lines(image_path[0])[:max(0, test_limit - len(files))])
        return files
    pairs = _by_name(glob(image_path + "/*"))
    return pairs[::max(1, len(pairs) // test_limit)]


def _pick(pair, stem):
    p = f"{pair}/{stem}.jpg"
    return p if os.path.exists(p) else p.replace(".jpg", ".png")


class InpaintingCrossViewDataset(Dataset):
    templates = InpaintingDataset.templates
    get_prompt = InpaintingDataset.get_prompt

    def __init__(self, image_path, pair_path, mask_path, mode="train", img_size=256, only_mask_image=False, no_padding=True,
                 token_map=None, view_mask_rate=0.9, test_limit=150, flip=False, constant_place=False, raw=False, **kwargs):
        if raw and not no_padding:
            raise ValueError("raw=True with no_padding=False: lr_batch_prep writes canvases of S rows, the padded 2S x 2S canvas is "
                             "built on the host route only (raw=False)")
        if mode == "train":
            with open(image_path, "rb") as f:
                self.image_dict = pickle.load(f)
            with open(pair_path, "rb") as f:
                self.pairs = pickle.load(f)
        else:
            self.pairs = _val_pairs(image_path, test_limit)
        self.mask_path, self.mode, self.img_size, self.raw = mask_path, mode, img_size, raw
        self.only_mask_image, self.no_padding, self.token_map = only_mask_image, no_padding, token_map
        self.view_mask_rate = view_mask_rate                      # how often the whole other view is masked
        self.repeat_sp_token = kwargs.get("repeat_sp_token", 0)   # > 0: the prompt is the special token repeated that often
        self.sp_token = kwargs.get("sp_token", None)
        self.match_mask = kwargs.get("match_mask", False)         # use the matching-based mask ...
        self.match_mask_rate = kwargs.get("match_mask_rate", 0.0)   # ... in this share of the random masks
        self.match_path = kwargs.get("match_path", None)
        self.deep_prompt = kwargs.get("deep_prompt", False)
        self.cross_attn_layers = 16
        self.flip, self.constant_place = flip, constant_place
        if mode == "train":       # irregular and segmentation masks, one list file each
            self.irregular_mask_list = _by_name(_read_lines(mask_path[0]))
            self.segment_mask_list = _by_name(_read_lines(mask_path[1]))
        else:
            self.mask_list = _by_name(glob(mask_path + "/*"))

    def __len__(self):
        return len(self.pairs)

    collate_raw = staticmethod(dataprep.collate_raw)      # collate_fn of the raw=True items (rawbatch.loader)

    def device_prep(self, device="cuda"):
        """What finishes the collated raw batches on the device: [left | right], two tiles per canvas."""
        return dataprep.DevicePrep(self.img_size, 2, device)

    def _resize(self, img):
        """(resize decisions, crop record) of one image: `plan_resize_train` in train mode, the direct resize otherwise."""
        S = self.img_size
        if self.mode != "train":
            return dict(rh=S, rw=S, y0=0, x0=0), None
        state = random.getstate()      # peek at the branch draw: a crop branch can land on S x S too, and still has a record
        cropped = not random.random() < 0.5
        random.setstate(state)
        resize = dataprep.plan_resize_train(img.shape[0], img.shape[1], S)
        return resize, (dict(w_start=resize["x0"], h_start=resize["y0"], w=resize["rw"], h=resize["rh"]) if cropped else None)

    def _random_mask(self, raw):
        """`get_inpainting_mask` (200-229): mask sources appended to raw; (their indices, mask_left)."""
        lists = {"irregular": self.irregular_mask_list, "segment": self.segment_mask_list}
        masks = []
        for kind, i in dataprep.plan_mask_train(len(self.irregular_mask_list), len(self.segment_mask_list)):
            raw.append(_read_grey(lists[kind][i]))
            masks.append(len(raw) - 1)
        return masks, random.random() < 0.5

    def plan(self, idx):
        """(plan, raw) of item idx: decode, then decide."""
        S, pair = self.img_size, self.pairs[idx]
        if self.mode == "train":
            names = self.image_dict[pair["source"]], self.image_dict[pair["target"]]
        else:
            names = _pick(pair, "source"), _pick(pair, "target")
        raw = [_read_rgb(names[0]), _read_rgb(names[1])]
        (s_resize, s_crop), (t_resize, t_crop) = self._resize(raw[0]), self._resize(raw[1])
        rdv = random.random()      # drawn in every mode
        gt_pos = "left" if self.mode == "train" and rdv < 0.5 and not self.constant_place else "right"
        order = (1, 0) if gt_pos == "left" else (0, 1)      # the raw index shown by the left and the right tile
        resizes = {0: s_resize, 1: t_resize}
        mask_kw = [dict(zero_mask=True), dict(zero_mask=True)]      # per half
        view = dict(outpaint_col=0)
        if self.mode != "train":      # a pair's own mask before the cycled list; always on the right
            own = pair + "/mask.png"
            raw.append(_read_grey(own if os.path.exists(own) else self.mask_list[idx % len(self.mask_list)]))
            mask_kw[1] = dict(masks=[2])
        elif self.only_mask_image:
            mask_kw[0 if gt_pos == "left" else 1] = view
        elif random.random() < 1.0 - self.view_mask_rate:      # a random mask, as in the regular inpainting task
            matched = None
            if self.match_mask and random.random() < self.match_mask_rate:
                matched = dataprep.plan_match_mask(self.match_path, idx, gt_pos, t_crop, s_crop, self.constant_place)
            if matched is not None:
                raw.append(matched[1])
                masks, mask_left = [len(raw) - 1], matched[0]
            else:
                masks, mask_left = self._random_mask(raw)
            mask_kw[0 if mask_left else 1] = dict(masks=masks)
        else:      # the whole left or right view
            mask_kw[0 if random.random() < 0.5 else 1] = view
        flips = [False, False]
        if self.mode == "train" and self.flip:
            flips = [random.random() < 0.5, random.random() < 0.5]
        tiles = [dataprep.plan_tile(order[k], flip=flips[k], mask_flip=flips[k], **resizes[order[k]], **mask_kw[k]) for k in (0, 1)]
        return dict(img_size=S, tiles=tiles, txt=self.get_prompt()), raw

    def __getitem__(self, idx):
        plan, raw = self.plan(idx)
        if self.raw:
            return plan, raw
        out = dataprep.run_plan_numpy(plan, raw)
        if not self.no_padding:      # S / 2 rows above and below, a 2S x 2S canvas (240-248): uint8 0 in the image (-1 here), 0 in the mask
            def pad(a, value):
                rows = np.full((self.img_size // 2,) + a.shape[1:], value, a.dtype)
                return np.concatenate([rows, a, rows], axis=0)
            image, mask = pad(out["image"], -1.0), pad(out["mask"], 0.0)
            out = dict(image=image, txt=out["txt"], masked_image=image * (mask < 0.5), mask=mask)
        return out


class InpaintingMultiViewDataset(Dataset):
    def __init__(self, image_path, pair_path, mask_path, mode="train", img_size=256, only_mask_image=False, no_padding=True,
                 token_map=None, view_mask_rate=0.9, test_limit=150, flip=False, constant_place=False, max_ref_view=3, raw=False,
                 **kwargs):
        if mode == "train":
            raise NotImplementedError("InpaintingMultiViewDataset(mode='train'): the reference's own training item cannot be built -- "
                                      "its __getitem__ ends in `pair.split('/')` on the pair dict (line 766), and its random-mask "
                                      "branch reads an undefined `source_crop_info` (line 721); there is no behaviour to reproduce")
        if not no_padding:
            raise NotImplementedError("no_padding=False (the reference raises too, line 735)")
        self.pairs = _val_pairs(image_path, test_limit)
        self.mask_path, self.mode, self.img_size, self.raw = mask_path, mode, img_size, raw
        self.repeat_sp_token = kwargs.get("repeat_sp_token", 0)
        self.sp_token = kwargs.get("sp_token", None)
        self.deep_prompt = kwargs.get("deep_prompt", False)
        self.max_ref_view = max_ref_view
        self.view_num = kwargs.get("view_num", 4)
        self.view_token_len = kwargs.get("view_token_len", 30)
        self.source_shuffle = kwargs.get("source_shuffle", False)
        self.concat_target = kwargs.get("concat_target", False)
        self.mask_list = _by_name(glob(mask_path + "/*"))

    def __len__(self):
        return len(self.pairs)

    collate_raw = staticmethod(dataprep.collate_raw)      # collate_fn of the raw=True items (rawbatch.loader)

    def device_prep(self, device="cuda"):
        """What finishes the collated raw batches on the device: one tile per view, [reference | target] under concat_target."""
        return dataprep.DevicePrep(self.img_size, 2 if self.concat_target else 1, device)

    def get_prompt(self):
        """One prompt per view (per canvas under concat_target): the repeated special token, then that view's direction tokens."""
        if not (self.repeat_sp_token > 0 and self.sp_token is not None) or self.deep_prompt:
            raise NotImplementedError()      # as the reference (604-634)
        text = " ".join(self.sp_token.replace(">", f"{i}>") for i in range(self.repeat_sp_token))
        views = self.view_num - 1 if self.concat_target else self.view_num
        return [text + "".join(f"<view_direct-{j}-{l}>" for l in range(self.view_token_len)) for j in range(views)]

    def plan(self, idx):
        S, pair = self.img_size, self.pairs[idx]
        names = [_pick(pair, stem) for stem in ("source", "source_1", "source_2", "source_3")]
        raw = [_read_rgb(_pick(pair, "target"))]
        # the first view_num - 1 references, shuffled on request (np.random.choice without replacement)
        chosen = np.random.choice(self.view_num - 1, self.view_num - 1, replace=False) if self.source_shuffle else range(self.view_num - 1)
        for i in chosen:
            raw.append(_read_rgb(names[i]))
        own = pair + "/mask.png"
        raw.append(_read_grey(own if os.path.exists(own) else self.mask_list[idx % len(self.mask_list)]))
        target = dataprep.plan_tile(0, S, S, masks=[len(raw) - 1])
        refs = [dataprep.plan_tile(k, S, S, zero_mask=True) for k in range(1, len(raw) - 1)]
        views = [[ref, target] for ref in refs] if self.concat_target else [[target]] + [[ref] for ref in refs]
        return dict(img_size=S, views=views, txt=self.get_prompt(), idx=int(pair.split("/")[-1])), raw

    def __getitem__(self, idx):
        plan, raw = self.plan(idx)
        return (plan, raw) if self.raw else dataprep.run_plan_numpy(plan, raw)


class BalancedRandomSampler(Sampler):
    """MegaDepth is very unbalanced: every epoch takes `n_sample_per_scene` pairs of each scene (the scene is the third path component
    from the end of the source image), shuffles them together and hands rank r every num_replicas-th one."""

    def __init__(self, image_dict, pairs, n_sample_per_scene=100, rank=0, num_replicas=1):
        self.n_sample_per_scene, self.rank, self.epoch, self.num_replicas = n_sample_per_scene, rank, 0, num_replicas
        if rank >= num_replicas or rank < 0:
            raise ValueError("Invalid rank {}, rank should be in the interval [0, {}]".format(rank, num_replicas - 1))
        self.scene_idx = collections.defaultdict(list)
        for i, p in enumerate(pairs):
            self.scene_idx[image_dict[p["source"]].split("/")[-3]].append(i)
        for scene in self.scene_idx:
            if n_sample_per_scene > len(self.scene_idx[scene]):
                raise ValueError("n_sample_per_scene should be less than the min scene sample but got {}>{}".format(
                    n_sample_per_scene, len(self.scene_idx[scene])))
        self.n_scene = len(self.scene_idx)
        total_size = self.n_scene * self.n_sample_per_scene
        if total_size % self.num_replicas != 0:      # the reference's arithmetic, its non-divisible case included
            self.num_samples = math.ceil((total_size - self.num_replicas) / self.num_replicas)
        else:
            self.num_samples = math.ceil(total_size / self.num_replicas)
        self.total_size = self.num_samples * self.num_replicas

    def __iter__(self):
        new_list = []
        random.seed(self.epoch)      # deterministic in the epoch -- and in the epochs before it: the lists are shuffled in place
        for scene in self.scene_idx:
            random.shuffle(self.scene_idx[scene])
            new_list.extend(self.scene_idx[scene][:self.n_sample_per_scene])
        random.shuffle(new_list)
        indices = new_list[:self.total_size]
        assert len(indices) == self.total_size
        indices = indices[self.rank:self.total_size:self.num_replicas]
        assert len(indices) == self.num_samples
        return iter(indices)

    def __len__(self):
        return self.num_samples

    def set_epoch(self, epoch):
        self.epoch = epoch
