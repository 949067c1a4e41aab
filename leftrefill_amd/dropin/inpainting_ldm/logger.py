"""`inpainting_ldm.logger.InpaintingLogger` -- the reference's training image logger (inpainting_ldm/logger.py) as a callback of
leftrefill_amd.trainer.Trainer: every `batch_frequency` batches it samples the current batch with the prompt tokens as they are, writes
a JPEG grid `masked_image | origin_image | pred` under <logger.save_dir>/<save_dir>/<split>/, and logs how far each learned token moved
since the last look.

Same constructor arguments, defaults, methods and file names as the reference.  What differs is where the work happens:

  device route (CUDA tensors, `device=True`): the whole canvas -- per-key make_grid, clamp, rescale, 8-bit -- is ONE launch of
      lr_image_grid into a persistent uint8 buffer, read straight from the logged tensors through their strides (`masked_image` is an NHWC
      view, `pred` is NCHW: neither is copied), then one `.cpu()` of the canvas; the token drift and the refresh of the snapshot are one
      launch of lr_token_drift, and the distances go to `pl_module.log` as views of one device tensor (no `.item()`: nothing is read
      back, as with everything else leftrefill_amd.trainer.Trainer keeps in `logged`).
  host route (CPU tensors, or `device=False`, the one extra keyword): leftrefill_amd.imagelog.grid_numpy -- the reference's arithmetic
      stated in numpy -- and torch on the host.

Both routes produce the same array and therefore the same file.

Stated deviations: a 5-D entry [B, V, C, H, W] (the multi-view model's `reference`) is laid out as V columns where the reference's
make_grid raises; `mapping_color` keeps its signature and imports matplotlib only when called; an `att_scores` entry (a list with one
[N, h, w] map in [0, 1] per attention layer, what `log_images(return_attn=True)` hands out) is drawn as the reference draws it
(logger.py:47-58: nearest resize, `make_grid(nrow=1, padding=2)`, viridis over [0, 1], appended to the right of the canvas) except
that the maps are resized to the logged images' [H, W] -- the reference resizes to a fixed 512 x 512, which only concatenates with
the other grids when H = 512.  The image keys keep their route; the attention panels are host work (matplotlib's colour map).
"""
import os

import numpy as np
import torch
from PIL import Image

from leftrefill_amd import imagelog


def mapping_color(img, vmin, vmax, cmap="rainbow"):
    import matplotlib.pyplot as plt      # only the att_scores panels call this
    from matplotlib import cm
    np_img = img
    if vmin is not None and vmax is not None:
        np_img = plt.Normalize(vmin=vmin, vmax=vmax)(np_img)
    mapped_img = getattr(cm, cmap)(np_img)
    results = mapped_img[:, :, 0:3]
    return results


def _process_rank():
    """Lightning's rank_zero_only reads the launcher's environment."""
    for key in ("RANK", "LOCAL_RANK"):
        if os.environ.get(key) is not None:
            return int(os.environ[key])
    return 0


class InpaintingLogger:
    def __init__(self, batch_frequency=2000, max_images=4, clamp=True, increase_log_steps=True,
                 rescale=True, disabled=False, log_on_batch_idx=False, log_first_step=False,
                 log_images_kwargs=None, save_dir='image_log', device=True):
        self.rescale = rescale
        self.batch_freq = batch_frequency
        self.max_images = max_images
        if not increase_log_steps:
            self.log_steps = [self.batch_freq]
        self.clamp = clamp
        self.disabled = disabled
        self.log_on_batch_idx = log_on_batch_idx
        self.log_images_kwargs = log_images_kwargs if log_images_kwargs is not None else {}
        self.log_first_step = log_first_step
        self.save_dir = save_dir
        self.device = device
        self.special_tokens = None
        self.special_token_embeddings_old = None
        self._canvas = None      # the persistent uint8 canvas of the device route
        self._drift = None       # the persistent fp32 [T] distances of the device route

    # ---- the canvas ----------------------------------------------------------------------------------------------------------------------
    def canvas(self, images):
        """uint8 [Hc, Wc, 3] numpy canvas of the logged images, by the device route when every entry is a CUDA tensor and `device`."""
        att = images.get('att_scores')
        images = {k: v for k, v in images.items() if k in imagelog.KEYS and torch.is_tensor(v)}
        if att:
            first = next(images[k] for k in imagelog.KEYS if k in images)
            return np.concatenate([self._image_canvas(images), self.attention_panels(att, first.shape[-2], first.shape[-1])], axis=1)
        return self._image_canvas(images)

    def attention_panels(self, att_scores, H, W):
        """uint8 [Hc, n (W + 2 pad), 3]: one viridis panel per attention map [N, h, w] (values in [0, 1]; the first max_images are drawn),
        nearest-resized to [H, W] and laid out like an image key (reference logger.py:51-58)."""
        panels = []
        for a in att_scores:
            a = a[:min(a.shape[0], self.max_images)].detach().float().cpu()
            a = torch.nn.functional.interpolate(a.unsqueeze(1), size=[H, W], mode='nearest').numpy()
            grid = imagelog.make_grid_numpy(a)[0]
            panels.append((mapping_color(grid, 0, 1, cmap="viridis") * 255).astype(np.uint8))
        return np.concatenate(panels, axis=1)

    def _image_canvas(self, images):
        if self.device and images and all(v.is_cuda for v in images.values()):
            from leftrefill_amd import ops
            sources = [s.detach() for s in imagelog.sources_of(images, max_images=self.max_images)]
            N, H = sources[0].shape[0], sources[0].shape[2]
            Hc, Wc, _ = imagelog.canvas_layout([s.shape[3] for s in sources], N, H)
            if self._canvas is None or tuple(self._canvas.shape) != (Hc, Wc, 3) or self._canvas.device != sources[0].device:
                self._canvas = torch.empty(Hc, Wc, 3, device=sources[0].device, dtype=torch.uint8)
            return ops.image_grid(sources, N, H, self.clamp, self.rescale, out=self._canvas).cpu().numpy()
        host = {k: v.detach().float().cpu().numpy() for k, v in images.items()}      # 16-bit entries: widened first
        return imagelog.grid_numpy(host, max_images=self.max_images, clamp=self.clamp, rescale=self.rescale)

    def log_local(self, save_dir, split, images, global_step, current_epoch, batch_idx):
        if _process_rank() != 0:
            return
        root = os.path.join(save_dir, self.save_dir, split)
        grids = self.canvas(images)
        filename = "gs-{:06}_e-{:06}_b-{:06}.jpg".format(global_step, current_epoch, batch_idx)
        path = os.path.join(root, filename)
        os.makedirs(os.path.split(path)[0], exist_ok=True)
        Image.fromarray(grids).save(path)

    def log_img(self, pl_module, batch, batch_idx, split="train"):
        check_idx = batch_idx
        if (self.check_frequency(check_idx) and
                hasattr(pl_module, "log_images") and
                callable(pl_module.log_images) and
                self.max_images > 0):
            is_train = pl_module.training
            if is_train:
                pl_module.eval()

            with torch.no_grad():
                images = pl_module.log_images(batch, split=split, **self.log_images_kwargs)

            for k in images:      # views; clamp, cut to max_images and the move to the host happen where the canvas is made
                if k == 'att_scores':
                    images[k] = [a[:min(a.shape[0], self.max_images)].detach() for a in images[k]]
                elif torch.is_tensor(images[k]):
                    images[k] = images[k][:min(images[k].shape[0], self.max_images)].detach()

            if pl_module.local_rank == 0:
                self.log_local(pl_module.logger.save_dir, split, images,
                               pl_module.global_step, pl_module.current_epoch, batch_idx)

            if is_train:
                pl_module.train()

    def check_frequency(self, check_idx):
        return check_idx % self.batch_freq == 0

    # ---- how far the learned tokens moved ---------------------------------------------------------------------------------------------------
    def _log_drift(self, pl_module, weight):
        weight = weight.detach()
        old = self.special_token_embeddings_old
        if self.device and weight.is_cuda and weight.dtype == torch.float32 and weight.is_contiguous():
            from leftrefill_amd import ops
            if self._drift is None or self._drift.numel() != weight.shape[0] or self._drift.device != weight.device:
                self._drift = torch.empty(weight.shape[0], device=weight.device, dtype=torch.float32)
            ops.token_drift(old, weight, out=self._drift)      # the distances, and old <- weight
            for j, special_token in enumerate(self.special_tokens):
                pl_module.log(f'special_tokens/{special_token}', self._drift[j], on_step=True)
            return
        d = torch.sqrt(torch.sum((old.float() - weight.float()) ** 2, dim=1))
        for j, special_token in enumerate(self.special_tokens):
            pl_module.log(f'special_tokens/{special_token}', d[j].item(), on_step=True)
        self.special_token_embeddings_old = weight.clone()

    def on_train_batch_end(self, trainer, pl_module, outputs, batch, batch_idx, dataloader_idx):
        if not self.disabled:
            self.log_img(pl_module, batch, batch_idx, split="train")

        cond = getattr(pl_module, "cond_stage_model", None)
        if batch_idx % trainer.log_every_n_steps == 0 and hasattr(cond, 'special_tokens'):
            if self.special_token_embeddings_old is None:
                self.special_tokens = cond.special_tokens
                self.special_token_embeddings_old = cond.special_embeddings.weight.detach().clone()
            else:
                self._log_drift(pl_module, cond.special_embeddings.weight)
