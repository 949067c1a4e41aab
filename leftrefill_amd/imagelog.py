"""The image grid of the training logger, stated in numpy: what the reference's `InpaintingLogger.log_local` (inpainting_ldm/logger.py:43-71)
computes for a dict of logged image batches, and the yardstick of the HIP kernel that writes the same bytes in one launch
(csrc/image_grid.hip: lr_image_grid; leftrefill_amd.ops.image_grid).

    canvas = grid_numpy({"masked_image": a, "origin_image": b, "pred": c})      # uint8 [Hc, Wc, 3], ready for Image.fromarray

Per key, in the order of KEYS: cut to N = min(B, max_images) images, `torchvision.utils.make_grid(t, nrow=1, padding=2, pad_value=0)`
restated (torchvision is not a dependency of this tree, so the layout is restated from its documentation and source, not pinned against
it): one channel is repeated to three; ONE image is returned as it is, unpadded; N > 1 images sit below each other in a
[3, N (H + 2) + 2, W + 4] array of zeros, image k at rows k (H + 2) + 2 and columns 2.  Then, all in fp32 and in this order,
clamp(x, -1, 1), (g + 1.0) / 2.0 (the padding value 0 becomes grey 127), * 255, truncation to uint8; the per-key grids are concatenated
along the width.

16-bit inputs are widened to fp32 first; the reference would compute in the input's dtype (its logged tensors are fp32 in practice).

Generalisation: a 5-D entry [B, V, C, H, W] (the multi-view model's `reference`) makes the reference's make_grid raise; here its V views
are laid side by side as V consecutive sources of the same N and H.
"""
import numpy as np

KEYS = ('masked_image', 'origin_image', 'control', 'warp_image', 'pred', 'reference')
PADDING = 2           # make_grid's default
MAX_SOURCES = 8       # LR_GRID_MAX_SOURCES: sources of one lr_image_grid launch


def sources_of(images, keys=KEYS, max_images=4):
    """The 4-D sources [N, C, H, W] of the canvas, left to right: the entries of `images` named by `keys`, in the order of `keys`, each
    cut to its first min(B, max_images) images; a 5-D entry [B, V, C, H, W] gives V sources.  Slices only: numpy arrays and torch
    tensors both stay views of what was passed."""
    out = []
    for k in keys:
        if k not in images:
            continue
        t = images[k]
        if t.ndim == 5:
            out.extend(t[:max_images, v] for v in range(t.shape[1]))
        elif t.ndim == 4:
            out.append(t[:max_images])
        else:
            raise ValueError(f"{k}: [B, C, H, W] or [B, V, C, H, W] expected, got {tuple(t.shape)}")
    if not out:
        raise ValueError(f"none of {tuple(keys)} is among the logged images {tuple(images)}")
    N, H = out[0].shape[0], out[0].shape[2]
    for s in out:
        if s.shape[1] not in (1, 3):
            raise ValueError(f"1 or 3 channels expected, got {s.shape[1]}")
        if s.shape[0] != N or s.shape[2] != H:
            raise ValueError(f"every source needs the same image count and height: {tuple(s.shape)} against N = {N}, H = {H}")
    return out


def canvas_layout(widths, N, H):
    """(Hc, Wc, cols): the canvas of sources of widths `widths`, N images of H rows each, and every source's first canvas column (of its
    grid, padding included)."""
    pad = 0 if N == 1 else PADDING
    cols, x = [], 0
    for w in widths:
        cols.append(x)
        x += w + 2 * pad
    return (H if N == 1 else N * (H + pad) + pad), x, cols


def make_grid_numpy(t):
    """make_grid(t, nrow=1, padding=2, pad_value=0) of fp32 [N, C, H, W], C in {1, 3} -> fp32 [3, Hg, Wg]."""
    N, C, H, W = t.shape
    if C == 1:
        t = np.repeat(t, 3, axis=1)
    if N == 1:
        return t[0]
    g = np.zeros((3, N * (H + PADDING) + PADDING, W + 2 * PADDING), np.float32)
    for k in range(N):
        y = k * (H + PADDING) + PADDING
        g[:, y:y + H, PADDING:PADDING + W] = t[k]
    return g


def to_uint8(g, rescale=True):
    """The reference's three fp32 operations and the truncation: (g + 1.0) / 2.0 when rescale, * 255, astype(uint8)."""
    g = np.asarray(g, np.float32)
    if rescale:
        g = (g + np.float32(1.0)) / np.float32(2.0)
    return (g * np.float32(255)).astype(np.uint8)


def grid_numpy(images, keys=KEYS, max_images=4, clamp=True, rescale=True):
    """uint8 [Hc, Wc, 3] canvas of the logged `images` (name -> array [B, C, H, W] or [B, V, C, H, W], values in [-1, 1] when rescale,
    [0, 1] otherwise).  Non-finite values raise ValueError, and so do, with clamp=False, values whose 8-bit image the reference leaves
    undefined (outside [-1, 1] with rescale, outside [0, 1] without)."""
    grids = []
    for s in sources_of(images, keys, max_images):
        t = np.asarray(s).astype(np.float32)      # 16-bit inputs: widened first
        if not np.isfinite(t).all():
            raise ValueError("grid_numpy: non-finite values have no 8-bit image")
        if clamp:
            t = np.clip(t, np.float32(-1.0), np.float32(1.0))
        lo = -1.0 if rescale else 0.0
        if t.min() < lo or t.max() > 1.0:
            raise ValueError(f"grid_numpy: values outside [{lo:g}, 1] have no defined 8-bit image (clamp={clamp}, rescale={rescale})")
        grids.append(to_uint8(make_grid_numpy(t), rescale).transpose(1, 2, 0))
    return np.ascontiguousarray(np.concatenate(grids, axis=1))


def token_drift_numpy(old, new):
    """float64 [T]: how far each token moved, sqrt(sum((old - new)^2, axis=1)) (reference logger.py:119-122)."""
    d = np.asarray(old, np.float64) - np.asarray(new, np.float64)
    return np.sqrt((d * d).sum(axis=1))
