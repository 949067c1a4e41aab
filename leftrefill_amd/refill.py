"""Reference-guided inpainting in one call: a photo, a drawn mask and a reference photo in, the filled photo out -- the call pattern of
the reference's ref_inpainting_gradio.py (`predict` 148-211, `pad_image` 142-145, `make_batch_sd` 54-79, `inpaint` 82-138) without
the UI.

Around the sampler the reference does image work on the host with Pillow: three `Image.resize` calls (BICUBIC for source and reference,
BILINEAR for the mask), `> 0 -> 255`, the edge pad to a multiple of 64, the [reference | source] stitch, `convert("L")`, the
threshold and the [-1, 1] mapping; afterwards the composite, the crop, the 8-bit conversion and one more BICUBIC resize.  Pillow's
resampler is exactly specified integer arithmetic, restated here in numpy (`pil_coeffs`, `resample_axis`, `resize_u8`) and pinned
against Pillow itself by the tests; the device route (csrc/pil_resample.hip: lr_pil_resize, lr_refill_canvas, and the existing
lr_eval_metrics for the tail) is held to it bit for bit.  `prepare_numpy` / `finish_numpy` are the statement and, with Pillow doing
the resizes, the host route (`device_prep=False`).

Two generalisations of the reference, which only ever runs at 512: the crop keeps columns `W:` of the H x 2W canvas (the reference
hard-codes `512:`, which is W there), and a `size` that is no multiple of 64 -- or is 64 itself, `pad_image` pads to at least 128 --
is edge-padded, sampled padded, and the padded right half is what the final resize shrinks.
"""
import math

import numpy as np

from . import _lib

FILTER_SUPPORT = {"bicubic": 2.0, "bilinear": 1.0}
PRECISION_BITS = 22            # Pillow's Resample.c: 32 - 8 - 2
MAX_KSIZE = 1025               # LR_PIL_MAX_KSIZE
JOB_DTYPE = np.dtype(_lib.PilJob)      # numpy image of struct lr_pil_job


def _filter(name, x):
    x = np.abs(x)
    if name == "bilinear":
        return np.where(x < 1.0, 1.0 - x, 0.0)
    a = -0.5
    return np.where(x < 1.0, ((a + 2.0) * x - (a + 3.0)) * x * x + 1, np.where(x < 2.0, (((x - 5) * x + 8) * x - 4) * a, 0.0))


def pil_ksize(n_in, n_out, filter):
    return int(math.ceil(FILTER_SUPPORT[filter] * max(n_in / n_out, 1.0))) * 2 + 1


def pil_coeffs(n_in, n_out, filter):
    """Pillow's `precompute_coeffs` + `normalize_coeffs_8bpc` for one axis: (lo int32[n_out], cnt int32[n_out],
    kk int32[n_out][ksize]); output index i reads inputs lo[i] .. lo[i] + cnt[i] - 1 with the 22-bit fixed-point weights kk[i][:cnt[i]]
    (the rest of the row is zero).  All double arithmetic; the weights are summed in index order."""
    scale = n_in / n_out
    fs = max(scale, 1.0)
    support = FILTER_SUPPORT[filter] * fs
    ksize = int(math.ceil(support)) * 2 + 1
    ss = 1.0 / fs              # Pillow multiplies by the reciprocal
    center = (np.arange(n_out, dtype=np.float64) + 0.5) * scale
    lo = np.maximum((center - support + 0.5).astype(np.int64), 0)
    cnt = np.minimum((center + support + 0.5).astype(np.int64), n_in) - lo
    x = np.arange(ksize, dtype=np.float64)[None, :]
    w = _filter(filter, (x + lo[:, None] - center[:, None] + 0.5) * ss)
    w = np.where(x < cnt[:, None], w, 0.0)
    ww = np.zeros(n_out, np.float64)
    for j in range(ksize):      # in index order, as the C loop adds them
        ww = ww + w[:, j]
    w = np.where(ww[:, None] != 0.0, w / np.where(ww == 0.0, 1.0, ww)[:, None], w)
    kk = np.where(w < 0, -0.5 + w * (1 << PRECISION_BITS), 0.5 + w * (1 << PRECISION_BITS)).astype(np.int64)      # truncates toward zero
    return lo.astype(np.int32), cnt.astype(np.int32), kk.astype(np.int32)


def resample_axis(a, n_out, filter, axis):
    """One pass of the resampler along `axis` (0: vertical, 1: horizontal) of a uint8 [h][w][c] array."""
    lo, cnt, kk = pil_coeffs(a.shape[axis], n_out, filter)
    a = np.moveaxis(a, axis, 0).astype(np.int64)
    acc = np.full((n_out,) + a.shape[1:], 1 << (PRECISION_BITS - 1), np.int64)
    for j in range(kk.shape[1]):
        idx = np.minimum(lo.astype(np.int64) + j, a.shape[0] - 1)      # past cnt the weight is zero
        acc += kk[:, j].astype(np.int64).reshape((-1,) + (1,) * (a.ndim - 1)) * a[idx]
    return np.moveaxis(np.clip(acc >> PRECISION_BITS, 0, 255).astype(np.uint8), 0, axis)


def resize_u8(a, w, h, filter):
    """`PIL.Image.resize((w, h), filter)` of a uint8 [hs][ws] or [hs][ws][c] array: the horizontal pass first and only when the width
    changes (it writes a uint8 intermediate), the vertical pass only when the height changes, a copy when neither runs."""
    a = np.asarray(a)
    assert a.dtype == np.uint8 and a.ndim in (2, 3)
    out = a[:, :, None] if a.ndim == 2 else a
    if w != out.shape[1]:
        out = resample_axis(out, w, filter, 1)
    if h != out.shape[0]:
        out = resample_axis(out, h, filter, 0)
    return np.array(out.reshape(out.shape[:a.ndim]), copy=True)


def resize_pil(a, w, h, filter):
    """The same through Pillow itself: the host route and the yardstick."""
    from PIL import Image
    return np.asarray(Image.fromarray(np.ascontiguousarray(a)).resize((w, h), resample=getattr(Image.Resampling, filter.upper())))


def plan(source_hw, size=512):
    """Sizes of one call: the square (Sh, Sw) every input is resized to ("directly resizing", reference 167), the padded (H, W) of
    `pad_image` -- each side rounded up to a multiple of 64, at least 128 --, the canvas H x 2W and the result's (width, height)
    `(int(size / ratio), size)` with ratio = origin_h / origin_w (reference 151, 207)."""
    origin_h, origin_w = int(source_hw[0]), int(source_hw[1])
    size = int(size)
    side = max(2, -(-size // 64)) * 64
    ratio = origin_h / origin_w
    return dict(size=size, Sh=size, Sw=size, H=side, W=side, canvas=(side, 2 * side), out_wh=(int(size / ratio), size))


def pad_edge(a, H, W):
    """`np.pad(a, ((0, H - h), (0, W - w), (0, 0)), mode="edge")` as an index statement: out[y][x] = a[min(y, h - 1)][min(x, w - 1)]."""
    return a[np.minimum(np.arange(H), a.shape[0] - 1)][:, np.minimum(np.arange(W), a.shape[1] - 1)]


def luma_mask(rgb):
    """`convert("L")` of an RGB uint8 array, `/ 255.0` in fp32, `>= 0.5`: L = (19595 R + 38470 G + 7471 B + 32768) >> 16, 1 where
    L >= 128 (127 / 255 < 0.5 <= 128 / 255 in fp32)."""
    v = rgb.astype(np.int64)
    L = (19595 * v[..., 0] + 38470 * v[..., 1] + 7471 * v[..., 2] + 32768) >> 16
    return (L >= 128).astype(np.float32)


def prepare_numpy(source_rgb, mask_rgb, reference_rgb, size=512, n=1, resize=resize_u8):
    """The reference's `predict` 167-188 and `make_batch_sd` on uint8 RGB arrays -> (image, masked_image [n,3,H,2W], mask [n,1,H,2W])
    fp32, NCHW, the n copies identical.  `resize(a, w, h, filter)`: `resize_u8` (the numpy statement) or `resize_pil`."""
    p = plan(source_rgb.shape[:2], size)
    src = resize(source_rgb, p["Sw"], p["Sh"], "bicubic")
    ref = resize(reference_rgb, p["Sw"], p["Sh"], "bicubic")
    m = resize(mask_rgb, p["Sw"], p["Sh"], "bilinear")
    m = np.where(m > 0, 255, 0).astype(np.uint8)
    src, ref, m = (pad_edge(a, p["H"], p["W"]) for a in (src, ref, m))
    canvas = np.concatenate([ref, src], axis=1)
    mask = luma_mask(np.concatenate([np.zeros_like(m), m], axis=1))[None, None]
    image = (canvas.astype(np.float32) / np.float32(127.5) - np.float32(1.0)).transpose(2, 0, 1)[None]
    masked = image * (mask < 0.5).astype(np.float32)
    rep = lambda a: np.ascontiguousarray(np.repeat(a, n, axis=0))
    return rep(image), rep(masked), rep(mask)


def finish_numpy(pred, image, mask, out_wh, resize=resize_u8):
    """The reference's `inpaint` 131-138 and `predict` 207 on fp32 arrays [N,3,H,2W] / [N,1,H,2W]: the composite, columns W: of the
    canvas, `clamp((x + 1) / 2, 0, 1) * 255` truncated to uint8 HWC, a bicubic resize to out_wh = (width, height).  -> list of arrays."""
    pred, image, mask = (np.asarray(a, np.float32) for a in (pred, image, mask))
    x = pred * mask + image * (np.float32(1.0) - mask)
    W = x.shape[3] // 2
    x = np.clip((x[:, :, :, W:] + np.float32(1.0)) / np.float32(2.0), np.float32(0.0), np.float32(1.0)) * np.float32(255.0)
    x = x.transpose(0, 2, 3, 1).astype(np.uint8)
    return [resize(np.ascontiguousarray(a), out_wh[0], out_wh[1], "bicubic") for a in x]


def prompt(repeat_sp_token=50, sp_token="<special-token>"):
    """`repeat_sp_token` copies of the special token with the index spliced in before the `>` (reference 190-193)."""
    return " ".join(sp_token.replace(">", f"{i}>") for i in range(repeat_sp_token))


# ---- the device route: job tables for lr_pil_resize ----------------------------------------------------------------------------------

_COEFFS = {}


def _coeffs_cached(n_in, n_out, filter):
    key = (n_in, n_out, filter)
    if key not in _COEFFS:
        if len(_COEFFS) > 64:
            _COEFFS.clear()
        _COEFFS[key] = pil_coeffs(n_in, n_out, filter)
    return _COEFFS[key]


class ResizeTable:
    """The int32 table arena and the job table of one lr_pil_resize call.  `add(src_off, (hs, ws, c), (w, h), filter)` plans one job and
    returns the byte offset of its [h][w][c] result in the destination; intermediates are given room in the workspace."""

    def __init__(self):
        self.words, self.n_words, self.axis_at = [], 0, {}
        self.jobs, self.work_bytes, self.dst_bytes = [], 0, 0

    def _axis(self, n_in, n_out, filter):
        key = (n_in, n_out, filter)
        if key not in self.axis_at:      # jobs of equal geometry share their rows
            lo, cnt, kk = _coeffs_cached(*key)
            self.axis_at[key] = (self.n_words, kk.shape[1])
            self.words += [lo, cnt, kk.reshape(-1)]
            self.n_words += 2 * n_out + kk.size
        return self.axis_at[key]

    def add(self, src_off, shape, wh, filter):
        hs, ws, c = shape
        wd, hd = wh
        h_off, h_ksize = self._axis(ws, wd, filter) if wd != ws else (0, 0)
        v_off, v_ksize = self._axis(hs, hd, filter) if hd != hs else (0, 0)
        tmp_off = 0
        if h_ksize and v_ksize:
            tmp_off, self.work_bytes = self.work_bytes, self.work_bytes + hs * wd * c
        dst_off, self.dst_bytes = self.dst_bytes, self.dst_bytes + hd * wd * c
        self.jobs.append((src_off, tmp_off, dst_off, h_off, v_off, hs, ws, hd, wd, c, h_ksize, v_ksize, 0))
        return dst_off

    def arrays(self):
        tables = np.concatenate(self.words).astype(np.int32) if self.words else np.zeros(0, np.int32)
        return tables, np.array(self.jobs, dtype=JOB_DTYPE)


def refused(shape, wh, filter):
    """True when lr_pil_resize answers LR_E_UNSUPPORTED for this job: a coefficient row longer than LR_PIL_MAX_KSIZE."""
    return (wh[0] != shape[1] and pil_ksize(shape[1], wh[0], filter) > MAX_KSIZE) or \
        (wh[1] != shape[0] and pil_ksize(shape[0], wh[1], filter) > MAX_KSIZE)


def device_resize(sources, sizes, filters, device, timing=None):
    """A batch of `PIL.Image.resize` jobs in one lr_pil_resize call (at most two launches).  sources: uint8 host arrays [h][w][c]
    (packed into one arena and uploaded) or ONE uint8 device tensor [N][h][w][c] whose N images are the jobs' sources; sizes:
    (width, height) per job; filters: a name per job.  A job the library would refuse is resized on the host and uploaded as a copy job.
    -> the list of uint8 device tensors [h][w][c] (views of one destination buffer).  timing: dict that collects host seconds of 'pack'
    and 'copy' (the caller times the launches around its own synchronisation)."""
    import time

    import torch

    from . import ops, rawbatch
    t0 = time.perf_counter()
    table = ResizeTable()
    on_device = torch.is_tensor(sources)
    pin = torch.cuda.is_available()
    shapes, offs = [], []
    if on_device:
        assert sources.is_cuda and sources.dtype == torch.uint8 and sources.dim() == 4 and sources.is_contiguous()
        per = sources[0].numel()
        for i in range(sources.shape[0]):
            assert not refused(tuple(sources.shape[1:]), sizes[i], filters[i]), "a device source the library refuses: resize it on the host"
            shapes.append(tuple(sources.shape[1:]))
            offs.append(i * per)
        src_dev = sources.reshape(-1)
    else:
        arena = rawbatch.Arena(1)
        for a, wh, f in zip(sources, sizes, filters):
            a = a[:, :, None] if a.ndim == 2 else a
            if refused(a.shape, wh, f):
                a = resize_pil(a.reshape(a.shape[:2]) if a.shape[2] == 1 else a, wh[0], wh[1], f).reshape(wh[1], wh[0], a.shape[2])
            shapes.append(a.shape)
            offs.append(arena.add(a))
        src_host = arena.tensor(pin)
    out_at = [table.add(o, s, wh, f) for o, s, wh, f in zip(offs, shapes, sizes, filters)]
    tables, jobs = table.arrays()
    tables_host = torch.from_numpy(tables) if tables.size else torch.zeros(4, dtype=torch.int32)
    tables_host = tables_host.pin_memory() if pin else tables_host
    jobs_host = rawbatch.table_tensor(jobs, pin)
    t1 = time.perf_counter()
    if not on_device:
        src_dev = src_host.to(device, non_blocking=True)
    tables_dev, jobs_dev = tables_host.to(device, non_blocking=True), jobs_host.to(device, non_blocking=True)
    work = torch.empty(max(16, table.work_bytes), dtype=torch.uint8, device=device)
    dst = torch.empty(max(16, table.dst_bytes), dtype=torch.uint8, device=device)
    if timing is not None:
        torch.cuda.synchronize(device)
        t2 = time.perf_counter()
        timing["pack"] = timing.get("pack", 0.0) + t1 - t0
        timing["copy"] = timing.get("copy", 0.0) + t2 - t1
    with torch.cuda.device(device):
        ops.pil_resize(src_dev, tables_dev, tables_host, jobs_dev, jobs_host, len(jobs), work, dst)
    return [dst[o:o + wh[1] * wh[0] * s[2]].view(wh[1], wh[0], s[2]) for o, wh, s in zip(out_at, sizes, shapes)]


def prepare_device(sources, masks, references, size, n, device, timing=None):
    """`prepare_numpy` of P pairs on the device: 3 P resize jobs in one lr_pil_resize call, then one lr_refill_canvas launch.
    -> (image, masked_image [P n,3,H,2W], mask [P n,1,H,2W]) fp32 device tensors, each pair's n copies adjacent."""
    import torch

    from . import ops
    P = len(sources)
    p = plan(sources[0].shape[:2], size)
    S = p["size"]
    outs = device_resize(list(references) + list(sources) + list(masks), [(S, S)] * (3 * P), ["bicubic"] * (2 * P) + ["bilinear"] * P,
                         device, timing)
    # the 3 P results are adjacent in the destination buffer, in job order: [3][P][S][S][3]
    base = outs[0]
    whole = torch.as_strided(base, (3, P, S, S, 3), (P * S * S * 3, S * S * 3, S * 3, 3, 1))
    with torch.cuda.device(device):
        return ops.refill_canvas(whole[0], whole[1], whole[2], p["H"], p["W"], n)


def finish_device(pred, image, mask, out_whs, timing=None):
    """`finish_numpy` on the device: lr_eval_metrics forms the truncated 8-bit composite of the right half, lr_pil_resize does the final
    bicubic resizes (out_whs: one (width, height) per sample).  -> list of uint8 host arrays."""
    import torch

    from . import ops
    W = pred.shape[3] // 2
    with torch.cuda.device(pred.device):
        _, rgb8 = ops.eval_metrics(pred, image, mask, x0=W, Wc=W, r=1, want_rgb8=True)
    host = [i for i, wh in enumerate(out_whs) if refused(tuple(rgb8.shape[1:]), wh, "bicubic")]
    if host:      # a coefficient row longer than the library takes: the batch's final resizes run on the host
        arrays = rgb8.cpu().numpy()
        return [resize_pil(arrays[i], wh[0], wh[1], "bicubic") for i, wh in enumerate(out_whs)]
    outs = device_resize(rgb8, list(out_whs), ["bicubic"] * len(out_whs), pred.device, timing)
    return [o.cpu().numpy() for o in outs]


def _rgb(img):
    from PIL import Image
    if not isinstance(img, Image.Image):
        img = Image.fromarray(np.asarray(img, np.uint8))
    return np.asarray(img.convert("RGB"))


def sample_latents(model, image, masked_image, mask, txt, steps, scale, seeds, num_samples, sampler=None, attn=None, noise="torch"):
    """The reference's `inpaint` 88-130 on a prepared batch (NCHW fp32 device tensors of P * num_samples canvases): conditioning, the
    seeded start code, DDIM at eta 1 with classifier-free guidance, the VAE decode.  -> the decoded prediction [N,3,H,2W].
    attn: a dict to fill with the reference-attention maps of the sampling (`refill(return_attn=True)`), or None.
    noise: "torch" -- the start code from numpy.random.RandomState(seed), everything else from torch's global generators, as in the
    reference; "seeded" -- sample j of the pair with seed s has the key (s, j) of leftrefill_amd/noise.py, and the posterior sample
    of the masked-image encoding, the start code and the noise of every step are that key's draws (lr_seeded_normal)."""
    import torch
    import torch.nn.functional as F
    from ldm.models.diffusion.ddim import DDIMSampler
    N, _, H, W2 = image.shape
    h, w = H // 8, W2 // 8
    if noise not in ("torch", "seeded"):
        raise ValueError(f"noise: 'torch' or 'seeded', not {noise!r}")
    sn = None
    if noise == "seeded":
        from .noise import POSTERIOR, SeededNoise
        sn = SeededNoise([s for s in seeds for _ in range(num_samples)], subs=list(range(num_samples)) * len(seeds), device=image.device)
        assert len(sn) == N
    batch = {"image": image, "masked_image": masked_image, "mask": mask}
    c = model.cond_stage_model.encode([txt] * N)
    c_cat = []
    for ck in model.concat_keys:
        cc = batch[ck].float()
        if ck != model.masked_image_key:
            cc = F.interpolate(cc, size=(h, w))
        else:
            posterior = model.encode_first_stage(cc)
            if sn is not None and hasattr(posterior, "mean"):
                cc = model.get_first_stage_encoding(posterior, noise=sn.normal(POSTERIOR, 0, posterior.mean.shape[1:]))
            else:
                cc = model.get_first_stage_encoding(posterior)
        c_cat.append(cc)
    c_cat = torch.cat(c_cat, dim=1)
    cond = {"c_concat": [c_cat], "c_crossattn": [c]}
    uc_full = {"c_concat": [c_cat], "c_crossattn": [model.get_unconditional_conditioning(N)]}
    start = None
    if sn is None:
        start = np.concatenate([np.random.RandomState(s).randn(num_samples, 4, h, w) for s in seeds], axis=0)
        start = torch.from_numpy(start).to(device=image.device, dtype=torch.float32)
    sampler = DDIMSampler(model) if sampler is None else sampler
    import contextlib
    probe = contextlib.nullcontext()
    if attn is not None:
        from .attnprobe import AttentionProbe
        probe = AttentionProbe(model.model.diffusion_model)
    with probe:
        samples, _ = sampler.sample(steps, N, [model.channels, h, w], cond, verbose=False, eta=1.0, unconditional_guidance_scale=scale,
                                    unconditional_conditioning=uc_full, x_T=start, seeds=sn)
    if attn is not None:
        # the conditional half of the guided [uncond; cond] batch (all of it at scale 1): the maps of the pass that saw the prompt
        rows = slice(N, 2 * N) if float(scale) != 1. else slice(0, N)
        attn["mass"] = [probe.mass(l)[rows][:, :, probe.raw(l).shape[2] // 2:2 * (probe.raw(l).shape[2] // 2)] for l in probe.recorded]
        attn["correspondence"] = [probe.correspondence(l)[rows] for l in probe.recorded]
    return model.decode_first_stage(samples)


def refill(model, source, mask, reference, steps=50, scale=2.5, seed=0, num_samples=1, size=512, device_prep=True, sampler=None,
           return_attn=False, noise="torch"):
    """Fill the masked part of `source` guided by `reference`: `predict` of the reference's ref_inpainting_gradio.py.

    source, mask, reference: PIL images or uint8 arrays (`.convert("RGB")` is host work on both routes), or lists of equal length: a
    batch of P pairs sampled together at UNet batch 2 * P * num_samples; `seed` is then an int or one int per pair.  Returns the list
    of `num_samples` PIL images of size `(int(size / ratio), size)` -- for lists, one such list per pair.

    Randomness, noise="torch" (the default, the reference's behaviour): the start code of a pair is
    `numpy.random.RandomState(seed).randn(num_samples, 4, H / 8, 2W / 8)`; the sample of the VAE posterior and the eta = 1 noise of every
    DDIM step come from torch's global generators.
    noise="seeded": sample j of a pair with seed s has the key (s, j) of leftrefill_amd/noise.py, and the start code, the noise of every
    step and the posterior sample of the masked-image encoding are that key's draws (one lr_seeded_normal launch each).  The result
    then depends only on the inputs and the seed -- not on torch's or numpy's generators, on what ran before, on the pair's place in
    the batch or on the pairs beside it -- up to the UNet's batch-dependent kernel plans: a pair sampled alone and in a batch gets
    bit-identical noise, but its latents may differ in the last fp16 bits where a GEMM's plan depends on the batch size.

    device_prep=True: resizes, canvas, composite and 8-bit tail are HIP kernels (lr_pil_resize, lr_refill_canvas, lr_eval_metrics);
    an image whose resize the library refuses is resized on the host and uploaded.  device_prep=False: `prepare_numpy` / `finish_numpy`
    with Pillow doing the resizes; the stages between are the same code, and the two routes return the same bytes.
    `steps` goes to DDIM's uniform schedule as it is: the stride `1000 // steps` must keep the last timestep inside the table (50, 20,
    4 do; 3 does not, here as in the reference).  `sampler` is reserved: a ready `DDIMSampler(model)` to reuse, nothing else.

    return_attn=True: returns `(images, attn)`; the sampling runs under a leftrefill_amd.attnprobe.AttentionProbe (the UNet's eager
    route: same launches, same images).  attn = {"mass": [...], "correspondence": [...]}: per self-attention layer of the UNet (execution
    order) a CUDA tensor [N, h, w // 2] over the (padded, `plan`) target half of the latent canvas -- how much of its attention each
    target token puts on the reference half, head and step mean of the prompted pass -- and [N, h, w // 2, 2], the (x, y) inside the reference half it looks at (token units, nan where
    the mass is 0); N = all samples of all pairs, in the order of the returned images.  Nothing is read back."""
    import torch
    from PIL import Image

    import leftrefill_amd.dropin as dropin
    dropin.install()
    single = not isinstance(source, (list, tuple))
    sources, masks, references = ([x] if single else list(x) for x in (source, mask, reference))
    P = len(sources)
    assert P >= 1 and len(masks) == P and len(references) == P, "source, mask and reference: lists of equal length"
    seeds = [int(seed)] * P if isinstance(seed, (int, np.integer)) else [int(s) for s in seed]
    assert len(seeds) == P, "seed: an int or one per pair"
    sources, masks, references = ([_rgb(x) for x in xs] for xs in (sources, masks, references))
    plans = [plan(s.shape[:2], size) for s in sources]
    n = int(num_samples)
    data_cfg = getattr(model, "data_cfg", None) or {}
    txt = prompt(int(data_cfg.get("repeat_sp_token", 50)), data_cfg.get("sp_token", "<special-token>"))
    device = next(model.parameters()).device
    out_whs = [pl["out_wh"] for pl in plans for _ in range(n)]
    with torch.no_grad(), torch.autocast("cuda"):
        if device_prep:
            image, masked_image, mask_t = prepare_device(sources, masks, references, size, n, device)
        else:
            parts = [prepare_numpy(s, m, r, size, n, resize=resize_pil) for s, m, r in zip(sources, masks, references)]
            image, masked_image, mask_t = (torch.from_numpy(np.concatenate([p[k] for p in parts], axis=0)).to(device) for k in range(3))
        attn = {} if return_attn else None
        pred = sample_latents(model, image, masked_image, mask_t, txt, steps, scale, seeds, n, sampler, attn=attn, noise=noise)
        if device_prep:
            arrays = finish_device(pred, image, mask_t, out_whs)
        else:
            arrays = []
            for i, wh in enumerate(out_whs):
                arrays += finish_numpy(pred[i:i + 1].float().cpu().numpy(), image[i:i + 1].cpu().numpy(), mask_t[i:i + 1].cpu().numpy(), wh,
                                       resize=resize_pil)
    images = [Image.fromarray(a) for a in arrays]
    groups = [images[i * n:(i + 1) * n] for i in range(P)]
    out = groups[0] if single else groups
    return (out, attn) if return_attn else out
