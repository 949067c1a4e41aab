"""What the raw data routes share.  A `raw=True` dataset hands out `(plan, raw)` items; its collate function packs the batch's uint8
sources into one byte arena (`Arena`) and its decisions into a job table (`table_tensor`); a device-prep object (`DevicePrepBase`)
uploads both and finishes the batch with one HIP launch; `DevicePrepLoader` chains the two and `loader` builds the chain from a
dataset, which names its own collate function (`collate_raw`) and device prep (`device_prep(device)`: canvas size and tile count).
The routes themselves -- job structs, plans, numpy statements, entries -- are dataprep.py (lr_batch_prep) and nvsprep.py (lr_nvs_prep).
"""
import numpy as np
import torch

from . import _lib


def default_pin(pin):
    """A collate function's `pin` argument: None means page-locked memory when a GPU is present and this is not a loader worker (in a
    worker leave it to `DataLoader(pin_memory=True)`)."""
    from torch.utils.data import get_worker_info
    return bool(get_worker_info() is None and torch.cuda.is_available() if pin is None else pin)


def table_tensor(jobs, pin):
    """The bytes of a structured job array as a uint8 tensor."""
    table = torch.empty(jobs.nbytes, dtype=torch.uint8, pin_memory=pin)
    table.numpy()[:] = jobs.view(np.uint8).reshape(-1)
    return table


class Arena:
    """The byte arena of a batch: every source at the next multiple of `align`; the tensor ends on a multiple of 16 (at least 16 bytes)
    and every byte that is not source data is zero."""

    def __init__(self, align):
        self.align, self.end, self.placed = align, 0, []

    def add(self, arr):
        arr = np.ascontiguousarray(arr)
        assert arr.dtype == np.uint8, "raw sources are uint8"
        off = -(-self.end // self.align) * self.align
        self.placed.append((off, arr))
        self.end = off + arr.size
        return off

    def tensor(self, pin):
        out = torch.empty(max(16, -(-self.end // 16) * 16), dtype=torch.uint8, pin_memory=pin)
        view, at = out.numpy(), 0
        for off, arr in self.placed:
            view[at:off] = 0
            view[off:off + arr.size] = arr.reshape(-1)
            at = off + arr.size
        view[at:] = 0
        return out


class DevicePrepBase:
    """A collated raw batch -> `dict(image, masked_image, mask, txt, ...)` on the device: one copy of the arena, one of the job table,
    one launch of `entry`.  The arena, table and output buffers are kept and grow only when a batch needs more, so a fixed-shape loop
    allocates nothing per step -- and the returned tensors are views of those buffers: the next call overwrites them.
    A subclass names the `entry` symbol, gives the scalars it takes between the table and the outputs (`dims`) and completes the
    returned dict (`finish`)."""
    entry = None

    def __init__(self, img_size, tiles, device):
        self.img_size, self.tiles, self.device = int(img_size), int(tiles), torch.device(device)
        self.arena = self.jobs = self.image = self.masked_image = self.mask = None

    def _grown(self, buf, n):
        return buf if buf is not None and buf.numel() >= n else torch.empty(n, dtype=torch.uint8, device=self.device)

    def allocate(self, N):
        S, T = self.img_size, self.tiles
        self.image = torch.empty(N, S, T * S, 3, device=self.device)
        self.masked_image = torch.empty(N, S, T * S, 3, device=self.device)
        self.mask = torch.empty(N, S, T * S, 1, device=self.device)

    def __call__(self, batch):
        assert (batch["img_size"], batch.get("tiles", self.tiles)) == (self.img_size, self.tiles), "the batch was planned for another canvas"
        N = batch["batch"] * (batch.get("views") or 1)      # canvases: the kernel's samples
        lib = _lib.load()
        n_bytes, n_table = batch["arena"].numel(), batch["jobs"].numel()
        self.arena, self.jobs = self._grown(self.arena, n_bytes), self._grown(self.jobs, n_table)
        if self.image is None or self.image.shape[0] < N:
            self.allocate(N)
        self.arena[:n_bytes].copy_(batch["arena"], non_blocking=True)
        self.jobs[:n_table].copy_(batch["jobs"], non_blocking=True)
        with torch.cuda.device(self.device):
            stream = torch.cuda.current_stream().cuda_stream
            _lib.check(getattr(lib, self.entry)(self.arena.data_ptr(), n_bytes, self.jobs.data_ptr(), batch["jobs"].data_ptr(), *self.dims(N),
                                                self.image.data_ptr(), self.masked_image.data_ptr(), self.mask.data_ptr(), stream),
                       self.entry[3:])
        return self.finish(batch, dict(image=self.image[:N], masked_image=self.masked_image[:N], mask=self.mask[:N], txt=batch["txt"]))


class DevicePrepLoader:
    """A re-iterable of device batches: every batch of `loader` (a raw-collating DataLoader) through `prep`."""

    def __init__(self, loader, prep):
        self.loader, self.prep = loader, prep

    def __len__(self):
        return len(self.loader)

    @property
    def sampler(self):
        return self.loader.sampler

    @property
    def dataset(self):
        return self.loader.dataset

    def __iter__(self):
        return (self.prep(batch) for batch in self.loader)


def loader(dataset, raw, device=None, **kw):
    """`DataLoader(dataset, **kw)`; with raw, the dataset's (plan, raw) items collated by its own `collate_raw` into page-locked memory
    and -- given a device -- finished there by its own `device_prep`."""
    from torch.utils.data import DataLoader
    if not raw:
        return DataLoader(dataset, **kw)
    inner = DataLoader(dataset, collate_fn=dataset.collate_raw, pin_memory=True, **kw)
    return inner if device is None else DevicePrepLoader(inner, dataset.device_prep(device))
