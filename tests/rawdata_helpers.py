"""Shared by the raw-route GPU tests (test_gpu_pairdata.py, test_gpu_nvsdata.py): a batch through a device prep, read back, and the
bit-for-bit comparison of its three planes.  No tests here."""
import numpy as np
import torch

KEYS = ("image", "masked_image", "mask")


def device_batch(collate, prep, items):
    """`prep(collate(items))`, synchronised, every tensor a host copy (the prep's own buffers are overwritten by its next call)."""
    out = prep(collate(items))
    torch.cuda.synchronize()
    return {k: (v.cpu().clone() if torch.is_tensor(v) else v) for k, v in out.items()}


def same_bits(got, want, what):
    for k in KEYS:
        g = got[k].numpy()
        assert g.dtype == np.float32 and g.shape == want[k].shape, (what, k, g.shape, want[k].shape)
        assert g.tobytes() == want[k].tobytes(), (what, k, int((g != want[k]).sum()), "values differ")
