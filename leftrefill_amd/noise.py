"""Seeded sampling noise, stated once on the host in numpy: what lr_seeded_normal (csrc/seeded_noise.hip) regenerates on the device.

A sample's key is (seed: uint64, sub: uint32) -- the user's seed and the number of the sample among those that share it.  A draw is
named by (stream: uint32, step: uint32): what it is for (the constants below) and the 0-based loop counter in execution order (not the
timestep).  Element i of a sample, g = i >> 2 (g < 2^32):

    w0..w3 = philox4x32_10(counter = (g, sub, step, stream), key = (seed & 0xffffffff, seed >> 32))
    u(w)   = ((w >> 9) + 0.5) * 2^-23          # in (0, 1); exact in fp32: 24 significant bits
    pair p in {0, 1}:  r = sqrt(-2 ln u(w[2p])),  z[4g + 2p] = r cos(2 pi u(w[2p+1])),  z[4g + 2p + 1] = r sin(2 pi u(w[2p+1]))

The value is a pure function of (seed, sub, stream, step, i): the same whatever the batch, the row's place in it, the rank or the
history of the process.  `normal_numpy` evaluates it in float64 and rounds once to fp32: the yardstick of the kernel tests and the
route of CPU tensors.  The device evaluates it in fp32 (logf, sqrtf, sincospif) and agrees to a few units of 2^-24 max(r, 1), not bit
for bit.  Nothing here touches torch's or numpy's global generators.
"""
import numpy as np

from .lora_dropout import philox4x32_10

# streams: what a draw is for
START = 0          # the start code x_T
STEP = 1           # the sampler's noise of one step
KNOWN = 2          # the q_sample noise of the known region in the masked loops
ENCODE = 3         # DDIMSampler.stochastic_encode
POSTERIOR = 4      # the sample of the VAE posterior
STREAMS = {"START": START, "STEP": STEP, "KNOWN": KNOWN, "ENCODE": ENCODE, "POSTERIOR": POSTERIOR}

_U64 = 2 ** 64 - 1


def _u32(v, what):
    v = int(v)
    if not 0 <= v < 2 ** 32:
        raise ValueError(f"{what} {v} is outside uint32")
    return v


def normal_parts(seed, sub, stream, step, n, first=0):
    """(z, r) in float64, each [n]: the statement above before its one rounding, and the radius sqrt(-2 ln u1) of every element.
    first: the index of the first element wanted (elements first .. first + n - 1 of the sample)."""
    n, first = int(n), int(first)
    if n < 1 or first < 0 or (first + n + 3) // 4 > 2 ** 32:
        raise ValueError(f"{n} elements per sample from {first}: need 1 <= n, 0 <= first and (first + n - 1) >> 2 < 2^32")
    seed = int(seed) & _U64
    g = np.arange(first // 4, (first + n + 3) // 4, dtype=np.uint64)
    w = philox4x32_10((g, _u32(sub, "sub"), _u32(step, "step"), _u32(stream, "stream")), (seed & 0xFFFFFFFF, seed >> 32))
    u = [((v >> np.uint32(9)).astype(np.float64) + 0.5) * 2.0 ** -23 for v in w]
    z, rr = np.empty((g.size, 4), dtype=np.float64), np.empty((g.size, 4), dtype=np.float64)
    for p in (0, 1):
        r = np.sqrt(-2.0 * np.log(u[2 * p]))
        a = 2.0 * np.pi * u[2 * p + 1]
        z[:, 2 * p], z[:, 2 * p + 1] = r * np.cos(a), r * np.sin(a)
        rr[:, 2 * p] = rr[:, 2 * p + 1] = r
    lo = first - 4 * (first // 4)
    return z.reshape(-1)[lo:lo + n], rr.reshape(-1)[lo:lo + n]


def normal_numpy(seed, sub, stream, step, n, first=0):
    """The n standard normals of draw (stream, step) of the sample with key (seed, sub): float64 arithmetic, rounded once -> fp32 [n].
    Element i depends on i alone, so a shorter n is a prefix of a longer one; first: start at element `first` instead of 0."""
    return normal_parts(seed, sub, stream, step, n, first)[0].astype(np.float32)


def _signed(v):      # uint64 bits -> the int64 that holds them
    v = int(v) & _U64
    return v - 2 ** 64 if v >= 2 ** 63 else v


class SeededNoise(object):
    """The keys of a batch of B samples and the draws made from them.

    seeds: B ints (any sign; their low 64 bits are the seed), an integer tensor [B], or a [B, 2] integer tensor of (seed, sub) rows;
    subs: B sub-sample numbers (uint32), default 0 -- not with a [B, 2] table.  The table lives on `device` as int64 [B, 2] holding the
    uint64 bits; a device tensor is used where it is (no read-back unless the host route needs the keys)."""

    def __init__(self, seeds, subs=None, device=None):
        import torch
        if torch.is_tensor(seeds):
            assert not seeds.is_floating_point() and seeds.dim() in (1, 2), "seeds: an integer tensor [B] or [B, 2]"
            keys = seeds.to(torch.int64)
            if keys.dim() == 2:
                assert keys.shape[1] == 2 and subs is None, "a [B, 2] table holds the sub-sample numbers itself"
            else:
                sub = torch.zeros_like(keys) if subs is None else torch.as_tensor(subs, dtype=torch.int64, device=keys.device)
                assert sub.shape == keys.shape, "subs: one per seed"
                keys = torch.stack([keys, sub], dim=1)
            self._host = None
        else:
            seeds = [int(s) for s in seeds]
            subs = [0] * len(seeds) if subs is None else [_u32(s, "sub") for s in subs]
            assert len(subs) == len(seeds), "subs: one per seed"
            self._host = [(s & _U64, u) for s, u in zip(seeds, subs)]
            keys = torch.tensor([[_signed(s), u] for s, u in self._host], dtype=torch.int64).reshape(-1, 2)
        self.keys = keys.to(device=device if device is not None else keys.device).contiguous()
        assert self.keys.shape[0] >= 1, "at least one sample"
        self._row0 = None

    def __len__(self):
        return self.keys.shape[0]

    @property
    def device(self):
        return self.keys.device

    def host_keys(self):
        """[(seed, sub)] as python ints (seed in uint64); read back once when the table came as a device tensor."""
        if self._host is None:
            self._host = [(int(s) & _U64, _u32(int(u) & 0xFFFFFFFF, "sub")) for s, u in self.keys.tolist()]
        return self._host

    def to(self, device):
        import torch
        if torch.device(device) == self.keys.device:
            return self
        out = SeededNoise(self.keys.to(device))
        out._host = self._host
        return out

    def shard(self, s, e):
        """The keys of rows s:e (a rank's slice of the batch)."""
        out = SeededNoise(self.keys[s:e])
        out._host = None if self._host is None else self._host[s:e]
        return out

    def row0(self):
        """Row 0's key for every row (`repeat_noise`)."""
        if self._row0 is None:
            self._row0 = SeededNoise(self.keys[:1].repeat(len(self), 1))
            self._row0._host = None if self._host is None else [self._host[0]] * len(self)
        return self._row0

    def normal(self, stream, step, per_sample_shape, out=None):
        """fp32 [B, *per_sample_shape]: row b is draw (stream, step) of key b.  On the device one lr_seeded_normal launch; for CPU
        tensors the numpy statement.  out: a contiguous fp32 tensor of that shape on the keys' device to fill instead."""
        import torch
        shape = (len(self),) + tuple(int(d) for d in per_sample_shape)
        if out is None:
            out = torch.empty(shape, dtype=torch.float32, device=self.keys.device)
        assert tuple(out.shape) == shape and out.dtype == torch.float32 and out.device == self.keys.device and out.is_contiguous()
        if out.is_cuda:
            from . import ops
            return ops.seeded_normal(self.keys, stream, step, out)
        n = out[0].numel()
        for b, (seed, sub) in enumerate(self.host_keys()):
            out[b].copy_(torch.from_numpy(normal_numpy(seed, sub, stream, step, n)).reshape(shape[1:]))
        return out


def as_seeded(seeds, batch, device):
    """The samplers' `seeds=` argument -> a SeededNoise of `batch` rows on `device`, or None for None."""
    if seeds is None:
        return None
    sn = seeds.to(device) if isinstance(seeds, SeededNoise) else SeededNoise(seeds, device=device)
    if len(sn) != int(batch):
        raise ValueError(f"seeds: {len(sn)} keys for a batch of {int(batch)}")
    return sn


def shard_seeds(seeds, s, e):
    """Rows s:e of a `seeds=` argument in any of its forms."""
    if seeds is None:
        return None
    return seeds.shard(s, e) if isinstance(seeds, SeededNoise) else seeds[s:e]
