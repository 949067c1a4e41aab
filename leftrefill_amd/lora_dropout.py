"""The LoRA dropout mask, stated once on the host in numpy: what the `lr_lora_*_drop` kernels (csrc/lora.hip) regenerate on the device.

    keep(seed, stream, draw, row, col) = philox4x32_10((row, col >> 2, stream, draw), (seed & 0xffffffff, seed >> 32))[col & 3] >= thr

  row     row of the layer's own [M, K] input (b * L + l in the reference's `b (h w) c` order; b * 77 + j for the context projections)
  col     the layer's output feature as the reference numbers it -- not its place in a fused [q | k | v] buffer, not the packed GEGLU order
  stream  the layer's index in injection order (`inject_trainable_lora`)
  draw    32-bit counter of training forwards (wraps)
  thr     min(2^32 - 1, floor(p 2^32)) in float64;  inv_keep = fp32(1 / (1 - p))

One Philox call gives the mask of four consecutive columns of one row.  A mask only zeroes; 1 / (1 - p) is an fp32 scalar.  Every kernel
test compares against this module; nothing here touches the device.
"""
import numpy as np

PHILOX_M0, PHILOX_M1 = 0xD2511F53, 0xCD9E8D57
PHILOX_W0, PHILOX_W1 = 0x9E3779B9, 0xBB67AE85
_U32 = np.uint64(0xFFFFFFFF)


def philox4x32_10(counter, key):
    """Philox-4x32 with 10 rounds.  counter: 4 and key: 2 arrays (or ints) of 32-bit words, broadcast against each other -> a tuple of 4
    uint32 arrays."""
    c = [np.asarray(v, dtype=np.uint64) & _U32 for v in counter]
    k = [np.asarray(v, dtype=np.uint64) & _U32 for v in key]
    assert len(c) == 4 and len(k) == 2
    m0, m1 = np.uint64(PHILOX_M0), np.uint64(PHILOX_M1)
    for r in range(10):
        p0, p1 = m0 * c[0], m1 * c[2]                      # 32 x 32 -> 64 bits: exact in uint64
        c = [(p1 >> np.uint64(32)) ^ c[1] ^ k[0], p1 & _U32, (p0 >> np.uint64(32)) ^ c[3] ^ k[1], p0 & _U32]
        k = [(k[0] + np.uint64(PHILOX_W0)) & _U32, (k[1] + np.uint64(PHILOX_W1)) & _U32]
    return tuple(v.astype(np.uint32) for v in c)


def threshold(p):
    """uint32 threshold of drop probability p: an element is kept when its Philox word is >= it."""
    if not 0.0 <= p < 1.0:
        raise ValueError(f"LoRA dropout probability {p} is outside [0, 1)")
    return int(min(2 ** 32 - 1, np.floor(np.float64(p) * np.float64(2 ** 32))))


def inv_keep(p):
    """1 / (1 - p), formed in float64 and rounded to fp32 once."""
    return float(np.float32(1.0 / (1.0 - np.float64(p))))


def keep(seed, stream, draw, row, col, p):
    """Boolean keep mask at (row, col), broadcast; col is the logical output feature."""
    seed = int(seed) & (2 ** 64 - 1)
    row, col = np.asarray(row, dtype=np.int64), np.asarray(col, dtype=np.int64)
    words = philox4x32_10((row, col >> 2, int(stream) & 0xFFFFFFFF, int(draw) & 0xFFFFFFFF), (seed & 0xFFFFFFFF, seed >> 32))
    lane = np.broadcast_to(col & 3, words[0].shape)
    w = np.choose(lane, [np.broadcast_to(v, lane.shape) for v in words])
    return w >= np.uint32(threshold(p))


def keep_mask(seed, stream, draw, M, N, p, row0=0):
    """The [M, N] keep mask of one layer at one draw (rows row0 .. row0 + M - 1, logical columns 0 .. N - 1)."""
    return keep(seed, stream, draw, np.arange(row0, row0 + M)[:, None], np.arange(N)[None, :], p)


def colgrp_of(perm):
    """Logical group of four columns behind each packed group of four, for a packed-row permutation (packed row j = logical row perm[j],
    e.g. packing.geglu_perm): int32 [N / 4].  ValueError unless every packed group is an aligned logical group."""
    perm = np.asarray(perm, dtype=np.int64).reshape(-1, 4)
    if perm.size == 0 or (perm[:, 0] % 4).any() or (perm != perm[:, :1] + np.arange(4)).any():
        raise ValueError("the permutation does not keep aligned groups of four columns together")
    return (perm[:, 0] // 4).astype(np.int32)
