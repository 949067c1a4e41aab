"""tests/golden/seeded_noise.npz: a small pinned vector of the seeded-noise statement (leftrefill_amd/noise.py), for two keys.

    python -m tools.make_golden_seeded_noise

Written from the float64 statement (`normal_parts`): per key the first N values in float64, their one rounding to fp32 and the Philox
words of the first group.  tests/test_seeded_noise_cpu.py holds `normal_numpy` to it bit for bit, so a change of the counter layout, of
the uniform's bits or of the Box-Muller pairing cannot pass unnoticed.
"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from leftrefill_amd import noise as N  # noqa: E402
from leftrefill_amd.lora_dropout import philox4x32_10  # noqa: E402

OUT = os.path.join(ROOT, "tests", "golden", "seeded_noise.npz")
N_VALUES = 37      # nine groups and a tail of one
# (seed, sub, stream, step)
PINNED = [(0, 0, N.START, 0), (2 ** 40 + 7, 3, N.STEP, 49)]


def main():
    out = {"keys": np.array(PINNED, dtype=np.uint64), "n": np.array(N_VALUES)}
    for k, (seed, sub, stream, step) in enumerate(PINNED):
        z, r = N.normal_parts(seed, sub, stream, step, N_VALUES)
        out[f"key{k}.z64"], out[f"key{k}.r64"], out[f"key{k}.z32"] = z, r, z.astype(np.float32)
        out[f"key{k}.words0"] = np.array([int(w) for w in philox4x32_10((0, sub, step, stream), (seed & 0xFFFFFFFF, seed >> 32))],
                                         dtype=np.uint32)
    np.savez_compressed(OUT, **out)
    print(f"seeded noise golden: {len(PINNED)} keys x {N_VALUES} values, {os.path.getsize(OUT)} bytes; key0 z[:4] = {out['key0.z32'][:4]}")


if __name__ == "__main__":
    sys.exit(main())
