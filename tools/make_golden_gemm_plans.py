"""Record what the five host-side plan queries of lr_gemm_conv_f16 answer -> tests/golden/gemm_plans.npz.

    python tools/make_golden_gemm_plans.py            # with the library of the commit whose answers are to be pinned

The queries (lr_gemm_plan, lr_gemm_gn_rows, lr_gemm_gn_group_chunks, lr_gemm_stats_parts, lr_gemm_workspace_bytes) are pure host
code: hipcc cross-compiles the library without a GPU and they run there.  tests/test_gemm_plan_cpu.py regenerates the same cases
(`cases()`, shared) and asserts the recorded numbers one for one, so a change of the host code that moves any of them -- and with it
the size of a statistics buffer the front end allocates -- fails on the CPU.
"""
import itertools
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)
OUT = os.path.join(ROOT, "tests", "golden", "gemm_plans.npz")

# one case = these lr_gemm_args fields (the rest zero); p2 / skip1 are presence flags (the queries only test them for null)
FIELDS = ("B", "H", "W", "Hs", "Ws", "N", "taps", "up", "C1", "geglu", "splits", "gn_hw", "skip1", "Cs1", "tile_m", "tile_n", "pipe")
# the seven pinned numbers; the 64-bit byte count is stored as two non-negative int32 (bytes >> 31, bytes & (2^31 - 1))
ANSWERS = ("tile_m", "tile_n", "splits", "stages", "gn_rows", "gn_group_chunks", "stats_parts", "workspace_hi", "workspace_lo")

GRID_M = (64, 128, 256, 512, 777, 1024, 2048, 4096, 8192, 16384, 32768, 65536)      # 777: no tile divides it
GRID_N = (64, 128, 160, 192, 320, 640, 1280, 2560)
GRID_C = (16, 64, 320, 640, 1280, 2560)                                            # 16: the 16-channel 3x3 source (taps 9 only)
GRID_TAPS = ((1, 0), (9, 0), (4, 3))                                               # (taps, up); up = 3: the phase form
GRID_STRIDE = 23                                                                   # every 23rd case of the product: ~20 000


def dispatch_accepts(tm, tn, pipe, mode, phase, taps):
    """Whether the dispatch at the end of lr_gemm_conv_f16 has an instance for a TILE_CANDIDATES entry; mode 0 plain, 1 GEGLU, 2 erf-GELU.
    Read off the if / else-if chain of the recorded commit (c630dfd)."""
    if pipe == 8:                                   # halo-tile conv: plain 3x3 only
        return mode == 0 and not phase and taps == 9
    if phase:                                       # pipelined instances only; the 128-row tiles always run on the 4-stage ring
        return mode == 0 and (tm, tn) in ((128, 128), (128, 160), (256, 128), (256, 160), (256, 320))
    if mode == 0:
        return True
    if mode == 1:
        return (tm, tn, pipe) in ((128, 64, 0), (128, 128, 0), (128, 128, 4), (256, 128, 0), (256, 256, 0), (256, 320, 0))
    return (tm, tn, pipe) in ((128, 64, 0), (128, 128, 0), (256, 128, 0))


def tile_requests(mode, phase, taps):
    from leftrefill_amd import ops
    return [(0, 0, 0), (128, 0, 0), (256, 0, 0)] + [c for c in ops.TILE_CANDIDATES if dispatch_accepts(*c, mode, phase, taps)]


def cases():
    """Every case as a tuple in FIELDS order: (a) the keys of tile_table.json, args as ops.gemm_plan builds them, with zeros and with the
    table's plan as the request; (b) every GRID_STRIDE-th point of the grid."""
    from leftrefill_amd import ops
    out = []
    for key, plan in sorted(json.load(open(ops.TILE_TABLE_PATH)).items()):
        M, N, K, taps, _stride, _up, geglu, _cat, _asym, _gelu, ln, stats = map(int, key.split(","))
        base = dict(B=1, H=1, W=M, N=N, taps=taps, C1=K // taps, geglu=geglu, splits=1 if ln or stats else 0)
        out.append(base)
        out.append(dict(base, tile_m=plan[0], tile_n=plan[1], splits=plan[2], pipe=plan[3] if len(plan) > 3 else 0))
    grid = []
    for M, N, C, (taps, up), geglu, splits, gn, Cs1 in itertools.product(GRID_M, GRID_N, GRID_C, GRID_TAPS, (0, 1, 2), (0, 1, 4), (0, 1), (0, 320)):
        if (C == 16 and taps != 9) or (up == 3 and M % 8):
            continue
        B = 2 if M % 2 == 0 else 1
        H = 2 if up == 3 else 1
        W = M // (B * H)
        for tm, tn, pipe in tile_requests(geglu, up == 3, taps):
            grid.append(dict(B=B, H=H, W=W, Hs=H // 2 if up == 3 else H, Ws=W // 2 if up == 3 else W, N=N, taps=taps, up=up, C1=C, geglu=geglu,
                             splits=splits, gn_hw=(M // 2) * gn, skip1=int(Cs1 > 0), Cs1=Cs1, tile_m=tm, tile_n=tn, pipe=pipe))
    out += grid[::GRID_STRIDE]
    return [tuple(c.get(f, 0) for f in FIELDS) for c in out]


def answers(lib, case):
    """The seven numbers of one case, in ANSWERS order."""
    import ctypes
    from leftrefill_amd import _lib
    a = _lib.GemmArgs()
    for f, v in zip(FIELDS, case):
        setattr(a, f, v)
    a.Hs, a.Ws = a.Hs or a.H, a.Ws or a.W
    plan = (ctypes.c_int32 * 4)()
    assert lib.lr_gemm_plan(a, plan) == 0
    ws = lib.lr_gemm_workspace_bytes(a)
    return tuple(plan) + (lib.lr_gemm_gn_rows(a), lib.lr_gemm_gn_group_chunks(a), lib.lr_gemm_stats_parts(a), ws >> 31, ws & 0x7FFFFFFF)


def check_coverage(cs, ans):
    """The fixture must see every branch of the plan: widen the grid if one of these fails, not the assertion."""
    from leftrefill_amd import ops
    f, g = {n: i for i, n in enumerate(FIELDS)}, {n: i for i, n in enumerate(ANSWERS)}
    c, r = np.asarray(cs), np.asarray(ans)
    resolved = set(zip(r[:, g["tile_m"]], r[:, g["tile_n"]], np.where(np.isin(r[:, g["stages"]], (4, 8)), r[:, g["stages"]], 0)))
    assert set(ops.TILE_CANDIDATES) <= resolved, set(ops.TILE_CANDIDATES) - resolved
    split, phase = r[:, g["splits"]] > 1, c[:, f["up"]] == 3
    for name, sel in (("standard", ~np.isin(r[:, g["stages"]], (4, 8)) & ~phase), ("deep", (r[:, g["stages"]] == 4) & ~phase),
                      ("halo", r[:, g["stages"]] == 8), ("phase", phase)):
        assert (split & sel).any(), f"no split-K case on a {name} instance"
    auto = c[:, f["splits"]] == 0
    for name, sel in (("deep", r[:, g["stages"]] == 4), ("halo", r[:, g["stages"]] == 8), ("phase", phase)):
        assert (split & sel & auto).any(), f"no automatic split-K case on a {name} instance"
    assert (r[:, g["gn_group_chunks"]] == 0).any() and (r[:, g["gn_group_chunks"]] > 0).any()
    assert ((c[:, f["C1"]] == 16) & (c[:, f["taps"]] == 9)).any(), "no 16-channel source"


def main():
    from leftrefill_amd import _lib
    lib = _lib.load()
    cs = cases()
    ans = [answers(lib, c) for c in cs]
    check_coverage(cs, ans)
    np.savez_compressed(OUT, cases=np.asarray(cs, dtype=np.int32), answers=np.asarray(ans, dtype=np.int32))
    print(f"{OUT}: {len(cs)} cases, {os.path.getsize(OUT)} bytes")


if __name__ == "__main__":
    main()
