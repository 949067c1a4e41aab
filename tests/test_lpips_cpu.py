"""The host side of device LPIPS (no GPU): the declaration / binding of lr_lpips_alex and lr_lpips_workspace_bytes under ABI 30, the
packed weight layout, the workspace formula, the honesty of the parity inputs, and `validation_result` with an ordinary callable.

This module also holds what tests/test_gpu_lpips.py shares with it: the seeded weights (nothing is committed: the `lpips` package and
its weights are absent, LPIPSAlex is parity-unpinned), the image families, the float64 yardstick and the fp16-storage emulation.

Yardstick: `evalglue.LPIPSAlex` with the seeded weights in float64 on the CPU, on the float64 composite / crop / area mean.
Floor: `emulate_fp16_storage` -- the shifted and scaled input, the conv weights and every post-ReLU activation rounded to fp16,
everything else fp32 -- against the yardstick.  The kernel gets 4 x the family's floor, capped at CAP = 5e-5 (half a unit of the four
decimals the harness prints).  Here the emulation itself must stay inside the cap on every family and every case shape small enough
for the CPU: the inputs were not chosen to flatter the kernel."""
import functools
import os

import pytest
import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CAP = 5e-5
FAMILIES = {"far": 0.5, "near": 0.05, "vnear": 0.005}      # sigma of pred - origin

# (id, n, h, w, x0, Wc, r, masked, pred dtype)
CASES = [
    ("min_31x35", 2, 31, 35, 0, 35, 1, False, torch.float32),
    ("odd_67x95", 3, 67, 95, 0, 95, 1, True, torch.float32),
    ("edges_131x257", 1, 131, 257, 0, 257, 1, False, torch.float16),
    ("right_64x128", 2, 64, 128, 64, 64, 1, True, torch.float16),
    ("r2_128x256_right", 2, 128, 256, 128, 128, 2, True, torch.bfloat16),
    ("harness_512x1024_right", 2, 512, 1024, 512, 512, 1, True, torch.float16),
]
CPU_CASES = [c for c in CASES if c[2] * c[3] <= 131 * 257]


def seeded_state_dict(seed=0):
    """Conv weights N(0, 2 / fan_in), bias 0.1 N(0, 1), lin U(0, 4 / C) (non-negative like the real ones), in the key spelling
    LPIPSAlex.load_weights reads."""
    from leftrefill_amd.evalglue import LPIPSAlex
    g = torch.Generator().manual_seed(seed)
    sd = {}
    for i, ((ci, co, k, _, _), fi) in enumerate(zip(LPIPSAlex.CONVS, LPIPSAlex.FEATURE_INDEX)):
        sd[f"features.{fi}.weight"] = torch.randn(co, ci, k, k, generator=g) * (2.0 / (ci * k * k)) ** 0.5
        sd[f"features.{fi}.bias"] = 0.1 * torch.randn(co, generator=g)
        sd[f"lin{i}.model.1.weight"] = torch.rand(1, co, 1, 1, generator=g) * (4.0 / co)
    return sd


@functools.lru_cache(maxsize=None)
def reference_module():
    """The yardstick: LPIPSAlex with the seeded weights, float64, CPU."""
    from leftrefill_amd.evalglue import LPIPSAlex
    return LPIPSAlex().load_weights(seeded_state_dict()).double()


def family(name, n, h, w, seed):
    """origin: 5 x 5-box-smoothed uniform noise, x 2, clamped; pred = origin + sigma N(0, 1), clamped.  fp32 [n,3,h,w] in [-1, 1]."""
    g = torch.Generator().manual_seed(seed)
    origin = (2 * F.avg_pool2d(torch.rand(n, 3, h, w, generator=g) * 2 - 1, 5, 1, 2)).clamp(-1, 1)
    pred = (origin + FAMILIES[name] * torch.randn(n, 3, h, w, generator=g)).clamp(-1, 1)
    return pred.contiguous(), origin.contiguous()


def block_mask(n, h, w, seed, cell=8):
    g = torch.Generator().manual_seed(1000 + seed)
    blocks = (torch.rand(n, 1, -(-h // cell), -(-w // cell), generator=g) < 0.5).float()
    return blocks.repeat_interleave(cell, 2).repeat_interleave(cell, 3)[:, :, :h, :w].contiguous()


def case_inputs(fam, case, seed):
    _, n, h, w, x0, Wc, r, masked, dtype = case
    pred, origin = family(fam, n, h, w, seed)
    return pred.to(dtype), origin, (block_mask(n, h, w, seed) if masked else None), x0, Wc, r      # the stored prediction is what both sides read


def scored_pair(pred, origin, mask, x0, Wc, r, dtype=torch.float64):
    """The image lr_lpips_alex scores, and its origin: composite, columns [x0, x0 + Wc), r x r area mean -- in `dtype` on the CPU."""
    p, o = pred.to(dtype), origin.to(dtype)
    if mask is not None:
        m = mask.to(dtype)
        p = p * m + o * (1 - m)
    p, o = p[:, :, :, x0:x0 + Wc], o[:, :, :, x0:x0 + Wc]
    if r > 1:
        N, C, H, W = p.shape
        p = p.reshape(N, C, H // r, r, W // r, r).mean((3, 5))
        o = o.reshape(N, C, H // r, r, W // r, r).mean((3, 5))
    return p, o


def yardstick(pred, origin, mask, x0, Wc, r):
    """[N] float64."""
    p, o = scored_pair(pred, origin, mask, x0, Wc, r)
    return _forward64(p, o)


def _forward64(p, o):
    m = reference_module()
    total = 0
    for fa, fb, lin in zip(m.features(p), m.features(o), m.lins):
        na = fa / (fa.pow(2).sum(1, keepdim=True).sqrt() + 1e-10)
        nb = fb / (fb.pow(2).sum(1, keepdim=True).sqrt() + 1e-10)
        total = total + ((na - nb) ** 2 * lin).sum(1, keepdim=True).mean((2, 3), keepdim=True)
    assert total.dtype == torch.float64      # LPIPSAlex.forward itself casts to fp32: this is its body on float64 tensors
    return total.flatten()


def emulate_fp16_storage(pred, origin, mask, x0, Wc, r):
    """What fp16 storage alone costs: (x - shift) / scale, the conv weights and every post-ReLU activation rounded to fp16, the rest
    (composite, area mean, accumulation, bias, head) in fp32 on the CPU.  [N] float64 of fp32 results."""
    m = reference_module()
    p, o = scored_pair(pred, origin, mask, x0, Wc, r, torch.float32)
    q = lambda t: t.half().float()

    def feats(x):
        outs, h = [], q((x - m.shift.float()) / m.scale.float())
        for conv, pool in zip(m.convs, m.POOL_BEFORE):
            if pool:
                h = F.max_pool2d(h, 3, 2)
            h = q(F.relu(F.conv2d(h, q(conv.weight.float()), conv.bias.float(), conv.stride, conv.padding)))
            outs.append(h)
        return outs

    total = 0
    for fa, fb, lin in zip(feats(p), feats(o), m.lins):
        na = fa / (fa.pow(2).sum(1, keepdim=True).sqrt() + 1e-10)
        nb = fb / (fb.pow(2).sum(1, keepdim=True).sqrt() + 1e-10)
        total = total + ((na - nb) ** 2 * lin.float()).sum(1, keepdim=True).mean((2, 3), keepdim=True)
    assert total.dtype == torch.float32
    return total.flatten().double()


@functools.lru_cache(maxsize=None)
def family_references(fam, cpu_only=False):
    """Per case of the family: (inputs, float64 yardstick, emulation), computed once and shared; and the family's floor."""
    rows = []
    for ci, case in enumerate(CPU_CASES if cpu_only else CASES):
        inputs = case_inputs(fam, case, seed=10 * ci + list(FAMILIES).index(fam))
        ref, emu = yardstick(*inputs), emulate_fp16_storage(*inputs)
        rows.append(dict(case=case, inputs=inputs, ref=ref, emu=emu, floor=float((emu - ref).abs().max())))
    return rows, max(r["floor"] for r in rows)


# ---- the tests ---------------------------------------------------------------------------------------------------------------------
def test_lpips_symbols_are_declared_bound_and_built_under_abi_30():
    import ctypes
    import abi_helpers as abi
    from leftrefill_amd import _lib, build, ops
    header = abi.header().text
    assert _lib.ABI_VERSION == 30
    assert abi.c_params("lr_lpips_alex") == ["const lr_lpips_args* args", "lr_stream_t s"]
    # 4 pointers-or-ints rows: the C layout on LP64 -- pred 8, kind 4 (+4), origin 8, mask 8, 6 x int32, 15 pointers, ws 8, bytes 8, out 8
    assert ctypes.sizeof(_lib.LpipsArgs) == 8 + 8 + 8 + 8 + 24 + 15 * 8 + 8 + 8 + 8
    comment = header[header.index("LPIPS(alex) of a decoded prediction"):header.index("typedef struct lr_lpips_args")]
    for needle in ("test_inpainting.py:159", "LR_E_ARG", "tap-major", "13 launches", "(Ho - 7) / 4 + 1", "363 -> 384"):
        assert needle in comment, needle
    assert f"#define LR_LPIPS_LAUNCHES {ops.LPIPS_LAUNCHES}" in header and f"#define LR_LPIPS_MIN_SIDE {ops.LPIPS_MIN_SIDE}" in header
    assert f"#define LR_LPIPS_HEAD_PIXELS {ops.LPIPS_HEAD_PIXELS}" in header
    assert "lpips.hip" in build.SOURCES
    lib = _lib.load()      # a stale library fails here on the missing symbols
    assert lib.lr_lpips_workspace_bytes.restype is ctypes.c_int64
    assert callable(ops.lpips_alex) and callable(ops.pack_lpips)


def test_pack_lpips_layout():
    from leftrefill_amd import ops
    from leftrefill_amd.evalglue import DeviceLPIPS, LPIPSAlex
    m = DeviceLPIPS().load_weights(seeded_state_dict())
    packed = ops.pack_lpips(m)
    kpads = (384, 1600, 1728, 3456, 2304)
    for k, (ci, co, ks, _, _) in enumerate(LPIPSAlex.CONVS):
        wt = packed["wt"][k]
        assert wt.dtype == torch.float16 and wt.shape == (co, kpads[k]) and wt.is_contiguous()
        K = ks * ks * ci
        back = wt[:, :K].reshape(co, ks, ks, ci).permute(0, 3, 1, 2)      # K index = (ky * ks + kx) * Cin + c
        assert torch.equal(back, m.convs[k].weight.half())
        assert not wt[:, K:].any()                                         # zero K padding
        assert packed["bias"][k].dtype == torch.float32 and torch.equal(packed["bias"][k], m.convs[k].bias)
        assert packed["lin"][k].dtype == torch.float32 and torch.equal(packed["lin"][k], m.lins[k].flatten())
        assert (packed["lin"][k] >= 0).all()
    # spot value: output channel 5, tap (ky 2, kx 7), input channel 1 of conv 1
    assert packed["wt"][0][5, (2 * 11 + 7) * 3 + 1] == m.convs[0].weight[5, 1, 2, 7].half()


def test_workspace_bytes_equals_the_stage_size_formula():
    from leftrefill_amd import _lib, ops
    lib = _lib.load()
    assert ops.lpips_stage_sizes(31, 35) == [(7, 8), (3, 3), (1, 1), (1, 1), (1, 1)]
    assert ops.lpips_stage_sizes(512, 512) == [(127, 127), (63, 63), (31, 31), (31, 31), (31, 31)]
    for _, n, h, _, _, Wc, r, _, _ in CASES + [("bench", 4, 512, 1024, 512, 512, 1, True, torch.float16)]:
        got = lib.lr_lpips_workspace_bytes(n, h, Wc, r)
        assert got == ops.lpips_workspace_bytes(n, h, Wc, r) > 0, (n, h, Wc, r, got)
    up = lambda v: (v + 255) // 256 * 256      # the formula once more, by hand, for the smallest case
    want = sum(up(4 * hw * c * 2) for hw, c in ((56, 64), (9, 192), (1, 384), (1, 256), (1, 256))) + up(4 * 9 * 64 * 2) + up(4 * 192 * 2) \
        + up(8 * 2 * 5)
    assert lib.lr_lpips_workspace_bytes(2, 31, 35, 1) == want
    for bad in ((2, 30, 64, 1), (2, 64, 30, 1), (2, 63, 64, 2), (2, 64, 63, 2), (2, 60, 60, 2), (0, 64, 64, 1), (2, 64, 64, 0)):
        assert lib.lr_lpips_workspace_bytes(*bad) == -1, bad      # LR_E_ARG


@pytest.mark.parametrize("fam", list(FAMILIES))
def test_emulation_stays_inside_the_cap(fam):
    """The check that the inputs were chosen honestly: fp16 storage alone stays far inside the cap, so 4 x floor is what binds."""
    rows, floor = family_references(fam, cpu_only=True)
    for r in rows:
        print(fam, r["case"][0], "lpips", float(r["ref"].mean()), "floor", r["floor"], "rel", float(((r["emu"] - r["ref"]) / r["ref"]).abs().max()))
        assert torch.isfinite(r["ref"]).all() and (r["ref"] > 0).all()
    assert 4 * floor < CAP, (fam, floor)
    lo, hi = {"far": (3e-3, 0.3), "near": (1e-4, 1e-2), "vnear": (1e-6, 1e-4)}[fam]      # the three families are three decades apart
    assert all(lo < float(r["ref"].mean()) < hi for r in rows), [float(r["ref"].mean()) for r in rows]


def test_yardstick_is_lpipsalex():
    """`_forward64` is LPIPSAlex.forward's body on float64 tensors: in fp32 the two agree to fp32 rounding."""
    pred, origin, mask, x0, Wc, r = case_inputs("far", CASES[1], seed=3)
    p, o = scored_pair(pred, origin, mask, x0, Wc, r)
    from leftrefill_amd.evalglue import LPIPSAlex
    m32 = LPIPSAlex().load_weights(seeded_state_dict())
    got = m32(p.float(), o.float()).flatten().double()
    want = _forward64(p, o)
    assert got.shape == want.shape == (3,) and ((got - want).abs() <= 1e-5 * want).all()


def _stub_lpips(a, b):
    return ((a.float() - b.float()) ** 2).mean().reshape(1, 1, 1, 1)


def test_validation_result_with_an_ordinary_callable_is_unchanged():
    """Any callable other than a DeviceLPIPS: per sample, through lpips_pair, whether or not the model offers the device hook."""
    import numpy as np
    from leftrefill_amd import evalglue
    g = torch.Generator().manual_seed(0)
    metrics = {"psnr": torch.rand(3, generator=g) * 30, "ssim": torch.rand(3, generator=g)}
    pred, origin = torch.rand(3, 3, 8, 8, generator=g), torch.rand(3, 3, 8, 8, generator=g)
    calls = []

    def pair():
        calls.append("pair")
        return pred, origin

    def device(fn):
        raise AssertionError("the device hook is for DeviceLPIPS only")

    class M:
        pass

    m = M()
    m.loss_fn_alex = None
    want = {"psnr": float(metrics["psnr"].double().mean()), "ssim": float(metrics["ssim"].double().mean())}
    assert evalglue.validation_result(m, metrics, pair) == want and evalglue.validation_result(m, metrics, pair, device) == want and not calls
    m.loss_fn_alex = _stub_lpips
    want["lpips"] = float(np.mean([float(_stub_lpips(pred[i:i + 1], origin[i:i + 1])) for i in range(3)]))
    logged = {}
    m.log = lambda k, v, sync_dist=False: logged.update({k: (v, sync_dist)})
    assert evalglue.validation_result(m, metrics, pair) == want
    assert evalglue.validation_result(m, metrics, pair, device) == want and calls == ["pair", "pair"]
    assert logged == {"val/" + k: (v, True) for k, v in want.items()}
    host = evalglue.LPIPSAlex().load_weights(seeded_state_dict())      # the eager module is an ordinary callable too
    big = torch.rand(2, 3, 40, 40, generator=g) * 2 - 1
    m.loss_fn_alex = host
    res = evalglue.validation_result(m, {k: v[:2] for k, v in metrics.items()}, lambda: (big, -big), device)
    assert res["lpips"] == float(np.mean([float(host(big[i:i + 1], -big[i:i + 1])) for i in range(2)]))


def test_validation_result_with_device_lpips_scores_the_batch_in_one_call():
    """The DeviceLPIPS branch without a GPU: the hook's [N] tensor is averaged and joins the one read-back; lpips_pair is not built."""
    from leftrefill_amd import evalglue
    metrics = {"psnr": torch.tensor([20.0, 30.0]), "ssim": torch.tensor([0.5, 0.7])}
    fn = evalglue.DeviceLPIPS()
    seen = []

    class M:
        loss_fn_alex = fn

    def device(f):
        seen.append(f)
        return torch.tensor([0.25, 0.75])

    res = evalglue.validation_result(M(), metrics, lambda: (_ for _ in ()).throw(AssertionError("host pair built")), device)
    assert res == {"psnr": 25.0, "ssim": float(torch.tensor([0.5, 0.7]).double().mean()), "lpips": 0.5} and seen == [fn]
    with pytest.raises(RuntimeError, match="no weights"):
        fn.packed()
