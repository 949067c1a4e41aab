"""CPU: leftrefill_amd/fid.py without a GPU -- the eager network's names and shapes, FID_PROGRAM (table, channel offsets, K layout, folded
BatchNorm) through a small float64 interpreter against `FIDInception` in float64, the Frechet distance, the statistics and the 8-bit /
bilinear input mapping.  `interpret`, `images` and `references` are shared with tests/test_gpu_fid.py."""
import functools
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from leftrefill_amd import fid

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def interpret(program, layout, wt, bias, x_nhwc, round16=False):
    """FID_PROGRAM in torch float64: x_nhwc [B, 299, 299, 4] -> [B, 2048].  Regions are [B, H, W, ld] at offset * B of one flat arena,
    as lr_fid_run lays them out.  round16: every stored activation is rounded to fp16 (the storage of the device route)."""
    B = x_nhwc.shape[0]
    q = (lambda t: t.half().double()) if round16 else (lambda t: t)
    arena = torch.zeros(B * layout["arena_halfs"], dtype=torch.float64)
    region = lambda off, h, w, ld: arena[int(off) * B:int(off) * B + B * int(h) * int(w) * int(ld)].view(B, int(h), int(w), int(ld))
    region(layout["input_off"], fid.SIZE, fid.SIZE, 4).copy_(q(x_nhwc.double()))
    for r in program.tolist():
        w = dict(zip(("op", "so", "sl", "sc", "do", "dl", "dc", "hi", "wi", "ci", "ho", "wo", "co", "kh", "kw", "st", "ph", "pw", "wo_", "bo", "kp"), r))
        x = region(w["so"], w["hi"], w["wi"], w["sl"])[..., w["sc"]:w["sc"] + w["ci"]].permute(0, 3, 1, 2)
        if w["op"] == fid.OP_CONV:
            k = wt[w["wo_"]:w["wo_"] + w["co"] * w["kp"]].double().view(w["co"], w["kp"])
            assert not k[:, w["kh"] * w["kw"] * w["ci"]:].any()
            k = k[:, :w["kh"] * w["kw"] * w["ci"]].view(w["co"], w["kh"], w["kw"], w["ci"]).permute(0, 3, 1, 2)
            y = F.relu(F.conv2d(x, k, bias[w["bo"]:w["bo"] + w["co"]].double(), w["st"], (w["ph"], w["pw"])))
        else:
            y = fid._pool_eager(w["op"], x)
        assert y.shape[2:] == (w["ho"], w["wo"])
        region(w["do"], w["ho"], w["wo"], w["dl"])[..., w["dc"]:w["dc"] + w["co"]] = q(y.permute(0, 2, 3, 1))
    return region(layout["output_off"], 1, layout["output_hw"], layout["output_c"]).view(B, layout["output_hw"], -1).mean(1)


def images(n, h, w, seed):
    """n distinct smooth seeded uint8 images [n, h, w, 3]: a few random low-frequency waves per channel."""
    g = torch.Generator().manual_seed(seed)
    yy, xx = torch.meshgrid(torch.linspace(0, 1, h), torch.linspace(0, 1, w), indexing="ij")
    out = torch.zeros(n, h, w, 3)
    for i in range(n):
        for c in range(3):
            for _ in range(4):
                fy, fx, ph, amp = (torch.rand(4, generator=g) * torch.tensor([6.0, 6.0, 6.28, 0.3])).tolist()
                out[i, :, :, c] += amp * torch.sin(6.28 * (fy * yy + fx * xx) + ph)
    return fid.to_uint8(out.clamp(-1, 1))


def nhwc4(x_nchw):
    return F.pad(x_nchw.permute(0, 2, 3, 1), (0, 1))


@functools.lru_cache(maxsize=None)
def module64(seed=0):
    return fid.FIDInception().load_weights(fid.seeded_state_dict(seed)).double()


@functools.lru_cache(maxsize=None)
def references(n, h, w, seed):
    """(u8 images, float64 yardstick features [n, 2048], fp16-storage emulation [n, 2048]): computed once, shared, never changed.
    The emulation is FID_PROGRAM in float64 with the packed fp16 weights and every stored activation rounded to fp16."""
    u8 = images(n, h, w, seed)
    x = fid.preprocess(u8, torch.float64)
    ref = module64()(x)
    packed = fid.pack_fid(fid.FIDInception().load_weights(fid.seeded_state_dict(0)))
    emu = interpret(fid.FID_PROGRAM, fid.FID_LAYOUT, packed["wt"], packed["bias"], nhwc4(x), round16=True)
    return u8, ref, emu


def rel_l2(a, b):
    return ((a.double() - b.double()).norm(dim=1) / b.double().norm(dim=1)).tolist()


# ---- the eager network -----------------------------------------------------------------------------------------------------------------
def test_state_dict_names_and_loading():
    net = fid.FIDInception()
    sd = net.state_dict()
    assert len(fid.CONVS) == 94 and len(sd) == 94 * 5
    leaves = ("conv.weight", "bn.weight", "bn.bias", "bn.running_mean", "bn.running_var")
    assert set(sd) == {f"{o['name']}.{leaf}" for o in fid.CONVS for leaf in leaves}
    for k in ("Conv2d_1a_3x3.conv.weight", "Conv2d_4a_3x3.bn.running_var", "Mixed_5b.branch1x1.bn.running_mean", "Mixed_6a.branch3x3dbl_3.conv.weight",
              "Mixed_6c.branch7x7dbl_5.bn.weight", "Mixed_7a.branch7x7x3_4.bn.bias", "Mixed_7c.branch3x3dbl_3b.conv.weight"):
        assert k in sd, k
    assert sd["Mixed_6b.branch7x7_2.conv.weight"].shape == (128, 128, 1, 7) and sd["Mixed_6b.branch7x7dbl_2.conv.weight"].shape == (128, 128, 7, 1)
    assert sd["Mixed_7b.branch3x3_2a.conv.weight"].shape == (384, 384, 1, 3) and sd["Mixed_7c.branch1x1.conv.weight"].shape == (320, 2048, 1, 1)
    seeded = fid.seeded_state_dict(0)
    with pytest.raises(RuntimeError):
        net(torch.zeros(1, 3, 299, 299))
    net.load_weights({**seeded, "fc.weight": torch.zeros(1000, 2048), "fc.bias": torch.zeros(1000), "AuxLogits.fc.bias": torch.zeros(1000),
                      "Conv2d_1a_3x3.bn.num_batches_tracked": torch.tensor(0)})
    assert torch.equal(net.state_dict()["Mixed_7c.branch_pool.bn.bias"], seeded["Mixed_7c.branch_pool.bn.bias"])
    short = dict(seeded)
    del short["Mixed_6d.branch7x7dbl_3.bn.running_var"]
    with pytest.raises(KeyError, match="Mixed_6d.branch7x7dbl_3.bn.running_var"):
        fid.FIDInception().load_weights(short)


def test_shape_trace():
    u8, _, _ = references(1, 64, 64, 3)
    t = module64().trace(fid.preprocess(u8, torch.float64))
    assert t["Mixed_5d"].shape == (1, 288, 35, 35) and t["Mixed_6e"].shape == (1, 768, 17, 17) and t["Mixed_7c"].shape == (1, 2048, 8, 8)
    sizes = [t[n].shape[2] for n in ("input", "s1", "s2", "s3", "s4", "s5", "s6", "s7", "Mixed_6a", "Mixed_7a")]
    assert sizes == [299, 149, 147, 147, 73, 73, 71, 35, 17, 8]


def test_program_equals_the_eager_network_in_float64():
    """The padded layout and the folded BatchNorm are exact in real arithmetic: float64 on both sides, 1e-10 relative."""
    u8, ref, _ = references(1, 64, 64, 3)
    exact = fid.pack_fid(module64(), exact=True)
    got = interpret(fid.FID_PROGRAM, fid.FID_LAYOUT, exact["wt"], exact["bias"], nhwc4(fid.preprocess(u8, torch.float64)))
    err = rel_l2(got, ref)[0]
    print("program vs eager, float64 rel-L2", err, "largest feature", float(ref.max()), "zero fraction", float((ref == 0).double().mean()))
    assert got.shape == (1, 2048) and float(ref.abs().max()) > 0.1
    assert float((got - ref).abs().max()) <= 1e-10 * float(ref.abs().max()) and err <= 1e-10


def test_program_table_rules():
    """What lr_fid_run checks, stated on the table: regions inside the arena, channel ranges inside their strides, weights and biases
    tiling their blobs without gaps, K padded to the next multiple of 64."""
    P, L = fid.FID_PROGRAM, fid.FID_LAYOUT
    assert P.dtype == np.int32 and P.shape == (len(fid.GRAPH.ops), fid.ROW_WORDS) and (P >= 0).all() and not P[:, 21:].any()
    assert (P[:, fid.W_SRC_OFF] % 8 == 0).all() and (P[:, fid.W_DST_OFF] % 8 == 0).all()
    assert (P[:, fid.W_SRC_OFF] + P[:, fid.W_HIN] * P[:, fid.W_WIN] * P[:, fid.W_SRC_LD] <= L["arena_halfs"]).all()
    assert (P[:, fid.W_DST_OFF] + P[:, fid.W_HOUT] * P[:, fid.W_WOUT] * P[:, fid.W_DST_LD] <= L["arena_halfs"]).all()
    assert (P[:, fid.W_DST_C0] + P[:, fid.W_COUT] <= P[:, fid.W_DST_LD]).all() and (P[:, fid.W_DST_C0] % 4 == 0).all()
    conv = P[P[:, fid.W_OP] == fid.OP_CONV]
    k = conv[:, fid.W_KH] * conv[:, fid.W_KW] * conv[:, fid.W_CIN]
    assert len(conv) == 94 and (conv[:, fid.W_KPAD] % 64 == 0).all() and (conv[:, fid.W_KPAD] >= k).all() and (conv[:, fid.W_KPAD] < k + 64).all()
    assert conv[0, fid.W_CIN] == 4 and (conv[1:, fid.W_CIN] % 8 == 0).all()
    w_end = conv[:, fid.W_W_OFF] + conv[:, fid.W_COUT] * conv[:, fid.W_KPAD]
    assert conv[0, fid.W_W_OFF] == 0 and (conv[1:, fid.W_W_OFF] == w_end[:-1]).all() and w_end[-1] == L["wt_halfs"]
    assert (np.cumsum(conv[:, fid.W_COUT]) == conv[:, fid.W_B_OFF] + conv[:, fid.W_COUT]).all() and L["bias_floats"] == conv[:, fid.W_COUT].sum()
    src, dst = P[:, fid.W_SRC_OFF], P[:, fid.W_DST_OFF]      # an op never reads the region it writes
    src_end, dst_end = src + P[:, fid.W_HIN] * P[:, fid.W_WIN] * P[:, fid.W_SRC_LD], dst + P[:, fid.W_HOUT] * P[:, fid.W_WOUT] * P[:, fid.W_DST_LD]
    assert ((src_end <= dst) | (dst_end <= src)).all()


# ---- statistics and distance ---------------------------------------------------------------------------------------------------------
def _random_stats(d, n, seed):
    x = np.random.default_rng(seed).standard_normal((n, d)) * np.linspace(0.5, 2.0, d) + np.linspace(-1, 1, d)
    return x, x.mean(0), np.cov(x, rowvar=False)


def test_frechet_distance_properties():
    _, mu, s = _random_stats(16, 200, 0)
    assert abs(fid.frechet_distance(mu, s, mu, s)) <= 1e-8 * np.trace(s)
    rng = np.random.default_rng(1)
    a, b, m1, m2 = rng.uniform(0.5, 3, 16), rng.uniform(0.5, 3, 16), rng.standard_normal(16), rng.standard_normal(16)
    closed = float(((np.sqrt(a) - np.sqrt(b)) ** 2).sum() + ((m1 - m2) ** 2).sum())
    assert abs(fid.frechet_distance(m1, np.diag(a), m2, np.diag(b)) - closed) <= 1e-9 * closed
    _, mu2, s2 = _random_stats(16, 150, 2)
    d12, d21 = fid.frechet_distance(mu, s, mu2, s2), fid.frechet_distance(mu2, s2, mu, s)
    assert d12 > 0 and abs(d12 - d21) <= 1e-9 * d12


def test_frechet_distance_rank_deficient_pair_is_finite():
    """n = 8 samples of 2048 features: both covariances have rank 7."""
    rng = np.random.default_rng(3)
    xa, xb = rng.standard_normal((8, 2048)), rng.standard_normal((8, 2048)) + 0.1
    d = fid.frechet_distance(xa.mean(0), np.cov(xa, rowvar=False), xb.mean(0), np.cov(xb, rowvar=False))
    assert np.isfinite(d) and d > 0


def test_stats_from_sums_and_fidstats_host():
    x, mu, s = _random_stats(64, 13, 4)
    st = fid.FIDStats(64)
    st.update_host(x[:5].astype(np.float32))
    st.update_host(torch.from_numpy(x[5:].astype(np.float32)))
    x32 = x.astype(np.float32).astype(np.float64)
    total, gram, n = st.sums()
    assert n == 13 and np.allclose(total, x32.sum(0), rtol=1e-13, atol=1e-13) and np.allclose(gram, x32.T @ x32, rtol=1e-13, atol=1e-12)
    mu_, s_ = fid.stats_from_sums(total, gram, n)
    assert np.allclose(mu_, x32.mean(0), rtol=1e-12, atol=1e-13) and np.allclose(s_, np.cov(x32, rowvar=False), rtol=1e-10, atol=1e-12)
    with pytest.raises(ValueError):
        fid.stats_from_sums(total, gram, 1)


# ---- the input mapping ------------------------------------------------------------------------------------------------------------------
def test_eight_bit_mapping():
    x = torch.tensor([-3.0, -1.0, -0.999, -0.5, 0.0, 0.5, 0.999, 1.0, 7.0, 2 / 255 * 100 - 1])
    want = np.trunc((np.clip(x.numpy(), -1, 1).astype(np.float32) + np.float32(1)) / np.float32(2) * np.float32(255)).astype(np.uint8)
    assert fid.to_uint8(x).tolist() == want.tolist() and fid.to_uint8(x)[:5].tolist() == [0, 0, 0, 63, 127] and fid.to_uint8(x)[7:9].tolist() == [255, 255]
    assert fid.to_uint8(x.half()).dtype == torch.uint8


@pytest.mark.parametrize("side", [256, 512])
def test_bilinear_coordinates_against_interpolate(side):
    """The kernel's taps against F.interpolate in float64, enlarging (256 -> 299) and shrinking (512 -> 299, no antialiasing).  Both
    sides are float64: a coordinate is a few roundings of a number below `side`, |df| <= 4 * 2^-53 * side per axis, the image 2 p - 1
    changes by at most 2 per unit of either coordinate, and the blend itself adds a few roundings of numbers below 1."""
    u8 = images(1, side, side - 32, side)
    want = fid.preprocess(u8, torch.float64).permute(0, 2, 3, 1).numpy()
    got = fid.resize_numpy(u8.numpy())
    tol = 2 * 2 * 4 * 2.0 ** -53 * side + 16 * 2.0 ** -53
    err = float(np.abs(got - want).max())
    print(side, "-> 299: max |taps - F.interpolate|", err, "tolerance", tol)
    assert got.shape == (1, 299, 299, 3) and err <= tol
    i0, i1, l = fid.bilinear_taps(side, 299)
    assert i0[0] == 0 and i1[-1] == side - 1 and (i1 - i0 <= 1).all() and (l >= 0).all() and (l < 1).all()
