"""The lr_fid_* kernels (csrc/inception.hip) on the MI355X: the convolution and the pools through single-row programs against torch in
float64 on the fp16-rounded operands, the input kernel against lr_eval_metrics' bytes and F.interpolate in float64, the whole network
against `FIDInception` in float64 on the CPU (yardstick, noise floor and images: tests/test_fid_cpu.py), the float64 statistics against
numpy, `DeviceFID` against `HostFID`, and the refusal of an invalid program row.

Bounds.  Convolution: |err| <= 2^-10 |y| + 2^-22 sum|w x| elementwise -- one fp16 rounding of the output (2^-11 |y|, doubled) plus the
fp32 accumulation of K products, whose rounding errors are each below 2^-24 of the running sum <= sum|w x| (K of them, adding like a
random walk: sqrt(2048) 2^-24 < 2^-18 of the SIGNED sum; 2^-22 of sum|w x|, which is ~sqrt(K) larger, is the same statement).  Whole
network: the floor e is the rel-L2 distance per image between the float64 yardstick and the same network with the packed fp16 weights
and every stored activation rounded to fp16, measured on the CPU by tests/test_fid_cpu.py `references`; the kernels get 2 e.
A run with LEFTREFILL_WRITE_PROFILES set writes e, the kernel's errors and the two FIDs to profiles/fid_parity.json."""
import json
import os
import sys

import numpy as np
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import test_fid_cpu as C  # noqa: E402
from leftrefill_amd import fid  # noqa: E402

DEV = "cuda"


def _profile(key, value):
    if os.environ.get("LEFTREFILL_WRITE_PROFILES"):
        path = os.path.join(os.environ["LEFTREFILL_WRITE_PROFILES"], "fid_parity.json")
        doc = json.load(open(path)) if os.path.exists(path) else {}
        doc[key] = value
        with open(path, "w") as f:
            json.dump(doc, f, indent=1)


def _up8(v):
    return -(-v // 8) * 8


def _row(op, B, hi, wi, cs, src_ld, ho, wo, cout, dst_ld, c0, k=(3, 3), stride=1, pad=(1, 1), w_off=0, b_off=0, src_c0=0):
    """One program row on an arena of two regions: the source at offset 0, the destination behind it."""
    r = np.zeros((1, fid.ROW_WORDS), dtype=np.int32)
    v = r[0]
    v[fid.W_OP], v[fid.W_SRC_OFF], v[fid.W_SRC_LD], v[fid.W_SRC_C0] = op, 0, src_ld, src_c0
    v[fid.W_DST_OFF], v[fid.W_DST_LD], v[fid.W_DST_C0] = _up8(hi * wi * src_ld), dst_ld, c0
    v[fid.W_HIN], v[fid.W_WIN], v[fid.W_CIN], v[fid.W_HOUT], v[fid.W_WOUT], v[fid.W_COUT] = hi, wi, cs, ho, wo, cout
    if op == fid.OP_CONV:
        v[fid.W_KH], v[fid.W_KW], v[fid.W_STRIDE], v[fid.W_PH], v[fid.W_PW] = k[0], k[1], stride, pad[0], pad[1]
        v[fid.W_W_OFF], v[fid.W_B_OFF], v[fid.W_KPAD] = w_off, b_off, -(-k[0] * k[1] * cs // 64) * 64
    return r


def _run_row(row, B, x_nhwc, dst_nhwc, wt=None, bias=None):
    """x_nhwc fp16 [B, H, W, src_ld], dst_nhwc fp16 [B, Ho, Wo, dst_ld] (its contents are what the row finds there) -> the destination."""
    from leftrefill_amd import ops
    v = row[0]
    arena = torch.zeros(B * (int(v[fid.W_DST_OFF]) + dst_nhwc[0].numel()), dtype=torch.float16, device=DEV)
    arena[:x_nhwc.numel()] = x_nhwc.flatten().to(DEV)
    d0 = int(v[fid.W_DST_OFF]) * B
    arena[d0:d0 + dst_nhwc.numel()] = dst_nhwc.flatten().to(DEV)
    ops.fid_run(row, B, arena, wt, bias)
    return arena[d0:d0 + dst_nhwc.numel()].view(dst_nhwc.shape).cpu()


def _pack_single(w16, cs):
    """fp16 [Cout, Cin, kh, kw] -> [Cout, Kpad], K index (ky kw + kx) cs + c, zeros in the padded channels and behind the last tap."""
    co, ci, kh, kw = w16.shape
    blk = torch.zeros(co, kh * kw, cs, dtype=torch.float16)
    blk[:, :, :ci] = w16.permute(0, 2, 3, 1).reshape(co, kh * kw, ci)
    out = torch.zeros(co, -(-kh * kw * cs // 64) * 64, dtype=torch.float16)
    out[:, :kh * kw * cs] = blk.reshape(co, -1)
    return out.flatten()


# name, B, H, W, Cin, Cout, (kh, kw), stride, (ph, pw), dst_ld, c0
CONV_CASES = [
    ("1x7_pad03_M90_into_768", 2, 5, 9, 160, 192, (1, 7), 1, (0, 3), 768, 192),
    ("7x1_pad30_M90_into_768", 2, 5, 9, 160, 192, (7, 1), 1, (3, 0), 768, 192),
    ("3x3_s2_9x9_to_4x4_M32", 2, 9, 9, 96, 96, (3, 3), 2, (0, 0), 96, 0),
    ("5x5_p2_cin48", 1, 7, 6, 48, 64, (5, 5), 1, (2, 2), 64, 0),
    ("stem_cin3_s2_15x15_to_7x7", 2, 15, 15, 3, 32, (3, 3), 2, (0, 0), 32, 0),
    ("1x1_cout80", 1, 6, 7, 64, 80, (1, 1), 1, (0, 0), 80, 0),
    ("1x1_cout48_into_96", 1, 6, 7, 192, 48, (1, 1), 1, (0, 0), 96, 48),
    ("1x1_cin2048_cout320_M128", 2, 8, 8, 2048, 320, (1, 1), 1, (0, 0), 320, 0),
    ("3x3_p1_M18_underfull", 2, 3, 3, 64, 96, (3, 3), 1, (1, 1), 96, 0),
    ("3x3_p1_cout448", 1, 5, 5, 64, 448, (3, 3), 1, (1, 1), 448, 0),
]


def _conv_case(B, H, W, ci, co, k, stride, pad, seed):
    g = torch.Generator().manual_seed(seed)
    cs = fid.stored_channels(ci)
    x = torch.zeros(B, H, W, cs)
    x[..., :ci] = torch.randn(B, H, W, ci, generator=g)
    if cs != ci:
        x[..., ci:] = 1.0      # a stored padding channel meets zero weights
    w = (torch.randn(co, ci, k[0], k[1], generator=g) * (2.0 / (ci * k[0] * k[1])) ** 0.5).half()
    b = 0.05 * torch.randn(co, generator=g)
    x16 = x.half()
    xd, wd = x16[..., :ci].permute(0, 3, 1, 2).double(), w.double()
    y = F.relu(F.conv2d(xd, wd, b.double(), stride, pad)).permute(0, 2, 3, 1)
    mag = (F.conv2d(xd.abs(), wd.abs(), b.double().abs(), stride, pad)).permute(0, 2, 3, 1)
    return cs, x16, w, b, y, mag


@pytest.mark.parametrize("case", CONV_CASES, ids=[c[0] for c in CONV_CASES])
def test_conv_single_row(case):
    name, B, H, W, ci, co, k, stride, pad, dst_ld, c0 = case
    cs, x16, w, b, y, mag = _conv_case(B, H, W, ci, co, k, stride, pad, seed=len(name))
    ho, wo = y.shape[1], y.shape[2]
    pattern = ((torch.arange(B * ho * wo * dst_ld) % 251).float() / 16 - 7).half().view(B, ho, wo, dst_ld)
    row = _row(fid.OP_CONV, B, H, W, cs, cs, ho, wo, co, dst_ld, c0, k, stride, pad)
    got = _run_row(row, B, x16, pattern, _pack_single(w, cs).to(DEV), b.to(DEV))
    err = (got[..., c0:c0 + co].double() - y).abs()
    bound = 2.0 ** -10 * y.abs() + 2.0 ** -22 * mag
    print(name, "M", B * ho * wo, "K", k[0] * k[1] * cs, "max err", float(err.max()), "max err / bound", float((err / bound).max()))
    assert torch.isfinite(got).all() and float(y.max()) > 0.1
    assert (err <= bound).all()
    keep = torch.ones(dst_ld, dtype=torch.bool)
    keep[c0:c0 + co] = False
    assert torch.equal(got[..., keep].view(torch.int16), pattern[..., keep].view(torch.int16))


def test_conv_1x3_and_3x1_fill_the_two_halves_of_one_range():
    """Mixed_7b's branch3x3_2a || _2b: two rows of ONE program write channels [0, 384) and [384, 768) of one 768-wide destination."""
    from leftrefill_amd import ops
    B, H, W, ci, co = 1, 4, 5, 384, 384
    cs, x16, wa, ba, ya, ma = _conv_case(B, H, W, ci, co, (1, 3), 1, (0, 1), seed=21)
    _, _, wb, bb, _, _ = _conv_case(B, H, W, ci, co, (3, 1), 1, (1, 0), seed=22)
    xd = x16.permute(0, 3, 1, 2).double()
    yb = F.relu(F.conv2d(xd, wb.double(), bb.double(), 1, (1, 0))).permute(0, 2, 3, 1)
    mb = F.conv2d(xd.abs(), wb.double().abs(), bb.double().abs(), 1, (1, 0)).permute(0, 2, 3, 1)
    pa, pb = _pack_single(wa, cs), _pack_single(wb, cs)
    prog = np.concatenate([_row(fid.OP_CONV, B, H, W, cs, cs, H, W, co, 768, 0, (1, 3), 1, (0, 1)),
                           _row(fid.OP_CONV, B, H, W, cs, cs, H, W, co, 768, 384, (3, 1), 1, (1, 0), w_off=pa.numel(), b_off=co)])
    before = ops.FID_LAUNCHES.value
    got = _run_row(prog, B, x16, torch.full((B, H, W, 768), float("nan")).half(), torch.cat([pa, pb]).to(DEV), torch.cat([ba, bb]).to(DEV))
    assert ops.FID_LAUNCHES.value - before == 2
    for lo, y, m in ((0, ya, ma), (384, yb, mb)):
        err = (got[..., lo:lo + co].double() - y).abs()
        assert (err <= 2.0 ** -10 * y.abs() + 2.0 ** -22 * m).all(), lo


@pytest.mark.parametrize("side", [7, 8])
def test_pools(side):
    g = torch.Generator().manual_seed(side)
    B, C = 2, 64
    x16 = torch.randn(B, side, side, C, generator=g).half()
    neg = (-x16.float().abs() - 0.5).half()
    ones = torch.ones(B, side, side, C).half()
    nchw = lambda t: t.permute(0, 3, 1, 2).double()
    small = (side - 3) // 2 + 1
    # average pool: the divisor is the number of taps inside the image -- a map of ones stays ones (4 / 6 / 9 at corner / edge / interior)
    row = _row(fid.OP_AVGPOOL_S1, B, side, side, C, C, side, side, C, C, 0)
    assert torch.equal(_run_row(row, B, ones, torch.zeros_like(ones)), ones)
    got, want = _run_row(row, B, x16, torch.zeros_like(x16)), fid._pool_eager(fid.OP_AVGPOOL_S1, nchw(x16)).permute(0, 2, 3, 1)
    cnt = fid._pool_eager(fid.OP_AVGPOOL_S1, torch.ones(1, 1, side, side).double())      # all ones: F.avg_pool2d divides by the same count
    assert torch.equal(cnt, torch.ones_like(cnt))
    # one fp16 rounding of the result + an fp32 sum of cnt <= 9 terms: <= 8 roundings of 2^-24 sum|x| each, divided by cnt = 2^-21 mean|x|
    mag = fid._pool_eager(fid.OP_AVGPOOL_S1, nchw(x16).abs()).permute(0, 2, 3, 1)
    assert ((got.double() - want).abs() <= 2.0 ** -10 * want.abs() + 2.0 ** -21 * mag).all()
    # max pool, stride 1, pad 1, on an all-negative map: a padding of 0 would win everywhere along the border
    row = _row(fid.OP_MAXPOOL_S1, B, side, side, C, C, side, side, C, C, 0)
    got = _run_row(row, B, neg, torch.zeros_like(neg))
    assert torch.equal(got.double(), fid._pool_eager(fid.OP_MAXPOOL_S1, nchw(neg)).permute(0, 2, 3, 1)) and (got < 0).all()
    # max pool, stride 2, floor: 7 -> 3 and 8 -> 3, written into channels [64, 128) of a 192-wide destination that keeps its other bits
    row = _row(fid.OP_MAXPOOL_S2, B, side, side, C, C, small, small, C, 192, 64)
    pattern = ((torch.arange(B * small * small * 192) % 13).float() - 6).half().view(B, small, small, 192)
    got = _run_row(row, B, x16, pattern)
    assert small == 3 and torch.equal(got[..., 64:128].double(), fid._pool_eager(fid.OP_MAXPOOL_S2, nchw(x16)).permute(0, 2, 3, 1))
    assert torch.equal(got[..., :64], pattern[..., :64]) and torch.equal(got[..., 128:], pattern[..., 128:])


def _input(src, out, **kw):
    from leftrefill_amd import ops
    n = src.shape[0]
    return ops.fid_input(src, torch.empty(n, out, out, 4, dtype=torch.float16, device=DEV), out, **kw)


def test_input_eight_bit_stage_equals_eval_metrics_bytes():
    """At out == in the resize is the identity, so the stored fp16 2 b / 255 - 1 names the byte b: they must be lr_eval_metrics' rgb8 of
    the same composited batch, byte for byte (fp16 separates neighbouring bytes: 2 / 255 is 8 ulps at 1)."""
    from leftrefill_amd import ops
    g = torch.Generator().manual_seed(5)
    N, H, W = 2, 32, 64
    pred = (torch.rand(N, 3, H, W, generator=g) * 2.6 - 1.3).half().to(DEV)      # some values leave [-1, 1]
    origin = (torch.rand(N, 3, H, W, generator=g) * 2 - 1).to(DEV)
    mask = (torch.rand(N, 1, H, W, generator=g) < 0.5).float().to(DEV)
    _, rgb8 = ops.eval_metrics(pred, origin, mask, x0=W // 2, Wc=H, r=1, want_rgb8=True)
    got = _input(pred, H, x0=W // 2, Wc=H, origin=origin, mask=mask)
    assert not got[..., 3].any()
    b = torch.round((got[..., :3].double() + 1) / 2 * 255)
    assert torch.equal(b.to(torch.uint8), rgb8) and len(torch.unique(rgb8)) > 200
    assert torch.equal(_input(rgb8, H), got)      # the uint8 route continues from the same bytes with the same arithmetic


def _ulp16(v):
    return 2.0 ** (torch.floor(torch.log2(v.abs().clamp_min(2.0 ** -14))) - 10)


@pytest.mark.parametrize("side", [256, 512])
def test_input_resize_against_float64_interpolate(side):
    """256 -> 299 (enlarging) and 512 -> 299 (shrinking, no antialiasing), from uint8 and from an fp16 NCHW canvas with x0 = W / 2:
    within one fp16 ulp of F.interpolate in float64 on the same bytes."""
    u8 = C.images(1, side, side, seed=side)
    want = fid.preprocess(u8, torch.float64).permute(0, 2, 3, 1)
    got = _input(u8.to(DEV), fid.SIZE).cpu()
    err = (got[..., :3].double() - want).abs()
    print(side, "uint8: max err", float(err.max()), "in ulps", float((err / _ulp16(want)).max()))
    assert (err <= _ulp16(want)).all() and not got[..., 3].any()
    g = torch.Generator().manual_seed(side)
    canvas = (torch.rand(1, 3, side, 2 * side, generator=g) * 2.2 - 1.1).half()
    want = fid.preprocess(fid.to_uint8(canvas[:, :, :, side:]).permute(0, 2, 3, 1), torch.float64).permute(0, 2, 3, 1)
    got = _input(canvas.to(DEV), fid.SIZE, x0=side, Wc=side).cpu()
    err = (got[..., :3].double() - want).abs()
    print(side, "fp16 NCHW: max err", float(err.max()), "in ulps", float((err / _ulp16(want)).max()))
    assert (err <= _ulp16(want)).all()


@pytest.fixture(scope="module")
def packed():
    return fid.pack_fid(fid.FIDInception().load_weights(fid.seeded_state_dict(0)).to(DEV))


def test_whole_network_against_float64(packed):
    from leftrefill_amd import ops
    u8, ref, emu = C.references(3, 64, 64, 11)
    floor = C.rel_l2(emu, ref)
    apart = C.rel_l2(ref[1:2], ref[0:1])[0]
    before = ops.FID_LAUNCHES.value
    got = fid.fid_features(u8.to(DEV), packed)
    launches = ops.FID_LAUNCHES.value - before
    again = fid.fid_features(u8.to(DEV), packed)
    alone = fid.fid_features(u8[:1].to(DEV), packed)
    errs = C.rel_l2(got.cpu(), ref)
    print("floor e per image", floor, "kernel rel-L2 per image", errs, "images 0 / 1 apart", apart, "launches", launches)
    _profile("whole_network", dict(images="3 seeded 64 x 64, seeded_state_dict(0)", floor_e=floor, kernel_rel_l2=errs, images_apart=apart,
                                   kernel_vs_emulation=C.rel_l2(got.cpu(), emu), launches=launches))
    assert got.shape == (3, 2048) and got.dtype == torch.float32 and torch.isfinite(got).all()
    assert launches == len(fid.FID_PROGRAM) + 2
    assert torch.equal(got, again) and torch.equal(alone, got[:1])
    assert apart > 20 * max(floor)      # the images are distinct at the scale the bound resolves
    for i in range(3):
        assert errs[i] <= 2 * floor[i], (i, errs[i], floor[i])


def test_statistics_against_numpy():
    from leftrefill_amd import ops
    g = torch.Generator().manual_seed(9)
    f = torch.randn(8, 2048, generator=g).abs() * torch.rand(8, 2048, generator=g)
    fd = f.to(DEV)

    def run():
        total = torch.zeros(2048, dtype=torch.float64, device=DEV)
        gram = torch.zeros(2048, 2048, dtype=torch.float64, device=DEV)
        ops.fid_accumulate(fd[:5].contiguous(), total, gram)
        ops.fid_accumulate(fd[5:].contiguous(), total, gram)
        return total, gram

    total, gram = run()
    total2, gram2 = run()
    assert torch.equal(total, total2) and torch.equal(gram, gram2)
    x = f.double().numpy()
    n = 8
    assert (np.abs(total.cpu().numpy() - x.sum(0)) <= n * 2.0 ** -52 * np.abs(x).sum(0)).all()
    assert (np.abs(gram.cpu().numpy() - x.T @ x) <= n * 2.0 ** -52 * (np.abs(x).T @ np.abs(x))).all()
    st = fid.FIDStats()
    st.update(fd[:5])
    st.update(fd[5:])
    s, gr, cnt = st.sums()
    assert cnt == 8 and np.array_equal(s, total.cpu().numpy()) and np.array_equal(gr, gram.cpu().numpy())


def test_device_fid_against_host_fid():
    """Two sets of 8 small images through both routes.  n = 8 of 2048 features is rank-deficient: the two numbers are recorded, and
    the device route's own statistics pushed through the host frechet_distance must BE DeviceFID.compute() -- same function, same sums."""
    sd = fid.seeded_state_dict(0)
    pred, real = C.images(8, 32, 32, 31).to(DEV), C.images(8, 32, 32, 32).to(DEV)
    dev, host = fid.DeviceFID().load_weights(sd).to(DEV), fid.HostFID().load_weights(sd).to(DEV)
    with pytest.raises(ValueError):
        dev.compute()
    for route in (dev, host):
        route.update_images(pred[:4], real[:4])
        route.update_images(pred[4:], real[4:])
    d, h = dev.compute(), host.compute()
    print("DeviceFID", d, "HostFID", h)
    _profile("device_vs_host", dict(sets="2 x 8 seeded 32 x 32 images, seeded_state_dict(0)", device_fid=d, host_fid=h))
    assert np.isfinite(d) and np.isfinite(h) and d > 0
    mine = fid.frechet_distance(*fid.stats_from_sums(*dev.pred_stats.sums()), *fid.stats_from_sums(*dev.real_stats.sums()))
    assert mine == d
    mu_d, _ = fid.stats_from_sums(*dev.pred_stats.sums())
    mu_h, _ = fid.stats_from_sums(*host.pred_stats.sums())
    assert np.linalg.norm(mu_d - mu_h) <= 1e-2 * np.linalg.norm(mu_h)      # the two routes see the same images (floor ~5e-4 per image)
    # update(): the composited right half and the origin's, as device_metrics takes them
    g = torch.Generator().manual_seed(33)
    out = {"pred": (torch.rand(2, 3, 32, 64, generator=g) * 2 - 1).half().to(DEV), "origin_image": (torch.rand(2, 3, 32, 64, generator=g) * 2 - 1).to(DEV)}
    mask = (torch.rand(2, 32, 64, 1, generator=g) < 0.5).float().to(DEV)
    dev.reset()
    host.reset()
    dev.update(out, mask)
    host.update(out, mask)
    assert dev.pred_stats.n == dev.real_stats.n == 2
    for a, b in ((dev.pred_stats, host.pred_stats), (dev.real_stats, host.real_stats)):
        assert np.linalg.norm(a.sums()[0] - b.sums()[0]) <= 1e-2 * np.linalg.norm(b.sums()[0])
    dev.reset()
    with pytest.raises(ValueError):
        dev.compute()


@pytest.mark.parametrize("what", ["arena_offset", "channel_range", "weight_offset"])
def test_invalid_row_is_refused_before_any_launch(what):
    from leftrefill_amd import ops
    B, H, W, ci, co = 1, 4, 4, 64, 64
    cs, x16, w, b, y, _ = _conv_case(B, H, W, ci, co, (1, 1), 1, (0, 0), seed=3)
    good = _row(fid.OP_CONV, B, H, W, cs, cs, H, W, co, 128, 64, (1, 1), 1, (0, 0))
    bad = good.copy()
    if what == "arena_offset":
        bad[0, fid.W_DST_OFF] = good[0, fid.W_DST_OFF] + 8        # the destination region now ends 8 halves past the arena
    elif what == "channel_range":
        bad[0, fid.W_DST_C0] = 68                                    # [68, 132) of a 128-wide destination
    else:
        bad[0, fid.W_W_OFF] = 8                                      # [8, 8 + 64 * 64) of a 64 * 64 blob
    sentinel = torch.full((B, H, W, 128), -7.0).half()
    wt, bias = _pack_single(w, cs).to(DEV), b.to(DEV)
    before = ops.FID_LAUNCHES.value
    with pytest.raises(RuntimeError, match="bad argument"):
        _run_row(np.concatenate([good, bad]), B, x16, sentinel, wt, bias)      # the valid first row is not launched either
    assert ops.FID_LAUNCHES.value == before
    got = _run_row(good, B, x16, sentinel, wt, bias)
    assert ops.FID_LAUNCHES.value == before + 1
    assert torch.equal(got[..., :64], sentinel[..., :64]) and (got[..., 64:] >= 0).all() and float(got[..., 64:].max()) > 0
