"""CPU: the numpy statement of the one-call inpainting route (leftrefill_amd/refill.py) against Pillow itself -- the resampler, the luma
threshold, the edge pad, `prepare_numpy` against a transcription with PIL calls, the sizes -- and the binding of the two new symbols."""
import os

import numpy as np
import pytest
from PIL import Image

import abi_helpers as abi
from leftrefill_amd import refill

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
# (h, w) -> (H, W)
CASES = [((37, 53), (64, 64)), ((96, 70), (64, 64)), ((64, 64), (91, 64)), ((64, 64), (33, 64)), ((200, 300), (64, 64)),
         ((64, 64), (64, 64)), ((5, 7), (64, 64)), ((301, 199), (128, 128)), ((64, 128), (512, 200))]
FILTERS = {"bicubic": Image.Resampling.BICUBIC, "bilinear": Image.Resampling.BILINEAR}


def _case_id(case):
    (h, w), (H, W) = case
    return f"{h}x{w}_to_{H}x{W}"


@pytest.mark.parametrize("filter", sorted(FILTERS))
@pytest.mark.parametrize("case", CASES, ids=_case_id)
def test_resize_u8_equals_pil(case, filter):
    (h, w), (H, W) = case
    rng = np.random.RandomState(h * 1000 + w)
    for c in (3, 1):
        a = rng.randint(0, 256, (h, w, c), dtype=np.uint8)
        a = a[:, :, 0] if c == 1 else a
        want = np.asarray(Image.fromarray(a).resize((W, H), resample=FILTERS[filter]))
        got = refill.resize_u8(a, W, H, filter)
        assert got.dtype == np.uint8 and got.shape == want.shape and np.array_equal(got, want)
    assert got is not a and not np.shares_memory(got, a)      # the identity case is a copy


@pytest.mark.parametrize("filter", sorted(FILTERS))
def test_resize_u8_checkerboard_hits_both_clamps(filter):
    yy, xx = np.mgrid[0:48, 0:80]
    a = np.repeat((((yy + xx) % 2) * 255).astype(np.uint8)[:, :, None], 3, axis=2)
    a[:, :, 1] = 255 - a[:, :, 1]
    for W, H in ((131, 77), (64, 64), (80, 96)):
        want = np.asarray(Image.fromarray(a).resize((W, H), resample=FILTERS[filter]))
        assert np.array_equal(refill.resize_u8(a, W, H, filter), want)
    # 2-pixel blocks: the bicubic overshoot leaves [0, 255] on both sides before the clamp
    b = np.repeat(np.repeat(a[:24, :40], 2, axis=0), 2, axis=1)
    lo, cnt, kk = refill.pil_coeffs(b.shape[1], 131, "bicubic")
    raw = [(1 << 21) + sum(int(kk[i, j]) * int(b[0, lo[i] + j, 0]) for j in range(cnt[i])) >> 22 for i in range(131)]
    assert min(raw) < 0 and max(raw) > 255
    want = np.asarray(Image.fromarray(b).resize((131, 77), resample=Image.Resampling.BICUBIC))
    assert np.array_equal(refill.resize_u8(b, 131, 77, "bicubic"), want) and want.min() == 0 and want.max() == 255


def test_pil_coeffs_rows_stay_inside_the_axis_and_fit_32_bits():
    for n_in, n_out in ((53, 64), (300, 64), (7, 64), (4000, 512), (16384, 64)):
        for f, support in refill.FILTER_SUPPORT.items():
            lo, cnt, kk = refill.pil_coeffs(n_in, n_out, f)
            assert kk.shape == (n_out, refill.pil_ksize(n_in, n_out, f)) and lo.dtype == cnt.dtype == kk.dtype == np.int32
            assert (lo >= 0).all() and (cnt >= 1).all() and (lo + cnt <= n_in).all() and (cnt <= kk.shape[1]).all()
            assert np.abs(kk.astype(np.int64)).sum(axis=1).max() < 1.4 * 2 ** 22
            assert all((kk[i, cnt[i]:] == 0).all() for i in range(n_out))
    assert refill.pil_ksize(16384, 64, "bicubic") == refill.MAX_KSIZE == 1025      # the cap admits exactly this shrink
    assert refill.refused((16500, 8, 3), (8, 64), "bicubic") and not refill.refused((16384, 8, 3), (8, 64), "bicubic")


def test_luma_threshold_equals_convert_L():
    colours = np.array([[r, g, b] for r in (0, 255) for g in (0, 255) for b in (0, 255)], np.uint8)
    rnd = np.random.RandomState(3).randint(0, 256, (4096, 3), dtype=np.uint8)
    px = np.concatenate([colours, rnd])[None]
    L = np.asarray(Image.fromarray(px).convert("L")).astype(np.float32) / 255.0
    want = np.where(L >= 0.5, 1.0, 0.0).astype(np.float32)
    got = refill.luma_mask(px)
    assert np.array_equal(got, want) and 0 < got.mean() < 1


@pytest.mark.parametrize("size", [64, 100, 128, 130, 512])
def test_pad_equals_np_pad_edge(size):
    p = refill.plan((30, 40), size)
    a = np.random.RandomState(size).randint(0, 256, (size, size, 3), dtype=np.uint8)
    want = np.pad(a, ((0, p["H"] - size), (0, p["W"] - size), (0, 0)), mode="edge")
    assert np.array_equal(refill.pad_edge(a, p["H"], p["W"]), want)
    assert p["H"] == p["W"] == {64: 128, 100: 128, 128: 128, 130: 192, 512: 512}[size] and p["canvas"] == (p["H"], 2 * p["W"])


def _inputs(hs, ws, hr, wr, seed=0):
    rng = np.random.RandomState(seed)
    source = rng.randint(0, 256, (hs, ws, 3), dtype=np.uint8)
    reference = rng.randint(0, 256, (hr, wr, 3), dtype=np.uint8)
    mask = np.zeros((hs, ws, 3), np.uint8)
    mask[hs // 4:hs // 2, ws // 5:ws // 2] = 255      # a stroke
    mask[hs // 2:hs // 2 + 3, :] = 255
    mask[hs - 5, ws - 7] = (0, 0, 200)                # a coloured pixel: > 0 -> 255 per channel, then a luma below the threshold
    mask[3, 4] = (0, 90, 0)
    return source, mask, reference


def _prepare_with_pil(source, mask, reference, size, n):
    """`predict` 167-188 and `make_batch_sd` of the reference's interactive entry point, said with PIL and numpy calls."""
    src = Image.fromarray(source).resize((size, size), resample=Image.Resampling.BICUBIC)
    ref = Image.fromarray(reference).resize((size, size), resample=Image.Resampling.BICUBIC)
    m = np.array(Image.fromarray(mask).resize((size, size), resample=Image.Resampling.BILINEAR))
    m[m > 0] = 255

    def pad(img):
        a = np.asarray(img)
        pw, ph = np.max(((2, 2), np.ceil(np.array([a.shape[1], a.shape[0]]) / 64).astype(int)), axis=0) * 64 - [a.shape[1], a.shape[0]]
        return np.pad(a, ((0, ph), (0, pw), (0, 0)), mode="edge")
    src, ref, m = pad(src), pad(ref), pad(m)
    canvas = np.concatenate([ref, src], axis=1)
    m = np.concatenate([np.zeros_like(m), m], axis=1)
    image = canvas[None].transpose(0, 3, 1, 2).astype(np.float32) / np.float32(127.5) - np.float32(1.0)
    L = np.array(Image.fromarray(m).convert("L")).astype(np.float32) / np.float32(255.0)
    L = L[None, None]
    L[L < 0.5] = 0
    L[L >= 0.5] = 1
    masked = image * (L < 0.5)
    return tuple(np.repeat(a, n, axis=0) for a in (image, masked.astype(np.float32), L))


@pytest.mark.parametrize("size,shape", [(64, (96, 70)), (128, (50, 120)), (100, (77, 77))])
def test_prepare_numpy_equals_the_transcription(size, shape):
    source, mask, reference = _inputs(*shape, 120, 50, seed=size)
    want = _prepare_with_pil(source, mask, reference, size, 2)
    for resize in (refill.resize_u8, refill.resize_pil):
        got = refill.prepare_numpy(source, mask, reference, size, 2, resize=resize)
        for g, w in zip(got, want):
            assert g.dtype == np.float32 and g.shape == w.shape and np.array_equal(g, w)
    image, masked, m = got
    H = refill.plan(shape, size)["H"]
    assert image.shape == (2, 3, H, 2 * H) and m.shape == (2, 1, H, 2 * H) and not m[:, :, :, :H].any() and 0 < m[:, :, :, H:].mean() < 1


def test_finish_numpy_composite_crop_and_resize():
    rng = np.random.RandomState(1)
    H = W = 128
    pred = (rng.rand(2, 3, H, 2 * W).astype(np.float32) * 3 - 1.5)
    image = rng.randint(0, 256, (2, 3, H, 2 * W)).astype(np.float32) / np.float32(127.5) - np.float32(1.0)
    mask = (rng.rand(2, 1, H, 2 * W) < 0.5).astype(np.float32)
    out = refill.finish_numpy(pred, image, mask, (45, 64))
    x = (pred * mask + image * (1 - mask))[:, :, :, W:]
    u8 = (np.clip((x + 1) / 2, 0, 1) * 255).transpose(0, 2, 3, 1).astype(np.uint8)
    for o, a in zip(out, u8):
        assert o.shape == (64, 45, 3) and np.array_equal(o, np.asarray(Image.fromarray(a).resize((45, 64), resample=Image.Resampling.BICUBIC)))
    assert u8.min() == 0 and u8.max() == 255


def test_plan_sizes():
    p = refill.plan((3000, 4000), 512)
    assert (p["Sh"], p["Sw"], p["H"], p["W"], p["canvas"]) == (512, 512, 512, 512, (512, 1024))
    assert p["out_wh"] == (int(512 / (3000 / 4000)), 512) == (682, 512)
    assert refill.plan((96, 70), 64)["out_wh"] == (int(64 / (96 / 70)), 64) == (46, 64)
    assert refill.plan((50, 120), 64)["out_wh"] == (153, 64) and refill.plan((50, 120), 64)["canvas"] == (128, 256)
    assert refill.plan((10, 10), 130)["canvas"] == (192, 384)


def test_prompt_string():
    assert refill.prompt(4, "<special-token>") == "<special-token0> <special-token1> <special-token2> <special-token3>"
    want = ""
    for i in range(50):
        want = want + "<special-token>".replace(">", f"{i}> ")
    assert refill.prompt() == want.strip()


def test_resize_table_shares_axes_and_places_results():
    t = refill.ResizeTable()
    a = t.add(0, (96, 70, 3), (64, 64), "bicubic")
    b = t.add(96 * 70 * 3, (96, 70, 3), (64, 64), "bicubic")
    c = t.add(2 * 96 * 70 * 3, (64, 64, 1), (64, 64), "bilinear")
    tables, jobs = t.arrays()
    assert (a, b, c) == (0, 64 * 64 * 3, 2 * 64 * 64 * 3) and t.dst_bytes == 2 * 64 * 64 * 3 + 64 * 64
    assert jobs["h_off"][0] == jobs["h_off"][1] and jobs["v_off"][0] == jobs["v_off"][1] and jobs["tmp_off"][1] == 96 * 64 * 3
    assert (jobs["h_ksize"][2], jobs["v_ksize"][2]) == (0, 0) and t.work_bytes == 2 * 96 * 64 * 3
    lo, cnt, kk = refill.pil_coeffs(70, 64, "bicubic")
    o = int(jobs["h_off"][0])
    assert np.array_equal(tables[o:o + 64], lo) and np.array_equal(tables[o + 64:o + 128], cnt)
    assert np.array_equal(tables[o + 128:o + 128 + kk.size].reshape(kk.shape), kk) and jobs["h_ksize"][0] == kk.shape[1]


def test_header_binding_and_source_list_agree_on_the_new_symbols():
    from leftrefill_amd import _lib, build
    for name, count in (("lr_pil_resize", 13), ("lr_refill_canvas", 13)):
        assert len(abi.c_params(name)) == count, name
    assert "pil_resample.hip" in build.SOURCES and _lib.ABI_VERSION == 30
    assert "lr_abi_version(void) { return 30; }" in open(os.path.join(ROOT, "leftrefill_amd", "csrc", "elementwise.hip")).read()
    assert abi.define("LR_PIL_MAX_KSIZE") == refill.MAX_KSIZE
    from leftrefill_amd import ops
    assert ops.PIL_MAX_KSIZE == refill.MAX_KSIZE
