"""The host side of device scoring (no GPU): the declaration / binding of lr_eval_metrics under ABI 30, `evalglue.metrics_reference`
against the pinned pieces it is composed from, the argument handling of `evalglue.device_metrics*`, and `validation_step` /
`validation_epoch_end` of the three task models against a from-the-definition float64 evaluation of the reference methods
(ref_inpainting_ldm.py:119-157, multiview_ref_inpainting_ldm.py:225-274, NVS_ldm.py:374-412).

The kernel has no CPU path.  Where a test needs `device_metrics*` to run here, `ops.eval_metrics` -- the one call below them -- is
replaced by `metrics_reference` packed into the kernel's output format ([N, 4] fp32), so the real argument handling runs on top of it.
Tolerance of those comparisons: the fp32 output format, 2^-23 relative -> 1e-5 dB on a PSNR below 80 dB and 1e-6 on an SSIM <= 1."""
import json
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from oracle import golden_spec as G

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PSNR_TOL, SSIM_TOL = 1e-5, 1e-6


# ---- 1. header vs binding -----------------------------------------------------------------------------------------------------
def test_eval_metrics_is_declared_bound_and_built_under_abi_30():
    import abi_helpers as abi
    from leftrefill_amd import _lib, build, ops
    header, macro = abi.header().text, abi.define
    params = abi.c_params("lr_eval_metrics")
    assert len(params) == 14
    for p, ct in zip(params, _lib.SIGNATURES["lr_eval_metrics"]):
        want = (_lib.c_void_p if "*" in p or "lr_stream_t" in p else _lib.c_int64 if "int64_t" in p else
                _lib.c_float if p.startswith("float") else _lib.c_int)
        assert ct is want, (p, ct)
    assert "lr_eval_metrics" not in _lib.BF16_TWINS and "lr_eval_metrics_bf16" not in header      # the element type is an argument
    comment = header[header.index("scoring a decoded prediction"):header.index("int lr_eval_metrics(")]
    for cite in ("test_inpainting.py:146", "test_inpainting.py:158", "test_inpainting.py:160-162", "ref_inpainting_ldm.py:119",
                 "multiview_ref_inpainting_ldm.py:225", "NVS_ldm.py:374"):
        assert cite in comment, cite
    assert _lib.ABI_VERSION == 30
    assert "eval_metrics.hip" in build.SOURCES
    assert (ops.EVAL_TILE_H, ops.EVAL_TILE_W, ops.EVAL_SLOT_FLOATS) == (macro("LR_EVAL_TILE_H"), macro("LR_EVAL_TILE_W"),
                                                                        macro("LR_EVAL_SLOT_FLOATS"))
    assert ops.EVAL_PRED_KIND == {torch.float32: macro("LR_EVAL_PRED_F32"), torch.float16: macro("LR_EVAL_PRED_F16"),
                                  torch.bfloat16: macro("LR_EVAL_PRED_BF16")}


# ---- 2. metrics_reference against the pinned pieces ---------------------------------------------------------------------------
def _random_case(n=2, h=64, w=128, seed=0):
    g = torch.Generator().manual_seed(seed)
    origin = torch.rand(n, 3, h, w, generator=g) * 2 - 1
    pred = (origin + 0.3 * torch.randn(n, 3, h, w, generator=g)).clamp(-1, 1)
    blocks = (torch.rand(n, h // 8, w // 8, 1, generator=g) < 0.5).float()
    mask = blocks.repeat_interleave(8, 1).repeat_interleave(8, 2)      # [n, h, w, 1]
    return pred, origin, mask


def _pieces(pred, origin, mask_nhwc, test_size=None, metric_size=None):
    """The pinned functions exactly as the host route calls them (fp32 composite, fp32 psnr01, fp32 luma, float64 ssim_gray)."""
    from leftrefill_amd import evalglue
    p, o = evalglue.compose_prediction({"pred": pred, "origin_image": origin}, mask_nhwc, test_size, metric_size)
    psnr = evalglue.psnr01(p, o).double()
    ssim = torch.tensor([evalglue.ssim_gray(evalglue.rgb_to_gray01(p[j]), evalglue.rgb_to_gray01(o[j])) for j in range(p.shape[0])],
                        dtype=torch.float64)
    return psnr, ssim


def _pieces64(pred, origin, mask_nhwc, r=1):
    """compose_prediction's fp32 composite and crop, then F.interpolate(mode='area'), psnr01's formula and rgb_to_gray01's weights
    evaluated in float64 (both functions cast to fp32 inside, so their formulas are restated here), and ssim_gray as it is."""
    from leftrefill_amd import evalglue
    p, o = evalglue.compose_prediction({"pred": pred, "origin_image": origin}, mask_nhwc)
    assert p.dtype == torch.float32
    p, o = p.double(), o.double()
    if r > 1:
        size = (p.shape[2] // r, p.shape[3] // r)
        p, o = F.interpolate(p, size=size, mode="area"), F.interpolate(o, size=size, mode="area")
    p01, o01 = (p + 1) / 2, (o + 1) / 2
    psnr = 10.0 * torch.log10(1.0 / ((p01 - o01) ** 2).flatten(1).mean(1))
    gray = lambda x: 0.2989 * x[0] + 0.587 * x[1] + 0.114 * x[2]
    ssim = torch.tensor([evalglue.ssim_gray(gray(p01[j]), gray(o01[j])) for j in range(p.shape[0])], dtype=torch.float64)
    return psnr, ssim


@pytest.mark.parametrize("seed", [0, 1, 2])
@pytest.mark.parametrize("r", [1, 2])
def test_metrics_reference_agrees_with_the_pinned_pieces(r, seed):
    """Two comparisons on random inputs with a block mask; r = 2 is F.interpolate(mode='area') followed by the same pieces.

    (a) float64 against float64: compose_prediction's fp32 composite, then the formulas of psnr01 and rgb_to_gray01 in float64 and
        ssim_gray.  Bounds: <= 1e-6 dB in PSNR (what the fp32 composite against the float64 one accounts for) and <= 1e-9 in SSIM.
        Measured here: both differences are exactly 0 (a 0 / 1 mask makes the fp32 composite exact).
    (b) the functions themselves, which cast to fp32 inside.  psnr01 RETURNS fp32: between 16 and 32 dB half an fp32 ulp of the
        result is 9.5e-7 dB before any error of its fp32 mean (2^-23 relative per rounding, 4.3 dB per unit of relative mse error),
        so 1e-6 dB is below what that function can represent; measured over these six cases 2.5e-7 .. 2.6e-6 dB and 6e-10 .. 5e-9 in
        SSIM (fp32 luma, fp32 area mean).  The bound that follows from the format: 4 fp32 ulps of a PSNR below 32 dB = 7.6e-6 dB,
        and 1e-7 in SSIM (one fp32 rounding of a luma in [0, 1] is 6e-8; the mean over > 3000 windows only averages it down)."""
    from leftrefill_amd import evalglue
    pred, origin, mask = _random_case(seed=seed)
    h, w = pred.shape[2:]
    mse_r, psnr_r, ssim_r = evalglue.metrics_reference(pred, origin, mask.permute(0, 3, 1, 2), x0=w // 2, Wc=w // 2, r=r)
    assert psnr_r.dtype == ssim_r.dtype == mse_r.dtype == torch.float64
    assert torch.allclose(psnr_r, 10 * torch.log10(1 / mse_r), rtol=1e-14, atol=0)
    psnr64, ssim64 = _pieces64(pred, origin, mask, r)
    psnr32, ssim32 = _pieces(pred, origin, mask, test_size=h, metric_size=h // r)
    print(f"r={r} seed={seed}: float64 pieces |dpsnr| {(psnr64 - psnr_r).abs().max():.3e} dB |dssim| {(ssim64 - ssim_r).abs().max():.3e}; "
          f"fp32 functions |dpsnr| {(psnr32 - psnr_r).abs().max():.3e} dB |dssim| {(ssim32 - ssim_r).abs().max():.3e}")
    assert (psnr64 - psnr_r).abs().max() <= 1e-6
    assert (ssim64 - ssim_r).abs().max() <= 1e-9
    assert psnr32.max() < 32.0
    assert (psnr32 - psnr_r).abs().max() <= 4 * 2.0 ** -19
    assert (ssim32 - ssim_r).abs().max() <= 1e-7


def test_metrics_reference_on_the_hand_derived_fixture():
    from leftrefill_amd import evalglue
    fx = json.load(open(os.path.join(ROOT, "tests", "golden", "harness_fixture.json")))
    h, w, c = fx["h"], fx["w"], fx["channels"]
    pred = torch.full((1, c, h, w), fx["pred_value"])
    origin = torch.cat([torch.full((1, c, h, w // 2), fx["origin_left_value"]), torch.full((1, c, h, w // 2), fx["origin_right_value"])], dim=3)
    mask = torch.zeros(1, 1, h, w)
    mask[:, :, :, fx["mask_columns"]] = 1.0
    mse, psnr, ssim = evalglue.metrics_reference(pred, origin, mask, x0=w // 2, Wc=w // 2, r=fx["test_size"] // fx["metric_size"])
    assert abs(mse.item() - fx["expected_mse01"]) < 1e-9
    assert abs(psnr.item() - fx["expected_psnr_db"]) < 1e-4
    assert torch.isnan(ssim).all()      # a 2 x 2 image holds no 7 x 7 window
    assert abs(evalglue.metrics_reference(pred, origin, mask, x0=w // 2)[1].item() - fx["expected_psnr_without_downsampling_db"]) < 1e-4
    same = evalglue.metrics_reference(origin, origin)
    assert same[0].item() == 0.0 and same[1].item() == float("inf")


# ---- the kernel's stand-in for CPU runs ---------------------------------------------------------------------------------------
@pytest.fixture
def fake_kernel(monkeypatch):
    """ops.eval_metrics -> metrics_reference in the kernel's output format; records the arguments of every call."""
    from leftrefill_amd import evalglue, ops
    calls = []

    def eval_metrics(pred, origin, mask=None, x0=0, Wc=None, r=1, want_rgb8=False):
        calls.append(dict(mask=mask, x0=x0, Wc=Wc, r=r, want_rgb8=want_rgb8, shape=tuple(pred.shape)))
        mse, psnr, ssim = evalglue.metrics_reference(pred, origin, mask, x0, Wc, r)
        return torch.stack([mse, psnr, ssim, torch.zeros_like(mse)], 1).float(), None

    monkeypatch.setattr(ops, "eval_metrics", eval_metrics)
    return calls


# ---- 4. device_metrics argument handling --------------------------------------------------------------------------------------
def test_device_metrics_argument_handling(fake_kernel):
    from leftrefill_amd import evalglue
    pred, origin, mask = _random_case(h=32, w=64)
    out = {"pred": pred, "origin_image": origin}
    m = evalglue.device_metrics(out, mask)                                   # h != w: columns w//2:
    assert (fake_kernel[-1]["x0"], fake_kernel[-1]["Wc"], fake_kernel[-1]["r"]) == (32, 32, 1)
    assert set(m) == {"psnr", "ssim", "mse", "nonfinite", "rgb8"} and m["psnr"].shape == (2,) and m["rgb8"] is None
    psnr, ssim = _pieces(pred, origin, mask)
    assert (m["psnr"].double() - psnr).abs().max() <= PSNR_TOL and (m["ssim"].double() - ssim).abs().max() <= SSIM_TOL
    sq = {"pred": pred[:, :, :, :32].contiguous(), "origin_image": origin[:, :, :, :32].contiguous()}
    evalglue.device_metrics(sq, mask[:, :, :32])                             # h == w: the whole image
    assert (fake_kernel[-1]["x0"], fake_kernel[-1]["Wc"]) == (0, 32)
    evalglue.device_metrics(sq, mask[:, :, :32], right_half=True)            # the validation_step rule: always w//2:
    assert (fake_kernel[-1]["x0"], fake_kernel[-1]["Wc"]) == (16, 16)
    evalglue.device_metrics(out, None, compose=False)
    assert fake_kernel[-1]["mask"] is None
    evalglue.device_metrics(out, mask, test_size=32, metric_size=16, want_rgb8=True)
    assert fake_kernel[-1]["r"] == 2 and fake_kernel[-1]["want_rgb8"] is True
    evalglue.device_metrics(out, mask, test_size=32, metric_size=32)
    assert fake_kernel[-1]["r"] == 1
    n = len(fake_kernel)
    with pytest.raises(ValueError, match="compose_prediction.*ssim_gray"):
        evalglue.device_metrics(out, mask, test_size=32, metric_size=24)
    assert len(fake_kernel) == n                                             # refused before any launch


def test_device_metrics_multiview_selects_the_mask_like_the_host_route(fake_kernel):
    from leftrefill_amd import evalglue
    g = torch.Generator().manual_seed(3)
    b, v, s = 2, 2, 16
    pred, origin = torch.rand(b, 3, s, s, generator=g) * 2 - 1, torch.rand(b, 3, s, s, generator=g) * 2 - 1
    for concat in (True, False):
        mask = (torch.rand(b * v, s, 2 * s if concat else s, 1, generator=g) < 0.5).float()
        out = {"pred": pred, "origin_image": origin}
        m, gv = evalglue.device_metrics_multiview(out, mask, b)
        p, o, gv_host = evalglue.compose_prediction_multiview(out, mask, b)
        assert gv == gv_host == v
        assert (m["psnr"].double() - evalglue.psnr01(p, o).double()).abs().max() <= PSNR_TOL
        # a last, smaller batch is split by the first batch's view count
        m1, gv1 = evalglue.device_metrics_multiview({"pred": pred[:1], "origin_image": origin[:1]}, mask[:v], b, global_view_num=v)
        assert gv1 == v and abs(m1["psnr"][0].item() - m["psnr"][0].item()) <= PSNR_TOL


# ---- 3. validation_step / validation_epoch_end of the three task models -------------------------------------------------------
def _task_model(module, cls, **extra):
    import leftrefill_amd.dropin as dropin
    dropin.install()
    import importlib
    cfg = G.CONFIGS["SMALL"]
    return getattr(importlib.import_module("inpainting_ldm." + module), cls)(
        first_stage_config={"target": "torch.nn.Identity"}, cond_stage_config={"target": "torch.nn.Identity"},
        unet_config={"target": "ldm.modules.diffusionmodules.openaimodel.UNetModel", "params": cfg.kwargs()},
        conditioning_key="hybrid", scale_factor=0.18215, linear_start=0.00085, linear_end=0.0120, timesteps=1000, channels=4,
        data_config={"img_size": 16, "cfg": 2.5}, **extra)


def _definition(pred, origin, mask_nchw, crop, lpips_fn=None):
    """The body the three reference methods share, in float64: [0, 1] images, optional paste, optional w//2: crop, per-sample PSNR
    (data_range 1) and SSIM of the luma, batch means."""
    from leftrefill_amd import evalglue
    p, o = (pred.double() + 1) / 2, (origin.double() + 1) / 2
    if mask_nchw is not None:
        p = p * mask_nchw.double() + o * (1 - mask_nchw.double())
    if crop:
        w = o.shape[3]
        p, o = p[:, :, :, w // 2:], o[:, :, :, w // 2:]
    gray = lambda x: 0.2989 * x[0] + 0.587 * x[1] + 0.114 * x[2]
    psnr = [float(10 * torch.log10(1 / ((p[i] - o[i]) ** 2).mean())) for i in range(len(p))]
    ssim = [evalglue.ssim_gray(gray(p[i]), gray(o[i])) for i in range(len(p))]
    res = {"psnr": float(np.mean(psnr)), "ssim": float(np.mean(ssim))}
    if lpips_fn is not None:
        res["lpips"] = float(np.mean([lpips_fn((p[i:i + 1] * 2 - 1).float(), (o[i:i + 1] * 2 - 1).float()).item() for i in range(len(p))]))
    return res


def _check(res, want):
    assert set(res) == set(want)
    assert all(type(v) is float for v in res.values())
    assert abs(res["psnr"] - want["psnr"]) <= PSNR_TOL and abs(res["ssim"] - want["ssim"]) <= SSIM_TOL
    if "lpips" in want:
        assert abs(res["lpips"] - want["lpips"]) <= 1e-6      # an fp32 mean of |differences| <= 2


def _stub_lpips(a, b):
    assert a.dtype == torch.float32 and a.shape[0] == 1 and -1.0 <= a.min() and a.max() <= 1.0
    return (a - b).abs().mean().reshape(1, 1, 1, 1)


def _patch_log_images(monkeypatch, model, log, flatten=False):
    seen = {}

    def log_images(batch, N=4, unconditional_guidance_scale=9.0, **kw):
        seen.update(N=N, scale=unconditional_guidance_scale)
        if flatten and batch["image"].dim() == 5:      # the multi-view get_input flattens the batch in place (reference 100-104)
            for k in ("image", "masked_image", "mask"):
                t = batch[k]
                batch[k] = t.reshape(t.shape[0] * t.shape[1], *t.shape[2:])
        return log

    monkeypatch.setattr(model, "log_images", log_images)
    return seen


@pytest.mark.parametrize("module,cls,paste", [("ref_inpainting_ldm", "RefInpaintLDM", True), ("NVS_ldm", "NVSLDM", False)])
def test_validation_step_single_view(monkeypatch, fake_kernel, module, cls, paste):
    """ref model: crops w//2: and pastes the mask; NVS: crops and does NOT paste (NVS_ldm.py:380-381)."""
    model = _task_model(module, cls)
    pred, origin, mask = _random_case(h=16, w=32, seed=1)
    batch = {"image": origin.permute(0, 2, 3, 1), "masked_image": (origin * (1 - mask.permute(0, 3, 1, 2))).permute(0, 2, 3, 1), "mask": mask,
             "txt": [""] * 2}
    log = {"pred": pred, "origin_image": batch["image"].permute(0, 3, 1, 2), "masked_image": batch["masked_image"].permute(0, 3, 1, 2)}
    seen = _patch_log_images(monkeypatch, model, log)
    assert model.loss_fn_alex is None and not hasattr(model, "log")
    res = model.validation_step(batch, 0)
    assert seen == {"N": 2, "scale": 2.5}
    want = _definition(pred, origin, mask.permute(0, 3, 1, 2) if paste else None, crop=True)
    _check(res, want)                                      # no 'lpips' key without loss_fn_alex
    other = _definition(pred, origin, None if paste else mask.permute(0, 3, 1, 2), crop=True)
    assert abs(other["psnr"] - want["psnr"]) > 0.1         # the paste matters on these inputs: the two models must differ
    assert (fake_kernel[-1]["x0"], fake_kernel[-1]["Wc"]) == (16, 16) and (fake_kernel[-1]["mask"] is not None) == paste
    model.loss_fn_alex = _stub_lpips
    logged = {}
    model.log = lambda k, v, sync_dist=False: logged.update({k: (v, sync_dist)})      # what a LightningModule offers
    res = model.validation_step(batch, 1)
    _check(res, _definition(pred, origin, mask.permute(0, 3, 1, 2) if paste else None, crop=True, lpips_fn=_stub_lpips))
    assert logged == {"val/" + k: (v, True) for k, v in res.items()}


@pytest.mark.parametrize("concat", [True, False], ids=["concat_target", "plain"])
def test_validation_step_multiview(monkeypatch, fake_kernel, concat):
    """The mask of canvas 0 of every sample (its target half under concat_target) pastes the target view; nothing is cropped."""
    b, s = 2, 16
    view_num = 3 if concat else 2
    v = view_num - 1 if concat else view_num
    model = _task_model("multiview_ref_inpainting_ldm", "RefInpaintLDM", view_mode=True, view_num=view_num, concat_target=concat)
    g = torch.Generator().manual_seed(7)
    wc = 2 * s if concat else s
    image = torch.rand(b, v, s, wc, 3, generator=g) * 2 - 1
    mask = (torch.rand(b, v, s // 4, wc // 4, 1, generator=g) < 0.5).float().repeat_interleave(4, 2).repeat_interleave(4, 3)
    assert not torch.equal(mask[:, 0], mask[:, 1])         # taking another canvas' mask would show
    batch = {"image": image.clone(), "masked_image": image * (1 - mask), "mask": mask.clone(), "txt": [[""] * b] * v}
    origin = image[:, 0, :, wc - s:].permute(0, 3, 1, 2)
    pred = (origin + 0.3 * torch.randn(b, 3, s, s, generator=g)).clamp(-1, 1)
    seen = _patch_log_images(monkeypatch, model, {"pred": pred, "origin_image": origin}, flatten=True)
    model.loss_fn_alex = _stub_lpips
    res = model.validation_step(batch, 0)
    assert seen == {"N": b * v, "scale": 2.5}
    m0 = mask[:, 0, :, wc - s:].permute(0, 3, 1, 2)
    _check(res, _definition(pred, origin, m0, crop=False, lpips_fn=_stub_lpips))
    assert fake_kernel[-1]["shape"] == (b, 3, s, s) and (fake_kernel[-1]["x0"], fake_kernel[-1]["Wc"]) == (0, s)
    m1 = mask[:, 1, :, wc - s:].permute(0, 3, 1, 2)
    assert abs(_definition(pred, origin, m1, crop=False)["psnr"] - res["psnr"]) > 1e-3


@pytest.mark.parametrize("module,cls", [("ref_inpainting_ldm", "RefInpaintLDM"), ("multiview_ref_inpainting_ldm", "RefInpaintLDM"),
                                        ("NVS_ldm", "NVSLDM")])
def test_validation_epoch_end_averages_per_key(capsys, module, cls):
    model = _task_model(module, cls)
    outs = [{"psnr": 20.0, "ssim": 0.5, "lpips": 0.25}, {"psnr": 30.0, "ssim": 0.75, "lpips": 0.75}, {"psnr": 25.0, "ssim": 1.0}]
    means = model.validation_epoch_end(outs)
    assert means == {"psnr": 25.0, "ssim": 0.75, "lpips": 0.5}
    printed = capsys.readouterr().out
    assert "Steps:" in printed and "psnr 25.0" in printed and "lpips 0.5" in printed
