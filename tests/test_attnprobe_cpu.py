"""Attention-map probe, host side (no GPU): the float64 statement `probe_reference`, the canvas columns, the CFG fold, the read-outs,
the C-ABI surface of lr_attention_probe_f16 and the logger's `att_scores` panels."""
import inspect
import os

import numpy as np
import pytest
import torch

from leftrefill_amd import attnprobe as AP

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _dense(q, k, cols, B, heads, Nq, Nkv, scale):
    """The formula with python loops over samples, heads and queries."""
    out = torch.zeros(B, Nq, cols.shape[1], dtype=torch.float64)
    for b in range(B):
        for h in range(heads):
            for i in range(Nq):
                qv = q[b * Nq + i, h * 64:(h + 1) * 64].double()
                s = torch.stack([scale * (qv * k[b * Nkv + j, h * 64:(h + 1) * 64].double()).sum() for j in range(Nkv)])
                p = torch.exp(s - s.max())
                p = p / p.sum()
                out[b, i] += (p[:, None] * cols.double()).sum(0) / heads
    return out


def test_probe_reference_is_the_dense_softmax_on_three_keys():
    # one head, one query, three keys with logits log(1), log(2), log(5) -> p = (1, 2, 5) / 8
    q = torch.zeros(1, 64, dtype=torch.float16)
    q[0, 0] = 1.0
    k = torch.zeros(3, 64, dtype=torch.float16)
    k[:, 0] = torch.tensor([0.0, np.log(2.0), np.log(5.0)]).half()
    cols = torch.tensor([[1.0, 0.0], [0.0, 1.0], [1.0, 3.0]], dtype=torch.float16)
    out = AP.probe_reference(q, k, cols, 1, 1, 1, 3, 1.0)
    lg = k[:, 0].double()
    p = torch.exp(lg) / torch.exp(lg).sum()
    assert out.dtype == torch.float64 and out.shape == (1, 1, 2)
    assert torch.allclose(out[0, 0], torch.stack([p[0] + p[2], p[1] + 3 * p[2]]), rtol=0, atol=1e-15)
    assert abs(out[0, 0, 0].item() - 6 / 8) < 2e-3      # (fp16 rounding of the logarithms)
    # two samples, two heads, strided operands, scale != 1: against the loops
    g = torch.Generator().manual_seed(3)
    B, heads, Nq, Nkv = 2, 2, 2, 3
    qkv = torch.randn(B * Nkv, 3 * 128, generator=g).half()
    qq = torch.randn(B * Nq, 128, generator=g).half()
    cols = torch.randn(Nkv, 4, generator=g).half()
    got = AP.probe_reference(qq, qkv[:, 128:256], cols, B, heads, Nq, Nkv, 0.37)
    assert torch.allclose(got, _dense(qq, qkv[:, 128:256], cols, B, heads, Nq, Nkv, 0.37), rtol=0, atol=1e-13)


def test_probe_reference_rows_sum_to_one():
    g = torch.Generator().manual_seed(4)
    q, k = torch.randn(2 * 5, 192, generator=g).half(), torch.randn(2 * 7, 192, generator=g).half()
    out = AP.probe_reference(q, k, torch.ones(7, 1, dtype=torch.float16), 2, 3, 5, 7, 0.125)
    assert torch.allclose(out, torch.ones_like(out), rtol=0, atol=1e-14)


@pytest.mark.parametrize("dtype", [torch.float16, torch.bfloat16], ids=["f16", "bf16"])
@pytest.mark.parametrize("h,w", [(2, 1), (1, 2), (3, 6), (8, 16), (5, 7), (64, 128)])
def test_canvas_columns(dtype, h, w):
    cols = AP.canvas_columns(h, w, dtype)
    assert cols.shape == (h * w, 3) and cols.dtype == dtype
    for y in range(h):
        for x in range(w):
            ref = 1 if x < w // 2 else 0
            assert cols[y * w + x].tolist() == [ref, ref * x, ref * y], (y, x)      # exact in the 16-bit type
    assert cols.float().max().item() <= 128


def test_fold_cfg():
    u, c = torch.tensor([0.2, 0.5]), torch.tensor([0.4, 0.1])
    assert torch.equal(AP.fold_cfg(u, c, 2.5), u + 2.5 * (c - u))
    assert torch.equal(AP.fold_cfg(u, c, 1.0), u + (c - u)) and torch.equal(AP.fold_cfg(u, c, 0.0), u)


class _NoUNet:
    _run_plan = None


def test_read_outs_and_nan_where_the_mass_is_zero():
    p = AP.AttentionProbe(_NoUNet(), layers=[0])
    h, w = 2, 4
    acc = torch.zeros(1, h * w, 3)
    acc[0, 2] = torch.tensor([1.0, 0.5, 1.5])      # target token (0, 2): mass 1 over two steps, looking at (0.5, 1.5)
    acc[0, 7] = torch.tensor([0.5, 0.5, 0.0])      # target token (1, 3)
    acc[0, 0] = torch.tensor([2.0, 2.0, 2.0])      # a reference token: not part of the correspondence
    p._acc[0], p._hw[0], p.steps = acc, (h, w), 2
    assert p.recorded == [0] and p.raw(0).shape == (1, h, w, 3)
    assert torch.equal(p.mass(0), acc[..., 0].view(1, h, w) / 2)
    c = p.correspondence(0)
    assert c.shape == (1, h, w // 2, 2)
    assert c[0, 0, 0].tolist() == [0.5, 1.5] and c[0, 1, 1].tolist() == [1.0, 0.0]
    assert torch.isnan(c[0, 0, 1]).all() and torch.isnan(c[0, 1, 0]).all()
    with pytest.raises(TypeError):
        AP.AttentionProbe(object())


def test_header_binding_and_wrapper_agree():
    import abi_helpers as abi
    from leftrefill_amd import _lib, build, ops
    header = abi.header().text
    for name in ("lr_attention_probe_f16", "lr_attention_probe_bf16"):
        assert len(abi.c_params(name)) == 16, name       # header against binding: tests/test_abi_cpu.py
    assert "lr_attention_probe_f16" in _lib.BF16_TWINS and _lib.SIGNATURES["lr_attention_probe_bf16"] is _lib.SIGNATURES["lr_attention_probe_f16"]
    sig = _lib.SIGNATURES["lr_attention_probe_f16"]
    assert sig[12:15] == [_lib.c_float] * 3 and sig[7] == _lib.c_void_p and sig[6] == _lib.c_int
    assert _lib.ABI_VERSION == 30      # additive: nothing renumbered
    assert "softmax_j(scale * q_h[b,i,:] . k_h[b,j,:]) * cols[j, c]" in header
    assert list(inspect.signature(ops.attention_probe).parameters) == ["q", "k", "cols", "B", "heads", "Nq", "Nkv", "scale", "out", "alpha", "beta"]
    p = inspect.signature(ops.attention_probe).parameters
    assert p["out"].default is None and p["alpha"].default == 1.0 and p["beta"].default == 0.0
    assert "attention_probe.hip" in build.SOURCES and build.EXTRA["attention_probe.hip"] == build.EXTRA["attention.hip"]
    # the softmax exists once: both translation units take it from the shared header
    csrc = os.path.join(ROOT, "leftrefill_amd", "csrc")
    assert "void softmax_block(" in open(os.path.join(csrc, "attention_common.h")).read()
    for f in ("attention.hip", "attention_probe.hip"):
        src = open(os.path.join(csrc, f)).read()
        assert '#include "attention_common.h"' in src and "void softmax_block(" not in src, f


def _logger(**kw):
    import leftrefill_amd.dropin as dropin
    dropin.install()
    from inpainting_ldm.logger import InpaintingLogger
    return InpaintingLogger(**kw)


@pytest.mark.parametrize("B", [3, 1], ids=["grid", "single_image"])
def test_logger_draws_att_scores_on_the_host_route(B):
    pytest.importorskip("matplotlib")
    lg = _logger(max_images=2)
    from inpainting_ldm.logger import mapping_color
    from leftrefill_amd.imagelog import make_grid_numpy
    g = torch.Generator().manual_seed(5)
    H, W = 8, 16
    images = {"masked_image": torch.rand(B, 3, H, W, generator=g) * 2 - 1, "pred": torch.rand(B, 3, H, W, generator=g) * 2 - 1}
    att = [torch.rand(B, 2, 4, generator=g), torch.rand(B, 1, 2, generator=g)]
    plain = lg.canvas(images)
    full = lg.canvas(dict(images, att_scores=att))
    N = min(B, 2)
    pw = W if N == 1 else W + 4
    assert full.dtype == np.uint8 and full.shape == (plain.shape[0], plain.shape[1] + 2 * pw, 3)
    assert np.array_equal(full[:, :plain.shape[1]], plain)
    for i, a in enumerate(att):
        r = torch.nn.functional.interpolate(a[:N].unsqueeze(1), size=[H, W], mode="nearest").numpy()
        want = (mapping_color(make_grid_numpy(r)[0], 0, 1, cmap="viridis") * 255).astype(np.uint8)
        assert np.array_equal(full[:, plain.shape[1] + i * pw:plain.shape[1] + (i + 1) * pw], want), i
    # nearest resize: block (0, 0) of the first map is one colour, the one mapping_color gives its value
    y0 = 0 if N == 1 else 2
    x0 = plain.shape[1] + (0 if N == 1 else 2)
    block = full[y0:y0 + H // 2, x0:x0 + W // 4]
    assert (block == block[0, 0]).all()
    assert np.array_equal(block[0, 0], (mapping_color(att[0][0, :1, :1].numpy(), 0, 1, cmap="viridis") * 255).astype(np.uint8)[0, 0])


def test_logger_log_img_cuts_att_scores_and_writes_the_file(tmp_path):
    pytest.importorskip("matplotlib")
    from types import SimpleNamespace
    from PIL import Image
    lg = _logger(batch_frequency=1, max_images=2, save_dir="s", log_images_kwargs={"return_attn": True})
    g = torch.Generator().manual_seed(6)
    seen = {}

    class M:
        training = False
        local_rank, global_step, current_epoch = 0, 1, 0
        logger = SimpleNamespace(save_dir=str(tmp_path))

        def eval(self):
            pass

        def log_images(self, batch, split, **kw):
            seen.update(kw)
            return {"pred": torch.rand(3, 3, 8, 16, generator=g) * 2 - 1, "att_scores": [torch.rand(3, 2, 4, generator=g)]}

    lg.log_img(M(), {}, 0)
    assert seen == {"return_attn": True}
    im = Image.open(str(tmp_path / "s" / "train" / "gs-000001_e-000000_b-000000.jpg"))
    assert im.size == (2 * (16 + 4), 2 * (8 + 2) + 2)


def test_structure_sampler_still_refuses_return_attn_and_ddim_refuses_ucg_schedule():
    import leftrefill_amd.dropin as dropin
    dropin.install()
    from ldm.models.diffusion.ddim import DDIMSampler, StructureDDIMSampler
    from oracle import ddim_ref

    class Model:
        num_timesteps = 1000
        alphas_cumprod = torch.from_numpy(ddim_ref.alphas_cumprod())
        betas = torch.zeros(1000)
        parameterization = "eps"

        def apply_model(self, *a, **k):
            raise AssertionError("the model must not be called")

    x, c = torch.zeros(1, 4, 8, 16), torch.zeros(1, 77, 8)
    st = StructureDDIMSampler(Model())
    with pytest.raises(NotImplementedError, match="return_attn"):
        st.sample(10, 1, (4, 8, 16), conditioning=c, return_attn=True, verbose=False, Tm=5, cond_simple=c, cond_weight=0.7, x_T=x)
    s = DDIMSampler(Model())
    assert "return_attn" in inspect.signature(s.sample).parameters and "return_attn" in inspect.signature(s.ddim_sampling).parameters
    with pytest.raises(NotImplementedError, match="ucg_schedule"):
        s.sample(10, 1, (4, 8, 16), conditioning=c, return_attn=True, ucg_schedule=[1.0] * 10, verbose=False, x_T=x)
    with pytest.raises(NotImplementedError, match="list conditioning"):
        s.sample(10, 1, (4, 8, 16), conditioning=[c], return_attn=True, verbose=False, x_T=x)
