"""Training of the prompt tokens through the OpenCLIP text tower on the HIP kernels (ABI 29): causal attention forward with its
log-sum-exp and backward, the plain-GELU forward / backward pair, the tower's differentiable sequence (text_engine), the encoders'
`use_hip_backward` switch, the whole prompt-tuning step and the multi-view objective -- against torch autograd and against
tests/golden/prompt_tuning.npz (the REFERENCE's own encoder / LatentDiffusion / multi-view p_losses on the CPU,
tools/make_golden_prompt_tuning.py)."""
import math
import os
import sys

import numpy as np
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

from oracle import golden_spec as G, weights  # noqa: E402

DEV = torch.device("cuda:0")
DTYPES = [torch.float16, torch.bfloat16]


def rel_l2(got, ref):
    got, ref = got.float().cpu(), ref.float().cpu()
    assert torch.isfinite(got).all()
    return ((got - ref).norm() / ref.norm()).item()


def check(name, got, ref, tol=1e-2):
    """rel-L2 bound plus an elementwise bound of a few times it against the largest reference value (test_gpu_backward.check's form)."""
    got, ref = got.float().cpu(), ref.float().cpu()
    assert torch.isfinite(got).all(), name
    err = (got - ref).abs()
    rel = (err.norm() / ref.norm()).item()
    scale = ref.abs().max().item()
    print(f"[{name}] rel_l2 {rel:.3e} max_abs {err.max().item():.3e} (|ref| max {scale:.3e})")
    assert rel < tol, (name, rel)
    assert err.max().item() <= 10 * tol * scale, name


# ---- causal attention ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES, ids=["f16", "bf16"])
@pytest.mark.parametrize("B,heads,N", [(2, 4, 77), (1, 16, 77), (1, 2, 33), (1, 1, 200)])
def test_causal_attention_forward_lse_backward(B, heads, N, dtype):
    from leftrefill_amd import train_ops
    C = heads * 64
    scale = 64 ** -0.5
    qkv = (G.T(f"pt.qkv.{B}.{heads}.{N}", (B * N, 3 * C)) * 1.5).to(DEV, dtype).requires_grad_(True)
    dout = G.T(f"pt.dout.{B}.{heads}.{N}", (B * N, C)).to(DEV, dtype)
    out = train_ops.attention_causal(qkv[:, :C], qkv[:, C:2 * C], qkv[:, 2 * C:], B, heads, N, scale)
    out.backward(dout)

    r = qkv.detach().float().requires_grad_(True)
    q, k, v = (r[:, i * C:(i + 1) * C].reshape(B, N, heads, 64).transpose(1, 2) for i in range(3))
    ref = F.scaled_dot_product_attention(q, k, v, is_causal=True, scale=scale)
    ref.transpose(1, 2).reshape(B * N, C).backward(dout.float())
    ref = ref.transpose(1, 2).reshape(B * N, C)
    err = (out.detach().float() - ref.detach()).abs().max().item()
    print(f"[causal fwd {dtype}] max_abs {err:.3e}")
    # 2e-3 for fp16; bf16 output rounding alone is up to 2^-9 relative (4x fp16's 2^-11 step at |o| ~ 1): 4x the bound
    assert err < 2e-3 * max(1.0, ref.abs().max().item()) * (4 if dtype == torch.bfloat16 else 1), err
    for i, n in enumerate("qkv"):
        check(f"causal d{n} {B}x{heads}x{N} {dtype}", qkv.grad[:, i * C:(i + 1) * C], r.grad[:, i * C:(i + 1) * C])

    # the saved log-sum-exp: log2 domain, lse = log2(sum_j exp(scale q.k_j)) over j <= i
    from leftrefill_amd import _lib
    from leftrefill_amd.ops import _p, _stream
    lib = _lib.load()
    o2 = torch.empty(B * N, C, device=DEV, dtype=dtype)
    lse = torch.empty(B * heads * N, device=DEV, dtype=torch.float32)
    qd = qkv.detach()
    _lib.check(_lib.fn(lib, "lr_attention_causal_lse_f16", dtype)(_p(qd), qd.stride(0), _p(qd[:, C:]), qd.stride(0), _p(qd[:, 2 * C:]),
                                                                 qd.stride(0), _p(o2), C, _p(lse), B, heads, N, float(scale), _stream()),
               "causal_lse")
    torch.cuda.synchronize()
    qf, kf = (qd.float()[:, i * C:(i + 1) * C].reshape(B, N, heads, 64).transpose(1, 2) for i in range(2))
    s = (qf @ kf.transpose(-1, -2)) * scale
    s = s.masked_fill(torch.ones(N, N, dtype=torch.bool, device=DEV).triu(1), float("-inf"))
    lse_ref = torch.logsumexp(s, dim=-1) * (1.0 / math.log(2.0))
    e = (lse.reshape(B, heads, N) - lse_ref).abs().max().item()
    print(f"[causal lse {dtype}] max_abs {e:.3e}")
    assert e < 1e-3, e
    assert torch.equal(o2, out.detach())


def test_causal_backward_rejects_query_split():
    from leftrefill_amd import _lib
    from leftrefill_amd._lib import AttnBwdArgs
    from leftrefill_amd.ops import _p
    lib = _lib.load()
    B, heads, N = 1, 2, 77
    C = heads * 64
    t = torch.zeros(B * N, 3 * C, device=DEV, dtype=torch.float16)
    lse = torch.zeros(B * heads * N, device=DEV, dtype=torch.float32)
    ws = torch.zeros(4 * B * heads * 2 * 128 * 64, device=DEV, dtype=torch.float32)
    sentinel = torch.full((B * N, C), 7.0, device=DEV, dtype=torch.float16)
    a = AttnBwdArgs()
    a.q, a.k, a.v, a.o, a.dout = _p(t), _p(t[:, C:]), _p(t[:, 2 * C:]), _p(t), _p(t)
    a.qt, a.kt, a.dot, a.lse, a.dsum = _p(ws), 0, 0, _p(lse), _p(lse)
    a.dq, a.dk, a.dv = _p(sentinel), _p(sentinel), _p(sentinel)
    a.ldq = a.ldk = a.ldv = a.ldo = a.lddo = 3 * C
    a.ld_qt, a.ld_kt = 4, 0
    a.lddq = a.lddk = a.lddv = C
    a.B, a.heads, a.Nq, a.Nkv, a.scale = B, heads, N, N, 0.125
    for dt in DTYPES:
        assert _lib.fn(lib, "lr_attention_causal_bwd_f16", dt)(a, 0) == -3      # LR_E_UNSUPPORTED
    torch.cuda.synchronize()
    assert (sentinel == 7.0).all()      # nothing was launched


# ---- GELU --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES, ids=["f16", "bf16"])
def test_gelu_forward_backward(dtype):
    from leftrefill_amd import train_ops
    x = (G.T("pt.gelu.x", (333, 4096)) * 3.0).to(DEV, dtype)
    dy = G.T("pt.gelu.dy", (333, 4096)).to(DEV, dtype)
    y = train_ops.gelu_fwd(x)
    xr = x.float().requires_grad_(True)
    yr = F.gelu(xr)
    yr.backward(dy.float())
    e = (y.float() - yr.detach()).abs().max().item()
    print(f"[gelu fwd {dtype}] max_abs {e:.3e}")
    # 2e-3 for fp16, scaled by max|y| / 8 because fp16's rounding step grows with |y| (2^-7 between 8 and 16; x = 3 * N(0, 1) reaches
    # |y| ~ 13); bf16 stores 7 mantissa bits against fp16's 10, so its rounding is 8x coarser: 8x the bound
    assert e < 2e-3 * (8 if dtype == torch.bfloat16 else 1) * max(1.0, yr.abs().max().item() / 8), e
    check(f"gelu bwd {dtype}", train_ops.gelu_bwd(x, dy), xr.grad)


@pytest.mark.parametrize("dtype", DTYPES, ids=["f16", "bf16"])
def test_gemm_conv_gelu_is_differentiable(dtype):
    from leftrefill_amd import train_ops
    M, K, N = 154, 256, 1024
    x = G.T("pt.fc.x", (M, K)).to(DEV, dtype).requires_grad_(True)
    w = (G.T("pt.fc.w", (N, K)) * K ** -0.5).to(dtype)
    b = G.T("pt.fc.b", (N,)) * 0.1
    dy = G.T("pt.fc.dy", (M, N)).to(DEV, dtype)
    y = train_ops.gemm_conv(x, w.to(DEV), B=1, H=1, W=M, taps=1, bias=b.to(DEV), gelu=True)
    y.backward(dy)
    xr = x.detach().float().requires_grad_(True)
    yr = F.gelu(F.linear(xr, w.float().to(DEV), b.to(DEV)))
    yr.backward(dy.float())
    check(f"gemm+gelu fwd {dtype}", y.detach(), yr.detach())
    check(f"gemm+gelu dX {dtype}", x.grad, xr.grad)


# ---- the tower ---------------------------------------------------------------------------------------------------------------
def _stub_tower(width=256, heads=4, layers=3):
    from oracle import clip_stub
    return clip_stub.TextModel(width, heads, layers)


def _eager_encode(m, emb, layer_idx):
    x = (emb + m.positional_embedding).permute(1, 0, 2)
    blocks = m.transformer.resblocks
    for r in blocks[:len(blocks) - layer_idx]:
        x = r(x, attn_mask=m.attn_mask)
    return m.ln_final(x.permute(1, 0, 2))


@pytest.mark.parametrize("dtype", DTYPES, ids=["f16", "bf16"])
@pytest.mark.parametrize("layer_idx", [0, 1], ids=["last", "penultimate"])
def test_text_tower_grad_path(layer_idx, dtype):
    from leftrefill_amd import text_engine
    m = _stub_tower().to(DEV).eval()
    for p in m.parameters():
        p.requires_grad_(False)
    emb = G.T("pt.tower.emb", (3, 77, 256)).half().float()
    dz = G.T("pt.tower.dz", (3, 77, 256))
    tower = text_engine.PackedTextTower(m, layer_idx, compute_dtype=dtype)
    x = emb.to(DEV).requires_grad_(True)
    z = text_engine.encode_with_transformer(x, tower)
    (z * dz.to(DEV)).sum().backward()
    with torch.no_grad():
        z_inf = text_engine.encode_with_transformer(emb.to(DEV), tower)
    err = (z.detach() - z_inf).abs()
    rel = (err.norm() / z_inf.norm()).item()
    print(f"[tower grad path vs no-grad {dtype}] rel_l2 {rel:.3e} max_abs {err.max().item():.3e}")
    assert rel < 3e-3 and err.max().item() < 3e-2      # the inference test's tolerance (test_gpu_text.py)
    mc = m.float().cpu()
    xr = emb.clone().requires_grad_(True)
    zr = _eager_encode(mc, xr, layer_idx)
    (zr * dz).sum().backward()
    check(f"tower dX layer_idx={layer_idx} {dtype}", x.grad, xr.grad)
    if dtype == torch.float16:
        assert rel_l2(z.detach(), zr.detach()) < 3e-3


def test_bf16_no_grad_tower_matches_fp16():
    from leftrefill_amd import text_engine
    m = _stub_tower().to(DEV).eval()
    emb = G.T("pt.tower.emb", (3, 77, 256)).half().float().to(DEV)
    with torch.no_grad():
        z16 = text_engine.encode_with_transformer(emb, text_engine.PackedTextTower(m, 1))
        zb = text_engine.encode_with_transformer(emb, text_engine.PackedTextTower(m, 1, compute_dtype=torch.bfloat16))
    assert rel_l2(zb, z16) < 1.5e-2


# ---- encoders with use_hip_backward = True ---------------------------------------------------------------------------------
@pytest.fixture
def ref_stub_env():
    import leftrefill_amd.dropin as dropin
    from oracle import clip_stub
    dropin.install()
    prev = sys.modules.get("open_clip")
    sys.modules["open_clip"] = clip_stub
    yield
    if prev is None:
        sys.modules.pop("open_clip", None)
    else:
        sys.modules["open_clip"] = prev


class _NoEagerMHA:
    """Makes the eager tower unusable inside the block: proves the HIP route was taken."""

    def __enter__(self):
        self.prev = torch.nn.MultiheadAttention.forward

        def boom(*a, **k):
            raise AssertionError("eager nn.MultiheadAttention ran")
        torch.nn.MultiheadAttention.forward = boom

    def __exit__(self, *exc):
        torch.nn.MultiheadAttention.forward = self.prev


GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "prompt_tuning.npz")


def _golden():
    return np.load(GOLDEN)


def _encoder_grad(emb, inputs, dz, amp=None):
    from ldm.modules.encoders.Refill_modules import PromptCLIPEmbedder
    assert PromptCLIPEmbedder.use_hip_backward is False
    emb.use_hip_backward = True
    emb.special_embeddings.weight.requires_grad_(True)
    with _NoEagerMHA(), torch.autocast("cuda", dtype=amp or torch.float16, enabled=amp is not None):
        z = emb(inputs)
    (z.float() * dz.to(z.device)).sum().backward()
    return z


def _enc_cases():
    return ([("text", n, kw, p, None) for n, kw, p in G.TEXT_CASES] + [("mv", n, kw, p, None) for n, kw, p in G.MV_TEXT_CASES] +
            [("nvs", n, kw, p, ps) for n, kw, p, ps in G.NVS_TEXT_CASES])


_BF16_ENC = ("txt_repeat8_pen", "txt_nvs_pose")
_ENC_PARAMS = [c + (None,) for c in _enc_cases()] + [c + (torch.bfloat16,) for c in _enc_cases() if c[1] in _BF16_ENC]


@pytest.mark.parametrize("kind,name,kw,prompts,pose_shape,amp", _ENC_PARAMS,
                         ids=[c[1] + ("-bf16-autocast" if c[-1] else "") for c in _ENC_PARAMS])
def test_encoder_hip_backward_matches_reference_golden(ref_stub_env, kind, name, kw, prompts, pose_shape, amp):
    """fp16 tower (no autocast) against the fp32 reference: z within the inference test's tolerance, gradients within rel-L2 1e-2.
    Under a bf16 autocast the encoder packs a bf16 tower and the splice / pose MLP run in bf16 as well: bf16 keeps 8 significant bits
    (2^-9 = 2e-3 relative rounding per value against fp16's 2^-12), so z is held to 1.5e-2 and the gradients to 2e-2 there."""
    gold = _golden()
    kw = {k: (list(v) if isinstance(v, list) else v) for k, v in kw.items()}
    torch.manual_seed(0)
    if kind == "text":
        from ldm.modules.encoders.Refill_modules import PromptCLIPEmbedder as E
    elif kind == "mv":
        from ldm.modules.encoders.multiview_Refill_modules import PromptCLIPEmbedder as E
    else:
        from ldm.modules.encoders.NVS_modules import NVSCLIPEmbedder as E
    emb = E(device="cuda", **kw)
    if kind == "nvs" and emb.rel_pos_model is not None:
        emb.rel_pos_model.load_state_dict(G.nvs_pose_state(name, emb.rel_pos_model.state_dict()))
        for p_ in emb.rel_pos_model.parameters():
            p_.requires_grad_(True)
    emb = emb.to(DEV)
    inputs = prompts if pose_shape is None else [prompts, G.T(name + ".rel_pos", pose_shape).to(DEV)]
    zshape = tuple(gold[f"{name}.z_shape"])
    dz = G.T(f"prompt_tuning.{name}.dz", zshape)
    z = _encoder_grad(emb, inputs, dz, amp)
    assert tuple(z.shape) == zshape
    if amp is not None:
        assert getattr(emb, "_lr_tower_bf16", None) is not None, "the bf16 HIP tower must have run"
    tag = f"{name}{'-bf16' if amp else ''}"
    z_rows = z.detach().float()[..., G.NVS_Z_ROWS, :].cpu()
    z_ref = torch.from_numpy(gold[f"{name}.z_rows"])
    err = (z_rows - z_ref).abs()
    rel = (err.norm() / z_ref.norm()).item()
    print(f"[{tag} z rows] rel_l2 {rel:.3e} max_abs {err.max().item():.3e}")
    assert rel < (1.5e-2 if amp else 3e-3) and err.max().item() < (1.5e-1 if amp else 3e-2)
    tol = 2e-2 if amp else 1e-2
    check(f"{tag} d special_embeddings", emb.special_embeddings.weight.grad, torch.from_numpy(gold[f"{name}.d_special"]), tol)
    if kind == "nvs" and emb.rel_pos_model is not None:
        for k, p_ in emb.rel_pos_model.named_parameters():
            ref = torch.from_numpy(gold[f"{name}.d_rel_pos.{k}"])
            check(f"{tag} d rel_pos.{k}", p_.grad[:ref.shape[0]], ref, tol)


# ---- the whole prompt-tuning step and the multi-view objective --------------------------------------------------------------
def _ldm(cls, cfg, sd, target="ldm.modules.diffusionmodules.openaimodel.UNetModel", **extra):
    m = cls(first_stage_config={"target": "torch.nn.Identity"}, cond_stage_config={"target": "torch.nn.Identity"},
            unet_config={"target": target, "params": cfg.kwargs()},
            conditioning_key="hybrid", scale_factor=0.18215, linear_start=0.00085, linear_end=0.0120,
            timesteps=1000, channels=4, data_config={"img_size": 256}, **extra)
    m.model.diffusion_model.load_state_dict(sd, strict=True)
    m = m.to(DEV).train()
    for p_ in m.parameters():
        p_.requires_grad_(False)
    return m


def test_prompt_tuning_step_matches_reference_golden(ref_stub_env):
    """RefInpaintLDM.p_losses with the stub-1024 encoder on HIP (tower forward + backward) and loss scale 2^14 against golden (b); then an
    AdamW step over the encoder's parameters moves only special_embeddings."""
    from inpainting_ldm.ref_inpainting_ldm import RefInpaintLDM
    from ldm.modules.encoders.Refill_modules import PromptCLIPEmbedder
    from tools import make_golden_prompt_tuning as MG
    gold = _golden()
    case, B, h, w, ts = G.TRAIN_CASES[0]
    m = _ldm(RefInpaintLDM, MG.PT_UNET, MG.pt_unet_state())
    torch.manual_seed(0)
    emb = PromptCLIPEmbedder(device="cuda", **MG.PT_KW).to(DEV)
    emb.use_hip_backward = True
    emb.special_embeddings.weight.requires_grad_(True)
    before = {k: v.detach().clone() for k, v in emb.state_dict().items()}
    x_start, noise = (G.T(case + s_, (B, 4, h, w)).to(DEV) for s_ in (".x_start", ".noise"))
    c_concat = G.T(case + ".c_concat", (B, 5, h, w)).to(DEV)
    t = torch.tensor(ts, dtype=torch.long, device=DEV)
    with _NoEagerMHA():
        z = emb(MG.PT_PROMPTS[:B])
    loss, ld = m.p_losses(x_start, {"c_concat": [c_concat], "c_crossattn": [z]}, t, noise=noise)
    scale = 2.0 ** 14
    (loss * scale).backward()
    grad = emb.special_embeddings.weight.grad.float().cpu() / scale
    ref_loss = float(gold["step.loss"])
    print(f"[prompt-tuning step] loss {loss.item():.6f} (reference {ref_loss:.6f})")
    assert set(ld) == {"train/loss_simple", "train/loss_vlb", "train/loss"}
    assert abs(loss.item() - ref_loss) <= 2e-3 * ref_loss
    check("step d special_embeddings", grad, torch.from_numpy(gold["step.d_special"]))
    opt = torch.optim.AdamW(emb.parameters(), lr=1e-3)      # every parameter: AdamW skips those without a gradient
    emb.special_embeddings.weight.grad /= scale
    opt.step()
    after = emb.state_dict()
    changed = {k for k in before if not torch.equal(before[k], after[k])}
    assert changed == {"special_embeddings.weight"}, changed


@pytest.mark.parametrize("case", [0, 1], ids=["concat_v3", "plain_v2"])
def test_multiview_p_losses_matches_reference_golden(case):
    import leftrefill_amd.dropin as dropin
    dropin.install()
    from inpainting_ldm.multiview_ref_inpainting_ldm import RefInpaintLDM
    from tools import make_golden_prompt_tuning as MG
    from oracle import unet_ref
    gold = _golden()
    name, V, concat, b, h, w, ts = MG.MV_LOSS_CASES[case]
    cfg = G.mv_config(V, concat)
    m = _ldm(RefInpaintLDM, cfg, weights.fill_state_dict(unet_ref.param_shapes(cfg), prefix="unet.MV."),
             target="ldm.modules.diffusionmodules.multiview_unet.MultiViewUnetModel", view_mode=True, view_num=V, concat_target=concat)
    v = V - 1 if concat else V
    n = b * v
    x_start, noise = (G.T(name + s_, (n, 4, h, w)).to(DEV) for s_ in (".x_start", ".noise"))
    c_concat = G.T(name + ".c_concat", (n, 5, h, w)).to(DEV)
    ctx = G.T(name + ".ctx", (n, 77, cfg.context_dim)).to(DEV).requires_grad_(True)
    t = torch.tensor([tt for tt in ts for _ in range(v)], dtype=torch.long, device=DEV)
    loss, ld = m.p_losses(x_start, {"c_concat": [c_concat], "c_crossattn": [ctx]}, t, noise=noise)
    scale = 2.0 ** 14
    (loss * scale).backward()
    ref_loss = float(gold[name + ".loss"])
    print(f"[multi-view p_losses {name}] loss {loss.item():.6f} (reference {ref_loss:.6f})")
    assert sorted(ld) == list(gold[name + ".keys"])
    assert abs(loss.item() - ref_loss) <= 2e-3 * ref_loss
    for k in ("loss_simple", "loss_vlb"):
        ref = float(gold[f"{name}.{k}"])
        assert abs(ld[f"train/{k}"].item() - ref) <= 3e-3 * max(abs(ref), 1e-12), k
    check(f"{name} d context", ctx.grad[:, G.NVS_Z_ROWS].float().cpu() / scale, torch.from_numpy(gold[name + ".dctx_rows"]))
