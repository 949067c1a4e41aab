"""GPU parity: every HIP kernel through the C ABI vs the CPU oracle / golden vectors.

Tolerance (north star): fp16 outputs within rtol 2e-3 / atol 1e-3 of the fp32 reference evaluated on the SAME
fp16-rounded inputs and weights; composite operators (several fp16 round trips inside) get a proportionally
scaled absolute term, stated per test.
"""

import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

from oracle import ddim_ref, golden_spec as G, unet_ref, weights  # noqa: E402

RTOL, ATOL = 2e-3, 1e-3


def dev():
    assert torch.cuda.is_available(), "GPU tests need a MI355X"
    return torch.device("cuda:0")


def h16(x):
    return x.half().float()


def to_tok(x):
    """NCHW fp32 -> [N*H*W, C] fp16 cuda"""
    N, C, H, W = x.shape
    return x.permute(0, 2, 3, 1).reshape(N * H * W, C).half().contiguous().to(dev())


def from_tok(y, N, H, W):
    return y.float().cpu().reshape(N, H, W, -1).permute(0, 3, 1, 2)


import contextlib


@contextlib.contextmanager
def v_path(mode):
    """How V reaches the PV product of ops.attention: "tr" = natural V + LDS transpose read (lr_attention_f16, the default), "vt" =
    lr_transpose_v_f16 + lr_attention_vt_f16 for every length, "reg" = natural V transposed in registers (LR_ATTN_TR=0)."""
    from leftrefill_amd import _lib, ops
    old = (ops.VT_MIN_KEYS, ops.ATTN_VT)
    ops.VT_MIN_KEYS, ops.ATTN_VT = (1, True) if mode == "vt" else (1 << 30, False)
    # "reg" is a variant of developer builds (LR_DEV_VARIANTS); against the product library the mode is the default path again
    dev = _lib.dev_variants()
    if dev:
        _lib.dev_set("LR_ATTN_TR", 0 if mode == "reg" else None)
    try:
        yield
    finally:
        ops.VT_MIN_KEYS, ops.ATTN_VT = old
        if dev:
            _lib.dev_set("LR_ATTN_TR", None)


def need_dev_build():
    """Tests of kernel variants that only a -DLR_DEV_VARIANTS library contains (tools/build_variant.sh dev -DLR_DEV_VARIANTS;
    LEFTREFILL_LIB_PATH=<that .so> pytest ...)."""
    from leftrefill_amd import _lib
    if not _lib.dev_variants():
        pytest.skip("variant compiled in developer builds only (LR_DEV_VARIANTS)")


def report(name, out, ref, rtol=RTOL, atol=ATOL):
    out, ref = out.float().cpu(), ref.float().cpu()
    err = (out - ref).abs()
    tol = atol + rtol * ref.abs()
    bad = (err > tol).sum().item()
    print(f"[{name}] max_abs_err {err.max().item():.3e} rel_l2 {(err.norm() / ref.norm()).item():.3e} "
          f"viol {bad}/{err.numel()}")
    assert torch.isfinite(out).all(), name
    assert bad == 0, f"{name}: {bad} elements outside rtol={rtol} atol={atol}; max err {err.max().item():.3e}"


def test_library_loads_and_abi():
    from leftrefill_amd import _lib
    lib = _lib.load()
    assert lib.lr_abi_version() == _lib.ABI_VERSION


def test_layout_roundtrip():
    from leftrefill_amd import ops
    x = G.T("lay.x", (2, 9, 6, 10)).to(dev())
    y = ops.nchw_to_nhwc(x[:, :4].contiguous(), x[:, 4:].contiguous(), cpad=64)
    assert y.shape == (120, 64)
    ref = to_tok(x.cpu())
    assert torch.equal(y[:, :9], ref)
    assert (y[:, 9:] == 0).all()
    back = ops.nhwc_to_nchw(y, 2, 6, 10, 9, torch.float32)
    assert torch.equal(back.cpu(), h16(x.cpu()))


@pytest.mark.parametrize("C1,C2,N,H,W,eps,silu", [(320, 0, 2, 8, 16, 1e-5, True), (640, 320, 2, 8, 8, 1e-5, True),
                                                  (1280, 1280, 1, 4, 8, 1e-5, True), (640, 0, 2, 16, 8, 1e-6, False),
                                                  (128, 64, 2, 8, 8, 1e-5, True), (1920, 0, 1, 5, 7, 1e-5, True)])
def test_groupnorm(C1, C2, N, H, W, eps, silu):
    from leftrefill_amd import ops
    C = C1 + C2
    x = h16(G.T(f"gn.{C1}.{C2}.x", (N, C, H, W)) * 1.7 + 0.3)
    gamma = torch.from_numpy(weights.fill_like("gn.weight", (C,)))
    beta = torch.from_numpy(weights.fill_like("gn.bias", (C,)))
    ref = F.group_norm(x, 32, gamma, beta, eps)
    if silu:
        ref = F.silu(ref)
    x1 = to_tok(x[:, :C1])
    x2 = to_tok(x[:, C1:]) if C2 else None
    y = ops.group_norm(x1, N, H * W, gamma.to(dev()), beta.to(dev()), eps, silu, x2)
    report(f"groupnorm {C1}+{C2}", from_tok(y, N, H, W), ref)
    y2 = ops.group_norm(x1, N, H * W, gamma.to(dev()), beta.to(dev()), eps, silu, x2)
    assert torch.equal(y, y2), "groupnorm must be bitwise reproducible"


def test_groupnorm_large_mean_small_variance():
    """fp32 single-pass (sum, sumsq) statistics with mean 50, std 0.5 (variance 1e-4 of the mean square): the kernels
    accumulate per-thread partials of few elements and combine them in fp64, so E[x^2] - mean^2 keeps ~4 digits here."""
    from leftrefill_amd import ops
    d = dev()
    N, C, H, W = 2, 320, 16, 32
    x = h16(50.0 + 0.5 * G.T("gn_big.x", (N, C, H, W)))
    gam = 1.0 + 0.3 * G.T("gn_big.g", (C,))
    bet = 0.2 * G.T("gn_big.b", (C,))
    ref = F.silu(F.group_norm(x.double(), 32, gam.double(), bet.double(), 1e-5)).float()
    y = ops.group_norm(to_tok(x), N, H * W, gam.to(d), bet.to(d), 1e-5, True)
    # fp16 inputs near 50 are quantised to 1/32: the normalised values carry that input noise (6e-2 sigma); what is tested
    # is the statistics: any loss in the variance shows up as a uniform scale error of the whole output
    out = from_tok(y, N, H, W)
    scale = (out * ref).sum() / (ref * ref).sum()
    print(f"[gn large mean] fitted scale {scale.item():.6f}  max_abs_err {(out - ref).abs().max().item():.3e}")
    assert abs(scale.item() - 1.0) < 2e-3
    report("gn large mean", out, ref, rtol=4e-3, atol=4e-3)


@pytest.mark.parametrize("M,C", [(256, 320), (77, 640), (130, 1280), (64, 128)])
def test_layernorm(M, C):
    from leftrefill_amd import ops
    x = h16(G.T(f"ln.{C}.x", (M, C)) * 2.0 - 0.5)
    g = torch.from_numpy(weights.fill_like("ln.weight", (C,)))
    b = torch.from_numpy(weights.fill_like("ln.bias", (C,)))
    ref = F.layer_norm(x, (C,), g, b, 1e-5)
    y = ops.layer_norm(x.half().to(dev()), g.to(dev()), b.to(dev()))
    report(f"layernorm {M}x{C}", y, ref)


def test_timestep_embedding_and_time_mlp(golden):
    from leftrefill_amd import ops
    t = torch.tensor([1, 21, 481, 981])
    emb = ops.timestep_embedding(t.to(dev()), 320)
    report("timestep_embedding", emb, torch.from_numpy(golden("ops")["timestep_embedding_320"]))
    # time MLP: Linear(320,1280) -> SiLU -> Linear(1280,1280); then SiLU -> Linear(1280, 640) (emb_layers)
    w0 = h16(torch.from_numpy(weights.fill_like("tm.0.weight", (1280, 320))))
    b0 = torch.from_numpy(weights.fill_like("tm.0.bias", (1280,)))
    w2 = h16(torch.from_numpy(weights.fill_like("tm.2.weight", (1280, 1280))))
    b2 = torch.from_numpy(weights.fill_like("tm.2.bias", (1280,)))
    we = h16(torch.from_numpy(weights.fill_like("tm.e.weight", (640, 1280))))
    be = torch.from_numpy(weights.fill_like("tm.e.bias", (640,)))
    e16 = emb.float().cpu()
    r1 = h16(F.silu(F.linear(e16, w0, b0)))
    r2 = h16(F.linear(r1, w2, b2))
    r3 = F.linear(h16(F.silu(r2)), we, be)
    d = dev()
    o1 = ops.linear_small_m(emb, w0.half().to(d), b0.to(d), act_out=True)
    o2 = ops.linear_small_m(o1, w2.half().to(d), b2.to(d))
    o3 = ops.linear_small_m(o2, we.half().to(d), be.to(d), act_in=True)
    report("time_mlp.0", o1, r1)
    report("time_mlp.2", o2, r2, atol=2e-3)
    report("emb_layer", o3, r3, atol=2e-3)


def _conv_case(name, N, Cin, Cout, H, W, taps=9, stride=1, up=0, C2=0, bias=True, rowvec=False, resid=False,
               tile_n=0, wscale=1.0, tile_m=0, splits=0, asym=False, pipe=0):
    from leftrefill_amd import ops, packing
    d = dev()
    Ct = Cin + C2
    Hs, Ws = H, W
    if stride == 2:
        Hs, Ws = 2 * H, 2 * W
    if up:
        Hs, Ws = H // 2, W // 2
    x = h16(G.T(name + ".x", (N, Ct, Hs, Ws)))
    k = 3 if taps == 9 else 1
    w = h16(torch.from_numpy(weights.fill_like(name + ".w", (Cout, Ct, k, k))) * wscale)
    b = torch.from_numpy(weights.fill_like(name + ".b", (Cout,))) if bias else None
    xin = x
    if up:
        xin = F.interpolate(x, scale_factor=2, mode="nearest")
    if asym:     # VAE Downsample: F.pad (0,1,0,1) + padding 0 (model.py:83-86)
        ref = F.conv2d(F.pad(xin, (0, 1, 0, 1)), w, b, stride=stride, padding=0)
    else:
        ref = F.conv2d(xin, w, b, stride=stride, padding=1 if taps == 9 else 0)
    rv = rs = None
    if rowvec:
        rv = h16(G.T(name + ".rv", (N, Cout)))
        ref = ref + rv[:, :, None, None]
    if resid:
        rs = h16(G.T(name + ".rs", (N, Cout, H, W)))
        ref = ref + rs
    wp = packing.pack_conv(w, cin_pad=Ct).to(d)
    bp = packing.pack_bias(b).to(d) if bias else None
    x1 = to_tok(x[:, :Cin])
    x2 = to_tok(x[:, Cin:]) if C2 else None
    y = ops.gemm_conv(x1, wp, B=N, H=H, W=W, Hs=Hs, Ws=Ws, taps=taps, stride=stride, up=up, asym=asym, x2=x2, bias=bp,
                      rowvec=rv.half().to(d) if rowvec else None, resid=to_tok(rs) if resid else None, tile_n=tile_n,
                      tile_m=tile_m, splits=splits, pipe=pipe)
    y = y[:, :Cout]
    # fp32 accumulation over K = taps*Ct products of fp16 values: the error is one final fp16 rounding
    report(name, from_tok(y, N, H, W), ref)


@pytest.mark.parametrize("tile_n", [64, 128])
def test_gemm_linear(tile_n):
    _conv_case(f"lin{tile_n}", 1, 320, 640, 16, 24, taps=1, tile_n=tile_n)
    _conv_case(f"lin_odd{tile_n}", 1, 128, 128 if tile_n == 128 else 192, 7, 11, taps=1, tile_n=tile_n)  # M = 77 (tail)


def test_conv3x3_variants():
    _conv_case("c3_s1", 2, 320, 320, 12, 20)
    _conv_case("c3_s1_big", 2, 640, 1280, 8, 16, rowvec=True)
    _conv_case("c3_cat_res", 2, 320, 640, 8, 12, C2=640, rowvec=True, resid=True)
    _conv_case("c3_s2", 2, 320, 320, 6, 10, stride=2)
    _conv_case("c3_s2_asym", 2, 128, 128, 6, 10, stride=2, asym=True)
    _conv_case("c3_s2_asym64", 1, 64, 64, 5, 7, stride=2, asym=True, tile_n=64)
    _conv_case("c3_up", 1, 640, 640, 8, 12, up=1)
    _conv_case("c1_cat", 2, 640, 320, 8, 8, taps=1, C2=320)
    _conv_case("c3_in", 2, 64, 320, 16, 32)   # padded input conv (9 -> 64 channels handled by caller)
    _conv_case("c3_m_tail", 1, 128, 64, 5, 9)  # M = 45 < tile


@pytest.mark.parametrize("tile_n", [128, 160, 256, 320])
def test_conv_tile256(tile_n):
    """The 256-row, 8-wave, 3-stage counted-vmcnt kernel: every gather mode, tails in M and N, split-K."""
    k = dict(tile_m=256, tile_n=tile_n)
    co = 384 if tile_n in (128, 256) else 320
    _conv_case(f"t256_{tile_n}_c3", 2, 320, co, 16, 24, **k)                       # M = 768
    _conv_case(f"t256_{tile_n}_tail", 1, 128, co, 9, 13, rowvec=True, resid=True, **k)   # M = 117 (< one tile)
    _conv_case(f"t256_{tile_n}_cat", 2, 320, 640, 12, 20, C2=640, rowvec=True, resid=True, **k)
    _conv_case(f"t256_{tile_n}_s2", 2, 320, co, 10, 14, stride=2, **k)
    _conv_case(f"t256_{tile_n}_s2a", 2, 128, co, 10, 14, stride=2, asym=True, **k)
    _conv_case(f"t256_{tile_n}_up", 1, 640, 640, 16, 24, up=1, **k)
    _conv_case(f"t256_{tile_n}_lin", 1, 320, 960, 1, 700, taps=1, **k)              # short K (5 steps), M tail
    _conv_case(f"t256_{tile_n}_lin1", 1, 64, 320, 1, 300, taps=1, **k)             # single K-step
    _conv_case(f"t256_{tile_n}_lin2", 1, 128, 320, 1, 300, taps=1, **k)            # two K-steps
    _conv_case(f"t256_{tile_n}_splitk", 2, 1280, 640, 8, 16, splits=3, **k)
    _conv_case(f"t256_{tile_n}_c1cat", 2, 640, 320, 16, 16, taps=1, C2=320, **k)


@pytest.mark.parametrize("tile_n", [160, 320])
def test_conv_halo_tile(tile_n):
    """LR_PIPE_HALO (conv_halo.hip): the 3x3 stride-1 conv with the 18 x 18 input patch resident in LDS, 16 x 16 pixel tiles -- image
    borders on every side of a tile, several tiles per line / column / sample, the virtual channel concat, N tails, every epilogue
    operand; against F.conv2d in fp32 on the same fp16 operands (reference openaimodel.py:200-231)."""
    from leftrefill_amd import ops, packing
    k = dict(tile_m=256, tile_n=tile_n, pipe=8, splits=1)
    _conv_case(f"halo{tile_n}_one", 1, 64, 320, 16, 16, **k)                                  # one tile, one chunk: border on all four sides
    _conv_case(f"halo{tile_n}_c3", 2, 320, 320, 32, 48, rowvec=True, **k)                     # 2 x 3 tiles per sample
    _conv_case(f"halo{tile_n}_res", 3, 320, 640, 16, 32, resid=True, **k)                     # N = 640: 2 (4) column tiles
    _conv_case(f"halo{tile_n}_cat", 2, 320, 320, 32, 16, C2=640, rowvec=True, resid=True, **k)
    _conv_case(f"halo{tile_n}_ntail", 1, 128, 384, 16, 32, **k)                               # N = 384: ragged last column tile
    for sp in (2, 3, 7):                                                                      # split-K by whole chunks (20 chunks: 10 | 7,7,6 | 3,3,3,3,3,3,2)
        _conv_case(f"halo{tile_n}_splitk{sp}", 2, 1280, 640, 16, 32, rowvec=True, resid=True, **dict(k, splits=sp))
    _conv_case(f"halo{tile_n}_splitk_empty", 1, 128, 320, 16, 16, **dict(k, splits=3))        # 2 chunks over 3 slices: one slice has no work
    # 8-line images (the 8 x 16 level of the UNet): a tile = the 8 x 16 pixels of two consecutive samples, each with its own zero padding
    _conv_case(f"halo{tile_n}_h8", 4, 320, 320, 8, 16, rowvec=True, resid=True, **k)
    _conv_case(f"halo{tile_n}_h8_wide", 2, 128, 640, 8, 48, C2=192, **k)                      # three column tiles per pair of samples
    _conv_case(f"halo{tile_n}_h8_splitk", 8, 1280, 1280, 8, 16, resid=True, **dict(k, splits=4))
    # shapes the instance does not cover are refused, never run wrong
    d = dev()
    x = torch.zeros(2 * 24 * 16, 64, device=d, dtype=torch.float16)
    w = torch.zeros(320, 576, device=d, dtype=torch.float16)
    with pytest.raises(RuntimeError):
        ops.gemm_conv(x, w, B=2, H=24, W=16, taps=9, **k)                                     # H not a multiple of 16
    with pytest.raises(RuntimeError):
        ops.gemm_conv(x[:3 * 8 * 16], w, B=3, H=8, W=16, taps=9, **k)                         # 8-line images come in pairs
    with pytest.raises(RuntimeError):
        ops.gemm_conv(x[:2 * 8 * 8 * 4], w, B=2, H=8, W=8, Hs=16, Ws=16, taps=9, stride=2, **k)


@pytest.mark.parametrize("tile_n", [160, 320])
def test_conv_halo_matches_gather_kernel_and_its_statistics(tile_n):
    """The halo-tile conv against the gather kernel (gemm_conv_pipe_kernel) on the same call: same products, chunk-major instead of
    tap-major accumulation order -> equal up to the fp32 summation order (at most one fp16 ulp on a few outputs); with the fused
    skip_connection (lr_gemm_args.skip1: extra chunks with one tap); the GroupNorm partials (per-channel row blocks AND per-group
    chunks, numbered by 16 x 16 pixel tile) describe the stored tensor and feed lr_groupnorm_apply_n; reruns are bit-identical."""
    from leftrefill_amd import ops, packing
    d = dev()
    N, H, W = 2, 32, 32
    Ch, Cx1, Cx2, Cout = 320, 320, 640, 320
    name = f"halo_skip{tile_n}"
    hx = h16(G.T(name + ".h", (N, Ch, H, W)))
    x1 = h16(G.T(name + ".x1", (N, Cx1, H, W)))
    x2 = h16(G.T(name + ".x2", (N, Cx2, H, W)))
    w3 = h16(torch.from_numpy(weights.fill_like(name + ".w3", (Cout, Ch, 3, 3))))
    ws = h16(torch.from_numpy(weights.fill_like(name + ".ws", (Cout, Cx1 + Cx2, 1, 1))) * 2.0)
    b3 = torch.from_numpy(weights.fill_like(name + ".b3", (Cout,)))
    bs = torch.from_numpy(weights.fill_like(name + ".bs", (Cout,))) + 0.2
    rv = h16(G.T(name + ".rv", (N, Cout)))
    ref = F.conv2d(hx, w3, b3, padding=1) + F.conv2d(torch.cat([x1, x2], 1), ws, bs) + rv[:, :, None, None]
    wf = torch.cat([packing.pack_conv(w3), packing.pack_conv(ws)], dim=1).half().contiguous().to(d)
    bf = packing.pack_bias(b3 + bs).to(d)
    th, t1, t2 = to_tok(hx), to_tok(x1), to_tok(x2)
    kw = dict(B=N, H=H, W=W, taps=9, bias=bf, splits=1, rowvec=rv.half().to(d), tile_m=256, tile_n=tile_n)
    y, gs = ops.gemm_conv(th, wf, skip=(t1, t2), want_gn_stats=True, pipe=8, **kw)
    report(f"halo conv + fused skip {tile_n}", from_tok(y, N, H, W), ref, rtol=3e-3, atol=3e-3)
    assert torch.equal(y, ops.gemm_conv(th, wf, skip=(t1, t2), pipe=8, **kw)), "reruns must be bit-identical"
    # piece-major weights [K / 64][N][64] (lr_gemm_args.wt_pm): same products in the same order, on both kernels, incl. the extension
    assert torch.equal(y, ops.gemm_conv(th, packing.pack_pm(wf), wt_pm=True, skip=(t1, t2), pipe=8, **kw)), "piece-major weights change bits"
    yg_ = ops.gemm_conv(th, wf, skip=(t1, t2), **kw)
    assert torch.equal(yg_, ops.gemm_conv(th, packing.pack_pm(wf), wt_pm=True, skip=(t1, t2), **kw))
    dmax = (y.float() - yg_.float()).abs().max().item()
    neq = (y != yg_).float().mean().item()
    print(f"halo vs gather: max diff {dmax:.3e}, {100 * neq:.2f} % of elements differ")
    assert dmax <= 2 ** -9 * max(1.0, ref.abs().max().item()) and neq < 0.05
    assert gs is not None
    part, R, gp, chunks = gs
    # row blocks / chunks are numbered by pixel tile: tile (sample, ty, tx), wave row block = R / 16 consecutive lines of it
    yt = y.float().reshape(N, H // 16, 16, W // 16, 16, Cout).permute(0, 1, 3, 2, 4, 5).reshape(N * (H // 16) * (W // 16), 256, Cout)
    yb = yt.reshape(-1, R, Cout)
    assert torch.allclose(part[..., 0], yb.sum(1), rtol=1e-5, atol=5e-3)
    assert torch.allclose(part[..., 1], (yb * yb).sum(1), rtol=1e-5, atol=5e-3)
    assert gp is not None and chunks == H * W // 256
    ygp = yt.double().reshape(N, chunks, 256, 32, Cout // 32)
    assert torch.allclose(gp[..., 0].double(), ygp.sum((2, 4)), rtol=1e-5, atol=1e-2)
    assert torch.allclose(gp[..., 1].double(), (ygp * ygp).sum((2, 4)), rtol=1e-5, atol=1e-2)
    gam = 1.0 + 0.3 * G.T(name + ".g", (Cout,))
    bet = 0.2 * G.T(name + ".be", (Cout,))
    refn = F.silu(F.group_norm(from_tok(y, N, H, W), 32, gam, bet, 1e-5))
    report("halo gn(groups)", from_tok(ops.group_norm_groups(y, N, H * W, gam.to(d), bet.to(d), 1e-5, True, gp, chunks), N, H, W), refn)
    report("halo gn(finalize)", from_tok(ops.group_norm_fused(y, N, H * W, gam.to(d), bet.to(d), 1e-5, True, gs), N, H, W), refn)


def test_conv_tile128x160():
    k = dict(tile_m=128, tile_n=160)
    _conv_case("t128x160_c3", 2, 320, 320, 12, 20, rowvec=True, resid=True, **k)
    _conv_case("t128x160_tail", 1, 128, 480, 9, 13, **k)
    _conv_case("t128x160_lin", 1, 320, 960, 1, 300, taps=1, **k)
    _conv_case("t128x160_splitk", 2, 1280, 640, 8, 16, splits=3, **k)


def test_geglu_tile256():
    from leftrefill_amd import ops, packing
    d = dev()
    C, M = 320, 700
    x = h16(G.T("geglu2.x", (M, C)))
    w = h16(torch.from_numpy(weights.fill_like("geglu2.w", (8 * C, C))))
    b = torch.from_numpy(weights.fill_like("geglu2.b", (8 * C,)))
    u, gate = F.linear(x, w, b).chunk(2, dim=-1)
    ref = u * F.gelu(gate)
    wp, bp = packing.pack_geglu(w, b)
    for tn in (128, 256, 320):
        y = ops.gemm_conv(x.half().to(d), wp.to(d), B=1, H=1, W=M, taps=1, bias=bp.to(d), geglu=True, tile_m=256,
                          tile_n=tn)
        report(f"geglu tile256x{tn}", y, ref)


def test_conv_split_k():
    """Small-M / long-K shapes take the split-K path (fp32 partials + fixed-order reduce)."""
    from leftrefill_amd import ops
    _conv_case("c3_splitk_auto", 2, 1280, 1280, 8, 16, rowvec=True, resid=True)       # M=256, K=11520 -> auto split
    _conv_case("c3_splitk_cat", 1, 1280, 640, 8, 16, C2=1280)                          # K=23040
    d = dev()
    x = h16(G.T("sk.x", (256, 2560))).half().to(d)
    w = h16(torch.from_numpy(weights.fill_like("sk.w", (256, 2560)))).half().to(d)
    ys = [ops.gemm_conv(x, w, B=1, H=1, W=256, taps=1, splits=s_) for s_ in (1, 2, 5)]
    ref = F.linear(x.float().cpu(), w.float().cpu())
    for y in ys:
        report("splitk explicit", y, ref)
    assert torch.equal(ops.gemm_conv(x, w, B=1, H=1, W=256, taps=1, splits=5), ys[2]), "split-K must be deterministic"


@pytest.mark.parametrize("tile", [(256, 160), (256, 320), (128, 160, 4), (256, 160, 8), (256, 320, 8)], ids=lambda t_: "x".join(map(str, t_)))
def test_splitk_in_launch_reduce(tile, monkeypatch):
    """lr_gemm_args.splitk_mode = 1: the K-slice blocks of a tile reduce the partials inside the GEMM launch (agent-scope counter,
    write-through partials, every slice reduces its share of the rows in slice order) -- the 16-bit output is bit-identical to the
    separate fixed-order reduce launch, the GroupNorm statistics describe the stored tensor, repeated launches stay identical (the
    counters re-arm themselves), no spin ever times out; plans whose grid would not be resident at once fall back silently."""
    from leftrefill_amd import _lib, ops, packing
    need_dev_build()
    d = dev()
    N, H, W, Cin, Cout = 8, 8, 16, 1280, 640                  # M = 1024 rows (the 8 x 16 level), K = 11520
    name = "skf." + "x".join(map(str, tile))
    x = h16(G.T(name + ".x", (N, Cin, H, W)) * 0.5 + 0.1)
    w = h16(torch.from_numpy(weights.fill_like(name + ".w", (Cout, Cin, 3, 3))))
    b = torch.from_numpy(weights.fill_like(name + ".b", (Cout,))) + 0.3
    rs = h16(G.T(name + ".rs", (N, Cout, H, W)))
    rv = h16(G.T(name + ".rv", (N, Cout)))
    wp, bp = packing.pack_conv(w, cin_pad=Cin).to(d), packing.pack_bias(b).to(d)
    kw = dict(B=N, H=H, W=W, taps=9, bias=bp, resid=to_tok(rs), rowvec=rv.half().to(d), want_gn_stats=True, **tile_kw(tile))
    ref = F.conv2d(x, w, b, padding=1) + rs + rv[:, :, None, None]
    lib = _lib.load()
    for splits in (2, 4, 5, 8):
        monkeypatch.setattr(ops, "SPLITK_MODE", 0)
        y0, gs0 = ops.gemm_conv(to_tok(x), wp, splits=splits, **kw)
        monkeypatch.setattr(ops, "SPLITK_MODE", 1)
        ys = [ops.gemm_conv(to_tok(x), wp, splits=splits, **kw) for _ in range(6)]
        y1, gs1 = ys[0]
        report(f"in-launch split-K {tile} s{splits}", from_tok(y1, N, H, W), ref)
        assert torch.equal(y1, y0), "the in-launch reduce sums the slices in the same order as the reduce launch"
        assert all(torch.equal(y_, y1) and torch.equal(g_[0], gs1[0]) for y_, g_ in ys[1:]), "reruns (self-resetting counters)"
        part, R, gp, chunks = gs1
        assert R == 32
        yf = y1.float()
        if len(tile) > 2 and tile[2] == 8:      # halo tiles: a 32-row statistics block = two 16-pixel line segments of a 16 x 16 tile (pairs of samples here)
            yt = yf.reshape(N // 2, 16, W // 16, 16, Cout).permute(0, 2, 1, 3, 4).reshape(-1, 32, Cout)
        else:
            yt = yf.reshape(-1, 32, Cout)
        assert torch.allclose(part[..., 0], yt.sum(1), rtol=1e-5, atol=5e-3)
        assert torch.allclose(part[..., 1], (yt * yt).sum(1), rtol=1e-5, atol=5e-3)
        if gp is not None:
            tot = y1.double().reshape(N, H * W, 32, Cout // 32)
            assert torch.allclose(gp[..., 0].double().sum(1), tot.sum((1, 3)), rtol=1e-5, atol=2e-2)
            assert torch.allclose(gp[..., 1].double().sum(1), (tot * tot).sum((1, 3)), rtol=1e-5, atol=2e-2)
            gam = 1.0 + 0.3 * G.T(name + ".g", (Cout,))
            bet = 0.2 * G.T(name + ".be", (Cout,))
            out = ops.group_norm_groups(y1, N, H * W, gam.to(d), bet.to(d), 1e-5, True, gp, chunks)
            report(f"in-launch split-K gn(groups) {tile} s{splits}", from_tok(out, N, H, W),
                   F.silu(F.group_norm(from_tok(y1, N, H, W), 32, gam, bet, 1e-5)))
        assert lib.lr_gemm_splitk_timeouts() == 0
    # a grid that is not resident at once (tiles x splits > 256) takes the reduce launch: same bits, nothing to wait for
    xb = h16(G.T(name + ".xb", (256, 256, 8, 16)))
    wb = packing.pack_conv(h16(torch.from_numpy(weights.fill_like(name + ".wb", (320, 256, 3, 3)))), cin_pad=256).to(d)
    monkeypatch.setattr(ops, "SPLITK_MODE", 0)
    ya = ops.gemm_conv(to_tok(xb), wb, B=256, H=8, W=16, taps=9, splits=2, **tile_kw(tile))
    monkeypatch.setattr(ops, "SPLITK_MODE", 1)
    assert torch.equal(ops.gemm_conv(to_tok(xb), wb, B=256, H=8, W=16, taps=9, splits=2, **tile_kw(tile)), ya)
    assert lib.lr_gemm_splitk_timeouts() == 0


def test_conv_golden_cases(golden):
    """The reference-generated operator goldens (G3) for the conv family."""
    from leftrefill_amd import ops, packing
    d = dev()
    g = golden("ops")
    for name, kind, p in G.OP_CASES:
        if kind not in ("conv3x3", "conv1x1", "down", "up"):
            continue
        st = G.op_state(name, kind, p)
        x = G.op_inputs(name, kind, p)["x"]
        N, _, Hs, Ws = x.shape
        wkey = {"conv3x3": "weight", "conv1x1": "weight", "down": "op.weight", "up": "conv.weight"}[kind]
        w, b = st[wkey], st[wkey.replace("weight", "bias")]
        taps = 1 if kind == "conv1x1" else 9
        stride, up = (2, 0) if kind == "down" else ((1, 1) if kind == "up" else (1, 0))
        H, W = (Hs // 2, Ws // 2) if kind == "down" else ((Hs * 2, Ws * 2) if kind == "up" else (Hs, Ws))
        y = ops.gemm_conv(to_tok(x), packing.pack_conv(w).to(d), B=N, H=H, W=W, Hs=Hs, Ws=Ws, taps=taps, stride=stride,
                          up=up, bias=packing.pack_bias(b).to(d))
        # golden is pure fp32 (unrounded inputs/weights): add the input/weight rounding noise, ~sqrt(K)*2^-11*|x||w|
        report("golden " + name, from_tok(y, N, H, W), torch.from_numpy(g[name]), rtol=4e-3, atol=4e-3)


@pytest.mark.parametrize("tile,splits", [((256, 320), 1), ((256, 160), 1), ((256, 128), 1), ((256, 256), 1), ((128, 160, 4), 1), ((128, 128, 4), 1),
                                         ((256, 160), 3), ((256, 128), 4)], ids=lambda v: "x".join(map(str, v)) if isinstance(v, tuple) else f"s{v}")
def test_conv_with_fused_skip_connection(tile, splits):
    """lr_gemm_args.skip1: `skip_connection(x) + conv3x3(h)` of a width-changing ResBlock (reference openaimodel.py:253-259, 274) in ONE
    accumulation -- 3x3 part over [h] or a virtual concat [h1 | h2], then the 1x1 part over the virtual concat [x1 | x2] -- against
    F.conv2d + F.conv2d in fp32 on the same 16-bit operands, on every pipelined tile, with split-K, image borders and an M tail; the
    result also agrees with the two-launch path (separate skip GEMM + residual epilogue) to its extra fp16 rounding; the GroupNorm
    partials of the epilogue describe the stored tensor; tiles of the non-pipelined kernel are refused."""
    from leftrefill_amd import ops, packing
    d = dev()
    N, H, W = 3, 16, 24                      # M = 1152 = 4.5 x 256: a tail tile; H W = 384 rows per sample
    Ch, Cx1, Cx2, Cout = 320, 320, 640, 320
    name = f"skipf.{'x'.join(map(str, tile))}.{splits}"
    hx = h16(G.T(name + ".h", (N, Ch, H, W)))
    x1 = h16(G.T(name + ".x1", (N, Cx1, H, W)))
    x2 = h16(G.T(name + ".x2", (N, Cx2, H, W)))
    w3 = h16(torch.from_numpy(weights.fill_like(name + ".w3", (Cout, Ch, 3, 3))))
    ws = h16(torch.from_numpy(weights.fill_like(name + ".ws", (Cout, Cx1 + Cx2, 1, 1))) * 2.0)
    b3 = torch.from_numpy(weights.fill_like(name + ".b3", (Cout,)))
    bs = torch.from_numpy(weights.fill_like(name + ".bs", (Cout,))) + 0.2
    ref = F.conv2d(hx, w3, b3, padding=1) + F.conv2d(torch.cat([x1, x2], 1), ws, bs)
    wf = torch.cat([packing.pack_conv(w3), packing.pack_conv(ws)], dim=1).half().contiguous().to(d)
    bf = packing.pack_bias(b3 + bs).to(d)
    th, t1, t2 = to_tok(hx), to_tok(x1), to_tok(x2)
    kw = dict(B=N, H=H, W=W, taps=9, bias=bf, splits=splits, **tile_kw(tile))
    y, gs = ops.gemm_conv(th, wf, skip=(t1, t2), want_gn_stats=True, **kw)
    report(f"conv + fused skip {tile} s{splits}", from_tok(y, N, H, W), ref, rtol=3e-3, atol=3e-3)
    assert torch.equal(y, ops.gemm_conv(th, wf, skip=(t1, t2), **kw))
    if gs is not None:
        part, R, gp, chunks = gs
        yf = y.float()
        rows = torch.arange(yf.shape[0], device=d) // R
        sums = torch.zeros(part.shape[0], Cout, device=d).index_add_(0, rows, yf)
        assert torch.allclose(part[..., 0], sums, rtol=1e-5, atol=5e-3)
    # two launches: skip GEMM -> fp16 -> residual of the 3x3 conv
    r2 = ops.gemm_conv(t1, packing.pack_conv(ws).half().to(d), B=N, H=H, W=W, taps=1, x2=t2, bias=packing.pack_bias(bs).to(d))
    y2 = ops.gemm_conv(th, packing.pack_conv(w3).half().to(d), B=N, H=H, W=W, taps=9, bias=packing.pack_bias(b3).to(d), resid=r2)
    assert (y.float() - y2.float()).abs().max().item() <= 4e-3 * max(1.0, ref.abs().max().item())
    # the 3x3 part over a virtual concat as well (an output block whose conv input is a concat does not occur in the UNet, the kernel allows it)
    ha, hb = hx[:, :128].contiguous(), hx[:, 128:].contiguous()      # (per tap the K order is [x1 channels | x2 channels]: the same weights)
    assert torch.equal(ops.gemm_conv(to_tok(ha), wf, x2=to_tok(hb), skip=(t1, t2), **kw), y)
    # a single skip source
    y1 = ops.gemm_conv(th, torch.cat([packing.pack_conv(w3), packing.pack_conv(ws[:, :Cx1])], 1).half().contiguous().to(d), skip=(t1, None), **kw)
    report("conv + fused skip, one source", from_tok(y1, N, H, W), F.conv2d(hx, w3, b3, padding=1) + F.conv2d(x1, ws[:, :Cx1], bs), rtol=3e-3, atol=3e-3)
    # the 2-stage 128-row kernel gathers the extension too
    y64 = ops.gemm_conv(th, wf, skip=(t1, t2), B=N, H=H, W=W, taps=9, bias=bf, tile_m=128, tile_n=64, splits=1)
    report("conv + fused skip 128x64", from_tok(y64, N, H, W), ref, rtol=3e-3, atol=3e-3)
    # pointwise main part: out = W_a g + W_s x + b + resid (SpatialTransformer.proj_out composed with the last feed-forward Linear)
    M = N * H * W
    g = h16(G.T(name + ".g", (M, 1280)))
    xs = h16(G.T(name + ".xs", (M, 320)))
    rs = h16(G.T(name + ".rs", (M, 320)))
    wa = h16(torch.from_numpy(weights.fill_like(name + ".wa", (320, 1280))))
    wsx = h16(torch.from_numpy(weights.fill_like(name + ".wsx", (320, 320))))
    refp = g @ wa.t() + xs @ wsx.t() + b3 + rs
    yp = ops.gemm_conv(g.half().to(d), torch.cat([wa, wsx], 1).half().contiguous().to(d), B=1, H=1, W=M, taps=1, bias=packing.pack_bias(b3).to(d)[:320].contiguous(),
                       resid=rs.half().to(d), skip=(xs.half().to(d), None), splits=splits, **tile_kw(tile))
    report(f"pointwise + extension {tile} s{splits}", yp.float().cpu(), refp, rtol=3e-3, atol=3e-3)


# (tile_m, tile_n[, pipe]): every GEMM instance; pipe 4 = the 8-wave 4-stage 128-row kernel
ALL_TILES = [(128, 64), (128, 128), (128, 160), (256, 128), (256, 160), (256, 256), (256, 320), (128, 128, 4), (128, 160, 4)]


def tile_kw(t):
    return dict(tile_m=t[0], tile_n=t[1], pipe=t[2] if len(t) > 2 else 0)


@pytest.mark.parametrize("tile", ALL_TILES, ids=lambda t_: "x".join(map(str, t_)))
def test_gemm_row_stats_and_layernorm_fold(tile):
    """LayerNorm folded into the consumer GEMM (lr_gemm_args.ln_stats): the producer's epilogue writes per-row
    (sum, sumsq) partials of its fp16 output, the consumer normalises inside its own epilogue.  Checked against
    F.linear(F.layer_norm(x)) in fp32 on the same fp16-rounded x (attention.py:271-283 semantics), every tile."""
    from leftrefill_amd import ops, packing
    d = dev()
    for C, N2, M in ((320, 960, 700), (640, 640, 300), (1280, 320, 130)):
        tm, tn = tile[:2]
        name = f"lnf{C}_{tm}x{tn}"
        a = h16(G.T(name + ".a", (M, C)))
        w0 = h16(torch.from_numpy(weights.fill_like(name + ".w0", (C, C))))
        b0 = torch.from_numpy(weights.fill_like(name + ".b0", (C,)))
        r0 = h16(G.T(name + ".r0", (M, C)) * 3.0 + 0.7)          # non-zero mean rows
        x_ref = (F.linear(a, w0, b0) + r0).half()                 # what the producer stores
        x, st = ops.gemm_conv(a.half().to(d), w0.half().to(d), B=1, H=1, W=M, taps=1, bias=b0.to(d), resid=r0.half().to(d),
                              want_stats=True, **tile_kw(tile))
        report(name + " producer", x, x_ref.float())
        xs = x.float()
        s = st.sum(dim=1)
        assert torch.allclose(s[:, 0].cpu(), xs.sum(1).cpu(), rtol=1e-5, atol=1e-3), name
        assert torch.allclose(s[:, 1].cpu(), (xs * xs).sum(1).cpu(), rtol=1e-5, atol=1e-3), name
        # consumer: Linear(LayerNorm(x)) with non-trivial gamma / beta
        gam = 1.0 + 0.3 * G.T(name + ".g", (C,))
        bet = 0.2 * G.T(name + ".be", (C,))
        w1 = h16(torch.from_numpy(weights.fill_like(name + ".w1", (N2, C))))
        b1 = torch.from_numpy(weights.fill_like(name + ".b1", (N2,)))
        xc = x.float().cpu()
        ref = F.linear(F.layer_norm(xc, (C,), gam, bet, 1e-5), w1, b1)
        wf, bf, cs = packing.fold_layernorm(w1, b1, gam, bet)
        y = ops.gemm_conv(x, wf.to(d), B=1, H=1, W=M, taps=1, bias=bf.to(d), ln=(st, 1e-5, cs.to(d)), **tile_kw(tile))
        # two fp16 roundings differ from the reference pipeline (gamma folded into W; no rounded LayerNorm output)
        report(name + " consumer", y, ref, rtol=4e-3, atol=4e-3)


def test_layernorm_fold_large_mean_rows():
    """rows with |mean| >> std (outlier / massive-activation tokens).  The fold derives mean / rstd from
    (sum, sumsq) partials, combined in fp64 inside the consumer: the result must track the two-pass LayerNorm."""
    from leftrefill_amd import ops, packing
    d = dev()
    C, N2, M = 320, 320, 256
    x = G.T("lnbig.x", (M, C)) * 0.5
    x[::3] += 40.0                       # every third row: mean 40, std 0.5
    x[1::3] -= 25.0
    x = h16(x)
    xf = x.float()
    st = torch.stack([xf.sum(1), (xf * xf).sum(1)], 1).reshape(M, 1, 2).contiguous().to(d)
    gam = 1.0 + 0.3 * G.T("lnbig.g", (C,))
    bet = 0.2 * G.T("lnbig.be", (C,))
    w1 = h16(torch.from_numpy(weights.fill_like("lnbig.w1", (N2, C))))
    ref = F.linear(F.layer_norm(xf, (C,), gam, bet, 1e-5), w1)
    wf, bf, cs = packing.fold_layernorm(w1, None, gam, bet)
    y = ops.gemm_conv(x.half().to(d), wf.to(d), B=1, H=1, W=M, taps=1, bias=bf.to(d), ln=(st, 1e-5, cs.to(d)))
    # fp32 (sum, sumsq) carry ~1e-7 * mean^2 / var of relative error into the variance (6e-4 here): graceful, not a collapse
    report("layernorm fold, large-mean rows", y, ref, rtol=6e-3, atol=6e-3)


@pytest.mark.parametrize("tile", [(128, 64), (128, 128), (256, 128), (256, 256), (256, 320), (128, 128, 4)],
                         ids=lambda t_: "x".join(map(str, t_)))
def test_geglu_layernorm_fold(tile):
    from leftrefill_amd import ops, packing
    tm, tn = tile[:2]
    d = dev()
    C, M = 320, 520
    name = f"lng_{tm}x{tn}"
    x = h16(G.T(name + ".x", (M, C)) * 2.0 + 0.3)
    gam = 1.0 + 0.3 * G.T(name + ".g", (C,))
    bet = 0.2 * G.T(name + ".be", (C,))
    w = h16(torch.from_numpy(weights.fill_like(name + ".w", (8 * C, C))))
    b = torch.from_numpy(weights.fill_like(name + ".b", (8 * C,)))
    u, gate = F.linear(F.layer_norm(x, (C,), gam, bet, 1e-5), w, b).chunk(2, dim=-1)
    ref = u * F.gelu(gate)
    st = torch.stack([x.sum(1), (x * x).sum(1)], dim=1).reshape(M, 1, 2).contiguous().to(d)
    wf, bf, cs = packing.fold_layernorm(w, b, gam, bet)
    perm = packing.geglu_perm(4 * C)
    y = ops.gemm_conv(x.half().to(d), wf[perm].contiguous().to(d), B=1, H=1, W=M, taps=1, bias=bf[perm].contiguous().to(d),
                      geglu=True, ln=(st, 1e-5, cs[perm].contiguous().to(d)), **tile_kw(tile))
    report(name, y, ref, rtol=4e-3, atol=4e-3)


@pytest.mark.parametrize("tile", ALL_TILES, ids=lambda t_: "x".join(map(str, t_)))
def test_groupnorm_statistics_from_gemm_epilogue(tile):
    """GroupNorm whose statistics come out of the producing GEMMs' epilogues (lr_gemm_args.gn_stats_out +
    lr_groupnorm_finalize) instead of a pass over x: per-channel block sums match the stored tensor, and the normalised
    output matches F.group_norm on the virtual concat of two producers with different block sizes (openaimodel.py:781)."""
    from leftrefill_amd import ops, packing
    d = dev()
    N, H, W = 2, 8, 16                      # HW = 128 rows per sample (the 8 x 16 level)
    tm, tn = tile[:2]
    name = f"gnf_{tm}x{tn}"
    outs = []
    for k, (Cin, Cout, taps) in enumerate(((320, 320, 9), (128, 640, 1))):
        x = h16(G.T(f"{name}.x{k}", (N, Cin, H, W)) * 1.5 + 0.4)
        w = h16(torch.from_numpy(weights.fill_like(f"{name}.w{k}", (Cout, Cin, 3 if taps == 9 else 1, 3 if taps == 9 else 1))))
        b = torch.from_numpy(weights.fill_like(f"{name}.b{k}", (Cout,))) + 0.3
        kw = dict(splits=1, **tile_kw(tile)) if k == 0 else dict(tile_m=128, tile_n=64, splits=1)
        y, gs = ops.gemm_conv(to_tok(x), packing.pack_conv(w, cin_pad=Cin).to(d), B=N, H=H, W=W, taps=taps,
                              bias=packing.pack_bias(b).to(d), want_gn_stats=True, **kw)
        assert gs is not None
        part, R, gp, chunks = gs
        yf = y.float().reshape(N * H * W // R, R, Cout)
        assert torch.allclose(part[..., 0], yf.sum(1), rtol=1e-5, atol=2e-3), name
        assert torch.allclose(part[..., 1], (yf * yf).sum(1), rtol=1e-5, atol=2e-3), name
        if gp is not None:      # per-group sums of the tile's rows (lr_gemm_args.gn_group_out): chunk = row tile inside the sample
            yg = y.double().reshape(N, chunks, H * W // chunks, 32, Cout // 32)
            assert torch.allclose(gp[..., 0].double(), yg.sum((2, 4)), rtol=1e-5, atol=5e-3), name
            assert torch.allclose(gp[..., 1].double(), (yg * yg).sum((2, 4)), rtol=1e-5, atol=5e-3), name
        elif k == 0:
            assert tn % (Cout // 32) != 0 or (H * W) % tm != 0, f"{name}: no group sums although the tile covers whole groups"
        outs.append((y, gs))
    (y1, g1), (y2, g2) = outs
    C = y1.shape[1] + y2.shape[1]
    gam = 1.0 + 0.3 * G.T(name + ".g", (C,))
    bet = 0.2 * G.T(name + ".be", (C,))
    xcat = torch.cat([from_tok(y1, N, H, W), from_tok(y2, N, H, W)], 1)
    ref = F.silu(F.group_norm(xcat, 32, gam, bet, 1e-5))
    out = ops.group_norm_fused(y1, N, H * W, gam.to(d), bet.to(d), 1e-5, True, g1, y2, g2)
    report(name + " gn(concat)", from_tok(out, N, H, W), ref)
    ref1 = F.group_norm(from_tok(y1, N, H, W), 32, gam[:320], bet[:320], 1e-6)
    out1 = ops.group_norm_fused(y1, N, H * W, gam[:320].contiguous().to(d), bet[:320].contiguous().to(d), 1e-6, False, g1)
    report(name + " gn(single)", from_tok(out1, N, H, W), ref1)
    if g1[2] is not None:       # the same GroupNorm straight from the producer's per-group sums: no finalize launch
        out2 = ops.group_norm_groups(y1, N, H * W, gam[:320].contiguous().to(d), bet[:320].contiguous().to(d), 1e-6, False, g1[2], g1[3])
        report(name + " gn(groups)", from_tok(out2, N, H, W), ref1)
        assert (out2.float() - out1.float()).abs().max().item() <= 2e-3


@pytest.mark.parametrize("M,C", [(10240, 320), (9000, 640)])
def test_geglu_many_tiles_agree_bitwise(M, C):
    """GEGLU projections with more tiles than CUs (several tile waves per launch): every 256-row instance gives the bits of
    the 128 x 128 tile, with and without the LayerNorm fold, ragged M.  (Also the regression test of the persistent
    continuous-ring variant that was measured in round 2 and not kept.)"""
    from leftrefill_amd import ops, packing
    d = dev()
    x = h16(G.T(f"gps.x{C}", (M, C)) * 1.5 + 0.2)
    w = h16(torch.from_numpy(weights.fill_like(f"gps.w{C}", (8 * C, C))))
    b = torch.from_numpy(weights.fill_like(f"gps.b{C}", (8 * C,)))
    gam = 1.0 + 0.3 * G.T("gps.g", (C,))
    bet = 0.2 * G.T("gps.be", (C,))
    wp, bp = packing.pack_geglu(w, b)
    wf, bf, cs = packing.fold_layernorm(w, b, gam, bet)
    perm = packing.geglu_perm(4 * C)
    xd = x.half().to(d)
    st = torch.stack([x.sum(1), (x * x).sum(1)], dim=1).reshape(M, 1, 2).contiguous().to(d)
    ref = ops.gemm_conv(xd, wp.to(d), B=1, H=1, W=M, taps=1, bias=bp.to(d), geglu=True, tile_m=128, tile_n=128)
    ref_ln = ops.gemm_conv(xd, wf[perm].contiguous().to(d), B=1, H=1, W=M, taps=1, bias=bf[perm].contiguous().to(d), geglu=True,
                           ln=(st, 1e-5, cs[perm].contiguous().to(d)), tile_m=128, tile_n=128)
    for tn in (128, 256, 320):
        y = ops.gemm_conv(xd, wp.to(d), B=1, H=1, W=M, taps=1, bias=bp.to(d), geglu=True, tile_m=256, tile_n=tn)
        assert torch.equal(y, ref), f"256x{tn}"
        y = ops.gemm_conv(xd, wf[perm].contiguous().to(d), B=1, H=1, W=M, taps=1, bias=bf[perm].contiguous().to(d), geglu=True,
                          ln=(st, 1e-5, cs[perm].contiguous().to(d)), tile_m=256, tile_n=tn)
        assert torch.equal(y, ref_ln), f"256x{tn} ln"
    u, gate = F.linear(x, w, b).chunk(2, dim=-1)
    report(f"geglu many tiles {M}x{C}", ref[:2048], (u * F.gelu(gate))[:2048])


def test_groupnorm_statistics_from_splitk_reduce():
    """A split-K producer hands the GroupNorm statistics over from its reduce kernel (32-row blocks of the rounded output):
    block sums match the stored tensor, the output equals the unsplit GEMM's bit for bit, GroupNorm matches F.group_norm."""
    from leftrefill_amd import ops, packing
    d = dev()
    N, H, W, Cin, Cout = 2, 8, 16, 640, 320              # M = 256 rows, K = 5760
    x = h16(G.T("gns.x", (N, Cin, H, W)) * 1.2 + 0.2)
    w = h16(torch.from_numpy(weights.fill_like("gns.w", (Cout, Cin, 3, 3))))
    b = torch.from_numpy(weights.fill_like("gns.b", (Cout,))) + 0.3
    rs = h16(G.T("gns.rs", (N, Cout, H, W)))
    wp, bp = packing.pack_conv(w, cin_pad=Cin).to(d), packing.pack_bias(b).to(d)
    for splits in (2, 3, 5):
        y, gs = ops.gemm_conv(to_tok(x), wp, B=N, H=H, W=W, taps=9, bias=bp, resid=to_tok(rs), want_gn_stats=True, splits=splits)
        assert gs is not None and gs[1] == 32
        part, R, gp, chunks = gs
        yf = y.float().reshape(N * H * W // R, R, Cout)
        assert torch.allclose(part[..., 0], yf.sum(1), rtol=1e-5, atol=2e-3)
        assert torch.allclose(part[..., 1], (yf * yf).sum(1), rtol=1e-5, atol=2e-3)
        assert gp is not None and chunks == H * W // 32      # the reduce kernel's 32-row x 160-channel blocks cover whole groups of 10
        yg = y.double().reshape(N, chunks, 32, 32, Cout // 32)
        assert torch.allclose(gp[..., 0].double(), yg.sum((2, 4)), rtol=1e-5, atol=5e-3)
        assert torch.allclose(gp[..., 1].double(), (yg * yg).sum((2, 4)), rtol=1e-5, atol=5e-3)
        y1 = ops.gemm_conv(to_tok(x), wp, B=N, H=H, W=W, taps=9, bias=bp, resid=to_tok(rs), splits=splits)
        assert torch.equal(y, y1)
        report(f"splitk{splits} conv", from_tok(y, N, H, W), F.conv2d(x, w, b, padding=1) + rs)
        gam = 1.0 + 0.3 * G.T("gns.g", (Cout,))
        bet = 0.2 * G.T("gns.be", (Cout,))
        out = ops.group_norm_fused(y, N, H * W, gam.to(d), bet.to(d), 1e-5, True, gs)
        report(f"splitk{splits} gn", from_tok(out, N, H, W), F.silu(F.group_norm(from_tok(y, N, H, W), 32, gam, bet, 1e-5)))
        out = ops.group_norm_groups(y, N, H * W, gam.to(d), bet.to(d), 1e-5, True, gp, chunks)
        report(f"splitk{splits} gn(groups)", from_tok(out, N, H, W), F.silu(F.group_norm(from_tok(y, N, H, W), 32, gam, bet, 1e-5)))
    # ragged M and N (tails of the reduce kernel's 32-row x 256-channel blocks), rowvec, no statistics
    M, K, Nn = 300, 2560, 328
    a = h16(G.T("gns.a", (M, K)))
    w2 = h16(torch.from_numpy(weights.fill_like("gns.w2", (Nn, K))))
    rv = h16(G.T("gns.rv", (1, Nn)))
    y2 = ops.gemm_conv(a.half().to(d), w2.half().to(d), B=1, H=1, W=M, taps=1, rowvec=rv.half().to(d), splits=4)
    report("splitk ragged", y2, F.linear(a, w2) + rv)


@pytest.mark.parametrize("C,HW,tile", [(320, 2048, (256, 320)), (320, 512, (256, 160)), (640, 512, (256, 160)), (640, 256, (128, 160)),
                                       (1280, 512, (128, 160, 4)), (1280, 256, (256, 320)), (640, 512, (256, 128))],
                         ids=lambda v: "x".join(map(str, v)) if isinstance(v, tuple) else str(v))
def test_groupnorm_group_sums_at_unet_widths(C, HW, tile):
    """lr_gemm_args.gn_group_out at the UNet's widths (10 / 20 / 40 channels per group) for every tile family that produces GroupNorm
    inputs, several row tiles per sample: the per-group partials equal the sums over the stored tensor, and the one-launch GroupNorm
    (no finalize) matches F.group_norm of it.  A tile whose width is not a whole number of groups reports none (fallback path)."""
    from leftrefill_amd import ops
    d = dev()
    N = 3
    M = N * HW
    x = h16(G.T(f"gng.{C}.{HW}.x", (M, 320)) + 0.3)
    w = h16(torch.from_numpy(weights.fill_like(f"gng.{C}.w", (C, 320))) * 2.0)
    b = torch.from_numpy(weights.fill_like(f"gng.{C}.b", (C,))) + 0.5
    y, gs = ops.gemm_conv(x.half().to(d), w.half().to(d), B=N, H=1, W=HW, taps=1, bias=b.to(d), want_gn_stats=True, splits=1, **tile_kw(tile))
    part, R, gp, chunks = gs
    if tile[1] % (C // 32):
        assert gp is None
        return
    assert gp is not None and chunks == HW // tile[0]
    yg = y.double().reshape(N, chunks, HW // chunks, 32, C // 32)
    assert torch.allclose(gp[..., 0].double(), yg.sum((2, 4)), rtol=1e-5, atol=1e-2)
    assert torch.allclose(gp[..., 1].double(), (yg * yg).sum((2, 4)), rtol=1e-5, atol=1e-2)
    gam = 1.0 + 0.3 * G.T(f"gng.{C}.g", (C,))
    bet = 0.2 * G.T(f"gng.{C}.be", (C,))
    ref = F.silu(F.group_norm(y.float().cpu().reshape(N, HW, C).permute(0, 2, 1), 32, gam, bet, 1e-5)).permute(0, 2, 1).reshape(M, C)
    out = ops.group_norm_groups(y, N, HW, gam.to(d), bet.to(d), 1e-5, True, gp, chunks)
    report(f"gn(groups) C{C} HW{HW} {tile}", out, ref)
    assert torch.equal(out, ops.group_norm_groups(y, N, HW, gam.to(d), bet.to(d), 1e-5, True, gp, chunks))


@pytest.mark.parametrize("N,H,W,C,cout,chunks", [(2, 16, 32, 320, 4, 2), (1, 8, 16, 64, 3, 1), (3, 24, 48, 128, 1, 4), (2, 64, 128, 320, 4, 32)],
                         ids=lambda v: str(v))
def test_out_block_groupnorm_silu_conv_one_launch(N, H, W, C, cout, chunks):
    """lr_gn_conv_out_f16 = `self.out(h)` of the UNet (reference openaimodel.py:714-718, 812: GroupNorm32 -> SiLU -> 3x3 conv to
    out_channels) incl. the NCHW conversion, against F.conv2d(F.silu(F.group_norm(x))) in fp32 on the same 16-bit inputs (the
    normalised activation rounded to fp16 like the two-launch path stores it); image borders (zero padding of the ACTIVATED tensor),
    tiles at every edge, fewer than 4 output channels; the headline shape; and agreement with the two-launch HIP path."""
    from leftrefill_amd import ops, packing
    d = dev()
    HW = H * W
    x = h16(G.T(f"outb.{N}.{H}.{C}.x", (N * HW, C)) * 1.5 + 0.4)
    wc = torch.from_numpy(weights.fill_like(f"outb.{C}.{cout}.w", (cout, C, 3, 3))) * 3.0
    bc = torch.from_numpy(weights.fill_like(f"outb.{C}.{cout}.b", (cout,))) + 0.1
    gam = 1.0 + 0.3 * G.T(f"outb.{C}.g", (C,))
    bet = 0.2 * G.T(f"outb.{C}.be", (C,))
    wp = packing.pack_conv(wc, dtype=torch.float16).to(d)          # [64, 9 C], k = tap * C + channel
    bp = packing.pack_bias(bc).to(d)
    xd = x.half().to(d)
    xg = xd.double().reshape(N, chunks, HW // chunks, 32, C // 32)      # the producer's per-group partial sums
    gp = torch.stack([xg.sum((2, 4)), (xg * xg).sum((2, 4))], dim=-1).float().contiguous()
    out = ops.gn_conv_out(xd, N, H, W, gam.to(d), bet.to(d), 1e-5, gp, chunks, wp, bp, cout)
    assert out.shape == (N, cout, H, W) and out.dtype == torch.float16
    xn = F.silu(F.group_norm(x.reshape(N, H, W, C).permute(0, 3, 1, 2), 32, gam, bet, 1e-5))
    ref = F.conv2d(h16(xn).to(d), h16(wc).to(d), bc.to(d), padding=1).cpu()
    report(f"out block N{N} {H}x{W} C{C} -> {cout}", out, ref, atol=2e-3)
    assert torch.equal(out, ops.gn_conv_out(xd, N, H, W, gam.to(d), bet.to(d), 1e-5, gp, chunks, wp, bp, cout))
    # the two-launch path on the same operands: same normalised fp16 activation, same products, another summation order
    yn = ops.group_norm_groups(xd, N, HW, gam.to(d), bet.to(d), 1e-5, True, gp, chunks)
    y2 = ops.nhwc_to_nchw(ops.gemm_conv(yn, wp, B=N, H=H, W=W, taps=9, bias=bp), N, H, W, cout)
    assert (out.float() - y2.float()).abs().max().item() <= 2e-3 * max(1.0, y2.float().abs().max().item())
    with pytest.raises(RuntimeError):          # a width that is not a whole number of 16-pixel tiles: refused, never silently wrong
        ops._lib.check(ops._fn(ops._lib.load(), "lr_gn_conv_out_f16", xd.dtype)(xd.data_ptr(), N, H, W - 8, C, gp.data_ptr(), chunks,
                                                                                 gam.to(d).data_ptr(), bet.to(d).data_ptr(), 1e-5, wp.data_ptr(),
                                                                                 wp.stride(0), bp.data_ptr(), cout, out.data_ptr(), 0), "gn_conv_out")


@pytest.mark.parametrize("C,HW", [(320, 2048), (640, 512), (320, 256)])
def test_groupnorm_folded_into_pointwise_gemm(C, HW):
    """SpatialTransformer.norm folded into proj_in (lr_gn_fold_weights_f16 + lr_gemm_args.wt_bstride, attention.py:399-408): the GEMM on
    the RAW activation with per-sample weights equals proj_in(GroupNorm(x)) in fp32 on the same fp16 inputs; samples with very
    different statistics (a constant offset of 10 on one of them, |mean| >> std) keep the tolerance (the mean term is formed with the
    rounded weights)."""
    from leftrefill_amd import ops
    need_dev_build()
    d = dev()
    N = 3
    M = N * HW
    # (|mean| / std ~ 30 on sample 1; the statistics are fp32 (sum, sumsq) partials from the producer's epilogue, combined in fp64 --
    # like every fused GroupNorm here they resolve var = E[x^2] - mean^2 down to ~1e-6 mean^2, see test_groupnorm_large_mean_small_variance)
    scale = torch.tensor([1.0, 0.2, 4.0]).reshape(N, 1, 1)
    shift = torch.tensor([0.2, 10.0, -3.0]).reshape(N, 1, 1)
    x0 = h16(G.T(f"gnfold.{C}.x0", (M, 320)))
    w0 = h16(torch.from_numpy(weights.fill_like(f"gnfold.{C}.w0", (C, 320))) * 2.0)
    # producer: a linear layer whose output is the tensor to be normalised; its epilogue supplies the per-group sums
    tile = dict(tile_m=256, tile_n=320 if C == 320 else 160)                   # a tile that covers whole groups (10 / 20 channels)
    y = ops.gemm_conv(x0.half().to(d), w0.half().to(d), B=N, H=1, W=HW, taps=1, splits=1)
    y = (y.float().reshape(N, HW, C).cpu() * scale + shift).half()            # re-scaled per sample on the host ...
    yd = y.reshape(M, C).to(d)
    one = torch.eye(C).half().to(d)                                            # ... and passed through an identity GEMM for its sums
    y2, gs = ops.gemm_conv(yd, one, B=N, H=1, W=HW, taps=1, want_gn_stats=True, splits=1, **tile)
    assert torch.equal(y2, yd) and gs[2] is not None
    gam = 1.0 + 0.3 * G.T(f"gnfold.{C}.g", (C,))
    bet = 0.2 * G.T(f"gnfold.{C}.be", (C,))
    w = h16(torch.from_numpy(weights.fill_like(f"gnfold.{C}.w", (C, C))))
    b = torch.from_numpy(weights.fill_like(f"gnfold.{C}.b", (C,)))
    xn = F.group_norm(y.float().reshape(N, HW, C).permute(0, 2, 1), 32, gam, bet, 1e-6).permute(0, 2, 1).reshape(M, C)
    ref = F.linear(xn, w, b)
    wb, bb = ops.gn_fold_weights(gs[2], gs[3], N, HW, gam.to(d), bet.to(d), 1e-6, w.half().to(d), b.to(d))
    assert wb.shape == (N, C, C) and bb.shape == (N, C)
    out, st = ops.gemm_conv(yd, wb, B=N, H=1, W=HW, taps=1, bias=bb, per_sample=True, want_stats=True)
    # composite: the unfused path rounds the normalised tensor to fp16 before the GEMM, the fold rounds W a instead
    report(f"gn-fold C{C} HW{HW}", out, ref, rtol=3e-3, atol=4e-3)
    unf = ops.gemm_conv(ops.group_norm_groups(yd, N, HW, gam.to(d), bet.to(d), 1e-6, False, gs[2], gs[3]), w.half().to(d), B=1, H=1, W=M,
                        taps=1, bias=b.to(d))
    e_f, e_u = (out.float().cpu() - ref).norm() / ref.norm(), (unf.float().cpu() - ref).norm() / ref.norm()
    print(f"[gn-fold C{C}] rel-L2 folded {e_f:.3e} unfused {e_u:.3e}")
    assert e_f <= 2.0 * e_u + 1e-4
    of = out.float()
    assert torch.allclose(st[:, :, 0].sum(1), of.sum(1), rtol=1e-4, atol=2e-2)


@pytest.mark.parametrize("tile", [(128, 64), (128, 160), (256, 160), (256, 320), (128, 160, 4)], ids=lambda t_: "x".join(map(str, t_)))
def test_gemm_piece_major_weights_are_bit_identical(tile):
    """lr_gemm_args.wt_pm: the same weights stored [K / 64][N][64] (a K-step's 128-byte pieces consecutive) give the same bits as
    the [N][K] layout -- 3x3 conv with a virtual concat, a split-K call, a pointwise call with ragged N."""
    from leftrefill_amd import ops, packing
    d = dev()
    N, H, W = 2, 8, 16
    x1 = to_tok(h16(G.T("pm.x1", (N, 128, H, W))))
    x2 = to_tok(h16(G.T("pm.x2", (N, 64, H, W))))
    w = packing.pack_conv(h16(torch.from_numpy(weights.fill_like("pm.w", (320, 192, 3, 3)))), cin_pad=192).to(d)
    b = torch.from_numpy(weights.fill_like("pm.b", (320,))).to(d)
    for splits in (1, 3):
        y0 = ops.gemm_conv(x1, w, x2=x2, B=N, H=H, W=W, taps=9, bias=b, splits=splits, **tile_kw(tile))
        y1 = ops.gemm_conv(x1, packing.pack_pm(w), x2=x2, B=N, H=H, W=W, taps=9, bias=b, splits=splits, wt_pm=True, **tile_kw(tile))
        assert torch.equal(y0, y1), (tile, splits)
    report("pm conv", from_tok(y1, N, H, W), F.conv2d(torch.cat([from_tok(x1, N, H, W), from_tok(x2, N, H, W)], 1),
                                                       h16(torch.from_numpy(weights.fill_like("pm.w", (320, 192, 3, 3)))), b.cpu(), padding=1))
    a = h16(G.T("pm.a", (300, 640))).half().to(d)
    wl = h16(torch.from_numpy(weights.fill_like("pm.wl", (328, 640)))).half().to(d)
    assert torch.equal(ops.gemm_conv(a, wl, B=1, H=1, W=300, taps=1, splits=1, **tile_kw(tile)),
                       ops.gemm_conv(a, packing.pack_pm(wl), B=1, H=1, W=300, taps=1, splits=1, wt_pm=True, **tile_kw(tile)))


@pytest.mark.parametrize("N,H,W,Cout", [(2, 8, 16, 320), (1, 16, 32, 128), (3, 9, 7, 320)])
def test_conv_in_sixteen_channel_gather(N, H, W, Cout):
    """The UNet's input conv (openaimodel.py:546: 9 -> model_channels, 3x3 pad 1) through the 16-channel gather of lr_gemm_conv_f16
    (k = tap * 16 + c, four taps per K-step, K = 144 zero-padded to 192) instead of a 64-channel padded source: vs F.conv2d on the
    same fp16 inputs, borders and ragged row tails included, and vs the 64-padded path."""
    from leftrefill_amd import engine as E, ops
    d = dev()
    x = h16(G.T(f"c16.{H}.x", (N, 9, H, W)))
    conv = torch.nn.Conv2d(9, Cout, 3, padding=1)
    with torch.no_grad():
        conv.weight.copy_(h16(torch.from_numpy(weights.fill_like(f"c16.{Cout}.w", (Cout, 9, 3, 3)))))
        conv.bias.copy_(torch.from_numpy(weights.fill_like(f"c16.{Cout}.b", (Cout,))))
    ref = F.conv2d(x, conv.weight, conv.bias, padding=1)
    p16, p64 = E.PackedConv(conv, cin_pad=16), E.PackedConv(conv, cin_pad=64)
    assert p16.w.shape[1] == 192 and p64.w.shape[1] == 576
    a16 = E.Act(ops.nchw_to_nhwc(x.to(d), cpad=16), N, H, W)
    a64 = E.Act(ops.nchw_to_nhwc(x.to(d), cpad=64), N, H, W)
    y16 = E.conv(a16, E_to(p16, d), gn_stats=False)
    y64 = E.conv(a64, E_to(p64, d), gn_stats=False)
    report(f"conv_in c16 {N}x{H}x{W}->{Cout}", from_tok(y16.tok, N, H, W)[:, :Cout], ref)
    assert (y16.tok.float() - y64.tok.float()).abs().max().item() <= 2e-3
    assert torch.equal(y16.tok, E.conv(a16, E_to(p16, d)).tok)


def E_to(pc, d):
    pc.w = pc.w.to(d)
    if pc.b is not None:
        pc.b = pc.b.to(d)
    return pc


def test_tile_plan_is_static_and_tiles_agree_bitwise():
    """The (tile, split-K) plan is a pure function of the shape (in-tree table or the static heuristic -- never timing),
    and with the split factor pinned every tile gives bit-identical results (same K order per output element)."""
    from leftrefill_amd import ops
    d = dev()
    assert not ops.AUTOTUNE, "timing-based tile selection must be opt-in"
    assert ops.gemm_plan(1024, 1280, 11520, taps=9) == ops.gemm_plan(1024, 1280, 11520, taps=9)
    x = h16(G.T("tp.x", (300, 2560))).half().to(d)
    w = h16(torch.from_numpy(weights.fill_like("tp.w", (640, 2560)))).half().to(d)
    for splits in (1, 4):
        ys = [ops.gemm_conv(x, w, B=1, H=1, W=300, taps=1, splits=splits, **tile_kw(t_)) for t_ in ALL_TILES]
        for t_, y in zip(ALL_TILES[1:], ys[1:]):
            assert torch.equal(y, ys[0]), f"tile {t_} differs bitwise from {ALL_TILES[0]} at splits={splits}"


def test_geglu_epilogue():
    from leftrefill_amd import ops, packing
    d = dev()
    C, M = 320, 256
    x = h16(G.T("geglu.x", (M, C)))
    w = h16(torch.from_numpy(weights.fill_like("geglu.w", (8 * C, C))))
    b = torch.from_numpy(weights.fill_like("geglu.b", (8 * C,)))
    p = F.linear(x, w, b)
    u, gate = p.chunk(2, dim=-1)
    ref = u * F.gelu(gate)
    wp, bp = packing.pack_geglu(w, b)
    y = ops.gemm_conv(x.half().to(d), wp.to(d), B=1, H=1, W=M, taps=1, bias=bp.to(d), geglu=True)
    assert y.shape == (M, 4 * C)
    report("geglu", y, ref)


@pytest.mark.parametrize("B,heads,Nq,Nkv", [(2, 5, 128, 128), (1, 10, 512, 512), (2, 10, 64, 77), (1, 2, 200, 333),
                                            (1, 5, 2048, 2048)])
def test_attention(B, heads, Nq, Nkv):
    from leftrefill_amd import ops
    d = dev()
    C = heads * 64
    q = h16(G.T(f"att.{Nq}.{Nkv}.q", (B, Nq, C)))
    k = h16(G.T(f"att.{Nq}.{Nkv}.k", (B, Nkv, C)))
    v = h16(G.T(f"att.{Nq}.{Nkv}.v", (B, Nkv, C)))
    ref = unet_ref.attention(q, k, v, heads, unet_ref._Mode("fp32"))
    # fused-projection style strided inputs: q|k|v side by side when shapes allow
    if Nq == Nkv:
        qkv = torch.cat([q, k, v], dim=-1).reshape(B * Nq, 3 * C).half().to(d)
        o = ops.attention(qkv[:, :C], qkv[:, C:2 * C], qkv[:, 2 * C:], B, heads, Nq, Nkv, 64 ** -0.5)
    else:
        o = ops.attention(q.reshape(B * Nq, C).half().to(d), k.reshape(B * Nkv, C).half().to(d),
                          v.reshape(B * Nkv, C).half().to(d), B, heads, Nq, Nkv, 64 ** -0.5)
    # P is rounded to fp16 before the PV product (as in the xformers/flash kernels): error <= 2^-11 * max|v|
    report(f"attention B{B} h{heads} {Nq}x{Nkv}", o.reshape(B, Nq, C), ref, atol=2e-3)


@pytest.mark.parametrize("B,heads,Nq,Nkv", [(2, 2, 256, 256), (1, 3, 300, 200), (2, 1, 64, 77), (1, 2, 1024, 1024),
                                            (1, 1, 130, 1100), (1, 1, 256, 192), (1, 2, 70, 128), (1, 1, 1000, 4096), (2, 3, 333, 320)])
def test_attention_pretransposed_v(B, heads, Nq, Nkv):
    """The three ways V reaches the PV product -- natural V gathered by the LDS transpose read (ds_read_b64_tr_b16, the default),
    lr_transpose_v_f16 + lr_attention_vt_f16 (V^T streamed by LDS-DMA), natural V transposed in registers -- give bit-identical
    results (the MFMA operands are the same values in the same k order), incl. key tails and strided operands."""
    from leftrefill_amd import ops
    d = dev()
    C = heads * 64
    q = h16(G.T(f"attvt.{Nq}.{Nkv}.q", (B, Nq, C))).reshape(B * Nq, C).half().to(d)
    kv = torch.cat([h16(G.T(f"attvt.{Nq}.{Nkv}.k", (B, Nkv, C))), h16(G.T(f"attvt.{Nq}.{Nkv}.v", (B, Nkv, C)))], -1)
    kv = kv.reshape(B * Nkv, 2 * C).half().to(d)
    k, v = kv[:, :C], kv[:, C:]                       # strided column slices like the fused projections
    vt = ops.transpose_v(v, B, heads, Nkv)
    ld = vt.shape[2]
    assert ld % 64 == 0 and ld >= Nkv
    # layout check: within each 16-key group the order is [0-3, 8-11, 4-7, 12-15]; tail keys are zero
    perm = torch.tensor([0, 1, 2, 3, 8, 9, 10, 11, 4, 5, 6, 7, 12, 13, 14, 15])
    vpad = torch.zeros(B, ld, C, dtype=torch.float16, device=d)
    vpad[:, :Nkv] = v.reshape(B, Nkv, C)
    idx = (torch.arange(ld).reshape(-1, 16)[:, perm]).reshape(-1).to(d)
    assert torch.equal(vt, vpad[:, idx].permute(0, 2, 1).contiguous())
    outs = {}
    for mode in ("tr", "vt", "reg"):
        with v_path(mode):
            outs[mode] = ops.attention(q, k, v, B, heads, Nq, Nkv, 64 ** -0.5)
    assert torch.equal(outs["tr"], outs["vt"]) and torch.equal(outs["tr"], outs["reg"])
    assert torch.equal(ops.attention(q, k, v, B, heads, Nq, Nkv, 64 ** -0.5, vt=vt), outs["tr"])
    # 128- and 256-query blocks (LR_ATTN_NQB; the library picks by grid size) run the same arithmetic per query
    from leftrefill_amd import _lib
    if _lib.dev_variants():      # (forcing the block size is a developer knob)
        try:
            for nqb in (1, 2):
                _lib.dev_set("LR_ATTN_NQB", nqb)
                assert torch.equal(ops.attention(q, k, v, B, heads, Nq, Nkv, 64 ** -0.5), outs["tr"]), nqb
        finally:
            _lib.dev_set("LR_ATTN_NQB", None)


def test_attention_online_softmax_rescale():
    """Force the running max to jump late in the sequence (guide rule 26): one key matches one query strongly."""
    from leftrefill_amd import ops
    d = dev()
    B, heads, N = 1, 1, 512
    q = h16(G.T("attr.q", (B, N, 64)))
    k = h16(G.T("attr.k", (B, N, 64)))
    v = h16(G.T("attr.v", (B, N, 64)))
    k[0, 450] = q[0, 7] * 6.0      # spike in the last tile for query 7
    k[0, 70] = q[0, 300] * 4.0     # and in tile 1 for query 300
    ref = unet_ref.attention(q, k, v, heads, unet_ref._Mode("fp32"))
    o = ops.attention(q.reshape(N, 64).half().to(d), k.reshape(N, 64).half().to(d), v.reshape(N, 64).half().to(d),
                      B, heads, N, N, 64 ** -0.5)
    report("attention spike", o.reshape(B, N, 64), ref, atol=2e-3)


@pytest.mark.parametrize("vt", ["tr", "vt", "reg"])
def test_attention_logit_jumps_of_every_size(vt):
    """The inference kernels fold the scale and the running max into the QK^T accumulators (the first tile anchors the max, later tiles
    move it only when a shifted logit exceeds 2^3 in the exp2 domain): logits ~20 / ~70 / > 127 octaves above the running max in the
    first, a middle and the last tile, against the fp32 oracle (guide rule 26), on every V path."""
    from leftrefill_amd import ops
    d = dev()
    B, heads, N = 1, 2, 768
    C = heads * 64
    q = h16(G.T("attj.q", (B, N, C)))
    k = h16(G.T("attj.k", (B, N, C)))
    v = h16(G.T("attj.v", (B, N, C)))
    # head 0: moderate and large jumps (repair path); head 1: an overflowing one (robust rerun), each in a different tile
    k[0, 70, :64] = q[0, 300, :64] * 2.0       # ~ +20 octaves in tile 1
    k[0, 400, :64] = q[0, 40, :64] * 6.0       # ~ +70 octaves in a middle tile
    k[0, 760, :64] = q[0, 7, :64] * 5.0        # last tile
    k[0, 130, 64:] = q[0, 500, 64:] * 14.0     # > 127 octaves: fp32 overflow of P
    k[0, 5, 64:] = q[0, 100, 64:] * 3.0        # first tile (covered by the anchor)
    ref = unet_ref.attention(q, k, v, heads, unet_ref._Mode("fp32"))
    with v_path(vt):
        o = ops.attention(q.reshape(N, C).half().to(d), k.reshape(N, C).half().to(d), v.reshape(N, C).half().to(d), B, heads, N, N, 64 ** -0.5)
        o2 = ops.attention(q.reshape(N, C).half().to(d), k.reshape(N, C).half().to(d), v.reshape(N, C).half().to(d), B, heads, N, N, 64 ** -0.5)
    assert torch.equal(o, o2)
    # rows that jumped are dominated by one key (weight ~1): P near 1 is rounded to fp16, a few times the plain error
    report(f"attention jumps vt={vt}", o.reshape(B, N, C), ref, atol=4e-3)


@pytest.mark.parametrize("vmode", ["tr", "vt"])
def test_attention_vt_rescale_and_hot_shapes(vmode):
    """The long-sequence kernels (the self-attention path of the UNet: natural V through the LDS transpose read, and the
    pre-transposed-V kernel) against the CPU oracle DIRECTLY: (a) forced running-max jumps in the first, a middle and the last tile
    (guide rule 26), (b) the level-0 shape of configs[1] (8192 x 8192, one head) and the multi-view sequence of configs[3] (20480 keys)."""
    from leftrefill_amd import ops
    d = dev()
    with v_path(vmode):
        B, heads, N = 1, 1, 512
        q = h16(G.T("attp.q", (B, N, 64)))
        k = h16(G.T("attp.k", (B, N, 64)))
        v = h16(G.T("attp.v", (B, N, 64)))
        k[0, 450] = q[0, 7] * 6.0      # last tile, query block A of wave 0
        k[0, 70] = q[0, 300] * 4.0     # tile 1
        k[0, 200] = q[0, 40] * 5.0     # middle tile, query block B of wave 0
        k[0, 3] = q[0, 100] * 5.0      # first tile
        ref = unet_ref.attention(q, k, v, heads, unet_ref._Mode("fp32"))
        o = ops.attention(q.reshape(N, 64).half().to(d), k.reshape(N, 64).half().to(d), v.reshape(N, 64).half().to(d),
                          B, heads, N, N, 64 ** -0.5)
        # rows whose max jumped carry P up to 2^8 in fp16 until the deferred rescale (threshold 2^8): ~3x the plain error
        report("attention vt spike", o.reshape(B, N, 64), ref, atol=4e-3)
        for name, Nq, Nkv in (("8192x8192", 8192, 8192), ("2048x20480", 2048, 20480)):
            q = h16(G.T(f"atth.{name}.q", (1, Nq, 64)))
            k = h16(G.T(f"atth.{name}.k", (1, Nkv, 64)))
            v = h16(G.T(f"atth.{name}.v", (1, Nkv, 64)))
            ref = torch.softmax((q[0] @ k[0].t()) * 64 ** -0.5, dim=-1) @ v[0]        # fp32, attention.py:173-195
            o = ops.attention(q.reshape(Nq, 64).half().to(d), k.reshape(Nkv, 64).half().to(d),
                              v.reshape(Nkv, 64).half().to(d), 1, 1, Nq, Nkv, 64 ** -0.5)
            # averaging ~1e4 values: outputs are O(1e-2); P is rounded to fp16 before the second product
            report("attention vt " + name, o, ref, rtol=2e-3, atol=2e-4)


@pytest.mark.parametrize("B,heads,Nq,Nkv", [(1, 1, 512, 256), (2, 3, 1000, 1024), (1, 2, 700, 320), (1, 1, 2048, 2048), (1, 1, 130, 4096)])
def test_attention_pingpong_kernel_matches_reference_kernel(B, heads, Nq, Nkv):
    """attention_pp_kernel (8 waves, the two waves of a SIMD held in complementary matrix / softmax segments) runs the same
    arithmetic per wave as attention_kernel: bit-identical outputs for 512- and 256-query blocks, query tails, every ring
    slot phase (T = 4, 5, 16, 32, 64 key tiles), with forced running-max jumps (guide rule 26) in the first, a middle and
    the last key tile."""
    from leftrefill_amd import _lib, ops
    need_dev_build()
    d = dev()
    C = heads * 64
    q = h16(G.T(f"attpp.{Nq}.{Nkv}.q", (B, Nq, C)))
    k = h16(G.T(f"attpp.{Nq}.{Nkv}.k", (B, Nkv, C)))
    v = h16(G.T(f"attpp.{Nq}.{Nkv}.v", (B, Nkv, C)))
    k[0, 3, :64] = q[0, 100, :64] * 5.0
    k[0, Nkv // 2 + 5, :64] = q[0, 40, :64] * 5.0
    k[0, Nkv - 2, :64] = q[0, 7, :64] * 6.0
    qd, kd, vd = (t_.reshape(-1, C).half().to(d) for t_ in (q, k, v))
    vt = ops.transpose_v(vd, B, heads, Nkv)
    outs = {}
    try:
        for mode in ("0", "2", "3", "1"):
            _lib.dev_set("LR_ATTN_PP", int(mode))
            outs[mode] = ops.attention(qd, kd, vd, B, heads, Nq, Nkv, 64 ** -0.5, vt=vt)
            assert torch.equal(outs[mode], ops.attention(qd, kd, vd, B, heads, Nq, Nkv, 64 ** -0.5, vt=vt)), f"mode {mode}: rerun differs"
    finally:
        _lib.dev_set("LR_ATTN_PP", None)
    for mode in ("2", "3", "1"):
        assert torch.equal(outs[mode], outs["0"]), f"LR_ATTN_PP={mode} differs from attention_kernel"
    ref = unet_ref.attention(q, k, v, heads, unet_ref._Mode("fp32"))
    # rows whose max jumped carry P up to 2^8 in fp16 until the deferred rescale: a few times the plain error on those rows
    report(f"attention pp B{B} h{heads} {Nq}x{Nkv}", outs["1"].reshape(B, Nq, C), ref, atol=8e-3)


def test_row_copy_jobs():
    """lr_row_copy: several gather / scatter jobs with index tables, byte offsets and different row sizes in one launch."""
    from leftrefill_amd import ops
    d = dev()
    g = torch.Generator().manual_seed(5)
    src = torch.randint(0, 255, (37, 104), dtype=torch.uint8, generator=g).to(d)          # 104-byte rows: 64 "x" bytes + 40 "stats" bytes
    si = torch.randperm(37, generator=g)[:20].to(torch.int32).to(d)
    di = torch.randperm(25, generator=g)[:20].to(torch.int32).to(d)
    a = torch.zeros(20, 32, dtype=torch.float16, device=d)
    b_ = torch.zeros(25, 10, dtype=torch.float32, device=d)
    c = torch.zeros(37, 104, dtype=torch.uint8, device=d)
    ops.row_copy([dict(src=src, dst=a, row_bytes=64, n_rows=20, src_idx=si),
                  dict(src=src, src_off=64, dst=b_, row_bytes=40, n_rows=20, src_idx=si, dst_idx=di),
                  dict(src=src, dst=c, row_bytes=104, n_rows=37)])
    assert torch.equal(a.view(torch.uint8), src[si.long(), :64])
    want = torch.zeros(25, 40, dtype=torch.uint8, device=d)
    want[di.long()] = src[si.long(), 64:]
    assert torch.equal(b_.view(torch.uint8), want) and torch.equal(c, src)
    with pytest.raises(RuntimeError):
        ops.row_copy([dict(src=src, dst=a, row_bytes=60, n_rows=20)])                     # not a multiple of 8 bytes


def test_mv_gather_scatter():
    from leftrefill_amd import ops
    b, V, s, C = 2, 5, 4, 64
    v = V - 1
    x = h16(G.T("mv.x", (b * v, 2 * s * s, C)))
    seq_ref, info = unet_ref.mv_gather(x, V, True, False)
    seq = ops.mv_gather(x.reshape(-1, C).half().to(dev()), b, v, s)
    assert torch.equal(seq.float().cpu().reshape(seq_ref.shape), seq_ref)
    back_ref = unet_ref.mv_scatter(seq_ref, V, True, False, info)
    back = ops.mv_scatter(seq, b, v, s)
    assert torch.equal(back.float().cpu().reshape(back_ref.shape), back_ref)


@pytest.mark.parametrize("case,S,eta,index", G.STEP_CASES, ids=[c[0] for c in G.STEP_CASES])
def test_ddim_step_golden(golden, case, S, eta, index):
    from leftrefill_amd import ops
    g = golden("sampler")
    d = dev()
    B, h, w = 2, 8, 16
    x = G.T(case + ".x", (B, 4, h, w))
    e = G.T(case + ".e", (2 * B, 4, h, w))
    noise = G.T(case + ".noise", (B, 4, h, w))
    tabs = ddim_ref.ddim_tables(S, eta)
    xp, p0 = ops.ddim_cfg_step(x.to(d), e.to(d), noise.to(d), G.CFG_SCALE, tabs["alphas"][index],
                               tabs["alphas_prev"][index], tabs["sigmas"][index], tabs["sqrt_one_minus_alphas"][index])
    np.testing.assert_allclose(xp.cpu().numpy(), g[case + ".x_prev"], rtol=2e-6, atol=2e-6)
    np.testing.assert_allclose(p0.cpu().numpy(), g[case + ".pred_x0"], rtol=2e-6, atol=2e-6)
    # fp16 eps path (what the UNet emits): same formula on fp16-rounded eps with the fp16 CFG combine
    e16 = e.half()
    eu, ec = e16.chunk(2)
    e_t = (eu + (G.CFG_SCALE * (ec - eu))).float()  # fp16 arithmetic as in the reference under autocast
    xr, pr = ddim_ref.cfg_ddim_update(x, e_t, e_t, 1.0, tabs["alphas"][index], tabs["alphas_prev"][index],
                                      tabs["sigmas"][index], tabs["sqrt_one_minus_alphas"][index], noise)
    xp16, p016 = ops.ddim_cfg_step(x.to(d), e16.to(d), noise.to(d), G.CFG_SCALE, tabs["alphas"][index],
                                   tabs["alphas_prev"][index], tabs["sigmas"][index],
                                   tabs["sqrt_one_minus_alphas"][index])
    np.testing.assert_allclose(xp16.cpu().numpy(), xr.numpy(), rtol=1e-5, atol=1e-5)
    np.testing.assert_allclose(p016.cpu().numpy(), pr.numpy(), rtol=1e-5, atol=1e-5)


def test_argument_errors_are_reported_not_launched():
    """Error behaviour of the C ABI (include/leftrefill_hip.h): negative codes for bad arguments / alignment / unsupported
    shapes -- surfaced as RuntimeError by the Python binding -- and no launch happens (the output stays untouched)."""
    import ctypes
    from leftrefill_amd import _lib, ops
    lib = _lib.load()
    d = dev()
    st = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    x = torch.zeros(64, 96, device=d, dtype=torch.float16)          # 96 channels: not a multiple of 64
    w = torch.zeros(64, 96, device=d, dtype=torch.float16)
    with pytest.raises(RuntimeError, match="gemm_conv"):
        ops.gemm_conv(x, w, B=1, H=1, W=64, taps=1)
    a = _lib.GemmArgs()
    assert lib.lr_gemm_conv_f16(a, st) == -1                          # null pointers -> LR_E_ARG
    x64 = torch.zeros(64, 64, device=d, dtype=torch.float16)
    out = torch.full((64, 64), 7.0, device=d, dtype=torch.float16)
    a.p1, a.C1, a.B, a.H, a.W, a.Hs, a.Ws, a.taps, a.stride = x64.data_ptr(), 64, 1, 1, 64, 1, 64, 4, 1   # taps = 4
    a.wt, a.N, a.out, a.ld_out = x64.data_ptr(), 64, out.data_ptr(), 64
    assert lib.lr_gemm_conv_f16(a, st) == -3                          # LR_E_UNSUPPORTED
    a.taps, a.ld_out = 1, 60
    assert lib.lr_gemm_conv_f16(a, st) == -2                          # LR_E_ALIGN (ld_out % 8)
    a.ld_out, a.geglu = 64, 5
    assert lib.lr_gemm_conv_f16(a, st) == -1
    torch.cuda.synchronize()
    assert torch.all(out == 7.0)
    q = torch.zeros(128, 64, device=d, dtype=torch.float16)
    assert lib.lr_attention_f16(q.data_ptr(), 60, q.data_ptr(), 64, q.data_ptr(), 64, out.data_ptr(), 64, 1, 1, 128, 128,
                                ctypes.c_float(0.125), st) == -2       # ldq % 8
    assert lib.lr_layernorm(q.data_ptr(), None, None, ctypes.c_float(1e-5), q.data_ptr(), 128, 64, st) == -1
    assert lib.lr_groupnorm_stats(q.data_ptr(), 48, None, 0, 1, 128, q.data_ptr(), st) == -2     # C % 32
    assert lib.lr_softmax_rows_f16(q.data_ptr(), q.data_ptr(), 4, 20000, ctypes.c_float(1.0), st) == -3


def test_c_abi_from_plain_cpp_without_torch(tmp_path):
    """The boundary is a C ABI: a stand-alone C++ host program (no Python, no torch types) links the shared library, owns
    its buffers and stream, and gets correct results."""
    import shutil
    import subprocess
    from leftrefill_amd import build as b
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    exe = str(tmp_path / "cabi_smoke")
    subprocess.run([hipcc, "--offload-arch=gfx950", "-O2", "-I", os.path.join(b.HERE, "..", "include"),
                    os.path.join(b.HERE, "..", "tests", "cabi", "cabi_smoke.cpp"), "-L", b.LIBDIR, "-lleftrefill_hip",
                    "-Wl,-rpath," + b.LIBDIR, "-o", exe], check=True, capture_output=True, timeout=600)
    p = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    print(p.stdout.strip())
    assert p.returncode == 0, p.stdout + p.stderr


def test_gemm_conv_randomised_shapes():
    """60 random problems (seeded): odd spatial sizes, every gather mode, concat sources, ragged N, random tile / split-K
    requests, random epilogue combinations -- each against F.conv2d on the fp16-rounded operands."""
    import random
    from leftrefill_amd import ops, packing
    rng = random.Random(1234)
    d = dev()
    tiles = [(0, 0, 0), (128, 64, 0), (128, 128, 0), (128, 160, 0), (256, 128, 0), (256, 160, 0), (256, 256, 0), (256, 320, 0),
             (128, 128, 4), (128, 160, 4)]
    n_checked = 0
    for case in range(60):
        taps = rng.choice([1, 9, 9])
        mode = rng.choice(["s1", "s1", "s2", "up", "asym"]) if taps == 9 else "s1"
        C1 = rng.choice([64, 128, 192, 320])
        C2 = rng.choice([0, 0, 64, 128])
        N = rng.choice([64, 72, 128, 200, 320, 384])
        B = rng.randint(1, 3)
        H, W = rng.randint(1, 12), rng.randint(1, 14)
        Hs, Ws, stride, up, asym = H, W, 1, 0, False
        if mode in ("s2", "asym"):
            Hs, Ws, stride, asym = 2 * H, 2 * W, 2, mode == "asym"
        elif mode == "up":
            H, W = 2 * rng.randint(1, 6), 2 * rng.randint(1, 7)
            Hs, Ws, up = H // 2, W // 2, 1
        tm, tn, stg = rng.choice(tiles)
        splits = rng.choice([0, 0, 1, 2, 3])
        use_bias, use_rv, use_res = rng.random() < 0.8, rng.random() < 0.3, rng.random() < 0.5
        name = f"fz{case}"
        Ct = C1 + C2
        k = 3 if taps == 9 else 1
        x = h16(G.T(name + ".x", (B, Ct, Hs, Ws)))
        w = h16(torch.from_numpy(weights.fill_like(name + ".w", (N, Ct, k, k))))
        b = torch.from_numpy(weights.fill_like(name + ".b", (N,))) if use_bias else None
        xin = F.interpolate(x, scale_factor=2, mode="nearest") if up else x
        if asym:
            ref = F.conv2d(F.pad(xin, (0, 1, 0, 1)), w, b, stride=2, padding=0)
        else:
            ref = F.conv2d(xin, w, b, stride=stride, padding=1 if taps == 9 else 0)
        rv = rs = None
        if use_rv:
            rv = h16(G.T(name + ".rv", (B, N)))
            ref = ref + rv[:, :, None, None]
        if use_res:
            rs = h16(G.T(name + ".rs", (B, N, H, W)))
            ref = ref + rs
        wp = packing.pack_conv(w, cin_pad=Ct, cout_pad=N).to(d)
        try:
            y = ops.gemm_conv(to_tok(x[:, :C1]), wp, B=B, H=H, W=W, Hs=Hs, Ws=Ws, taps=taps, stride=stride, up=up, asym=asym,
                              x2=to_tok(x[:, C1:]) if C2 else None, bias=b.to(d) if use_bias else None,
                              rowvec=rv.half().to(d) if use_rv else None, resid=to_tok(rs) if use_res else None,
                              tile_m=tm, tile_n=tn, splits=splits, pipe=stg)
        except RuntimeError as e:        # an explicit split request that the shape cannot honour is an argument error
            assert splits > 1 and "gemm_conv" in str(e), (case, str(e))
            continue
        got = from_tok(y, B, H, W)
        err = (got - ref).abs()
        tol = 2e-3 * ref.abs() + 2e-3 * max(1.0, ref.abs().max().item())
        assert (err <= tol).all(), (case, mode, taps, C1, C2, N, B, H, W, tm, tn, splits, err.max().item())
        n_checked += 1
    assert n_checked >= 50


# which entries of ops.TILE_CANDIDATES lr_gemm_conv_f16 has an instance for, per epilogue mode (fp16 and bf16 alike, except that the erf-GELU
# epilogue is fp16 only) and for the phase form of the upsample conv; every other request is refused as `unsupported`
GEMM_INSTANCES = {
    "plain": {(128, 64, 0), (128, 128, 0), (128, 160, 0), (128, 128, 4), (128, 160, 4), (256, 128, 0), (256, 160, 0), (256, 256, 0),
              (256, 320, 0), (256, 160, 8), (256, 320, 8)},
    "geglu": {(128, 64, 0), (128, 128, 0), (128, 128, 4), (256, 128, 0), (256, 256, 0), (256, 320, 0)},
    "gelu": {(128, 64, 0), (128, 128, 0), (256, 128, 0)},
    # (pipe 0 on a 128-row tile is planned as the 4-stage ring: the only 128-row instances with the phase gather)
    "phase": {(128, 128, 0), (128, 160, 0), (128, 128, 4), (128, 160, 4), (256, 128, 0), (256, 160, 0), (256, 320, 0)},
}


def test_gemm_every_instance_is_reached_and_only_those():
    """Every ops.TILE_CANDIDATES entry under plain / GEGLU / erf-GELU in fp16 and bf16, and as the phase form, splits = 1, on a 3x3 conv of
    2 x 16 x 32 pixels, 320 -> 640 channels (four 256-row tiles; 640 = a multiple of 64, 128, 160, 320 with a column tail at 256): the
    combinations of GEMM_INSTANCES launch, the others raise `unsupported`, and what launches equals the 128 x 64 instance of its mode and
    dtype bit for bit (phase form: the 128 x 128 instance, there is no 128 x 64 one).
    Not bit-equal: the halo-tile instances (256, 160, 8) and (256, 320, 8), which accumulate chunk-major -- they are held to the bound of
    test_gemm_conv_randomised_shapes against F.conv2d instead."""
    from leftrefill_amd import ops, packing
    d = dev()
    B, H, W, C, N = 2, 16, 32, 320, 640
    w = torch.from_numpy(weights.fill_like("inst.w", (N, C, 3, 3)))
    launched = {}
    for dtype in (torch.float16, torch.bfloat16):
        tok = lambda t: t.permute(0, 2, 3, 1).reshape(-1, C).to(dtype).contiguous().to(d)
        x, xs = G.T("inst.x", (B, C, H, W)).to(dtype).float(), G.T("inst.xs", (B, C, H // 2, W // 2)).to(dtype).float()
        wr = w.to(dtype).float()
        w9, wp = packing.pack_conv(wr, cin_pad=C, dtype=dtype).to(d), packing.pack_conv_up_phase(wr, cin_pad=C, dtype=dtype).to(d)
        refs = {"plain": F.conv2d(x, wr, padding=1), "phase": F.conv2d(F.interpolate(xs, scale_factor=2, mode="nearest"), wr, padding=1)}

        def close(y, ref):
            err = (from_tok(y, B, H, W) - ref).abs()
            return bool((err <= 2e-3 * ref.abs() + 2e-3 * max(1.0, ref.abs().max().item())).all())

        for mode in ("plain", "geglu", "gelu", "phase"):
            base = {}
            for tm, tn, pipe in sorted(ops.TILE_CANDIDATES, key=lambda c: c != ((128, 128, 0) if mode == "phase" else (128, 64, 0))):
                kw = dict(B=B, H=H, W=W, tile_m=tm, tile_n=tn, pipe=pipe, splits=1)
                try:
                    if mode == "phase":
                        y = ops.gemm_conv(tok(xs), wp, Hs=H // 2, Ws=W // 2, taps=4, up=3, **kw)
                    else:
                        y = ops.gemm_conv(tok(x), w9, taps=9, geglu=mode == "geglu", gelu=mode == "gelu", **kw)
                except RuntimeError as e:
                    assert "unsupported" in str(e), (mode, dtype, tm, tn, pipe, str(e))
                    continue
                launched.setdefault((mode, dtype), set()).add((tm, tn, pipe))
                if not base:
                    base["y"] = y
                    assert mode not in refs or close(y, refs[mode]), (mode, dtype, tm, tn, pipe)
                elif pipe == 8:
                    assert close(y, refs[mode]), (mode, dtype, tm, tn, pipe)
                else:
                    assert torch.equal(y, base["y"]), (mode, dtype, tm, tn, pipe)
    want = {(mode, dtype): inst for mode, inst in GEMM_INSTANCES.items() for dtype in (torch.float16, torch.bfloat16)
            if (mode, dtype) != ("gelu", torch.bfloat16)}
    assert launched == want


def test_attention_randomised_shapes():
    """30 random (B, heads, Nq, Nkv) problems, ragged in both dimensions, on all three V paths (transpose read, pre-transposed,
    register-transposed), against the oracle's attention."""
    import random
    from leftrefill_amd import ops
    rng = random.Random(99)
    d = dev()
    for case in range(30):
        B, heads = rng.randint(1, 3), rng.randint(1, 4)
        Nq, Nkv = rng.randint(1, 400), rng.randint(1, 600)
        mode = rng.choice(["tr", "vt", "reg"])
        with v_path(mode):
            C = heads * 64
            q = h16(G.T(f"attfz{case}.q", (B, Nq, C)))
            k = h16(G.T(f"attfz{case}.k", (B, Nkv, C)))
            v = h16(G.T(f"attfz{case}.v", (B, Nkv, C)))
            ref = unet_ref.attention(q, k, v, heads, unet_ref._Mode("fp32"))
            kv = torch.cat([k, v], -1).reshape(B * Nkv, 2 * C).half().to(d)
            o = ops.attention(q.reshape(B * Nq, C).half().to(d), kv[:, :C], kv[:, C:], B, heads, Nq, Nkv, 64 ** -0.5)
            err = (o.float().cpu().reshape(B, Nq, C) - ref).abs().max().item()
            assert err < 3e-3, (case, B, heads, Nq, Nkv, mode, err)
