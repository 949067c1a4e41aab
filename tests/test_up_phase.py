"""The phase form of the Upsample conv (lr_gemm_args.up = 3): nearest-2x + 3x3 pad-1 conv as four 2x2 convs on the source.

Reference for every GPU case: F.conv2d(F.interpolate(x, 2, "nearest"), w, b, padding=1) in fp32 on the fp16-rounded inputs and
weights; bound rtol 2e-3 / atol 1e-3, no element outside (what tests/test_gpu_ops.py asks of `c3_up`).  The phase form multiplies
by merged taps that were rounded to fp16 once more, so it is NOT bit-equal to up = 1 and nothing here asserts that; each case prints
the max error of both forms side by side.  Within the phase form everything that is bit-exact for up = 1 stays so: repeated calls,
batch permutation, eager == graph replay of a UNet.

bf16 twin: same reference on bf16-rounded inputs; bound = the fp16 bound times 8, the ratio of the two formats' roundings (2^-8 against
2^-11) -- the bound tests/test_gpu_bf16.py uses for every bf16 operator: rtol 1.6e-2 / atol 8e-3.
"""
import zlib

import pytest
import torch
import torch.nn.functional as F

RTOL, ATOL = 2e-3, 1e-3


# ---------------------------------------------------------------------------------------------------------------------
# CPU: the weight identity and its rounding
# ---------------------------------------------------------------------------------------------------------------------
def _phase_conv(x, taps, b):
    """The four 2x2 convs on the zero-padded source, interleaved into the 2x output (taps [2, 2, Cout, Cin, 2, 2])."""
    N, _, H, W = x.shape
    out = x.new_zeros(N, taps.shape[2], 2 * H, 2 * W)
    xp = F.pad(x, (1, 1, 1, 1))
    for a in (0, 1):
        for c in (0, 1):
            out[:, :, a::2, c::2] = F.conv2d(xp[:, :, a:a + H + 1, c:c + W + 1], taps[a, c], b)
    return out


def test_phase_weights_reproduce_upsample_conv_fp64():
    from leftrefill_amd import packing
    g = torch.Generator().manual_seed(11)
    x = torch.randn(2, 6, 5, 7, generator=g, dtype=torch.float64)
    w = torch.randn(10, 6, 3, 3, generator=g, dtype=torch.float64)
    b = torch.randn(10, generator=g, dtype=torch.float64)
    ref = F.conv2d(F.interpolate(x, scale_factor=2, mode="nearest"), w, b, padding=1)
    got = _phase_conv(x, packing.up_phase_taps(w), b)
    assert (got - ref).abs().max().item() <= 1e-12


@pytest.mark.parametrize("dtype", [torch.float16, torch.bfloat16])
def test_phase_pack_is_nearest_to_exact_sum(dtype):
    from leftrefill_amd import packing
    g = torch.Generator().manual_seed(12)
    cout, cin = 40, 70
    w = torch.randn(cout, cin, 3, 3, generator=g) * 0.05
    pk = packing.pack_conv_up_phase(w, dtype=dtype)
    cin_pad, cout_pad = 128, 64
    assert pk.shape == (4, cout_pad, 4 * cin_pad) and pk.dtype == dtype and pk.is_contiguous()
    # the taps the up = 1 form multiplies by are the rounded ones; their sums in fp64 are exact, and fp64 -> 16 bits rounds to nearest
    exact = packing.up_phase_taps(w.to(dtype).double())                       # [2, 2, Cout, Cin, 2, 2]
    want = exact.to(dtype).permute(0, 1, 2, 4, 5, 3).reshape(4, cout, 4, cin)
    pk4 = pk.reshape(4, cout_pad, 4, cin_pad)
    assert torch.equal(pk4[:, :cout, :, :cin], want)
    assert pk4[:, cout:].abs().max().item() == 0 and pk4[:, :, :, cin:].abs().max().item() == 0
    # slice 2a + b, K index (2 dy + dx) * Cin_pad + c: spot check against the definition
    a, c, dy, dx = 1, 0, 0, 1          # rows i (ky 0, 1), columns j (kx 1, 2)
    wr = w.to(dtype).double()
    s = wr[:, :, 0, 1] + wr[:, :, 0, 2] + wr[:, :, 1, 1] + wr[:, :, 1, 2]
    assert torch.equal(pk4[2 * a + c, :cout, 2 * dy + dx, :cin], s.to(dtype))


# ---------------------------------------------------------------------------------------------------------------------
# GPU
# ---------------------------------------------------------------------------------------------------------------------
def dev():
    assert torch.cuda.is_available(), "GPU tests need a MI355X"
    return torch.device("cuda:0")


def to_tok(x, dtype=torch.float16):
    N, C, H, W = x.shape
    return x.permute(0, 2, 3, 1).reshape(N * H * W, C).to(dtype).contiguous().to(dev())


def from_tok(y, N, H, W):
    return y.float().cpu().reshape(N, H, W, -1).permute(0, 3, 1, 2)


_cases = {}


def make_case(key, N, Cin, Cout, Hs, Ws, C2=0, dtype=torch.float16):
    """Inputs rounded to `dtype`, the fp32 reference and the packed operands; built once per key and shared."""
    ck = (key, dtype)
    if ck in _cases:
        return _cases[ck]
    from leftrefill_amd import packing
    g = torch.Generator().manual_seed(zlib.crc32(key.encode()))
    Ct = Cin + C2
    x = torch.randn(N, Ct, Hs, Ws, generator=g).to(dtype).float()
    w = (torch.randn(Cout, Ct, 3, 3, generator=g) * (1.0 / (9 * Ct)) ** 0.5).to(dtype).float()
    b = 0.1 * torch.randn(Cout, generator=g)
    ref = F.conv2d(F.interpolate(x, scale_factor=2, mode="nearest"), w, b, padding=1)
    d = dev()
    c = dict(N=N, Cin=Cin, C2=C2, Cout=Cout, Hs=Hs, Ws=Ws, ref=ref,
             x1=to_tok(x[:, :Cin], dtype), x2=to_tok(x[:, Cin:], dtype) if C2 else None,
             w9=packing.pack_conv(w, cin_pad=Ct, dtype=dtype).to(d), wp=packing.pack_conv_up_phase(w, cin_pad=Ct, dtype=dtype).to(d),
             b=packing.pack_bias(b).to(d))
    _cases[ck] = c
    return c


def run_phase(c, **kw):
    from leftrefill_amd import ops
    return ops.gemm_conv(c["x1"], c["wp"], B=c["N"], H=2 * c["Hs"], W=2 * c["Ws"], Hs=c["Hs"], Ws=c["Ws"], taps=4, up=3, x2=c["x2"],
                         bias=c["b"], **kw)


def run_up1(c, **kw):
    from leftrefill_amd import ops
    return ops.gemm_conv(c["x1"], c["w9"], B=c["N"], H=2 * c["Hs"], W=2 * c["Ws"], Hs=c["Hs"], Ws=c["Ws"], taps=9, up=1, x2=c["x2"],
                         bias=c["b"], **kw)


def check(name, c, y, y1, rtol=RTOL, atol=ATOL):
    N, H, W, Cout = c["N"], 2 * c["Hs"], 2 * c["Ws"], c["Cout"]
    ref = c["ref"]
    out, out1 = from_tok(y[:, :Cout], N, H, W), from_tok(y1[:, :Cout], N, H, W)
    err, err1 = (out - ref).abs(), (out1 - ref).abs()
    tol = atol + rtol * ref.abs()
    bad = (err > tol).sum().item()
    print(f"[{name}] phase max_abs_err {err.max().item():.3e} viol {bad}/{err.numel()} | up=1 max_abs_err {err1.max().item():.3e} "
          f"viol {(err1 > tol).sum().item()} | bit-equal {100 * (out == out1).float().mean().item():.1f} %")
    assert torch.isfinite(out).all(), name
    assert bad == 0, f"{name}: {bad} elements outside rtol={rtol} atol={atol}; max err {err.max().item():.3e}"
    if y.shape[1] > Cout:      # padded output channels: zero weights, zero bias
        assert y[:, Cout:].abs().max().item() == 0


SHAPES = [
    # name, N, Cin, Cout, Hs, Ws, C2
    ("src1x1", 1, 64, 64, 1, 1, 0),              # every tap but one is out of the image
    ("odd3x5", 2, 128, 192, 3, 5, 0),            # sample boundary, odd sizes, an M tail inside every phase, an N tail
    ("c3_up", 1, 640, 640, 4, 6, 0),             # the c3_up case of test_gpu_ops.py: output 8 x 12
    ("src8x12", 1, 640, 640, 8, 12, 0),          # ... and with 8 x 12 as the source grid
    ("cat6x10", 2, 320, 320, 6, 10, 320),        # concat source 2
]


@pytest.mark.gpu
@pytest.mark.parametrize("name,N,Cin,Cout,Hs,Ws,C2", SHAPES, ids=[s[0] for s in SHAPES])
def test_phase_form_matches_upsample_conv(name, N, Cin, Cout, Hs, Ws, C2):
    c = make_case(name, N, Cin, Cout, Hs, Ws, C2)
    y = run_phase(c)
    check(name, c, y, run_up1(c))
    assert torch.equal(y, run_phase(c)), "two calls on the same input differ"


# one case per tile instance the mode can select, two row tiles per phase with a row tail (2 x 12 x 12 = 288 source pixels), the second
# sample starting inside a tile, and an N tail: Cout = 192 on 128-column tiles, 384 on 160- and 320-column tiles; split-K on both tile heights
TILES = [(128, 128, 192, 1), (128, 160, 384, 1), (256, 128, 192, 1), (256, 160, 384, 1), (256, 320, 384, 1), (256, 160, 384, 2), (128, 160, 384, 3)]


@pytest.mark.gpu
@pytest.mark.parametrize("tm,tn,Cout,splits", TILES, ids=["%dx%d_n%d_s%d" % t for t in TILES])
def test_phase_form_every_tile_instance(tm, tn, Cout, splits):
    c = make_case(f"tiles{Cout}", 2, 128, Cout, 12, 12)
    y = run_phase(c, tile_m=tm, tile_n=tn, splits=splits)
    check(f"tile {tm}x{tn} s{splits}", c, y, run_up1(c))
    assert torch.equal(y, run_phase(c, tile_m=tm, tile_n=tn, splits=splits))


@pytest.mark.gpu
def test_phase_form_rowvec_and_residual():
    """The per-sample row vector and the residual are addressed by OUTPUT row."""
    from leftrefill_amd import ops
    c = make_case("rvres", 2, 128, 192, 5, 6)
    N, H, W, Cout = 2, 10, 12, 192
    g = torch.Generator().manual_seed(5)
    rv = torch.randn(N, Cout, generator=g).half().float()
    rs = torch.randn(N, Cout, H, W, generator=g).half().float()
    kw = dict(rowvec=rv.half().to(dev()), resid=to_tok(rs))
    y, y1 = run_phase(c, **kw), run_up1(c, **kw)
    c2 = dict(c, ref=c["ref"] + rv[:, :, None, None] + rs)
    check("rowvec + resid", c2, y, y1)


@pytest.mark.gpu
def test_phase_form_bf16():
    c = make_case("bf16_odd3x5", 2, 128, 192, 3, 5, dtype=torch.bfloat16)
    y = run_phase(c)
    assert y.dtype == torch.bfloat16
    check("bf16 odd3x5", c, y, run_up1(c), rtol=8 * RTOL, atol=8 * ATOL)


@pytest.mark.gpu
def test_phase_form_batch_permutation():
    c = make_case("perm", 2, 128, 192, 6, 8)
    M1 = c["Hs"] * c["Ws"]
    y = run_phase(c)
    sw = dict(c, x1=torch.cat([c["x1"][M1:], c["x1"][:M1]]).contiguous())
    ys = run_phase(sw)
    assert torch.equal(y[:4 * M1], ys[4 * M1:]) and torch.equal(y[4 * M1:], ys[:4 * M1])


@pytest.mark.gpu
@pytest.mark.parametrize("tm,tn,splits", [(128, 160, 1), (256, 160, 1), (256, 320, 1), (256, 160, 2)], ids=["128x160", "256x160", "256x320", "256x160_s2"])
def test_phase_form_groupnorm_statistics(tm, tn, splits):
    """The GroupNorm statistics of the consumer come out of the phase launch: the per-channel partials (through lr_groupnorm_finalize) and,
    where the tile lies inside one sample, the per-group partials (straight into the apply kernel) normalise the launch's own fp16 output
    like F.group_norm in fp32 does -- the bound of test_groupnorm_statistics_from_gemm_epilogue (rtol 2e-3 / atol 1e-3 on the normalised
    output, block sums within rtol 1e-5 / atol 2e-3)."""
    from leftrefill_amd import ops
    N, Hs, Ws, Cout = 2, 8, 16, 320            # 128 source pixels per sample: whole 128-row tiles, half a 256-row tile
    c = make_case("gnstat", N, 128, Cout, Hs, Ws)
    H, W = 2 * Hs, 2 * Ws
    y, gs = run_phase(c, tile_m=tm, tile_n=tn, splits=splits, want_gn_stats=True)
    check(f"gn producer {tm}x{tn}", c, y, run_up1(c))
    assert gs is not None
    part, R, gp, chunks = gs
    assert part.shape == (N * H * W // R, Cout, 2)
    yf = y.float()
    # the row blocks of a sample are contiguous, whatever rows each one holds: per-sample totals
    tot = part.double().reshape(N, H * W // R, Cout, 2).sum(1)
    ys = yf.double().reshape(N, H * W, Cout)
    nb = H * W // R
    assert torch.allclose(tot[..., 0], ys.sum(1), rtol=1e-5, atol=2e-3 * nb)
    assert torch.allclose(tot[..., 1], (ys * ys).sum(1), rtol=1e-5, atol=2e-3 * nb)
    if splits == 1:      # block (sample, phase, k): R consecutive source pixels of one phase
        yb = yf.reshape(N, Hs, 2, Ws, 2, Cout).permute(0, 2, 4, 1, 3, 5).reshape(N * 4 * Hs * Ws // R, R, Cout)
        assert torch.allclose(part[..., 0], yb.sum(1), rtol=1e-5, atol=2e-3)
        assert torch.allclose(part[..., 1], (yb * yb).sum(1), rtol=1e-5, atol=2e-3)
    g = torch.Generator().manual_seed(3)
    gam, bet = 1.0 + 0.3 * torch.randn(Cout, generator=g), 0.2 * torch.randn(Cout, generator=g)
    ref = F.group_norm(from_tok(y, N, H, W), 32, gam, bet, 1e-5)
    d = dev()
    out = ops.group_norm_fused(y, N, H * W, gam.to(d), bet.to(d), 1e-5, False, gs)
    err = (from_tok(out, N, H, W) - ref).abs()
    print(f"[gn(finalize) {tm}x{tn}] max_abs_err {err.max().item():.3e}")
    assert (err > ATOL + RTOL * ref.abs()).sum().item() == 0
    if (Hs * Ws) % tm == 0 or splits > 1:
        assert gp is not None and chunks == H * W // (tm if splits == 1 else 32)
    if gp is not None:
        gt = gp.double().sum(1)                                                      # [N, 32, 2]
        yg = ys.reshape(N, H * W, 32, Cout // 32)
        assert torch.allclose(gt[..., 0], yg.sum((1, 3)), rtol=1e-5, atol=5e-3 * chunks)
        assert torch.allclose(gt[..., 1], (yg * yg).sum((1, 3)), rtol=1e-5, atol=5e-3 * chunks)
        out2 = ops.group_norm_groups(y, N, H * W, gam.to(d), bet.to(d), 1e-5, False, gp, chunks)
        err2 = (from_tok(out2, N, H, W) - ref).abs()
        print(f"[gn(groups) {tm}x{tn}] max_abs_err {err2.max().item():.3e}")
        assert (err2 > ATOL + RTOL * ref.abs()).sum().item() == 0
    # the statistics do not depend on where a sample sits in the batch
    M1 = Hs * Ws
    sw = dict(c, x1=torch.cat([c["x1"][M1:], c["x1"][:M1]]).contiguous())
    _, gs2 = run_phase(sw, tile_m=tm, tile_n=tn, splits=splits, want_gn_stats=True)
    p2 = gs2[0].reshape(N, nb, Cout, 2)
    assert torch.equal(part.reshape(N, nb, Cout, 2), torch.cat([p2[1:], p2[:1]]))


@pytest.mark.gpu
def test_phase_form_rejects_what_it_does_not_support():
    from leftrefill_amd import ops
    c = make_case("odd3x5", 2, 128, 192, 3, 5)
    for kw in (dict(asym=True), dict(geglu=True), dict(pipe=8, tile_m=256, tile_n=160), dict(tile_m=128, tile_n=64), dict(want_stats=True)):
        with pytest.raises(RuntimeError):
            run_phase(c, **kw)


@pytest.mark.gpu
def test_unet_with_upsample_eager_equals_graph_replay():
    """The MID config has an Upsample: its conv takes the phase form at inference, and eager launches, the captured graph and a second
    replay give the same bits."""
    import leftrefill_amd.dropin as dropin
    dropin.install()
    from ldm.modules.diffusionmodules.openaimodel import UNetModel
    from oracle import golden_spec as G
    from leftrefill_amd import ops
    case, cname, N, H, W, ts = [u for u in G.UNET_CASES if u[1] == "MID"][0]
    cfg = G.CONFIGS[cname]
    m = UNetModel(**cfg.kwargs())
    m.load_state_dict(G.unet_state(cname), strict=True)
    m = m.to(dev()).eval()
    x, t, ctx = G.unet_inputs(case, cfg, N, H, W, ts)
    x, t, ctx = x.to(dev()), t.to(dev()), ctx.to(dev())
    ups = []
    orig = ops.gemm_conv

    def spy(*a, **k):
        ups.append(k.get("up", 0))
        return orig(*a, **k)

    m.use_hip_graph = False
    ops.gemm_conv = spy
    try:
        with torch.no_grad():
            y_eager = m(x, t, ctx)
    finally:
        ops.gemm_conv = orig
    assert 3 in ups and 1 not in ups, "the Upsample convs of the inference step take the phase form"
    m.use_hip_graph = True
    with torch.no_grad():
        y_graph = m(x, t, ctx)
        y_graph2 = m(x, t, ctx)
    assert torch.equal(y_eager, y_graph) and torch.equal(y_graph, y_graph2)
