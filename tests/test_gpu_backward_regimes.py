"""The backward kernels at the loop regimes the training benchmark runs (batch 16 on 64x128 latents), in fp16 AND bf16: the 4-deep load batches
plus serial tail of the GroupNorm backward, uneven / empty statistics chunks, the complete LayerNorm width dispatch, uneven / tail-only / empty
query slices of the dK / dV kernel, the GEGLU grid-stride loop past its wrap, and the exact re-arrangement kernels called directly.

Conventions of tests/test_gpu_backward.py: inputs, weights and upstream gradients are rounded to the 16-bit type first so both sides
differentiate the same function; the reference is torch.autograd on the CPU, here in float64; every figure is printed before it is asserted.

Tolerances.  fp16: `check` of test_gpu_backward.py unchanged (rel-L2 < 3e-3; per element 2e-3 max|ref| + 2e-3 |ref|; 4e-3 for the GroupNorm that
reads producer statistics).  bf16: 8x the fp16 bound per element (tolerance table: the ratio of the unit roundoffs) =
1.6e-2 max|ref| + 1.6e-2 |ref|, and the relative L2 figures of test_gpu_bf16.py::test_backward_kernels_bf16 (1.2e-2; 1.5e-2 for attention).

Every test asserts, from a pure-Python mirror of the launch arithmetic (`gn_bwd_launch`, `attn_bwd_slices`, `geglu_grid`), that its shape is in
the regime it names: a shape that silently falls out of its regime fails."""
import ctypes
import functools

import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

from oracle import golden_spec as G, unet_ref, weights  # noqa: E402
from tests.test_gpu_backward import check as check_f16, dev  # noqa: E402

F16, BF = torch.float16, torch.bfloat16
both_types = pytest.mark.parametrize("dt", [F16, BF], ids=["f16", "bf16"])
BF_ELEM, BF_REL_L2, BF_REL_L2_ATTN = 1.6e-2, 1.2e-2, 1.5e-2


def r16(t, dt):
    """Rounded to the 16-bit type, as float64 (what the reference differentiates)."""
    return t.to(dt).double()


def to_tok(x, dt):       # NCHW -> token-major 16-bit on the device
    n, c, hh, ww = x.shape
    return x.permute(0, 2, 3, 1).reshape(n * hh * ww, c).to(dt).contiguous().to(dev())


def from_tok(t, n, hh, ww):
    return t.float().cpu().reshape(n, hh, ww, -1).permute(0, 3, 1, 2)


def check(name, got, ref, dt, rtol=2e-3, atol_scale=2e-3, attn=False):
    """fp16: the bound of test_gpu_backward.py as it stands.  bf16: the documented 8x of the plain fp16 bound per element + the relative L2 of
    test_backward_kernels_bf16."""
    if dt == F16:
        return check_f16(name, got, ref, rtol=rtol, atol_scale=atol_scale)
    got, ref = got.float().cpu().double(), ref.double()
    assert torch.isfinite(got).all(), name
    scale = ref.abs().max().item()
    err = (got - ref).abs()
    rel = (err.norm() / ref.norm()).item()
    print(f"[bwd bf16 {name}] rel_l2 {rel:.3e} max_abs {err.max().item():.3e} (|ref| max {scale:.3e})")
    assert rel <= (BF_REL_L2_ATTN if attn else BF_REL_L2), (name, rel)
    assert (err <= BF_ELEM * scale + BF_ELEM * ref.abs()).all(), name


# =====================================================================================================================
# 1. Regime guard: the launch arithmetic, restated
# =====================================================================================================================
# mirrors leftrefill_amd/csrc/norm.hip: gn_nchunks (lines 276-287), lr_groupnorm_bwd_t (794-798: nOct / R / threads; 802-809: the backward's own
# nchunks; 816-820: ppb of the apply pass), the chunk bounds of gn_bwd_stats_kernel (649-650), the pixel loops of both kernels (678-690, 769-781)
LR_GN_CHUNKS = 256


def gn_nchunks(N, HW, C):
    want = (N * HW * C * 2) >> 19
    c = (max(want, 256) + N - 1) // N
    return max(1, min(c, LR_GN_CHUNKS, HW // 8))


def gn_bwd_launch(N, HW, C):
    nOct = C // 8
    R = max(1, 256 // nOct)
    nchunks = max((1024 + N - 1) // N, gn_nchunks(N, HW, C))
    nchunks = max(1, min(nchunks, LR_GN_CHUNKS, HW // 8))
    per = (HW + nchunks - 1) // nchunks
    ppb = (N * HW + max((N * HW * C * 2) >> 18, 512) - 1) // max((N * HW * C * 2) >> 18, 512)
    ppb = min(max(ppb, 16), HW)
    spans = [(c * per, min(HW, c * per + per)) for c in range(nchunks)]      # (p0, p1) of every statistics chunk; p1 < p0: empty
    return dict(R=R, threads=nOct * R, fwd_chunks=gn_nchunks(N, HW, C), nchunks=nchunks, per=per, ppb=ppb, spans=spans,
                apply_last=HW - (HW - 1) // ppb * ppb)


def pixel_loop(R, r, length):
    """(4-deep batches, serial tail iterations) of pixel row r over a span of `length` pixels."""
    p, nb, ns = r, 0, 0
    while p + 3 * R < length:
        p, nb = p + 4 * R, nb + 1
    while p < length:
        p, ns = p + R, ns + 1
    return nb, ns


# mirrors leftrefill_amd/csrc/attention_bwd.hip, attn_bwd_dkv_kernel (lines 255-258: ntiles_all, t_per, t0, ntiles); the slice count is the front
# end's (train_ops.attn_bwd_q_splits)
def attn_bwd_slices(Nq, q_splits):
    ntiles = (Nq + 63) // 64
    t_per = (ntiles + q_splits - 1) // q_splits
    return ntiles, t_per, [(sp * t_per, min(ntiles, sp * t_per + t_per)) for sp in range(q_splits)]


# mirrors leftrefill_amd/csrc/elementwise.hip, lr_geglu_fwd_t / lr_geglu_bwd_t (lines 816-818, 827-829): work items and grid
def geglu_grid(M, H):
    total = M * (H // 8)
    return total, min((total + 255) // 256, 65536) * 256


def test_regime_mirror_constants():
    from leftrefill_amd import ops
    assert ops.GN_CHUNKS == LR_GN_CHUNKS
    # the benchmark's own shape (N = 16, HW = 8192, C = 320): 128-pixel statistics chunks, 256-pixel apply blocks
    L = gn_bwd_launch(16, 8192, 320)
    assert (L["R"], L["per"], L["ppb"]) == (6, 128, 256)
    # every shape of tests/test_gpu_backward.py sees 8-pixel chunks and 16-pixel apply blocks: no batch for R = 6 / R = 3
    for N, C, HW in ((2, 320, 128), (1, 960, 128), (2, 320, 256), (1, 2560, 64)):
        L = gn_bwd_launch(N, HW, C)
        assert (L["per"], L["ppb"]) == (8, 16)


# =====================================================================================================================
# 2. GroupNorm backward
# =====================================================================================================================
def _samples(name, shape, base=4):
    """G.T for the first `base` samples; every further sample is one of them rotated along W and mapped affinely, so that a batch of 32 costs
    the generator 4 samples and no two samples are alike."""
    N = shape[0]
    if N <= base:
        return G.T(name, shape)
    b = G.T(name, (base,) + tuple(shape[1:]))
    return torch.cat([torch.roll(b, 3 * i, -1) * (1.0 + 0.125 * i) + 0.0625 * i for i in range((N + base - 1) // base)])[:N].contiguous()


@functools.lru_cache(maxsize=2)
def _gn_reference(tag, N, C, H, W, silu, eps, dt, big_mean=False):
    """(x, dy) rounded to dt, gamma, beta and d/dx of [SiLU](GroupNorm(x)) . dy in float64: computed once per shape and type, shared by the plain
    and the fork form (whose gradient is this one + 0.5 dy)."""
    x = _samples(tag + ".x", (N, C, H, W))
    if big_mean:
        x = 50.0 + 0.5 * x
        g, b = 1.0 + 0.3 * G.T(tag + ".g", (C,)), 0.2 * G.T(tag + ".b", (C,))
    else:
        g = torch.from_numpy(weights.fill_like(tag + ".weight", (C,)))
        b = torch.from_numpy(weights.fill_like(tag + ".bias", (C,)))
    # dy leans on x and has a mean: the two group sums of the backward (S1, S2) are then O(1) terms of every dx, and a pixel the statistics
    # pass misses shows in the whole sample (with independent zero-mean dy they are O(1 / sqrt(HW C / 32)) and hide a lost chunk in rounding)
    x16 = x.to(dt)
    dy16 = (0.7 * _samples(tag + ".dy", (N, C, H, W)) + 0.4 * (x - x.mean()) / x.std() + 0.25).to(dt)
    xr = x16.double().requires_grad_(True)
    y = F.group_norm(xr, 32, g.double(), b.double(), eps)
    (F.silu(y) if silu else y).backward(dy16.double())
    return x16, dy16, g, b, xr.grad


def _gn_claims(N, C, H, W, claims):
    L = gn_bwd_launch(N, H * W, C)
    R, per, ppb, HW = L["R"], L["per"], L["ppb"], H * W
    print(f"[regime gn N={N} C={C} HW={HW}] R {R} threads {L['threads']} nchunks {L['nchunks']} (forward {L['fwd_chunks']}) per {per} ppb {ppb} "
          f"last apply block {L['apply_last']}")
    lens = [p1 - p0 for p0, p1 in L["spans"]]
    for c in claims:
        if c == "stats: >= 2 batches and a serial tail for row 0":
            nb, ns = pixel_loop(R, 0, per)
            assert lens[0] == per and nb >= 2 and ns >= 1 and per % (4 * R), (c, per, nb, ns)
        elif c == "apply: batches and a serial tail for row 0":
            nb, ns = pixel_loop(R, 0, ppb)
            assert ppb > 4 * R and nb >= 1 and ns >= 1 and HW >= ppb, (c, ppb, nb, ns)
        elif c == "last chunk empty, the one before short":
            assert lens[-1] <= 0 and 0 < lens[-2] < per, (c, lens[-3:])
        elif c == "short last apply block":
            assert 0 < L["apply_last"] < ppb, (c, L["apply_last"], ppb)
        elif c == "R = 1, more than 256 threads":
            assert R == 1 and L["threads"] > 256, (c, R, L["threads"])
        elif c == "R = 2":
            assert R == 2, (c, R)
        elif c == "stats: batches and a serial tail for row 0":
            nb, ns = pixel_loop(R, 0, per)
            assert nb >= 1 and ns >= 1, (c, per, nb, ns)
        else:
            raise AssertionError(c)
    return L


def _gn_run(dt, name, ref, N, C1, C2, H, W, silu, eps, fork):
    from leftrefill_amd import train_ops as T
    d = dev()
    x16, dy16, g, b, grad = ref
    if fork:
        grad = grad + 0.5 * dy16.double()
    x1 = to_tok(x16[:, :C1], dt).requires_grad_(True)
    x2 = to_tok(x16[:, C1:], dt).requires_grad_(True) if C2 else None
    assert x1.dtype == dt
    if fork:
        out, a1, a2 = T.group_norm_fork(x1, N, H * W, g.to(d), b.to(d), eps, silu, x2)
        res = 0.5 * (a1 if a2 is None else torch.cat([a1, a2], dim=1))      # (C2 > 0: dres1 AND dres2 reach lr_groupnorm_bwd_res)
        (out + res).backward(to_tok(dy16, dt))
    else:
        T.group_norm(x1, N, H * W, g.to(d), b.to(d), eps, silu, x2).backward(to_tok(dy16, dt))
    check(name + " dx1", from_tok(x1.grad, N, H, W), grad[:, :C1], dt)
    if C2:
        check(name + " dx2", from_tok(x2.grad, N, H, W), grad[:, C1:], dt)


TRAIN = ("stats: >= 2 batches and a serial tail for row 0", "apply: batches and a serial tail for row 0")
UNEVEN = ("last chunk empty, the one before short", "short last apply block")
GN_CASES = [      # (tag, N, C1, C2, H, W, SiLU, eps, fork, claims); a shape's plain and fork cases are neighbours and share one reference
    # C = 320 (R = 6): 32 chunks of 56 pixels (batches at 0 and 24, tail 48, 54), apply blocks of 112; the fork takes it as two 160-channel
    # sources, so both residual gradients (dres1, dres2) are present
    ("c320", 32, 320, 0, 32, 56, True, 1e-5, False, TRAIN),
    ("c320", 32, 160, 160, 32, 56, True, 1e-5, True, TRAIN),
    # C = 640 (R = 3): 32 chunks of 25 (batches at 0 and 12, tail 24), the last one 7 pixels; apply blocks of 49, the last one 47
    ("c640", 32, 640, 0, 23, 34, True, 1e-5, False, TRAIN + ("short last apply block",)),
    ("c640", 32, 640, 0, 23, 34, False, 1e-6, False, TRAIN + ("short last apply block",)),
    # 1280 + 1280 (R = 1, 320 threads): 40 chunks of 9 (batches at 0 and 4, tail 8), chunk 36 holds 1 pixel, chunks 37-39 are empty
    ("c2560", 1, 1280, 1280, 13, 25, True, 1e-5, False, ("R = 1, more than 256 threads", "stats: >= 2 batches and a serial tail for row 0",
                                                         "short last apply block")),
    # HW = 105 = 8 * 13 + 1: 13 chunks of 9, chunk 11 holds 6 pixels, chunk 12 is empty; 7 apply blocks, the last one 9 pixels
    ("uneven320", 2, 320, 0, 7, 15, True, 1e-5, False, UNEVEN),
    ("uneven320", 2, 320, 0, 7, 15, True, 1e-5, True, UNEVEN),
    ("uneven960", 2, 640, 320, 7, 15, True, 1e-5, False, UNEVEN + ("R = 2", "stats: batches and a serial tail for row 0")),
    ("uneven960", 2, 640, 320, 7, 15, True, 1e-5, True, UNEVEN + ("R = 2", "stats: batches and a serial tail for row 0")),
]


@both_types
@pytest.mark.parametrize("tag,N,C1,C2,H,W,silu,eps,fork,claims", GN_CASES,
                         ids=[f"{c[0]}{'' if c[6] else '_nosilu'}{'_fork' if c[8] else ''}" for c in GN_CASES])
def test_groupnorm_backward_training_regime(dt, tag, N, C1, C2, H, W, silu, eps, fork, claims):
    """[SiLU](GroupNorm([x1 | x2])) through lr_groupnorm_bwd_res at chunk / block sizes that run the 4-deep load batches AND the serial tail, at
    uneven chunking, and (fork) + 0.5 [x1 | x2] with the residual gradients added inside the kernel."""
    _gn_claims(N, C1 + C2, H, W, claims)
    ref = _gn_reference("gnr." + tag, N, C1 + C2, H, W, silu, eps, dt)
    _gn_run(dt, f"groupnorm {tag}{' fork' if fork else ''}", ref, N, C1, C2, H, W, silu, eps, fork)


@both_types
def test_groupnorm_backward_producer_statistics_at_training_hw(dt):
    """conv -> GroupNorm + SiLU at the HW of the C = 320 shape above: the forward partials come from the conv's epilogue in the GEMM's own row
    blocks, so the backward finalises mean / rstd over `fwd_chunks` != its own chunk count."""
    from leftrefill_amd import engine as E, packing, train_ops as T
    N, Cin, C, H, W = 2, 320, 320, 32, 56
    tag = "gnr.prod"
    x = r16(G.T(tag + ".x", (N, Cin, H, W)), dt)
    w = r16(torch.from_numpy(weights.fill_like(tag + ".w", (C, Cin, 3, 3))), dt)
    bb = torch.from_numpy(weights.fill_like(tag + ".b", (C,)))
    g = torch.from_numpy(weights.fill_like(tag + ".weight", (C,)))
    b = torch.from_numpy(weights.fill_like(tag + ".bias", (C,)))
    dy = r16(G.T(tag + ".dy", (N, C, H, W)), dt)
    xr = x.clone().requires_grad_(True)
    yr = F.conv2d(xr, w, bb.double(), padding=1)
    F.silu(F.group_norm(r16(yr.detach(), dt) + (yr - yr.detach()), 32, g.double(), b.double(), 1e-5)).backward(dy)   # (the HIP side normalises the rounded conv output)
    wp = packing.pack_conv(w.float(), cin_pad=Cin, dtype=dt).to(dev())
    x1 = to_tok(x, dt).requires_grad_(True)
    y1, gs1 = T.gemm_conv(x1, wp, B=N, H=H, W=W, taps=9, bias=packing.pack_bias(bb).to(dev()), want_gn_stats=True)
    assert gs1 is not None and y1.requires_grad
    act = E.Act(y1, N, H, W, gs=gs1)
    st = E._gn_train_stats(act)
    assert st is not None and st[0] == "groups"
    L = gn_bwd_launch(N, H * W, C)
    print(f"[regime gn producer] forward chunks {st[2]} (producer), backward chunks {L['nchunks']}, own statistics pass {L['fwd_chunks']}")
    assert st[2] not in (L["nchunks"], L["fwd_chunks"])
    pn = type("PN", (), {"g": g.to(dev()), "b": b.to(dev()), "eps": 1e-5})()
    E.gn(act, pn, True).tok.backward(to_tok(dy, dt))
    check("conv -> groupnorm (producer statistics) dx", from_tok(x1.grad, N, H, W), xr.grad, dt, rtol=4e-3, atol_scale=4e-3)


@both_types
def test_groupnorm_backward_large_mean_small_variance(dt):
    """Mean 50, std 0.5 (the inputs of test_groupnorm_large_mean_small_variance): the backward re-derives mean / rstd from the same (sum, sumsq)
    partials as the forward; a loss in the variance scales the whole gradient.  Plain and fork."""
    N, C, H, W = 2, 320, 16, 32
    ref = _gn_reference("gn_big", N, C, H, W, True, 1e-5, dt, True)
    grad = ref[4]
    _gn_run(dt, "groupnorm large mean", ref, N, C, 0, H, W, True, 1e-5, fork=False)
    _gn_run(dt, "groupnorm large mean fork", ref, N, C, 0, H, W, True, 1e-5, fork=True)
    assert grad.abs().max().item() > 0.5          # (rstd ~ 2: a gradient of the size of dy / std, not a degenerate case)


# =====================================================================================================================
# 3. LayerNorm backward
# =====================================================================================================================
def _ln_case(dt, name, x, dy, g, b):
    from leftrefill_amd import train_ops as T
    d = dev()
    M, C = x.shape
    xr = x.clone().requires_grad_(True)
    F.layer_norm(xr, (C,), g.double(), b.double(), 1e-5).backward(dy)
    xd = x.to(dt).to(d).requires_grad_(True)
    T.layer_norm(xd, g.to(d), b.to(d), 1e-5).backward(dy.to(dt).to(d))
    check(f"layernorm {name}", xd.grad, xr.grad, dt)
    # fork: 2 LayerNorm(x) + x, the residual gradient added inside lr_layernorm_bwd_res
    xf = x.to(dt).to(d).requires_grad_(True)
    n, xa = T.layer_norm_fork(xf, g.to(d), b.to(d), 1e-5)
    (2.0 * n + xa).backward(dy.to(dt).to(d))
    check(f"layernorm fork {name}", xf.grad, 2.0 * xr.grad + dy, dt)


@both_types
@pytest.mark.parametrize("C", [1024, 1536, 2048])
def test_layernorm_backward_full_waves(dt, C):
    """NV = 2, 3, 4 with every lane of the last octet wave busy (C = 64 * 8 * NV); M = 130: the last 4-row block is half full."""
    M = 130
    assert (C // 8 + 63) // 64 == C // 512 and C % 512 == 0 and M % 4 == 2
    x = r16(G.T(f"lnr.x{C}", (M, C)), dt)
    dy = r16(0.7 * G.T(f"lnr.dy{C}", (M, C)) + 0.4 * x + 0.25, dt)      # (leans on x, has a mean: the row sums of the backward are O(1) terms)
    g = torch.from_numpy(weights.fill_like(f"lnr.{C}.weight", (C,)))
    b = torch.from_numpy(weights.fill_like(f"lnr.{C}.bias", (C,)))
    _ln_case(dt, f"{M}x{C}", x, dy, g, b)


@both_types
def test_layernorm_backward_large_mean_rows(dt):
    """The rows of test_layernorm_fold_large_mean_rows (mean 40 / -25, std 0.5) through the backward."""
    M, C = 256, 320
    x = G.T("lnbig.x", (M, C)) * 0.5
    x[::3] += 40.0
    x[1::3] -= 25.0
    x = r16(x, dt)
    dy = r16(0.7 * G.T("lnbig.dy", (M, C)) + 0.4 * (x - x.mean(1, keepdim=True)) + 0.25, dt)
    g, b = 1.0 + 0.3 * G.T("lnbig.g", (C,)), 0.2 * G.T("lnbig.be", (C,))
    _ln_case(dt, "large-mean rows", x, dy, g, b)


@both_types
def test_layernorm_backward_rejects_width_2056(dt):
    """C = 2056 (a multiple of 8 past the NV = 4 limit): the alignment error, and no launch -- the pre-filled output stays as it was."""
    from leftrefill_amd import _lib
    lib = _lib.load()
    d = dev()
    st = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    M, C = 8, 2056
    x = torch.zeros(M, C, device=d, dtype=dt)
    gam = torch.ones(C, device=d)
    dx = torch.full((M, C), 7.0, device=d, dtype=dt)
    eps = ctypes.c_float(1e-5)
    assert _lib.fn(lib, "lr_layernorm_bwd", dt)(x.data_ptr(), x.data_ptr(), gam.data_ptr(), eps, dx.data_ptr(), M, C, st) == -2
    assert _lib.fn(lib, "lr_layernorm_bwd_res", dt)(x.data_ptr(), x.data_ptr(), x.data_ptr(), gam.data_ptr(), eps, dx.data_ptr(), M, C, st) == -2
    assert _lib.fn(lib, "lr_layernorm_bwd_res", dt)(x.data_ptr(), x.data_ptr(), None, gam.data_ptr(), eps, dx.data_ptr(), M, C, st) == -2
    torch.cuda.synchronize()
    assert torch.all(dx == 7.0)


# =====================================================================================================================
# 4. Attention backward
# =====================================================================================================================
def _attn_inputs(tag, dt, B, heads, Nq, Nkv, spike=False):
    C = heads * 64
    q, k, v, do = (r16(G.T(f"{tag}.{n}", (B, s, C)), dt) for n, s in (("q", Nq), ("k", Nkv), ("v", Nkv), ("do", Nq)))
    if spike:
        k[0, 450] = r16(q[0, 7] * 6.0, dt)
        k[0, 70] = r16(q[0, 300] * 4.0, dt)
    return q, k, v, do


def _attn_reference(q, k, v, do, B, heads, Nq, Nkv):
    C = heads * 64
    qr, kr, vr = (t_.clone().requires_grad_(True) for t_ in (q, k, v))

    def split(t_, n):
        return t_.reshape(B, n, heads, 64).permute(0, 2, 1, 3)

    o = F.scaled_dot_product_attention(split(qr, Nq), split(kr, Nkv), split(vr, Nkv), scale=0.125)
    o.permute(0, 2, 1, 3).reshape(B, Nq, C).backward(do)
    return qr.grad, kr.grad, vr.grad


def _attn_run(dt, q, k, v, do, B, heads, Nq, Nkv):
    """T.attention on column slices of fused buffers (q alone; [k | v]); returns dq, dk, dv on the device."""
    from leftrefill_amd import train_ops as T
    d = dev()
    C = heads * 64
    qd = q.reshape(B * Nq, C).to(dt).to(d).requires_grad_(True)
    kv = torch.cat([k, v], -1).reshape(B * Nkv, 2 * C).to(dt).to(d).requires_grad_(True)
    T.attention(qd, kv[:, :C], kv[:, C:], B, heads, Nq, Nkv, 0.125).backward(do.reshape(B * Nq, C).to(dt).to(d))
    return qd.grad.reshape(B, Nq, C), kv.grad[:, :C].reshape(B, Nkv, C), kv.grad[:, C:].reshape(B, Nkv, C)


def _check_attn(tag, dt, got, ref):
    for n, a_, r_ in zip(("dq", "dk", "dv"), got, ref):
        check(f"{tag} {n}", a_, r_, dt, attn=True)


ATTN_SPLIT_CASES = [
    # 2 slices of 5 and 4 tiles; two key blocks, the second with a 72-key tail; B * heads = 6 in the workspace index
    (2, 3, 576, 200, dict(q_splits=2, t_per=5, slices=[(0, 5), (5, 9)], kblocks=2)),
    # 41 tiles, 10 slices of 5: slice 8 holds only the 40-query tail tile, slice 9 is empty (and must still write zero partials)
    (1, 1, 2600, 77, dict(q_splits=10, t_per=5, slices=[(5 * i, 5 * i + 5) for i in range(8)] + [(40, 41), (45, 41)], kblocks=1)),
    # the benchmark's block count (80): 2 slices
    (16, 5, 512, 77, dict(q_splits=2, t_per=4, slices=[(0, 4), (4, 8)], kblocks=1)),
]


@both_types
@pytest.mark.parametrize("B,heads,Nq,Nkv,regime", ATTN_SPLIT_CASES, ids=["uneven_2kblk", "tail_only_and_empty", "bench_blocks"])
def test_attention_backward_query_split_regimes(dt, monkeypatch, B, heads, Nq, Nkv, regime):
    """The query-split dK / dV kernel vs float64 autograd, and the same call with the split switched off: dQ is bit-identical between the two
    (the split does not touch its kernel), dK / dV of both meet the same reference bound -- a split bug shows in the first run only."""
    from leftrefill_amd import train_ops as T
    qs = T.attn_bwd_q_splits(B, heads, Nq, Nkv)
    ntiles, t_per, slices = attn_bwd_slices(Nq, qs)
    print(f"[regime attn {B}x{heads}x{Nq}x{Nkv}] blocks {B * heads * ((Nkv + 127) // 128)} q_splits {qs} tiles {ntiles} t_per {t_per} slices {slices}")
    assert (qs, t_per, slices, (Nkv + 127) // 128) == (regime["q_splits"], regime["t_per"], regime["slices"], regime["kblocks"])
    if Nq == 2600:
        assert slices[8] == (40, 41) and Nq - 40 * 64 == 40 and slices[9][0] >= ntiles       # tail tile alone; empty slice
    if B == 16:
        assert B * heads * ((Nkv + 127) // 128) == 80
    tag = f"attr.{Nq}.{Nkv}.{heads}"
    q, k, v, do = _attn_inputs(tag, dt, B, heads, Nq, Nkv)
    ref = _attn_reference(q, k, v, do, B, heads, Nq, Nkv)
    got = _attn_run(dt, q, k, v, do, B, heads, Nq, Nkv)
    monkeypatch.setattr(T, "ATTN_BWD_QSPLIT", False)
    assert T.attn_bwd_q_splits(B, heads, Nq, Nkv) == 1
    got1 = _attn_run(dt, q, k, v, do, B, heads, Nq, Nkv)
    dq_same = torch.equal(got[0], got1[0])
    print(f"[bwd {tag}] dq bit-identical with / without the query split: {dq_same}; "
          f"max |dk split - dk unsplit| {(got[1].float() - got1[1].float()).abs().max().item():.3e}")
    _check_attn(tag + " unsplit", dt, got1, ref)
    _check_attn(tag + " split", dt, got, ref)
    assert dq_same


@pytest.mark.parametrize("B,heads,Nq,Nkv", [(1, 3, 300, 200), (2, 5, 256, 77)])
def test_attention_backward_tail_shapes_bf16(B, heads, Nq, Nkv):
    """The query / key tail shapes of test_attention_backward, in bf16."""
    tag = f"attb.{Nq}.{Nkv}.{heads}"
    q, k, v, do = _attn_inputs(tag, BF, B, heads, Nq, Nkv)
    _check_attn(tag, BF, _attn_run(BF, q, k, v, do, B, heads, Nq, Nkv), _attn_reference(q, k, v, do, B, heads, Nq, Nkv))


def test_attention_backward_with_late_score_spike_bf16():
    """test_attention_backward_with_late_score_spike in bf16: deferred running-max rescale + saved log-sum-exp."""
    q, k, v, do = _attn_inputs("attbs", BF, 1, 1, 512, 512, spike=True)
    _check_attn("spike", BF, _attn_run(BF, q, k, v, do, 1, 1, 512, 512), _attn_reference(q, k, v, do, 1, 1, 512, 512))


def _attn_direct(dt, qd, kd, vd, out, lse, dout, B, heads, Nq, Nkv, ld_qt, ws_ptr, fill=7.0):
    """lr_attention_bwd through the C ABI with the struct filled as train_ops._attention_backward fills it, except for the query split
    (ld_qt, qt).  Outputs and the D scratch are pre-filled with `fill`."""
    from leftrefill_amd import _lib
    lib = _lib.load()
    C = heads * 64
    dq = torch.full((B * Nq, C), fill, device=qd.device, dtype=dt)
    dk = torch.full((B * Nkv, C), fill, device=qd.device, dtype=dt)
    dv = torch.full((B * Nkv, C), fill, device=qd.device, dtype=dt)
    dsum = torch.full_like(lse, fill)
    a = _lib.AttnBwdArgs()
    a.q, a.k, a.v, a.o, a.dout = qd.data_ptr(), kd.data_ptr(), vd.data_ptr(), out.data_ptr(), dout.data_ptr()
    a.qt, a.kt, a.dot, a.lse, a.dsum = ws_ptr, 0, 0, lse.data_ptr(), dsum.data_ptr()
    a.dq, a.dk, a.dv = dq.data_ptr(), dk.data_ptr(), dv.data_ptr()
    a.ldq, a.ldk, a.ldv, a.ldo, a.lddo = qd.stride(0), kd.stride(0), vd.stride(0), out.stride(0), dout.stride(0)
    a.ld_qt, a.ld_kt = ld_qt, 0
    a.lddq, a.lddk, a.lddv = dq.stride(0), dk.stride(0), dv.stride(0)
    a.B, a.heads, a.Nq, a.Nkv, a.scale = B, heads, Nq, Nkv, 0.125
    rc = _lib.fn(lib, "lr_attention_bwd_f16", dt)(a, ctypes.c_void_p(torch.cuda.current_stream().cuda_stream))
    torch.cuda.synchronize()
    return rc, dq, dk, dv, dsum


@both_types
def test_attention_backward_c_abi_query_split_arguments(dt):
    """ld_qt = 64 (one tile per slice, 55 empty slices) with a workspace of the documented size gives dK / dV within the reference bound, like
    the front end's 2 slices; ld_qt = 65 and a workspace that is not 16-byte aligned return LR_E_ARG and launch NOTHING (dQ runs first: the
    arguments of the later dK / dV launch are validated before it)."""
    from leftrefill_amd import train_ops as T
    B, heads, Nq, Nkv = 2, 3, 576, 200
    C, kblocks = heads * 64, (Nkv + 127) // 128
    ntiles, t_per, slices = attn_bwd_slices(Nq, 64)
    assert t_per == 1 and ntiles == 9 and all(t0 >= ntiles for t0, _ in slices[9:]) and T.attn_bwd_q_splits(B, heads, Nq, Nkv) == 2
    tag = f"attr.{Nq}.{Nkv}.{heads}"
    q, k, v, do = _attn_inputs(tag, dt, B, heads, Nq, Nkv)
    ref = _attn_reference(q, k, v, do, B, heads, Nq, Nkv)
    d = dev()
    qd = q.reshape(B * Nq, C).to(dt).to(d)
    kv = torch.cat([k, v], -1).reshape(B * Nkv, 2 * C).to(dt).to(d)
    kd, vd = kv[:, :C], kv[:, C:]
    dout = do.reshape(B * Nq, C).to(dt).to(d)
    out, lse = T._attention_forward(qd, kd, vd, B, heads, Nq, Nkv, 0.125)
    ws = torch.empty(64 * B * heads * kblocks * 2 * 128 * 64 + 4, device=d, dtype=torch.float32)
    assert ws.data_ptr() % 16 == 0
    rc, dq, dk, dv, _ = _attn_direct(dt, qd, kd, vd, out, lse, dout, B, heads, Nq, Nkv, 64, ws.data_ptr())
    assert rc == 0
    _check_attn(tag + " ld_qt=64", dt, [t_.reshape(B, -1, C) for t_ in (dq, dk, dv)], ref)
    fe = [torch.empty_like(t_) for t_ in (dq, dk, dv)]
    T._attention_backward(qd, kd, vd, out, lse, dout, (B, heads, Nq, Nkv, 0.125), *fe)
    _check_attn(tag + " front end", dt, [t_.reshape(B, -1, C) for t_ in fe], ref)
    assert torch.equal(fe[0], dq)
    for what, ld_qt, ptr in (("ld_qt = 65", 65, ws.data_ptr()), ("workspace + 8 bytes", 2, ws.data_ptr() + 8)):
        rc, dq, dk, dv, dsum = _attn_direct(dt, qd, kd, vd, out, lse, dout, B, heads, Nq, Nkv, ld_qt, ptr)
        untouched = [bool(torch.all(t_ == 7.0)) for t_ in (dq, dk, dv, dsum)]
        print(f"[bwd attention C ABI] {what}: rc {rc}, dq / dk / dv / D untouched {untouched}")
        assert rc == -1, what
        assert all(untouched), (what, untouched)


# =====================================================================================================================
# 5. GEGLU past the grid-stride wrap
# =====================================================================================================================
@both_types
def test_geglu_forward_backward_past_grid_wrap(dt):
    """M * H / 8 work items > 65536 blocks x 256 threads: the second trip of the grid-stride loop of geglu_fwd_kernel / geglu_bwd_kernel.  The
    one-call result equals, bit for bit, the calls on row slices far below the wrap, and matches float64 autograd on the first rows, the last
    rows and the rows around the wrap."""
    from leftrefill_amd import train_ops as T
    d = dev()
    H, M = 1280, 104960
    total, grid = geglu_grid(M, H)
    assert M % 128 == 0 and total > grid == 65536 * 256 and geglu_grid(M - 128, H)[0] <= grid      # the smallest such multiple of 128
    assert max(geglu_grid(32768, H)[0], geglu_grid(M % 32768, H)[0]) < grid
    wrap = grid * 8 // H
    assert 32 <= wrap < M - 32
    # inputs on the device: a block of rows tiled with a per-tile rotation, so no two tiles line up
    RB = 2048
    pre_b = G.T("ggr.pre", (RB, 2 * H)).to(dt).to(d)
    dy_b = G.T("ggr.dy", (RB, H)).to(dt).to(d)
    pre = torch.empty(M, 2 * H, device=d, dtype=dt)
    dy = torch.empty(M, H, device=d, dtype=dt)
    for i, r0 in enumerate(range(0, M, RB)):
        n = min(RB, M - r0)
        pre[r0:r0 + n] = torch.roll(pre_b, 131 * i, 0)[:n]
        dy[r0:r0 + n] = torch.roll(dy_b, 89 * i, 0)[:n]
    out = T.geglu_fwd(pre)
    dpre = T.geglu_bwd(pre, dy)
    # 1. bit for bit against calls that never wrap
    for r0 in range(0, M, 32768):
        r1 = min(M, r0 + 32768)
        assert torch.equal(T.geglu_fwd(pre[r0:r1]), out[r0:r1]), ("out", r0)
        assert torch.equal(T.geglu_bwd(pre[r0:r1], dy[r0:r1]), dpre[r0:r1]), ("dpre", r0)
    # 2. float64 autograd on three row windows; pre is packed in 16-column groups [u16 | g16 | u16 | g16 ...]
    for name, r0 in (("first rows", 0), ("last rows", M - 64), ("wrap rows", wrap - 32)):
        pr = pre[r0:r0 + 64].cpu().double().requires_grad_(True)
        p4 = pr.reshape(64, H // 16, 2, 16)
        o = p4[:, :, 0].reshape(64, H) * F.gelu(p4[:, :, 1].reshape(64, H))
        o.backward(dy[r0:r0 + 64].cpu().double())
        check(f"geglu {name} out", out[r0:r0 + 64], o.detach(), dt)
        g4 = pr.grad.reshape(64, H // 16, 2, 16)
        d4 = dpre[r0:r0 + 64].reshape(64, H // 16, 2, 16)
        check(f"geglu {name} du", d4[:, :, 0], g4[:, :, 0], dt)
        check(f"geglu {name} dg", d4[:, :, 1], g4[:, :, 1], dt)
    del pre, dy, out, dpre, pre_b, dy_b
    torch.cuda.empty_cache()


# =====================================================================================================================
# 6. Exact kernels, called directly
# =====================================================================================================================
@both_types
@pytest.mark.parametrize("N,H,W,C", [(3, 5, 7, 320), (1, 1, 1, 8), (2, 4, 6, 1288)])
def test_sumpool2x2_exact(dt, N, H, W, C):
    """The fp32 sum of the four fine pixels in the kernel's order ((x00 + x01) + x10) + x11, rounded once: bit equality."""
    from leftrefill_amd import train_ops as T
    x = G.T(f"spr.{H}.{W}.{C}", (N, 2 * H, 2 * W, C)).to(dt)
    xf = x.float()
    exp = (((xf[:, 0::2, 0::2] + xf[:, 0::2, 1::2]) + xf[:, 1::2, 0::2]) + xf[:, 1::2, 1::2]).to(dt)
    y = T.sumpool2x2(x.reshape(-1, C).contiguous().to(dev()), N, H, W)
    assert y.dtype == dt and y.shape == (N * H * W, C)
    diff = (y.float().cpu().reshape(exp.shape) - exp.float()).abs().max().item()
    print(f"[bwd sumpool2x2 {N}x{H}x{W}x{C}] rel_l2 {diff / exp.float().norm().item():.3e} max_abs {diff:.3e}")
    assert torch.equal(y.cpu().reshape(exp.shape), exp)


@both_types
@pytest.mark.parametrize("b,v,s,C", [(2, 4, 4, 64), (1, 1, 3, 320)])
def test_mv_gather_scatter_backward_exact(dt, b, v, s, C):
    """lr_mv_gather_bwd / lr_mv_scatter_bwd vs autograd of unet_ref.mv_gather / mv_scatter: every position bit-exact; the shared target slot is
    the fp32 sum over canvases 0..v-1 in that order, rounded once; the right halves that received nothing are exactly +0."""
    from leftrefill_amd import train_ops as T
    d = dev()
    V = v + 1
    # gather: x [b*v, 2 s s, C] -> seq [b, V s s, C]
    x = r16(G.T(f"mvr.x.{v}.{s}", (b * v, 2 * s * s, C)), dt)
    dseq = r16(G.T(f"mvr.dseq.{v}.{s}", (b, V * s * s, C)), dt)
    xr = x.clone().requires_grad_(True)
    seq_ref, info = unet_ref.mv_gather(xr, V, True, False)
    seq_ref.backward(dseq)
    xd = x.reshape(-1, C).to(dt).to(d).requires_grad_(True)
    seq = T.mv_gather(xd, b, v, s)
    assert torch.equal(seq.detach().cpu().reshape(seq_ref.shape), seq_ref.detach().to(dt))
    seq.backward(dseq.reshape(-1, C).to(dt).to(d))
    got = xd.grad.cpu().reshape(b, v, s, 2 * s, C)
    exp = xr.grad.to(dt).reshape(b, v, s, 2 * s, C)
    err = (got.double() - exp.double()).abs()
    print(f"[bwd mv_gather {b}.{v}.{s}.{C}] rel_l2 {(err.norm() / exp.double().norm()).item():.3e} max_abs {err.max().item():.3e}")
    assert torch.equal(got, exp)
    assert not got[:, 1:, :, s:].contiguous().view(torch.int16).any()             # (bit pattern 0x0000: +0, not -0)
    # scatter: seq [b, V s s, C] -> x [b*v, 2 s s, C]
    sq = r16(G.T(f"mvr.seq.{v}.{s}", (b, V * s * s, C)), dt)
    dx = r16(G.T(f"mvr.dx.{v}.{s}", (b * v, 2 * s * s, C)), dt)
    sr = sq.clone().requires_grad_(True)
    back_ref = unet_ref.mv_scatter(sr, V, True, False, info)
    back_ref.backward(dx)
    sd = sq.reshape(-1, C).to(dt).to(d).requires_grad_(True)
    back = T.mv_scatter(sd, b, v, s)
    assert torch.equal(back.detach().cpu().reshape(back_ref.shape), back_ref.detach().to(dt))
    back.backward(dx.reshape(-1, C).to(dt).to(d))
    got = sd.grad.cpu().reshape(b, V, s, s, C)
    exp = sr.grad.to(dt).reshape(b, V, s, s, C).clone()
    acc = torch.zeros(b, s, s, C, dtype=torch.float32)
    for cv in range(v):                                                             # the kernel's order: canvases 0..v-1, fp32
        acc = acc + dx.float().reshape(b, v, s, 2 * s, C)[:, cv, :, s:]
    target = acc.to(dt)
    err = (got.double() - exp.double()).abs()
    print(f"[bwd mv_scatter {b}.{v}.{s}.{C}] rel_l2 {(err.norm() / exp.double().norm()).item():.3e} max_abs {err.max().item():.3e}; "
          f"target slot: fp32 ordered sum == float64 sum rounded once at {(target == exp[:, 0]).float().mean().item():.4f} of the elements")
    assert torch.equal(got[:, 1:], exp[:, 1:])
    assert torch.equal(got[:, 0], target)
