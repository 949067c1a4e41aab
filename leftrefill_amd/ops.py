"""Torch-tensor front end of the C ABI: shape/dtype checks, output allocation, current-stream plumbing.

PyTorch is used only for device memory and streams (`torch.cuda.current_stream()` is the HIP stream on ROCm).
Activations are NHWC / token-major fp16: a tensor [M, C] with M = N*H*W rows.
"""
import ctypes
import os

import torch

from . import _lib
from ._lib import FfnArgs, GemmArgs, RowlinArgs, StinArgs, XattnArgs

GN_CHUNKS = 256
# per-group GroupNorm partials from the producers' epilogues (no lr_groupnorm_finalize launch); LEFTREFILL_GN_GROUPS=0 keeps the
# per-channel partials + finalize for every GroupNorm
GN_GROUPS = os.environ.get("LEFTREFILL_GN_GROUPS", "1") != "0"

# ---- tile plan of lr_gemm_conv_f16 ----------------------------------------------------------------------------------
# The UNet has ~60 distinct static GEMM shapes.  Their (tile_m, tile_n, splits) come from an IN-TREE table
# (tile_table.json, produced on an MI355X by tools/tune_tiles.py and committed): the plan is a pure function of the
# shape, identical in every process and on every rank, so results are bit-reproducible across runs (the split-K factor
# changes fp32 rounding) and the replicated rows of the sharded multi-view path are bit-identical on every rank.
# Shapes missing from the table use the library's static heuristic (also a pure function of the shape).
# LEFTREFILL_AUTOTUNE=1 is a developer mode: unknown shapes are timed on first sight and added to the in-memory table
# (dump it with tile_cache()); it is never on by default.
AUTOTUNE = os.environ.get("LEFTREFILL_AUTOTUNE", "0") == "1"
# (tile_m, tile_n, pipe): pipe 0 = the tile's standard instance; 4 = the 8-wave 4-stage one-block-per-CU 128-row instance
# (lr_gemm_args.pipe)
# 8 = LR_PIPE_HALO: the halo-tile 3x3 conv (16 x 16 pixel tiles, input patch resident in LDS; refused for every other kind of call)
TILE_CANDIDATES = ((128, 64, 0), (128, 128, 0), (128, 160, 0), (128, 128, 4), (128, 160, 4), (256, 128, 0), (256, 160, 0),
                   (256, 256, 0), (256, 320, 0), (256, 160, 8), (256, 320, 8))
TILE_TABLE_PATH = os.environ.get("LEFTREFILL_TILE_TABLE_PATH",      # (developer override: A/B of a freshly tuned table)
                                 os.path.join(os.path.dirname(os.path.abspath(__file__)), "tile_table.json"))
_tile_cache = None
PLAN_LOG = os.environ.get("LEFTREFILL_PLAN_LOG", "0") == "1"
# lr_gemm_args.splitk_mode: 1 = split-K partials reduced inside the GEMM launch where the plan allows it (every K-slice block resident
# at once), 0 = by the separate fixed-order reduce launch
SPLITK_MODE = int(os.environ.get("LEFTREFILL_SPLITK_MODE", "0"))      # (1 needs a developer build of the library)
_untabulated = set()
# shape keys of the GEMM calls since the sets were last cleared, by whether the in-tree table knew them (bench.py batch_sensitivity)
TABLE_HITS, TABLE_MISSES = set(), set()
# developer hooks of tools/tune_in_step.py (None in the product): PLAN_TRIAL maps a table key to the (tile_m, tile_n, splits, pipe) to try
# instead of the table's plan (splits 0 = the library's static choice for that tile; a plan the library refuses falls back to the table's);
# LAUNCH_HOOK(key, phase, plan) is called right before (0) and after (1) the launch
PLAN_TRIAL = None
LAUNCH_HOOK = None


# Plan GEMMs as if the batch were `scale` times larger (the shared prefix of a CFG batch runs on half the samples but must
# form every partial sum exactly like the full batch would: same tile, same split-K, same statistics partials).
_PLAN_BATCH_SCALE = [1]


class plan_batch_scale:
    def __init__(self, scale):
        self.scale = int(scale)

    def __enter__(self):
        self.prev = _PLAN_BATCH_SCALE[0]
        _PLAN_BATCH_SCALE[0] = self.scale

    def __exit__(self, *exc):
        _PLAN_BATCH_SCALE[0] = self.prev


def tile_key(M, N, K, taps=1, stride=1, up=0, geglu=False, concat=False, asym=False, gelu=False, ln=False, stats=False):
    return "%d,%d,%d,%d,%d,%d,%d,%d,%d,%d,%d,%d" % (M, N, K, taps, stride, up, int(geglu), int(concat), int(asym),
                                                      int(gelu), int(ln), int(stats))


def tile_cache():
    """shape key -> [tile_m, tile_n, splits]; loaded once from the in-tree table."""
    global _tile_cache
    if _tile_cache is None:
        _tile_cache = {}
        if os.path.exists(TILE_TABLE_PATH) and os.environ.get("LEFTREFILL_TILE_TABLE", "1") != "0":
            import json
            with open(TILE_TABLE_PATH) as f:
                _tile_cache = {k: tuple(v) for k, v in json.load(f).items()}
    return _tile_cache


def _stream():
    return torch.cuda.current_stream().cuda_stream


def _p(t):
    return 0 if t is None else t.data_ptr()


HALF_TYPES = (torch.float16, torch.bfloat16)


def _chk16(t, name):
    assert t.is_cuda and t.dtype in HALF_TYPES and t.is_contiguous(), f"{name}: need contiguous cuda fp16 / bf16"


def _fn(lib, name, dtype):
    return _lib.fn(lib, name, dtype)


def nchw_to_nhwc(x1, x2=None, cpad=None, dtype=torch.float16):
    """[N,C1,H,W] fp32 (+ optional [N,C2,H,W]) -> [N*H*W, cpad] fp16 (or bf16)."""
    lib = _lib.load()
    N, C1, H, W = x1.shape
    C2 = 0 if x2 is None else x2.shape[1]
    cpad = cpad or ((C1 + C2 + 7) // 8) * 8
    x1 = x1.float().contiguous()
    x2 = None if x2 is None else x2.float().contiguous()
    y = torch.empty(N * H * W, cpad, device=x1.device, dtype=dtype)
    _lib.check(_fn(lib, "lr_nchw_f32_to_nhwc_f16", dtype)(_p(x1), C1, _p(x2), C2, _p(y), cpad, N, H, W, _stream()), "nchw_to_nhwc")
    return y


def nhwc_to_nchw(y, N, H, W, C, out_dtype=None):
    """[N*H*W, >=C] -> [N,C,H,W] in out_dtype: float32, or the 16-bit type of y (default)."""
    lib = _lib.load()
    _chk16(y, "y")
    out_dtype = y.dtype if out_dtype is None or out_dtype in HALF_TYPES else out_dtype
    out = torch.empty(N, C, H, W, device=y.device, dtype=out_dtype)
    _lib.check(_fn(lib, "lr_nhwc_f16_to_nchw", y.dtype)(_p(y), y.shape[-1], C, _p(out), int(out_dtype == torch.float32), N, H, W,
                                       _stream()), "nhwc_to_nchw")
    return out


def group_norm(x1, N, HW, gamma, beta, eps, silu, x2=None):
    """GroupNorm(32)(+SiLU) over the virtual concat [x1 | x2]; x* are [N*HW, C*] fp16 -> [N*HW, C1+C2] fp16."""
    lib = _lib.load()
    _chk16(x1, "x1")
    C1 = x1.shape[-1]
    C2 = 0
    if x2 is not None:
        _chk16(x2, "x2")
        C2 = x2.shape[-1]
    assert gamma.dtype == torch.float32 and beta.dtype == torch.float32 and gamma.numel() == C1 + C2
    partials = torch.empty(N * GN_CHUNKS * 64, device=x1.device, dtype=torch.float32)
    y = torch.empty(N * HW, C1 + C2, device=x1.device, dtype=x1.dtype)
    st = _stream()
    _lib.check(_fn(lib, "lr_groupnorm_stats", x1.dtype)(_p(x1), C1, _p(x2), C2, N, HW, _p(partials), st), "groupnorm_stats")
    _lib.check(_fn(lib, "lr_groupnorm_apply", x1.dtype)(_p(x1), C1, _p(x2), C2, N, HW, _p(partials), _p(gamma), _p(beta), float(eps),
                                      int(bool(silu)), _p(y), st), "groupnorm_apply")
    return y


def group_norm_fused(x1, N, HW, gamma, beta, eps, silu, gs1, x2=None, gs2=None):
    """GroupNorm(32)(+SiLU) whose statistics come from the producers' epilogues: gs* = (partials [M/R, C, 2] fp32, R) as
    returned by gemm_conv(..., want_gn_stats=True) for x1 / x2.  One tiny finalize launch replaces the pass over x."""
    lib = _lib.load()
    _chk16(x1, "x1")
    C1 = x1.shape[-1]
    C2 = 0 if x2 is None else x2.shape[-1]
    p1, r1 = gs1[:2]
    p2, r2 = gs2[:2] if x2 is not None else (None, 1)
    assert p1.shape == (N * HW // r1, C1, 2) and HW % r1 == 0
    if x2 is not None:
        _chk16(x2, "x2")
        assert p2.shape == (N * HW // r2, C2, 2) and HW % r2 == 0
    assert gamma.dtype == torch.float32 and beta.dtype == torch.float32 and gamma.numel() == C1 + C2
    partials = torch.empty(N * 64, device=x1.device, dtype=torch.float32)
    y = torch.empty(N * HW, C1 + C2, device=x1.device, dtype=x1.dtype)
    st = _stream()
    _lib.check(lib.lr_groupnorm_finalize(_p(p1), C1, r1, _p(p2), C2, r2, N, HW, _p(partials), st), "groupnorm_finalize")
    _lib.check(_fn(lib, "lr_groupnorm_apply_n", x1.dtype)(_p(x1), C1, _p(x2), C2, N, HW, _p(partials), 1, _p(gamma), _p(beta), float(eps),
                                        int(bool(silu)), _p(y), st), "groupnorm_apply_n")
    return y


def group_norm_groups(x1, N, HW, gamma, beta, eps, silu, gp, chunks):
    """GroupNorm(32)(+SiLU) of a single tensor whose per-GROUP (sum, sumsq) partials gp [N, chunks, 32, 2] came out of its producer's
    epilogue (gemm_conv / ffn_block `want_gn_stats`): ONE launch, the apply kernel reduces the chunks in its prologue."""
    lib = _lib.load()
    _chk16(x1, "x1")
    C1 = x1.shape[-1]
    assert gp.dtype == torch.float32 and gp.is_contiguous() and gp.shape == (N, chunks, 32, 2), (gp.shape, N, chunks)
    assert gamma.dtype == torch.float32 and beta.dtype == torch.float32 and gamma.numel() == C1
    y = torch.empty(N * HW, C1, device=x1.device, dtype=x1.dtype)
    _lib.check(_fn(lib, "lr_groupnorm_apply_n", x1.dtype)(_p(x1), C1, 0, 0, N, HW, _p(gp), chunks, _p(gamma), _p(beta), float(eps),
                                                          int(bool(silu)), _p(y), _stream()), "groupnorm_apply_n")
    return y


OUT_FUSED = os.environ.get("LEFTREFILL_OUT_FUSED", "1") != "0"   # the UNet's `out` block as one launch (lr_gn_conv_out_f16)


def gn_conv_out_ok(H, W, C, cout):
    """Shapes lr_gn_conv_out_f16 takes (anything else keeps GroupNorm -> conv -> layout conversion)."""
    return OUT_FUSED and 1 <= cout <= 4 and C % 64 == 0 and 64 <= C <= 704 and H % 8 == 0 and W % 16 == 0


def gn_conv_out(x, N, H, W, gamma, beta, eps, gp, chunks, w, bias, cout):
    """GroupNorm(32) + SiLU + 3x3 pad-1 conv to cout <= 4 channels + NHWC -> NCHW in one launch (the UNet's `out` block,
    reference openaimodel.py:714-718).  x [N*H*W, C] 16-bit tokens, gp [N, chunks, 32, 2] group partials of x from its producer,
    w [>= cout, 9*C] packed conv weight (k = tap * C + channel), bias fp32 | None -> [N, cout, H, W] in x's dtype."""
    lib = _lib.load()
    _chk16(x, "x")
    _chk16(w, "w")
    C = x.shape[1]
    assert x.shape[0] == N * H * W and gn_conv_out_ok(H, W, C, cout), (x.shape, N, H, W, cout)
    assert gp.dtype == torch.float32 and gp.is_contiguous() and gp.shape == (N, chunks, 32, 2), (gp.shape, N, chunks)
    assert gamma.dtype == torch.float32 and beta.dtype == torch.float32 and gamma.numel() == C and beta.numel() == C
    assert w.dtype == x.dtype and w.shape[0] >= cout and w.shape[1] == 9 * C and (bias is None or (bias.dtype == torch.float32 and bias.numel() >= cout))
    y = torch.empty(N, cout, H, W, device=x.device, dtype=x.dtype)
    _lib.check(_fn(lib, "lr_gn_conv_out_f16", x.dtype)(_p(x), N, H, W, C, _p(gp), chunks, _p(gamma), _p(beta), float(eps), _p(w), w.stride(0),
                                                       _p(bias), cout, _p(y), _stream()), "gn_conv_out")
    return y


def gn_fold_weights(gp, chunks, N, HW, gamma, beta, eps, w, bias):
    """Per-sample copies of a pointwise layer's weights with GroupNorm(32, affine) folded in (lr_gn_fold_weights_f16):
    w [Nout, C] 16-bit, bias [Nout] fp32 | None -> (w_b [N, Nout, C], bias_b [N, Nout] fp32); gp / chunks as in group_norm_groups."""
    lib = _lib.load()
    if not _lib.dev_variants():
        raise RuntimeError("lr_gn_fold_weights_f16 is compiled in developer builds only (tools/build_variant.sh)")
    _chk16(w, "w")
    Nout, C = w.shape
    assert gp.dtype == torch.float32 and gp.is_contiguous() and gp.shape == (N, chunks, 32, 2)
    wb = torch.empty(N, Nout, C, device=w.device, dtype=w.dtype)
    bb = torch.empty(N, Nout, device=w.device, dtype=torch.float32)
    _lib.check(_fn(lib, "lr_gn_fold_weights_f16", w.dtype)(_p(gp), chunks, N, HW, C, _p(gamma), _p(beta), float(eps), _p(w), _p(bias), Nout,
                                                           _p(wb), _p(bb), _stream()), "gn_fold_weights")
    return wb, bb


def layer_norm(x, gamma, beta, eps=1e-5):
    lib = _lib.load()
    _chk16(x, "x")
    M, C = x.shape
    y = torch.empty_like(x)
    _lib.check(_fn(lib, "lr_layernorm", x.dtype)(_p(x), _p(gamma), _p(beta), float(eps), _p(y), M, C, _stream()), "layernorm")
    return y


def timestep_embedding(t, dim, dtype=torch.float16):
    """t [N]: a floating-point t is embedded at its fp32 value (continuous-time samplers), any other dtype as int64."""
    lib = _lib.load()
    name = "lr_timestep_embedding_f32" if t.is_floating_point() else "lr_timestep_embedding"
    t = t.to(torch.float32 if t.is_floating_point() else torch.int64).contiguous()
    out = torch.empty(t.shape[0], dim, device=t.device, dtype=dtype)
    _lib.check(_fn(lib, name, dtype)(_p(t), t.shape[0], dim, _p(out), _stream()), "timestep_embedding")
    return out


def linear_small_m(a, w, bias, act_in=False, act_out=False):
    """a [M<=16, K] fp16, w [N, K] fp16, bias [N] fp32 or None -> [M, N] fp16."""
    lib = _lib.load()
    _chk16(a, "a")
    _chk16(w, "w")
    M, K = a.shape
    N = w.shape[0]
    out = torch.empty(M, N, device=a.device, dtype=a.dtype)
    st = _stream()
    for m0 in range(0, M, 16):   # the kernel keeps <= 16 rows in LDS; larger batches go in row chunks
        mc = min(16, M - m0)
        _lib.check(_fn(lib, "lr_linear_small_m", a.dtype)(a[m0:].data_ptr(), K, _p(w), _p(bias), out[m0:].data_ptr(), N, mc, N, K,
                                         int(act_in), int(act_out), st), "linear_small_m")
    return out


def gemm_conv(x1, wt, *, B, H, W, Hs=None, Ws=None, taps=1, stride=1, up=0, asym=False, x2=None, bias=None, rowvec=None,
              resid=None, geglu=False, gelu=False, out=None, tile_n=0, tile_m=0, splits=0, pipe=0, ln=None,
              want_stats=False, want_gn_stats=False, gn_hw=0, per_sample=False, wt_pm=False, skip=None):
    """Implicit-GEMM conv / linear (see lr_gemm_conv_f16).  x1 [B*Hs*Ws, C1] fp16, wt [N, taps*(C1+C2)] fp16.

    skip = (s1, s2 | None): pointwise K extension over the virtual concat [s1 | s2] at the output resolution -- wt is
    [N, 9 (C1 + C2) + Cs1 + Cs2], out = conv3x3([x1 | x2]) + W_s [s1 | s2] in one accumulation (lr_gemm_args.skip1: a ResBlock's
    skip_connection inside its last conv); bias must be the sum of the two layers' biases.

    ln = (stats [M, parts, 2] fp32, eps, colsum [N] fp32): LayerNorm folded into the GEMM (x1 is the raw input, wt / bias
    are the gamma / beta folded weights, see lr_gemm_args).  want_stats: also return the per-row (sum, sumsq) partials of
    the output, [M, parts, 2] fp32 -- the `stats` a following LayerNorm-folded GEMM consumes; returns (out, stats).
    want_gn_stats: also return per-channel (sum, sumsq) over row blocks for the GroupNorm that consumes the output:
    returns (out, (partials [M / R, N, 2] fp32, R, gp, chunks)), or (out, None) when R does not divide the rows of a sample
    (gn_hw, default H*W); gp [samples, chunks, 32, 2] = per-GROUP sums for a consumer that normalises this tensor alone
    (group_norm_groups: no finalize launch), None when the plan cannot produce them.
    per_sample: wt is [B, N, K] and bias [B, N] -- one weight set per sample (rows b*H*W .. of sample b), see ops.gn_fold_weights.
    up = 3, taps = 4: the phase form of the nearest-2x upsample + 3x3 conv -- wt is [4, N, 4 (C1 + C2)] (packing.pack_conv_up_phase), B / H / W
    the output grid and Hs / Ws the source grid as for up = 1; pipelined tiles only."""
    lib = _lib.load()
    _chk16(x1, "x1")
    _chk16(wt, "wt")
    Hs = H if Hs is None else Hs
    Ws = W if Ws is None else Ws
    C1 = x1.shape[-1]
    C2 = 0
    if x2 is not None:
        _chk16(x2, "x2")
        C2 = x2.shape[-1]
    if up == 3:
        assert wt.dim() == 3 and wt.shape[0] == 4 and wt.is_contiguous() and taps == 4 and H == 2 * Hs and W == 2 * Ws and not per_sample and not wt_pm
    if per_sample:
        assert wt.dim() == 3 and wt.shape[0] == B and taps == 1 and x2 is None and wt.is_contiguous() and not wt_pm
    if wt_pm:      # piece-major weights [K / 64, N, 64] (packing.pack_pm)
        assert wt.dim() == 3 and wt.shape[2] == 64 and wt.is_contiguous()
        Nw, Kw = wt.shape[1], wt.shape[0] * 64
    else:
        Nw, Kw = wt.shape[-2], wt.shape[-1]
    c16 = C1 == 16 and C2 == 0 and taps == 9 and Kw == 192      # 16-channel 3x3 source: K = 144 zero-padded to three K-steps
    Cs1 = Cs2 = 0
    if skip is not None:
        s1, s2 = skip
        _chk16(s1, "skip1")
        Cs1 = s1.shape[-1]
        if s2 is not None:
            _chk16(s2, "skip2")
            Cs2 = s2.shape[-1]
        assert stride == 1 and not up and s1.shape[0] == B * H * W and (s2 is None or s2.shape[0] == s1.shape[0])
    assert c16 or Kw == taps * (C1 + C2) + Cs1 + Cs2, (wt.shape, taps, C1, C2, Cs1, Cs2)
    if c16 and tile_m == 0 and tile_n == 0:
        # only the pipelined 256-row instances gather 16-channel taps
        tile_m, tile_n, splits = 256, (320 if Nw % 320 == 0 else 160 if Nw % 160 == 0 else 128), 1
    assert x1.shape[0] == B * Hs * Ws, (x1.shape, B, Hs, Ws)
    M = B * H * W
    n_out = Nw // 2 if geglu else Nw
    if out is None:
        out = torch.empty(M, n_out, device=x1.device, dtype=x1.dtype)
    a = GemmArgs()
    a.p1, a.C1, a.p2, a.C2 = _p(x1), C1, _p(x2), C2
    a.B, a.H, a.W, a.Hs, a.Ws = B, H, W, Hs, Ws
    a.taps, a.stride, a.up, a.asym = taps, stride, up, int(bool(asym))
    a.wt, a.N = _p(wt), Nw
    a.bias = _p(bias)
    if bias is not None:
        assert bias.dtype == torch.float32 and bias.numel() == (Nw * B if per_sample else Nw)
    a.rowvec, a.ld_rowvec = _p(rowvec), (rowvec.stride(0) if rowvec is not None else 0)
    a.resid, a.ld_resid = _p(resid), (resid.stride(0) if resid is not None else 0)
    if resid is not None:
        assert resid.shape[0] == M and resid.dtype == x1.dtype
    a.out, a.ld_out = _p(out), out.stride(0)
    assert not (geglu and gelu)
    a.geglu = 2 if gelu else int(geglu)      # 1: fused GEGLU, 2: plain erf-GELU epilogue
    a.tile_n = tile_n
    a.tile_m = tile_m
    a.splits = splits
    a.pipe = pipe
    a.workspace, a.workspace_bytes = 0, 0
    a.ln_stats, a.ln_parts, a.ln_eps, a.ln_colsum, a.stats_out, a.gn_stats_out = 0, 0, 0.0, 0, 0, 0
    a.gn_group_out, a.gn_hw = 0, int(gn_hw)
    a.wt_bstride, a.bias_bstride = (Nw * Kw, Nw if bias is not None else 0) if per_sample else (0, 0)
    a.wt_pm = int(bool(wt_pm))
    a.skip1, a.skip2, a.Cs1, a.Cs2 = (_p(skip[0]), _p(skip[1]), Cs1, Cs2) if skip is not None else (0, 0, 0, 0)
    a.splitk_mode = SPLITK_MODE
    assert wt.dtype == x1.dtype, (wt.dtype, x1.dtype)
    a.dtype = int(x1.dtype == torch.bfloat16)      # LR_DTYPE_F16 | LR_DTYPE_BF16
    if ln is not None:
        st_in, eps, colsum = ln
        assert st_in.dtype == torch.float32 and st_in.is_contiguous() and st_in.shape[0] == M and st_in.shape[2] == 2
        assert colsum.dtype == torch.float32 and colsum.numel() == Nw and taps == 1 and x2 is None
        a.ln_stats, a.ln_parts, a.ln_eps, a.ln_colsum = _p(st_in), st_in.shape[1], float(eps), _p(colsum)
    st = _stream()
    if tile_m == 0 and tile_n == 0 and splits == 0:
        scale = _PLAN_BATCH_SCALE[0]
        # (a conv with the pointwise extension is planned like the plain conv: the table knows that shape)
        key = tile_key(M * scale, Nw, Kw - Cs1 - Cs2, taps, stride, up, geglu, C2 > 0, asym, gelu, ln is not None, want_stats)
        plan = _choose_plan(lib, a, key, scale, x1.device, refine=skip is None and not per_sample and not c16, want_stats=want_stats)
        if plan is not None:
            a.tile_m, a.tile_n, a.splits, a.pipe = plan
    stats = None
    if want_stats:
        if a.splits == 0:
            a.splits = 1     # row statistics come out of the epilogue: no split-K
        parts = lib.lr_gemm_stats_parts(a)
        stats = torch.empty(M, parts, 2, device=x1.device, dtype=torch.float32)
        a.stats_out = _p(stats)
    if ln is not None and a.splits == 0:
        a.splits = 1
    gstats = None
    if want_gn_stats:
        a.splits = _lib_plan(lib, a)[2]     # pinned: the row-block size of the statistics depends on it (32 behind split-K)
        rows = lib.lr_gemm_gn_rows(a)
        hw = gn_hw or H * W
        # (phase form, statistics from the epilogue: the row blocks hold source pixels of one phase -- they must divide a sample's Hs * Ws)
        if (Hs * Ws if up == 3 and a.splits == 1 else hw) % rows == 0:                  # row blocks never straddle two samples
            chunks = lib.lr_gemm_gn_group_chunks(a) if GN_GROUPS else 0
            gp = torch.empty(M // hw, chunks, 32, 2, device=x1.device, dtype=torch.float32) if chunks > 0 else None
            gstats = (torch.empty((M + rows - 1) // rows, n_out, 2, device=x1.device, dtype=torch.float32), rows, gp, chunks)
            a.gn_stats_out = _p(gstats[0])
            a.gn_group_out = _p(gp)
    ws = _workspace(lib, a, x1.device)
    if LAUNCH_HOOK is not None and tile_m == 0 and tile_n == 0 and splits == 0:
        LAUNCH_HOOK(key, 0, _lib_plan(lib, a))
        rc = lib.lr_gemm_conv_f16(a, st)
        LAUNCH_HOOK(key, 1, rc)
        if rc != 0 and PLAN_TRIAL is not None and PLAN_TRIAL.get(key) is not None:      # the trial plan is not one this call can take
            PLAN_TRIAL[key] = None
            return gemm_conv(x1, wt, B=B, H=H, W=W, Hs=Hs, Ws=Ws, taps=taps, stride=stride, up=up, asym=asym, x2=x2, bias=bias, rowvec=rowvec,
                             resid=resid, geglu=geglu, gelu=gelu, out=out, ln=ln, want_stats=want_stats, want_gn_stats=want_gn_stats, gn_hw=gn_hw,
                             per_sample=per_sample, wt_pm=wt_pm, skip=skip)
        _lib.check(rc, "gemm_conv")
    else:
        _lib.check(lib.lr_gemm_conv_f16(a, st), "gemm_conv")
    if want_gn_stats:
        return out, gstats
    return (out, stats) if want_stats else out


# untabulated shapes: refine the library's static plan (LEFTREFILL_HEURISTIC_REFINE=0: take it as is)
HEURISTIC_REFINE = os.environ.get("LEFTREFILL_HEURISTIC_REFINE", "1") != "0"


def _lib_plan(lib, a):
    plan = (ctypes.c_int32 * 4)()
    lib.lr_gemm_plan(a, plan)
    return tuple(plan)


def _refine_plan(lib, a, act_epilogue):
    """The static heuristic's plan for `a`, with the two regularities of the in-step tuned table applied to 128-row tiles (round 6: with weights
    streamed from HBM the 2-stage 4-wave kernel loses to the 4-stage ring on every shape whose tiles fit the chip in one round, and 160-column
    tiles beat 128 where they divide N): tile_n 160 if N % 160 == 0, the 4-stage ring (pipe 4) if the tiles number <= 256.  A pure function of
    the shape like the table."""
    base = _lib_plan(lib, a)
    tm, tn = base[0], base[1]
    M = a.B * a.H * a.W
    if (a.taps == 9 and a.stride == 1 and a.up == 0 and not a.asym and not act_epilogue and not a.ln_stats and not a.stats_out and a.W % 16 == 0
            and a.H % 16 == 0 and a.Hs == a.H and a.Ws == a.W and a.N % 160 == 0 and M >= 8192 and (a.C1 + a.C2) % 64 == 0 and M < (1 << 28)):
        # third regularity: the 3x3 stride-1 convs of the large levels run on the halo-tile instance (input patch resident in LDS) -- 320-column
        # tiles where they still fill the chip
        tn = 320 if a.N % 320 == 0 and ((M + 255) // 256) * (a.N // 320) >= 200 else 160
        keep = (a.tile_m, a.tile_n, a.pipe)
        a.tile_m, a.tile_n, a.pipe = 256, tn, 8
        plan = _lib_plan(lib, a)
        a.tile_m, a.tile_n, a.pipe = keep
        return (256, tn, plan[2], 8)
    if tm != 128 or act_epilogue:
        return base
    if a.N % 160 == 0:
        tn = 160
    if tn not in (128, 160) or ((M + 127) // 128) * ((a.N + tn - 1) // tn) > 256:
        return base
    keep = (a.tile_m, a.tile_n, a.pipe)
    a.tile_m, a.tile_n, a.pipe = 128, tn, 4
    plan = _lib_plan(lib, a)                 # split-K factor of the refined tile
    a.tile_m, a.tile_n, a.pipe = keep
    return (128, tn, plan[2], 4)


def _static_plan(lib, a, tabulated, *, scale=1, act, refine=True, no_split=False, always=True):
    """The plan that is a pure function of the shape: the in-tree table's entry, else the library's static heuristic for the (scaled) batch,
    refined by what the in-step tuning of round 6 found on every small-M shape (_refine_plan); a caller of the C ABI without this front end
    gets the unrefined heuristic.  `a` has tile_m = tile_n = splits = 0 and comes back as it was.  always = False: None where the
    heuristic is the launch's business (an unscaled batch that is not refined, or one that the autotuner will time)."""
    refine = refine and HEURISTIC_REFINE
    if tabulated is not None or not (always or scale != 1 or (refine and not AUTOTUNE)):
        return tabulated
    a.B, a.splits = a.B * scale, int(no_split)      # (row statistics / the LayerNorm fold never split K)
    best = _refine_plan(lib, a, act) if refine else _lib_plan(lib, a)
    a.B, a.splits = a.B // scale, 0
    return best


def _choose_plan(lib, a, key, scale, device, *, refine, want_stats):
    """(tile_m, tile_n, splits, pipe) of a gemm_conv call that requests none, or None (the launch plans for itself).  In order: the table,
    the batch-scaled / refined heuristic, the autotuner, a trial plan, the halo guard, the skip fallback."""
    geglu, no_split = a.geglu == 1, bool(a.ln_stats) or want_stats
    hit = tile_cache().get(key)
    (TABLE_HITS if hit is not None else TABLE_MISSES).add(key)
    best = hit if hit is not None else _static_plan(lib, a, None, scale=scale, act=a.geglu != 0, refine=refine, no_split=no_split, always=False)
    if PLAN_LOG and hit is None and key not in _untabulated:      # developer aid: which shapes fall back to the static heuristic
        _untabulated.add(key)
        import sys
        print(f"[leftrefill] untabulated GEMM shape {key} (taps {a.taps}, H {a.H}, W {a.W}, skip {bool(a.skip1)})", file=sys.stderr, flush=True)
    if best is None and AUTOTUNE and not torch.cuda.is_current_stream_capturing():
        best = _tune_tiles(lib, a, device, geglu, no_split, want_stats)
        tile_cache()[key] = best
    if best is not None and PLAN_TRIAL is not None and PLAN_TRIAL.get(key) is not None:
        best = PLAN_TRIAL[key]
    if best is not None:
        M, pipe = a.B * a.H * a.W, best[3] if len(best) > 3 else 0
        # the table is keyed by M: the halo-tile instance needs 16 x 16 pixel tiles (or pairs of 8-line images; decided for the planned batch
        # AND this call), any other latent of the same size takes the tile's gather instance
        if pipe == 8 and (a.W % 16 or (a.H % 16 and not (a.H == 8 and M % 256 == 0 and (M * scale) % 256 == 0))):
            pipe = 0
        return best[0], best[1], best[2], pipe
    return _lib_plan(lib, a) if a.skip1 else None      # skip: ask the library, so that the tile is a pipelined one


def gemm_plan(M, N, K, **kw):
    """(tile_m, tile_n, splits, pipe) lr_gemm_conv_f16 uses for a shape: the in-tree table, else the static heuristic."""
    a = GemmArgs()
    a.B, a.H, a.W, a.N, a.taps, a.C1 = 1, 1, M, N, kw.get("taps", 1), K // kw.get("taps", 1)
    a.geglu = int(kw.get("geglu", False))
    best = _static_plan(_lib.load(), a, tile_cache().get(tile_key(M, N, K, **kw)), act=bool(kw.get("geglu") or kw.get("gelu")),
                        no_split=bool(kw.get("ln") or kw.get("stats")))
    return tuple(best[:3]) + (best[3] if len(best) > 3 and best[3] in (4, 8) else 0,)


def _workspace(lib, a, device):
    """split-K partials (small-M shapes); the caller owns the workspace."""
    a.workspace, a.workspace_bytes = 0, 0
    need = lib.lr_gemm_workspace_bytes(a)
    if need <= 0:
        return None
    ws = torch.empty(need // 4, device=device, dtype=torch.float32)
    a.workspace, a.workspace_bytes = ws.data_ptr(), need
    return ws


def _time_launch(lib, a, st, reps, rounds):
    t = float("inf")
    for _ in range(rounds):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(reps):
            lib.lr_gemm_conv_f16(a, st)
        e1.record()
        e1.synchronize()
        t = min(t, e0.elapsed_time(e1))
    return t


def _tune_tiles(lib, a, device, geglu, no_split, want_stats, reps=4, rounds=2):
    """Developer mode: time every (tile, split-K) configuration and return the fastest (tile_m, tile_n, splits)."""
    st = _stream()
    best, best_t = None, float("inf")
    for tm, tn, stg in TILE_CANDIDATES:
        if geglu and tn == 160:
            continue
        a.tile_m, a.tile_n, a.splits, a.pipe = tm, tn, 0, stg
        cands = {1} if no_split else {1, _lib_plan(lib, a)[2]}
        for sp in sorted(cands):
            a.splits = sp
            stats = None
            if want_stats:
                parts = lib.lr_gemm_stats_parts(a)
                stats = torch.empty(a.B * a.H * a.W, parts, 2, device=device, dtype=torch.float32)
                a.stats_out = stats.data_ptr()
            ws = _workspace(lib, a, device)
            if sp > 1 and ws is None:
                continue
            if lib.lr_gemm_conv_f16(a, st) != 0:
                continue
            t = _time_launch(lib, a, st, reps, rounds)
            del ws, stats
            if t < best_t:
                best, best_t = (tm, tn, sp, stg), t
    a.stats_out = 0
    return best


VT_MIN_KEYS = int(os.environ.get("LEFTREFILL_VT_MIN_KEYS", "1024"))   # pre-transpose V for key sequences at least this long
# 0 (default): V stays in its natural [key][d] layout (lr_attention_f16 gathers the PV fragments with the LDS transpose read of gfx950):
# no lr_transpose_v_f16 copy in front of long-sequence attention, no cached V^T of the context.  1: the round-1..3 path (pre-transposed,
# key-permuted V^T through lr_attention_vt_f16 from VT_MIN_KEYS keys up).  Measured (profiles/r04_attn_tr.txt): the kernel itself is
# 1-2 % slower on natural V, the copy it saves costs 11-18 us per launch -- 8192^2: 693 vs 681 + 18 us, 2048^2: 115 vs 113 + 13 us.
ATTN_VT = os.environ.get("LEFTREFILL_ATTN_VT", "0") != "0"


def transpose_v(v, B, heads, Nkv, out=None):
    """v [B*Nkv, >=heads*64] (row stride ldv) -> V^T [B, heads*64, pad64(Nkv)] in the attention kernel's key order."""
    lib = _lib.load()
    assert v.is_cuda and v.dtype in HALF_TYPES and v.stride(1) == 1
    ld = ((Nkv + 63) // 64) * 64
    vt = torch.empty(B, heads * 64, ld, device=v.device, dtype=v.dtype) if out is None else out
    assert vt.shape == (B, heads * 64, ld) and vt.is_contiguous()
    _lib.check(_fn(lib, "lr_transpose_v_f16", v.dtype)(_p(v), v.stride(0), _p(vt), ld, B, heads, Nkv, _stream()), "transpose_v")
    return vt


def attention(q, k, v, B, heads, Nq, Nkv, scale, out=None, vt=None):
    """q [B*Nq, >=heads*64] (row stride = ldq), k/v [B*Nkv, ...]; returns [B*Nq, heads*64] fp16.

    q/k/v may be column slices of a fused projection (strided rows, unit column stride).  vt: optional transpose_v(v) -- the
    pre-transposed-V kernel runs when it is given (or, with ATTN_VT, made here for long key sequences)."""
    lib = _lib.load()
    for t_ in (q, k, v):
        assert t_.is_cuda and t_.dtype == q.dtype and q.dtype in HALF_TYPES and t_.stride(1) == 1
    if out is None:
        out = torch.empty(B * Nq, heads * 64, device=q.device, dtype=q.dtype)
    if vt is None and ATTN_VT and Nkv >= VT_MIN_KEYS:
        vt = transpose_v(v, B, heads, Nkv)
    if vt is not None:
        _lib.check(_fn(lib, "lr_attention_vt_f16", q.dtype)(_p(q), q.stride(0), _p(k), k.stride(0), _p(vt), vt.shape[2], _p(out),
                                           out.stride(0), B, heads, Nq, Nkv, float(scale), _stream()), "attention_vt")
        return out
    _lib.check(_fn(lib, "lr_attention_f16", q.dtype)(_p(q), q.stride(0), _p(k), k.stride(0), _p(v), v.stride(0), _p(out), out.stride(0),
                                    B, heads, Nq, Nkv, float(scale), _stream()), "attention")
    return out


def attention_causal(q, k, v, B, heads, N, scale):
    """Causal self-attention (query i sees keys <= i), q/k/v [B*N, >=heads*64] strided column slices; the text tower."""
    lib = _lib.load()
    for t_ in (q, k, v):
        assert t_.is_cuda and t_.dtype == q.dtype and q.dtype in HALF_TYPES and t_.stride(1) == 1
    out = torch.empty(B * N, heads * 64, device=q.device, dtype=q.dtype)
    _lib.check(_fn(lib, "lr_attention_causal_f16", q.dtype)(_p(q), q.stride(0), _p(k), k.stride(0), _p(v), v.stride(0), _p(out), out.stride(0),
                                           B, heads, N, float(scale), _stream()), "attention_causal")
    return out


def attention_qkv(qkv, B, heads, L, scale):
    """Self-attention on the fused projection qkv [B*L, 3C] (q | k | v column blocks)."""
    C = heads * 64
    return attention(qkv[:, :C], qkv[:, C:2 * C], qkv[:, 2 * C:], B, heads, L, L, scale)


def attention_probe(q, k, cols, B, heads, Nq, Nkv, scale, out=None, alpha=1.0, beta=0.0):
    """lr_attention_probe_f16: out[b, i, c] = beta out[b, i, c] + alpha mean_h sum_j softmax_j(scale q_h[b,i] . k_h[b,j]) cols[j, c].

    q [B*Nq, >= heads*64], k [B*Nkv, >= heads*64]: 16-bit, strided rows, unit column stride (column slices of a fused projection, as
    `attention` takes them).  cols [Nkv, ncols <= 8] in q's dtype (any row stride), shared by samples and heads.  out: contiguous fp32
    [B, Nq, ncols], made here when None (then beta must be 0); with beta == 0 it is not read.  leftrefill_amd.attnprobe.probe_reference
    states the arithmetic."""
    lib = _lib.load()
    for t_ in (q, k, cols):
        assert t_.is_cuda and t_.dtype == q.dtype and q.dtype in HALF_TYPES and t_.dim() == 2 and t_.stride(1) == 1
    assert cols.shape[0] == Nkv, "cols: [Nkv, ncols]"
    ncols = cols.shape[1]
    if out is None:
        assert beta == 0.0, "beta != 0 needs the tensor to accumulate into"
        out = torch.empty(B, Nq, ncols, device=q.device, dtype=torch.float32)
    assert out.is_cuda and out.dtype == torch.float32 and out.is_contiguous() and out.numel() == B * Nq * ncols, "out: fp32 [B, Nq, ncols]"
    _lib.check(_fn(lib, "lr_attention_probe_f16", q.dtype)(_p(q), q.stride(0), _p(k), k.stride(0), _p(cols), cols.stride(0), ncols, _p(out),
                                                          B, heads, Nq, Nkv, float(scale), float(alpha), float(beta), _stream()),
               "attention_probe")
    return out


def attention_q_kv(q, kv, B, heads, Nq, Nkv, scale, vt=None):
    """Cross-attention: q [B*Nq, C], fused context projection kv [B*Nkv, 2C] (k | v column blocks); vt: optional cached
    transpose_v of the v block (the context is constant over the DDIM steps)."""
    C = heads * 64
    return attention(q, kv[:, :C], kv[:, C:], B, heads, Nq, Nkv, scale, vt=vt)


XATTN_C, XATTN_ROWS, XATTN_MAX_KEYS = 320, 128, 96
# widths lr_xattn_block_f16 has an instance for -> rows per block (C = 640: the 64-row / 4-wave instance of xattn_block640.hip)
XATTN_WIDTHS = {320: 128, 640: 64}
# LEFTREFILL_XATTN_WIDE=0 keeps the to_q -> attention -> to_out launches at C = 640
XATTN_WIDE = os.environ.get("LEFTREFILL_XATTN_WIDE", "1") != "0"


def xattn_ok(M, HW, C, heads, Lc):
    """Shapes lr_xattn_block_f16 takes (everything else keeps the to_q -> attention -> to_out path)."""
    rows = XATTN_WIDTHS.get(C)
    if rows is None or (C != XATTN_C and not XATTN_WIDE):
        return False
    return heads * 64 == C and M % rows == 0 and HW % rows == 0 and 0 < Lc <= XATTN_MAX_KEYS


def xattn_pack_vt(v, B, heads, Lc, out=None):
    """v [B*Lc, >= heads*64] (V projection of the context, unit column stride) -> V^T pack [B, heads, 2, 64, 64]."""
    lib = _lib.load()
    assert v.is_cuda and v.dtype in HALF_TYPES and v.stride(1) == 1 and v.shape[0] == B * Lc
    vt = torch.empty(B, heads, 2, 64, 64, device=v.device, dtype=v.dtype) if out is None else out
    assert vt.shape == (B, heads, 2, 64, 64) and vt.is_contiguous()
    _lib.check(_fn(lib, "lr_xattn_pack_vt_f16", v.dtype)(_p(v), v.stride(0), _p(vt), B, heads, Lc, _stream()), "xattn_pack_vt")
    return vt


def xattn_block(x, wq, bq, k, vt, wo, bo, *, HW, heads, Lc, eps, scale, want_stats=False, out=None, pre=None):
    """x + to_out(attention(LayerNorm(x) Wq, K, V)) in one launch (lr_xattn_block_f16).  wq / bq: LayerNorm-folded to_q;
    k [B*Lc, ld] = context projection with packing.pack_xattn's row order; vt = xattn_pack_vt(V); wo: packing.pack_pieces(to_out).
    pre = (a, Wo1, bo1): also fuses the preceding self-attention's out-projection, x1 = a Wo1^T + bo1 + x (wq: xattn_perm columns).
    Returns out [M, C] (, stats [M, 1, 2] for the LayerNorm fold of the next GEMM)."""
    lib = _lib.load()
    _chk16(x, "x")
    M, C = x.shape
    assert xattn_ok(M, HW, C, heads, Lc), (M, HW, C, heads, Lc)
    assert wq.dtype == x.dtype and wq.is_contiguous() and wq.shape == (C, C)
    assert wo.dtype == x.dtype and wo.is_contiguous() and wo.shape == (heads, C, 64)
    assert bq.dtype == torch.float32 and bo.dtype == torch.float32 and bq.numel() == C and bo.numel() == C
    assert k.dtype == x.dtype and k.stride(1) == 1 and k.shape[0] == (M // HW) * Lc and vt.dtype == x.dtype and vt.is_contiguous()
    if out is None:
        out = torch.empty_like(x)
    assert out.shape == x.shape and out.dtype == x.dtype and out.is_contiguous() and out.device == x.device
    stats = torch.empty(M, 1, 2, device=x.device, dtype=torch.float32) if want_stats else None
    a = XattnArgs()
    a.x, a.out, a.wq, a.bq, a.k, a.ldk, a.vt, a.wo, a.bo = _p(x), _p(out), _p(wq), _p(bq), _p(k), k.stride(0), _p(vt), _p(wo), _p(bo)
    a.stats_out = _p(stats)
    a.M, a.HW, a.C, a.heads, a.Lc, a.ln_eps, a.scale = M, HW, C, heads, Lc, float(eps), float(scale)
    a.pre_a = a.pre_w = a.pre_b = 0
    if pre is not None:
        # (a_self, Wo1, bo1): x1 = a_self Wo1^T + bo1 + x runs in front, in the same launch; wq then has pi-ordered COLUMNS
        pa_, pw_, pb_ = pre
        _chk16(pa_, "pre_a")
        assert pa_.shape == (M, C) and pw_.dtype == x.dtype and pw_.is_contiguous() and pw_.shape == (C, C)
        assert pb_.dtype == torch.float32 and pb_.numel() == C
        a.pre_a, a.pre_w, a.pre_b = _p(pa_), _p(pw_), _p(pb_)
    _lib.check(_fn(lib, "lr_xattn_block_f16", x.dtype)(a, _stream()), "xattn_block")
    return (out, stats) if want_stats else out


STIN_C, STIN_ROWS = 320, 256


def stin_ok(M, C, NQ):
    """Shapes lr_stin_block_f16 takes (everything else keeps the proj_in GEMM -> LayerNorm-folded q|k|v GEMM path)."""
    return C == STIN_C and M % STIN_ROWS == 0 and NQ > 0 and NQ % 192 == 0 and NQ <= 4096


def stin_block(x, wp, bp, wqkv, bqkv, *, eps, out=None, qkv_out=None, gn=None):
    """x1 = x wp^T + bp;  qkv = LayerNorm(x1) wqkv^T + bqkv  in one launch (lr_stin_block_f16): SpatialTransformer.proj_in and the
    LayerNorm-folded fused q|k|v projection of its block's self-attention.  wqkv / bqkv: packing.fold_layernorm of [to_q; to_k; to_v]
    (natural column order).  gn = (gp [samples, chunks, 32, 2], chunks, HW, gamma, beta, eps): x is the RAW tensor and the SpatialTransformer's
    GroupNorm is applied to the rows on the way in (what group_norm_groups would have written, bit for bit).  Returns (x1 [M, C], qkv [M, NQ])."""
    lib = _lib.load()
    _chk16(x, "x")
    M, C = x.shape
    NQ = wqkv.shape[0]
    assert stin_ok(M, C, NQ), (M, C, NQ)
    assert wp.dtype == x.dtype and wp.is_contiguous() and wp.shape == (C, C) and wqkv.dtype == x.dtype and wqkv.is_contiguous() and wqkv.shape == (NQ, C)
    assert bp.dtype == torch.float32 and bp.numel() == C and bqkv.dtype == torch.float32 and bqkv.numel() == NQ
    x1 = torch.empty_like(x) if out is None else out
    qkv = torch.empty(M, NQ, device=x.device, dtype=x.dtype) if qkv_out is None else qkv_out
    assert x1.shape == x.shape and x1.is_contiguous() and qkv.shape == (M, NQ) and qkv.stride(1) == 1 and qkv.dtype == x.dtype
    a = StinArgs()
    a.x, a.wp, a.bp, a.wqkv, a.bqkv, a.x1, a.qkv = _p(x), _p(wp), _p(bp), _p(wqkv), _p(bqkv), _p(x1), _p(qkv)
    a.M, a.C, a.NQ, a.ld_qkv, a.ln_eps = M, C, NQ, qkv.stride(0), float(eps)
    a.gn_part = a.gn_gamma = a.gn_beta = 0
    a.gn_chunks = a.gn_hw = 0
    a.gn_eps = 0.0
    if gn is not None:
        gp, chunks, hw, gamma, beta, geps = gn
        assert gp.dtype == torch.float32 and gp.is_contiguous() and gp.shape == (M // hw, chunks, 32, 2) and hw % STIN_ROWS == 0
        assert gamma.dtype == torch.float32 and beta.dtype == torch.float32 and gamma.numel() == C and beta.numel() == C
        a.gn_part, a.gn_gamma, a.gn_beta, a.gn_chunks, a.gn_hw, a.gn_eps = _p(gp), _p(gamma), _p(beta), int(chunks), int(hw), float(geps)
    _lib.check(_fn(lib, "lr_stin_block_f16", x.dtype)(a, _stream()), "stin_block")
    return x1, qkv


ROWLIN_ROWS = 128
# widths the row-resident kernel takes, by kind of projection: "qkv" (LayerNorm + fused q|k|v), "q" (LayerNorm + attn2.to_q), "in" (plain
# proj_in), "geglu" (LayerNorm + gated projection).  Level 1 only: at level 2 (C = 1280, 4096 rows) it was measured and lost to the tiled
# GEMM (31.9 vs 24.5 us at N = 1280, 58.2 vs 54.8 q|k|v, 128 vs 113 GEGLU; profiles/r06_rowlin_microbench.txt) -- that instance is
# compiled in developer builds only.
ROWLIN_WIDTHS = {"qkv": (640,), "q": (), "in": (640,), "geglu": (640,)}
# level 0 (C = 320), developer builds of the library only: the feed-forward as row-resident GEGLU projection (256-row blocks) + ONE GEMM for
# ff.net[2] composed with proj_out, instead of the fused lr_ffn_block_f16.  Measured and lost: 129.5 + 99.1 us against 220-225 us, UNet step
# 17.92 vs 17.87 ms same box (profiles/r06_ffn_split_ab.txt) -- off; LEFTREFILL_FFN_SPLIT=1 with LEFTREFILL_LIB_PATH=<developer build> enables it.
FFN_SPLIT = os.environ.get("LEFTREFILL_FFN_SPLIT", "0") != "0"
ROWLIN_MIN_ROWS = 2048      # below this the column slices of a launch cannot fill the chip
# LEFTREFILL_ROWLIN=0 keeps the tiled GEMMs everywhere
ROWLIN = os.environ.get("LEFTREFILL_ROWLIN", "1") != "0"


def rowlin_ok(M, C, N, kind="qkv"):
    """Shapes / uses lr_rowlin_f16 takes (everything else keeps the [LayerNorm-folded] GEMM)."""
    if kind == "geglu" and C == 320:
        return ROWLIN and FFN_SPLIT and _lib.dev_variants() and M % (2 * ROWLIN_ROWS) == 0 and M >= 8 * ROWLIN_MIN_ROWS and N > 0 and N % 64 == 0 and N <= 2560
    return ROWLIN and C in ROWLIN_WIDTHS.get(kind, ()) and M % ROWLIN_ROWS == 0 and M >= ROWLIN_MIN_ROWS and N > 0 and N % 64 == 0


def rowlin(x, w, bias, *, eps=1e-5, geglu=False, ln=True, out=None, gn=None):
    """LayerNorm(x) w^T + bias (geglu: value * gelu(gate) of the interleaved rows) with the rows resident in registers (lr_rowlin_f16):
    the wide short-K projections of a C = 640 block.  w / bias: packing.fold_layernorm (GEGLU: in packing.geglu_perm row order)."""
    lib = _lib.load()
    _chk16(x, "x")
    M, C = x.shape
    N = w.shape[0]
    assert C in (320, 640, 1280) and M % (ROWLIN_ROWS * (2 if C == 320 else 1)) == 0 and N % 64 == 0, (M, C, N)      # (1280: developer builds only; 320: GEGLU only)
    assert w.dtype == x.dtype and w.is_contiguous() and w.shape == (N, C) and bias.dtype == torch.float32 and bias.numel() == N
    n_out = N // 2 if geglu else N
    if out is None:
        out = torch.empty(M, n_out, device=x.device, dtype=x.dtype)
    assert out.shape == (M, n_out) and out.stride(1) == 1 and out.dtype == x.dtype
    a = RowlinArgs()
    a.x, a.w, a.bias, a.out = _p(x), _p(w), _p(bias), _p(out)
    a.M, a.C, a.N, a.ld_out, a.geglu, a.ln_eps, a.ln = M, C, N, out.stride(0), int(bool(geglu)), float(eps), int(bool(ln))
    a.gn_part = a.gn_gamma = a.gn_beta = 0
    a.gn_chunks = a.gn_hw = 0
    a.gn_eps = 0.0
    if gn is not None:      # (gp, chunks, HW, gamma, beta, eps): GroupNorm of the raw rows on the way in, see stin_block
        gp, chunks, hw, gamma, beta, geps = gn
        assert not ln and not geglu and gp.dtype == torch.float32 and gp.is_contiguous() and gp.shape == (M // hw, chunks, 32, 2) and hw % ROWLIN_ROWS == 0
        assert gamma.dtype == torch.float32 and beta.dtype == torch.float32 and gamma.numel() == C and beta.numel() == C
        a.gn_part, a.gn_gamma, a.gn_beta, a.gn_chunks, a.gn_hw, a.gn_eps = _p(gp), _p(gamma), _p(beta), int(chunks), int(hw), float(geps)
    _lib.check(_fn(lib, "lr_rowlin_f16", x.dtype)(a, _stream()), "rowlin")
    return out


FFN_C, FFN_ROWS, FFN_MAX_H = 320, 128, 2048


def ffn_ok(M, C, H):
    """Shapes lr_ffn_block_f16 takes (everything else keeps the GEGLU GEMM -> Linear GEMM path)."""
    return C == FFN_C and M % FFN_ROWS == 0 and H % 64 == 0 and 0 < H <= FFN_MAX_H


def ffn_block(x, w1, b1, w2, b2, *, eps, want_stats=False, out=None, post=None, want_gn_stats=False, gn_hw=0):
    """x + W2 (u * gelu(g)) + b2 with [u | g] = LayerNorm(x) W1^T + b1, in one launch (lr_ffn_block_f16).
    w1 / b1: LayerNorm-folded GEGLU projection in the interleaved [u16 | g16] row order (packing.pack_geglu / fold_layernorm);
    w2: second Linear as packing.pack_pieces ([H / 64, C, 64]).  post = (Wp pieces, bp, x_in): out = x3 Wp^T + bp + x_in as well
    (SpatialTransformer.proj_out + outer residual).  Returns out [M, C]; (out, stats [M, 2, 2]) with want_stats; (out, (column sums
    [M / 128, C, 2], 128)) with want_gn_stats (needs post; takes precedence over want_stats)."""
    lib = _lib.load()
    _chk16(x, "x")
    M, C = x.shape
    H = w2.shape[0] * 64
    assert ffn_ok(M, C, H), (M, C, H)
    assert w1.dtype == x.dtype and w1.is_contiguous() and w1.shape == (2 * H, C)
    assert w2.dtype == x.dtype and w2.is_contiguous() and w2.shape == (H // 64, C, 64)
    assert b1.dtype == torch.float32 and b1.numel() == 2 * H and b2.dtype == torch.float32 and b2.numel() == C
    if out is None:
        out = torch.empty_like(x)
    assert out.shape == x.shape and out.dtype == x.dtype and out.is_contiguous() and out.device == x.device
    stats = torch.empty(M, 2, 2, device=x.device, dtype=torch.float32) if want_stats else None      # one partial per wave of a pair
    a = FfnArgs()
    a.x, a.out, a.w1, a.b1, a.w2, a.b2, a.stats_out = _p(x), _p(out), _p(w1), _p(b1), _p(w2), _p(b2), _p(stats)
    a.M, a.C, a.H, a.ln_eps = M, C, H, float(eps)
    a.post_w = a.post_b = a.post_resid = a.gn_stats_out = 0
    a.gn_group_out, a.gn_hw = 0, 0
    gstats = None
    if post is not None:
        # (Wp pieces [5, C, 64], bp, x_in): out = (x + ff(LN x)) Wp^T + bp + x_in in the same launch (SpatialTransformer.proj_out)
        pw_, pb_, pr_ = post
        _chk16(pr_, "post_resid")
        assert pw_.dtype == x.dtype and pw_.is_contiguous() and pw_.shape == (C // 64, C, 64) and pr_.shape == (M, C)
        assert pb_.dtype == torch.float32 and pb_.numel() == C
        a.post_w, a.post_b, a.post_resid = _p(pw_), _p(pb_), _p(pr_)
        if want_gn_stats:
            gp, chunks = None, 0
            if GN_GROUPS and gn_hw and gn_hw % FFN_ROWS == 0 and M % gn_hw == 0:
                chunks = gn_hw // FFN_ROWS
                gp = torch.empty(M // gn_hw, chunks, 32, 2, device=x.device, dtype=torch.float32)
                a.gn_group_out, a.gn_hw = _p(gp), gn_hw
            gstats = (torch.empty(M // FFN_ROWS, C, 2, device=x.device, dtype=torch.float32), FFN_ROWS, gp, chunks)
            a.gn_stats_out = _p(gstats[0])
    else:
        assert not want_gn_stats
    _lib.check(_fn(lib, "lr_ffn_block_f16", x.dtype)(a, _stream()), "ffn_block")
    if want_gn_stats:
        return out, gstats
    return (out, stats) if want_stats else out


def softmax_rows(s, scale, out=None):
    """p = softmax(scale * s, dim=-1) for materialised fp16 logits s [M, N] (VAE AttnBlock); in place when out is s."""
    lib = _lib.load()
    _chk16(s, "s")
    M, N = s.shape
    if out is None:
        out = torch.empty_like(s)
    _lib.check(lib.lr_softmax_rows_f16(_p(s), _p(out), M, N, float(scale), _stream()), "softmax_rows")
    return out


def mv_gather(x, b, v, s):
    lib = _lib.load()
    _chk16(x, "x")
    C = x.shape[-1]
    seq = torch.empty(b * (v + 1) * s * s, C, device=x.device, dtype=x.dtype)
    _lib.check(_fn(lib, "lr_mv_gather", x.dtype)(_p(x), _p(seq), b, v, s, C, _stream()), "mv_gather")
    return seq


def row_copy(jobs):
    """Up to four row-copy jobs in one launch (lr_row_copy).  job = dict(src, dst, row_bytes, n_rows[, src_off, dst_off, src_idx,
    dst_idx]): tensors with contiguous rows (pitch = stride(0) in bytes); index tables int32 device tensors or None (identity)."""
    lib = _lib.load()
    assert 1 <= len(jobs) <= 4
    arr = (_lib.RowCopyJob * len(jobs))()
    for a, j in zip(arr, jobs):
        src, dst = j["src"], j["dst"]
        assert src.is_cuda and dst.is_cuda and src.stride(-1) == 1 and dst.stride(-1) == 1
        a.src, a.src_pitch, a.src_off = src.data_ptr(), src.stride(0) * src.element_size(), int(j.get("src_off", 0))
        a.dst, a.dst_pitch, a.dst_off = dst.data_ptr(), dst.stride(0) * dst.element_size(), int(j.get("dst_off", 0))
        a.row_bytes, a.n_rows = int(j["row_bytes"]), int(j["n_rows"])
        si, di = j.get("src_idx"), j.get("dst_idx")
        for t_ in (si, di):
            assert t_ is None or (t_.dtype == torch.int32 and t_.is_cuda and t_.is_contiguous() and t_.numel() >= a.n_rows)
        a.src_idx, a.dst_idx = _p(si), _p(di)
    _lib.check(lib.lr_row_copy(arr, len(jobs), _stream()), "row_copy")


def mv_scatter(seq, b, v, s):
    lib = _lib.load()
    _chk16(seq, "seq")
    C = seq.shape[-1]
    x = torch.empty(b * v * s * 2 * s, C, device=seq.device, dtype=seq.dtype)
    _lib.check(_fn(lib, "lr_mv_scatter", seq.dtype)(_p(seq), _p(x), b, v, s, C, _stream()), "mv_scatter")
    return x


def _eps16(eps):
    return torch.bfloat16 if eps.dtype == torch.bfloat16 else torch.float16


def _cfg_step(name, x, eps, n_eps, extra, outs, scalars):
    """The call path of the fused CFG sampler steps: lr_<name>[_bf16](x, eps, eps_is_f32, *extra, *outputs, numel, *scalars,
    stream), the 16-bit twin chosen by eps.dtype.  x [B,...] fp32; eps [n_eps B,...] fp16|bf16|fp32; extra: the step's own
    arguments in front of the outputs -- an optional fp32 stream (tensor or None: its fp32 contiguous form is passed) or a plain
    ctypes value; outs: one flag per output, False = not wanted (null).  Returns the fp32 outputs, each like x (None where not
    wanted), in the order of the C signature."""
    lib = _lib.load()
    assert x.dtype == torch.float32 and x.is_contiguous() and eps.is_contiguous()
    assert eps.numel() == n_eps * x.numel() and eps.dtype in (torch.float16, torch.bfloat16, torch.float32)
    extra = [a.float().contiguous() if torch.is_tensor(a) else a for a in extra]
    outs = [torch.empty_like(x) if wanted else None for wanted in outs]
    _lib.check(_fn(lib, "lr_" + name, _eps16(eps))(
        _p(x), _p(eps), int(eps.dtype == torch.float32), *[_p(a) if a is None or torch.is_tensor(a) else a for a in extra],
        *[_p(o) for o in outs], x.numel(), *[float(v) for v in scalars], _stream()), name)
    return outs


def ddim_cfg_step(x, eps, noise, cfg_scale, a_t, a_prev, sigma_t, sqrt_one_minus_at):
    """x [B,...] fp32; eps [2B,...] fp16|fp32 (uncond first); returns (x_prev, pred_x0) fp32."""
    x_prev, pred = _cfg_step("ddim_cfg_step", x, eps, 2, (noise,), (True, True),
                             (cfg_scale, a_t, a_prev, sigma_t, sqrt_one_minus_at))
    return x_prev, pred


def ddpm_step(x, eps, noise, sqrt_recip_ac, sqrt_recipm1_ac, coef1, coef2, sigma, clip_denoised=False, return_x0=False,
              known=None):
    """One ancestral DDPM posterior step (LatentDiffusion.p_sample after the model call).  x [B,...] fp32; eps like x,
    fp16|bf16|fp32 (one slab: no guidance); noise fp32 like x (None allowed when sigma == 0); the five coefficients are host
    floats, the fp32 table entries of the step's timestep -- sigma = (t != 0) exp(0.5 logvar_clipped[t]).  known: None, or
    (x0, q_noise, mask, sqrt_ac, sqrt_one_minus_ac) -- the known-region blend (sqrt_ac x0 + sqrt_one_minus_ac q_noise) mask +
    (1 - mask) x_prev in the same launch; mask is shaped like x or [B,1,H,W] against x [B,C,H,W].
    Returns (x_prev, x_recon) fp32; x_recon is None unless return_x0."""
    x0 = qn = mask = None
    chw = hw = 0
    sa = s1ma = 0.0
    if known is not None:
        x0, qn, mask, sa, s1ma = known
        assert x0.shape == x.shape and qn.shape == x.shape
        if mask.shape != x.shape:
            assert x.dim() == 4 and mask.shape == (x.shape[0], 1) + tuple(x.shape[2:]), "mask: like x, or [B,1,H,W]"
            hw = x.shape[2] * x.shape[3]
            chw = x.shape[1] * hw
    if float(sigma) == 0.0:
        noise = None
    x_prev, x_recon = _cfg_step("ddpm_step", x, eps, 1, (noise, x0, qn, mask, chw, hw, int(bool(clip_denoised))),
                                (True, return_x0), (sqrt_recip_ac, sqrt_recipm1_ac, coef1, coef2, sigma, sa, s1ma))
    return x_prev, x_recon


def plms_cfg_step(x, eps, hist, weights, divisor, cfg_scale, a_t, a_prev, sqrt_one_minus_at, write_e=True):
    """One PLMS update (sigma = 0).  x [B,...] fp32; eps [2B,...] fp16|bf16|fp32 (uncond first); hist: up to 3 fp32 tensors
    like x, newest first; weights: len(hist) + 1 integer weights, divisor their common denominator.
    Returns (x_prev, pred_x0, e): e is this evaluation's CFG-combined eps in fp32 (None unless write_e)."""
    assert len(hist) <= 3 and len(weights) == len(hist) + 1
    for h in hist:
        assert h.dtype == torch.float32 and h.is_contiguous() and h.numel() == x.numel() and h.device == x.device
    ptrs = (ctypes.c_void_p * 3)(*[h.data_ptr() for h in hist], *([None] * (3 - len(hist))))
    w = (ctypes.c_float * 4)(*[float(w_) for w_ in weights], *([0.0] * (4 - len(weights))))
    e, x_prev, pred = _cfg_step("plms_cfg_step", x, eps, 2, (ctypes.addressof(ptrs), len(hist), ctypes.addressof(w), float(divisor)),
                                (write_e, True, True), (cfg_scale, a_t, a_prev, sqrt_one_minus_at))
    return x_prev, pred, e


def dpmpp_cfg_step(x, eps, x0_prev, cfg_scale, sigma_s, alpha_s, ratio, c, c_half=0.0, inv_r0=0.0):
    """One DPM-Solver++ multistep update: order 1 when x0_prev is None, else order 2.  x [B,...] fp32; eps [2B,...]
    fp16|bf16|fp32 (uncond first); x0_prev fp32 like x.  Returns (x_next, x0) -- x0 is this step's data prediction."""
    if x0_prev is not None:
        assert x0_prev.dtype == torch.float32 and x0_prev.is_contiguous() and x0_prev.numel() == x.numel()
    x0, x_next = _cfg_step("dpmpp_cfg_step", x, eps, 2, (x0_prev,), (True, True),
                           (cfg_scale, sigma_s, alpha_s, ratio, c, c_half, inv_r0))
    return x_next, x0


def ddim_inv_cfg_step(x, eps, cfg_scale, c1, c2):
    """One DDIM inversion step (DDIMSampler.encode): x_next = c1 x + c2 e with e = e_u + s (e_c - e_u).  x [B,...] fp32;
    eps [2B,...] fp16|bf16|fp32 (uncond first); c1, c2: the host coefficients (python / float64 values).  Returns x_next fp32."""
    if eps.dtype in HALF_TYPES:      # the reference casts the 0-dim float64 c2 to eps's dtype: round once, from float64
        c2 = torch.tensor(float(c2), dtype=torch.float64).to(eps.dtype).item()
    return _cfg_step("ddim_inv_cfg_step", x, eps, 2, (), (True,), (cfg_scale, c1, c2))[0]


def ddim_cfg3_step(x, eps, noise, cfg_scale, cond_weight, a_t, a_prev, sigma_t, sqrt_one_minus_at):
    """Three-way guidance + DDIM update (StructureDDIMSampler.p_sample_ddim_guide).  x [B,...] fp32; eps [3B,...] fp16|bf16|fp32
    in the order uncond, cond, cond_simple; noise fp32 like x or None.  Returns (x_prev, pred_x0) fp32."""
    w = float(cond_weight)
    x_prev, pred = _cfg_step("ddim_cfg3_step", x, eps, 3, (noise,), (True, True),
                             (cfg_scale, w, 1 - w, a_t, a_prev, sigma_t, sqrt_one_minus_at))
    return x_prev, pred


Q_SAMPLE_MAX_B = 32          # LR_Q_SAMPLE_MAX_B: coefficient pairs per launch (kernel arguments)


def ddim_q_sample(x0, noise, sa, s1ma):
    """out[b] = sa[b] x0[b] + s1ma[b] noise[b] (DDIMSampler.stochastic_encode).  x0, noise [B,...] fp32; sa, s1ma: B host floats
    (the fp32 values).  One launch per Q_SAMPLE_MAX_B samples."""
    lib = _lib.load()
    assert x0.dtype == torch.float32 and noise.dtype == torch.float32 and x0.shape == noise.shape
    x0, noise = x0.contiguous(), noise.contiguous()
    B = x0.shape[0]
    assert len(sa) == len(s1ma) == B
    per = x0.numel() // B
    out = torch.empty_like(x0)
    for b0 in range(0, B, Q_SAMPLE_MAX_B):
        n = min(Q_SAMPLE_MAX_B, B - b0)
        a = (ctypes.c_float * n)(*[float(v) for v in sa[b0:b0 + n]])
        s = (ctypes.c_float * n)(*[float(v) for v in s1ma[b0:b0 + n]])
        _lib.check(lib.lr_ddim_q_sample(_p(x0[b0:b0 + n]), _p(noise[b0:b0 + n]), _p(out[b0:b0 + n]), n, per, ctypes.addressof(a),
                                        ctypes.addressof(s), _stream()), "ddim_q_sample")
    return out


def seeded_normal(keys, stream, step, out):
    """Fill out [B, ...] (fp32, cuda, contiguous as [B][per_sample]; its base may sit at any 4-byte offset) with the seeded normals of
    the B keys (lr_seeded_normal, one launch; leftrefill_amd/noise.py states the values).  keys: int64 [B, 2] on out's device -- the
    uint64 seed bits and the sub-sample number of every row; stream, step: uint32 names of the draw.  Returns out.  Draws nothing from
    torch's generators."""
    lib = _lib.load()
    assert out.is_cuda and out.dtype == torch.float32 and out.is_contiguous() and out.dim() >= 1, "out: contiguous cuda fp32 [B, ...]"
    B = out.shape[0]
    assert keys.dtype == torch.int64 and keys.device == out.device and keys.is_contiguous() and tuple(keys.shape) == (B, 2), \
        "keys: contiguous int64 [B, 2] on out's device"
    stream, step = int(stream), int(step)
    assert 0 <= stream < 2 ** 32 and 0 <= step < 2 ** 32, "stream, step: uint32"
    per = out.numel() // B if B else 0
    with torch.cuda.device(out.device):
        _lib.check(lib.lr_seeded_normal(_p(keys), B, per, ctypes.c_int32(stream).value, ctypes.c_int32(step).value, _p(out), _stream()),
                   "seeded_normal")
    return out


EVAL_TILE_H, EVAL_TILE_W, EVAL_SLOT_FLOATS = 32, 64, 8      # LR_EVAL_TILE_H / _W / LR_EVAL_SLOT_FLOATS
EVAL_PRED_KIND = {torch.float32: 0, torch.float16: 1, torch.bfloat16: 2}      # LR_EVAL_PRED_*


def eval_metrics(pred, origin, mask=None, x0=0, Wc=None, r=1, want_rgb8=False):
    """Score a decoded prediction on the device (lr_eval_metrics: composite, crop, area down-sampling, PSNR, SSIM, finite count, uint8
    image in one pass).  pred [N,3,H,W] fp32|fp16|bf16 and origin [N,3,H,W] (fp32 is passed) in [-1, 1]; mask [N,1,H,W] or None (no
    composite); columns [x0, x0 + Wc) are scored (Wc None: to the right edge); r: integer area-down-sampling factor.
    Returns (out, rgb8): out [N,4] fp32 = (mse, psnr_db, ssim, nonfinite) per sample, rgb8 [N,H/r,Wc/r,3] uint8 or None -- device
    tensors, nothing is read back here."""
    lib = _lib.load()
    assert pred.is_cuda and pred.dim() == 4 and pred.shape[1] == 3 and pred.dtype in EVAL_PRED_KIND, "pred: cuda [N,3,H,W] fp32 / fp16 / bf16"
    N, _, H, W = pred.shape
    assert origin.shape == pred.shape and origin.device == pred.device, "origin: like pred"
    pred, origin = pred.contiguous(), origin.float().contiguous()
    if mask is not None:
        assert mask.shape == (N, 1, H, W) and mask.device == pred.device, "mask: [N,1,H,W]"
        mask = mask.float().contiguous()
    Wc = W - x0 if Wc is None else Wc
    r = int(r)
    if r < 1 or H % r or Wc % r:
        raise ValueError(f"eval_metrics: r={r} must divide the scored size {H} x {Wc}")
    Ho, Wo = H // r, Wc // r
    slots = N * (-(-Ho // EVAL_TILE_H)) * (-(-Wo // EVAL_TILE_W))
    partials = torch.empty(slots * EVAL_SLOT_FLOATS, device=pred.device, dtype=torch.float32)
    out = torch.empty(N, 4, device=pred.device, dtype=torch.float32)
    rgb8 = torch.empty(N, Ho, Wo, 3, device=pred.device, dtype=torch.uint8) if want_rgb8 else None
    _lib.check(lib.lr_eval_metrics(_p(pred), EVAL_PRED_KIND[pred.dtype], _p(origin), _p(mask), N, H, W, int(x0), int(Wc), r,
                                   _p(partials), _p(out), _p(rgb8), _stream()), "eval_metrics")
    return out, rgb8


OPT_GRAD_KIND = {torch.float32: 0, torch.float16: 1, torch.bfloat16: 2}      # LR_OPT_GRAD_*
OPT_MAX_GROUPS, OPT_MAX_BLOCKS, OPT_STATE_WORDS, OPT_CONSTS = 8, 1024, 48, 16      # LR_OPT_* of include/leftrefill_hip.h
# state-block word -> name (LR_OPT_SCALE ... LR_OPT_LR_INDEX); scale / grad_norm / inv_scale are float bits, the rest int32
OPT_STATE_FIELDS = ("scale", "growth_tracker", "found_inf", "applied_steps", "sched_steps", "skipped", "grad_norm", "inv_scale",
                    "lr_index")
# kernel launches of amp_adamw_step so far, as the library itself counted them (no profiler involved)
OPT_LAUNCHES = ctypes.c_int(0)


def amp_adamw_step(tensors, n_tensors, groups, n_groups, state, partials, blocks, growth_factor=2.0, backoff_factor=0.5,
                   growth_interval=2000):
    """lr_amp_adamw_step: unscale + non-finite scan, GradScaler update and AdamW over the device table `tensors` (uint8 image of
    n_tensors lr_optim_tensor), `groups` (n_groups lr_optim_group), the int32 `state` block and `partials` [4 * blocks] fp32.  Nothing
    is read back; three launches whatever n_tensors."""
    lib = _lib.load()
    for t, name in ((tensors, "tensors"), (groups, "groups"), (state, "state"), (partials, "partials")):
        assert t.is_cuda and t.is_contiguous(), f"{name}: contiguous device tensor"
    assert tensors.numel() * tensors.element_size() >= n_tensors * ctypes.sizeof(_lib.OptimTensor), "tensor table too small"
    assert groups.numel() * groups.element_size() >= n_groups * ctypes.sizeof(_lib.OptimGroup), "group table too small"
    assert state.dtype == torch.int32 and state.numel() >= OPT_STATE_WORDS, "state: int32 [LR_OPT_STATE_WORDS]"
    assert partials.dtype == torch.float32 and partials.numel() >= 4 * blocks, "partials: fp32 [4 * blocks]"
    _lib.check(lib.lr_amp_adamw_step(_p(tensors), int(n_tensors), _p(groups), int(n_groups), _p(state), _p(partials), int(blocks),
                                     float(growth_factor), float(backoff_factor), int(growth_interval), ctypes.byref(OPT_LAUNCHES),
                                     _stream()), "amp_adamw_step")


LPIPS_LAUNCHES, LPIPS_MIN_SIDE, LPIPS_HEAD_PIXELS = 13, 31, 64      # LR_LPIPS_* of include/leftrefill_hip.h
LPIPS_CONVS = ((3, 64, 11, 4, 2), (64, 192, 5, 1, 2), (192, 384, 3, 1, 1), (384, 256, 3, 1, 1), (256, 256, 3, 1, 1))   # evalglue.LPIPSAlex.CONVS


def lpips_stage_sizes(Ho, Wo):
    """(h_k, w_k) of the five stage outputs on an Ho x Wo scored image (the formula of the lr_lpips_alex header comment)."""
    s1 = ((Ho - 7) // 4 + 1, (Wo - 7) // 4 + 1)
    s2 = ((s1[0] - 3) // 2 + 1, (s1[1] - 3) // 2 + 1)
    s3 = ((s2[0] - 3) // 2 + 1, (s2[1] - 3) // 2 + 1)
    return [s1, s2, s3, s3, s3]


def lpips_workspace_bytes(N, H, Wc, r=1):
    """The Python statement of lr_lpips_workspace_bytes: five fp16 stage outputs of the 2N images, the two pooled maps, 8 bytes per
    head workgroup; every term rounded up to 256 bytes."""
    up = lambda v: (v + 255) // 256 * 256
    sizes = lpips_stage_sizes(H // r, Wc // r)
    total = sum(up(2 * N * h * w * conv[1] * 2) for (h, w), conv in zip(sizes, LPIPS_CONVS))
    total += up(2 * N * sizes[1][0] * sizes[1][1] * 64 * 2) + up(2 * N * sizes[2][0] * sizes[2][1] * 192 * 2)
    return total + up(8 * N * sum(-(-h * w // LPIPS_HEAD_PIXELS) for h, w in sizes))


def pack_lpips(module):
    """evalglue.LPIPSAlex (weights loaded) -> the operands of lr_lpips_alex on the module's device: {"wt": five fp16 [Cout, Kpad] with
    K index (ky * ks + kx) * Cin + c and Kpad = K rounded up to 64 with zeros, "bias": five fp32 [Cout], "lin": five fp32 [Cout]}."""
    wt, bias, lin = [], [], []
    for conv, l in zip(module.convs, module.lins):
        w = conv.weight.detach().float()
        co = w.shape[0]
        w = w.permute(0, 2, 3, 1).reshape(co, -1)
        kpad = -(-w.shape[1] // 64) * 64
        packed = torch.zeros(co, kpad, device=w.device, dtype=torch.float16)
        packed[:, :w.shape[1]] = w.half()
        wt.append(packed.contiguous())
        bias.append(conv.bias.detach().float().contiguous().clone())
        lin.append(l.detach().float().reshape(-1).contiguous().clone())
    return {"wt": wt, "bias": bias, "lin": lin}


def lpips_alex(pred, origin, mask, x0, Wc, r, packed, out=None):
    """LPIPS(alex) of the image lr_eval_metrics scores -- composite pred * mask + origin * (1 - mask) (mask None: none), columns
    [x0, x0 + Wc), r x r area mean -- against the same crop of origin, on the device (lr_lpips_alex: 13 launches whatever N, nothing
    read back).  pred [N,3,H,W] fp32|fp16|bf16, origin like it (fp32 is passed), mask [N,1,H,W] or None; packed: pack_lpips(module).
    Returns out [N] fp32 (a device tensor; `out` is filled when given)."""
    lib = _lib.load()
    assert pred.is_cuda and pred.dim() == 4 and pred.shape[1] == 3 and pred.dtype in EVAL_PRED_KIND, "pred: cuda [N,3,H,W] fp32 / fp16 / bf16"
    N, _, H, W = pred.shape
    assert origin.shape == pred.shape and origin.device == pred.device, "origin: like pred"
    pred, origin = pred.contiguous(), origin.float().contiguous()
    if mask is not None:
        assert mask.shape == (N, 1, H, W) and mask.device == pred.device, "mask: [N,1,H,W]"
        mask = mask.float().contiguous()
    Wc = W - x0 if Wc is None else Wc
    x0, Wc, r = int(x0), int(Wc), int(r)
    need = int(lib.lr_lpips_workspace_bytes(N, H, Wc, r))
    if need < 0:
        _lib.check(need, f"lpips_alex (N {N}, scored {H} x {Wc}, r {r}: r must divide both sides and leave {LPIPS_MIN_SIDE} pixels)")
    workspace = torch.empty(need, device=pred.device, dtype=torch.uint8)
    if out is None:
        out = torch.empty(N, device=pred.device, dtype=torch.float32)
    assert out.is_cuda and out.dtype == torch.float32 and out.numel() == N and out.is_contiguous(), "out: fp32 [N]"
    a = _lib.LpipsArgs()
    a.pred, a.pred_kind, a.origin, a.mask = _p(pred), EVAL_PRED_KIND[pred.dtype], _p(origin), _p(mask)
    a.N, a.H, a.W, a.x0, a.Wc, a.r = N, H, W, x0, Wc, r
    for k in range(5):
        assert packed["wt"][k].dtype == torch.float16 and packed["wt"][k].device == pred.device, "packed: pack_lpips on pred's device"
        a.wt[k], a.bias[k], a.lin[k] = _p(packed["wt"][k]), _p(packed["bias"][k]), _p(packed["lin"][k])
    a.workspace, a.workspace_bytes, a.out = _p(workspace), need, _p(out)
    _lib.check(lib.lr_lpips_alex(ctypes.byref(a), _stream()), "lpips_alex")
    return out


# kernel launches of the four lr_fid_* entry points so far, as the library itself counted them (no profiler involved)
FID_LAUNCHES = ctypes.c_int(0)
FID_SRC_U8 = 3      # LR_FID_SRC_U8


def fid_input(src, dst, out, x0=0, Wc=None, origin=None, mask=None):
    """lr_fid_input: src uint8 [N,H,W,3], or [N,3,H,W] fp32|fp16|bf16 in [-1, 1] (truncated to 8 bits; with mask [N,1,H,W] and origin
    [N,3,H,W] after the composite src * mask + origin * (1 - mask)), columns [x0, x0 + Wc) -> dst, fp16 [N, out, out, 4]: / 255,
    bilinear resize without antialiasing, 2 x - 1, channel 3 zero.  One launch, nothing read back."""
    lib = _lib.load()
    assert src.is_cuda and src.dim() == 4, "src: cuda [N,H,W,3] uint8 or [N,3,H,W]"
    if src.dtype == torch.uint8:
        assert src.shape[3] == 3 and mask is None and origin is None, "uint8 src: [N,H,W,3], no composite"
        N, H, W, _ = src.shape
        kind = FID_SRC_U8
    else:
        assert src.shape[1] == 3 and src.dtype in EVAL_PRED_KIND, "src: [N,3,H,W] fp32 / fp16 / bf16"
        N, _, H, W = src.shape
        kind = EVAL_PRED_KIND[src.dtype]
    src = src.contiguous()
    if mask is not None:
        assert origin is not None and origin.shape == src.shape and mask.shape == (N, 1, H, W), "origin like src, mask [N,1,H,W]"
        origin, mask = origin.float().contiguous(), mask.float().contiguous()
    else:
        origin = None
    Wc = W - x0 if Wc is None else Wc
    assert dst.is_cuda and dst.dtype == torch.float16 and dst.is_contiguous() and dst.numel() == N * out * out * 4, "dst: fp16 [N,out,out,4]"
    _lib.check(lib.lr_fid_input(_p(src), kind, _p(origin), _p(mask), N, H, W, int(x0), int(Wc), _p(dst), int(out),
                                ctypes.byref(FID_LAUNCHES), _stream()), "fid_input")
    return dst


def fid_run(program, B, arena, wt, bias):
    """lr_fid_run: the rows of `program` (int32 numpy [n, 24], words LR_FID_*; leftrefill_amd.fid.FID_PROGRAM is the network) on a batch
    of B images whose activations live in `arena` (fp16); wt (fp16) / bias (fp32): the packed blobs (fid.pack_fid).  Every row is
    checked against the three sizes before the first launch (RuntimeError "bad argument", nothing launched); one launch per row."""
    import numpy as np
    lib = _lib.load()
    program = np.ascontiguousarray(program, dtype=np.int32)
    assert program.ndim == 2 and program.shape[1] == 24, "program: int32 [n, LR_FID_ROW_WORDS]"
    assert arena.is_cuda and arena.dtype == torch.float16 and arena.is_contiguous(), "arena: contiguous cuda fp16"
    assert wt is None or (wt.dtype == torch.float16 and wt.device == arena.device and wt.is_contiguous()), "wt: fp16 on the arena's device"
    assert bias is None or (bias.dtype == torch.float32 and bias.device == arena.device and bias.is_contiguous()), "bias: fp32 on the arena's device"
    _lib.check(lib.lr_fid_run(program.ctypes.data, program.shape[0], int(B), _p(arena), arena.numel(), _p(wt),
                              0 if wt is None else wt.numel(), _p(bias), 0 if bias is None else bias.numel(),
                              ctypes.byref(FID_LAUNCHES), _stream()), "fid_run")


def fid_head(src, B, HW, C, ld, out):
    """lr_fid_head: src fp16 [B, HW, ld] -> out fp32 [B, C], the mean over the pixels in index order.  One launch."""
    lib = _lib.load()
    assert src.is_cuda and src.dtype == torch.float16 and src.is_contiguous() and src.numel() >= B * HW * ld, "src: fp16 [B,HW,ld]"
    assert out.is_cuda and out.dtype == torch.float32 and out.is_contiguous() and out.numel() == B * C, "out: fp32 [B,C]"
    _lib.check(lib.lr_fid_head(_p(src), int(B), int(HW), int(C), int(ld), _p(out), ctypes.byref(FID_LAUNCHES), _stream()), "fid_head")
    return out


def fid_accumulate(feats, total, gram):
    """lr_fid_accumulate: total[D] += sum_r feats[r], gram[D,D] += sum_r feats[r] feats[r]^T in float64, rows added in order by the
    one thread that owns an element: no atomics, bitwise reproducible.  feats fp32 [n, D], D a multiple of 64.  One launch."""
    lib = _lib.load()
    n, D = feats.shape
    assert feats.is_cuda and feats.dtype == torch.float32 and feats.is_contiguous(), "feats: contiguous cuda fp32 [n,D]"
    for t, shape in ((total, (D,)), (gram, (D, D))):
        assert t.dtype == torch.float64 and t.device == feats.device and t.is_contiguous() and tuple(t.shape) == shape, "sums: float64 [D], [D,D]"
    _lib.check(lib.lr_fid_accumulate(_p(feats), int(n), int(D), _p(total), _p(gram), ctypes.byref(FID_LAUNCHES), _stream()), "fid_accumulate")


PIL_MAX_KSIZE = 1025      # LR_PIL_MAX_KSIZE


def pil_resize(src, tables, tables_host, jobs, jobs_host, n_jobs, work, dst):
    """lr_pil_resize: `n_jobs` independent `PIL.Image.resize` jobs (bicubic / bilinear, 8-bit, 1 or 3 channels) in at most two launches.
    src: the uint8 source arena on the device; tables / tables_host: the int32 coefficient arena on the device and in host memory;
    jobs / jobs_host: the uint8 image of the lr_pil_job table on the device and in host memory (leftrefill_amd.refill.ResizeTable
    builds both); work: the uint8 workspace of the intermediates; dst: the uint8 destination, which is returned.  Nothing is read back."""
    lib = _lib.load()
    for t, name in ((src, "src"), (work, "work"), (dst, "dst"), (jobs, "jobs")):
        assert t.is_cuda and t.dtype == torch.uint8 and t.is_contiguous(), f"{name}: contiguous cuda uint8"
    assert tables.is_cuda and tables.dtype == torch.int32 and tables.is_contiguous(), "tables: contiguous cuda int32"
    assert not tables_host.is_cuda and tables_host.dtype == torch.int32 and tables_host.numel() == tables.numel(), "tables_host: tables in host memory"
    assert not jobs_host.is_cuda and jobs_host.dtype == torch.uint8 and jobs_host.numel() == jobs.numel(), "jobs_host: jobs in host memory"
    assert jobs.numel() >= n_jobs * ctypes.sizeof(_lib.PilJob), "jobs: n_jobs lr_pil_job"
    _lib.check(lib.lr_pil_resize(_p(src), src.numel(), _p(tables), _p(tables_host), tables.numel(), _p(work), work.numel(), _p(dst),
                                 dst.numel(), _p(jobs), _p(jobs_host), int(n_jobs), _stream()), "pil_resize")
    return dst


def refill_canvas(ref, src, mask, H, W, n):
    """lr_refill_canvas: uint8 [P,Sh,Sw,3] reference, source and mask (resize destinations) -> the one-call route's batch of P * n
    canvases [reference | source], edge-padded to H x 2W: (image, masked_image [P n,3,H,2W], mask [P n,1,H,2W]) fp32, NCHW."""
    lib = _lib.load()
    P, Sh, Sw, _ = ref.shape
    for t, name in ((ref, "ref"), (src, "src"), (mask, "mask")):
        assert t.is_cuda and t.dtype == torch.uint8 and t.is_contiguous() and tuple(t.shape) == (P, Sh, Sw, 3), f"{name}: contiguous cuda uint8 [P,Sh,Sw,3]"
    image = torch.empty(P * n, 3, H, 2 * W, device=ref.device, dtype=torch.float32)
    masked_image = torch.empty_like(image)
    mask_out = torch.empty(P * n, 1, H, 2 * W, device=ref.device, dtype=torch.float32)
    _lib.check(lib.lr_refill_canvas(_p(ref), _p(src), _p(mask), P, Sh, Sw, int(H), int(W), int(n), _p(image), _p(masked_image), _p(mask_out),
                                    _stream()), "refill_canvas")
    return image, masked_image, mask_out


GRID_MAX_SOURCES = 8      # LR_GRID_MAX_SOURCES


def image_grid(sources, N, H, clamp=True, rescale=True, out=None):
    """lr_image_grid: the logger's uint8 canvas [Hc, Wc, 3] of up to GRID_MAX_SOURCES image batches in one launch (per source
    `make_grid(nrow=1, padding=2)`, clamp, (x + 1) / 2, * 255, truncation; leftrefill_amd.imagelog.grid_numpy states it).  sources: cuda
    tensors [B >= N, C, H, W], C in {1, 3}, fp32 | fp16 | bf16, of ANY strides (an NHWC view, a sliced batch: read in place, never copied),
    laid left to right; the first N images of each are used.  `out` (cuda uint8 [Hc, Wc, 3], contiguous) is filled when given.  Nothing
    is read back."""
    from .imagelog import canvas_layout
    lib = _lib.load()
    N, H = int(N), int(H)
    for t in sources:
        assert t.is_cuda and t.dim() == 4 and t.dtype in EVAL_PRED_KIND and t.shape[0] >= N and t.shape[2] == H, \
            "sources: cuda [B >= N, C, H, W] fp32 / fp16 / bf16"
    Hc, Wc, cols = canvas_layout([t.shape[3] for t in sources], N, H)
    arr = (_lib.GridSource * max(1, len(sources)))()
    for a, t, col in zip(arr, sources, cols):
        a.ptr, a.kind, a.C, a.W, a.col = t.data_ptr(), EVAL_PRED_KIND[t.dtype], t.shape[1], t.shape[3], col
        a.stride_n, a.stride_c, a.stride_h, a.stride_w = t.stride()
    if out is None:
        out = torch.empty(Hc, Wc, 3, device=sources[0].device, dtype=torch.uint8)
    assert out.is_cuda and out.dtype == torch.uint8 and tuple(out.shape) == (Hc, Wc, 3) and out.is_contiguous(), f"out: cuda uint8 [{Hc}, {Wc}, 3]"
    _lib.check(lib.lr_image_grid(arr, len(sources), N, H, int(bool(clamp)), int(bool(rescale)), _p(out), Wc, _stream()), "image_grid")
    return out


def token_drift(old, new, out=None):
    """lr_token_drift: out[t] = sqrt(sum_d (old[t, d] - new[t, d])^2) and old <- new in the same launch (the logger's "log the distance,
    then re-clone").  old, new: distinct contiguous cuda fp32 [T, D]; returns out fp32 [T] (a device tensor; `out` is filled when given)."""
    lib = _lib.load()
    for t, name in ((old, "old"), (new, "new")):
        assert t.is_cuda and t.dtype == torch.float32 and t.dim() == 2 and t.is_contiguous(), f"{name}: contiguous cuda fp32 [T, D]"
    assert old.shape == new.shape and old.device == new.device, "old: like new"
    T, D = new.shape
    if out is None:
        out = torch.empty(T, device=new.device, dtype=torch.float32)
    assert out.is_cuda and out.dtype == torch.float32 and out.numel() == T and out.is_contiguous(), "out: fp32 [T]"
    _lib.check(lib.lr_token_drift(_p(old), _p(new), T, D, _p(out), _stream()), "token_drift")
    return out


# ---- LoRA (csrc/lora.hip) -------------------------------------------------------------------------------------------
LORA_GRANULE = 32      # rank granule of the 16-bit LoRA kernels: the factors are zero-padded to 32 or 64


def lora_pad_rank(r):
    """Padded rank the 16-bit LoRA kernels run at (32 | 64)."""
    r = int(r)
    if not 1 <= r <= 64:
        raise ValueError(f"LoRA rank {r} is not supported: the HIP LoRA kernels take 1 <= r <= 64 (factors are zero-padded to the rank "
                         f"granule {LORA_GRANULE}, i.e. to 32 or 64)")
    return LORA_GRANULE * ((r + LORA_GRANULE - 1) // LORA_GRANULE)


def _rows16(t, name):
    assert (t.is_cuda and t.dtype in HALF_TYPES and t.dim() == 2 and t.stride(1) == 1 and t.stride(0) % 8 == 0
            and t.data_ptr() % 16 == 0), f"{name}: cuda fp16 / bf16 [rows, cols], unit column stride, 16-byte aligned rows"


class LoraDrop:
    """The dropout mask of one LoRA layer at one draw, as the `drop=` argument of lora_down / lora_up / lora_wgrad (struct lr_lora_drop;
    leftrefill_amd.lora_dropout states the mask).  colgrp: int32 device table [columns / 4] of the logical group of four columns behind each
    stored group (lora_dropout.colgrp_of), None = identity."""

    def __init__(self, seed, stream, draw, p, colgrp=None, threshold=None, inv_keep=None):
        from . import lora_dropout
        self.p, self.colgrp = float(p), colgrp
        if colgrp is not None:
            assert colgrp.is_cuda and colgrp.dtype == torch.int32 and colgrp.is_contiguous()
        self.c = _lib.LoraDrop(int(seed) & (2 ** 64 - 1), int(stream) & 0xFFFFFFFF, int(draw) & 0xFFFFFFFF,
                               lora_dropout.threshold(p) if threshold is None else int(threshold),
                               lora_dropout.inv_keep(p) if inv_keep is None else float(inv_keep),
                               None if colgrp is None else colgrp.data_ptr())

    @property
    def inv_keep(self):
        return float(self.c.inv_keep)

    def ref(self, columns):
        assert self.colgrp is None or self.colgrp.numel() * 4 == columns, "colgrp: one entry per four columns of the masked operand"
        return ctypes.byref(self.c)


def lora_down(x, a, alpha=1.0, out=None, drop=None):
    """lr_lora_down: t [M, R] = alpha * x [M, K] . a [R, K]^T (R = padded rank 32 | 64; x may be a column slice of a wider buffer).
    drop (LoraDrop): lr_lora_down_drop, x masked at its own (row, column)."""
    lib = _lib.load()
    _rows16(x, "x")
    _rows16(a, "a")
    M, K = x.shape
    R = a.shape[0]
    assert a.shape[1] == K and a.dtype == x.dtype
    if out is None:
        out = torch.empty(M, R, device=x.device, dtype=x.dtype)
    _rows16(out, "out")
    assert out.shape == (M, R) and out.dtype == x.dtype
    if drop is not None:
        _lib.check(_fn(lib, "lr_lora_down_drop_f16", x.dtype)(_p(x), x.stride(0), _p(a), a.stride(0), _p(out), out.stride(0), M, K, R,
                                                             float(alpha), drop.ref(K), _stream()), "lora_down_drop")
        return out
    _lib.check(_fn(lib, "lr_lora_down_f16", x.dtype)(_p(x), x.stride(0), _p(a), a.stride(0), _p(out), out.stride(0), M, K, R, float(alpha),
                                                    _stream()), "lora_down")
    return out


def lora_up(t, u, out=None, accumulate=False, drop=None):
    """lr_lora_up: out [M, N] (+)= t [M, R] . u [N, R]^T; `out` may be a column slice of a wider buffer (accumulate adds to what it holds).
    drop (LoraDrop): lr_lora_up_drop, the product masked (and scaled by inv_keep) at out's own (row, column)."""
    lib = _lib.load()
    _rows16(t, "t")
    _rows16(u, "u")
    M, R = t.shape
    N = u.shape[0]
    assert u.shape[1] == R and u.dtype == t.dtype
    if out is None:
        assert not accumulate, "accumulate needs out="
        out = torch.empty(M, N, device=t.device, dtype=t.dtype)
    _rows16(out, "out")
    assert out.shape == (M, N) and out.dtype == t.dtype
    if drop is not None:
        _lib.check(_fn(lib, "lr_lora_up_drop_f16", t.dtype)(_p(t), t.stride(0), _p(u), u.stride(0), _p(out), out.stride(0), M, N, R,
                                                           int(bool(accumulate)), drop.ref(N), _stream()), "lora_up_drop")
        return out
    _lib.check(_fn(lib, "lr_lora_up_f16", t.dtype)(_p(t), t.stride(0), _p(u), u.stride(0), _p(out), out.stride(0), M, N, R,
                                                  int(bool(accumulate)), _stream()), "lora_up")
    return out


def lora_wgrad_workspace(M, R, C, device):
    """fp32 workspace of lr_lora_wgrad for the shape (lr_lora_wgrad_workspace_bytes)."""
    nbytes = _lib.load().lr_lora_wgrad_workspace_bytes(M, R, C)
    if nbytes < 0:
        _lib.check(int(nbytes), "lora_wgrad_workspace_bytes")
    return torch.empty(nbytes // 4, device=device, dtype=torch.float32)


def lora_wgrad(p, q, alpha=1.0, out=None, workspace=None, drop=None):
    """lr_lora_wgrad: d [R, C] fp32 = alpha * p [M, R]^T . q [M, C] (fixed-order split over M, no atomics).  out / workspace
    (lora_wgrad_workspace): buffers of a caller that keeps them.  drop (LoraDrop): lr_lora_wgrad_drop, q masked at its own (row, column)."""
    lib = _lib.load()
    _rows16(p, "p")
    _rows16(q, "q")
    M, R = p.shape
    C = q.shape[1]
    assert q.shape[0] == M and q.dtype == p.dtype
    ws = lora_wgrad_workspace(M, R, C, p.device) if workspace is None else workspace
    d = torch.empty(R, C, device=p.device, dtype=torch.float32) if out is None else out
    assert ws.is_cuda and ws.dtype == torch.float32 and ws.is_contiguous() and d.is_cuda and d.dtype == torch.float32 and d.shape == (R, C) \
        and d.is_contiguous()
    if drop is not None:
        _lib.check(_fn(lib, "lr_lora_wgrad_drop_f16", p.dtype)(_p(p), p.stride(0), _p(q), q.stride(0), _p(d), C, M, R, C, float(alpha), _p(ws),
                                                              ws.numel() * 4, drop.ref(C), _stream()), "lora_wgrad_drop")
        return d
    _lib.check(_fn(lib, "lr_lora_wgrad_f16", p.dtype)(_p(p), p.stride(0), _p(q), q.stride(0), _p(d), C, M, R, C, float(alpha), _p(ws),
                                                     ws.numel() * 4, _stream()), "lora_wgrad")
    return d


def lora_merge(w, up, down, alpha=1.0):
    """lr_lora_merge_f32: w [N, K] + alpha * up [N, r] . down [r, K], all fp32 (a new tensor)."""
    lib = _lib.load()
    w, up, down = (t.detach().float().contiguous() for t in (w, up, down))
    N, K = w.shape
    r = up.shape[1]
    assert w.is_cuda and up.shape == (N, r) and down.shape == (r, K)
    if not 1 <= r <= 64:
        lora_pad_rank(r)
    out = torch.empty_like(w)
    _lib.check(lib.lr_lora_merge_f32(_p(w), _p(up), _p(down), _p(out), N, K, r, float(alpha), _stream()), "lora_merge")
    return out
