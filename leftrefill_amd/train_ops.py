"""Differentiable front end of the HIP operators (training with frozen weights: input gradients only).

Same call signatures as `leftrefill_amd.ops`; every function falls straight through to `ops` unless autograd is recording
and an input requires grad, in which case it runs as a `torch.autograd.Function` whose backward is made of HIP kernels:

  conv / linear    dX = lr_gemm_conv_f16 on flipped, transposed weights (stride 2: zero-insertion gather, `up = 2`;
                   nearest-up conv: dgrad at the fine resolution + lr_sumpool2x2); GEGLU: the training forward keeps the
                   projection (lr_geglu_fwd applies the gate), lr_geglu_bwd, then the same dgrad GEMM; plain GELU (text tower):
                   the same with lr_gelu_fwd_f16 / lr_gelu_bwd_f16
  GroupNorm(+SiLU) lr_groupnorm_stats (recomputed) + lr_groupnorm_bwd
  LayerNorm        lr_layernorm_bwd
  attention        lr_attention_bwd_f16 (flash-style recomputation from the saved log-sum-exp); causal (text tower):
                   lr_attention_causal_lse_f16 + lr_attention_causal_bwd_f16

  LoRA factors     lr_lora_down / lr_lora_up next to the base GEMM, lr_lora_wgrad for the two fp32 factor gradients (`lora_linear`)

torch.autograd only orchestrates (graph, fan-in sums of residual branches, `torch.utils.checkpoint` recomputation like
the reference's CheckpointFunction, ldm/modules/diffusionmodules/util.py:102-151); the base weights never receive gradients --
the optimizer of the reference owns only the prompt tokens (ref_inpainting_ldm.py:86-87), which sit upstream of `context`, and,
with `lora.do_lora`, the LoRA factors of the attention / GEGLU Linears (NVS_ldm.py:333-335).
"""
import torch

from . import _lib, ops
from .ops import *  # noqa: F401,F403  (re-export the non-differentiable entry points unchanged)
from .ops import _p, _stream
from ._lib import AttnBwdArgs


def _needs_grad(*ts):
    return torch.is_grad_enabled() and any(t is not None and t.requires_grad for t in ts)


def dgrad_weight(wt, taps, lo, hi):
    """Packed forward weight [N][taps*Ct] -> input-gradient weight [hi-lo][taps*N]: transposed, taps flipped.
    Cached ON the weight tensor (its lifetime, invalidated by in-place updates through `_version`)."""
    cache = wt.__dict__.setdefault("_lr_dgrad", {})
    key = (wt._version, taps, lo, hi)
    w = cache.get(key)
    if w is None:
        N = wt.shape[0]
        Ct = wt.shape[1] // taps
        w3 = wt.detach().reshape(N, taps, Ct)[:, :, lo:hi]
        w = w3.permute(2, 1, 0).flip(1).reshape(hi - lo, taps * N).contiguous()
        for k in [k for k in cache if k[0] != wt._version]:
            del cache[k]
        cache[key] = w
    return w


class _GemmConv(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x1, x2, resid, wt, bias, rowvec, kw):
        ctx.set_materialize_grads(False)      # (the statistics outputs carry no gradient: no zero tensors made for them)
        ctx.kw, ctx.wt, ctx.bias = kw, wt, bias
        ctx.C1 = x1.shape[-1]
        ctx.C2 = 0 if x2 is None else x2.shape[-1]
        ctx.has_resid = resid is not None
        if kw.get("geglu"):
            # training: keep the projection (u | g, packed layout) for the backward and apply the gate in a second kernel --
            # one elementwise pass now instead of recomputing the [M, 8C] GEMM later
            assert resid is None and rowvec is None
            pre = ops.gemm_conv(x1, wt, x2=x2, bias=bias, **{k: v for k, v in kw.items() if k != "geglu"})
            ctx.save_for_backward(pre)
            return geglu_fwd(pre)
        ctx.save_for_backward()                                            # plain conv / linear: dX needs only dY and W
        if kw.get("want_gn_stats"):
            # the producer-side GroupNorm statistics of the inference path (per-channel row-block partials + per-group sums): no
            # gradient flows through them, the consuming GroupNorm's backward re-derives mean / rstd from the same sums
            meta = kw.pop("_gs_meta")
            y, gs = ops.gemm_conv(x1, wt, x2=x2, bias=bias, rowvec=rowvec, resid=resid, **kw)
            if gs is None:
                return y, None, None
            meta[:] = [gs[1], gs[3]]
            ctx.mark_non_differentiable(*[t for t in (gs[0], gs[2]) if t is not None])
            return y, gs[0], gs[2]
        return ops.gemm_conv(x1, wt, x2=x2, bias=bias, rowvec=rowvec, resid=resid, **kw)

    @staticmethod
    def backward(ctx, dy, *_unused):
        kw, wt = ctx.kw, ctx.wt
        if dy is None:
            return None, None, None, None, None, None, None
        dy = dy.contiguous()
        B, H, W = kw["B"], kw["H"], kw["W"]
        Hs, Ws = kw.get("Hs") or H, kw.get("Ws") or W
        taps, stride, up = kw.get("taps", 1), kw.get("stride", 1), kw.get("up", 0)
        if kw.get("asym"):
            raise NotImplementedError("asymmetric-pad stride-2 conv (VAE encoder) has no backward: the VAE is frozen and not differentiated")
        g = dy
        if kw.get("geglu"):
            g = geglu_bwd(ctx.saved_tensors[0], dy)
        dxs = []
        for lo, hi in ((0, ctx.C1), (ctx.C1, ctx.C1 + ctx.C2)):
            if hi == lo or not ctx.needs_input_grad[0 if lo == 0 else 1]:
                dxs.append(None)
                continue
            wd = dgrad_weight(wt, taps, lo, hi)
            if taps == 1:
                dx = ops.gemm_conv(g, wd, B=1, H=1, W=B * H * W, taps=1)
            elif stride == 2:
                dx = ops.gemm_conv(g, wd, B=B, H=Hs, W=Ws, Hs=H, Ws=W, taps=9, up=2)
            elif up:
                fine = ops.gemm_conv(g, wd, B=B, H=H, W=W, taps=9)
                dx = sumpool2x2(fine, B, Hs, Ws)
            else:
                dx = ops.gemm_conv(g, wd, B=B, H=H, W=W, taps=9)
            dxs.append(dx)
        dresid = dy if ctx.has_resid and ctx.needs_input_grad[2] else None
        return dxs[0], dxs[1], dresid, None, None, None, None


class _ConvSkip(torch.autograd.Function):
    """3x3 conv with the pointwise skip_connection riding on its K loop (lr_gemm_args.skip1: `skip_connection(x) + conv(h)` of a width-changing
    ResBlock as ONE accumulation): the forward is the inference launch; the backward is three independent input-gradient GEMMs on the two
    layers' own packed weights (d h: 3x3 dgrad; d s1 / d s2: pointwise dgrads on the row slices of the skip weight)."""

    @staticmethod
    def forward(ctx, h, s1, s2, wf, bias, w_main, w_skip, kw):
        ctx.set_materialize_grads(False)
        ctx.kw, ctx.w_main, ctx.w_skip = kw, w_main, w_skip
        ctx.Cs1 = s1.shape[-1]
        ctx.Cs2 = 0 if s2 is None else s2.shape[-1]
        want = kw.pop("want_gn_stats", False)
        meta = kw.pop("_gs_meta", None)
        r = ops.gemm_conv(h, wf, bias=bias, skip=(s1, s2), want_gn_stats=want, **kw)
        if not want:
            return r
        y, gs = r
        if gs is None:
            return y, None, None
        meta[:] = [gs[1], gs[3]]
        ctx.mark_non_differentiable(*[t for t in (gs[0], gs[2]) if t is not None])
        return y, gs[0], gs[2]

    @staticmethod
    def backward(ctx, dy, *_unused):
        if dy is None:
            return (None,) * 8
        kw = ctx.kw
        dy = dy.contiguous()
        B, H, W = kw["B"], kw["H"], kw["W"]
        M = B * H * W
        dh = ds1 = ds2 = None
        if ctx.needs_input_grad[0]:
            Ch = ctx.w_main.shape[1] // 9
            dh = ops.gemm_conv(dy, dgrad_weight(ctx.w_main, 9, 0, Ch), B=B, H=H, W=W, taps=9)
        if ctx.needs_input_grad[1]:
            ds1 = ops.gemm_conv(dy, dgrad_weight(ctx.w_skip, 1, 0, ctx.Cs1), B=1, H=1, W=M, taps=1)
        if ctx.Cs2 and ctx.needs_input_grad[2]:
            ds2 = ops.gemm_conv(dy, dgrad_weight(ctx.w_skip, 1, ctx.Cs1, ctx.Cs1 + ctx.Cs2), B=1, H=1, W=M, taps=1)
        return dh, ds1, ds2, None, None, None, None, None


def gemm_conv(x1, wt, *, x2=None, bias=None, rowvec=None, resid=None, skip_parts=None, **kw):
    """skip_parts = (packed 3x3 weight, packed pointwise skip weight): the two layers of a skip-extended conv (`skip=`) on their own -- what its
    backward multiplies by; without them a skip-extended conv cannot be differentiated."""
    sk = kw.get("skip") or ()
    if not _needs_grad(x1, x2, resid, *[t for t in sk if t is not None]):
        return ops.gemm_conv(x1, wt, x2=x2, bias=bias, rowvec=rowvec, resid=resid, **kw)
    if sk:
        if skip_parts is None or x2 is not None or rowvec is not None or resid is not None or kw.get("taps") != 9 or kw.get("stride", 1) != 1 or kw.get("up"):
            raise NotImplementedError("a K-extended GEMM (skip=) is differentiable only as a plain 3x3 conv + pointwise skip with skip_parts=")
        kw = dict(kw)
        s1, s2 = kw.pop("skip")
        if kw.get("want_gn_stats"):
            meta = kw["_gs_meta"] = []
            y, part, gp = _ConvSkip.apply(x1, s1, s2, wt, bias, skip_parts[0], skip_parts[1], kw)
            return y, (None if part is None else (part, meta[0], gp, meta[1]))
        kw.pop("want_gn_stats", None)
        return _ConvSkip.apply(x1, s1, s2, wt, bias, skip_parts[0], skip_parts[1], kw)
    if kw.get("ln") is not None:
        raise NotImplementedError("the LayerNorm-folded GEMM is an inference kernel; differentiate layer_norm + gemm_conv")
    if kw.pop("want_stats", False):                                     # row statistics feed the LayerNorm fold: inference only
        kw.pop("want_gn_stats", None)
        return gemm_conv(x1, wt, x2=x2, bias=bias, rowvec=rowvec, resid=resid, **kw), None
    if kw.get("want_gn_stats") and (kw.get("geglu") or kw.get("gelu") or kw.get("out") is not None):
        kw.pop("want_gn_stats")
        return gemm_conv(x1, wt, x2=x2, bias=bias, rowvec=rowvec, resid=resid, **kw), None
    if rowvec is not None and rowvec.requires_grad:
        raise NotImplementedError("gradient w.r.t. the time embedding is not produced (nothing trainable sits upstream of it)")
    if kw.get("out") is not None:
        raise ValueError("out= is not supported while autograd is recording")
    if kw.get("gelu"):
        # training: the GEMM without its GELU epilogue, `pre` kept for lr_gelu_bwd (as the GEGLU projection keeps its own)
        if rowvec is not None or resid is not None or kw.get("want_gn_stats"):
            raise NotImplementedError("the differentiable GELU GEMM takes no rowvec / resid / statistics outputs")
        kw = {k: v for k, v in kw.items() if k != "gelu"}
        return _Gelu.apply(_GemmConv.apply(x1, x2, None, wt, bias, None, kw))
    if kw.get("want_gn_stats"):
        meta = kw["_gs_meta"] = []
        y, part, gp = _GemmConv.apply(x1, x2, resid, wt, bias, rowvec, kw)
        return y, (None if part is None else (part, meta[0], gp, meta[1]))
    kw.pop("want_gn_stats", None)
    return _GemmConv.apply(x1, x2, resid, wt, bias, rowvec, kw)


def geglu_fwd(pre):
    lib = _lib.load()
    M, H2 = pre.shape
    out = torch.empty(M, H2 // 2, device=pre.device, dtype=pre.dtype)
    _lib.check(_lib.fn(lib, "lr_geglu_fwd", pre.dtype)(_p(pre), _p(out), M, H2 // 2, _stream()), "geglu_fwd")
    return out


def geglu_bwd(pre, dy):
    lib = _lib.load()
    M, H = dy.shape
    assert pre.shape == (M, 2 * H) and pre.is_contiguous() and dy.is_contiguous()
    dpre = torch.empty_like(pre)
    _lib.check(_lib.fn(lib, "lr_geglu_bwd", pre.dtype)(_p(pre), _p(dy), _p(dpre), M, H, _stream()), "geglu_bwd")
    return dpre


def gelu_fwd(pre):
    """y = gelu(pre): the erf-GELU of the fused epilogue as its own pass (lr_gelu_fwd_f16)."""
    lib = _lib.load()
    assert pre.is_contiguous()
    y = torch.empty_like(pre)
    _lib.check(_lib.fn(lib, "lr_gelu_fwd_f16", pre.dtype)(_p(pre), _p(y), pre.numel(), _stream()), "gelu_fwd")
    return y


def gelu_bwd(pre, dy):
    """dpre = dy * gelu'(pre) (lr_gelu_bwd_f16)."""
    lib = _lib.load()
    assert pre.is_contiguous() and dy.is_contiguous() and dy.shape == pre.shape and dy.dtype == pre.dtype
    dpre = torch.empty_like(pre)
    _lib.check(_lib.fn(lib, "lr_gelu_bwd_f16", pre.dtype)(_p(pre), _p(dy), _p(dpre), pre.numel(), _stream()), "gelu_bwd")
    return dpre


class _Gelu(torch.autograd.Function):
    @staticmethod
    def forward(ctx, pre):
        ctx.save_for_backward(pre)
        return gelu_fwd(pre)

    @staticmethod
    def backward(ctx, dy):
        return gelu_bwd(ctx.saved_tensors[0], dy.contiguous())


def sumpool2x2(x, N, H, W):
    """x [N*2H*2W, C] -> [N*H*W, C]: backward of the nearest-2x upsample."""
    lib = _lib.load()
    C = x.shape[-1]
    assert x.shape[0] == N * 4 * H * W and x.is_contiguous()
    y = torch.empty(N * H * W, C, device=x.device, dtype=x.dtype)
    _lib.check(_lib.fn(lib, "lr_sumpool2x2", x.dtype)(_p(x), _p(y), N, H, W, C, _stream()), "sumpool2x2")
    return y


class _GroupNorm(torch.autograd.Function):
    """GroupNorm(32)(+SiLU) over the virtual concat [x1 | x2].
    stats: None (statistics pass), ("groups", gp [N, chunks, 32, 2], chunks) = per-group sums of x1 out of its producer's epilogue,
           or ("channels", gs1, gs2) = per-channel row-block partials of the source(s), reduced by lr_groupnorm_finalize.
    fork: also return x1 (and x2) as outputs -- the caller routes the residual branch (`x + f(GroupNorm(x))`, or the ResBlock's
          skip_connection) through them, so its gradient arrives HERE and is added inside the backward kernel (lr_groupnorm_bwd_res)
          instead of by a separate fan-in add of torch.autograd."""

    @staticmethod
    def forward(ctx, x1, x2, gamma, beta, N, HW, eps, silu, stats, fork):
        ctx.set_materialize_grads(False)      # an unused fork output arrives as None, not as a tensor of zeros
        lib = _lib.load()
        C1 = x1.shape[-1]
        C2 = 0 if x2 is None else x2.shape[-1]
        y = torch.empty(N * HW, C1 + C2, device=x1.device, dtype=x1.dtype)
        st = _stream()
        if stats is None:
            partials, chunks = torch.empty(N * ops.GN_CHUNKS * 64, device=x1.device, dtype=torch.float32), 0
            _lib.check(_lib.fn(lib, "lr_groupnorm_stats", x1.dtype)(_p(x1), C1, _p(x2), C2, N, HW, _p(partials), st), "groupnorm_stats")
        elif stats[0] == "groups":
            assert x2 is None
            partials, chunks = stats[1], stats[2]
            assert partials.dtype == torch.float32 and partials.is_contiguous() and partials.shape == (N, chunks, 32, 2)
        else:
            gs1, gs2 = stats[1], stats[2]
            p1, r1 = gs1[:2]
            p2, r2 = gs2[:2] if x2 is not None else (None, 1)
            assert p1.shape == (N * HW // r1, C1, 2) and HW % r1 == 0 and (x2 is None or (p2.shape == (N * HW // r2, C2, 2) and HW % r2 == 0))
            partials, chunks = torch.empty(N * 64, device=x1.device, dtype=torch.float32), 1
            _lib.check(lib.lr_groupnorm_finalize(_p(p1), C1, r1, _p(p2), C2, r2, N, HW, _p(partials), st), "groupnorm_finalize")
        if chunks == 0:
            _lib.check(_lib.fn(lib, "lr_groupnorm_apply", x1.dtype)(_p(x1), C1, _p(x2), C2, N, HW, _p(partials), _p(gamma), _p(beta),
                                                                  float(eps), int(bool(silu)), _p(y), st), "groupnorm_apply")
        else:
            _lib.check(_lib.fn(lib, "lr_groupnorm_apply_n", x1.dtype)(_p(x1), C1, _p(x2), C2, N, HW, _p(partials), chunks, _p(gamma),
                                                                    _p(beta), float(eps), int(bool(silu)), _p(y), st), "groupnorm_apply_n")
        ctx.save_for_backward(x1, x2, gamma, beta, partials)
        ctx.meta = (N, HW, float(eps), int(bool(silu)), chunks)
        if fork:
            return y, x1, x2
        return y

    @staticmethod
    def backward(ctx, dy, d1=None, d2=None):
        lib = _lib.load()
        x1, x2, gamma, beta, partials = ctx.saved_tensors
        N, HW, eps, silu, chunks = ctx.meta
        C1 = x1.shape[-1]
        C2 = 0 if x2 is None else x2.shape[-1]
        if dy is None:      # only the residual branch carries a gradient
            return d1, d2, None, None, None, None, None, None, None, None
        dy = dy.contiguous()
        d1 = None if d1 is None else d1.contiguous()
        d2 = None if d2 is None else d2.contiguous()
        scratch = torch.empty(N * ops.GN_CHUNKS * 64, device=x1.device, dtype=torch.float32)
        dx1 = torch.empty_like(x1)
        dx2 = None if x2 is None else torch.empty_like(x2)
        _lib.check(_lib.fn(lib, "lr_groupnorm_bwd_res", x1.dtype)(_p(x1), C1, _p(x2), C2, _p(dy), _p(d1), _p(d2), N, HW, _p(partials), chunks,
                                                                _p(gamma), _p(beta), eps, silu, _p(scratch), _p(dx1), _p(dx2), _stream()),
                   "groupnorm_bwd_res")
        return dx1, dx2, None, None, None, None, None, None, None, None


def group_norm(x1, N, HW, gamma, beta, eps, silu, x2=None, stats=None):
    if not _needs_grad(x1, x2):
        assert stats is None
        return ops.group_norm(x1, N, HW, gamma, beta, eps, silu, x2)
    return _GroupNorm.apply(x1.contiguous(), None if x2 is None else x2.contiguous(), gamma, beta, N, HW, eps, silu, stats, False)


def group_norm_fork(x1, N, HW, gamma, beta, eps, silu, x2=None, stats=None):
    """(GroupNorm(...), x1', x2'): x1' / x2' are x1 / x2 for the residual branch around the GroupNorm (see _GroupNorm)."""
    assert _needs_grad(x1, x2)
    return _GroupNorm.apply(x1.contiguous(), None if x2 is None else x2.contiguous(), gamma, beta, N, HW, eps, silu, stats, True)


class _LayerNorm(torch.autograd.Function):
    """fork: also return x as an output -- the residual `x + f(LayerNorm(x))` is taken from it, so the residual branch's gradient is
    added inside the backward kernel (lr_layernorm_bwd_res) instead of by a separate fan-in add of torch.autograd."""

    @staticmethod
    def forward(ctx, x, gamma, beta, eps, fork):
        ctx.set_materialize_grads(False)
        y = ops.layer_norm(x, gamma, beta, eps)
        ctx.save_for_backward(x, gamma)
        ctx.eps = float(eps)
        return (y, x) if fork else y

    @staticmethod
    def backward(ctx, dy, dres=None):
        lib = _lib.load()
        x, gamma = ctx.saved_tensors
        if dy is None:
            return dres, None, None, None, None
        dy = dy.contiguous()
        dres = None if dres is None else dres.contiguous()
        dx = torch.empty_like(x)
        M, C = x.shape
        _lib.check(_lib.fn(lib, "lr_layernorm_bwd_res", x.dtype)(_p(x), _p(dy), _p(dres), _p(gamma), ctx.eps, _p(dx), M, C, _stream()),
                   "layernorm_bwd_res")
        return dx, None, None, None, None


def layer_norm(x, gamma, beta, eps=1e-5):
    if not _needs_grad(x):
        return ops.layer_norm(x, gamma, beta, eps)
    return _LayerNorm.apply(x.contiguous(), gamma, beta, eps, False)


def layer_norm_fork(x, gamma, beta, eps=1e-5):
    """(LayerNorm(x), x'): use x' for the residual add behind the branch (see _LayerNorm); plain (LayerNorm(x), x) without autograd."""
    if not _needs_grad(x):
        return ops.layer_norm(x, gamma, beta, eps), x
    return _LayerNorm.apply(x.contiguous(), gamma, beta, eps, True)


class _ToNCHW(torch.autograd.Function):
    @staticmethod
    def forward(ctx, y, N, H, W, C, out_dtype):
        ctx.meta = (y.shape[-1], y.dtype)
        return ops.nhwc_to_nchw(y, N, H, W, C, out_dtype)

    @staticmethod
    def backward(ctx, dout):
        # the gradient takes the activation's 16-bit type: an fp16 detour would flush the unscaled bf16 gradients
        # (~1e-6 at training sizes) to zero before autograd casts them back
        return ops.nchw_to_nhwc(dout.float().contiguous(), cpad=ctx.meta[0], dtype=ctx.meta[1]), None, None, None, None, None


def nhwc_to_nchw(y, N, H, W, C, out_dtype=None):
    if not _needs_grad(y):
        return ops.nhwc_to_nchw(y, N, H, W, C, out_dtype)
    return _ToNCHW.apply(y, N, H, W, C, out_dtype)


ATTN_BWD_QSPLIT = __import__("os").environ.get("LEFTREFILL_ATTN_BWD_QSPLIT", "1") != "0"


def attn_bwd_q_splits(B, heads, Nq, Nkv):
    """Query slices of the dK / dV kernel (lr_attn_bwd_args.ld_qt): 1 unless its (batch, head, key block) grid leaves most of the 256 CUs
    idle while every block walks >= 8 query tiles -- then enough slices to fill the chip once, at least 4 tiles each.  A pure function of
    the shape (the sum order of the slices is fixed)."""
    blocks = B * heads * ((Nkv + 127) // 128)
    tiles = (Nq + 63) // 64
    if not ATTN_BWD_QSPLIT or blocks > 128 or tiles < 8:
        return 1
    return max(1, min(256 // blocks, tiles // 4, 64))


def _attention_backward(q, k, v, out, lse, dout, meta, dq, dk, dv, causal=False):
    """dq / dk / dv: pre-allocated (possibly strided column-slice) outputs.  causal: lr_attention_causal_bwd_f16 (no query split)."""
    lib = _lib.load()
    B, heads, Nq, Nkv, scale = meta
    dout = dout.contiguous()
    dsum = torch.empty_like(lse)
    a = AttnBwdArgs()
    a.q, a.k, a.v, a.o, a.dout = _p(q), _p(k), _p(v), _p(out), _p(dout)
    a.qt, a.kt, a.dot, a.lse, a.dsum = 0, 0, 0, _p(lse), _p(dsum)       # (no transposed copies since ABI 25: LDS transpose reads)
    qs, ws = (1 if causal else attn_bwd_q_splits(B, heads, Nq, Nkv)), None
    if qs > 1:      # few key blocks against many queries (the level-0 cross-attention): the dK / dV kernel's query tiles split over more blocks
        ws = torch.empty(qs * B * heads * ((Nkv + 127) // 128) * 2 * 128 * 64, device=q.device, dtype=torch.float32)
        a.qt = _p(ws)
    a.dq, a.dk, a.dv = _p(dq), _p(dk), _p(dv)
    a.ldq, a.ldk, a.ldv, a.ldo, a.lddo = q.stride(0), k.stride(0), v.stride(0), out.stride(0), dout.stride(0)
    a.ld_qt, a.ld_kt = (qs if qs > 1 else 0), 0
    a.lddq, a.lddk, a.lddv = dq.stride(0), dk.stride(0), dv.stride(0)
    a.B, a.heads, a.Nq, a.Nkv, a.scale = B, heads, Nq, Nkv, scale
    name = "lr_attention_causal_bwd_f16" if causal else "lr_attention_bwd_f16"
    _lib.check(_lib.fn(lib, name, q.dtype)(a, _stream()), "attention_bwd")


def _attention_forward(q, k, v, B, heads, Nq, Nkv, scale):
    lib = _lib.load()
    out = torch.empty(B * Nq, heads * 64, device=q.device, dtype=q.dtype)
    lse = torch.empty(B * heads * Nq, device=q.device, dtype=torch.float32)
    _lib.check(_lib.fn(lib, "lr_attention_lse_f16", q.dtype)(_p(q), q.stride(0), _p(k), k.stride(0), _p(v), v.stride(0), _p(out), out.stride(0),
                                        _p(lse), B, heads, Nq, Nkv, float(scale), _stream()), "attention_lse")
    return out, lse


class _Attention(torch.autograd.Function):
    @staticmethod
    def forward(ctx, q, k, v, B, heads, Nq, Nkv, scale):
        out, lse = _attention_forward(q, k, v, B, heads, Nq, Nkv, scale)
        ctx.save_for_backward(q, k, v, out, lse)
        ctx.meta = (B, heads, Nq, Nkv, float(scale))
        return out

    @staticmethod
    def backward(ctx, dout):
        q, k, v, out, lse = ctx.saved_tensors
        B, heads, Nq, Nkv, _ = ctx.meta
        C = heads * 64
        dq = torch.empty(B * Nq, C, device=q.device, dtype=q.dtype)
        dk = torch.empty(B * Nkv, C, device=q.device, dtype=q.dtype)
        dv = torch.empty(B * Nkv, C, device=q.device, dtype=q.dtype)
        _attention_backward(q, k, v, out, lse, dout, ctx.meta, dq, dk, dv)
        return dq, dk, dv, None, None, None, None, None


class _AttentionQKV(torch.autograd.Function):
    """Self-attention on the fused [q | k | v] projection: the three gradients land in ONE [M, 3C] buffer."""

    @staticmethod
    def forward(ctx, qkv, B, heads, L, scale):
        C = heads * 64
        out, lse = _attention_forward(qkv[:, :C], qkv[:, C:2 * C], qkv[:, 2 * C:], B, heads, L, L, scale)
        ctx.save_for_backward(qkv, out, lse)
        ctx.meta = (B, heads, L, L, float(scale))
        return out

    @staticmethod
    def backward(ctx, dout):
        qkv, out, lse = ctx.saved_tensors
        C = ctx.meta[1] * 64
        d = torch.empty_like(qkv)
        _attention_backward(qkv[:, :C], qkv[:, C:2 * C], qkv[:, 2 * C:], out, lse, dout, ctx.meta, d[:, :C], d[:, C:2 * C],
                            d[:, 2 * C:])
        return d, None, None, None, None


class _AttentionQ_KV(torch.autograd.Function):
    """Cross-attention: q plus the fused [k | v] context projection."""

    @staticmethod
    def forward(ctx, q, kv, B, heads, Nq, Nkv, scale):
        C = heads * 64
        out, lse = _attention_forward(q, kv[:, :C], kv[:, C:], B, heads, Nq, Nkv, scale)
        ctx.save_for_backward(q, kv, out, lse)
        ctx.meta = (B, heads, Nq, Nkv, float(scale))
        return out

    @staticmethod
    def backward(ctx, dout):
        q, kv, out, lse = ctx.saved_tensors
        C = ctx.meta[1] * 64
        dq = torch.empty_like(q)
        dkv = torch.empty_like(kv)
        _attention_backward(q, kv[:, :C], kv[:, C:], out, lse, dout, ctx.meta, dq, dkv[:, :C], dkv[:, C:])
        return dq, dkv, None, None, None, None, None


class _SplitCols(torch.autograd.Function):
    """x [M, sum sizes] -> column-slice views; the backward concatenates the slices' gradients (ONE copy launch) instead of
    scattering each of them into a zero tensor of the full width and summing those."""

    @staticmethod
    def forward(ctx, x, sizes):
        ctx.set_materialize_grads(False)
        ctx.sizes, ctx.rows = tuple(sizes), x.shape[0]
        outs, off = [], 0
        for n in sizes:
            outs.append(x[:, off:off + n])
            off += n
        assert off == x.shape[1]
        return tuple(outs)

    @staticmethod
    def backward(ctx, *grads):
        ref = next(g for g in grads if g is not None)
        parts = [g if g is not None else ref.new_zeros(ctx.rows, n) for g, n in zip(grads, ctx.sizes)]
        return torch.cat(parts, dim=1), None


def split_cols(x, sizes):
    if not _needs_grad(x):
        outs, off = [], 0
        for n in sizes:
            outs.append(x[:, off:off + n])
            off += n
        return tuple(outs)
    return _SplitCols.apply(x, tuple(sizes))


def _rows_ok(t):
    """[rows, cols] with unit column stride and 16-byte aligned rows (a column slice of a wider buffer): the attention kernels take it as is."""
    return t.dim() == 2 and t.stride(1) == 1 and t.stride(0) % 8 == 0 and t.data_ptr() % 16 == 0


def attention(q, k, v, B, heads, Nq, Nkv, scale, out=None, vt=None):
    if not _needs_grad(q, k, v):
        return ops.attention(q, k, v, B, heads, Nq, Nkv, scale, out=out, vt=vt)
    return _Attention.apply(q, k, v, B, heads, Nq, Nkv, scale)


def attention_qkv(qkv, B, heads, L, scale):
    if not _needs_grad(qkv):
        return ops.attention_qkv(qkv, B, heads, L, scale)
    return _AttentionQKV.apply(qkv.contiguous(), B, heads, L, scale)


def attention_q_kv(q, kv, B, heads, Nq, Nkv, scale, vt=None):
    if not _needs_grad(q, kv):
        return ops.attention_q_kv(q, kv, B, heads, Nq, Nkv, scale, vt=vt)
    return _AttentionQ_KV.apply(q.contiguous(), kv if _rows_ok(kv) else kv.contiguous(), B, heads, Nq, Nkv, scale)


class _AttentionCausal(torch.autograd.Function):
    """Causal self-attention of the text tower (query i sees keys <= i) on the fused in_proj output qkv [M, 3C] (q | k | v column blocks):
    the three gradients land in ONE [M, 3C] buffer."""

    @staticmethod
    def forward(ctx, qkv, B, heads, N, scale):
        lib = _lib.load()
        C = heads * 64
        q, k, v = qkv[:, :C], qkv[:, C:2 * C], qkv[:, 2 * C:]
        out = torch.empty(B * N, C, device=q.device, dtype=q.dtype)
        lse = torch.empty(B * heads * N, device=q.device, dtype=torch.float32)
        _lib.check(_lib.fn(lib, "lr_attention_causal_lse_f16", q.dtype)(_p(q), q.stride(0), _p(k), k.stride(0), _p(v), v.stride(0), _p(out),
                                                                       out.stride(0), _p(lse), B, heads, N, float(scale), _stream()),
                   "attention_causal_lse")
        ctx.save_for_backward(qkv, out, lse)
        ctx.meta = (B, heads, N, N, float(scale))
        return out

    @staticmethod
    def backward(ctx, dout):
        qkv, out, lse = ctx.saved_tensors
        C = ctx.meta[1] * 64
        d = torch.empty_like(qkv)
        _attention_backward(qkv[:, :C], qkv[:, C:2 * C], qkv[:, 2 * C:], out, lse, dout, ctx.meta, d[:, :C], d[:, C:2 * C],
                            d[:, 2 * C:], causal=True)
        return d, None, None, None, None


def _fused_qkv(q, k, v, C):
    """The [M, 3C] tensor q / k / v are the three column blocks of, or None."""
    base = q._base
    if base is None or k._base is not base or v._base is not base or base.dim() != 2 or base.shape[1] != 3 * C:
        return None
    if not base.is_contiguous() or q.shape != (base.shape[0], C) or k.shape != q.shape or v.shape != q.shape:
        return None
    e = base.element_size()
    p0 = base.data_ptr()
    return base if (q.data_ptr(), k.data_ptr(), v.data_ptr()) == (p0, p0 + C * e, p0 + 2 * C * e) else None


def attention_causal(q, k, v, B, heads, N, scale):
    """Causal self-attention on [B*N, heads*64] column slices (ops.attention_causal); differentiable when an input requires grad.  The text
    tower passes the three column blocks of its fused in_proj output: the backward then writes one [M, 3C] gradient."""
    if not _needs_grad(q, k, v):
        return ops.attention_causal(q, k, v, B, heads, N, scale)
    C = heads * 64
    qkv = _fused_qkv(q, k, v, C)
    if qkv is None:
        qkv = torch.cat([q, k, v], dim=1)
    return _AttentionCausal.apply(qkv, B, heads, N, scale)


class _MvGather(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, b, v, s):
        ctx.meta = (b, v, s)
        return ops.mv_gather(x, b, v, s)

    @staticmethod
    def backward(ctx, dseq):
        lib = _lib.load()
        b, v, s = ctx.meta
        dseq = dseq.contiguous()
        C = dseq.shape[-1]
        dx = torch.empty(b * v * s * 2 * s, C, device=dseq.device, dtype=dseq.dtype)
        _lib.check(_lib.fn(lib, "lr_mv_gather_bwd", dseq.dtype)(_p(dseq), _p(dx), b, v, s, C, _stream()), "mv_gather_bwd")
        return dx, None, None, None


class _MvScatter(torch.autograd.Function):
    @staticmethod
    def forward(ctx, seq, b, v, s):
        ctx.meta = (b, v, s)
        return ops.mv_scatter(seq, b, v, s)

    @staticmethod
    def backward(ctx, dx):
        lib = _lib.load()
        b, v, s = ctx.meta
        dx = dx.contiguous()
        C = dx.shape[-1]
        dseq = torch.empty(b * (v + 1) * s * s, C, device=dx.device, dtype=dx.dtype)
        _lib.check(_lib.fn(lib, "lr_mv_scatter_bwd", dx.dtype)(_p(dx), _p(dseq), b, v, s, C, _stream()), "mv_scatter_bwd")
        return dseq, None, None, None


def xattn_block(*a, **k):
    """Fused cross-attention block: inference only (engine.cross_attention takes it only when nothing requires grad); looked up
    on `ops` at call time like every wrapper here, so instrumentation that patches ops.xattn_block sees the launches."""
    assert not _needs_grad(a[0])
    return ops.xattn_block(*a, **k)


def ffn_block(*a, **k):
    """Fused feed-forward block: inference only, looked up on `ops` at call time (see xattn_block)."""
    assert not _needs_grad(a[0])
    return ops.ffn_block(*a, **k)


def rowlin(*a, **k):
    """Row-resident LayerNorm + Linear at C = 640: inference only, looked up on `ops` at call time (see xattn_block)."""
    assert not _needs_grad(a[0])
    return ops.rowlin(*a, **k)


def stin_block(*a, **k):
    """Fused SpatialTransformer entry (proj_in + LayerNorm + q|k|v): inference only, looked up on `ops` at call time (see xattn_block)."""
    assert not _needs_grad(a[0])
    return ops.stin_block(*a, **k)


def mv_gather(x, b, v, s):
    return _MvGather.apply(x, b, v, s) if _needs_grad(x) else ops.mv_gather(x, b, v, s)


def mv_scatter(seq, b, v, s):
    return _MvScatter.apply(seq, b, v, s) if _needs_grad(seq) else ops.mv_scatter(seq, b, v, s)


# ---- LoRA: the first weight gradients of this package (csrc/lora.hip) ---------------------------------------------------------------
def _operand16(f, axis, R, dtype):
    """The fp32 factor (or a view of it: transposed, row-permuted) as a contiguous 16-bit kernel operand, zero-padded along its rank
    `axis` to R: one fill and one converting copy."""
    shape = list(f.shape)
    shape[axis] = R
    buf = torch.zeros(shape, device=f.device, dtype=dtype)
    buf.narrow(axis, 0, f.shape[axis]).copy_(f)
    return buf


class _LoraLinear(torch.autograd.Function):
    """y = x W^T (+ bias) (+ resid) + sum_i  (x down_i^T) (scale_i up_i)^T  added into the column range of segment i; with `geglu` the
    GEGLU gate follows (W, bias and the `up` rows in the packed u | g order).  One node for a whole fused projection ([q | k | v],
    [k | v], every cross-attention's [k | v] of TRAIN_KV_BATCH): the fp32 factors are inputs, read (and cast to the 16-bit operands) at
    every forward -- the optimizer writes them through raw pointers, no `_version` would tell.

    backward: dx = g W (the base input-gradient GEMM) + sum_i dT_i down_i (lr_lora_up, accumulate), dT_i = scale_i g_i up_i (lr_lora_down);
              d up_i^T = scale_i T_i^T g_i,  d down_i = dT_i^T x  (lr_lora_wgrad: fp32, fixed-order split sums, no atomics).
    Saved: x and every T_i = x down_i^T (16-bit, [M, padded rank]); the GEGLU form also keeps the projection, as _GemmConv does.

    LoRA dropout (a segment whose meta carries (seed, stream, draw, p, colgrp)): y_i += scale_i inv_keep (T_i up_i^T) (.) keep_i through
    lr_lora_up_drop; backward dT_i = scale_i inv_keep (g_i (.) keep_i) up_i (lr_lora_down_drop) and d up_i^T = scale_i inv_keep T_i^T
    (g_i (.) keep_i) (lr_lora_wgrad_drop); d down_i and dx take dT_i as they are, the base GEMM the unmasked g.  The mask is regenerated
    from the meta's numbers in every launch -- nothing is saved, and a recomputed forward sees the draw it was given."""

    @staticmethod
    def forward(ctx, x, resid, wt, bias, meta, *factors):
        ctx.set_materialize_grads(False)
        segs, geglu = meta
        x = x.contiguous()
        M = x.shape[0]
        y = ops.gemm_conv(x, wt, B=1, H=1, W=M, taps=1, bias=bias, resid=resid)
        ts = []
        for i, (off, n, scale, perm, drop) in enumerate(segs):
            down, up = factors[2 * i].detach(), factors[2 * i + 1].detach()
            R = ops.lora_pad_rank(down.shape[0])
            u = up * scale if scale != 1.0 else up
            if perm is not None:
                u = u[perm]
            t = ops.lora_down(x, _operand16(down, 0, R, x.dtype))
            ops.lora_up(t, _operand16(u, 1, R, x.dtype), out=y[:, off:off + n], accumulate=True, drop=drop and ops.LoraDrop(*drop))
            ts.append(t)
        ctx.meta, ctx.wt, ctx.has_resid, ctx.n_seg = meta, wt, resid is not None, len(segs)
        ctx.save_for_backward(x, *ts, *factors, *((y,) if geglu else ()))
        return geglu_fwd(y) if geglu else y

    @staticmethod
    def backward(ctx, dy):
        segs, geglu = ctx.meta
        ns = ctx.n_seg
        if dy is None:
            return (None,) * (5 + 2 * ns)
        saved = ctx.saved_tensors
        x, ts, factors = saved[0], saved[1:1 + ns], saved[1 + ns:1 + 3 * ns]
        g = dy.contiguous()
        if geglu:
            g = geglu_bwd(saved[1 + 3 * ns], g)
        M, K = x.shape
        dx = ops.gemm_conv(g, dgrad_weight(ctx.wt, 1, 0, K), B=1, H=1, W=M, taps=1) if ctx.needs_input_grad[0] else None
        grads = []
        for i, (off, n, scale, perm, drop) in enumerate(segs):
            down, up = factors[2 * i].detach(), factors[2 * i + 1].detach()
            r = down.shape[0]
            R = ops.lora_pad_rank(r)
            gi = g[:, off:off + n]
            upk = up if perm is None else up[perm]
            if drop:      # the mask of the forward, regenerated on g_i; 1 / (1 - p) rides in alpha
                drop = ops.LoraDrop(*drop)
                scale = scale * drop.inv_keep
            dt = ops.lora_down(gi, _operand16(upk.t(), 0, R, x.dtype), alpha=scale, drop=drop)                 # [M, R] = scale g_i up
            if dx is not None:
                ops.lora_up(dt, _operand16(down.t(), 1, R, x.dtype), out=dx, accumulate=True)                   # dx += dT down
            d_down = d_up = None
            if ctx.needs_input_grad[5 + 2 * i]:
                d_down = ops.lora_wgrad(dt, x)[:r]                                                             # [r, K] fp32 (the first rows: contiguous)
            if ctx.needs_input_grad[6 + 2 * i]:
                d_up = ops.lora_wgrad(ts[i], gi, alpha=scale, drop=drop)[:r].t()                                 # [n, r] fp32 (packed row order)
                if perm is not None:
                    unp = torch.empty(n, r, device=d_up.device, dtype=d_up.dtype)
                    unp[perm] = d_up
                    d_up = unp
                d_up = d_up.contiguous()
            grads += [d_down, d_up]
        dresid = dy if ctx.has_resid and ctx.needs_input_grad[1] else None
        return (dx, dresid, None, None, None) + tuple(grads)


def _lora_colgrp(perm):
    """The masked kernels' column-group table of a packed-row permutation, built once and kept on the permutation (i.e. per packing)."""
    tab = getattr(perm, "_lr_colgrp", None)
    if tab is None:
        from . import lora_dropout
        tab = perm._lr_colgrp = torch.from_numpy(lora_dropout.colgrp_of(perm.cpu().numpy())).to(perm.device)
    return tab


def lora_dropout_live(mod):
    """True for a LoraInjectedLinear in training mode with p > 0; NotImplementedError when such a layer has no dropout stream."""
    if not (mod.training and mod.dropout.p > 0):
        return False
    if getattr(mod, "drop_stream", None) is None or getattr(mod, "drop_state", None) is None:
        raise NotImplementedError("LoRA dropout (dropout_p > 0 in training mode): this layer was not injected with a dropout stream -- only "
                                  "inject_trainable_lora(..., dropout_p=p) gives a layer the stream id its mask is drawn from")
    return True


def lora_linear(x, wt, bias, segs, resid=None, geglu=False, draw=None):
    """Linear with unmerged LoRA factors.  segs: (LoraInjectedLinear, first output column, columns, packed-row permutation | None) per
    injected Linear whose rows lie in `wt` (engine.lora_segments).  Differentiable w.r.t. x, resid and the fp32 factors; under
    torch.no_grad() it is the same launches without a graph.  draw: the dropout draw number of this forward (LoraDropoutState.take), needed
    when a segment's layer trains with dropout under autograd; without autograd (or with p == 0, or in eval mode) no mask is applied."""
    meta, factors = [], []
    for mod, off, n, perm in segs:
        drop = None
        if lora_dropout_live(mod) and torch.is_grad_enabled():
            if draw is None:
                raise ValueError("LoRA dropout needs the draw number of this forward (draw=)")
            drop = (mod.drop_state.seed, mod.drop_stream, int(draw), float(mod.dropout.p), None if perm is None else _lora_colgrp(perm))
        if off % 8 or n % 8:
            raise ValueError("LoRA segment columns must be multiples of 8")
        meta.append((off, n, float(mod.scale), perm, drop))
        factors += [mod.lora_down.weight, mod.lora_up.weight]
    if resid is not None and geglu:
        raise ValueError("the GEGLU projection takes no residual")
    return _LoraLinear.apply(x, resid, wt, bias, (tuple(meta), bool(geglu)), *factors)


class _GradAnchor(torch.autograd.Function):
    """x, unchanged, as a tensor that requires grad (its backward hands nothing on).  With trainable LoRA factors the input of the first
    SpatialTransformer takes this, so every injected layer -- the first block's self-attention too, whose input depends on no trainable
    tensor -- runs the differentiable route; the decisions of engine.fold_ok / gn_fuse_ok / forking then hold as they are."""

    @staticmethod
    def forward(ctx, x, anchor):
        return x.view_as(x)

    @staticmethod
    def backward(ctx, g):
        return None, None


def grad_anchor(x, anchor):
    return _GradAnchor.apply(x, anchor) if torch.is_grad_enabled() and not x.requires_grad and anchor.requires_grad else x
