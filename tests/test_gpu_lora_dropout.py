"""GPU: LoRA dropout -- the masked forms of the three LoRA kernels (csrc/lora.hip, lr_lora_*_drop) against float64 on the same
16-bit-rounded inputs with the numpy mask of leftrefill_amd/lora_dropout.py, then the wiring: `_LoraLinear` with masked segments against
torch float64 autograd of the stated formula, the whole model against the reference's gradients under the same stated masks
(tests/golden/lora_dropout.npz, tools/make_golden_lora_dropout.py), the draw rule, and three optimizer steps end to end.

Bounds: those of tests/test_gpu_lora.py (`check` for down / up, the summation bound for wgrad with |q (.) keep| in it) -- a mask only zeroes
a 16-bit value exactly and 1 / (1 - p) is one fp32 factor, so the masked route has the unmasked route's rounding points."""
import json
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from oracle import golden_spec as G  # noqa: E402
from leftrefill_amd import lora_dropout as D  # noqa: E402
from tests.test_gpu_lora import check, dev, padded, rnd  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
P, SEED = 0.1, 20240807
F16, BF16 = torch.float16, torch.bfloat16


def _perm(N):
    from leftrefill_amd import packing
    return packing.geglu_perm(N // 2)


def _colgrp(perm):
    return torch.from_numpy(D.colgrp_of(perm.numpy())).to(dev())


def keep_of(stream, draw, M, N, perm=None, p=P, seed=SEED):
    """[M, N] bool keep mask in STORAGE order: stored column j is logical column perm[j]."""
    k = torch.from_numpy(np.ascontiguousarray(D.keep_mask(seed, stream, draw, M, N, p)))
    return k if perm is None else k[:, perm]


def drop_of(stream, draw, perm=None, p=P, seed=SEED):
    from leftrefill_amd import ops
    return ops.LoraDrop(seed, stream, draw, p, colgrp=None if perm is None else _colgrp(perm))


# (M, N | K, r, dtype, packed): a partial 16-row wave (154 = 9 x 16 + 10) in one column block; bf16 with a partial 256-column block
# (320); the GEGLU width in packed order with its column-group table, ten column blocks; KS = 2 (padded rank 64).  `down` adds a K tail.
SHAPES = [(154, 256, 4, F16, False), (1024, 320, 16, BF16, False), (512, 2560, 6, F16, True), (160, 1280, 64, F16, False)]
IDS = [f"{m}x{n}r{r}{'bf' if d == BF16 else ''}{'geglu' if g else ''}" for m, n, r, d, g in SHAPES]


@pytest.mark.parametrize("M,N,r,dtype,packed", SHAPES, ids=IDS)
@pytest.mark.parametrize("mode", ["plain", "strided_accumulate"])
def test_lora_up_drop(M, N, r, dtype, packed, mode):
    from leftrefill_amd import ops
    R = ops.lora_pad_rank(r)
    perm = _perm(N) if packed else None
    t = rnd(3, (M, r), dtype)
    u = rnd(4, (N, r), dtype, 0.5)                                   # rows in STORAGE order
    keep = keep_of(5, 9, M, N, perm)
    prod = torch.where(keep, (t.double() @ u.double().t()) * D.inv_keep(P), torch.zeros((), dtype=torch.float64))
    td, ud = padded(t, 1, R).to(dtype).to(dev()), padded(u, 1, R).to(dtype).to(dev())
    drop, none = drop_of(5, 9, perm), drop_of(5, 9, perm, p=0.0)
    assert none.c.threshold == 0 and none.c.inv_keep == 1.0
    if mode == "plain":
        y = ops.lora_up(td, ud, drop=drop)
        check(f"up_drop {M}x{N} r{r}", y, prod)
        assert not y.cpu()[~keep].any()                               # a dropped element is +0
        assert torch.equal(y, ops.lora_up(td, ud, drop=drop))         # two runs are bit-identical
        assert torch.equal(ops.lora_up(td, ud, drop=none), ops.lora_up(td, ud))      # threshold 0, inv_keep 1: the unmasked entry's bits
        assert not torch.equal(y, ops.lora_up(td, ud, drop=drop_of(5, 10, perm))) and not torch.equal(y, ops.lora_up(td, ud, drop=drop_of(6, 9, perm)))
        if packed:      # the same logical layer in logical row order without a table: the same values at the permuted places
            inv = torch.empty_like(perm)
            inv[perm] = torch.arange(N)
            y_log = ops.lora_up(td, ud[inv.to(dev())].contiguous(), drop=drop_of(5, 9))
            assert torch.equal(y_log[:, perm.to(dev())], y)
        return
    ldy, off = N + 72, 40
    y0 = rnd(5, (M, ldy), dtype, 2.0)
    y = y0.to(dtype).to(dev())
    ops.lora_up(td, ud, out=y[:, off:off + N], accumulate=True, drop=drop)
    check(f"up_drop+= {M}x{N} r{r}", y[:, off:off + N], y0[:, off:off + N].double() + prod)
    got = y.float().cpu()
    assert torch.equal(got[:, :off], y0[:, :off]) and torch.equal(got[:, off + N:], y0[:, off + N:])      # nothing outside the range is touched
    assert torch.equal(got[:, off:off + N][~keep], y0[:, off:off + N][~keep])                              # a dropped element keeps y's bits
    # the same layer as a slice at another offset: the same mask (columns count from the pointer the kernel is given)
    y2 = y0.to(dtype).to(dev())
    y2[:, 8:8 + N] = y0[:, off:off + N].to(dtype).to(dev())
    ops.lora_up(td, ud, out=y2[:, 8:8 + N], accumulate=True, drop=drop)
    assert torch.equal(y2[:, 8:8 + N], y[:, off:off + N])
    y3, y4 = y0.to(dtype).to(dev()), y0.to(dtype).to(dev())
    ops.lora_up(td, ud, out=y3[:, off:off + N], accumulate=True, drop=none)
    ops.lora_up(td, ud, out=y4[:, off:off + N], accumulate=True)
    assert torch.equal(y3, y4)


DOWN = SHAPES + [(48, 2568, 4, F16, False)]                           # K % 32 == 8: the K tail


@pytest.mark.parametrize("M,K,r,dtype,packed", DOWN, ids=IDS + ["48x2568r4"])
def test_lora_down_drop(M, K, r, dtype, packed):
    """t = alpha (x (.) keep) a^T: the mask on the wide operand at x's own (row, column), x a column slice of a wider buffer."""
    from leftrefill_amd import ops
    R = ops.lora_pad_rank(r)
    perm = _perm(K) if packed else None
    ld = K + 64
    xw = rnd(1, (M, ld), dtype)
    a = rnd(2, (r, K), dtype, 1.0 / r)
    keep = keep_of(2, 4, M, K, perm)
    alpha = 0.75 * D.inv_keep(P)
    ref = alpha * ((xw[:, 32:32 + K].double() * keep) @ a.double().t())
    xd, ad = xw.to(dtype).to(dev())[:, 32:32 + K], padded(a, 0, R).to(dtype).to(dev())
    drop = drop_of(2, 4, perm)
    t = ops.lora_down(xd, ad, alpha, drop=drop)
    assert t.shape == (M, R) and not t[:, r:].any()                  # the padded ranks stay exactly zero
    check(f"down_drop {M}x{K} r{r}", t[:, :r], ref)
    assert torch.equal(t, ops.lora_down(xd, ad, alpha, drop=drop))
    assert torch.equal(ops.lora_down(xd, ad, alpha, drop=drop_of(2, 4, perm, p=0.0)), ops.lora_down(xd, ad, alpha))
    # the same slice at another offset of another buffer: the same mask
    x2 = torch.zeros(M, K + 16, dtype=dtype, device=dev())
    x2[:, 8:8 + K] = xd
    assert torch.equal(ops.lora_down(x2[:, 8:8 + K], ad, alpha, drop=drop), t)
    if packed:
        inv = torch.empty_like(perm)
        inv[perm] = torch.arange(K)
        inv = inv.to(dev())
        t_log = ops.lora_down(xd[:, inv].contiguous(), ad[:, inv].contiguous(), alpha, drop=drop_of(2, 4))
        # (the K order of the sum differs between the two layouts: equal within the bound, not bit for bit)
        check(f"down_drop {M}x{K} r{r} logical order", t_log[:, :r], ref)


WGRAD = [(154, 128, 4, F16, False), (1024, 320, 16, BF16, False), (1100, 2560, 64, F16, True)]


@pytest.mark.parametrize("M,C,r,dtype,packed", WGRAD, ids=[f"{m}x{c}r{r}{'bf' if d == BF16 else ''}" for m, c, r, d, g in WGRAD])
def test_lora_wgrad_drop(M, C, r, dtype, packed):
    """d = alpha p^T (q (.) keep), fp32: the summation bound of test_lora_wgrad with |q (.) keep| in it; two runs are bit-identical."""
    from leftrefill_amd import ops
    R = ops.lora_pad_rank(r)
    perm = _perm(C) if packed else None
    ldq = C + 64
    p = rnd(6, (M, r), dtype)
    qw = rnd(7, (M, ldq), dtype)
    keep = keep_of(11, 2, M, C, perm)
    q = qw[:, 16:16 + C].double() * keep
    alpha = 0.5 * D.inv_keep(P)
    ref = alpha * (p.double().t() @ q)
    bound = alpha * 2.0 * M * 2.0 ** -24 * (p.double().abs().t() @ q.abs())
    pd, qd = padded(p, 1, R).to(dtype).to(dev()), qw.to(dtype).to(dev())[:, 16:16 + C]
    drop = drop_of(11, 2, perm)
    d1 = ops.lora_wgrad(pd, qd, alpha, drop=drop)
    d2 = ops.lora_wgrad(pd, qd, alpha, drop=drop)
    assert d1.shape == (R, C) and d1.dtype == torch.float32 and torch.equal(d1, d2)
    assert not d1[r:].any()
    err = (d1[:r].double().cpu() - ref).abs()
    print(f"[lora wgrad_drop {M}x{C} r{r}] max err {err.max().item():.3e}, max err / bound {(err / bound.clamp_min(1e-300)).max().item():.3e}")
    assert (err <= bound).all()
    assert torch.equal(ops.lora_wgrad(pd, qd, alpha, drop=drop_of(11, 2, perm, p=0.0)), ops.lora_wgrad(pd, qd, alpha))
    if packed:      # column c of the packed run is logical column perm[c]: the same sum over rows, bit for bit
        inv = torch.empty_like(perm)
        inv[perm] = torch.arange(C)
        d_log = ops.lora_wgrad(pd, qd[:, inv.to(dev())].contiguous(), alpha, drop=drop_of(11, 2))
        assert torch.equal(d_log[:, perm.to(dev())], d1)


def test_descriptor_is_checked():
    from leftrefill_amd import ops
    t, u = torch.zeros(16, 32, dtype=F16, device=dev()), torch.zeros(64, 32, dtype=F16, device=dev())
    for bad in (dict(inv_keep=0.5), dict(inv_keep=float("inf")), dict(inv_keep=float("nan")), dict(inv_keep=2.0), dict(threshold=2 ** 31)):
        with pytest.raises(RuntimeError):
            ops.lora_up(t, u, drop=ops.LoraDrop(SEED, 0, 0, P, **bad))
    with pytest.raises(AssertionError, match="colgrp"):
        ops.lora_up(t, u, drop=ops.LoraDrop(SEED, 0, 0, P, colgrp=torch.zeros(8, dtype=torch.int32, device=dev())))


# ---------------------------------------------------------------------------------------------------------------------
# _LoraLinear with masked segments against torch float64 autograd of the stated formula
# ---------------------------------------------------------------------------------------------------------------------
def _layers(widths, K, r, scale, p=P):
    import leftrefill_amd.dropin as dropin
    dropin.install()
    from inpainting_ldm.lora import LoraDropoutState, LoraInjectedLinear
    h16 = lambda t_: t_.half().float()
    state = LoraDropoutState(seed=SEED)
    mods = []
    for i, n in enumerate(widths):
        lin = LoraInjectedLinear(K, n, bias=False, r=r, dropout_p=p, scale=scale)
        lin.drop_stream, lin.drop_state = 3 + i, state
        with torch.no_grad():
            lin.lora_down.weight.copy_(h16(torch.randn(r, K) / r))
            lin.lora_up.weight.copy_(h16(torch.randn(n, r) * 0.05))
        mods.append(lin.train())
    return mods


def _ref_linear(x, w, b, mods, draw, geglu=False):
    """float64 on the CPU: x W^T + b + per layer scale * where(keep, (x down^T) up^T * inv_keep, 0) in the layer's columns, then the gate."""
    x = x.double().requires_grad_(True)
    M = x.shape[0]
    leaves, cols = [], []
    for lin in mods:
        down, up = lin.lora_down.weight.detach().double().requires_grad_(True), lin.lora_up.weight.detach().double().requires_grad_(True)
        leaves += [down, up]
        keep = torch.from_numpy(np.ascontiguousarray(D.keep_mask(SEED, lin.drop_stream, draw, M, up.shape[0], lin.dropout.p)))
        cols.append(lin.scale * torch.where(keep, (x @ down.t()) @ up.t() * D.inv_keep(lin.dropout.p), torch.zeros((), dtype=torch.float64)))
    y = x @ w.double().t() + torch.cat(cols, 1)
    if b is not None:
        y = y + b.double()
    if geglu:
        u, g = y.chunk(2, dim=-1)
        y = u * torch.nn.functional.gelu(g)
    return x, leaves, y


@pytest.mark.parametrize("kind", ["qkv", "geglu"])
def test_lora_linear_with_masked_segments(kind):
    """M = 154 rows: a fused [q | k | v] (K = 320, three streams) and a GEGLU projection (K = 320, N = 2560, packed rows + column-group
    table): forward, dx and every factor gradient against float64 autograd of the stated formula.  Bounds: check() for the single
    projection; twice that for the projection + gate in a row (test_standalone_modules_apply_the_factors)."""
    from leftrefill_amd import train_ops
    torch.manual_seed(21)
    M, K, r, draw = 154, 320, 4, 6
    h16 = lambda t_: t_.half().float()
    x = h16(torch.randn(M, K))
    if kind == "qkv":
        mods, geglu, perm, tol = _layers([320, 320, 320], K, r, 0.5), False, None, {}
        bias = None
    else:
        mods, geglu, perm, tol = _layers([2560], K, r, 1.0), True, _perm(2560), dict(rtol=4e-3, atol_scale=4e-3)
        bias = torch.randn(2560) * 0.1
    N = sum(m_.lora_up.weight.shape[0] for m_ in mods)
    w = h16(torch.randn(N, K) * K ** -0.5)
    dy = h16(torch.randn(M, N // 2 if geglu else N))
    xr, leaves, yr = _ref_linear(x, w, bias, mods, draw, geglu)
    (yr * dy.double()).sum().backward()
    pd = None if perm is None else perm.to(dev())
    wd = (w if perm is None else w[perm]).half().to(dev()).contiguous()
    bd = None if bias is None else (bias[perm] if perm is not None else bias).to(dev()).contiguous()
    segs, off = [], 0
    for m_ in mods:
        m_.to(dev())
        n = m_.lora_up.weight.shape[0]
        segs.append((m_, off, n, pd))
        off += n
    xd = x.half().to(dev()).requires_grad_(True)

    def run(d):
        for m_ in mods:
            m_.lora_down.weight.grad = m_.lora_up.weight.grad = None
        xd.grad = None
        y = train_ops.lora_linear(xd, wd, bd, segs, geglu=geglu, draw=d)
        y.backward(dy.half().to(dev()))
        return [y.detach()] + [xd.grad.clone()] + [g_ for m_ in mods for g_ in (m_.lora_down.weight.grad.clone(), m_.lora_up.weight.grad.clone())]

    got = run(draw)
    check(f"lora_linear {kind} forward", got[0], yr.detach(), **tol)
    check(f"lora_linear {kind} dx", got[1], xr.grad, **tol)
    for i, (g_, leaf) in enumerate(zip(got[2:], leaves)):
        assert g_.dtype == torch.float32
        check(f"lora_linear {kind} d {'down' if i % 2 == 0 else 'up'}{i // 2}", g_, leaf.grad, **tol)
    again, other = run(draw), run(draw + 1)
    assert all(torch.equal(a_, b_) for a_, b_ in zip(got, again))
    assert not any(torch.equal(a_, b_) for a_, b_ in zip(got, other))
    # eval mode under autograd: today's unmasked launches (no draw needed)
    for m_ in mods:
        m_.eval()
    y_eval = train_ops.lora_linear(xd, wd, bd, segs, geglu=geglu)
    for m_ in mods:
        m_.dropout.p = 0.0
        m_.train()
    assert torch.equal(train_ops.lora_linear(xd, wd, bd, segs, geglu=geglu), y_eval)
    mods[0].dropout.p = P
    with pytest.raises(ValueError, match="draw"):
        train_ops.lora_linear(xd, wd, bd, segs, geglu=geglu)


# ---------------------------------------------------------------------------------------------------------------------
# the whole model against the reference's gradients under the same stated masks, and the draw rule
# ---------------------------------------------------------------------------------------------------------------------
def _golden():
    return np.load(os.path.join(ROOT, "tests", "golden", "lora_dropout.npz"))


def test_factor_gradients_with_dropout_against_the_reference():
    """p_losses + backward at loss scale 2^14 with `lora_dropout: 0.1`, seed 20240807, draw 0, against the REAL reference run with the same
    stated masks in place of its nn.Dropout (tests/golden/lora_dropout.npz).  Bounds of test_factor_gradients_against_the_reference: loss
    2e-3 relative, d context rel-L2 1e-2, every factor-gradient norm and the stored full gradients within max(2 e, 1e-2), e the noise floor
    stored with the golden.  Then the draw rule: a second run from the same draw and recompute_in_backward = True are bit-identical,
    forward A, forward B, backward A, backward B gives the gradients of the separate runs, the next draw gives other gradients.
    LEFTREFILL_WRITE_PROFILES=1 writes profiles/lora_dropout_parity.json."""
    import leftrefill_amd.dropin as dropin
    dropin.install()
    from inpainting_ldm.lora import lora_dropout_state
    from inpainting_ldm.NVS_ldm import NVSLDM
    from tools.make_golden_lora import set_factors
    g = _golden()
    cfg = G.CONFIGS["MID"]
    m = NVSLDM(first_stage_config={"target": "torch.nn.Identity"}, cond_stage_config={"target": "torch.nn.Identity"},
               unet_config={"target": "ldm.modules.diffusionmodules.openaimodel.UNetModel", "params": cfg.kwargs()},
               conditioning_key="hybrid", scale_factor=0.18215, linear_start=0.00085, linear_end=0.0120, timesteps=1000, channels=4,
               data_config={"img_size": 256},
               lora={"do_lora": True, "lora_type": "default", "lora_rank": 4, "lora_scale": 1.0, "lora_dropout": float(g["p"])})
    unet = m.model.diffusion_model
    unet.load_state_dict(G.unet_state("MID"), strict=True)
    m.set_lora()
    set_factors(unet, 4)
    m = m.to(dev()).train()
    state = lora_dropout_state(unet)
    state.seed = int(g["seed"])
    by_name = dict(unet.named_modules())
    assert [by_name[str(n)].drop_stream for n in g["stream_names"]] == list(range(len(g["stream_names"])))
    factors = {n: p for n, p in unet.named_parameters() if ".lora_" in n}
    assert sorted(factors) == sorted(str(n) for n in g["grad_names"])
    for p in m.parameters():
        p.requires_grad_(False)
    for p in factors.values():
        p.requires_grad_(True)
    case, B, h, w, ts = G.TRAIN_CASES[0]
    x_start, noise = G.T(case + ".x_start", (B, 4, h, w)), G.T(case + ".noise", (B, 4, h, w))
    c_concat, c_cross0 = G.T(case + ".c_concat", (B, 5, h, w)), G.T(case + ".c_cross", (B, 77, cfg.context_dim))
    t = torch.tensor(ts, dtype=torch.long)
    scale = 2.0 ** 14

    def forward():
        c_cross = c_cross0.to(dev()).requires_grad_(True)
        loss, _ = m.p_losses(x_start.to(dev()), {"c_concat": [c_concat.to(dev())], "c_crossattn": [c_cross]}, t.to(dev()), noise=noise.to(dev()))
        return loss, c_cross

    def backward(loss, c_cross):
        for p in factors.values():
            p.grad = None
        (loss * scale).backward()
        return loss.item(), c_cross.grad.float().cpu() / scale, {n: p.grad.detach().clone() for n, p in factors.items()}

    def run(draw):
        state.draw = draw
        out = backward(*forward())
        assert state.draw == draw + 1                                  # one draw per training forward
        return out

    same = lambda a_, b_: torch.equal(a_[1], b_[1]) and all(torch.equal(a_[2][n], b_[2][n]) for n in factors)
    first = run(int(g["draw"]))
    loss, dctx, grads = first
    assert all(v.dtype == torch.float32 and torch.isfinite(v).all() for v in grads.values())
    ref_loss, ref_dctx = float(g["loss"]), torch.from_numpy(g["dctx"])
    rel_ctx = ((dctx - ref_dctx).norm() / ref_dctx.norm()).item()
    print(f"[lora dropout train] loss {loss:.6f} (reference {ref_loss:.6f}); d/dcontext rel_l2 {rel_ctx:.3e}")
    names = [str(n) for n in g["grad_names"]]
    ref_norm, norm_e = dict(zip(names, g["grad_norms"])), dict(zip(names, g["grad_norm_emul"]))
    rows, worst = {}, 0.0
    for n in names:
        got = grads[n].double().cpu().norm().item() / scale
        err = abs(got - ref_norm[n]) / ref_norm[n]
        rows[n] = dict(norm_rel_err=err, norm_emul=float(norm_e[n]), bound=max(2 * float(norm_e[n]), 1e-2))
        worst = max(worst, err / rows[n]["bound"])
    full = [k[len("grad."):] for k in g.files if k.startswith("grad.")]
    assert len(full) == 3 * 18
    for n in full:
        ref = torch.from_numpy(g["grad." + n]).double()
        got = grads[n].double().cpu() / scale
        e = float(g["emul." + n])
        rows[n].update(rel_l2=((got - ref).norm() / ref.norm()).item(), rel_l2_emul=e, rel_l2_bound=max(2 * e, 1e-2))
    worst_full = max(rows[n]["rel_l2"] / rows[n]["rel_l2_bound"] for n in full)
    print(f"[lora dropout train] factor-gradient norms: worst err / bound {worst:.3f} over {len(names)} factors; full gradients of 3 blocks: "
          f"worst rel_l2 / bound {worst_full:.3f} (max rel_l2 {max(rows[n]['rel_l2'] for n in full):.3e})")
    if os.environ.get("LEFTREFILL_WRITE_PROFILES"):
        out_dir = os.environ.get("LEFTREFILL_PROFILE_DIR") or os.path.join(ROOT, "profiles")
        with open(os.path.join(out_dir, "lora_dropout_parity.json"), "w") as f:
            json.dump(dict(case=case, p=float(g["p"]), seed=int(g["seed"]), draw=int(g["draw"]), loss=loss, reference_loss=ref_loss,
                           dctx_rel_l2=rel_ctx, worst_norm_err_over_bound=worst, worst_full_rel_l2_over_bound=worst_full, factors=rows),
                      f, indent=1)
    assert abs(loss - ref_loss) <= 2e-3 * ref_loss
    assert torch.isfinite(dctx).all() and rel_ctx <= 1e-2
    bad = [n for n in names if rows[n]["norm_rel_err"] > rows[n]["bound"]] + [n for n in full if rows[n]["rel_l2"] > rows[n]["rel_l2_bound"]]
    assert not bad, [(n, rows[n]) for n in bad[:5]]

    # ---- the draw rule ----
    assert same(run(0), first)                                        # same seed, draw reset: bit-identical
    second = run(1)
    assert not torch.equal(second[1], first[1]) and not any(torch.equal(second[2][n], first[2][n]) for n in factors)      # the next draw: other masks
    for recompute in (False, True):
        unet.recompute_in_backward = recompute
        assert same(run(0), first), recompute                         # a recomputed forward replays the masks of the draw it was given
        state.draw = 0
        a, b = forward(), forward()                                   # draws 0 and 1; both backwards come after both forwards
        assert state.draw == 2
        assert same(backward(*a), first) and same(backward(*b), second), recompute
    unet.recompute_in_backward = False
    # eval mode under autograd and no_grad in training mode: no masks, no draw taken
    state.draw = 5
    with torch.no_grad():
        forward()
    m.eval()
    forward()
    assert state.draw == 5


# ---------------------------------------------------------------------------------------------------------------------
# end to end: three Trainer.fit steps with `lora_dropout: 0.1`, checkpoint, resume, sampling
# ---------------------------------------------------------------------------------------------------------------------
def _nvs_model(seed=0):
    from tests.test_gpu_lora import _nvs_model as plain
    m, cfg = plain(seed=seed, lora=False)
    m.lora_cfg = {"do_lora": True, "lora_type": "default", "lora_rank": 4, "lora_scale": 1.0, "lora_dropout": 0.1}
    m.set_lora()                                                      # after the base weights, before the optimizer
    return m.to(dev()), cfg


def test_three_training_steps_with_dropout_checkpoint_resume_and_sampling(tmp_path):
    from inpainting_ldm.lora import lora_dropout_state
    from leftrefill_amd.trainer import Trainer
    from tests.test_gpu_trainer import _batches
    m, cfg = _nvs_model()
    unet = m.model.diffusion_model
    state = lora_dropout_state(unet)
    seed = state.seed
    assert state.draw == 0 and all(s.dropout.p == 0.1 for s in unet.modules() if hasattr(s, "lora_up"))
    factors = {n: p for n, p in m.named_parameters() if ".lora_" in n}
    before = {n: p.detach().clone() for n, p in factors.items()}
    batches = _batches(cfg, 3)
    tr = Trainer(max_steps=3, precision=16, growth_interval=3, default_root_dir=str(tmp_path), verbose=False)
    torch.manual_seed(123)
    tr.fit(m, batches)
    assert len(tr.optimizer.param_groups) == 2 and tr.optimizer.amp_state()["applied_steps"] >= 2
    assert state.draw == 3 and state.seed == seed                     # one draw per training step
    after = {n: p.detach().clone() for n, p in factors.items()}
    assert all(torch.isfinite(v).all() for v in after.values())
    assert all(not torch.equal(after[n], before[n]) for n in after), "every factor moves"
    # last.ckpt carries the dropout state; a resumed model continues at draw 3
    path = os.path.join(str(tmp_path), "ckpts", "last.ckpt")
    ckpt = torch.load(path, map_location="cpu", weights_only=False)
    assert ckpt["lora_dropout_state"] == {"seed": seed, "draw": 3}
    m2, _ = _nvs_model(seed=9)
    s2 = lora_dropout_state(m2.model.diffusion_model)
    s2.seed = 1
    Trainer(max_steps=3, precision=16, resume_from_checkpoint=path, verbose=False).fit(m2, batches)      # (global_step 3: no further step)
    assert (s2.seed, s2.draw) == (seed, 3)
    assert all(torch.equal(p.detach(), after[n]) for n, p in m2.named_parameters() if ".lora_" in n)
    # sampling afterwards is the merged route and equals the eval-mode unmerged forward; neither takes a draw
    m.eval()
    x = torch.randn(2, 9, 8, 16, generator=torch.Generator().manual_seed(3)).to(dev())
    t = torch.tensor([501, 21], device=dev())
    ctx = batches[0]["ctx"]
    with torch.no_grad():
        y_m = unet(x, t, context=ctx).float()
    assert unet._plan is not unet._plan["root"]
    for p in factors.values():
        p.requires_grad_(True)
    y_u = unet(x, t, context=ctx).detach().float()
    assert unet._plan is unet._plan["root"] and state.draw == 3
    rel = ((y_m - y_u).norm() / y_u.norm()).item()
    print(f"[lora dropout e2e] merged vs unmerged (eval) after training rel_l2 {rel:.3e}")
    assert rel <= 4e-3                                                # (test_gpu_unet.py's cap on the MID forward's rel-L2)
