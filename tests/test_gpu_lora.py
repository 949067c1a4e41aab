"""GPU: LoRA on the UNet -- the four kernels of csrc/lora.hip against float64 on the same 16-bit-rounded inputs, then the wiring:
merged (no-grad) and unmerged (grad-enabled) forwards, the factor gradients against the reference's (tests/golden/lora.npz, made by
tools/make_golden_lora.py), and three optimizer steps end to end."""
import json
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from oracle import golden_spec as G  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def dev():
    return torch.device("cuda:0")


def rnd(seed, shape, dtype, scale=1.0):
    """Deterministic N(0, scale^2) values already rounded to the 16-bit type (as fp32 on the host)."""
    g = torch.Generator().manual_seed(seed)
    return (torch.randn(shape, generator=g) * scale).to(dtype).float()


def check(name, got, ref, rtol=2e-3, atol_scale=2e-3):
    """The bound of tests/test_gpu_backward.py::check."""
    got, ref = got.float().cpu(), ref.float()
    assert torch.isfinite(got).all(), name
    scale = ref.abs().max().item()
    err = (got - ref).abs()
    rel = (err.norm() / ref.norm()).item()
    print(f"[lora {name}] rel_l2 {rel:.3e} max_abs {err.max().item():.3e} (|ref| max {scale:.3e})")
    assert rel < 3e-3, (name, rel)
    assert (err <= atol_scale * scale + rtol * ref.abs()).all(), name


def padded(f, r_axis, R):
    """Zero-pad a factor along its rank axis to the kernels' padded rank."""
    shape = list(f.shape)
    shape[r_axis] = R - shape[r_axis]
    return torch.cat([f, f.new_zeros(shape)], dim=r_axis)


DOWN_UP = [(154, 256, 4, torch.float16), (1024, 320, 16, torch.float16), (4160, 1280, 64, torch.float16), (512, 2560, 6, torch.float16),
           (1024, 320, 16, torch.bfloat16)]


@pytest.mark.parametrize("M,K,r,dtype", DOWN_UP, ids=[f"{m}x{k}r{r}{'bf' if d == torch.bfloat16 else ''}" for m, k, r, d in DOWN_UP])
def test_lora_down(M, K, r, dtype):
    from leftrefill_amd import ops
    R = ops.lora_pad_rank(r)
    ld = K + 64                                                    # X is a column slice of a wider buffer
    xw = rnd(1, (M, ld), dtype)
    a = rnd(2, (r, K), dtype, 1.0 / r)
    alpha = 0.75
    ref = alpha * (xw[:, 32:32 + K].double() @ a.double().t())
    t = ops.lora_down(xw.to(dtype).to(dev())[:, 32:32 + K], padded(a, 0, R).to(dtype).to(dev()), alpha)
    assert t.shape == (M, R) and not t[:, r:].any()                # the padded ranks stay exactly zero
    check(f"down {M}x{K} r{r}", t[:, :r], ref)


@pytest.mark.parametrize("M,N,r,dtype", DOWN_UP, ids=[f"{m}x{k}r{r}{'bf' if d == torch.bfloat16 else ''}" for m, k, r, d in DOWN_UP])
@pytest.mark.parametrize("mode", ["plain", "strided_accumulate"])
def test_lora_up(M, N, r, dtype, mode):
    from leftrefill_amd import ops
    R = ops.lora_pad_rank(r)
    t = rnd(3, (M, r), dtype)
    u = rnd(4, (N, r), dtype, 0.5)
    prod = t.double() @ u.double().t()
    td, ud = padded(t, 1, R).to(dtype).to(dev()), padded(u, 1, R).to(dtype).to(dev())
    if mode == "plain":
        check(f"up {M}x{N} r{r}", ops.lora_up(td, ud), prod)
        return
    ldy, off = N + 72, 40                                          # ldy > N: the call lands in a column range of a wider buffer
    y0 = rnd(5, (M, ldy), dtype, 2.0)
    y = y0.to(dtype).to(dev())
    ops.lora_up(td, ud, out=y[:, off:off + N], accumulate=True)
    check(f"up+= {M}x{N} r{r}", y[:, off:off + N], y0[:, off:off + N].double() + prod)
    got = y.float().cpu()
    assert torch.equal(got[:, :off], y0[:, :off]) and torch.equal(got[:, off + N:], y0[:, off + N:])      # nothing outside the range is touched


WGRAD = [(154, 128, 4, torch.float16), (1024, 320, 16, torch.float16), (5000, 2560, 64, torch.float16), (2048, 10240, 16, torch.float16),
         (1024, 320, 16, torch.bfloat16)]


@pytest.mark.parametrize("M,C,r,dtype", WGRAD, ids=[f"{m}x{c}r{r}{'bf' if d == torch.bfloat16 else ''}" for m, c, r, d in WGRAD])
def test_lora_wgrad(M, C, r, dtype):
    """fp32 output: the order-independent summation bound |err| <= 2 M 2^-24 (|P|^T |Q|) elementwise (exact products, fp32 accumulation;
    the factor 2 covers the matrix core's internal rounding); two runs are bit-identical."""
    from leftrefill_amd import ops
    R = ops.lora_pad_rank(r)
    ldq = C + 64
    p = rnd(6, (M, r), dtype)
    qw = rnd(7, (M, ldq), dtype)
    q = qw[:, 16:16 + C]
    alpha = 0.5
    ref = alpha * (p.double().t() @ q.double())
    bound = alpha * 2.0 * M * 2.0 ** -24 * (p.double().abs().t() @ q.double().abs())
    pd, qd = padded(p, 1, R).to(dtype).to(dev()), qw.to(dtype).to(dev())[:, 16:16 + C]
    d1 = ops.lora_wgrad(pd, qd, alpha)
    d2 = ops.lora_wgrad(pd, qd, alpha)
    assert d1.shape == (R, C) and d1.dtype == torch.float32 and torch.equal(d1, d2)
    assert not d1[r:].any()
    err = (d1[:r].double().cpu() - ref).abs()
    print(f"[lora wgrad {M}x{C} r{r}] max err {err.max().item():.3e}, max err / bound {(err / bound.clamp_min(1e-300)).max().item():.3e}")
    assert (err <= bound).all()


def test_lora_merge_f32():
    """The summation bound of test_lora_wgrad with R in place of M, over all R + 1 terms of an element (the base weight is the last
    one added): |err| <= 2 R 2^-24 (|W| + alpha |B| |A|)."""
    from leftrefill_amd import ops
    N, K, r, alpha = 2560, 320, 16, 0.7
    g = torch.Generator().manual_seed(8)
    w, up, down = torch.randn(N, K, generator=g), torch.randn(N, r, generator=g) * 0.02, torch.randn(r, K, generator=g) / r
    ref = w.double() + alpha * (up.double() @ down.double())
    bound = 2.0 * r * 2.0 ** -24 * (w.double().abs() + alpha * (up.double().abs() @ down.double().abs()))
    out = ops.lora_merge(w.to(dev()), up.to(dev()), down.to(dev()), alpha)
    err = (out.double().cpu() - ref).abs()
    print(f"[lora merge] max err {err.max().item():.3e}, max err / bound {(err / bound).max().item():.3e}")
    assert out.dtype == torch.float32 and (err <= bound).all()
    # up == 0 leaves the weight bit for bit, a -0.0 included
    w[0, :4] = -0.0
    same = ops.lora_merge(w.to(dev()), torch.zeros(N, r, device=dev()), down.to(dev()), 1.0).cpu()
    assert torch.equal(same.view(torch.int32), w.view(torch.int32))


def test_lora_rank_rule():
    from leftrefill_amd import ops
    assert [ops.lora_pad_rank(r) for r in (1, 4, 16, 32, 33, 64)] == [32, 32, 32, 32, 64, 64]
    for r in (0, 65, 128):
        with pytest.raises(ValueError, match="rank"):
            ops.lora_pad_rank(r)


# ---------------------------------------------------------------------------------------------------------------------
# wiring: the MID UNet with the reference's injection (r = 4, scale = 1) and the golden's factor values
# ---------------------------------------------------------------------------------------------------------------------
def _golden():
    return np.load(os.path.join(ROOT, "tests", "golden", "lora.npz"))


def _plain_unet():
    import leftrefill_amd.dropin as dropin
    dropin.install()
    from ldm.modules.diffusionmodules.openaimodel import UNetModel
    m = UNetModel(**G.CONFIGS["MID"].kwargs())
    m.load_state_dict(G.unet_state("MID"), strict=True)
    return m


def _injected_unet(set_values=True, r=4):
    m = _plain_unet()                                              # (installs the drop-in packages)
    from inpainting_ldm.lora import inject_trainable_lora
    from tools.make_golden_lora import set_factors
    inject_trainable_lora(m, r=r, scale=1.0)
    if set_values:
        set_factors(m, r)
    return m.to(dev()).eval()


def _merged_state(m):
    """The un-injected state dict with W + scale up down in place of every injected weight (host fp32: the oracle's input)."""
    sd = {}
    mods = dict(m.named_modules())
    for k, v in m.state_dict().items():
        v = v.detach().float().cpu()
        if ".lora_down." in k or ".lora_up." in k:
            continue
        if ".linear." in k:
            name = k.split(".linear.")[0]
            if k.endswith("weight"):
                mod = mods[name]
                v = v + mod.scale * (mod.lora_up.weight.detach().float().cpu() @ mod.lora_down.weight.detach().float().cpu())
            k = k.replace(".linear.", ".")
        sd[k] = v
    return sd


def _unet_case():
    case, cname, N, H, W, ts = [c for c in G.UNET_CASES if c[1] == "MID"][0]
    return G.unet_inputs(case, G.CONFIGS["MID"], N, H, W, ts)


def test_fresh_injection_leaves_the_model_bit_identical():
    """up = 0: the merged weights are the base weights bit for bit, so sampling is the un-injected model's launches and bits; with
    do_lora: False nothing is injected."""
    x, t, ctx = _unet_case()
    plain = _plain_unet().to(dev()).eval()
    from inpainting_ldm.lora import LoraInjectedLinear
    m = _injected_unet(set_values=False)
    with torch.no_grad():
        y0 = plain(x.to(dev()), t.to(dev()), ctx.to(dev()))
        y1 = m(x.to(dev()), t.to(dev()), ctx.to(dev()))
    assert torch.equal(y0, y1)
    assert m._plan is not m._plan["root"] and not any(pt.attn1.qkv.lora for pt in m._plan["tblocks"])      # the merged packing ran
    from tests.test_lora_cpu import _nvs
    nv = _nvs({"do_lora": False})
    nv.set_lora()
    assert nv.unet_lora_params is None and not any(isinstance(s, LoraInjectedLinear) for s in nv.modules())


def test_merged_and_unmerged_forward_against_the_oracle_on_the_merged_weights():
    """no-grad (merged) and grad-enabled (unmerged: base GEMM + lr_lora_down + lr_lora_up) forwards with the golden's factor values;
    yardstick: the oracle's fp32 forward on the merged state dict; bound: tests/test_gpu_unet.py::assert_unet_row (the MID forward's)."""
    from oracle import unet_ref
    from tests.test_gpu_unet import assert_unet_row, stats, viol_frac
    cfg = G.CONFIGS["MID"]
    x, t, ctx = _unet_case()
    m = _injected_unet()
    sd = _merged_state(m)
    ref = unet_ref.unet_forward(sd, cfg, x, t, ctx)
    emul = unet_ref.unet_forward(sd, cfg, x, t, ctx, mode="autocast16")
    rel_e, mx_e = stats("lora autocast16-emulation", emul, ref)
    with torch.no_grad():
        y_merged = m(x.to(dev()), t.to(dev()), ctx.to(dev()))
    assert m._plan is not m._plan["root"]
    y_unmerged = m(x.to(dev()), t.to(dev()), ctx.to(dev())).detach()
    assert m._plan is m._plan["root"] and y_unmerged is not None
    base = _plain_unet().to(dev()).eval()
    with torch.no_grad():
        y_base = base(x.to(dev()), t.to(dev()), ctx.to(dev()))
    moved = ((y_merged.float() - y_base.float()).norm() / y_base.float().norm()).item()
    print(f"[lora forward] the factors move the output by rel_l2 {moved:.3e}")
    assert moved > 10 * rel_e                                        # the low-rank term is far above the noise both routes are held to
    for name, y in (("merged", y_merged), ("unmerged", y_unmerged)):
        rel, mx = stats("lora forward " + name, y, ref)
        row = dict(rel=rel, rel_emu=rel_e, max_abs=mx, max_abs_emu=mx_e, viol=viol_frac(y, ref), viol_emu=viol_frac(emul, ref),
                   rel_hip_vs_emu=((y.float().cpu() - emul).norm() / emul.norm()).item())
        print(f"[lora forward {name}] {row}")
        assert_unet_row(row)


def _oracle_factor_grads(m, mode, x_in, t, ctx, noise):
    """d mse(unet(x_in, t, ctx), noise) / d factors by torch.autograd through the oracle on W + scale up down (CPU)."""
    from oracle import unet_ref
    cfg = G.CONFIGS["MID"]
    sd, leaves = {}, {}
    mods = dict(m.named_modules())
    for k, v in m.state_dict().items():
        v = v.detach().float().cpu()
        if ".lora_down." in k or ".lora_up." in k:
            continue
        if ".linear." in k:
            name = k.split(".linear.")[0]
            if k.endswith("weight"):
                mod = mods[name]
                up = mod.lora_up.weight.detach().float().cpu().clone().requires_grad_(True)
                down = mod.lora_down.weight.detach().float().cpu().clone().requires_grad_(True)
                leaves[name + ".lora_up.weight"], leaves[name + ".lora_down.weight"] = up, down
                v = v + mod.scale * (up @ down)
            k = k.replace(".linear.", ".")
        sd[k] = v
    with torch.enable_grad():
        out = unet_ref.unet_forward.__wrapped__(sd, cfg, x_in, t, ctx, mode=mode)
        torch.nn.functional.mse_loss(out, noise).backward()
    return {k: v.grad for k, v in leaves.items()}


def test_factor_gradients_against_the_reference():
    """p_losses + backward at loss scale 2^14 (as test_training_step_vs_reference_golden) with trainable factors: loss and d context
    take that test's bounds; every factor gradient's norm and the full gradients of three transformer blocks are compared with the REAL
    reference's (tests/golden/lora.npz) by rel-L2 under max(2 e, 1e-2), e = the same quantity's error of the oracle's autocast16
    emulation differentiated through W + scale up down on the CPU (the form of test_unet_context_gradient_matches_oracle_autograd).
    A second run and recompute_in_backward = True are bit-identical.  LEFTREFILL_WRITE_PROFILES=1 writes profiles/lora_parity.json."""
    import leftrefill_amd.dropin as dropin
    dropin.install()
    from inpainting_ldm.NVS_ldm import NVSLDM
    from tools.make_golden_lora import set_factors
    g = _golden()
    gt = np.load(os.path.join(ROOT, "tests", "golden", "train.npz"))
    cfg = G.CONFIGS["MID"]
    m = NVSLDM(first_stage_config={"target": "torch.nn.Identity"}, cond_stage_config={"target": "torch.nn.Identity"},
               unet_config={"target": "ldm.modules.diffusionmodules.openaimodel.UNetModel", "params": cfg.kwargs()},
               conditioning_key="hybrid", scale_factor=0.18215, linear_start=0.00085, linear_end=0.0120, timesteps=1000, channels=4,
               data_config={"img_size": 256}, lora={"do_lora": True, "lora_type": "default", "lora_rank": 4, "lora_scale": 1.0})
    unet = m.model.diffusion_model
    unet.load_state_dict(G.unet_state("MID"), strict=True)
    m.set_lora()
    set_factors(unet, 4)
    m = m.to(dev()).train()
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

    def run():
        for p in factors.values():
            p.grad = None
        c_cross = c_cross0.to(dev()).requires_grad_(True)
        loss, _ = m.p_losses(x_start.to(dev()), {"c_concat": [c_concat.to(dev())], "c_crossattn": [c_cross]}, t.to(dev()), noise=noise.to(dev()))
        (loss * scale).backward()
        return loss.item(), c_cross.grad.float().cpu() / scale, {n: p.grad.detach().clone() for n, p in factors.items()}

    loss, dctx, grads = run()
    assert all(v.dtype == torch.float32 and torch.isfinite(v).all() for v in grads.values())
    ref_loss, ref_dctx = float(g["loss"]), torch.from_numpy(g["dctx"])
    rel_ctx = ((dctx - ref_dctx).norm() / ref_dctx.norm()).item()
    print(f"[lora train] loss {loss:.6f} (reference {ref_loss:.6f}); d/dcontext rel_l2 {rel_ctx:.3e}")
    # the noise floor: the oracle's fp32 and autocast16 gradients of the same loss (x_noisy from the reference's q_sample, train.npz)
    x_in = torch.cat([torch.from_numpy(gt[case + ".x_noisy"]), c_concat], dim=1)
    o32 = _oracle_factor_grads(unet, "fp32", x_in, t, c_cross0, noise)
    o16 = _oracle_factor_grads(unet, "autocast16", x_in, t, c_cross0, noise)
    names = [str(n) for n in g["grad_names"]]
    ref_norm = dict(zip(names, g["grad_norms"]))
    rows, worst = {}, 0.0
    for n in names:
        got = grads[n].double().cpu().norm().item() / scale
        e = abs(o16[n].double().norm().item() - o32[n].double().norm().item()) / o32[n].double().norm().item()
        err = abs(got - ref_norm[n]) / ref_norm[n]
        rows[n] = dict(norm_rel_err=err, norm_emul=e, bound=max(2 * e, 1e-2))
        worst = max(worst, err / rows[n]["bound"])
    full = [k[len("grad."):] for k in g.files if k.startswith("grad.")]
    assert len(full) == 3 * 18
    for n in full:
        ref = torch.from_numpy(g["grad." + n]).double()
        got = grads[n].double().cpu() / scale
        e = ((o16[n].double() - o32[n].double()).norm() / o32[n].double().norm()).item()
        rows[n].update(rel_l2=((got - ref).norm() / ref.norm()).item(), rel_l2_emul=e, rel_l2_bound=max(2 * e, 1e-2),
                       oracle_fp32_vs_reference=((o32[n].double() - ref).norm() / ref.norm()).item())
    worst_full = max(rows[n]["rel_l2"] / rows[n]["rel_l2_bound"] for n in full)
    print(f"[lora train] factor-gradient norms: worst err / bound {worst:.3f} over {len(names)} factors; full gradients of 3 blocks: worst "
          f"rel_l2 / bound {worst_full:.3f} (max rel_l2 {max(rows[n]['rel_l2'] for n in full):.3e})")
    if os.environ.get("LEFTREFILL_WRITE_PROFILES"):
        out_dir = os.environ.get("LEFTREFILL_PROFILE_DIR") or os.path.join(ROOT, "profiles")
        with open(os.path.join(out_dir, "lora_parity.json"), "w") as f:
            json.dump(dict(case=case, loss=loss, reference_loss=ref_loss, dctx_rel_l2=rel_ctx, worst_norm_err_over_bound=worst,
                           worst_full_rel_l2_over_bound=worst_full, factors=rows), f, indent=1)
    assert abs(loss - ref_loss) <= 2e-3 * ref_loss
    assert torch.isfinite(dctx).all() and rel_ctx <= 1e-2
    bad = [n for n in names if rows[n]["norm_rel_err"] > rows[n]["bound"]] + [n for n in full if rows[n]["rel_l2"] > rows[n]["rel_l2_bound"]]
    assert not bad, [(n, rows[n]) for n in bad[:5]]
    # a second run is bit-identical (fixed-order split sums, no atomics), and so is the reference's activation checkpointing
    _, dctx2, grads2 = run()
    assert torch.equal(dctx2, dctx) and all(torch.equal(grads2[n], grads[n]) for n in names)
    unet.recompute_in_backward = True
    _, dctx3, grads3 = run()
    unet.recompute_in_backward = False
    assert torch.equal(dctx3, dctx) and all(torch.equal(grads3[n], grads[n]) for n in names)


# ---------------------------------------------------------------------------------------------------------------------
# end to end: NVSLDM with the reference's lora block, three Trainer.fit steps, checkpoint, resume, sampling
# ---------------------------------------------------------------------------------------------------------------------
def _nvs_model(seed=0, lora=True):
    import leftrefill_amd.dropin as dropin
    dropin.install()
    from inpainting_ldm.NVS_ldm import NVSLDM
    from tests.test_gpu_trainer import _Encoder

    class Tiny(NVSLDM):
        def get_input(self, batch, k, **kw):      # latents and conditioning straight from the batch: no VAE, no tokenizer
            enc = self.cond_stage_model
            ctx = torch.cat([batch["ctx"][:, :1], batch["ctx"][:, 1:51] + enc.special_embeddings.weight, batch["ctx"][:, 51:]], dim=1)
            return batch["x"], {"c_concat": [batch["c_concat"]], "c_crossattn": [ctx], "c_input": None}

        def get_unconditional_conditioning(self, N):
            return torch.zeros(N, 77, self.cond_stage_model.special_embeddings.weight.shape[1], device=self.device)

        def decode_first_stage(self, z, **kw):
            return z

    cfg = G.CONFIGS["MID"]
    torch.manual_seed(seed)
    m = Tiny(first_stage_config={"target": "torch.nn.Identity"}, cond_stage_config={"target": "torch.nn.Identity"},
             unet_config={"target": "ldm.modules.diffusionmodules.openaimodel.UNetModel", "params": cfg.kwargs()},
             conditioning_key="hybrid", scale_factor=0.18215, linear_start=0.00085, linear_end=0.0120, timesteps=1000, channels=4,
             data_config={"img_size": 16, "cfg": 2.5}, save_prompt_only=True,
             lora={"do_lora": lora, "lora_type": "default", "lora_rank": 4, "lora_scale": 1.0})
    m.model.diffusion_model.load_state_dict(G.unet_state("MID"), strict=True)
    m.cond_stage_model = _Encoder(cfg.context_dim)
    m.set_lora()                                                      # after the base weights, before the optimizer
    m.optim_cfg = {"learning_rate": 1e-3, "weight_decay": 0.01, "lr_scheduler": "cosine", "eta_min": 0.01, "lr_lora": 1e-3, "wd_lora": 0.0}      # (no decay on the factors: only a gradient moves them)
    return m.to(dev()), cfg


def test_three_training_steps_checkpoint_resume_and_sampling(tmp_path):
    import importlib
    from leftrefill_amd.trainer import Trainer
    from tests.test_gpu_trainer import _batches
    m, cfg = _nvs_model()
    unet = m.model.diffusion_model
    factors = {n: p for n, p in m.named_parameters() if ".lora_" in n}
    before = {n: p.detach().clone() for n, p in factors.items()}
    batches = _batches(cfg, 3)
    log_batch = dict(batches[0], image=torch.zeros(2, 8, 16, 3, device=dev()), masked_image=torch.zeros(2, 8, 16, 3, device=dev()))
    sample = lambda: m.log_images(log_batch, N=2, ddim_steps=2, unconditional_guidance_scale=2.5)["pred"].float().clone()
    torch.manual_seed(7)
    s0 = sample()
    convs0 = [id(p_) for steps in unet._plan["root"]["input"] + [unet._plan["root"]["middle"]] + unet._plan["root"]["output"]
              for kind, p_ in steps if kind != "st"]
    tr = Trainer(max_steps=3, precision=16, growth_interval=3, default_root_dir=str(tmp_path), verbose=False)
    torch.manual_seed(123)
    tr.fit(m, batches)
    print("[lora e2e] amp state", tr.optimizer.amp_state())
    assert len(tr.optimizer.param_groups) == 2 and tr.optimizer.amp_state()["applied_steps"] >= 2      # (a skipped step is the scaler's business)
    after = {n: p.detach().clone() for n, p in factors.items()}
    assert all(torch.isfinite(v).all() for v in after.values())
    moved_down = [n for n in after if ".lora_down." in n and not torch.equal(after[n], before[n])]
    moved_up = [n for n in after if ".lora_up." in n and not torch.equal(after[n], before[n])]
    assert len(moved_up) == len(after) // 2, "every up factor moves from zero"
    # wd_lora = 0: a down factor moves only through d down, which is zero while up is (step 1) and nonzero from step 2 on
    assert len(moved_down) == len(after) // 2, "every down factor moves once up is nonzero"
    # sampling after training: the merge is rebuilt although the optimizer wrote the factors through raw pointers (no _version bump) ...
    m.eval()
    torch.manual_seed(7)
    s1 = sample()
    assert not torch.equal(s1, s0)
    plan = unet._plan["root"]
    convs1 = [id(p_) for steps in plan["input"] + [plan["middle"]] + plan["output"] for kind, p_ in steps if kind != "st"]
    assert convs1 == convs0, "the conv packing objects survive training and re-merging: no full re-pack"
    # ... and matches the unmerged forward of the trained factors within the forward bound (one UNet evaluation, both routes)
    x = torch.randn(2, 9, 8, 16, generator=torch.Generator().manual_seed(3)).to(dev())
    t = torch.tensor([501, 21], device=dev())
    ctx = batches[0]["ctx"]
    with torch.no_grad():
        y_m = unet(x, t, context=ctx).float()
    assert unet._plan is not unet._plan["root"]
    for p in factors.values():
        p.requires_grad_(True)
    y_u = unet(x, t, context=ctx).detach().float()
    assert unet._plan is unet._plan["root"]
    rel = ((y_m - y_u).norm() / y_u.norm()).item()
    print(f"[lora e2e] merged vs unmerged after training rel_l2 {rel:.3e}")
    # a second training forward + re-merge: the merged plan holds no earlier merged plan and no training-only entries (nothing piles up)
    merged1 = unet._plan["root"]["merged"]
    unet(x, t, context=ctx)
    with torch.no_grad():
        unet(x, t, context=ctx)
    merged2 = unet._plan["root"]["merged"]
    assert merged2 is not merged1 and unet._plan is merged2 and not {"merged", "merged_stale", "kv_all_w"} & set(merged2)
    assert set(unet._plan["root"]) - set(merged2) <= {"merged", "merged_stale", "kv_all_w"}      # ... and lacks nothing else of the packing
    for p in factors.values():
        p.requires_grad_(True)
    assert rel <= 4e-3                                                # (test_gpu_unet.py's cap on the MID forward's rel-L2)
    # last.ckpt holds the factor keys, and a fresh model resumes to the same values
    load_state_dict = importlib.import_module("inpainting_ldm.model").load_state_dict
    path = os.path.join(str(tmp_path), "ckpts", "last.ckpt")
    sd = load_state_dict(path)
    assert sorted(k for k in sd if ".lora_" in k) == sorted(after) and not any(".linear." in k for k in sd)
    m2, _ = _nvs_model(seed=9)
    res = m2.load_state_dict(sd, strict=False)
    assert not res.unexpected_keys
    assert all(torch.equal(p.detach(), after[n]) for n, p in m2.named_parameters() if ".lora_" in n)


def test_standalone_modules_apply_the_factors():
    """The drop-in FeedForward / CrossAttention modules called on their own (not through UNetModel's plan) run an injected Linear
    unmerged: against the plain-torch statement of the same modules on the CPU (fp32 on the 16-bit-rounded inputs and weights)."""
    import torch.nn.functional as F
    _plain_unet()                                                    # (installs the drop-in packages)
    from inpainting_ldm.lora import LoraInjectedLinear, inject_trainable_lora
    from ldm.modules.attention import CrossAttention, FeedForward
    torch.manual_seed(11)
    h16 = lambda t_: t_.half().float()
    ff, ca = FeedForward(320, glu=True), CrossAttention(320, 1024, heads=5, dim_head=64)
    for mod in (ff, ca):
        inject_trainable_lora(mod, r=8, scale=0.5)
        with torch.no_grad():
            for n, p in mod.named_parameters():
                p.copy_(h16(torch.randn_like(p) * (0.05 if ".lora_up." in n else 1.0 / 8 if ".lora_down." in n else p.shape[-1] ** -0.5 if p.dim() > 1 else 0.1)))
    lin = lambda m_, x_: m_(x_) if isinstance(m_, LoraInjectedLinear) else F.linear(x_, m_.weight, m_.bias)
    x, ctx = h16(torch.randn(2, 96, 320)), h16(torch.randn(2, 77, 1024))
    with torch.no_grad():
        u, g = lin(ff.net[0].proj, x).chunk(2, dim=-1)
        ref_ff = lin(ff.net[2], u * F.gelu(g))
        q, k, v = (lin(m_, s_).reshape(2, -1, 5, 64).transpose(1, 2) for m_, s_ in ((ca.to_q, x), (ca.to_k, ctx), (ca.to_v, ctx)))
        a = torch.softmax(q @ k.transpose(-1, -2) * 0.125, dim=-1) @ v
        ref_ca = lin(ca.to_out[0], a.transpose(1, 2).reshape(2, 96, 320))
        assert isinstance(ff.net[0].proj, LoraInjectedLinear) and isinstance(ca.to_out[0], LoraInjectedLinear)
        ff, ca = ff.to(dev()), ca.to(dev())
        got_ff, got_ca = ff(x.to(dev())), ca(x.to(dev()), context=ctx.to(dev()))
    check("standalone FeedForward", got_ff, ref_ff, rtol=4e-3, atol_scale=4e-3)      # (two 16-bit GEMMs and the gate in a row: twice check()'s single-op bound)
    check("standalone CrossAttention", got_ca, ref_ca, rtol=4e-3, atol_scale=4e-3)
