"""Trainer.fit on the GPU with small synthetic weights: the fp16 AmpAdamW route against the same model stepped by torch.optim.AdamW and a
host-side loss scaler (bench.py's) on identical batches / noise / timesteps; what changes, the checkpoint and resume, accumulation.

The prompt encoder is a stand-in that owns `special_embeddings` and adds them to a fixed context, as bench.py's training workload
does: the CLIP tower between tokens and context has its own tests (test_gpu_prompt_tuning.py).

Token bound: both routes feed bit-identical gradients to the same AdamW arithmetic; per applied step each route rounds the parameter
once (half an fp32 ulp of max|token|) and the update terms differ by a few ulp of the update (lr-sized), so the trajectories may differ
by N ulp32(max|token|) after N steps -- the per-step bound of test_gpu_optim.py scaled by the step count.
"""
import importlib
import json
import os
import subprocess
import sys

import pytest
import torch

from oracle import golden_spec as G

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
B, h, w, CTX = 2, 8, 16, 77
LR, WD = 1e-3, 0.01


class _Encoder(torch.nn.Module):
    def __init__(self, dim):
        super().__init__()
        self.special_embeddings = torch.nn.Embedding(50, dim)
        self.model = torch.nn.Linear(4, 4)      # stands for the frozen CLIP tower
        torch.nn.init.normal_(self.special_embeddings.weight, std=0.02)


def _model(seed=0):
    import leftrefill_amd.dropin as dropin
    dropin.install()
    from inpainting_ldm.ref_inpainting_ldm import RefInpaintLDM

    class Tiny(RefInpaintLDM):
        def get_input(self, batch, k, **kw):      # latents and conditioning straight from the batch: no VAE, no tokenizer
            enc = self.cond_stage_model
            ctx = torch.cat([batch["ctx"][:, :1], batch["ctx"][:, 1:51] + enc.special_embeddings.weight, batch["ctx"][:, 51:]], dim=1)
            return batch["x"], {"c_concat": [batch["c_concat"]], "c_crossattn": [ctx]}

        def shared_step(self, batch, **kw):       # timesteps / noise from the batch when it carries them (no generator involved)
            if "t" not in batch:
                return super().shared_step(batch, **kw)
            x, c = self.get_input(batch, self.first_stage_key)
            return self.p_losses(x, c, batch["t"], noise=batch["noise"])

    cfg = G.CONFIGS["MID"]
    torch.manual_seed(seed)
    m = Tiny(first_stage_config={"target": "torch.nn.Identity"}, cond_stage_config={"target": "torch.nn.Identity"},
             unet_config={"target": "ldm.modules.diffusionmodules.openaimodel.UNetModel", "params": cfg.kwargs()},
             conditioning_key="hybrid", scale_factor=0.18215, linear_start=0.00085, linear_end=0.0120, timesteps=1000, channels=4,
             data_config={"img_size": 16, "cfg": 2.5}, save_prompt_only=True)
    m.model.diffusion_model.load_state_dict(G.unet_state("MID"), strict=True)
    m.cond_stage_model = _Encoder(cfg.context_dim)
    m.optim_cfg = {"learning_rate": LR, "weight_decay": WD, "lr_scheduler": "cosine", "eta_min": 0.01}
    return m.to(DEV), cfg


def _batches(cfg, n, bad_at=None, seed=5, with_t_noise=False):
    g = torch.Generator().manual_seed(seed)
    out = []
    for k in range(n):
        b = {"x": torch.randn(B, 4, h, w, generator=g), "c_concat": torch.randn(B, 5, h, w, generator=g),
             "ctx": torch.randn(B, CTX, cfg.context_dim, generator=g)}
        if with_t_noise:
            b["t"] = torch.randint(0, 1000, (B,), generator=g)
            b["noise"] = torch.randn(B, 4, h, w, generator=g)
        if k == bad_at:
            b["x"][0, 0, 0, 0] = float("inf")      # a non-finite loss: every gradient of this step is non-finite
        out.append({k_: v.to(DEV) for k_, v in b.items()})
    return out


def _tokens(m):
    return m.cond_stage_model.special_embeddings.weight.detach().clone()


def _fit(m, batches, tmp=None, **kw):
    from leftrefill_amd.trainer import Trainer
    kw.setdefault("max_steps", len(batches))
    tr = Trainer(precision=16, growth_interval=3, default_root_dir=tmp, verbose=False, **kw)
    torch.manual_seed(123)
    tr.fit(m, batches)
    return tr


def _torch_route(m, batches, max_steps):
    """bench.py's tail: torch AdamW, loss scale and skip decision on the host, CosineAnnealingLR stepped every iteration."""
    from leftrefill_amd.trainer import Trainer
    m.trainer = Trainer(max_steps=max_steps, precision=16, verbose=False)
    m.train()
    tok = m.cond_stage_model.special_embeddings.weight
    for p in m.parameters():
        p.requires_grad_(p is tok)
    opt = torch.optim.AdamW([tok], lr=LR, weight_decay=WD)
    sche = torch.optim.lr_scheduler.CosineAnnealingLR(opt, max_steps, eta_min=0.01 * LR)
    scale, good, skips = 65536.0, 0, []
    m.model.diffusion_model.compute_dtype = torch.float16
    torch.manual_seed(123)
    for i, b in enumerate(batches):
        loss = m.training_step(b, i)
        (loss * scale).backward()
        bad = not bool(torch.isfinite(tok.grad).all())
        skips.append(int(bad))
        if bad:
            scale, good = scale * 0.5, 0
        else:
            tok.grad /= scale
            opt.step()
            good += 1
            if good == 3:
                scale, good = scale * 2.0, 0
        opt.zero_grad(set_to_none=True)
        sche.step()
    return skips, scale


def test_fit_fp16_matches_torch_adamw_with_a_host_scaler(tmp_path):
    N = 6
    m1, cfg = _model()
    m2, _ = _model()
    backbone = {k: v.detach().clone() for k, v in m1.state_dict().items() if "special_embeddings" not in k}
    t0 = _tokens(m1)
    tr = _fit(m1, _batches(cfg, N, bad_at=2), str(tmp_path))
    skips, scale = _torch_route(m2, _batches(cfg, N, bad_at=2), N)
    s = tr.optimizer.amp_state()
    print("amp state", s, "torch route skips", skips, "scale", scale)
    assert skips == [0, 0, 1, 0, 0, 0] and (s["skipped"], s["applied_steps"], s["sched_steps"]) == (1, N - 1, N)
    assert [int(f) for f in tr.found_inf_history] == skips          # the decision of every single step, not only the totals
    assert s["scale"] == scale and torch.is_tensor(m1.loss_scale) and m1.loss_scale.is_cuda and float(m1.loss_scale) == scale
    a, b = _tokens(m1), _tokens(m2)
    dist, bound = (a - b).abs().max().item(), N * 2.0 ** -23 * a.abs().max().item()
    print(f"tokens: |fit - torch| {dist:.3e}, bound {bound:.3e}, moved {(a - t0).abs().max().item():.3e}")
    assert not torch.equal(a, t0) and dist <= bound
    # only the tokens moved
    after = m1.state_dict()
    assert all(torch.equal(v, after[k]) for k, v in backbone.items())
    assert set(tr.logged) >= {"train/loss_simple", "train/loss_vlb", "train/loss", "global_step", "loss"}

    # last.ckpt -> the evaluation CLI's load path -> a fresh model
    import leftrefill_amd.dropin as dropin
    dropin.install()
    load_state_dict = importlib.import_module("inpainting_ldm.model").load_state_dict
    path = os.path.join(str(tmp_path), "ckpts", "last.ckpt")
    assert os.path.getsize(path) < 2 ** 20
    m3, _ = _model(seed=9)
    res = m3.load_state_dict(load_state_dict(path), strict=False)
    assert not res.unexpected_keys and torch.equal(_tokens(m3), a)


def test_resume_continues_like_an_uninterrupted_run(tmp_path):
    from leftrefill_amd.trainer import Trainer
    N = 5
    m1, cfg = _model()
    batches = _batches(cfg, N)
    _fit(m1, batches)
    # the same run stopped by hand after step 3 (the schedule spans all N steps), saved, and resumed by a fresh model and trainer
    m2, _ = _model()
    tr = Trainer(max_steps=N, precision=16, growth_interval=3, default_root_dir=str(tmp_path), verbose=False)
    torch.manual_seed(123)
    tr._setup(m2)
    for i, b in enumerate(batches[:3]):
        tr._micro_step(m2, b, i)
        tr._optimizer_step()
        tr.global_step += 1
    rng = torch.cuda.get_rng_state(), torch.get_rng_state()
    path = tr.save_checkpoint(m2)
    m3, _ = _model(seed=4)                                  # other initial tokens: they must come from the checkpoint
    m3.model.diffusion_model.load_state_dict(G.unet_state("MID"), strict=True)
    tr2 = Trainer(max_steps=N, precision=16, growth_interval=3, resume_from_checkpoint=path, verbose=False)
    torch.cuda.set_rng_state(rng[0])
    torch.set_rng_state(rng[1])
    tr2.fit(m3, batches[3:])
    assert tr2.global_step == N and tr2.optimizer.amp_state()["sched_steps"] == N
    assert torch.equal(_tokens(m3), _tokens(m1)), (_tokens(m3) - _tokens(m1)).abs().max().item()


def test_accumulate_two_equals_one_step_on_the_summed_gradients():
    m1, cfg = _model()
    batches = _batches(cfg, 2)
    from leftrefill_amd.trainer import Trainer
    tr = Trainer(max_steps=1, precision=16, accumulate_grad_batches=2, verbose=False)
    torch.manual_seed(123)
    tr.fit(m1, batches)
    assert tr.global_step == 1 and tr.optimizer.amp_state()["applied_steps"] == 1
    # by hand: the two scaled half-losses' gradients summed, one AmpAdamW step
    m2, _ = _model()
    tr2 = Trainer(max_steps=1, precision=16, verbose=False)
    tr2._setup(m2)
    torch.manual_seed(123)
    tok = m2.cond_stage_model.special_embeddings.weight
    grads = []
    for i, b in enumerate(batches):
        tr2.optimizer.zero_grad()
        tr2.optimizer.scale(m2.training_step(b, i) / 2).backward()
        grads.append(tok.grad.clone())
    tok.grad.copy_(grads[0] + grads[1])
    tr2.optimizer.step()
    assert torch.equal(_tokens(m1), _tokens(m2))


def test_hip_graph_step_matches_eager():
    """Timesteps and noise travel in the batch, so the captured and the eager run see the same inputs: same decisions at every step and
    tokens within the N-ulp bound of the module docstring (the arithmetic is the same kernels in the same order)."""
    N = 4
    m1, cfg = _model()
    m2, _ = _model()
    t0 = _tokens(m1)
    tr1 = _fit(m1, _batches(cfg, N, bad_at=1, with_t_noise=True))
    tr2 = _fit(m2, _batches(cfg, N, bad_at=1, with_t_noise=True), hip_graph=True)
    s1, s2 = tr1.optimizer.amp_state(), tr2.optimizer.amp_state()
    assert [int(f) for f in tr1.found_inf_history] == [int(f) for f in tr2.found_inf_history] == [0, 1, 0, 0]
    assert s1 == s2 and (s2["skipped"], s2["applied_steps"], s2["sched_steps"], s2["scale"]) == (1, N - 1, N, 32768.0)
    assert tr2.optimizer.param_groups[0]["lr"] == tr1.optimizer.param_groups[0]["lr"]
    a, b = _tokens(m1), _tokens(m2)
    dist, bound = (a - b).abs().max().item(), N * 2.0 ** -23 * a.abs().max().item()
    print(f"tokens: |graph - eager| {dist:.3e}, bound {bound:.3e}, moved {(a - t0).abs().max().item():.3e}")
    assert not torch.equal(b, t0) and dist <= bound


def test_hip_graph_refuses_what_a_capture_would_freeze():
    m, cfg = _model()
    m.ucg_training = {"txt": {"p": 0.1, "val": ""}}
    from leftrefill_amd.trainer import Trainer
    with pytest.raises(RuntimeError, match="ucg_training"):
        Trainer(max_steps=1, precision=16, hip_graph=True, verbose=False).fit(m, _batches(cfg, 1))


def test_two_ranks_share_gpu_identical_tokens_and_a_shared_skip(tmp_path):
    """Two ranks on the one GPU over gloo (the pattern of test_train_workload_two_ranks_share_gpu): rank-dependent batches, the
    non-finite batch on rank 1 only.  The averaged gradient carries the inf to both ranks: both skip that step, and the tokens end
    bit-identical."""
    out = str(tmp_path / "ranks.json")
    env = dict(os.environ, LR_TRAINER_RANKS_OUT=out)
    p = subprocess.run([sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "2", "--master-addr", "127.0.0.1",
                        "--master-port", "29533", os.path.join(os.path.dirname(os.path.abspath(__file__)), "trainer_two_ranks_worker.py")],
                       capture_output=True, text=True, timeout=600, cwd=str(tmp_path), env=env)
    assert p.returncode == 0, (p.stdout[-1500:], p.stderr[-2500:])
    with open(out) as f:
        r = json.load(f)
    print(r)
    assert r["world"] == 2 and r["tokens_bit_identical"] and r["moved"] > 0
    assert r["found_inf"] == [[0, 1, 0, 0], [0, 1, 0, 0]]           # rank 1's overflow skipped both
    assert r["scale"] == [32768.0, 32768.0] and r["ckpt_written_by"] == [True, False]
