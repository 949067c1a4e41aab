"""Golden vectors of prompt tuning from the REFERENCE's own code on the CPU (writes tests/golden/prompt_tuning.npz).

open_clip is bound to oracle/clip_stub.py, as oracle/make_golden_text.py does; the reference's task-model modules are imported with
stand-ins for the dataset / metric packages they import at module level but never use on these paths.
  a. tower gradient: for TEXT_CASES, MV_TEXT_CASES and NVS_TEXT_CASES, the reference encoder's z (rows G.NVS_Z_ROWS) and
     d(sum z * dz) / d special_embeddings.weight for dz = G.T("prompt_tuning.<case>.dz"); NVS: also the rel_pos_model gradients
     (weights: the first REL_ROWS rows).
  b. whole prompt-tuning step: the reference PromptCLIPEmbedder (stub-1024, penultimate, repeat_8_<special-token>) feeds its z as
     c_crossattn into LatentDiffusion.p_losses on the MID UNet widened to a 1024-wide context (fake-LDM set-up of
     oracle/make_golden.gen_train, TRAIN_CASES inputs): loss, loss_dict and d loss / d special_embeddings.weight.
  c. multi-view objective: the reference's multi-view RefInpaintLDM.p_losses on golden_spec.mv_config (concat_target True with V = 3,
     False with V = 2): loss, loss_dict and d loss / d context (rows G.NVS_Z_ROWS of every canvas).

    python tools/make_golden_prompt_tuning.py
"""
import dataclasses
import os
import sys
import types

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from oracle import clip_stub, golden_spec as G, ref_import, unet_ref, weights  # noqa: E402

PT_PROMPT = "".join(f"<special-token{i}>" for i in range(8))
PT_KW = dict(arch="stub-1024", layer="penultimate", special_tokens=["repeat_8_<special-token>"], init_text=[G._TXT])
PT_PROMPTS = [PT_PROMPT, "a photo of <special-token3> and a cat"]
REL_ROWS = 16      # rows of the rel_pos_model weight gradients kept
PT_UNET = dataclasses.replace(unet_ref.MID, context_dim=1024)
# multi-view objective cases: (name, view_num, concat_target, samples b, latent h, w, timesteps per sample)
MV_LOSS_CASES = [("mvloss_concat_v3", 3, True, 2, 8, 16, [501, 21]), ("mvloss_plain_v2", 2, False, 2, 8, 8, [801, 101])]


def pt_unet_state():
    return weights.fill_state_dict(unet_ref.param_shapes(PT_UNET), prefix="unet.PT1024.")


def _stub_modules():
    for name in ("dataloaders", "dataloaders.inpainting_dataset", "dataloaders.inpainting_crossview_dataset", "torchmetrics",
                 "torchmetrics.functional", "skimage", "skimage.metrics", "torchvision.transforms", "torchvision.transforms.functional"):
        if name not in sys.modules:
            sys.modules[name] = types.ModuleType(name)
    for n in ("InpaintingDataset", "InpaintingCrossViewDataset", "InpaintingMultiViewDataset", "BalancedRandomSampler"):
        setattr(sys.modules["dataloaders.inpainting_dataset"], n, object)
        setattr(sys.modules["dataloaders.inpainting_crossview_dataset"], n, object)
    sys.modules["torchmetrics.functional"].peak_signal_noise_ratio = None
    sys.modules["skimage.metrics"].structural_similarity = None


def _fake_ldm(ns, wrapper):
    from oracle.make_golden import _FakeLDM
    fake = _FakeLDM(ns, wrapper=wrapper)
    fake.register_buffer = lambda name, val, persistent=True, _f=fake: setattr(_f, name, val)
    fake.v_posterior = 0.
    ns.ddpm.DDPM.register_schedule(fake, beta_schedule="linear", timesteps=1000, linear_start=0.00085, linear_end=0.0120)
    fake.loss_type, fake.learn_logvar, fake.logvar = "l2", False, torch.zeros(1000)
    fake.l_simple_weight, fake.original_elbo_weight, fake.training = 1., 0., True
    fake.q_sample = types.MethodType(ns.ddpm.DDPM.q_sample, fake)
    fake.get_loss = types.MethodType(ns.ddpm.DDPM.get_loss, fake)
    return fake


def _load(m, sd):
    m.load_state_dict({k: v for k, v in sd.items()}, strict=True)


def gen_tower(out, R, MV, NV):
    cases = ([(n, R.PromptCLIPEmbedder, kw, p, None) for n, kw, p in G.TEXT_CASES] +
             [(n, MV.PromptCLIPEmbedder, kw, p, None) for n, kw, p in G.MV_TEXT_CASES] +
             [(n, NV.NVSCLIPEmbedder, kw, p, ps) for n, kw, p, ps in G.NVS_TEXT_CASES])
    for name, cls, kw, prompts, pose_shape in cases:
        torch.manual_seed(0)
        emb = cls(device="cpu", **{k: (list(v) if isinstance(v, list) else v) for k, v in kw.items()})
        emb.eval()
        emb.special_embeddings.weight.requires_grad_(True)
        rel = getattr(emb, "rel_pos_model", None) if pose_shape is not None else None
        if rel is not None:
            rel.load_state_dict(G.nvs_pose_state(name, rel.state_dict()))
            for p in rel.parameters():
                p.requires_grad_(True)
        with torch.enable_grad():
            z = emb(prompts if pose_shape is None else [prompts, G.T(name + ".rel_pos", pose_shape)])
            dz = G.T(f"prompt_tuning.{name}.dz", tuple(z.shape))
            (z * dz).sum().backward()
        out[name + ".z_shape"] = np.asarray(z.shape)
        out[name + ".z_rows"] = z.detach()[..., G.NVS_Z_ROWS, :].numpy()
        out[name + ".d_special"] = emb.special_embeddings.weight.grad.numpy()
        if rel is not None:
            for k, p in rel.named_parameters():      # weights: the first REL_ROWS output rows (size limit), biases whole
                out[f"{name}.d_rel_pos.{k}"] = (p.grad[:REL_ROWS] if p.dim() == 2 else p.grad).numpy()
        print(f"  tower {name}: z {tuple(z.shape)} |d special| max {emb.special_embeddings.weight.grad.abs().max():.3e}")


def gen_step(out, ns, R):
    case, B, h, w, ts = G.TRAIN_CASES[0]
    torch.manual_seed(0)
    emb = R.PromptCLIPEmbedder(device="cpu", **PT_KW)
    emb.eval()
    emb.special_embeddings.weight.requires_grad_(True)
    wrapper = ns.ddpm.DiffusionWrapper({"target": "ldm.modules.diffusionmodules.openaimodel.UNetModel", "params": PT_UNET.kwargs()},
                                       "hybrid")
    _load(wrapper.diffusion_model, pt_unet_state())
    fake = _fake_ldm(ns, wrapper)
    x_start = G.T(case + ".x_start", (B, 4, h, w))
    noise = G.T(case + ".noise", (B, 4, h, w))
    c_concat = G.T(case + ".c_concat", (B, 5, h, w))
    t = torch.tensor(ts, dtype=torch.long)
    with torch.enable_grad():
        z = emb(PT_PROMPTS[:B])
        loss, ld = ns.ddpm.LatentDiffusion.p_losses(fake, x_start, {"c_concat": [c_concat], "c_crossattn": [z]}, t, noise=noise)
        loss.backward()
    out["step.loss"] = loss.detach().numpy()
    out["step.loss_simple"] = ld["train/loss_simple"].detach().numpy()
    out["step.loss_vlb"] = ld["train/loss_vlb"].detach().numpy()
    out["step.d_special"] = emb.special_embeddings.weight.grad.numpy()
    print(f"  step: loss {float(loss):.6f} |d special| max {emb.special_embeddings.weight.grad.abs().max():.3e}")


def gen_mv_loss(out, ns, MVLDM):
    for name, V, concat, b, h, w, ts in MV_LOSS_CASES:
        cfg = G.mv_config(V, concat)
        # the reference's CheckpointFunction cannot differentiate the multi-view blocks (a bool among its input tensors):
        # run them without recomputation, which changes no value
        unet = ns.multiview_unet.MultiViewUnetModel(**dict(cfg.kwargs(), use_checkpoint=False))
        _load(unet, weights.fill_state_dict(unet_ref.param_shapes(cfg), prefix="unet.MV."))
        wrapper = ns.ddpm.DiffusionWrapper({"target": "torch.nn.Identity"}, "hybrid")
        wrapper.diffusion_model = unet
        fake = _fake_ldm(ns, wrapper)
        fake.view_num, fake.concat_target = V, concat
        v = V - 1 if concat else V
        n = b * v
        x_start = G.T(name + ".x_start", (n, 4, h, w))
        noise = G.T(name + ".noise", (n, 4, h, w))
        c_concat = G.T(name + ".c_concat", (n, 5, h, w))
        ctx = G.T(name + ".ctx", (n, 77, cfg.context_dim)).requires_grad_(True)
        t = torch.tensor([tt for tt in ts for _ in range(v)], dtype=torch.long)
        with torch.enable_grad():
            loss, ld = MVLDM.p_losses(fake, x_start, {"c_concat": [c_concat], "c_crossattn": [ctx]}, t, noise=noise)
            loss.backward()
        out[name + ".loss"] = loss.detach().numpy()
        for k, val in ld.items():
            out[f"{name}.{k.split('/')[-1]}"] = val.detach().numpy()
        out[name + ".keys"] = np.asarray(sorted(ld))
        out[name + ".dctx_rows"] = ctx.grad[:, G.NVS_Z_ROWS].numpy()
        print(f"  mv loss {name}: loss {float(loss):.6f} |dctx| max {ctx.grad.abs().max():.3e}")


def main():
    torch.manual_seed(0)
    sys.modules["open_clip"] = clip_stub
    from transformers import CLIPTextModel, CLIPTokenizer, T5EncoderModel, T5Tokenizer  # noqa: F401  (see make_golden_text.py)
    ns = ref_import.import_reference()
    _stub_modules()
    from ldm.modules.encoders import Refill_modules as R, multiview_Refill_modules as MV, NVS_modules as NV
    from inpainting_ldm.multiview_ref_inpainting_ldm import RefInpaintLDM as MVLDM
    out = {}
    gen_tower(out, R, MV, NV)
    gen_step(out, ns, R)
    gen_mv_loss(out, ns, MVLDM)
    path = os.path.join(ROOT, "tests", "golden", "prompt_tuning.npz")
    np.savez_compressed(path, **out)
    print("wrote", path, os.path.getsize(path))


if __name__ == "__main__":
    main()
