"""tests/golden/lora.npz: LoRA factor gradients of the REAL reference on the CPU (authoring container only; the reference does not travel).

    python -m tools.make_golden_lora

The reference's MID UNet (oracle.golden_spec.unet_state("MID")) gets the reference's own `inject_trainable_lora` (r = 4, scale = 1.0);
both factors of every injected layer are set from names (`factor_values`: nothing random, the `up` factor nonzero or `d down` would be
zero), then `p_losses` + backward run on TRAIN_CASES[0] exactly as oracle/make_golden.py::gen_train does for train.npz.  Stored: the
loss, d context, the injected child names, the sorted state-dict keys, the float64 Frobenius norm of every factor gradient and the full
fp32 gradients of the first input, the middle and the last output transformer block.  No reference code is stored, only these arrays.
"""
import importlib
import os
import sys
import types

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from oracle import golden_spec as G  # noqa: E402

R, SCALE = 4, 1.0
OUT = os.path.join(ROOT, "tests", "golden", "lora.npz")


def factor_values(layer, r, in_features, out_features):
    """(down [r, in], up [out, r]) of the injected layer with full module name `layer` (e.g. `input_blocks.1.1.transformer_blocks.0.attn1.to_q`)."""
    return G.T(layer + ".lora_down", (r, in_features)) / r, G.T(layer + ".lora_up", (out_features, r)) * 0.02


def lora_layers(model):
    """[(full module name, module)] of the injected layers, in module order."""
    return [(n, m) for n, m in model.named_modules() if hasattr(m, "lora_down") and hasattr(m, "lora_up")]


def set_factors(model, r=R):
    with torch.no_grad():
        for name, m in lora_layers(model):
            down, up = factor_values(name, r, m.lora_down.weight.shape[1], m.lora_up.weight.shape[0])
            m.lora_down.weight.copy_(down)
            m.lora_up.weight.copy_(up)


def full_blocks(layer_names):
    """Prefixes of the first input, the middle and the last output SpatialTransformer among the injected layers."""
    sts = list(dict.fromkeys(n.split(".transformer_blocks.")[0] + "." for n in layer_names))
    ins = [s for s in sts if s.startswith("input_blocks.")]
    mid = [s for s in sts if s.startswith("middle_block.")]
    outs = [s for s in sts if s.startswith("output_blocks.")]
    return ins[0], mid[0], outs[-1]


def main():
    from oracle import make_golden as MG, ref_import
    torch.manual_seed(0)
    ns = ref_import.import_reference()
    ref_lora = importlib.import_module("inpainting_ldm.lora")
    cfg = G.CONFIGS["MID"]
    ucfg = {"target": "ldm.modules.diffusionmodules.openaimodel.UNetModel", "params": cfg.kwargs()}
    wrapper = ns.ddpm.DiffusionWrapper(ucfg, "hybrid")
    unet = wrapper.diffusion_model
    MG._load(unet, G.unet_state("MID"))
    params, names = ref_lora.inject_trainable_lora(unet, r=R, scale=SCALE)
    param_ids = [id(p) for gen in params for p in gen]
    set_factors(unet)
    layers = lora_layers(unet)
    # the order of unet_lora_params: (up, down) per layer, layers in injection order
    by_id = {id(m.lora_up.weight): n + ".lora_up.weight" for n, m in layers}
    by_id.update({id(m.lora_down.weight): n + ".lora_down.weight" for n, m in layers})
    out = {"names": np.array(names), "keys": np.array(sorted(unet.state_dict().keys())), "param_order": np.array([by_id[i] for i in param_ids]),
           "r": np.array(R), "scale": np.array(SCALE)}

    case, B, h, w, ts = G.TRAIN_CASES[0]
    fake = MG._FakeLDM(ns, wrapper=wrapper)
    fake.register_buffer = lambda name, val, persistent=True, _f=fake: setattr(_f, name, val)
    fake.v_posterior = 0.
    ns.ddpm.DDPM.register_schedule(fake, beta_schedule="linear", timesteps=1000, linear_start=0.00085, linear_end=0.0120)
    fake.loss_type, fake.learn_logvar, fake.logvar = "l2", False, torch.zeros(1000)
    fake.l_simple_weight, fake.original_elbo_weight, fake.training = 1., 0., True
    fake.q_sample = types.MethodType(ns.ddpm.DDPM.q_sample, fake)
    fake.get_loss = types.MethodType(ns.ddpm.DDPM.get_loss, fake)
    x_start = G.T(case + ".x_start", (B, 4, h, w))
    noise = G.T(case + ".noise", (B, 4, h, w))
    c_concat = G.T(case + ".c_concat", (B, 5, h, w))
    c_cross = G.T(case + ".c_cross", (B, 77, cfg.context_dim)).requires_grad_(True)
    t = torch.tensor(ts, dtype=torch.long)
    with torch.enable_grad():
        loss, _ = ns.ddpm.LatentDiffusion.p_losses(fake, x_start, {"c_concat": [c_concat], "c_crossattn": [c_cross]}, t, noise=noise)
        loss.backward()
    out["loss"] = loss.detach().numpy()
    out["dctx"] = c_cross.grad.numpy()
    gnames, norms = [], []
    blocks = full_blocks([n for n, _ in layers])
    for n, m in layers:
        for f in ("lora_down", "lora_up"):
            g = getattr(m, f).weight.grad
            gnames.append(f"{n}.{f}.weight")
            norms.append(float(g.double().norm()))
            if n.startswith(blocks):
                out["grad." + gnames[-1]] = g.numpy().astype(np.float32)
    out["grad_names"], out["grad_norms"] = np.array(gnames), np.array(norms, dtype=np.float64)
    out["full_blocks"] = np.array(blocks)
    np.savez_compressed(OUT, **out)
    print(f"lora golden: loss {float(loss):.6f}, {len(layers)} layers, |d factor| in [{min(norms):.3e}, {max(norms):.3e}], "
          f"{os.path.getsize(OUT) / 1e6:.2f} MB")


if __name__ == "__main__":
    sys.exit(main())
