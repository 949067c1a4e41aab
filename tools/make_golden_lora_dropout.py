"""tests/golden/lora_dropout.npz: LoRA factor gradients of the REAL reference WITH LoRA dropout, on the CPU (authoring container only; the
reference does not travel).

    python -m tools.make_golden_lora_dropout

Built like tools/make_golden_lora.py: the reference's MID UNet gets the reference's own `inject_trainable_lora(unet, r=4, scale=1.0,
dropout_p=0.1)` and the factor values of `make_golden_lora.factor_values`.  The `dropout` submodule of injected layer i (injection order) is
then replaced by a module that multiplies its [.., N] input by `keep(seed=20240807, stream=i, draw=0, row, col) * inv_keep` -- the mask
leftrefill_amd/lora_dropout.py states, row = the input's row in [M, N] order -- and `p_losses` + backward run on TRAIN_CASES[0].

Stored, as lora.npz does: the loss, d context, the float64 norm of every factor gradient and the full fp32 gradients of the same three
blocks; the stream id of every layer; and per stored quantity the noise floor `e`: the fp32-vs-autocast16 difference of the project's own
oracle on the dropout-free merged weights (tests/test_gpu_lora.py::_oracle_factor_grads), so that the GPU test runs no CPU oracle.
No reference code is stored, only these arrays.
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
from leftrefill_amd import lora_dropout  # noqa: E402
from tools.make_golden_lora import R, SCALE, full_blocks, lora_layers, set_factors  # noqa: E402

P, SEED, DRAW = 0.1, 20240807, 0
OUT = os.path.join(ROOT, "tests", "golden", "lora_dropout.npz")


class StatedMask(torch.nn.Module):
    """x -> x * keep * inv_keep with the stated counter-based mask of one stream at one draw."""

    def __init__(self, stream, p=P, seed=SEED, draw=DRAW):
        super().__init__()
        self.stream, self.p, self.seed, self.draw = stream, p, seed, draw

    def forward(self, x):
        n = x.shape[-1]
        keep = lora_dropout.keep_mask(self.seed, self.stream, self.draw, x.numel() // n, n, self.p)
        keep = torch.from_numpy(np.ascontiguousarray(keep)).reshape(x.shape)
        return torch.where(keep, x * lora_dropout.inv_keep(self.p), torch.zeros((), dtype=x.dtype))


def main():
    from oracle import make_golden as MG, ref_import
    from tests.test_gpu_lora import _oracle_factor_grads
    torch.manual_seed(0)
    ns = ref_import.import_reference()
    ref_lora = importlib.import_module("inpainting_ldm.lora")
    cfg = G.CONFIGS["MID"]
    ucfg = {"target": "ldm.modules.diffusionmodules.openaimodel.UNetModel", "params": cfg.kwargs()}
    wrapper = ns.ddpm.DiffusionWrapper(ucfg, "hybrid")
    unet = wrapper.diffusion_model
    MG._load(unet, G.unet_state("MID"))
    params, names = ref_lora.inject_trainable_lora(unet, r=R, scale=SCALE, dropout_p=P)
    set_factors(unet)
    layers = lora_layers(unet)
    # injection order = the order of the returned parameter iterators: (up, down) per layer
    by_up = {id(m.lora_up.weight): (n, m) for n, m in layers}
    order = [by_up[id(p)] for gen in params for p in gen if id(p) in by_up]
    assert len(order) == len(layers) == len(names)
    for i, (n, m) in enumerate(order):
        assert isinstance(m.dropout, torch.nn.Dropout) and m.dropout.p == P
        m.dropout = StatedMask(i)
    out = {"stream_names": np.array([n for n, _ in order]), "r": np.array(R), "scale": np.array(SCALE), "p": np.array(P),
           "seed": np.array(SEED, dtype=np.int64), "draw": np.array(DRAW, dtype=np.int64)}

    case, B, h, w, ts = G.TRAIN_CASES[0]
    fake = MG._FakeLDM(ns, wrapper=wrapper)
    fake.register_buffer = lambda name, val, persistent=True, _f=fake: setattr(_f, name, val)
    fake.v_posterior = 0.
    ns.ddpm.DDPM.register_schedule(fake, beta_schedule="linear", timesteps=1000, linear_start=0.00085, linear_end=0.0120)
    fake.loss_type, fake.learn_logvar, fake.logvar = "l2", False, torch.zeros(1000)
    fake.l_simple_weight, fake.original_elbo_weight, fake.training = 1., 0., True
    fake.q_sample = types.MethodType(ns.ddpm.DDPM.q_sample, fake)
    fake.get_loss = types.MethodType(ns.ddpm.DDPM.get_loss, fake)
    unet.train()
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
    # the noise floor: the oracle's fp32 and autocast16 gradients of the same loss on the dropout-free merged weights
    gt = np.load(os.path.join(ROOT, "tests", "golden", "train.npz"))
    x_in = torch.cat([torch.from_numpy(gt[case + ".x_noisy"]), c_concat], dim=1)
    o32 = _oracle_factor_grads(unet, "fp32", x_in, t, c_cross.detach(), noise)
    o16 = _oracle_factor_grads(unet, "autocast16", x_in, t, c_cross.detach(), noise)
    gnames, norms, norm_e = [], [], []
    blocks = full_blocks([n for n, _ in layers])
    for n, m in layers:
        for f in ("lora_down", "lora_up"):
            g = getattr(m, f).weight.grad
            k = f"{n}.{f}.weight"
            gnames.append(k)
            norms.append(float(g.double().norm()))
            n32 = o32[k].double().norm().item()
            norm_e.append(abs(o16[k].double().norm().item() - n32) / n32)
            if n.startswith(blocks):
                out["grad." + k] = g.numpy().astype(np.float32)
                out["emul." + k] = np.array(((o16[k].double() - o32[k].double()).norm() / o32[k].double().norm()).item())
    out["grad_names"], out["grad_norms"] = np.array(gnames), np.array(norms, dtype=np.float64)
    out["grad_norm_emul"] = np.array(norm_e, dtype=np.float64)
    out["full_blocks"] = np.array(blocks)
    np.savez_compressed(OUT, **out)
    print(f"lora dropout golden: loss {float(loss):.6f}, {len(layers)} layers, |d factor| in [{min(norms):.3e}, {max(norms):.3e}], "
          f"noise floor of the norms up to {max(norm_e):.3e}, {os.path.getsize(OUT) / 1e6:.2f} MB")


if __name__ == "__main__":
    sys.exit(main())
