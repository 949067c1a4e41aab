"""CPU: the LoRA drop-in (leftrefill_amd/dropin/inpainting_ldm/lora.py) against what the reference's own module produced
(tests/golden/lora.npz, tools/make_golden_lora.py): injected names, state-dict keys, parameter order, initialisation, the optimizer
group, the checkpoint filter, and the refusals of what is out of scope."""
import importlib
import itertools
import os
import types

import numpy as np
import pytest
import torch
import torch.nn as nn

from oracle import golden_spec as G

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _lora():
    import leftrefill_amd.dropin as dropin
    dropin.install()
    return importlib.import_module("inpainting_ldm.lora")


def _unet(name="MID"):
    import leftrefill_amd.dropin as dropin
    dropin.install()
    from ldm.modules.diffusionmodules.openaimodel import UNetModel
    return UNetModel(**G.CONFIGS[name].kwargs())


@pytest.fixture(scope="module")
def injected():
    L = _lora()
    m = _unet()
    params, names = L.inject_trainable_lora(m, r=4, scale=1.0)
    return L, m, params, names


def test_injected_names_count_and_state_dict_keys_equal_the_reference(golden, injected):
    L, m, params, names = injected
    g = golden("lora")
    assert names == [str(n) for n in g["names"]]
    assert sorted(m.state_dict().keys()) == [str(k) for k in g["keys"]]
    blocks = [b for b in m.modules() if b.__class__.__name__ == "BasicTransformerBlock"]
    layers = [n for n, mod in m.named_modules() if isinstance(mod, L.LoraInjectedLinear)]
    assert len(layers) == 9 * len(blocks) == len(names)
    per_block = sorted(n.split(".transformer_blocks.0.")[1] for n in layers if n.startswith("input_blocks.1.1."))
    assert per_block == sorted(["attn1.to_q", "attn1.to_k", "attn1.to_v", "attn1.to_out.0", "attn2.to_q", "attn2.to_k", "attn2.to_v",
                                "attn2.to_out.0", "ff.net.0.proj"])
    assert all(isinstance(b.ff.net[2], nn.Linear) for b in blocks)              # ff.net.2 sits below FeedForward, not GEGLU: not selected
    assert all(k in m.state_dict() for k in ("input_blocks.1.1.transformer_blocks.0.attn1.to_q.linear.weight",
                                             "input_blocks.1.1.transformer_blocks.0.attn1.to_q.lora_down.weight",
                                             "input_blocks.1.1.transformer_blocks.0.attn1.to_q.lora_up.weight"))


def test_parameter_order_is_up_then_down_per_layer(golden, injected):
    L, m, params, names = injected
    by_id = {id(p): n for n, p in m.named_parameters()}
    flat = list(itertools.chain(*[list(gen) for gen in params]))
    assert [by_id[id(p)] for p in flat] == [str(n) for n in golden("lora")["param_order"]]
    assert all(p.requires_grad and p.dtype == torch.float32 for p in flat)
    ups_downs = L.extract_lora_ups_down(m)
    assert len(ups_downs) == len(names) and ups_downs[0][0].weight is flat[0] and ups_downs[0][1].weight is flat[1]
    with pytest.raises(ValueError, match="No LoRA layer"):
        L.extract_lora_ups_down(_unet("SMALL"))


def test_initialisation_realize_and_cpu_forward():
    L = _lora()
    torch.manual_seed(0)
    lin = L.LoraInjectedLinear(1024, 640, bias=True, r=16, dropout_p=0.0, scale=0.5)
    assert not lin.lora_up.weight.any() and lin.lora_up.weight.shape == (640, 16) and lin.lora_down.weight.shape == (16, 1024)
    assert abs(lin.lora_down.weight.std().item() - 1 / 16) < 0.05 / 16
    assert isinstance(lin.selector, nn.Identity) and isinstance(lin.dropout, nn.Dropout) and lin.scale == 0.5 and lin.r == 16
    with torch.no_grad():
        lin.lora_up.weight.normal_()
    up, down = lin.realize_as_lora()
    assert torch.equal(up, lin.lora_up.weight * 0.5) and torch.equal(down, lin.lora_down.weight)
    x = torch.randn(3, 1024)
    want = x @ (lin.linear.weight + 0.5 * lin.lora_up.weight @ lin.lora_down.weight).t() + lin.linear.bias
    assert torch.allclose(lin.eval()(x), want, rtol=1e-4, atol=1e-4)


def test_injection_shares_the_base_parameters_and_marks_the_unet(injected):
    L, m, params, names = injected
    ref = _unet()
    assert m._lora_injected and m._weights_dirty
    q = m.input_blocks[1][1].transformer_blocks[0].attn1.to_q
    assert isinstance(q, L.LoraInjectedLinear) and q.linear.weight.shape == ref.input_blocks[1][1].transformer_blocks[0].attn1.to_q.weight.shape
    # the factors are no part of the packing signature: moving them re-packs nothing
    sig = m._sig()
    with torch.no_grad():
        q.lora_up.weight.add_(1.0)
    assert m._sig() == sig
    with torch.no_grad():
        q.linear.weight.add_(1.0)
    assert m._sig() != sig


def _nvs(lora, **optim):
    import leftrefill_amd.dropin as dropin
    dropin.install()
    from inpainting_ldm.NVS_ldm import NVSLDM
    cfg = G.CONFIGS["SMALL"]
    m = NVSLDM(first_stage_config={"target": "torch.nn.Identity"}, cond_stage_config={"target": "torch.nn.Identity"},
               unet_config={"target": "ldm.modules.diffusionmodules.openaimodel.UNetModel", "params": cfg.kwargs()},
               conditioning_key="hybrid", scale_factor=0.18215, linear_start=0.00085, linear_end=0.0120, timesteps=1000, channels=4,
               data_config={"img_size": 16, "cfg": 2.5}, save_prompt_only=True, lora=lora)
    enc = nn.Module()
    enc.special_embeddings = nn.Embedding(73, 8)
    enc.model = nn.Linear(2, 2)
    m.cond_stage_model = enc
    m.optim_cfg = dict({"learning_rate": 3e-5, "weight_decay": 0.01, "lr_scheduler": "cosine", "eta_min": 0.001, "lr_lora": 1e-4,
                        "wd_lora": 0.02}, **optim)
    m.trainer = types.SimpleNamespace(max_steps=8, precision=16, hip_graph=False)
    return m


def test_nvsldm_set_lora_and_the_optimizer_group():
    m = _nvs({"do_lora": False})
    m.set_lora()
    assert m.unet_lora_params is None and not any("lora" in k for k in m.state_dict())
    (opt,), _ = m.configure_optimizers()
    assert len(opt.param_groups) == 1

    m = _nvs({"do_lora": True, "lora_type": "default", "lora_rank": 4, "lora_scale": 1.0})
    assert not any("lora" in k for k in m.state_dict())       # nothing is injected before set_lora()
    m.set_lora()
    factors = [p for n, p in m.model.diffusion_model.named_parameters() if "lora_" in n]
    assert len(m.unet_lora_params) == len(factors) > 0
    (opt,), _ = m.configure_optimizers()
    assert len(opt.param_groups) == 2
    g1 = opt.param_groups[1]
    assert g1["lr"] == 1e-4 and g1["weight_decay"] == 0.02 and opt.param_groups[0]["lr"] == 3e-5
    assert [id(p) for p in g1["params"]] == [id(p) for gen_owner in _pairs(m) for p in gen_owner]

    # on_save_checkpoint(save_prompt_only) keeps exactly the factor keys of the UNet (next to the prompt tokens)
    sd = m.state_dict()
    ckpt = {"state_dict": {k: 0 for k in sd}}
    m.on_save_checkpoint(ckpt)
    kept_unet = sorted(k for k in ckpt["state_dict"] if k.startswith("model.diffusion_model."))
    assert kept_unet == sorted(k for k in sd if k.startswith("model.diffusion_model.") and (".lora_down." in k or ".lora_up." in k))
    assert len(kept_unet) == len(factors) and "cond_stage_model.special_embeddings.weight" in ckpt["state_dict"]

    m.trainer.hip_graph = True
    with pytest.raises(NotImplementedError, match="hip_graph"):
        m.configure_optimizers()


def _pairs(m):
    from inpainting_ldm.lora import LoraInjectedLinear
    for mod in m.model.diffusion_model.modules():
        if isinstance(mod, LoraInjectedLinear):
            yield [mod.lora_up.weight]
            yield [mod.lora_down.weight]


def test_out_of_scope_cases_raise():
    L = _lora()
    m = _nvs({"do_lora": True, "lora_type": "extended", "lora_rank": 4, "lora_scale": 1.0})
    with pytest.raises(NotImplementedError, match="dropout_p = 0.1"):
        m.set_lora()
    with pytest.raises(NotImplementedError, match="Not implemented LoRA"):
        m.lora_cfg["lora_type"] = "simple"
        m.set_lora()
    m = _nvs({"do_lora": False}, all_trainable=True)
    with pytest.raises(NotImplementedError, match="weight gradients"):
        m.configure_optimizers()
    m = _nvs({"do_lora": False})
    m.unet_lora_params = [[nn.Parameter(torch.zeros(1))]]      # a "LoRA group" of parameters that no injected layer owns
    with pytest.raises(NotImplementedError, match="weight gradients"):
        m.configure_optimizers()
    with pytest.raises(NotImplementedError, match="LoraInjectedConv2d"):
        L.LoraInjectedConv2d(4, 4, 3)
    lin = L.LoraInjectedLinear(64, 64, r=4, dropout_p=0.0)
    with pytest.raises(NotImplementedError, match="selector"):
        lin.set_selector_from_diag(torch.ones(4))
    with pytest.raises(NotImplementedError, match="text tower"):
        L.inject_trainable_lora(nn.Linear(4, 4), L.TEXT_ENCODER_DEFAULT_TARGET_REPLACE, r=4)
    for r in (65, 128):
        with pytest.raises(ValueError, match="rank"):
            L.LoraInjectedLinear(1024, 1024, r=r)
    with pytest.raises(ValueError, match="rank"):
        L.LoraInjectedLinear(8, 8, r=16)
    # the multi-view UNet
    from ldm.modules.diffusionmodules.multiview_unet import MultiViewUnetModel
    mv = MultiViewUnetModel(**G.mv_config(2, False).kwargs())
    with pytest.raises(NotImplementedError, match="multi-view"):
        L.inject_trainable_lora(mv, r=4)
    assert not any("lora" in k for k in mv.state_dict())      # refused before anything is swapped
    # dropout in training mode: refused where the layer would run
    from leftrefill_amd import train_ops
    lin = L.LoraInjectedLinear(64, 64, r=4, dropout_p=0.1).train()
    with pytest.raises(NotImplementedError, match="dropout"):
        train_ops.lora_linear(torch.zeros(8, 64), torch.zeros(64, 64), None, [(lin, 0, 64, None)])


def test_abi_declares_the_lora_symbols():
    import abi_helpers as abi
    from leftrefill_amd import _lib
    for name in ("lr_lora_down_f16", "lr_lora_up_f16", "lr_lora_wgrad_f16", "lr_lora_down_bf16", "lr_lora_up_bf16", "lr_lora_wgrad_bf16",
                 "lr_lora_merge_f32", "lr_lora_wgrad_workspace_bytes"):
        assert name in _lib.SIGNATURES and name in abi.header().protos, name
    assert _lib.ABI_VERSION == 30


def test_merged_plan_carries_nothing_of_an_earlier_merge():
    """UNetModel._merged_plan: the merged twin shares the listed records with the unmerged plan, swaps the SpatialTransformers' records
    and holds neither the previous merged plan nor the training route's entries -- re-merging after every training forward piles nothing up."""
    import leftrefill_amd.dropin as dropin
    dropin.install()
    from ldm.modules.diffusionmodules.openaimodel import UNetModel

    class Rec:                                       # stands for a PackedST (weak-referenceable)
        def __init__(self):
            self.blocks = [types.SimpleNamespace(kv_slot=None)]

    st = Rec

    a, b, res = st(), st(), object()
    base = {k: object() for k in UNetModel.MERGED_SHARED}
    base.update(input=[[("res", res), ("st", a)]], middle=[("st", b)], output=[[("res", res)]], tblocks=a.blocks + b.blocks,
                kv_all_w=object(), merged_stale=True)
    base["root"] = base
    plans = []
    for _ in range(3):
        mp = UNetModel._merged_plan(base, {id(a): st(), id(b): st()})
        base["merged"], base["merged_stale"] = mp, False
        plans.append(mp)
        assert set(mp) == set(UNetModel.MERGED_SHARED) | {"input", "middle", "output", "tblocks"}
        assert not {"merged", "merged_stale", "kv_all_w"} & set(mp) and mp["root"] is base
        assert all(mp[k] is base[k] for k in UNetModel.MERGED_SHARED)
        assert mp["input"][0][0][1] is res and mp["output"][0][0][1] is res                  # ResBlock / conv records: the same objects
        assert mp["input"][0][1][1] is not a and mp["middle"][0][1] is not b
        assert [pt.kv_slot for pt in mp["tblocks"]] == [0, 1] and mp["tblocks"][0] is mp["input"][0][1][1].blocks[0]
    import gc
    import weakref
    first = weakref.ref(plans[0]["middle"][0][1])
    del plans, mp
    gc.collect()
    assert first() is None                                                                   # the first merge's records are gone
