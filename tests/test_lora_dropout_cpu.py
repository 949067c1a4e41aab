"""CPU: LoRA dropout -- the host statement of the mask (leftrefill_amd/lora_dropout.py: Philox-4x32-10 known answers, threshold, keep
fraction, streams and draws), the new C-ABI symbols, and the wiring of the drop-in: stream ids in injection order, the module's CPU
forward against the explicit formula, the `lora_dropout` config key and the (seed, draw) pair in checkpoints."""
import importlib
import math
import os
import types

import numpy as np
import pytest
import torch

from leftrefill_amd import lora_dropout as D
from tests.test_lora_cpu import _lora, _nvs, _unet

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _hex(words):
    return " ".join(f"{int(w):08x}" for w in words)


def test_philox_known_answers():
    assert _hex(D.philox4x32_10((0, 0, 0, 0), (0, 0))) == "6627e8d5 e169c58d bc57ac4c 9b00dbd8"
    assert _hex(D.philox4x32_10((0xFFFFFFFF,) * 4, (0xFFFFFFFF,) * 2)) == "408f276d 41c83b0e a20bc7c6 6d5451fd"
    assert _hex(D.philox4x32_10((0x243F6A88, 0x85A308D3, 0x13198A2E, 0x03707344), (0xA4093822, 0x299F31D0))) == \
        "d16cfe09 94fdcceb 5001e420 24126ea1"
    # arrays broadcast: the same words as the scalar calls
    w = D.philox4x32_10((np.array([0, 0xFFFFFFFF]), np.array([0, 0xFFFFFFFF]), np.array([0, 0xFFFFFFFF]), np.array([0, 0xFFFFFFFF])),
                        (np.array([0, 0xFFFFFFFF]), np.array([0, 0xFFFFFFFF])))
    assert _hex(v[0] for v in w) == "6627e8d5 e169c58d bc57ac4c 9b00dbd8" and _hex(v[1] for v in w) == "408f276d 41c83b0e a20bc7c6 6d5451fd"


def test_threshold_and_inv_keep():
    assert D.threshold(0.1) == 429496729 and D.threshold(0.0) == 0 and D.threshold(0.5) == 2 ** 31
    assert D.threshold(1.0 - 2.0 ** -40) == 2 ** 32 - 1
    assert D.inv_keep(0.1) == float(np.float32(1.0 / 0.9)) and D.inv_keep(0.0) == 1.0
    assert D.inv_keep(0.1) == torch.tensor(1.0 / (1.0 - 0.1), dtype=torch.float64).float().item()
    for p in (-0.1, 1.0):
        with pytest.raises(ValueError, match="probability"):
            D.threshold(p)


def test_keep_is_the_stated_word_of_the_stated_counter():
    seed, stream, draw = (5 << 32) | 17, 3, 7
    m = D.keep_mask(seed, stream, draw, 6, 12, 0.1, row0=100)
    for row in (100, 105):
        for col in (0, 3, 4, 11):
            word = D.philox4x32_10((row, col >> 2, stream, draw), (17, 5))[col & 3]
            assert bool(m[row - 100, col]) == (int(word) >= 429496729)


def test_keep_fraction():
    m = D.keep_mask(1234, 3, 7, 154, 256, 0.1)
    assert m.shape == (154, 256) and int(m.sum()) == 35441
    for p, M, N in ((0.1, 154, 256), (0.5, 96, 320), (0.25, 77, 1280)):
        kept = D.keep_mask(99, 0, 0, M, N, p).mean()
        assert abs(kept - (1 - p)) <= 5 * math.sqrt(p * (1 - p) / (M * N)), (p, kept)
    assert D.keep_mask(1, 0, 0, 16, 16, 0.0).all()


def test_streams_draws_and_seeds_give_different_masks():
    base = D.keep_mask(1234, 3, 7, 154, 256, 0.1)
    for other in (D.keep_mask(1234, 4, 7, 154, 256, 0.1), D.keep_mask(1234, 3, 8, 154, 256, 0.1), D.keep_mask(1235, 3, 7, 154, 256, 0.1),
                  D.keep_mask(1234 + (1 << 32), 3, 7, 154, 256, 0.1)):
        # two independent masks at p = 0.1 disagree on 2 p (1 - p) = 18 % of the elements
        assert 0.15 < (other != base).mean() < 0.21
    assert np.array_equal(D.keep_mask(1234, 3, 7, 154, 256, 0.1), base)
    # a row offset is the same mask further down; the draw wraps at 32 bits
    assert np.array_equal(D.keep_mask(1234, 3, 7, 54, 256, 0.1, row0=100), base[100:])
    assert np.array_equal(D.keep_mask(1234, 3, 7 + 2 ** 32, 154, 256, 0.1), base)


def test_colgrp_of_the_geglu_permutation():
    from leftrefill_amd import packing
    H = 1280
    perm = packing.geglu_perm(H).numpy()
    tab = D.colgrp_of(perm)
    assert tab.dtype == np.int32 and tab.shape == (2 * H // 4,)
    assert np.array_equal(np.repeat(tab.astype(np.int64) * 4, 4) + np.tile(np.arange(4), tab.size), perm)
    assert np.array_equal(D.colgrp_of(np.arange(64)), np.arange(16))
    with pytest.raises(ValueError, match="groups of four"):
        D.colgrp_of(np.array([1, 2, 3, 4]))


def test_abi_declares_the_dropout_symbols():
    import ctypes
    import abi_helpers as abi
    from leftrefill_amd import _lib
    lib = ctypes.CDLL(_lib.LIB_PATH)
    for name in ("lr_lora_down_drop_f16", "lr_lora_up_drop_f16", "lr_lora_wgrad_drop_f16", "lr_lora_down_drop_bf16", "lr_lora_up_drop_bf16",
                 "lr_lora_wgrad_drop_bf16"):
        assert name in _lib.SIGNATURES and name in abi.header().protos, name
        assert hasattr(lib, name), name
    assert "lr_lora_drop" in abi.header().structs and _lib.ABI_VERSION == 30
    assert [f[0] for f in _lib.LoraDrop._fields_] == ["seed", "stream", "draw", "threshold", "inv_keep", "colgrp"]
    assert ctypes.sizeof(_lib.LoraDrop) == 32
    # the unmasked entries keep their signatures
    assert len(_lib.SIGNATURES["lr_lora_up_f16"]) == 11 and len(_lib.SIGNATURES["lr_lora_up_drop_f16"]) == 12


def test_stream_ids_equal_injection_order(golden):
    L = _lora()
    m = _unet()
    torch.manual_seed(4321)
    params, names = L.inject_trainable_lora(m, r=4, scale=1.0, dropout_p=0.1)
    by_name = dict(m.named_modules())
    order = [str(n)[:-len(".lora_up.weight")] for n in golden("lora")["param_order"] if str(n).endswith(".lora_up.weight")]
    assert len(order) == len(names)
    assert [by_name[n].drop_stream for n in order] == list(range(len(names)))
    assert [str(n) for n in golden("lora_dropout")["stream_names"]] == order          # the streams the reference's golden run used
    state = L.lora_dropout_state(m)
    assert state.seed == 4321 and state.draw == 0 and all(by_name[n].drop_state is state for n in order)
    assert all(by_name[n].dropout.p == 0.1 for n in order)
    assert not any("drop" in k for k in m.state_dict())
    # a layer built by hand has no stream
    lin = L.LoraInjectedLinear(64, 64, r=4, dropout_p=0.1)
    assert lin.drop_stream is None and not lin.dropout_live()


def test_module_cpu_forward_equals_the_explicit_formula():
    L = _lora()
    import torch.nn as nn
    torch.manual_seed(0)
    holder = nn.Module()
    holder.add_module("attn", type("CrossAttention", (nn.Module,), {})())
    holder.attn.to_q, holder.attn.to_k = nn.Linear(48, 40, bias=False), nn.Linear(48, 24, bias=True)
    L.inject_trainable_lora(holder, r=4, scale=0.5, dropout_p=0.25)
    state = L.lora_dropout_state(holder)
    state.seed, state.draw = 77, 5
    x = torch.randn(2, 7, 48)
    for stream, lin in enumerate((holder.attn.to_q, holder.attn.to_k)):
        assert lin.drop_stream == stream
        with torch.no_grad():
            lin.lora_up.weight.normal_()
        low = x @ lin.lora_down.weight.t() @ lin.lora_up.weight.t()
        keep = torch.from_numpy(D.keep_mask(77, stream, 5, 14, low.shape[-1], 0.25)).reshape(low.shape)
        want = lin.linear(x) + 0.5 * torch.where(keep, low * D.inv_keep(0.25), torch.zeros(()))
        got = lin.train()(x)
        assert torch.allclose(got, want, rtol=1e-5, atol=1e-6)
        assert (~keep).any() and torch.equal(got[~keep], lin.linear(x)[~keep])             # a dropped element is the base output, exactly
        assert torch.equal(lin.train()(x), got)                                              # the module's forward does not move the draw
        state.draw = 6
        assert not torch.equal(lin.train()(x), got)
        state.draw = 5
        # eval mode: no mask
        assert torch.allclose(lin.eval()(x), lin.linear(x) + 0.5 * low, rtol=1e-5, atol=1e-6)
    assert state.take() == 5 and state.draw == 6
    state.draw = 2 ** 32 - 1
    assert state.take() == 2 ** 32 - 1 and state.draw == 0


def test_set_lora_reads_the_lora_dropout_key():
    from inpainting_ldm.lora import LoraInjectedLinear
    m = _nvs({"do_lora": True, "lora_type": "default", "lora_rank": 4, "lora_scale": 1.0, "lora_dropout": 0.1})
    m.set_lora()
    layers = [s for s in m.model.diffusion_model.modules() if isinstance(s, LoraInjectedLinear)]
    assert layers and all(s.dropout.p == 0.1 and s.drop_stream == i for i, s in enumerate(layers))
    m = _nvs({"do_lora": True, "lora_type": "default", "lora_rank": 4, "lora_scale": 1.0})
    m.set_lora()
    assert all(s.dropout.p == 0.0 for s in m.model.diffusion_model.modules() if isinstance(s, LoraInjectedLinear))


def test_dropout_state_round_trips_through_a_checkpoint(tmp_path):
    from inpainting_ldm.lora import lora_dropout_state
    from leftrefill_amd.trainer import Trainer
    cfg = {"do_lora": True, "lora_type": "default", "lora_rank": 4, "lora_scale": 1.0, "lora_dropout": 0.1}
    m = _nvs(cfg)
    m.set_lora()
    state = lora_dropout_state(m.model.diffusion_model)
    state.seed, state.draw = (9 << 40) + 3, 41
    tr = Trainer(max_steps=1, default_root_dir=str(tmp_path), verbose=False)
    (tr.optimizer,), _ = m.configure_optimizers()
    tr.lr_schedulers = []
    path = tr.save_checkpoint(m)
    ckpt = torch.load(path, map_location="cpu", weights_only=False)
    assert ckpt["lora_dropout_state"] == {"seed": (9 << 40) + 3, "draw": 41}
    m2 = _nvs(cfg)
    m2.set_lora()
    (tr.optimizer,), _ = m2.configure_optimizers()
    tr._resume(m2, path)
    s2 = lora_dropout_state(m2.model.diffusion_model)
    assert (s2.seed, s2.draw) == ((9 << 40) + 3, 41)
    # a checkpoint without the key loads, and leaves the state as it is
    del ckpt["lora_dropout_state"]
    old = os.path.join(str(tmp_path), "old.ckpt")
    torch.save(ckpt, old)
    s2.draw = 7
    tr._resume(m2, old)
    assert (s2.seed, s2.draw) == ((9 << 40) + 3, 7)
    # a model without LoRA writes no key
    m3 = _nvs({"do_lora": False})
    m3.set_lora()
    c3 = {"state_dict": dict(m3.state_dict())}
    m3.on_save_checkpoint(c3)
    assert "lora_dropout_state" not in c3


def test_a_layer_without_a_stream_is_still_refused_and_p0_or_eval_is_unmasked():
    L = _lora()
    from leftrefill_amd import train_ops
    lin = L.LoraInjectedLinear(64, 64, r=4, dropout_p=0.1).train()
    with pytest.raises(NotImplementedError, match="not injected with a dropout stream"):
        train_ops.lora_dropout_live(lin)
    assert not train_ops.lora_dropout_live(lin.eval())
    assert not train_ops.lora_dropout_live(L.LoraInjectedLinear(64, 64, r=4, dropout_p=0.0).train())
    lin.drop_stream, lin.drop_state = 0, L.LoraDropoutState(seed=1)
    assert train_ops.lora_dropout_live(lin.train())
