"""Host side of the training driver (no GPU): the C ABI of lr_amp_adamw_step, the lr table, the task models' optimizer groups and
checkpoint filters against tests/golden/optim.npz (tools/make_golden_optim.py), and the trainer's checkpoint layout."""
import ctypes
import importlib
import json
import os
import types

import numpy as np
import pytest
import torch

from conftest import GOLDEN, ROOT
from oracle import golden_spec as G


def _gold():
    return np.load(os.path.join(GOLDEN, "optim.npz"))


def _json(gold, key):
    return json.loads(bytes(gold[key]).decode())


# ---- 1. the C ABI --------------------------------------------------------------------------------------------------------------------
def test_symbol_declared_bound_and_exported_under_abi_30():
    from leftrefill_amd import _lib, ops
    assert _lib.ABI_VERSION == 30
    import abi_helpers as abi
    args = abi.c_params("lr_amp_adamw_step")
    assert len(args) == 12       # header against binding: tests/test_abi_cpu.py; this entry's exact ctypes kinds stay here
    for a, ct in zip(args, _lib.SIGNATURES["lr_amp_adamw_step"]):
        if "*" in a or a.startswith("lr_stream_t"):
            assert ct in (ctypes.c_void_p, ctypes.POINTER(ctypes.c_int)), a
        else:
            assert ct is (ctypes.c_float if a.startswith("float") else ctypes.c_int), a
    lib = _lib.load()
    assert hasattr(lib, "lr_amp_adamw_step") and lib.lr_abi_version() == 30
    # the structs and constants the binding restates
    for name, val in (("LR_OPT_MAX_GROUPS", ops.OPT_MAX_GROUPS), ("LR_OPT_MAX_BLOCKS", ops.OPT_MAX_BLOCKS), ("LR_OPT_CONSTS", ops.OPT_CONSTS)):
        assert abi.define(name) == val
    assert ops.OPT_STATE_WORDS == ops.OPT_CONSTS + 4 * ops.OPT_MAX_GROUPS
    for i, n in enumerate(ops.OPT_STATE_FIELDS):
        word = {"scale": "SCALE", "sched_steps": "SCHED_STEPS", "applied_steps": "APPLIED_STEPS"}.get(n, n.upper())
        assert abi.define(f"LR_OPT_{word}") == i, n
    assert ctypes.sizeof(_lib.OptimTensor) == 48 and ctypes.sizeof(_lib.OptimGroup) == 48
    assert "optim.hip" in importlib.import_module("leftrefill_amd.build").SOURCES


def test_bad_arguments_are_refused_before_any_launch():
    from leftrefill_amd import _lib
    lib = _lib.load()
    n = ctypes.c_int(0)
    assert lib.lr_amp_adamw_step(0, 1, 0, 1, 0, 0, 1, 2.0, 0.5, 2000, ctypes.byref(n), 0) == -1
    assert lib.lr_amp_adamw_step(16, 1, 16, 9, 16, 16, 1, 2.0, 0.5, 2000, ctypes.byref(n), 0) == -1      # too many groups
    assert lib.lr_amp_adamw_step(16, 1, 16, 1, 16, 16, 2000, 2.0, 0.5, 2000, ctypes.byref(n), 0) == -1   # too many blocks
    assert lib.lr_amp_adamw_step(16, 1, 16, 1, 16, 16, 1, 0.5, 0.5, 2000, ctypes.byref(n), 0) == -1      # growth factor <= 1
    assert lib.lr_amp_adamw_step(16, 1, 16, 1, 16, 8, 1, 2.0, 0.5, 2000, ctypes.byref(n), 0) == -2       # misaligned partials
    assert n.value == 0


# ---- 2. the lr table -----------------------------------------------------------------------------------------------------------------
def _golden_optimizer(gold, device="cpu"):
    from leftrefill_amd.optim import AmpAdamW, cosine_schedule
    meta = _json(gold, "meta")
    ps = [torch.nn.Parameter(torch.from_numpy(gold["p0.%d" % i]).clone().to(device)) for i in range(len(meta["shapes"]))]
    groups = [dict(params=[p for p, gi in zip(ps, meta["group_of"]) if gi == k], **meta["groups"][k]) for k in range(len(meta["groups"]))]
    opt = AmpAdamW(groups, lr=meta["groups"][0]["lr"], growth_interval=meta["growth_interval"])
    opt.set_schedule(cosine_schedule(opt, meta["max_steps"], meta["eta_min"] * meta["groups"][0]["lr"]))
    return opt, ps, meta


def test_lr_table_is_bit_equal_to_the_fp32_cast_of_torchs_schedule():
    gold = _gold()
    opt, _, meta = _golden_optimizer(gold)
    want = gold["schedule"].astype(np.float32).T            # [groups][steps]
    got = opt.lr_table().cpu().numpy()
    assert got.dtype == np.float32 and got.shape == want.shape == (2, meta["max_steps"] + 1)
    assert got.tobytes() == want.tobytes()
    assert [g["lr"] for g in opt.param_groups] == list(gold["schedule"][0])      # host mirror: step 0, in float64
    opt.advance_host(3)
    assert [g["lr"] for g in opt.param_groups] == list(gold["schedule"][3])
    opt.advance_host(100)                                                          # past the end: the last entry holds
    assert [g["lr"] for g in opt.param_groups] == list(gold["schedule"][-1])


def test_optimizer_state_dict_round_trip_on_the_host():
    gold = _gold()
    opt, ps, _ = _golden_optimizer(gold)
    opt.advance_host(2)
    d = opt.state_dict()
    assert d["amp"]["scale"] == 65536.0 and d["amp"]["growth_interval"] == 3 and len(d["param_groups"]) == 2
    d["amp"]["scale"], d["amp"]["sched_steps"], d["amp"]["growth_tracker"] = 1024.0, 5, 2
    opt2, _, _ = _golden_optimizer(gold)
    opt2.load_state_dict(d)
    s = opt2.amp_state()
    assert (s["scale"], s["sched_steps"], s["growth_tracker"]) == (1024.0, 5, 2)
    assert opt2.param_groups[0]["lr"] == gold["schedule"][5][0]
    assert opt2.scaler_state_dict() == {"scale": 1024.0, "growth_factor": 2.0, "backoff_factor": 0.5, "growth_interval": 3, "_growth_tracker": 2}


# ---- 3. the task models ----------------------------------------------------------------------------------------------------------------
def _task_model(module, cls, **extra):
    import leftrefill_amd.dropin as dropin
    dropin.install()
    cfg = G.CONFIGS["SMALL"]
    m = getattr(importlib.import_module("inpainting_ldm." + module), cls)(
        first_stage_config={"target": "torch.nn.Identity"}, cond_stage_config={"target": "torch.nn.Identity"},
        unet_config={"target": "ldm.modules.diffusionmodules.openaimodel.UNetModel", "params": cfg.kwargs()},
        conditioning_key="hybrid", scale_factor=0.18215, linear_start=0.00085, linear_end=0.0120, timesteps=1000, channels=4,
        data_config={"img_size": 16, "cfg": 2.5}, save_prompt_only=True, **extra)
    enc = torch.nn.Module()                                  # the prompt encoder's parameter families, small
    enc.special_embeddings = torch.nn.Embedding(73, 8)
    enc.model = torch.nn.Linear(2, 2)                        # stands for the frozen CLIP tower
    m.cond_stage_model = enc
    m.optim_cfg = {"learning_rate": 3e-5, "weight_decay": 0.01, "lr_scheduler": "cosine", "eta_min": 0.001}
    m.trainer = types.SimpleNamespace(max_steps=8, precision=16)
    return m


def _nvs_pose_refine():
    m = _task_model("NVS_ldm", "NVSLDM", refinement_config={"use_input_refinement": True})
    m.cond_stage_model.rel_pos_model = torch.nn.Sequential(torch.nn.Linear(4, 8), torch.nn.Linear(8, 8))
    m.refinement_model = torch.nn.Sequential(torch.nn.Conv2d(4, 8, 3))      # same families as the golden's host
    return m


CASES = [("single", lambda: _task_model("ref_inpainting_ldm", "RefInpaintLDM")),
         ("multiview", lambda: _task_model("multiview_ref_inpainting_ldm", "RefInpaintLDM", view_num=3)),
         ("nvs_plain", lambda: _task_model("NVS_ldm", "NVSLDM")), ("nvs_pose_refine", _nvs_pose_refine)]


@pytest.mark.parametrize("name,make", CASES, ids=[c[0] for c in CASES])
def test_configure_optimizers_groups_match_the_reference(name, make):
    from leftrefill_amd.optim import AmpAdamW, TableSchedule
    names = _json(_gold(), "names")
    m = make()
    opts, sches = m.configure_optimizers()
    opt = opts[0]
    assert isinstance(opt, AmpAdamW) and isinstance(sches[0]["scheduler"], TableSchedule)
    assert (sches[0]["interval"], sches[0]["frequency"]) == ("step", 1)
    by_id = {id(p): n for n, p in m.named_parameters()}
    assert [sorted(by_id[id(p)] for p in g["params"]) for g in opt.param_groups] == names["groups"][name]
    assert all(g["weight_decay"] == 0.01 for g in opt.param_groups) and opt.param_groups[0]["lr"] == 3e-5
    # the schedule is torch's CosineAnnealingLR(opt, max_steps, eta_min = eta_min * lr)
    ref = torch.optim.AdamW([torch.nn.Parameter(torch.zeros(1))], lr=3e-5)
    sche = torch.optim.lr_scheduler.CosineAnnealingLR(ref, 8, eta_min=0.001 * 3e-5)
    want = [3e-5]
    for _ in range(8):
        ref.step()
        sche.step()
        want.append(ref.param_groups[0]["lr"])
    assert opt.lr_table().cpu().numpy().tobytes() == np.asarray([want], dtype=np.float64).astype(np.float32).tobytes()


def test_unknown_scheduler_prints_the_message_and_returns_the_bare_optimizer(capsys):
    from leftrefill_amd.optim import AmpAdamW
    m = _task_model("ref_inpainting_ldm", "RefInpaintLDM")
    m.optim_cfg["lr_scheduler"] = "none"
    opt = m.configure_optimizers()
    assert isinstance(opt, AmpAdamW)
    assert "Unknown scheduler none" in capsys.readouterr().out
    m.trainer.precision = "bf16"                      # no scaler dynamics outside fp16
    opt = m.configure_optimizers()
    assert opt.growth_interval == 0 and opt.amp_state()["scale"] == 1.0


def test_all_trainable_and_lora_groups_refuse():
    m = _task_model("NVS_ldm", "NVSLDM")
    m.optim_cfg["all_trainable"] = True
    with pytest.raises(NotImplementedError, match="weight gradients"):
        m.configure_optimizers()
    m.optim_cfg["all_trainable"] = False
    m.unet_lora_params = [[torch.nn.Parameter(torch.zeros(1))]]
    with pytest.raises(NotImplementedError, match="weight gradients"):
        m.configure_optimizers()


@pytest.mark.parametrize("name,make", [("single", CASES[0][1]), ("multiview", CASES[1][1]), ("nvs", CASES[2][1])], ids=["single", "multiview", "nvs"])
def test_on_save_checkpoint_keeps_the_reference_keys(name, make):
    names = _json(_gold(), "names")
    m = make()
    ckpt = {"state_dict": {k: 0 for k in names["key_universe"]}}
    m.on_save_checkpoint(ckpt)
    assert sorted(ckpt["state_dict"]) == names["survivors"][name]
    m.save_prompt_only = False
    ckpt = {"state_dict": {k: 0 for k in names["key_universe"]}}
    m.on_save_checkpoint(ckpt)
    assert len(ckpt["state_dict"]) == len(names["key_universe"])


def test_training_step_and_hooks_exist_on_all_three_models():
    for _, make in CASES[:3]:
        m = make()
        for hook in ("shared_step", "training_step", "configure_optimizers", "on_save_checkpoint", "on_train_batch_end"):
            assert callable(getattr(m, hook)), hook
        assert m.global_step == 0 and m.local_rank == 0 and m.ucg_training == {}


# ---- 4. the trainer's checkpoint ---------------------------------------------------------------------------------------------------------
def test_trainer_checkpoint_round_trips_and_loads_through_the_dropin_loader(tmp_path):
    from leftrefill_amd.trainer import Trainer
    names = _json(_gold(), "names")
    m = _task_model("ref_inpainting_ldm", "RefInpaintLDM")
    tr = Trainer(max_steps=8, precision=16, default_root_dir=str(tmp_path), growth_interval=3, verbose=False)
    tr._setup(m)
    m.log("val/psnr", 30.0, sync_dist=True)                      # the trainer serves Lightning's logging calls
    m.log_dict({"train/loss": 1.0})
    assert tr.logged == {"val/psnr": 30.0, "train/loss": 1.0}
    tr.global_step, tr.current_epoch = 5, 1
    assert [n for n, p in m.named_parameters() if p.requires_grad] == ["cond_stage_model.special_embeddings.weight"]
    path = tr.save_checkpoint(m)
    assert path == os.path.join(str(tmp_path), "ckpts", "last.ckpt")
    ck = torch.load(path, map_location="cpu", weights_only=False)
    assert sorted(ck) == names["shipped_ckpt"]["top_level"]                       # Lightning 1.5's layout, as the shipped file
    assert sorted(ck["native_amp_scaling_state"]) == names["shipped_ckpt"]["scaler_keys"]
    assert list(ck["state_dict"]) == list(names["shipped_ckpt"]["state_dict"]) == ["cond_stage_model.special_embeddings.weight"]
    assert (ck["global_step"], ck["epoch"], ck["native_amp_scaling_state"]["growth_interval"]) == (5, 1, 3)
    import leftrefill_amd.dropin as dropin
    dropin.install()
    from inpainting_ldm.model import load_state_dict
    sd = load_state_dict(path, location="cpu")
    assert torch.equal(sd["cond_stage_model.special_embeddings.weight"], m.cond_stage_model.special_embeddings.weight.detach())
    # a fresh model and trainer resume from it
    m2 = _task_model("ref_inpainting_ldm", "RefInpaintLDM")
    tr2 = Trainer(max_steps=8, precision=16, resume_from_checkpoint=path, growth_interval=3, verbose=False)
    tr2._setup(m2)
    assert (tr2.global_step, tr2.current_epoch) == (5, 1)
    assert torch.equal(m2.cond_stage_model.special_embeddings.weight, m.cond_stage_model.special_embeddings.weight)
    assert tr2.optimizer.state_dict()["amp"] == tr.optimizer.state_dict()["amp"]
