"""CPU checks of prompt tuning through the text tower: the golden fixture written by tools/make_golden_prompt_tuning.py holds every key
tests/test_gpu_prompt_tuning.py reads, and the HIP backward of the prompt encoders stays opt-in."""
import os

import numpy as np

from oracle import golden_spec as G

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "prompt_tuning.npz")


def test_golden_has_every_key_the_gpu_tests_read():
    g = np.load(GOLDEN)
    keys = set(g.keys())
    for name, *_ in G.TEXT_CASES + G.MV_TEXT_CASES + G.NVS_TEXT_CASES:
        assert {f"{name}.z_shape", f"{name}.z_rows", f"{name}.d_special"} <= keys, name
    for name in ("txt_nvs_pose", "txt_nvs_pose2"):
        assert {f"{name}.d_rel_pos.mlp1.0.weight", f"{name}.d_rel_pos.mlp1.0.bias", f"{name}.d_rel_pos.mlp1.2.weight",
                f"{name}.d_rel_pos.mlp1.2.bias"} <= keys, name
    assert {"txt_nvs_pose2.d_rel_pos.mlp2.1.weight", "txt_nvs_pose2.d_rel_pos.mlp2.1.bias"} <= keys
    assert {"step.loss", "step.loss_simple", "step.loss_vlb", "step.d_special"} <= keys
    for name in ("mvloss_concat_v3", "mvloss_plain_v2"):
        assert {f"{name}.{k}" for k in ("loss", "loss_simple", "loss_vlb", "keys", "dctx_rows")} <= keys, name
        assert list(g[name + ".keys"]) == ["train/loss", "train/loss_simple", "train/loss_vlb"]
    assert os.path.getsize(GOLDEN) < 1 << 20


def test_golden_shapes():
    from tools import make_golden_prompt_tuning as MG
    g = np.load(GOLDEN)
    assert tuple(g["txt_deep.z_shape"]) == (2, 4, 77, 256)
    assert g["step.d_special"].shape == (8, 1024)
    for name, V, concat, b, h, w, ts in MG.MV_LOSS_CASES:
        n = b * (V - 1 if concat else V)
        assert g[name + ".dctx_rows"].shape == (n, len(G.NVS_Z_ROWS), 256)


def test_use_hip_backward_defaults_to_false():
    import leftrefill_amd.dropin as dropin
    dropin.install()
    from ldm.modules.encoders.Refill_modules import PromptCLIPEmbedder
    from ldm.modules.encoders.multiview_Refill_modules import PromptCLIPEmbedder as MV
    from ldm.modules.encoders.NVS_modules import NVSCLIPEmbedder
    assert PromptCLIPEmbedder.use_hip_backward is False
    assert MV.use_hip_backward is False and NVSCLIPEmbedder.use_hip_backward is False

