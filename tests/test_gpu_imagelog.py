"""The training image logger on the GPU: lr_image_grid byte for byte against its numpy statement (leftrefill_amd/imagelog.py),
lr_token_drift, the two routes of the drop-in InpaintingLogger, Trainer.fit with the logger as a callback (eager and hipGraph), and the
training CLI with `logger_freq` / `save_top_k`.

Shapes are the smallest at which the grid kernel can go wrong: H = 5, sources of W = 7 and W = 16 in one call (3 Wc is no multiple of 4:
ragged row ends, dwords that span sources and rows, unaligned column offsets), C = 1 and 3 mixed, an NHWC-strided view, an NCHW tensor and
a slice of a larger batch, one image (unpadded) and three (padded)."""
import ctypes
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from oracle import golden_spec as G

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
H = 5


def _pool():
    """fp32(k / 127.5 - 1) and both neighbours (the truncation steps), -1, 1, and values outside [-1, 1]."""
    x = (np.arange(256) / 127.5 - 1).astype(np.float32)
    xs = np.unique(np.concatenate([x, np.nextafter(x, np.float32(2)), np.nextafter(x, np.float32(-2))]))
    return np.concatenate([xs, np.float32([-1.0, 1.0, -1.5, 1.25, 3.0, -7.0, 1.0000001, -1.0000001])])


def _fill(shape, seed, lo=None):
    pool = _pool() if lo is None else np.clip(_pool(), lo, 1.0)
    idx = np.random.RandomState(seed).randint(0, len(pool), size=int(np.prod(shape)))
    return torch.from_numpy(pool[idx].reshape(shape))


def _sources(N, dtype, lo=None):
    """NHWC-strided view (W 7, C 3), NCHW (W 16, C 1), rows 1 .. N of a larger NCHW batch (W 16, C 3: a storage offset)."""
    a = _fill((N, H, 7, 3), 1, lo).to(DEV, dtype).permute(0, 3, 1, 2)
    b = _fill((N, 1, H, 16), 2, lo).to(DEV, dtype)
    c = _fill((N + 2, 3, H, 16), 3, lo).to(DEV, dtype)[1:1 + N]
    assert not a.is_contiguous() and a.stride(1) == 1 and c.storage_offset() > 0
    return [a, b, c]


def _want(sources, N, **kw):
    from leftrefill_amd.imagelog import KEYS, grid_numpy
    assert len(sources) <= len(KEYS)
    return grid_numpy({k: s.float().cpu().numpy() for k, s in zip(KEYS, sources)}, max_images=N, **kw)


@pytest.mark.parametrize("dtype", [torch.float32, torch.float16, torch.bfloat16], ids=["fp32", "fp16", "bf16"])
@pytest.mark.parametrize("N", [1, 3])
def test_image_grid_matches_numpy_byte_for_byte(N, dtype):
    from leftrefill_amd import ops
    src = _sources(N, dtype)
    want = _want(src, N)
    assert want.shape == ((H if N == 1 else N * (H + 2) + 2), 39 if N == 1 else 51, 3) and (3 * want.shape[1]) % 4
    got = ops.image_grid(src, N, H)
    assert got.dtype == torch.uint8 and np.array_equal(got.cpu().numpy(), want)
    assert torch.equal(got, ops.image_grid(src, N, H))      # bitwise reproducible
    # no rescale, no clamp, on values in [0, 1]
    src01 = _sources(N, dtype, lo=0.0)
    got01 = ops.image_grid(src01, N, H, clamp=False, rescale=False)
    assert np.array_equal(got01.cpu().numpy(), _want(src01, N, clamp=False, rescale=False))
    # a canvas at every byte alignment: the ragged head and tail are byte stores, and nothing outside the canvas is touched
    n = want.size
    for off in (1, 2, 3):
        buf = torch.full((n + 8,), 0xA5, device=DEV, dtype=torch.uint8)
        ops.image_grid(src, N, H, out=buf[off:off + n].view(*want.shape))
        host = buf.cpu().numpy()
        assert np.array_equal(host[off:off + n].reshape(want.shape), want), off
        assert (host[:off] == 0xA5).all() and (host[off + n:] == 0xA5).all(), off


@pytest.mark.parametrize("N", [1, 3])
def test_image_grid_one_source_and_eight(N):
    from leftrefill_amd import ops
    from leftrefill_amd.imagelog import make_grid_numpy, to_uint8
    one = _sources(N, torch.float32)[:1]
    assert np.array_equal(ops.image_grid(one, N, H).cpu().numpy(), _want(one, N))
    eight = [_fill((N, 1 + 2 * (i % 2), H, 3 + i), 10 + i).to(DEV, (torch.float32, torch.float16, torch.bfloat16)[i % 3]) for i in range(8)]
    want = np.concatenate([to_uint8(make_grid_numpy(np.clip(s.float().cpu().numpy(), -1, 1))).transpose(1, 2, 0) for s in eight], axis=1)
    assert np.array_equal(ops.image_grid(eight, N, H).cpu().numpy(), want)
    with pytest.raises(RuntimeError, match="bad argument"):
        ops.image_grid(eight + one, N, H)


def test_image_grid_refuses_before_any_launch():
    from leftrefill_amd import _lib
    lib = _lib.load()
    N = 3
    t = torch.zeros(N, 3, H, 7, device=DEV)
    out = torch.full((N * (H + 2) + 2, 9 * 11, 3), 0x5A, device=DEV, dtype=torch.uint8)
    st = torch.cuda.current_stream().cuda_stream

    def call(n_sources, edit=lambda arr: None, N=N, Wc=out.shape[1]):
        arr = (_lib.GridSource * 9)()
        for i, a in enumerate(arr):
            a.ptr, a.kind, a.C, a.W, a.col = t.data_ptr(), 0, 3, 7, 11 * i
            a.stride_n, a.stride_c, a.stride_h, a.stride_w = t.stride()
        edit(arr)
        return lib.lr_image_grid(arr, n_sources, N, H, 1, 1, out.data_ptr(), Wc, st)

    assert call(9) == -1                                                     # a ninth source
    assert call(2, lambda a: setattr(a[1], "C", 2)) == -1                    # C outside {1, 3}
    assert call(2, lambda a: setattr(a[1], "col", 10)) == -1                 # overlaps source 0's columns 0 .. 10
    assert call(2, lambda a: setattr(a[1], "col", 9 * 11 - 10)) == -1        # leaves the canvas
    assert call(2, lambda a: setattr(a[1], "col", -1)) == -1
    assert call(2, lambda a: setattr(a[0], "kind", 3)) == -1
    assert call(0) == -1 and call(1, N=0) == -1
    torch.cuda.synchronize()
    assert (out == 0x5A).all()                                               # untouched
    assert call(8) == 0                                                      # and the same table is served when it is valid
    torch.cuda.synchronize()
    assert (out[:, :88] != 0x5A).all() and (out[:, 88:] == 127).all()        # columns no source owns are padding


@pytest.mark.parametrize("D", [5, 1024])
def test_token_drift(D):
    from leftrefill_amd import ops
    from leftrefill_amd.imagelog import token_drift_numpy
    T = 3
    g = torch.Generator().manual_seed(D)
    old = torch.randn(T, D, generator=g)
    new = old + 0.01 * torch.randn(T, D, generator=g)
    new[1] = old[1]                                                          # a token that did not move
    want = token_drift_numpy(old.numpy(), new.numpy())
    o, n = old.to(DEV), new.to(DEV)
    out = ops.token_drift(o, n)
    assert torch.equal(o, n) and torch.equal(n.cpu(), new)                   # the snapshot is refreshed bit for bit, the tokens untouched
    got = out.cpu().numpy().astype(np.float64)
    rel = np.abs(got - want) / np.maximum(want, 1e-300)
    print(f"D = {D}: drift {got}, relative error {rel}, bound {D * 2.0 ** -24:.3e}")
    assert got[1] == 0.0 and want[1] == 0.0
    assert (rel[[0, 2]] <= D * 2.0 ** -24).all()
    assert float(ops.token_drift(o, n)[0]) == 0.0                            # second look: nothing moved since


# ---- the logger's two routes ---------------------------------------------------------------------------------------------------------------
def _logger(**kw):
    import leftrefill_amd.dropin as dropin
    dropin.install()
    from inpainting_ldm.logger import InpaintingLogger
    return InpaintingLogger(**kw)


def test_logger_device_and_host_routes_write_the_same_file(tmp_path):
    images = {"pred": _fill((5, 3, H, 16), 21).to(DEV), "masked_image": _fill((5, H, 16, 3), 22).to(DEV).permute(0, 3, 1, 2),
              "origin_image": _fill((5, 3, H, 16), 23).to(DEV).half(), "reference": _fill((5, 2, 3, H, 7), 24).to(DEV)}
    files = {}
    for route, device in (("device", True), ("host", False)):
        lg = _logger(max_images=3, save_dir=route, device=device)
        canvas = lg.canvas(dict(images))
        assert (lg._canvas is not None) == device
        lg.log_local(str(tmp_path), "train", dict(images), 3, 0, 4)
        files[route] = (canvas, (tmp_path / route / "train" / "gs-000003_e-000000_b-000004.jpg").read_bytes())
    assert files["device"][0].shape == (3 * (H + 2) + 2, 3 * 20 + 2 * 11, 3)
    assert np.array_equal(files["device"][0], files["host"][0]) and files["device"][1] == files["host"][1]


# ---- Trainer.fit with the logger as a callback -------------------------------------------------------------------------------------------------
B, h, w, CTX = 2, 8, 16, 77


class _Encoder(torch.nn.Module):
    def __init__(self, dim):
        super().__init__()
        self.special_embeddings = torch.nn.Embedding(50, dim)
        self.special_tokens = [f"<t{i}>" for i in range(50)]
        self.model = torch.nn.Linear(4, 4)
        torch.nn.init.normal_(self.special_embeddings.weight, std=0.02)


def _model():
    """The tiny model of tests/test_gpu_trainer.py, restated, with what `log_images` needs from a model without VAE and tokenizer: the
    empty-prompt context is the fixed context without the learned tokens, and a latent's first three channels are its "image"."""
    import leftrefill_amd.dropin as dropin
    dropin.install()
    from inpainting_ldm.ref_inpainting_ldm import RefInpaintLDM

    class Tiny(RefInpaintLDM):
        def get_input(self, batch, k, **kw):
            enc = self.cond_stage_model
            ctx = torch.cat([batch["ctx"][:, :1], batch["ctx"][:, 1:51] + enc.special_embeddings.weight, batch["ctx"][:, 51:]], dim=1)
            self._uc = batch["ctx"]
            return batch["x"], {"c_concat": [batch["c_concat"]], "c_crossattn": [ctx]}

        def get_unconditional_conditioning(self, N):
            return self._uc[:N]

        def decode_first_stage(self, z, **kw):
            return z[:, :3].float()

        def shared_step(self, batch, **kw):
            x, c = self.get_input(batch, self.first_stage_key)
            return self.p_losses(x, c, batch["t"], noise=batch["noise"])

    cfg = G.CONFIGS["MID"]
    torch.manual_seed(0)
    m = Tiny(first_stage_config={"target": "torch.nn.Identity"}, cond_stage_config={"target": "torch.nn.Identity"},
             unet_config={"target": "ldm.modules.diffusionmodules.openaimodel.UNetModel", "params": cfg.kwargs()},
             conditioning_key="hybrid", scale_factor=0.18215, linear_start=0.00085, linear_end=0.0120, timesteps=1000, channels=4,
             data_config={"img_size": 16, "cfg": 2.5}, save_prompt_only=True)
    m.model.diffusion_model.load_state_dict(G.unet_state("MID"), strict=True)
    m.cond_stage_model = _Encoder(cfg.context_dim)
    m.optim_cfg = {"learning_rate": 1e-3, "weight_decay": 0.01, "lr_scheduler": "cosine", "eta_min": 0.01}
    return m.to(DEV), cfg


def _batches(cfg, n):
    g = torch.Generator().manual_seed(5)
    out = []
    for _ in range(n):
        b = {"x": torch.randn(B, 4, h, w, generator=g), "c_concat": torch.randn(B, 5, h, w, generator=g),
             "ctx": torch.randn(B, CTX, cfg.context_dim, generator=g), "t": torch.randint(0, 1000, (B,), generator=g),
             "noise": torch.randn(B, 4, h, w, generator=g), "image": torch.rand(B, h, w, 3, generator=g) * 2 - 1}
        b["masked_image"] = b["image"] * (torch.rand(B, h, w, 1, generator=g) < 0.5)
        out.append({k: v.to(DEV) for k, v in b.items()})
    return out


@pytest.mark.parametrize("hip_graph", [False, True], ids=["eager", "hip_graph"])
def test_fit_with_the_logger_writes_grids_and_does_not_perturb_training(tmp_path, hip_graph):
    """Three steps with InpaintingLogger(batch_frequency=2, two DDIM steps): grids after batches 0 and 2, three key columns each, the
    token drift logged as device values -- and, the batches carrying their own t and noise, the trained tokens equal those of the
    same run without callbacks bit for bit."""
    from PIL import Image
    from leftrefill_amd.trainer import LearningRateMonitor, Trainer
    tokens = {}
    for name, callbacks in (("plain", None), ("logged", [_logger(batch_frequency=2, save_dir="samples",
                                                                 log_images_kwargs={"ddim_steps": 2, "unconditional_guidance_scale": 2.5}),
                                                         LearningRateMonitor()])):
        m, cfg = _model()
        tr = Trainer(max_steps=3, precision=16, growth_interval=3, default_root_dir=str(tmp_path / name), verbose=False, hip_graph=hip_graph,
                     log_every_n_steps=1, callbacks=callbacks)
        torch.manual_seed(123)
        tr.fit(m, _batches(cfg, 3))
        tokens[name] = m.cond_stage_model.special_embeddings.weight.detach().clone()
        if callbacks:
            root = tmp_path / name / "samples" / "train"
            assert sorted(os.listdir(str(root))) == ["gs-000001_e-000000_b-000000.jpg", "gs-000003_e-000000_b-000002.jpg"]
            for f in os.listdir(str(root)):
                assert Image.open(str(root / f)).size == (3 * (w + 4), B * (h + 2) + 2)
            drift = tr.logged["special_tokens/<t0>"]
            assert torch.is_tensor(drift) and drift.is_cuda and float(drift) > 0 and "special_tokens/<t49>" in tr.logged
            assert callbacks[0]._canvas is not None and m.training and "lr-AdamW" in tr.logged
    assert torch.equal(tokens["plain"], tokens["logged"])


# ---- the training CLI ------------------------------------------------------------------------------------------------------------------------
def test_train_cli_writes_samples_and_top_k_checkpoints_only_when_configured(tmp_path):
    """tools/train_inpainting.py --synthetic 2 --val on the synthetic tiny model of tests/test_gpu_harness.py (restated): with
    `logger_freq: 1` and `save_top_k: 1` (monitor psnr, max: the synthetic model has no LPIPS weights) it leaves samples/train/*.jpg, one
    epoch=*-step=*.ckpt and last.ckpt; the same config without the two keys leaves only last.ckpt."""
    import yaml
    from oracle import weights
    size = 64
    cfg = G.CONFIGS["MID"]
    dd = dict(double_z=True, z_channels=4, resolution=size, in_channels=3, out_ch=3, ch=64, ch_mult=[1, 2, 4, 4], num_res_blocks=1,
              attn_resolutions=[], dropout=0.0)
    model_cfg = {"target": "inpainting_ldm.ref_inpainting_ldm.RefInpaintLDM", "params": dict(
        linear_start=0.00085, linear_end=0.0120, timesteps=1000, first_stage_key="image", cond_stage_key="txt", channels=4,
        cond_stage_trainable=True, conditioning_key="hybrid", scale_factor=0.18215, save_prompt_only=True,
        data_config={"img_size": size, "repeat_sp_token": 4, "sp_token": "<special-token>", "cfg": 2.5},
        unet_config={"target": "ldm.modules.diffusionmodules.openaimodel.UNetModel", "params": cfg.kwargs()},
        first_stage_config={"target": "ldm.models.autoencoder.AutoencoderKL",
                            "params": {"ddconfig": dd, "embed_dim": 4, "lossconfig": {"target": "torch.nn.Identity"}}},
        cond_stage_config={"target": "ldm.modules.encoders.Refill_modules.PromptCLIPEmbedder",
                           "params": dict(freeze=True, layer="penultimate", special_tokens=["repeat_4_<special-token>"],
                                          init_text=["reference on the left target on the right"])})}
    with open(str(tmp_path / "model_config.yaml"), "w") as f:
        yaml.safe_dump({"model": model_cfg}, f)
    stub = tmp_path / "stubs"
    stub.mkdir()
    (stub / "open_clip.py").write_text("from oracle.clip_stub import *  # noqa: F401,F403  (test stand-in for the absent package)\n")
    import leftrefill_amd.dropin as dropin
    dropin.install()
    sys.path.insert(0, str(stub))
    try:
        from inpainting_ldm.model import create_model
        model = create_model(str(tmp_path / "model_config.yaml"))
    finally:
        sys.path.remove(str(stub))
    sd = dict(model.state_dict())
    for k, v in model.state_dict().items():
        if k.startswith("first_stage_model."):
            sd[k] = torch.from_numpy(weights.fill_like("vae2." + k[len("first_stage_model."):], v.shape)).to(v.dtype)
    for k, v in G.unet_state("MID").items():
        sd["model.diffusion_model." + k] = v
    torch.save({"state_dict": sd}, str(tmp_path / "backbone.ckpt"))
    base = dict(model_config=str(tmp_path / "model_config.yaml"), resume_path=str(tmp_path / "backbone.ckpt"), max_steps=2, batch_size=2,
                optim_cfg=dict(learning_rate=1e-3, weight_decay=0.01, lr_scheduler="cosine", eta_min=0.01), val_check_interval=2)
    env = dict(os.environ, PYTHONPATH=os.pathsep.join([str(stub), ROOT, os.environ.get("PYTHONPATH", "")]))
    for name, extra in (("logged", dict(logger_freq=1, save_top_k=1, monitor="psnr", monitor_mode="max")), ("plain", {})):
        with open(str(tmp_path / f"{name}.yaml"), "w") as f:
            yaml.safe_dump(dict(base, **extra), f)
        cmd = [sys.executable, os.path.join(ROOT, "tools", "train_inpainting.py"), "--config_file", str(tmp_path / f"{name}.yaml"),
               "--exp_name", name, "--save_path", str(tmp_path / "runs"), "--fp16", "--synthetic", "2", "--val", "--seed", "3",
               "--log_every_n_steps", "1"]
        r = subprocess.run(cmd, capture_output=True, text=True, cwd=str(tmp_path), env=env, timeout=600)
        assert r.returncode == 0, r.stdout[-1500:] + r.stderr[-3000:]
        assert "step 2: loss" in r.stdout and "psnr " in r.stdout
        run = tmp_path / "runs" / name
        ckpts = sorted(os.listdir(str(run / "ckpts")))
        if extra:
            assert ckpts == ["epoch=0-step=2.ckpt", "last.ckpt"], ckpts
            assert sorted(os.listdir(str(run / "samples" / "train"))) == ["gs-000001_e-000000_b-000000.jpg", "gs-000002_e-000000_b-000001.jpg"]
        else:
            assert ckpts == ["last.ckpt"] and sorted(os.listdir(str(run))) == ["ckpts"]
