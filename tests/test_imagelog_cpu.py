"""CPU: the training image logger -- the numpy statement of the grid (leftrefill_amd/imagelog.py), the drop-in InpaintingLogger on host
tensors, the Trainer's callbacks, ModelCheckpoint, and the C-ABI surface of lr_image_grid / lr_token_drift."""
import ctypes
import os
from types import SimpleNamespace

import numpy as np
import pytest
import torch

import abi_helpers as abi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _rand(shape, seed):
    return (np.random.RandomState(seed).rand(*shape) * 2 - 1).astype(np.float32)


def _byte(x):
    """The reference's three fp32 operations on one array, each rounded on its own."""
    x = np.asarray(x, np.float32)
    return (((x + np.float32(1)) / np.float32(2)) * np.float32(255)).astype(np.uint8)


# ---- grid_numpy ----------------------------------------------------------------------------------------------------------------------------
def test_grid_single_image_is_unpadded_and_keys_follow_KEYS_not_dict_order():
    from leftrefill_amd.imagelog import KEYS, grid_numpy
    assert KEYS == ('masked_image', 'origin_image', 'control', 'warp_image', 'pred', 'reference')
    a, b = _rand((1, 3, 5, 7), 0), _rand((1, 3, 5, 4), 1)
    g = grid_numpy({"pred": b, "masked_image": a, "ignored": a})
    assert g.dtype == np.uint8 and g.shape == (5, 11, 3)
    assert np.array_equal(g[:, :7], _byte(a[0]).transpose(1, 2, 0)) and np.array_equal(g[:, 7:], _byte(b[0]).transpose(1, 2, 0))


@pytest.mark.parametrize("rescale,pad_byte", [(True, 127), (False, 0)])
def test_grid_three_images_padding_and_rows(rescale, pad_byte):
    from leftrefill_amd.imagelog import grid_numpy
    N, H, W = 3, 5, 7
    a = _rand((N, 3, H, W), 2)
    if not rescale:
        a = np.abs(a)
    g = grid_numpy({"origin_image": a}, rescale=rescale)
    assert g.shape == (N * (H + 2) + 2, W + 4, 3)
    inside = np.zeros(g.shape[:2], bool)
    for k in range(N):
        y = k * (H + 2) + 2
        want = _byte(a[k]) if rescale else (a[k] * np.float32(255)).astype(np.uint8)
        assert np.array_equal(g[y:y + H, 2:2 + W], want.transpose(1, 2, 0)), k
        inside[y:y + H, 2:2 + W] = True
    assert (g[~inside] == pad_byte).all()


def test_grid_one_channel_is_repeated_max_images_cuts_and_views_lie_side_by_side():
    from leftrefill_amd.imagelog import grid_numpy
    m = _rand((5, 1, 4, 6), 3)
    g = grid_numpy({"control": m}, max_images=2)
    assert g.shape == (2 * 6 + 2, 10, 3)
    assert np.array_equal(g[..., 0], g[..., 1]) and np.array_equal(g[..., 0], g[..., 2])
    assert np.array_equal(g[8:12, 2:8, 0], _byte(m[1, 0]))
    # generalisation: a 5-D entry [B, V, C, H, W] is V consecutive sources (the reference's make_grid raises on it)
    r = _rand((2, 2, 3, 4, 6), 4)
    g5 = grid_numpy({"reference": r, "pred": r[:, 0]})
    want = np.concatenate([grid_numpy({"pred": r[:, 0]}), grid_numpy({"pred": r[:, 0]}), grid_numpy({"pred": r[:, 1]})], axis=1)
    assert np.array_equal(g5, want)      # KEYS order: pred before reference


def test_grid_refusals():
    from leftrefill_amd.imagelog import grid_numpy
    a = _rand((2, 3, 4, 4), 5)
    a[0, 0, 0, 0] = 1.5
    assert grid_numpy({"pred": a})[2, 2, 0] == 255          # clamped
    with pytest.raises(ValueError, match="outside"):
        grid_numpy({"pred": a}, clamp=False)
    a[0, 0, 0, 0] = np.nan
    with pytest.raises(ValueError, match="non-finite"):
        grid_numpy({"pred": a})
    with pytest.raises(ValueError):
        grid_numpy({"pred": _rand((2, 2, 4, 4), 6)})            # two channels
    with pytest.raises(ValueError):
        grid_numpy({"not_a_key": _rand((2, 3, 4, 4), 6)})


def test_grid_16_bit_inputs_are_widened_first():
    from leftrefill_amd.imagelog import grid_numpy
    a = _rand((2, 3, 4, 4), 7).astype(np.float16)
    assert np.array_equal(grid_numpy({"pred": a}), grid_numpy({"pred": a.astype(np.float32)}))


def boundary_values():
    """fp32(k / 127.5 - 1), k = 0 .. 255, and both fp32 neighbours of each, inside [-1, 1]: the inputs that sit on the truncation steps."""
    x = (np.arange(256) / 127.5 - 1).astype(np.float32)
    xs = np.unique(np.concatenate([x, np.nextafter(x, np.float32(2)), np.nextafter(x, np.float32(-2))]))
    return xs[(xs >= -1) & (xs <= 1)]


def test_truncation_on_the_byte_boundaries():
    """The byte is what the three separately rounded fp32 operations give.  Note: scaling by 2 is exact, so fma(x, 0.5, 0.5) * 255 and
    (x + 1) * 127.5 give the same bytes; the form that rounds once, fma(x, 127.5, 127.5) -- what reassociating and contracting the
    expression would make of it -- does NOT (112 of these 766 inputs differ), which is why the kernel may do neither."""
    from leftrefill_amd.imagelog import grid_numpy
    xs = boundary_values()
    assert len(xs) >= 700
    pad = (-len(xs)) % 3
    img = np.concatenate([xs, np.zeros(pad, np.float32)]).reshape(1, 3, 1, -1)
    g = grid_numpy({"pred": img})
    got = g.transpose(2, 0, 1).reshape(-1)[:len(xs)]
    assert np.array_equal(got, _byte(xs))
    x64 = xs.astype(np.float64)
    once = np.float32(x64 * 127.5 + 127.5).astype(np.uint8)                       # one rounding: the fused, reassociated form
    halves = (np.float32(np.float64(np.float32(x64 * 0.5 + 0.5)) * 255.0)).astype(np.uint8)
    assert (once != got).sum() > 0 and np.array_equal(halves, got)


def test_token_drift_numpy():
    from leftrefill_amd.imagelog import token_drift_numpy
    old, new = _rand((3, 5), 8), _rand((3, 5), 9)
    d = token_drift_numpy(old, new)
    assert d.dtype == np.float64 and d.shape == (3,)
    np.testing.assert_allclose(d, [np.linalg.norm(old[t].astype(np.float64) - new[t]) for t in range(3)], rtol=1e-15)
    assert (token_drift_numpy(old, old) == 0).all()


# ---- the drop-in logger on CPU tensors --------------------------------------------------------------------------------------------------
class _Stub(torch.nn.Module):
    def __init__(self, save_dir, local_rank=0, tokens=True):
        super().__init__()
        self.logger = SimpleNamespace(save_dir=str(save_dir))
        self.local_rank, self.global_step, self.current_epoch = local_rank, 7, 1
        self.logged, self.seen_training, self.kwargs = [], [], None
        if tokens:
            self.cond_stage_model = torch.nn.Module()
            self.cond_stage_model.special_tokens = ["<a>", "<b>"]
            self.cond_stage_model.special_embeddings = torch.nn.Embedding(2, 5)
        g = torch.Generator().manual_seed(0)
        self.images = {"masked_image": (torch.rand(6, 5, 8, 3, generator=g) * 2 - 1).permute(0, 3, 1, 2),
                       "origin_image": torch.rand(6, 3, 5, 8, generator=g) * 2 - 1, "pred": torch.rand(6, 3, 5, 8, generator=g) * 3 - 1.5}

    def log_images(self, batch, split="train", **kw):
        self.seen_training.append(self.training)
        self.kwargs = kw
        assert not torch.is_grad_enabled()
        return dict(self.images)

    def log(self, name, value, **kw):
        self.logged.append((name, float(value)))


def _logger(**kw):
    import leftrefill_amd.dropin as dropin
    dropin.install()
    from inpainting_ldm.logger import InpaintingLogger
    return InpaintingLogger(**kw)


def test_logger_keeps_the_reference_constructor_and_methods():
    import inspect
    lg = _logger()
    sig = inspect.signature(type(lg).__init__).parameters
    want = dict(batch_frequency=2000, max_images=4, clamp=True, increase_log_steps=True, rescale=True, disabled=False, log_on_batch_idx=False,
                log_first_step=False, log_images_kwargs=None, save_dir='image_log')
    assert list(sig)[1:11] == list(want) and all(sig[k].default == v for k, v in want.items())
    assert list(sig)[11:] == ["device"] and sig["device"].default is True
    assert list(inspect.signature(lg.log_local).parameters) == ["save_dir", "split", "images", "global_step", "current_epoch", "batch_idx"]
    assert list(inspect.signature(lg.log_img).parameters) == ["pl_module", "batch", "batch_idx", "split"]
    assert list(inspect.signature(lg.on_train_batch_end).parameters) == ["trainer", "pl_module", "outputs", "batch", "batch_idx", "dataloader_idx"]
    import inpainting_ldm.logger as mod
    assert list(inspect.signature(mod.mapping_color).parameters) == ["img", "vmin", "vmax", "cmap"]


def test_logger_writes_the_reference_file_on_cpu_tensors(tmp_path):
    from PIL import Image
    from leftrefill_amd.imagelog import grid_numpy
    lg = _logger(batch_frequency=2, max_images=4, save_dir="exp/samples", log_images_kwargs={"unconditional_guidance_scale": 2.5})
    m = _Stub(tmp_path)
    m.train()
    trainer = SimpleNamespace(log_every_n_steps=2)
    for idx in range(5):
        if idx == 3:
            with torch.no_grad():
                m.cond_stage_model.special_embeddings.weight[1] += 0.5
        lg.on_train_batch_end(trainer, m, None, {}, idx, 0)
    root = tmp_path / "exp" / "samples" / "train"
    assert sorted(os.listdir(str(root))) == [f"gs-000007_e-000001_b-{i:06}.jpg" for i in (0, 2, 4)]
    assert m.seen_training == [False] * 3 and m.training and m.kwargs == {"unconditional_guidance_scale": 2.5}
    want = grid_numpy({k: v.numpy() for k, v in m.images.items()}, max_images=4)
    assert want.shape == (4 * 7 + 2, 3 * 12, 3) and np.array_equal(lg.canvas(m.images), want)
    im = Image.open(str(root / "gs-000007_e-000001_b-000002.jpg"))
    assert im.size == (want.shape[1], want.shape[0])
    # drift: the first eligible call (batch 0) takes the snapshot, batches 2 and 4 log per token name and refresh it
    names = [n for n, _ in m.logged]
    assert names == ["special_tokens/<a>", "special_tokens/<b>"] * 2
    vals = [v for _, v in m.logged]
    assert vals[0] == vals[1] == vals[2] == 0.0 and abs(vals[3] - 0.5 * 5 ** 0.5) < 1e-6


def test_logger_rank_one_and_disabled_write_nothing(tmp_path):
    lg = _logger(batch_frequency=1)
    m = _Stub(tmp_path / "r1", local_rank=1, tokens=False)
    lg.on_train_batch_end(SimpleNamespace(log_every_n_steps=1), m, None, {}, 0, 0)
    assert m.seen_training == [False] and not (tmp_path / "r1").exists()      # sampled (as the reference does), not written
    off = _logger(batch_frequency=1, disabled=True)
    m0 = _Stub(tmp_path / "off", tokens=False)
    off.on_train_batch_end(SimpleNamespace(log_every_n_steps=1), m0, None, {}, 0, 0)
    assert m0.seen_training == [] and not (tmp_path / "off").exists()
    none = _logger(batch_frequency=1, max_images=0)
    none.on_train_batch_end(SimpleNamespace(log_every_n_steps=1), m0, None, {}, 0, 0)
    assert m0.seen_training == []


# ---- Trainer callbacks on a CPU-only module and optimizer -------------------------------------------------------------------------------------
class _Opt:
    def __init__(self, params):
        self.param_groups = [{"params": params, "lr": 0.25}]
        self.steps = 0

    def scale(self, loss):
        return loss

    def step(self):
        self.steps += 1
        with torch.no_grad():
            for p in self.param_groups[0]["params"]:
                p -= self.param_groups[0]["lr"] * p.grad

    def zero_grad(self):
        for p in self.param_groups[0]["params"]:
            p.grad = None

    def found_inf_tensor(self):
        return torch.zeros(())

    def state_dict(self):
        return {"steps": self.steps}


class _Module(torch.nn.Module):
    def __init__(self):
        super().__init__()
        self.w = torch.nn.Parameter(torch.ones(3))
        self.scores = iter([])

    def configure_optimizers(self):
        return _Opt([self.w])

    def training_step(self, batch, idx):
        return (self.w * batch["x"]).sum()

    def on_train_batch_end(self):
        pass

    def on_save_checkpoint(self, ckpt):
        pass

    def validation_step(self, batch, idx):
        return {"psnr": next(self.scores)}

    def validation_epoch_end(self, outs):
        return {"psnr": float(np.mean([o["psnr"] for o in outs]))}


class _Recorder:
    def __init__(self):
        self.calls, self.vals = [], []

    def on_train_batch_end(self, trainer, model, outputs, batch, batch_idx, dataloader_idx):
        self.calls.append((batch_idx, trainer.global_step, float(outputs.detach()), float(batch["x"][0]), dataloader_idx))

    def on_validation_end(self, trainer, model):
        self.vals.append((trainer.global_step, trainer.logged["val/psnr"]))


def test_trainer_calls_callbacks_after_every_micro_batch(tmp_path):
    from leftrefill_amd.trainer import LearningRateMonitor, ModelCheckpoint, Trainer
    batches = [{"x": torch.full((3,), float(i + 1))} for i in range(3)]
    rec, m = _Recorder(), _Module()
    m.scores = iter([10.0, 20.0])
    tr = Trainer(max_steps=3, accumulate_grad_batches=2, precision=32, verbose=False, default_root_dir=str(tmp_path), val_check_interval=2,
                 callbacks=[rec, LearningRateMonitor(), ModelCheckpoint(str(tmp_path / "ckpts"), 1, "val/psnr", "max")])
    tr.fit(m, batches, val_batches=[batches[0]])
    assert sorted(os.listdir(str(tmp_path / "ckpts"))) == ["epoch=1-step=2.ckpt", "last.ckpt"]      # a callback with one hook only
    assert torch.load(str(tmp_path / "ckpts" / "epoch=1-step=2.ckpt"), weights_only=False)["global_step"] == 2
    # 3 optimizer steps = 6 micro-batches = two passes over the three batches; in-epoch indices; global_step moves every second call
    assert [(c[0], c[1]) for c in rec.calls] == [(0, 0), (1, 1), (2, 1), (0, 2), (1, 2), (2, 3)]
    assert [c[3] for c in rec.calls] == [1.0, 2.0, 3.0, 1.0, 2.0, 3.0] and all(c[4] == 0 for c in rec.calls)
    assert rec.vals == [(2, 10.0)] and tr.logged["val/psnr"] == 10.0 and tr.logged["lr-AdamW"] == 0.25
    assert tr.logger.save_dir == str(tmp_path) and m.logger is tr.logger and m.current_epoch == tr.current_epoch
    # without callbacks: the same parameters
    m2 = _Module()
    Trainer(max_steps=3, accumulate_grad_batches=2, precision=32, verbose=False).fit(m2, batches)
    assert torch.equal(m.w, m2.w) and Trainer(max_steps=1).callbacks == []


@pytest.mark.parametrize("mode,kept", [("min", {1: 2.0, 3: 1.0}), ("max", {2: 5.0, 4: 4.0})])
def test_model_checkpoint_keeps_the_top_two_of_five(tmp_path, mode, kept):
    from leftrefill_amd.trainer import ModelCheckpoint
    saved = []

    class _T:
        local_rank, current_epoch, global_step, default_root_dir, logged = 0, 0, 0, None, {}

        def save_checkpoint(self, model, path):
            os.makedirs(os.path.dirname(path), exist_ok=True)
            open(path, "w").write(str(self.logged["val/s"]))
            saved.append(os.path.basename(path))

    t, d = _T(), str(tmp_path / "ckpts")
    mc = ModelCheckpoint(d, 2, "val/s", mode, save_last=False)
    history = []
    for step, score in enumerate([3.0, 2.0, 5.0, 1.0, 4.0]):
        t.global_step, t.current_epoch, t.logged = step, step // 2, {"val/s": score}
        mc.on_validation_end(t, None)
        history.append(sorted(os.listdir(d)))
    name = lambda s: f"epoch={s // 2}-step={s}.ckpt"
    assert history[-1] == sorted(name(s) for s in kept)
    assert {float(open(os.path.join(d, name(s))).read()) for s in kept} == set(kept.values())
    if mode == "min":      # 3 | 3 2 | (5 refused) | 2 1 (3 deleted) | (4 refused)
        assert saved == [name(0), name(1), name(3)] and history[2] == sorted([name(0), name(1)])
        assert mc.best_model_path == os.path.join(d, name(3))
    else:                  # 3 | 3 2 | 3 5 (2 deleted) | (1 refused) | 5 4 (3 deleted)
        assert saved == [name(0), name(1), name(2), name(4)] and history[3] == sorted([name(0), name(2)])
    # save_top_k = 0 keeps none, -1 keeps all
    for k, n in ((0, 0), (-1, 3)):
        dk = str(tmp_path / f"k{k}")
        os.makedirs(dk)
        mk = ModelCheckpoint(dk, k, "val/s", mode, save_last=False)
        for step, score in enumerate([3.0, 2.0, 5.0]):
            t.global_step, t.logged = 10 + step, {"val/s": score}
            mk.on_validation_end(t, None)
        assert len(os.listdir(dk)) == n
    with pytest.raises(KeyError):
        t.logged = {}
        mc.on_validation_end(t, None)


# ---- ABI and struct ----------------------------------------------------------------------------------------------------------------------------
def test_abi_surface_of_the_logger_kernels():
    from leftrefill_amd import _lib, build
    for name, count in (("lr_image_grid", 9), ("lr_token_drift", 6)):
        assert len(abi.c_params(name)) == count, name        # header against binding: tests/test_abi_cpu.py
    assert "image_grid.hip" in build.SOURCES and _lib.ABI_VERSION == 30
    assert abi.define("LR_GRID_MAX_SOURCES") == 8
    from leftrefill_amd import imagelog
    assert imagelog.MAX_SOURCES == 8 and ctypes.sizeof(_lib.GridSource) == 56      # every offset: tests/test_abi_cpu.py
