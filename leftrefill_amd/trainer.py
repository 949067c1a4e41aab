"""A small fit loop for the drop-in task models: what the reference gets from pytorch_lightning.Trainer in train_inpainting.py.

    trainer = Trainer(max_steps=12000, precision=16, accumulate_grad_batches=2, default_root_dir="check_points/exp")
    trainer.fit(model, train_batches, val_batches)

The module's own hooks do the work -- training_step, configure_optimizers (AmpAdamW: unscale, skip decision, loss-scale update, lr
schedule and AdamW in one device-side step), on_train_epoch_start (when defined: at the start of every pass over the training
batches, `trainer.train_dataloader` set), on_train_batch_end, validation_step / validation_epoch_end, on_save_checkpoint -- and
the trainer serves what they expect from Lightning: `module.trainer`, `global_step`, `local_rank`, `log`.  Gradients are averaged over
ranks with dist.allreduce_mean_grads before the step, so every rank takes the same skip decision.

`<default_root_dir>/ckpts/last.ckpt` has Lightning 1.5's keys (`state_dict` after on_save_checkpoint, `optimizer_states`,
`lr_schedulers`, `global_step`, `epoch`, `native_amp_scaling_state`), so inpainting_ldm.model.load_state_dict and
tools/run_inpainting.py read it; `resume_from_checkpoint` continues from one.

`callbacks`: objects with Lightning's hooks.  After EVERY micro-batch (accumulate_grad_batches does not thin it; on a batch that ends an
optimizer step, after the step) each one's `on_train_batch_end(trainer, model, loss, batch, idx, 0)` is called with the in-epoch index --
under hip_graph with the static batch -- and after each validation its `on_validation_end(trainer, model)`; a callback has either hook
or both.  The trainer serves them `global_step`, `current_epoch`, `local_rank`, `log_every_n_steps`, `log`, `logged` (validation adds
the means of `validation_epoch_end` as `val/<key>`) and `logger.save_dir` (= default_root_dir; the module gets the same `logger`).
`inpainting_ldm.logger.InpaintingLogger`, `ModelCheckpoint` and `LearningRateMonitor` below are such callbacks.

hip_graph=True captures training_step + backward + optimizer step of one micro-batch as one hipGraph (fixed shapes; batches must be
dicts of tensors, which are copied into static device buffers before every replay).  It needs accumulate_grad_batches == 1 and a
single rank.
"""
import os
from types import SimpleNamespace

import torch

from . import dist as lrd


class Trainer:
    def __init__(self, max_steps, accumulate_grad_batches=1, val_check_interval=None, precision=16, default_root_dir=None,
                 resume_from_checkpoint=None, hip_graph=False, growth_interval=2000, local_rank=0, log_every_n_steps=50, verbose=True,
                 callbacks=None):
        assert str(precision) in ("16", "bf16", "32"), "precision: 16 | 'bf16' | 32"
        self.max_steps, self.accumulate_grad_batches = int(max_steps), int(accumulate_grad_batches)
        self.val_check_interval, self.precision = val_check_interval, precision
        self.default_root_dir, self.resume_from_checkpoint = default_root_dir, resume_from_checkpoint
        self.hip_graph, self.growth_interval, self.local_rank = bool(hip_graph), int(growth_interval), int(local_rank)
        self.log_every_n_steps, self.verbose = log_every_n_steps, verbose
        self.callbacks = list(callbacks or [])
        self.logger = SimpleNamespace(save_dir=default_root_dir)      # what Lightning's `trainer.logger` / `module.logger` give a callback
        self.global_step = self.current_epoch = 0
        self.optimizer = self.lr_schedulers = None
        self.logged = {}            # last value of every logged name (device tensors stay on the device until someone reads them)
        self.val_results = []
        self.found_inf_history = []      # one 0-dim device tensor per optimizer step (1 = skipped); never read back by the trainer
        self.loss_history = []           # the loss of every optimizer step's last micro-batch, 0-dim device tensors (fp32 copies)
        if hip_graph and self.accumulate_grad_batches != 1:
            raise ValueError("hip_graph needs accumulate_grad_batches == 1")

    # ---- what the module reads through `self.trainer` -----------------------------------------------------------------------------
    def log(self, name, value, **_):
        self.logged[name] = value

    def log_dict(self, d, **kw):
        for k, v in d.items():
            self.log(k, v, **kw)

    @property
    def loss_scale_after_step(self):
        """Callable returning the loss scale as a 0-dim DEVICE tensor (a view of the optimizer's state block: nothing is read back), or
        None when the precision has no scaler."""
        if str(self.precision) != "16" or self.optimizer is None:
            return None
        return self.optimizer.scale_tensor

    # ---- checkpoints ---------------------------------------------------------------------------------------------------------------
    def checkpoint(self, model):
        ckpt = {"epoch": self.current_epoch, "global_step": self.global_step, "pytorch-lightning_version": "1.5.0",
                "state_dict": {k: v.detach().cpu().clone() for k, v in model.state_dict().items()},
                "optimizer_states": [self.optimizer.state_dict()],
                "lr_schedulers": [s["scheduler"].state_dict() for s in self.lr_schedulers], "callbacks": {}}
        if str(self.precision) == "16":
            ckpt["native_amp_scaling_state"] = self.optimizer.scaler_state_dict()
        model.on_save_checkpoint(ckpt)
        return ckpt

    def save_checkpoint(self, model, path=None):
        if path is None:
            if self.default_root_dir is None:
                return None
            path = os.path.join(self.default_root_dir, "ckpts", "last.ckpt")
        if self.local_rank == 0:
            os.makedirs(os.path.dirname(path), exist_ok=True)
            torch.save(self.checkpoint(model), path + ".tmp")
            os.replace(path + ".tmp", path)
        return path

    def _resume(self, model, path):
        ckpt = torch.load(path, map_location="cpu", weights_only=False)
        missing, unexpected = model.load_state_dict(ckpt["state_dict"], strict=False)
        assert not unexpected, f"{path}: keys the model does not have: {unexpected[:5]}"
        self.optimizer.load_state_dict(ckpt["optimizer_states"][0])
        self.global_step, self.current_epoch = int(ckpt["global_step"]), int(ckpt.get("epoch", 0))
        hook = getattr(model, "on_load_checkpoint", None)      # Lightning's hook: state a module keeps outside its state_dict
        if hook is not None:
            hook(ckpt)

    # ---- the loop ----------------------------------------------------------------------------------------------------------------------
    def _setup(self, model):
        model.trainer = self
        model.log, model.log_dict = self.log, self.log_dict      # Lightning's logging calls of the module's hooks
        model.logger = self.logger
        if not hasattr(model, "current_epoch"):      # the task models have it (ddpm.py); a bare module gets Lightning's live view
            type(model).current_epoch = property(lambda m: getattr(m.trainer, "current_epoch", 0))
        model.train()
        conf = model.configure_optimizers()
        if isinstance(conf, tuple):
            opts, sches = conf
            self.optimizer, self.lr_schedulers = opts[0], list(sches)
        else:
            self.optimizer, self.lr_schedulers = conf, []
        self.params = [p for g in self.optimizer.param_groups for p in g["params"]]
        owned = {id(p) for p in self.params}
        for p in model.parameters():
            p.requires_grad_(id(p) in owned)
        unet = getattr(getattr(model, "model", None), "diffusion_model", None)
        if unet is not None and hasattr(unet, "compute_dtype") and str(self.precision) != "32":
            unet.compute_dtype = torch.bfloat16 if str(self.precision) == "bf16" else torch.float16
        if self.resume_from_checkpoint:
            self._resume(model, self.resume_from_checkpoint)

    def _micro_step(self, model, batch, idx):
        loss = model.training_step(batch, idx)
        self.optimizer.scale(loss / self.accumulate_grad_batches).backward()
        return loss

    def _optimizer_step(self):
        lrd.allreduce_mean_grads(self.params)
        self.optimizer.step()
        self.optimizer.zero_grad()

    def _capture(self, model, batch):
        """Warm up on a side stream, then capture one whole step; returns (graph, static batch)."""
        import torch.distributed as dist
        if dist.is_available() and dist.is_initialized() and dist.get_world_size() > 1:
            raise RuntimeError("hip_graph: single rank only (the gradient all-reduce is not captured)")
        if getattr(model, "ucg_training", None):
            raise RuntimeError("hip_graph: ucg_training edits the batch on the host at every step; a captured step would freeze it")
        static = {k: (v.to(model.device).clone() if torch.is_tensor(v) else v) for k, v in batch.items()}
        rng = torch.get_rng_state(), torch.cuda.get_rng_state()      # the warm-up draws noise / timesteps: give them back
        snap = ([p.detach().clone() for p in self.params], self.optimizer.snapshot())
        side = torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):
            for _ in range(2):      # allocates gradient buffers, moments and the descriptor table; undone below
                self._micro_step(model, static, 0)
                self._optimizer_step()
        torch.cuda.current_stream().wait_stream(side)
        torch.cuda.synchronize()
        with torch.no_grad():
            for p, q in zip(self.params, snap[0]):
                p.copy_(q)
        self.optimizer.restore(snap[1])
        torch.set_rng_state(rng[0])
        torch.cuda.set_rng_state(rng[1])
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph):
            self._static_loss = self._micro_step(model, static, 0)
            self._optimizer_step()
        return graph, static

    def fit(self, model, train_batches, val_batches=None):
        self._setup(model)
        self.train_dataloader = train_batches      # what a module's on_train_epoch_start reaches the sampler through
        graph = static = None
        micro = 0
        while self.global_step < self.max_steps:
            if hasattr(model, "on_train_epoch_start"):
                model.on_train_epoch_start()
            seen = 0
            for idx, batch in enumerate(train_batches):
                seen += 1
                if self.hip_graph:
                    if graph is None:
                        graph, static = self._capture(model, batch)
                    for k, v in batch.items():
                        if torch.is_tensor(v):
                            static[k].copy_(v)
                        elif v != static[k]:
                            raise RuntimeError(f"hip_graph: batch entry {k!r} is not a tensor and changed since the capture")
                    graph.replay()
                    self.optimizer.advance_host()
                    loss = self._static_loss
                else:
                    loss = self._micro_step(model, batch, idx)
                micro += 1
                stepped = micro % self.accumulate_grad_batches == 0
                if stepped:
                    if not self.hip_graph:
                        self._optimizer_step()
                    self.global_step += 1
                    self.found_inf_history.append(self.optimizer.found_inf_tensor().clone())
                    self.logged["loss"] = loss.detach()
                    self.loss_history.append(loss.detach().float().clone())
                    model.on_train_batch_end()
                for cb in self.callbacks:
                    if hasattr(cb, "on_train_batch_end"):
                        cb.on_train_batch_end(self, model, loss, static if self.hip_graph else batch, idx, 0)
                if not stepped:
                    continue
                if self.verbose and self.local_rank == 0 and self.global_step % self.log_every_n_steps == 0:
                    print(f"step {self.global_step}: loss {float(loss):.5f} lr {self.optimizer.param_groups[0]['lr']:.3e} "
                          f"scale {self.optimizer.amp_state()['scale']:g}", flush=True)
                if self.val_check_interval and val_batches is not None and self.global_step % self.val_check_interval == 0:
                    self.validate(model, val_batches)
                    self.save_checkpoint(model)
                if self.global_step >= self.max_steps:
                    break
            if seen == 0:
                raise ValueError("Trainer.fit: the training iterable is empty")
            self.current_epoch += 1
        self.save_checkpoint(model)
        return self

    def validate(self, model, val_batches):
        was_training = model.training
        model.eval()
        device = next(model.parameters()).device      # Lightning moves a batch to the module's device; a DataLoader hands over host tensors
        with torch.no_grad():
            outs = [model.validation_step({k: (v.to(device) if torch.is_tensor(v) else v) for k, v in b.items()} if isinstance(b, dict) else b, i)
                    for i, b in enumerate(val_batches)]
        means = model.validation_epoch_end(outs)
        for k, v in (means or {}).items():
            self.logged[f"val/{k}"] = v
        self.val_results.append(outs)
        model.train(was_training)
        for cb in self.callbacks:
            if hasattr(cb, "on_validation_end"):
                cb.on_validation_end(self, model)
        return outs


class ModelCheckpoint:
    """Keeps the best `save_top_k` checkpoints by `trainer.logged[monitor]` (what Lightning's ModelCheckpoint does for the reference's
    train_inpainting.py:104-111): after every validation, `<dirpath>/epoch={e}-step={s}.ckpt` with the payload of `Trainer.checkpoint`
    when the score is among the best so far, and the worst kept file deleted when a better one arrives.  save_top_k = 0 keeps none, -1
    all.  mode: 'min' | 'max'.  Rank 0 writes and deletes.  save_last: `<dirpath>/last.ckpt` after every validation as well (the trainer's
    own `<default_root_dir>/ckpts/last.ckpt` is written by the trainer as before, and not twice when it is the same file)."""

    def __init__(self, dirpath, save_top_k, monitor, mode="min", save_last=True):
        if mode not in ("min", "max"):
            raise ValueError(f"ModelCheckpoint: mode {mode!r} is neither 'min' nor 'max'")
        self.dirpath, self.save_top_k, self.monitor, self.mode, self.save_last = dirpath, int(save_top_k), monitor, mode, save_last
        self.best_k = {}      # path -> score of the kept checkpoints

    def _worse(self, a, b):
        return a > b if self.mode == "min" else a < b

    def on_validation_end(self, trainer, model):
        if self.save_last:
            last = os.path.join(self.dirpath, "last.ckpt")
            own = trainer.default_root_dir and os.path.join(trainer.default_root_dir, "ckpts", "last.ckpt")
            if not own or os.path.abspath(own) != os.path.abspath(last):
                trainer.save_checkpoint(model, last)
        if self.save_top_k == 0:
            return
        if self.monitor not in trainer.logged:
            raise KeyError(f"ModelCheckpoint: {self.monitor!r} was not logged by the validation (logged: {sorted(trainer.logged)})")
        score = float(trainer.logged[self.monitor])
        path = os.path.join(self.dirpath, f"epoch={trainer.current_epoch}-step={trainer.global_step}.ckpt")
        full = self.save_top_k > 0 and len(self.best_k) >= self.save_top_k and path not in self.best_k
        worst = None
        if full:
            worst = (max if self.mode == "min" else min)(self.best_k, key=self.best_k.get)
            if not self._worse(self.best_k[worst], score):
                return
        trainer.save_checkpoint(model, path)
        self.best_k[path] = score
        if full:
            del self.best_k[worst]
            if trainer.local_rank == 0 and os.path.exists(worst):
                os.remove(worst)

    @property
    def best_model_path(self):
        if not self.best_k:
            return ""
        return (min if self.mode == "min" else max)(self.best_k, key=self.best_k.get)


class LearningRateMonitor:
    """One `trainer.log('lr-AdamW', lr)` per optimizer step (Lightning's LearningRateMonitor names a single AdamW that way)."""

    def __init__(self):
        self._step = None

    def on_train_batch_end(self, trainer, model, outputs, batch, batch_idx, dataloader_idx):
        if trainer.global_step != self._step:      # micro-batches inside an accumulation window take no optimizer step
            self._step = trainer.global_step
            trainer.log("lr-AdamW", trainer.optimizer.param_groups[0]["lr"])
