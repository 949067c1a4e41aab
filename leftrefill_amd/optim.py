"""AmpAdamW: torch.optim.AdamW + torch.amp.GradScaler as ONE device-side step (csrc/optim.hip, lr_amp_adamw_step).

The gradient unscale, the non-finite scan, the skip decision, the loss-scale update, the per-step learning rate and the AdamW update
all happen on the device: `step()` is a single ops call of three launches that reads nothing back, so a whole training step --
forward, HIP backward, optimizer -- replays as one hipGraph even in fp16 with a dynamic loss scale.

    opt = AmpAdamW(params, lr=1e-4, weight_decay=0.01)                 # fp16: scale 65536, x2 every 2000 clean steps, /2 on overflow
    opt = AmpAdamW(params, lr=1e-4, init_scale=1.0, growth_interval=0) # bf16 / fp32: same kernel, no scaler dynamics
    opt.set_schedule(cosine_schedule(opt, max_steps, eta_min))         # per-step lr table, torch's own CosineAnnealingLR values
    opt.scale(loss).backward(); opt.step(); opt.zero_grad()

The lr index advances on every step() (a per-step scheduler steps whether or not the update was skipped); the AdamW bias-correction
step advances only on applied steps.  Gradient buffers are kept between steps (zero_grad() zeroes in place) so that the descriptor
table, which holds raw pointers, stays valid; a changed pointer rebuilds it outside of graph capture and is an error inside.
"""
import torch

from . import _lib, ops

_THREADS = 256


def cosine_schedule(opt, max_steps, eta_min):
    """Per-step learning rates [max_steps + 1][n_groups] of `CosineAnnealingLR(opt, max_steps, eta_min=eta_min)` (eta_min absolute), produced by
    stepping torch's own scheduler on a scratch optimizer with `opt`'s group learning rates (entry k is the rate of step k)."""
    lrs = [g["lr"] for g in opt.param_groups]
    scratch = torch.optim.SGD([{"params": [torch.zeros(1, requires_grad=True)], "lr": lr} for lr in lrs], lr=lrs[0])
    sche = torch.optim.lr_scheduler.CosineAnnealingLR(scratch, max_steps, eta_min=eta_min)
    rows = [[g["lr"] for g in scratch.param_groups]]
    for _ in range(max_steps):
        scratch.step()
        sche.step()
        rows.append([g["lr"] for g in scratch.param_groups])
    return rows


class AmpAdamW(torch.optim.Optimizer):
    def __init__(self, params, lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=1e-2, init_scale=65536.0, growth_factor=2.0,
                 backoff_factor=0.5, growth_interval=2000):
        if growth_interval < 0 or (growth_interval > 0 and not (growth_factor > 1.0 and 0.0 < backoff_factor < 1.0)):
            raise ValueError("AmpAdamW: growth_interval >= 0, growth_factor > 1, 0 < backoff_factor < 1")
        super().__init__(params, dict(lr=lr, betas=betas, eps=eps, weight_decay=weight_decay))
        if len(self.param_groups) > ops.OPT_MAX_GROUPS:
            raise ValueError(f"AmpAdamW: at most {ops.OPT_MAX_GROUPS} parameter groups")
        self.growth_factor, self.backoff_factor, self.growth_interval = float(growth_factor), float(backoff_factor), int(growth_interval)
        ps = [p for g in self.param_groups for p in g["params"]]
        for p in ps:
            if p.dtype != torch.float32 or not p.is_contiguous():      # (a CPU model can be configured and checkpointed; step() needs the GPU)
                raise ValueError("AmpAdamW: parameters are contiguous fp32 tensors (the master copy)")
        self.device = ps[0].device
        self._state = torch.zeros(ops.OPT_STATE_WORDS, dtype=torch.int32, device=self.device)
        self._state_f = self._state.view(torch.float32)
        self._state_f[0] = float(init_scale)
        self._ext_grads = {}
        self._calls = 0                                   # host mirror of sched_steps: step() advances it unconditionally
        self._schedule = [[g["lr"] for g in self.param_groups]]      # [steps][groups], host copy of the lr tables
        self._lr_tables = None
        self._sig = None
        self._upload_schedule()

    # ---- learning-rate table -------------------------------------------------------------------------------------------------------
    def set_schedule(self, values):
        """values[k]: the learning rate of step k -- a number (every group) or one number per group.  Past the end the last entry holds."""
        rows = [[float(v)] * len(self.param_groups) if not hasattr(v, "__len__") else [float(x) for x in v] for v in values]
        if not rows or any(len(r) != len(self.param_groups) for r in rows):
            raise ValueError("set_schedule: a non-empty list of one rate, or one rate per group, per step")
        self._schedule = rows
        self._upload_schedule()

    def _upload_schedule(self):
        t = torch.tensor(self._schedule, dtype=torch.float64).to(torch.float32)      # the fp32 cast of the scheduler's values
        self._lr_tables = t.t().contiguous().to(self.device)                          # [groups][steps]
        self._sig = None
        self._sync_host_lr()

    def lr_table(self):
        """[groups][steps] fp32 device table the kernel indexes."""
        return self._lr_tables

    def _sync_host_lr(self):
        row = self._schedule[min(self._calls, len(self._schedule) - 1)]
        for g, lr in zip(self.param_groups, row):
            g["lr"] = lr

    # ---- loss scale ----------------------------------------------------------------------------------------------------------------
    def scale(self, loss):
        """loss * scale, the scale read on the device."""
        return loss * self._state_f[0]

    def scale_tensor(self):
        """The loss scale as a 0-dim device tensor (a view of the state block)."""
        return self._state_f[0]

    def found_inf_tensor(self):
        """1 when the last step() was skipped, as a 0-dim int32 device tensor (a view of the state block)."""
        return self._state[2]

    def amp_state(self):
        """The device state block as a dict (one read-back: for checkpoints, logging and tests, not for the step)."""
        w = self._state[:ops.OPT_CONSTS].cpu()
        f = w.view(torch.float32)
        out = {n: (float(f[i]) if n in ("scale", "grad_norm", "inv_scale") else int(w[i])) for i, n in enumerate(ops.OPT_STATE_FIELDS)}
        c = self._state_f[ops.OPT_CONSTS:ops.OPT_CONSTS + 4 * len(self.param_groups)].cpu().reshape(-1, 4)
        out["lr"] = [float(r[3]) for r in c]
        return out

    def scaler_state_dict(self):
        """What torch.amp.GradScaler.state_dict() holds, from the device block."""
        s = self.amp_state()
        return {"scale": s["scale"], "growth_factor": self.growth_factor, "backoff_factor": self.backoff_factor,
                "growth_interval": self.growth_interval, "_growth_tracker": s["growth_tracker"]}

    def bind_grads(self, grads):
        """Read gradients from `grads` ({param: tensor}, fp32 / fp16 / bf16, scaled by the loss scale) instead of `param.grad` -- the 16-bit
        buffers a HIP backward leaves behind need no fp32 copy."""
        self._ext_grads = dict(grads)
        self._sig = None

    def _grad(self, p):
        return self._ext_grads.get(p, p.grad)

    # ---- descriptor tables ---------------------------------------------------------------------------------------------------------
    def _signature(self):
        sig = []
        for gi, g in enumerate(self.param_groups):
            sig.append((g["betas"], g["eps"], g["weight_decay"]))
            for p in g["params"]:
                gr = self._grad(p)
                if gr is None:
                    continue
                st = self.state.get(p)
                sig.append((gi, p.data_ptr(), gr.data_ptr(), gr.dtype, st["exp_avg"].data_ptr() if st else 0,
                            st["exp_avg_sq"].data_ptr() if st else 0))
        return tuple(sig)

    def _build(self):
        if torch.cuda.is_current_stream_capturing():
            raise RuntimeError("AmpAdamW: a gradient buffer moved during graph capture; run one eager step first and zero gradients in place")
        rows, numel = [], 1
        for gi, g in enumerate(self.param_groups):
            for p in g["params"]:
                gr = self._grad(p)
                if gr is None:
                    continue
                if gr.dtype not in ops.OPT_GRAD_KIND or not gr.is_contiguous() or gr.shape != p.shape or not p.is_cuda:
                    raise ValueError("AmpAdamW: gradients are contiguous device fp32 / fp16 / bf16 tensors of the parameter's shape")
                st = self.state[p]
                if "exp_avg" not in st:
                    st["exp_avg"] = torch.zeros_like(p, memory_format=torch.contiguous_format)
                    st["exp_avg_sq"] = torch.zeros_like(p, memory_format=torch.contiguous_format)
                rows.append(_lib.OptimTensor(p.data_ptr(), gr.data_ptr(), st["exp_avg"].data_ptr(), st["exp_avg_sq"].data_ptr(),
                                             p.numel(), ops.OPT_GRAD_KIND[gr.dtype], gi))
                numel = max(numel, p.numel())
        if not rows:
            raise RuntimeError("AmpAdamW.step: no parameter has a gradient")
        steps = self._lr_tables.shape[1]
        groups = [_lib.OptimGroup(g["betas"][0], g["betas"][1], g["eps"], g["weight_decay"],
                                  self._lr_tables.data_ptr() + 4 * steps * gi, steps, 0) for gi, g in enumerate(self.param_groups)]

        def upload(structs):
            arr = (type(structs[0]) * len(structs))(*structs)
            return torch.frombuffer(bytearray(bytes(arr)), dtype=torch.uint8).to(self.device)

        self._tensors, self._n_tensors = upload(rows), len(rows)
        self._groups = upload(groups)
        self._blocks = max(1, min(512, -(-numel // (4 * _THREADS))))
        self._partials = torch.zeros(4 * self._blocks, dtype=torch.float32, device=self.device)
        self._sig = self._signature()

    # ---- torch.optim.Optimizer surface -----------------------------------------------------------------------------------------------
    def zero_grad(self, set_to_none=False):
        """Zeroes in place by default: the descriptor table holds the gradient pointers."""
        super().zero_grad(set_to_none=set_to_none)

    @torch.no_grad()
    def step(self, closure=None):
        loss = None
        if closure is not None:
            with torch.enable_grad():
                loss = closure()
        if self._sig is None or self._sig != self._signature():
            self._build()
        ops.amp_adamw_step(self._tensors, self._n_tensors, self._groups, len(self.param_groups), self._state, self._partials,
                           self._blocks, self.growth_factor, self.backoff_factor, self.growth_interval)
        if not torch.cuda.is_current_stream_capturing():      # a replayed graph advances the device index; advance_host() mirrors it
            self.advance_host()
        return loss

    def advance_host(self, n=1):
        """Advance the host mirror of the lr index (param_groups[i]['lr']) by n steps -- call it after a graph replay."""
        self._calls += n
        self._sync_host_lr()

    def snapshot(self):
        """Device state block, moments and host step count, for restore(): buffers keep their addresses (a captured graph stays valid)."""
        return (self._state.clone(), self._calls, {p: (st["exp_avg"].clone(), st["exp_avg_sq"].clone()) for p, st in self.state.items()})

    def restore(self, snap):
        block, calls, moments = snap
        self._state.copy_(block)
        for p, st in self.state.items():
            for name, old in zip(("exp_avg", "exp_avg_sq"), moments.get(p, (None, None))):
                st[name].zero_() if old is None else st[name].copy_(old)
        self._calls = calls
        self._sync_host_lr()

    def state_dict(self):
        d = super().state_dict()
        d["amp"] = dict(self.amp_state(), growth_factor=self.growth_factor, backoff_factor=self.backoff_factor,
                        growth_interval=self.growth_interval)
        d["lr_schedule"] = [list(r) for r in self._schedule]
        return d

    def load_state_dict(self, state_dict):
        state_dict = dict(state_dict)
        amp, sched = state_dict.pop("amp", None), state_dict.pop("lr_schedule", None)
        super().load_state_dict(state_dict)
        if sched is not None:
            self._schedule = [list(r) for r in sched]
        if amp is not None:
            self.growth_factor, self.backoff_factor = float(amp["growth_factor"]), float(amp["backoff_factor"])
            self.growth_interval = int(amp["growth_interval"])
            w = torch.zeros(ops.OPT_STATE_WORDS, dtype=torch.int32)
            f = w.view(torch.float32)
            for i, n in enumerate(ops.OPT_STATE_FIELDS):
                if n in ("scale", "grad_norm", "inv_scale"):
                    f[i] = float(amp[n])
                else:
                    w[i] = int(amp[n])
            self._state.copy_(w)
            self._calls = int(amp["sched_steps"])
        self._upload_schedule()


class TableSchedule:
    """The `scheduler` entry configure_optimizers returns beside an AmpAdamW with a schedule: the rates live in the optimizer's device
    table and the kernel advances the index, so step() has nothing to do; state_dict() is what a checkpoint's `lr_schedulers` holds."""

    def __init__(self, opt):
        self.optimizer = opt

    def step(self):
        pass

    def get_last_lr(self):
        return [g["lr"] for g in self.optimizer.param_groups]

    def state_dict(self):
        return {"last_epoch": self.optimizer._calls, "_last_lr": self.get_last_lr(), "T_max": len(self.optimizer._schedule) - 1}

    def load_state_dict(self, d):
        pass      # the optimizer's own state carries the index


def configure_prompt_optimizer(module, groups):
    """configure_optimizers of the task models: `groups` (torch param-group dicts) on AmpAdamW with `module.optim_cfg`'s learning rate and
    weight decay; fp16 (`trainer.precision == 16`, the default) gets GradScaler's dynamics, bf16 / 32 the scale-1 mode.  `cosine` returns
    ([opt], [{scheduler, interval: step, frequency: 1}]) like the reference; any other name prints its message and returns the optimizer."""
    cfg = module.optim_cfg
    lr, wd = cfg["learning_rate"], cfg["weight_decay"]
    trainer = getattr(module, "trainer", None)
    if str(getattr(trainer, "precision", 16)) == "16":
        amp = dict(growth_interval=int(getattr(trainer, "growth_interval", 2000)))
    else:
        amp = dict(init_scale=1.0, growth_interval=0)
    opt = AmpAdamW(groups, lr=lr, weight_decay=wd, **amp)
    name = cfg["lr_scheduler"]
    if name == "cosine":
        opt.set_schedule(cosine_schedule(opt, trainer.max_steps, cfg["eta_min"] * lr))
        return [opt], [{"scheduler": TableSchedule(opt), "interval": "step", "frequency": 1}]
    print("Unknown scheduler", name)
    return opt


def keep_keys(checkpoint, keep):
    """on_save_checkpoint's filter: drop every state_dict entry `keep(key)` refuses, in place."""
    sd = checkpoint["state_dict"]
    for key in [k for k in sd if not keep(k)]:
        del sd[key]
