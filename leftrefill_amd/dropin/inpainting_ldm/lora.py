"""`inpainting_ldm.lora` -- LoRA injection for the UNet's attention and GEGLU Linears on the MI355X build.

The surface of the reference module (inpainting_ldm/lora.py), written for this package:
  * `LoraInjectedLinear(in_features, out_features, bias, r, dropout_p, scale)` with the sub-modules `linear` / `lora_down` / `dropout` /
    `lora_up` / `selector`, the attributes `r` and `scale`, `realize_as_lora()`; down ~ N(0, 1/r^2), up = 0;
  * `_find_modules` (= `_find_modules_v2`): every module of the searched classes below a module whose class NAME is in the ancestor set,
    as (direct parent, name in that parent, module), children of an injected layer left out;
  * `inject_trainable_lora(model, target_replace_module, r, loras, verbose, dropout_p, scale)` -> (parameter iterators in the order
    up, down per layer; the child names) and `extract_lora_ups_down`;
  * state-dict keys `<layer>.linear.weight`, `<layer>.lora_down.weight`, `<layer>.lora_up.weight`.
tests/test_lora_cpu.py pins names, order and keys against what the reference's module produced (tests/golden/lora.npz).

On the device the injected layers do not run as modules: `UNetModel` packs them (leftrefill_amd.engine: merged for sampling, base GEMM +
lr_lora_down + lr_lora_up with HIP factor gradients for training).  `LoraInjectedLinear.forward` is the plain-torch statement of the layer
for CPU tensors (what the CPU tests compare against); a device tensor is refused -- this package has no BLAS path.

LoRA dropout: `inject_trainable_lora(..., dropout_p=p)` gives layer i the stream id `drop_stream = i` (the order of the returned names) and
the model one `LoraDropoutState` (seed, draw).  The mask is counter-based (leftrefill_amd.lora_dropout: Philox on (row, column group,
stream, draw)), regenerated inside the HIP kernels and never stored; a layer that has a stream uses the same stated mask in its CPU
`forward` in place of nn.Dropout.  A layer without a stream (built by hand) keeps nn.Dropout on the CPU and is refused on the device.

Out of scope, each a NotImplementedError: `inject_trainable_lora_extended` (it builds its Linears with dropout 0.1 on the [M, N] branch and
LoraInjectedConv2d layers), dropout_p > 0 in training mode on a layer that was not injected with a dropout stream, `LoraInjectedConv2d`,
`set_selector_from_diag`, the multi-view UNet and the text tower.
"""
import numpy as np
import torch
import torch.nn as nn

UNET_DEFAULT_TARGET_REPLACE = {"CrossAttention", "Attention", "MemoryEfficientCrossAttention", "GEGLU"}
UNET_EXTENDED_TARGET_REPLACE = {"ResnetBlock2D", "CrossAttention", "Attention", "MemoryEfficientCrossAttention", "GEGLU"}
TEXT_ENCODER_DEFAULT_TARGET_REPLACE = {"CLIPAttention"}
TEXT_ENCODER_EXTENDED_TARGET_REPLACE = {"CLIPAttention"}
DEFAULT_TARGET_REPLACE = UNET_DEFAULT_TARGET_REPLACE
EMBED_FLAG = "<embed>"
MAX_RANK = 64      # the HIP LoRA kernels run at a padded rank of 32 or 64 (leftrefill_amd.ops.lora_pad_rank)


class LoraDropoutState:
    """The dropout state of one injected model: `seed` (64 bits) and `draw`, the 32-bit count of training forwards so far (it wraps).
    The UNet advances `draw` once per grad-enabled training forward that has a live dropout layer and hands the number it took down to
    every layer's node; checkpoints carry the pair."""

    def __init__(self, seed=None, draw=0):
        self.seed = int(torch.initial_seed() if seed is None else seed) & (2 ** 64 - 1)
        self.draw = int(draw) & 0xFFFFFFFF

    def take(self):
        """The draw number of this forward; the counter moves on."""
        d = self.draw
        self.draw = (d + 1) & 0xFFFFFFFF
        return d

    def state_dict(self):
        return {"seed": self.seed, "draw": self.draw}

    def load_state_dict(self, sd):
        self.seed, self.draw = int(sd["seed"]) & (2 ** 64 - 1), int(sd["draw"]) & 0xFFFFFFFF


class LoraInjectedLinear(nn.Module):
    """y = linear(x) + scale * dropout(lora_up(selector(lora_down(x)))); the two factors are fp32 masters."""

    def __init__(self, in_features, out_features, bias=False, r=4, dropout_p=0.1, scale=1.0):
        super().__init__()
        widest = min(in_features, out_features)
        if r > widest:
            raise ValueError(f"LoRA rank {r} exceeds the layer's smaller dimension {widest}")
        if not 1 <= r <= MAX_RANK:
            raise ValueError(f"LoRA rank {r} is not supported: the HIP LoRA kernels take 1 <= r <= {MAX_RANK} (the factors are zero-padded "
                             "to the rank granule 32)")
        self.r, self.scale = r, scale
        self.linear = nn.Linear(in_features, out_features, bias)
        self.lora_down = nn.Linear(in_features, r, bias=False)
        self.dropout = nn.Dropout(dropout_p)
        self.lora_up = nn.Linear(r, out_features, bias=False)
        self.selector = nn.Identity()
        self.drop_stream = self.drop_state = None      # set by inject_trainable_lora: the layer's stream id and the model's LoraDropoutState
        with torch.no_grad():
            self.lora_down.weight.normal_(mean=0.0, std=1.0 / r)
            self.lora_up.weight.zero_()

    def forward(self, input):
        if input.is_cuda:
            raise RuntimeError("LoraInjectedLinear runs on the device through UNetModel's packed routes only (no BLAS path in this package)")
        low_rank = self.lora_up(self.selector(self.lora_down(input)))
        if self.dropout_live():
            # the stated mask at the state's current draw (row = the input's row in [M, K] order), not nn.Dropout's generator
            from leftrefill_amd import lora_dropout
            p, n = self.dropout.p, low_rank.shape[-1]
            keep = lora_dropout.keep_mask(self.drop_state.seed, self.drop_stream, self.drop_state.draw, low_rank.numel() // n, n, p)
            keep = torch.from_numpy(np.ascontiguousarray(keep)).reshape(low_rank.shape)
            low_rank = torch.where(keep, low_rank * lora_dropout.inv_keep(p), torch.zeros((), dtype=low_rank.dtype))
            return self.linear(input) + self.scale * low_rank
        return self.linear(input) + self.scale * self.dropout(low_rank)

    def dropout_live(self):
        """Training with p > 0 on a layer that inject_trainable_lora gave a dropout stream: the counter-based mask applies."""
        return self.training and self.dropout.p > 0 and self.drop_stream is not None and self.drop_state is not None

    def realize_as_lora(self):
        """(scale * up, down): the two matrices whose product is what the layer adds to its base weight."""
        return self.scale * self.lora_up.weight.data, self.lora_down.weight.data

    def set_selector_from_diag(self, diag):
        raise NotImplementedError("set_selector_from_diag: the HIP LoRA route has no selector matrix between the two factors")


class LoraInjectedConv2d(nn.Module):
    def __init__(self, *args, **kwargs):
        raise NotImplementedError("LoraInjectedConv2d: this build computes no convolution weight gradients (LoRA covers the attention and "
                                  "GEGLU Linears)")


def _find_children(model, search_class=(nn.Linear,)):
    """(parent, child name, child) for every direct child of a searched class, anywhere in the model."""
    wanted = tuple(search_class)
    for owner in model.modules():
        yield from ((owner, leaf, child) for leaf, child in owner.named_children() if isinstance(child, wanted))


def _find_modules_v2(model, ancestor_class=None, search_class=(nn.Linear,), exclude_children_of=(LoraInjectedLinear, LoraInjectedConv2d)):
    """(direct parent, name in that parent, module) for every module of a searched class that lies at any depth below -- or is -- a module
    whose class name is in `ancestor_class` (None: below any module), except the children of the excluded classes.  A module below two
    matching ancestors is reported once per ancestor."""
    wanted, barred = tuple(search_class), tuple(exclude_children_of or ())
    for ancestor in model.modules():
        if ancestor_class is not None and type(ancestor).__name__ not in ancestor_class:
            continue
        below = dict(ancestor.named_modules())                 # qualified name -> module ("" is the ancestor itself)
        for qualified, module in below.items():
            if isinstance(module, wanted):
                owner_name, _, leaf = qualified.rpartition(".")
                owner = below[owner_name]
                if not isinstance(owner, barred):
                    yield owner, leaf, module


_find_modules = _find_modules_v2


def _check_target(model, target_replace_module):
    if set(target_replace_module) & (TEXT_ENCODER_DEFAULT_TARGET_REPLACE | TEXT_ENCODER_EXTENDED_TARGET_REPLACE):
        raise NotImplementedError("LoRA on the text tower is not implemented: its weights receive no gradients in this build")
    if "ResnetBlock2D" in target_replace_module:
        raise NotImplementedError("the extended target set needs LoraInjectedConv2d, which is not implemented")
    for m in model.modules():
        if type(m).__name__ in ("FrozenOpenCLIPEmbedder", "PromptCLIPEmbedder", "NVSCLIPEmbedder", "CLIP"):
            raise NotImplementedError("LoRA on the text tower is not implemented: its weights receive no gradients in this build")
        chk = getattr(m, "_lora_check", None)
        if chk is not None:
            chk()


def inject_trainable_lora(model, target_replace_module=DEFAULT_TARGET_REPLACE, r=4, loras=None, verbose=False, dropout_p=0.0, scale=1.0):
    """Wrap every nn.Linear below the target classes in a LoraInjectedLinear that keeps it as its `linear` (same Parameters, so a loaded
    checkpoint stays loaded).  loras: path of a saved [up, down, up, down, ...] list to start from.  dropout_p: the rate of the dropout on
    the low-rank branch; layer i (the order of the returned names) draws its mask from stream i of the model's LoraDropoutState.  Returns ([up.parameters(),
    down.parameters(), ...] layer by layer, [name of each wrapped child in its parent])."""
    _check_target(model, target_replace_module)
    saved = iter(torch.load(loras)) if loras is not None else None
    sites = list(_find_modules(model, target_replace_module, search_class=[nn.Linear]))      # found first, swapped after: the walk sees one tree
    param_iters, names = [], []
    state = model.__dict__.get("_lora_dropout")
    if state is None:
        state = model.__dict__["_lora_dropout"] = LoraDropoutState()      # (a plain attribute: no module, no buffer, no state_dict key)
    first = sum(1 for m in model.modules() if isinstance(m, LoraInjectedLinear) and m.drop_stream is not None)
    for i, (owner, leaf, base) in enumerate(sites):
        layer = LoraInjectedLinear(base.in_features, base.out_features, base.bias is not None, r=r, dropout_p=dropout_p, scale=scale)
        layer.linear = base
        layer.drop_stream, layer.drop_state = first + i, state
        layer.to(base.weight.device)      # (the factors stay fp32 whatever the base weight's dtype: their gradients arrive in fp32)
        if saved is not None:
            layer.lora_up.weight, layer.lora_down.weight = next(saved), next(saved)
        for factor in (layer.lora_up, layer.lora_down):
            factor.weight.requires_grad_(True)
            param_iters.append(factor.parameters())
        setattr(owner, leaf, layer)
        names.append(leaf)
        if verbose:
            print(f"LoRA: wrapped {type(owner).__name__}.{leaf} {tuple(base.weight.shape)} at rank {r}")
    for m in model.modules():
        hook = getattr(m, "_on_lora_injected", None)
        if hook is not None:
            hook()
    return param_iters, names


def lora_dropout_state(model):
    """The LoraDropoutState inject_trainable_lora put on `model`, or None."""
    return model.__dict__.get("_lora_dropout")


def inject_trainable_lora_extended(model, target_replace_module=UNET_EXTENDED_TARGET_REPLACE, r=4, loras=None, verbose=False, scale=1.0):
    raise NotImplementedError("lora_type 'extended': it builds the injected Linears with the default dropout_p = 0.1 on the [M, N] branch and "
                              "LoraInjectedConv2d layers in the ResBlocks; neither is implemented by the HIP path")


def extract_lora_ups_down(model, target_replace_module=DEFAULT_TARGET_REPLACE):
    """[(lora_up, lora_down)] of the injected layers below the target classes, in injection order; ValueError when there is none."""
    pairs = [(layer.lora_up, layer.lora_down) for _, _, layer in _find_modules(model, target_replace_module, search_class=[LoraInjectedLinear])]
    if not pairs:
        raise ValueError("No LoRA layer below the target classes: inject_trainable_lora has not run on this model")
    return pairs
