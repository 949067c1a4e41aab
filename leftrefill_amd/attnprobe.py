"""Reference-attention maps: how much every query of a `[reference | target]` canvas looks at the reference half.

LeftRefill's claim is that the frozen inpainting UNet fills the target by attending to the reference.  The reference code meant to
show it through `return_attn` (ddim.py:139-141, 282-300, 334-340) but its score computation is commented out
(multiview_attention.py:333-343).  Here the map is `softmax(Q K^T) @ cols` -- attention with a tiny V that all samples and heads
share -- computed by lr_attention_probe_f16 (csrc/attention_probe.hip) on the very `q|k|v` projection the UNet hands to its attention
kernel; the L x L matrix never exists.

    probe_reference   the formula in float64 torch: the yardstick of the kernel tests
    canvas_columns    the three probe columns of a stitched canvas: reference mass and the reference coordinate it comes from
    AttentionProbe    context manager that records every selected self-attention of a single-view UNet
    fold_cfg          the reference's classifier-free-guidance rule for the maps (ddim.py:338-340)

Deviations from the reference's (dead) path, by design: the maps are head means of the reference MASS (a `[N, h, w]` map per layer, as
the logger draws them), not raw scores; cross-attention (77 keys), the multi-view / NVS-separator UNets, recording inside a replayed
hipGraph and recording under rank sharding are not served (NotImplementedError names them).
"""
import torch

from . import engine, ops


def probe_reference(q, k, cols, B, heads, Nq, Nkv, scale):
    """out[b, i, c] = mean_h sum_j softmax_j(scale q_h[b, i] . k_h[b, j]) cols[j, c] in float64, on the given 16-bit values.

    q [B*Nq, >= heads*64], k [B*Nkv, >= heads*64] (any strides), cols [Nkv, ncols]; returns float64 [B, Nq, ncols]."""
    C = heads * 64
    qd = q[:, :C].to(torch.float64).reshape(B, Nq, heads, 64).permute(0, 2, 1, 3)
    kd = k[:, :C].to(torch.float64).reshape(B, Nkv, heads, 64).permute(0, 2, 1, 3)
    p = torch.softmax(float(scale) * (qd @ kd.transpose(-1, -2)), dim=-1)          # [B, heads, Nq, Nkv]
    return (p @ cols.to(torch.float64)).mean(dim=1)


def canvas_columns(h, w, dtype=torch.float16, device=None):
    """[h*w, 3] probe columns of a stitched canvas whose left half (x < w // 2) is the reference: token t = y*w + x has the row
    [ref, ref*x, ref*y], ref = 1 if x < w // 2 else 0.  Column 0 gives the reference mass; columns 1-2 divided by it the expected
    reference coordinate of a query.  Small integers: exact in fp16 (< 2048) and bf16 (<= 256)."""
    y, x = torch.meshgrid(torch.arange(h, device=device), torch.arange(w, device=device), indexing="ij")
    ref = (x < w // 2).to(torch.float32)
    cols = torch.stack([ref, ref * x, ref * y], dim=-1).reshape(h * w, 3)
    out = cols.to(dtype)
    assert torch.equal(out.to(torch.float32), cols), f"canvas {h} x {w}: coordinates are not exact in {dtype}"
    return out


def fold_cfg(a_uncond, a_cond, scale):
    """The reference's guidance rule for attention scores (ddim.py:338-340): a_uncond + scale (a_cond - a_uncond)."""
    return a_uncond + scale * (a_cond - a_uncond)


def _refuse_sharding(who):
    from . import dist
    if engine.MV_SHARDED:
        raise NotImplementedError(f"{who}: engine.MV_SHARDED (canvas sharding across ranks) is not recorded")
    if dist.split_cfg_active():
        raise NotImplementedError(f"{who}: dist split-CFG (the guidance halves on two ranks) is not recorded")


class AttentionProbe:
    """`with AttentionProbe(unet, layers=None) as probe:` -- while active, every selected self-attention of `unet` also launches
    ops.attention_probe on the same `qkv` with canvas_columns(h_l, w_l), accumulating (beta = 1) into a per-layer fp32
    [N_unet, h_l * w_l, 3] tensor.  Layer index = execution order over input, middle and output blocks; layers: an iterable of
    indices, None = all.  While a probe is active the UNet runs its eager route (the same launches as the captured step without
    the CFG shared prefix), never the captured graph.  Works around any sampler; nothing is read back to the host.

    Refused (NotImplementedError): a multi-view UNet, a grad-enabled forward, engine.MV_SHARDED / dist split-CFG."""

    def __init__(self, unet, layers=None):
        if not hasattr(unet, "_run_plan"):
            raise TypeError("AttentionProbe needs the diffusion UNet (model.model.diffusion_model)")
        self.unet = unet
        self.layers = None if layers is None else frozenset(int(l) for l in layers)
        self._reset()

    def _reset(self):
        self.steps = 0            # UNet calls recorded
        self.num_layers = 0       # self-attentions met in the last UNet call (recorded or not)
        self.canvas = None        # (H, W) of the SpatialTransformer being run (engine.spatial_transformer sets it)
        self._acc = {}            # layer -> fp32 [N, h*w, 3], summed over the steps
        self._hw = {}             # layer -> (h, w)
        self._cols = {}
        self._running = False
        self._call = 0

    # ---- context manager
    def __enter__(self):
        if engine.PROBE is not None:
            raise RuntimeError("an AttentionProbe is already active")
        self.unet.prepare()
        if any(pt.view_num is not None for pt in self.unet._plan["tblocks"]):
            raise NotImplementedError("AttentionProbe: the multi-view UNet (view_num blocks re-arrange the canvases into one sequence) "
                                      "is not recorded")
        _refuse_sharding("AttentionProbe")
        self._reset()
        engine.PROBE = self
        return self

    def __exit__(self, *exc):
        engine.PROBE = None
        self._running = False
        return False

    # ---- called by UNetModel.forward / the engine
    def begin_step(self, unet):
        """A forward of `unet` starts; False when it is not the UNet this probe watches."""
        if unet is not self.unet:
            return False
        if torch.is_grad_enabled():
            raise NotImplementedError("AttentionProbe: a grad-enabled forward is not recorded (wrap the call in torch.no_grad())")
        _refuse_sharding("AttentionProbe")
        self._running, self._call = True, 0
        return True

    def end_step(self, ok):
        self._running = False
        if ok:
            self.steps += 1
            self.num_layers = self._call

    def record(self, qkv, B, heads, L, scale):
        """engine.self_attention / self_then_cross_attention: qkv [B*L, 3 heads*64] is about to go to ops.attention_qkv."""
        if not self._running:
            return
        l = self._call
        self._call += 1
        if self.layers is not None and l not in self.layers:
            return
        h, w = self.canvas
        if h * w != L:
            raise NotImplementedError(f"AttentionProbe: layer {l} attends over {L} tokens on a {h} x {w} canvas (separator tokens of the "
                                      "NVS UNet are not recorded)")
        key = (h, w, qkv.dtype, qkv.device)
        cols = self._cols.get(key)
        if cols is None:
            cols = self._cols[key] = canvas_columns(h, w, qkv.dtype, qkv.device)
        acc = self._acc.get(l)
        if acc is None:
            acc = self._acc[l] = torch.zeros(B, L, 3, device=qkv.device, dtype=torch.float32)
            self._hw[l] = (h, w)
        assert acc.shape[0] == B and self._hw[l] == (h, w), f"layer {l}: the UNet batch or canvas changed under one probe"
        C = heads * 64
        ops.attention_probe(qkv[:, :C], qkv[:, C:2 * C], cols, B, heads, L, L, scale, out=acc, alpha=1.0, beta=1.0)

    # ---- read-outs (device tensors)
    @property
    def recorded(self):
        """The recorded layer indices, ascending."""
        return sorted(self._acc)

    def canvas_of(self, l):
        """(h, w) of the token canvas of recorded layer l."""
        return self._hw[l]

    def raw(self, l):
        """[N_unet, h, w, 3]: the accumulator of layer l (sum over the steps of [mass, mass * x_ref, mass * y_ref])."""
        h, w = self._hw[l]
        return self._acc[l].view(-1, h, w, 3)

    def mass(self, l):
        """[N_unet, h, w]: step mean of the attention mass every query puts on the reference half."""
        return self.raw(l)[..., 0] / max(self.steps, 1)

    def correspondence(self, l):
        """[N_unet, h, w // 2, 2]: for the target half's queries the expected (x, y) they attend to inside the reference half, in
        token units (ratio of the step means of columns 1-2 and column 0, i.e. mass-weighted over the steps); nan where the mass is 0."""
        h, w = self._hw[l]
        r = self.raw(l)[:, :, w // 2:2 * (w // 2), :]
        return mass_to_correspondence(r)


def mass_to_correspondence(raw):
    """[..., 3] (mass, mass*x, mass*y) -> [..., 2] expected (x, y); nan where the mass is 0."""
    m = raw[..., 0:1]
    nan = torch.full_like(raw[..., 1:3], float("nan"))
    return torch.where(m > 0, raw[..., 1:3] / torch.where(m > 0, m, torch.ones_like(m)), nan)
