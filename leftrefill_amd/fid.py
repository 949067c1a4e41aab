"""Frechet Inception Distance of the evaluation harness: the fourth image metric of the paper's tables, next to PSNR / SSIM
(evalglue.device_metrics) and LPIPS (evalglue.LPIPSAlex).  The reference computes none of it: its harnesses write every prediction to
disk "for fid metric" (test_inpainting.py --save_single, test_multiview_inpainting.py) and leave the number to the pytorch-fid package.

This module restates the PUBLISHED algorithm (Heusel et al. 2017; the pool3 features of pytorch-fid's `InceptionV3`) and is
**parity-unpinned**: pytorch-fid, torchvision and the Inception weights are absent from this tree and no weights ship.  The float64
form of `FIDInception` is the yardstick of the kernels (tests/test_gpu_fid.py), not pytorch-fid.

  image      8-bit RGB / 255, F.interpolate(mode='bilinear', align_corners=False) to 299 x 299 without antialiasing, 2 x - 1
  network    `GRAPH`: the stem, Mixed_5b .. Mixed_7c, the mean over the 8 x 8 map -> 2048 features.  ONE table drives the eager module
             (`FIDInception.forward` interprets it) and the device route (`FID_PROGRAM`, the int32 rows lr_fid_run interprets)
  statistics mu = mean(f), sigma = cov(f) with divisor n - 1 from float64 sums (`FIDStats`, `stats_from_sums`)
  distance   |mu1 - mu2|^2 + tr(s1) + tr(s2) - 2 tr(sqrtm(s1 s2)) on the host with scipy (`frechet_distance`)
`DeviceFID` runs the network on the HIP kernels of csrc/inception.hip, `HostFID` through the eager module in fp32 and numpy."""
import numpy as np
import torch
import torch.nn.functional as F

SIZE = 299          # side of the network's input
FEATURES = 2048
BN_EPS = 1e-3

# words of a program row and the op codes (LR_FID_* of include/leftrefill_hip.h)
ROW_WORDS = 24
(W_OP, W_SRC_OFF, W_SRC_LD, W_SRC_C0, W_DST_OFF, W_DST_LD, W_DST_C0, W_HIN, W_WIN, W_CIN, W_HOUT, W_WOUT, W_COUT, W_KH, W_KW, W_STRIDE,
 W_PH, W_PW, W_W_OFF, W_B_OFF, W_KPAD) = range(21)
OP_CONV, OP_MAXPOOL_S2, OP_MAXPOOL_S1, OP_AVGPOOL_S1 = 1, 2, 3, 4
SRC_U8 = 3          # LR_FID_SRC_U8
K_STEP = 64


def _pair(v):
    return tuple(v) if isinstance(v, (tuple, list)) else (v, v)


class _Graph:
    """The network as a list of ops on named NHWC tensors.  A conv / pool writes the channel range [c0, c0 + cout) of its destination,
    so a block's concat is a tensor several ops write into."""

    def __init__(self):
        self.tensors = {"input": (SIZE, SIZE, 3)}      # name -> (H, W, C)
        self.ops = []

    def _dst(self, dst, h, w, c):
        if dst in self.tensors:
            assert self.tensors[dst] == (h, w, c), (dst, self.tensors[dst], (h, w, c))
        self.tensors[dst] = (h, w, c)

    def conv(self, name, src, dst, cout, k=1, stride=1, pad=0, c0=0, ctot=None):
        (kh, kw), (ph, pw) = _pair(k), _pair(pad)
        h, w, cin = self.tensors[src]
        ho, wo = (h + 2 * ph - kh) // stride + 1, (w + 2 * pw - kw) // stride + 1
        self._dst(dst, ho, wo, ctot or cout)
        self.ops.append(dict(op=OP_CONV, name=name, src=src, dst=dst, c0=c0, cin=cin, cout=cout, kh=kh, kw=kw, stride=stride, ph=ph, pw=pw))

    def pool(self, op, src, dst, c0=0, ctot=None):
        h, w, c = self.tensors[src]
        ho, wo = ((h - 3) // 2 + 1, (w - 3) // 2 + 1) if op == OP_MAXPOOL_S2 else (h, w)
        self._dst(dst, ho, wo, ctot or c)
        self.ops.append(dict(op=op, name=None, src=src, dst=dst, c0=c0, cin=c, cout=c))


def _build_graph():
    g = _Graph()
    g.conv("Conv2d_1a_3x3", "input", "s1", 32, 3, 2)
    g.conv("Conv2d_2a_3x3", "s1", "s2", 32, 3)
    g.conv("Conv2d_2b_3x3", "s2", "s3", 64, 3, pad=1)
    g.pool(OP_MAXPOOL_S2, "s3", "s4")
    g.conv("Conv2d_3b_1x1", "s4", "s5", 80)
    g.conv("Conv2d_4a_3x3", "s5", "s6", 192, 3)
    g.pool(OP_MAXPOOL_S2, "s6", "s7")
    x = "s7"

    def block_a(n, x, pf):
        t = 224 + pf
        g.conv(n + ".branch1x1", x, n, 64, ctot=t)
        g.conv(n + ".branch5x5_1", x, n + ".a", 48)
        g.conv(n + ".branch5x5_2", n + ".a", n, 64, 5, pad=2, c0=64, ctot=t)
        g.conv(n + ".branch3x3dbl_1", x, n + ".b", 64)
        g.conv(n + ".branch3x3dbl_2", n + ".b", n + ".c", 96, 3, pad=1)
        g.conv(n + ".branch3x3dbl_3", n + ".c", n, 96, 3, pad=1, c0=128, ctot=t)
        g.pool(OP_AVGPOOL_S1, x, n + ".p")
        g.conv(n + ".branch_pool", n + ".p", n, pf, c0=224, ctot=t)
        return n

    def block_b(n, x):
        g.conv(n + ".branch3x3", x, n, 384, 3, 2, ctot=768)
        g.conv(n + ".branch3x3dbl_1", x, n + ".a", 64)
        g.conv(n + ".branch3x3dbl_2", n + ".a", n + ".b", 96, 3, pad=1)
        g.conv(n + ".branch3x3dbl_3", n + ".b", n, 96, 3, 2, c0=384, ctot=768)
        g.pool(OP_MAXPOOL_S2, x, n, c0=480, ctot=768)
        return n

    def block_c(n, x, c7):
        g.conv(n + ".branch1x1", x, n, 192, ctot=768)
        g.conv(n + ".branch7x7_1", x, n + ".a", c7)
        g.conv(n + ".branch7x7_2", n + ".a", n + ".b", c7, (1, 7), pad=(0, 3))
        g.conv(n + ".branch7x7_3", n + ".b", n, 192, (7, 1), pad=(3, 0), c0=192, ctot=768)
        g.conv(n + ".branch7x7dbl_1", x, n + ".c", c7)
        g.conv(n + ".branch7x7dbl_2", n + ".c", n + ".d", c7, (7, 1), pad=(3, 0))
        g.conv(n + ".branch7x7dbl_3", n + ".d", n + ".e", c7, (1, 7), pad=(0, 3))
        g.conv(n + ".branch7x7dbl_4", n + ".e", n + ".f", c7, (7, 1), pad=(3, 0))
        g.conv(n + ".branch7x7dbl_5", n + ".f", n, 192, (1, 7), pad=(0, 3), c0=384, ctot=768)
        g.pool(OP_AVGPOOL_S1, x, n + ".p")
        g.conv(n + ".branch_pool", n + ".p", n, 192, c0=576, ctot=768)
        return n

    def block_d(n, x):
        g.conv(n + ".branch3x3_1", x, n + ".a", 192)
        g.conv(n + ".branch3x3_2", n + ".a", n, 320, 3, 2, ctot=1280)
        g.conv(n + ".branch7x7x3_1", x, n + ".b", 192)
        g.conv(n + ".branch7x7x3_2", n + ".b", n + ".c", 192, (1, 7), pad=(0, 3))
        g.conv(n + ".branch7x7x3_3", n + ".c", n + ".d", 192, (7, 1), pad=(3, 0))
        g.conv(n + ".branch7x7x3_4", n + ".d", n, 192, 3, 2, c0=320, ctot=1280)
        g.pool(OP_MAXPOOL_S2, x, n, c0=512, ctot=1280)
        return n

    def block_e(n, x, pool):
        g.conv(n + ".branch1x1", x, n, 320, ctot=2048)
        g.conv(n + ".branch3x3_1", x, n + ".a", 384)
        g.conv(n + ".branch3x3_2a", n + ".a", n, 384, (1, 3), pad=(0, 1), c0=320, ctot=2048)
        g.conv(n + ".branch3x3_2b", n + ".a", n, 384, (3, 1), pad=(1, 0), c0=704, ctot=2048)
        g.conv(n + ".branch3x3dbl_1", x, n + ".b", 448)
        g.conv(n + ".branch3x3dbl_2", n + ".b", n + ".c", 384, 3, pad=1)
        g.conv(n + ".branch3x3dbl_3a", n + ".c", n, 384, (1, 3), pad=(0, 1), c0=1088, ctot=2048)
        g.conv(n + ".branch3x3dbl_3b", n + ".c", n, 384, (3, 1), pad=(1, 0), c0=1472, ctot=2048)
        g.pool(pool, x, n + ".p")
        g.conv(n + ".branch_pool", n + ".p", n, 192, c0=1856, ctot=2048)
        return n

    x = block_a("Mixed_5b", x, 32)
    x = block_a("Mixed_5c", x, 64)
    x = block_a("Mixed_5d", x, 64)
    x = block_b("Mixed_6a", x)
    for n, c7 in (("Mixed_6b", 128), ("Mixed_6c", 160), ("Mixed_6d", 160), ("Mixed_6e", 192)):
        x = block_c(n, x, c7)
    x = block_d("Mixed_7a", x)
    x = block_e("Mixed_7b", x, OP_AVGPOOL_S1)      # pytorch-fid: 7b averages without the padding, 7c takes the maximum
    x = block_e("Mixed_7c", x, OP_MAXPOOL_S1)
    g.output = x
    return g


GRAPH = _build_graph()
CONVS = [o for o in GRAPH.ops if o["op"] == OP_CONV]      # the 94 BasicConv2d in execution order


def stored_channels(c):
    """Channels a tensor of c channels is stored with: the image's 3 become 4, every other count is a multiple of 8 already."""
    return 4 if c == 3 else c


def _plan():
    """Arena offsets (halves per image), weight / bias offsets and the program.  A tensor lives from the first op that writes it to the
    last that reads it; it gets the lowest offset (a multiple of 8) that no tensor alive at the same time occupies."""
    ops, tensors = GRAPH.ops, GRAPH.tensors
    life = {"input": [-1, -1]}
    for i, o in enumerate(ops):
        life.setdefault(o["dst"], [i, i])[1] = i
        life[o["src"]][1] = i
    life[GRAPH.output][1] = len(ops)      # the head reads it
    size = {n: -(-h * w * stored_channels(c) // 8) * 8 for n, (h, w, c) in tensors.items()}
    off, placed = {}, []
    for n in sorted(life, key=lambda n: life[n][0]):
        at = 0
        for m in sorted((m for m in placed if life[m][0] <= life[n][1] and life[n][0] <= life[m][1]), key=lambda m: off[m]):
            if at + size[n] <= off[m]:
                break
            at = max(at, off[m] + size[m])
        off[n] = at
        placed.append(n)
    arena = max(off[n] + size[n] for n in off)
    rows = np.zeros((len(ops), ROW_WORDS), dtype=np.int32)
    w_off = b_off = 0
    for i, o in enumerate(ops):
        (hi, wi, ci), (ho, wo, ct) = tensors[o["src"]], tensors[o["dst"]]
        r = rows[i]
        r[W_OP], r[W_SRC_OFF], r[W_SRC_LD], r[W_SRC_C0] = o["op"], off[o["src"]], stored_channels(ci), 0
        r[W_DST_OFF], r[W_DST_LD], r[W_DST_C0] = off[o["dst"]], stored_channels(ct), o["c0"]
        r[W_HIN], r[W_WIN], r[W_CIN], r[W_HOUT], r[W_WOUT], r[W_COUT] = hi, wi, stored_channels(ci), ho, wo, o["cout"]
        if o["op"] == OP_CONV:
            kpad = -(-o["kh"] * o["kw"] * stored_channels(ci) // K_STEP) * K_STEP
            r[W_KH], r[W_KW], r[W_STRIDE], r[W_PH], r[W_PW] = o["kh"], o["kw"], o["stride"], o["ph"], o["pw"]
            r[W_W_OFF], r[W_B_OFF], r[W_KPAD] = w_off, b_off, kpad
            w_off += o["cout"] * kpad
            b_off += o["cout"]
    ho, wo, co = tensors[GRAPH.output]
    return rows, dict(arena_halfs=arena, input_off=off["input"], output_off=off[GRAPH.output], output_hw=ho * wo, output_c=co,
                      wt_halfs=w_off, bias_floats=b_off)


FID_PROGRAM, FID_LAYOUT = _plan()


class _EvalBatchNorm(torch.nn.Module):
    """The four tensors of an inference BatchNorm2d under its names; a file's `num_batches_tracked` has no use here and is ignored."""

    def __init__(self, c):
        super().__init__()
        self.weight, self.bias = torch.nn.Parameter(torch.ones(c)), torch.nn.Parameter(torch.zeros(c))
        self.register_buffer("running_mean", torch.zeros(c))
        self.register_buffer("running_var", torch.ones(c))


class BasicConv2d(torch.nn.Module):
    """conv without bias, BatchNorm (eps 1e-3, running statistics), ReLU."""

    def __init__(self, cin, cout, k, stride, pad):
        super().__init__()
        self.conv = torch.nn.Conv2d(cin, cout, k, stride, pad, bias=False)
        self.bn = _EvalBatchNorm(cout)

    def forward(self, x):
        return F.relu(F.batch_norm(self.conv(x), self.bn.running_mean, self.bn.running_var, self.bn.weight, self.bn.bias, False, 0.0, BN_EPS))


def _pool_eager(op, x):
    if op == OP_MAXPOOL_S2:
        return F.max_pool2d(x, 3, 2)
    if op == OP_MAXPOOL_S1:
        return F.max_pool2d(x, 3, 1, 1)
    return F.avg_pool2d(x, 3, 1, 1, count_include_pad=False)


def to_uint8(x):
    """What the reference's harness would have saved of an image in [-1, 1]: trunc((clamp(x, -1, 1) + 1) / 2 * 255) in fp32, uint8."""
    return ((x.float().clamp(-1, 1) + 1) / 2 * 255).to(torch.uint8)


def preprocess(u8_nhwc, dtype=torch.float32, size=SIZE):
    """uint8 [N, H, W, 3] -> [N, 3, size, size] in [-1, 1]: / 255, bilinear (align_corners False, no antialiasing), 2 x - 1."""
    x = u8_nhwc.permute(0, 3, 1, 2).to(dtype) / 255
    x = F.interpolate(x, size=(size, size), mode="bilinear", align_corners=False)
    return 2 * x - 1


def bilinear_taps(n_in, n_out):
    """The input kernel's taps along one axis, in its float64 arithmetic: f = max(0, (d + 0.5) n_in / n_out - 0.5), i0 = min(int(f),
    n_in - 1), i1 = min(i0 + 1, n_in - 1), l = f - i0.  Returns (i0, i1, l)."""
    d = np.arange(n_out, dtype=np.float64)
    f = np.maximum((d + 0.5) * (float(n_in) / float(n_out)) - 0.5, 0.0)
    i0 = np.minimum(f.astype(np.int64), n_in - 1)
    return i0, np.minimum(i0 + 1, n_in - 1), f - i0


def resize_numpy(u8_nhwc, size=SIZE):
    """The input kernel's image in float64 numpy: uint8 [N, H, W, 3] -> [N, size, size, 3] = 2 bilinear(u8 / 255) - 1 on `bilinear_taps`."""
    p = np.asarray(u8_nhwc, dtype=np.float64) / 255
    y0, y1, ly = bilinear_taps(p.shape[1], size)
    x0, x1, lx = bilinear_taps(p.shape[2], size)
    ly, lx = ly[None, :, None, None], lx[None, None, :, None]
    top = (1 - lx) * p[:, y0][:, :, x0] + lx * p[:, y0][:, :, x1]
    bot = (1 - lx) * p[:, y1][:, :, x0] + lx * p[:, y1][:, :, x1]
    return 2 * ((1 - ly) * top + ly * bot) - 1


class FIDInception(torch.nn.Module):
    """pytorch-fid's `InceptionV3` up to pool3 under torchvision's `Inception3` names (`Conv2d_1a_3x3.conv.weight`,
    `Mixed_5b.branch1x1.bn.running_mean`, `Mixed_7c.branch3x3dbl_3b.conv.weight`, ...), so a user's pytorch-fid weight file loads.
    forward: [N, 3, 299, 299] in [-1, 1] (see `preprocess`) -> [N, 2048], in the dtype of the module; float64 is the yardstick.
    Parity-unpinned (module docstring); no weights ship: `load_weights` takes the user's state dict, `seeded_state_dict` gives test
    weights."""

    def __init__(self):
        super().__init__()
        for o in CONVS:
            parent = self
            *path, leaf = o["name"].split(".")
            for p in path:
                if not hasattr(parent, p):
                    parent.add_module(p, torch.nn.Module())
                parent = getattr(parent, p)
            parent.add_module(leaf, BasicConv2d(o["cin"], o["cout"], (o["kh"], o["kw"]), o["stride"], (o["ph"], o["pw"])))
        self.loaded = False
        for p in self.parameters():
            p.requires_grad_(False)
        self.eval()

    def layer(self, name):
        return self.get_submodule(name)

    def load_weights(self, sd):
        """A state dict of torchvision's Inception3 / pytorch-fid's FID network; `fc.*` and `AuxLogits.*` are ignored.  KeyError names
        what is missing."""
        own = self.state_dict()
        missing = [k for k in own if k not in sd]
        if missing:
            raise KeyError("FID Inception weights missing: " + ", ".join(missing))
        self.load_state_dict({k: sd[k] for k in own if k in sd}, strict=False)
        self.loaded = True
        return self

    def trace(self, x):
        """Every tensor of GRAPH as NCHW, by name."""
        t = {"input": x}
        for o in GRAPH.ops:
            y = self.layer(o["name"])(t[o["src"]]) if o["op"] == OP_CONV else _pool_eager(o["op"], t[o["src"]])
            if o["dst"] not in t:
                h, w, c = GRAPH.tensors[o["dst"]]
                t[o["dst"]] = x.new_zeros(x.shape[0], c, h, w)
            t[o["dst"]][:, o["c0"]:o["c0"] + o["cout"]] = y
        return t

    @torch.no_grad()
    def forward(self, x):
        if not self.loaded:
            raise RuntimeError("FIDInception has no weights: call load_weights(state_dict) first")
        return self.trace(x)[GRAPH.output].mean((2, 3))


def seeded_state_dict(seed=0):
    """Test weights: He-normal conv weights, BN weight 1, bias 0.05 N(0, 1), running mean 0, running variance 1."""
    g = torch.Generator().manual_seed(seed)
    sd = {}
    for o in CONVS:
        fan_in = o["cin"] * o["kh"] * o["kw"]
        n = o["name"]
        sd[n + ".conv.weight"] = torch.randn(o["cout"], o["cin"], o["kh"], o["kw"], generator=g) * (2.0 / fan_in) ** 0.5
        sd[n + ".bn.weight"] = torch.ones(o["cout"])
        sd[n + ".bn.bias"] = 0.05 * torch.randn(o["cout"], generator=g)
        sd[n + ".bn.running_mean"] = torch.zeros(o["cout"])
        sd[n + ".bn.running_var"] = torch.ones(o["cout"])
    return sd


def pack_fid(module, exact=False):
    """FIDInception (weights loaded) -> {"wt", "bias"}: the blobs FID_PROGRAM's W_OFF / B_OFF point into, on the module's device.
    BatchNorm is folded in fp32: scale = gamma / sqrt(var + 1e-3), w * scale rounded ONCE to fp16, bias = beta - mean * scale kept fp32.
    wt of a layer: [Cout][Kpad], K index (ky * kw + kx) * Cs + c with Cs the stored channels (3 -> 4), zeros from kh kw Cs to Kpad.
    exact: fold in float64 and keep float64 blobs (the CPU test's real-arithmetic statement of the same layout)."""
    if not module.loaded:
        raise RuntimeError("pack_fid: the module has no weights")
    ft, wt_t = (torch.float64, torch.float64) if exact else (torch.float32, torch.float16)
    dev = module.layer(CONVS[0]["name"]).conv.weight.device
    wt = torch.zeros(FID_LAYOUT["wt_halfs"], device=dev, dtype=wt_t)
    bias = torch.zeros(FID_LAYOUT["bias_floats"], device=dev, dtype=ft)
    for r, o in zip(FID_PROGRAM[FID_PROGRAM[:, W_OP] == OP_CONV], CONVS):
        m = module.layer(o["name"])
        scale = m.bn.weight.detach().to(ft) / torch.sqrt(m.bn.running_var.detach().to(ft) + BN_EPS)
        w = (m.conv.weight.detach().to(ft) * scale.view(-1, 1, 1, 1)).permute(0, 2, 3, 1)      # [Cout, kh, kw, Cin]
        cs, kpad, co = int(r[W_CIN]), int(r[W_KPAD]), o["cout"]
        blk = torch.zeros(co, o["kh"] * o["kw"], cs, device=dev, dtype=wt_t)
        blk[:, :, :o["cin"]] = w.reshape(co, -1, o["cin"]).to(wt_t)
        dst = wt[int(r[W_W_OFF]):int(r[W_W_OFF]) + co * kpad].view(co, kpad)
        dst[:, :blk.shape[1] * cs] = blk.reshape(co, -1)
        bias[int(r[W_B_OFF]):int(r[W_B_OFF]) + co] = m.bn.bias.detach().to(ft) - m.bn.running_mean.detach().to(ft) * scale
    return {"wt": wt, "bias": bias}


def fid_features(images, packed, *, x0=0, Wc=None, origin=None, mask=None):
    """The 2048 pool3 features of a batch on the device: fp32 [N, 2048], nothing read back.  images: uint8 [N, H, W, 3], or
    [N, 3, H, W] fp32 / fp16 / bf16 in [-1, 1], which is truncated to 8 bits first (with mask [N, 1, H, W] and origin [N, 3, H, W]:
    after the composite images * mask + origin * (1 - mask)); columns [x0, x0 + Wc) are the image.  A list of such
    (images, x0, Wc, origin, mask) tuples runs as ONE batch.  Launches: one per source, len(FID_PROGRAM), one for the head."""
    from . import ops
    sources = images if isinstance(images, list) else [(images, x0, Wc, origin, mask)]
    counts = [s[0].shape[0] for s in sources]
    B, dev = sum(counts), sources[0][0].device
    arena = torch.empty(B * FID_LAYOUT["arena_halfs"], device=dev, dtype=torch.float16)
    at = FID_LAYOUT["input_off"] * B
    for (img, sx0, sWc, sorigin, smask), n in zip(sources, counts):
        ops.fid_input(img, arena[at:at + n * SIZE * SIZE * 4], SIZE, x0=sx0, Wc=sWc, origin=sorigin, mask=smask)
        at += n * SIZE * SIZE * 4
    ops.fid_run(FID_PROGRAM, B, arena, packed["wt"], packed["bias"])
    feats = torch.empty(B, FID_LAYOUT["output_c"], device=dev, dtype=torch.float32)
    ops.fid_head(arena[FID_LAYOUT["output_off"] * B:], B, FID_LAYOUT["output_hw"], FID_LAYOUT["output_c"], FID_LAYOUT["output_c"], feats)
    return feats


class FIDStats:
    """The float64 sum, Gram matrix and count of one set's features.  `update` adds device features with the statistics kernel (sums
    stay on the device), `update_host` adds host features with numpy; one instance uses one of the two."""

    def __init__(self, dim=FEATURES):
        self.dim, self.n = dim, 0
        self.sum = self.gram = None

    def update(self, feats):
        from . import ops
        assert feats.is_cuda and feats.dtype == torch.float32 and feats.dim() == 2 and feats.shape[1] == self.dim
        if self.sum is None:
            self.sum = torch.zeros(self.dim, device=feats.device, dtype=torch.float64)
            self.gram = torch.zeros(self.dim, self.dim, device=feats.device, dtype=torch.float64)
        ops.fid_accumulate(feats.contiguous(), self.sum, self.gram)
        self.n += feats.shape[0]

    def update_host(self, feats):
        f = np.asarray(feats.detach().cpu() if torch.is_tensor(feats) else feats, dtype=np.float64)
        if self.sum is None:
            self.sum, self.gram = np.zeros(self.dim), np.zeros((self.dim, self.dim))
        self.sum += f.sum(0)
        self.gram += f.T @ f
        self.n += f.shape[0]

    def sums(self):
        """(sum, gram, n) as float64 numpy arrays: the one read-back of a device instance."""
        if self.sum is None:
            return np.zeros(self.dim), np.zeros((self.dim, self.dim)), 0
        if torch.is_tensor(self.sum):
            return self.sum.cpu().numpy(), self.gram.cpu().numpy(), self.n
        return self.sum, self.gram, self.n


def stats_from_sums(s, gram, n):
    """mu = s / n and the unbiased covariance (gram - n mu mu^T) / (n - 1), float64."""
    if n < 2:
        raise ValueError(f"FID statistics need at least 2 samples, got {n}")
    s, gram = np.asarray(s, dtype=np.float64), np.asarray(gram, dtype=np.float64)
    mu = s / n
    return mu, (gram - n * np.outer(mu, mu)) / (n - 1)


def frechet_distance(mu1, sigma1, mu2, sigma2, eps=1e-6):
    """|mu1 - mu2|^2 + tr(s1) + tr(s2) - 2 tr(sqrtm(s1 s2)) in float64.  A root that is not finite is retried with eps on both
    diagonals; an imaginary part whose diagonal is within 1e-3 of zero is dropped, a larger one raises ValueError."""
    from scipy import linalg
    mu1, mu2 = np.atleast_1d(np.asarray(mu1, dtype=np.float64)), np.atleast_1d(np.asarray(mu2, dtype=np.float64))
    sigma1, sigma2 = np.atleast_2d(np.asarray(sigma1, dtype=np.float64)), np.atleast_2d(np.asarray(sigma2, dtype=np.float64))
    assert mu1.shape == mu2.shape and sigma1.shape == sigma2.shape, "statistics of different sizes"
    diff = mu1 - mu2
    covmean = linalg.sqrtm(sigma1.dot(sigma2))
    covmean = covmean[0] if isinstance(covmean, tuple) else covmean
    if not np.isfinite(covmean).all():
        offset = np.eye(sigma1.shape[0]) * eps
        covmean = linalg.sqrtm((sigma1 + offset).dot(sigma2 + offset))
        covmean = covmean[0] if isinstance(covmean, tuple) else covmean
    if np.iscomplexobj(covmean):
        if not np.allclose(np.diagonal(covmean).imag, 0, atol=1e-3):
            raise ValueError(f"frechet_distance: imaginary component {np.max(np.abs(covmean.imag))}")
        covmean = covmean.real
    return float(diff.dot(diff) + np.trace(sigma1) + np.trace(sigma2) - 2 * np.trace(covmean))


def _select(out, mask_nhwc, compose, right_half):
    pred = out["pred"]
    h, w = pred.shape[2], pred.shape[3]
    x0 = w // 2 if (h != w if right_half is None else right_half) else 0
    return pred, out["origin_image"], (mask_nhwc.permute(0, 3, 1, 2) if compose else None), x0


def _select_multiview(out, mask_flat_nhwc, batch_size, global_view_num):
    """evalglue.device_metrics_multiview's mask selection."""
    mask = mask_flat_nhwc.permute(0, 3, 1, 2)
    view_num = int(mask.shape[0] / batch_size)
    if global_view_num == 0:
        global_view_num = view_num
    real_bs = int(mask.shape[0] / global_view_num)
    mask = mask.reshape(real_bs, global_view_num, *mask.shape[1:])[:, 0]
    if mask.shape[3] != mask.shape[2]:
        mask = mask[:, :, :, mask.shape[2]:]
    h, w = out["pred"].shape[2], out["pred"].shape[3]
    return out["pred"], out["origin_image"], mask, (w // 2 if h != w else 0), global_view_num


class _FIDBase:
    """The interface both routes share: two sets -- predictions and originals -- fed batch by batch, one distance at the end."""

    def __init__(self):
        self.net = FIDInception()
        self.reset()

    def reset(self):
        self.pred_stats, self.real_stats = FIDStats(), FIDStats()

    def load_weights(self, sd):
        self.net.load_weights(sd)
        self._packed = None
        return self

    def to(self, device):
        self.net.to(device)
        self._packed = None
        return self

    def cuda(self):
        return self.to("cuda")

    def update(self, out, mask_nhwc, *, compose=True, right_half=None):
        """One batch of what device_metrics scores, same arguments: the composited prediction (right half when h != w) joins the
        predicted set, the same crop of origin_image the real set, both through the 8-bit mapping of the saved PNG."""
        pred, origin, mask, x0 = _select(out, mask_nhwc, compose, right_half)
        self._update_pair(pred, origin, mask, x0)

    def update_multiview(self, out, mask_flat_nhwc, batch_size, global_view_num=0):
        """One batch of what device_metrics_multiview scores, same arguments; returns global_view_num."""
        pred, origin, mask, x0, global_view_num = _select_multiview(out, mask_flat_nhwc, batch_size, global_view_num)
        self._update_pair(pred, origin, mask, x0)
        return global_view_num

    def compute(self):
        s1, g1, n1 = self.pred_stats.sums()
        s2, g2, n2 = self.real_stats.sums()
        if min(n1, n2) < 2:
            raise ValueError(f"FID needs at least 2 images per set, got {n1} and {n2}")
        if not (np.isfinite(s1).all() and np.isfinite(s2).all() and np.isfinite(g1).all() and np.isfinite(g2).all()):
            raise ValueError("FID: a feature sum is not finite")
        return frechet_distance(*stats_from_sums(s1, g1, n1), *stats_from_sums(s2, g2, n2))


class DeviceFID(_FIDBase):
    """FID through the HIP kernels of csrc/inception.hip: per batch the N predictions and the N originals run as ONE batch of 2N
    through the network (`fid_features`), their features are added to float64 sums on the device (`FIDStats.update`); `compute` reads
    the sums back once and takes the distance on the host.  The weights are packed on first use on the device of `to()`."""

    def packed(self):
        if getattr(self, "_packed", None) is None:
            self._packed = pack_fid(self.net)
        return self._packed

    def _split(self, feats, n):
        self.pred_stats.update(feats[:n])
        self.real_stats.update(feats[n:])

    def _update_pair(self, pred, origin, mask, x0):
        if pred.dtype not in (torch.float32, torch.float16, torch.bfloat16):
            pred = pred.float()
        Wc = pred.shape[3] - x0
        origin = origin.float().contiguous()
        self._split(fid_features([(pred, x0, Wc, origin, mask), (origin, x0, Wc, None, None)], self.packed()), pred.shape[0])

    def update_images(self, pred_u8, real_u8):
        """uint8 [N, H, W, 3] predictions and originals (decoded PNGs), on the network's device."""
        self._split(fid_features([(pred_u8, 0, None, None, None), (real_u8, 0, None, None, None)], self.packed()), pred_u8.shape[0])


class HostFID(_FIDBase):
    """The same interface without the kernels: torch composite and 8-bit mapping, `FIDInception` in fp32 on the device the module was
    moved to, statistics in numpy float64.  The route tools/bench_fid.py compares `DeviceFID` against."""

    def _update_pair(self, pred, origin, mask, x0):
        p, o = pred.float(), origin.float()
        if mask is not None:
            m = mask.float()
            p = p * m + o * (1 - m)
        self.update_images(to_uint8(p[:, :, :, x0:]).permute(0, 2, 3, 1), to_uint8(o[:, :, :, x0:]).permute(0, 2, 3, 1))

    def update_images(self, pred_u8, real_u8):
        dev = self.net.layer(CONVS[0]["name"]).conv.weight.device
        n = pred_u8.shape[0]
        feats = self.net(preprocess(torch.cat([pred_u8, real_u8]).to(dev), torch.float32))
        self.pred_stats.update_host(feats[:n])
        self.real_stats.update_host(feats[n:])
