"""OpenCLIP text tower of the prompt encoder on the HIP kernels.

Replaces `PromptCLIPEmbedder.encode_with_transformer` (reference ldm/modules/encoders/Refill_modules.py:181-201): add the
positional embedding, run the first `n_layers - layer_idx` pre-LN residual attention blocks with the causal mask
(open_clip `ResidualAttentionBlock`: x += out_proj(MHA(ln_1(x))); x += c_proj(gelu(c_fc(ln_2(x))))), then `ln_final`.
Token / special-token embedding lookup and the splice stay torch indexing in the caller (a gather of 77 rows).

The tower is described by duck-typed modules with open_clip's attribute names (`transformer.resblocks[i].{ln_1, attn
(nn.MultiheadAttention: in_proj_weight / in_proj_bias / out_proj), ln_2, mlp.c_fc, mlp.c_proj}`, `positional_embedding`,
`ln_final`), so the packed weights come straight from a loaded open_clip model.  open_clip itself is not in this image:
parity is checked against a PyTorch module of the same published architecture (tests/test_gpu_text.py) -- unpinned by the
reference's own weights / tokenizer.

Training of the prompt tokens (the gradient runs loss -> UNet -> context -> this tower -> the learned token rows) takes the
differentiable sequence of `train_ops` instead: the tower is frozen, only input gradients are produced.  c_fc runs as a plain GEMM
whose output is kept for the GELU backward (lr_gelu_fwd / lr_gelu_bwd); the causal attention saves its log-sum-exp for
lr_attention_causal_bwd.
"""
import torch

from . import engine, ops, train_ops
from .engine import PackedLinear, PackedNorm


class PackedTextBlock:
    def __init__(self, blk):
        self.ln1, self.ln2 = PackedNorm(blk.ln_1), PackedNorm(blk.ln_2)
        self.qkv = PackedLinear(weight=blk.attn.in_proj_weight, bias=blk.attn.in_proj_bias)
        self.out = PackedLinear(blk.attn.out_proj)
        self.fc, self.proj = PackedLinear(blk.mlp.c_fc), PackedLinear(blk.mlp.c_proj)
        self.heads = blk.attn.num_heads


class PackedTextTower:
    """compute_dtype: 16-bit type of the packed weights and activations (float16, or bfloat16 for training)."""

    def __init__(self, model, layer_idx=0, compute_dtype=torch.float16):
        blocks = list(model.transformer.resblocks)
        self.compute_dtype = compute_dtype
        with engine.compute(compute_dtype):
            self.blocks = [PackedTextBlock(b) for b in blocks[:len(blocks) - layer_idx]]     # "penultimate": drop the last block
        self.pos = model.positional_embedding.detach().float()
        self.ln_final = PackedNorm(model.ln_final)
        self.width = self.pos.shape[1]
        if self.width % 64 or any(self.width // b.heads != 64 for b in self.blocks):
            raise RuntimeError("the attention kernel is specialised for d_head = 64 (ViT-H text tower: width 1024, 16 heads)")


def encode_with_transformer(text_emb, tower: PackedTextTower):
    """text_emb [B, L, width] (token embeddings with the special tokens spliced in) -> [B, L, width] fp32.  Differentiable w.r.t.
    text_emb when autograd is recording and it requires grad (or whenever the tower computes in bfloat16, whose GEMMs have no fused
    GELU epilogue)."""
    if (torch.is_grad_enabled() and text_emb.requires_grad) or tower.compute_dtype != torch.float16:
        return _encode_unfused(text_emb, tower)
    B, L, D = text_emb.shape
    x = (text_emb.float() + tower.pos[:L]).reshape(B * L, D).to(torch.float16).contiguous()
    M = B * L
    for p in tower.blocks:
        h = ops.layer_norm(x, p.ln1.g, p.ln1.b, p.ln1.eps)
        qkv = ops.gemm_conv(h, p.qkv.w, B=1, H=1, W=M, taps=1, bias=p.qkv.b)
        a = ops.attention_causal(qkv[:, :D], qkv[:, D:2 * D], qkv[:, 2 * D:], B, p.heads, L, 64 ** -0.5)
        x = ops.gemm_conv(a, p.out.w, B=1, H=1, W=M, taps=1, bias=p.out.b, resid=x)
        h = ops.layer_norm(x, p.ln2.g, p.ln2.b, p.ln2.eps)
        h = ops.gemm_conv(h, p.fc.w, B=1, H=1, W=M, taps=1, bias=p.fc.b, gelu=True)
        x = ops.gemm_conv(h, p.proj.w, B=1, H=1, W=M, taps=1, bias=p.proj.b, resid=x)
    x = ops.layer_norm(x, tower.ln_final.g, tower.ln_final.b, tower.ln_final.eps)
    return x.float().reshape(B, L, D)


def _encode_unfused(text_emb, tower):
    """The same sequence on the `train_ops` entry points: layer_norm -> qkv -> causal attention -> out_proj (+ residual) -> layer_norm ->
    c_fc -> GELU -> c_proj (+ residual), then ln_final.  The residual's gradient is added inside the LayerNorm backward (layer_norm_fork)."""
    B, L, D = text_emb.shape
    M = B * L
    grad = torch.is_grad_enabled() and text_emb.requires_grad
    x = (text_emb.float() + tower.pos[:L]).reshape(M, D).to(tower.compute_dtype).contiguous()
    for p in tower.blocks:
        h, x = train_ops.layer_norm_fork(x, p.ln1.g, p.ln1.b, p.ln1.eps)
        qkv = train_ops.gemm_conv(h, p.qkv.w, B=1, H=1, W=M, taps=1, bias=p.qkv.b)
        a = train_ops.attention_causal(qkv[:, :D], qkv[:, D:2 * D], qkv[:, 2 * D:], B, p.heads, L, 64 ** -0.5)
        x = train_ops.gemm_conv(a, p.out.w, B=1, H=1, W=M, taps=1, bias=p.out.b, resid=x)
        h, x = train_ops.layer_norm_fork(x, p.ln2.g, p.ln2.b, p.ln2.eps)
        if grad:
            h = train_ops.gemm_conv(h, p.fc.w, B=1, H=1, W=M, taps=1, bias=p.fc.b, gelu=True)
        else:
            h = train_ops.gelu_fwd(ops.gemm_conv(h, p.fc.w, B=1, H=1, W=M, taps=1, bias=p.fc.b))
        x = train_ops.gemm_conv(h, p.proj.w, B=1, H=1, W=M, taps=1, bias=p.proj.b, resid=x)
    x = train_ops.layer_norm(x, tower.ln_final.g, tower.ln_final.b, tower.ln_final.eps)
    return x.float().reshape(B, L, D)
