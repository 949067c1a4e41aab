/*
 * leftrefill_hip.h -- C ABI of the MI355X (gfx950) kernels behind LeftRefill's diffusion-sampling hot path.
 *
 * Boundary contract:
 *   - extern "C", raw device pointers + explicit sizes + a hipStream_t (passed as void*), no torch types;
 *   - no allocation, no synchronisation, no global mutable state inside; the caller owns every buffer,
 *     including workspaces; every call is stream-ordered and re-entrant;
 *   - return value: 0 = ok, > 0 = hipError_t of the launch, < 0 = argument error (LR_E_*).
 *
 * Layout convention on the device: activations are NHWC fp16 ("token-major": row m = (n*H + y)*W + x,
 * channels contiguous), weights are [Cout][tap][Cin] fp16 (K contiguous), statistics and accumulators fp32.
 *
 * Each entry point cites the reference call site it replaces (paths relative to the reference repo).
 */
#ifndef LEFTREFILL_HIP_H
#define LEFTREFILL_HIP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define LR_E_ARG (-1)      /* bad size / null pointer */
#define LR_E_ALIGN (-2)    /* channel count / leading dimension not a multiple the kernel needs */
#define LR_E_UNSUPPORTED (-3)

typedef void* lr_stream_t; /* hipStream_t */
typedef uint16_t lr_half;  /* 16-bit activation / weight element: IEEE binary16 bits, or bfloat16 bits in the *_bf16 entry points */
/* 16-bit compute type.  Every kernel exists for both: fp16 is what the reference's autocast inference and its fp16 AMP training
 * use (train_inpainting.py:52,127); bf16 is BASELINE configs[4].  Entry points named lr_<op>_bf16 have the signature of
 * lr_<op> (lr_<op>_f16) and read / write bfloat16 (declared at the end of this header); lr_gemm_args carries a `dtype` field. */
#define LR_DTYPE_F16 0
#define LR_DTYPE_BF16 1
/* lr_gemm_args.pipe */
#define LR_PIPE_DEFAULT 0
#define LR_PIPE_W8_DEEP 4
#define LR_PIPE_HALO 8
#define LR_UP_PHASE 3      /* lr_gemm_args.up: the phase form of the nearest-2x upsample conv */

/* ABI version; bump on any signature change. */
int lr_abi_version(void);

/* ---- layout converters at the UNet boundary ------------------------------------------------------------------
 * replaces: `h = x.type(self.dtype)` + the NCHW<->token-major rearranges, openaimodel.py:775, attention.py:402,412;
 *           `torch.cat([x] + c_concat, dim=1)` ddpm.py:1349 (optional second source x2).
 * y[n,h,w,0:C1] = x1[n,:,h,w]; y[...,C1:C1+C2] = x2 (may be NULL with C2 = 0); y[...,C1+C2:Cpad] = 0. */
int lr_nchw_f32_to_nhwc_f16(const float* x1, int C1, const float* x2, int C2, lr_half* y, int Cpad, int N, int H,
                            int W, lr_stream_t s);
/* out_nchw[n,c,h,w] = y[n,h,w,c] for c < C; out_is_f32 selects float or half output (UNet returns eps). */
int lr_nhwc_f16_to_nchw(const lr_half* y, int Cstride, int C, void* out_nchw, int out_is_f32, int N, int H, int W,
                        lr_stream_t s);

/* ---- GroupNorm(32) [+ SiLU] -------------------------------------------------------------------------------------
 * replaces: GroupNorm32 / normalization (util.py:202-219, eps 1e-5) followed by nn.SiLU in ResBlock.in_layers /
 *           out_layers / UNetModel.out (openaimodel.py:200-231,726-731) and Normalize (attention.py:90-91, eps 1e-6).
 * Input is the virtual concat [x1 (C1 ch) | x2 (C2 ch)] (th.cat([h, hs.pop()], 1), openaimodel.py:781); x2 may be NULL.
 * Two launches: stats writes per-chunk partial (sum, sumsq) to `partials` (caller provides N*LR_GN_CHUNKS*64 floats; the
 * number of chunks actually used is a deterministic function of N and HW) -- no atomics, bitwise reproducible; apply
 * finalises mean/rstd in fp64 from the partials and writes y [N*HW][C1+C2] fp16. */
#define LR_GN_CHUNKS 256
int lr_groupnorm_stats(const lr_half* x1, int C1, const lr_half* x2, int C2, int N, int HW, float* partials,
                       lr_stream_t s);
int lr_groupnorm_apply(const lr_half* x1, int C1, const lr_half* x2, int C2, int N, int HW, const float* partials,
                       const float* gamma, const float* beta, float eps, int silu, lr_half* y, lr_stream_t s);
/* Statistics from the producers instead of a pass over x: p1 / p2 = gn_stats_out of the GEMMs that wrote x1 / x2
 * ([M / R1][C1][2], [M / R2][C2][2], M = N*HW; R1, R2 must divide HW).  finalize reduces them (fp64, fixed order) to
 * group sums in the layout lr_groupnorm_apply_n reads with nchunks = 1: partials [N][1][32][2]. */
int lr_groupnorm_finalize(const float* p1, int C1, int R1, const float* p2, int C2, int R2, int N, int HW, float* partials,
                          lr_stream_t s);

/* ---- the UNet's `out` block in one launch (ABI 21) -------------------------------------------------------------------------
 * replaces: `self.out = nn.Sequential(normalization(ch), nn.SiLU(), zero_module(conv_nd(dims, model_channels, out_channels, 3,
 *           padding=1)))` applied as `self.out(h)` (reference ldm/modules/diffusionmodules/openaimodel.py:714-718, 812) and the
 *           NHWC -> NCHW conversion of its result: GroupNorm(32) + SiLU + 3x3 pad-1 conv to Cout <= 4 channels, input read once.
 *   x [B][H][W][C] fp16 (NHWC tokens), gpart [B][chunks][32][2] per-group (sum, sumsq) partials of x from its producer
 *   (lr_gemm_args.gn_group_out), gamma / beta [C] fp32; w [>= Cout][ldw] fp16 with k = tap * C + channel (the packed conv weight,
 *   rows >= Cout ignored), bias [>= Cout] fp32 or NULL; y [B][Cout][H][W] fp16 (NCHW).  The normalised + SiLU'd activation is
 *   rounded to fp16 before the product exactly like the two-launch path stores it.
 *   C % 64 == 0, H % 8 == 0, W % 16 == 0, Cout <= 4, 9 C small enough for LDS (C <= 704): otherwise LR_E_UNSUPPORTED. */
int lr_gn_conv_out_f16(const lr_half* x, int B, int H, int W, int C, const float* gpart, int chunks, const float* gamma, const float* beta,
                       float eps, const lr_half* w, int ldw, const float* bias, int Cout, lr_half* y, lr_stream_t s);
/* lr_groupnorm_apply with an explicit chunk count of `partials` ([N][nchunks][32][2]) */
int lr_groupnorm_apply_n(const lr_half* x1, int C1, const lr_half* x2, int C2, int N, int HW, const float* partials,
                         int nchunks, const float* gamma, const float* beta, float eps, int silu, lr_half* y, lr_stream_t s);

/* ---- LayerNorm over the channel dimension -------------------------------------------------------------------------
 * replaces: nn.LayerNorm norm1/2/3 in BasicTransformerBlock (attention.py:271-273, eps 1e-5). x,y [M][C] fp16. */
int lr_layernorm(const lr_half* x, const float* gamma, const float* beta, float eps, lr_half* y, int M, int C,
                 lr_stream_t s);

/* ---- timestep embedding + small-M linear (time MLP) -------------------------------------------------------------
 * replaces: timestep_embedding (util.py:154-174; cos first), UNetModel.time_embed (openaimodel.py:528-532) and the
 *           22 ResBlock.emb_layers (217-223) batched as one [sum Cout][1280] weight. */
int lr_timestep_embedding(const int64_t* t, int N, int dim, lr_half* out, lr_stream_t s);
/* replaces: timestep_embedding (util.py:154-174) at continuous times -- `timesteps[:, None].float() * freqs` of the fp32 times
 *           DPM-Solver feeds the model (dpm_solver.py:239-240, 999.0, 899.1, ...).  Same expression as lr_timestep_embedding
 *           with t read as fp32: an integer-valued t gives the same bytes (ABI 27). */
int lr_timestep_embedding_f32(const float* t, int N, int dim, lr_half* out, lr_stream_t s);
/* out[m][n] = act_out( sum_k act_in(a[m][k]) * w[n][k] + bias[n] ), M <= 16; act: 0 none, 1 SiLU. K % 8 == 0. */
int lr_linear_small_m(const lr_half* a, int lda, const lr_half* w, const float* bias, lr_half* out, int ldo, int M,
                      int N, int K, int act_in, int act_out, lr_stream_t s);

/* ---- implicit-GEMM convolution / linear on MFMA --------------------------------------------------------------------
 * replaces: conv3x3 s1/s2 (+bias) in ResBlock / Downsample / Upsample / input / output conv (openaimodel.py:106,150,
 *           200-231,546,730), the 1x1 skip_connection (240), nn.Linear in CrossAttention / SpatialTransformer /
 *           GEGLU / FeedForward (attention.py:54,74,156-163,359,381); fused epilogues replace `h + emb_out`
 *           (openaimodel.py:272), `skip(x) + h` (274), the attention/FF residual adds (attention.py:280-282,419) and
 *           `x * F.gelu(gate)` (attention.py:56-58).
 *
 *   C[m][n] = sum_{tap,c} A(m,tap,c) * Wt[n][tap*(C1+C2)+c]  (+ bias[n]) (+ rowvec[m / rows_per_batch][n]) (+ R[m][n])
 *   rows m = (b*H + y)*W + x over the OUTPUT grid; A gathers from the source grid [Hs][Ws]:
 *     taps = 1: pointwise (Linear / 1x1);  taps = 9: 3x3 pad 1 with `stride` (1|2) and optional nearest-2x `up`sample.
 *   Source is the virtual channel concat [p1 (C1) | p2 (C2)];  C1, C2 multiples of 64.
 *   geglu == 1: Wt/bias rows are pre-interleaved in 16-row groups [u16 | g16 | ...]; output has N/2 columns:
 *     out = (u + bu) * gelu_erf(g + bg).
 *   geglu == 2: plain erf-GELU of (acc + bias [+ rowvec]) before the residual (the text tower's MLP, nn.GELU).
 */
typedef struct lr_gemm_args {
  const lr_half* p1; int32_t C1;
  const lr_half* p2; int32_t C2;
  int32_t B, H, W;          /* output grid; M = B*H*W */
  int32_t Hs, Ws;           /* source grid */
  int32_t taps, stride, up; /* up: 0 none | 1 nearest 2x | 2 zero-insertion 2x (odd source rows / columns read as 0: with
                               flipped, transposed weights this is the input gradient of a stride-2 conv)
                               | LR_UP_PHASE (3): nearest 2x + 3x3 pad-1 conv as four 2x2 convs on the source, one per output phase
                               (a, b) = (y & 1, x & 1): taps = 4, wt = [4][N][4 (C1 + C2)] with wt[2a + b][n][(2 dy + dx) (C1 + C2) + c] =
                               the taps of the 3x3 kernel that read source pixel (i + a - 1 + dy, j + b - 1 + dx), summed
                               (packing.pack_conv_up_phase); H = 2 Hs, W = 2 Ws, 4/9 of the multiplies of up = 1, results equal up to one
                               more rounding of the merged weights.  Pipelined tiles only (tile_m 256 with tile_n 128 | 160 | 320,
                               tile_m 128 with tile_n 128 | 160); bias, rowvec, resid, gn_stats_out (Hs Ws a multiple of the statistics
                               row block), gn_group_out, split-K.  stride != 1, asym, geglu, ln_stats, stats_out, per-sample or
                               piece-major weights, skip1, LR_PIPE_HALO: LR_E_UNSUPPORTED */
  int32_t asym;             /* 0: 3x3 pad 1 on every side; 1: pad only bottom/right (F.pad (0,1,0,1) + padding 0, the VAE
                               Downsample, ldm/modules/diffusionmodules/model.py:83-86) */
  const lr_half* wt; int32_t N;      /* weights [N][taps*(C1+C2)] */
  const float* bias;                 /* [N] or NULL */
  const lr_half* rowvec; int32_t ld_rowvec; /* [B][ld_rowvec] per-sample vector added to every row of sample b, or NULL */
  const lr_half* resid; int32_t ld_resid;   /* [M][ld_resid] or NULL */
  lr_half* out; int32_t ld_out;             /* [M][ld_out] */
  int32_t geglu;
  int32_t tile_n;           /* 0 = auto; 64 | 128 | 160 (tile_m 128) or 128 | 160 | 256 | 320 (tile_m 256) */
  int32_t tile_m;           /* 0 = auto; 128 (4 waves, 2-stage) | 256 (8 waves, 3-stage counted-vmcnt pipeline) */
  /* split-K (small-M shapes that cannot fill 256 CUs): fp32 partial tiles go to `workspace`
   * [splits][M][N] and a second launch reduces them in a fixed order and applies the epilogue.
   * splits: 0 = auto, 1 = off.  workspace may be NULL (=> no split).  Not available with geglu. */
  int32_t splits;
  float* workspace; int64_t workspace_bytes;
  /* LayerNorm folded into a pointwise GEMM (replaces nn.LayerNorm norm1/2/3 + the Linear that follows it,
   * attention.py:271-283): p1 is the RAW x [M][K], wt = W * gamma (gamma folded along K), bias = W beta + b,
   * ln_colsum[n] = sum_k wt[n][k] (fp32, of the fp16-rounded wt):
   *     out[m][n] = rstd[m] * (acc[m][n] - mean[m] * ln_colsum[n]) + bias[n]
   * mean / rstd of row m are finalised inside the kernel from ln_stats [M][ln_parts][2] = per-row partial (sum, sumsq)
   * written by the GEMM that produced x (stats_out below).  ln_stats == NULL: plain GEMM. */
  const float* ln_stats; int32_t ln_parts; float ln_eps;
  const float* ln_colsum;
  /* stats_out != NULL: per-row (sum, sumsq) of the fp16-rounded output over each wave's column range,
   * [M][lr_gemm_stats_parts(args)][2] fp32 (fixed order, no atomics). Not with split-K. */
  float* stats_out;
  /* gn_stats_out != NULL: per-channel (sum, sumsq) of the fp16-rounded output over each block of R = lr_gemm_gn_rows(args)
   * consecutive rows, [ceil(M / R)][N][2] fp32 -- the statistics pass of the GroupNorm that consumes this tensor
   * (openaimodel.py:254-274) comes out of the producer's epilogue (of the reduce kernel, R = 32, when the call splits K);
   * lr_groupnorm_finalize turns the blocks of one sample (H*W must be a multiple of R) into per-group sums.
   * Fixed order, no atomics.  Not with GEGLU. */
  float* gn_stats_out;
  int32_t dtype;            /* LR_DTYPE_F16 | LR_DTYPE_BF16: type of p1, p2, wt, rowvec, resid, out (geglu == 2 is fp16 only) */
  int32_t pipe;             /* pipeline variant of the tile: LR_PIPE_DEFAULT (0) = the tile's standard instance (tile_m 128: 4 waves,
                             * 2-stage ring, 2-4 blocks per CU; 256 x {128,160}: 3-stage ring; 256 x {256,320}: 2-stage ring).
                             * LR_PIPE_W8_DEEP (4), tile_m 128 with tile_n 128 | 160: 8 waves (4 x 2, wave tile 32 x tile_n/2), 4-stage
                             * ring, one block per CU (the 4096- / 1024-row levels).
                             * LR_PIPE_HALO (8, ABI 23), tile_m 256 with tile_n 160 | 320: the halo-tile conv -- 3x3, stride 1, pad 1, no
                             * upsample, W a multiple of 16 and H a multiple of 16 (or H = 8 with an even number of samples: a tile is then the
                             * 8 x 16 pixels of two samples); split-K by whole 64-channel chunks: a block owns a 16 x 16 pixel tile, the 18 x 18 input patch of a
                             * 64-channel chunk is copied to LDS once and the nine taps are shifted reads of it (conv_halo.hip); K is
                             * accumulated chunk-major, so results agree with the other instances to fp32 rounding, not bit for bit.
                             * Anything else: LR_E_UNSUPPORTED */
  /* gn_group_out != NULL (ABI 20): per-GROUP (sum, sumsq) of the fp16-rounded output for the GroupNorm(32) of a consumer that
   * normalises THIS tensor alone (N / 32 channels per group), [samples][chunks][32][2] fp32 with chunks = lr_gemm_gn_group_chunks(args)
   * row tiles per sample (a sample = gn_hw rows; 0 = H * W): the tile reduces its per-channel sums to the groups it covers, so
   * lr_groupnorm_apply_n(partials = gn_group_out, nchunks = chunks) runs without lr_groupnorm_finalize.  LR_E_ARG when the plan
   * cannot produce it (lr_gemm_gn_group_chunks == 0: tile width not a whole number of groups, tiles straddling samples).  Fixed
   * order, no atomics; behind split-K it comes out of the reduce kernel (32-row chunks).  May be combined with gn_stats_out. */
  float* gn_group_out; int32_t gn_hw;
  /* wt_bstride != 0 (ABI 20): per-sample weights / bias -- rows of sample b = m / (H * W) use wt + b * wt_bstride and
   * bias + b * bias_bstride (elements).  Pointwise calls only (taps == 1), H * W a multiple of the tile's rows, no split-K.
   * Used for the GroupNorm of SpatialTransformer folded into proj_in (lr_gn_fold_weights_f16). */
  int32_t wt_bstride, bias_bstride;
  /* wt_pm != 0 (ABI 20): wt is piece-major, [K / 64][N][64] -- the 64-element (128-byte) pieces of all N rows for K-step 0, then for
   * K-step 1, ... (lr packing: w.reshape(N, K / 64, 64).permute(1, 0, 2)).  Same arithmetic, same K order; a tile's weight slice of one
   * K-step is then one contiguous run instead of tile_n pieces 2 K bytes apart.  Not with wt_bstride. */
  int32_t wt_pm;
  /* skip1 != NULL (ABI 22): pointwise K extension -- out = conv3x3([p1 | p2]) + W_s [skip1 | skip2] in ONE accumulation:
   *   wt = [N][9 (C1 + C2) + Cs1 + Cs2] (the 3x3 part first, then the pointwise weights over skip1's, then skip2's channels),
   *   bias = the sum of the two layers' biases.  skip1 / skip2: [B*H*W, Cs1 / Cs2] at the OUTPUT resolution (virtual channel concat).
   * replaces: `self.skip_connection(x) + h` of ResBlock._forward (openaimodel.py:274) where skip_connection is the 1x1 conv of a block
   *           whose width changes (253-259): the separate GEMM, its [M, N] output and the residual read of this conv's epilogue.
   * With taps == 1 the main part is pointwise too: out = W_a [p1 | p2] + W_s [skip1 | skip2] (wt = [N][C1 + C2 + Cs1 + Cs2]) -- used for
   * SpatialTransformer.proj_out composed with the last feed-forward Linear (attention.py:75-77, 412-419): proj_out(ff2(g) + x) + x_in =
   * (Wp W2) g + Wp x + (Wp b2 + bp) + x_in, one GEMM with resid = x_in.
   * stride 1, no upsample, no GEGLU / LayerNorm fold / per-sample weights: anything else LR_E_UNSUPPORTED.  resid / rowvec / statistics
   * outputs work as without it. */
  const lr_half* skip1; const lr_half* skip2; int32_t Cs1, Cs2;
  /* splitk_mode (ABI 23): 0 = the split-K partials are reduced by a second launch (fixed order); 1 (developer builds only -- measured
   * slower, profiles/r05_splitk_inlaunch.txt; the product library answers LR_E_UNSUPPORTED, ABI 24) = in-launch reduce where the plan
   * allows it (8-wave instances with 160- / 320-column tiles, tiles x splits <= 256 so that every K-slice block of the grid is
   * resident at once): every slice block publishes its partial tile write-through, waits for its tile's other slices on an
   * agent-scope counter (bounded spin) and reduces its share of the tile's rows in slice order with the full epilogue -- still
   * deterministic, no second launch.  Plans that do not qualify fall back to mode 0 silently. */
  int32_t splitk_mode;
} lr_gemm_args;
/* The five queries below and lr_gemm_conv_f16 share ONE resolution of args (resolve_plan in csrc/gemm_conv.hip: tile, pipe, split-K
 * factor and kernel instance), so a buffer sized from a query is the size the launch writes.  They read only the integer fields and
 * whether p2 / skip1 / skip2 are null; the launch alone may still drop an automatic split for want of a workspace. */
/* row tiles per sample of gn_group_out in the resolved plan, 0 if it cannot produce per-group sums */
int lr_gemm_gn_group_chunks(const lr_gemm_args* args);
/* rows per block of gn_stats_out: the resolved instance's wave-tile rows, 32 behind split-K */
int lr_gemm_gn_rows(const lr_gemm_args* args);
/* plan[0..3] = (tile_m, tile_n, splits, pipe) of the resolved plan: explicit requests as given, zeros resolved by the static
 * heuristics (a pure function of the shape -- never of timing; the Python front end ships its tuned choices as a table). */
int lr_gemm_plan(const lr_gemm_args* args, int32_t* plan);
/* number of per-row partials this call writes to stats_out: column tiles of the resolved plan x its instance's waves along N */
int lr_gemm_stats_parts(const lr_gemm_args* args);
/* bytes of workspace lr_gemm_conv_f16 would like for the resolved plan (0 if it will not split) */
int64_t lr_gemm_workspace_bytes(const lr_gemm_args* args);
int lr_gemm_conv_f16(const lr_gemm_args* args, lr_stream_t s);
/* number of bounded-spin timeouts of the in-launch split-K reduce since the library was loaded (0 in a healthy run; synchronises
 * the device; -1 on a runtime error).  A timeout means a K-slice block did not see its tile's other slices arrive: wrong results
 * for that launch instead of a hang. */
int lr_gemm_splitk_timeouts(void);

/* ---- fused scaled-dot-product attention (flash-style, d_head = 64) ---------------------------------------------
 * replaces: xformers.ops.memory_efficient_attention (attention.py:236) == softmax(q k^T * d^-0.5) v of the vanilla
 *           path (attention.py:173-195), self (Nkv = HW or view_num*h^2) and cross (Nkv = 77).
 * q [B][Nq][ldq], k/v [B][Nkv][ldk|ldv], o [B][Nq][ldo]; head h occupies columns [h*64, h*64+64). */
int lr_attention_f16(const lr_half* q, int ldq, const lr_half* k, int ldk, const lr_half* v, int ldv, lr_half* o,
                     int ldo, int B, int heads, int Nq, int Nkv, float scale, lr_stream_t s);

/* Causal self-attention (query i sees keys j <= i): the OpenCLIP text tower of the prompt encoder
 * (ldm/modules/encoders/Refill_modules.py:189-201, model.attn_mask), N = 77 tokens, heads of 64. */
int lr_attention_causal_f16(const lr_half* q, int ldq, const lr_half* k, int ldk, const lr_half* v, int ldv, lr_half* o,
                            int ldo, int B, int heads, int N, float scale, lr_stream_t s);
/* Same attention with V supplied pre-transposed: vt [B][heads*64][ld_vt] from lr_transpose_v_f16 (ld_vt = Nkv rounded up
 * to 64, tail keys zero, keys permuted inside every group of 16 to the MFMA k-slot order).  The V tile then streams into
 * LDS by DMA like K; worth it for long key sequences (self-attention), the transpose costs one read + write of V. */
int lr_attention_vt_f16(const lr_half* q, int ldq, const lr_half* k, int ldk, const lr_half* vt, int ld_vt, lr_half* o,
                        int ldo, int B, int heads, int Nq, int Nkv, float scale, lr_stream_t s);
int lr_transpose_v_f16(const lr_half* v, int ldv, lr_half* vt, int ld_vt, int B, int heads, int Nkv, lr_stream_t s);

/* ---- fused cross-attention block (C = 320, 5 heads of 64: level 0 of the SD2 UNet) --------------------------------
 * replaces: `x = self.attn2(self.norm2(x), context=context) + x` (attention.py:281) = norm2 (LayerNorm, attention.py:272),
 *           CrossAttention.to_q, softmax(q k^T * d^-0.5) v over the <= 96 context tokens, to_out[0] + bias
 *           (attention.py:165-196) and the residual add, in ONE launch: x is read once, out written once, q and the attention
 *           output never leave the registers (instead of LayerNorm-folded to_q GEMM -> attention -> to_out GEMM).
 *   x, out [M][320]; M = B * HW rows, a block of 128 rows stays inside one sample (M % 128 == 0, HW % 128 == 0).
 *   wq [320][320] = to_q.weight * gamma (LayerNorm folded along K), bq [320] = to_q.weight @ beta (fp32);
 *   k  [B * Lc][ldk]: K projection of the context whose columns are permuted inside every head: position 32 p + 8 f + i
 *      (f < 4, i < 8) holds channel 32 p + 16 (i >> 2) + 4 f + (i & 3) -- project the context with the same permutation
 *      of to_k.weight's rows;
 *   vt [B][5][2][64][64]: lr_xattn_pack_vt_f16 of the V projection (transposed, key slots in the same order);
 *   wo [5][320][64] = to_out[0].weight as per-head pieces (piece h = columns 64 h .. 64 h + 63, 40 KB contiguous) with the columns of
 *      every piece in that order, bo [320] = to_out[0].bias (fp32);
 *   stats_out (optional) [M][2]: per-row (sum, sumsq) of the rounded output (lr_gemm_args.ln_stats of the next GEMM, ln_parts = 1).
 * Anything else (other widths, Lc > 96, ragged M): LR_E_UNSUPPORTED -- callers keep the three-kernel path for those. */
typedef struct lr_xattn_args {
  const lr_half* x; lr_half* out;
  const lr_half* wq; const float* bq;
  const lr_half* k; int32_t ldk;
  const lr_half* vt;
  const lr_half* wo; const float* bo;
  float* stats_out;
  int32_t M, HW, C, heads, Lc;
  float ln_eps, scale;
  /* pre_a != NULL: the out-projection of the preceding self-attention runs in front, in the same launch
   * (`x = self.attn1(self.norm1(x)) + x`, attention.py:280):  x1 = pre_a pre_w^T + pre_b + x;  out = x1 + to_out(attention(LayerNorm(x1) ...)).
   * pre_a [M][320] = the self-attention output, pre_w [320][320] = attn1.to_out[0].weight (natural layout), pre_b [320] its bias (fp32);
   * wq must then have its COLUMNS in the k-slot order (inside every 64 columns: position 32 p + 8 f + i holds column
   * 32 p + 16 (i >> 2) + 4 f + (i & 3)): the normalised x1 reaches the q projection in accumulator order, never through memory. */
  const lr_half* pre_a; const lr_half* pre_w; const float* pre_b;
} lr_xattn_args;
int lr_xattn_block_f16(const lr_xattn_args* args, lr_stream_t s);
int lr_xattn_pack_vt_f16(const lr_half* v, int ldv, lr_half* vt, int B, int heads, int Lc, lr_stream_t s);

/* ---- entry of a SpatialTransformer's block (C = 320: level 0 of the SD2 UNet; ABI 24) --------------------------------------
 * replaces: `x = self.proj_in(x)` (use_linear, attention.py:405-408) and, of the block that follows, `self.norm1(x)` (attention.py:280)
 *           with attn1's `q = self.to_q(x); k = self.to_k(context); v = self.to_v(context)` on context = x (attention.py:168-172), in ONE
 *           launch instead of a K = 320 GEMM and a LayerNorm-folded 960-column GEMM:
 *               x1 = x wp^T + bp;     qkv = LayerNorm(x1) [Wq; Wk; Wv]^T
 *   x [M][320] (the GroupNorm-ed tokens), M % 256 == 0;  wp [320][320] = proj_in.weight, bp [320] its bias (fp32);
 *   wqkv [NQ][320] = [to_q; to_k; to_v].weight * gamma (LayerNorm folded along K, natural column order), bqkv [NQ] = W beta (fp32);
 *      NQ a multiple of 192 (960 for the SD2 block);
 *   x1 [M][320] and qkv [M][ld_qkv] out (x1 is rounded to 16 bits before the LayerNorm, like the two-launch path stores it).
 * Other widths / ragged M: LR_E_UNSUPPORTED -- callers keep the two-GEMM path. */
typedef struct lr_stin_args {
  const lr_half* x; const lr_half* wp; const float* bp; const lr_half* wqkv; const float* bqkv;
  lr_half* x1; lr_half* qkv;
  int32_t M, C, NQ, ld_qkv;
  float ln_eps;
  /* gn_part != NULL: x holds the RAW tokens and `x = self.norm(x)` of SpatialTransformer.forward (attention.py:399-404: GroupNorm(32, eps 1e-6,
   * affine), no activation) is applied to the rows as they are loaded -- same arithmetic as lr_groupnorm_apply_n, bit for bit, without
   * writing the normalised tensor.  gn_part [M / gn_hw][gn_chunks][32][2] = per-group (sum, sumsq) partials of x from its producer
   * (lr_gemm_args.gn_group_out / lr_ffn_args.gn_group_out), gn_hw rows per sample (gn_hw % 256 == 0), gn_gamma / gn_beta [320] fp32. */
  const float* gn_part; const float* gn_gamma; const float* gn_beta;
  int32_t gn_chunks, gn_hw;
  float gn_eps;
} lr_stin_args;
int lr_stin_block_f16(const lr_stin_args* args, lr_stream_t s);

/* ---- row-resident [LayerNorm +] Linear (C = 640 | 1280: levels 1 / 2 of the SD2 UNet; ABI 24) ---------------------------------
 * replaces: `self.norm1(x)` + attn1's fused `to_q / to_k / to_v` (attention.py:280, 168-172; geglu = 0, N = 3 C) and `self.norm3(x)` +
 *           GEGLU.proj + `x * F.gelu(gate)` (attention.py:282, 51-58; geglu = 1, N = 8 C -> 4 C output columns) where the tiled GEMM's
 *           K loop is only 10 steps long:   out = [gate of] LayerNorm(x) w^T + bias,  rows held in registers, weights streamed.
 *   x [M][C], C = 640 | 1280 (levels 1 / 2), M % 128 == 0;  w [N][C] = weight * gamma (LayerNorm folded along K), bias [N] = W beta + b (fp32); N % 64 == 0;
 *   geglu = 1: w / bias rows interleaved in 16-row groups [u16 | g16 | ...] (the layout of lr_gemm_args.geglu == 1), out [M][N / 2];
 *   out [M][ld_out].  The LayerNorm is two-pass in registers on the 16-bit x (no producer statistics needed).
 * Other widths / ragged M: LR_E_UNSUPPORTED -- callers keep the LayerNorm-folded GEMM. */
typedef struct lr_rowlin_args {
  const lr_half* x; const lr_half* w; const float* bias; lr_half* out;
  int32_t M, C, N, ld_out, geglu;
  float ln_eps;
  int32_t ln;      /* 1: LayerNorm the rows first (w / bias carry gamma / beta); 0: plain Linear (SpatialTransformer.proj_in, attention.py:405-408) */
  /* gn_part != NULL (ln = 0, geglu = 0): x holds RAW tokens and SpatialTransformer.norm (GroupNorm(32), attention.py:399-404) is applied to the
   * rows as they are loaded, exactly as in lr_stin_args (gn_hw % 128 == 0). */
  const float* gn_part; const float* gn_gamma; const float* gn_beta;
  int32_t gn_chunks, gn_hw;
  float gn_eps;
} lr_rowlin_args;
int lr_rowlin_f16(const lr_rowlin_args* args, lr_stream_t s);

/* ---- fused feed-forward block (C = 320: level 0 of the SD2 UNet) ------------------------------------------------------
 * replaces: `x = self.ff(self.norm3(x)) + x` (attention.py:282) = norm3 (LayerNorm), GEGLU.proj + `x * F.gelu(gate)` (attention.py:51-58),
 *           FeedForward.net[2] Linear + bias (attention.py:74-78) and the residual add, in ONE launch: the [M][H] hidden activation
 *           (168 MB at M = 65536, H = 1280) is never written (instead of LayerNorm-folded GEGLU GEMM -> Linear GEMM).
 *   x, out [M][320], M % 128 == 0;
 *   w1 [2H][320] = GEGLU.proj.weight * gamma (LayerNorm folded along K) with its rows interleaved in 16-row groups [u16 | g16 | ...]
 *      (the layout of lr_gemm_args.geglu == 1), b1 [2H] = proj.weight @ beta + proj.bias in the same row order (fp32);
 *   w2 [H / 64][320][64] = net[2].weight as 64-column pieces (each 40 KB contiguous) in the k-slot order of lr_xattn_args.wo (inside a
 *      piece: position 32 p + 8 f + i holds column 32 p + 16 (i >> 2) + 4 f + (i & 3)), b2 [320] = net[2].bias (fp32);  H % 64 == 0, H <= 2048;
 *   stats_out (optional) [M][2][2]: per-row (sum, sumsq) of the rounded output, one partial per column half (ln_parts = 2).
 * Other widths / ragged M: LR_E_UNSUPPORTED -- callers keep the two-GEMM path. */
typedef struct lr_ffn_args {
  const lr_half* x; lr_half* out;
  const lr_half* w1; const float* b1;
  const lr_half* w2; const float* b2;
  float* stats_out;
  int32_t M, C, H;
  float ln_eps;
  /* post_w != NULL: the Linear after the block runs in the same launch (SpatialTransformer.proj_out + `x + x_in`, attention.py:412-419):
   *   x3 = x + ff(LayerNorm(x));  out = x3 post_w^T + post_b + post_resid.
   * post_w [5][320][64] = proj_out.weight as 64-column pieces in k-slot order (like w2), post_b [320] fp32, post_resid [M][320];
   * gn_stats_out (optional) [M / 128][320][2] = per-channel (sum, sumsq) of the rounded output over each block of 128 rows, for the
   * GroupNorm that consumes `out` (lr_groupnorm_finalize with R = 128); stats_out is then the row statistics of `out`. */
  const lr_half* post_w; const float* post_b; const lr_half* post_resid; float* gn_stats_out;
  /* gn_group_out (optional, with post_w; ABI 20) [M / gn_hw][gn_hw / 128][32][2]: per-GROUP (sum, sumsq) of the rounded output over each
   * block of 128 rows (10 channels per group) -- lr_groupnorm_apply_n reads it directly (nchunks = gn_hw / 128), no finalize launch. */
  float* gn_group_out; int32_t gn_hw;
} lr_ffn_args;
int lr_ffn_block_f16(const lr_ffn_args* args, lr_stream_t s);

/* ---- row softmax of materialised logits (VAE AttnBlock: single head, d_head = C = 512) ---------------------------
 * replaces: `w_ = w_ * (int(c)**(-0.5)); w_ = softmax(w_, dim=2)` (ldm/modules/diffusionmodules/model.py:186-187) between
 *           the two bmm's (185, 192), which run through lr_gemm_conv_f16 (logits = q k^T with wt = k; out = p v with
 *           wt = v^T).  p[m][:] = softmax(scale * s[m][:]), fp32 math, fp16 in/out, N % 8 == 0, N <= 16384; p may alias s. */
int lr_softmax_rows_f16(const lr_half* s, lr_half* p, int M, int N, float scale, lr_stream_t st);

/* ---- re-arranged multi-view token gather / scatter ----------------------------------------------------------------
 * replaces: multiview_attention.py:436-448 (gather to [target, ref_0..]) and 452-462 (scatter back; target -> every
 *           canvas) for concat_target=True.  x [b*v][2*s*s][C] canvases (left = ref_i, right = target), seq [b][(v+1)*s*s][C].
 * (concat_target=False is a pure reshape and needs no kernel.) */
int lr_mv_gather(const lr_half* x, lr_half* seq, int b, int v, int s, int C, lr_stream_t st);
/* ---- row copies with index tables (ABI 23) -----------------------------------------------------------------------------------
 * replaces: the rearranges around the cross-view self-attention when the canvases of a sample live on different ranks
 *           (`rearrange(x, '(b v) hw c -> b (v hw) c')`, the concat_target slicing and the write-back, reference
 *           ldm/modules/multiview_attention.py:436-462): pack rows + per-row statistics into one message, unpack a received message
 *           into sequence order and into this rank's own rows, assemble the canvas -- up to 4 independent jobs in ONE launch.
 * job: for r < n_rows copy row_bytes bytes  src + src_idx[r] * src_pitch + src_off  ->  dst + dst_idx[r] * dst_pitch + dst_off
 *      (a NULL index table = the identity).  All byte counts / offsets / pitches / pointers multiples of 8. */
typedef struct lr_row_copy_job {
  const void* src; int64_t src_pitch, src_off;
  void* dst; int64_t dst_pitch, dst_off;
  int32_t row_bytes, n_rows;
  const int32_t* src_idx; const int32_t* dst_idx;
} lr_row_copy_job;
int lr_row_copy(const lr_row_copy_job* jobs, int n_jobs, lr_stream_t s);
int lr_mv_scatter(const lr_half* seq, lr_half* x, int b, int v, int s, int C, lr_stream_t st);

/* ---- fused classifier-free-guidance + DDIM update ----------------------------------------------------------------
 * replaces: p_sample_ddim's ~15 elementwise kernels (ddim.py:343,366,377-381): e = e_u + s (e_c - e_u);
 *           pred_x0 = (x - sqrt(1-a_t) e)/sqrt(a_t); x_prev = sqrt(a_prev) pred_x0 + sqrt(1-a_prev-sigma^2) e + sigma*noise.
 * x, x_prev, pred_x0, noise: fp32 [numel]; eps: fp16 or fp32 [2*numel], uncond half first (ddim.py:317-333).
 * noise may be NULL (sigma = 0).  Coefficients are host scalars (no device->host sync, cf. ddim.py:359-362). */
int lr_ddim_cfg_step(const float* x, const void* eps, int eps_is_f32, const float* noise, float* x_prev,
                     float* pred_x0, int64_t numel, float cfg_scale, float a_t, float a_prev, float sigma_t,
                     float sqrt_one_minus_at, lr_stream_t s);

/* ---- fused classifier-free-guidance + PLMS update (ABI 27) -------------------------------------------------------
 * replaces: PLMSSampler.p_sample_plms after the model call (plms.py:189-190 CFG combine, 225-241 multistep combination,
 *           204-223 pred_x0 / x_prev with sigma = 0): e = e_u + s (e_c - e_u) rounded in the eps dtype;
 *           e' = (w[0] e + w[1] hist[0] + ... + w[n_hist] hist[n_hist-1]) / divisor, left to right;
 *           pred_x0 = (x - sqrt(1-a_t) e') / sqrt(a_t); x_prev = sqrt(a_prev) pred_x0 + sqrt(1-a_prev) e'.
 * hist: n_hist (0..3) fp32 [numel] CFG-combined eps of earlier steps, newest first; weights: n_hist + 1 integer weights
 *   (55,-59,37,-9 / 24; 23,-16,5 / 12; 3,-1 / 2; 1,1 / 2 for the second pass of the first step; 1 / 1).
 * e_out (NULL = not written): fp32 [numel] CFG-combined e of this evaluation, the next step's history.  No device->host sync. */
int lr_plms_cfg_step(const float* x, const void* eps, int eps_is_f32, const float* const* hist, int n_hist, const float* weights,
                     float divisor, float* e_out, float* x_prev, float* pred_x0, int64_t numel, float cfg_scale, float a_t,
                     float a_prev, float sqrt_one_minus_at, lr_stream_t s);

/* ---- fused classifier-free-guidance + DPM-Solver++ multistep update (ABI 27) ---------------------------------------
 * replaces: model_wrapper's CFG combine (dpm_solver.py:302-314), DPM_Solver.data_prediction_fn (360-373, no thresholding) and
 *           the predict_x0 updates: dpm_solver_first_update (469-514) for x0_prev == NULL, else
 *           multistep_dpm_solver_second_update (723-778, solver_type 'dpm_solver').
 *   x0_out = m0 = (x - sigma_s e) / alpha_s       (the next step's history)
 *   order 1: x_next = ratio x - c m0                     ratio = sigma_t / sigma_s, c = alpha_t expm1(-h)
 *   order 2: x_next = ratio x - c m0 - c_half D          c = alpha_t (exp(-h) - 1), c_half = 0.5 c, D = inv_r0 (m0 - x0_prev)
 * The per-step scalars are computed once per sampling on the host, in fp32, in the reference's order. */
int lr_dpmpp_cfg_step(const float* x, const void* eps, int eps_is_f32, const float* x0_prev, float* x0_out, float* x_next,
                      int64_t numel, float cfg_scale, float sigma_s, float alpha_s, float ratio, float c, float c_half,
                      float inv_r0, lr_stream_t s);

/* ---- DDIM inversion step: classifier-free guidance + x_next = c1 x + c2 e (ABI 28) ---------------------------------
 * replaces: DDIMSampler.encode after the model call (ddim.py:411-421): e = e_u + s (e_c - e_u) rounded in the eps dtype exactly
 *           as lr_ddim_cfg_step; x_next = c1 x + c2 e, two products and an add, each rounded in fp32 (no fused multiply-add).
 *           c2 is a 0-dim tensor in the reference, cast to the dtype of eps: with 16-bit eps, c2 and the product c2 e are
 *           rounded to the eps dtype (pass c2 already rounded from float64 to that dtype, so it is not rounded twice).
 * c1 = sqrt(a_next / a), c2 = sqrt(a_next) (sqrt(1/a_next - 1) - sqrt(1/a - 1)): host scalars formed in the reference's dtype
 * chain (a_next fp32, a float64), rounded to fp32.  x, x_next: fp32 [numel]; eps [2 numel], uncond half first.  A scale-1 call
 * (no unconditional pass) passes the single eps twice. */
int lr_ddim_inv_cfg_step(const float* x, const void* eps, int eps_is_f32, float* x_next, int64_t numel, float cfg_scale,
                         float c1, float c2, lr_stream_t s);

/* ---- three-way guidance + DDIM update of StructureDDIMSampler (ABI 28) ----------------------------------------------
 * replaces: p_sample_ddim_guide (ddim.py:605-607 combine, 623-647 update): eps [3 numel] = uncond, cond, cond_simple;
 *           e = e_u + s ((w e_c + (1 - w) e_s) - e_u), each operation rounded in the eps dtype; then pred_x0 / x_prev as
 *           lr_ddim_cfg_step (op by op in fp32).  one_minus_cond_weight: (1 - w) formed in double by the caller, as python does.
 * noise may be NULL (sigma = 0).  Coefficients are host scalars. */
int lr_ddim_cfg3_step(const float* x, const void* eps, int eps_is_f32, const float* noise, float* x_prev, float* pred_x0,
                      int64_t numel, float cfg_scale, float cond_weight, float one_minus_cond_weight, float a_t, float a_prev,
                      float sigma_t, float sqrt_one_minus_at, lr_stream_t s);

/* ---- ancestral DDPM posterior step (ABI 30) -----------------------------------------------------------------------------
 * replaces: LatentDiffusion.p_sample after the model call (ddpm.py:950-960 predict_start_from_noise / clamp / q_posterior, 986-997
 *           noise and nonzero mask) and, with a known region, the blend of p_sample_loop / progressive_denoising
 *           (ddpm.py:1093-1095, 1044-1047), op by op in fp32 (no fused multiply-add):
 *             x_recon = sqrt_recip_ac x - sqrt_recipm1_ac eps;  clamp to [-1, 1] if clip_denoised
 *             x_prev  = coef1 x_recon + coef2 x + sigma noise
 *             x_prev  = (sqrt_ac known_x0 + sqrt_one_minus_ac known_noise) mask + (1 - mask) x_prev        if mask
 * x, noise, x_prev, x0_out (= x_recon, may be NULL), known_x0, known_noise: fp32 [numel]; eps: ONE slab [numel] fp16 (bf16 in
 * the twin) or fp32 (eps_is_f32), widened to fp32 on load -- the ancestral sampler has no classifier-free guidance.
 * The coefficients are the fp32 table entries at the step's timestep, read on the HOST (no device->host sync in the loop):
 * sqrt_recip(m1)_alphas_cumprod[t], posterior_mean_coef1/2[t], sigma = (t != 0) exp(0.5 posterior_log_variance_clipped[t]) formed
 * in fp32; a temperature is applied to `noise` by the caller.  noise may be NULL when sigma == 0 (t == 0: x_prev is the mean).
 * They are scalars: a batch whose samples sit at different timesteps (a direct p_sample call) is one call per run of equal t on
 * that run's slice -- the sampling loops step the whole batch at one t, so they issue one launch.
 * mask, known_x0, known_noise: all three or none.  mask_hw > 0: mask is [numel / mask_chw][mask_hw] and broadcasts over the
 * mask_chw / mask_hw channels of each sample ([B,1,H,W] against [B,C,H,W]); mask_hw == 0: mask is fp32 [numel]. */
int lr_ddpm_step(const float* x, const void* eps, int eps_is_f32, const float* noise, const float* known_x0,
                 const float* known_noise, const float* mask, int64_t mask_chw, int64_t mask_hw, int clip_denoised, float* x_prev,
                 float* x0_out, int64_t numel, float sqrt_recip_ac, float sqrt_recipm1_ac, float coef1, float coef2, float sigma,
                 float sqrt_ac, float sqrt_one_minus_ac, lr_stream_t s);

/* ---- DDIM forward noising with a per-sample step (ABI 28) ----------------------------------------------------------
 * replaces: DDIMSampler.stochastic_encode (ddim.py:436-449): out[b] = sa[b] x0[b] + s1ma[b] noise[b] with
 *           sa = sqrt(ddim_alphas)[t[b]], s1ma = ddim_sqrt_one_minus_alphas[t[b]] (extract_into_tensor), all fp32.
 * x0, noise, out: fp32 [B][per_sample]; sa, s1ma: HOST arrays of B floats, passed by value -- B <= LR_Q_SAMPLE_MAX_B per call
 * (larger batches: one call per chunk of samples). */
#define LR_Q_SAMPLE_MAX_B 32
int lr_ddim_q_sample(const float* x0, const float* noise, float* out, int B, int64_t per_sample, const float* sa,
                     const float* s1ma, lr_stream_t s);

/* ==== backward of the same operators (training with frozen weights: input gradients only) =========================
 * replaces: what torch.autograd derives for the reference's modules under `loss.backward()` (train_inpainting.py:141 ->
 *           LatentDiffusion.p_losses, ldm/models/diffusion/ddpm.py:900-935), recomputed per block by
 *           CheckpointFunction.backward (ldm/modules/diffusionmodules/util.py:133-151).
 * Input gradients of conv / linear are lr_gemm_conv_f16 itself on flipped / transposed weights (stride-2: `up = 2`). */

/* LayerNorm: dx = rstd * (g - mean(g) - xhat * mean(g * xhat)), g = dy * gamma.  x, dy, dx [M][C] fp16. */
int lr_layernorm_bwd(const lr_half* x, const lr_half* dy, const float* gamma, float eps, lr_half* dx, int M, int C,
                     lr_stream_t s);
/* GroupNorm(32)[+SiLU] over the virtual concat [x1 | x2]: fwd_partials = lr_groupnorm_stats of the same input;
 * bwd_partials: N*LR_GN_CHUNKS*64 floats of scratch; dy [N*HW][C1+C2]; dx1 [N*HW][C1], dx2 [N*HW][C2] (NULL if C2 = 0). */
int lr_groupnorm_bwd(const lr_half* x1, int C1, const lr_half* x2, int C2, const lr_half* dy, int N, int HW,
                     const float* fwd_partials, const float* gamma, const float* beta, float eps, int silu,
                     float* bwd_partials, lr_half* dx1, lr_half* dx2, lr_stream_t s);
/* ABI 25: the two backward passes with the gradient of the residual branch around the normalisation added in fp32 before the one
 * rounding -- `x + f(LayerNorm(x))` (attention.py:279-283) and `skip_connection(x) + f(GroupNorm(x))` (openaimodel.py:254-274,
 * attention.py:399-419) send two gradients to x; dres* (same layout as x*, NULL = none) is the one that does not pass through the
 * normalisation, so the fan-in sum costs no pass of its own.  fwd_chunks: chunk count of fwd_partials ([N][fwd_chunks][32][2]: the
 * per-group sums a producing GEMM wrote through lr_gemm_args.gn_group_out, or lr_groupnorm_finalize's [N][1][32][2]); 0 = the
 * lr_groupnorm_stats layout of lr_groupnorm_bwd. */
int lr_layernorm_bwd_res(const lr_half* x, const lr_half* dy, const lr_half* dres, const float* gamma, float eps, lr_half* dx,
                         int M, int C, lr_stream_t s);
int lr_groupnorm_bwd_res(const lr_half* x1, int C1, const lr_half* x2, int C2, const lr_half* dy, const lr_half* dres1,
                         const lr_half* dres2, int N, int HW, const float* fwd_partials, int fwd_chunks, const float* gamma,
                         const float* beta, float eps, int silu, float* bwd_partials, lr_half* dx1, lr_half* dx2, lr_stream_t s);
/* GEGLU: pre = projection + bias in the packed [u16 | g16] column layout (lr_gemm_conv_f16 with geglu = 0 on the packed
 * weights), dy [M][H] -> dpre [M][2H] (same layout): du = dy * gelu(g), dg = dy * u * gelu'(g). */
int lr_geglu_bwd(const lr_half* pre, const lr_half* dy, lr_half* dpre, int M, int H, lr_stream_t s);
/* training forward: out [M][H] = u * gelu(g) from the stored packed projection (kept for lr_geglu_bwd instead of recomputing). */
int lr_geglu_fwd(const lr_half* pre, lr_half* out, int M, int H, lr_stream_t s);
/* Attention: forward that also saves the log2-domain log-sum-exp (lse [B][heads][Nq] fp32), and the backward that
 * recomputes P from it (two deterministic kernels: dQ over key tiles; dK, dV over query tiles; plus D = rowsum(dO o O)).
 * kt / dot / ld_kt: ignored since ABI 25 (rounds 2-5 took lr_transpose_v_f16 copies of q / k / dout in qt / kt / dot; the kernels now gather
 * the k-major operands from the natural tiles with the LDS transpose read); the fields keep the struct layout, pass NULL / 0.
 * qt / ld_qt (ABI 26): query split of the dK / dV kernel for few keys against many queries (the 77-key cross-attention of the 64 x 128
 * level is ONE key block per (batch, head)): ld_qt = number of query slices (0 / 1 = none, <= 64), qt = fp32 workspace of
 * ld_qt * B * heads * ceil(Nkv / 128) * 2 * 128 * 64 floats (16-byte aligned); the slices' partial dK / dV are summed in slice order by a
 * second launch (deterministic).  NULL / 0 keep the single-slice kernel.
 * dsum: scratch [B][heads][Nq] fp32.  dq [B][Nq][lddq], dk / dv [B][Nkv][lddk | lddv], head h in columns h*64.. like q/k/v. */
int lr_attention_lse_f16(const lr_half* q, int ldq, const lr_half* k, int ldk, const lr_half* v, int ldv, lr_half* o,
                         int ldo, float* lse, int B, int heads, int Nq, int Nkv, float scale, lr_stream_t s);
typedef struct lr_attn_bwd_args {
  const lr_half* q; const lr_half* k; const lr_half* v; const lr_half* o; const lr_half* dout;
  const lr_half* qt; const lr_half* kt; const lr_half* dot;
  const float* lse; float* dsum;
  lr_half* dq; lr_half* dk; lr_half* dv;
  int32_t ldq, ldk, ldv, ldo, lddo, ld_qt, ld_kt, lddq, lddk, lddv;
  int32_t B, heads, Nq, Nkv;
  float scale;
} lr_attn_bwd_args;
int lr_attention_bwd_f16(const lr_attn_bwd_args* args, lr_stream_t s);
/* ---- training of the prompt tokens through the text tower (ABI 29) -------------------------------------------------
 * Causal self-attention (key j visible to query i iff j <= i, the tower's attn_mask): lr_attention_causal_lse_f16 is
 * lr_attention_causal_f16 that also writes the log2-domain log-sum-exp lse [B][heads][N] fp32 (the convention of
 * lr_attention_lse_f16); lr_attention_causal_bwd_f16 is lr_attention_bwd_f16 under the same mask (P = 0 above the diagonal, tiles
 * wholly above it skipped).  Same argument struct; requires Nq == Nkv (else LR_E_ARG) and ld_qt == 0 (else LR_E_UNSUPPORTED, before any
 * launch): the causal dK / dV kernel takes no query split. */
int lr_attention_causal_lse_f16(const lr_half* q, int ldq, const lr_half* k, int ldk, const lr_half* v, int ldv, lr_half* o,
                                int ldo, float* lse, int B, int heads, int N, float scale, lr_stream_t s);
int lr_attention_causal_bwd_f16(const lr_attn_bwd_args* args, lr_stream_t s);
/* plain erf-GELU (the tower's MLP, nn.GELU) over n contiguous elements, n % 8 == 0, 16-byte aligned: y = gelu(pre) with the
 * formula of the lr_gemm_args.geglu == 2 epilogue, and dpre = dy * gelu'(pre), gelu'(x) = Phi(x) + x phi(x).  Training runs c_fc as a
 * plain GEMM and keeps pre for the backward; inference keeps the fused epilogue. */
int lr_gelu_fwd_f16(const lr_half* pre, lr_half* y, int64_t n, lr_stream_t s);
int lr_gelu_bwd_f16(const lr_half* pre, const lr_half* dy, lr_half* dpre, int64_t n, lr_stream_t s);

/* multi-view re-arrangement: gradient of lr_mv_gather (dseq -> dx: canvases other than 0 get zero in their right half) and
 * of lr_mv_scatter (dx -> dseq: the target slot sums the right halves of all canvases). */
int lr_mv_gather_bwd(const lr_half* dseq, lr_half* dx, int b, int v, int s, int C, lr_stream_t st);
int lr_mv_scatter_bwd(const lr_half* dx, lr_half* dseq, int b, int v, int s, int C, lr_stream_t st);
/* nearest-2x upsample: y[n][h][w][:] = sum of the four fine pixels of x [N][2H][2W][C]. */
int lr_sumpool2x2(const lr_half* x, lr_half* y, int N, int H, int W, int C, lr_stream_t s);

/* ---- scoring a decoded prediction: PSNR, SSIM, finite check and 8-bit image in one pass (added under ABI 30: one new symbol,
 *      nothing renumbered or re-typed; a library without it fails to bind, which is the staleness check) -----------------------------
 * replaces: the tail of the evaluation harness and of the task models' validation_step --
 *             `pred = pred * mask + origin_image * (1 - mask)`, the `[:, :, :, w // 2:]` crop                 test_inpainting.py:146-150
 *             `F.interpolate(..., mode='area')` to metric_size at an integer ratio                            test_inpainting.py:151-155
 *             `peak_signal_noise_ratio((pred + 1) / 2, (origin + 1) / 2, data_range=1.0)` per image           test_inpainting.py:158
 *             `TF.rgb_to_grayscale` + `structural_similarity` (scikit-image 0.18.1 defaults) per image        test_inpainting.py:160-162
 *             `((pred.clamp(-1, 1) + 1) / 2 * 255).astype(uint8)` for the PNG                                 test_inpainting.py:168-190
 *           and the same sequence in ref_inpainting_ldm.py:119-146, multiview_ref_inpainting_ldm.py:225-263, NVS_ldm.py:374-401
 *           (the NVS validation scores the raw prediction: mask = NULL, NVS_ldm.py:380-381).
 * pred [N][3][H][W] of element type `pred_kind`, origin [N][3][H][W] fp32, both in [-1, 1]; mask [N][1][H][W] fp32 or NULL (no
 * composite).  Columns [x0, x0 + Wc) of the canvas are scored; r >= 1 is the integer area-down-sampling factor (H % r == 0,
 * Wc % r == 0, H / r >= 7, Wc / r >= 7).  SSIM: 7 x 7 uniform window on the luma 0.2989 R + 0.587 G + 0.114 B of (x + 1) / 2, sample
 * covariance (49 / 48), K1 = 0.01, K2 = 0.03, data_range = 2, mean over the windows that lie fully inside the scored image.
 *   out [N][4] fp32 = (mse of (x + 1) / 2, psnr in dB (+inf when mse == 0), ssim, number of non-finite pred values in the scored columns);
 *   rgb8 [N][H / r][Wc / r][3] or NULL: (clamp(p, -1, 1) + 1) / 2 * 255 of the (composited, down-sampled) prediction, truncated;
 *   partials: LR_EVAL_SLOT_FLOATS floats per workgroup = N * ceil(H / r / LR_EVAL_TILE_H) * ceil(Wc / r / LR_EVAL_TILE_W) slots,
 *   16-byte aligned like out.  Two launches (tiles, then a fixed-order fp64 sum per sample); no atomics: bitwise reproducible. */
#define LR_EVAL_PRED_F32 0
#define LR_EVAL_PRED_F16 1
#define LR_EVAL_PRED_BF16 2
#define LR_EVAL_TILE_H 32
#define LR_EVAL_TILE_W 64
#define LR_EVAL_SLOT_FLOATS 8
#define LR_EVAL_MAX_R 32
int lr_eval_metrics(const void* pred, int pred_kind, const float* origin, const float* mask, int N, int H, int W, int x0, int Wc,
                    int r, float* partials, float* out, uint8_t* rgb8, lr_stream_t s);

/* ---- the optimizer tail of a mixed-precision training step (added under ABI 30 like lr_eval_metrics: one new symbol, a library
 *      without it fails to bind) ------------------------------------------------------------------------------------------------------
 * replaces: `scaler.unscale_(opt)`, the host-side isfinite read-back, `opt.step()` of torch.optim.AdamW and `scaler.update()` --
 *           what Lightning `precision=16` runs after every backward of train_inpainting.py, and the hand-rolled scaler of bench.py.
 * Semantics: torch.amp.GradScaler around torch.optim.AdamW (decoupled decay, bias correction, amsgrad off).  Gradients are up-cast to
 * fp32 and multiplied by 1 / scale; if any scaled gradient of any tensor is non-finite the whole update is skipped (parameters and
 * moments keep their bits), the scale is multiplied by backoff_factor and the growth tracker reset; otherwise AdamW is applied and
 * after growth_interval applied steps in a row the scale is multiplied by growth_factor.  growth_interval == 0: no scaler dynamics
 * (the scale, normally 1, never changes -- the bf16 / fp32 mode); a non-finite gradient still skips and is counted.
 * The index into each group's lr table advances on EVERY call (a per-step scheduler steps whether or not the optimizer did) and
 * holds the last entry past the end; the bias-correction step advances only on applied steps.
 *   tensors [n_tensors], groups [n_groups <= LR_OPT_MAX_GROUPS], state [LR_OPT_STATE_WORDS 32-bit words], partials [4 * blocks floats]:
 *   DEVICE memory, 16-byte aligned.  blocks (1 .. LR_OPT_MAX_BLOCKS): workgroups of the two element-wise launches.
 *   launches: host counter incremented once per kernel launch, or NULL.
 * Three launches for any number of tensors; sums in a fixed order, no atomics: bitwise reproducible.  Reads nothing back: capturable. */
#define LR_OPT_GRAD_F32 0
#define LR_OPT_GRAD_F16 1
#define LR_OPT_GRAD_BF16 2
#define LR_OPT_MAX_GROUPS 8
#define LR_OPT_MAX_BLOCKS 1024
/* state block, 32-bit words */
#define LR_OPT_SCALE 0           /* float: loss scale */
#define LR_OPT_GROWTH_TRACKER 1  /* int: applied steps since the scale last changed */
#define LR_OPT_FOUND_INF 2       /* int: 1 when the last call skipped */
#define LR_OPT_APPLIED_STEPS 3   /* int: AdamW bias-correction step */
#define LR_OPT_SCHED_STEPS 4     /* int: calls so far = next lr index */
#define LR_OPT_SKIPPED 5         /* int: skipped calls so far */
#define LR_OPT_GRAD_NORM 6       /* float: l2 norm of the last call's finite unscaled gradients */
#define LR_OPT_INV_SCALE 7       /* float: 1 / scale the last call unscaled with */
#define LR_OPT_LR_INDEX 8        /* int: lr index the last call used (before the clamp to the table) */
#define LR_OPT_CONSTS 16         /* per group: float step_size, decay, sqrt(bias_correction2), lr of the last call */
#define LR_OPT_STATE_WORDS (LR_OPT_CONSTS + 4 * LR_OPT_MAX_GROUPS)
typedef struct lr_optim_tensor {
  float* param;
  const void* grad;      /* element type grad_kind, scaled by the loss scale */
  float* exp_avg;
  float* exp_avg_sq;
  int64_t numel;
  int32_t grad_kind;     /* LR_OPT_GRAD_* */
  int32_t group;
} lr_optim_tensor;
typedef struct lr_optim_group {
  double beta1, beta2, eps, weight_decay;
  const float* lr_table; /* device, lr_len entries */
  int32_t lr_len;
  int32_t reserved;
} lr_optim_group;
int lr_amp_adamw_step(const lr_optim_tensor* tensors, int n_tensors, const lr_optim_group* groups, int n_groups, void* state,
                      float* partials, int blocks, float growth_factor, float backoff_factor, int growth_interval, int* launches,
                      lr_stream_t s);

/* ---- LPIPS(alex) of a decoded prediction: AlexNet features on the matrix cores and the learned distance, results left on the device
 *      (added under ABI 30 like lr_eval_metrics: new symbols only, nothing renumbered or re-typed; a library without them fails to
 *      bind, which is the staleness check) ------------------------------------------------------------------------------------------------
 * replaces: `model.loss_fn_alex(pred, origin)` of the evaluation harness and of the task models' validation_step, one sample at a
 *           time with a read-back each --                                                                       test_inpainting.py:159
 *             ref_inpainting_ldm.py:119-146, multiview_ref_inpainting_ldm.py:225-263, NVS_ldm.py:374-401 (`val/lpips`)
 *           together with the composite / crop / area image they are handed (test_inpainting.py:146-155), which is formed inside the
 *           first convolution's gather exactly as lr_eval_metrics forms it and never written to memory; in this tree
 *           leftrefill_amd/evalglue.py: LPIPSAlex.forward, validation_result, and tools/run_inpainting.py (`lpips_fn(...)`).
 * pred, origin, mask, N, H, W, x0, Wc, r: as lr_eval_metrics (pred_kind: LR_EVAL_PRED_*; mask NULL: no composite; r <= LR_EVAL_MAX_R).
 * The scored image is Ho x Wo = H / r x Wc / r.  Stage sizes (height; widths alike), all floor divisions:
 *     h1 = (Ho - 7) / 4 + 1           conv 11 x 11 stride 4 pad 2,  3 ->  64
 *     h2 = (h1 - 3) / 2 + 1           MaxPool(3, 2), conv 5 x 5 pad 2,  64 -> 192
 *     h3 = h4 = h5 = (h2 - 3) / 2 + 1 MaxPool(3, 2), conv 3 x 3 pad 1, 192 -> 384 -> 256 -> 256
 * each followed by ReLU; per stage and pixel sum_c lin_c (fa_c / (|fa| + 1e-10) - fb_c / (|fb| + 1e-10))^2, spatial mean, sum of the
 * five stages -> out [N] fp32.  Activations are fp16 NHWC, accumulation fp32, the head fp32 with fp64 sums.
 * Packing: wt[k] = [Cout_k][Kpad_k] fp16, K index = (ky * ks + kx) * Cin + c (tap-major, channel-minor), Kpad_k = K rounded up to
 * 64 with ZERO weights (363 -> 384 for conv 1; 1600, 1728, 3456, 2304); bias[k] [Cout_k], lin[k] [Cout_k] fp32.  wt / bias 16-byte
 * aligned, workspace 256-byte aligned (LR_E_ALIGN).
 * Workspace (lr_lpips_workspace_bytes; every term rounded up to 256): the five stage outputs 2N * h_k * w_k * Cout_k * 2 bytes, the
 * two pooled maps 2N * h2 * w2 * 64 * 2 and 2N * h3 * w3 * 192 * 2, and 8 bytes per head workgroup: N * sum_k ceil(h_k w_k /
 * LR_LPIPS_HEAD_PIXELS).
 * LR_LPIPS_LAUNCHES = 13 launches (5 conv, 2 pool, 5 head, 1 finish) whatever N and the image size; no atomics, sums in a fixed
 * order: bitwise reproducible, and a sample's score does not depend on the rest of the batch.  No synchronisation, allocation or
 * read-back: capturable on one stream.
 * LR_E_ARG, before any launch: a null pointer, N outside 1 .. 32767, H % r or Wc % r non-zero, a scored side below
 * LR_LPIPS_MIN_SIDE = 31 pixels (some stage would be empty), columns outside the canvas, workspace_bytes below
 * lr_lpips_workspace_bytes (which itself returns LR_E_ARG for such sizes). */
#define LR_LPIPS_LAUNCHES 13
#define LR_LPIPS_MIN_SIDE 31
#define LR_LPIPS_HEAD_PIXELS 64
typedef struct lr_lpips_args {
  const void* pred; int32_t pred_kind; const float* origin; const float* mask;
  int32_t N, H, W, x0, Wc, r;
  const lr_half* wt[5]; const float* bias[5]; const float* lin[5];   /* packed: wt[k] = [Cout][Kpad], tap-major */
  void* workspace; int64_t workspace_bytes;
  float* out;                                                        /* [N] fp32 */
} lr_lpips_args;
int64_t lr_lpips_workspace_bytes(int N, int H, int Wc, int r);
int lr_lpips_alex(const lr_lpips_args* args, lr_stream_t s);

/* ---- assembling a batch from raw decoded images: area shrink, crop, flip, masks and the [-1, 1] mapping in one launch (added under
 *      ABI 30 like lr_eval_metrics: one new symbol, nothing renumbered or re-typed; a library without it fails to bind) -----------------
 * replaces: the per-sample host work of the loaders --
 *             `cv2.resize(..., INTER_AREA)`, the random crop, the flips, `/ 127.5 - 1`       dataloaders/inpainting_dataset.py:68-86, 175-184
 *             `cv2.resize(mask, ..., INTER_NEAREST)`, `clip(m1 + m2, 0, 255)`, `> 127`, the outpainting mask             :88-118, 170-173
 *             the [source | target] canvas with the all-zero left mask                           dataloaders/test_dataset.py:91-105
 *           in this tree dropin/dataloaders/test_dataset.py (resize_area, resize_nearest) and leftrefill_amd/dataprep.py (run_plan_numpy),
 *           whose float64 numpy statement is the yardstick.
 * arena: the batch's raw bytes on the device, images uint8 [h][w][3] and masks uint8 [h][w] packed tightly at any byte offset; the
 * arena itself 16-byte aligned, arena_bytes a multiple of 16 (LR_E_ALIGN).  jobs: n_jobs (<= 65535) lr_prep_job on the device,
 * jobs_host the same table in host memory -- every offset, size and window is checked there before the launch.
 * A job is one S x S tile of the canvas of sample `sample` (tiles tiles wide; tile column `tile`):
 *   image: the source is area-averaged to rh x rw (destination cell i averages the source interval [i r, (i + 1) r) per axis with
 *   coverage weights normalised per axis, fp64) and the S x S window at (y0, x0) of that is kept -- only the window is computed --,
 *   rounded half-to-even to 0 .. 255, flipped left-right with LR_PREP_FLIP_IMAGE, mapped by v / 127.5f - 1.  rh <= img_h and
 *   rw <= img_w: enlarging is LR_E_UNSUPPORTED, as is a window whose source row exceeds LR_PREP_ROW_BYTES - 30 bytes.
 *   mask: outpaint_col >= 0: 1 from that column on; else LR_PREP_ZERO_MASK: 0; else up to two sources (mask_off[q] < 0: absent) read
 *   at the nearest index min((int)(dst * (src / S)), src - 1), summed, clipped to 255, 1 where > 127.  LR_PREP_FLIP_MASK flips the
 *   mask left-right, independent of the image flip.
 *   LR_PREP_HOST: the kernel leaves the tile alone (the caller fills it).
 * image, masked_image [B][S][tiles * S][3], mask [B][S][tiles * S][1] fp32; masked_image = image * (mask < 0.5).
 * One launch, workgroups own (tile, band of output rows); plain stores, no atomics, nothing read back: capturable. */
#define LR_PREP_FLIP_IMAGE 1
#define LR_PREP_FLIP_MASK 2
#define LR_PREP_ZERO_MASK 4
#define LR_PREP_HOST 8
#define LR_PREP_MAX_SIZE 512
#define LR_PREP_ROW_BYTES 24576
typedef struct lr_prep_job {
  int64_t img_off;       /* byte offsets into the arena */
  int64_t mask_off[2];
  int32_t img_h, img_w, rh, rw, y0, x0;
  int32_t mask_h[2], mask_w[2];
  int32_t outpaint_col;  /* -1: none */
  int32_t flags;         /* LR_PREP_* */
  int32_t sample, tile;
} lr_prep_job;
int lr_batch_prep(const uint8_t* arena, int64_t arena_bytes, const lr_prep_job* jobs, const lr_prep_job* jobs_host, int n_jobs, int S,
                  int tiles, int B, float* image, float* masked_image, float* mask, lr_stream_t s);

/* ---- assembling a novel-view-synthesis batch from raw RGBA renders: composite on white, 8-bit bilinear resize, alpha occupancy,
 *      elliptic dilation, stroke / file masks and the [-1, 1] mapping in one launch (added under ABI 30 like lr_batch_prep: one new
 *      symbol, nothing renumbered or re-typed; a library without it fails to bind) -------------------------------------------------------
 * replaces: the per-sample host work of the Objaverse loader --
 *             `imread(UNCHANGED) / 255.`, alpha == 0 -> white, `* 255.` to uint8, `cv2.resize(im, (S, S))`   dataloaders/obj_nvs_dataset.py:117-129
 *             `cv2.resize(alpha > 0, (S, S), INTER_AREA) > 0`, `cv2.dilate(mask, MORPH_ELLIPSE k x k)`, `clip(mask + strokes, 0, 1)`,
 *             the ones mask, the fixed mask file, [cond | target], `/ 127.5 - 1`, `* (mask < 0.5)`, the white right half    :130-189
 *           in this tree leftrefill_amd/nvsprep.py (run_nvs_plan_numpy), whose numpy statement is the yardstick.
 * arena: the batch's raw bytes on the device, 16-byte aligned and a multiple of 16 long; every render (uint8 [h][w][4] RGBA) and
 * plane (uint8 [S][S]) starts at a 16-byte-aligned offset (LR_E_ALIGN).  jobs: B lr_nvs_job on the device, one per sample,
 * jobs_host the same table in host memory -- every offset, size, k and span is checked there before the launch.
 * A job is the S x 2S canvas [cond | target] of sample `sample`:
 *   image, both tiles: a pixel of alpha 0 becomes RGB 255, every other keeps its bytes; then to S x S in integer arithmetic --
 *   h == w == S: copy; h == w == 2S: (a + b + c + d + 2) >> 2 over each 2 x 2 block; else, per axis of n cells,
 *   f = (float)((d + 0.5) * ((double)n / S) - 0.5), s = floor(f), f -= s, (s < 0: s = 0, f = 0; s >= n - 1: s = n - 1, f = 0), taps
 *   s and min(s + 1, n - 1), a0 = rint((1.f - f) * 2048), a1 = rint(f * 2048), R = S0 a0 + S1 a1 along the row,
 *   out = (((b0 (R0 >> 4)) >> 16) + ((b1 (R1 >> 4)) >> 16) + 2) >> 2 down the column; then v / 127.5f - 1.  A render smaller than S on
 *   either axis is LR_E_UNSUPPORTED.
 *   mask, target tile (the cond tile's is 0):
 *     LR_NVS_MODE_ALPHA: occupancy(i, j) = any alpha > 0 over the product of the axes' area taps (per axis: scale = n / S,
 *       f1 = d scale, f2 = f1 + scale, s1 = ceil(f1), s2 = min(floor(f2), n - 1), s1 = min(s1, s2); cells s1 .. s2 - 1, cell s1 - 1
 *       iff s1 - f1 > 1e-3, cell s2 iff f2 - s2 > 1e-3), dilated by the k x k element whose row e has ones in columns
 *       [lo[e], hi[e]), anchor (k / 2, k / 2): dst(y, x) = OR src(y + e - k / 2, x + j - k / 2), outside ignored; 1 <= k <=
 *       LR_NVS_MAX_DILATE, lo[e] < hi[e] <= k (larger k: LR_E_UNSUPPORTED); OR-ed with plane > 0 where plane_off >= 0.
 *     LR_NVS_MODE_ONES: 1.   LR_NVS_MODE_FILE: (float)(plane / 255.0), not thresholded.
 *   masked_image = image * (mask < 0.5 ? 1.f : 0.f); with LR_NVS_REF_WHITE the target tile's is 1.f * (mask < 0.5 ? 1.f : 0.f).
 * image, masked_image [B][S][2S][3], mask [B][S][2S][1] fp32.  S <= LR_NVS_MAX_SIZE.
 * One launch, workgroups own (sample, tile, band of output rows); plain stores, no atomics, nothing read back: capturable. */
#define LR_NVS_MODE_ALPHA 0
#define LR_NVS_MODE_ONES 1
#define LR_NVS_MODE_FILE 2
#define LR_NVS_REF_WHITE 1
#define LR_NVS_MAX_SIZE 512
#define LR_NVS_MAX_DILATE 32
typedef struct lr_nvs_job {
  int64_t cond_off, target_off;   /* byte offsets into the arena, multiples of 16 */
  int64_t plane_off;              /* -1: none */
  int32_t cond_h, cond_w, target_h, target_w;
  int32_t mode;                   /* LR_NVS_MODE_* */
  int32_t k;                      /* side of the dilation element (LR_NVS_MODE_ALPHA) */
  int32_t flags;                  /* LR_NVS_REF_WHITE */
  int32_t sample;
  uint8_t lo[LR_NVS_MAX_DILATE], hi[LR_NVS_MAX_DILATE];
} lr_nvs_job;
int lr_nvs_prep(const uint8_t* arena, int64_t arena_bytes, const lr_nvs_job* jobs, const lr_nvs_job* jobs_host, int B, int S,
                float* image, float* masked_image, float* mask, lr_stream_t s);

/* ---- Pillow's 8-bit resampler and the inpainting canvas of the one-call route (leftrefill_amd/refill.py) on the device (added under
 *      ABI 30 like lr_batch_prep: two new symbols, nothing renumbered or re-typed; a library without them fails to bind) ----------------
 * replaces: the host image work of the reference's interactive entry point --
 *             `Image.resize((512, 512), BICUBIC)` of source and reference, `BILINEAR` of the mask         ref_inpainting_gradio.py:168-170
 *             `r.resize((int(512 / ratio), 512), BICUBIC)` of every result                                                            :207
 *             `init_mask[init_mask > 0] = 255`, `pad_image` (np.pad mode='edge'), the [reference | source] stitch        :142-145, 171-188
 *             `convert("L") / 255.0`, `< 0.5 -> 0, >= 0.5 -> 1`, `/ 127.5 - 1.0`, `image * (mask < 0.5)`, the n copies             :54-79
 *           in this tree leftrefill_amd/refill.py (pil_coeffs, resize_u8, prepare_numpy), whose numpy statement is pinned against Pillow
 *           itself and is the yardstick.  The tail (composite, crop, 8-bit) is lr_eval_metrics with x0 = Wc = W, r = 1.
 * lr_pil_resize: n_jobs (1 .. 65535) independent `Image.resize` jobs in at most two launches.
 *   src: a byte arena on the device, 16-byte aligned (LR_E_ALIGN); a job's source is uint8 [hs][ws][c], c in {1, 3}, packed at ANY byte
 *   offset src_off.  tables: an int32 arena on the device and the same words in host memory (tables_host).  A pass along an axis of
 *   n_in cells to n_out cells has at word offset h_off / v_off: lo[n_out], cnt[n_out], kk[n_out][ksize], computed on the host in double
 *   arithmetic (Pillow's precompute_coeffs + normalize_coeffs_8bpc): scale = n_in / n_out, fs = max(scale, 1), support = S_f fs (S_f = 2
 *   bicubic, 1 bilinear), ksize = (int)ceil(support) * 2 + 1; per output index i: center = (i + 0.5) scale,
 *   lo = max((int)(center - support + 0.5), 0), cnt = min((int)(center + support + 0.5), n_in) - lo,
 *   w[x] = f((x + lo - center + 0.5) * (1 / fs)), summed in index order and divided by a non-zero sum,
 *   kk = (int)(w < 0 ? -0.5 + w 2^22 : 0.5 + w 2^22); bicubic f(|x|), a = -0.5: ((a + 2) x - (a + 3)) x x + 1 below 1,
 *   (((x - 5) x + 8) x - 4) a below 2, else 0; bilinear: 1 - x below 1, else 0.
 *   One pass: out[i] = clamp((2^21 + sum_{j < cnt[i]} kk[i][j] in[lo[i] + j]) >> 22, 0, 255) per channel, arithmetic shift, 32-bit
 *   accumulation (sum |kk| < 1.4 * 2^22 for both filters, times 255 stays below 2^31).
 *   Launch 1: the horizontal pass of every job that has one (h_ksize > 0; wd == ws otherwise), into the workspace at tmp_off when a
 *   vertical pass follows, else straight to dst.  Launch 2: the vertical pass (v_ksize > 0; hd == hs otherwise) from the workspace or
 *   the source, or -- neither pass -- the copy.  Jobs of different sizes share a launch; a launch no job needs is not made.
 *   jobs on the device, jobs_host the same table in host memory: every offset, size, window, ksize and lo + cnt <= n_in is checked
 *   there before any launch.  LR_E_ARG: a null pointer, n_jobs out of range, c not 1 or 3, a side outside 1 .. 2^20, a window outside its
 *   buffer, a skipped pass whose sizes differ, a table row outside the axis.  LR_E_UNSUPPORTED: ksize > LR_PIL_MAX_KSIZE = 1025, which admits shrinking by
 *   up to 256 x under bicubic and 512 x under bilinear (16384 -> 64 bicubic is ksize 1025: served).
 * lr_refill_canvas: ref, src, mask uint8 [P][Sh][Sw][3] (resize destinations of P pairs) -> the batch of P n canvases H x 2W
 *   [reference | source], each pair's n copies adjacent: edge pad v(y, x) = in[min(y, Sh - 1)][min(x, Sw - 1)] (Sh <= H, Sw <= W);
 *   image = (float)v / 127.5f - 1 [P n][3][H][2W]; mask [P n][1][H][2W]: 0 on the left half, on the right every channel of the mask
 *   pixel first becomes (> 0 ? 255 : 0), then L = (19595 R + 38470 G + 7471 B + 32768) >> 16, 1 where L >= 128;
 *   masked_image = image * (mask < 0.5 ? 1.f : 0.f).  One launch; 1 <= P, H <= 65535, n >= 1 (LR_E_ARG).
 * Plain integer code with plain vector stores, no atomics, nothing read back: capturable, bitwise reproducible. */
#define LR_PIL_MAX_KSIZE 1025
typedef struct lr_pil_job {
  int64_t src_off;       /* byte offset of the source in the src arena */
  int64_t tmp_off;       /* byte offset of the [hs][wd][c] intermediate in the workspace (both passes run) */
  int64_t dst_off;       /* byte offset of the [hd][wd][c] result in dst */
  int64_t h_off, v_off;  /* word offsets of the passes' lo / cnt / kk in the table arena */
  int32_t hs, ws, hd, wd, c;
  int32_t h_ksize, v_ksize; /* 0: the pass is skipped */
  int32_t reserved;
} lr_pil_job;
int lr_pil_resize(const uint8_t* src, int64_t src_bytes, const int32_t* tables, const int32_t* tables_host, int64_t table_words,
                  uint8_t* work, int64_t work_bytes, uint8_t* dst, int64_t dst_bytes, const lr_pil_job* jobs,
                  const lr_pil_job* jobs_host, int n_jobs, lr_stream_t s);
int lr_refill_canvas(const uint8_t* ref, const uint8_t* src, const uint8_t* mask, int P, int Sh, int Sw, int H, int W, int n,
                     float* image, float* masked_image, float* mask_out, lr_stream_t s);

/* ---- the training logger's image grid and token drift (leftrefill_amd/imagelog.py, dropin inpainting_ldm/logger.py) on the device (added
 *      under ABI 30 like lr_batch_prep: two new symbols, nothing renumbered or re-typed; a library without them fails to bind) -------------
 * replaces: the host work of the reference's image logger --
 *             `.detach().cpu()`, `torch.clamp(-1, 1)` of every logged batch                               inpainting_ldm/logger.py:93-98
 *             `torchvision.utils.make_grid(images[k], nrow=1)`, `(grid + 1.0) / 2.0`, the transposes,
 *             `(grid * 255).astype(np.uint8)`, `np.concatenate(grids, axis=1)`                                                  :60-67
 *             `sqrt(sum((old[j] - weight[j])**2)).item()` per token and the re-clone of the snapshot                         :118-123
 *           in this tree leftrefill_amd/imagelog.py (grid_numpy, token_drift_numpy) states the arithmetic and is the yardstick.
 * lr_image_grid: n_sources (1 .. LR_GRID_MAX_SOURCES) batches of N images, H rows each -> ONE uint8 canvas out [Hc][Wc][3] in one launch.
 *   N == 1: Hc = H and a source of width W owns the canvas columns col .. col + W - 1 (make_grid returns a single image unpadded).
 *   N > 1:  Hc = N (H + 2) + 2 and a source owns col .. col + W + 3: image k at canvas rows k (H + 2) + 2 .., columns col + 2 ..;
 *           every other pixel of the canvas, the columns no source owns included, is padding (value 0).
 *   A source is read in place through its ELEMENT strides: value(k, c, y, x) = ptr[k stride_n + c stride_c + y stride_h + x stride_w] of
 *   kind LR_EVAL_PRED_F32 / _F16 / _BF16 (16-bit values are widened to fp32 first); C == 1 is repeated to three channels.  An NHWC view
 *   (stride_c = 1, stride_w = 3) and an NCHW tensor share a launch; the caller vouches that N, C, H, W and the strides stay inside the
 *   source's buffer.
 *   Per byte, fp32, in this order and never contracted: v = clamp ? min(max(v, -1), 1) : v;  v = rescale ? (v + 1) / 2 : v;  v = v * 255;
 *   truncation towards zero (padding: grey 127 with rescale, 0 without).  Without clamp, what falls outside 0 .. 255 saturates and a
 *   NaN's byte is unspecified (the numpy statement refuses both); with clamp a NaN becomes 0.
 *   out needs no alignment: bytes in front of the first and behind the last 4-byte-aligned address are byte stores, the rest dword stores.
 *   LR_E_ARG, before any launch: a null pointer, n_sources outside 1 .. LR_GRID_MAX_SOURCES, N < 1, H < 1, Wc < 1, a kind outside the
 *   three, C outside {1, 3}, W < 1, a column range that leaves 0 .. Wc - 1 or overlaps another source's, a canvas of 2^31 bytes or more.
 * lr_token_drift: old_, new_ fp32 [T][D], contiguous and distinct -> out[t] = sqrt(sum_d (old_[t][d] - new_[t][d])^2), fp32, summed in a
 *   fixed order (lane l of one wave adds elements l, l + 64, ... -- groups of four when D % 4 == 0 and both pointers are 16-byte aligned --
 *   then a butterfly over the lanes), and new_ copied into old_ in the same pass.  LR_E_ARG: a null pointer, T < 1, D < 1, old_ == new_.
 * Plain vector and byte stores from C++, no atomics, no allocation, nothing read back: capturable, bitwise reproducible. */
#define LR_GRID_MAX_SOURCES 8
typedef struct lr_grid_source {
  const void* ptr;       /* element (0, 0, 0, 0) of the batch */
  int32_t kind;          /* LR_EVAL_PRED_F32 | _F16 | _BF16 */
  int32_t C;             /* 1 | 3 */
  int32_t W;             /* image width */
  int32_t col;           /* first canvas column of this source's grid (its padding included) */
  int64_t stride_n, stride_c, stride_h, stride_w;   /* in elements */
} lr_grid_source;
int lr_image_grid(const lr_grid_source* sources, int n_sources, int N, int H, int clamp, int rescale, uint8_t* out, int Wc, lr_stream_t s);
int lr_token_drift(float* old_, const float* new_, int T, int D, float* out, lr_stream_t s);

/* ---- attention-map probe (leftrefill_amd/attnprobe.py, the `return_attn` surface of the drop-in; csrc/attention_probe.hip) (added
 *      under ABI 30 like lr_image_grid: two new symbols, nothing renumbered or re-typed; a library without them fails to bind) ------------
 * replaces: the commented-out `q @ k^T` score computation of the reference's attention modules       multiview_attention.py:333-343, 357-358
 *
 *   out[b, i, c] = beta * out[b, i, c]
 *                + alpha * (1/heads) * sum_h  sum_j softmax_j(scale * q_h[b,i,:] . k_h[b,j,:]) * cols[j, c]
 *
 * i.e. attention with a tiny V that all samples and heads share, head-averaged; the L x L matrix is never materialised.
 *   q, k: 16-bit, [B*Nq, >= heads*64] / [B*Nkv, >= heads*64] with row strides ldq / ldk (multiples of 8, 16-byte aligned pointers:
 *         LR_E_ALIGN) and unit column stride -- column slices of a fused projection as lr_attention_f16 takes them; d_head = 64.
 *   cols: the probe columns, 16-bit in the compute type, [Nkv][ldc] with 1 <= ncols <= 8 and ldc >= ncols (LR_E_ARG), 2-byte aligned.
 *   out:  fp32 [B][Nq][ncols], contiguous, 4-byte aligned.  beta == 0: out is not read (it may hold NaNs).
 *   Any Nq >= 1, Nkv >= 1 (LR_E_ARG otherwise, as for a null pointer); key and query tails are masked as in lr_attention_f16.
 * QK^T and the online softmax are those of lr_attention_f16 (scale folded into Q); a block keeps its 128 queries for all heads,
 * normalises each head by its own row sum and adds the head terms in head order in fp32: no atomics, no workspace, bit-identical
 * from run to run, capturable. */
int lr_attention_probe_f16(const lr_half* q, int ldq, const lr_half* k, int ldk, const lr_half* cols, int ldc, int ncols, float* out,
                           int B, int heads, int Nq, int Nkv, float scale, float alpha, float beta, lr_stream_t s);
int lr_attention_probe_bf16(const lr_half* q, int ldq, const lr_half* k, int ldk, const lr_half* cols, int ldc, int ncols, float* out,
                            int B, int heads, int Nq, int Nkv, float scale, float alpha, float beta, lr_stream_t s);

/* ---- LoRA on the attention / GEGLU Linears (added under ABI 30; csrc/lora.hip) ---------------------------------------------------------
 * replaces: LoraInjectedLinear.forward (inpainting_ldm/lora.py:28-33) `linear(x) + lora_up(lora_down(x)) * scale` and its autograd
 *           backward for the factors, and, for sampling, the fold W + scale * up . down into the weight the packers read.
 * R is the PADDED rank of the 16-bit kernels: 32 or 64 (LR_E_UNSUPPORTED otherwise); the caller pads the factors with zero rows / columns.
 * 16-bit operands: unit column stride, row strides multiples of 8, 16-byte aligned pointers (LR_E_ALIGN); K, N, C multiples of 8; any M >= 1.
 *
 *   lr_lora_down   t[M][R] = 16-bit(alpha * x[M][K] . a[R][K]^T)            fp32 accumulation on the matrix cores, one rounding
 *   lr_lora_up     y[M][N] = 16-bit((accumulate ? y : 0) + t[M][R] . u[N][R]^T)   fp32 add to the stored y, one rounding; ldy >= N lets a
 *                            call land in a column range of a wider buffer
 *   lr_lora_wgrad  d[R][C] = alpha * p[M][R]^T . q[M][C]  (fp32, row stride ldd % 4 == 0)   the sum over the M rows is split over
 *                            workgroups into fp32 partials in `workspace` (>= lr_lora_wgrad_workspace_bytes(M, R, C) bytes, 16-byte
 *                            aligned; LR_E_ARG when smaller) and added in split order by a second launch: no atomics, bit-identical from
 *                            run to run; the split is a function of (M, C) alone
 *   lr_lora_merge_f32  w_eff[N][K] = w[N][K] + alpha * b[N][R] . a[R][K]   all fp32, contiguous, 1 <= R <= 64 (the TRUE rank, no padding),
 *                            K % 4 == 0; terms added in r order by fmaf; an element whose low-rank sum is zero (up == 0)
 *                            keeps the bits of w; w_eff may be w. */
int lr_lora_down_f16(const lr_half* x, int ldx, const lr_half* a, int lda, lr_half* t, int ldt, int M, int K, int R, float alpha, lr_stream_t s);
int lr_lora_up_f16(const lr_half* t, int ldt, const lr_half* u, int ldu, lr_half* y, int ldy, int M, int N, int R, int accumulate, lr_stream_t s);
int64_t lr_lora_wgrad_workspace_bytes(int M, int R, int C);
int lr_lora_wgrad_f16(const lr_half* p, int ldp, const lr_half* q, int ldq, float* d, int ldd, int M, int R, int C, float alpha,
                      void* workspace, int64_t workspace_bytes, lr_stream_t s);
int lr_lora_merge_f32(const float* w, const float* b, const float* a, float* w_eff, int N, int K, int R, float alpha, lr_stream_t s);
int lr_lora_down_bf16(const lr_half* x, int ldx, const lr_half* a, int lda, lr_half* t, int ldt, int M, int K, int R, float alpha, lr_stream_t s);
int lr_lora_up_bf16(const lr_half* t, int ldt, const lr_half* u, int ldu, lr_half* y, int ldy, int M, int N, int R, int accumulate, lr_stream_t s);
int lr_lora_wgrad_bf16(const lr_half* p, int ldp, const lr_half* q, int ldq, float* d, int ldd, int M, int R, int C, float alpha,
                       void* workspace, int64_t workspace_bytes, lr_stream_t s);

/* ---- LoRA dropout: the mask of `dropout(lora_up(lora_down(x)))` regenerated inside the three LoRA kernels (added under ABI 30 like the
 *      entries above: six new symbols, nothing renumbered or re-typed; a library without them fails to bind; csrc/lora.hip) --------------
 * replaces: the nn.Dropout of LoraInjectedLinear (inpainting_ldm/lora.py:21, 32) on the [M, N] low-rank branch, forward and backward,
 *           without a [M, N] temporary or a stored mask.
 * The mask (leftrefill_amd/lora_dropout.py states it on the host):
 *   keep(row, col) = philox4x32_10(counter (row, col >> 2, stream, draw), key (seed & 0xffffffff, seed >> 32))[col & 3] >= threshold
 * row: the row of the masked [M, N] operand; col: the layer's LOGICAL output feature.  The kernels see columns as they lie in memory,
 * relative to the pointer they are given (a slice of a fused buffer starts at column 0); colgrp, a device table of N / 4 (C / 4, K / 4)
 * int32 entries, names the logical group of four columns behind each stored group of four (the GEGLU row interleave), NULL = identity.
 * threshold = min(2^32 - 1, floor(p 2^32)); inv_keep = 1 / (1 - p) as fp32: finite, >= 1 and within 1e-3 (relative) of
 * 1 / (1 - threshold / 2^32), LR_E_ARG otherwise.  A mask only zeroes a 16-bit value; inv_keep is applied in fp32.
 * Argument rules otherwise as the unmasked entries; threshold 0 with inv_keep 1 gives their bits.
 *
 *   lr_lora_up_drop     y = 16-bit((accumulate ? y : 0) + (keep ? inv_keep * t . u^T : 0)); a dropped element under `accumulate` keeps
 *                       y's bits.  (row, col) = y's own, col relative to `y`.
 *   lr_lora_down_drop   t = 16-bit(alpha * (x (.) keep) . a^T): the mask on the wide operand at x's own (row, col) -- the backward's
 *                       dT = scale inv_keep (g (.) keep) up with alpha = scale * inv_keep.
 *   lr_lora_wgrad_drop  d = alpha * p^T . (q (.) keep): the mask on q's own (row, col); split plan, workspace and sum order as
 *                       lr_lora_wgrad (bit-identical from run to run). */
typedef struct lr_lora_drop {
  uint64_t seed;
  uint32_t stream, draw, threshold;
  float inv_keep;
  const int32_t* colgrp;
} lr_lora_drop;
int lr_lora_down_drop_f16(const lr_half* x, int ldx, const lr_half* a, int lda, lr_half* t, int ldt, int M, int K, int R, float alpha,
                          const lr_lora_drop* drop, lr_stream_t s);
int lr_lora_up_drop_f16(const lr_half* t, int ldt, const lr_half* u, int ldu, lr_half* y, int ldy, int M, int N, int R, int accumulate,
                        const lr_lora_drop* drop, lr_stream_t s);
int lr_lora_wgrad_drop_f16(const lr_half* p, int ldp, const lr_half* q, int ldq, float* d, int ldd, int M, int R, int C, float alpha,
                           void* workspace, int64_t workspace_bytes, const lr_lora_drop* drop, lr_stream_t s);
int lr_lora_down_drop_bf16(const lr_half* x, int ldx, const lr_half* a, int lda, lr_half* t, int ldt, int M, int K, int R, float alpha,
                           const lr_lora_drop* drop, lr_stream_t s);
int lr_lora_up_drop_bf16(const lr_half* t, int ldt, const lr_half* u, int ldu, lr_half* y, int ldy, int M, int N, int R, int accumulate,
                         const lr_lora_drop* drop, lr_stream_t s);
int lr_lora_wgrad_drop_bf16(const lr_half* p, int ldp, const lr_half* q, int ldq, float* d, int ldd, int M, int R, int C, float alpha,
                            void* workspace, int64_t workspace_bytes, const lr_lora_drop* drop, lr_stream_t s);

/* ---- FID features and statistics on the device: the pool3 features of pytorch-fid's Inception network and the float64 sums of a set
 *      (added under ABI 30 like lr_lpips_alex: four new symbols, no struct, nothing renumbered or re-typed; a library without them
 *      fails to bind; csrc/inception.hip) -----------------------------------------------------------------------------------------------
 * replaces: the outside program the reference leaves FID to -- its harnesses only write every prediction to disk "for fid metric"
 *           (test_inpainting.py --save_single, test_multiview_inpainting.py); in this tree leftrefill_amd/fid.py states the network
 *           (FIDInception), the table (FID_PROGRAM) and the distance, and its float64 form is the yardstick.  Parity-unpinned: neither
 *           pytorch-fid nor its weights are available to this tree.
 * lr_fid_input: N source images -> dst fp16 NHWC [N][out][out][4] (8-byte aligned: LR_E_ALIGN), channel 3 zero, one launch.
 *   kind LR_FID_SRC_U8: src uint8 [N][H][W][3]; kind LR_EVAL_PRED_F32 / _F16 / _BF16: src [N][3][H][W] in [-1, 1], first made 8-bit as
 *   lr_eval_metrics makes its rgb8: v = mask ? v * m + origin * (1 - m) : v (fp32, not contracted; mask [N][1][H][W], origin
 *   [N][3][H][W] fp32, both NULL for no composite), b = (uint8_t)((min(max(v, -1), 1) + 1) / 2 * 255).  Columns [x0, x0 + Wc) are the
 *   image.  From the bytes on in float64 (2 v - 1 cancels around mid-grey, where the stored fp16 is finer than fp32 arithmetic near 1):
 *   p = b / 255; per axis of n_in cells: f = max(0, (d + 0.5) * ((double)n_in / out) - 0.5), i0 = min((int)f, n_in - 1),
 *   i1 = min(i0 + 1, n_in - 1), l = f - i0; v = (1 - ly) ((1 - lx) p00 + lx p01) + ly ((1 - lx) p10 + lx p11); stored fp16(2 v - 1).
 *   F.interpolate(mode='bilinear', align_corners=False) without antialiasing, whether it enlarges or shrinks.
 * lr_fid_run: an interpreter over `program`, n_rows rows of LR_FID_ROW_WORDS int32 words in HOST memory (words LR_FID_*), for a batch
 *   of B images.  An activation is a region [B][H][W][ld] of fp16 in `arena`; a row names a region by its offset PER IMAGE in halves
 *   (multiplied by B here, so one table serves every batch size; a multiple of 8), its channel stride ld and the first channel c0 it
 *   reads / writes.  LR_FID_OP_CONV: out[.., c0 + o] = fp16(relu(bias[o] + sum_{ky, kx, c} wt[o][(ky kw + kx) Cin + c] in[.., c])),
 *   fp32 accumulation on the matrix cores; kh x kw in {1x1, 3x3, 5x5, 1x7, 7x1, 1x3, 3x1}, stride 1 | 2, pads ph < kh, pw < kw,
 *   Cin the STORED channels per tap (a multiple of 8, or 4), wt fp16 [Cout][Kpad] at W_OFF halves (a multiple of 8) of `wt`, Kpad =
 *   kh kw Cin rounded up to 64 with zero weights, bias fp32 [Cout] at B_OFF floats (a multiple of 4) of `bias`; Cout, c0 and ld of
 *   the destination multiples of 4.  LR_FID_OP_MAXPOOL_S2: MaxPool(3, 2), floor, no padding; LR_FID_OP_MAXPOOL_S1: MaxPool(3, 1, 1),
 *   padding never wins; LR_FID_OP_AVGPOOL_S1: AvgPool(3, 1, 1, count_include_pad=False), fp32 sum in (dy, dx) order; C, c0 and ld
 *   multiples of 8.  Channels of the destination outside [c0, c0 + Cout) keep their bits.  HOUT / WOUT must equal
 *   (in + 2 pad - k) / stride + 1.  EVERY row is checked before the first launch against arena_halfs, wt_halfs and bias_floats:
 *   LR_E_ARG for an unknown op, a negative word, a size or range that breaks the rules above, a region, weight or bias range past its
 *   buffer, B outside 1 .. 32767; arena, wt, bias 16-byte aligned (LR_E_ALIGN).  Then one launch per row, in order, on one stream.
 * lr_fid_head: src [B][HW][ld] fp16 -> out [B][C] fp32, the mean over the HW pixels added in index order.  One launch.
 * lr_fid_accumulate: feats fp32 [n][D] (D a multiple of 64) -> sum[D] += sum_r f_r, gram[D][D] += sum_r f_r f_r^T in float64; every
 *   element is owned by one thread and the rows are added in order, each product exact.  One launch; a second call accumulates.
 * launches: host counter incremented once per kernel launch, or NULL.  No atomics, no allocation, no synchronisation, nothing read
 * back: capturable, bitwise reproducible, and an image's features do not depend on the rest of the batch. */
#define LR_FID_SRC_U8 3          /* kind of lr_fid_input next to LR_EVAL_PRED_* */
#define LR_FID_OP_CONV 1
#define LR_FID_OP_MAXPOOL_S2 2
#define LR_FID_OP_MAXPOOL_S1 3
#define LR_FID_OP_AVGPOOL_S1 4
#define LR_FID_ROW_WORDS 24
#define LR_FID_OP 0
#define LR_FID_SRC_OFF 1
#define LR_FID_SRC_LD 2
#define LR_FID_SRC_C0 3
#define LR_FID_DST_OFF 4
#define LR_FID_DST_LD 5
#define LR_FID_DST_C0 6
#define LR_FID_HIN 7
#define LR_FID_WIN 8
#define LR_FID_CIN 9
#define LR_FID_HOUT 10
#define LR_FID_WOUT 11
#define LR_FID_COUT 12
#define LR_FID_KH 13
#define LR_FID_KW 14
#define LR_FID_STRIDE 15
#define LR_FID_PH 16
#define LR_FID_PW 17
#define LR_FID_W_OFF 18
#define LR_FID_B_OFF 19
#define LR_FID_KPAD 20           /* words 21 .. 23: reserved, zero */
int lr_fid_input(const void* src, int kind, const float* origin, const float* mask, int N, int H, int W, int x0, int Wc, lr_half* dst,
                 int out, int* launches, lr_stream_t s);
int lr_fid_run(const int32_t* program, int n_rows, int B, lr_half* arena, int64_t arena_halfs, const lr_half* wt, int64_t wt_halfs,
               const float* bias, int64_t bias_floats, int* launches, lr_stream_t s);
int lr_fid_head(const lr_half* src, int B, int HW, int C, int ld, float* out, int* launches, lr_stream_t s);
int lr_fid_accumulate(const float* feats, int n, int D, double* sum, double* gram, int* launches, lr_stream_t s);

/* ---- seeded sampling noise: per-sample Philox normals (added under ABI 30 like lr_eval_metrics: one new symbol, nothing renumbered or
 *      re-typed; a library without it fails to bind; csrc/seeded_noise.hip) -------------------------------------------------------------
 * replaces: the `torch.randn` / `randn_like` / `noise_like` draws of the samplers when the caller passes `seeds=` -- the start code
 *           (ddim.py:235, 489; ddpm.py:1013, 1066), the noise of every step (ddim.py:378, 642; ddpm.py:986), the q_sample noise of the
 *           known region in the masked loops (ddpm.py:368 under ddim.py:259, 517 and ddpm.py:1046, 1094), stochastic_encode (ddim.py:447) and the
 *           VAE posterior sample (distributions.py:36-39); leftrefill_amd/noise.py states it (normal_numpy, float64) and is the yardstick.
 * keys [B][2]: the uint64 seed bits and the sub-sample number (low 32 bits used) of every sample, in DEVICE memory.  stream, step: the
 * uint32 names of the draw, passed as their int32 bits.  out [B][per_sample] fp32, 4-byte aligned (LR_E_ALIGN).  Element i of sample b,
 * g = i >> 2:
 *   w0..w3 = philox4x32_10(counter = (g, sub_b, step, stream), key = (seed_b & 0xffffffff, seed_b >> 32))
 *   u(w) = ((w >> 9) + 0.5) 2^-23 (exact in fp32);  pair p in {0, 1}: r = sqrtf(-2 logf(u(w[2p]))), (z[4g + 2p + 1], z[4g + 2p]) =
 *   r * sincospif(2 u(w[2p+1])) -- the accurate forms, the argument of sincospif exact.
 * One launch.  A value depends on (key, stream, step, i) alone: not on B, the row's place in the batch, per_sample, the alignment of
 * `out` (16-byte stores where out + b per_sample is 16-byte aligned, scalar stores for a row's tail and for unaligned rows) or anything
 * run before.  LR_E_ARG, before any launch: a null pointer, B <= 0, per_sample <= 0, per_sample / 4 >= 2^32. */
int lr_seeded_normal(const int64_t* keys, int B, int64_t per_sample, int32_t stream, int32_t step, float* out, lr_stream_t s);

/* ---- bfloat16 twins: same signatures and semantics as the fp16 entry points above, every lr_half is bfloat16 bits -------- */
int lr_groupnorm_stats_bf16(const lr_half* x1, int C1, const lr_half* x2, int C2, int N, int HW, float* partials,
    lr_stream_t s);
int lr_groupnorm_apply_bf16(const lr_half* x1, int C1, const lr_half* x2, int C2, int N, int HW, const float*
    partials, const float* gamma, const float* beta, float eps, int silu, lr_half* y, lr_stream_t s);
int lr_groupnorm_apply_n_bf16(const lr_half* x1, int C1, const lr_half* x2, int C2, int N, int HW, const float*
    partials, int nchunks, const float* gamma, const float* beta, float eps, int silu, lr_half* y, lr_stream_t s);
int lr_layernorm_bf16(const lr_half* x, const float* gamma, const float* beta, float eps, lr_half* y, int M, int C,
    lr_stream_t s);
int lr_layernorm_bwd_bf16(const lr_half* x, const lr_half* dy, const float* gamma, float eps, lr_half* dx, int M, int
    C, lr_stream_t s);
int lr_groupnorm_bwd_bf16(const lr_half* x1, int C1, const lr_half* x2, int C2, const lr_half* dy, int N, int HW,
    const float* fwd_partials, const float* gamma, const float* beta, float eps, int silu, float* bwd_partials,
    lr_half* dx1, lr_half* dx2, lr_stream_t s);
int lr_layernorm_bwd_res_bf16(const lr_half* x, const lr_half* dy, const lr_half* dres, const float* gamma, float eps, lr_half*
    dx, int M, int C, lr_stream_t s);
int lr_groupnorm_bwd_res_bf16(const lr_half* x1, int C1, const lr_half* x2, int C2, const lr_half* dy, const lr_half* dres1,
    const lr_half* dres2, int N, int HW, const float* fwd_partials, int fwd_chunks, const float* gamma, const float* beta,
    float eps, int silu, float* bwd_partials, lr_half* dx1, lr_half* dx2, lr_stream_t s);
int lr_nchw_f32_to_nhwc_bf16(const float* x1, int C1, const float* x2, int C2, lr_half* y, int Cpad, int N, int H, int
    W, lr_stream_t s);
int lr_nhwc_f16_to_nchw_bf16(const lr_half* y, int Cstride, int C, void* out_nchw, int out_is_f32, int N, int H, int W,
    lr_stream_t s);
int lr_timestep_embedding_bf16(const int64_t* t, int N, int dim, lr_half* out, lr_stream_t s);
int lr_timestep_embedding_f32_bf16(const float* t, int N, int dim, lr_half* out, lr_stream_t s);
int lr_linear_small_m_bf16(const lr_half* a, int lda, const lr_half* w, const float* bias, lr_half* out, int ldo, int
    M, int N, int K, int act_in, int act_out, lr_stream_t s);
int lr_mv_gather_bf16(const lr_half* x, lr_half* seq, int b, int v, int s, int C, lr_stream_t st);
int lr_mv_scatter_bf16(const lr_half* seq, lr_half* x, int b, int v, int s, int C, lr_stream_t st);
int lr_ddim_cfg_step_bf16(const float* x, const void* eps, int eps_is_f32, const float* noise, float* x_prev, float*
    pred_x0, int64_t numel, float cfg_scale, float a_t, float a_prev, float sigma_t, float sqrt_one_minus_at,
    lr_stream_t s);
int lr_plms_cfg_step_bf16(const float* x, const void* eps, int eps_is_f32, const float* const* hist, int n_hist, const float*
    weights, float divisor, float* e_out, float* x_prev, float* pred_x0, int64_t numel, float cfg_scale, float a_t, float a_prev,
    float sqrt_one_minus_at, lr_stream_t s);
int lr_dpmpp_cfg_step_bf16(const float* x, const void* eps, int eps_is_f32, const float* x0_prev, float* x0_out, float* x_next,
    int64_t numel, float cfg_scale, float sigma_s, float alpha_s, float ratio, float c, float c_half, float inv_r0, lr_stream_t s);
int lr_ddim_inv_cfg_step_bf16(const float* x, const void* eps, int eps_is_f32, float* x_next, int64_t numel, float cfg_scale,
    float c1, float c2, lr_stream_t s);
int lr_ddim_cfg3_step_bf16(const float* x, const void* eps, int eps_is_f32, const float* noise, float* x_prev, float* pred_x0,
    int64_t numel, float cfg_scale, float cond_weight, float one_minus_cond_weight, float a_t, float a_prev, float sigma_t,
    float sqrt_one_minus_at, lr_stream_t s);
int lr_ddpm_step_bf16(const float* x, const void* eps, int eps_is_f32, const float* noise, const float* known_x0,
    const float* known_noise, const float* mask, int64_t mask_chw, int64_t mask_hw, int clip_denoised, float* x_prev,
    float* x0_out, int64_t numel, float sqrt_recip_ac, float sqrt_recipm1_ac, float coef1, float coef2, float sigma,
    float sqrt_ac, float sqrt_one_minus_ac, lr_stream_t s);
int lr_geglu_fwd_bf16(const lr_half* pre, lr_half* out, int M, int H, lr_stream_t s);
int lr_geglu_bwd_bf16(const lr_half* pre, const lr_half* dy, lr_half* dpre, int M, int H, lr_stream_t s);
int lr_sumpool2x2_bf16(const lr_half* x, lr_half* y, int N, int H, int W, int C, lr_stream_t s);
int lr_mv_gather_bwd_bf16(const lr_half* dseq, lr_half* dx, int b, int v, int s, int C, lr_stream_t st);
int lr_mv_scatter_bwd_bf16(const lr_half* dx, lr_half* dseq, int b, int v, int s, int C, lr_stream_t st);
int lr_gn_conv_out_bf16(const lr_half* x, int B, int H, int W, int C, const float* gpart, int chunks, const float* gamma, const float* beta,
                        float eps, const lr_half* w, int ldw, const float* bias, int Cout, lr_half* y, lr_stream_t s);
int lr_attention_bf16(const lr_half* q, int ldq, const lr_half* k, int ldk, const lr_half* v, int ldv, lr_half* o, int
    ldo, int B, int heads, int Nq, int Nkv, float scale, lr_stream_t s);
int lr_attention_causal_bf16(const lr_half* q, int ldq, const lr_half* k, int ldk, const lr_half* v, int ldv, lr_half*
    o, int ldo, int B, int heads, int N, float scale, lr_stream_t s);
int lr_attention_lse_bf16(const lr_half* q, int ldq, const lr_half* k, int ldk, const lr_half* v, int ldv, lr_half* o,
    int ldo, float* lse, int B, int heads, int Nq, int Nkv, float scale, lr_stream_t s);
int lr_attention_vt_bf16(const lr_half* q, int ldq, const lr_half* k, int ldk, const lr_half* vt, int ld_vt, lr_half*
    o, int ldo, int B, int heads, int Nq, int Nkv, float scale, lr_stream_t s);
int lr_transpose_v_bf16(const lr_half* v, int ldv, lr_half* vt, int ld_vt, int B, int heads, int Nkv, lr_stream_t s);
int lr_attention_bwd_bf16(const lr_attn_bwd_args* args, lr_stream_t s);
int lr_attention_causal_lse_bf16(const lr_half* q, int ldq, const lr_half* k, int ldk, const lr_half* v, int ldv, lr_half* o,
    int ldo, float* lse, int B, int heads, int N, float scale, lr_stream_t s);
int lr_attention_causal_bwd_bf16(const lr_attn_bwd_args* args, lr_stream_t s);
int lr_gelu_fwd_bf16(const lr_half* pre, lr_half* y, int64_t n, lr_stream_t s);
int lr_gelu_bwd_bf16(const lr_half* pre, const lr_half* dy, lr_half* dpre, int64_t n, lr_stream_t s);
int lr_xattn_block_bf16(const lr_xattn_args* args, lr_stream_t s);
int lr_ffn_block_bf16(const lr_ffn_args* args, lr_stream_t s);
int lr_stin_block_bf16(const lr_stin_args* args, lr_stream_t s);
int lr_rowlin_bf16(const lr_rowlin_args* args, lr_stream_t s);
int lr_xattn_pack_vt_bf16(const lr_half* v, int ldv, lr_half* vt, int B, int heads, int Lc, lr_stream_t s);

/* ==== developer builds only (-DLR_DEV_VARIANTS, tools/build_variant.sh) ==================================================================
 * The product library (python -m leftrefill_amd.build) exports none of the following and reads no environment variable or other
 * process-global switch: every behaviour is selected by the arguments of a call.  A developer build additionally compiles the kernel
 * variants that were measured and not adopted (the 8-wave ping-pong attention kernel, the in-launch split-K reduce of
 * lr_gemm_args.splitk_mode = 1, alternative tile orders, the GroupNorm fold below; profiles/README.md has the measurements) and a small
 * name -> integer table that selects them; leftrefill_amd/_lib.py forwards LR_* environment variables to lr_dev_set. */
#ifdef LR_DEV_VARIANTS
int lr_dev_set(const char* name, int value);
int lr_dev_unset(const char* name);
/* ---- GroupNorm folded into the pointwise GEMM that consumes it (ABI 20) -------------------------------------------------
 * replaces: `x = self.norm(x)` of SpatialTransformer.forward (attention.py:399-404: Normalize = GroupNorm(32, eps 1e-6, affine), no
 *           activation) in front of proj_in (attention.py:405-408): per sample b the normalisation is a per-channel scale / shift
 *           a[b][c] = gamma[c] rstd[b][g(c)], t[b][c] = beta[c] - mean[b][g(c)] a[b][c], so
 *              proj_in(norm(x))[m][n] = sum_c (W[n][c] a[b][c]) x[m][c] + (bias[n] + sum_c W[n][c] t[b][c])
 *           -- the GEMM runs on the RAW x with per-sample weights (lr_gemm_args.wt_bstride) and the normalised tensor is never written.
 *   gpart [B][chunks][32][2]: per-group (sum, sumsq) partials of x from its producer (lr_gemm_args.gn_group_out), HW rows per sample;
 *   w [N][C] fp16, bias [N] fp32 or NULL  ->  w_out [B][N][C] = fp16(W a_b),  bias_out [B][N] = bias + W beta - rounded(W a_b) mean_b
 *   (the mean term uses the ROUNDED weights, so it cancels exactly what the matrix cores accumulate for a constant input).
 *   C % 32 == 0, C % 8 == 0, C <= 2048. */
int lr_gn_fold_weights_f16(const float* gpart, int chunks, int B, int HW, int C, const float* gamma, const float* beta, float eps,
                           const lr_half* w, const float* bias, int N, lr_half* w_out, float* bias_out, lr_stream_t s);
int lr_gn_fold_weights_bf16(const float* gpart, int chunks, int B, int HW, int C, const float* gamma, const float* beta, float eps,
                            const lr_half* w, const float* bias, int N, lr_half* w_out, float* bias_out, lr_stream_t s);
#endif /* LR_DEV_VARIANTS */

#ifdef __cplusplus
}
#endif
#endif /* LEFTREFILL_HIP_H */
