/*
 * afm_hip.h - C-ABI of libafm_hip.so: hand-written gfx950 (MI355X / CDNA4) kernels for the
 * afford-motion diffusion denoising hot path.
 *
 * The reference (pure Python on PyTorch) has no FFI of its own; its only native dependency on
 * this path is the external CUDA extension `pointops_cuda` (reference
 * models/scene_models/pointops.py:7) and ATen's fused transformer kernels.  Every entry point
 * below names the reference interface it replaces (file:line under /root/reference).
 *
 * Conventions ("C-ABI face"):
 *   - extern "C", plain pointers and sizes; all pointers are DEVICE pointers unless named h_*.
 *   - every function returns 0 on success, a positive hipError_t, or a negative AFM_E_* code.
 *   - no allocation, no host synchronisation, no global state: work is enqueued on `stream`
 *     (a hipStream_t passed as void*); the caller owns all memory and keeps it alive until the
 *     stream is synchronised.  Thread-safe by construction.  In particular the library reads NO
 *     environment variables and has no setters: every arithmetic or tuning choice is a field of
 *     the argument structs (ABI v3; the one exception is the opt-in measurement profiler at the end).
 *   - all matrices are row-major float32; indices int32; masks uint8 (1 = padded/ignored).
 */
#ifndef AFM_HIP_H
#define AFM_HIP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define AFM_ABI_VERSION 7

#define AFM_E_BADARG   (-1)   /* shape / pointer validation failed              */
#define AFM_E_WORKSPACE (-2)  /* workspace too small                            */
#define AFM_E_UNSUPPORTED (-3)

/* activation codes for afm_linear */
#define AFM_ACT_NONE 0
#define AFM_ACT_GELU 1        /* exact erf GELU (nn.GELU / activation='gelu')   */
#define AFM_ACT_RELU 2
#define AFM_ACT_SILU 3

int afm_version(void);

/* ------------------------------------------------------------------------------------------
 * afm_linear: C = act_post(act(scale * (A @ W^T) + bias) + residual + rowtab[row % period])
 * Replaces F.linear / nn.Linear (+ the elementwise op that follows it) wherever the reference
 * calls one on this path: cmdm.py:146,156,159,195; nn.TransformerEncoderLayer's in_proj /
 * out_proj / linear1 / linear2 (cmdm.py:66-77); modules.py:52-53,317-319,377,651-661;
 * pointtransformer.py:28,49,51,115-120 (with eval-mode BatchNorm folded into scale/bias).
 * f32 MFMA (v_mfma_f32_32x32x2_f32): exact-f32 products, f32 accumulate.
 *
 *   A [M,K] (row stride lda), W [N,K] (row stride ldw, the nn.Linear weight layout),
 *   C [M,N] (row stride ldc).  bias/scale [N] or NULL.  residual [M,N] (stride ldr) or NULL,
 *   indexed by the OUTPUT row.  rowtab [period,N] or NULL.
 *   Row remaps (0 = identity): logical row r reads A row (r / a_grp) * a_stride + a_off + r % a_grp
 *   and writes C row (r / c_grp) * c_stride + c_off + r % c_grp  (token gather / scatter of
 *   cmdm.py:161,169).
 */
typedef struct {
    const float* A; int64_t lda;
    const float* W; int64_t ldw;
    float* C; int64_t ldc;
    int32_t M, N, K;
    const float* bias;
    const float* scale;
    const float* residual; int64_t ldr;
    const float* rowtab; int32_t rowtab_period;
    int32_t act;                    /* AFM_ACT_* applied before the residual               */
    int32_t act_post;               /* AFM_ACT_* applied after residual / rowtab (ReLU(bn3(.) + identity), pointtransformer.py:120-122) */
    int32_t a_grp, a_stride, a_off;
    int32_t c_grp, c_stride, c_off;
    /* optional fused DDPM update on the output (gaussian_diffusion.py:209-231,431-439):
     * x_next[r,n] = c1[r / rows_per_sample] * C[r,n] + c2[..] * x_t[r,n] + sigma[..] * noise[r,n]
     * (all [M,N] with row stride ldx).  C itself (pred_xstart) is still written if C != NULL. */
    const float* ddpm_xt; const float* ddpm_noise; float* ddpm_out; int64_t ldx;
    const float* ddpm_c1; const float* ddpm_c2; const float* ddpm_sigma; int32_t rows_per_sample;
    /* ---- training hooks (all optional, zero = off; ABI v2).  Order inside the epilogue:
     *   v = scale*acc + bias; preact <- v; v = act(v); v = dropout(v) [drop_after == 0]; v *= act'(dact_z) [dact];
     *   v += residual + rowtab; v = act_post(v); v = dropout(v) [drop_after == 1]; C <- v
     * preact [M,N] (stride ldp): the pre-activation saved for the backward pass (linear1 of the encoder layer,
     *   time_embed.0).  dact / dact_z [M,N] (stride ldz): multiply by the derivative of AFM_ACT_* at the saved
     *   pre-activation - the input-gradient GEMM of the NEXT linear produces dz directly (GELU/SiLU backward fused).
     * dropout: keep-mask from a counter hash of (drop_seed, drop_id, output_row * N + col), scaled by 1/(1-p)
     *   (nn.Dropout of the encoder layer / PositionalEncoding, modules.py:43-45; regenerated, never stored). */
    float* preact; int64_t ldp;
    const float* dact_z; int64_t ldz; int32_t dact;
    float drop_p; uint64_t drop_seed; uint32_t drop_id; int32_t drop_after;
    /* ---- arithmetic of the product (ABI v3; replaces the process-wide afm_linear_set_split of v2).  A GEMM is ELIGIBLE for the
     * bf16-split path when K >= 128, K % 16 == 0 and A / W are 16-byte aligned with lda / ldw % 4 == 0; everything else always runs
     * the native f32 MFMA kernels (v_mfma_f32_32x32x2_f32, 157 TF peak on gfx950).
     *   AFM_ARITH_DEFAULT  every eligible GEMM with N >= 32 takes AFM_ARITH_BF16X6 (ABI v7; v3-v6: X9), all others AFM_ARITH_F32 (arith_min_n
     *                      ignored).  Decided by a worst-case measurement, not an rms: over adversarial operand families (catastrophic
     *                      cancellation, 2^+-60 dynamic range inside a row, mantissas that maximise the dropped terms with every product of one
     *                      sign, K = 128 ... 4096) the worst output element of X6 is never above X9's and both sit in the error class of the
     *                      native f32 MFMA kernel and of an unfused f32 multiply-add chain (tests/test_gpu_arith.py, profiles/r06_arith_worstcase.json).
     *                      Domain of both split forms: operands of magnitude >= 2^-110 (or zero) - a split term below 2^-126 is a bf16
     *                      subnormal and is flushed; AFM_ARITH_F32 has no such limit;
     *   AFM_ARITH_F32      native f32 MFMA;
     *   AFM_ARITH_BF16X9   eligible GEMMs with N >= arith_min_n: every f32 operand is split exactly into three bf16 terms inside the
     *                      kernel and all nine cross products run on the bf16 matrix pipe (v_mfma_f32_32x32x16_bf16, 2500 TF peak)
     *                      with f32 accumulation: the same exact products as the f32 MFMA in a different summation order
     *                      (measured error vs float64 <= the native kernel's, tools/kernel_sweep.cpp);
     *   AFM_ARITH_BF16X6   as X9 without the three smallest products a2 w3, a3 w2, a3 w3 (together <= 2^-23 |a||w|, i.e. two f32 roundings of
     *                      that product; what oneMKL calls float_to_bf16x3 and XLA's "highest" precision on bf16 matrix units).
     *   AFM_ARITH_BF16X1   INFORMATIONAL, not f32 arithmetic: only the product of the two leading bf16 terms (what a plain bf16 x bf16 GEMM with f32
     *                      accumulation computes; relative error ~2^-9 per product).  Exists to MEASURE what bf16 would cost in accuracy
     *                      (tests/test_gpu_cmdm.py::test_bf16_one_product_drift...); never selected by the library.
     * The kernel choice is a function of (arith, arith_min_n, N, K, alignment) - never of M - and every tile shape of one
     * arithmetic sums a given output element in the same order, so a batch and its shards compute identical bits. */
    int32_t arith; int32_t arith_min_n;
    /* performance-only knobs for experiments (bit-neutral; 0 = the library's heuristics): AFM_TUNE_* bits */
    int32_t tune;
    /* ---- fused row-dot epilogue (ABI v4; NULL = off): for a linear layer that is followed by a NARROW linear one (the CDM's
     * contact_layer, contact_dim <= 8 outputs) the wide output never has to exist: with R = rowdot_n vectors rowdot_w [R, N] the kernel
     * writes rowdot_out[row, g, r] = sum over the 64-column group g of C[row, col] * rowdot_w[r, col]  ([M, ceil(N / 64), R], rows
     * through the c_* remap) in a fixed summation order that does not depend on the tile shape; the consumer adds the groups left to
     * right.  C may be NULL.  Needs N % 4 == 0 and 16-byte aligned side inputs. */
    const float* rowdot_w; float* rowdot_out; int32_t rowdot_n;
    /* ---- fused LayerNorm of the output rows (ABI v5; ln_out NULL = off): out_proj / linear2 of a post-LN encoder layer are followed by
     * nn.LayerNorm over the whole output row (cmdm.py:66-77), which no column tile owns.  With ln_out set, the workgroup that finishes the
     * LAST column tile of a block of output rows ("last arriver": one agent-scope release per tile, one ticket per tile on ln_counters, one
     * agent-scope acquire by the last) reads those rows of C back and writes ln_out[row] = LayerNorm(C[row]) * ln_gamma + ln_beta with
     * the arithmetic of afm_layernorm (bit-identical to the two-launch form).  ln_out rows follow the c_* remap, row stride ldo.
     * ln_counters: >= ceil(M / 32) device words, ZERO on entry, zero again on exit.  Needs C, N % 4 == 0, N <= 1024, 16-byte rows; ln_out
     * must not alias C, A or residual. */
    const float* ln_gamma; const float* ln_beta; float* ln_out; int64_t ldo; float ln_eps; uint32_t* ln_counters;
    /* ---- LayerNorm folded ACROSS kernel boundaries (ABI v5; all NULL = off).  In a post-LN encoder layer the LayerNorm output is only
     * ever (i) the A operand of the next linear layer and (ii) a residual input, so it need not exist:
     *   stat_out   [C rows][N / 64][2]  the producer writes, per stored output row and 64-column group, (mean, M2 = sum of squared
     *              deviations from that mean).  Needs N % 64 == 0.  A fixed butterfly per group: independent of the tile shape.
     *   a_stat     statistics of the (raw) A rows as written by their producer ([A rows][a_stat_groups][2], a_stat_groups = K / 64).
     *              W must carry the LayerNorm weight (W[n][k] * gamma[k]), bias the term b[n] + sum_k W[n][k] beta[k], and
     *              a_fold_g [N] = sum_k W[n][k] gamma[k]:  out = rstd * (acc - mean * a_fold_g[n]) + bias[n]  ( = W LN(a) + b ).
     *   res_stat   statistics of the (raw) residual rows ([C rows][N / 64][2]): the residual added is LayerNorm(residual) with
     *              res_gamma / res_beta [N].
     * ln_eps2 = the LayerNorm epsilon.  Plain forward inputs only (no preact / dact / dropout / rowtab / act_post / scale); bf16-split
     * kernels only (AFM_E_UNSUPPORTED when the arithmetic selects the native kernels). */
    float* stat_out; const float* a_stat; int32_t a_stat_groups; const float* a_fold_g;
    const float* res_stat; const float* res_gamma; const float* res_beta; float ln_eps2;
    /* ---- a hole inside every group of the row remaps (ABI v6; 0 = none): with a_skip > 0 the members j >= a_skip_after of a group sit
     * a_skip rows further on: A row = (r / a_grp) * a_stride + a_off + j + (j >= a_skip_after ? a_skip : 0), j = r % a_grp (c_* alike).
     * One launch then covers the time token AND the L motion tokens of every sample while skipping the n_cond step-invariant condition
     * tokens between them (layer 0's in_proj of the sampling loop: a_grp = 1 + L, a_stride = T, a_skip_after = 1, a_skip = n_cond). */
    int32_t a_skip_after, a_skip, c_skip_after, c_skip;
    /* ---- clip_denoised (ABI v6; with ddpm_out only): the epilogue's value (pred_xstart) is clamped to [-1, 1] before it is stored to C
     * and enters the DDPM update - `process_xstart` of gaussian_diffusion.py:289-294 with clip_denoised=True, the reference's default. */
    int32_t ddpm_clip;
    /* ---- riders of the sampling loop's first and last launch of a step (ABI v6; NULL = off; bf16-split kernels only): what used to be a
     * launch of its own per step (prologue_kernel: ~8 us of a 430 us step at one sample per GPU).
     *   ddpm_out2 / ldx2   a second copy of the DDPM update's x_next with row stride ldx2 >= N (the K-padded copy of x_t the NEXT step's
     *                      motion adapter reads; its padding columns are zeroed once per loop)
     *   aux_*              aux_rows rows of aux_cols floats: aux_dst[r * aux_dst_ld + c] = aux_src[clamp(aux_idx[r], 0, aux_idx_max - 1) * aux_cols + c]
     *                      + aux_add[c]  - the time token of every sample (TimestepEmbedder table row of t[r] + positional row 0), written by the
     *                      first aux_rows workgroups of the launch behind their own tile. */
    float* ddpm_out2; int64_t ldx2;
    const float* aux_src; const int64_t* aux_idx; const float* aux_add; float* aux_dst; int64_t aux_dst_ld;
    int32_t aux_rows, aux_cols, aux_idx_max;
} afm_linear_args;

#define AFM_ARITH_DEFAULT 0
#define AFM_ARITH_F32     1
#define AFM_ARITH_BF16X1  3
#define AFM_ARITH_BF16X6  6
#define AFM_ARITH_BF16X9  9

#define AFM_TUNE_NO_DMA      0x1     /* register-staged operand loads instead of global_load_lds                         */
#define AFM_TUNE_TILE_SHIFT  4       /* bits 4..7: force the workgroup tile: 1 = 32x32, 2 = 32x64, 3 = 64x64, 4 = 64x128, 5 = 128x128, 7 = 64x64 with the K segments split over wave groups, 8 = weight-stationary 64-column slabs (row-dot launches with K = 256), 9 = 64x64 on three LDS stages, 10 = split-K on three LDS stages (K = 1024: two groups x two segments), 11 = split-K two groups x two segments on two stages, 12 = 64x64 tiles WALKED by 768 resident workgroups (bf16-split arithmetic), 13 = 256x128 tiles on 512 threads (bf16-split arithmetic; round 6, measurement), 14 = 128x128 tiles on 512 threads (bf16-split arithmetic; what the CMDM sampling loop forces on its wide GEMMs) with the streamed epilogue: every global load of a tile's epilogue issued before its first store, 15 = code 14's tile with the shared epilogue (measurement: the baseline and bit reference of 14); all bit-identical */
#define AFM_TUNE_TILE_MASK   0xF0

int afm_linear(const afm_linear_args* args, void* stream);
/* Two independent afm_linear launches as ONE grid of 128 x 128 tiles of the bf16-split tile program (ABI v7): workgroups [0, tiles0) compute
 * args0's output, the rest args1's.  Both must take the bf16-split path with the same arithmetic and K > 256 (AFM_E_UNSUPPORTED otherwise -
 * the caller then issues two afm_linear calls).  Bit-identical to the two calls; the sampling loop pairs one sub-batch's out_proj with the
 * other's linear1 (cmdm.py:66-77: 164 + 328 tiles = one resident round of 512). */
int afm_linear_pair(const afm_linear_args* args0, const afm_linear_args* args1, void* stream);


/* ------------------------------------------------------------------------------------------
 * afm_mha_fwd: multi-head self-attention core, softmax(QK^T / sqrt(dh) + key mask) V.
 * Replaces the attention inside nn.TransformerEncoderLayer's fast path
 * (torch._transformer_encoder_layer_fwd, reached from cmdm.py:167).
 *   qkv [B*T, 3*H*dh] packed as in_proj output (q | k | v), out [B*T, H*dh];
 *   key_mask [B,T] uint8, 1 = padded key (-inf), or NULL.  dh must be 64.
 * Flash-style single pass, S^T = K Q^T and O^T = V^T P^T on f32 MFMA, K/V tiles staged in LDS.
 */
int afm_mha_fwd(const float* qkv, const uint8_t* key_mask, float* out,
                int32_t B, int32_t T, int32_t H, int32_t dh, void* stream);
/* Same with an explicit workgroup shape: group_waves in {1, 2, 4, 6, 8, 12} 32-query waves per workgroup (the grid is
 * (sample, head, query group)), or 100 + {2, 4}: the two key segments of every query block on two waves (workgroups of twice that many
 * waves - what small launches take: the serial chain of a wave halves); 0 = the library's choice from B*H and T.  The softmax of a
 * row is computed over two key segments (blocks [0, ceil(nkb / 2)) and the rest) whose states are merged in a fixed operation order, so
 * a query row's arithmetic does not depend on the grouping: results are bit-identical. */
int afm_mha_fwd_grouped(const float* qkv, const uint8_t* key_mask, float* out,
                        int32_t B, int32_t T, int32_t H, int32_t dh, int32_t group_waves, void* stream);
/* Same, for the query rows q_first .. T - 1 of every sample only (all T keys): rows 0 .. q_first - 1 of `out` are not written.  The CMDM's
 * last encoder layer is read on its L motion tokens only (cmdm.py:169,195), so its attention skips the 2 + n_groups condition-token
 * queries (q_first = 130 of T = 326: 7 query blocks instead of 11).  A query row's arithmetic does not depend on q_first (bit-identical
 * to afm_mha_fwd_grouped on the rows it computes).  ABI v6. */
int afm_mha_fwd_rows(const float* qkv, const uint8_t* key_mask, float* out,
                     int32_t B, int32_t T, int32_t H, int32_t dh, int32_t q_first, int32_t group_waves, void* stream);
/* Same with the arithmetic of the two products S = Q K^T and O = P V as an argument (ABI v7), `arith` as in afm_linear_args: the inference
 * kernel splits Q, K, V and the probabilities P exactly into three bf16 terms; AFM_ARITH_DEFAULT / AFM_ARITH_BF16X6 run the six largest cross
 * products of every operand pair, every other setting all nine (exact f32 products).  q_first = 0: all query rows.  The entry points above
 * (and afm_mha_cross_fwd) run AFM_ARITH_DEFAULT.  A query row's arithmetic depends on `arith` only - never on the grouping, q_first or B. */
int afm_mha_fwd_arith(const float* qkv, const uint8_t* key_mask, float* out,
                      int32_t B, int32_t T, int32_t H, int32_t dh, int32_t q_first, int32_t group_waves, int32_t arith, void* stream);

/* Cross-attention core of nn.TransformerDecoderLayer (CMDM `trans_dec`, cmdm.py:78-113,171-191): Tq queries q [B*Tq, H*dh] over a
 * packed memory kv [B*Tk, 2*H*dh] (k | v), key_mask [B,Tk] or NULL.  Same kernel as afm_mha_fwd (dh = 64). */
int afm_mha_cross_fwd(const float* q, const float* kv, const uint8_t* key_mask, float* out,
                      int32_t B, int32_t Tq, int32_t Tk, int32_t H, int32_t dh, void* stream);

/* afm_layernorm: y = LN(x) * gamma + beta over the last dim (eps 1e-5).  Replaces nn.LayerNorm
 * (norm1 / norm2 of the encoder layer, modules.py:399-400,459,653).  In-place allowed. */
int afm_layernorm(const float* x, const float* gamma, const float* beta, float* y,
                  int64_t rows, int32_t dim, float eps, void* stream);
/* Same, on a strided subset of token rows: logical row r -> (r / grp) * stride + off + r % grp of both x and y
 * (grp == 0: identity).  Used to normalise only the L motion tokens of each sample in the last encoder layer. */
int afm_layernorm_rows(const float* x, const float* gamma, const float* beta, float* y, int64_t rows, int32_t dim,
                       float eps, int32_t grp, int32_t stride, int32_t off, void* stream);

/* ------------------------------------------------------------------------------------------
 * afm_ddpm_step: x_next = (c1[b] * x0 + c2[b] * x_t) + sigma[b] * noise, evaluated WITHOUT fma
 * contraction so it is bit-identical to the reference's float32 expression
 * (gaussian_diffusion.py:222-225 and :439) given the same inputs.  c1/c2/sigma are per-sample
 * [B] device arrays the host gathers from the float32-cast schedule tables
 * (sigma = (t != 0) * exp(0.5 * posterior_log_variance_clipped[t])).
 * If noise == NULL, counter-based Philox4x32-10 + Box-Muller noise keyed by
 * (seed, sample_index0 + b, step, element) is generated in-kernel (sharding-invariant).
 */
int afm_ddpm_step(const float* x0, const float* x_t, const float* noise, float* x_next,
                  const float* c1, const float* c2, const float* sigma,
                  int32_t B, int64_t per_sample, uint64_t seed, int64_t sample_index0,
                  int32_t step, void* stream);

/* ---- DDIM (v7-additive: new struct and entry points, no existing struct changed).
 * afm_ddim_rows: five float32 rows of the DDIM update, each indexed like the afm_ddpm_step coefficients (afm_ddim_step: per sample [B];
 * the loops below: per timestep index [T], like d_c1).  The host builds them in float32 in the reference's order of operations
 * (ddim_sample, gaussian_diffusion.py:538-586) from the float32-cast tables:
 *   a = sqrt_recip_alphas_cumprod, b = sqrt_recipm1_alphas_cumprod, c = sqrt(alphas_cumprod_prev),
 *   d = sqrt(1 - alphas_cumprod_prev - sigma^2), sigma = (t != 0) * eta * sqrt((1 - abar_prev) / (1 - abar)) * sqrt(1 - abar / abar_prev)
 * ddim_reverse_sample uses c = sqrt(alphas_cumprod_next), d = sqrt(1 - alphas_cumprod_next) and sigma = NULL (no noise term). */
typedef struct {
    const float* a; const float* b; const float* c; const float* d; const float* sigma;
} afm_ddim_rows;

/* afm_ddim_step: eps = (a[b] * x_t - x0) / b[b];  x_next = (x0 * c[b] + d[b] * eps) + sigma[b] * noise, every operation rounded on its own
 * (no fma contraction, IEEE division): bit-identical to the reference's float32 expression given the same inputs.  rows: host struct of
 * per-sample [B] device arrays.  rows->sigma == NULL: no noise term (x_next = the mean; `noise` is not read).  noise == NULL: Philox noise
 * keyed like afm_ddpm_step.  x_next may alias x_t. */
int afm_ddim_step(const float* x0, const float* x_t, const float* noise, float* x_next, const afm_ddim_rows* rows,
                  int32_t B, int64_t per_sample, uint64_t seed, int64_t sample_index0, int32_t step, void* stream);

/* ---- DPM-Solver++(2M) (v7-additive; Lu et al. 2022, the second-order multistep solver for x_start-predicting models; the reference has
 * no such sampler).  afm_dpm_rows: three float32 rows indexed like the afm_ddim_rows.  With alpha_i = sqrt(abar_i), sigma_i =
 * sqrt(1 - abar_i), lambda_i = ln(alpha_i / sigma_i) of the (respaced) process, the step from timestep index i to i - 1 has
 *   h_i = lambda_{i-1} - lambda_i,  a_i = sigma_{i-1} / sigma_i,  k_i = -alpha_{i-1} * expm1(-h_i),  r_i = h_{i+1} / h_i
 *   (b_i, c_i) = (k_i, 0) at the first executed step i = n - 1 and for order 1; (k_i * (1 + 1 / (2 r_i)), -k_i / (2 r_i)) otherwise;
 *   (a_0, b_0, c_0) = (0, 1, 0): the last step returns pred_xstart.
 * The host computes them in float64 and stores float32. */
typedef struct {
    const float* a; const float* b; const float* c;
} afm_dpm_rows;

/* afm_dpm_step: x_next = a[b] * x_t + b[b] * x0 (x0_prev == NULL: no history; x0_prev is never read) or
 * x_next = (a[b] * x_t + b[b] * x0) + c[b] * x0_prev, float32, this association, every operation rounded on its own.  rows: host struct of
 * per-sample [B] device arrays.  No noise term: the sampler is deterministic.  x_next may alias x_t. */
int afm_dpm_step(const float* x0, const float* x_t, const float* x0_prev, float* x_next, const afm_dpm_rows* rows,
                 int32_t B, int64_t per_sample, void* stream);

/* afm_clamp: x <- min(max(x, lo), hi) in place (NaN propagates, as torch.clamp): `process_xstart` with clip_denoised=True on the
 * step-by-step path (gaussian_diffusion.py:289-294).  ABI v6. */
int afm_clamp(float* x, int64_t n, float lo, float hi, void* stream);

/* afm_randn: standalone Philox normal generator with the same keying as afm_ddpm_step
 * (replaces th.randn / th.randn_like, gaussian_diffusion.py:431,514). */
int afm_randn(float* out, int32_t B, int64_t per_sample, uint64_t seed, int64_t sample_index0,
              int32_t step, void* stream);

/* afm_bn_fold (ABI v5): eval-mode nn.BatchNorm1d as y = x * scale + shift (pointtransformer.py:31-36,56-57,111-113 call it after a
 * Linear): scale = w / sqrt(running_var + eps), shift = b - running_mean * scale (+ lin_bias * scale when the Linear has a bias),
 * every operation individually rounded.  All vectors [C]. */
int afm_bn_fold(const float* w, const float* b, const float* running_mean, const float* running_var, float eps, const float* lin_bias,
                float* scale, float* shift, int32_t C, void* stream);

/* afm_contact_glue (ABI v5): the ADM -> AMDM hand-off of the two-stage pipeline kept in HBM.  The reference writes
 * dist = sqrt(-2 ln(clip(sample * std + mean, 1e-20, 1)) sigma^2) to H3D/pred_contact/<id>.npy (utils/evaluate.py:41-82) and reads it back as
 * exp(-dist^2 / (2 sigma^2)) (datasets/humanml3d.py:763-774); out[i] is that condition value, n elements.  sigma_sq = sigma^2 rounded to
 * float32 once by the caller (the reference's Python scalar `sigma ** 2`). */
int afm_contact_glue(const float* sample, float* out, int64_t n, float sigma_sq, float mean, float std, void* stream);

/* afm_masked_mse: out[b] = sum((target - pred)^2 * keep) / (sum(keep) * D) over [L, D], keep = !frame_mask.
 * Replaces the loss reduction of training_losses (gaussian_diffusion.py:815-818, sum_flat nn.py:93-97).  B == 0 is an empty batch: this
 * entry point and afm_masked_mse_bwd return 0 and touch nothing, whatever the pointers.  A sample without a kept frame gives NaN (0 / 0,
 * as the torch expression) and an all-zero dpred. */
int afm_masked_mse(const float* target, const float* pred, const uint8_t* frame_mask, float* out,
                   int32_t B, int32_t L, int32_t D, void* stream);

/* ------------------------------------------------------------------------------------------
 * Training (backward) entry points - the kernels behind `loss.backward()` of training_losses
 * (gaussian_diffusion.py:757-823 called from utils/training.py:140-152).  Gradients are
 * deterministic (fixed-order split reductions, no atomics on floats).  The two scatter-adds of the point branch whose reference CUDA
 * kernels use f32 atomics - the backward of a row gather / of the neighbour grouping and of the 3-NN interpolation - run as segmented sums
 * over an inverse index built once per index list (afm_scatter_plan + afm_segment_sum_rows, ABI v7); the atomic forms
 * (afm_scatter_add_rows, afm_interpolate_bwd) remain for callers without a plan and are the only order-dependent entry points.
 */

/* out[c][r] = in[r][c] (rows x cols -> cols x rows).  The input-gradient GEMM dX = dY @ W is run as
 * afm_linear(A = dY, W = W^T), so the [N,K] nn.Linear weights are transposed once per optimiser step. */
int afm_transpose(const float* in, float* out, int32_t rows, int32_t cols, void* stream);

/* Weight / bias gradient of y = x @ W^T + b:  dW[N,K] = dY^T @ X,  db[N] = colsum(dY)  (db may be NULL).
 * dY [M,N] (row stride lddy), X [M,K] (row stride ldx); logical row r of dY / X lives at row
 * (r / grp) * stride + off + r % grp when the corresponding grp != 0 (token subsets, as in afm_linear).
 * f32 MFMA with both operands reduction-major; the M reduction is split over workgroups into `ws`
 * (afm_linear_wgrad_workspace_bytes) and summed in a fixed order.  accumulate != 0: dW += / db +=. */
typedef struct {
    const float* dY; int64_t lddy;
    const float* X; int64_t ldx;
    float* dW; int64_t lddw;
    float* db;
    int32_t M, N, K;
    int32_t dy_grp, dy_stride, dy_off;
    int32_t x_grp, x_stride, x_off;
    int32_t accumulate;
    void* ws; int64_t ws_bytes;
} afm_linear_wgrad_args;
int64_t afm_linear_wgrad_workspace_bytes(int32_t M, int32_t N, int32_t K);
int afm_linear_wgrad(const afm_linear_wgrad_args* args, void* stream);

/* nn.LayerNorm backward.  x = the LayerNorm INPUT (statistics are recomputed), dy = grad of the output.
 *   dx = rstd * (g - mean(g) - xhat * mean(g * xhat)),  g = dy * gamma
 *   dgamma = sum_rows dy * xhat, dbeta = sum_rows dy  (two-stage fixed-order reduction through ws)
 * dx_drop (optional): dx with the dropout keep-mask of (drop_p, drop_seed, drop_id) applied - the gradient of the
 * residual BRANCH when the forward was  LN(x + dropout(branch))  (encoder layer dropout1 / dropout2). */
int64_t afm_layernorm_bwd_workspace_bytes(int64_t rows, int32_t dim);
int afm_layernorm_bwd(const float* x, const float* gamma, const float* dy, float* dx, float* dx_drop,
                      float* dgamma, float* dbeta, int64_t rows, int32_t dim, float eps,
                      float drop_p, uint64_t drop_seed, uint32_t drop_id, void* ws, int64_t ws_bytes, void* stream);

/* Training-mode attention: as afm_mha_fwd plus lse [B,H,T] (log-sum-exp of the scaled, masked logits, saved for the
 * backward) and attention-probability dropout (F.multi_head_attention_forward dropout_p; 0 = off). */
int afm_mha_fwd_train(const float* qkv, const uint8_t* key_mask, float* out, float* lse,
                      int32_t B, int32_t T, int32_t H, int32_t dh,
                      float drop_p, uint64_t drop_seed, uint32_t drop_id, void* stream);
/* Attention backward: dqkv [B*T, 3*H*dh] packed like qkv, from qkv / out / lse of the forward and dout [B*T, H*dh].
 * Two flash-style passes on f32 MFMA (probabilities recomputed from lse, nothing [T,T]-sized is stored):
 * dQ with one wave per 32-query block, then dK/dV with one wave per 32-key block.  ws: B*H*T floats. */
int afm_mha_bwd(const float* qkv, const uint8_t* key_mask, const float* out, const float* dout, const float* lse,
                float* dqkv, int32_t B, int32_t T, int32_t H, int32_t dh,
                float drop_p, uint64_t drop_seed, uint32_t drop_id, void* ws, int64_t ws_bytes, void* stream);
/* The same pair for cross-attention (nn.TransformerDecoderLayer.multihead_attn of the CMDM's `trans_dec` variant under autograd, cmdm.py:78-113,
 * 171-191): q [B,Tq,H*dh], kv [B,Tk,2*H*dh] = packed K | V projections of the memory, key_mask [B,Tk] or NULL; the forward also writes
 * lse [B*H, Tq]; the backward fills dq [B,Tq,H*dh] and dkv [B,Tk,2*H*dh].  ws: B*H*Tq floats.  Dropout as afm_mha_fwd_train. */
int afm_mha_cross_fwd_train(const float* q, const float* kv, const uint8_t* key_mask, float* out, float* lse, int32_t B, int32_t Tq, int32_t Tk,
                            int32_t H, int32_t dh, float drop_p, uint64_t drop_seed, uint32_t drop_id, void* stream);
int afm_mha_cross_bwd(const float* q, const float* kv, const uint8_t* key_mask, const float* out, const float* dout, const float* lse, float* dq,
                      float* dkv, int32_t B, int32_t Tq, int32_t Tk, int32_t H, int32_t dh, float drop_p, uint64_t drop_seed, uint32_t drop_id,
                      void* ws, int64_t ws_bytes, void* stream);

/* d(afm_masked_mse)/d(pred): dpred[b,l,:] = dloss[b] * 2 * (pred - target) * keep[b,l] / (sum(keep[b]) * D). */
int afm_masked_mse_bwd(const float* target, const float* pred, const uint8_t* frame_mask, const float* dloss,
                       float* dpred, int32_t B, int32_t L, int32_t D, void* stream);

/* out[r,c] = (x[r,c] + rowtab[r % period, c]) * act'(z[r,c]) * keep(r,c)/(1-p)  (rowtab, z optional; in-place allowed).
 * The elementwise glue of the training graph: PositionalEncoding add + dropout (modules.py:43-45) and the
 * activation / dropout backward in front of a stand-alone linear's gradient GEMMs. */
int afm_rowop(const float* x, const float* rowtab, int32_t period, const float* z, int32_t act, float* out,
              int64_t rows, int32_t cols, float drop_p, uint64_t drop_seed, uint32_t drop_id, void* stream);

/* ---- train-mode point-cloud operators (BatchNorm on batch statistics; models/scene_models/pointtransformer.py:26-69,
 * 102-123 under model.train()).  Batch statistics force a full pass between every BatchNorm and its consumer, so the
 * training graph is composed from bandwidth-bound passes over materialised [n, k, c] tensors. */

/* Column statistics of a row-major [rows, C] matrix (C <= 512, rows >= 1), fixed summation order, taken about a pivot K
 * = the mean of the matrix's first min(rows, 64) rows (shifted-data variance: no E[x^2] - mean^2 cancellation; near the
 * column mean whatever a single row holds):
 *   stats[0..C) = sum_r (x[r,c] - K[c]),  stats[C..2C) = sum_r (x[r,c] - K[c])^2,  stats[2C..3C) = K. */
int64_t afm_colstats_workspace_bytes(int64_t rows, int32_t C);
int afm_colstats(const float* x, int64_t rows, int32_t C, float* stats, void* ws, int64_t ws_bytes, void* stream);
/* nn.BatchNorm1d / nn.SyncBatchNorm training-mode bookkeeping from the statistics of `world` ranks ([world][3C], as
 * produced by afm_colstats on every rank and all-gathered; world = 1 without synchronisation), rows_per_rank rows each:
 * per-rank means / M2 are merged with the parallel-variance formula; outputs mean, rstd = 1/sqrt(biased var + eps),
 * scale = gamma*rstd, shift = beta - mean*scale, and the running-statistics update
 * running = (1-momentum)*running + momentum*batch (unbiased variance); running_* may be NULL. */
int afm_bn_finalize(const float* stats, int32_t world, int64_t rows_per_rank, const float* gamma, const float* beta, float eps,
                    float momentum, float* running_mean, float* running_var, float* mean, float* rstd, float* scale,
                    float* shift, int32_t C, void* stream);
/* y = relu?(x * scale[c] + shift[c] + residual)   (BatchNorm apply [+ identity] [+ ReLU]; residual may be NULL) */
int afm_colaffine(const float* x, const float* scale, const float* shift, const float* residual, int32_t relu, float* y,
                  int64_t rows, int32_t C, void* stream);
/* BatchNorm backward, stage 1: stats[0..C) = sum g, stats[C..2C) = sum g*xhat with g = dy * (y > 0 if y given) - these
 * are dbeta and dgamma.  Stage 2: dx = gamma*rstd*(g - sum_g/count - xhat*sum_gx/count), dres = g (optional). */
int afm_bn_bwd_stats(const float* dy, const float* x, const float* y, const float* mean, const float* rstd, int64_t rows,
                     int32_t C, float* stats, void* ws, int64_t ws_bytes, void* stream);
int afm_bn_bwd_apply(const float* dy, const float* x, const float* y, const float* mean, const float* rstd,
                     const float* gamma, const float* stats, int64_t count, float* dx, float* dres, int64_t rows,
                     int32_t C, void* stream);
/* out[r, 0:3] = xyz[idx[r]] - new_xyz[r / k], out[r, 3:3+C] = feat[idx[r]]  (pointops.queryandgroup, pointops.py:79-100;
 * C = 0: relative coordinates only). */
int afm_group_points(const float* xyz, const float* new_xyz, const float* feat, const int32_t* idx, float* out,
                     int64_t rows, int32_t k, int32_t C, void* stream);
/* dst[idx[r], c] += src[r*ld + col_offset + c], c < C  (backward of a row gather; f32 atomics like the CUDA original) */
int afm_scatter_add_rows(const float* src, int64_t ld, int32_t col_offset, const int32_t* idx, float* dst, int64_t rows,
                         int32_t C, void* stream);
/* Deterministic form (ABI v7).  afm_scatter_plan: the inverse of an index list idx [entries] with values in [0, n_dst) - entries outside
 * that range are SKIPPED by the plan (and so by every segmented sum through it; off[n_dst] counts the valid ones) - plan = int32 words
 * [n_dst + 1 segment offsets | entries: the entries of every destination, ASCENDING | scratch], afm_scatter_plan_words(entries, n_dst) words in
 * all; integer atomics only, the result does not depend on any arrival order.  afm_segment_sum_rows: dst[d, c] = sum over the entries e of
 * destination d, in ascending order, of weight(e) * src[(e / row_div) * ld + col_offset + c]  (every destination row is WRITTEN: no zero-fill;
 * row_div = 1: the backward of a row gather, entry = source row; row_div = k with dist2 [rows, k]: the backward of afm_interpolate, weight(e) =
 * w_e / sum_j w_(row, j), w = 1 / (sqrt(dist2) + 1e-8)).  One plan serves every operator that scatters through the same index list. */
int64_t afm_scatter_plan_words(int64_t entries, int64_t n_dst);
int afm_scatter_plan(const int32_t* idx, int64_t entries, int64_t n_dst, int32_t* plan, void* stream);
int afm_segment_sum_rows(const float* src, int64_t ld, int32_t col_offset, int32_t row_div, const float* dist2, const int32_t* plan, float* dst,
                         int64_t n_dst, int32_t C, void* stream);
/* nn.MaxPool1d(k) over [m, k, C] with argmax, and its backward (pointtransformer.py:66-68) */
int afm_group_max(const float* x, float* y, int32_t* arg, int64_t m, int32_t k, int32_t C, void* stream);
int afm_group_max_bwd(const float* dy, const int32_t* arg, float* dx, int64_t m, int32_t k, int32_t C, void* stream);
/* out[g,c] = scale * sum_j x[g,j,c] */
int afm_group_sum(const float* x, float* out, int64_t m, int32_t k, int32_t C, float scale, void* stream);
/* vector-attention glue of PointTransformerLayer (pointtransformer.py:34-37):
 * w0 = k_g - q[:,None] + p_r;  sw = softmax_k(w2);  out[g, s*Cs+j] = sum_k (v_g + p_r)[g,k,s*Cs+j] * sw[g,k,j] */
int afm_pt_w0(const float* kg, const float* q, const float* pr, float* out, int64_t m, int32_t k, int32_t C, void* stream);
int afm_pt_aggregate(const float* vg, const float* pr, const float* w2, float* out, float* sw, int64_t m, int32_t k,
                     int32_t C, int32_t share_planes, void* stream);
int afm_pt_aggregate_bwd(const float* vg, const float* pr, const float* sw, const float* dout, float* da, float* dw2,
                         int64_t m, int32_t k, int32_t C, int32_t share_planes, void* stream);

/* ---- training-path attention of the CDM ContactPerceiver (models/cdm.py:155-188 under model.train()).
 * Few-query cross-attention (encoder, 2 latent queries over N point keys): Q [B,2,C], K/V [B,N,C], H heads;
 * P [B, H*2, N] (row h*2+q) receives the softmax probabilities (saved for the backward), O [B,2,C];
 * attention-probability dropout by the (seed, id, row of P, n) counter hash.  C in {256, 512}. */
int64_t afm_xq_workspace_bytes(int32_t B, int32_t N, int32_t C);
int afm_xq_attention_fwd(const float* Q, const float* K, const float* V, float* P, float* O, int32_t B, int32_t N, int32_t H,
                         int32_t C, float drop_p, uint64_t drop_seed, uint32_t drop_id, void* ws, int64_t ws_bytes, void* stream);
int afm_xq_attention_bwd(const float* Q, const float* K, const float* V, const float* P, const float* dO, float* dS,
                         float* dQ, float* dK, float* dV, int32_t B, int32_t N, int32_t H, int32_t C, float drop_p,
                         uint64_t drop_seed, uint32_t drop_id, void* ws, int64_t ws_bytes, void* stream);
/* Few-key cross-attention (decoder, N point queries over 2 latent keys): Q/O [B,N,C], K/V [B,2,C]; probabilities are
 * recomputed in the backward; dK/dV are fixed-order sums of per-workgroup partials (ws). */
int64_t afm_xk_workspace_bytes(int32_t B, int32_t N, int32_t C);
int afm_xk_attention_fwd(const float* Q, const float* K, const float* V, float* O, int32_t B, int32_t N, int32_t H, int32_t C,
                         float drop_p, uint64_t drop_seed, uint32_t drop_id, void* stream);
int afm_xk_attention_bwd(const float* Q, const float* K, const float* V, const float* dO, float* dQ, float* dK, float* dV,
                         int32_t B, int32_t N, int32_t H, int32_t C, float drop_p, uint64_t drop_seed, uint32_t drop_id,
                         void* ws, int64_t ws_bytes, void* stream);

/* Fused AdamW over one flat parameter (torch.optim.AdamW semantics, utils/training.py:48-53):
 *   p *= 1 - lr*wd; m = b1*m + (1-b1)*g; v = b2*v + (1-b2)*g*g; p -= lr/(1-b1^t) * m / (sqrt(v)/sqrt(1-b2^t) + eps) */
int afm_adamw(float* p, const float* g, float* m, float* v, int64_t n, float lr, float beta1, float beta2,
              float eps, float weight_decay, int32_t step, void* stream);
/* The same update for every parameter tensor of the model in ONE launch: d_table is a DEVICE array of n_tensors
 * descriptors (all tensors at the same step count), max_n the largest element count. */
typedef struct { float* p; const float* g; float* m; float* v; int64_t n; } afm_adamw_tensor;
int afm_adamw_multi(const afm_adamw_tensor* d_table, int32_t n_tensors, int64_t max_n, float lr, float beta1, float beta2,
                    float eps, float weight_decay, int32_t step, void* stream);

/* ------------------------------------------------------------------------------------------
 * Point-cloud operators.  Every sample holds the same number of points, so the reference's
 * offset arrays are implicit: sample b owns rows [b*n, (b+1)*n).  Returned indices are GLOBAL rows.
 *
 * afm_fps replaces pointops_cuda.furthestsampling_cuda (pointops.py:10-27; called from
 * TransitionDown.forward, pointtransformer.py:61): start at the sample's first point, running
 * min squared distance initialised to 1e10, arg-max each round (ties -> lowest index).
 * n <= 16384 points per sample; beyond that afm_fps returns AFM_E_UNSUPPORTED (before any launch).
 * afm_knn replaces pointops_cuda.knnquery_cuda (pointops.py:30-45): brute force, neighbours in
 * ascending (dist2, index) order; dist2 is the SQUARED distance (the wrapper's sqrt is the caller's).
 * Both evaluate d2 = (dx*dx + dy*dy) + dz*dz in float32 without fma contraction (bit-exact indices
 * against oracle/pointops_ref.py).  k in {3, 8, 16}.
 *
 * The kNN / FPS contract on coordinates that are not finite (afm_knn and afm_knn_ws alike, bit for bit against the oracle):
 *  1. Every entry of idx_out and dist2_out is written, and every index lies in its own sample [b*n, (b+1)*n), whatever the
 *     coordinates are - NaN, +-inf, or finite values whose squared difference overflows.  afm_fps likewise writes every index
 *     in range (which points it samples from such a cloud is not specified further).
 *  2. A candidate whose d2 to the query is not finite (NaN or +inf) is not a neighbour.
 *  3. With j < k candidates at a finite distance (fewer than k points in the sample among them), entries j .. k-1 repeat entry j-1.
 *  4. With j = 0 every entry is b*n with dist2 = +inf.
 * The consumers (afm_transition_down, afm_pt_attention, afm_interpolate, afm_gather_rows) do not check the indices they are given.
 */
int afm_fps(const float* xyz, int32_t B, int32_t n, int32_t m, int32_t* idx_out, void* stream);
int afm_knn(int32_t k, const float* xyz, const float* new_xyz, int32_t B, int32_t n, int32_t m,
            int32_t* idx_out, float* dist2_out, void* stream);
/* Same result through an EXACT spatial pruning (ABI v7): the candidates of a sample are sorted along a Morton curve and cut into tiles of 64 with
 * bounding boxes, the queries are sorted the same way, and a wave scans a tile only if some lane's distance to the tile's box (same float operations
 * as the point distances) is not above its current k-th distance; the k best are kept as (distance bits, index) keys, so the neighbours and
 * their order are those of afm_knn bit for bit.  workspace: afm_knn_workspace_bytes(k, B, n, m) bytes, 16-byte aligned (0 = the form does not apply and
 * afm_knn_ws runs afm_knn: it is taken for 4096 <= n <= 8192 candidates with m >= n queries and k in {3, 8, 16} - the large self-searches, the only
 * shapes of this path where it measured faster, 0.60 vs 0.83 ms at 32 x 8192 points, k = 8). */
int64_t afm_knn_workspace_bytes(int32_t k, int32_t B, int32_t n, int32_t m);
int afm_knn_ws(int32_t k, const float* xyz, const float* new_xyz, int32_t B, int32_t n, int32_t m, int32_t* idx_out, float* dist2_out,
               void* workspace, int64_t workspace_bytes, void* stream);
/* out[r, :] = src[idx[r], :]  (the `p[idx.long(), :]` of pointtransformer.py:62) */
int afm_gather_rows(const float* src, const int32_t* idx, float* out, int64_t rows, int32_t c, void* stream);

/* afm_interpolate: inverse-distance-weighted feature upsampling of pointops.interpolation (pointops.py:164-178):
 *   out[i,:] = base[i,:] + sum_j w_ij feat[idx[i,j],:],  w_ij = r_ij / sum_j r_ij,  r_ij = 1 / (sqrt(dist2[i,j]) + 1e-8)
 * idx / dist2 [n,k] come from afm_knn (k = 3); base may be NULL.  Fuses the `linear1(x1) +` of TransitionUp
 * (pointtransformer.py:98).  afm_segment_mean: per-sample mean over n rows (TransitionUp head mode, :90), summed in float32 in a FIXED
 * order - row i of a sample joins partial chain i mod 64, a chain adds its rows in ascending order, the chains are combined by the tree
 * s[p] += s[p + h], h = 32 ... 1, the total is divided by n - which depends on the sample's rows alone: the same bits from run to run, for
 * every B and every place of the sample in the batch. */
int afm_interpolate(const float* feat, const int32_t* idx, const float* dist2, const float* base, float* out,
                    int64_t n, int32_t c, int32_t k, void* stream);
int afm_segment_mean(const float* x, float* out, int32_t B, int32_t n, int32_t c, void* stream);
/* backward of afm_interpolate with respect to feat (autograd of pointops.interpolation reached from loss.backward() of the PointTrans
 * denoisers, utils/training.py:152): dfeat [m, c] = 0, then dfeat[idx[i,j], :] += w_ij * dout[i, :] over the n fine points (f32 atomics,
 * as the reference's CUDA backward).  The gradient of `base` is dout itself. */
int afm_interpolate_bwd(const float* dout, const int32_t* idx, const float* dist2, float* dfeat, int64_t n, int64_t m, int32_t c,
                        int32_t k, void* stream);

/* afm_transition_down: fused "set abstraction" of TransitionDown.forward (pointtransformer.py:53-69,
 * stride != 1, eval-mode BN folded to scale/shift):
 *   out[i, o] = max_j ReLU(scale[o] * (W[o,:] . [p[knn[i,j]] - new_p[i] ; x[knn[i,j]]]) + shift[o])
 * p [R,3], x [R,c], new_p [M,3], knn_idx [M,nsample] (nsample must be 16), weight [cout, 3+c].
 * The grouped (M, nsample, 3+c) tensor of pointops.queryandgroup (pointops.py:79-100) is never built. */
int afm_transition_down(const float* p, const float* x, int32_t c, const float* new_p, const int32_t* knn_idx,
                        int32_t nsample, const float* weight, int32_t cout, const float* scale, const float* shift,
                        float* out, int32_t M, void* stream);

/* afm_pt_attention: PointTransformerLayer.forward after the q/k/v projections (pointtransformer.py:26-38):
 *   p_r = lp3(ReLU(BN(lp0(p_j - p_i)))),  w = softmax_j(w5(ReLU(BN(w2(ReLU(BN(k_j - q_i + p_r))))))),
 *   out[i, c] = sum_j (v_j + p_r)[c] * w[j, c mod (C/share_planes)],  then optional out*out_scale+out_shift, ReLU.
 * qkv [n, 3C] = [linear_q(x) | linear_k(x) | linear_v(x)], knn_idx [n, nsample] (self-kNN, nsample 8 or 16).
 * BatchNorms are passed folded (scale, shift).
 * Shapes served: channels <= 512, channels % share_planes == 0 (else AFM_E_BADARG), C/share_planes a divisor of 64, nsample 8 (channels
 * <= 256 only) or 16.  channels <= 256 runs four points per workgroup with w2 held in LDS, above that one point per workgroup with w2
 * read from global memory.  A shape whose workgroup would need more than the 160 KB of LDS a gfx950 workgroup has - channels = 256,
 * share_planes = 4, nsample = 16 asks for 180 480 bytes - is refused with AFM_E_UNSUPPORTED like every other unserved shape, before
 * anything is launched and with `out` untouched. */
typedef struct {
    const float* p; const float* qkv; const int32_t* knn_idx; float* out;
    int32_t n, channels, nsample, share_planes;
    const float* lp0_w; const float* lp0_b;              /* linear_p.0  [3,3],[3]      */
    const float* lp_bn_scale; const float* lp_bn_shift;  /* linear_p.1  BN(3)          */
    const float* lp3_w; const float* lp3_b;              /* linear_p.3  [C,3],[C]      */
    const float* w0_bn_scale; const float* w0_bn_shift;  /* linear_w.0  BN(C)          */
    const float* w2_w; const float* w2_b;                /* linear_w.2  [C/s, C],[C/s] */
    const float* w3_bn_scale; const float* w3_bn_shift;  /* linear_w.3  BN(C/s)        */
    const float* w5_w; const float* w5_b;                /* linear_w.5  [C/s,C/s],[C/s]*/
    const float* out_scale; const float* out_shift;      /* optional fused bn2 of the block, or NULL */
    int32_t relu;
} afm_pt_attention_args;
int afm_pt_attention(const afm_pt_attention_args* args, void* stream);

/* ------------------------------------------------------------------------------------------
 * CMDM (`trans_enc`) denoiser forward, sampling form.  Replaces CMDM.forward (cmdm.py:118-196)
 * with the step-invariant condition tokens supplied pre-computed (they depend only on
 * c_text / c_pc_xyz / c_pc_contact, see afm_cmdm_cond_tokens in the Python host layer).
 */
typedef struct {
    const float* in_proj_w;  const float* in_proj_b;    /* [3d,d], [3d]  self_attn.in_proj_*      */
    const float* out_proj_w; const float* out_proj_b;   /* [d,d],  [d]   self_attn.out_proj.*     */
    const float* lin1_w; const float* lin1_b;           /* [ff,d], [ff]  linear1.*                */
    const float* lin2_w; const float* lin2_b;           /* [d,ff], [d]   linear2.*                */
    const float* norm1_w; const float* norm1_b;         /* [d]           norm1.*                  */
    const float* norm2_w; const float* norm2_b;         /* [d]           norm2.*                  */
    /* ABI v5, all six or none (the host builds them in eval mode, float64 products rounded once): the layer's two LayerNorm-fed linears
     * with the LayerNorm folded in (afm_linear_args.a_stat): W' = W * gamma (per input column), g = row sums of W', c = b + W beta.
     * lin1_* folds norm1 of THIS layer; in_proj_* folds norm2 of the PREVIOUS layer (unused in layer 0, whose input is not normalised). */
    const float* lin1_wg; const float* lin1_g; const float* lin1_c;             /* [ff,d], [ff], [ff]   */
    const float* in_proj_wg; const float* in_proj_g; const float* in_proj_c;    /* [3d,d], [3d], [3d]   */
} afm_encoder_layer_weights;

#define AFM_MAX_LAYERS 16

typedef struct {
    int32_t d, heads, ff, n_layers;        /* latent_dim, num_heads, dim_feedforward, sum(num_layers) */
    int32_t motion_dim;                    /* input_feats (263 'h3d', 66 'pos')                        */
    int32_t n_cond;                        /* number of step-invariant tokens after the time token      */
    const float* motion_adapter_w; const float* motion_adapter_b;   /* [d, motion_dim], [d]  */
    const float* motion_layer_w;   const float* motion_layer_b;     /* [motion_dim, d], [motion_dim] */
    const float* time_table;               /* [n_timesteps, d] TimestepEmbedder output for every t (modules.py:52-53) */
    int32_t n_timesteps;
    const float* pos_table;                /* [>= 1+n_cond+L, d] sinusoid table (modules.py:10-26)    */
    afm_encoder_layer_weights layer[AFM_MAX_LAYERS];
    /* ABI v3: arithmetic of every nn.Linear of the denoiser (afm_linear_args.arith / arith_min_n) and bit-neutral tuning */
    int32_t gemm_arith, gemm_arith_min_n;
    int32_t attn_group_waves;              /* afm_mha_fwd_grouped's group_waves (0 = auto)                              */
    int32_t flags;                         /* AFM_CMDM_* bits                                                           */
    /* ABI v5: 0, or the row length (a multiple of 4, >= motion_dim) motion_adapter_w is zero-padded to: [d, kpad].  The loop then keeps a
     * padded copy of x_t in its workspace so that the adapter (K = 263 for 'h3d') runs with K = 272 on the bf16-split GEMM. */
    int32_t motion_adapter_kpad;
    /* ABI v5: motion_layer with the LAST layer's norm2 folded in (see afm_encoder_layer_weights.lin1_wg); NULL = not folded.  With all
     * folded tensors present the step runs WITHOUT LayerNorm launches and without materialised LayerNorm outputs: out_proj / linear2
     * write per-row statistics next to their raw outputs, the consumers apply them (afm_linear_args.stat_out / a_stat / res_stat). */
    const float* motion_layer_wg; const float* motion_layer_g; const float* motion_layer_c;      /* [motion_dim,d], [motion_dim] x 2 */
} afm_cmdm_weights;

#define AFM_CMDM_NO_L0_CACHE 0x1           /* measurement: recompute layer 0's q|k|v rows of the condition tokens every step */
#define AFM_CMDM_NO_LN_FOLD  0x4           /* measurement: separate afm_layernorm launches although the folded tensors are present */
#define AFM_CMDM_WIDE_TILE_SHIFT 8        /* bits 8..11, measurement: AFM_TUNE_TILE code forced on the encoder GEMMs with N >= 512 and M >= 2048 (bit-neutral) */
#define AFM_CMDM_NO_RIDERS   0x20          /* measurement: the per-step prologue launch of round 3 instead of the riders on the first / last GEMM of a step (bit-identical) */
#define AFM_CMDM_CLIP_X0     0x10          /* clip_denoised=True (gaussian_diffusion.py:289-294): pred_xstart clamped to [-1, 1] inside the fused DDPM update */
#define AFM_CMDM_ALL_QUERIES 0x8           /* measurement: the last layer's attention computes all T query rows (bit-identical on the rows that are read) */
#define AFM_CMDM_PAIR_LAUNCH 0x40          /* ABI v7, native loop with two sub-batch streams: sub-batch A's out_proj and sub-batch B's linear1 of every layer as ONE 128 x 128-tile launch (afm_linear_pair; bit-identical) */
#define AFM_CMDM_FUSED_LN    0x2           /* norm1 / norm2 inside out_proj / linear2 (afm_linear_args.ln_*; bit-identical, measured slower: off by default) */

/* bytes of workspace afm_cmdm_forward needs for (B, L). */
int64_t afm_cmdm_workspace_bytes(const afm_cmdm_weights* w, int32_t B, int32_t L);

/* One denoiser evaluation (+ optional fused DDPM update).
 *   x_t [B,L,motion_dim]; t [B] int64 ORIGINAL timesteps (after respace.py:124-129 mapping);
 *   cond_tokens [B, n_cond, d] = adapters(conditions) + positional encoding of positions 1..n_cond;
 *   frame_mask [B,L] uint8 (1 = padded frame) or NULL (mask_motion False);
 *   x0_out [B,L,motion_dim] (may be NULL when ddpm != NULL).
 *   ddpm: if non-NULL, also writes x_next (see afm_ddpm_args).
 */
typedef struct {
    const float* noise;      /* [B,L,motion_dim] or NULL -> Philox */
    float* x_next;           /* [B,L,motion_dim] */
    const float* c1; const float* c2; const float* sigma;   /* [B] */
    uint64_t seed; int64_t sample_index0; int32_t step;
} afm_ddpm_args;

int afm_cmdm_forward(const afm_cmdm_weights* w, const float* x_t, const int64_t* t,
                     const float* cond_tokens, const uint8_t* frame_mask, float* x0_out,
                     const afm_ddpm_args* ddpm, int32_t B, int32_t L,
                     void* workspace, int64_t workspace_bytes, void* stream);

/* Whole p_sample_loop (gaussian_diffusion.py:442-536) enqueued from native code with no host
 * synchronisation and no host<->device traffic: for i = n_steps-1 .. 0: x <- p_sample(x, t = i).
 *   d_timestep_map [n_steps] int64 (respace.py timestep_map), d_c1/d_c2/d_sigma [n_steps] float32
 *   schedule rows (posterior_mean_coef1/2 and (i != 0) * exp(0.5 * posterior_log_variance_clipped)),
 *   all DEVICE arrays indexed by the spaced step i.
 *   x [B,L,motion_dim] holds x_T on entry and the final sample on exit.
 *   step_noise: [n_steps, B, L, motion_dim] device (row j = j-th executed step, t = n_steps-1-j)
 *   or NULL -> Philox keyed by (seed, sample_index0 + b, step = j).
 *   sched_scratch: device scratch of >= afm_cmdm_sched_scratch_bytes(n_steps, B) bytes.
 *   Sub-batching: samples are independent for the whole loop, so the batch may be split into
 *   n_streams contiguous sub-batches, sub-batch s running its own loop on side_streams[s] (caller-owned
 *   hipStream_t handles; NULL / 0 = everything on `stream`).  One sub-batch's kernels fill the
 *   wave-quantisation tails of the other's; results are bit-identical to the single-stream run.
 *   `stream` is joined with every side stream before the call returns its work to the caller
 *   (event wait, no host sync).  workspace must hold afm_cmdm_loop_workspace_bytes(w, B, L, n_streams).
 */
int64_t afm_cmdm_sched_scratch_bytes(int32_t n_steps, int32_t B);
int64_t afm_cmdm_loop_workspace_bytes(const afm_cmdm_weights* w, int32_t B, int32_t L, int32_t n_streams);

int afm_cmdm_sample_loop(const afm_cmdm_weights* w, float* x, const float* cond_tokens,
                         const uint8_t* frame_mask, const float* step_noise,
                         const int64_t* d_timestep_map, const float* d_c1, const float* d_c2,
                         const float* d_sigma, int32_t n_steps, uint64_t seed, int64_t sample_index0,
                         int32_t B, int32_t L, void* sched_scratch, void* workspace,
                         int64_t workspace_bytes, int32_t n_streams, void* const* side_streams, void* stream);

/* A contiguous slice of the same loop: runs executed steps first_step .. first_step+n_steps-1 of a longer chain (the
 * Philox step counter continues at first_step, so chunks chained over [0, T) reproduce afm_cmdm_sample_loop bit for bit).
 * The schedule rows and step_noise passed in are the SLICE's: d_*[i] for the slice's timesteps in ascending order (the
 * slice walks them from index n_steps-1 down to 0), step_noise row 0 = the slice's first executed step.  This is what
 * `progress=True` in the reference's test.py maps to (gaussian_diffusion.py:520-523: tqdm over the step indices): the host
 * advances the progress bar between slices while each slice stays one native enqueue. */
int afm_cmdm_sample_loop_range(const afm_cmdm_weights* w, float* x, const float* cond_tokens,
                               const uint8_t* frame_mask, const float* step_noise,
                               const int64_t* d_timestep_map, const float* d_c1, const float* d_c2,
                               const float* d_sigma, int32_t n_steps, int32_t first_step, uint64_t seed,
                               int64_t sample_index0, int32_t B, int32_t L, void* sched_scratch, void* workspace,
                               int64_t workspace_bytes, int32_t n_streams, void* const* side_streams, void* stream);

/* DDIM form of the native loop (v7-additive; ddim_sample_loop, gaussian_diffusion.py:626-710): the arguments of
 * afm_cmdm_sample_loop_range with the three DDPM rows replaced by `rows`, a host struct of DDIM rows per timestep index (device arrays,
 * the slice's rows in ascending order, as d_c1).  rows->sigma == NULL: no noise term (eta = 0) and no noise is generated or read.
 * The launches of a step are the DDPM loop's plus ONE elementwise launch per sub-batch: motion_layer stores pred_xstart and that launch
 * applies the DDIM update (clip_denoised included) and writes the next step's K-padded copy of x (the DDPM update stays fused in the GEMM
 * epilogue, whose registers a second update form would grow).  Sub-batch streams and AFM_CMDM_PAIR_LAUNCH are bit-identical to one stream.  sched_scratch >= afm_ddim_sched_scratch_bytes(n_steps, B). */
int64_t afm_ddim_sched_scratch_bytes(int32_t n_steps, int32_t B);
int afm_cmdm_ddim_loop_range(const afm_cmdm_weights* w, float* x, const float* cond_tokens,
                             const uint8_t* frame_mask, const float* step_noise,
                             const int64_t* d_timestep_map, const afm_ddim_rows* rows, int32_t n_steps, int32_t first_step, uint64_t seed,
                             int64_t sample_index0, int32_t B, int32_t L, void* sched_scratch, void* workspace,
                             int64_t workspace_bytes, int32_t n_streams, void* const* side_streams, void* stream);

/* ---- Classifier-free guided sampling of the CMDM (v7-additive: new structs and entry points, no existing struct changed).
 * The reference trains every motion task with condition dropout (datasets/transforms.py:46-92: c_text_mask / c_pc_mask with probability
 * 0.1; models/cmdm.py:142-166 turns them into key-padding masks when mask_motion is true), so a CMDM checkpoint is a guidance model.
 * For sample b with scale s[b]:   x0_guided = x0_u + s[b] * (x0_c - x0_u)     (float32, no contraction, this association)
 * x0_c is the ordinary forward; x0_u the forward of the SAME x_t, t, frame mask with the dropped condition tokens key-masked in every
 * layer (token 1 = text, tokens 2 .. n_cond = the contact groups).  clip_denoised clamps x0_guided, not the branches.
 * The unconditioned branch has two forms.  Compact (every condition dropped): a masked key is read by no query in any layer, so the
 * condition rows need not exist - the branch runs on [time | motion] tokens only (T_u = 1 + L), the motion tokens keeping their
 * positional rows 1 + n_cond ..; it differs from the masked form only in where the attention's key blocks fall.  Masked (partial drop, or
 * AFM_CFG_FORCE_MASKED): all T rows, the key mask also covering the dropped tokens.  Both need frame_mask != NULL for a partial drop or
 * the forced masked form (the key mask is built from it). */
typedef struct {
    const float* scale;                    /* device [B]: guidance scale per sample                                      */
    int32_t drop_text, drop_pc;            /* which conditions the unconditioned branch drops (at least one)             */
    int32_t flags;                         /* AFM_CFG_* bits                                                             */
    void* const* branch_streams;           /* guided loops only: one more stream per sub-batch (max(n_streams, 1) handles) for the
                                            * unconditioned branch, or NULL = both branches on the sub-batch's stream (bit-identical) */
} afm_cfg_args;
#define AFM_CFG_FORCE_MASKED 0x1           /* measurement: the masked full-T form although every condition is dropped   */

/* out = x0_u + scale[b] * (x0_c - x0_u), [B][per_sample]; out may alias either input. */
int afm_cfg_combine(const float* x0_c, const float* x0_u, const float* scale, float* out, int32_t B, int64_t per_sample, void* stream);

/* One guided sampling update from the two branches' pred_xstart: x0 = the combination above, clamped to [-1, 1] if `clip`, then the
 * afm_ddpm_step expression with the per-sample rows c1 / c2 / sigma (ddim == NULL) or the afm_ddim_step expression with the per-sample
 * rows *ddim (ddim->sigma == NULL: no noise term).  noise == NULL: Philox keyed like afm_ddpm_step.  x_next may alias x_t.  Bit-identical
 * to afm_cfg_combine -> afm_clamp -> afm_ddpm_step / afm_ddim_step. */
typedef struct {
    const float* x0_c; const float* x0_u; const float* scale;       /* [B][per_sample] x 2, [B] */
    const float* x_t; const float* noise; float* x_next;            /* [B][per_sample]          */
    const float* c1; const float* c2; const float* sigma;           /* DDPM rows [B]            */
    const afm_ddim_rows* ddim;                                      /* or DDIM rows [B]         */
    int32_t clip; int32_t B; int64_t per_sample;
    uint64_t seed; int64_t sample_index0; int32_t step;
} afm_cfg_step_args;
int afm_cfg_step(const afm_cfg_step_args* args, void* stream);

/* Both branches of one guided evaluation and their combination: x0_c, x0_u, x0_guided [B,L,motion_dim] (x0_c / x0_u may be NULL: the
 * workspace then holds them).  The conditioned branch is afm_cmdm_forward's launches; the workspace of afm_cmdm_workspace_bytes plus
 * 2 * B * L * motion_dim floats (afm_cmdm_cfg_workspace_bytes) serves both branches in turn. */
int64_t afm_cmdm_cfg_workspace_bytes(const afm_cmdm_weights* w, int32_t B, int32_t L);
int afm_cmdm_cfg_forward(const afm_cmdm_weights* w, const float* x_t, const int64_t* t, const float* cond_tokens,
                         const uint8_t* frame_mask, const afm_cfg_args* cfg, float* x0_c, float* x0_u, float* x0_guided,
                         int32_t B, int32_t L, void* workspace, int64_t workspace_bytes, void* stream);

/* Guided native loops, range form: the arguments of afm_cmdm_sample_loop_range / afm_cmdm_ddim_loop_range plus `cfg` (cfg->scale [B]).
 * Per sub-batch and step: the conditioned branch (the unguided step's launches, layer-0 cache and riders included), the unconditioned
 * branch, ONE update launch (the afm_cfg_step expression, in place on x, plus the next step's K-padded copy of x) - all on the
 * sub-batch's stream, or with cfg->branch_streams the unconditioned branch on a stream of its own between two events per step (after the
 * previous update, before this one).  Both motion_layer GEMMs store pred_xstart with the plain epilogue, for DDPM too.  AFM_CMDM_PAIR_LAUNCH is ignored
 * (a guided loop runs unpaired).  workspace >= afm_cmdm_cfg_loop_workspace_bytes; sched_scratch as the unguided loop of the same update. */
int64_t afm_cmdm_cfg_loop_workspace_bytes(const afm_cmdm_weights* w, int32_t B, int32_t L, int32_t n_streams, const afm_cfg_args* cfg);
int afm_cmdm_cfg_sample_loop_range(const afm_cmdm_weights* w, float* x, const float* cond_tokens,
                                   const uint8_t* frame_mask, const float* step_noise,
                                   const int64_t* d_timestep_map, const float* d_c1, const float* d_c2,
                                   const float* d_sigma, const afm_cfg_args* cfg, int32_t n_steps, int32_t first_step, uint64_t seed,
                                   int64_t sample_index0, int32_t B, int32_t L, void* sched_scratch, void* workspace,
                                   int64_t workspace_bytes, int32_t n_streams, void* const* side_streams, void* stream);
int afm_cmdm_cfg_ddim_loop_range(const afm_cmdm_weights* w, float* x, const float* cond_tokens,
                                 const uint8_t* frame_mask, const float* step_noise,
                                 const int64_t* d_timestep_map, const afm_ddim_rows* rows, const afm_cfg_args* cfg, int32_t n_steps,
                                 int32_t first_step, uint64_t seed,
                                 int64_t sample_index0, int32_t B, int32_t L, void* sched_scratch, void* workspace,
                                 int64_t workspace_bytes, int32_t n_streams, void* const* side_streams, void* stream);

/* ------------------------------------------------------------------------------------------
 * Imputation of known motion values (editing: keyframes, a root trajectory, a prefix).  The reference's denoised_fn hook of
 * p_mean_variance (gaussian_diffusion.py:289-294), as a SELECT on pred_xstart, per element and in this order:
 *   v = x0 (guided: the afm_cfg_combine expression)  ->  v = mask ? known : v  ->  clamp to [-1, 1] if clip  ->  the update.
 * mask: uint8, nonzero = known.  Where mask == 0, `known` is never read into the result (a NaN there does not propagate).  Known values
 * outside [-1, 1] are clamped with clip (denoised_fn runs before the clamp).  Nothing is imputed in x_t space.
 * ------------------------------------------------------------------------------------------ */

/* out[i] = mask[i] ? known[i] : x0[i], n values; out may alias x0. */
int afm_impute(const float* x0, const float* known, const uint8_t* mask, float* out, int64_t n, void* stream);

/* One imputing sampling update: afm_cfg_step with known / mask [B][per_sample] (both required), and x0_u / scale optional (both NULL:
 * unguided, x0 = x0_c).  Rows and noise as afm_cfg_step.  x_next may alias x_t.  Bit-identical to (afm_cfg_combine ->) afm_impute ->
 * afm_clamp -> afm_ddpm_step / afm_ddim_step.  per_sample need not be a multiple of 4 (the mask is read bytewise). */
typedef struct {
    const float* x0_c; const float* x0_u; const float* scale;       /* [B][per_sample] x 2, [B]; x0_u, scale: both or neither */
    const float* known; const uint8_t* mask;                        /* [B][per_sample]          */
    const float* x_t; const float* noise; float* x_next;            /* [B][per_sample]          */
    const float* c1; const float* c2; const float* sigma;           /* DDPM rows [B]            */
    const afm_ddim_rows* ddim;                                      /* or DDIM rows [B]         */
    int32_t clip; int32_t B; int64_t per_sample;
    uint64_t seed; int64_t sample_index0; int32_t step;
} afm_impute_step_args;
int afm_impute_step(const afm_impute_step_args* args, void* stream);

/* The imputing native loop, all four forms behind one entry: the arguments of the *_loop_range entries with both kinds of rows
 * (rows != NULL: the DDIM loop, d_c1 / d_c2 / d_sigma ignored; rows == NULL: the DDPM loop), cfg (NULL: unguided) and known / mask
 * [B][L][motion_dim] (both required; AFM_E_BADARG otherwise).  Every step stores pred_xstart with the plain motion_layer epilogue - for
 * DDPM too: the update fused into that epilogue has no place for the select - and runs ONE update launch per sub-batch (the
 * afm_impute_step expression, in place on x, plus the next step's K-padded copy).  Launches per step: the unguided DDPM loop's + 1; the
 * DDIM and guided loops' unchanged.  AFM_CMDM_PAIR_LAUNCH and AFM_CMDM_FUSED_LN are ignored.  Noise, sub-batch streams, branch streams
 * and first_step as the other loops.  workspace >= afm_cmdm_loop_workspace_bytes (cfg == NULL; the loop workspace always holds a
 * pred_xstart region) or afm_cmdm_cfg_loop_workspace_bytes (cfg != NULL); sched_scratch: afm_ddim_sched_scratch_bytes with rows,
 * afm_cmdm_sched_scratch_bytes without. */
int afm_cmdm_impute_loop_range(const afm_cmdm_weights* w, float* x, const float* cond_tokens,
                               const uint8_t* frame_mask, const float* step_noise, const int64_t* d_timestep_map,
                               const afm_ddim_rows* rows, const float* d_c1, const float* d_c2, const float* d_sigma,
                               const afm_cfg_args* cfg, const float* known, const uint8_t* mask, int32_t n_steps, int32_t first_step,
                               uint64_t seed, int64_t sample_index0, int32_t B, int32_t L, void* sched_scratch, void* workspace,
                               int64_t workspace_bytes, int32_t n_streams, void* const* side_streams, void* stream);

/* ---- Two-scale guidance of the CMDM: one scale per condition (v7-additive: new structs and entry points, no existing struct changed).
 * The reference drops text and scene contact independently in training, so a checkpoint is a guidance model for each condition
 * separately.  (first, second) name the two conditions in the caller's order; three evaluations share x_t, t and the frame mask:
 *   u: both dropped (the compact unconditioned form of afm_cfg_args, or the masked one with AFM_CFG_FORCE_MASKED),
 *   a: only `first` kept (the masked partial-drop form: the second condition's tokens key-masked),
 *   c: nothing dropped (the ordinary forward).
 * For sample b, in float32, no contraction, this association:
 *   g1 = u + scale_first[b] * (a - u);      x0_guided = g1 + scale_second[b] * (c - a)
 * No shortcut for equal or zero scales: equal scales are NOT bit-equal to the single-scale form.  frame_mask is required (a is a masked
 * form).  Branch streams are not built for three branches. */
typedef struct {
    const float* scale_first;              /* device [B]: the first condition's scale per sample                          */
    const float* scale_second;             /* device [B]: the second condition's                                          */
    int32_t first;                         /* the first condition: 0 = text, 1 = pc (the second is the other one)         */
    int32_t flags;                         /* AFM_CFG_FORCE_MASKED: applies to u                                          */
} afm_cfg2_args;

/* out = (x0_u + scale_first[b] * (x0_a - x0_u)) + scale_second[b] * (x0_c - x0_a), [B][per_sample]; out may alias any input. */
int afm_cfg2_combine(const float* x0_c, const float* x0_a, const float* x0_u, const float* scale_first, const float* scale_second,
                     float* out, int32_t B, int64_t per_sample, void* stream);

/* One two-scale sampling update from the three branches' pred_xstart: x0 = the combination above, := known where mask is set (known /
 * mask: both or neither), clamped to [-1, 1] if `clip`, then the afm_ddpm_step expression (rows c1 / c2 / sigma, ddim == NULL) or the
 * afm_ddim_step expression (rows *ddim).  Noise as afm_cfg_step.  x_next may alias x_t.  Bit-identical to afm_cfg2_combine ->
 * afm_impute -> afm_clamp -> afm_ddpm_step / afm_ddim_step. */
typedef struct {
    const float* x0_c; const float* x0_a; const float* x0_u;        /* [B][per_sample] x 3      */
    const float* scale_first; const float* scale_second;            /* [B] x 2                  */
    const float* known; const uint8_t* mask;                        /* [B][per_sample] or NULL  */
    const float* x_t; const float* noise; float* x_next;            /* [B][per_sample]          */
    const float* c1; const float* c2; const float* sigma;           /* DDPM rows [B]            */
    const afm_ddim_rows* ddim;                                      /* or DDIM rows [B]         */
    int32_t clip; int32_t B; int64_t per_sample;
    uint64_t seed; int64_t sample_index0; int32_t step;
} afm_cfg2_step_args;
int afm_cfg2_step(const afm_cfg2_step_args* args, void* stream);

/* The three branches of one two-scale evaluation and their combination: x0_c, x0_a, x0_u, x0_guided [B,L,motion_dim] (the branches may
 * be NULL: the workspace then holds them).  One workspace (afm_cmdm_workspace_bytes plus 3 * B * L * motion_dim floats) serves the three
 * branches in turn. */
int64_t afm_cmdm_cfg2_workspace_bytes(const afm_cmdm_weights* w, int32_t B, int32_t L);
int afm_cmdm_cfg2_forward(const afm_cmdm_weights* w, const float* x_t, const int64_t* t, const float* cond_tokens,
                          const uint8_t* frame_mask, const afm_cfg2_args* cfg, float* x0_c, float* x0_a, float* x0_u, float* x0_guided,
                          int32_t B, int32_t L, void* workspace, int64_t workspace_bytes, void* stream);

/* The two-scale native loop, every form behind one entry, like afm_cmdm_impute_loop_range: both kinds of rows (rows != NULL: DDIM,
 * d_c1 / d_c2 / d_sigma ignored), known / mask [B][L][motion_dim] optional (both or neither).  Per sub-batch and step, all on the
 * sub-batch's stream: the conditioned branch, the a branch on a workspace of its own behind it, the u branch behind that, and ONE update
 * launch (the afm_cfg2_step expression, in place on x, plus the next step's K-padded copy).  The three branches read the same x and the
 * one K-padded copy.  The motion_layer GEMMs store pred_xstart with the plain epilogue, for DDPM too.  AFM_CMDM_PAIR_LAUNCH and
 * AFM_CMDM_FUSED_LN are ignored.  workspace >= afm_cmdm_cfg2_loop_workspace_bytes; sched_scratch as the unguided loop of the same rows. */
int64_t afm_cmdm_cfg2_loop_workspace_bytes(const afm_cmdm_weights* w, int32_t B, int32_t L, int32_t n_streams, const afm_cfg2_args* cfg);
int afm_cmdm_cfg2_loop_range(const afm_cmdm_weights* w, float* x, const float* cond_tokens,
                             const uint8_t* frame_mask, const float* step_noise, const int64_t* d_timestep_map,
                             const afm_ddim_rows* rows, const float* d_c1, const float* d_c2, const float* d_sigma,
                             const afm_cfg2_args* cfg, const float* known, const uint8_t* mask, int32_t n_steps, int32_t first_step,
                             uint64_t seed, int64_t sample_index0, int32_t B, int32_t L, void* sched_scratch, void* workspace,
                             int64_t workspace_bytes, int32_t n_streams, void* const* side_streams, void* stream);

/* The DPM-Solver++(2M) native loop, every form behind one entry: `rows` [T] like the DDIM rows, cfg (one scale) or cfg2 (one scale per
 * condition) or neither (both: AFM_E_BADARG), known / mask [B][L][motion_dim] optional (both or neither).  No noise, no seed.  The
 * launches are those of the eta = 0 DDIM loop of the same form (AFM_CMDM_PAIR_LAUNCH / AFM_CMDM_FUSED_LN as there; branch streams for one
 * scale only), the update launch applying the afm_dpm_step expression to the final pred_xstart - after the guidance combine, the
 * imputation select and the clamp - and keeping that value as the next step's x0_prev in a history buffer [count][L * motion_dim] per
 * sub-batch, carved from the workspace for this loop alone.  first_step == 0: executed step 0 has no history (two-term form).
 * first_step > 0: the history is what the previous range call left in the SAME workspace (same B, L, n_streams, guidance) - chained
 * range calls are bit-identical to one call.  workspace >= afm_cmdm_dpm_loop_workspace_bytes; sched_scratch >=
 * afm_ddim_sched_scratch_bytes(n_steps, B). */
int64_t afm_cmdm_dpm_loop_workspace_bytes(const afm_cmdm_weights* w, int32_t B, int32_t L, int32_t n_streams, const afm_cfg_args* cfg,
                                          const afm_cfg2_args* cfg2);
int afm_cmdm_dpm_loop_range(const afm_cmdm_weights* w, float* x, const float* cond_tokens, const uint8_t* frame_mask,
                            const int64_t* d_timestep_map, const afm_dpm_rows* rows, const afm_cfg_args* cfg, const afm_cfg2_args* cfg2,
                            const float* known, const uint8_t* mask, int32_t n_steps, int32_t first_step, int32_t B, int32_t L,
                            void* sched_scratch, void* workspace, int64_t workspace_bytes, int32_t n_streams, void* const* side_streams,
                            void* stream);

/* ------------------------------------------------------------------------------------------
 * cond_fn guidance (v7-additive).  The reference's condition_mean / condition_score (gaussian_diffusion.py:357-394): a gradient
 * grad = d log p(y | x_t) / d x_t steers the sample.  Both rules are  target += gk[b] * grad  in the sampling update:
 *   DDPM (condition_mean):       gk = posterior_variance[t] (unclipped, 0 at t == 0);  the target is the posterior mean:
 *                                x_next = ((c1 * x0 + c2 * x_t) + gk * grad) + sigma * noise
 *   DDIM / 2M (condition_score): gk = (1 - abar_t) / sqrt(abar_t);  the target is the final pred_xstart, after the guidance combine, the
 *                                imputation select and the clamp:  x0' = x0 + gk * grad,  then the afm_ddim_step / afm_dpm_step expression
 *                                on x0'.  x0' is what a 2M chain keeps as its history.
 * float32, m = gk * grad rounded, then the addition rounded (no contraction).  The host builds gk in float64 and rounds it once.
 * ------------------------------------------------------------------------------------------ */

/* One sampling update with every optional ingredient: the branches of afm_cfg_step (x0_u / scale) or afm_cfg2_step (x0_a / scale2 too),
 * known / mask of afm_impute_step, grad / gk [B][per_sample] / [B] (both or neither: AFM_E_BADARG otherwise; without them grad is never
 * read and the result is the unguided entry's, bit for bit).  Rows: DDPM (c1, c2, sigma), or ddim, or dpm (with x0_prev or NULL) -
 * exactly one kind.  x0_out (optional, ddim with grad or dpm only): the final pred_xstart x0'.  x_next may alias x_t. */
typedef struct {
    const float* x0_c; const float* x0_a; const float* x0_u;        /* [B][per_sample]; x0_a, x0_u optional                */
    const float* scale; const float* scale2;                        /* [B]: with x0_u; scale2 with x0_a                    */
    const float* known; const uint8_t* mask;                        /* [B][per_sample] or NULL                             */
    const float* grad; const float* gk;                             /* [B][per_sample], [B]; both or neither               */
    const float* x_t; const float* noise; float* x_next;            /* [B][per_sample]                                     */
    float* x0_out;                                                  /* [B][per_sample] or NULL                             */
    const float* c1; const float* c2; const float* sigma;           /* DDPM rows [B]                                       */
    const afm_ddim_rows* ddim;                                      /* or DDIM rows [B]                                    */
    const afm_dpm_rows* dpm; const float* x0_prev;                  /* or 2M rows [B] and the history (NULL: two-term)     */
    int32_t clip; int32_t B; int64_t per_sample;
    uint64_t seed; int64_t sample_index0; int32_t step;
} afm_guide_step_args;
int afm_guide_step(const afm_guide_step_args* args, void* stream);

/* Contact guidance: the analytic gradient of the energy between the contact map a motion implies and the map it was given.
 *   p[b,f,k,a] = x[b,f,cols[k]+a] * std[cols[k]+a] + mean[cols[k]+a]           (a = 0..2; absolute joint positions)
 *   d2[b,n,k]  = min over frames f with frame_mask[b,f] == 0 of ((dx*dx + dy*dy) + dz*dz), d = p[b,f,k,:] - q[b,n,:]; f* the FIRST such f
 *   chat       = exp(-d2 / (2 sigma^2)) (no valid frame: chat = 0);   w[b,n,k] = (chat - c[b,n,k]) * chat
 *   energy[b]  = (sum_{n,k} (chat - c)^2) / (N K)
 *   grad[b,f,cols[k]+a] = (scale[b] * coef * std[cols[k]+a]) * S,   S = sum_{n: f*(b,n,k) == f} w * (p_a - q_a),   coef = 2 / (N K sigma^2)
 * which is -scale[b] * dE/dx.  grad is zero in every other column, in masked frames, in a sample without a valid frame and (t != NULL) in
 * a sample with t[b] >= t_start.  Two launches: pass 1 per (b, k, n) with the sample's joint positions in LDS, pass 2 one wave per
 * (b, f, k) summing its points in a fixed order (lane l takes n = l, l + 64, ...; then a fixed butterfly) - no atomics, bit-identical
 * run to run, and a function of the sample alone (no value depends on B or on the sample's place in the batch).  The column triples must
 * lie inside D and must not overlap; K <= AFM_GUIDE_MAX_JOINTS; K * L * 3 floats must fit the LDS (AFM_E_UNSUPPORTED).
 *
 * HumanML3D features (`h3d`, D = 263; v7-additive: afm_contact_guide.h3d, NULL = the absolute columns above).  The motion vector holds no
 * joint positions: with u = x * std + mean (columns 0..66 are read; D >= 67) and the velocity columns 0..2 of a padded frame taken as zero,
 *   th_f = sum_{g<f} u[g,0]  (the reference's HALF angle);  c_f = cos(2 th_f), s_f = sin(2 th_f)
 *   X_f = sum_{1<=h<=f} (u[h-1,1] c_h - u[h-1,2] s_h),   Z_f = sum_{1<=h<=f} (u[h-1,1] s_h + u[h-1,2] c_h),   Y_f = u[f,3]
 *   joint 0: P = (X_f, Y_f, Z_f);   joint j = 1..21, l = u[f, 4+3(j-1) ..]: P = (l_x c_f - l_z s_f + X_f, l_y, l_x s_f + l_z c_f + Z_f)
 *   p = A P + t,  to_scene = [A|t] (3 x 4 row-major; the reference does not fix how an h3d motion lies in its scene, e.g. y-up to z-up:
 *   A = [[1,0,0],[0,0,-1],[0,1,0]], t = 0)
 * which is recover_from_ric(data, 22) of the reference's utils/visualize.py on valid-frames-first masks.  Everything behind p is the
 * guidance above; grad is the adjoint of the recovery applied to A^T S, scaled per column as above: nonzero only in columns 0..66 of valid
 * frames.  Four launches: the recovery (one block per sample; positions [K][L][3], c and s to the workspace), passes 1 and 2 reading those
 * positions (pass 2 leaves S[b,f,k,:] in the workspace), the adjoint (one block per sample, reads c and s back, writes complete rows).
 * Every scan over the frames is one lane's serial chain in frame order: no value depends on B, on the sample's place or on L's wave shape.
 * 7 * L floats must fit the LDS too (AFM_E_UNSUPPORTED). */
#define AFM_GUIDE_MAX_JOINTS 16
#define AFM_H3D_JOINTS 22
typedef struct {
    int32_t joints[AFM_GUIDE_MAX_JOINTS];  /* joint index 0..21 of guided joint k (K of afm_contact_guide; no joint twice)  */
    const float* to_scene;                 /* device [3][4], or [B][3][4] with to_scene_stride 12; NULL: the identity      */
    int32_t to_scene_stride;               /* floats between two samples' matrices: 0 (one shared) or 12                   */
} afm_h3d_layout;
typedef struct {
    const float* q;                       /* device [B][N][3]: the scene points                                          */
    const float* c;                        /* device [B][N][K]: the target contact map, un-normalised exp(-d^2 / 2 sigma^2) */
    const float* mean; const float* std;   /* device [D]: de-normalisation of the motion                                  */
    const float* scale;                    /* device [B]                                                                  */
    const float* gk;                       /* loops only: device [T][B], row i = the coefficient of spaced timestep i     */
    const uint8_t* frame_mask;             /* loops only: device [B][L], nonzero = padded frame, or NULL - the guidance's own mask (x_mask),
                                              whether or not the denoiser masks its motion tokens                          */
    int32_t cols[AFM_GUIDE_MAX_JOINTS];    /* column of x of joint k (y, z: the next two)                                 */
    int32_t K; int32_t N;
    double sigma;                          /* of the contact map; 2 sigma^2 and the coefficient are formed in float64 and rounded once */
    int32_t first_guided;                  /* loops only: executed steps (first_step + j) below it run unguided - no gradient launch */
    int64_t t_start;                       /* afm_contact_guidance with t: samples with t[b] >= t_start get a zero gradient */
    const afm_h3d_layout* h3d;             /* NULL: `cols` name absolute positions; set: x holds HumanML3D features, `cols` is ignored */
} afm_contact_guide;

/* grad [B][L][D] and / or energy [B] (either may be NULL) of x [B][L][D]; frame_mask [B][L] (nonzero = padded) or NULL; t [B] or NULL.
 * The workspace: afm_contact_guidance_workspace_bytes (absolute columns), afm_contact_guidance_h3d_workspace_bytes (g->h3d set: the
 * positions, c / s and S scale with B * L * K). */
int64_t afm_contact_guidance_workspace_bytes(int32_t B, int32_t N, int32_t K);
int64_t afm_contact_guidance_h3d_workspace_bytes(int32_t B, int32_t L, int32_t N, int32_t K);
int afm_contact_guidance(const afm_contact_guide* g, const float* x, const uint8_t* frame_mask, const int64_t* t, float* grad,
                         float* energy, int32_t B, int32_t L, int32_t D, void* workspace, int64_t workspace_bytes, void* stream);

/* The joint positions of a HumanML3D-feature motion (the reference's recover_from_ric, on the device): out [B][L][J][3] of x [B][L][D] for
 * the joint list `joints` [J] (host; NULL: all 22 in order, J ignored), with mean / std device [D], frame_mask [B][L] or NULL (a padded
 * frame's velocities count as zero; its own row still gives its height and local coordinates) and to_scene as in afm_h3d_layout.  One
 * launch of the recovery kernel the guidance uses.  AFM_E_BADARG: D < 67, J outside 1..22, a joint outside 0..21 or named twice, a stride
 * other than 0 / 12; AFM_E_UNSUPPORTED: 7 * L floats beyond the LDS. */
int afm_h3d_joints(const float* x, const float* mean, const float* std, const uint8_t* frame_mask, const int32_t* joints, int32_t J,
                   const float* to_scene, int32_t to_scene_stride, float* out, int32_t B, int32_t L, int32_t D, void* stream);

/* The contact-guided native loop, every form behind one entry: DDPM (d_c1 / d_c2 / d_sigma), DDIM (rows) or 2M (dpm; no noise) - exactly
 * one kind of rows; cfg or cfg2 or neither; known / mask optional (both or neither); guide required.  The loop runs in the
 * separate-update form (as an imputing loop: the update fused into the motion_layer epilogue has no place for the term).  Per sub-batch
 * and executed step first_step + j >= guide->first_guided, on the sub-batch's stream and in front of the evaluations, the two launches
 * of afm_contact_guidance on the x the evaluations read, with guide->frame_mask (not the denoiser's frame_mask, which a model
 * without motion masking does not have); the update launch takes grad and gk row n_steps - 1 - j.  Earlier steps launch
 * what an imputing loop of the same form launches (grad NULL).  guide->q / c / scale / gk cover the whole batch.  A 2M history buffer is
 * always carved, so chained range calls share one layout.  workspace >= afm_cmdm_guide_loop_workspace_bytes.  A description with
 * guide->h3d set runs through the same entry: four gradient launches per guided step in place of two, the workspace sized for them. */
int64_t afm_cmdm_guide_loop_workspace_bytes(const afm_cmdm_weights* w, int32_t B, int32_t L, int32_t n_streams, const afm_cfg_args* cfg,
                                            const afm_cfg2_args* cfg2, const afm_contact_guide* guide);
int afm_cmdm_guide_loop_range(const afm_cmdm_weights* w, float* x, const float* cond_tokens, const uint8_t* frame_mask,
                              const float* step_noise, const int64_t* d_timestep_map, const afm_ddim_rows* rows, const afm_dpm_rows* dpm,
                              const float* d_c1, const float* d_c2, const float* d_sigma, const afm_cfg_args* cfg,
                              const afm_cfg2_args* cfg2, const float* known, const uint8_t* mask, const afm_contact_guide* guide,
                              int32_t n_steps, int32_t first_step, uint64_t seed, int64_t sample_index0, int32_t B, int32_t L,
                              void* sched_scratch, void* workspace, int64_t workspace_bytes, int32_t n_streams, void* const* side_streams,
                              void* stream);

/* Joint-position targets (v7-additive): "joint k is at target[b,f,k,:] in the scene at frame f", a second energy on the joint positions
 * p[b,f,k,:] the contact guidance computes - the columns of x (cols; p = x * std rounded, + mean rounded) or, with `h3d` set, the output
 * of the recovery kernel for the layout's joints.  float32, every operation rounded on its own:
 *   E[b] = sum over valid frames f and joints k of  w * ((dx*dx + dy*dy) + dz*dz),   d = p - target,   w = weight[b,f,k]
 * not normalised.  The sum's order: the items e = f * K + k of a sample are dealt to the 256 threads of one block, thread i adds
 * e = i, i + 256, ... in that order to 0, then the fixed butterfly of a wave and ((r0 + r1) + r2) + r3 over the four waves - a function of
 * the sample alone.  An item with w == 0 or in a padded frame adds exactly 0, and its target is NOT READ (it may be NaN).
 *   column form:  d = target_a - p_a;  m = w * d;  grad[b,f,cols[k]+a] = ((scale[b] * 2) * std_a) * m       (one launch)
 *   h3d form:     S[b,f,k,:] = w * (target - p) (zero where w == 0 or the frame is padded), carried through the adjoint of the recovery with
 *                 coef = 2 exactly as the contact guidance carries its S: three launches - recovery, targets, adjoint.  Joint 0 is the root.
 * which is -scale[b] * dE/dx.  grad is exactly zero in every other column, in padded frames, where w == 0 and (t != NULL) in a sample with
 * t[b] >= t_start.  No atomics. */
typedef struct {
    const float* target;                   /* device [B][L][K][3]: scene coordinates                                      */
    const float* weight;                   /* device [B][L][K]: 0 = no target (the target value is not read)              */
    const float* scale;                    /* device [B]                                                                  */
    const float* mean; const float* std;   /* device [D]: de-normalisation of the motion                                  */
    int32_t cols[AFM_GUIDE_MAX_JOINTS];    /* column of x of joint k (y, z: the next two); ignored with `h3d`             */
    int32_t K;
    int32_t first_guided;                  /* loops only: executed steps (first_step + j) below it do not carry this term */
    int64_t t_start;                       /* with t: samples with t[b] >= t_start get a zero gradient                    */
    const afm_h3d_layout* h3d;             /* NULL: `cols` name absolute positions; set: x holds HumanML3D features       */
} afm_joint_targets;

/* The sum of the two guidances: grad = grad_contact + grad_targets, each term the float32 result of that guidance alone, joined by one
 * rounded addition per element (the targets' launch - the column kernel, or the adjoint - adds its complete result to what the contact
 * term wrote; a sample with t[b] >= a term's t_start gets zeros from that term).  At least one of contact / targets is set; both set: they
 * name the same mean / std, the same form, and the same to_scene (pointer and stride).  Through this struct contact->gk and
 * contact->frame_mask are not read.  The recovery of an h3d motion runs once per term (the two joint lists may differ).  Launches: the
 * contact term's 2 (h3d: 4), plus the targets' 1 (h3d: 3). */
typedef struct {
    const afm_contact_guide* contact;      /* or NULL                                                                     */
    const afm_joint_targets* targets;      /* or NULL                                                                     */
    const float* gk;                       /* loops only: device [T][B], row i = the coefficient of spaced timestep i     */
    const uint8_t* frame_mask;             /* loops only: device [B][L], nonzero = padded frame, or NULL                  */
} afm_motion_guide;

/* grad [B][L][D] and / or the two energies [B] (each may be NULL; an energy of a term that is not set must be NULL) of x [B][L][D];
 * frame_mask [B][L] or NULL; t [B] or NULL.  AFM_E_BADARG before anything is enqueued: neither term set, K outside 1..16, column triples
 * that overlap or leave D, a joint outside 0..21 or named twice, D < 67 with h3d, terms that disagree (above). */
int64_t afm_motion_guidance_workspace_bytes(const afm_motion_guide* g, int32_t B, int32_t L, int32_t D);
int afm_motion_guidance(const afm_motion_guide* g, const float* x, const uint8_t* frame_mask, const int64_t* t, float* grad,
                        float* energy_contact, float* energy_targets, int32_t B, int32_t L, int32_t D, void* workspace,
                        int64_t workspace_bytes, void* stream);

/* afm_cmdm_guide_loop_range with the description swapped: the same loop body, the step's gradient the sum above over the terms whose own
 * first_guided the executed step has reached (a term not yet reached launches nothing and contributes exactly zero; no term reached: the
 * step launches what an imputing loop launches).  Also AFM_E_BADARG: g->gk missing, a negative first_guided. */
int64_t afm_cmdm_motion_guide_loop_workspace_bytes(const afm_cmdm_weights* w, int32_t B, int32_t L, int32_t n_streams, const afm_cfg_args* cfg,
                                                   const afm_cfg2_args* cfg2, const afm_motion_guide* guide);
int afm_cmdm_motion_guide_loop_range(const afm_cmdm_weights* w, float* x, const float* cond_tokens, const uint8_t* frame_mask,
                                     const float* step_noise, const int64_t* d_timestep_map, const afm_ddim_rows* rows, const afm_dpm_rows* dpm,
                                     const float* d_c1, const float* d_c2, const float* d_sigma, const afm_cfg_args* cfg,
                                     const afm_cfg2_args* cfg2, const float* known, const uint8_t* mask, const afm_motion_guide* guide,
                                     int32_t n_steps, int32_t first_step, uint64_t seed, int64_t sample_index0, int32_t B, int32_t L,
                                     void* sched_scratch, void* workspace, int64_t workspace_bytes, int32_t n_streams, void* const* side_streams,
                                     void* stream);

/* Scene clearance (v7-additive): the one term that pushes - every joint-frame is pushed off the obstacle points of the scene cloud that lie
 * inside the joint's radius.  p[b,f,k,:] are the positions the other terms use (the de-normalised columns, or with `h3d` the recovery
 * kernel's output); q = the scene points [B][N][3].  The obstacle weight of a point, decided once per point:
 *   w[b,n] = weight[b,n] (1 where weight == NULL), but 0 if  (has_min_height and q[b,n,up] < min_height)  - the floor -
 *            or  (exempt and max_j c[b,n,j] >= c_min, j < Kc)  - points the contact map marks stay reachable
 * (both comparisons are exact: the float32 value against the double threshold).  float32, every operation rounded on its own, with
 * ir2[k] = (float)(1 / r_k^2) and coef[k] = (float)(4 / r_k^2), each formed in float64 and rounded once:
 *   d  = p[b,f,k,:] - q[b,n,:];   d2 = (dx*dx + dy*dy) + dz*dz;   u = max(0, 1 - d2 * ir2[k]);   wu = w * u
 *   E[b]       = sum over valid frames f, joints k, points n of  wu * u                      (not normalised)
 *   S[b,f,k,a] = sum_n wu * d_a
 *   column form:  grad[b,f,cols[k]+a] = ((scale[b] * coef[k]) * std_a) * S_a                  (one launch)
 *   h3d form:     (coef[k] * S_a), rounded, goes to S[b][f][k][3] and through the recovery's adjoint with coef = 1, i.e. with scale[b]
 *                 alone (three launches: recovery, clearance, adjoint)
 * which is -scale[b] * dE/dx: u * u and its derivative both vanish at d = r.  grad is exactly zero in every other column, in padded
 * frames, in a sample with t[b] >= t_start and in a joint-frame with no obstacle point inside its radius; a sample whose frames are all
 * padded has E = 0.  A point with wu == 0 adds nothing and is skipped.
 * The order of the sums (no atomics; a function of the sample alone - not of B, of the sample's place or of the run): the kernel runs
 * AFM_CLEAR_WAVES = 8 waves per block on tiles of AFM_CLEAR_TILE = 1024 points.  For one joint-frame, wave v adds, from 0 and in ascending
 * n, the points with (n mod 1024) / 128 == v; then S = ((((((s_0 + s_1) + s_2) + s_3) + s_4) + s_5) + s_6) + s_7, and the joint-frame's
 * energy e likewise.  E[b]: a block of whole frames holds at most 64 joint-frames i = (f - f0) * K + k, f0 = block * (64 / K); lane i adds
 * its e over the blocks in ascending block order (a padded frame's e counts as 0), then the fixed butterfly of one wave.  The energy is
 * computed by the sample's first block alone (a score, not part of a sampling step).
 * Any N fits (the points are tiled through 16 KiB of LDS); AFM_E_UNSUPPORTED: L or B beyond 65535, 7 * L floats beyond the LDS with h3d. */
#define AFM_CLEAR_WAVES 8
#define AFM_CLEAR_TILE 1024
typedef struct {
    const float* q;                        /* device [B][N][3]: the scene points                                          */
    const float* weight;                   /* device [B][N] or NULL (every point weighs 1)                                */
    const float* c;                        /* device [B][N][Kc]: the contact map of the exemption, or NULL                */
    const float* mean; const float* std;   /* device [D]: de-normalisation of the motion                                  */
    const float* scale;                    /* device [B]                                                                  */
    int32_t cols[AFM_GUIDE_MAX_JOINTS];    /* column of x of joint k (y, z: the next two); ignored with `h3d`             */
    int32_t K; int32_t N;
    int32_t Kc;                            /* columns of c                                                                */
    int32_t exempt;                        /* nonzero: points with max_j c >= c_min weigh 0 (needs c)                     */
    double c_min;
    double radius[AFM_GUIDE_MAX_JOINTS];   /* r_k > 0                                                                     */
    int32_t up;                            /* 0..2: the coordinate min_height is compared with                            */
    int32_t has_min_height;                /* nonzero: points with q[up] < min_height weigh 0                             */
    double min_height;
    int32_t first_guided;                  /* loops only: executed steps (first_step + j) below it do not carry this term */
    int64_t t_start;                       /* with t: samples with t[b] >= t_start get a zero gradient                    */
    const afm_h3d_layout* h3d;             /* NULL: `cols` name absolute positions; set: x holds HumanML3D features       */
} afm_scene_clearance;

/* The sum of the three terms: grad = (grad_contact + grad_targets) + grad_clearance, each term the float32 result of that term alone,
 * joined by one rounded addition per element in that order (the clearance launch - the column kernel, or the adjoint - adds its complete
 * result to what the terms in front of it wrote); a term that is not set contributes nothing.  At least one term is set; the clearance
 * and `terms` agree exactly as the two terms of afm_motion_guide must: the same mean / std, the same form, the same to_scene (pointer
 * and stride).  The gk and frame_mask of `terms` are not read through this struct. */
typedef struct {
    const afm_motion_guide* terms;         /* or NULL                                                                     */
    const afm_scene_clearance* clearance;  /* or NULL                                                                     */
    const float* gk;                       /* loops only: device [T][B], row i = the coefficient of spaced timestep i     */
    const uint8_t* frame_mask;             /* loops only: device [B][L], nonzero = padded frame, or NULL                  */
} afm_scene_guide;

/* grad [B][L][D] and / or the three energies [B] (each may be NULL; an energy of a term that is not set must be NULL) of x [B][L][D];
 * frame_mask [B][L] or NULL; t [B] or NULL.  AFM_E_BADARG before anything is enqueued: no term set, what afm_motion_guidance refuses, a
 * radius that is not positive, `up` outside 0..2, an exemption without c (or with Kc <= 0), terms that disagree (above). */
int64_t afm_scene_guidance_workspace_bytes(const afm_scene_guide* g, int32_t B, int32_t L, int32_t D);
int afm_scene_guidance(const afm_scene_guide* g, const float* x, const uint8_t* frame_mask, const int64_t* t, float* grad,
                       float* energy_contact, float* energy_targets, float* energy_clearance, int32_t B, int32_t L, int32_t D,
                       void* workspace, int64_t workspace_bytes, void* stream);

/* afm_cmdm_motion_guide_loop_range with the description swapped: the same loop body, the step's gradient the sum above over the terms
 * whose own first_guided the executed step has reached (a term not yet reached launches nothing and contributes exactly zero).  The
 * clearance adds one launch per guided step and sub-batch (h3d: three).  Also AFM_E_BADARG: g->gk missing, a negative first_guided. */
int64_t afm_cmdm_scene_guide_loop_workspace_bytes(const afm_cmdm_weights* w, int32_t B, int32_t L, int32_t n_streams, const afm_cfg_args* cfg,
                                                  const afm_cfg2_args* cfg2, const afm_scene_guide* guide);
int afm_cmdm_scene_guide_loop_range(const afm_cmdm_weights* w, float* x, const float* cond_tokens, const uint8_t* frame_mask,
                                    const float* step_noise, const int64_t* d_timestep_map, const afm_ddim_rows* rows, const afm_dpm_rows* dpm,
                                    const float* d_c1, const float* d_c2, const float* d_sigma, const afm_cfg_args* cfg,
                                    const afm_cfg2_args* cfg2, const float* known, const uint8_t* mask, const afm_scene_guide* guide,
                                    int32_t n_steps, int32_t first_step, uint64_t seed, int64_t sample_index0, int32_t B, int32_t L,
                                    void* sched_scratch, void* workspace, int64_t workspace_bytes, int32_t n_streams, void* const* side_streams,
                                    void* stream);

/* Foot grounding (v7-additive): no floor penetration, no foot skating - the one term that couples frame f with frame f + 1.  p[b,f,k,:]
 * are the positions the other terms use (the de-normalised columns, or with `h3d` the recovery kernel's output).  float32, every operation
 * rounded on its own, with ih[k] = (float)(1 / height[k]), fw = (float)floor_weight, sw = (float)skate_weight,
 * cf = (float)(2 * floor_weight) and cs = (float)(2 * skate_weight), each formed in float64 and rounded once; a, b = the two axes that are
 * not `up`, a < b:
 *   h      = p[b,f,k,up] - (float)floor
 *   pen    = max(0, -h)                                          depth below the floor
 *   g      = min(1, max(0, 1 - h * ih[k]))                       1 at / below the floor, 0 at / above height[k]
 *   s[f,k] = g[f,k] * g[f+1,k]  if the frames f and f + 1 both exist and are valid, else 0                       (labels == 0)
 *   s[f,k] = min(1, max(0, x[b,f,259+slot(k)] * std + mean))  under the same validity rule                       (labels != 0, h3d only)
 *   dl_a   = p[b,f+1,k,a] - p[b,f,k,a]
 *   E[b]   = sum over valid f, k of  fw * (pen * pen) + sw * (s[f,k] * (dl_a * dl_a + dl_b * dl_b))
 *   m[f,k,up] = cf * pen;   m[f,k,a] = cs * (s[f,k] * dl_a[f] - s[f-1,k] * dl_a[f-1])     (a missing or invalid pair contributes 0)
 *   column form:  grad[b,f,cols[k]+a] = (scale[b] * std_a) * m_a                                                  (one launch)
 *   h3d form:     S[b][f][k][3] = m goes through the recovery's adjoint with coef = 1, i.e. with scale[b] alone    (three launches:
 *                 recovery, grounding, adjoint)
 * grad is -scale[b] * dE/dx WITH THE PAIR WEIGHTS s HELD CONSTANT - on purpose: a sliding foot is slowed down, it is not lifted out of
 * contact to escape the penalty.  The floor part is the exact gradient.  grad is exactly zero in every other column, in padded frames, in
 * a sample with t[b] >= t_start, in a sample without a valid frame (E = 0) and in a joint-frame that neither penetrates the floor nor
 * belongs to a pair with s > 0.
 * labels: HumanML3D's own foot-contact columns 259..262 weight the pairs; its feature layout puts the left foot (joints 7, 10) before the
 * right one (8, 11): slot = {7: 0, 10: 1, 8: 2, 11: 3}; the label of frame f describes the step f -> f + 1.  (The convention is
 * HumanML3D's; the project this library follows holds no code that reads these columns.)  Needs `h3d`, D >= 263 and joints out of
 * {7, 10, 8, 11}: AFM_E_BADARG otherwise.
 * One launch: a block of 256 threads owns 8 frames of one sample and holds their K x 3 positions, and those of one neighbouring frame on
 * either side, in LDS; the weight of a pair is recomputed by both of its frames from the same staged values.  Every element of grad is
 * the result of one expression: there is no sum across threads in it.
 * The order of the energy's sum (no atomics; a function of the sample alone - not of B, of the sample's place or of the run): the sample's
 * first block stages the sample's L x K x 3 positions; thread i adds, from 0, the items e = f * K + k = i, i + 256, ... in that order (an
 * item of a padded frame is skipped), item = fw * (pen * pen) + sw * (s * (dl_a * dl_a + dl_b * dl_b)) with the second addend 0 where
 * s == 0; then the fixed butterfly of each wave and ((r0 + r1) + r2) + r3 over the four waves.  (A score, not part of a sampling step.)
 * AFM_E_UNSUPPORTED: (3 K + 1) L floats beyond 60 KiB of LDS, L or B beyond 65535, 7 * L floats beyond the LDS with h3d. */
typedef struct {
    const float* mean; const float* std;   /* device [D]: de-normalisation of the motion                                  */
    const float* scale;                    /* device [B]                                                                  */
    int32_t cols[AFM_GUIDE_MAX_JOINTS];    /* column of x of joint k (y, z: the next two); ignored with `h3d`             */
    int32_t K;
    int32_t up;                            /* 0..2: the coordinate that is the height                                     */
    int32_t labels;                        /* nonzero: the pair weights are the motion's own foot-contact columns         */
    int32_t first_guided;                  /* loops only: executed steps (first_step + j) below it do not carry this term */
    double floor;                          /* the floor's height along `up`                                               */
    double height[AFM_GUIDE_MAX_JOINTS];   /* > 0: joint k counts as planted at the floor, as free at floor + height[k]   */
    double floor_weight; double skate_weight;  /* both >= 0, not both 0                                                   */
    int64_t t_start;                       /* with t: samples with t[b] >= t_start get a zero gradient                    */
    const afm_h3d_layout* h3d;             /* NULL: `cols` name absolute positions; set: x holds HumanML3D features       */
} afm_foot_grounding;

/* The sum of the four terms: grad = ((grad_contact + grad_targets) + grad_clearance) + grad_feet, each term the float32 result of that
 * term alone, joined by one rounded addition per element in that order (the grounding's launch - the column kernel, or the adjoint - adds
 * its complete result to what the terms in front of it wrote); a term that is not set contributes nothing.  At least one term is set; the
 * grounding and the terms in front agree as the terms of afm_scene_guide must: the same mean / std, the same form, the same to_scene.
 * The gk and frame_mask of `terms` are not read through this struct. */
typedef struct {
    const afm_scene_guide* terms;          /* or NULL                                                                     */
    const afm_foot_grounding* feet;        /* or NULL                                                                     */
    const float* gk;                       /* loops only: device [T][B], row i = the coefficient of spaced timestep i     */
    const uint8_t* frame_mask;             /* loops only: device [B][L], nonzero = padded frame, or NULL                  */
} afm_ground_guide;

/* grad [B][L][D] and / or the four energies [B] (each may be NULL; an energy of a term that is not set must be NULL) of x [B][L][D];
 * frame_mask [B][L] or NULL; t [B] or NULL.  AFM_E_BADARG before anything is enqueued: no term set, what afm_scene_guidance refuses, a
 * height that is not positive, `up` outside 0..2, a negative weight or both 0, labels without h3d / with D < 263 / with another joint,
 * terms that disagree (above).  AFM_E_WORKSPACE: a workspace below afm_ground_guidance_workspace_bytes. */
int64_t afm_ground_guidance_workspace_bytes(const afm_ground_guide* g, int32_t B, int32_t L, int32_t D);
int afm_ground_guidance(const afm_ground_guide* g, const float* x, const uint8_t* frame_mask, const int64_t* t, float* grad,
                        float* energy_contact, float* energy_targets, float* energy_clearance, float* energy_feet, int32_t B, int32_t L,
                        int32_t D, void* workspace, int64_t workspace_bytes, void* stream);

/* afm_cmdm_scene_guide_loop_range with the description swapped: the same loop body, the step's gradient the sum above over the terms
 * whose own first_guided the executed step has reached (a term not yet reached launches nothing and contributes exactly zero).  The
 * grounding adds one launch per guided step and sub-batch (h3d: three).  Also AFM_E_BADARG: g->gk missing, a negative first_guided.
 * Stitched and long descriptions take no grounding. */
int64_t afm_cmdm_ground_guide_loop_workspace_bytes(const afm_cmdm_weights* w, int32_t B, int32_t L, int32_t n_streams, const afm_cfg_args* cfg,
                                                   const afm_cfg2_args* cfg2, const afm_ground_guide* guide);
int afm_cmdm_ground_guide_loop_range(const afm_cmdm_weights* w, float* x, const float* cond_tokens, const uint8_t* frame_mask,
                                     const float* step_noise, const int64_t* d_timestep_map, const afm_ddim_rows* rows, const afm_dpm_rows* dpm,
                                     const float* d_c1, const float* d_c2, const float* d_sigma, const afm_cfg_args* cfg,
                                     const afm_cfg2_args* cfg2, const float* known, const uint8_t* mask, const afm_ground_guide* guide,
                                     int32_t n_steps, int32_t first_step, uint64_t seed, int64_t sample_index0, int32_t B, int32_t L,
                                     void* sched_scratch, void* workspace, int64_t workspace_bytes, int32_t n_streams, void* const* side_streams,
                                     void* stream);

/* ------------------------------------------------------------------------------------------
 * Long motions as overlapping windows (v7-additive).  G long motions are B = G * S samples [B][L][D]: sample g * S + w is window w of
 * motion g and holds the long frames w * (L - overlap) .. w * (L - overlap) + L - 1, so neighbouring windows share `overlap` frames and,
 * with 2 * overlap <= L, a frame lies in at most two windows.  The windows are denoised side by side; at every step the frames two
 * windows share get ONE pred_xstart: for f = 0 .. overlap - 1, the earlier window's frame L - overlap + f ("left") and the later
 * window's frame f ("right") both become
 *     v = (wl[f] * x0_left) + (wr[f] * x0_right)          float32, each product rounded, then the sum (no contraction)
 * with the weight row `weights` = device [2][overlap], wl then wr; the host forms wr[f] = (f + 1) / (overlap + 1), wl[f] = 1 - wr[f] in
 * float64 and rounds once.  Both windows evaluate the same expression on the same operands: with a deterministic update (DDIM eta = 0,
 * DPM-Solver++(2M)) and shared frames that start from the same noise, the shared frames stay bit-identical in both windows at every
 * step.  Order inside a sampling update: guidance combine (each window with its own scales) -> blend -> imputation select -> clamp ->
 * update; a 2M history keeps the blended value.  windows == 1 or overlap == 0: no blend.  A long motion of F frames,
 * (S - 1) * (L - overlap) + overlap < F <= S * L - (S - 1) * overlap, leaves a padded tail in the last window only, outside every overlap.
 * ------------------------------------------------------------------------------------------ */
typedef struct {
    int32_t windows;          /* S >= 1: windows per long motion; the batch is a multiple of it                 */
    int32_t overlap;          /* frames two neighbouring windows share; 2 * overlap <= L                        */
    const float* weights;     /* device [2][overlap]: wl then wr (may be NULL when nothing is blended)          */
} afm_stitch;

/* The blend of an x0 [B][L][D] alone; out may be x0 (one thread owns both copies of a shared element).  No blend: out = x0's bits.
 * AFM_E_BADARG: B % windows != 0, 2 * overlap > L, a NULL tensor, weights missing where something is blended. */
int afm_stitch_blend(const float* x0, float* out, const afm_stitch* stitch, int32_t B, int32_t L, int32_t D, void* stream);

/* windows [G * S][L][D] of long_motion [G][F][D] (a frame at or behind F: zeros) and back (a shared frame is read from the later
 * window).  Copies.  AFM_E_BADARG: F outside the range above, 2 * overlap > L, more than 65535 samples. */
int afm_stitch_windows(const float* long_motion, float* windows, int32_t G, int32_t S, int32_t overlap, int32_t L, int32_t D, int32_t F,
                       void* stream);
int afm_stitch_join(const float* windows, float* long_motion, int32_t G, int32_t S, int32_t overlap, int32_t L, int32_t D, int32_t F,
                    void* stream);

/* One stitched sampling update in ONE launch, the order above: the branches of afm_cfg_step (x0_u / scale) or afm_cfg2_step (x0_a /
 * scale2 too), the blend - in an overlap the kernel also reads the neighbour sample's x0 buffers, overlap * D values on or back, and
 * combines them with the neighbour's scales - known / mask, the clamp, then the afm_ddim_step expression (ddim, sigma NULL) or the
 * afm_dpm_step expression (dpm, with x0_prev or NULL; x0_out, optional, receives the final blended x0).  Exactly one kind of rows;
 * rows with a noise term are refused (the step noise of shared frames would have to be shared).  x_next may alias x_t; neither x_next
 * nor x0_out may alias an x0 buffer. */
typedef struct {
    const float* x0_c; const float* x0_a; const float* x0_u;        /* [B][L][D]; x0_a, x0_u optional                      */
    const float* scale; const float* scale2;                        /* [B]: with x0_u; scale2 with x0_a                    */
    const float* known; const uint8_t* mask;                        /* [B][L][D] or NULL                                   */
    const float* x_t; float* x_next;                                /* [B][L][D]                                           */
    float* x0_out;                                                  /* dpm only: [B][L][D] or NULL                         */
    const afm_ddim_rows* ddim;                                      /* DDIM rows [B], sigma NULL                           */
    const afm_dpm_rows* dpm; const float* x0_prev;                  /* or 2M rows [B] and the history (NULL: two-term)     */
    const afm_stitch* stitch;
    int32_t clip; int32_t B; int32_t L; int32_t D;
} afm_stitch_step_args;
int afm_stitch_step(const afm_stitch_step_args* args, void* stream);

/* The stitched native loop: afm_cmdm_guide_loop_range's signature with the stitch description in the guidance's place, built the same
 * way (the separate-update form of an imputing loop; a 2M history buffer is always carved).  rows (eta = 0: sigma NULL) or dpm - exactly
 * one; cfg or cfg2 or neither; known / mask or neither (they must agree in the overlaps: a description that does not is the caller's
 * error).  The update launch of every step is the stitched one above, in place on x.  Sub-batches are cut over long motions - a window and
 * its neighbour always share a sub-batch and a stream - n_streams > 1: at most one sub-batch per long motion; the sizer uses the same rule.
 * AFM_E_BADARG: DDPM rows (d_c1 / d_c2 / d_sigma), rows with a noise term, a step_noise, B % windows != 0, 2 * overlap > L.  seed and
 * sample_index0 are unused (no noise is drawn).  Chained range calls on one workspace are bit-identical to one call. */
int64_t afm_cmdm_stitch_loop_workspace_bytes(const afm_cmdm_weights* w, int32_t B, int32_t L, int32_t n_streams, const afm_cfg_args* cfg,
                                             const afm_cfg2_args* cfg2, const afm_stitch* stitch);
int afm_cmdm_stitch_loop_range(const afm_cmdm_weights* w, float* x, const float* cond_tokens, const uint8_t* frame_mask,
                               const float* step_noise, const int64_t* d_timestep_map, const afm_ddim_rows* rows, const afm_dpm_rows* dpm,
                               const float* d_c1, const float* d_c2, const float* d_sigma, const afm_cfg_args* cfg,
                               const afm_cfg2_args* cfg2, const float* known, const uint8_t* mask, const afm_stitch* stitch,
                               int32_t n_steps, int32_t first_step, uint64_t seed, int64_t sample_index0, int32_t B, int32_t L,
                               void* sched_scratch, void* workspace, int64_t workspace_bytes, int32_t n_streams, void* const* side_streams,
                               void* stream);

/* ------------------------------------------------------------------------------------------
 * Guidance of stitched long motions (v7-additive): the contact and joint-target terms evaluated on the JOINED motion, so a target or a
 * root path may lie beyond the first window and an h3d root is integrated from long frame 0.
 *
 * stitch: S windows, overlap ov, `frames` = F long frames; hop = L - ov.  Window w of long motion g is batch row b = g * S + w and holds the
 * long frames a_w = w * hop .. a_w + L - 1, clipped to < F.  In a stitched chain the shared frames are bit-identical in both windows at
 * every step, so the windows join into one long x_t.  With x [G * S][L][D]:
 *   1. long = afm_stitch_join(x) [G][F][D] (a shared frame is read from the later window).
 *   2. P[g,f,k,:] = the positions of `long` exactly as the kernels above compute them: the de-normalised columns, or the h3d recovery over
 *      all F frames.  float32, every operation in its present order.
 *   3. Targets term: the afm_motion_guidance targets launches on (long, B = G, L = F); target / weight are long-form [G][F][K][3] /
 *      [G][F][K].  Its value is by definition targets(long).
 *   4. Contact term, per window b (q [G * S][N][3] and c [G * S][N][K]: each window keeps its own map):
 *      d2[b,n,k] = min over the window's long frames f of |P[g,f,k] - q[b,n]|^2, summed (dx*dx + dy*dy) + dz*dz; f* the first such frame,
 *      stored as a long frame index; chat and w as above; E_b = sum (chat - c)^2 / (N K) with the partial and serial sums above;
 *      S_b[f,k,:] = sum over {n: f*(b,n,k) = f} of w * (p - q) in the frame_sum order above.
 *   5. Per long frame the windows' sums are joined: a frame in one window takes that window's sum as is, a frame in two windows takes
 *      S_earlier + S_later - one rounded addition, earlier window first.  With w1 = min(f / hop, S - 1) the earlier window w1 - 1 also
 *      holds f iff w1 > 0 and f - w1 * hop < ov.
 *   6. Column form: grad_long[g,f,col+a] = ((scale[g] * coef) * std_a) * S.  h3d form: the joined S goes through the adjoint kernel on
 *      (B = G, L = F) with scale[g].
 *   7. The targets' launch adds its complete result to what the contact term wrote, as afm_motion_guidance does.
 *   8. grad = afm_stitch_windows(grad_long): the padded tail is exact zeros, both copies of a shared frame hold the same bits.
 * The terms' `scale` rows are [G]; to_scene is [3][4] or [G][3][4]; no frame mask is read - validity is the geometry (long frames
 * 0 .. F-1 are valid, the padded tail of a last window does not exist in the long form).  t [G * S] or NULL: long motion g has t[g * S].
 * energy_contact[g] = the serial sum of its windows' E_b in window order; energy_targets[g] = the targets' energy of the long motion.
 * No atomics: a long motion's result depends neither on G nor on its place in the batch.  Launches with a gradient: join, the contact
 * term's 2 (h3d: 4), the targets' 1 (h3d: 3), windows (+1 copying t when t is given).
 * AFM_E_BADARG: the checks of afm_motion_guidance (on L for the contact staging, on F for the targets), a geometry F outside
 * (S-1) hop + ov < F <= S L - (S-1) ov, B % S != 0.  AFM_E_UNSUPPORTED: 7 * F floats beyond the LDS with h3d, F > 65535.
 * ------------------------------------------------------------------------------------------ */
typedef struct {
    const afm_motion_guide* terms;         /* scale rows [G]; targets long-form; q / c [G * S]; gk (loops) [T][G * S]; frame_mask unread */
    afm_stitch stitch;
    int32_t frames;                        /* F */
} afm_long_guide;
int64_t afm_long_guidance_workspace_bytes(const afm_long_guide* g, int32_t B, int32_t L, int32_t D);
int afm_long_guidance(const afm_long_guide* g, const float* x_windows, const int64_t* t, float* grad_windows, float* energy_contact,
                      float* energy_targets, int32_t B, int32_t L, int32_t D, void* workspace, int64_t workspace_bytes, void* stream);

/* afm_stitch_step with a cond_fn gradient term, one launch: combine -> blend -> select -> clamp -> x0 += gk * grad -> update (the
 * afm_guide_step shift: m = gk[b] * grad rounded, then the addition rounded).  grad [B][L][D] and gk [B] are both required; x0_out
 * (optional, DDIM rows too; overrides args->x0_out) receives the shifted x0.  afm_stitch_step_args is unchanged. */
int afm_stitch_guide_step(const afm_stitch_step_args* args, const float* grad, const float* gk, float* x0_out, void* stream);

/* The stitched native loop guided by an afm_long_guide: afm_cmdm_guide_loop_range's signature with the long description in the guidance's
 * slot; the stitch is the description's own.  rows with eta = 0 (sigma NULL) or dpm only; cfg / cfg2 / known + mask as in the stitched
 * loop; sub-batches are cut over whole long motions.  Per sub-batch and executed step first_step + j that has reached a term's
 * first_guided, the launches of afm_long_guidance for the reached terms (t NULL) run on the sub-batch's stream in front of the
 * evaluations, and the stitched update takes grad and gk row n_steps - 1 - j (terms->gk [T][G * S]).  Earlier steps launch exactly what
 * afm_cmdm_stitch_loop_range launches.  Chained range calls on one workspace are bit-identical to one call. */
int64_t afm_cmdm_long_guide_loop_workspace_bytes(const afm_cmdm_weights* w, int32_t B, int32_t L, int32_t n_streams, const afm_cfg_args* cfg,
                                                 const afm_cfg2_args* cfg2, const afm_long_guide* guide);
int afm_cmdm_long_guide_loop_range(const afm_cmdm_weights* w, float* x, const float* cond_tokens, const uint8_t* frame_mask,
                                   const float* step_noise, const int64_t* d_timestep_map, const afm_ddim_rows* rows, const afm_dpm_rows* dpm,
                                   const float* d_c1, const float* d_c2, const float* d_sigma, const afm_cfg_args* cfg,
                                   const afm_cfg2_args* cfg2, const float* known, const uint8_t* mask, const afm_long_guide* guide,
                                   int32_t n_steps, int32_t first_step, uint64_t seed, int64_t sample_index0, int32_t B, int32_t L,
                                   void* sched_scratch, void* workspace, int64_t workspace_bytes, int32_t n_streams, void* const* side_streams,
                                   void* stream);

/* ------------------------------------------------------------------------------------------
 * Scene clearance of stitched long motions (v7-additive): afm_scene_clearance as a third term of the long guidance.  Each window clears
 * ITS OWN frames of the joined motion against ITS OWN scene: q [G * S][N][3], weight [G * S][N] or NULL and - with `exempt` - c
 * [G * S][N][Kc] are per window (the window "sit down" exempts the sofa its contact map marks, the window "walk" does not); scale is [G],
 * to_scene [3][4] or [G][3][4], t of long motion g is t[g * S], no frame mask is read.  With P[g,f,k,:] the positions of the joined motion
 * (afm_long_guide, steps 1 and 2), per window b = g * S + w and each of its long frames f = a_w .. min(a_w + L, F) - 1:
 *   d, d2, u, wu of p = P[g,f,k,:] against the points of window b exactly as afm_scene_clearance forms them (ir2, coef rounded once from
 *   float64, the w rules of min_height and exempt unchanged);  S_b[f,k,:] = sum_n wu * d,  e_b[f,k] = sum_n wu * u  in the order of the
 *   clearance kernel: wave v adds, from 0 and in ascending n, the points with (n mod 1024) / 128 == v, then the eight partial sums are
 *   joined serially, v = 0 .. 7.
 * Per long frame the windows' sums are crossfaded with the stitch's own weight row (wl, wr = afm_stitch.weights, [2][ov]): with
 * w1 = min(f / hop, S - 1), the earlier window w1 - 1 also holds f iff w1 > 0 and i = f - w1 * hop < ov;
 *   one window:   J[g,f,k,:] = S_b[f,k,:]                               (the bits as they are)
 *   two windows:  J[g,f,k,:] = (wl[i] * S_earlier) + (wr[i] * S_later)  float32, each product rounded, then the sum, no contraction
 * (a plain sum would push twice as hard inside every overlap of one room; identical clouds in both windows give the single-scene push up
 * to rounding; an exemption fades out as the next action fades in).
 *   column form:  grad_long[g,f,cols[k]+a] = ((scale[g] * coef[k]) * std_a) * J_a
 *   h3d form:     coef[k] * J_a, rounded, goes to S[g][f][k][3] and through the recovery's adjoint on (B = G, L = F) with scale[g]
 * With S == 1, F == L and no mask this is bit-identical to afm_scene_guidance's clearance on the one window.
 * The sum: grad_long = (grad_contact + grad_targets) + grad_clearance - the clearance's last launch (the join, or the adjoint) adds its
 * complete result to what the terms in front of it wrote, one rounded addition per element; then afm_stitch_windows.  Exact zeros: every
 * unnamed column, the padded tail, a long motion with t >= t_start, a joint-frame with no obstacle point inside its radius in any window
 * that holds it.
 * energy_clearance[g]: a joint-frame's e_b times its frame weight omega, rounded (omega = 1 outside overlaps - the value as it is -,
 * wl[i] / wr[i] in the earlier / later window of a shared frame); E_b = the clearance kernel's energy reduction over the window's L
 * frames - blocks of 64 / K whole frames, lane i adds its joint-frame's value over the blocks in ascending order, a frame at or behind F
 * counting 0, then one wave's butterfly; E[g] = the serial sum of its windows' E_b from 0 in window order.  The gradient is
 * -scale * dE/dx.  No atomics: a long motion's result depends neither on G nor on its place in the batch.
 * Launches of the clearance with a gradient: the long pass (blocks over (frame block of a window, window)) and the join (blocks over
 * (frame block of the long motion, long motion)) - 2; h3d: recovery over F frames, long pass, join, adjoint - 4.  afm_long_guidance's join
 * and windows launches are shared with the terms in front.
 *
 * base->terms is always set (it carries gk [T][G * S] for the loops) and may name neither term; then the clearance must be set.
 * AFM_E_BADARG before anything is enqueued: everything afm_long_guidance and afm_scene_guidance refuse (a radius that is not positive,
 * `up` outside 0..2, an exemption without c), terms and clearance that disagree on mean / std, form or to_scene, no term at all, weights
 * missing where two windows share frames.  AFM_E_UNSUPPORTED: F > 65535, more than 65535 windows, 7 * F floats beyond the LDS with h3d.
 * ------------------------------------------------------------------------------------------ */
typedef struct {
    const afm_long_guide* base;            /* stitch, frames, terms; base->terms is always set and may name neither term */
    const afm_scene_clearance* clearance;  /* q / weight / c per window [G * S]; scale [G]; first_guided / t_start as everywhere; or NULL */
} afm_long_scene_guide;
int64_t afm_long_scene_guidance_workspace_bytes(const afm_long_scene_guide* g, int32_t B, int32_t L, int32_t D);
int afm_long_scene_guidance(const afm_long_scene_guide* g, const float* x_windows, const int64_t* t, float* grad_windows,
                            float* energy_contact, float* energy_targets, float* energy_clearance, int32_t B, int32_t L, int32_t D,
                            void* workspace, int64_t workspace_bytes, void* stream);

/* afm_cmdm_long_guide_loop_range with the description swapped: the same loop body, the step's gradient the sum above over the terms whose
 * own first_guided the executed step has reached (a term not yet reached launches nothing and contributes exactly zero; steps before any
 * term starts launch exactly what afm_cmdm_stitch_loop_range launches).  gk: base->terms->gk [T][G * S]. */
int64_t afm_cmdm_long_scene_guide_loop_workspace_bytes(const afm_cmdm_weights* w, int32_t B, int32_t L, int32_t n_streams, const afm_cfg_args* cfg,
                                                       const afm_cfg2_args* cfg2, const afm_long_scene_guide* guide);
int afm_cmdm_long_scene_guide_loop_range(const afm_cmdm_weights* w, float* x, const float* cond_tokens, const uint8_t* frame_mask,
                                         const float* step_noise, const int64_t* d_timestep_map, const afm_ddim_rows* rows, const afm_dpm_rows* dpm,
                                         const float* d_c1, const float* d_c2, const float* d_sigma, const afm_cfg_args* cfg,
                                         const afm_cfg2_args* cfg2, const float* known, const uint8_t* mask, const afm_long_scene_guide* guide,
                                         int32_t n_steps, int32_t first_step, uint64_t seed, int64_t sample_index0, int32_t B, int32_t L,
                                         void* sched_scratch, void* workspace, int64_t workspace_bytes, int32_t n_streams, void* const* side_streams,
                                         void* stream);

/* ------------------------------------------------------------------------------------------
 * CDM (`Perceiver`) denoiser forward.  Replaces CDM.forward + ContactPerceiver.forward
 * (models/cdm.py:474-513,155-188) and the Perceiver-IO blocks it uses (models/modules.py:234-661:
 * CrossAttentionLayer, SelfAttentionBlock, MLP, Residual; pad mask / rotary / kv-cache never used).
 *
 * The encoder has only TWO latent queries (text, time), so its cross-attention over the N points is
 * evaluated without materialising K/V: q.(W_k x + b_k) = (W_k^T q).x + q.b_k and
 * sum_n a_n (W_v x_n + b_v) = W_v (sum_n a_n x_n) + b_v (fp re-association only); the decoder's
 * two-key attention folds the same way.  The dense per-point layers (decoder adapter, MLP) run on afm_linear.
 *
 * All weights are the reference's tensors (state-dict names in the comments, prefix `contact_model.`).
 */
typedef struct { const float* w; const float* b; } afm_lin;                 /* nn.Linear weight [out,in], bias [out] */
typedef struct { const float* g; const float* b; } afm_ln;                  /* nn.LayerNorm weight, bias             */
typedef struct { afm_lin q, k, v, o; } afm_mha_w;                          /* attention.{q,k,v,o}_proj               */
typedef struct { afm_ln norm; afm_lin fc1, fc2; } afm_mlp_w;               /* MLP: module.0 (LN), .1, .3              */
typedef struct {
    int32_t contact_dim;       /* input_feats (6)                                                  */
    int32_t feat_dim;          /* encoder_adapter in_features = contact_dim + point_feat_dim + 3   */
    int32_t dq, dkv;           /* encoder_q_input_channels (512), encoder_kv_input_channels (256)  */
    int32_t enc_heads, dec_heads, n_self;   /* 8, 8, encoder_self_attn_num_layers (2)              */
    int32_t text_dim, time_dim, n_timesteps;
    /* per-timestep tables of the TIME latent, built once per weight version with afm_cdm_latent_tokens(which = 1) on
     * the TimestepEmbedder output of every t (modules.py:38-53): enc_q0 row, folded queries, folded key-bias terms */
    const float* time_q0;      /* [n_timesteps, dq]                 */
    const float* time_u;       /* [n_timesteps, enc_heads, dkv]     */
    const float* time_cu;      /* [n_timesteps, enc_heads]          */
    afm_lin language_adapter, time_embedding_adapter, encoder_adapter, decoder_adapter;
    afm_ln enc_q_norm, enc_kv_norm; afm_mha_w enc_attn; afm_mlp_w enc_mlp;          /* encoder_cross_attn.{0,1}.module */
    afm_ln self_norm[4]; afm_mha_w self_attn[4]; afm_mlp_w self_mlp[4];             /* encoder_self_attn.{l}.{0,1}.module */
    afm_ln dec_q_norm, dec_kv_norm; afm_mha_w dec_attn; afm_mlp_w dec_mlp;          /* decoder_cross_attn.{0,1}.module */
    afm_lin contact_layer;     /* [contact_dim, dkv]                                               */
    int32_t gemm_arith, gemm_arith_min_n;   /* ABI v3: afm_linear_args.arith / arith_min_n of the dense per-point layers */
    /* ABI v4 (all five or none; the host builds them in eval mode when contact_dim <= 8 < ... and feat_dim > contact_dim): weight
     * products that let the sampling form skip everything that is linear in step-invariant data.  Only the contact_dim leading
     * columns of the encoder input (the noisy contact map x_t) change between the steps of a loop and no nonlinearity separates
     * encoder_adapter from decoder_adapter, nor linear2 (+ residual) from contact_layer (cdm.py:176-186,509-510):
     *   enc_kv[n] = C[n] + sum_j x_t[n,j] xu[j],  C = encoder_adapter(input with x = 0)      computed once per loop,
     *   dec_q0[n] = D[n] + sum_j x_t[n,j] xv[j],  D = decoder_adapter(C)                     computed once per loop,
     *   out[n]    = w2 . GELU(linear1 z[n]) + contact_layer.w . h1[n] + c0                   (linear2 and h1 never materialise;
     *               contact_layer.w . h1 = sum_jh a[n,jh] (contact_layer.w . P[jh]) + contact_layer.w . dec_q0[n] + const, the last
     *               again split into an invariant part E[n] and q . x_t[n]).
     * Same function as the layer-by-layer form up to f32 re-association (tests: 2e-4 abs against the reference goldens). */
    const float* fold_xu;      /* [contact_dim, dkv]  encoder_adapter.w[:, j]                                 */
    const float* fold_xv;      /* [contact_dim, dkv]  decoder_adapter.w @ encoder_adapter.w[:, j]             */
    const float* fold_w2;      /* [contact_dim, dkv]  contact_layer.w @ dec_mlp.fc2.w                         */
    int32_t flags;             /* AFM_CDM_* bits (ABI v4)                                                       */
    const float* fold_q;       /* [contact_dim, contact_dim]  contact_layer.w @ fold_xv^T                     */
    const float* fold_c0;      /* [contact_dim]  contact_layer.w @ (dec_mlp.fc2.b + dec_attn.o.b) + contact_layer.b */
    /* ABI v5 (all or none; built by the host next to fold_* when feat_dim + 1 <= 44): the sampling form without per-point rows.  A point is
     * x = [x_t | point features, xyz | 1 | 0 ...], K numbers: K = 12 when feat_dim + 1 <= 12 (the H3D variant's 9 input channels), else K = 44 (the
     * HUMANISE variant's 41), NT = ceil(K / 16).  Everything between the nonlinearities is linear in x and in the 16 attention weights a[jh] of the
     * decoder:
     *   encoder side   the rows the two latents attend over are LayerNorm_kv(x G_enc): var = x Qe x^T, any dot with a vector u is rstd (x . (Ec u)),
     *                  the attention-weighted row sum is linear in sum_n a_n rstd_n x_n (enc_point_kernel accumulates 16 x K numbers per wave):
     *     enc_ec  [K, dkv]   G_enc = [encoder_adapter.w^T ; encoder_adapter.b ; 0] minus its row means
     *     enc_qee [K, 16 NT] enc_ec enc_ec^T / dkv in MFMA operand order: entry (k, 16 t + i) = Q[4 (4 t + (i & 3)) + (i >> 2)][k], 0 where that index is >= K
     *     enc_wove [8 K, dq], enc_c1 [dq]   head of the latent chain: x1 = q0 + o_proj(v_proj(.)) as one product with the 8 x K accumulated numbers
     *                  (row K h + k = o_proj.w[:, head h] v_proj.w[head h] (enc_kv_norm.w * enc_ec[k]); enc_c1 = o_proj.b + o_proj.w (v_proj.w enc_kv_norm.b + v_proj.b))
     *   decoder side   with G_dec = [(decoder_adapter.w encoder_adapter.w)^T ; decoder_adapter.w encoder_adapter.b + decoder_adapter.b ; 0]:
     *                  scores = rstd_q (x . EG) + const, var_q = x Qd x^T;  h1 = [a | x] T with T = [P ; G_dec + dec_attn.o.b on the constant's row];
     *                  LayerNorm_mlp(h1) W1^T = rstd ([a | x] TWc) + C, var = [a | x] Qc [a | x]^T: linear1 is a K + 16 product.  Step-invariant parts:
     *     dec_qdd [K, 16 NT] (G_dec - row means)(...)^T / dkv in operand order (as enc_qee)    dec_c   [dkv]      dec_mlp.fc1.b + dec_mlp.fc1.w dec_mlp.norm.b
     *     dec_twx [K, dkv]   Xc (dec_mlp.fc1.w * dec_mlp.norm.w)^T, Xc = centred input rows of T     dec_qxx [K, K]     Xc Xc^T / dkv
     *     gen_qe  [contact_dim, K]  contact_layer.w G_dec^T
     *                  and the parts that depend on the sample's latents come from their decoder keys / values (o = 32 h + r over a head's entries,
     *                  Woc = dec_attn.o.w minus its column means) through
     *     dec_dwq [K, dkv]  = ((G_dec - row means) * dec_q_norm.w) dec_attn.q.w^T      dec_wqb [dkv] = dec_attn.q.w dec_q_norm.b + dec_attn.q.b
     *     dec_wco [8, dkv]  = contact_layer.w dec_attn.o.w (zero rows >= contact_dim)   dec_wow [dkv, dkv] = Woc^T (dec_mlp.fc1.w * dec_mlp.norm.w)^T
     *     dec_wog [dkv, dkv] = Woc^T Woc / dkv                                          dec_xwo [K, dkv] = Xc Woc / dkv */
    const float* gen_qe;
    const float* dec_c; const float* dec_twx; const float* dec_qxx; const float* dec_qdd;
    const float* enc_ec; const float* enc_qee; const float* enc_wove; const float* enc_c1;
    const float* dec_dwq; const float* dec_wqb; const float* dec_wco; const float* dec_wow; const float* dec_wog; const float* dec_xwo;
    /* optional (any sampling form): LayerNorm folded into the six kinds of latent-chain stages that follow one.  lat_fold[3 s + 0 / 1 / 2] =
     * (W * gamma [N, K], g[n] = sum_k (W * gamma)[n, k], b + W beta) for slot s: 0 enc_mlp.fc1; 1 + 4 l .. 3 + 4 l the q / k / v projections of
     * self-attention layer l (self_norm[l]); 4 + 4 l self_mlp[l].fc1; 17 / 18 dec_attn.k / dec_attn.v (dec_kv_norm).  The stage then computes
     * rstd (W' x - mean g) + c on the RAW rows: its matrix products do not wait for the statistics. */
    const float* const* lat_fold;
} afm_cdm_weights;

#define AFM_CDM_TILE_SHIFT     8       /* bits 8..11, measurement: AFM_TUNE_TILE code forced on the linear1 GEMM of the sampling forms (bit-neutral) */
#define AFM_CDM_CHAIN_SIDE     0x4     /* row-less form with sub-batch streams: the 2-latent chain (lat_head .. lat_dectables) of a sub-batch runs on its SIDE stream (fork / join by events), so that it can sit on CUs of its own (a CU-masked stream) under the other sub-batch's point kernels; bit-identical */
#define AFM_CDM_PIPELINE       0x10    /* ABI v7, row-less form with n_sub > 1: the point kernels (enc_point, dec_point) of ALL sub-batches in round-robin order on streams[0], the 2-latent chain of sub-batch s on streams[2 s + 1] between two events - one sub-batch's launch-latency-bound chain always runs under the other sub-batches' point kernels; bit-identical */
#define AFM_CDM_DEC_CHUNKS_SHIFT 12    /* bits 12..17: workgroups per sample of enc_point's successor dec_point_kernel (0 = 16); a tuning knob, bit-identical (a point's arithmetic does not depend on its chunk) */
#define AFM_CDM_CLIP_X0        0x8     /* clip_denoised=True: pred_xstart clamped to [-1, 1] inside the fused DDPM update of every sampling form */
#define AFM_CDM_NO_GEN         0x2     /* measurement: round 2's folded form (step-invariant adapter parts materialised, per-point rows) although the row-less tables are present */

int64_t afm_cdm_workspace_bytes(const afm_cdm_weights* w, int32_t B, int32_t N);

/* One denoiser evaluation (+ optional fused DDPM update, same afm_ddpm_args as the CMDM).
 *   feat [B,N,feat_dim] = cat(x_t, (point features), xyz) as cdm.py:167-171 builds it; x_t itself is feat[..., :contact_dim]
 *   (needed separately, contiguous [B,N,contact_dim], only for the DDPM update); t [B] int64;
 *   text_q0 / text_u / text_cu: the TEXT latent of every sample from afm_cdm_latent_tokens(which = 0) on text_feat [B,text_dim];
 *   x0_out [B,N,contact_dim] (may be NULL when ddpm != NULL). */
int afm_cdm_forward(const afm_cdm_weights* w, const float* feat, const float* x_t, const int64_t* t,
                    const float* text_q0, const float* text_u, const float* text_cu, float* x0_out,
                    const afm_ddpm_args* ddpm, int32_t B, int32_t N, void* workspace, int64_t workspace_bytes, void* stream);
/* Same, with the decoder-adapter GEMM enqueued on `side_stream` underneath the per-sample latent chain (fork / join by events on
 * `stream`; results identical).  side_stream == NULL behaves like afm_cdm_forward. */
int afm_cdm_forward_overlap(const afm_cdm_weights* w, const float* feat, const float* x_t, const int64_t* t,
                    const float* text_q0, const float* text_u, const float* text_cu, float* x0_out,
                    const afm_ddpm_args* ddpm, int32_t B, int32_t N, void* workspace, int64_t workspace_bytes, void* side_stream, void* stream);

/* Whole ADM p_sample_loop (gaussian_diffusion.py:442-536 with the CDM Perceiver denoiser) enqueued natively, no host synchronisation:
 *   x [B,N,contact_dim]: x_T on entry, the sample on exit.  feat [B,N,feat_dim]: the encoder input; its step-invariant columns
 *   (per-point features, xyz) are filled by the caller, the leading contact_dim columns are rewritten from x every step.
 *   text_q0 / text_u / text_cu: afm_cdm_latent_tokens of the text features.  step_noise [n_steps,B,N,contact_dim] or NULL (Philox
 *   keyed by (seed, sample_index0 + b, step)).  Schedule rows / sched_scratch as for afm_cmdm_sample_loop
 *   (afm_cmdm_sched_scratch_bytes).  Sub-batching: n_sub > 1 splits the batch; sub-batch s runs on streams[2s] and uses streams[2s+1]
 *   as the side stream of its decoder-adapter GEMM (one half's per-sample latent chain overlaps the other half's GEMMs);
 *   n_sub <= 1: everything on `stream`, streams[0] (if given) = side stream.  workspace >= afm_cdm_loop_workspace_bytes. */
int64_t afm_cdm_loop_workspace_bytes(const afm_cdm_weights* w, int32_t B, int32_t N, int32_t n_sub);
int afm_cdm_sample_loop(const afm_cdm_weights* w, float* x, float* feat, const float* text_q0, const float* text_u,
                        const float* text_cu, const float* step_noise, const int64_t* d_timestep_map, const float* d_c1,
                        const float* d_c2, const float* d_sigma, int32_t n_steps, uint64_t seed, int64_t sample_index0,
                        int32_t B, int32_t N, void* sched_scratch, void* workspace, int64_t workspace_bytes, int32_t n_sub,
                        void* const* streams, void* stream);
/* Slice of the loop, as afm_cmdm_sample_loop_range. */
int afm_cdm_sample_loop_range(const afm_cdm_weights* w, float* x, float* feat, const float* text_q0, const float* text_u,
                              const float* text_cu, const float* step_noise, const int64_t* d_timestep_map, const float* d_c1,
                              const float* d_c2, const float* d_sigma, int32_t n_steps, int32_t first_step, uint64_t seed,
                              int64_t sample_index0, int32_t B, int32_t N, void* sched_scratch, void* workspace,
                              int64_t workspace_bytes, int32_t n_sub, void* const* streams, void* stream);
/* DDIM form of the loop slice (v7-additive), as afm_cmdm_ddim_loop_range: the DDIM update is fused into the last kernel of the row-less
 * (dec_point) and folded-rows (output kernel) forms; the layer-by-layer form adds one elementwise launch behind its contact_layer GEMM.
 * sched_scratch >= afm_ddim_sched_scratch_bytes(n_steps, B). */
int afm_cdm_ddim_loop_range(const afm_cdm_weights* w, float* x, float* feat, const float* text_q0, const float* text_u,
                            const float* text_cu, const float* step_noise, const int64_t* d_timestep_map, const afm_ddim_rows* rows,
                            int32_t n_steps, int32_t first_step, uint64_t seed,
                            int64_t sample_index0, int32_t B, int32_t N, void* sched_scratch, void* workspace,
                            int64_t workspace_bytes, int32_t n_sub, void* const* streams, void* stream);
/* The imputing loop slice (v7-additive), DDPM and DDIM behind one entry, as afm_cmdm_impute_loop_range: the arguments of the two entries
 * above with both kinds of rows (rows != NULL: the DDIM loop, d_c1 / d_c2 / d_sigma ignored; rows == NULL: the DDPM loop) and known / mask
 * [B][N][contact_dim] (the imputation rule above: a select on pred_xstart in front of the clamp; mask uint8, nonzero = known).  known
 * without mask or the reverse: AFM_E_BADARG, in front of every other check; both NULL: the loop without imputation.
 * Row-less form (the default): the select is fused into dec_point in front of its update - no extra launch, no stored pred_xstart - and
 * the DDPM update is the afm_ddpm_step expression, every operation rounded on its own: the loop is bit-identical to afm_cdm_forward ->
 * afm_impute -> (afm_clamp ->) afm_ddpm_step / afm_ddim_step per step.  Folded-rows and layer-by-layer forms: pred_xstart stored with the
 * plain output, then ONE update launch per sub-batch (the afm_impute_step expression, in place on x), for DDPM too.  Workspace, schedule
 * scratch (afm_ddim_sched_scratch_bytes with rows, afm_cmdm_sched_scratch_bytes without), noise, sub-batches and first_step as above. */
int afm_cdm_impute_loop_range(const afm_cdm_weights* w, float* x, float* feat, const float* text_q0, const float* text_u,
                              const float* text_cu, const float* step_noise, const int64_t* d_timestep_map, const afm_ddim_rows* rows,
                              const float* d_c1, const float* d_c2, const float* d_sigma, const float* known, const uint8_t* mask,
                              int32_t n_steps, int32_t first_step, uint64_t seed, int64_t sample_index0, int32_t B, int32_t N,
                              void* sched_scratch, void* workspace, int64_t workspace_bytes, int32_t n_sub, void* const* streams,
                              void* stream);
/* The DPM-Solver++(2M) loop slice (v7-additive), as afm_cmdm_dpm_loop_range: the arguments of afm_cdm_ddim_loop_range with the 2M rows in
 * place of the DDIM rows, no step noise and no seed (the sampler has no noise term), and known / mask [B][N][contact_dim] optional (both or
 * neither; the imputation rule above).  The update is the afm_dpm_step expression on the final pred_xstart - after the select and the
 * clamp - which is also kept as the next step's x0_prev in a history buffer [count][N * contact_dim] per sub-batch, carved behind the
 * sub-batch's workspace for this loop alone (afm_cdm_dpm_loop_workspace_bytes; afm_cdm_loop_workspace_bytes stays what it was).
 * Row-less form (the default): update, select and history ride in dec_point - the launches of the eta = 0 DDIM loop, bit-identical to
 * afm_cdm_forward -> (afm_impute ->) (afm_clamp ->) afm_dpm_step per step.  Folded-rows and layer-by-layer forms: pred_xstart stored where
 * their imputing loops store it, then ONE update launch per sub-batch and step.  first_step == 0: executed step 0 has no history (the
 * two-term form); first_step > 0: the history is what the previous range call left in the SAME workspace (same B, N, n_sub) - chained
 * range calls are bit-identical to one call.  AFM_E_BADARG: NULL rows (or a NULL row), first_step < 0, known without mask or the
 * reverse; AFM_E_WORKSPACE: workspace < afm_cdm_dpm_loop_workspace_bytes.  sched_scratch >= afm_ddim_sched_scratch_bytes(n_steps, B). */
int64_t afm_cdm_dpm_loop_workspace_bytes(const afm_cdm_weights* w, int32_t B, int32_t N, int32_t n_sub);
int afm_cdm_dpm_loop_range(const afm_cdm_weights* w, float* x, float* feat, const float* text_q0, const float* text_u,
                           const float* text_cu, const int64_t* d_timestep_map, const afm_dpm_rows* rows, const float* known,
                           const uint8_t* mask, int32_t n_steps, int32_t first_step, int32_t B, int32_t N, void* sched_scratch,
                           void* workspace, int64_t workspace_bytes, int32_t n_sub, void* const* streams, void* stream);

/* Latent-token precomputation (step-invariant, off the per-step path): for n input rows `in` [n, text_dim] (which = 0,
 * language_adapter) or [n, time_dim] (which = 1, time_embedding_adapter) compute the latent's enc_q0 row
 * q0_out [n, dq], q = dp_scale * q_proj(LN_q(q0)) folded through k_proj: u_out [n, enc_heads, dkv], cu_out [n, enc_heads]. */
int afm_cdm_latent_tokens(const afm_cdm_weights* w, int32_t which, const float* in, int32_t n,
                          float* q0_out, float* u_out, float* cu_out, void* stream);

/* ------------------------------------------------------------------------------------------
 * Opt-in profiler (measurement only, no reference counterpart): when enabled, every kernel launch of
 * this library is bracketed by HIP events on its own stream.  afm_profile_read synchronises, returns
 * per-kernel totals since the last read (work = algorithmic FLOPs, or bytes for streaming kernels) and
 * clears them.  Returns the number of entries written, or a negative AFM_E_* code. */
typedef struct {
    const char* name;       /* kernel name as it appears in rocprofv3 kernel traces (template args abbreviated) */
    int64_t launches;
    double total_ms;
    double total_work;
} afm_profile_entry;
int afm_profile_enable(int32_t on);
int afm_profile_read(afm_profile_entry* out, int32_t max_entries);

#ifdef __cplusplus
}
#endif
#endif /* AFM_HIP_H */
