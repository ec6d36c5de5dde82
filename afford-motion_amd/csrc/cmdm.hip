// CMDM (`trans_enc`) denoiser step and the native p_sample_loop driver.
//
// Token layout per sample (reference cmdm.py:161): [time | n_cond step-invariant tokens | L motion].
// Per step only the time token and the L motion tokens change, so the host pre-computes the
// n_cond condition tokens (text + contact groups, adapters and positional encoding applied) once
// per sampling run; the time token is a table lookup (TimestepEmbedder depends on t only).
//
// Launch sequence per step (all on one stream, no host sync):
//   prologue (time token + cond copy + key mask) -> motion_adapter GEMM (scatter into the token
//   buffer, +bias +positional rows) -> n_layers x { in_proj GEMM, flash MHA, out_proj GEMM(+bias
//   +residual), LN, FFN1 GEMM(+bias+GELU), FFN2 GEMM(+bias+residual), LN } -> motion_layer GEMM
//   (gather motion tokens, +bias, fused DDPM posterior update).
// Classifier-free guided steps (afm_cmdm_cfg_*, afm_cmdm_cfg2_*): this sequence for the conditioned evaluation, then once per branch of the
// list struct Guidance holds ([middle,] unconditioned), every motion_layer GEMM storing pred_xstart, then one launch that combines them.
#include <memory>

#include "sample_loop.h"

using namespace afm_loop;

extern "C" int afm_linear(const afm_linear_args*, void*);
extern "C" int afm_linear_pair(const afm_linear_args*, const afm_linear_args*, void*);
extern "C" int afm_mha_fwd_grouped(const float*, const uint8_t*, float*, int32_t, int32_t, int32_t, int32_t, int32_t, void*);
extern "C" int afm_mha_fwd_rows(const float*, const uint8_t*, float*, int32_t, int32_t, int32_t, int32_t, int32_t, int32_t, void*);
extern "C" int afm_mha_fwd_arith(const float*, const uint8_t*, float*, int32_t, int32_t, int32_t, int32_t, int32_t, int32_t, int32_t, void*);
extern "C" int afm_layernorm(const float*, const float*, const float*, float*, int64_t, int32_t, float, void*);
extern "C" int afm_layernorm_rows(const float*, const float*, const float*, float*, int64_t, int32_t, float, int32_t, int32_t, int32_t, void*);
extern "C" int afm_randn(float*, int32_t, int64_t, uint64_t, int64_t, int32_t, void*);

namespace {

struct Workspace {
    float *seq0, *y, *x1, *tmp, *qkv, *qkv0, *att, *hid, *noise, *xpad;
    float* x0;                // loop workspaces only: pred_xstart [B][L][motion_dim] of the DDIM loop's step (its update launch reads it)
    uint8_t* keymask;
    uint32_t* lncnt;          // tickets of the fused LayerNorm (one word per 32 output rows; zero between launches)
    float *stat1, *stat2;     // folded LayerNorm: (mean, M2) per row and 64-column group of the raw out_proj / linear2 outputs
    int64_t bytes;
};

Workspace carve(const afm_cmdm_weights& w, int B, int L, void* base, int noise_steps = 1) {
    const int64_t T = 1 + w.n_cond + L, M = (int64_t)B * T, d = w.d;
    char* p = (char*)base;
    int64_t off = 0;
    auto take = [&](int64_t nbytes) { char* r = p ? p + off : nullptr; off += align256(nbytes); return r; };
    Workspace ws;
    ws.seq0 = (float*)take(M * d * 4);
    ws.y = (float*)take(M * d * 4);
    ws.x1 = (float*)take(M * d * 4);
    ws.tmp = (float*)take(M * d * 4);
    ws.qkv = (float*)take(M * 3 * d * 4);
    ws.qkv0 = (float*)take(M * 3 * d * 4);            // layer 0's in_proj output: its condition-token rows persist across the steps of a loop
    ws.att = (float*)take(M * d * 4);
    ws.hid = (float*)take(M * (int64_t)w.ff * 4);
    ws.noise = (float*)take((int64_t)noise_steps * B * L * w.motion_dim * 4);      // the native loop draws the Philox noise of NOISE_STEPS steps per launch (single-step forward: 1)
    ws.keymask = (uint8_t*)take(M);
    ws.lncnt = (uint32_t*)take(((M + 31) / 32) * 4);
    ws.stat1 = (float*)take(M * (d / 64 + 1) * 2 * 4); ws.stat2 = (float*)take(M * (d / 64 + 1) * 2 * 4);
    ws.xpad = w.motion_adapter_kpad > 0 ? (float*)take((int64_t)B * L * w.motion_adapter_kpad * 4) : nullptr;      // x_t with rows padded to the GEMM's K
    // behind every other region, so the single-step layout is unchanged
    ws.x0 = noise_steps > 1 ? (float*)take((int64_t)B * L * w.motion_dim * 4) : nullptr;
    ws.bytes = off;
    return ws;
}

// grid (B, 1 + n_cond): token 0 = time_table[t] + pos[0]; tokens 1..n_cond = cond copy; also key mask.  With xpad != NULL the
// blocks of a sample also copy its x_t rows into rows of kpad floats (zero padded): the motion adapter's K = 263 is not a multiple
// of 16, its padded copy is (the A operand of the bf16-split GEMM needs 16-byte rows and whole K16 steps).
__global__ __launch_bounds__(128) void prologue_kernel(float* __restrict__ seq0, const float* __restrict__ time_table,
                                                       const float* __restrict__ pos_table, const int64_t* __restrict__ t,
                                                       const float* __restrict__ cond, const uint8_t* __restrict__ frame_mask,
                                                       uint8_t* __restrict__ keymask, int T, int L, int n_cond, int d,
                                                       int n_timesteps, int copy_cond, const float* __restrict__ x_t,
                                                       float* __restrict__ xpad, int md, int kpad) {
    const int b = blockIdx.x, tok = blockIdx.y;
    if (xpad) {
        for (int l = tok; l < L; l += gridDim.y) {
            const float* src = x_t + ((int64_t)b * L + l) * md;
            float* dstp = xpad + ((int64_t)b * L + l) * kpad;
            for (int c = threadIdx.x; c < kpad; c += blockDim.x) dstp[c] = c < md ? src[c] : 0.0f;
        }
    }
    float* dst = seq0 + ((int64_t)b * T + tok) * d;
    if (tok == 0) {
        int64_t ti = t[b];
        ti = ti < 0 ? 0 : (ti >= n_timesteps ? n_timesteps - 1 : ti);
        const float* src = time_table + ti * d;
        for (int c = threadIdx.x * 4; c < d; c += blockDim.x * 4) {
            const float4 a = *reinterpret_cast<const float4*>(src + c);
            const float4 p = *reinterpret_cast<const float4*>(pos_table + c);
            *reinterpret_cast<float4*>(dst + c) = make_float4(a.x + p.x, a.y + p.y, a.z + p.z, a.w + p.w);
        }
        if (keymask)
            for (int i = threadIdx.x; i < T; i += blockDim.x)
                keymask[(int64_t)b * T + i] = (i < 1 + n_cond) ? 0 : frame_mask[(int64_t)b * L + (i - 1 - n_cond)];
    } else if (copy_cond) {
        const float* src = cond + ((int64_t)b * n_cond + (tok - 1)) * d;
        for (int c = threadIdx.x * 4; c < d; c += blockDim.x * 4)
            *reinterpret_cast<float4*>(dst + c) = *reinterpret_cast<const float4*>(src + c);
    }
}

// The unconditioned branch of a guided evaluation (classifier-free guidance).  Compact form: the weight pack's copy has n_cond = 0 (no
// condition rows exist) and the motion tokens keep the positional rows of the full layout, pos_off = 1 + n_cond of the real pack.  Masked
// form: the full layout, with the key mask also set on the dropped condition tokens (token 1 = text, tokens 2 .. n_cond = contact groups).
struct Branch { int pos_off, mask_text, mask_pc; };

// grid (B): the condition tokens' entries of the key mask the prologue has just written (0 there): 1 on the dropped ones
__global__ __launch_bounds__(64) void cond_keymask_kernel(uint8_t* __restrict__ keymask, int T, int n_cond, int mask_text, int mask_pc) {
    for (int i = threadIdx.x; i < n_cond; i += blockDim.x)
        keymask[(int64_t)blockIdx.x * T + 1 + i] = (uint8_t)(i == 0 ? mask_text : mask_pc);
}

#define AFM_TRY(expr) do { int rc__ = (expr); if (rc__ != 0) return rc__; } while (0)

// ---- the launches of one step as DATA (round 6, AFM_CMDM_PAIR_LAUNCH): with a Recorder, forward_impl does not launch - it lists the step's
// launches in order, tagged, and the paired schedule (issue_paired below) interleaves the lists of the two sub-batches on their streams and
// fuses sub-batch A's out_proj with sub-batch B's linear1 into ONE afm_linear_pair launch per layer.
enum { OP_LINEAR = 0, OP_MHA = 1 };
enum { TAG_NONE = 0, TAG_OUT_PROJ = 1, TAG_LINEAR1 = 2 };
struct Op {
    int kind, tag;
    afm_linear_args a;
    const float* qkv; const uint8_t* keymask; float* out; int B, T, H, dh, q_first, group_waves, arith;
};
struct Recorder { Op ops[8 * AFM_MAX_LAYERS + 8]; int n = 0; };

inline int launch_op(const Op& o, hipStream_t s) {
    if (o.kind == OP_LINEAR) return afm_linear(&o.a, s);
    return afm_mha_fwd_arith(o.qkv, o.keymask, o.out, o.B, o.T, o.H, o.dh, o.q_first, o.group_waves, o.arith, s);
}

// every nn.Linear of the denoiser runs with the arithmetic the caller put into the weight pack (ABI v3: no process-wide switch)
inline int run_linear(const afm_cmdm_weights& w, afm_linear_args& a, hipStream_t s, Recorder* rec = nullptr, int tag = TAG_NONE) {
    a.arith = w.gemm_arith; a.arith_min_n = w.gemm_arith_min_n;
    const int tile = (w.flags >> AFM_CMDM_WIDE_TILE_SHIFT) & 0xF;          // measurement knob (tile shapes of one arithmetic are bit-identical)
    if (tile && a.N >= 512 && a.M >= 2048) a.tune = tile << AFM_TUNE_TILE_SHIFT;
    if (rec) {
        if (rec->n >= (int)(sizeof(rec->ops) / sizeof(rec->ops[0]))) return AFM_E_UNSUPPORTED;
        Op& o = rec->ops[rec->n++];
        o = Op{};
        o.kind = OP_LINEAR; o.tag = tag; o.a = a;
        return 0;
    }
    return afm_linear(&a, s);
}

inline int run_mha(const afm_cmdm_weights& w, const float* qkv, const uint8_t* keymask, float* out, int B, int T, int q_first, hipStream_t s, Recorder* rec) {
    if (rec) {
        if (rec->n >= (int)(sizeof(rec->ops) / sizeof(rec->ops[0]))) return AFM_E_UNSUPPORTED;
        Op& o = rec->ops[rec->n++];
        o = Op{};
        o.kind = OP_MHA; o.qkv = qkv; o.keymask = keymask; o.out = out; o.B = B; o.T = T; o.H = w.heads; o.dh = w.d / w.heads; o.q_first = q_first;
        o.group_waves = w.attn_group_waves; o.arith = w.gemm_arith;
        return 0;
    }
    return afm_mha_fwd_arith(qkv, keymask, out, B, T, w.heads, w.d / w.heads, q_first, w.attn_group_waves, w.gemm_arith, s);
}

int forward_impl(const afm_cmdm_weights& w, const float* x_t, const int64_t* t, const float* cond,
                 const uint8_t* frame_mask, float* x0_out, const afm_ddpm_args* ddpm, int B, int L, const Workspace& ws,
                 bool copy_cond, hipStream_t s, Recorder* rec = nullptr, const Branch* br = nullptr) {
    const int d = w.d, T = 1 + w.n_cond + L;
    const int M = B * T;
    uint8_t* keymask = frame_mask ? ws.keymask : nullptr;
    const int pos_off = br ? br->pos_off : 1 + w.n_cond;          // positional row of the first motion token
    const bool mask_cond = br && (br->mask_text || br->mask_pc);
    if (mask_cond && (!keymask || w.n_cond < 1 || rec)) return AFM_E_BADARG;
    if (w.n_cond == 0) cond = nullptr;               // (a compact branch runs on the caller's arguments: no condition rows, none read)

    // Steps after the first of a native loop need no prologue launch: the condition tokens and the key mask persist in the workspace, the
    // K-padded copy of x_t was written by the previous step's DDPM update (ddpm_out2), and the time tokens ride on the motion adapter's
    // launch (aux_*) - one launch less per step (~8 us of a 430 us step at one sample per GPU).
    const bool riders = !copy_cond && ddpm && ws.xpad && !(w.flags & AFM_CMDM_NO_RIDERS) && w.gemm_arith != AFM_ARITH_F32 &&
                        (w.gemm_arith == AFM_ARITH_DEFAULT || w.gemm_arith_min_n <= d) && B <= ((B * L + 127) / 128) * ((d + 127) / 128);
    if (rec && !riders) return AFM_E_UNSUPPORTED;       // (a recorded step has no prologue launch: the caller records riders-steps only)
    if (!riders) {
        hipLaunchKernelGGL(prologue_kernel, dim3(B, 1 + w.n_cond), dim3(128), 0, s, ws.seq0, w.time_table, w.pos_table, t, cond,
                           frame_mask, keymask, T, L, w.n_cond, d, w.n_timesteps, copy_cond ? 1 : 0, x_t, ws.xpad, w.motion_dim, w.motion_adapter_kpad);
        AFM_CHECK_LAUNCH();
        if (mask_cond) {                              // (with the riders the mask of the loop's first step persists in the workspace)
            hipLaunchKernelGGL(cond_keymask_kernel, dim3(B), dim3(64), 0, s, keymask, T, w.n_cond, br->mask_text, br->mask_pc);
            AFM_CHECK_LAUNCH();
        }
    }

    {   // motion_adapter (cmdm.py:159) scattered to token rows 1+n_cond.., + positional encoding (cmdm.py:162)
        afm_linear_args a = {};
        const int kp = w.motion_adapter_kpad;           // > 0: motion_adapter_w is [d, kp] (zero-padded columns) and the A rows are ws.xpad
        a.A = kp ? ws.xpad : x_t; a.lda = kp ? kp : w.motion_dim; a.W = w.motion_adapter_w; a.ldw = a.lda;
        a.C = ws.seq0; a.ldc = d; a.M = B * L; a.N = d; a.K = (int)a.lda;
        a.bias = w.motion_adapter_b;
        a.rowtab = w.pos_table + (int64_t)pos_off * d; a.rowtab_period = L;
        a.c_grp = L; a.c_stride = T; a.c_off = 1 + w.n_cond;
        if (riders) {       // time token of every sample: seq0[b T] = time_table[t_b] + pos[0]
            a.aux_src = w.time_table; a.aux_idx = t; a.aux_idx_max = w.n_timesteps; a.aux_add = w.pos_table; a.aux_dst = ws.seq0;
            a.aux_dst_ld = (int64_t)T * d; a.aux_rows = B; a.aux_cols = d;
        }
        AFM_TRY(run_linear(w, a, s, rec));
    }

    // LayerNorm folded across the kernel boundaries (round 3): with the folded tensors in the pack (eval mode) and every GEMM of the layer on
    // the bf16-split kernels, norm1 / norm2 are never launched and their outputs never exist: out_proj / linear2 store the RAW residual
    // sums plus (mean, M2) per row and 64-column group, linear1 / the next in_proj / motion_layer run on the raw rows with gamma folded
    // into their weights and apply (mean, rstd) in the epilogue, the residual adds normalise their (raw) input on the fly
    // (afm_linear_args.stat_out / a_stat / res_stat).  10 launches and ~170 MB of traffic less per step at B = 32.
    // Every folded GEMM must run on the bf16-split kernels (the native ones do not carry the row statistics): K = d or ff >= 128 and a
    // multiple of 16, N >= the arithmetic's minimum width for all five shapes (N = 3d, d, ff, d, motion_dim) - otherwise the layers fall
    // back to the separate LayerNorm launches instead of failing with AFM_E_UNSUPPORTED.
    const int split_min_n = w.gemm_arith == AFM_ARITH_DEFAULT ? 32 : w.gemm_arith_min_n;
    bool fold = !(w.flags & (AFM_CMDM_NO_LN_FOLD | AFM_CMDM_FUSED_LN)) && w.motion_layer_wg && w.motion_layer_g && w.motion_layer_c && (d % 64) == 0 &&
                w.gemm_arith != AFM_ARITH_F32 && d >= 128 && w.ff >= 128 && (w.ff % 16) == 0 && d >= split_min_n && w.ff >= split_min_n &&
                w.motion_dim >= split_min_n;
    for (int li = 0; li < w.n_layers && fold; ++li)
        fold = w.layer[li].lin1_wg && w.layer[li].lin1_g && w.layer[li].lin1_c && (li == 0 || (w.layer[li].in_proj_wg && w.layer[li].in_proj_g && w.layer[li].in_proj_c));
    const int sg = d / 64;                            // statistic groups per row
    const float* X = ws.seq0;
    for (int li = 0; li < w.n_layers; ++li) {
        const afm_encoder_layer_weights& lw = w.layer[li];
        // Layer 0 reads the token buffer itself, whose condition rows (text + contact groups) do not change between the steps of a
        // sampling loop: their q | k | v rows are computed on the loop's first step only (copy_cond) and kept in qkv0; afterwards the
        // in_proj runs on the time-token rows and the motion rows (a GEMM row depends on its own input row only: bit-identical).
        float* qkv = li == 0 ? ws.qkv0 : ws.qkv;
        afm_linear_args a = {};
        a.A = X; a.lda = d; a.W = lw.in_proj_w; a.ldw = d; a.C = qkv; a.ldc = 3 * d;
        a.N = 3 * d; a.K = d; a.bias = lw.in_proj_b;
        if (fold && li > 0) {                         // X = the previous layer's raw linear2 output: its norm2 is folded into W / bias
            a.W = lw.in_proj_wg; a.bias = lw.in_proj_c; a.a_stat = ws.stat2; a.a_stat_groups = sg; a.a_fold_g = lw.in_proj_g; a.ln_eps2 = 1e-5f;
        }
        const bool no_l0_cache = (w.flags & AFM_CMDM_NO_L0_CACHE) != 0;                  // measurement knob
        if (li == 0 && !copy_cond && w.n_cond > 0 && !no_l0_cache) {
            // ONE launch over the time token and the L motion tokens of every sample: groups of 1 + L rows with a hole of n_cond rows
            // behind the first (afm_linear_args.a_skip; round 3 ran two launches - a launch is ~17 us of a small-batch step)
            a.M = B * (1 + L);
            a.a_grp = 1 + L; a.a_stride = T; a.a_off = 0; a.a_skip_after = 1; a.a_skip = w.n_cond;
            a.c_grp = 1 + L; a.c_stride = T; a.c_off = 0; a.c_skip_after = 1; a.c_skip = w.n_cond;
            AFM_TRY(run_linear(w, a, s, rec));
        } else {
            a.M = M;
            AFM_TRY(run_linear(w, a, s, rec));
        }
        // After the LAST layer only the L motion tokens of each sample are read (motion_layer, cmdm.py:169,195), and
        // everything after the attention's key / value side is row-local: the attention computes the motion tokens' QUERY rows only
        // (7 query blocks instead of 11 at T = 326) and the stages behind it run on the B*L motion rows only (token rows gathered /
        // scattered by the row maps; the other rows of att/tmp/x1/y keep stale values nobody reads).
        const bool last = (li == w.n_layers - 1);
        if (last && w.n_cond > 0 && !(w.flags & AFM_CMDM_ALL_QUERIES))
            AFM_TRY(run_mha(w, qkv, keymask, ws.att, B, T, 1 + w.n_cond, s, rec));
        else
            AFM_TRY(run_mha(w, qkv, keymask, ws.att, B, T, 0, s, rec));
        const int rows = last ? B * L : M;
        const int g = last ? L : 0, gs = last ? T : 0, go = last ? 1 + w.n_cond : 0;
        a = {};
        a.A = ws.att; a.lda = d; a.W = lw.out_proj_w; a.ldw = d; a.C = ws.tmp; a.ldc = d;
        a.M = rows; a.N = d; a.K = d; a.bias = lw.out_proj_b; a.residual = X; a.ldr = d;
        a.a_grp = g; a.a_stride = gs; a.a_off = go; a.c_grp = g; a.c_stride = gs; a.c_off = go;
        // norm1 / norm2 CAN run inside the GEMM that produces their input (afm_linear_args.ln_*: the workgroup finishing the last column
        // tile of a block of rows normalises it; bit-identical).  Measured SLOWER than the separate launch on MI355X (B = 32: +20 us per
        // GEMM launch against 10.7 us per LayerNorm launch; B = 4: 0.679 vs 0.628 ms/step; profiles/r03_ln_fusion.md): every tile's
        // workgroup has to drain its write-through stores and wait for its ticket before it can retire.  Opt-in: AFM_CMDM_FUSED_LN.
        const bool fuse_ln = (w.flags & AFM_CMDM_FUSED_LN) != 0;
        if (fold) {
            a.stat_out = ws.stat1; a.ln_eps2 = 1e-5f;
            if (li > 0) { a.res_stat = ws.stat2; a.res_gamma = w.layer[li - 1].norm2_w; a.res_beta = w.layer[li - 1].norm2_b; }     // residual = LayerNorm(raw X)
            AFM_TRY(run_linear(w, a, s, rec, TAG_OUT_PROJ));
            a = {};                                   // linear1 on the raw rows, norm1 folded
            a.A = ws.tmp; a.lda = d; a.W = lw.lin1_wg; a.ldw = d; a.C = ws.hid; a.ldc = w.ff;
            a.M = rows; a.N = w.ff; a.K = d; a.bias = lw.lin1_c; a.act = AFM_ACT_GELU;
            a.a_stat = ws.stat1; a.a_stat_groups = sg; a.a_fold_g = lw.lin1_g; a.ln_eps2 = 1e-5f;
            a.a_grp = g; a.a_stride = gs; a.a_off = go;
            AFM_TRY(run_linear(w, a, s, rec, TAG_LINEAR1));
            a = {};                                   // linear2 + LayerNorm1(raw) as the residual -> raw output + its statistics
            a.A = ws.hid; a.lda = w.ff; a.W = lw.lin2_w; a.ldw = w.ff; a.C = ws.y; a.ldc = d;
            a.M = rows; a.N = d; a.K = w.ff; a.bias = lw.lin2_b; a.residual = ws.tmp; a.ldr = d;
            a.res_stat = ws.stat1; a.res_gamma = lw.norm1_w; a.res_beta = lw.norm1_b; a.stat_out = ws.stat2; a.ln_eps2 = 1e-5f;
            a.c_grp = g; a.c_stride = gs; a.c_off = go;
            AFM_TRY(run_linear(w, a, s, rec));
            X = ws.y;
            continue;
        }
        if (rec) return AFM_E_UNSUPPORTED;             // (the paired schedule exists for the folded-LayerNorm step only)
        if (fuse_ln) { a.ln_gamma = lw.norm1_w; a.ln_beta = lw.norm1_b; a.ln_out = ws.x1; a.ldo = d; a.ln_eps = 1e-5f; a.ln_counters = ws.lncnt; }
        AFM_TRY(run_linear(w, a, s));
        if (!fuse_ln) AFM_TRY(afm_layernorm_rows(ws.tmp, lw.norm1_w, lw.norm1_b, ws.x1, rows, d, 1e-5f, g, gs, go, s));
        a = {};
        a.A = ws.x1; a.lda = d; a.W = lw.lin1_w; a.ldw = d; a.C = ws.hid; a.ldc = w.ff;
        a.M = rows; a.N = w.ff; a.K = d; a.bias = lw.lin1_b; a.act = AFM_ACT_GELU;
        a.a_grp = g; a.a_stride = gs; a.a_off = go;                       // hid is written compactly [rows, ff]
        AFM_TRY(run_linear(w, a, s));
        a = {};
        a.A = ws.hid; a.lda = w.ff; a.W = lw.lin2_w; a.ldw = w.ff; a.C = ws.tmp; a.ldc = d;
        a.M = rows; a.N = d; a.K = w.ff; a.bias = lw.lin2_b; a.residual = ws.x1; a.ldr = d;
        a.c_grp = g; a.c_stride = gs; a.c_off = go;
        if (fuse_ln) { a.ln_gamma = lw.norm2_w; a.ln_beta = lw.norm2_b; a.ln_out = ws.y; a.ldo = d; a.ln_eps = 1e-5f; a.ln_counters = ws.lncnt; }
        AFM_TRY(run_linear(w, a, s));
        if (!fuse_ln) AFM_TRY(afm_layernorm_rows(ws.tmp, lw.norm2_w, lw.norm2_b, ws.y, rows, d, 1e-5f, g, gs, go, s));
        X = ws.y;
    }

    {   // motion_layer (cmdm.py:195) on the motion tokens only (cmdm.py:169), optional DDPM update
        afm_linear_args a = {};
        a.A = X; a.lda = d; a.W = w.motion_layer_w; a.ldw = d;
        a.C = x0_out; a.ldc = w.motion_dim; a.M = B * L; a.N = w.motion_dim; a.K = d;
        a.bias = w.motion_layer_b;
        if (fold) {                                   // X = the last layer's raw linear2 output
            a.W = w.motion_layer_wg; a.bias = w.motion_layer_c; a.a_stat = ws.stat2; a.a_stat_groups = sg; a.a_fold_g = w.motion_layer_g; a.ln_eps2 = 1e-5f;
        }
        a.a_grp = L; a.a_stride = T; a.a_off = 1 + w.n_cond;
        if (ddpm && (w.flags & AFM_PRIV_DDIM)) {
            // native DDIM loop: pred_xstart goes to the loop workspace's own buffer; the loop's update launch (afm_sampling_update)
            // then writes x_next and its K-padded copy.  The GEMM's epilogue is the one of the plain forward.
            if (!ws.x0) return AFM_E_BADARG;
            a.C = ws.x0; a.ldc = w.motion_dim;
        } else if (ddpm) {
            const float* nz = ddpm->noise;
            if (rec && !nz) return AFM_E_UNSUPPORTED;      // (recorded steps get their noise from the loop)
            if (!nz) {
                AFM_TRY(afm_randn(ws.noise, B, (int64_t)L * w.motion_dim, ddpm->seed, ddpm->sample_index0, ddpm->step, s));
                nz = ws.noise;
            }
            a.ddpm_xt = x_t; a.ddpm_noise = nz; a.ddpm_out = ddpm->x_next; a.ldx = w.motion_dim;
            a.ddpm_c1 = ddpm->c1; a.ddpm_c2 = ddpm->c2; a.ddpm_sigma = ddpm->sigma; a.rows_per_sample = L;
            a.ddpm_clip = (w.flags & AFM_CMDM_CLIP_X0) ? 1 : 0;
            if (ws.xpad) { a.ddpm_out2 = ws.xpad; a.ldx2 = w.motion_adapter_kpad; }      // x_next also as the NEXT step's K-padded A rows (the padding columns stay zero)
        }
        AFM_TRY(run_linear(w, a, s, rec));
    }
    return 0;
}

int validate(const afm_cmdm_weights* w, int B, int L) {
    if (!w || B < 0 || L <= 0) return AFM_E_BADARG;
    if (w->d <= 0 || (w->d & 3) || w->heads <= 0 || w->d % w->heads || w->ff <= 0 || (w->ff & 3)) return AFM_E_BADARG;
    if (w->n_layers <= 0 || w->n_layers > AFM_MAX_LAYERS || w->n_cond < 0 || w->motion_dim <= 0) return AFM_E_BADARG;
    if (w->d / w->heads != 64) return AFM_E_UNSUPPORTED;
    if (w->gemm_arith != AFM_ARITH_DEFAULT && w->gemm_arith != AFM_ARITH_F32 && w->gemm_arith != AFM_ARITH_BF16X6 && w->gemm_arith != AFM_ARITH_BF16X9 &&
        w->gemm_arith != AFM_ARITH_BF16X1) return AFM_E_BADARG;
    if (w->gemm_arith_min_n < 0 || w->attn_group_waves < 0) return AFM_E_BADARG;
    if (w->motion_adapter_kpad != 0 && (w->motion_adapter_kpad < w->motion_dim || (w->motion_adapter_kpad & 3))) return AFM_E_BADARG;
    if (!w->motion_adapter_w || !w->motion_layer_w || !w->time_table || !w->pos_table) return AFM_E_BADARG;
    return 0;
}

// a caller's pack as the library takes it: the library-private flag bits are never taken from a caller (`also`: more bits to clear)
inline afm_cmdm_weights callers_pack(const afm_cmdm_weights& w, uint32_t also = 0) {
    afm_cmdm_weights r = w;
    r.flags &= ~(AFM_PRIV_DDIM | AFM_PRIV_NO_NOISE | also);
    return r;
}

// The extra evaluations of a guided step, in launch order behind the conditioned one: [middle,] unconditioned.
struct GuideBranch { afm_cmdm_weights w; Branch br; };       // the pack copy an extra evaluation runs on, and its layout
struct Guidance {                     // n == 0: unguided
    int n;
    GuideBranch b[2];
    const float* scale[2];            // [B] rows: scale[0] = Update::scale, scale[1] = Update::scale2 (two scales only)
    void* const* branch_streams;      // one extra branch only
};

inline bool cfg2_ok(const afm_cfg2_args* c) { return c && c->scale_first && c->scale_second && (c->first == 0 || c->first == 1); }

// The list of either public description (`two` wins; neither: AFM_E_BADARG) for the pack `w`.  One scale: the unconditioned branch drops
// what the caller names.  Two scales: the middle branch keeps the first condition only - always a masked form - and the unconditioned one
// drops both (scale[0]: the first condition's, the row cfg_combine2's inner cfg_combine reads).  A branch that drops every condition is
// compact (n_cond = 0 in its pack, the positional rows of the full layout) unless AFM_CFG_FORCE_MASKED.  `to_run`: also refuse a masked
// form without a frame mask (the key mask is built from it); the workspace sizes do not depend on it.
int make_guidance(const afm_cmdm_weights& w, const afm_cfg_args* one, const afm_cfg2_args* two, bool to_run, const uint8_t* frame_mask, Guidance* g) {
    *g = {};
    if (two ? !cfg2_ok(two) : (!one || !one->scale || (!one->drop_text && !one->drop_pc))) return AFM_E_BADARG;
    if (w.n_cond < 1) return AFM_E_BADARG;
    const bool text = two || one->drop_text, pc = two || one->drop_pc;         // what the unconditioned branch drops
    const bool compact = text && pc && !((two ? two->flags : one->flags) & AFM_CFG_FORCE_MASKED);
    if (to_run && !frame_mask && (two || !compact)) return AFM_E_BADARG;
    auto add = [&](bool mask_text, bool mask_pc) { g->b[g->n++] = GuideBranch{w, {1 + w.n_cond, mask_text, mask_pc}}; };
    if (two) add(two->first == 1, two->first == 0);
    add(!compact && text, !compact && pc);
    if (compact) g->b[g->n - 1].w.n_cond = 0;
    g->scale[0] = two ? two->scale_first : one->scale;
    g->scale[1] = two ? two->scale_second : nullptr;
    g->branch_streams = two ? nullptr : one->branch_streams;
    return 0;
}

// One guided evaluation: validate, the library's own copy of the pack, the conditioned evaluation and each branch of the list in turn on
// one workspace (no branch's layout is larger than the conditioned one's), then the combine launch.  outs: pred_xstart of c, [a,] u
// (NULL: the region behind the workspace, in that order).
int guided_forward(const afm_cmdm_weights* w, const afm_cfg_args* one, const afm_cfg2_args* two, const float* x_t, const int64_t* t,
                   const float* cond_tokens, const uint8_t* frame_mask, float** outs, float* x0_guided, int B, int L, void* workspace,
                   int64_t workspace_bytes, hipStream_t s) {
    AFM_TRY(validate(w, B, L));
    if (!x_t || !t || !cond_tokens || !workspace || !x0_guided) return AFM_E_BADARG;
    const afm_cmdm_weights wc = callers_pack(*w, AFM_CMDM_FUSED_LN);         // (the opt-in fused LayerNorm is not built here)
    Guidance g;
    AFM_TRY(make_guidance(wc, one, two, true, frame_mask, &g));
    if (B == 0) return 0;
    const Workspace ws = carve(wc, B, L, workspace);
    const int64_t xb = align256((int64_t)B * L * w->motion_dim * 4);
    if (ws.bytes + (1 + g.n) * xb > workspace_bytes) return AFM_E_WORKSPACE;
    Workspace wsb[2];
    for (int i = 0; i < g.n; ++i) {
        wsb[i] = carve(g.b[i].w, B, L, workspace);
        if (wsb[i].bytes > ws.bytes) return AFM_E_WORKSPACE;
    }
    for (int i = 0; i <= g.n; ++i)
        if (!outs[i]) outs[i] = (float*)((char*)workspace + ws.bytes + i * xb);
    AFM_TRY(forward_impl(wc, x_t, t, cond_tokens, frame_mask, outs[0], nullptr, B, L, ws, true, s));
    for (int i = 0; i < g.n; ++i)
        AFM_TRY(forward_impl(g.b[i].w, x_t, t, cond_tokens, frame_mask, outs[1 + i], nullptr, B, L, wsb[i], true, s, nullptr, &g.b[i].br));
    const int64_t per = (int64_t)L * w->motion_dim;
    if (g.n == 1) return afm_cfg_combine(outs[0], outs[1], g.scale[0], x0_guided, B, per, s);
    return afm_cfg2_combine(outs[0], outs[1], outs[2], g.scale[0], g.scale[1], x0_guided, B, per, s);
}

// the workspace of a guided evaluation: the conditioned one's, and a pred_xstart region for it and for each of the n_extra branches
int64_t guided_workspace_bytes(const afm_cmdm_weights* w, int B, int L, int n_extra) {
    if (validate(w, B, L) != 0) return AFM_E_BADARG;
    return carve(*w, B, L, nullptr).bytes + (1 + n_extra) * align256((int64_t)B * L * w->motion_dim * 4);
}

}  // namespace

extern "C" int afm_version(void) { return AFM_ABI_VERSION; }

extern "C" int64_t afm_cmdm_workspace_bytes(const afm_cmdm_weights* w, int32_t B, int32_t L) {
    if (validate(w, B, L) != 0) return AFM_E_BADARG;
    return carve(*w, B, L, nullptr).bytes;
}

extern "C" int afm_cmdm_forward(const afm_cmdm_weights* w, const float* x_t, const int64_t* t, const float* cond_tokens,
                                const uint8_t* frame_mask, float* x0_out, const afm_ddpm_args* ddpm, int32_t B, int32_t L,
                                void* workspace, int64_t workspace_bytes, void* stream) {
    AFM_TRY(validate(w, B, L));
    if (!x_t || !t || (w->n_cond > 0 && !cond_tokens) || !workspace) return AFM_E_BADARG;
    if (!x0_out && !ddpm) return AFM_E_BADARG;
    if (ddpm && (!ddpm->x_next || !ddpm->c1 || !ddpm->c2 || !ddpm->sigma)) return AFM_E_BADARG;
    if (B == 0) return 0;
    const afm_cmdm_weights wpub = callers_pack(*w);
    w = &wpub;
    const Workspace ws = carve(*w, B, L, workspace);
    if (ws.bytes > workspace_bytes) return AFM_E_WORKSPACE;
    if ((w->flags & AFM_CMDM_FUSED_LN) &&           // ticket words of the opt-in fused LayerNorm only
        hipMemsetAsync(ws.lncnt, 0, (size_t)(((int64_t)B * (1 + w->n_cond + L) + 31) / 32) * 4, (hipStream_t)stream) != hipSuccess) return (int)hipGetLastError();
    return forward_impl(*w, x_t, t, cond_tokens, frame_mask, x0_out, ddpm, B, L, ws, true, (hipStream_t)stream);
}

extern "C" int64_t afm_cmdm_cfg_workspace_bytes(const afm_cmdm_weights* w, int32_t B, int32_t L) {
    return guided_workspace_bytes(w, B, L, 1);
}

extern "C" int afm_cmdm_cfg_forward(const afm_cmdm_weights* w, const float* x_t, const int64_t* t, const float* cond_tokens,
                                    const uint8_t* frame_mask, const afm_cfg_args* cfg, float* x0_c, float* x0_u, float* x0_guided,
                                    int32_t B, int32_t L, void* workspace, int64_t workspace_bytes, void* stream) {
    float* outs[] = {x0_c, x0_u};
    return guided_forward(w, cfg, nullptr, x_t, t, cond_tokens, frame_mask, outs, x0_guided, B, L, workspace, workspace_bytes, (hipStream_t)stream);
}

extern "C" int64_t afm_cmdm_cfg2_workspace_bytes(const afm_cmdm_weights* w, int32_t B, int32_t L) {
    return guided_workspace_bytes(w, B, L, 2);
}

extern "C" int afm_cmdm_cfg2_forward(const afm_cmdm_weights* w, const float* x_t, const int64_t* t, const float* cond_tokens,
                                     const uint8_t* frame_mask, const afm_cfg2_args* cfg, float* x0_c, float* x0_a, float* x0_u, float* x0_guided,
                                     int32_t B, int32_t L, void* workspace, int64_t workspace_bytes, void* stream) {
    float* outs[] = {x0_c, x0_a, x0_u};
    return guided_forward(w, nullptr, cfg, x_t, t, cond_tokens, frame_mask, outs, x0_guided, B, L, workspace, workspace_bytes, (hipStream_t)stream);
}

extern "C" int64_t afm_cmdm_sched_scratch_bytes(int32_t n_steps, int32_t B) {
    if (n_steps <= 0 || B < 0) return AFM_E_BADARG;
    return align256((int64_t)n_steps * B * 8) + 3 * align256((int64_t)n_steps * B * 4);
}

// DDIM loops (CMDM and CDM): t [n_steps][B] int64, {a, b, c, d} records [n_steps][B] float4, s [n_steps][B] float
extern "C" int64_t afm_ddim_sched_scratch_bytes(int32_t n_steps, int32_t B) {
    if (n_steps <= 0 || B < 0) return AFM_E_BADARG;
    return align256((int64_t)n_steps * B * 8) + align256((int64_t)n_steps * B * 16) + align256((int64_t)n_steps * B * 4);
}

// ------------------------------------------------------------------------------------------------ native sampling loop
// One driver for the four loops: DDPM (the ancestral update with the rows c1 / c2 / sigma, fused into the motion_layer epilogue) or DDIM
// (`ddim` != NULL: motion_layer stores pred_xstart and ONE elementwise launch per sub-batch and step, afm_sampling_update, applies the
// update), each unguided or guided (`cfg` != NULL).  (The DDIM update fused into the shared GEMM epilogue grew the registers - and on three
// variants the scratch - of DDPM GEMM kernels that every sampling step runs; a launch of its own leaves them as they were.)
// The DPM-Solver++(2M) loop (`a.dpm`) is the eta = 0 DDIM loop with the 2M update in that launch and one history buffer per sub-batch.
// plan_loop decides everything a call fixes before its first launch; the step functions enqueue one (sub-batch, step); sample_loop_impl
// owns the schedule, the events and the order.  The shared pieces (sub-batches, schedule, noise, events) live in sample_loop.h.
namespace {

constexpr int MAX_SUB = 16;           // sub-batches (streams) of one loop call
constexpr int NEV = 2 * AFM_MAX_LAYERS;      // events of the paired schedule: two cross-stream edges per layer

// the arguments of the loop entry points (afm_cmdm_sample_loop and the thirteen *_loop_range entries): the model's tensors, the guidance as
// the caller describes it (at most one of cfg / cfg2; neither: unguided), what every loop takes, the imputation
struct LoopCall {
    const afm_cmdm_weights* w;
    float* x;
    const float* cond_tokens;
    const uint8_t* frame_mask;
    const afm_cfg_args* cfg;
    int L;
    LoopArgs a;                       // (a.streams: one side stream per sub-batch)
    const float* known = nullptr;     // imputing loop: [B][L][motion_dim] each, both set (neither: no imputation)
    const uint8_t* mask = nullptr;
    const afm_cfg2_args* cfg2 = nullptr;
    afm_motion_guide guide = {};      // guided loop: the terms' descriptions of the whole batch (neither term set: none)
    const afm_scene_clearance* clear = nullptr;      // scene-guided loop: the clearance next to (or without) the terms of `guide`
    const afm_foot_grounding* feet = nullptr;        // ground-guided loop: the foot grounding behind (or without) the other terms
    bool guided() const { return guide.contact || guide.targets || clear || feet; }
    afm_stitch stitch = {};           // stitched loop: the batch is windows of long motions (windows == 0: not stitched)
    const afm_long_guide* lguide = nullptr;      // long-guided stitched loop: `guide` holds its terms, `stitch` its stitch
    bool stitched() const { return stitch.windows > 0; }
};

// the one maker of a LoopCall, from what the entries' signatures hold in one form or another (`ddim` set: DDPM rows next to it are
// dropped).  a.dpm, the term and the windows are set on the result by the one function that knows them (every_form_range).
LoopCall loop_call(const afm_cmdm_weights* w, float* x, const float* cond_tokens, const uint8_t* frame_mask, const float* step_noise,
                   const int64_t* tmap, const afm_ddim_rows* ddim, const float* c1, const float* c2, const float* sigma, int n_steps, int first_step,
                   uint64_t seed, int64_t sample_index0, int B, int L, void* sched_scratch, void* workspace, int64_t workspace_bytes, int n_streams,
                   void* const* side_streams, void* stream, const afm_cfg_args* cfg = nullptr, const afm_cfg2_args* cfg2 = nullptr,
                   const float* known = nullptr, const uint8_t* mask = nullptr) {
    if (ddim) c1 = c2 = sigma = nullptr;
    return {w, x, cond_tokens, frame_mask, cfg, L, {step_noise, tmap, c1, c2, sigma, ddim, n_steps, first_step, seed, sample_index0, B,
            sched_scratch, workspace, workspace_bytes, n_streams, side_streams, stream}, known, mask, cfg2};
}

// exactly one kind of rows - DDIM, 2M (complete) or (`ddpm`) DDPM - else AFM_E_BADARG; 2M rows travel through the DDIM schedule layout
// as {a, b, c, d = c: any valid row, never used by dpm_update}: written to *as_ddim, which *rows then names
int one_kind_of_rows(const afm_ddim_rows** rows, const afm_dpm_rows* dpm, bool ddpm, afm_ddim_rows* as_ddim) {
    if ((*rows != nullptr) + (dpm != nullptr) + (ddpm ? 1 : 0) != 1 || (dpm && (!dpm->a || !dpm->b || !dpm->c))) return AFM_E_BADARG;
    if (dpm) { *as_ddim = {dpm->a, dpm->b, dpm->c, dpm->c, nullptr}; *rows = as_ddim; }
    return 0;
}

// the sample range of sub-batch s of n over a batch of B cut in units of `unit` samples (a stitched loop: the windows of one long motion,
// so a window and its neighbour share a sub-batch and a stream; 1: single samples): the one rule of the loops and of their sizers
inline int unit_sub_count(int B, int unit, int n_streams) { return sub_count(B / unit, n_streams, MAX_SUB); }
inline void unit_sub_range(int B, int unit, int n, int s, int* start, int* count) {
    sub_range(B / unit, n, s, start, count);
    *start *= unit; *count *= unit;
}

struct SubBatch : SubRange {
    Workspace ws, wsb[2];             // guided loops: wsb[i] the workspace of branch i of the list, behind ws in list order
    // guided loop with branch streams: the unconditioned branch runs on `branch`; two events order it against the guided update, the only
    // writer of x and of its K-padded copy (x_ready: x is ready, u_ready: the branch's pred_xstart is ready)
    hipStream_t branch;
    hipEvent_t x_ready, u_ready;
    float* hist;                      // 2M loop only: the previous step's final x0 [count][L * motion_dim], behind every evaluation's workspace
    float* ggrad;                     // guided loop only: the step's gradient [count][L * motion_dim], behind the history, and the
    char* gws;                        //   workspace of afm_motion_guidance for `count` samples behind it
    int64_t gws_bytes;
};

// carves the workspaces of a sub-batch whose range is set at `base` (NULL: sizes only); -> their bytes
int64_t carve_sub(const afm_cmdm_weights& w, const Guidance& g, int L, char* base, SubBatch* sb, bool hist, const afm_motion_guide* guide = nullptr,
                  const afm_long_guide* lguide = nullptr, const afm_scene_clearance* clear = nullptr, const afm_foot_grounding* feet = nullptr) {
    sb->ws = carve(w, sb->count, L, base, NOISE_STEPS);
    int64_t off = sb->ws.bytes;
    for (int i = 0; i < g.n; ++i) {
        // (2 "noise steps": a pred_xstart region of its own, as little noise space as the layout allows)
        sb->wsb[i] = carve(g.b[i].w, sb->count, L, base ? base + off : nullptr, 2);
        sb->wsb[i].xpad = sb->ws.xpad;       // one K-padded copy of x_t serves every branch
        off += sb->wsb[i].bytes;
    }
    sb->hist = nullptr;
    if (hist) {                       // (carved for the 2M loop alone: the other forms' sizes stay as they are)
        sb->hist = base ? (float*)(base + off) : nullptr;
        off += align256((int64_t)sb->count * L * w.motion_dim * 4);
    }
    sb->ggrad = nullptr; sb->gws = nullptr; sb->gws_bytes = 0;
    if (guide) {                      // (carved for the guided loops alone)
        sb->ggrad = base ? (float*)(base + off) : nullptr;
        off += align256((int64_t)sb->count * L * w.motion_dim * 4);
        sb->gws = base ? base + off : nullptr;
        sb->gws_bytes = lguide ? afm_long_scene_guide_workspace_bytes(lguide, clear, sb->count / lguide->stitch.windows, L, w.motion_dim)
                               : afm_ground_guide_workspace_bytes(guide, clear, feet, sb->count, L, w.motion_dim);
        off += align256(sb->gws_bytes);
    }
    return off;
}

// the loop workspace of either public description of the guidance (neither: the unguided loop's); AFM_E_BADARG as the loop itself
int64_t loop_workspace_bytes(const afm_cmdm_weights* w, const afm_cfg_args* one, const afm_cfg2_args* two, int B, int L, int n_streams,
                             bool hist = false, const afm_motion_guide* guide = nullptr, int unit = 1, const afm_long_guide* lguide = nullptr,
                             const afm_scene_clearance* clear = nullptr, const afm_foot_grounding* feet = nullptr) {
    if (validate(w, B, L) != 0 || n_streams < 0 || unit < 1 || B % unit != 0) return AFM_E_BADARG;
    if (guide && !guide->contact && !guide->targets && !clear && !feet) return AFM_E_BADARG;
    if (feet && lguide) return AFM_E_BADARG;
    if ((clear || feet) &&
        (lguide ? afm_long_scene_guide_check(lguide, clear, L, w->motion_dim) : afm_ground_guide_check(guide, clear, feet, L, w->motion_dim)) != 0)
        return AFM_E_BADARG;
    if (guide && guide->contact && afm_contact_guidance_workspace_bytes(B, guide->contact->N, guide->contact->K) < 0) return AFM_E_BADARG;
    if (guide && guide->targets && (guide->targets->K <= 0 || guide->targets->K > AFM_GUIDE_MAX_JOINTS)) return AFM_E_BADARG;
    Guidance g = {};
    if ((one || two) && make_guidance(*w, one, two, false, nullptr, &g) != 0) return AFM_E_BADARG;
    const int n = unit_sub_count(B, unit, n_streams);
    int64_t total = 0;
    for (int s = 0; s < n; ++s) {
        SubBatch sb = {};
        unit_sub_range(B, unit, n, s, &sb.start, &sb.count);
        total += carve_sub(*w, g, L, nullptr, &sb, hist, guide, lguide, clear, feet);
    }
    return total;
}

// what a loop call fixes before its first launch: the loop's own weight packs, the sub-batches with their streams and workspaces, the form
struct LoopPlan {
    afm_cmdm_weights w;               // the loop's copy: flags (private bits, tile code) set here
    Guidance g;                       // the extra evaluations of a guided loop, the loop's flags on their packs too
    int nsub;                         // 0: an empty batch, nothing to enqueue
    SubBatch sb[MAX_SUB];
    bool paired;                      // AFM_CMDM_PAIR_LAUNCH, two sub-batches: every step after the first is recorded and issued interleaved
    bool branch_streams;
    int64_t row;                      // values per sample
};

int plan_loop(const LoopCall& c, LoopPlan* p) {
    const LoopArgs& a = c.a;
    AFM_TRY(validate(c.w, a.B, c.L));
    // Guided loop (g.n > 0): per sub-batch and step the conditioned evaluation (this loop's step as it is, pred_xstart stored the DDIM
    // loop's way, for DDPM too), each branch of the list on a workspace of its own behind it on the same stream, and ONE update launch
    // (afm_sampling_update).  Every evaluation reads the same x / K-padded copy; only the update writes them.
    Guidance& g = p->g;               // (n == 0 as the caller zeroed the plan)
    if (c.cfg || c.cfg2) AFM_TRY(make_guidance(*c.w, c.cfg, c.cfg2, true, c.frame_mask, &g));
    if (g.n > 1 && g.branch_streams) return AFM_E_UNSUPPORTED;       // (four hardware queues do not fit 2 sub-batches x 3 evaluations)
    if (!c.x || (c.w->n_cond > 0 && !c.cond_tokens) || !a.ok() || !c.known != !c.mask) return AFM_E_BADARG;
    if (a.dpm && (!a.ddim || a.noise_term() || a.step_noise || a.first_step < 0)) return AFM_E_BADARG;
    if (c.guided()) {
        if (c.lguide && c.feet) return AFM_E_BADARG;          // (a long or stitched description takes no grounding)
        AFM_TRY(c.lguide ? afm_long_scene_guide_check(c.lguide, c.clear, c.L, c.w->motion_dim)
                         : afm_ground_guide_check(&c.guide, c.clear, c.feet, c.L, c.w->motion_dim));
        if (!c.guide.gk || (c.guide.contact && c.guide.contact->first_guided < 0) || (c.guide.targets && c.guide.targets->first_guided < 0) ||
            (c.clear && c.clear->first_guided < 0) || (c.feet && c.feet->first_guided < 0)) return AFM_E_BADARG;
    }
    const int unit = c.stitched() ? c.stitch.windows : 1;
    if (c.lguide && !c.stitched()) return AFM_E_BADARG;
    if (c.stitched()) {               // whole long motions, a frame in at most two windows, a deterministic update, no gradient term but a long one
        const afm_stitch& st = c.stitch;
        if (st.overlap < 0 || 2 * (int64_t)st.overlap > c.L || a.B % st.windows != 0 || !a.ddim || a.noise_term() || a.step_noise || (c.guided() && !c.lguide)) return AFM_E_BADARG;
        if (st.windows > 1 && st.overlap > 0 && !st.weights) return AFM_E_BADARG;
    }
    p->nsub = 0;
    if (a.B == 0) return 0;
    p->nsub = unit_sub_count(a.B, unit, a.n_streams);
    p->branch_streams = g.branch_streams != nullptr;
    int64_t off = 0;
    for (int s = 0; s < p->nsub; ++s) {
        SubBatch& sb = p->sb[s];
        sb = {};
        unit_sub_range(a.B, unit, p->nsub, s, &sb.start, &sb.count);
        off += carve_sub(*c.w, g, c.L, (char*)a.workspace + off, &sb, a.dpm || c.guided() || c.stitched(), c.guided() ? &c.guide : nullptr, c.lguide, c.clear, c.feet);
        sb.stream = p->nsub > 1 ? (hipStream_t)a.streams[s] : (hipStream_t)a.stream;
        if (p->branch_streams) sb.branch = (hipStream_t)g.branch_streams[s];
    }
    if (off > a.workspace_bytes) return AFM_E_WORKSPACE;

    // Tile shape of the wide encoder GEMMs inside the multi-stream loop (round 6).  afm_linear's own rule prices ONE launch: 128 x 128 tiles only
    // when their last resident round is >= 90 % full (in_proj), 64 x 64 otherwise.  Inside this loop a second sub-batch's kernels fill the
    // slots a partial round leaves, and what counts is the work per matrix instruction (the loop runs at the board's power limit): with the
    // six-product arithmetic, 128 x 128 on EVERY GEMM with N >= 512 measured 588-590 against 568-574 steps/s at 16 + 16 samples in the same
    // calls, but 853 against 995 at 8 + 8 and 1168 against 1470 at 4 + 4 (profiles/r06_tile_rule.md) - so: sub-batches of >= 4096 rows only.
    // Round 7: the same 128 x 128 tile on 512 threads (tile code 14: two of the tile's waves per SIMD) - 611-612 against 580 steps/s for code 5
    // in one call (profiles/r07_gemm128_timeline.md); code 5 stays reachable through the override.  Code 14's epilogue is the streamed one
    // (csrc/gemm_epilogue.h; 633-638 against 612-618 steps/s for code 15, the same tile with the shared epilogue: profiles/gemm128_epilogue.md).
    // Tile shapes of one arithmetic are bit-identical; a caller's explicit AFM_CMDM_WIDE_TILE code wins.
    const int T = 1 + c.w->n_cond + c.L;
    p->w = *c.w;
    p->w.flags = a.loop_flags(p->w.flags);
    // (an imputing loop likewise: the update fused into the motion_layer epilogue is contracted and has no place for the select)
    // (a contact- or target-guided loop too: no place for the gradient term either)
    // (a stitched loop too: the blend reads the neighbour window's pred_xstart, which only a launch behind the evaluation can)
    if (g.n || c.mask || c.guided() || c.stitched()) p->w.flags = (p->w.flags | AFM_PRIV_DDIM) & ~(AFM_CMDM_PAIR_LAUNCH | AFM_CMDM_FUSED_LN);
    if (p->nsub >= 2 && ((p->w.flags >> AFM_CMDM_WIDE_TILE_SHIFT) & 0xF) == 0) {
        bool big = true;
        for (int s = 0; s < p->nsub; ++s) big = big && (int64_t)p->sb[s].count * T >= 4096;
        if (big) p->w.flags |= 14 << AFM_CMDM_WIDE_TILE_SHIFT;
    }
    for (int i = 0; i < g.n; ++i) g.b[i].w.flags = p->w.flags;       // the loop's flags (tile code, private bits) on every branch's pack
    p->paired = (p->w.flags & AFM_CMDM_PAIR_LAUNCH) && p->nsub == 2 && p->sb[0].count > 0 && p->sb[1].count > 0;
    p->row = (int64_t)c.L * c.w->motion_dim;
    return 0;
}

struct Loop {
    const LoopCall& c;
    LoopPlan p;
    Schedule sched;
};

// the sub-batch's slices of the call's tensors
inline float* sub_x(const Loop& l, const SubBatch& sb) { return l.c.x + (int64_t)sb.start * l.p.row; }
inline const float* sub_cond(const Loop& l, const SubBatch& sb) { return l.c.cond_tokens ? l.c.cond_tokens + (int64_t)sb.start * l.p.w.n_cond * l.p.w.d : nullptr; }
inline const uint8_t* sub_fmask(const Loop& l, const SubBatch& sb) { return l.c.frame_mask ? l.c.frame_mask + (int64_t)sb.start * l.c.L : nullptr; }

// the conditioned evaluation of (sub-batch, step j) on the sub-batch's stream, or into `rec`; *rows and *dd: what the update launches
// behind it read (in a DDPM loop the evaluation's own epilogue is the update)
int cond_forward(const Loop& l, const SubBatch& sb, int j, StepRows* rows, afm_ddpm_args* dd, Recorder* rec) {
    const LoopCall& c = l.c;
    const float* nz;
    AFM_TRY(step_noise(c.a, l.p.row, sb, sb.ws.noise, j, sub_x(l, sb), &sb.stream, &nz));
    *rows = l.sched.at(j, sb.start);
    *dd = ddpm_args(c.a, *rows, nz, sub_x(l, sb), sb, j);
    return forward_impl(l.p.w, sub_x(l, sb), rows->t, sub_cond(l, sb), sub_fmask(l, sb), nullptr, dd, sb.count, c.L, sb.ws, j == 0, sb.stream, rec);
}

// the terms of the guidance executed step j of the call carries: each one at or behind its own first guided step
inline bool contact_step(const Loop& l, int j) { return l.c.guide.contact && l.c.a.first_step + j >= l.c.guide.contact->first_guided; }
inline bool targets_step(const Loop& l, int j) { return l.c.guide.targets && l.c.a.first_step + j >= l.c.guide.targets->first_guided; }
inline bool clear_step(const Loop& l, int j) { return l.c.clear && l.c.a.first_step + j >= l.c.clear->first_guided; }
inline bool feet_step(const Loop& l, int j) { return l.c.feet && l.c.a.first_step + j >= l.c.feet->first_guided; }
inline bool guided_step(const Loop& l, int j) { return contact_step(l, j) || targets_step(l, j) || clear_step(l, j) || feet_step(l, j); }

// the gradient of (sub-batch, step j) at the x the step's evaluations read, on the sub-batch's stream: the launches of afm_motion_guidance
// for the step's terms (contact: two, h3d four; targets: one, h3d three; clearance: one, h3d three; grounding: one, h3d three) into the sub-batch's gradient buffer
int guide_launch(const Loop& l, const SubBatch& sb, int j) {
    if (l.c.lguide) {                 // (sb.start and sb.count are whole long motions)
        const int S = l.c.lguide->stitch.windows;
        return afm_long_scene_guidance_sub(l.c.lguide, l.c.clear, contact_step(l, j), targets_step(l, j), clear_step(l, j), sb.start / S, sub_x(l, sb),
                                           nullptr, sb.ggrad, nullptr, nullptr, nullptr, sb.count / S, l.c.L, l.p.w.motion_dim, sb.gws, sb.gws_bytes,
                                           sb.stream);
    }
    // (the guidance's own mask: the denoiser's frame_mask is NULL for a model that does not mask its motion tokens)
    const uint8_t* fm = l.c.guide.frame_mask ? l.c.guide.frame_mask + (int64_t)sb.start * l.c.L : nullptr;
    return afm_ground_guidance_sub(&l.c.guide, l.c.clear, l.c.feet, contact_step(l, j), targets_step(l, j), clear_step(l, j), feet_step(l, j), sb.start,
                                   sub_x(l, sb), fm, nullptr, sb.ggrad, nullptr, nullptr, nullptr, nullptr, sb.count, l.c.L, l.p.w.motion_dim, sb.gws,
                                   sb.gws_bytes, sb.stream);
}

// the update of a sub-batch from its stored pred_xstart (ws.x0; guided: and each branch's, wsb[i].x0 - the list's last branch is the
// unconditioned one, a branch in front of it the middle one), in place on x, with the K-padded copy the next step reads.  2M loop: the
// final x0 of step j is kept in the sub-batch's history, which the next step - of this call or of the next range call on the same
// workspace - reads; the first executed step of a chain (first_step + j == 0) has no history and takes the two-term form
int update_launch(const Loop& l, const SubBatch& sb, const StepRows& rows, const float* noise, int j) {
    const afm_cmdm_weights& w = l.p.w;
    const Guidance& g = l.p.g;
    Update u = loop_update(l.c.a, rows, sb.ws.x0, sub_x(l, sb), noise, l.p.row, w.flags & AFM_CMDM_CLIP_X0);
    if (g.n > 0) { u.x0_u = sb.wsb[g.n - 1].x0; u.scale = g.scale[0] + sb.start; }
    if (g.n > 1) { u.x0_a = sb.wsb[0].x0; u.scale2 = g.scale[1] + sb.start; }
    if (l.c.mask) { u.known = l.c.known + (int64_t)sb.start * l.p.row; u.mask = l.c.mask + (int64_t)sb.start * l.p.row; }
    u.xpad = sb.ws.xpad; u.ldpad = w.motion_adapter_kpad; u.cols = w.motion_dim;
    if (l.c.a.dpm) { u.x0_prev = l.c.a.first_step + j > 0 ? sb.hist : nullptr; u.x0_keep = sb.hist; }
    if (l.c.stitched()) {             // (sb.start is a multiple of the windows: the kernel's b % st_S is the window's place)
        u.st_S = l.c.stitch.windows; u.st_ov = l.c.stitch.overlap; u.st_L = l.c.L; u.st_D = w.motion_dim; u.st_w = l.c.stitch.weights;
    }
    if (guided_step(l, j)) { u.grad = sb.ggrad; u.gk = l.c.guide.gk + ((int64_t)(l.c.a.n_steps - 1 - j) * l.c.a.B + sb.start); }
    return afm_sampling_update(u, sb.count, sb.stream);
}

// one (sub-batch, step): the conditioned evaluation, each branch of a guided loop's list, the update launch (a plain DDPM loop has none:
// the conditioned evaluation's own epilogue is the update)
int loop_step(const Loop& l, const SubBatch& sb, int j) {
    const LoopCall& c = l.c;
    const Guidance& g = l.p.g;
    StepRows rows;
    afm_ddpm_args dd;
    if (guided_step(l, j)) AFM_TRY(guide_launch(l, sb, j));
    AFM_TRY(cond_forward(l, sb, j, &rows, &dd, nullptr));
    for (int i = 0; i < g.n; ++i) {
        // every branch behind the conditioned evaluation on the sub-batch's stream, on its own workspace - but the last one on the branch
        // stream when there is one.  step 0: the branch's prologue rewrites the shared K-padded copy (same values), so it starts behind
        // the conditioned evaluation; later steps: behind the previous update, next to the conditioned evaluation
        const bool bs = l.p.branch_streams && i == g.n - 1;
        const hipStream_t su = bs ? sb.branch : sb.stream;
        if (bs) {
            if (j == 0) (void)hipEventRecord(sb.x_ready, sb.stream);
            (void)hipStreamWaitEvent(su, sb.x_ready, 0);
        }
        const int rc = forward_impl(g.b[i].w, sub_x(l, sb), rows.t, sub_cond(l, sb), sub_fmask(l, sb), nullptr, &dd, sb.count, c.L, sb.wsb[i], j == 0, su,
                                    nullptr, &g.b[i].br);
        if (bs) {       // (also behind a failed branch: the sub-batch's stream never runs ahead of its branch stream)
            (void)hipEventRecord(sb.u_ready, su);
            (void)hipStreamWaitEvent(sb.stream, sb.u_ready, 0);
        }
        AFM_TRY(rc);
    }
    if (!(g.n || c.a.ddim || c.mask || c.guided())) return 0;
    AFM_TRY(update_launch(l, sb, rows, dd.noise, j));
    if (l.p.branch_streams) (void)hipEventRecord(sb.x_ready, sb.stream);       // x and its padded copy of the next step
    return 0;
}

// ---- the paired schedule of one step (AFM_CMDM_PAIR_LAUNCH; two sub-batches A, B on streams sa, sb).  Both lists hold the same launch
// sequence.  Per layer: sub-batch B runs up to and including its out_proj on sb; then ONE launch on sa computes A's out_proj AND B's linear1
// (afm_linear_pair: 164 + 328 = 492 tiles of 128 x 128 at 16 samples per sub-batch - one full resident round); B continues with linear2 on
// sb, A with linear1 on sa.  Two cross-stream edges per layer: sb -> sa before the pair (B's out_proj output and statistics), sa -> sb after
// it (B's hidden rows).  Every element is computed by the same tile program on the same operands: bit-identical to the unpaired schedule.
int issue_paired(const Recorder& A, const Recorder& B, hipStream_t sa, hipStream_t sb, const hipEvent_t* ev, int nev) {
    if (A.n != B.n) return AFM_E_UNSUPPORTED;
    int ia = 0, ib = 0, e = 0;
    while (ia < A.n) {
        const bool pair = A.ops[ia].tag == TAG_OUT_PROJ && ia + 1 < B.n && B.ops[ia + 1].tag == TAG_LINEAR1 && ib <= ia + 1 && e + 2 <= nev;
        if (pair) {
            while (ib <= ia) AFM_TRY(launch_op(B.ops[ib++], sb));                     // B up to and including its out_proj
            if (hipEventRecord(ev[e], sb) != hipSuccess || hipStreamWaitEvent(sa, ev[e], 0) != hipSuccess) return (int)hipGetLastError();
            const int rc = afm_linear_pair(&A.ops[ia].a, &B.ops[ia + 1].a, sa);
            if (rc == AFM_E_UNSUPPORTED) {                                             // shapes the paired form does not take: two plain launches
                AFM_TRY(launch_op(A.ops[ia], sa));
                AFM_TRY(launch_op(B.ops[ia + 1], sa));
            } else if (rc != 0) return rc;
            if (hipEventRecord(ev[e + 1], sa) != hipSuccess || hipStreamWaitEvent(sb, ev[e + 1], 0) != hipSuccess) return (int)hipGetLastError();
            e += 2;
            ia += 1; ib = ia + 1;                                                      // B's linear1 is done
        } else {
            AFM_TRY(launch_op(A.ops[ia++], sa));
        }
    }
    while (ib < B.n) AFM_TRY(launch_op(B.ops[ib++], sb));
    return 0;
}

// a step of the paired schedule: both sub-batches' launches recorded, issued interleaved, then (DDIM) each sub-batch's update behind its
// recorded launches
int paired_step(const Loop& l, int j, Recorder* recs, const hipEvent_t* pev) {
    StepRows rows[2];
    afm_ddpm_args dd[2];
    for (int s = 0; s < 2; ++s) {
        recs[s].n = 0;
        AFM_TRY(cond_forward(l, l.p.sb[s], j, &rows[s], &dd[s], &recs[s]));
    }
    AFM_TRY(issue_paired(recs[0], recs[1], l.p.sb[0].stream, l.p.sb[1].stream, pev, NEV));
    for (int s = 0; l.c.a.ddim && s < 2; ++s) AFM_TRY(update_launch(l, l.p.sb[s], rows[s], dd[s].noise, j));
    return 0;
}

// the events of a loop call, all owned by `ev`: the guided branch pairs, the fork of the sub-batch streams, the paired schedule's
int loop_events(Loop& l, Events& ev, hipEvent_t* pev) {
    LoopPlan& p = l.p;
    for (int s = 0; p.branch_streams && s < p.nsub; ++s) {
        AFM_TRY(ev.make(&p.sb[s].x_ready));
        AFM_TRY(ev.make(&p.sb[s].u_ready));
    }
    hipEvent_t fork;
    if (p.nsub > 1) AFM_TRY(fork_streams(ev, (hipStream_t)l.c.a.stream, p.sb, p.nsub, &fork));
    for (int i = 0; p.paired && i < NEV; ++i) AFM_TRY(ev.make(&pev[i]));
    return 0;
}

// ticket words of the fused LayerNorm: zero once, every launch leaves them zero
int zero_ln_tickets(const Loop& l) {
    if (!(l.p.w.flags & AFM_CMDM_FUSED_LN)) return 0;
    const int T = 1 + l.p.w.n_cond + l.c.L;
    for (int s = 0; s < l.p.nsub; ++s) {
        const SubBatch& sb = l.p.sb[s];
        if (sb.count > 0 && hipMemsetAsync(sb.ws.lncnt, 0, (size_t)(((int64_t)sb.count * T + 31) / 32) * 4, sb.stream) != hipSuccess) return (int)hipGetLastError();
    }
    return 0;
}

int sample_loop_impl(const LoopCall& c) {
    Loop l{c, {}, {}};
    AFM_TRY(plan_loop(c, &l.p));
    if (l.p.nsub == 0) return 0;
    AFM_TRY(l.sched.expand(c.a));
    Events ev;                        // every return below releases what was created
    hipEvent_t pev[NEV] = {};
    AFM_TRY(loop_events(l, ev, pev));
    AFM_TRY(zero_ln_tickets(l));
    const std::unique_ptr<Recorder[]> recs(l.p.paired ? new Recorder[2] : nullptr);
    int rc = 0;
    for (int j = 0; j < c.a.n_steps && rc == 0; ++j) {
        if (l.p.paired && j > 0) { rc = paired_step(l, j, recs.get(), pev); continue; }
        for (int s = 0; s < l.p.nsub && rc == 0; ++s) {
            if (l.p.sb[s].count == 0) continue;
            rc = loop_step(l, l.p.sb[s], j);
        }
    }
    // (every branch stream's last work is joined to its sub-batch's stream before the last update)
    if (l.p.nsub > 1) join_streams(ev, (hipStream_t)c.a.stream, l.p.sb, l.p.nsub);
    return rc;
}

// the entries that run every form - 2M, guided by a term (`guide`), stitched (`stitch`): the separate-update loop of the form the rows
// and the guidance name, on a workspace with a history buffer; the 2M form draws no noise and takes no seed
int every_form_range(const afm_cmdm_weights* w, float* x, const float* cond_tokens, const uint8_t* frame_mask, const float* step_noise,
                     const int64_t* d_timestep_map, const afm_ddim_rows* rows, const afm_dpm_rows* dpm, const float* d_c1, const float* d_c2,
                     const float* d_sigma, const afm_cfg_args* cfg, const afm_cfg2_args* cfg2, const float* known, const uint8_t* mask,
                     const afm_motion_guide* guide, const afm_stitch* stitch, int32_t n_steps, int32_t first_step, uint64_t seed,
                     int64_t sample_index0, int32_t B, int32_t L, void* sched_scratch, void* workspace, int64_t workspace_bytes, int32_t n_streams,
                     void* const* side_streams, void* stream, const afm_long_guide* lguide = nullptr, const afm_scene_clearance* clear = nullptr,
                     const afm_foot_grounding* feet = nullptr) {
    if (first_step < 0 || (guide && !guide->contact && !guide->targets && !clear && !feet) || (cfg && cfg2) || !known != !mask) return AFM_E_BADARG;
    afm_ddim_rows as_ddim = {};
    AFM_TRY(one_kind_of_rows(&rows, dpm, d_c1 || d_c2 || d_sigma, &as_ddim));
    if ((dpm && step_noise) || (cfg2 && (!frame_mask || !cfg2_ok(cfg2)))) return AFM_E_BADARG;
    LoopCall c = loop_call(w, x, cond_tokens, frame_mask, step_noise, d_timestep_map, rows, d_c1, d_c2, d_sigma, n_steps, first_step, dpm ? 0 : seed,
                           dpm ? 0 : sample_index0, B, L, sched_scratch, workspace, workspace_bytes, n_streams, side_streams, stream, cfg, cfg2, known, mask);
    c.a.dpm = dpm != nullptr;
    if (guide) c.guide = *guide;
    if (stitch) c.stitch = *stitch;
    c.lguide = lguide;
    c.clear = clear;
    c.feet = feet;
    return sample_loop_impl(c);
}

}  // namespace

extern "C" int64_t afm_cmdm_loop_workspace_bytes(const afm_cmdm_weights* w, int32_t B, int32_t L, int32_t n_streams) {
    return loop_workspace_bytes(w, nullptr, nullptr, B, L, n_streams);
}

extern "C" int64_t afm_cmdm_cfg_loop_workspace_bytes(const afm_cmdm_weights* w, int32_t B, int32_t L, int32_t n_streams, const afm_cfg_args* cfg) {
    return cfg ? loop_workspace_bytes(w, cfg, nullptr, B, L, n_streams) : AFM_E_BADARG;
}

extern "C" int64_t afm_cmdm_cfg2_loop_workspace_bytes(const afm_cmdm_weights* w, int32_t B, int32_t L, int32_t n_streams, const afm_cfg2_args* cfg) {
    return cfg ? loop_workspace_bytes(w, nullptr, cfg, B, L, n_streams) : AFM_E_BADARG;
}

extern "C" int afm_cmdm_sample_loop(const afm_cmdm_weights* w, float* x, const float* cond_tokens, const uint8_t* frame_mask,
                                    const float* step_noise, const int64_t* d_timestep_map, const float* d_c1,
                                    const float* d_c2, const float* d_sigma, int32_t n_steps, uint64_t seed,
                                    int64_t sample_index0, int32_t B, int32_t L, void* sched_scratch, void* workspace,
                                    int64_t workspace_bytes, int32_t n_streams, void* const* side_streams, void* stream) {
    return sample_loop_impl(loop_call(w, x, cond_tokens, frame_mask, step_noise, d_timestep_map, nullptr, d_c1, d_c2, d_sigma, n_steps, 0, seed, sample_index0,
                                      B, L, sched_scratch, workspace, workspace_bytes, n_streams, side_streams, stream));
}

extern "C" int afm_cmdm_sample_loop_range(const afm_cmdm_weights* w, float* x, const float* cond_tokens,
                                          const uint8_t* frame_mask, const float* step_noise, const int64_t* d_timestep_map,
                                          const float* d_c1, const float* d_c2, const float* d_sigma, int32_t n_steps,
                                          int32_t first_step, uint64_t seed, int64_t sample_index0, int32_t B, int32_t L,
                                          void* sched_scratch, void* workspace, int64_t workspace_bytes, int32_t n_streams,
                                          void* const* side_streams, void* stream) {
    if (first_step < 0) return AFM_E_BADARG;
    return sample_loop_impl(loop_call(w, x, cond_tokens, frame_mask, step_noise, d_timestep_map, nullptr, d_c1, d_c2, d_sigma, n_steps, first_step, seed,
                                      sample_index0, B, L, sched_scratch, workspace, workspace_bytes, n_streams, side_streams, stream));
}

extern "C" int afm_cmdm_ddim_loop_range(const afm_cmdm_weights* w, float* x, const float* cond_tokens,
                                        const uint8_t* frame_mask, const float* step_noise, const int64_t* d_timestep_map,
                                        const afm_ddim_rows* rows, int32_t n_steps, int32_t first_step, uint64_t seed, int64_t sample_index0,
                                        int32_t B, int32_t L, void* sched_scratch, void* workspace, int64_t workspace_bytes, int32_t n_streams,
                                        void* const* side_streams, void* stream) {
    if (first_step < 0 || !rows) return AFM_E_BADARG;
    return sample_loop_impl(loop_call(w, x, cond_tokens, frame_mask, step_noise, d_timestep_map, rows, nullptr, nullptr, nullptr, n_steps, first_step, seed,
                                      sample_index0, B, L, sched_scratch, workspace, workspace_bytes, n_streams, side_streams, stream));
}

extern "C" int afm_cmdm_cfg_sample_loop_range(const afm_cmdm_weights* w, float* x, const float* cond_tokens,
                                              const uint8_t* frame_mask, const float* step_noise, const int64_t* d_timestep_map,
                                              const float* d_c1, const float* d_c2, const float* d_sigma, const afm_cfg_args* cfg, int32_t n_steps,
                                              int32_t first_step, uint64_t seed, int64_t sample_index0, int32_t B, int32_t L,
                                              void* sched_scratch, void* workspace, int64_t workspace_bytes, int32_t n_streams,
                                              void* const* side_streams, void* stream) {
    if (first_step < 0 || !cfg) return AFM_E_BADARG;
    return sample_loop_impl(loop_call(w, x, cond_tokens, frame_mask, step_noise, d_timestep_map, nullptr, d_c1, d_c2, d_sigma, n_steps, first_step, seed,
                                      sample_index0, B, L, sched_scratch, workspace, workspace_bytes, n_streams, side_streams, stream, cfg));
}

extern "C" int afm_cmdm_cfg_ddim_loop_range(const afm_cmdm_weights* w, float* x, const float* cond_tokens,
                                            const uint8_t* frame_mask, const float* step_noise, const int64_t* d_timestep_map,
                                            const afm_ddim_rows* rows, const afm_cfg_args* cfg, int32_t n_steps, int32_t first_step, uint64_t seed,
                                            int64_t sample_index0, int32_t B, int32_t L, void* sched_scratch, void* workspace, int64_t workspace_bytes,
                                            int32_t n_streams, void* const* side_streams, void* stream) {
    if (first_step < 0 || !rows || !cfg) return AFM_E_BADARG;
    return sample_loop_impl(loop_call(w, x, cond_tokens, frame_mask, step_noise, d_timestep_map, rows, nullptr, nullptr, nullptr, n_steps, first_step, seed,
                                      sample_index0, B, L, sched_scratch, workspace, workspace_bytes, n_streams, side_streams, stream, cfg));
}

extern "C" int afm_cmdm_impute_loop_range(const afm_cmdm_weights* w, float* x, const float* cond_tokens,
                                          const uint8_t* frame_mask, const float* step_noise, const int64_t* d_timestep_map,
                                          const afm_ddim_rows* rows, const float* d_c1, const float* d_c2, const float* d_sigma,
                                          const afm_cfg_args* cfg, const float* known, const uint8_t* mask, int32_t n_steps, int32_t first_step,
                                          uint64_t seed, int64_t sample_index0, int32_t B, int32_t L, void* sched_scratch, void* workspace,
                                          int64_t workspace_bytes, int32_t n_streams, void* const* side_streams, void* stream) {
    if (first_step < 0 || !known || !mask) return AFM_E_BADARG;
    return sample_loop_impl(loop_call(w, x, cond_tokens, frame_mask, step_noise, d_timestep_map, rows, d_c1, d_c2, d_sigma, n_steps, first_step, seed, sample_index0,
                                      B, L, sched_scratch, workspace, workspace_bytes, n_streams, side_streams, stream, cfg, nullptr, known, mask));
}

extern "C" int afm_cmdm_cfg2_loop_range(const afm_cmdm_weights* w, float* x, const float* cond_tokens,
                                        const uint8_t* frame_mask, const float* step_noise, const int64_t* d_timestep_map,
                                        const afm_ddim_rows* rows, const float* d_c1, const float* d_c2, const float* d_sigma,
                                        const afm_cfg2_args* cfg, const float* known, const uint8_t* mask, int32_t n_steps, int32_t first_step,
                                        uint64_t seed, int64_t sample_index0, int32_t B, int32_t L, void* sched_scratch, void* workspace,
                                        int64_t workspace_bytes, int32_t n_streams, void* const* side_streams, void* stream) {
    if (first_step < 0 || !frame_mask || !known != !mask || !cfg2_ok(cfg)) return AFM_E_BADARG;
    return sample_loop_impl(loop_call(w, x, cond_tokens, frame_mask, step_noise, d_timestep_map, rows, d_c1, d_c2, d_sigma, n_steps, first_step, seed, sample_index0,
                                      B, L, sched_scratch, workspace, workspace_bytes, n_streams, side_streams, stream, nullptr, cfg, known, mask));
}

// DPM-Solver++(2M): the eta = 0 DDIM loop's launches (pred_xstart stored, one update launch per sub-batch and step) with the 2M update and
// one history buffer per sub-batch.  The rows travel through the DDIM schedule layout as {a, b, c, unused}.
extern "C" int64_t afm_cmdm_dpm_loop_workspace_bytes(const afm_cmdm_weights* w, int32_t B, int32_t L, int32_t n_streams, const afm_cfg_args* cfg,
                                                     const afm_cfg2_args* cfg2) {
    if (cfg && cfg2) return AFM_E_BADARG;
    return loop_workspace_bytes(w, cfg, cfg2, B, L, n_streams, true);
}

extern "C" int afm_cmdm_dpm_loop_range(const afm_cmdm_weights* w, float* x, const float* cond_tokens, const uint8_t* frame_mask,
                                       const int64_t* d_timestep_map, const afm_dpm_rows* rows, const afm_cfg_args* cfg, const afm_cfg2_args* cfg2,
                                       const float* known, const uint8_t* mask, int32_t n_steps, int32_t first_step, int32_t B, int32_t L,
                                       void* sched_scratch, void* workspace, int64_t workspace_bytes, int32_t n_streams, void* const* side_streams, void* stream) {
    if (!rows) return AFM_E_BADARG;
    return every_form_range(w, x, cond_tokens, frame_mask, nullptr, d_timestep_map, nullptr, rows, nullptr, nullptr, nullptr, cfg, cfg2, known, mask, nullptr,
                            nullptr, n_steps, first_step, 0, 0, B, L, sched_scratch, workspace, workspace_bytes, n_streams, side_streams, stream);
}

// The contact-guided loop, every form behind one entry: the separate-update loop of the form the rows and the guidance name, with the two
// gradient launches in front of a guided step's evaluations and grad / gk in its update launch.  A 2M history buffer is always carved, so
// every form shares one workspace layout.
extern "C" int64_t afm_cmdm_guide_loop_workspace_bytes(const afm_cmdm_weights* w, int32_t B, int32_t L, int32_t n_streams, const afm_cfg_args* cfg,
                                                       const afm_cfg2_args* cfg2, const afm_contact_guide* guide) {
    if ((cfg && cfg2) || !guide) return AFM_E_BADARG;
    const afm_motion_guide sum = {guide, nullptr, nullptr, nullptr};
    return loop_workspace_bytes(w, cfg, cfg2, B, L, n_streams, true, &sum);
}

extern "C" int afm_cmdm_guide_loop_range(const afm_cmdm_weights* w, float* x, const float* cond_tokens, const uint8_t* frame_mask,
                                         const float* step_noise, const int64_t* d_timestep_map, const afm_ddim_rows* rows, const afm_dpm_rows* dpm,
                                         const float* d_c1, const float* d_c2, const float* d_sigma, const afm_cfg_args* cfg,
                                         const afm_cfg2_args* cfg2, const float* known, const uint8_t* mask, const afm_contact_guide* guide,
                                         int32_t n_steps, int32_t first_step, uint64_t seed, int64_t sample_index0, int32_t B, int32_t L,
                                         void* sched_scratch, void* workspace, int64_t workspace_bytes, int32_t n_streams, void* const* side_streams, void* stream) {
    if (!guide) return AFM_E_BADARG;
    const afm_motion_guide sum = {guide, nullptr, guide->gk, guide->frame_mask};
    return every_form_range(w, x, cond_tokens, frame_mask, step_noise, d_timestep_map, rows, dpm, d_c1, d_c2, d_sigma, cfg, cfg2, known, mask, &sum, nullptr,
                            n_steps, first_step, seed, sample_index0, B, L, sched_scratch, workspace, workspace_bytes, n_streams, side_streams, stream);
}

// The same loop with the sum of the contact and the joint-target guidance as its description (afm_motion_guide): the terms a step has
// reached are computed into the one gradient buffer, the targets' launch adding to what the contact term wrote.
extern "C" int64_t afm_cmdm_motion_guide_loop_workspace_bytes(const afm_cmdm_weights* w, int32_t B, int32_t L, int32_t n_streams, const afm_cfg_args* cfg,
                                                              const afm_cfg2_args* cfg2, const afm_motion_guide* guide) {
    if ((cfg && cfg2) || !guide) return AFM_E_BADARG;
    return loop_workspace_bytes(w, cfg, cfg2, B, L, n_streams, true, guide);
}

extern "C" int afm_cmdm_motion_guide_loop_range(const afm_cmdm_weights* w, float* x, const float* cond_tokens, const uint8_t* frame_mask,
                                                const float* step_noise, const int64_t* d_timestep_map, const afm_ddim_rows* rows,
                                                const afm_dpm_rows* dpm, const float* d_c1, const float* d_c2, const float* d_sigma,
                                                const afm_cfg_args* cfg, const afm_cfg2_args* cfg2, const float* known, const uint8_t* mask,
                                                const afm_motion_guide* guide, int32_t n_steps, int32_t first_step, uint64_t seed, int64_t sample_index0,
                                                int32_t B, int32_t L, void* sched_scratch, void* workspace, int64_t workspace_bytes, int32_t n_streams,
                                                void* const* side_streams, void* stream) {
    if (!guide) return AFM_E_BADARG;
    return every_form_range(w, x, cond_tokens, frame_mask, step_noise, d_timestep_map, rows, dpm, d_c1, d_c2, d_sigma, cfg, cfg2, known, mask, guide, nullptr,
                            n_steps, first_step, seed, sample_index0, B, L, sched_scratch, workspace, workspace_bytes, n_streams, side_streams, stream);
}

// The same loop with the scene clearance next to (or without) the two terms (afm_scene_guide): the clearance's launch adds to what the
// terms in front of it wrote.  The loop reads the description's own gk and frame_mask.
extern "C" int64_t afm_cmdm_scene_guide_loop_workspace_bytes(const afm_cmdm_weights* w, int32_t B, int32_t L, int32_t n_streams, const afm_cfg_args* cfg,
                                                             const afm_cfg2_args* cfg2, const afm_scene_guide* guide) {
    if ((cfg && cfg2) || !guide || (!guide->terms && !guide->clearance)) return AFM_E_BADARG;
    const afm_motion_guide sum = {guide->terms ? guide->terms->contact : nullptr, guide->terms ? guide->terms->targets : nullptr, guide->gk, guide->frame_mask};
    return loop_workspace_bytes(w, cfg, cfg2, B, L, n_streams, true, &sum, 1, nullptr, guide->clearance);
}

extern "C" int afm_cmdm_scene_guide_loop_range(const afm_cmdm_weights* w, float* x, const float* cond_tokens, const uint8_t* frame_mask,
                                               const float* step_noise, const int64_t* d_timestep_map, const afm_ddim_rows* rows,
                                               const afm_dpm_rows* dpm, const float* d_c1, const float* d_c2, const float* d_sigma,
                                               const afm_cfg_args* cfg, const afm_cfg2_args* cfg2, const float* known, const uint8_t* mask,
                                               const afm_scene_guide* guide, int32_t n_steps, int32_t first_step, uint64_t seed, int64_t sample_index0,
                                               int32_t B, int32_t L, void* sched_scratch, void* workspace, int64_t workspace_bytes, int32_t n_streams,
                                               void* const* side_streams, void* stream) {
    if (!guide || (!guide->terms && !guide->clearance)) return AFM_E_BADARG;
    const afm_motion_guide sum = {guide->terms ? guide->terms->contact : nullptr, guide->terms ? guide->terms->targets : nullptr, guide->gk, guide->frame_mask};
    return every_form_range(w, x, cond_tokens, frame_mask, step_noise, d_timestep_map, rows, dpm, d_c1, d_c2, d_sigma, cfg, cfg2, known, mask, &sum, nullptr,
                            n_steps, first_step, seed, sample_index0, B, L, sched_scratch, workspace, workspace_bytes, n_streams, side_streams, stream, nullptr,
                            guide->clearance);
}

// The same loop with the foot grounding behind (or without) the three terms (afm_ground_guide): the grounding's launch adds to what the
// terms in front of it wrote.  The loop reads the description's own gk and frame_mask.
namespace {
afm_motion_guide ground_sum(const afm_ground_guide* guide) {
    const afm_motion_guide* m = guide->terms ? guide->terms->terms : nullptr;
    return {m ? m->contact : nullptr, m ? m->targets : nullptr, guide->gk, guide->frame_mask};
}
}  // namespace

extern "C" int64_t afm_cmdm_ground_guide_loop_workspace_bytes(const afm_cmdm_weights* w, int32_t B, int32_t L, int32_t n_streams, const afm_cfg_args* cfg,
                                                              const afm_cfg2_args* cfg2, const afm_ground_guide* guide) {
    if ((cfg && cfg2) || !guide || (!guide->terms && !guide->feet)) return AFM_E_BADARG;
    const afm_motion_guide sum = ground_sum(guide);
    return loop_workspace_bytes(w, cfg, cfg2, B, L, n_streams, true, &sum, 1, nullptr, guide->terms ? guide->terms->clearance : nullptr, guide->feet);
}

extern "C" int afm_cmdm_ground_guide_loop_range(const afm_cmdm_weights* w, float* x, const float* cond_tokens, const uint8_t* frame_mask,
                                                const float* step_noise, const int64_t* d_timestep_map, const afm_ddim_rows* rows,
                                                const afm_dpm_rows* dpm, const float* d_c1, const float* d_c2, const float* d_sigma,
                                                const afm_cfg_args* cfg, const afm_cfg2_args* cfg2, const float* known, const uint8_t* mask,
                                                const afm_ground_guide* guide, int32_t n_steps, int32_t first_step, uint64_t seed, int64_t sample_index0,
                                                int32_t B, int32_t L, void* sched_scratch, void* workspace, int64_t workspace_bytes, int32_t n_streams,
                                                void* const* side_streams, void* stream) {
    if (!guide || (!guide->terms && !guide->feet)) return AFM_E_BADARG;
    const afm_motion_guide sum = ground_sum(guide);
    return every_form_range(w, x, cond_tokens, frame_mask, step_noise, d_timestep_map, rows, dpm, d_c1, d_c2, d_sigma, cfg, cfg2, known, mask, &sum, nullptr,
                            n_steps, first_step, seed, sample_index0, B, L, sched_scratch, workspace, workspace_bytes, n_streams, side_streams, stream, nullptr,
                            guide->terms ? guide->terms->clearance : nullptr, guide->feet);
}

// The stitched loop (afm_stitch: the batch is G * S windows of G long motions), every form behind one entry: the separate-update loop of
// the form the rows and the guidance name, its update launch the stitched one (the frames two windows share get one pred_xstart between
// the combine and the select).  Sub-batches are cut over long motions.  A 2M history buffer is always carved, so every form shares one
// workspace layout.
extern "C" int64_t afm_cmdm_stitch_loop_workspace_bytes(const afm_cmdm_weights* w, int32_t B, int32_t L, int32_t n_streams, const afm_cfg_args* cfg,
                                                        const afm_cfg2_args* cfg2, const afm_stitch* stitch) {
    if ((cfg && cfg2) || !stitch || stitch->windows < 1 || stitch->overlap < 0 || 2 * (int64_t)stitch->overlap > L) return AFM_E_BADARG;
    return loop_workspace_bytes(w, cfg, cfg2, B, L, n_streams, true, nullptr, stitch->windows);
}

extern "C" int afm_cmdm_stitch_loop_range(const afm_cmdm_weights* w, float* x, const float* cond_tokens, const uint8_t* frame_mask,
                                          const float* step_noise, const int64_t* d_timestep_map, const afm_ddim_rows* rows, const afm_dpm_rows* dpm,
                                          const float* d_c1, const float* d_c2, const float* d_sigma, const afm_cfg_args* cfg,
                                          const afm_cfg2_args* cfg2, const float* known, const uint8_t* mask, const afm_stitch* stitch,
                                          int32_t n_steps, int32_t first_step, uint64_t seed, int64_t sample_index0, int32_t B, int32_t L,
                                          void* sched_scratch, void* workspace, int64_t workspace_bytes, int32_t n_streams, void* const* side_streams, void* stream) {
    (void)seed; (void)sample_index0;          // (no noise is drawn)
    if (first_step < 0 || !stitch || stitch->windows < 1 || (cfg && cfg2) || !known != !mask) return AFM_E_BADARG;
    if (d_c1 || d_c2 || d_sigma || step_noise) return AFM_E_BADARG;          // DDPM rows, explicit step noise: the noise of shared frames would have to be shared
    if (rows && rows->sigma) return AFM_E_BADARG;          // a noise term (eta != 0)
    if (B < 0 || B % stitch->windows != 0 || stitch->overlap < 0 || 2 * (int64_t)stitch->overlap > L) return AFM_E_BADARG;
    return every_form_range(w, x, cond_tokens, frame_mask, nullptr, d_timestep_map, rows, dpm, nullptr, nullptr, nullptr, cfg, cfg2, known, mask, nullptr, stitch,
                            n_steps, first_step, 0, 0, B, L, sched_scratch, workspace, workspace_bytes, n_streams, side_streams, stream);
}

// The stitched loop guided on the joined long motions (afm_long_guide): the stitched loop above with the launches of afm_long_guidance in
// front of a guided step's evaluations and grad / gk in its stitched update launch.
extern "C" int64_t afm_cmdm_long_guide_loop_workspace_bytes(const afm_cmdm_weights* w, int32_t B, int32_t L, int32_t n_streams, const afm_cfg_args* cfg,
                                                            const afm_cfg2_args* cfg2, const afm_long_guide* guide) {
    if ((cfg && cfg2) || !guide || !w || afm_long_guide_check(guide, L, w->motion_dim) != 0) return AFM_E_BADARG;
    return loop_workspace_bytes(w, cfg, cfg2, B, L, n_streams, true, guide->terms, guide->stitch.windows, guide);
}

extern "C" int afm_cmdm_long_guide_loop_range(const afm_cmdm_weights* w, float* x, const float* cond_tokens, const uint8_t* frame_mask,
                                              const float* step_noise, const int64_t* d_timestep_map, const afm_ddim_rows* rows, const afm_dpm_rows* dpm,
                                              const float* d_c1, const float* d_c2, const float* d_sigma, const afm_cfg_args* cfg,
                                              const afm_cfg2_args* cfg2, const float* known, const uint8_t* mask, const afm_long_guide* guide,
                                              int32_t n_steps, int32_t first_step, uint64_t seed, int64_t sample_index0, int32_t B, int32_t L,
                                              void* sched_scratch, void* workspace, int64_t workspace_bytes, int32_t n_streams, void* const* side_streams, void* stream) {
    (void)seed; (void)sample_index0;          // (no noise is drawn)
    if (first_step < 0 || !guide || !guide->terms || guide->stitch.windows < 1 || (cfg && cfg2) || !known != !mask) return AFM_E_BADARG;
    if (d_c1 || d_c2 || d_sigma || step_noise || (rows && rows->sigma)) return AFM_E_BADARG;          // a deterministic update only
    if (B < 0 || B % guide->stitch.windows != 0) return AFM_E_BADARG;
    return every_form_range(w, x, cond_tokens, frame_mask, nullptr, d_timestep_map, rows, dpm, nullptr, nullptr, nullptr, cfg, cfg2, known, mask, guide->terms,
                            &guide->stitch, n_steps, first_step, 0, 0, B, L, sched_scratch, workspace, workspace_bytes, n_streams, side_streams, stream, guide);
}

// The same stitched loop with the scene clearance next to (or without) the long description's terms (afm_long_scene_guide): per window its
// own frames against its own cloud, crossfaded per long frame; its last launch adds to what the terms in front of it wrote.
extern "C" int64_t afm_cmdm_long_scene_guide_loop_workspace_bytes(const afm_cmdm_weights* w, int32_t B, int32_t L, int32_t n_streams,
                                                                  const afm_cfg_args* cfg, const afm_cfg2_args* cfg2,
                                                                  const afm_long_scene_guide* guide) {
    if ((cfg && cfg2) || !guide || !w || afm_long_scene_guide_check(guide->base, guide->clearance, L, w->motion_dim) != 0) return AFM_E_BADARG;
    return loop_workspace_bytes(w, cfg, cfg2, B, L, n_streams, true, guide->base->terms, guide->base->stitch.windows, guide->base, guide->clearance);
}

extern "C" int afm_cmdm_long_scene_guide_loop_range(const afm_cmdm_weights* w, float* x, const float* cond_tokens, const uint8_t* frame_mask,
                                                    const float* step_noise, const int64_t* d_timestep_map, const afm_ddim_rows* rows,
                                                    const afm_dpm_rows* dpm, const float* d_c1, const float* d_c2, const float* d_sigma,
                                                    const afm_cfg_args* cfg, const afm_cfg2_args* cfg2, const float* known, const uint8_t* mask,
                                                    const afm_long_scene_guide* guide, int32_t n_steps, int32_t first_step, uint64_t seed,
                                                    int64_t sample_index0, int32_t B, int32_t L, void* sched_scratch, void* workspace,
                                                    int64_t workspace_bytes, int32_t n_streams, void* const* side_streams, void* stream) {
    (void)seed; (void)sample_index0;          // (no noise is drawn)
    if (first_step < 0 || !guide || !guide->base || !guide->base->terms || guide->base->stitch.windows < 1 || (cfg && cfg2) || !known != !mask)
        return AFM_E_BADARG;
    if (d_c1 || d_c2 || d_sigma || step_noise || (rows && rows->sigma)) return AFM_E_BADARG;          // a deterministic update only
    if (B < 0 || B % guide->base->stitch.windows != 0) return AFM_E_BADARG;
    return every_form_range(w, x, cond_tokens, frame_mask, nullptr, d_timestep_map, rows, dpm, nullptr, nullptr, nullptr, cfg, cfg2, known, mask,
                            guide->base->terms, &guide->base->stitch, n_steps, first_step, 0, 0, B, L, sched_scratch, workspace, workspace_bytes, n_streams,
                            side_streams, stream, guide->base, guide->clearance);
}
