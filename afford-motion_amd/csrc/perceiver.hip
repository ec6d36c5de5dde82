// CDM / ContactPerceiver denoiser (reference models/cdm.py:155-188,474-513; Perceiver-IO blocks of
// models/modules.py:234-661).
//
// Per sample: N = 8192 points x 256 channels on the key/value side, but only TWO latent queries.
//   latent_token : (hoisted: once per text / once per timestep) enc_q0 row = adapter(input), q = q_proj(LN(enc_q0)) and the
//                  FOLDED queries u[h] = W_k[h]^T q[h] (8 vectors of 256 per latent), c[h] = q[h].b_k[h]
//   (afm_linear) : enc_kv = encoder_adapter(feat)                                         [B*N, 256]
//   enc_reduce   : flash-style reduction over the points: scores = LN_kv(enc_kv).u + c, online softmax,
//                  s[i,h] = sum_n a_n LN_kv(enc_kv_n)  -> per-wave partials (m, l, s)   (K / V never exist)
//   latent_post  : combine partials, o = W_v s + b_v, o_proj, residual, MLP, 2 self-attention layers on the 2
//                  latents, then the decoder's folded keys/values G[j,h] = W_q[h]^T k[j,h], P[j,h] = W_o[:,h] v[j,h]
//   (afm_linear) : dec_q0 = decoder_adapter(enc_kv)                                        [B*N, 256]
//   dec_attend   : per point: qn = LN(dec_q0); 16 scores qn.G + cb; softmax over the 2 keys per head; attention
//                  output = sum a P + b_o; + residual; LN of the MLP -> h1, z
//   (afm_linear) : t = GELU(fc1 z), h2 = fc2 t + h1, out = contact_layer h2 (+ fused DDPM update)
// The three dense 256x256 per-point layers are the FLOPs (103 of the 115 GFLOP/step folded work at B = 32)
// and run on the f32-MFMA GEMM; the kernels here are streaming / latency kernels (one wave per point).
//
// This file: the C-ABI entry points (include/afm_hip.h: afm_cdm_*), the workspace, the latent-token kernel (off the per-step path), the choice
// of the sampling form and the forward / native-loop drivers.  The kernels of a step live in perceiver_rows.hip (forms that read per-point
// rows: layer by layer, FOLD), perceiver_points.hip (the row-less form of the sampling loop) and perceiver_chain.hip (the latent chain).
#include "perceiver_internal.h"
#include "sample_loop.h"

extern "C" int afm_linear(const afm_linear_args*, void*);

using namespace afm_cdm;
using namespace afm_loop;

namespace {

// ---------------------------------------------------------------- small device helpers (latent kernels)
// out[tok][o] = b[o] + sum_k W[o][k] * in[tok][k]   for 2 tokens.  Each wave takes 4 output rows at a time
// (8 independent accumulators, float4 weight loads in flight for all 4 rows) and finishes them with ONE
// 8-value halving reduction.  ind must be a multiple of 4; W rows 16-byte aligned.
__device__ void matvec2(const float* __restrict__ W, const float* __restrict__ b, const float* in, float* out, int outd, int ind,
                        int in_stride, int out_stride) {
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63, nw = blockDim.x >> 6;
    for (int o0 = wave * 4; o0 < outd; o0 += nw * 4) {
        float a[8];
#pragma unroll
        for (int i = 0; i < 8; ++i) a[i] = 0.f;
        for (int k = lane * 4; k < ind; k += 256) {
            const float4 x0 = *reinterpret_cast<const float4*>(in + k);
            const float4 x1 = *reinterpret_cast<const float4*>(in + in_stride + k);
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int o = min(o0 + r, outd - 1);
                const float4 wv = *reinterpret_cast<const float4*>(W + (int64_t)o * ind + k);
                a[r] += (wv.x * x0.x + wv.y * x0.y) + (wv.z * x0.z + wv.w * x0.w);
                a[4 + r] += (wv.x * x1.x + wv.y * x1.y) + (wv.z * x1.z + wv.w * x1.w);
            }
        }
        const float tot = wave_reduce_multi<8>(a, lane);
        if ((lane & 7) == 0) {                       // one lane per owned index: idx = tok * 4 + r
            const int idx = multi_owned_index<8>(lane), tok = idx >> 2, o = o0 + (idx & 3);
            if (o < outd) out[tok * out_stride + o] = tot + (b ? b[o] : 0.f);
        }
    }
}

// LayerNorm of 2 tokens (waves 0 and 1), eps 1e-5
__device__ void ln2(const float* in, float* out, afm_ln p, int dim, int stride) {
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    if (wave < 2) {
        const float* x = in + wave * stride;
        float s = 0.f;
        for (int k = lane; k < dim; k += 64) s += x[k];
        const float mean = wave_sum(s) / dim;
        float q = 0.f;
        for (int k = lane; k < dim; k += 64) { const float d = x[k] - mean; q += d * d; }
        const float rstd = 1.0f / sqrtf(wave_sum(q) / dim + 1e-5f);
        for (int k = lane; k < dim; k += 64) out[wave * stride + k] = (x[k] - mean) * rstd * p.g[k] + p.b[k];
    }
}

// ---------------------------------------------------------------- latent_token
// One latent token per workgroup (grid = number of tokens, block 1024): adapter -> enc_q0 row, LN_q, q_proj, dp_scale,
// and the folded queries u[h][c] = sum_r W_k[h*hd + r][c] q[h*hd + r], cu[h] = q_h . b_k[h].
// Both latents are per-step invariant given their input: the text token depends on the sample's text only (once per
// sampling run) and the time token on t only (tabulated for every timestep when the weights are packed), so this
// kernel is OFF the per-step path; the per-step kernels gather its outputs.
__global__ __launch_bounds__(1024) void latent_token_kernel(const afm_cdm_weights w, const float* __restrict__ in, int in_dim,
                                                           afm_lin adapter, float* __restrict__ q0_out, float* __restrict__ u_out,
                                                           float* __restrict__ cu_out) {
    __shared__ __attribute__((aligned(16))) float vin[2][MAXD], q0[2][MAXD], qn[2][MAXD], q[2][MAXD];
    const int tok = blockIdx.x, dq = w.dq, dkv = w.dkv, He = w.enc_heads, hd = dq / He;
    for (int i = threadIdx.x; i < MAXD; i += blockDim.x) { vin[0][i] = i < in_dim ? in[(int64_t)tok * in_dim + i] : 0.f; vin[1][i] = 0.f; }
    __syncthreads();
    matvec2(adapter.w, adapter.b, &vin[0][0], &q0[0][0], dq, in_dim, MAXD, MAXD);      // row 1 is a dummy token
    __syncthreads();
    for (int i = threadIdx.x; i < dq; i += blockDim.x) q0_out[(int64_t)tok * dq + i] = q0[0][i];
    ln2(&q0[0][0], &qn[0][0], w.enc_q_norm, dq, MAXD);
    __syncthreads();
    matvec2(w.enc_attn.q.w, w.enc_attn.q.b, &qn[0][0], &q[0][0], dq, dq, MAXD, MAXD);
    __syncthreads();
    const float scale = 1.0f / sqrtf((float)hd);                                          // q * dp_scale (modules.py:330)
    for (int e = threadIdx.x; e < He * dkv; e += blockDim.x) {
        const int h = e / dkv, c = e % dkv;
        float acc = 0.f;
        for (int r = 0; r < hd; ++r) acc += w.enc_attn.k.w[(int64_t)(h * hd + r) * dkv + c] * (q[0][h * hd + r] * scale);
        u_out[((int64_t)tok * He + h) * dkv + c] = acc;
    }
    for (int h = threadIdx.x; h < He; h += blockDim.x) {
        float acc = 0.f;
        for (int r = 0; r < hd; ++r) acc += w.enc_attn.k.b[h * hd + r] * (q[0][h * hd + r] * scale);
        cu_out[(int64_t)tok * He + h] = acc;
    }
}

// rows = false (the native loop in the row-less sampling form): the four [B N, dkv] row buffers and the folded form's per-point scratch are
// never touched and are not carved (about 1 GB at B = 32, N = 8192)
CdmWs carve(const afm_cdm_weights& w, int B, int N, void* base, bool rows = true) {
    char* p = (char*)base;
    int64_t off = 0;
    auto take = [&](int64_t n) { char* r = p ? p + off : nullptr; off += align256(n); return (float*)r; };
    const int64_t M = (int64_t)B * N, nih = 2 * w.enc_heads, njh = 2 * w.dec_heads;
    CdmWs s;
    const int64_t Mr = rows ? M : 0;
    s.enc_kv = take(Mr * w.dkv * 4); s.bufB = take(Mr * w.dkv * 4); s.h1 = take(Mr * w.dkv * 4); s.z = take(Mr * w.dkv * 4);
    s.pm = take((int64_t)B * NPART * nih * 4); s.pl = take((int64_t)B * NPART * nih * 4);
    s.pacc = take((int64_t)B * NPART * nih * w.dkv * 4);
    s.dec_lat = take((int64_t)B * DEC_LAT_STRIDE(njh) * 4);
    s.s1 = take(Mr * 8 * 4);                                 // folded path: contact_layer . h1 per point (<= 8 channels)
    s.rdot = take(Mr * (w.dkv / 64) * 8 * 4);                // folded path: row-dot partials of the fc1 GEMM
    s.qe = take(Mr * 8 * 4);                                 // folded path: contact_layer . (step-invariant part of the decoder query)
    const int64_t ntok = 2 * (int64_t)B;
    s.lat_s = take(ntok * w.enc_heads * w.dkv * 4); s.lat_x = take(ntok * w.dq * 4); s.lat_t1 = take(ntok * w.dq * 4);
    s.lat_t2 = take(ntok * w.dq * 4); s.lat_qkv = take(ntok * 3 * w.dq * 4); s.lat_kv = take(ntok * 2 * w.dkv * 4);
    s.twp = take((int64_t)B * 16 * 256 * 4); s.qtab = take((int64_t)B * RowLess<11>::TAB * 4);
    s.bytes = off;
    return s;
}

int validate(const afm_cdm_weights* w, int B, int N) {
    if (!w || B < 0 || N <= 0) return AFM_E_BADARG;
    if (w->dkv != 256 || w->dq <= 0 || w->dq > MAXD || (w->dq & 3) || w->text_dim > MAXD || w->time_dim > MAXD) return AFM_E_UNSUPPORTED;
    if (w->enc_heads != 8 || w->dec_heads != 8 || w->n_self < 0 || w->n_self > 4) return AFM_E_UNSUPPORTED;
    if (w->feat_dim <= 0 || w->contact_dim <= 0 || w->n_timesteps <= 0) return AFM_E_BADARG;
    // the batched latent chain: one wave per 16 tokens x 16 outputs (a head's outputs are whole tiles)
    if ((w->dq % 128) != 0 || (w->dq / w->enc_heads) % TL_OB != 0) return AFM_E_UNSUPPORTED;
    return 0;
}
}  // namespace

extern "C" int64_t afm_cdm_workspace_bytes(const afm_cdm_weights* w, int32_t B, int32_t N) {
    if (validate(w, B, N) != 0) return AFM_E_BADARG;
    return carve(*w, B, N, nullptr).bytes;
}

extern "C" int afm_cdm_latent_tokens(const afm_cdm_weights* wp, int32_t which, const float* in, int32_t n, float* q0_out,
                                     float* u_out, float* cu_out, void* stream) {
    AFM_TRY(validate(wp, 0, 1));
    if (!in || !q0_out || !u_out || !cu_out || n < 0 || (which != 0 && which != 1)) return AFM_E_BADARG;
    if (n == 0) return 0;
    const afm_cdm_weights& w = *wp;
    const int in_dim = which == 0 ? w.text_dim : w.time_dim;
    if (in_dim & 3) return AFM_E_UNSUPPORTED;
    AfmProf prof(AFM_PROF_CDM, 0.0, (hipStream_t)stream);
    hipLaunchKernelGGL(latent_token_kernel, dim3(n), dim3(1024), 0, (hipStream_t)stream, w, in, in_dim,
                       which == 0 ? w.language_adapter : w.time_embedding_adapter, q0_out, u_out, cu_out);
    AFM_CHECK_LAUNCH();
    return 0;
}
namespace {

// sampling form of the per-point kernels: 3 = no rows (enc_point_kernel, lat_head_kernel, lat_dectables_kernel, dec_point_kernel: every fused
// table present and rowless_nks(feat_dim) != 0: at most 43 input channels), 1 = FOLD (round 2: step-invariant adapter parts materialised once per loop), 0 = layer by layer
inline int cdm_mode(const afm_cdm_weights& w) {
    const bool folded = w.fold_xu && w.fold_xv && w.fold_w2 && w.fold_q && w.fold_c0 && w.contact_dim <= 8 && w.feat_dim > w.contact_dim && (w.dkv % 64) == 0;
    if (!folded) return 0;
    const bool fused = w.gen_qe && w.dec_c && w.dec_twx && w.dec_qxx && w.dec_qdd && w.enc_ec && w.enc_qee && w.enc_wove && w.enc_c1 && w.dec_dwq && w.dec_wqb &&
                       w.dec_wco && w.dec_wow && w.dec_wog && w.dec_xwo && rowless_nks(w.feat_dim) != 0 && w.enc_heads == 8 && w.dec_heads == 8 && w.dkv == 256 &&
                       !(w.flags & AFM_CDM_NO_GEN);
    return fused ? 3 : 1;
}
inline bool cdm_folded(const afm_cdm_weights& w) { return cdm_mode(w) != 0; }

// the step-invariant parts of the two adapters: C = encoder_adapter(input with x = 0) -> ws.enc_kv, D = decoder_adapter(C) -> ws.bufB
int cdm_prepare_invariants(const afm_cdm_weights& w, const float* feat, int B, int N, const CdmWs& ws, hipStream_t s) {
    const int M = B * N, dkv = w.dkv, cd = w.contact_dim;
    afm_linear_args a = {};
    a.A = feat + cd; a.lda = w.feat_dim; a.W = w.encoder_adapter.w + cd; a.ldw = w.feat_dim; a.C = ws.enc_kv; a.ldc = dkv;
    a.M = M; a.N = dkv; a.K = w.feat_dim - cd; a.bias = w.encoder_adapter.b;
    a.arith = w.gemm_arith; a.arith_min_n = w.gemm_arith_min_n;
    AFM_TRY(afm_linear(&a, s));
    a = {};
    a.A = ws.enc_kv; a.lda = dkv; a.W = w.decoder_adapter.w; a.ldw = dkv; a.C = ws.bufB; a.ldc = dkv;
    a.M = M; a.N = dkv; a.K = dkv; a.bias = w.decoder_adapter.b;
    a.arith = w.gemm_arith; a.arith_min_n = w.gemm_arith_min_n;
    AFM_TRY(afm_linear(&a, s));
    a = {};                                  // E = contact_layer.w . D: the step-invariant part of what the output layer sees of the query
    a.A = ws.bufB; a.lda = dkv; a.W = w.contact_layer.w; a.ldw = dkv; a.C = ws.qe; a.ldc = cd;
    a.M = M; a.N = cd; a.K = dkv;
    a.arith = w.gemm_arith; a.arith_min_n = w.gemm_arith_min_n;
    return afm_linear(&a, s);
}

// one denoiser evaluation in the folded (mode 1) or generated (mode 2) form; `prepared` (mode 1): ws.enc_kv / ws.bufB already hold C / D
int cdm_forward_folded(const afm_cdm_weights& w, const float* feat, const float* x_t, const int64_t* t, const float* text_q0,
                       const float* text_u, const float* text_cu, float* x0_out, const afm_ddpm_args* ddpm, int B, int N, const CdmWs& ws,
                       bool prepared, hipStream_t s, const CdmChainSide* cs = nullptr, const Update* loop_upd = nullptr) {
    const int M = B * N, dkv = w.dkv, cd = w.contact_dim, mode = cdm_mode(w);
    // the imputing loops: known / mask of the sub-batch ride in the loop's update description (row-less: fused into dec_point; FOLD: below)
    const float* known = loop_upd ? loop_upd->known : nullptr;
    const uint8_t* mask = loop_upd ? loop_upd->mask : nullptr;
    // the 2M loop: the sub-batch's history rides there too (row-less: fused into dec_point; FOLD: the update launch below)
    const float* x0_prev = loop_upd ? loop_upd->x0_prev : nullptr;
    float* x0_keep = loop_upd ? loop_upd->x0_keep : nullptr;
    if (mode == 1 && !prepared) AFM_TRY(cdm_prepare_invariants(w, feat, B, N, ws, s));
    if (mode == 3) AFM_TRY(launch_enc_point(w, text_u, text_cu, t, B, N, ws, x_t, feat, s));
    else AFM_TRY(launch_enc_reduce(w, ws.enc_kv, text_u, text_cu, t, B, N, ws, x_t, mode, s));
    if (mode == 3 && cs && cs->chain) {
        // the chain (13 small launches for 2 B tokens) on the sub-batch's side stream: enc_point -> [event] -> chain + tables -> [event] -> dec_point
        (void)hipEventRecord(cs->forked, s);
        (void)hipStreamWaitEvent(cs->chain, cs->forked, 0);
        AFM_TRY(cdm_latent_chain(w, text_q0, t, ws, B, cs->chain, true));
        AFM_TRY(launch_dec_tables(w, B, ws, cs->chain));
        (void)hipEventRecord(cs->joined, cs->chain);
        (void)hipStreamWaitEvent(s, cs->joined, 0);
        return launch_dec_point(w, B, N, ws, x_t, feat, x0_out, ddpm, s, false, known, mask, x0_prev, x0_keep);
    }
    AFM_TRY(cdm_latent_chain(w, text_q0, t, ws, B, s, mode == 3));
    if (mode == 3) return launch_dec_point(w, B, N, ws, x_t, feat, x0_out, ddpm, s, true, known, mask, x0_prev, x0_keep);
    AFM_TRY(launch_dec_attend(w, B, N, ws, x_t, mode, s));
    afm_linear_args a = {};                 // GELU(linear1 z) . w2 per 64-column group; the hidden activations are never stored
    a.A = ws.z; a.lda = dkv; a.W = w.dec_mlp.fc1.w; a.ldw = dkv; a.M = M; a.N = dkv; a.K = dkv; a.bias = w.dec_mlp.fc1.b; a.act = AFM_ACT_GELU;
    a.rowdot_w = w.fold_w2; a.rowdot_out = ws.rdot; a.rowdot_n = cd;
    a.arith = w.gemm_arith; a.arith_min_n = w.gemm_arith_min_n;
    a.tune = ((w.flags >> AFM_CDM_TILE_SHIFT) & 0xF) << AFM_TUNE_TILE_SHIFT;
    AFM_TRY(afm_linear(&a, s));
    if (mask || x0_keep) {       // imputing loop and 2M loop, FOLD: pred_xstart to ws.h1 (not used by this form) with the plain output, then the one update
                                 // launch that selects (and, 2M, reads and writes the history)
        AFM_TRY(launch_cdm_output(w, B, N, ws, x_t, ws.h1, nullptr, s));
        Update u = *loop_upd;
        u.x0 = ws.h1;
        return afm_sampling_update(u, B, s);
    }
    return launch_cdm_output(w, B, N, ws, x_t, x0_out, ddpm, s);
}

}  // namespace

static int cdm_forward_impl(const afm_cdm_weights* wp, const float* feat, const float* x_t, const int64_t* t,
                            const float* text_q0, const float* text_u, const float* text_cu, float* x0_out,
                            const afm_ddpm_args* ddpm, int32_t B, int32_t N, void* workspace, int64_t workspace_bytes,
                            void* side_stream, void* stream, bool prepared = false, bool rowless_ws = false, const CdmChainSide* cs = nullptr,
                            const afm_loop::Update* loop_upd = nullptr) {      // loop_upd: the update launch of a loop step (the layer-by-layer DDIM loop's;
                                                                              // an imputing loop's, known / mask set), its x0 set here
    AFM_TRY(validate(wp, B, N));
    if (!feat || !t || !text_q0 || !text_u || !text_cu || !workspace || (!x0_out && !ddpm)) return AFM_E_BADARG;
    if (!wp->time_q0 || !wp->time_u || !wp->time_cu) return AFM_E_BADARG;
    if (ddpm && (!ddpm->x_next || !ddpm->c1 || !ddpm->c2 || !ddpm->sigma || !ddpm->noise || !x_t)) return AFM_E_BADARG;
    if (B == 0) return 0;
    const afm_cdm_weights& w = *wp;
    hipStream_t s = (hipStream_t)stream;
    if (rowless_ws && !(cdm_mode(w) == 3 && x_t)) return AFM_E_BADARG;          // a workspace without row buffers serves the row-less form only
    const CdmWs ws = carve(w, B, N, workspace, !rowless_ws);
    if (ws.bytes > workspace_bytes) return AFM_E_WORKSPACE;
    const int M = B * N, dkv = w.dkv;
    if (loop_upd && (loop_upd->mask || loop_upd->x0_keep) && !ddpm) return AFM_E_BADARG;
    if (cdm_folded(w) && x_t) return cdm_forward_folded(w, feat, x_t, t, text_q0, text_u, text_cu, x0_out, ddpm, B, N, ws, prepared, s, cs, loop_upd);

    afm_linear_args a = {};
    a.A = feat; a.lda = w.feat_dim; a.W = w.encoder_adapter.w; a.ldw = w.feat_dim; a.C = ws.enc_kv; a.ldc = dkv;
    a.M = M; a.N = dkv; a.K = w.feat_dim; a.bias = w.encoder_adapter.b;
    a.arith = w.gemm_arith; a.arith_min_n = w.gemm_arith_min_n;
    AFM_TRY(afm_linear(&a, s));
    // The decoder adapter GEMM (34 GFLOP at B = 32) only needs enc_kv, while the latent chain (enc_reduce -> latent_post: one
    // workgroup per SAMPLE, a serial 0.5 ms dependency chain that leaves the chip idle) only produces the 2 latent tokens:
    // with a side stream the GEMM runs under the latent chain and the two join in front of dec_attend.
    hipStream_t side = (hipStream_t)side_stream;
    hipEvent_t ev_fork = nullptr, ev_join = nullptr;
    AFM_TRY(launch_enc_reduce(w, ws.enc_kv, text_u, text_cu, t, B, N, ws, nullptr, 0, s));
    if (side) {           // fork AFTER enc_reduce (a full-chip kernel): the GEMM shares the chip with latent_post only
        if (hipEventCreateWithFlags(&ev_fork, hipEventDisableTiming) != hipSuccess ||
            hipEventCreateWithFlags(&ev_join, hipEventDisableTiming) != hipSuccess) return (int)hipGetLastError();
        (void)hipEventRecord(ev_fork, s);
    }
    AFM_TRY(cdm_latent_chain(w, text_q0, t, ws, B, s, false));
    if (side) {           // enqueued after latent_post so that its 32 workgroups get their CUs first
        (void)hipStreamWaitEvent(side, ev_fork, 0);
        afm_linear_args d = {};
        d.A = ws.enc_kv; d.lda = dkv; d.W = w.decoder_adapter.w; d.ldw = dkv; d.C = ws.bufB; d.ldc = dkv;
        d.M = M; d.N = dkv; d.K = dkv; d.bias = w.decoder_adapter.b;
        d.arith = w.gemm_arith; d.arith_min_n = w.gemm_arith_min_n;
        const int rc = afm_linear(&d, side);
        (void)hipEventRecord(ev_join, side);
        if (rc) { (void)hipEventDestroy(ev_fork); (void)hipEventDestroy(ev_join); return rc; }
    }
    if (side) {
        (void)hipStreamWaitEvent(s, ev_join, 0);
        (void)hipEventDestroy(ev_fork); (void)hipEventDestroy(ev_join);
    } else {
        a = {};
        a.A = ws.enc_kv; a.lda = dkv; a.W = w.decoder_adapter.w; a.ldw = dkv; a.C = ws.bufB; a.ldc = dkv;
        a.M = M; a.N = dkv; a.K = dkv; a.bias = w.decoder_adapter.b;
        a.arith = w.gemm_arith; a.arith_min_n = w.gemm_arith_min_n;
    AFM_TRY(afm_linear(&a, s));
    }
    AFM_TRY(launch_dec_attend(w, B, N, ws, nullptr, 0, s));
    a = {};
    a.A = ws.z; a.lda = dkv; a.W = w.dec_mlp.fc1.w; a.ldw = dkv; a.C = ws.bufB; a.ldc = dkv;
    a.M = M; a.N = dkv; a.K = dkv; a.bias = w.dec_mlp.fc1.b; a.act = AFM_ACT_GELU;
    a.arith = w.gemm_arith; a.arith_min_n = w.gemm_arith_min_n;
    AFM_TRY(afm_linear(&a, s));
    a = {};
    a.A = ws.bufB; a.lda = dkv; a.W = w.dec_mlp.fc2.w; a.ldw = dkv; a.C = ws.z; a.ldc = dkv;
    a.M = M; a.N = dkv; a.K = dkv; a.bias = w.dec_mlp.fc2.b; a.residual = ws.h1; a.ldr = dkv;
    a.arith = w.gemm_arith; a.arith_min_n = w.gemm_arith_min_n;
    AFM_TRY(afm_linear(&a, s));
    a = {};
    a.A = ws.z; a.lda = dkv; a.W = w.contact_layer.w; a.ldw = dkv; a.C = x0_out; a.ldc = w.contact_dim;
    a.M = M; a.N = w.contact_dim; a.K = dkv; a.bias = w.contact_layer.b;
    const int upd = ddpm ? cdm_update_bits(w) : 0;
    if ((upd & AFM_UPD_DDIM) || (loop_upd && loop_upd->mask)) {       // native DDIM loop, and every imputing loop (the fused DDPM epilogue has no
                                    // place for the select): pred_xstart to bufB (read by nothing after fc2), then the update in place on x_t
        if (dkv < w.contact_dim) return AFM_E_UNSUPPORTED;          // (bufB holds [M][dkv]; pred_xstart needs [M][contact_dim])
        a.C = ws.bufB;
        a.arith = w.gemm_arith; a.arith_min_n = w.gemm_arith_min_n;
        AFM_TRY(afm_linear(&a, s));
        if (!loop_upd) return AFM_E_BADARG;
        Update u = *loop_upd;
        u.x0 = ws.bufB;
        return afm_sampling_update(u, B, s);
    }
    if (ddpm) {
        a.ddpm_xt = x_t; a.ddpm_noise = ddpm->noise; a.ddpm_out = ddpm->x_next; a.ldx = w.contact_dim;
        a.ddpm_c1 = ddpm->c1; a.ddpm_c2 = ddpm->c2; a.ddpm_sigma = ddpm->sigma; a.rows_per_sample = N;
        a.ddpm_clip = (w.flags & AFM_CDM_CLIP_X0) ? 1 : 0;
    }
    a.arith = w.gemm_arith; a.arith_min_n = w.gemm_arith_min_n;
    AFM_TRY(afm_linear(&a, s));
    return 0;
}

extern "C" int afm_cdm_forward(const afm_cdm_weights* wp, const float* feat, const float* x_t, const int64_t* t,
                               const float* text_q0, const float* text_u, const float* text_cu, float* x0_out,
                               const afm_ddpm_args* ddpm, int32_t B, int32_t N, void* workspace, int64_t workspace_bytes,
                               void* stream) {
    afm_cdm_weights wpub;
    if (wp && (wp->flags & (AFM_PRIV_DDIM | AFM_PRIV_NO_NOISE))) { wpub = *wp; wpub.flags &= ~(AFM_PRIV_DDIM | AFM_PRIV_NO_NOISE); wp = &wpub; }      // library-private bits
    return cdm_forward_impl(wp, feat, x_t, t, text_q0, text_u, text_cu, x0_out, ddpm, B, N, workspace, workspace_bytes, nullptr, stream);
}

extern "C" int afm_cdm_forward_overlap(const afm_cdm_weights* wp, const float* feat, const float* x_t, const int64_t* t,
                                       const float* text_q0, const float* text_u, const float* text_cu, float* x0_out,
                                       const afm_ddpm_args* ddpm, int32_t B, int32_t N, void* workspace, int64_t workspace_bytes,
                                       void* side_stream, void* stream) {
    afm_cdm_weights wpub;
    if (wp && (wp->flags & (AFM_PRIV_DDIM | AFM_PRIV_NO_NOISE))) { wpub = *wp; wpub.flags &= ~(AFM_PRIV_DDIM | AFM_PRIV_NO_NOISE); wp = &wpub; }      // library-private bits
    return cdm_forward_impl(wp, feat, x_t, t, text_q0, text_u, text_cu, x0_out, ddpm, B, N, workspace, workspace_bytes, side_stream, stream);
}

// ------------------------------------------------------------------------------------------------ native sampling loop
namespace {

// feat[r, 0:cd] = x[r, :]  (the noisy contact map is the leading block of the encoder input, cdm.py:167-171)
__global__ __launch_bounds__(256) void pack_x_kernel(const float* __restrict__ x, float* __restrict__ feat, int64_t rows, int cd, int fd) {
    const int64_t n = rows * cd;
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (int64_t)gridDim.x * 256) {
        const int64_t r = i / cd;
        feat[r * fd + (i - r * cd)] = x[i];
    }
}

constexpr int MAX_SUB = 8;            // sub-batches (stream pairs) of one loop call

// the arguments of the three loop entry points
struct LoopCall {
    const afm_cdm_weights* w;
    float *x, *feat;
    const float *text_q0, *text_u, *text_cu;
    int N;
    LoopArgs a;                       // (a.streams: a stream pair per sub-batch)
    const float* known = nullptr;     // imputing loop: [B][N][contact_dim] each, both set (neither: no imputation)
    const uint8_t* mask = nullptr;
};

// sub-batch s runs on `stream` (streams[2s]) with `side` (streams[2s+1]) as the side stream of its decoder-adapter GEMM, of its latent chain
// (AFM_CDM_CHAIN_SIDE, AFM_CDM_PIPELINE); n_sub <= 1: everything on the caller's stream, streams[0] = optional side stream
struct SubBatch : SubRange {
    hipStream_t side;
    char* base;                       // the sub-batch's workspace: ws, then the noise
    CdmWs ws;
    float* noise;                     // NOISE_STEPS steps of noise, behind ws
    // AFM_CDM_CHAIN_SIDE: one event pair per sub-batch, reused by every step (an event re-recorded on a stream orders behind the waits
    // already enqueued on its previous record)
    CdmChainSide chain;
    hipEvent_t enc_done, tables_done; // AFM_CDM_PIPELINE: enc_point -> [enc_done] -> chain + tables -> [tables_done] -> dec_point
    float* hist;                      // 2M loop only: the previous step's final x0 [count][N * contact_dim], behind the noise
};

// carves the workspace of a sub-batch whose range is set at `base` (NULL: sizes only); -> its bytes
int64_t carve_sub(const afm_cdm_weights& w, int N, char* base, SubBatch* sb, bool hist = false) {
    sb->base = base;
    sb->ws = carve(w, sb->count, N, base, cdm_mode(w) != 3);
    sb->noise = base ? (float*)(base + sb->ws.bytes) : nullptr;
    int64_t off = sb->ws.bytes + align256((int64_t)NOISE_STEPS * sb->count * N * w.contact_dim * 4);
    sb->hist = nullptr;
    if (hist) {                       // (carved for the 2M loop alone: the other loops' sizes stay as they are)
        sb->hist = base ? (float*)(base + off) : nullptr;
        off += align256((int64_t)sb->count * N * w.contact_dim * 4);
    }
    return off;
}

// what a loop call fixes before its first launch
struct LoopPlan {
    afm_cdm_weights w;                // the loop's own pack: the update selectors are library-private flag bits
    int nsub;                         // 0: an empty batch, nothing to enqueue
    SubBatch sb[MAX_SUB];
    bool rowless, folded, chain_side, pipe;
    int64_t per;                      // values per sample
};

int plan_loop(const LoopCall& c, LoopPlan* p) {
    const LoopArgs& a = c.a;
    AFM_TRY(validate(c.w, a.B, c.N));
    if (!c.x || !c.feat || !c.text_q0 || !c.text_u || !c.text_cu || !a.ok() || !c.known != !c.mask) return AFM_E_BADARG;
    if (a.dpm && (!a.ddim || a.noise_term() || a.step_noise || a.first_step < 0)) return AFM_E_BADARG;
    p->nsub = 0;
    if (a.B == 0) return 0;
    p->w = *c.w;
    p->w.flags = a.loop_flags(p->w.flags);
    p->nsub = sub_count(a.B, a.n_streams, MAX_SUB);
    int64_t off = 0;
    for (int s = 0; s < p->nsub; ++s) {
        SubBatch& sb = p->sb[s];
        sb = {};
        sub_range(a.B, p->nsub, s, &sb.start, &sb.count);
        off += carve_sub(p->w, c.N, (char*)a.workspace + off, &sb, a.dpm);
        if (p->nsub > 1) { sb.stream = (hipStream_t)a.streams[2 * s]; sb.side = (hipStream_t)a.streams[2 * s + 1]; }
        else { sb.stream = (hipStream_t)a.stream; sb.side = a.streams ? (hipStream_t)a.streams[0] : nullptr; }
    }
    if (off > a.workspace_bytes) return AFM_E_WORKSPACE;
    p->rowless = cdm_mode(p->w) == 3;
    // folded form: the step-invariant parts of the two adapters are computed once for the whole range of steps and x_t is read where
    // it is needed - no per-step rewrite of the input block, no adapter GEMMs inside the loop
    p->folded = cdm_folded(p->w);
    p->chain_side = p->rowless && p->nsub > 1 && (p->w.flags & AFM_CDM_CHAIN_SIDE);
    p->pipe = p->rowless && p->nsub > 1 && (p->w.flags & AFM_CDM_PIPELINE) && !p->chain_side;
    p->per = (int64_t)c.N * p->w.contact_dim;
    return 0;
}

struct Loop {
    const LoopCall& c;
    LoopPlan p;
    Schedule sched;
};

inline float* sub_x(const Loop& l, const SubBatch& sb) { return l.c.x + (int64_t)sb.start * l.p.per; }
inline float* sub_feat(const Loop& l, const SubBatch& sb) { return l.c.feat + (int64_t)sb.start * l.c.N * l.p.w.feat_dim; }
inline const float* sub_known(const Loop& l, const SubBatch& sb) { return l.c.mask ? l.c.known + (int64_t)sb.start * l.p.per : nullptr; }
inline const uint8_t* sub_mask(const Loop& l, const SubBatch& sb) { return l.c.mask ? l.c.mask + (int64_t)sb.start * l.p.per : nullptr; }
// 2M loop: the history step j writes (NULL in every other loop), and the one it reads - what step j - 1 of this call, or the last step of
// the previous range call on the same workspace, left there; the first executed step of a chain (first_step + j == 0) has none
inline float* hist_keep(const Loop& l, const SubBatch& sb) { return l.c.a.dpm ? sb.hist : nullptr; }
inline const float* hist_prev(const Loop& l, const SubBatch& sb, int j) { return l.c.a.dpm && l.c.a.first_step + j > 0 ? sb.hist : nullptr; }

// the events of a loop call, all owned by `ev`: the fork of the sub-batch streams, the chain-side pairs, the pipeline's pairs
int loop_events(Loop& l, Events& ev) {
    LoopPlan& p = l.p;
    hipEvent_t fork = nullptr;
    if (p.nsub > 1) AFM_TRY(fork_streams(ev, (hipStream_t)l.c.a.stream, p.sb, p.nsub, &fork));
    for (int s = 0; s < p.nsub; ++s) {
        SubBatch& sb = p.sb[s];
        if (p.chain_side) {
            sb.chain.chain = sb.side;
            AFM_TRY(ev.make(&sb.chain.forked));
            AFM_TRY(ev.make(&sb.chain.joined));
            (void)hipStreamWaitEvent(sb.side, fork, 0);
        }
        if (p.pipe) {
            AFM_TRY(ev.make(&sb.enc_done));
            AFM_TRY(ev.make(&sb.tables_done));
        }
    }
    return 0;
}

// mode 1: the step-invariant tensors of every sub-batch, once per call (the generated form has nothing to prepare)
int prepare_invariants(const Loop& l) {
    for (int s = 0; cdm_mode(l.p.w) == 1 && s < l.p.nsub; ++s) {
        const SubBatch& sb = l.p.sb[s];
        if (sb.count > 0) AFM_TRY(cdm_prepare_invariants(l.p.w, sub_feat(l, sb), sb.count, l.c.N, sb.ws, sb.stream));
    }
    return 0;
}

// ---- AFM_CDM_PIPELINE (round 6; row-less form, sub-batches): the step of a sub-batch is heavy - chain - heavy: enc_point (fills the chip,
// ~15 us per 32 samples), the 13-launch latent chain (~70 us of launch latency on a handful of CUs), dec_point (fills the chip, ~88 us).
// Independent sub-batch streams fall into lockstep (a stream that is behind gets the chip to itself and catches up: both chains end up
// under each other, profiles/r04_cdm_streams.jsonl).  Here the phase is FIXED by construction: the heavy kernels of ALL sub-batches run on
// ONE stream - the caller's - in round-robin order - dec(s, j), enc(s, j + 1) for s = 0 .. nsub - 1 - and the chain of sub-batch s on its
// own side stream (streams[2 s + 1]) between two events, so that the chain of one sub-batch always sits under the point kernels of the
// others.  1 + nsub streams: the runtime has four hardware queues, and two streams on one queue do not overlap whatever the events say.
// Per-sample arithmetic does not depend on the sub-batching: bit-identical.

// noise (every NOISE_STEPS steps) and enc_point on the caller's stream H; the chain + decoder tables on the sub-batch's side stream
int pipe_enc(const Loop& l, const SubBatch& sb, int j) {
    if (sb.count == 0) return 0;
    const LoopCall& c = l.c;
    const afm_cdm_weights& w = l.p.w;
    const hipStream_t H = (hipStream_t)c.a.stream;
    const float* nz;
    AFM_TRY(step_noise(c.a, l.p.per, sb, sb.noise, j, sub_x(l, sb), &H, &nz));
    const int64_t* tj = l.sched.at(j, sb.start).t;
    AFM_TRY(launch_enc_point(w, c.text_u + (int64_t)sb.start * w.enc_heads * w.dkv, c.text_cu + (int64_t)sb.start * w.enc_heads, tj, sb.count, c.N, sb.ws,
                             sub_x(l, sb), sub_feat(l, sb), H));
    if (hipEventRecord(sb.enc_done, H) != hipSuccess || hipStreamWaitEvent(sb.side, sb.enc_done, 0) != hipSuccess) return (int)hipGetLastError();
    AFM_TRY(cdm_latent_chain(w, c.text_q0 + (int64_t)sb.start * w.dq, tj, sb.ws, sb.count, sb.side, true));
    AFM_TRY(launch_dec_tables(w, sb.count, sb.ws, sb.side));
    if (hipEventRecord(sb.tables_done, sb.side) != hipSuccess) return (int)hipGetLastError();
    return 0;
}

// dec_point (+ the update, in place) on H once the sub-batch's tables are there
int pipe_dec(const Loop& l, const SubBatch& sb, int j) {
    if (sb.count == 0) return 0;
    const hipStream_t H = (hipStream_t)l.c.a.stream;
    if (hipStreamWaitEvent(H, sb.tables_done, 0) != hipSuccess) return (int)hipGetLastError();
    const float* nz;
    AFM_TRY(step_noise(l.c.a, l.p.per, sb, sb.noise, j, sub_x(l, sb), nullptr, &nz));
    const afm_ddpm_args dd = ddpm_args(l.c.a, l.sched.at(j, sb.start), nz, sub_x(l, sb), sb, j);
    return launch_dec_point(l.p.w, sb.count, l.c.N, sb.ws, sub_x(l, sb), sub_feat(l, sb), nullptr, &dd, H, false, sub_known(l, sb), sub_mask(l, sb),
                            hist_prev(l, sb, j), hist_keep(l, sb));
}

int pipelined_steps(const Loop& l) {
    for (int s = 0; s < l.p.nsub; ++s) AFM_TRY(pipe_enc(l, l.p.sb[s], 0));
    for (int j = 0; j < l.c.a.n_steps; ++j)
        for (int s = 0; s < l.p.nsub; ++s) {
            AFM_TRY(pipe_dec(l, l.p.sb[s], j));
            if (j + 1 < l.c.a.n_steps) AFM_TRY(pipe_enc(l, l.p.sb[s], j + 1));
        }
    return 0;
}

// (sub-batch, step j) of every other form, on the sub-batch's streams
int plain_step(const Loop& l, const SubBatch& sb, int j) {
    const LoopCall& c = l.c;
    const afm_cdm_weights& w = l.p.w;
    float *xs = sub_x(l, sb), *fs = sub_feat(l, sb);
    const int64_t rows = (int64_t)sb.count * c.N;
    int64_t gx = (rows * w.contact_dim + 255) / 256; if (gx > 2048) gx = 2048;
    if (!l.p.folded) hipLaunchKernelGGL(pack_x_kernel, dim3((unsigned)gx), dim3(256), 0, sb.stream, xs, fs, rows, w.contact_dim, w.feat_dim);
    const float* nz;
    AFM_TRY(step_noise(c.a, l.p.per, sb, sb.noise, j, xs, &sb.stream, &nz));
    const StepRows r = l.sched.at(j, sb.start);
    const afm_ddpm_args dd = ddpm_args(c.a, r, nz, xs, sb, j);
    Update upd = loop_update(c.a, r, nullptr, xs, nz, l.p.per, w.flags & AFM_CDM_CLIP_X0);
    upd.known = sub_known(l, sb); upd.mask = sub_mask(l, sb);
    upd.x0_prev = hist_prev(l, sb, j); upd.x0_keep = hist_keep(l, sb);
    return cdm_forward_impl(&w, fs, xs, r.t, c.text_q0 + (int64_t)sb.start * w.dq, c.text_u + (int64_t)sb.start * w.enc_heads * w.dkv,
                            c.text_cu + (int64_t)sb.start * w.enc_heads, nullptr, &dd, sb.count, c.N, sb.base, sb.ws.bytes, sb.side, sb.stream,
                            l.p.folded, l.p.rowless, l.p.chain_side ? &sb.chain : nullptr, &upd);
}

// Whole p_sample_loop of the ADM (gaussian_diffusion.py:442-536) enqueued natively: x [B,N,contact_dim] holds x_T on entry and the
// sample on exit; feat [B,N,feat_dim] holds the step-invariant columns (point features, xyz) - its leading contact_dim columns are
// rewritten from x every step.
// One loop body for both updates: `ddim` == NULL runs the DDPM update with c1 / c2 / sigma, otherwise the DDIM update with the rows
// *ddim - in the same fused site of every sampling form, with the same launches per step.
int cdm_sample_loop_impl(const LoopCall& c) {
    Loop l{c, {}, {}};
    AFM_TRY(plan_loop(c, &l.p));
    if (l.p.nsub == 0) return 0;
    AFM_TRY(l.sched.expand(c.a));
    Events ev;                        // every return below releases what was created
    AFM_TRY(loop_events(l, ev));
    int rc = prepare_invariants(l);
    if (rc == 0 && l.p.pipe) rc = pipelined_steps(l);
    for (int j = 0; j < c.a.n_steps && rc == 0 && !l.p.pipe; ++j)
        for (int s = 0; s < l.p.nsub && rc == 0; ++s)
            if (l.p.sb[s].count > 0) rc = plain_step(l, l.p.sb[s], j);
    if (l.p.nsub > 1) join_streams(ev, (hipStream_t)c.a.stream, l.p.sb, l.p.nsub);
    return rc;
}

}  // namespace

static int64_t cdm_loop_workspace_bytes(const afm_cdm_weights* w, int32_t B, int32_t N, int32_t n_sub, bool hist) {
    if (validate(w, B, N) != 0 || n_sub < 0) return AFM_E_BADARG;
    const int nsub = sub_count(B, n_sub, MAX_SUB);
    int64_t total = 0;
    for (int s = 0; s < nsub; ++s) {
        SubBatch sb = {};
        sub_range(B, nsub, s, &sb.start, &sb.count);
        total += carve_sub(*w, N, nullptr, &sb, hist);
    }
    return total;
}

extern "C" int64_t afm_cdm_loop_workspace_bytes(const afm_cdm_weights* w, int32_t B, int32_t N, int32_t n_sub) {
    return cdm_loop_workspace_bytes(w, B, N, n_sub, false);
}

extern "C" int afm_cdm_sample_loop(const afm_cdm_weights* w, float* x, float* feat, const float* text_q0, const float* text_u,
                                   const float* text_cu, const float* step_noise, const int64_t* d_timestep_map, const float* d_c1,
                                   const float* d_c2, const float* d_sigma, int32_t n_steps, uint64_t seed, int64_t sample_index0, int32_t B,
                                   int32_t N, void* sched_scratch, void* workspace, int64_t workspace_bytes, int32_t n_sub, void* const* streams,
                                   void* stream) {
    return cdm_sample_loop_impl({w, x, feat, text_q0, text_u, text_cu, N, {step_noise, d_timestep_map, d_c1, d_c2, d_sigma, nullptr, n_steps, 0, seed, sample_index0, B,
                                 sched_scratch, workspace, workspace_bytes, n_sub, streams, stream}});
}

extern "C" int afm_cdm_sample_loop_range(const afm_cdm_weights* w, float* x, float* feat, const float* text_q0, const float* text_u,
                                         const float* text_cu, const float* step_noise, const int64_t* d_timestep_map, const float* d_c1,
                                         const float* d_c2, const float* d_sigma, int32_t n_steps, int32_t first_step, uint64_t seed,
                                         int64_t sample_index0, int32_t B, int32_t N, void* sched_scratch, void* workspace,
                                         int64_t workspace_bytes, int32_t n_sub, void* const* streams, void* stream) {
    if (first_step < 0) return AFM_E_BADARG;
    return cdm_sample_loop_impl({w, x, feat, text_q0, text_u, text_cu, N, {step_noise, d_timestep_map, d_c1, d_c2, d_sigma, nullptr, n_steps, first_step, seed, sample_index0, B,
                                 sched_scratch, workspace, workspace_bytes, n_sub, streams, stream}});
}

extern "C" int afm_cdm_ddim_loop_range(const afm_cdm_weights* w, float* x, float* feat, const float* text_q0, const float* text_u,
                                       const float* text_cu, const float* step_noise, const int64_t* d_timestep_map, const afm_ddim_rows* rows,
                                       int32_t n_steps, int32_t first_step, uint64_t seed, int64_t sample_index0, int32_t B, int32_t N,
                                       void* sched_scratch, void* workspace, int64_t workspace_bytes, int32_t n_sub, void* const* streams, void* stream) {
    if (first_step < 0 || !rows) return AFM_E_BADARG;
    return cdm_sample_loop_impl({w, x, feat, text_q0, text_u, text_cu, N, {step_noise, d_timestep_map, nullptr, nullptr, nullptr, rows, n_steps, first_step, seed, sample_index0, B,
                                 sched_scratch, workspace, workspace_bytes, n_sub, streams, stream}});
}

// The imputing native loop, DDPM and DDIM behind one entry (rows != NULL: DDIM, d_c1 / d_c2 / d_sigma ignored): known / mask both NULL is
// the loop without imputation
extern "C" int afm_cdm_impute_loop_range(const afm_cdm_weights* w, float* x, float* feat, const float* text_q0, const float* text_u,
                                         const float* text_cu, const float* step_noise, const int64_t* d_timestep_map, const afm_ddim_rows* rows,
                                         const float* d_c1, const float* d_c2, const float* d_sigma, const float* known, const uint8_t* mask,
                                         int32_t n_steps, int32_t first_step, uint64_t seed, int64_t sample_index0, int32_t B, int32_t N,
                                         void* sched_scratch, void* workspace, int64_t workspace_bytes, int32_t n_sub, void* const* streams, void* stream) {
    if (!known != !mask) return AFM_E_BADARG;
    if (first_step < 0) return AFM_E_BADARG;
    if (rows) d_c1 = d_c2 = d_sigma = nullptr;
    return cdm_sample_loop_impl({w, x, feat, text_q0, text_u, text_cu, N, {step_noise, d_timestep_map, d_c1, d_c2, d_sigma, rows, n_steps, first_step, seed, sample_index0, B,
                                 sched_scratch, workspace, workspace_bytes, n_sub, streams, stream}, known, mask});
}

// DPM-Solver++(2M): the eta = 0 DDIM loop with dpm_update in its place and one history buffer per sub-batch.  Row-less form: the update and
// the history ride in dec_point (dec_point_dpm_kernel), with or without known / mask - the launches of the DDIM loop.  Folded-rows and
// layer-by-layer forms: pred_xstart stored where their imputing loops store it, then one update launch per sub-batch and step.  The rows
// travel through the DDIM schedule layout as {a, b, c, unused}.
extern "C" int64_t afm_cdm_dpm_loop_workspace_bytes(const afm_cdm_weights* w, int32_t B, int32_t N, int32_t n_sub) {
    return cdm_loop_workspace_bytes(w, B, N, n_sub, true);
}

extern "C" int afm_cdm_dpm_loop_range(const afm_cdm_weights* w, float* x, float* feat, const float* text_q0, const float* text_u,
                                      const float* text_cu, const int64_t* d_timestep_map, const afm_dpm_rows* rows, const float* known,
                                      const uint8_t* mask, int32_t n_steps, int32_t first_step, int32_t B, int32_t N, void* sched_scratch,
                                      void* workspace, int64_t workspace_bytes, int32_t n_sub, void* const* streams, void* stream) {
    if (first_step < 0 || !rows || !rows->a || !rows->b || !rows->c || !known != !mask) return AFM_E_BADARG;
    const afm_ddim_rows as_ddim = {rows->a, rows->b, rows->c, rows->c, nullptr};          // (d: any valid row, never used by dpm_update)
    LoopCall c = {w, x, feat, text_q0, text_u, text_cu, N, {nullptr, d_timestep_map, nullptr, nullptr, nullptr, &as_ddim, n_steps, first_step, 0, 0, B,
                  sched_scratch, workspace, workspace_bytes, n_sub, streams, stream}, known, mask};
    c.a.dpm = true;
    return cdm_sample_loop_impl(c);
}
