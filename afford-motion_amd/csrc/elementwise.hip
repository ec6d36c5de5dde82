// LayerNorm, DDPM posterior update, Philox normal generator.
// All three are HBM/L2-streaming kernels: float4 accesses, one wave per LayerNorm row.
#include "common.h"
#include "profile.h"

namespace {

// one wave per row; the row lives in registers (dim <= 64 * 4 * MAXV)
template <int MAXV>
__global__ __launch_bounds__(256) void layernorm_kernel(const float* __restrict__ x, const float* __restrict__ gamma,
                                                        const float* __restrict__ beta, float* __restrict__ y,
                                                        int64_t rows, int dim, float eps, int grp, int stride, int off) {
    const int lane = threadIdx.x & 63;
    int64_t row = (int64_t)blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6);
    if (row >= rows) return;
    if (grp) row = (row / grp) * stride + off + row % grp;          // logical row -> strided token row
    layernorm_row<MAXV>(x + row * dim, gamma, beta, y + row * dim, dim, eps, lane);
}

// any dim (not a multiple of 4, e.g. the 646-wide input LayerNorm of the CDM 'MLP' arch, cdm.py:18-23): wave per row,
// lane-strided scalar accesses, three passes over the (L1/L2-resident) row
__global__ __launch_bounds__(256) void layernorm_generic_kernel(const float* __restrict__ x, const float* __restrict__ gamma,
                                                                const float* __restrict__ beta, float* __restrict__ y, int64_t rows, int dim,
                                                                float eps) {
    const int lane = threadIdx.x & 63;
    const int64_t row = (int64_t)blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6);
    if (row >= rows) return;
    const float* xp = x + row * dim;
    float sum = 0.f;
    for (int c = lane; c < dim; c += 64) sum += xp[c];
    const float mean = wave_sum(sum) / (float)dim;
    float sq = 0.f;
    for (int c = lane; c < dim; c += 64) { const float d = xp[c] - mean; sq += d * d; }
    const float rstd = 1.0f / sqrtf(wave_sum(sq) / (float)dim + eps);
    float* yp = y + row * dim;
    for (int c = lane; c < dim; c += 64) yp[c] = (xp[c] - mean) * rstd * gamma[c] + beta[c];
}

// x_next = (c1*x0 + c2*x_t) + sigma*noise with every product and sum individually rounded
// (bit-identical to the reference's float32 torch expression).
__global__ __launch_bounds__(256) void ddpm_step_kernel(const float* __restrict__ x0, const float* __restrict__ xt,
                                                        const float* __restrict__ noise, float* __restrict__ xn,
                                                        const float* __restrict__ c1, const float* __restrict__ c2,
                                                        const float* __restrict__ sigma, int64_t per_sample, uint64_t seed,
                                                        int64_t sample0, int step) {
#pragma clang fp contract(off)
    const int b = blockIdx.y;
    const float a1 = c1[b], a2 = c2[b], sg = sigma[b];
    const int64_t base = (int64_t)b * per_sample;
    const int64_t nquad = (per_sample + 3) >> 2;
    for (int64_t q = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; q < nquad; q += (int64_t)gridDim.x * blockDim.x) {
        float z[4];
        if (!noise) philox_normal4(seed, sample0 + b, step, (uint64_t)q, z);
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            const int64_t i = q * 4 + e;
            if (i < per_sample) {
                const float nz = noise ? noise[base + i] : z[e];
                const float m1 = a1 * x0[base + i];
                const float m2 = a2 * xt[base + i];
                const float mean = m1 + m2;
                const float sn = sg * nz;
                xn[base + i] = mean + sn;
            }
        }
    }
}

// DDIM update (ddim_sample / ddim_reverse_sample): ddim_update of common.h per element; sg == NULL: no noise term
__global__ __launch_bounds__(256) void ddim_step_kernel(const float* __restrict__ x0, const float* xt, const float* __restrict__ noise,
                                                        float* xn, const float* __restrict__ ra, const float* __restrict__ rb,
                                                        const float* __restrict__ rc, const float* __restrict__ rd,
                                                        const float* __restrict__ sg, int64_t per_sample, uint64_t seed, int64_t sample0, int step) {
    const int b = blockIdx.y;
    const float4 r = make_float4(ra[b], rb[b], rc[b], rd[b]);
    const float s = sg ? sg[b] : 0.f;
    const int64_t base = (int64_t)b * per_sample;
    const int64_t nquad = (per_sample + 3) >> 2;
    for (int64_t q = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; q < nquad; q += (int64_t)gridDim.x * blockDim.x) {
        float z[4];
        if (sg && !noise) philox_normal4(seed, sample0 + b, step, (uint64_t)q, z);
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            const int64_t i = q * 4 + e;
            if (i < per_sample) {
                const float v0 = x0[base + i], vt = xt[base + i];
                xn[base + i] = sg ? ddim_update(v0, vt, r, s, noise ? noise[base + i] : z[e]) : ddim_update(v0, vt, r);
            }
        }
    }
}

// DDIM update of a native loop's step: x <- ddim_update(clamp?(x0), x, rec[b], s[b], noise) in place (one thread reads then writes an element),
// plus the copy into the K-padded rows the next step's motion adapter reads (xpad [rows][ldpad], columns >= cols stay zero)
__global__ __launch_bounds__(256) void ddim_update_rows_kernel(const float* __restrict__ x0, float* x, const float* __restrict__ noise,
                                                               const float4* __restrict__ rec, const float* __restrict__ sg, int64_t per_sample,
                                                               int cols, int clip, float* __restrict__ xpad, int64_t ldpad) {
    const int b = blockIdx.y;
    const float4 r = rec[b];
    const float s = sg ? sg[b] : 0.f;
    const int64_t base = (int64_t)b * per_sample;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < per_sample; i += (int64_t)gridDim.x * blockDim.x) {
        float v = x0[base + i];
        if (clip) v = v < -1.0f ? -1.0f : (v > 1.0f ? 1.0f : v);          // clip_denoised (NaN passes through, as torch.clamp)
        const float xn = sg ? ddim_update(v, x[base + i], r, s, noise[base + i]) : ddim_update(v, x[base + i], r);
        x[base + i] = xn;
        if (xpad) {
            const int64_t g = base + i, row = g / cols;
            xpad[row * ldpad + (g - row * cols)] = xn;
        }
    }
}

// grid (x, B, steps): blockIdx.z = a further step of the same keying, its [B][per_sample] block behind the previous one
__global__ __launch_bounds__(256) void randn_kernel(float* __restrict__ out, int64_t per_sample, uint64_t seed,
                                                    int64_t sample0, int step) {
    const int b = blockIdx.y;
    out += (int64_t)blockIdx.z * gridDim.y * per_sample;
    step += (int)blockIdx.z;
    const int64_t base = (int64_t)b * per_sample;
    const int64_t nquad = (per_sample + 3) >> 2;
    for (int64_t q = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; q < nquad; q += (int64_t)gridDim.x * blockDim.x) {
        float z[4];
        philox_normal4(seed, sample0 + b, step, (uint64_t)q, z);
#pragma unroll
        for (int e = 0; e < 4; ++e)
            if (q * 4 + e < per_sample) out[base + q * 4 + e] = z[e];
    }
}

// per-sample masked MSE: sum((a-b)^2 * keep) / (sum(keep) * D), one 1024-thread workgroup per sample: a thread walks
// whole frames (row l, then its D contiguous values are spread over the 16 lanes of its group -> coalesced, no division
// per element), fixed-order tree at the end
__global__ __launch_bounds__(1024) void masked_mse_kernel(const float* __restrict__ a, const float* __restrict__ b,
                                                          const uint8_t* __restrict__ mask, float* __restrict__ out, int L, int D) {
    __shared__ float red[2][16];
    const int s = blockIdx.x;
    const int sub = threadIdx.x & 15, grp = threadIdx.x >> 4;       // 64 groups of 16 lanes, one frame per group at a time
    float acc = 0.f, cnt = 0.f;
    for (int l = grp; l < L; l += 64) {
        if (mask && mask[(int64_t)s * L + l]) continue;
        const float* ap = a + ((int64_t)s * L + l) * D;
        const float* bp = b + ((int64_t)s * L + l) * D;
        for (int c = sub; c < D; c += 16) { const float d = ap[c] - bp[c]; acc += d * d; }
        if (sub == 0) cnt += (float)D;
    }
    acc = wave_sum(acc); cnt = wave_sum(cnt);
    if ((threadIdx.x & 63) == 0) { red[0][threadIdx.x >> 6] = acc; red[1][threadIdx.x >> 6] = cnt; }
    __syncthreads();
    if (threadIdx.x == 0) {
        float sa = 0.f, sc = 0.f;
#pragma unroll
        for (int i = 0; i < 16; ++i) { sa += red[0][i]; sc += red[1][i]; }
        out[s] = sa / sc;            // sc == sum(keep) * D
    }
}

// eval-mode BatchNorm folded into y = x * scale + shift (optionally around a preceding nn.Linear's bias: BN(W x + lb) = scale W x + (lb scale + shift)):
// scale = w / sqrt(var + eps), shift = b - mean * scale.  Individually rounded operations (the torch expression, bit for bit).
__global__ __launch_bounds__(256) void bn_fold_kernel(const float* __restrict__ w, const float* __restrict__ b, const float* __restrict__ mean,
                                                      const float* __restrict__ var, float eps, const float* __restrict__ lin_bias,
                                                      float* __restrict__ scale, float* __restrict__ shift, int C) {
#pragma clang fp contract(off)
    const int c = blockIdx.x * 256 + threadIdx.x;
    if (c >= C) return;
    const float sc = w[c] / sqrtf(var[c] + eps);
    const float ms = mean[c] * sc;
    float sh = b[c] - ms;
    if (lin_bias) { const float lb = lin_bias[c] * sc; sh = lb + sh; }
    scale[c] = sc;
    shift[c] = sh;
}

// ADM -> AMDM hand-off in HBM (the reference goes through .npy files): contact = clip(sample * std + mean, 1e-20, 1)
// (datasets/humanml3d.py:494-511), dist = sqrt(-2 ln(contact) sigma^2) (utils/evaluate.py:56-66), condition = exp(-dist^2 / (2 sigma^2))
// (datasets/humanml3d.py:773-774) - the reference's chain of float32 operations, one element per thread.
__global__ __launch_bounds__(256) void contact_glue_kernel(const float* __restrict__ sample, float* __restrict__ out, int64_t n, float sigma2, float mean, float std) {
#pragma clang fp contract(off)
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (int64_t)gridDim.x * 256) {
        float c = sample[i] * std;
        c = c + mean;
        c = fminf(fmaxf(c, 1e-20f), 1.0f);
        const float l = -2.0f * logf(c);
        const float d = sqrtf(l * sigma2);
        const float e = -0.5f * (d * d);
        out[i] = expf(e / sigma2);
    }
}

}  // namespace

namespace {
__global__ void clamp_kernel(float* __restrict__ x, int64_t n, float lo, float hi) {
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) {
        const float v = x[i];
        x[i] = v < lo ? lo : (v > hi ? hi : v);
    }
}
}  // namespace

extern "C" int afm_clamp(float* x, int64_t n, float lo, float hi, void* stream) {
    if (n == 0) return 0;
    if (!x || n < 0 || !(lo <= hi)) return AFM_E_BADARG;
    int64_t g = (n + 255) / 256; if (g > 4096) g = 4096;
    hipLaunchKernelGGL(clamp_kernel, dim3((unsigned)g), dim3(256), 0, (hipStream_t)stream, x, n, lo, hi);
    AFM_CHECK_LAUNCH();
    return 0;
}

extern "C" int afm_bn_fold(const float* w, const float* b, const float* mean, const float* var, float eps, const float* lin_bias, float* scale,
                           float* shift, int32_t C, void* stream) {
    if (C == 0) return 0;
    if (!w || !b || !mean || !var || !scale || !shift || C < 0 || !(eps >= 0.0f)) return AFM_E_BADARG;
    hipLaunchKernelGGL(bn_fold_kernel, dim3((C + 255) / 256), dim3(256), 0, (hipStream_t)stream, w, b, mean, var, eps, lin_bias, scale, shift, C);
    AFM_CHECK_LAUNCH();
    return 0;
}

extern "C" int afm_contact_glue(const float* sample, float* out, int64_t n, float sigma_sq, float mean, float std, void* stream) {
    if (n == 0) return 0;
    if (!sample || !out || n < 0 || !(sigma_sq > 0.0f)) return AFM_E_BADARG;
    int64_t g = (n + 255) / 256; if (g > 4096) g = 4096;
    hipLaunchKernelGGL(contact_glue_kernel, dim3((unsigned)g), dim3(256), 0, (hipStream_t)stream, sample, out, n, sigma_sq, mean, std);
    AFM_CHECK_LAUNCH();
    return 0;
}

extern "C" int afm_masked_mse(const float* target, const float* pred, const uint8_t* frame_mask, float* out, int32_t B,
                              int32_t L, int32_t D, void* stream) {
    if (!target || !pred || !out || B < 0 || L <= 0 || D <= 0) return AFM_E_BADARG;
    if (B == 0) return 0;
    hipLaunchKernelGGL(masked_mse_kernel, dim3(B), dim3(1024), 0, (hipStream_t)stream, target, pred, frame_mask, out, L, D);
    AFM_CHECK_LAUNCH();
    return 0;
}

extern "C" int afm_layernorm_rows(const float* x, const float* gamma, const float* beta, float* y, int64_t rows, int32_t dim,
                                  float eps, int32_t grp, int32_t stride, int32_t off, void* stream);

extern "C" int afm_layernorm(const float* x, const float* gamma, const float* beta, float* y, int64_t rows, int32_t dim,
                             float eps, void* stream) {
    return afm_layernorm_rows(x, gamma, beta, y, rows, dim, eps, 0, 0, 0, stream);
}

extern "C" int afm_layernorm_rows(const float* x, const float* gamma, const float* beta, float* y, int64_t rows, int32_t dim,
                                  float eps, int32_t grp, int32_t stride, int32_t off, void* stream) {
    if (dim <= 0) return AFM_E_BADARG;
    if (rows == 0) return 0;                                  // empty batch (pointers may be null)
    if (!x || !gamma || !beta || !y || rows < 0) return AFM_E_BADARG;
    if ((dim & 3) || ((((uintptr_t)x) | ((uintptr_t)y) | ((uintptr_t)gamma) | ((uintptr_t)beta)) & 15)) {
        if (grp) return AFM_E_UNSUPPORTED;                     // the row-subset form is only used with d_model (multiple of 4)
        AfmProf prof(AFM_PROF_LN, 8.0 * rows * dim, (hipStream_t)stream);
        hipLaunchKernelGGL(layernorm_generic_kernel, dim3((unsigned)((rows + 3) / 4)), dim3(256), 0, (hipStream_t)stream, x, gamma, beta, y, rows, dim, eps);
        AFM_CHECK_LAUNCH();
        return 0;
    }
    if (rows == 0) return 0;
    hipStream_t s = (hipStream_t)stream;
    const dim3 block(256), grid((unsigned)((rows + 3) / 4));
    AfmProf prof(AFM_PROF_LN, 8.0 * rows * dim, s);
    if (dim <= 256) hipLaunchKernelGGL(layernorm_kernel<1>, grid, block, 0, s, x, gamma, beta, y, rows, dim, eps, grp, stride, off);
    else if (dim <= 512) hipLaunchKernelGGL(layernorm_kernel<2>, grid, block, 0, s, x, gamma, beta, y, rows, dim, eps, grp, stride, off);
    else if (dim <= 1024) hipLaunchKernelGGL(layernorm_kernel<4>, grid, block, 0, s, x, gamma, beta, y, rows, dim, eps, grp, stride, off);
    else if (dim <= 2048) hipLaunchKernelGGL(layernorm_kernel<8>, grid, block, 0, s, x, gamma, beta, y, rows, dim, eps, grp, stride, off);
    else return AFM_E_UNSUPPORTED;
    AFM_CHECK_LAUNCH();
    return 0;
}

extern "C" int afm_ddpm_step(const float* x0, const float* x_t, const float* noise, float* x_next, const float* c1,
                             const float* c2, const float* sigma, int32_t B, int64_t per_sample, uint64_t seed,
                             int64_t sample_index0, int32_t step, void* stream) {
    if (!x0 || !x_t || !x_next || !c1 || !c2 || !sigma || B < 0 || per_sample <= 0) return AFM_E_BADARG;
    if (B == 0) return 0;
    const int64_t nquad = (per_sample + 3) >> 2;
    unsigned gx = (unsigned)((nquad + 255) / 256);
    if (gx > 1024) gx = 1024;
    hipLaunchKernelGGL(ddpm_step_kernel, dim3(gx, B), dim3(256), 0, (hipStream_t)stream, x0, x_t, noise, x_next, c1, c2, sigma,
                       per_sample, seed, sample_index0, step);
    AFM_CHECK_LAUNCH();
    return 0;
}

extern "C" int afm_ddim_step(const float* x0, const float* x_t, const float* noise, float* x_next, const afm_ddim_rows* rows,
                             int32_t B, int64_t per_sample, uint64_t seed, int64_t sample_index0, int32_t step, void* stream) {
    if (!x0 || !x_t || !x_next || !rows || !rows->a || !rows->b || !rows->c || !rows->d || B < 0 || per_sample <= 0) return AFM_E_BADARG;
    if (B == 0) return 0;
    const int64_t nquad = (per_sample + 3) >> 2;
    unsigned gx = (unsigned)((nquad + 255) / 256);
    if (gx > 1024) gx = 1024;
    hipLaunchKernelGGL(ddim_step_kernel, dim3(gx, B), dim3(256), 0, (hipStream_t)stream, x0, x_t, noise, x_next, rows->a, rows->b, rows->c,
                       rows->d, rows->sigma, per_sample, seed, sample_index0, step);
    AFM_CHECK_LAUNCH();
    return 0;
}

// the DDIM update of a native loop's step (cmdm.hip, perceiver.hip): x0 [B][per_sample] pred_xstart, x [B][per_sample] x_t -> x_next in
// place, rec [B] {a, b, c, d}, s [B] (NULL: no noise term, `noise` not read), rows of `cols` values copied to xpad (row stride ldpad) if given
__attribute__((visibility("hidden"))) int afm_ddim_update_rows(const float* x0, float* x, const float* noise, const float4* rec, const float* s, int32_t B,
                                                               int64_t per_sample, int32_t cols, int32_t clip, float* xpad, int64_t ldpad, void* stream) {
    if (!x0 || !x || !rec || (s && !noise) || B < 0 || per_sample <= 0 || cols <= 0 || (xpad && ldpad < cols)) return AFM_E_BADARG;
    if (B == 0) return 0;
    unsigned gx = (unsigned)((per_sample + 255) / 256);
    if (gx > 1024) gx = 1024;
    hipLaunchKernelGGL(ddim_update_rows_kernel, dim3(gx, B), dim3(256), 0, (hipStream_t)stream, x0, x, noise, rec, s, per_sample, cols, clip, xpad, ldpad);
    AFM_CHECK_LAUNCH();
    return 0;
}

// the DDPM rows of a native loop (sample_loop.h: Schedule), per step and sample: row j <-> spaced timestep i = n_steps - 1 - j
__global__ void ddpm_expand_schedule_kernel(const int64_t* __restrict__ tmap, const float* __restrict__ c1, const float* __restrict__ c2,
                                            const float* __restrict__ sg, int n_steps, int B, int64_t* __restrict__ t_all,
                                            float* __restrict__ c1_all, float* __restrict__ c2_all, float* __restrict__ sg_all) {
    const int64_t n = (int64_t)n_steps * B;
    for (int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; e < n; e += (int64_t)gridDim.x * blockDim.x) {
        const int i = n_steps - 1 - (int)(e / B);
        t_all[e] = tmap[i]; c1_all[e] = c1[i]; c2_all[e] = c2[i]; sg_all[e] = sg[i];
    }
}

__attribute__((visibility("hidden"))) int afm_ddpm_expand_rows(const int64_t* tmap, const float* c1, const float* c2, const float* sigma, int32_t n_steps,
                                                               int32_t B, int64_t* t_all, float* c1_all, float* c2_all, float* s_all, void* stream) {
    const int64_t nb = (int64_t)n_steps * B;
    hipLaunchKernelGGL(ddpm_expand_schedule_kernel, dim3((unsigned)((nb + 255) / 256)), dim3(256), 0, (hipStream_t)stream, tmap, c1, c2, sigma, n_steps, B,
                       t_all, c1_all, c2_all, s_all);
    AFM_CHECK_LAUNCH();
    return 0;
}

// the DDIM rows of a native loop (sample_loop.h: Schedule), expanded like their DDPM rows: entry e = j * B + b of step j (timestep index
// n_steps - 1 - j of the slice's rows): t_all[e] = tmap[i], rec_all[e] = {a, b, c, d}[i], s_all[e] = sigma[i] (rows->sigma NULL: s_all not written)
__global__ void ddim_expand_kernel(const int64_t* __restrict__ tmap, const float* __restrict__ ra, const float* __restrict__ rb,
                                   const float* __restrict__ rc, const float* __restrict__ rd, const float* __restrict__ sg, int n_steps, int B,
                                   int64_t* __restrict__ t_all, float4* __restrict__ rec_all, float* __restrict__ s_all) {
    const int64_t n = (int64_t)n_steps * B;
    for (int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; e < n; e += (int64_t)gridDim.x * blockDim.x) {
        const int i = n_steps - 1 - (int)(e / B);
        t_all[e] = tmap[i]; rec_all[e] = make_float4(ra[i], rb[i], rc[i], rd[i]);
        if (sg) s_all[e] = sg[i];
    }
}

__attribute__((visibility("hidden"))) int afm_ddim_expand_rows(const int64_t* tmap, const afm_ddim_rows* rows, int32_t n_steps, int32_t B, int64_t* t_all,
                                                               float4* rec_all, float* s_all, void* stream) {
    if (!tmap || !rows || !t_all || !rec_all || (rows->sigma && !s_all) || n_steps <= 0 || B < 0) return AFM_E_BADARG;
    const int64_t nb = (int64_t)n_steps * B;
    if (nb == 0) return 0;
    hipLaunchKernelGGL(ddim_expand_kernel, dim3((unsigned)((nb + 255) / 256)), dim3(256), 0, (hipStream_t)stream, tmap, rows->a, rows->b, rows->c, rows->d,
                       rows->sigma, n_steps, B, t_all, rec_all, s_all);
    AFM_CHECK_LAUNCH();
    return 0;
}

// the noise of `nsteps` consecutive steps in one launch: out [nsteps][B][per_sample], step index step0 + i (same values as nsteps calls of afm_randn)
__attribute__((visibility("hidden"))) int afm_randn_steps(float* out, int32_t B, int64_t per_sample, uint64_t seed, int64_t sample_index0, int32_t step0, int32_t nsteps, void* stream) {
    if (!out || B < 0 || per_sample <= 0 || nsteps < 0 || nsteps > 65535) return AFM_E_BADARG;
    if (B == 0 || nsteps == 0) return 0;
    const int64_t nquad = (per_sample + 3) >> 2;
    unsigned gx = (unsigned)((nquad + 255) / 256);
    if (gx > 1024) gx = 1024;
    hipLaunchKernelGGL(randn_kernel, dim3(gx, B, nsteps), dim3(256), 0, (hipStream_t)stream, out, per_sample, seed, sample_index0, step0);
    AFM_CHECK_LAUNCH();
    return 0;
}

extern "C" int afm_randn(float* out, int32_t B, int64_t per_sample, uint64_t seed, int64_t sample_index0, int32_t step,
                         void* stream) {
    if (!out || B < 0 || per_sample <= 0) return AFM_E_BADARG;
    if (B == 0) return 0;
    const int64_t nquad = (per_sample + 3) >> 2;
    unsigned gx = (unsigned)((nquad + 255) / 256);
    if (gx > 1024) gx = 1024;
    hipLaunchKernelGGL(randn_kernel, dim3(gx, B), dim3(256), 0, (hipStream_t)stream, out, per_sample, seed, sample_index0, step);
    AFM_CHECK_LAUNCH();
    return 0;
}

// ---- classifier-free guidance (afm_cfg_combine, afm_cfg_step, the guided native loops of cmdm.hip)
namespace {

// x0_guided = cfg_combine(x0_c, x0_u, scale[b]) per element
__global__ __launch_bounds__(256) void cfg_combine_kernel(const float* __restrict__ x0c, const float* __restrict__ x0u, const float* __restrict__ scale,
                                                          float* __restrict__ out, int64_t per_sample) {
    const int b = blockIdx.y;
    const float s = scale[b];
    const int64_t base = (int64_t)b * per_sample;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < per_sample; i += (int64_t)gridDim.x * blockDim.x)
        out[base + i] = cfg_combine(x0c[base + i], x0u[base + i], s);
}

// The guided sampling update, the guided sibling of ddim_update_rows_kernel: x0 = cfg_combine(x0_c, x0_u, scale[b]), clamped if asked,
// then ddpm_update (ddim == 0; rows c1 / c2 / sg per sample) or ddim_update (rows rec, or ra..rd, per sample; sg == NULL: no noise term).
// xn may alias xt (one thread reads then writes an element).  noise == NULL with a noise term: Philox keyed like ddpm_step_kernel (quad q).
// xpad: x_next also into rows of ldpad floats (the next motion-adapter GEMM's K-padded A rows; columns >= cols stay zero).
struct CfgUpd {
    const float *x0c, *x0u, *scale, *xt, *noise;
    float* xn;
    const float *c1, *c2, *sg;
    const float *ra, *rb, *rc, *rd;
    const float4* rec;
    float* xpad;
    int64_t ldpad, per_sample, sample0;
    uint64_t seed;
    int cols, clip, ddim, step;
};

__global__ __launch_bounds__(256) void cfg_update_kernel(const CfgUpd p) {
    const int b = blockIdx.y;
    const float s = p.scale[b];
    const float sg = p.sg ? p.sg[b] : 0.f;
    float4 r = make_float4(0.f, 1.f, 0.f, 0.f);
    float c1 = 0.f, c2 = 0.f;
    if (p.ddim) r = p.rec ? p.rec[b] : make_float4(p.ra[b], p.rb[b], p.rc[b], p.rd[b]);
    else { c1 = p.c1[b]; c2 = p.c2[b]; }
    const int64_t base = (int64_t)b * p.per_sample;
    const int64_t nquad = (p.per_sample + 3) >> 2;
    for (int64_t q = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; q < nquad; q += (int64_t)gridDim.x * blockDim.x) {
        float z[4] = {0.f, 0.f, 0.f, 0.f};
        if (p.sg && !p.noise) philox_normal4(p.seed, p.sample0 + b, p.step, (uint64_t)q, z);
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            const int64_t i = q * 4 + e;
            if (i < p.per_sample) {
                const int64_t g = base + i;
                float v = cfg_combine(p.x0c[g], p.x0u[g], s);
                if (p.clip) v = v < -1.0f ? -1.0f : (v > 1.0f ? 1.0f : v);          // clip_denoised on x0_guided (NaN passes through, as torch.clamp)
                const float nz = p.sg ? (p.noise ? p.noise[g] : z[e]) : 0.f;
                const float vt = p.xt[g];
                float xn;
                if (p.ddim) xn = p.sg ? ddim_update(v, vt, r, sg, nz) : ddim_update(v, vt, r);
                else xn = ddpm_update(v, vt, c1, c2, sg, nz);
                p.xn[g] = xn;
                if (p.xpad) {
                    const int64_t row = g / p.cols;
                    p.xpad[row * p.ldpad + (g - row * p.cols)] = xn;
                }
            }
        }
    }
}

int launch_cfg_update(const CfgUpd& p, int32_t B, void* stream) {
    if (!p.x0c || !p.x0u || !p.scale || !p.xt || !p.xn || B < 0 || p.per_sample <= 0) return AFM_E_BADARG;
    if (p.ddim ? !(p.rec || (p.ra && p.rb && p.rc && p.rd)) : !(p.c1 && p.c2 && p.sg)) return AFM_E_BADARG;
    if (p.xpad && (p.cols <= 0 || p.ldpad < p.cols)) return AFM_E_BADARG;
    if (B == 0) return 0;
    const int64_t nquad = (p.per_sample + 3) >> 2;
    unsigned gx = (unsigned)((nquad + 255) / 256);
    if (gx > 1024) gx = 1024;
    AfmProf prof(AFM_PROF_MISC, 5.0 * B * p.per_sample, (hipStream_t)stream);
    hipLaunchKernelGGL(cfg_update_kernel, dim3(gx, B), dim3(256), 0, (hipStream_t)stream, p);
    AFM_CHECK_LAUNCH();
    return 0;
}

}  // namespace

extern "C" int afm_cfg_combine(const float* x0_c, const float* x0_u, const float* scale, float* out, int32_t B, int64_t per_sample, void* stream) {
    if (!x0_c || !x0_u || !scale || !out || B < 0 || per_sample <= 0) return AFM_E_BADARG;
    if (B == 0) return 0;
    unsigned gx = (unsigned)((per_sample + 255) / 256);
    if (gx > 1024) gx = 1024;
    AfmProf prof(AFM_PROF_MISC, 3.0 * B * per_sample, (hipStream_t)stream);
    hipLaunchKernelGGL(cfg_combine_kernel, dim3(gx, B), dim3(256), 0, (hipStream_t)stream, x0_c, x0_u, scale, out, per_sample);
    AFM_CHECK_LAUNCH();
    return 0;
}

extern "C" int afm_cfg_step(const afm_cfg_step_args* a, void* stream) {
    if (!a) return AFM_E_BADARG;
    CfgUpd p = {};
    p.x0c = a->x0_c; p.x0u = a->x0_u; p.scale = a->scale; p.xt = a->x_t; p.noise = a->noise; p.xn = a->x_next;
    p.per_sample = a->per_sample; p.clip = a->clip ? 1 : 0; p.seed = a->seed; p.sample0 = a->sample_index0; p.step = a->step;
    if (a->ddim) { p.ddim = 1; p.ra = a->ddim->a; p.rb = a->ddim->b; p.rc = a->ddim->c; p.rd = a->ddim->d; p.sg = a->ddim->sigma; }
    else { p.c1 = a->c1; p.c2 = a->c2; p.sg = a->sigma; }
    return launch_cfg_update(p, a->B, stream);
}

// the guided update of a native loop's step (cmdm.hip): x0_c / x0_u [B][per_sample] the two branches' pred_xstart, x [B][per_sample] x_t ->
// x_next in place, scale [B]; rec != NULL: DDIM records {a, b, c, d} [B] with s [B] (NULL: no noise term), else the DDPM rows c1 / c2 / s [B];
// rows of `cols` values copied to xpad (row stride ldpad) if given
__attribute__((visibility("hidden"))) int afm_cfg_update_rows(const float* x0_c, const float* x0_u, const float* scale, float* x, const float* noise,
                                                              const float4* rec, const float* c1, const float* c2, const float* s, int32_t B,
                                                              int64_t per_sample, int32_t cols, int32_t clip, float* xpad, int64_t ldpad, void* stream) {
    if (s && !noise) return AFM_E_BADARG;          // (the loops hand their noise in: no Philox draw inside this launch)
    CfgUpd p = {};
    p.x0c = x0_c; p.x0u = x0_u; p.scale = scale; p.xt = x; p.xn = x; p.noise = noise; p.per_sample = per_sample; p.clip = clip ? 1 : 0;
    p.cols = cols; p.xpad = xpad; p.ldpad = ldpad;
    if (rec) { p.ddim = 1; p.rec = rec; p.sg = s; }
    else { p.c1 = c1; p.c2 = c2; p.sg = s; }
    return launch_cfg_update(p, B, stream);
}
