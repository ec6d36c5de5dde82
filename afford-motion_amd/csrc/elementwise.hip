// LayerNorm, the sampling update (DDPM, DDIM, DPM-Solver++(2M), guided), Philox normal generator.
// All three are HBM/L2-streaming kernels: float4 accesses, one wave per LayerNorm row.
#include "profile.h"
#include "sample_loop.h"

namespace {

// grid of a grid-stride elementwise launch over n items per (y, z) slice: 256-thread blocks, at most `cap` of them along x
inline dim3 stream_grid(int64_t n, int64_t cap, int y = 1, int z = 1) {
    const int64_t g = (n + 255) / 256;
    return dim3((unsigned)(g < cap ? g : cap), (unsigned)y, (unsigned)z);
}
inline int64_t quads(int64_t per_sample) { return (per_sample + 3) >> 2; }

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

// The sampling update of sample_loop.h (afm_loop::Update), one quad of a sample per thread iteration: v = x0, or cfg_combine(x0, x0_u,
// scale[b]) when guided (cfg_combine2(x0, x0_a, x0_u, scale[b], scale2[b]) with a middle branch), then known where mask is set (a select: known is not read where mask == 0; the mask by byte loads, a sample's base
// need not be 4-aligned), clamped if asked; then ddpm_update (rows c1 / c2 / sg per sample) or ddim_update (rows rec, or ra..rd, per sample;
// sg == NULL: no noise term).  Every operation is one of common.h's individually rounded helpers (the reference's float32 torch expression,
// bit for bit).  xn may alias xt (one thread reads then writes an element).  noise == NULL with a noise term: Philox keyed by the quad q.
// xpad: x_next also into rows of ldpad floats (the next motion-adapter GEMM's K-padded A rows; columns >= cols stay zero).
// dpm: dpm_update on the rows {a, b, c} instead (x0_prev NULL: its two-term form), v - the final x0 - also stored to x0_keep when asked.
// grad (cond_fn guidance, with its per-sample coefficient gk), float32, each operation rounded on its own:
//   DDIM / 2M:  m = gk[b] * grad;  v = v + m          after the clamp; this shifted v enters the update and is what x0_keep stores
//   DDPM:       m = gk[b] * grad;  x_next = ((c1 * v + c2 * x_t) + m) + sg * noise          (guided_ddpm_update)
// grad == NULL: the kernel computes what it computed without the term, and grad is never read.
__device__ __forceinline__ float guided_x0(float v, float gk, float grad) {
#pragma clang fp contract(off)
    const float m = gk * grad;
    return v + m;
}
__device__ __forceinline__ float guided_ddpm_update(float x0, float xt, float c1, float c2, float sg, float nz, float gk, float grad) {
#pragma clang fp contract(off)
    const float m1 = c1 * x0;
    const float m2 = c2 * xt;
    const float mean = guided_x0(m1 + m2, gk, grad);
    const float sn = sg * nz;
    return mean + sn;
}
__global__ __launch_bounds__(256) void sampling_update_kernel(const afm_loop::Update p) {
    const int b = blockIdx.y;
    const float s = p.x0_u ? p.scale[b] : 0.f;
    const float s2 = p.x0_a ? p.scale2[b] : 0.f;
    const float sg = p.sg ? p.sg[b] : 0.f;
    const float gk = p.grad ? p.gk[b] : 0.f;
    float4 r = make_float4(0.f, 1.f, 0.f, 0.f);
    float c1 = 0.f, c2 = 0.f;
    if (p.ddim) r = p.rec ? p.rec[b] : make_float4(p.ra[b], p.rb[b], p.rc[b], p.rd ? p.rd[b] : 0.f);
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
                float v = p.x0[g];
                if (p.x0_a) v = cfg_combine2(v, p.x0_a[g], p.x0_u[g], s, s2);
                else if (p.x0_u) v = cfg_combine(v, p.x0_u[g], s);
                if (p.mask && p.mask[g]) v = p.known[g];
                if (p.clip) v = v < -1.0f ? -1.0f : (v > 1.0f ? 1.0f : v);          // clip_denoised (NaN passes through, as torch.clamp)
                const float nz = p.sg ? (p.noise ? p.noise[g] : z[e]) : 0.f;
                const float vt = p.xt[g];
                float xn;
                if (p.grad && p.ddim) v = guided_x0(v, gk, p.grad[g]);
                if (p.dpm) {
                    xn = p.x0_prev ? dpm_update(v, vt, r, p.x0_prev[g]) : dpm_update(v, vt, r);
                    if (p.x0_keep) p.x0_keep[g] = v;
                } else if (p.ddim) {
                    xn = p.sg ? ddim_update(v, vt, r, sg, nz) : ddim_update(v, vt, r);
                    if (p.x0_keep) p.x0_keep[g] = v;
                }
                else if (p.grad) xn = guided_ddpm_update(v, vt, c1, c2, sg, nz, gk, p.grad[g]);
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
    hipLaunchKernelGGL(clamp_kernel, stream_grid(n, 4096), dim3(256), 0, (hipStream_t)stream, x, n, lo, hi);
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
    hipLaunchKernelGGL(contact_glue_kernel, stream_grid(n, 4096), dim3(256), 0, (hipStream_t)stream, sample, out, n, sigma_sq, mean, std);
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

// ---- the sampling update: one launcher behind afm_ddpm_step, afm_ddim_step, afm_dpm_step, afm_cfg_step and the update launch of the native loops
namespace {
int enqueue_update(const afm_loop::Update& p, int32_t B, hipStream_t s) {
    hipLaunchKernelGGL(sampling_update_kernel, stream_grid(quads(p.per_sample), 1024, B), dim3(256), 0, s, p);
    AFM_CHECK_LAUNCH();
    return 0;
}
}  // namespace

__attribute__((visibility("hidden"))) int afm_sampling_update(const afm_loop::Update& p, int32_t B, void* stream) {
    if (!p.x0 || !p.xt || !p.xn || !p.x0_u != !p.scale || !p.known != !p.mask || B < 0 || p.per_sample <= 0) return AFM_E_BADARG;
    if (!p.x0_a != !p.scale2 || (p.x0_a && !p.x0_u)) return AFM_E_BADARG;          // a middle branch: both scales and the unconditioned branch
    if (p.ddim ? !(p.rec || (p.ra && p.rb && p.rc && (p.rd || p.dpm))) : !(p.c1 && p.c2 && p.sg)) return AFM_E_BADARG;
    if (p.dpm ? (!p.ddim || p.sg) : (p.x0_prev || (p.x0_keep && !(p.ddim && p.grad)))) return AFM_E_BADARG;          // 2M: DDIM-layout rows, no noise term; history only there
    if (!p.grad != !p.gk) return AFM_E_BADARG;          // cond_fn guidance: the gradient and its coefficient row go together
    if (p.sg && !p.noise && !p.philox) return AFM_E_BADARG;          // (the loops hand their noise in: no Philox draw inside their launch)
    if (p.xpad && (p.cols <= 0 || p.ldpad < p.cols)) return AFM_E_BADARG;
    if (B == 0) return 0;
    if (!p.x0_u) return enqueue_update(p, B, (hipStream_t)stream);
    AfmProf prof(AFM_PROF_MISC, (p.x0_a ? 6.0 : 5.0) * B * p.per_sample, (hipStream_t)stream);          // (profiling records: the guided launches only)
    return enqueue_update(p, B, (hipStream_t)stream);
}

namespace {
// the update of a public single-step entry point: out of place, noise given or drawn in the kernel
afm_loop::Update step_update(const float* x0, const float* x_t, const float* noise, float* x_next, int64_t per_sample, uint64_t seed,
                             int64_t sample_index0, int32_t step) {
    afm_loop::Update p = {};
    p.x0 = x0; p.xt = x_t; p.noise = noise; p.xn = x_next; p.per_sample = per_sample;
    p.philox = 1; p.seed = seed; p.sample0 = sample_index0; p.step = step;
    return p;
}
void set_ddim_rows(afm_loop::Update* p, const afm_ddim_rows* r) {
    p->ddim = 1; p->ra = r->a; p->rb = r->b; p->rc = r->c; p->rd = r->d; p->sg = r->sigma;
}
// what the afm_*_step_args entry points share (A: any of the three structs): step_update, the clamp, either kind of rows
template <class A>
afm_loop::Update args_update(const A* a) {
    afm_loop::Update p = step_update(a->x0_c, a->x_t, a->noise, a->x_next, a->per_sample, a->seed, a->sample_index0, a->step);
    p.clip = a->clip ? 1 : 0;
    if (a->ddim) set_ddim_rows(&p, a->ddim);
    else { p.c1 = a->c1; p.c2 = a->c2; p.sg = a->sigma; }
    return p;
}
}  // namespace

extern "C" int afm_ddpm_step(const float* x0, const float* x_t, const float* noise, float* x_next, const float* c1,
                             const float* c2, const float* sigma, int32_t B, int64_t per_sample, uint64_t seed,
                             int64_t sample_index0, int32_t step, void* stream) {
    afm_loop::Update p = step_update(x0, x_t, noise, x_next, per_sample, seed, sample_index0, step);
    p.c1 = c1; p.c2 = c2; p.sg = sigma;
    return afm_sampling_update(p, B, stream);
}

extern "C" int afm_ddim_step(const float* x0, const float* x_t, const float* noise, float* x_next, const afm_ddim_rows* rows,
                             int32_t B, int64_t per_sample, uint64_t seed, int64_t sample_index0, int32_t step, void* stream) {
    if (!rows) return AFM_E_BADARG;
    afm_loop::Update p = step_update(x0, x_t, noise, x_next, per_sample, seed, sample_index0, step);
    set_ddim_rows(&p, rows);
    return afm_sampling_update(p, B, stream);
}

extern "C" int afm_dpm_step(const float* x0, const float* x_t, const float* x0_prev, float* x_next, const afm_dpm_rows* rows, int32_t B,
                            int64_t per_sample, void* stream) {
    if (!rows) return AFM_E_BADARG;
    afm_loop::Update p = {};
    p.x0 = x0; p.xt = x_t; p.xn = x_next; p.per_sample = per_sample; p.x0_prev = x0_prev;
    p.ddim = 1; p.dpm = 1; p.ra = rows->a; p.rb = rows->b; p.rc = rows->c;
    return afm_sampling_update(p, B, stream);
}

extern "C" int afm_cfg_step(const afm_cfg_step_args* a, void* stream) {
    if (!a || !a->x0_c || !a->x0_u || !a->scale) return AFM_E_BADARG;
    afm_loop::Update p = args_update(a);
    p.x0_u = a->x0_u; p.scale = a->scale;
    return afm_sampling_update(p, a->B, stream);
}

extern "C" int afm_cfg2_step(const afm_cfg2_step_args* a, void* stream) {
    if (!a || !a->x0_c || !a->x0_a || !a->x0_u || !a->scale_first || !a->scale_second || !a->known != !a->mask) return AFM_E_BADARG;
    afm_loop::Update p = args_update(a);
    p.x0_a = a->x0_a; p.x0_u = a->x0_u; p.scale = a->scale_first; p.scale2 = a->scale_second;
    p.known = a->known; p.mask = a->mask;
    return afm_sampling_update(p, a->B, stream);
}

extern "C" int afm_impute_step(const afm_impute_step_args* a, void* stream) {
    if (!a || !a->x0_c || !a->known || !a->mask) return AFM_E_BADARG;
    afm_loop::Update p = args_update(a);
    p.x0_u = a->x0_u; p.scale = a->scale; p.known = a->known; p.mask = a->mask;
    return afm_sampling_update(p, a->B, stream);
}

extern "C" int afm_guide_step(const afm_guide_step_args* a, void* stream) {
    if (!a || !a->x0_c || !a->known != !a->mask) return AFM_E_BADARG;
    if ((a->ddim != nullptr) + (a->dpm != nullptr) + (a->c1 || a->c2 || a->sigma ? 1 : 0) != 1) return AFM_E_BADARG;          // one kind of rows
    if (a->dpm && !(a->dpm->a && a->dpm->b && a->dpm->c)) return AFM_E_BADARG;
    afm_loop::Update p = step_update(a->x0_c, a->x_t, a->noise, a->x_next, a->per_sample, a->seed, a->sample_index0, a->step);
    p.clip = a->clip ? 1 : 0;
    if (a->ddim) set_ddim_rows(&p, a->ddim);
    else if (a->dpm) { p.ddim = 1; p.dpm = 1; p.ra = a->dpm->a; p.rb = a->dpm->b; p.rc = a->dpm->c; p.x0_prev = a->x0_prev; p.noise = nullptr; }
    else { p.c1 = a->c1; p.c2 = a->c2; p.sg = a->sigma; }
    if (a->x0_prev && !a->dpm) return AFM_E_BADARG;
    p.x0_a = a->x0_a; p.x0_u = a->x0_u; p.scale = a->scale; p.scale2 = a->scale2;
    p.known = a->known; p.mask = a->mask; p.grad = a->grad; p.gk = a->gk; p.x0_keep = a->x0_out;
    return afm_sampling_update(p, a->B, stream);
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
    hipLaunchKernelGGL(randn_kernel, stream_grid(quads(per_sample), 1024, B, nsteps), dim3(256), 0, (hipStream_t)stream, out, per_sample, seed, sample_index0, step0);
    AFM_CHECK_LAUNCH();
    return 0;
}

extern "C" int afm_randn(float* out, int32_t B, int64_t per_sample, uint64_t seed, int64_t sample_index0, int32_t step,
                         void* stream) {
    return afm_randn_steps(out, B, per_sample, seed, sample_index0, step, 1, stream);
}

// ---- classifier-free guidance of an x0 alone (the guided updates are the sampling update above)
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

// x0_guided = cfg_combine2(x0_c, x0_a, x0_u, scale_first[b], scale_second[b]) per element
__global__ __launch_bounds__(256) void cfg2_combine_kernel(const float* __restrict__ x0c, const float* __restrict__ x0a, const float* __restrict__ x0u,
                                                           const float* __restrict__ s1, const float* __restrict__ s2, float* __restrict__ out,
                                                           int64_t per_sample) {
    const int b = blockIdx.y;
    const float sa = s1[b], sb = s2[b];
    const int64_t base = (int64_t)b * per_sample;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < per_sample; i += (int64_t)gridDim.x * blockDim.x)
        out[base + i] = cfg_combine2(x0c[base + i], x0a[base + i], x0u[base + i], sa, sb);
}

}  // namespace

// ---- imputation of an x0 alone (the imputing updates are the sampling update above)
namespace {
__global__ __launch_bounds__(256) void impute_kernel(const float* __restrict__ known, const uint8_t* __restrict__ mask, const float* x0, float* out,
                                                     int64_t n) {
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x)
        out[i] = mask[i] ? known[i] : x0[i];          // out may alias x0: one thread reads then writes an element
}
}  // namespace

extern "C" int afm_impute(const float* x0, const float* known, const uint8_t* mask, float* out, int64_t n, void* stream) {
    if (n == 0) return 0;
    if (!x0 || !known || !mask || !out || n < 0) return AFM_E_BADARG;
    hipLaunchKernelGGL(impute_kernel, stream_grid(n, 4096), dim3(256), 0, (hipStream_t)stream, known, mask, x0, out, n);
    AFM_CHECK_LAUNCH();
    return 0;
}

extern "C" int afm_cfg_combine(const float* x0_c, const float* x0_u, const float* scale, float* out, int32_t B, int64_t per_sample, void* stream) {
    if (!x0_c || !x0_u || !scale || !out || B < 0 || per_sample <= 0) return AFM_E_BADARG;
    if (B == 0) return 0;
    AfmProf prof(AFM_PROF_MISC, 3.0 * B * per_sample, (hipStream_t)stream);
    hipLaunchKernelGGL(cfg_combine_kernel, stream_grid(per_sample, 1024, B), dim3(256), 0, (hipStream_t)stream, x0_c, x0_u, scale, out, per_sample);
    AFM_CHECK_LAUNCH();
    return 0;
}

extern "C" int afm_cfg2_combine(const float* x0_c, const float* x0_a, const float* x0_u, const float* scale_first, const float* scale_second,
                                float* out, int32_t B, int64_t per_sample, void* stream) {
    if (!x0_c || !x0_a || !x0_u || !scale_first || !scale_second || !out || B < 0 || per_sample <= 0) return AFM_E_BADARG;
    if (B == 0) return 0;
    AfmProf prof(AFM_PROF_MISC, 4.0 * B * per_sample, (hipStream_t)stream);
    hipLaunchKernelGGL(cfg2_combine_kernel, stream_grid(per_sample, 1024, B), dim3(256), 0, (hipStream_t)stream, x0_c, x0_a, x0_u, scale_first,
                       scale_second, out, per_sample);
    AFM_CHECK_LAUNCH();
    return 0;
}
