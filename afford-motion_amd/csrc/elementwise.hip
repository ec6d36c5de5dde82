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
// the combined pred_xstart of element g of a sample with the scales s / s2: x0, or cfg_combine / cfg_combine2 of the branches
__device__ __forceinline__ float combined_x0(const afm_loop::Update& p, int64_t g, float s, float s2) {
    const float v = p.x0[g];
    if (p.x0_a) return cfg_combine2(v, p.x0_a[g], p.x0_u[g], s, s2);
    if (p.x0_u) return cfg_combine(v, p.x0_u[g], s);
    return v;
}
// STITCH (afm_loop::Update: st_*): between the combine and the select, the elements of a frame two windows share become stitch_blend of
// the two windows' combined x0, the neighbour's read st_ov * st_D values further on in its own sample (the later window's first frames)
// or back (the earlier window's last frames), with the neighbour's scales - decided per element (per_sample need not be a multiple of
// 4: a quad may straddle the edge of an overlap).  The unstitched instantiation is the kernel as it was.
template <bool STITCH>
__global__ __launch_bounds__(256) void sampling_update_kernel(const afm_loop::Update p) {
    const int b = blockIdx.y;
    const float s = p.x0_u ? p.scale[b] : 0.f;
    const float s2 = p.x0_a ? p.scale2[b] : 0.f;
    // stitched: the edges of the window's two overlaps inside the sample [0, st_lo) and [st_hi, per_sample), the neighbours' scales
    int64_t st_lo = 0, st_hi = 0;
    bool has_left = false, has_right = false;
    float sl = 0.f, sl2 = 0.f, sr = 0.f, sr2 = 0.f;
    if constexpr (STITCH) {
        const int w = b % p.st_S;
        has_left = w > 0;                    // an earlier window shares this one's first st_ov frames
        has_right = w + 1 < p.st_S;          // a later window shares this one's last st_ov frames
        st_lo = (int64_t)p.st_ov * p.st_D;
        st_hi = p.per_sample - st_lo;
        if (has_left) { sl = p.x0_u ? p.scale[b - 1] : 0.f; sl2 = p.x0_a ? p.scale2[b - 1] : 0.f; }
        if (has_right) { sr = p.x0_u ? p.scale[b + 1] : 0.f; sr2 = p.x0_a ? p.scale2[b + 1] : 0.f; }
    }
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
                if constexpr (STITCH) {
                    if (has_right && i >= st_hi) {               // this window is the left one of the pair
                        const int k = (int)((i - st_hi) / p.st_D);
                        v = stitch_blend(v, combined_x0(p, g + st_lo, sr, sr2), p.st_w[k], p.st_w[p.st_ov + k]);
                    } else if (has_left && i < st_lo) {          // the right one
                        const int k = (int)(i / p.st_D);
                        v = stitch_blend(combined_x0(p, g - st_lo, sl, sl2), v, p.st_w[k], p.st_w[p.st_ov + k]);
                    }
                }
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
    if (B == 0) return 0;                                     // empty batch (pointers may be null), as afm_masked_mse_bwd
    if (!target || !pred || !out || B < 0 || L <= 0 || D <= 0) return AFM_E_BADARG;
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
    if (p.stitched()) hipLaunchKernelGGL(sampling_update_kernel<true>, stream_grid(quads(p.per_sample), 1024, B), dim3(256), 0, s, p);
    else hipLaunchKernelGGL(sampling_update_kernel<false>, stream_grid(quads(p.per_sample), 1024, B), dim3(256), 0, s, p);
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
    if (p.st_S != 0 || p.st_ov != 0) {          // stitched windows: whole long motions, a frame in at most two windows, a deterministic update
        if (p.st_S < 1 || p.st_ov < 0 || p.st_L <= 0 || p.st_D <= 0 || (int64_t)p.st_L * p.st_D != p.per_sample || 2 * (int64_t)p.st_ov > p.st_L ||
            B % p.st_S != 0 || !p.ddim || p.sg || (p.stitched() && !p.st_w)) return AFM_E_BADARG;
        if (p.x0_keep && (p.x0_keep == p.x0 || p.x0_keep == p.x0_u || p.x0_keep == p.x0_a)) return AFM_E_BADARG;
        if (p.xn == p.x0 || p.xn == p.x0_u || p.xn == p.x0_a) return AFM_E_BADARG;          // (the neighbour's x0 is read by another thread)
    }
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

// ---- stitched windows of long motions (afm_stitch): B = G * S samples [B][L][D], sample g * S + w window w of long motion g, holding the
// long frames w * (L - ov) .. w * (L - ov) + L - 1.  The same elementwise family as above: no atomics, one writer per element.
namespace {

// the blend of an x0 alone.  One thread owns BOTH elements of a shared frame (it runs over the earlier window's copy, reads the two, writes
// the one value to both), an element outside every overlap is copied: out may be x0.
__global__ __launch_bounds__(256) void stitch_blend_kernel(const float* x0, float* out, const float* __restrict__ wrow, int S, int ov, int D,
                                                           int64_t per_sample) {
    const int b = blockIdx.y;
    const int w = b % S;
    const int64_t lo = (int64_t)ov * D, hi = per_sample - lo;
    const int64_t base = (int64_t)b * per_sample;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < per_sample; i += (int64_t)gridDim.x * blockDim.x) {
        const int64_t g = base + i;
        if (w + 1 < S && i >= hi) {
            const int k = (int)((i - hi) / D);
            const float v = stitch_blend(x0[g], x0[g + lo], wrow[k], wrow[ov + k]);
            out[g] = v;
            out[g + lo] = v;
        } else if (!(w > 0 && i < lo)) {
            out[g] = x0[g];
        }
    }
}

// windows [G * S][L][D] of long [G][F][D]: copies; a frame at or behind F (the padded tail of the last window) is zero
__global__ __launch_bounds__(256) void stitch_windows_kernel(const float* __restrict__ lng, float* __restrict__ win, int S, int ov, int L, int D, int F) {
    const int b = blockIdx.y;
    const int g = b / S, w = b % S;
    const int64_t per = (int64_t)L * D;
    const int64_t first = (int64_t)w * (L - ov);
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < per; i += (int64_t)gridDim.x * blockDim.x) {
        const int64_t f = first + i / D;
        win[(int64_t)b * per + i] = f < F ? lng[((int64_t)g * F) * D + first * D + i] : 0.f;
    }
}

// long [G][F][D] of windows [G * S][L][D]: copies; a shared frame is read from the later window (both hold the same bits after a
// stitched chain)
__global__ __launch_bounds__(256) void stitch_join_kernel(const float* __restrict__ win, float* __restrict__ lng, int S, int ov, int L, int D, int F) {
    const int g = blockIdx.y;
    const int64_t per = (int64_t)F * D;
    const int P = L - ov;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < per; i += (int64_t)gridDim.x * blockDim.x) {
        const int64_t f = i / D;
        int64_t w = f / P;
        if (w > S - 1) w = S - 1;
        lng[(int64_t)g * per + i] = win[(((int64_t)g * S + w) * L) * D + (i - w * P * D)];
    }
}

// the geometry of a stitch description against a batch: whole long motions, a frame in at most two windows
inline bool stitch_ok(int S, int ov, int L, int D) { return S >= 1 && ov >= 0 && L > 0 && D > 0 && 2 * (int64_t)ov <= L; }

}  // namespace

extern "C" int afm_stitch_blend(const float* x0, float* out, const afm_stitch* st, int32_t B, int32_t L, int32_t D, void* stream) {
    if (!st || !stitch_ok(st->windows, st->overlap, L, D) || B < 0 || B % st->windows != 0) return AFM_E_BADARG;
    if (B == 0) return 0;
    if (!x0 || !out) return AFM_E_BADARG;
    const int64_t per = (int64_t)L * D;
    if (st->windows == 1 || st->overlap == 0) {          // no blend: the input's bits
        if (out != x0 && hipMemcpyAsync(out, x0, (size_t)B * per * 4, hipMemcpyDeviceToDevice, (hipStream_t)stream) != hipSuccess) return (int)hipGetLastError();
        return 0;
    }
    if (!st->weights) return AFM_E_BADARG;
    hipLaunchKernelGGL(stitch_blend_kernel, stream_grid(per, 1024, B), dim3(256), 0, (hipStream_t)stream, x0, out, st->weights, st->windows, st->overlap, D, per);
    AFM_CHECK_LAUNCH();
    return 0;
}

extern "C" int afm_stitch_windows(const float* long_motion, float* windows, int32_t G, int32_t S, int32_t overlap, int32_t L, int32_t D, int32_t F,
                                  void* stream) {
    if (!stitch_ok(S, overlap, L, D) || G < 0 || F <= (int64_t)(S - 1) * (L - overlap) + (S > 1 ? overlap : 0) || F > (int64_t)S * L - (int64_t)(S - 1) * overlap) return AFM_E_BADARG;
    if (G == 0) return 0;
    if (!long_motion || !windows || (int64_t)G * S > 65535) return AFM_E_BADARG;
    hipLaunchKernelGGL(stitch_windows_kernel, stream_grid((int64_t)L * D, 1024, G * S), dim3(256), 0, (hipStream_t)stream, long_motion, windows, S, overlap, L, D, F);
    AFM_CHECK_LAUNCH();
    return 0;
}

extern "C" int afm_stitch_join(const float* windows, float* long_motion, int32_t G, int32_t S, int32_t overlap, int32_t L, int32_t D, int32_t F,
                               void* stream) {
    if (!stitch_ok(S, overlap, L, D) || G < 0 || F <= (int64_t)(S - 1) * (L - overlap) + (S > 1 ? overlap : 0) || F > (int64_t)S * L - (int64_t)(S - 1) * overlap) return AFM_E_BADARG;
    if (G == 0) return 0;
    if (!long_motion || !windows || G > 65535) return AFM_E_BADARG;
    hipLaunchKernelGGL(stitch_join_kernel, stream_grid((int64_t)F * D, 1024, G), dim3(256), 0, (hipStream_t)stream, windows, long_motion, S, overlap, L, D, F);
    AFM_CHECK_LAUNCH();
    return 0;
}

namespace {
// afm_stitch_step, with the gradient term of afm_stitch_guide_step when grad is given (x0_out: the shifted x0, DDIM rows too)
int stitch_step(const afm_stitch_step_args* a, const float* grad, const float* gk, float* x0_out, void* stream) {
    if (!a || !a->x0_c || !a->stitch || !a->known != !a->mask) return AFM_E_BADARG;
    if ((a->ddim != nullptr) + (a->dpm != nullptr) != 1) return AFM_E_BADARG;          // one kind of rows, both deterministic
    if (a->ddim && a->ddim->sigma) return AFM_E_BADARG;          // (the step noise of shared frames would have to be shared)
    if (a->dpm && !(a->dpm->a && a->dpm->b && a->dpm->c)) return AFM_E_BADARG;
    if (a->x0_prev && !a->dpm) return AFM_E_BADARG;
    if (a->L <= 0 || a->D <= 0) return AFM_E_BADARG;
    afm_loop::Update p = {};
    p.x0 = a->x0_c; p.xt = a->x_t; p.xn = a->x_next; p.per_sample = (int64_t)a->L * a->D; p.clip = a->clip ? 1 : 0;
    if (a->ddim) set_ddim_rows(&p, a->ddim);
    else { p.ddim = 1; p.dpm = 1; p.ra = a->dpm->a; p.rb = a->dpm->b; p.rc = a->dpm->c; p.x0_prev = a->x0_prev; p.x0_keep = a->x0_out; }
    p.x0_a = a->x0_a; p.x0_u = a->x0_u; p.scale = a->scale; p.scale2 = a->scale2;
    p.known = a->known; p.mask = a->mask;
    if (a->x0_out && !a->dpm) return AFM_E_BADARG;
    if (grad) { p.grad = grad; p.gk = gk; if (x0_out) p.x0_keep = x0_out; }
    p.st_S = a->stitch->windows; p.st_ov = a->stitch->overlap; p.st_L = a->L; p.st_D = a->D; p.st_w = a->stitch->weights;
    return afm_sampling_update(p, a->B, stream);
}
}  // namespace

extern "C" int afm_stitch_step(const afm_stitch_step_args* a, void* stream) { return stitch_step(a, nullptr, nullptr, nullptr, stream); }

extern "C" int afm_stitch_guide_step(const afm_stitch_step_args* a, const float* grad, const float* gk, float* x0_out, void* stream) {
    if (!grad || !gk) return AFM_E_BADARG;
    return stitch_step(a, grad, gk, x0_out, stream);
}
