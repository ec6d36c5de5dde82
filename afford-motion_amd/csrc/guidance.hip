// Contact guidance (afm_contact_guidance): the analytic gradient and value of the energy between the contact map a motion implies and the
// map it was given - a cond_fn of the samplers without a second network and without autograd.  Two launches, no atomics: every sum has a
// fixed order and reads one sample's data only, so a sample's result does not depend on the batch it is computed in.
#include "sample_loop.h"

namespace {

constexpr int GUIDE_LDS_BYTES = 60 * 1024;          // the sample's K x L joint positions, staged by both passes' first

struct GuideDev {
    const float *q, *c, *mean, *std, *scale;
    int cols[AFM_GUIDE_MAX_JOINTS];
    int K, N, L, D, nblk;
    float two_s2, coef;             // 2 sigma^2 and 2 / (N K sigma^2), rounded once from float64
    int64_t t_start;
};

// the column list into LDS with static indices (a dynamic index into the by-value argument would put the array in scratch)
__device__ __forceinline__ void stage_cols(const GuideDev& g, int* scols) {
#pragma unroll
    for (int k = 0; k < AFM_GUIDE_MAX_JOINTS; ++k)
        if (threadIdx.x == k) scols[k] = g.cols[k];
}

// p = x * std + mean of one coordinate, each operation rounded on its own: both passes call this, so they see the same positions
__device__ __forceinline__ float joint_coord(const float* __restrict__ xrow, const GuideDev& g, int col) {
#pragma clang fp contract(off)
    const float m = xrow[col] * g.std[col];
    return m + g.mean[col];
}

// Pass 1, one thread per (k, n) of sample blockIdx.y (e = k * N + n: a wave shares k but for one boundary): the minimum of
// d2 = (dx*dx + dy*dy) + dz*dz over the valid frames and the FIRST frame that attains it (strict <), chat = exp(-d2 / two_s2) (no valid
// frame: f* = -1, chat = 0), w = (chat - c) * chat; the block's sum of (chat - c)^2 in a fixed order into partial[b][block].
__global__ __launch_bounds__(256) void guide_nearest_kernel(const GuideDev g, const float* __restrict__ x, const uint8_t* __restrict__ fmask,
                                                            int* __restrict__ fstar, float* __restrict__ w, float* __restrict__ partial) {
#pragma clang fp contract(off)
    extern __shared__ float sp[];                   // [K][L][3] positions, then [L] validity
    __shared__ int scols[AFM_GUIDE_MAX_JOINTS];
    __shared__ float red[4];
    const int b = blockIdx.y, K = g.K, N = g.N, L = g.L;
    int* sval = reinterpret_cast<int*>(sp + (size_t)K * L * 3);
    stage_cols(g, scols);
    __syncthreads();
    for (int i = threadIdx.x; i < K * L; i += 256) {
        const int k = i / L, f = i - k * L;
        const float* xrow = x + ((int64_t)b * L + f) * g.D;
#pragma unroll
        for (int a = 0; a < 3; ++a) sp[i * 3 + a] = joint_coord(xrow, g, scols[k] + a);
    }
    for (int f = threadIdx.x; f < L; f += 256) sval[f] = !(fmask && fmask[(int64_t)b * L + f]);
    __syncthreads();
    const int e = blockIdx.x * 256 + threadIdx.x;
    float sq = 0.f;
    if (e < K * N) {
        const int k = e / N, n = e - k * N;
        const float* qp = g.q + ((int64_t)b * N + n) * 3;
        const float qx = qp[0], qy = qp[1], qz = qp[2];
        const float* pk = sp + (size_t)k * L * 3;
        float best = INFINITY;
        int bf = -1;
        for (int f = 0; f < L; ++f) {
            if (!sval[f]) continue;
            const float dx = pk[f * 3] - qx, dy = pk[f * 3 + 1] - qy, dz = pk[f * 3 + 2] - qz;
            const float xx = dx * dx, yy = dy * dy, zz = dz * dz;
            const float d2 = (xx + yy) + zz;
            if (d2 < best) { best = d2; bf = f; }
        }
        const float chat = bf >= 0 ? expf(-best / g.two_s2) : 0.f;
        const float df = chat - g.c[((int64_t)b * N + n) * K + k];
        const int64_t o = ((int64_t)b * K + k) * N + n;
        fstar[o] = bf;
        w[o] = df * chat;
        sq = df * df;
    }
    sq = wave_sum(sq);
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = sq;
    __syncthreads();
    if (threadIdx.x == 0) partial[(int64_t)b * g.nblk + blockIdx.x] = ((red[0] + red[1]) + red[2]) + red[3];
}

// Pass 2, one block per (frame blockIdx.x, sample blockIdx.y), wave v the joints k = v, v + 4, ...: S_a = sum over the points n with
// f*(b, n, k) == f of w * (p_a - q_a) - lane l adds n = l, l + 64, ... in that order, then the fixed butterfly of wave_sum - and
// grad[b, f, cols[k] + a] = ((scale[b] * coef) * std_a) * S_a.  Every other column of the row, and the whole row of a masked frame or of a
// sample with t[b] >= t_start, is written as zero.  Block 0 of a sample adds its energy partials in order: energy[b] = sum / (N K).
__global__ __launch_bounds__(256) void guide_gather_kernel(const GuideDev g, const float* __restrict__ x, const uint8_t* __restrict__ fmask,
                                                           const int64_t* __restrict__ t, const int* __restrict__ fstar,
                                                           const float* __restrict__ w, const float* __restrict__ partial,
                                                           float* __restrict__ grad, float* __restrict__ energy) {
#pragma clang fp contract(off)
    __shared__ int scols[AFM_GUIDE_MAX_JOINTS];
    const int b = blockIdx.y, f = blockIdx.x, K = g.K, N = g.N;
    stage_cols(g, scols);
    __syncthreads();
    if (f == 0 && energy && threadIdx.x == 0) {
        float s = 0.f;
        for (int i = 0; i < g.nblk; ++i) s += partial[(int64_t)b * g.nblk + i];
        energy[b] = s / (float)((int64_t)N * K);
    }
    if (!grad) return;
    float* row = grad + ((int64_t)b * g.L + f) * g.D;
    const bool guided = !(fmask && fmask[(int64_t)b * g.L + f]) && !(t && t[b] >= g.t_start);
    for (int d = threadIdx.x; d < g.D; d += 256) {
        bool named = false;
        for (int k = 0; k < K; ++k) named = named || (d >= scols[k] && d < scols[k] + 3);
        if (!guided || !named) row[d] = 0.f;
    }
    if (!guided) return;
    const float* xrow = x + ((int64_t)b * g.L + f) * g.D;
    const int lane = threadIdx.x & 63;
    const float ks = g.scale[b] * g.coef;
    for (int k = threadIdx.x >> 6; k < K; k += 4) {
        const int col = scols[k];
        const float p0 = joint_coord(xrow, g, col), p1 = joint_coord(xrow, g, col + 1), p2 = joint_coord(xrow, g, col + 2);
        const int64_t o = ((int64_t)b * K + k) * N;
        float s0 = 0.f, s1 = 0.f, s2 = 0.f;
        for (int n = lane; n < N; n += 64) {
            if (fstar[o + n] != f) continue;
            const float ww = w[o + n];
            const float* qp = g.q + ((int64_t)b * N + n) * 3;
            const float m0 = ww * (p0 - qp[0]), m1 = ww * (p1 - qp[1]), m2 = ww * (p2 - qp[2]);
            s0 = s0 + m0; s1 = s1 + m1; s2 = s2 + m2;
        }
        s0 = wave_sum(s0); s1 = wave_sum(s1); s2 = wave_sum(s2);
        if (lane < 3) {
            const float s = lane == 0 ? s0 : (lane == 1 ? s1 : s2);
            const float kss = ks * g.std[col + lane];
            row[col + lane] = kss * s;
        }
    }
}

int64_t guide_nblk(int N, int K) { return ((int64_t)N * K + 255) / 256; }

}  // namespace

extern "C" int64_t afm_contact_guidance_workspace_bytes(int32_t B, int32_t N, int32_t K) {
    if (B < 0 || N <= 0 || K <= 0 || K > AFM_GUIDE_MAX_JOINTS) return AFM_E_BADARG;
    const int64_t nk = (int64_t)B * N * K;
    return 2 * afm_loop::align256(nk * 4) + afm_loop::align256((int64_t)B * guide_nblk(N, K) * 4);
}

// what a description must satisfy before anything is enqueued (L, D: the motion's)
__attribute__((visibility("hidden"))) int afm_contact_guide_check(const afm_contact_guide* a, int32_t L, int32_t D) {
    if (!a || !a->q || !a->c || !a->mean || !a->std || !a->scale || L <= 0 || D <= 0) return AFM_E_BADARG;
    if (a->K <= 0 || a->K > AFM_GUIDE_MAX_JOINTS || a->N <= 0 || !(a->sigma > 0.0) || (int64_t)a->N * a->K > (int64_t)1 << 30) return AFM_E_BADARG;
    for (int k = 0; k < a->K; ++k) {
        if (a->cols[k] < 0 || a->cols[k] + 3 > D) return AFM_E_BADARG;
        for (int j = 0; j < k; ++j)
            if (a->cols[k] < a->cols[j] + 3 && a->cols[j] < a->cols[k] + 3) return AFM_E_BADARG;          // overlapping triples
    }
    if (((size_t)a->K * L * 3 + L) * 4 > (size_t)GUIDE_LDS_BYTES || L > 65535) return AFM_E_UNSUPPORTED;
    return 0;
}

// the samples [start, start + count) of the description's batch; x, frame_mask, t, grad, energy already point at sample `start`
__attribute__((visibility("hidden"))) int afm_contact_guidance_sub(const afm_contact_guide* a, int32_t start, const float* x, const uint8_t* frame_mask,
                                                                   const int64_t* t, float* grad, float* energy, int32_t count, int32_t L, int32_t D,
                                                                   void* workspace, int64_t workspace_bytes, void* stream) {
    const int rc = afm_contact_guide_check(a, L, D);
    if (rc != 0) return rc;
    if (!x || (!grad && !energy) || start < 0 || count < 0) return AFM_E_BADARG;
    if (count > 65535) return AFM_E_UNSUPPORTED;
    const size_t lds = ((size_t)a->K * L * 3 + L) * 4;
    if (count == 0) return 0;
    const int64_t need = afm_contact_guidance_workspace_bytes(count, a->N, a->K);
    if (!workspace || workspace_bytes < need) return AFM_E_WORKSPACE;
    GuideDev g = {};
    g.q = a->q + (int64_t)start * a->N * 3; g.c = a->c + (int64_t)start * a->N * a->K; g.mean = a->mean; g.std = a->std; g.scale = a->scale + start;
    for (int k = 0; k < a->K; ++k) g.cols[k] = a->cols[k];
    g.K = a->K; g.N = a->N; g.L = L; g.D = D; g.nblk = (int)guide_nblk(a->N, a->K);
    g.two_s2 = (float)(2.0 * a->sigma * a->sigma);
    g.coef = (float)(2.0 / ((double)a->N * a->K * a->sigma * a->sigma));
    g.t_start = a->t_start;
    char* wp = (char*)workspace;
    const int64_t nk = (int64_t)count * a->N * a->K;
    int* fstar = (int*)wp; wp += afm_loop::align256(nk * 4);
    float* w = (float*)wp; wp += afm_loop::align256(nk * 4);
    float* partial = (float*)wp;
    hipStream_t s = (hipStream_t)stream;
    hipLaunchKernelGGL(guide_nearest_kernel, dim3((unsigned)g.nblk, (unsigned)count), dim3(256), lds, s, g, x, frame_mask, fstar, w, partial);
    AFM_CHECK_LAUNCH();
    hipLaunchKernelGGL(guide_gather_kernel, dim3(grad ? (unsigned)L : 1u, (unsigned)count), dim3(256), 0, s, g, x, frame_mask, t, fstar, w, partial, grad,
                       energy);
    AFM_CHECK_LAUNCH();
    return 0;
}

extern "C" int afm_contact_guidance(const afm_contact_guide* g, const float* x, const uint8_t* frame_mask, const int64_t* t, float* grad,
                                    float* energy, int32_t B, int32_t L, int32_t D, void* workspace, int64_t workspace_bytes, void* stream) {
    return afm_contact_guidance_sub(g, 0, x, frame_mask, t, grad, energy, B, L, D, workspace, workspace_bytes, stream);
}
