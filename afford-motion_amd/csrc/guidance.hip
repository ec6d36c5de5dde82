// Contact guidance (afm_contact_guidance): the analytic gradient and value of the energy between the contact map a motion implies and the
// map it was given - a cond_fn of the samplers without a second network and without autograd.  Two launches, no atomics: every sum has a
// fixed order and reads one sample's data only, so a sample's result does not depend on the batch it is computed in.
//
// HumanML3D features (`h3d`, afm_h3d_layout): the joints are not columns of x but a function of it - the root's rotation and planar velocities
// integrated over the frames (the reference's recover_from_ric).  A recovery kernel in front of the two passes writes the guided joints'
// scene-frame positions to the workspace, the passes read them from there, pass 2 leaves S[b,f,k,:] in the workspace, and an adjoint kernel
// behind them carries S through the transposed recovery into complete grad rows: four launches, every scan one lane's serial chain.
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

constexpr int H3D_JOINTS = 22;                       // joints of the HumanML3D skeleton
constexpr int H3D_COLS = 4 + 3 * (H3D_JOINTS - 1);   // 67: rotation velocity, two planar velocities, root height, 21 local triples
constexpr int H3D_SCAN_ROWS = 7;                     // per-frame LDS rows of the recovery and of the adjoint

// what the recovery kernel takes: positions of J joints to pos[b * out_b + k * out_j + f * 3]
struct H3dDev {
    const float *mean, *std, *to_scene;              // to_scene: the first sample's [3][4], sample b at b * ts_stride (NULL: identity)
    int joints[H3D_JOINTS];
    int J, L, D, ts_stride;
    int64_t out_b, out_j, out_f;
};

struct H3dAdjDev {
    const float *mean, *std, *scale, *to_scene;
    int joints[AFM_GUIDE_MAX_JOINTS];
    int K, L, D, ts_stride;
    float coef;
    int64_t t_start;
};

// u = x * std + mean of one column, each operation rounded on its own.  Every kernel of this file de-normalises through this, so the
// recovery, the passes, the adjoint and the targets see the same features and the same positions.
__device__ __forceinline__ float denorm(const float* __restrict__ xrow, const float* __restrict__ mean, const float* __restrict__ std, int col) {
#pragma clang fp contract(off)
    const float m = xrow[col] * std[col];
    return m + mean[col];
}

// the column or joint list of a by-value kernel argument into LDS with static indices (a dynamic index into the argument would put the
// array in scratch)
__device__ __forceinline__ void stage_index(const int (&src)[AFM_GUIDE_MAX_JOINTS], int* dst) {
#pragma unroll
    for (int k = 0; k < AFM_GUIDE_MAX_JOINTS; ++k)
        if (threadIdx.x == k) dst[k] = src[k];
}

// the block's sum of one value per thread in a fixed order: the wave butterfly, then ((r0 + r1) + r2) + r3 over the four waves, read and
// added by thread 0 alone, which gets the sum (the others get 0)
__device__ __forceinline__ float block_sum(float v, float* red) {
#pragma clang fp contract(off)
    v = wave_sum(v);
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
    __syncthreads();
    return threadIdx.x == 0 ? ((red[0] + red[1]) + red[2]) + red[3] : 0.f;
}

// [A|t] of sample b into LDS (row-major 3 x 4; NULL: the identity)
__device__ __forceinline__ void stage_to_scene(const float* __restrict__ to_scene, int64_t off, float* sA) {
    if (threadIdx.x < 12) sA[threadIdx.x] = to_scene ? to_scene[off + threadIdx.x] : (threadIdx.x % 5 == 0 ? 1.f : 0.f);
}

// The recovery, one block per sample.  With w, vx, vz = u[f, 0..2] (zero in a padded frame):
//   th_f = sum_{g<f} w_g;  c_f = cosf(2 th_f), s_f = sinf(2 th_f);  dX_f = vx_{f-1} c_f - vz_{f-1} s_f, dZ_f = vx_{f-1} s_f + vz_{f-1} c_f (f >= 1)
//   X_f = sum_{h<=f} dX_h, Z_f likewise;  joint 0: P = (X, u[f,3], Z);  joint j: P = (lx c - lz s + X, ly, lx s + lz c + Z), l = u[f, 4+3(j-1)..]
//   p = (A_r0 P_x + A_r1 P_y) + A_r2 P_z + t_r
// The three scans are serial chains in frame order, f = 0, 1, ..., each on one lane (th on lane 0; then X on lane 0 and Z on lane 64):
// the order depends on nothing at all, not on L, B or the sample's place.  c, s go to cs[b][f][2] (if given) for the adjoint to read back.
__global__ __launch_bounds__(256) void h3d_recover_kernel(const H3dDev h, const float* __restrict__ x, const uint8_t* __restrict__ fmask,
                                                          float* __restrict__ pos, float* __restrict__ cs) {
#pragma clang fp contract(off)
    extern __shared__ float sh[];                   // [H3D_SCAN_ROWS][L]
    __shared__ int sj[H3D_JOINTS];
    __shared__ float sA[12];
    const int b = blockIdx.x, L = h.L;
    float *sth = sh, *sc = sh + L, *ss = sh + 2 * L, *sX = sh + 3 * L, *sZ = sh + 4 * L, *svx = sh + 5 * L, *svz = sh + 6 * L;
#pragma unroll
    for (int k = 0; k < H3D_JOINTS; ++k)
        if (threadIdx.x == k) sj[k] = h.joints[k];
    stage_to_scene(h.to_scene, (int64_t)b * h.ts_stride, sA);
    const float* xb = x + (int64_t)b * L * h.D;
    for (int f = threadIdx.x; f < L; f += 256) {
        const float* xrow = xb + (int64_t)f * h.D;
        const bool pad = fmask && fmask[(int64_t)b * L + f];
        sth[f] = pad ? 0.f : denorm(xrow, h.mean, h.std, 0);
        svx[f] = pad ? 0.f : denorm(xrow, h.mean, h.std, 1);
        svz[f] = pad ? 0.f : denorm(xrow, h.mean, h.std, 2);
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        float acc = 0.f;
        for (int f = 0; f < L; ++f) { const float w = sth[f]; sth[f] = acc; acc = acc + w; }
    }
    __syncthreads();
    for (int f = threadIdx.x; f < L; f += 256) {
        const float a = 2.f * sth[f];
        const float c = cosf(a), s = sinf(a);
        float dX = 0.f, dZ = 0.f;
        if (f > 0) {
            const float vx = svx[f - 1], vz = svz[f - 1];
            dX = vx * c - vz * s;
            dZ = vx * s + vz * c;
        }
        sc[f] = c; ss[f] = s; sX[f] = dX; sZ[f] = dZ;
    }
    __syncthreads();
    if (threadIdx.x == 0 || threadIdx.x == 64) {
        float* v = threadIdx.x == 0 ? sX : sZ;
        float acc = 0.f;
        for (int f = 0; f < L; ++f) { acc = acc + v[f]; v[f] = acc; }
    }
    __syncthreads();
    for (int i = threadIdx.x; i < h.J * L; i += 256) {
        const int k = i / L, f = i - k * L, j = sj[k];
        const float* xrow = xb + (int64_t)f * h.D;
        float Px, Py, Pz;
        if (j == 0) {
            Px = sX[f]; Py = denorm(xrow, h.mean, h.std, 3); Pz = sZ[f];
        } else {
            const int col = 4 + 3 * (j - 1);
            const float lx = denorm(xrow, h.mean, h.std, col), ly = denorm(xrow, h.mean, h.std, col + 1), lz = denorm(xrow, h.mean, h.std, col + 2);
            const float c = sc[f], s = ss[f];
            Px = (lx * c - lz * s) + sX[f];
            Py = ly;
            Pz = (lx * s + lz * c) + sZ[f];
        }
        float* o = pos + (int64_t)b * h.out_b + (int64_t)k * h.out_j + (int64_t)f * h.out_f;
#pragma unroll
        for (int r = 0; r < 3; ++r) o[r] = ((sA[4 * r] * Px + sA[4 * r + 1] * Py) + sA[4 * r + 2] * Pz) + sA[4 * r + 3];
    }
    if (cs)
        for (int f = threadIdx.x; f < L; f += 256) {
            cs[((int64_t)b * L + f) * 2] = sc[f];
            cs[((int64_t)b * L + f) * 2 + 1] = ss[f];
        }
}

// Pass 1 behind its staging, for sample blockIdx.y with the positions in sp[K][L][3] and the [L] validity flags behind them (both staged by
// the front: valid_of_mask, or a window's frame count), one
// thread per (k, n) (e = k * N + n: a wave shares k but for one boundary): the minimum of d2 = (dx*dx + dy*dy) + dz*dz over the valid
// frames and the FIRST frame that attains it (strict <), chat = exp(-d2 / two_s2) (no valid frame: f* = -1, chat = 0),
// w = (chat - c) * chat; the block's sum of (chat - c)^2 in a fixed order into partial[b][block].  Every form's pass 1 is this on its p.
// `first`: the index of staged frame 0 in what fstar counts (a window of a long motion stores long frame indices).

// the validity flags of sample blockIdx.y from its frame mask (NULL: every frame valid)
__device__ __forceinline__ void valid_of_mask(const GuideDev& g, float* sp, const uint8_t* __restrict__ fmask) {
    int* sval = reinterpret_cast<int*>(sp + (size_t)g.K * g.L * 3);
    for (int f = threadIdx.x; f < g.L; f += 256) sval[f] = !(fmask && fmask[(int64_t)blockIdx.y * g.L + f]);
}

__device__ __forceinline__ void nearest_of_staged(const GuideDev& g, float* sp, int* __restrict__ fstar, float* __restrict__ w,
                                                  float* __restrict__ partial, int first = 0) {
#pragma clang fp contract(off)
    __shared__ float red[4];
    const int b = blockIdx.y, K = g.K, N = g.N, L = g.L;
    const int* sval = reinterpret_cast<const int*>(sp + (size_t)K * L * 3);
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
        fstar[o] = bf >= 0 ? first + bf : -1;
        w[o] = df * chat;
        sq = df * df;
    }
    sq = block_sum(sq, red);
    if (threadIdx.x == 0) partial[(int64_t)b * g.nblk + blockIdx.x] = sq;
}

// pass 1 of the column form: p = the de-normalised columns of x
__global__ __launch_bounds__(256) void guide_nearest_kernel(const GuideDev g, const float* __restrict__ x, const uint8_t* __restrict__ fmask,
                                                            int* __restrict__ fstar, float* __restrict__ w, float* __restrict__ partial) {
    extern __shared__ float sp[];                   // [K][L][3] positions, then [L] validity
    __shared__ int scols[AFM_GUIDE_MAX_JOINTS];
    const int b = blockIdx.y, L = g.L;
    stage_index(g.cols, scols);
    __syncthreads();
    for (int i = threadIdx.x; i < g.K * L; i += 256) {
        const int k = i / L, f = i - k * L;
        const float* xrow = x + ((int64_t)b * L + f) * g.D;
#pragma unroll
        for (int a = 0; a < 3; ++a) sp[i * 3 + a] = denorm(xrow, g.mean, g.std, scols[k] + a);
    }
    valid_of_mask(g, sp, fmask);
    nearest_of_staged(g, sp, fstar, w, partial);
}

// pass 1 of the h3d form: p = the recovery kernel's pos[b][K][L][3], the very order staged
__global__ __launch_bounds__(256) void guide_nearest_h3d_kernel(const GuideDev g, const float* __restrict__ pos, const uint8_t* __restrict__ fmask,
                                                                int* __restrict__ fstar, float* __restrict__ w, float* __restrict__ partial) {
    extern __shared__ float sp[];                   // [K][L][3] positions, then [L] validity
    const int n = g.K * g.L * 3;
    const float* pb = pos + (int64_t)blockIdx.y * n;
    for (int i = threadIdx.x; i < n; i += 256) sp[i] = pb[i];
    valid_of_mask(g, sp, fmask);
    nearest_of_staged(g, sp, fstar, w, partial);
}

// Pass 2's energy: block 0 of sample blockIdx.y adds the sample's partials in order, energy[b] = sum / (N K)
__device__ __forceinline__ void sample_energy(const GuideDev& g, const float* __restrict__ partial, float* __restrict__ energy) {
#pragma clang fp contract(off)
    const int b = blockIdx.y;
    if (blockIdx.x == 0 && energy && threadIdx.x == 0) {
        float s = 0.f;
        for (int i = 0; i < g.nblk; ++i) s += partial[(int64_t)b * g.nblk + i];
        energy[b] = s / (float)((int64_t)g.N * g.K);
    }
}

// Pass 2's sums for (frame f, sample b, joint k) on one wave: S_a = sum over the points n with f*(b, n, k) == f of
// w * (p_a - q_a) - lane l adds n = l, l + 64, ... in that order, then the fixed butterfly of wave_sum.  Lane a < 3 gets S_a.
__device__ __forceinline__ float frame_sum(const GuideDev& g, const int* __restrict__ fstar, const float* __restrict__ w, int b, int f, int k,
                                           float p0, float p1, float p2) {
#pragma clang fp contract(off)
    const int N = g.N, lane = threadIdx.x & 63;
    const int64_t o = ((int64_t)b * g.K + k) * N;
    float s0 = 0.f, s1 = 0.f, s2 = 0.f;
    for (int n = lane; n < N; n += 64) {
        if (fstar[o + n] != f) continue;
        const float ww = w[o + n];
        const float* qp = g.q + ((int64_t)b * N + n) * 3;
        const float m0 = ww * (p0 - qp[0]), m1 = ww * (p1 - qp[1]), m2 = ww * (p2 - qp[2]);
        s0 = s0 + m0; s1 = s1 + m1; s2 = s2 + m2;
    }
    s0 = wave_sum(s0); s1 = wave_sum(s1); s2 = wave_sum(s2);
    return lane == 0 ? s0 : (lane == 1 ? s1 : s2);
}

// Pass 2 of the column form, one block per (frame blockIdx.x, sample blockIdx.y), wave v the joints k = v, v + 4, ...:
// grad[b, f, cols[k] + a] = ((scale[b] * coef) * std_a) * S_a.  Every other column of the row, and the whole row of a masked frame or of a
// sample with t[b] >= t_start, is written as zero.
__global__ __launch_bounds__(256) void guide_gather_kernel(const GuideDev g, const float* __restrict__ x, const uint8_t* __restrict__ fmask,
                                                           const int64_t* __restrict__ t, const int* __restrict__ fstar,
                                                           const float* __restrict__ w, const float* __restrict__ partial,
                                                           float* __restrict__ grad, float* __restrict__ energy) {
#pragma clang fp contract(off)
    __shared__ int scols[AFM_GUIDE_MAX_JOINTS];
    const int b = blockIdx.y, f = blockIdx.x, K = g.K;
    stage_index(g.cols, scols);
    __syncthreads();
    sample_energy(g, partial, energy);
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
        const float s = frame_sum(g, fstar, w, b, f, k, denorm(xrow, g.mean, g.std, col), denorm(xrow, g.mean, g.std, col + 1),
                                  denorm(xrow, g.mean, g.std, col + 2));
        if (lane < 3) {
            const float kss = ks * g.std[col + lane];
            row[col + lane] = kss * s;
        }
    }
}

// Pass 2 of the h3d form, the column form's blocks, waves and sums: p is the recovery kernel's, and the bare sums go to S[b][f][k][3] for
// the adjoint (a padded frame is nobody's nearest frame, so its sums are zero; scale, t_start and the mask are the adjoint's business).
// S == NULL: the energy alone, one block per sample.
__global__ __launch_bounds__(256) void guide_sums_h3d_kernel(const GuideDev g, const float* __restrict__ pos, const int* __restrict__ fstar,
                                                             const float* __restrict__ w, const float* __restrict__ partial,
                                                             float* __restrict__ S, float* __restrict__ energy) {
    const int b = blockIdx.y, f = blockIdx.x, K = g.K, lane = threadIdx.x & 63;
    sample_energy(g, partial, energy);
    if (!S) return;
    for (int k = threadIdx.x >> 6; k < K; k += 4) {
        const float* pp = pos + (((int64_t)b * K + k) * g.L + f) * 3;
        const float s = frame_sum(g, fstar, w, b, f, k, pp[0], pp[1], pp[2]);
        if (lane < 3) S[(((int64_t)b * g.L + f) * K + k) * 3 + lane] = s;
    }
}

// ---- long motions (afm_long_guide): the batch is G * S windows of L frames, window b = g * S + w holding the long frames a_w = w * hop ..
// a_w + L - 1 (hop = L - ov) clipped to < F; the positions come from the joined long motion [G][F][D], q / c / fstar / w stay per window.
struct LongGeo { int S, ov, F; };

// the frames window blockIdx.y holds, n_w = min(L, F - a_w), as the validity flags of pass 1; -> a_w
__device__ __forceinline__ int valid_of_window(const GuideDev& g, const LongGeo& lg, float* sp) {
    int* sval = reinterpret_cast<int*>(sp + (size_t)g.K * g.L * 3);
    const int first = ((int)blockIdx.y % lg.S) * (g.L - lg.ov);
    const int n = min(g.L, lg.F - first);
    for (int f = threadIdx.x; f < g.L; f += 256) sval[f] = f < n;
    return first;
}

// windowed pass 1 of the column form: p = the de-normalised columns of the window's rows of the long motion
__global__ __launch_bounds__(256) void long_nearest_kernel(const GuideDev g, const LongGeo lg, const float* __restrict__ lng, int* __restrict__ fstar,
                                                           float* __restrict__ w, float* __restrict__ partial) {
    extern __shared__ float sp[];                   // [K][L][3] positions, then [L] validity
    __shared__ int scols[AFM_GUIDE_MAX_JOINTS];
    const int L = g.L, gi = blockIdx.y / lg.S;
    stage_index(g.cols, scols);
    const int first = valid_of_window(g, lg, sp);
    const int n = min(L, lg.F - first);
    __syncthreads();
    for (int i = threadIdx.x; i < g.K * L; i += 256) {
        const int k = i / L, f = i - k * L;
        if (f >= n) continue;
        const float* xrow = lng + ((int64_t)gi * lg.F + first + f) * g.D;
#pragma unroll
        for (int a = 0; a < 3; ++a) sp[i * 3 + a] = denorm(xrow, g.mean, g.std, scols[k] + a);
    }
    nearest_of_staged(g, sp, fstar, w, partial, first);
}

// windowed pass 1 of the h3d form: p = the recovery's pos[g][K][F][3] of the long motion, the window's frames of every joint
__global__ __launch_bounds__(256) void long_nearest_h3d_kernel(const GuideDev g, const LongGeo lg, const float* __restrict__ pos, int* __restrict__ fstar,
                                                               float* __restrict__ w, float* __restrict__ partial) {
    extern __shared__ float sp[];                   // [K][L][3] positions, then [L] validity
    const int L = g.L, gi = blockIdx.y / lg.S;
    const int first = valid_of_window(g, lg, sp);
    const int n3 = min(L, lg.F - first) * 3;
    const float* pb = pos + (int64_t)gi * g.K * lg.F * 3 + (int64_t)first * 3;
    for (int i = threadIdx.x; i < g.K * L * 3; i += 256) {
        const int k = i / (L * 3), r = i - k * (L * 3);
        if (r < n3) sp[i] = pb[(int64_t)k * lg.F * 3 + r];
    }
    nearest_of_staged(g, sp, fstar, w, partial, first);
}

// the one or two windows of a long motion that hold long frame f: *later = min(f / hop, S - 1); the window in front of it holds f too iff
// there is one and f lies in the later window's first ov frames
__device__ __forceinline__ bool windows_of_frame(const LongGeo& lg, int L, int f, int* later) {
    const int hop = L - lg.ov;
    const int w1 = min(f / hop, lg.S - 1);
    *later = w1;
    return w1 > 0 && f - w1 * hop < lg.ov;
}

// the joined sums of (long frame blockIdx.x, long motion blockIdx.y, joint k) on one wave: the frame's window's frame_sum, or - a shared
// frame - S_earlier + S_later, one rounded addition
__device__ __forceinline__ float long_frame_sum(const GuideDev& g, const LongGeo& lg, const int* __restrict__ fstar, const float* __restrict__ w,
                                                int k, float p0, float p1, float p2) {
#pragma clang fp contract(off)
    const int f = blockIdx.x;
    int w1;
    const bool two = windows_of_frame(lg, g.L, f, &w1);
    const int b = (int)blockIdx.y * lg.S + w1;
    const float later = frame_sum(g, fstar, w, b, f, k, p0, p1, p2);
    if (!two) return later;
    const float earlier = frame_sum(g, fstar, w, b - 1, f, k, p0, p1, p2);
    return earlier + later;
}

// the long motion's contact energy: the windows' energies (each its partials in order, / (N K)) added serially in window order
__device__ __forceinline__ void long_energy(const GuideDev& g, const LongGeo& lg, const float* __restrict__ partial, float* __restrict__ energy) {
#pragma clang fp contract(off)
    if (blockIdx.x == 0 && energy && threadIdx.x == 0) {
        float e = 0.f;
        for (int wi = 0; wi < lg.S; ++wi) {
            const int64_t b = (int64_t)blockIdx.y * lg.S + wi;
            float s = 0.f;
            for (int i = 0; i < g.nblk; ++i) s += partial[b * g.nblk + i];
            const float eb = s / (float)((int64_t)g.N * g.K);
            e = e + eb;
        }
        energy[blockIdx.y] = e;
    }
}

// Long pass 2 of the column form, one block per (long frame blockIdx.x, long motion blockIdx.y), wave v the joints k = v, v + 4, ...:
// grad_long[g, f, cols[k] + a] = ((scale[g] * coef) * std_a) * S with S the joined sum; every other column of the row, and the whole row of
// a long motion with t[g] >= t_start, is written as zero.  g.q / fstar / w are the windows', g.scale and t the long motions'.
__global__ __launch_bounds__(256) void long_gather_kernel(const GuideDev g, const LongGeo lg, const float* __restrict__ lng, const int64_t* __restrict__ t,
                                                          const int* __restrict__ fstar, const float* __restrict__ w,
                                                          const float* __restrict__ partial, float* __restrict__ grad, float* __restrict__ energy) {
#pragma clang fp contract(off)
    __shared__ int scols[AFM_GUIDE_MAX_JOINTS];
    const int gi = blockIdx.y, f = blockIdx.x, K = g.K;
    stage_index(g.cols, scols);
    __syncthreads();
    long_energy(g, lg, partial, energy);
    if (!grad) return;
    float* row = grad + ((int64_t)gi * lg.F + f) * g.D;
    const bool guided = !(t && t[gi] >= g.t_start);
    for (int d = threadIdx.x; d < g.D; d += 256) {
        bool named = false;
        for (int k = 0; k < K; ++k) named = named || (d >= scols[k] && d < scols[k] + 3);
        if (!guided || !named) row[d] = 0.f;
    }
    if (!guided) return;
    const float* xrow = lng + ((int64_t)gi * lg.F + f) * g.D;
    const int lane = threadIdx.x & 63;
    const float ks = g.scale[gi] * g.coef;
    for (int k = threadIdx.x >> 6; k < K; k += 4) {
        const int col = scols[k];
        const float s = long_frame_sum(g, lg, fstar, w, k, denorm(xrow, g.mean, g.std, col), denorm(xrow, g.mean, g.std, col + 1),
                                       denorm(xrow, g.mean, g.std, col + 2));
        if (lane < 3) {
            const float kss = ks * g.std[col + lane];
            row[col + lane] = kss * s;
        }
    }
}

// Long pass 2 of the h3d form: the same blocks, waves and joined sums on the recovery's pos[g][K][F][3]; the bare sums go to S[g][f][k][3] for
// the adjoint over the F frames.  S == NULL: the energy alone, one block per long motion.
__global__ __launch_bounds__(256) void long_sums_h3d_kernel(const GuideDev g, const LongGeo lg, const float* __restrict__ pos, const int* __restrict__ fstar,
                                                            const float* __restrict__ w, const float* __restrict__ partial, float* __restrict__ S,
                                                            float* __restrict__ energy) {
    const int gi = blockIdx.y, f = blockIdx.x, K = g.K, lane = threadIdx.x & 63;
    long_energy(g, lg, partial, energy);
    if (!S) return;
    for (int k = threadIdx.x >> 6; k < K; k += 4) {
        const float* pp = pos + (((int64_t)gi * K + k) * lg.F + f) * 3;
        const float s = long_frame_sum(g, lg, fstar, w, k, pp[0], pp[1], pp[2]);
        if (lane < 3) S[(((int64_t)gi * lg.F + f) * K + k) * 3 + lane] = s;
    }
}

// t of long motion g is its first window's: tl[g] = t[g * S]
__global__ __launch_bounds__(256) void long_t_kernel(const int64_t* __restrict__ t, int64_t* __restrict__ tl, int S, int G) {
    const int gi = blockIdx.x * 256 + threadIdx.x;
    if (gi < G) tl[gi] = t[(int64_t)gi * S];
}

// The adjoint of the recovery for sample blockIdx.x: S[b][f][k][3] -> the sample's complete rows in `rows` [B][L][D], the zeros included.
// Per frame (one thread each), G_k = A^T S_k, the local-coordinate and root-height terms written at once, gX_f = sum_k G_x, gZ_f likewise
// and the rotation term of the joints, in joint order; then SX, SZ = inclusive suffix sums of gX, gZ (lane 0 and lane 64, f = L-1 down
// to 0); per frame the velocity terms and T_f; then dw = the exclusive suffix sum of T (lane 0, f = L-1 down to 0).  c_f, s_f are read back
// from what the recovery stored.  A padded frame's row, and every row of a sample with t[b] >= t_start (the return below, uniform over
// the block), stays zero.  No atomics.
__device__ __forceinline__ void h3d_adjoint_rows(const H3dAdjDev& a, const float* __restrict__ x, const uint8_t* __restrict__ fmask,
                                                 const int64_t* __restrict__ t, const float* __restrict__ cs, const float* __restrict__ S,
                                                 float* __restrict__ rows) {
#pragma clang fp contract(off)
    extern __shared__ float sh[];                   // [H3D_SCAN_ROWS][L]
    __shared__ int sj[AFM_GUIDE_MAX_JOINTS];
    __shared__ float sA[12];
    const int b = blockIdx.x, L = a.L, D = a.D, K = a.K;
    float *sgX = sh, *sgZ = sh + L, *sT = sh + 2 * L, *sc = sh + 3 * L, *ss = sh + 4 * L, *svx = sh + 5 * L, *svz = sh + 6 * L;
    float* gb = rows + (int64_t)b * L * D;
    for (int64_t i = threadIdx.x; i < (int64_t)L * D; i += 256) gb[i] = 0.f;
    if (t && t[b] >= a.t_start) return;
    stage_index(a.joints, sj);
    stage_to_scene(a.to_scene, (int64_t)b * a.ts_stride, sA);
    __syncthreads();                                // (the zeros above are in place before any thread writes a term over them)
    const float* xb = x + (int64_t)b * L * D;
    const uint8_t* mb = fmask ? fmask + (int64_t)b * L : nullptr;
    const float ks = a.scale[b] * a.coef;
    for (int f = threadIdx.x; f < L; f += 256) {
        const float* xrow = xb + (int64_t)f * D;
        float* row = gb + (int64_t)f * D;
        const bool pad = mb && mb[f];
        const float c = cs[((int64_t)b * L + f) * 2], s = cs[((int64_t)b * L + f) * 2 + 1];
        sc[f] = c; ss[f] = s;
        svx[f] = pad ? 0.f : denorm(xrow, a.mean, a.std, 1);
        svz[f] = pad ? 0.f : denorm(xrow, a.mean, a.std, 2);
        float gX = 0.f, gZ = 0.f, T = 0.f;
        for (int k = 0; k < K; ++k) {
            const float* Sp = S + (((int64_t)b * L + f) * K + k) * 3;
            const float S0 = Sp[0], S1 = Sp[1], S2 = Sp[2];
            const float Gx = (sA[0] * S0 + sA[4] * S1) + sA[8] * S2;
            const float Gy = (sA[1] * S0 + sA[5] * S1) + sA[9] * S2;
            const float Gz = (sA[2] * S0 + sA[6] * S1) + sA[10] * S2;
            gX = gX + Gx; gZ = gZ + Gz;
            const int j = sj[k];
            if (j == 0) {
                if (!pad) row[3] = (ks * a.std[3]) * Gy;
                continue;
            }
            const int col = 4 + 3 * (j - 1);
            const float lx = denorm(xrow, a.mean, a.std, col), lz = denorm(xrow, a.mean, a.std, col + 2);
            T = T + (Gx * (-lx * s - lz * c) + Gz * (lx * c - lz * s));
            if (!pad) {
                row[col] = (ks * a.std[col]) * (Gx * c + Gz * s);
                row[col + 1] = (ks * a.std[col + 1]) * Gy;
                row[col + 2] = (ks * a.std[col + 2]) * (Gz * c - Gx * s);
            }
        }
        sgX[f] = gX; sgZ[f] = gZ; sT[f] = T;
    }
    __syncthreads();
    if (threadIdx.x == 0 || threadIdx.x == 64) {
        float* v = threadIdx.x == 0 ? sgX : sgZ;
        float acc = 0.f;
        for (int f = L - 1; f >= 0; --f) { acc = acc + v[f]; v[f] = acc; }
    }
    __syncthreads();
    for (int f = threadIdx.x; f < L; f += 256) {
        if (f == 0) { sT[0] = 2.f * sT[0]; continue; }            // (never read: dw_g sums the frames behind g)
        const float SX = sgX[f], SZ = sgZ[f], c = sc[f], s = ss[f], vx = svx[f - 1], vz = svz[f - 1];
        sT[f] = 2.f * ((sT[f] + SX * (-vx * s - vz * c)) + SZ * (vx * c - vz * s));
        if (!(mb && mb[f - 1])) {
            float* row = gb + (int64_t)(f - 1) * D;
            row[1] = (ks * a.std[1]) * (SX * c + SZ * s);
            row[2] = (ks * a.std[2]) * (SZ * c - SX * s);
        }
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        float acc = 0.f;
        for (int f = L - 1; f >= 0; --f) { const float v = sT[f]; sT[f] = acc; acc = acc + v; }
    }
    __syncthreads();
    for (int f = threadIdx.x; f < L; f += 256)
        if (!(mb && mb[f])) gb[(int64_t)f * D] = (ks * a.std[0]) * sT[f];
}

// the adjoint, one block per sample: the rows are the gradient
__global__ __launch_bounds__(256) void h3d_adjoint_kernel(const H3dAdjDev a, const float* __restrict__ x, const uint8_t* __restrict__ fmask,
                                                          const int64_t* __restrict__ t, const float* __restrict__ cs, const float* __restrict__ S,
                                                          float* __restrict__ grad) {
    h3d_adjoint_rows(a, x, fmask, t, cs, S, grad);
}

// The adjoint ADDED to the rows the contact term wrote, one launch: the sample's rows go to tmp[b][L][D], then grad = grad + tmp, one
// rounded addition per element - the zeros of a padded frame, of the other columns and of a sample with t[b] >= t_start included.
__global__ __launch_bounds__(256) void h3d_adjoint_add_kernel(const H3dAdjDev a, const float* __restrict__ x, const uint8_t* __restrict__ fmask,
                                                              const int64_t* __restrict__ t, const float* __restrict__ cs, const float* __restrict__ S,
                                                              float* __restrict__ tmp, float* __restrict__ grad) {
#pragma clang fp contract(off)
    h3d_adjoint_rows(a, x, fmask, t, cs, S, tmp);
    __syncthreads();                                // (the block's own global writes to tmp are visible to it behind the barrier)
    const int64_t n = (int64_t)a.L * a.D, o = blockIdx.x * n;
    for (int64_t i = threadIdx.x; i < n; i += 256) grad[o + i] = grad[o + i] + tmp[o + i];
}

// ---- joint-position targets (afm_joint_targets): E = sum over valid (f, k) of w * |p - g|^2 on the positions p the kernels above compute.
struct TargetDev {
    const float *target, *weight, *mean, *std, *scale;
    int cols[AFM_GUIDE_MAX_JOINTS];
    int K, L, D;
    int64_t t_start;
};

// one item's energy term w * ((dx*dx + dy*dy) + dz*dz), d = p - g
__device__ __forceinline__ float target_term(float w, float p0, float p1, float p2, const float* __restrict__ gp) {
#pragma clang fp contract(off)
    const float dx = p0 - gp[0], dy = p1 - gp[1], dz = p2 - gp[2];
    const float xx = dx * dx, yy = dy * dy, zz = dz * dz;
    return w * ((xx + yy) + zz);
}

// The column form, one block per (frame blockIdx.x, sample blockIdx.y): thread i < 3 K the coordinate a = i % 3 of joint k = i / 3,
// d = g_a - p_a, m = w * d, term = ((scale[b] * 2) * std_a) * m; every other column of the row, a joint with w == 0 (its target is not
// read), a padded frame and a sample with t[b] >= t_start give the term 0.  ACC: row[d] = row[d] + term for EVERY column of the row (one
// rounded addition per element on what the contact term wrote), else row[d] = term.  Block 0 of a sample adds its energy: thread i the
// items e = f * K + k = i, i + 256, ... in that order, then block_sum.
template <bool ACC>
__global__ __launch_bounds__(256) void target_cols_kernel(const TargetDev g, const float* __restrict__ x, const uint8_t* __restrict__ fmask,
                                                          const int64_t* __restrict__ t, float* __restrict__ grad, float* __restrict__ energy) {
#pragma clang fp contract(off)
    __shared__ int scols[AFM_GUIDE_MAX_JOINTS];
    __shared__ float red[4];
    const int b = blockIdx.y, f = blockIdx.x, K = g.K, L = g.L, D = g.D;
    stage_index(g.cols, scols);
    __syncthreads();
    if (f == 0 && energy) {
        float acc = 0.f;
        for (int e = threadIdx.x; e < L * K; e += 256) {
            const int ff = e / K, k = e - ff * K;
            if (fmask && fmask[(int64_t)b * L + ff]) continue;
            const int64_t o = ((int64_t)b * L + ff) * K + k;
            const float w = g.weight[o];
            if (w == 0.f) continue;
            const float* xrow = x + ((int64_t)b * L + ff) * D;
            const int col = scols[k];
            const float p0 = denorm(xrow, g.mean, g.std, col), p1 = denorm(xrow, g.mean, g.std, col + 1), p2 = denorm(xrow, g.mean, g.std, col + 2);
            acc = acc + target_term(w, p0, p1, p2, g.target + o * 3);
        }
        acc = block_sum(acc, red);
        if (threadIdx.x == 0) energy[b] = acc;
    }
    if (!grad) return;
    float* row = grad + ((int64_t)b * L + f) * D;
    const float* xrow = x + ((int64_t)b * L + f) * D;
    const bool guided = !(fmask && fmask[(int64_t)b * L + f]) && !(t && t[b] >= g.t_start);
    const float ks = g.scale[b] * 2.f;
    for (int d = threadIdx.x; d < D; d += 256) {
        float term = 0.f;
        if (guided)
            for (int k = 0; k < K; ++k) {
                const int a = d - scols[k];
                if (a < 0 || a >= 3) continue;
                const int64_t o = ((int64_t)b * L + f) * K + k;
                const float w = g.weight[o];
                if (w == 0.f) break;
                const float dd = g.target[o * 3 + a] - denorm(xrow, g.mean, g.std, d);
                const float m = w * dd;
                term = (ks * g.std[d]) * m;
                break;
            }
        row[d] = ACC ? row[d] + term : term;
    }
}

// The h3d form, one block per sample: the recovery's positions pos[b][f][k][3] (the targets' own order) -> S[b][f][k][3] = w * (g - p),
// zero where w == 0 (the target is not read) or the frame is padded, for the adjoint; scale, t_start and the rows are the adjoint's
// business.  The energy as in the column form: thread i the items e = i, i + 256, ... in that order, then block_sum.
__global__ __launch_bounds__(256) void target_h3d_kernel(const TargetDev g, const float* __restrict__ pos, const uint8_t* __restrict__ fmask,
                                                         float* __restrict__ S, float* __restrict__ energy) {
#pragma clang fp contract(off)
    __shared__ float red[4];
    const int b = blockIdx.x, K = g.K, L = g.L;
    float acc = 0.f;
    for (int e = threadIdx.x; e < L * K; e += 256) {
        const int f = e / K;
        const int64_t o = (int64_t)b * L * K + e;
        float s0 = 0.f, s1 = 0.f, s2 = 0.f;
        const float w = (fmask && fmask[(int64_t)b * L + f]) ? 0.f : g.weight[o];
        if (w != 0.f) {
            const float* pp = pos + o * 3;
            const float* gp = g.target + o * 3;
            const float p0 = pp[0], p1 = pp[1], p2 = pp[2];
            s0 = w * (gp[0] - p0); s1 = w * (gp[1] - p1); s2 = w * (gp[2] - p2);
            acc = acc + target_term(w, p0, p1, p2, gp);
        }
        if (S) { S[o * 3] = s0; S[o * 3 + 1] = s1; S[o * 3 + 2] = s2; }
    }
    if (!energy) return;
    acc = block_sum(acc, red);
    if (threadIdx.x == 0) energy[b] = acc;
}

int64_t guide_nblk(int N, int K) { return ((int64_t)N * K + 255) / 256; }

// the h3d form's buffers behind the three of the absolute form: positions [B][K][L][3], c / s [B][L][2], S [B][L][K][3]
int64_t h3d_extra_bytes(int64_t B, int64_t L, int64_t K) {
    return 2 * afm_loop::align256(B * K * L * 3 * 4) + afm_loop::align256(B * L * 2 * 4);
}

bool h3d_joint_list_ok(const int32_t* joints, int n) {
    for (int k = 0; k < n; ++k) {
        if (joints[k] < 0 || joints[k] >= H3D_JOINTS) return false;
        for (int j = 0; j < k; ++j)
            if (joints[j] == joints[k]) return false;
    }
    return true;
}

// the K joints of a description, either term's: h3d joints 0..21, none twice, in a motion that holds the feature columns, placed by one
// matrix or one per sample; else column triples inside D that do not overlap
int joints_check(const int32_t* cols, const afm_h3d_layout* h3d, int K, int D) {
    if (h3d) {
        if (D < H3D_COLS || !h3d_joint_list_ok(h3d->joints, K)) return AFM_E_BADARG;
        if (h3d->to_scene_stride != 0 && h3d->to_scene_stride != 12) return AFM_E_BADARG;
        return 0;
    }
    for (int k = 0; k < K; ++k) {
        if (cols[k] < 0 || cols[k] + 3 > D) return AFM_E_BADARG;
        for (int j = 0; j < k; ++j)
            if (cols[k] < cols[j] + 3 && cols[j] < cols[k] + 3) return AFM_E_BADARG;          // overlapping triples
    }
    return 0;
}

// What an h3d term launches around its own kernels: the recovery's and the adjoint's descriptions of the samples [start, start + count)
// and their buffers, carved from wp - positions and S, [count][K][L][3] (k_major: the order pass 1 stages) or [count][L][K][3] (the
// targets' own), then c / s [count][L][2]; `end` is the byte behind them.  `scale` already points at sample `start`.
struct H3dPlan {
    H3dDev rec;
    H3dAdjDev adj;
    float *pos, *S, *cs;
    char* end;
    size_t scan_lds;
};

H3dPlan h3d_plan(const float* mean, const float* std, const float* scale, const afm_h3d_layout& lay, int K, int L, int D, int start, int count,
                 bool k_major, float coef, int64_t t_start, char* wp) {
    H3dPlan p = {};
    const int64_t klb = afm_loop::align256((int64_t)count * K * L * 3 * 4);
    p.pos = (float*)wp; wp += klb;
    p.S = (float*)wp; wp += klb;
    p.cs = (float*)wp; p.end = wp + afm_loop::align256((int64_t)count * L * 2 * 4);
    p.scan_lds = (size_t)H3D_SCAN_ROWS * L * 4;
    p.rec.mean = p.adj.mean = mean; p.rec.std = p.adj.std = std;
    p.rec.to_scene = p.adj.to_scene = lay.to_scene ? lay.to_scene + (int64_t)start * lay.to_scene_stride : nullptr;
    p.rec.ts_stride = p.adj.ts_stride = lay.to_scene_stride;
    for (int k = 0; k < K; ++k) p.rec.joints[k] = p.adj.joints[k] = lay.joints[k];
    p.rec.J = p.adj.K = K; p.rec.L = p.adj.L = L; p.rec.D = p.adj.D = D;
    p.rec.out_b = (int64_t)K * L * 3; p.rec.out_j = k_major ? (int64_t)L * 3 : 3; p.rec.out_f = k_major ? 3 : (int64_t)K * 3;
    p.adj.scale = scale; p.adj.coef = coef; p.adj.t_start = t_start;
    return p;
}

}  // namespace

extern "C" int64_t afm_contact_guidance_workspace_bytes(int32_t B, int32_t N, int32_t K) {
    if (B < 0 || N <= 0 || K <= 0 || K > AFM_GUIDE_MAX_JOINTS) return AFM_E_BADARG;
    const int64_t nk = (int64_t)B * N * K;
    return 2 * afm_loop::align256(nk * 4) + afm_loop::align256((int64_t)B * guide_nblk(N, K) * 4);
}

extern "C" int64_t afm_contact_guidance_h3d_workspace_bytes(int32_t B, int32_t L, int32_t N, int32_t K) {
    const int64_t base = afm_contact_guidance_workspace_bytes(B, N, K);
    if (base < 0 || L <= 0) return AFM_E_BADARG;
    return afm_loop::align256(base) + h3d_extra_bytes(B, L, K);
}

// the workspace of `count` samples of a description, either form
__attribute__((visibility("hidden"))) int64_t afm_contact_guide_workspace_bytes(const afm_contact_guide* a, int32_t count, int32_t L) {
    return a->h3d ? afm_contact_guidance_h3d_workspace_bytes(count, L, a->N, a->K) : afm_contact_guidance_workspace_bytes(count, a->N, a->K);
}

// what a description must satisfy before anything is enqueued (L, D: the motion's)
__attribute__((visibility("hidden"))) int afm_contact_guide_check(const afm_contact_guide* a, int32_t L, int32_t D) {
    if (!a || !a->q || !a->c || !a->mean || !a->std || !a->scale || L <= 0 || D <= 0) return AFM_E_BADARG;
    if (a->K <= 0 || a->K > AFM_GUIDE_MAX_JOINTS || a->N <= 0 || !(a->sigma > 0.0) || (int64_t)a->N * a->K > (int64_t)1 << 30) return AFM_E_BADARG;
    if (joints_check(a->cols, a->h3d, a->K, D) != 0) return AFM_E_BADARG;
    if (((size_t)a->K * L * 3 + L) * 4 > (size_t)GUIDE_LDS_BYTES || L > 65535) return AFM_E_UNSUPPORTED;
    if (a->h3d && (size_t)H3D_SCAN_ROWS * L * 4 > (size_t)GUIDE_LDS_BYTES) return AFM_E_UNSUPPORTED;
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
    const int64_t need = afm_contact_guide_workspace_bytes(a, count, L);
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
    if (a->h3d) {
        wp = (char*)workspace + afm_loop::align256(afm_contact_guidance_workspace_bytes(count, a->N, a->K));
        const H3dPlan p = h3d_plan(a->mean, a->std, g.scale, *a->h3d, a->K, L, D, start, count, true, g.coef, a->t_start, wp);
        hipLaunchKernelGGL(h3d_recover_kernel, dim3((unsigned)count), dim3(256), p.scan_lds, s, p.rec, x, frame_mask, p.pos, grad ? p.cs : nullptr);
        AFM_CHECK_LAUNCH();
        hipLaunchKernelGGL(guide_nearest_h3d_kernel, dim3((unsigned)g.nblk, (unsigned)count), dim3(256), lds, s, g, p.pos, frame_mask, fstar, w, partial);
        AFM_CHECK_LAUNCH();
        hipLaunchKernelGGL(guide_sums_h3d_kernel, dim3(grad ? (unsigned)L : 1u, (unsigned)count), dim3(256), 0, s, g, p.pos, fstar, w, partial,
                           grad ? p.S : nullptr, energy);
        AFM_CHECK_LAUNCH();
        if (!grad) return 0;
        hipLaunchKernelGGL(h3d_adjoint_kernel, dim3((unsigned)count), dim3(256), p.scan_lds, s, p.adj, x, frame_mask, t, p.cs, p.S, grad);
        AFM_CHECK_LAUNCH();
        return 0;
    }
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

// ---- joint targets and the sum of the two guidances (afm_motion_guide)
namespace {

int64_t targets_workspace_bytes(const afm_joint_targets* a, bool add, int64_t count, int64_t L, int64_t D) {
    if (!a->h3d) return 0;
    // positions [count][L][K][3], S likewise, c / s [count][L][2]; added to a contact term: the adjoint's own rows [count][L][D]
    return h3d_extra_bytes(count, L, a->K) + (add ? afm_loop::align256(count * L * D * 4) : 0);
}

int targets_check(const afm_joint_targets* a, int32_t L, int32_t D) {
    if (!a->target || !a->weight || !a->mean || !a->std || !a->scale || L <= 0 || D <= 0) return AFM_E_BADARG;
    if (a->K <= 0 || a->K > AFM_GUIDE_MAX_JOINTS) return AFM_E_BADARG;
    if (joints_check(a->cols, a->h3d, a->K, D) != 0) return AFM_E_BADARG;
    if (a->h3d && (size_t)H3D_SCAN_ROWS * L * 4 > (size_t)GUIDE_LDS_BYTES) return AFM_E_UNSUPPORTED;
    if (L > 65535 || (int64_t)L * a->K > (int64_t)1 << 30) return AFM_E_UNSUPPORTED;
    return 0;
}

// the targets' launches on the samples [start, start + count); add: grad holds the contact term's result, the sum goes there
int targets_sub(const afm_joint_targets* a, bool add, int32_t start, const float* x, const uint8_t* frame_mask, const int64_t* t, float* grad,
                float* energy, int32_t count, int32_t L, int32_t D, char* wp, hipStream_t s) {
    TargetDev g = {};
    g.target = a->target + (int64_t)start * L * a->K * 3; g.weight = a->weight + (int64_t)start * L * a->K;
    g.mean = a->mean; g.std = a->std; g.scale = a->scale + start;
    for (int k = 0; k < a->K; ++k) g.cols[k] = a->h3d ? 0 : a->cols[k];
    g.K = a->K; g.L = L; g.D = D; g.t_start = a->t_start;
    if (!a->h3d) {
        const dim3 grid(grad ? (unsigned)L : 1u, (unsigned)count);
        if (add) hipLaunchKernelGGL(target_cols_kernel<true>, grid, dim3(256), 0, s, g, x, frame_mask, t, grad, energy);
        else hipLaunchKernelGGL(target_cols_kernel<false>, grid, dim3(256), 0, s, g, x, frame_mask, t, grad, energy);
        AFM_CHECK_LAUNCH();
        return 0;
    }
    const H3dPlan p = h3d_plan(a->mean, a->std, g.scale, *a->h3d, a->K, L, D, start, count, false, 2.f, a->t_start, wp);
    float* tmp = (float*)p.end;                     // (add: the adjoint's own rows [count][L][D])
    hipLaunchKernelGGL(h3d_recover_kernel, dim3((unsigned)count), dim3(256), p.scan_lds, s, p.rec, x, frame_mask, p.pos, grad ? p.cs : nullptr);
    AFM_CHECK_LAUNCH();
    hipLaunchKernelGGL(target_h3d_kernel, dim3((unsigned)count), dim3(256), 0, s, g, p.pos, frame_mask, grad ? p.S : nullptr, energy);
    AFM_CHECK_LAUNCH();
    if (!grad) return 0;
    if (add) hipLaunchKernelGGL(h3d_adjoint_add_kernel, dim3((unsigned)count), dim3(256), p.scan_lds, s, p.adj, x, frame_mask, t, p.cs, p.S, tmp, grad);
    else hipLaunchKernelGGL(h3d_adjoint_kernel, dim3((unsigned)count), dim3(256), p.scan_lds, s, p.adj, x, frame_mask, t, p.cs, p.S, grad);
    AFM_CHECK_LAUNCH();
    return 0;
}

}  // namespace

// what a sum must satisfy before anything is enqueued (L, D: the motion's)
__attribute__((visibility("hidden"))) int afm_motion_guide_check(const afm_motion_guide* g, int32_t L, int32_t D) {
    if (!g || (!g->contact && !g->targets)) return AFM_E_BADARG;
    if (g->contact) {
        const int rc = afm_contact_guide_check(g->contact, L, D);
        if (rc != 0) return rc;
    }
    if (g->targets) {
        const int rc = targets_check(g->targets, L, D);
        if (rc != 0) return rc;
    }
    if (g->contact && g->targets) {
        const afm_contact_guide* c = g->contact;
        const afm_joint_targets* a = g->targets;
        if (c->mean != a->mean || c->std != a->std || !c->h3d != !a->h3d) return AFM_E_BADARG;
        if (c->h3d && (c->h3d->to_scene != a->h3d->to_scene || c->h3d->to_scene_stride != a->h3d->to_scene_stride)) return AFM_E_BADARG;
    }
    return 0;
}

// the workspace of `count` samples of a checked sum: the contact term's, then the targets'
__attribute__((visibility("hidden"))) int64_t afm_motion_guide_workspace_bytes(const afm_motion_guide* g, int32_t count, int32_t L, int32_t D) {
    int64_t n = g->contact ? afm_loop::align256(afm_contact_guide_workspace_bytes(g->contact, count, L)) : 0;
    if (g->targets) n += targets_workspace_bytes(g->targets, g->contact != nullptr, count, L, D);
    return n;
}

// the samples [start, start + count) of the sum's batch; x, frame_mask, t, grad and the energies already point at sample `start`.
// run_contact / run_targets: the terms this call computes (a loop step in front of a term's first_guided leaves it out)
__attribute__((visibility("hidden"))) int afm_motion_guidance_sub(const afm_motion_guide* g, bool run_contact, bool run_targets, int32_t start, const float* x,
                                                                  const uint8_t* frame_mask, const int64_t* t, float* grad, float* energy_contact,
                                                                  float* energy_targets, int32_t count, int32_t L, int32_t D, void* workspace,
                                                                  int64_t workspace_bytes, void* stream) {
    const int rc = afm_motion_guide_check(g, L, D);
    if (rc != 0) return rc;
    run_contact = run_contact && g->contact;
    run_targets = run_targets && g->targets;
    if (!x || (!grad && !energy_contact && !energy_targets) || start < 0 || count < 0 || (energy_contact && !run_contact) ||
        (energy_targets && !run_targets) || (!run_contact && !run_targets)) return AFM_E_BADARG;
    if (count > 65535) return AFM_E_UNSUPPORTED;
    if (count == 0) return 0;
    if (!workspace || workspace_bytes < afm_motion_guide_workspace_bytes(g, count, L, D)) return AFM_E_WORKSPACE;
    const int64_t cbytes = g->contact ? afm_loop::align256(afm_contact_guide_workspace_bytes(g->contact, count, L)) : 0;
    if (run_contact && (grad || energy_contact))
    {
        const int rcc = afm_contact_guidance_sub(g->contact, start, x, frame_mask, t, grad, energy_contact, count, L, D, workspace, cbytes, stream);
        if (rcc != 0) return rcc;
    }
    if (run_targets && (grad || energy_targets))
        return targets_sub(g->targets, run_contact && grad, start, x, frame_mask, t, grad, energy_targets, count, L, D, (char*)workspace + cbytes,
                           (hipStream_t)stream);
    return 0;
}

extern "C" int64_t afm_motion_guidance_workspace_bytes(const afm_motion_guide* g, int32_t B, int32_t L, int32_t D) {
    if (B < 0 || afm_motion_guide_check(g, L, D) != 0) return AFM_E_BADARG;
    return afm_motion_guide_workspace_bytes(g, B, L, D) + 256;          // (never zero: the column-form targets alone need none)
}

extern "C" int afm_motion_guidance(const afm_motion_guide* g, const float* x, const uint8_t* frame_mask, const int64_t* t, float* grad,
                                   float* energy_contact, float* energy_targets, int32_t B, int32_t L, int32_t D, void* workspace,
                                   int64_t workspace_bytes, void* stream) {
    return afm_motion_guidance_sub(g, true, true, 0, x, frame_mask, t, grad, energy_contact, energy_targets, B, L, D, workspace, workspace_bytes, stream);
}

extern "C" int afm_h3d_joints(const float* x, const float* mean, const float* std, const uint8_t* frame_mask, const int32_t* joints, int32_t J,
                              const float* to_scene, int32_t to_scene_stride, float* out, int32_t B, int32_t L, int32_t D, void* stream) {
    if (!x || !mean || !std || !out || B < 0 || L <= 0 || D < H3D_COLS) return AFM_E_BADARG;
    if (to_scene_stride != 0 && to_scene_stride != 12) return AFM_E_BADARG;
    if (!joints) J = H3D_JOINTS;
    if (J <= 0 || J > H3D_JOINTS || (joints && !h3d_joint_list_ok(joints, J))) return AFM_E_BADARG;
    if ((size_t)H3D_SCAN_ROWS * L * 4 > (size_t)GUIDE_LDS_BYTES || B > 65535) return AFM_E_UNSUPPORTED;
    if (B == 0) return 0;
    H3dDev h = {};
    h.mean = mean; h.std = std; h.to_scene = to_scene; h.ts_stride = to_scene_stride;
    for (int k = 0; k < J; ++k) h.joints[k] = joints ? joints[k] : k;
    h.J = J; h.L = L; h.D = D;
    h.out_b = (int64_t)L * J * 3; h.out_j = 3; h.out_f = (int64_t)J * 3;
    hipLaunchKernelGGL(h3d_recover_kernel, dim3((unsigned)B), dim3(256), (size_t)H3D_SCAN_ROWS * L * 4, (hipStream_t)stream, h, x, frame_mask, out,
                       (float*)nullptr);
    AFM_CHECK_LAUNCH();
    return 0;
}

// ---- scene clearance (afm_scene_clearance): every joint-frame against every obstacle point of its sample, n-body style.  A block owns
// whole frames - at most 64 joint-frames, one per lane - and all of its CLEAR_WAVES waves hold the same joint-frames in registers; the
// sample's points pass through LDS in tiles of {x, y, z, w} (w decided once by the staging threads), each wave takes its own fixed span
// of every tile - all lanes read the same entry, an LDS broadcast - and the waves' partial sums are joined through LDS in wave order.
namespace {

constexpr int CLEAR_WAVES = AFM_CLEAR_WAVES, CLEAR_THREADS = 64 * CLEAR_WAVES, CLEAR_TILE = AFM_CLEAR_TILE, CLEAR_SPAN = CLEAR_TILE / CLEAR_WAVES;

struct ClearDev {
    const float *q, *weight, *c, *mean, *std, *scale;          // c: NULL without the exemption
    int cols[AFM_GUIDE_MAX_JOINTS];
    float ir2[AFM_GUIDE_MAX_JOINTS], coef[AFM_GUIDE_MAX_JOINTS];          // 1 / r^2 and 4 / r^2, rounded once from float64
    int K, N, Kc, L, D, up, fpb;                                // fpb: frames per block, 64 / K
    float min_height, c_min;                                    // the smallest float32 >= the threshold (-inf / +inf: not set)
    int64_t t_start;
};

// the per-joint rows of a by-value kernel argument into LDS with static indices (a dynamic index would put the arrays in scratch)
__device__ __forceinline__ void stage_clear_rows(const ClearDev& g, int* scols, float* sir2, float* scoef) {
#pragma unroll
    for (int k = 0; k < AFM_GUIDE_MAX_JOINTS; ++k)
        if (threadIdx.x == k) { scols[k] = g.cols[k]; sir2[k] = g.ir2[k]; scoef[k] = g.coef[k]; }
}

struct ClearShared {
    float4 pt[CLEAR_TILE];                  // the tile: x, y, z, w
    float join[CLEAR_WAVES][4][64];         // a wave's partial S_x, S_y, S_z, e of lane i
    float term[64][3];                      // the column form's finished terms of joint-frame i
    int cols[AFM_GUIDE_MAX_JOINTS];
    float ir2[AFM_GUIDE_MAX_JOINTS], coef[AFM_GUIDE_MAX_JOINTS];
};

// The sums of block `blk` of sample blockIdx.y, on every wave alike: lane i holds joint-frame (f, k) = (blk * fpb + i / K, i % K);
// *live: the lane has one; *valid: and its frame is not padded.  -> S (s[0..2]) and e (s[3]), zero where not valid.  Wave v adds, from 0
// and in ascending n, the points with (n mod CLEAR_TILE) / CLEAR_SPAN == v; the join is the serial sum over v = 0 .. CLEAR_WAVES - 1.
// `pos`: the recovery's positions [b][f][k][3] (h3d), else the de-normalised columns of x.  The first barrier of the tile loop also
// separates this call's writes to sh.join from the previous call's reads (N > 0: the loop runs).  `row0`: the row of x / pos that holds the
// sample's frame 0 (b * L; a window of a long motion: its first long frame's row of the joined motion), `nfr`: the frames that exist (L; a
// window: those in front of the long motion's end).
__device__ __forceinline__ void clear_block_sums(const ClearDev& g, ClearShared& sh, const float* __restrict__ x, const float* __restrict__ pos,
                                                 const uint8_t* __restrict__ fmask, int blk, int64_t row0, int nfr, float s[4], int* fo, int* ko,
                                                 bool* live, bool* valid) {
#pragma clang fp contract(off)
    const int b = blockIdx.y, K = g.K, L = g.L, N = g.N;
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int fr = lane / K, k = lane - fr * K, f = blk * g.fpb + fr;
    *fo = f; *ko = k;
    *live = fr < g.fpb && f < L;
    *valid = *live && f < nfr && !(fmask && fmask[(int64_t)b * L + f]);
    float p0 = 0.f, p1 = 0.f, p2 = 0.f, ir2 = 0.f;
    if (*valid) {
        if (pos) {
            const float* pp = pos + ((row0 + f) * K + k) * 3;
            p0 = pp[0]; p1 = pp[1]; p2 = pp[2];
        } else {
            const float* xrow = x + (row0 + f) * g.D;
            const int col = sh.cols[k];
            p0 = denorm(xrow, g.mean, g.std, col); p1 = denorm(xrow, g.mean, g.std, col + 1); p2 = denorm(xrow, g.mean, g.std, col + 2);
        }
        ir2 = sh.ir2[k];
    }
    float s0 = 0.f, s1 = 0.f, s2 = 0.f, e = 0.f;
    for (int t0 = 0; t0 < N; t0 += CLEAR_TILE) {
        __syncthreads();
        for (int j = threadIdx.x; j < CLEAR_TILE; j += CLEAR_THREADS) {
            const int n = t0 + j;
            float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
            if (n < N) {
                const int64_t o = (int64_t)b * N + n;
                const float* qp = g.q + o * 3;
                v.x = qp[0]; v.y = qp[1]; v.z = qp[2];
                float w = g.weight ? g.weight[o] : 1.f;
                const float h = g.up == 0 ? v.x : (g.up == 1 ? v.y : v.z);
                if (h < g.min_height) w = 0.f;
                if (g.c) {
                    const float* cp = g.c + o * g.Kc;
                    float mx = cp[0];
                    for (int j2 = 1; j2 < g.Kc; ++j2) mx = fmaxf(mx, cp[j2]);
                    if (mx >= g.c_min) w = 0.f;
                }
                v.w = w;
            }
            sh.pt[j] = v;
        }
        __syncthreads();
        const int cnt = min(CLEAR_SPAN, N - t0 - wave * CLEAR_SPAN);
        const float4* my = sh.pt + wave * CLEAR_SPAN;
        float4 next = my[0];
        for (int j = 0; j < cnt; ++j) {
            const float4 v = next;
            next = my[min(j + 1, CLEAR_SPAN - 1)];              // (the entry behind this one is on its way while this one is used)
            const float dx = p0 - v.x, dy = p1 - v.y, dz = p2 - v.z;
            const float xx = dx * dx, yy = dy * dy, zz = dz * dz;
            const float d2 = (xx + yy) + zz;
            const float m = d2 * ir2;
            const float u = fmaxf(0.f, 1.f - m);
            const float wu = v.w * u;
            if (wu != 0.f) {
                const float m0 = wu * dx, m1 = wu * dy, m2 = wu * dz, me = wu * u;
                s0 = s0 + m0; s1 = s1 + m1; s2 = s2 + m2; e = e + me;
            }
        }
    }
    sh.join[wave][0][lane] = s0; sh.join[wave][1][lane] = s1; sh.join[wave][2][lane] = s2; sh.join[wave][3][lane] = e;
    __syncthreads();
#pragma unroll
    for (int a = 0; a < 4; ++a) {
        float acc = sh.join[0][a][lane];
#pragma unroll
        for (int v = 1; v < CLEAR_WAVES; ++v) acc = acc + sh.join[v][a][lane];
        s[a] = *valid ? acc : 0.f;
    }
}

// One launch, blocks (frame block blockIdx.x, sample blockIdx.y).  out != NULL, column form (pos == NULL): the block's complete grad rows -
// grad[b,f,cols[k]+a] = ((scale[b] * coef_k) * std_a) * S_a, zero in every other column, in a padded frame and in a sample with
// t[b] >= t_start; acc: row[d] = row[d] + term for EVERY column (one rounded addition per element on what the terms in front wrote).
// h3d form (pos set): coef_k * S_a (zero in a padded frame) to out = S[b][f][k][3] for the adjoint, whose business scale, t_start and
// the rows are.  energy != NULL: the sample's block 0 walks every frame block in order, lane i adding its e, then one wave's butterfly.
__global__ __launch_bounds__(CLEAR_THREADS) void clear_kernel(const ClearDev g, const float* __restrict__ x, const float* __restrict__ pos,
                                                              const uint8_t* __restrict__ fmask, const int64_t* __restrict__ t, int acc,
                                                              float* __restrict__ out, float* __restrict__ energy) {
#pragma clang fp contract(off)
    __shared__ ClearShared sh;
    const int b = blockIdx.y, K = g.K, L = g.L, D = g.D, lane = threadIdx.x & 63;
    stage_clear_rows(g, sh.cols, sh.ir2, sh.coef);
    __syncthreads();
    float s[4];
    int f, k;
    bool live, valid;
    if (out) {
        const bool late = t && t[b] >= g.t_start;               // (uniform over the block)
        if (late) {
            const int fr = lane / K;
            k = lane - fr * K; f = blockIdx.x * g.fpb + fr;
            live = fr < g.fpb && f < L; valid = false;
            s[0] = s[1] = s[2] = 0.f;
        } else {
            clear_block_sums(g, sh, x, pos, fmask, blockIdx.x, (int64_t)b * L, L, s, &f, &k, &live, &valid);
        }
        if (pos) {
            if (threadIdx.x < 64 && live) {
                float* o = out + (((int64_t)b * L + f) * K + k) * 3;
                const float ck = sh.coef[k];
#pragma unroll
                for (int a = 0; a < 3; ++a) o[a] = valid ? ck * s[a] : 0.f;
            }
        } else {
            if (threadIdx.x < 64 && live) {
                const float ks = g.scale[b] * sh.coef[k];
                const int col = sh.cols[k];
#pragma unroll
                for (int a = 0; a < 3; ++a) {
                    const float kss = ks * g.std[col + a];
                    sh.term[lane][a] = valid ? kss * s[a] : 0.f;
                }
            }
            __syncthreads();
            const int f0 = blockIdx.x * g.fpb, nf = min(g.fpb, L - f0);
            float* rows = out + ((int64_t)b * L + f0) * D;
            for (int i = threadIdx.x; i < nf * D; i += CLEAR_THREADS) {
                const int fr = i / D, d = i - fr * D;
                float term = 0.f;
                for (int kk = 0; kk < K; ++kk) {
                    const int a = d - sh.cols[kk];
                    if (a >= 0 && a < 3) { term = sh.term[fr * K + kk][a]; break; }
                }
                rows[i] = acc ? rows[i] + term : term;
            }
        }
    }
    if (energy && blockIdx.x == 0) {
        float e = 0.f;
        const int nblk = (L + g.fpb - 1) / g.fpb;
        for (int c = 0; c < nblk; ++c) {
            clear_block_sums(g, sh, x, pos, fmask, c, (int64_t)b * L, L, s, &f, &k, &live, &valid);
            e = e + s[3];
        }
        if (threadIdx.x < 64) {
            e = wave_sum(e);
            if (threadIdx.x == 0) energy[b] = e;
        }
    }
}

// ---- the clearance of stitched long motions: every window clears its own frames of the joined motion against its own cloud, and per long
// frame the windows' sums are crossfaded with the stitch's weight row.
//
// The long pass, blocks (frame block blockIdx.x of a window, window blockIdx.y = g * S + w): clear_block_sums on the window's frames -
// positions from row g * F + a_w + f of the joined motion (`lng`, or the recovery's pos[g][F][K][3]), points from the window's cloud - and
// the raw S_b (3) and e_b of every joint-frame to Sb[b][f][k][4]; a frame at or behind F gets zeros.  tl (the gradient alone is asked for):
// a long motion with tl[g] >= t_start is skipped, the join writes its zeros without reading Sb.
__global__ __launch_bounds__(CLEAR_THREADS) void long_clear_kernel(const ClearDev g, const LongGeo lg, const float* __restrict__ lng,
                                                                   const float* __restrict__ pos, const int64_t* __restrict__ tl,
                                                                   float* __restrict__ Sb) {
    __shared__ ClearShared sh;
    const int b = blockIdx.y, K = g.K, L = g.L;
    const int gi = b / lg.S, first = (b % lg.S) * (L - lg.ov);
    if (tl && tl[gi] >= g.t_start) return;                      // (uniform over the block)
    stage_clear_rows(g, sh.cols, sh.ir2, sh.coef);
    __syncthreads();
    float s[4];
    int f, k;
    bool live, valid;
    clear_block_sums(g, sh, lng, pos, nullptr, blockIdx.x, (int64_t)gi * lg.F + first, min(L, lg.F - first), s, &f, &k, &live, &valid);
    if (threadIdx.x < 64 && live) {
        float* o = Sb + (((int64_t)b * L + f) * K + k) * 4;
#pragma unroll
        for (int a = 0; a < 4; ++a) o[a] = s[a];
    }
}

// The join, blocks (long frame block blockIdx.x, long motion blockIdx.y) of 64 / K whole long frames, lane i < 64 the joint-frame
// (f, k) = (blockIdx.x * fpb + i / K, i % K).  J = the frame's window's sum as it is, or - a shared frame, i = f - w1 * hop -
// (wl[i] * S_earlier) + (wr[i] * S_later), each product rounded, then the sum.  out, column form: the block's complete rows of grad_long -
// ((scale[g] * coef_k) * std_a) * J_a, zero in every other column and in a long motion with tl[g] >= t_start; acc: row[d] = row[d] + term
// for EVERY column.  h3d: coef_k * J_a to out = S[g][f][k][3] for the adjoint.  energy: block 0's first wave - per window, lane i adds
// omega * e_b of its joint-frame over the window's frame blocks in ascending order (omega = wl[i] / wr[i] of a shared frame in the earlier /
// later window, a frame at or behind F counts 0), one butterfly; E[g] = the windows' values added serially from 0 in window order.
__global__ __launch_bounds__(256) void long_clear_join_kernel(const ClearDev g, const LongGeo lg, const float* __restrict__ wgt,
                                                              const float* __restrict__ Sb, const int64_t* __restrict__ tl, int h3d, int acc,
                                                              float* __restrict__ out, float* __restrict__ energy) {
#pragma clang fp contract(off)
    __shared__ int scols[AFM_GUIDE_MAX_JOINTS];
    __shared__ float sir2[AFM_GUIDE_MAX_JOINTS], scoef[AFM_GUIDE_MAX_JOINTS];
    __shared__ float term[64][3];
    const int gi = blockIdx.y, K = g.K, L = g.L, D = g.D, F = lg.F, hop = L - lg.ov;
    stage_clear_rows(g, scols, sir2, scoef);
    __syncthreads();
    if (out) {
        const bool late = tl && tl[gi] >= g.t_start;            // (uniform over the block)
        const int fr = (int)threadIdx.x / K, k = (int)threadIdx.x - fr * K, f = blockIdx.x * g.fpb + fr;
        const bool live = threadIdx.x < 64 && fr < g.fpb && f < F;
        float J[3] = {0.f, 0.f, 0.f};
        if (live && !late) {
            int w1;
            const bool two = windows_of_frame(lg, L, f, &w1);
            const int fl = f - w1 * hop;
            const int64_t bl = (int64_t)gi * lg.S + w1;
            const float* sl = Sb + ((bl * L + fl) * K + k) * 4;
            if (two) {
                const float* se = Sb + (((bl - 1) * L + fl + hop) * K + k) * 4;
                const float wl = wgt[fl], wr = wgt[lg.ov + fl];
#pragma unroll
                for (int a = 0; a < 3; ++a) {
                    const float m0 = wl * se[a], m1 = wr * sl[a];
                    J[a] = m0 + m1;
                }
            } else {
#pragma unroll
                for (int a = 0; a < 3; ++a) J[a] = sl[a];
            }
        }
        if (h3d) {
            if (live) {
                float* o = out + (((int64_t)gi * F + f) * K + k) * 3;
                const float ck = scoef[k];
#pragma unroll
                for (int a = 0; a < 3; ++a) o[a] = late ? 0.f : ck * J[a];
            }
        } else {
            if (live) {
                const float ks = g.scale[gi] * scoef[k];
                const int col = scols[k];
#pragma unroll
                for (int a = 0; a < 3; ++a) {
                    const float kss = ks * g.std[col + a];
                    term[threadIdx.x][a] = late ? 0.f : kss * J[a];
                }
            }
            __syncthreads();
            const int f0 = blockIdx.x * g.fpb, nf = min(g.fpb, F - f0);
            float* rows = out + ((int64_t)gi * F + f0) * D;
            for (int i = threadIdx.x; i < nf * D; i += 256) {
                const int fr2 = i / D, d = i - fr2 * D;
                float v = 0.f;
                for (int kk = 0; kk < K; ++kk) {
                    const int a = d - scols[kk];
                    if (a >= 0 && a < 3) { v = term[fr2 * K + kk][a]; break; }
                }
                rows[i] = acc ? rows[i] + v : v;
            }
        }
    }
    if (energy && blockIdx.x == 0 && threadIdx.x < 64) {
        const int fr = (int)threadIdx.x / K, k = (int)threadIdx.x - fr * K;
        const int nblk = (L + g.fpb - 1) / g.fpb;
        float E = 0.f;
        for (int w = 0; w < lg.S; ++w) {
            const int64_t b = (int64_t)gi * lg.S + w;
            const int first = w * hop;
            float e = 0.f;
            for (int c = 0; c < nblk; ++c) {
                const int fl = c * g.fpb + fr;
                float v = 0.f;
                if (fr < g.fpb && fl < L && first + fl < F) {
                    v = Sb[((b * L + fl) * K + k) * 4 + 3];
                    if (w + 1 < lg.S && fl >= hop) v = wgt[fl - hop] * v;
                    else if (w > 0 && fl < lg.ov) v = wgt[lg.ov + fl] * v;
                }
                e = e + v;
            }
            e = wave_sum(e);
            E = E + e;
        }
        if (threadIdx.x == 0) energy[gi] = E;
    }
}

// the smallest float32 >= v: a float32 value compares with it as with v itself
float ceil_f32(double v) {
    float f = (float)v;
    if ((double)f < v) f = nextafterf(f, INFINITY);
    return f;
}

int clear_check(const afm_scene_clearance* a, int32_t L, int32_t D) {
    if (!a->q || !a->mean || !a->std || !a->scale || L <= 0 || D <= 0) return AFM_E_BADARG;
    if (a->K <= 0 || a->K > AFM_GUIDE_MAX_JOINTS || a->N <= 0 || a->up < 0 || a->up > 2) return AFM_E_BADARG;
    for (int k = 0; k < a->K; ++k)
        if (!(a->radius[k] > 0.0) || !(1.0 / (a->radius[k] * a->radius[k]) <= 3.0e38)) return AFM_E_BADARG;
    if (a->exempt && (!a->c || a->Kc <= 0)) return AFM_E_BADARG;
    if (a->has_min_height && a->min_height != a->min_height) return AFM_E_BADARG;
    if (joints_check(a->cols, a->h3d, a->K, D) != 0) return AFM_E_BADARG;
    if (L > 65535) return AFM_E_UNSUPPORTED;
    if (a->h3d && (size_t)H3D_SCAN_ROWS * L * 4 > (size_t)GUIDE_LDS_BYTES) return AFM_E_UNSUPPORTED;
    return 0;
}

// what the clearance kernels take of a description: the clouds from sample (window) `cloud0` on, the scale rows from `scale0` on (a long
// motion's windows have one), L frames per sample
ClearDev clear_dev(const afm_scene_clearance* a, int64_t cloud0, int64_t scale0, int32_t L, int32_t D) {
    ClearDev g = {};
    g.q = a->q + cloud0 * a->N * 3;
    g.weight = a->weight ? a->weight + cloud0 * a->N : nullptr;
    g.c = a->exempt ? a->c + cloud0 * a->N * a->Kc : nullptr;
    g.mean = a->mean; g.std = a->std; g.scale = a->scale + scale0;
    for (int k = 0; k < a->K; ++k) {
        g.cols[k] = a->h3d ? 0 : a->cols[k];
        const double r2 = a->radius[k] * a->radius[k];
        g.ir2[k] = (float)(1.0 / r2);
        g.coef[k] = (float)(4.0 / r2);
    }
    g.K = a->K; g.N = a->N; g.Kc = a->Kc; g.L = L; g.D = D; g.up = a->up; g.fpb = 64 / a->K;
    g.min_height = a->has_min_height ? ceil_f32(a->min_height) : -INFINITY;
    g.c_min = a->exempt ? ceil_f32(a->c_min) : INFINITY;
    g.t_start = a->t_start;
    return g;
}

// h3d: positions and S [count][L][K][3], c / s [count][L][2]; added to the terms in front: the adjoint's own rows [count][L][D]
int64_t clear_workspace_bytes(const afm_scene_clearance* a, bool add, int64_t count, int64_t L, int64_t D) {
    if (!a->h3d) return 0;
    return h3d_extra_bytes(count, L, a->K) + (add ? afm_loop::align256(count * L * D * 4) : 0);
}

// the clearance's launches on the samples [start, start + count); add: grad holds the result of the terms in front, the sum goes there
int clear_sub(const afm_scene_clearance* a, bool add, int32_t start, const float* x, const uint8_t* frame_mask, const int64_t* t, float* grad,
              float* energy, int32_t count, int32_t L, int32_t D, char* wp, hipStream_t s) {
    const ClearDev g = clear_dev(a, start, start, L, D);
    const unsigned nblk = (unsigned)((L + g.fpb - 1) / g.fpb);
    const dim3 grid(grad ? nblk : 1u, (unsigned)count);
    if (!a->h3d) {
        hipLaunchKernelGGL(clear_kernel, grid, dim3(CLEAR_THREADS), 0, s, g, x, (const float*)nullptr, frame_mask, t, add ? 1 : 0, grad, energy);
        AFM_CHECK_LAUNCH();
        return 0;
    }
    const H3dPlan p = h3d_plan(a->mean, a->std, g.scale, *a->h3d, a->K, L, D, start, count, false, 1.f, a->t_start, wp);
    float* tmp = (float*)p.end;                     // (add: the adjoint's own rows [count][L][D])
    hipLaunchKernelGGL(h3d_recover_kernel, dim3((unsigned)count), dim3(256), p.scan_lds, s, p.rec, x, frame_mask, p.pos, grad ? p.cs : nullptr);
    AFM_CHECK_LAUNCH();
    hipLaunchKernelGGL(clear_kernel, grid, dim3(CLEAR_THREADS), 0, s, g, x, (const float*)p.pos, frame_mask, (const int64_t*)nullptr, 0,
                       grad ? p.S : nullptr, energy);
    AFM_CHECK_LAUNCH();
    if (!grad) return 0;
    if (add) hipLaunchKernelGGL(h3d_adjoint_add_kernel, dim3((unsigned)count), dim3(256), p.scan_lds, s, p.adj, x, frame_mask, t, p.cs, p.S, tmp, grad);
    else hipLaunchKernelGGL(h3d_adjoint_kernel, dim3((unsigned)count), dim3(256), p.scan_lds, s, p.adj, x, frame_mask, t, p.cs, p.S, grad);
    AFM_CHECK_LAUNCH();
    return 0;
}

// the long clearance's buffers of `count` long motions: the windows' raw sums Sb [count * S][L][K][4], then - h3d - the recovery's and the
// adjoint's of (count, F), with the adjoint's own rows when its result is added
int64_t long_clear_workspace_bytes(const afm_scene_clearance* a, bool add, int64_t count, int64_t S, int64_t L, int64_t F, int64_t D) {
    return afm_loop::align256(count * S * L * a->K * 16) + clear_workspace_bytes(a, add, count, F, D);
}

// the long clearance's launches on the long motions [start, start + count): lng / glong [count][F][D] the joined motion and its gradient,
// tl [count] or NULL; add: glong holds the result of the terms in front, the sum goes there.  Column form: the long pass and the join;
// h3d: recovery over F frames, long pass, join, adjoint.
int long_clear_sub(const afm_scene_clearance* a, const afm_stitch& st, int32_t F, bool add, int32_t start, const float* lng, const int64_t* tl,
                   float* glong, float* energy, int32_t count, int32_t L, int32_t D, char* wp, hipStream_t s) {
    const int S = st.windows, wins = count * S;
    const ClearDev g = clear_dev(a, (int64_t)start * S, start, L, D);
    const LongGeo lg = {S, st.overlap, F};
    float* Sb = (float*)wp; wp += afm_loop::align256((int64_t)wins * L * a->K * 16);
    const dim3 g1((unsigned)((L + g.fpb - 1) / g.fpb), (unsigned)wins), g2(glong ? (unsigned)((F + g.fpb - 1) / g.fpb) : 1u, (unsigned)count);
    const int64_t* skip = energy ? nullptr : tl;                // (the energy reads every long motion's sums)
    if (!a->h3d) {
        hipLaunchKernelGGL(long_clear_kernel, g1, dim3(CLEAR_THREADS), 0, s, g, lg, lng, (const float*)nullptr, skip, Sb);
        AFM_CHECK_LAUNCH();
        hipLaunchKernelGGL(long_clear_join_kernel, g2, dim3(256), 0, s, g, lg, st.weights, (const float*)Sb, tl, 0, add ? 1 : 0, glong, energy);
        AFM_CHECK_LAUNCH();
        return 0;
    }
    const H3dPlan p = h3d_plan(a->mean, a->std, g.scale, *a->h3d, a->K, F, D, start, count, false, 1.f, a->t_start, wp);
    float* tmp = (float*)p.end;                     // (add: the adjoint's own rows [count][F][D])
    hipLaunchKernelGGL(h3d_recover_kernel, dim3((unsigned)count), dim3(256), p.scan_lds, s, p.rec, lng, (const uint8_t*)nullptr, p.pos,
                       glong ? p.cs : nullptr);
    AFM_CHECK_LAUNCH();
    hipLaunchKernelGGL(long_clear_kernel, g1, dim3(CLEAR_THREADS), 0, s, g, lg, lng, (const float*)p.pos, skip, Sb);
    AFM_CHECK_LAUNCH();
    hipLaunchKernelGGL(long_clear_join_kernel, g2, dim3(256), 0, s, g, lg, st.weights, (const float*)Sb, tl, 1, 0, glong ? p.S : nullptr, energy);
    AFM_CHECK_LAUNCH();
    if (!glong) return 0;
    if (add) hipLaunchKernelGGL(h3d_adjoint_add_kernel, dim3((unsigned)count), dim3(256), p.scan_lds, s, p.adj, lng, (const uint8_t*)nullptr, tl, p.cs,
                                p.S, tmp, glong);
    else hipLaunchKernelGGL(h3d_adjoint_kernel, dim3((unsigned)count), dim3(256), p.scan_lds, s, p.adj, lng, (const uint8_t*)nullptr, tl, p.cs, p.S,
                            glong);
    AFM_CHECK_LAUNCH();
    return 0;
}

inline const afm_motion_guide* set_terms(const afm_motion_guide* terms) { return terms && (terms->contact || terms->targets) ? terms : nullptr; }

// a sum's terms and the clearance next to them describe one motion: the same mean / std, the same form, the same to_scene
bool terms_agree(const afm_motion_guide* terms, const afm_scene_clearance* clear) {
    const float *mean = terms->contact ? terms->contact->mean : terms->targets->mean, *std = terms->contact ? terms->contact->std : terms->targets->std;
    const afm_h3d_layout* h = terms->contact ? terms->contact->h3d : terms->targets->h3d;
    if (mean != clear->mean || std != clear->std || !h != !clear->h3d) return false;
    return !h || (h->to_scene == clear->h3d->to_scene && h->to_scene_stride == clear->h3d->to_scene_stride);
}

}  // namespace

__attribute__((visibility("hidden"))) int afm_scene_guide_check(const afm_motion_guide* terms, const afm_scene_clearance* clear, int32_t L, int32_t D) {
    terms = set_terms(terms);
    if (!terms && !clear) return AFM_E_BADARG;
    if (terms) {
        const int rc = afm_motion_guide_check(terms, L, D);
        if (rc != 0) return rc;
    }
    if (!clear) return 0;
    const int rc = clear_check(clear, L, D);
    if (rc != 0) return rc;
    if (terms && !terms_agree(terms, clear)) return AFM_E_BADARG;
    return 0;
}

// the workspace of `count` samples of a checked sum: the terms', then the clearance's
__attribute__((visibility("hidden"))) int64_t afm_scene_guide_workspace_bytes(const afm_motion_guide* terms, const afm_scene_clearance* clear, int32_t count,
                                                                              int32_t L, int32_t D) {
    terms = set_terms(terms);
    const int64_t n = terms ? afm_motion_guide_workspace_bytes(terms, count, L, D) : 0;
    return clear ? afm_loop::align256(n) + clear_workspace_bytes(clear, terms != nullptr, count, L, D) : n;
}

__attribute__((visibility("hidden"))) int afm_scene_guidance_sub(const afm_motion_guide* terms, const afm_scene_clearance* clear, bool run_contact,
                                                                 bool run_targets, bool run_clear, int32_t start, const float* x, const uint8_t* frame_mask,
                                                                 const int64_t* t, float* grad, float* energy_contact, float* energy_targets,
                                                                 float* energy_clear, int32_t count, int32_t L, int32_t D, void* workspace,
                                                                 int64_t workspace_bytes, void* stream) {
    terms = set_terms(terms);
    const int rc = afm_scene_guide_check(terms, clear, L, D);
    if (rc != 0) return rc;
    run_contact = run_contact && terms && terms->contact;
    run_targets = run_targets && terms && terms->targets;
    run_clear = run_clear && clear;
    if (!x || (!grad && !energy_contact && !energy_targets && !energy_clear) || start < 0 || count < 0 || (energy_contact && !run_contact) ||
        (energy_targets && !run_targets) || (energy_clear && !run_clear) || (!run_contact && !run_targets && !run_clear)) return AFM_E_BADARG;
    if (count > 65535) return AFM_E_UNSUPPORTED;
    if (count == 0) return 0;
    if (!workspace || workspace_bytes < afm_scene_guide_workspace_bytes(terms, clear, count, L, D)) return AFM_E_WORKSPACE;
    const int64_t tbytes = terms ? afm_loop::align256(afm_motion_guide_workspace_bytes(terms, count, L, D)) : 0;
    const bool front = (run_contact || run_targets) && (grad || energy_contact || energy_targets);
    if (front) {
        const int rcm = afm_motion_guidance_sub(terms, run_contact, run_targets, start, x, frame_mask, t, grad, energy_contact, energy_targets, count, L, D,
                                                workspace, tbytes, stream);
        if (rcm != 0) return rcm;
    }
    if (run_clear && (grad || energy_clear))
        return clear_sub(clear, front && grad, start, x, frame_mask, t, grad, energy_clear, count, L, D, (char*)workspace + tbytes, (hipStream_t)stream);
    return 0;
}

extern "C" int64_t afm_scene_guidance_workspace_bytes(const afm_scene_guide* g, int32_t B, int32_t L, int32_t D) {
    if (!g || B < 0 || afm_scene_guide_check(g->terms, g->clearance, L, D) != 0) return AFM_E_BADARG;
    return afm_scene_guide_workspace_bytes(g->terms, g->clearance, B, L, D) + 256;          // (never zero: the column forms need none)
}

extern "C" int afm_scene_guidance(const afm_scene_guide* g, const float* x, const uint8_t* frame_mask, const int64_t* t, float* grad,
                                  float* energy_contact, float* energy_targets, float* energy_clearance, int32_t B, int32_t L, int32_t D,
                                  void* workspace, int64_t workspace_bytes, void* stream) {
    if (!g) return AFM_E_BADARG;
    return afm_scene_guidance_sub(g->terms, g->clearance, true, true, true, 0, x, frame_mask, t, grad, energy_contact, energy_targets, energy_clearance, B, L,
                                  D, workspace, workspace_bytes, stream);
}

// ---- foot grounding (afm_foot_grounding): the one term that couples frame f with frame f + 1.  A block owns GROUND_FPB frames of one
// sample and keeps their K x 3 positions and validity flags, and those of one neighbouring frame on either side, in LDS, so every item
// (f, k) reads its joint's neighbouring frames from there; the contact weights of a pair are recomputed by both of its frames from the
// same staged values, hence with the same bits.  The energy, a score, is summed by the sample's block 0 alone, which then stages the whole
// sample (the contact term's fit: (3 K + 1) L floats).
namespace {

struct GroundDev {
    const float *mean, *std, *scale;
    int cols[AFM_GUIDE_MAX_JOINTS];
    int lab[AFM_GUIDE_MAX_JOINTS];          // the label column of joint k (contact = labels), else -1
    float ih[AFM_GUIDE_MAX_JOINTS];         // 1 / height_k, rounded once from float64
    int K, L, D, up, ax0, ax1;              // ax0 < ax1: the two axes that are not `up`
    float floor, fw, sw, cf, cs;            // floor_weight, skate_weight, 2 * floor_weight, 2 * skate_weight, each rounded once
    int64_t t_start;
};

struct GroundRows {
    int cols[AFM_GUIDE_MAX_JOINTS], lab[AFM_GUIDE_MAX_JOINTS];
    float ih[AFM_GUIDE_MAX_JOINTS];
};

constexpr int GROUND_FPB = 8;               // frames per block: a block stages its frames and one neighbour on either side

// the frames [fs0, fs1) of the sample staged in LDS: positions [fs1 - fs0][K][3] and the validity flags
struct GroundView {
    const float* sp;
    const int* sval;
    int fs0;
};

__device__ __forceinline__ float ground_p(const GroundDev& g, const GroundView& v, int f, int k, int a) { return v.sp[((f - v.fs0) * g.K + k) * 3 + a]; }

// g = min(1, max(0, 1 - h * ih)) of the staged joint-frame (f, k)
__device__ __forceinline__ float ground_gate(const GroundDev& g, const GroundView& v, int f, int k, float ih) {
#pragma clang fp contract(off)
    const float h = ground_p(g, v, f, k, g.up) - g.floor;
    const float m = h * ih;
    return fminf(1.f, fmaxf(0.f, 1.f - m));
}

// s[f,k]: the weight of the pair (f, f + 1) of joint k - 0 unless both frames exist and are valid
__device__ __forceinline__ float ground_pair(const GroundDev& g, const GroundRows& r, const GroundView& v, const float* __restrict__ xb, int f, int k) {
#pragma clang fp contract(off)
    if (f < 0 || f + 1 >= g.L || !v.sval[f - v.fs0] || !v.sval[f + 1 - v.fs0]) return 0.f;
    if (r.lab[k] >= 0) return fminf(1.f, fmaxf(0.f, denorm(xb + (int64_t)f * g.D, g.mean, g.std, r.lab[k])));
    const float g0 = ground_gate(g, v, f, k, r.ih[k]), g1 = ground_gate(g, v, f + 1, k, r.ih[k]);
    return g0 * g1;
}

// s * (p[f+1,k,a] - p[f,k,a]) of a pair with weight s (0: nothing is read)
__device__ __forceinline__ float ground_slide(const GroundDev& g, const GroundView& v, float s, int f, int k, int a) {
#pragma clang fp contract(off)
    if (s == 0.f) return 0.f;
    const float dl = ground_p(g, v, f + 1, k, a) - ground_p(g, v, f, k, a);
    return s * dl;
}

// m[f,k,:] of a valid frame's item: m_up = cf * pen, m_a = cs * (s[f] * dl_a[f] - s[f-1] * dl_a[f-1])
__device__ __forceinline__ void ground_item(const GroundDev& g, const GroundRows& r, const GroundView& v, const float* __restrict__ xb, int f, int k,
                                            float m[3]) {
#pragma clang fp contract(off)
    const float h = ground_p(g, v, f, k, g.up) - g.floor;
    const float pen = fmaxf(0.f, -h);
    const float s1 = ground_pair(g, r, v, xb, f, k), s0 = ground_pair(g, r, v, xb, f - 1, k);
    const float mu = g.cf * pen;
    const float u0 = ground_slide(g, v, s1, f, k, g.ax0), v0 = ground_slide(g, v, s0, f - 1, k, g.ax0);
    const float u1 = ground_slide(g, v, s1, f, k, g.ax1), v1 = ground_slide(g, v, s0, f - 1, k, g.ax1);
    const float m0 = g.cs * (u0 - v0), m1 = g.cs * (u1 - v1);
#pragma unroll
    for (int a = 0; a < 3; ++a) m[a] = a == g.up ? mu : (a == g.ax0 ? m0 : m1);          // (static indices: the array stays in registers)
}

// One launch, blocks (frame block blockIdx.x, sample blockIdx.y); a block owns the frames [f0, f1), f0 = blockIdx.x * GROUND_FPB, and stages
// them with one neighbour on either side.  pos == NULL, the column form: p = the de-normalised columns; out = the block's complete grad
// rows - grad[b,f,cols[k]+a] = (scale[b] * std_a) * m_a, zero in every other column, in a padded frame and in a sample with
// t[b] >= t_start; ACC: row[d] = row[d] + term for EVERY column (one rounded addition per element on what the terms in front wrote).
// pos set, the h3d form: p = the recovery's positions [b][f][k][3]; out = S[b][f][k][3] = m (zero in a padded frame) for the adjoint, whose
// business scale, t_start and the rows are.  energy: the sample's block 0 stages every frame and thread i adds the items
// e = f * K + k = i, i + 256, ... in that order (a padded frame's item counts as 0 and is skipped),
// item = fw * (pen * pen) + sw * (s * (dl_a0 * dl_a0 + dl_a1 * dl_a1)), then block_sum (a score, not part of a sampling step).
template <bool ACC>
__global__ __launch_bounds__(256) void ground_kernel(const GroundDev g, const float* __restrict__ x, const float* __restrict__ pos,
                                                     const uint8_t* __restrict__ fmask, const int64_t* __restrict__ t, float* __restrict__ out,
                                                     float* __restrict__ energy) {
#pragma clang fp contract(off)
    extern __shared__ float gsh[];                  // positions [frames staged][K][3], then their validity flags
    __shared__ GroundRows r;
    __shared__ float red[4];
    const int b = blockIdx.y, K = g.K, L = g.L, D = g.D;
    const bool whole = energy && blockIdx.x == 0;               // (uniform over the block)
    const int f0 = blockIdx.x * GROUND_FPB, f1 = min(L, f0 + GROUND_FPB);
    const int fs0 = whole ? 0 : max(0, f0 - 1), fs1 = whole ? L : min(L, f1 + 1), nfs = fs1 - fs0;
    float* sp = gsh;
    int* sval = reinterpret_cast<int*>(gsh + (size_t)nfs * K * 3);
#pragma unroll
    for (int k = 0; k < AFM_GUIDE_MAX_JOINTS; ++k)
        if (threadIdx.x == k) { r.cols[k] = g.cols[k]; r.lab[k] = g.lab[k]; r.ih[k] = g.ih[k]; }
    __syncthreads();
    const float* xb = x + (int64_t)b * L * D;
    const bool late = !pos && t && t[b] >= g.t_start;           // (uniform over the block)
    for (int i = threadIdx.x; i < nfs; i += 256) sval[i] = !(fmask && fmask[(int64_t)b * L + fs0 + i]);
    for (int e = threadIdx.x; e < nfs * K; e += 256) {
        const int fr = e / K, k = e - fr * K, f = fs0 + fr;
        float p0 = 0.f, p1 = 0.f, p2 = 0.f;
        if (!(fmask && fmask[(int64_t)b * L + f])) {
            if (pos) {
                const float* pp = pos + (((int64_t)b * L + f) * K + k) * 3;
                p0 = pp[0]; p1 = pp[1]; p2 = pp[2];
            } else {
                const float* xrow = xb + (int64_t)f * D;
                const int col = r.cols[k];
                p0 = denorm(xrow, g.mean, g.std, col); p1 = denorm(xrow, g.mean, g.std, col + 1); p2 = denorm(xrow, g.mean, g.std, col + 2);
            }
        }
        sp[e * 3] = p0; sp[e * 3 + 1] = p1; sp[e * 3 + 2] = p2;
    }
    __syncthreads();
    const GroundView v = {sp, sval, fs0};
    if (whole) {
        float acc = 0.f;
        for (int e = threadIdx.x; e < L * K; e += 256) {
            const int f = e / K, k = e - f * K;
            if (!sval[f]) continue;
            const float h = ground_p(g, v, f, k, g.up) - g.floor;
            const float pen = fmaxf(0.f, -h);
            const float ef = g.fw * (pen * pen);
            const float s = ground_pair(g, r, v, xb, f, k);
            float es = 0.f;
            if (s != 0.f) {
                const float d0 = ground_p(g, v, f + 1, k, g.ax0) - ground_p(g, v, f, k, g.ax0);
                const float d1 = ground_p(g, v, f + 1, k, g.ax1) - ground_p(g, v, f, k, g.ax1);
                const float q0 = d0 * d0, q1 = d1 * d1;
                es = g.sw * (s * (q0 + q1));
            }
            acc = acc + (ef + es);
        }
        acc = block_sum(acc, red);
        if (threadIdx.x == 0) energy[b] = acc;
    }
    if (!out || f0 >= L) return;
    const int nf = f1 - f0;
    if (pos) {
        for (int e = threadIdx.x; e < nf * K; e += 256) {
            const int fr = e / K, k = e - fr * K, f = f0 + fr;
            float m[3] = {0.f, 0.f, 0.f};
            if (sval[f - fs0]) ground_item(g, r, v, xb, f, k, m);
            float* o = out + (((int64_t)b * L + f) * K + k) * 3;
            o[0] = m[0]; o[1] = m[1]; o[2] = m[2];
        }
        return;
    }
    float* rows = out + ((int64_t)b * L + f0) * D;
    const float sc = g.scale[b];
    for (int i = threadIdx.x; i < nf * D; i += 256) {
        const int fr = i / D, d = i - fr * D, f = f0 + fr;
        float term = 0.f;
        if (!late && sval[f - fs0])
            for (int k = 0; k < K; ++k) {
                const int a = d - r.cols[k];
                if (a < 0 || a >= 3) continue;
                float m[3];
                ground_item(g, r, v, xb, f, k, m);
                const float ma = a == 0 ? m[0] : (a == 1 ? m[1] : m[2]);
                term = (sc * g.std[d]) * ma;
                break;
            }
        rows[i] = ACC ? rows[i] + term : term;
    }
}

constexpr int GROUND_LABEL_COL = 259;       // HumanML3D's foot-contact columns 259..262: left foot (joints 7, 10), then right (8, 11)

int ground_label_slot(int joint) { return joint == 7 ? 0 : joint == 10 ? 1 : joint == 8 ? 2 : joint == 11 ? 3 : -1; }

int ground_check(const afm_foot_grounding* a, int32_t L, int32_t D) {
    if (!a->mean || !a->std || !a->scale || L <= 0 || D <= 0) return AFM_E_BADARG;
    if (a->K <= 0 || a->K > AFM_GUIDE_MAX_JOINTS || a->up < 0 || a->up > 2) return AFM_E_BADARG;
    for (int k = 0; k < a->K; ++k)
        if (!(a->height[k] > 0.0) || !(1.0 / a->height[k] <= 3.0e38)) return AFM_E_BADARG;
    if (!(a->floor_weight >= 0.0) || !(a->skate_weight >= 0.0) || !(a->floor_weight + a->skate_weight > 0.0) ||
        !(a->floor_weight <= 1.0e38) || !(a->skate_weight <= 1.0e38) || !(a->floor == a->floor)) return AFM_E_BADARG;
    if (joints_check(a->cols, a->h3d, a->K, D) != 0) return AFM_E_BADARG;
    if (a->labels) {
        if (!a->h3d || D < GROUND_LABEL_COL + 4) return AFM_E_BADARG;
        for (int k = 0; k < a->K; ++k)
            if (ground_label_slot(a->h3d->joints[k]) < 0) return AFM_E_BADARG;
    }
    if (((size_t)a->K * L * 3 + L) * 4 > (size_t)GUIDE_LDS_BYTES || L > 65535) return AFM_E_UNSUPPORTED;
    if (a->h3d && (size_t)H3D_SCAN_ROWS * L * 4 > (size_t)GUIDE_LDS_BYTES) return AFM_E_UNSUPPORTED;
    return 0;
}

// h3d: positions and S [count][L][K][3], c / s [count][L][2]; added to the terms in front: the adjoint's own rows [count][L][D]
int64_t ground_workspace_bytes(const afm_foot_grounding* a, bool add, int64_t count, int64_t L, int64_t D) {
    if (!a->h3d) return 0;
    return h3d_extra_bytes(count, L, a->K) + (add ? afm_loop::align256(count * L * D * 4) : 0);
}

// the grounding's launches on the samples [start, start + count); add: grad holds the result of the terms in front, the sum goes there
int ground_sub(const afm_foot_grounding* a, bool add, int32_t start, const float* x, const uint8_t* frame_mask, const int64_t* t, float* grad,
               float* energy, int32_t count, int32_t L, int32_t D, char* wp, hipStream_t s) {
    GroundDev g = {};
    g.mean = a->mean; g.std = a->std; g.scale = a->scale + start;
    for (int k = 0; k < AFM_GUIDE_MAX_JOINTS; ++k) { g.cols[k] = 0; g.lab[k] = -1; g.ih[k] = 0.f; }
    for (int k = 0; k < a->K; ++k) {
        g.cols[k] = a->h3d ? 0 : a->cols[k];
        g.lab[k] = a->labels ? GROUND_LABEL_COL + ground_label_slot(a->h3d->joints[k]) : -1;
        g.ih[k] = (float)(1.0 / a->height[k]);
    }
    g.K = a->K; g.L = L; g.D = D; g.up = a->up;
    g.ax0 = a->up == 0 ? 1 : 0; g.ax1 = a->up == 2 ? 1 : 2;
    g.floor = (float)a->floor;
    g.fw = (float)a->floor_weight; g.sw = (float)a->skate_weight;
    g.cf = (float)(2.0 * a->floor_weight); g.cs = (float)(2.0 * a->skate_weight);
    g.t_start = a->t_start;
    // (the energy's block stages the whole sample; a launch without it GROUND_FPB frames and the two around them)
    const size_t lds = ((size_t)a->K * 3 + 1) * (energy || L < GROUND_FPB + 2 ? L : GROUND_FPB + 2) * 4;
    const dim3 grid(grad ? (unsigned)((L + GROUND_FPB - 1) / GROUND_FPB) : 1u, (unsigned)count);
    if (!a->h3d) {
        if (add) hipLaunchKernelGGL(ground_kernel<true>, grid, dim3(256), lds, s, g, x, (const float*)nullptr, frame_mask, t, grad, energy);
        else hipLaunchKernelGGL(ground_kernel<false>, grid, dim3(256), lds, s, g, x, (const float*)nullptr, frame_mask, t, grad, energy);
        AFM_CHECK_LAUNCH();
        return 0;
    }
    const H3dPlan p = h3d_plan(a->mean, a->std, g.scale, *a->h3d, a->K, L, D, start, count, false, 1.f, a->t_start, wp);
    float* tmp = (float*)p.end;                     // (add: the adjoint's own rows [count][L][D])
    hipLaunchKernelGGL(h3d_recover_kernel, dim3((unsigned)count), dim3(256), p.scan_lds, s, p.rec, x, frame_mask, p.pos, grad ? p.cs : nullptr);
    AFM_CHECK_LAUNCH();
    hipLaunchKernelGGL(ground_kernel<false>, grid, dim3(256), lds, s, g, x, (const float*)p.pos, frame_mask, (const int64_t*)nullptr,
                       grad ? p.S : nullptr, energy);
    AFM_CHECK_LAUNCH();
    if (!grad) return 0;
    if (add) hipLaunchKernelGGL(h3d_adjoint_add_kernel, dim3((unsigned)count), dim3(256), p.scan_lds, s, p.adj, x, frame_mask, t, p.cs, p.S, tmp, grad);
    else hipLaunchKernelGGL(h3d_adjoint_kernel, dim3((unsigned)count), dim3(256), p.scan_lds, s, p.adj, x, frame_mask, t, p.cs, p.S, grad);
    AFM_CHECK_LAUNCH();
    return 0;
}

// the grounding and the terms in front of it describe one motion: the same mean / std, the same form, the same to_scene
bool feet_agree(const afm_motion_guide* terms, const afm_scene_clearance* clear, const afm_foot_grounding* feet) {
    const float *mean, *std;
    const afm_h3d_layout* h;
    if (clear) { mean = clear->mean; std = clear->std; h = clear->h3d; }
    else if (terms->contact) { mean = terms->contact->mean; std = terms->contact->std; h = terms->contact->h3d; }
    else { mean = terms->targets->mean; std = terms->targets->std; h = terms->targets->h3d; }
    if (mean != feet->mean || std != feet->std || !h != !feet->h3d) return false;
    return !h || (h->to_scene == feet->h3d->to_scene && h->to_scene_stride == feet->h3d->to_scene_stride);
}

}  // namespace

// the sum with the foot grounding; feet == NULL: afm_scene_guide_check / _workspace_bytes / afm_scene_guidance_sub exactly
__attribute__((visibility("hidden"))) int afm_ground_guide_check(const afm_motion_guide* terms, const afm_scene_clearance* clear,
                                                                 const afm_foot_grounding* feet, int32_t L, int32_t D) {
    terms = set_terms(terms);
    if (!feet) return afm_scene_guide_check(terms, clear, L, D);
    if (terms || clear) {
        const int rc = afm_scene_guide_check(terms, clear, L, D);
        if (rc != 0) return rc;
    }
    const int rc = ground_check(feet, L, D);
    if (rc != 0) return rc;
    if ((terms || clear) && !feet_agree(terms, clear, feet)) return AFM_E_BADARG;
    return 0;
}

__attribute__((visibility("hidden"))) int64_t afm_ground_guide_workspace_bytes(const afm_motion_guide* terms, const afm_scene_clearance* clear,
                                                                               const afm_foot_grounding* feet, int32_t count, int32_t L, int32_t D) {
    terms = set_terms(terms);
    const int64_t n = terms || clear ? afm_scene_guide_workspace_bytes(terms, clear, count, L, D) : 0;
    return feet ? afm_loop::align256(n) + ground_workspace_bytes(feet, terms || clear, count, L, D) : n;
}

__attribute__((visibility("hidden"))) int afm_ground_guidance_sub(const afm_motion_guide* terms, const afm_scene_clearance* clear,
                                                                  const afm_foot_grounding* feet, bool run_contact, bool run_targets, bool run_clear,
                                                                  bool run_feet, int32_t start, const float* x, const uint8_t* frame_mask,
                                                                  const int64_t* t, float* grad, float* energy_contact, float* energy_targets,
                                                                  float* energy_clear, float* energy_feet, int32_t count, int32_t L, int32_t D,
                                                                  void* workspace, int64_t workspace_bytes, void* stream) {
    terms = set_terms(terms);
    if (!feet) {
        if (energy_feet) return AFM_E_BADARG;
        return afm_scene_guidance_sub(terms, clear, run_contact, run_targets, run_clear, start, x, frame_mask, t, grad, energy_contact, energy_targets,
                                      energy_clear, count, L, D, workspace, workspace_bytes, stream);
    }
    const int rc = afm_ground_guide_check(terms, clear, feet, L, D);
    if (rc != 0) return rc;
    run_contact = run_contact && terms && terms->contact;
    run_targets = run_targets && terms && terms->targets;
    run_clear = run_clear && clear;
    if (!x || (!grad && !energy_contact && !energy_targets && !energy_clear && !energy_feet) || start < 0 || count < 0 ||
        (energy_contact && !run_contact) || (energy_targets && !run_targets) || (energy_clear && !run_clear) || (energy_feet && !run_feet) ||
        (!run_contact && !run_targets && !run_clear && !run_feet)) return AFM_E_BADARG;
    if (count > 65535) return AFM_E_UNSUPPORTED;
    if (count == 0) return 0;
    if (!workspace || workspace_bytes < afm_ground_guide_workspace_bytes(terms, clear, feet, count, L, D)) return AFM_E_WORKSPACE;
    const int64_t fbytes = terms || clear ? afm_loop::align256(afm_scene_guide_workspace_bytes(terms, clear, count, L, D)) : 0;
    const bool front = (run_contact || run_targets || run_clear) && (grad || energy_contact || energy_targets || energy_clear);
    if (front) {
        const int rcs = afm_scene_guidance_sub(terms, clear, run_contact, run_targets, run_clear, start, x, frame_mask, t, grad, energy_contact,
                                               energy_targets, energy_clear, count, L, D, workspace, fbytes, stream);
        if (rcs != 0) return rcs;
    }
    if (run_feet && (grad || energy_feet))
        return ground_sub(feet, front && grad, start, x, frame_mask, t, grad, energy_feet, count, L, D, (char*)workspace + fbytes, (hipStream_t)stream);
    return 0;
}

namespace {
inline const afm_motion_guide* ground_motion(const afm_ground_guide* g) { return g->terms ? g->terms->terms : nullptr; }
inline const afm_scene_clearance* ground_clear(const afm_ground_guide* g) { return g->terms ? g->terms->clearance : nullptr; }
}  // namespace

extern "C" int64_t afm_ground_guidance_workspace_bytes(const afm_ground_guide* g, int32_t B, int32_t L, int32_t D) {
    if (!g || B < 0 || afm_ground_guide_check(ground_motion(g), ground_clear(g), g->feet, L, D) != 0) return AFM_E_BADARG;
    return afm_ground_guide_workspace_bytes(ground_motion(g), ground_clear(g), g->feet, B, L, D) + 256;          // (never zero)
}

extern "C" int afm_ground_guidance(const afm_ground_guide* g, const float* x, const uint8_t* frame_mask, const int64_t* t, float* grad,
                                   float* energy_contact, float* energy_targets, float* energy_clearance, float* energy_feet, int32_t B, int32_t L,
                                   int32_t D, void* workspace, int64_t workspace_bytes, void* stream) {
    if (!g) return AFM_E_BADARG;
    return afm_ground_guidance_sub(ground_motion(g), ground_clear(g), g->feet, true, true, true, true, 0, x, frame_mask, t, grad, energy_contact,
                                   energy_targets, energy_clearance, energy_feet, B, L, D, workspace, workspace_bytes, stream);
}

// ---- the guidance of stitched long motions (afm_long_guide): the windows joined, the terms evaluated on the long motion, one gradient per
// long frame handed back to the windows
namespace {

bool long_geometry_ok(const afm_long_guide* g, int32_t L) {
    const int64_t S = g->stitch.windows, ov = g->stitch.overlap, F = g->frames;
    if (S < 1 || ov < 0 || L <= 0 || 2 * ov > L) return false;
    return F > (S - 1) * (L - ov) + (S > 1 ? ov : 0) && F <= S * L - (S - 1) * ov;
}

// the buffers of `count` long motions in front of the terms' own: the joined motion and its gradient [count][F][D], t per long motion
struct LongPlan {
    float *lng, *glong;
    int64_t* tl;
    char *cws, *tws, *lws;          // the contact term's buffers (its windows', then the h3d form's of the long motion), the targets', the clearance's
    int64_t cbytes, bytes;
};

LongPlan long_plan(const afm_long_guide* g, int64_t count, int32_t L, int32_t D, char* wp, const afm_scene_clearance* clear = nullptr) {
    const afm_motion_guide* m = g->terms;
    const int64_t F = g->frames, S = g->stitch.windows;
    LongPlan p = {};
    char* base = wp;
    const int64_t fd = afm_loop::align256(count * F * D * 4);
    p.lng = (float*)wp; wp += fd;
    p.glong = (float*)wp; wp += fd;
    p.tl = (int64_t*)wp; wp += afm_loop::align256(count * 8);
    p.cws = wp;
    if (m->contact) {
        p.cbytes = afm_loop::align256(afm_contact_guidance_workspace_bytes((int32_t)(count * S), m->contact->N, m->contact->K));
        if (m->contact->h3d) p.cbytes += h3d_extra_bytes(count, F, m->contact->K);
    }
    wp += p.cbytes;
    p.tws = wp;
    if (m->targets) wp += targets_workspace_bytes(m->targets, m->contact != nullptr, count, F, D);
    p.lws = wp;
    if (clear) wp += long_clear_workspace_bytes(clear, m->contact || m->targets, count, S, L, F, D);
    p.bytes = wp - base;
    return p;
}

}  // namespace

// what a long description must satisfy before anything is enqueued (L, D: the windows')
__attribute__((visibility("hidden"))) int afm_long_guide_check(const afm_long_guide* g, int32_t L, int32_t D) {
    if (!g || !g->terms || !long_geometry_ok(g, L)) return AFM_E_BADARG;
    const int rc = afm_motion_guide_check(g->terms, L, D);
    if (rc != 0) return rc;
    const afm_motion_guide* m = g->terms;
    if (g->frames > 65535) return AFM_E_UNSUPPORTED;
    if (((m->contact && m->contact->h3d) || (m->targets && m->targets->h3d)) && (size_t)H3D_SCAN_ROWS * g->frames * 4 > (size_t)GUIDE_LDS_BYTES)
        return AFM_E_UNSUPPORTED;           // the recovery and the adjoint hold 7 * F floats in LDS
    return m->targets ? targets_check(m->targets, g->frames, D) : 0;
}

// the workspace of `count` long motions of a checked description
__attribute__((visibility("hidden"))) int64_t afm_long_guide_workspace_bytes(const afm_long_guide* g, int32_t count, int32_t L, int32_t D) {
    return long_plan(g, count, L, D, nullptr).bytes;
}

// what a long description with a clearance next to its terms (either may be missing, not both) must satisfy before anything is enqueued
__attribute__((visibility("hidden"))) int afm_long_scene_guide_check(const afm_long_guide* g, const afm_scene_clearance* clear, int32_t L, int32_t D) {
    if (!g || !g->terms || !long_geometry_ok(g, L)) return AFM_E_BADARG;
    const afm_motion_guide* terms = set_terms(g->terms);
    if (!terms && !clear) return AFM_E_BADARG;
    if (terms) {
        const int rc = afm_long_guide_check(g, L, D);
        if (rc != 0) return rc;
    }
    if (!clear) return 0;
    const int rc = clear_check(clear, L, D);
    if (rc != 0) return rc;
    if (g->stitch.windows > 1 && g->stitch.overlap > 0 && !g->stitch.weights) return AFM_E_BADARG;          // the crossfade reads the row
    if (terms && !terms_agree(terms, clear)) return AFM_E_BADARG;
    if (g->frames > 65535) return AFM_E_UNSUPPORTED;
    if (clear->h3d && (size_t)H3D_SCAN_ROWS * g->frames * 4 > (size_t)GUIDE_LDS_BYTES) return AFM_E_UNSUPPORTED;
    return 0;
}

// the workspace of `count` long motions of a checked description (clear == NULL: afm_long_guide_workspace_bytes exactly)
__attribute__((visibility("hidden"))) int64_t afm_long_scene_guide_workspace_bytes(const afm_long_guide* g, const afm_scene_clearance* clear, int32_t count,
                                                                                   int32_t L, int32_t D) {
    return long_plan(g, count, L, D, nullptr, clear).bytes;
}

// the long motions [start, start + count) of the description's batch; x, t and grad already point at window start * S, the energies at
// long motion `start`.  run_contact / run_targets / run_clear: the terms this call computes (clear == NULL: afm_long_guidance's launches)
__attribute__((visibility("hidden"))) int afm_long_scene_guidance_sub(const afm_long_guide* g, const afm_scene_clearance* clear, bool run_contact,
                                                                      bool run_targets, bool run_clear, int32_t start, const float* x, const int64_t* t,
                                                                      float* grad, float* energy_contact, float* energy_targets, float* energy_clear,
                                                                      int32_t count, int32_t L, int32_t D, void* workspace, int64_t workspace_bytes,
                                                                      void* stream) {
    const int rc = afm_long_scene_guide_check(g, clear, L, D);
    if (rc != 0) return rc;
    const afm_motion_guide* m = g->terms;
    run_contact = run_contact && m->contact;
    run_targets = run_targets && m->targets;
    run_clear = run_clear && clear;
    if (!x || (!grad && !energy_contact && !energy_targets && !energy_clear) || start < 0 || count < 0 || (energy_contact && !run_contact) ||
        (energy_targets && !run_targets) || (energy_clear && !run_clear) || (!run_contact && !run_targets && !run_clear)) return AFM_E_BADARG;
    const int S = g->stitch.windows, ov = g->stitch.overlap, F = g->frames;
    if ((int64_t)count * S > 65535) return AFM_E_UNSUPPORTED;
    if (count == 0) return 0;
    const LongPlan p = long_plan(g, count, L, D, (char*)workspace, clear);
    if (!workspace || workspace_bytes < p.bytes) return AFM_E_WORKSPACE;
    hipStream_t s = (hipStream_t)stream;
    const int rcj = afm_stitch_join(x, p.lng, count, S, ov, L, D, F, stream);
    if (rcj != 0) return rcj;
    const int64_t* tl = nullptr;
    if (t && grad) {
        hipLaunchKernelGGL(long_t_kernel, dim3((unsigned)((count + 255) / 256)), dim3(256), 0, s, t, p.tl, S, count);
        AFM_CHECK_LAUNCH();
        tl = p.tl;
    }
    const bool contact = run_contact && (grad || energy_contact);
    if (contact) {
        const afm_contact_guide* a = m->contact;
        const int wins = count * S;
        GuideDev d = {};
        d.q = a->q + (int64_t)start * S * a->N * 3; d.c = a->c + (int64_t)start * S * a->N * a->K; d.mean = a->mean; d.std = a->std; d.scale = a->scale + start;
        for (int k = 0; k < a->K; ++k) d.cols[k] = a->cols[k];
        d.K = a->K; d.N = a->N; d.L = L; d.D = D; d.nblk = (int)guide_nblk(a->N, a->K);
        d.two_s2 = (float)(2.0 * a->sigma * a->sigma);
        d.coef = (float)(2.0 / ((double)a->N * a->K * a->sigma * a->sigma));
        d.t_start = a->t_start;
        const LongGeo lg = {S, ov, F};
        char* wp = p.cws;
        const int64_t nk = (int64_t)wins * a->N * a->K;
        int* fstar = (int*)wp; wp += afm_loop::align256(nk * 4);
        float* w = (float*)wp; wp += afm_loop::align256(nk * 4);
        float* partial = (float*)wp;
        const size_t lds = ((size_t)a->K * L * 3 + L) * 4;
        const dim3 g1((unsigned)d.nblk, (unsigned)wins), g2(grad ? (unsigned)F : 1u, (unsigned)count);
        if (a->h3d) {
            wp = p.cws + afm_loop::align256(afm_contact_guidance_workspace_bytes(wins, a->N, a->K));
            const H3dPlan h = h3d_plan(a->mean, a->std, d.scale, *a->h3d, a->K, F, D, start, count, true, d.coef, a->t_start, wp);
            hipLaunchKernelGGL(h3d_recover_kernel, dim3((unsigned)count), dim3(256), h.scan_lds, s, h.rec, p.lng, (const uint8_t*)nullptr, h.pos,
                               grad ? h.cs : nullptr);
            AFM_CHECK_LAUNCH();
            hipLaunchKernelGGL(long_nearest_h3d_kernel, g1, dim3(256), lds, s, d, lg, h.pos, fstar, w, partial);
            AFM_CHECK_LAUNCH();
            hipLaunchKernelGGL(long_sums_h3d_kernel, g2, dim3(256), 0, s, d, lg, h.pos, fstar, w, partial, grad ? h.S : nullptr, energy_contact);
            AFM_CHECK_LAUNCH();
            if (grad) {
                hipLaunchKernelGGL(h3d_adjoint_kernel, dim3((unsigned)count), dim3(256), h.scan_lds, s, h.adj, p.lng, (const uint8_t*)nullptr, tl, h.cs, h.S,
                                   p.glong);
                AFM_CHECK_LAUNCH();
            }
        } else {
            hipLaunchKernelGGL(long_nearest_kernel, g1, dim3(256), lds, s, d, lg, p.lng, fstar, w, partial);
            AFM_CHECK_LAUNCH();
            hipLaunchKernelGGL(long_gather_kernel, g2, dim3(256), 0, s, d, lg, p.lng, tl, fstar, w, partial, grad ? p.glong : nullptr, energy_contact);
            AFM_CHECK_LAUNCH();
        }
    }
    const bool targets = run_targets && (grad || energy_targets);
    if (targets) {
        const int rct = targets_sub(m->targets, contact && grad, start, p.lng, nullptr, tl, grad ? p.glong : nullptr, energy_targets, count, F, D, p.tws, s);
        if (rct != 0) return rct;
    }
    if (run_clear && (grad || energy_clear)) {
        const int rcl = long_clear_sub(clear, g->stitch, F, (contact || targets) && grad, start, p.lng, tl, grad ? p.glong : nullptr, energy_clear, count, L,
                                       D, p.lws, s);
        if (rcl != 0) return rcl;
    }
    if (!grad) return 0;
    return afm_stitch_windows(p.glong, grad, count, S, ov, L, D, F, stream);
}

__attribute__((visibility("hidden"))) int afm_long_guidance_sub(const afm_long_guide* g, bool run_contact, bool run_targets, int32_t start, const float* x,
                                                                const int64_t* t, float* grad, float* energy_contact, float* energy_targets,
                                                                int32_t count, int32_t L, int32_t D, void* workspace, int64_t workspace_bytes,
                                                                void* stream) {
    const int rc = afm_long_guide_check(g, L, D);
    if (rc != 0) return rc;
    return afm_long_scene_guidance_sub(g, nullptr, run_contact, run_targets, false, start, x, t, grad, energy_contact, energy_targets, nullptr, count, L, D,
                                       workspace, workspace_bytes, stream);
}

extern "C" int64_t afm_long_guidance_workspace_bytes(const afm_long_guide* g, int32_t B, int32_t L, int32_t D) {
    if (B < 0 || afm_long_guide_check(g, L, D) != 0 || B % g->stitch.windows != 0) return AFM_E_BADARG;
    return afm_long_guide_workspace_bytes(g, B / g->stitch.windows, L, D) + 256;
}

extern "C" int afm_long_guidance(const afm_long_guide* g, const float* x_windows, const int64_t* t, float* grad_windows, float* energy_contact,
                                 float* energy_targets, int32_t B, int32_t L, int32_t D, void* workspace, int64_t workspace_bytes, void* stream) {
    const int rc = afm_long_guide_check(g, L, D);
    if (rc != 0) return rc;
    if (B < 0 || B % g->stitch.windows != 0) return AFM_E_BADARG;
    return afm_long_guidance_sub(g, true, true, 0, x_windows, t, grad_windows, energy_contact, energy_targets, B / g->stitch.windows, L, D, workspace,
                                 workspace_bytes, stream);
}

extern "C" int64_t afm_long_scene_guidance_workspace_bytes(const afm_long_scene_guide* g, int32_t B, int32_t L, int32_t D) {
    if (!g || B < 0 || afm_long_scene_guide_check(g->base, g->clearance, L, D) != 0 || B % g->base->stitch.windows != 0) return AFM_E_BADARG;
    return afm_long_scene_guide_workspace_bytes(g->base, g->clearance, B / g->base->stitch.windows, L, D) + 256;
}

extern "C" int afm_long_scene_guidance(const afm_long_scene_guide* g, const float* x_windows, const int64_t* t, float* grad_windows,
                                       float* energy_contact, float* energy_targets, float* energy_clearance, int32_t B, int32_t L, int32_t D,
                                       void* workspace, int64_t workspace_bytes, void* stream) {
    if (!g) return AFM_E_BADARG;
    const int rc = afm_long_scene_guide_check(g->base, g->clearance, L, D);
    if (rc != 0) return rc;
    if (B < 0 || B % g->base->stitch.windows != 0) return AFM_E_BADARG;
    return afm_long_scene_guidance_sub(g->base, g->clearance, true, true, true, 0, x_windows, t, grad_windows, energy_contact, energy_targets,
                                       energy_clearance, B / g->base->stitch.windows, L, D, workspace, workspace_bytes, stream);
}
