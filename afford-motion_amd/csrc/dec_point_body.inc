// Body of dec_point_kernel / dec_point_imputing_kernel / dec_point_dpm_kernel (perceiver_points.hip), included into each with the kernel's
// arguments and IMPUTE, known, mask, x0_out, DPM, x0_prev, x0_keep in scope (template parameters NKS, NPROD, DDIM).  IMPUTE and DPM are
// compile-time constants in the first two kernels; in the 2M kernel IMPUTE is the uniform run-time `mask != NULL`.
    using RL = RowLess<NKS>;
    constexpr int K = RL::K, NT = RL::NT, LDQ = RL::LDQ, XS = RL::XS, NSTEP = RL::NSTEP, NW = RL::NW, NTH = 64 * NW, QEW = 16 * NT;
    extern __shared__ __attribute__((aligned(16))) float dp_sm[];
    // linear1 runs on the bf16 pipe with the exact three-way split (csrc/bf16split.h): the f32 MFMA issues at the vector rate and does not
    // overlap with the VALU work of the GELUs (122 us with all products in f32: VALU + f32 MFMA cycles add up), v_mfma_f32_16x16x32_bf16 does.
    // Operand order of its K = 32 steps: lane group g carries k = {a[4 g .. 4 g + 3], x[ks = 0 .. 3]} in step 0 and x[ks = 4 .. 11] in step 1 (x[ks] =
    // input 4 ks + g, zeros past NKS), i.e. what lane (p, g) already holds.
    uint4* TWP = reinterpret_cast<uint4*>(dp_sm);                 // [16 tiles][NSTEP][3 planes][64 lanes] 8 bf16: TWc rows in that order, split once per workgroup
    float* Qs = dp_sm + 16 * NSTEP * 3 * 64 * 4;                  // [QCOL][LDQ] quadratic form of the MLP's LayerNorm, operand order (lat_dectables_kernel)
    float* EGs = Qs + RL::QTAB;                                   // [K][16]    scores: row k = input, column jh
    float* gcs = EGs + K * 16;                                    // [16]       beta_q . G[jh] + cb[jh]
    float* WPs = gcs + 16;                                        // [8][16]    contact_layer.w . P
    float* W2s = WPs + 8 * 16;                                    // [8][LDW]   contact_layer.w fc2.w  (rows >= cd: 0)
    float* Cv = W2s + 8 * DP_LDW;                                 // [256]      b1 + W1 beta_mlp
    float* QDs = Cv + 256;                                        // [K][16 NT] quadratic form of the query's LayerNorm, operand order (host)
    float* QEs = QDs + K * 16 * NT;                               // [8][16 NT] contact_layer.w . G_dec^T  (columns >= feat_dim + 1: 0)
    float* c0s = QEs + 8 * QEW;                                   // [16]
    const int b = blockIdx.y, wave = threadIdx.x >> 6, lane = threadIdx.x & 63, p16 = lane & 15, g = lane >> 4;
    float* aT = c0s + 16 + wave * 16 * 17;                        // [16 points][17] attention weights of the tile, transposed
    float* tr = c0s + 16 + NW * 16 * 17 + wave * 16;              // [16] a per-point scalar from lanes (p, .) to lanes (., g)
    for (int it = threadIdx.x; it < 16 * NSTEP * 64; it += NTH) { // (channel tile, K32 step, lane) items: 8 operand values -> three planes
        const int l = it & 63, st = (it >> 6) % NSTEP, tt = it / (64 * NSTEP), n = 16 * tt + (l & 15), gg = l >> 4;
        float v[8];
#pragma unroll
        for (int e = 0; e < 8; ++e) {
            const int slot = 8 * st + e;                           // slots 0..3: attention weights 4 g + e; slot 4 + ks: input 4 ks + g
            v[e] = slot < 4 ? twp[((int64_t)b * 16 + 4 * gg + slot) * 256 + n] : (slot - 4 < NKS ? twx[(4 * (slot - 4) + gg) * 256 + n] : 0.f);
        }
        uint4 p1, p2, p3;
        split2(v[0], v[1], p1.x, p2.x, p3.x); split2(v[2], v[3], p1.y, p2.y, p3.y); split2(v[4], v[5], p1.z, p2.z, p3.z); split2(v[6], v[7], p1.w, p2.w, p3.w);
        uint4* d = TWP + ((tt * NSTEP + st) * 3) * 64 + l;
        d[0] = p1; d[64] = p2; d[128] = p3;
    }
    for (int i = threadIdx.x; i < RL::TAB; i += NTH) Qs[i] = qtab[(int64_t)b * RL::TAB + i];      // Qs | EGs | gcs | WPs are contiguous, like the table
    for (int i = threadIdx.x; i < 8 * 256; i += NTH) W2s[(i >> 8) * DP_LDW + (i & 255)] = (i >> 8) < cd ? w2f[i] : 0.f;
    for (int i = threadIdx.x; i < 256; i += NTH) Cv[i] = cvec[i];
    for (int i = threadIdx.x; i < K * 16 * NT; i += NTH) QDs[i] = qdd[i];
    for (int i = threadIdx.x; i < 8 * QEW; i += NTH) {
        const int j = i / QEW, k = i - j * QEW;
        QEs[i] = (j < cd && k < K) ? gen_qe[j * K + k] : 0.f;
    }
    if (threadIdx.x < 16) c0s[threadIdx.x] = (int)threadIdx.x < cd ? c0[threadIdx.x] : 0.f;
    __syncthreads();
    const float gconst = gcs[p16];

    const int per = (N + gridDim.x - 1) / gridDim.x;
    const int n0 = blockIdx.x * per, n1 = min(N, n0 + per);
    const int wper = ((per + NW - 1) / NW + 15) & ~15;            // points per wave, whole tiles
    const int w0 = n0 + wave * wper, w1 = min(n1, w0 + wper);

    float xin[NKS], xnext[NKS];
    auto fetch = [&](int nb, float (&dst)[NKS]) {                  // inputs k = 4 ks + g of point nb + p16
        const unsigned pti = (unsigned)(b * N + min(nb + p16, n1 - 1));
#pragma unroll
        for (int ks = 0; ks < NKS; ++ks) {
            const int k = 4 * ks + g;
            // one load per input, from the array that holds it (round 6: both arrays were read unconditionally and one value selected - twice the
            // requests and 34.5 MB of traffic per launch against 15.7 MB algorithmic, VERDICT r5 item 5; the lanes of a group take the same branch)
            float v = k == fd ? 1.0f : 0.0f;
            if (k < cd) v = xt[pti * (unsigned)cd + (unsigned)k];
            else if (k < fd) v = feat[pti * (unsigned)fd + (unsigned)k];
            dst[ks] = v;
        }
    };
    if (w0 < w1) fetch(w0, xnext);
    for (int nb = w0; nb < w1; nb += 16) {
        const int64_t pt = (int64_t)b * N + nb + p16;
        const bool pvalid = nb + p16 < w1;
#pragma unroll
        for (int ks = 0; ks < NKS; ++ks) xin[ks] = xnext[ks];
        if (nb + 16 < w1) fetch(nb + 16, xnext);
        // IMPUTE: what the tile's output site reads - mask bytes, known values, x_t and the noise of the lane's own elements - is requested here,
        // a tile's work ahead of its use, and without a branch: loaded at the site, a `known` under a test of its mask byte stood behind that
        // byte's round trip at the end of every tile (4.7 % of the kernel).  A lane without an output element reads element 0 and drops it;
        // `known` is read everywhere and selected, never blended.  (x_t here is the lane's own element, which only this lane writes, below.)
        // DPM (the 2M kernel): x_t and the previous step's final x0 of the lane's own elements are requested here as well - per element, a
        // sample's base b N cd is not 16-byte aligned in general - and the mask bytes / known values only where there is a mask.
        unsigned km[4] = {0u, 0u, 0u, 0u};
        float kn[4] = {0.f, 0.f, 0.f, 0.f}, xo[4] = {0.f, 0.f, 0.f, 0.f}, zo[4] = {0.f, 0.f, 0.f, 0.f}, hp[4] = {0.f, 0.f, 0.f, 0.f};
        if (IMPUTE || DPM) {
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int j = 4 * g + r;
                const int64_t i = (pvalid && j < cd) ? pt * cd + j : 0;
                if (IMPUTE) {
                    km[r] = mask[i];
                    kn[r] = known[i];
                }
                xo[r] = xt[i];
                if (!DPM && !(clip & AFM_UPD_NO_NOISE)) zo[r] = noise[i];
                if (DPM && x0_prev) hp[r] = x0_prev[i];
            }
        }
        // ---- LayerNorm statistics of the (never generated) query row: var_q = x Qd x^T; scores = rstd_q (x . EG) + const; softmax over the
        // two keys of a head (jh and jh ^ 8: eight lanes apart)
        f32x4 sc = {0.f, 0.f, 0.f, 0.f};
        float varq = 0.f;
#pragma unroll
        for (int ks = 0; ks < NKS; ++ks) sc = __builtin_amdgcn_mfma_f32_16x16x4f32(xin[ks], EGs[(4 * ks + g) * 16 + p16], sc, 0, 0, 0);       // lane (jh = p16, g) reg r: point 4 g + r
#pragma unroll
        for (int tt = 0; tt < NT; ++tt) {
            f32x4 yq = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
            for (int ks = 0; ks < NKS; ++ks) yq = __builtin_amdgcn_mfma_f32_16x16x4f32(QDs[(4 * ks + g) * (16 * NT) + 16 * tt + p16], xin[ks], yq, 0, 0, 0);       // reg r: input 4 (4 t + r) + g
#pragma unroll
            for (int r = 0; r < 4; ++r)
                if (4 * tt + r < NKS) varq += yq[r] * xin[4 * tt + r];
        }
        varq += xor16(varq); varq += xor32(varq);
        if (g == 0) tr[p16] = 1.0f / sqrtf(fmaxf(varq, 0.f) + 1e-5f);
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const float s_own = tr[4 * g + r] * sc[r] + gconst, s_oth = lane_xor<8>(s_own);
            const float mx = fmaxf(s_own, s_oth);
            const float e_own = __expf(s_own - mx), e_oth = __expf(s_oth - mx);
            aT[(4 * g + r) * 17 + p16] = e_own / (e_own + e_oth);
        }
        float aB[4];
#pragma unroll
        for (int sI = 0; sI < 4; ++sI) aB[sI] = aT[p16 * 17 + 4 * g + sI];       // lane (p = p16, g): a[p, jh = 4 g + s]
        // ---- variance of the MLP's LayerNorm input: u Qc u^T (y = Qc u on the matrix pipe, the dot with u in the lane + across g)
        float var = 0.f;
#pragma unroll
        for (int tt = 0; tt < 1 + NT; ++tt) {                      // output tile 0: attention weights; 1 + t: inputs 4 (4 t + r) + g
            f32x4 y = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
            for (int sI = 0; sI < 4; ++sI) y = __builtin_amdgcn_mfma_f32_16x16x4f32(Qs[(4 * g + sI) * LDQ + 16 * tt + p16], aB[sI], y, 0, 0, 0);
#pragma unroll
            for (int ks = 0; ks < NKS; ++ks) y = __builtin_amdgcn_mfma_f32_16x16x4f32(Qs[(16 + XS * g + ks) * LDQ + 16 * tt + p16], xin[ks], y, 0, 0, 0);
            if (tt == 0) var += (y[0] * aB[0] + y[1] * aB[1]) + (y[2] * aB[2] + y[3] * aB[3]);
            else {
#pragma unroll
                for (int r = 0; r < 4; ++r)
                    if (4 * (tt - 1) + r < NKS) var += y[r] * xin[4 * (tt - 1) + r];
            }
        }
        var += xor16(var); var += xor32(var);
        const float rstd2 = 1.0f / sqrtf(fmaxf(var, 0.f) + 1e-5f);
        // ---- linear1 (K = 16 + 4 NKS) -> GELU -> row-dots with w2; then the attention and query parts of contact_layer.w . h1.
        // TG 16-channel tiles at a time, phase by phase (operand reads, interleaved MFMA chains, independent GELUs, separate row-dot accumulators):
        // tile by tile the wave would sit through an LDS round trip, a dependent MFMA chain and a GELU dependency chain per tile.
        uint4 ub[NSTEP][3];                                        // u = [a | x] of this lane's point, three bf16 planes in linear1's operand order
        {
            float v[8 * NSTEP];
#pragma unroll
            for (int e = 0; e < 8 * NSTEP; ++e) v[e] = e < 4 ? aB[e] : (e - 4 < NKS ? xin[e - 4 < NKS ? e - 4 : 0] : 0.f);
#pragma unroll
            for (int st = 0; st < NSTEP; ++st) {
                split2(v[8 * st + 0], v[8 * st + 1], ub[st][0].x, ub[st][1].x, ub[st][2].x); split2(v[8 * st + 2], v[8 * st + 3], ub[st][0].y, ub[st][1].y, ub[st][2].y);
                split2(v[8 * st + 4], v[8 * st + 5], ub[st][0].z, ub[st][1].z, ub[st][2].z); split2(v[8 * st + 6], v[8 * st + 7], ub[st][0].w, ub[st][1].w, ub[st][2].w);
            }
        }
        constexpr int TG = NSTEP == 1 ? 4 : 2;                     // channel tiles in flight (registers: TG x NSTEP x 3 operand vectors)
        f32x4 sa[4];
#pragma unroll
        for (int q = 0; q < 4; ++q) sa[q] = f32x4{0.f, 0.f, 0.f, 0.f};
        for (int t4 = 0; t4 < 16; t4 += TG) {
            uint4 wp[TG][NSTEP][3];
            float4 cv[TG], w4[TG];
#pragma unroll
            for (int q = 0; q < TG; ++q) {
                const int tt = t4 + q;
#pragma unroll
                for (int st = 0; st < NSTEP; ++st)
#pragma unroll
                    for (int pl = 0; pl < 3; ++pl) wp[q][st][pl] = TWP[((tt * NSTEP + st) * 3 + pl) * 64 + lane];
                cv[q] = *reinterpret_cast<const float4*>(Cv + 16 * tt + 4 * g);
                w4[q] = p16 < 8 ? *reinterpret_cast<const float4*>(W2s + p16 * DP_LDW + 16 * tt + 4 * g) : make_float4(0.f, 0.f, 0.f, 0.f);
            }
            __builtin_amdgcn_sched_barrier(0);
            f32x4 acc[TG];
#pragma unroll
            for (int q = 0; q < TG; ++q) acc[q] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
            for (int st = 0; st < NSTEP; ++st)
#pragma unroll
                for (int pq = 9 - NPROD; pq < 9; ++pq)
#pragma unroll
                    for (int q = 0; q < TG; ++q)
                        acc[q] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(__builtin_bit_cast(bf16x8, wp[q][st][AFM_PA[pq]]), __builtin_bit_cast(bf16x8, ub[st][AFM_PB[pq]]), acc[q], 0, 0, 0);
            __builtin_amdgcn_sched_barrier(0);
            float hid[TG][4];
#pragma unroll
            for (int q = 0; q < TG; ++q) {
                hid[q][0] = gelu_erf_fast(rstd2 * acc[q][0] + cv[q].x); hid[q][1] = gelu_erf_fast(rstd2 * acc[q][1] + cv[q].y);
                hid[q][2] = gelu_erf_fast(rstd2 * acc[q][2] + cv[q].z); hid[q][3] = gelu_erf_fast(rstd2 * acc[q][3] + cv[q].w);
            }
            __builtin_amdgcn_sched_barrier(0);
#pragma unroll
            for (int q = 0; q < TG; ++q) sa[q & 3] = __builtin_amdgcn_mfma_f32_16x16x4f32(w4[q].x, hid[q][0], sa[q & 3], 0, 0, 0);
#pragma unroll
            for (int q = 0; q < TG; ++q) sa[(q + 2) & 3] = __builtin_amdgcn_mfma_f32_16x16x4f32(w4[q].y, hid[q][1], sa[(q + 2) & 3], 0, 0, 0);
#pragma unroll
            for (int q = 0; q < TG; ++q) sa[q & 3] = __builtin_amdgcn_mfma_f32_16x16x4f32(w4[q].z, hid[q][2], sa[q & 3], 0, 0, 0);
#pragma unroll
            for (int q = 0; q < TG; ++q) sa[(q + 2) & 3] = __builtin_amdgcn_mfma_f32_16x16x4f32(w4[q].w, hid[q][3], sa[(q + 2) & 3], 0, 0, 0);
        }
#pragma unroll
        for (int sI = 0; sI < 4; ++sI) sa[sI & 1] = __builtin_amdgcn_mfma_f32_16x16x4f32(p16 < 8 ? WPs[p16 * 16 + 4 * g + sI] : 0.f, aB[sI], sa[sI & 1], 0, 0, 0);
#pragma unroll
        for (int ks = 0; ks < NKS; ++ks) sa[2 + (ks & 1)] = __builtin_amdgcn_mfma_f32_16x16x4f32(p16 < 8 ? QEs[p16 * QEW + 4 * ks + g] : 0.f, xin[ks], sa[2 + (ks & 1)], 0, 0, 0);
        const f32x4 sat = (sa[0] + sa[1]) + (sa[2] + sa[3]);
        if (pvalid) {                                              // lane (point p16, g): contact channels 4 g + r
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int j = 4 * g + r;
                if (j < cd) {
                    const int64_t i = pt * cd + j;
                    float v = sat[r] + c0s[j];
                    if (IMPUTE) v = km[r] ? kn[r] : v;                                           // the select of afm_impute
                    if (clip & AFM_UPD_CLIP) v = v < -1.0f ? -1.0f : (v > 1.0f ? 1.0f : v);      // clip_denoised
                    if (x0_out) x0_out[i] = v;
                    if (DPM) {                       // v is the final x0 of the step: the update, and the next step's history (this lane read hp[r] above)
                        const float4 rr = reinterpret_cast<const float4*>(c1)[b];
                        x_next[i] = x0_prev ? dpm_update(v, xo[r], rr, hp[r]) : dpm_update(v, xo[r], rr);
                        x0_keep[i] = v;
                    } else if (DDIM && IMPUTE) {
                        const float4 rr = reinterpret_cast<const float4*>(c1)[b];
                        x_next[i] = (clip & AFM_UPD_NO_NOISE) ? ddim_update(v, xo[r], rr) : ddim_update(v, xo[r], rr, sigma[b], zo[r]);
                    } else if (DDIM) {
                        if (x_next) {
                            const float4 r = reinterpret_cast<const float4*>(c1)[b];
                            x_next[i] = (clip & AFM_UPD_NO_NOISE) ? ddim_update(v, xt[i], r) : ddim_update(v, xt[i], r, sigma[b], noise[i]);
                        }
                    } else if (IMPUTE) x_next[i] = ddpm_update(v, xo[r], c1[b], c2[b], sigma[b], zo[r]);
                    else if (x_next) x_next[i] = (c1[b] * v + c2[b] * xt[i]) + sigma[b] * noise[i];
                }
            }
        }
    }
