// The tile program of one workgroup of gemm_f32_split_bf16 (csrc/gemm_split.hip), as TEXT: included once per kernel that runs it, so that the
// one-tile-per-workgroup kernel stays instruction for instruction what rounds 2-4 tuned while the walking kernels (round 5) run the very same
// program per tile.  Expects in scope: template parameters BM, BN, BKS, NPROD, KG, RING, GSEG; `const afm_linear_args& p`, `int nbm, nbn`;
// macros AFM_WG (the tile's linear index in its launch), AFM_TIDX (threadIdx.x, or an opaque per-tile copy of it) and AFM_TIMELINE_SLOT;
// optionally AFM_BODY_WM = waves along M of one K group (default 2: a 256-thread group of 2 x 2 waves; 4: the 512-thread 256 x 128 tile of round 6)
// and AFM_BODY_STREAMED = a constant expression, true where the tile runs the streamed epilogue (gemm_epilogue.h: the 512-thread 128 x 128 tile).
    static_assert(BKS == 16, "one K16 MFMA step per K-tile");
    static_assert(RING == 2 || RING == 3, "two or three LDS stages");
    static_assert(GSEG == 1 || (GSEG == 2 && KG > 1), "two segments per group: split-K forms only");
    // the RING == 3 K loop is unrolled four K-tiles deep: a split-K group's K-tile count is a compile-time fact, the sequential form's
    // (KG == 1, tile code 9: measurement only) is checked by its launcher (K % 64 == 0).  AFM_ABLATE applies to the RING == 2 loop only.
    static_assert(RING != 3 || KG == 1 || (GSEG * 256 / BKS) % 4 == 0, "three-stage K loop: K-tiles per group must be a multiple of four");
#ifdef AFM_BODY_WM
    constexpr int WMv = AFM_BODY_WM;
#else
    constexpr int WMv = 2;
#endif
#ifdef AFM_BODY_STREAMED
    constexpr bool STREAMED = AFM_BODY_STREAMED;
#else
    constexpr bool STREAMED = false;
#endif
    constexpr int GT = WMv * 2 * 64;                  // threads of one K group: WMv x 2 waves, each a (BM / WMv) x (BN / 2) wave tile
    static_assert(WMv == 2 || KG == 1, "groups of more than 256 threads: one K group only");
    constexpr int TM = BM / (WMv * 32), TN = BN / 64;
    static_assert(KG == 1 || (BM == 64 && BN == 64), "the split-K form exists for 64x64 tiles");
    constexpr int ROWB = BKS * 2 + 16;                // LDS row bytes (bf16 + pad)
    constexpr int ROWS = BM + BN;                     // A rows then W rows
    constexpr int PLANE = ROWS * ROWB;
    constexpr int STAGE = 3 * PLANE;
    constexpr int NA = BM * 4 / GT, NW = BN * 4 / GT;   // (row, 4 consecutive k) items of A / of W per thread and K-tile
    constexpr int NI = NA + NW;
    constexpr int LDC = BN + 4;
    extern __shared__ __attribute__((aligned(16))) unsigned char lds_raw[];
    const int grp = KG > 1 ? __builtin_amdgcn_readfirstlane((int)(AFM_TIDX >> 8)) : 0;      // K segment of this 256-thread group
    unsigned char* lds = lds_raw + grp * (RING * STAGE);
#if defined(AFM_TIMELINE) && defined(AFM_DESYNC_TICKS)
    // experiment (tools/gemm_timeline builds only): half of the workgroups of a CU start AFM_DESYNC_TICKS x 10 ns late, so that the prologue /
    // epilogue phases of one half meet the K loops of the other - what a desynchronised (persistent, stream-K like) schedule would buy
    if ((AFM_WG >> 8) & 1) {
        const unsigned long long td = __builtin_amdgcn_s_memrealtime();
        while (__builtin_amdgcn_s_memrealtime() - td < AFM_DESYNC_TICKS) __builtin_amdgcn_s_sleep(20);
    }
#endif
#ifdef AFM_TIMELINE          // tools/gemm_timeline.hip only (single translation unit with gemm.hip, which defines the record type)
    const unsigned long long tl_t0 = __builtin_amdgcn_s_memrealtime(), tl_c0 = afm_cycles();
#endif

    const int nblk = nbm * nbn;
    int bid = AFM_WG;
    {
        const int xcd = bid & 7, idx = bid >> 3, q = nblk >> 3, r = nblk & 7;
        bid = (xcd < r ? xcd * (q + 1) : r * (q + 1) + (xcd - r) * q) + idx;
    }
    const int bm = bid / nbn, bn = bid % nbn;
    const int tid = AFM_TIDX & (GT - 1), lane = tid & 63, wave = tid >> 6;      // position inside the K group
    const int wm = wave >> 1, wn = wave & 1;
    const int r32 = lane & 31, hh = lane >> 5;

    // Staging items are (row, quarter) = 4 floats: the four lanes of a row fetch its 64 contiguous bytes of the K-tile with ONE
    // load instruction (16 cache lines per wave-instruction; an 8-float item needs two instructions of 32 lines each:
    // TCP_TOTAL_CACHE_ACCESSES 11.7 M -> 6.0 M per out_proj launch, 2-3 % faster), and every thread carries the same mix of A and W
    // work.  16 consecutive lanes (the unit ds_write_b64 is serviced in) take the four quarters of four rows of equal parity inside a
    // block of 8 rows: with rows 48 B apart those are four disjoint 32-byte windows of the 128-byte bank row.
    // (The 512-thread 128 x 128 tile - one A and one W item per thread, it = tid for both - maps a 16-lane group exactly as the 256-thread
    // tiles do, so the same row permutation stays conflict-free.)
    // SOFF (the 512-thread 128 x 128 tile, tile code 14): the items are addressed as 32-bit byte offsets from the uniform bases p.A / p.W
    // (saddr + voffset loads) instead of 64-bit pointers - two VGPRs less, what it takes to fit four waves per SIMD without spilling a
    // register set in the K loop.  Its launcher checks that every offset fits.  Its K loop also keeps ONE register set instead of two: an
    // item's next tile (kt + 2) is requested as soon as the item's split of tile kt + 1 is done (A after the sixth MFMA, W after the twelfth),
    // about half a K-tile of lead instead of one - the other waves of the SIMD (four per SIMD) cover the rest.  Eight VGPRs: with both sets
    // hipcc parks one set in scratch behind a vmcnt(0) wait per load.
    constexpr bool SOFF = GT == 512 && BM == 128;
    const RowMap amap{p.a_grp, p.a_stride, p.a_off, p.a_skip_after, p.a_skip};
    const float* src[NI];
    uint32_t soff[NI];
    int dst[NI];
#pragma unroll
    for (int i = 0; i < NI; ++i) {
        const int it = tid + GT * (i < NA ? i : i - NA), q = it & 3, v = it >> 2, row = (v & ~7) + ((v & 3) << 1) + ((v >> 2) & 1);
        const int64_t eoff = (i < NA ? amap(min(bm * BM + row, p.M - 1)) * p.lda : (int64_t)min(bn * BN + row, p.N - 1) * p.ldw) + q * 4 + grp * (GSEG * KSEG);
        src[i] = (i < NA ? p.A : p.W) + eoff;
        soff[i] = (uint32_t)eoff * 4u;
        dst[i] = ((i < NA ? 0 : BM) + row) * ROWB + q * 8;
    }

    f32x16 acc[TM][TN];
#pragma unroll
    for (int i = 0; i < TM; ++i)
#pragma unroll
        for (int j = 0; j < TN; ++j)
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[i][j][r] = 0.f;

    // Two register sets, always indexed with compile-time constants: at the top of K-tile kt the set (kt & 1) is free (its
    // tile went to LDS during kt - 1) and receives tile kt + 2; the other set holds tile kt + 1 (loaded one full K-tile
    // ago) and is split into the other LDS stage between the MFMAs of tile kt.
    // RING == 3 keeps NSET = 4 register sets: tile j lives in set j % 4 and is requested THREE K-tiles before its split (round 5: with one
    // K-tile of lead - ~950 cycles on a small launch - the split waited for operands that the previous kernel had just written on other
    // XCDs, an HBM / Infinity-Cache round trip of the same length; removing all split arithmetic moved a small launch by 0.3 us, removing one
    // operand's loads by 1.2: profiles/r04_gemm_w_ablation.txt).  A small launch holds two waves per SIMD: the registers are there.
    constexpr int NSET = RING == 3 ? 4 : 2;
    f32x4 g[NSET][NI];
    const int nk = KG > 1 ? GSEG * KSEG / BKS : p.K / BKS;
    constexpr int SEGT = KSEG / BKS;                  // K-tiles per segment
    f32x16 tot[TM][TN];                               // sum of the finished segments (KG == 1 with K > KSEG only)
    bool have_tot = false;
    auto load_item = [&](auto SETC, int i, int kt) {  // (SOFF: one item of one register set)
        constexpr int S = decltype(SETC)::value;
        const int k = min(kt, nk - 1) * BKS;
        g[S][i] = *reinterpret_cast<const f32x4*>(reinterpret_cast<const unsigned char*>(i < NA ? p.A : p.W) + (soff[i] + (uint32_t)k * 4u));
    };
    auto load = [&](auto SETC, int kt) {
        constexpr int S = decltype(SETC)::value;
        const int k = min(kt, nk - 1) * BKS;          // past the end: re-load the last tile (never consumed)
        if ((AFM_ABLATE & 1) && kt >= 2) {
#pragma unroll
            for (int i = 0; i < NI; ++i) asm volatile("" : "+v"(g[S][i]));
            return;
        }
#pragma unroll
        for (int i = 0; i < NI; ++i) {
            if ((AFM_ABLATE & 32) && i >= NA && kt >= 2) { asm volatile("" : "+v"(g[S][i])); continue; }
            if ((AFM_ABLATE & 64) && i < NA && kt >= 2) { asm volatile("" : "+v"(g[S][i])); continue; }
            if constexpr (SOFF) g[S][i] = *reinterpret_cast<const f32x4*>(reinterpret_cast<const unsigned char*>(i < NA ? p.A : p.W) + (soff[i] + (uint32_t)k * 4u));
            else g[S][i] = *reinterpret_cast<const f32x4*>(src[i] + k);
        }
    };
    using Set0 = std::integral_constant<int, 0>;
    using Set1 = std::integral_constant<int, 1>;
    load(Set0{}, 0);
    load(Set1{}, 1);
    // folded LayerNorm: row statistics, an LDS region of their own - behind the operand stages AND behind the staged accumulators (which only the
    // 256 x 128 tile lets outgrow the stages)
    constexpr int ROWST_OFF = KG * RING * STAGE > BM * LDC * 4 ? KG * RING * STAGE : BM * LDC * 4;
    float* rowst = reinterpret_cast<float*>(lds_raw + ROWST_OFF);
    gemm_rowstats<BM>(p, rowst, bm);                  // (loads in flight with the operands'; published by the barrier below)
    auto split_set = [&](auto SETC, int stage) {      // prologue only: a whole register set -> one LDS stage, no interleaving
        constexpr int S = decltype(SETC)::value;
#pragma unroll
        for (int i = 0; i < NI; ++i) {
            unsigned char* d = lds + stage * STAGE + dst[i];
            uint32_t a1, a2, a3, b1, b2, b3;
            split2(g[S][i][0], g[S][i][1], a1, a2, a3);
            split2(g[S][i][2], g[S][i][3], b1, b2, b3);
            *reinterpret_cast<u32x2*>(d) = u32x2{a1, b1};
            *reinterpret_cast<u32x2*>(d + PLANE) = u32x2{a2, b2};
            *reinterpret_cast<u32x2*>(d + 2 * PLANE) = u32x2{a3, b3};
        }
    };
    using Set2 = std::integral_constant<int, 2>;
    using Set3 = std::integral_constant<int, 3>;
    if constexpr (RING == 3) {                        // tiles 0 .. 4 requested, tiles 0 and 1 in LDS (K-tile 0 splits set 2 and refills set 1 with tile 5)
        load(Set2{}, 2);
        load(Set3{}, 3);
        split_set(Set0{}, 0);
        load(Set0{}, 4);
        split_set(Set1{}, 1);
    } else {
        split_set(Set0{}, 0);
        if constexpr (SOFF) {                         // the K loop's single register set holds tile 1 (set 1 is dead from here on)
#pragma unroll
            for (int i = 0; i < NI; ++i) g[0][i] = g[1][i];
        }
    }
    __syncthreads();
#ifdef AFM_TIMELINE
    const unsigned long long tl_pro = __builtin_amdgcn_s_memrealtime();          // prologue done: first K-tile split and published
#endif

    const int a_off = (wm * (BM / WMv) + r32) * ROWB + hh * 16;
    const int w_off = (BM + wn * (BN / 2) + r32) * ROWB + hh * 16;
    constexpr int NMFMA = NPROD * TM * TN;                    // MFMAs per wave per K-tile
    constexpr int NPIECE = NI * 2 * 3;                        // split pieces per thread per K-tile (pair of floats x residual level)

    // One K-tile.  The instruction order is written out and pinned with sched_barrier fences (hipcc otherwise hoists all
    // MFMAs in front of the split and chains the nine MFMAs of one accumulator back to back): after every MFMA a piece of
    // the next tile's split (~5 VALU) issues in the shadow of the 32-cycle matrix op.
    uint4 af[TM][3], bf[TN][3];
    auto body = [&](auto CURC, int kt) {          // K-tile kt with kt & 1 == cur: register set cur is free, set cur ^ 1 holds tile kt + 1
        constexpr int cur = decltype(CURC)::value;
        constexpr int RS = SOFF ? 0 : cur ^ 1;        // register set holding tile kt + 1
        if constexpr (!SOFF) load(CURC, kt + 2);
        const unsigned char* base = lds + cur * STAGE;
        unsigned char* wbase = lds + (cur ^ 1) * STAGE;
        float r0[NI * 2], r1[NI * 2];
        uint32_t sp[NI * 2][3];
        int piece = 0, m = 0;
        auto do_piece = [&](int t) {
            const int u = t / 3, lvl = t % 3, i = u / 2, c = u % 2;
            if ((AFM_ABLATE & 32) && i >= NA && kt >= 1) return;          // W items: nothing to split, nothing to store
            if ((AFM_ABLATE & 64) && i < NA && kt >= 1) return;           // A items likewise (the floor of "A already in LDS": out_proj fused behind attention)
            if (lvl == 0) {
                r0[u] = g[RS][i][2 * c];
                r1[u] = g[RS][i][2 * c + 1];
            }
            const uint32_t pk = (AFM_ABLATE & 2) ? __float_as_uint(lvl == 1 ? r1[u] : r0[u]) : cvt_pk_bf16(r0[u], r1[u]);
            sp[u][lvl] = pk;
            if (lvl < 2) {
                if (!(AFM_ABLATE & 2)) {
                    r0[u] = sub_bf16_lo(r0[u], pk);              // (one v_dot2c_f32_bf16 each: bf16split.h)
                    r1[u] = sub_bf16_hi(r1[u], pk);
                }
            } else if (c == 1) {
                unsigned char* d = wbase + dst[i];
                if (AFM_ABLATE & 4) {
#pragma unroll
                    for (int pl = 0; pl < 3; ++pl) asm volatile("" :: "v"(sp[2 * i][pl]), "v"(sp[2 * i + 1][pl]), "v"(d));
                } else {
#pragma unroll
                    for (int pl = 0; pl < 3; ++pl) *reinterpret_cast<u32x2*>(d + pl * PLANE) = u32x2{sp[2 * i][pl], sp[2 * i + 1][pl]};
                }
            }
        };
        if (!(AFM_ABLATE & 8) || kt == 0)
#pragma unroll
        for (int pl = 0; pl < 3; ++pl) {
#pragma unroll
            for (int i = 0; i < TM; ++i) af[i][pl] = *reinterpret_cast<const uint4*>(base + pl * PLANE + a_off + i * 32 * ROWB);
#pragma unroll
            for (int j = 0; j < TN; ++j) bf[j][pl] = *reinterpret_cast<const uint4*>(base + pl * PLANE + w_off + j * 32 * ROWB);
        }
        __builtin_amdgcn_sched_barrier(0);
#pragma unroll
        for (int q = 9 - NPROD; q < 9; ++q)
#pragma unroll
            for (int tm = 0; tm < TM; ++tm)
#pragma unroll
                for (int tn = 0; tn < TN; ++tn) {
                    if (AFM_ABLATE & 16) asm volatile("" : "+v"(acc[tm][tn][q]) : "v"(af[tm][AFM_PA[q]].x), "v"(af[tm][AFM_PA[q]].w), "v"(bf[tn][AFM_PB[q]].x), "v"(bf[tn][AFM_PB[q]].w));
                    else acc[tm][tn] = mfma_bf16(af[tm][AFM_PA[q]], bf[tn][AFM_PB[q]], acc[tm][tn]);
                    ++m;
#pragma unroll
                    for (int t = 0; t < NPIECE; ++t)
                        if (t >= piece && t < (m * NPIECE) / NMFMA) do_piece(t);
                    if constexpr (SOFF) {             // an item whose split just finished: request its tile kt + 2 into the same registers
#pragma unroll
                        for (int i = 0; i < NI; ++i)
                            if (piece < (i + 1) * 6 && (m * NPIECE) / NMFMA >= (i + 1) * 6) load_item(Set0{}, i, kt + 2);
                    }
                    piece = (m * NPIECE) / NMFMA;
                    __builtin_amdgcn_sched_barrier(0);
                }
        if ((KG == 1 || GSEG > 1) && ((kt + 1) % SEGT) == 0 && kt + 1 < nk) {        // segment finished, more to come: bank it, restart from zero
#pragma unroll
            for (int tm = 0; tm < TM; ++tm)
#pragma unroll
                for (int tn = 0; tn < TN; ++tn)
#pragma unroll
                    for (int r = 0; r < 16; ++r) {
                        tot[tm][tn][r] = have_tot ? tot[tm][tn][r] + acc[tm][tn][r] : acc[tm][tn][r];
                        acc[tm][tn][r] = 0.f;
                    }
            have_tot = true;
        }
        __syncthreads();
    };
    // RING == 3: K-tile kt runs its MFMAs on fragment set kt & 1 (read during kt - 1), requests tile kt + 1's fragments from stage
    // (kt + 1) % 3 (written during kt - 1, published by that K-tile's barrier) into the other set, and splits tile kt + 2 (register set
    // kt & 1, loaded during kt - 1) into stage (kt + 2) % 3, whose previous tile (kt - 1) was last read during kt - 2.
    u32x4 fa[2][TM][3], fb[2][TN][3];
    auto read_frag = [&](auto FC, int stage) {
        constexpr int F = decltype(FC)::value;
        const unsigned char* base = lds + stage * STAGE;
#pragma unroll
        for (int pl = 0; pl < 3; ++pl) {
#pragma unroll
            for (int i = 0; i < TM; ++i) fa[F][i][pl] = *reinterpret_cast<const u32x4*>(base + pl * PLANE + a_off + i * 32 * ROWB);
#pragma unroll
            for (int j = 0; j < TN; ++j) fb[F][j][pl] = *reinterpret_cast<const u32x4*>(base + pl * PLANE + w_off + j * 32 * ROWB);
        }
    };
#ifndef AFM_R3_TAIL
#define AFM_R3_TAIL 2         // MFMAs at the end of a K-tile that carry no split work: the last LDS stores land under them
#endif
    auto body3 = [&](auto SC, int kt, int st_next, int st_wr) {          // K-tile kt, S = kt % 4
        constexpr int S = decltype(SC)::value;
        constexpr int cur = S & 1;                    // fragment set of this K-tile
        constexpr int SS = (S + 2) & 3;               // register set that is split (tile kt + 2)
        using LoadSet = std::integral_constant<int, (S + 1) & 3>;       // ... and the one that is refilled (tile kt + 5)
        using FragNext = std::integral_constant<int, cur ^ 1>;
        unsigned char* wbase = lds + st_wr * STAGE;
        float r0[NI * 2], r1[NI * 2];
        uint32_t sp[NI * 2][3];
        int piece = 0, m = 0;
        auto do_piece = [&](int t) {
            const int u = t / 3, lvl = t % 3, i = u / 2, c = u % 2;
            if (lvl == 0) {
                r0[u] = g[SS][i][2 * c];
                r1[u] = g[SS][i][2 * c + 1];
            }
            const uint32_t pk = cvt_pk_bf16(r0[u], r1[u]);
            sp[u][lvl] = pk;
            if (lvl < 2) {
                r0[u] = sub_bf16_lo(r0[u], pk);
                r1[u] = sub_bf16_hi(r1[u], pk);
            } else if (c == 1) {
                unsigned char* d = wbase + dst[i];
#pragma unroll
                for (int pl = 0; pl < 3; ++pl) *reinterpret_cast<u32x2*>(d + pl * PLANE) = u32x2{sp[2 * i][pl], sp[2 * i + 1][pl]};
            }
        };
        constexpr int NFILL = NMFMA - 1 - AFM_R3_TAIL > 0 ? NMFMA - 1 - AFM_R3_TAIL : 1;      // MFMAs 2 .. NFILL + 1 carry the split
        __builtin_amdgcn_sched_barrier(0);
#pragma unroll
        for (int q = 9 - NPROD; q < 9; ++q)
#pragma unroll
            for (int tm = 0; tm < TM; ++tm)
#pragma unroll
                for (int tn = 0; tn < TN; ++tn) {
                    acc[tm][tn] = mfma_bf16(fa[cur][tm][AFM_PA[q]], fb[cur][tn][AFM_PB[q]], acc[tm][tn]);
                    ++m;
                    if (m == 1) {               // behind the first MFMA: the requests of this K-tile (nothing in it waits for them)
                        __builtin_amdgcn_sched_barrier(0);
                        load(LoadSet{}, kt + 5);
                        read_frag(FragNext{}, st_next);
                    } else {
                        const int want = ((m - 1) * NPIECE + NFILL - 1) / NFILL;
#pragma unroll
                        for (int t = 0; t < NPIECE; ++t)
                            if (t >= piece && t < want) do_piece(t);
                        piece = want < NPIECE ? want : NPIECE;
                    }
                    __builtin_amdgcn_sched_barrier(0);
                }
#pragma unroll
        for (int t = 0; t < NPIECE; ++t)              // (NPROD == 1: a single MFMA per K-tile has no slot for the split)
            if (t >= piece) do_piece(t);
        if ((KG == 1 || GSEG > 1) && ((kt + 1) % SEGT) == 0 && kt + 1 < nk) {
#pragma unroll
            for (int tm = 0; tm < TM; ++tm)
#pragma unroll
                for (int tn = 0; tn < TN; ++tn)
#pragma unroll
                    for (int r = 0; r < 16; ++r) {
                        tot[tm][tn][r] = have_tot ? tot[tm][tn][r] + acc[tm][tn][r] : acc[tm][tn][r];
                        acc[tm][tn][r] = 0.f;
                    }
            have_tot = true;
        }
        __syncthreads();
    };
    if constexpr (RING == 2) {
        for (int kt = 0; kt < nk; kt += 2) {
            body(Set0{}, kt);
            if (kt + 1 < nk) body(Set1{}, kt + 1);
        }
    } else {
        read_frag(Set0{}, 0);
        int s1 = 1, s2 = 2;                           // (kt + 1) % 3, (kt + 2) % 3
        for (int kt = 0; kt < nk; kt += 4) {         // nk % 4 == 0 (the launcher checks K)
            body3(Set0{}, kt, s1, s2);
            s1 = s2; s2 = (s1 + 1) % 3;
            body3(Set1{}, kt + 1, s1, s2);
            s1 = s2; s2 = (s1 + 1) % 3;
            body3(Set2{}, kt + 2, s1, s2);
            s1 = s2; s2 = (s1 + 1) % 3;
            body3(Set3{}, kt + 3, s1, s2);
            s1 = s2; s2 = (s1 + 1) % 3;
        }
    }

#ifdef AFM_TIMELINE
    const unsigned long long tl_kloop = __builtin_amdgcn_s_memrealtime();        // K loop done
#endif
    if (have_tot && (KG == 1 || grp == 0)) {          // ((s0 + s1) + ...) + s_last (of a later split-K group: both segment sums travel, see below)
#pragma unroll
        for (int tm = 0; tm < TM; ++tm)
#pragma unroll
            for (int tn = 0; tn < TN; ++tn)
#pragma unroll
                for (int r = 0; r < 16; ++r) acc[tm][tn][r] = tot[tm][tn][r] + acc[tm][tn][r];
    }
    if (KG > 1) {
        // groups 1 .. KG-1 hand their segment sums (GSEG of them, in segment order) to group 0 through their own (now idle) operand
        // regions: [segment][r / 4][thread] float4
        static_assert(RING * STAGE >= GSEG * 4 * 256 * 16, "the segment sums of a group fit its operand stages");
        f32x4* part = reinterpret_cast<f32x4*>(lds);
        if (grp > 0) {
            if (GSEG == 2) {
#pragma unroll
                for (int q = 0; q < 4; ++q) part[q * 256 + tid] = f32x4{tot[0][0][4 * q], tot[0][0][4 * q + 1], tot[0][0][4 * q + 2], tot[0][0][4 * q + 3]};
            }
#pragma unroll
            for (int q = 0; q < 4; ++q) part[((GSEG - 1) * 4 + q) * 256 + tid] = f32x4{acc[0][0][4 * q], acc[0][0][4 * q + 1], acc[0][0][4 * q + 2], acc[0][0][4 * q + 3]};
        }
        __syncthreads();
        if (grp == 0) {
            for (int gI = 1; gI < KG; ++gI) {
                const f32x4* pg = reinterpret_cast<const f32x4*>(lds_raw + gI * (RING * STAGE));
#pragma unroll
                for (int sI = 0; sI < GSEG; ++sI)
#pragma unroll
                    for (int q = 0; q < 4; ++q) {
                        const f32x4 v = pg[(sI * 4 + q) * 256 + tid];
                        acc[0][0][4 * q] += v[0]; acc[0][0][4 * q + 1] += v[1]; acc[0][0][4 * q + 2] += v[2]; acc[0][0][4 * q + 3] += v[3];
                    }
            }
        }
    }
    // streamed epilogue: every global input of the tile's epilogue is requested here - the operand and fragment registers and the banked
    // segment sums are dead - and flies while the accumulators are staged in LDS, across the barrier below
    static_assert(!STREAMED || (GT == 512 && BM == 128 && BN == 128 && KG == 1), "streamed epilogue: the 512-thread 128 x 128 tile");
    [[maybe_unused]] StreamedEpilogue<STREAMED ? 8 : 1> se;
    if constexpr (STREAMED) gemm_epilogue_streamed_prefetch<BM, BN, GT>(p, bm, bn, tid, se);
    float* ldsf = reinterpret_cast<float*>(lds_raw);
    if (grp == 0) {
#pragma unroll
        for (int tm = 0; tm < TM; ++tm)
#pragma unroll
            for (int tn = 0; tn < TN; ++tn)
#pragma unroll
                for (int r = 0; r < 16; ++r)
                    ldsf[(wm * (BM / WMv) + tm * 32 + mfma_row(r, lane)) * LDC + wn * (BN / 2) + tn * 32 + r32] = acc[tm][tn][r];
    }
    __syncthreads();
#ifdef AFM_TIMELINE
    const unsigned long long tl_staged = __builtin_amdgcn_s_memrealtime();       // K groups merged, accumulators staged in LDS
#endif
    // The split-K form's epilogue runs on ALL its wave groups (512 / 1024 threads: two trips / one over the 64 x 64 tile instead of four -
    // a small launch has nothing else to hide the trips' memory round trips behind; profiles/r04_gemm_timeline_small.txt: epilogue 3.5 of
    // 14.8 us).  An output element's arithmetic does not depend on which thread handles it: bit-identical.
    constexpr int ENT = (KG == 2 || KG == 4) ? 256 * KG : GT;
    if constexpr (STREAMED) {
        // Two tests in this order, the second on an opaque copy of the flag: written as if / else, hipcc lays the shared epilogue out first
        // and runs into the streamed one behind it, which keeps the 64 prefetched registers alive across the shared epilogue (104 B of scratch).
        // (the copy is made opaque in a VGPR and read back with the builtin: a v_readfirstlane written out in inline assembly is invisible to
        // hipcc's hazard recognizer and read its source one instruction behind the VALU write - both epilogues ran)
        int shared = (int)!se.on;
        asm volatile("" : "+v"(shared));
        shared = __builtin_amdgcn_readfirstlane(shared);
        if (se.on) gemm_epilogue_streamed<BM, BN, GT>(p, ldsf, bm, bn, tid, rowst, se);
        if (shared) gemm_epilogue<BM, BN, ENT>(p, ldsf, bm, bn, (int)AFM_TIDX, rowst);
    } else if (ENT > 256) gemm_epilogue<BM, BN, ENT>(p, ldsf, bm, bn, (int)AFM_TIDX, rowst);
    else if (grp == 0) gemm_epilogue<BM, BN>(p, ldsf, bm, bn, tid, rowst);
    gemm_ln_tail<BM>(p, bm, nbn, reinterpret_cast<int*>(ldsf));
    if (p.aux_dst && AFM_WG < p.aux_rows) {          // rider: one row copy (+ add) per workgroup, behind its own tile
        const int r = AFM_WG;
        int64_t ix = p.aux_idx ? p.aux_idx[r] : r;
        ix = ix < 0 ? 0 : (ix >= p.aux_idx_max ? p.aux_idx_max - 1 : ix);
        for (int c = AFM_TIDX; c < p.aux_cols; c += blockDim.x)
            p.aux_dst[(int64_t)r * p.aux_dst_ld + c] = p.aux_src[ix * p.aux_cols + c] + (p.aux_add ? p.aux_add[c] : 0.0f);
    }
#ifdef AFM_TIMELINE
    if (afm_timeline && AFM_TIDX == 0) {
        unsigned hw, xcc;
        asm volatile("s_getreg_b32 %0, hwreg(HW_REG_HW_ID)" : "=s"(hw));
        asm volatile("s_getreg_b32 %0, hwreg(HW_REG_XCC_ID)" : "=s"(xcc));
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");       // the epilogue's stores have left the wave
        const unsigned long long tl_end = __builtin_amdgcn_s_memrealtime();
        // phase spans in s_memrealtime ticks (10 ns): prologue | K loop | merge + staging | epilogue
        afm_timeline[AFM_TIMELINE_SLOT] = AfmTimelineRec{tl_t0, tl_end, hw, xcc, tl_c0, afm_cycles(), tl_pro - tl_t0, tl_kloop - tl_pro, tl_staged - tl_kloop, tl_end - tl_staged};
    }
#endif
