// qg_mfma_body.h — the body of k_mfma and k_mfma_bd (qg_mfma.hip), k_mfma_ep_bd (qg_mfma_ep_bd.hip), k_mfma_grp (qg_mfma_grp.hip) and k_mfma_ep_grp (qg_mfma_ep_grp.hip), included INSIDE the
// kernels: no include guard, nothing at namespace scope.  In scope where it is included: the kernel argument `QMfmaArgs g` (BD with
// EP: a QMfmaEpBdArgs; GRP: a QMfmaGrpArgs, with EP a QMfmaEpGrpArgs: k_mfma_ep_grp, qg_mfma_ep_grp.hip) and the compile-time constants LA, LB, BK, WGM, WGN, TI, TJ, NSTAGE, ABL, EP, SA, SB, KARA,
// KS, BD, GRP (their meaning: the comment in front of k_mfma; GRP: k_mfma_grp, qg_mfma_grp.hip).
    if constexpr (SA == 3 && SB == 3 && ABL == 0) {
        const unsigned ma = qg_plane_mask(g.maskA);
        const unsigned mb = qg_plane_mask(g.maskB);
        const bool two_planes_suffice = ((ma | mb) & 4u) == 0;
        if (two_planes_suffice != (LA == 2)) return;   // the other kernel of this launch pair does the work
    }
    constexpr int TM = WGM * TI * 32, TN = WGN * TJ * 32;
    constexpr int NWAVES = WGM * WGN;
    constexpr int NW = LA + LB - 1;            // limb weights
    constexpr int ROWS = LA * TM + LB * TN;    // LDS rows per stage
    constexpr int STAGE = ROWS * BK;           // bytes per stage
    constexpr int PIECES = STAGE / 1024;       // 1-KiB LDS-DMA pieces per stage
    constexpr int PPW = PIECES / NWAVES;       // pieces (LDS-DMA instructions) per wave per stage
    constexpr int KSTEPS = BK / 32;            // MFMA k-steps per tile
    static_assert(PIECES % NWAVES == 0, "every wave issues the same number of LDS-DMA pieces");
    static_assert(NSTAGE >= 2 && (NSTAGE - 2) * PPW < 64, "vmcnt is a 6-bit counter");
    extern __shared__ __attribute__((aligned(16))) char smem_all[];

    const int lane = threadIdx.x & 63;
    const int wave_all = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int kg = KS > 1 ? wave_all / NWAVES : 0;          // k group of this wave (wave-uniform)
    const int wave = KS > 1 ? wave_all % NWAVES : wave_all;
    char* smem = smem_all + kg * (NSTAGE * STAGE);           // the group's own ring
    const int wm = wave / WGN, wn = wave % WGN;

    // XCD-aware tile order (qg_tile_walk.h): a contiguous run of tiles per XCD, walked in column-major groups of 8 tile rows
    const int tiles_m = (int)(g.Mp / TM), tiles_n = (int)(g.Np / TN);
    const int nwg = tiles_m * tiles_n;
    int tile_m, tile_n;
    int64_t bd_c_tile = 0;   // BD: this workgroup's tile of the batch's packed C
    int bd_member = 0;       // BD: the member that tile belongs to (wave-uniform)
    int64_t grp_a = 0, grp_b = 0, grp_c = 0, grp_corr = 0;   // GRP: this workgroup's record of the host's schedule (qg_grp.h)
    int grp_nk = 0;
    int grp_member = 0;      // GRP with EP: the member of the caller's list this workgroup's tile belongs to (wave-uniform)
    if constexpr (GRP) {
        // grouped launch: block bid reads record bid — where its A and B blocks start, where its C tile goes, its k-tile count, its
        // rows of the stack's row sums and its member's K biasA biasB.  One wave-uniform load of 48 bytes; no division, no tile walk
        static_assert(!GRP || (!BD && KS == 1 && !KARA && ABL == 0 && TM == 64 && TN == 64), "grouped form: the plain lock-step body on 64 x 64 tiles");
        const QGrpTile rec = qg_dependent<LA>(g).tiles[blockIdx.x];   // (a field of the grouped kernels' argument structs only: qg_dependent, qg_kernels.h)
        grp_a = rec.a_off;
        grp_b = rec.b_off;
        grp_c = rec.c_off;
        grp_corr = rec.corr;
        grp_nk = rec.nk;
        if constexpr (EP) {   // (wave-uniform; said so: the member indexes the scalar tables, the C offset goes into base pointers)
            grp_member = __builtin_amdgcn_readfirstlane(rec.member);
            grp_c = (int64_t)(((uint64_t)(uint32_t)__builtin_amdgcn_readfirstlane((int)(rec.c_off >> 32)) << 32) | (uint32_t)__builtin_amdgcn_readfirstlane((int)rec.c_off));
        }
        tile_m = (int)((unsigned)rec.row_a / (unsigned)TM);   // (the row sums' rows: tile_m * TM, tile_n * TN)
        tile_n = (int)((unsigned)rec.row_b / (unsigned)TN);
    } else
    if constexpr (BD) {
        // tiles_m, tiles_n count the STACK's row tiles; the batch has gridDim.x = batch * bd_tm * bd_tn tiles on its diagonal
        static_assert(!BD || (KS == 1 && !KARA && ABL == 0), "block-diagonal form: the plain lock-step body");
        int member, lm, ln;
        qg_bd_tile_of<int>(qg_xcd_block<int>(blockIdx.x, (int)gridDim.x), g.bd_tm, g.bd_tn, member, lm, ln);
        tile_m = member * g.bd_tm + lm;
        tile_n = member * g.bd_tn + ln;
        bd_c_tile = ((int64_t)member * g.bd_tm + lm) * g.bd_tn + ln;
        bd_member = member;
    } else
    qg_tile_of<8, true>(qg_xcd_block<int>(blockIdx.x, nwg), tiles_m, tiles_n, tile_m, tile_n);

    // operands are pre-tiled: block (row tile, k tile) of A is LA*TM*BK contiguous bytes that are
    // already the swizzled LDS image; same for B.  A stage is two linear copies.
    const int nk_all = GRP ? grp_nk : (int)(g.Kp / BK);
    const int nk = nk_all / KS;                                         // k-tiles of this group (the launcher checks divisibility)
    constexpr int A_BYTES = LA * TM * BK, B_BYTES = LB * TN * BK;       // copied per stage (the first LA / LB planes)
    constexpr int A_STORED = SA * TM * BK, B_STORED = SB * TN * BK;     // stride of a (row tile, k tile) block in memory
    constexpr int A_PIECES = A_BYTES / 1024;
    const int8_t* Ag = g.A + (GRP ? grp_a : ((int64_t)tile_m * nk_all + (int64_t)kg * nk) * A_STORED) + lane * 16;
    const int8_t* Bg = g.B + (GRP ? grp_b : ((int64_t)tile_n * nk_all + (int64_t)kg * nk) * B_STORED) + lane * 16;

    auto issue = [&](int stage, int kt) {
        char* sbase = smem + stage * STAGE;
        const int kts = ABL == 6 ? 0 : kt;  // diagnostic: re-read k-tile 0 (cache hits) to separate DMA cost from traffic cost
        const int8_t* a = Ag + (int64_t)kts * A_STORED;
        const int8_t* b = Bg + (int64_t)kts * B_STORED;
#pragma unroll
        for (int pi = 0; pi < PPW; ++pi) {
            const int p = wave + NWAVES * pi;       // wave-uniform piece id
            const int8_t* src = p < A_PIECES ? a + p * 1024 : b + (p - A_PIECES) * 1024;
            __builtin_amdgcn_global_load_lds(QG_GLOBAL_PTR(src), QG_LDS_PTR(sbase + p * 1024), 16, 0, 0);
        }
    };

    v16i acc[NW][TI][TJ];
#pragma unroll
    for (int w = 0; w < NW; ++w)
#pragma unroll
        for (int i = 0; i < TI; ++i)
#pragma unroll
            for (int j = 0; j < TJ; ++j)
#pragma unroll
                for (int e = 0; e < 16; ++e) acc[w][i][j][e] = 0;

    const int fr = lane & 31, fh = lane >> 5;
    // Software pipeline (needs NSTAGE == 3 stages, KSTEPS even):
    //   * fragments are double-buffered in registers: while the MFMAs of k-step s run, the
    //     ds_read_b128s of k-step s+1 are already in flight, so LDS latency is never exposed;
    //   * ONE barrier per k-tile, placed before the LAST k-step of tile kt: it publishes tile kt+1
    //     (every wave has waited for its own LDS-DMA pieces of that tile), after which the first
    //     fragments of tile kt+1 are prefetched and the stage last read in iteration kt-1 is
    //     refilled with tile kt+2 (raw s_barrier: __syncthreads() would also drain the DMA queue).
    static_assert((NSTAGE == 3 || (NSTAGE > 3 && ABL == 0)) && KSTEPS % 2 == 0, "pipeline shape");
    v4i fa[2][LA][TI], fb[2][LB][TJ];
    auto load_frags = [&](int set, const char* stage_base, int ks) {
        const char* sA = stage_base;
        const char* sB = stage_base + LA * TM * BK;
        const int c = 2 * ks + fh;
#pragma unroll
        for (int i = 0; i < TI; ++i) {
            const int ra = (wm * TI + i) * 32 + fr;
#pragma unroll
            for (int l = 0; l < LA; ++l) fa[set][l][i] = *(const v4i*)(sA + (l * TM + ra) * BK + ((c ^ qg_swz<BK>(ra)) * 16));
        }
#pragma unroll
        for (int j = 0; j < TJ; ++j) {
            const int rb = (wn * TJ + j) * 32 + fr;
#pragma unroll
            for (int l = 0; l < LB; ++l) fb[set][l][j] = *(const v4i*)(sB + (l * TN + rb) * BK + ((c ^ qg_swz<BK>(rb)) * 16));
        }
    };
    // the LA*LB*TI*TJ MFMAs of one k-step, optionally only those with index in [first, last)
    auto mfmas = [&](int set, int first, int last) {
        if constexpr (KARA) {
            static_assert(!KARA || (LA == 2 && LB == 2), "Karatsuba variant: 2 x 2 digits");
            v4i sa[TI], sb[TJ];
#pragma unroll
            for (int i = 0; i < TI; ++i) sa[i] = fa[set][0][i] + fa[set][1][i];
#pragma unroll
            for (int j = 0; j < TJ; ++j) sb[j] = fb[set][0][j] + fb[set][1][j];
#pragma unroll
            for (int i = 0; i < TI; ++i)
#pragma unroll
                for (int j = 0; j < TJ; ++j) {
                    acc[0][i][j] = __builtin_amdgcn_mfma_i32_32x32x32_i8(fa[set][0][i], fb[set][0][j], acc[0][i][j], 0, 0, 0);   // P0
                    acc[2][i][j] = __builtin_amdgcn_mfma_i32_32x32x32_i8(fa[set][1][i], fb[set][1][j], acc[2][i][j], 0, 0, 0);   // P1
                    acc[1][i][j] = __builtin_amdgcn_mfma_i32_32x32x32_i8(sa[i], sb[j], acc[1][i][j], 0, 0, 0);                   // P01
                }
            return;
        }
        int n = 0;
#pragma unroll
        for (int la = 0; la < LA; ++la)
#pragma unroll
            for (int lb = 0; lb < LB; ++lb)
#pragma unroll
                for (int i = 0; i < TI; ++i)
#pragma unroll
                    for (int j = 0; j < TJ; ++j, ++n)
                        if (n >= first && n < last)
                            acc[la + lb][i][j] = __builtin_amdgcn_mfma_i32_32x32x32_i8(fa[set][la][i], fb[set][lb][j], acc[la + lb][i][j], 0, 0, 0);
    };
    constexpr int NM = (KARA ? 3 : LA * LB) * TI * TJ;  // MFMAs per k-step per wave

    // prologue: tiles 0 and 1 in flight, tile 0 published, its first fragments loaded
    issue(0, 0);
    if constexpr (NSTAGE == 3) {
        if (nk > 1) issue(1, 1);
        if (nk > 1) asm volatile("s_waitcnt vmcnt(%0)" ::"n"(PPW) : "memory");
        else asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    } else {
        // NSTAGE - 1 tiles in flight (small problems: a k-tile of a 64x64-tile kernel is ~100 issue cycles, a fraction of one
        // trip to L2, so with two tiles in flight every k-tile waits for its data); past the end the last tile is fetched again
#pragma unroll
        for (int t = 1; t < NSTAGE - 1; ++t) issue(t, t < nk ? t : nk - 1);
        asm volatile("s_waitcnt vmcnt(%0)" ::"n"((NSTAGE - 2) * PPW) : "memory");
    }
    __builtin_amdgcn_s_barrier();
    asm volatile("" ::: "memory");
    load_frags(0, smem, 0);
    int cur = 0;  // stage of tile kt
    for (int kt = 0; kt < nk; ++kt) {
        const char* sc = smem + cur * STAGE;
        const int nx = cur + 1 == NSTAGE ? 0 : cur + 1;   // stage of tile kt+1
        const int rf = cur == 0 ? NSTAGE - 1 : cur - 1;   // stage of tile kt-1: refilled with tile kt+NSTAGE-1
#pragma unroll
        for (int ks = 0; ks < KSTEPS; ++ks) {
            if (ks + 1 < KSTEPS) {
                if (ABL != 2 && ABL != 3 && ABL != 4) load_frags((ks + 1) & 1, sc, ks + 1);
                if constexpr (ABL == 0) {
                    mfmas(ks & 1, 0, NM);
                    interleave_hint<NM, LA * TI + LB * TJ, 0>(std::make_integer_sequence<int, NM>{});
                    continue;
                }
            } else {
                // tile kt+1 was issued one iteration ago: wait for this wave's pieces, then publish
                if (ABL != 4) {
                    asm volatile("s_waitcnt vmcnt(%0)" ::"n"((NSTAGE - 3) * PPW) : "memory");   // tile kt+1 is in; kt+2 ... may fly on
                    __builtin_amdgcn_s_barrier();
                    asm volatile("" ::: "memory");
                }
                // (staggering the DMA issue between the two waves of a SIMD was measured: no gain for
                // the limb kernel, 2-4 % slower for the single-limb one — all waves issue here)
                if constexpr (ABL == 0) {
                    // branch-free refill (past the end: the last tile once more, into a stage nobody reads again) so that the
                    // LDS-DMA issues, the fragment reads of the next tile and this k-step's MFMAs share one basic block
                    issue(rf, kt + NSTAGE - 1 < nk ? kt + NSTAGE - 1 : nk - 1);
                    load_frags(0, smem + nx * STAGE, 0);
                    mfmas(ks & 1, 0, NM);
                    interleave_hint<NM, LA * TI + LB * TJ, PPW>(std::make_integer_sequence<int, NM>{});
                    continue;
                }
                if (kt + 2 < nk && ABL != 1 && ABL != 3 && ABL != 4) issue(rf, kt + 2);
                if (kt + 1 < nk && ABL != 2 && ABL != 3 && ABL != 4) load_frags(0, smem + nx * STAGE, 0);
            }
            mfmas(ks & 1, 0, NM);
        }
        cur = nx;
    }
    // the branch-free refill leaves LDS-DMA transfers of the clamped tile in flight: they must have landed before this
    // workgroup can end and its LDS be handed to another one
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");

    if constexpr (KS > 1) {
        // sum the groups' accumulators: groups 1 .. KS-1 park theirs in LDS (the rings are free now), group 0 adds them
        static_assert(KS == 1 || (NW == 1 && !KARA && !EP), "k split: single-limb kernels");
        __syncthreads();
        int* red = (int*)smem_all;   // [KS - 1][NWAVES][TI * TJ][16][64]
        if (kg > 0) {
#pragma unroll
            for (int i = 0; i < TI; ++i)
#pragma unroll
                for (int j = 0; j < TJ; ++j)
#pragma unroll
                    for (int e = 0; e < 16; ++e) red[((((kg - 1) * NWAVES + wave) * (TI * TJ) + i * TJ + j) * 16 + e) * 64 + lane] = acc[0][i][j][e];
        }
        __syncthreads();
        if (kg > 0) return;
#pragma unroll
        for (int q = 0; q < KS - 1; ++q)
#pragma unroll
            for (int i = 0; i < TI; ++i)
#pragma unroll
                for (int j = 0; j < TJ; ++j)
#pragma unroll
                    for (int e = 0; e < 16; ++e) acc[0][i][j][e] += red[(((q * NWAVES + wave) * (TI * TJ) + i * TJ + j) * 16 + e) * 64 + lane];
    }

    // epilogue: recombine limb weights, ONE round + overflow into C, store.
    // C/D layout of the 32x32 MFMA: col = lane & 31, row = (e & 3) + 8 * (e >> 2) + 4 * (lane >> 5),
    // i.e. every lane owns runs of 4 consecutive rows of one column.  Packed C is tiled
    // [tile_m][tile_n][col][row] (column-major inside the tile, the order of the host tensor), so a
    // run of 4 rows is one 4/8/16/32-byte store per lane.
    const QStep st = g.to_c;
    char* C = (char*)g.C;
    const int64_t tile_base = GRP ? grp_c : (BD ? bd_c_tile : ((int64_t)tile_m * tiles_n + tile_n)) * TM * TN;
    using S = std::conditional_t<(NW == 1), int32_t, int64_t>;  // one limb pair: the int32 accumulator is the dot product
#pragma unroll
    for (int i = 0; i < TI; ++i)
#pragma unroll
        for (int j = 0; j < TJ; ++j) {
            S s[16];
            if constexpr (KARA) {
                const int64_t cj = g.corr - g.biasA * g.rsB[(int64_t)tile_n * TN + (wn * TJ + j) * 32 + fr];
                const int64_t* ra = g.rsA + (int64_t)tile_m * TM + (wm * TI + i) * 32 + 4 * fh;
#pragma unroll
                for (int e = 0; e < 16; ++e) {
                    const int64_t p0 = acc[0][i][j][e], p01 = acc[1][i][j][e], p1 = acc[2][i][j][e];
                    s[e] = (S)(p0 + 64 * (p01 - p0 - p1) + 4096 * p1 - g.biasB * ra[(e & 3) + 8 * (e >> 2)] + cj);
                }
            } else {
#pragma unroll
                for (int e = 0; e < 16; ++e) {
                    S x = (S)acc[NW - 1][i][j][e];
#pragma unroll
                    for (int w = NW - 2; w >= 0; --w) x = x * 256 + (S)acc[w][i][j][e];
                    s[e] = x;
                }
                if constexpr (NW > 1) {
                    if (g.rsA) {   // centred operands (QPackedGeom::offs): sum a b = sum a'b' - biasB rsA[row] - biasA rsB[col] + K biasA biasB (wrapping)
                        const uint64_t cj = (uint64_t)(GRP ? grp_corr : g.corr) - (uint64_t)g.biasA * (uint64_t)g.rsB[(int64_t)tile_n * TN + (wn * TJ + j) * 32 + fr];
                        const int64_t* ra = g.rsA + (int64_t)tile_m * TM + (wm * TI + i) * 32 + 4 * fh;
#pragma unroll
                        for (int e = 0; e < 16; ++e) s[e] = (S)((uint64_t)s[e] + cj - (uint64_t)g.biasB * (uint64_t)ra[(e & 3) + 8 * (e >> 2)]);
                    }
                }
            }
            bool converted = false;
            if constexpr (NW == 1 && !KARA) {
                if (g.rsA) {   // a centred single-limb pair: the sum needs 64 bits, its image in C (at most 31 bits: qg_geom.cpp) does not
                    const uint64_t cj = (uint64_t)(GRP ? grp_corr : g.corr) - (uint64_t)g.biasA * (uint64_t)g.rsB[(int64_t)tile_n * TN + (wn * TJ + j) * 32 + fr];
                    const int64_t* ra = g.rsA + (int64_t)tile_m * TM + (wm * TI + i) * 32 + 4 * fh;
#pragma unroll
                    for (int e = 0; e < 16; ++e)
                        s[e] = (S)qg_step<int64_t>((int64_t)((uint64_t)(int64_t)s[e] + cj - (uint64_t)g.biasB * (uint64_t)ra[(e & 3) + 8 * (e >> 2)]), st);
                    converted = true;
                }
            }
            if (!converted) qg_step_all<S, 16>(s, st);
            if (ABL == 5 && s[0] != (S)0x7ead1234) continue; // diagnostic: keep the arithmetic, drop the stores
            const int col = (wn * TJ + j) * 32 + fr;
            const int row0 = (wm * TI + i) * 32 + 4 * fh;
            const int64_t base = tile_base + (int64_t)col * TM + row0;
            if constexpr (EP) {
                // the value just converted into C's element type goes through the element-wise chain and is stored
                // as D: C itself never reaches memory (qg_eltwise.h); 32-bit arithmetic when the planner allows it
                // (fused only for chains the planner has bounded by 32 bits: qg_geom.cpp, qg_fuses_epilogue)
                int32_t v[16];
#pragma unroll
                for (int e = 0; e < 16; ++e) v[e] = (int32_t)s[e];
                if constexpr (GRP) {
                    // the tile's base is the launch-wide element index already (D and every tensor operand: the members back to back).
                    // It is wave-uniform and goes into the operands' and D's base pointers; what a lane adds is its index inside the
                    // tile, below 4096: 32-bit offsets, where 64-bit element indices per run and container cost a third wave per SIMD.
                    // A per-member scalar stage takes its member's value from the plan's table: a uniform load, nothing per lane
                    const uint32_t lane0 = (uint32_t)(col * TM + row0);
                    qg_ep_apply_runs<int32_t, 4>(v, g.ep, QEpSrcGroup{g.epa, tile_base, lane0, 8, qg_dependent<LA>(g).ge, grp_member});
                    char* Dt = C + tile_base * g.ep.dbytes;
#pragma unroll
                    for (int q = 0; q < 4; ++q) qg_ep_store_run<int32_t>(Dt + (lane0 + 8u * q) * (uint32_t)g.ep.dbytes, 0, g.ep.dbytes, v + 4 * q);
                    continue;
                } else
                if constexpr (BD) {   // D and per-member operands at the stack-wide index, a shared operand at the member-local one
                    const QBdEp be = qg_dependent<LA>(g).bd;
                    qg_ep_apply_runs<int32_t, 4>(v, g.ep, QEpSrcStack{g.epa, base, 8, (int64_t)bd_member * be.msize, be.shared});
                } else
                qg_ep_apply_runs<int32_t, 4>(v, g.ep, QEpSrcOne{g.epa, base, 8});
#pragma unroll
                for (int q = 0; q < 4; ++q) qg_ep_store_run<int32_t>(C, base + 8 * q, g.ep.dbytes, v + 4 * q);
            } else   // (written out, not qg_store_run4 with a run-time container size: as a function it moves this kernel's instruction stream)
            switch (g.cbytes) {
            case 1:
#pragma unroll
                for (int q = 0; q < 4; ++q)
                    *(uint32_t*)(C + base + 8 * q) = (uint32_t)(s[4 * q] & 0xff) | ((uint32_t)(s[4 * q + 1] & 0xff) << 8) |
                                                     ((uint32_t)(s[4 * q + 2] & 0xff) << 16) | ((uint32_t)(s[4 * q + 3] & 0xff) << 24);
                break;
            case 2:
#pragma unroll
                for (int q = 0; q < 4; ++q)
                    *(uint2*)(C + (base + 8 * q) * 2) = make_uint2((uint32_t)(s[4 * q] & 0xffff) | ((uint32_t)(s[4 * q + 1] & 0xffff) << 16),
                                                                 (uint32_t)(s[4 * q + 2] & 0xffff) | ((uint32_t)(s[4 * q + 3] & 0xffff) << 16));
                break;
            case 4:
#pragma unroll
                for (int q = 0; q < 4; ++q)
                    *(int4*)(C + (base + 8 * q) * 4) = make_int4((int)s[4 * q], (int)s[4 * q + 1], (int)s[4 * q + 2], (int)s[4 * q + 3]);
                break;
            default:
#pragma unroll
                for (int q = 0; q < 4; ++q) {
                    int64_t* p = (int64_t*)(C + (base + 8 * q) * 8);
                    *(longlong2*)p = make_longlong2((int64_t)s[4 * q], (int64_t)s[4 * q + 1]);
                    *(longlong2*)(p + 2) = make_longlong2((int64_t)s[4 * q + 2], (int64_t)s[4 * q + 3]);
                }
                break;
            }
        }
