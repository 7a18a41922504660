// qg_mfma_ring.hip — RING plans of the linear class on the gfx950 matrix cores (v_mfma_i32_16x16x64_i8).
//
// The descriptor's product and every tree level wrap (WRP::TCPL) into one signed format R of n <= 32 bits, so the tree is a
// chain of ring homomorphisms and equals the exact dot product reduced modulo 2^n ONCE (the rule and the proof: qg_plan.cpp,
// ring_plan):        C[i,j] = cvt_C( wrap_R( 2^s * sum_k a_ik b_kj ) ).
// Everything before wrap_R may therefore be computed modulo 2^32, which 2^n divides:
//   * the operands are stored as the first LA, LB <= L = ceil(n / 8) balanced base-256 digits (QPackedGeom, the planes k_pack
//     peels anyway; the remainder is dropped): a = sum_i A_i 256^i (mod 2^(8 L));
//   * only the limb products A_i.B_j of weight i + j < L are formed: 1 / 3 / 6 / 10 of the 1 / 4 / 9 / 16 of an L x L plan;
//   * the int32 accumulators, one set per weight, are allowed to WRAP: there is no bound on K and no k-chunk
//     (the other MFMA plans keep K * min(LA, LB) < 2^17 so that theirs never do);
//   * epilogue: v = sum_w acc_w << 8 w in uint32 arithmetic, v <<= s, sign-extend the low n bits (one v_bfe_i32), then the
//     one round + overflow R -> C of qg_step_all.h (skipped where C is R) and the container store into the 128 x 128-tiled
//     packed C of every other limb plan.
//
// Tiling: 128 x 128 outputs per workgroup of 8 waves (2 x 4), a wave 64 x 32 = 4 x 2 MFMA tiles of 16 x 16: L x 32 accumulator
// registers (128 for a 32-bit ring).  64-byte k-tiles, LDS image = the packed (row tile, k tile) block, copied by lane-linear
// LDS-DMA (PPW = LA + LB pieces of 1 KiB per wave and k-tile).  The k-tile is walked in 4 row steps as k_mfma16's limb form
// does: the A fragments of row step i + 1 are read under the MFMAs of row step i, B's fragments are held for the whole k-tile.
//
// LDS ring.  A stage is (LA + LB) x 8 KiB: 64 KiB for 4 + 4 planes, and the three stages k_mfma16 keeps (tile k read, tile
// k + 1 landed, tile k + 2 in flight) would be 192 KiB of the CU's 160.  So the ONE barrier of a k-tile sits before its LAST
// row step: by then every fragment of tile k is in registers (A's last row step, B's planes), the barrier publishes tile
// k + 1 — whose first fragments are read under the last row step's MFMAs — and the stage of tile k ITSELF is refilled.  A ring
// of two stages then keeps one tile in flight for three quarters of a k-tile (4 + 4 planes: 60 of 80 MFMAs per wave), and
// three stages — taken wherever they fit, LA + LB <= 6 — keep two in flight with a counted wait.
#include <hip/hip_runtime.h>

#include <utility>

#include "qg_kernels.h"
#include "qg_mfma_tile.h"
#include "qg_ring.h"
#include "qg_step_all.h"

namespace {

constexpr int BK = QG_RING_BK, TM = QG_RING_TM, TN = QG_RING_TN;
constexpr int WGM = 2, WGN = 4, TI = 4, TJ = 2, NWAVES = WGM * WGN;
constexpr int LDS_MAX = 160 * 1024;

// limb products of weight below L
constexpr int ring_np(int LA, int LB, int L)
{
    int c = 0;
    for (int a = 0; a < LA; ++a)
        for (int b = 0; b < LB; ++b) c += a + b < L ? 1 : 0;
    return c;
}
constexpr int ring_stages(int LA, int LB) { return 3 * (LA * TM + LB * TN) * BK <= LDS_MAX ? 3 : 2; }

// LA, LB: limb planes of A, B;  L: weights kept (digits of the ring, at most LA + LB - 1: beyond that no product exists)
template <int LA, int LB, int L>
__global__ __launch_bounds__(64 * NWAVES) void k_mfma_ring(QRingArgs g)
{
    static_assert(LA >= 1 && LB >= 1 && LA <= L && LB <= L && L <= 4 && L <= LA + LB - 1, "limb planes / weights of a ring plan");
    constexpr int NSTAGE = ring_stages(LA, LB);
    constexpr int STAGE = (LA * TM + LB * TN) * BK;
    constexpr int PPW = STAGE / 1024 / NWAVES;   // = LA + LB
    constexpr int A_BYTES = LA * TM * BK, B_BYTES = LB * TN * BK, A_PIECES = A_BYTES / 1024;
    static_assert(NSTAGE * STAGE <= LDS_MAX && (NSTAGE - 1) * PPW < 64, "LDS ring; vmcnt is a 6-bit counter");
    extern __shared__ __attribute__((aligned(16))) char smem[];

    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int wm = wave / WGN, wn = wave % WGN;
    // XCD-aware tile order (qg_tile_walk.h): a contiguous run of tiles per XCD, walked in column-major groups of 8 tile rows
    const int tiles_m = (int)(g.Mp / TM), tiles_n = (int)(g.Np / TN);
    const int nwg = tiles_m * tiles_n;
    int tile_m, tile_n;
    qg_tile_of<8, true>(qg_xcd_block<int>(blockIdx.x, nwg), tiles_m, tiles_n, tile_m, tile_n);

    const int nk = (int)(g.Kp / BK);
    const int8_t* Ag = g.A + (int64_t)tile_m * nk * A_BYTES + lane * 16;
    const int8_t* Bg = g.B + (int64_t)tile_n * nk * B_BYTES + lane * 16;
    // this wave's PPW pieces of k-tile kt (clamped past the end: the last tile once more, into a stage nobody reads again, so
    // that the count of outstanding transfers is the same in every iteration)
    auto issue = [&](int stage, int kt) {
        char* sbase = smem + stage * STAGE;
        const int kc = kt < nk ? kt : nk - 1;
        const int8_t* a = Ag + (int64_t)kc * A_BYTES;
        const int8_t* b = Bg + (int64_t)kc * B_BYTES;
#pragma unroll
        for (int pi = 0; pi < PPW; ++pi) {
            const int p = wave + NWAVES * pi;   // wave-uniform piece id
            const int8_t* src = p < A_PIECES ? a + p * 1024 : b + (p - A_PIECES) * 1024;
            __builtin_amdgcn_global_load_lds(QG_GLOBAL_PTR(src), QG_LDS_PTR(sbase + p * 1024), 16, 0, 0);
        }
    };

    v4i acc[L][TI][TJ];
#pragma unroll
    for (int w = 0; w < L; ++w)
#pragma unroll
        for (int i = 0; i < TI; ++i)
#pragma unroll
            for (int j = 0; j < TJ; ++j)
#pragma unroll
                for (int e = 0; e < 4; ++e) acc[w][i][j][e] = 0;

    // fragment of v_mfma_i32_16x16x64_i8: lane l holds row (l & 15), bytes [16 (l >> 4), +16) of the 64-byte k-step; chunk c of
    // row r sits at slot c ^ qg_swz<BK>(r), and every row read is (a multiple of 16) + fr: the swizzle of fr
    const int fr = lane & 15, fq = lane >> 4;
    v4i pa[2][LA], pb[2][LB][TJ];
    auto load_a = [&](int buf, const char* sA, int i) {
        const int ra = (wm * TI + i) * 16 + fr;
#pragma unroll
        for (int l = 0; l < LA; ++l) pa[buf][l] = *(const v4i*)(sA + (l * TM + ra) * BK + ((fq ^ qg_swz<BK>(fr)) * 16));
    };
    auto load_b = [&](int buf, const char* sA) {
        const char* sB = sA + A_BYTES;
#pragma unroll
        for (int j = 0; j < TJ; ++j) {
            const int rb = (wn * TJ + j) * 16 + fr;
#pragma unroll
            for (int l = 0; l < LB; ++l) pb[buf][l][j] = *(const v4i*)(sB + (l * TN + rb) * BK + ((fq ^ qg_swz<BK>(fr)) * 16));
        }
    };
    constexpr int NM = ring_np(LA, LB, L) * TJ;   // MFMAs of one row step
    // the limb products of weight below L, row step i, A fragments from pa[i & 1], B fragments from pb[h]
    auto mfmas = [&](int i, int h) {
#pragma unroll
        for (int la = 0; la < LA; ++la)
#pragma unroll
            for (int lb = 0; lb < LB; ++lb) {
                if (la + lb >= L) continue;   // weight 256^(la + lb) >= 2^n: a multiple of the modulus
#pragma unroll
                for (int j = 0; j < TJ; ++j)
                    acc[la + lb][i][j] = __builtin_amdgcn_mfma_i32_16x16x64_i8(pa[i & 1][la], pb[h][lb][j], acc[la + lb][i][j], 0, 0, 0);
            }
    };

    // prologue: NSTAGE k-tiles in flight, tile 0 published, its first fragments read
#pragma unroll
    for (int t = 0; t < NSTAGE; ++t) issue(t, t);
    asm volatile("s_waitcnt vmcnt(%0)" ::"n"((NSTAGE - 1) * PPW) : "memory");
    __builtin_amdgcn_s_barrier();
    asm volatile("" ::: "memory");
    load_b(0, smem);
    load_a(0, smem, 0);
    int cur = 0;   // stage of tile k
    for (int kt = 0; kt < nk; kt += 2) {
#pragma unroll
        for (int h = 0; h < 2; ++h) {
            const int k = kt + h;
            if (k < nk) {
                const char* sc = smem + cur * STAGE;
                const int nx = cur + 1 == NSTAGE ? 0 : cur + 1;
                const char* sn = smem + nx * STAGE;
#pragma unroll
                for (int i = 0; i < TI; ++i) {
                    if (i + 1 < TI) {
                        load_a((i + 1) & 1, sc, i + 1);   // first use a whole row step away
                        __builtin_amdgcn_sched_barrier(0);
                        mfmas(i, h);
                        __builtin_amdgcn_sched_barrier(0);
                    } else {
                        // every fragment of tile k is in registers (lgkmcnt(0): this wave's last reads have returned) and this
                        // wave's pieces of tile k + 1 have landed; tiles k + 2 .. k + NSTAGE - 1 may fly on
                        asm volatile("s_waitcnt vmcnt(%0) lgkmcnt(0)" ::"n"((NSTAGE - 2) * PPW) : "memory");
                        __builtin_amdgcn_s_barrier();
                        asm volatile("" ::: "memory");
                        load_b(h ^ 1, sn);
                        load_a(0, sn, 0);
                        __builtin_amdgcn_sched_barrier(0);
                        issue(cur, k + NSTAGE);           // the stage of tile k itself: nobody reads it again
                        mfmas(i, h);
                        interleave_hint<NM, 0, PPW>(std::make_integer_sequence<int, NM>{});
                        __builtin_amdgcn_sched_barrier(0);
                    }
                }
                cur = nx;
            }
        }
    }
    // the clamped refills are still in flight: they must land before the workgroup ends and its LDS is handed on
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");

    // epilogue.  C/D of the 16x16 MFMA: col = lane & 15, rows 4 (lane >> 4) + e; packed C is column-major inside its tile, so a
    // lane's 4 results are one run of 4 rows
    const QStep st = g.to_c;
    char* C = (char*)g.C;
    const int64_t tile_base = ((int64_t)tile_m * tiles_n + tile_n) * TM * TN;
    const int sl = g.s, sx = 32 - g.n;
#pragma unroll
    for (int i = 0; i < TI; ++i) {
        int64_t s[4 * TJ];
#pragma unroll
        for (int j = 0; j < TJ; ++j)
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                uint32_t v = (uint32_t)acc[L - 1][i][j][e];
#pragma unroll
                for (int w = L - 2; w >= 0; --w) v = (v << 8) + (uint32_t)acc[w][i][j][e];   // modulo 2^32 throughout
                v <<= sl;
                s[j * 4 + e] = (int64_t)((int32_t)(v << sx) >> sx);                          // wrap_R: the canonical representative
            }
        qg_step_all<int64_t, 4 * TJ>(s, st);
        const int row0 = (wm * TI + i) * 16 + 4 * fq;
#pragma unroll
        for (int j = 0; j < TJ; ++j) {
            const int col = (wn * TJ + j) * 16 + fr;
            const int64_t base = tile_base + (int64_t)col * TM + row0;
            const int64_t* q = s + j * 4;
            switch (g.cbytes) {   // (written out, not qg_store_run4 with a run-time container size: as a function it moves this kernel's instruction stream)
            case 1:
                *(uint32_t*)(C + base) = (uint32_t)(q[0] & 0xff) | ((uint32_t)(q[1] & 0xff) << 8) | ((uint32_t)(q[2] & 0xff) << 16) | ((uint32_t)(q[3] & 0xff) << 24);
                break;
            case 2:
                *(uint2*)(C + base * 2) = make_uint2((uint32_t)(q[0] & 0xffff) | ((uint32_t)(q[1] & 0xffff) << 16), (uint32_t)(q[2] & 0xffff) | ((uint32_t)(q[3] & 0xffff) << 16));
                break;
            case 4:
                *(int4*)(C + base * 4) = make_int4((int)q[0], (int)q[1], (int)q[2], (int)q[3]);
                break;
            default: {
                int64_t* p = (int64_t*)(C + base * 8);
                *(longlong2*)p = make_longlong2(q[0], q[1]);
                *(longlong2*)(p + 2) = make_longlong2(q[2], q[3]);
                break;
            }
            }
        }
    }
}

template <int LA, int LB, int L>
hipError_t launch_ring(const QRingArgs& a, hipStream_t st)
{
    constexpr int lds = ring_stages(LA, LB) * (LA * TM + LB * TN) * BK;
    const int64_t blocks = (a.Mp / TM) * (a.Np / TN);
    return qg_launch_lds<k_mfma_ring<LA, LB, L>>((unsigned)blocks, 64 * NWAVES, lds, st, a);
}

} // namespace

hipError_t qg_launch_mfma_ring(int LA, int LB, int L, const QRingArgs& a, hipStream_t st)
{
    if (LA < 1 || LB < 1 || L < 1 || L > 4 || LA > L || LB > L) return hipErrorInvalidValue;
    if (a.n < 1 || a.n > 32 || a.s < 0 || a.s >= a.n || qg_ring_digits(a.n) != L) return hipErrorInvalidValue;
    if (a.cbytes != 1 && a.cbytes != 2 && a.cbytes != 4 && a.cbytes != 8) return hipErrorInvalidValue;
    if (a.Kp <= 0 || a.Kp % BK || a.Mp % TM || a.Np % TN) return hipErrorInvalidValue;
    const int64_t blocks = (a.Mp / TM) * (a.Np / TN);
    if (blocks <= 0) return hipSuccess;
    if (blocks > 0x7fffffffll) return hipErrorInvalidValue;
    const int W = L < LA + LB - 1 ? L : LA + LB - 1;   // weights that have a product at all
    switch (LA * 100 + LB * 10 + W) {
#define QG_RING_CASE(la, lb, w) case la * 100 + lb * 10 + w: return launch_ring<la, lb, w>(a, st)
    QG_RING_CASE(1, 1, 1);
    QG_RING_CASE(1, 2, 2); QG_RING_CASE(2, 1, 2); QG_RING_CASE(2, 2, 2); QG_RING_CASE(2, 2, 3);
    QG_RING_CASE(1, 3, 3); QG_RING_CASE(3, 1, 3); QG_RING_CASE(2, 3, 3); QG_RING_CASE(3, 2, 3); QG_RING_CASE(3, 3, 3);
    QG_RING_CASE(2, 3, 4); QG_RING_CASE(3, 2, 4); QG_RING_CASE(3, 3, 4);
    QG_RING_CASE(1, 4, 4); QG_RING_CASE(4, 1, 4); QG_RING_CASE(2, 4, 4); QG_RING_CASE(4, 2, 4);
    QG_RING_CASE(3, 4, 4); QG_RING_CASE(4, 3, 4); QG_RING_CASE(4, 4, 4);
#undef QG_RING_CASE
    default: return hipErrorInvalidValue;
    }
}
