// qg_mfma_k6.hip — operands of 17/18 value+sign bits as THREE UNSIGNED BASE-64 DIGITS, six digit products per MAC instead of the
// nine limb products of k_mfma_ppl (three-digit Karatsuba), on 96x128 output tiles and 64-byte k-tiles, with the two wave groups
// of a workgroup taking turns on the matrix cores (the scheme of qg_mfma_ppl.hip).
//
// Arithmetic.  The planes hold the digits d0, d1, d2 of a' = a + biasA (QPackedGeom::digit6; padding holds 0), e0, e1, e2 of b'.
// Digits are <= 63, a sum of two is <= 126: four bytes add with ONE v_add_u32, no carry crosses a byte, and the sum is a valid int8.
// Six int32 accumulator sets, ONE product each (so K * 126^2 < 2^31 is the planner's bound):
//     S00 = d0.e0   S11 = d1.e1   S22 = d2.e2   P01 = (d0+d1).(e0+e1)   P12 = (d1+d2).(e1+e2)   P02 = (d0+d2).(e0+e2)
//     sum a'b' = S00 + 64 (P01-S00-S11) + 64^2 (P02-S00-S22+S11) + 64^3 (P12-S11-S22) + 64^4 S22          (64-bit, epilogue)
//     sum a b  = sum a'b' - biasB rsA[i] - biasA rsB[j] + K biasA biasB                                    (row sums of a', b')
// then the ONE round + overflow into C's format (qg_step_all.h), as the KARA epilogue of qg_mfma.hip.
//
// A workgroup is 8 waves (2 x 4); group g owns rows 48g .. 48g+47 of the tile, a wave 48 x 32 outputs (3 x 2 tiles of 16 x 16):
// 6 sets x 6 tiles x 4 = 144 accumulator registers.  All three digit planes of a k-tile are held in registers (3 x (12 + 8) = 60)
// and the three sums are formed IN PLACE, so a k-tile is ONE phase:
//     LOAD : 15 ds_read_b128 (d0, e0, d1, e1, d2, e2); 6 LDS-DMA issues; vmcnt(6); lgkmcnt(0); s_barrier
//            No vector ALU instruction: the two LDS read addresses are carried in registers, and a DMA address is a scalar base
//            (cursor + piece) beside the lane's 32-bit offset.  The partner on the SIMD is in its MFMA interval at priority 1,
//            and a vector instruction beside it waits for an issue slot.
//     MFMA : S00, S11, S22 (18 MFMAs on the plain digits), and beside them on the vector pipe
//            d1 += d2 -> P12;   d1 += d0 - d2 (= d0 + d1; hipcc forms the pairwise sum directly) -> P01;   d0 += d2 -> P02;
//            36 MFMAs, 60 v_add_u32 and the two adds that move the LDS read addresses on to the next k-tile, in a FIXED issue
//            order (paced_valu_hint, qg_mfma_tile.h): 31 x (one MFMA, two adds), then 5 MFMAs.  The interval opens with an MFMA,
//            no run of adds outlasts the issue slots a 16-cycle MFMA leaves free, and every sum is formed at least one MFMA
//            ahead of the MFMA that reads it (no s_nop).                                                      s_barrier
// and waves 4-7 run one barrier interval behind waves 0-3: on every SIMD one wave feeds the matrix pipe while its partner reads
// LDS and issues DMA.  (The first version walked a k-tile in two phases of 18 MFMAs with the sums formed in the LOAD intervals
// and A's 18 pieces rounded up to 24 issues: 0.364 ms at 4096^3, no faster than the nine products; a LOAD interval — reads, their
// latency, the dependent adds, DMA issue — was longer than 288 matrix-pipe cycles.  One phase of 576: 0.318 ms.  DESIGN.md §5.1b.)
//
// LDS: a ring of THREE buffers of one whole k-tile each: A's planes (96 rows x 64 B = 6 KiB each), then B's (128 x 64 B = 8 KiB
// each): 42 KiB, 126 KiB in all.  During k-tile kt every wave issues its pieces of k-tile kt+2 into the buffer that k-tile kt-1
// has left (both groups are past it: group 1's reads of kt-1 retire before the barrier that opens group 0's LOAD interval of kt).
// In global memory the three planes of a (row tile, k-tile) block are contiguous (QPackedGeom), and so they are in LDS: B is 24
// pieces of 1 KiB, A is 18.  Wave w issues, per k-tile, a CONSTANT six:
//     B pieces w, 8+w, 16+w (its eighth of e0, e1, e2);   A pieces w and 8+w;   and of A's last 2 KiB the quarter piece w
//     (global_load_lds of 4 bytes per lane, 256 B per wave): 8 x (2 KiB + 256 B) = 18 KiB, nothing fetched twice.
// ONE counted wait per k-tile: at the end of the LOAD interval all but the 6 youngest issues (those of kt+2) must have landed,
// i.e. the wave's share of k-tile kt+1 — before the barrier that closes the LOAD interval preceding group 0's first read of kt+1,
// for both groups.  Every piece has a whole k-tile to arrive.  Workgroups are persistent (one per CU, a list of tiles each) and
// the DMA ring runs across tile boundaries; both groups run a tile's epilogue at the same time.
#include <hip/hip_runtime.h>

#include <type_traits>

#include "qg_kernels.h"
#include "qg_mfma_tile.h"
#include "qg_step_all.h"

namespace {

constexpr int TM = 96, TN = 128, BK = 64;
constexpr int PLANE_A = TM * BK, PLANE_B = TN * BK;   // 6 and 8 pieces of 1 KiB
constexpr int BUF = 3 * PLANE_A + 3 * PLANE_B;        // one k-tile: A's planes, then B's
constexpr int NBUF = 3;

// base + S00 + 2^6 c1 + 2^12 c2 + 2^18 c3 + 2^24 S22 (mod 2^64) from five unsigned 32-bit pieces: one 64-bit add and four
// v_mad_u64_u32.  The weights pass through an empty asm so that they stay run-time scalars: written as constants hipcc turns each
// product into v_lshlrev_b64 + v_lshl_add_u64 with a v_mov of the zero high half — 216 vector instructions more per tile, 3 us
// more fixed cost per 4096^2 launch.
__device__ __forceinline__ uint64_t k6_recombine(uint32_t s00, uint32_t c1, uint32_t c2, uint32_t c3, uint32_t s22, uint64_t base)
{
    uint32_t m6 = 1u << 6, m12 = 1u << 12, m18 = 1u << 18, m24 = 1u << 24;
    asm("" : "+s"(m6), "+s"(m12), "+s"(m18), "+s"(m24));
    uint64_t x = base + s00;
    x = (uint64_t)c1 * m6 + x;
    x = (uint64_t)c2 * m12 + x;
    x = (uint64_t)c3 * m18 + x;
    return (uint64_t)s22 * m24 + x;
}

// FAST: truncation (TRN::TCPL, right shift d >= 0) + SAT::TCPL as a 64-bit shift and a clamp; otherwise the general routine.
// CB: container bytes of C (4 or 8).
template <bool FAST, int CB>
__global__ __launch_bounds__(512) void k_mfma_k6(QMfmaArgs g)
{
    extern __shared__ __attribute__((aligned(16))) char smem[];
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int wm = wave >> 2, wn = wave & 3;   // group 0 = waves 0-3 (rows 0-47 of the tile), group 1 = waves 4-7

    const int tiles_m = (int)(g.Mp / TM), tiles_n = (int)(g.Np / TN);
    const int nwg = tiles_m * tiles_n;
    const QTileList my = qg_tile_list(nwg, blockIdx, gridDim);   // this workgroup's tiles (qg_tile_walk.h)
    const int n_my = my.count;
    if (n_my == 0) return;

    const int nk = (int)(g.Kp / BK);
    const int64_t panel_a = (int64_t)nk * 3 * PLANE_A, panel_b = (int64_t)nk * 3 * PLANE_B;
    // lane offsets of the DMA sources: 32-bit, in one register each, beside a scalar base (c.a + piece): global_load_lds v, s[..]
    uint32_t lane16 = (uint32_t)(lane * 16), lane4 = (uint32_t)(lane * 4);
    // this wave's pieces (byte offsets inside a k-tile block of A / of B; the LDS image has the same order)
    const int pa0 = wave * 1024, pa1 = (8 + wave) * 1024, pa2 = 16 * 1024 + wave * 256;   // (pa2: a quarter piece, 4 bytes per lane)
    const int pb0 = wave * 1024, pb1 = (8 + wave) * 1024, pb2 = (16 + wave) * 1024;
    struct Cursor { const int8_t* a; const int8_t* b; int kt, ti; };
    auto cursor_at_tile = [&](int ti) {
        int tm, tn;
        qg_tile_of<8>(my.first + ti * my.step, tiles_m, tiles_n, tm, tn);
        return Cursor{g.A + tm * panel_a, g.B + tn * panel_b, 0, ti};
    };
    auto advance = [&](Cursor c) {
        if (c.kt + 1 < nk) return Cursor{c.a + 3 * PLANE_A, c.b + 3 * PLANE_B, c.kt + 1, c.ti};
        if (c.ti + 1 < n_my) return cursor_at_tile(c.ti + 1);
        return c;   // past the end: the last k-tile again, into a buffer nobody reads (branch-free issue keeps the vmcnt count)
    };
    auto issue_a = [&](int buf_off, int piece, const Cursor& c) {
        __builtin_amdgcn_global_load_lds(QG_GLOBAL_PTR(c.a + piece + lane16), QG_LDS_PTR(smem + buf_off + piece), 16, 0, 0);
    };
    auto issue_b = [&](int buf_off, int piece, const Cursor& c) {
        __builtin_amdgcn_global_load_lds(QG_GLOBAL_PTR(c.b + piece + lane16), QG_LDS_PTR(smem + buf_off + 3 * PLANE_A + piece), 16, 0, 0);
    };
    auto issue_tile = [&](int buf_off, const Cursor& c) {
        issue_b(buf_off, pb0, c);
        issue_a(buf_off, pa0, c);
        issue_b(buf_off, pb1, c);
        issue_a(buf_off, pa1, c);
        issue_b(buf_off, pb2, c);
        __builtin_amdgcn_global_load_lds(QG_GLOBAL_PTR(c.a + pa2 + lane4), QG_LDS_PTR(smem + buf_off + pa2), 4, 0, 0);
    };

    enum { S00, S11, P01, S22, P12, P02, NACC };
    v4i acc[NACC][3][2];
    // fragment of v_mfma_i32_16x16x64_i8: lane l holds row (l & 15), bytes [16 (l >> 4), +16) of the 64-byte k-step; LDS image:
    // 64-byte rows, chunk c of row r at slot c ^ qg_swz<64>(r); 48 wm + 16 i is a multiple of 16, so the slot is a lane constant
    const int fr = lane & 15, fq = lane >> 4;
    const int chunk = (fq ^ qg_swz<64>(fr)) * 16;
    const int a_lane = (wm * 48 + fr) * BK + chunk;
    const int b_lane = 3 * PLANE_A + (wn * 32 + fr) * BK + chunk;
    v4i fa[3][3], fb[3][2];   // [register set][tile]
    // the two LDS read addresses of the k-tile to come (buffer + a_lane, buffer + b_lane) are carried in registers: a wave moves
    // them on at the end of its MFMA interval, so that its LOAD interval holds no vector ALU instruction
    typedef const __attribute__((address_space(3))) v4i* LdsFrag;
    const uint32_t lds0 = (uint32_t)(uintptr_t)QG_LDS_PTR(smem);
    uint32_t rd_a = lds0 + a_lane, rd_b = lds0 + b_lane;
    auto read_ab = [&](int plane, int set) {
#pragma unroll
        for (int i = 0; i < 3; ++i) fa[set][i] = *(LdsFrag)(uintptr_t)(rd_a + plane * PLANE_A + i * (16 * BK));
#pragma unroll
        for (int j = 0; j < 2; ++j) fb[set][j] = *(LdsFrag)(uintptr_t)(rd_b + plane * PLANE_B + j * (16 * BK));
    };
    auto product = [&](int s, int set) {
#pragma unroll
        for (int i = 0; i < 3; ++i)
#pragma unroll
            for (int j = 0; j < 2; ++j) acc[s][i][j] = __builtin_amdgcn_mfma_i32_16x16x64_i8(fa[set][i], fb[set][j], acc[s][i][j], 0, 0, 0);
    };
#define QG_LOAD_DONE(WAIT)                                          \
    do {                                                            \
        WAIT;                                                       \
        asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");          \
        __builtin_amdgcn_sched_barrier(0);                          \
        __builtin_amdgcn_s_barrier();                               \
        __builtin_amdgcn_sched_barrier(0);                          \
    } while (0)
#define QG_MFMA_DONE()                                              \
    do {                                                            \
        __builtin_amdgcn_s_setprio(0);                              \
        __builtin_amdgcn_sched_barrier(0);                          \
        __builtin_amdgcn_s_barrier();                               \
        __builtin_amdgcn_sched_barrier(0);                          \
    } while (0)

    // prologue (once per workgroup): k-tiles 0 and 1 whole; k-tile 0 has landed when all but the 6 youngest pieces have
    Cursor nxt = cursor_at_tile(0);
    issue_tile(0, nxt);
    nxt = advance(nxt);
    issue_tile(BUF, nxt);
    nxt = advance(nxt);   // k-tile 2: the first one the loop issues
    asm volatile("s_waitcnt vmcnt(6)" ::: "memory");
    __builtin_amdgcn_s_barrier();
    asm volatile("" ::: "memory");

    int cur = 0, fill = 2 * BUF;   // buffer of this k-tile; buffer that takes k-tile kt+2
    for (int ti = 0; ti < n_my; ++ti) {
#pragma unroll
        for (int s = 0; s < NACC; ++s)
#pragma unroll
            for (int i = 0; i < 3; ++i)
#pragma unroll
                for (int j = 0; j < 2; ++j)
#pragma unroll
                    for (int e = 0; e < 4; ++e) acc[s][i][j][e] = 0;
        if (wm == 1) __builtin_amdgcn_s_barrier();   // group 1 runs one interval behind
        __builtin_amdgcn_sched_barrier(0);

        for (int kt = 0; kt < nk; ++kt) {
            asm volatile("" : "+v"(lane16), "+v"(lane4));   // (no instruction: keeps the zero-extension of the offsets in this block)
            read_ab(0, 0);
            read_ab(1, 1);
            read_ab(2, 2);
            issue_tile(fill, nxt);
            QG_LOAD_DONE(asm volatile("s_waitcnt vmcnt(6)" ::: "memory"));   // this wave's share of k-tile kt+1 is in
            __builtin_amdgcn_s_setprio(1);
            product(S00, 0);
            product(S11, 1);
            product(S22, 2);
            // the three sums in place, while the matrix pipe works on the plain products: d1 <- d1 + d2 (P12), then
            // d1 <- d1 + d0 - d2 = d0 + d1 (P01: at most 189 in a byte on the way, still no carry), then d0 <- d0 + d2 (P02)
#pragma unroll
            for (int i = 0; i < 3; ++i) fa[1][i] += fa[2][i];
#pragma unroll
            for (int j = 0; j < 2; ++j) fb[1][j] += fb[2][j];
            product(P12, 1);
#pragma unroll
            for (int i = 0; i < 3; ++i) fa[1][i] = fa[1][i] + fa[0][i] - fa[2][i];
#pragma unroll
            for (int j = 0; j < 2; ++j) fb[1][j] = fb[1][j] + fb[0][j] - fb[2][j];
            product(P01, 1);
#pragma unroll
            for (int i = 0; i < 3; ++i) fa[0][i] += fa[2][i];
#pragma unroll
            for (int j = 0; j < 2; ++j) fb[0][j] += fb[2][j];
            product(P02, 0);
            const int t = cur, step = cur + BUF == NBUF * BUF ? -(NBUF - 1) * BUF : BUF;
            cur += step;
            fill = t;
            rd_a += step;
            rd_b += step;
            asm volatile("" : "+v"(rd_a), "+v"(rd_b));   // formed here, beside the last MFMAs, and nowhere else
            paced_valu_hint<31, 2, 5>();
            QG_MFMA_DONE();
            nxt = advance(nxt);
        }
        if (wm == 0) __builtin_amdgcn_s_barrier();   // pairs with group 1's last barrier: both groups are level again
        __builtin_amdgcn_sched_barrier(0);

        // epilogue: recombine the six sums into 64 bits, take the biases out with the row sums, one round + overflow, stores of 4
        // consecutive rows.  C/D of the 16x16 MFMA: col = lane & 15, rows 4 (lane >> 4) + e; packed C is column-major inside the tile
        int tile_m, tile_n;
        qg_tile_of<8>(my.first + ti * my.step, tiles_m, tiles_n, tile_m, tile_n);
        const QStep st = g.to_c;
        char* C = (char*)g.C;
        // packed C keeps the 128 x 128 tiling of every other limb plan (QCGeom), whatever A's row-tile pitch: a run of 4 rows lies in
        // one of its tiles; rows beyond its padded extent g.Mc (the tail of A's last 96-row tile) are not stored
        constexpr int CT = 128;
        [[maybe_unused]] const int sh = st.d;
        // The recombination in 32-bit pieces.  Every accumulator is a sum of K products of two bytes <= 126, and the planner admits
        // the form only for K * 126^2 < 2^31: all six are non-negative int32.  The Karatsuba differences are sums of digit products
        // themselves — c1 = sum d0 e1 + d1 e0 <= 2 K 63^2, c2 = sum d0 e2 + d1 e1 + d2 e0 <= 3 K 63^2, c3 = sum d1 e2 + d2 e1
        // <= 2 K 63^2, and 3 K 63^2 = 3/4 K 126^2 < 2^31 — so wrapping 32-bit subtraction gives them exactly and they zero-extend.
        // What depends on the column alone (corr - biasA rsB[col]) is formed once per column of the lane, what depends on the row
        // alone (biasB rsA[row]) once per row; the 64-bit sums are modulo 2^64, as they were.
        // Every row sum the lane needs — 2 of B, 12 of A — is loaded here as one batch (the fragment registers are dead) and turned
        // into its term ahead of the first store of C: one round trip per tile, and no later wait that a store has to satisfy.
        // The wait itself is vmcnt(0), not a counted one: vector memory operations return in order and these loads are the youngest,
        // so it also drains the 12 DMA pieces already issued for the next tile.  That is once per tile, where it was three times.
        uint64_t colt[2], rowt[3][4];
#pragma unroll
        for (int j = 0; j < 2; ++j) colt[j] = (uint64_t)g.rsB[(int64_t)tile_n * TN + wn * 32 + j * 16 + fr];
#pragma unroll
        for (int i = 0; i < 3; ++i)
#pragma unroll
            for (int e = 0; e < 4; ++e) rowt[i][e] = (uint64_t)g.rsA[(int64_t)tile_m * TM + wm * 48 + i * 16 + 4 * fq + e];
#pragma unroll
        for (int j = 0; j < 2; ++j) colt[j] = (uint64_t)g.corr - (uint64_t)g.biasA * colt[j];
#pragma unroll
        for (int i = 0; i < 3; ++i)
#pragma unroll
            for (int e = 0; e < 4; ++e) rowt[i][e] = (uint64_t)g.biasB * rowt[i][e];
#pragma unroll
        for (int i = 0; i < 3; ++i) {
            int64_t s[8];
#pragma unroll
            for (int j = 0; j < 2; ++j)
#pragma unroll
                for (int e = 0; e < 4; ++e) {
                    const uint32_t s00 = (uint32_t)acc[S00][i][j][e], s11 = (uint32_t)acc[S11][i][j][e], s22 = (uint32_t)acc[S22][i][j][e];
                    const uint32_t c1 = (uint32_t)acc[P01][i][j][e] - s00 - s11, c3 = (uint32_t)acc[P12][i][j][e] - s11 - s22,
                                   c2 = (uint32_t)acc[P02][i][j][e] - s00 - s22 + s11;
                    s[j * 4 + e] = (int64_t)k6_recombine(s00, c1, c2, c3, s22, colt[j] - rowt[i][e]);
                }
            if constexpr (FAST) {
#pragma unroll
                for (int o = 0; o < 8; ++o) {
                    const int64_t x = s[o] >> sh, y = x < st.lo ? st.lo : x;
                    s[o] = y > st.hi ? st.hi : y;
                }
            } else {
                qg_step_all<int64_t, 8>(s, st);
            }
            const int row0 = wm * 48 + i * 16 + 4 * fq;
#pragma unroll
            for (int j = 0; j < 2; ++j) {
                const int col = wn * 32 + j * 16 + fr;
                const int64_t* q = s + j * 4;
                if (g.c_host) {   // the reference layout itself (wave-uniform choice): element (r, c) at r + c * ld.  (Written out in each of
                    // k_mfma_pp, k_mfma_ppl and k_mfma_k6: as a shared function it moves every one of their instruction streams)
                    const int64_t gr = (int64_t)tile_m * TM + row0, gc = (int64_t)tile_n * TN + col;
                    if (gc < g.c_N) {
                        using E = std::conditional_t<CB == 4, int32_t, int64_t>;
                        E* dst = (E*)C + gc * g.c_ld + gr;
                        if (gr + 3 < g.c_M && g.c_vec) {
                            if constexpr (CB == 4) *(int4*)dst = make_int4((int)q[0], (int)q[1], (int)q[2], (int)q[3]);
                            else { *(longlong2*)dst = make_longlong2(q[0], q[1]); *(longlong2*)(dst + 2) = make_longlong2(q[2], q[3]); }
                        } else {
#pragma unroll
                            for (int e = 0; e < 4; ++e)
                                if (gr + e < g.c_M) dst[e] = (E)q[e];
                        }
                    }
                    continue;
                }
                const int64_t gr = (int64_t)tile_m * TM + row0;
                if (gr >= g.Mc) continue;
                const int64_t base = (((gr / CT) * tiles_n + tile_n) * CT + col) * CT + gr % CT;
                qg_store_run4<CB>(C, base, q);
            }
        }
    }
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");   // the clamped refills must land before the LDS is handed on
#undef QG_LOAD_DONE
#undef QG_MFMA_DONE
}

template <bool FAST, int CB>
hipError_t launch_k6(const QMfmaArgs& a, unsigned grid, hipStream_t st)
{
    return qg_launch_lds<k_mfma_k6<FAST, CB>>(grid, 512, NBUF * BUF, st, a);
}

} // namespace

bool qg_mfma_k6_applies(const QMfmaArgs& a)
{
    if (a.has_ep || !a.kara || a.variant != QG_MFMA_K6 || !a.rsA || !a.rsB) return false;
    if (a.cbytes != 4 && a.cbytes != 8) return false;
    return a.Kp > 0 && a.Kp % BK == 0 && a.Mp % TM == 0 && a.Np % TN == 0 && a.Mc > 0 && a.Mc % 128 == 0 && a.Mc <= a.Mp + 127;
}

hipError_t qg_launch_mfma_k6(const QMfmaArgs& a, hipStream_t st)
{
    if (!qg_mfma_k6_applies(a)) return hipErrorInvalidValue;   // (the packed layout belongs to this kernel alone: no other takes it)
    const int64_t blocks = (a.Mp / TM) * (a.Np / TN);
    if (blocks <= 0) return hipSuccess;
    if (blocks > 0x7fffffffll) return hipErrorInvalidValue;
    unsigned grid = 0;
    if (hipError_t e = qg_persistent_grid(blocks, &grid); e != hipSuccess) return e;
    const bool fast = qg_step_is_shift_clamp(a.to_c);
    if (a.cbytes == 4) return fast ? launch_k6<true, 4>(a, grid, st) : launch_k6<false, 4>(a, grid, st);
    return fast ? launch_k6<true, 8>(a, grid, st) : launch_k6<false, 8>(a, grid, st);
}
