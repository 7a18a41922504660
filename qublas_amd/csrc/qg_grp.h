// qg_grp.h — the host-side schedule of a grouped launch (grouped Qgemul: GEMMs of different shapes in ONE launch of k_mfma_grp,
// qg_mfma_grp.hip).  Plain functions of integers, no HIP header, so that a host compiler builds them alone
// (tests/san/grouped_schedule_driver.cpp; tests/test_grouped_schedule.py pins the table against a restatement).
//
// A lock-step workgroup's time is proportional to its k-tile count and the members of a group differ in it, so the HOST is the
// scheduler: one 48-byte record per workgroup, built at plan creation, uploaded once, owned by the plan.  Block `bid` reads record
// `bid` and finds there everything that the plain kernel derives from its block id with divisions: where its A and B blocks start,
// where its C tile goes, how many k-tiles it walks, which row sums are its own and the member's K biasA biasB.
//
// Correctness does not depend on the order of the records, speed does.
//   QG_GRP_DEALT (the default):
//     * members sorted by decreasing k-tile count, ties by list index; each member's tiles in the order qg_tile_of<8, true> walks
//       them: the SEQUENCE;
//     * the sequence is cut into chunks of 8 consecutive tiles (a chunk shares A rows wherever the member has 8 tile rows), and
//       the chunks are dealt round-robin to the eight residue classes of the block id (bid and bid + 8 share an XCD and its L2:
//       qg_tile_walk.h): chunk c goes to class c % 8, and inside a class the block ids follow the sequence, so that the long
//       k-loops of every XCD start first and the short ones fill in behind them;
//     * LEFTOVER RULE.  Only whole rounds of 8 chunks are dealt: with T tiles, the first 64 * (T / 64) tiles of the sequence.  They
//       fill the block ids below 64 * (T / 64) exactly, every class alike.  The tail of the sequence (fewer than 64 tiles, the
//       shortest k-loops of the launch) takes the remaining block ids in sequence order, tail tile i -> block 64 * (T / 64) + i.
//       So the table is a bijection onto the tiles, along every class's block ids nk never increases, and the 8 tiles of every
//       dealt chunk sit in one class; the tiles of the tail do not (with fewer than 64 tiles left there is no such placement
//       without empty records).
//   QG_GRP_MEMBER (diagnostic library only: QG_GRP_MEMBER_ORDER): the tiles in list order through qg_xcd_block, as the batched
//     walk (qg_bd_tile_of) takes them.
// The rule for the order was fixed before anything was measured: dealt order stays the default unless member order's maximum is below
// dealt order's minimum at every measured point.  Measured (tools/measure_grouped.py, profiles/grouped_measure.jsonl, DESIGN.md
// section 9; us per group, dealt / member): int<4,3> 256 random members 29 / 26, 1024 random 125 / 130, 1000 short + 24 long members
// 22 / 45; int<8,8> 88 / 116, 410 / 408, 68 / 198.  Member order wins at one point of six: DEALT ORDER STAYS THE DEFAULT.
#pragma once
#include <stdint.h>

#include "qg_tile_walk.h"

struct QGrpTile {
    int64_t a_off, b_off;   // bytes from packed A / B to this tile's first (row tile, k-tile) block
    int64_t c_off;          // elements from packed C to this tile
    int64_t corr;           // K_g * biasA * biasB (wrapping), centred operands
    int32_t nk;             // this member's k-tiles
    int32_t row_a, row_b;   // first stack row of the tile, for the row sums
    int32_t member;
};
static_assert(sizeof(QGrpTile) == 48, "one 48-byte record per workgroup");

// what the schedule needs to know of a member in the launch
struct QGrpShape {
    int64_t a_off, b_off;   // bytes from packed A / B to the member's first block (multiples of 1024)
    int64_t c_off;          // elements from packed C to the member's first tile
    int64_t corr;
    int64_t a_blk, b_blk;   // bytes of one stored (row tile, k-tile) block of A / B: stored planes * tile rows * k-tile bytes
    int64_t c_tile;         // elements of one C tile
    int32_t tiles_m, tiles_n, nk;
    int32_t row_a, row_b;   // first stack row of the member
    int32_t tm, tn;         // tile rows of A / B
    int32_t member;         // index in the caller's list
};

enum { QG_GRP_DEALT = 0, QG_GRP_MEMBER = 1 };

inline int64_t qg_grp_tiles(const QGrpShape* m, int64_t n)
{
    int64_t t = 0;
    for (int64_t g = 0; g < n; ++g) t += (int64_t)m[g].tiles_m * m[g].tiles_n;
    return t;
}

// tile number w (qg_tile_of<8, true>) of member s
inline QGrpTile qg_grp_record(const QGrpShape& s, int32_t w)
{
    int32_t lm, ln;
    qg_tile_of<8, true, int32_t>(w, s.tiles_m, s.tiles_n, lm, ln);
    QGrpTile t;
    t.a_off = s.a_off + (int64_t)lm * s.nk * s.a_blk;
    t.b_off = s.b_off + (int64_t)ln * s.nk * s.b_blk;
    t.c_off = s.c_off + ((int64_t)lm * s.tiles_n + ln) * s.c_tile;
    t.corr = s.corr;
    t.nk = s.nk;
    t.row_a = s.row_a + lm * s.tm;
    t.row_b = s.row_b + ln * s.tn;
    t.member = s.member;
    return t;
}

// The chain pass of a grouped plan with an element-wise chain (k_eltwise_grp, qg_eltwise.hip; k_approx_grp, qg_approx.hip) walks the launch's
// packed C linearly, one 64 x 64 tile per workgroup, and must know whose per-member scalars a tile takes: out[w] = the member (index
// in the caller's list) of C tile w IN MEMORY ORDER, w = c_off / c_tile, 4 bytes per workgroup.  out[T], T = qg_grp_tiles(m, n); the
// members' C tiles are disjoint and cover [0, T) (the planner lays them back to back), so every entry is written exactly once.
inline void qg_grp_tile_members(const QGrpShape* m, int64_t n, int32_t* out)
{
    for (int64_t g = 0; g < n; ++g) {
        const int64_t w0 = m[g].c_off / m[g].c_tile, cnt = (int64_t)m[g].tiles_m * m[g].tiles_n;
        for (int64_t w = 0; w < cnt; ++w) out[w0 + w] = m[g].member;
    }
}

// out[T], T = qg_grp_tiles(m, n) < 2^31; order[n] is scratch of the caller (member indices).  Members without tiles take none.
inline void qg_grp_schedule(const QGrpShape* m, int64_t n, int mode, int64_t* order, QGrpTile* out)
{
    const int64_t T = qg_grp_tiles(m, n);
    for (int64_t g = 0; g < n; ++g) order[g] = g;
    if (mode == QG_GRP_DEALT) {
        // decreasing nk, ties in list order: a bottom-up merge sort of the index array (the right run wins only when strictly longer)
        int64_t* tmp = new int64_t[n > 0 ? n : 1];
        for (int64_t w = 1; w < n; w *= 2) {
            for (int64_t lo = 0; lo < n; lo += 2 * w) {
                const int64_t mid = lo + w < n ? lo + w : n, hi = lo + 2 * w < n ? lo + 2 * w : n;
                int64_t i = lo, j = mid, k = lo;
                while (i < mid && j < hi) tmp[k++] = m[order[j]].nk > m[order[i]].nk ? order[j++] : order[i++];
                while (i < mid) tmp[k++] = order[i++];
                while (j < hi) tmp[k++] = order[j++];
            }
            for (int64_t i = 0; i < n; ++i) order[i] = tmp[i];
        }
        delete[] tmp;
    }
    const int64_t dealt = T / 64 * 64;   // whole rounds of 8 chunks of 8 tiles
    int64_t s = 0;                       // position in the sequence
    for (int64_t q = 0; q < n; ++q) {
        const QGrpShape& sh = m[order[q]];
        const int32_t cnt = sh.tiles_m * sh.tiles_n;
        for (int32_t w = 0; w < cnt; ++w, ++s) {
            int64_t bid;
            if (mode == QG_GRP_DEALT) {
                const int64_t chunk = s / 8, e = s % 8;
                bid = s < dealt ? chunk % 8 + 8 * (chunk / 8 * 8 + e) : s;
            } else {
                // block bid works on tile number qg_xcd_block(bid, T): the inverse, class by class
                int64_t x = 0;
                while (x < 7 && qg_xcd_run_start<int64_t>(T, x + 1) <= s) ++x;
                bid = x + 8 * (s - qg_xcd_run_start<int64_t>(T, x));
            }
            out[bid] = qg_grp_record(sh, w);
        }
    }
}
