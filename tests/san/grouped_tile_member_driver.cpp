// Builds the tile -> member table of a grouped chain's pass (qublas_amd/csrc/qg_grp.h: qg_grp_tile_members) next to the schedule
// (qg_grp_schedule) on the host (g++ -fsanitize=address,undefined: tests/test_grouped_ep_table.py) for swept groups and prints, per
// group, the members, the table and every record's (c_off, member) as one JSON line.  Tile counts per member are drawn from {0x1
// (an empty member), 1x1, 2x1, 3x3, 9x2, 17x5}, k-tile counts from {1, 2, 3, 8, 1024}, group sizes are 1, 2, 7, 8, 9 and 300; the
// member numbers are list indices with gaps (the stragglers of a real group are not in the launch).
#include <cstdint>
#include <cstdio>
#include <vector>

#include "../../qublas_amd/csrc/qg_grp.h"

int main()
{
    static const int TILES[6][2] = {{0, 1}, {1, 1}, {2, 1}, {3, 3}, {9, 2}, {17, 5}};
    static const int NK[5] = {1, 2, 3, 8, 1024};
    static const int SIZES[6] = {1, 2, 7, 8, 9, 300};
    const int64_t A_BLK = 2 * 64 * 64, B_BLK = 3 * 64 * 64, C_TILE = 64 * 64;
    uint64_t x = 0x2545f4914f6cdd1dull;
    auto draw = [&](int n) { x = x * 6364136223846793005ull + 1442695040888963407ull; return (int)((x >> 33) % (uint64_t)n); };
    for (int si = 0; si < 6; ++si)
        for (int rep = 0; rep < 4; ++rep) {
            const int n = SIZES[si];
            std::vector<QGrpShape> m((size_t)n);
            int64_t a = 0, b = 0, c = 0;
            int32_t ra = 0, rb = 0, member = 0;
            for (int g = 0; g < n; ++g) {
                const int t = rep == 0 ? (g + 1) % 6 : draw(6), k = rep == 0 ? (g / 5 + g) % 5 : draw(5);
                QGrpShape& s = m[(size_t)g];
                s.tiles_m = TILES[t][0];
                s.tiles_n = TILES[t][1];
                s.nk = NK[k];
                s.a_off = a; s.b_off = b; s.c_off = c;
                s.corr = 0;
                s.a_blk = A_BLK; s.b_blk = B_BLK; s.c_tile = C_TILE;
                s.row_a = ra; s.row_b = rb;
                s.tm = 64; s.tn = 64;
                member += 1 + (rep > 1 ? draw(3) : 0);   // (gaps: list indices of the members in the launch)
                s.member = member;
                a += (int64_t)s.tiles_m * s.nk * A_BLK;
                b += (int64_t)s.tiles_n * s.nk * B_BLK;
                c += (int64_t)s.tiles_m * s.tiles_n * C_TILE;
                ra += s.tiles_m * 64;
                rb += s.tiles_n * 64;
            }
            const int64_t T = qg_grp_tiles(m.data(), n);
            std::vector<QGrpTile> sched((size_t)T);
            std::vector<int64_t> order((size_t)n);
            std::vector<int32_t> table((size_t)T, -1);
            qg_grp_schedule(m.data(), n, QG_GRP_DEALT, order.data(), sched.data());
            qg_grp_tile_members(m.data(), n, table.data());
            std::printf("{\"members\":[");
            for (int g = 0; g < n; ++g) std::printf("%s[%d,%d,%d]", g ? "," : "", m[(size_t)g].tiles_m, m[(size_t)g].tiles_n, m[(size_t)g].member);
            std::printf("],\"table\":[");
            for (int64_t i = 0; i < T; ++i) std::printf("%s%d", i ? "," : "", table[(size_t)i]);
            std::printf("],\"schedule\":[");
            for (int64_t i = 0; i < T; ++i) std::printf("%s[%lld,%d]", i ? "," : "", (long long)sched[(size_t)i].c_off, sched[(size_t)i].member);
            std::printf("]}\n");
        }
    return 0;
}
