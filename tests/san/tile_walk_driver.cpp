// Prints what qublas_amd/csrc/qg_tile_walk.h computes, for tests/test_tile_walk.py to compare with its own restatement.  Host compiler
// only (no HIP), built with -fsanitize=address,undefined.
//   swz  r  qg_swz<64>(r)  qg_swz<128>(r)  qg_swz(64, r)  qg_swz(128, r)                       r = 0 .. 255
//   walk GM MOD tiles_m tiles_n : tile_m * 64 + tile_n of block 0 .. nwg - 1                    GM 8: int, GM 16: int64_t
//   list tiles_m tiles_n grid : first step count of workgroup 0 .. grid - 1
#include <stdint.h>
#include <stdio.h>

#include "../../qublas_amd/csrc/qg_tile_walk.h"

template <int GM, bool MOD, class I>
static void walk(I tiles_m, I tiles_n)
{
    const I nwg = tiles_m * tiles_n;
    printf("walk %d %d %d %d :", GM, MOD ? 1 : 0, (int)tiles_m, (int)tiles_n);
    for (I bid = 0; bid < nwg; ++bid) {
        I tm = -1, tn = -1;
        qg_tile_of<GM, MOD>(qg_xcd_block<I>(bid, nwg), tiles_m, tiles_n, tm, tn);
        printf(" %d", (int)(tm * 64 + tn));
    }
    printf("\n");
}

int main()
{
    for (int r = 0; r < 256; ++r) printf("swz %d %d %d %d %d\n", r, qg_swz<64>(r), qg_swz<128>(r), qg_swz(64, r), qg_swz(128, r));
    const unsigned grids[] = {8, 16, 24, 256, 304};
    for (int tiles_m = 1; tiles_m <= 40; ++tiles_m)
        for (int tiles_n = 1; tiles_n <= 40; ++tiles_n) {
            walk<8, false, int>(tiles_m, tiles_n);
            walk<8, true, int>(tiles_m, tiles_n);
            walk<16, false, int64_t>(tiles_m, tiles_n);
            walk<16, true, int64_t>(tiles_m, tiles_n);
            for (unsigned grid : grids) {
                printf("list %d %d %u :", tiles_m, tiles_n, grid);
                for (unsigned b = 0; b < grid; ++b) {
                    const QTileList l = qg_tile_list(tiles_m * tiles_n, QDimX{b}, QDimX{grid});
                    printf(" %d %d %d", l.first, l.step, l.count);
                }
                printf("\n");
            }
        }
    return 0;
}
