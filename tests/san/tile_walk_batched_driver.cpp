// Prints qg_bd_tile_of (qublas_amd/csrc/qg_tile_walk.h) fed from qg_xcd_block over a batch's total tile count, as k_mfma's
// block-diagonal form calls it, for tests/test_tile_walk_batched.py.  Host compiler only, built with -fsanitize=address,undefined.
//   bd tmM tnN batch : member tile_m tile_n of block 0 .. batch * tmM * tnN - 1
#include <stdio.h>

#include "../../qublas_amd/csrc/qg_tile_walk.h"

int main()
{
    const int batches[] = {1, 2, 7, 8, 9, 300};
    const int rows[] = {1, 2, 3, 8, 9, 10, 17};   // tile rows of a member: below, on and beyond the walk's groups of 8, ragged last groups
    const int cols[] = {1, 2, 3, 5};
    for (int tmM : rows)
        for (int tnN : cols)
            for (int batch : batches) {
                const int nwg = batch * tmM * tnN;
                printf("bd %d %d %d :", tmM, tnN, batch);
                for (int bid = 0; bid < nwg; ++bid) {
                    int member = -1, tm = -1, tn = -1;
                    qg_bd_tile_of<int>(qg_xcd_block<int>(bid, nwg), tmM, tnN, member, tm, tn);
                    printf(" %d %d %d", member, tm, tn);
                }
                printf("\n");
            }
    return 0;
}
