// Prints the two walks of a stacked batched plan (QG_OPT_BATCHED_STACKED) from qublas_amd/csrc/qg_tile_walk.h, for
// tests/test_batched_stacked_plan.py: the block-diagonal GEMM launch's (qg_bd_tile_of over the member block's bd_tm x bd_tn tiles, fed
// from qg_xcd_block as k_mfma_bd calls it) and the combine pass's (qg_bd_tile_of over the tm x tn tiles of one part straight from the
// block id, then qg_stack_src_tile, as k_stack_combine_bd calls them).  Host compiler only, built with -fsanitize=address,undefined.
//   gemm mode tm tn batch : workspace tile number of block 0 .. batch * bd_tm * bd_tn - 1
//   comb mode tm tn batch : per block: member lm ln, then per part its source tiles' workspace tile numbers (complex: 2 + 2; mixed: 1 + 1)
// mode: QStackMode (1 complex, 2 real x complex, 3 complex x real)
#include <stdio.h>

#include "../../qublas_amd/csrc/qg_tile_walk.h"

int main()
{
    const int batches[] = {1, 2, 9};
    const int rows[] = {1, 2, 3, 8, 9, 17};   // part tile rows of a member: the doubled counts cross the walk's groups of 8 at 4, 8 and 9
    const int cols[] = {1, 2, 3, 5};
    for (int mode = 1; mode <= 3; ++mode)
        for (int tm : rows)
            for (int tn : cols)
                for (int batch : batches) {
                    const bool cplx = mode == 1;
                    const int im_r = mode == 3 ? tm : 0, im_c = mode == 2 ? tn : 0;
                    const int bd_tm = cplx ? 2 * tm : tm + im_r, bd_tn = cplx ? 2 * tn : tn + im_c;
                    const int nwg = batch * bd_tm * bd_tn;
                    printf("gemm %d %d %d %d :", mode, tm, tn, batch);
                    for (int bid = 0; bid < nwg; ++bid) {
                        int member = -1, lm = -1, ln = -1;
                        qg_bd_tile_of<int>(qg_xcd_block<int>(bid, nwg), bd_tm, bd_tn, member, lm, ln);
                        printf(" %lld", ((long long)member * bd_tm + lm) * bd_tn + ln);
                    }
                    printf("\ncomb %d %d %d %d :", mode, tm, tn, batch);
                    for (int bid = 0; bid < batch * tm * tn; ++bid) {
                        int member = -1, lm = -1, ln = -1;
                        qg_bd_tile_of<int>(bid, tm, tn, member, lm, ln);
                        printf(" %d %d %d", member, lm, ln);
                        for (int part = 0; part < 2; ++part)
                            for (int k = 0; k < (cplx ? 2 : 1); ++k) {
                                int r = -1, c = -1;
                                qg_stack_src_tile(cplx, part, k, lm, ln, tm, tn, im_r, im_c, r, c);
                                printf(" %lld", ((long long)member * bd_tm + r) * bd_tn + c);
                            }
                    }
                    printf("\n");
                }
    return 0;
}
