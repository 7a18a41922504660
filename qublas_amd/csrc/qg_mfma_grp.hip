// qg_mfma_grp.hip — grouped Qgemul: GEMMs of DIFFERENT shapes (M, N, K, transA) of one launch key in ONE launch of the lock-step MFMA
// kernel (gfx950).
//
// k_mfma_grp is the body of k_mfma (qg_mfma_body.h) with GRP: the k-loop, the LDS ring, the fragments, the MFMAs and the epilogue's
// conversion are the body's own.  What differs is where a workgroup finds its work.  The plain kernel and the block-diagonal one
// (k_mfma_bd) derive tile, operand blocks and k-loop length from the block id and from uniform arguments, which is only possible
// while every workgroup shares one tile count and one k-loop length.  Here block bid reads record bid of a table the host built at
// plan creation (qg_grp.h: QGrpTile, 48 bytes): byte offsets of its first A and B blocks, the element offset of its C tile, its
// k-tile count, its rows of the stack's row sums and its member's K biasA biasB.  The table is const and read-only, the load is
// wave-uniform; no division and no tile walk happen in the kernel.  The order of the records is the host's schedule.
// What every workgroup shares travels in QMfmaArgs as before: the limb counts and stored planes (template parameters), the k-tile
// size, the centres of A and B, C's container and the one conversion into C — the launch key of the planner (qg_geom.cpp).
// The kernels live in this file, under this name: tests/test_batched_resources.py pins the block-diagonal instantiations of
// qg_mfma.hip by name and by count.
#include <hip/hip_runtime.h>
#include <stdlib.h>

#include <utility>

#include "qg_eltwise.h"
#include "qg_kernels.h"
#include "qg_member_forms.h"
#include "qg_mfma_tile.h"
#include "qg_step_all.h"

namespace {

typedef int v16i __attribute__((ext_vector_type(16)));

// template parameters: those of k_mfma_bd
template <int LA, int LB, int BK, int WGM, int WGN, int TI, int TJ, int NSTAGE, int SA = LA, int SB = LB>
__global__ __launch_bounds__(64 * WGM * WGN) void k_mfma_grp(QMfmaGrpArgs g)
{
    constexpr int ABL = 0, KS = 1;
    constexpr bool EP = false, KARA = false, BD = false, GRP = true;
#include "qg_mfma_body.h"
}

} // namespace

// n_tiles workgroups, the forms and the 3 x 3 pair of qg_member_forms.h: both partners read the same records (the stored stride of a
// block is SA-based, and the host computed the offsets from the stored planes), and the plane masks they choose by are the launch's
hipError_t qg_launch_mfma_grp(int LA, int LB, const QMfmaGrpArgs& a, int64_t n_tiles, hipStream_t st)
{
    return qg_member_form(LA, LB, a.variant, [&](auto form) -> hipError_t {
        if (n_tiles <= 0) return hipSuccess;
        if (n_tiles > 0x7fffffffll || !a.tiles || a.has_ep || a.kara || a.c_host) return hipErrorInvalidValue;
        return qg_member_launch(form, a, [&](auto k) {
            using K = decltype(k);
            return qg_launch_lds<k_mfma_grp<QG_MEMBER_FORM_ARGS(K)>>((unsigned)n_tiles, K::THREADS, K::LDS, st, a);
        });
    });
}
