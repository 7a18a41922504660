// qg_mfma_ep_grp.hip — the grouped form of the lock-step MFMA kernel (k_mfma_grp, qg_mfma_grp.hip) with the element-wise chain of a
// grouped plan in its epilogue: ONE launch computes  D_g = chain_g(Qgemul(A_g, B_g))  for every member g in the launch (gfx950).
//
// k_mfma_ep_grp is the body of k_mfma (qg_mfma_body.h) with GRP and EP together: the record load and the main loop of k_mfma_grp, the
// epilogue of k_mfma's fused variants.  What is new sits in the epilogue only.  D and the tensor operands are the members' packed
// tensors back to back, so they are read and written at the element index the body computes from the record's c_off, which is the
// launch-wide one already.  A per-member scalar stage takes  table[k][rec.member]  (QGrpEp, qg_eltwise_args.h: a table of the plan, one raw
// value per member of the caller's list); the record is loaded at a wave-uniform address and so is the table entry, nothing per lane
// depends on the member.  Chains the planner has bounded by 32-bit arithmetic only (QEpTable::bits32), as for every fused variant.
// The kernels live in this file, under this name: tests/test_grouped_resources.py pins the ten grouped instantiations of
// qg_mfma_grp.hip by name and by count, tests/test_batched_resources.py the block-diagonal ones of qg_mfma.hip.
#include <hip/hip_runtime.h>
#include <stdlib.h>

#include <utility>

#include "qg_eltwise.h"
#include "qg_kernels.h"
#include "qg_mfma_tile.h"
#include "qg_step_all.h"

namespace {

typedef int v16i __attribute__((ext_vector_type(16)));

// template parameters: those of k_mfma_bd
template <int LA, int LB, int BK, int WGM, int WGN, int TI, int TJ, int NSTAGE, int SA = LA, int SB = LB>
__global__ __launch_bounds__(64 * WGM * WGN) void k_mfma_ep_grp(QMfmaEpGrpArgs g)
{
    constexpr int ABL = 0, KS = 1;
    constexpr bool EP = true, KARA = false, BD = false, GRP = true;
#include "qg_mfma_body.h"
}

// n_tiles workgroups; a 3 x 3 launch is the pair <3,3> + <2,2 on 3-plane storage> of launch_grp (qg_mfma_grp.hip), and both partners
// carry the chain as in launch_ep_bd: the one the launch's plane masks (the OR over every member) select stores D
template <int LA, int LB, int BK, int WGM, int WGN, int TI, int TJ, int NSTAGE>
hipError_t launch_ep_grp(const QMfmaEpGrpArgs& a, int64_t n_tiles, hipStream_t st)
{
    constexpr int TM = WGM * TI * 32, TN = WGN * TJ * 32;
    constexpr int STAGE = (LA * TM + LB * TN) * BK;
    if (n_tiles <= 0) return hipSuccess;
    if (n_tiles > 0x7fffffffll || !a.tiles || !a.has_ep || !a.ep.bits32 || a.kara || a.c_host) return hipErrorInvalidValue;
    const hipError_t e = qg_launch_lds<k_mfma_ep_grp<LA, LB, BK, WGM, WGN, TI, TJ, NSTAGE>>((unsigned)n_tiles, 64 * WGM * WGN, NSTAGE * STAGE, st, a);
    if constexpr (LA == 3 && LB == 3) {
        if (e == hipSuccess && (a.maskA || a.maskB))
            return qg_launch_lds<k_mfma_ep_grp<2, 2, BK, WGM, WGN, TI, TJ, NSTAGE, 3, 3>>((unsigned)n_tiles, 64 * WGM * WGN, NSTAGE * (2 * TM + 2 * TN) * BK, st, a);
    }
    return e;
}

} // namespace

hipError_t qg_launch_mfma_ep_grp(int LA, int LB, const QMfmaEpGrpArgs& a, int64_t n_tiles, hipStream_t st)
{
    if (LA == 1 && LB == 1) {
        if (a.variant == QG_MFMA_64_BK128) return launch_ep_grp<1, 1, 128, 2, 2, 1, 1, 3>(a, n_tiles, st);
        return hipErrorInvalidValue;
    }
    if (a.variant != QG_MFMA_LIMB_64) return hipErrorInvalidValue;
    switch (LA * 10 + LB) {
    case 12: return launch_ep_grp<1, 2, 64, 2, 2, 1, 1, 3>(a, n_tiles, st);
    case 21: return launch_ep_grp<2, 1, 64, 2, 2, 1, 1, 3>(a, n_tiles, st);
    case 22: return launch_ep_grp<2, 2, 64, 2, 2, 1, 1, 3>(a, n_tiles, st);
    case 13: return launch_ep_grp<1, 3, 64, 2, 2, 1, 1, 3>(a, n_tiles, st);
    case 31: return launch_ep_grp<3, 1, 64, 2, 2, 1, 1, 3>(a, n_tiles, st);
    case 23: return launch_ep_grp<2, 3, 64, 2, 2, 1, 1, 3>(a, n_tiles, st);
    case 32: return launch_ep_grp<3, 2, 64, 2, 2, 1, 1, 3>(a, n_tiles, st);
    case 33: return launch_ep_grp<3, 3, 64, 2, 2, 1, 1, 3>(a, n_tiles, st);
    default: return hipErrorInvalidValue;
    }
}
