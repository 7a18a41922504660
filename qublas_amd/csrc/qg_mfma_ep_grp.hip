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
#include "qg_member_forms.h"
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

} // namespace

// n_tiles workgroups, the forms and the 3 x 3 pair of qg_member_forms.h; both partners carry the chain
hipError_t qg_launch_mfma_ep_grp(int LA, int LB, const QMfmaEpGrpArgs& a, int64_t n_tiles, hipStream_t st)
{
    return qg_member_form(LA, LB, a.variant, [&](auto form) -> hipError_t {
        if (n_tiles <= 0) return hipSuccess;
        if (n_tiles > 0x7fffffffll || !a.tiles || !a.has_ep || !a.ep.bits32 || a.kara || a.c_host) return hipErrorInvalidValue;
        return qg_member_launch(form, a, [&](auto k) {
            using K = decltype(k);
            return qg_launch_lds<k_mfma_ep_grp<QG_MEMBER_FORM_ARGS(K)>>((unsigned)n_tiles, K::THREADS, K::LDS, st, a);
        });
    });
}
