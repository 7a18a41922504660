// qg_mfma_ep_bd.hip — the block-diagonal form of the lock-step MFMA kernel (k_mfma_bd, qg_mfma.hip) with the element-wise chain of a
// batched plan in its epilogue: ONE launch computes  D_b = chain(Qgemul(A_b, B_b))  for every member b (gfx950).
//
// k_mfma_ep_bd is the body of k_mfma (qg_mfma_body.h) with BD and EP together: the tile walk and the main loop of k_mfma_bd, the
// epilogue of k_mfma's fused variants.  What is new sits in the epilogue only: D and the per-member tensor operands are read and
// written at the stack-wide element index the body computes from the workgroup's tile of the batch, a SHARED operand (one M x N
// tensor for every member: a bias) at that index minus  member * (elements of one member's packed C).  The member size and the
// shared mask travel in QMfmaEpBdArgs (qg_kernels.h), an argument struct of this kernel alone.  Chains the planner has bounded by
// 32-bit arithmetic only (QEpTable::bits32), as for every fused variant.
// The kernels live in this file, under this name, because tests/test_batched_resources.py pins the ten k_mfma_bd instantiations of
// qg_mfma.hip by name and by count.
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
__global__ __launch_bounds__(64 * WGM * WGN) void k_mfma_ep_bd(QMfmaEpBdArgs g)
{
    constexpr int ABL = 0, KS = 1;
    constexpr bool EP = true, KARA = false, BD = true, GRP = false;
#include "qg_mfma_body.h"
}

// batch * bd_tm * bd_tn workgroups; a 3 x 3 launch is the pair <3,3> + <2,2 on 3-plane storage> of launch_bd (qg_mfma.hip), and
// both partners carry the chain: the one the stack's plane masks select stores D
template <int LA, int LB, int BK, int WGM, int WGN, int TI, int TJ, int NSTAGE>
hipError_t launch_ep_bd(const QMfmaEpBdArgs& a, int64_t batch, hipStream_t st)
{
    constexpr int TM = WGM * TI * 32, TN = WGN * TJ * 32;
    constexpr int STAGE = (LA * TM + LB * TN) * BK;
    const int64_t blocks = batch * a.bd_tm * a.bd_tn;
    if (blocks <= 0) return hipSuccess;
    if (blocks > 0x7fffffffll || a.Kp % BK || a.Mp != batch * a.bd_tm * TM || a.Np != batch * a.bd_tn * TN || !a.has_ep || !a.ep.bits32 || a.kara || a.c_host ||
        a.bd.msize != (int64_t)a.bd_tm * a.bd_tn * TM * TN)
        return hipErrorInvalidValue;
    const hipError_t e = qg_launch_lds<k_mfma_ep_bd<LA, LB, BK, WGM, WGN, TI, TJ, NSTAGE>>((unsigned)blocks, 64 * WGM * WGN, NSTAGE * STAGE, st, a);
    if constexpr (LA == 3 && LB == 3) {
        if (e == hipSuccess && (a.maskA || a.maskB))
            return qg_launch_lds<k_mfma_ep_bd<2, 2, BK, WGM, WGN, TI, TJ, NSTAGE, 3, 3>>((unsigned)blocks, 64 * WGM * WGN, NSTAGE * (2 * TM + 2 * TN) * BK, st, a);
    }
    return e;
}

} // namespace

hipError_t qg_launch_mfma_ep_bd(int LA, int LB, const QMfmaEpBdArgs& a, int64_t batch, hipStream_t st)
{
    if (LA == 1 && LB == 1) {
        if (a.variant == QG_MFMA_64_BK128) return launch_ep_bd<1, 1, 128, 2, 2, 1, 1, 3>(a, batch, st);
        return hipErrorInvalidValue;
    }
    if (a.variant != QG_MFMA_LIMB_64) return hipErrorInvalidValue;
    switch (LA * 10 + LB) {
    case 12: return launch_ep_bd<1, 2, 64, 2, 2, 1, 1, 3>(a, batch, st);
    case 21: return launch_ep_bd<2, 1, 64, 2, 2, 1, 1, 3>(a, batch, st);
    case 22: return launch_ep_bd<2, 2, 64, 2, 2, 1, 1, 3>(a, batch, st);
    case 13: return launch_ep_bd<1, 3, 64, 2, 2, 1, 1, 3>(a, batch, st);
    case 31: return launch_ep_bd<3, 1, 64, 2, 2, 1, 1, 3>(a, batch, st);
    case 23: return launch_ep_bd<2, 3, 64, 2, 2, 1, 1, 3>(a, batch, st);
    case 32: return launch_ep_bd<3, 2, 64, 2, 2, 1, 1, 3>(a, batch, st);
    case 33: return launch_ep_bd<3, 3, 64, 2, 2, 1, 1, 3>(a, batch, st);
    default: return hipErrorInvalidValue;
    }
}
