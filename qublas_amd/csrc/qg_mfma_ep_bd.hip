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
#include "qg_member_forms.h"
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

} // namespace

// batch * bd_tm * bd_tn workgroups, the forms and the 3 x 3 pair of qg_member_forms.h; both partners carry the chain
hipError_t qg_launch_mfma_ep_bd(int LA, int LB, const QMfmaEpBdArgs& a, int64_t batch, hipStream_t st)
{
    return qg_member_form(LA, LB, a.variant, [&](auto form) -> hipError_t {
        using F = decltype(form);
        const int64_t blocks = batch * a.bd_tm * a.bd_tn;
        if (blocks <= 0) return hipSuccess;
        if (blocks > 0x7fffffffll || a.Kp % F::BK || a.Mp != batch * a.bd_tm * F::TM || a.Np != batch * a.bd_tn * F::TN || !a.has_ep || !a.ep.bits32 || a.kara || a.c_host ||
            a.bd.msize != (int64_t)a.bd_tm * a.bd_tn * F::TM * F::TN)
            return hipErrorInvalidValue;
        return qg_member_launch(form, a, [&](auto k) {
            using K = decltype(k);
            return qg_launch_lds<k_mfma_ep_bd<QG_MEMBER_FORM_ARGS(K)>>((unsigned)blocks, K::THREADS, K::LDS, st, a);
        });
    });
}
