// qg_bd_ep.h — the element-wise chain of a batched plan as ONE block-diagonal pass over the stack's packed C -> the stack's
// packed D (qg_eltwise_bd.hip): k_eltwise's and k_approx's framing, plus the member an element belongs to (QBdEp, qg_kernels.h).
#pragma once
#include "qg_approx.h"
#include "qg_kernels.h"

// g.n = batch * bd.msize elements; a member's packed C is a whole number of 64 x 64 tiles, i.e. of 4096-element workgroups
struct QEltwiseBdArgs {
    QEltwiseArgs g;
    QBdEp bd;
};
struct QApproxBdArgs {
    QApproxArgs x;
    QBdEp bd;
};
#if defined(__HIPCC__)
hipError_t qg_launch_eltwise_bd(const QEltwiseBdArgs& a, hipStream_t st);
hipError_t qg_launch_approx_bd(const QApproxBdArgs& a, hipStream_t st);
#endif
