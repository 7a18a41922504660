// qg_grp_ep.h — the element-wise chain of a grouped plan as ONE pass over the launch's packed C -> the launch's packed D
// (qg_eltwise_grp.hip): k_eltwise_bd's and k_approx_bd's framing, plus the member a 64 x 64 tile belongs to (qg_grp.h:
// qg_grp_tile_members) for the per-member scalars (QGrpEp, qg_eltwise_args.h).
#pragma once
#include "qg_approx.h"
#include "qg_kernels.h"

// g.n = the launch's elements: a whole number of 64 x 64 tiles, i.e. of 4096-element workgroups; tile_member[g.n / 4096]
struct QEltwiseGrpArgs {
    QEltwiseArgs g;
    const int32_t* tile_member;
    QGrpEp ge;
};
struct QApproxGrpArgs {
    QApproxArgs x;
    const int32_t* tile_member;
    QGrpEp ge;
};
#if defined(__HIPCC__)
hipError_t qg_launch_eltwise_grp(const QEltwiseGrpArgs& a, hipStream_t st);
hipError_t qg_launch_approx_grp(const QApproxGrpArgs& a, hipStream_t st);
#endif
