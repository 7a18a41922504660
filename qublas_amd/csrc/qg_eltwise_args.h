// qg_eltwise_args.h — plain argument structs of the element-wise epilogue (host and device code)
#pragma once
#include "qg_plan.h"

// run-time operands of the stages (device pointers to packed tensors in the plan's packed-C index space, or scalars)
struct QEpArgs {
    const char* e[QG_MAX_EW];
    int64_t scalar[QG_MAX_EW];
};

// a grouped plan's chain (qgemul_plan_create_grouped_epx): scal[k] != nullptr: scalar stage k takes the raw value scal[k][member], one
// entry per member of the caller's list, instead of QEpArgs::scalar[k]
struct QGrpEp {
    const int64_t* scal[QG_MAX_EW];
};

// arguments of the stand-alone pass: packed C (cbytes containers, n elements incl. padding) -> packed D
struct QEltwiseArgs {
    const char* C;
    char* D;
    int64_t n;
    int32_t cbytes, pad_;
    QEpTable t;
    QEpArgs a;
};

