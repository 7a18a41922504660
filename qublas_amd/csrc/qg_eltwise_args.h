// qg_eltwise_args.h — plain argument structs of the element-wise epilogue (host and device code)
#pragma once
#include "qg_plan.h"

// run-time operands of the stages (device pointers to packed tensors in the plan's packed-C index space, or scalars)
struct QEpArgs {
    const char* e[QG_MAX_EW];
    int64_t scalar[QG_MAX_EW];
};

// a batched plan's chain (qgemul_plan_create_batched_epx) in its block-diagonal forms: C, D and every per-member tensor operand are the
// members' packed tensors back to back (one index space over the whole stack); a SHARED operand is ONE member's packed tensor, read at
// the member-local index  i - member * msize  (it is not replicated when it is packed: for 1024 members of 64 x 64 that would add as
// many bytes as C itself).  msize = elements of one member's packed C (a whole number of 64 x 64 tiles), shared bit k = stage k's
// tensor operand is shared
struct QBdEp {
    int64_t msize;
    uint32_t shared, pad_;
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
// ... over the stack of a batched plan: g.n = batch * bd.msize elements; a member's packed C is a whole number of 64 x 64 tiles, i.e.
// of 4096-element workgroups
struct QEltwiseBdArgs {
    QEltwiseArgs g;
    QBdEp bd;
};
// ... over the launch of a grouped plan: g.n = the launch's elements, a whole number of 64 x 64 tiles, i.e. of 4096-element
// workgroups; tile_member[g.n / 4096]: the member a tile belongs to (qg_grp.h: qg_grp_tile_members)
struct QEltwiseGrpArgs {
    QEltwiseArgs g;
    const int32_t* tile_member;
    QGrpEp ge;
};
// what the launchers of the member passes (these and their APPROX forms, qg_approx.h) check before they launch.  The stack: a whole
// number of members, a member a whole number of workgroups
inline bool qg_pass_stack_ok(int64_t n, const QBdEp& bd) { return bd.msize > 0 && bd.msize % 4096 == 0 && n % bd.msize == 0 && n / 4096 <= 0x7fffffffll; }
// the launch part: whole 64 x 64 tiles, one per workgroup, each with its entry in the tile -> member table
inline bool qg_pass_launch_ok(int64_t n, const int32_t* tile_member) { return tile_member && n % 4096 == 0 && n / 4096 <= 0x7fffffffll; }
