// qg_api_int.h — what the translation units of the C-ABI layer share: qg_api.hip (contexts, the entry points, plans' resources, pack /
// execute), qg_run.hip (the one-shot calls) and qg_comm.hip; the planner they ask is qg_geom.h.  Nothing here is part of the library's interface: functions that cross a
// translation unit are QG_INTERNAL (hidden visibility).
#pragma once
#include <hip/hip_runtime.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <new>

#include "../../include/qgemul.h"
#include "qg_geom.h"
#include "qg_kernels.h"
#include "qg_ring.h"
#include "qg_plan.h"
#include "qg_approx.h"
#include "qg_cmul.h"
#include "qg_run_key.h"

#define QG_INTERNAL __attribute__((visibility("hidden")))

// the calling thread's last HIP error (qgemul_last_hip_error)
extern "C" {
QG_INTERNAL int qg_last_hip();
QG_INTERNAL void qg_set_last_hip(int e);
}

#define QG_HIP(expr)                         \
    do {                                     \
        hipError_t e_ = (expr);              \
        if (e_ != hipSuccess) {              \
            qg_set_last_hip((int)e_);        \
            return QG_EHIP;                  \
        }                                    \
    } while (0)

struct qgemul_ctx {
    int device;
    hipStream_t stream;
    int* flag_dev;
};

// Every entry point that launches, allocates or frees runs on ITS context's device, whatever device the calling thread has
// current, and leaves the caller's current device as it found it (one process may drive several GPUs: qgemul_run_sharded).
struct DeviceScope {
    int prev = -1;
    bool changed = false;
    hipError_t err = hipSuccess;
    explicit DeviceScope(int dev)
    {
        err = hipGetDevice(&prev);
        if (err == hipSuccess && prev != dev) {
            err = hipSetDevice(dev);
            changed = err == hipSuccess;
        }
    }
    ~DeviceScope() { if (changed) hipSetDevice(prev); }
    DeviceScope(const DeviceScope&) = delete;
    DeviceScope& operator=(const DeviceScope&) = delete;
};
#define QG_ON_DEVICE(ctxp)                 \
    DeviceScope dev_scope_((ctxp)->device); \
    QG_HIP(dev_scope_.err)

// a plan: its geometry (qg_geom.h; a batched plan: the STACK's QPlanGeom and the batch's QBatchGeom), what it was made from and its device resources
struct qgemul_plan : QPlanGeom, QBatchGeom {
    qgemul_ctx* ctx;
    qgemul_desc desc;
    uint32_t flags;
    QTreeTable* dev_table;
    QTreeChoice tc;       // the tree kernels' step form that launches (qg_tree_choice: the diagnostic library's A/B switches applied)
    int64_t* workspace;   // complex linear class: raw dot products [2Mh x 2Nh] int64
    // element-wise epilogue (qgemul_epilogue): pc then describes packed D; pc_c is the kernel's own packed C, which
    // only exists in memory (cwork) for the kernels that do not fuse the chain
    int has_ep;
    qgemul_epilogue ep;
    // complex chain (qgemul_epilogue_cplx): ep / ept are the chain of the real parts, ep_im / ept_im of the imaginary parts
    int ep_cplx;
    qgemul_epilogue ep_im;
    uint8_t e_cplx[QG_MAX_EW];
    // APPROX stages (qg_approx.h): has_ax = the chain holds one (it then always runs as the pass of qg_approx.hip); ax_dev[k] = stage k's
    // table on the device, ax_uniform = every table has the uniform form
    int has_ax, ax_uniform;
    QApproxTable* ax_dev[QG_MAX_EW];
    // CMUL stages (qg_cmul.h): has_cmul = the complex chain holds one (it then runs as the one pass of qg_eltwise_cplx.hip, never as
    // two k_eltwise launches); cx = the plan's copy of the caller's records, cm_dev = QG_MAX_EW pre-resolved records on the device
    int has_cmul;
    qgemul_cmul cx[QG_MAX_EW];
    QCmulStage* cm_dev;
    void* cwork;
    int32_t* wide_ws;     // single-limb MFMA with a left-shifting epilogue that leaves 32 bits: raw int32 dot products
    void* hostc_pc;       // qgemul_execute_host_c on a kernel that cannot store the reference layout: its packed C
    void* comp_slabs;     // comp.ga * comp.gb slabs of raw dot products, one common packed-C layout
    void* comp_acc;       // running exact sums between k-chunks (comp.nc > 1)
    // batched plan (qgemul_plan_create_batched; QBatchGeom::batch > 0): `member` is the plain plan of ONE member and owns every device
    // resource; with a chain, ep / ept / pc (D) / pc_c (C) are the member's, and the block-diagonal pass form's packed C of the whole stack
    // is this plan's cwork
    qgemul_plan* member;
    // ... in the stacked form (QPlanGeom::bd_stack, QG_OPT_BATCHED_STACKED): the raw dot products between the block-diagonal launch and
    // the combine pass, QBatchGeom::stack_ws bytes, owned by the batched plan itself
    int64_t* stack_work;
    // grouped plan (qgemul_plan_create_grouped): batch == -1, so that the plain entry points refuse it as they refuse a batched plan and
    // the batched ones as they refuse a plain plan; everything else is in grp.  With a chain (qgemul_plan_create_grouped_epx): has_ep, ep, ept
    // and has_ax are the group's one chain, the device tables of its APPROX stages are the key plan's (grp->up[grp->key])
    QGrouped* grp;
};

// (defined next to the entry points of include/qgemul.h, inside their extern "C" block)
extern "C" {
QG_INTERNAL int classify_view(const qgemul_desc* d, const EpView* ev, uint32_t opt_flags, qgemul_info* out);
QG_INTERNAL int plan_create_view(qgemul_ctx* c, const qgemul_desc* d, const EpView* ev, uint32_t opt_flags, qgemul_plan** out, int64_t batch = 0);   // batch > 0: the member of a batched plan
// batched plans: ev == nullptr: no chain; bep: which tensor operands of the chain are shared
QG_INTERNAL int classify_batched_view(const qgemul_desc* d, int64_t batch, const EpView* ev, const qgemul_batched_ep* bep, uint32_t opt_flags, qgemul_info* out, int* launches);
QG_INTERNAL int plan_create_batched_view(qgemul_ctx* c, const qgemul_desc* d, int64_t batch, const EpView* ev, const qgemul_batched_ep* bep, uint32_t opt_flags, qgemul_plan** out);
QG_INTERNAL bool stores_host_c(const qgemul_plan* p);
}
