// qg_api_int.h — what the translation units of the C-ABI layer share: qg_api.hip (contexts, classification, plans, pack / execute),
// qg_run.hip (the one-shot calls) and qg_comm.hip.  Nothing here is part of the library's interface: functions that cross a
// translation unit are QG_INTERNAL (hidden visibility).
#pragma once
#include <hip/hip_runtime.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <new>

#include "../../include/qgemul.h"
#include "qg_kernels.h"
#include "qg_ring.h"
#include "qg_plan.h"
#include "qg_approx.h"
#include "qg_cmul.h"
#include "qg_bd_ep.h"
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

// Composite linear plan.  The MFMA kernels take operands of at most 3 int8 limbs and keep exact int32 accumulators only while
// K * min(LA, LB) < 2^17.  Beyond either bound the linear class used to fall to the 64-bit VALU tree kernel (40-300x slower); the
// reference has no such boundary (Reducer, QuBLAS.h:4960-4990; ArbiInt elements up to 64 bits, :347-564).  Now:
//   * an operand of L > 3 limbs is stored as limb GROUPS of 2-3 limbs (x = sum_g x_g * 256^limb0[g], every x_g a balanced
//     base-256 number of its own), each group a complete packed operand of the existing layout;
//   * K is cut into chunks of at most kc reduction indices (a multiple of 256), each chunk a complete packed operand as well;
//   * every (chunk, A group, B group) is ONE launch of an existing MFMA kernel that stores raw dot products (identity
//     epilogue) into a slab, and k_lin_combine (qg_pack.hip) adds the slabs by weight into an exact running sum and, after the
//     last chunk, rounds + overflow-handles it once into C — the linear class's whole epilogue (QuBLAS.h:2398-2411).
// Packed operand = the sub-operands back to back, chunk-major, each 256-byte aligned.
struct QComposite {
    int on;
    int ga, gb;            // limb groups of A, B (1..3)
    int la[3], lb[3];      // limbs per group
    int la0[3], lb0[3];    // first limb of each group
    int var[3][3];         // MFMA variant of the pair (A group, B group); one tile geometry for all pairs
    int nc;                // k-chunks
    int64_t kc;            // reduction indices per chunk (the last chunk: K - (nc - 1) * kc)
    int slab_bytes;        // 4: single-limb pairs (raw int32), 8 otherwise
    int wide;              // 128-bit sums
    int64_t chunk_bytes[2];   // bytes of one FULL chunk of packed A / B (all groups)
};
// what plan_geometry computes for a descriptor, pure host data: the analysis, the kernel and its tile geometry, the packed layouts
struct QPlanGeom {
    QAnalysis an;
    qgemul_info info;
    int LA, LB, variant;
    QMfmaCfg cfg;
    QPackedGeom pa, pb;
    QCGeom pc;            // with an element-wise chain: packed D
    QHostElem ha, hb, hc;
    QEpTable ept;         // the chain (a complex one: of the real parts)
    QEpTable ept_im;      // ... of the imaginary parts
    QCGeom pc_c;          // the kernel's own packed C, which only exists in memory (cwork) for the kernels that do not fuse the chain
    QComposite comp;      // composite linear plan (comp.on): limb groups x k-chunks of sub-GEMMs + an exact combine pass
    int bd;               // the member of a batched plan: k_mfma's block-diagonal form takes it (a batched plan: it launches that form)
};

// Grouped plan (qgemul_plan_create_grouped): `groups` descriptors, analysed once per DISTINCT descriptor (ug / up: its geometry and its
// plain plan, which owns the device resources and serves pack, unpack and — for a straggler — execute).  The members in the one
// grouped launch have the batched analysis' 64 x 64 geometry; their packed operands sit back to back in front of the launch's one
// trailer and one row-sum array (sa / sb: the stack's geometry), the stragglers' behind them.  tiles: the schedule (qg_grp.h).
struct QGrpMember {
    int32_t uniq, in_launch;
    int64_t off[3], bytes[3];   // inside packed A / B / C
    int64_t row_a, row_b;       // in the launch: first row of the member in the stack's row sums
    QPackedGeom pa, pb;         // in the launch: the member's geometry with trailer / row sums relative to ITS start (qg_launch_pack_member)
};
struct QGrouped {
    int64_t groups, n_uniq, n_in, n_tiles;
    qgemul_desc* ud;            // [n_uniq]
    QPlanGeom* ug;              // [n_uniq]
    uint8_t* u_in;              // [n_uniq]: in the launch
    qgemul_plan** up;           // [n_uniq]; nullptr entries while classifying
    QGrpMember* m;              // [groups]
    int64_t key;                // the distinct descriptor whose launch key the launch has (-1: no member is eligible)
    QPackedGeom sa, sb;
    int launches;
    QGrpTile* tiles;            // [n_tiles] host
    QGrpTile* tiles_dev;
    ~QGrouped()
    {
        delete[] ud;
        delete[] ug;
        delete[] u_in;
        delete[] up;
        delete[] m;
        delete[] tiles;
    }
};

struct qgemul_plan : QPlanGeom {
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
    // batched plan (qgemul_plan_create_batched; batch > 0): `batch` GEMMs of desc at constant strides.  `member` is the plain plan of
    // ONE member and owns every device resource; this object holds what belongs to the batch: info (packed_bytes of the whole
    // batch), the packed operands' stride from member to member (mstride) and, in the block-diagonal form (bd: one launch of
    // k_mfma's BD form over the stacked operands), the STACK's packed geometries in pa / pb — member's with batch times the
    // rows, one plane-mask trailer and one row-sum array behind the planes of all members.  bd == 0: member by member on `member`
    int64_t batch;
    int member_launches;
    qgemul_plan* member;
    int64_t mstride[3];
    // element-wise chain on a batched plan (qgemul_plan_create_batched_epx: batch > 0 with has_ep).  ep / ept / pc (D) / pc_c (C) are
    // the member's.  e_shared[k]: stage k's tensor operand is ONE M x N tensor for every member; estride[k]: bytes of one member's
    // packed operand of stage k (0: no tensor operand) = the step from member to member of a per-member one.  With bd the chain runs
    // inside the block-diagonal launch (bd_fused: k_mfma_ep_bd) or as one block-diagonal pass over the stack's packed C, which is
    // this plan's cwork; without bd member by member through qgemul_execute_ep on `member`
    uint8_t e_shared[QG_MAX_EW];
    int bd_fused;
    int64_t estride[QG_MAX_EW];
    // grouped plan (qgemul_plan_create_grouped): batch == -1, so that the plain entry points refuse it as they refuse a batched plan and
    // the batched ones as they refuse a plain plan; everything else is in grp
    QGrouped* grp;
};

// (defined next to the entry points of include/qgemul.h, inside their extern "C" block)
extern "C" {
QG_INTERNAL int classify_view(const qgemul_desc* d, const EpView* ev, uint32_t opt_flags, qgemul_info* out);
QG_INTERNAL int plan_create_view(qgemul_ctx* c, const qgemul_desc* d, const EpView* ev, uint32_t opt_flags, qgemul_plan** out, int64_t batch = 0);   // batch > 0: the member of a batched plan
// batched plans: ev == nullptr: no chain; bep: which tensor operands of the chain are shared
QG_INTERNAL int classify_batched_view(const qgemul_desc* d, int64_t batch, const EpView* ev, const qgemul_batched_ep* bep, uint32_t opt_flags, qgemul_info* out, int* launches);
// grouped plans: the geometry alone (pure host; *out is the caller's to `delete`, whatever the status) / the plan
QG_INTERNAL int grouped_plan_new(const qgemul_desc* d, int64_t groups, uint32_t opt_flags, qgemul_plan** out);
QG_INTERNAL int plan_create_batched_view(qgemul_ctx* c, const qgemul_desc* d, int64_t batch, const EpView* ev, const qgemul_batched_ep* bep, uint32_t opt_flags, qgemul_plan** out);
QG_INTERNAL bool stores_host_c(const qgemul_plan* p);
// host elements one member of operand `operand` spans at leading dimension ld (0: tight); 0: ld is too small
QG_INTERNAL int64_t member_extent(const qgemul_desc& d, int operand, int64_t ld);
}
