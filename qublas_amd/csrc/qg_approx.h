// qg_approx.h — the piecewise-polynomial activation stage (QG_EW_APPROX, include/qgemul.h; the reference's ANUS::Qapprox,
// QuBLAS.h:4829-4897), pre-resolved for the device, and the launcher of the pass that runs chains which hold such a stage.
//
// Segment s is selected by the number of LEADING thresholds the raw value has reached (raw >= thr[0], raw >= thr[1], ...: the
// first s with raw < thr[s], the last segment when there is none), Horner level i is
//     p = Qmul<f_i>(x, v)  ->  lvl[i].mul  (the product, F_x + F_{i+1} fraction bits, rounded and overflowed into f_i)
//     v = Qadd<f_i>(a_i, p) ->  lvl[i].add (both operands in f_i: the overflow handling only)
// and to_x is the converting constructor back into x's own format.
#pragma once
#include "qg_eltwise_args.h"

struct QApproxLevel {
    QStep mul, add;
};
struct QApproxSeg {
    int32_t n_coef, pad_;
    QStep to_x;
    QApproxLevel lvl[QG_MAX_COEF - 1];
};
// one table per APPROX stage, in a device buffer of the plan (12.6 KiB: the step records are read with scalar loads, the
// thresholds and coefficients — the first 1168 bytes — are what the kernel copies into LDS)
struct QApproxTable {
    int32_t n_seg;
    int32_t uniform;     // every segment has the same n_coef, the same format at every level and the same step records: seg[0] serves all
    int32_t n_coef_max, pad_;
    int64_t thr[QG_MAX_SEG];                 // thr[s], s < n_seg - 1, clamped to [lo, hi + 1] of x's format (+-inf and huge breakpoints included); the rest: hi + 1
    int64_t coef[QG_MAX_COEF][QG_MAX_SEG];   // coef[i][s]: level-major, so that one level's fetch touches 16 consecutive words
    QApproxSeg seg[QG_MAX_SEG];
};
enum { QG_APPROX_LDS_WORDS = QG_MAX_SEG + QG_MAX_COEF * QG_MAX_SEG };   // thr + coef

// qg_analyze_ep with APPROX stages: ax[k] non-null exactly for them; axt: QG_MAX_EW tables to fill (nullptr: classification only)
int qg_analyze_epx(qfmt c, const qgemul_epilogue* ep, const qgemul_approx* const* ax, QEpTable* out, QApproxTable* axt, int* max_bits, char* reason,
                   size_t reason_len);

// the chain as a pass over packed C -> packed D (k_eltwise's framing), for chains with APPROX stages
struct QApproxArgs {
    QEltwiseArgs g;
    const QApproxTable* ax[QG_MAX_EW];   // device pointers; nullptr for the plain stages
    int32_t force_general, pad_;         // QG_OPT_APPROX_GENERAL: uniform tables run the general form too
};
// ... over the stack of a batched plan and over the launch of a grouped plan (QEltwiseBdArgs, QEltwiseGrpArgs: qg_eltwise_args.h)
struct QApproxBdArgs {
    QApproxArgs x;
    QBdEp bd;
};
struct QApproxGrpArgs {
    QApproxArgs x;
    const int32_t* tile_member;
    QGrpEp ge;
};
#if defined(__HIPCC__)
hipError_t qg_launch_approx(const QApproxArgs& a, hipStream_t st);
hipError_t qg_launch_approx_bd(const QApproxBdArgs& a, hipStream_t st);
hipError_t qg_launch_approx_grp(const QApproxGrpArgs& a, hipStream_t st);
#endif
