// qg_cmul.h — complex x complex multiplication as a stage of a complex element-wise chain (QG_EW_CMUL, include/qgemul.h; the
// reference's BasicComplexMul / TFComplexMul, QuBLAS.h:3421-3534), pre-resolved for the device, the planner entry that walks the
// two part chains of such a chain in lock step, and the launcher of the one pass that runs it.
//
// With f1 = a + bi the first argument of the Qmul and f2 = c + di the second (x_first: f1 = the running value, f2 = the operand):
//   Basic  n[QG_B_AC] = a c, n[QG_B_BD] = b d, n[QG_B_AD] = a d, n[QG_B_BC] = b c, n[QG_B_RE] = ac - bd, n[QG_B_IM] = ad + bc
//   TF     n[QG_T_AB] = a + b, n[QG_T_CD] = c + d, n[QG_T_BA] = b - a, n[QG_T_A] = ab c, n[QG_T_B] = cd b, n[QG_T_C] = ba d,
//          n[QG_T_RE] = A - B, n[QG_T_IM] = B - C
// every node rounded and overflowed into its own format (QNode::q; add / sub nodes align their operands by sa / sb first).
#pragma once
#include "qg_eltwise_args.h"

struct QCmulStage {
    int32_t cmul, x_first, scalar, ebytes;   // QG_CMUL_*; ebytes: container of the packed complex operand (both halves)
    QNode n[8];                              // qgemul.h slot order
};

// qg_analyze_ep for a complex chain that holds CMUL stages: cx[k] non-null exactly for them.  t[0] / t[1]: the part chains' tables
// (a CMUL stage's entry holds op, scalar, ebytes, its RE / IM node and the assignment to the stage's tensor); cmt: QG_MAX_EW
// records to fill (nullptr: classification only).  ONE range tracking serves both parts, so max_bits and bits32 (equal in both
// tables) speak for the two chains and every CMUL node together.
int qg_analyze_epcx(const qfmt c[2], const qgemul_epilogue_cplx* ep, const qgemul_cmul* const* cx, QEpTable t[2], QCmulStage* cmt, int* max_bits,
                    char* reason, size_t reason_len);

// the chain as ONE pass over packed complex C -> packed complex D: a lane owns both halves of its elements
struct QCplxPassArgs {
    const char* C;          // [2][n] containers of cbytes
    char* D;                // [2][n] containers of t[0].dbytes
    int64_t n;              // elements per half, padding included
    int32_t cbytes, pad_;
    QEpTable t[2];
    QEpArgs a;              // tensor operands (complex: [2][n] in st.ebytes containers; real: [n]) and the real parts' scalars
    int64_t scalar_im[QG_MAX_EW];
    uint8_t e_cplx[QG_MAX_EW];
    int32_t pad2_;
    const QCmulStage* cm;   // device: QG_MAX_EW records, entry k valid for a CMUL stage
};
#if defined(__HIPCC__)
hipError_t qg_launch_eltwise_cplx(const QCplxPassArgs& g, hipStream_t st);
#endif
