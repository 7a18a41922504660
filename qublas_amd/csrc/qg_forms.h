// qg_forms.h — the step forms of the 32-bit tree kernels, named once for the planner (qg_plan.cpp), the kernel choice
// (qg_tree_choice) and the launchers.  Where a kernel is templated on `int MODE`, the enumerator's value IS that template
// argument; the forms that select a different kernel have values of their own.
#pragma once

// k_tree_fast<SPLIT, MUL24, MAXL, MODE> / k_tree_pk16<MAXL, HYB, UNS> (qg_tree_fast.hip), real data
enum QTreeForm : int {
    QTF_RUNTIME = 0,      // per-node formats and modes are run-time values (any real descriptor the planner admits)
    QTF_ONE_ZERO = 1,     // the product and every tree level share ONE format, TRN::TCPL rounding, SAT::ZERO overflow: a node is
                          //   3 VALU instructions on values biased by -lo (the range test is one unsigned compare)
    QTF_ONE_TCPL = 2,     // ... SAT::TCPL overflow: a node is v_add + v_med3 (the default-tag shapes)
    QTF_REC_CLAMP = 3,    // per-level formats, every step in the compact form of qg_fix.h (QFix, qg_plan.h): the node's record is one
                          //   scalar load, the node v_add3 (+ the rounding addend), a shift where the level has fewer fraction bits
                          //   and one v_med3 — every step of the descriptor clamps
    QTF_REC_BIASED = 4,   // ... SAT::ZERO / WRP::TCPL steps exist: values biased by -lo of their format, the overflow by the record's
                          //   kind (one unsigned compare + select, med3(u, 0, span) or u & span)
    QTF_REC_KINDS = 5,    // ... the same kinds on unbiased values, where a format is too wide for the biased form
    QTF_LJ = 6,           // one signed SAT::TCPL format for the product and every level, held LEFT-JUSTIFIED (qg_fix.h,
                          //   QTreeTable::lj): the product one saturating v_mad_i32_i24 + v_and, a node one saturating v_add_i32
                          //   (+ v_and at the odd levels); never split
    QTF_LJ_U = 16,        // ... on an unsigned format (every operand unsigned): the uint32 range, v_mad_u32_u24 / v_add_u32 ... clamp
    QTF_WORD = 17,        // 32-BIT WORDS (one signed SAT::TCPL format of exactly 32 bits): floor((a b + t) / 2^d) of the exact 64-bit
                          //   product saturated to the word by a range test, a node one v_add_i32 ... clamp (QTreeTable::lj: s = d)
    QTF_WORD_MAD = 18,    // ... with a product shift of 10 ... 23: the product's word from one saturating multiply-add
    QTF_JWORD = 19,       // QTF_WORD on JUSTIFIED words (signed SAT::TCPL formats of fewer than 32 bits held as x * 2^sj, lj.e[0] = sj)
    QTF_JWORD_MAD = 20,   // QTF_WORD_MAD on justified words
    QTF_WORD_WRAP = 21,   // a WRAPPING 32-bit word (signed WRP::TCPL, lj.e[1] = 1): the word is v_alignbit of the exact product's
                          //   halves, a node a plain 32-bit add
    // k_tree_pk16<MAXL, HYB, UNS>: QTF_LJ for formats of at most 16 bits, TWO outputs per register
    QTF_PK16 = 7,         // HYB 0: products and nodes in packed 16-bit halves (QTreeTable::lj16)
    QTF_PK16_HYB = 8,     // HYB 1: 32-bit justified products, packed 16-bit nodes (formats of fewer than 16 bits)
    QTF_PK16_HYB16 = 9,   // HYB 2: ... formats of exactly 16 bits (no bits below the unit in a half)
    QTF_PK16_U = 22,      // the same three on unsigned formats (UNS)
    QTF_PK16_HYB_U = 23,
    QTF_PK16_HYB16_U = 24,
};

// k_gemv<CH, MODE> / k_gemv_short<KK, MODE> (qg_gemv.hip), one output column
enum QGemvForm : int {
    QGF_RUNTIME = 0,      // run-time modes
    QGF_ONE_ZERO = 1,     // every tree level has ONE format (the product's), no rounding shift, SAT::ZERO overflow
    QGF_ONE_TCPL = 2,     // ... SAT::TCPL overflow
    QGF_REC_CLAMP = 3,    // per-level formats in the compact records of qg_plan.h (QFix), every level clamps
    QGF_REC_KINDS = 5,    // ... with the records' rounding / overflow kinds
    QGF_WORD = 6,         // 32-bit words (QAnalysis::gemv_w32): a node is one saturating v_add_i32; long rows only
    QGF_WORD_RND = 7,     // ... and the product "add a constant, shift right by 1 ... 31, saturate to the word"
};

// k_tree_cplx<MAXL, MODE, TF> / k_tree_cplx_pk16<MAXL, TF> (qg_tree_cplx.hip), complex data
enum QCplxForm : int {
    QCF_RUNTIME = 0,      // run-time modes
    QCF_TABLE = 1,        // every step RND::POS_INF (or exact) + SAT::TCPL: fixed modes, steps read from the step table
    QCF_COMPACT = 2,      // ... in the compact branch-free records (QFix, qg_plan.h)
    QCF_KINDS = 3,        // compact records with a branch on the rounding / overflow kind
    QCF_UNIFORM = 4,      // ONE clamp for the whole loop: the common range and the products' (t, d) in registers (QTreeTable::uni)
    QCF_LJ = 5,           // ... on left-justified values (QTreeTable::lj)
    // compact records with the branch-free kinds of a feature set f (qg_fix.h, fx_finish_feat): 8 + f
    QCF_KINDS_R = 9,      // f = 1: value-dependent roundings
    QCF_KINDS_Z = 10,     // f = 2: SAT::ZERO
    QCF_KINDS_RZ = 11,
    QCF_KINDS_W = 12,     // f = 4: wraps
    QCF_KINDS_RW = 13,
    QCF_KINDS_ALL = 15,   // f = 7, and f = 6 (ZW) as well: the full set
    QCF_PK16 = 6,         // k_tree_cplx_pk16: QCF_LJ in packed 16-bit halves, two outputs per register (QTreeTable::lj16)
};

// the branch-free form of the feature set f = 1 ... 7 (QCF_KINDS_R ... QCF_KINDS_ALL)
inline QCplxForm qcf_kinds(int f)
{
    return f == 6 ? QCF_KINDS_ALL : (QCplxForm)(8 + f);
}
