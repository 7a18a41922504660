// qg_tree_counter.h — the streamed pairwise tree of the tiled tree kernels (k_tree_fast, k_tree_pk16, k_tree_cplx,
// k_tree_cplx_pk16, k_tree64), once.
//
// The reference reduces K leaves pairwise, level by level (Reducer::reduce_impl); a kernel that streams the leaves in order
// holds one pending value per level — a binary counter over the leaf index.  A new value of level l (v) looks at bit l of
// its index: 0 — it is a LEFT child and PARKS in the level's slot; 1 — the parked left child and v make the level's NODE,
// whose result CARRIES into level l + 1.  After the last leaf of a tree of 2^n leaves the carry has run through every level
// and v is the root.
//
// The counter is split where the leaf index stops being a compile-time value: the kernels unroll blocks of 16 leaves, so
//   QG_TREE_LOW  runs levels 0 ... 3 on the leaf's index inside its block (kk, known once the loop is unrolled: every test
//                folds away and a leaf costs its nodes alone), slots low[0 ... 3];
//   QG_TREE_UP   runs levels 4 ... n_levels - 1 on the block's index (wave-uniform: scalar branches), slots up[0 ... MAXL - 5]
//                of an array that is indexed statically only and so stays in registers.
// Both take the kernel's node operation as NODE(SLOTS, i, L): "v = the node of level L of (slot i of SLOTS, v)", and how a value
// parks as PARK(SLOTS, i, V): QG_TREE_PARK for [slot][N] slots and a [N] value, QG_TREE_PARK2 for the complex kernels, which
// carry both parts at once in [2][slot][N] and [2][N].
//
// Why macros, and why QG_TREE_LOW has a twin.  The change that brought the five kernels' counters here had to leave their code
// as it was, instruction for instruction (tools/isa_diff.py, profiles/tree_counter_isa_identity.txt), and the compiler allowed
// no more than this:
//   * QG_TREE_UP as a __forceinline__ function template taking `up`, `v` and a [&] lambda for the node moved `up` out of the
//     registers in all 12 symbols of k_tree_pk16: scratch 0 -> 64 bytes (MAXL 12) and 0 -> 96 bytes (MAXL 16), 13 ... 15 fewer
//     VGPRs, about 5 % more instructions (2247 -> 2366, 2369 -> 2544); __attribute__((always_inline)) on the lambda changed
//     nothing.  As a macro it is identical in all 108 symbols of the five kernels.
//   * The lower levels were written as an `if` nest in the real kernels (k_tree_fast, k_tree_pk16, k_tree64) and as a loop with a
//     `parked` flag in the complex ones.  After unrolling both are the same nodes in the same order, but neither compiles to the
//     other's code.  The loop in qg_tree_fast.hip: 48 of 54 symbols change, registers included (k_tree_fast<false, false, 16,
//     QTF_WORD>: 186 -> 169 VGPRs, 3251 -> 3197 instructions; <false, false, 12, QTF_RUNTIME>: 221 -> 174 VGPRs).  The nest
//     in qg_tree_cplx.hip: 38 of 52 symbols change (k_tree_cplx<12, QCF_KINDS_RZ, false>: 9171 -> 11719 instructions, 14 -> 20
//     spilled SGPRs; <16, QCF_KINDS_RW, true>: 0 -> 20 bytes of scratch).  A third spelling (count the index's trailing ones,
//     then "node below, park at") changed 48 and 28.  So both spellings are kept, here and nowhere else: QG_TREE_LOW is the nest,
//     QG_TREE_LOW_LOOP the loop.
//   * Even the copy that parks a value cannot be a function in QG_TREE_LOW: with `park(low, 0, v)` (or the slot's row passed by
//     reference) in place of the loop, 24 of the 54 symbols of qg_tree_fast.hip change, register counts among them.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#define QG_TREE_PARK(S, i, V)                                                                                               \
    do {                                                                                                                    \
        _Pragma("unroll") for (int o_ = 0; o_ < (int)(sizeof(V) / sizeof((V)[0])); ++o_) S[i][o_] = V[o_];                  \
    } while (0)
#define QG_TREE_PARK2(S, i, V)                                                                                              \
    do {                                                                                                                    \
        _Pragma("unroll") for (int p_ = 0; p_ < 2; ++p_)                                                                    \
            _Pragma("unroll") for (int o_ = 0; o_ < (int)(sizeof((V)[0]) / sizeof((V)[0][0])); ++o_) S[p_][i][o_] = V[p_][o_]; \
    } while (0)

// levels 0 ... 3 for leaf KK (0 ... 15) of a 16-leaf block; after leaf 15, V is the block's node of level 3
#define QG_TREE_LOW(KK, LOW, V, PARK, NODE)                     \
    do {                                                        \
        if (((KK) & 1) == 0) PARK(LOW, 0, V);                   \
        else {                                                  \
            NODE(LOW, 0, 0);                                    \
            if (((KK) & 2) == 0) PARK(LOW, 1, V);               \
            else {                                              \
                NODE(LOW, 1, 1);                                \
                if (((KK) & 4) == 0) PARK(LOW, 2, V);           \
                else {                                          \
                    NODE(LOW, 2, 2);                            \
                    if (((KK) & 8) == 0) PARK(LOW, 3, V);       \
                    else NODE(LOW, 3, 3);                       \
                }                                               \
            }                                                   \
        }                                                       \
    } while (0)

// the same on the complex kernels (see above: each spelling compiles to the parent's code only where the parent had it)
#define QG_TREE_LOW_LOOP(KK, LOW, V, PARK, NODE)                \
    do {                                                        \
        bool parked_low_ = false;                               \
        _Pragma("unroll") for (int l_ = 0; l_ < 4; ++l_) {      \
            if (!parked_low_) {                                 \
                if ((((KK) >> l_) & 1) == 0) {                  \
                    PARK(LOW, l_, V);                           \
                    parked_low_ = true;                         \
                } else {                                        \
                    NODE(LOW, l_, l_);                          \
                }                                               \
            }                                                   \
        }                                                       \
    } while (0)

// levels 4 ... NL - 1 for 16-leaf block BLOCK (its index in the row: (k0 >> 4) + kb); MAXL: the instantiation's level capacity
#define QG_TREE_UP(MAXL, BLOCK, NL, UP, V, PARK, NODE)                                \
    do {                                                                              \
        const unsigned idx_ = (unsigned)(BLOCK);                                      \
        bool parked_ = false; /* wave-uniform: the carry stopped at a free slot */    \
        _Pragma("unroll") for (int u_ = 0; u_ < (MAXL) - 4; ++u_) {                   \
            if (!parked_ && 4 + u_ < (NL)) {                                          \
                if (((idx_ >> u_) & 1u) == 0) {                                       \
                    PARK(UP, u_, V);                                                  \
                    parked_ = true;                                                   \
                } else {                                                              \
                    NODE(UP, u_, 4 + u_);                                             \
                }                                                                     \
            }                                                                         \
        }                                                                             \
    } while (0)

// ---- launching: the kernels are instantiated for trees of at most 12 and at most 16 levels (the size of `up`)
constexpr int QG_TREE_KC = 32;   // leaves per staged k-chunk: two 16-leaf blocks

// the checks every launcher of these kernels makes: K in whole k-chunks, 5 ... 16 levels, a grid that fits; blocks = 0: nothing to do
inline hipError_t qg_tree_blocks(int64_t M, int64_t N, int64_t K, int n_levels, int tile_m, int tile_n, int64_t& blocks)
{
    blocks = 0;
    if (K % QG_TREE_KC != 0 || n_levels < 5 || n_levels > 16) return hipErrorInvalidValue;
    const int64_t b = ((M + tile_m - 1) / tile_m) * ((N + tile_n - 1) / tile_n);
    if (b > 0x7fffffffll) return hipErrorInvalidValue;
    blocks = b > 0 ? b : 0;
    return hipSuccess;
}

template <class Args>
inline hipError_t qg_launch_by_levels(int n_levels, void (*k12)(Args), void (*k16)(Args), int64_t blocks, hipStream_t st, const Args& g)
{
    hipLaunchKernelGGL(n_levels <= 12 ? k12 : k16, dim3((unsigned)blocks), dim3(256), 0, st, g);
    return hipGetLastError();
}
