// qg_tree_rc.hip — exact tree-order evaluation for ONE REAL and ONE COMPLEX operand, 32-bit VALU path
// (QG_CMUL_REAL_A / QG_CMUL_REAL_B, include/qgemul.h).
//
// The reference's Qmul(real, complex) and Qmul(complex, real) are part-wise (the reference's QuBLAS.h:3604-3644):
//     re = Qmul<realT...>(x, y.real), im = Qmul<imagT...>(x, y.imag)        (or x.real * y, x.imag * y)
// and the pairwise tree reduces the two parts separately with their own per-level formats (complex Qadd is part-wise,
// QuBLAS.h:3549-3564; the level buffer converts on store, :4966).  So a mixed Qgemul is two real trees that share one operand:
// the shared real value is read from LDS once per leaf and row / column and feeds both parts' products.
//
// Framing: k_tree_cplx's (qg_tree_cplx.hip) — a 32 x 32 tile per block, 32-leaf chunks staged in LDS, each lane owns a 2 x 2 block of
// outputs of both parts, the tree is the register-resident binary counter of qg_tree_counter.h, blocks walk the tiles in the
// XCD-aware order of qg_tile_walk.h.  LDS holds ONE plane of the real operand and TWO of the complex one.  A k step is two
// quantised multiplications (slots QG_M_RE, QG_M_IM) and the two parts' nodes.  Step forms (MODE): QCF_RUNTIME — every step through the
// run-time-mode conversion of qg_step_all.h; QCF_COMPACT — the branch-free records of qg_fix.h (QFix, qg_plan.h), fetched with scalar
// loads that share a wait.  CA says which operand is the complex one; there is one body.
#include <hip/hip_runtime.h>
#include <stddef.h>

#include "qg_fix.h"
#include "qg_forms.h"
#include "qg_kernels.h"
#include "qg_step_all.h"
#include "qg_tile_walk.h"
#include "qg_tree_counter.h"
#include "qg_tree_io.h"

namespace {

constexpr int KC = QG_TREE_KC;
constexpr int TMB = 32, TNB = 32;  // 16x16 threads x (2x2)
constexpr int PITCH = KC + 4;

// one quantised multiplication on N values: slot QG_M_RE / QG_M_IM
template <int MODE, int N>
__device__ __forceinline__ void op_mul(int (&out)[N], const int (&x)[N], const int (&y)[N], const QTreeTable* __restrict__ t, const QFix& f, int slot)
{
    if constexpr (MODE == QCF_COMPACT) {
        if (f.ka != 1) {   // an exact product that is brought to MORE fraction bits: scale one factor (wave-uniform, rare)
#pragma unroll
            for (int o = 0; o < N; ++o) out[o] = mad24_vvs(__mul24(x[o], f.ka), y[o], f.t);
        } else {
#pragma unroll
            for (int o = 0; o < N; ++o) out[o] = mad24_vvs(x[o], y[o], f.t);
        }
        fx_finish<N>(out, f);
    } else {
#pragma unroll
        for (int o = 0; o < N; ++o) out[o] = x[o] * y[o];
        qg_step_all<int, N>(out, t->mul[slot].q);
    }
}

// the compact node of one part: add, the add's conversion, the level buffer's conversion
template <int N>
__device__ __forceinline__ void fx_node(int (&v)[N], const int (&x)[N], const QFix& fa, const QFix& fc)
{
#pragma unroll
    for (int o = 0; o < N; ++o) v[o] = x[o] + v[o] + fa.t;   // v_add3_u32
    if (fa.ls) {      // (wave-uniform, rare: the add's result type has more fraction bits than its operands)
#pragma unroll
        for (int o = 0; o < N; ++o) v[o] = (int)((unsigned)v[o] << fa.ls);
    }
    fx_finish<N>(v, fa);
    if (!(fc.skip & 1)) {   // the level buffer's conversion (identity unless the level type differs from the add's result)
        if (fc.ls) {
#pragma unroll
            for (int o = 0; o < N; ++o) v[o] = (int)((unsigned)v[o] << fc.ls);
        } else {
#pragma unroll
            for (int o = 0; o < N; ++o) v[o] += fc.t;
        }
        fx_finish<N>(v, fc);
    }
}

// level l's node of BOTH parts (children share a format, so no alignment shift); compact: their four records in one wait
template <int MODE, int N>
__device__ __forceinline__ void op_node2(int (&v0)[N], int (&v1)[N], const int (&x0)[N], const int (&x1)[N], const QTreeTable* __restrict__ t, int l)
{
    if constexpr (MODE == QCF_COMPACT) {
        QFix fa0, fc0, fa1, fc1;
        fx_at4(t, FX_OFF_ADD(0, l), FX_OFF_CVT(0, l), FX_OFF_ADD(1, l), FX_OFF_CVT(1, l), fa0, fc0, fa1, fc1);
        fx_node<N>(v0, x0, fa0, fc0);
        fx_node<N>(v1, x1, fa1, fc1);
    } else {
#pragma unroll
        for (int o = 0; o < N; ++o) { v0[o] = x0[o] + v0[o]; v1[o] = x1[o] + v1[o]; }
        qg_step_all<int, N>(v0, t->level_add[0][l].q);
        qg_step_all<int, N>(v0, t->level_cvt[0][l]);
        qg_step_all<int, N>(v1, t->level_add[1][l].q);
        qg_step_all<int, N>(v1, t->level_cvt[1][l]);
    }
}

struct QTreeRcArgs {
    const QTreeTable* tab;
    const int32_t* A;  // CA: [2][M][K], else [M][K]
    const int32_t* B;  // CA: [N][K], else [2][N][K]
    char* C;           // [2][M][N] containers
    int64_t M, N, K;   // K: the packed operands' padded length, a multiple of KC
    int32_t cbytes;
};

template <int MAXL, int MODE, bool CA>   // CA: A is the complex operand (QG_CMUL_REAL_B), else B (QG_CMUL_REAL_A)
__global__ __launch_bounds__(256, 1) void k_tree_rc(QTreeRcArgs g)
{
    constexpr int NPA = CA ? 2 : 1, NPB = CA ? 1 : 2;   // LDS planes per operand
    __shared__ __attribute__((aligned(16))) int sA[NPA][TMB][PITCH];
    __shared__ __attribute__((aligned(16))) int sB[NPB][TNB][PITCH];
    const QTreeTable* __restrict__ tab = g.tab;
    const int tid = threadIdx.x;
    const int tx = tid & 15, ty = tid >> 4;
    const int64_t tiles_n = (g.N + TNB - 1) / TNB, tiles_m = (g.M + TMB - 1) / TMB;
    int64_t tile_m, tile_n;   // XCD-aware block order (qg_tile_walk.h), as k_tree_cplx
    qg_tile_of<16, true>(qg_xcd_block<int64_t>(blockIdx.x, tiles_m * tiles_n), tiles_m, tiles_n, tile_m, tile_n);
    const int64_t m0 = tile_m * TMB, n0 = tile_n * TNB;
    const int nl = tab->n_levels_k;   // (a tree shorter than 5 levels is continued with identity levels: qg_plan.h)

    int low[2][4][4];
    int up[2][MAXL - 4][4];
    int v[2][4];
#pragma unroll
    for (int p = 0; p < 2; ++p)
#pragma unroll
        for (int o = 0; o < 4; ++o) v[p][o] = 0;
#define NODE_RC(S, i, L) op_node2<MODE, 4>(v[0], v[1], S[0][i], S[1][i], tab, L)

    for (int64_t k0 = 0; k0 < g.K; k0 += KC) {
        __syncthreads();
        // stage: 32 rows x 32 k of every plane = 256 16-byte chunks per plane; a thread takes one chunk of each plane.  Rows beyond M / N
        // hold zeros; k never leaves the operand (K is a multiple of KC)
        {
            const int r = (tid >> 3) & 31, q = tid & 7;
#pragma unroll
            for (int p = 0; p < NPA; ++p) {
                int4 x = make_int4(0, 0, 0, 0);
                if (m0 + r < g.M) x = *(const int4*)(g.A + ((int64_t)p * g.M + m0 + r) * g.K + k0 + q * 4);
                *(int4*)&sA[p][r][q * 4] = x;
            }
#pragma unroll
            for (int p = 0; p < NPB; ++p) {
                int4 y = make_int4(0, 0, 0, 0);
                if (n0 + r < g.N) y = *(const int4*)(g.B + ((int64_t)p * g.N + n0 + r) * g.K + k0 + q * 4);
                *(int4*)&sB[p][r][q * 4] = y;
            }
        }
        __syncthreads();
#pragma unroll 1
        for (int kb = 0; kb < KC / 16; ++kb) {
#pragma unroll
            for (int kq = 0; kq < 4; ++kq) {
                int a4[NPA][2][4], b4[NPB][2][4];  // [plane][row/col of the 2x2 block][leaf]
#pragma unroll
                for (int i = 0; i < 2; ++i) {
#pragma unroll
                    for (int p = 0; p < NPA; ++p) {
                        const int4 x = *(const int4*)&sA[p][ty * 2 + i][kb * 16 + kq * 4];
                        a4[p][i][0] = x.x; a4[p][i][1] = x.y; a4[p][i][2] = x.z; a4[p][i][3] = x.w;
                    }
#pragma unroll
                    for (int p = 0; p < NPB; ++p) {   // columns tx and tx + 16: 16 consecutive rows per read group, no bank conflict (qg_tree_fast.hip)
                        const int4 y = *(const int4*)&sB[p][tx + 16 * i][kb * 16 + kq * 4];
                        b4[p][i][0] = y.x; b4[p][i][1] = y.y; b4[p][i][2] = y.z; b4[p][i][3] = y.w;
                    }
                }
#pragma unroll
                for (int e = 0; e < 4; ++e) {
                    const int kk = kq * 4 + e;   // compile-time leaf index inside the 16-leaf block
                    // ---- the two part-wise products per output: re = a.re * b.re, im = (CA ? a.im * b.re : a.re * b.im)
                    int xr[4], xi[4], yr[4], yi[4];
#pragma unroll
                    for (int i = 0; i < 2; ++i)
#pragma unroll
                        for (int j = 0; j < 2; ++j) {
                            xr[i * 2 + j] = a4[0][i][e]; xi[i * 2 + j] = a4[NPA - 1][i][e];
                            yr[i * 2 + j] = b4[0][j][e]; yi[i * 2 + j] = b4[NPB - 1][j][e];
                        }
                    QFix f0{}, f1{};
                    if constexpr (MODE == QCF_COMPACT) fx_at2(tab, FX_OFF_MUL(QG_M_RE), FX_OFF_MUL(QG_M_IM), f0, f1);
                    op_mul<MODE, 4>(v[0], xr, yr, tab, f0, QG_M_RE);
                    op_mul<MODE, 4>(v[1], xi, yi, tab, f1, QG_M_IM);   // (xi == xr when A is real, yi == yr when B is real)
                    // ---- lower four levels (compile-time leaf index)
                    QG_TREE_LOW_LOOP(kk, low, v, QG_TREE_PARK2, NODE_RC);
                }
            }
            QG_TREE_UP(MAXL, (k0 >> 4) + kb, nl, up, v, QG_TREE_PARK2, NODE_RC);
        }
    }
#undef NODE_RC
    qg_step_all<int, 4>(v[0], tab->c_cvt[0]);
    qg_step_all<int, 4>(v[1], tab->c_cvt[1]);
#pragma unroll
    for (int p = 0; p < 2; ++p)
#pragma unroll
        for (int i = 0; i < 2; ++i)
#pragma unroll
            for (int j = 0; j < 2; ++j) {
                const int64_t m = m0 + ty * 2 + i, n = n0 + tx + 16 * j;
                if (m < g.M && n < g.N) qg_store_c(g.C, ((int64_t)p * g.M + m) * g.N + n, g.cbytes, v[p][i * 2 + j]);
            }
}

template <int MODE>
hipError_t launch_rc(int n_levels, int a_complex, int64_t blocks, hipStream_t st, const QTreeRcArgs& g)
{
    return a_complex ? qg_launch_by_levels(n_levels, k_tree_rc<12, MODE, true>, k_tree_rc<16, MODE, true>, blocks, st, g)
                     : qg_launch_by_levels(n_levels, k_tree_rc<12, MODE, false>, k_tree_rc<16, MODE, false>, blocks, st, g);
}

} // namespace

hipError_t qg_launch_tree_rc(const QTreeTable* dev_table, int n_levels, QCplxForm form, int a_complex, const void* A, const void* B, void* C, int64_t M,
                             int64_t N, int64_t K, int cbytes, hipStream_t st)
{
    int64_t blocks;
    if (const hipError_t e = qg_tree_blocks(M, N, K, n_levels, TMB, TNB, blocks); e != hipSuccess || blocks == 0) return e;
    QTreeRcArgs g{dev_table, (const int32_t*)A, (const int32_t*)B, (char*)C, M, N, K, cbytes};
    switch (form) {
    case QCF_RUNTIME:
        // at most 12 levels: with 16, the counter's upper levels around the run-time-mode node no longer unroll and `up` leaves the registers
        // (400 bytes of scratch per lane); the planner sends such descriptors to the general kernel (qg_plan.cpp: qg_tree_choice)
        if (n_levels > 12) return hipErrorInvalidValue;
        hipLaunchKernelGGL(HIP_KERNEL_NAME(a_complex ? k_tree_rc<12, QCF_RUNTIME, true> : k_tree_rc<12, QCF_RUNTIME, false>), dim3((unsigned)blocks), dim3(256), 0, st, g);
        return hipGetLastError();
    case QCF_COMPACT: return launch_rc<QCF_COMPACT>(n_levels, a_complex, blocks, st, g);
    default: return hipErrorInvalidValue;   // (the planner gives a mixed descriptor no other form)
    }
}
