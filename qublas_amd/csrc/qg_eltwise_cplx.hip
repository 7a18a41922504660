// qg_eltwise_cplx.hip — complex element-wise chains that hold a complex x complex multiplication (QG_EW_CMUL; the reference's
// BasicComplexMul / TFComplexMul, QuBLAS.h:3421-3534) as ONE pass over packed complex C -> packed complex D (gfx950).
//
// k_eltwise (qg_eltwise.hip) runs a complex chain as two real chains, one launch per half of packed C; a complex multiply needs
// both parts of an element in one thread.  Here a lane takes a run of QG_CPLX_RUN consecutive elements and loads that run from
// the real half and from the imaginary half of packed C, of every complex tensor operand ([2][n], both halves in one container)
// and, once, of every real tensor operand.  Plain stages are qg_ep_stage with each part's own table, unchanged.  A CMUL stage runs
// its 6 (Basic) or 8 (TF) nodes through qg_step_all: the records are wave-uniform (scalar loads from the plan's device table), as
// is the choice of algorithm and of operand order, so no lane branches on a mode.  The arithmetic is 32-bit where the planner has
// bounded both chains and every CMUL node (QEpTable::bits32), 64-bit otherwise.
#include <hip/hip_runtime.h>

#include "qg_cmul.h"
#include "qg_eltwise.h"

namespace {

// elements per lane and half.  8: the 64-bit instantiation holds v and e of both halves (4 x 8 values) plus a CMUL stage's
// products without scratch; resources of both instantiations: profiles/cmul_kernel_resources.txt
enum { QG_CPLX_RUN = 8 };

__device__ __forceinline__ void store_one(char* dst, int64_t idx, int bytes, int64_t v)
{
    switch (bytes) {
    case 1: ((int8_t*)dst)[idx] = (int8_t)v; break;
    case 2: ((int16_t*)dst)[idx] = (int16_t)v; break;
    case 4: ((int32_t*)dst)[idx] = (int32_t)v; break;
    default: ((int64_t*)dst)[idx] = v; break;
    }
}

// N values starting at element idx; `full`: all exist (16-byte loads), else the first `cnt` do and the rest read as 0 — a value
// of every format, so the lane's arithmetic on them stays defined; they are not stored
template <class T, int N>
__device__ __forceinline__ void load_n(const char* p, int64_t idx, int bytes, bool full, int cnt, T (&out)[N])
{
    if (full) {
#pragma unroll
        for (int q = 0; q < N / 4; ++q) qg_ep_load_run<4, T>(p, idx + 4 * q, bytes, out + 4 * q);
        return;
    }
#pragma unroll
    for (int o = 0; o < N; ++o) out[o] = o < cnt ? (T)qg_ep_load_one(p, idx + o, bytes) : (T)0;
}

template <class T, int N>
__device__ __forceinline__ void store_n(char* p, int64_t idx, int bytes, bool full, int cnt, const T (&v)[N])
{
    if (full) {
#pragma unroll
        for (int q = 0; q < N / 4; ++q) qg_ep_store_run<T>(p, idx + 4 * q, bytes, v + 4 * q);
        return;
    }
#pragma unroll
    for (int o = 0; o < N; ++o)
        if (o < cnt) store_one(p, idx + o, bytes, (int64_t)v[o]);
}

template <class T, int N>
__device__ __forceinline__ void mul_node(T (&r)[N], const T (&x)[N], const T (&y)[N], const QNode& n)
{
#pragma unroll
    for (int o = 0; o < N; ++o) r[o] = x[o] * y[o];
    qg_step_all<T, N>(r, n.q);
}
template <class T, int N>
__device__ __forceinline__ void add_node(T (&r)[N], const T (&x)[N], const T (&y)[N], const QNode& n)
{
#pragma unroll
    for (int o = 0; o < N; ++o) r[o] = qg_shl<T>(x[o], n.sa) + qg_shl<T>(y[o], n.sb);
    qg_step_all<T, N>(r, n.q);
}
template <class T, int N>
__device__ __forceinline__ void sub_node(T (&r)[N], const T (&x)[N], const T (&y)[N], const QNode& n)
{
#pragma unroll
    for (int o = 0; o < N; ++o) r[o] = qg_shl<T>(x[o], n.sa) - qg_shl<T>(y[o], n.sb);
    qg_step_all<T, N>(r, n.q);
}

// Qmul<M>(f1, f2), f1 = a + bi, f2 = c + di, on N elements: re / im receive the RE / IM nodes' results (they may alias no input)
template <class T, int N>
__device__ __forceinline__ void cmul_nodes(T (&re)[N], T (&im)[N], const T (&a)[N], const T (&b)[N], const T (&c)[N], const T (&d)[N],
                                           const QCmulStage& s)
{
    T p[N], q[N];
    if (s.cmul == QG_CMUL_BASIC) {
        mul_node<T, N>(p, a, c, s.n[QG_B_AC]);
        mul_node<T, N>(q, b, d, s.n[QG_B_BD]);
        sub_node<T, N>(re, p, q, s.n[QG_B_RE]);
        mul_node<T, N>(p, a, d, s.n[QG_B_AD]);
        mul_node<T, N>(q, b, c, s.n[QG_B_BC]);
        add_node<T, N>(im, p, q, s.n[QG_B_IM]);
        return;
    }
    T B[N];
    add_node<T, N>(p, c, d, s.n[QG_T_CD]);
    mul_node<T, N>(B, p, b, s.n[QG_T_B]);
    add_node<T, N>(p, a, b, s.n[QG_T_AB]);
    mul_node<T, N>(q, p, c, s.n[QG_T_A]);
    sub_node<T, N>(re, q, B, s.n[QG_T_RE]);
    sub_node<T, N>(p, b, a, s.n[QG_T_BA]);
    mul_node<T, N>(q, p, d, s.n[QG_T_C]);
    sub_node<T, N>(im, B, q, s.n[QG_T_IM]);
}

template <class T>
__global__ __launch_bounds__(256) void k_eltwise_cplx(QCplxPassArgs g)
{
    constexpr int R = QG_CPLX_RUN;
    const int64_t i0 = ((int64_t)blockIdx.x * 256 + threadIdx.x) * R;
    if (i0 >= g.n) return;
    const bool full = i0 + R <= g.n;
    const int cnt = full ? R : (int)(g.n - i0);
    T vr[R], vi[R];
    load_n<T, R>(g.C, i0, g.cbytes, full, cnt, vr);
    load_n<T, R>(g.C + g.n * g.cbytes, i0, g.cbytes, full, cnt, vi);
    const int n_st = g.t[0].n;
    for (int k = 0; k < n_st; ++k) {
        const QEpStage &sr = g.t[0].st[k], &si = g.t[1].st[k];
        T er[R], ei[R];
        const bool tr = sr.op != QG_EW_PASS && !sr.scalar, ti = si.op != QG_EW_PASS && !si.scalar;
        if (tr) {
            load_n<T, R>(g.a.e[k], i0, sr.ebytes, full, cnt, er);
        } else {
#pragma unroll
            for (int o = 0; o < R; ++o) er[o] = (T)g.a.scalar[k];
        }
        if (ti && (g.e_cplx[k] || !tr)) {
            load_n<T, R>(g.a.e[k] + (g.e_cplx[k] ? g.n * si.ebytes : 0), i0, si.ebytes, full, cnt, ei);
        } else if (ti) {   // a real tensor operand that both parts read: loaded once
#pragma unroll
            for (int o = 0; o < R; ++o) ei[o] = er[o];
        } else {
#pragma unroll
            for (int o = 0; o < R; ++o) ei[o] = (T)g.scalar_im[k];
        }
        if (sr.op != QG_EW_CMUL) {
            qg_ep_stage<T, R>(vr, er, sr);
            qg_ep_stage<T, R>(vi, ei, si);
            continue;
        }
        const QCmulStage& cm = g.cm[k];
        T re[R], im[R];
        if (cm.x_first) cmul_nodes<T, R>(re, im, vr, vi, er, ei, cm);
        else cmul_nodes<T, R>(re, im, er, ei, vr, vi, cm);
#pragma unroll
        for (int o = 0; o < R; ++o) { vr[o] = re[o]; vi[o] = im[o]; }
        qg_step_all<T, R>(vr, sr.cvt);
        qg_step_all<T, R>(vi, si.cvt);
    }
    qg_step_all<T, R>(vr, g.t[0].to_d);
    qg_step_all<T, R>(vi, g.t[1].to_d);
    const int db = g.t[0].dbytes;
    store_n<T, R>(g.D, i0, db, full, cnt, vr);
    store_n<T, R>(g.D + g.n * db, i0, db, full, cnt, vi);
}

} // namespace

hipError_t qg_launch_eltwise_cplx(const QCplxPassArgs& g, hipStream_t st)
{
    if (g.n <= 0) return hipSuccess;
    const int64_t per_block = 256 * QG_CPLX_RUN;
    const int64_t blocks = (g.n + per_block - 1) / per_block;
    if (blocks > 0x7fffffffll) return hipErrorInvalidValue;
    if (g.t[0].bits32) hipLaunchKernelGGL(k_eltwise_cplx<int32_t>, dim3((unsigned)blocks), dim3(256), 0, st, g);
    else hipLaunchKernelGGL(k_eltwise_cplx<int64_t>,dim3((unsigned)blocks), dim3(256), 0, st, g);
    return hipGetLastError();
}
