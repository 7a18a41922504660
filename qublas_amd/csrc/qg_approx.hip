// qg_approx.hip — element-wise chains with a piecewise-polynomial activation stage (QG_EW_APPROX; the reference's ANUS::Qapprox,
// QuBLAS.h:4829-4897) as ONE pass over packed C -> packed D (gfx950).
//
// k_eltwise's framing (qg_eltwise.hip): C, the tensor operands and D share the plan's packed-C index space, every lane handles 16
// consecutive elements with 16-byte loads and stores, and the arithmetic is 32-bit where the planner has bounded the whole chain
// (QEpTable::bits32), 64-bit otherwise.  The plain stages are qg_ep_stage, unchanged.
//
// The APPROX stage, per lane on its 16 values:
//   * thresholds and coefficients of every table (1152 bytes each) sit in LDS.  The segment index is the number of LEADING
//     thresholds the value has reached: 2 VALU instructions per threshold and value, no branch; a threshold read is a broadcast;
//   * UNIFORM table (one format per Horner level for all segments — a datapath with a coefficient LUT): one Horner loop; the step
//     records are wave-uniform (scalar loads, qg_step_all), only the coefficient is per lane: coef[level][segment] — the at most
//     16 distinct addresses of one fetch are consecutive words, i.e. distinct LDS banks, equal addresses broadcast: conflict-free;
//   * GENERAL table (formats differ between segments): the segments present in the wave (ballot) one after the other, each with
//     its own wave-uniform steps and broadcast coefficients, the result kept where the lane's segment index matches.  The planner
//     has bounded every segment's chain on x's WHOLE range, so the values a lane computes for a segment that is not its own
//     stay inside the arithmetic as well.
#include <hip/hip_runtime.h>

#include <stddef.h>

#include "qg_approx.h"
#include "qg_approx_dev.h"
#include "qg_eltwise.h"

namespace {

static_assert(offsetof(QApproxTable, coef) == offsetof(QApproxTable, thr) + sizeof(int64_t) * QG_MAX_SEG, "thr and coef are copied to LDS as one block");

// the pass in k_eltwise's three framings (qg_eltwise.hip: eltwise_pass): src_of(i0) is the lane's operand source, TAIL: n need not be
// a multiple of 16
template <class T, bool TAIL, class SrcOf>
__device__ __forceinline__ void approx_pass(const QApproxArgs& a, SrcOf src_of)
{
    __shared__ int64_t tabs[QG_MAX_EW][QG_APPROX_LDS_WORDS];
    const QEltwiseArgs& g = a.g;
    for (int k = 0; k < g.t.n; ++k) {
        if (!a.ax[k]) continue;
        const int64_t* src = a.ax[k]->thr;
        for (int i = threadIdx.x; i < QG_APPROX_LDS_WORDS; i += 256) tabs[k][i] = src[i];
    }
    __syncthreads();
    const int64_t i0 = ((int64_t)blockIdx.x * 256 + threadIdx.x) * 16;
    if (TAIL ? i0 >= g.n : i0 + 16 > g.n) return;
    const bool full = !TAIL || i0 + 16 <= g.n;
    const int cnt = full ? 16 : (int)(g.n - i0);
    const auto src = src_of(i0);
    T v[16];
    load16<T>(g.C, i0, g.cbytes, full, cnt, v);
    for (int k = 0; k < g.t.n; ++k) {
        const QEpStage& s = g.t.st[k];
        if (s.op == QG_EW_APPROX) {
            approx_stage<T>(v, a.ax[k], tabs[k], a.force_general || !a.ax[k]->uniform);
            qg_step_all<T, 16>(v, s.cvt);
            continue;
        }
        T e[16];
        if (s.scalar) {
#pragma unroll
            for (int o = 0; o < 16; ++o) e[o] = (T)src.scalar(k);
        } else if (TAIL && !full) {   // (a tail: one GEMM's packed C, no member)
            load16<T>(g.a.e[k], i0, s.ebytes, false, cnt, e);
        } else {
#pragma unroll
            for (int q = 0; q < 4; ++q) src.template run<T>(k, q, s.ebytes, e + 4 * q);
        }
        qg_ep_stage<T, 16>(v, e, s);
    }
    qg_step_all<T, 16>(v, g.t.to_d);
    if (full) {
#pragma unroll
        for (int q = 0; q < 4; ++q) qg_ep_store_run<T>(g.D, i0 + 4 * q, g.t.dbytes, v + 4 * q);
        return;
    }
#pragma unroll
    for (int o = 0; o < 16; ++o)
        if (o < cnt) qg_ep_store_one(g.D, i0 + o, g.t.dbytes, (int64_t)v[o]);
}

template <class T>
__global__ __launch_bounds__(256) void k_approx(QApproxArgs a)
{
    approx_pass<T, true>(a, [&](int64_t i0) { return qg_pass_src(a.g, i0); });
}
// (the stack form keeps the body it had, instruction for instruction: as approx_pass with the stack's source its code differed and its
// pass measured up to 1.3 % over the former build's on 256 and 1024 members of 64^3, beyond the spread of the repetitions.  Two of
// those points stay 1 % over with this body as well — profiles/ep_member_forms_ab.jsonl — so the shared body is not shown to be the cause)
template <class T>
__global__ __launch_bounds__(256) void k_approx_bd(QApproxBdArgs a)
{
    __shared__ int64_t tabs[QG_MAX_EW][QG_APPROX_LDS_WORDS];
    const QEltwiseArgs& g = a.x.g;
    for (int k = 0; k < g.t.n; ++k) {   // (approx_pass's table copy, written out here too: as a shared function it moved four instructions in every approx kernel)
        if (!a.x.ax[k]) continue;
        const int64_t* src = a.x.ax[k]->thr;
        for (int i = threadIdx.x; i < QG_APPROX_LDS_WORDS; i += 256) tabs[k][i] = src[i];
    }
    __syncthreads();
    const int64_t w0 = (int64_t)blockIdx.x * 4096;
    const int64_t member_off = w0 / a.bd.msize * a.bd.msize;
    const int64_t i0 = w0 + (int64_t)threadIdx.x * 16;
    if (i0 + 16 > g.n) return;
    T v[16];
    load16<T>(g.C, i0, g.cbytes, true, 16, v);
    for (int k = 0; k < g.t.n; ++k) {
        const QEpStage& s = g.t.st[k];
        if (s.op == QG_EW_APPROX) {
            approx_stage<T>(v, a.x.ax[k], tabs[k], a.x.force_general || !a.x.ax[k]->uniform);
            qg_step_all<T, 16>(v, s.cvt);
            continue;
        }
        T e[16];
        if (s.scalar) {
#pragma unroll
            for (int o = 0; o < 16; ++o) e[o] = (T)g.a.scalar[k];
        } else {
            load16<T>(g.a.e[k], ((a.bd.shared >> k) & 1u) ? i0 - member_off : i0, s.ebytes, true, 16, e);
        }
        qg_ep_stage<T, 16>(v, e, s);
    }
    qg_step_all<T, 16>(v, g.t.to_d);
#pragma unroll
    for (int q = 0; q < 4; ++q) qg_ep_store_run<T>(g.D, i0 + 4 * q, g.t.dbytes, v + 4 * q);
}
template <class T>
__global__ __launch_bounds__(256) void k_approx_grp(QApproxGrpArgs a)
{
    approx_pass<T, false>(a.x, [&](int64_t) { return qg_pass_src(a.x.g, a.ge, a.tile_member); });
}

} // namespace

hipError_t qg_launch_approx(const QApproxArgs& a, hipStream_t st)
{
    if (a.g.n <= 0) return hipSuccess;
    const int64_t blocks = (a.g.n + 4095) / 4096;
    if (blocks > 0x7fffffffll) return hipErrorInvalidValue;
    if (a.g.t.bits32) hipLaunchKernelGGL(k_approx<int32_t>, dim3((unsigned)blocks), dim3(256), 0, st, a);
    else hipLaunchKernelGGL(k_approx<int64_t>, dim3((unsigned)blocks), dim3(256), 0, st, a);
    return hipGetLastError();
}

hipError_t qg_launch_approx_bd(const QApproxBdArgs& a, hipStream_t st)
{
    const int64_t n = a.x.g.n;
    if (n <= 0) return hipSuccess;
    if (!qg_pass_stack_ok(n, a.bd)) return hipErrorInvalidValue;
    if (a.x.g.t.bits32) hipLaunchKernelGGL(k_approx_bd<int32_t>, dim3((unsigned)(n / 4096)), dim3(256), 0, st, a);
    else hipLaunchKernelGGL(k_approx_bd<int64_t>, dim3((unsigned)(n / 4096)), dim3(256), 0, st, a);
    return hipGetLastError();
}

hipError_t qg_launch_approx_grp(const QApproxGrpArgs& a, hipStream_t st)
{
    const int64_t n = a.x.g.n;
    if (n <= 0) return hipSuccess;
    if (!qg_pass_launch_ok(n, a.tile_member)) return hipErrorInvalidValue;
    if (a.x.g.t.bits32) hipLaunchKernelGGL(k_approx_grp<int32_t>, dim3((unsigned)(n / 4096)), dim3(256), 0, st, a);
    else hipLaunchKernelGGL(k_approx_grp<int64_t>, dim3((unsigned)(n / 4096)), dim3(256), 0, st, a);
    return hipGetLastError();
}
