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

__device__ __forceinline__ void store_one(char* dst, int64_t idx, int bytes, int64_t v)
{
    switch (bytes) {
    case 1: ((int8_t*)dst)[idx] = (int8_t)v; break;
    case 2: ((int16_t*)dst)[idx] = (int16_t)v; break;
    case 4: ((int32_t*)dst)[idx] = (int32_t)v; break;
    default: ((int64_t*)dst)[idx] = v; break;
    }
}

template <class T>
__global__ __launch_bounds__(256) void k_approx(QApproxArgs a)
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
    if (i0 >= g.n) return;
    const bool full = i0 + 16 <= g.n;
    const int cnt = full ? 16 : (int)(g.n - i0);
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
            for (int o = 0; o < 16; ++o) e[o] = (T)g.a.scalar[k];
        } else {
            load16<T>(g.a.e[k], i0, s.ebytes, full, cnt, e);
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
        if (o < cnt) store_one(g.D, i0 + o, g.t.dbytes, (int64_t)v[o]);
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
