// qg_eltwise_bd.hip — the element-wise chain of a batched plan as ONE pass over the whole stack (gfx950): the block-diagonal forms
// of k_eltwise (qg_eltwise.hip) and k_approx (qg_approx.hip).
//
// The block-diagonal GEMM launch (k_mfma_bd) leaves the members' packed Cs back to back; D and every per-member tensor operand
// have the same layout, so the pass is linear in memory over batch * msize elements exactly as k_eltwise is over one C: 16
// consecutive elements per lane, 4096 per workgroup.  A member's packed C is a whole number of 64 x 64 tiles = of workgroups, so a
// workgroup never straddles two members: its member number is  (blockIdx.x * 4096) / msize,  wave-uniform, and a SHARED operand
// (ONE member's packed tensor for the whole batch: a bias) is read at the member-local index  i - member * msize.  It is not
// replicated when it is packed: for 1024 members of 64 x 64 that would add as many bytes as C itself.
// There is no tail: the element count is a multiple of 4096 (the launchers check it).
#include <hip/hip_runtime.h>

#include "qg_approx_dev.h"
#include "qg_bd_ep.h"
#include "qg_eltwise.h"

namespace {

__global__ __launch_bounds__(256) void k_eltwise_bd(QEltwiseBdArgs a)
{
    const QEltwiseArgs& g = a.g;
    const int64_t w0 = (int64_t)blockIdx.x * 4096;
    const int64_t member_off = w0 / a.bd.msize * a.bd.msize;
    const int64_t i0 = w0 + (int64_t)threadIdx.x * 16;
    if (i0 + 16 > g.n) return;
    if (g.t.bits32) {
        int32_t v[16];
#pragma unroll
        for (int q = 0; q < 4; ++q) qg_ep_load_run<4, int32_t>(g.C, i0 + 4 * q, g.cbytes, v + 4 * q);
        qg_ep_apply_runs_bd<int32_t, 4>(v, g.t, g.a, i0, 4, member_off, a.bd.shared);
#pragma unroll
        for (int q = 0; q < 4; ++q) qg_ep_store_run<int32_t>(g.D, i0 + 4 * q, g.t.dbytes, v + 4 * q);
    } else {
        int64_t v[16];
#pragma unroll
        for (int q = 0; q < 4; ++q) qg_ep_load_run<4, int64_t>(g.C, i0 + 4 * q, g.cbytes, v + 4 * q);
        qg_ep_apply_runs_bd<int64_t, 4>(v, g.t, g.a, i0, 4, member_off, a.bd.shared);
#pragma unroll
        for (int q = 0; q < 4; ++q) qg_ep_store_run<int64_t>(g.D, i0 + 4 * q, g.t.dbytes, v + 4 * q);
    }
}

template <class T>
__global__ __launch_bounds__(256) void k_approx_bd(QApproxBdArgs a)
{
    __shared__ int64_t tabs[QG_MAX_EW][QG_APPROX_LDS_WORDS];
    const QEltwiseArgs& g = a.x.g;
    for (int k = 0; k < g.t.n; ++k) {
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

// the stack: a whole number of members, a member a whole number of workgroups
bool stack_ok(int64_t n, const QBdEp& bd) { return bd.msize > 0 && bd.msize % 4096 == 0 && n % bd.msize == 0 && n / 4096 <= 0x7fffffffll; }

} // namespace

hipError_t qg_launch_eltwise_bd(const QEltwiseBdArgs& a, hipStream_t st)
{
    if (a.g.n <= 0) return hipSuccess;
    if (!stack_ok(a.g.n, a.bd)) return hipErrorInvalidValue;
    hipLaunchKernelGGL(k_eltwise_bd, dim3((unsigned)(a.g.n / 4096)), dim3(256), 0, st, a);
    return hipGetLastError();
}

hipError_t qg_launch_approx_bd(const QApproxBdArgs& a, hipStream_t st)
{
    const int64_t n = a.x.g.n;
    if (n <= 0) return hipSuccess;
    if (!stack_ok(n, a.bd)) return hipErrorInvalidValue;
    if (a.x.g.t.bits32) hipLaunchKernelGGL(k_approx_bd<int32_t>, dim3((unsigned)(n / 4096)), dim3(256), 0, st, a);
    else hipLaunchKernelGGL(k_approx_bd<int64_t>, dim3((unsigned)(n / 4096)), dim3(256), 0, st, a);
    return hipGetLastError();
}
