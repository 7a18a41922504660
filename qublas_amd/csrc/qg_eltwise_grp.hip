// qg_eltwise_grp.hip — the element-wise chain of a grouped plan as ONE pass over the launch's packed C (gfx950): the grouped forms of
// k_eltwise (qg_eltwise.hip) and k_approx (qg_approx.hip), in the framing of k_eltwise_bd / k_approx_bd (qg_eltwise_bd.hip).
//
// The grouped GEMM launch (k_mfma_grp) leaves the packed Cs of the members in the launch back to back; D and every tensor operand
// have the same layout, so the pass is linear in memory: 16 consecutive elements per lane, 4096 per workgroup = one 64 x 64 tile, and
// a tile belongs to one member.  The members differ in size, so the workgroup's member is not a quotient: it is entry blockIdx.x of
// the plan's tile -> member table (qg_grp.h: qg_grp_tile_members), a wave-uniform load, and a per-member scalar stage reads the
// plan's table of raw values at that member (QGrpEp, qg_eltwise_args.h).  Nothing per lane depends on the member.
// There is no tail: the launch part is whole tiles (the launchers check it).
#include <hip/hip_runtime.h>

#include "qg_approx_dev.h"
#include "qg_eltwise.h"
#include "qg_grp_ep.h"

namespace {

__global__ __launch_bounds__(256) void k_eltwise_grp(QEltwiseGrpArgs a)
{
    const QEltwiseArgs& g = a.g;
    const int64_t i0 = (int64_t)blockIdx.x * 4096 + (int64_t)threadIdx.x * 16;
    if (i0 + 16 > g.n) return;
    const int member = a.tile_member[blockIdx.x];
    if (g.t.bits32) {
        int32_t v[16];
#pragma unroll
        for (int q = 0; q < 4; ++q) qg_ep_load_run<4, int32_t>(g.C, i0 + 4 * q, g.cbytes, v + 4 * q);
        qg_ep_apply_runs_grp<int32_t, 4>(v, g.t, g.a, (int64_t)blockIdx.x * 4096, threadIdx.x * 16u, 4, a.ge, member);
#pragma unroll
        for (int q = 0; q < 4; ++q) qg_ep_store_run<int32_t>(g.D, i0 + 4 * q, g.t.dbytes, v + 4 * q);
    } else {
        int64_t v[16];
#pragma unroll
        for (int q = 0; q < 4; ++q) qg_ep_load_run<4, int64_t>(g.C, i0 + 4 * q, g.cbytes, v + 4 * q);
        qg_ep_apply_runs_grp<int64_t, 4>(v, g.t, g.a, (int64_t)blockIdx.x * 4096, threadIdx.x * 16u, 4, a.ge, member);
#pragma unroll
        for (int q = 0; q < 4; ++q) qg_ep_store_run<int64_t>(g.D, i0 + 4 * q, g.t.dbytes, v + 4 * q);
    }
}

template <class T>
__global__ __launch_bounds__(256) void k_approx_grp(QApproxGrpArgs a)
{
    __shared__ int64_t tabs[QG_MAX_EW][QG_APPROX_LDS_WORDS];
    const QEltwiseArgs& g = a.x.g;
    for (int k = 0; k < g.t.n; ++k) {
        if (!a.x.ax[k]) continue;
        const int64_t* src = a.x.ax[k]->thr;
        for (int i = threadIdx.x; i < QG_APPROX_LDS_WORDS; i += 256) tabs[k][i] = src[i];
    }
    __syncthreads();
    const int64_t i0 = (int64_t)blockIdx.x * 4096 + (int64_t)threadIdx.x * 16;
    if (i0 + 16 > g.n) return;
    const int member = a.tile_member[blockIdx.x];
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
            const int64_t* tab = a.ge.scal[k];
            const int64_t sc = tab ? tab[member] : g.a.scalar[k];
#pragma unroll
            for (int o = 0; o < 16; ++o) e[o] = (T)sc;
        } else {
            load16<T>(g.a.e[k], i0, s.ebytes, true, 16, e);
        }
        qg_ep_stage<T, 16>(v, e, s);
    }
    qg_step_all<T, 16>(v, g.t.to_d);
#pragma unroll
    for (int q = 0; q < 4; ++q) qg_ep_store_run<T>(g.D, i0 + 4 * q, g.t.dbytes, v + 4 * q);
}

// the launch part: whole 64 x 64 tiles, one per workgroup, each with its entry in the tile -> member table
bool launch_ok(int64_t n, const int32_t* tile_member) { return tile_member && n % 4096 == 0 && n / 4096 <= 0x7fffffffll; }

} // namespace

hipError_t qg_launch_eltwise_grp(const QEltwiseGrpArgs& a, hipStream_t st)
{
    if (a.g.n <= 0) return hipSuccess;
    if (!launch_ok(a.g.n, a.tile_member)) return hipErrorInvalidValue;
    hipLaunchKernelGGL(k_eltwise_grp, dim3((unsigned)(a.g.n / 4096)), dim3(256), 0, st, a);
    return hipGetLastError();
}

hipError_t qg_launch_approx_grp(const QApproxGrpArgs& a, hipStream_t st)
{
    const int64_t n = a.x.g.n;
    if (n <= 0) return hipSuccess;
    if (!launch_ok(n, a.tile_member)) return hipErrorInvalidValue;
    if (a.x.g.t.bits32) hipLaunchKernelGGL(k_approx_grp<int32_t>, dim3((unsigned)(n / 4096)), dim3(256), 0, st, a);
    else hipLaunchKernelGGL(k_approx_grp<int64_t>, dim3((unsigned)(n / 4096)), dim3(256), 0, st, a);
    return hipGetLastError();
}
