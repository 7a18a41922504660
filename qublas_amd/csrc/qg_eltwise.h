// qg_eltwise.h — device side of the fused element-wise epilogue (include/qgemul.h, qgemul_epilogue).
//
// The reference evaluates  D[i] = cvt_DT( Qop_n<..>( ... Qop_1<..>(C[i], e_1[i]) ..., e_n[i]) )  one element at a
// time through its lazy tensor expressions (/root/reference/include/QuBLAS.h:3780-3877, :4079-4100, tensor
// construction :2732-2746).  Here the chain runs on a small register array of values the GEMM kernel has just
// converted into C's element type; the (wave-uniform) op and mode switches are hoisted out of the per-element loops
// exactly as in qg_step_all.h.  All arithmetic is 64-bit: the planner has bounded every intermediate by 62 bits.
#pragma once
#include "qg_eltwise_args.h"
#include "qg_step_all.h"

// RUN consecutive packed elements starting at element index idx
template <int RUN, class T>
__device__ __forceinline__ void qg_ep_load_run(const char* p, int64_t idx, int ebytes, T* out)
{
    static_assert(RUN == 4, "the MFMA C/D layouts give every lane runs of 4 consecutive rows");
    switch (ebytes) {
    case 1: {
        const uint32_t w = *(const uint32_t*)(p + idx);
#pragma unroll
        for (int r = 0; r < 4; ++r) out[r] = (T)(int8_t)(w >> (8 * r));
        break;
    }
    case 2: {
        const uint2 w = *(const uint2*)(p + idx * 2);
        out[0] = (T)(int16_t)(w.x & 0xffff);
        out[1] = (T)(int16_t)(w.x >> 16);
        out[2] = (T)(int16_t)(w.y & 0xffff);
        out[3] = (T)(int16_t)(w.y >> 16);
        break;
    }
    case 4: {
        const int4 w = *(const int4*)(p + idx * 4);
        out[0] = w.x; out[1] = w.y; out[2] = w.z; out[3] = w.w;
        break;
    }
    default: {
        const longlong2 a = *(const longlong2*)(p + idx * 8), b = *(const longlong2*)(p + idx * 8 + 16);
        out[0] = (T)a.x; out[1] = (T)a.y; out[2] = (T)b.x; out[3] = (T)b.y;
        break;
    }
    }
}

__device__ __forceinline__ int64_t qg_ep_load_one(const char* p, int64_t idx, int ebytes)
{
    switch (ebytes) {
    case 1: return ((const int8_t*)p)[idx];
    case 2: return ((const int16_t*)p)[idx];
    case 4: return ((const int32_t*)p)[idx];
    default: return ((const int64_t*)p)[idx];
    }
}

// one stage on N values: v = Qop(v, e) or Qop(e, v), rounded / overflowed into the stage's format
template <class T, int N>
__device__ __forceinline__ void qg_ep_stage(T (&v)[N], const T (&e)[N], const QEpStage& s)
{
    if (s.op == QG_EW_PASS) {
        qg_step_all<T, N>(v, s.cvt);
        return;
    }
    if (s.op == QG_EW_MUL) {
#pragma unroll
        for (int o = 0; o < N; ++o) v[o] *= e[o];
    } else {
        const int sx = s.x_first ? s.node.sa : s.node.sb, se = s.x_first ? s.node.sb : s.node.sa;
        if (s.op == QG_EW_ADD) {
#pragma unroll
            for (int o = 0; o < N; ++o) v[o] = qg_shl<T>(v[o], sx) + qg_shl<T>(e[o], se);
        } else if (s.x_first) {
#pragma unroll
            for (int o = 0; o < N; ++o) v[o] = qg_shl<T>(v[o], sx) - qg_shl<T>(e[o], se);
        } else {
#pragma unroll
            for (int o = 0; o < N; ++o) v[o] = qg_shl<T>(e[o], se) - qg_shl<T>(v[o], sx);
        }
    }
    qg_step_all<T, N>(v, s.node.q);
    qg_step_all<T, N>(v, s.cvt);
}

// Where a stage's operand comes from.  The stage loop below asks a source two things: stage k's scalar, and run q (4 consecutive
// packed elements) of stage k's tensor operand.  There are three, one per launch form; a fourth form (say, members addressed through a
// pointer table) is a fourth struct here with the same two members, and neither the loop nor the stages change.
//
// ONE GEMM: the index as given, run q at idx0 + q * stride; the call-wide scalar.
struct QEpSrcOne {
    const QEpArgs& a;
    int64_t idx0, stride;
    __device__ __forceinline__ int64_t scalar(int k) const { return a.scalar[k]; }
    template <class T>
    __device__ __forceinline__ void run(int k, int q, int ebytes, T* out) const { qg_ep_load_run<4, T>(a.e[k], idx0 + q * stride, ebytes, out); }
};
// A MEMBER OF A STACK (the block-diagonal forms of a batched plan; QBdEp): idx0 runs over the whole stack; stage k's tensor operand is
// read there too unless bit k of `shared` is set: a shared operand is one member's tensor, read `member_off` elements lower
struct QEpSrcStack {
    const QEpArgs& a;
    int64_t idx0, stride, member_off;
    uint32_t shared;
    __device__ __forceinline__ int64_t scalar(int k) const { return a.scalar[k]; }
    template <class T>
    __device__ __forceinline__ void run(int k, int q, int ebytes, T* out) const
    {
        const int64_t i0 = ((shared >> k) & 1u) ? idx0 - member_off : idx0;
        qg_ep_load_run<4, T>(a.e[k], i0 + q * stride, ebytes, out);
    }
};
// A MEMBER OF A GROUPED LAUNCH (QGrpEp): the element index runs over the whole launch, as D and every tensor operand do, and comes in
// two parts: ubase, wave-uniform (the workgroup's tile), which goes into the operand's base pointer, and the lane's 32-bit index lane0
// behind it; run q starts at lane0 + q * stride.  A scalar stage with a table takes the table's entry of `member` (wave-uniform, like
// the table pointer: a scalar load)
struct QEpSrcGroup {
    const QEpArgs& a;
    int64_t ubase;
    uint32_t lane0, stride;
    const QGrpEp& ge;
    int member;
    __device__ __forceinline__ int64_t scalar(int k) const
    {
        const int64_t* tab = ge.scal[k];
        const int64_t raw = tab ? tab[member] : a.scalar[k];
        // (wave-uniform by construction; said so, so that the value lives in scalar registers like a call-wide scalar does)
        return (int64_t)(((uint64_t)(uint32_t)__builtin_amdgcn_readfirstlane((int)(raw >> 32)) << 32) | (uint32_t)__builtin_amdgcn_readfirstlane((int)raw));
    }
    template <class T>
    __device__ __forceinline__ void run(int k, int q, int ebytes, T* out) const
    {
        // (the lane's BYTE offset in 32 bits as well: one register per run instead of a 64-bit pair per run and container)
        const char* p = a.e[k] + ubase * ebytes;
        qg_ep_load_run<4, T>(p + (lane0 + q * stride) * (uint32_t)ebytes, 0, ebytes, out);
    }
};

// the whole chain on NR runs of 4 consecutive packed elements, the operands from `src`.  (The operand is fetched here, in the loop's
// own body, and src is taken by reference: as a function of its own the fetch moved the instruction streams of the fused MFMA kernels.)
// T = int32_t when the planner has bounded the whole chain by 32 bits (QEpTable::bits32), else int64_t
template <class T, int NR, class Src>
__device__ __forceinline__ void qg_ep_apply_runs(T (&v)[4 * NR], const QEpTable& t, const Src& src)
{
    for (int k = 0; k < t.n; ++k) {
        T e[4 * NR];
        if (t.st[k].scalar) {
#pragma unroll
            for (int o = 0; o < 4 * NR; ++o) e[o] = (T)src.scalar(k);
        } else {
#pragma unroll
            for (int q = 0; q < NR; ++q) src.template run<T>(k, q, t.st[k].ebytes, e + 4 * q);
        }
        qg_ep_stage<T, 4 * NR>(v, e, t.st[k]);
    }
    qg_step_all<T, 4 * NR>(v, t.to_d);
}

// RUN consecutive packed elements of `bytes` each, starting at element index idx
template <class T>
__device__ __forceinline__ void qg_ep_store_run(char* D, int64_t idx, int bytes, const T* v)
{
    switch (bytes) {
    case 1:
        *(uint32_t*)(D + idx) = (uint32_t)(v[0] & 0xff) | ((uint32_t)(v[1] & 0xff) << 8) | ((uint32_t)(v[2] & 0xff) << 16) | ((uint32_t)(v[3] & 0xff) << 24);
        break;
    case 2:
        *(uint2*)(D + idx * 2) = make_uint2((uint32_t)(v[0] & 0xffff) | ((uint32_t)(v[1] & 0xffff) << 16), (uint32_t)(v[2] & 0xffff) | ((uint32_t)(v[3] & 0xffff) << 16));
        break;
    case 4:
        *(int4*)(D + idx * 4) = make_int4((int)v[0], (int)v[1], (int)v[2], (int)v[3]);
        break;
    default: {
        int64_t* p = (int64_t*)(D + idx * 8);
        *(longlong2*)p = make_longlong2((int64_t)v[0], (int64_t)v[1]);
        *(longlong2*)(p + 2) = make_longlong2((int64_t)v[2], (int64_t)v[3]);
        break;
    }
    }
}

__device__ __forceinline__ void qg_ep_store_one(char* dst, int64_t idx, int bytes, int64_t v)
{
    switch (bytes) {
    case 1: ((int8_t*)dst)[idx] = (int8_t)v; break;
    case 2: ((int16_t*)dst)[idx] = (int16_t)v; break;
    case 4: ((int32_t*)dst)[idx] = (int32_t)v; break;
    default: ((int64_t*)dst)[idx] = v; break;
    }
}

// The sources of the stand-alone passes (qg_eltwise.hip, qg_approx.hip): 4096 consecutive elements per workgroup, 16 per lane from
// i0 = blockIdx.x * 4096 + threadIdx.x * 16 on, 4 runs of 4.  What differs is how a workgroup finds its member:
// no member at all (one GEMM's packed C)
__device__ __forceinline__ QEpSrcOne qg_pass_src(const QEltwiseArgs& g, int64_t i0) { return QEpSrcOne{g.a, i0, 4}; }
// a stack: a member's packed C is a whole number of 64 x 64 tiles = of workgroups, so a workgroup never straddles two members and its
// member is the quotient (blockIdx.x * 4096) / msize, wave-uniform
__device__ __forceinline__ QEpSrcStack qg_pass_src(const QEltwiseArgs& g, const QBdEp& bd, int64_t i0)
{
    return QEpSrcStack{g.a, i0, 4, (int64_t)blockIdx.x * 4096 / bd.msize * bd.msize, bd.shared};
}
// a grouped launch: the members differ in size, so the member is entry blockIdx.x of the plan's tile -> member table (qg_grp.h:
// qg_grp_tile_members), a wave-uniform load; nothing per lane depends on the member
__device__ __forceinline__ QEpSrcGroup qg_pass_src(const QEltwiseArgs& g, const QGrpEp& ge, const int32_t* tile_member)
{
    return QEpSrcGroup{g.a, (int64_t)blockIdx.x * 4096, threadIdx.x * 16u, 4, ge, tile_member[blockIdx.x]};
}
