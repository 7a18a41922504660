// qg_approx_dev.h — device pieces of the pass that runs chains with an APPROX stage (qg_approx.hip: k_approx and its member forms
// k_approx_bd, k_approx_grp), where the stage itself is described.
#pragma once
#include "qg_approx.h"
#include "qg_eltwise.h"

namespace {

template <class T>
__device__ __forceinline__ T lds_word(const int64_t* p)
{
    if constexpr (sizeof(T) == 4) return (T) * (const int32_t*)p;   // little-endian low half: one ds_read_b32
    else return (T)*p;
}

template <class T>
__device__ __forceinline__ void approx_stage(T (&v)[16], const QApproxTable* __restrict__ tab, const int64_t* lds, bool general)
{
    const int64_t* thr = lds;
    const int64_t* coef = lds + QG_MAX_SEG;
    const int n_seg = tab->n_seg;
    int seg[16];
    {
        int alive[16];
#pragma unroll
        for (int o = 0; o < 16; ++o) { seg[o] = 0; alive[o] = 1; }
        for (int s = 0; s + 1 < n_seg; ++s) {
            const T t = lds_word<T>(thr + s);
#pragma unroll
            for (int o = 0; o < 16; ++o) {
                alive[o] &= (int)(v[o] >= t);
                seg[o] += alive[o];
            }
        }
    }
    T x[16];
#pragma unroll
    for (int o = 0; o < 16; ++o) x[o] = v[o];
    if (!general) {
        const QApproxSeg& S = tab->seg[0];
        const int n = S.n_coef;
#pragma unroll
        for (int o = 0; o < 16; ++o) v[o] = lds_word<T>(coef + (n - 1) * QG_MAX_SEG + seg[o]);
        for (int i = n - 2; i >= 0; --i) {
#pragma unroll
            for (int o = 0; o < 16; ++o) v[o] *= x[o];
            qg_step_all<T, 16>(v, S.lvl[i].mul);
#pragma unroll
            for (int o = 0; o < 16; ++o) v[o] += lds_word<T>(coef + i * QG_MAX_SEG + seg[o]);
            qg_step_all<T, 16>(v, S.lvl[i].add);
        }
        qg_step_all<T, 16>(v, S.to_x);
        return;
    }
    unsigned mine = 0;
#pragma unroll
    for (int o = 0; o < 16; ++o) mine |= 1u << seg[o];
    for (int s = 0; s < n_seg; ++s) {
        if (__ballot((mine >> s) & 1u) == 0) continue;   // wave-uniform: nobody in the wave is in this segment
        const QApproxSeg& S = tab->seg[s];
        const int n = S.n_coef;
        T r[16];
        const T top = lds_word<T>(coef + (n - 1) * QG_MAX_SEG + s);
#pragma unroll
        for (int o = 0; o < 16; ++o) r[o] = top;
        for (int i = n - 2; i >= 0; --i) {
            const T a = lds_word<T>(coef + i * QG_MAX_SEG + s);
#pragma unroll
            for (int o = 0; o < 16; ++o) r[o] *= x[o];
            qg_step_all<T, 16>(r, S.lvl[i].mul);
#pragma unroll
            for (int o = 0; o < 16; ++o) r[o] += a;
            qg_step_all<T, 16>(r, S.lvl[i].add);
        }
        qg_step_all<T, 16>(r, S.to_x);
#pragma unroll
        for (int o = 0; o < 16; ++o) v[o] = seg[o] == s ? r[o] : v[o];
    }
}

// 16 values starting at element idx; `full`: all 16 exist (16-byte loads), else the first `cnt` do and the rest read as 0 — a
// value of every format, so the lane's arithmetic on them stays defined; they are not stored
template <class T>
__device__ __forceinline__ void load16(const char* p, int64_t idx, int bytes, bool full, int cnt, T (&out)[16])
{
    if (full) {
#pragma unroll
        for (int q = 0; q < 4; ++q) qg_ep_load_run<4, T>(p, idx + 4 * q, bytes, out + 4 * q);
        return;
    }
#pragma unroll
    for (int o = 0; o < 16; ++o) out[o] = o < cnt ? (T)qg_ep_load_one(p, idx + o, bytes) : (T)0;
}

} // namespace
