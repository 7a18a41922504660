// qg_combine_bd.hip — the second launch of a STACKED batched plan (QG_OPT_BATCHED_STACKED; qg_geom.h: QBatchGeom::stack_ws).  The
// block-diagonal GEMM launch (k_mfma_bd, identity epilogue, 8-byte containers) has left the raw dot products of every member's stacked
// parts in the plan's workspace: bd_tm x bd_tn tiles of 64 x 64 int64 per member, tile (r, c) of member b at
// ((b * bd_tm + r) * bd_tn + c) * 4096 elements, element (i, j) inside it at j * 64 + i (the MFMA kernels' packed-C tile).  k_stack_combine_bd
// turns them into the members' packed Cs, [2][M][N] row-major in C's container, back to back at cstride bytes: the arithmetic of
// k_cplx_combine / k_rc_convert (qg_pack.hip), which stay the plain plans' passes.
//
// One workgroup per 64 x 64 OUTPUT tile of a member (batch * tm * tn workgroups; tm, tn: the tiles of ONE part), member and tile from
// the block id alone (qg_bd_tile_of; scalar registers).  Per part the workgroup reads its source tiles — complex: two products per
// part, (lm, ln) and (lm + tm, ln + tn) for re, (lm, ln + tn) and (lm + tm, ln) for im; mixed: one, the imaginary product (im_r, im_c)
// tiles behind the real one — with 16-byte loads along i, combines, rounds and overflow-handles once per part, and transposes the tile
// through LDS so that the stores run along n, the contiguous axis of packed C.  No per-element division: every index is a shift or a
// mask of the lane id.
//   loads   a wave covers 16 rows x 8 columns per instruction: 8 lanes along i (one 128-byte line of a column), 8 lanes along j
//   LDS     int64 t[64][65] (33 280 bytes).  Writes (ds_write_b64: 16-lane groups, banks (a / 4) % 32): lane (li, lj) of a group
//           holds t[16 ib + 2 li (+ 1)][8 jb + lj] at dword 130 (16 ib + 2 li) + 2 (8 jb + lj) = const + 4 li + 2 lj (mod 32), li < 8,
//           lj < 2: sixteen distinct even dwords, all 32 banks once.  Reads (ds_read_b64: 32-lane halves, banks (a / 4) % 64): a
//           wave reads one row, 64 consecutive int64: every bank once per half.  Conflict-free both ways.
//   stores  a wave writes 64 consecutive containers of one row of C: coalesced whatever C's alignment (a member's C is 256-byte
//           aligned, its row pitch N * cbytes is arbitrary: element-wise stores, no vector store that could straddle)
#include <hip/hip_runtime.h>

#include "qg_kernels.h"
#include "qg_tile_walk.h"

namespace {

__device__ __forceinline__ void store_container(char* dst, int64_t idx, int cbytes, int64_t v)
{
    switch (cbytes) {
    case 1: ((int8_t*)dst)[idx] = (int8_t)v; break;
    case 2: ((int16_t*)dst)[idx] = (int16_t)v; break;
    case 4: ((int32_t*)dst)[idx] = (int32_t)v; break;
    default: ((int64_t*)dst)[idx] = v; break;
    }
}

// CPLX: complex x complex members (four quadrant products); else one real and one complex operand (two products)
template <bool CPLX>
__global__ __launch_bounds__(256) void k_stack_combine_bd(QStackCombine g)
{
    constexpr int T = 64, PITCH = T + 1, TILE = T * T;
    __shared__ int64_t t[T][PITCH];
    int member, lm, ln;
    qg_bd_tile_of<int>((int)blockIdx.x, g.tm, g.tn, member, lm, ln);
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int li = lane & 7, lj = lane >> 3;
    const int64_t* const W = g.W + (int64_t)member * g.bd_tm * g.bd_tn * TILE;   // the member's block of the workspace
    auto tile = [&](int r, int c) { return W + ((int64_t)r * g.bd_tn + c) * TILE; };
    char* const Cm = g.C + (int64_t)member * g.cstride;
    const int64_t m0 = (int64_t)lm * T, n0 = (int64_t)ln * T;
#pragma unroll 1
    for (int part = 0; part < 2; ++part) {
        int r0, c0, r1 = 0, c1 = 0;
        qg_stack_src_tile(CPLX, part, 0, lm, ln, g.tm, g.tn, g.im_r, g.im_c, r0, c0);                      // P1 = re re | P3 = re im; mixed: the part's product
        if constexpr (CPLX) qg_stack_src_tile(true, part, 1, lm, ln, g.tm, g.tn, 0, 0, r1, c1);            // P2 = im im | P4 = im re
        const int64_t* const s0 = tile(r0, c0);
        const int64_t* const s1 = tile(r1, c1);
        const int sh0 = g.sh[2 * part], sh1 = g.sh[2 * part + 1];
        const QStep st = g.to_c[part];
        longlong2 a[8], b[8];
#pragma unroll
        for (int q = 0; q < 8; ++q) {   // wave-iteration q * 4 + wave: rows 16 ib + 2 li (+ 1), column 8 jb + lj
            const int blk = q * 4 + wave, ib = blk & 3, jb = blk >> 2;
            const int off = (jb * 8 + lj) * T + ib * 16 + 2 * li;
            a[q] = *(const longlong2*)(s0 + off);
            if constexpr (CPLX) b[q] = *(const longlong2*)(s1 + off);
        }
        if (part) __syncthreads();   // (the stores of part 0 have read the tile)
#pragma unroll
        for (int q = 0; q < 8; ++q) {
            const int blk = q * 4 + wave, ib = blk & 3, jb = blk >> 2;
            int64_t x = a[q].x, y = a[q].y;
            if constexpr (CPLX) {
                const int64_t bx = qg_shl<int64_t>(b[q].x, sh1), by = qg_shl<int64_t>(b[q].y, sh1);
                x = qg_shl<int64_t>(x, sh0);
                y = qg_shl<int64_t>(y, sh0);
                x = part ? x + bx : x - bx;
                y = part ? y + by : y - by;
            }
            t[ib * 16 + 2 * li][jb * 8 + lj] = qg_step<int64_t>(x, st);
            t[ib * 16 + 2 * li + 1][jb * 8 + lj] = qg_step<int64_t>(y, st);
        }
        __syncthreads();
        char* const Cp = Cm + (int64_t)part * g.M * g.N * g.cbytes;
        const int64_t n = n0 + lane;
#pragma unroll 4
        for (int r = 0; r < 16; ++r) {
            const int i = r * 4 + wave;
            const int64_t m = m0 + i;
            if (m < g.M && n < g.N) store_container(Cp, m * g.N + n, g.cbytes, t[i][lane]);   // rows and columns beyond M, N are not written
        }
    }
}

}   // namespace

hipError_t qg_launch_stack_combine_bd(const QStackCombine& g, int64_t batch, hipStream_t st)
{
    const int64_t blocks = batch * g.tm * g.tn;
    if (blocks <= 0 || g.M <= 0 || g.N <= 0) return hipSuccess;
    // the geometry the kernel relies on: one part's tiles cover M x N, the member's block holds the source tiles of every mode
    const bool cplx = g.mode == QG_STACK_CPLX;
    const int im_r = g.mode == QG_STACK_REAL_B ? g.tm : 0, im_c = g.mode == QG_STACK_REAL_A ? g.tn : 0;
    if (blocks > 0x7fffffffll || g.tm < 1 || g.tn < 1 || (int64_t)g.tm * 64 < g.M || (int64_t)g.tn * 64 < g.N || g.cstride < 2 * g.M * g.N * g.cbytes ||
        (g.cbytes != 1 && g.cbytes != 2 && g.cbytes != 4 && g.cbytes != 8) || (g.mode != QG_STACK_CPLX && g.mode != QG_STACK_REAL_A && g.mode != QG_STACK_REAL_B) ||
        g.bd_tm != (cplx ? 2 * g.tm : g.tm + im_r) || g.bd_tn != (cplx ? 2 * g.tn : g.tn + im_c) || g.im_r != im_r || g.im_c != im_c)
        return hipErrorInvalidValue;
    if (cplx) hipLaunchKernelGGL(k_stack_combine_bd<true>, dim3((unsigned)blocks), dim3(256), 0, st, g);
    else hipLaunchKernelGGL(k_stack_combine_bd<false>, dim3((unsigned)blocks), dim3(256), 0, st, g);
    return hipGetLastError();
}
