// qg_tree_bd.h — the batched twins of the tiled 32-bit tree kernels (QG_OPT_BATCHED_TREE): `batch` members of one
// descriptor in ONE launch of batch x tiles workgroups.  A kernel's text (qg_tree_fast.hip, qg_tree_cplx.hip) is compiled twice;
// the four macros below are all that differs.  QG_TREE_BD unset: the kernel as it always was — its parameter is `g`, nothing stands
// in front of its body and its block number comes from blockIdx.x alone.  QG_TREE_BD set (qg_tree_fast_bd.hip, qg_tree_cplx_bd.hip, which
// include those files):
// the kernel <name>_bd takes the arguments with a QTreeBdWalk behind them, and in front of the body qg_tree_bd_member moves A, B and C
// to the workgroup's member (g: a QTreeBdMember) and leaves the member-local block number, which the unchanged body walks as it walks one GEMM.
#pragma once
#include <stdint.h>

#include "qg_tile_walk.h"

// the walk over the members: byte steps of packed A, B, C from member to member (QBatchGeom::mstride), the tiles of ONE member and the
// launch's workgroups, batch * tiles <= 2^31 - 1 (qg_batched_geometry)
struct QTreeBdWalk {
    int64_t sa, sb, sc;
    uint32_t tiles, nwg;
};

#if defined(__HIPCC__)
// What the body's last lines need to store a tile — C of the workgroup's member and the container size, g.C and g.cbytes — waits in LDS
// while the k-loop runs.  Held in scalar registers (the moved pointer, or the member and the pointer to the kernel's arguments), these are
// values alive across a loop whose scalar registers are all taken in the larger forms, and the twin would spill where its plain kernel
// does not; this way a twin keeps fewer values across the loop than its plain kernel, which keeps the pointer to its arguments.
template <class T>
struct QTreeBdLds {
    const int64_t* at;   // (LDS)
    __device__ __forceinline__ operator T() const { return (T)*at; }
};
// the member's arguments: the launch's, with A and B moved to the member, and C and cbytes (hiding those of Args) as above
template <class Args>
struct QTreeBdMember : Args {
    QTreeBdLds<char*> C;
    QTreeBdLds<int32_t> cbytes;
};
// Workgroup w = qg_xcd_block(blockIdx.x, nwg) belongs to member w / tiles and works on its tile w % tiles: a member's tiles are
// consecutive in the walk and fall into one XCD residue class's run (or two neighbouring ones), as qg_bd_tile_of's do.  All of it is
// wave-uniform scalar arithmetic.  Every lane writes the two LDS words (one value each for the workgroup), which are read behind the
// k-loop.
template <class ArgsBd, class Args>
__device__ __forceinline__ int64_t qg_tree_bd_member(const ArgsBd& gb, QTreeBdMember<Args>& g, int64_t* lds)
{
    const uint32_t w = qg_xcd_block<uint32_t>(blockIdx.x, gb.bd.nwg);
    const uint32_t member = w / gb.bd.tiles;
    static_cast<Args&>(g) = gb;
    g.A = (decltype(g.A))((const char*)gb.A + (int64_t)member * gb.bd.sa);
    g.B = (decltype(g.B))((const char*)gb.B + (int64_t)member * gb.bd.sb);
    lds[0] = (int64_t)(gb.C + (int64_t)member * gb.bd.sc);
    lds[1] = gb.cbytes;
    g.C = {lds};
    g.cbytes = {lds + 1};
    return (int64_t)(w - member * gb.bd.tiles);
}
// ... and its launch: the walk's workgroups
template <class ArgsBd>
inline hipError_t qg_tree_bd_launch(void (*k)(ArgsBd), hipStream_t st, const ArgsBd& g)
{
    hipLaunchKernelGGL(k, dim3(g.bd.nwg), dim3(256), 0, st, g);
    return hipGetLastError();
}
#endif

#ifdef QG_TREE_BD
#define QG_TREE_KERNEL(name) name##_bd
#define QG_TREE_PARAM(Args) Args##Bd gb
#define QG_TREE_MEMBER(Args)             \
    __shared__ int64_t bd_lds_[2];       \
    QTreeBdMember<Args> g;               \
    const int64_t bd_block_ = qg_tree_bd_member(gb, g, bd_lds_)
#define QG_TREE_BLOCK(tiles) bd_block_
#else
#define QG_TREE_KERNEL(name) name
#define QG_TREE_PARAM(Args) Args g
#define QG_TREE_MEMBER(Args)
#define QG_TREE_BLOCK(tiles) qg_xcd_block<int64_t>(blockIdx.x, tiles)
#endif
