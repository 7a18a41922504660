// qg_tile_walk.h — the integer arithmetic that the pack kernels, the MFMA kernels and the tiled tree kernels must agree on: the
// swizzle of the packed operands' LDS image and the XCD-aware walk over the output tiles.  Plain functions of integers, no HIP
// header, so that the host compiler can build them too: tests/test_tile_walk.py pins every one against a restatement.
#pragma once

#ifndef QG_HD   // (as qg_ops.h defines it)
#if defined(__HIPCC__)
#define QG_HD __host__ __device__ __forceinline__
#else
#define QG_HD inline
#endif
#endif

// LDS image of one k-tile of a packed limb operand (QPackedGeom, qg_kernels.h): rows of BK bytes; the 16-byte chunk c of row r
// sits at slot c ^ qg_swz<BK>(r).  The pack kernels write it, every MFMA kernel reads through it.
//   q = (r / rows per 256-byte bank row) % chunks per row  puts the 16 lanes of every ds_read_b128 group of a 32x32x32 fragment
//   (rows l & 31, one chunk column) on 16 distinct 16-byte bank slots.  For 64-byte rows q -> {0,2,3,1}[q] keeps those reads
//   conflict free (any bijection does) AND the 16x16x64 fragment reads (rows l & 15, chunk l >> 4).
// 64-byte rows: {0,2,3,1}[(r / 4) % 4]; 128-byte rows: (r / 2) % 8.  A row that is (a multiple of 16) + (lane & 15) has the
// swizzle of (lane & 15): the kernels that read such rows only keep it as a lane constant.
template <int BK>
QG_HD constexpr int qg_swz(int r)
{
    static_assert(BK == 64 || BK == 128, "k-tiles of 64 or 128 bytes");
    constexpr int CPR = BK / 16;   // chunks per row
    constexpr int RPB = 256 / BK;  // rows per 256-byte bank row
    const int q = (r / RPB) % CPR;
    return BK == 64 ? ((0x78 >> (2 * q)) & 3) : q;
}
// the same for a k-tile size known at run time only (the pack kernels: QPackedGeom::bk)
QG_HD int qg_swz(int bk, int r)
{
    const int cpr = bk / 16, rpb = 256 / bk;
    const int q = (r / rpb) % cpr;
    return bk == 64 ? ((0x78 >> (2 * q)) & 3) : q;
}

// XCD-aware order of the output tiles.  Block ids b and b + 8 share an XCD and its L2 (observed dispatch; speed only), so each
// of the 8 residue classes of the block id gets a contiguous run of the walk: class x owns the tile numbers
// [qg_xcd_run_start(nwg, x), qg_xcd_run_start(nwg, x + 1)), the first nwg % 8 classes one tile more than the others.
template <class I>
QG_HD I qg_xcd_run_start(I nwg, I x)
{
    const I q = nwg / 8, r = nwg % 8;
    return x < r ? x * (q + 1) : r * (q + 1) + (x - r) * q;
}
// lock-step kernels (one workgroup per tile): the tile number of block bid, qg_xcd_run_start(nwg, bid % 8) + bid / 8
template <class I>
QG_HD I qg_xcd_block(I bid, I nwg)
{
    const I q = nwg / 8, r = nwg % 8, x = bid % 8;
    return (x < r ? x * (q + 1) : r * (q + 1) + (x - r) * q) + bid / 8;
}

// The walk: tile number w -> (tile_m, tile_n) in groups of GM tile rows (the last group may be shorter), column by column inside
// a group, so that neighbouring tiles re-use A rows and B columns in L2.  GM: 8 for the MFMA kernels, 16 for the tree kernels.
// MOD only chooses how w's position inside its group is spelled.  The value is the same; hipcc's instruction order for a whole
// kernel is not, and the lock-step and tree kernels (MOD) and the persistent kernels keep the code they were measured with.
template <int GM, bool MOD = false, class I>
QG_HD void qg_tile_of(I w, I tiles_m, I tiles_n, I& tile_m, I& tile_n)
{
    const I grp = w / (GM * tiles_n);
    const I first_m = grp * GM;
    const I gsz = (tiles_m - first_m) < GM ? (tiles_m - first_m) : GM;
    const I rem = MOD ? w % (GM * tiles_n) : w - grp * (GM * tiles_n);
    tile_m = first_m + rem % gsz;
    tile_n = rem / gsz;
}

// Block-diagonal walk (batched Qgemul: `batch` members of tmM x tnN tiles each, operands stacked): tile number w of the batch's
// batch * tmM * tnN tiles -> (member, tile_m, tile_n), the tile indices local to the member.  A member's tiles are consecutive
// tile numbers, walked inside the member as qg_tile_of<8, true> walks one GEMM, so that with qg_xcd_block over the batch's total a
// member's tiles fall into one XCD residue class's run (or two neighbouring ones) and share that L2.
template <class I>
QG_HD void qg_bd_tile_of(I w, I tmM, I tnN, I& member, I& tile_m, I& tile_n)
{
    const I per = tmM * tnN;
    member = w / per;
    qg_tile_of<8, true>(w % per, tmM, tnN, tile_m, tile_n);
}

// Stacked batched plans (QG_OPT_BATCHED_STACKED): a member's block of the block-diagonal launch holds the products of its stacked
// parts, tm x tn tiles per product.  Source tile k of part `part` of the OUTPUT tile (lm, ln), as (row tile, column tile) inside the
// member's block.  Complex members (cplx; the block is 2 tm x 2 tn): re = P(lm, ln) - P(lm + tm, ln + tn), im = P(lm, ln + tn) +
// P(lm + tm, ln), k = 0, 1 in this order.  Mixed members: one product per part (k = 0), the imaginary one im_r tile rows / im_c tile
// columns behind the real one (real x complex: 0, tn; complex x real: tm, 0).
QG_HD void qg_stack_src_tile(bool cplx, int part, int k, int lm, int ln, int tm, int tn, int im_r, int im_c, int& r, int& c)
{
    if (cplx) {
        r = lm + (k ? tm : 0);
        c = ln + (k != part ? tn : 0);
    } else {
        r = lm + (part ? im_r : 0);
        c = ln + (part ? im_c : 0);
    }
}

// Persistent kernels (grid workgroups, a multiple of 8, each walking a list of tiles): the grid / 8 workgroups of a residue
// class take the tiles of the class's run round-robin, i.e. in every round a class works on grid / 8 consecutive tiles of the
// walk.  Workgroup block.x of grid.x owns the tile numbers first + i * step, i < count (count == 0: nothing to do).  A kernel
// passes blockIdx and gridDim themselves, so that each is read where it is used; the host passes two QDimX.
struct QTileList {
    int first, step, count;
};
struct QDimX {
    unsigned x;
};
template <class B, class G>
QG_HD QTileList qg_tile_list(int nwg, const B& block, const G& grid)
{
    const int q = nwg / 8, r = nwg % 8, x = block.x % 8;
    const int start = qg_xcd_run_start<int>(nwg, x);
    const int cnt = q + (x < r ? 1 : 0), j = block.x / 8, P = grid.x / 8;
    return QTileList{start + j, P, j < cnt ? (cnt - j + P - 1) / P : 0};
}
