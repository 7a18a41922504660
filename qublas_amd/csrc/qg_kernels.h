// qg_kernels.h — launch interface between the C-ABI layer (qg_api.hip) and the gfx950 kernels.
#pragma once
#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>
#include <stdlib.h>

#include <atomic>

#include "qg_eltwise_args.h"
#include "qg_grp.h"
#include "qg_plan.h"
#include "qg_ring.h"

// geometry of one operand in host (reference) layout as seen by pack / fill / unpack kernels
struct QOperandGeom {
    int64_t rows, K;        // logical rows (M for A, N for B) and reduction length
    int64_t rs, ks;         // host element index of (r,k) = r*rs + k*ks   (column-major tensors)
    int32_t elem_bytes;     // host element size (complex: whole struct)
    int32_t off[2], sb[2];  // byte offset / byte width (4|8) of each part inside the element
    int32_t parts;          // 1 real, 2 complex
    int32_t W[2], S[2];     // format of each part (range check, synthetic fill)
    int32_t F[2], Q[2], O[2]; // quantise-on-load: fracBits, QuMode, OfMode of each part
    int64_t k0;             // this packed operand holds the reduction indices [k0, k0 + K) of the host tensor (a k-chunk of a
                            // composite linear plan, qg_api.hip; 0 otherwise)
};

// packed (device-private) layouts
//   tree  : [part][rows_p][K_p] containers of cbytes (4|8), K contiguous
//   limbs : int8 balanced base-256 digits, PRE-TILED and PRE-SWIZZLED for the MFMA kernel:
//           [row tile][k tile][limb][tr rows][bk bytes], where the 16-byte chunk c of row r sits at
//           slot c ^ ((r / (256/bk)) % (bk/16)).  One (row tile, k tile) block is exactly the LDS
//           image of that operand for one pipeline stage, so the kernel streams it with lane-linear
//           LDS-DMA (1 KiB per wave instruction, fully sequential in HBM; no row pitch, hence no
//           power-of-two-stride channel camping).
struct QPackedGeom {
    int64_t rows_p, K_p;    // padded extents (rows_p per part: complex limb operands stack their parts along rows)
    int32_t cbytes;         // container bytes (tree layout), 1 for limb layout
    int32_t limbs;          // 0 = tree layout, >0 = limb layout
    int32_t tr, bk;         // limb layout: rows per tile, k bytes per tile
    // limb layout with limbs > 1: the planes are followed by a 256-byte trailer whose first word is the OR over all
    // elements of (1 << l) for every limb l that is non-zero somewhere ("plane mask", written by the pack kernels).  The
    // MFMA kernel skips the products of planes that are zero everywhere: data that stays inside [-32640, 32639] never
    // touches the third int8 limb of a 17-bit format, and 4 instead of 9 products are exact for it.
    int64_t trailer;        // byte offset of the trailer (0: none)
    // Karatsuba layout (2 x 2 digits, operands of at most 12 value+sign bits): the two planes hold the UNSIGNED base-64 digits
    // of x + bias (bias = 2^W for a signed format, so the biased value is non-negative; padding holds 0), and int64
    // row_sum[rows_p] = sum_k (x + bias) follows the trailer — the kernel's epilogue takes the bias back out with it.
    int32_t digit6;
    // limb layout: the planes hold digits limb0 .. limb0 + limbs - 1 of the balanced base-256 expansion (a limb GROUP of an
    // operand of more than 3 limbs, composite linear plans; 0 otherwise)
    int32_t limb0;
    // CENTRED operands (offs != 0; qg_plan.h: qg_limbs_centred): the planes hold the balanced digits of x + bias (bias = -centre;
    // padding holds 0) and int64 row_sum[rows_p] = sum_k (x + bias) sits at rowsum_off — sum a b = sum a'b' - biasB rsA[i]
    // - biasA rsB[j] + K biasA biasB, taken back out by the MFMA kernels' epilogues / the composite plan's combine pass.
    // offs 1: this packed operand owns its row sums (the pack zeroes and fills them); 2: a sub-operand of a composite plan adding
    // its k-chunk to the operand's one array (zeroed by the caller; only the groups with limb0 == 0 add); 3: ... a group that does not
    int32_t offs, pad_;
    int64_t bias, rowsum_off;
};
enum { QG_TRAILER_BYTES = 256, QG_MASK_WORDS = 64 };

// The plane mask lives in ALL 64 words of the trailer: a pack kernel's waves OR their findings into word (wave id % 64) — on
// one word the 16 384 atomics of a 4096^2 operand serialise (0.2 ms against 0.03 ms for the pack itself, found when bench.py
// began to pack non-zero data) — and a consumer ORs the 64 words: one load per lane and a wave reduction.
#if defined(__HIPCC__)
__device__ __forceinline__ unsigned qg_plane_mask(const uint32_t* m)
{
    if (!m) return 7u;
    unsigned v = m[threadIdx.x & 63];
#pragma unroll
    for (int o = 32; o; o >>= 1) v |= __shfl_xor(v, o);
    return (unsigned)__builtin_amdgcn_readfirstlane(v);
}
#endif

struct QCGeom {
    int64_t M, N, Mp, Np;   // logical / padded extents of packed C
    int32_t tm, tn;         // 0: row-major [part][Mp][Np]; else tiled [part][Mp/tm][Np/tn][tn cols][tm rows]
    int32_t cbytes;         // 1|2|4|8 container
    int32_t parts;
    int64_t ldc;            // host leading dimension (elements)
    int32_t elem_bytes, off[2], sb[2];
};

// element index of (part, m, n) in packed C
__host__ __device__ inline int64_t qg_c_index(const QCGeom& c, int part, int64_t m, int64_t n)
{
    if (c.tm == 0) return ((int64_t)part * c.Mp + m) * c.Np + n;
    return ((((int64_t)part * (c.Mp / c.tm) + m / c.tm) * (c.Np / c.tn) + n / c.tn) * c.tn + n % c.tn) * c.tm + m % c.tm;
}

hipError_t qg_launch_pack(const QOperandGeom& g, const QPackedGeom& p, const void* src, void* dst, int check_range,
                          int* range_flag, hipStream_t st, int generic = 0);   // generic: the any-format kernel even where a fast path exists
// the same with a column-major tensor of DOUBLES as source (complex: {re, im} pairs), quantised on load with each
// part's own QuMode / OfMode exactly as Qu_s(double) does (QuBLAS.h:2387-2393)
hipError_t qg_launch_pack_f64(const QOperandGeom& g, const QPackedGeom& p, const void* src, void* dst, hipStream_t st, int generic = 0);
hipError_t qg_launch_fill(const QOperandGeom& g, const QPackedGeom& p, uint64_t seed, int dist, void* dst, hipStream_t st);
hipError_t qg_launch_unpack_c(const QCGeom& c, const void* packed, void* dst, hipStream_t st, int generic = 0);
// batched plans, block-diagonal form: `batch` members of geometry g / member (ONE member's packed geometry; limb layout) at
// src + b * stride_bytes are packed into the row tiles [b * member.rows_p / tr, ...) of the stack `stack` (member with batch times
// the rows).  What belongs to the STACK is set up once, not per member: the plane-mask trailer (the OR over every member) and
// the row sums of centred operands, which sit behind the planes of all members.
hipError_t qg_launch_pack_stack(const QOperandGeom& g, const QPackedGeom& member, const QPackedGeom& stack, int64_t batch, const void* src,
                                int64_t stride_bytes, void* dst, int check_range, int* range_flag, hipStream_t st, int generic = 0);

// complex linear class: combine the four raw dot-product blocks of D (tiled int64) into packed complex C [2][M][N]
struct QCplxCombine {
    const int64_t* D;   // [Mp/tm][Np/tn][tn][tm], Mp = 2*Mh, Np = 2*Nh
    char* C;
    int64_t M, N, Mh, Nh, Np;
    int32_t tm, tn, cbytes;
    int32_t sh[4];
    QStep to_c[2];
};
hipError_t qg_launch_cplx_combine(const QCplxCombine& g, hipStream_t st);

// composite linear plans (operands of more than 3 int8 limbs, or K beyond the int32 accumulators' exact range): the limb-group /
// k-chunk sub-GEMMs store RAW dot products (int32 for single-limb pairs, int64 otherwise) in slabs of one common packed-C
// layout; this pass forms  s = acc_in + sum_j (slab_j << sh[j])  per element, exactly, and either keeps it for the next
// k-chunk (acc_out) or rounds + overflow-handles it ONCE into C's format (out).  wide: 128-bit sums (two-word accumulator
// elements, C containers of up to 16 bytes).
enum { QG_MAX_SLABS = 9 };
struct QLinCombine {
    const void* slab[QG_MAX_SLABS];
    int32_t sh[QG_MAX_SLABS];
    int32_t n_slabs, slab_bytes;   // 4 | 8
    int64_t n;                     // elements (the padded packed-C index space)
    const void* acc_in;            // nullptr: start from 0
    void* acc_out;                 // nullptr: this is the last chunk
    void* out;                     // packed C (cbytes containers), written when acc_out == nullptr
    int32_t cbytes, wide;
    QStep to_c;
    // centred operands (QPackedGeom::offs): the correction of the last chunk, per element of the tiled packed-C index space
    // (element i: tile i / (tm tn), column (i / tm) % tn, row i % tm of that tile; tiles_n tiles per tile row)
    const int64_t* rsA;
    const int64_t* rsB;
    int64_t biasA, biasB, corr;   // corr: the reduction length K (K biasA biasB is formed in the accumulator's width)
    int32_t tm, tn;
    int64_t tiles_n;
};
hipError_t qg_launch_lin_combine(const QLinCombine& g, hipStream_t st);

// exact tree evaluation, any descriptor (real / complex, any K), 64-bit arithmetic
hipError_t qg_launch_tree_generic(const QTreeTable* dev_table, int parts, const void* A, const void* B, void* C, int64_t M,
                                  int64_t N, int64_t K, const QPackedGeom& pa, const QPackedGeom& pb, const QCGeom& pc,
                                  hipStream_t st, int wide = 0);   // wide: 128-bit values (C containers of up to 16 bytes)

// exact tree evaluation, real descriptors with K = 2^p >= 32 and 32-bit intermediates (A, B packed as int32); an unknown form is
// hipErrorInvalidValue
hipError_t qg_launch_tree_fast(const QTreeTable* dev_table, int n_levels, int split_s, int mul24, QTreeForm form, const void* A, const void* B,
                               void* C, int64_t M, int64_t N, int64_t K, int cbytes, hipStream_t st);

// exact tree evaluation, real descriptors with 5..16 levels and 64-bit values (A, B packed as int32 or int64, K = 2^n_levels)
hipError_t qg_launch_tree64(const QTreeTable* dev_table, int n_levels, const void* A, const void* B, void* C, int64_t M, int64_t N,
                            int64_t K, int abytes, int bbytes, int cbytes, hipStream_t st);

// exact tree evaluation of ONE output column (batched Qreduce / GEMV): A [M][K] int32, B [K] int32
hipError_t qg_launch_gemv(const QTreeTable* dev_table, int n_levels, int b_is_bit, QGemvForm form, const void* A, const void* B, void* C,
                          int64_t M, int64_t K, int cbytes, hipStream_t st, int wide = 0);   // wide: 64-bit tree values (4-byte elements)

// exact tree evaluation, complex descriptors with K = 2^p >= 32 and 32-bit intermediates
hipError_t qg_launch_tree_cplx_fast(const QTreeTable* dev_table, int n_levels, QCplxForm form, int tf, const void* A, const void* B, void* C,
                                    int64_t M, int64_t N, int64_t K, int cbytes, hipStream_t st);

// linear class on int8 MFMA with LA x LB limbs
struct QMfmaCfg {
    int variant;    // QMfmaVariant; 0 = no kernel for this limb combination
    int TM, TN, BK; // output tile and k-tile (bytes) the packed operands are padded to
};
QMfmaCfg qg_mfma_pick(int LA, int LB, int64_t M, int64_t N, uint32_t opt_flags = 0);
struct QMfmaArgs {
    const int8_t* A;  // [LA][Mp][Kp]
    const int8_t* B;  // [LB][Np][Kp]
    void* C;          // [Mp][Np] containers
    int64_t Mp, Np, Kp;
    int32_t cbytes;
    int32_t variant;
    QStep to_c;
    // Karatsuba variant (kara != 0): sum a*b = sum a'b' - biasB * rsA[i] - biasA * rsB[j] + corr, with a' = a + biasA etc.
    const int64_t* rsA;
    const int64_t* rsB;
    int64_t biasA, biasB, corr;
    // bd_tm, bd_tn (below): the block-diagonal form (batched Qgemul, qg_launch_mfma_bd; 0: one GEMM).  A and B are the members'
    // packed operands stacked by row tiles (Mp, Np: the stack's rows), bd_tm x bd_tn the tiles of ONE member; workgroup w of
    // batch * bd_tm * bd_tn works on qg_bd_tile_of(w) and stores into the members' packed Cs back to back.  (The two fields sit
    // where the struct had padding: its size and every other field's offset are what they were, so no kernel's code moves.)
    int32_t kara, bd_tm;
    int64_t Mc;             // k_mfma_k6: padded rows of packed C (128-row tiles), which differ from Mp (A on 96-row tiles)
    const uint32_t* maskA;  // plane masks of the packed operands (QPackedGeom::trailer); nullptr: all planes
    const uint32_t* maskB;
    int32_t has_ep, bd_tn;  // fused element-wise epilogue: C below is then packed D (ep.dbytes containers)
    uint32_t* dbg;          // diagnostic build: in-kernel clock stamps (qg_mfma_pp.hip); nullptr otherwise
    // c_host != 0 (k_mfma_pp / k_mfma_ppl, 4- and 8-byte containers): C is the REFERENCE layout on the device — element (i, j)
    // at i + j * c_ld, c_M x c_N logical — and the epilogue's runs of 4 rows land there directly: no packed C, no unpack pass.
    // c_vec: every run of 4 rows is 16-byte aligned (base and c_ld permitting): one vector store per run.
    int32_t c_host, c_vec;
    int64_t c_ld, c_M, c_N;
    QEpTable ep;
    QEpArgs epa;
};
// bd_tm / bd_tn took the place of two padding words: the struct's size and every other field's offset are the parent's
static_assert(offsetof(QMfmaArgs, bd_tm) == offsetof(QMfmaArgs, kara) + 4 && offsetof(QMfmaArgs, Mc) == offsetof(QMfmaArgs, kara) + 8 &&
              offsetof(QMfmaArgs, bd_tn) == offsetof(QMfmaArgs, has_ep) + 4 && offsetof(QMfmaArgs, dbg) == offsetof(QMfmaArgs, has_ep) + 8,
              "QMfmaArgs: the block-diagonal fields sit in former padding; no field may move");
hipError_t qg_launch_mfma(int LA, int LB, const QMfmaArgs& a, hipStream_t st);
// An element-wise chain on a batched plan (qgemul_plan_create_batched_epx) in its block-diagonal forms: C, D and every per-member
// tensor operand are the members' packed tensors back to back (one index space over the whole stack); a SHARED operand is ONE
// member's packed tensor, read at the member-local index  i - member * msize.  msize = elements of one member's packed C (a
// whole number of 64 x 64 tiles), shared bit k = stage k's tensor operand is shared.  The new kernels carry this in argument
// structs of their own: QMfmaArgs, QEpArgs and QEltwiseArgs are what they were, so no existing kernel's code moves.
struct QBdEp {
    int64_t msize;
    uint32_t shared, pad_;
};
struct QMfmaEpBdArgs : QMfmaArgs {
    QBdEp bd;
};
// the QBdEp of a kernel's argument struct (kernels whose arguments have none never evaluate the result)
template <class G>
QG_HD auto qg_bd_ep_of(const G& g, int) -> decltype(g.bd) { return g.bd; }
template <class G>
QG_HD QBdEp qg_bd_ep_of(const G&, long) { return QBdEp{0, 0, 0}; }
// the block-diagonal launch with the chain in the kernel's epilogue (qg_mfma_ep_bd.hip: k_mfma_ep_bd, the body of k_mfma with BD and
// EP together): the geometries of qg_launch_mfma_bd, chains the planner has bounded by 32-bit arithmetic
hipError_t qg_launch_mfma_ep_bd(int LA, int LB, const QMfmaEpBdArgs& a, int64_t batch, hipStream_t st);
// `batch` GEMMs of one member shape in ONE launch of k_mfma's block-diagonal form (qg_mfma.hip): the variants qg_mfma_pick_batched
// returns, no element-wise chain, no Karatsuba digits; anything else is hipErrorInvalidValue
hipError_t qg_launch_mfma_bd(int LA, int LB, const QMfmaArgs& a, int64_t batch, hipStream_t st);
// Grouped Qgemul: GEMMs of DIFFERENT shapes in one launch of k_mfma_grp (qg_mfma_grp.hip), the body of k_mfma with GRP.  A, B and C
// are the members' packed operands back to back (every member with its own padded rows and its own K_p), maskA / maskB the launch's
// one plane mask per operand (the OR over every member), rsA / rsB one row-sum array per operand over the stack's rows, and
// tiles[] the host's schedule (qg_grp.h): one record per workgroup.  Mp, Np, Kp, corr, bd_tm and bd_tn are not read.  The kernel has
// an argument struct of its own: QMfmaArgs is what it was.
struct QMfmaGrpArgs : QMfmaArgs {
    const QGrpTile* tiles;
};
// the schedule of a kernel's argument struct (kernels whose arguments have none never evaluate the result)
template <class G>
QG_HD auto qg_grp_tiles_of(const G& g, int) -> decltype(g.tiles) { return g.tiles; }
template <class G>
QG_HD const QGrpTile* qg_grp_tiles_of(const G&, long) { return nullptr; }
// n_tiles workgroups, the ten geometries of qg_launch_mfma_bd (a 3 x 3 launch is the pair <3,3> + <2,2 on three-plane storage>,
// both reading the same records); anything else is hipErrorInvalidValue
hipError_t qg_launch_mfma_grp(int LA, int LB, const QMfmaGrpArgs& a, int64_t n_tiles, hipStream_t st);
// one member of a stack the caller has cleared (trailer, row sums): qg_launch_pack without the clearing, as qg_launch_pack_stack
// packs its members (p.trailer and p.rowsum_off relative to dst, p.offs == 2 for centred operands)
hipError_t qg_launch_pack_member(const QOperandGeom& g, const QPackedGeom& p, const void* src, void* dst, int check_range, int* range_flag,
                                 hipStream_t st, int generic = 0);
// tile geometry of a batched plan; variant 0: no block-diagonal form for this member (it runs member by member on `plain`, the
// member's own qg_mfma_pick)
QMfmaCfg qg_mfma_pick_batched(int LA, int LB, int64_t batch, const QMfmaCfg& plain);
// single limb, 256x256 tiles, 128-byte k-tiles, two wave groups alternating on the matrix cores (qg_mfma_pp.hip; variant 9)
hipError_t qg_launch_mfma_pp(const QMfmaArgs& a, hipStream_t st);
// 3 x 3 and 2 x 2 limbs, 128x128 tiles, the two-group scheme with one A limb plane per phase (qg_mfma_ppl.hip; variant 10)
bool qg_mfma_ppl_applies(int LA, int LB, const QMfmaArgs& a);
hipError_t qg_launch_mfma_ppl(int limbs, const QMfmaArgs& a, hipStream_t st);   // limbs: 3 (3 x 3, plane masks) or 2 (2 x 2 on two-plane storage)
// three unsigned base-64 digits per operand, six products, 96x128 tiles, the two-group scheme (qg_mfma_k6.hip; variant 11).  Its
// packed operands (QPackedGeom::digit6 with 3 planes, 96-row tiles of A) belong to this kernel alone; packed C is the 128 x 128-tiled
// layout of the other limb plans
enum { QG_K6_VARIANT = 11, QG_K6_TM = 96, QG_K6_TN = 128, QG_K6_BK = 64 };
bool qg_mfma_k6_applies(const QMfmaArgs& a);
hipError_t qg_launch_mfma_k6(const QMfmaArgs& a, hipStream_t st);

// QMfmaCfg::variant / QMfmaArgs::variant: which kernel qg_mfma_pick() and plan_geometry (qg_api.hip) chose and qg_launch_mfma
// starts.  Output tile x k-tile bytes; "limb": any LA x LB other than 1 x 1.
enum QMfmaVariant {
    QG_MFMA_NONE = 0,
    QG_MFMA_128 = 1,         // single limb, k_mfma (32x32x32), 128x128 x 64: more than one workgroup per CU, too few for 256x256
    QG_MFMA_256 = 2,         // single limb, k_mfma16 (16x16x64), 256x256 x 64, lock-step (QG_OPT_LOCKSTEP_TILES, fused chains)
    QG_MFMA_LIMB_128 = 3,    // limb, k_mfma16's row-step form (k_mfma where that has no instantiation), 128x128 x 64; Karatsuba 2 x 2
    QG_MFMA_64 = 5,          // single limb, k_mfma, 64x64 x 64 (diagnostic build: QG_BK64)
    QG_MFMA_LIMB_64 = 6,     // limb, k_mfma, 64x64 x 64 (small problems; a 5-stage ring at one workgroup per CU)
    QG_MFMA_64_BK128 = 7,    // single limb, k_mfma, 64x64 x 128 (small problems; two k groups per workgroup for long k)
    QG_MFMA_128_BK128 = 8,   // single limb, k_mfma, 128x128 x 128 (at most one workgroup per CU)
    QG_MFMA_PP = 9,          // single limb, k_mfma_pp, 256x256 x 128, two wave groups, persistent (qg_mfma_pp.hip)
    QG_MFMA_PPL = 10,        // 3 x 3 / 2 x 2 limbs, k_mfma_ppl / k_mfma_ppl22, 128x128 x 64, two wave groups, persistent
                             // (qg_mfma_ppl.hip); fused chains and narrow C run QG_MFMA_LIMB_128 on the same packed layout
    QG_MFMA_K6 = QG_K6_VARIANT,       // 11: three base-64 digits, k_mfma_k6, 96x128 x 64 (qg_mfma_k6.hip)
    QG_MFMA_RING = QG_RING_VARIANT,   // 12: ring plans, k_mfma_ring, 128x128 x 64 (qg_ring.h; launched by qg_launch_mfma_ring)
};

// hipFuncAttributeMaxDynamicSharedMemorySize is set once per DEVICE (one process may drive several: qgemul_run_sharded);
// `done` holds one bit per device ordinal of the calling thread's current device
inline hipError_t qg_lds_attr(const void* fn, int bytes, std::atomic<uint64_t>& done)
{
    int dev = 0;
    hipError_t e = hipGetDevice(&dev);
    if (e != hipSuccess) return e;
    if (dev >= 0 && dev < 64 && ((done.load(std::memory_order_acquire) >> dev) & 1)) return hipSuccess;
    e = hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize, bytes);
    if (e == hipSuccess && dev >= 0 && dev < 64) done.fetch_or(1ull << dev, std::memory_order_release);
    return e;
}

// ... and the launch that goes with it, for a kernel with dynamic LDS: one `done` word per kernel instantiation.  lds_max: the
// attribute's value where launches of one kernel differ in their LDS size (0: lds)
template <auto Kernel, class Args>
hipError_t qg_launch_lds(unsigned grid, unsigned block, int lds, hipStream_t st, const Args& a, int lds_max = 0)
{
    static std::atomic<uint64_t> attr_done{0};
    if (hipError_t e = qg_lds_attr((const void*)Kernel, lds_max ? lds_max : lds, attr_done); e != hipSuccess) return e;
    hipLaunchKernelGGL(Kernel, dim3(grid), dim3(block), lds, st, a);
    return hipGetLastError();
}

// grid of a persistent kernel (k_mfma_pp, k_mfma_ppl, k_mfma_k6): one workgroup per CU, a multiple of 8 so that every XCD residue
// class has the same number (qg_tile_walk.h); fewer tiles than CUs: the tile count rounded up to 8, surplus workgroups find
// their list empty
inline hipError_t qg_persistent_grid(int64_t tiles, unsigned* grid)
{
    int dev = 0, cus = 0;
    if (hipError_t e = hipGetDevice(&dev); e != hipSuccess) return e;
    if (hipError_t e = hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev); e != hipSuccess) return e;
    int64_t g = cus / 8 * 8;
    if (g < 8) g = 8;
    if (g > tiles) g = (tiles + 7) / 8 * 8;
    *grid = (unsigned)g;
    return hipSuccess;
}

// the conversion into C's format that the epilogues specialise at compile time (FAST): truncation (TRN::TCPL, right shift
// d >= 0) + SAT::TCPL, a shift and a clamp per value
inline bool qg_step_is_shift_clamp(const QStep& q) { return !q.identity && q.O == QG_SAT_TCPL && q.Q == QG_TRN_TCPL && q.d >= 0; }

// A/B and ablation switches read from the environment exist only in the diagnostic build (libqugemm_diag.so, -DQG_DIAG,
// used by tools/); the product library ignores the environment altogether.
#ifdef QG_DIAG
#define QG_DIAG_ENV(name) (getenv(name) != nullptr)
#else
#define QG_DIAG_ENV(name) false
#endif

// element-wise epilogue as its own pass (kernels that do not fuse it) and the operand packer; see qg_eltwise.h
hipError_t qg_launch_eltwise(const QEltwiseArgs& g, hipStream_t st);
hipError_t qg_launch_pack_e(const QCGeom& c, int part, const void* src, int64_t ld, int stride, int off, int src_bytes, void* dst, int ebytes,
                            hipStream_t st);

// BitStream export of packed C (qg_pack.hip): n = M*N elements of `width` characters each
struct QBitsArgs {
    QCGeom c;
    const char* packed;
    char* out;
    int32_t width, tensor_chunk, elem_chunk, packed_bits;
};
hipError_t qg_launch_bitstream(const QBitsArgs& a, hipStream_t st);
// ... of a packed COMPLEX C: an element is the string "(re-bits, im-bits)" after its chunk reversal; tab[j] says what output
// character j of an element is: 0..63 bit k of the real part, 64..127 bit (k - 64) of the imaginary part, 128.. a literal
enum { QG_BITS_LIT_OPEN = 128, QG_BITS_LIT_COMMA = 129, QG_BITS_LIT_SPACE = 130, QG_BITS_LIT_CLOSE = 131 };
struct QBitsCplxArgs {
    QCGeom c;
    const char* packed;
    char* out;
    int32_t width, nbits, tensor_chunk, packed_bits;   // characters per element; binary characters per element (wr + wi)
    uint8_t tab[136];
};
hipError_t qg_launch_bitstream_cplx(const QBitsCplxArgs& a, hipStream_t st);
