// qg_kernels.h — launch interface between the C-ABI layer (qg_api.hip) and the gfx950 kernels; the layouts it launches on: qg_geom.h.
#pragma once
#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>
#include <stdlib.h>

#include <atomic>

#include "qg_eltwise_args.h"
#include "qg_geom.h"
#include "qg_grp.h"
#include "qg_plan.h"
#include "qg_ring.h"

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
// the row sums of centred operands, which sit behind the planes of all members.  A two-part operand (g.parts == 2: the stacked form of
// a complex / mixed batch) brings both parts of a member, [part][row tile] ..., so `stack` then has parts * batch times the rows.
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
// mixed linear class (one real and one complex operand): the two raw dot-product blocks of D (tiled int64: the real operand against
// the stacked parts of the complex one) converted into packed complex C [2][M][N]; P_im sits im_r rows / im_c columns behind P_re
struct QRcConvert {
    const int64_t* D;   // [Mp/tm][Np/tn][tn][tm]
    char* C;
    int64_t M, N, Np, im_r, im_c;
    int32_t tm, tn, cbytes;
    QStep to_c[2];
};
hipError_t qg_launch_rc_convert(const QRcConvert& g, hipStream_t st);
// stacked batched plans (QG_OPT_BATCHED_STACKED; qg_combine_bd.hip): the block-diagonal launch's workspace -> the members' packed
// complex Cs.  W: bd_tm x bd_tn tiles of 64 x 64 int64 per member (tile-major, column-major inside a tile); tm x tn: the tiles of ONE
// part; mode: QStackMode, which fixes bd_tm, bd_tn and where the imaginary product of a mixed member sits (im_r / im_c tiles behind
// the real one); C: [2][M][N] per member in cbytes containers, cstride bytes from member to member
struct QStackCombine {
    const int64_t* W;
    char* C;
    int64_t M, N, cstride;
    int32_t tm, tn, bd_tm, bd_tn, im_r, im_c;
    int32_t mode, cbytes;
    int32_t sh[4];
    QStep to_c[2];
};
hipError_t qg_launch_stack_combine_bd(const QStackCombine& g, int64_t batch, hipStream_t st);

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

// the batched twins of the two (QG_OPT_BATCHED_TREE; qg_tree_fast_bd.hip, qg_tree_cplx_bd.hip): `batch` members of one descriptor in ONE
// launch of batch x tiles workgroups, member b's packed A, B, C at stride[0..2] * b bytes behind member 0's; the checks of the plain
// launchers, and an unknown form, more than 12 levels or more than 2^31 - 1 workgroups is hipErrorInvalidValue
hipError_t qg_launch_tree_fast_bd(const QTreeTable* dev_table, int n_levels, int split_s, int mul24, QTreeForm form, const void* A, const void* B,
                                  void* C, int64_t M, int64_t N, int64_t K, int cbytes, int64_t batch, const int64_t stride[3], hipStream_t st);
hipError_t qg_launch_tree_cplx_fast_bd(const QTreeTable* dev_table, int n_levels, QCplxForm form, int tf, const void* A, const void* B, void* C,
                                       int64_t M, int64_t N, int64_t K, int cbytes, int64_t batch, const int64_t stride[3], hipStream_t st);

// exact tree evaluation, real descriptors with 5..16 levels and 64-bit values (A, B packed as int32 or int64, K = 2^n_levels)
hipError_t qg_launch_tree64(const QTreeTable* dev_table, int n_levels, const void* A, const void* B, void* C, int64_t M, int64_t N,
                            int64_t K, int abytes, int bbytes, int cbytes, hipStream_t st);

// exact tree evaluation of ONE output column (batched Qreduce / GEMV): A [M][K] int32, B [K] int32
hipError_t qg_launch_gemv(const QTreeTable* dev_table, int n_levels, int b_is_bit, QGemvForm form, const void* A, const void* B, void* C,
                          int64_t M, int64_t K, int cbytes, hipStream_t st, int wide = 0);   // wide: 64-bit tree values (4-byte elements)

// exact tree evaluation, complex descriptors with K = 2^p >= 32 and 32-bit intermediates
hipError_t qg_launch_tree_cplx_fast(const QTreeTable* dev_table, int n_levels, QCplxForm form, int tf, const void* A, const void* B, void* C,
                                    int64_t M, int64_t N, int64_t K, int cbytes, hipStream_t st);
// one real and one complex operand (qg_tree_rc.hip): forms QCF_RUNTIME and QCF_COMPACT; a_complex: A is the complex operand
// ([2][M][K], B [N][K]), else B ([2][N][K], A [M][K]); C [2][M][N]
hipError_t qg_launch_tree_rc(const QTreeTable* dev_table, int n_levels, QCplxForm form, int a_complex, const void* A, const void* B, void* C, int64_t M,
                             int64_t N, int64_t K, int cbytes, hipStream_t st);

// linear class on int8 MFMA with LA x LB limbs (QMfmaCfg, qg_mfma_pick: qg_geom.h)
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
// g itself, as a type-dependent expression (I: any template parameter of the caller).  qg_mfma_body.h is one text for kernels with
// different argument structs; through this it names a field that only some of them have inside an `if constexpr` branch, which the
// other kernels discard without looking the field up
template <int I, class G>
QG_HD const G& qg_dependent(const G& g) { return g; }
// An element-wise chain on a batched plan (qgemul_plan_create_batched_epx) in its block-diagonal forms (QBdEp: qg_eltwise_args.h).  The
// kernels carry it in argument structs of their own: QMfmaArgs, QEpArgs and QEltwiseArgs are what they were, so no other kernel's code moves.
struct QMfmaEpBdArgs : QMfmaArgs {
    QBdEp bd;
};
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
// n_tiles workgroups, the ten geometries of qg_launch_mfma_bd (a 3 x 3 launch is the pair <3,3> + <2,2 on three-plane storage>,
// both reading the same records); anything else is hipErrorInvalidValue
hipError_t qg_launch_mfma_grp(int LA, int LB, const QMfmaGrpArgs& a, int64_t n_tiles, hipStream_t st);
// An element-wise chain on a grouped plan (qgemul_plan_create_grouped_epx).  C, D and every tensor operand are the members' packed
// tensors back to back, one index space over the launch, so the chain runs at the launch-wide element index; what differs from member
// to member is a scalar stage's value: scal[k] != nullptr: stage k takes the raw value scal[k][member] (a table of the plan, one entry
// per member of the caller's list; a wave-uniform load), nullptr: QEpArgs::scalar[k] for all (QGrpEp: qg_eltwise_args.h).  The new kernels
// carry this in argument structs of their own: QMfmaArgs, QMfmaGrpArgs, QMfmaEpBdArgs, QEpArgs and QEltwiseArgs are what they were.
struct QMfmaEpGrpArgs : QMfmaArgs {
    const QGrpTile* tiles;
    QGrpEp ge;
};
// the grouped launch with the chain in the kernel's epilogue (qg_mfma_ep_grp.hip: k_mfma_ep_grp, the body of k_mfma with GRP and EP
// together): the geometries of qg_launch_mfma_grp, chains the planner has bounded by 32-bit arithmetic
hipError_t qg_launch_mfma_ep_grp(int LA, int LB, const QMfmaEpGrpArgs& a, int64_t n_tiles, hipStream_t st);
// one member of a stack the caller has cleared (trailer, row sums): qg_launch_pack without the clearing, as qg_launch_pack_stack
// packs its members (p.trailer and p.rowsum_off relative to dst, p.offs == 2 for centred operands)
hipError_t qg_launch_pack_member(const QOperandGeom& g, const QPackedGeom& p, const void* src, void* dst, int check_range, int* range_flag,
                                 hipStream_t st, int generic = 0);
// single limb, 256x256 tiles, 128-byte k-tiles, two wave groups alternating on the matrix cores (qg_mfma_pp.hip; variant 9)
hipError_t qg_launch_mfma_pp(const QMfmaArgs& a, hipStream_t st);
// 3 x 3 and 2 x 2 limbs, 128x128 tiles, the two-group scheme with one A limb plane per phase (qg_mfma_ppl.hip; variant 10)
bool qg_mfma_ppl_applies(int LA, int LB, const QMfmaArgs& a);
hipError_t qg_launch_mfma_ppl(int limbs, const QMfmaArgs& a, hipStream_t st);   // limbs: 3 (3 x 3, plane masks) or 2 (2 x 2 on two-plane storage)
// three unsigned base-64 digits per operand, six products, 96x128 tiles, the two-group scheme (qg_mfma_k6.hip; variant 11).  Its
// packed operands (QPackedGeom::digit6 with 3 planes, 96-row tiles of A) belong to this kernel alone; packed C is the 128 x 128-tiled
// layout of the other limb plans (QG_K6_*: qg_geom.h)
bool qg_mfma_k6_applies(const QMfmaArgs& a);
hipError_t qg_launch_mfma_k6(const QMfmaArgs& a, hipStream_t st);

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

// element-wise epilogue as its own pass (kernels that do not fuse it) and the operand packer; see qg_eltwise.h
hipError_t qg_launch_eltwise(const QEltwiseArgs& g, hipStream_t st);
// ... over the stack of a batched plan / the launch of a grouped plan (qg_eltwise_args.h); a stack that is no whole number of members
// of whole workgroups, a launch that is no whole number of tiles or has no tile -> member table: hipErrorInvalidValue
hipError_t qg_launch_eltwise_bd(const QEltwiseBdArgs& a, hipStream_t st);
hipError_t qg_launch_eltwise_grp(const QEltwiseGrpArgs& a, hipStream_t st);
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
