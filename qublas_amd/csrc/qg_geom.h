// qg_geom.h — plan geometry: which kernel a descriptor gets and where every byte of its packed operands sits (qg_geom.cpp).  Host
// code without HIP types, like qg_plan.h and qg_run_key.h: a host compiler builds it alone (tests/san/geom_san_driver.cpp), the
// C-ABI layer (qg_api.hip) copies its answers into plans and launches by them, the kernels' launch interface (qg_kernels.h) shares
// its layout structs.
#pragma once
#include <stdint.h>
#include <stdlib.h>

#include "qg_approx.h"
#include "qg_cmul.h"
#include "qg_grp.h"
#include "qg_plan.h"
#include "qg_run_key.h"

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
                            // composite linear plan, qg_geom.cpp; 0 otherwise)
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

struct QCGeom {
    int64_t M, N, Mp, Np;   // logical / padded extents of packed C
    int32_t tm, tn;         // 0: row-major [part][Mp][Np]; else tiled [part][Mp/tm][Np/tn][tn cols][tm rows]
    int32_t cbytes;         // 1|2|4|8 container
    int32_t parts;
    int64_t ldc;            // host leading dimension (elements)
    int32_t elem_bytes, off[2], sb[2];
};

// linear class on int8 MFMA with LA x LB limbs
struct QMfmaCfg {
    int variant;    // QMfmaVariant; 0 = no kernel for this limb combination
    int TM, TN, BK; // output tile and k-tile (bytes) the packed operands are padded to
};
// three unsigned base-64 digits per operand (qg_mfma_k6.hip; variant 11): its tile geometry
enum { QG_K6_VARIANT = 11, QG_K6_TM = 96, QG_K6_TN = 128, QG_K6_BK = 64 };
// QMfmaCfg::variant of a ring plan (qg_ring.h) and the one tile geometry of its kernel (packed C: the 128 x 128 tiles of every limb plan)
enum { QG_RING_VARIANT = 12, QG_RING_TM = 128, QG_RING_TN = 128, QG_RING_BK = 64 };
// digits of a ring of n bits, and the limb products A_i B_j (i < LA, j < LB) of weight i + j below it
inline int qg_ring_digits(int n) { return (n + 7) / 8; }
inline int qg_ring_products(int LA, int LB, int L)
{
    int c = 0;
    for (int i = 0; i < LA; ++i)
        for (int j = 0; j < LB; ++j) c += i + j < L ? 1 : 0;
    return c;
}

// QMfmaCfg::variant / QMfmaArgs::variant: which kernel qg_mfma_pick() and qg_plan_geometry (qg_geom.cpp) chose and qg_launch_mfma
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

// A/B and ablation switches read from the environment exist only in the diagnostic build (libqugemm_diag.so, -DQG_DIAG,
// used by tools/); the product library ignores the environment altogether.
#ifdef QG_DIAG
#define QG_DIAG_ENV(name) (getenv(name) != nullptr)
#else
#define QG_DIAG_ENV(name) false
#endif

// Composite linear plan.  The MFMA kernels take operands of at most 3 int8 limbs and keep exact int32 accumulators only while
// K * min(LA, LB) < 2^17.  Beyond either bound the linear class used to fall to the 64-bit VALU tree kernel (40-300x slower); the
// reference has no such boundary (Reducer, QuBLAS.h:4960-4990; ArbiInt elements up to 64 bits, :347-564).  Now:
//   * an operand of L > 3 limbs is stored as limb GROUPS of 2-3 limbs (x = sum_g x_g * 256^limb0[g], every x_g a balanced
//     base-256 number of its own), each group a complete packed operand of the existing layout;
//   * K is cut into chunks of at most kc reduction indices (a multiple of 256), each chunk a complete packed operand as well;
//   * every (chunk, A group, B group) is ONE launch of an existing MFMA kernel that stores raw dot products (identity
//     epilogue) into a slab, and k_lin_combine (qg_pack.hip) adds the slabs by weight into an exact running sum and, after the
//     last chunk, rounds + overflow-handles it once into C — the linear class's whole epilogue (QuBLAS.h:2398-2411).
// Packed operand = the sub-operands back to back, chunk-major, each 256-byte aligned.
struct QComposite {
    int on;
    int ga, gb;            // limb groups of A, B (1..3)
    int la[3], lb[3];      // limbs per group
    int la0[3], lb0[3];    // first limb of each group
    int var[3][3];         // MFMA variant of the pair (A group, B group); one tile geometry for all pairs
    int nc;                // k-chunks
    int64_t kc;            // reduction indices per chunk (the last chunk: K - (nc - 1) * kc)
    int slab_bytes;        // 4: single-limb pairs (raw int32), 8 otherwise
    int wide;              // 128-bit sums
    int64_t chunk_bytes[2];   // bytes of one FULL chunk of packed A / B (all groups)
};
// what qg_plan_geometry computes for a descriptor, pure host data: the analysis, the kernel and its tile geometry, the packed layouts
struct QPlanGeom {
    QAnalysis an;
    qgemul_info info;
    int LA, LB, variant;
    QMfmaCfg cfg;
    QPackedGeom pa, pb;
    QCGeom pc;            // with an element-wise chain: packed D
    QHostElem ha, hb, hc;
    QEpTable ept;         // the chain (a complex one: of the real parts)
    QEpTable ept_im;      // ... of the imaginary parts
    QCGeom pc_c;          // the kernel's own packed C, which only exists in memory (cwork) for the kernels that do not fuse the chain
    QComposite comp;      // composite linear plan (comp.on): limb groups x k-chunks of sub-GEMMs + an exact combine pass
    int bd;               // the member of a batched plan: k_mfma's block-diagonal form takes it (a batched plan: it launches that form)
    int bd_stack;         // QG_OPT_BATCHED_STACKED, a complex / mixed member of a batched plan: the stacked block-diagonal form takes it
                          // (QStackMode; bd stays 0: nothing that serves the real form sees such a member)
    int bd_tree;          // QG_OPT_BATCHED_TREE, a member of a batched plan on the tiled 32-bit tree kernels: the tiles of ONE member in the
                          // one launch of the kernel's batched twin (qg_tree_bd.h); 0: not that form
};
// tiles of the tiled 32-bit tree kernels (qg_tree_fast.hip; qg_tree_cplx.hip: 32 rows, its packed 16-bit form 64)
enum { QG_TREE_TILE_M = 64, QG_TREE_TILE_N = 32, QG_TREE_CPLX_TILE_M = 32, QG_TREE_BD_MAX_LEVELS = 12 };
// the stacked block-diagonal form: which operands carry two parts, i.e. which source tiles of the workspace one output tile has
enum QStackMode { QG_STACK_NONE = 0, QG_STACK_CPLX = 1, QG_STACK_REAL_A = 2, QG_STACK_REAL_B = 3 };

// Batched plan (qg_batched_geometry; batch > 0): `batch` GEMMs of one descriptor at constant strides.  Next to it stand two QPlanGeoms:
// the MEMBER's, and the STACK's, which is the member's with info (packed_bytes of the whole batch) and, in the block-diagonal form
// (bd: one launch of k_mfma's BD form over the stacked operands), the stack's packed geometries in pa / pb — the member's with
// batch times the rows, one plane-mask trailer and one row-sum array behind the planes of all members.  bd == 0: member by member,
// unless bd_stack (QG_OPT_BATCHED_STACKED): the members' two-part packed operands back to back ([part][row tile][k tile][limb][TM][BK]
// each; pa / pb.rows_p: ALL rows of the stack, parts included), one plane-mask trailer, no row sums, and the launch's raw dot products
// in a workspace of stack_ws bytes: bd_tm x bd_tn tiles of 64 x 64 int64 per member, which k_stack_combine_bd turns into packed C.
struct QBatchGeom {
    int64_t batch;
    int64_t stack_ws;     // bd_stack: bytes of the workspace between the two launches
    int32_t bd_tm, bd_tn; // bd_stack: tiles of ONE member in the launch (its parts included)
    int member_launches;  // kernel launches of one member's execute (with a chain: its pass included unless fused)
    int64_t mstride[3];   // the packed operands' stride from member to member
    // element-wise chain (qgemul_plan_create_batched_epx).  e_shared[k]: stage k's tensor operand is ONE M x N tensor for every member;
    // estride[k]: bytes of one member's packed operand of stage k (0: no tensor operand) = the step from member to member of a
    // per-member one.  With bd the chain runs inside the block-diagonal launch (bd_fused: k_mfma_ep_bd) or as one block-diagonal pass
    // over the stack's packed C; without bd member by member
    uint8_t e_shared[QG_MAX_EW];
    int bd_fused;
    int64_t estride[QG_MAX_EW];
};

// Grouped plan (qgemul_plan_create_grouped): `groups` descriptors, analysed once per DISTINCT descriptor (ug / up: its geometry and its
// plain plan, which owns the device resources and serves pack, unpack and — for a straggler — execute).  The members in the one
// grouped launch have the batched analysis' 64 x 64 geometry; their packed operands sit back to back in front of the launch's one
// trailer and one row-sum array (sa / sb: the stack's geometry), the stragglers' behind them.  tiles: the schedule (qg_grp.h).
struct QGrpMember {
    int32_t uniq, in_launch;
    int64_t off[3], bytes[3];   // inside packed A / B / C
    int64_t row_a, row_b;       // in the launch: first row of the member in the stack's row sums
    QPackedGeom pa, pb;         // in the launch: the member's geometry with trailer / row sums relative to ITS start (qg_launch_pack_member)
    int64_t eoff[QG_MAX_EW];    // with a chain: byte offset of the member inside stage k's packed tensor operand
};
struct QGrouped {
    int64_t groups, n_uniq, n_in, n_tiles;
    qgemul_desc* ud;            // [n_uniq]
    QPlanGeom* ug;              // [n_uniq]
    uint8_t* u_in;              // [n_uniq]: in the launch
    qgemul_plan** up;           // [n_uniq]; nullptr entries while classifying
    QGrpMember* m;              // [groups]
    int64_t key;                // the distinct descriptor whose launch key the launch has (-1: no member is eligible)
    QPackedGeom sa, sb;
    int launches;
    QGrpTile* tiles;            // [n_tiles] host
    QGrpTile* tiles_dev;
    // Element-wise chain (qgemul_plan_create_grouped_epx; has_ep).  ONE chain serves the group: off[2] / bytes[2] of a member then describe
    // packed D, and stage k's packed tensor operand follows D's layout (QGrpMember::eoff, ebytes[k] = the whole group's bytes; 0: no
    // tensor operand).  The members in the launch run the chain inside the launch's epilogue (fused: k_mfma_ep_grp) or as ONE pass over
    // the launch's packed C (cwork_dev, launch_elems elements) whose workgroup w finds its member in tile_member[w] (qg_grp.h); a
    // straggler runs its own plain _epx plan.  per_member[k]: scalar stage k takes member g's raw value scal[k][g] (host copy for the
    // stragglers, scal_dev[k] for the launch; scal_set[k]: qgemul_grouped_set_scalars has filled them) instead of the call's e_scalar[k].
    int has_ep, has_ax, fused;
    uint32_t flags;             // the plan's option flags
    int64_t launch_elems;
    uint8_t per_member[QG_MAX_EW], scal_set[QG_MAX_EW];
    int64_t ebytes[QG_MAX_EW];
    int32_t* tile_member;       // [n_tiles] host (pass form)
    int32_t* tile_member_dev;
    int64_t* scal[QG_MAX_EW];   // [groups] host
    int64_t* scal_dev[QG_MAX_EW];
    void* cwork_dev;
    ~QGrouped()
    {
        delete[] ud, delete[] ug, delete[] u_in, delete[] up, delete[] m, delete[] tiles, delete[] tile_member;
        for (int k = 0; k < QG_MAX_EW; ++k) delete[] scal[k];
    }
};

#pragma GCC visibility push(hidden)   // internal to the library: nothing here is an exported symbol
int qg_pow2_bytes(int storage_bits);
inline int64_t qg_round_up(int64_t x, int64_t m) { return (x + m - 1) / m * m; }
// tile geometry of a plain plan / of a batched plan (variant 0: no kernel / no block-diagonal form, the member runs alone on `plain`)
QMfmaCfg qg_mfma_pick(int LA, int LB, int64_t M, int64_t N, uint32_t opt_flags = 0);
QMfmaCfg qg_mfma_pick_batched(int LA, int LB, int64_t batch, const QMfmaCfg& plain);
// composite linear plans (see QComposite): reduction indices of chunk c; the packed sub-operand (chunk c, group g) of operand `which`
// (0 A, 1 B): its bytes, its geometry and its byte offset in the packed operand
int64_t qg_comp_sub_bytes(int limbs, int64_t rows_p, int64_t K_p);
int64_t qg_comp_chunk_len(const QComposite& q, int64_t K, int c);
QPackedGeom qg_comp_sub_geom(const QComposite& q, const QPackedGeom& base, int which, int64_t K, int c, int g, int64_t* off);
int qg_comp_split(int L, int* sizes, int* first);
bool qg_comp_geometry(int LA, int LB, const qgemul_desc* d, uint32_t flags, QComposite* q, QMfmaCfg* cfg);
// a chain that came in through an _epcx entry point and holds a CMUL stage in either part (such a chain is planned in lock step)
bool qg_view_has_cmul(const EpView* ev);
// fill info + geometry for a descriptor; batch > 0: the member of a batched plan
// ev: the element-wise chain (nullptr: none); axt / cmt: receive the pre-resolved tables of APPROX / CMUL stages (nullptr: not wanted)
int qg_plan_geometry(const qgemul_desc* d, uint32_t flags, const EpView* ev, int64_t batch, QPlanGeom* out, QApproxTable* axt, QCmulStage* cmt);
// the single-limb kernel stores raw dot products and a 64-bit pass converts them / the kernel's epilogue runs the chain
bool qg_wide_epilogue(const QPlanGeom* p);
bool qg_fuses_epilogue(const QPlanGeom* p, uint32_t flags, bool has_ax, bool has_cmul);
// kernel launches of one qgemul_execute on a plain plan (a 3 x 3 launch pair counts once: its partner returns in its first instructions)
int qg_plan_launches(const QPlanGeom* p);
// host elements one member of operand `operand` spans at leading dimension ld (0: tight); 0: ld is too small
int64_t qg_member_extent(const qgemul_desc& d, int operand, int64_t ld);
// the geometry of a batched plan: m, s, b (all zeroed) receive the member's, the stack's and the batch's (QBatchGeom); s->info says why a
// descriptor was refused.  ev: the chain of a batched plan with one, bep: which of its tensor operands are shared
int qg_batched_geometry(const qgemul_desc* d, int64_t batch, uint32_t flags, const EpView* ev, const qgemul_batched_ep* bep, QPlanGeom* m, QPlanGeom* s, QBatchGeom* b);
int qg_batched_launches(const QPlanGeom* s, const QBatchGeom* b, bool has_ep);
// the launch key of a grouped plan: what the instantiation of k_mfma_grp and its uniform arguments depend on
bool qg_same_launch_key(const QPlanGeom& x, const QPlanGeom& y);
inline bool qg_grp_empty(const qgemul_desc& d) { return d.M == 0 || d.N == 0; }
// the geometry of a grouped plan: G (fresh) and info receive it; info says why a descriptor was refused
// ev: the ONE element-wise chain of a grouped plan with one (nullptr: none), gep: which of its scalar stages take per-member values
int qg_grouped_geometry(const qgemul_desc* d, int64_t groups, uint32_t flags, QGrouped* G, qgemul_info* info, const EpView* ev = nullptr,
                        const qgemul_grouped_ep* gep = nullptr);
void qg_grouped_member_out(const QGrouped* G, int64_t g, qgemul_grouped_member* out);
#pragma GCC visibility pop
