// qg_geom.cpp — plan geometry (qg_geom.h): the kernel and tile geometry a descriptor gets, the packed layouts of A, B and C, the
// composite, batched and grouped forms built from them.  Nothing here launches or needs a device.
#include "qg_geom.h"

#include <stdio.h>
#include <string.h>

#include <new>

int qg_pow2_bytes(int storage_bits)
{
    int b = (storage_bits + 7) / 8;
    int c = 1;
    while (c < b) c *= 2;
    return c;
}

QMfmaCfg qg_mfma_pick(int LA, int LB, int64_t M, int64_t N, uint32_t opt_flags)
{
    QMfmaCfg c = {QG_MFMA_NONE, 0, 0, 0};
    if (LA < 1 || LB < 1 || LA > 3 || LB > 3) return c;
    if (LA == 1 && LB == 1) {
        // 256x256 tiles halve the L2->LDS traffic per MAC; use them once they fill the 256 CUs
        const int64_t big = ((M + 255) / 256) * ((N + 255) / 256);
        // two wave groups alternating on the matrix cores, 128-byte k-tiles (qg_mfma_pp.hip); QG_OPT_LOCKSTEP_TILES keeps k_mfma16
        if (big >= 256) return (opt_flags & QG_OPT_LOCKSTEP_TILES) ? QMfmaCfg{QG_MFMA_256, 256, 256, 64} : QMfmaCfg{QG_MFMA_PP, 256, 256, 128};
        // small problems: 64x64 tiles once 128x128 ones would leave more than half of the 256 CUs without a workgroup
        // (1024^2: 64 -> 256 workgroups)
        const int64_t mid = ((M + 127) / 128) * ((N + 127) / 128);
        static const bool no_small = QG_DIAG_ENV("QG_NO_SMALL_TILES");   // A/B switch for tools/measure_small.py
        if (!no_small && mid <= 128 && ((M + 63) / 64) * ((N + 63) / 64) > mid) {
            // 128-byte k-tiles: these launches are bound by the per-k-tile barrier, DMA issue and exposed fragment reads of a
            // one-wave-per-SIMD workgroup (~0.2 us per 64-byte k-tile whatever the ring depth), so half as many k-tiles:
            // 1024^3 5.97 -> 5.35 us, 512^2 x 4096 13.3 -> 10.2 us (profiles/r03n_small_ring.jsonl).  QG_BK64 for A/B.
            static const bool bk64 = QG_DIAG_ENV("QG_BK64");
            return bk64 ? QMfmaCfg{QG_MFMA_64, 64, 64, 64} : QMfmaCfg{QG_MFMA_64_BK128, 64, 64, 128};
        }
        {   // at most one workgroup per CU: 128-byte k-tiles here as well (2048^2 x 8192 55.3 -> 44.8 us, 1792^2 x 4096 30.8 -> 24.4 us,
            // 2048^3 15.3 -> 15.2 us); with more workgroups the 96 KB LDS image would cost co-residency.  QG_BK64 for A/B.
            static const bool bk64 = QG_DIAG_ENV("QG_BK64");
            if (!bk64 && mid <= 256) return QMfmaCfg{QG_MFMA_128_BK128, 128, 128, 128};
        }
        return QMfmaCfg{QG_MFMA_128, 128, 128, 64};
    }
    {   // limb kernels: the same small-problem rule (1024^2 outputs: 64 -> 256 workgroups)
        static const bool no_small = QG_DIAG_ENV("QG_NO_SMALL_TILES");
        const int64_t mid = ((M + 127) / 128) * ((N + 127) / 128);
        // 3 x 3 limbs with at least a tile per CU: the two-group kernel (qg_mfma_ppl.hip; same packed layout as QG_MFMA_LIMB_128)
        // (2 x 2: unless the operands are Karatsuba-eligible, which qg_plan_geometry decides and then returns to QG_MFMA_LIMB_128)
        if (((LA == 3 && LB == 3) || (LA == 2 && LB == 2)) && mid >= 256 && !(opt_flags & QG_OPT_LOCKSTEP_TILES)) return QMfmaCfg{QG_MFMA_PPL, 128, 128, 64};
        if (!no_small && mid <= 128 && ((M + 63) / 64) * ((N + 63) / 64) > mid) return QMfmaCfg{QG_MFMA_LIMB_64, 64, 64, 64};
    }
    return QMfmaCfg{QG_MFMA_LIMB_128, 128, 128, 64};
}

// Tile geometry of a batched plan.  The block-diagonal launch exists for members that alone would leave CUs idle: a member the
// plain planner gives to a two-group kernel or to 256x256 tiles (a tile per CU on its own) has no such form and runs member by
// member.  Every other member gets 64x64 tiles, the small-problem kernels of qg_mfma_pick: single limb on 128-byte k-tiles,
// limbs on 64-byte ones.  This rule is NOT the outcome of a 64x64-against-128x128 timing: no 128x128 block-diagonal kernel
// exists to time.  The single-limb 128x128 instantiation of the body keeps a 320-byte private array in scratch (hipcc's resource
// report; its non-batched twin does too), which the block-diagonal form may not have (tests/test_batched_resources.py), and
// the 128x128 limb geometries have not been instantiated.  So neither the batch's total tile count nor
// the member's padding waste enters yet: with one tile size there is nothing for them to choose between.  What WAS measured is
// the 64x64 form against the loop of plain launches, 33x to 1100x at the twelve points of tools/measure_batched.py
// (profiles/batched_measure.jsonl): the loop is bound by its launches, 3 to 11 us per member.
QMfmaCfg qg_mfma_pick_batched(int LA, int LB, int64_t batch, const QMfmaCfg& plain)
{
    const QMfmaCfg none = {QG_MFMA_NONE, 0, 0, 0};
    if (batch < 1 || LA < 1 || LB < 1 || LA > 3 || LB > 3) return none;
    switch (plain.variant) {
    case QG_MFMA_128: case QG_MFMA_64: case QG_MFMA_LIMB_64: case QG_MFMA_64_BK128: case QG_MFMA_128_BK128: case QG_MFMA_LIMB_128: break;
    default: return none;   // two-group kernels, 256x256 tiles, three-digit and ring plans
    }
    if (LA != 1 || LB != 1) return QMfmaCfg{QG_MFMA_LIMB_64, 64, 64, 64};
    return QMfmaCfg{QG_MFMA_64_BK128, 64, 64, 128};
}

// ---- composite linear plans (see QComposite) ----
int64_t qg_comp_sub_bytes(int limbs, int64_t rows_p, int64_t K_p)
{
    return qg_round_up((int64_t)limbs * rows_p * K_p + (limbs > 1 ? QG_TRAILER_BYTES : 0), 256);
}
int64_t qg_comp_chunk_len(const QComposite& q, int64_t K, int c) { return c + 1 < q.nc ? q.kc : K - (int64_t)(q.nc - 1) * q.kc; }
QPackedGeom qg_comp_sub_geom(const QComposite& q, const QPackedGeom& base, int which, int64_t K, int c, int g, int64_t* off)
{
    const int* L = which ? q.lb : q.la;
    const int* L0 = which ? q.lb0 : q.la0;
    const int ng = which ? q.gb : q.ga;
    const int64_t K_p = qg_round_up(qg_comp_chunk_len(q, K, c), base.bk);
    QPackedGeom s = base;
    s.K_p = K_p;
    s.limbs = L[g];
    s.limb0 = L0[g];
    s.trailer = L[g] > 1 ? (int64_t)L[g] * base.rows_p * K_p : 0;
    s.digit6 = 0;
    int64_t o = (int64_t)c * q.chunk_bytes[which];
    for (int h = 0; h < g && h < ng; ++h) o += qg_comp_sub_bytes(L[h], base.rows_p, K_p);
    if (off) *off = o;
    if (base.offs) {   // centred operand: ONE row-sum array behind all sub-operands; the groups that hold digit 0 add their k-chunk to it
        s.offs = L0[g] == 0 ? 2 : 3;
        s.rowsum_off = base.rowsum_off - o;
    }
    return s;
}
// groups of 2-3 limbs, low limbs first
int qg_comp_split(int L, int* sizes, int* first)
{
    static const int tab[9][3] = {{0, 0, 0}, {1, 0, 0}, {2, 0, 0}, {3, 0, 0}, {2, 2, 0}, {3, 2, 0}, {3, 3, 0}, {3, 2, 2}, {3, 3, 2}};
    if (L < 1 || L > 8) return 0;
    int n = 0, f = 0;
    for (int i = 0; i < 3 && tab[L][i]; ++i) { sizes[n] = tab[L][i]; first[n] = f; f += tab[L][i]; ++n; }
    return n;
}
bool qg_comp_geometry(int LA, int LB, const qgemul_desc* d, uint32_t flags, QComposite* q, QMfmaCfg* cfg)
{
    memset(q, 0, sizeof *q);
    q->ga = qg_comp_split(LA, q->la, q->la0);
    q->gb = qg_comp_split(LB, q->lb, q->lb0);
    if (!q->ga || !q->gb) return false;
    int maxa = 0, maxb = 0;
    bool single = true;
    for (int i = 0; i < q->ga; ++i)
        for (int j = 0; j < q->gb; ++j) {
            const QMfmaCfg c = qg_mfma_pick(q->la[i], q->lb[j], d->M, d->N, flags);
            if (!c.variant) return false;
            if (i + j == 0) *cfg = c;
            else if (c.TM != cfg->TM || c.TN != cfg->TN || c.BK != cfg->BK) return false;   // (one packed layout for all pairs)
            q->var[i][j] = c.variant;
            if (q->la[i] > maxa) maxa = q->la[i];
            if (q->lb[j] > maxb) maxb = q->lb[j];
            single = single && q->la[i] == 1 && q->lb[j] == 1;
        }
    // int32 accumulators of a limb weight collect min(la, lb) products of magnitude <= 2^14 per reduction index
    const int mn = maxa < maxb ? maxa : maxb;
    const int64_t kmax = (((1ll << 17) - 1) / mn) / 256 * 256;
    q->nc = (int)((d->K + kmax - 1) / kmax);
    q->kc = q->nc > 1 ? kmax : d->K;
    q->slab_bytes = single ? 4 : 8;
    q->on = 1;
    return true;
}

bool qg_view_has_cmul(const EpView* ev)
{
    if (!ev || !ev->cx || !ev->im) return false;
    for (int p = 0; p < 2; ++p)
        for (uint32_t k = 0; k < ev->epc->part[p].n_stages && k < QG_MAX_EW; ++k)
            if (ev->epc->part[p].stage[k].op == QG_EW_CMUL) return true;
    return false;
}

namespace {   // ---- qg_plan_geometry and its stages ----

int storage_bits(const qfmt* f, int parts)
{
    int m = 0;
    for (int p = 0; p < parts; ++p) {
        int b = 1 + (int)f[p].I + (int)f[p].F;
        if (b > m) m = b;
    }
    return m;
}
int value_bits(qfmt f) { return (int)f.I + (int)f.F + (f.S ? 1 : 0); }
int refuse(qgemul_info* info, int st, const char* why)
{
    info->supported = 0;
    snprintf(info->reason, sizeof info->reason, "%s", why);
    return st;
}

// The single-limb MFMA kernels keep the dot product in int32 and run their epilogue in 32 bits.  An exact LEFT shift into a C
// with finer fracBits can leave 32 bits before the overflow handling sees the value (found by tests/extended_fuzz.py:
// int<10,-3> operands into Qu<5,7>, shift by 13).  Those descriptors store the raw dot products and convert them in the
// 64-bit linear pass instead, which keeps the hot kernels' epilogue as it is.
// ... and a C format beyond 31 value bits does not fit the 32-bit epilogue's clamp bounds at all (second find of the
// extended fuzz runs: int<7,-2> x int<7,-1> into Qu<24,9>)
bool raw_dot_pass(int kernel, const QStep& q, int dot_bits)
{
    return kernel == QG_KERNEL_MFMA_I8 && !q.identity && (q.W > 30 || (q.d < 0 && dot_bits - q.d > 31));
}

// one call of qg_plan_geometry: its arguments, the parts of *out under their names, and what the stages hand on to each other
struct Planner {
    const qgemul_desc* const d;
    const uint32_t flags;
    const EpView* const ev;
    const qgemul_epilogue* const ep;   // the chain (a complex one: of the real parts); nullptr: none
    const int64_t batch;
    QPlanGeom* const out;
    QAnalysis* const an = &out->an;
    qgemul_info* const info = &out->info;
    QPackedGeom *const pa = &out->pa, *const pb = &out->pb;
    QCGeom* const pc = &out->pc;
    QHostElem* const hc = &out->hc;
    QComposite& comp = out->comp;
    const int parts = d->is_complex ? 2 : 1;
    // one real and one complex operand (QG_CMUL_REAL_A / QG_CMUL_REAL_B): complex-ness is a property of each operand
    const bool mixed = d->is_complex && (d->cmul == QG_CMUL_REAL_A || d->cmul == QG_CMUL_REAL_B);
    const int parts_a = d->is_complex && d->cmul != QG_CMUL_REAL_A ? 2 : 1, parts_b = d->is_complex && d->cmul != QG_CMUL_REAL_B ? 2 : 1;
    int LA = 0, LB = 0, kernel = QG_KERNEL_NONE;
    int64_t centreA = 0, centreB = 0;
    bool centred = false;
    QMfmaCfg cfg = {0, 0, 0, 0};
    bool bd = false;                  // batch > 0 and k_mfma has a block-diagonal form for the member: see linear_kernel
    // QG_OPT_BATCHED_STACKED on a batched plan without a chain (a grouped plan's members come in without the flag): a complex or mixed
    // member may take the stacked block-diagonal form; stacked: it does (see linear_kernel)
    const bool want_stack = batch > 0 && (flags & QG_OPT_BATCHED_STACKED) && d->is_complex && !ev;
    bool stacked = false;
    bool k6 = false, ppl33 = false;   // the six-product kernel / the 3 x 3 body of k_mfma_ppl takes the plan


    // 1. the analysis, the host elements and the header of info
    int analysis_and_header()
    {
        out->bd = 0;
        out->bd_stack = QG_STACK_NONE;
        out->bd_tree = 0;
        memset(&comp, 0, sizeof comp);
        qg_analyze(d, an);
        memset(info, 0, sizeof *info);
        snprintf(info->reason, sizeof info->reason, "%s", an->reason);
        if (an->status != QG_OK) {
            info->supported = 0;
            return an->status;
        }
        out->ha = qg_host_elem(d->a, parts_a == 2);
        out->hb = qg_host_elem(d->b, parts_b == 2);
        *hc = qg_host_elem(d->c, d->is_complex);
        info->cls = an->cls;
        info->max_bits = an->max_bits;
        info->supported = 1;
        info->in_bits[0] = storage_bits(d->a, parts_a);
        info->in_bits[1] = storage_bits(d->b, parts_b);
        const QHostElem* h[3] = {&out->ha, &out->hb, hc};
        for (int w = 0; w < 3; ++w) {
            info->host_elem_bytes[w] = h[w]->size;
            info->host_imag_off[w] = h[w]->off[1];
        }
        const double mnk = (double)d->M * (double)d->N * (double)d->K;
        info->ops = !d->is_complex ? 2.0 * mnk : mixed ? 4.0 * mnk : (d->cmul == QG_CMUL_TF ? 6.0 * mnk : 8.0 * mnk);
        // what a mixed descriptor is refused: the entry points that have no part-wise form yet (include/qgemul.h)
        if (mixed && ev) return refuse(info, QG_EUNSUPPORTED, "mixed real-complex: no element-wise chain");
        // (under QG_OPT_BATCHED_STACKED the answer waits for the kernel choice: mixed_member_refusal)
        if (mixed && batch > 0 && !want_stack) return mixed_member_refusal();
        return QG_OK;
    }
    int mixed_member_refusal() { return refuse(info, QG_EUNSUPPORTED, "mixed real-complex: no batched or grouped plan"); }

    // 2 + 3, RING plans (qg_plan.cpp: ring_plan; qg_mfma_ring.hip): product and every level wrap into one signed format of n <= 32 bits,
    // so the tree is the dot product modulo 2^n.  The operands keep their first min(L, limbs) balanced digits, L = ceil(n / 8) — no
    // centring, no base-64 digits, no plane-mask shortcut —, and ONE launch takes any K: the accumulators may wrap.  Descriptors
    // that are exact anyway keep their exact linear plan, one output column the one-column kernels walk stays with them, and
    // QG_OPT_FORCE_TREE selects today's tree plan (the invariance arm of the tests).
    void ring_plan()
    {
        const int L = qg_ring_digits(an->ring_n);
        LA = qg_limbs_for(d->a[0]) < L ? qg_limbs_for(d->a[0]) : L;
        LB = qg_limbs_for(d->b[0]) < L ? qg_limbs_for(d->b[0]) : L;
        cfg = QMfmaCfg{QG_MFMA_RING, QG_RING_TM, QG_RING_TN, QG_RING_BK};
        kernel = L == 1 ? QG_KERNEL_MFMA_I8 : QG_KERNEL_MFMA_I8_LIMB;
        const int np = qg_ring_products(LA, LB, L);
        snprintf(info->reason, sizeof info->reason, "linear class: wrapping ring mod 2^%d, %d limb product%s", an->ring_n, np, np == 1 ? "" : "s");
    }

    // 2. limb counts of the linear class
    void linear_limbs()
    {
        LA = qg_limbs_for(d->a[0]);
        LB = qg_limbs_for(d->b[0]);
        if (d->is_complex) {  // parts are stacked along the row axis and share one limb count (a mixed descriptor's real operand has one part)
            const int la2 = parts_a == 2 ? qg_limbs_for(d->a[1]) : 0, lb2 = parts_b == 2 ? qg_limbs_for(d->b[1]) : 0;
            if (la2 > LA) LA = la2;
            if (lb2 > LB) LB = lb2;
        }
        // CENTRED operands (qg_plan.h: qg_limbs_centred; QPackedGeom::offs): x - c in balanced limbs where that saves a limb — signed
        // formats of 16 / 24 / 32 bits (3 -> 2, 4 -> 3, 5 -> 4 limbs), unsigned formats (uint8: 2 -> 1) — the centre taken back out
        // with row sums after the dot product.  Real descriptors only (stacked complex parts have different centres).
        if (d->is_complex || (flags & QG_OPT_BALANCED_LIMBS)) return;
        int64_t c = 0;
        int l = qg_limbs_centred(d->a[0], &c);
        if (l < LA) { LA = l; centreA = c; centred = true; }
        l = qg_limbs_centred(d->b[0], &c);
        if (l < LB) { LB = l; centreB = c; centred = true; }
        // the row sums are int64.  A 64-bit plan may let them wrap (its whole correction is arithmetic modulo 2^64 and the sum
        // itself fits); a wide plan (128-bit combine) may not: there an operand's row sums must fit — |x'| < 2^(8 L - 1) * 1.01,
        // K of them (found by the wide fuzzer: a 56-bit operand over K = 43 519 next to a centred 32-bit one)
        if (centred && an->wide) {
            int lgk = 0;
            while (((int64_t)1 << lgk) < d->K) ++lgk;
            const bool fitA = 8 * LA + lgk <= 62, fitB = 8 * LB + lgk <= 62;
            if ((centreB != 0 && !fitA) || (centreA != 0 && !fitB)) {
                LA = qg_limbs_for(d->a[0]);
                LB = qg_limbs_for(d->b[0]);
                centreA = centreB = 0;
                centred = false;
            }
        }
    }

    // 3. kernel choice of the linear class: a single launch, a composite plan, or the tree kernels after all (kernel stays NONE); the
    // member of a batched plan: whether the block-diagonal form takes it
    void linear_kernel()
    {
        const int mn = LA < LB ? LA : LB;
        QMfmaCfg plain_cfg = {0, 0, 0, 0};   // what qg_mfma_pick chose for the member alone
        cfg = qg_mfma_pick(LA, LB, d->M * parts_a, d->N * parts_b, (ep ? QG_OPT_LOCKSTEP_TILES : 0u) | flags);   // (the fused / unfused element-wise chain keeps the kernel it was measured on)
        // batch > 0: the member of a batched plan.  Where k_mfma has a block-diagonal form for it, the tile geometry comes from
        // qg_mfma_pick_batched (the batch's total tile count, the member's padding waste) and out->bd = 1: the packed layouts then belong
        // to the batched plan and may differ from the plain plan of the same descriptor
        if (batch > 0 && (!d->is_complex || want_stack) && (!ep || !ev->im)) {   // (with a real chain: qgemul_plan_create_batched_epx)
            const QMfmaCfg bc = qg_mfma_pick_batched(LA, LB, batch, cfg);
            if (bc.variant) { plain_cfg = cfg; cfg = bc; bd = true; }
        }
        // (wide plans: the kernels' own epilogues are 64-bit; the composite plan's combine pass is not.  Centred single-limb pairs: the
        //  single-limb kernels' epilogue is 32-bit, sum a b of two uint8 operands is not: raw int32 slab + combine pass)
        // (... except where its image in C fits 31 bits and no element-wise chain follows: the single-limb kernels' epilogues then restore
        //  the sum in 64 bits themselves)
        const QStep& tc = an->lin.to_c[0];
        const bool pp_centred = cfg.variant && !ep && storage_bits(d->c, parts) <= 31 && (tc.identity || (tc.d >= 0 && tc.W <= 30));   // (every single-limb kernel has the 64-bit branch)
        if (cfg.variant && (int64_t)mn * d->K <= (1ll << 17) - 1 && !an->wide && !an->generic_only && !(centred && LA == 1 && LB == 1 && !pp_centred))
            kernel = mixed ? QG_KERNEL_MFMA_RC : d->is_complex ? QG_KERNEL_MFMA_CPLX : ((LA == 1 && LB == 1) ? QG_KERNEL_MFMA_I8 : QG_KERNEL_MFMA_I8_LIMB);
        // (one output column whose tree the one-column kernels can walk: those stream A once at HBM rate; a composite plan would read
        // it once per limb group and write slabs — the batched Qreduce of 32-bit words with exact level types stays there)
        else if (!d->is_complex && !(d->N == 1 && (an->gemv_ok || an->gemv_wide_ok) && !(flags & QG_OPT_GENERIC_TREE)) &&
                 qg_comp_geometry(LA, LB, d, flags, &comp, &cfg)) {
            // more than 3 limbs, or K beyond the int32 accumulators' exact range: limb groups x k-chunks on the same kernels
            kernel = (LA == 1 && LB == 1) ? QG_KERNEL_MFMA_I8 : QG_KERNEL_MFMA_I8_LIMB;
            comp.wide = an->wide;
            snprintf(info->reason, sizeof info->reason, "linear class: %d k-chunk(s) x %d x %d limb groups on the MFMA kernels, exact %s combine", comp.nc, comp.ga, comp.gb,
                     comp.wide ? "128-bit" : "64-bit");
        } else {
            LA = LB = 0;
            centred = false;
            snprintf(info->reason, sizeof info->reason, "linear class, but limbs/K outside the MFMA kernels' range: tree kernel");
        }
        // the block-diagonal form takes what ONE launch of a lock-step kernel with its own conversion serves: no composite plan, no
        // raw-dot-product detour (qg_wide_epilogue).  A member without it runs on the plain plan's own geometry
        // The STACKED form (want_stack): the member's plan is already one real GEMM on stacked parts with an identity epilogue into an
        // int64 workspace, so the block-diagonal launch takes it as it is, on the 64 x 64 geometry, and the combine pass follows it.
        // bd itself stays with the real members: nothing that serves their form (grouped plans, chains) sees a stacked member
        if (bd && want_stack && (kernel == QG_KERNEL_MFMA_CPLX || kernel == QG_KERNEL_MFMA_RC)) {
            stacked = true;
            bd = false;
        }
        if (bd && (comp.on || raw_dot_pass(kernel, tc, an->dot_bits) || (kernel != QG_KERNEL_MFMA_I8 && kernel != QG_KERNEL_MFMA_I8_LIMB))) {
            bd = false;
            if (!comp.on) cfg = plain_cfg;
        }
    }

    // 4. packed layouts.  C: index space, container and host element
    void packed_c()
    {
        pc->M = d->M;
        pc->N = d->N;
        pc->parts = parts;
        pc->cbytes = qg_pow2_bytes(storage_bits(d->c, parts));
        // (a multi-word value in the band the reference mis-compares comes out as its low WORD — int32_t / int64_t — whatever C's
        // format says: such plans keep the host element's width in packed C)
        if (an->band && pc->cbytes < (hc->sb[0] > hc->sb[1] ? hc->sb[0] : hc->sb[1])) pc->cbytes = hc->sb[0] > hc->sb[1] ? hc->sb[0] : hc->sb[1];
        pc->ldc = d->M;
        pc->elem_bytes = hc->size;
        for (int p = 0; p < 2; ++p) { pc->off[p] = hc->off[p]; pc->sb[p] = hc->sb[p]; }
    }

    // Three-digit Karatsuba (qg_mfma_k6.hip): both operands of 17 / 18 value+sign bits (3 limbs each; operands of 2 limbs take 4 or
    // 6 schoolbook products already), real, not centred, no element-wise chain, a shape the two-group 3 x 3 kernel takes, C in a 4-
    // or 8-byte container, and ONE product per int32 accumulator exact: K * 126^2 < 2^31.  The planes then hold the unsigned base-64
    // digits of x + bias on 96-row tiles of A; QG_OPT_SCHOOLBOOK_LIMBS / QG_OPT_LOCKSTEP_TILES keep the balanced limbs.
    void three_digit_choice()
    {
        static const bool no_kara3 = QG_DIAG_ENV("QG_NO_KARA3");   // A/B switch
        const int cb = qg_pow2_bytes(storage_bits(d->c, parts));
        // (what k_mfma_ppl's 3 x 3 body takes: qg_mfma_ppl_applies)
        ppl33 = kernel == QG_KERNEL_MFMA_I8_LIMB && !comp.on && !d->is_complex && !ep && LA == 3 && LB == 3 && cfg.variant == QG_MFMA_PPL && (cb == 4 || cb == 8);
        k6 = ppl33 && !no_kara3 && !(flags & QG_OPT_SCHOOLBOOK_LIMBS) && !centred && !an->band && value_bits(d->a[0]) >= 13 && value_bits(d->a[0]) <= 18 &&
             value_bits(d->b[0]) >= 13 && value_bits(d->b[0]) <= 18 && d->K * (int64_t)(126 * 126) < (1ll << 31);
        if (k6) cfg = QMfmaCfg{QG_MFMA_K6, QG_K6_TM, QG_K6_TN, QG_K6_BK};
    }

    // ... A, B and the tiles of C on an MFMA kernel
    void limb_layout()
    {
        *pa = QPackedGeom{qg_round_up(d->M, cfg.TM), qg_round_up(d->K, cfg.BK), 1, LA, cfg.TM, cfg.BK};
        *pb = QPackedGeom{qg_round_up(d->N, cfg.TN), qg_round_up(d->K, cfg.BK), 1, LB, cfg.TN, cfg.BK};
        if (comp.on) {   // pa / pb: the first sub-operand (group 0 of chunk 0); the others through qg_comp_sub_geom
            pa->K_p = pb->K_p = qg_round_up(comp.kc, cfg.BK);
            pa->limbs = comp.la[0];
            pb->limbs = comp.lb[0];
        }
        pc->Mp = pa->rows_p;
        pc->Np = pb->rows_p;
        pc->tm = cfg.TM;
        pc->tn = cfg.TN;
        if (k6) {   // packed C keeps the 128 x 128 tiles of the other limb plans: callers that size or move packed C see no change
            pc->Mp = qg_round_up(d->M, 128);
            pc->tm = 128;
        }
        if (d->is_complex) {
            // the MFMA kernel writes the raw 2Mh x 2Nh dot products into the plan's workspace; the combine
            // pass writes the packed complex C row-major [2][M][N]
            pc->Mp = d->M;
            pc->Np = d->N;
            pc->tm = pc->tn = 0;
        }
    }

    // ... on a tree kernel, which is chosen here (no MFMA kernel took the descriptor)
    void tree_layout()
    {
        const bool fast = !(flags & QG_OPT_GENERIC_TREE);
        const QTreeChoice tc = qg_tree_choice(an, d, flags, false);
        kernel = tc.kernel;
        // which form of the kernel's steps this descriptor gets (tests assert their coverage through it)
        if (kernel == QG_KERNEL_TREE_I128)
            snprintf(info->reason, sizeof info->reason, "exact tree evaluation on 128-bit values (intermediates of %d bits)", an->max_bits);
        if (kernel == QG_KERNEL_TREE_I32)
            snprintf(info->reason, sizeof info->reason, "exact tree evaluation; tree kernel steps: %s", qg_form_name(tc.tree));
        if (kernel == QG_KERNEL_GEMV_I64)
            snprintf(info->reason, sizeof info->reason, "exact tree evaluation; one-column kernel steps: run-time modes, 64-bit values");
        if (kernel == QG_KERNEL_GEMV_I32)
            snprintf(info->reason, sizeof info->reason, "exact tree evaluation; one-column kernel steps: %s", qg_form_name(tc.gemv));
        if (kernel == QG_KERNEL_TREE_CPLX_I32)
            snprintf(info->reason, sizeof info->reason, "exact tree evaluation; complex kernel steps: %s", qg_form_name(tc.cplx));
        if (mixed) {   // the form's name first: qgemul_info.reason says which mixed product this is
            const char* form = d->cmul == QG_CMUL_REAL_A ? "real x complex" : "complex x real";
            if (kernel == QG_KERNEL_TREE_RC_I32) snprintf(info->reason, sizeof info->reason, "%s: exact tree evaluation; mixed kernel steps: %s", form, qg_form_name(tc.cplx));
            else snprintf(info->reason, sizeof info->reason, "%s: exact tree evaluation, part by part%s", form, kernel == QG_KERNEL_TREE_I128 ? ", on 128-bit values" : "");
        }
        // the 32-bit tree kernels walk a perfect binary tree: their operands are zero-padded along K to 2^n_levels leaves
        // (a node whose right child is a zero leaf / zero subtree is the reference's converting copy of an odd leftover)
        const bool t64 = kernel == QG_KERNEL_TREE_I64 && an->tree64_ok && fast;   // the 2x2-per-lane 64-bit kernel, not the general one
        const int64_t Kt = (kernel == QG_KERNEL_TREE_I32 || kernel == QG_KERNEL_TREE_CPLX_I32 || kernel == QG_KERNEL_TREE_RC_I32 || kernel == QG_KERNEL_GEMV_I32 || kernel == QG_KERNEL_GEMV_I64 || t64)
                               ? ((int64_t)1 << an->tree.n_levels_k) : d->K;   // (n_levels_k: at least 5 levels, qg_plan.h)
        *pa = QPackedGeom{d->M, Kt, info->in_bits[0] <= 32 ? 4 : 8, 0, 0, 0};
        *pb = QPackedGeom{d->N, Kt, info->in_bits[1] <= 32 ? 4 : 8, 0, 0, 0};
        pc->Mp = d->M;
        pc->Np = d->N;
        pc->tm = pc->tn = 0;
    }

    // ... bytes of packed A and B: the planes, the plane-mask trailer, a composite plan's sub-operands, the row sums of centred operands
    int packed_ab_bytes()
    {
        info->packed_bytes[0] = (int64_t)parts_a * (pa->limbs ? pa->limbs : 1) * pa->rows_p * pa->K_p * pa->cbytes;
        info->packed_bytes[1] = (int64_t)parts_b * (pb->limbs ? pb->limbs : 1) * pb->rows_p * pb->K_p * pb->cbytes;
        // multi-limb operands carry their plane mask in a trailer behind the planes (QPackedGeom::trailer)
        if (pa->limbs > 1) { pa->trailer = info->packed_bytes[0]; info->packed_bytes[0] += QG_TRAILER_BYTES; }
        if (pb->limbs > 1) { pb->trailer = info->packed_bytes[1]; info->packed_bytes[1] += QG_TRAILER_BYTES; }
        if (comp.on) {
            // the packed operand = every (chunk, group) sub-operand back to back
            for (int w = 0; w < 2; ++w) {
                const QPackedGeom& base = w ? *pb : *pa;
                const int ng = w ? comp.gb : comp.ga;
                const int* L = w ? comp.lb : comp.la;
                int64_t full = 0, last = 0;
                const int64_t Kl = qg_round_up(qg_comp_chunk_len(comp, d->K, comp.nc - 1), base.bk);
                for (int g = 0; g < ng; ++g) { full += qg_comp_sub_bytes(L[g], base.rows_p, base.K_p); last += qg_comp_sub_bytes(L[g], base.rows_p, Kl); }
                comp.chunk_bytes[w] = full;
                info->packed_bytes[w] = (int64_t)(comp.nc - 1) * full + last;
            }
            pa->trailer = pb->trailer = 0;   // (per sub-operand: qg_comp_sub_geom)
            if ((int64_t)comp.ga * comp.gb * pa->rows_p * pb->rows_p * comp.slab_bytes > (64ll << 30))
                return refuse(info, QG_EUNSUPPORTED, "composite linear plan: the slabs of raw dot products would exceed 64 GiB");
        }
        if (centred && kernel != QG_KERNEL_NONE) {   // both operands carry row sums (an uncentred partner: bias 0), behind everything else
            pa->offs = pb->offs = 1;
            pa->bias = -centreA;
            pb->bias = -centreB;
            pa->rowsum_off = qg_round_up(info->packed_bytes[0], 256);
            pb->rowsum_off = qg_round_up(info->packed_bytes[1], 256);
            info->packed_bytes[0] = pa->rowsum_off + pa->rows_p * 8;
            info->packed_bytes[1] = pb->rowsum_off + pb->rows_p * 8;
        }
        return QG_OK;
    }

    // 5. base-64 digit layouts: the planes hold the unsigned digits of x + bias, the row sums sit behind the trailer
    void digit6_layout()
    {
        QPackedGeom* g[2] = {pa, pb};
        for (int w = 0; w < 2; ++w) {
            const qfmt f = w ? d->b[0] : d->a[0];
            g[w]->digit6 = 1;
            g[w]->bias = f.S ? ((int64_t)1 << ((int)f.I + (int)f.F)) : 0;
            g[w]->rowsum_off = g[w]->trailer + QG_TRAILER_BYTES;
            info->packed_bytes[w] += g[w]->rows_p * 8;
        }
    }
    void digit_layouts()
    {
        // Karatsuba (qg_mfma.hip, KARA): two-limb operands whose biased values fit 12 bits are stored as two unsigned base-64
        // digits each, and the product takes 3 MFMAs per k-step instead of 4
        if (!comp.on && !centred) {
            static const bool no_kara = QG_DIAG_ENV("QG_NO_KARA");   // A/B switch
            // (problems small enough for the 64x64 tiles are latency-bound: measured 9.5 vs 8.9 us at 1024^3, schoolbook kept there)
            if (!no_kara && !d->is_complex && LA == 2 && LB == 2 && (kernel == QG_KERNEL_MFMA_I8_LIMB) && (cfg.variant == QG_MFMA_LIMB_128 || cfg.variant == QG_MFMA_PPL) &&
                value_bits(d->a[0]) <= 12 && value_bits(d->b[0]) <= 12 && d->K * (int64_t)(126 * 126) < (1ll << 31)) {
                cfg.variant = QG_MFMA_LIMB_128;   // three products on the lock-step Karatsuba kernel (same tiles and k-tiles as QG_MFMA_PPL)
                digit6_layout();
            }
        }
        if (k6) {
            digit6_layout();
            snprintf(info->reason, sizeof info->reason, "linear class: three base-64 digits per operand, six products (two-group kernel, 96x128 tiles)");
        } else if (ppl33) {
            snprintf(info->reason, sizeof info->reason, "linear class: balanced base-256 limbs, nine products (two-group kernel, 128x128 tiles)");
        }
    }

    // 6. the element-wise chain: its tables, and D in the place of C as the stored result (same index space, D's container and host element)
    int chain(QApproxTable* axt, QCmulStage* cmt)
    {
        if (an->band) return refuse(info, QG_EUNSUPPORTED, "element-wise chain after a plan whose C can leave its format (multi-word comparison artefact of the reference)");
        if ((d->is_complex != 0) != (ev->im != nullptr))
            return refuse(info, QG_EINVAL, d->is_complex ? "complex GEMM: the chain is a qgemul_epilogue_cplx" : "real GEMM: the chain is a qgemul_epilogue");
        QEpTable* const t[2] = {&out->ept, &out->ept_im};
        qfmt df[2] = {ep->d, ep->d};
        const bool lockstep = qg_view_has_cmul(ev);   // a CMUL stage needs both running values: the part chains are planned together
        if (ev->cx && !lockstep)
            for (int k = 0; k < QG_MAX_EW; ++k)
                if (ev->cx[k]) return refuse(info, QG_EINVAL, "a CMUL record for a stage that is no CMUL stage");
        QEpTable both[2];
        for (int part = 0; part < parts; ++part) {
            const qgemul_epilogue* e = part ? ev->im : ep;
            int ep_bits = 0;
            char why[96];
            int st = QG_OK;
            if (lockstep) {
                if (part == 0) {
                    st = qg_analyze_epcx(d->c, ev->epc, ev->cx, both, cmt, &ep_bits, why, sizeof why);
                    *t[0] = both[0];
                    *t[1] = both[1];
                }
            } else {
                st = qg_analyze_epx(d->c[part], e, part ? nullptr : ev->ax, t[part], part ? nullptr : axt, &ep_bits, why, sizeof why);
            }
            if (st != QG_OK) return refuse(info, st, why);
            if (ep_bits > info->max_bits) info->max_bits = ep_bits;
            df[part] = e->d;
            if (!d->is_complex)
                for (uint32_t k = 0; k < e->n_stages; ++k)
                    if (e->stage[k].op == QG_EW_PASS) return refuse(info, QG_EINVAL, "QG_EW_PASS: complex chains only");
        }
        if (d->is_complex) {
            // the two chains describe the same operators: same length; a tensor operand is one packed buffer in one container;
            // a real operand has no imaginary half to read
            if (ev->im->n_stages != ep->n_stages) return refuse(info, QG_EINVAL, "complex chain: the part chains differ in length");
            for (int k = 0; k < t[0]->n; ++k) {
                QEpStage &a = t[0]->st[k], &b = t[1]->st[k];
                const bool ta = a.op != QG_EW_PASS && !a.scalar, tb = b.op != QG_EW_PASS && !b.scalar;
                if (ev->e_cplx[k] && ta != tb) return refuse(info, QG_EINVAL, "complex chain: a complex tensor operand feeds both parts");
                if (!ev->e_cplx[k] && ta && tb && !same_fmt(ep->stage[k].e, ev->im->stage[k].e)) return refuse(info, QG_EINVAL, "complex chain: a real tensor operand has one format");
                if (ta && tb) a.ebytes = b.ebytes = a.ebytes > b.ebytes ? a.ebytes : b.ebytes;
            }
            t[0]->dbytes = t[1]->dbytes = t[0]->dbytes > t[1]->dbytes ? t[0]->dbytes : t[1]->dbytes;
        }
        *hc = qg_host_elem(df, d->is_complex);
        pc->cbytes = t[0]->dbytes;
        pc->elem_bytes = hc->size;
        for (int part = 0; part < 2; ++part) { pc->off[part] = hc->off[part]; pc->sb[part] = hc->sb[part]; }
        info->host_elem_bytes[2] = hc->size;
        info->host_imag_off[2] = hc->off[1];
        info->packed_bytes[2] = (int64_t)parts * pc->Mp * pc->Np * pc->cbytes;
        return QG_OK;
    }
};

}   // namespace

int qg_plan_geometry(const qgemul_desc* d, uint32_t flags, const EpView* ev, int64_t batch, QPlanGeom* out, QApproxTable* axt, QCmulStage* cmt)
{
    Planner p = {d, flags, ev, ev ? ev->re : nullptr, batch, out};
    if (const int st = p.analysis_and_header(); st != QG_OK) return st;
    if (p.an->ring_ok && !(flags & QG_OPT_FORCE_TREE)) {
        p.ring_plan();
    } else if (p.an->linear_ok && !(flags & QG_OPT_FORCE_TREE)) {
        p.linear_limbs();
        p.linear_kernel();
    }
    // a mixed member without the stacked form is refused as without QG_OPT_BATCHED_STACKED (nothing but the header of info is filled yet)
    if (p.mixed && batch > 0 && !p.stacked) return p.mixed_member_refusal();
    out->bd_stack = !p.stacked ? QG_STACK_NONE : !p.mixed ? QG_STACK_CPLX : d->cmul == QG_CMUL_REAL_A ? QG_STACK_REAL_A : QG_STACK_REAL_B;
    p.packed_c();
    p.three_digit_choice();
    if (p.kernel != QG_KERNEL_NONE) p.limb_layout();
    else p.tree_layout();
    if (p.kernel == QG_KERNEL_MFMA_RC)
        snprintf(out->info.reason, sizeof out->info.reason, "%s: linear class, one %d x %d limb GEMM on the stacked operand + two-product convert",
                 d->cmul == QG_CMUL_REAL_A ? "real x complex" : "complex x real", p.LA, p.LB);
    out->bd = p.bd ? 1 : 0;
    out->info.kernel = p.kernel;
    out->info.limbs[0] = p.LA;
    out->info.limbs[1] = p.LB;
    if (const int st = p.packed_ab_bytes(); st != QG_OK) return st;
    p.digit_layouts();
    out->info.packed_bytes[2] = (int64_t)p.parts * out->pc.Mp * out->pc.Np * out->pc.cbytes;
    out->LA = p.LA;
    out->LB = p.LB;
    out->cfg = p.cfg;
    out->variant = p.cfg.variant;
    out->pc_c = out->pc;
    return p.ep ? p.chain(axt, cmt) : QG_OK;
}

// Where the chain runs (measurements: profiles/r01v_eltwise.jsonl, chain = scale + bias into C's own type):
//   3x3-limb kernel, 4096^3: plain 0.458 ms, chain fused into the kernel's epilogue 0.473, chain as a pass 0.490
//   single-limb 256^2-tile kernel, 8192^2 x 4096: plain 0.280, fused 0.503, pass 0.436  (the fused epilogue spills:
//   128 accumulator registers stay live; and with one workgroup per CU the matrix cores idle meanwhile)
// so the default fuses on the limb kernel only, and only chains the planner has bounded by 32-bit arithmetic (a 64-bit
// chain inside the kernel was measured slower than the pass on every kernel).  Everything else runs as ONE linear,
// HBM-bound pass over the stored C (all stages and the final conversion in that pass, 5-6 TB/s).
bool qg_wide_epilogue(const QPlanGeom* p)
{
    if (p->comp.on || p->variant == QG_MFMA_RING) return false;   // (the combine pass / the ring kernel's epilogue convert in 64-bit arithmetic anyway)
    return raw_dot_pass(p->info.kernel, p->an.lin.to_c[0], p->an.dot_bits);
}

bool qg_fuses_epilogue(const QPlanGeom* p, uint32_t flags, bool has_ax, bool has_cmul)
{
    if (has_ax) return false;   // (an APPROX stage: always the pass of qg_approx.hip)
    if (has_cmul) return false; // (a CMUL stage: always the pass of qg_eltwise_cplx.hip)
    if (qg_wide_epilogue(p) || p->comp.on || p->variant == QG_MFMA_RING) return false;
    if (flags & QG_OPT_UNFUSED_EPILOGUE) return false;
    if (!p->ept.bits32) return false;
    if (p->info.kernel == QG_KERNEL_MFMA_I8_LIMB && p->LA == 3 && p->LB == 3) return true;
    return p->info.kernel == QG_KERNEL_MFMA_I8 && (flags & QG_OPT_FUSED_EPILOGUE);
}

int qg_plan_launches(const QPlanGeom* p)
{
    if (p->comp.on) return p->comp.nc * (p->comp.ga * p->comp.gb + 1);
    switch (p->info.kernel) {
    case QG_KERNEL_MFMA_I8:
    case QG_KERNEL_MFMA_I8_LIMB: return p->variant != QG_MFMA_RING && qg_wide_epilogue(p) ? 2 : 1;
    case QG_KERNEL_MFMA_CPLX:
    case QG_KERNEL_MFMA_RC: return 2;
    default: return 1;
    }
}

int64_t qg_member_extent(const qgemul_desc& d, int operand, int64_t ld)
{
    const int64_t rows = operand == QG_OPERAND_A ? (d.transA ? d.K : d.M) : operand == QG_OPERAND_B ? d.K : d.M;
    const int64_t cols = operand == QG_OPERAND_A ? (d.transA ? d.M : d.K) : d.N;
    if (!ld) ld = rows;
    if (ld < rows) return 0;
    return cols > 0 && rows > 0 ? (cols - 1) * ld + rows : 1;
}

// ---- batched Qgemul: `batch` GEMMs of one descriptor at constant strides (include/qgemul.h) ----
// the block-diagonal form: the stack's packed geometries, total[] = the stack's bytes; true: beyond the tile / address range
// The STACKED form (m->bd_stack): an operand of two parts brings both into the stack — a member's packed operand is [part][row tile]
// ..., so member b owns parts * rows_p / TM consecutive row tiles and the stack's rows_p counts them all —, the launch has bd_tm x bd_tn
// tiles per member, its raw dot products go into a workspace of 64 x 64 int64 tiles (stack_ws), and packed C keeps the step of the
// member-by-member form.  Complex plans are never centred (linear_limbs), a mixed plan's real operand included: no row sums.
static bool batched_stack(const QPlanGeom* m, int64_t batch, QPlanGeom* s, QBatchGeom* b, int64_t total[3])
{
    const int64_t parts[2] = {m->bd_stack == QG_STACK_CPLX || m->bd_stack == QG_STACK_REAL_B ? 2 : 1, m->bd_stack == QG_STACK_CPLX || m->bd_stack == QG_STACK_REAL_A ? 2 : 1};
    const int64_t tm = parts[0] * (m->pa.rows_p / m->cfg.TM), tn = parts[1] * (m->pb.rows_p / m->cfg.TN);
    int64_t tiles = 0;
    bool over = __builtin_mul_overflow(tm * tn, batch, &tiles) || tiles > 0x7fffffffll;
    if (m->bd_stack) {
        b->bd_tm = (int32_t)tm;
        b->bd_tn = (int32_t)tn;
        over |= m->pa.offs != 0 || m->pb.offs != 0 || __builtin_mul_overflow(tiles, (int64_t)m->cfg.TM * m->cfg.TN * 8, &b->stack_ws) || b->stack_ws > (1ll << 60);
    }
    QPackedGeom* sg[2] = {&s->pa, &s->pb};
    const QPackedGeom* mg[2] = {&m->pa, &m->pb};
    for (int w = 0; w < 2 && !over; ++w) {
        QPackedGeom& g = *sg[w];
        g = *mg[w];
        int64_t planes = 0;
        over |= __builtin_mul_overflow(g.rows_p * parts[w], batch, &g.rows_p) || __builtin_mul_overflow((int64_t)g.limbs * g.K_p, g.rows_p, &planes) || planes > (1ll << 60);
        b->mstride[w] = parts[w] * mg[w]->limbs * mg[w]->rows_p * mg[w]->K_p;
        int64_t bytes = planes;
        g.trailer = 0;
        if (g.limbs > 1) { g.trailer = bytes; bytes += QG_TRAILER_BYTES; }   // ONE plane mask: the OR over every member
        if (g.offs) {                                                         // ONE row-sum array behind the planes of all members
            g.rowsum_off = qg_round_up(bytes, 256);
            bytes = g.rowsum_off + g.rows_p * 8;
        }
        total[w] = bytes;
    }
    b->mstride[2] = m->bd_stack ? qg_round_up(m->info.packed_bytes[2], 256) : m->info.packed_bytes[2];
    over |= __builtin_mul_overflow(b->mstride[2], batch, &total[2]) || (m->bd_stack && total[2] > (1ll << 60));
    return over;
}

// QG_OPT_BATCHED_TREE: the tiles of ONE member in the one launch of its tree kernel's batched twin (qg_tree_bd.h), 0 where the member
// has none: any kernel but the two tiled 32-bit ones, a tree of more than 12 levels (only the 12-level instantiations have a twin)
static int64_t tree_bd_tiles(const QPlanGeom* m, const qgemul_desc* d, uint32_t flags)
{
    const int k = m->info.kernel;
    if ((k != QG_KERNEL_TREE_I32 && k != QG_KERNEL_TREE_CPLX_I32) || m->an.tree.n_levels_k > QG_TREE_BD_MAX_LEVELS) return 0;
    const bool rows64 = k == QG_KERNEL_TREE_I32 || qg_tree_choice(&m->an, d, flags, false).cplx == QCF_PK16;
    const int64_t tm = rows64 ? QG_TREE_TILE_M : QG_TREE_CPLX_TILE_M;
    return ((d->M + tm - 1) / tm) * ((d->N + QG_TREE_TILE_N - 1) / QG_TREE_TILE_N);
}

int qg_batched_geometry(const qgemul_desc* d, int64_t batch, uint32_t flags, const EpView* ev, const qgemul_batched_ep* bep, QPlanGeom* m, QPlanGeom* s, QBatchGeom* b)
{
    if (!d || batch < 1) return QG_EINVAL;
    bool has_ax = false;
    for (int k = 0; ev && ev->ax && k < QG_MAX_EW; ++k) has_ax |= ev->ax[k] != nullptr;
    const int st = qg_plan_geometry(d, flags, ev, batch, m, nullptr, nullptr);
    s->info = m->info;
    if (st != QG_OK) return st;
    b->batch = batch;
    // the stack has the member's kernel, host elements and packed C (pa / pb: below; an and comp stay the member's alone)
    s->bd = m->bd, s->bd_stack = m->bd_stack, s->LA = m->LA, s->LB = m->LB, s->cfg = m->cfg, s->variant = m->variant;
    s->ha = m->ha, s->hb = m->hb, s->hc = m->hc, s->pc = m->pc;
    b->member_launches = qg_plan_launches(m);
    int64_t total[3] = {0, 0, 0};
    bool over = false;
    if (ev) {
        s->ept = m->ept;
        s->pc_c = m->pc_c;
        // the chain is the member's; what one member's qgemul_execute_ep issues: its kernel and, unless fused, the chain's pass
        if (!qg_fuses_epilogue(m, flags, has_ax, false)) b->member_launches += 1;
        // fused form: what qg_fuses_epilogue accepts on arithmetic grounds, on request (the default between the two block-diagonal
        // forms is the pass until tools/measure_batched_ep.py has decided otherwise: DESIGN.md section 9)
        b->bd_fused = m->bd && m->ept.bits32 && !has_ax && (flags & QG_OPT_FUSED_EPILOGUE) && !(flags & QG_OPT_UNFUSED_EPILOGUE);
        for (int k = 0; k < m->ept.n; ++k) {
            const QEpStage& e = m->ept.st[k];
            if (e.scalar || e.op == QG_EW_APPROX) continue;
            b->e_shared[k] = bep && bep->e_shared[k] ? 1 : 0;
            // (member by member: 256-byte steps like the other packed operands', so that every member's operand keeps the alignment the
            // pass's 16-byte loads have on a plain plan)
            int64_t stack = 0;
            over |= __builtin_mul_overflow(m->pc.Mp * m->pc.Np, (int64_t)e.ebytes, &b->estride[k]);
            if (!m->bd) b->estride[k] = qg_round_up(b->estride[k], 256);
            over |= __builtin_mul_overflow(b->estride[k], batch, &stack) || stack > (1ll << 60);
        }
    }
    if (m->bd) {
        over |= batched_stack(m, batch, s, b, total);
        snprintf(s->info.reason, sizeof s->info.reason, "linear class: %lld members in one block-diagonal launch, %dx%d tiles", (long long)batch, m->cfg.TM, m->cfg.TN);
        if (ev)
            snprintf(s->info.reason, sizeof s->info.reason, b->bd_fused ? "linear class: %lld members, chain fused into one block-diagonal launch" : "linear class: %lld members, block-diagonal launch + one chain pass over the stack",
                     (long long)batch);
    } else if (m->bd_stack) {
        over |= batched_stack(m, batch, s, b, total);
        // (every batch count fits qgemul_info.reason)
        if (m->bd_stack == QG_STACK_CPLX) snprintf(s->info.reason, sizeof s->info.reason, "linear class: %lld complex members, one block-diagonal launch + one combine pass", (long long)batch);
        else if (m->bd_stack == QG_STACK_REAL_A) snprintf(s->info.reason, sizeof s->info.reason, "linear class: %lld real x complex members, block-diagonal launch + combine pass", (long long)batch);
        else snprintf(s->info.reason, sizeof s->info.reason, "linear class: %lld complex x real members, block-diagonal launch + combine pass", (long long)batch);
    } else {
        for (int w = 0; w < 3; ++w) {
            b->mstride[w] = qg_round_up(m->info.packed_bytes[w], 256);
            over |= __builtin_mul_overflow(b->mstride[w], batch, &total[w]) || total[w] > (1ll << 60);
        }
        s->pa = m->pa;
        s->pb = m->pb;
        if (ev) snprintf(s->info.reason, sizeof s->info.reason, "chain member by member: %.70s", m->info.reason);
        // the one-launch tree form, on request and without a chain: the layout above is its layout too; more workgroups than a grid
        // holds: member by member
        const int64_t tiles = (flags & QG_OPT_BATCHED_TREE) && !ev ? tree_bd_tiles(m, d, flags) : 0;
        if (tiles > 0 && tiles <= 0x7fffffffll / batch) {
            m->bd_tree = s->bd_tree = (int)tiles;
            const char* steps = strstr(m->info.reason, "; ");   // ("exact tree evaluation; <tree | complex> kernel steps: <form>")
            // (the prefix is no longer than the one it replaces: the longest step-form name still fits qgemul_info.reason)
            snprintf(s->info.reason, sizeof s->info.reason, "batch in one launch; %.74s", steps ? steps + 2 : m->info.reason);
        }
    }
    if (over) {
        s->info.supported = 0;
        snprintf(s->info.reason, sizeof s->info.reason, "batched plan: more than 2^31 - 1 tiles / packed operands beyond the address range");
        return QG_EINVAL;
    }
    for (int w = 0; w < 3; ++w) s->info.packed_bytes[w] = total[w];
    s->info.ops = m->info.ops * (double)batch;
    return QG_OK;
}

int qg_batched_launches(const QPlanGeom* s, const QBatchGeom* b, bool has_ep)
{
    if (s->bd) return has_ep && !b->bd_fused ? 2 : 1;
    if (s->bd_stack) return 2;   // the block-diagonal GEMM and the combine pass
    if (s->bd_tree) return 1;    // the tree kernel's batched twin
    const int64_t n = b->batch * b->member_launches;
    return n > 0x7fffffffll ? 0x7fffffff : (int)n;
}

// ---- grouped Qgemul: GEMMs of different shapes in one launch (include/qgemul.h) ----
bool qg_same_launch_key(const QPlanGeom& x, const QPlanGeom& y)
{
    return x.LA == y.LA && x.LB == y.LB && x.pa.limbs == y.pa.limbs && x.pb.limbs == y.pb.limbs && x.variant == y.variant && x.cfg.BK == y.cfg.BK &&
           x.pa.offs == y.pa.offs && x.pb.offs == y.pb.offs && x.pa.bias == y.pa.bias && x.pb.bias == y.pb.bias && x.pc.cbytes == y.pc.cbytes &&
           !memcmp(&x.an.lin.to_c[0], &y.an.lin.to_c[0], sizeof(QStep));
}

// a chain's stage kinds: a tensor operand / a scalar one (an APPROX stage has neither)
static bool stage_has_tensor(const QEpStage& s) { return !s.scalar && s.op != QG_EW_APPROX; }
static bool stage_is_scalar(const QEpStage& s) { return s.scalar && s.op != QG_EW_APPROX && s.op != QG_EW_PASS; }
// what a straggler's own execute issues: its kernel and, with a chain that its plain plan does not fuse, the chain's pass
static int straggler_launches(const QGrouped* G, const QPlanGeom& q, uint32_t flags)
{
    return qg_plan_launches(&q) + (G->has_ep && !qg_fuses_epilogue(&q, flags, G->has_ax != 0, false) ? 1 : 0);
}

// every distinct descriptor once, with the geometry it has in the group: in the launch (u_in) the batched analysis' 64 x 64
// geometry, a straggler its plain plan's
static int grouped_distinct(const qgemul_desc* d, int64_t groups, uint32_t flags, const EpView* ev, QGrouped* G, qgemul_info* info)
{
    flags &= ~(uint32_t)(QG_OPT_BATCHED_STACKED | QG_OPT_BATCHED_TREE);   // (a batched plan's switches: a grouped plan plans its members as without them)
    // (the comparison of the one-shot cache: qg_run_key.h)
    for (int64_t g = 0; g < groups; ++g) {
        int64_t u = 0;
        while (u < G->n_uniq && !same_desc(G->ud[u], d[g])) ++u;
        if (u == G->n_uniq) G->ud[G->n_uniq++] = d[g];
        G->m[g].uniq = (int32_t)u;
    }
    G->ug = new (std::nothrow) QPlanGeom[G->n_uniq]();
    G->u_in = new (std::nothrow) uint8_t[G->n_uniq]();
    G->up = new (std::nothrow) qgemul_plan*[G->n_uniq]();
    if (!G->ug || !G->u_in || !G->up) return QG_EINVAL;
    // batch = groups: an eligible member gets the 64 x 64 geometry of qg_mfma_pick_batched
    for (int64_t u = 0; u < G->n_uniq; ++u) {
        const int st = qg_plan_geometry(&G->ud[u], flags, ev, groups, &G->ug[u], nullptr, nullptr);
        if (st != QG_OK) { *info = G->ug[u].info; return st; }
    }
    auto eligible = [&](int64_t u) { return G->ug[u].bd && G->ug[u].pa.K_p >= G->ug[u].cfg.BK; };
    for (int64_t g = 0; g < groups && G->key < 0; ++g)
        if (eligible(G->m[g].uniq)) G->key = G->m[g].uniq;
    for (int64_t u = 0; u < G->n_uniq; ++u)
        // (with a chain the key also holds C's whole format: the chain's analysis depends on it, and to_c alone does not pin it)
        G->u_in[u] = G->key >= 0 && eligible(u) && qg_same_launch_key(G->ug[u], G->ug[G->key]) && (!ev || same_fmt(G->ud[u].c[0], G->ud[G->key].c[0]));
    for (int64_t u = 0; u < G->n_uniq; ++u) {
        if (G->u_in[u]) continue;
        // a straggler runs on its own PLAIN plan
        G->ug[u] = QPlanGeom();
        const int st = qg_plan_geometry(&G->ud[u], flags, ev, 0, &G->ug[u], nullptr, nullptr);
        if (st != QG_OK) { *info = G->ug[u].info; return st; }
    }
    return QG_OK;
}

// layout: the members in the launch back to back, the launch's one trailer and one row-sum array (cur: the bytes so far); true:
// beyond the tile / address range
static bool grouped_launch_layout(QGrouped* G, int64_t cur[3], double* ops)
{
    bool over = false;
    int64_t rows[2] = {0, 0}, tiles = 0;
    for (int64_t g = 0; g < G->groups; ++g) {
        QGrpMember& m = G->m[g];
        const QPlanGeom& q = G->ug[m.uniq];
        *ops += q.info.ops;
        m.in_launch = G->u_in[m.uniq];
        if (!m.in_launch) continue;
        ++G->n_in;
        m.pa = q.pa;
        m.pb = q.pb;
        m.bytes[0] = (int64_t)q.pa.limbs * q.pa.rows_p * q.pa.K_p;
        m.bytes[1] = (int64_t)q.pb.limbs * q.pb.rows_p * q.pb.K_p;
        m.bytes[2] = q.pc.Mp * q.pc.Np * q.pc.cbytes;
        m.row_a = rows[0];
        m.row_b = rows[1];
        for (int w = 0; w < 3; ++w) {
            m.off[w] = cur[w];
            over |= __builtin_add_overflow(cur[w], m.bytes[w], &cur[w]) || cur[w] > (1ll << 60);
        }
        // a chain's tensor operands: the members at the element offsets they have in D (q.pc is D, whole 64 x 64 tiles per member)
        for (int k = 0; G->has_ep && k < q.ept.n; ++k) {
            if (!stage_has_tensor(q.ept.st[k])) continue;
            m.eoff[k] = G->launch_elems * q.ept.st[k].ebytes;
            over |= __builtin_add_overflow(m.eoff[k], q.pc.Mp * q.pc.Np * q.ept.st[k].ebytes, &G->ebytes[k]) || G->ebytes[k] > (1ll << 60);
        }
        G->launch_elems += q.pc.Mp * q.pc.Np;
        rows[0] += q.pa.rows_p;
        rows[1] += q.pb.rows_p;
        tiles += (q.pa.rows_p / q.cfg.TM) * (q.pb.rows_p / q.cfg.TN);
        over |= rows[0] > 0x7fffffffll || rows[1] > 0x7fffffffll || tiles > 0x7fffffffll || q.pa.K_p / q.cfg.BK > 0x7fffffffll;
    }
    G->n_tiles = tiles;
    if (!G->n_in || over) return over;
    const QPlanGeom& k = G->ug[G->key];
    QPackedGeom* sg[2] = {&G->sa, &G->sb};
    for (int w = 0; w < 2; ++w) {
        QPackedGeom& s = *sg[w];
        s = w ? k.pb : k.pa;
        s.rows_p = rows[w];
        s.K_p = 0;   // (every member has its own)
        s.trailer = 0;
        if (s.limbs > 1) { s.trailer = cur[w]; cur[w] += QG_TRAILER_BYTES; }   // ONE plane mask: the OR over every member in the launch
        if (s.offs) {                                                           // ONE row-sum array over the stack's rows
            s.rowsum_off = qg_round_up(cur[w], 256);
            cur[w] = s.rowsum_off + s.rows_p * 8;
        }
    }
    for (int64_t g = 0; g < G->groups; ++g) {
        QGrpMember& m = G->m[g];
        if (!m.in_launch) continue;
        QPackedGeom* mg[2] = {&m.pa, &m.pb};
        for (int w = 0; w < 2; ++w) {
            // trailer and row sums relative to the member's start (both stay positive: they lie behind the planes of ALL members)
            mg[w]->trailer = sg[w]->trailer ? sg[w]->trailer - m.off[w] : 0;
            if (sg[w]->offs) {
                mg[w]->offs = 2;   // adds to row sums its caller has zeroed
                mg[w]->rowsum_off = sg[w]->rowsum_off + (w ? m.row_b : m.row_a) * 8 - m.off[w];
            }
        }
    }
    return false;
}

// the schedule: one record per workgroup (qg_grp.h)
static int grouped_schedule(QGrouped* G)
{
    const QPlanGeom& k = G->ug[G->key];
    QGrpShape* sh = new (std::nothrow) QGrpShape[G->n_in];
    int64_t* order = new (std::nothrow) int64_t[G->n_in];
    G->tiles = new (std::nothrow) QGrpTile[G->n_tiles];
    const bool pass = G->has_ep && !G->fused;   // the chain's pass over the launch's packed C: the member of every C tile
    if (pass) G->tile_member = new (std::nothrow) int32_t[G->n_tiles];
    if (!sh || !order || !G->tiles || (pass && !G->tile_member)) { delete[] sh; delete[] order; return QG_EINVAL; }
    int64_t n = 0;
    for (int64_t g = 0; g < G->groups; ++g) {
        const QGrpMember& m = G->m[g];
        if (!m.in_launch) continue;
        const QPlanGeom& q = G->ug[m.uniq];
        QGrpShape& s = sh[n++];
        s.a_off = m.off[0];
        s.b_off = m.off[1];
        s.c_off = m.off[2] / q.pc.cbytes;
        s.corr = (int64_t)((uint64_t)G->ud[m.uniq].K * (uint64_t)k.pa.bias * (uint64_t)k.pb.bias);
        s.a_blk = (int64_t)q.pa.limbs * q.cfg.TM * q.cfg.BK;
        s.b_blk = (int64_t)q.pb.limbs * q.cfg.TN * q.cfg.BK;
        s.c_tile = (int64_t)q.cfg.TM * q.cfg.TN;
        s.tiles_m = (int32_t)(q.pa.rows_p / q.cfg.TM);
        s.tiles_n = (int32_t)(q.pb.rows_p / q.cfg.TN);
        s.nk = (int32_t)(q.pa.K_p / q.cfg.BK);
        s.row_a = (int32_t)m.row_a;
        s.row_b = (int32_t)m.row_b;
        s.tm = q.cfg.TM;
        s.tn = q.cfg.TN;
        s.member = (int32_t)g;
    }
    // (the alternative order exists in the diagnostic library only: tools/measure_grouped.py)
    const bool member_order = QG_DIAG_ENV("QG_GRP_MEMBER_ORDER");
    qg_grp_schedule(sh, n, member_order ? QG_GRP_MEMBER : QG_GRP_DEALT, order, G->tiles);
    if (pass) qg_grp_tile_members(sh, n, G->tile_member);
    delete[] sh;
    delete[] order;
    return QG_OK;
}

int qg_grouped_geometry(const qgemul_desc* d, int64_t groups, uint32_t flags, QGrouped* G, qgemul_info* info, const EpView* ev, const qgemul_grouped_ep* gep)
{
    if (!d || groups < 1 || groups > 0x7fffffffll) return QG_EINVAL;
    G->groups = groups;
    G->flags = flags;
    G->key = -1;
    G->m = new (std::nothrow) QGrpMember[groups]();
    G->ud = new (std::nothrow) qgemul_desc[groups];
    if (!G->m || !G->ud) return QG_EINVAL;
    G->has_ep = ev ? 1 : 0;
    for (int k = 0; ev && ev->ax && k < QG_MAX_EW; ++k) G->has_ax |= ev->ax[k] != nullptr;
    if (const int st = grouped_distinct(d, groups, flags, ev, G, info); st != QG_OK) return st;
    if (ev) {
        // per-member values belong to scalar stages (the stage kinds depend on the chain alone: any member's table shows them)
        const QEpTable& t = G->ug[0].ept;
        for (int k = 0; gep && k < QG_MAX_EW; ++k) {
            if (!gep->scalar_per_member[k]) continue;
            if (k >= t.n || !stage_is_scalar(t.st[k])) {
                *info = G->ug[0].info;
                info->supported = 0;
                snprintf(info->reason, sizeof info->reason, "grouped chain: scalar_per_member on stage %d, which is no scalar stage", k);
                return QG_EINVAL;
            }
            G->per_member[k] = 1;
        }
        // fused form: what the 32-bit epilogue can carry, on request (the default between the two forms is the pass: DESIGN.md section 9)
        G->fused = G->key >= 0 && G->ug[G->key].ept.bits32 && !G->has_ax && (flags & QG_OPT_FUSED_EPILOGUE) && !(flags & QG_OPT_UNFUSED_EPILOGUE);
    }
    int64_t cur[3] = {0, 0, 0};
    double ops = 0;
    bool over = grouped_launch_layout(G, cur, &ops);
    // ... then the stragglers
    int64_t launches = G->n_in ? (ev && !G->fused ? 2 : 1) : 0;
    for (int64_t g = 0; g < groups && !over; ++g) {
        QGrpMember& m = G->m[g];
        if (m.in_launch) continue;
        const QPlanGeom& q = G->ug[m.uniq];
        for (int w = 0; w < 3; ++w) {
            m.off[w] = qg_round_up(cur[w], 256);
            m.bytes[w] = q.info.packed_bytes[w];
            over |= __builtin_add_overflow(m.off[w], m.bytes[w], &cur[w]) || cur[w] > (1ll << 60);
        }
        for (int k = 0; ev && k < q.ept.n; ++k) {
            if (!stage_has_tensor(q.ept.st[k])) continue;
            m.eoff[k] = qg_round_up(G->ebytes[k], 256);
            over |= __builtin_add_overflow(m.eoff[k], q.pc.Mp * q.pc.Np * q.ept.st[k].ebytes, &G->ebytes[k]) || G->ebytes[k] > (1ll << 60);
        }
        if (!qg_grp_empty(G->ud[m.uniq])) launches += straggler_launches(G, q, flags);
    }
    *info = G->ug[G->key >= 0 ? G->key : G->m[0].uniq].info;
    if (over) {
        info->supported = 0;
        snprintf(info->reason, sizeof info->reason, "grouped plan: more than 2^31 - 1 tiles / packed operands beyond the address range");
        return QG_EINVAL;
    }
    G->launches = launches > 0x7fffffffll ? 0x7fffffff : (int)launches;
    for (int w = 0; w < 3; ++w) info->packed_bytes[w] = cur[w];
    info->ops = ops;
    snprintf(info->reason, sizeof info->reason, "grouped plan: %lld members in one launch (%lld 64x64 tiles), %lld run alone", (long long)G->n_in,
             (long long)G->n_tiles, (long long)(groups - G->n_in));
    if (ev && !G->n_in)
        snprintf(info->reason, sizeof info->reason, "grouped chain: no member eligible, %lld run alone", (long long)groups);
    else if (ev)
        snprintf(info->reason, sizeof info->reason, G->fused ? "grouped chain fused: %lld members in one launch (%lld 64x64 tiles), %lld run alone"
                                                             : "grouped chain pass: %lld members in one launch (%lld 64x64 tiles) + one pass, %lld run alone",
                 (long long)G->n_in, (long long)G->n_tiles, (long long)(groups - G->n_in));
    return G->n_tiles > 0 ? grouped_schedule(G) : QG_OK;
}

void qg_grouped_member_out(const QGrouped* G, int64_t g, qgemul_grouped_member* out)
{
    const QGrpMember& m = G->m[g];
    const QPlanGeom& q = G->ug[m.uniq];
    memset(out, 0, sizeof *out);
    out->in_launch = m.in_launch;
    out->launches = m.in_launch || qg_grp_empty(G->ud[m.uniq]) ? 0 : straggler_launches(G, q, G->flags);
    for (int w = 0; w < 3; ++w) { out->off[w] = m.off[w]; out->bytes[w] = m.bytes[w]; }
    if (m.in_launch) {
        out->tiles_m = q.pa.rows_p / q.cfg.TM;
        out->tiles_n = q.pb.rows_p / q.cfg.TN;
        out->k_tiles = q.pa.K_p / q.cfg.BK;
    }
}
