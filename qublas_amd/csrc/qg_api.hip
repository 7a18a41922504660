// qg_api.hip — the C-ABI of include/qgemul.h: contexts, classification, plans, packing, execution (the one-shot calls: qg_run.hip).
//
// There is deliberately no CPU arithmetic path in this library: without a gfx950 device every
// compute entry point returns QG_ENOGPU.  (The CPU restatement lives in oracle/ and is test
// infrastructure only.)
#include "qg_api_int.h"

static thread_local int g_last_hip = 0;
int qg_last_hip() { return g_last_hip; }
void qg_set_last_hip(int e) { g_last_hip = e; }

struct HostC { void* C; int64_t ld; };
// an element-wise chain as the planner sees it: a real chain (im == nullptr) or the two part chains of a complex one
// a chain that came in through an _epcx entry point and holds a CMUL stage in either part (such a chain is planned in lock step)
static bool view_has_cmul(const EpView* ev)
{
    if (!ev || !ev->cx || !ev->im) return false;
    for (int p = 0; p < 2; ++p)
        for (uint32_t k = 0; k < ev->epc->part[p].n_stages && k < QG_MAX_EW; ++k)
            if (ev->epc->part[p].stage[k].op == QG_EW_CMUL) return true;
    return false;
}   // execute_kernel: store the reference layout directly (kernels that can)

static int pow2_bytes(int storage_bits)
{
    int b = (storage_bits + 7) / 8;
    int c = 1;
    while (c < b) c *= 2;
    return c;
}

static int64_t round_up(int64_t x, int64_t m) { return (x + m - 1) / m * m; }

// ---- composite linear plans: geometry helpers (see QComposite) ----
static int64_t comp_sub_bytes(int limbs, int64_t rows_p, int64_t K_p)
{
    return round_up((int64_t)limbs * rows_p * K_p + (limbs > 1 ? QG_TRAILER_BYTES : 0), 256);
}
// reduction indices of chunk c
static int64_t comp_chunk_len(const QComposite& q, int64_t K, int c) { return c + 1 < q.nc ? q.kc : K - (int64_t)(q.nc - 1) * q.kc; }
// the packed sub-operand (chunk c, group g) of operand `which` (0 A, 1 B): its geometry and its byte offset in the packed operand
static QPackedGeom comp_sub_geom(const QComposite& q, const QPackedGeom& base, int which, int64_t K, int c, int g, int64_t* off)
{
    const int* L = which ? q.lb : q.la;
    const int* L0 = which ? q.lb0 : q.la0;
    const int ng = which ? q.gb : q.ga;
    const int64_t K_p = round_up(comp_chunk_len(q, K, c), base.bk);
    QPackedGeom s = base;
    s.K_p = K_p;
    s.limbs = L[g];
    s.limb0 = L0[g];
    s.trailer = L[g] > 1 ? (int64_t)L[g] * base.rows_p * K_p : 0;
    s.digit6 = 0;
    int64_t o = (int64_t)c * q.chunk_bytes[which];
    for (int h = 0; h < g && h < ng; ++h) o += comp_sub_bytes(L[h], base.rows_p, K_p);
    if (off) *off = o;
    if (base.offs) {   // centred operand: ONE row-sum array behind all sub-operands; the groups that hold digit 0 add their k-chunk to it
        s.offs = L0[g] == 0 ? 2 : 3;
        s.rowsum_off = base.rowsum_off - o;
    }
    return s;
}
// groups of 2-3 limbs, low limbs first
static int comp_split(int L, int* sizes, int* first)
{
    static const int tab[9][3] = {{0, 0, 0}, {1, 0, 0}, {2, 0, 0}, {3, 0, 0}, {2, 2, 0}, {3, 2, 0}, {3, 3, 0}, {3, 2, 2}, {3, 3, 2}};
    if (L < 1 || L > 8) return 0;
    int n = 0, f = 0;
    for (int i = 0; i < 3 && tab[L][i]; ++i) { sizes[n] = tab[L][i]; first[n] = f; f += tab[L][i]; ++n; }
    return n;
}
static bool comp_geometry(int LA, int LB, const qgemul_desc* d, uint32_t flags, QComposite* q, QMfmaCfg* cfg)
{
    memset(q, 0, sizeof *q);
    q->ga = comp_split(LA, q->la, q->la0);
    q->gb = comp_split(LB, q->lb, q->lb0);
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

// composite plans: run `fn` on every (k-chunk, limb group) sub-operand of A or B — its view of the host tensor (the chunk's
// reduction indices), its packed geometry, its byte offset inside the packed operand
template <class F>
static hipError_t comp_for_each_sub(const qgemul_plan* p, int operand, const QOperandGeom& g, F fn)
{
    const QComposite& q = p->comp;
    const int w = operand == QG_OPERAND_A ? 0 : 1;
    const QPackedGeom& base = w ? p->pb : p->pa;
    for (int c = 0; c < q.nc; ++c)
        for (int gi = 0; gi < (w ? q.gb : q.ga); ++gi) {
            int64_t off = 0;
            const QPackedGeom sp = comp_sub_geom(q, base, w, p->desc.K, c, gi, &off);
            QOperandGeom sg = g;
            sg.k0 = (int64_t)c * q.kc;
            sg.K = comp_chunk_len(q, p->desc.K, c);
            if (hipError_t e = fn(sg, sp, off); e != hipSuccess) return e;
        }
    return hipSuccess;
}

// composite plan on a centred operand: its one row-sum array is zeroed before the sub-operands' packs add to it
static hipError_t comp_zero_rowsums(const qgemul_plan* p, int operand, void* packed_dev)
{
    const QPackedGeom& base = operand == QG_OPERAND_A ? p->pa : p->pb;
    if (!p->comp.on || !base.offs) return hipSuccess;
    return hipMemsetAsync((char*)packed_dev + base.rowsum_off, 0, (size_t)base.rows_p * 8, p->ctx->stream);
}

// fill info + geometry for a descriptor; no GPU access
// ev: the element-wise chain (nullptr: none); axt / cmt: receive the pre-resolved tables of APPROX / CMUL stages (nullptr: not wanted)
static int plan_geometry(const qgemul_desc* d, uint32_t flags, const EpView* ev, int64_t batch, QPlanGeom* out, QApproxTable* axt, QCmulStage* cmt)
{
    QAnalysis* const an = &out->an;
    qgemul_info* const info = &out->info;
    QPackedGeom *const pa = &out->pa, *const pb = &out->pb;
    QCGeom* const pc = &out->pc;
    QHostElem *const ha = &out->ha, *const hb = &out->hb, *const hc = &out->hc;
    QComposite& comp = out->comp;
    // batch > 0: the member of a batched plan.  Where k_mfma has a block-diagonal form for it, the tile geometry comes from
    // qg_mfma_pick_batched (the batch's total tile count, the member's padding waste) and out->bd = 1: the packed layouts then belong
    // to the batched plan and may differ from the plain plan of the same descriptor
    out->bd = 0;
    bool bd = false;
    QMfmaCfg plain_cfg = {0, 0, 0, 0};   // what qg_mfma_pick chose for the member alone
    memset(&comp, 0, sizeof comp);
    const qgemul_epilogue* ep = ev ? ev->re : nullptr;
    qg_analyze(d, an);
    memset(info, 0, sizeof *info);
    snprintf(info->reason, sizeof info->reason, "%s", an->reason);
    if (an->status != QG_OK) {
        info->supported = 0;
        return an->status;
    }
    const int parts = d->is_complex ? 2 : 1;
    *ha = qg_host_elem(d->a, d->is_complex);
    *hb = qg_host_elem(d->b, d->is_complex);
    *hc = qg_host_elem(d->c, d->is_complex);
    info->cls = an->cls;
    info->max_bits = an->max_bits;
    info->supported = 1;
    auto sbits = [&](const qfmt* f) {
        int m = 0;
        for (int p = 0; p < parts; ++p) {
            int b = 1 + (int)f[p].I + (int)f[p].F;
            if (b > m) m = b;
        }
        return m;
    };
    info->in_bits[0] = sbits(d->a);
    info->in_bits[1] = sbits(d->b);
    info->host_elem_bytes[0] = ha->size;
    info->host_elem_bytes[1] = hb->size;
    info->host_elem_bytes[2] = hc->size;
    info->host_imag_off[0] = ha->off[1];
    info->host_imag_off[1] = hb->off[1];
    info->host_imag_off[2] = hc->off[1];
    const double mnk = (double)d->M * (double)d->N * (double)d->K;
    info->ops = !d->is_complex ? 2.0 * mnk : (d->cmul == QG_CMUL_TF ? 6.0 * mnk : 8.0 * mnk);

    int LA = 0, LB = 0, kernel = QG_KERNEL_NONE;
    int64_t centreA = 0, centreB = 0;
    bool centred = false;
    QMfmaCfg cfg = {0, 0, 0, 0};
    // RING plans (qg_plan.cpp: ring_plan; qg_mfma_ring.hip): product and every level wrap into one signed format of n <= 32 bits, so
    // the tree is the dot product modulo 2^n.  The operands keep their first min(L, limbs) balanced digits, L = ceil(n / 8) — no
    // centring, no base-64 digits, no plane-mask shortcut —, and ONE launch takes any K: the accumulators may wrap.  Descriptors
    // that are exact anyway keep their exact linear plan, one output column the one-column kernels walk stays with them, and
    // QG_OPT_FORCE_TREE selects today's tree plan (the invariance arm of the tests).
    const bool ring = an->ring_ok && !(flags & QG_OPT_FORCE_TREE);
    if (ring) {
        const int L = qg_ring_digits(an->ring_n);
        LA = qg_limbs_for(d->a[0]) < L ? qg_limbs_for(d->a[0]) : L;
        LB = qg_limbs_for(d->b[0]) < L ? qg_limbs_for(d->b[0]) : L;
        cfg = QMfmaCfg{QG_MFMA_RING, QG_RING_TM, QG_RING_TN, QG_RING_BK};
        kernel = L == 1 ? QG_KERNEL_MFMA_I8 : QG_KERNEL_MFMA_I8_LIMB;
        const int np = qg_ring_products(LA, LB, L);
        snprintf(info->reason, sizeof info->reason, "linear class: wrapping ring mod 2^%d, %d limb product%s", an->ring_n, np, np == 1 ? "" : "s");
    } else if (an->linear_ok && !(flags & QG_OPT_FORCE_TREE)) {
        LA = qg_limbs_for(d->a[0]);
        LB = qg_limbs_for(d->b[0]);
        if (d->is_complex) {  // parts are stacked along the row axis and share one limb count
            const int la2 = qg_limbs_for(d->a[1]), lb2 = qg_limbs_for(d->b[1]);
            if (la2 > LA) LA = la2;
            if (lb2 > LB) LB = lb2;
        }
        // CENTRED operands (qg_plan.h: qg_limbs_centred; QPackedGeom::offs): x - c in balanced limbs where that saves a limb — signed
        // formats of 16 / 24 / 32 bits (3 -> 2, 4 -> 3, 5 -> 4 limbs), unsigned formats (uint8: 2 -> 1) — the centre taken back out
        // with row sums after the dot product.  Real descriptors only (stacked complex parts have different centres).
        if (!d->is_complex && !(flags & QG_OPT_BALANCED_LIMBS)) {
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
        const int mn = LA < LB ? LA : LB;
        cfg = qg_mfma_pick(LA, LB, d->M * parts, d->N * parts, (ep ? QG_OPT_LOCKSTEP_TILES : 0u) | flags);   // (the fused / unfused element-wise chain keeps the kernel it was measured on)
        if (batch > 0 && !d->is_complex && (!ep || !ev->im)) {   // (with a real chain: qgemul_plan_create_batched_epx)
            const QMfmaCfg bc = qg_mfma_pick_batched(LA, LB, batch, cfg);
            if (bc.variant) { plain_cfg = cfg; cfg = bc; bd = true; }
        }
        // (wide plans: the kernels' own epilogues are 64-bit; the composite plan's combine pass is not.  Centred single-limb pairs: the
        //  single-limb kernels' epilogue is 32-bit, sum a b of two uint8 operands is not: raw int32 slab + combine pass)
        // (... except where its image in C fits 31 bits and no element-wise chain follows: the single-limb kernels' epilogues then restore
        //  the sum in 64 bits themselves)
        const QStep& tc = an->lin.to_c[0];
        const bool pp_centred = cfg.variant && !ep && sbits(d->c) <= 31 && (tc.identity || (tc.d >= 0 && tc.W <= 30));   // (every single-limb kernel has the 64-bit branch)
        if (cfg.variant && (int64_t)mn * d->K <= (1ll << 17) - 1 && !an->wide && !an->generic_only && !(centred && LA == 1 && LB == 1 && !pp_centred))
            kernel = d->is_complex ? QG_KERNEL_MFMA_CPLX : ((LA == 1 && LB == 1) ? QG_KERNEL_MFMA_I8 : QG_KERNEL_MFMA_I8_LIMB);
        // (one output column whose tree the one-column kernels can walk: those stream A once at HBM rate; a composite plan would read
        // it once per limb group and write slabs — the batched Qreduce of 32-bit words with exact level types stays there)
        else if (!d->is_complex && !(d->N == 1 && (an->gemv_ok || an->gemv_wide_ok) && !(flags & QG_OPT_GENERIC_TREE)) &&
                 comp_geometry(LA, LB, d, flags, &comp, &cfg)) {
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
        if (bd) {
            // the block-diagonal form takes what ONE launch of a lock-step kernel with its own conversion serves: no composite plan, no
            // raw-dot-product detour (wide_epilogue below).  A member without it runs on the plain plan's own geometry
            const QStep& q = an->lin.to_c[0];
            const bool raw_pass = kernel == QG_KERNEL_MFMA_I8 && !q.identity && (q.W > 30 || (q.d < 0 && an->dot_bits - q.d > 31));
            if (comp.on || raw_pass || (kernel != QG_KERNEL_MFMA_I8 && kernel != QG_KERNEL_MFMA_I8_LIMB)) {
                bd = false;
                if (!comp.on) cfg = plain_cfg;
            }
        }
    }
    pc->M = d->M;
    pc->N = d->N;
    pc->parts = parts;
    pc->cbytes = pow2_bytes(sbits(d->c));
    // (a multi-word value in the band the reference mis-compares comes out as its low WORD — int32_t / int64_t — whatever C's
    // format says: such plans keep the host element's width in packed C)
    if (an->band && pc->cbytes < (hc->sb[0] > hc->sb[1] ? hc->sb[0] : hc->sb[1])) pc->cbytes = hc->sb[0] > hc->sb[1] ? hc->sb[0] : hc->sb[1];
    pc->ldc = d->M;
    pc->elem_bytes = hc->size;
    for (int p = 0; p < 2; ++p) { pc->off[p] = hc->off[p]; pc->sb[p] = hc->sb[p]; }
    // Three-digit Karatsuba (qg_mfma_k6.hip): both operands of 17 / 18 value+sign bits (3 limbs each; operands of 2 limbs take 4 or
    // 6 schoolbook products already), real, not centred, no element-wise chain, a shape the two-group 3 x 3 kernel takes, C in a 4-
    // or 8-byte container, and ONE product per int32 accumulator exact: K * 126^2 < 2^31.  The planes then hold the unsigned base-64
    // digits of x + bias on 96-row tiles of A; QG_OPT_SCHOOLBOOK_LIMBS / QG_OPT_LOCKSTEP_TILES keep the balanced limbs.
    bool k6 = false, ppl33 = false;
    {
        static const bool no_kara3 = QG_DIAG_ENV("QG_NO_KARA3");   // A/B switch
        auto ubits = [](qfmt f) { return (int)f.I + (int)f.F + (f.S ? 1 : 0); };
        const int cb = pow2_bytes(sbits(d->c));
        // (what k_mfma_ppl's 3 x 3 body takes: qg_mfma_ppl_applies)
        ppl33 = kernel == QG_KERNEL_MFMA_I8_LIMB && !comp.on && !d->is_complex && !ep && LA == 3 && LB == 3 && cfg.variant == QG_MFMA_PPL && (cb == 4 || cb == 8);
        k6 = ppl33 && !no_kara3 && !(flags & QG_OPT_SCHOOLBOOK_LIMBS) && !centred && !an->band && ubits(d->a[0]) >= 13 && ubits(d->a[0]) <= 18 &&
             ubits(d->b[0]) >= 13 && ubits(d->b[0]) <= 18 && d->K * (int64_t)(126 * 126) < (1ll << 31);
        if (k6) cfg = QMfmaCfg{QG_MFMA_K6, QG_K6_TM, QG_K6_TN, QG_K6_BK};
    }
    if (kernel != QG_KERNEL_NONE) {
        *pa = QPackedGeom{round_up(d->M, cfg.TM), round_up(d->K, cfg.BK), 1, LA, cfg.TM, cfg.BK};
        *pb = QPackedGeom{round_up(d->N, cfg.TN), round_up(d->K, cfg.BK), 1, LB, cfg.TN, cfg.BK};
        if (comp.on) {   // pa / pb: the first sub-operand (group 0 of chunk 0); the others through comp_sub_geom
            pa->K_p = pb->K_p = round_up(comp.kc, cfg.BK);
            pa->limbs = comp.la[0];
            pb->limbs = comp.lb[0];
        }
        pc->Mp = pa->rows_p;
        pc->Np = pb->rows_p;
        pc->tm = cfg.TM;
        pc->tn = cfg.TN;
        if (k6) {   // packed C keeps the 128 x 128 tiles of the other limb plans: callers that size or move packed C see no change
            pc->Mp = round_up(d->M, 128);
            pc->tm = 128;
        }
        if (d->is_complex) {
            // the MFMA kernel writes the raw 2Mh x 2Nh dot products into the plan's workspace; the combine
            // pass writes the packed complex C row-major [2][M][N]
            pc->Mp = d->M;
            pc->Np = d->N;
            pc->tm = pc->tn = 0;
        }
    } else {
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
        // the 32-bit tree kernels walk a perfect binary tree: their operands are zero-padded along K to 2^n_levels leaves
        // (a node whose right child is a zero leaf / zero subtree is the reference's converting copy of an odd leftover)
        const bool t64 = kernel == QG_KERNEL_TREE_I64 && an->tree64_ok && fast;   // the 2x2-per-lane 64-bit kernel, not the general one
        const int64_t Kt = (kernel == QG_KERNEL_TREE_I32 || kernel == QG_KERNEL_TREE_CPLX_I32 || kernel == QG_KERNEL_GEMV_I32 || kernel == QG_KERNEL_GEMV_I64 || t64)
                               ? ((int64_t)1 << an->tree.n_levels_k) : d->K;   // (n_levels_k: at least 5 levels, qg_plan.h)
        *pa = QPackedGeom{d->M, Kt, info->in_bits[0] <= 32 ? 4 : 8, 0, 0, 0};
        *pb = QPackedGeom{d->N, Kt, info->in_bits[1] <= 32 ? 4 : 8, 0, 0, 0};
        pc->Mp = d->M;
        pc->Np = d->N;
        pc->tm = pc->tn = 0;
    }
    out->bd = bd ? 1 : 0;
    info->kernel = kernel;
    info->limbs[0] = LA;
    info->limbs[1] = LB;
    info->packed_bytes[0] = (int64_t)parts * (pa->limbs ? pa->limbs : 1) * pa->rows_p * pa->K_p * pa->cbytes;
    info->packed_bytes[1] = (int64_t)parts * (pb->limbs ? pb->limbs : 1) * pb->rows_p * pb->K_p * pb->cbytes;
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
            const int64_t Kl = round_up(comp_chunk_len(comp, d->K, comp.nc - 1), base.bk);
            for (int g = 0; g < ng; ++g) { full += comp_sub_bytes(L[g], base.rows_p, base.K_p); last += comp_sub_bytes(L[g], base.rows_p, Kl); }
            comp.chunk_bytes[w] = full;
            info->packed_bytes[w] = (int64_t)(comp.nc - 1) * full + last;
        }
        pa->trailer = pb->trailer = 0;   // (per sub-operand: comp_sub_geom)
        if ((int64_t)comp.ga * comp.gb * pa->rows_p * pb->rows_p * comp.slab_bytes > (64ll << 30)) {
            info->supported = 0;
            snprintf(info->reason, sizeof info->reason, "composite linear plan: the slabs of raw dot products would exceed 64 GiB");
            return QG_EUNSUPPORTED;
        }
    }
    if (centred && kernel != QG_KERNEL_NONE) {   // both operands carry row sums (an uncentred partner: bias 0), behind everything else
        pa->offs = pb->offs = 1;
        pa->bias = -centreA;
        pb->bias = -centreB;
        pa->rowsum_off = round_up(info->packed_bytes[0], 256);
        pb->rowsum_off = round_up(info->packed_bytes[1], 256);
        info->packed_bytes[0] = pa->rowsum_off + pa->rows_p * 8;
        info->packed_bytes[1] = pb->rowsum_off + pb->rows_p * 8;
    }
    // Karatsuba (qg_mfma.hip, KARA): two-limb operands whose biased values fit 12 bits are stored as two unsigned base-64
    // digits each, and the product takes 3 MFMAs per k-step instead of 4
    if (!comp.on && !centred) {
        static const bool no_kara = QG_DIAG_ENV("QG_NO_KARA");   // A/B switch
        auto ubits = [](qfmt f) { return (int)f.I + (int)f.F + (f.S ? 1 : 0); };
        // (problems small enough for the 64x64 tiles are latency-bound: measured 9.5 vs 8.9 us at 1024^3, schoolbook kept there)
        if (!no_kara && !d->is_complex && LA == 2 && LB == 2 && (kernel == QG_KERNEL_MFMA_I8_LIMB) && (cfg.variant == QG_MFMA_LIMB_128 || cfg.variant == QG_MFMA_PPL) && ubits(d->a[0]) <= 12 &&
            ubits(d->b[0]) <= 12 && d->K * (int64_t)(126 * 126) < (1ll << 31)) {
            cfg.variant = QG_MFMA_LIMB_128;   // three products on the lock-step Karatsuba kernel (same tiles and k-tiles as QG_MFMA_PPL)
            for (QPackedGeom* g : {pa, pb}) {
                const qfmt f = g == pa ? d->a[0] : d->b[0];
                g->digit6 = 1;
                g->bias = f.S ? ((int64_t)1 << ((int)f.I + (int)f.F)) : 0;
                g->rowsum_off = g->trailer + QG_TRAILER_BYTES;
            }
            info->packed_bytes[0] += pa->rows_p * 8;
            info->packed_bytes[1] += pb->rows_p * 8;
        }
    }
    if (k6) {
        for (QPackedGeom* g : {pa, pb}) {
            const qfmt f = g == pa ? d->a[0] : d->b[0];
            g->digit6 = 1;
            g->bias = f.S ? ((int64_t)1 << ((int)f.I + (int)f.F)) : 0;
            g->rowsum_off = g->trailer + QG_TRAILER_BYTES;
        }
        info->packed_bytes[0] += pa->rows_p * 8;
        info->packed_bytes[1] += pb->rows_p * 8;
        snprintf(info->reason, sizeof info->reason, "linear class: three base-64 digits per operand, six products (two-group kernel, 96x128 tiles)");
    } else if (ppl33) {
        snprintf(info->reason, sizeof info->reason, "linear class: balanced base-256 limbs, nine products (two-group kernel, 128x128 tiles)");
    }
    info->packed_bytes[2] = (int64_t)parts * pc->Mp * pc->Np * pc->cbytes;
    out->LA = LA;
    out->LB = LB;
    out->cfg = cfg;
    out->variant = cfg.variant;
    out->pc_c = *pc;
    if (ep && an->band) {
        info->supported = 0;
        snprintf(info->reason, sizeof info->reason, "element-wise chain after a plan whose C can leave its format (multi-word comparison artefact of the reference)");
        return QG_EUNSUPPORTED;
    }
    if (ep) {
        // D replaces C as the stored result: same index space, D's container and host element
        if ((d->is_complex != 0) != (ev->im != nullptr)) {
            info->supported = 0;
            snprintf(info->reason, sizeof info->reason, d->is_complex ? "complex GEMM: the chain is a qgemul_epilogue_cplx" : "real GEMM: the chain is a qgemul_epilogue");
            return QG_EINVAL;
        }
        QEpTable* t[2] = {&out->ept, &out->ept_im};
        qfmt df[2] = {ep->d, ep->d};
        const bool lockstep = view_has_cmul(ev);   // a CMUL stage needs both running values: the part chains are planned together
        if (ev->cx && !lockstep)
            for (int k = 0; k < QG_MAX_EW; ++k)
                if (ev->cx[k]) {
                    info->supported = 0;
                    snprintf(info->reason, sizeof info->reason, "a CMUL record for a stage that is no CMUL stage");
                    return QG_EINVAL;
                }
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
            if (st != QG_OK) {
                info->supported = 0;
                snprintf(info->reason, sizeof info->reason, "%s", why);
                return st;
            }
            if (ep_bits > info->max_bits) info->max_bits = ep_bits;
            df[part] = e->d;
            if (!d->is_complex)
                for (uint32_t k = 0; k < e->n_stages; ++k)
                    if (e->stage[k].op == QG_EW_PASS) {
                        info->supported = 0;
                        snprintf(info->reason, sizeof info->reason, "QG_EW_PASS: complex chains only");
                        return QG_EINVAL;
                    }
        }
        if (d->is_complex) {
            // the two chains describe the same operators: same length; a tensor operand is one packed buffer in one container;
            // a real operand has no imaginary half to read
            if (ev->im->n_stages != ep->n_stages) {
                info->supported = 0;
                snprintf(info->reason, sizeof info->reason, "complex chain: the part chains differ in length");
                return QG_EINVAL;
            }
            for (int k = 0; k < t[0]->n; ++k) {
                QEpStage &a = t[0]->st[k], &b = t[1]->st[k];
                const bool ta = a.op != QG_EW_PASS && !a.scalar, tb = b.op != QG_EW_PASS && !b.scalar;
                if (ev->e_cplx[k] && ta != tb) {
                    info->supported = 0;
                    snprintf(info->reason, sizeof info->reason, "complex chain: a complex tensor operand feeds both parts");
                    return QG_EINVAL;
                }
                if (!ev->e_cplx[k] && ta && tb && !same_fmt(ep->stage[k].e, ev->im->stage[k].e)) {
                    info->supported = 0;
                    snprintf(info->reason, sizeof info->reason, "complex chain: a real tensor operand has one format");
                    return QG_EINVAL;
                }
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
    }
    return QG_OK;
}

// Where the chain runs (measurements: profiles/r01v_eltwise.jsonl, chain = scale + bias into C's own type):
//   3x3-limb kernel, 4096^3: plain 0.458 ms, chain fused into the kernel's epilogue 0.473, chain as a pass 0.490
//   single-limb 256^2-tile kernel, 8192^2 x 4096: plain 0.280, fused 0.503, pass 0.436  (the fused epilogue spills:
//   128 accumulator registers stay live; and with one workgroup per CU the matrix cores idle meanwhile)
// so the default fuses on the limb kernel only, and only chains the planner has bounded by 32-bit arithmetic (a 64-bit
// chain inside the kernel was measured slower than the pass on every kernel).  Everything else runs as ONE linear,
// HBM-bound pass over the stored C (all stages and the final conversion in that pass, 5-6 TB/s).
// The single-limb MFMA kernels keep the dot product in int32 and run their epilogue in 32 bits.  An exact LEFT shift into a C
// with finer fracBits can leave 32 bits before the overflow handling sees the value (found by tests/extended_fuzz.py:
// int<10,-3> operands into Qu<5,7>, shift by 13).  Those descriptors store the raw dot products and convert them in the
// 64-bit linear pass instead, which keeps the hot kernels' epilogue as it is.
static bool wide_epilogue(const QPlanGeom* p)
{
    if (p->comp.on || p->variant == QG_MFMA_RING) return false;   // (the combine pass / the ring kernel's epilogue convert in 64-bit arithmetic anyway)
    const QStep& q = p->an.lin.to_c[0];
    // ... and a C format beyond 31 value bits does not fit the 32-bit epilogue's clamp bounds at all (second find of the
    // extended fuzz runs: int<7,-2> x int<7,-1> into Qu<24,9>)
    return p->info.kernel == QG_KERNEL_MFMA_I8 && !q.identity && (q.W > 30 || (q.d < 0 && p->an.dot_bits - q.d > 31));
}

// centred operands (QPackedGeom::offs): the limb kernels' epilogues take the centres back out before the one round + overflow
static void centre_args(const qgemul_plan* p, QMfmaArgs& a, const void* packedA, const void* packedB)
{
    if (!p->pa.offs || p->comp.on) return;
    a.rsA = (const int64_t*)((const char*)packedA + p->pa.rowsum_off);
    a.rsB = (const int64_t*)((const char*)packedB + p->pb.rowsum_off);
    a.biasA = p->pa.bias;
    a.biasB = p->pb.bias;
    a.corr = (int64_t)((uint64_t)p->desc.K * (uint64_t)p->pa.bias * (uint64_t)p->pb.bias);
}

// plane mask of a packed multi-limb operand (QPackedGeom::trailer); nullptr: all planes
static const uint32_t* plane_mask(const void* packed, const QPackedGeom& g)
{
    return g.trailer ? (const uint32_t*)((const char*)packed + g.trailer) : nullptr;
}

// what every MFMA launch is given: operands of the geometries ga / gb, the result and its container, the kernel
static QMfmaArgs mfma_args(const QPackedGeom& ga, const QPackedGeom& gb, int variant, const void* A, const void* B, void* C, int cbytes)
{
    QMfmaArgs a;
    memset(&a, 0, sizeof a);
    a.A = (const int8_t*)A;
    a.B = (const int8_t*)B;
    a.C = C;
    a.Mp = ga.rows_p;
    a.Np = gb.rows_p;
    a.Kp = ga.K_p;
    a.cbytes = cbytes;
    a.variant = variant;
    a.maskA = plane_mask(A, ga);
    a.maskB = plane_mask(B, gb);
    return a;
}
// ... of a plan's own operands, with the one conversion into C's format and the centres of centred operands
static QMfmaArgs mfma_args(const qgemul_plan* p, const void* A, const void* B, void* C, int cbytes)
{
    QMfmaArgs a = mfma_args(p->pa, p->pb, p->variant, A, B, C, cbytes);
    a.to_c = p->an.lin.to_c[0];
    centre_args(p, a, A, B);
    return a;
}

#ifdef QG_DIAG
static uint32_t* g_diag_stamps = nullptr;   // device buffer for in-kernel clock stamps (diagnostic build only)
extern "C" void qgemul_diag_set_stamps(void* dev) { g_diag_stamps = (uint32_t*)dev; }
#endif

static bool fuses_epilogue(const QPlanGeom* p, uint32_t flags, bool has_ax, bool has_cmul)
{
    if (has_ax) return false;   // (an APPROX stage: always the pass of qg_approx.hip)
    if (has_cmul) return false; // (a CMUL stage: always the pass of qg_eltwise_cplx.hip)
    if (wide_epilogue(p) || p->comp.on || p->variant == QG_MFMA_RING) return false;
    if (flags & QG_OPT_UNFUSED_EPILOGUE) return false;
    if (!p->ept.bits32) return false;
    if (p->info.kernel == QG_KERNEL_MFMA_I8_LIMB && p->LA == 3 && p->LB == 3) return true;
    return p->info.kernel == QG_KERNEL_MFMA_I8 && (flags & QG_OPT_FUSED_EPILOGUE);
}
static bool fuses_epilogue(const qgemul_plan* p) { return fuses_epilogue(p, p->flags, p->has_ax, p->has_cmul); }

extern "C" {

uint32_t qgemul_abi_version(void) { return QGEMUL_ABI_VERSION; }
int qgemul_last_hip_error(void) { return qg_last_hip(); }

const char* qgemul_strerror(int st)
{
    switch (st) {
    case QG_OK: return "ok";
    case QG_EINVAL: return "invalid descriptor or argument";
    case QG_EUNSUPPORTED: return "descriptor outside the engine's supported range";
    case QG_EHIP: return "HIP runtime error";
    case QG_ERCCL: return "RCCL error";
    case QG_ERANGE: return "input raw value outside its declared format";
    case QG_ENOGPU: return "no gfx950 device: the engine has no CPU fallback";
    default: return "unknown status";
    }
}

int qgemul_classify(const qgemul_desc* d, uint32_t opt_flags, qgemul_info* out) { return qgemul_classify_ep(d, nullptr, opt_flags, out); }

int classify_view(const qgemul_desc* d, const EpView* ev, uint32_t opt_flags, qgemul_info* out)
{
    if (!d || !out) return QG_EINVAL;
    QPlanGeom* g = new (std::nothrow) QPlanGeom();
    if (!g) return QG_EINVAL;
    const int st = plan_geometry(d, opt_flags, ev, 0, g, nullptr, nullptr);
    *out = g->info;
    delete g;
    return st;
}

int qgemul_classify_ep(const qgemul_desc* d, const qgemul_epilogue* ep, uint32_t opt_flags, qgemul_info* out)
{
    const EpView v = {ep, nullptr, nullptr};
    return classify_view(d, ep ? &v : nullptr, opt_flags, out);
}

int qgemul_classify_epx(const qgemul_desc* d, const qgemul_epilogue* ep, const qgemul_approx* const ax[QG_MAX_EW], uint32_t opt_flags, qgemul_info* out)
{
    if (!ep || !ax) return QG_EINVAL;
    const EpView v = {ep, nullptr, nullptr, ax};
    return classify_view(d, &v, opt_flags, out);
}

int qgemul_approx_plan_form(const qgemul_desc* d, const qgemul_epilogue* ep, const qgemul_approx* const ax[QG_MAX_EW], qgemul_approx_form* out)
{
    if (!d || !ep || !ax || !out) return QG_EINVAL;
    memset(out, 0, sizeof *out);
    if (d->is_complex) return QG_EINVAL;
    QApproxTable* axt = new (std::nothrow) QApproxTable[QG_MAX_EW];
    if (!axt) return QG_EINVAL;
    QEpTable t;
    int bits = 0;
    const int st = qg_analyze_epx(d->c[0], ep, ax, &t, axt, &bits, nullptr, 0);
    if (st == QG_OK) {
        out->bits32 = t.bits32;
        out->max_bits = bits;
        for (int k = 0; k < QG_MAX_EW; ++k) {
            const bool on = k < t.n && t.st[k].op == QG_EW_APPROX;
            out->uniform[k] = on ? axt[k].uniform : -1;
            for (int g = 0; on && g < QG_MAX_SEG; ++g) out->threshold[k][g] = axt[k].thr[g];
        }
    }
    delete[] axt;
    return st;
}

size_t qgemul_sizeof(int which)
{
    switch (which) {
    case QG_SIZEOF_QFMT: return sizeof(qfmt);
    case QG_SIZEOF_DESC: return sizeof(qgemul_desc);
    case QG_SIZEOF_OPTS: return sizeof(qgemul_opts);
    case QG_SIZEOF_INFO: return sizeof(qgemul_info);
    case QG_SIZEOF_EW_STAGE: return sizeof(qgemul_ew_stage);
    case QG_SIZEOF_EPILOGUE: return sizeof(qgemul_epilogue);
    case QG_SIZEOF_EP_ARGS: return sizeof(qgemul_ep_args);
    case QG_SIZEOF_EPILOGUE_CPLX: return sizeof(qgemul_epilogue_cplx);
    case QG_SIZEOF_APPROX_SEG: return sizeof(qgemul_approx_seg);
    case QG_SIZEOF_APPROX: return sizeof(qgemul_approx);
    case QG_SIZEOF_CMUL: return sizeof(qgemul_cmul);
    case QG_SIZEOF_GROUPED_MEMBER: return sizeof(qgemul_grouped_member);
    default: return 0;
    }
}

int qgemul_classify_epc(const qgemul_desc* d, const qgemul_epilogue_cplx* ep, uint32_t opt_flags, qgemul_info* out)
{
    if (!ep) return QG_EINVAL;
    const EpView v = {&ep->part[0], &ep->part[1], ep->e_complex};
    return classify_view(d, &v, opt_flags, out);
}

int qgemul_classify_epcx(const qgemul_desc* d, const qgemul_epilogue_cplx* ep, const qgemul_cmul* const cx[QG_MAX_EW], uint32_t opt_flags, qgemul_info* out)
{
    if (!ep || !cx) return QG_EINVAL;
    const EpView v = {&ep->part[0], &ep->part[1], ep->e_complex, nullptr, ep, cx};
    return classify_view(d, &v, opt_flags, out);
}

int qgemul_cmul_plan_form(const qgemul_desc* d, const qgemul_epilogue_cplx* ep, const qgemul_cmul* const cx[QG_MAX_EW], qgemul_cmul_form* out)
{
    if (!d || !ep || !cx || !out) return QG_EINVAL;
    memset(out, 0, sizeof *out);
    if (!d->is_complex) return QG_EINVAL;
    const EpView v = {&ep->part[0], &ep->part[1], ep->e_complex, nullptr, ep, cx};
    if (!view_has_cmul(&v)) {
        for (int k = 0; k < QG_MAX_EW; ++k)
            if (cx[k]) return QG_EINVAL;
        return QG_OK;
    }
    QEpTable t[2];
    int bits = 0;
    const int st = qg_analyze_epcx(d->c, ep, cx, t, nullptr, &bits, nullptr, 0);
    if (st == QG_OK) {
        out->has_cmul = 1;
        out->bits32 = t[0].bits32;
        out->max_bits = bits;
    }
    return st;
}

int qgemul_ctx_create(int device, qgemul_ctx** out)
{
    if (!out) return QG_EINVAL;
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess || n <= 0) return QG_ENOGPU;
    if (device < 0) QG_HIP(hipGetDevice(&device));
    if (device >= n) return QG_EINVAL;
    DeviceScope scope(device);   // the caller's current device is restored on return
    QG_HIP(scope.err);
    hipDeviceProp_t prop;
    QG_HIP(hipGetDeviceProperties(&prop, device));
    if (strncmp(prop.gcnArchName, "gfx950", 6) != 0) return QG_ENOGPU; // kernels exist for gfx950 only
    qgemul_ctx* c = (qgemul_ctx*)calloc(1, sizeof *c);
    if (!c) return QG_EINVAL;
    c->device = device;
    if (hipStreamCreateWithFlags(&c->stream, hipStreamNonBlocking) != hipSuccess) { free(c); return QG_EHIP; }
    if (hipMalloc((void**)&c->flag_dev, 64) != hipSuccess) { hipStreamDestroy(c->stream); free(c); return QG_EHIP; }
    hipMemsetAsync(c->flag_dev, 0, 64, c->stream);
    *out = c;
    return QG_OK;
}

void qgemul_ctx_destroy(qgemul_ctx* c)
{
    if (!c) return;
    DeviceScope scope(c->device);
    hipStreamSynchronize(c->stream);
    hipFree(c->flag_dev);
    hipStreamDestroy(c->stream);
    free(c);
}

int qgemul_ctx_sync(qgemul_ctx* c)
{
    if (!c) return QG_EINVAL;
    QG_ON_DEVICE(c);
    QG_HIP(hipStreamSynchronize(c->stream));
    return QG_OK;
}

void* qgemul_ctx_stream(qgemul_ctx* c) { return c ? (void*)c->stream : nullptr; }
int qgemul_ctx_device(const qgemul_ctx* c) { return c ? c->device : -1; }

int qgemul_dev_alloc(qgemul_ctx* c, size_t bytes, void** out)
{
    if (!c || !out) return QG_EINVAL;
    QG_ON_DEVICE(c);
    QG_HIP(hipMalloc(out, bytes ? bytes : 16));
    return QG_OK;
}
int qgemul_dev_free(qgemul_ctx* c, void* p)
{
    if (!c) return QG_EINVAL;
    QG_ON_DEVICE(c);
    QG_HIP(hipStreamSynchronize(c->stream));
    QG_HIP(hipFree(p));
    return QG_OK;
}
int qgemul_memcpy_h2d(qgemul_ctx* c, void* dst, const void* src, size_t bytes)
{
    if (!c) return QG_EINVAL;
    if (!bytes) return QG_OK;
    QG_ON_DEVICE(c);
    QG_HIP(hipMemcpyAsync(dst, src, bytes, hipMemcpyHostToDevice, c->stream));
    QG_HIP(hipStreamSynchronize(c->stream));
    return QG_OK;
}
int qgemul_memcpy_d2h(qgemul_ctx* c, void* dst, const void* src, size_t bytes)
{
    if (!c) return QG_EINVAL;
    if (!bytes) return QG_OK;
    QG_ON_DEVICE(c);
    QG_HIP(hipMemcpyAsync(dst, src, bytes, hipMemcpyDeviceToHost, c->stream));
    QG_HIP(hipStreamSynchronize(c->stream));
    return QG_OK;
}

int qgemul_plan_create(qgemul_ctx* c, const qgemul_desc* d, uint32_t opt_flags, qgemul_plan** out)
{
    return qgemul_plan_create_ep(c, d, nullptr, opt_flags, out);
}

int qgemul_plan_create_ep(qgemul_ctx* c, const qgemul_desc* d, const qgemul_epilogue* ep, uint32_t opt_flags, qgemul_plan** out)
{
    const EpView v = {ep, nullptr, nullptr};
    return plan_create_view(c, d, ep ? &v : nullptr, opt_flags, out);
}

int qgemul_plan_create_epx(qgemul_ctx* c, const qgemul_desc* d, const qgemul_epilogue* ep, const qgemul_approx* const ax[QG_MAX_EW], uint32_t opt_flags,
                           qgemul_plan** out)
{
    if (!ep || !ax) return QG_EINVAL;
    const EpView v = {ep, nullptr, nullptr, ax};
    return plan_create_view(c, d, &v, opt_flags, out);
}

int qgemul_plan_approx_uniform(const qgemul_plan* p) { return p && p->has_ax ? p->ax_uniform : -1; }

int qgemul_plan_create_epc(qgemul_ctx* c, const qgemul_desc* d, const qgemul_epilogue_cplx* ep, uint32_t opt_flags, qgemul_plan** out)
{
    if (!ep) return QG_EINVAL;
    const EpView v = {&ep->part[0], &ep->part[1], ep->e_complex};
    return plan_create_view(c, d, &v, opt_flags, out);
}

int qgemul_plan_create_epcx(qgemul_ctx* c, const qgemul_desc* d, const qgemul_epilogue_cplx* ep, const qgemul_cmul* const cx[QG_MAX_EW],
                            uint32_t opt_flags, qgemul_plan** out)
{
    if (!ep || !cx) return QG_EINVAL;
    const EpView v = {&ep->part[0], &ep->part[1], ep->e_complex, nullptr, ep, cx};
    return plan_create_view(c, d, &v, opt_flags, out);
}

int plan_create_view(qgemul_ctx* c, const qgemul_desc* d, const EpView* ev, uint32_t opt_flags, qgemul_plan** out, int64_t batch)   // batch > 0: the member of a batched plan
{
    if (!c || !d || !out) return QG_EINVAL;
    qgemul_plan* p = new (std::nothrow) qgemul_plan;
    if (!p) return QG_EINVAL;
    memset(p, 0, sizeof *p);
    p->ctx = c;
    p->desc = *d;
    p->flags = opt_flags;
    if (ev) {
        p->has_ep = 1;
        p->ep = *ev->re;
        if (ev->im) {
            p->ep_cplx = 1;
            p->ep_im = *ev->im;
            memcpy(p->e_cplx, ev->e_cplx, sizeof p->e_cplx);
        }
        for (int k = 0; ev->ax && k < QG_MAX_EW; ++k) p->has_ax |= ev->ax[k] != nullptr;
        p->has_cmul = view_has_cmul(ev) ? 1 : 0;
        for (int k = 0; p->has_cmul && k < QG_MAX_EW; ++k)
            if (ev->cx[k]) p->cx[k] = *ev->cx[k];
    }
    QCmulStage cmt[QG_MAX_EW];
    QApproxTable* axt = p->has_ax ? new (std::nothrow) QApproxTable[QG_MAX_EW] : nullptr;
    if (p->has_ax && !axt) { delete p; return QG_EINVAL; }
    struct AxtGuard { QApproxTable* t; ~AxtGuard() { delete[] t; } } axt_guard = {axt};
    int st = plan_geometry(d, opt_flags, ev, batch, p, axt, p->has_cmul ? cmt : nullptr);
    if (st != QG_OK) { delete p; return st; }
    p->tc = qg_tree_choice(&p->an, d, opt_flags, true);
    // from here on the plan may own device memory: every failure leaves through qgemul_plan_destroy, which frees whatever there is
    const auto fail = [p] { qgemul_plan_destroy(p); return QG_EHIP; };
    DeviceScope scope(c->device);
    if (scope.err != hipSuccess || hipMalloc((void**)&p->dev_table, sizeof(QTreeTable)) != hipSuccess) return fail();
    if (hipMemcpyAsync(p->dev_table, &p->an.tree, sizeof(QTreeTable), hipMemcpyHostToDevice, c->stream) != hipSuccess ||
        hipStreamSynchronize(c->stream) != hipSuccess)
        return fail();
    if (p->info.kernel == QG_KERNEL_MFMA_CPLX) {
        const size_t ws = (size_t)(2 * p->pa.rows_p) * (size_t)(2 * p->pb.rows_p) * sizeof(int64_t);
        if (hipMalloc((void**)&p->workspace, ws) != hipSuccess) return fail();
    }
    if (wide_epilogue(p) && hipMalloc((void**)&p->wide_ws, (size_t)(p->pc_c.Mp * p->pc_c.Np) * sizeof(int32_t)) != hipSuccess) return fail();
    if (p->comp.on) {
        const size_t n = (size_t)p->pa.rows_p * (size_t)p->pb.rows_p;
        const size_t sl = n * (size_t)(p->comp.ga * p->comp.gb) * (size_t)p->comp.slab_bytes;
        const size_t ac = p->comp.nc > 1 ? n * (p->comp.wide ? 16 : 8) : 0;
        if (hipMalloc(&p->comp_slabs, sl ? sl : 16) != hipSuccess || (ac && hipMalloc(&p->comp_acc, ac) != hipSuccess)) return fail();
    }
    if (p->has_ep && !fuses_epilogue(p)) {
        // the tree kernels store C; the chain then runs as a pass over it
        const size_t cb = (size_t)(p->pc_c.parts * p->pc_c.Mp * p->pc_c.Np) * (size_t)p->pc_c.cbytes;
        if (hipMalloc(&p->cwork, cb ? cb : 16) != hipSuccess) return fail();
    }
    if (p->has_ax) {
        // the plan's copy of the tables, pre-resolved: one device buffer per APPROX stage
        p->ax_uniform = 1;
        bool ok = true;
        for (int k = 0; k < p->ept.n && ok; ++k) {
            if (p->ept.st[k].op != QG_EW_APPROX) continue;
            p->ax_uniform &= axt[k].uniform;
            ok = hipMalloc((void**)&p->ax_dev[k], sizeof(QApproxTable)) == hipSuccess &&
                 hipMemcpyAsync(p->ax_dev[k], &axt[k], sizeof(QApproxTable), hipMemcpyHostToDevice, c->stream) == hipSuccess;
        }
        if (!ok || hipStreamSynchronize(c->stream) != hipSuccess) return fail();   // (the tables are host temporaries: copied before they go)
    }
    if (p->has_cmul) {
        // the pre-resolved records of the CMUL stages: one device buffer (host temporaries: copied before they go)
        if (hipMalloc((void**)&p->cm_dev, sizeof cmt) != hipSuccess ||
            hipMemcpyAsync(p->cm_dev, cmt, sizeof cmt, hipMemcpyHostToDevice, c->stream) != hipSuccess || hipStreamSynchronize(c->stream) != hipSuccess)
            return fail();
    }
    *out = p;
    return QG_OK;
}

void qgemul_plan_destroy(qgemul_plan* p)
{
    if (!p) return;
    if (p->member) qgemul_plan_destroy(p->member);   // (a batched plan: its member owns the device resources)
    if (p->grp) {                                      // (a grouped plan: the distinct descriptors' plans do)
        for (int64_t u = 0; u < p->grp->n_uniq; ++u)
            if (p->grp->up[u]) qgemul_plan_destroy(p->grp->up[u]);
    }
    DeviceScope scope(p->ctx->device);
    hipStreamSynchronize(p->ctx->stream);
    if (p->grp) hipFree(p->grp->tiles_dev);
    delete p->grp;
    hipFree(p->dev_table);
    hipFree(p->workspace);
    hipFree(p->cwork);
    hipFree(p->wide_ws);
    hipFree(p->hostc_pc);
    hipFree(p->comp_slabs);
    hipFree(p->comp_acc);
    for (int k = 0; k < QG_MAX_EW; ++k) hipFree(p->ax_dev[k]);
    hipFree(p->cm_dev);
    delete p;
}

int qgemul_plan_info(const qgemul_plan* p, qgemul_info* out)
{
    if (!p || !out) return QG_EINVAL;
    *out = p->info;
    return QG_OK;
}

static QOperandGeom operand_geom(const qgemul_plan* p, int operand, int64_t ld)
{
    const qgemul_desc& d = p->desc;
    QOperandGeom g;
    memset(&g, 0, sizeof g);
    const QHostElem& h = operand == QG_OPERAND_A ? p->ha : p->hb;
    const qfmt* f = operand == QG_OPERAND_A ? d.a : d.b;
    g.K = d.K;
    g.parts = d.is_complex ? 2 : 1;
    g.elem_bytes = h.size;
    for (int q = 0; q < 2; ++q) {
        g.off[q] = h.off[q];
        g.sb[q] = h.sb[q];
        g.W[q] = (int)f[q].I + (int)f[q].F;
        g.S[q] = f[q].S;
        g.F[q] = f[q].F;
        g.Q[q] = f[q].Q;
        g.O[q] = f[q].O;
    }
    if (operand == QG_OPERAND_A) {
        g.rows = d.M;
        if (d.transA) { g.rs = ld ? ld : d.K; g.ks = 1; }   // A declared dim<K,M>: (i,k) at k + i*ld
        else { g.rs = 1; g.ks = ld ? ld : d.M; }            // A declared dim<M,K>: (i,k) at i + k*ld
    } else {
        g.rows = d.N;
        g.rs = ld ? ld : d.K;                                // B declared dim<K,N>: (k,j) at k + j*ld
        g.ks = 1;
    }
    return g;
}

int qgemul_pack(qgemul_plan* p, int operand, const void* src_dev, int64_t ld, void* packed_dev)
{
    if (!p || !src_dev || !packed_dev || (operand != QG_OPERAND_A && operand != QG_OPERAND_B)) return QG_EINVAL;
    if (p->batch) return QG_EINVAL;   // a batched plan runs through the _batched entry points
    QG_ON_DEVICE(p->ctx);
    QOperandGeom g = operand_geom(p, operand, ld);
    const QPackedGeom& pg = operand == QG_OPERAND_A ? p->pa : p->pb;
    const int check = (p->flags & QG_OPT_CHECK_RANGE) ? 1 : 0;
    if (check) QG_HIP(hipMemsetAsync(p->ctx->flag_dev, 0, 4, p->ctx->stream));
    if (p->comp.on) {
        QG_HIP(comp_zero_rowsums(p, operand, packed_dev));
        QG_HIP(comp_for_each_sub(p, operand, g, [&](const QOperandGeom& sg, const QPackedGeom& sp, int64_t off) {
            return qg_launch_pack(sg, sp, src_dev, (char*)packed_dev + off, check, p->ctx->flag_dev, p->ctx->stream, (p->flags & QG_OPT_GENERIC_LAYOUT) ? 1 : 0);
        }));
    } else
    QG_HIP(qg_launch_pack(g, pg, src_dev, packed_dev, check, p->ctx->flag_dev, p->ctx->stream, (p->flags & QG_OPT_GENERIC_LAYOUT) ? 1 : 0));
    if (check) {
        int flag = 0;
        QG_HIP(hipMemcpyAsync(&flag, p->ctx->flag_dev, 4, hipMemcpyDeviceToHost, p->ctx->stream));
        QG_HIP(hipStreamSynchronize(p->ctx->stream));
        if (flag) return QG_ERANGE;
    }
    return QG_OK;
}

int qgemul_pack_f64(qgemul_plan* p, int operand, const double* src_dev, int64_t ld, void* packed_dev)
{
    if (!p || !src_dev || !packed_dev || (operand != QG_OPERAND_A && operand != QG_OPERAND_B)) return QG_EINVAL;
    if (p->batch) return QG_EINVAL;   // a batched plan runs through the _batched entry points
    if (!(p->flags & QG_OPT_ARITHMETIC_CONV)) {
        // Qu_s(double) with QuMode<RND::CONV>: the reference's result is an artefact of its multi-word CONV branch
        // (QuBLAS.h:2137-2156 on ArbiInt<2400>); silently returning the arithmetic answer would break bit-exactness
        const qfmt* f = operand == QG_OPERAND_A ? p->desc.a : p->desc.b;
        for (int q = 0; q < (p->desc.is_complex ? 2 : 1); ++q)
            if (f[q].Q == QG_RND_CONV) return QG_EUNSUPPORTED;
    }
    QG_ON_DEVICE(p->ctx);
    QOperandGeom g = operand_geom(p, operand, ld);
    const QPackedGeom& pg = operand == QG_OPERAND_A ? p->pa : p->pb;
    if (p->comp.on) {
        QG_HIP(comp_zero_rowsums(p, operand, packed_dev));
        QG_HIP(comp_for_each_sub(p, operand, g, [&](const QOperandGeom& sg, const QPackedGeom& sp, int64_t off) {
            return qg_launch_pack_f64(sg, sp, src_dev, (char*)packed_dev + off, p->ctx->stream, (p->flags & QG_OPT_GENERIC_LAYOUT) ? 1 : 0);
        }));
        return QG_OK;
    }
    QG_HIP(qg_launch_pack_f64(g, pg, src_dev, packed_dev, p->ctx->stream, (p->flags & QG_OPT_GENERIC_LAYOUT) ? 1 : 0));
    return QG_OK;
}

int qgemul_fill_packed(qgemul_plan* p, int operand, uint64_t seed, int dist, void* packed_dev)
{
    if (!p || !packed_dev || (operand != QG_OPERAND_A && operand != QG_OPERAND_B)) return QG_EINVAL;
    if (p->batch) return QG_EINVAL;   // a batched plan runs through the _batched entry points
    QG_ON_DEVICE(p->ctx);
    QOperandGeom g = operand_geom(p, operand, 0);
    const QPackedGeom& pg = operand == QG_OPERAND_A ? p->pa : p->pb;
    if (p->comp.on) {
        QG_HIP(comp_zero_rowsums(p, operand, packed_dev));
        QG_HIP(comp_for_each_sub(p, operand, g, [&](const QOperandGeom& sg, const QPackedGeom& sp, int64_t off) {
            return qg_launch_fill(sg, sp, seed, dist, (char*)packed_dev + off, p->ctx->stream);
        }));
        return QG_OK;
    }
    QG_HIP(qg_launch_fill(g, pg, seed, dist, packed_dev, p->ctx->stream));
    return QG_OK;
}

int qgemul_unpack_c(qgemul_plan* p, const void* packed_dev, void* dst_dev, int64_t ld)
{
    if (!p || !packed_dev || !dst_dev) return QG_EINVAL;
    if (p->batch) return QG_EINVAL;   // a batched plan runs through the _batched entry points
    QG_ON_DEVICE(p->ctx);
    QCGeom c = p->pc;
    c.ldc = ld ? ld : p->desc.M;
    QG_HIP(qg_launch_unpack_c(c, packed_dev, dst_dev, p->ctx->stream, (p->flags & QG_OPT_GENERIC_LAYOUT) ? 1 : 0));
    return QG_OK;
}

static int execute_kernel(qgemul_plan* p, void* packedC, const void* packedA, const void* packedB, const qgemul_ep_args* epa, const HostC* hostc = nullptr);

int qgemul_execute(qgemul_plan* p, void* packedC, const void* packedA, const void* packedB)
{
    if (!p || !packedC || !packedA || !packedB) return QG_EINVAL;
    if (p->batch) return QG_EINVAL;   // a batched plan runs through the _batched entry points
    if (p->has_ep) return QG_EINVAL;  // a plan with an epilogue runs through qgemul_execute_ep
    if (p->desc.M == 0 || p->desc.N == 0) return QG_OK;
    QG_ON_DEVICE(p->ctx);
    return execute_kernel(p, packedC, packedA, packedB, nullptr);
}

// the kernels whose epilogue can store the reference layout: k_mfma_pp (QG_MFMA_PP) / k_mfma_ppl (QG_MFMA_PPL), real, 4- or 8-byte
// container equal to the host element, no raw-dot-product detour
bool stores_host_c(const qgemul_plan* p)
{
    if (p->has_ep || p->desc.is_complex || wide_epilogue(p) || p->comp.on) return false;
    if (p->info.kernel != QG_KERNEL_MFMA_I8 && p->info.kernel != QG_KERNEL_MFMA_I8_LIMB) return false;
    if (p->variant != QG_MFMA_PP && p->variant != QG_MFMA_PPL && p->variant != QG_MFMA_K6) return false;
    if (p->variant == QG_MFMA_PPL && (p->pa.rows_p / p->cfg.TM) * (p->pb.rows_p / p->cfg.TN) < 256) return false;   // (falls back to the lock-step kernel)
    return (p->pc.cbytes == 4 || p->pc.cbytes == 8) && p->pc.cbytes == p->hc.size;
}

int qgemul_plan_stores_host_c(const qgemul_plan* p) { return p && stores_host_c(p) ? 1 : 0; }

int qgemul_execute_host_c(qgemul_plan* p, void* C_dev, int64_t ldc, const void* packedA, const void* packedB)
{
    if (!p || !C_dev || !packedA || !packedB || p->has_ep) return QG_EINVAL;
    if (p->batch) return QG_EINVAL;   // a batched plan runs through the _batched entry points
    if (ldc && ldc < p->desc.M) return QG_EINVAL;
    if (p->desc.M == 0 || p->desc.N == 0) return QG_OK;
    QG_ON_DEVICE(p->ctx);
    if (stores_host_c(p)) {
        const HostC h{C_dev, ldc ? ldc : p->desc.M};
        return execute_kernel(p, C_dev, packedA, packedB, nullptr, &h);
    }
    if (!p->hostc_pc) QG_HIP(hipMalloc(&p->hostc_pc, (size_t)p->info.packed_bytes[2] ? (size_t)p->info.packed_bytes[2] : 16));
    const int st = execute_kernel(p, p->hostc_pc, packedA, packedB, nullptr);
    if (st != QG_OK) return st;
    QCGeom c = p->pc;
    c.ldc = ldc ? ldc : p->desc.M;
    QG_HIP(qg_launch_unpack_c(c, p->hostc_pc, C_dev, p->ctx->stream, (p->flags & QG_OPT_GENERIC_LAYOUT) ? 1 : 0));
    return QG_OK;
}

static int ep_args_ok(const qgemul_plan* p, const qgemul_ep_args* args)
{
    if (!args && p->ept.n > 0) return QG_EINVAL;
    for (int k = 0; k < p->ept.n; ++k)
        if ((!p->ept.st[k].scalar || (p->ep_cplx && !p->ept_im.st[k].scalar)) && !args->e_packed[k]) return QG_EINVAL;
    return QG_OK;
}

// the plan's chain as ONE linear pass: packed C (the kernel's own layout and container, pc_c) -> packed D
static int run_chain_pass(qgemul_plan* p, const void* packedC, void* packedD, const QEpArgs& a, const qgemul_ep_args* args)
{
    hipStream_t st = p->ctx->stream;
    QEltwiseArgs g;
    memset(&g, 0, sizeof g);
    g.C = (const char*)packedC;
    g.D = (char*)packedD;
    g.n = p->pc_c.Mp * p->pc_c.Np;
    g.cbytes = p->pc_c.cbytes;
    g.t = p->ept;
    g.a = a;
    if (p->has_ax) {
        QApproxArgs x;
        memset(&x, 0, sizeof x);
        x.g = g;
        for (int k = 0; k < QG_MAX_EW; ++k) x.ax[k] = p->ax_dev[k];
        x.force_general = (p->flags & QG_OPT_APPROX_GENERAL) ? 1 : 0;   // result-identical form choice (include/qgemul.h)
        QG_HIP(qg_launch_approx(x, st));
        return QG_OK;
    }
    if (p->has_cmul) {
        // a CMUL stage needs both parts of an element in one thread: ONE pass whose lanes own both halves
        QCplxPassArgs x;
        memset(&x, 0, sizeof x);
        x.C = g.C;
        x.D = g.D;
        x.n = g.n;
        x.cbytes = g.cbytes;
        x.t[0] = p->ept;
        x.t[1] = p->ept_im;
        x.a = a;
        for (int k = 0; k < p->ept.n; ++k) x.scalar_im[k] = args->e_scalar_im[k];
        memcpy(x.e_cplx, p->e_cplx, sizeof x.e_cplx);
        x.cm = p->cm_dev;
        QG_HIP(qg_launch_eltwise_cplx(x, st));
        return QG_OK;
    }
    QG_HIP(qg_launch_eltwise(g, st));
    if (p->ep_cplx) {
        // the chain of the imaginary parts: the second half of packed C, of packed D and of every complex tensor operand
        g.C += g.n * g.cbytes;
        g.D += g.n * p->ept.dbytes;
        g.t = p->ept_im;
        for (int k = 0; k < p->ept_im.n; ++k) {
            if (g.a.e[k] && p->e_cplx[k]) g.a.e[k] += g.n * p->ept_im.st[k].ebytes;
            g.a.scalar[k] = args->e_scalar_im[k];
        }
        QG_HIP(qg_launch_eltwise(g, st));
    }
    return QG_OK;
}

static QEpArgs ep_device_args(const qgemul_plan* p, const qgemul_ep_args* args)
{
    QEpArgs a;
    memset(&a, 0, sizeof a);
    for (int k = 0; k < p->ept.n; ++k) {
        a.e[k] = (const char*)args->e_packed[k];
        a.scalar[k] = args->e_scalar[k];
    }
    return a;
}

int qgemul_apply_epilogue(qgemul_plan* p, void* packedD, const void* packedC, const qgemul_ep_args* args)
{
    if (!p || !packedD || !packedC || !p->has_ep) return QG_EINVAL;
    if (p->batch) return QG_EINVAL;   // a batched plan runs through the _batched entry points
    if (int s = ep_args_ok(p, args)) return s;
    if (p->desc.M == 0 || p->desc.N == 0) return QG_OK;
    QG_ON_DEVICE(p->ctx);
    return run_chain_pass(p, packedC, packedD, ep_device_args(p, args), args);
}

int qgemul_time_apply_epilogue(qgemul_plan* p, void* packedD, const void* packedC, const qgemul_ep_args* args, int warmup, int iters, float* avg_ms)
{
    if (!p || !avg_ms || iters < 1) return QG_EINVAL;
    for (int i = 0; i < warmup; ++i)
        if (int s = qgemul_apply_epilogue(p, packedD, packedC, args)) return s;
    QG_ON_DEVICE(p->ctx);
    hipStream_t st = p->ctx->stream;
    hipEvent_t e0 = nullptr, e1 = nullptr;
    int rc = QG_OK;
    float ms = 0;
    hipError_t he = hipEventCreate(&e0);
    if (he == hipSuccess) he = hipEventCreate(&e1);
    if (he == hipSuccess) he = hipEventRecord(e0, st);
    for (int i = 0; he == hipSuccess && rc == QG_OK && i < iters; ++i) rc = qgemul_apply_epilogue(p, packedD, packedC, args);
    if (he == hipSuccess && rc == QG_OK) he = hipEventRecord(e1, st);
    if (he == hipSuccess && rc == QG_OK) he = hipEventSynchronize(e1);
    if (he == hipSuccess && rc == QG_OK) he = hipEventElapsedTime(&ms, e0, e1);
    if (e0) hipEventDestroy(e0);
    if (e1) hipEventDestroy(e1);
    if (he != hipSuccess) { g_last_hip = (int)he; return QG_EHIP; }
    if (rc != QG_OK) return rc;
    *avg_ms = ms / (float)iters;
    return QG_OK;
}

int qgemul_execute_ep(qgemul_plan* p, void* packedD, const void* packedA, const void* packedB, const qgemul_ep_args* args)
{
    if (!p || !packedD || !packedA || !packedB) return QG_EINVAL;
    if (p->batch) return QG_EINVAL;   // a batched plan runs through the _batched entry points
    if (!p->has_ep) return args ? QG_EINVAL : qgemul_execute(p, packedD, packedA, packedB);
    if (int s = ep_args_ok(p, args)) return s;
    if (p->desc.M == 0 || p->desc.N == 0) return QG_OK;
    QG_ON_DEVICE(p->ctx);
    const QEpArgs a = ep_device_args(p, args);
    hipStream_t st = p->ctx->stream;
    if (fuses_epilogue(p)) {
        // fused: the MFMA kernel's epilogue runs the chain on the value it has just converted into C's type
        QMfmaArgs m = mfma_args(p, packedA, packedB, packedD, p->pc_c.cbytes);
        m.has_ep = 1;
        m.ep = p->ept;
        m.epa = a;
        QG_HIP(qg_launch_mfma(p->LA, p->LB, m, st));
        return QG_OK;
    }
    // not fused: the kernel stores C into the plan's buffer, one linear pass turns it into D
    const int s = execute_kernel(p, p->cwork, packedA, packedB, nullptr);
    if (s != QG_OK) return s;
    return run_chain_pass(p, p->cwork, packedD, a, args);
}

int qgemul_plan_fuses_epilogue(const qgemul_plan* p)
{
    if (p && p->batch) return p->has_ep && (p->bd ? p->bd_fused : fuses_epilogue(p->member)) ? 1 : 0;
    return p && p->has_ep && fuses_epilogue(p) ? 1 : 0;
}

int qgemul_plan_packed_layout(const qgemul_plan* p, int operand, int64_t out[4])
{
    if (!p || !out || (operand != QG_OPERAND_A && operand != QG_OPERAND_B)) return QG_EINVAL;
    if (p->grp) return QG_EINVAL;   // a grouped plan answers qgemul_plan_grouped_member
    const QPackedGeom& g = operand == QG_OPERAND_A ? p->pa : p->pb;
    out[0] = p->comp.on ? 0 : g.trailer;
    out[1] = g.offs ? g.rowsum_off : 0;
    out[2] = g.rows_p;
    out[3] = g.offs ? -g.bias : 0;
    return QG_OK;
}

// the stage entry that reads stage k's tensor operand (nullptr: the stage has no tensor operand)
static const QEpStage* stage_tensor(const qgemul_plan* p, int k)
{
    if (!p->ept.st[k].scalar) return &p->ept.st[k];
    if (p->ep_cplx && !p->ept_im.st[k].scalar) return &p->ept_im.st[k];
    return nullptr;
}

int64_t qgemul_packed_c_bytes(const qgemul_plan* p)
{
    return p && p->has_ep && p->batch < 1 ? (int64_t)p->pc_c.parts * p->pc_c.Mp * p->pc_c.Np * p->pc_c.cbytes : 0;
}

// a tensor of the GEMM result's own element type -> the packed C the chain's pass reads (qgemul_apply_epilogue)
int qgemul_pack_c(qgemul_plan* p, const void* src_dev, int64_t ld, void* packed_dev)
{
    if (!p || !src_dev || !packed_dev || !p->has_ep) return QG_EINVAL;
    if (p->batch) return QG_EINVAL;   // a batched plan runs through the _batched entry points
    if (ld && ld < p->desc.M) return QG_EINVAL;
    QG_ON_DEVICE(p->ctx);
    const QHostElem h = qg_host_elem(p->desc.c, p->desc.is_complex);
    for (int part = 0; part < p->pc_c.parts; ++part)
        QG_HIP(qg_launch_pack_e(p->pc_c, part, src_dev, ld ? ld : p->desc.M, h.size, h.off[part], h.sb[part], packed_dev, p->pc_c.cbytes, p->ctx->stream));
    return QG_OK;
}

int64_t qgemul_packed_e_bytes(const qgemul_plan* p, int stage)
{
    if (!p || !p->has_ep || stage < 0 || stage >= p->ept.n) return 0;
    if (p->batch) return p->e_shared[stage] ? p->estride[stage] : p->batch * p->estride[stage];   // (one member's / the stack's)
    const QEpStage* t = stage_tensor(p, stage);
    if (!t) return 0;
    return (p->ep_cplx && p->e_cplx[stage] ? 2 : 1) * p->pc.Mp * p->pc.Np * (int64_t)t->ebytes;
}

int qgemul_pack_e(qgemul_plan* p, int stage, const void* src_dev, int64_t ld, void* packed_dev)
{
    if (!p || !src_dev || !packed_dev || !p->has_ep || stage < 0 || stage >= p->ept.n) return QG_EINVAL;
    if (p->batch) return QG_EINVAL;   // a batched plan runs through the _batched entry points
    const QEpStage* t = stage_tensor(p, stage);
    if (!t) return QG_EINVAL;
    if (ld && ld < p->desc.M) return QG_EINVAL;
    QG_ON_DEVICE(p->ctx);
    const bool cplx = p->ep_cplx && p->e_cplx[stage];
    // host element of the operand tensor: int32 / int64 raw values, {re, im} structs for a complex operand (QuBLAS.h:2512-2513)
    const qfmt f[2] = {t == &p->ept.st[stage] ? p->ep.stage[stage].e : p->ep_im.stage[stage].e, p->ep_im.stage[stage].e};
    const QHostElem h = qg_host_elem(f, cplx ? 1 : 0);
    for (int part = 0; part < (cplx ? 2 : 1); ++part)
        QG_HIP(qg_launch_pack_e(p->pc, part, src_dev, ld ? ld : p->desc.M, h.size, h.off[part], h.sb[part], packed_dev, t->ebytes, p->ctx->stream));
    return QG_OK;
}

// composite linear plan: per k-chunk, one MFMA launch per (A group, B group) storing raw dot products into its slab, then the
// exact combine pass (running sums between chunks; one round + overflow into C after the last)
static int execute_composite(qgemul_plan* p, void* packedC, const void* packedA, const void* packedB, const QCGeom& pcg)
{
    const QComposite& q = p->comp;
    hipStream_t st = p->ctx->stream;
    const int64_t n = p->pa.rows_p * p->pb.rows_p;
    for (int c = 0; c < q.nc; ++c) {
        QLinCombine cb;
        memset(&cb, 0, sizeof cb);
        for (int i = 0; i < q.ga; ++i)
            for (int j = 0; j < q.gb; ++j) {
                int64_t offA = 0, offB = 0;
                const QPackedGeom sa = comp_sub_geom(q, p->pa, 0, p->desc.K, c, i, &offA);
                const QPackedGeom sb = comp_sub_geom(q, p->pb, 1, p->desc.K, c, j, &offB);
                char* slab = (char*)p->comp_slabs + (size_t)(i * q.gb + j) * (size_t)n * (size_t)q.slab_bytes;
                QMfmaArgs a = mfma_args(sa, sb, q.var[i][j], (const char*)packedA + offA, (const char*)packedB + offB, slab, q.slab_bytes);
                a.to_c.identity = 1;   // raw dot products
                QG_HIP(qg_launch_mfma(sa.limbs, sb.limbs, a, st));
                cb.slab[cb.n_slabs] = slab;
                cb.sh[cb.n_slabs] = 8 * (sa.limb0 + sb.limb0);
                ++cb.n_slabs;
            }
        cb.slab_bytes = q.slab_bytes;
        cb.n = n;
        cb.acc_in = c > 0 ? p->comp_acc : nullptr;
        cb.acc_out = c + 1 < q.nc ? p->comp_acc : nullptr;
        cb.out = packedC;
        cb.cbytes = pcg.cbytes;
        cb.wide = q.wide;
        cb.to_c = p->an.lin.to_c[0];
        if (p->pa.offs) {   // centred operands: the last chunk's pass takes the centres back out
            cb.rsA = (const int64_t*)((const char*)packedA + p->pa.rowsum_off);
            cb.rsB = (const int64_t*)((const char*)packedB + p->pb.rowsum_off);
            cb.biasA = p->pa.bias;
            cb.biasB = p->pb.bias;
            cb.corr = p->desc.K;
            cb.tm = pcg.tm;
            cb.tn = pcg.tn;
            cb.tiles_n = pcg.tn ? pcg.Np / pcg.tn : 1;
        }
        QG_HIP(qg_launch_lin_combine(cb, st));
    }
    return QG_OK;
}

static int execute_kernel(qgemul_plan* p, void* packedC, const void* packedA, const void* packedB, const qgemul_ep_args*, const HostC* hostc)
{
    hipStream_t st = p->ctx->stream;
    const QCGeom& pcg = p->has_ep ? p->pc_c : p->pc;
    if (p->comp.on) return execute_composite(p, packedC, packedA, packedB, pcg);
    switch (p->info.kernel) {
    case QG_KERNEL_MFMA_I8:
    case QG_KERNEL_MFMA_I8_LIMB: {
        if (p->variant == QG_MFMA_RING) {
            QRingArgs r;
            memset(&r, 0, sizeof r);
            r.A = (const int8_t*)packedA;
            r.B = (const int8_t*)packedB;
            r.C = packedC;
            r.Mp = p->pa.rows_p;
            r.Np = p->pb.rows_p;
            r.Kp = p->pa.K_p;
            r.cbytes = pcg.cbytes;
            r.n = p->an.ring_n;
            r.s = p->an.ring_s;
            r.to_c = p->an.tree.c_cvt[0];
            QG_HIP(qg_launch_mfma_ring(p->LA, p->LB, qg_ring_digits(p->an.ring_n), r, st));
            return QG_OK;
        }
        QMfmaArgs a = mfma_args(p, packedA, packedB, packedC, pcg.cbytes);
#ifdef QG_DIAG
        a.dbg = g_diag_stamps;
#endif
        if (p->pa.digit6) {
            a.kara = 1;
            a.rsA = (const int64_t*)((const char*)packedA + p->pa.rowsum_off);
            a.rsB = (const int64_t*)((const char*)packedB + p->pb.rowsum_off);
            a.biasA = p->pa.bias;
            a.biasB = p->pb.bias;
            a.corr = p->desc.K * p->pa.bias * p->pb.bias;
            a.Mc = pcg.Mp;
        }
        if (wide_epilogue(p)) {
            a.C = p->wide_ws;
            a.cbytes = 4;
            memset(&a.to_c, 0, sizeof a.to_c);
            a.to_c.identity = 1;                    // raw int32 dot products ...
            QG_HIP(qg_launch_mfma(p->LA, p->LB, a, st));
            QEltwiseArgs f;
            memset(&f, 0, sizeof f);
            f.C = (const char*)p->wide_ws;
            f.D = (char*)packedC;
            f.n = pcg.Mp * pcg.Np;
            f.cbytes = 4;
            f.t.dbytes = pcg.cbytes;
            f.t.to_d = p->an.lin.to_c[0];           // ... shifted, overflow-handled and stored in 64-bit arithmetic
            QG_HIP(qg_launch_eltwise(f, st));
            return QG_OK;
        }
        if (hostc) {   // (only reached when stores_host_c(p): see qgemul_execute_host_c)
            a.C = hostc->C;
            a.c_host = 1;
            a.c_ld = hostc->ld;
            a.c_M = p->desc.M;
            a.c_N = p->desc.N;
            a.c_vec = (((uintptr_t)hostc->C & 15) == 0 && (hostc->ld * pcg.cbytes) % 16 == 0) ? 1 : 0;
        }
        QG_HIP(qg_launch_mfma(p->LA, p->LB, a, st));
        return QG_OK;
    }
    case QG_KERNEL_MFMA_CPLX: {
        QMfmaArgs a = mfma_args(p->pa, p->pb, p->variant, packedA, packedB, p->workspace, 8);
        a.Mp = 2 * p->pa.rows_p;   // the parts stacked along the rows: one real GEMM of twice the extents
        a.Np = 2 * p->pb.rows_p;
        a.to_c.identity = 1;  // raw 64-bit dot products
        QG_HIP(qg_launch_mfma(p->LA, p->LB, a, st));
        QCplxCombine g;
        g.D = p->workspace;
        g.C = (char*)packedC;
        g.M = p->desc.M;
        g.N = p->desc.N;
        g.Mh = p->pa.rows_p;
        g.Nh = p->pb.rows_p;
        g.Np = 2 * p->pb.rows_p;
        g.tm = p->cfg.TM;
        g.tn = p->cfg.TN;
        g.cbytes = pcg.cbytes;
        for (int i = 0; i < 4; ++i) g.sh[i] = p->an.lin.sh[i];
        g.to_c[0] = p->an.lin.to_c[0];
        g.to_c[1] = p->an.lin.to_c[1];
        QG_HIP(qg_launch_cplx_combine(g, st));
        return QG_OK;
    }
    case QG_KERNEL_TREE_I32:
        QG_HIP(qg_launch_tree_fast(p->dev_table, p->an.tree.n_levels_k, p->an.split_s, p->an.mul24_ok, p->tc.tree, packedA, packedB, packedC,
                                   p->desc.M, p->desc.N, p->pa.K_p, pcg.cbytes, st));
        return QG_OK;
    case QG_KERNEL_GEMV_I64:
        QG_HIP(qg_launch_gemv(p->dev_table, p->an.tree.n_levels_k, p->an.gemv_b_bit, QGF_RUNTIME, packedA, packedB, packedC, p->desc.M, p->pa.K_p,
                              pcg.cbytes, st, 1));
        return QG_OK;
    case QG_KERNEL_GEMV_I32:
        QG_HIP(qg_launch_gemv(p->dev_table, p->an.tree.n_levels_k, p->an.gemv_b_bit, p->tc.gemv, packedA, packedB, packedC, p->desc.M, p->pa.K_p,
                              pcg.cbytes, st));
        return QG_OK;
    case QG_KERNEL_TREE_CPLX_I32:
        QG_HIP(qg_launch_tree_cplx_fast(p->dev_table, p->an.tree.n_levels_k, p->tc.cplx, p->desc.cmul == QG_CMUL_TF ? 1 : 0, packedA, packedB, packedC,
                                        p->desc.M, p->desc.N, p->pa.K_p, pcg.cbytes, st));
        return QG_OK;
    case QG_KERNEL_TREE_I64:
        if (p->an.tree64_ok && !(p->flags & QG_OPT_GENERIC_TREE)) {
            QG_HIP(qg_launch_tree64(p->dev_table, p->an.tree.n_levels_k, packedA, packedB, packedC, p->desc.M, p->desc.N, p->pa.K_p,
                                    p->pa.cbytes, p->pb.cbytes, pcg.cbytes, st));
            return QG_OK;
        }
        [[fallthrough]];
    case QG_KERNEL_TREE_CPLX:
        QG_HIP(qg_launch_tree_generic(p->dev_table, p->desc.is_complex ? 2 : 1, packedA, packedB, packedC, p->desc.M, p->desc.N,
                                      p->desc.K, p->pa, p->pb, pcg, st));
        return QG_OK;
    case QG_KERNEL_TREE_I128:
        QG_HIP(qg_launch_tree_generic(p->dev_table, p->desc.is_complex ? 2 : 1, packedA, packedB, packedC, p->desc.M, p->desc.N,
                                      p->desc.K, p->pa, p->pb, pcg, st, 1));
        return QG_OK;
    default:
        return QG_EUNSUPPORTED;
    }
}

static int result_width(const qgemul_plan* p, int part = 0)
{
    const qfmt f = p->has_ep ? (part ? p->ep_im.d : p->ep.d) : p->desc.c[part];
    return (int)f.I + (int)f.F + (f.S ? 1 : 0);
}

int64_t qgemul_bitstream_bytes(const qgemul_plan* p, int format)
{
    if (!p || p->batch) return 0;
    const int64_t n = p->desc.M * p->desc.N;
    // complex: "(re-bits, im-bits)" per element as characters; packed: the binary characters only
    const int64_t bits = p->desc.is_complex ? n * (result_width(p, 0) + result_width(p, 1) + (format == QG_BITS_PACKED ? 0 : 4)) : n * (int64_t)result_width(p);
    // the packed form is written with 32-bit atomics: sized to whole words
    return format == QG_BITS_PACKED ? ((bits + 7) / 8 + 3) / 4 * 4 : bits;
}

int qgemul_export_bitstream(qgemul_plan* p, const void* packedC, int tensor_chunk, int elem_chunk, int format, void* out_dev)
{
    if (!p || !packedC || !out_dev || (format != QG_BITS_ASCII && format != QG_BITS_PACKED)) return QG_EINVAL;
    if (p->batch) return QG_EINVAL;   // a batched plan runs through the _batched entry points
    const int w = p->desc.is_complex ? result_width(p, 0) + result_width(p, 1) + 4 : result_width(p);
    const int64_t n = p->desc.M * p->desc.N;
    if (w <= 0 || tensor_chunk < 0 || elem_chunk < 0) return QG_EINVAL;
    if (!p->desc.is_complex && (w > 64 || p->pc.cbytes > 8)) return QG_EUNSUPPORTED;   // (multi-word elements: not exported)
    if (elem_chunk > 0 && w % elem_chunk) return QG_EINVAL;      // the reference throws (QuBLAS.h:4599-4602)
    if (tensor_chunk > 0 && n % tensor_chunk) return QG_EINVAL;  // the reference's loop does not terminate (:4745)
    QG_ON_DEVICE(p->ctx);
    if (p->desc.is_complex) {
        const int wr = result_width(p, 0), wi = result_width(p, 1);
        if (wr < 0 || wi < 0 || wr > 64 || wi > 64) return QG_EINVAL;   // (a part without bits prints as the empty string)
        QBitsCplxArgs a;
        memset(&a, 0, sizeof a);
        a.c = p->pc;
        a.packed = (const char*)packedC;
        a.out = (char*)out_dev;
        a.width = w;
        a.nbits = wr + wi;
        a.tensor_chunk = tensor_chunk;
        a.packed_bits = format == QG_BITS_PACKED;
        // the element string "(" re ", " im ")" (QuBLAS.h:2553-2556), MSB first per part, then its chunks reversed (:4593-4611)
        uint8_t str[136];
        int k = 0;
        str[k++] = QG_BITS_LIT_OPEN;
        for (int j = 0; j < wr; ++j) str[k++] = (uint8_t)(wr - 1 - j);
        str[k++] = QG_BITS_LIT_COMMA;
        str[k++] = QG_BITS_LIT_SPACE;
        for (int j = 0; j < wi; ++j) str[k++] = (uint8_t)(64 + wi - 1 - j);
        str[k++] = QG_BITS_LIT_CLOSE;
        if (elem_chunk > 0) {
            const int nch = w / elem_chunk;
            for (int q = 0; q < nch; ++q)
                for (int r = 0; r < elem_chunk; ++r) a.tab[q * elem_chunk + r] = str[(nch - 1 - q) * elem_chunk + r];
        } else {
            memcpy(a.tab, str, (size_t)w);
        }
        QG_HIP(qg_launch_bitstream_cplx(a, p->ctx->stream));
        return QG_OK;
    }
    QBitsArgs a;
    memset(&a, 0, sizeof a);
    a.c = p->pc;
    a.packed = (const char*)packedC;
    a.out = (char*)out_dev;
    a.width = w;
    a.tensor_chunk = tensor_chunk;
    a.elem_chunk = elem_chunk;
    a.packed_bits = format == QG_BITS_PACKED;
    QG_HIP(qg_launch_bitstream(a, p->ctx->stream));
    return QG_OK;
}

static int time_execute(qgemul_plan* p, void* packedC, const void* packedA, const void* packedB, const qgemul_ep_args* args,
                        int warmup, int iters, float* avg_ms, int kind = 0)   // kind: 0 a plain plan, 1 a batched one, 2 a grouped one
{
    const bool batched = kind == 1;
    if (!p || !avg_ms || iters < 1 || (kind == 2 ? !p->grp : (p->batch != 0) != batched)) return QG_EINVAL;
    QG_ON_DEVICE(p->ctx);
    hipStream_t st = p->ctx->stream;
    auto once = [&]() {
        if (kind == 2) return qgemul_execute_grouped(p, packedC, packedA, packedB);
        if (batched) return p->has_ep ? qgemul_execute_batched_ep(p, packedC, packedA, packedB, args) : qgemul_execute_batched(p, packedC, packedA, packedB);
        return p->has_ep ? qgemul_execute_ep(p, packedC, packedA, packedB, args) : qgemul_execute(p, packedC, packedA, packedB);
    };
    for (int i = 0; i < warmup; ++i) {
        int s = once();
        if (s) return s;
    }
    hipEvent_t e0 = nullptr, e1 = nullptr;
    int rc = QG_OK;
    float ms = 0;
    hipError_t he = hipEventCreate(&e0);
    if (he == hipSuccess) he = hipEventCreate(&e1);
    if (he == hipSuccess) he = hipEventRecord(e0, st);
    for (int i = 0; he == hipSuccess && rc == QG_OK && i < iters; ++i) rc = once();
    if (he == hipSuccess && rc == QG_OK) he = hipEventRecord(e1, st);
    if (he == hipSuccess && rc == QG_OK) he = hipEventSynchronize(e1);
    if (he == hipSuccess && rc == QG_OK) he = hipEventElapsedTime(&ms, e0, e1);
    if (e0) hipEventDestroy(e0);   // (released on every path)
    if (e1) hipEventDestroy(e1);
    if (he != hipSuccess) { g_last_hip = (int)he; return QG_EHIP; }
    if (rc != QG_OK) return rc;
    *avg_ms = ms / (float)iters;
    return QG_OK;
}

int qgemul_time_execute(qgemul_plan* p, void* packedC, const void* packedA, const void* packedB, int warmup, int iters,
                        float* avg_ms)
{
    return time_execute(p, packedC, packedA, packedB, nullptr, warmup, iters, avg_ms);
}

int qgemul_time_execute_ep(qgemul_plan* p, void* packedD, const void* packedA, const void* packedB, const qgemul_ep_args* args,
                           int warmup, int iters, float* avg_ms)
{
    return time_execute(p, packedD, packedA, packedB, args, warmup, iters, avg_ms);
}


// ---- batched Qgemul: `batch` GEMMs of one descriptor at constant strides (include/qgemul.h) ----
// kernel launches of one qgemul_execute on a plain plan (a 3 x 3 launch pair counts once: its partner returns in its first instructions)
static int plan_launches(const QPlanGeom* p)
{
    if (p->comp.on) return p->comp.nc * (p->comp.ga * p->comp.gb + 1);
    switch (p->info.kernel) {
    case QG_KERNEL_MFMA_I8:
    case QG_KERNEL_MFMA_I8_LIMB: return p->variant != QG_MFMA_RING && wide_epilogue(p) ? 2 : 1;
    case QG_KERNEL_MFMA_CPLX: return 2;
    default: return 1;
    }
}

int64_t member_extent(const qgemul_desc& d, int operand, int64_t ld)
{
    const int64_t rows = operand == QG_OPERAND_A ? (d.transA ? d.K : d.M) : operand == QG_OPERAND_B ? d.K : d.M;
    const int64_t cols = operand == QG_OPERAND_A ? (d.transA ? d.M : d.K) : d.N;
    if (!ld) ld = rows;
    if (ld < rows) return 0;
    return cols > 0 && rows > 0 ? (cols - 1) * ld + rows : 1;
}

// the geometry of a batched plan, pure host code: m (zeroed) receives the member's, b (zeroed) the batch's
// ev: the chain of a batched plan with one (qgemul_plan_create_batched_epx), bep: which of its tensor operands are shared
static int batched_geometry(const qgemul_desc* d, int64_t batch, uint32_t flags, QPlanGeom* m, qgemul_plan* b, const EpView* ev, const qgemul_batched_ep* bep)
{
    if (!d || batch < 1) return QG_EINVAL;
    bool has_ax = false;
    for (int k = 0; ev && ev->ax && k < QG_MAX_EW; ++k) has_ax |= ev->ax[k] != nullptr;
    const int st = plan_geometry(d, flags, ev, batch, m, nullptr, nullptr);
    b->info = m->info;
    if (st != QG_OK) return st;
    const int bd = m->bd;
    b->desc = *d;
    b->flags = flags;
    b->batch = batch;
    b->bd = bd;
    b->LA = m->LA;
    b->LB = m->LB;
    b->cfg = m->cfg;
    b->variant = m->variant;
    b->ha = m->ha;
    b->hb = m->hb;
    b->hc = m->hc;
    b->pc = m->pc;
    b->member_launches = plan_launches(m);
    int64_t total[3];
    bool over = false;
    if (ev) {
        // the chain is the member's; what one member's qgemul_execute_ep issues: its kernel and, unless fused, the chain's pass
        b->has_ep = 1;
        b->has_ax = has_ax;
        b->ep = *ev->re;
        b->ept = m->ept;
        b->pc_c = m->pc_c;
        if (!fuses_epilogue(m, flags, has_ax, false)) b->member_launches += 1;
        // fused form: what fuses_epilogue accepts on arithmetic grounds, on request (the default between the two block-diagonal
        // forms is the pass until tools/measure_batched_ep.py has decided otherwise: DESIGN.md section 9)
        b->bd_fused = bd && m->ept.bits32 && !has_ax && (flags & QG_OPT_FUSED_EPILOGUE) && !(flags & QG_OPT_UNFUSED_EPILOGUE);
        for (int k = 0; k < m->ept.n; ++k) {
            const QEpStage& s = m->ept.st[k];
            if (s.scalar || s.op == QG_EW_APPROX) continue;
            b->e_shared[k] = bep && bep->e_shared[k] ? 1 : 0;
            // (member by member: 256-byte steps like the other packed operands', so that every member's operand keeps the alignment the
            // pass's 16-byte loads have on a plain plan)
            int64_t stack = 0;
            over |= __builtin_mul_overflow(m->pc.Mp * m->pc.Np, (int64_t)s.ebytes, &b->estride[k]);
            if (!bd) b->estride[k] = round_up(b->estride[k], 256);
            over |= __builtin_mul_overflow(b->estride[k], batch, &stack) || stack > (1ll << 60);
        }
    }
    if (bd) {
        int64_t tiles = 0;
        over |= __builtin_mul_overflow((m->pa.rows_p / m->cfg.TM) * (m->pb.rows_p / m->cfg.TN), batch, &tiles) || tiles > 0x7fffffffll;
        QPackedGeom* sg[2] = {&b->pa, &b->pb};
        const QPackedGeom* mg[2] = {&m->pa, &m->pb};
        for (int w = 0; w < 2 && !over; ++w) {
            QPackedGeom& s = *sg[w];
            s = *mg[w];
            int64_t planes = 0;
            over |= __builtin_mul_overflow(s.rows_p, batch, &s.rows_p) || __builtin_mul_overflow((int64_t)s.limbs * s.K_p, s.rows_p, &planes) || planes > (1ll << 60);
            b->mstride[w] = (int64_t)mg[w]->limbs * mg[w]->rows_p * mg[w]->K_p;
            int64_t bytes = planes;
            s.trailer = 0;
            if (s.limbs > 1) { s.trailer = bytes; bytes += QG_TRAILER_BYTES; }   // ONE plane mask: the OR over every member
            if (s.offs) {                                                         // ONE row-sum array behind the planes of all members
                s.rowsum_off = round_up(bytes, 256);
                bytes = s.rowsum_off + s.rows_p * 8;
            }
            total[w] = bytes;
        }
        b->mstride[2] = m->info.packed_bytes[2];
        over |= __builtin_mul_overflow(b->mstride[2], batch, &total[2]);
        snprintf(b->info.reason, sizeof b->info.reason, "linear class: %lld members in one block-diagonal launch, %dx%d tiles", (long long)batch, m->cfg.TM, m->cfg.TN);
        if (ev)
            snprintf(b->info.reason, sizeof b->info.reason, b->bd_fused ? "linear class: %lld members, chain fused into one block-diagonal launch" : "linear class: %lld members, block-diagonal launch + one chain pass over the stack",
                     (long long)batch);
    } else {
        for (int w = 0; w < 3; ++w) {
            b->mstride[w] = round_up(m->info.packed_bytes[w], 256);
            over |= __builtin_mul_overflow(b->mstride[w], batch, &total[w]) || total[w] > (1ll << 60);
        }
        b->pa = m->pa;
        b->pb = m->pb;
        if (ev) {
            char why[sizeof m->info.reason];
            memcpy(why, m->info.reason, sizeof why);
            snprintf(b->info.reason, sizeof b->info.reason, "chain member by member: %.70s", why);
        }
    }
    if (over) {
        b->info.supported = 0;
        snprintf(b->info.reason, sizeof b->info.reason, "batched plan: more than 2^31 - 1 tiles / packed operands beyond the address range");
        return QG_EINVAL;
    }
    for (int w = 0; w < 3; ++w) b->info.packed_bytes[w] = total[w];
    b->info.ops = m->info.ops * (double)batch;
    return QG_OK;
}

// a batched plan's host side: *out = the plan (heap, zeroed, then filled; the caller's to release with `delete`, whatever the status:
// its info says why a descriptor was refused).  ev == nullptr: no chain
static int batched_plan_new(const qgemul_desc* d, int64_t batch, uint32_t flags, const EpView* ev, const qgemul_batched_ep* bep, qgemul_plan** out)
{
    *out = nullptr;
    qgemul_plan* b = new (std::nothrow) qgemul_plan();
    QPlanGeom* m = new (std::nothrow) QPlanGeom();   // the member's geometry: needed only while the batch's is derived from it
    const int st = b && m ? batched_geometry(d, batch, flags, m, b, ev, bep) : QG_EINVAL;
    delete m;
    if (!b) return QG_EINVAL;
    *out = b;
    return st;
}

int classify_batched_view(const qgemul_desc* d, int64_t batch, const EpView* ev, const qgemul_batched_ep* bep, uint32_t opt_flags, qgemul_info* out, int* launches)
{
    if (!d) return QG_EINVAL;
    qgemul_plan* b = nullptr;
    const int st = batched_plan_new(d, batch, opt_flags, ev, bep, &b);
    if (!b) return st;
    if (out && batch >= 1) *out = b->info;
    if (launches && st == QG_OK) *launches = qgemul_plan_batched_launches(b);
    delete b;
    return st;
}

int qgemul_classify_batched(const qgemul_desc* d, int64_t batch, uint32_t opt_flags, qgemul_info* out)
{
    if (!d || !out) return QG_EINVAL;
    return classify_batched_view(d, batch, nullptr, nullptr, opt_flags, out, nullptr);
}

int qgemul_classify_batched_launches(const qgemul_desc* d, int64_t batch, uint32_t opt_flags)
{
    int n = 0;
    const int st = classify_batched_view(d, batch, nullptr, nullptr, opt_flags, nullptr, &n);
    return st == QG_OK ? n : st;
}

// the member owns every device resource (with a chain: its device tables as well) except the block-diagonal pass form's packed C
int plan_create_batched_view(qgemul_ctx* c, const qgemul_desc* d, int64_t batch, const EpView* ev, const qgemul_batched_ep* bep, uint32_t opt_flags, qgemul_plan** out)
{
    if (!c || !d || !out) return QG_EINVAL;
    qgemul_plan* b = nullptr;
    int st = batched_plan_new(d, batch, opt_flags, ev, bep, &b);
    if (!b) return st;
    if (st == QG_OK) st = plan_create_view(c, d, ev, opt_flags, &b->member, batch);
    if (st != QG_OK) { delete b; return st; }
    b->ctx = c;
    if (b->has_ep && b->bd && !b->bd_fused) {   // the pass form: the stack's packed C between the two launches
        DeviceScope scope(c->device);
        const size_t cb = (size_t)batch * (size_t)(b->pc_c.Mp * b->pc_c.Np) * (size_t)b->pc_c.cbytes;
        if (scope.err != hipSuccess || hipMalloc(&b->cwork, cb ? cb : 16) != hipSuccess) {
            qgemul_plan_destroy(b);
            return QG_EHIP;
        }
    }
    *out = b;
    return QG_OK;
}

int qgemul_plan_create_batched(qgemul_ctx* c, const qgemul_desc* d, int64_t batch, uint32_t opt_flags, qgemul_plan** out)
{
    return plan_create_batched_view(c, d, batch, nullptr, nullptr, opt_flags, out);
}

int qgemul_plan_batched_launches(const qgemul_plan* p)
{
    if (!p || p->batch < 1) return QG_EINVAL;
    if (p->bd) return p->has_ep && !p->bd_fused ? 2 : 1;
    const int64_t n = p->batch * p->member_launches;
    return n > 0x7fffffffll ? 0x7fffffff : (int)n;
}

int qgemul_pack_batched(qgemul_plan* p, int operand, const void* src_dev, int64_t ld, int64_t member_stride, void* packed_dev)
{
    if (!p || p->batch < 1 || !src_dev || !packed_dev || (operand != QG_OPERAND_A && operand != QG_OPERAND_B)) return QG_EINVAL;
    const int64_t ext = member_extent(p->desc, operand, ld);
    if (ext < 1 || member_stride < ext) return QG_EINVAL;
    qgemul_plan* m = p->member;
    const int64_t eb = operand == QG_OPERAND_A ? p->ha.size : p->hb.size;
    if (!p->bd) {
        for (int64_t b = 0; b < p->batch; ++b)
            if (const int st = qgemul_pack(m, operand, (const char*)src_dev + b * member_stride * eb, ld, (char*)packed_dev + b * p->mstride[operand]); st != QG_OK) return st;
        return QG_OK;
    }
    QG_ON_DEVICE(p->ctx);
    const QOperandGeom g = operand_geom(m, operand, ld);
    const int check = (p->flags & QG_OPT_CHECK_RANGE) ? 1 : 0;
    if (check) QG_HIP(hipMemsetAsync(p->ctx->flag_dev, 0, 4, p->ctx->stream));
    QG_HIP(qg_launch_pack_stack(g, operand == QG_OPERAND_A ? m->pa : m->pb, operand == QG_OPERAND_A ? p->pa : p->pb, p->batch, src_dev, member_stride * eb,
                                packed_dev, check, p->ctx->flag_dev, p->ctx->stream, (p->flags & QG_OPT_GENERIC_LAYOUT) ? 1 : 0));
    if (check) {
        int flag = 0;
        QG_HIP(hipMemcpyAsync(&flag, p->ctx->flag_dev, 4, hipMemcpyDeviceToHost, p->ctx->stream));
        QG_HIP(hipStreamSynchronize(p->ctx->stream));
        if (flag) return QG_ERANGE;
    }
    return QG_OK;
}

int qgemul_unpack_c_batched(qgemul_plan* p, const void* packed_dev, void* dst_dev, int64_t ld, int64_t member_stride)
{
    if (!p || p->batch < 1 || !packed_dev || !dst_dev) return QG_EINVAL;
    const int64_t ext = member_extent(p->desc, QG_OPERAND_C, ld);
    if (ext < 1 || member_stride < ext) return QG_EINVAL;
    for (int64_t b = 0; b < p->batch; ++b)   // (a layout step: one launch per member, the members' packed Cs back to back)
        if (const int st = qgemul_unpack_c(p->member, (const char*)packed_dev + b * p->mstride[2], (char*)dst_dev + b * member_stride * p->hc.size, ld); st != QG_OK) return st;
    return QG_OK;
}

// the block-diagonal launch of a batched plan: the stack is a packed A and a packed B, with its own plane masks and row sums, and the
// member's conversion into C
static QMfmaArgs bd_mfma_args(const qgemul_plan* p, void* packedC, const void* packedA, const void* packedB, int cbytes)
{
    const qgemul_plan* m = p->member;
    QMfmaArgs a = mfma_args(p->pa, p->pb, p->variant, packedA, packedB, packedC, cbytes);
    a.to_c = m->an.lin.to_c[0];
    if (p->pa.offs) {   // centred operands: one centre per operand for the whole stack (centre_args)
        a.rsA = (const int64_t*)((const char*)packedA + p->pa.rowsum_off);
        a.rsB = (const int64_t*)((const char*)packedB + p->pb.rowsum_off);
        a.biasA = p->pa.bias;
        a.biasB = p->pb.bias;
        a.corr = (int64_t)((uint64_t)p->desc.K * (uint64_t)p->pa.bias * (uint64_t)p->pb.bias);
    }
    a.bd_tm = (int32_t)(m->pa.rows_p / p->cfg.TM);
    a.bd_tn = (int32_t)(m->pb.rows_p / p->cfg.TN);
    return a;
}

int qgemul_execute_batched(qgemul_plan* p, void* packedC, const void* packedA, const void* packedB)
{
    if (!p || p->batch < 1 || !packedC || !packedA || !packedB) return QG_EINVAL;
    if (p->has_ep) return QG_EINVAL;  // a batched plan with a chain runs through qgemul_execute_batched_ep
    if (p->desc.M == 0 || p->desc.N == 0) return QG_OK;
    qgemul_plan* m = p->member;
    if (!p->bd) {
        for (int64_t b = 0; b < p->batch; ++b)
            if (const int st = qgemul_execute(m, (char*)packedC + b * p->mstride[2], (const char*)packedA + b * p->mstride[0], (const char*)packedB + b * p->mstride[1]); st != QG_OK)
                return st;
        return QG_OK;
    }
    QG_ON_DEVICE(p->ctx);
    const QMfmaArgs a = bd_mfma_args(p, packedC, packedA, packedB, p->pc.cbytes);
    QG_HIP(qg_launch_mfma_bd(p->LA, p->LB, a, p->batch, p->ctx->stream));
    return QG_OK;
}

int qgemul_time_execute_batched(qgemul_plan* p, void* packedC, const void* packedA, const void* packedB, int warmup, int iters, float* avg_ms)
{
    if (p && p->has_ep) return QG_EINVAL;
    return time_execute(p, packedC, packedA, packedB, nullptr, warmup, iters, avg_ms, true);
}

// ---- element-wise chains on batched plans (include/qgemul.h): member b is Qgemul<...>(C_b, A_b, B_b) followed by the chain ----
// (ax == nullptr: a chain without APPROX stages)
static const qgemul_approx* const g_no_ax[QG_MAX_EW] = {};

int qgemul_classify_batched_epx(const qgemul_desc* d, int64_t batch, const qgemul_epilogue* ep, const qgemul_approx* const ax[QG_MAX_EW],
                                const qgemul_batched_ep* bep, uint32_t opt_flags, qgemul_info* out)
{
    if (!out || !ep) return QG_EINVAL;
    const EpView v = {ep, nullptr, nullptr, ax ? ax : g_no_ax};
    return classify_batched_view(d, batch, &v, bep, opt_flags, out, nullptr);
}

int qgemul_classify_batched_epx_launches(const qgemul_desc* d, int64_t batch, const qgemul_epilogue* ep, const qgemul_approx* const ax[QG_MAX_EW],
                                         const qgemul_batched_ep* bep, uint32_t opt_flags)
{
    if (!ep) return QG_EINVAL;
    const EpView v = {ep, nullptr, nullptr, ax ? ax : g_no_ax};
    int n = 0;
    const int st = classify_batched_view(d, batch, &v, bep, opt_flags, nullptr, &n);
    return st == QG_OK ? n : st;
}

int qgemul_plan_create_batched_epx(qgemul_ctx* c, const qgemul_desc* d, int64_t batch, const qgemul_epilogue* ep, const qgemul_approx* const ax[QG_MAX_EW],
                                   const qgemul_batched_ep* bep, uint32_t opt_flags, qgemul_plan** out)
{
    if (!c || !d || !ep || !out) return QG_EINVAL;
    const EpView v = {ep, nullptr, nullptr, ax ? ax : g_no_ax};
    return plan_create_batched_view(c, d, batch, &v, bep, opt_flags, out);
}

int qgemul_pack_e_batched(qgemul_plan* p, int stage, const void* src_dev, int64_t ld, int64_t member_stride, void* packed_dev)
{
    if (!p || p->batch < 1 || !p->has_ep || !src_dev || !packed_dev || stage < 0 || stage >= p->ept.n) return QG_EINVAL;
    if (!p->estride[stage]) return QG_EINVAL;   // a scalar or APPROX stage has no tensor operand
    const int64_t ext = member_extent(p->desc, QG_OPERAND_C, ld);
    if (ext < 1) return QG_EINVAL;
    if (p->e_shared[stage] ? member_stride != 0 : member_stride < ext) return QG_EINVAL;
    const qfmt f[2] = {p->ep.stage[stage].e, p->ep.stage[stage].e};
    const int64_t eb = qg_host_elem(f, 0).size;
    const int64_t n = p->e_shared[stage] ? 1 : p->batch;
    for (int64_t b = 0; b < n; ++b)   // (a layout step like qgemul_unpack_c_batched: one launch per member)
        if (const int st = qgemul_pack_e(p->member, stage, (const char*)src_dev + b * member_stride * eb, ld, (char*)packed_dev + b * p->estride[stage]); st != QG_OK) return st;
    return QG_OK;
}

int qgemul_execute_batched_ep(qgemul_plan* p, void* packedD, const void* packedA, const void* packedB, const qgemul_ep_args* args)
{
    if (!p || p->batch < 1 || !p->has_ep || !packedD || !packedA || !packedB) return QG_EINVAL;
    if (int s = ep_args_ok(p, args)) return s;
    if (p->desc.M == 0 || p->desc.N == 0) return QG_OK;
    qgemul_plan* m = p->member;
    if (!p->bd) {
        for (int64_t b = 0; b < p->batch; ++b) {
            qgemul_ep_args ma;
            memset(&ma, 0, sizeof ma);
            for (int k = 0; k < p->ept.n; ++k) {
                ma.e_scalar[k] = args->e_scalar[k];
                if (p->estride[k]) ma.e_packed[k] = (const char*)args->e_packed[k] + (p->e_shared[k] ? 0 : b * p->estride[k]);
            }
            if (const int st = qgemul_execute_ep(m, (char*)packedD + b * p->mstride[2], (const char*)packedA + b * p->mstride[0], (const char*)packedB + b * p->mstride[1], &ma); st != QG_OK)
                return st;
        }
        return QG_OK;
    }
    QG_ON_DEVICE(p->ctx);
    hipStream_t st = p->ctx->stream;
    QBdEp be;
    memset(&be, 0, sizeof be);
    be.msize = p->pc_c.Mp * p->pc_c.Np;
    for (int k = 0; k < p->ept.n; ++k)
        if (p->estride[k] && p->e_shared[k]) be.shared |= 1u << k;
    const QEpArgs ea = ep_device_args(p, args);
    if (p->bd_fused) {
        // ONE launch: the block-diagonal kernel's epilogue runs the chain on the value it has just converted into C's type
        QMfmaEpBdArgs a;
        memset(&a, 0, sizeof a);
        (QMfmaArgs&)a = bd_mfma_args(p, packedD, packedA, packedB, p->pc_c.cbytes);
        a.has_ep = 1;
        a.ep = p->ept;
        a.epa = ea;
        a.bd = be;
        QG_HIP(qg_launch_mfma_ep_bd(p->LA, p->LB, a, p->batch, st));
        return QG_OK;
    }
    // TWO launches: the block-diagonal kernel as it is into the plan's packed C of the whole stack, then ONE pass over the stack
    const QMfmaArgs a = bd_mfma_args(p, p->cwork, packedA, packedB, p->pc_c.cbytes);
    QG_HIP(qg_launch_mfma_bd(p->LA, p->LB, a, p->batch, st));
    QEltwiseArgs g;
    memset(&g, 0, sizeof g);
    g.C = (const char*)p->cwork;
    g.D = (char*)packedD;
    g.n = p->batch * be.msize;
    g.cbytes = p->pc_c.cbytes;
    g.t = p->ept;
    g.a = ea;
    if (p->has_ax) {
        QApproxBdArgs x;
        memset(&x, 0, sizeof x);
        x.x.g = g;
        for (int k = 0; k < QG_MAX_EW; ++k) x.x.ax[k] = m->ax_dev[k];
        x.x.force_general = (p->flags & QG_OPT_APPROX_GENERAL) ? 1 : 0;
        x.bd = be;
        QG_HIP(qg_launch_approx_bd(x, st));
        return QG_OK;
    }
    QEltwiseBdArgs e;
    memset(&e, 0, sizeof e);
    e.g = g;
    e.bd = be;
    QG_HIP(qg_launch_eltwise_bd(e, st));
    return QG_OK;
}

int qgemul_time_execute_batched_ep(qgemul_plan* p, void* packedD, const void* packedA, const void* packedB, const qgemul_ep_args* args, int warmup, int iters,
                                   float* avg_ms)
{
    if (!p || !p->has_ep) return QG_EINVAL;
    return time_execute(p, packedD, packedA, packedB, args, warmup, iters, avg_ms, true);
}


// ---- grouped Qgemul: GEMMs of different shapes in one launch (include/qgemul.h) ----
// the launch key: what the instantiation of k_mfma_grp and its uniform arguments depend on
static bool same_launch_key(const QPlanGeom& x, const QPlanGeom& y)
{
    return x.LA == y.LA && x.LB == y.LB && x.pa.limbs == y.pa.limbs && x.pb.limbs == y.pb.limbs && x.variant == y.variant && x.cfg.BK == y.cfg.BK &&
           x.pa.offs == y.pa.offs && x.pb.offs == y.pb.offs && x.pa.bias == y.pa.bias && x.pb.bias == y.pb.bias && x.pc.cbytes == y.pc.cbytes &&
           !memcmp(&x.an.lin.to_c[0], &y.an.lin.to_c[0], sizeof(QStep));
}

static bool grp_empty(const qgemul_desc& d) { return d.M == 0 || d.N == 0; }

// the geometry of a grouped plan, pure host code: b (zeroed) receives info and grp
static int grouped_geometry(const qgemul_desc* d, int64_t groups, uint32_t flags, qgemul_plan* b)
{
    if (!d || groups < 1 || groups > 0x7fffffffll) return QG_EINVAL;
    QGrouped* G = new (std::nothrow) QGrouped();
    if (!G) return QG_EINVAL;
    b->grp = G;
    b->batch = -1;
    b->flags = flags;
    b->desc = d[0];
    G->groups = groups;
    G->key = -1;
    G->m = new (std::nothrow) QGrpMember[groups]();
    G->ud = new (std::nothrow) qgemul_desc[groups];
    if (!G->m || !G->ud) return QG_EINVAL;
    // every distinct descriptor once (the comparison of the one-shot cache: qg_run_key.h)
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
        const int st = plan_geometry(&G->ud[u], flags, nullptr, groups, &G->ug[u], nullptr, nullptr);
        if (st != QG_OK) { b->info = G->ug[u].info; return st; }
    }
    auto eligible = [&](int64_t u) { return G->ug[u].bd && G->ug[u].pa.K_p >= G->ug[u].cfg.BK; };
    for (int64_t g = 0; g < groups && G->key < 0; ++g)
        if (eligible(G->m[g].uniq)) G->key = G->m[g].uniq;
    for (int64_t u = 0; u < G->n_uniq; ++u)
        G->u_in[u] = G->key >= 0 && eligible(u) && same_launch_key(G->ug[u], G->ug[G->key]);
    for (int64_t u = 0; u < G->n_uniq; ++u) {
        if (G->u_in[u]) continue;
        // a straggler runs on its own PLAIN plan
        G->ug[u] = QPlanGeom();
        const int st = plan_geometry(&G->ud[u], flags, nullptr, 0, &G->ug[u], nullptr, nullptr);
        if (st != QG_OK) { b->info = G->ug[u].info; return st; }
    }
    // layout: the members in the launch back to back, the launch's one trailer and one row-sum array, then the stragglers
    bool over = false;
    int64_t cur[3] = {0, 0, 0}, rows[2] = {0, 0}, tiles = 0;
    double ops = 0;
    for (int64_t g = 0; g < groups; ++g) {
        QGrpMember& m = G->m[g];
        const QPlanGeom& q = G->ug[m.uniq];
        ops += q.info.ops;
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
        rows[0] += q.pa.rows_p;
        rows[1] += q.pb.rows_p;
        tiles += (q.pa.rows_p / q.cfg.TM) * (q.pb.rows_p / q.cfg.TN);
        over |= rows[0] > 0x7fffffffll || rows[1] > 0x7fffffffll || tiles > 0x7fffffffll || q.pa.K_p / q.cfg.BK > 0x7fffffffll;
    }
    G->n_tiles = tiles;
    if (G->n_in && !over) {
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
                s.rowsum_off = round_up(cur[w], 256);
                cur[w] = s.rowsum_off + s.rows_p * 8;
            }
        }
        for (int64_t g = 0; g < groups; ++g) {
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
    }
    int64_t launches = G->n_in ? 1 : 0;
    for (int64_t g = 0; g < groups && !over; ++g) {
        QGrpMember& m = G->m[g];
        if (m.in_launch) continue;
        const QPlanGeom& q = G->ug[m.uniq];
        for (int w = 0; w < 3; ++w) {
            m.off[w] = round_up(cur[w], 256);
            m.bytes[w] = q.info.packed_bytes[w];
            over |= __builtin_add_overflow(m.off[w], m.bytes[w], &cur[w]) || cur[w] > (1ll << 60);
        }
        if (!grp_empty(G->ud[m.uniq])) launches += plan_launches(&q);
    }
    b->info = G->ug[G->key >= 0 ? G->key : G->m[0].uniq].info;
    if (over) {
        b->info.supported = 0;
        snprintf(b->info.reason, sizeof b->info.reason, "grouped plan: more than 2^31 - 1 tiles / packed operands beyond the address range");
        return QG_EINVAL;
    }
    G->launches = launches > 0x7fffffffll ? 0x7fffffff : (int)launches;
    for (int w = 0; w < 3; ++w) b->info.packed_bytes[w] = cur[w];
    b->info.ops = ops;
    snprintf(b->info.reason, sizeof b->info.reason, "grouped plan: %lld members in one launch (%lld 64x64 tiles), %lld run alone", (long long)G->n_in,
             (long long)G->n_tiles, (long long)(groups - G->n_in));
    // the schedule: one record per workgroup (qg_grp.h)
    if (G->n_tiles > 0) {
        const QPlanGeom& k = G->ug[G->key];
        QGrpShape* sh = new (std::nothrow) QGrpShape[G->n_in];
        int64_t* order = new (std::nothrow) int64_t[G->n_in];
        G->tiles = new (std::nothrow) QGrpTile[G->n_tiles];
        if (!sh || !order || !G->tiles) { delete[] sh; delete[] order; return QG_EINVAL; }
        int64_t n = 0;
        for (int64_t g = 0; g < groups; ++g) {
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
        delete[] sh;
        delete[] order;
    }
    return QG_OK;
}

int grouped_plan_new(const qgemul_desc* d, int64_t groups, uint32_t opt_flags, qgemul_plan** out)
{
    *out = nullptr;
    qgemul_plan* b = new (std::nothrow) qgemul_plan();
    if (!b) return QG_EINVAL;
    *out = b;
    return grouped_geometry(d, groups, opt_flags, b);
}

static void grouped_plan_drop(qgemul_plan* b)   // a plan that owns no device resource
{
    if (!b) return;
    delete b->grp;
    delete b;
}

static void grouped_member_out(const QGrouped* G, int64_t g, qgemul_grouped_member* out)
{
    const QGrpMember& m = G->m[g];
    const QPlanGeom& q = G->ug[m.uniq];
    memset(out, 0, sizeof *out);
    out->in_launch = m.in_launch;
    out->launches = m.in_launch || grp_empty(G->ud[m.uniq]) ? 0 : plan_launches(&q);
    for (int w = 0; w < 3; ++w) { out->off[w] = m.off[w]; out->bytes[w] = m.bytes[w]; }
    if (m.in_launch) {
        out->tiles_m = q.pa.rows_p / q.cfg.TM;
        out->tiles_n = q.pb.rows_p / q.cfg.TN;
        out->k_tiles = q.pa.K_p / q.cfg.BK;
    }
}

int qgemul_classify_grouped(const qgemul_desc* d, int64_t groups, uint32_t opt_flags, qgemul_info* out)
{
    if (!d || !out) return QG_EINVAL;
    qgemul_plan* b = nullptr;
    const int st = grouped_plan_new(d, groups, opt_flags, &b);
    if (b && groups >= 1) *out = b->info;
    grouped_plan_drop(b);
    return st;
}

int qgemul_classify_grouped_launches(const qgemul_desc* d, int64_t groups, uint32_t opt_flags)
{
    if (!d) return QG_EINVAL;
    qgemul_plan* b = nullptr;
    const int st = grouped_plan_new(d, groups, opt_flags, &b);
    const int n = st == QG_OK ? b->grp->launches : st;
    grouped_plan_drop(b);
    return n;
}

int qgemul_classify_grouped_member(const qgemul_desc* d, int64_t groups, uint32_t opt_flags, int64_t g, qgemul_grouped_member* out)
{
    if (!d || !out || g < 0 || g >= groups) return QG_EINVAL;
    qgemul_plan* b = nullptr;
    const int st = grouped_plan_new(d, groups, opt_flags, &b);
    if (st == QG_OK) grouped_member_out(b->grp, g, out);
    grouped_plan_drop(b);
    return st;
}

// every distinct descriptor's plain plan owns its device resources; the grouped plan owns the schedule on the device
int qgemul_plan_create_grouped(qgemul_ctx* c, const qgemul_desc* d, int64_t groups, uint32_t opt_flags, qgemul_plan** out)
{
    if (!c || !d || !out) return QG_EINVAL;
    qgemul_plan* b = nullptr;
    int st = grouped_plan_new(d, groups, opt_flags, &b);
    if (st != QG_OK) { grouped_plan_drop(b); return st; }
    b->ctx = c;
    QGrouped* G = b->grp;
    for (int64_t u = 0; u < G->n_uniq && st == QG_OK; ++u) st = plan_create_view(c, &G->ud[u], nullptr, opt_flags, &G->up[u], G->u_in[u] ? groups : 0);
    if (st == QG_OK && G->n_tiles > 0) {
        DeviceScope scope(c->device);
        const size_t tb = (size_t)G->n_tiles * sizeof(QGrpTile);
        hipError_t e = scope.err;
        if (e == hipSuccess) e = hipMalloc((void**)&G->tiles_dev, tb);
        if (e == hipSuccess) e = hipMemcpyAsync(G->tiles_dev, G->tiles, tb, hipMemcpyHostToDevice, c->stream);
        if (e == hipSuccess) e = hipStreamSynchronize(c->stream);
        if (e != hipSuccess) { g_last_hip = (int)e; st = QG_EHIP; }
    }
    if (st != QG_OK) { qgemul_plan_destroy(b); return st; }
    *out = b;
    return QG_OK;
}

int qgemul_plan_grouped_launches(const qgemul_plan* p)
{
    if (!p || !p->grp) return QG_EINVAL;
    return p->grp->launches;
}

int qgemul_plan_grouped_member(const qgemul_plan* p, int64_t g, qgemul_grouped_member* out)
{
    if (!p || !p->grp || !out || g < 0 || g >= p->grp->groups) return QG_EINVAL;
    grouped_member_out(p->grp, g, out);
    return QG_OK;
}

int qgemul_pack_grouped(qgemul_plan* p, int operand, const void* const* src_dev, const int64_t* ld, void* packed_dev)
{
    if (!p || !p->grp || !src_dev || !packed_dev || (operand != QG_OPERAND_A && operand != QG_OPERAND_B)) return QG_EINVAL;
    const QGrouped* G = p->grp;
    for (int64_t g = 0; g < G->groups; ++g) {   // every member is checked before the first launch
        const qgemul_desc& d = G->ud[G->m[g].uniq];
        if (grp_empty(d)) continue;
        if (!src_dev[g] || member_extent(d, operand, ld ? ld[g] : 0) < 1) return QG_EINVAL;
    }
    QG_ON_DEVICE(p->ctx);
    hipStream_t st = p->ctx->stream;
    const int check = (p->flags & QG_OPT_CHECK_RANGE) ? 1 : 0;
    const QPackedGeom& s = operand == QG_OPERAND_A ? G->sa : G->sb;
    if (G->n_in) {
        // what belongs to the launch is cleared ONCE; every member then ORs / adds into it (qg_launch_pack_stack does the same)
        if (check) QG_HIP(hipMemsetAsync(p->ctx->flag_dev, 0, 4, st));
        if (s.trailer) QG_HIP(hipMemsetAsync((char*)packed_dev + s.trailer, 0, QG_TRAILER_BYTES, st));
        if (s.offs && s.rows_p) QG_HIP(hipMemsetAsync((char*)packed_dev + s.rowsum_off, 0, (size_t)s.rows_p * 8, st));
        for (int64_t g = 0; g < G->groups; ++g) {
            const QGrpMember& m = G->m[g];
            if (!m.in_launch || grp_empty(G->ud[m.uniq])) continue;
            const QOperandGeom og = operand_geom(G->up[m.uniq], operand, ld ? ld[g] : 0);
            QG_HIP(qg_launch_pack_member(og, operand == QG_OPERAND_A ? m.pa : m.pb, src_dev[g], (char*)packed_dev + m.off[operand], check, p->ctx->flag_dev, st,
                                         (p->flags & QG_OPT_GENERIC_LAYOUT) ? 1 : 0));
        }
        if (check) {
            int flag = 0;
            QG_HIP(hipMemcpyAsync(&flag, p->ctx->flag_dev, 4, hipMemcpyDeviceToHost, st));
            QG_HIP(hipStreamSynchronize(st));
            if (flag) return QG_ERANGE;
        }
    }
    for (int64_t g = 0; g < G->groups; ++g) {
        const QGrpMember& m = G->m[g];
        if (m.in_launch || grp_empty(G->ud[m.uniq])) continue;
        if (const int rc = qgemul_pack(G->up[m.uniq], operand, src_dev[g], ld ? ld[g] : 0, (char*)packed_dev + m.off[operand]); rc != QG_OK) return rc;
    }
    return QG_OK;
}

int qgemul_unpack_c_grouped(qgemul_plan* p, const void* packed_dev, void* const* dst_dev, const int64_t* ld)
{
    if (!p || !p->grp || !packed_dev || !dst_dev) return QG_EINVAL;
    const QGrouped* G = p->grp;
    for (int64_t g = 0; g < G->groups; ++g) {
        const qgemul_desc& d = G->ud[G->m[g].uniq];
        if (grp_empty(d)) continue;
        if (!dst_dev[g] || member_extent(d, QG_OPERAND_C, ld ? ld[g] : 0) < 1) return QG_EINVAL;
    }
    for (int64_t g = 0; g < G->groups; ++g) {   // (a layout step: one launch per member)
        const QGrpMember& m = G->m[g];
        if (grp_empty(G->ud[m.uniq])) continue;
        if (const int rc = qgemul_unpack_c(G->up[m.uniq], (const char*)packed_dev + m.off[2], dst_dev[g], ld ? ld[g] : 0); rc != QG_OK) return rc;
    }
    return QG_OK;
}

int qgemul_execute_grouped(qgemul_plan* p, void* packedC, const void* packedA, const void* packedB)
{
    if (!p || !p->grp || !packedC || !packedA || !packedB) return QG_EINVAL;
    const QGrouped* G = p->grp;
    if (G->n_tiles > 0) {
        QG_ON_DEVICE(p->ctx);
        const QPlanGeom& k = G->ug[G->key];
        QMfmaGrpArgs a;
        memset((void*)&a, 0, sizeof a);
        (QMfmaArgs&)a = mfma_args(G->sa, G->sb, k.variant, packedA, packedB, packedC, k.pc.cbytes);
        a.to_c = k.an.lin.to_c[0];
        if (G->sa.offs) {   // centred operands: one centre per operand for the whole launch, K biasA biasB per member (the records)
            a.rsA = (const int64_t*)((const char*)packedA + G->sa.rowsum_off);
            a.rsB = (const int64_t*)((const char*)packedB + G->sb.rowsum_off);
            a.biasA = G->sa.bias;
            a.biasB = G->sb.bias;
        }
        a.tiles = G->tiles_dev;
        QG_HIP(qg_launch_mfma_grp(k.LA, k.LB, a, G->n_tiles, p->ctx->stream));
    }
    for (int64_t g = 0; g < G->groups; ++g) {
        const QGrpMember& m = G->m[g];
        if (m.in_launch) continue;
        if (const int rc = qgemul_execute(G->up[m.uniq], (char*)packedC + m.off[2], (const char*)packedA + m.off[0], (const char*)packedB + m.off[1]); rc != QG_OK)
            return rc;
    }
    return QG_OK;
}

int qgemul_time_execute_grouped(qgemul_plan* p, void* packedC, const void* packedA, const void* packedB, int warmup, int iters, float* avg_ms)
{
    return time_execute(p, packedC, packedA, packedB, nullptr, warmup, iters, avg_ms, 2);
}

} // extern "C"
