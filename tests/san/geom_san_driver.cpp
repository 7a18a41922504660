// TEST INFRASTRUCTURE: the plan geometry (qublas_amd/csrc/qg_geom.cpp on qg_plan.cpp) compiled for the CPU with AddressSanitizer +
// UndefinedBehaviorSanitizer and driven with queries read from stdin (tests/geom_sweep.py: pack_query).  A query is a header
//   uint32 kind (0 plain, 1 batched, 2 grouped), uint32 flags, int64 n (batch / groups), uint32 chain, uint32 reserved
// followed by n descriptors (grouped) or one, and the chain: 1 / 3 a qgemul_epilogue (qgemul_classify_ep / _epx: the latter with
// uint8 on[QG_MAX_EW] and the qgemul_approx tables that are on), then for a batched query a qgemul_batched_ep; 2 / 4 a
// qgemul_epilogue_cplx (qgemul_classify_epc / _epcx: the latter with uint8 on[QG_MAX_EW] and the qgemul_cmul records that are on).
// Prints one line of key=value fields per query (grouped: one more per member and per tile record); any sanitizer report fails the
// run.  No GPU code is involved.
#include <stdio.h>
#include <string.h>

#include <vector>

#include "../../qublas_amd/csrc/qg_geom.h"

struct Reader {
    std::vector<unsigned char> buf;
    size_t at = 0;
    template <class T>
    bool get(T* out, size_t n = 1)
    {
        if (at + n * sizeof(T) > buf.size()) return false;
        memcpy((void*)out, buf.data() + at, n * sizeof(T));
        at += n * sizeof(T);
        return true;
    }
};
struct Header { uint32_t kind, flags; int64_t n; uint32_t chain, reserved; };

static void print_info(int st, const qgemul_info& i)
{
    printf("st=%d sup=%d cls=%d kernel=%d limbs=%d,%d max_bits=%d in_bits=%d,%d packed=%lld,%lld,%lld ops=%.17g heb=%d,%d,%d hio=%d,%d,%d", st, i.supported, i.cls, i.kernel,
           i.limbs[0], i.limbs[1], i.max_bits, i.in_bits[0], i.in_bits[1], (long long)i.packed_bytes[0], (long long)i.packed_bytes[1], (long long)i.packed_bytes[2], i.ops,
           i.host_elem_bytes[0], i.host_elem_bytes[1], i.host_elem_bytes[2], i.host_imag_off[0], i.host_imag_off[1], i.host_imag_off[2]);
}
static void print_packed(const char* name, const QPackedGeom& g)
{
    printf(" %s=%lld,%lld,%d,%d,%d,%d,%lld,%d,%d,%d,%lld,%lld", name, (long long)g.rows_p, (long long)g.K_p, g.cbytes, g.limbs, g.tr, g.bk, (long long)g.trailer, g.digit6, g.limb0, g.offs,
           (long long)g.bias, (long long)g.rowsum_off);
}
static void print_c(const char* name, const QCGeom& c)
{
    printf(" %s=%lld,%lld,%lld,%lld,%d,%d,%d,%d,%lld,%d,%d,%d,%d,%d", name, (long long)c.M, (long long)c.N, (long long)c.Mp, (long long)c.Np, c.tm, c.tn, c.cbytes, c.parts, (long long)c.ldc,
           c.elem_bytes, c.off[0], c.off[1], c.sb[0], c.sb[1]);
}
static void print_geom(const QPlanGeom& g)
{
    printf(" cfg=%d,%d,%d,%d LA=%d LB=%d bd=%d", g.cfg.variant, g.cfg.TM, g.cfg.TN, g.cfg.BK, g.LA, g.LB, g.bd);
    print_packed("pa", g.pa);
    print_packed("pb", g.pb);
    print_c("pc", g.pc);
    print_c("pc_c", g.pc_c);
    const QComposite& q = g.comp;
    printf(" comp=%d,%d,%d,%d,%lld,%d,%d,%lld,%lld", q.on, q.ga, q.gb, q.nc, (long long)q.kc, q.slab_bytes, q.wide, (long long)q.chunk_bytes[0], (long long)q.chunk_bytes[1]);
    for (int i = 0; i < 3; ++i) printf(";%d,%d,%d,%d,%d,%d,%d", q.la[i], q.lb[i], q.la0[i], q.lb0[i], q.var[i][0], q.var[i][1], q.var[i][2]);
    printf(" ept=%d,%d,%d,%d wide_ep=%d launches=%d", g.ept.n, g.ept.dbytes, g.ept.bits32, g.ept_im.n, qg_wide_epilogue(&g) ? 1 : 0, qg_plan_launches(&g));
}
// the centred retreat of a wide plan: centring would have saved a limb, the plan is wide, on the MFMA kernels and not centred
static int retreated(const qgemul_desc& d, uint32_t flags, const QPlanGeom& g)
{
    if (g.an.status != QG_OK || !g.an.wide || !g.an.linear_ok || g.an.ring_ok || d.is_complex || (flags & (QG_OPT_FORCE_TREE | QG_OPT_BALANCED_LIMBS))) return 0;
    if (g.info.kernel != QG_KERNEL_MFMA_I8 && g.info.kernel != QG_KERNEL_MFMA_I8_LIMB) return 0;
    int64_t c = 0;
    const bool saves = qg_limbs_centred(d.a[0], &c) < qg_limbs_for(d.a[0]) || qg_limbs_centred(d.b[0], &c) < qg_limbs_for(d.b[0]);
    return saves && !g.pa.offs ? 1 : 0;
}

int main()
{
    Reader r;
    unsigned char tmp[65536];
    size_t n;
    while ((n = fread(tmp, 1, sizeof tmp, stdin)) > 0) r.buf.insert(r.buf.end(), tmp, tmp + n);
    size_t count = 0;
    Header h;
    QPlanGeom* g = new QPlanGeom[2];
    while (r.get(&h)) {
        if (h.kind > 2 || h.chain > 4 || h.n < (h.kind == 2 ? 1 : 0) || h.n > (h.kind == 2 ? 4096 : INT64_MAX)) { fprintf(stderr, "query %zu: bad header\n", count); return 2; }
        std::vector<qgemul_desc> d(h.kind == 2 ? (size_t)h.n : 1);
        if (!r.get(d.data(), d.size())) return 2;
        qgemul_epilogue ep;
        qgemul_epilogue_cplx epc;
        qgemul_batched_ep bep;
        uint8_t on[QG_MAX_EW] = {};
        std::vector<qgemul_approx> ax(QG_MAX_EW);
        qgemul_cmul cx[QG_MAX_EW];
        const qgemul_approx* axp[QG_MAX_EW] = {};
        const qgemul_cmul* cxp[QG_MAX_EW] = {};
        memset(&bep, 0, sizeof bep);
        EpView v = {};
        if (h.chain == 1 || h.chain == 3) {
            if (!r.get(&ep)) return 2;
            v.re = &ep;
            if (h.chain == 3) {
                if (!r.get(on, QG_MAX_EW)) return 2;
                for (int k = 0; k < QG_MAX_EW; ++k)
                    if (on[k]) { if (!r.get(&ax[k])) return 2; axp[k] = &ax[k]; }
                v.ax = axp;
            }
            if (h.kind == 1 && !r.get(&bep)) return 2;
        } else if (h.chain) {
            if (!r.get(&epc)) return 2;
            v.re = &epc.part[0];
            v.im = &epc.part[1];
            v.e_cplx = epc.e_complex;
            if (h.chain == 4) {
                if (!r.get(on, QG_MAX_EW)) return 2;
                for (int k = 0; k < QG_MAX_EW; ++k)
                    if (on[k]) { if (!r.get(&cx[k])) return 2; cxp[k] = &cx[k]; }
                v.epc = &epc;
                v.cx = cxp;
            }
        }
        const EpView* ev = h.chain ? &v : nullptr;
        printf("%zu kind=%u ", count++, h.kind);
        g[0] = QPlanGeom();
        g[1] = QPlanGeom();
        if (h.kind == 0) {
            const int st = qg_plan_geometry(&d[0], h.flags, ev, 0, &g[0], nullptr, nullptr);
            print_info(st, g[0].info);
            if (st == QG_OK) {
                print_geom(g[0]);
                bool has_ax = false;
                for (int k = 0; k < QG_MAX_EW; ++k) has_ax |= axp[k] != nullptr;
                printf(" fuses=%d retreat=%d", ev && qg_fuses_epilogue(&g[0], h.flags, has_ax, qg_view_has_cmul(ev)) ? 1 : 0, retreated(d[0], h.flags, g[0]));
            }
            printf(" reason=%s\n", g[0].info.reason);
        } else if (h.kind == 1) {
            QBatchGeom b = {};
            const int st = qg_batched_geometry(&d[0], h.n, h.flags, ev, &bep, &g[0], &g[1], &b);
            print_info(st, g[1].info);
            if (st == QG_OK) {
                print_geom(g[0]);
                print_packed("spa", g[1].pa);
                print_packed("spb", g[1].pb);
                printf(" mstride=%lld,%lld,%lld bd_fused=%d member_launches=%d blaunches=%d", (long long)b.mstride[0], (long long)b.mstride[1], (long long)b.mstride[2], b.bd_fused,
                       b.member_launches, qg_batched_launches(&g[1], &b, ev != nullptr));
                for (int k = 0; k < QG_MAX_EW; ++k) printf(" e%d=%d,%lld", k, b.e_shared[k], (long long)b.estride[k]);
            }
            printf(" reason=%s\n", g[1].info.reason);
        } else {
            QGrouped G{};
            qgemul_info info;
            memset(&info, 0, sizeof info);
            const int st = qg_grouped_geometry(d.data(), h.n, h.flags, &G, &info);
            print_info(st, info);
            if (st == QG_OK) {
                printf(" n_uniq=%lld n_in=%lld n_tiles=%lld key=%lld glaunches=%d", (long long)G.n_uniq, (long long)G.n_in, (long long)G.n_tiles, (long long)G.key, G.launches);
                print_packed("sa", G.sa);
                print_packed("sb", G.sb);
            }
            printf(" reason=%s\n", info.reason);
            for (int64_t m = 0; st == QG_OK && m < G.groups; ++m) {
                qgemul_grouped_member o;
                qg_grouped_member_out(&G, m, &o);
                printf("  member %lld in=%d launches=%d off=%lld,%lld,%lld bytes=%lld,%lld,%lld tiles=%lld,%lld,%lld uniq=%d rows=%lld,%lld", (long long)m, o.in_launch, o.launches,
                       (long long)o.off[0], (long long)o.off[1], (long long)o.off[2], (long long)o.bytes[0], (long long)o.bytes[1], (long long)o.bytes[2], (long long)o.tiles_m,
                       (long long)o.tiles_n, (long long)o.k_tiles, G.m[m].uniq, (long long)G.m[m].row_a, (long long)G.m[m].row_b);
                if (o.in_launch) { print_packed("pa", G.m[m].pa); print_packed("pb", G.m[m].pb); }
                printf("\n");
            }
            for (int64_t t = 0; st == QG_OK && t < G.n_tiles; ++t) {
                const unsigned char* p = (const unsigned char*)&G.tiles[t];
                printf("  tile %lld ", (long long)t);
                for (size_t i = 0; i < sizeof(QGrpTile); ++i) printf("%02x", p[i]);
                printf("\n");
            }
        }
    }
    delete[] g;
    if (r.at != r.buf.size()) { fprintf(stderr, "trailing bytes after query %zu\n", count); return 2; }
    fprintf(stderr, "answered %zu queries\n", count);
    return 0;
}
