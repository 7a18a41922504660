// TEST INFRASTRUCTURE: the host-side planner (qublas_amd/csrc/qg_plan.cpp — interval propagation, class L / class T, lowering of
// the element-wise chain) compiled for the CPU with AddressSanitizer + UndefinedBehaviorSanitizer, as the reference compiles its
// own tests (CMakeLists.txt:17,26), and driven with descriptors read from stdin: the raw bytes of qgemul_desc structs (and,
// after each, one qgemul_epilogue).  Prints status, class, kernel-selection flags and the tree kernel / step form
// the plan flags resolve to (qg_tree_choice) per descriptor; any sanitizer report
// fails the run.  No GPU code is involved.
//
// --digest: every byte the planner writes, as a hash.  stdin is a sequence of records
//   uint32 chain (0 none, 3 a real chain, 4 a complex chain), qgemul_desc,
//   chain 3: qgemul_epilogue, uint8 on[QG_MAX_EW], the qgemul_approx tables that are on    (qg_analyze_epx on the descriptor's C)
//   chain 4: qgemul_epilogue_cplx, uint8 on[QG_MAX_EW], the qgemul_cmul records that are on (qg_analyze_epcx)
// Each output struct is filled with 0xAB before the call.  Per record: index, status, the 64-bit FNV-1a hash of the whole QAnalysis
// and, for a chain, the status and the hash of its tables; then what the corpus covered (tests/test_plan_digest.py) and one hash
// folded over all of them.  Two builds of the planner that print the same lines wrote the same bytes.
#include <stdio.h>
#include <string.h>

#include <vector>

#include "../../qublas_amd/csrc/qg_plan.h"
#include "../../qublas_amd/csrc/qg_approx.h"
#include "../../qublas_amd/csrc/qg_cmul.h"

namespace {

struct Fnv {
    uint64_t h = 1469598103934665603ull;
    void add(const void* p, size_t n)
    {
        const unsigned char* b = (const unsigned char*)p;
        for (size_t i = 0; i < n; ++i) { h ^= b[i]; h *= 1099511628211ull; }
    }
};
template <class T> uint64_t fnv_of(const T& v) { Fnv f; f.add(&v, sizeof v); return f.h; }

struct Reader {
    std::vector<unsigned char> buf;
    size_t pos = 0;
    template <class T> bool get(T* out, size_t n = 1)
    {
        if (pos + n * sizeof(T) > buf.size()) return false;
        memcpy((void*)out, buf.data() + pos, n * sizeof(T));
        pos += n * sizeof(T);
        return true;
    }
};

// what the corpus reached (descriptors the planner accepted, unless said otherwise)
struct Coverage {
    long status[3] = {0, 0, 0};   // QG_OK, QG_EINVAL, QG_EUNSUPPORTED
    long tree[32] = {}, gemv[8] = {}, cplx[16] = {};
    long wide = 0, band = 0, generic_only = 0, ring = 0, real_a = 0, real_b = 0, tf = 0, basic = 0, copy0_odd = 0, artefact_c = 0, split = 0, biased_fallback = 0,
         uniform_basic = 0, chain_real = 0, chain_cplx = 0;
    static bool plain_rounding(const QStep& q) { return q.identity || q.d <= 0 || q.Q == QG_RND_POS_INF || q.Q == QG_RND_NEG_INF || q.Q == QG_TRN_TCPL; }
    void note(const qgemul_desc& d, const QAnalysis& an)
    {
        ++status[an.status == QG_OK ? 0 : an.status == QG_EINVAL ? 1 : 2];
        if (an.status != QG_OK) return;
        ++tree[(int)an.tree_form & 31];
        ++gemv[(int)an.gemv_form & 7];
        ++cplx[(int)an.cplx_form & 15];
        wide += an.wide != 0;
        band += an.band != 0;
        generic_only += an.generic_only != 0;
        ring += an.ring_ok != 0;
        real_a += d.cmul == QG_CMUL_REAL_A;
        real_b += d.cmul == QG_CMUL_REAL_B;
        tf += d.cmul == QG_CMUL_TF;
        basic += d.cmul == QG_CMUL_BASIC;
        copy0_odd += (d.flags & QG_DESC_LEFTOVER0_COPY) && (d.K & 1) && d.K > 1;
        for (int p = 0; p < (d.is_complex ? 2 : 1); ++p)
            artefact_c += (d.flags & QG_DESC_REFERENCE_ARTEFACTS) && d.c[p].O == QG_WRP_TCPL && !d.c[p].S && (int)d.c[p].I + (int)d.c[p].F == 32;
        split += an.split_s > 0;
        // QTF_REC_KINDS although no step rounds by a value-dependent mode: the biased records did not fit and the unbiased ones stand
        bool plain = an.tree_form == QTF_REC_KINDS && plain_rounding(an.tree.mul[0].q);
        for (int l = 0; l < an.tree.n_levels_k && plain; ++l) plain = plain_rounding(an.tree.level_add[0][l].q);
        biased_fallback += plain;
        uniform_basic += an.cplx_form == QCF_UNIFORM && d.cmul == QG_CMUL_BASIC;
    }
    static void list(const char* name, const long* n, int len)
    {
        printf("%s", name);
        for (int i = 0; i < len; ++i)
            if (n[i]) printf(" %d:%ld", i, n[i]);
        printf("\n");
    }
    void print() const
    {
        printf("status ok=%ld einval=%ld eunsupported=%ld\n", status[0], status[1], status[2]);
        list("tree_forms", tree, 32);
        list("gemv_forms", gemv, 8);
        list("cplx_forms", cplx, 16);
        printf("covered wide=%ld band=%ld generic_only=%ld ring_ok=%ld real_a=%ld real_b=%ld cmul_tf=%ld cmul_basic=%ld leftover0_copy_odd_k=%ld artefact_rewrites_c=%ld "
               "split_s=%ld biased_fallback=%ld uniform_basic=%ld real_chains=%ld cplx_chains=%ld\n",
               wide, band, generic_only, ring, real_a, real_b, tf, basic, copy0_odd, artefact_c, split, biased_fallback, uniform_basic, chain_real, chain_cplx);
    }
};

int digest()
{
    Reader r;
    unsigned char tmp[65536];
    size_t n;
    while ((n = fread(tmp, 1, sizeof tmp, stdin)) > 0) r.buf.insert(r.buf.end(), tmp, tmp + n);
    Coverage cov;
    Fnv all;
    size_t count = 0;
    uint32_t chain;
    QAnalysis* an = new QAnalysis;
    std::vector<QApproxTable> axt(QG_MAX_EW);
    for (; r.get(&chain); ++count) {
        qgemul_desc d;
        if (chain > 4 || chain == 1 || chain == 2 || !r.get(&d)) { fprintf(stderr, "record %zu: bad header\n", count); return 2; }
        memset((void*)an, 0xAB, sizeof *an);
        qg_analyze(&d, an);
        cov.note(d, *an);
        const uint64_t h = fnv_of(*an);
        all.add(&h, sizeof h);
        printf("%zu %d %016llx", count, an->status, (unsigned long long)h);
        uint8_t on[QG_MAX_EW];
        char why[96];
        int bits = -1, st = 0;
        Fnv c;
        memset(why, 0xAB, sizeof why);
        if (chain == 3) {
            qgemul_epilogue ep;
            std::vector<qgemul_approx> ax(QG_MAX_EW);
            const qgemul_approx* axp[QG_MAX_EW] = {};
            if (!r.get(&ep) || !r.get(on, QG_MAX_EW)) return 2;
            for (int k = 0; k < QG_MAX_EW; ++k)
                if (on[k]) { if (!r.get(&ax[k])) return 2; axp[k] = &ax[k]; }
            QEpTable t;
            memset((void*)&t, 0xAB, sizeof t);
            memset((void*)axt.data(), 0xAB, QG_MAX_EW * sizeof(QApproxTable));
            st = qg_analyze_epx(d.c[0], &ep, axp, &t, axt.data(), &bits, why, sizeof why);
            c.add(&t, sizeof t);
            c.add(axt.data(), QG_MAX_EW * sizeof(QApproxTable));
            ++cov.chain_real;
        } else if (chain == 4) {
            qgemul_epilogue_cplx epc;
            qgemul_cmul cx[QG_MAX_EW];
            const qgemul_cmul* cxp[QG_MAX_EW] = {};
            if (!r.get(&epc) || !r.get(on, QG_MAX_EW)) return 2;
            for (int k = 0; k < QG_MAX_EW; ++k)
                if (on[k]) { if (!r.get(&cx[k])) return 2; cxp[k] = &cx[k]; }
            QEpTable t[2];
            QCmulStage cmt[QG_MAX_EW];
            memset((void*)t, 0xAB, sizeof t);
            memset((void*)cmt, 0xAB, sizeof cmt);
            st = qg_analyze_epcx(d.c, &epc, cxp, t, cmt, &bits, why, sizeof why);
            c.add(t, sizeof t);
            c.add(cmt, sizeof cmt);
            ++cov.chain_cplx;
        }
        if (chain) {
            c.add(&bits, sizeof bits);
            c.add(why, strnlen(why, sizeof why));
            all.add(&st, sizeof st);
            all.add(&c.h, sizeof c.h);
            printf(" chain %d %016llx", st, (unsigned long long)c.h);
        }
        printf("\n");
    }
    delete an;
    if (r.pos != r.buf.size()) { fprintf(stderr, "trailing bytes after record %zu\n", count); return 2; }
    cov.print();
    printf("digest %zu %016llx\n", count, (unsigned long long)all.h);
    return 0;
}

} // namespace

int main(int argc, char** argv)
{
    if (argc > 1 && !strcmp(argv[1], "--digest")) return digest();
    std::vector<unsigned char> buf;
    unsigned char tmp[65536];
    size_t n;
    while ((n = fread(tmp, 1, sizeof tmp, stdin)) > 0) buf.insert(buf.end(), tmp, tmp + n);
    const size_t rec = sizeof(qgemul_desc) + sizeof(qgemul_epilogue);
    size_t count = 0;
    for (size_t off = 0; off + rec <= buf.size(); off += rec, ++count) {
        qgemul_desc d;
        qgemul_epilogue ep;
        memcpy(&d, buf.data() + off, sizeof d);
        memcpy(&ep, buf.data() + off + sizeof d, sizeof ep);
        QAnalysis* an = new QAnalysis;
        qg_analyze(&d, an);
        int ep_st = -99, ep_bits = 0;
        if (an->status == QG_OK && !d.is_complex && ep.n_stages <= QG_MAX_EW) {
            QEpTable t;
            char why[96];
            ep_st = qg_analyze_ep(d.c[0], &ep, &t, &ep_bits, why, sizeof why);
        }
        printf("%zu %d %d %d %d %d %d %d %d %d", count, an->status, an->cls, an->max_bits, an->linear_ok ? 1 : 0, an->tree_fast_ok ? 1 : 0, ep_st,
               an->status == QG_OK ? (int)an->tree_form : -1, an->status == QG_OK ? (int)an->cplx_form : -1, an->status == QG_OK ? (int)an->gemv_form : -1);
        // the tree kernel and the name of its step form under plan flags 0, QG_OPT_RUNTIME_MODES, QG_OPT_GENERIC_TREE (qg_tree_choice)
        for (uint32_t flags : {0u, (uint32_t)QG_OPT_RUNTIME_MODES, (uint32_t)QG_OPT_GENERIC_TREE}) {
            if (an->status != QG_OK) { printf("|-1 -"); continue; }
            const QTreeChoice c = qg_tree_choice(an, &d, flags, true);
            const char* name = c.kernel == QG_KERNEL_TREE_I32 ? qg_form_name(c.tree) : c.kernel == QG_KERNEL_GEMV_I32 ? qg_form_name(c.gemv)
                             : c.kernel == QG_KERNEL_TREE_CPLX_I32 ? qg_form_name(c.cplx) : "-";
            printf("|%d %s", c.kernel, name);
        }
        printf("\n");
        delete an;
    }
    fprintf(stderr, "analysed %zu descriptors\n", count);
    return 0;
}
