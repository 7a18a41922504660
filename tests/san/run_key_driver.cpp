// The one-shot calls' plan key (qublas_amd/csrc/qg_run_key.h) on its own, under AddressSanitizer + UndefinedBehaviorSanitizer
// (tests/test_run_key.py builds and runs this).  One descriptor and one group of three, every kind of request an entry point of
// qgemul_run* can make.
#include <stdio.h>

#include "../../qublas_amd/csrc/qg_run_key.h"

static qfmt fmt(int I, int F, int S, int Q, int O)
{
    qfmt f;
    memset(&f, 0, sizeof f);
    f.I = (int16_t)I; f.F = (int16_t)F; f.S = (uint8_t)S; f.Q = (uint8_t)Q; f.O = (uint8_t)O;
    return f;
}
// field by field, so that the destination's padding / reserved bytes keep the poison
static void put(qfmt& dst, qfmt v) { dst.I = v.I; dst.F = v.F; dst.S = v.S; dst.Q = v.Q; dst.O = v.O; }

// every public struct a request is made of.  fill(): the whole object is `poison` bytes first, then the meaningful fields are
// assigned one by one — padding, reserved bytes and the entries beyond n_levels / n_stages / n_seg / n_coef keep the poison
struct Inputs {
    qgemul_desc d;
    qgemul_desc g[3];              // the members of a group: d's formats at three shapes, g[0] = d
    qgemul_epilogue ep;
    qgemul_approx t1, t2;          // t2: one coefficient differs
    qgemul_epilogue_cplx epc;
    qgemul_cmul basic, tf;
    qgemul_batched_ep shared, per_member, shared0;   // shared0: the bit pattern of per0 below
    qgemul_grouped_ep per_none, per0;                // no scalar stage per member; stage 0 per member

    void fill(int poison)
    {
        memset((void*)this, poison, sizeof *this);
        desc(d, 65, 33, 100);
        desc(g[0], 65, 33, 100);
        desc(g[1], 3, 5, 7);
        desc(g[2], 33, 17, 64);
        chain(ep, 0);
        chain(epc.part[0], 0);
        chain(epc.part[1], 1);
        for (uint32_t k = 0; k < ep.n_stages; ++k) epc.e_complex[k] = k == 1;
        table(t1, 3);
        table(t2, 4);
        basic.cmul = QG_CMUL_BASIC;
        tf.cmul = QG_CMUL_TF;
        for (int i = 0; i < 8; ++i) { put(basic.mul[i], fmt(10 + i, 6, 1, 5, 0)); put(tf.mul[i], fmt(10 + i, 6, 1, 5, 0)); }
        for (int k = 0; k < QG_MAX_EW; ++k) {
            shared.e_shared[k] = k == 1; per_member.e_shared[k] = 0; shared0.e_shared[k] = k == 0;
            per_none.scalar_per_member[k] = 0; per0.scalar_per_member[k] = k == 0;
        }
    }
    static void desc(qgemul_desc& d, int64_t M, int64_t N, int64_t K)
    {
        d.abi = QGEMUL_ABI_VERSION; d.transA = 0; d.is_complex = 0; d.cmul = QG_CMUL_NONE; d.flags = 0;
        d.M = M; d.N = N; d.K = K; d.n_levels = 7;
        for (int p = 0; p < 2; ++p) {
            put(d.a[p], fmt(7, 8, 1, 5, 0)); put(d.b[p], fmt(7, 8, 1, 5, 0)); put(d.c[p], fmt(12, 8, 1, 5, 0));
            for (uint32_t l = 0; l < d.n_levels; ++l) { put(d.level_add[p][l], fmt(20 + (int)l, 10, 1, 5, 0)); put(d.level[p][l], fmt(21 + (int)l, 10, 1, 5, 0)); }
        }
        for (int i = 0; i < 8; ++i) put(d.mul[i], fmt(14 + i, 16, 1, 5, 0));
    }
    // MUL by a scalar, ADD of a tensor, then a third stage (the one that carries a table or a record in the kinds that have one)
    static void chain(qgemul_epilogue& e, int part)
    {
        e.n_stages = 3;
        put(e.d, fmt(9, 6 + part, 1, 5, 0));
        const uint8_t ops[3] = {QG_EW_MUL, QG_EW_ADD, QG_EW_MUL};
        for (int k = 0; k < 3; ++k) {
            qgemul_ew_stage& s = e.stage[k];
            s.op = ops[k]; s.x_first = 1; s.e_scalar = k != 1;
            put(s.e, fmt(3, 4, 1, 5, 0)); put(s.r, fmt(16, 12, 1, 5, 0)); put(s.t, fmt(12, 8 + k, 1, 5, 0));
        }
    }
    static void table(qgemul_approx& t, int64_t last)
    {
        t.n_seg = 2;
        for (uint32_t g = 0; g < t.n_seg; ++g) {
            t.seg[g].breakpoint = g ? 1e300 : 0.5;
            t.seg[g].n_coef = 3;
            for (uint32_t i = 0; i < 3; ++i) { put(t.seg[g].f[i], fmt(4, 10, 1, 5, 0)); t.seg[g].a[i] = 1 + (int64_t)(g * 3 + i); }
        }
        t.seg[1].a[2] = last;
    }
};

enum Kind { PLAIN, CHAIN, CHAIN_T1, CHAIN_T2, CPLX, CPLX_BASIC, CPLX_TF, BATCH1, BATCH2, BATCH7, BCHAIN_SHARED, BCHAIN_MEMBER, BCHAIN_MEMBER_T1,
            GROUP1, GROUP3, GROUP3_LAST_K, GROUP3_ORDER, GCHAIN, GCHAIN_PER0, BCHAIN3_SHARED0, NKIND };
static const char* const NAME[NKIND] = {"plain", "chain", "chain+table1", "chain+table2", "complex chain", "complex chain+CMUL basic", "complex chain+CMUL TF",
                                        "batched 1", "batched 2", "batched 7", "batched chain shared", "batched chain per member", "batched chain per member+table1",
                                        "group of one", "group of three", "group of three, last K changed", "group of three, another order", "grouped chain",
                                        "grouped chain, stage 0 per member", "batched 3 chain, stage 0 shared"};
// the requests that hold the most: (c) sets and assigns every kind over each of them
static const int LARGEST[2] = {BCHAIN_MEMBER_T1, GCHAIN_PER0};

// the key as the entry point of that kind builds it (qg_run.hip)
static void key_of(int kind, const Inputs& in, QRunKey& key)
{
    static const qgemul_approx* const none[QG_MAX_EW] = {};
    const qgemul_approx* ax[QG_MAX_EW] = {nullptr, nullptr, kind == CHAIN_T2 ? &in.t2 : &in.t1, nullptr};
    const qgemul_cmul* cx[QG_MAX_EW] = {nullptr, nullptr, kind == CPLX_TF ? &in.tf : &in.basic, nullptr};
    const EpView re = {&in.ep, nullptr, nullptr};
    const EpView rex = {&in.ep, nullptr, nullptr, ax};
    const EpView ren = {&in.ep, nullptr, nullptr, none};
    const EpView cp = {&in.epc.part[0], &in.epc.part[1], in.epc.e_complex};
    const EpView cpx = {&in.epc.part[0], &in.epc.part[1], in.epc.e_complex, nullptr, &in.epc, cx};
    // (the lists are copies: their padding and unused levels are those of `in`)
    const qgemul_desc one[1] = {in.d}, three[3] = {in.g[0], in.g[1], in.g[2]}, order[3] = {in.g[2], in.g[0], in.g[1]};
    qgemul_desc last_k[3] = {in.g[0], in.g[1], in.g[2]};
    last_k[2].K = 65;   // (three[0] and the count stay)
    switch (kind) {
    case PLAIN: qg_run_key_set(key, in.d, 0, 0, nullptr, nullptr); break;
    case CHAIN: qg_run_key_set(key, in.d, 0, 0, &re, nullptr); break;
    case CHAIN_T1:
    case CHAIN_T2: qg_run_key_set(key, in.d, 0, 0, &rex, nullptr); break;
    case CPLX: qg_run_key_set(key, in.d, 0, 0, &cp, nullptr); break;
    case CPLX_BASIC:
    case CPLX_TF: qg_run_key_set(key, in.d, 0, 0, &cpx, nullptr); break;
    case BATCH1: qg_run_key_set(key, in.d, 0, 1, nullptr, nullptr); break;
    case BATCH2: qg_run_key_set(key, in.d, 0, 2, nullptr, nullptr); break;
    case BATCH7: qg_run_key_set(key, in.d, 0, 7, nullptr, nullptr); break;
    case BCHAIN_SHARED: qg_run_key_set(key, in.d, 0, 7, &ren, &in.shared); break;
    case BCHAIN_MEMBER: qg_run_key_set(key, in.d, 0, 7, &ren, &in.per_member); break;
    case BCHAIN_MEMBER_T1: qg_run_key_set(key, in.d, 0, 7, &rex, &in.per_member); break;
    case GROUP1: qg_run_key_set_grouped(key, one, 1, 0, nullptr, &in.per_none); break;
    case GROUP3: qg_run_key_set_grouped(key, three, 3, 0, nullptr, &in.per_none); break;
    case GROUP3_LAST_K: qg_run_key_set_grouped(key, last_k, 3, 0, nullptr, &in.per_none); break;
    case GROUP3_ORDER: qg_run_key_set_grouped(key, order, 3, 0, nullptr, &in.per_none); break;
    case GCHAIN: qg_run_key_set_grouped(key, three, 3, 0, &ren, &in.per_none); break;
    case GCHAIN_PER0: qg_run_key_set_grouped(key, three, 3, 0, &ren, &in.per0); break;
    case BCHAIN3_SHARED0: qg_run_key_set(key, in.g[0], 0, 3, &ren, &in.shared0); break;   // (the batched twin of GCHAIN_PER0: same count, same bit pattern)
    }
}

int main()
{
    static Inputs first, copy;
    first.fill(0x5A);
    copy.fill(0xA5);
    int bad = 0, checks = 0;
    auto expect = [&](bool ok, const char* what, int i, int j) {
        ++checks;
        if (!ok) { ++bad; printf("FAIL %s: %s / %s\n", what, NAME[i], NAME[j]); }
    };
    static QRunKey a[NKIND], b[NKIND];
    for (int k = 0; k < NKIND; ++k) { key_of(k, first, a[k]); key_of(k, copy, b[k]); }
    // (a) the same request from copies of its inputs whose padding, reserved bytes and unused entries differ
    for (int k = 0; k < NKIND; ++k) {
        expect(qg_run_key_equal(a[k], b[k]), "copy differs", k, k);
        expect(qg_run_key_equal(b[k], a[k]), "copy differs (swapped)", k, k);
    }
    // ... and a chain without tables is one plan whether it comes with no table list or with a list of null tables
    {
        static const qgemul_approx* const none[QG_MAX_EW] = {};
        const EpView ren = {&first.ep, nullptr, nullptr, none};
        QRunKey n;
        qg_run_key_set(n, first.d, 0, 0, &ren, nullptr);
        expect(qg_run_key_equal(n, a[CHAIN]) && qg_run_key_equal(a[CHAIN], n), "null tables differ from no tables", CHAIN, CHAIN);
    }
    // (b) two different kinds never compare equal
    for (int i = 0; i < NKIND; ++i)
        for (int j = 0; j < NKIND; ++j)
            if (i != j) expect(!qg_run_key_equal(a[i], b[j]), "kinds conflated", i, j);
    // (c) no field keeps an earlier plan's value: set over each of the largest requests, and assigned over it (a plain key over a
    // grouped one drops the list, a group of one over a group of three shortens it)
    for (int big : LARGEST)
        for (int k = 0; k < NKIND; ++k) {
            QRunKey over, assigned;
            key_of(big, copy, over);
            key_of(CPLX_TF, copy, assigned);
            assigned = over;
            expect(qg_run_key_equal(assigned, a[big]), "assignment", big, big);
            key_of(k, first, over);
            assigned = a[k];
            expect(qg_run_key_equal(over, a[k]) && qg_run_key_equal(a[k], over), "set over a larger request", k, big);
            expect(qg_run_key_equal(assigned, a[k]) && qg_run_key_equal(a[k], assigned), "assigned over a larger request", k, big);
            for (int j = 0; j < NKIND; ++j)
                if (j != k) expect(!qg_run_key_equal(over, b[j]) && !qg_run_key_equal(b[j], over), "set over a larger request conflates", k, j);
        }
    // flags and every size are part of the key
    {
        QRunKey f;
        qg_run_key_set(f, first.d, QG_OPT_FORCE_TREE, 0, nullptr, nullptr);
        expect(!qg_run_key_equal(f, a[PLAIN]), "flags ignored", PLAIN, PLAIN);
        Inputs* m = new Inputs(first);
        m->d.M = 64;   // (the band of a sharded call)
        qg_run_key_set(f, m->d, 0, 0, nullptr, nullptr);
        expect(!qg_run_key_equal(f, a[PLAIN]), "M ignored", PLAIN, PLAIN);
        delete m;
    }
    printf("%s %d checks, %d failed\n", bad ? "FAILED" : "ok", checks, bad);
    return bad ? 1 : 0;
}
