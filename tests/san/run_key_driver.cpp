// The one-shot calls' plan key (qublas_amd/csrc/qg_run_key.h) on its own, under AddressSanitizer + UndefinedBehaviorSanitizer
// (tests/test_run_key.py builds and runs this).  One descriptor, every kind of request an entry point of qgemul_run* can make.
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
    qgemul_epilogue ep;
    qgemul_approx t1, t2;          // t2: one coefficient differs
    qgemul_epilogue_cplx epc;
    qgemul_cmul basic, tf;
    qgemul_batched_ep shared, per_member;

    void fill(int poison)
    {
        memset((void*)this, poison, sizeof *this);
        d.abi = QGEMUL_ABI_VERSION; d.transA = 0; d.is_complex = 0; d.cmul = QG_CMUL_NONE; d.flags = 0;
        d.M = 65; d.N = 33; d.K = 100; d.n_levels = 7;
        for (int p = 0; p < 2; ++p) {
            put(d.a[p], fmt(7, 8, 1, 5, 0)); put(d.b[p], fmt(7, 8, 1, 5, 0)); put(d.c[p], fmt(12, 8, 1, 5, 0));
            for (uint32_t l = 0; l < d.n_levels; ++l) { put(d.level_add[p][l], fmt(20 + (int)l, 10, 1, 5, 0)); put(d.level[p][l], fmt(21 + (int)l, 10, 1, 5, 0)); }
        }
        for (int i = 0; i < 8; ++i) put(d.mul[i], fmt(14 + i, 16, 1, 5, 0));
        chain(ep, 0);
        chain(epc.part[0], 0);
        chain(epc.part[1], 1);
        for (uint32_t k = 0; k < ep.n_stages; ++k) epc.e_complex[k] = k == 1;
        table(t1, 3);
        table(t2, 4);
        basic.cmul = QG_CMUL_BASIC;
        tf.cmul = QG_CMUL_TF;
        for (int i = 0; i < 8; ++i) { put(basic.mul[i], fmt(10 + i, 6, 1, 5, 0)); put(tf.mul[i], fmt(10 + i, 6, 1, 5, 0)); }
        for (int k = 0; k < QG_MAX_EW; ++k) { shared.e_shared[k] = k == 1; per_member.e_shared[k] = 0; }
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

enum Kind { PLAIN, CHAIN, CHAIN_T1, CHAIN_T2, CPLX, CPLX_BASIC, CPLX_TF, BATCH2, BATCH7, BCHAIN_SHARED, BCHAIN_MEMBER, BCHAIN_MEMBER_T1, NKIND };
static const char* const NAME[NKIND] = {"plain", "chain", "chain+table1", "chain+table2", "complex chain", "complex chain+CMUL basic", "complex chain+CMUL TF",
                                        "batched 2", "batched 7", "batched chain shared", "batched chain per member", "batched chain per member+table1"};

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
    switch (kind) {
    case PLAIN: qg_run_key_set(key, in.d, 0, 0, nullptr, nullptr); break;
    case CHAIN: qg_run_key_set(key, in.d, 0, 0, &re, nullptr); break;
    case CHAIN_T1:
    case CHAIN_T2: qg_run_key_set(key, in.d, 0, 0, &rex, nullptr); break;
    case CPLX: qg_run_key_set(key, in.d, 0, 0, &cp, nullptr); break;
    case CPLX_BASIC:
    case CPLX_TF: qg_run_key_set(key, in.d, 0, 0, &cpx, nullptr); break;
    case BATCH2: qg_run_key_set(key, in.d, 0, 2, nullptr, nullptr); break;
    case BATCH7: qg_run_key_set(key, in.d, 0, 7, nullptr, nullptr); break;
    case BCHAIN_SHARED: qg_run_key_set(key, in.d, 0, 7, &ren, &in.shared); break;
    case BCHAIN_MEMBER: qg_run_key_set(key, in.d, 0, 7, &ren, &in.per_member); break;
    case BCHAIN_MEMBER_T1: qg_run_key_set(key, in.d, 0, 7, &rex, &in.per_member); break;
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
    // (c) no field keeps an earlier plan's value: set over the largest request, and assigned over it
    for (int k = 0; k < NKIND; ++k) {
        QRunKey over, assigned;
        key_of(BCHAIN_MEMBER_T1, copy, over);
        key_of(CPLX_TF, copy, assigned);
        assigned = over;
        expect(qg_run_key_equal(assigned, a[BCHAIN_MEMBER_T1]), "assignment", BCHAIN_MEMBER_T1, BCHAIN_MEMBER_T1);
        key_of(k, first, over);
        assigned = a[k];
        expect(qg_run_key_equal(over, a[k]) && qg_run_key_equal(a[k], over), "set over a larger request", k, BCHAIN_MEMBER_T1);
        expect(qg_run_key_equal(assigned, a[k]) && qg_run_key_equal(a[k], assigned), "assigned over a larger request", k, BCHAIN_MEMBER_T1);
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
