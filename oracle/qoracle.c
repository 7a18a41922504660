/*
 * qoracle.c — TEST INFRASTRUCTURE, NOT PRODUCT CODE.
 *
 * A plain-C, CPU-only restatement of the arithmetic that the reference header
 * (/root/reference/include/QuBLAS.h, snapshot 2025-04-04) performs for a fixed-point GEMM
 *     C[i,j] = cvt_C( Qreduce<AddArgs…>( { Qmul<MulArgs…>(A'[i,k], B[k,j]) }_k ) ).
 * Only tests/, __graft_entry__.smoke() and bench.py's cpu_baseline leg may load this file's
 * shared object; the engine (qublas_amd/csrc) never links or calls it and has no CPU fallback.
 *
 * Pinning: the functions below are checked bit-for-bit against
 *   (a) the reference's own rounding tests  test/TRN/{TCPL,SMGN}.cpp, test/RND/{POSINF,NEGINF,
 *       ZERO,INF,CONV}.cpp (40 known answers, tests/golden/ref_rounding_kat.json), and
 *   (b) golden vectors produced in the build container by oracle/ref_driver.cpp, which includes
 *       the real reference header and composes Qmul + Qreduce + converting assignment
 *       (tests/golden/ref_*.json; generator oracle/gen_golden.py).
 * `Qgemul` itself does not exist in the reference snapshot (only readme.md:84-87 mentions it),
 * so the GEMM-level composition is "parity unpinned by reference tests" and pinned by (b) only.
 *
 * Every intermediate is held in __int128, so the restatement is exact for any expression whose
 * intermediates stay below 2^120 (unrounded products: 2^127); the wide part of that range — values the
 * reference keeps in its multi-word ArbiInt<N>64>, QuBLAS.h:566-912 — is pinned by tests/golden/ref_wide_*
 * (oracle/ref_cases_wide.cpp).  Wider expressions are outside it.
 */
#include "../include/qgemul.h"

#include <pthread.h>
#include <stdlib.h>
#include <string.h>

typedef __int128 qi;
typedef unsigned __int128 qu;

#define QO_MAX_SHIFT 100

static inline qi qo_shl(qi x, int s) { return (qi)((qu)x << s); }
static inline qi qo_pow2(int s) { return (qi)((qu)1 << s); }

/* arithmetic shift right that also covers s >= width (staticShiftRight with N <= shift returns
 * all-sign, QuBLAS.h:1597-1604) */
static inline qi qo_sar(qi x, int s) { return s >= 127 ? (x < 0 ? -1 : 0) : (x >> s); }

/*
 * fracConvert<from,to,QuMode>::convert, QuBLAS.h:2002-2204.  d = from - to.
 * d <= 0: exact left shift for every mode (:2011-2014, :2166 via the negative-shift overload
 * :1689-1694, :2181-2184).
 */
static qi qo_round(qi x, int d, int mode)
{
    if (d <= 0) return qo_shl(x, -d);
    qi h = qo_sar(x, d);                       /* Xh = staticShiftRight<d>(val) */
    qi l = x & (qo_pow2(d) - 1);               /* Xl = val & allOnes<d> */
    qi T = qo_pow2(d - 1);                     /* staticShiftLeft<d-1>(1) */
    switch (mode) {
    case QG_RND_POS_INF: return h + (l >= T);                                  /* :2026 */
    case QG_RND_NEG_INF: return h + (l > T);                                   /* :2056 */
    case QG_RND_ZERO:    return h + (l > T || (l == T && x < 0));              /* :2086 */
    case QG_RND_INF:     return h + (l > T || (l == T && x > 0));              /* :2116 */
    case QG_RND_CONV:    return h + (l > T || (l == T && (h & 1)));            /* :2137-2156 */
    case QG_TRN_TCPL:    return h;                                             /* :2166 */
    case QG_TRN_SMGN:    return x < 0 ? -qo_sar(-x, d) : h;                    /* :2189-2199 */
    default:             return h;
    }
}

/*
 * Width (in bits) of the ArbiInt that fracConvert<from,to,QuMode> returns for an N-bit input: staticShiftLeft / Right change
 * the width by the shift (QuBLAS.h:1485-1701); the four RND modes (and CONV) end in `Xh + ArbiInt<1>`, one bit more
 * (:2032, operator+ :917-938); TRN::TCPL / TRN::SMGN keep N - d (:2166, :2175-2178).
 */
static int qo_round_width(int N, int d, int mode)
{
    if (d <= 0) return N - d;
    int w = N - d < 1 ? 1 : N - d;
    return (mode == QG_TRN_TCPL || mode == QG_TRN_SMGN) ? w : w + 1;
}

/*
 * The saturating modes compare the value with the target's bounds (`val > floor`, `val < ceil`, QuBLAS.h:2239-2250).  When the
 * value is a MULTI-WORD ArbiInt (more than 64 bits wide as a TYPE) and the target's storage fits one word, that comparison is
 * operator<=>(ArbiInt<N > 64>, ArbiInt<M <= 64>) (:1781-1793): the upper words are compared with the bound's sign extension
 * and then the LOW word is compared AS A SIGNED 64-bit number — so a value in [2^63, 2^64) or [-2^64, -2^63) passes for one of
 * the opposite sign and is neither above the maximum nor below the minimum; it is then narrowed by ArbiInt<M>(val), which keeps
 * the low word (:436-441; int32_t storage for M <= 32).  Everything else agrees with the arithmetic definition.  This is what a
 * user of the reference gets (tests/golden/ref_wide_*: the tables hold values in those bands), so it is restated, not "fixed".
 */
static int qo_ref_cmp(qi v, qi bound)   /* sign of (v <=> bound) as the reference computes it for a multi-word v, one-word bound */
{
    int64_t hi = (int64_t)(v >> 64), lo = (int64_t)(uint64_t)(qu)v, ext = bound < 0 ? -1 : 0;
    if (hi != ext) return hi < ext ? -1 : 1;
    return lo < (int64_t)bound ? -1 : (lo > (int64_t)bound ? 1 : 0);
}

/* intConvert<I,F,S,OfMode>::convert, QuBLAS.h:2227-2334; nin = width of the incoming ArbiInt type (0: a one-word value) */
static qi qo_overflow_n(qi x, qfmt f, int nin)
{
    int W = (int)f.I + (int)f.F;
    qi maxv = qo_pow2(W) - 1;                  /* ArbiInt<1+W>::maximum() */
    qi minv = f.S ? -qo_pow2(W) : 0;           /* minimum() or 0 */
    if (nin > 64 && 1 + W <= 64 && f.O <= QG_SAT_SMGN) {
        qi lo = f.O == QG_SAT_SMGN ? (f.S ? -maxv : 0) : minv;
        if (qo_ref_cmp(x, maxv) > 0) return f.O == QG_SAT_ZERO ? 0 : maxv;
        if (qo_ref_cmp(x, lo) < 0) return f.O == QG_SAT_ZERO ? 0 : lo;
        return 1 + W <= 32 ? (qi)(int32_t)(uint32_t)(qu)x : (qi)(int64_t)(uint64_t)(qu)x;   /* ArbiInt<M>(val): the low word */
    }
    switch (f.O) {
    case QG_SAT_TCPL:                                                           /* :2239-2250 */
        return x > maxv ? maxv : (x < minv ? minv : x);
    case QG_SAT_ZERO:                                                           /* :2265-2276 */
        return (x > maxv || x < minv) ? 0 : x;
    case QG_SAT_SMGN: {                                                         /* :2286-2300 */
        qi lo = f.S ? -maxv : 0;
        return x > maxv ? maxv : (x < lo ? lo : x);
    }
    case QG_WRP_TCPL:                                                           /* :2308-2332 */
        if (f.S) {
            qi mask = qo_pow2(W + 1) - 1;
            qi m = x & mask;
            return (m >> W) ? (m | ~mask) : m;
        }
        return x & (qo_pow2(W) - 1);
    default:
        /* WRP::TCPL_SAT<N>: a stub returning its input (:2336-2344); the assignment into the target's storage narrows it to the
         * storage WORD — ArbiInt<M <= 32> keeps an int32_t, <= 64 an int64_t, never masked to M bits (:353, :431-441; pinned by
         * tests/golden/ref_scalar_9, ref_gemm_real_8) */
        if (1 + W <= 32) return (qi)(int32_t)(uint32_t)(qu)x;
        if (1 + W <= 64) return (qi)(int64_t)(uint64_t)(qu)x;
        return x;
    }
}
static qi qo_overflow(qi x, qfmt f) { return qo_overflow_n(x, f, 0); }
static int qo_sbits(qfmt f) { return 1 + (int)f.I + (int)f.F; }

static inline int qo_same(qfmt a, qfmt b)
{
    return a.I == b.I && a.F == b.F && a.S == b.S && a.Q == b.Q && a.O == b.O;
}

/* converting constructor Qu_s(const Qu_s<from>&), QuBLAS.h:2398-2411: identity when the five
 * parameters agree, otherwise round with the TARGET's QuMode then overflow with its OfMode. */
static qi qo_cvt(qi x, qfmt from, qfmt to)
{
    if (qo_same(from, to)) return x;
    int d = (int)from.F - (int)to.F;
    return qo_overflow_n(qo_round(x, d, to.Q), to, qo_round_width(qo_sbits(from), d, to.Q));
}

/* Qmul_s::mul, QuBLAS.h:3152-3170: full product, fracConvert<Fa+Fb -> Fr>, intConvert */
static qi qo_mul(qi a, qfmt fa, qi b, qfmt fb, qfmt r)
{
    int d = (int)fa.F + (int)fb.F - (int)r.F;
    /* operator*: an N-bit by an M-bit integer gives N + M bits (QuBLAS.h:1186-1207) */
    return qo_overflow_n(qo_round(a * b, d, r.Q), r, qo_round_width(qo_sbits(fa) + qo_sbits(fb), d, r.Q));
}

/* Qadd_s::add / Qsub_s::sub, QuBLAS.h:3185-3203 / :3219-3234: align to max frac, add, convert */
static qi qo_addsub(qi a, qfmt fa, qi b, qfmt fb, qfmt r, int sub)
{
    int fm = fa.F > fb.F ? fa.F : fb.F;
    qi x = qo_shl(a, fm - fa.F), y = qo_shl(b, fm - fb.F);
    qi s = sub ? x - y : x + y;
    /* the aligned operands are N + shift bits wide, their sum / difference one bit more than the wider one (:914-1010) */
    int na = qo_sbits(fa) + fm - fa.F, nb = qo_sbits(fb) + fm - fb.F;
    int n = (na > nb ? na : nb) + 1;
    return qo_overflow_n(qo_round(s, fm - (int)r.F, r.Q), r, qo_round_width(n, fm - (int)r.F, r.Q));
}

/* format of the value entering the tree, per part */
static qfmt qo_prod_fmt(const qgemul_desc* d, int part)
{
    if (!d->is_complex) return d->mul[QG_MUL_REAL];
    if (d->cmul == QG_CMUL_TF) return d->mul[part ? QG_T_IM : QG_T_RE];
    return d->mul[part ? QG_B_IM : QG_B_RE];
}

/* one (possibly complex) product: x = A'[i,k] = (a, b), y = B[k,j] = (c, dd) */
static void qo_product(const qgemul_desc* d, const qi x[2], const qi y[2], qi out[2])
{
    const qfmt* m = d->mul;
    if (!d->is_complex) {
        out[0] = qo_mul(x[0], d->a[0], y[0], d->b[0], m[QG_MUL_REAL]);
        out[1] = 0;
        return;
    }
    qi a = x[0], b = x[1], c = y[0], dd = y[1];
    qfmt fa = d->a[0], fb = d->a[1], fc = d->b[0], fd = d->b[1];
    if (d->cmul == QG_CMUL_TF) { /* QuBLAS.h:3524-3529 */
        qi ab = qo_addsub(a, fa, b, fb, m[QG_T_AB], 0);
        qi cd = qo_addsub(c, fc, dd, fd, m[QG_T_CD], 0);
        qi ba = qo_addsub(b, fb, a, fa, m[QG_T_BA], 1);
        qi A = qo_mul(ab, m[QG_T_AB], c, fc, m[QG_T_A]);
        qi B = qo_mul(cd, m[QG_T_CD], b, fb, m[QG_T_B]);
        qi C = qo_mul(ba, m[QG_T_BA], dd, fd, m[QG_T_C]);
        out[0] = qo_addsub(A, m[QG_T_A], B, m[QG_T_B], m[QG_T_RE], 1);
        out[1] = qo_addsub(B, m[QG_T_B], C, m[QG_T_C], m[QG_T_IM], 1);
    } else { /* BasicComplexMul, QuBLAS.h:3439-3440 */
        qi ac = qo_mul(a, fa, c, fc, m[QG_B_AC]);
        qi bd = qo_mul(b, fb, dd, fd, m[QG_B_BD]);
        qi ad = qo_mul(a, fa, dd, fd, m[QG_B_AD]);
        qi bc = qo_mul(b, fb, c, fc, m[QG_B_BC]);
        out[0] = qo_addsub(ac, m[QG_B_AC], bd, m[QG_B_BD], m[QG_B_RE], 1);
        out[1] = qo_addsub(ad, m[QG_B_AD], bc, m[QG_B_BC], m[QG_B_IM], 0);
    }
}

/*
 * Reducer::reduce_impl (vector overload), QuBLAS.h:4960-4984, one part of the value.
 * buf holds len values in format `fin`; returns the root and writes its format to *fout.
 * Level l: pairs are added into level_add[l] then stored into the level buffer of type level[l]
 * (:4966, :4974); an odd leftover is copied with the converting constructor (:4977-4980; the identity for equal types,
 * which the Qreduce lowering of a signed SAT::SMGN element type requests for level 0 with QG_DESC_LEFTOVER0_COPY);
 * a length-1 input is returned unconverted (:4967-4970).
 */
static qi qo_tree(qi* buf, int64_t len, qfmt fin, const qfmt* level_add, const qfmt* level,
                  qfmt* fout, int copy0)
{
    int l = 0;
    qfmt cur = fin;
    while (len > 1) {
        qfmt fa = level_add[l], fl = level[l];
        int64_t half = len / 2;
        for (int64_t t = 0; t < half; ++t)
            buf[t] = qo_cvt(qo_addsub(buf[2 * t], cur, buf[2 * t + 1], cur, fa, 0), fa, fl);
        /* copy0 (QG_DESC_LEFTOVER0_COPY): level 0's type IS the element type in the reference, the copy is the identity */
        if (len & 1) buf[half] = (l == 0 && copy0) ? buf[len - 1] : qo_cvt(buf[len - 1], cur, fl);
        len = (len + 1) / 2;
        cur = fl;
        ++l;
    }
    *fout = cur;
    return buf[0];
}

/* ---- host ("reference") element layout: ArbiInt<N<=32> is int32_t, <=64 int64_t
 *      (QuBLAS.h:353); a complex element is struct { real; imag; } (:2512-2513) ---- */
/* ArbiInt<N > 64> is a little-endian std::array<uint64_t, ceil(N/64)> whose top word carries the sign (QuBLAS.h:572-573,
 * :635-638): 16 bytes, 8-byte aligned, for 65 .. 128 storage bits (wider elements are outside this restatement). */
static int qo_sbytes(qfmt f)
{
    int b = 1 + (int)f.I + (int)f.F;
    return b <= 32 ? 4 : b <= 64 ? 8 : 16;
}

typedef struct { int size, off[2], sb[2]; } qo_layout;

static qo_layout qo_elem_layout(const qfmt f[2], int is_complex)
{
    qo_layout L;
    L.sb[0] = qo_sbytes(f[0]);
    L.off[0] = 0;
    if (!is_complex) { L.sb[1] = 0; L.off[1] = 0; L.size = L.sb[0]; return L; }
    L.sb[1] = qo_sbytes(f[1]);
    int a0 = L.sb[0] > 8 ? 8 : L.sb[0], a1 = L.sb[1] > 8 ? 8 : L.sb[1];   /* alignment of int32_t / int64_t / uint64_t[2] */
    int al = a0 > a1 ? a0 : a1;
    L.off[1] = (L.sb[0] + a1 - 1) / a1 * a1;
    L.size = (L.off[1] + L.sb[1] + al - 1) / al * al;
    return L;
}

static inline qi qo_load(const char* p, int sb)
{
    if (sb == 4) { int32_t v; memcpy(&v, p, 4); return v; }
    if (sb == 8) { int64_t v; memcpy(&v, p, 8); return v; }
    uint64_t w[2]; memcpy(w, p, 16);
    return (qi)(((qu)w[1] << 64) | (qu)w[0]);
}
static inline void qo_store(char* p, int sb, qi x)
{
    if (sb == 4) { int32_t v = (int32_t)x; memcpy(p, &v, 4); }
    else if (sb == 8) { int64_t v = (int64_t)x; memcpy(p, &v, 8); }
    else { uint64_t w[2] = {(uint64_t)(qu)x, (uint64_t)((qu)x >> 64)}; memcpy(p, w, 16); }
}

int qoracle_elem_bytes(const qfmt* f2, int is_complex)
{
    return qo_elem_layout(f2, is_complex).size;
}
int qoracle_imag_offset(const qfmt* f2, int is_complex)
{
    return qo_elem_layout(f2, is_complex).off[1];
}

static int qo_check(const qgemul_desc* d)
{
    if (!d || d->abi != QGEMUL_ABI_VERSION) return QG_EINVAL;
    if (d->M < 0 || d->N < 0 || d->K < 1) return QG_EINVAL;
    int64_t len = d->K; uint32_t n = 0;
    while (len > 1) { len = (len + 1) / 2; ++n; }
    if (n != d->n_levels || n > QG_MAX_LEVELS) return QG_EINVAL;
    return QG_OK;
}

typedef struct {
    const qgemul_desc* d;
    char* C; const char* A; const char* B;
    int64_t lda, ldb, ldc;
    int64_t row0, row1, col0, col1;
    int tid, nthreads;
    int status;
} qo_job;

static void* qo_worker(void* arg)
{
    qo_job* j = (qo_job*)arg;
    const qgemul_desc* d = j->d;
    const int parts = d->is_complex ? 2 : 1;
    qo_layout LA = qo_elem_layout(d->a, d->is_complex);
    qo_layout LB = qo_elem_layout(d->b, d->is_complex);
    qo_layout LC = qo_elem_layout(d->c, d->is_complex);
    const int64_t K = d->K;
    qi* buf[2];
    buf[0] = (qi*)malloc(sizeof(qi) * (size_t)K);
    buf[1] = (qi*)malloc(sizeof(qi) * (size_t)K);
    if (!buf[0] || !buf[1]) { j->status = QG_EINVAL; free(buf[0]); free(buf[1]); return 0; }
    for (int64_t col = j->col0 + j->tid; col < j->col1; col += j->nthreads) {
        for (int64_t row = j->row0; row < j->row1; ++row) {
            for (int64_t k = 0; k < K; ++k) {
                /* A'[i,k]: A is dim<M,K> (element i + k*lda) or, transposed, dim<K,M> (k + i*lda) */
                int64_t ia = d->transA ? (k + row * j->lda) : (row + k * j->lda);
                int64_t ib = k + col * j->ldb;
                const char* pa = j->A + ia * LA.size;
                const char* pb = j->B + ib * LB.size;
                qi x[2] = {0, 0}, y[2] = {0, 0}, p[2];
                for (int q = 0; q < parts; ++q) {
                    x[q] = qo_load(pa + LA.off[q], LA.sb[q]);
                    y[q] = qo_load(pb + LB.off[q], LB.sb[q]);
                }
                qo_product(d, x, y, p);
                buf[0][k] = p[0];
                buf[1][k] = p[1];
            }
            char* pc = j->C + (row + col * j->ldc) * LC.size;
            for (int q = 0; q < parts; ++q) {
                qfmt fr;
                qi r = qo_tree(buf[q], K, qo_prod_fmt(d, q), d->level_add[q], d->level[q], &fr, d->flags & QG_DESC_LEFTOVER0_COPY);
                qo_store(pc + LC.off[q], LC.sb[q], qo_cvt(r, fr, d->c[q]));
            }
        }
    }
    free(buf[0]); free(buf[1]);
    return 0;
}

/*
 * The GEMM restatement.  Host pointers in reference layout, leading dimensions in elements
 * (0 = tight).  Only the block rows [row0,row1) x cols [col0,col1) of C is computed and written
 * (row1/col1 <= 0 mean "to the end"), so large configurations can be sampled.
 */
int qoracle_gemm(const qgemul_desc* d, void* C, const void* A, const void* B, int64_t lda,
                 int64_t ldb, int64_t ldc, int64_t row0, int64_t row1, int64_t col0, int64_t col1,
                 int nthreads)
{
    int st = qo_check(d);
    if (st) return st;
    if (!C || !A || !B) return QG_EINVAL;
    /* QG_DESC_REFERENCE_ARTEFACTS (include/qgemul.h): C of an unsigned WRP::TCPL format with exactly 32 value bits comes out of the
       reference unwrapped (mask = ArbiInt<32>::allOnes() = -1, /root/reference/include/QuBLAS.h:361-377, :2328-2331;
       tests/golden/ref_scalar_6) — the behaviour of its WRP::TCPL_SAT stub */
    qgemul_desc with_artefacts;
    if (d->flags & QG_DESC_REFERENCE_ARTEFACTS) {
        with_artefacts = *d;
        for (int p = 0; p < (d->is_complex ? 2 : 1); ++p) {
            qfmt* f = &with_artefacts.c[p];
            if (f->O == QG_WRP_TCPL && !f->S && (int)f->I + (int)f->F == 32) f->O = QG_WRP_TCPL_SAT;
        }
        d = &with_artefacts;
    }
    if (row1 <= 0) row1 = d->M;
    if (col1 <= 0) col1 = d->N;
    if (row0 < 0 || row1 > d->M || col0 < 0 || col1 > d->N) return QG_EINVAL;
    if (!lda) lda = d->transA ? d->K : d->M;
    if (!ldb) ldb = d->K;
    if (!ldc) ldc = d->M;
    if (nthreads < 1) nthreads = 1;
    if (nthreads > 256) nthreads = 256;
    qo_job jobs[256];
    pthread_t th[256];
    for (int t = 0; t < nthreads; ++t) {
        jobs[t] = (qo_job){d, (char*)C, (const char*)A, (const char*)B, lda, ldb, ldc,
                           row0, row1, col0, col1, t, nthreads, 0};
        if (nthreads == 1) qo_worker(&jobs[t]);
        else pthread_create(&th[t], 0, qo_worker, &jobs[t]);
    }
    for (int t = 0; t < nthreads; ++t) {
        if (nthreads > 1) pthread_join(th[t], 0);
        if (jobs[t].status) st = jobs[t].status;
    }
    return st;
}

/*
 * Qu_s(double), QuBLAS.h:2387-2393: the double is loaded EXACTLY into a 2400-bit buffer with 1200+F fraction
 * bits (loadFromDouble, :663-749: 0 for zero / NaN / infinity), then fracConvert<1200+F -> F> with the type's
 * QuMode and intConvert with its OfMode.  Restated on a 53-bit mantissa: v = m * 2^e exactly, so the raw
 * value at F fraction bits is m * 2^(e+F): an exact left shift, or one rounding by d = -(e+F) bits.
 */
int64_t qoracle_from_double(double v, qfmt f)
{
    if (v == 0.0 || v != v || v - v != 0.0) return 0;
    uint64_t bits;
    memcpy(&bits, &v, 8);
    const int neg = (int)(bits >> 63);
    int ex = (int)((bits >> 52) & 0x7ff);
    qi m = (qi)(bits & 0xfffffffffffffull);
    if (ex == 0) ex = 1;                 /* subnormal: no implicit one */
    else m |= (qi)1 << 52;
    int e = ex - 1075 + (int)f.F;        /* value * 2^F = m * 2^e */
    if (neg) m = -m;
    qi r;
    if (e >= 0) {
        if (e > 60) e = 60;              /* |m| >= 1: far outside every supported format either way */
        r = qo_shl(m, e);
    } else {
        int d = -e;
        if (d > 120) {                   /* every mantissa bit is below the rounding position */
            qi tiny = neg ? -1 : 1;      /* same rounding class as any 0 < |x| < 1/2 ulp */
            r = qo_round(tiny, 8, f.Q);
        } else {
            r = qo_round(m, d, f.Q);
        }
    }
    return (int64_t)qo_overflow(r, f);
}

/* ---- scalar entry points for the known-answer tests (values as int64 raw integers) ---- */
int64_t qoracle_convert(int64_t x, qfmt from, qfmt to) { return (int64_t)qo_cvt(x, from, to); }
/* source wider than 64 bits (the reference tests' 141-bit High_t): value = hi*2^64 + lo */
int64_t qoracle_convert128(int64_t hi, uint64_t lo, qfmt from, qfmt to)
{
    qi x = (qi)(((qu)(uint64_t)hi << 64) | (qu)lo);
    return (int64_t)qo_cvt(x, from, to);
}
/* ---- the same primitives on values of up to 128 bits: w = {low word, high word (signed)} ---- */
static inline qi qo_from_w(const uint64_t w[2]) { return (qi)(((qu)w[1] << 64) | (qu)w[0]); }
static inline void qo_to_w(qi x, uint64_t w[2]) { w[0] = (uint64_t)(qu)x; w[1] = (uint64_t)((qu)x >> 64); }
void qoracle_convert_w(const uint64_t x[2], qfmt from, qfmt to, uint64_t y[2]) { qo_to_w(qo_cvt(qo_from_w(x), from, to), y); }
void qoracle_mul_w(const uint64_t a[2], qfmt fa, const uint64_t b[2], qfmt fb, qfmt r, uint64_t y[2])
{
    qo_to_w(qo_mul(qo_from_w(a), fa, qo_from_w(b), fb, r), y);
}
void qoracle_add_w(const uint64_t a[2], qfmt fa, const uint64_t b[2], qfmt fb, qfmt r, int sub, uint64_t y[2])
{
    qo_to_w(qo_addsub(qo_from_w(a), fa, qo_from_w(b), fb, r, sub), y);
}
int64_t qoracle_round(int64_t x, int d, int mode) { return (int64_t)qo_round(x, d, mode); }
int64_t qoracle_overflow(int64_t x, qfmt f) { return (int64_t)qo_overflow(x, f); }
int64_t qoracle_mul(int64_t a, qfmt fa, int64_t b, qfmt fb, qfmt r)
{
    return (int64_t)qo_mul(a, fa, b, fb, r);
}
int64_t qoracle_add(int64_t a, qfmt fa, int64_t b, qfmt fb, qfmt r, int sub)
{
    return (int64_t)qo_addsub(a, fa, b, fb, r, sub);
}
/* Qreduce over `len` real values of format fin with per-level formats (level_add == level) */
int64_t qoracle_reduce(const int64_t* v, int64_t len, qfmt fin, const qfmt* level, int nlev)
{
    qi* buf = (qi*)malloc(sizeof(qi) * (size_t)(len > 0 ? len : 1));
    qfmt lv[QG_MAX_LEVELS];
    for (int l = 0; l < QG_MAX_LEVELS; ++l) lv[l] = nlev ? level[l < nlev ? l : nlev - 1] : fin;
    for (int64_t t = 0; t < len; ++t) buf[t] = v[t];
    qfmt fo;
    qi r = qo_tree(buf, len, fin, lv, lv, &fo, 0);
    free(buf);
    return (int64_t)r;
}
/* one complex product through the descriptor's mul[] slots */
void qoracle_cproduct(const qgemul_desc* d, const int64_t x[2], const int64_t y[2], int64_t out[2])
{
    qi xx[2] = {x[0], x[1]}, yy[2] = {y[0], y[1]}, p[2];
    qo_product(d, xx, yy, p);
    out[0] = (int64_t)p[0];
    out[1] = (int64_t)p[1];
}

/* ---- BitStream export of a real tensor ----
 * Restates BitStream<tensorProcessT, elemProcessT>(tensor) (/root/reference/include/QuBLAS.h:4811-4827):
 *   element string = the low (isS + intB + fracB) bits of the raw value, MSB first (Qu_s::toString :2433-2438);
 *   elemProcessT  r2l<e>: the element string's e-character chunks in reverse order (SingleString_s :4593-4611, the string
 *                 length must be a multiple of e); l2r (e = 0): unchanged;
 *   tensorProcessT r2l<t>: the elements (storage order) in chunks of t, chunks in reverse order, order inside a chunk kept
 *                 (TensorString_s<r2l<index>,...>::toString :4738-4752; n must be a multiple of t); l2r (t = 0): unchanged.
 * out receives n * width characters '0' / '1' (no terminator).  Returns 0, or -1 for an invalid chunk. */
int qoracle_bitstream(qfmt f, int64_t n, const int64_t* x, int tensor_chunk, int elem_chunk, char* out)
{
    const int w = (int)f.I + (int)f.F + (f.S ? 1 : 0);
    if (w <= 0 || w > 64 || tensor_chunk < 0 || elem_chunk < 0) return -1;
    if (elem_chunk > 0 && w % elem_chunk) return -1;
    if (tensor_chunk > 0 && n % tensor_chunk) return -1;
    char es[64], ts[64];
    for (int64_t pos = 0; pos < n; ++pos) {
        int64_t src = pos;
        if (tensor_chunk > 0) {
            const int64_t nch = n / tensor_chunk, c = pos / tensor_chunk;
            src = (nch - 1 - c) * tensor_chunk + pos % tensor_chunk;
        }
        const uint64_t v = (uint64_t)x[src];
        for (int j = 0; j < w; ++j) es[j] = ((v >> (w - 1 - j)) & 1) ? '1' : '0';
        if (elem_chunk > 0) {
            const int nch = w / elem_chunk;
            for (int q = 0; q < nch; ++q)
                for (int r = 0; r < elem_chunk; ++r) ts[q * elem_chunk + r] = es[(nch - 1 - q) * elem_chunk + r];
            memcpy(out + pos * w, ts, (size_t)w);
        } else {
            memcpy(out + pos * w, es, (size_t)w);
        }
    }
    return 0;
}

/* ---- BitStream export of a COMPLEX tensor ----
 * A complex element's string is "(" + real.toString() + ", " + imag.toString() + ")" (Qu_s<complex>::toString,
 * /root/reference/include/QuBLAS.h:2553-2556), wr + wi + 4 characters; TensorString_s::fromQu hands exactly that string to the
 * element processing (:4672-4681), so r2l<e> reverses e-character chunks of the WHOLE string, punctuation included, and its
 * length must be a multiple of e; the tensor-level processing is that of a real tensor.  out receives n * (wr + wi + 4)
 * characters. */
int qoracle_bitstream_cplx(qfmt fre, qfmt fim, int64_t n, const int64_t* re, const int64_t* im, int tensor_chunk, int elem_chunk, char* out)
{
    const int wr = (int)fre.I + (int)fre.F + (fre.S ? 1 : 0), wi = (int)fim.I + (int)fim.F + (fim.S ? 1 : 0);
    if (wr < 0 || wr > 64 || wi < 0 || wi > 64 || tensor_chunk < 0 || elem_chunk < 0) return -1;   /* a part without bits prints as "" (substr of length 0, :2436) */
    const int w = wr + wi + 4;
    if (elem_chunk > 0 && w % elem_chunk) return -1;
    if (tensor_chunk > 0 && n % tensor_chunk) return -1;
    char es[136], ts[136];
    for (int64_t pos = 0; pos < n; ++pos) {
        int64_t src = pos;
        if (tensor_chunk > 0) {
            const int64_t nch = n / tensor_chunk, c = pos / tensor_chunk;
            src = (nch - 1 - c) * tensor_chunk + pos % tensor_chunk;
        }
        const uint64_t a = (uint64_t)re[src], b = (uint64_t)im[src];
        int k = 0;
        es[k++] = '(';
        for (int j = 0; j < wr; ++j) es[k++] = ((a >> (wr - 1 - j)) & 1) ? '1' : '0';
        es[k++] = ',';
        es[k++] = ' ';
        for (int j = 0; j < wi; ++j) es[k++] = ((b >> (wi - 1 - j)) & 1) ? '1' : '0';
        es[k++] = ')';
        if (elem_chunk > 0) {
            const int nch = w / elem_chunk;
            for (int q = 0; q < nch; ++q)
                for (int r = 0; r < elem_chunk; ++r) ts[q * elem_chunk + r] = es[(nch - 1 - q) * elem_chunk + r];
            memcpy(out + pos * w, ts, (size_t)w);
        } else {
            memcpy(out + pos * w, es, (size_t)w);
        }
    }
    return 0;
}

/* ---- element-wise epilogue: the lazy tensor operators applied per element after a Qgemul ----
 * Restates MulExpression / AddExpression / SubExpression::operator[] (/root/reference/include/QuBLAS.h:3795-3798,
 * :3828-3831, :3861-3864: Qop<toArgs...>(autoCall(q1, i), autoCall(q2, i)), a scalar operand used as is
 * :3767-3778) followed by the tensor's constructor from an indexable expression (:2732-2746), whose
 * data[i] = val[i] is the converting constructor (:2398-2411).  x[] holds C's raw values (format c), e[k] the
 * tensor operands' raw values (or one value for a scalar stage); out[] receives D's raw values. */
int qoracle_eltwise(const qgemul_epilogue* ep, qfmt c, int64_t n, const int64_t* x, const int64_t* const* e, int64_t* out)
{
    if (!ep || ep->n_stages > QG_MAX_EW) return -1;
    for (int64_t i = 0; i < n; ++i) {
        qi v = x[i];
        qfmt f = c;
        for (uint32_t k = 0; k < ep->n_stages; ++k) {
            const qgemul_ew_stage* s = &ep->stage[k];
            if (s->op == QG_EW_PASS) {   /* complex chains: the part the operator carries over (QuBLAS.h:3654, :3670, :3701) */
                if (k + 1 < ep->n_stages) { v = qo_cvt(v, f, s->t); f = s->t; }
                continue;
            }
            const qi ev = s->e_scalar ? e[k][0] : e[k][i];
            const qi a = s->x_first ? v : ev, b = s->x_first ? ev : v;
            const qfmt fa = s->x_first ? f : s->e, fb = s->x_first ? s->e : f;
            if (s->op == QG_EW_MUL) v = qo_mul(a, fa, b, fb, s->r);
            else if (s->op == QG_EW_ADD || s->op == QG_EW_SUB) v = qo_addsub(a, fa, b, fb, s->r, s->op == QG_EW_SUB);
            else return -1;
            f = s->r;
            if (k + 1 < ep->n_stages) { v = qo_cvt(v, f, s->t); f = s->t; }   /* the intermediate tensor */
        }
        out[i] = (int64_t)qo_cvt(v, f, ep->d);
    }
    return 0;
}


/*
 * Synthetic operands: raw value of host element e, part p is drawn from the
 * counter-based generator below, so host and device produce identical tensors without sharing
 * state.  dist 0: uniform over the whole representable range, as Qu::fill() does
 * (QuBLAS.h:526-536); dist 1: |raw| < 2^(W/2) ("small", keeps narrow accumulators unsaturated);
 * dist 2 ("edges", host only: the device fill knows dist 0 and 1): the lowest bit of the random value picks, about half the
 * time, an entry of the format's edge set (qo_edges) chosen by the other bits, else the dist-0 value.  The edge set puts exact
 * boundary products (-1 * min, 1 * max, (1 + ulp) * max), rounding ties (1/2 * odd) and boundary node sums into every
 * reduction of a few dozen leaves.  oracle/ref_driver.hpp restates all of this bit for bit.
 */
static inline uint64_t qo_rand(uint64_t seed, uint64_t idx)
{
    uint64_t z = seed + (idx + 1) * 0x9E3779B97F4A7C15ull;
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    return z ^ (z >> 31);
}

/* E(f): the sorted, distinct values of  lo, lo+1, -2^F-1, -2^F, -2^(F-1), -1, 0, 1, 2^(F-1), 2^F-1, 2^F, 2^F+1, hi-1, hi
 * that lie in the format's raw range [lo, hi] (clipped to int64); terms that are not integers (F <= 0) are left out.
 * 2^F is the format's one.  Returns the count (at most 14). */
static int qo_edges(qfmt f, int64_t out[14])
{
    const int W = (int)f.I + (int)f.F, F = (int)f.F;
    const __int128 lo = f.S ? (W >= 64 ? (__int128)INT64_MIN : -((__int128)1 << W)) : 0;
    const __int128 hi = W >= 63 ? (__int128)INT64_MAX : ((__int128)1 << W) - 1;
    __int128 c[14];
    int n = 0;
    c[n++] = lo; c[n++] = lo + 1; c[n++] = -1; c[n++] = 0; c[n++] = 1; c[n++] = hi - 1; c[n++] = hi;
    if (F >= 0 && F <= 63) {
        const __int128 one = (__int128)1 << F;
        c[n++] = -one - 1; c[n++] = -one; c[n++] = one - 1; c[n++] = one; c[n++] = one + 1;
        if (F >= 1) { c[n++] = -(one >> 1); c[n++] = one >> 1; }
    }
    int m = 0;
    for (int i = 0; i < n; ++i) {
        if (c[i] < lo || c[i] > hi) continue;
        int j = m;                                  /* insertion into the sorted, distinct list */
        while (j > 0 && out[j - 1] > (int64_t)c[i]) --j;
        if (j > 0 && out[j - 1] == (int64_t)c[i]) continue;
        for (int k = m; k > j; --k) out[k] = out[k - 1];
        out[j] = (int64_t)c[i];
        ++m;
    }
    return m;
}

int64_t qoracle_synth(qfmt f, uint64_t seed, int dist, uint64_t elem, int part)
{
    int W = (int)f.I + (int)f.F;
    int b = dist == 1 ? W / 2 : W;
    int bits = b + (f.S ? 1 : 0);
    if (bits <= 0) return 0;
    uint64_t r = qo_rand(seed, elem * 2 + (uint64_t)part);
    if (dist == 2 && (r & 1)) {
        int64_t e[14];
        const int n = qo_edges(f, e);
        return e[(r >> 1) % (uint64_t)n];
    }
    uint64_t v = bits >= 64 ? r : (r >> (64 - bits));
    uint64_t lo = f.S ? (uint64_t)0 - ((uint64_t)1 << b) : 0;   /* unsigned arithmetic: well defined for b = 63 too */
    return (int64_t)(lo + v);
}

/* fill a tight host-layout tensor of n elements */
void qoracle_fill(const qfmt* f2, int is_complex, uint64_t seed, int dist, int64_t n, void* out)
{
    qo_layout L = qo_elem_layout(f2, is_complex);
    char* p = (char*)out;
    for (int64_t e = 0; e < n; ++e, p += L.size) {
        if (L.size > L.sb[0] + L.sb[1]) memset(p, 0, (size_t)L.size);
        for (int q = 0; q < (is_complex ? 2 : 1); ++q)
            qo_store(p + L.off[q], L.sb[q], qoracle_synth(f2[q], seed, dist, (uint64_t)e, q));
    }
}
