// qg_plan.cpp — descriptor analysis (host only).  See qg_plan.h.
#include "qg_plan.h"
#include "qg_approx.h"
#include "qg_cmul.h"

#include <math.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <vector>

typedef __int128 I128;

namespace {

struct Rng {
    I128 lo, hi;
};

int bits_of(I128 v)
{
    // signed width of v
    unsigned __int128 u = v < 0 ? (unsigned __int128)(~v) : (unsigned __int128)v;
    int n = 0;
    while (u) { ++n; u >>= 1; }
    return n + 1;
}

struct Ctx {
    QAnalysis* out;
    bool exact = true;      // every step so far was the identity
    int max_bits = 1;
    int max_bits_np = 1;    // the same, not counting full-precision products before their rounding
    int max_fmt_bits = 0;   // widest storage (1 + W) of any target format make_step has seen
    bool raw_product = false;
    bool band = false;      // a multi-word value in [2^63, 2^64) / [-2^64, -2^63) can reach a one-word target (through())
    bool final_step = false; // the conversion into C is being analysed (nothing follows it)
    bool raw_c = false;     // C's WRP::TCPL_SAT lets the root through unclamped: host-word containers, general kernels
    void fail(int st, const char* why)
    {
        if (out->status == QG_OK) {
            out->status = st;
            snprintf(out->reason, sizeof out->reason, "%.*s", (int)sizeof out->reason - 1, why);   // (a long reason is cut to the field, on purpose)
        }
    }
    void note(Rng r)
    {
        int b = bits_of(r.lo), c = bits_of(r.hi);
        if (c > b) b = c;
        if (b > max_bits) max_bits = b;
        if (!raw_product && b > max_bits_np) max_bits_np = b;
    }
    QStep make_step(int fromF, qfmt to, bool identity)
    {
        if (1 + (int)to.I + (int)to.F > max_fmt_bits) max_fmt_bits = 1 + (int)to.I + (int)to.F;
        QStep s;
        memset(&s, 0, sizeof s);
        s.d = fromF - (int)to.F;
        s.Q = to.Q;
        s.O = to.O;
        s.W = (int)to.I + (int)to.F;
        s.S = to.S;
        s.identity = identity ? 1 : 0;
        if (s.W <= 62) {   // (wide steps derive their bounds from W and S on the device: qg_overflow_w)
            s.hi = (int64_t)(((I128)1 << s.W) - 1);
            s.lo = to.S ? -(int64_t)((I128)1 << s.W) : 0;
        }
        return s;
    }
};

bool same(qfmt a, qfmt b) { return a.I == b.I && a.F == b.F && a.S == b.S && a.Q == b.Q && a.O == b.O; }

bool fmt_ok(Ctx& c, qfmt f)
{
    int W = (int)f.I + (int)f.F;
    if (W < 0) { c.fail(QG_EINVAL, "intBits + fracBits < 0"); return false; }
    if (f.Q > QG_TRN_SMGN) { c.fail(QG_EINVAL, "unknown QuMode code"); return false; }
    if (f.O > QG_WRP_TCPL_SAT) { c.fail(QG_EINVAL, "unknown OfMode code"); return false; }   // (WRP::TCPL_SAT: see through())
    if (W > 119) { c.fail(QG_EUNSUPPORTED, "format wider than 120 storage bits"); return false; }
    // ArbiInt<65>::maximum() is -1 (oneBits = 65 % 64 - 1 = 0 selects ~0 for the top word, QuBLAS.h:594-603): every saturating
    // conversion INTO a format of exactly 65 storage bits is an artefact in the reference (tests/golden/ref_wide_1: Qu<32,32>, Qu<64,0>)
    if (W == 64) { c.fail(QG_EUNSUPPORTED, "a format of exactly 65 storage bits: ArbiInt<65>::maximum() artefact of the reference"); return false; }
    return true;
}

Rng fmt_range(qfmt f)
{
    int W = (int)f.I + (int)f.F;
    Rng r;
    r.hi = ((I128)1 << W) - 1;
    r.lo = f.S ? -((I128)1 << W) : 0;
    return r;
}

// width of the ArbiInt that fracConvert returns for an n-bit input: shifts change the width by the shift (QuBLAS.h:1485-1701),
// the RND modes end in `Xh + ArbiInt<1>` — one bit more (:2032) —, TRN::TCPL / TRN::SMGN keep n - d (:2166, :2175-2178)
int round_width(int n, int d, int Q)
{
    if (d <= 0) return n - d;
    const int w = n - d < 1 ? 1 : n - d;
    return (Q == QG_TRN_TCPL || Q == QG_TRN_SMGN) ? w : w + 1;
}

// propagate an exact interval (raw values at frac fromF) through round + overflow into `to`.  nin: width of the ArbiInt TYPE
// the value has in the reference before this step (0: not tracked — element-wise chains, which stay within 62 bits); st: the
// step record, whose refcmp this sets.
Rng through(Ctx& c, Rng in, int fromF, qfmt to, bool identity, int nin = 0, QStep* st = nullptr)
{
    c.note(in);
    c.raw_product = false;
    if (identity) return in;
    // Converting INTO an unsigned WRP::TCPL format of exactly 32 value bits: the reference's mask is ArbiInt<32>::allOnes(),
    // whose data is -1 (QuBLAS.h:361-377), so `val & mask` (:2328-2331) masks nothing and the value is stored unwrapped in
    // the 33-bit storage (-7 -> -7, 2^33 + 5 -> 2^33 + 5; pinned by tests/golden ref_scalar cvt tables).  An artefact of
    // the same family as the d = 32 RND case below: rejected, not imitated.  (Signed, 32 storage bits: the reference's
    // int32 storage wraps by itself and agrees with the arithmetic definition.)  Checked BELOW, only where a value can actually
    // leave the range: an in-range value is untouched by the reference's `val & allOnes` too (uint32-style formats run).
    int d = fromF - (int)to.F;
    Rng r = in;
    if (d <= 0) {
        if (-d > 100 || bits_of(in.lo) - d > 126 || bits_of(in.hi) - d > 126) { c.fail(QG_EUNSUPPORTED, "left shift beyond 127 bits"); return in; }
        r.lo = in.lo * ((I128)1 << -d);
        r.hi = in.hi * ((I128)1 << -d);
        c.note(r);
    } else {
        if (d > 119) { c.fail(QG_EUNSUPPORTED, "rounding shift beyond 119 bits"); return in; }
        if ((d == 32 || d == 64) && to.Q <= QG_RND_CONV)
            c.fail(QG_EUNSUPPORTED, "RND over a 32/64-bit shift: reference result is an ArbiInt<32>::allOnes artefact");
        // RND::CONV of a multi-word value: the reference's floor / ceil construction (QuBLAS.h:2137-2156) returns artefacts (every
        // RND::CONV table of tests/golden/ref_wide_* with a source wider than 64 bits differs from round-half-to-even)
        if (to.Q == QG_RND_CONV && nin > 64)
            c.fail(QG_EUNSUPPORTED, "RND::CONV of a value wider than 64 bits: multi-word artefact of the reference");
        c.exact = false;
        r.lo = in.lo >> d;
        r.hi = (in.hi >> d) + 1;
    }
    const int nr = nin ? round_width(nin, d, to.Q) : 0;   // type width of what reaches the overflow handling
    const int mbits = 1 + (int)to.I + (int)to.F;
    // signed WRP::TCPL from one multi-word type into another of a different width: operator| of two wide integers of different
    // sizes is ill-formed (QuBLAS.h:1946-1950) — the reference does not compile such a conversion (oracle/ref_cases_wide_probe.log)
    if (to.O == QG_WRP_TCPL && to.S && mbits > 64 && nr > 64 && nr != mbits)
        c.fail(QG_EUNSUPPORTED, "signed WRP::TCPL between multi-word types of different widths: the reference does not compile it");
    Rng R = fmt_range(to);
    Rng Re = R;
    if (to.O == QG_SAT_SMGN) Re.lo = to.S ? -R.hi : 0;
    if (to.O == QG_WRP_TCPL_SAT) {
        // WRP::TCPL_SAT<N> is a stub in the reference: intConvert returns its input (QuBLAS.h:2336-2344) and the assignment into the
        // target's storage narrows it to the storage WORD (int32_t / int64_t, never masked to the format's bits: :353, :431-441;
        // tests/golden/ref_scalar_9, ref_gemm_real_8).  In range that is the identity; out of range the value leaves its format,
        // and what the reference's next operation would make of it (int32_t arithmetic on a word that holds more bits than its
        // type says) is not something to build on: accepted only where nothing follows — the conversion into C.
        if (r.lo >= R.lo && r.hi <= R.hi) { if (st) st->O = QG_SAT_TCPL; return r; }   // (any in-range overflow mode: a clamp that never fires)
        if (!c.final_step) { c.fail(QG_EUNSUPPORTED, "WRP::TCPL_SAT (a stub in the reference) whose value can leave its format before the last conversion"); return r; }
        c.exact = false;
        c.raw_c = true;
        const I128 full = mbits <= 32 ? ((I128)1 << 31) : mbits <= 64 ? ((I128)1 << 63) : ((I128)1 << 126);
        if (r.lo < -full) r.lo = -full;
        if (r.hi > full - 1) r.hi = full - 1;
        return r;
    }
    if (nr > 64 && mbits <= 64 && to.O <= QG_SAT_SMGN) {
        // a multi-word value compared with one-word bounds: the reference reads the low word as a signed number (operator<=>,
        // QuBLAS.h:1781-1793) and narrows by keeping the low word (:436-441).  Identical to the arithmetic definition unless the
        // value lies in [2^63, 2^64) or [-2^64, -2^63); the kernels reproduce it (QStep::refcmp, qg_overflow_w).
        if (st) st->refcmp = 1;
        const I128 b63 = (I128)1 << 63, b64 = (I128)1 << 64;
        if ((r.hi >= b63 && r.lo < b64) || (r.lo < -b63 && r.hi >= -b64)) {
            // ... reachable: such a value comes out as its low word, whatever the format says (int32_t / int64_t storage)
            c.exact = false;
            c.band = true;
            const I128 full = mbits <= 32 ? ((I128)1 << 31) : ((I128)1 << 63);
            Rng q = r;
            if (q.lo < Re.lo) q.lo = Re.lo;
            if (q.hi > Re.hi) q.hi = Re.hi;
            if (to.O == QG_SAT_ZERO) { if (q.lo > 0) q.lo = 0; if (q.hi < 0) q.hi = 0; }
            if (q.lo > -full) q.lo = -full;
            if (q.hi < full - 1) q.hi = full - 1;
            return q;
        }
    }
    if (r.lo >= Re.lo && r.hi <= Re.hi) return r; // overflow handling is the identity
    c.exact = false;
    if (to.O == QG_WRP_TCPL && !to.S && (int)to.I + (int)to.F == 32)
        c.fail(QG_EUNSUPPORTED, "unsigned WRP::TCPL into exactly 32 bits: reference result is an ArbiInt<32>::allOnes artefact");
    switch (to.O) {
    case QG_SAT_TCPL:
    case QG_SAT_SMGN:
        if (r.lo < Re.lo) r.lo = Re.lo;
        if (r.hi > Re.hi) r.hi = Re.hi;
        if (r.lo > Re.hi) r.lo = Re.hi;
        if (r.hi < Re.lo) r.hi = Re.lo;
        return r;
    case QG_SAT_ZERO: {
        Rng q = r;
        if (q.lo < Re.lo) q.lo = Re.lo;
        if (q.hi > Re.hi) q.hi = Re.hi;
        if (q.lo > 0) q.lo = 0;
        if (q.hi < 0) q.hi = 0;
        if (q.lo > q.hi) { q.lo = 0; q.hi = 0; }
        return q;
    }
    default:
        return R; // wrap: anything representable
    }
}

Rng mul_rng(Rng a, Rng b)
{
    I128 p[4] = {a.lo * b.lo, a.lo * b.hi, a.hi * b.lo, a.hi * b.hi};
    Rng r = {p[0], p[0]};
    for (int i = 1; i < 4; ++i) {
        if (p[i] < r.lo) r.lo = p[i];
        if (p[i] > r.hi) r.hi = p[i];
    }
    return r;
}

struct Val {
    Rng r;
    qfmt f;
};
Val whole(qfmt f) { return Val{fmt_range(f), f}; }       // any value of the format
int sbits(qfmt f) { return 1 + (int)f.I + (int)f.F; }   // storage bits = width of the value's ArbiInt type (QuBLAS.h:2384-2385)
int rng_bits(Rng r) { const int a = bits_of(r.lo), b = bits_of(r.hi); return a > b ? a : b; }

Val do_mul(Ctx& c, Val a, Val b, qfmt res, QNode* node)
{
    node->sa = node->sb = 0;
    node->q = c.make_step((int)a.f.F + (int)b.f.F, res, false);
    Val v = whole(res);
    if (rng_bits(a.r) + rng_bits(b.r) > 127) { c.fail(QG_EUNSUPPORTED, "a product needs more than 127 bits"); return v; }
    c.raw_product = true; // the unrounded product is noted for max_bits only
    // operator*: an N-bit by an M-bit integer gives N + M bits (QuBLAS.h:1186-1207)
    v.r = through(c, mul_rng(a.r, b.r), (int)a.f.F + (int)b.f.F, res, false, sbits(a.f) + sbits(b.f), &node->q);
    return v;
}

Val do_addsub(Ctx& c, Val a, Val b, qfmt res, bool sub, QNode* node)
{
    int fm = a.f.F > b.f.F ? a.f.F : b.f.F;
    node->sa = fm - a.f.F;
    node->sb = fm - b.f.F;
    node->q = c.make_step(fm, res, false);
    Val v = whole(res);
    if (rng_bits(a.r) + node->sa > 125 || rng_bits(b.r) + node->sb > 125) { c.fail(QG_EUNSUPPORTED, "an aligned operand needs more than 126 bits"); return v; }
    Rng x = {a.r.lo * ((I128)1 << node->sa), a.r.hi * ((I128)1 << node->sa)};
    Rng y = {b.r.lo * ((I128)1 << node->sb), b.r.hi * ((I128)1 << node->sb)};
    c.note(x);
    c.note(y);
    // the aligned operands are N + shift bits wide, their sum / difference one bit more than the wider one (QuBLAS.h:914-1010)
    const int na = sbits(a.f) + node->sa, nb = sbits(b.f) + node->sb;
    // operator-(multi-word, one-word) loses the borrow / sign extension of the one-word operand (tests/golden/ref_wide_2:
    // Qsub(Qu<43,32>, Qu<31,32>) is off by multiples of 2^63): an artefact, rejected
    if (sub && na > 64 && nb <= 64) c.fail(QG_EUNSUPPORTED, "Qsub of a one-word value from a multi-word one: artefact of the reference's operator-");
    Rng s = sub ? Rng{x.lo - y.hi, x.hi - y.lo} : Rng{x.lo + y.lo, x.hi + y.hi};
    v.r = through(c, s, fm, res, false, (na > nb ? na : nb) + 1, &node->q);
    return v;
}

Val do_cvt(Ctx& c, Val a, qfmt to, QStep* st)
{
    bool id = same(a.f, to);
    *st = c.make_step((int)a.f.F, to, id);
    return Val{through(c, a.r, (int)a.f.F, to, id, sbits(a.f), st), to};
}

// One complex multiplication (a + b i)(c + d i) by the Basic or the TF multiplier, sub-operation by sub-operation in
// the slot order of include/qgemul.h: result formats m[], nodes into nd[], the real and the imaginary part into part[]
void do_cmul(Ctx& c, bool tf, Val a, Val b, Val cc, Val dd, const qfmt* m, QNode* nd, Val part[2])
{
    if (tf) {
        const Val ab = do_addsub(c, a, b, m[QG_T_AB], false, &nd[QG_T_AB]), cd = do_addsub(c, cc, dd, m[QG_T_CD], false, &nd[QG_T_CD]);
        const Val ba = do_addsub(c, b, a, m[QG_T_BA], true, &nd[QG_T_BA]);
        const Val A = do_mul(c, ab, cc, m[QG_T_A], &nd[QG_T_A]), B = do_mul(c, cd, b, m[QG_T_B], &nd[QG_T_B]), C = do_mul(c, ba, dd, m[QG_T_C], &nd[QG_T_C]);
        part[0] = do_addsub(c, A, B, m[QG_T_RE], true, &nd[QG_T_RE]);
        part[1] = do_addsub(c, B, C, m[QG_T_IM], true, &nd[QG_T_IM]);
    } else {
        const Val ac = do_mul(c, a, cc, m[QG_B_AC], &nd[QG_B_AC]), bd = do_mul(c, b, dd, m[QG_B_BD], &nd[QG_B_BD]);
        const Val ad = do_mul(c, a, dd, m[QG_B_AD], &nd[QG_B_AD]), bc = do_mul(c, b, cc, m[QG_B_BC], &nd[QG_B_BC]);
        part[0] = do_addsub(c, ac, bd, m[QG_B_RE], true, &nd[QG_B_RE]);
        part[1] = do_addsub(c, ad, bc, m[QG_B_IM], false, &nd[QG_B_IM]);
    }
}


// RING plans of the linear class (qg_mfma_ring.hip).  A real descriptor whose product format R = mul[0] is signed WRP::TCPL
// with n = W_R + 1 <= 32 bits, whose product shift d = F_a + F_b - F_R is <= 0 (an exact left shift s = -d < n: nothing is ever
// rounded), and whose every level_add / level format has R's (I, F, S) and WRP::TCPL (the QuMode may differ: there is nothing
// to round), with operands of at most 32 storage bits, evaluates to
//     C[i,j] = cvt_C( wrap_R( 2^s * sum_k a_ik b_kj ) ),      wrap_R(x) = the representative of x mod 2^n in [-2^(n-1), 2^(n-1)).
// Proof.  wrap_R is the canonical map Z -> Z / 2^n Z followed by the choice of a representative, and
//   * Qmul<R>(a, b) = wrap_R(a b 2^s): the product is exact (QuBLAS.h:1186-1207), the shift is exact, the overflow step wraps;
//   * Qadd<R>(x, y) = wrap_R(x + y): equal fraction bits, no alignment, no rounding; the store into the level buffer of the same
//     (I, F, S) and WRP::TCPL re-wraps a value that is already canonical: the identity;
//   * the odd-leftover copy converts a value of R into the same range: the identity;
// so by induction over the tree every node is the canonical representative of 2^s * (sum of the leaves below it) mod 2^n: the
// class of a sum is the sum of the classes.  The root is wrap_R(2^s * sum_k a_ik b_kj) whatever the tree's shape; zero leaves
// (padding) add the class of 0.  The operands' own modes never act inside Qgemul (they are stored values), and C's converting
// assignment sees a value of at most 32 bits.  Kept out: an unsigned R (its 32-bit case is the reference's allOnes() artefact,
// through() above), complex descriptors, levels of another width, any saturating level, any d > 0 — those round or clamp
// between the additions and are no homomorphisms.  C: any format the 64-bit step converts a 32-bit value into (at most 62 value
// bits, shifts that stay inside int64, no value that can leave its format: `c_leaves`).
void ring_plan(const qgemul_desc* d, bool c_leaves, QAnalysis* out)
{
    out->ring_ok = out->ring_n = out->ring_s = 0;
    if (d->is_complex || c_leaves) return;
    const qfmt R = d->mul[0];
    const int n = (int)R.I + (int)R.F + 1;
    if (R.O != QG_WRP_TCPL || !R.S || n < 1 || n > 32) return;
    const int s = (int)R.F - ((int)d->a[0].F + (int)d->b[0].F);
    if (s < 0 || s >= n) return;
    for (uint32_t l = 0; l < d->n_levels; ++l)
        for (const qfmt f : {d->level_add[0][l], d->level[0][l]})
            if (f.I != R.I || f.F != R.F || f.S != R.S || f.O != QG_WRP_TCPL) return;
    if (sbits(d->a[0]) > 32 || sbits(d->b[0]) > 32) return;
    const QStep& q = out->tree.c_cvt[0];
    if (!q.identity && (q.W > 62 || q.d < -30 || q.d > 61 || q.O > QG_WRP_TCPL || q.refcmp)) return;
    out->ring_ok = 1;
    out->ring_n = n;
    out->ring_s = s;
}

} // namespace

int qg_analyze_ep(qfmt cfmt, const qgemul_epilogue* ep, QEpTable* out, int* max_bits, char* reason, size_t reason_len)
{
    return qg_analyze_epx(cfmt, ep, nullptr, out, nullptr, max_bits, reason, reason_len);
}

namespace {

// One APPROX stage (include/qgemul.h): validates the table, walks every segment's Horner chain through the same range tracking as
// any other node, fills the device table.  x: the running value, replaced by the stage's result (x's own format; the hull of the
// segments' result ranges).  ok32: cleared when a step or a constant of the stage does not fit the 32-bit form of the pass.
bool approx_stage(Ctx& c, const qgemul_ew_stage& s, const qgemul_approx& A, Val& x, QApproxTable* T, bool* ok32)
{
    static const qfmt zero = {0, 0, 0, 0, 0, 0};
    if (s.x_first || s.e_scalar || !same(s.e, zero)) { c.fail(QG_EINVAL, "APPROX stage: e, e_scalar and x_first must be zero"); return false; }
    if (!same(s.r, x.f)) { c.fail(QG_EINVAL, "APPROX stage: r must be the running value's own format (Qapprox returns decltype(x))"); return false; }
    if (A.n_seg < 1 || A.n_seg > QG_MAX_SEG) { c.fail(QG_EINVAL, "APPROX table: n_seg outside 1..16"); return false; }
    for (uint32_t g = 0; g < A.n_seg; ++g) {
        const qgemul_approx_seg& sg = A.seg[g];
        if (sg.n_coef < 1 || sg.n_coef > QG_MAX_COEF) { c.fail(QG_EINVAL, "APPROX table: n_coef outside 1..8"); return false; }
        if (sg.breakpoint != sg.breakpoint) { c.fail(QG_EINVAL, "APPROX table: a NaN breakpoint"); return false; }
        for (uint32_t i = 0; i < sg.n_coef; ++i) {
            if (!fmt_ok(c, sg.f[i])) return false;
            if ((int)sg.f[i].I + (int)sg.f[i].F > 62) { c.fail(QG_EUNSUPPORTED, "APPROX table: a Horner format wider than 62 value bits"); return false; }
            const Rng r = fmt_range(sg.f[i]);
            if (sg.a[i] < r.lo || sg.a[i] > r.hi) { c.fail(QG_EINVAL, "APPROX table: a coefficient outside its format"); return false; }
            if (sbits(sg.f[i]) > 32) *ok32 = false;
        }
    }
    const int Wx = (int)x.f.I + (int)x.f.F;
    // x.toDouble() is double(raw) / 2^F (QuBLAS.h:2413-2416): exact, and the comparison an integer one, up to 53 value bits
    if (Wx > 53) { c.fail(QG_EUNSUPPORTED, "APPROX stage: x has more than 53 value bits (toDouble() rounds)"); return false; }
    if (Wx > 30) *ok32 = false;   // (the clamped threshold hi + 1 = 2^31 is no int32 value)
    if (T) memset(T, 0, sizeof *T);
    const Rng xr = fmt_range(x.f);
    Rng res = {0, 0};
    QApproxSeg first;
    bool uniform = true;
    int ncmax = 0;
    for (uint32_t g = 0; g < A.n_seg; ++g) {
        const qgemul_approx_seg& sg = A.seg[g];
        const int n = (int)sg.n_coef;
        QApproxSeg S;
        memset(&S, 0, sizeof S);
        S.n_coef = n;
        Val v;
        v.f = sg.f[n - 1];
        v.r = Rng{(I128)sg.a[n - 1], (I128)sg.a[n - 1]};
        for (int i = n - 2; i >= 0; --i) {
            QNode nm, na;
            const Val p = do_mul(c, x, v, sg.f[i], &nm);
            Val a;
            a.f = sg.f[i];
            a.r = Rng{(I128)sg.a[i], (I128)sg.a[i]};
            v = do_addsub(c, a, p, sg.f[i], false, &na);
            S.lvl[i].mul = nm.q;
            S.lvl[i].add = na.q;
            if (nm.q.d > 62) { c.fail(QG_EUNSUPPORTED, "APPROX stage: rounding shift beyond 62 bits"); return false; }
            if (nm.q.d > 30) *ok32 = false;
        }
        const Val y = do_cvt(c, v, x.f, &S.to_x);
        if (!S.to_x.identity && S.to_x.d > 62) { c.fail(QG_EUNSUPPORTED, "APPROX stage: rounding shift beyond 62 bits"); return false; }
        if (!S.to_x.identity && S.to_x.d > 30) *ok32 = false;
        if (c.out->status != QG_OK) return false;
        res = g ? Rng{y.r.lo < res.lo ? y.r.lo : res.lo, y.r.hi > res.hi ? y.r.hi : res.hi} : y.r;
        if (n > ncmax) ncmax = n;
        // uniform = the formats agree, nothing else: the step records follow from the formats (make_step), except refcmp, which only
        // the 128-bit kernels read, and WRP::TCPL_SAT's rewrite into a clamp, which every accepted segment gets alike
        if (!g) first = S;
        else if (n != first.n_coef) uniform = false;
        for (int i = 0; g && i < n && uniform; ++i) uniform = same(sg.f[i], A.seg[0].f[i]);
        if (g && uniform) {
            QApproxSeg a = S, b = first;
            a.to_x.refcmp = b.to_x.refcmp = 0;
            for (int i = 0; i + 1 < n; ++i) a.lvl[i].mul.refcmp = a.lvl[i].add.refcmp = b.lvl[i].mul.refcmp = b.lvl[i].add.refcmp = 0;
            if (memcmp(&a, &b, sizeof a)) { c.fail(QG_EUNSUPPORTED, "APPROX table: equal formats resolved to different steps (planner invariant)"); return false; }
        }
        if (T) {
            T->seg[g] = S;
            for (int i = 0; i < n; ++i) T->coef[i][g] = sg.a[i];
        }
    }
    if (T) {
        T->n_seg = (int)A.n_seg;
        T->uniform = uniform ? 1 : 0;
        T->n_coef_max = ncmax;
        const int64_t lo = (int64_t)xr.lo, hi1 = (int64_t)xr.hi + 1;
        for (int g = 0; g < QG_MAX_SEG; ++g) {
            int64_t t = hi1;
            if (g + 1 < (int)A.n_seg) {
                // raw / 2^F < bp  <=>  raw < bp * 2^F  <=>  raw < ceil(bp * 2^F): the scaling is exact in double unless it leaves the
                // double range, and then the result lies far outside [lo, hi + 1] (or, underflowing, inside (0, 1): ceil = 1)
                const double bp = A.seg[g].breakpoint;
                double sc = ldexp(bp, (int)x.f.F);
                if (bp > 0 && sc < 1) sc = 1;
                else sc = ceil(sc);
                t = sc <= (double)lo ? lo : (sc >= (double)hi1 ? hi1 : (int64_t)sc);
            }
            T->thr[g] = t;
        }
    }
    x.r = res;
    return true;
}

int ep_pow2_bytes(qfmt f)
{
    int b = (1 + (int)f.I + (int)f.F + 7) / 8, r = 1;
    while (r < b) r *= 2;
    return r;
}

// the chain kernels are 64-bit only: make_step gives a step bounds only up to 62 value bits
bool chain_fmt_ok(Ctx& c, qfmt f)
{
    if (!fmt_ok(c, f)) return false;
    if ((int)f.I + (int)f.F > 62) { c.fail(QG_EUNSUPPORTED, "element-wise chain format wider than 62 value bits"); return false; }
    return true;
}

// a stage that reads no operand (PASS, APPROX, and what a CMUL stage starts from): nothing acts yet
void no_operand_stage(QEpStage& t, int op)
{
    memset(&t, 0, sizeof t);
    t.op = op;
    t.scalar = 1;
    t.ebytes = 1;
    t.node.q.identity = 1;
    t.cvt.identity = 1;
}

// the assignment of a stage's result x to the stage's tensor (`last`: the last stage's result goes into D instead, by the caller's to_d)
bool to_stage_tensor(Ctx& c, const qgemul_ew_stage& s, bool last, Val& x, QStep* cvt)
{
    if (last) return true;
    if (!chain_fmt_ok(c, s.t)) return false;
    x = do_cvt(c, x, s.t, cvt);
    return true;
}

// One ADD / SUB / MUL / PASS stage: x, the running value, is replaced by the stage's result as assigned to the stage's tensor
bool plain_stage(Ctx& c, const qgemul_ew_stage& s, bool last, Val& x, QEpStage& t)
{
    if (s.op == QG_EW_PASS) {
        // the part is carried over in its own format (the imaginary part under a real operand, QuBLAS.h:3654/3670/3701);
        // only the assignment to the stage's tensor touches it
        no_operand_stage(t, QG_EW_PASS);
        return to_stage_tensor(c, s, last, x, &t.cvt);
    }
    if (!chain_fmt_ok(c, s.e) || !chain_fmt_ok(c, s.r)) return false;
    const Val e = whole(s.e);
    t.op = s.op;
    t.x_first = s.x_first ? 1 : 0;
    t.scalar = s.e_scalar ? 1 : 0;
    t.ebytes = ep_pow2_bytes(s.e);
    const Val& first = t.x_first ? x : e;
    const Val& second = t.x_first ? e : x;
    x = s.op == QG_EW_MUL ? do_mul(c, first, second, s.r, &t.node) : do_addsub(c, first, second, s.r, s.op == QG_EW_SUB, &t.node);
    memset(&t.cvt, 0, sizeof t.cvt);
    t.cvt.identity = 1;
    return to_stage_tensor(c, s, last, x, &t.cvt);
}

bool shift32_ok(const QStep& q) { return q.identity || q.d <= 30; }

// the range tracking of a chain: its QAnalysis only carries the status and the reason
struct ChainCtx : Ctx {
    ChainCtx() { out = new QAnalysis; memset(out, 0, sizeof *out); out->status = QG_OK; }
    ~ChainCtx() { delete out; }
    int answer(int* bits, char* reason, size_t reason_len) const
    {
        if (reason && reason_len) snprintf(reason, reason_len, "%s", out->reason);
        if (bits) *bits = max_bits;
        return out->status;
    }
};

} // namespace

int qg_analyze_epx(qfmt cfmt, const qgemul_epilogue* ep, const qgemul_approx* const* ax, QEpTable* out, QApproxTable* axt, int* max_bits, char* reason,
                   size_t reason_len)
{
    memset(out, 0, sizeof *out);
    bool ax32 = true;
    ChainCtx c;
    do {
        if (!ep || ep->n_stages > QG_MAX_EW) { c.fail(QG_EINVAL, "null epilogue or too many stages"); break; }
        if (!chain_fmt_ok(c, cfmt) || !chain_fmt_ok(c, ep->d)) break;
        Val x = whole(cfmt);
        bool ok = true;
        for (uint32_t k = 0; k < ep->n_stages && ok; ++k) {
            const qgemul_ew_stage& s = ep->stage[k];
            if (s.op < QG_EW_ADD || s.op > (ax ? QG_EW_APPROX : QG_EW_PASS)) { c.fail(QG_EINVAL, "unknown element-wise op"); ok = false; break; }
            if (ax && (s.op == QG_EW_APPROX) != (ax[k] != nullptr)) {
                c.fail(QG_EINVAL, s.op == QG_EW_APPROX ? "APPROX stage without its table" : "a table for a stage that is no APPROX stage");
                ok = false;
                break;
            }
            if (s.op == QG_EW_APPROX) {
                no_operand_stage(out->st[k], QG_EW_APPROX);
                ok = approx_stage(c, s, *ax[k], x, axt ? &axt[k] : nullptr, &ax32) && to_stage_tensor(c, s, k + 1 == ep->n_stages, x, &out->st[k].cvt);
                continue;
            }
            ok = plain_stage(c, s, k + 1 == ep->n_stages, x, out->st[k]);
        }
        if (!ok) break;
        for (uint32_t k = ep->n_stages; ax && k < QG_MAX_EW; ++k)
            if (ax[k]) { c.fail(QG_EINVAL, "a table beyond the last stage"); ok = false; }
        if (!ok) break;
        do_cvt(c, x, ep->d, &out->to_d);
        out->n = (int)ep->n_stages;
        out->dbytes = ep_pow2_bytes(ep->d);
        out->max_bits = c.max_bits;
        {
            // 32-bit arithmetic: every intermediate (raw products and aligned operands included) within 32 bits, every
            // format within 32 storage bits, every rounding shift below 31
            bool ok32 = ax32 && c.max_bits <= 32 && c.max_fmt_bits <= 32 && 1 + (int)cfmt.I + (int)cfmt.F <= 32;
            for (int k = 0; k < out->n; ++k) ok32 = ok32 && shift32_ok(out->st[k].node.q) && shift32_ok(out->st[k].cvt) && out->st[k].ebytes <= 4;
            out->bits32 = (ok32 && shift32_ok(out->to_d)) ? 1 : 0;
        }
        if (c.max_bits > 62) c.fail(QG_EUNSUPPORTED, "epilogue intermediate wider than 62 bits");
    } while (0);
    return c.answer(max_bits, reason, reason_len);
}

// A complex chain with CMUL stages (qg_cmul.h): the two part chains in lock step, since a CMUL stage needs both running values.
// Every sub-operation goes through do_mul / do_addsub / do_cvt on the parts' whole ranges, so max_bits, bits32 and every refusal
// of a plain chain hold here with no rule of their own.
int qg_analyze_epcx(const qfmt cf[2], const qgemul_epilogue_cplx* ep, const qgemul_cmul* const* cx, QEpTable t[2], QCmulStage* cmt, int* max_bits,
                    char* reason, size_t reason_len)
{
    memset(t, 0, 2 * sizeof *t);
    if (cmt) memset(cmt, 0, QG_MAX_EW * sizeof *cmt);
    ChainCtx c;
    do {
        if (!ep || !cx || ep->part[0].n_stages > QG_MAX_EW) { c.fail(QG_EINVAL, "null epilogue or too many stages"); break; }
        if (ep->part[1].n_stages != ep->part[0].n_stages) { c.fail(QG_EINVAL, "complex chain: the part chains differ in length"); break; }
        const uint32_t n = ep->part[0].n_stages;
        bool ok = true;
        Val x[2];
        for (int p = 0; p < 2 && ok; ++p) {
            ok = chain_fmt_ok(c, cf[p]) && chain_fmt_ok(c, ep->part[p].d);
            if (!ok) break;
            x[p] = whole(cf[p]);
        }
        bool cm32 = true;
        for (uint32_t k = 0; k < n && ok; ++k) {
            const qgemul_ew_stage* s[2] = {&ep->part[0].stage[k], &ep->part[1].stage[k]};
            const bool last = k + 1 == n;
            for (int p = 0; p < 2 && ok; ++p)
                if (s[p]->op < QG_EW_ADD || s[p]->op > QG_EW_CMUL || s[p]->op == QG_EW_APPROX) { c.fail(QG_EINVAL, "unknown element-wise op"); ok = false; }
            if (!ok) break;
            const bool cm = s[0]->op == QG_EW_CMUL;
            if (cm != (s[1]->op == QG_EW_CMUL)) { c.fail(QG_EINVAL, "CMUL stage: op 6 in one part only"); ok = false; break; }
            if (cm != (cx[k] != nullptr)) {
                c.fail(QG_EINVAL, cm ? "CMUL stage without its record" : "a CMUL record for a stage that is no CMUL stage");
                ok = false;
                break;
            }
            if (!cm) {
                for (int p = 0; p < 2 && ok; ++p) ok = plain_stage(c, *s[p], last, x[p], t[p].st[k]);
                continue;
            }
            const qgemul_cmul& M = *cx[k];
            if ((s[0]->x_first != 0) != (s[1]->x_first != 0) || (s[0]->e_scalar != 0) != (s[1]->e_scalar != 0)) {
                c.fail(QG_EINVAL, "CMUL stage: x_first / e_scalar differ between the parts");
                ok = false;
                break;
            }
            if (!ep->e_complex[k]) { c.fail(QG_EINVAL, "CMUL stage: the operand is complex (e_complex = 1)"); ok = false; break; }
            if (M.cmul != QG_CMUL_BASIC && M.cmul != QG_CMUL_TF) { c.fail(QG_EINVAL, "CMUL stage: cmul is neither Basic nor TF"); ok = false; break; }
            const bool tf = M.cmul == QG_CMUL_TF;
            const int n_nodes = tf ? 8 : 6, RE = tf ? QG_T_RE : QG_B_RE, IM = tf ? QG_T_IM : QG_B_IM;
            if (!same(s[0]->r, M.mul[RE]) || !same(s[1]->r, M.mul[IM])) { c.fail(QG_EINVAL, "CMUL stage: r is not the RE / IM slot of mul[]"); ok = false; break; }
            for (int i = 0; i < n_nodes && ok; ++i) ok = chain_fmt_ok(c, M.mul[i]);
            for (int p = 0; p < 2 && ok; ++p) ok = chain_fmt_ok(c, s[p]->e);
            if (!ok) break;
            const Val e[2] = {whole(s[0]->e), whole(s[1]->e)};
            const bool xf = s[0]->x_first != 0;
            const Val &a = xf ? x[0] : e[0], &b = xf ? x[1] : e[1], &cc = xf ? e[0] : x[0], &d = xf ? e[1] : x[1];
            QNode nd[8];
            memset(nd, 0, sizeof nd);
            Val part[2];
            do_cmul(c, tf, a, b, cc, d, M.mul, nd, part);
            for (int i = 0; i < n_nodes; ++i) cm32 = cm32 && shift32_ok(nd[i].q);
            const int eb = ep_pow2_bytes(s[0]->e) > ep_pow2_bytes(s[1]->e) ? ep_pow2_bytes(s[0]->e) : ep_pow2_bytes(s[1]->e);
            for (int p = 0; p < 2 && ok; ++p) {
                QEpStage& q = t[p].st[k];
                no_operand_stage(q, QG_EW_CMUL);
                q.x_first = xf ? 1 : 0;
                q.scalar = s[0]->e_scalar ? 1 : 0;
                q.ebytes = eb;
                q.node = nd[p ? IM : RE];
                x[p] = part[p];
                ok = to_stage_tensor(c, *s[p], last, x[p], &q.cvt);
            }
            if (cmt) {
                QCmulStage& q = cmt[k];
                q.cmul = M.cmul;
                q.x_first = xf ? 1 : 0;
                q.scalar = s[0]->e_scalar ? 1 : 0;
                q.ebytes = eb;
                memcpy(q.n, nd, sizeof nd);
            }
        }
        if (!ok) break;
        for (uint32_t k = n; k < QG_MAX_EW; ++k)
            if (cx[k]) { c.fail(QG_EINVAL, "a CMUL record beyond the last stage"); ok = false; }
        if (!ok) break;
        for (int p = 0; p < 2; ++p) {
            do_cvt(c, x[p], ep->part[p].d, &t[p].to_d);
            t[p].n = (int)n;
            t[p].dbytes = ep_pow2_bytes(ep->part[p].d);
        }
        // the one pass runs in 32-bit arithmetic when that holds for both chains and every CMUL node
        bool ok32 = cm32 && c.max_bits <= 32 && c.max_fmt_bits <= 32 && sbits(cf[0]) <= 32 && sbits(cf[1]) <= 32;
        for (int p = 0; p < 2; ++p) {
            for (uint32_t k = 0; k < n; ++k) ok32 = ok32 && shift32_ok(t[p].st[k].node.q) && shift32_ok(t[p].st[k].cvt) && t[p].st[k].ebytes <= 4;
            ok32 = ok32 && shift32_ok(t[p].to_d);
        }
        for (int p = 0; p < 2; ++p) {
            t[p].bits32 = ok32 ? 1 : 0;
            t[p].max_bits = c.max_bits;
        }
        if (c.max_bits > 62) c.fail(QG_EUNSUPPORTED, "epilogue intermediate wider than 62 bits");
    } while (0);
    return c.answer(max_bits, reason, reason_len);
}

QHostElem qg_host_elem(const qfmt f[2], int is_complex)
{
    QHostElem L;
    // int32_t / int64_t (ArbiInt<N <= 64>, QuBLAS.h:353) or two little-endian uint64_t words (ArbiInt<65..128>, :572-573; 8-byte aligned)
    auto sb = [](qfmt q) { const int b = 1 + (int)q.I + (int)q.F; return b <= 32 ? 4 : b <= 64 ? 8 : 16; };
    L.sb[0] = sb(f[0]);
    L.off[0] = 0;
    if (!is_complex) {
        L.sb[1] = 0;
        L.off[1] = 0;
        L.size = L.sb[0];
        return L;
    }
    L.sb[1] = sb(f[1]);
    const int a0 = L.sb[0] > 8 ? 8 : L.sb[0], a1 = L.sb[1] > 8 ? 8 : L.sb[1];
    const int al = a0 > a1 ? a0 : a1;
    L.off[1] = (L.sb[0] + a1 - 1) / a1 * a1;
    L.size = (L.off[1] + L.sb[1] + al - 1) / al * al;
    return L;
}

int qg_limbs_for(qfmt f)
{
    // balanced base-256 digits d in [-128,127]; the remainder after peeling n-1 digits is
    // floor((x + 128) / 256) applied n-1 times, monotone in x, so the extremes decide
    Rng r = fmt_range(f);
    for (int n = 1; n <= 8; ++n) {
        I128 lo = r.lo, hi = r.hi;
        for (int i = 1; i < n; ++i) {
            lo = (lo + 128) >> 8;
            hi = (hi + 128) >> 8;
        }
        if (lo >= -128 && hi <= 127) return n;
    }
    return 9;
}

int qg_limbs_centred(qfmt f, int64_t* centre)
{
    const Rng r = fmt_range(f);
    *centre = 0;
    I128 S = 0;
    for (int n = 1; n <= 7; ++n) {
        S = S * 256 + 1;                                  // (256^n - 1) / 255
        if (r.hi - r.lo <= 255 * S) {
            const I128 c = r.lo + 128 * S;                // lo - c = -128 S, hi - c <= 127 S
            if (c < -((I128)1 << 62) || c > ((I128)1 << 62)) return 9;
            *centre = (int64_t)c;
            return n;
        }
    }
    return 9;
}

namespace {

I128 mag(Rng r) { const I128 a = r.lo < 0 ? -r.lo : r.lo; return a > r.hi ? a : r.hi; }   // the largest magnitude of the range
int ilog2(int64_t k) { int n = 0; while (((int64_t)1 << n) < k) ++n; return n; }            // the smallest n with 2^n >= k
int width_of_hi(int64_t hi) { int n = 0; while (((int64_t)1 << n) <= hi) ++n; return n; }   // value bits n of an upper bound hi = 2^n - 1

// a rounding that is "add a constant, shift right by d": TRN::TCPL (+0), RND::POS_INF (+2^(d-1)), RND::NEG_INF (+2^(d-1) - 1) ...
bool adds_constant(const QStep& q) { return q.Q == QG_TRN_TCPL || q.Q == QG_RND_POS_INF || q.Q == QG_RND_NEG_INF; }
// ... and that constant (0 for every other mode: theirs depends on the value, rounding_kind)
int64_t round_addend(int Q, int d)
{
    if (d <= 0) return 0;
    const int64_t half = (int64_t)1 << (d - 1);
    return Q == QG_RND_POS_INF ? half : Q == QG_RND_NEG_INF ? half - 1 : 0;
}
// the value-dependent roundings and the overflows that are no clamp, as the kinds of the compact records (QFix, qg_plan.h; qg_fix.h)
int rounding_kind(const QStep& q)
{
    if (q.identity || q.d <= 0) return 0;
    return q.Q == QG_RND_ZERO ? 1 : q.Q == QG_RND_INF ? 2 : q.Q == QG_RND_CONV ? 3 : q.Q == QG_TRN_SMGN ? 4 : 0;
}
int overflow_kind(const QStep& q) { return q.O == QG_SAT_ZERO ? 1 : q.O == QG_WRP_TCPL ? (q.S ? 2 : 3) : 0; }
int64_t clamp_lo(const QStep& q) { return q.O == QG_SAT_SMGN ? (q.S ? -q.hi : 0) : q.lo; }   // (SAT::SMGN clamps to [-hi, hi])
// a step the compact records can hold (every QuMode: the value-dependent ones as a rounding kind; the overflows as kinds: QTF_REC_*, QCF_KINDS*)
bool compact_step_ok(const QStep& q)
{
    return q.identity || (q.d >= -22 && q.d <= 29 && (q.O == QG_SAT_TCPL || q.O == QG_SAT_SMGN || q.O == QG_SAT_ZERO || (q.O == QG_WRP_TCPL && q.W >= 1)));
}

// the compact record of a step of the REAL kernels: unbiased values, kb = the overflow kind, a value-dependent rounding as kind + constant
void real_record(const QStep& q, QFix* f)
{
    memset(f, 0, sizeof *f);
    f->ka = 1;
    if (q.identity) { f->lo = INT32_MIN; f->hi = INT32_MAX; return; }
    f->kb = overflow_kind(q);   // (qg_plan.h)
    f->lo = (int32_t)clamp_lo(q);
    f->hi = (int32_t)q.hi;
    if (q.d < 0) { f->ls = -q.d; return; }
    f->d = q.d;
    f->t = (int32_t)round_addend(q.Q, q.d);
    if (const int rk = rounding_kind(q)) {   // value-dependent roundings: kind + constant (qg_fix.h)
        const int32_t half = 1 << (q.d - 1);
        f->skip = rk;
        f->ka = rk == 2 ? half : rk == 4 ? (int32_t)(((int64_t)1 << q.d) - 1) : half - 1;
    }
}

// QTF_REC_BIASED: what a step's format means for a value kept biased by -lo: the overflow kind (0 clamp, 1 zero, 2 wrap, 4 none), the bias
// B = -lo and span = hi - lo
struct Biased { int kind; int64_t B, span; };
Biased biased_of(const QStep& q)
{
    if (q.identity) return {4, 0, 0};
    const int64_t lo = clamp_lo(q);
    return {q.O == QG_SAT_ZERO ? 1 : q.O == QG_WRP_TCPL ? 2 : 0, -lo, q.hi - lo};
}
// rewrites the unbiased record *f (its t, d, ls) as the biased one; bias_in2: the bias the inputs carry, summed.  False: too wide for the form
bool biased_record(const Biased& me, int64_t bias_in2, QFix* f)
{
    const QFix u = *f;
    memset(f, 0, sizeof *f);
    f->ka = 1;
    f->d = u.d;
    f->ls = u.ls;
    f->kb = me.kind;
    f->hi = (int32_t)me.span;
    f->lo = (int32_t)me.B;
    const int64_t cst = u.ls ? -bias_in2 : (int64_t)u.t - bias_in2 + (me.B << u.d);   // (left shift: B is added after it)
    f->t = (int32_t)cst;
    return me.span < (1ll << 30) && (me.B << u.d) < (1ll << 29) && cst > -(1ll << 30) && cst < (1ll << 30) && (me.B << u.ls) < (1ll << 30);
}

// The complex kernel's compact records (QFix).  kinds: any rounding / overflow kind met; feat: the branch-free feature bits they need
// (qg_fix.h, fx_finish_feat: 1 R, 2 Z, 4 W), -1 once a kind only the branching form covers was met (unsigned WRP::TCPL, TRN::SMGN by
// > 23 bits); bf: pack for the branch-free form (the second pass of cplx_records)
struct KindPacker {
    bool kinds = false, bf = false;
    int feat = 0;
    // the rounding / overflow part; returns the rounding factor k of the branch-free form
    int32_t pack(const QStep& q, QFix* f)
    {
        memset(f, 0, sizeof *f);
        f->ka = f->kb = 1;
        if (q.identity) { f->skip = bf ? (1 | 31 << 16 | 1 << 24) : 1; f->lo = INT32_MIN; f->hi = INT32_MAX; return 0; }
        f->lo = (int32_t)clamp_lo(q);
        f->hi = (int32_t)q.hi;
        const int ok = overflow_kind(q), rk = rounding_kind(q);
        kinds = kinds || rk || ok;
        if (ok == 3 || (rk == 4 && q.d > 23)) feat = -1;
        else if (feat >= 0) feat |= (rk ? 1 : 0) | (ok == 1 ? 2 : 0) | (ok == 2 || rk == 2 ? 4 : 0);
        int32_t k = 0;
        if (bf) {
            const int off = rk == 3 ? q.d : 31;
            int wd = ok == 2 ? q.W + 1 : 31;
            // RND::INF adds the INVERTED sign bit: the step's constant carries 2^31, which inverts bit 31 before it is read; the
            // shifted value is then right in its low 31 - d bits, which the wrap's sign-extraction (feature W) keeps
            if (rk == 2 && wd > 31 - q.d) wd = 31 - q.d;
            f->skip = off << 8 | wd << 16 | (ok == 1 ? 0 : 1) << 24;
            k = rk == 4 ? ((int32_t)1 << q.d) - 1 : rk ? 1 : 0;
        } else {
            f->skip = (rk << 8) | (ok << 16);   // (qg_fix.h, fx_finish_packed)
        }
        if (q.d < 0) { f->ls = -q.d; return 0; }
        f->d = q.d;
        f->t = (int32_t)round_addend(q.Q, q.d);
        const int32_t half = q.d ? (int32_t)1 << (q.d - 1) : 0;
        if (bf && (rk == 1 || rk == 3)) f->t = half - 1;
        if (bf && rk == 2) f->t = INT32_MIN + (half - 1);
        return k;
    }
};

// a sub-operation of the complex product: its slot, whether it multiplies, the formats of its first operand x and its second operand y
struct Slot { int idx; bool mul; qfmt x, y; };
bool fits24(qfmt f, int extra) { return sbits(f) + extra <= 24; }
int32_t pow2_factor(int sh) { return sh >= 0 && sh <= 22 ? (int32_t)1 << sh : 0; }   // (0: out of the compact form's range, see cplx_records)

// what a one-format tree asks of a level: the overflow mode and the bounds (which fix the sign); S >= 0: that isSigned code as well
struct LevelFormat { int O; int64_t lo, hi; int S; };
bool same_clamp(const QFix& f, const QFix& r) { return f.lo == r.lo && f.hi == r.hi; }

// The analysis of one descriptor, stage by stage (qg_analyze below calls them in order; each reads what the earlier ones left in *out)
struct Analyzer {
    Ctx c;
    const qgemul_desc* d;                 // (validate may point it at with_artefacts)
    QAnalysis* const out;
    QTreeTable& T;                        // out->tree
    qgemul_desc with_artefacts;
    // what validate derives from the descriptor
    int cx = 0, parts = 1, bitsA = 0, bitsB = 0;   // complex; 1 or 2 parts; storage bits of a[0], b[0]
    bool mixed = false, real_a = false;   // one real and one complex operand (QG_CMUL_REAL_A / QG_CMUL_REAL_B, QuBLAS.h:3600-3644): two part-wise products on a shared real value
    bool copy0 = false;                   // QG_DESC_LEFTOVER0_COPY with an odd K (leftover0_copy)
    // what a stage leaves for a later one
    Val prod[2];                          // product -> tree: the parts' products
    bool recs = false, rec_clamps = false;   // tree_records -> gemv_forms: the unbiased records are valid (every level clamps / overflow kinds)
    bool tf = false;                      // cplx_forms -> its parts: the multiplier, the slots of RE, IM and of the products
    int re = 0, im = 0;
    std::vector<int> prods;

    Analyzer(const qgemul_desc* d_, QAnalysis* out_) : d(d_), out(out_), T(out_->tree) { c.out = out_; }

    bool validate()
    {
        if (!d || d->abi != QGEMUL_ABI_VERSION) { c.fail(QG_EINVAL, "null descriptor or ABI mismatch"); return false; }
        // QG_DESC_REFERENCE_ARTEFACTS: C of an unsigned WRP::TCPL format with exactly 32 value bits is stored unwrapped by the reference
        // (include/qgemul.h) — which is what its WRP::TCPL_SAT stub does: analysed, and executed, as that
        if (d->flags & QG_DESC_REFERENCE_ARTEFACTS) {
            with_artefacts = *d;
            for (int p = 0; p < (d->is_complex ? 2 : 1); ++p) {
                qfmt& f = with_artefacts.c[p];
                if (f.O == QG_WRP_TCPL && !f.S && (int)f.I + (int)f.F == 32) f.O = QG_WRP_TCPL_SAT;
            }
            d = &with_artefacts;
        }
        if (d->M < 0 || d->N < 0 || d->K < 1) { c.fail(QG_EINVAL, "bad M/N/K"); return false; }
        if (d->M > (1ll << 31) || d->N > (1ll << 31) || d->K > (1ll << 31)) { c.fail(QG_EUNSUPPORTED, "dimension beyond 2^31"); return false; }
        uint32_t n = 0;
        for (int64_t len = d->K; len > 1; len = (len + 1) / 2) ++n;
        if (n != d->n_levels || n > QG_MAX_LEVELS) { c.fail(QG_EINVAL, "n_levels != ceil(log2 K)"); return false; }
        cx = d->is_complex ? 1 : 0;
        parts = cx ? 2 : 1;
        mixed = cx && (d->cmul == QG_CMUL_REAL_A || d->cmul == QG_CMUL_REAL_B);
        real_a = mixed && d->cmul == QG_CMUL_REAL_A;
        if (cx && !mixed && d->cmul != QG_CMUL_BASIC && d->cmul != QG_CMUL_TF) { c.fail(QG_EINVAL, "complex descriptor without cmul"); return false; }
        if (!cx && (d->cmul == QG_CMUL_REAL_A || d->cmul == QG_CMUL_REAL_B)) { c.fail(QG_EINVAL, "mixed real-complex: C is complex (is_complex = 1)"); return false; }
        if (mixed) {   // the real operand has ONE spelling: its format in [0], [1] all zero (the plan cache compares field by field)
            const qfmt z = real_a ? d->a[1] : d->b[1];
            // (pad is no part of a format's meaning: qg_run_key.h)
            if (z.I || z.F || z.S || z.Q || z.O) { c.fail(QG_EINVAL, "mixed real-complex: [1] of the real operand's format must be zero"); return false; }
        }
        if (!cx && d->cmul != QG_CMUL_NONE) { c.fail(QG_EINVAL, "real descriptor with cmul"); return false; }
        bitsA = sbits(d->a[0]);
        bitsB = sbits(d->b[0]);
        copy0 = (d->flags & QG_DESC_LEFTOVER0_COPY) && (d->K & 1) && d->K > 1;

        T.is_complex = cx;
        T.cmul = d->cmul;
        T.n_levels = (int)d->n_levels;
        T.n_levels_k = d->n_levels < 5 ? 5 : (int)d->n_levels;
        QNode idn;
        memset(&idn, 0, sizeof idn);
        idn.q.identity = 1;
        for (int p = 0; p < 2; ++p)
            for (int l = (int)d->n_levels; l < T.n_levels_k && l < QG_MAX_LEVELS; ++l) {   // identity levels behind a short tree
                T.level_add[p][l] = idn;
                T.level_cvt[p][l] = T.leftover[p][l] = idn.q;
            }
        T.parts = parts;

        for (int p = 0; p < parts; ++p) {
            const bool has_a = !(real_a && p), has_b = !(mixed && !real_a && p);   // (the real operand of a mixed descriptor has no [1])
            if ((has_a && !fmt_ok(c, d->a[p])) || (has_b && !fmt_ok(c, d->b[p])) || !fmt_ok(c, d->c[p])) return false;
            // operand ELEMENTS are one-word values (int32_t / int64_t host elements); products, sums, levels and C may be multi-word
            if ((has_a && sbits(d->a[p]) > 64) || (has_b && sbits(d->b[p]) > 64)) { c.fail(QG_EUNSUPPORTED, "operand element wider than 64 storage bits"); return false; }
        }
        const int nslots = !cx ? 1 : mixed ? 2 : (d->cmul == QG_CMUL_TF ? 8 : 6);
        for (int i = 0; i < nslots; ++i)
            if (!fmt_ok(c, d->mul[i])) return false;
        for (int p = 0; p < parts; ++p)
            for (uint32_t l = 0; l < d->n_levels; ++l)
                if (!fmt_ok(c, d->level_add[p][l]) || !fmt_ok(c, d->level[p][l])) return false;
        return true;
    }

    void product()
    {
        const qfmt* m = d->mul;
        if (!cx) {
            const Val a = whole(d->a[0]), b = whole(d->b[0]);
            prod[0] = do_mul(c, a, b, m[QG_MUL_REAL], &T.mul[0]);
            prod[1] = prod[0];
            // the exact dot product, for the linear class
            Rng pr = mul_rng(a.r, b.r);
            Rng dot = {pr.lo * d->K, pr.hi * d->K};
            out->dot_bits = rng_bits(dot);
        } else if (mixed) {
            // re = Qmul<realT...>(x, y.real), im = Qmul<imagT...>(x, y.imag) — or (x.real, y), (x.imag, y) — QuBLAS.h:3604-3644
            for (int p = 0; p < 2; ++p) {
                prod[p] = do_mul(c, whole(d->a[real_a ? 0 : p]), whole(d->b[real_a ? p : 0]), m[p], &T.mul[p]);
            }
        } else {
            do_cmul(c, d->cmul == QG_CMUL_TF, whole(d->a[0]), whole(d->a[1]), whole(d->b[0]), whole(d->b[1]), m, T.mul, prod);
        }
    }

    void tree()
    {
        for (int p = 0; p < parts; ++p) {
            Val cur = prod[p];
            int64_t len = d->K;
            for (uint32_t l = 0; l < d->n_levels; ++l) {
                Val s = do_addsub(c, cur, cur, d->level_add[p][l], false, &T.level_add[p][l]);
                Val st = do_cvt(c, s, d->level[p][l], &T.level_cvt[p][l]);
                // odd leftover: the converting copy is on the path only when this level has odd length
                bool was_exact = c.exact;
                Val lf = do_cvt(c, cur, d->level[p][l], &T.leftover[p][l]);
                if (l == 0 && (d->flags & QG_DESC_LEFTOVER0_COPY)) {
                    // the level-0 buffer has the leaf's own type in the reference: a same-type copy (QuBLAS.h:4977-4980, :2401-2404)
                    T.leftover[p][l].identity = 1;
                    lf.r = cur.r;
                    if (len & 1) c.exact = was_exact;
                }
                if (!(len & 1)) c.exact = was_exact;
                else {
                    if (lf.r.lo < st.r.lo) st.r.lo = lf.r.lo;
                    if (lf.r.hi > st.r.hi) st.r.hi = lf.r.hi;
                }
                cur = st;
                len = (len + 1) / 2;
            }
            bool tree_exact = c.exact;
            c.final_step = true;
            do_cvt(c, cur, d->c[p], &T.c_cvt[p]);
            c.final_step = false;
            c.exact = tree_exact; // the epilogue is allowed (and expected) to quantise
        }
    }

    // linear-class epilogue: D = sum a*b at frac Fa+Fb, one round+overflow into C.
    // Equal to cvt_C(root) because root = D << (F_root - Fa - Fb) exactly and the root
    // lies inside the root format's range.
    void linear_real()
    {
        int fp = (int)d->a[0].F + (int)d->b[0].F;
        out->lin.to_c[0] = c.make_step(fp, d->c[0], false);
        out->lin.to_c[0].refcmp = T.c_cvt[0].refcmp;   // (the root's type width decides how the reference compares with C's bounds)
        if (d->c[0].O == QG_WRP_TCPL_SAT && !T.c_cvt[0].identity) out->lin.to_c[0].O = T.c_cvt[0].O;   // (in range: a clamp that never fires)
        out->lin.to_c[1] = out->lin.to_c[0];
        if (out->lin.to_c[0].d > 100 || out->lin.to_c[0].d < -100) c.exact = false;
    }

    // Mixed linear class.  When both products and every node of both trees are exact, the parts are the plain dot products
    //   re = sum_k x y.real,  im = sum_k x y.imag   (or x.real y, x.imag y)
    // at frac Fa + Fb of their own operands: ONE real GEMM on the stacked operand gives both, each then rounded / overflowed ONCE
    // into C's part by to_c[part] (sh[] stays 0: the parts are never combined).  The limits are those of the complex linear class.
    void linear_mixed()
    {
        I128 mx = 0;
        for (int p = 0; p < 2; ++p) {
            const qfmt fa = d->a[real_a ? 0 : p], fb = d->b[real_a ? p : 0];
            out->lin.to_c[p] = c.make_step((int)fa.F + (int)fb.F, d->c[p], false);
            if (out->lin.to_c[p].d > 61 || out->lin.to_c[p].d < -61) c.exact = false;
            const I128 t = mag(fmt_range(fa)) * mag(fmt_range(fb)) * d->K;
            if (t > mx) mx = t;
        }
        out->dot_bits = bits_of(mx);
        if (out->dot_bits > 62) c.exact = false;
    }

    // Complex linear class.  When every sub-operation and tree node is exact, both multipliers reduce to
    //   re = sum_k (a c - b d),  im = sum_k (a d + b c)
    // (TF: A - B = (a+b)c - (c+d)b, B - C = (c+d)b - (b-a)d), each term carrying the power of two of its
    // operands' fracBits.  Evaluate the two parts at frac Fx = max(Fa+Fc, Fb+Fd) and Fy = max(Fa+Fd, Fb+Fc).
    void linear_cplx()
    {
        const int Fa = d->a[0].F, Fb = d->a[1].F, Fc = d->b[0].F, Fd = d->b[1].F;
        const int Fx = (Fa + Fc > Fb + Fd) ? Fa + Fc : Fb + Fd;
        const int Fy = (Fa + Fd > Fb + Fc) ? Fa + Fd : Fb + Fc;
        int32_t* sh = out->lin.sh;
        sh[0] = Fx - (Fa + Fc);
        sh[1] = Fx - (Fb + Fd);
        sh[2] = Fy - (Fa + Fd);
        sh[3] = Fy - (Fb + Fc);
        out->lin.to_c[0] = c.make_step(Fx, d->c[0], false);
        out->lin.to_c[1] = c.make_step(Fy, d->c[1], false);
        for (int p = 0; p < 2; ++p)
            if (out->lin.to_c[p].d > 61 || out->lin.to_c[p].d < -61) c.exact = false;
        // width of the combined value: K terms of |a c| 2^sh + |b d| 2^sh
        const I128 ma = mag(fmt_range(d->a[0])), mb = mag(fmt_range(d->a[1])), mc = mag(fmt_range(d->b[0])), md = mag(fmt_range(d->b[1]));
        const I128 t1 = ma * mc * ((I128)1 << sh[0]) + mb * md * ((I128)1 << sh[1]);
        const I128 t2 = ma * md * ((I128)1 << sh[2]) + mb * mc * ((I128)1 << sh[3]);
        out->dot_bits = bits_of((t1 > t2 ? t1 : t2) * d->K);
        if (out->dot_bits > 62 || sh[0] > 40 || sh[1] > 40 || sh[2] > 40 || sh[3] > 40) c.exact = false;
    }

    // 64-bit kernels: every value within 62 bits, so that sums, alignment shifts and rounding addends stay inside int64 — except
    // the unrounded product of two operands, which is formed exactly by one 64-bit multiply and goes straight into its rounding
    // shift: it may use all of int64 (two signed 32-bit words: |a * b| <= 2^62).  32-bit fixed-point words therefore run.
    // Beyond that ("wide" plans): 128-bit values — the reference's multi-word ArbiInt<N > 64> (QuBLAS.h:566-912) — on the
    // general tree kernel's 128-bit instantiation, or, for the linear class, the composite MFMA plan with a 128-bit combine pass.
    bool widths_and_class()
    {
        out->max_bits = c.max_bits;
        out->max_bits_np = c.max_bits_np;
        if (c.max_bits_np > 120 || c.max_bits > 127) { c.fail(QG_EUNSUPPORTED, "an intermediate needs more than 120 bits"); return false; }
        out->wide = (c.max_bits_np > 62 || c.max_bits > 64 || c.max_fmt_bits > 62) ? 1 : 0;
        out->band = (c.band || c.raw_c) ? 1 : 0;
        out->generic_only = c.raw_c ? 1 : 0;
        if ((out->wide || out->generic_only) && cx) c.exact = false;   // (complex linear class: its own 62-bit combine only)
        if (!out->wide && (out->lin.to_c[0].d > 61 || out->lin.to_c[0].d < -61)) c.exact = false;
        out->linear_ok = c.exact ? 1 : 0;
        out->cls = out->linear_ok ? QG_CLASS_LINEAR : QG_CLASS_TREE;
        return true;
    }

    // the 32-bit kernels keep every value and every format's bounds in 32-bit registers
    bool fits32(bool with_products) const { return !out->wide && !out->generic_only && (with_products ? c.max_bits : c.max_bits_np) <= 31 && c.max_fmt_bits <= 31; }

    // which real tree kernels may run the descriptor (the forms below refine them; leftover0_copy may take them away again)
    void admissions()
    {
        const bool col = !cx && d->N == 1 && d->n_levels <= 30;
        // one-column kernel (qg_gemv.hip): products are formed in 64 bits, everything else in 32
        out->gemv_ok = (col && fits32(false)) ? 1 : 0;
        // ... with 64-bit tree values when only the ELEMENTS fit 32 storage bits (sums of 32-bit words, wide level types)
        out->gemv_wide_ok = (col && !out->wide && !out->generic_only && !out->gemv_ok && bitsA <= 32 && bitsB <= 32) ? 1 : 0;
        out->tree64_ok = (!cx && !out->wide && !out->generic_only && d->n_levels <= 16) ? 1 : 0;   // (64-bit values: not a wide plan)
        // 32-bit tree kernel (qg_tree_fast.hip): real, K a power of two >= 32, every value except the
        // unrounded product fits 31 bits, and the product is either directly 32-bit or splittable at
        // its rounding shift
        // (any K with 5..16 levels: the packed operands are zero-padded to 2^n_levels leaves — a node whose right child is a
        // zero is the reference's converting copy of an odd leftover, QuBLAS.h:4977-4980)
        out->tree_fast_ok = 0;
        if (cx || !fits32(false) || d->n_levels > 16) return;
        const int sh = T.mul[0].q.d, bh = bitsB - sh < 1 ? 1 : bitsB - sh;
        const bool direct = bitsA + bitsB <= 31;
        if (!direct && !(sh >= 1 && sh <= 23 && bitsA + bh <= 31 && bitsA + sh <= 31)) return;
        out->tree_fast_ok = 1;
        out->split_s = direct ? 0 : sh;
        out->mul24_ok = bitsA <= 24 && (direct ? bitsB : bh) <= 24;
    }

    // fixed-mode variants of the 32-bit tree kernel: product and all levels in one format, truncating
    // product, SAT::ZERO or SAT::TCPL overflow (the shapes default tags produce)
    void tree_one_format()
    {
        out->tree_form = QTF_RUNTIME;
        if (!out->tree_fast_ok || !out->mul24_ok) return;
        const qfmt pf = d->mul[0];
        bool one = (pf.Q == QG_TRN_TCPL || T.mul[0].q.d <= 0) && T.mul[0].q.d >= 0 && (pf.O == QG_SAT_ZERO || pf.O == QG_SAT_TCPL);
        for (uint32_t l = 0; l < d->n_levels && one; ++l) one = same(d->level[0][l], pf) && same(d->level_add[0][l], pf);
        const int W = (int)pf.I + (int)pf.F;
        if (one && W + 1 + T.mul[0].q.d <= 30) out->tree_form = pf.O == QG_SAT_ZERO ? QTF_ONE_ZERO : QTF_ONE_TCPL;
    }

    // every level neither converts nor aligns, and is either padding behind a short tree (x + 0) or a plain node — no shift — of the format F
    bool plain_levels(const LevelFormat& F) const
    {
        for (int l = 0; l < T.n_levels_k; ++l) {
            const QNode& n = T.level_add[0][l];
            const bool pad = l >= T.n_levels && n.q.identity;
            const bool node = !n.q.identity && n.q.O == F.O && (F.S < 0 || n.q.S == F.S) && n.q.d == 0 && n.q.lo == F.lo && n.q.hi == F.hi;
            if (!T.level_cvt[0][l].identity || n.sa != 0 || n.sb != 0 || !(pad || node)) return false;
        }
        return true;
    }

    // QTF_REC_CLAMP: per-level formats, but every step "add a constant, shift right, clamp" (QFix, qg_plan.h): TRN::TCPL /
    // RND::POS_INF / RND::NEG_INF rounding; SAT::TCPL / SAT::SMGN (one clamp), SAT::ZERO (range test + select) or WRP::TCPL
    // (sign extension / mask) overflow — e.g. default modes with a wider level type in QgemulAddArgs, which used to take the
    // run-time-mode form (4.3x slower at 2048^3)
    void tree_records()
    {
        const bool tree_rt = out->tree_fast_ok && out->mul24_ok && out->tree_form == QTF_RUNTIME;
        if (!tree_rt && !out->gemv_ok) return;
        const bool for_tree = tree_rt && !out->gemv_ok;
        const QStep& pq = T.mul[0].q;
        // (the split product is rounded inside its low half: its shift is the split, never a left shift)
        // (the one-column kernel forms its products itself: only the levels' records matter there)
        bool ok3 = out->gemv_ok || (compact_step_ok(pq) && (out->split_s == 0 || (!pq.identity && pq.d == out->split_s)));
        for (int l = 0; l < T.n_levels_k && ok3; ++l)
            ok3 = compact_step_ok(T.level_add[0][l].q) && T.level_cvt[0][l].identity && T.level_add[0][l].sa == 0 && T.level_add[0][l].sb == 0;
        if (!ok3) return;
        if (compact_step_ok(pq)) real_record(pq, &T.fmul[0]);
        bool clamps = out->gemv_ok || (T.fmul[0].kb == 0 && rounding_kind(pq) == 0);
        bool plain_rounding = out->gemv_ok || rounding_kind(pq) == 0;   // no value-dependent rounding anywhere: the biased form applies
        for (int l = 0; l < T.n_levels_k; ++l) {
            real_record(T.level_add[0][l].q, &T.fadd[0][l]);
            clamps = clamps && T.fadd[0][l].kb == 0 && rounding_kind(T.level_add[0][l].q) == 0;
            plain_rounding = plain_rounding && rounding_kind(T.level_add[0][l].q) == 0;
        }
        recs = true;
        rec_clamps = clamps;
        // every step clamps (one v_med3 per value, no branch on the overflow kind), or the records' overflow kinds on unbiased values
        if (for_tree) out->tree_form = clamps ? QTF_REC_CLAMP : QTF_REC_KINDS;
        if (!clamps && for_tree && plain_rounding && biased_records()) out->tree_form = QTF_REC_BIASED;
    }

    // QTF_REC_BIASED: some step tests the range (SAT::ZERO) or wraps.  The running value is then kept BIASED by -lo of its own
    // format, u = v - lo >= 0 (as the one-format SAT::ZERO form does): the range test is ONE unsigned compare
    // against span = hi - lo with the biased zero as the select's other operand, a clamp is med3(u, 0, span) with
    // no register for a bound, a wrap is u & span; the change of bias from level to level, the rounding addend and
    // the new bias (scaled by 2^d: subtracting a multiple of 2^d before a right shift by d is exact) are ONE
    // constant of the node's v_add3.  Record fields (QFix): t = that constant, d, ls, kb = overflow kind
    // (0 clamp, 1 zero, 2 wrap, 4 none), hi = span, lo = the bias B = -lo (also the biased zero).
    bool biased_records()
    {
        const QFix keep_mul = T.fmul[0];
        const std::vector<QFix> keep_add(T.fadd[0], T.fadd[0] + T.n_levels_k);
        bool fits = c.max_bits_np <= 30;   // (the raw product is never formed: split, or bitsA + bitsB <= 31)
        Biased cur = biased_of(T.mul[0].q);
        fits &= biased_record(cur, 0, &T.fmul[0]);
        for (int l = 0; l < T.n_levels_k; ++l) {
            const Biased me = biased_of(T.level_add[0][l].q);
            fits &= biased_record(me, 2 * cur.B, &T.fadd[0][l]);
            cur = me;
        }
        T.fmul[0].ka = (int32_t)cur.B;   // the root's bias, removed once per output
        if (!fits) {   // too wide for the bias arithmetic: the unbiased records stand
            T.fmul[0] = keep_mul;
            for (int l = 0; l < T.n_levels_k; ++l) T.fadd[0][l] = keep_add[l];
        }
        return fits;
    }

    // the left shift e of a justified product, shared between the staged operands: A takes what a factor of `opbits` bits has room for
    bool split_shift(int e, int opbits, int* ea, int* eb) const
    {
        *ea = e > opbits - bitsA ? opbits - bitsA : e;
        if (*ea < 0) *ea = 0;
        *eb = e - *ea;
        return bitsA + *ea <= opbits && bitsB + *eb <= opbits && *eb >= 0;
    }

    // QTF_LJ, left-justified values (qg_fix.h): the product and every level clamp into ONE signed SAT::TCPL format of
    // Wt = W + 1 bits, the product rounds by "add a constant, shift right by d" (TRN::TCPL, RND::POS_INF, RND::NEG_INF) and the
    // nodes do not shift.  Values are held as x * 2^s, s = 32 - Wt: the operands are staged with factors 2^ea, 2^eb,
    // ea + eb = s - d, so that a * b * 2^(s-d) + t * 2^(s-d), saturated by the multiply-add itself and its low s bits cleared,
    // is the quantised product; a node is one saturating add.  tree_form_base keeps the form such a descriptor had before.
    void tree_justified()
    {
        out->tree_form_base = out->tree_form;
        if (!out->tree_fast_ok || (out->tree_form != QTF_ONE_TCPL && out->tree_form != QTF_REC_CLAMP)) return;
        const QStep& pq = T.mul[0].q;
        // (unsigned: every operand, the product and the levels unsigned — nothing ever goes below 0 — and [0, 2^W - 1] is the uint32
        //  range of x * 2^(32 - W): the unsigned multiply-add / add with the clamp bit, QTF_LJ_U)
        const bool uns = !pq.S && !d->a[0].S && !d->b[0].S && pq.lo == 0;
        const int Wt = width_of_hi(pq.hi) + (uns ? 0 : 1);   // hi = 2^(Wt-1) - 1 (signed), 2^Wt - 1 (unsigned)
        const int sj = 32 - Wt;
        int ea = 0, eb = 0;
        const bool lj = !pq.identity && pq.O == QG_SAT_TCPL && (uns || (pq.S && pq.lo == -pq.hi - 1)) && pq.d >= 0 && ((pq.hi + 1) & pq.hi) == 0 && pq.hi > 0 &&
                        (pq.d == 0 || adds_constant(pq)) && sj >= 1 && sj - pq.d >= 0 && plain_levels({QG_SAT_TCPL, pq.lo, pq.hi, pq.S}) &&
                        split_shift(sj - pq.d, 24, &ea, &eb);
        if (!lj) return;
        memset(&T.lj, 0, sizeof T.lj);
        const int64_t t = round_addend(pq.Q, pq.d);
        T.lj.t[0] = (int32_t)(t << (sj - pq.d));   // (< 2^(s-1))
        T.lj.s = sj;
        T.lj.e[0] = ea;
        T.lj.e[1] = eb;
        out->tree_form = uns ? QTF_LJ_U : QTF_LJ;
        // QTF_PK16: ... in 16-bit halves, two outputs per register (k_tree_pk16): the format has at most 16 bits and the justified
        // operands fit int16 (QTreeTable::lj16).
        const int s16 = 16 - Wt;
        if (s16 >= 1 && s16 - pq.d >= 0 && split_shift(s16 - pq.d, 16, &ea, &eb)) {
            memset(&T.lj16, 0, sizeof T.lj16);
            T.lj16.s = s16;
            T.lj16.e[0] = ea;
            T.lj16.e[1] = eb;
            T.lj16.t[0] = (int32_t)(t << (s16 - pq.d));
            out->tree_form = uns ? QTF_PK16_U : QTF_PK16;
        }
        // QTF_PK16_HYB: the format has at most 16 bits but its product does not fit the halves (bits + shift > 16): QTF_LJ's 32-bit
        // justified product, whose high half is the value justified in 16 bits, and the tree on packed halves
        if ((out->tree_form == QTF_LJ || out->tree_form == QTF_LJ_U) && Wt >= 2 && Wt <= 16)   // (HYB16: no bits below the unit in a half)
            out->tree_form = Wt == 16 ? (uns ? QTF_PK16_HYB16_U : QTF_PK16_HYB16) : (uns ? QTF_PK16_HYB_U : QTF_PK16_HYB);
    }

    // QTF_WORD, 32-BIT WORDS (Q15.16 with default tags, the 32-bit fixed-point format of most code): the product and every level
    // clamp into ONE signed SAT::TCPL format of exactly 32 bits — whose range is the int32 range as it stands, no justification and
    // no bits below the unit — the nodes do not shift, and the product rounds by "add a constant, shift right by d" out of the
    // exact 64-bit product of two elements of at most 32 bits.  Then a node is ONE v_add_i32 ... clamp, where the 64-bit tree
    // kernel spends a 64-bit add and a 64-bit clamp; the product is v_mul_hi / v_mul_lo, the shift and a saturation to the word.
    // Runs on the 32-bit tree kernel's frame, which has no run-time-mode form for such a format: the plan
    // flag QG_OPT_RUNTIME_MODES sends the descriptor to the 64-bit kernel (qg_geom.cpp).
    void tree_words()
    {
        if (out->tree_fast_ok || cx || out->wide || out->generic_only || d->n_levels > 16 || T.n_levels_k > 16) return;
        const QStep& pq = T.mul[0].q;
        // ... and JUSTIFIED WORDS: a signed SAT::TCPL format of Wt < 32 bits (Q11.12: 24-bit words) held as x * 2^sj, sj = 32 - Wt, as
        // QTF_LJ holds it, when the product needs a net RIGHT shift dn = d - sj >= 1 (QTF_LJ needs a left one, and 24-bit
        // factors): the word is floor((a b + t) / 2^dn) of the same exact 64-bit product with its low sj bits cleared, the nodes
        // are QTF_LJ's (T.lj.e[0] = sj; QTF_JWORD / QTF_JWORD_MAD).  Such descriptors ran on the 64-bit tree kernel.
        const int Wt = 1 + width_of_hi(pq.hi);      // hi = 2^(Wt-1) - 1
        const int sj = 32 - Wt, dn = pq.d - sj;
        const bool elems = bitsA <= 32 && bitsB <= 32 && (d->a[0].S || bitsA <= 31) && (d->b[0].S || bitsB <= 31);   // (elements are int32 words in the packed operands)
        // the root is converted into C by the kernel's 32-bit step: C's bounds must be words too, and no left shift
        const QStep& cq = T.c_cvt[0];
        const bool c_word = cq.identity || (cq.d >= 0 && sbits(d->c[0]) <= 32);
        const bool w32 = !pq.identity && pq.O == QG_SAT_TCPL && pq.S && Wt >= 2 && Wt <= 32 && pq.hi == ((int64_t)1 << (Wt - 1)) - 1 && pq.lo == -pq.hi - 1 &&
                         dn >= 1 && dn <= 31 && pq.d <= 31 &&   // (dn = 0: the kernel's range test of the high half has no form; d <= 31: the rounding addend is an int32)
                         adds_constant(pq) && elems && plain_levels({QG_SAT_TCPL, pq.lo, pq.hi, -1}) && c_word;
        // ... and WRAPPING words: the same frame for a signed WRP::TCPL format of exactly 32 bits (T.lj.e[1] = 1; QTF_WORD_WRAP) — the
        // product's word is the low 32 bits of floor((a b + t) / 2^d), 0 <= d <= 31, a node a plain 32-bit add
        const bool wrap32 = !w32 && !pq.identity && pq.O == QG_WRP_TCPL && pq.S && pq.W == 31 && pq.d >= 0 && pq.d <= 31 && (pq.d == 0 || adds_constant(pq)) && elems &&
                            plain_levels({QG_WRP_TCPL, -((int64_t)1 << 31), ((int64_t)1 << 31) - 1, -1}) && c_word;
        if (!w32 && !wrap32) return;
        memset(&T.lj, 0, sizeof T.lj);
        T.lj.t[0] = (int32_t)round_addend(pq.Q, pq.d);
        out->tree_fast_ok = 1;
        out->split_s = 0;
        out->mul24_ok = 0;
        if (wrap32) {
            T.lj.s = pq.d;
            T.lj.e[1] = 1;
            out->tree_form = out->tree_form_base = QTF_WORD_WRAP;
        } else {
            T.lj.s = dn;      // the product's shift (to the justified word)
            T.lj.e[0] = sj;   // bits below the unit in a word (0: 32-bit formats)
            const bool mad = dn >= 10 && dn <= 23;   // a product shift of 10 ... 23: the multiply-add form
            out->tree_form = out->tree_form_base = sj > 0 ? (mad ? QTF_JWORD_MAD : QTF_JWORD) : (mad ? QTF_WORD_MAD : QTF_WORD);
        }
    }

    // QG_DESC_LEFTOVER0_COPY with an odd K: the zero-padded kernels would form the leftover as x + 0 in level 0's type — a
    // conversion, where the reference copies — so only the general kernel, which has the leftover step itself, may run it
    void leftover0_copy()
    {
        if (!copy0) return;
        out->tree_fast_ok = out->tree64_ok = out->gemv_ok = out->gemv_wide_ok = 0;
        out->tree_form = QTF_RUNTIME;
    }

    void gemv_forms()
    {
        const int64_t lo32 = -((int64_t)1 << 31), hi32 = ((int64_t)1 << 31) - 1;
        // (the Qreduce lowering: a * 1 into a's own format.  That is the identity for every raw value EXCEPT -2^W of a signed
        // SAT::SMGN format, which the conversion clamps to -(2^W - 1); the lowerings therefore name a's format with SAT::TCPL
        // as the leaf format of such element types, and only that form takes the shortcut)
        qfmt leaf = d->a[0];
        if (leaf.S && leaf.O == QG_SAT_SMGN) leaf.O = QG_SAT_TCPL;
        out->gemv_b_bit = ((out->gemv_ok || out->gemv_wide_ok) && d->b[0].I == 1 && d->b[0].F == 0 && !d->b[0].S && same(d->mul[0], leaf)) ? 1 : 0;
        // 32-bit words in the one-column kernel (a Qreduce / GEMV of Q15.16 with default levels): the values fit the element
        // registers and a node is one v_add_i32 ... clamp; the 64-bit-value form of the same kernel spends a 64-bit add and a
        // run-time step per node (65 536 x 4096: 7.6 ms where the bytes take 0.2).  The product is formed in 64 bits by the
        // general step (or not at all: gemv_b_bit), so any rounding / overflow pair into a format of at most 32 bits will do.
        out->gemv_w32 = 0;
        if (out->gemv_wide_ok && d->n_levels >= 1) {
            const int bitsM = (d->mul[0].S ? 1 : 0) + (int)d->mul[0].I + (int)d->mul[0].F;
            out->gemv_w32 = (bitsM <= (d->mul[0].S ? 32 : 31) && (int)d->mul[0].I + (int)d->mul[0].F >= 0 && plain_levels({QG_SAT_TCPL, lo32, hi32, -1})) ? 1 : 0;
        }
        out->gemv_form = out->gemv_w32 ? QGF_WORD : QGF_RUNTIME;   // (only with gemv_wide_ok, i.e. never together with the forms below)
        if (out->gemv_w32 && !out->gemv_b_bit) {    // ... and the product itself is QTF_WORD's "add a constant, shift right, saturate to the word"
            const QStep& pq = T.mul[0].q;
            if (!pq.identity && pq.O == QG_SAT_TCPL && pq.S && pq.lo == lo32 && pq.hi == hi32 && pq.d >= 1 && pq.d <= 31 && adds_constant(pq)) out->gemv_form = QGF_WORD_RND;
        }
        if (out->gemv_ok) {
            // all levels one format (the product's), exact alignment (d == 0), SAT::ZERO or SAT::TCPL
            const qfmt lf = d->level_add[0][0];
            bool one = (lf.O == QG_SAT_ZERO || lf.O == QG_SAT_TCPL) && same(lf, d->mul[0]) && (int)lf.I + (int)lf.F <= 29;
            for (uint32_t l = 0; l < d->n_levels && one; ++l)
                one = same(d->level_add[0][l], lf) && same(d->level[0][l], lf) && T.level_add[0][l].q.d == 0;
            if (one) out->gemv_form = lf.O == QG_SAT_ZERO ? QGF_ONE_ZERO : QGF_ONE_TCPL;
            else if (recs) out->gemv_form = rec_clamps ? QGF_REC_CLAMP : QGF_REC_KINDS;   // per-level formats in compact records
        }
    }

    // every product slot and every tree step of both parts satisfies `ok`
    template <class Pred> bool every_cplx_step(Pred ok) const
    {
        bool all = true;
        const int ns = mixed ? 2 : d->cmul == QG_CMUL_TF ? 8 : 6;
        for (int i = 0; i < ns; ++i) all = all && ok(T.mul[i].q);
        for (int p = 0; p < 2; ++p)
            for (uint32_t l = 0; l < d->n_levels; ++l) all = all && ok(T.level_add[p][l].q) && ok(T.level_cvt[p][l]);
        return all;
    }

    void cplx_forms()
    {
        // (mixed real-complex descriptors: the same conditions admit them to their own 32-bit kernel, qg_tree_rc.hip)
        out->cplx_fast_ok = (cx && fits32(true) && !copy0 && d->n_levels <= 16) ? 1 : 0;
        out->cplx_form = QCF_RUNTIME;
        if (!out->cplx_fast_ok) return;
        // fixed-mode variant of the complex kernel (BASELINE configuration 5's "RND + SAT"): every sub-operation and every tree
        // step either the identity, or an exact left shift / a rounding shift with RND::POS_INF, followed by SAT::TCPL, so a
        // step is (v + 2^(d-1)) >> d (or v << -d) and one clamp
        const bool all = every_cplx_step([](const QStep& q) { return q.identity || (q.d >= -29 && q.d <= 29 && q.O == QG_SAT_TCPL && (q.d <= 0 || q.Q == QG_RND_POS_INF)); });
        out->cplx_form = all && !mixed ? QCF_TABLE : QCF_RUNTIME;   // (the mixed kernel has the forms QCF_RUNTIME and QCF_COMPACT)
        // ... and QCF_COMPACT when every step fits the branch-free forms of QFix (qg_plan.h): a rounding that is "add a constant, shift
        // right" — TRN::TCPL (+0; the reference's default QuMode), RND::POS_INF (+2^(d-1)), RND::NEG_INF (+2^(d-1) - 1) — and an
        // overflow that is one clamp — SAT::TCPL (the reference's default OfMode) or SAT::SMGN ([-hi, hi]); the values that
        // enter a multiplication or an alignment fit 24 bits (v_mad_i32_i24), alignment and exact left shifts are folded
        // into power-of-two factors of at most 2^22
        // (the other modes as rounding / overflow kinds: QCF_KINDS, QCF_KINDS_*)
        if (!every_cplx_step(compact_step_ok)) return;
        tf = d->cmul == QG_CMUL_TF;
        re = tf ? QG_T_RE : QG_B_RE;
        im = tf ? QG_T_IM : QG_B_IM;
        prods = tf ? std::vector<int>{QG_T_A, QG_T_B, QG_T_C} : std::vector<int>{QG_B_AC, QG_B_BD, QG_B_AD, QG_B_BC};
        KindPacker P;
        if (!cplx_records(P)) return;
        out->cplx_form = !P.kinds ? QCF_COMPACT : mixed ? QCF_RUNTIME : P.feat > 0 ? qcf_kinds(P.feat) : QCF_KINDS;
        if (out->cplx_form != QCF_COMPACT || mixed) return;
        const bool uni = cplx_uniform();
        cplx_justified(uni);
    }

    std::vector<Slot> cplx_slots() const
    {
        const qfmt a = d->a[0], b = d->a[1], cc = d->b[0], dd = d->b[1], *m = d->mul;
        if (mixed)   // the two part-wise products on the shared real value
            return {{QG_M_RE, true, a, cc}, {QG_M_IM, true, real_a ? a : b, real_a ? dd : cc}};
        if (tf)
            return {{QG_T_AB, false, a, b}, {QG_T_CD, false, cc, dd}, {QG_T_BA, false, b, a}, {QG_T_A, true, m[QG_T_AB], cc}, {QG_T_B, true, m[QG_T_CD], b},
                    {QG_T_C, true, m[QG_T_BA], dd}, {QG_T_RE, false, m[QG_T_A], m[QG_T_B]}, {QG_T_IM, false, m[QG_T_B], m[QG_T_C]}};
        return {{QG_B_AC, true, a, cc}, {QG_B_BD, true, b, dd}, {QG_B_AD, true, a, dd}, {QG_B_BC, true, b, cc},
                {QG_B_RE, false, m[QG_B_AC], m[QG_B_BD]}, {QG_B_IM, false, m[QG_B_AD], m[QG_B_BC]}};
    }

    // the compact records of every slot and tree step, packed once — and, where kinds were met that the branch-free form covers, a
    // second time for that form.  False: a value or a factor leaves the form's range (24-bit operands, factors of at most 2^22)
    bool cplx_records(KindPacker& P)
    {
        const std::vector<Slot> slots = cplx_slots();
        bool reg = true;
        for (int pass = 0; pass < 2 && reg; ++pass) {
            P.bf = pass == 1;
            memset(T.fmul, 0, sizeof T.fmul);
            for (const Slot& sl : slots) {
                const QNode& n = T.mul[sl.idx];
                QFix& f = T.fmul[sl.idx];
                const int32_t k = P.pack(n.q, &f);
                const int ls = (!n.q.identity && n.q.d < 0) ? -n.q.d : 0;   // exact left shift after the operation: folded into the factors
                if (n.q.identity) f.skip &= ~1;   // (the operation itself still runs; only its rounding / overflow is the identity)
                f.ls = k;                         // (slots fold their shift into the factors: ls carries the rounding factor)
                if (sl.mul) {
                    f.ka = pow2_factor(ls);
                    reg = reg && ls <= 22 && fits24(sl.x, ls) && fits24(sl.y, 0);
                } else {
                    f.ka = pow2_factor(n.sa + ls);
                    f.kb = pow2_factor(n.sb + ls);
                    reg = reg && n.sa >= 0 && n.sb >= 0 && n.sa + ls <= 22 && n.sb + ls <= 22 && fits24(sl.x, 0) && fits24(sl.y, 0);
                }
            }
            for (int p = 0; p < 2 && reg; ++p)
                for (int l = 0; l < T.n_levels_k && reg; ++l) {
                    reg = reg && T.level_add[p][l].sa == 0 && T.level_add[p][l].sb == 0;
                    T.fadd[p][l].ka = P.pack(T.level_add[p][l].q, &T.fadd[p][l]);   // (a left shift at a node is QFix::ls; ka: the rounding factor)
                    T.fcvt[p][l].ka = P.pack(T.level_cvt[p][l], &T.fcvt[p][l]);
                    if (T.level_add[p][l].q.identity) T.fadd[p][l].skip &= ~1;
                }
            if (!P.kinds || P.feat <= 0) break;   // plain compact records, or the branching form: the first packing stands
        }
        return reg;
    }

    // every level of both parts stores without converting and clamps into the range of r0 without shifting or rounding
    // (levels that continue a short tree add 0 to a value of the common range: clamping it again changes nothing; an
    //  identity node of the tree proper is a WIDER format the sum always fits — not this form)
    bool cplx_levels_one_clamp(const QFix& r0) const
    {
        for (int p = 0; p < 2; ++p)
            for (int l = 0; l < T.n_levels_k; ++l) {
                const QFix &fa = T.fadd[p][l], &fc = T.fcvt[p][l];
                const bool pad = l >= T.n_levels && T.level_add[p][l].q.identity != 0;
                if (!(fc.skip & 1) || !(pad || (same_clamp(fa, r0) && fa.t == 0 && fa.d == 0 && fa.ls == 0))) return false;
            }
        return true;
    }

    // QCF_UNIFORM ("one clamp for the whole loop"): the plain compact form where, in addition, every value made in the k loop — the
    // products, their sum / differences and every tree node of both parts — is clamped into ONE range, the sums and the
    // nodes neither shift nor round (equal fraction bits throughout), and the level buffers do not convert.  That is what
    // default tags give on operands whose parts merge into one format (BASELINE configuration 5: everything is int<6,3>
    // RND::POS_INF / SAT::TCPL inside the loop).  The kernel then keeps (lo, hi) and the products' (t, d) in registers for
    // the whole launch — no record loads, no moves of bounds — and the products' exact left shifts are folded into the
    // staged operand planes: 18 vector instructions per complex MAC instead of 24.8 (TF), 21 instead of 27.4 (Basic).
    bool cplx_uniform()
    {
        const QFix &r0 = T.fmul[re], &fi = T.fmul[im];
        bool uni = r0.lo > INT32_MIN && r0.hi < INT32_MAX;
        for (int sl : prods) uni = uni && same_clamp(T.fmul[sl], r0) && T.fmul[sl].d >= 0 && T.fmul[sl].ka >= 1;
        for (const QFix* f : {&r0, &fi}) uni = uni && same_clamp(*f, r0) && f->ka == 1 && f->kb == 1 && f->t == 0 && f->d == 0;
        if (!uni || !cplx_levels_one_clamp(r0)) return false;
        memset(&T.uni, 0, sizeof T.uni);
        T.uni.lo = r0.lo;
        T.uni.hi = r0.hi;
        if (tf) {   // every product owns one plane: the plane takes the product's left shift (checked against 24 bits above: fits24(x, ls))
            for (int i = 0; i < 3; ++i) { const QFix& f = T.fmul[prods[i]]; T.uni.t[i] = f.t; T.uni.d[i] = f.d; T.uni.k[i] = f.ka; }
            T.uni.k[3] = 1;
        } else if (!basic_plane_shifts()) {
            return false;
        }
        out->cplx_form = QCF_UNIFORM;
        return true;
    }

    // Basic: a plane serves two products (a: ac, ad; b: bd, bc; c: ac, bc; d: bd, ad).  Plane shifts la, lb, lc, ld with
    // lx + ly >= the product's left shift; what they exceed it by is shifted out again after the rounding addend (scaled
    // alike): (x y 2^(lx+ly) + t 2^e) >> (d + e) = (x y 2^ls + t) >> d.  The smallest total that keeps planes within
    // 24 bits and products within 31.
    bool basic_plane_shifts()
    {
        const int px[4] = {0, 1, 0, 1}, py[4] = {2, 3, 3, 2};   // ac, bd, ad, bc over planes a b c d
        const qfmt pf[4] = {d->a[0], d->a[1], d->b[0], d->b[1]};
        int w[4], ls[4], best[4] = {0, 0, 0, 0}, best_sum = -1;
        for (int i = 0; i < 4; ++i) { w[i] = sbits(pf[i]); ls[i] = ilog2(T.fmul[prods[i]].ka); }
        for (int la = 0; la <= 12; ++la)
            for (int lb = 0; lb <= 12; ++lb)
                for (int lc = 0; lc <= 12; ++lc)
                    for (int ld = 0; ld <= 12; ++ld) {
                        const int l[4] = {la, lb, lc, ld};
                        bool ok = true;
                        for (int i = 0; i < 4 && ok; ++i) ok = w[i] + l[i] <= 24;
                        for (int i = 0; i < 4 && ok; ++i) {
                            const int e = l[px[i]] + l[py[i]] - ls[i];
                            ok = e >= 0 && w[px[i]] + w[py[i]] + l[px[i]] + l[py[i]] <= 30 && T.fmul[prods[i]].d + e <= 30;
                        }
                        const int sum = la + lb + lc + ld;
                        if (ok && (best_sum < 0 || sum < best_sum)) { best_sum = sum; memcpy(best, l, sizeof best); }
                    }
        for (int i = 0; i < 4 && best_sum >= 0; ++i) {
            const QFix& f = T.fmul[prods[i]];
            const int e = best[px[i]] + best[py[i]] - ls[i];
            T.uni.t[i] = (int32_t)((uint32_t)f.t << e);
            T.uni.d[i] = f.d + e;
            T.uni.k[i] = (int32_t)1 << best[i];
        }
        return best_sum >= 0;
    }

    // The justified forms also take products with FEWER fraction bits than the common format but the same integer
    // bits (BasicComplexMul on Qcomplex<int<6,3>, int<6,-3>>: b d lives in int<6,-3>, RE = ac - 64 bd): left-justified, such
    // a product's range ends where the common range does, its alignment factor in RE / IM is implicit, and only its mask
    // (which floors to ITS unit) differs.  gfac[i] = log2 of that factor.
    void cplx_justified(bool uni)
    {
        const QFix &r0 = T.fmul[re], &fi = T.fmul[im];
        int gfac[4] = {0, 0, 0, 0};
        bool ru = r0.lo > INT32_MIN && r0.hi < INT32_MAX;
        // the factor each product is aligned with: TF re = A - B, im = B - C; Basic re = ac - bd, im = ad + bc
        const int32_t kf[4] = {r0.ka, r0.kb, tf ? fi.kb : fi.ka, tf ? 0 : fi.kb};
        if (tf) ru = ru && fi.ka == r0.kb;   // (B enters both with one factor)
        for (size_t i = 0; i < prods.size() && ru; ++i) {
            const QFix& f = T.fmul[prods[i]];
            gfac[i] = ilog2(kf[i]);
            if (((int64_t)1 << gfac[i]) != kf[i]) gfac[i] = -1;   // (no power of two)
            ru = gfac[i] >= 0 && gfac[i] <= 16 && f.d >= 0 && f.ka >= 1 && f.lo > INT32_MIN && f.hi < INT32_MAX &&
                 (int64_t)f.lo * kf[i] == r0.lo && ((int64_t)f.hi + 1) * kf[i] == (int64_t)r0.hi + 1;
        }
        for (const QFix* f : {&r0, &fi}) ru = ru && same_clamp(*f, r0) && f->t == 0 && f->d == 0;
        ru = ru && cplx_levels_one_clamp(r0);
        out->cplx_form_base = uni ? QCF_UNIFORM : QCF_COMPACT;
        // QCF_LJ: ... and that one range is a signed SAT::TCPL format: left-justified values (qg_fix.h).  The planes are staged with the
        // left shifts that justify each product exactly (x y 2^(s + ls - d), the addend scaled alike), so a product is one
        // saturating multiply-add + v_and, RE / IM one saturating add / subtract, a node one saturating add (+ v_and at the
        // even levels): 12.5 instead of 18 vector instructions per complex MAC (TF).
        if (!ru || r0.lo != -r0.hi - 1 || ((r0.hi + 1) & r0.hi) != 0 || r0.hi <= 0) return;
        const int Wt = 1 + width_of_hi(r0.hi);
        // word: 32 (operands of v_mad_i32_i24: 24 bits) or 16 (halves of v_pk_mad_i16: 16 bits)
        if (!cplx_justify(32, 24, Wt, gfac, &T.lj)) return;
        out->cplx_form = QCF_LJ;
        // QCF_PK16: ... in packed 16-bit halves, two outputs per register
        if (cplx_justify(16, 16, Wt, gfac, &T.lj16)) out->cplx_form = QCF_PK16;
    }

    bool cplx_justify(int word, int opbits, int Wt, const int gfac[4], QJustify* J) const
    {
        const qfmt a = d->a[0], b = d->a[1], cc = d->b[0], dd = d->b[1];
        const int sj = word - Wt;
        bool lj = sj >= 1;
        memset(J, 0, sizeof *J);
        J->s = sj;
        int E[4] = {0, 0, 0, 0};
        for (size_t i = 0; i < prods.size() && lj; ++i) {
            const QFix& f = T.fmul[prods[i]];
            E[i] = sj + gfac[i] + ilog2(f.ka) - f.d;
            lj = E[i] >= 0 && (f.d == 0 || sj + gfac[i] - f.d >= 0);
            if (lj) J->t[i] = f.d ? (int32_t)((uint32_t)f.t << (sj + gfac[i] - f.d)) : 0;
            J->g[i] = gfac[i];
        }
        if (lj && tf) {
            // products A = (a+b) c, B = (c+d) b, C = (b-a) d: every plane serves one product
            const qfmt fx[3] = {d->mul[QG_T_AB], d->mul[QG_T_CD], d->mul[QG_T_BA]}, fy[3] = {cc, b, dd};
            const int px[3] = {0, 4, 2}, py[3] = {3, 1, 5};   // planes (a+b), b, (b-a), c, (c+d), d
            for (int i = 0; i < 3 && lj; ++i) {
                int ex = E[i] < opbits - sbits(fx[i]) ? E[i] : opbits - sbits(fx[i]);
                if (ex < 0) ex = 0;
                const int ey = E[i] - ex;
                lj = sbits(fx[i]) + ex <= opbits && sbits(fy[i]) + ey <= opbits;
                J->e[px[i]] = ex;
                J->e[py[i]] = ey;
            }
        } else if (lj) {
            const qfmt pf[4] = {a, b, cc, dd};   // ac, bd, ad, bc over planes a b c d
            bool found = false;
            for (int la = 0; la <= opbits - sbits(pf[0]) && !found; ++la) {
                const int lc = E[0] - la, ld = E[2] - la, lb = E[3] - lc;
                if (lc < 0 || ld < 0 || lb < 0 || lb + ld != E[1]) continue;
                if (sbits(pf[1]) + lb > opbits || sbits(pf[2]) + lc > opbits || sbits(pf[3]) + ld > opbits) continue;
                J->e[0] = la; J->e[1] = lb; J->e[2] = lc; J->e[3] = ld;
                found = true;
            }
            lj = found;
        }
        return lj;
    }

    void finish()
    {
        if (!out->linear_ok)
            snprintf(out->reason, sizeof out->reason, "%s",
                     mixed ? (real_a ? "real x complex: exact tree evaluation, part by part" : "complex x real: exact tree evaluation, part by part")
                           : "a product or tree node may round or overflow: exact tree evaluation");
        // ring plans: decided on the formats alone (a "wide" unrounded product, 2^62 for int32 operands, is no obstacle: it is never
        // formed).  A descriptor that is exact anyway keeps its exact linear plan, one output column the one-column kernels walk
        // stays with them (they stream A once at HBM rate).
        if (!out->linear_ok && !(d->N == 1 && (out->gemv_ok || out->gemv_wide_ok))) ring_plan(d, c.raw_c || c.band, out);
        if (out->ring_ok) out->cls = QG_CLASS_LINEAR;
    }
};

} // namespace

void qg_analyze(const qgemul_desc* d, QAnalysis* out)
{
    memset(out, 0, sizeof *out);
    out->status = QG_OK;
    Analyzer a(d, out);
    if (!a.validate()) return;
    a.product();
    a.tree();
    if (!a.cx) a.linear_real();
    else if (a.mixed) a.linear_mixed();
    else a.linear_cplx();
    if (out->status != QG_OK || !a.widths_and_class()) return;
    // the real tree kernel's forms, the one-column kernel's, the complex kernel's
    a.admissions();
    a.tree_one_format();
    a.tree_records();
    a.tree_justified();
    a.tree_words();
    a.leftover0_copy();
    a.gemv_forms();
    a.cplx_forms();
    a.finish();
}

QTreeChoice qg_tree_choice(const QAnalysis* an, const qgemul_desc* d, uint32_t flags, bool ab)
{
    const bool fast = !(flags & QG_OPT_GENERIC_TREE), rt = (flags & QG_OPT_RUNTIME_MODES) != 0;
#ifdef QG_DIAG
    // A/B switches (diagnostic library): the form such a descriptor had before
    static const bool no_lj = getenv("QG_NO_LEFT_JUSTIFIED"), no_pk = getenv("QG_NO_PACKED16"), no_uniform = getenv("QG_NO_UNIFORM_CLAMP");
#else
    const bool no_lj = false, no_pk = false, no_uniform = false;
#endif
    QTreeChoice c{QG_KERNEL_TREE_I64, QTF_RUNTIME, QGF_RUNTIME, QCF_RUNTIME};
    if (an->wide) {
        c.kernel = QG_KERNEL_TREE_I128;
    } else if (d->is_complex) {
        const bool mixed = d->cmul == QG_CMUL_REAL_A || d->cmul == QG_CMUL_REAL_B;
        c.kernel = an->cplx_fast_ok && fast ? (mixed ? QG_KERNEL_TREE_RC_I32 : QG_KERNEL_TREE_CPLX_I32) : QG_KERNEL_TREE_CPLX;
        c.cplx = rt ? QCF_RUNTIME : an->cplx_form;
        // (the mixed kernel's run-time-mode form is built for at most 12 levels, qg_tree_rc.hip: longer trees take the general kernel)
        if (c.kernel == QG_KERNEL_TREE_RC_I32 && c.cplx == QCF_RUNTIME && an->tree.n_levels_k > 12) c.kernel = QG_KERNEL_TREE_CPLX;
        if (ab && no_uniform && (c.cplx == QCF_UNIFORM || c.cplx == QCF_LJ || c.cplx == QCF_PK16)) c.cplx = QCF_COMPACT;
        else if (ab && no_lj && (c.cplx == QCF_LJ || c.cplx == QCF_PK16)) c.cplx = an->cplx_form_base;
        else if (ab && no_pk && c.cplx == QCF_PK16) c.cplx = QCF_LJ;
    } else if ((an->gemv_ok || (an->gemv_wide_ok && an->gemv_w32 && !rt && an->tree.n_levels_k >= 8)) && fast) {
        // (32-bit words on the one-column kernel, QAnalysis::gemv_w32: rows of at least 256 leaves; like QTF_WORD they have no
        //  run-time-mode form, QG_OPT_RUNTIME_MODES keeps the 64-bit-value form — the tests' second opinion)
        c.kernel = QG_KERNEL_GEMV_I32;
        c.gemv = rt ? QGF_RUNTIME : an->gemv_form;
    } else if (an->gemv_wide_ok && fast) {
        c.kernel = QG_KERNEL_GEMV_I64;
    } else if (an->tree_fast_ok && fast && !(rt && an->tree_form >= QTF_WORD && an->tree_form <= QTF_WORD_WRAP)) {
        // (the 32-bit words have no run-time-mode form on that kernel: QG_OPT_RUNTIME_MODES takes the 64-bit one)
        c.kernel = QG_KERNEL_TREE_I32;
        c.tree = rt ? QTF_RUNTIME : an->tree_form;
        const bool pk = c.tree == QTF_PK16 || c.tree == QTF_PK16_HYB || c.tree == QTF_PK16_HYB16, pku = c.tree == QTF_PK16_U || c.tree == QTF_PK16_HYB_U || c.tree == QTF_PK16_HYB16_U;
        if (ab && no_lj && (c.tree == QTF_LJ || c.tree == QTF_LJ_U || pk || pku)) c.tree = an->tree_form_base;
        else if (ab && no_pk && (pk || pku)) c.tree = pku ? QTF_LJ_U : QTF_LJ;
    }
    return c;
}

const char* qg_form_name(QTreeForm f)
{
    switch (f) {
    case QTF_ONE_ZERO: return "one format, SAT::ZERO";
    case QTF_ONE_TCPL: return "one format, SAT::TCPL";
    case QTF_REC_CLAMP: return "per-level formats, compact (clamps)";
    case QTF_REC_BIASED: return "per-level formats, compact";
    case QTF_REC_KINDS: return "per-level formats, compact (unbiased)";
    case QTF_LJ: case QTF_LJ_U: return "one format, SAT::TCPL, left-justified";
    case QTF_PK16: case QTF_PK16_U: return "one format, SAT::TCPL, left-justified, packed 16-bit";
    case QTF_PK16_HYB: case QTF_PK16_HYB16: case QTF_PK16_HYB_U: case QTF_PK16_HYB16_U: return "one format, SAT::TCPL, left-justified, packed nodes";
    case QTF_WORD: case QTF_WORD_MAD: return "one 32-bit format, SAT::TCPL, saturating word adds";
    case QTF_JWORD: case QTF_JWORD_MAD: return "one format, SAT::TCPL, justified words";
    case QTF_WORD_WRAP: return "one 32-bit format, WRP::TCPL, wrapping word adds";
    default: return "run-time modes";
    }
}

const char* qg_form_name(QGemvForm f)
{
    switch (f) {
    case QGF_ONE_ZERO: return "one format, SAT::ZERO";
    case QGF_ONE_TCPL: return "one format, SAT::TCPL";
    case QGF_REC_CLAMP: return "per-level formats, compact (clamps)";
    case QGF_REC_KINDS: return "per-level formats, compact";
    case QGF_WORD: case QGF_WORD_RND: return "one 32-bit format, saturating adds";
    default: return "run-time modes";
    }
}

const char* qg_form_name(QCplxForm f)
{
    switch (f) {
    case QCF_TABLE: return "fixed modes, table";
    case QCF_COMPACT: return "fixed modes, compact";
    case QCF_KINDS: return "compact, rounding / overflow kinds";
    case QCF_UNIFORM: return "fixed modes, one clamp for the whole loop";
    case QCF_LJ: return "fixed modes, one clamp, left-justified";
    case QCF_PK16: return "fixed modes, one clamp, packed 16-bit";
    case QCF_KINDS_R: case QCF_KINDS_Z: case QCF_KINDS_RZ: case QCF_KINDS_W: case QCF_KINDS_RW: case QCF_KINDS_ALL:
        return "compact, branch-free rounding / overflow kinds";
    default: return "run-time modes";
    }
}
