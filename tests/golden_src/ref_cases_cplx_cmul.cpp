// ref_cases_cplx_cmul.cpp — generator of tests/golden/ref_cplx_cmul_0.jsonl.gz: the reference's lazy tensor Qmul on two COMPLEX
// tensors (its own header, through oracle/ref_driver.hpp) — BasicComplexMul, TFComplexMul and no tags, both operand orders, tensor
// and scalar operands, alone and inside chains with the part-wise operators — and the tensors' converting construction from the
// resulting expressions.  A tensor X of the complex "C" element type with synthetic raw values stands for a complex Qgemul result.
// Printed per operator: the operand's formats, the operator's result type as the reference's types report it, the element type of
// the tensor it was assigned to, the operand's raw values and, for a complex x complex Qmul (op 6), the algorithm and the resolved
// format of every sub-operation (ref_driver.hpp: mul_slots, from the reference's own member typedefs); then the raw values of the
// final tensor D, part by part.  The records are data: formats, raw inputs, the reference's raw results.
// Build and run (the recipe of oracle/Makefile's _ref/% rule; REF_INC = the reference's include directory):
//     clang++ -std=c++23 -O2 -w -I$(REF_INC) -Ioracle tests/golden_src/ref_cases_cplx_cmul.cpp -o oracle/_ref/ref_cases_cplx_cmul
//     oracle/_ref/ref_cases_cplx_cmul | gzip -9n > tests/golden/ref_cplx_cmul_0.jsonl.gz
#include "ref_driver.hpp"

using namespace refdrv;

enum { ADD = 1, SUB = 2, MUL = 3, CMUL = 6 };

template <int OP, bool XFIRST, class... Tags>
struct Op {
    template <class X, class E>
    static auto apply(const X& x, const E& e)
    {
        if constexpr (OP == MUL) { if constexpr (XFIRST) return Qmul<Tags...>(x, e); else return Qmul<Tags...>(e, x); }
        else if constexpr (OP == ADD) { if constexpr (XFIRST) return Qadd<Tags...>(x, e); else return Qadd<Tags...>(e, x); }
        else { if constexpr (XFIRST) return Qsub<Tags...>(x, e); else return Qsub<Tags...>(e, x); }
    }
    template <class XT, class ET>
    using res_t = decltype(apply(std::declval<XT>(), std::declval<ET>()));
    template <class XT, class ET>
    using slots = std::conditional_t<XFIRST, mul_slots<XT, ET, TypeList<Tags...>>, mul_slots<ET, XT, TypeList<Tags...>>>;
    static constexpr int op = OP;
    static constexpr bool xfirst = XFIRST;
};

template <class T, size_t N>
Qu_s<dim<N>, T> make_tensor(uint64_t seed, int dist, std::vector<int64_t>& re, std::vector<int64_t>& im)
{
    Qu_s<dim<N>, T> t;
    re.resize(N);
    im.resize(N);
    for (size_t i = 0; i < N; ++i) {
        re[i] = synth<typename parts<T>::re>(seed, dist, i, 0);
        im[i] = is_cplx<T> ? synth<typename parts<T>::im>(seed, dist, i, 1) : 0;
        set_raw(t[i], re[i], im[i]);
    }
    return t;
}

static std::string vec_json(const char* key, const std::vector<int64_t>& v)
{
    std::string s = std::string("\"") + key + "\":[";
    for (size_t i = 0; i < v.size(); ++i) s += (i ? "," : "") + std::to_string((long long)v[i]);
    return s + "]";
}

// one operator: X (complex elements XT) op E (tensor or scalar of ET, complex or real) -> tensor of TT
template <class OpT, class XT, class ET, class TT, bool SCALAR, size_t N>
Qu_s<dim<N>, TT> stage(const Qu_s<dim<N>, XT>& X, uint64_t seed, int dist, std::string& js)
{
    using r_t = typename OpT::template res_t<XT, ET>;
    static_assert(is_cplx<r_t> && is_cplx<TT>);
    constexpr bool cm = OpT::op == MUL && is_cplx<ET>;
    char buf[512];
    std::snprintf(buf, sizeof buf, "{\"op\":%d,\"x_first\":%d,\"scalar\":%d,\"e_complex\":%d,\"e\":%s,\"r\":%s,\"t\":%s,", cm ? int(CMUL) : OpT::op,
                  int(OpT::xfirst), int(SCALAR), int(is_cplx<ET>), fmt2_json<ET>().c_str(), fmt2_json<r_t>().c_str(), fmt2_json<TT>().c_str());
    js += buf;
    if constexpr (cm) {
        using S = typename OpT::template slots<XT, ET>;
        js += "\"cmul\":" + std::to_string(S::cmul) + ",\"mul\":" + S::json() + ",";
    }
    std::vector<int64_t> ere, eim;
    if constexpr (SCALAR) {
        ET e;
        ere = {synth<typename parts<ET>::re>(seed, dist, 0, 0)};
        eim = {is_cplx<ET> ? synth<typename parts<ET>::im>(seed, dist, 0, 1) : 0};
        set_raw(e, ere[0], eim[0]);
        Qu_s<dim<N>, TT> out = OpT::apply(X, e);
        js += vec_json("Ere", ere) + "," + vec_json("Eim", eim) + "}";
        return out;
    } else {
        auto E = make_tensor<ET, N>(seed, dist, ere, eim);
        Qu_s<dim<N>, TT> out = OpT::apply(X, E);
        js += vec_json("Ere", ere) + "," + vec_json("Eim", eim) + "}";
        return out;
    }
}

template <class CT, class DT, size_t N>
void emit(const char* name, const std::vector<int64_t>& xre, const std::vector<int64_t>& xim, const std::string& stages, const Qu_s<dim<N>, DT>& D)
{
    std::vector<int64_t> dre(N), dim_(N);
    for (size_t i = 0; i < N; ++i) get_raw(D[i], dre[i], dim_[i]);
    std::printf("{\"name\":\"%s\",\"n\":%zu,\"c\":%s,%s,%s,\"stages\":[%s],\"d\":%s,%s,%s}\n", name, N, fmt2_json<CT>().c_str(),
                vec_json("Xre", xre).c_str(), vec_json("Xim", xim).c_str(), stages.c_str(), fmt2_json<DT>().c_str(), vec_json("Dre", dre).c_str(),
                vec_json("Dim", dim_).c_str());
}

// the same seeds for every one-operator case: records that differ in one tag only are comparable value by value
template <class CT, class OpT, class ET, class DT, bool SCALAR = false, size_t N = 64>
void case1(const char* name, int dist)
{
    std::vector<int64_t> xre, xim;
    auto X = make_tensor<CT, N>(161, dist, xre, xim);
    std::string js;
    auto D = stage<OpT, CT, ET, DT, SCALAR, N>(X, 162, dist, js);
    emit<CT, DT, N>(name, xre, xim, js, D);
}

template <class CT, class Op1, class E1, class T1, bool S1, class Op2, class E2, class DT, bool S2, size_t N = 64>
void case2(const char* name, int dist)
{
    std::vector<int64_t> xre, xim;
    auto X = make_tensor<CT, N>(171, dist, xre, xim);
    std::string js;
    auto T = stage<Op1, CT, E1, T1, S1, N>(X, 172, dist, js);
    js += ",";
    auto D = stage<Op2, T1, E2, DT, S2, N>(T, 173, dist, js);
    emit<CT, DT, N>(name, xre, xim, js, D);
}

template <class CT, class Op1, class E1, class T1, bool S1, class Op2, class E2, class T2, bool S2, class Op3, class E3, class DT, bool S3, size_t N = 64>
void case3(const char* name, int dist)
{
    std::vector<int64_t> xre, xim;
    auto X = make_tensor<CT, N>(181, dist, xre, xim);
    std::string js;
    auto Ta = stage<Op1, CT, E1, T1, S1, N>(X, 182, dist, js);
    js += ",";
    auto Tb = stage<Op2, T1, E2, T2, S2, N>(Ta, 183, dist, js);
    js += ",";
    auto D = stage<Op3, T2, E3, DT, S3, N>(Tb, 184, dist, js);
    emit<CT, DT, N>(name, xre, xim, js, D);
}

// part types
using x64 = Qu<intBits<6>, fracBits<4>>;                          // the running value: 11 storage bits
using e35 = Qu<intBits<3>, fracBits<5>>;                          // the operand: 9 storage bits
using r63 = Qu<intBits<6>, fracBits<3>, QuMode<RND::POS_INF>, OfMode<SAT::TCPL>>;
using r6n3 = Qu<intBits<6>, fracBits<-3>, QuMode<RND::POS_INF>, OfMode<SAT::TCPL>>;
using r54 = Qu<intBits<5>, fracBits<4>>;
using r32 = Qu<intBits<3>, fracBits<2>>;
using s22 = Qu<intBits<2>, fracBits<2>>;
using u44 = Qu<intBits<4>, fracBits<4>, isSigned<false>>;
using r104 = Qu<intBits<10>, fracBits<4>, QuMode<RND::CONV>, OfMode<SAT::SMGN>>;
using r82z = Qu<intBits<8>, fracBits<2>, QuMode<TRN::TCPL>, OfMode<SAT::ZERO>>;
using r73w = Qu<intBits<7>, fracBits<3>, QuMode<RND::ZERO>, OfMode<WRP::TCPL>>;
using r91s = Qu<intBits<9>, fracBits<1>, QuMode<TRN::SMGN>, OfMode<SAT::SMGN>>;
using r206 = Qu<intBits<20>, fracBits<6>>;
using w2412 = Qu<intBits<24>, fracBits<12>>;                      // 37 storage bits: an int64 host part
using w1012 = Qu<intBits<10>, fracBits<12>>;
using w4018 = Qu<intBits<40>, fracBits<18>>;                      // 59 storage bits
// complex element types
using cx = Qcomplex<x64, x64>;
using ce = Qcomplex<e35, e35>;
using c5 = Qcomplex<r63, r6n3>;                                   // parts of different formats, one with negative fracBits
using cb = Qcomplex<r54, r32>;
using cu = Qcomplex<u44, r54>;
using cd = Qcomplex<r104, r82z>;
using cq = Qcomplex<r73w, r91s>;
using cw = Qcomplex<r206, r206>;
using cwx = Qcomplex<w2412, w2412>;
using cwe = Qcomplex<w1012, w1012>;
using cwd = Qcomplex<w4018, w4018>;

// one tag per sub-operation: the seven QuModes and the four OfModes between them
using tAC = acT<intBits<8>, fracBits<3>, QuMode<RND::POS_INF>>;
using tBD = bdT<fracBits<2>, QuMode<RND::NEG_INF>, OfMode<SAT::ZERO>>;
using tAD = adT<fracBits<1>, QuMode<RND::ZERO>, OfMode<WRP::TCPL>>;
using tBC = bcT<fracBits<2>, QuMode<RND::INF>, OfMode<SAT::SMGN>>;
using tACBD = acbdT<intBits<5>, fracBits<2>, QuMode<RND::CONV>>;
using tADBC = adbcT<intBits<5>, fracBits<1>, QuMode<TRN::SMGN>, OfMode<WRP::TCPL>>;
using tAB = abT<intBits<6>, fracBits<3>, QuMode<RND::INF>>;
using tCD = cdT<intBits<3>, fracBits<4>, QuMode<RND::ZERO>, OfMode<WRP::TCPL>>;
using tBA = baT<intBits<2>, fracBits<0>, OfMode<SAT::ZERO>>;     // never honoured by the reference
using tABC = abcT<intBits<8>, fracBits<3>, QuMode<RND::CONV>>;
using tCDB = cdbT<intBits<7>, fracBits<2>, QuMode<RND::NEG_INF>, OfMode<SAT::SMGN>>;   // lands on C = (b - a) d
using tBAD = badT<intBits<6>, fracBits<4>, QuMode<RND::POS_INF>, OfMode<SAT::ZERO>>;   // lands on B = (c + d) b
using tABT = ABT<intBits<7>, fracBits<2>, QuMode<TRN::SMGN>>;
using tBCT = BCT<intBits<6>, fracBits<3>, OfMode<WRP::TCPL>>;
using wide_full = BasicComplexMul<acT<FullPrec>, bdT<FullPrec>, adT<FullPrec>, bcT<FullPrec>, acbdT<FullPrec>, adbcT<FullPrec>>;

int main()
{
    // BasicComplexMul: no tags at all, the empty wrapper, each sub-operation's tag alone, all six, loose tags; both orders
    case1<cx, Op<MUL, true>, ce, cd>("basic_no_tags", 2);
    case1<cx, Op<MUL, false>, ce, cd>("basic_no_tags_efirst", 2);
    case1<cx, Op<MUL, true, BasicComplexMul<tAC>>, ce, cd>("basic_acT", 2);
    case1<cx, Op<MUL, true, BasicComplexMul<tBD>>, ce, cd>("basic_bdT", 2);
    case1<cx, Op<MUL, true, BasicComplexMul<tAD>>, ce, cd>("basic_adT", 2);
    case1<cx, Op<MUL, true, BasicComplexMul<tBC>>, ce, cd>("basic_bcT", 2);
    case1<cx, Op<MUL, true, BasicComplexMul<tACBD>>, ce, cq>("basic_acbdT", 2);
    case1<cx, Op<MUL, true, BasicComplexMul<tADBC>>, ce, cq>("basic_adbcT", 2);
    case1<cx, Op<MUL, false, BasicComplexMul<tAC, tBD, tAD, tBC, tACBD, tADBC>>, ce, cq>("basic_all_six_efirst", 0);
    case1<cx, Op<MUL, true, BasicComplexMul<intBits<7>, fracBits<3>, QuMode<RND::CONV>>>, ce, cd>("basic_loose_tags", 2);
    // TFComplexMul: no tags, baT alone (no effect: equal to tf_no_tags value by value), all eight, loose tags; both orders
    case1<cx, Op<MUL, true, TFComplexMul<>>, ce, cd>("tf_no_tags", 2);
    case1<cx, Op<MUL, true, TFComplexMul<tBA>>, ce, cd>("tf_baT_only", 2);
    case1<cx, Op<MUL, false, TFComplexMul<>>, ce, cd>("tf_no_tags_efirst", 2);
    case1<cx, Op<MUL, true, TFComplexMul<tAB, tCD, tBA, tABC, tCDB, tBAD, tABT, tBCT>>, ce, cq>("tf_all_eight", 0);
    case1<cx, Op<MUL, false, TFComplexMul<tAB, tCD, tBA, tABC, tCDB, tBAD, tABT, tBCT>>, ce, cq>("tf_all_eight_efirst", 2);
    case1<cx, Op<MUL, true, TFComplexMul<intBits<8>, fracBits<2>, QuMode<RND::NEG_INF>, OfMode<SAT::SMGN>>>, ce, cd>("tf_loose_tags", 2);
    // a complex scalar operand
    case1<cx, Op<MUL, true, BasicComplexMul<tAC, tACBD>>, ce, cd, true>("basic_scalar", 2);
    case1<cx, Op<MUL, false, TFComplexMul<tABC, tBCT>>, cb, cq, true>("tf_scalar_efirst", 0);
    // parts of different formats (negative fracBits, an unsigned part)
    case1<c5, Op<MUL, true>, cb, cd>("mixed_parts_basic", 2);
    case1<c5, Op<MUL, false, TFComplexMul<>>, cu, cq>("mixed_parts_tf_unsigned_efirst", 2);
    // chains: the stage's tensor type differs from the result type; part-wise stages before and after; two CMUL stages
    case2<cx, Op<MUL, true, BasicComplexMul<tAC>>, ce, cq, false, Op<MUL, true>, s22, cd, true>("cmul_into_then_real_scale", 2);
    case3<cx, Op<ADD, true>, cb, cw, false, Op<MUL, true, TFComplexMul<tABC>>, ce, c5, false, Op<MUL, false, imagT<r91s>>, r32, cq, false>("add_cmul_mul_by_real", 0);
    case2<cx, Op<MUL, true>, ce, cx, false, Op<MUL, false, TFComplexMul<>>, cb, cd, true>("cmul_then_cmul", 1);
    // 8-byte parts: full-precision products of 37- and 23-bit parts (60 bits), their sums near 62
    case1<cwx, Op<MUL, true, wide_full>, cwe, cwd, false, 128>("wide_basic_fullprec", 0);
    case1<cwx, Op<MUL, false, TFComplexMul<abcT<FullPrec>, cdbT<FullPrec>, badT<FullPrec>>>, cwe, cwd, false, 128>("wide_tf_fullprec_efirst", 0);
    return 0;
}
