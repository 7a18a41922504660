// ref_cases_mixed.cpp — generator of tests/golden/ref_mixed_0.jsonl.gz: GEMMs of the reference (its own header, through the helpers
// of oracle/ref_driver.hpp) with ONE real and ONE complex operand, the "Real-Complex Operations" of QuBLAS.h:3600-3644:
//     p[k]   = Qmul<MulTags...>(A'[i,k], B[k,j])      real x complex or complex x real: part-wise, realT / imagT tags
//     s      = Qreduce<Levels...>(p)                   the complex tree (QuBLAS.h:3549-3564, :4966)
//     C[i,j] = s                                       converting constructor, part by part
// Cases, each in both operand orders: default tags on Qu<4,3> x configuration 5's element, realT / imagT tags with different
// formats per part, two bare Qu types as tags, a complex level-type list, wide exact product and level types, TransposedA,
// K = 1, 2, 5, 37, 64 and 1000, the edge distribution and full-range operands, a 70-bit level type, narrow C on full-range inputs.
// The records are data: formats as the reference's own types report them, seeds, the reference's raw results.
// Build and run (the recipe of oracle/Makefile's _ref/% rule; REF_INC = the reference's include directory):
//     clang++ -std=c++23 -O2 -w -I$(REF_INC) -Ioracle tests/golden_src/ref_cases_mixed.cpp -o oracle/_ref/ref_cases_mixed
//     oracle/_ref/ref_cases_mixed | gzip -9n > tests/golden/ref_mixed_0.jsonl.gz
#include "ref_driver.hpp"
using namespace refdrv;

// the mixed form of ref_driver.hpp's run_case: complex-ness is a property of each operand
template <class EA, class EB, class EC, class MulList, class AddList, bool TA, size_t M, size_t N, size_t K>
static void run_mixed(const char* name, uint64_t seedA, uint64_t seedB, int dist, FILE* out)
{
    using prod_t = decltype(apply_mul<MulList>::mul(std::declval<EA>(), std::declval<EB>()));
    constexpr size_t NL = ceil_log2(K);
    constexpr bool ca = is_cplx<EA>, cb = is_cplx<EB>;
    static_assert(ca != cb && is_cplx<EC> && is_cplx<prod_t>);
    std::vector<EA> A(M * K);
    std::vector<EB> B(K * N);
    for (size_t e = 0; e < M * K; ++e)
        set_raw(A[e], synth<typename parts<EA>::re>(seedA, dist, e, 0), ca ? synth<typename parts<EA>::im>(seedA, dist, e, 1) : 0);
    for (size_t e = 0; e < K * N; ++e)
        set_raw(B[e], synth<typename parts<EB>::re>(seedB, dist, e, 0), cb ? synth<typename parts<EB>::im>(seedB, dist, e, 1) : 0);
    std::vector<raw_t> C(M * N * 2);
    std::vector<EA> arow(K);
    std::vector<EB> bcol(K);
    for (size_t j = 0; j < N; ++j) {
        for (size_t k = 0; k < K; ++k) bcol[k] = B[k + j * K];
        for (size_t i = 0; i < M; ++i) {
            for (size_t k = 0; k < K; ++k) arow[k] = TA ? A[k + i * K] : A[i + k * M];
            EC c = ref_dot<EA, EB, EC, MulList, AddList, K>(arow, bcol);
            get_raw(c, C[2 * (i + j * M)], C[2 * (i + j * M) + 1]);
        }
    }
    std::string la, lv;
    print_levels<0, NL, prod_t, AddList>(la, lv);
    const std::string z = "[0,0,0,0,0]";
    auto opnd = [&](bool cx, std::string re, std::string im) { return "[" + re + "," + (cx ? im : z) + "]"; };
    std::fprintf(out, "{\"name\":\"%s\",\"M\":%zu,\"N\":%zu,\"K\":%zu,\"transA\":%d,\"is_complex\":1,\"cmul\":%d,\n", name, M, N, K, int(TA), ca ? 4 : 3);
    std::fprintf(out, " \"a\":%s,\"b\":%s,\"c\":%s,\n", opnd(ca, fmt_json<typename parts<EA>::re>(), fmt_json<typename parts<EA>::im>()).c_str(),
                 opnd(cb, fmt_json<typename parts<EB>::re>(), fmt_json<typename parts<EB>::im>()).c_str(), fmt2_json<EC>().c_str());
    std::string mul = "[" + fmt_json<typename prod_t::realType>() + "," + fmt_json<typename prod_t::imagType>();
    for (int i = 2; i < 8; ++i) mul += "," + z;
    std::fprintf(out, " \"mul\":%s],\"n_levels\":%zu,\n \"level_add\":[%s],\"level\":[%s],\n", mul.c_str(), NL, la.c_str(), lv.c_str());
    std::fprintf(out, " \"inputs\":{\"seedA\":%llu,\"seedB\":%llu,\"dist\":%d},\n \"C\":[", (unsigned long long)seedA, (unsigned long long)seedB, dist);
    for (size_t e = 0; e < C.size(); ++e) std::fprintf(out, "%s%s", e ? "," : "", dec(C[e]).c_str());
    std::fprintf(out, "]}\n");
}

// both operand orders of one case: R x Z ("ra") and Z x R ("rb")
template <class R, class Z, class EC, class MulList, class AddList, bool TA, size_t M, size_t N, size_t K>
static void both(const char* name, uint64_t seed, int dist, FILE* out)
{
    const std::string s(name);
    run_mixed<R, Z, EC, MulList, AddList, TA, M, N, K>((s + "_ra").c_str(), seed, seed + 1, dist, out);
    run_mixed<Z, R, EC, MulList, AddList, TA, M, N, K>((s + "_rb").c_str(), seed + 2, seed + 3, dist, out);
}

using e43 = Qu<intBits<4>, fracBits<3>>;
using r63 = Qu<intBits<6>, fracBits<3>, isSigned<true>, QuMode<RND::POS_INF>, OfMode<SAT::TCPL>>;
using i63n = Qu<intBits<6>, fracBits<-3>, isSigned<true>, QuMode<RND::POS_INF>, OfMode<SAT::TCPL>>;
using c5 = Qcomplex<r63, i63n>;   // configuration 5's element
using cC = Qcomplex<Qu<intBits<14>, fracBits<3>>, Qu<intBits<14>, fracBits<3>>>;   // wide enough for 1000 products of the default format
using e88 = Qu<intBits<8>, fracBits<8>>;
using c88 = Qcomplex<Qu<intBits<8>, fracBits<8>>, Qu<intBits<7>, fracBits<5>>>;

int main()
{
    FILE* out = stdout;
    // default tags (both parts land in (6,3)), every K, edges and full range
    both<e43, c5, cC, TypeList<>, TypeList<>, false, 5, 3, 1>("default_5x3xK1_edges", 101, 2, out);
    both<e43, c5, cC, TypeList<>, TypeList<>, false, 5, 3, 2>("default_5x3xK2_edges", 105, 2, out);
    both<e43, c5, cC, TypeList<>, TypeList<>, false, 5, 3, 5>("default_5x3xK5_edges", 109, 2, out);
    both<e43, c5, cC, TypeList<>, TypeList<>, false, 9, 7, 37>("default_9x7xK37_full", 113, 0, out);
    both<e43, c5, cC, TypeList<>, TypeList<>, true, 9, 7, 37>("default_9x7xK37_tn_edges", 117, 2, out);
    both<e43, c5, cC, TypeList<>, TypeList<>, false, 6, 5, 64>("default_6x5xK64_full", 121, 0, out);
    both<e43, c5, cC, TypeList<>, TypeList<>, false, 3, 2, 1000>("default_3x2xK1000_full", 125, 0, out);
    // narrow C on full-range operands: the saturation case
    both<e43, c5, c5, TypeList<>, TypeList<>, false, 6, 5, 64>("default_narrowC_6x5xK64_full_saturation", 129, 0, out);
    // realT / imagT tags with different formats per part
    using RI = TypeList<realT<Qu<intBits<12>, fracBits<6>>>, imagT<intBits<10>, fracBits<0>>>;
    using cRI = Qcomplex<Qu<intBits<18>, fracBits<6>>, Qu<intBits<16>, fracBits<0>>>;
    both<e43, c5, cRI, RI, TypeList<>, false, 9, 7, 37>("realT_imagT_9x7xK37_edges", 133, 2, out);
    both<e43, c5, cRI, RI, TypeList<>, true, 6, 5, 64>("realT_imagT_6x5xK64_tn_full", 137, 0, out);
    // one part tagged, loose tags for the other
    using RL = TypeList<realT<intBits<9>, fracBits<2>, QuMode<RND::CONV>>, OfMode<SAT::ZERO>>;
    both<e43, c5, cC, RL, TypeList<>, false, 9, 7, 37>("realT_loose_9x7xK37_full", 141, 0, out);
    // two bare Qu types as tags: <realT<first>, imagT<second>>
    using QQ = TypeList<Qu<intBits<7>, fracBits<5>, QuMode<RND::ZERO>, OfMode<SAT::SMGN>>, Qu<intBits<9>, fracBits<-1>, QuMode<TRN::SMGN>, OfMode<WRP::TCPL>>>;
    both<e43, c5, cC, QQ, TypeList<>, false, 9, 7, 37>("two_types_9x7xK37_edges", 145, 2, out);
    both<e88, c88, cC, QQ, TypeList<>, false, 5, 3, 5>("two_types_e88_5x3xK5_full", 149, 0, out);
    // a complex level-type list (the add tag is ignored, the level buffer converts)
    using l1 = Qcomplex<Qu<intBits<8>, fracBits<4>, QuMode<RND::CONV>, OfMode<SAT::SMGN>>, Qu<intBits<9>, fracBits<1>, QuMode<TRN::SMGN>, OfMode<SAT::ZERO>>>;
    using l2 = Qcomplex<Qu<intBits<12>, fracBits<2>, QuMode<RND::ZERO>>, Qu<intBits<12>, fracBits<3>, QuMode<RND::INF>, OfMode<WRP::TCPL>>>;
    both<e43, c5, cC, TypeList<>, TypeList<l1, l2>, false, 9, 7, 37>("levels_9x7xK37_full", 153, 0, out);
    both<e43, c5, cC, RI, TypeList<l1, l2>, true, 3, 2, 1000>("levels_tags_3x2xK1000_tn_edges", 157, 2, out);
    // wide exact product and level types: nothing rounds or overflows before C
    using WP = TypeList<realT<Qu<intBits<12>, fracBits<6>>>, imagT<Qu<intBits<12>, fracBits<3>>>>;
    using lw = Qcomplex<Qu<intBits<24>, fracBits<6>>, Qu<intBits<24>, fracBits<3>>>;
    using cW = Qcomplex<Qu<intBits<20>, fracBits<4>>, Qu<intBits<20>, fracBits<3>>>;
    both<e43, c5, cW, WP, TypeList<lw>, false, 9, 7, 37>("exact_9x7xK37_full", 161, 0, out);
    both<e88, c88, Qcomplex<Qu<intBits<28>, fracBits<10>>, Qu<intBits<27>, fracBits<13>>>,
         TypeList<realT<Qu<intBits<17>, fracBits<16>>>, imagT<Qu<intBits<16>, fracBits<13>>>>,
         TypeList<Qcomplex<Qu<intBits<28>, fracBits<16>>, Qu<intBits<27>, fracBits<13>>>>, false, 6, 5, 64>("exact_e88_6x5xK64_full", 165, 0, out);
    // a level type of 70 bits: multi-word values
    using l70 = Qcomplex<Qu<intBits<40>, fracBits<30>>, Qu<intBits<12>, fracBits<3>>>;
    both<e43, c5, cW, TypeList<>, TypeList<l70>, false, 9, 7, 37>("level70_9x7xK37_full", 169, 0, out);
    return 0;
}
