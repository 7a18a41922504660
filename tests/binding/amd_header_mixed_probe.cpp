// Compiles include/QuBLAS_amd.h on its own (no reference header) and prints the descriptors it lowers for Qgemul calls with one real
// and one complex operand: the tags of tests/golden_src/ref_cases_mixed.cpp, names as in tests/golden/ref_mixed_0.
#include <string>

#include "QuBLAS_amd.h"
#include "desc_json.hpp"

using namespace QuBLAS_amd;

template <class EC, class EA, class EB, size_t M, size_t N, size_t K, bool TA, class... Tags>
void probe(const std::string& name)
{
    Qu<dim<M, N>, EC> C;
    std::conditional_t<TA, Qu<dim<K, M>, EA>, Qu<dim<M, K>, EA>> A;
    Qu<dim<K, N>, EB> B;
    if constexpr (TA) print_desc(name.c_str(), Qgemul_lower<QgemulTransposedA<true>, Tags...>(C, A, B));
    else print_desc(name.c_str(), Qgemul_lower<Tags...>(C, A, B));
}
// both operand orders of one case
template <class R, class Z, class EC, size_t M, size_t N, size_t K, bool TA, class... Tags>
void both(const char* name)
{
    probe<EC, R, Z, M, N, K, TA, Tags...>(std::string(name) + "_ra");
    probe<EC, Z, R, M, N, K, TA, Tags...>(std::string(name) + "_rb");
}

using e43 = Qu<intBits<4>, fracBits<3>>;
using r63 = Qu<intBits<6>, fracBits<3>, isSigned<true>, QuMode<RND::POS_INF>, OfMode<SAT::TCPL>>;
using i63n = Qu<intBits<6>, fracBits<-3>, isSigned<true>, QuMode<RND::POS_INF>, OfMode<SAT::TCPL>>;
using c5 = Qcomplex<r63, i63n>;
using cC = Qcomplex<Qu<intBits<14>, fracBits<3>>, Qu<intBits<14>, fracBits<3>>>;
using e88 = Qu<intBits<8>, fracBits<8>>;
using c88 = Qcomplex<Qu<intBits<8>, fracBits<8>>, Qu<intBits<7>, fracBits<5>>>;

int main()
{
    both<e43, c5, cC, 5, 3, 1, false>("default_5x3xK1_edges");
    both<e43, c5, cC, 5, 3, 2, false>("default_5x3xK2_edges");
    both<e43, c5, cC, 5, 3, 5, false>("default_5x3xK5_edges");
    both<e43, c5, cC, 9, 7, 37, false>("default_9x7xK37_full");
    both<e43, c5, cC, 6, 5, 64, false>("default_6x5xK64_full");
    both<e43, c5, cC, 3, 2, 1000, false>("default_3x2xK1000_full");
    both<e43, c5, cC, 9, 7, 37, true>("default_9x7xK37_tn_edges");
    both<e43, c5, c5, 6, 5, 64, false>("default_narrowC_6x5xK64_full_saturation");
    using RI = QgemulMulArgs<realT<Qu<intBits<12>, fracBits<6>>>, imagT<intBits<10>, fracBits<0>>>;
    using cRI = Qcomplex<Qu<intBits<18>, fracBits<6>>, Qu<intBits<16>, fracBits<0>>>;
    both<e43, c5, cRI, 9, 7, 37, false, RI>("realT_imagT_9x7xK37_edges");
    both<e43, c5, cRI, 6, 5, 64, true, RI>("realT_imagT_6x5xK64_tn_full");
    using RL = QgemulMulArgs<realT<intBits<9>, fracBits<2>, QuMode<RND::CONV>>, OfMode<SAT::ZERO>>;
    both<e43, c5, cC, 9, 7, 37, false, RL>("realT_loose_9x7xK37_full");
    using QQ = QgemulMulArgs<Qu<intBits<7>, fracBits<5>, QuMode<RND::ZERO>, OfMode<SAT::SMGN>>, Qu<intBits<9>, fracBits<-1>, QuMode<TRN::SMGN>, OfMode<WRP::TCPL>>>;
    both<e43, c5, cC, 9, 7, 37, false, QQ>("two_types_9x7xK37_edges");
    both<e88, c88, cC, 5, 3, 5, false, QQ>("two_types_e88_5x3xK5_full");
    using l1 = Qcomplex<Qu<intBits<8>, fracBits<4>, QuMode<RND::CONV>, OfMode<SAT::SMGN>>, Qu<intBits<9>, fracBits<1>, QuMode<TRN::SMGN>, OfMode<SAT::ZERO>>>;
    using l2 = Qcomplex<Qu<intBits<12>, fracBits<2>, QuMode<RND::ZERO>>, Qu<intBits<12>, fracBits<3>, QuMode<RND::INF>, OfMode<WRP::TCPL>>>;
    both<e43, c5, cC, 9, 7, 37, false, QgemulAddArgs<l1, l2>>("levels_9x7xK37_full");
    both<e43, c5, cC, 3, 2, 1000, true, RI, QgemulAddArgs<l1, l2>>("levels_tags_3x2xK1000_tn_edges");
    using WP = QgemulMulArgs<realT<Qu<intBits<12>, fracBits<6>>>, imagT<Qu<intBits<12>, fracBits<3>>>>;
    using lw = Qcomplex<Qu<intBits<24>, fracBits<6>>, Qu<intBits<24>, fracBits<3>>>;
    using cW = Qcomplex<Qu<intBits<20>, fracBits<4>>, Qu<intBits<20>, fracBits<3>>>;
    both<e43, c5, cW, 9, 7, 37, false, WP, QgemulAddArgs<lw>>("exact_9x7xK37_full");
    both<e88, c88, Qcomplex<Qu<intBits<28>, fracBits<10>>, Qu<intBits<27>, fracBits<13>>>, 6, 5, 64, false,
         QgemulMulArgs<realT<Qu<intBits<17>, fracBits<16>>>, imagT<Qu<intBits<16>, fracBits<13>>>>,
         QgemulAddArgs<Qcomplex<Qu<intBits<28>, fracBits<16>>, Qu<intBits<27>, fracBits<13>>>>>("exact_e88_6x5xK64_full");
    using l70 = Qcomplex<Qu<intBits<40>, fracBits<30>>, Qu<intBits<12>, fracBits<3>>>;
    both<e43, c5, cW, 9, 7, 37, false, QgemulAddArgs<l70>>("level70_9x7xK37_full");
    return 0;
}
