// ref_cases_real.cpp — TEST INFRASTRUCTURE: real-valued golden GEMM cases evaluated with the
// reference header's own Qmul / Qreduce / converting constructor (see ref_driver.hpp).
// Usage: ref_cases_real <part> > out.jsonl   (part selects a slice so the slices build in parallel)
#include "ref_driver.hpp"

#include <cstdlib>

using namespace refdrv;

// element types of the BASELINE.json configurations
using e88z = Qu<intBits<8>, fracBits<8>, isSigned<true>, QuMode<TRN::TCPL>, OfMode<SAT::ZERO>>; // c1, c3
using e43 = Qu<intBits<4>, fracBits<3>>;                                                        // c2, c4
using u44 = Qu<intBits<4>, fracBits<4>, isSigned<false>>;
using n63 = Qu<intBits<6>, fracBits<-3>>;
using w16 = Qu<intBits<16>, fracBits<3>>; // wide C so that parity is not hidden by saturation

// class-L tags of SURVEY.md §8-d
using L2mul = TypeList<intBits<9>, fracBits<6>>;
using L2add = TypeList<Qu<intBits<19>, fracBits<6>>>;
using L4add = TypeList<Qu<intBits<21>, fracBits<6>>>;
using L3mul = TypeList<intBits<17>, fracBits<16>>;
using L3add = TypeList<Qu<intBits<29>, fracBits<16>>>;

static Inputs one_to_sixteen()
{
    Inputs in;
    in.synthetic = false;
    for (int v = 1; v <= 16; ++v) { in.A.push_back(v * 256); in.B.push_back(v * 256); }
    return in;
}
static Inputs syn(int dist, uint64_t sa = 1, uint64_t sb = 2)
{
    Inputs in;
    in.dist = dist; in.seedA = sa; in.seedB = sb;
    return in;
}

// dist 2 (edge-heavy operands, oracle/qoracle.c: qo_edges) for the step forms of qublas_amd/csrc/qg_forms.h: each form once with
// K <= 3 (the product step alone, one node) and once with an odd K, whose leftover leaves take the vector overload's
// saturate-then-return path (QuBLAS.h:4977-4980)
static Inputs edges(uint64_t sa = 21, uint64_t sb = 22) { return syn(2, sa, sb); }

template <class EA, class EB, class EC, class Mul, class Add, size_t KS, size_t KL, bool TL = false>
static void form_pair(const char* name, FILE* out)
{
    std::string a = std::string(name) + "_33x17xK" + std::to_string(KS) + "_edges";
    std::string b = std::string(name) + "_9x7xK" + std::to_string(KL) + (TL ? "_tn" : "") + "_edges";
    run_case<EA, EB, EC, Mul, Add, false, 33, 17, KS>(a.c_str(), edges(), out);
    run_case<EA, EB, EC, Mul, Add, TL, 9, 7, KL>(b.c_str(), edges(23, 24), out);
}

// every QuMode x OfMode on C (the GEMM epilogue = converting constructor)
template <class Q, class O>
using c43 = Qu<intBits<4>, fracBits<3>, QuMode<Q>, OfMode<O>>;

template <class O>
static void epilogue_row(const char* oname, FILE* out)
{
    auto nm = [&](const char* q) { static std::string s; s = std::string("epi_e43_L_8x8x64_") + q + "_" + oname; return s.c_str(); };
    run_case<e43, e43, c43<RND::POS_INF, O>, L2mul, L2add, false, 8, 8, 64>(nm("POS_INF"), syn(0), out);
    run_case<e43, e43, c43<RND::NEG_INF, O>, L2mul, L2add, false, 8, 8, 64>(nm("NEG_INF"), syn(0), out);
    run_case<e43, e43, c43<RND::ZERO, O>, L2mul, L2add, false, 8, 8, 64>(nm("ZERO"), syn(0), out);
    run_case<e43, e43, c43<RND::INF, O>, L2mul, L2add, false, 8, 8, 64>(nm("INF"), syn(0), out);
    run_case<e43, e43, c43<RND::CONV, O>, L2mul, L2add, false, 8, 8, 64>(nm("CONV"), syn(0), out);
    run_case<e43, e43, c43<TRN::TCPL, O>, L2mul, L2add, false, 8, 8, 64>(nm("TCPL"), syn(0), out);
    run_case<e43, e43, c43<TRN::SMGN, O>, L2mul, L2add, false, 8, 8, 64>(nm("SMGN"), syn(0), out);
    // the same with small inputs so that results are not all saturated
    run_case<e43, e43, c43<RND::CONV, O>, L2mul, L2add, false, 8, 8, 64>(nm("CONV_small"), syn(1), out);
    run_case<e43, e43, c43<TRN::SMGN, O>, L2mul, L2add, false, 8, 8, 64>(nm("SMGN_small"), syn(1), out);
}

int main(int argc, char** argv)
{
    int part = argc > 1 ? std::atoi(argv[1]) : 0;
    FILE* out = stdout;
    switch (part) {
    case 0: // configuration 1 (README example shapes) and its class-L sibling
        run_case<e88z, e88z, e88z, TypeList<e88z>, TypeList<e88z>, false, 4, 4, 4>("c1_nn_classT", one_to_sixteen(), out);
        run_case<e88z, e88z, e88z, TypeList<e88z>, TypeList<e88z>, true, 4, 4, 4>("c1_tn_classT", one_to_sixteen(), out);
        run_case<e88z, e88z, e88z, TypeList<>, TypeList<>, false, 4, 4, 4>("c1_nn_default", one_to_sixteen(), out);
        run_case<e88z, e88z, e88z, L3mul, L3add, false, 4, 4, 4>("c1_nn_classL", one_to_sixteen(), out);
        run_case<e88z, e88z, e88z, L3mul, L3add, true, 4, 4, 4>("c1_tn_classL", one_to_sixteen(), out);
        run_case<e88z, e88z, e88z, TypeList<>, TypeList<>, false, 16, 16, 64>("e88z_default_16x16x64_full", syn(0), out);
        run_case<e88z, e88z, e88z, TypeList<>, TypeList<>, true, 16, 16, 64>("e88z_default_tn_16x16x64_small", syn(1), out);
        run_case<e88z, e88z, e88z, L3mul, L3add, false, 16, 16, 64>("e88z_L_16x16x64_full", syn(0), out);
        run_case<e88z, e88z, Qu<intBits<20>, fracBits<10>, QuMode<RND::CONV>, OfMode<SAT::SMGN>>, L3mul, L3add, true, 16, 16, 64>(
            "e88z_L_tn_16x16x64_wideC", syn(0), out);
        break;
    case 1: // configuration 2 formats, tree and linear, ragged shape
        run_case<e43, e43, e43, TypeList<>, TypeList<>, false, 33, 17, 128>("e43_default_33x17x128_full", syn(0), out);
        run_case<e43, e43, w16, TypeList<>, TypeList<>, false, 33, 17, 128>("e43_default_33x17x128_small_wideC", syn(1), out);
        run_case<e43, e43, w16, L2mul, L2add, false, 33, 17, 128>("e43_L_33x17x128_full_wideC", syn(0), out);
        run_case<e43, e43, e43, L2mul, L2add, true, 33, 17, 128>("e43_L_tn_33x17x128_full", syn(0), out);
        run_case<e43, e43, w16, L2mul, L2add, false, 16, 16, 512>("e43_L_16x16x512_full_wideC", syn(0), out);
        break;
    case 2: // epilogue modes (SAT::TCPL, SAT::ZERO)
        epilogue_row<SAT::TCPL>("SAT_TCPL", out);
        epilogue_row<SAT::ZERO>("SAT_ZERO", out);
        break;
    case 3: // epilogue modes (SAT::SMGN, WRP::TCPL)
        epilogue_row<SAT::SMGN>("SAT_SMGN", out);
        epilogue_row<WRP::TCPL>("WRP_TCPL", out);
        break;
    case 4: // long reductions, blocked 512-leaf subtrees
        run_case<e43, e43, w16, L2mul, L2add, false, 8, 8, 1024>("e43_L_8x8x1024_full_wideC", syn(0), out);
        run_case<e43, e43, w16, TypeList<>, TypeList<>, false, 8, 8, 1024>("e43_default_8x8x1024_small_wideC", syn(1), out);
        run_case<e43, e43, e43, L2mul, L4add, true, 4, 4, 4096>("e43_L_tn_4x4x4096_full", syn(0), out);
        run_case<e88z, e88z, e88z, TypeList<>, TypeList<>, false, 4, 4, 4096>("e88z_default_4x4x4096_small", syn(1), out);
        run_case<e88z, e88z, e88z, L3mul, L3add, false, 4, 4, 4096>("e88z_L_4x4x4096_full", syn(0), out);
        run_case<e88z, e88z, Qu<intBits<24>, fracBits<8>>, L3mul, L3add, true, 4, 4, 4096>("e88z_L_tn_4x4x4096_full_wideC", syn(0), out);
        break;
    case 5: { // unsigned, negative fracBits, mixed operand formats, wrapping levels
        run_case<u44, u44, u44, TypeList<>, TypeList<>, false, 8, 8, 64>("u44_default_8x8x64_full", syn(0), out);
        run_case<u44, u44, Qu<intBits<14>, fracBits<4>, isSigned<false>>, TypeList<>, TypeList<>, false, 8, 8, 64>("u44_default_8x8x64_small_wideC", syn(1), out);
        run_case<u44, u44, Qu<intBits<14>, fracBits<8>, isSigned<false>>, TypeList<intBits<8>, fracBits<8>>, TypeList<Qu<intBits<14>, fracBits<8>, isSigned<false>>>, false, 8, 8,
                 64>("u44_L_8x8x64_full", syn(0), out);
        run_case<n63, n63, n63, TypeList<>, TypeList<>, false, 8, 8, 64>("n63_default_8x8x64_full", syn(0), out);
        run_case<n63, n63, Qu<intBits<16>, fracBits<-3>>, TypeList<FullPrec>, TypeList<Qu<intBits<20>, fracBits<-6>>>, true, 8, 8, 64>("n63_fullprec_tn_8x8x64_full", syn(0), out);
        run_case<e88z, e43, w16, TypeList<>, TypeList<>, false, 8, 8, 64>("mixed_e88z_e43_default_8x8x64_small", syn(1), out);
        run_case<e43, u44, w16, TypeList<>, TypeList<>, false, 8, 8, 64>("mixed_e43_u44_default_8x8x64_full", syn(0), out);
        using wl = Qu<intBits<5>, fracBits<3>, OfMode<WRP::TCPL>>;
        run_case<e43, e43, w16, TypeList<wl>, TypeList<wl>, false, 8, 8, 64>("e43_wrap_levels_8x8x64_full", syn(0), out);
        using ul = Qu<intBits<6>, fracBits<4>, isSigned<false>, OfMode<WRP::TCPL>>;
        run_case<e43, e43, w16, TypeList<ul>, TypeList<ul>, false, 8, 8, 64>("e43_unsigned_wrap_levels_8x8x64_full", syn(0), out);
        break;
    }
    case 6: { // per-level type lists with differing formats and modes; rounding products
        using t1 = Qu<intBits<6>, fracBits<5>, QuMode<RND::CONV>, OfMode<SAT::SMGN>>;
        using t2 = Qu<intBits<8>, fracBits<4>, QuMode<RND::ZERO>, OfMode<SAT::TCPL>>;
        using t3 = Qu<intBits<9>, fracBits<2>, QuMode<TRN::SMGN>, OfMode<SAT::ZERO>>;
        using pm = Qu<intBits<5>, fracBits<4>, QuMode<RND::INF>, OfMode<SAT::TCPL>>;
        run_case<e43, e43, w16, TypeList<pm>, TypeList<t1, t2, t3>, false, 8, 8, 64>("e43_levels3_8x8x64_full", syn(0), out);
        run_case<e43, e43, w16, TypeList<pm>, TypeList<t1, t2, t3>, true, 8, 8, 64>("e43_levels3_tn_8x8x64_small", syn(1), out);
        run_case<e43, e43, e43, TypeList<QuMode<RND::POS_INF>, fracBits<2>>, TypeList<t2, t1>, false, 8, 8, 16>("e43_levels2_8x8x16_full", syn(0), out);
        run_case<e88z, e88z, e88z, TypeList<QuMode<RND::NEG_INF>, OfMode<SAT::SMGN>, intBits<10>>, TypeList<Qu<intBits<12>, fracBits<6>, QuMode<RND::POS_INF>>>, false, 8, 8,
                 32>("e88z_rnd_levels1_8x8x32_small", syn(1), out);
        // README shapes: type1 / type2 list
        using type1 = Qu<isSigned<true>, intBits<6>, fracBits<3>, OfMode<SAT::ZERO>>;
        using type2 = Qu<intBits<6>, fracBits<-3>>;
        run_case<type1, type1, type1, TypeList<type1>, TypeList<type1, type2>, true, 4, 4, 4>("readme_list_tn_4x4x4", syn(1), out);
        run_case<type1, type1, type1, TypeList<type1>, TypeList<type1, type2>, false, 8, 8, 32>("readme_list_8x8x32_small", syn(1), out);
        break;
    }
    case 7: { // reduction lengths that are not powers of two follow the vector overload (QuBLAS.h:4977-4980)
        using t1 = Qu<intBits<6>, fracBits<5>, QuMode<RND::CONV>, OfMode<SAT::SMGN>>;
        using t2 = Qu<intBits<8>, fracBits<4>, QuMode<RND::ZERO>, OfMode<SAT::TCPL>>;
        run_case<e43, e43, w16, TypeList<>, TypeList<t1, t2>, false, 4, 4, 1>("e43_K1", syn(0), out);
        run_case<e43, e43, w16, TypeList<>, TypeList<t1, t2>, false, 4, 4, 2>("e43_K2", syn(0), out);
        run_case<e43, e43, w16, TypeList<>, TypeList<t1, t2>, false, 4, 4, 3>("e43_K3", syn(0), out);
        run_case<e43, e43, w16, TypeList<>, TypeList<t1, t2>, false, 4, 4, 5>("e43_K5", syn(0), out);
        run_case<e43, e43, w16, TypeList<>, TypeList<t1, t2>, false, 4, 4, 6>("e43_K6", syn(0), out);
        run_case<e43, e43, w16, TypeList<>, TypeList<t1, t2>, false, 4, 4, 7>("e43_K7", syn(0), out);
        run_case<e43, e43, w16, TypeList<>, TypeList<t1>, true, 4, 4, 100>("e43_K100_tn", syn(1), out);
        run_case<e43, e43, w16, TypeList<>, TypeList<>, false, 3, 5, 37>("e43_K37_default", syn(1), out);
        run_case<e43, e43, w16, L2mul, L2add, false, 4, 4, 1000>("e43_L_K1000", syn(0), out);
        run_case<e88z, e88z, e88z, TypeList<>, TypeList<t2, t1>, false, 2, 2, 1000>("e88z_K1000_levels2_small", syn(1), out);
        break;
    }
    case 8: {   // C with WRP::TCPL_SAT<N> (the stub: the root goes into C's storage word unclamped)
        using csat = Qu<intBits<4>, fracBits<3>, OfMode<WRP::TCPL_SAT<2>>>;
        using csat2 = Qu<intBits<6>, fracBits<2>, QuMode<RND::CONV>, OfMode<WRP::TCPL_SAT<1>>>;
        run_case<e43, e43, csat, L2mul, L2add, false, 8, 8, 64>("e43_L_8x8x64_tcplsatC", syn(0), out);
        run_case<e43, e43, csat2, TypeList<>, TypeList<w16>, true, 9, 7, 37>("e43_T_tn_9x7x37_tcplsatC", syn(0), out);
        run_case<e88z, e88z, Qu<intBits<8>, fracBits<8>, OfMode<WRP::TCPL_SAT<4>>>, L3mul, L3add, false, 6, 6, 256>("e88z_L_6x6x256_tcplsatC", syn(0), out);
        break;
    }
    case 9: { // 32-bit words: QTF_WORD (product shifts 31, 24), QTF_WORD_MAD (16), QTF_JWORD / QTF_JWORD_MAD (justified), QTF_WORD_WRAP
        using q031 = Qu<intBits<0>, fracBits<31>>;
        using q724 = Qu<intBits<7>, fracBits<24>>;
        using q1516 = Qu<intBits<15>, fracBits<16>>;
        using q128 = Qu<intBits<1>, fracBits<28>>;
        using q1112 = Qu<intBits<11>, fracBits<12>>;
        using q1416 = Qu<intBits<14>, fracBits<16>>;
        using w1516 = Qu<intBits<15>, fracBits<16>, QuMode<TRN::TCPL>, OfMode<WRP::TCPL>>;
        using d = TypeList<>;
        form_pair<q031, q031, q031, d, d, 3, 37>("word_q031", out);
        form_pair<q724, q724, q724, d, d, 1, 100, true>("word_q724", out);
        form_pair<q1516, q1516, q1516, d, d, 2, 37>("wordmad_q1516", out);
        form_pair<q128, q128, q128, d, d, 2, 37, true>("jword_q128", out);
        form_pair<q1112, q1112, q1112, d, d, 3, 37>("jword_q1112", out);
        form_pair<q1416, q1416, q1416, d, d, 1, 100, true>("jwordmad_q1416", out);
        form_pair<w1516, w1516, w1516, d, d, 2, 37>("wordwrap_q1516", out);
        // the generator's dist-2 values written out (tests/test_oracle_golden.py pins oracle/qoracle.c's restatement to them)
        run_case<q1516, q1516, q1516, d, d, false, 5, 3, 7>("wordmad_q1516_5x3x7_edges_explicit", explicit_synth<q1516, q1516>(5 * 7, 7 * 3, 25, 26, 2), out);
        break;
    }
    case 10: { // packed 16-bit nodes and products, unsigned forms, left-justified words, one format, compact records
        using q65 = Qu<intBits<6>, fracBits<5>>;
        using q92 = Qu<intBits<9>, fracBits<2>>;
        using q78 = Qu<intBits<7>, fracBits<8>>;
        using q78p = Qu<intBits<7>, fracBits<8>, QuMode<RND::POS_INF>, OfMode<SAT::TCPL>>;
        using u125 = Qu<intBits<12>, fracBits<5>, isSigned<false>>;
        using u80 = Qu<intBits<8>, fracBits<0>, isSigned<false>>;
        using u88 = Qu<intBits<8>, fracBits<8>, isSigned<false>>;
        using u54 = Qu<intBits<5>, fracBits<4>, isSigned<false>>;
        using u76 = Qu<intBits<7>, fracBits<6>, isSigned<false>>;
        using u92 = Qu<intBits<9>, fracBits<2>, isSigned<false>>;
        using e88 = Qu<intBits<8>, fracBits<8>>;
        using d = TypeList<>;
        form_pair<q65, q65, q92, TypeList<Qu<intBits<7>, fracBits<6>, QuMode<RND::NEG_INF>, OfMode<SAT::TCPL>>>, TypeList<Qu<intBits<7>, fracBits<6>>>, 2, 37>("pk16hyb_q65", out);
        form_pair<q78, q78, q78, d, d, 3, 37, true>("pk16hyb16_q78", out);
        form_pair<q78p, q78p, Qu<intBits<12>, fracBits<4>>, d, d, 1, 100>("pk16hyb16_q78_posinf", out);
        form_pair<u125, u125, u125, d, d, 1, 37>("lju_u125", out);
        form_pair<u80, u80, u80, d, d, 2, 100, true>("pk16u_u80", out);
        form_pair<u54, u54, u92, TypeList<Qu<intBits<7>, fracBits<4>, isSigned<false>, QuMode<RND::POS_INF>, OfMode<SAT::TCPL>>>, TypeList<Qu<intBits<7>, fracBits<4>, isSigned<false>>>, 3, 37>("pk16u_u54", out);
        form_pair<u76, u76, u92, TypeList<Qu<intBits<8>, fracBits<6>, isSigned<false>, QuMode<RND::NEG_INF>, OfMode<SAT::TCPL>>>, TypeList<Qu<intBits<8>, fracBits<6>, isSigned<false>>>, 3, 37>("pk16hybu_u76", out);
        form_pair<u88, u88, u88, d, d, 1, 37, true>("pk16hyb16u_u88", out);
        form_pair<e88, e88, e88, d, d, 2, 37>("lj_e88", out);
        form_pair<e43, e43, e43, d, d, 3, 37>("pk16_e43", out);
        form_pair<e88z, e88z, e88z, d, d, 2, 37>("onezero_e88z", out);
        using u86 = Qu<intBits<8>, fracBits<6>, isSigned<false>>;   // signed operands, unsigned product: not left-justified
        form_pair<e43, e43, u86, TypeList<u86>, TypeList<u86>, 2, 37>("onetcpl_e43_u86", out);
        using z126 = Qu<intBits<12>, fracBits<6>, QuMode<TRN::TCPL>, OfMode<SAT::ZERO>>;
        using z108 = Qu<intBits<10>, fracBits<8>, QuMode<TRN::TCPL>, OfMode<SAT::ZERO>>;
        form_pair<e88, e88, Qu<intBits<12>, fracBits<8>>, d, TypeList<Qu<intBits<12>, fracBits<8>>>, 2, 37>("recclamp_e88", out);   // (K = 1: no add level, one format: QTF_LJ)
        form_pair<e88z, e88z, z126, d, TypeList<z108, z126>, 3, 37, true>("recbiased_e88z", out);
        form_pair<e88, e88, Qu<intBits<12>, fracBits<8>>, TypeList<Qu<intBits<10>, fracBits<6>, QuMode<RND::CONV>>>, TypeList<Qu<intBits<12>, fracBits<8>, QuMode<RND::CONV>>>, 2, 37>(
            "reckinds_e88", out);
        run_case<u80, u80, u80, d, d, false, 5, 3, 3>("pk16u_u80_5x3x3_edges_explicit", explicit_synth<u80, u80>(5 * 3, 3 * 3, 27, 28, 2), out);
        break;
    }
    case 11: { // one column (N = 1): the one-column kernel's forms; the 64-bit fallbacks at the same edges
        using q1516 = Qu<intBits<15>, fracBits<16>>;
        using z1516 = Qu<intBits<15>, fracBits<16>, QuMode<TRN::TCPL>, OfMode<SAT::ZERO>>;
        using w1516 = Qu<intBits<15>, fracBits<16>, QuMode<TRN::TCPL>, OfMode<WRP::TCPL>>;
        using one = Qu<intBits<1>, fracBits<0>, isSigned<false>>;   // a 0/1 vector: the product is the element itself (QGF_WORD)
        using d = TypeList<>;
        run_case<q1516, one, q1516, TypeList<q1516>, d, false, 33, 1, 256>("gemvword_q1516_bit_33x1x256_edges", edges(), out);
        run_case<q1516, one, q1516, TypeList<q1516>, d, true, 9, 1, 257>("gemvword_q1516_bit_9x1x257_tn_edges", edges(23, 24), out);
        run_case<q1516, q1516, q1516, d, d, false, 33, 1, 256>("gemvwordrnd_q1516_33x1x256_edges", edges(), out);
        using p1516 = Qu<intBits<15>, fracBits<16>, QuMode<RND::POS_INF>, OfMode<SAT::TCPL>>;
        run_case<q1516, q1516, q1516, TypeList<p1516>, d, true, 9, 1, 257>("gemvwordrnd_q1516_posinf_9x1x257_tn_edges", edges(23, 24), out);
        using u86 = Qu<intBits<8>, fracBits<6>, isSigned<false>>;
        run_case<e88z, e88z, e88z, d, d, false, 33, 1, 3>("gemvonezero_e88z_33x1xK3_edges", edges(), out);
        run_case<e88z, e88z, e88z, d, d, false, 9, 1, 37>("gemvonezero_e88z_9x1xK37_edges", edges(23, 24), out);
        using q128 = Qu<intBits<1>, fracBits<28>>;
        run_case<q128, q128, q128, d, d, false, 33, 1, 2>("gemvonetcpl_q128_33x1xK2_edges", edges(), out);
        run_case<e43, e43, e43, d, d, true, 9, 1, 100>("gemvonetcpl_e43_9x1xK100_tn_edges", edges(23, 24), out);
        using e88 = Qu<intBits<8>, fracBits<8>>;
        using l108 = Qu<intBits<10>, fracBits<8>>;
        using l128 = Qu<intBits<12>, fracBits<8>>;
        run_case<e88, e88, l128, d, TypeList<l108, l128>, false, 33, 1, 2>("gemvrecclamp_e88_33x1xK2_edges", edges(), out);
        run_case<e88, e88, l128, d, TypeList<l108, l128>, false, 9, 1, 37>("gemvrecclamp_e88_9x1xK37_edges", edges(23, 24), out);
        using t1 = Qu<intBits<6>, fracBits<5>, QuMode<RND::CONV>, OfMode<SAT::SMGN>>;
        using t2 = Qu<intBits<8>, fracBits<4>, QuMode<RND::ZERO>, OfMode<SAT::TCPL>>;
        run_case<e43, e43, w16, d, TypeList<t1, t2>, false, 33, 1, 3>("gemvreckinds_e43_33x1xK3_edges", edges(), out);
        run_case<e43, e43, w16, d, TypeList<t1, t2>, true, 9, 1, 37>("gemvreckinds_e43_9x1xK37_tn_edges", edges(23, 24), out);
        // 64-bit fallbacks: SAT::ZERO words on the 64-bit tree kernel, wrapping words on the 64-bit one-column kernel
        form_pair<z1516, z1516, z1516, d, d, 3, 37>("treei64_q1516_zero", out);
        run_case<w1516, w1516, w1516, d, d, false, 33, 1, 2>("gemvi64_q1516_wrap_33x1xK2_edges", edges(), out);
        run_case<w1516, w1516, w1516, d, d, false, 9, 1, 37>("gemvi64_q1516_wrap_9x1xK37_edges", edges(23, 24), out);
        run_case<u86, u86, u86, d, d, false, 5, 1, 2>("gemvonetcpl_u86_5x1x2_edges_explicit", explicit_synth<u86, u86>(5 * 2, 2, 29, 30, 2), out);
        break;
    }
    case 12: { // linear plans at the edges: single limb, plain limbs, centred 1x1 / 2x2 / 3x3 limbs, narrow C (the epilogue rounds and
               // saturates); the composite plan's limb groups over a 65536-leaf row
        using q78 = Qu<intBits<7>, fracBits<8>>;
        using u80 = Qu<intBits<8>, fracBits<0>, isSigned<false>>;
        using q1112 = Qu<intBits<11>, fracBits<12>>;
        using e88 = Qu<intBits<8>, fracBits<8>>;
        form_pair<q78, q78, Qu<intBits<9>, fracBits<3>, QuMode<RND::CONV>, OfMode<SAT::SMGN>>, TypeList<intBits<15>, fracBits<16>>, TypeList<Qu<intBits<28>, fracBits<16>>>, 3, 100>(
            "centred2_q78", out);
        form_pair<u80, u80, Qu<intBits<12>, fracBits<-4>, isSigned<false>, QuMode<RND::CONV>, OfMode<SAT::SMGN>>, TypeList<intBits<16>, fracBits<0>, isSigned<false>>,
                  TypeList<Qu<intBits<28>, fracBits<0>, isSigned<false>>>, 2, 37, true>("centred1_u80", out);
        form_pair<q1112, q1112, Qu<intBits<20>, fracBits<8>, QuMode<RND::CONV>, OfMode<SAT::SMGN>>, TypeList<intBits<23>, fracBits<24>>, TypeList<Qu<intBits<35>, fracBits<24>>>, 1, 37>(
            "centred3_q1112", out);
        form_pair<e43, e43, Qu<intBits<8>, fracBits<2>, QuMode<RND::CONV>, OfMode<SAT::SMGN>>, L2mul, L2add, 3, 37>("single_e43", out);
        form_pair<e88z, e88z, Qu<intBits<10>, fracBits<4>, QuMode<RND::CONV>, OfMode<SAT::SMGN>>, L3mul, L3add, 2, 37, true>("plain_e88z", out);
        run_case<e88, e88, Qu<intBits<24>, fracBits<8>>, L3mul, TypeList<Qu<intBits<33>, fracBits<16>>>, false, 2, 2, 65536>("composite_e88_2x2x65536_edges", edges(), out);
        run_case<q78, q78, Qu<intBits<9>, fracBits<3>, QuMode<RND::CONV>, OfMode<SAT::SMGN>>, TypeList<intBits<15>, fracBits<16>>, TypeList<Qu<intBits<28>, fracBits<16>>>, false, 5, 3, 2>(
            "centred2_q78_5x3x2_edges_explicit", explicit_synth<q78, q78>(5 * 2, 2 * 3, 31, 32, 2), out);
        break;
    }
    default:
        return 2;
    }
    return 0;
}
