// ref_cases_ring.cpp — generator of tests/golden/ref_ring_0.jsonl.gz: GEMMs of the reference (its own header, through
// oracle/ref_driver.hpp) whose product and every tree level WRAP into one signed format: plain C integers of 8 / 12 / 16 / 24 / 32
// bits with default tags (each: 33x17x3 and a transposed-A 9x7x37 on the edge distribution, 8x8x1000 on full-range operands),
// saturating 16-bit operands into an int16 ring with a saturating 8-bit C, and int16 operands into a Qu<13,2> ring (the product
// enters by a left shift of 2) with C Qu<20,4>.  The records are data: formats, seeds, the reference's raw results.
// Build and run (the recipe of oracle/Makefile's _ref/% rule; REF_INC = the reference's include directory):
//     clang++ -std=c++23 -O2 -w -I$(REF_INC) -Ioracle tests/golden_src/ref_cases_ring.cpp -o oracle/_ref/ref_cases_ring
//     oracle/_ref/ref_cases_ring | gzip -9n > tests/golden/ref_ring_0.jsonl.gz
#include "ref_driver.hpp"
using namespace refdrv;
using i8  = Qu<intBits<7>,  fracBits<0>, isSigned<true>, QuMode<TRN::TCPL>, OfMode<WRP::TCPL>>;
using i12 = Qu<intBits<11>, fracBits<0>, isSigned<true>, QuMode<TRN::TCPL>, OfMode<WRP::TCPL>>;
using i16 = Qu<intBits<15>, fracBits<0>, isSigned<true>, QuMode<TRN::TCPL>, OfMode<WRP::TCPL>>;
using i24 = Qu<intBits<23>, fracBits<0>, isSigned<true>, QuMode<TRN::TCPL>, OfMode<WRP::TCPL>>;
using i32 = Qu<intBits<31>, fracBits<0>, isSigned<true>, QuMode<TRN::TCPL>, OfMode<WRP::TCPL>>;
using s16 = Qu<intBits<15>, fracBits<0>>;
using r132 = Qu<intBits<13>, fracBits<2>, isSigned<true>, QuMode<TRN::TCPL>, OfMode<WRP::TCPL>>;
static Inputs syn(int dist, uint64_t sa = 1, uint64_t sb = 2) { Inputs in; in.dist = dist; in.seedA = sa; in.seedB = sb; return in; }
template <class E> static void trio(const char* n, FILE* out)
{
    std::string s(n);
    run_case<E, E, E, TypeList<>, TypeList<>, false, 33, 17, 3>((s + "_ring_33x17xK3_edges").c_str(), syn(2, 21, 22), out);
    run_case<E, E, E, TypeList<>, TypeList<>, true, 9, 7, 37>((s + "_ring_9x7xK37_tn_edges").c_str(), syn(2, 23, 24), out);
    run_case<E, E, E, TypeList<>, TypeList<>, false, 8, 8, 1000>((s + "_ring_8x8x1000_full").c_str(), syn(0), out);
}
int main()
{
    FILE* out = stdout;
    trio<i8>("i8", out); trio<i12>("i12", out); trio<i16>("i16", out); trio<i24>("i24", out); trio<i32>("i32", out);
    run_case<s16, s16, Qu<intBits<7>, fracBits<0>>, TypeList<i16>, TypeList<i16>, false, 9, 7, 37>("s16_into_i16_ring_satC_9x7xK37_edges", syn(2, 25, 26), out);
    run_case<i16, i16, Qu<intBits<20>, fracBits<4>>, TypeList<r132>, TypeList<r132>, false, 9, 7, 37>("i16_lshift2_ring_9x7xK37_edges", syn(2, 27, 28), out);
    return 0;
}
