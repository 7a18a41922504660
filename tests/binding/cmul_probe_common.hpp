// shared by the two complex x complex ThenMul lowering probes (tests/test_cmul_lowering.py): the chain's C-ABI form as hex bytes, one
// JSON line; CHAINS(print) lowers the same chains through whichever header the including probe has brought in
#pragma once
#include <cstdio>

#include "qgemul.h"

template <class T>
static void hex_bytes(const T& v)
{
    const unsigned char* p = reinterpret_cast<const unsigned char*>(&v);
    std::printf("\"");
    for (size_t i = 0; i < sizeof(T); ++i) std::printf("%02x", p[i]);
    std::printf("\"");
}

template <class Records>
static void print_chain(const char* name, const qgemul_epilogue_cplx& ep, const Records& cx)
{
    const qgemul_cmul* p[QG_MAX_EW];
    cx.pointers(p);
    std::printf("{\"name\":\"%s\",\"ep\":", name);
    hex_bytes(ep);
    std::printf(",\"cx\":[");
    for (int k = 0; k < QG_MAX_EW; ++k) {
        if (k) std::printf(",");
        if (p[k]) hex_bytes(*p[k]);
        else std::printf("null");
    }
    std::printf("]}\n");
}

// the chains, spelled once for both headers (every name below is declared by both)
static void lower_and_print_chains()
{
    using x64 = Qu<intBits<6>, fracBits<4>>;
    using e35 = Qu<intBits<3>, fracBits<5>>;
    using r63 = Qu<intBits<6>, fracBits<3>, QuMode<RND::POS_INF>, OfMode<SAT::TCPL>>;
    using r6n3 = Qu<intBits<6>, fracBits<-3>, QuMode<RND::POS_INF>, OfMode<SAT::TCPL>>;
    using r54 = Qu<intBits<5>, fracBits<4>>;
    using r32 = Qu<intBits<3>, fracBits<2>>;
    using r206 = Qu<intBits<20>, fracBits<6>>;
    using r73w = Qu<intBits<7>, fracBits<3>, QuMode<RND::ZERO>, OfMode<WRP::TCPL>>;
    using r91s = Qu<intBits<9>, fracBits<1>, QuMode<TRN::SMGN>, OfMode<SAT::SMGN>>;
    using cx = Qcomplex<x64, x64>;
    using ce = Qcomplex<e35, e35>;
    using c5 = Qcomplex<r63, r6n3>;
    using cb = Qcomplex<r54, r32>;
    using cw = Qcomplex<r206, r206>;
    using cq = Qcomplex<r73w, r91s>;
    constexpr size_t M = 4, N = 3;
    Qu<dim<M, N>, cq> D;
    Qu<dim<M, N>, cb> Bias;
    Qu<dim<M, N>, ce> E;
    r32 s;
    cb z;
    {
        // complex bias, a Basic multiplication with two tagged sub-operations and loose tags for the rest, a real scale
        auto a = ThenAdd<cw>(Bias);
        auto b = ThenMul<c5, BasicComplexMul<acT<intBits<8>, fracBits<3>, QuMode<RND::POS_INF>>, adbcT<intBits<5>, fracBits<1>, QuMode<TRN::SMGN>, OfMode<WRP::TCPL>>,
                                             fracBits<2>, QuMode<RND::CONV>>>(E);
        auto c = ThenRmul<void, imagT<r91s>>(s);
        print_chain("basic_chain", Qgemul_lower_epilogue_cplx<QgemulResult<cx>>(D, a, b, c), Qgemul_lower_cmul<QgemulResult<cx>>(D, a, b, c));
    }
    {
        // TF with the operand first, a complex scalar, all the quirks in play (baT given, badT / cdbT distinct), parts of different formats
        auto a = ThenRmul<void, TFComplexMul<baT<intBits<2>, fracBits<0>, OfMode<SAT::ZERO>>, abcT<intBits<8>, fracBits<3>, QuMode<RND::CONV>>,
                                             cdbT<intBits<7>, fracBits<2>, QuMode<RND::NEG_INF>, OfMode<SAT::SMGN>>,
                                             badT<intBits<6>, fracBits<4>, QuMode<RND::POS_INF>, OfMode<SAT::ZERO>>, BCT<intBits<6>, fracBits<3>, OfMode<WRP::TCPL>>>>(z);
        auto b = ThenMul<>(E);   // no tags: BasicComplexMul<>
        print_chain("tf_rmul_scalar_then_plain", Qgemul_lower_epilogue_cplx<QgemulResult<c5>>(D, a, b), Qgemul_lower_cmul<QgemulResult<c5>>(D, a, b));
    }
}
