// The chains of amd_header_approx_probe.cpp on the REFERENCE header's own types (its ANUS::Segment included) through
// include/qgemul_reference_binding.hpp; compiled by tests/test_approx_plan.py where the reference header is present.
#include "QuBLAS.h"
#include "qgemul_reference_binding.hpp"
#include "approx_probe_common.hpp"

template <class T>
constexpr T K(long long raw)
{
    T t;
    t.data.data = decltype(t.data.data)(raw);
    return t;
}

int main()
{
    using FA = Qu<intBits<4>, fracBits<10>, QuMode<RND::CONV>, OfMode<SAT::TCPL>>;
    using FB = Qu<intBits<3>, fracBits<9>, QuMode<TRN::TCPL>, OfMode<SAT::ZERO>>;
    using FC = Qu<intBits<2>, fracBits<8>, QuMode<RND::ZERO>, OfMode<WRP::TCPL>>;
    using ct = Qu<intBits<15>, fracBits<8>>;
    using x78 = Qu<intBits<7>, fracBits<8>>;
    using s34 = Qu<intBits<3>, fracBits<4>>;
    using q44 = Qu<intBits<4>, fracBits<4>>;
    using dt = Qu<intBits<9>, fracBits<3>, QuMode<RND::NEG_INF>, OfMode<SAT::SMGN>>;
    using Seg0 = ANUS::Segment<-2.0, K<FA>(-1234)>;
    using Seg1 = ANUS::Segment<0.3, K<FB>(700), K<FC>(-300), K<FA>(515)>;
    using Seg2 = ANUS::Segment<1e30, K<FB>(-2047), K<FA>(9000)>;
    constexpr size_t M = 4, N = 3;
    Qu<dim<M, N>, dt> D;
    Qu<dim<M, N>, s34> T;
    Qu<dim<M, N>, x78> Dx;
    s34 s;
    {
        auto a = ThenMul<x78, intBits<24>, fracBits<8>>(s);
        auto b = ThenApprox<q44, Seg0, Seg1, Seg2>();
        auto c = ThenMul<>(T);
        print_chain("scale_approx_mul", Qgemul_lower_epilogue<QgemulResult<ct>>(D, a, b, c), Qgemul_lower_approx(a, b, c));
    }
    {
        auto a = ThenApprox<void, Seg1>();
        print_chain("approx_alone", Qgemul_lower_epilogue<QgemulResult<x78>>(Dx, a), Qgemul_lower_approx(a));
    }
    return 0;
}
