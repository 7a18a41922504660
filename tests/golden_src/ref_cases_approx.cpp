// ref_cases_approx.cpp — generator of tests/golden/ref_approx_0.jsonl.gz: the reference's own ANUS::Qapprox (its header, QuBLAS.h:4829-4897)
// evaluated on scalar inputs.  A record holds x's format, the segments (breakpoint as a C hex-float string, every coefficient's format and
// the raw value the reference holds for it, c.data.data), the inputs and the outputs, all as raw integers.  Coefficients are built from raw
// integers, never from doubles: Qu_s(double) with RND::CONV returns the format maximum for negative inputs (tests/test_from_double.py).
// Inputs per table: the format's edges, each threshold ceil(bp * 2^F) - 1 / 0 / + 1, and a pseudo-random sample of the rest.
// Build and run (the recipe of oracle/Makefile's _ref/% rule; REF_INC = the reference's include directory):
//     clang++ -std=c++23 -O1 -w -I$(REF_INC) -Ioracle tests/golden_src/ref_cases_approx.cpp -o oracle/_ref/ref_cases_approx
//     oracle/_ref/ref_cases_approx | gzip -9n > tests/golden/ref_approx_0.jsonl.gz
#include "ref_driver.hpp"

#include <algorithm>
#include <cmath>
#include <limits>
using namespace refdrv;

template <int I, int F, bool S = true, class Q = TRN::TCPL, class O = SAT::TCPL>
using Q_ = Qu<intBits<I>, fracBits<F>, isSigned<S>, QuMode<Q>, OfMode<O>>;
// a coefficient from its raw value
template <class T>
constexpr T K(long long raw)
{
    T t;
    t.data.data = decltype(t.data.data)(raw);
    return t;
}
constexpr double INF = std::numeric_limits<double>::infinity();

template <class S> struct seg_info;
template <double BP, auto... as>
struct seg_info<ANUS::Segment<BP, as...>> {
    static std::string json()
    {
        char b[64];
        std::snprintf(b, sizeof b, "%a", BP);
        std::string f, r;
        ((f += (f.empty() ? "" : ",") + fmt_json<decltype(as)>()), ...);
        ((r += (r.empty() ? "" : ",") + dec(raw_t(as.data.data))), ...);
        return std::string("{\"bp\":\"") + b + "\",\"f\":[" + f + "],\"a\":[" + r + "]}";
    }
    static double bp() { return BP; }
};

template <class X, class... Segs>
void run(const char* name, int nrand, FILE* out)
{
    constexpr int W = X::intB + X::fracB, F = X::fracB;
    const int64_t lo = X::isS ? -(int64_t(1) << W) : 0, hi = (int64_t(1) << W) - 1;
    std::vector<int64_t> xs = {lo, lo + 1, -1, 0, 1, hi - 1, hi};
    for (double bp : {seg_info<Segs>::bp()...}) {
        const double t = std::ceil(std::ldexp(bp, F));
        if (!(t >= double(lo) - 2 && t <= double(hi) + 2)) continue;
        for (int k = -1; k <= 1; ++k) xs.push_back(int64_t(t) + k);
    }
    for (int i = 0; i < nrand; ++i) xs.push_back(synth<X>(0xA990 + W, 0, uint64_t(i), 0));
    std::vector<int64_t> in;
    for (int64_t v : xs)
        if (v >= lo && v <= hi) in.push_back(v);
    std::sort(in.begin(), in.end());
    in.erase(std::unique(in.begin(), in.end()), in.end());
    std::string segs;
    ((segs += (segs.empty() ? "" : ",") + seg_info<Segs>::json()), ...);
    std::fprintf(out, "{\"name\":\"%s\",\"x\":%s,\"segments\":[%s],\"X\":[", name, fmt_json<X>().c_str(), segs.c_str());
    for (size_t i = 0; i < in.size(); ++i) std::fprintf(out, "%s%lld", i ? "," : "", (long long)in[i]);
    std::fprintf(out, "],\"Y\":[");
    for (size_t i = 0; i < in.size(); ++i) {
        X x;
        set_raw(x, in[i], 0);
        const X y = ANUS::Qapprox<Segs...>(x);
        int64_t re, im;
        get_raw(y, re, im);
        std::fprintf(out, "%s%lld", i ? "," : "", (long long)re);
    }
    std::fprintf(out, "]}\n");
}

using FA = Q_<4, 10, true, RND::CONV, SAT::TCPL>;
using FB = Q_<3, 9, true, TRN::TCPL, SAT::ZERO>;
using FC = Q_<2, 8, true, RND::ZERO, WRP::TCPL>;
using FD = Q_<5, 6, true, TRN::SMGN, SAT::SMGN>;
using X78 = Q_<7, 8>;
// uniform table: a degree-3 fit of the logistic function on [-8, 8), one format per Horner level
using L0 = Q_<1, 14, true, RND::CONV, SAT::TCPL>;
using L1 = Q_<1, 13, true, RND::POS_INF, SAT::TCPL>;
using L2 = Q_<0, 14>;
using L3 = Q_<0, 15>;
template <double BP, long long a0, long long a1, long long a2, long long a3>
using Sig = ANUS::Segment<BP, K<L0>(a0), K<L1>(a1), K<L2>(a2), K<L3>(a3)>;

int main()
{
    FILE* out = stdout;
    using namespace ANUS;
    // the three probe configurations
    run<X78, Segment<-2.0, K<FA>(-1234)>,
        Segment<0.3, K<FB>(700), K<FC>(-300), K<FA>(515)>,
        Segment<1.7, K<FD>(-77), K<FA>(9000), K<FB>(-2047), K<FC>(333)>,
        Segment<INF, K<FD>(-2047)>>("probe_four_segments_mixed_modes", 400, out);
    run<X78, Segment<-1.0, K<FA>(100), K<FA>(-3000)>, Segment<0.5, K<FB>(5), K<FC>(129)>, Segment<2.0, K<FD>(1000), K<FB>(-600), K<FB>(44)>,
        Segment<0.0, K<FC>(-1), K<FA>(16383)>>("probe_unsorted_breakpoints", 120, out);
    run<Q_<8, 4, false, RND::INF, SAT::ZERO>, Segment<10.0, K<FA>(321), K<FB>(-100)>, Segment<100.3, K<FD>(640), K<FA>(1023), K<FC>(-9)>,
        Segment<200.0, K<FB>(4095)>>("probe_unsigned_x_rnd_inf_sat_zero", 160, out);
    // uniform formats, 8 segments, degree 3
    run<Q_<3, 12>, Sig<-4.0, 2976, 616, 173, 16>, Sig<-2.0, 8506, 2606, 1145, 178>, Sig<-1.0, 8505, 2499, 937, 77>, Sig<0.0, 8193, 2056, 69, -516>,
        Sig<1.0, 8191, 2056, -69, -516>, Sig<2.0, 7879, 2499, -937, 77>, Sig<4.0, 7878, 2606, -1145, 178>, Sig<8.0, 13408, 616, -173, 16>>(
        "uniform_sigmoid_8x_degree3", 400, out);
    // a degree-7 segment next to a constant
    run<Q_<2, 10>, Segment<-0.75, K<FB>(-999)>,
        Segment<1e30, K<FA>(11), K<FB>(-2222), K<FA>(3333), K<FC>(-444), K<FD>(555), K<FA>(-6666), K<FB>(777), K<FC>(-88)>>("degree7_segment", 200, out);
    // one segment (what the plain four-stage chain can also express)
    run<Q_<5, 5>, Segment<0.0, K<Q_<6, 6, true, RND::CONV, SAT::TCPL>>(-1500), K<Q_<4, 7, true, TRN::TCPL, SAT::TCPL>>(900),
                          K<Q_<4, 7, true, TRN::TCPL, SAT::TCPL>>(-70)>>("one_segment_degree2", 150, out);
    // x with negative fracBits; breakpoints that are no multiples of 2^-F = 4
    run<Q_<12, -2>, Segment<-100.0, K<FD>(300)>, Segment<37.0, K<Q_<12, 0>>(1000), K<Q_<3, 4, true, RND::NEG_INF, SAT::TCPL>>(-19)>,
        Segment<1000.5, K<Q_<12, -2, true, RND::INF, SAT::SMGN>>(-200), K<Q_<1, 6>>(33), K<Q_<-2, 8>>(20)>,
        Segment<5000.0, K<Q_<10, 2, true, RND::CONV, WRP::TCPL>>(77), K<Q_<2, 4>>(-60)>>("negative_fracbits_x", 200, out);
    // x of 40 value bits: 64-bit arithmetic
    run<Q_<20, 20>, Segment<-1000.25, K<Q_<20, 20>>(123456789012LL)>,
        Segment<3.0000001, K<Q_<20, 20, true, RND::CONV, SAT::TCPL>>(-98765432101LL), K<Q_<3, 12>>(20000), K<Q_<3, 12>>(-31000)>,
        Segment<70000.5, K<Q_<18, 18, true, RND::ZERO, WRP::TCPL>>(5555555555LL), K<Q_<2, 13, true, TRN::SMGN, SAT::ZERO>>(-30001)>>(
        "x_of_40_value_bits", 300, out);
    // breakpoints outside x's range: above (the last segment takes everything from 0 on), below (only as the fallback)
    run<Q_<3, 4>, Segment<0.0, K<FA>(5), K<FB>(-6)>, Segment<1e30, K<FC>(7), K<FD>(8)>>("breakpoint_above_range", 60, out);
    run<Q_<3, 4>, Segment<0.0, K<FA>(5), K<FB>(-6)>, Segment<-1e30, K<FC>(7), K<FD>(8)>>("breakpoint_below_range", 60, out);
    return 0;
}
