// Runs Qgemul with a scale, a bias and a ThenApprox stage (an 8-segment degree-3 fit of the logistic function, one format per Horner
// level) through include/QuBLAS_amd.h on the GPU (compiled by tests/test_gpu_approx.py with clang++ -std=c++23, linked against
// qublas_amd/libqugemm.so).  Prints D; the test recomputes it with the oracle and the restatement from the same raw inputs.
#include "QuBLAS_amd.h"

#include <cstdio>

using namespace QuBLAS_amd;

using L0 = Qu<intBits<1>, fracBits<14>, QuMode<RND::CONV>, OfMode<SAT::TCPL>>;
using L1 = Qu<intBits<1>, fracBits<13>, QuMode<RND::POS_INF>, OfMode<SAT::TCPL>>;
using L2 = Qu<intBits<0>, fracBits<14>>;
using L3 = Qu<intBits<0>, fracBits<15>>;
template <double BP, long long a0, long long a1, long long a2, long long a3>
using Sig = ANUS::Segment<BP, L0::from_raw(a0), L1::from_raw(a1), L2::from_raw(a2), L3::from_raw(a3)>;

int main()
{
    try {
        using e88 = Qu<intBits<8>, fracBits<8>, isSigned<true>, QuMode<TRN::TCPL>, OfMode<SAT::ZERO>>;
        using ct = Qu<intBits<15>, fracBits<8>>;
        using t1 = Qu<intBits<24>, fracBits<8>>;
        using x312 = Qu<intBits<3>, fracBits<12>>;
        using bt = Qu<intBits<10>, fracBits<6>>;
        using st = Qu<intBits<3>, fracBits<4>>;
        using dt = Qu<intBits<1>, fracBits<10>, QuMode<RND::CONV>, OfMode<SAT::TCPL>>;
        constexpr size_t M = 24, N = 10, K = 40;
        Qu<dim<M, K>, e88> A;
        Qu<dim<K, N>, e88> B;
        Qu<dim<M, N>, bt> Bias;
        Qu<dim<M, N>, dt> D;
        for (size_t i = 0; i < M * K; ++i) A[i].fill(int64_t((i * 2654435761ull) % 128) - 64);
        for (size_t i = 0; i < K * N; ++i) B[i].fill(int64_t((i * 40503ull + 7) % 128) - 64);
        for (size_t i = 0; i < M * N; ++i) Bias[i].fill(int64_t((i * 97ull) % 512) - 256);
        st s;
        s.fill(13);
        Qgemul<QgemulMulArgs<intBits<17>, fracBits<16>>, QgemulAddArgs<Qu<intBits<29>, fracBits<16>>>, QgemulResult<ct>>(
            D, A, B, ThenMul<t1, intBits<24>, fracBits<8>>(s), ThenAdd<x312>(Bias),
            ThenApprox<void, Sig<-4.0, 2976, 616, 173, 16>, Sig<-2.0, 8506, 2606, 1145, 178>, Sig<-1.0, 8505, 2499, 937, 77>, Sig<0.0, 8193, 2056, 69, -516>,
                       Sig<1.0, 8191, 2056, -69, -516>, Sig<2.0, 7879, 2499, -937, 77>, Sig<4.0, 7878, 2606, -1145, 178>, Sig<8.0, 13408, 616, -173, 16>>());
        std::printf("{\"name\":\"scale_bias_sigmoid\",\"M\":%zu,\"N\":%zu,\"K\":%zu,\"D\":[", M, N, K);
        for (size_t e = 0; e < D.data.size(); ++e) std::printf("%s%lld", e ? "," : "", (long long)D.data[e].data);
        std::printf("]}\n");
    } catch (const std::exception& e) {
        std::printf("{\"error\":\"%s\"}\n", e.what());
        return 3;
    }
    return 0;
}
