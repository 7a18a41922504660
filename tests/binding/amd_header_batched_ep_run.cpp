// Runs QgemulBatched with an element-wise chain through include/QuBLAS_amd.h on the GPU (compiled by tests/test_gpu_batched_ep.py with
// clang++ -std=c++23, linked against qublas_amd/libqugemm.so): a scalar scale, ONE shared bias for every member (dim<M, N>), one
// residual tensor per member (dim<M, N, Bt>) and a ThenApprox stage (the 8-segment degree-3 fit of the logistic function of
// amd_header_approx_run.cpp).  Prints D; the test recomputes every member with the oracle and the restatement from the same inputs.
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
        constexpr size_t M = 65, N = 33, K = 40, Bt = 5;
        Qu<dim<M, K, Bt>, e88> A;
        Qu<dim<K, N, Bt>, e88> B;
        Qu<dim<M, N>, bt> Bias;          // shared
        Qu<dim<M, N, Bt>, bt> Res;       // one per member
        Qu<dim<M, N, Bt>, dt> D;
        for (size_t i = 0; i < A.data.size(); ++i) A[i].fill(int64_t((i * 2654435761ull) % 128) - 64);
        for (size_t i = 0; i < B.data.size(); ++i) B[i].fill(int64_t((i * 40503ull + 7) % 128) - 64);
        for (size_t i = 0; i < Bias.data.size(); ++i) Bias[i].fill(int64_t((i * 97ull) % 512) - 256);
        for (size_t i = 0; i < Res.data.size(); ++i) Res[i].fill(int64_t((i * 131ull + 5) % 1024) - 512);
        st s;
        s.fill(13);
        QgemulBatched<QgemulMulArgs<intBits<17>, fracBits<16>>, QgemulAddArgs<Qu<intBits<29>, fracBits<16>>>, QgemulResult<ct>>(
            D, A, B, ThenMul<t1, intBits<24>, fracBits<8>>(s), ThenAdd<t1>(Bias), ThenSub<x312>(Res),
            ThenApprox<void, Sig<-4.0, 2976, 616, 173, 16>, Sig<-2.0, 8506, 2606, 1145, 178>, Sig<-1.0, 8505, 2499, 937, 77>, Sig<0.0, 8193, 2056, 69, -516>,
                       Sig<1.0, 8191, 2056, -69, -516>, Sig<2.0, 7879, 2499, -937, 77>, Sig<4.0, 7878, 2606, -1145, 178>, Sig<8.0, 13408, 616, -173, 16>>());
        std::printf("{\"name\":\"scale_bias_residual_sigmoid\",\"M\":%zu,\"N\":%zu,\"K\":%zu,\"batch\":%zu,\"D\":[", M, N, K, Bt);
        for (size_t e = 0; e < D.data.size(); ++e) std::printf("%s%lld", e ? "," : "", (long long)D.data[e].data);
        std::printf("]}\n");
        QgemulRelease();
    } catch (const std::exception& e) {
        std::printf("{\"error\":\"%s\"}\n", e.what());
        return 3;
    }
    return 0;
}
