// Runs QgemulGrouped with an element-wise chain through include/QuBLAS_amd.h on the GPU (compiled by tests/test_gpu_grouped_ep.py with
// clang++ -std=c++23, linked against qublas_amd/libqugemm.so): three layers of different dim<>, each with its OWN scale
// (PerMember(s0, s1, s2)) and its own bias tensor (std::tie(Bias0, Bias1, Bias2)), then one offset for all.  Prints every D; the
// test recomputes every member with the oracle from the same inputs.
#include "QuBLAS_amd.h"

#include <cstdio>

using namespace QuBLAS_amd;

template <class T>
void fill(T& t, unsigned long long mul, unsigned long long add, long long mod, long long off)
{
    for (size_t i = 0; i < t.data.size(); ++i) t[i].fill(int64_t((i * mul + add) % (unsigned long long)mod) - off);
}
template <class T>
void print(const char* name, const T& t, bool last)
{
    std::printf("\"%s\":[", name);
    for (size_t e = 0; e < t.data.size(); ++e) std::printf("%s%lld", e ? "," : "", (long long)t.data[e].data);
    std::printf("]%s", last ? "" : ",");
}

int main()
{
    try {
        using e88 = Qu<intBits<8>, fracBits<8>, isSigned<true>, QuMode<TRN::TCPL>, OfMode<SAT::ZERO>>;
        using ct = Qu<intBits<7>, fracBits<8>>;
        using t1 = Qu<intBits<20>, fracBits<8>>;
        using bt = Qu<intBits<10>, fracBits<6>>;
        using st = Qu<intBits<3>, fracBits<4>>;
        using dt = Qu<intBits<12>, fracBits<6>, QuMode<RND::CONV>, OfMode<SAT::TCPL>>;
        Qu<dim<65, 40>, e88> A0;
        Qu<dim<40, 33>, e88> B0;
        Qu<dim<3, 100>, e88> A1;
        Qu<dim<100, 130>, e88> B1;
        Qu<dim<64, 7>, e88> A2;
        Qu<dim<7, 64>, e88> B2;
        Qu<dim<65, 33>, bt> Bias0;
        Qu<dim<3, 130>, bt> Bias1;
        Qu<dim<64, 64>, bt> Bias2;
        Qu<dim<65, 33>, dt> D0;
        Qu<dim<3, 130>, dt> D1;
        Qu<dim<64, 64>, dt> D2;
        fill(A0, 2654435761ull, 0, 128, 64);
        fill(B0, 40503ull, 7, 128, 64);
        fill(A1, 2246822519ull, 3, 128, 64);
        fill(B1, 3266489917ull, 11, 128, 64);
        fill(A2, 668265263ull, 5, 128, 64);
        fill(B2, 374761393ull, 13, 128, 64);
        fill(Bias0, 97ull, 0, 512, 256);
        fill(Bias1, 131ull, 5, 512, 256);
        fill(Bias2, 193ull, 9, 512, 256);
        st s0, s1, s2, off;
        s0.fill(13);
        s1.fill(-7);
        s2.fill(29);
        off.fill(5);
        QgemulGrouped<QgemulMulArgs<intBits<17>, fracBits<16>>, QgemulAddArgs<Qu<intBits<29>, fracBits<16>>>, QgemulResult<ct>>(
            std::tie(D0, D1, D2), std::tie(A0, A1, A2), std::tie(B0, B1, B2), ThenMul<t1, intBits<20>, fracBits<8>>(PerMember(s0, s1, s2)),
            ThenAdd<t1>(std::tie(Bias0, Bias1, Bias2)), ThenSub<void>(off));
        std::printf("{\"name\":\"per_member_scale_tied_bias\",\"scales\":[13,-7,29],\"offset\":5,");
        print("D0", D0, false);
        print("D1", D1, false);
        print("D2", D2, true);
        std::printf("}\n");
        QgemulRelease();
    } catch (const std::exception& e) {
        std::printf("{\"error\":\"%s\"}\n", e.what());
        return 3;
    }
    return 0;
}
