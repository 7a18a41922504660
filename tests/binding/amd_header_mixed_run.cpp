// Runs Qgemul with one real and one complex operand through include/QuBLAS_amd.h on the GPU (compiled by tests/test_gpu_mixed.py with
// clang++ -std=c++23 and linked against qublas_amd/libqugemm.so): real coefficients x complex samples with default tags, and complex
// samples x real coefficients with realT / imagT tags under QgemulTransposedA.  Raw operand values follow fixed formulas the test repeats.
#include "QuBLAS_amd.h"

#include <cstdio>

using namespace QuBLAS_amd;

using e43 = Qu<intBits<4>, fracBits<3>>;
using r63 = Qu<intBits<6>, fracBits<3>, isSigned<true>, QuMode<RND::POS_INF>, OfMode<SAT::TCPL>>;
using i63n = Qu<intBits<6>, fracBits<-3>, isSigned<true>, QuMode<RND::POS_INF>, OfMode<SAT::TCPL>>;
using c5 = Qcomplex<r63, i63n>;

template <class T>
static void fill_real(T& t)
{
    for (size_t e = 0; e < t.data.size(); ++e) t.data[e].data = int32_t((e * 37 + 11) % 256) - 128;
}
template <class T>
static void fill_cplx(T& t)
{
    for (size_t e = 0; e < t.data.size(); ++e) {
        t.data[e].real.data = int32_t((e * 53 + 7) % 1024) - 512;
        t.data[e].imag.data = int32_t((e * 5 + 3) % 16) - 8;
    }
}
template <class T>
static void print_cplx(const char* name, const T& m)
{
    std::printf("{\"name\":\"%s\",\"C\":[", name);
    for (size_t e = 0; e < m.data.size(); ++e) std::printf("%s%lld,%lld", e ? "," : "", (long long)m.data[e].real.data, (long long)m.data[e].imag.data);
    std::printf("]}\n");
}

int main()
{
    try {
        constexpr size_t M = 9, N = 7, K = 37;
        {
            Qu<dim<M, K>, e43> A;
            Qu<dim<K, N>, c5> B;
            Qu<dim<M, N>, Qcomplex<Qu<intBits<14>, fracBits<3>>, Qu<intBits<14>, fracBits<3>>>> C;
            fill_real(A);
            fill_cplx(B);
            Qgemul<>(C, A, B);
            print_cplx("real_x_complex_default", C);
        }
        {
            Qu<dim<K, M>, c5> A;
            Qu<dim<K, N>, e43> B;
            Qu<dim<M, N>, Qcomplex<Qu<intBits<18>, fracBits<6>>, Qu<intBits<16>, fracBits<0>>>> C;
            fill_cplx(A);
            fill_real(B);
            Qgemul<QgemulTransposedA<true>, QgemulMulArgs<realT<Qu<intBits<12>, fracBits<6>>>, imagT<intBits<10>, fracBits<0>>>>(C, A, B);
            print_cplx("complex_x_real_tagged_tn", C);
        }
    } catch (const std::exception& e) {
        std::printf("{\"error\":\"%s\"}\n", e.what());
        return 1;
    }
    return 0;
}
