// Runs QgemulBatched on complex 3-d tensors through include/QuBLAS_amd.h on the GPU with QgemulRunFlags() |= QG_OPT_BATCHED_STACKED
// (compiled by tests/test_gpu_batched_stacked.py with clang++ -std=c++23, linked against qublas_amd/libqugemm.so): a complex x complex
// batch and a real x complex batch of the linear class, each ONE block-diagonal launch plus one combine pass.  Prints the launch count the
// planner answers for the lowered descriptor under the flag and every C; raw operand values follow fixed formulas the test repeats.
#include "QuBLAS_amd.h"

#include <cstdio>

using namespace QuBLAS_amd;

using r63 = Qu<intBits<6>, fracBits<3>, isSigned<true>, QuMode<RND::POS_INF>, OfMode<SAT::TCPL>>;
using i63n = Qu<intBits<6>, fracBits<-3>, isSigned<true>, QuMode<RND::POS_INF>, OfMode<SAT::TCPL>>;
using c5 = Qcomplex<r63, i63n>;
using e66 = Qu<intBits<6>, fracBits<6>>;

template <class T>
static void fill_real(T& t)
{
    for (size_t e = 0; e < t.data.size(); ++e) t.data[e].data = int32_t((e * 2654435761ull) % 8192) - 4096;
}
template <class T>
static void fill_cplx(T& t)
{
    for (size_t e = 0; e < t.data.size(); ++e) {
        t.data[e].real.data = int32_t((e * 53 + 7) % 1024) - 512;
        t.data[e].imag.data = int32_t((e * 40503ull + 3) % 16) - 8;
    }
}
template <class T>
static void print_cplx(const char* name, int launches, const T& m)
{
    std::printf("{\"name\":\"%s\",\"launches\":%d,\"C\":[", name, launches);
    for (size_t e = 0; e < m.data.size(); ++e) std::printf("%s%lld,%lld", e ? "," : "", (long long)m.data[e].real.data, (long long)m.data[e].imag.data);
    std::printf("]}\n");
}
// what qgemul_plan_batched_launches will answer for this call under the run flags
template <typename... Tags, class TC, class TA, class TB>
static int launches_of(const TC& C, const TA& A, const TB& B)
{
    int64_t batch = 0, strides[3];
    const qgemul_desc d = QgemulBatched_lower<Tags...>(C, A, B, &batch, strides);
    return qgemul_classify_batched_launches(&d, batch, QgemulRunFlags());
}

int main()
{
    try {
        QgemulRunFlags() |= QG_OPT_BATCHED_STACKED;
        constexpr size_t M = 65, N = 40, K = 72, Bt = 5;
        {   // complex x complex, two limbs per part: every sub-product and tree level exact
            using Mul = QgemulMulArgs<BasicComplexMul<acT<Qu<intBits<14>, fracBits<6>>>, bdT<Qu<intBits<14>, fracBits<-6>>>, adT<Qu<intBits<14>, fracBits<0>>>,
                                                      bcT<Qu<intBits<14>, fracBits<0>>>, acbdT<Qu<intBits<15>, fracBits<6>>>, adbcT<Qu<intBits<15>, fracBits<0>>>>>;
            using Add = QgemulAddArgs<Qcomplex<Qu<intBits<30>, fracBits<6>>, Qu<intBits<30>, fracBits<0>>>>;
            Qu<dim<M, K, Bt>, c5> A;
            Qu<dim<K, N, Bt>, c5> B;
            Qu<dim<M, N, Bt>, Qcomplex<Qu<intBits<20>, fracBits<4>, isSigned<true>, QuMode<RND::POS_INF>>, Qu<intBits<20>, fracBits<0>>>> C;
            fill_cplx(A);
            fill_cplx(B);
            QgemulBatched<Mul, Add>(C, A, B);
            print_cplx("complex_x_complex", launches_of<Mul, Add>(C, A, B), C);
        }
        {   // real x complex under QgemulTransposedA, two limbs
            using Mul = QgemulMulArgs<realT<Qu<intBits<14>, fracBits<9>>>, imagT<Qu<intBits<14>, fracBits<3>>>>;
            using Add = QgemulAddArgs<Qcomplex<Qu<intBits<22>, fracBits<9>>, Qu<intBits<22>, fracBits<3>>>>;
            Qu<dim<K, M, Bt>, e66> A;
            Qu<dim<K, N, Bt>, c5> B;
            Qu<dim<M, N, Bt>, Qcomplex<Qu<intBits<22>, fracBits<6>>, Qu<intBits<22>, fracBits<0>>>> C;
            fill_real(A);
            fill_cplx(B);
            QgemulBatched<QgemulTransposedA<true>, Mul, Add>(C, A, B);
            print_cplx("real_x_complex_tn", launches_of<QgemulTransposedA<true>, Mul, Add>(C, A, B), C);
        }
        QgemulRelease();
    } catch (const std::exception& e) {
        std::printf("{\"error\":\"%s\"}\n", e.what());
        return 1;
    }
    return 0;
}
