// Runs QgemulBatched on 3-d tensors of the TREE class through include/QuBLAS_amd.h on the GPU, first without and then with
// QgemulRunFlags() |= QG_OPT_BATCHED_TREE (compiled by tests/test_gpu_batched_tree.py with clang++ -std=c++23, linked against
// qublas_amd/libqugemm.so): a default-tag int<8,8> batch and a TFComplexMul batch of configuration 5's complex type.  Prints, per run,
// the launch count the planner answers for the lowered descriptor under the run flags and every C; raw operand values follow fixed
// formulas the test repeats.
#include "QuBLAS_amd.h"

#include <cstdio>

using namespace QuBLAS_amd;

using e88 = Qu<intBits<8>, fracBits<8>>;
using r63 = Qu<intBits<6>, fracBits<3>, isSigned<true>, QuMode<RND::POS_INF>, OfMode<SAT::TCPL>>;
using i63n = Qu<intBits<6>, fracBits<-3>, isSigned<true>, QuMode<RND::POS_INF>, OfMode<SAT::TCPL>>;
using c5 = Qcomplex<r63, i63n>;

template <class T>
static void fill_real(T& t, unsigned long long mul, unsigned long long add)
{
    for (size_t e = 0; e < t.data.size(); ++e) t.data[e].data = int32_t((e * mul + add) % 8192) - 4096;
}
template <class T>
static void fill_cplx(T& t, unsigned long long mul)
{
    for (size_t e = 0; e < t.data.size(); ++e) {
        t.data[e].real.data = int32_t((e * mul + 7) % 1024) - 512;
        t.data[e].imag.data = int32_t((e * 40503ull + 3) % 16) - 8;
    }
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
        constexpr size_t M = 70, N = 41, K = 40, Bt = 5;
        for (int flagged = 0; flagged < 2; ++flagged) {
            if (flagged) QgemulRunFlags() |= QG_OPT_BATCHED_TREE;
            {   // default tags: every product and every level rounds and saturates into int<8,8>
                Qu<dim<M, K, Bt>, e88> A;
                Qu<dim<K, N, Bt>, e88> B;
                Qu<dim<M, N, Bt>, e88> C;
                fill_real(A, 37, 0);
                fill_real(B, 53, 1);
                QgemulBatched<>(C, A, B);
                std::printf("{\"name\":\"e88_default\",\"flagged\":%d,\"launches\":%d,\"C\":[", flagged, launches_of<>(C, A, B));
                for (size_t e = 0; e < C.data.size(); ++e) std::printf("%s%lld", e ? "," : "", (long long)C.data[e].data);
                std::printf("]}\n");
            }
            {   // configuration 5's complex type under TFComplexMul
                using Mul = QgemulMulArgs<TFComplexMul<>>;
                Qu<dim<M, K, Bt>, c5> A;
                Qu<dim<K, N, Bt>, c5> B;
                Qu<dim<M, N, Bt>, c5> C;
                fill_cplx(A, 53);
                fill_cplx(B, 29);
                QgemulBatched<Mul>(C, A, B);
                std::printf("{\"name\":\"c5_tf\",\"flagged\":%d,\"launches\":%d,\"C\":[", flagged, launches_of<Mul>(C, A, B));
                for (size_t e = 0; e < C.data.size(); ++e) std::printf("%s%lld,%lld", e ? "," : "", (long long)C.data[e].real.data, (long long)C.data[e].imag.data);
                std::printf("]}\n");
            }
        }
        QgemulRelease();
    } catch (const std::exception& e) {
        std::printf("{\"error\":\"%s\"}\n", e.what());
        return 1;
    }
    return 0;
}
