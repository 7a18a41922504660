// Runs QgemulBatched through include/QuBLAS_amd.h on the GPU (compiled by tests/test_gpu_batched.py with clang++ -std=c++23, linked
// against qublas_amd/libqugemm.so): a linear-class batch (one block-diagonal launch) and a default-tag batch (member by member).
// Prints every C; the test recomputes each member with the oracle from the same raw inputs.
#include "QuBLAS_amd.h"

#include <cstdio>

using namespace QuBLAS_amd;

template <class T>
static void print_c(const char* name, size_t M, size_t N, size_t K, size_t Bt, const T& C)
{
    std::printf("{\"name\":\"%s\",\"M\":%zu,\"N\":%zu,\"K\":%zu,\"batch\":%zu,\"C\":[", name, M, N, K, Bt);
    for (size_t e = 0; e < C.data.size(); ++e) std::printf("%s%lld", e ? "," : "", (long long)C.data[e].data);
    std::printf("]}\n");
}

int main()
{
    try {
        using e88 = Qu<intBits<8>, fracBits<8>>;
        constexpr size_t M = 65, N = 33, K = 40, Bt = 5;
        {
            Qu<dim<K, M, Bt>, e88> A;   // QgemulTransposedA<true>: members declared dim<K, M>
            Qu<dim<K, N, Bt>, e88> B;
            Qu<dim<M, N, Bt>, Qu<intBits<24>, fracBits<8>>> C;
            for (size_t i = 0; i < A.data.size(); ++i) A[i].fill(int64_t((i * 2654435761ull) % 131072) - 65536);
            for (size_t i = 0; i < B.data.size(); ++i) B[i].fill(int64_t((i * 40503ull + 7) % 131072) - 65536);
            QgemulBatched<QgemulTransposedA<true>, QgemulMulArgs<intBits<17>, fracBits<16>>, QgemulAddArgs<Qu<intBits<29>, fracBits<16>>>>(C, A, B);
            print_c("e88_L_tn", M, N, K, Bt, C);
        }
        {
            constexpr size_t m = 7, n = 5, k = 9, bt = 3;
            Qu<dim<m, k, bt>, e88> A;
            Qu<dim<k, n, bt>, e88> B;
            Qu<dim<m, n, bt>, e88> C;
            for (size_t i = 0; i < A.data.size(); ++i) A[i].fill(int64_t((i * 37ull) % 8192) - 4096);
            for (size_t i = 0; i < B.data.size(); ++i) B[i].fill(int64_t((i * 53ull + 1) % 8192) - 4096);
            QgemulBatched<>(C, A, B);
            print_c("e88_default", m, n, k, bt, C);
        }
        QgemulRelease();
    } catch (const std::exception& e) {
        std::printf("{\"error\":\"%s\"}\n", e.what());
        return 1;
    }
    return 0;
}
