// Runs QgemulGrouped through include/QuBLAS_amd.h on the GPU (compiled by tests/test_gpu_grouped.py, linked against
// qublas_amd/libqugemm.so): three linear-class triples of different dim<>, one call with QgemulTransposedA<true>, and a default-tag
// group (tree class: every member a straggler).  Every C is compared with the header's own Qgemul of that triple.
#include "QuBLAS_amd.h"

#include <cstdio>

using namespace QuBLAS_amd;

template <class T>
static void fill(T& t, unsigned long long mul, unsigned long long add, long long range)
{
    for (size_t i = 0; i < t.data.size(); ++i) t[i].fill((long long)((i * mul + add) % (unsigned long long)(2 * range)) - range);
}
template <class T>
static bool same(const char* name, const T& x, const T& y)
{
    size_t distinct = 0;
    for (size_t e = 0; e < x.data.size(); ++e) {
        if (x.data[e].data != y.data[e].data) { std::printf("%s: element %zu differs\n", name, e); return false; }
        if (e && x.data[e].data != x.data[e - 1].data) ++distinct;
    }
    if (x.data.size() > 16 && distinct < 8) { std::printf("%s: the result is nearly constant\n", name); return false; }
    return true;
}

int main()
{
    try {
        using e88 = Qu<intBits<8>, fracBits<8>>;
        using c24 = Qu<intBits<24>, fracBits<8>>;
        using MA = QgemulMulArgs<intBits<17>, fracBits<16>>;
        using AA = QgemulAddArgs<Qu<intBits<29>, fracBits<16>>>;
        bool ok = true;
        {   // three triples of different dim<>
            Qu<dim<65, 100>, e88> A0; Qu<dim<100, 33>, e88> B0; Qu<dim<65, 33>, c24> C0, R0;
            Qu<dim<3, 7>, e88> A1; Qu<dim<7, 5>, e88> B1; Qu<dim<3, 5>, c24> C1, R1;
            Qu<dim<129, 65>, e88> A2; Qu<dim<65, 130>, e88> B2; Qu<dim<129, 130>, c24> C2, R2;
            fill(A0, 2654435761ull, 0, 65536); fill(B0, 40503ull, 7, 65536);
            fill(A1, 37ull, 3, 4096); fill(B1, 53ull, 1, 4096);
            fill(A2, 7919ull, 11, 65536); fill(B2, 104729ull, 5, 65536);
            QgemulGrouped<MA, AA>(std::tie(C0, C1, C2), std::tie(A0, A1, A2), std::tie(B0, B1, B2));
            Qgemul<MA, AA>(R0, A0, B0); Qgemul<MA, AA>(R1, A1, B1); Qgemul<MA, AA>(R2, A2, B2);
            ok = same("L0", C0, R0) && same("L1", C1, R1) && same("L2", C2, R2) && ok;
        }
        {   // QgemulTransposedA<true>: A declared dim<K, M>
            using TA = QgemulTransposedA<true>;
            Qu<dim<40, 33>, e88> A0; Qu<dim<40, 17>, e88> B0; Qu<dim<33, 17>, c24> C0, R0;
            Qu<dim<130, 5>, e88> A1; Qu<dim<130, 9>, e88> B1; Qu<dim<5, 9>, c24> C1, R1;
            fill(A0, 2654435761ull, 1, 65536); fill(B0, 40503ull, 9, 65536);
            fill(A1, 7919ull, 2, 65536); fill(B1, 104729ull, 4, 65536);
            QgemulGrouped<TA, MA, AA>(std::tie(C0, C1), std::tie(A0, A1), std::tie(B0, B1));
            Qgemul<TA, MA, AA>(R0, A0, B0); Qgemul<TA, MA, AA>(R1, A1, B1);
            ok = same("T0", C0, R0) && same("T1", C1, R1) && ok;
        }
        {   // default tags (tree class): stragglers through the same call
            Qu<dim<7, 9>, e88> A0; Qu<dim<9, 5>, e88> B0; Qu<dim<7, 5>, e88> C0, R0;
            Qu<dim<33, 40>, e88> A1; Qu<dim<40, 17>, e88> B1; Qu<dim<33, 17>, e88> C1, R1;
            // (|x| < 2: the default tags' int<8,8> products and sums stay inside C's range, so the results vary)
            fill(A0, 37ull, 0, 512); fill(B0, 53ull, 1, 512);
            fill(A1, 41ull, 2, 512); fill(B1, 59ull, 3, 512);
            QgemulGrouped<>(std::tie(C0, C1), std::tie(A0, A1), std::tie(B0, B1));
            Qgemul<>(R0, A0, B0); Qgemul<>(R1, A1, B1);
            ok = same("D0", C0, R0) && same("D1", C1, R1) && ok;
        }
        QgemulRelease();
        if (!ok) return 1;
        std::printf("grouped ok\n");
    } catch (const std::exception& e) {
        std::printf("error: %s\n", e.what());
        return 1;
    }
    return 0;
}
