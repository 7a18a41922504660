// shared by amd_header_grouped_probe.cpp and ref_binding_grouped_probe.cpp: the QgemulGrouped lowering of triples of different dim<>
// next to the Qgemul lowering of each triple, as hex of the descriptors' bytes (tests/test_grouped_binding.py compares them with
// each other and with qublas_amd/desc.py).  The including file provides the header under test and `using namespace` for its names.
#pragma once
#include <cstdio>
#include <cstring>
#include <tuple>

inline void print_hex(const qgemul_desc& d)
{
    std::printf("\"");
    const unsigned char* p = reinterpret_cast<const unsigned char*>(&d);
    for (size_t i = 0; i < sizeof d; ++i) std::printf("%02x", p[i]);
    std::printf("\"");
}

template <size_t G>
void print_group(const char* name, const std::array<qgemul_desc, G>& grouped, const std::array<qgemul_desc, G>& single)
{
    std::printf("{\"name\":\"%s\",\"grouped\":[", name);
    for (size_t g = 0; g < G; ++g) { if (g) std::printf(","); print_hex(grouped[g]); }
    std::printf("],\"single\":[");
    for (size_t g = 0; g < G; ++g) { if (g) std::printf(","); print_hex(single[g]); }
    std::printf("]}\n");
}

inline int grouped_probe_main()
{
    using e43 = Qu<intBits<4>, fracBits<3>>;
    using e88 = Qu<intBits<8>, fracBits<8>>;
    using w16 = Qu<intBits<16>, fracBits<3>>;
    {   // three shapes of one linear-class tag set
        Qu<dim<64, 64>, w16> C0; Qu<dim<64, 64>, e43> A0; Qu<dim<64, 64>, e43> B0;
        Qu<dim<65, 33>, w16> C1; Qu<dim<65, 100>, e43> A1; Qu<dim<100, 33>, e43> B1;
        Qu<dim<3, 5>, w16> C2; Qu<dim<3, 7>, e43> A2; Qu<dim<7, 5>, e43> B2;
        using MA = QgemulMulArgs<intBits<9>, fracBits<6>>;
        using AA = QgemulAddArgs<Qu<intBits<19>, fracBits<6>>>;
        print_group<3>("e43_L_three_shapes", QgemulGrouped_lower<MA, AA>(std::tie(C0, C1, C2), std::tie(A0, A1, A2), std::tie(B0, B1, B2)),
                       {{Qgemul_lower<MA, AA>(C0, A0, B0), Qgemul_lower<MA, AA>(C1, A1, B1), Qgemul_lower<MA, AA>(C2, A2, B2)}});
    }
    {   // transposed A, two shapes
        using c24 = Qu<intBits<24>, fracBits<8>>;
        Qu<dim<33, 17>, c24> C0; Qu<dim<40, 33>, e88> A0; Qu<dim<40, 17>, e88> B0;
        Qu<dim<5, 9>, c24> C1; Qu<dim<130, 5>, e88> A1; Qu<dim<130, 9>, e88> B1;
        using TA = QgemulTransposedA<true>;
        using MA = QgemulMulArgs<intBits<17>, fracBits<16>>;
        using AA = QgemulAddArgs<Qu<intBits<29>, fracBits<16>>>;
        print_group<2>("e88_L_tn_two_shapes", QgemulGrouped_lower<TA, MA, AA>(std::tie(C0, C1), std::tie(A0, A1), std::tie(B0, B1)),
                       {{Qgemul_lower<TA, MA, AA>(C0, A0, B0), Qgemul_lower<TA, MA, AA>(C1, A1, B1)}});
    }
    {   // default tags, one member
        Qu<dim<3, 5>, e88> C0; Qu<dim<3, 7>, e88> A0; Qu<dim<7, 5>, e88> B0;
        print_group<1>("e88_default_one", QgemulGrouped_lower<>(std::tie(C0), std::tie(A0), std::tie(B0)), {{Qgemul_lower<>(C0, A0, B0)}});
    }
    return 0;
}
