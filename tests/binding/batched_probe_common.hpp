// shared by amd_header_batched_probe.cpp and ref_binding_batched_probe.cpp: the QgemulBatched lowering of three tag combinations
// next to the Qgemul lowering of ONE member, as hex of the descriptor's bytes (tests/test_batched_plan.py compares them with
// qublas_amd/desc.py).  The including file provides the header under test and `using namespace` for its names.
#pragma once
#include <cstdio>
#include <cstring>

inline void print_hex(const char* key, const qgemul_desc& d)
{
    std::printf("\"%s\":\"", key);
    const unsigned char* p = reinterpret_cast<const unsigned char*>(&d);
    for (size_t i = 0; i < sizeof d; ++i) std::printf("%02x", p[i]);
    std::printf("\"");
}

template <class EC, class EA, class EB, size_t M, size_t N, size_t K, size_t Bt, bool TA, class... Tags>
void probe_batched(const char* name)
{
    Qu<dim<M, N, Bt>, EC> C;
    std::conditional_t<TA, Qu<dim<K, M, Bt>, EA>, Qu<dim<M, K, Bt>, EA>> A;
    Qu<dim<K, N, Bt>, EB> B;
    Qu<dim<M, N>, EC> C1;
    std::conditional_t<TA, Qu<dim<K, M>, EA>, Qu<dim<M, K>, EA>> A1;
    Qu<dim<K, N>, EB> B1;
    int64_t batch = 0, st[3] = {0, 0, 0};
    // (value-initialised descriptors: the padding bytes are zero in both)
    const qgemul_desc db = QgemulBatched_lower<Tags...>(C, A, B, &batch, st);
    const qgemul_desc d1 = Qgemul_lower<Tags...>(C1, A1, B1);
    std::printf("{\"name\":\"%s\",\"batch\":%lld,\"strides\":[%lld,%lld,%lld],", name, (long long)batch, (long long)st[0], (long long)st[1], (long long)st[2]);
    print_hex("batched", db);
    std::printf(",");
    print_hex("member", d1);
    std::printf("}\n");
}

inline int batched_probe_main()
{
    using e43 = Qu<intBits<4>, fracBits<3>>;
    using e88 = Qu<intBits<8>, fracBits<8>>;
    using w16 = Qu<intBits<16>, fracBits<3>>;
    probe_batched<w16, e43, e43, 64, 64, 64, 7, false, QgemulMulArgs<intBits<9>, fracBits<6>>, QgemulAddArgs<Qu<intBits<19>, fracBits<6>>>>("e43_L_64x64x64_b7");
    probe_batched<Qu<intBits<24>, fracBits<8>>, e88, e88, 33, 17, 40, 3, true, QgemulTransposedA<true>, QgemulMulArgs<intBits<17>, fracBits<16>>,
                  QgemulAddArgs<Qu<intBits<29>, fracBits<16>>>>("e88_L_tn_33x17x40_b3");
    probe_batched<e88, e88, e88, 3, 5, 7, 2, false>("e88_default_3x5x7_b2");
    return 0;
}
