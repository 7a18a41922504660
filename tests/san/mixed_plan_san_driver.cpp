// TEST INFRASTRUCTURE: the planner (qublas_amd/csrc/qg_plan.cpp under qg_geom.cpp) on descriptors with one real and one complex
// operand (QG_CMUL_REAL_A / QG_CMUL_REAL_B), compiled for the CPU with AddressSanitizer + UndefinedBehaviorSanitizer.  Reads records of
//   uint32 flags, uint32 kind (0 plain, 1 batched with batch 3, 2 with a one-stage real chain), qgemul_desc
// from stdin and prints one line per record: the verdict of qg_plan_geometry, which tests/test_mixed_plan.py compares with the product
// library's.  Any sanitizer report fails the run.  No GPU code is involved.
#include <stdio.h>
#include <string.h>

#include <vector>

#include "../../qublas_amd/csrc/qg_geom.h"

int main()
{
    std::vector<unsigned char> buf;
    unsigned char tmp[65536];
    size_t n;
    while ((n = fread(tmp, 1, sizeof tmp, stdin)) > 0) buf.insert(buf.end(), tmp, tmp + n);
    const size_t rec = 8 + sizeof(qgemul_desc);
    if (buf.size() % rec) { fprintf(stderr, "truncated input\n"); return 2; }
    QPlanGeom* g = new QPlanGeom();
    qgemul_epilogue ep;
    for (size_t at = 0; at < buf.size(); at += rec) {
        uint32_t flags, kind;
        qgemul_desc d;
        memcpy(&flags, buf.data() + at, 4);
        memcpy(&kind, buf.data() + at + 4, 4);
        memcpy((void*)&d, buf.data() + at + 8, sizeof d);
        memset(&ep, 0, sizeof ep);   // n_stages = 0: D = C converted into d
        ep.d = d.c[0];
        const EpView v = {&ep, nullptr, nullptr};
        *g = QPlanGeom();
        const int st = qg_plan_geometry(&d, flags, kind == 2 ? &v : nullptr, kind == 1 ? 3 : 0, g, nullptr, nullptr);
        const qgemul_info& i = g->info;
        printf("st=%d sup=%d cls=%d kernel=%d max_bits=%d in_bits=%d,%d packed=%lld,%lld,%lld ops=%.17g heb=%d,%d,%d hio=%d,%d,%d reason=%s\n", st, i.supported, st == QG_OK ? i.cls : 0,
               st == QG_OK ? i.kernel : 0, st == QG_OK ? i.max_bits : 0, st == QG_OK ? i.in_bits[0] : 0, st == QG_OK ? i.in_bits[1] : 0,
               st == QG_OK ? (long long)i.packed_bytes[0] : 0ll, st == QG_OK ? (long long)i.packed_bytes[1] : 0ll, st == QG_OK ? (long long)i.packed_bytes[2] : 0ll,
               st == QG_OK ? i.ops : 0.0, st == QG_OK ? i.host_elem_bytes[0] : 0, st == QG_OK ? i.host_elem_bytes[1] : 0, st == QG_OK ? i.host_elem_bytes[2] : 0,
               st == QG_OK ? i.host_imag_off[0] : 0, st == QG_OK ? i.host_imag_off[1] : 0, st == QG_OK ? i.host_imag_off[2] : 0, i.reason);
    }
    delete g;
    return 0;
}
