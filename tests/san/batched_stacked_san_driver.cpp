// TEST INFRASTRUCTURE: the batched planner (qg_batched_geometry / qg_batched_launches, qublas_amd/csrc/qg_geom.cpp over qg_plan.cpp) on
// complex and mixed members with and without QG_OPT_BATCHED_STACKED, compiled for the CPU with AddressSanitizer +
// UndefinedBehaviorSanitizer.  Reads records of
//   uint32 flags, int64 batch, qgemul_desc
// from stdin and prints one line per record: the verdict, the stack's info, the launch count and — in the stacked form — the member
// block's tile counts and the workspace, which tests/test_batched_stacked_plan.py compares with the product library's answers and with
// its own restatement of the geometry.  Any sanitizer report fails the run.  No GPU code is involved.
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
    const size_t rec = 12 + sizeof(qgemul_desc);
    if (buf.size() % rec) { fprintf(stderr, "truncated input\n"); return 2; }
    QPlanGeom* m = new QPlanGeom();
    QPlanGeom* s = new QPlanGeom();
    for (size_t at = 0; at < buf.size(); at += rec) {
        uint32_t flags;
        int64_t batch;
        qgemul_desc d;
        memcpy(&flags, buf.data() + at, 4);
        memcpy(&batch, buf.data() + at + 4, 8);
        memcpy((void*)&d, buf.data() + at + 12, sizeof d);
        *m = QPlanGeom();
        *s = QPlanGeom();
        QBatchGeom b = QBatchGeom();
        const int st = qg_batched_geometry(&d, batch, flags, nullptr, nullptr, m, s, &b);
        const qgemul_info& i = s->info;
        const bool ok = st == QG_OK;
        printf("st=%d sup=%d kernel=%d limbs=%d,%d packed=%lld,%lld,%lld ops=%.17g launches=%d stack=%d tiles=%d,%d ws=%lld reason=%s\n", st, batch >= 1 ? i.supported : 0,
               ok ? i.kernel : 0, ok ? i.limbs[0] : 0, ok ? i.limbs[1] : 0, ok ? (long long)i.packed_bytes[0] : 0ll, ok ? (long long)i.packed_bytes[1] : 0ll,
               ok ? (long long)i.packed_bytes[2] : 0ll, ok ? i.ops : 0.0, ok ? qg_batched_launches(s, &b, false) : 0, ok ? s->bd_stack : 0, ok ? b.bd_tm : 0,
               ok ? b.bd_tn : 0, ok ? (long long)b.stack_ws : 0ll, batch >= 1 ? i.reason : "");
    }
    delete m;
    delete s;
    return 0;
}
