// Random complex chains with CMUL stages — well-formed, borderline (formats at the 62-bit guard) and deliberately malformed (wild
// format fields, unknown ops and algorithms, mismatched parts, missing and surplus records, part chains of different lengths) —
// through qg_analyze_epcx.  Built with AddressSanitizer + UndefinedBehaviorSanitizer by tests/test_cmul_plan.py (a stand-alone CPU
// program): the planner must answer every one of them with a status and report nothing; nothing accepted exceeds 62 bits.
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include "../../qublas_amd/csrc/qg_plan.h"
#include "../../qublas_amd/csrc/qg_cmul.h"
static unsigned long long s = 88172645463325252ull;
static unsigned rnd() { s ^= s << 13; s ^= s >> 7; s ^= s << 17; return (unsigned)(s >> 11); }
static qfmt rf(bool wild) {
    qfmt f; memset(&f, 0, sizeof f);
    if (wild && rnd() % 8 == 0) { f.I = (int16_t)(rnd() % 65536 - 32768); f.F = (int16_t)(rnd() % 65536 - 32768); }
    else { f.F = (int16_t)((int)(rnd() % 40) - 8); f.I = (int16_t)((int)(rnd() % 40) - (f.F < 0 ? f.F : 0)); if (rnd()%6==0) f.I = (int16_t)(62 - f.F); }
    f.S = rnd() % 4 != 0; f.Q = rnd() % (wild ? 9 : 7); f.O = rnd() % (wild ? 6 : 5);
    return f;
}
int main() {
    int ok = 0, inv = 0, uns = 0;
    for (int it = 0; it < 60000; ++it) {
        bool wild = it % 3 == 0;
        qgemul_epilogue_cplx ep; memset(&ep, 0, sizeof ep);
        qgemul_cmul cx[QG_MAX_EW]; const qgemul_cmul* pcx[QG_MAX_EW] = {};
        unsigned n = rnd() % (wild ? 6 : 5);
        ep.part[0].n_stages = n; ep.part[1].n_stages = (wild && rnd() % 16 == 0) ? rnd() % 6 : n;
        qfmt c[2] = {rf(wild), rf(wild)};
        for (unsigned k = 0; k < QG_MAX_EW; ++k) {
            bool cm = rnd() % 2;
            memset(&cx[k], 0, sizeof cx[k]);
            cx[k].cmul = wild ? rnd() % 4 : 1 + rnd() % 2;
            for (int i = 0; i < 8; ++i) cx[k].mul[i] = rf(wild);
            for (int p = 0; p < 2; ++p) {
                qgemul_ew_stage& st = ep.part[p].stage[k];
                st.op = cm ? QG_EW_CMUL : 1 + rnd() % 4; if (wild && rnd() % 16 == 0) st.op = rnd() % 9;
                st.x_first = rnd() % 2; st.e_scalar = rnd() % 2;
                if (cm && !(wild && rnd() % 8 == 0)) { st.x_first = ep.part[0].stage[k].x_first; st.e_scalar = ep.part[0].stage[k].e_scalar; }
                st.e = rf(wild); st.t = rf(wild);
                st.r = cm ? cx[k].mul[(cx[k].cmul == 2 ? 6 : 4) + p] : rf(wild);
            }
            ep.e_complex[k] = cm ? !(wild && rnd() % 8 == 0) : rnd() % 2;
            if ((cm && k < n) != (wild && rnd() % 16 == 0)) pcx[k] = &cx[k];
        }
        ep.part[0].d = rf(wild); ep.part[1].d = rf(wild);
        QEpTable t[2]; QCmulStage cmt[QG_MAX_EW]; int mb = 0; char why[96];
        int st = qg_analyze_epcx(c, &ep, pcx, t, rnd() % 2 ? cmt : nullptr, &mb, why, sizeof why);
        if (st == QG_OK) { ++ok; if (mb > 62) { printf("max_bits %d accepted\n", mb); return 1; } } else if (st == QG_EINVAL) ++inv; else ++uns;
    }
    printf("ok %d einval %d eunsupported %d\n", ok, inv, uns);
    return 0;
}
