#!/usr/bin/env python3
"""The complex x complex multiplication pass (QG_EW_CMUL, qg_eltwise_cplx.hip) against the pass of equal bytes.

Every arm is the chain ALONE over a packed complex C that already exists (qgemul_apply_epilogue: HIP events on the context's
stream, one process, warm-up, the arms alternating over the rounds), at S x S complex elements whose parts — of C, of the complex
tensor operand and of D — sit in 2-byte (Qu<7,8>) or 4-byte (Qu<15,12>) containers:
  basic  one CMUL stage, BasicComplexMul, x first: 4 products, 2 sums         (one launch, a lane owns both halves)
  tf     one CMUL stage, TFComplexMul, x first: 3 products, 5 sums
  add    the yardstick of equal bytes: one complex ADD stage on the same containers (two k_eltwise launches, one per half)
Every sub-operation's result is named in the parts' own format, so the three arms differ in arithmetic only.  There is no "before"
arm: the capability did not exist on the device.
Prints one JSON line per (size, container, arm): milliseconds (min / median / max over the rounds), elements per second, the
algorithmic 2 (c + e + d) container bytes per element, GB/s = bytes / median time, its share of the 8 TB/s HBM peak, the time relative
to `add`, and the arithmetic width the planner chose.
    python tools/measure_cmul.py [--sizes 8192,16384] [--cbytes 2,4] [--only basic] [--rounds 5] [--iters 20] [--out FILE]
Needs an MI355X."""
import argparse
import json
import os
import statistics
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from qublas_amd import capi  # noqa: E402
from qublas_amd.desc import BasicComplexMul, EwC, Qcomplex, Qu, TFComplexMul, lower, lower_epilogue_cplx_x  # noqa: E402

HBM_PEAK = 8.0e12
G63 = Qcomplex(Qu(6, 3), Qu(6, 3))     # the operands of the descriptor's GEMM, which never runs here


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="8192,16384")
    ap.add_argument("--cbytes", default="2,4")
    ap.add_argument("--only", default="")
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    out = open(a.out, "a") if a.out else None
    rng = np.random.default_rng(7)
    with capi.Context() as ctx:
        for S in [int(s) for s in a.sizes.split(",")]:
            for cb in [int(s) for s in a.cbytes.split(",")]:
                P = Qu(7, 8) if cb == 2 else Qu(15, 12)
                X = Qcomplex(P, P)
                d = lower(G63, G63, X, S, S, 32, mul_args=TFComplexMul())
                n = S * S
                # one host tensor of {int32 re, int32 im} elements, uniform over the part format's range: C and the operand
                host = rng.integers(P.raw_min, P.raw_max + 1, size=2 * n, dtype=np.int32)
                dX = ctx.alloc(host.nbytes)
                ctx.h2d(dX, host)
                del host
                chains = {"basic": [EwC("mul", X, tags=BasicComplexMul(loose=P))], "tf": [EwC("mul", X, tags=TFComplexMul(loose=P))], "add": [EwC("add", X, tags=P)]}
                arms, pC, pE, pD = {}, 0, 0, 0
                for name, stages in chains.items():
                    if a.only and name not in a.only.split(",") + ["add"]:
                        continue
                    epc, cx = lower_epilogue_cplx_x(X, stages, X)
                    plan = capi.Plan(ctx, d, epilogue=epc, cmul=cx)
                    if not pC:                                       # the three plans share one packed layout and container
                        pC, pE, pD = ctx.alloc(plan.packed_c_bytes()), ctx.alloc(plan.packed_e_bytes(0)), ctx.alloc(int(plan.info.packed_bytes[2]))
                        plan.pack_c(dX, pC)
                        plan.pack_e(0, dX, pE)
                        ctx.sync()
                    assert plan.packed_c_bytes() == plan.packed_e_bytes(0) == int(plan.info.packed_bytes[2]) == 2 * n * cb
                    st, form = capi.cmul_plan_form(d, epc, cx)
                    arms[name] = dict(plan=plan, args=plan.ep_args(packed=[pE]), ms=[], bits32=form.bits32 if form.has_cmul else None)
                for r in arms.values():                              # clock and code-object warm-up
                    r["plan"].time_apply_epilogue(pD, pC, r["args"], 10, 10)
                for _ in range(a.rounds):
                    for r in arms.values():
                        r["ms"].append(r["plan"].time_apply_epilogue(pD, pC, r["args"], 2, a.iters))
                base = statistics.median(arms["add"]["ms"])
                for name, r in arms.items():
                    ms = sorted(r["ms"])
                    med = statistics.median(ms)
                    bytes_el = 2 * 3 * cb
                    rec = {"arm": name, "S": S, "elements": n, "part_bytes": cb, "bytes_per_element": bytes_el, "bits32": r["bits32"],
                           "ms_min": ms[0], "ms_median": med, "ms_max": ms[-1], "rounds": a.rounds, "iters": a.iters,
                           "Gelements_per_s": n / (med * 1e-3) / 1e9, "GBps": bytes_el * n / (med * 1e-3) / 1e9,
                           "share_of_hbm_peak": bytes_el * n / (med * 1e-3) / HBM_PEAK, "time_over_add": med / base}
                    line = json.dumps(rec)
                    print(line, flush=True)
                    if out:
                        out.write(line + "\n")
                        out.flush()
                    r["plan"].close()
                for ptr in (dX, pC, pE, pD):
                    ctx.free(ptr)
    return 0


if __name__ == "__main__":
    sys.exit(main())
