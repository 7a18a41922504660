#!/usr/bin/env python3
"""The piecewise-polynomial activation pass (QG_EW_APPROX, qg_approx.hip) against the HBM yardstick and the plain chain.

Every arm is the chain ALONE over a packed C that already exists (qgemul_apply_epilogue: HIP events on the context's stream,
one process, warm-up, the arms alternating over the rounds), at S x S elements of a 2-byte (Qu<3,12>) or 4-byte (Qu<15,12>) C:
  a  convert-only pass (n_stages = 0, k_eltwise): read C, write D — the HBM yardstick
  b  k_eltwise on the four-stage chain a0 + x (a1 + x a2) with x read as a TENSOR operand (twice) and C = a2
  c  the new pass, one segment of degree 2: the arithmetic of (b), x read once
  d  the new pass, 8 uniform segments of degree 3 (a fit of the logistic function)
  e  (d) with one level's QuMode changed in one segment: the general form
Prints one JSON line per (size, container, arm): milliseconds (min / median / max over the rounds), algorithmic bytes per
element, GB/s = bytes / min time, share of the 8 TB/s HBM peak.  (c) and (b) are also compared byte for byte, and a run in which
(c) is slower than (b) beyond the spread between its own rounds says so in a "check" line and exits with status 1.
    python tools/measure_approx.py [--sizes 4096,16384] [--cbytes 2,4] [--only d] [--rounds 5] [--iters 20] [--out FILE]
Needs an MI355X."""
import argparse
import json
import os
import statistics
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from qublas_amd import capi  # noqa: E402
from qublas_amd.desc import Approx, Ew, Qu, RND, SAT, Tags, lower, lower_epilogue, lower_epilogue_x  # noqa: E402

HBM_PEAK = 8.0e12
E43 = Qu(4, 3)
GEMM = dict(mul_args=Tags(9, 6), add_args=[Qu(21, 6)])
L0, L1, L2, L3 = Qu(1, 14, True, RND.CONV, SAT.TCPL), Qu(1, 13, True, RND.POS_INF, SAT.TCPL), Qu(0, 14), Qu(0, 15)
SIG = [(-4.0, 2976, 616, 173, 16), (-2.0, 8506, 2606, 1145, 178), (-1.0, 8505, 2499, 937, 77), (0.0, 8193, 2056, 69, -516),
       (1.0, 8191, 2056, -69, -516), (2.0, 7879, 2499, -937, 77), (4.0, 7878, 2606, -1145, 178), (8.0, 13408, 616, -173, 16)]
SIGMOID = [(bp, [(a0, L0), (a1, L1), (a2, L2), (a3, L3)]) for bp, a0, a1, a2, a3 in SIG]
GENERAL = [(bp, [(a, Qu(f.intBits, f.fracBits, True, RND.ZERO, f.OfMode) if (s == 3 and i == 1) else f) for i, (a, f) in enumerate(c)])
           for s, (bp, c) in enumerate(SIGMOID)]
F0, F1, F2 = Qu(3, 12, True, RND.CONV, SAT.TCPL), Qu(1, 13), Qu(0, 14)
DEG2 = [(0.0, [(8192, F0), (2056, F1), (-300, F2)])]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="4096,16384")
    ap.add_argument("--cbytes", default="2,4")
    ap.add_argument("--only", default="")
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    out = open(a.out, "a") if a.out else None
    failed = False
    with capi.Context() as ctx:
        for S in [int(s) for s in a.sizes.split(",")]:
            for cb in [int(s) for s in a.cbytes.split(",")]:
                X = Qu(3, 12) if cb == 2 else Qu(15, 12)
                d = lower(E43, E43, X, S, S, 16, **GEMM)
                base = capi.Plan(ctx, d)
                nC = int(base.info.packed_bytes[2])
                pA, pB, pC, pD = (ctx.alloc(int(n)) for n in (base.info.packed_bytes[0], base.info.packed_bytes[1], nC, nC))
                base.fill(capi.OPERAND_A, 1, 1, pA)
                base.fill(capi.OPERAND_B, 2, 1, pB)
                base.execute(pC, pA, pB)
                dX = ctx.alloc(S * S * 4)                            # C in reference layout (int32 elements)
                base.unpack_c(pC, dX)
                ctx.sync()
                for ptr in (pA, pB, pC):
                    ctx.free(ptr)
                pC = 0
                arms, keep = {}, [dX, pD]
                # (b): the running value starts as the constant a2 (format F2, 2-byte containers); x is the operand of stages 0 and 2
                (a0, _), (a1, _), (a2, _) = DEG2[0][1]
                db = lower(E43, E43, F2, S, S, 16, **GEMM)
                chain_b = [Ew("mul", X, F1, x_first=False), Ew("add", F1, F1, x_first=False, scalar=True),
                           Ew("mul", X, F0, x_first=False), Ew("add", F0, F0, x_first=False, scalar=True)]
                for name, desc, ep, tabs in (("a", d, lower_epilogue(X, [], X), None), ("b", db, lower_epilogue(F2, chain_b, X), None),
                                             ("c", d, *lower_epilogue_x(X, [Approx(DEG2)], X)), ("d", d, *lower_epilogue_x(X, [Approx(SIGMOID)], X)),
                                             ("e", d, *lower_epilogue_x(X, [Approx(GENERAL)], X))):
                    if a.only and name not in a.only.split(","):
                        continue
                    plan = capi.Plan(ctx, desc, flags=capi.OPT_UNFUSED_EPILOGUE, epilogue=ep, approx=tabs)
                    args, bytes_el = plan.ep_args(), cb + cb
                    if name != "b":
                        if not pC:                                   # one packed C for the four arms that read x as C
                            pC = ctx.alloc(plan.packed_c_bytes())
                            plan.pack_c(dX, pC)
                            keep.append(pC)
                        assert plan.packed_c_bytes() == nC
                        src = pC
                    else:
                        nb = plan.packed_c_bytes()
                        src = ctx.alloc(nb)
                        ctx.h2d(src, np.full(nb // 2, a2, dtype=np.int16))
                        pE = ctx.alloc(plan.packed_e_bytes(0))
                        plan.pack_e(0, dX, pE)
                        ctx.sync()
                        args = plan.ep_args(packed=[pE, 0, pE, 0], scalars=[0, a1, 0, a0])
                        bytes_el = 2 + 2 * (plan.packed_e_bytes(0) // (nC // cb)) + cb
                        keep += [src, pE]
                    form = capi.approx_plan_form(desc, ep, tabs) if tabs else None
                    arms[name] = dict(plan=plan, src=src, args=args, bytes_el=bytes_el, ms=[],
                                      form=None if form is None else {"bits32": form.bits32, "uniform": form.uniform[0]})
                if "b" in arms and "c" in arms and S <= 4096:     # the same bytes before any time is compared
                    outs = []
                    for name in ("b", "c"):
                        r = arms[name]
                        r["plan"].apply_epilogue(pD, r["src"], r["args"])
                        h = np.zeros(nC, dtype=np.uint8)
                        ctx.d2h(h, pD)
                        outs.append(h)
                    assert np.array_equal(outs[0], outs[1]), "one-segment table and plain chain differ"
                for r in arms.values():                            # clock and code-object warm-up
                    r["plan"].time_apply_epilogue(pD, r["src"], r["args"], 10, 10)
                for _ in range(a.rounds):
                    for r in arms.values():
                        r["ms"].append(r["plan"].time_apply_epilogue(pD, r["src"], r["args"], 2, a.iters))
                if "b" in arms and "c" in arms:
                    # (c) does the arithmetic of (b) with a third of the x traffic: not slower beyond the spread of this very run
                    b, c = sorted(arms["b"]["ms"]), sorted(arms["c"]["ms"])
                    spread = max((m[-1] - m[0]) / m[0] for m in (b, c))
                    verdict = {"check": "c_not_slower_than_b", "S": S, "c_bytes": cb, "c_over_b": c[0] / b[0], "spread": spread,
                               "ok": c[0] <= b[0] * (1 + spread)}
                    print(json.dumps(verdict), flush=True)
                    if out:
                        out.write(json.dumps(verdict) + "\n")
                    failed = failed or not verdict["ok"]
                for name, r in arms.items():
                    ms = sorted(r["ms"])
                    rec = {"arm": name, "S": S, "elements": S * S, "c_bytes": cb, "bytes_per_element": r["bytes_el"], "form": r["form"],
                           "ms_min": ms[0], "ms_median": statistics.median(ms), "ms_max": ms[-1], "rounds": a.rounds, "iters": a.iters,
                           "GBps": r["bytes_el"] * S * S / (ms[0] * 1e-3) / 1e9, "share_of_hbm_peak": r["bytes_el"] * S * S / (ms[0] * 1e-3) / HBM_PEAK,
                           "ps_per_element": ms[0] * 1e9 / (S * S)}
                    line = json.dumps(rec)
                    print(line, flush=True)
                    if out:
                        out.write(line + "\n")
                        out.flush()
                    r["plan"].close()
                base.close()
                for ptr in keep:
                    ctx.free(ptr)
    return 1 if failed else 0


if __name__ == "__main__":
    sys.exit(main())
