#!/usr/bin/env python3
"""What the six-product kernel (k_mfma_k6) pays for a tile round that is not full.  Kernel time (HIP events, plan.time_execute) of
the headline descriptor at N = K = 4096 and M = 3840 (1280 tiles of 96 x 128: exactly 5 rounds of 256 workgroups), 4096 (1376 tiles:
5.375 rounds) and 4608 (1536: exactly 6), and at 2048^3 (352 tiles: 1.375 rounds).  If t(4096) is close to t(4608) a whole round is
paid for the 3/8 of one; if it lies near the straight line through t(3840) and t(4608), the tail round is cheap already.  The last
line gives the step time a perfectly balanced schedule would reach, t(3840) * 1376 / 1280.  Needs an MI355X.
    python tools/measure_tail.py [--label NAME] [--out FILE.jsonl]"""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from qublas_amd import capi  # noqa: E402
from qublas_amd.desc import Qu, SAT, TRN, Tags, lower  # noqa: E402

E88 = Qu(8, 8, True, TRN.TCPL, SAT.ZERO)
SHAPES = [(3840, 4096, 4096), (4096, 4096, 4096), (4608, 4096, 4096), (2048, 2048, 2048)]
TM, TN = 96, 128


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--label", default="")
    ap.add_argument("--out", default="")
    ap.add_argument("--reps", type=int, default=5)
    a = ap.parse_args()
    lines, t = [], {}
    with capi.Context() as ctx:
        for M, N, K in SHAPES:
            d = lower(E88, E88, Qu(23, 8), M, N, K, mul_args=Tags(17, 16), add_args=[Qu(29, 16)])
            plan = capi.Plan(ctx, d)
            pb = plan.info.packed_bytes
            pA, pB, pC = ctx.alloc(pb[0]), ctx.alloc(pb[1]), ctx.alloc(pb[2])
            plan.fill(capi.OPERAND_A, 1, 0, pA)
            plan.fill(capi.OPERAND_B, 2, 0, pB)
            plan.time_execute(pC, pA, pB, 300, 100)
            ms = sorted(plan.time_execute(pC, pA, pB, 20, 100) for _ in range(a.reps))
            tiles = -(-M // TM) * -(-N // TN)
            t[(M, N, K)] = ms[len(ms) // 2]
            lines.append({"label": a.label, "M": M, "N": N, "K": K, "kernel": capi.KERNEL_NAMES[plan.info.kernel], "tiles": tiles,
                          "rounds_of_256": tiles / 256, "kernel_ms": ms, "median_ms": ms[len(ms) // 2], "spread_ms": ms[-1] - ms[0]})
            print(json.dumps(lines[-1]), flush=True)
            for p in (pA, pB, pC):
                ctx.free(p)
            plan.close()
    t5, t54, t6 = t[(3840, 4096, 4096)], t[(4096, 4096, 4096)], t[(4608, 4096, 4096)]
    lines.append({"label": a.label, "summary": "tail round of 4096^3",
                  "t_3840_ms": t5, "t_4096_ms": t54, "t_4608_ms": t6, "round_ms": t6 - t5,
                  "tail_paid_as_share_of_a_round": (t54 - t5) / (t6 - t5), "tail_work_share_of_a_round": 0.375,
                  "predicted_balanced_4096_ms": t5 * 1376 / 1280, "predicted_gain_ms": t54 - t5 * 1376 / 1280})
    print(json.dumps(lines[-1]), flush=True)
    if a.out:
        with open(a.out, "a") as f:
            for ln in lines:
                f.write(json.dumps(ln) + "\n")


if __name__ == "__main__":
    main()
