#!/usr/bin/env python3
"""Two-digit Karatsuba kernel (operands of 9..12 value+sign bits, here int<6,5>) at 4096^3: QG_KARA32=1 keeps it on the 32x32x32
MFMA shape, QG_NO_KARA=1 runs the four-product 2x2 limb kernel instead; then the three-digit form of 17-bit operands (int<8,8>)
against the nine-product kernel, both arms through the plan flag.  Needs an MI355X."""
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from qublas_amd import capi  # noqa: E402
from qublas_amd.desc import Qu, SAT, TRN, Tags, lower  # noqa: E402

E = Qu(6, 5)
S = 4096
with capi.Context() as ctx:
    d = lower(E, E, Qu(25, 10), S, S, S, mul_args=Tags(13, 10), add_args=[Qu(25, 10)])
    plan = capi.Plan(ctx, d)
    pb = plan.info.packed_bytes
    pA, pB, pC = ctx.alloc(pb[0]), ctx.alloc(pb[1]), ctx.alloc(pb[2])
    plan.fill(capi.OPERAND_A, 1, 0, pA)
    plan.fill(capi.OPERAND_B, 2, 0, pB)
    plan.time_execute(pC, pA, pB, 100, 100)
    ms = min(plan.time_execute(pC, pA, pB, 20, 100) for _ in range(3))
    print(json.dumps({"workload": "4096^3 int<6,5>", "kernel": capi.KERNEL_NAMES[plan.info.kernel], "limbs": list(plan.info.limbs), "kernel_ms": ms,
                      "T_op_per_s": 2.0 * S ** 3 / (ms * 1e-3) / 1e12, "env": {k: v for k, v in os.environ.items() if k.startswith("QG_")}}), flush=True)
    plan.close()
    for p in (pA, pB, pC):
        ctx.free(p)

    # Three-digit form (17-bit operands, bench.py's headline descriptor): six products on k_mfma_k6 against the nine of k_mfma_ppl
    # under QG_OPT_SCHOOLBOOK_LIMBS, both plans alive in one process, the arms interleaved.  dist 1 (|x| < 2^8): the nine-product
    # kernel's plane masks make it a 2 x 2 launch there, the digit form has no such shortcut.
    E88 = Qu(8, 8, True, TRN.TCPL, SAT.ZERO)
    d = lower(E88, E88, Qu(23, 8), S, S, S, mul_args=Tags(17, 16), add_args=[Qu(29, 16)])
    for dist in (0, 1):
        arms = []
        for name, flags in (("six_products", 0), ("nine_products", capi.OPT_SCHOOLBOOK_LIMBS)):
            plan = capi.Plan(ctx, d, flags)
            pb = plan.info.packed_bytes
            bufs = [ctx.alloc(pb[0]), ctx.alloc(pb[1]), ctx.alloc(pb[2])]
            plan.fill(capi.OPERAND_A, 1, dist, bufs[0])
            plan.fill(capi.OPERAND_B, 2, dist, bufs[1])
            plan.time_execute(bufs[2], bufs[0], bufs[1], 100, 100)
            arms.append((name, plan, bufs, []))
        for _ in range(5):
            for name, plan, bufs, ms in arms:
                ms.append(plan.time_execute(bufs[2], bufs[0], bufs[1], 20, 100))
        for name, plan, bufs, ms in arms:
            print(json.dumps({"workload": "4096^3 int<8,8>", "dist": dist, "arm": name, "form": bytes(plan.info.reason).decode(), "kernel_ms": ms,
                              "median_ms": sorted(ms)[len(ms) // 2], "T_op_per_s": 2.0 * S ** 3 / (sorted(ms)[len(ms) // 2] * 1e-3) / 1e12}), flush=True)
            plan.close()
            for p in bufs:
                ctx.free(p)
