#!/usr/bin/env python3
"""Opt-in fuzz of the RING plans on an MI355X (not collected by pytest): product and every level in one signed
WRP::TCPL format of n = 2 ... 32 bits entered by a left shift s = 0 ... n - 1, operands of any width up to 32 storage bits and any
modes (signed and unsigned, narrower and wider than the ring), level types whose QuMode differs, C of any width up to 62 bits and
any modes, any shape around the tiles, K up to 20 000, transposed A, the three operand distributions.  Descriptors that are exact
anyway or that the one-column kernels keep are counted and checked too.  Each case: the default plan against the oracle AND against
QG_OPT_FORCE_TREE (the tree kernels these descriptors ran on before), bit for bit.
usage: python tests/extended_fuzz_ring.py [cases] [seed] [dry]"""
import json
import os
import random
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
from oracle import qoracle as oracle  # noqa: E402
from qublas_amd import capi  # noqa: E402
from qublas_amd.desc import Qu, RND, SAT, TRN, WRP, Tags, lower  # noqa: E402

QM = [TRN.TCPL, TRN.SMGN, RND.POS_INF, RND.NEG_INF, RND.ZERO, RND.INF, RND.CONV]
OM = [SAT.TCPL, SAT.SMGN, SAT.ZERO, WRP.TCPL]


def main():
    cases = int(sys.argv[1]) if len(sys.argv) > 1 else 1500
    seed = int(sys.argv[2]) if len(sys.argv) > 2 else 2468
    rng = random.Random(seed)
    dry = len(sys.argv) > 3 and sys.argv[3] == "dry"      # (no GPU: only which plans the planner picks)
    oracle.lib()
    ran = skipped = 0
    plans = {}
    while ran < cases:
        n = rng.choice([8, 12, 16, 24, 32, 32, rng.randint(2, 32)])
        s = rng.choice([0, 0, 0, rng.randint(0, n - 1)])
        # operands: fraction bits fa + fb = F_R - s; widths around the ring's
        wa, wb = (min(31, max(1, n - 1 + rng.randint(-9, 4))) for _ in range(2))
        fa, fb = rng.randint(-2, max(0, wa // 2)), rng.randint(-2, max(0, wb // 2))
        fr = fa + fb + s
        ring = Qu(n - 1 - fr, fr, True, rng.choice(QM), WRP.TCPL)
        level = Qu(n - 1 - fr, fr, True, rng.choice(QM), WRP.TCPL)
        sa, sb = rng.random() < 0.85, rng.random() < 0.85
        ea = Qu(wa - fa, fa, sa, rng.choice(QM), rng.choice(OM))
        eb = Qu(wb - fb, fb, sb, rng.choice(QM), rng.choice(OM))
        if rng.random() < 0.4:
            ec = ring
        else:
            cw = rng.choice([3, 7, 12, 15, 23, 31, 40, 62])
            cf = fr + rng.randint(-8, 8)
            ec = Qu(cw - cf, cf, rng.random() < 0.8, rng.choice(QM), rng.choice(OM))
        M, N = rng.choice([1, 5, 64, 127, 128, 129, 200, 300]), rng.choice([1, 2, 7, 127, 128, 129, 260])
        K = rng.choice([1, 2, 3, 63, 64, 65, 100, 129, 1000, 4097, 20000])
        if K >= 4097:
            M, N = min(M, 129), min(N, 129)
        try:
            d = lower(ea, eb, ec, M, N, K, mul_args=Tags.of(ring), add_args=[level], transposed_a=rng.random() < 0.5)
        except (ValueError, OverflowError):
            skipped += 1
            continue
        st, info = capi.classify_status(d)
        if st != capi.QG_OK:
            skipped += 1
            continue
        reason = info.reason.decode()
        kind = "ring, %s" % reason.split(", ")[-1] if "wrapping ring" in reason else capi.KERNEL_NAMES[info.kernel] + (" (exact linear)" if info.cls == 1 else "")
        plans[kind] = plans.get(kind, 0) + 1
        ran += 1
        if dry:
            continue
        dist = rng.choice([0, 0, 1, 2])
        A = oracle.fill(ea, M * K, rng.randint(1, 1 << 30), dist)
        B = oracle.fill(eb, K * N, rng.randint(1, 1 << 30), dist)
        exp = oracle.gemm(d, A, B, ec, nthreads=8)
        out = capi.run(d, np.zeros(M * N, dtype=oracle.host_dtype(ec)), A, B)
        tree = capi.run(d, np.zeros(M * N, dtype=oracle.host_dtype(ec)), A, B, flags=capi.OPT_FORCE_TREE)
        if not (np.array_equal(out, exp) and np.array_equal(tree, exp)):
            print(json.dumps({"mismatch": ran, "plan": kind, "ring_vs_oracle": bool(np.array_equal(out, exp)), "tree_vs_oracle": bool(np.array_equal(tree, exp)),
                              "M": M, "N": N, "K": K, "a": str(ea), "b": str(eb), "c": str(ec), "ring": str(ring), "level": str(level), "transA": int(d.transA), "dist": dist}), flush=True)
            sys.exit(1)
    print(json.dumps({"ring_fuzz_cases": ran, "seed": seed, "skipped_unsupported": skipped, "plans": plans, "mismatches": 0}), flush=True)


if __name__ == "__main__":
    main()
