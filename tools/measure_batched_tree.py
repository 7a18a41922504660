#!/usr/bin/env python3
"""Batched tree-class Qgemul: the one-launch form (QG_OPT_BATCHED_TREE: every member in ONE launch of the tree kernel's batched twin)
against the path the library takes without the flag (member by member, one kernel launch each, issued from C).

Both arms run in ONE process on the same context and stream ON THE SAME PACKED BUFFERS (the two plans share their packed layouts), HIP
events around `iters` back-to-back executions issued from C (qgemul_time_execute_batched), a warm-up of both arms first, then `rounds`
rounds in which the arms alternate; the flagged arm's packed C is compared with the unflagged arm's byte for byte before anything is
timed.
  one_launch  qgemul_time_execute_batched on the flagged plan: 1 launch per batch
  loop        qgemul_time_execute_batched on the SAME descriptor's plan without the flag: `members` launches per batch
Points: members of 64^3, 128^3 and 256 x 256 x 64 at 256 and 1024 members; formats int<4,3> (packed 16-bit steps), int<8,8>
(left-justified), int<8,8> with SAT::ZERO, Q15.16 (32-bit words) — all with default tags — and configuration 5's complex type under
TFComplexMul.  Prints one JSON line per point: microseconds per batch of both arms (min / median / max over the rounds), loop /
one_launch of the medians (above 1: the one-launch form is faster), and whether the flagged arm's maximum lay below the unflagged
arm's minimum.  No threshold: the tool reports.
    python tools/measure_batched_tree.py [--members 256,1024] [--shapes 64x64x64,128x128x128,256x256x64] [--formats i43,i88,i88z,q1516,c5tf]
                                         [--rounds 5] [--iters 10] [--out FILE]
Needs an MI355X."""
import argparse
import json
import os
import statistics
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from qublas_amd import capi  # noqa: E402
from qublas_amd.desc import Qcomplex, Qu, RND, SAT, TRN, TFComplexMul, lower  # noqa: E402

F = capi.OPT_BATCHED_TREE
FORMATS = {
    "i43": (Qu(4, 3), {}),
    "i88": (Qu(8, 8), {}),
    "i88z": (Qu(8, 8, True, TRN.TCPL, SAT.ZERO), {}),
    "q1516": (Qu(15, 16), {}),
    "c5tf": (Qcomplex(Qu(6, 3, True, RND.POS_INF, SAT.TCPL), Qu(6, -3, True, RND.POS_INF, SAT.TCPL)), dict(mul_args=TFComplexMul())),
}


def host(rng, e, n):
    """n host elements of e with uniformly random raw values: int32 words, complex = {re, im} pairs (every part here fits 32 bits)"""
    if isinstance(e, Qcomplex):
        h = np.empty((n, 2), dtype=np.int32)
        h[:, 0] = rng.integers(e.real.raw_min, e.real.raw_max + 1, size=n)
        h[:, 1] = rng.integers(e.imag.raw_min, e.imag.raw_max + 1, size=n)
        return h.reshape(-1)
    return rng.integers(e.raw_min, e.raw_max + 1, size=n, dtype=np.int32)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--members", default="256,1024")
    ap.add_argument("--shapes", default="64x64x64,128x128x128,256x256x64")
    ap.add_argument("--formats", default="i43,i88,i88z,q1516,c5tf")
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    out = open(a.out, "a") if a.out else None
    rng = np.random.default_rng(17)
    with capi.Context() as ctx:
        for name in a.formats.split(","):
            e, kw = FORMATS[name]
            for shape in a.shapes.split(","):
                M, N, K = (int(x) for x in shape.split("x"))
                d = lower(e, e, e, M, N, K, **kw)
                for batch in [int(x) for x in a.members.split(",")]:
                    on, off = capi.BatchedPlan(ctx, d, batch, F), capi.BatchedPlan(ctx, d, batch)
                    assert on.launches == 1 and off.launches == batch, (name, shape, batch, on.launches, off.launches)
                    pb = list(on.info.packed_bytes)
                    assert pb == list(off.info.packed_bytes)
                    A, B = host(rng, e, batch * M * K), host(rng, e, batch * K * N)
                    dA, dB = ctx.alloc(A.nbytes), ctx.alloc(B.nbytes)
                    ctx.h2d(dA, A)
                    ctx.h2d(dB, B)
                    pA, pB, pC = ctx.alloc(pb[0]), ctx.alloc(pb[1]), [ctx.alloc(pb[2]) for _ in range(2)]
                    on.pack(capi.OPERAND_A, dA, pA, M * K)
                    on.pack(capi.OPERAND_B, dB, pB, K * N)
                    # the arms compute the same bytes (the gaps between the members' packed Cs hold the same fill in both)
                    got = []
                    for plan, c in ((on, pC[0]), (off, pC[1])):
                        ctx.h2d(c, np.zeros(pb[2], dtype=np.uint8))
                        plan.execute(c, pA, pB)
                        ctx.sync()
                        g = np.zeros(pb[2], dtype=np.uint8)
                        ctx.d2h(g, c)
                        got.append(g)
                    assert got[0].tobytes() == got[1].tobytes(), (name, shape, batch)
                    assert len(set(got[0][:4096].tolist())) > 8

                    loop_iters = max(2, a.iters // 4)
                    on.time_execute(pC[0], pA, pB, 5, 5)
                    off.time_execute(pC[1], pA, pB, 1, loop_iters)
                    t1, tl = [], []
                    for _ in range(a.rounds):
                        t1.append(on.time_execute(pC[0], pA, pB, 2, a.iters) * 1e3)
                        tl.append(off.time_execute(pC[1], pA, pB, 1, loop_iters) * 1e3)
                    med = statistics.median
                    mmm = lambda t: {"min": min(t), "median": med(t), "max": max(t)}
                    rec = {"format": name, "M": M, "N": N, "K": K, "members": batch, "reason": bytes(on.info.reason).rstrip(b"\0").decode(),
                           "launches_one_launch": on.launches, "launches_loop": off.launches, "one_launch_us": mmm(t1), "loop_us": mmm(tl),
                           "loop_over_one_launch": med(tl) / med(t1), "loop_over_one_launch_range": [min(tl) / max(t1), max(tl) / min(t1)],
                           "one_launch_max_below_loop_min": max(t1) < min(tl), "rounds": a.rounds, "iters": a.iters, "loop_iters": loop_iters}
                    line = json.dumps(rec)
                    print(line, flush=True)
                    if out:
                        out.write(line + "\n")
                        out.flush()
                    for p in (dA, dB, pA, pB, pC[0], pC[1]):
                        ctx.free(p)
                    on.close()
                    off.close()
    return 0


if __name__ == "__main__":
    sys.exit(main())
