#!/usr/bin/env python3
"""Batched Qgemul: the one-launch block-diagonal form against the loop of qgemul_execute calls it replaces.

Both arms run in ONE process on the same context and stream, on operands packed once from the same host data, HIP events around
`iters` back-to-back executions, a warm-up of both arms first (clock, code objects), then `rounds` rounds in which the arms alternate;
the result of the batched arm is compared with the loop's, member by member, before anything is timed.
  batched  qgemul_execute_batched on a batched plan: one kernel launch for the whole batch
  loop     `members` calls of qgemul_execute on ONE plain plan of the member's descriptor, each member with its own packed operands
           and its own packed C: what the library offered for this work before the batched entry points existed (the baseline).
           Issued from Python; "loop_in_c" prices the same launches issued from C (qgemul_time_execute on one member x members)
Points: members 64^3, 128^3 and 256 x 256 x 64, in int<4,3> (one int8 limb) and int<8,8> (3 x 3 limbs), 256 and 1024 members each.
Prints one JSON line per point: microseconds per batch of either arm (min / median / max over the rounds), the ratio of the medians
(loop / batched: above 1 the one-launch form is faster), microseconds per member, launches per execute, and the tile geometry.
Exit status 1 when the one-launch form is slower than the loop (either pricing) at any point.
    python tools/measure_batched.py [--members 256,1024] [--shapes 64x64x64,128x128x128,256x256x64] [--formats e43,e88] [--rounds 7]
                                    [--iters 20] [--out FILE]
Needs an MI355X."""
import argparse
import ctypes as C
import json
import os
import statistics
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from qublas_amd import capi  # noqa: E402
from qublas_amd.desc import Qu, Tags, lower  # noqa: E402

FORMATS = {
    "e43": (Qu(4, 3), Qu(16, 3), dict(mul_args=Tags(9, 6), add_args=[Qu(19, 6)])),
    "e88": (Qu(8, 8), Qu(24, 8), dict(mul_args=Tags(17, 16), add_args=[Qu(29, 16)])),
}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--members", default="256,1024")
    ap.add_argument("--shapes", default="64x64x64,128x128x128,256x256x64")
    ap.add_argument("--formats", default="e43,e88")
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    out = open(a.out, "a") if a.out else None
    rng = np.random.default_rng(11)
    hip = C.CDLL("libamdhip64.so")
    slower = 0
    with capi.Context() as ctx:
        for fmt in a.formats.split(","):
            e, ec, kw = FORMATS[fmt]
            for shape in a.shapes.split(","):
                M, N, K = (int(x) for x in shape.split("x"))
                d = lower(e, e, ec, M, N, K, **kw)
                for batch in [int(x) for x in a.members.split(",")]:
                    bp, pp = capi.BatchedPlan(ctx, d, batch), capi.Plan(ctx, d)
                    hb = pp.info.host_elem_bytes
                    A = rng.integers(e.raw_min, e.raw_max + 1, size=batch * M * K, dtype=np.int32)
                    B = rng.integers(e.raw_min, e.raw_max + 1, size=batch * K * N, dtype=np.int32)
                    dA, dB = ctx.alloc(A.nbytes), ctx.alloc(B.nbytes)
                    ctx.h2d(dA, A)
                    ctx.h2d(dB, B)
                    bb, mb = bp.info.packed_bytes, [(x + 255) // 256 * 256 for x in pp.info.packed_bytes]
                    bA, bB, bC = ctx.alloc(bb[0]), ctx.alloc(bb[1]), ctx.alloc(bb[2])
                    lA, lB, lC = ctx.alloc(batch * mb[0]), ctx.alloc(batch * mb[1]), ctx.alloc(batch * mb[2])
                    hC = [ctx.alloc(batch * M * N * hb[2]) for _ in range(2)]
                    bp.pack(capi.OPERAND_A, dA, bA, M * K)
                    bp.pack(capi.OPERAND_B, dB, bB, K * N)
                    for b in range(batch):
                        pp.pack(capi.OPERAND_A, dA + b * M * K * hb[0], lA + b * mb[0])
                        pp.pack(capi.OPERAND_B, dB + b * K * N * hb[1], lB + b * mb[1])

                    def loop():
                        for b in range(batch):
                            pp.execute(lC + b * mb[2], lA + b * mb[0], lB + b * mb[1])

                    # the two arms compute the same bytes
                    bp.execute(bC, bA, bB)
                    bp.unpack_c(bC, hC[0], M * N)
                    loop()
                    for b in range(batch):
                        pp.unpack_c(lC + b * mb[2], hC[1] + b * M * N * hb[2])
                    ctx.sync()
                    got = [np.zeros(batch * M * N * hb[2], dtype=np.uint8) for _ in range(2)]
                    ctx.d2h(got[0], hC[0])
                    ctx.d2h(got[1], hC[1])
                    assert got[0].tobytes() == got[1].tobytes(), (fmt, shape, batch)
                    assert len(set(got[0][:4096].tolist())) > 8

                    def time_loop(warm, iters):
                        """HIP events on the context's stream around iters x members qgemul_execute calls; ms per batch"""
                        e0, e1 = C.c_void_p(), C.c_void_p()
                        assert hip.hipEventCreate(C.byref(e0)) == 0 and hip.hipEventCreate(C.byref(e1)) == 0
                        st = C.c_void_p(ctx.stream)
                        for _ in range(warm):
                            loop()
                        assert hip.hipEventRecord(e0, st) == 0
                        for _ in range(iters):
                            loop()
                        assert hip.hipEventRecord(e1, st) == 0 and hip.hipEventSynchronize(e1) == 0
                        ms = C.c_float()
                        assert hip.hipEventElapsedTime(C.byref(ms), e0, e1) == 0
                        hip.hipEventDestroy(e0)
                        hip.hipEventDestroy(e1)
                        return ms.value / iters

                    # The loop arm issues its launches from Python, one ctypes call each; a caller in C issues them faster.  So the
                    # loop is ALSO priced without the interpreter: qgemul_time_execute on one member (back-to-back launches of the
                    # member's kernel from C) times the member count — "loop_in_c", the stricter baseline of the two.
                    bp.time_execute(bC, bA, bB, 10, 10)
                    time_loop(2, 2)
                    tb, tl, t1 = [], [], []
                    for _ in range(a.rounds):
                        tb.append(bp.time_execute(bC, bA, bB, 2, a.iters) * 1e3)
                        tl.append(time_loop(1, max(2, a.iters // 4)) * 1e3)
                        t1.append(pp.time_execute(lC, lA, lB, 2, a.iters * 8) * 1e3 * batch)
                    medb, medl, med1 = statistics.median(tb), statistics.median(tl), statistics.median(t1)
                    rec = {"format": fmt, "M": M, "N": N, "K": K, "members": batch, "launches_batched": bp.launches, "reason": bytes(bp.info.reason).decode(),
                           "batched_us": {"min": min(tb), "median": medb, "max": max(tb)},
                           "loop_us": {"min": min(tl), "median": medl, "max": max(tl)},
                           "loop_in_c_us": {"min": min(t1), "median": med1, "max": max(t1)},
                           "loop_over_batched": medl / medb, "loop_in_c_over_batched": med1 / medb,
                           "batched_us_per_member": medb / batch, "loop_us_per_member": medl / batch, "loop_in_c_us_per_member": med1 / batch,
                           "batched_TOPS": 2.0 * M * N * K * batch / (medb * 1e-6) / 1e12, "rounds": a.rounds, "iters": a.iters}
                    # the condition this tool checks: the one-launch form is not slower than the loop, however the loop is issued
                    rec["not_slower_than_loop"] = bool(medb <= medl and medb <= med1)
                    slower += 0 if rec["not_slower_than_loop"] else 1
                    line = json.dumps(rec)
                    print(line, flush=True)
                    if out:
                        out.write(line + "\n")
                        out.flush()
                    for p in (dA, dB, bA, bB, bC, lA, lB, lC, hC[0], hC[1]):
                        ctx.free(p)
                    bp.close()
                    pp.close()
    if slower:
        print(f"{slower} point(s) where the one-launch form is slower than the loop", file=sys.stderr)
    return 1 if slower else 0


if __name__ == "__main__":
    sys.exit(main())
