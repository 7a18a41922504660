#!/usr/bin/env python3
"""Grouped Qgemul: GEMMs of different shapes in one launch, against what a user could do before it existed.

All arms run in ONE process on the same context and stream, on operands packed once from the same host data, HIP events around
`iters` back-to-back executions, a warm-up of every arm first (clock, code objects), then `rounds` rounds in which the arms alternate;
the grouped arms' results are compared with the loop's, member by member, before anything is timed.
  loop      (a) one qgemul_execute per member on plain plans (one per distinct shape): the baseline.  Issued from Python with HIP
            events around the whole loop; "loop_in_c" prices the same launches issued from C (qgemul_time_execute per member, summed)
  padded    (b) a batched plan with every member padded to the group's largest M, N and K: the other thing a user could do.  Timed
            on operands of the padded size (skipped, and reported so, where its operands would exceed --padded-gib)
  dealt     (c) the grouped plan in dealt order (qg_grp.h), the default
  member    (d) the grouped plan in member order (the diagnostic library's QG_GRP_MEMBER_ORDER)
Workloads: 256 and 1024 members, int<4,3> and int<8,8>, shapes drawn with a fixed seed from M, N in [16, 256] and K in [64, 2048];
one skewed set of 1000 members of 32x32x64 plus 24 of 256x256x4096.  And the lookup cost of the schedule table: a group of IDENTICAL
64x64x64 members in dealt order against qgemul_execute_batched on the same members ("identical").
The rule for the order (fixed before anything was measured): dealt order stays the default unless member order's maximum is below
dealt order's minimum at every measured point; the last line printed says which.
    python tools/measure_grouped.py [--formats e43,e88] [--rounds 7] [--iters 10] [--padded-gib 12] [--out FILE]
Needs an MI355X and the diagnostic library (python -m qublas_amd.build --diag)."""
import argparse
import ctypes as C
import json
import os
import statistics
import sys

import numpy as np

os.environ.setdefault("QUBLAS_AMD_DIAG", "1")   # arm (d) exists in the diagnostic library only
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from qublas_amd import capi  # noqa: E402
from qublas_amd.desc import Qu, Tags, lower  # noqa: E402

FORMATS = {
    "e43": (Qu(4, 3), Qu(16, 3), dict(mul_args=Tags(9, 6), add_args=[Qu(21, 6)])),   # (the level type holds K = 4096 products exactly)
    "e88": (Qu(8, 8), Qu(24, 8), dict(mul_args=Tags(17, 16), add_args=[Qu(29, 16)])),
}


def workloads():
    rng = np.random.default_rng(2026)
    out = {}
    for n in (256, 1024):
        out[f"random_{n}"] = [(int(rng.integers(16, 257)), int(rng.integers(16, 257)), int(rng.integers(64, 2049))) for _ in range(n)]
    out["skewed_1024"] = [(32, 32, 64)] * 1000 + [(256, 256, 4096)] * 24
    return out


def up256(x):
    return (x + 255) // 256 * 256


def stats(v):
    return {"min": min(v), "median": statistics.median(v), "max": max(v)}


class Events:
    def __init__(self, ctx):
        self.hip = C.CDLL("libamdhip64.so")
        self.st = C.c_void_p(ctx.stream)

    def time(self, fn, warm, iters):
        """ms per call of fn, HIP events on the context's stream"""
        hip, e0, e1 = self.hip, C.c_void_p(), C.c_void_p()
        assert hip.hipEventCreate(C.byref(e0)) == 0 and hip.hipEventCreate(C.byref(e1)) == 0
        for _ in range(warm):
            fn()
        assert hip.hipEventRecord(e0, self.st) == 0
        for _ in range(iters):
            fn()
        assert hip.hipEventRecord(e1, self.st) == 0 and hip.hipEventSynchronize(e1) == 0
        ms = C.c_float()
        assert hip.hipEventElapsedTime(C.byref(ms), e0, e1) == 0
        hip.hipEventDestroy(e0)
        hip.hipEventDestroy(e1)
        return ms.value / iters


def grouped_plan(ctx, descs, member_order):
    if member_order:
        os.environ["QG_GRP_MEMBER_ORDER"] = "1"
    try:
        return capi.GroupedPlan(ctx, descs)
    finally:
        os.environ.pop("QG_GRP_MEMBER_ORDER", None)


def measure(ctx, ev, fmt, name, shapes, a, rng):
    e, ec, kw = FORMATS[fmt]
    n = len(shapes)
    descs = [lower(e, e, ec, M, N, K, **kw) for M, N, K in shapes]
    # host data, one device buffer per operand, members at 256-byte-aligned offsets
    hostA = [rng.integers(e.raw_min, e.raw_max + 1, size=M * K, dtype=np.int32) for M, N, K in shapes]
    hostB = [rng.integers(e.raw_min, e.raw_max + 1, size=K * N, dtype=np.int32) for M, N, K in shapes]
    offA = np.concatenate([[0], np.cumsum([up256(x.nbytes) for x in hostA])]).tolist()
    offB = np.concatenate([[0], np.cumsum([up256(x.nbytes) for x in hostB])]).tolist()
    ce = capi.classify(descs[0]).host_elem_bytes[2]   # bytes of one host element of C (8 for int<8,8>'s Qu<24,8>)
    assert list(capi.classify(descs[0]).host_elem_bytes[:2]) == [4, 4]
    offC = np.concatenate([[0], np.cumsum([up256(M * N * ce) for M, N, K in shapes])]).tolist()
    dA, dB, dC1, dC2 = ctx.alloc(offA[-1]), ctx.alloc(offB[-1]), ctx.alloc(offC[-1]), ctx.alloc(offC[-1])
    frees = [dA, dB, dC1, dC2]
    for g in range(n):
        ctx.h2d(dA + offA[g], hostA[g])
        ctx.h2d(dB + offB[g], hostB[g])
    # (a) plain plans, one per distinct shape; every member has its own packed operands and its own packed C
    plans = {}
    for s, d in zip(shapes, descs):
        if s not in plans:
            plans[s] = capi.Plan(ctx, d)
    lo = [[0], [0], [0]]
    for s in shapes:
        for w in range(3):
            lo[w].append(lo[w][-1] + up256(plans[s].info.packed_bytes[w]))
    lA, lB, lC = ctx.alloc(lo[0][-1]), ctx.alloc(lo[1][-1]), ctx.alloc(lo[2][-1])
    frees += [lA, lB, lC]
    for g, s in enumerate(shapes):
        plans[s].pack(capi.OPERAND_A, dA + offA[g], lA + lo[0][g])
        plans[s].pack(capi.OPERAND_B, dB + offB[g], lB + lo[1][g])

    def loop():
        for g, s in enumerate(shapes):
            plans[s].execute(lC + lo[2][g], lA + lo[0][g], lB + lo[1][g])

    loop()
    for g, s in enumerate(shapes):
        plans[s].unpack_c(lC + lo[2][g], dC1 + offC[g])
    ctx.sync()
    ref = np.zeros(offC[-1], dtype=np.uint8)
    ctx.d2h(ref, dC1)
    assert len(set(ref[:4096].tolist())) > 8
    # (c), (d) the grouped plan in either order: the same bytes as the loop, member by member
    arms = {}
    for arm, member_order in (("dealt", False), ("member", True)):
        gp = grouped_plan(ctx, descs, member_order)
        pb = gp.info.packed_bytes
        bufs = [ctx.alloc(pb[0]), ctx.alloc(pb[1]), ctx.alloc(pb[2])]
        frees += bufs
        gp.pack(capi.OPERAND_A, [dA + offA[g] for g in range(n)], bufs[0])
        gp.pack(capi.OPERAND_B, [dB + offB[g] for g in range(n)], bufs[1])
        gp.execute(bufs[2], bufs[0], bufs[1])
        ctx.h2d(dC2, np.zeros(offC[-1], dtype=np.uint8))
        gp.unpack_c(bufs[2], [dC2 + offC[g] for g in range(n)])
        ctx.sync()
        got = np.zeros(offC[-1], dtype=np.uint8)
        ctx.d2h(got, dC2)
        for g, (M, N, K) in enumerate(shapes):
            assert got[offC[g]:offC[g] + M * N * ce].tobytes() == ref[offC[g]:offC[g] + M * N * ce].tobytes(), (fmt, name, arm, g)
        arms[arm] = (gp, bufs)
    # (b) the batched plan on the group's largest shape (timing only: operands of the padded size, the members' data in their corners)
    Mx, Nx, Kx = max(s[0] for s in shapes), max(s[1] for s in shapes), max(s[2] for s in shapes)
    dpad = lower(e, e, ec, Mx, Nx, Kx, **kw)
    padded = None
    pad_host = 4 * n * (Mx * Kx + Kx * Nx)
    st, pinfo = capi.classify_batched_status(dpad, n)
    if st == capi.QG_OK and pad_host + sum(pinfo.packed_bytes) <= a.padded_gib * (1 << 30):
        bp = capi.BatchedPlan(ctx, dpad, n)
        pA, pB = ctx.alloc(4 * n * Mx * Kx), ctx.alloc(4 * n * Kx * Nx)
        bufs = [ctx.alloc(x) for x in bp.info.packed_bytes]
        frees += [pA, pB] + bufs
        for g, (M, N, K) in enumerate(shapes):
            pa = np.zeros((Kx, Mx), dtype=np.int32)
            pa[:K, :M] = hostA[g].reshape(K, M)
            pbm = np.zeros((Nx, Kx), dtype=np.int32)
            pbm[:N, :K] = hostB[g].reshape(N, K)
            ctx.h2d(pA + 4 * g * Mx * Kx, pa.reshape(-1))
            ctx.h2d(pB + 4 * g * Kx * Nx, pbm.reshape(-1))
        bp.pack(capi.OPERAND_A, pA, bufs[0], Mx * Kx)
        bp.pack(capi.OPERAND_B, pB, bufs[1], Kx * Nx)
        padded = (bp, bufs)
    # timing: warm-up of every arm, then rounds with the arms alternating
    ev.time(loop, 1, 1)
    for gp, bufs in arms.values():
        gp.time_execute(bufs[2], bufs[0], bufs[1], 3, 3)
    if padded:
        padded[0].time_execute(padded[1][2], padded[1][0], padded[1][1], 2, 2)
    t = {"loop": [], "loop_in_c": [], "padded": [], "dealt": [], "member": []}
    for _ in range(a.rounds):
        for arm, (gp, bufs) in arms.items():
            t[arm].append(gp.time_execute(bufs[2], bufs[0], bufs[1], 2, a.iters) * 1e3)
        if padded:
            t["padded"].append(padded[0].time_execute(padded[1][2], padded[1][0], padded[1][1], 1, max(2, a.iters // 2)) * 1e3)
        t["loop"].append(ev.time(loop, 0, 2) * 1e3)
        t["loop_in_c"].append(sum(plans[s].time_execute(lC + lo[2][g], lA + lo[0][g], lB + lo[1][g], 1, 4) for g, s in enumerate(shapes)) * 1e3)
    ops = sum(2.0 * M * N * K for M, N, K in shapes)
    gp = arms["dealt"][0]
    rec = {"format": fmt, "workload": name, "members": n, "distinct_shapes": len(plans), "launches_grouped": gp.launches, "reason": bytes(gp.info.reason).decode(),
           "padded_shape": [Mx, Nx, Kx], "padded_launches": padded[0].launches if padded else None,
           "padded_note": None if padded else "skipped: the padded operands exceed --padded-gib",
           "loop_us": stats(t["loop"]), "loop_in_c_us": stats(t["loop_in_c"]), "padded_us": stats(t["padded"]) if padded else None,
           "dealt_us": stats(t["dealt"]), "member_us": stats(t["member"]),
           "loop_over_dealt": statistics.median(t["loop"]) / statistics.median(t["dealt"]),
           "loop_in_c_over_dealt": statistics.median(t["loop_in_c"]) / statistics.median(t["dealt"]),
           "padded_over_dealt": statistics.median(t["padded"]) / statistics.median(t["dealt"]) if padded else None,
           "member_order_max_below_dealt_min": bool(max(t["member"]) < min(t["dealt"])),
           "dealt_TOPS": ops / (statistics.median(t["dealt"]) * 1e-6) / 1e12, "rounds": a.rounds, "iters": a.iters}
    for gp, _ in arms.values():
        gp.close()
    if padded:
        padded[0].close()
    for p in plans.values():
        p.close()
    for p in frees:
        ctx.free(p)
    return rec


def measure_identical(ctx, fmt, n, a, rng):
    """the lookup cost: a group of identical members in dealt order against the batched plan's in-kernel division"""
    e, ec, kw = FORMATS[fmt]
    M = N = K = 64
    d = lower(e, e, ec, M, N, K, **kw)
    A = rng.integers(e.raw_min, e.raw_max + 1, size=n * M * K, dtype=np.int32)
    B = rng.integers(e.raw_min, e.raw_max + 1, size=n * K * N, dtype=np.int32)
    dA, dB = ctx.alloc(A.nbytes), ctx.alloc(B.nbytes)
    ctx.h2d(dA, A)
    ctx.h2d(dB, B)
    gp, bp = capi.GroupedPlan(ctx, [d] * n), capi.BatchedPlan(ctx, d, n)
    assert list(gp.info.packed_bytes) == list(bp.info.packed_bytes)
    gb = [ctx.alloc(x) for x in gp.info.packed_bytes]
    bb = [ctx.alloc(x) for x in bp.info.packed_bytes]
    gp.pack(capi.OPERAND_A, [dA + 4 * g * M * K for g in range(n)], gb[0])
    gp.pack(capi.OPERAND_B, [dB + 4 * g * K * N for g in range(n)], gb[1])
    bp.pack(capi.OPERAND_A, dA, bb[0], M * K)
    bp.pack(capi.OPERAND_B, dB, bb[1], K * N)
    gp.execute(gb[2], gb[0], gb[1])
    bp.execute(bb[2], bb[0], bb[1])
    ctx.sync()
    got = [np.zeros(gp.info.packed_bytes[2], dtype=np.uint8) for _ in range(2)]
    ctx.d2h(got[0], gb[2])
    ctx.d2h(got[1], bb[2])
    assert got[0].tobytes() == got[1].tobytes() and len(set(got[0][:4096].tolist())) > 8     # (packed C: the same layout in both)
    gp.time_execute(gb[2], gb[0], gb[1], 5, 5)
    bp.time_execute(bb[2], bb[0], bb[1], 5, 5)
    tg, tb = [], []
    for _ in range(a.rounds):
        tg.append(gp.time_execute(gb[2], gb[0], gb[1], 2, a.iters * 4) * 1e3)
        tb.append(bp.time_execute(bb[2], bb[0], bb[1], 2, a.iters * 4) * 1e3)
    rec = {"format": fmt, "workload": f"identical_{n}", "members": n, "M": M, "N": N, "K": K, "grouped_us": stats(tg), "batched_us": stats(tb),
           "grouped_over_batched": statistics.median(tg) / statistics.median(tb), "rounds": a.rounds, "iters": a.iters * 4}
    gp.close()
    bp.close()
    for p in [dA, dB] + gb + bb:
        ctx.free(p)
    return rec


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--formats", default="e43,e88")
    ap.add_argument("--workloads", default="random_256,random_1024,skewed_1024")
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--padded-gib", type=float, default=12.0)
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    out = open(a.out, "a") if a.out else None
    rng = np.random.default_rng(11)
    wl = workloads()
    recs = []

    def emit(rec):
        line = json.dumps(rec)
        print(line, flush=True)
        if out:
            out.write(line + "\n")
            out.flush()

    with capi.Context() as ctx:
        ev = Events(ctx)
        for fmt in a.formats.split(","):
            for name in a.workloads.split(","):
                recs.append(measure(ctx, ev, fmt, name, wl[name], a, rng))
                emit(recs[-1])
            for n in (256, 1024):
                emit(measure_identical(ctx, fmt, n, a, rng))
    switch = bool(recs) and all(r["member_order_max_below_dealt_min"] for r in recs)
    emit({"order_rule": "dealt order stays the default unless member order's maximum is below dealt order's minimum at every measured point",
          "member_order_wins_everywhere": switch, "default": "member" if switch else "dealt"})
    return 0


if __name__ == "__main__":
    sys.exit(main())
