#!/usr/bin/env python3
"""Element-wise chains on grouped plans: the two grouped forms against the host loop they replace and against the grouped GEMM alone.

Everything runs in ONE process on one context and stream, on operands packed once from the same host data; every arm is warmed up
first, then `rounds` rounds in which the arms alternate (the method of tools/measure_batched_ep.py).  Before anything is timed, D of
every arm is compared byte for byte, member by member.
  L  (a) a host loop of qgemul_execute_ep over plain plans with the chain, one plan per distinct shape, every member with its own
     packed A, B, bias and D and its own scale: what the library offered before grouped chains existed, the "was".  Issued from
     Python, HIP events around the loop; "L_in_c" prices the same launches issued from C (the sum of qgemul_time_execute_ep over
     the members)
  G  (b) qgemul_execute_grouped on a grouped plan WITHOUT a chain: the GEMMs alone, the floor
  P  (c) the pass form: the grouped launch into the plan's packed C, then one pass over its tiles (2 launches)
  F  (d) the fused form: the chain in the grouped launch's epilogue (1 launch, QG_OPT_FUSED_EPILOGUE); 32-bit chains without an
     APPROX stage only, so chain "scale_bias" only
Workloads: the 256- and 1024-member random sets and the skewed set of tools/measure_grouped.py (same seeds), int<4,3> and int<8,8>
operands into a 16-bit C.  Chain "scale_bias" = a per-member scalar multiply and a per-member bias tensor, into C's own type; chain
"scale_bias_act" = the same into Qu<3,12> followed by the 8-segment degree-3 APPROX stage (the sigmoid table of tests/golden).
Prints one JSON line per (format, workload, chain): microseconds per group of every arm (min / median / max over the rounds).  The
last line is the decision the planner's default rests on: "fused_faster_everywhere" is true only if F's maximum is below P's
minimum at every measured (format, workload) point of chain "scale_bias".
    python tools/measure_grouped_ep.py [--workloads random_256,random_1024,skewed_1024] [--formats e43,e88] [--rounds 5] [--iters 10] [--out FILE]
Needs an MI355X."""
import argparse
import ctypes as C
import json
import os
import statistics
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import approx_ref as R  # noqa: E402
from qublas_amd import capi  # noqa: E402
from qublas_amd.desc import Approx, Ew, Qu, RND, SAT, Tags, lower, lower_epilogue_x  # noqa: E402

FORMATS = {
    "e43": (Qu(4, 3), Qu(9, 6), dict(mul_args=Tags(9, 6), add_args=[Qu(21, 6)])),     # (the level type holds K = 4096 products exactly)
    "e88": (Qu(8, 8), Qu(7, 8), dict(mul_args=Tags(17, 16), add_args=[Qu(29, 16)])),
}
S34, B106 = Qu(3, 4), Qu(10, 6)


def chains(cq):
    x312, sigmoid = R.case_table(next(j for j in R.cases() if j["name"] == "uniform_sigmoid_8x_degree3"))
    return {
        "scale_bias": ([Ew("mul", S34, scalar=True), Ew("add", B106)], cq),
        "scale_bias_act": ([Ew("mul", S34, Tags(24, 8), scalar=True, into=Qu(24, 8)), Ew("add", B106, into=x312), Approx(sigmoid)],
                           Qu(1, 10, True, RND.CONV, SAT.TCPL)),
    }


def workloads():
    """the sets of tools/measure_grouped.py, same seed"""
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


def measure(ctx, ev, fmt, name, shapes, cname, a, rng):
    e, ec, kw = FORMATS[fmt]
    stages, dq = chains(ec)[cname]
    ep, tabs = lower_epilogue_x(ec, stages, dq)
    pm = [1, 0, 0][:len(stages)]
    fusable = cname == "scale_bias"
    n = len(shapes)
    descs = [lower(e, e, ec, M, N, K, **kw) for M, N, K in shapes]
    hostA = [rng.integers(e.raw_min, e.raw_max + 1, size=M * K, dtype=np.int32) for M, N, K in shapes]
    hostB = [rng.integers(e.raw_min, e.raw_max + 1, size=K * N, dtype=np.int32) for M, N, K in shapes]
    hostE = [rng.integers(-128, 129, size=M * N, dtype=np.int32) for M, N, K in shapes]
    scales = [int(x) for x in rng.integers(1, 9, size=n)]
    off = [np.concatenate([[0], np.cumsum([up256(x.nbytes) for x in h])]).tolist() for h in (hostA, hostB, hostE)]
    frees = []

    def alloc(nbytes):
        frees.append(ctx.alloc(max(16, int(nbytes))))
        return frees[-1]

    dA, dB, dE = alloc(off[0][-1]), alloc(off[1][-1]), alloc(off[2][-1])
    for g in range(n):
        ctx.h2d(dA + off[0][g], hostA[g])
        ctx.h2d(dB + off[1][g], hostB[g])
        ctx.h2d(dE + off[2][g], hostE[g])
    ptr = lambda base, o: [base + o[g] for g in range(n)]
    # (a) plain plans with the chain, one per distinct shape
    plans = {}
    for s, d in zip(shapes, descs):
        if s not in plans:
            plans[s] = capi.Plan(ctx, d, epilogue=ep, approx=tabs)
    de = plans[shapes[0]].info.host_elem_bytes[2]
    offD = np.concatenate([[0], np.cumsum([up256(M * N * de) for M, N, K in shapes])]).tolist()
    dD1, dD2 = alloc(offD[-1]), alloc(offD[-1])
    lo = [[0], [0], [0], [0]]
    for s in shapes:
        for w in range(3):
            lo[w].append(lo[w][-1] + up256(plans[s].info.packed_bytes[w]))
        lo[3].append(lo[3][-1] + up256(plans[s].packed_e_bytes(1)))
    lA, lB, lD, lE = alloc(lo[0][-1]), alloc(lo[1][-1]), alloc(lo[2][-1]), alloc(lo[3][-1])
    largs = []
    for g, s in enumerate(shapes):
        plans[s].pack(capi.OPERAND_A, dA + off[0][g], lA + lo[0][g])
        plans[s].pack(capi.OPERAND_B, dB + off[1][g], lB + lo[1][g])
        plans[s].pack_e(1, dE + off[2][g], lE + lo[3][g])
        largs.append(capi.Plan.ep_args(packed=[0, lE + lo[3][g], 0][:len(stages)], scalars=[scales[g], 0, 0][:len(stages)]))

    def loop():
        for g, s in enumerate(shapes):
            plans[s].execute_ep(lD + lo[2][g], lA + lo[0][g], lB + lo[1][g], largs[g])

    loop()
    for g, s in enumerate(shapes):
        plans[s].unpack_c(lD + lo[2][g], dD1 + offD[g])
    ctx.sync()
    ref = np.zeros(offD[-1], dtype=np.uint8)
    ctx.d2h(ref, dD1)
    # (full-range operands at K up to 4096 saturate a 16-bit C, as they do in tools/measure_grouped.py's sets; the per-member bias keeps
    # D of "scale_bias" varied, so that chain's comparison is not hidden by saturation; behind the activation D is mostly 0 or 1, and
    # the comparison of that chain rests on tests/test_gpu_grouped_ep.py)
    assert len(set(ref[:65536].tolist())) > (8 if fusable else 1)
    # (b) the grouped GEMM alone; (c), (d) the grouped chain in either form: the same bytes as the loop, member by member
    gp = capi.GroupedPlan(ctx, descs)
    arms = {"P": capi.GroupedPlan(ctx, descs, capi.OPT_UNFUSED_EPILOGUE, ep=ep, approx=tabs, per_member=pm)}
    if fusable:
        arms["F"] = capi.GroupedPlan(ctx, descs, capi.OPT_FUSED_EPILOGUE, ep=ep, approx=tabs, per_member=pm)
        assert arms["F"].fuses() == 1 and arms["F"].launches == 1, arms["F"].info.reason
    assert arms["P"].fuses() == 0 and arms["P"].launches == 2 and gp.launches == 1, arms["P"].info.reason
    pb = arms["P"].info.packed_bytes
    assert list(gp.info.packed_bytes)[:2] == list(pb)[:2]                       # one layout of A and B for every grouped plan of this list
    bA, bB, gC, bE = alloc(pb[0]), alloc(pb[1]), alloc(gp.info.packed_bytes[2]), alloc(arms["P"].packed_e_bytes(1))
    gp.pack(capi.OPERAND_A, ptr(dA, off[0]), bA)
    gp.pack(capi.OPERAND_B, ptr(dB, off[1]), bB)
    arms["P"].pack_e(1, ptr(dE, off[2]), bE)
    bargs = capi.Plan.ep_args(packed=[0, bE, 0][:len(stages)], scalars=[0, 0, 0][:len(stages)])
    bD = {}
    for k, p in arms.items():
        p.set_scalars(0, scales)
        bD[k] = alloc(pb[2])
        p.execute_ep(bD[k], bA, bB, bargs)
        ctx.h2d(dD2, np.zeros(offD[-1], dtype=np.uint8))
        p.unpack_c(bD[k], ptr(dD2, offD))
        ctx.sync()
        got = np.zeros(offD[-1], dtype=np.uint8)
        ctx.d2h(got, dD2)
        for g, (M, N, K) in enumerate(shapes):
            assert got[offD[g]:offD[g] + M * N * de].tobytes() == ref[offD[g]:offD[g] + M * N * de].tobytes(), (fmt, name, cname, k, g)
    timers = {"G": lambda it: gp.time_execute(gC, bA, bB, 2, it)}
    for k, p in arms.items():
        timers[k] = (lambda p, k: lambda it: p.time_execute_ep(bD[k], bA, bB, bargs, 2, it))(p, k)
    timers["L"] = lambda it: ev.time(loop, 0, 2)
    timers["L_in_c"] = lambda it: sum(plans[s].time_execute_ep(lD + lo[2][g], lA + lo[0][g], lB + lo[1][g], largs[g], 1, 4) for g, s in enumerate(shapes))
    for k, f in timers.items():                                                 # warm-up of every arm: clocks, code objects
        f(3)
    t = {k: [] for k in timers}
    for _ in range(a.rounds):
        for k, f in timers.items():
            t[k].append(f(a.iters) * 1e3)
    rec = {"format": fmt, "workload": name, "members": n, "distinct_shapes": len(plans), "chain": cname, "C": list(ec.as_tuple()), "D": list(dq.as_tuple()),
           "reason_P": bytes(arms["P"].info.reason).split(b"\0")[0].decode(), "rounds": a.rounds, "iters": a.iters}
    for k in timers:
        rec[k + "_us"] = stats(t[k])
    rec["L_over_P"] = rec["L_us"]["median"] / rec["P_us"]["median"]
    rec["L_in_c_over_P"] = rec["L_in_c_us"]["median"] / rec["P_us"]["median"]
    rec["P_over_G"] = rec["P_us"]["median"] / rec["G_us"]["median"]
    if fusable:
        rec["F_over_G"] = rec["F_us"]["median"] / rec["G_us"]["median"]
        rec["F_max_below_P_min"] = bool(rec["F_us"]["max"] < rec["P_us"]["min"])
    for p in list(arms.values()) + [gp] + list(plans.values()):
        p.close()
    for q in frees:
        ctx.free(q)
    return rec


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--workloads", default="random_256,random_1024,skewed_1024")
    ap.add_argument("--formats", default="e43,e88")
    ap.add_argument("--chains", default="scale_bias,scale_bias_act")
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    assert a.rounds >= 5
    out = open(a.out, "a") if a.out else None
    rng = np.random.default_rng(12)
    decisive = []

    def emit(rec):
        line = json.dumps(rec)
        print(line, flush=True)
        if out:
            out.write(line + "\n")
            out.flush()

    sets = workloads()
    with capi.Context() as ctx:
        ev = Events(ctx)
        for fmt in a.formats.split(","):
            for name in a.workloads.split(","):
                for cname in a.chains.split(","):
                    rec = measure(ctx, ev, fmt, name, sets[name], cname, a, rng)
                    if "F_max_below_P_min" in rec:
                        decisive.append(rec["F_max_below_P_min"])
                    emit(rec)
    if decisive:
        emit({"decision": "default between the fused and the pass form for fusable chains on grouped plans", "points": len(decisive),
              "fused_faster_everywhere": bool(all(decisive)),
              "rule": "fused becomes the default only if F's maximum is below P's minimum at every measured (format, workload) point"})
    return 0


if __name__ == "__main__":
    sys.exit(main())
