#!/usr/bin/env python3
"""Element-wise chains on batched plans: the two block-diagonal forms against the host loop they replace and against the GEMM alone.

Everything runs in ONE process on one context and stream, on operands packed once from the same host data; HIP events around
`iters` back-to-back executions; every arm is warmed up first, then `rounds` rounds in which the arms alternate.  Before anything is
timed, D of every arm is compared byte for byte, member by member.
  L  a host loop of qgemul_execute_ep over the members on ONE plain plan with the chain: each member its own packed A, B, D, its own
     or the shared packed bias.  That code is what the library offered before the batched chain existed: the "before".  Issued
     from Python; "L_in_c" prices the same launches issued from C (qgemul_time_execute_ep on one member, times the member count)
  G  qgemul_execute_batched on a batched plan WITHOUT a chain: the GEMM alone, the floor
  P  the pass form: the block-diagonal launch into the plan's packed C, then one block-diagonal pass over the stack (2 launches)
  F  the fused form: the chain in the block-diagonal launch's epilogue (1 launch, QG_OPT_FUSED_EPILOGUE); 32-bit chains without
     an APPROX stage only, so chain "scale_bias" only
Workloads: 256 and 1024 members of 64^3, int<4,3> and int<8,8> operands into a 16-bit C (a fused chain needs 32-bit arithmetic);
chain "scale_bias" = a scalar multiply and ONE shared 64 x 64 bias for all members, into C's own type; chain "scale_bias_act" = the
same into Qu<3,12> followed by an 8-segment degree-3 APPROX stage (the sigmoid table of tests/golden).
Prints one JSON line per (format, members, chain): microseconds per batch of every arm (min / median / max over the rounds).
The last line is the decision the planner's default rests on: "fused_faster_everywhere" is true only if F's maximum is below P's
minimum at all four (format, members) points of chain "scale_bias".
    python tools/measure_batched_ep.py [--members 256,1024] [--formats e43,e88] [--rounds 7] [--iters 20] [--out FILE]
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

C16 = Qu(7, 8)
FORMATS = {
    "e43": (Qu(4, 3), Qu(8, 6), dict(mul_args=Tags(9, 6), add_args=[Qu(19, 6)])),
    "e88": (Qu(8, 8), C16, dict(mul_args=Tags(17, 16), add_args=[Qu(29, 16)])),
}
S34, B106 = Qu(3, 4), Qu(10, 6)


def chains(cq):
    x312, sigmoid = R.case_table(next(j for j in R.cases() if j["name"] == "uniform_sigmoid_8x_degree3"))
    return {
        "scale_bias": ([Ew("mul", S34, scalar=True), Ew("add", B106)], cq),
        "scale_bias_act": ([Ew("mul", S34, Tags(24, 8), scalar=True, into=Qu(24, 8)), Ew("add", B106, into=x312), Approx(sigmoid)],
                           Qu(1, 10, True, RND.CONV, SAT.TCPL)),
    }


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--members", default="256,1024")
    ap.add_argument("--formats", default="e43,e88")
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    assert a.rounds >= 5
    out = open(a.out, "a") if a.out else None
    rng = np.random.default_rng(11)
    hip = C.CDLL("libamdhip64.so")
    M = N = K = 64
    n = M * N
    decisive = []

    def emit(rec):
        line = json.dumps(rec)
        print(line, flush=True)
        if out:
            out.write(line + "\n")
            out.flush()

    with capi.Context() as ctx:
        for fmt in a.formats.split(","):
            e, ec, kw = FORMATS[fmt]
            d = lower(e, e, ec, M, N, K, **kw)
            for batch in [int(x) for x in a.members.split(",")]:
                A = rng.integers(e.raw_min, e.raw_max + 1, size=batch * M * K, dtype=np.int32)
                B = rng.integers(e.raw_min, e.raw_max + 1, size=batch * K * N, dtype=np.int32)
                # a scale of 1/16 and a bias inside (-2, 2): the activation's input then covers its whole range instead of saturating
                bias = rng.integers(-128, 129, size=n, dtype=np.int32)
                scale = 1
                dA, dB, dE = ctx.alloc(A.nbytes), ctx.alloc(B.nbytes), ctx.alloc(bias.nbytes)
                ctx.h2d(dA, A)
                ctx.h2d(dB, B)
                ctx.h2d(dE, bias)
                for cname, (stages, dq) in chains(ec).items():
                    ep, tabs = lower_epilogue_x(ec, stages, dq)
                    shared = [0, 1, 0][:len(stages)]
                    fusable = cname == "scale_bias"
                    gp = capi.BatchedPlan(ctx, d, batch)
                    plans = {"P": capi.BatchedPlan(ctx, d, batch, capi.OPT_UNFUSED_EPILOGUE, ep=ep, approx=tabs, shared=shared)}
                    if fusable:
                        plans["F"] = capi.BatchedPlan(ctx, d, batch, capi.OPT_FUSED_EPILOGUE, ep=ep, approx=tabs, shared=shared)
                        assert plans["F"].fuses == 1 and plans["F"].launches == 1
                    assert plans["P"].fuses == 0 and plans["P"].launches == 2 and gp.launches == 1
                    pp = capi.Plan(ctx, d, epilogue=ep, approx=tabs)
                    hb = pp.info.host_elem_bytes
                    mb = [(x + 255) // 256 * 256 for x in pp.info.packed_bytes]
                    frees = [dA, dB, dE] if cname == list(chains(ec))[-1] else []
                    # the batched arms share the stack's packed A and B (one layout for every batched plan of this descriptor)
                    bb = plans["P"].info.packed_bytes
                    assert list(gp.info.packed_bytes)[:2] == list(bb)[:2]
                    bA, bB = ctx.alloc(bb[0]), ctx.alloc(bb[1])
                    gp.pack(capi.OPERAND_A, dA, bA, M * K)
                    gp.pack(capi.OPERAND_B, dB, bB, K * N)
                    gC = ctx.alloc(gp.info.packed_bytes[2])
                    bD = {k: ctx.alloc(bb[2]) for k in plans}
                    bE = ctx.alloc(plans["P"].packed_e_bytes(1))
                    plans["P"].pack_e(1, dE, bE, 0)                       # ONE member's bytes: the shared bias is not replicated
                    bargs = capi.Plan.ep_args(packed=[0, bE], scalars=[scale, 0])
                    lA, lB, lD = ctx.alloc(batch * mb[0]), ctx.alloc(batch * mb[1]), ctx.alloc(batch * mb[2])
                    lE = ctx.alloc(pp.packed_e_bytes(1))
                    pp.pack_e(1, dE, lE)
                    largs = capi.Plan.ep_args(packed=[0, lE], scalars=[scale, 0])
                    for b in range(batch):
                        pp.pack(capi.OPERAND_A, dA + b * M * K * hb[0], lA + b * mb[0])
                        pp.pack(capi.OPERAND_B, dB + b * K * N * hb[1], lB + b * mb[1])
                    frees += [bA, bB, gC, bE, lA, lB, lD, lE] + list(bD.values())

                    def loop():
                        for b in range(batch):
                            pp.execute_ep(lD + b * mb[2], lA + b * mb[0], lB + b * mb[1], largs)

                    # every arm computes the same bytes
                    hD = ctx.alloc(batch * n * hb[2])
                    frees.append(hD)
                    loop()
                    for b in range(batch):
                        pp.unpack_c(lD + b * mb[2], hD + b * n * hb[2])
                    ctx.sync()
                    want = np.zeros(batch * n * hb[2], dtype=np.uint8)
                    ctx.d2h(want, hD)
                    assert len(set(want[:4096].tolist())) > 8                  # (the comparison is not hidden by saturation)
                    for k, p in plans.items():
                        p.execute_ep(bD[k], bA, bB, bargs)
                        p.unpack_c(bD[k], hD, n)
                        ctx.sync()
                        got = np.zeros_like(want)
                        ctx.d2h(got, hD)
                        assert got.tobytes() == want.tobytes(), (fmt, batch, cname, k)

                    def time_loop(warm, iters):
                        """HIP events on the context's stream around iters x members qgemul_execute_ep calls; ms per batch"""
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

                    arms = {"G": lambda it: gp.time_execute(gC, bA, bB, 2, it)}
                    for k, p in plans.items():
                        arms[k] = (lambda p, k: lambda it: p.time_execute_ep(bD[k], bA, bB, bargs, 2, it))(p, k)
                    arms["L"] = lambda it: time_loop(1, max(2, it // 4))
                    arms["L_in_c"] = lambda it: pp.time_execute_ep(lD, lA, lB, largs, 2, it * 8) * batch
                    for f in arms.values():                               # warm-up of every arm: clocks, code objects
                        f(4)
                    t = {k: [] for k in arms}
                    for _ in range(a.rounds):
                        for k, f in arms.items():
                            t[k].append(f(a.iters) * 1e3)
                    rec = {"format": fmt, "M": M, "N": N, "K": K, "members": batch, "chain": cname, "C": list(ec.as_tuple()), "D": list(dq.as_tuple()),
                           "rounds": a.rounds, "iters": a.iters}
                    for k in arms:
                        rec[k + "_us"] = {"min": min(t[k]), "median": statistics.median(t[k]), "max": max(t[k])}
                    rec["L_over_P"] = rec["L_us"]["median"] / rec["P_us"]["median"]
                    rec["P_over_G"] = rec["P_us"]["median"] / rec["G_us"]["median"]
                    if fusable:
                        rec["F_over_G"] = rec["F_us"]["median"] / rec["G_us"]["median"]
                        rec["F_max_below_P_min"] = bool(rec["F_us"]["max"] < rec["P_us"]["min"])
                        decisive.append(rec["F_max_below_P_min"])
                    emit(rec)
                    for p in list(plans.values()) + [gp, pp]:
                        p.close()
                    for q in frees:
                        ctx.free(q)
    if decisive:
        emit({"decision": "default between the fused and the pass form for fusable chains", "points": len(decisive),
              "fused_faster_everywhere": bool(len(decisive) == 4 and all(decisive)),
              "rule": "fused becomes the default only if F's maximum is below P's minimum at all four (format, members) points"})
    return 0


if __name__ == "__main__":
    sys.exit(main())
