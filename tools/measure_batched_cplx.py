#!/usr/bin/env python3
"""Batched complex and real x complex Qgemul: the stacked form (QG_OPT_BATCHED_STACKED: one block-diagonal MFMA launch + one combine
pass for the whole batch) against the path the library takes without the flag.

All arms run in ONE process on the same context and stream, on operands packed once from the same host data, HIP events around `iters`
back-to-back executions issued from C (qgemul_time_execute*), a warm-up of every arm first, then `rounds` rounds in which the arms
alternate; the stacked arm's result is compared with the baseline's, member by member and byte for byte, before anything is timed.
  stacked   qgemul_time_execute_batched on the flagged plan: 2 launches per batch
  baseline  complex members: qgemul_time_execute_batched on the SAME descriptor's plan without the flag — member by member, one MFMA launch
            and one k_cplx_combine launch each (2 x members launches), issued from C.  Mixed members: a batched plan refuses them
            without the flag, so the baseline is what a caller had: qgemul_time_execute on ONE member's plain plan (MFMA launch +
            k_rc_convert, back to back from C) times the member count
  gemm      launch 0 of the flagged plan alone (qgemul_time_execute_batched_launch), and launch 1, the combine pass, alone: its share of
            the two-launch time is combine / (gemm + combine)
Points: complex (cc) and mixed (ra: real x complex, rb: complex x real) members of 64^3, 128^3 and 256 x 256 x 64 at 256 and 1024
members, in the 1-, 2- and 3-limb formats of tests/stacked_cases.py.  Prints one JSON line per point: microseconds per batch of every arm
(min / median / max over the rounds), baseline / stacked of the medians (above 1: the stacked form is faster), the combine pass's share,
and the workspace's size.  No threshold: the tool reports.
    python tools/measure_batched_cplx.py [--members 256,1024] [--shapes 64x64x64,128x128x128,256x256x64] [--kinds cc,ra,rb] [--limbs 1,2,3]
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
sys.path.insert(0, os.path.join(ROOT, "tests"))
from qublas_amd import capi  # noqa: E402
from qublas_amd.desc import Qcomplex, lower  # noqa: E402
from stacked_cases import COMPLEX, LINEAR  # noqa: E402

F = capi.OPT_BATCHED_STACKED


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
    ap.add_argument("--kinds", default="cc,ra,rb")
    ap.add_argument("--limbs", default="1,2,3")
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    out = open(a.out, "a") if a.out else None
    rng = np.random.default_rng(13)
    with capi.Context() as ctx:
        for kind in a.kinds.split(","):
            for limbs in a.limbs.split(","):
                if kind == "cc":
                    e, ec, kw = COMPLEX["limb" + limbs]
                    ea = eb = e
                else:
                    er, ez, ec, kw = LINEAR["limb" + limbs]
                    ea, eb = (er, ez) if kind == "ra" else (ez, er)
                for shape in a.shapes.split(","):
                    M, N, K = (int(x) for x in shape.split("x"))
                    d = lower(ea, eb, ec, M, N, K, **kw)
                    for batch in [int(x) for x in a.members.split(",")]:
                        sp, pp = capi.BatchedPlan(ctx, d, batch, F), capi.Plan(ctx, d)
                        up = capi.BatchedPlan(ctx, d, batch) if kind == "cc" else None   # (mixed: refused without the flag)
                        assert sp.launches == 2 and (up is None or up.launches == 2 * batch)
                        hb = pp.info.host_elem_bytes
                        A, B = host(rng, ea, batch * M * K), host(rng, eb, batch * K * N)
                        dA, dB = ctx.alloc(A.nbytes), ctx.alloc(B.nbytes)
                        ctx.h2d(dA, A)
                        ctx.h2d(dB, B)
                        sb = sp.info.packed_bytes
                        mb = [(x + 255) // 256 * 256 for x in pp.info.packed_bytes]   # the member step of the unflagged batched plan
                        sA, sB, sC = ctx.alloc(sb[0]), ctx.alloc(sb[1]), ctx.alloc(sb[2])
                        lA, lB, lC = ctx.alloc(batch * mb[0]), ctx.alloc(batch * mb[1]), ctx.alloc(batch * mb[2])
                        hC = [ctx.alloc(batch * M * N * hb[2]) for _ in range(2)]
                        sp.pack(capi.OPERAND_A, dA, sA, M * K)
                        sp.pack(capi.OPERAND_B, dB, sB, K * N)
                        for b in range(batch):
                            pp.pack(capi.OPERAND_A, dA + b * M * K * hb[0], lA + b * mb[0])
                            pp.pack(capi.OPERAND_B, dB + b * K * N * hb[1], lB + b * mb[1])
                        # the arms compute the same bytes
                        sp.execute(sC, sA, sB)
                        sp.unpack_c(sC, hC[0], M * N)
                        if up is not None:
                            up.execute(lC, lA, lB)
                            up.unpack_c(lC, hC[1], M * N)
                        else:
                            for b in range(batch):
                                pp.execute(lC + b * mb[2], lA + b * mb[0], lB + b * mb[1])
                                pp.unpack_c(lC + b * mb[2], hC[1] + b * M * N * hb[2])
                        ctx.sync()
                        got = [np.zeros(batch * M * N * hb[2], dtype=np.uint8) for _ in range(2)]
                        ctx.d2h(got[0], hC[0])
                        ctx.d2h(got[1], hC[1])
                        assert got[0].tobytes() == got[1].tobytes(), (kind, limbs, shape, batch)
                        assert len(set(got[0][:4096].tolist())) > 8

                        def baseline(iters):
                            if up is not None:
                                return up.time_execute(lC, lA, lB, 1, max(2, iters // 4)) * 1e3
                            return pp.time_execute(lC, lA, lB, 2, iters * 8) * 1e3 * batch
                        sp.time_execute(sC, sA, sB, 5, 5)
                        baseline(a.iters)
                        ts, tb, tg, tc = [], [], [], []
                        for _ in range(a.rounds):
                            ts.append(sp.time_execute(sC, sA, sB, 2, a.iters) * 1e3)
                            tb.append(baseline(a.iters))
                            tg.append(sp.time_execute_launch(sC, sA, sB, 0, 2, a.iters) * 1e3)
                            tc.append(sp.time_execute_launch(sC, sA, sB, 1, 2, a.iters) * 1e3)
                        med = statistics.median
                        mmm = lambda t: {"min": min(t), "median": med(t), "max": max(t)}
                        rec = {"kind": kind, "limbs": int(limbs), "M": M, "N": N, "K": K, "members": batch, "reason": bytes(sp.info.reason).decode(),
                               "baseline": "unflagged batched plan (member by member, from C)" if up is not None else "one member's plain plan from C x members",
                               "launches_stacked": sp.launches, "launches_baseline": 2 * batch,
                               "stacked_us": mmm(ts), "baseline_us": mmm(tb), "gemm_launch_us": mmm(tg), "combine_launch_us": mmm(tc),
                               "baseline_over_stacked": med(tb) / med(ts), "baseline_over_stacked_range": [min(tb) / max(ts), max(tb) / min(ts)],
                               "combine_share": med(tc) / (med(tg) + med(tc)),
                               # (64 x 64 int64 tiles: the parts of A times those of B per part tile of a member)
                               "workspace_MiB": batch * (2 if kind != "ra" else 1) * ((M + 63) // 64) * (2 if kind != "rb" else 1) * ((N + 63) // 64) * 32768 / 2 ** 20,
                               "rounds": a.rounds, "iters": a.iters}
                        line = json.dumps(rec)
                        print(line, flush=True)
                        if out:
                            out.write(line + "\n")
                            out.flush()
                        for p in (dA, dB, sA, sB, sC, lA, lB, lC, hC[0], hC[1]):
                            ctx.free(p)
                        sp.close()
                        pp.close()
                        if up is not None:
                            up.close()
    return 0


if __name__ == "__main__":
    sys.exit(main())
