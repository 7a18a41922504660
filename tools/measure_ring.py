#!/usr/bin/env python3
"""Kernel times of the ring plans (qg_mfma_ring.hip) against what they replace and against the nearest exact plans, one process,
event-timed (qgemul_time_execute), arms ALTERNATING over the rounds so that clock drift hits every arm alike:

  replace   2048^3 int32 / int16 / int8, default tags: the ring plan against QG_OPT_FORCE_TREE — the tree_i128 / tree_i64 / tree_i32
            plan the same descriptor had before (those kernels are unchanged), the factor the feature is about;
  yardstick 4096^3 int32 ring (10 products, two-stage LDS ring) against k_mfma16<3,3> (int<8,8>, QG_OPT_LOCKSTEP_TILES, 9 products),
            4096^3 int16 ring (3 products) against k_mfma16<2,2> (int<7,7>, 4 products), int24 (6 products) for the table;
  long_k    int8 ring at 4096^2 x 262 144 in ONE launch against the 3-chunk composite plan of the exact int<4,3> case;
  pack      int32 operands (4 planes, W = 31) through k_pack_limb32 and through the generic k_pack (QG_OPT_GENERIC_LAYOUT).

One JSON line per arm on stdout (and into --out); `--only NAME` runs one group, so that a rocprofv3 --kernel-trace --stats run can
wrap a short one.  Needs an MI355X."""
import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from qublas_amd import capi  # noqa: E402
from qublas_amd.desc import Qu, TRN, WRP, Tags, lower  # noqa: E402


def I(bits):
    return Qu(bits - 1, 0, True, TRN.TCPL, WRP.TCPL)


class Arm:
    def __init__(self, ctx, name, d, flags=0):
        self.name, self.d = name, d
        self.plan = capi.Plan(ctx, d, flags)
        info = self.plan.info
        pb = info.packed_bytes
        self.buf = [ctx.alloc(pb[0]), ctx.alloc(pb[1]), ctx.alloc(pb[2])]
        self.plan.fill(capi.OPERAND_A, 1, 0, self.buf[0])
        self.plan.fill(capi.OPERAND_B, 2, 0, self.buf[1])
        self.ctx = ctx
        self.ms = []
        self.kernel = capi.KERNEL_NAMES[info.kernel]
        self.reason = bytes(info.reason).split(b"\0")[0].decode()
        self.limbs = [info.limbs[0], info.limbs[1]]

    def round(self, warmup, iters):
        self.ms.append(self.plan.time_execute(self.buf[2], self.buf[0], self.buf[1], warmup, iters))

    def close(self):
        for p in self.buf:
            self.ctx.free(p)
        self.plan.close()

    def line(self, group):
        ms = sorted(self.ms)
        ops = 2.0 * self.d.M * self.d.N * self.d.K
        return {"group": group, "arm": self.name, "shape": [self.d.M, self.d.N, self.d.K], "kernel": self.kernel, "reason": self.reason,
                "limbs": self.limbs, "rounds_ms": [round(x, 5) for x in self.ms], "median_ms": ms[len(ms) // 2], "min_ms": ms[0],
                "tops_at_median": ops / (ms[len(ms) // 2] * 1e-3) / 1e12}


def run_group(ctx, group, arms, rounds, warmup, iters, out):
    for _ in range(rounds):
        for a in arms:
            a.round(warmup, iters)
    lines = [a.line(group) for a in arms]
    for ln in lines:
        ln["ratio_to_first_arm"] = ln["median_ms"] / lines[0]["median_ms"]
        s = json.dumps(ln)
        print(s, flush=True)
        if out:
            out.write(s + "\n")
            out.flush()
    for a in arms:
        a.close()


def time_pack(ctx, d, flags, reps=20):
    import numpy as np
    plan = capi.Plan(ctx, d, flags)
    host = np.random.default_rng(1).integers(-(1 << 31), 1 << 31, d.M * d.K, dtype=np.int64).astype(np.int32)
    src, dst = ctx.alloc(host.nbytes), ctx.alloc(int(plan.info.packed_bytes[0]))
    ctx.h2d(src, host)
    for _ in range(3):
        plan.pack(capi.OPERAND_A, src, dst)
    ctx.sync()
    t0 = time.perf_counter()
    for _ in range(reps):
        plan.pack(capi.OPERAND_A, src, dst)
    ctx.sync()
    ms = (time.perf_counter() - t0) * 1e3 / reps
    ctx.free(src)
    ctx.free(dst)
    plan.close()
    return ms, host.nbytes


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--only", default="")
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--out", default="")
    args = ap.parse_args()
    out = open(args.out, "a") if args.out else None
    want = lambda g: not args.only or args.only == g
    E88, E77, E43 = Qu(8, 8), Qu(7, 7), Qu(4, 3)
    with capi.Context() as ctx:
        if want("replace"):
            for bits in (32, 16, 8):
                d = lower(I(bits), I(bits), I(bits), 2048, 2048, 2048)
                slow = bits == 32   # tree_i128: 50 ms a launch
                run_group(ctx, "replace_int%d_2048" % bits, [Arm(ctx, "ring", d), Arm(ctx, "forced tree (the plan before)", d, capi.OPT_FORCE_TREE)],
                          args.rounds, 2 if slow else 5, 3 if slow else 20, out)
        if want("yardstick"):
            S = 4096
            d33 = lower(E88, E88, Qu(29, 16), S, S, S, mul_args=Tags(17, 16), add_args=[Qu(29, 16)])
            d22 = lower(E77, E77, Qu(27, 14), S, S, S, mul_args=Tags(15, 14), add_args=[Qu(27, 14)])
            run_group(ctx, "yardstick_int32_4096", [Arm(ctx, "k_mfma16<3,3> int<8,8> lock-step, 9 products", d33, capi.OPT_LOCKSTEP_TILES),
                                                    Arm(ctx, "ring int32, 10 products", lower(I(32), I(32), I(32), S, S, S)),
                                                    Arm(ctx, "ring int24, 6 products", lower(I(24), I(24), I(24), S, S, S))], args.rounds, 10, 30, out)
            run_group(ctx, "yardstick_int16_4096", [Arm(ctx, "k_mfma16<2,2> int<7,7> lock-step, 4 products", d22, capi.OPT_LOCKSTEP_TILES),
                                                    Arm(ctx, "ring int16, 3 products", lower(I(16), I(16), I(16), S, S, S)),
                                                    Arm(ctx, "ring int8, 1 product", lower(I(8), I(8), I(8), S, S, S))], args.rounds, 10, 30, out)
        if want("long_k"):
            K = 262144
            dc = lower(E43, E43, Qu(27, 6), 4096, 4096, K, mul_args=Tags(9, 6), add_args=[Qu(27, 6)])
            run_group(ctx, "long_k_int8_4096x4096x262144", [Arm(ctx, "composite int<4,3>, 3 k-chunks", dc), Arm(ctx, "ring int8, one launch", lower(I(8), I(8), I(8), 4096, 4096, K))],
                      3, 1, 3, out)
        if want("pack"):
            d = lower(I(32), I(32), I(32), 4096, 4096, 4096)
            for name, flags in (("k_pack_limb32", 0), ("k_pack (generic)", capi.OPT_GENERIC_LAYOUT)):
                ms, nbytes = time_pack(ctx, d, flags)
                ln = {"group": "pack_int32_4096x4096", "arm": name, "ms": ms, "host_GB_per_s": nbytes / (ms * 1e-3) / 1e9}
                print(json.dumps(ln), flush=True)
                if out:
                    out.write(json.dumps(ln) + "\n")


if __name__ == "__main__":
    main()
