#!/usr/bin/env python3
"""Qgemul of one real and one complex operand (QG_CMUL_REAL_A / QG_CMUL_REAL_B) against what a user had before it.

Workload: S x S x S (default 2048) with BASELINE configuration 5's element Qcomplex<int<6,3>, int<6,-3>> (RND::POS_INF, SAT::TCPL) as
the complex operand and its real part's format as the real one, with default tags (the tree class) and with wide tags (products and
levels that hold every value: the linear class).  Three arms per tag set, interleaved in one process over the rounds, HIP events on the
context's stream (qgemul_time_execute), synthetic operands filled on the device:
  mixed   the mixed plan (k_tree_rc; wide tags: one limb GEMM on the stacked operand + the two-product convert pass)
  padded  on the same build, the complex BasicComplexMul plan with the real operand zero-padded to a complex one: the device
          workaround of before (four multiplications per MAC, and not the reference's result)
  parts   the two REAL plans of the parts (real x B.real, real x B.imag, each with that part's product and level formats), timed
          one after the other and added: what a user who splits the planes by hand runs
Prints one JSON line per (order, arm, round) with the plan's kernel and reason and the provenance of qublas_amd/profmeta.py.
    python tools/measure_mixed.py [--size 2048] [--rounds 3] [--iters 10] [--orders ra,rb] [--tags default,wide] [--out profiles/mixed_measure.jsonl]
Needs an MI355X."""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from qublas_amd import capi, profmeta  # noqa: E402
from qublas_amd.desc import (BasicComplexMul, CMUL_NONE, CMUL_REAL_A, QGEMUL_ABI_VERSION, Qcomplex, Qu, RealComplexMul, RND, SAT, lower,  # noqa: E402
                             qgemul_desc)

DEFAULT_SIZE = 2048
R63 = Qu(6, 3, True, RND.POS_INF, SAT.TCPL)
C5 = Qcomplex(R63, Qu(6, -3, True, RND.POS_INF, SAT.TCPL))


def part_desc(d, p):
    """part p of a mixed descriptor as a real descriptor (what tests/mixed_ref.py checks the engine against)"""
    r = qgemul_desc()
    r.abi, r.transA, r.is_complex, r.cmul, r.flags = QGEMUL_ABI_VERSION, d.transA, 0, CMUL_NONE, d.flags
    r.M, r.N, r.K, r.n_levels = d.M, d.N, d.K, d.n_levels
    r.a[0] = r.a[1] = d.a[0] if d.cmul == CMUL_REAL_A else d.a[p]
    r.b[0] = r.b[1] = d.b[p] if d.cmul == CMUL_REAL_A else d.b[0]
    r.c[0] = r.c[1] = d.c[p]
    r.mul[0] = d.mul[p]
    for l in range(d.n_levels):
        r.level_add[0][l] = r.level_add[1][l] = d.level_add[p][l]
        r.level[0][l] = r.level[1][l] = d.level[p][l]
    return r


def wide_descs(order, S):
    """(mixed, padded) descriptors of the wide-tag workload: every product with one spare bit, levels and C that hold the sum of S
    products, so nothing rounds or overflows (the linear class; tests/test_stacked_tile_coverage.py pins the kernel variant it runs on)"""
    ea, eb = (R63, C5) if order == "ra" else (C5, R63)
    zp = Qcomplex(R63, R63)   # the real operand as a complex one whose imaginary parts are zero
    lg = max(1, (S - 1).bit_length())
    cw = Qcomplex(Qu(15 + lg, 6), Qu(15 + lg, 0))
    mixed = lower(ea, eb, cw, S, S, S, mul_args=RealComplexMul(realT=Qu(14, 6), imagT=Qu(14, 0)), add_args=[cw])
    # (Basic on the padded operand: x = a + bi, y = c + di; the products with the (6, -3) part have 0 fraction bits)
    hi, lo = Qu(14, 6), Qu(14, 0)
    bm = BasicComplexMul(acT=hi, bdT=lo, adT=lo if order == "ra" else hi, bcT=hi if order == "ra" else lo, acbdT=Qu(15, 6), adbcT=Qu(15, 6))
    cp = Qcomplex(Qu(16 + lg, 6), Qu(16 + lg, 6))
    padded = lower(zp if order == "ra" else C5, C5 if order == "ra" else zp, cp, S, S, S, mul_args=bm, add_args=[cp])
    return mixed, padded


class Arm:
    def __init__(self, ctx, descs):
        self.plans, self.bufs = [], []
        for d in descs:
            plan = capi.Plan(ctx, d)
            pb = plan.info.packed_bytes
            ptrs = [ctx.alloc(int(pb[0])), ctx.alloc(int(pb[1])), ctx.alloc(int(pb[2]))]
            plan.fill(capi.OPERAND_A, 1, 0, ptrs[0])
            plan.fill(capi.OPERAND_B, 2, 0, ptrs[1])
            self.plans.append(plan)
            self.bufs.append(ptrs)

    def time(self, warmup, iters):
        return sum(p.time_execute(b[2], b[0], b[1], warmup, iters) for p, b in zip(self.plans, self.bufs))

    def close(self, ctx):
        for p, b in zip(self.plans, self.bufs):
            p.close()
            for x in b:
                ctx.free(x)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--size", type=int, default=DEFAULT_SIZE)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--orders", default="ra,rb")
    ap.add_argument("--tags", default="default,wide")
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    out = open(a.out, "a") if a.out else None
    S = a.size
    with capi.Context() as ctx:
        for order, tags in ((o, t) for t in a.tags.split(",") for o in a.orders.split(",")):
            ea, eb = (R63, C5) if order == "ra" else (C5, R63)
            zp = Qcomplex(R63, R63)   # the real operand as a complex one whose imaginary parts are zero
            if tags == "default":
                mixed = lower(ea, eb, C5, S, S, S)
                padded = lower(zp if order == "ra" else C5, C5 if order == "ra" else zp, C5, S, S, S)
            else:
                mixed, padded = wide_descs(order, S)
            arms = {"mixed": Arm(ctx, [mixed]), "padded": Arm(ctx, [padded]), "parts": Arm(ctx, [part_desc(mixed, 0), part_desc(mixed, 1)])}
            for arm in arms.values():   # clock and code-object warm-up
                arm.time(2, 2)
            for rnd in range(a.rounds):
                for name, arm in arms.items():
                    ms = arm.time(1, a.iters)
                    info = arm.plans[0].info
                    kernel = capi.KERNEL_NAMES[info.kernel]
                    rec = {"workload": "mixed_%s_%s_%d" % (order, tags, S), "arm": name, "round": rnd, "ms": ms, "iters": a.iters, "kernel": kernel,
                           "reason": info.reason.decode(), "launches": len(arm.plans), "real_macs": 2.0 * S * S * S,
                           "provenance": profmeta.profile_key(kernel, info.reason.decode(), 2.0 * S * S * S)}
                    line = json.dumps(rec)
                    print(line, flush=True)
                    if out:
                        out.write(line + "\n")
                        out.flush()
            for arm in arms.values():
                arm.close(ctx)
    return 0


if __name__ == "__main__":
    sys.exit(main())
