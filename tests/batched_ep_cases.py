"""Shared by tests/test_batched_ep_plan.py (CPU) and tests/test_gpu_batched_ep.py (GPU): the member formats, the chains and the
expected values of element-wise chains on batched plans (include/qgemul.h, qgemul_*_batched_ep).  Not a test module.

FORMATS holds the five rows of tests/test_gpu_batched.py that the batched chains are pinned on, by value, plus *_c16 twins of the
limb rows: the same operands and tags into a 16-bit C.  A fused chain needs 32-bit arithmetic, which a Qgemul result of 33 storage
bits (Qu<24,8>) never has; the twins are how every limb geometry of the fused kernel runs."""
import math

import numpy as np

import approx_ref as R
from qublas_amd import capi
from qublas_amd.desc import Approx, Ew, Qu, RND, SAT, TRN, WRP, Tags, ew_result, lower, lower_epilogue, lower_epilogue_x

E43, E88, Q78 = Qu(4, 3), Qu(8, 8), Qu(7, 8)
# name -> (A element, B element, C element, lowering keywords, transposed A, limbs the planner must report)
FORMATS = {
    "e43_c1byte": (E43, E43, Qu(4, 3), dict(mul_args=Tags(9, 6), add_args=[Qu(19, 6)]), False, [1, 1]),
    "e88_3x3": (E88, E88, Qu(24, 8), dict(mul_args=Tags(17, 16), add_args=[Qu(29, 16)]), False, [3, 3]),
    "q78_centred": (Q78, Q78, Qu(20, 8), dict(mul_args=Tags(15, 16), add_args=[Qu(28, 16)]), False, [2, 2]),
    "e88_x_e43_3x1": (E88, E43, Qu(20, 8), dict(mul_args=Tags(13, 11), add_args=[Qu(25, 11)]), False, [3, 1]),
    "e88_3x3_tn": (E88, E88, Qu(24, 8), dict(mul_args=Tags(17, 16), add_args=[Qu(29, 16)]), True, [3, 3]),
}
C16 = Qu(7, 8)
for _n in ("e88_3x3", "q78_centred", "e88_x_e43_3x1", "e88_3x3_tn"):
    FORMATS[_n + "_c16"] = FORMATS[_n][:2] + (C16,) + FORMATS[_n][3:]
SHAPES = [(3, 5, 7), (65, 33, 100), (129, 130, 65)]      # one ragged tile, 2 x 1 tiles, 3 x 3 tiles per member
BATCHES = (1, 2, 9)                                      # nine is no multiple of the 8 XCD classes
POISON = 0x5a
# the planner's default between the fused and the pass form where both apply: decided by tools/measure_batched_ep.py (DESIGN.md
# section 9).  QG_OPT_FUSED_EPILOGUE / QG_OPT_UNFUSED_EPILOGUE select either form whatever the default is.
DEFAULT_FUSED = False


def fused_expected(fusable: bool, flags: int) -> bool:
    if not fusable or (flags & capi.OPT_UNFUSED_EPILOGUE):
        return False
    return DEFAULT_FUSED or bool(flags & capi.OPT_FUSED_EPILOGUE)

S34, B106 = Qu(3, 4), Qu(10, 6)
X312 = Qu(3, 12)
FA = Qu(4, 10, True, RND.CONV, SAT.TCPL)
FB = Qu(3, 9, True, TRN.TCPL, SAT.ZERO)
FC = Qu(2, 8, True, RND.ZERO, WRP.TCPL)
FD = Qu(5, 6, True, TRN.SMGN, SAT.SMGN)
# two segments of degree 1, one format per level for both: the uniform form
UNIFORM2 = [(-0.5, [(300, FA), (-1100, FA)]), (math.inf, [(-512, FA), (900, FA)])]
# two segments whose formats (and lengths) differ: the general form
GENERAL2 = [(0.25, [(700, FB), (-300, FC)]), (math.inf, [(-77, FD), (900, FA), (-247, FB)])]


def chains(cq: Qu):
    """name -> (stages, D's element type, per stage: is its tensor operand shared).  1 .. 5 are the chains of the issue's list."""
    scale = Ew("mul", S34, scalar=True)
    narrow = Qu(max(cq.intBits - 2, 1), max(cq.fracBits - 1, 0), True, RND.CONV, SAT.TCPL)
    act_in = [Ew("mul", S34, Tags(24, 8), scalar=True, into=Qu(24, 8)), Ew("add", B106, into=X312)]
    return {
        "1_scale_shared_bias": ([scale, Ew("add", B106)], cq, [0, 1]),
        "2_member_sub_shared_mul_wide": ([Ew("sub", B106, x_first=False), Ew("mul", Qu(10, 6))], Qu(30, 12), [0, 1]),
        "3_no_stage_narrow_sat": ([], narrow, []),
        "4_four_stages_1_2_4_8_bytes": ([Ew("add", Qu(3, 4), into=Qu(12, 8)), Ew("mul", Qu(10, 5), into=Qu(12, 8)),
                                         Ew("sub", Qu(20, 8), x_first=False, into=Qu(21, 8)), Ew("add", Qu(30, 10))], Qu(20, 6), [1, 0, 1, 0]),
        "5_act_uniform": (act_in + [Approx(UNIFORM2)], Qu(1, 10, True, RND.CONV, SAT.TCPL), [0, 1, 0]),
        "5_act_general": (act_in + [Approx(GENERAL2)], Qu(1, 10, True, RND.CONV, SAT.TCPL), [0, 1, 0]),
        "5_act_member_operand": ([Ew("add", B106, into=X312), Approx(UNIFORM2)], X312, [0, 0]),
    }


def branch_chains(cq: Qu):
    """APPROX chains for the branches of the pass kernels k_approx_bd / k_approx_grp that chains 5_* leave out (those are 64-bit with a
    shared bias, or 32-bit without a scalar stage): 32-bit arithmetic with a scalar stage and a shared tensor operand, and 64-bit
    arithmetic with per-member tensor operands only.  Kept out of chains(): the plan tests walk that list"""
    act_in = [Ew("mul", S34, Tags(24, 8), scalar=True, into=Qu(24, 8)), Ew("add", B106, into=X312)]
    return {
        "6_act_scalar_32bit": ([Ew("mul", S34, scalar=True), Ew("add", B106, into=X312), Approx(UNIFORM2)], X312, [0, 1, 0]),
        "6_act_member_operand_wide": (act_in + [Approx(UNIFORM2)], Qu(1, 10, True, RND.CONV, SAT.TCPL), [0, 0, 0]),
    }


def lowered(fmt, shape, chain):
    """(descriptor, epilogue, tables, stages, C type, D type, shared flags) of one case"""
    ea, eb, ec, kw, ta, _ = FORMATS[fmt]
    M, N, K = shape
    d = lower(ea, eb, ec, M, N, K, transposed_a=ta, **kw)
    stages, dq, shared = {**chains(ec), **branch_chains(ec)}[chain]
    ep, tabs = lower_epilogue_x(ec, stages, dq)
    return d, ep, tabs, stages, ec, dq, shared


def bits32(d, ep, tabs) -> bool:
    """the planner has bounded the whole chain by 32-bit arithmetic (what a fused chain needs)"""
    return bool(capi.approx_plan_form(d, ep, tabs).bits32)


def has_approx(stages) -> bool:
    return any(isinstance(s, Approx) for s in stages)


def expected(oracle, c: Qu, stages, dq: Qu, x, E):
    """the chain on raw values x (format c): oracle.eltwise for each plain stage (with the assignment that follows it), the
    restatement (tests/approx_ref.py) for an Approx stage and a convert-only oracle.eltwise for its assignment"""
    x = np.asarray(x, dtype=np.int64)
    if not stages:
        return oracle.eltwise(lower_epilogue(c, [], dq), c, x, [])
    f = c
    for k, st in enumerate(stages):
        last = k + 1 == len(stages)
        if isinstance(st, Approx):
            x = R.approx(x, f, list(st.segments))
            nxt = dq if last else (st.into or f)
            if nxt != f:
                x = oracle.eltwise(lower_epilogue(f, [], nxt), f, x, [])
        else:
            nxt = dq if last else (st.into or ew_result(f, st))
            x = oracle.eltwise(lower_epilogue(f, [st], nxt), f, x, [E[k]])
        f = nxt
    return x


def extents(d, lda=0, ldb=0, ldc=0):
    ra, ca = (d.K, d.M) if d.transA else (d.M, d.K)
    return (ca - 1) * (lda or ra) + ra, (d.N - 1) * (ldb or d.K) + d.K, (d.N - 1) * (ldc or d.M) + d.M


def host_batch(oracle, e, batch, ext, stride, seed, dists):
    """a host buffer of `batch` members at `stride` elements: member b filled by the oracle's generator, poison between the members"""
    buf = np.empty((batch - 1) * stride + ext, dtype=oracle.host_dtype(e))
    buf.view(np.uint8)[:] = POISON
    members = []
    for b in range(batch):
        m = oracle.fill(e, ext, seed + 17 * b, dists[b % len(dists)])
        buf[b * stride:b * stride + ext] = m
        members.append(m)
    return buf, members
