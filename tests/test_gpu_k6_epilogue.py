"""k_mfma_k6's epilogue (qg_mfma_k6.hip) recombines its six accumulators in 32-bit pieces; the range argument rests on the planner's
bound K * 126^2 < 2^31.  These cases run the shapes the benchmark and the tools time — 4096^3 and 2048^3, with and without a
partly filled last tile round — and the corners of that argument (the longest k-loop the planner admits, edge operands, 4- and
8-byte C, the general round + overflow routine, the host-layout store), each byte for byte against QG_OPT_SCHOOLBOOK_LIMBS (the
nine-product kernel, whose epilogue is untouched) and on sampled blocks against the oracle.  Every case is a valid launch.
Run time on an MI355X: about 10 s."""
import numpy as np
import pytest

from qublas_amd import capi
from qublas_amd.desc import Qu, RND, SAT, TRN, Tags, lower

pytestmark = pytest.mark.gpu

E88 = Qu(8, 8, True, TRN.TCPL, SAT.ZERO)     # bench.py's operand: 17 bits
C4 = Qu(23, 8)                               # 4-byte container, shift-and-clamp epilogue (the headline's)
C8 = Qu(29, 16)                              # 8-byte container, shift-and-clamp epilogue
CG = Qu(12, 8, True, RND.CONV, SAT.SMGN)     # the general round + overflow routine
K6 = b"six products"


def pack_or_fill(ctx, plan, dist, seeds, host, pA, pB):
    if host is None:
        plan.fill(capi.OPERAND_A, seeds[0], dist, pA)
        plan.fill(capi.OPERAND_B, seeds[1], dist, pB)
        return
    for op, arr, dst in ((capi.OPERAND_A, host[0], pA), (capi.OPERAND_B, host[1], pB)):
        dev = ctx.alloc(arr.nbytes)
        ctx.h2d(dev, arr)
        plan.pack(op, dev, dst)
        ctx.sync()
        ctx.free(dev)


def run_arm(d, flags, dist, seeds=(1, 2), host=None, host_c=False):
    """returns the host-layout bytes of C"""
    with capi.Context() as ctx:
        plan = capi.Plan(ctx, d, flags)
        info = plan.info
        assert capi.KERNEL_NAMES[info.kernel] == "mfma_i8_limb"
        assert (K6 in bytes(info.reason)) == (not flags & capi.OPT_SCHOOLBOOK_LIMBS)
        pb = info.packed_bytes
        pA, pB, pC = ctx.alloc(pb[0]), ctx.alloc(pb[1]), ctx.alloc(pb[2])
        nbytes = d.M * d.N * info.host_elem_bytes[2]
        dC = ctx.alloc(nbytes)
        pack_or_fill(ctx, plan, dist, seeds, host, pA, pB)
        if host_c:
            assert plan.stores_host_c
            plan.execute_host_c(dC, pA, pB)
        else:
            plan.execute(pC, pA, pB)
            plan.unpack_c(pC, dC)
        out = np.zeros(nbytes, np.uint8)
        ctx.d2h(out, dC)
        for p in (pA, pB, pC, dC):
            ctx.free(p)
        plan.close()
    return out


def check(oracle, d, ec, got, rows, cols, dist, seeds=(1, 2)):
    A = oracle.fill(E88, d.M * d.K, seeds[0], dist)
    B = oracle.fill(E88, d.K * d.N, seeds[1], dist)
    cdt = oracle.host_dtype(ec)
    exp = np.zeros(d.M * d.N, dtype=cdt)
    oracle.gemm(d, A, B, ec, rows=rows, cols=cols, nthreads=16, out=exp)
    sl = (slice(cols[0], cols[1]), slice(rows[0], rows[1]))
    assert np.array_equal(got.view(cdt).reshape(d.N, d.M)[sl], exp.reshape(d.N, d.M)[sl])


SHAPES = [
    # M, N, K, C, dist, host-layout store
    (4096, 4096, 4096, C4, 0, False),     # the headline: 1376 tiles of 96 x 128 = 5.375 rounds of 256 workgroups
    (2048, 2048, 2048, C4, 1, False),     # 352 tiles = 1.375 rounds
    (2048, 2048, 2048, C8, 2, False),     # 8-byte C, the edge operands
    (2048, 2048, 2048, CG, 0, False),     # the general routine behind the recombination
    (3000, 2100, 1536, C4, 0, True),      # M no multiple of 96 or 128, ragged N; host-layout store
    (2500, 1920, 1590, C8, 2, True),      # ragged K, 8-byte host-layout store, edge operands
    (3840, 4096, 1024, C4, 0, False),     # 1280 tiles: exactly 5 rounds
    (2016, 2048, 43690, C8, 0, False),    # the longest k-loop the planner admits for a single launch
]


@pytest.mark.parametrize("M,N,K,ec,dist,host_c", SHAPES)
def test_same_bytes_as_nine_products(oracle, M, N, K, ec, dist, host_c):
    d = lower(E88, E88, ec, M, N, K, mul_args=Tags(17, 16), add_args=[Qu(33, 16) if K > 4096 else Qu(29, 16)])
    host = (oracle.fill(E88, M * K, 1, 2), oracle.fill(E88, K * N, 2, 2)) if dist == 2 else None
    got = run_arm(d, 0, dist, host=host, host_c=host_c)
    ref = run_arm(d, capi.OPT_SCHOOLBOOK_LIMBS, dist, host=host)
    assert np.array_equal(got, ref), "six products differ from QG_OPT_SCHOOLBOOK_LIMBS"
    kr = 2 if K > 4096 else 8
    for rows, cols in (((0, kr), (0, 64)), ((M // 2, M // 2 + kr), (N // 2 - 32, N // 2 + 32)), ((M - kr, M), (N - 64, N)),
                       ((M - 100, M - 100 + kr), (0, 64)), ((0, kr), (N - 64, N))):
        check(oracle, d, ec, got, rows, cols, dist)


def test_one_plan_many_launches_on_alternating_operands():
    """the kernel keeps no state between launches: 12 launches of one plan, A alternating between two fills"""
    d = lower(E88, E88, C4, 2048, 2048, 2048, mul_args=Tags(17, 16), add_args=[Qu(29, 16)])
    with capi.Context() as ctx:
        plan, nine = capi.Plan(ctx, d, 0), capi.Plan(ctx, d, capi.OPT_SCHOOLBOOK_LIMBS)
        pb, qb = plan.info.packed_bytes, nine.info.packed_bytes
        assert pb[2] == qb[2]
        pA, qA = [ctx.alloc(pb[0]), ctx.alloc(pb[0])], [ctx.alloc(qb[0]), ctx.alloc(qb[0])]
        pB, qB, pC, pR = ctx.alloc(pb[1]), ctx.alloc(qb[1]), ctx.alloc(pb[2]), ctx.alloc(pb[2])
        for pl, As, B in ((plan, pA, pB), (nine, qA, qB)):
            pl.fill(capi.OPERAND_A, 1, 0, As[0])
            pl.fill(capi.OPERAND_A, 3, 1, As[1])
            pl.fill(capi.OPERAND_B, 2, 0, B)
        ref = []
        for a in qA:
            nine.execute(pR, a, qB)
            r = np.zeros(pb[2], np.uint8)
            ctx.d2h(r, pR)
            ref.append(r)
        assert not np.array_equal(ref[0], ref[1])
        got = np.zeros(pb[2], np.uint8)
        for it in range(12):
            plan.execute(pC, pA[it % 2], pB)
            ctx.d2h(got, pC)
            assert np.array_equal(got, ref[it % 2]), f"launch {it}"
        for p in pA + qA + [pB, qB, pC, pR]:
            ctx.free(p)
        plan.close()
        nine.close()
