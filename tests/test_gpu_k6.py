"""k_mfma_k6 (qg_mfma_k6.hip): operands of 17 / 18 value+sign bits as three unsigned base-64 digits, six products per MAC on
96x128 tiles.  Every case runs the whole matrix through the arms that exist for it — the default plan (the new kernel where the
planner admits it), QG_OPT_SCHOOLBOOK_LIMBS (balanced base-256 limbs, k_mfma_ppl's nine products) and QG_OPT_LOCKSTEP_TILES
(k_mfma16<3,3>) — compares all outputs byte for byte and then checks blocks against the oracle.  Shapes sit around the 96-row
tile (21 x 96 -+ 1) and the 128-column tile; K covers one / two / odd numbers of k-tiles and ragged ends; operand distributions
are uniform, small values and the edge set; one case sits at the largest K the planner admits for the form with every element
at the format's bounds.  Every case is a valid launch.  The fast pack path of the new layout is compared byte for byte with the
generic kernel.  Run time on an MI355X: about 6 s (42 tests)."""
import numpy as np
import pytest

from qublas_amd import capi
from qublas_amd.desc import Qu, RND, SAT, TRN, WRP, Tags, lower

pytestmark = pytest.mark.gpu

E88 = Qu(8, 8, True, TRN.TCPL, SAT.ZERO)     # bench.py's operand: 17 bits
KW88 = dict(mul_args=Tags(17, 16), add_args=[Qu(29, 16)])
E98 = Qu(9, 8)                                # 18 bits
U98 = Qu(9, 8, False)                         # unsigned, 17 bits
U108 = Qu(10, 8, False)                       # unsigned, 18 bits
E66 = Qu(6, 6)                                # 13 bits: two limbs
K6 = b"six products"
NINE = b"nine products"
ARMS = (0, capi.OPT_SCHOOLBOOK_LIMBS, capi.OPT_LOCKSTEP_TILES)


def run_arm(d, flags, dist, seeds=(1, 2), host=None):
    """device fill (or, host = (A, B): pack these host-layout operands), execute, unpack; returns the host-layout bytes of C and
    the plan's reason"""
    with capi.Context() as ctx:
        plan = capi.Plan(ctx, d, flags)
        info = plan.info
        assert capi.KERNEL_NAMES[info.kernel] == "mfma_i8_limb"
        pb = info.packed_bytes
        pA, pB, pC = ctx.alloc(pb[0]), ctx.alloc(pb[1]), ctx.alloc(pb[2])
        nbytes = d.M * d.N * info.host_elem_bytes[2]
        dC = ctx.alloc(nbytes)
        if host is None:
            plan.fill(capi.OPERAND_A, seeds[0], dist, pA)
            plan.fill(capi.OPERAND_B, seeds[1], dist, pB)
        else:
            for op, arr, dst in ((capi.OPERAND_A, host[0], pA), (capi.OPERAND_B, host[1], pB)):
                dev = ctx.alloc(arr.nbytes)
                ctx.h2d(dev, arr)
                plan.pack(op, dev, dst)
                ctx.sync()
                ctx.free(dev)
        plan.execute(pC, pA, pB)
        plan.unpack_c(pC, dC)
        out = np.zeros(nbytes, np.uint8)
        ctx.d2h(out, dC)
        for p in (pA, pB, pC, dC):
            ctx.free(p)
        reason = bytes(info.reason)
        plan.close()
    return out, reason


def operands(oracle, d, ea, eb, dist, seeds=(1, 2)):
    """dist 2 (the edge set of oracle/qoracle.c) exists on the host only: such operands are packed from the host layout"""
    if dist != 2:
        return None
    return oracle.fill(ea, d.M * d.K, seeds[0], 2), oracle.fill(eb, d.K * d.N, seeds[1], 2)


def run_arms(d, dist, seeds=(1, 2), expect_k6=True, host=None):
    outs = []
    for flags in ARMS:
        out, reason = run_arm(d, flags, dist, seeds, host)
        if flags == 0:
            assert (K6 in reason) == expect_k6, reason
        else:
            assert K6 not in reason, reason
        outs.append(out)
    assert np.array_equal(outs[0], outs[1]), "default plan differs from QG_OPT_SCHOOLBOOK_LIMBS"
    assert np.array_equal(outs[0], outs[2]), "default plan differs from QG_OPT_LOCKSTEP_TILES"
    return outs[0]


def check(oracle, d, ec, got, rows, cols, dist, ea, eb, seeds=(1, 2)):
    A = oracle.fill(ea, d.M * d.K, seeds[0], dist)
    B = oracle.fill(eb, d.K * d.N, seeds[1], dist)
    cdt = oracle.host_dtype(ec)
    exp = np.zeros(d.M * d.N, dtype=cdt)
    oracle.gemm(d, A, B, ec, rows=rows, cols=cols, nthreads=16, out=exp)
    sl = (slice(cols[0], cols[1]), slice(rows[0], rows[1]))
    assert np.array_equal(got.view(cdt).reshape(d.N, d.M)[sl], exp.reshape(d.N, d.M)[sl])


@pytest.mark.parametrize("M,N,K,dist", [
    (2015, 2048, 64, 0),      # one row short of 21 tiles of 96; one k-tile: every refill of the loop is a clamped one
    (2016, 2047, 1, 2),       # exactly 21 tiles; a single reduction index
    (2017, 2049, 63, 0),      # one row / one column into the next tile
    (2016, 2048, 65, 1),      # two k-tiles, the second almost empty
    (2017, 2047, 320, 2),     # odd number of k-tiles (ring position)
    (2015, 2049, 1000, 0),    # ragged everything
    (4096, 1024, 2048, 0),    # 43 x 8 tiles, 4096 = 42 x 96 + 64
])
def test_shapes_around_the_tile(oracle, M, N, K, dist):
    ec = Qu(23, 8)
    d = lower(E88, E88, ec, M, N, K, **KW88)
    got = run_arms(d, dist, host=operands(oracle, d, E88, E88, dist))
    check(oracle, d, ec, got, rows=(0, 8), cols=(0, 256), dist=dist, ea=E88, eb=E88)
    check(oracle, d, ec, got, rows=(M - 100, M - 90), cols=(N - 200, N), dist=dist, ea=E88, eb=E88)   # group 1's rows of the last-but-one tile
    check(oracle, d, ec, got, rows=(M - 6, M), cols=(N - 130, N), dist=dist, ea=E88, eb=E88)          # the ragged corner


FORMATS = [
    ("int<8,8>", E88, E88, KW88, True),
    ("int<9,8>", E98, E98, dict(mul_args=Tags(19, 16), add_args=[Qu(31, 16)]), True),
    ("uint17", U98, U98, dict(mul_args=Tags(18, 16), add_args=[Qu(30, 16)]), True),
    ("uint18", U108, U108, dict(mul_args=Tags(20, 16), add_args=[Qu(32, 16)]), True),
    ("int<9,8> x uint17", E98, U98, dict(mul_args=Tags(19, 16), add_args=[Qu(31, 16)]), True),
    ("13 x 18 bits", E66, E98, dict(mul_args=Tags(16, 14), add_args=[Qu(28, 14)]), False),   # 2 x 3 limbs: six schoolbook products already
]


@pytest.mark.parametrize("dist", [0, 1, 2])
@pytest.mark.parametrize("name,ea,eb,kw,k6", FORMATS, ids=[f[0] for f in FORMATS])
def test_formats_and_distributions(oracle, name, ea, eb, kw, k6, dist):
    ec = Qu(25, 8)      # 8-byte container
    d = lower(ea, eb, ec, 2016, 2048, 512, **kw)
    if ea is E66:       # (2 x 3 limbs have no two-group kernel: the flags change nothing there, one arm)
        got, reason = run_arm(d, 0, dist, host=operands(oracle, d, ea, eb, dist))
        assert K6 not in reason
    else:
        got = run_arms(d, dist, expect_k6=k6, host=operands(oracle, d, ea, eb, dist))
    check(oracle, d, ec, got, rows=(40, 56), cols=(1900, 2048), dist=dist, ea=ea, eb=eb)
    check(oracle, d, ec, got, rows=(2008, 2016), cols=(0, 128), dist=dist, ea=ea, eb=eb)


KMAX = 43690   # 3 K <= 2^17 - 1: the largest reduction length of a single-launch 3 x 3-limb plan, far inside K * 126^2 < 2^31 (135 266)


@pytest.mark.parametrize("va,vb", [("hi", "hi"), ("lo", "hi")])
def test_every_element_at_the_bound_at_the_largest_k(oracle, va, vb):
    """all digits at their maximum: the Karatsuba sums reach 126 in every byte and P01 = K * 126^2 — against the closed form"""
    lo, hi = -(1 << 16), (1 << 16) - 1
    a, b = (hi if va == "hi" else lo), (hi if vb == "hi" else lo)
    ec = Qu(32, 16)     # holds K * 2^32 exactly, no shift
    d = lower(E88, E88, ec, 2016, 2048, KMAX, mul_args=Tags(17, 16), add_args=[Qu(33, 16)])
    assert capi.classify(d).cls == capi.classify(lower(E88, E88, Qu(23, 8), 4096, 4096, 4096, **KW88)).cls
    A = np.full(d.M * d.K, a, dtype=np.int32)
    B = np.full(d.K * d.N, b, dtype=np.int32)
    got, reason = run_arm(d, 0, 0, host=(A, B))
    assert K6 in reason, reason
    assert np.all(got.view(np.int64) == KMAX * a * b)
    ref, _ = run_arm(d, capi.OPT_SCHOOLBOOK_LIMBS, 0, host=(A, B))
    assert np.array_equal(got, ref)
    exp = np.zeros(d.M * d.N, dtype=np.int64)
    oracle.gemm(d, A, B, ec, rows=(2000, 2004), cols=(2040, 2048), nthreads=16, out=exp)
    assert np.array_equal(got.view(np.int64).reshape(d.N, d.M)[2040:2048, 2000:2004], exp.reshape(d.N, d.M)[2040:2048, 2000:2004])


@pytest.mark.parametrize("ec", [
    Qu(23, 8),                                 # 4 bytes, truncation + SAT::TCPL: the shift-and-clamp epilogue
    Qu(14, 16, True, TRN.TCPL, SAT.TCPL),      # no shift at all, saturates
    Qu(12, 8, True, RND.CONV, SAT.SMGN),       # general routine
    Qu(20, 4, False, RND.INF, SAT.ZERO),       # unsigned, SAT::ZERO
    Qu(18, 10, True, TRN.SMGN, WRP.TCPL),
    Qu(29, 16),                                # 8-byte container, the shift-and-clamp epilogue
    Qu(40, 6, True, RND.NEG_INF, SAT.TCPL),    # 8 bytes, general routine
])
def test_every_container_and_mode(oracle, ec):
    d = lower(E88, E88, ec, 2016, 2048, 512, **KW88)
    got = run_arms(d, 0)
    check(oracle, d, ec, got, rows=(1000, 1016), cols=(1024, 1280), dist=0, ea=E88, eb=E88)


def test_host_layout_store_matches_the_unpacked_result():
    """qgemul_execute_host_c: the epilogue that stores the reference layout directly, ragged M and N"""
    ec = Qu(23, 8)
    d = lower(E88, E88, ec, 2017, 2047, 200, **KW88)
    ref, reason = run_arm(d, 0, 0)
    assert K6 in reason
    with capi.Context() as ctx:
        plan = capi.Plan(ctx, d, 0)
        pb = plan.info.packed_bytes
        pA, pB = ctx.alloc(pb[0]), ctx.alloc(pb[1])
        dC = ctx.alloc(ref.nbytes)
        plan.fill(capi.OPERAND_A, 1, 0, pA)
        plan.fill(capi.OPERAND_B, 2, 0, pB)
        assert plan.stores_host_c
        plan.execute_host_c(dC, pA, pB)
        out = np.zeros(ref.nbytes, np.uint8)
        ctx.d2h(out, dC)
        for p in (pA, pB, dC):
            ctx.free(p)
        plan.close()
    assert np.array_equal(out, ref)


def test_which_plans_take_the_form():
    c3l = lower(E88, E88, Qu(23, 8), 4096, 4096, 4096, **KW88)
    assert K6 in capi.classify(c3l).reason and list(capi.classify(c3l).limbs)[:2] == [3, 3]
    assert NINE in capi.classify(c3l, capi.OPT_SCHOOLBOOK_LIMBS).reason
    assert K6 not in capi.classify(c3l, capi.OPT_LOCKSTEP_TILES).reason
    e19 = Qu(10, 8)
    assert NINE in capi.classify(lower(e19, e19, Qu(25, 8), 2048, 2048, 512, mul_args=Tags(21, 16), add_args=[Qu(33, 16)])).reason
    over = lower(E88, E88, Qu(23, 8), 2048, 2048, KMAX + 1, mul_args=Tags(17, 16), add_args=[Qu(33, 16)])
    assert K6 not in capi.classify(over).reason and b"k-chunk" in capi.classify(over).reason


@pytest.mark.parametrize("e,kw", [
    (Qu(10, 8), dict(mul_args=Tags(21, 16), add_args=[Qu(33, 16)])),       # 19 bits
    (Qu(12, 10), dict(mul_args=Tags(25, 20), add_args=[Qu(37, 20)])),      # 23 bits
])
def test_wider_operands_keep_the_nine_product_kernel(oracle, e, kw):
    """k_mfma_ppl's 3 x 3 body through the default path, now that int<8,8> no longer reaches it by default"""
    ec = Qu(25, 8)
    d = lower(e, e, ec, 2048, 2048, 320, **kw)
    a, ra = run_arm(d, 0, 0)
    b, _ = run_arm(d, capi.OPT_LOCKSTEP_TILES, 0)
    assert NINE in ra
    assert np.array_equal(a, b)
    check(oracle, d, ec, a, rows=(700, 708), cols=(0, 256), dist=0, ea=e, eb=e)


@pytest.mark.parametrize("ta,pad", [(False, 0), (False, 3), (True, 4), (True, 1)])
def test_fast_pack_writes_the_bytes_of_the_generic_kernel(ta, pad):
    """k_pack_limb32 on the three-digit layout (rows contiguous; k contiguous with 16-byte and with scalar loads; 96-row tiles whose
    last 64-row block reaches beyond the padded rows) against k_pack (QG_OPT_GENERIC_LAYOUT): planes, trailer and row sums"""
    M, N, K = 2017, 2047, 1000
    d = lower(E88, E88, Qu(23, 8), M, N, K, transposed_a=ta, **KW88)
    rng = np.random.default_rng(7)
    bufs = {}
    for flags in (0, capi.OPT_GENERIC_LAYOUT):
        with capi.Context() as ctx:
            plan = capi.Plan(ctx, d, flags)
            assert K6 in bytes(plan.info.reason)
            pb = [int(x) for x in plan.info.packed_bytes]
            for op, rows, cols in ((capi.OPERAND_A, K if ta else M, M if ta else K), (capi.OPERAND_B, K, N)):
                ld = rows + pad
                host = np.zeros(ld * cols, dtype=np.int32)
                host.reshape(cols, ld)[:, :rows] = np.random.default_rng(op + 11).integers(E88.raw_min, E88.raw_max + 1, (cols, rows), dtype=np.int32)
                hd, pk = ctx.alloc(host.nbytes), ctx.alloc(pb[op])
                ctx.h2d(hd, host)
                plan.pack(op, hd, pk, ld)
                ctx.sync()
                buf = np.zeros(pb[op], dtype=np.uint8)
                ctx.d2h(buf, pk)
                bufs[(flags, op)] = buf
                ctx.free(hd)
                ctx.free(pk)
            plan.close()
    for op in (capi.OPERAND_A, capi.OPERAND_B):
        assert np.array_equal(bufs[(0, op)], bufs[(capi.OPT_GENERIC_LAYOUT, op)]), op
        assert np.count_nonzero(bufs[(0, op)]) > 0.5 * bufs[(0, op)].size
