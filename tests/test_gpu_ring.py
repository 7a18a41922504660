"""Ring plans of the linear class (qublas_amd/csrc/qg_mfma_ring.hip; the rule: qg_plan.cpp, ring_plan): product and every tree level
wrap into one signed format of n <= 32 bits, so the tree equals the dot product modulo 2^n and runs on the int8 matrix cores with
only the limb products of weight below 2^n and int32 accumulators that are ALLOWED to wrap.  Everything here is bit-exact:
  * the reference's own results (tests/golden/ref_ring_0.jsonl.gz), and the same descriptor through QG_OPT_FORCE_TREE (the exact
    tree kernels these descriptors ran on before), byte for byte;
  * a shape grid around the 128 x 128 tile and the 64-byte k-tile, transposed A, padded leading dimensions, the three operand
    distributions, every ring width, against the oracle;
  * the hardware question the kernel rests on — v_mfma_i32_16x16x64_i8 accumulates modulo 2^32, it does not saturate — with valid
    launches whose true sums pass 2^31, against modular numpy arithmetic (a truth independent of the oracle);
  * the resident API, the fast pack path of the 4-plane / 31-bit operands, an element-wise chain, BitStream export, the host-C
    entry, and the full sizes 2048^3 int32 and 4096^3 int16 on sampled blocks."""
import numpy as np
import pytest

import golden_io as G
from qublas_amd import capi
from qublas_amd.desc import Ew, Qu, RND, SAT, TRN, WRP, Tags, desc_from_dict, lower, lower_epilogue

pytestmark = pytest.mark.gpu

RING = b"wrapping ring"
RECORDS = list(G._records(G.GOLD + "/ref_ring_0.jsonl.gz"))


def I(bits):
    """plain C integer of `bits` bits: Qu<bits-1, 0, WRP::TCPL>"""
    return Qu(bits - 1, 0, True, TRN.TCPL, WRP.TCPL)


def ring_desc(e, M, N, K, **kw):
    return lower(e, e, e, M, N, K, **kw)


def is_ring(d, flags=0):
    return RING in bytes(capi.classify(d, flags).reason)


def both_arms(d, ec, A, B, **ld):
    """the default plan (a ring plan) and QG_OPT_FORCE_TREE on the same host operands: C of the first, after comparing the bytes"""
    n = (ld.get("ldc") or d.M) * d.N
    dt = np.dtype(np.int32 if ec.host_bytes == 4 else np.int64)
    got = capi.run(d, np.zeros(n, dt), A, B, **ld)
    tree = capi.run(d, np.zeros(n, dt), A, B, flags=capi.OPT_FORCE_TREE, **ld)
    assert not is_ring(d, capi.OPT_FORCE_TREE)
    assert got.tobytes() == tree.tobytes(), "ring plan differs from QG_OPT_FORCE_TREE"
    return got


@pytest.mark.parametrize("j", RECORDS, ids=lambda j: j["name"])
def test_reference_records(oracle, j):
    d = desc_from_dict(j)
    assert is_ring(d)
    _, _, ec = G.case_elems(j)
    A, B = G.case_inputs(j, oracle)
    exp = G.case_expected(j, oracle)
    got = both_arms(d, ec, A, B)
    assert np.array_equal(got, exp)


BITS = (8, 12, 16, 24, 32)
GRID = [(M, N, K) for M in (1, 127, 128, 129, 300) for N in (1, 127, 128, 129, 300) for K in (1, 63, 64, 65, 1000, 4097)]


def padded(arr, rows, cols, ld):
    """column-major rows x cols tensor with leading dimension ld; the padding holds a value no result may pick up"""
    out = np.full(ld * cols, 0x5a5a5a5 if arr.dtype == np.int32 else 0x5a5a5a5a5a5a, dtype=arr.dtype)
    out.reshape(cols, ld)[:, :rows] = arr.reshape(cols, rows)
    return out


@pytest.mark.parametrize("idx", range(len(GRID)), ids=lambda i: "%dx%dx%d" % GRID[i])
def test_shape_grid(oracle, idx):
    """every (M, N, K) of the grid; ring width, distribution, transposition and padding rotate through it, so that every width
    meets every K and every M"""
    M, N, K = GRID[idx]
    e = I(BITS[(idx + idx // 6) % 5])
    dist = idx % 3
    ta = (idx // 3) % 2 == 1
    pad = (idx // 2) % 2 == 1
    d = ring_desc(e, M, N, K, transposed_a=ta)
    if N > 1:
        assert is_ring(d), bytes(capi.classify(d).reason)
    A = oracle.fill(e, M * K, 100 + idx, dist)
    B = oracle.fill(e, K * N, 200 + idx, dist)
    exp = oracle.gemm(d, A, B, e, nthreads=16)
    if not pad:
        got = both_arms(d, e, A, B)
        assert np.array_equal(got, exp)
        return
    ar, ac = (K, M) if ta else (M, K)
    lda, ldb, ldc = ar + 3, K + 5, M + 2
    got = both_arms(d, e, padded(A, ar, ac, lda), padded(B, K, N, ldb), lda=lda, ldb=ldb, ldc=ldc)
    assert np.array_equal(got.reshape(N, ldc)[:, :M], exp.reshape(N, M))
    assert np.all(got.reshape(N, ldc)[:, M:] == 0)          # the rows between M and ldc are not written


R132 = Qu(13, 2, True, TRN.TCPL, WRP.TCPL)
FORMS = [
    # name, A, B, C, ring type (None: default tags), n, limbs, products
    ("int16 << 2 into Qu<13,2> ring, C Qu<20,4>", I(16), I(16), Qu(20, 4), R132, 16, (2, 2), 3),
    ("int8 operands into an int12 ring", I(8), I(8), I(12), I(12), 12, (1, 1), 1),
    ("int8 x int16 into an int24 ring", I(8), I(16), I(24), I(24), 24, (1, 3), 3),
    ("int12 x int32 into an int32 ring", I(12), I(32), I(32), I(32), 32, (2, 4), 7),
    ("saturating operands, saturating 8-bit C", Qu(15, 0), Qu(15, 0), Qu(7, 0), I(16), 16, (2, 2), 3),
    ("rounded C: Qu<13,2> ring into Qu<10,0,RND::CONV,SAT::SMGN>", Qu(7, 1, True, RND.INF, SAT.ZERO), Qu(7, 1), Qu(10, 0, True, RND.CONV, SAT.SMGN), R132, 16, (2, 2), 3),
    ("unsigned C", I(16), I(16), Qu(12, 0, False, TRN.TCPL, SAT.TCPL), None, 16, (2, 2), 3),
    ("C wider than the ring: 8-byte container", I(32), I(32), Qu(40, 4), None, 32, (4, 4), 10),
    ("levels with another QuMode", I(24), I(24), I(24), Qu(23, 0, True, RND.POS_INF, WRP.TCPL), 24, (3, 3), 6),
    ("int32 ring, fraction bits: Qu<15,8> x Qu<15,8> into Qu<15,16>", Qu(15, 8, True, TRN.TCPL, WRP.TCPL), Qu(15, 8, True, TRN.TCPL, WRP.TCPL),
     Qu(15, 16, True, TRN.TCPL, WRP.TCPL), Qu(15, 16, True, TRN.TCPL, WRP.TCPL), 32, (4, 4), 10),
]


@pytest.mark.parametrize("dist", [0, 2])
@pytest.mark.parametrize("name,ea,eb,ec,ring,n,limbs,products", FORMS, ids=[f[0] for f in FORMS])
def test_operand_ring_and_c_formats(oracle, name, ea, eb, ec, ring, n, limbs, products, dist):
    M, N, K = 130, 70, 777
    kw = dict(mul_args=Tags.of(ring), add_args=[ring]) if ring is not None else {}
    d = lower(ea, eb, ec, M, N, K, **kw)
    info = capi.classify(d)
    reason = bytes(info.reason)
    assert b"wrapping ring mod 2^%d, %d limb product" % (n, products) in reason, reason
    assert tuple(info.limbs) == limbs
    A = oracle.fill(ea, M * K, 31, dist)
    B = oracle.fill(eb, K * N, 32, dist)
    got = both_arms(d, ec, A, B)
    assert np.array_equal(got, oracle.gemm(d, A, B, ec, nthreads=16))


def modular(A, B, M, N, K, n):
    """C = A B modulo 2^n in numpy: uint64 arithmetic wraps modulo 2^64, which 2^n divides; then the signed representative"""
    a = A.astype(np.int64).view(np.uint64).reshape(K, M).T       # A is column-major M x K
    b = B.astype(np.int64).view(np.uint64).reshape(N, K).T       # B is column-major K x N
    c = (a @ b) & np.uint64((1 << n) - 1)
    c = c.astype(np.int64)
    c = np.where(c >= (1 << (n - 1)), c - (1 << n), c)
    return c.T.reshape(-1)                                       # column-major M x N


@pytest.mark.parametrize("K,ring_bits", [(262144, 8), (131072, 8), (131072, 32), (262144, 32)])
def test_the_int32_accumulators_wrap_and_do_not_saturate(K, ring_bits):
    """every element -128: each int8 product is 2^14 and the accumulator passes through exactly 2^31 at K = 2^17 and 2^32 at 2^18.
    A wrapping accumulate gives -2^31 / 0; a saturating one would stop at 2^31 - 1: C = -1 in the 8-bit ring, 2^31 - 1 in the 32-bit
    ring (int8 operands into an int32 ring: the one-product kernel with n = 32)."""
    M, N = 32, 16
    e8, r = I(8), I(ring_bits)
    d = lower(e8, e8, r, M, N, K, mul_args=Tags.of(r), add_args=[r])
    reason = bytes(capi.classify(d).reason)
    assert RING in reason and b"k-chunk" not in reason, reason
    A = np.full(M * K, -128, np.int32)
    B = np.full(K * N, -128, np.int32)
    got = capi.run(d, np.zeros(M * N, np.int32), A, B)
    true_sum = K << 14
    exp = ((true_sum + (1 << (ring_bits - 1))) % (1 << ring_bits)) - (1 << (ring_bits - 1))
    assert exp in (0, -(1 << 31))
    assert np.all(got == exp), (int(got[0]), exp)


@pytest.mark.parametrize("bits", [8, 32])
def test_long_k_in_one_launch_against_modular_numpy(oracle, bits):
    """random operands at K > 200 000: the sums of the limb products pass 2^31 many times over"""
    M, N, K = 32, 24, 200003
    e = I(bits)
    d = ring_desc(e, M, N, K)
    reason = bytes(capi.classify(d).reason)
    assert RING in reason and b"k-chunk" not in reason, reason
    A = oracle.fill(e, M * K, 5, 0)
    B = oracle.fill(e, K * N, 6, 0)
    got = capi.run(d, np.zeros(M * N, np.int32), A, B)
    assert np.array_equal(got.astype(np.int64), modular(A, B, M, N, K, bits))


def resident(d, flags=0, seeds=(1, 2), dist=0, host=None, host_c=False):
    """fill (or pack `host` = (A, B)) -> execute -> unpack on the device; the host-layout bytes of C"""
    with capi.Context() as ctx:
        plan = capi.Plan(ctx, d, flags)
        info = plan.info
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
        if host_c:
            plan.execute_host_c(dC, pA, pB)
        else:
            plan.execute(pC, pA, pB)
            plan.unpack_c(pC, dC)
        out = np.zeros(nbytes, np.uint8)
        ctx.d2h(out, dC)
        for p in (pA, pB, pC, dC):
            ctx.free(p)
        reason = bytes(info.reason)
        plan.close()
    return out, reason


@pytest.mark.parametrize("bits", BITS)
def test_device_fill_equals_host_pack(oracle, bits):
    e = I(bits)
    d = ring_desc(e, 257, 130, 1000)
    a, reason = resident(d)
    assert RING in reason
    A, B = oracle.fill(e, d.M * d.K, 1, 0), oracle.fill(e, d.K * d.N, 2, 0)
    b, _ = resident(d, host=(A, B))
    assert np.array_equal(a, b)
    c, _ = resident(d, host=(A, B), host_c=True)            # qgemul_execute_host_c
    assert np.array_equal(a, c)
    assert np.array_equal(a.view(np.int32), oracle.gemm(d, A, B, e, nthreads=16))


@pytest.mark.parametrize("bits,ta,pad", [(32, False, 0), (32, False, 3), (32, True, 4), (32, True, 1), (24, False, 0), (16, True, 4), (8, False, 3)])
def test_fast_pack_writes_the_bytes_of_the_generic_kernel(bits, ta, pad):
    """k_pack_limb32 on ring operands — four planes and W = 31 are new to it — against k_pack (QG_OPT_GENERIC_LAYOUT): planes and
    trailer, rows contiguous / k contiguous with 16-byte and with scalar loads, full-range values (the dropped remainder differs
    from zero for every width that fills its digits)"""
    M, N, K = 300, 257, 1000
    e = I(bits)
    d = ring_desc(e, M, N, K, transposed_a=ta)
    bufs = {}
    for flags in (0, capi.OPT_GENERIC_LAYOUT):
        with capi.Context() as ctx:
            plan = capi.Plan(ctx, d, flags)
            assert RING in bytes(plan.info.reason)
            pb = [int(x) for x in plan.info.packed_bytes]
            for op, rows, cols in ((capi.OPERAND_A, K if ta else M, M if ta else K), (capi.OPERAND_B, K, N)):
                ld = rows + pad
                host = np.zeros(ld * cols, dtype=np.int32)
                host.reshape(cols, ld)[:, :rows] = np.random.default_rng(op + 11).integers(e.raw_min, e.raw_max + 1, (cols, rows), dtype=np.int64).astype(np.int32)
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
        assert np.count_nonzero(bufs[(0, op)]) > 0.3 * bufs[(0, op)].size


def test_range_check_still_sees_the_operands_own_format():
    """QG_OPT_CHECK_RANGE: a ring operand keeps only its low digits, but a value outside the operand's format is still reported"""
    e = I(12)
    d = ring_desc(e, 64, 64, 64)
    A = np.zeros(64 * 64, np.int32)
    B = np.zeros(64 * 64, np.int32)
    capi.run(d, np.zeros(64 * 64, np.int32), A, B, flags=capi.OPT_CHECK_RANGE)
    A[77] = 1 << 11
    with pytest.raises(capi.QgemulError):
        capi.run(d, np.zeros(64 * 64, np.int32), A, B, flags=capi.OPT_CHECK_RANGE)


def test_elementwise_chain_behind_a_ring_gemm(oracle):
    e = I(16)
    M, N, K = 200, 131, 500
    d = ring_desc(e, M, N, K)
    s34, b106 = Qu(3, 4), Qu(10, 6)
    stages = [Ew("mul", s34, Tags(24, 8), scalar=True, into=Qu(24, 8)), Ew("add", b106)]
    dq = Qu(16, 6, True, RND.ZERO, SAT.TCPL)
    ep = lower_epilogue(e, stages, dq)
    st, info = capi.classify_ep_status(d, ep)
    assert st == 0 and RING in bytes(info.reason)
    A, B = oracle.fill(e, M * K, 3, 0), oracle.fill(e, K * N, 4, 0)
    E = [np.array([37], dtype=np.int32), oracle.fill(b106, M * N, 9, 0)]
    got = capi.run_ep(d, ep, np.zeros(M * N, np.int32), A, B, E)
    exp = oracle.eltwise(ep, e, oracle.gemm(d, A, B, e, nthreads=16).astype(np.int64), E)
    assert np.array_equal(got.astype(np.int64), exp)


def test_bitstream_export_of_a_ring_result(oracle):
    e = I(12)
    M, N, K = 130, 9, 100
    d = ring_desc(e, M, N, K)
    A, B = oracle.fill(e, M * K, 7, 0), oracle.fill(e, K * N, 8, 0)
    exp_c = oracle.gemm(d, A, B, e).astype(np.int64)
    with capi.Context() as ctx:
        plan = capi.Plan(ctx, d)
        assert RING in bytes(plan.info.reason)
        dA, dB = ctx.alloc(A.nbytes), ctx.alloc(B.nbytes)
        ctx.h2d(dA, A); ctx.h2d(dB, B)
        pA, pB, pC = (ctx.alloc(int(plan.info.packed_bytes[i])) for i in range(3))
        plan.pack(capi.OPERAND_A, dA, pA); plan.pack(capi.OPERAND_B, dB, pB)
        plan.execute(pC, pA, pB)
        for tc, ec in ((0, 0), (2, 4)):
            nb = plan.bitstream_bytes(capi.BITS_ASCII)
            assert nb == M * N * 12
            dev = ctx.alloc(nb)
            plan.export_bitstream(pC, dev, tc, ec, capi.BITS_ASCII)
            out = np.zeros(nb, dtype=np.uint8)
            ctx.d2h(out, dev)
            ctx.free(dev)
            assert out.tobytes() == oracle.bitstream(e, exp_c, tc, ec), (tc, ec)
        for p in (dA, dB, pA, pB, pC):
            ctx.free(p)
        plan.close()


def check_block(oracle, d, e, got_bytes, rows, cols, seeds=(1, 2)):
    A = oracle.fill(e, d.M * d.K, seeds[0], 0)
    B = oracle.fill(e, d.K * d.N, seeds[1], 0)
    exp = np.zeros(d.M * d.N, dtype=np.int32)
    oracle.gemm(d, A, B, e, rows=rows, cols=cols, nthreads=16, out=exp)
    sl = (slice(cols[0], cols[1]), slice(rows[0], rows[1]))
    assert np.array_equal(got_bytes.view(np.int32).reshape(d.N, d.M)[sl], exp.reshape(d.N, d.M)[sl])


@pytest.mark.parametrize("bits,size", [(32, 2048), (16, 4096)])
def test_full_size_on_sampled_blocks(oracle, bits, size):
    e = I(bits)
    d = ring_desc(e, size, size, size)
    got, reason = resident(d)
    assert RING in reason
    check_block(oracle, d, e, got, rows=(1000, 1016), cols=(0, 256))
    check_block(oracle, d, e, got, rows=(size - 6, size), cols=(size - 300, size))
    check_block(oracle, d, e, got, rows=(size // 2 - 2, size // 2 + 2), cols=(size // 2 - 64, size // 2 + 64))
    tree, reason_t = resident(d, flags=capi.OPT_FORCE_TREE)
    assert RING not in reason_t
    assert np.array_equal(got, tree)
    c = got.view(np.int32)
    assert len(np.unique(c[:100000])) > 1000       # a real comparison, not a constant
