"""The block-diagonal batched Qgemul (k_mfma_bd, qg_launch_pack_stack, the batched branch of qg_plan_geometry) where tests/test_gpu_batched.py
stops (run with -m gpu).  Every case compares each member with the oracle (qoracle_gemm) AND byte for byte with qgemul_execute +
qgemul_unpack_c of that member through a plain plan; host buffers carry poison between the members and C's gaps must survive; the
limbs and the launch count the planner answers are asserted BEFORE any device work, so that a case that silently left the form it
was written for fails.  What is pinned: all nine launch_bd<LA, LB> instantiations; 1 to 8 k-tiles on both k-tile sizes (the LDS ring
of three stages refilled with real tiles and wrapped; the members' operand offsets with more than one k-tile); the largest K of the
one-launch form with operands at the formats' bounds; every container width and conversion mode of C, saturating and wrapping;
members of 10, 17 and 18 tile rows / columns (the walk's groups of 8); a Karatsuba-eligible member; the fallbacks that loop over
plain launches; packing a second batch into packed buffers that hold one.  Every case is a valid launch.
Run time on an MI355X: about 2 s (78 tests)."""
import itertools
import re

import numpy as np
import pytest

from qublas_amd import capi
from qublas_amd.desc import Qcomplex, Qu, RND, SAT, TRN, WRP, Tags, lower
from test_batched_plan import BOUND, bound_case, roomy, tags
from test_gpu_batched import POISON, expected_buffer, extents, host_batch, read_mask, run_batched_plan, run_plain_members

pytestmark = pytest.mark.gpu

E43, E55, E77, E88, Q78, E12 = Qu(4, 3), Qu(5, 5), Qu(7, 7), Qu(8, 8), Qu(7, 8), Qu(12, 12)
LIMBS = {E43: 1, E55: 2, E77: 2, E88: 3}
ONE_LAUNCH = b"in one block-diagonal launch, 64x64 tiles"


@pytest.fixture(scope="module")
def ctx():
    with capi.Context() as c:
        yield c


def planned(d, batch, limbs, launches):
    """what the planner answers for the batch, asserted before any device work; returns the batched plan's info"""
    st, info = capi.classify_batched_status(d, batch)
    assert st == capi.QG_OK and list(info.limbs) == list(limbs), (list(info.limbs), info.reason)
    assert capi.classify_batched_launches(d, batch) == launches, info.reason
    assert (ONE_LAUNCH in bytes(info.reason)) == (launches == 1 and batch > 0), info.reason
    return info


def check(ctx, oracle, d, ea, eb, ec, batches, limbs, per_member=0, dists=(0, 1), seed=1000, edit=None):
    """members of max(batches) generated once; oracle == plain plan == batched plan for every batch count.  per_member: 0 = the
    one-launch form, else the launches of one member's plain plan (the batch loops).  edit(mA, mB): changes the members in place."""
    nb = max(batches)
    for batch in batches:
        planned(d, batch, limbs, per_member * batch if per_member else 1)
    extA, extB, extC = extents(d)
    strides = (extA + 3, extB + 5, extC + 7)
    A, mA = host_batch(oracle, ea, nb, extA, strides[0], seed, dists)
    B, mB = host_batch(oracle, eb, nb, extB, strides[1], seed + 500, dists)
    if edit:
        edit(mA, mB)
        for b in range(nb):
            A[b * strides[0]:b * strides[0] + extA] = mA[b]
            B[b * strides[1]:b * strides[1] + extB] = mB[b]
    exp = [oracle.gemm(d, a, b, ec, nthreads=8) for a, b in zip(mA, mB)]
    plain = run_plain_members(ctx, oracle, d, ec, mA, mB)
    for b in range(nb):
        assert plain[b].tobytes() == exp[b].tobytes(), ("plain plan", b)
    for batch in batches:
        got, launches = run_batched_plan(ctx, oracle, d, ec, batch, A[:(batch - 1) * strides[0] + extA], B[:(batch - 1) * strides[1] + extB], strides)
        assert launches == (per_member * batch if per_member else 1), batch
        assert got.tobytes() == expected_buffer(oracle, d, ec, batch, exp, strides[2]).tobytes(), batch
    return exp


# ---- a. all nine limb pairs: every launch_bd<LA, LB> of qg_launch_mfma_bd
PAIRS = [(ea, eb, False) for ea, eb in itertools.product((E43, E77, E88), repeat=2)] + [(E43, E77, True), (E77, E88, True)]


@pytest.mark.parametrize("ea,eb,ta", PAIRS, ids=["%dx%d%s" % (LIMBS[a], LIMBS[b], "_tn" if t else "") for a, b, t in PAIRS])
def test_all_nine_limb_pairs(ctx, oracle, ea, eb, ta):
    ec = roomy(ea, eb)
    d = lower(ea, eb, ec, 65, 33, 193, transposed_a=ta, **tags(ea, eb))
    exp = check(ctx, oracle, d, ea, eb, ec, (2, 9), [LIMBS[ea], LIMBS[eb]])
    assert all(len(np.unique(e)) > 100 for e in exp)


# ---- b. k-tile counts: one tile, the ring of three stages filled, refilled with real tiles, wrapped; exact and ragged ends
K_SINGLE = [(128, 1), (129, 2), (256, 2), (384, 3), (385, 4), (512, 4), (640, 5), (1000, 8)]      # 128-byte k-tiles
K_LIMBS = [(128, 2), (129, 3), (192, 3), (193, 4), (320, 5), (449, 8)]                            # 64-byte k-tiles
K_CASES = [(E43, K, n) for K, n in K_SINGLE] + [(e, K, n) for e in (E88, E77) for K, n in K_LIMBS]


@pytest.mark.parametrize("e,K,nk", K_CASES, ids=["%dx%d_K%d" % (LIMBS[e], LIMBS[e], K) for e, K, _ in K_CASES])
def test_k_tile_counts(ctx, oracle, e, K, nk):
    ec = roomy(e, e)
    d = lower(e, e, ec, 65, 33, K, **tags(e, e))
    bk = 128 if LIMBS[e] == 1 else 64
    assert (K + bk - 1) // bk == nk
    info = planned(d, 3, [LIMBS[e]] * 2, 1)
    # the stack's planes: batch x limbs x tile-padded rows x K padded to nk k-tiles (+ the 256-byte plane-mask trailer of limb operands)
    assert info.packed_bytes[0] == 3 * LIMBS[e] * 128 * nk * bk + (256 if LIMBS[e] > 1 else 0)
    check(ctx, oracle, d, e, e, ec, (3,), [LIMBS[e]] * 2, seed=2000 + K)


@pytest.mark.parametrize("e", [E43, E77, E88], ids=["1x1", "2x2", "3x3"])
def test_k_tiles_with_nine_members_of_nine_tiles(ctx, oracle, e):
    ec = roomy(e, e)
    d = lower(e, e, ec, 129, 130, 320, **tags(e, e))
    check(ctx, oracle, d, e, e, ec, (9,), [LIMBS[e]] * 2, seed=2500)


# ---- c. the planner's bound: the largest K of the one-launch form, operands constant per member at the formats' bounds
def low_limbs_most_negative(e):
    """the raw values of e whose balanced base-256 limbs below the top one are all -128"""
    x = np.arange(e.raw_min, e.raw_max + 1, dtype=np.int64)
    r, ok = x.copy(), np.ones(x.size, dtype=bool)
    for _ in range(LIMBS[e] - 1):
        digit = ((r + 128) & 255) - 128
        ok &= digit == -128
        r = (r - digit) >> 8
    return x[ok]


# (a single limb has no low limbs: two constants for that pair)
BOUND_CASES = [(n, w) for n in sorted(BOUND) for w in ("min_x_min", "min_x_max", "low_limbs_most_negative") if (n, w) != ("1x1", "low_limbs_most_negative")]


@pytest.mark.parametrize("name,which", BOUND_CASES, ids=["%s_%s" % c for c in BOUND_CASES])
def test_largest_k_of_the_one_launch_form(ctx, oracle, name, which):
    ea, eb, ec, K, d = bound_case(name)
    if which == "min_x_min":      # member 1: maximum x maximum; the single-limb pair keeps a factor of -2^7 there (see bound_case)
        consts = [(ea.raw_min, eb.raw_min), (ea.raw_min, eb.raw_min + 2) if name == "1x1" else (ea.raw_max, eb.raw_max)]
    elif which == "min_x_max":
        consts = [(ea.raw_min, eb.raw_max), (ea.raw_max, eb.raw_min)]
    else:
        la, lb = low_limbs_most_negative(ea), low_limbs_most_negative(eb)
        assert la.size > 1 and int(la.max()) % 256 == 128 and int(la.min()) % 256 == 128
        consts = [(int(la.max()), int(lb.max())), (int(la.min()), int(lb.max()))]
    assert consts[0] != consts[1]
    shift = ea.fracBits + eb.fracBits - ec.fracBits
    closed = [(K * a * b) >> shift for a, b in consts]
    assert all(((K * a * b) >> shift) << shift == K * a * b for a, b in consts)          # nothing is rounded away
    assert all(ec.raw_min <= c <= ec.raw_max for c in closed)
    if name == "1x1" and which == "min_x_min":
        assert K * consts[0][0] * consts[0][1] == 2 ** 31 - 2 ** 14                      # the int32 accumulator's last exact multiple

    def edit(mA, mB):
        for b, (a, bb) in enumerate(consts):
            mA[b][:] = a
            mB[b][:] = bb
    exp = check(ctx, oracle, d, ea, eb, ec, (2,), [LIMBS[ea], LIMBS[eb]], edit=edit)
    for b in range(2):
        assert exp[b].astype(np.int64).tolist() == [closed[b]] * 6, b


# ---- d. containers and modes of C: the 32-bit epilogue (single limb) and the 64-bit one (3 x 3 limbs)
def skew(mA, mB):
    """Single-limb operands cannot reach Qu<14,16>'s or Qu<12,8>'s bounds with the generator (|sum| ~ 850 against 4096 and 16384):
    every even row of A at the format's maximum, B positive and in the upper half of its range — the even rows of C then lie near
    127 * 95 * K / 2^6 ~ 19 000 and saturate, the odd rows stay a random sum and do not."""
    for a, b in zip(mA, mB):
        a.reshape(100, 65)[:, 0::2] = E43.raw_max
        b[:] = np.abs(b.astype(np.int64)).clip(0, E43.raw_max) | 64


# C, the data of the single-limb case, the data of the 3 x 3 case (a generator distribution or skew), launches of a single-limb member
MODES = {
    "4B_trn_sat": (Qu(23, 8), 0, 0, 2),                                     # holds every dot product of both cases: never at its bounds
    "4B_noshift_sat": (Qu(14, 16, True, TRN.TCPL, SAT.TCPL), skew, 0, 2),
    "4B_conv_smgn": (Qu(12, 8, True, RND.CONV, SAT.SMGN), skew, 0, 0),
    "4B_unsigned_zero": (Qu(20, 4, False, RND.INF, SAT.ZERO), 0, 0, 0),
    "4B_smgn_wrap": (Qu(18, 10, True, TRN.SMGN, WRP.TCPL), 0, 0, 0),
    "8B_sat": (Qu(29, 16), 0, 0, 2),                                        # never at its bounds
    "8B_neginf_sat": (Qu(40, 6, True, RND.NEG_INF, SAT.TCPL), 0, 0, 2),     # never at its bounds
    "1B_sat": (Qu(2, 5), 1, 1, 0),
    "2B_sat": (Qu(2, 13), 1, 1, 0),
}


@pytest.mark.parametrize("e", [E43, E88], ids=["1x1", "3x3"])
@pytest.mark.parametrize("mode", sorted(MODES))
def test_every_container_and_mode_of_c(ctx, oracle, mode, e):
    """A single-limb member whose conversion needs more than 30 value bits in C (or a left shift beyond 31) has no one-launch form:
    raw dot products and a conversion pass, two launches per member — recorded in MODES and asserted.  Condition on the data,
    checked on the oracle's own output: a saturating C that the case's largest dot product (K max|a| max|b|) exceeds has between
    1 % and 99 % of its elements at its bounds; one that holds it has none there; the wrapping C holds more than 100 values."""
    ec, data43, data88, per_member43 = MODES[mode]
    data = data43 if e is E43 else data88
    M, N, K = 65, 33, 100
    d = lower(e, e, ec, M, N, K, **tags(e, e))
    exp = check(ctx, oracle, d, e, e, ec, (3,), [LIMBS[e]] * 2, per_member=per_member43 if e is E43 else 0, seed=3000,
                dists=(data,) if isinstance(data, int) else (0,), edit=None if isinstance(data, int) else data)
    out = np.concatenate(exp).astype(np.int64)
    lo, hi = (0 if ec.OfMode == SAT.ZERO else -ec.raw_max if ec.OfMode == SAT.SMGN else ec.raw_min), ec.raw_max
    if ec.OfMode == WRP.TCPL:
        assert len(np.unique(out)) > 100
        return
    at_bounds = float(np.mean((out == lo) | (out == hi)))
    reach = K * max(abs(e.raw_min), e.raw_max) ** 2 / 2.0 ** (2 * e.fracBits - ec.fracBits)       # in C's raw units
    if reach > hi or not ec.isSigned:
        assert 0.01 <= at_bounds <= 0.99, at_bounds
    else:
        assert at_bounds == 0.0 and len(np.unique(out)) > 100


# ---- e. tall and wide members: the walk's groups of 8 tile rows, a ragged last group, many tile columns
@pytest.mark.parametrize("M,N,K,batch", [(577, 70, 130, 3), (70, 1030, 130, 2), (1089, 65, 65, 2)], ids=["10x2_tiles", "2x17_tiles", "18x2_tiles"])
@pytest.mark.parametrize("e", [E43, E88], ids=["1x1", "3x3"])
def test_tall_and_wide_members(ctx, oracle, e, M, N, K, batch):
    ec = roomy(e, e)
    d = lower(e, e, ec, M, N, K, **tags(e, e))
    info = planned(d, batch, [LIMBS[e]] * 2, 1)
    cb = 4 if ec.storage_bits <= 32 else 8
    assert info.packed_bytes[2] == batch * ((M + 63) // 64) * ((N + 63) // 64) * 64 * 64 * cb          # 64x64 tiles, that many per member
    check(ctx, oracle, d, e, e, ec, (batch,), [LIMBS[e]] * 2, seed=4000)


# ---- f. a Karatsuba-eligible member: base-64 digits and three products in the plain plan, balanced limbs and four in the batch
@pytest.mark.parametrize("M,N,K", [(64, 64, 64), (65, 33, 193)])
def test_karatsuba_eligible_member(ctx, oracle, M, N, K):
    """(The plain plan's reason does not name the Karatsuba form; its packed layout does: int64 row sums behind the planes and the
    plane-mask trailer, as tests/test_gpu_parity.py::test_karatsuba_two_digit_kernel reads it.)"""
    ec = roomy(E55, E55)
    d = lower(E55, E55, ec, M, N, K, **tags(E55, E55))
    p = capi.classify(d)
    rows_p, k_p = (M + 127) // 128 * 128, (K + 63) // 64 * 64
    kara = p.packed_bytes[0] == 2 * rows_p * k_p + 256 + 8 * rows_p
    assert kara == ((M, N, K) == (64, 64, 64))             # 128x128 tiles: Karatsuba; (65, 33): 64x64 tiles, schoolbook limbs
    info = planned(d, 7, [2, 2], 1)
    assert info.packed_bytes[0] == 7 * 2 * ((M + 63) // 64 * 64) * k_p + 256          # two balanced limb planes per member, no row sums
    check(ctx, oracle, d, E55, E55, ec, (7,), [2, 2], seed=5000)


# ---- g. fallbacks that execute through qgemul_execute_batched
def composite_launches(d):
    """k-chunks x (limb-group sub-GEMMs + the combine pass), from the plain plan's reason"""
    m = re.search(rb"(\d+) k-chunk\(s\) x (\d+) x (\d+) limb groups", bytes(capi.classify(d).reason))
    assert m, capi.classify(d).reason
    nc, ga, gb = map(int, m.groups())
    return nc * (ga * gb + 1)


def test_composite_k_chunk_members(ctx, oracle):
    ec = Qu(30, 3)
    d = lower(E43, E43, ec, 5, 3, 140000, mul_args=Tags(9, 6), add_args=[Qu(27, 6)])
    per = composite_launches(d)
    assert per == 4                                        # two k-chunks x (one sub-GEMM + the combine pass)
    check(ctx, oracle, d, E43, E43, ec, (2,), [1, 1], per_member=per, seed=6000)


def test_four_limb_members(ctx, oracle):
    ec = roomy(E12, E12)
    d = lower(E12, E12, ec, 33, 17, 40, **tags(E12, E12))
    per = composite_launches(d)
    assert per == 5                                        # 2 x 2 limb groups + the combine pass
    check(ctx, oracle, d, E12, E12, ec, (3,), [4, 4], per_member=per, seed=6100)


def test_complex_member_of_the_linear_class(ctx, oracle):
    cw = Qcomplex(Qu(18, 6, True, RND.POS_INF, SAT.TCPL), Qu(18, 6, True, RND.POS_INF, SAT.TCPL))
    c55 = Qcomplex(Qu(5, 5), Qu(5, 5))
    d = lower(c55, c55, cw, 33, 17, 40)
    p = capi.classify(d)
    per = capi.classify_batched_launches(d, 3) // 3
    if capi.KERNEL_NAMES[p.kernel] == "mfma_cplx":
        assert per == 2                                    # the MFMA kernel + the combine pass
    check(ctx, oracle, d, c55, c55, cw, (3,), list(p.limbs), per_member=per, dists=(1,), seed=6200)


@pytest.mark.parametrize("e,M,ec,why,back", [(E43, 4096, Qu(16, 3), b"", 300), (E88, 2048, Qu(24, 8), b"six products", 100)], ids=["256x256_tiles", "six_product_kernel"])
def test_members_of_the_two_group_kernels(ctx, oracle, e, M, ec, why, back):
    """a member that fills the GPU alone has no block-diagonal form: one plain launch per member, on the plain plan's own layout.
    Three oracle blocks per member (first tile, rows of the last-but-one tile row `back` rows from the end, last corner); the plain
    plan over the whole C."""
    K, batch = 64, 2
    d = lower(e, e, ec, M, M, K, **tags(e, e, 11 if e is E43 else 13))
    info = planned(d, batch, [LIMBS[e]] * 2, batch)
    p = capi.classify(d)
    assert why in bytes(p.reason) and list(info.packed_bytes) == [batch * b for b in p.packed_bytes]
    n = M * K
    A, mA = host_batch(oracle, e, batch, n, n + 3, 7000, (0, 1))
    B, mB = host_batch(oracle, e, batch, n, n + 5, 7500, (0, 1))
    stride_c = M * M + 7
    got, launches = run_batched_plan(ctx, oracle, d, ec, batch, A, B, (n + 3, n + 5, stride_c))
    assert launches == batch
    plain = run_plain_members(ctx, oracle, d, ec, mA, mB)
    cdt = oracle.host_dtype(ec)
    for b in range(batch):
        c = got[b * stride_c:b * stride_c + M * M]
        assert np.array_equal(c, plain[b]), b
        for rows, cols in (((0, 8), (0, 256)), ((M - back, M - back + 8), (M - 200, M)), ((M - 6, M), (M - 130, M))):
            exp = np.zeros(M * M, dtype=cdt)
            oracle.gemm(d, mA[b], mB[b], ec, rows=rows, cols=cols, nthreads=16, out=exp)
            sl = (slice(cols[0], cols[1]), slice(rows[0], rows[1]))
            assert np.array_equal(c.reshape(M, M)[sl], exp.reshape(M, M)[sl]), (b, rows, cols)
            assert b or len(np.unique(exp.reshape(M, M)[sl])) > 100           # (member 1 holds small values)
    gap = got[M * M:stride_c].view(np.uint8)
    assert gap.size and np.all(gap == POISON)


# ---- h. packing twice into the same packed buffers
@pytest.mark.parametrize("name,e,ec,kw,limbs", [("3x3", E88, Qu(24, 8), tags(E88, E88), [3, 3]),
                                                ("centred", Q78, Qu(20, 8), dict(mul_args=Tags(15, 16), add_args=[Qu(28, 16)]), [2, 2])], ids=["3x3", "centred"])
def test_packing_a_second_batch_into_the_same_buffers(ctx, oracle, name, e, ec, kw, limbs):
    """qg_launch_pack_stack clears the stack's plane mask and row sums once per call and the members OR / add into them: a second
    pack must not see the first one's.  Full-range members first (third plane in use, large row sums), then small ones."""
    M, N, K, batch = 65, 33, 100, 2
    d = lower(e, e, ec, M, N, K, **kw)
    planned(d, batch, limbs, 1)
    extA, extB, extC = extents(d)
    sA, sB = extA + 5, extB + 3
    plan = capi.BatchedPlan(ctx, d, batch)
    pb = plan.info.packed_bytes
    nA, nB = (batch - 1) * sA + extA, (batch - 1) * sB + extB
    cdt = oracle.host_dtype(ec)
    bufs = [ctx.alloc(nA * 4), ctx.alloc(nB * 4), ctx.alloc(batch * extC * np.dtype(cdt).itemsize), ctx.alloc(pb[0]), ctx.alloc(pb[1]), ctx.alloc(pb[2])]
    dA, dB, dC, pA, pB, pC = bufs
    try:
        assert plan.launches == 1
        for dist, third_plane in ((0, True), (1, False)):
            A, mA = host_batch(oracle, e, batch, extA, sA, 8000 + dist, (dist,))
            B, mB = host_batch(oracle, e, batch, extB, sB, 8500 + dist, (dist,))
            assert A.nbytes == nA * 4 and B.nbytes == nB * 4
            ctx.h2d(dA, A.view(np.uint8)); ctx.h2d(dB, B.view(np.uint8))
            plan.pack(capi.OPERAND_A, dA, pA, sA)
            plan.pack(capi.OPERAND_B, dB, pB, sB)
            plan.execute(pC, pA, pB)
            plan.unpack_c(pC, dC, extC)
            ctx.sync()
            if name == "3x3":
                for operand, packed in ((capi.OPERAND_A, pA), (capi.OPERAND_B, pB)):
                    mask = read_mask(ctx, plan, packed, operand)
                    assert bool(mask & 4) == third_plane and (mask & 3) == 3, (dist, operand, mask)
            got = np.zeros(batch * extC, dtype=cdt)
            ctx.d2h(got.view(np.uint8), dC)
            exp = [oracle.gemm(d, a, b, ec, nthreads=8) for a, b in zip(mA, mB)]
            assert got.tobytes() == np.concatenate(exp).tobytes(), dist
            assert len(np.unique(np.concatenate(exp))) > 100
            plain = run_plain_members(ctx, oracle, d, ec, mA, mB)
            for b in range(batch):
                assert plain[b].tobytes() == exp[b].tobytes(), (dist, b)
    finally:
        for p in bufs:
            ctx.free(p)
        plan.close()
