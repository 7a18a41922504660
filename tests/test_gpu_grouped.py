"""Grouped Qgemul on the GPU (run with -m gpu): GEMMs of DIFFERENT shapes, the eligible members of one launch key in ONE launch of
k_mfma_grp, every other member on its own plain plan through the same entry points.  Every case is compared, member by member,
with the oracle (qoracle_gemm) AND byte for byte with that member through a plain plan.  C buffers are poisoned: bytes outside the
members must survive.  The shapes are the smallest at which the schedule table (per-member tile counts and k-loop lengths, the
dealt block ids), the padding, the launch-wide data (ONE plane mask and ONE row-sum array, K biasA biasB per member) or the
stragglers' offsets can go wrong.

A condition keeps equality meaningful (checked on the oracle's values, before anything is compared): in every case the expected
values of the members filled with distribution 1 hold more than 20 distinct values, and for a signed C fewer than half of them sit
at C's range ends."""
import hashlib
import os
import subprocess

import numpy as np
import pytest

from qublas_amd import capi
from qublas_amd.desc import Qcomplex, Qu, RND, SAT, TRN, WRP, Tags, TFComplexMul, lower

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLANG = "/opt/rocm/lib/llvm/bin/clang++"

E43, E88, E77, U8, Q78 = Qu(4, 3), Qu(8, 8), Qu(7, 7), Qu(8, 0, False), Qu(7, 8)
# (the table of tests/test_gpu_batched.py, copied)
# name -> (A element, B element, C element, lowering keywords, transposed A, limbs the planner must report)
FORMATS = {
    "e43_c1byte": (E43, E43, Qu(4, 3), dict(mul_args=Tags(9, 6), add_args=[Qu(19, 6)]), False, [1, 1]),
    "e88_3x3": (E88, E88, Qu(24, 8), dict(mul_args=Tags(17, 16), add_args=[Qu(29, 16)]), False, [3, 3]),
    "e77_2x2": (E77, E77, Qu(20, 7), dict(mul_args=Tags(15, 14), add_args=[Qu(27, 14)]), False, [2, 2]),
    "u8_centred": (U8, U8, Qu(26, 0, False), dict(mul_args=Tags(16, 0, False), add_args=[Qu(28, 0, False)]), False, [1, 1]),
    "q78_centred": (Q78, Q78, Qu(20, 8), dict(mul_args=Tags(15, 16), add_args=[Qu(28, 16)]), False, [2, 2]),
    "e88_x_e43_3x1": (E88, E43, Qu(20, 8), dict(mul_args=Tags(13, 11), add_args=[Qu(25, 11)]), False, [3, 1]),
    "e88_3x3_tn": (E88, E88, Qu(24, 8), dict(mul_args=Tags(17, 16), add_args=[Qu(29, 16)]), True, [3, 3]),
}
# 1 x 1, 2 x 1 and 3 x 3 tile members; 1 to 11 k-tiles of 64 bytes, 1 to 6 of 128: the three-stage ring refilled and wrapped in some
# workgroups and never filled in others; 7 members: no multiple of 8
SHAPES = [(1, 1, 1), (3, 5, 7), (64, 64, 64), (65, 33, 100), (129, 130, 65), (64, 64, 300), (130, 10, 700)]
POISON = 0x5a

C5 = Qcomplex(Qu(6, 3, True, RND.POS_INF, SAT.TCPL), Qu(6, -3, True, RND.POS_INF, SAT.TCPL))
I16 = Qu(15, 0, True, TRN.TCPL, WRP.TCPL)
FALLBACKS = {
    # name -> (operand element, C element, lowering keywords, launches per member)   (tests/test_gpu_batched.py, copied)
    "tree_default_tags": (E88, E88, {}, 1),
    "complex_tf": (C5, C5, dict(mul_args=TFComplexMul()), 1),
    "ring_int16": (I16, I16, {}, 1),
    "raw_pass_left_shift": (Qu(10, -3), Qu(24, 9), dict(mul_args=Tags(21, -6), add_args=[Qu(28, -6)]), 2),
}


class Member:
    """one GEMM of a group: its formats, descriptor, leading dimensions, host operands, the oracle's C"""

    def __init__(self, oracle, ea, eb, ec, shape, kw, ta=False, seed=1, dist=0, ld=(0, 0, 0)):
        M, N, K = shape
        self.ea, self.eb, self.ec, self.dist, self.ld = ea, eb, ec, dist, ld
        self.d = lower(ea, eb, ec, M, N, K, transposed_a=ta, **kw)
        self.empty = M == 0 or N == 0
        ra, ca = (K, M) if ta else (M, K)
        self.ext = ((ca - 1) * (ld[0] or ra) + ra if ca else 0, (N - 1) * (ld[1] or K) + K if N else 0, (N - 1) * (ld[2] or M) + M if M and N else 0)
        self.A = oracle.fill(ea, max(self.ext[0], 1), seed, dist)
        self.B = oracle.fill(eb, max(self.ext[1], 1), seed + 1000, dist)
        self._exp = None

    def expected(self, oracle):
        """the poisoned C buffer as it must look afterwards: the member's columns at ldc, poison between them"""
        if self._exp is None:
            M, N = self.d.M, self.d.N
            buf = np.empty(max(self.ext[2], 1), dtype=oracle.host_dtype(self.ec))
            buf.view(np.uint8)[:] = POISON
            if not self.empty:
                out = np.zeros(self.ext[2] + M, dtype=oracle.host_dtype(self.ec))
                oracle.gemm(self.d, self.A, self.B, self.ec, lda=self.ld[0], ldb=self.ld[1], ldc=self.ld[2], out=out, nthreads=8)
                ldc = self.ld[2] or M
                for j in range(N):
                    buf[j * ldc:j * ldc + M] = out[j * ldc:j * ldc + M]
            self._exp = buf
        return self._exp

    def values(self, oracle):
        """the member's own C values (without the poison), real parts of a complex C"""
        M, N = self.d.M, self.d.N
        ldc = self.ld[2] or M
        e = self.expected(oracle)
        v = np.concatenate([e[j * ldc:j * ldc + M] for j in range(N)]) if not self.empty else e[:0]
        return v["re"] if v.dtype.names else v


def fmt_member(oracle, fmt, shape, **kw2):
    ea, eb, ec, kw, ta, _ = FORMATS[fmt]
    return Member(oracle, ea, eb, ec, shape, kw, ta=kw2.pop("ta", ta), **kw2)


def assert_meaningful(oracle, members):
    """the condition of the module's docstring, on the oracle's values of the members filled with distribution 1"""
    pool, ends, n = [], 0, 0
    for m in members:
        if m.dist != 1 or m.empty:
            continue
        v = np.asarray(m.values(oracle)).astype(object)
        pool.append(v)
        c = m.ec.real if isinstance(m.ec, Qcomplex) else m.ec
        if c.isSigned:
            ends += int(sum(1 for x in v if x == c.raw_min or x == c.raw_max))
        n += len(v)
    assert pool, "a case needs members filled with distribution 1"
    distinct = len(set(np.concatenate(pool).tolist()))
    assert distinct > 20, distinct
    assert 2 * ends < n, (ends, n)


def up256(x):
    return (x + 255) // 256 * 256


def run_grouped_plan(ctx, oracle, members, flags=0):
    """pack_grouped + execute_grouped + unpack_c_grouped into poisoned C buffers; returns (the C buffers, the plan's launch count,
    the members' records)"""
    descs = [m.d for m in members]
    plan = capi.GroupedPlan(ctx, descs, flags)
    host = [[m.A for m in members], [m.B for m in members], []]
    for m in members:
        c = np.empty(max(m.ext[2], 1), dtype=oracle.host_dtype(m.ec))
        c.view(np.uint8)[:] = POISON
        host[2].append(c)
    offs, tot = [[], [], []], [0, 0, 0]
    for w in range(3):
        for x in host[w]:
            offs[w].append(tot[w])
            tot[w] += up256(x.nbytes)
    pb = plan.info.packed_bytes
    bufs = [ctx.alloc(max(16, t)) for t in tot] + [ctx.alloc(max(16, b)) for b in pb]
    dev, packed = bufs[:3], bufs[3:]
    try:
        for w in range(3):
            for x, o in zip(host[w], offs[w]):
                ctx.h2d(dev[w] + o, x.view(np.uint8))
        ptrs = [[0 if m.empty else dev[w] + o for m, o in zip(members, offs[w])] for w in range(3)]
        lds = [[m.ld[w] for m in members] for w in range(3)]
        tight = all(m.ld == (0, 0, 0) for m in members)
        plan.pack(capi.OPERAND_A, ptrs[0], packed[0], None if tight else lds[0])
        plan.pack(capi.OPERAND_B, ptrs[1], packed[1], None if tight else lds[1])
        plan.execute(packed[2], packed[0], packed[1])
        plan.unpack_c(packed[2], ptrs[2], None if tight else lds[2])
        ctx.sync()
        for x, o in zip(host[2], offs[2]):
            ctx.d2h(x.view(np.uint8), dev[2] + o)
        recs = [plan.member(g) for g in range(len(members))]
        return host[2], plan.launches, recs
    finally:
        for p in bufs:
            ctx.free(p)
        plan.close()


def run_plain(ctx, oracle, m):
    """one member through a PLAIN plan: qgemul_pack, qgemul_execute, qgemul_unpack_c into a poisoned C"""
    plan = capi.Plan(ctx, m.d)
    pb = plan.info.packed_bytes
    c = np.empty(max(m.ext[2], 1), dtype=oracle.host_dtype(m.ec))
    c.view(np.uint8)[:] = POISON
    bufs = [ctx.alloc(max(16, m.A.nbytes)), ctx.alloc(max(16, m.B.nbytes)), ctx.alloc(max(16, c.nbytes)), ctx.alloc(max(16, pb[0])), ctx.alloc(max(16, pb[1])), ctx.alloc(max(16, pb[2]))]
    dA, dB, dC, pA, pB, pC = bufs
    try:
        ctx.h2d(dA, m.A.view(np.uint8)); ctx.h2d(dB, m.B.view(np.uint8)); ctx.h2d(dC, c.view(np.uint8))
        plan.pack(capi.OPERAND_A, dA, pA, m.ld[0])
        plan.pack(capi.OPERAND_B, dB, pB, m.ld[1])
        plan.execute(pC, pA, pB)
        plan.unpack_c(pC, dC, m.ld[2])
        ctx.sync()
        ctx.d2h(c.view(np.uint8), dC)
        return c
    finally:
        for p in bufs:
            ctx.free(p)
        plan.close()


def check_group(ctx, oracle, members, plain=None, flags=0):
    """the whole comparison of one case; plain: the members to send through a plain plan as well (None: all).  Returns (launches, records)"""
    assert_meaningful(oracle, members)
    exp = [m.expected(oracle) for m in members]
    got, launches, recs = run_grouped_plan(ctx, oracle, members, flags)
    # (the figures first, then the assertions: run with -s to see them)
    print(f"grouped case: members={len(members)} in_launch={sum(r.in_launch for r in recs)} tiles={sum(r.tiles_m * r.tiles_n for r in recs)} launches={launches} "
          f"got={hashlib.sha1(b''.join(g.tobytes() for g in got)).hexdigest()[:12]} exp={hashlib.sha1(b''.join(e.tobytes() for e in exp)).hexdigest()[:12]}")
    assert launches == capi.classify_grouped_launches([m.d for m in members], flags)
    for g, m in enumerate(members):
        assert got[g].tobytes() == exp[g].tobytes(), (g, m.d.M, m.d.N, m.d.K)
    for g in (range(len(members)) if plain is None else plain):
        if members[g].empty or getattr(members[g], "plain_ok", False):
            continue
        assert run_plain(ctx, oracle, members[g]).tobytes() == exp[g].tobytes(), g
        members[g].plain_ok = True   # (a member shared between cases goes through its plain plan once)
    return launches, recs


@pytest.fixture(scope="module")
def ctx():
    with capi.Context() as c:
        yield c


_BASE = {}


def base_members(oracle, fmt):
    """the seven shapes in one format, made once and shared by the orders: distributions 0 and 1 alternate"""
    if fmt not in _BASE:
        _BASE[fmt] = [fmt_member(oracle, fmt, s, seed=100 + 7 * i, dist=i % 2) for i, s in enumerate(SHAPES)]
    return _BASE[fmt]


ORDERS = {"list": [0, 1, 2, 3, 4, 5, 6], "reversed": [6, 5, 4, 3, 2, 1, 0], "nine_with_repeats": [3, 0, 6, 3, 4, 1, 6, 2, 5]}


@pytest.mark.parametrize("order", sorted(ORDERS))
@pytest.mark.parametrize("fmt", sorted(FORMATS))
def test_mixed_shapes_in_one_launch(ctx, oracle, fmt, order):
    base = base_members(oracle, fmt)
    members = [base[i] for i in ORDERS[order]]
    st, info = capi.classify_grouped_status([m.d for m in members])
    assert st == capi.QG_OK and list(info.limbs) == FORMATS[fmt][5], info.reason
    launches, recs = check_group(ctx, oracle, members)
    assert launches == 1                                    # (the 3 x 3 pair counts once)
    assert all(r.in_launch == 1 and r.launches == 0 for r in recs)
    bk = 128 if FORMATS[fmt][5] == [1, 1] else 64
    for m, r in zip(members, recs):
        assert (r.tiles_m, r.tiles_n, r.k_tiles) == ((m.d.M + 63) // 64, (m.d.N + 63) // 64, (m.d.K + bk - 1) // bk)


@pytest.mark.parametrize("fmt", ["u8_centred", "q78_centred"])
def test_per_member_k_with_centred_operands(ctx, oracle, fmt):
    """K biasA biasB is the MEMBER's: a corr taken from the wrong member changes every output"""
    members = [fmt_member(oracle, fmt, (33, 17, K), seed=300 + i, dist=1 if i % 2 == 0 else 0) for i, K in enumerate((1, 64, 65, 1000))]
    launches, recs = check_group(ctx, oracle, members)
    assert launches == 1 and all(r.in_launch for r in recs)


def launch_trailer_mask(ctx, recs, packed, operand):
    """the launch's ONE plane mask: the trailer behind the last member in the launch"""
    trailer = max(r.off[operand] + r.bytes[operand] for r in recs if r.in_launch)
    w = np.zeros(64, dtype=np.uint32)
    ctx.d2h(w.view(np.uint8), packed + trailer)
    return int(np.bitwise_or.reduce(w))


@pytest.mark.parametrize("dists,third_plane", [((1, 0), True), ((1, 1), False)], ids=["small_then_full_range", "all_small"])
def test_plane_mask_of_the_launch_is_the_or_over_every_member(ctx, oracle, dists, third_plane):
    """int<8,8> in three limb planes, two members of DIFFERENT shapes.  One small (the third plane is empty), one full range: the
    launch's one mask must keep the third plane whichever is packed first; with both small the 2 x 2 partner of the pair does the work"""
    shapes = [(65, 33, 100), (3, 130, 7)]
    for order in (dists, dists[::-1]):
        members = [fmt_member(oracle, "e88_3x3", s, seed=500 + i, dist=order[i]) for i, s in enumerate(shapes)]
        launches, recs = check_group(ctx, oracle, members)
        assert launches == 1
        plan = capi.GroupedPlan(ctx, [m.d for m in members])
        pb = plan.info.packed_bytes
        bufs = [ctx.alloc(up256(m.A.nbytes)) for m in members] + [ctx.alloc(up256(m.B.nbytes)) for m in members] + [ctx.alloc(pb[0]), ctx.alloc(pb[1])]
        try:
            for p, x in zip(bufs, [m.A for m in members] + [m.B for m in members]):
                ctx.h2d(p, x.view(np.uint8))
            plan.pack(capi.OPERAND_A, bufs[0:2], bufs[4])
            plan.pack(capi.OPERAND_B, bufs[2:4], bufs[5])
            ctx.sync()
            for operand, packed in ((0, bufs[4]), (1, bufs[5])):
                mask = launch_trailer_mask(ctx, recs, packed, operand)
                assert bool(mask & 4) == third_plane and (mask & 3) == 3, (order, operand, mask)
        finally:
            for p in bufs:
                ctx.free(p)
            plan.close()


def test_longest_k_loop_beside_the_shortest(ctx, oracle):
    """single limb: min(LA, LB) K = 2^17 - 1 is the longest k-loop a member of the launch can have (1024 k-tiles), beside members of one"""
    shapes = [(33, 17, 1), (1, 1, 131071), (1, 1, 1), (64, 64, 1), (1, 1, 1)]
    # (the level type holds K = 2^17 - 1 products exactly; C widened to Qu(13, 6), which keeps every product bit: one product of two small values has 16 values after C = Qu(4, 3) drops three bits)
    kw = dict(mul_args=Tags(9, 6), add_args=[Qu(26, 6)])
    members = [Member(oracle, E43, E43, Qu(13, 6), s, kw, seed=600 + i, dist=1 if i % 3 == 0 else 0) for i, s in enumerate(shapes)]
    launches, recs = check_group(ctx, oracle, members)
    assert launches == 1 and all(r.in_launch for r in recs)
    assert [r.k_tiles for r in recs] == [1, 1024, 1, 1, 1]


@pytest.mark.parametrize("fmt", ["e43_c1byte", "e88_3x3"])
def test_more_workgroups_than_cus(ctx, oracle, fmt):
    rng = np.random.RandomState(20261019)
    shapes = [(int(rng.randint(1, 131)), int(rng.randint(1, 131)), int(rng.randint(1, 301))) for _ in range(300)]
    members = [fmt_member(oracle, fmt, s, seed=700 + i, dist=i % 2) for i, s in enumerate(shapes)]
    launches, recs = check_group(ctx, oracle, members, plain=[0, 1, 7, 8, 9, 63, 64, 150, 299])
    assert launches == 1 and all(r.in_launch for r in recs)
    assert sum(r.tiles_m * r.tiles_n for r in recs) > 256


def eligible_e43(oracle):
    return [fmt_member(oracle, "e43_c1byte", (3, 5, 7), seed=800, dist=0), fmt_member(oracle, "e43_c1byte", (65, 33, 100), seed=801, dist=1)]


@pytest.mark.parametrize("name", sorted(FALLBACKS))
def test_straggler_kinds_run_alone_through_the_same_entry(ctx, oracle, name):
    e, ec, kw, per_member = FALLBACKS[name]
    el = eligible_e43(oracle)
    s1 = Member(oracle, e, e, ec, (33, 17, 40), kw, seed=810, dist=1)
    s2 = Member(oracle, e, e, ec, (5, 9, 40), kw, seed=811, dist=1)
    members = [s1, el[0], s2, el[1]]
    launches, recs = check_group(ctx, oracle, members)
    assert [r.in_launch for r in recs] == [0, 1, 0, 1]
    assert launches == 1 + 2 * per_member and [r.launches for r in recs] == [per_member, 0, per_member, 0]
    for w in range(3):   # stragglers at 256-byte-aligned offsets behind the launch's part
        assert recs[0].off[w] % 256 == 0 and recs[2].off[w] % 256 == 0 and recs[0].off[w] >= recs[3].off[w] + recs[3].bytes[w]


def test_a_second_key_runs_alone(ctx, oracle):
    """int<8,8> members first: theirs is the launch's key; the int<4,3> members behind them are eligible but have another key"""
    members = [fmt_member(oracle, "e88_3x3", (65, 33, 100), seed=820, dist=1), fmt_member(oracle, "e88_3x3", (3, 5, 7), seed=821, dist=0)] + eligible_e43(oracle)
    launches, recs = check_group(ctx, oracle, members)
    assert [r.in_launch for r in recs] == [1, 1, 0, 0] and launches == 3


def test_a_member_of_two_group_kernel_size_runs_alone(ctx, oracle):
    """single limb, 4096 x 4096 x 64: the plain planner gives it 256 x 256 tiles of the two-group kernel; sampled rows against the oracle"""
    ea, eb, ec, kw, _, _ = FORMATS["e43_c1byte"]
    el = eligible_e43(oracle)
    big = lower(ea, eb, ec, 4096, 4096, 64, **kw)
    descs = [el[0].d, big, el[1].d]
    assert capi.classify_grouped_launches(descs) == 2
    assert_meaningful(oracle, el)
    A, B = oracle.fill(ea, 4096 * 64, 830, 1), oracle.fill(eb, 64 * 4096, 831, 1)
    plan = capi.GroupedPlan(ctx, descs)
    assert plan.launches == 2 and [plan.member(g).in_launch for g in range(3)] == [1, 0, 1]
    hostA, hostB = [el[0].A, A, el[1].A], [el[0].B, B, el[1].B]
    nC = [m.ext[2] for m in el]
    nC = [nC[0], 4096 * 4096, nC[1]]
    pb = plan.info.packed_bytes
    bufs = [ctx.alloc(up256(x.nbytes)) for x in hostA + hostB] + [ctx.alloc(n * 4) for n in nC] + [ctx.alloc(b) for b in pb]
    try:
        for p, x in zip(bufs, hostA + hostB):
            ctx.h2d(p, x.view(np.uint8))
        plan.pack(capi.OPERAND_A, bufs[0:3], bufs[9])
        plan.pack(capi.OPERAND_B, bufs[3:6], bufs[10])
        plan.execute(bufs[11], bufs[9], bufs[10])
        plan.unpack_c(bufs[11], bufs[6:9])
        ctx.sync()
        got = [np.zeros(n, dtype=oracle.host_dtype(ec)) for n in nC]
        for g in range(3):
            ctx.d2h(got[g].view(np.uint8), bufs[6 + g])
    finally:
        for p in bufs:
            ctx.free(p)
        plan.close()
    assert got[0].tobytes() == el[0].expected(oracle).tobytes() and got[2].tobytes() == el[1].expected(oracle).tobytes()
    exp = np.zeros(4096 * 4096, dtype=oracle.host_dtype(ec))
    g2, e2 = got[1].reshape(4096, 4096), exp.reshape(4096, 4096)
    for rows, cols in (((1000, 1024), (0, 512)), ((4090, 4096), (3584, 4096))):
        oracle.gemm(big, A, B, ec, rows=rows, cols=cols, nthreads=16, out=exp)
        sl = (slice(cols[0], cols[1]), slice(rows[0], rows[1]))
        assert np.array_equal(g2[sl], e2[sl])
        assert len(set(e2[sl].ravel().tolist())) > 20


def test_transposed_a_mixed_inside_one_launch(ctx, oracle):
    members = [fmt_member(oracle, "e88_3x3", s, ta=(i % 2 == 1), seed=840 + i, dist=i % 2) for i, s in enumerate(SHAPES[1:6])]
    launches, recs = check_group(ctx, oracle, members)
    assert launches == 1 and all(r.in_launch for r in recs)


@pytest.mark.parametrize("fmt", ["e43_c1byte", "q78_centred", "e88_3x3_tn"])
def test_leading_dimensions_with_poison_and_empty_members(ctx, oracle, fmt):
    ta = FORMATS[fmt][4]
    members = []
    for i, (M, N, K) in enumerate([(65, 33, 100), (0, 5, 7), (3, 130, 7), (9, 0, 64), (64, 64, 65)]):
        ld = ((K if ta else M) + 3 + i, K + 5, M + 7 + i)
        members.append(fmt_member(oracle, fmt, (M, N, K), seed=850 + i, dist=1 if i % 2 == 0 else 0, ld=ld))
    launches, recs = check_group(ctx, oracle, members)
    assert launches == 1
    assert [(r.tiles_m * r.tiles_n) for r in recs] == [2, 0, 3, 0, 1]
    # an ld below the member's rows, a null member pointer
    import ctypes as C
    plan = capi.GroupedPlan(ctx, [m.d for m in members])
    buf = ctx.alloc(1 << 20)
    try:
        n, v = len(members), C.c_void_p
        ptrs = (v * n)(*[v(buf)] * n)
        bad_ld = (C.c_int64 * n)(*[m.ld[2] for m in members])
        bad_ld[0] = members[0].d.M - 1
        L = capi.lib()
        assert L.qgemul_unpack_c_grouped(plan.h, v(buf), ptrs, bad_ld) == capi.QG_EINVAL
        lda = (C.c_int64 * n)(*[m.ld[0] for m in members])
        lda[2] = (members[2].d.K if ta else members[2].d.M) - 1
        assert L.qgemul_pack_grouped(plan.h, 0, ptrs, lda, v(buf)) == capi.QG_EINVAL
        ptrs[4] = None
        assert L.qgemul_pack_grouped(plan.h, 1, ptrs, None, v(buf)) == capi.QG_EINVAL
        ptrs[4], ptrs[1] = v(buf), None     # (an empty member's pointer is not read)
        assert L.qgemul_pack_grouped(plan.h, 1, ptrs, None, v(buf)) == capi.QG_OK
        ctx.sync()
    finally:
        ctx.free(buf)
        plan.close()


@pytest.mark.parametrize("fmt", ["e43_c1byte", "q78_centred", "e88_3x3"])
def test_identical_descriptors_equal_the_batched_call(ctx, oracle, fmt):
    batch = 5
    members = [fmt_member(oracle, fmt, (65, 33, 100), seed=860 + i, dist=i % 2) for i in range(batch)]
    d, ec = members[0].d, members[0].ec
    check_group(ctx, oracle, members, plain=[0])
    extA, extB, extC = members[0].ext
    Cb = np.zeros(batch * extC, dtype=oracle.host_dtype(ec))
    capi.run_batched(d, batch, Cb, np.concatenate([m.A for m in members]), np.concatenate([m.B for m in members]), extC, extA, extB)
    Cs = [np.zeros(extC, dtype=oracle.host_dtype(ec)) for _ in members]
    capi.run_grouped([m.d for m in members], Cs, [m.A for m in members], [m.B for m in members])
    assert np.concatenate(Cs).tobytes() == Cb.tobytes()
    assert capi.classify_grouped_status([d] * batch)[1].packed_bytes[:] == capi.classify_batched_status(d, batch)[1].packed_bytes[:]


def test_plan_kinds_refuse_each_other(ctx):
    import ctypes as C
    ea, eb, ec, kw, _, _ = FORMATS["e43_c1byte"]
    d = lower(ea, eb, ec, 64, 64, 64, **kw)
    gp, bp, pp = capi.GroupedPlan(ctx, [d, d]), capi.BatchedPlan(ctx, d, 2), capi.Plan(ctx, d)
    buf = ctx.alloc(1 << 17)
    L, v = capi.lib(), C.c_void_p
    ptrs = (v * 2)(v(buf), v(buf))
    ms = C.c_float()
    rec = capi.qgemul_grouped_member()
    try:
        # a grouped plan at the plain and the batched entry points
        assert L.qgemul_execute(gp.h, v(buf), v(buf), v(buf)) == capi.QG_EINVAL
        assert L.qgemul_pack(gp.h, 0, v(buf), 0, v(buf)) == capi.QG_EINVAL
        assert L.qgemul_unpack_c(gp.h, v(buf), v(buf), 0) == capi.QG_EINVAL
        assert L.qgemul_fill_packed(gp.h, 0, 1, 0, v(buf)) == capi.QG_EINVAL
        assert L.qgemul_time_execute(gp.h, v(buf), v(buf), v(buf), 0, 1, C.byref(ms)) == capi.QG_EINVAL
        assert L.qgemul_execute_host_c(gp.h, v(buf), 0, v(buf), v(buf)) == capi.QG_EINVAL
        out4 = (C.c_int64 * 4)()
        assert L.qgemul_plan_packed_layout(gp.h, 0, out4) == capi.QG_EINVAL
        assert L.qgemul_execute_batched(gp.h, v(buf), v(buf), v(buf)) == capi.QG_EINVAL
        assert L.qgemul_pack_batched(gp.h, 0, v(buf), 0, 4096, v(buf)) == capi.QG_EINVAL
        assert L.qgemul_unpack_c_batched(gp.h, v(buf), v(buf), 0, 4096) == capi.QG_EINVAL
        assert L.qgemul_time_execute_batched(gp.h, v(buf), v(buf), v(buf), 0, 1, C.byref(ms)) == capi.QG_EINVAL
        assert L.qgemul_plan_batched_launches(gp.h) == capi.QG_EINVAL
        # plain and batched plans at the grouped entry points
        for other in (pp, bp):
            assert L.qgemul_execute_grouped(other.h, v(buf), v(buf), v(buf)) == capi.QG_EINVAL
            assert L.qgemul_pack_grouped(other.h, 0, ptrs, None, v(buf)) == capi.QG_EINVAL
            assert L.qgemul_unpack_c_grouped(other.h, v(buf), ptrs, None) == capi.QG_EINVAL
            assert L.qgemul_time_execute_grouped(other.h, v(buf), v(buf), v(buf), 0, 1, C.byref(ms)) == capi.QG_EINVAL
            assert L.qgemul_plan_grouped_launches(other.h) == capi.QG_EINVAL
            assert L.qgemul_plan_grouped_member(other.h, 0, C.byref(rec)) == capi.QG_EINVAL
        assert L.qgemul_plan_grouped_member(gp.h, 2, C.byref(rec)) == capi.QG_EINVAL
        info = capi.qgemul_info()
        assert L.qgemul_plan_info(gp.h, C.byref(info)) == capi.QG_OK and b"2 members in one launch" in bytes(info.reason)
        assert gp.time_execute(buf, buf + 32768, buf + 65536, 1, 2) > 0
    finally:
        ctx.free(buf)
        for p in (gp, bp, pp):
            p.close()


def test_one_shot_cache_replans_when_one_members_k_changes(oracle):
    """qgemul_run_grouped keeps its plan in the calling thread's one-plan cache, keyed on the whole descriptor list"""
    def group(k_last):
        return [fmt_member(oracle, "q78_centred", s, seed=870 + i, dist=1 if i == 0 else 0) for i, s in enumerate([(65, 33, 100), (3, 5, 7), (33, 17, k_last)])]

    def run(members):
        Cs = [np.zeros(m.ext[2], dtype=oracle.host_dtype(m.ec)) for m in members]
        capi.run_grouped([m.d for m in members], Cs, [m.A for m in members], [m.B for m in members])
        for m, c in zip(members, Cs):
            assert c.tobytes() == m.expected(oracle).tobytes(), (m.d.M, m.d.N, m.d.K)

    g1, g2 = group(64), group(65)
    assert_meaningful(oracle, g1)
    run(g1)
    run(g1)            # the cached plan
    run(g2)            # one member's K changed: re-planned
    m = g1[0]
    c = np.zeros(m.ext[2], dtype=oracle.host_dtype(m.ec))
    capi.run(m.d, c, m.A, m.B)   # a plain call takes the cache ...
    assert c.tobytes() == m.expected(oracle).tobytes()
    run(g2)            # ... and the grouped call takes it back
    run(g1)
    import ctypes as C
    o = capi.qgemul_opts(device=-1, flags=capi.OPT_ALL_DEVICES)
    n = len(g1)
    ptr = lambda xs: (C.c_void_p * n)(*[x.ctypes.data for x in xs])
    Cs = [np.zeros(m.ext[2], dtype=oracle.host_dtype(m.ec)) for m in g1]
    descs = (capi.qgemul_desc * n)(*[m.d for m in g1])
    assert capi.lib().qgemul_run_grouped(descs, n, ptr(Cs), ptr([m.A for m in g1]), ptr([m.B for m in g1]), None, None, None, C.byref(o)) == capi.QG_EUNSUPPORTED
    capi.run_release()


def test_standalone_header_program_runs_grouped(tmp_path):
    """include/QuBLAS_amd.h alone: QgemulGrouped on three triples of different dim<>, one of them QgemulTransposedA<true>, and one
    default-tag triple as a straggler; the program compares every C with the header's own Qgemul of that triple"""
    exe = str(tmp_path / "grouped_run")
    lib = os.path.join(ROOT, "qublas_amd")
    subprocess.check_call([CLANG, "-std=c++20", "-O1", "-I", os.path.join(ROOT, "include"), os.path.join(ROOT, "tests", "binding", "amd_header_grouped_run.cpp"),
                           "-L", lib, "-lqugemm", f"-Wl,-rpath,{lib}", "-o", exe])
    out = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "grouped ok" in out.stdout
