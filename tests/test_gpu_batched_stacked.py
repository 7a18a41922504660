"""The STACKED batched Qgemul on the GPU (QG_OPT_BATCHED_STACKED; run with -m gpu): a batch of complex or real x complex members of the
linear class as ONE block-diagonal MFMA launch over the members' stacked parts (k_mfma_bd into the plan's int64 workspace) plus ONE
block-diagonal combine pass (k_stack_combine_bd).  Every case compares, member by member and byte for byte on both parts of C, the
oracle (qoracle_gemm; tests/mixed_ref.py for mixed members) == the PLAIN plan of one member (qgemul_execute + qgemul_unpack_c) == the
flagged batched plan; the limbs, the form and the launch count (2) the planner answers are asserted BEFORE any device work.  Host
buffers carry poison between the members, and C's gaps must survive.  The shapes are the smallest at which the member block's walk
(1 x 1, 2 x 1 and 3 x 3 part tiles: the four quadrant tiles neighbours in the workspace, and not), the padding (ragged M, N, K on both
k-tile sizes), the store's bounds, or the stack-wide plane mask can go wrong.
Strength: in every comparison at least half of each part's compared outputs are neither zero nor at a bound of C (mixed_ref.strong on
the checker's output); the formats of tests/stacked_cases.py are sized so that nothing saturates at these K."""
import json
import os
import subprocess

import numpy as np
import pytest

import mixed_ref as R
from qublas_amd import capi
from qublas_amd.desc import Qcomplex, Qu, RND, SAT, WRP, lower
from stacked_cases import B8, C8, COMPLEX, L8, LINEAR, UNEQUAL
from test_gpu_batched import POISON, expected_buffer, extents, host_batch, run_plain_members

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLANG = "/opt/rocm/lib/llvm/bin/clang++"
F = capi.OPT_BATCHED_STACKED
STACKED = b"combine pass"   # what only the stacked form's reason says


def fmt(name):
    """(A element, B element, C element, lowering keywords, limbs) of a format name: cc<n> complex x complex with n limbs per part,
    ra<n> / rb<n> real x complex / complex x real (LINEAR), ra13 / ra12 / rb31 / rb21 the unequal limb pairs (UNEQUAL)"""
    if name.startswith("cc"):
        e, ec, kw = COMPLEX["limb" + name[2:]]
        return e, e, ec, kw, [int(name[2:])] * 2
    order, key = name[:2], name[2:]
    if len(key) == 2:
        er, ez, ec, kw = UNEQUAL["limb" + (key if order == "ra" else key[::-1])]
    else:
        er, ez, ec, kw = LINEAR["limb" + key]
    limbs = [int(key[0]), int(key[-1])]
    return (er, ez, ec, kw, limbs) if order == "ra" else (ez, er, ec, kw, limbs)


def container(ec):
    """bytes of C's container: the power of two that holds the wider part's storage bits"""
    b = (max(1 + f.intBits + f.fracBits for f in (ec.real, ec.imag)) + 7) // 8
    return 1 << max(0, (b - 1).bit_length())


def tight(X, ld, rows, cols):
    """the rows x cols tensor inside a column-major buffer of leading dimension ld"""
    buf = np.zeros(cols * ld, dtype=X.dtype)
    buf[:X.size] = X
    return np.ascontiguousarray(buf.reshape(cols, ld)[:, :rows]).reshape(-1)


FORMATS = ["cc1", "cc2", "cc3", "ra1", "rb1", "ra2", "rb2", "ra3", "rb3", "ra13", "rb31", "ra12", "rb21"]


@pytest.fixture(scope="module")
def ctx():
    with capi.Context() as c:
        yield c


def ref(oracle, d, a, b, ec):
    return R.gemm(d, a, b, nthreads=8) if R.is_mixed(d) else oracle.gemm(d, a, b, ec, nthreads=8)


def planned(d, batch, limbs):
    """what the planner answers under the flag, asserted before any device work"""
    st, info = capi.classify_batched_status(d, batch, F)
    assert st == capi.QG_OK and list(info.limbs) == list(limbs), (st, list(info.limbs), info.reason)
    assert capi.KERNEL_NAMES[info.kernel] == ("mfma_rc" if R.is_mixed(d) else "mfma_cplx"), info.reason
    assert capi.classify_batched_launches(d, batch, F) == 2 and STACKED in bytes(info.reason), info.reason
    return info


def run_stacked(ctx, oracle, d, ec, batch, A, B, strides, ld=(0, 0, 0), executes=1, packed_c=None):
    """pack_batched + execute_batched (executes times into the same buffers) + unpack_c_batched into a poisoned C through a flagged
    batched plan; returns the C buffer.  packed_c: a list that receives the plan's packed C (bytes; poisoned before the execute)"""
    extC = extents(d, *ld)[2]
    C = np.empty((batch - 1) * strides[2] + extC, dtype=oracle.host_dtype(ec))
    C.view(np.uint8)[:] = POISON
    plan = capi.BatchedPlan(ctx, d, batch, F)
    pb = plan.info.packed_bytes
    bufs = [ctx.alloc(max(16, A.nbytes)), ctx.alloc(max(16, B.nbytes)), ctx.alloc(max(16, C.nbytes)), ctx.alloc(max(16, pb[0])), ctx.alloc(max(16, pb[1])), ctx.alloc(max(16, pb[2]))]
    dA, dB, dC, pA, pB, pC = bufs
    try:
        assert plan.launches == 2
        raw = np.full(max(16, pb[2]), 0xA5, dtype=np.uint8)
        ctx.h2d(dA, A.view(np.uint8)); ctx.h2d(dB, B.view(np.uint8)); ctx.h2d(dC, C.view(np.uint8)); ctx.h2d(pC, raw)
        plan.pack(capi.OPERAND_A, dA, pA, strides[0], ld[0])
        plan.pack(capi.OPERAND_B, dB, pB, strides[1], ld[1])
        for _ in range(executes):
            plan.execute(pC, pA, pB)
        plan.unpack_c(pC, dC, strides[2], ld[2])
        ctx.sync()
        ctx.d2h(C.view(np.uint8), dC)
        if packed_c is not None:
            ctx.d2h(raw, pC)
            packed_c.append(raw)
        return C
    finally:
        for p in bufs:
            ctx.free(p)
        plan.close()


def check(ctx, oracle, d, ea, eb, ec, batches, limbs, dists=(0, 1), seed=1000, edit=None, strong=True):
    """members of max(batches) generated once; oracle == plain plan == flagged batched plan for every batch count.  edit(mA, mB): changes
    the members in place.  Returns (the members' expected Cs, A's members, B's members)"""
    nb = max(batches)
    for batch in batches:
        planned(d, batch, limbs)
    extA, extB, extC = extents(d)
    strides = (extA + 3, extB + 5, extC + 7)
    A, mA = host_batch(oracle, ea, nb, extA, strides[0], seed, dists)
    B, mB = host_batch(oracle, eb, nb, extB, strides[1], seed + 500, dists)
    if edit:
        edit(mA, mB)
        for b in range(nb):
            A[b * strides[0]:b * strides[0] + extA] = mA[b]
            B[b * strides[1]:b * strides[1] + extB] = mB[b]
    exp = [ref(oracle, d, a, b, ec) for a, b in zip(mA, mB)]
    if strong:
        assert all(R.strong(d, e) for e in exp)
    plain = run_plain_members(ctx, oracle, d, ec, mA, mB)
    for b in range(nb):
        assert plain[b].tobytes() == exp[b].tobytes(), ("plain plan", b)
    for batch in batches:
        got = run_stacked(ctx, oracle, d, ec, batch, A[:(batch - 1) * strides[0] + extA], B[:(batch - 1) * strides[1] + extB], strides)
        assert got.tobytes() == expected_buffer(oracle, d, ec, batch, exp, strides[2]).tobytes(), batch
    return exp, mA, mB


# ---- a. tile counts: members of 1 x 1, 1 x 1 (full), 2 x 1 and 3 x 3 part tiles; one ragged k-tile and several with a ragged tail
SHAPES = [(33, 17), (64, 64), (65, 40), (130, 170)]


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
@pytest.mark.parametrize("name", FORMATS)
def test_tile_counts(ctx, oracle, name, shape):
    ea, eb, ec, kw, limbs = fmt(name)
    M, N = shape
    for K in (40, 264 if limbs == [1, 1] else 200):   # (128-byte k-tiles for the single-limb pair, 64-byte ones otherwise)
        d = lower(ea, eb, ec, M, N, K, **kw)
        info = planned(d, 9, limbs)
        bk = 128 if limbs == [1, 1] else 64
        pa, pb = (1 if d.cmul == 3 else 2), (1 if d.cmul == 4 else 2)
        up = lambda x, m: (x + m - 1) // m * m
        assert info.packed_bytes[0] == 9 * pa * limbs[0] * up(M, 64) * up(K, bk) + (256 if limbs[0] > 1 else 0)
        assert info.packed_bytes[1] == 9 * pb * limbs[1] * up(N, 64) * up(K, bk) + (256 if limbs[1] > 1 else 0)
        check(ctx, oracle, d, ea, eb, ec, (1, 2, 9), limbs, seed=3000 + K)


# ---- b. the bounds of the store: nothing beyond M, N in packed C, between the members in host C, or beyond the rows of a leading dimension
@pytest.mark.parametrize("shape", [(1, 1, 1), (5, 3, 40)], ids=["1x1x1", "5x3x40"])
@pytest.mark.parametrize("name", ["cc2", "ra2", "rb1"])
def test_bounds_of_the_store_with_300_members(ctx, oracle, name, shape):
    ea, eb, ec, kw, limbs = fmt(name)
    M, N, K = shape
    batch = 300
    d = lower(ea, eb, ec, M, N, K, **kw)
    info = planned(d, batch, limbs)
    ld = (M + 2, K + 3, M + 5)
    extA, extB, extC = extents(d, *ld)
    strides = (extA + 3, extB + 5, extC + 7)
    A, mA = host_batch(oracle, ea, batch, extA, strides[0], 4000, (0, 1))   # (the gaps of the leading dimensions hold in-range values the GEMM must not read)
    B, mB = host_batch(oracle, eb, batch, extB, strides[1], 4500, (0, 1))
    tA, tB = [tight(a, ld[0], M, K) for a in mA], [tight(b, ld[1], K, N) for b in mB]
    exp = [ref(oracle, d, a, b, ec) for a, b in zip(tA, tB)]
    # (members of one or fifteen outputs: the strength condition over the whole batch)
    allc = np.concatenate(exp)
    for part, f in (("re", ec.real), ("im", ec.imag)):
        v = allc[part].astype(np.int64)
        assert 2 * np.count_nonzero((v != 0) & (v != f.raw_min) & (v != f.raw_max)) >= v.size
    plain = run_plain_members(ctx, oracle, d, ec, tA[:4], tB[:4])
    for b in range(4):
        assert plain[b].tobytes() == exp[b].tobytes(), ("plain plan", b)
    packed = []
    got = run_stacked(ctx, oracle, d, ec, batch, A, B, strides, ld, packed_c=packed)
    assert got.tobytes() == expected_buffer(oracle, d, ec, batch, exp, strides[2], ld[2]).tobytes()
    # packed C: [2][M][N] per member in C's container at steps of 256 bytes; the bytes behind a member's 2 M N containers keep the poison
    cb = info.packed_bytes[2] // batch
    used = 2 * M * N * container(ec)
    assert cb % 256 == 0 and used <= cb and info.packed_bytes[2] == batch * cb
    grid = packed[0][:batch * cb].reshape(batch, cb)
    assert (grid[:, used:] == 0xA5).all()
    assert not (grid[:, :used] == 0xA5).all(axis=1).any()


# ---- c. TransposedA
@pytest.mark.parametrize("name", ["cc2", "rb31"])
def test_transposed_a(ctx, oracle, name):
    ea, eb, ec, kw, limbs = fmt(name)
    d = lower(ea, eb, ec, 65, 40, 200, transposed_a=True, **kw)
    check(ctx, oracle, d, ea, eb, ec, (2, 9), limbs, seed=5000)


# ---- d. the stack's ONE plane mask: a member of two-limb values only next to one with 32640 in the imaginary part only
@pytest.mark.parametrize("order", ["two_limb_first", "three_limb_first"])
def test_plane_mask_is_the_or_over_every_member(ctx, oracle, order):
    ea, eb, ec, kw, limbs = fmt("cc3")
    d = lower(ea, eb, ec, 65, 40, 200, **kw)
    three = 0 if order == "three_limb_first" else 1

    def edit(mA, mB):
        for m in mA + mB:
            for part in ("re", "im"):
                np.clip(m[part], -30000, 30000, out=m[part])   # two balanced limbs hold [-32896, 32639]
        mA[three]["im"][7] = 32640                             # 127 * 256 + 128: the third limb, in this one value
        assert max(int(np.abs(m[p]).max()) for i, m in enumerate(mA + mB) for p in ("re", "im") if i != three) <= 30000
    # batch 1: the first member alone (two_limb_first: the 2 x 2 kernel on three-plane storage takes the launch); batch 2: both
    check(ctx, oracle, d, ea, eb, ec, (1, 2), limbs, dists=(0,), seed=6000, edit=edit)


# ---- e. edge operands: every part of every operand at its minimum and maximum inside the compared members (dist 2)
def _bounds_edit(ea, eb):
    def put(m, e, at):
        if isinstance(e, Qcomplex):
            m["re"][at], m["re"][at + 1], m["im"][at + 2], m["im"][at + 3] = e.real.raw_min, e.real.raw_max, e.imag.raw_min, e.imag.raw_max
        else:
            m[at], m[at + 1] = e.raw_min, e.raw_max

    def edit(mA, mB):
        for m in mA:
            put(m, ea, 5)
        for m in mB:
            put(m, eb, 9)
    return edit


@pytest.mark.parametrize("name", ["cc1", "cc3", "ra2", "rb31"])
def test_edge_operands(ctx, oracle, name):
    ea, eb, ec, kw, limbs = fmt(name)
    d = lower(ea, eb, ec, 65, 40, 200, **kw)
    check(ctx, oracle, d, ea, eb, ec, (2,), limbs, dists=(2,), seed=7000, edit=_bounds_edit(ea, eb))


def test_all_four_parts_at_the_minimum_of_the_8_bit_format(ctx, oracle):
    """a = b = c = d = -128: ad + bc reaches 2^15, the value stacked_cases.B8's adbcT was sized for, K times in one output"""
    ea, eb, ec, kw, limbs = fmt("cc1")
    M, N, K = 33, 17, 40
    d = lower(ea, eb, ec, M, N, K, **kw)

    def edit(mA, mB):
        for m in mA:
            for part in ("re", "im"):
                m[part][0::M] = C8.real.raw_min       # row 0 of A: (0, k) at k * M
        for m in mB:
            for part in ("re", "im"):
                m[part][0:K] = C8.real.raw_min        # column 0 of B: (k, 0) at k
    exp, _, _ = check(ctx, oracle, d, ea, eb, ec, (2,), limbs, dists=(2,), seed=7500, edit=edit)
    for e in exp:   # C(0, 0) = K * ((-128)^2 - (-128)^2, 2 * (-128)^2) at 6 fraction bits, into C's 3 and 4
        assert int(e["re"][0]) == 0 and int(e["im"][0]) == (K * 2 * 128 * 128) >> 2


# ---- f. every C container (the wider part's for both parts), a saturating C and a wrapping C
def _c_formats():
    out = []
    # (8 bytes: both parts beyond 32 storage bits, 34 and 33, so that the host element is two 64-bit words without padding bytes,
    # which a byte-for-byte comparison of host buffers could not pin)
    for cb, (wide, narrow) in {1: ((4, 3), (3, 2)), 2: ((12, 3), (5, 3)), 4: ((19, 3), (7, 4)), 8: ((27, 6), (25, 7))}.items():
        for mode, of in (("sat", SAT.TCPL), ("wrap", WRP.TCPL)):
            for wide_part in ("re", "im"):
                w, n = Qu(*wide, True, RND.POS_INF, of), Qu(*narrow, True, RND.POS_INF, of)
                out.append(("%dbyte_%s_wide_%s" % (cb, mode, wide_part), cb, Qcomplex(w, n) if wide_part == "re" else Qcomplex(n, w)))
    return out


@pytest.mark.parametrize("cname,cbytes,ec", _c_formats(), ids=[c[0] for c in _c_formats()])
def test_every_c_container(ctx, oracle, cname, cbytes, ec):
    M, N, K, batch = 65, 40, 40, 2
    d = lower(C8, C8, ec, M, N, K, mul_args=B8, add_args=[L8])
    info = planned(d, batch, [1, 1])
    assert info.packed_bytes[2] == batch * ((2 * M * N * cbytes + 255) // 256 * 256)
    # a saturating C: operands of half the bits (dist 1), so that a few per cent of the narrow part's outputs sit at a bound and the
    # strength condition still holds (checked with the oracle: 96 % or more of every part inside its range); a wrapping C: full-range
    # operands in the first member, whose sums wrap many times
    exp, _, _ = check(ctx, oracle, d, C8, C8, ec, (batch,), [1, 1], dists=(1,) if "sat" in cname else (0, 1), seed=8000)
    if "sat" in cname and cbytes == 1:
        v = np.concatenate(exp)
        assert any(int(np.count_nonzero((v[p] == f.raw_min) | (v[p] == f.raw_max))) > 0 for p, f in (("re", ec.real), ("im", ec.imag)))   # (it does saturate)


# ---- g. the resident entry points: execute twice into the same buffers, a second pack of a different batch, time_execute
@pytest.mark.parametrize("name", ["cc3", "ra13"])
def test_resident_entry_points(ctx, oracle, name):
    ea, eb, ec, kw, limbs = fmt(name)
    M, N, K, batch = 65, 40, 200, 5
    d = lower(ea, eb, ec, M, N, K, **kw)
    planned(d, batch, limbs)
    extA, extB, extC = extents(d)
    strides = (extA, extB, extC)
    sets = []
    for seed in (9000, 9100):   # two different batches for the same packed buffers
        A, mA = host_batch(oracle, ea, batch, extA, extA, seed, (0, 1))
        B, mB = host_batch(oracle, eb, batch, extB, extB, seed + 50, (0, 1))
        exp = [ref(oracle, d, a, b, ec) for a, b in zip(mA, mB)]
        assert all(R.strong(d, e) for e in exp)
        sets.append((A, B, exp))
    plan = capi.BatchedPlan(ctx, d, batch, F)
    pb = plan.info.packed_bytes
    C = np.empty(batch * extC, dtype=oracle.host_dtype(ec))
    bufs = [ctx.alloc(sets[0][0].nbytes), ctx.alloc(sets[0][1].nbytes), ctx.alloc(C.nbytes), ctx.alloc(pb[0]), ctx.alloc(pb[1]), ctx.alloc(pb[2])]
    dA, dB, dC, pA, pB, pC = bufs
    try:
        assert plan.launches == 2 and STACKED in bytes(plan.info.reason)
        for A, B, exp in sets:
            ctx.h2d(dA, A.view(np.uint8)); ctx.h2d(dB, B.view(np.uint8))
            plan.pack(capi.OPERAND_A, dA, pA, strides[0])
            plan.pack(capi.OPERAND_B, dB, pB, strides[1])
            for rep in range(2):   # twice into the same packed C and the same workspace
                plan.execute(pC, pA, pB)
                C.view(np.uint8)[:] = POISON
                ctx.h2d(dC, C.view(np.uint8))
                plan.unpack_c(pC, dC, strides[2])
                ctx.sync()
                ctx.d2h(C.view(np.uint8), dC)
                assert C.tobytes() == np.concatenate(exp).tobytes(), rep
        assert plan.time_execute(pC, pA, pB, 1, 3) > 0.0   # qgemul_time_execute_batched: launches, and leaves the result of one
        plan.unpack_c(pC, dC, strides[2])
        ctx.sync()
        ctx.d2h(C.view(np.uint8), dC)
        assert C.tobytes() == np.concatenate(sets[1][2]).tobytes()
    finally:
        for p in bufs:
            ctx.free(p)
        plan.close()


# ---- h. the one-shot cache keys on the flags: the same descriptor with and without the flag in alternation
def test_one_shot_cache_alternates_between_the_two_forms(oracle):
    ea, eb, ec, kw, limbs = fmt("cc2")
    M, N, K, batch = 65, 40, 200, 3
    d = lower(ea, eb, ec, M, N, K, **kw)
    planned(d, batch, limbs)
    assert capi.classify_batched_launches(d, batch) == 2 * batch
    A, mA = host_batch(oracle, ea, batch, M * K, M * K, 9500, (0, 1))
    B, mB = host_batch(oracle, eb, batch, K * N, K * N, 9600, (0, 1))
    exp = np.concatenate([ref(oracle, d, a, b, ec) for a, b in zip(mA, mB)])
    assert R.strong(d, exp)
    try:
        for flags in (F, 0, F, 0):
            out = np.zeros(batch * M * N, dtype=oracle.host_dtype(ec))
            capi.run_batched(d, batch, out, A, B, M * N, M * K, K * N, flags=flags)
            assert out.tobytes() == exp.tobytes(), flags
        # a mixed batch: served under the flag, refused without it, and served again
        ea, eb, ec, kw, limbs = fmt("rb2")
        d = lower(ea, eb, ec, M, N, K, **kw)
        planned(d, batch, limbs)
        A, mA = host_batch(oracle, ea, batch, M * K, M * K, 9700, (0, 1))
        B, mB = host_batch(oracle, eb, batch, K * N, K * N, 9800, (0, 1))
        exp = np.concatenate([ref(oracle, d, a, b, ec) for a, b in zip(mA, mB)])
        assert R.strong(d, exp)
        for flags in (F, 0, F):
            out = np.zeros(batch * M * N, dtype=oracle.host_dtype(ec))
            st = capi.run_batched_status(d, batch, out, A, B, M * N, M * K, K * N, flags=flags)
            assert st == (capi.QG_OK if flags else capi.QG_EUNSUPPORTED), flags
            if flags:
                assert out.tobytes() == exp.tobytes()
    finally:
        capi.run_release()


# ---- i. the drop-in program: QgemulBatched on complex 3-d tensors with QgemulRunFlags() |= QG_OPT_BATCHED_STACKED
@pytest.mark.skipif(not os.path.exists(CLANG), reason="needs AMD clang (C++23)")
def test_standalone_header_runs_stacked_batches(oracle, tmp_path):
    exe = tmp_path / "amd_header_batched_cplx_run"
    lib = os.path.join(ROOT, "qublas_amd")
    subprocess.check_call([CLANG, "-std=c++23", "-O1", "-w", "-I" + os.path.join(ROOT, "include"), os.path.join(ROOT, "tests", "binding", "amd_header_batched_cplx_run.cpp"),
                           "-o", str(exe), "-L" + lib, "-lqugemm", "-Wl,-rpath," + lib])
    recs = {r["name"]: r for r in (json.loads(l) for l in subprocess.check_output([str(exe)], text=True).splitlines() if l.strip())}
    assert "error" not in str(recs)
    M, N, K, Bt = 65, 40, 72, 5
    c5 = COMPLEX["limb2"][0]

    def real(n):
        return np.array([(e * 2654435761) % 8192 - 4096 for e in range(n)], dtype=np.int32)

    def cplx(n):
        h = np.zeros(n, dtype=oracle.host_dtype(c5))
        h["re"] = [(e * 53 + 7) % 1024 - 512 for e in range(n)]
        h["im"] = [(e * 40503 + 3) % 16 - 8 for e in range(n)]
        return h
    e, ec, kw = COMPLEX["limb2"]
    er, ez, ecm, kwm = LINEAR["limb2"]
    calls = {"complex_x_complex": (lower(e, e, ec, M, N, K, **kw), cplx(M * K * Bt), cplx(K * N * Bt), ec),
             "real_x_complex_tn": (lower(er, ez, ecm, M, N, K, transposed_a=True, **kwm), real(K * M * Bt), cplx(K * N * Bt), ecm)}
    try:
        for name, (d, A, B, ecc) in calls.items():
            assert recs[name]["launches"] == 2 == capi.classify_batched_launches(d, Bt, F), name
            exp = np.concatenate([ref(oracle, d, A[b * M * K:(b + 1) * M * K], B[b * K * N:(b + 1) * K * N], ecc) for b in range(Bt)])
            assert R.strong(d, exp)
            got = np.asarray(recs[name]["C"], dtype=np.int64)
            assert np.array_equal(got[0::2], exp["re"].astype(np.int64)) and np.array_equal(got[1::2], exp["im"].astype(np.int64)), name
            if not R.is_mixed(d):   # qgemul_run_batched without the flag: member by member (a mixed batch has no such form)
                out = np.zeros(Bt * M * N, dtype=oracle.host_dtype(ecc))
                capi.run_batched(d, Bt, out, A, B, M * N, M * K, K * N)
                assert np.array_equal(got[0::2], out["re"].astype(np.int64)) and np.array_equal(got[1::2], out["im"].astype(np.int64)), name
    finally:
        capi.run_release()
