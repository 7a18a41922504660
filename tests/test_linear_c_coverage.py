"""Coverage guard of the linear class's conversion sites (tests/linear_c_cases.py; the method: tests/designed_sums.py).  CPU only.
  * every case reaches the kernel variant, limb counts, centred / base-64 layout, composite form, wide_ep, launch count and C container
    it names, through the geometry driver (tests/san/geom_san_driver.cpp, built without sanitizers), on a shape with ragged last tiles,
    K across the k-tile and, for the persistent kernels, a partly filled second round;
  * the table reaches every variant qg_mfma_pick can return, the six-product kernel, the ring kernel and the lock-step 256 form; the
    two-group kernels get their compile-time FAST epilogue and the general one per container;
  * per site and container every QuMode and OfMode occurs, with the shift-and-clamp pair, its two neighbours, d = 1, d = 0, a left shift
    and an unsigned C fed by signed sums; a shift of 8 or more occurs in every container of every site (on a roomy C, ties
    only, where no short K reaches the bounds behind it);
  * witnesses ON THE DATA, no kernel involved: ties of both signs with even and odd kept parts, just above / below half, rounded values
    at hi, hi + 1, lo, lo - 1 (SAT::SMGN: -hi, -hi - 1; unsigned C: 0, -1), a multiple wrap; shares of in-range, above and below;
    every class in every full tile, every offset class in the ragged last tile row and column;
  * the stacked plans (complex x complex, complex x real; plain and as a stacked block-diagonal batch) reach their kernels with two
    launches, and the witnesses and shares hold per part of C;
  * the oracle's bands stay under the cost cap, and on the small shapes oracle.gemm over the WHOLE matrix equals the helper's
    expectation: the CPU proof that the designed sums and the oracle agree."""
import subprocess

import numpy as np
import pytest

import designed_sums as DS
import geom_sweep
import linear_c_cases as L
import stacked_cases as S
from qublas_amd.desc import SAT, TRN, WRP
from test_geom_sanitizers import fields
from test_stacked_tile_coverage import driver, picked_variants  # noqa: F401  (driver: the fixture)

KERNEL_I8, KERNEL_LIMB = 1, 2   # QG_KERNEL_MFMA_I8, QG_KERNEL_MFMA_I8_LIMB (include/qgemul.h)
FAST_SITES = {9, 10, 11}        # the kernels with a compile-time shift-and-clamp epilogue next to the general routine


def geometry(exe, cases):
    """{case name: the driver's answer} — one driver run per flag word"""
    out = {}
    for flags in sorted({L.BY_SITE[c.site].flags for c in cases}):
        group = [c for c in cases if L.BY_SITE[c.site].flags == flags]
        blob = b"".join(geom_sweep.pack_query(("plain", L.desc(c), flags, None)) for c in group)
        r = subprocess.run([exe], input=blob, capture_output=True, check=True, timeout=300)
        lines = r.stdout.decode().splitlines()
        assert len(lines) == len(group)
        out.update({c.name: fields(ln) for c, ln in zip(group, lines)})
    return out


@pytest.fixture(scope="module")
def answers(driver):  # noqa: F811
    return geometry(driver, L.CASES)


def test_every_case_reaches_its_site(answers):
    for c in L.CASES:
        s, (ea, eb, es), centres, offsets, K = L.plan(c)
        g, e = answers[c.name], L.expected(c)
        assert g["st"] == 0, (c.name, g["reason"])   # a valid launch, K inside what the planner admits
        variant, TM, TN, BK = g["cfg"]
        assert g["kernel"] == (KERNEL_I8 if s.limbs == (1, 1) and s.variant != 12 else KERNEL_LIMB), (c.name, g["kernel"], g["reason"])
        assert variant == s.variant and (g["LA"], g["LB"]) == s.limbs, (c.name, g["cfg"], g["LA"], g["LB"], g["reason"])
        assert L.VARIANTS[variant][1:] == (BK, TM, TN), c.name
        assert bool(g["pa"][9]) == bool(g["pb"][9]) == s.centred, (c.name, g["pa"][9])
        assert bool(g["pa"][7]) == bool(g["pb"][7]) == s.digit6, (c.name, g["pa"][7])
        comp = g["comp"][0]
        assert ((comp[1], comp[2], comp[3]) if comp[0] else None) == e["comp"], (c.name, comp)
        assert g["wide_ep"] == e["wide_ep"] and g["launches"] == e["launches"] and g["pc"][6] == e["container"], (c.name, g["wide_ep"], g["launches"], g["pc"][6])
        # the shape: ragged last tiles at least 9 wide and no multiple of 4, K across the k-tile with a ragged tail
        for extent, tile in ((s.M, TM), (s.N, TN)):
            assert extent % tile >= 9 and (extent % tile) % 4, (c.name, extent, tile)
        assert K > BK and K % BK and K >= DS.k_needed(ea, eb, centres, offsets), (c.name, K)
        tiles = -(-s.M // TM) * -(-s.N // TN)
        if variant in L.PERSISTENT:
            assert tiles > 256 and tiles % 256, (c.name, tiles)   # a partly filled second round
        if variant == 2:
            assert tiles >= 256, (c.name, tiles)
        # every (centre, offset) pair visits every position of every full tile; the ragged last tile column holds every offset class
        P, Q = len(centres), len(offsets)
        assert DS.well_formed(P, Q) and P <= min(TM, s.M) and Q <= min(TN, s.N) and Q <= s.N % TN, (c.name, P, Q)
        assert L.COST_CAP == S.COST_CAP and L.oracle_cost(s.M, s.N, K, TM, TN) <= L.COST_CAP, (c.name, L.oracle_cost(s.M, s.N, K, TM, TN))


def test_the_table_reaches_every_variant():
    """a variant added to qg_mfma_pick later fails here until a site joins the table"""
    want = picked_variants()
    assert want.pop(5) == "QG_MFMA_64"   # the diagnostic build's A/B form of QG_MFMA_64_BK128 (QG_BK64): no plan of the library takes it
    reached = {s.variant for s in L.SITES}
    assert set(want) <= reached, set(want) - reached
    assert reached == set(want) | {11, 12} == set(L.VARIANTS), reached   # ... and the six-product and ring kernels, which qg_plan_geometry picks
    assert 2 in reached   # the lock-step 256 x 256 form
    by = lambda **kw: [s for s in L.SITES if all(getattr(s, k) == v for k, v in kw.items())]
    # centred: one limb on the 64-bit step branch and in the two-group kernel, two limbs on the row-step form; Karatsuba; composite forms
    assert by(centred=True, limbs=(1, 1), variant=7) and by(centred=True, limbs=(1, 1), variant=9) and by(centred=True, limbs=(2, 2), variant=3)
    assert by(digit6=True, variant=3, limbs=(2, 2)) and by(digit6=True, variant=11)
    assert {s.comp for s in L.SITES if s.comp} == {(1, 1, 2), (2, 2, 1)}
    assert {s.limbs for s in L.SITES if s.variant == 12} == {(1, 1), (1, 3), (4, 4)}
    for v, limbs in ((6, (2, 2)), (6, (3, 3)), (3, (2, 2)), (3, (3, 3)), (10, (2, 2)), (10, (3, 3))):
        assert by(variant=v, limbs=limbs, centred=False, digit6=False, comp=None), (v, limbs)
    # the 64-bit conversion pass behind k_mfma and behind k_mfma_pp
    assert {s.variant for s in L.SITES if "wide" in s.containers and s.limbs == (1, 1)} == {7, 9}
    # the kernels' containers: 1, 2 and 4 everywhere, 8 on every limb kernel, 4 and 8 on the two-group limb kernels.  Spelled out per
    # site; the narrower lists have reasons: a single-limb plan reaches an 8-byte C only through the 64-bit pass (wide64, wide_pp); the
    # two-group limb kernels take 4- and 8-byte C only (a narrower C runs QG_MFMA_LIMB_128: limb128_*);
    # a ring holds sums of n bits only (16: containers 1 and 2; 24: 1 and 2; 32: up to 4); k_lin_combine's container switch is one
    # routine for all its plans, run on 1, 2, 4 and 8 bytes by comb_g, so the k-chunked and the 128-bit plans take two containers each
    want = {"k64": (1, 2, 4), "k64_deep": ("deep4",), "k128": (1, 2, 4), "k128bk64": (1, 2, 4), "k256": (1, 2, 4), "pp": (1, 2, 4), "wide64": ("wide",), "wide_pp": ("wide",),
            "limb64_22": (1, 2, 4, "wide"), "limb64_33": (1, 2, 4, 8, "pieces"), "limb128_22": (1, 2, 4, "wide"), "limb128_33": (1, 2, 4, 8, "pieces"),
            "kara": (1, 2, 4, "wide"), "cent_u8": (1, 2, 4), "cent_u8_128": (1, 2, 4), "cent_q78": (1, 2, 4, 8), "pp_cent_u8": (1, 2, 4),
            "ppl33": (4, 8, "pieces"), "ppl22": (4, "wide"), "k6": (4, 8, "pieces"), "k6_schoolbook": (4, 8),
            "ring1": (1, 2), "ring3": (1, 2), "ring10": (1, 2, 4), "comb_k": (2, 4), "comb_g": (1, 2, 4, 8), "comb_w": (4, 8, "huge")}
    assert {s.name: s.containers for s in L.SITES if s.name in want} == want
    for s in L.SITES:
        for cont in s.containers:
            bits = {c.ec.storage_bits for c in L.CASES if c.site == s.name and c.container == cont and not c.roomy}
            if isinstance(cont, int):
                assert {L.pow2_bytes(b) for b in bits} == {cont}, (s.name, cont, bits)
            elif cont == "wide":
                assert max(bits) > 32, s.name


def shift(c):
    return L.OPERANDS[L.BY_SITE[c.site].op][3].fracBits - c.ec.fracBits


def test_mode_coverage_per_site_and_container():
    for s in L.SITES:
        es = L.OPERANDS[s.op][3]
        for cont in s.containers:
            cs = [c for c in L.CASES if c.site == s.name and c.container == cont]
            if cont in ("pieces", "huge"):
                assert cs and all(c.roomy for c in cs)
                continue
            if cont == "deep4":   # the bounds behind a shift of 8 in a 4-byte C of a single limb pair: all witnesses, on long K
                assert cs and all(shift(c) == 8 and not c.roomy and L.pow2_bytes(c.ec.storage_bits) == 4 for c in cs)
                continue
            modes = {(c.ec.QuMode, c.ec.OfMode) for c in cs}
            wide_sum = es.W > 63   # (RND::CONV of a sum wider than 64 bits is refused)
            assert {q for q, _ in modes} >= set(range(7)) - ({4} if wide_sum else set()), (s.name, cont)
            assert {o for _, o in modes} == set(range(4)), (s.name, cont)
            fast = [c for c in cs if L.is_fast(es, c.ec)]
            assert any(shift(c) >= 1 for c in fast), (s.name, cont)
            if s.variant in FAST_SITES:
                assert len(fast) < len(cs)   # FAST and the general routine
            # a shift of 8 or more in every container: with C's bounds among the sums where K reaches them, on a roomy C (ties only) where
            # they lie beyond MAX_DIGITS reduction indices or beyond the sum format
            assert any(shift(c) >= 8 for c in cs), (s.name, cont)
            assert any(shift(c) >= 8 and not c.roomy for c in cs) or any(shift(c) == 8 and c.roomy for c in cs), (s.name, cont)
            if cont == "wide":
                assert any(shift(c) < -20 for c in cs) and any(not c.ec.isSigned for c in cs) and any(c.roomy for c in cs)
                continue
            # the two neighbours across qg_step_is_shift_clamp
            assert any(c.ec.QuMode == TRN.TCPL and c.ec.OfMode != SAT.TCPL and shift(c) >= 1 for c in cs), (s.name, cont)
            assert any(c.ec.QuMode != TRN.TCPL and c.ec.OfMode == SAT.TCPL and shift(c) >= 1 for c in cs), (s.name, cont)
            ds = {shift(c) for c in cs}
            assert {1, 0} <= ds and min(ds) < 0, (s.name, cont, ds)
            assert any(not c.ec.isSigned for c in cs), (s.name, cont)   # (with signed operands: an unsigned C fed by signed sums)


def test_witnesses_and_shares_of_the_designed_sums(oracle):
    for c in L.CASES:
        s, (ea, eb, es), centres, offsets, K = L.plan(c)
        signed = ea.isSigned
        dz = DS.table(centres, offsets, (3 * c.idx) % len(centres), (5 * c.idx) % len(offsets))
        w = DS.witnesses(oracle, dz, es, c.ec, signed, bounds=not c.roomy)
        assert all(w.values()), (c.name, sorted(k for k, v in w.items() if not v))
        d = es.fracBits - c.ec.fracBits
        if d >= 1:
            assert {"tie+even", "tie+odd"} <= set(w) and (not signed or {"tie-even", "tie-odd"} <= set(w)), c.name
        if c.roomy:
            assert d >= 0, c.name
            continue
        assert {"hi", "hi+1"} <= set(w) and (not signed or {"lo", "lo-1"} <= set(w)), c.name
        assert c.ec.OfMode != WRP.TCPL or "multi_wrap+" in w, c.name
        # shares over the matrix and over the first full tile (every full tile holds every class: P <= TM and Q <= TN, asserted with the
        # geometry; the ragged last tile row spans every column and the ragged last tile column is at least Q wide: every offset class)
        TM, TN = L.VARIANTS[s.variant][2:]
        for rows, cols in ((None, None), ((0, min(TM, s.M)), (0, min(TN, s.N)))):
            inside, above, below = DS.shares(oracle, dz, es, c.ec, s.M, s.N, rows, cols)
            assert inside >= 0.2 and above >= 0.1 and (below >= 0.1 or not signed), (c.name, rows, cols, inside, above, below)


WHOLE = ("k64", "k64_deep", "wide64", "limb64_22", "limb64_33", "cent_u8", "comb_g", "comb_w", "ring1", "ring3", "ring10")


@pytest.mark.parametrize("site", WHOLE)
def test_oracle_gemm_over_the_whole_matrix_equals_the_expectation(oracle, site):
    """the smallest shape of every limb count (1, 2, 3, 4 with groups, centred, ring): oracle.gemm on the designed operands, every
    element, against the tiled conversion of the P x Q designed sums"""
    cases = [c for c in L.CASES if c.site == site]
    assert cases
    for c in cases:
        s, (_, _, es), _, _, _ = L.plan(c)
        d, dz = L.designed(oracle, c)
        exp = DS.expectation(oracle, dz, es, c.ec, s.M, s.N)
        got = oracle.gemm(d, dz.A, dz.B, c.ec, nthreads=16)
        assert np.array_equal(got, exp), c.name + "\n" + DS.report(dz, got, exp, s.M, s.N, 64)


# ---- the stacked plans' second passes: k_cplx_combine, k_rc_convert, and k_stack_combine_bd behind the stacked block-diagonal batch
def stacked_expectation(oracle, c, dr, di):
    _, _, _, es = L.stacked_operands(c.kind)
    M, N = L.STACKED_SHAPE
    exp = np.zeros(M * N, dtype=oracle.host_dtype(c.ec))
    exp["re"] = DS.expectation(oracle, dr, es.real, c.ec.real, M, N)
    exp["im"] = DS.expectation(oracle, di, es.imag, c.ec.imag, M, N)
    return exp


def test_stacked_cases_reach_their_kernels(driver):  # noqa: F811
    from qublas_amd import capi
    descs = [L.stacked_desc(c) for c in L.STACKED_CASES]
    blob = b"".join(geom_sweep.pack_query(("plain", d, 0, None)) for d in descs)
    r = subprocess.run([driver, ], input=blob, capture_output=True, check=True, timeout=300)
    M, N = L.STACKED_SHAPE
    for c, d, ln in zip(L.STACKED_CASES, descs, r.stdout.decode().splitlines()):
        g = fields(ln)
        assert g["st"] == 0 and g["kernel"] == (L.KERNEL_CPLX if c.kind == "cc" else L.KERNEL_RC), (c.name, g["kernel"], g["reason"])
        variant, TM, TN, BK = g["cfg"]
        assert variant == 7 and (g["LA"], g["LB"]) == (1, 1) and g["launches"] == 2, (c.name, g["cfg"], g["launches"])   # one GEMM + the second pass
        assert g["pc"][6] == c.container, (c.name, g["pc"][6])
        assert M % TM >= 9 and (M % TM) % 4 and N % TN >= 9 and (N % TN) % 4 and d.K > BK and d.K % BK, c.name
        # the stacked block-diagonal batch of three members: one launch and one combine pass
        st, info = capi.classify_batched_status(d, 3, capi.OPT_BATCHED_STACKED)
        assert st == 0 and b"combine pass" in bytes(info.reason) and capi.classify_batched_launches(d, 3, capi.OPT_BATCHED_STACKED) == 2, (c.name, info.reason)
        _, _, _, _, cr, ci, offsets, K = L.stacked_plan(c)
        assert DS.well_formed(len(cr), len(offsets)) and len(cr) == len(ci) <= TM and len(offsets) <= N % TN, c.name
        assert 4 * M * N * K <= L.COST_CAP, c.name   # the oracle over the whole matrix, four real products per MAC at most
    # both kinds; per kind, container and part every QuMode and OfMode; the parts of every case differ in both modes or in the shift
    for kind in ("cc", "rc"):
        for cont in (2, 4):
            cs = [c for c in L.STACKED_CASES if c.kind == kind and c.container == cont]
            for part in ("real", "imag"):
                fs = [getattr(c.ec, part) for c in cs]
                assert {f.QuMode for f in fs} == set(range(7)) and {f.OfMode for f in fs} == set(range(4)), (kind, cont, part)
            assert all((c.ec.real.QuMode, c.ec.real.OfMode) != (c.ec.imag.QuMode, c.ec.imag.OfMode) for c in cs), (kind, cont)
            es = L.stacked_operands(kind)[3]
            assert any(es.real.fracBits - c.ec.real.fracBits >= 8 for c in cs) and any(es.imag.fracBits - c.ec.imag.fracBits >= 8 for c in cs), (kind, cont)


def test_stacked_witnesses_shares_and_oracle(oracle):
    """per part of C: the witnesses and shares of the designed sums; and oracle.gemm (part by part for the mixed plan) over the whole
    matrix equals the expectation"""
    import mixed_ref as R
    M, N = L.STACKED_SHAPE
    for c in L.STACKED_CASES:
        _, _, _, es = L.stacked_operands(c.kind)
        d, A, B, dr, di = L.stacked_designed(oracle, c)
        for dz, sp, cp, roomy in ((dr, es.real, c.ec.real, c.roomy[0]), (di, es.imag, c.ec.imag, c.roomy[1])):
            w = DS.witnesses(oracle, dz, sp, cp, True, bounds=not roomy)
            assert all(w.values()), (c.name, str(cp), sorted(k for k, v in w.items() if not v))
            if sp.fracBits - cp.fracBits >= 1:
                assert {"tie+even", "tie+odd", "tie-even", "tie-odd"} <= set(w), c.name
            if not roomy:
                assert {"hi", "hi+1", "lo", "lo-1"} <= set(w), c.name
                inside, above, below = DS.shares(oracle, dz, sp, cp, M, N)
                assert inside >= 0.2 and above >= 0.1 and below >= 0.1, (c.name, str(cp), inside, above, below)
        exp = stacked_expectation(oracle, c, dr, di)
        got = R.gemm(d, A, B, nthreads=16) if R.is_mixed(d) else oracle.gemm(d, A, B, c.ec, nthreads=16)
        assert np.array_equal(got, exp), c.name
