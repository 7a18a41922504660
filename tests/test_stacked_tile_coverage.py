"""Coverage guard of the stacked linear plans (mfma_rc: real x complex, mfma_cplx: complex x complex): every case of
tests/stacked_cases.py reaches the MFMA kernel variant, the limb counts and the plan kernel it names, on a launch of more than one tile
in both directions (more than 256 tiles for the persistent kernels, so that their second round is partly filled), with K across the
k-tile and oracle work below the cap; the table reaches every variant qg_mfma_pick can return, for both plans; and the descriptors
tools/measure_mixed.py times at its default size run on a variant the table covers.  The variants are read through the geometry driver
(tests/san/geom_san_driver.cpp, built without sanitizers).  tests/test_gpu_stacked_tiles.py runs the cases.  CPU only."""
import importlib.util
import os
import re
import subprocess

import pytest

import geom_sweep
import stacked_cases as S
from test_geom_sanitizers import CSRC, ROOT, fields


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("geom") / "geom_driver")
    subprocess.check_call(["g++", "-std=c++17", "-O1", os.path.join(ROOT, "tests", "san", "geom_san_driver.cpp"), os.path.join(CSRC, "qg_geom.cpp"),
                           os.path.join(CSRC, "qg_plan.cpp"), "-o", exe])
    return exe


def geometry(exe, descs, flags=0):
    """the driver's answer, {key: value}, for each descriptor's plain plan"""
    blob = b"".join(geom_sweep.pack_query(("plain", d, flags, None)) for d in descs)
    r = subprocess.run([exe], input=blob, capture_output=True, check=True, timeout=300)
    out = [fields(ln) for ln in r.stdout.decode().splitlines()]
    assert len(out) == len(descs)
    return out


def stacked_tiles(d, g):
    """(tiles along the rows, tiles along the columns) of the one real GEMM on the stacked operands"""
    _, TM, TN, _ = g["cfg"]
    parts_a, parts_b = (1 if d.cmul == 3 else 2), (1 if d.cmul == 4 else 2)   # QG_CMUL_REAL_A = 3, QG_CMUL_REAL_B = 4
    assert g["pa"][0] % TM == 0 and g["pb"][0] % TN == 0
    return parts_a * g["pa"][0] // TM, parts_b * g["pb"][0] // TN


def picked_variants():
    """the variants qg_mfma_pick names in its return statements"""
    src = open(os.path.join(CSRC, "qg_geom.cpp")).read()
    body = re.search(r"QMfmaCfg qg_mfma_pick\(.*?\n\}\n", src, re.S).group(0)
    names = set(re.findall(r"QMfmaCfg\{(QG_MFMA_\w+)", body))
    hdr = open(os.path.join(CSRC, "qg_geom.h")).read()
    value = {n: int(v) for n, v in re.findall(r"^\s*(QG_MFMA_\w+)\s*=\s*(\d+)", hdr, re.M)}
    return {value[n]: n for n in names if n != "QG_MFMA_NONE"}


def test_every_case_reaches_its_variant(driver):
    descs = [S.desc(c) for c in S.CASES]
    for c, d, g in zip(S.CASES, descs, geometry(driver, descs)):
        variant, TM, TN, BK = g["cfg"]
        assert g["st"] == 0 and g["kernel"] == c.kernel, (c.name, g["kernel"], g["reason"])
        assert variant == c.variant and (g["LA"], g["LB"]) == tuple(c.limbs), (c.name, g["cfg"], g["LA"], g["LB"])
        assert S.VARIANTS[variant][1:] == (BK, TM) and TM == TN, c.name   # (the GPU tests place their bands by this tile)
        tr, tc = stacked_tiles(d, g)
        if variant in S.PERSISTENT:
            assert tr * tc > 256 and (tr * tc) % 256, (c.name, tr, tc)   # a partly filled second round
        assert tr > 1 and tc > 1 and c.M % TM and c.N % TN, (c.name, tr, tc)   # (and a ragged last tile in both directions)
        # both parts of a stacked operand are more than one tile
        assert g["pa"][0] // TM > 1 and g["pb"][0] // TN > 1, c.name
        # K: one launch, and across the k-tile with a ragged tail (the QG_MFMA_PP case the cost cap shortens: one ragged k-tile)
        assert min(c.limbs) * c.K <= (1 << 17) - 1 and c.K % BK
        assert c.K > 2 * BK or c.name.endswith("_pp"), c.name
        assert S.oracle_cost(c.kernel, c.M, c.N, c.K, TM, TN) <= S.COST_CAP, (c.name, S.oracle_cost(c.kernel, c.M, c.N, c.K, TM, TN))


def test_the_table_reaches_every_variant_of_both_plans():
    """a variant added to qg_mfma_pick later, or one a stacked plan no longer reaches, fails here"""
    want = picked_variants()
    # QG_MFMA_64 and QG_MFMA_256 are the A/B and lock-step (QG_OPT_LOCKSTEP_TILES) forms of 7 and 9: no default plan takes them
    for opt_in in ("QG_MFMA_64", "QG_MFMA_256"):
        assert opt_in in want.values()
    want = {v for v, n in want.items() if n not in ("QG_MFMA_64", "QG_MFMA_256")}
    assert want == set(S.VARIANTS) == {1, 3, 6, 7, 8, 9, 10}
    for kernel in (S.KERNEL_RC, S.KERNEL_CPLX):
        assert {c.variant for c in S.CASES if c.kernel == kernel} == want, kernel
    # mixed plans: both operand orders on every variant, and the unequal limb pairs in both orders
    for order in ("_ra_", "_rb_"):
        assert {c.variant for c in S.CASES if order in c.name} == want, order
    # every (limbs, variant) pair of the table, spelled out: a case taken out of the table fails here
    sym = lambda pairs: {(l, v) for ls, v in pairs for l in ls}
    one, two, three = [(1, 1)], [(2, 2)], [(3, 3)]
    rc = sym([(one, 7), (one, 8), (one, 1), (one, 9), (two, 6), (two, 3), (two, 10), (three, 6), (three, 3), (three, 10),
              ([(1, 3), (3, 1)], 3), ([(1, 2), (2, 1)], 3)])
    cc = sym([(one, 7), (one, 8), (one, 1), (one, 9), (two, 6), (two, 3), (two, 10), (three, 10)])
    plain = [c for c in S.CASES if not c.kw["transposed_a"]]
    assert {(tuple(c.limbs), c.variant) for c in plain if c.kernel == S.KERNEL_RC and "_ra_" in c.name} == {p for p in rc if p[0][0] <= p[0][1]}
    assert {(tuple(c.limbs), c.variant) for c in plain if c.kernel == S.KERNEL_RC and "_rb_" in c.name} == {p for p in rc if p[0][0] >= p[0][1]}
    assert {(tuple(c.limbs), c.variant) for c in plain if c.kernel == S.KERNEL_CPLX} == cc
    # QG_MFMA_PP: its smallest shape, and one with K over more than two k-tiles; complex 2 x 2 limbs at all three complex shapes
    for tag in ("rc_limb1_ra", "rc_limb1_rb", "cc_limb1"):
        pp = [c for c in S.CASES if c.name.startswith(tag) and c.variant == 9]
        assert any(1921 in (c.M, c.N) for c in pp) and any(c.K == 264 for c in pp), tag
    assert {(c.M, c.N) for c in S.CASES if c.kernel == S.KERNEL_CPLX and tuple(c.limbs) == (2, 2)} >= {(901, 641), (1025, 1025), (2049, 1921)}
    # TransposedA on a multi-tile 128 x 128 geometry: both mixed orders and the complex plan
    ta = [c for c in S.CASES if c.kw["transposed_a"]]
    kinds = sorted("cc" if c.kernel == S.KERNEL_CPLX else "rc_ra" if "_ra_" in c.name else "rc_rb" for c in ta)
    assert all(c.variant in (1, 3, 8) for c in ta) and kinds == ["cc", "rc_ra", "rc_rb"], [c.name for c in ta]
    assert all(S.BY_NAME[n].variant in (1, 3, 8) for n in S.RESIDENT) and {S.BY_NAME[n].kernel for n in S.RESIDENT} == {S.KERNEL_RC, S.KERNEL_CPLX}


def test_plane_mask_cases_reach_their_kernels(driver):
    descs = [S.mask_desc(order, M, N, K) for order in ("ra", "rb") for M, N, K, _ in S.MASK_SHAPES]
    want = [v for _ in ("ra", "rb") for _, _, _, v in S.MASK_SHAPES]
    for d, v, g in zip(descs, want, geometry(driver, descs)):
        assert g["kernel"] == S.KERNEL_RC and g["cfg"][0] == v and (g["LA"], g["LB"]) == (3, 3), (g["cfg"], g["reason"])
        assert S.VARIANTS[v][1:] == (g["cfg"][3], g["cfg"][1]) and g["cfg"][1] == g["cfg"][2]
        tr, tc = stacked_tiles(d, g)
        assert tr > 1 and tc > 1 and (v not in S.PERSISTENT or tr * tc > 256)


def test_measured_workloads_run_on_a_covered_variant(driver):
    """the README's two 2048^3 linear-class rows: tools/measure_mixed.py's wide-tag descriptors at its default size"""
    spec = importlib.util.spec_from_file_location("measure_mixed", os.path.join(ROOT, "tools", "measure_mixed.py"))
    mm = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mm)
    for order in ("ra", "rb"):
        mixed, padded = mm.wide_descs(order, mm.DEFAULT_SIZE)
        for d, kernel in zip((mixed, padded), (S.KERNEL_RC, S.KERNEL_CPLX)):
            g = geometry(driver, [d])[0]
            assert g["kernel"] == kernel, g["reason"]
            covered = {(c.variant, tuple(c.limbs)) for c in S.CASES if c.kernel == kernel}
            assert (g["cfg"][0], (g["LA"], g["LB"])) in covered, (order, g["cfg"], g["LA"], g["LB"])
