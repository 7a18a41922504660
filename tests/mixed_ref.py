"""CPU checker of a Qgemul with one real and one complex operand (QG_CMUL_REAL_A / QG_CMUL_REAL_B, include/qgemul.h) — TEST
INFRASTRUCTURE, shared by the mixed tests.

Qmul(real, complex) and Qmul(complex, real) are part-wise (QuBLAS.h:3604-3644) and so are the complex tree and C's conversion, so
a mixed Qgemul is two REAL Qgemuls that share one operand.  Part p of a mixed descriptor is therefore evaluated as a real
qgemul_desc through the unchanged qoracle_gemm:  a / b[p] (or a[p] / b),  c[p],  mul[0] = mul[p],  level_add[0] = level_add[p],
level[0] = level[p]  (qoracle_gemm reads level_add and level separately for a real descriptor too).
tests/golden/ref_mixed_0.jsonl.gz holds what the reference itself computes (tests/golden_src/ref_cases_mixed.cpp).
"""
from __future__ import annotations

import functools
import glob
import os

import numpy as np

import golden_io as G
from oracle import qoracle
from qublas_amd.desc import CMUL_NONE, CMUL_REAL_A, CMUL_REAL_B, QGEMUL_ABI_VERSION, Qcomplex, Qu, desc_from_dict, qgemul_desc


def is_mixed(d: qgemul_desc) -> bool:
    return bool(d.is_complex) and d.cmul in (CMUL_REAL_A, CMUL_REAL_B)


def _qu(f) -> Qu:
    return Qu(f.I, f.F, bool(f.S), f.Q, f.O)


def elems(d: qgemul_desc):
    """(A element, B element, C element) of a mixed descriptor"""
    cplx = lambda f: Qcomplex(_qu(f[0]), _qu(f[1]))
    ea = _qu(d.a[0]) if d.cmul == CMUL_REAL_A else cplx(d.a)
    eb = _qu(d.b[0]) if d.cmul == CMUL_REAL_B else cplx(d.b)
    return ea, eb, cplx(d.c)


def part_desc(d: qgemul_desc, p: int) -> qgemul_desc:
    """the real descriptor of part p (0 real, 1 imaginary)"""
    assert is_mixed(d)
    r = qgemul_desc()
    r.abi, r.transA, r.is_complex, r.cmul, r.flags = QGEMUL_ABI_VERSION, d.transA, 0, CMUL_NONE, d.flags
    r.M, r.N, r.K, r.n_levels = d.M, d.N, d.K, d.n_levels
    fa = d.a[0] if d.cmul == CMUL_REAL_A else d.a[p]
    fb = d.b[0] if d.cmul == CMUL_REAL_B else d.b[p]
    r.a[0] = r.a[1] = fa
    r.b[0] = r.b[1] = fb
    r.c[0] = r.c[1] = d.c[p]
    r.mul[0] = d.mul[p]
    for l in range(d.n_levels):
        r.level_add[0][l] = r.level_add[1][l] = d.level_add[p][l]
        r.level[0][l] = r.level[1][l] = d.level[p][l]
    return r


def _part(arr: np.ndarray, p: int) -> np.ndarray:
    return np.ascontiguousarray(arr["im" if p else "re"]) if arr.dtype.names else arr


def gemm(d: qgemul_desc, A: np.ndarray, B: np.ndarray, *, lda=0, ldb=0, rows=(0, 0), cols=(0, 0), nthreads: int = 4,
         out: np.ndarray | None = None) -> np.ndarray:
    """C (tight, host layout of the complex C element) of a mixed descriptor, part by part through qoracle_gemm.  rows / cols / out as
    in qoracle.gemm: only the block rows x cols is evaluated ((0, 0): the whole extent) and written into out, whose other elements keep
    their values"""
    _, _, ec = elems(d)
    if out is None:
        out = np.zeros(d.M * d.N, dtype=qoracle.host_dtype(ec))
    r = slice(rows[0], rows[1] if rows[1] > 0 else d.M)   # (an end <= 0: to the end, as in qoracle_gemm)
    c = slice(cols[0], cols[1] if cols[1] > 0 else d.N)
    grid = out.reshape(d.N, d.M)
    for p, (name, f) in enumerate((("re", ec.real), ("im", ec.imag))):
        part = qoracle.gemm(part_desc(d, p), _part(A, p), _part(B, p), f, lda=lda, ldb=ldb, rows=rows, cols=cols, nthreads=nthreads)
        grid[name][c, r] = part.reshape(d.N, d.M)[c, r]
    return out


def strong(d: qgemul_desc, c: np.ndarray) -> bool:
    """the strength condition: at least half of each part's outputs are neither zero nor at a bound of C"""
    _, _, ec = elems(d)
    for name, f in (("re", ec.real), ("im", ec.imag)):
        v = c[name]
        if v.dtype.names:   # multi-word parts: compare as Python integers
            v = np.array(qoracle.from_host(v), dtype=object)
        good = sum(1 for x in v.tolist() if x != 0 and x != f.raw_min and x != f.raw_max)
        if 2 * good < len(v):
            return False
    return True


@functools.lru_cache(maxsize=None)
def cases():
    out = []
    for p in sorted(glob.glob(os.path.join(G.GOLD, "ref_mixed_*.jsonl.gz"))):
        out.extend(G._records(p))
    return out


def case_desc(j) -> qgemul_desc:
    return desc_from_dict(j)


def case_inputs(j):
    d = case_desc(j)
    ea, eb, _ = elems(d)
    inp = j["inputs"]
    return qoracle.fill(ea, d.M * d.K, inp["seedA"], inp["dist"]), qoracle.fill(eb, d.K * d.N, inp["seedB"], inp["dist"])


def case_expected(j) -> np.ndarray:
    d = case_desc(j)
    _, _, ec = elems(d)
    out = np.zeros(d.M * d.N, dtype=qoracle.host_dtype(ec))
    for k, (name, f) in enumerate((("re", ec.real), ("im", ec.imag))):
        vals = j["C"][k::2]
        out[name] = qoracle.to_host(vals, f)
    return out


@functools.lru_cache(maxsize=None)
def case_checked(name: str):
    """(descriptor, A, B, checker's C) of a golden record, computed once and shared (callers must not modify it)"""
    j = next(c for c in cases() if c["name"] == name)
    d = case_desc(j)
    A, B = case_inputs(j)
    return d, A, B, gemm(d, A, B)
