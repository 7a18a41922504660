"""CPU restatement of the reference's ANUS::Qapprox (QuBLAS.h:4829-4897) on the oracle's 64-bit scalar primitives
(qoracle_mul / qoracle_add / qoracle_convert) — TEST INFRASTRUCTURE, shared by the approx tests.

A table is a list of segments (breakpoint, [(raw, Qu), ...]), coefficient 0 first:
  selection  the first segment with x.toDouble() < breakpoint, else the last one; toDouble() = raw / 2^F is exact for
             the formats used here (at most 53 value bits), so the comparison is done on exact rationals;
  Horner     v = a_n;  v = Qadd<f_i>(a_i, Qmul<f_i>(x, v))  for i = n-1 .. 0;
  result     converted into x's own format.
"""
from __future__ import annotations

import glob
import math
import os
from fractions import Fraction

import numpy as np

import golden_io as G
from oracle import qoracle
from qublas_amd.desc import RND, WRP, Qu


def cases():
    out = []
    for p in sorted(glob.glob(os.path.join(G.GOLD, "ref_approx_*.jsonl.gz"))):
        out.extend(G._records(p))
    return out


def case_table(j):
    """(x format, segments) of a golden record"""
    segs = [(float.fromhex(s["bp"]), [(int(a), Qu.from_tuple(f)) for a, f in zip(s["a"], s["f"])]) for s in j["segments"]]
    return Qu.from_tuple(j["x"]), segs


def threshold(bp: float, F: int):
    """the integer T with  raw / 2^F < bp  <=>  raw < T   (None: +inf, never reached; -inf: any raw is >= it)"""
    if math.isinf(bp):
        return None if bp > 0 else -(1 << 200)
    return math.ceil(Fraction(bp) * Fraction(2) ** F)


def select(x: int, fx: Qu, segs) -> int:
    v = Fraction(x) / Fraction(2) ** fx.fracBits
    for s, (bp, _) in enumerate(segs):
        if bp == math.inf or (not math.isinf(bp) and v < Fraction(bp)):
            return s
    return len(segs) - 1


def _events(exact: int, d: int, f: Qu, ev):
    """what the step exact -> (round by d) -> overflow into f did: a tie rounded, a saturation, a wrap"""
    L = qoracle.lib()
    if d > 0 and f.QuMode <= RND.CONV and (exact & ((1 << d) - 1)) == (1 << (d - 1)):
        ev.add("tie")
    r = L.qoracle_round(exact, d, f.QuMode) if d > 0 else exact << -d
    if L.qoracle_overflow(r, f.c()) != r:
        ev.add("wrap" if f.OfMode == WRP.TCPL else "sat")


def approx_one(x: int, fx: Qu, segs, ev=None) -> int:
    L = qoracle.lib()
    _, coefs = segs[select(x, fx, segs)]
    v, fv = coefs[-1]
    for a, f in reversed(coefs[:-1]):
        if ev is not None:
            _events(x * v, fx.fracBits + fv.fracBits - f.fracBits, f, ev)
        p = L.qoracle_mul(x, fx.c(), v, fv.c(), f.c())
        if ev is not None:
            _events(a + p, 0, f, ev)
        v, fv = L.qoracle_add(a, f.c(), p, f.c(), f.c(), 0), f
    if ev is not None and fv != fx:
        _events(v, fv.fracBits - fx.fracBits, fx, ev)
    return L.qoracle_convert(v, fv.c(), fx.c())


def approx(xs, fx: Qu, segs) -> np.ndarray:
    """element by element; identical inputs are evaluated once"""
    xs = np.ascontiguousarray(xs, dtype=np.int64).reshape(-1)
    uniq, inv = np.unique(xs, return_inverse=True)
    ys = np.asarray([approx_one(int(v), fx, segs) for v in uniq], dtype=np.int64)
    return ys[inv]
