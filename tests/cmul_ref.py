"""CPU restatement of the reference's complex x complex Qmul (BasicComplexMul / TFComplexMul, QuBLAS.h:3421-3534) and of complex
chains that hold it, on the oracle's 64-bit scalar primitives (qoracle_mul / qoracle_add / qoracle_convert) — TEST INFRASTRUCTURE,
shared by the cmul tests.

With f1 = a + bi the first argument and f2 = c + di the second, and m[] the resolved result format of every sub-operation in the
slot order of include/qgemul.h:
  Basic  re = Qsub<m[RE]>(Qmul<m[AC]>(a, c), Qmul<m[BD]>(b, d)),  im = Qadd<m[IM]>(Qmul<m[AD]>(a, d), Qmul<m[BC]>(b, c))
  TF     A = Qmul<m[A]>(Qadd<m[AB]>(a, b), c),  B = Qmul<m[B]>(Qadd<m[CD]>(c, d), b),  C = Qmul<m[C]>(Qsub<m[BA]>(b, a), d),
         re = Qsub<m[RE]>(A, B),  im = Qsub<m[IM]>(B, C)
A chain is a qgemul_epilogue_cplx plus its qgemul_cmul records, exactly what the engine is given; the plain stages are restated here
as well (ADD / SUB / MUL / PASS per part), so that the whole chain has one independent evaluation.
"""
from __future__ import annotations

import functools
import glob
import os

import numpy as np

import golden_io as G
from oracle import qoracle
from qublas_amd.desc import (CMUL_BASIC, CMUL_TF, EW_ADD, EW_CMUL, EW_MUL, EW_PASS, EW_SUB, QG_MAX_EW, RND, WRP, Qcomplex, Qu, qgemul_cmul,
                             qgemul_epilogue_cplx)

B_AC, B_BD, B_AD, B_BC, B_RE, B_IM = range(6)
T_AB, T_CD, T_BA, T_A, T_B, T_C, T_RE, T_IM = range(8)


def cases():
    out = []
    for p in sorted(glob.glob(os.path.join(G.GOLD, "ref_cplx_cmul_*.jsonl.gz"))):
        out.extend(G._records(p))
    return out


def _qu(f) -> Qu:
    return f if isinstance(f, Qu) else Qu(f.I, f.F, bool(f.S), f.Q, f.O)


def case_chain(j):
    """(qgemul_epilogue_cplx, [qgemul_cmul or None] * QG_MAX_EW, C type, D type) of a golden record: what the reference's types report"""
    epc = qgemul_epilogue_cplx()
    cx = [None] * QG_MAX_EW
    for p in range(2):
        epc.part[p].n_stages = len(j["stages"])
        epc.part[p].d = Qu.from_tuple(j["d"][p]).c()
    for k, s in enumerate(j["stages"]):
        epc.e_complex[k] = s["e_complex"]
        for p in range(2):
            st = epc.part[p].stage[k]
            st.op, st.x_first, st.e_scalar = s["op"], s["x_first"], s["scalar"]
            # (the last stage's result goes into d and its t is ignored: written as the lowerings write it, t = r)
            st.e, st.r, st.t = (Qu.from_tuple(s[key][p]).c() for key in ("e", "r", "t" if k + 1 < len(j["stages"]) else "r"))
            if p == 1 and not s["e_complex"] and s["op"] != EW_MUL:      # complex (+|-) real: include/qgemul.h's table
                st.e_scalar = 1
                if s["op"] == EW_ADD or s["x_first"]:
                    st.op = EW_PASS
        if s["op"] == EW_CMUL:
            cx[k] = qgemul_cmul()
            cx[k].cmul = s["cmul"]
            for i, f in enumerate(s["mul"]):
                cx[k].mul[i] = Qu.from_tuple(f).c()
    c = Qcomplex(Qu.from_tuple(j["c"][0]), Qu.from_tuple(j["c"][1]))
    d = Qcomplex(Qu.from_tuple(j["d"][0]), Qu.from_tuple(j["d"][1]))
    return epc, cx, c, d


def case_operands(j):
    """per stage the values the real parts' / the imaginary parts' stage reads (what qgemul_ep_args carries)"""
    Ere, Eim = [], []
    for s in j["stages"]:
        Ere.append(np.asarray(s["Ere"], dtype=np.int64))
        if s["e_complex"] or s["op"] == EW_MUL:
            Eim.append(np.asarray(s["Eim"] if s["e_complex"] else s["Ere"], dtype=np.int64))
        else:
            Eim.append(np.zeros(1, dtype=np.int64))
    return Ere, Eim


def _events(exact: int, d: int, f: Qu, ev):
    """what the step exact -> (round by d) -> overflow into f did: a tie rounded, a saturation, a wrap"""
    L = qoracle.lib()
    if d > 0 and f.QuMode <= RND.CONV and (exact & ((1 << d) - 1)) == (1 << (d - 1)):
        ev.add("tie")
    r = L.qoracle_round(exact, d, f.QuMode) if d > 0 else exact << -d
    if L.qoracle_overflow(r, f.c()) != r:
        ev.add("wrap" if f.OfMode == WRP.TCPL else "sat")


@functools.lru_cache(maxsize=None)
def _c(f: Qu):
    return f.c()


# the primitives are pure: identical calls (a sweep over all pairs of small formats makes few distinct ones) are answered once
@functools.lru_cache(maxsize=1 << 20)
def _mul_raw(x, fx, y, fy, r):
    return qoracle.lib().qoracle_mul(x, _c(fx), y, _c(fy), _c(r))


@functools.lru_cache(maxsize=1 << 20)
def _add_raw(x, fx, y, fy, r, sub):
    return qoracle.lib().qoracle_add(x, _c(fx), y, _c(fy), _c(r), sub)


@functools.lru_cache(maxsize=1 << 20)
def _cvt_raw(x, fx, to):
    return qoracle.lib().qoracle_convert(x, _c(fx), _c(to))


def _mul(x, fx: Qu, y, fy: Qu, r: Qu, ev=None):
    if ev is not None:
        _events(x * y, fx.fracBits + fy.fracBits - r.fracBits, r, ev)
    return _mul_raw(x, fx, y, fy, r)


def _add(x, fx: Qu, y, fy: Qu, r: Qu, sub: bool, ev=None):
    if ev is not None:
        F = max(fx.fracBits, fy.fracBits)
        xa, ya = x << (F - fx.fracBits), y << (F - fy.fracBits)
        _events(xa - ya if sub else xa + ya, F - r.fracBits, r, ev)
    return _add_raw(x, fx, y, fy, r, int(sub))


def _cvt(x, fx: Qu, to: Qu, ev=None):
    if fx == to:
        return x
    if ev is not None:
        _events(x, fx.fracBits - to.fracBits, to, ev)
    return _cvt_raw(x, fx, to)


def cmul_one(a, fa, b, fb, c, fc, d, fd, cmul: int, m, ev=None):
    """Qmul<M>(a + bi, c + di) on raw integers; m: the eight slot formats.  Returns (re, im) in m[RE] / m[IM]."""
    if cmul == CMUL_BASIC:
        ac, bd = _mul(a, fa, c, fc, m[B_AC], ev), _mul(b, fb, d, fd, m[B_BD], ev)
        ad, bc = _mul(a, fa, d, fd, m[B_AD], ev), _mul(b, fb, c, fc, m[B_BC], ev)
        return _add(ac, m[B_AC], bd, m[B_BD], m[B_RE], True, ev), _add(ad, m[B_AD], bc, m[B_BC], m[B_IM], False, ev)
    assert cmul == CMUL_TF
    ab, cd, ba = _add(a, fa, b, fb, m[T_AB], False, ev), _add(c, fc, d, fd, m[T_CD], False, ev), _add(b, fb, a, fa, m[T_BA], True, ev)
    A, Bv, Cv = _mul(ab, m[T_AB], c, fc, m[T_A], ev), _mul(cd, m[T_CD], b, fb, m[T_B], ev), _mul(ba, m[T_BA], d, fd, m[T_C], ev)
    return _add(A, m[T_A], Bv, m[T_B], m[T_RE], True, ev), _add(Bv, m[T_B], Cv, m[T_C], m[T_IM], True, ev)


def chain_program(epc, cx):
    """the chain's records with their formats as Qu objects (made once per chain, not per element)"""
    prog = []
    for k in range(epc.part[0].n_stages):
        st = [epc.part[0].stage[k], epc.part[1].stage[k]]
        prog.append(dict(op=[st[0].op, st[1].op], x_first=[st[0].x_first, st[1].x_first], e=[_qu(st[0].e), _qu(st[1].e)], r=[_qu(st[0].r), _qu(st[1].r)],
                         t=[_qu(st[0].t), _qu(st[1].t)], cmul=cx[k].cmul if cx[k] is not None else 0,
                         m=[_qu(q) for q in cx[k].mul] if cx[k] is not None else None))
    return prog, [_qu(epc.part[0].d), _qu(epc.part[1].d)]


def chain_one(prog, d, c: Qcomplex, xr: int, xi: int, er, ei, ev=None):
    """the whole chain on one element: er[k] / ei[k] = the raw value stage k of that part reads"""
    x, f = [xr, xi], [c.real, c.imag]
    n = len(prog)
    for k, s in enumerate(prog):
        e, fe = [er[k], ei[k]], s["e"]
        if s["op"][0] == EW_CMUL:
            m = s["m"]
            first = (x[0], f[0], x[1], f[1]) if s["x_first"][0] else (e[0], fe[0], e[1], fe[1])
            second = (e[0], fe[0], e[1], fe[1]) if s["x_first"][0] else (x[0], f[0], x[1], f[1])
            x = list(cmul_one(*first, *second, s["cmul"], m, ev))
            f = [m[T_RE], m[T_IM]] if s["cmul"] == CMUL_TF else [m[B_RE], m[B_IM]]
        else:
            for p in range(2):
                op = s["op"][p]
                if op == EW_PASS:
                    continue
                r = s["r"][p]
                one, two = ((x[p], f[p]), (e[p], fe[p])) if s["x_first"][p] else ((e[p], fe[p]), (x[p], f[p]))
                x[p] = _mul(*one, *two, r, ev) if op == EW_MUL else _add(*one, *two, r, op == EW_SUB, ev)
                f[p] = r
        if k + 1 < n:
            for p in range(2):
                t = s["t"][p]
                x[p], f[p] = _cvt(x[p], f[p], t, ev), t
    return tuple(_cvt(x[p], f[p], d[p], ev) for p in range(2))


def chain(epc, cx, c: Qcomplex, Xre, Xim, Ere, Eim, ev=None):
    """element by element (identical inputs are evaluated once); Ere[k] / Eim[k]: arrays, or 1 element for a scalar stage.
    Returns (D_re, D_im) raw values as int64."""
    Xre = np.ascontiguousarray(Xre, dtype=np.int64).reshape(-1)
    n, ns = Xre.size, epc.part[0].n_stages
    cols = [Xre, np.ascontiguousarray(Xim, dtype=np.int64).reshape(-1)]
    for k in range(ns):
        for E in (Ere[k], Eim[k]):
            E = np.ascontiguousarray(E, dtype=np.int64).reshape(-1)
            cols.append(np.broadcast_to(E, n) if E.size == 1 else E)
    rows, inv = np.unique(np.stack(cols, axis=1), axis=0, return_inverse=True)
    prog, d = chain_program(epc, cx)
    out = np.asarray([chain_one(prog, d, c, r[0], r[1], r[2::2], r[3::2], ev) for r in rows.tolist()],
                     dtype=np.int64).reshape(-1, 2)
    inv = np.asarray(inv).reshape(-1)
    return out[inv, 0], out[inv, 1]
