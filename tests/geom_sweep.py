"""Shared by tests/test_geom_sanitizers.py and tools/dump_geometry.py: one fixed, seeded sweep of planner queries (plain, batched and
grouped; with and without element-wise chains), their wire form for tests/san/geom_san_driver.cpp and the same questions asked of the
loaded library through qublas_amd.capi.  Not a test module.  The descriptors are the other planner tests' own: they are imported."""
import ctypes as C
import random
import struct

import approx_ref
import batched_ep_cases as X
import cmul_ref
import golden_io as G
import test_approx_plan as TA
import test_batched_plan as TB
import test_cmul_plan as TC
import test_grouped_plan as TG
import test_ring_plan as TR
import test_wide as TW
from test_plan_sanitizers import compact_form_descs, random_descs
from qublas_amd import capi
from qublas_amd.desc import Approx, Qu, SAT, TRN, Tags, batched_ep, desc_from_dict, lower, lower_epilogue_x

FLAGS = [0, capi.OPT_FORCE_TREE, capi.OPT_BALANCED_LIMBS, capi.OPT_SCHOOLBOOK_LIMBS, capi.OPT_LOCKSTEP_TILES, capi.OPT_GENERIC_TREE, capi.OPT_FUSED_EPILOGUE,
         capi.OPT_UNFUSED_EPILOGUE]
# 1 << 40 members of 64 x 64 tiles: the "more than 2^31 - 1 tiles" refusal of a batched plan
BATCHES = [1, 3, 1000, 1 << 40]


def targets():
    """descriptors chosen for the paths the random ones seldom reach (what each is for: tests/test_geom_sanitizers.py, REACHED)"""
    e88, q1516, e55 = Qu(8, 8), Qu(15, 16), Qu(5, 5)
    l88 = dict(mul_args=Tags(17, 16), add_args=[Qu(29, 16)])
    out = [
        lower(e88, e88, Qu(24, 8), 4096, 4096, 4096, **l88),                                           # six products
        lower(e55, e55, Qu(16, 5), 2048, 2048, 512, mul_args=Tags(11, 10), add_args=[Qu(21, 10)]),      # Karatsuba 2 x 2
        lower(q1516, q1516, Qu(43, 32), 256, 256, 4096, mul_args=Tags(31, 32), add_args=[Qu(43, 32)]),  # wide composite, centred
        lower(e88, e88, Qu(34, 8), 128, 128, 100000, mul_args=Tags(17, 16), add_args=[Qu(35, 16)]),     # k-chunks
        # (the wide fuzzer's finds of tests/test_gpu_centred.py: row sums that would not fit keep the plain limbs)
        lower(Qu(44, 11), Qu(10, 21), Qu(48, 24, True, TRN.TCPL, SAT.SMGN), 16, 16, 43519, mul_args=Qu(55, 32), add_args=[Qu(71, 32)]),
        lower(Qu(13, 48, False), Qu(9, 14), Qu(5, 0, True, TRN.TCPL, SAT.TCPL), 257, 129, 7, transposed_a=True, mul_args=Qu(23, 62), add_args=[Qu(26, 62)]),
    ]
    for name in sorted(TB.BOUND):
        out += [TB.bound_case(name)[4], TB.bound_case(name, 1)[4]]   # at and one past the accumulators' exactness bound
    return out


def descriptors(n_random, n_compact):
    d = [desc_from_dict(j) for j in G.gemm_cases("real") + G.gemm_cases("cplx") + TW._gemm_cases()]
    d += [r[1] for r in TR.RINGS] + [r[1] for r in TR.NEIGHBOURS] + targets()
    for name in sorted(TG.ELIGIBLE):
        d += TG.group(name)
    for name in sorted(TG.FALLBACKS):
        e, ec, kw, _ = TG.FALLBACKS[name]
        d += [lower(e, e, ec, M, N, K, **kw) for M, N, K in TG.SHAPES[:3]]
    return d + random_descs(n_random, 11) + compact_form_descs(n_compact, 12)


def real_chains():
    """(descriptor, epilogue, tables, shared flags) of every batched-chain case and of the APPROX planner tests"""
    out = []
    for fmt in sorted(X.FORMATS):
        for shape in X.SHAPES:
            for chain in sorted(X.chains(X.E43)):
                d, ep, tabs, _, _, _, shared = X.lowered(fmt, shape, chain)
                out.append((d, ep, tabs, shared))
    for c, stages, dq in [(TA.X, [Approx(TA.TABLE)], TA.X), (Qu(15, 8), [TA.Ew("mul", Qu(3, 4), Tags(24, 8), scalar=True, into=TA.X), Approx(TA.TABLE), TA.Ew("mul", Qu(3, 4))], Qu(9, 3))]:
        ep, tabs = lower_epilogue_x(c, stages, dq)
        out.append((TA.ident(c), ep, tabs, None))
    for j in approx_ref.cases():
        fx, segs = approx_ref.case_table(j)
        ep, tabs = lower_epilogue_x(fx, [Approx(segs)], fx)
        out.append((TA.ident(fx), ep, tabs, None))
    return out


def cplx_chains():
    out = []
    for j in cmul_ref.cases():
        epc, cx, c, _ = cmul_ref.case_chain(j)
        out.append((TC.ident(c, j["n"]), epc, cx))
    return out


def queries(n_random=500, n_compact=250, n_groups=24):
    """[(kind, ...)]: ("plain", d, flags, chain), ("batched", d, batch, flags, chain, shared), ("grouped", descs, flags); chain = None or
    (entry point, struct, per-stage records): "ep" / "epx" (qgemul_epilogue, tables), "epc" / "epcx" (qgemul_epilogue_cplx, CMUL records)"""
    rng = random.Random(2024)
    descs = descriptors(n_random, n_compact)
    q = [("plain", d, f, None) for d in descs for f in FLAGS]
    chains = real_chains()
    for d, ep, tabs, _ in chains:
        for f in FLAGS:
            q.append(("plain", d, f, ("epx", ep, tabs)))
            if all(t is None for t in tabs):
                q.append(("plain", d, f, ("ep", ep, None)))
    for d, epc, cx in cplx_chains():
        for f in (0, capi.OPT_FORCE_TREE, capi.OPT_UNFUSED_EPILOGUE):
            q += [("plain", d, f, ("epcx", epc, cx)), ("plain", d, f, ("epc", epc, None))]
    members = descs[::max(1, len(descs) // 150)] + [c[0] for c in chains[::7]]
    q += [("batched", d, b, f, None, None) for d in members for b in BATCHES for f in FLAGS]
    for d, ep, tabs, shared in chains:
        for b in BATCHES:
            for f in (0, capi.OPT_FUSED_EPILOGUE, capi.OPT_UNFUSED_EPILOGUE):
                q.append(("batched", d, b, f, ("epx", ep, tabs), shared))
    groups = [TG.group(name) for name in sorted(TG.ELIGIBLE)] + [TG.group(name, TG.SHAPES + TG.SHAPES[::-1]) for name in sorted(TG.ELIGIBLE)]
    for name in sorted(TG.FALLBACKS):
        e, ec, kw, _ = TG.FALLBACKS[name]
        el = TG.group("e43", [(3, 5, 7), (65, 33, 100)])
        s = [lower(e, e, ec, 33, 17, 40, **kw), lower(e, e, ec, 5, 9, 40, **kw)]
        groups.append([s[0], el[0], s[1], el[1]])
    # 2^32 tiles in one launch: the "more than 2^31 - 1 tiles" refusal of a grouped plan (3 x 1 limbs: no two-group kernel takes a
    # large member of this pair away from the launch)
    ea, eb, ec, kw = X.FORMATS["e88_x_e43_3x1"][:4]
    groups.append([lower(ea, eb, ec, 1 << 22, 1 << 22, 1, **kw), lower(ea, eb, ec, 3, 5, 7, **kw)])
    groups.append([lower(X.E43, X.E43, Qu(4, 3), 0, 5, 7, **TG.L43)] + TG.group("e88", TG.SHAPES[:2]))
    small = [d for d in descs if d.M * d.N <= 1 << 16 and d.K <= 4096]
    for _ in range(n_groups):
        groups.append([rng.choice(small) for _ in range(rng.randint(1, 9))])
    q += [("grouped", g, f) for g in groups for f in FLAGS]
    return q


CHAIN_KIND = {"ep": 1, "epc": 2, "epx": 3, "epcx": 4}


def pack_query(q) -> bytes:
    kind = q[0]
    if kind == "grouped":
        return struct.pack("<IIqII", 2, q[2], len(q[1]), 0, 0) + b"".join(bytes(d) for d in q[1])
    d, n, flags, chain = (q[1], 0, q[2], q[3]) if kind == "plain" else (q[1], q[2], q[3], q[4])
    out = struct.pack("<IIqII", 0 if kind == "plain" else 1, flags, n, CHAIN_KIND[chain[0]] if chain else 0, 0) + bytes(d)
    if chain:
        out += bytes(chain[1])
        if chain[0] in ("epx", "epcx"):
            recs = (list(chain[2]) + [None] * capi.QG_MAX_EW)[:capi.QG_MAX_EW]
            out += bytes(1 if r is not None else 0 for r in recs) + b"".join(bytes(r) for r in recs if r is not None)
        if kind == "batched":
            out += bytes(batched_ep(q[5] or ()))
    return out


def info_fields(st, info):
    return {"st": st, "sup": info.supported, "cls": info.cls, "kernel": info.kernel, "limbs": list(info.limbs), "max_bits": info.max_bits, "in_bits": list(info.in_bits),
            "packed": list(info.packed_bytes), "ops": info.ops, "heb": list(info.host_elem_bytes), "hio": list(info.host_imag_off), "reason": bytes(info.reason).split(b"\0")[0].decode()}


def ask_library(q):
    """every field the classify entry points return for the query: info (when the entry point wrote one), launch counts, member records"""
    L = capi.lib()
    kind = q[0]
    if kind == "plain":
        _, d, flags, chain = q
        if chain is None:
            st, info = capi.classify_status(d, flags)
        elif chain[0] in ("ep", "epc"):
            st, info = capi.classify_ep_status(d, chain[1], flags)
        elif chain[0] == "epx":
            st, info = capi.classify_epx(d, chain[1], chain[2], flags)
        else:
            st, info = capi.classify_epcx(d, chain[1], chain[2], flags)
        return info_fields(st, info)
    if kind == "batched":
        _, d, batch, flags, chain, shared = q
        if chain is None:
            st, info = capi.classify_batched_status(d, batch, flags)
            n = capi.classify_batched_launches(d, batch, flags)
        else:
            st, info = capi.classify_batched_epx_status(d, batch, chain[1], chain[2], shared, flags)
            n = capi.classify_batched_epx_launches(d, batch, chain[1], chain[2], shared, flags)
        return dict(info_fields(st, info), launches=n)
    _, descs, flags = q
    st, info = capi.classify_grouped_status(descs, flags)
    out = dict(info_fields(st, info), launches=capi.classify_grouped_launches(descs, flags), members=[])
    arr = capi._desc_array(descs)
    for g in range(len(descs) if st == capi.QG_OK else 0):
        m = capi.qgemul_grouped_member()
        assert L.qgemul_classify_grouped_member(arr, len(descs), flags, g, C.byref(m)) == capi.QG_OK
        out["members"].append({"in": m.in_launch, "launches": m.launches, "off": list(m.off), "bytes": list(m.bytes), "tiles": [m.tiles_m, m.tiles_n, m.k_tiles]})
    return out
