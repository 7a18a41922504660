"""One thread, one cached plan, every kind of one-shot call in turn (qublas_amd/csrc/qg_run.hip: run_one_shot; qg_run_key.h: the key
the cached plan is recognised by).  Each single-feature test alternates two kinds at most; a key that conflated two others — a
batched plan taken for a plain one, a table or a CMUL record ignored, a shared operand taken for a per-member one, a group taken for
its first member or for the batch of its count, one member's K or the per-member pattern of a grouped chain ignored — would return
another plan's results without an error, and only a walk over all kinds, forwards and backwards, sees it."""
import numpy as np
import pytest

import batched_ep_cases as X
import cmul_ref as R
import grouped_ep_cases as GE
import test_gpu_batched as TB
import test_gpu_batched_ep as TE
import test_gpu_cmul as TC
import test_gpu_grouped as TG
from qublas_amd import capi
from qublas_amd.desc import Approx, Ew, EwC, Qu, lower, lower_epilogue, lower_epilogue_cplx_x, lower_epilogue_x

pytestmark = pytest.mark.gpu
POISON = X.POISON
GROUP = [(65, 33, 100), (3, 5, 7), (33, 17, 64)]   # the members of the grouped requests; the first is the walk's plain shape


def poisoned(n, dtype):
    out = np.empty(n, dtype=dtype)
    out.view(np.uint8)[:] = POISON
    return out


def requests(oracle):
    """[(name, call(out) -> None, out's length and dtype, expected bytes or (re, im))] in the order of the walk; pure host code
    except for the calls themselves"""
    ea, eb, ec, kw, _, _ = TB.FORMATS["q78_centred"]
    M, N, K = 65, 33, 100
    d = lower(ea, eb, ec, M, N, K, **kw)
    extA, extB, extC = X.extents(d)
    sC, sA, sB = extC + 9, extA + 1, extB + 2
    A, mA = X.host_batch(oracle, ea, 3, extA, sA, 40, (0, 1))
    B, mB = X.host_batch(oracle, eb, 3, extB, sB, 50, (0, 1))
    Cx = [oracle.gemm(d, a, b, ec, nthreads=8) for a, b in zip(mA, mB)]          # computed once, shared by every request below
    cdt = oracle.host_dtype(ec)
    out = []

    # plain, C with gaps between its columns
    ldc = M + 3
    out.append(("run", lambda o: capi.run(d, o, mA[0], mB[0], ldc=ldc), ((N - 1) * ldc + M, cdt),
                TB.expected_buffer(oracle, d, ec, 1, Cx[:1], 0, ldc).tobytes()))

    # the two-stage chain: MUL by a scalar, ADD of a tensor
    stages, dq, _ = X.chains(ec)["1_scale_shared_bias"]
    ep = lower_epilogue(ec, stages, dq)
    ddt = oracle.host_dtype(dq)
    shared = TE.Operands(oracle, stages, [0, 1], extC, 3)
    per = TE.Operands(oracle, stages, [0, 0], extC, 3, gap=3)

    def chain_members(ops):
        return [X.expected(oracle, ec, stages, dq, c.astype(np.int64), ops.of_member(b)[0]).astype(ddt) for b, c in enumerate(Cx)]
    exp_shared, exp_per = chain_members(shared), chain_members(per)
    out.append(("run_ep", lambda o: capi.run_ep(d, ep, o, mA[0], mB[0], shared.of_member(0)[1]), (extC, ddt), exp_shared[0].tobytes()))

    # a chain that ends in an APPROX stage (the scalar 2^-14 brings C into the table's range), with a table and with one that differs
    # in ONE coefficient by one unit
    act = [Ew("mul", Qu(1, 14), scalar=True, into=X.X312), Approx(X.UNIFORM2)]
    segs = [(bp, list(co)) for bp, co in X.UNIFORM2]
    segs[1][1][0] = (segs[1][1][0][0] + 1, segs[1][1][0][1])
    act2 = act[:-1] + [Approx(segs)]
    adq = X.FA
    adt = oracle.host_dtype(adq)
    scalar = np.ones(1, dtype=oracle.host_dtype(Qu(1, 14)))
    for name, chain in (("run_epx table 1", act), ("run_epx table 2", act2)):
        epx, tabs = lower_epilogue_x(ec, chain, adq)
        exp = X.expected(oracle, ec, chain, adq, Cx[0].astype(np.int64), [scalar.astype(np.int64), None]).astype(adt)
        out.append((name, lambda o, epx=epx, tabs=tabs: capi.run_epx(d, epx, tabs, o, mA[0], mB[0], [scalar, None]), (extC, adt), exp.tobytes()))
    assert bytes(lower_epilogue_x(ec, act, adq)[0]) == bytes(lower_epilogue_x(ec, act2, adq)[0]) and out[-1][3] != out[-2][3]

    # the complex sibling: a complex chain without and with a CMUL stage
    gname = "tree_1x1"
    cec, cM, cN = TC.GEMMS[gname][:3]
    cd, cA, cB, (cre, cim) = TC.gemm_case(oracle, gname)
    for name, cstages, cdq in (("run_epc", [EwC("add", TC.E1)], TC.D1), ("run_epcx", *TC.CHAINS["basic_tensor_e1_d1"])):
        epc, cx = lower_epilogue_cplx_x(cec, cstages, cdq)
        Eh, Ere, Eim = TC.operands(oracle, cstages, cM * cN)
        exp = R.chain(epc, cx, cec, cre, cim, Ere, Eim)
        if name == "run_epc":
            assert all(c is None for c in cx)
            call = lambda o, epc=epc, Eh=Eh: capi.run_ep(cd, epc, o, cA, cB, Eh)
        else:
            call = lambda o, epc=epc, cx=cx, Eh=Eh: capi.run_epcx(cd, epc, cx, o, cA, cB, Eh)
        out.append((name, call, (cM * cN, oracle.host_dtype(cdq)), exp))

    # batched, gaps between the members; then the batched chain with the ADD operand per member and shared
    for batch in (2, 3):
        out.append((f"run_batched {batch}", lambda o, batch=batch: capi.run_batched(d, batch, o, A, B, sC, sA, sB), ((batch - 1) * sC + extC, cdt),
                    TB.expected_buffer(oracle, d, ec, batch, Cx, sC).tobytes()))
    for name, ops, exp in (("run_batched_epx per member", per, exp_per), ("run_batched_epx shared", shared, exp_shared)):
        strideE = ops.stride + [0] * (4 - len(ops.stride))
        assert (strideE[1] == 0) == (ops is shared)
        out.append((name, lambda o, ops=ops, strideE=strideE: capi.run_batched_epx(d, 3, ep, None, o, A, B, ops.host, sC, sA, sB, strideE), (2 * sC + extC, ddt),
                    TE.expected_buffer(oracle, d, dq, 3, exp, sC).tobytes()))
    assert exp_per[0].tobytes() != exp_shared[0].tobytes()

    # grouped, the members' outputs back to back in the one buffer.  Behind the batched chains the same chain on a group, with one
    # scalar for all and with stage 0 per member; then a group without a chain, and the same with only the LAST member's K changed
    def views(o, members):
        ends = np.cumsum([m.ext[2] for m in members])
        return [o[e - m.ext[2]:e] for m, e in zip(members, ends)]

    gchain = GE.Chain.named("q78_centred", "1_scale_shared_bias")
    assert bytes(gchain.ep) == bytes(ep)
    gm = [GE.fmt_member(oracle, "q78_centred", s, gchain, seed=880 + i, dist=1 if i == 0 else 0) for i, s in enumerate(GROUP)]
    wide = 2                                        # the scalar for all; per member: 3, 4, 5
    for i, m in enumerate(gm):
        m.scal = [3 + i, None]
    exp_wide, exp_own = [m.values(oracle, [wide, None]) for m in gm], [m.values(oracle) for m in gm]
    assert all(w.tobytes() != o.tobytes() for w, o in zip(exp_wide, exp_own))
    E1 = [m.E[1] for m in gm]
    for name, pm, E0, S0, exp in (("run_grouped_epx one scalar", [0, 0], np.asarray([wide], dtype=oracle.host_dtype(stages[0].e)), None, exp_wide),
                                  ("run_grouped_epx stage 0 per member", [1, 0], None, [m.scal[0] for m in gm], exp_own)):
        out.append((name, lambda o, pm=pm, E0=E0, S0=S0: capi.run_grouped_epx([m.d for m in gm], gchain.ep, gchain.tabs, pm, views(o, gm), [m.A for m in gm],
                                                                             [m.B for m in gm], [E0, E1], [S0, None]),
                    (sum(m.ext[2] for m in gm), ddt), b"".join(e.tobytes() for e in exp)))
    g3 = [TG.fmt_member(oracle, "q78_centred", s, seed=890 + i, dist=1 if i == 0 else 0) for i, s in enumerate(GROUP)]
    g3k = g3[:2] + [TG.fmt_member(oracle, "q78_centred", GROUP[2][:2] + (65,), seed=892, dist=0)]
    assert g3k[0].d is g3[0].d
    for name, ms in (("run_grouped", g3), ("run_grouped last K", g3k)):
        out.append((name, lambda o, ms=ms: capi.run_grouped([m.d for m in ms], views(o, ms), [m.A for m in ms], [m.B for m in ms]),
                    (sum(m.ext[2] for m in ms), cdt), b"".join(m.expected(oracle).tobytes() for m in ms)))
    # ... and, in front of the plain call, the group that holds the plain call's descriptor alone
    out.insert(0, ("run_grouped [d]", lambda o: capi.run_grouped([d], [o], [mA[0]], [mB[0]]), (extC, cdt), TB.expected_buffer(oracle, d, ec, 1, Cx[:1], 0).tobytes()))
    return out


def test_one_thread_alternates_every_entry_kind(oracle):
    reqs = requests(oracle)
    assert len(reqs) == 15
    try:
        for name, call, (n, dtype), exp in reqs + reqs[::-1]:
            got = poisoned(n, dtype)
            call(got)
            if isinstance(exp, bytes):
                assert got.tobytes() == exp, name
            else:   # complex elements: the parts (a host element may have padding of its own)
                assert np.array_equal(got["re"].astype(np.int64), exp[0]) and np.array_equal(got["im"].astype(np.int64), exp[1]), name
    finally:
        capi.run_release()
