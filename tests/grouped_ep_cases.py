"""Shared by tests/test_grouped_ep_plan.py (CPU) and tests/test_gpu_grouped_ep.py (GPU): the members, the chains and the expected
values of element-wise chains on grouped plans (include/qgemul.h, qgemul_*_grouped_ep*).  Not a test module.

Formats, chains and the oracle's restatement of a chain are those of tests/batched_ep_cases.py (FORMATS, chains, expected, bits32,
has_approx); the shared flags of its chains are ignored: a grouped chain's tensor operands are per member.  Every scalar stage of a
chain takes one raw value per member unless a case says otherwise."""
import numpy as np

import batched_ep_cases as X
from qublas_amd import capi
from qublas_amd.desc import Approx, Ew, Qu, RND, SAT, TRN, WRP, Tags, lower, lower_epilogue_x

POISON = X.POISON
FUSED, UNFUSED = capi.OPT_FUSED_EPILOGUE, capi.OPT_UNFUSED_EPILOGUE
# the issue's member shapes in ASCENDING K, so that the schedule (decreasing k-tile count) differs from list order; one empty member
SHAPES = [(64, 64, 1), (3, 5, 7), (0, 5, 7), (16, 200, 64), (129, 130, 65), (65, 33, 100), (1, 1, 300)]
# ... plus three members of 4 x 4 tiles: 64 tiles dealt in whole rounds and a ragged rest
BIG = [(200, 200, 70)] * 3
CHAINS = ["1_scale_shared_bias", "3_no_stage_narrow_sat", "4_four_stages_1_2_4_8_bytes", "5_act_uniform"]

# a chain whose every stage names its result type: ONE qgemul_epilogue that means the same after members of DIFFERENT C formats (the
# stragglers of a group); 32-bit arithmetic throughout, so the members in the launch can run it fused
T208, D126 = Qu(20, 8), Qu(12, 6, True, RND.CONV, SAT.TCPL)
MIXED = [Ew("mul", X.S34, Tags(20, 8), scalar=True, into=T208), Ew("add", X.B106, Tags(21, 8), into=Qu(21, 8)), Ew("sub", X.S34, Tags(22, 8), scalar=True)]
I16 = Qu(15, 0, True, TRN.TCPL, WRP.TCPL)
L43 = dict(mul_args=Tags(9, 6), add_args=[Qu(19, 6)])
# straggler kinds beside int<4,3> members in the launch: name -> (A element, B element, C element, lowering keywords, shape)
STRAGGLERS = {
    "tree_default_tags": (X.E88, X.E88, X.E88, {}, (33, 17, 40)),
    "ring_int16": (I16, I16, I16, {}, (33, 17, 40)),
    "raw_pass_left_shift": (Qu(10, -3), Qu(10, -3), Qu(24, 9), dict(mul_args=Tags(21, -6), add_args=[Qu(28, -6)]), (33, 17, 40)),
    "another_key_3x3": (X.E88, X.E88, X.C16, dict(mul_args=Tags(17, 16), add_args=[Qu(29, 16)]), (65, 33, 100)),
    "another_c_format": (X.E43, X.E43, Qu(5, 3), L43, (65, 33, 100)),
    "composite_long_k": (X.E43, X.E43, Qu(30, 3), dict(mul_args=Tags(9, 6), add_args=[Qu(27, 6)]), (5, 3, 140000)),
}


def is_scalar(st):
    return not isinstance(st, Approx) and st.scalar


def is_tensor(st):
    return not isinstance(st, Approx) and not st.scalar


class Chain:
    """ONE chain for a group: its stages, D's element type, the C-ABI structs (lowered against C type ec) and the per-member pattern"""

    def __init__(self, ec, stages, dq, per_member=None):
        self.ec, self.stages, self.dq = ec, list(stages), dq
        self.ep, self.tabs = lower_epilogue_x(ec, self.stages, dq)
        self.per_member = [1 if is_scalar(s) else 0 for s in self.stages] if per_member is None else list(per_member)

    @classmethod
    def named(cls, fmt, name, per_member=None):
        ec = X.FORMATS[fmt][2]
        stages, dq, _ = {**X.chains(ec), **X.branch_chains(ec)}[name]
        return cls(ec, stages, dq, per_member)


class Member:
    """one GEMM of a group with its chain operands: descriptor, leading dimensions (A, B, D, E), host operands, per stage a host tensor
    (tight or at leading dimension ld[3]), a raw scalar or None; the oracle's D"""

    def __init__(self, oracle, ea, eb, ec, shape, kw, chain, ta=False, seed=1, dist=0, ld=(0, 0, 0, 0)):
        M, N, K = shape
        self.ea, self.eb, self.ec, self.chain, self.dist, self.ld, self.seed = ea, eb, ec, chain, dist, ld, seed
        self.d = lower(ea, eb, ec, M, N, K, transposed_a=ta, **kw)
        self.empty = M == 0 or N == 0
        ra, ca = (K, M) if ta else (M, K)
        ext = lambda cols, rows, l: (cols - 1) * (l or rows) + rows if cols and rows else 0
        self.ext = (ext(ca, ra, ld[0]), ext(N, K, ld[1]), ext(N, M, ld[2]), ext(N, M, ld[3]))
        self.A = oracle.fill(ea, max(self.ext[0], 1), seed, dist)
        self.B = oracle.fill(eb, max(self.ext[1], 1), seed + 1000, dist)
        self.E, self.scal = [], []
        for k, st in enumerate(chain.stages):
            self.E.append(oracle.fill(st.e, max(self.ext[3], 1), seed + 2000 + k, 0) if is_tensor(st) else None)
            self.scal.append(int(oracle.fill(st.e, 1, seed + 3000 + k, 0)[0]) if is_scalar(st) else None)
        self._exp = {}

    def tight(self, v, l):
        M, N = self.d.M, self.d.N
        return v[:M * N] if not l or l == M else np.concatenate([v[j * l:j * l + M] for j in range(N)])

    def values(self, oracle, scal=None):
        """the member's D values (tight, M * N) with the scalars `scal` (None: its own)"""
        scal = self.scal if scal is None else scal
        key = tuple(scal)
        if key not in self._exp:
            M, N = self.d.M, self.d.N
            if self.empty:
                self._exp[key] = np.zeros(0, dtype=oracle.host_dtype(self.chain.dq))
            else:
                if "c" not in self._exp:
                    out = np.zeros(self.ext[2] + M, dtype=oracle.host_dtype(self.ec))
                    oracle.gemm(self.d, self.A, self.B, self.ec, lda=self.ld[0], ldb=self.ld[1], ldc=self.ld[2], out=out, nthreads=8)
                    self._exp["c"] = self.tight(out, self.ld[2]).astype(np.int64)
                Eo = []
                for k, st in enumerate(self.chain.stages):
                    Eo.append(None if isinstance(st, Approx) else np.asarray([scal[k]], dtype=np.int64) if st.scalar else self.tight(self.E[k], self.ld[3]).astype(np.int64))
                self._exp[key] = X.expected(oracle, self.ec, self.chain.stages, self.chain.dq, self._exp["c"], Eo).astype(oracle.host_dtype(self.chain.dq))
        return self._exp[key]

    def expected(self, oracle, scal=None):
        """the poisoned D buffer as it must look afterwards: the member's columns at ldd, poison between and behind them"""
        M, N = self.d.M, self.d.N
        buf = np.empty(max(self.ext[2], 1) + 8, dtype=oracle.host_dtype(self.chain.dq))
        buf.view(np.uint8)[:] = POISON
        v = self.values(oracle, scal)
        l = self.ld[2] or M
        for j in range(N if not self.empty else 0):
            buf[j * l:j * l + M] = v[j * M:(j + 1) * M]
        return buf


def fmt_member(oracle, fmt, shape, chain, **kw2):
    ea, eb, ec, kw, ta, _ = X.FORMATS[fmt]
    return Member(oracle, ea, eb, ec, shape, kw, chain, ta=kw2.pop("ta", ta), **kw2)


def up256(x):
    return (x + 255) // 256 * 256


class Device:
    """the members' host-layout operands on the device, back to back at 256-byte steps; D buffers poisoned (8 elements longer than the
    member: bytes behind a member are checked too)"""

    def __init__(self, ctx, oracle, members):
        self.ctx, self.members = ctx, members
        chain = members[0].chain
        self.host = {"A": [m.A for m in members], "B": [m.B for m in members], "D": []}
        for m in members:
            c = np.empty(max(m.ext[2], 1) + 8, dtype=oracle.host_dtype(chain.dq))
            c.view(np.uint8)[:] = POISON
            self.host["D"].append(c)
        for k, st in enumerate(chain.stages):
            if is_tensor(st):
                self.host[k] = [m.E[k] for m in members]
        self.base, self.offs = {}, {}
        for key, xs in self.host.items():
            offs, tot = [], 0
            for x in xs:
                offs.append(tot)
                tot += up256(x.nbytes)
            self.base[key] = ctx.alloc(max(16, tot))
            self.offs[key] = offs
            for x, o in zip(xs, offs):
                ctx.h2d(self.base[key] + o, x.view(np.uint8))

    def ptrs(self, key):
        return [0 if m.empty else self.base[key] + o for m, o in zip(self.members, self.offs[key])]

    def fetch_d(self):
        out = []
        for x, o in zip(self.host["D"], self.offs["D"]):
            y = np.empty_like(x)
            self.ctx.d2h(y.view(np.uint8), self.base["D"] + o)
            out.append(y)
        return out

    def reset_d(self):
        for x, o in zip(self.host["D"], self.offs["D"]):
            self.ctx.h2d(self.base["D"] + o, x.view(np.uint8))

    def close(self):
        for p in self.base.values():
            self.ctx.free(p)


def lds(members, w):
    return None if all(m.ld[w] == 0 for m in members) else [m.ld[w] for m in members]


class GroupedRun:
    """a grouped plan with a chain and its packed buffers: pack once, then execute_ep + unpack as often as a test likes"""

    def __init__(self, ctx, dev, flags=0, per_member=None, scalars=None, e_scalar=None):
        self.ctx, self.dev = ctx, dev
        members = dev.members
        chain = self.chain = members[0].chain
        self.per_member = chain.per_member if per_member is None else per_member
        self.plan = capi.GroupedPlan(ctx, [m.d for m in members], flags, ep=chain.ep, approx=chain.tabs, per_member=self.per_member)
        pb = self.plan.info.packed_bytes
        self.bufs = [ctx.alloc(max(16, b)) for b in pb]
        self.plan.pack(capi.OPERAND_A, dev.ptrs("A"), self.bufs[0], lds(members, 0))
        self.plan.pack(capi.OPERAND_B, dev.ptrs("B"), self.bufs[1], lds(members, 1))
        self.packed = [0] * len(chain.stages)
        for k, st in enumerate(chain.stages):
            if is_tensor(st):
                pe = ctx.alloc(max(16, self.plan.packed_e_bytes(k)))
                self.bufs.append(pe)
                self.plan.pack_e(k, dev.ptrs(k), pe, lds(members, 3))
                self.packed[k] = pe
            else:
                assert self.plan.packed_e_bytes(k) == 0
        self.e_scalar = [0] * len(chain.stages) if e_scalar is None else e_scalar
        for k, st in enumerate(chain.stages):
            if self.per_member[k] and scalars is not False:
                self.plan.set_scalars(k, [m.scal[k] for m in members] if scalars is None else scalars[k])

    def run(self):
        """execute_ep + unpack into the (re-poisoned) D buffers; returns them"""
        self.dev.reset_d()
        self.plan.execute_ep(self.bufs[2], self.bufs[0], self.bufs[1], capi.Plan.ep_args(packed=self.packed, scalars=self.e_scalar))
        self.plan.unpack_c(self.bufs[2], self.dev.ptrs("D"), lds(self.dev.members, 2))
        self.ctx.sync()
        return self.dev.fetch_d()

    def close(self):
        for p in self.bufs:
            self.ctx.free(p)
        self.plan.close()


def run_plain_loop(ctx, oracle, dev, scal=None):
    """the "was": every member through its own PLAIN _epx plan (qgemul_pack, qgemul_pack_e, qgemul_execute_ep, qgemul_unpack_c) into
    the poisoned D buffers; scal[g][k]: the scalars (None: the members' own)"""
    dev.reset_d()
    members = dev.members
    chain = members[0].chain
    pA, pB, pD = dev.ptrs("A"), dev.ptrs("B"), dev.ptrs("D")
    for g, m in enumerate(members):
        if m.empty:
            continue
        plan = capi.Plan(ctx, m.d, epilogue=chain.ep, approx=chain.tabs)
        pb = plan.info.packed_bytes
        bufs = [ctx.alloc(max(16, b)) for b in pb]
        try:
            plan.pack(capi.OPERAND_A, pA[g], bufs[0], m.ld[0])
            plan.pack(capi.OPERAND_B, pB[g], bufs[1], m.ld[1])
            packed, scalars = [0] * len(chain.stages), [0] * len(chain.stages)
            for k, st in enumerate(chain.stages):
                if is_scalar(st):
                    scalars[k] = (m.scal if scal is None else scal[g])[k]
                elif is_tensor(st):
                    pe = ctx.alloc(max(16, plan.packed_e_bytes(k)))
                    bufs.append(pe)
                    plan.pack_e(k, dev.ptrs(k)[g], pe, m.ld[3])
                    packed[k] = pe
            plan.execute_ep(bufs[2], bufs[0], bufs[1], capi.Plan.ep_args(packed=packed, scalars=scalars))
            plan.unpack_c(bufs[2], pD[g], m.ld[2])
            ctx.sync()
        finally:
            for p in bufs:
                ctx.free(p)
            plan.close()
    return dev.fetch_d()


def fusable(members):
    """the planner has bounded the chain by 32-bit arithmetic after the first eligible member, and it has no APPROX stage"""
    chain = members[0].chain
    m = next(m for m in members if not m.empty)
    return X.bits32(m.d, chain.ep, chain.tabs) and not X.has_approx(chain.stages)
