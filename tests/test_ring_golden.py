"""The oracle (oracle/qoracle.c) equals the REFERENCE's own C on every record of tests/golden/ref_ring_0.jsonl.gz: GEMMs whose product
and tree levels wrap (plain C integers of 8 / 12 / 16 / 24 / 32 bits, a saturating C behind an int16 ring, a ring entered by a left
shift; generator: tests/golden_src/ref_cases_ring.cpp on the reference's header).  This pins the checker the GPU tests of the ring
plans lean on; and the cases really wrap — almost no output equals the unwrapped dot product."""
import numpy as np
import pytest

import golden_io as G
from qublas_amd.desc import desc_from_dict

RECORDS = list(G._records(G.GOLD + "/ref_ring_0.jsonl.gz"))


def test_the_fixture_is_complete():
    assert len(RECORDS) == 17
    assert {j["mul"][0][0] + j["mul"][0][1] + 1 for j in RECORDS} == {8, 12, 16, 24, 32}


@pytest.mark.parametrize("j", RECORDS, ids=lambda j: j["name"])
def test_oracle_equals_reference(oracle, j):
    d = desc_from_dict(j)
    _, _, ec = G.case_elems(j)
    A, B = G.case_inputs(j, oracle)
    exp = G.case_expected(j, oracle)
    assert np.array_equal(oracle.gemm(d, A, B, ec), exp)
    M, N, K = j["M"], j["N"], j["K"]
    a = A.astype(object).reshape(M, K) if j["transA"] else A.astype(object).reshape(K, M).T
    exact = a.dot(B.astype(object).reshape(N, K).T).T.reshape(-1)
    if "satC" not in j["name"] and "lshift" not in j["name"]:
        n = j["mul"][0][0] + j["mul"][0][1] + 1
        wrapped = np.array([((int(v) + (1 << (n - 1))) % (1 << n)) - (1 << (n - 1)) for v in exact], dtype=np.int64)
        assert np.array_equal(wrapped, exp.astype(np.int64))          # plain modular arithmetic, a third opinion
    assert int((exact != exp.astype(object)).sum()) > 0.9 * M * N     # the outputs really left the ring's range
