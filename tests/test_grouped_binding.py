"""QgemulGrouped_lower of both C++ headers (include/QuBLAS_amd.h, include/qgemul_reference_binding.hpp): byte for byte the descriptors
Qgemul's lowering gives for each triple, and the ones qublas_amd/desc.py lowers.  No GPU: lowering only."""
import json
import os
import subprocess

import pytest

from qublas_amd.desc import Qu, Tags, lower

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLANG = "/opt/rocm/lib/llvm/bin/clang++"
REF_INC = os.environ.get("REF_INC", "/root/reference/include")

E43, E88, W16 = Qu(4, 3), Qu(8, 8), Qu(16, 3)
L43 = dict(mul_args=Tags(9, 6), add_args=[Qu(19, 6)])
L88 = dict(mul_args=Tags(17, 16), add_args=[Qu(29, 16)])
PROBED = {
    "e43_L_three_shapes": [lower(E43, E43, W16, M, N, K, **L43) for M, N, K in ((64, 64, 64), (65, 33, 100), (3, 5, 7))],
    "e88_L_tn_two_shapes": [lower(E88, E88, Qu(24, 8), M, N, K, transposed_a=True, **L88) for M, N, K in ((33, 17, 40), (5, 9, 130))],
    "e88_default_one": [lower(E88, E88, E88, 3, 5, 7)],
}


def _probe(tmp_path, src, extra=()):
    exe = tmp_path / os.path.splitext(src)[0]
    subprocess.check_call([CLANG, "-std=c++23", "-O0", "-w", "-I" + os.path.join(ROOT, "include"), "-I" + os.path.join(ROOT, "tests", "binding"), *extra,
                           os.path.join(ROOT, "tests", "binding", src), "-o", str(exe)])
    return {l["name"]: l for l in (json.loads(x) for x in subprocess.check_output([str(exe)], text=True).strip().splitlines())}


def _check(recs):
    assert sorted(recs) == sorted(PROBED)
    for name, descs in PROBED.items():
        r = recs[name]
        assert r["grouped"] == r["single"], name
        assert r["grouped"] == [bytes(d).hex() for d in descs], name


@pytest.mark.skipif(not os.path.exists(CLANG), reason="needs AMD clang (C++23)")
def test_standalone_header_lowers_every_triple_as_qgemul_does(tmp_path):
    _check(_probe(tmp_path, "amd_header_grouped_probe.cpp"))


@pytest.mark.skipif(not os.path.exists(CLANG), reason="needs AMD clang (C++23)")
def test_reference_binding_lowers_every_triple_as_qgemul_does(tmp_path):
    if not os.path.exists(os.path.join(REF_INC, "QuBLAS.h")):
        pytest.skip("the reference header is not on this machine")
    _check(_probe(tmp_path, "ref_binding_grouped_probe.cpp", ["-I" + REF_INC]))
