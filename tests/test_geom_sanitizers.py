"""The plan geometry (qublas_amd/csrc/qg_geom.cpp: kernel choice, packed layouts, composite / batched / grouped forms) under
AddressSanitizer + UndefinedBehaviorSanitizer on the CPU, as tests/test_plan_sanitizers.py runs the analysis below it.  A stand-alone
driver (tests/san/geom_san_driver.cpp) answers the sweep of tests/geom_sweep.py as a child process; it must report nothing, agree with
the product library wherever the C-ABI exposes the quantity without a GPU, and have reached every form of plan the planner has."""
import os
import subprocess

import geom_sweep as S
from qublas_amd import capi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "qublas_amd", "csrc")


def build_driver(tmp):
    exe = os.path.join(tmp, "geom_san")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-fno-omit-frame-pointer",
                           os.path.join(ROOT, "tests", "san", "geom_san_driver.cpp"), os.path.join(CSRC, "qg_geom.cpp"), os.path.join(CSRC, "qg_plan.cpp"), "-o", exe])
    return exe


def fields(line):
    """{key: value} of one output line; lists of numbers as lists, the reason (last, may hold spaces) as text"""
    head, reason = line.split(" reason=", 1)
    out = {"reason": reason}
    for tok in head.split()[1:]:
        k, v = tok.split("=", 1)
        out[k] = [[float(x) if "." in x or "e" in x else int(x) for x in g.split(",")] for g in v.split(";")] if ";" in v else \
            [int(x) for x in v.split(",")] if "," in v else (float(v) if k == "ops" else int(v))
    return out


def test_geometry_under_asan_ubsan_agrees_with_the_library(tmp_path):
    exe = build_driver(str(tmp_path))
    qs = S.queries()
    blob = b"".join(S.pack_query(q) for q in qs)
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")
    r = subprocess.run([exe], input=blob, capture_output=True, env=env, timeout=300)
    assert r.returncode == 0, r.stderr.decode()[-3000:]
    assert b"runtime error" not in r.stderr and b"AddressSanitizer" not in r.stderr and b"LeakSanitizer" not in r.stderr, r.stderr.decode()[-3000:]
    lines = r.stdout.decode().splitlines()
    answers, extra = [], {}
    for ln in lines:
        if ln.startswith("  "):
            extra.setdefault(len(answers) - 1, []).append(ln.split())
        else:
            answers.append(fields(ln))
    assert len(answers) == len(qs)

    reached = set()
    kernels = set()
    for i, (q, a) in enumerate(zip(qs, answers)):
        lib = S.ask_library(q)
        ctx = (i, q[0], a["reason"], lib["reason"])
        # the C-ABI's view: status, and info wherever the entry point wrote one
        assert a["st"] == lib["st"], ctx
        for k in ("cls", "kernel", "limbs", "max_bits", "packed", "ops", "reason", "sup", "in_bits", "heb", "hio"):
            assert a[k] == lib[k], (k, a[k], lib[k]) + ctx
        if q[0] == "batched":
            assert (a["blaunches"] if a["st"] == 0 else a["st"]) == lib["launches"], ctx
        if q[0] == "grouped":
            assert (a["glaunches"] if a["st"] == 0 else a["st"]) == lib["launches"], ctx
            mem = [m for m in extra.get(i, []) if m[0] == "member"]
            assert len(mem) == len(lib["members"]) == (len(q[1]) if a["st"] == 0 else 0), ctx
            for m, want in zip(mem, lib["members"]):
                kv = dict(t.split("=", 1) for t in m[2:])
                got = {"in": int(kv["in"]), "launches": int(kv["launches"]), "off": [int(x) for x in kv["off"].split(",")], "bytes": [int(x) for x in kv["bytes"].split(",")],
                       "tiles": [int(x) for x in kv["tiles"].split(",")]}
                assert got == want, ctx
        if "more than 2^31 - 1 tiles" in a["reason"]:
            reached.add(q[0] + " overflow refusal")
        if a["st"] != 0:
            continue
        kernels.add(a["kernel"])
        if q[0] == "grouped":
            if 0 < a["n_in"] < len(q[1]):
                reached.add("group with stragglers")
            continue
        comp, pa = a["comp"][0], a["pa"]
        if comp[0] and comp[3] > 1:
            reached.add("composite, more than one k-chunk")
        if comp[0] and comp[6]:
            reached.add("wide composite")
        if pa[9]:
            reached.add("centred")
        if pa[7] and pa[3] == 2:
            reached.add("Karatsuba 2 x 2 layout")
        if a["cfg"][0] == 11 and pa[7] and pa[3] == 3:
            reached.add("six-product layout")
        if a["cfg"][0] == 12:
            reached.add("ring")
        if q[0] == "plain" and a["retreat"]:
            reached.add("centred retreat of a wide plan")
        if q[0] == "batched" and q[4] is not None and a["bd"]:
            reached.add("block-diagonal batch, fused chain" if a["bd_fused"] else "block-diagonal batch, chain as a pass")
    # every QG_KERNEL_* the planner returns (include/qgemul.h: 1 .. 10) and every form of plan
    assert kernels == set(range(1, 11)), kernels
    REACHED = {"composite, more than one k-chunk", "wide composite", "centred", "centred retreat of a wide plan", "Karatsuba 2 x 2 layout", "six-product layout", "ring",
               "block-diagonal batch, fused chain", "block-diagonal batch, chain as a pass", "group with stragglers", "batched overflow refusal", "grouped overflow refusal"}
    assert reached == REACHED, REACHED - reached
