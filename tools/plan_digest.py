"""Byte identity of the planner's output between two revisions of qublas_amd/csrc/qg_plan.cpp: the acceptance check of a change
that must not move a planner decision or a byte of a device table.

    python tools/plan_digest.py --parent REV [--runs 5]

Builds tests/san/plan_san_driver.cpp with g++ -O2 twice — against REV's qg_plan.cpp (git show) and against the working tree's — and
feeds both `--digest` the corpus of tests/test_plan_digest.py.  Prints the corpus sizes, each side's status counts, coverage and
folded digest, whether the two outputs are identical line for line, and the wall time of each side over `--runs` runs.  CPU only.
Exit status 0: identical.
"""
from __future__ import annotations

import argparse
import os
import statistics
import subprocess
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]
PLAN = "qublas_amd/csrc/qg_plan.cpp"


def main() -> int:
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--parent", required=True, help="the revision whose qg_plan.cpp is the yardstick")
    ap.add_argument("--runs", type=int, default=5, help="timed runs per side")
    a = ap.parse_args()
    import test_plan_digest as T
    records = T.corpus()
    blob = T.wire(records)
    rev = subprocess.check_output(["git", "-C", ROOT, "rev-parse", a.parent], text=True).strip()
    print(f"parent {rev}")
    print(f"corpus {len(records)} records ({sum(1 for _, c in records if c is None)} descriptors, {sum(1 for _, c in records if c and c[0] == 'epx')} real chains, "
          f"{sum(1 for _, c in records if c and c[0] == 'epcx')} complex chains), {len(blob)} bytes")
    out = {}
    with tempfile.TemporaryDirectory() as tmp:
        old = os.path.join(tmp, "qg_plan.cpp")
        with open(old, "wb") as f:
            f.write(subprocess.check_output(["git", "-C", ROOT, "show", f"{rev}:{PLAN}"]))
        for side, src in (("parent", old), ("this", os.path.join(ROOT, PLAN))):
            exe = T.build_driver(os.path.join(tmp, "digest_" + side), ["-O2"], src)
            times = []
            for _ in range(a.runs):
                t0 = time.perf_counter()
                r = subprocess.run([exe, "--digest"], input=blob, capture_output=True, check=True)
                times.append(time.perf_counter() - t0)
            out[side] = r.stdout.decode().splitlines()
            print(f"{side}: lines {sum(1 for _ in open(src))}; " + "; ".join(out[side][-6:]))
            print(f"{side}: seconds per run " + " ".join(f"{t:.3f}" for t in times) + f"; median {statistics.median(times):.3f} min {min(times):.3f} max {max(times):.3f}")
    same = out["parent"] == out["this"]
    print(f"identical line for line: {'yes' if same else 'NO'} ({len(out['this'])} lines)")
    for i, (x, y) in enumerate(zip(out["parent"], out["this"])):
        if x != y:
            print(f"first difference, line {i}: {x!r} != {y!r}")
            break
    return 0 if same else 1


if __name__ == "__main__":
    sys.exit(main())
