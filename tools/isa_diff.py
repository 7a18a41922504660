"""Do two source trees compile to the same gfx950 code?  (the acceptance check of a refactoring that must not move a timing)

    python tools/isa_diff.py <parent-tree> <child-tree> [--sources a.hip b.hip ...] [--workdir DIR] [--report FILE] [--diag]

Every source is compiled in both trees with the flags of qublas_amd/build.py plus `--cuda-device-only -S`, and the two assembly
texts are compared per function symbol: every instruction with its operands, in order, and the kernel's metadata (vector, accumulator
and scalar registers, both spill counts, scratch and LDS bytes).  Only what cannot affect execution is normalised away: comments,
assembler directives, the per-translation-unit `__hip_cuid_` symbol and the function ordinal inside local label names
(.LBB<ordinal>_<n>: it changes when a function is added or removed in front).  The script compares; it searches for nothing.
Below the table, every differing symbol gets a note: how many lines differ, the lines themselves where they are few, and for a kernel
with MFMAs whether the stretch from its first to its last MFMA (the k-loop) is among them.
Exit status 1 when a symbol differs or exists in one tree only.  hipcc cross-compiles without a GPU.
"""
from __future__ import annotations

import argparse
import difflib
import os
import re
import subprocess
import sys
import tempfile
from concurrent.futures import ThreadPoolExecutor

META = [("vgpr", ".vgpr_count"), ("agpr", ".agpr_count"), ("sgpr", ".sgpr_count"), ("vspill", ".vgpr_spill_count"),
        ("sspill", ".sgpr_spill_count"), ("scratch", ".private_segment_fixed_size"), ("lds", ".group_segment_fixed_size")]


def build_module(tree: str):
    sys.path.insert(0, tree)
    try:
        for m in [m for m in sys.modules if m == "qublas_amd" or m.startswith("qublas_amd.")]:
            del sys.modules[m]
        from qublas_amd import build
        return build
    finally:
        sys.path.pop(0)


def kernel_sources(tree: str):
    """every unit of the tree's build list (a host-only unit compiles to no device symbol and adds no line)"""
    return list(build_module(tree).SOURCES)


def compile_asm(tree: str, src: str, out: str, flags, diag: bool):
    csrc = os.path.join(tree, "qublas_amd", "csrc")
    if not os.path.exists(os.path.join(csrc, src)):
        return None   # a unit of the other tree only: its symbols are looked for in this tree's other units
    deps = [os.path.join(csrc, f) for f in os.listdir(csrc)]
    if os.path.exists(out) and all(os.path.getmtime(d) < os.path.getmtime(out) for d in deps):
        return out
    cmd = [os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")] + flags + ["--cuda-device-only", "-S", os.path.join(csrc, src), "-o", out]
    r = subprocess.run(cmd + (["-DQG_DIAG"] if diag else []), capture_output=True, text=True)
    if r.returncode != 0:
        raise RuntimeError(f"hipcc failed on {tree}: {src}\n{r.stderr[-3000:]}")
    return out


def parse(path: str):
    """{symbol: {"insts": [...], "meta": {...} or None}} of one assembly file"""
    if path is None:
        return {}
    text = open(path).read()
    funcs = {}
    names = set(re.findall(r"^\s*\.type\s+(\S+),@function", text, re.M))
    cur = None
    for ln in text.splitlines():
        s = ln.split(";", 1)[0].strip()
        if not s:
            continue
        m = re.match(r"^([^\s:]+):$", s)
        if m and m.group(1) in names:
            cur = funcs.setdefault(m.group(1), {"insts": [], "meta": None})["insts"]
            continue
        if s.startswith(".Lfunc_end"):
            cur = None
        if cur is None or (s.startswith(".") and not s.startswith(".LBB")):
            continue
        s = re.sub(r"\.LBB\d+_", ".LBB_", s)
        cur.append(re.sub(r"__hip_cuid_[0-9a-f]+", "__hip_cuid_", " ".join(s.split())))
    kernels = text.split("amdhsa.kernels:", 1)[-1].split("amdhsa.target:", 1)[0]
    for block in re.split(r"^  - (?=\.agpr_count:)", kernels, flags=re.M)[1:]:
        sym = re.search(r"^\s+\.symbol:\s+(\S+)\.kd", block, re.M).group(1)
        vals = {}
        for key, field in META:
            m = re.search(r"^\s*" + re.escape(field) + r":\s+(\d+)", block, re.M)
            vals[key] = int(m.group(1)) if m else 0
        funcs.setdefault(sym, {"insts": [], "meta": None})["meta"] = vals
    return funcs


def main() -> int:
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("parent")
    ap.add_argument("child")
    ap.add_argument("--sources", nargs="+", help="default: every unit with device code of either tree's qublas_amd/build.py list")
    ap.add_argument("--workdir", help="keep the assembly here (re-used while it is newer than the tree's csrc/)")
    ap.add_argument("--report", help="also write the table to this file")
    ap.add_argument("--diag", action="store_true", help="compare the diagnostic build (-DQG_DIAG)")
    a = ap.parse_args()
    work = a.workdir or tempfile.mkdtemp(prefix="isa_diff_")
    trees = {"parent": os.path.abspath(a.parent), "child": os.path.abspath(a.child)}
    flags = list(build_module(trees["child"]).FLAGS)
    if not a.sources:
        a.sources = kernel_sources(trees["child"])
        a.sources += [s for s in kernel_sources(trees["parent"]) if s not in a.sources]
    jobs = []
    with ThreadPoolExecutor(max_workers=min(16, os.cpu_count() or 1)) as ex:
        for side, tree in trees.items():
            os.makedirs(os.path.join(work, side), exist_ok=True)
            for s in a.sources:
                out = os.path.join(work, side, s.rsplit(".", 1)[0] + (".diag.s" if a.diag else ".s"))
                jobs.append((side, s, ex.submit(compile_asm, tree, s, out, flags, a.diag)))
    asm = {(side, s): parse(f.result()) for side, s, f in jobs}

    # a symbol is compared with the one of its name in the same unit of the other tree; where that unit has none (the kernel has
    # moved to another file), with the one of its name in the only other unit that has it
    def where(side, sym, src):
        if sym in asm[(side, src)]:
            return src
        hits = [s for s in a.sources if sym in asm[(side, s)]]
        return hits[0] if len(hits) == 1 else None

    def mfma_span(insts):
        at = [i for i, x in enumerate(insts) if x.startswith("v_mfma")]
        return insts[at[0]:at[-1] + 1] if at else []

    lines, notes, bad = [], [], 0
    for s in a.sources:
        p, c = asm[("parent", s)], asm[("child", s)]
        for sym in sorted(set(p) | set(c)):
            ps, cs = where("parent", sym, s), where("child", sym, s)
            if cs is not None and cs != s:
                continue   # moved: reported under the child's unit
            fp, fc = asm[("parent", ps)][sym] if ps else None, c.get(sym)
            if fp is None or fc is None:
                lines.append(f"{s} {sym} only in {'child' if fp is None else 'parent'}")
                bad += 1
                continue
            s_shown = s if ps == s else f"{s} (parent: {ps})"
            same = fp["insts"] == fc["insts"] and fp["meta"] == fc["meta"]
            bad += 0 if same else 1
            if not same:
                # per differing symbol: the differing lines where they are few (unified diff of the instruction lists, parent - /
                # child +), and whether anything between the first and the last MFMA, the k-loop, is among them
                d = [x for x in difflib.unified_diff(fp["insts"], fc["insts"], lineterm="", n=0) if not x.startswith(("---", "+++"))]
                span = "" if not mfma_span(fp["insts"]) else f", first..last MFMA identical={'yes' if mfma_span(fp['insts']) == mfma_span(fc['insts']) else 'NO'}"
                notes.append(f"# {sym}: {sum(x[0] in '+-' for x in d)} differing lines{span}")
                notes += ["#   " + x for x in d] if len(d) <= 24 else []
            fmt = lambda m: "-" if m is None else " ".join(f"{k}={v}" for k, v in m.items())
            meta = fmt(fc["meta"]) if fp["meta"] == fc["meta"] else f"parent[{fmt(fp['meta'])}] child[{fmt(fc['meta'])}]"
            lines.append(f"{s_shown} {sym} insts={len(fp['insts'])}/{len(fc['insts'])} identical={'yes' if same else 'NO'} {meta}")
    lines.append(f"# {len(lines) - bad} of {len(lines)} symbols identical")
    lines += notes
    print("\n".join(lines))
    if a.report:
        with open(a.report, "w") as f:
            f.write("\n".join(lines) + "\n")
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())
