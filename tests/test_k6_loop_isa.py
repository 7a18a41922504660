"""The k-loop of k_mfma_k6 (qg_mfma_k6.hip) in the ISA hipcc emits for gfx950, for each of the four instantiations.  The loop body is
the basic block that holds the 15 ds_read_b128 of a k-tile.
MFMA interval (s_setprio 1 ... s_setprio 0): 36 MFMAs, the first instruction is one, never more than three vector instructions
between two of them (an in-order wave cannot issue the next MFMA behind a longer run), and no s_nop (every sum is formed at least
one MFMA ahead of the MFMA that reads it).
LOAD interval (start of the block ... s_setprio 1): the 15 reads and the 6 LDS-DMA issues, each DMA address a scalar base plus a
32-bit lane offset, and no vector ALU instruction at all: beside a partner at priority 1 each one would wait for an issue slot.
Epilogue: every row sum is loaded ahead of the first store of C, so that no wait behind a load also waits for stores.
hipcc cross-compiles without a GPU: CPU only."""
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "qublas_amd", "csrc", "qg_mfma_k6.hip")
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
MFMA = "v_mfma_i32_16x16x64_i8"


def parse(asm):
    """{symbol: [basic blocks, each a list of instructions]} of the k_mfma_k6 kernels in an assembly file"""
    out, cur = {}, None
    for ln in open(asm):
        m = re.match(r"^(_Z\w*k_mfma_k6\w*):", ln)
        if m:
            cur = out.setdefault(m.group(1), [[]])
            continue
        if ln.startswith(".Lfunc_end"):
            cur = None
        if cur is None:
            continue
        if re.match(r"^\.LBB\d+_\d+:", ln):
            cur.append([])
            continue
        ins = ln.split(";")[0].strip()
        if ins and not ins.startswith("."):
            cur[-1].append(ins)
    return out


@pytest.fixture(scope="module")
def kernels(tmp_path_factory):
    if not os.path.exists(HIPCC):
        pytest.skip("needs hipcc")
    asm = str(tmp_path_factory.mktemp("k6loop") / "k6.s")
    r = subprocess.run([HIPCC, "--offload-arch=gfx950", "-O3", "-std=c++17", "-x", "hip", "--cuda-device-only", "-S", SRC, "-o", asm],
                       capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]
    out = parse(asm)
    assert len(out) == 4, sorted(out)
    return out


def op(ins):
    return ins.split()[0]


def loop_block(blocks):
    hits = [b for b in blocks if sum(1 for s in b if op(s) == "ds_read_b128") == 15]
    assert len(hits) == 1, [sum(1 for s in b if op(s) == "ds_read_b128") for b in blocks]
    return hits[0]


def split(block):
    up = [i for i, s in enumerate(block) if s.replace(" ", "") == "s_setprio1"]
    down = [i for i, s in enumerate(block) if s.replace(" ", "") == "s_setprio0"]
    assert len(up) == 1 and len(down) == 1 and up[0] < down[0], (up, down)
    return block[:up[0]], block[up[0] + 1:down[0]]


def test_mfma_interval_is_paced(kernels):
    for name, blocks in kernels.items():
        _, mfma = split(loop_block(blocks))
        assert sum(1 for s in mfma if op(s) == MFMA) == 36, name
        assert not any(op(s) == "s_nop" for s in mfma), (name, [s for s in mfma if op(s) == "s_nop"])
        first = next(s for s in mfma if not op(s).startswith("s_waitcnt"))
        assert op(first) == MFMA, (name, first)
        run = longest = 0
        for s in mfma:
            if op(s) == MFMA:
                run = 0
            elif op(s).startswith("v_"):
                run += 1
                longest = max(longest, run)
        assert longest <= 3, (name, longest)


def test_load_interval_has_no_vector_alu(kernels):
    for name, blocks in kernels.items():
        load, _ = split(loop_block(blocks))
        assert sum(1 for s in load if op(s) == "ds_read_b128") == 15, name
        dma = [s for s in load if op(s).startswith("global_load_lds_")]
        assert len(dma) == 6, (name, dma)
        for s in dma:      # global_load_lds_dwordx4 v1, s[4:5] offset:...: a 32-bit lane offset beside a scalar base
            assert re.match(r"^global_load_lds_dword(x4)?\s+v\d+,\s*s\[\d+:\d+\]", s), (name, s)
        assert not [s for s in load if op(s).startswith("v_")], (name, [s for s in load if op(s).startswith("v_")])


def test_row_sums_are_loaded_before_the_first_store(kernels):
    for name, blocks in kernels.items():
        k = next(i for i, b in enumerate(blocks) if sum(1 for s in b if op(s) == "ds_read_b128") == 15)
        tail = [s for b in blocks[k + 1:] for s in b]
        stores = [i for i, s in enumerate(tail) if op(s).startswith("global_store")]
        assert stores, name
        # the tile body does lie behind the loop block: its 14 row sums (2 of B, 12 of A) are loaded in it, ahead of the first store
        early = [s for s in tail[:stores[0]] if op(s).startswith("global_load_dword")]
        assert len(early) >= 8, (name, early)
        late =[s for s in tail[stores[0]:] if op(s).startswith("global_load_dword")]
        assert not late, (name, late)
