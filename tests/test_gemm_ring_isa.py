"""CPU-only: the gfx950 code of every gemm_fp4_ring_kernel instantiation in libfpq_hip.so (FPQ_GEMM_CFG 40, fpq_gemm_fp4.h), read
from the library's code objects the way tests/test_no_spill.py reads them.  The kernel's LDS-DMA loads are assembly the compiler
does not see, and its one purpose is that they stay in flight across the loop's barrier: a compiler-inserted `vmcnt` wait in the
loop leaves it correct and silently takes that away.  So: no spill, no scratch, dynamic LDS only; the steady-state loop waits
once, with the count the source states; the drain waits with the shrinking counts down to one spelled-out vmcnt(0); no vmcnt
wait stands among a group's MFMAs."""
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB = os.path.join(ROOT, "fpqvar_amd", "libfpq_hip.so")
LLVM = "/opt/rocm/lib/llvm/bin"
MAGIC = b"__CLANG_OFFLOAD_BUNDLE__"
KERNEL = "gemm_fp4_ring_kernel"
PIECES = 3            # LDS-DMA pieces per wavefront and stage: the 64 x 128 tile's twelve 1 KiB blocks over four wavefronts
MFMAS_PER_GROUP = 8   # MT x NT = 2 x 4 tiles per wavefront


def _tool(name):
    p = os.path.join(LLVM, name)
    return p if os.path.exists(p) else shutil.which(name)


def _stages():
    src = open(os.path.join(ROOT, "fpqvar_amd", "csrc", "fpq_gemm_fp4.h")).read()
    return int(re.search(r"#define FPQ_GEMM_RING_STAGES (\d+)", src).group(1))


@pytest.fixture(scope="module")
def code_objects(tmp_path_factory):
    """[(disassembly lines, notes text)] of the gfx950 code objects that hold the kernel"""
    import __graft_entry__ as g
    g.build_hip()
    tools = {t: _tool(t) for t in ("llvm-objcopy", "clang-offload-bundler", "llvm-readelf", "llvm-objdump")}
    assert all(tools.values()), f"LLVM binutils of the ROCm toolchain not found: {tools}"
    tmp = tmp_path_factory.mktemp("ring_isa")
    fat = str(tmp / "fatbin")
    subprocess.run([tools["llvm-objcopy"], "-O", "binary", "--only-section=.hip_fatbin", LIB, fat], check=True)
    data = open(fat, "rb").read()
    starts = [m.start() for m in re.finditer(re.escape(MAGIC), data)]
    assert starts, "no offload bundle in .hip_fatbin"
    out = []
    for k, a in enumerate(starts):
        b = starts[k + 1] if k + 1 < len(starts) else len(data)
        bundle, elf = str(tmp / f"bundle{k}"), str(tmp / f"co{k}.elf")
        open(bundle, "wb").write(data[a:b])
        subprocess.run([tools["clang-offload-bundler"], "--unbundle", "--type=o", "--targets=hipv4-amdgcn-amd-amdhsa--gfx950",
                        f"--input={bundle}", f"--output={elf}"], check=True)
        notes = subprocess.run([tools["llvm-readelf"], "--notes", elf], check=True, capture_output=True, text=True).stdout
        if KERNEL not in notes:
            continue
        dis = subprocess.run([tools["llvm-objdump"], "-d", elf], check=True, capture_output=True, text=True).stdout
        out.append((dis.splitlines(), notes))
    assert out, f"no code object holds {KERNEL}"
    return out


def _records(notes):
    """[{key: value}] of the kernels in a code object's metadata note"""
    recs, cur = [], None
    for line in notes.splitlines():
        m = re.match(r"\s*-?\s*\.(\w+):\s*(.*)$", line)
        if not m:
            continue
        key, val = m.group(1), m.group(2).strip().strip("'\"")
        if key == "agpr_count" and (cur is None or "agpr_count" in cur):   # first key of a kernel's record
            cur = {}
            recs.append(cur)
        if cur is not None:
            cur[key] = val
    return [r for r in recs if KERNEL in r.get("name", "")]


def test_every_instantiation_is_there_without_spill_scratch_or_static_lds(code_objects):
    recs = [r for _, notes in code_objects for r in _records(notes)]
    names = sorted(r["name"] for r in recs)
    # {fp16, fp32 weight scales} x {plain / split, q / k norm, fc1}
    assert len(names) == 6 and all(sum(x in n for n in names) == 2 for x in ("GemmNoFc1", "GemmQkNorm", "GemmFc1")), names
    assert not any("gemm_fp4_glds_kernel" in n for n in names)
    for r in recs:
        what = r["name"][:120]
        assert int(r.get("vgpr_spill_count", 0)) == 0 and int(r.get("sgpr_spill_count", 0)) == 0, what
        assert int(r.get("private_segment_fixed_size", 0)) == 0, what
        assert int(r["group_segment_fixed_size"]) == 0, what             # dynamic LDS only, as the two-stage kernel
        assert int(r["vgpr_count"]) + int(r.get("agpr_count", 0)) <= 168, (what, r["vgpr_count"])


def _kernels(lines):
    """[(symbol, [(address, instruction text)])] of the ring kernels in a disassembly"""
    out, cur = [], None
    for l in lines:
        h = re.match(r"^[0-9a-f]+ <(.*)>:$", l)
        if h:
            cur = [] if KERNEL in h.group(1) else None
            if cur is not None:
                out.append((h.group(1), cur))
            continue
        m = re.match(r"\t(.*?)\s*// ([0-9A-Fa-f]+):", l)
        if m and cur is not None:
            cur.append((int(m.group(2), 16), " ".join(m.group(1).split())))
    return out


def _branch_target(addr, text):
    off = int(text.split()[1])
    return addr + 4 + 4 * (off - 65536 if off >= 32768 else off)


def test_waits_of_the_ring(code_objects):
    S = _stages()
    steady = f"s_waitcnt vmcnt({PIECES * (S - 2)})"
    checked = 0
    for lines, _ in code_objects:
        for name, ops in _kernels(lines):
            what = name[:100]
            mf = [a for a, o in ops if o.startswith("v_mfma")]
            # two copies of a group's MFMAs: the steady-state loop's and the drain's
            assert len(mf) == 2 * MFMAS_PER_GROUP, (what, len(mf))
            groups = (mf[:MFMAS_PER_GROUP], mf[MFMAS_PER_GROUP:])
            for grp in groups:   # no vmcnt wait, and no way out, among the MFMAs of a group
                inside = [o for a, o in ops if grp[0] <= a <= grp[-1]]
                assert not [o for o in inside if "vmcnt" in o or o.startswith(("s_cbranch", "s_branch"))], (what, inside)
            back = [(a, _branch_target(a, o)) for a, o in ops if o.startswith(("s_cbranch", "s_branch")) and _branch_target(a, o) <= a]
            # the steady-state loop: the backward branch around the first group that stays in front of the second
            loops = [(t, a) for a, t in back if t <= groups[0][0] and groups[0][-1] < a < groups[1][0]]
            assert len(loops) == 1, (what, loops)
            lo, hi = loops[0]
            body = [o for a, o in ops if lo <= a <= hi]
            assert [o for o in body if "vmcnt" in o] == [steady], (what, [o for o in body if "vmcnt" in o])
            assert sum(o.startswith("global_load_lds_dwordx4") for o in body) == PIECES and "s_barrier" in body, what
            # the drain: every backward branch that lands at or in front of the second group's MFMAs, behind the steady loop
            drain = [(t, a) for a, t in back if hi < t <= groups[1][-1]]
            assert drain, what
            d_lo, d_hi = min(t for t, _ in drain), max(a for _, a in drain)
            assert d_lo <= groups[1][0] and d_hi > groups[1][-1], (what, hex(d_lo), hex(d_hi))
            d_body = [o for a, o in ops if d_lo <= a <= d_hi]
            assert not any(o.startswith("global_load") for o in d_body), what       # nothing is requested any more
            waits = sorted(int(re.fullmatch(r"s_waitcnt vmcnt\((\d+)\)", o).group(1)) for o in d_body if "vmcnt" in o)
            # the shrinking counts, each once (the steady count may stand twice: the switch's default and its own case)
            assert sorted(set(waits)) == [PIECES * n for n in range(S - 1)], (what, waits)
            assert waits.count(0) == 1 and all(waits.count(w) == 1 for w in waits if w != PIECES * (S - 2)), (what, waits)
            # from the head of the steady loop to the end of the drain: the one vmcnt(0) is the drain's last step
            ring = [o for a, o in ops if lo <= a <= d_hi]
            assert [o for o in ring if "vmcnt(0)" in o] == ["s_waitcnt vmcnt(0)"], what
            assert all(re.fullmatch(r"s_waitcnt vmcnt\(\d+\)", o) for o in ring if "vmcnt" in o), what
            checked += 1
    assert checked == 6, checked
