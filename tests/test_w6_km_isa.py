"""CPU-only: the gfx950 code of every gemm_w6_km_kernel, gemm_w6_fc1_km_kernel, gemm_w6_split_km_kernel and gemm_w6_qkn_km_kernel
instantiation in libfpq_hip.so (fpq_gemm_g6.h: the W6 GEMM's four forms on k-major images - three activation formats x two weight
formats x two tilings each), read from the library's code objects the way tests/test_w6_forms_isa.py reads the row-major forms'.
All 48 fit: none is routed to the smaller tiling.  The test is about registers, LDS and the matrix instruction - nothing else."""
import re
import subprocess

import pytest

from tests.test_gemm_ring_isa import LIB, MAGIC, _tool

KERNELS = ("gemm_w6_km_kernel", "gemm_w6_fc1_km_kernel", "gemm_w6_split_km_kernel", "gemm_w6_qkn_km_kernel")
WANT = {(k, mt, fa, fw) for k in KERNELS for mt in (2, 4) for fa in (4, 2, 3) for fw in (2, 3)}


@pytest.fixture(scope="module")
def code_objects(tmp_path_factory):
    """[(disassembly lines, notes text)] of the gfx950 code objects that hold one of the kernels"""
    import __graft_entry__ as g
    g.build_hip()
    tools = {t: _tool(t) for t in ("llvm-objcopy", "clang-offload-bundler", "llvm-readelf", "llvm-objdump")}
    assert all(tools.values()), f"LLVM binutils of the ROCm toolchain not found: {tools}"
    tmp = tmp_path_factory.mktemp("w6_km_isa")
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
        if not any(k_ in notes for k_ in KERNELS):
            continue
        dis = subprocess.run([tools["llvm-objdump"], "-d", "--no-show-raw-insn", elf], check=True, capture_output=True, text=True).stdout
        out.append((dis.splitlines(), notes))
    assert out, f"no code object holds any of {KERNELS}"
    return out


def _template_args(name):
    """(kernel, MT, FA, FW) from the mangled name <kernel><float, MT, 4, FA, FW>, or None for another kernel"""
    m = re.search(r"(gemm_w6_(?:fc1_|split_|qkn_)?km_kernel)IfLi(\d)ELi4ELi(\d)ELi(\d)E", name)
    return (m.group(1), int(m.group(2)), int(m.group(3)), int(m.group(4))) if m else None


def _records(notes):
    """[{key: value}] of the four kernels' instantiations in a code object's metadata note"""
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
    return [r for r in recs if _template_args(r.get("name", ""))]


def test_the_48_instantiations_are_there_and_do_not_spill(code_objects):
    """{plain, fc1, split, qkn} x {E2M1, E1M2, E3M0 activation} x {E1M2, E3M0 weight} x {64, 128 rows}, fp32 weight scales only: no
    scratch, no spill, at most 256 registers per lane (__launch_bounds__(256, 2)), no static LDS (the image is the launch's dynamic
    LDS)"""
    recs = [r for _, notes in code_objects for r in _records(notes)]
    assert len(recs) == 48, sorted(r["name"] for r in recs)
    assert {_template_args(r["name"]) for r in recs} == WANT
    for r in recs:
        what = r["name"][:120]
        assert int(r.get("vgpr_spill_count", 0)) == 0 and int(r.get("sgpr_spill_count", 0)) == 0, what
        assert int(r.get("private_segment_fixed_size", 0)) == 0, what
        assert int(r["vgpr_count"]) + int(r.get("agpr_count", 0)) <= 256, (what, r["vgpr_count"])
        assert int(r.get("group_segment_fixed_size", 0)) == 0, what


def test_matrix_instructions_and_the_main_loop(code_objects):
    """every matrix instruction is the f8f6f4 MFMA, decoding A by the activation's selector and B by the weight's - 4 MT of them, the
    row-major kernels' main loop; no vector-memory wait between the first and the last (the LDS-DMA pieces, the scale tiles' among
    them, are waited for once, in front of the barrier)"""
    seen = set()
    for lines, _ in code_objects:
        txt = "\n".join(lines)
        for block in re.split(r"\n(?=[0-9a-fA-F]+ <)", txt):
            head = block.split("\n", 1)[0]
            args = _template_args(head)
            if not args:
                continue
            _, mt, fa, fw = args
            body = [" ".join(l.split()).split(" //")[0] for l in block.splitlines()[1:] if l.strip()]
            mf = [i for i, l in enumerate(body) if l.startswith("v_mfma")]
            assert len(mf) == 4 * mt, (head, len(mf))
            for i in mf:
                assert "v_mfma_f32_16x16x128_f8f6f4" in body[i] and f"cbsz:{fa}" in body[i] and f"blgp:{fw}" in body[i], (head, body[i])
            between = [l for l in body[mf[0]:mf[-1] + 1] if l.startswith("s_waitcnt") and "vmcnt" in l]
            assert not between, (head, between)
            seen.add(args)
    assert seen == WANT, WANT - seen
