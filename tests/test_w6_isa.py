"""CPU-only: the gfx950 code of every gemm_w6_kernel instantiation in libfpq_hip.so (fpq_gemm_g6.h: three activation formats x two
weight formats x two tilings), read from the library's code objects the way tests/test_gemm_ring_isa.py reads them: no spill, no
scratch, dynamic LDS only; every matrix instruction is the f8f6f4 MFMA with the instantiation's format selectors."""
import re
import subprocess

import pytest

from tests.test_gemm_ring_isa import LIB, MAGIC, _tool

KERNEL = "gemm_w6_kernel"


@pytest.fixture(scope="module")
def code_objects(tmp_path_factory):
    """[(disassembly lines, notes text)] of the gfx950 code objects that hold the kernel"""
    import __graft_entry__ as g
    g.build_hip()
    tools = {t: _tool(t) for t in ("llvm-objcopy", "clang-offload-bundler", "llvm-readelf", "llvm-objdump")}
    assert all(tools.values()), f"LLVM binutils of the ROCm toolchain not found: {tools}"
    tmp = tmp_path_factory.mktemp("w6_isa")
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
        dis = subprocess.run([tools["llvm-objdump"], "-d", "--no-show-raw-insn", elf], check=True, capture_output=True, text=True).stdout
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


def _template_args(name):
    """(MT, FA, FW) from the mangled name gemm_w6_kernel<float, MT, 4, FA, FW>"""
    m = re.search(KERNEL + r"IfLi(\d)ELi4ELi(\d)ELi(\d)E", name)
    assert m, name
    return int(m.group(1)), int(m.group(2)), int(m.group(3))


WANT = {(mt, fa, fw) for mt in (2, 4) for fa in (4, 2, 3) for fw in (2, 3)}


def test_the_twelve_instantiations_do_not_spill(code_objects):
    """{E2M1, E1M2, E3M0 activation} x {E1M2, E3M0 weight} x {64, 128 rows}, fp32 weight scales only: no scratch, no spill, at most
    256 registers per lane (two workgroups of four wavefronts per CU), no static LDS (the image is the launch's dynamic LDS)."""
    recs = [r for _, notes in code_objects for r in _records(notes)]
    assert len(recs) == 12, sorted(r["name"] for r in recs)
    assert {_template_args(r["name"]) for r in recs} == WANT
    for r in recs:
        what = r["name"][:120]
        assert int(r.get("vgpr_spill_count", 0)) == 0 and int(r.get("sgpr_spill_count", 0)) == 0, what
        assert int(r.get("private_segment_fixed_size", 0)) == 0, what
        assert int(r["vgpr_count"]) + int(r.get("agpr_count", 0)) <= 256, (what, r["vgpr_count"])
        assert int(r.get("group_segment_fixed_size", 0)) == 0, what


def test_fragment_reads_and_selectors(code_objects):
    """Per K step: three ds_read_b64 per 6-bit fragment (4 weight fragments, MT activation ones) or one ds_read_b128 per nibble
    fragment, beside the scale tiles' 1 + MT ds_read_b128; every MFMA is the f8f6f4 one, decodes A by the activation's selector and
    B by the weight's; no scratch access, no packed fp32 VALU, no vector-memory wait among the MFMAs (the LDS-DMA pieces are
    waited for once, in front of the barrier); two stages' worth of LDS-DMA pieces (the prologue's and the loop's)."""
    seen = set()
    for lines, _ in code_objects:
        txt = "\n".join(lines)
        for block in re.split(r"\n(?=[0-9a-fA-F]+ <)", txt):
            head = block.split("\n", 1)[0]
            if KERNEL not in head:
                continue
            body = [" ".join(l.split()).split(" //")[0] for l in block.splitlines()[1:] if l.strip()]
            ops = [l.split()[0] for l in body]
            mt, fa, fw = _template_args(head)
            a4 = fa == 4
            assert ops.count("ds_read_b64") == 3 * (4 + (0 if a4 else mt)), (head, ops.count("ds_read_b64"))
            assert ops.count("ds_read_b128") == 1 + mt + (mt if a4 else 0), (head, ops.count("ds_read_b128"))
            assert not [o for o in ops if o.startswith("ds_read2")], head
            assert not [o for o in ops if o.startswith("scratch_")], head
            assert not [o for o in ops if o.startswith("v_pk_") and o.endswith("_f32")], head      # FPQ_NOPK: scalar fp32 VALU
            mf = [i for i, l in enumerate(body) if l.startswith("v_mfma")]
            assert len(mf) == 4 * mt, (head, len(mf))
            for i in mf:
                assert "v_mfma_f32_16x16x128_f8f6f4" in body[i] and f"cbsz:{fa}" in body[i] and f"blgp:{fw}" in body[i], (head, body[i])
            between = [l for l in body[mf[0]:mf[-1] + 1] if l.startswith("s_waitcnt") and "vmcnt" in l]
            assert not between, (head, between)
            pieces = ((2 * mt * (64 if a4 else 96) * 16) // 1024 + 12 + 3) // 4      # per wavefront and stage (the last round may be short)
            assert ops.count("global_load_lds_dwordx4") == 2 * pieces, (head, ops.count("global_load_lds_dwordx4"))
            seen.add((mt, fa, fw))
    assert seen == WANT, seen
