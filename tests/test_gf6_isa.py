"""CPU-only: the resource usage of the fc1 kernels whose tail keeps a NaN out of the maxima (fpq_gemm_fp4.h FPQ_GEMM_FC1_TAIL_X; the
kernels behind fpq_gemm_a6w4_gelu_dual_pair / fpq_gemm_w6_gelu_dual_pair with the INT- / E2M3+ pair) - gemm_a6w4_fc1x_kernel,
gemm_a6w4_fc1x_km_kernel, gemm_w6_fc1x_kernel, gemm_w6_fc1x_km_kernel - read from the library's code objects the way
tests/test_w6_forms_isa.py reads theirs.  Registers, scratch, spills and static LDS - nothing else."""
import re
import subprocess

import pytest

from tests.test_gemm_ring_isa import LIB, MAGIC, _tool

KERNELS = ("gemm_a6w4_fc1x_kernel", "gemm_a6w4_fc1x_km_kernel", "gemm_w6_fc1x_kernel", "gemm_w6_fc1x_km_kernel")
# row-major A6W4: fp16 and fp32 weight scales x two tilings x two activation formats; its images and the W6 family: fp32 only
WANT = {"gemm_a6w4_fc1x_kernel": 8, "gemm_a6w4_fc1x_km_kernel": 4, "gemm_w6_fc1x_kernel": 12, "gemm_w6_fc1x_km_kernel": 12}


@pytest.fixture(scope="module")
def notes(tmp_path_factory):
    """the metadata notes of the gfx950 code objects that hold one of the kernels"""
    import __graft_entry__ as g
    g.build_hip()
    tools = {t: _tool(t) for t in ("llvm-objcopy", "clang-offload-bundler", "llvm-readelf")}
    assert all(tools.values()), f"LLVM binutils of the ROCm toolchain not found: {tools}"
    tmp = tmp_path_factory.mktemp("gf6_isa")
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
        txt = subprocess.run([tools["llvm-readelf"], "--notes", elf], check=True, capture_output=True, text=True).stdout
        if any(k_ in txt for k_ in KERNELS):
            out.append(txt)
    assert out, f"no code object holds any of {KERNELS}"
    return out


def _kernel(name):
    m = re.search(r"(gemm_(?:a6w4|w6)_fc1x(?:_km)?_kernel)I", name)
    return m.group(1) if m else None


def _records(text):
    recs, cur = [], None
    for line in text.splitlines():
        m = re.match(r"\s*-?\s*\.(\w+):\s*(.*)$", line)
        if not m:
            continue
        key, val = m.group(1), m.group(2).strip().strip("'\"")
        if key == "agpr_count" and (cur is None or "agpr_count" in cur):   # first key of a kernel's record
            cur = {}
            recs.append(cur)
        if cur is not None:
            cur[key] = val
    return [r for r in recs if _kernel(r.get("name", ""))]


def test_the_instantiations_are_there_and_do_not_spill(notes):
    """no scratch, no spill, at most 256 registers per lane (__launch_bounds__(256, 2)), no static LDS (the image, the dual pair's
    bucket table included, is the launch's dynamic LDS)"""
    recs = [r for text in notes for r in _records(text)]
    count = {}
    for r in recs:
        count[_kernel(r["name"])] = count.get(_kernel(r["name"]), 0) + 1
    assert count == WANT, count
    for r in recs:
        what = r["name"][:120]
        print(what, "vgpr", r["vgpr_count"], "agpr", r.get("agpr_count", 0))
        assert int(r.get("vgpr_spill_count", 0)) == 0 and int(r.get("sgpr_spill_count", 0)) == 0, what
        assert int(r.get("private_segment_fixed_size", 0)) == 0, what
        assert int(r["vgpr_count"]) + int(r.get("agpr_count", 0)) <= 256, (what, r["vgpr_count"])
        assert int(r.get("group_segment_fixed_size", 0)) == 0, what
