"""CPU-only: every kernel compiled from the one text of the per-group GEMMs with a 6-bit side (fpqvar_amd/csrc/fpq_gemm_g6_kernel.h,
instantiated by fpq_gemm_g6.h / launch_g6 in fpq_gemm_g6.hip) is in libfpq_hip.so, as often as the launcher can choose it, and
within its resources - read from the code objects' metadata notes the way tests/test_gf6_isa.py reads its four kernels'.
The names: the A6W4 family's ten (templates over <Tsw, MT, NT, FA>) and the W6 family's ten (<Tsw, MT, NT, FA, FW>)."""
import re
import subprocess

import pytest

from tests.test_gemm_ring_isa import LIB, MAGIC, _tool

FORMS = ("", "fc1_", "fc1x_", "split_", "qkn_")
# A6W4: two activation formats x two tilings; fp16 and fp32 weight scales on the row-major plain, fc1 and fc1x kernels, fp32 only on
# the split forms and on every k-major kernel
A6W4 = {"gemm_a6w4_kernel": 8, "gemm_a6w4_fc1_kernel": 8, "gemm_a6w4_fc1x_kernel": 8, "gemm_a6w4_split_kernel": 4, "gemm_a6w4_qkn_kernel": 4,
        **{f"gemm_a6w4_{f}km_kernel": 4 for f in FORMS}}
# W6: three activation formats x two weight formats x two tilings, fp32 weight scales
W6 = {f"gemm_w6_{f}{km}kernel": 12 for f in FORMS for km in ("", "km_")}
WANT = {**A6W4, **W6}


@pytest.fixture(scope="module")
def notes(tmp_path_factory):
    """the metadata notes of the gfx950 code objects that hold one of the kernels"""
    import __graft_entry__ as g
    g.build_hip()
    tools = {t: _tool(t) for t in ("llvm-objcopy", "clang-offload-bundler", "llvm-readelf")}
    assert all(tools.values()), f"LLVM binutils of the ROCm toolchain not found: {tools}"
    tmp = tmp_path_factory.mktemp("g6_isa")
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
        if any(k_ in txt for k_ in WANT):
            out.append(txt)
    assert out, "no code object holds any of the kernels"
    return out


def _kernel(name):
    m = re.search(r"(gemm_(?:a6w4|w6)_(?:fc1_|fc1x_|split_|qkn_)?(?:km_)?kernel)I", name)
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


def test_every_instantiation_is_there_and_does_not_spill(notes):
    """52 A6W4 and 120 W6 kernels - no name more or less often than launch_g6 can choose it; no scratch, no spill, at most 256
    registers per lane (__launch_bounds__(256, 2)), no static LDS (the image is the launch's dynamic LDS)"""
    assert len(WANT) == 20 and sum(A6W4.values()) == 52 and sum(W6.values()) == 120
    recs = [r for text in notes for r in _records(text)]
    count = {}
    for r in recs:
        count[_kernel(r["name"])] = count.get(_kernel(r["name"]), 0) + 1
    assert count == WANT, count
    assert len({r["name"] for r in recs}) == len(recs) == 172
    for r in recs:
        what = r["name"][:120]
        assert int(r.get("vgpr_spill_count", 0)) == 0 and int(r.get("sgpr_spill_count", 0)) == 0, what
        assert int(r.get("private_segment_fixed_size", 0)) == 0, what
        assert int(r["vgpr_count"]) + int(r.get("agpr_count", 0)) <= 256, (what, r["vgpr_count"])
        assert int(r.get("group_segment_fixed_size", 0)) == 0, what
