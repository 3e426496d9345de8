"""CPU-only: the RESID forms of adaln_mfma_kernel (fpqvar_amd/csrc/fpq_adaln.h, instantiated by fpq_resid_adaln.hip through the
dispatch it shares with fpq_adaln.hip) - read from the code objects' metadata notes the way tests/test_g6_isa.py reads its kernels':
every variant the unfused entry points can launch has its fused form, none spills, and each stays in the occupancy class of its twin."""
import re
import subprocess

import pytest

from tests.test_gemm_ring_isa import LIB, MAGIC, _tool

# the template parameters behind Tmod, in the order of the kernel's declaration
PARAMS = ("MAXC", "CODES", "EMIT", "TOKEN", "X32", "HW4", "TIGHT", "NW", "PAIR2", "HW6", "G6", "RESID")
LDS_PER_CU, LDS_GRANULE = 160 * 1024, 1280      # gfx950; the granule: profiles/r03_occupancy_census.txt
VGPRS_PER_SIMD, VGPR_GRANULE = 512, 8


@pytest.fixture(scope="module")
def kernels(tmp_path_factory):
    """{(Tmod, MAXC, ..., RESID): metadata record} of every adaln_mfma_kernel in libfpq_hip.so"""
    import __graft_entry__ as g
    g.build_hip()
    tools = {t: _tool(t) for t in ("llvm-objcopy", "clang-offload-bundler", "llvm-readelf")}
    assert all(tools.values()), f"LLVM binutils of the ROCm toolchain not found: {tools}"
    tmp = tmp_path_factory.mktemp("resid_adaln_isa")
    fat = str(tmp / "fatbin")
    subprocess.run([tools["llvm-objcopy"], "-O", "binary", "--only-section=.hip_fatbin", LIB, fat], check=True)
    data = open(fat, "rb").read()
    starts = [m.start() for m in re.finditer(re.escape(MAGIC), data)]
    assert starts, "no offload bundle in .hip_fatbin"
    out = {}
    for k, a in enumerate(starts):
        b = starts[k + 1] if k + 1 < len(starts) else len(data)
        bundle, elf = str(tmp / f"bundle{k}"), str(tmp / f"co{k}.elf")
        open(bundle, "wb").write(data[a:b])
        subprocess.run([tools["clang-offload-bundler"], "--unbundle", "--type=o", "--targets=hipv4-amdgcn-amd-amdhsa--gfx950",
                        f"--input={bundle}", f"--output={elf}"], check=True)
        txt = subprocess.run([tools["llvm-readelf"], "--notes", elf], check=True, capture_output=True, text=True).stdout
        if "adaln_mfma_kernel" not in txt:
            continue
        for r in _records(txt):
            key = _key(r["name"])
            assert key not in out, f"{r['name']} twice"
            out[key] = r
    assert out, "no code object holds adaln_mfma_kernel"
    return out


def _key(name):
    m = re.search(r"adaln_mfma_kernelI(DF16_|Dh|f)((?:L[ib]\d+E)+)E", name)
    assert m, name
    vals = tuple(int(v) for v in re.findall(r"L[ib](\d+)E", m.group(2)))
    assert len(vals) == len(PARAMS), name
    return ("f16" if m.group(1) != "f" else "f32",) + vals


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
    return [r for r in recs if "adaln_mfma_kernel" in r.get("name", "")]


def _regs(r):
    return int(r["vgpr_count"]) + int(r.get("agpr_count", 0))


def _lds(r):
    return int(r.get("group_segment_fixed_size", 0))


def _min_workgroups(key):
    """the kernel's __launch_bounds__(256, n): n workgroups of four wavefronts per CU = n wavefronts per SIMD"""
    if _param(key, "EMIT") or (_param(key, "X32") and _param(key, "MAXC") == 5):
        return 3
    return 5 if _param(key, "TIGHT") else 4


def _workgroups_per_cu(key, r):
    """what registers and LDS allow, counted up to the kernel's own bound: the occupancy class"""
    by_regs = VGPRS_PER_SIMD // (-(-_regs(r) // VGPR_GRANULE) * VGPR_GRANULE)
    by_lds = LDS_PER_CU // (-(-_lds(r) // LDS_GRANULE) * LDS_GRANULE)
    return min(by_regs, by_lds, _min_workgroups(key))


def _param(key, name):
    return key[1 + PARAMS.index(name)]


def test_every_twin_variant_has_its_fused_form(kernels):
    """the fused entry points share the twins' dispatch: whatever form it can pick for a twin - TIGHT, PAIR2, the hardware levels,
    MAXC 1 .. 5, each modulation and row dtype - exists with RESID, and nothing else does (the 6-bit group forms have no fused twin)"""
    twins = {k[:-1] for k in kernels if not _param(k, "RESID") and not _param(k, "G6")}
    fused = {k[:-1] for k in kernels if _param(k, "RESID")}
    assert len(twins) >= 200 and fused == twins, (sorted(twins - fused), sorted(fused - twins))
    for name, want in (("TIGHT", 1), ("PAIR2", 1), ("HW4", 1), ("HW6", 1), ("HW6", 2), ("TOKEN", 1), ("EMIT", 1), ("CODES", 1), ("X32", 1)):
        assert any(_param(k, name) == want for k in fused), name
    assert {_param(k, "MAXC") for k in fused} == {1, 2, 3, 4, 5}
    assert not any(_param(k, "G6") for k in kernels if _param(k, "RESID"))


def test_no_scratch_no_spill_and_the_twins_occupancy_class(kernels):
    for key, r in kernels.items():
        if not _param(key, "RESID"):
            continue
        what = r["name"][:140]
        assert int(r.get("vgpr_spill_count", 0)) == 0 and int(r.get("sgpr_spill_count", 0)) == 0, what
        assert int(r.get("private_segment_fixed_size", 0)) == 0, what
        twin = kernels[key[:-1] + (0,)]
        assert _lds(r) == _lds(twin), (what, _lds(r), _lds(twin))            # y and the gate live in registers: no third plane
        assert _workgroups_per_cu(key, r) == _workgroups_per_cu(key, twin) == _min_workgroups(key), (what, _regs(r), _regs(twin), _lds(r))
        if _param(key, "TIGHT"):                                                 # five workgroups per CU (fpq_adaln.h)
            assert _regs(r) <= 96 and _lds(r) <= 32768, (what, _regs(r), _lds(r))
            assert _workgroups_per_cu(key, r) == 5
