"""CPU-only: the kernels of the GEMMs' squared-error forms (fpq_gemm_fp4.h, GemmSqErr) in libfpq_hip.so, from the code objects'
metadata notes as tests/test_g6_isa.py reads them: every instantiation the launchers can choose is there exactly once, none
spills, uses scratch or static LDS (the cross-wavefront exchange lives in an idle stage buffer of the launch's dynamic LDS), and
each keeps the workgroups-per-CU class of its plain twin - the register count must not cost the GEMM a resident workgroup."""
import re

import pytest

from tests.test_gemm_ring_isa import _tool
from tests.test_no_spill import kernel_metadata

SQ, PLAIN_XE = "NS_9GemmSqErrE", "NS_9GemmNoFc1E"
F16, F32 = "DF16_", "f"


def _want():
    """{mangled kernel name + template arguments: the same of the plain twin}"""
    want = {}
    for tw in (F16, F32):
        for mt in (2, 4, 8):       # FPQ_GEMM_CFG 30 / 20 / 10; never the ring
            want[f"20gemm_fp4_glds_kernelI{tw}Li{mt}ELi4E{SQ}E"] = f"20gemm_fp4_glds_kernelI{tw}Li{mt}ELi4E{PLAIN_XE}E"
        for mt in (2, 4):
            for fa in (2, 3):      # E1M2 / E3M0 activations against E2M1 nibbles, fp16 or fp32 weight scales
                want[f"22gemm_a6w4_sqerr_kernelI{tw}Li{mt}ELi4ELi{fa}EE"] = f"16gemm_a6w4_kernelI{tw}Li{mt}ELi4ELi{fa}EE"
    for mt in (2, 4):
        for fa in (4, 2, 3):
            for fw in (2, 3):      # fp32 weight scales only
                want[f"20gemm_w6_sqerr_kernelIfLi{mt}ELi4ELi{fa}ELi{fw}EE"] = f"14gemm_w6_kernelIfLi{mt}ELi4ELi{fa}ELi{fw}EE"
    for mt in (4, 8):              # FPQ_GEMM6_CFG 0 / 1
        for fa in (2, 3):
            for fb in (2, 3):
                for ta in (F16, F32):
                    if ta == F32 and (fa, fb) != (2, 2):
                        continue   # a pair with an E3M2 side: fp16 activation scales only
                    for tw in (F16, F32):
                        twin = (f"20gemm_fp6_rows_kernelI{ta}{tw}Li{mt}ELi4E{PLAIN_XE}E" if (fa, fb) == (2, 2) else
                                f"24gemm_fp6_rows_bf6_kernelI{ta}{tw}Li{mt}ELi4E{PLAIN_XE}Li{fa}ELi{fb}EE")
                        want[f"25gemm_f6_rows_sqerr_kernelI{ta}{tw}Li{mt}ELi4E{SQ}Li{fa}ELi{fb}EE"] = twin
    return want


@pytest.fixture(scope="module")
def records(tmp_path_factory):
    import __graft_entry__ as g
    g.build_hip()
    assert all(_tool(t) for t in ("llvm-objcopy", "clang-offload-bundler", "llvm-readelf")), "LLVM binutils of the ROCm toolchain not found"
    return kernel_metadata(tmp_path_factory.mktemp("gemm_sqerr_isa"))


def _key(name):
    """the kernel's name and template arguments out of a mangled symbol: between the anonymous namespace and the parameter list"""
    m = re.match(r"_ZN12_GLOBAL__N_1(\d+gemm_\w+?_kernelI.+?E)EvPKh", name)
    return m.group(1) if m else None


def _wg_per_cu(rec):
    """resident workgroups per CU by registers: four wavefronts, one per SIMD, 512 registers per lane and SIMD in granules of 8"""
    regs = int(rec["vgpr_count"]) + int(rec.get("agpr_count", 0))
    return 512 // ((regs + 7) // 8 * 8)


def test_every_instantiation_once_within_its_resources_and_its_twins_class(records):
    want = _want()
    assert len(want) == 6 + 8 + 12 + 20
    by_key = {}
    for name, rec in records:
        k = _key(name)
        if k is not None:
            assert k not in by_key, f"{k} twice"
            by_key[k] = rec
    mine = {k for k in by_key if "sqerr" in k or SQ in k}
    assert mine == set(want), (sorted(mine - set(want)), sorted(set(want) - mine))
    assert not any("gemm_fp4_ring_kernel" in k and SQ in k for k in by_key), "the ring kernel has no squared-error form"
    for k, twin in want.items():
        rec = by_key[k]
        assert twin in by_key, f"plain twin {twin} of {k} not found"
        assert int(rec.get("vgpr_spill_count", 0)) == 0 and int(rec.get("sgpr_spill_count", 0)) == 0, k
        assert int(rec.get("private_segment_fixed_size", 0)) == 0, k
        assert int(rec.get("group_segment_fixed_size", 0)) == 0, k
        assert int(rec["vgpr_count"]) + int(rec.get("agpr_count", 0)) <= 256, (k, rec["vgpr_count"])
        assert _wg_per_cu(rec) == _wg_per_cu(by_key[twin]), (k, rec["vgpr_count"], twin, by_key[twin]["vgpr_count"])
