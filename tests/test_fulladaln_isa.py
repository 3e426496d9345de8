"""CPU-only: the kernels behind fpq_fullrot_adaln_quant_rows* (csrc/fpq_fulladaln.h) as the library's code objects have them, read
as tests/test_fullrot_isa.py reads fullrot_quant_kernel's: their number, no scratch, no spilled register, registers and LDS within
the occupancy their launch bounds claim, and both matrix-core instructions in every body."""
import os
import re
import subprocess

import pytest

from tests.test_no_spill import LIB, _code_objects, _tool, kernel_metadata

NAME = "fullrot_adaln_kernel"
# {1920, 2304} x {fp16, fp32 rows} x {fp16, fp32 modulation} x {values, values + h / rotated rows, codes}; smooth is a run-time select
KERNELS = 24
# fp32 rows of 2304 with fp32 modulation (mangled: <36, 64, float, float, MODE>): launch bounds of three wavefronts per SIMD
THREE_WAVES = re.compile(r"fullrot_adaln_kernelILi36ELi64EffLi[012]E")


@pytest.mark.skipif(not os.path.exists(LIB), reason="libfpq_hip.so not built")
def test_fulladaln_kernels_do_not_spill(tmp_path):
    recs = [(n, r) for n, r in kernel_metadata(tmp_path) if NAME in n]
    assert len(recs) == KERNELS, [n for n, _ in recs]
    assert not [n for n, _ in recs if "fullrot_quant_kernel" in n]          # tests/test_fullrot_isa.py counts those by name
    three = [n for n, _ in recs if THREE_WAVES.search(n)]
    assert len(three) == 3, three
    for n, r in recs:
        waves = 3 if n in three else 4
        spill = int(r.get("vgpr_spill_count", 0)) + int(r.get("sgpr_spill_count", 0))
        assert spill == 0 and int(r.get("private_segment_fixed_size", 0)) == 0, (n, r)
        assert int(r["vgpr_count"]) + int(r.get("agpr_count", 0)) <= 512 // waves // 8 * 8, (n, r["vgpr_count"])   # 128; 168 at three
        assert int(r["group_segment_fixed_size"]) <= 160 * 1024 // waves, (n, r["group_segment_fixed_size"])   # as many workgroups per CU


@pytest.mark.skipif(not os.path.exists(LIB), reason="libfpq_hip.so not built")
def test_fulladaln_kernels_run_both_factors_on_the_matrix_cores(tmp_path):
    seen = 0
    for elf in _code_objects(tmp_path):
        txt = subprocess.run([_tool("llvm-objdump"), "-d", elf], capture_output=True, text=True, check=True).stdout
        for m in re.finditer(r"<(\S*" + NAME + r"\S*)>:\n(.*?)s_endpgm", txt, flags=re.S):
            body = m.group(2)
            assert "v_mfma_f32_16x16x32_f16" in body and "v_mfma_f32_16x16x32_bf16" in body, m.group(1)
            seen += 1
    assert seen == KERNELS, seen
