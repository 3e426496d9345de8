"""CPU-only: the kernels behind fpq_fullrot_quant_rows* (csrc/fpq_fullrot.h) as the library's code objects have them, read as
tests/test_no_spill.py reads the hot kernels': no scratch, no spilled register, four wavefronts per SIMD, the LDS that lets four
workgroups share a CU, and both matrix-core instructions in every body."""
import os
import re
import subprocess

import pytest

from tests.test_no_spill import LIB, _code_objects, _tool, kernel_metadata


@pytest.mark.skipif(not os.path.exists(LIB), reason="libfpq_hip.so not built")
def test_fullrot_kernels_do_not_spill(tmp_path):
    recs = [(n, r) for n, r in kernel_metadata(tmp_path) if "fullrot_quant_kernel" in n]
    # {1920, 2304} x {fp16, fp32 rows} x {no smooth, smooth} x {values, values + rotated rows, codes}
    assert len(recs) == 24, [n for n, _ in recs]
    for n, r in recs:
        spill = int(r.get("vgpr_spill_count", 0)) + int(r.get("sgpr_spill_count", 0))
        assert spill == 0 and int(r.get("private_segment_fixed_size", 0)) == 0, (n, r)
        assert int(r["vgpr_count"]) + int(r.get("agpr_count", 0)) <= 128, (n, r["vgpr_count"])     # kFrWaves = 4 per SIMD
        assert int(r["group_segment_fixed_size"]) <= 160 * 1024 // 4, (n, r["group_segment_fixed_size"])   # ... and 4 workgroups per CU


@pytest.mark.skipif(not os.path.exists(LIB), reason="libfpq_hip.so not built")
def test_fullrot_kernels_run_both_factors_on_the_matrix_cores(tmp_path):
    seen = 0
    for elf in _code_objects(tmp_path):
        txt = subprocess.run([_tool("llvm-objdump"), "-d", elf], capture_output=True, text=True, check=True).stdout
        for m in re.finditer(r"<(\S*fullrot_quant_kernel\S*)>:\n(.*?)s_endpgm", txt, flags=re.S):
            body = m.group(2)
            assert "v_mfma_f32_16x16x32_f16" in body and "v_mfma_f32_16x16x32_bf16" in body, m.group(1)
            assert "scratch_" not in body, m.group(1)
            seen += 1
    assert seen == 24, seen
