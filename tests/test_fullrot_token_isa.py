"""CPU-only: the kernels behind fpq_fullrot_quant_token_rows* and fpq_fullrot_adaln_quant_token_rows* (csrc/fpq_fulltoken.h) as the
library's code objects have them, read as tests/test_fulladaln_isa.py reads fullrot_adaln_kernel's: their number, no scratch, no
spilled register, registers and LDS within the occupancy their launch bounds claim, and both matrix-core instructions in every body."""
import os
import re
import subprocess

import pytest

from tests.test_no_spill import LIB, _code_objects, _tool, kernel_metadata

# fulltok_quant_kernel: {1920, 2304} x {fp16, fp32 rows} x {no smooth, smooth} x {values, codes} = 16;
# fulltok_adaln_kernel: {1920, 2304} x {fp16, fp32 rows} x {fp16, fp32 modulation} x {values, codes} = 16 (smooth is a run-time select);
# the rotated rows, h and the row scales of the values forms are run-time pointers, the table and the layout of the code forms arguments
NAMES = {"fulltok_quant_kernel": 16, "fulltok_adaln_kernel": 16}
# fp32 rows of 2304 with fp32 modulation (mangled: <36, 64, float, float, MODE>): launch bounds of three wavefronts per SIMD, as the
# per-group producer's same form (csrc/fpq_fulladaln.h, kFaWaves)
THREE_WAVES = re.compile(r"fulltok_adaln_kernelILi36ELi64EffLi[01]E")


def _mine(name):
    return any(n in name for n in NAMES)


@pytest.mark.skipif(not os.path.exists(LIB), reason="libfpq_hip.so not built")
def test_fulltoken_kernels_do_not_spill(tmp_path):
    recs = [(n, r) for n, r in kernel_metadata(tmp_path) if _mine(n)]
    for name, count in NAMES.items():
        assert len([n for n, _ in recs if name in n]) == count, [n for n, _ in recs if name in n]
    # tests/test_fullrot_isa.py and tests/test_fulladaln_isa.py count their kernels by these substrings
    assert not [n for n, _ in recs if "fullrot_quant_kernel" in n or "fullrot_adaln_kernel" in n]
    three = [n for n, _ in recs if THREE_WAVES.search(n)]
    assert len(three) == 2, three
    for n, r in recs:
        waves = 3 if n in three else 4
        spill = int(r.get("vgpr_spill_count", 0)) + int(r.get("sgpr_spill_count", 0))
        assert spill == 0 and int(r.get("private_segment_fixed_size", 0)) == 0, (n, r)
        assert int(r["vgpr_count"]) + int(r.get("agpr_count", 0)) <= 512 // waves // 8 * 8, (n, r["vgpr_count"])   # 128; 168 at three
        assert int(r["group_segment_fixed_size"]) <= 160 * 1024 // waves, (n, r["group_segment_fixed_size"])   # as many workgroups per CU


@pytest.mark.skipif(not os.path.exists(LIB), reason="libfpq_hip.so not built")
def test_fulltoken_kernels_run_both_factors_on_the_matrix_cores(tmp_path):
    seen = 0
    for elf in _code_objects(tmp_path):
        txt = subprocess.run([_tool("llvm-objdump"), "-d", elf], capture_output=True, text=True, check=True).stdout
        for m in re.finditer(r"<(\S*fulltok_(?:quant|adaln)_kernel\S*)>:\n(.*?)s_endpgm", txt, flags=re.S):
            body = m.group(2)
            assert "v_mfma_f32_16x16x32_f16" in body and "v_mfma_f32_16x16x32_bf16" in body, m.group(1)
            seen += 1
    assert seen == sum(NAMES.values()), seen
