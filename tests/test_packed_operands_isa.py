"""CPU-only: the kernels behind fpq_packed_to_operands / fpq_operands_to_packed (csrc/fpq_packed_operands.h) keep their code maps in
registers - no spills, no scratch, no LDS (there is no table in memory) - read from the library's code objects as
tests/test_no_spill.py reads the hot kernels'."""
import os

import pytest

from tests.test_no_spill import LIB, kernel_metadata


@pytest.mark.skipif(not os.path.exists(LIB), reason="libfpq_hip.so not built")
def test_packed_operand_kernels_do_not_spill(tmp_path):
    recs = [(n, r) for n, r in kernel_metadata(tmp_path) if "packed_to_operands_kernel" in n or "operands_to_packed_kernel" in n]
    # forward: three unit shapes x {fp16, fp32} file scales; inverse: three unit shapes
    assert len(recs) == 9, [n for n, _ in recs]
    for n, r in recs:
        spill = int(r.get("vgpr_spill_count", 0)) + int(r.get("sgpr_spill_count", 0))
        assert spill == 0 and int(r.get("private_segment_fixed_size", 0)) == 0 and int(r.get("group_segment_fixed_size", 0)) == 0, (n, r)
        assert int(r["vgpr_count"]) <= 64, (n, r["vgpr_count"])     # eight wavefronts per SIMD: a streaming kernel hides HBM with occupancy
