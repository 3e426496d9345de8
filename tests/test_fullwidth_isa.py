"""CPU-only: the full-width producers (csrc/fpq_fullrot.h: fullrot_rows_kernel<Front, Tail>) as the library's code objects have them,
read as tests/test_no_spill.py reads the hot kernels'.  Per (front, tail) family: the number of kernels, no scratch, no spilled
register, registers and LDS within the occupancy the launch bounds claim, and both matrix-core instructions in every body."""
import functools
import os
import pathlib
import re
import subprocess
import tempfile

import pytest

from tests.test_no_spill import LIB, _code_objects, _tool, kernel_metadata

KERNEL = "fullrot_rows_kernel"
# family -> (front and tail as the mangled names carry them, kernels, kernels with launch bounds of three wavefronts per SIMD)
# FrPlainFront: {1920, 2304} x {fp16, fp32 rows} x {no smooth, smooth}; FrAdalnFront: {1920, 2304} x {fp16, fp32 rows} x {fp16, fp32
# modulation}, smooth is a run-time select.  Per-group tail (FrTail<false, ..>) x {values, values + intermediates, codes}; per-token
# tail (FrTail<true, ..>) x {values, codes}: its intermediates and row scales are run-time pointers
FAMILIES = {"plain_group": ("12FrPlainFrontI", "6FrTailILb0E", 24, 0),
            "adaln_group": ("12FrAdalnFrontI", "6FrTailILb0E", 24, 3),
            "plain_token": ("12FrPlainFrontI", "6FrTailILb1E", 16, 0),
            "adaln_token": ("12FrAdalnFrontI", "6FrTailILb1E", 16, 2)}
# fp32 rows of 2304 with fp32 modulation (mangled: FrAdalnFront<36, 64, float, float, EMIT>): csrc/fpq_fulladaln.h, kFaWaves
THREE_WAVES = re.compile(r"12FrAdalnFrontILi36ELi64EffLb[01]EE")

pytestmark = pytest.mark.skipif(not os.path.exists(LIB), reason="libfpq_hip.so not built")


def _family(name):
    """The families a mangled kernel name belongs to"""
    return [f for f, (front, tail, _, _) in FAMILIES.items() if KERNEL in name and front in name and tail in name]


@functools.lru_cache(maxsize=None)
def _library():
    """([(mangled name, metadata record)], {mangled name: disassembled body}) of the kernels of KERNEL, read once"""
    with tempfile.TemporaryDirectory() as tmp:
        recs = [(n, r) for n, r in kernel_metadata(pathlib.Path(tmp)) if KERNEL in n]
        bodies = {}
        for elf in _code_objects(pathlib.Path(tmp)):
            txt = subprocess.run([_tool("llvm-objdump"), "-d", elf], capture_output=True, text=True, check=True).stdout
            for m in re.finditer(r"<(\S*" + KERNEL + r"\S*)>:\n(.*?)s_endpgm", txt, flags=re.S):
                bodies[m.group(1)] = m.group(2)
    return recs, bodies


def test_every_fullwidth_kernel_is_of_one_family():
    recs, bodies = _library()
    assert len(recs) == sum(count for _, _, count, _ in FAMILIES.values()), [n for n, _ in recs]
    assert all(len(_family(n)) == 1 for n, _ in recs), [n for n, _ in recs if len(_family(n)) != 1]
    assert sorted(bodies) == sorted(n for n, _ in recs)


@pytest.mark.parametrize("family", FAMILIES)
def test_fullwidth_kernels_do_not_spill(family):
    _, _, count, n_three = FAMILIES[family]
    recs = [(n, r) for n, r in _library()[0] if _family(n) == [family]]
    assert len(recs) == count, [n for n, _ in recs]
    three = [n for n, _ in recs if THREE_WAVES.search(n)]
    assert len(three) == n_three, three
    for n, r in recs:
        waves = 3 if n in three else 4
        spill = int(r.get("vgpr_spill_count", 0)) + int(r.get("sgpr_spill_count", 0))
        assert spill == 0 and int(r.get("private_segment_fixed_size", 0)) == 0, (n, r)
        assert int(r["vgpr_count"]) + int(r.get("agpr_count", 0)) <= 512 // waves // 8 * 8, (n, r["vgpr_count"])   # 128; 168 at three
        assert int(r["group_segment_fixed_size"]) <= 160 * 1024 // waves, (n, r["group_segment_fixed_size"])   # as many workgroups per CU


@pytest.mark.parametrize("family", FAMILIES)
def test_fullwidth_kernels_run_both_factors_on_the_matrix_cores(family):
    seen = 0
    for name, body in _library()[1].items():
        if _family(name) != [family]:
            continue
        assert "v_mfma_f32_16x16x32_f16" in body and "v_mfma_f32_16x16x32_bf16" in body, name
        assert "scratch_" not in body, name
        seen += 1
    assert seen == FAMILIES[family][2], seen
