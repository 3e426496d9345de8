"""CPU: the error model of fpq_sqerr_rows_weighted (tests/sqerr_model.py).  The emulation of the shipped order of operations is
within the derived bound on every finite family, each deliberate mistake exceeds it on at least one, the non-finite families
give the class the fp32 expression gives, and the bound meets the condition the format search needs of it.

Worst err / bound of the unmutated emulation over the cases below: 0.064 (weights, fp32 [65 x 1024]); exactly 0 on `equal`."""
import math

import pytest
import torch

from tests import sqerr_model as sm

F16, F32 = torch.float16, torch.float32
# small, one workgroup partly filled (51 and 102 vectors); several workgroups; a lane that iterates twice (n_it = 2)
SHAPES = ((1, 8), (3, 136), (65, 1024), (1100, 3840))
PLANES = 3


def _worst(rows, cols, dtype, family, mistake=None):
    ref, y, w = sm.make_case(family, rows, cols, dtype, PLANES)
    want = sm.reference(ref, y, w)
    assert bool((w > 0).all()) and bool(torch.isfinite(w).all())
    got = sm.emulate(ref, y, w, mistake)
    rel, floor = sm.bound(rows, cols, dtype, float(w.max()))
    return max(sm.ratio(float(got[p]), float(want[p]), rel, floor) for p in range(PLANES))


@pytest.mark.parametrize("dtype", (F16, F32), ids=("f16", "f32"))
@pytest.mark.parametrize("rows,cols", SHAPES, ids=lambda v: str(v))
def test_emulation_of_the_shipped_order_is_within_the_bound(rows, cols, dtype):
    for family in sm.FINITE_FAMILIES:
        worst = _worst(rows, cols, dtype, family)
        print(f"[{rows} x {cols}] {dtype} {family}: worst err / bound {worst:.3g}")
        assert worst <= 1.0, (family, worst)
    ref, y, w = sm.make_case("equal", rows, cols, dtype, PLANES)
    assert not bool(sm.emulate(ref, y, w).any()), "y == ref must give exactly 0"


# where each mistake must show: (family, rows, cols, dtype)
CAUGHT_ON = {
    "diff_fp16": [("fp16_max", 3, 136, F16), ("gauss", 3, 136, F32)],
    "square_acc_fp16": [("fp16_max", 3, 136, F16), ("gauss", 65, 1024, F16)],
    "neighbour_weight": [("weights", 65, 1024, F16)],
    "weight_plane0_only": [("gauss", 3, 136, F16), ("weights", 65, 1024, F32)],
    "drop_last_block": [("gauss", 3, 136, F16), ("weights", 3, 136, F32)],
    "planes_swapped": [("gauss", 65, 1024, F16)],
    "ref_plane_offset": [("gauss", 65, 1024, F16)],
}


@pytest.mark.parametrize("mistake", sm.MISTAKES)
def test_each_mistake_exceeds_the_bound(mistake):
    assert set(CAUGHT_ON) == set(sm.MISTAKES)
    for family, rows, cols, dtype in CAUGHT_ON[mistake]:
        worst = _worst(rows, cols, dtype, family, mistake)
        print(f"{mistake} on {family} [{rows} x {cols}] {dtype}: err / bound {worst:.3g}")
        assert worst > 1.0, (mistake, family, worst)


@pytest.mark.parametrize("dtype", (F16, F32), ids=("f16", "f32"))
def test_non_finite_families_give_the_fp32_class(dtype):
    for family in sm.NONFINITE_FAMILIES:
        ref, y, w = sm.make_case(family, 65, 1024, dtype, PLANES)
        want = sm.expected_class(ref, y)
        got = [sm.class_of(float(v)) for v in sm.emulate(ref, y, w)]
        ref64 = [sm.class_of(float(v)) for v in sm.reference(ref, y, w)]
        assert got == want == ref64, (family, got, want, ref64)
    # plane by plane: a NaN in plane 1 leaves planes 0 and 2 finite; inf - inf is NaN where both are +inf, +inf elsewhere
    assert sm.expected_class(*sm.make_case("nan_y", 65, 1024, dtype, PLANES)[:2]) == ["finite", "nan", "finite"]
    assert sm.expected_class(*sm.make_case("inf_both", 65, 1024, dtype, PLANES)[:2]) == ["inf", "nan", "inf"]
    assert sm.expected_class(*sm.make_case("nan_ref", 65, 1024, dtype, PLANES)[:2]) == ["nan"] * 3


def test_chain_and_the_config4_condition():
    """D and c as the kernel's source states them, and the condition the search needs: at config-4 size the reduction order moves
    a loss by less than 1e-4 relative, a twentieth of the 2e-3 the batched and the sample-by-sample forms must agree to."""
    assert sm.deal(13600, 5760, F16) == (13600 * 5760 // 8, 2048, 19)
    assert sm.chain(13600, 5760, F16) == (8 + 19 + 26, 3)
    assert sm.chain(13600, 5760, F32) == (4 + 38 + 26, 3)
    assert sm.deal(20, 5760, F16)[1] == 57 and sm.deal(70001, 8, F16)[1] == 274 and sm.deal(13600, 640, F16)[1] == 2048
    for dtype in (F16, F32):
        rel, _ = sm.bound(13600, 5760, dtype)
        assert rel < 1e-4, rel
    assert math.isclose(sm.bound(13600, 5760, F16)[0], 56 * sm.U, rel_tol=1e-5)
    assert sm.bound(3, 136, F16)[1] == 0.0 and sm.bound(3, 136, F32)[1] > 0.0


def test_header_states_the_same_bound():
    import os
    import re
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    hdr = open(os.path.join(root, "include", "fpq.h")).read()
    assert "D = V + n_it + 26,  c = 3" in hdr
    assert int(re.search(r"#define FPQ_SQERR_WORKSPACE_BYTES (\d+)", hdr).group(1)) == 16 * sm.MAX_BLOCKS
    src = open(os.path.join(root, "fpqvar_amd", "csrc", "fpq_kernels.hip")).read()
    assert "D = V + n_it + 26" in src and "c = 3 roundings" in src
