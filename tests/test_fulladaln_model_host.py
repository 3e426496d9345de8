"""CPU checks of tests/fulladaln_model.py: the bound that tests/test_gpu_fulladaln.py holds the full-width adaLN producer's h to is
sound for the kernel's arithmetic in its source order on every family, width and dtype, and sharp enough to catch each of a list
of plausible kernel mistakes."""
import itertools
import math

import pytest
import torch

from tests import adaln_model as am
from tests import fulladaln_model as fa

F16, F32 = torch.float16, torch.float32
B, L = 2, 13                                     # 26 rows: every family twice, batch entries of odd length
EPS = (1e-6, 1e-5, 1e-3)


def _ratio_by_family(h, ref, x_dtype, C, R):
    r = torch.nan_to_num((h.double() - ref["h"]).abs() / fa.bound(ref, x_dtype, C), nan=math.inf)
    out = {}
    for i, f in enumerate(am.families(R, C)):
        if bool(ref["finite"][i]):
            out[f] = max(out.get(f, 0.0), float(r[i].max()))
    return out


def test_geometry_and_depth():
    assert [fa.operands(C) for C in fa.WIDTHS] == [4, 6] and [fa.padded(C) for C in fa.WIDTHS] == [2048, 3072]
    assert [fa.depth(F16, C) for C in fa.WIDTHS] == [17, 19] and [fa.depth(F32, C) for C in fa.WIDTHS] == [17, 19]
    for C in fa.WIDTHS:                          # every channel of the row sits in exactly one live (operand, lane, element)
        v, live = fa._lanes(torch.arange(1, C + 1, dtype=torch.float32).view(1, C), C)
        got = v[0][live].flatten().sort().values
        assert torch.equal(got, torch.arange(1, C + 1, dtype=torch.float32)) and float(v[0][~live].abs().max()) == 0.0


@pytest.mark.parametrize("x_dtype", (F16, F32))
@pytest.mark.parametrize("C", fa.WIDTHS)
def test_the_emulation_is_within_the_bound(C, x_dtype):
    """All 13 families, both modulation dtypes, with and without a smoothing vector, three eps: the fp32 model of the kernel's
    arithmetic stays within bound() and puts its non-finite elements where the reference has them.  Worst err / bound of the model:
    0.9993 (the half-ulp term; the same figure at both widths and row dtypes)."""
    worst_all = 0.0
    for mod_dtype, with_smooth, eps in itertools.product((F16, F32), (False, True), EPS):
        x, scale, shift, smooth = fa.make_case(B, L, C, x_dtype, mod_dtype, with_smooth, eps)
        ref = fa.reference(x, scale, shift, smooth, eps, L)
        assert set(am.families(B * L, C)) == set(fa.FAMILIES) and len(fa.FAMILIES) == 13
        worst, where_ok = fa.check(fa.emulate(x, scale, shift, smooth, eps, L), ref, x_dtype, C)
        worst_all = max(worst_all, worst)
        assert worst <= 1.0 and where_ok, (mod_dtype, with_smooth, eps, worst, where_ok)
    print(f"fulladaln model C={C} {x_dtype}: worst err / bound {worst_all:.4f}")


@pytest.mark.parametrize("x_dtype", (F16, F32))
@pytest.mark.parametrize("vector", ("var30/mat_qkv", "var30/fc1", "var36/mat_qkv", "var36/fc1"))
def test_the_emulation_is_within_the_bound_under_the_learned_vectors(vector, x_dtype):
    """The smoothing vectors the reference ships (tests/golden/reference_blocks.npz: factors from 0.012 to 2.79, four of them
    negative) at their own widths, 17 rows (every family): the fp32 model stays within bound().  Only because this holds is the
    bound a fair limit for the kernel under these vectors (tests/test_gpu_learned_smoothing.py)."""
    from tests import block_fixture as bf
    smooth = bf.learned_vectors()[vector]
    C = smooth.numel()
    for mod_dtype in (F16, F32):
        x, scale, shift, _ = fa.make_case(1, 17, C, x_dtype, mod_dtype, False, 1e-6)
        ref = fa.reference(x, scale, shift, smooth, 1e-6, 17)
        assert set(am.families(17, C)) == set(fa.FAMILIES) and float(ref["h"][ref["finite"]].abs().max()) < 6.0e4
        worst, where_ok = fa.check(fa.emulate(x, scale, shift, smooth, 1e-6, 17), ref, x_dtype, C)
        assert worst <= 1.0 and where_ok, (mod_dtype, worst, where_ok)


# mutation -> (C, x dtype, modulation dtype, a family that must exceed the bound).  Every mutant is caught on make_case's own rows.
# batch_off_by_one moves only the last row of a batch entry to its neighbour's modulation: with (B, L) = (2, 13) that is row 12 - the
# "var_eps" row at C = 1920, the "inf" row at C = 2304 (not a finite row) - hence C = 1920.  scale_plus_one_fp32 needs fp16 modulation.
CAUGHT_AT = {
    "pad_in_centred_sum": (2304, F32, F16, "rho2_8.8"),
    "mean_over_padded": (1920, F32, F16, "gauss"),
    "eps_ignored": (1920, F16, F16, "var_eps"),
    "var_unbiased": (2304, F32, F16, "gauss"),
    "scale_plus_one_fp32": (1920, F32, F16, "gauss"),
    "batch_off_by_one": (1920, F32, F16, "var_eps"),
    "smooth_after_round": (2304, F16, F32, "gauss"),
    "stats_of_x_smooth": (1920, F32, F16, "lognormal"),
}


@pytest.mark.parametrize("mutation", fa.MUTATIONS)
def test_each_mutation_exceeds_the_bound(mutation):
    C, x_dtype, mod_dtype, family = CAUGHT_AT[mutation]
    x, scale, shift, smooth = fa.make_case(B, L, C, x_dtype, mod_dtype, True, 1e-6)
    ref = fa.reference(x, scale, shift, smooth, 1e-6, L)
    clean = _ratio_by_family(fa.emulate(x, scale, shift, smooth, 1e-6, L), ref, x_dtype, C, B * L)
    assert max(clean.values()) <= 1.0
    got = _ratio_by_family(fa.emulate(x, scale, shift, smooth, 1e-6, L, mutation=mutation), ref, x_dtype, C, B * L)
    assert got[family] > 1.0, (mutation, family, got)


def test_the_bound_is_the_block_kernels_or_tighter():
    """The same derivation with the same depth on fp32 rows (17 / 19, as adaln_model.depth has it at these widths), no one-pass
    branch and the fused modulate alone: never above adaln_model.bound."""
    for C in fa.WIDTHS:
        x, scale, shift, smooth = fa.make_case(B, L, C, F32, F16, True, 1e-6)
        ref = fa.reference(x, scale, shift, smooth, 1e-6, L)
        fin = ref["finite"]
        assert bool((fa.bound(ref, F32, C)[fin] <= am.bound(ref, F32, C)[fin] * (1 + 1e-12)).all())
