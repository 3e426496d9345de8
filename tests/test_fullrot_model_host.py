"""CPU-only: the float64 model of the full-width online rotation (tests/fullrot_model.py).  The factorisation the kernel runs equals
the product with half(Q) exactly; an emulation of the shipped arithmetic - the kernel's operand mapping, fp32 accumulators, the
three-piece split - meets the bound on every input family; and every way of getting the transform wrong that the bound has to
catch exceeds it."""
import pytest
import torch

from fpqvar_amd import rotation
from tests import fullrot_model as fm

ROWS = 6


@pytest.mark.parametrize("C", fm.WIDTHS)
def test_half_q_has_one_magnitude(C):
    q = fm.q_half(C)
    assert q.abs().unique().numel() == 1
    assert fm.c_h(C) == float(torch.tensor(C).sqrt().reciprocal().half())      # float32 1 / sqrt(C), rounded to fp16


@pytest.mark.parametrize("C", fm.WIDTHS)
def test_factorisation_is_the_product_exactly(C):
    for name, make in fm.FAMILIES.items():
        h = make(ROWS, C)
        assert float((fm.factorised(h, C) - fm.reference(h, C)).abs().max()) == 0.0, name


@pytest.mark.parametrize("C", fm.WIDTHS)
@pytest.mark.parametrize("family", list(fm.FAMILIES))
def test_emulated_kernel_meets_the_bound(C, family):
    h = fm.FAMILIES[family](ROWS, C)
    ref = fm.reference(h, C)
    y = fm.emulate(h, C)
    ratio = float(((y.double() - ref).abs() / fm.bound(h, ref, C)).max())
    print(f"C={C} {family}: worst err / bound {ratio:.3f}")
    assert ratio <= 1.0


def test_three_piece_split_is_exact():
    import numpy as np
    g = torch.Generator().manual_seed(5)
    p = (torch.randn(1 << 16, generator=g) * torch.exp(4.0 * torch.randn(1 << 16, generator=g))).float().numpy()
    t1, t2, t3 = fm._split3(p)
    assert np.array_equal(t1.astype(np.float64) + t2.astype(np.float64) + t3.astype(np.float64), p.astype(np.float64))
    assert np.array_equal(np.abs(t1) + np.abs(t2) + np.abs(t3), np.abs(p))    # the pieces carry p's sign
    for t in (t1, t2, t3):
        assert not (t.view(np.uint32) & 0xFFFF).any()                          # each one a bf16 number


MUTANTS = {
    "hadK transposed": lambda C: dict(had_t=True),
    "the 128-long sign vector tiled": lambda C: dict(d=rotation.sign_vector(128, 42).repeat(C // 128)),
    "Kronecker order swapped": lambda C: dict(swap=True),
    "c = 1 / sqrt(128)": lambda C: dict(c=float(torch.tensor(128).sqrt().reciprocal().half())),
    "one kj segment dropped": lambda C: dict(drop=5),
}


@pytest.mark.parametrize("C", fm.WIDTHS)
@pytest.mark.parametrize("mutant", list(MUTANTS))
def test_mutants_exceed_the_bound(C, mutant):
    if mutant == "hadK transposed" and C == 2304:
        had36, _ = rotation.get_hadK(2304)
        assert torch.equal(had36, had36.T)        # Paley II is symmetric: the transposed factor shows at C = 1920 only
        return
    h = fm.rows_heavy(ROWS, C)
    ref = fm.reference(h, C)
    ratio = float(((fm.factorised(h, C, **MUTANTS[mutant](C)) - ref).abs() / fm.bound(h, ref, C)).max())
    print(f"C={C} {mutant}: worst err / bound {ratio:.1f}")
    assert ratio > 100.0


def test_paley_59_is_not_symmetric():
    had60, k = rotation.get_hadK(1920)
    assert k == 60 and not torch.equal(had60, had60.T)
