"""CPU checks of tests/gelu_model.py, over all 65536 fp16 inputs: the bound that tests/test_gpu_gelu.py holds every instantiation
of gelu_tanh_fast to is derived from the reference's op sequence and the reference alone stays inside it (torch's fp32 chain on
the CPU), so does the fp32 model of the kernel; it is sharp enough to catch each modelled mistake; and the kernel's snap is what
it is documented to be - a deliberate loss of accuracy for parity with torch on the deep negatives."""
import math

import pytest
import torch
import torch.nn.functional as Fn

from tests import gelu_model as gm

# the worst ratio each mutation reaches over the 65536 inputs is printed; it must exceed 1 (measured with the snap: kappa 1.46,
# beta 3.9, erf 459, sigmoid 1.8e4, w_fp16 2.9, exp_for_exp2 3.4e3, ftz_out 2.0e3, rtz_out 2.0)


@pytest.fixture(scope="module")
def every():
    return gm.every_fp16()


def test_reference_non_finite_pattern_and_zeros(every):
    """NaN -> NaN, +inf -> +inf, -inf -> NaN; every finite input gives a finite value, the large negative ones -0, -0 gives -0."""
    g = gm.reference(every)
    x = every.double()
    assert torch.equal(torch.isnan(g), torch.isnan(x) | (x == -math.inf))
    assert torch.equal(torch.isinf(g), x == math.inf) and bool((g[x == math.inf] > 0).all())
    assert bool(torch.isfinite(g[torch.isfinite(x)]).all())
    deep = torch.isfinite(x) & (x < -10)
    assert bool((g[deep] == 0).all()) and bool(torch.signbit(g[deep]).all())
    zero = every == 0
    assert bool((g[zero] == 0).all()) and torch.equal(torch.signbit(g[zero]), torch.signbit(every[zero]))
    assert float(g[torch.isfinite(g)].abs().max()) == 65504.0                      # never at the overflow edge of fp16
    # float64 values pass through unchanged: tests/block_model.py calls it on the Linear's float64 output
    assert torch.equal(gm.reference(x[:1024]), g[:1024])


def test_ulp16():
    g = torch.tensor([0.0, 2.0 ** -24, 2.0 ** -14 - 2.0 ** -24, 2.0 ** -14, 1.0, 1.5, 2.0 - 2.0 ** -10, 2.0, 65504.0, -3.0], dtype=torch.float64)
    want = [2.0 ** -24, 2.0 ** -24, 2.0 ** -24, 2.0 ** -24, 2.0 ** -10, 2.0 ** -10, 2.0 ** -10, 2.0 ** -9, 32.0, 2.0 ** -9]
    assert gm.ulp16(g).tolist() == want


def test_reference_op_sequence_stays_inside_the_bound(every):
    """The condition that makes the bound the reference's: torch's own fp32 chain, rounded once to fp16, is within it on EVERY
    input (none excluded), with the exact non-finite pattern and zero signs.  Worst: 0.999 at the tie x = +-2^-24 (the value is
    2^-25 (1 + 4.7e-8), fp32 cannot see the excess, nearest-even gives 0: half a spacing, all of the first term)."""
    out = Fn.gelu(every.float(), approximate="tanh").half()
    assert not bool(gm.class_mismatch(out, every).any())
    r = gm.ratios(out, every)
    worst = int(r.argmax())
    print(f"torch fp32 chain on the CPU: worst ratio {float(r[worst]):.4f} at x = {float(every[worst])!r}")
    assert gm.ratio(out, every) <= 1.0


def test_bound_dominates_its_accounting(every):
    """The closed form of bound() is no smaller than the term-by-term sum its docstring derives it from, on every finite input."""
    fin = torch.isfinite(every)
    b, t = gm.bound(every)[fin], gm.bound_terms(every)[fin]
    assert bool(torch.isfinite(b).all()) and bool((b > 0).all())
    assert bool((t <= b).all()), every[fin][t > b][:8].tolist()


@pytest.mark.parametrize("snap", [True, False])
def test_emulated_kernel_stays_inside_the_bound(every, snap):
    out = gm.emulate(every, snap=snap)
    assert not bool(gm.class_mismatch(out, every).any())
    r = gm.ratios(out, every)
    worst = int(r.argmax())
    print(f"emulate(snap={snap}): worst ratio {float(r[worst]):.4f} at x = {float(every[worst])!r}")
    assert gm.ratio(out, every) <= 1.0


@pytest.mark.parametrize("mutation", gm.MUTATIONS)
def test_every_mutation_breaks_the_bound(every, mutation):
    """with the snap and without it"""
    for snap in (True, False):
        r = gm.ratio(gm.emulate(every, snap=snap, mutation=mutation), every)
        print(f"{mutation} (snap={snap}): worst ratio {r:.4g}")
        assert r > 1.0, (mutation, snap, r)


def test_ratio_is_infinite_on_a_wrong_class(every):
    good = gm.emulate(every)
    for x, wrong in ((math.inf, math.nan), (-math.inf, -math.inf), (-math.inf, 0.0), (math.nan, 0.0), (-100.0, 0.0), (-0.0, 0.0), (0.0, -0.0),
                     (100.0, math.inf)):
        i = int(gm.bits(torch.tensor([x], dtype=torch.float16)))
        out = good.clone()
        out[i] = wrong
        assert bool(gm.class_mismatch(out, every)[i]) and int(gm.class_mismatch(out, every).sum()) == 1 and gm.ratio(out, every) == math.inf, x


def test_snap_trades_accuracy_for_parity(every):
    """Without `(w - 0.5) + 0.5` the model returns the correctly rounded fp16 of the float64 value on every input that fp32 can
    decide: all but those whose value lies within 2^-24 (relative) of a rounding tie - seven inputs, +-2^-24, +-0.001339, +-0.3533
    and 1.978 - and on those it returns one of the tie's two neighbours.  With the snap it misses the correctly rounded value on
    a few hundred inputs more, every one of them with g < 0 (the deep negatives, where torch's 1 + tanh cancels and the snap puts w on
    the same 2^-24 grid): up to 3.4 half-spacings at x = -5.15625, against 5.0 for torch's own chain at x = -5.0625."""
    g = gm.reference(every)
    fin = torch.isfinite(g)
    cr = gm.correctly_rounded(every)
    assert not bool(gm.class_mismatch(cr, every).any()) and gm.ratio(cr, every) <= 1.0
    assert float(((cr.double() - g).abs() / gm.ulp16(g))[fin].max()) <= 0.5
    near_tie = (gm.tie_distance(every) < 2.0 ** -24) & fin
    assert int(near_tie.sum()) == 7
    miss = lambda out: fin & (gm.bits(out) != gm.bits(cr))
    half_spacings = lambda out: torch.where(fin, (out.double() - g).abs() / (0.5 * gm.ulp16(g)), torch.zeros_like(g))

    plain = gm.emulate(every, snap=False)
    assert not bool((miss(plain) & ~near_tie).any()), every[miss(plain) & ~near_tie].tolist()
    order = lambda h: torch.where(gm.bits(h) >= 0x8000, 0x8000 - gm.bits(h), gm.bits(h))
    assert int((order(plain) - order(cr)).abs()[fin].max()) <= 1

    snapped = gm.emulate(every, snap=True)
    m = miss(snapped) & ~near_tie
    torch_m = miss(Fn.gelu(every.float(), approximate="tanh").half()) & ~near_tie
    hs, ht = half_spacings(snapped), half_spacings(Fn.gelu(every.float(), approximate="tanh").half())
    print(f"not correctly rounded: model with snap {int(m.sum())} inputs, worst {float(hs.max()):.2f} half-spacings at x = {float(every[int(hs.argmax())])!r}; "
          f"torch's fp32 chain {int(torch_m.sum())} inputs, worst {float(ht.max()):.2f} at x = {float(every[int(ht.argmax())])!r}")
    assert 100 <= int(m.sum()) <= 500
    assert bool((g[m] < 0).all())
    assert 100 <= int(torch_m.sum()) <= 500 and bool((g[torch_m] < 0).all())
    assert float(hs.max()) <= float(ht.max())          # the snap copies torch's grid, not more than its error
