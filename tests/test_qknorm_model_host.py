"""CPU checks of tests/qknorm_model.py: the bound that tests/test_gpu_qknorm.py holds the q / k L2 norm to is sound for the
kernels' arithmetic in both lane splits (and for torch's own fp32 lines), sharp enough to catch each of a list of plausible
kernel mistakes, and the reference's non-finite pattern is the one F.normalize leaves."""
import math

import pytest
import torch

from tests import qknorm_model as qm

T = 24
SCALES = (1.0, 3.7, 100.0)


def _merge(into, worst):
    for f, r in worst.items():
        into[f] = max(into.get(f, 0.0), r)


def _run(fn, s_h, parts=(0, 1, 2)):
    """worst err / bound per family of fn(y16, bias, hs, part) over the parts, with and without the bias; and whether the
    non-finite elements were where the reference has them throughout"""
    y16, bias, hs = qm.make_case(T, s_h)
    worst, where_ok = {}, True
    for with_bias in (True, False):
        for part in parts:
            b = bias[part] if with_bias else None
            ref, fin = qm.reference(y16[:, part], b, hs, part)
            w, wrong = qm.check(fn(y16[:, part], b, hs, part), ref, fin)
            _merge(worst, w)
            where_ok = where_ok and not wrong
    return worst, where_ok


@pytest.mark.parametrize("s_h", SCALES)
def test_the_case_meets_the_input_conditions_and_holds_every_family(s_h):
    y16, bias, hs = qm.make_case(T, s_h)
    assert set(qm.HEADS) == set(qm.FAMILIES) and qm.H % 2 == 0
    for part in range(3):
        for b in (bias[part], None):
            assert float(qm.sum_of_squares(y16[:, part], b).max()) < 2.0 ** 120
            assert qm.clear_of_overflow(y16[:, part], b, hs, part)
    k, fin = qm.reference(y16[:, 1], bias[1], hs, 1)
    q, fin_q = qm.reference(y16[:, 0], bias[0], hs, 0)
    col = {f: slice(64 * qm.HEADS.index(f), 64 * qm.HEADS.index(f) + 64) for f in qm.FAMILIES}
    sub = k[:, col["dominant_3000"]].abs()
    assert bool(((sub > 0) & (sub < 2.0 ** -14)).any()), "dominant element: no fp16-subnormal output"
    assert float(k[:, col["dominant_60000"]].abs().min()) < 2.0 ** -24
    assert float(y16[:, 1, col["fp16_max"]].float().abs().min()) >= 60000
    y_sub = y16[:, 1, col["subnormal"]].float().abs()
    assert float(y_sub.max()) < 2.0 ** -14 and float(y_sub.max()) > 0
    y_c = y16[:, 1, col["cancel"]].double() + bias[1, col["cancel"]].double()
    assert float((y_c.abs() / bias[1, col["cancel"]].double().abs()).median()) < 2.0 ** -6, "no cancellation"
    assert float(k[:, col["constant"]].abs().max()) == pytest.approx(0.125) and float(k[:, col["constant"]].abs().min()) == pytest.approx(0.125)
    n_tiny = torch.sqrt(qm.sum_of_squares(y16[:, 1], bias[1]))
    assert 0 < float(n_tiny[:, qm.HEADS.index("norm_tiny")].max()) < 0.5e-12
    straddle = [h for h, f in enumerate(qm.HEADS) if f == "norm_straddle"]
    norms = torch.cat([torch.sqrt(qm.sum_of_squares(y16[:, p], bias[p]))[0, straddle] for p in (0, 1)])
    assert bool((norms < 1e-12).any() and (norms > 1e-12).any() and ((norms / 1e-12 - 1).abs() < 5e-3).all()), norms
    assert bool((k[:, col["zero"]] == 0).all())
    assert float(hs[qm.HEADS.index("scale_100")]) == 100.0
    big = q[:, col["scale_1e5"]]
    assert bool(torch.isinf(big).any(dim=1).all() and (torch.isfinite(big) & (big.abs() > 1000)).any(dim=1).all()), "s_h = 1e5: both kinds"
    for f in qm.NONFINITE:
        assert not bool(fin[:, col[f]].all(dim=1).any()), f
    assert bool(fin[:, : 64 * qm.HEADS.index("scale_1e5")].all())


@pytest.mark.parametrize("variant", qm.VARIANTS)
@pytest.mark.parametrize("s_h", SCALES)
def test_the_shipped_arithmetic_is_within_the_bound(variant, s_h):
    """the fp32 model of the kernels' lines, in the lane split of the GEMMs and of the KV step: err / bound <= 1 on every family, v
    bit for bit, non-finite elements exactly the reference's"""
    worst, where_ok = _run(lambda y, b, hs, part: qm.emulate(y, b, hs, part, variant), s_h)
    print(f"\n{variant} s_h={s_h}: worst err / bound {max(worst.values()):.4f} ({max(worst, key=worst.get)})")
    assert max(worst.values()) <= 1.0 and where_ok, (worst, where_ok)
    y16, bias, hs = qm.make_case(T, s_h)
    v = qm.emulate(y16[:, 2], bias[2], hs, 2, variant)
    assert torch.equal(v.view(torch.int16), (y16[:, 2].float() + bias[2]).half().view(torch.int16))


@pytest.mark.parametrize("s_h", SCALES)
def test_torchs_own_fp32_lines_are_within_the_bound(s_h):
    worst, where_ok = _run(qm.torch_lines, s_h)
    print(f"\ntorch fp32 lines s_h={s_h}: worst err / bound {max(worst.values()):.4f} ({max(worst, key=worst.get)})")
    assert max(worst.values()) <= 1.0 and where_ok, (worst, where_ok)


def test_the_bound_does_not_depend_on_its_fp32_constant():
    """the shipped arithmetic also meets the bound with a quarter of the fp32 term: the constant is a count, not a fit"""
    saved = qm.C_FP32
    try:
        qm.C_FP32 = 4
        for variant in qm.VARIANTS:
            worst, _ = _run(lambda y, b, hs, part: qm.emulate(y, b, hs, part, variant), 3.7)
            assert max(worst.values()) <= 1.0, worst
    finally:
        qm.C_FP32 = saved


# mutation -> (s_h, families of which at least one must exceed the bound)
CAUGHT_AT = {
    "q_half_before_scale": (3.7, ("gauss", "heavy", "constant")),
    "bias_before_half": (1.0, ("cancel", "norm_tiny", "norm_straddle")),
    "eps_on_sumsq": (1.0, ("norm_tiny", "norm_straddle", "subnormal")),
    "lane_missing": (1.0, ("gauss", "constant", "fp16_max")),
    "scale_on_k": (3.7, ("gauss", "constant")),
    "round_toward_zero": (1.0, ("gauss", "heavy")),
}


@pytest.mark.parametrize("mutation", sorted(CAUGHT_AT))
def test_each_wrong_variant_exceeds_the_bound(mutation):
    s_h, fams = CAUGHT_AT[mutation]
    for variant in qm.VARIANTS:
        got, _ = _run(lambda y, b, hs, part: qm.emulate(y, b, hs, part, variant, mutation), s_h, parts=(0, 1))
        print(f"\n{mutation} ({variant}, s_h={s_h}): " + ", ".join(f"{f} {got[f]:.3g}" for f in qm.FAMILIES if got[f] > 1.0))
        assert any(got[f] > 1.0 for f in fams), (mutation, variant, got)


def test_q_rounded_before_the_scale_is_caught_at_the_clamp_too():
    got, _ = _run(lambda y, b, hs, part: qm.emulate(y, b, hs, part, "gemm", "q_half_before_scale"), 100.0, parts=(0,))
    print(f"\nq_half_before_scale s_h=100: gauss {got['gauss']:.3g}, scale_100 {got['scale_100']:.3g}")
    assert got["gauss"] > 1.0 and got["scale_100"] > 1.0


@pytest.mark.parametrize("variant", qm.VARIANTS)
def test_the_unguarded_residual_step_poisons_inf_heads_and_nothing_else(variant):
    """the kernels as they were: fma(fma(-q, inf, y), 0, q) = NaN on all 64 elements of a head with an inf and no NaN, where the
    reference has NaN at the inf elements and zeros beside them; every other family keeps its bits"""
    y16, bias, hs = qm.make_case(T, 3.7)
    for part in (0, 1):
        old = qm.emulate(y16[:, part], bias[part], hs, part, variant, "inf_residual_unguarded")
        new = qm.emulate(y16[:, part], bias[part], hs, part, variant)
        ref, fin = qm.reference(y16[:, part], bias[part], hs, part)
        differ = (old.view(torch.int16) != new.view(torch.int16)).view(T, qm.H, 64).any(dim=2).any(dim=0)
        assert {qm.HEADS[h] for h in differ.nonzero().flatten().tolist()} == {"inf", "inf_pm"}
        for f in ("inf", "inf_pm"):
            cols = slice(64 * qm.HEADS.index(f), 64 * qm.HEADS.index(f) + 64)
            assert bool(torch.isnan(old[:, cols]).all())
            assert int(torch.isnan(ref[:, cols]).sum()) == T * (1 if f == "inf" else 2)
        assert qm.check(old, ref, fin)[1] == ["inf", "inf_pm"] and qm.check(new, ref, fin)[1] == []


@pytest.mark.parametrize("s_h", SCALES)
def test_the_references_non_finite_pattern_is_f_normalizes(s_h):
    y16, bias, hs = qm.make_case(T, s_h)
    for part in range(3):
        for b in (bias[part], None):
            ref, _ = qm.reference(y16[:, part], b, hs, part)
            want = qm.torch_lines(y16[:, part], b, hs, part).double()
            assert torch.equal(torch.isnan(ref), torch.isnan(want)), part
            assert torch.equal(torch.where(torch.isinf(ref), ref, torch.zeros_like(ref)), torch.where(torch.isinf(want), want, torch.zeros_like(want))), part
            nf = ~torch.isfinite(y16[:, part].float() + (b if b is not None else 0.0)).view(T, qm.H, 64).all(dim=2)
            if part < 2:   # the zeros beside an inf
                heads = (nf & ~torch.isnan(ref).view(T, qm.H, 64).all(dim=2)).unsqueeze(-1).expand(T, qm.H, 64).reshape(T, qm.C)
                assert bool(((ref == 0) | torch.isnan(ref))[heads].all()) and bool(((want == 0) | torch.isnan(want))[heads].all())
    assert math.isinf(float(torch.tensor(qm.HALF_OVERFLOW).half())) and float(torch.tensor(qm.HALF_OVERFLOW - 1).half()) == 65504.0
