"""CPU checks of tests/adaln_model.py: the bound that tests/test_gpu_adaln.py holds the adaLN producer to is sound for the
kernels' arithmetic in each of their summation orders, tight where the rows are benign, and sharp enough to catch each of a list
of plausible kernel mistakes; the row families have the mean^2 / var they claim."""
import math

import pytest
import torch

from tests import adaln_model as am

F16, F32 = torch.float16, torch.float32
WIDTHS = (128, 1024, 1152, 1920, 2304, 2560, 2688, 3072, 3968, 4096)
B, L = 2, 13                                     # 26 rows: every family twice, batch entries of odd length


def _orders(C, x_dtype):
    """the summation orders that exist at this width and row dtype"""
    o = ["lane_tree"]
    if x_dtype == F16 and am.maxc(C) == 5 and C <= am.WIDE_FROM:
        o.append("slot_hi")
    if x_dtype == F16 and C == 1024:
        o.append("pair2")
    return o


def _ratio_by_family(h, ref, x_dtype, C, R):
    r = torch.nan_to_num((h.double() - ref["h"]).abs() / am.bound(ref, x_dtype, C), nan=math.inf)
    out = {}
    for i, f in enumerate(am.families(R, C)):
        if bool(ref["finite"][i]):
            out[f] = max(out.get(f, 0.0), float(r[i].max()))
    return out


@pytest.mark.parametrize("x_dtype", (F16, F32))
@pytest.mark.parametrize("C", WIDTHS)
def test_every_emulation_order_is_within_the_bound(C, x_dtype):
    """On every family, width and dtype of the GPU test, the fp32 model of the kernel's arithmetic stays within bound() in each
    summation order, and puts its non-finite elements where the reference has them."""
    for mod_dtype, with_smooth, eps in ((F16, True, 1e-6), (F32, False, 1e-2)):
        x, scale, shift, smooth = am.make_case(B, L, C, x_dtype, mod_dtype, with_smooth, eps)
        ref = am.reference(x, scale, shift, smooth, eps, L)
        assert set(am.families(B * L, C)) == set(am.FAMILIES)
        assert float(ref["h"][ref["finite"]].abs().max()) < 6.0e4
        for order in _orders(C, x_dtype):
            worst, where_ok = am.check(am.emulate(x, scale, shift, smooth, eps, L, order), ref, x_dtype, C)
            assert worst <= 1.0 and where_ok, (order, mod_dtype, eps, worst, where_ok)


LEARNED = ("var30/mat_qkv", "var30/fc1", "var36/mat_qkv", "var36/fc1")


@pytest.mark.parametrize("x_dtype", (F16, F32))
@pytest.mark.parametrize("vector", LEARNED)
def test_every_emulation_order_is_within_the_bound_under_the_learned_vectors(vector, x_dtype):
    """The smoothing vectors the reference ships (tests/golden/reference_blocks.npz: factors from 0.012 to 2.79, four of them
    negative) instead of make_case's rand * 1.5 + 0.25, at their own widths, 17 rows (every family): the fp32 model stays within
    bound() in each summation order.  Only because this holds is the bound a fair limit for the kernels under these vectors
    (tests/test_gpu_learned_smoothing.py)."""
    from tests import block_fixture as bf
    smooth = bf.learned_vectors()[vector]
    C = smooth.numel()
    for mod_dtype in (F16, F32):
        x, scale, shift, _ = am.make_case(1, 17, C, x_dtype, mod_dtype, False, 1e-6)
        ref = am.reference(x, scale, shift, smooth, 1e-6, 17)
        assert set(am.families(17, C)) == set(am.FAMILIES) and float(ref["h"][ref["finite"]].abs().max()) < 6.0e4
        for order in _orders(C, x_dtype):
            worst, where_ok = am.check(am.emulate(x, scale, shift, smooth, 1e-6, 17, order), ref, x_dtype, C)
            assert worst <= 1.0 and where_ok, (order, mod_dtype, worst, where_ok)


# mutation -> (C, x dtype, modulation dtype, eps, a family that must exceed the bound)
CAUGHT_AT = {
    "one_pass_always": (1920, F32, F32, 1e-6, "rho_high"),                    # rho = 1000: E[x^2] - mean^2 cancels six digits
    "pad_subtract": (2688, F32, F16, 1e-6, "rho_high"),                       # the wide kernel before its fix
    "eps_ignored": (1920, F16, F16, 1e-6, "var_eps"),
    "scale_plus_one_fp32": (1920, F16, F16, 1e-6, "gauss"),
    "batch_off_by_one": (2688, F16, F16, 1e-6, "gauss"),
    "var_unbiased": (1920, F16, F16, 1e-6, "gauss"),
    "smooth_after_round": (1920, F16, F16, 1e-6, "gauss"),
    "mean_over_padded": (1920, F16, F16, 1e-6, "rho2_7.2"),
    "second_row_takes_first_rows_stats": (1920, F16, F16, 1e-6, "rho_30"),
}


@pytest.mark.parametrize("mutation", am.MUTATIONS)
def test_each_mutation_exceeds_the_bound(mutation):
    C, x_dtype, mod_dtype, eps, family = CAUGHT_AT[mutation]
    x, scale, shift, smooth = am.make_case(B, L, C, x_dtype, mod_dtype, True, eps)
    ref = am.reference(x, scale, shift, smooth, eps, L)
    clean = _ratio_by_family(am.emulate(x, scale, shift, smooth, eps, L), ref, x_dtype, C, B * L)
    assert max(clean.values()) <= 1.0
    got = _ratio_by_family(am.emulate(x, scale, shift, smooth, eps, L, mutation=mutation), ref, x_dtype, C, B * L)
    assert got[family] > 1.0, (mutation, family, got)


def test_the_wide_kernel_before_its_fix_fails_at_padded_widths_and_not_at_4096():
    """Padding lanes that add (0 - mean)^2 and take 8 mean^2 back out leave the rounding of mean^2, once per padding vector, in
    the variance: beyond the bound at rho = 1000 with 176 and 128 padding vectors (C = 2688, 3072); at C = 4096 there is no
    padding.  (C = 3968 has 16 padding vectors: the model's error there is about half the bound - no claim.)"""
    for C in (2688, 3072, 4096):
        x, scale, shift, smooth = am.make_case(B, L, C, F32, F16, True, 1e-6)
        ref = am.reference(x, scale, shift, smooth, 1e-6, L)
        got = _ratio_by_family(am.emulate(x, scale, shift, smooth, 1e-6, L, mutation="pad_subtract"), ref, F32, C, B * L)
        assert (got["rho_high"] > 1.0) == (C != 4096), (C, got)
        assert got["gauss"] <= 1.0


@pytest.mark.parametrize("x_dtype", (F16, F32))
@pytest.mark.parametrize("C", (128, 1920, 2304, 4096))
def test_bound_is_tight_on_gauss_rows(C, x_dtype):
    """On gauss rows the bound is at most 1.25 x its half-ulp term: summed over a row (the row's error budget is five quarters
    of what the fp16 rounding alone takes), and at every element with |h| >= 1/8.  (Element for element the ratio has no upper
    limit under ANY derivation: the mean's and rstd's fp32 errors are absolute, ~1e-6 |A|, and an element of h that happens to
    fall near zero has a half-ulp of 2^-25.)"""
    x, scale, shift, smooth = am.make_case(B, L, C, x_dtype, F16, True, 1e-6)
    ref = am.reference(x, scale, shift, smooth, 1e-6, L)
    t, half = am.bound_terms(ref, x_dtype, C)
    rows = [i for i, f in enumerate(am.families(B * L, C)) if f == "gauss"]
    assert rows
    for i in rows:
        assert float((t[i] + half[i]).sum() / half[i].sum()) <= 1.25
        big = ref["h"][i].abs() >= 0.125
        assert float(((t[i] + half[i]) / half[i])[big].max()) <= 1.25


@pytest.mark.parametrize("x_dtype", (F16, F32))
def test_families_have_the_rho_they_claim(x_dtype):
    C = 1920
    x = am.make_rows(B * L, C, x_dtype, 1e-6)
    xd = x.double()
    rho2 = xd.mean(dim=1) ** 2 / xd.var(dim=1, unbiased=False)
    T = am.switch_point(x_dtype)
    for i, f in enumerate(am.families(B * L, C)):
        r = float(rho2[i])
        if f.startswith("rho2_"):
            want = float(f[5:])
            assert abs(r / want - 1) < 0.01, (f, r)
            for t in (8.0, 64.0):                         # on the side of each switch point it claims, by ~10 %
                assert (r < t) == (want < t)
            assert min(abs(r / 8 - 1), abs(r / 64 - 1)) < 0.12
        elif f == "rho_30":
            assert abs(math.sqrt(r) / 30 - 1) < 0.01 and r > T
        elif f == "rho_high":
            assert abs(math.sqrt(r) / (256 if x_dtype == F16 else 1000) - 1) < 0.02
            if x_dtype == F16:                            # 64 + 0.25 z on fp16's grid there (2^-5 below 64, 2^-4 above)
                assert float((x[i].double() - 64).abs().max()) < 2.0
        elif f in ("gauss", "lognormal"):
            assert r < 0.1
        elif f == "constant":
            assert float(xd[i].var(unbiased=False)) == 0.0
        elif f == "var_eps":
            assert abs(float(xd[i].var(unbiased=False)) / 1e-6 - 1) < 0.05
        elif f == "mag_1e4":
            assert 5e3 < float(xd[i].std()) < 2e4
        else:
            assert not bool(torch.isfinite(xd[i]).all())


@pytest.mark.parametrize("C,order", ((1024, "pair2"), (2176, "slot_hi"), (2304, "slot_hi")))
def test_two_summation_orders_change_few_quantized_groups(C, order):
    """What (c) of the GPU test caps at 1 % on gauss and log-normal rows: the share of groups of 128 whose quantized values
    differ between two summation orders of the same row stays under 0.25 % in the model.  The other order applies to every
    second row (the second row of a pair); C = 1024: with a partner row that forces the centred pass on both."""
    R = 96
    x, scale, shift, smooth = am.make_case(1, R, C, F16, F16, True, 1e-6, fams=am.SHARE_CAPPED)
    if order == "pair2":
        x = x.clone()
        x[1::2] = am.make_rows(R // 2, C, F16, 1e-6, 1, ("rho_30",))
    a = am.emulate(x, scale, shift, smooth, 1e-6, R, "lane_tree")
    b = am.emulate(x, scale, shift, smooth, 1e-6, R, order)
    rows = slice(0, R, 2) if order == "pair2" else slice(0, R)
    qa, qb = am.quantized_groups(a[rows]), am.quantized_groups(b[rows])
    differ = (qa.view(torch.int16) != qb.view(torch.int16)).view(-1, C // 128, 128).any(dim=2)
    share = float(differ.float().mean()) * (1.0 if order == "pair2" else 0.5)   # slot_hi: every second row only
    print(f"C={C} {order}: {int(differ.sum())} of {differ.numel()} groups differ, share {share:.4%}")
    assert share < 0.0025
