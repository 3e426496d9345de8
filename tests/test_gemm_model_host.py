"""CPU checks of tests/gemm_model.py: the bound that tests/test_gpu_gemm.py holds the matrix-core GEMMs to is sound for the
kernels' arithmetic (the fp32 model emulate() stays inside it), sharp enough to catch each modelled kernel mistake, not vacuous,
and measured against a reference whose decoder agrees with the format definitions and with gemm.dequantize_*."""
import math

import pytest
import torch

from tests import gemm_model as gm

SHAPES = ((33, 136, 384), (17, 128, 1920), (5, 8, 2304), (65, 120, 256))    # (T, O, K): G = 3, 15 (a partial scale piece), 18, 2

# (kind, mutation) -> the family and shape (T, O, K) where the mistake must exceed 1.5 x the bound (truncation errs by less than
# one ulp, i.e. less than twice the bound's 2^-11 |ref|, by construction)
CATCHES = {
    ("fp4", "rtz_out"): ("gauss", (65, 392, 256)),
    ("fp4", "bias_after_round"): ("bias_cancel", (33, 136, 384)),
    ("fp4", "scale_fp16"): ("group_range", (33, 136, 384)),
    ("fp4", "tail_group_scale"): ("one_group", (17, 128, 1920)),
    ("fp4", "drop_last_k"): ("one_group", (17, 128, 1920)),
    ("fp4", "sat_out"): ("overflow", (33, 136, 384)),
    ("fp4", "w_scale_fp16"): ("group_range", (33, 136, 384)),
    ("fp6", "rtz_out"): ("gauss", (65, 392, 256)),
    ("fp6", "bias_after_round"): ("bias_cancel", (33, 136, 384)),
    ("fp6", "scale_fp16"): ("bias_cancel", (33, 136, 384)),
    ("fp6", "drop_last_k"): ("one_group", (17, 128, 1920)),
    ("fp6", "sat_out"): ("overflow", (33, 136, 384)),
    ("fp6", "w_scale_fp16"): ("bias_cancel", (33, 136, 384)),
    ("fp8", "rtz_out"): ("gauss", (65, 392, 256)),
    ("fp8", "bias_after_round"): ("bias_cancel", (33, 136, 384)),
    ("fp8", "scale_fp16"): ("e4m3_full", (33, 136, 384)),
    ("fp8", "drop_last_k"): ("one_group", (17, 128, 1920)),
    ("fp8", "sat_out"): ("overflow", (33, 136, 384)),
    ("fp8", "w_scale_fp16"): ("bias_cancel", (33, 136, 384)),
}


def _args(c):
    return c["a"], c["a_scales"], c["w"], c["w_scales"], c["bias"]


def _orders(kind):
    return ("lds", "reg") if kind == "fp4" else ("lds",)


@pytest.mark.parametrize("kind", gm.KINDS)
def test_emulated_kernels_stay_inside_the_bound(kind):
    for family in gm.KIND_FAMILIES[kind]:
        for T, O, K in SHAPES:
            c = gm.make_case(kind, family, T, O, K)
            r = gm.reference(kind, *_args(c))
            for order in _orders(kind):
                for acc_round in (("rne", "rtz") if kind != "fp4" else ("rne",)):
                    out = gm.emulate(kind, *_args(c), order, acc_round=acc_round)
                    assert gm.ratio(out, r) <= 1.0, (kind, family, T, O, K, order, acc_round)


def test_emulated_kernels_over_the_shape_sweep():
    t = tuple(n for n in gm.T_SWEEP if n <= 65)
    o = tuple(n for n in gm.O_SWEEP if n <= 392)
    k = tuple(n for n in gm.K_SWEEP if n <= 2304)
    for kind in gm.KINDS:
        for family, T, O, K in gm.shape_sweep(t, o, k, gm.KIND_FAMILIES[kind]):
            c = gm.make_case(kind, family, T, O, K)
            r = gm.reference(kind, *_args(c))
            for order in _orders(kind):
                assert gm.ratio(gm.emulate(kind, *_args(c), order), r) <= 1.0, (kind, family, T, O, K, order)


@pytest.mark.parametrize("kind,mutation", list(CATCHES))
def test_every_mutation_breaks_the_bound(kind, mutation):
    family, (T, O, K) = CATCHES[(kind, mutation)]
    c = gm.make_case(kind, family, T, O, K)
    r = gm.reference(kind, *_args(c))
    for order in _orders(kind):
        assert gm.ratio(gm.emulate(kind, *_args(c), order), r) <= 1.0
        rat = gm.ratio(gm.emulate(kind, *_args(c), order, mutation), r)
        print(f"{kind} {mutation} {family} {order}: {rat:.3g}")
        assert rat > 1.5, (kind, mutation, family, order, rat)


def test_every_mutation_is_caught_for_every_kind_it_applies_to():
    for kind in gm.KINDS:
        for m in gm.MUTATIONS:
            assert (kind, m) in CATCHES or (m == "tail_group_scale" and kind != "fp4"), (kind, m)


@pytest.mark.parametrize("kind", gm.KINDS)
def test_the_bound_is_not_vacuous(kind):
    """On gauss the faithful model reaches 0.9 of the bound: the fp16 output rounding, 2^-11 |ref|, is reached by some element
    and the other terms are small against it."""
    c = gm.make_case(kind, "gauss", 65, 392, 1920)
    r = gm.reference(kind, *_args(c))
    assert gm.ratio(gm.emulate(kind, *_args(c)), r) >= 0.9


@pytest.mark.parametrize("kind", gm.KINDS)
def test_zero_family_is_exactly_the_bias(kind):
    for T, O, K in ((9, 136, 384), (10, 128, 256)):
        c = gm.make_case(kind, "zero", T, O, K)
        out = gm.emulate(kind, *_args(c))
        want = c["bias"].view(1, O).expand(T, O) if c["bias"] is not None else torch.zeros(T, O, dtype=torch.float16)
        assert torch.equal(out.view(torch.int16), want.contiguous().view(torch.int16))
        assert bool((gm.reference(kind, *_args(c)).out == want.double()).all())


@pytest.mark.parametrize("kind", gm.KINDS)
def test_overflow_family_straddles_the_fp16_edge(kind):
    c = gm.make_case(kind, "overflow", 65, 392, 384)
    ref = gm.reference(kind, *_args(c)).out.abs()
    assert bool((ref < 65504).any()) and bool(((ref > 65504) & (ref < 65520)).any()) and bool((ref > 65520).any())


def test_non_finite_family_classes():
    for kind in gm.KINDS:
        c = gm.make_case(kind, "non_finite", 40, 136, 384)
        r = gm.reference(kind, *_args(c))
        assert bool(torch.isnan(r.out).any()) and bool(torch.isposinf(r.out).any()) and bool(torch.isneginf(r.out).any())
        assert not bool(gm.class_mismatch(gm.emulate(kind, *_args(c)), r).any())
        assert bool(gm.class_mismatch(torch.zeros(40, 136, dtype=torch.float16), r).any())


def test_decoders_follow_the_format_definitions():
    assert gm._code_values("fp4").tolist()[:8] == list(gm.E2M1)
    e2m3 = gm._code_values("fp6")
    assert float(e2m3[31]) == 7.5 and float(e2m3[1]) == 0.125 and float(e2m3[32 + 9]) == -1.125
    e4m3 = gm._code_values("fp8")
    assert float(e4m3[0x7E]) == 448.0 and float(e4m3[1]) == 2.0 ** -9 and float(e4m3[0x38]) == 1.0
    assert math.isnan(float(e4m3[0x7F])) and math.isnan(float(e4m3[0xFF])) and float(e4m3[0xB8]) == -1.0
    g = torch.Generator().manual_seed(3)
    for kind, n in (("fp4", 16), ("fp6", 64), ("fp8", 256)):
        idx = torch.randint(0, n, (7, 256), generator=g)
        if kind == "fp8":
            idx[(idx & 0x7F) == 0x7F] = 0
        assert torch.equal(gm.decode(kind, gm.encode(kind, idx)), gm._code_values(kind)[idx])


def test_decoders_agree_with_the_package_decoders():
    """The package's own torch decoders (gemm.dequantize_*) read the same codes the same way (they run on any device)."""
    from fpqvar_amd import gemm
    for kind, deq in (("fp4", gemm.dequantize_mx), ("fp6", gemm.dequantize_fp6), ("fp8", gemm.dequantize_fp8)):
        c = gm.make_case(kind, "e4m3_full" if kind == "fp8" else "gauss", 9, 8, 384)
        La = gm.decode(kind, c["a"])
        s = c["a_scales"].double()
        want = (La.view(9, 3, 128) * s.view(9, 3, 1)).view(9, 384) if kind == "fp4" else La * s.view(9, 1)
        assert torch.equal(deq(c["a"], c["a_scales"]).double(), want), kind


def test_reference_is_the_dense_product():
    for kind in gm.KINDS:
        c = gm.make_case(kind, "gauss", 13, 24, 384)
        La, Lw = gm.decode(kind, c["a"]), gm.decode(kind, c["w"])
        if kind == "fp4":
            A = (La.view(13, 3, 128) * c["a_scales"].double().view(13, 3, 1)).view(13, 384)
            W = (Lw.view(24, 3, 128) * c["w_scales"].double().view(24, 3, 1)).view(24, 384)
        else:
            A, W = La * c["a_scales"].double().view(-1, 1), Lw * c["w_scales"].double().view(-1, 1)
        r = gm.reference(kind, *_args(c))
        want = A @ W.t() + c["bias"].double()
        assert torch.allclose(r.out, want, rtol=1e-13, atol=1e-13 * float((A.abs() @ W.abs().t()).max()))
        assert bool((r.S >= (r.out - c["bias"].double()).abs() * (1 - 1e-12)).all()) and bool((r.R >= 0).all())


def test_from_kmajor_inverts_the_image_layout():
    """from_kmajor against the layout rule of fpq_codes_to_kmajor written forwards."""
    g = torch.Generator().manual_seed(5)
    for bits, seg in ((4, 64), (6, 96)):
        for dealt in (False, True):
            rows, S = 70, 3
            codes = torch.randint(0, 256, (rows, S * seg), generator=g, dtype=torch.uint8)
            R = (rows + 63) // 64 * 64 if dealt else rows
            image = torch.zeros(S, R, seg, dtype=torch.uint8)
            cps = seg // 16
            for s in range(S):
                for j in range(R):
                    row = (j & ~63) + 4 * (j & 15) + ((j >> 4) & 3) if dealt else j
                    if row >= rows:
                        continue
                    for pc in range(cps):
                        c = pc ^ ((0x78 >> (((j & 15) >> 2) << 1)) & 3) if bits == 4 else (pc - ((j & 31) >> 3 & 1) + 6) % 6
                        image[s, j, pc * 16:(pc + 1) * 16] = codes[row, s * seg + c * 16:s * seg + (c + 1) * 16]
            assert torch.equal(gm.from_kmajor(image, bits, rows, dealt), codes), (bits, dealt)


def test_shape_sweep_is_pairwise():
    sweep = gm.shape_sweep()
    assert {(s[1], s[2]) for s in sweep} == {(a, b) for a in gm.T_SWEEP for b in gm.O_SWEEP}
    for n in gm.T_SWEEP:
        assert {s[3] for s in sweep if s[1] == n} == set(gm.K_SWEEP)
    for n in gm.O_SWEEP:
        assert {s[3] for s in sweep if s[2] == n} == set(gm.K_SWEEP)
    assert {s[0] for s in sweep} == set(gm.FAMILIES)
