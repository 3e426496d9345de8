"""CPU checks of tests/attention_model.py: the bound that tests/test_gpu_attention.py holds fpq_attention_blhc to is sound
for the kernel's arithmetic (the fp32 model emulate() stays inside it with margin), sharp enough to catch each modelled
kernel mistake, and measured against a reference that is softmax(s) v."""
import pytest
import torch

from tests import attention_model as am

SHAPES = ((1, 3, 33, 65), (2, 2, 17, 193), (1, 2, 5, 129), (3, 1, 9, 2241))   # (B, H, Lq, Lkv)

# a family in which each mutation must exceed twice the bound, and the shape (B, H, Lq, Lkv) it is shown at
CATCHES = {
    "drop_last": ("plant_last_key_indicator", (1, 2, 9, 65)),
    "dup_last": ("uniform_indicator", (1, 2, 9, 65)),
    "no_rescale": ("plant_rising", (1, 2, 9, 193)),
    "half_l": ("plain", (1, 2, 9, 129)),
    "q_prescale": ("l2norm", (1, 4, 33, 193)),
    "p_bf16": ("plain_zeros", (1, 2, 33, 129)),
}


def _max_logit(q, k, scale):
    return float((torch.einsum("blhc,bmhc->bhlm", q.double(), k.double()) * scale).abs().max())


@pytest.mark.parametrize("family", list(am.FAMILIES))
def test_emulated_kernel_stays_inside_the_bound(family):
    """Faithful model: within 0.75 of the bound on normal outputs, within the bound everywhere (below 2^-14 the bound is
    the worst case of two roundings onto the subnormal grid).  Every family keeps |scale q.k| <= 100, the range the
    bound's fp32 term is derived for."""
    for B, H, Lq, Lkv in SHAPES:
        q, k, v, scale = am.make_case(family, B, H, Lq, Lkv)
        assert _max_logit(q, k, scale) <= 100.0
        r = am.reference(q, k, v, scale)
        out = am.emulate(q, k, v, scale)
        assert am.ratio(out, r, normal_only=True) <= 0.75, (family, B, H, Lq, Lkv)
        assert am.ratio(out, r) <= 1.0, (family, B, H, Lq, Lkv)


def test_emulated_kernel_over_the_shape_sweep():
    lkv = tuple(n for n in am.LKV_SWEEP if n < 1000)
    lq = tuple(n for n in am.LQ_SWEEP if n < 70)
    worst = 0.0
    for family, B, H, Lq, Lkv in am.shape_sweep(lkv, lq):
        q, k, v, scale = am.make_case(family, B, H, Lq, Lkv)
        r = am.reference(q, k, v, scale)
        out = am.emulate(q, k, v, scale)
        assert am.ratio(out, r) <= 1.0, (family, B, H, Lq, Lkv)
        worst = max(worst, am.ratio(out, r, normal_only=True))
    assert worst <= 0.75


@pytest.mark.parametrize("mutation", am.MUTATIONS)
def test_every_mutation_breaks_the_bound(mutation):
    family, (B, H, Lq, Lkv) = CATCHES[mutation]
    q, k, v, scale = am.make_case(family, B, H, Lq, Lkv)
    r = am.reference(q, k, v, scale)
    assert am.ratio(am.emulate(q, k, v, scale), r) <= 1.0
    assert am.ratio(am.emulate(q, k, v, scale, mutation), r) > 2.0, (mutation, family)


def test_the_padding_mutations_need_a_partial_last_tile():
    """dup_last counts a key past lkv: with lkv a multiple of 64 there is none, so the model must be unchanged there -
    the GPU test's Lkv sweep has to hold lkv mod 64 != 0 cases for this mistake to show."""
    q, k, v, scale = am.make_case("uniform_indicator", 1, 2, 9, 128)
    assert torch.equal(am.emulate(q, k, v, scale, "dup_last"), am.emulate(q, k, v, scale))


@pytest.mark.parametrize("family", ("l2norm", "plain", "uniform", "plant_last_key", "e2m3_ties", "l2norm_large"))
def test_reference_is_sdpa_in_float64(family):
    B, H, Lq, Lkv = 2, 3, 17, 70
    q, k, v, scale = am.make_case(family, B, H, Lq, Lkv)
    r = am.reference(q, k, v, scale)
    want = torch.nn.functional.scaled_dot_product_attention(*(t.double().transpose(1, 2) for t in (q, k, v)),
                                                            scale=scale).transpose(1, 2)
    assert torch.allclose(r.out, want, rtol=1e-12, atol=1e-12 * float(v.double().abs().max()))
    p = torch.softmax(torch.einsum("blhc,bmhc->bhlm", q.double(), k.double()) * scale, dim=-1)
    assert torch.allclose(r.A, torch.einsum("bhlm,bmhc->blhc", p, v.double().abs()), rtol=1e-12, atol=1e-300)
    assert bool((r.Z >= 1.0).all())


def test_shape_sweep_is_pairwise():
    sweep = am.shape_sweep()
    assert {(s[4], s[3]) for s in sweep} == {(a, b) for a in am.LKV_SWEEP for b in am.LQ_SWEEP}
    bh = {(s[1] * s[2]) for s in sweep}
    assert bh == {1, 7, 8, 9, 17}
    for n in am.LKV_SWEEP:
        assert {s[1] * s[2] for s in sweep if s[4] == n} == bh
    for n in am.LQ_SWEEP:
        assert {s[1] * s[2] for s in sweep if s[3] == n} == bh
    assert {s[0] for s in sweep} == set(am.FAMILIES)
