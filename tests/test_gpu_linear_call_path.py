"""FP4Linear / FP4LinearGeluDual reach the kernels of their activation format and weight layout through gemm.py's shared call path:
for E2M1 / E1M2 / E3M0 activations, row-major and k-major, `forward`, `forward_operands` and `qkv_to_cache` give bit for bit what
the public function of that format gives on operands quantized by hand, the k-major module what the row-major one gives, and
mat_qkv into the cache the slices of `forward` - with the compiled binding as built and with the ctypes path alone.
tokens 5: a ragged last group of four rows in the scale image's padding; 133 = 7 x 19: more than one 128-row tile, ragged."""
import functools

import pytest
import torch

from tests.conftest import assert_bits_equal

pytestmark = pytest.mark.gpu

K, OUTS, HEADS = 256, 384, 2            # out_features = 3 * C, C = HEADS * 64
ACT = {"e2m1": "fp_e2", "e1m2": "fp_e1", "e3m0": "fp_e3"}
BATCHES = ((1, 5), (7, 19))
POS = 2


def _dev():
    return torch.device("cuda:0")


@functools.lru_cache(maxsize=None)
def _modules(fmt, km):
    """(FP4Linear, FP4LinearGeluDual, FP4Linear without bias) from one torch.nn.Linear(256, 384)"""
    from fpqvar_amd import gemm
    torch.manual_seed(11)
    lin = torch.nn.Linear(K, OUTS).to(_dev())
    m = gemm.FP4Linear.from_float(lin, kmajor=km, act_fp_type=ACT[fmt], a6w4_kmajor=km)
    f = gemm.FP4LinearGeluDual.from_float(lin, kmajor=km, act_fp_type=ACT[fmt], a6w4_kmajor=km)
    assert m.kmajor == km and f.kmajor == km and m.act_table == fmt and f.act_table == fmt
    return m, f, gemm.FP4Linear(m.w_codes, m.w_scales, None, K, OUTS, fmt)


@functools.lru_cache(maxsize=None)
def _inputs(bsz, seq):
    g = torch.Generator().manual_seed(100 * bsz + seq)
    x = torch.randn(bsz, seq, K, generator=g).half()
    gate, res = (torch.randn(bsz, 1, OUTS, generator=g) * 0.5).half(), torch.randn(bsz, seq, OUTS, generator=g).half()
    bias32 = torch.randn(OUTS, generator=g) * 0.1
    bias32[OUTS // 3:2 * OUTS // 3] = 0
    hs = torch.rand(HEADS, generator=g) * 3 + 1
    return tuple(t.to(_dev()) for t in (x, gate, res, bias32, hs))


def _plain(gemm, fmt, km, a, sa, m, *tail):
    if fmt == "e2m1":
        return gemm.linear_fp4(a, sa, m.w_codes, m.w_scales, m.bias, *tail, outs=OUTS)
    if km:
        return gemm.linear_a6w4_km(a, sa, fmt, m.w_codes, m.w_scales, m.bias, *tail, outs=OUTS)
    return gemm.linear_a6w4(a, sa, fmt, m.w_codes, m.w_scales, m.bias, *tail)


def _fc1(gemm, fmt, km, a, sa, m):
    if fmt == "e2m1":
        return gemm.linear_fp4_gelu_dual(a, sa, m.w_codes, m.w_scales, m.bias, outs=OUTS)
    if km:
        return gemm.linear_a6w4_gelu_dual_km(a, sa, fmt, m.w_codes, m.w_scales, m.bias, outs=OUTS)
    return gemm.linear_a6w4_gelu_dual(a, sa, fmt, m.w_codes, m.w_scales, m.bias)


def _qkv(gemm, fmt, a, sa, m, bias, cache, seq, hs):
    if fmt == "e2m1":
        return gemm.linear_fp4_qkv_to_cache(a, sa, m.w_codes, m.w_scales, bias, cache, POS, seq, hs)
    return gemm.linear_a6w4_qkv_to_cache(a, sa, fmt, m.w_codes, m.w_scales, bias, cache, POS, seq, hs)


def _cache(bsz, seq):
    return torch.full((2, bsz, POS + seq + 1, HEADS, 64), 7.0, dtype=torch.float16, device=_dev())


def _assert_slots(cache, y, bsz, seq, what, parts=(1, 2)):
    """the cache's slots POS .. POS + seq hold the k / v slices of y [B, seq, 3C]; every other slot is untouched"""
    y5 = y.view(bsz, seq, 3, HEADS, 64)
    for p in parts:
        assert_bits_equal(cache[p - 1][:, POS:POS + seq], y5[:, :, p], f"{what}: part {p}")
    assert bool((cache[:, :, :POS] == 7.0).all()) and bool((cache[:, :, POS + seq:] == 7.0).all()), f"{what}: a slot outside the step was written"


@pytest.mark.parametrize("binding", ("as built", "ctypes"))
@pytest.mark.parametrize("km", (False, True), ids=("row-major", "k-major"))
@pytest.mark.parametrize("fmt", tuple(ACT))
def test_modules_reach_the_kernels_of_their_format(fmt, km, binding, monkeypatch):
    from fpqvar_amd import gemm
    if binding == "ctypes":
        monkeypatch.setattr(gemm, "_native", None)
    m, f, nb = _modules(fmt, km)
    for bsz, seq in BATCHES:
        what = f"{fmt} {'k-major' if km else 'row-major'} {binding} B {bsz} L {seq}"
        x, gate, res, bias32, hs = _inputs(bsz, seq)
        quantize = gemm.quantize_mx if fmt == "e2m1" else functools.partial(gemm.quantize_g6, table=fmt)
        a, sa = quantize(x.view(-1, K), kmajor=km)
        # forward and forward_operands against the public function on operands quantized by hand
        y, y_tail = m(x), m(x, gate, res)
        assert y.shape == (bsz, seq, OUTS)
        assert_bits_equal(y.view(-1, OUTS), _plain(gemm, fmt, km, a, sa, m), f"{what}: forward")
        assert_bits_equal(y_tail.view(-1, OUTS), _plain(gemm, fmt, km, a, sa, m, gate, res), f"{what}: forward with gate and residual")
        assert_bits_equal(m.forward_operands(a, sa), y.view(-1, OUTS), f"{what}: forward_operands")
        assert_bits_equal(m.forward_operands(a, sa, gate, res, table=ACT[fmt]), y_tail.view(-1, OUTS), f"{what}: forward_operands with the tail")
        z = f(x)
        assert_bits_equal(z.view(-1, OUTS), _fc1(gemm, fmt, km, a, sa, f), f"{what}: fc1 forward")
        assert_bits_equal(f.forward_operands(a, sa), z.view(-1, OUTS), f"{what}: fc1 forward_operands")
        if km:   # the k-major module against the row-major one
            m_rm, f_rm, _ = _modules(fmt, False)
            assert_bits_equal(y, m_rm(x), f"{what}: forward against the row-major module")
            assert_bits_equal(z, f_rm(x), f"{what}: fc1 against the row-major module")
        # mat_qkv into the cache: q and the slots are the slices of forward(x)
        cache = _cache(bsz, seq)
        q = m.qkv_to_cache(x, cache, POS, seq)
        assert_bits_equal(q, y.view(bsz, seq, 3, HEADS * 64)[:, :, 0].contiguous(), f"{what}: q")
        _assert_slots(cache, y, bsz, seq, what)
        # with the q / k norm, on the module without bias: the public function by hand; v is the slice of that module's forward
        cache_m, cache_h = _cache(bsz, seq), _cache(bsz, seq)
        q_m = nb.qkv_to_cache(x, cache_m, POS, seq, hs, bias32)
        q_h = _qkv(gemm, fmt, a, sa, nb, bias32, cache_h, seq, hs)
        assert_bits_equal(q_m, q_h, f"{what}: q of the norm form")
        assert_bits_equal(cache_m, cache_h, f"{what}: the cache of the norm form")
        cache_v = _cache(bsz, seq)
        nb.qkv_to_cache(x, cache_v, POS, seq, hs)
        _assert_slots(cache_v, nb(x), bsz, seq, f"{what}: norm form without bias", parts=(2,))
    torch.cuda.synchronize()
