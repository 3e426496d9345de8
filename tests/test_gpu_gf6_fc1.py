"""The fc1 tail with its dual pair as an argument (fpq_gemm_a6w4_gelu_dual_pair / fpq_gemm_w6_gelu_dual_pair, gemm.linear_g6_gelu_dual)
and the modules built on the GF6 Linears (gemm.FP6GroupLinear, FP6GroupLinearGeluDual, quant_linear.quantize_VAR(group_fp6=True)).

The 4-bit pair (E1M2-, E2M1+) must be the existing entry points bit for bit; the 6-bit pair (INT-, E2M3+: fc2's per-group input
format of the 6-bit configuration) must be `fp6_quant_int_neg_e2m3_pos_per_group_cuda(gelu_tanh(y), 6, 128)` bit for bit, y the
plain form's fp16 output: h == table[bits(y)] with the GELU table of tests/test_gpu_a6w4_fc1.py (all 65 536 patterns through
linear_fp4_gelu_dual), q == the stand-alone quantizer and the oracle on h - groups holding NaN, +inf and -inf included, since this
format has no global clamp and a NaN stays in its group.

Shapes: tokens 1, 17, 65, 130, outs 128, 384, K 128, 384, 1920 (tests/test_gpu_gf6.py)."""
import copy

import pytest
import torch

from oracle import fpq_oracle as orc
from tests import gemm_model as gm
from tests import gf6_model as fm
from tests.conftest import assert_bits_equal
from tests.test_a6w4_host import _Var
from tests.test_gpu_a6w4_fc1 import _lookup, fp4_tail, gelu_table  # noqa: F401  (module-scoped fixtures: the GELU, tabulated)
from tests.test_gpu_gf6 import _images, _quantize

pytestmark = pytest.mark.gpu

CFGS = (20, 30)
FC1_PAIRS = (("e2m3", "e2m1"), ("e2m3", "e2m3"), ("e2m1", "e3m2"))      # the A6W4 family; the W6 family with a 6-bit and a 4-bit activation
SHAPES = [(T, K, O) for T in (1, 17, 65, 130) for K, O in ((128, 128), (384, 384), (1920, 128))] + [(130, 1920, 384), (17, 128, 384)]
DECODE_NAME = {"e2m3": "e1m2", "e3m2": "e3m0", "e2m1": "e2m1", "e1m2": "e1m2", "e3m0": "e3m0"}


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "these tests need the GPU"
    return torch.device("cuda:0")


def _operands(dev, pair, T, K, O, seed, special=False):
    from fpqvar_amd import gemm
    g = torch.Generator().manual_seed(seed)
    x = (torch.randn(T, K, generator=g) * torch.exp(0.3 * torch.randn(T, K, generator=g))).half().to(dev)
    w = (torch.randn(O, K, generator=g) * 0.05).to(dev)
    bias = (torch.randn(O, generator=g) * 0.3).half()
    if special:   # a NaN in group 0 and, where there are three groups, +inf in group 1 and -inf in group 2 (a -inf Linear output: NaN)
        bias[77] = float("nan")
        if O >= 384:
            bias[130], bias[300] = float("inf"), float("-inf")
    return _quantize(gemm, pair[0], x), _quantize(gemm, pair[1], w), bias.to(dev)


@pytest.mark.parametrize("T,K,O", SHAPES)
@pytest.mark.parametrize("pair", FC1_PAIRS, ids=lambda p: "-".join(p))
def test_4bit_pair_is_the_existing_entry_point(dev, pair, T, K, O, lib_options):
    """fc2_pair (E1M2-, E2M1+) through fpq_gemm_*_gelu_dual_pair == the existing entry points (linear_a6w4_gelu_dual /
    linear_w6_gelu_dual: fpq_gemm_a6w4_gelu_dual, fpq_gemm_w6_gelu_dual) on the same codes, named by their decode format: q and
    gelu_out, both tilings and both layouts, a NaN row included (the global clamp's rule: everything zero)"""
    from fpqvar_amd import gemm
    at, wt = pair
    for special in (False, True):
        a, w, bias = _operands(dev, pair, T, K, O, 3 + T, special)
        case = dict(a=a[0], a_scales=a[1], w=w[0], w_scales=w[1])
        km = _images(gemm, pair, case)
        for cfg in CFGS:
            lib_options("FPQ_GEMM_CFG", cfg)
            if wt == "e2m1":
                want = gemm.linear_a6w4_gelu_dual(*a, DECODE_NAME[at], *w, bias, return_gelu=True)
            else:
                want = gemm.linear_w6_gelu_dual(*a, DECODE_NAME[at], *w, DECODE_NAME[wt], bias, return_gelu=True)
            for layout, ops_ in (("rows", (*a, at, *w, wt)), ("k-major", (km[0], km[1], at, km[2], km[3], wt))):
                q, h = gemm.linear_g6_gelu_dual(*ops_, bias, fc2_pair=("e1m2_neg", "e2m1_pos"), return_gelu=True)
                what = f"{pair} [{T} x {K} -> {O}] cfg {cfg} {layout} special {special}"
                assert_bits_equal(q, want[0], what + ": q")
                assert_bits_equal(h, want[1], what + ": gelu_out")
                assert bool(q.any()) != special, what


@pytest.mark.parametrize("T,K,O", SHAPES)
@pytest.mark.parametrize("pair", FC1_PAIRS, ids=lambda p: "-".join(p))
def test_6bit_pair_is_gemm_gelu_quantizer(dev, pair, T, K, O, gelu_table, lib_options):  # noqa: F811
    """fc2_pair (INT-, E2M3+): h == table[bits(linear_g6(...))], q == the stand-alone quantizer on h (ops, quant_utils) and the
    oracle, with and without gelu_out, both tilings and both layouts; groups with NaN / +inf / -inf keep to themselves"""
    from fpqvar_amd import gemm, ops, quant_utils as qu
    at, wt = pair
    for special in (False, True):
        a, w, bias = _operands(dev, pair, T, K, O, 11 + T, special)
        case = dict(a=a[0], a_scales=a[1], w=w[0], w_scales=w[1])
        km = _images(gemm, pair, case)
        first = None
        for cfg in CFGS:
            lib_options("FPQ_GEMM_CFG", cfg)
            y = gemm.linear_g6(*a, at, *w, wt, bias)
            for layout, ops_ in (("rows", (*a, at, *w, wt)), ("k-major", (km[0], km[1], at, km[2], km[3], wt))):
                what = f"{pair} [{T} x {K} -> {O}] cfg {cfg} {layout} special {special}"
                q, h = gemm.linear_g6_gelu_dual(*ops_, bias, return_gelu=True)
                assert q.shape == h.shape == (T, O) and q.dtype == h.dtype == torch.float16
                assert_bits_equal(h, _lookup(gelu_table, y), what + ": h == table[bits(y)]")
                assert_bits_equal(q, ops.quant_rows_dual(h, "int_neg", "e2m3_pos", 128, None), what + ": vs ops.quant_rows_dual")
                assert_bits_equal(q, qu.fp6_quant_int_neg_e2m3_pos_per_group_cuda(h, 6, 128), what + ": vs quant_utils")
                assert_bits_equal(q.cpu(), orc.dual_per_group_kernel_sem(h.cpu(), "int_neg", "e2m3_pos", 128, None), what + ": vs oracle")
                assert_bits_equal(gemm.linear_g6_gelu_dual(*ops_, bias), q, what + ": without the GELU output")
                if special:   # the NaN stays out of its group's maxima: the group's other values are quantized as ever
                    assert bool(torch.isnan(h[:, 77]).all())
                    keep = torch.ones(128, dtype=torch.bool, device=dev)
                    keep[77] = False
                    assert bool(torch.isfinite(q[:, :128][:, keep]).all()) and bool(q[:, :128][:, keep].any())
                    if O >= 384:   # +inf: its side's scale is infinite and the whole group NaN; -inf: gelu gives NaN, as above
                        assert bool(torch.isinf(h[:, 130]).all()) and bool(torch.isnan(q[:, 128:256]).all())
                else:
                    assert bool(q.any()) and not bool(torch.isnan(q).any())
                first = q if first is None else first
                assert_bits_equal(q, first, what + ": tilings / layouts")
    torch.cuda.synchronize()
    assert not bool(ops._nan_scratch(dev).any()), "this pair raises no flag"


# ------------------------------------------------------------------------------------------------------------ the modules
W6A6 = dict(weight_quant="per_group", act_quant="per_group", w_bit=6, a_bit=6, activation_fp_quant=True, weight_fp_quant=True,
            act_fp_type="fp6_e2m3", weight_fp_type="fp6_e2m3", fc2_fp_type="fp6_int_neg_e2m3_pos")


@pytest.mark.parametrize("kmajor", (False, True), ids=("rows", "kmajor"))
@pytest.mark.parametrize("pair", (("e2m3", "e2m3"), ("e3m2", "e2m1"), ("e2m1", "e2m3")), ids=lambda p: "-".join(p))
def test_fp6grouplinear(dev, pair, kmajor):
    """from_float holds the weight quantizer's operands; forward == the activation's quantizer + linear_g6 bit for bit, tail and
    qkv_to_cache included, row-major and k-major the same bits; the fused module == linear_g6_gelu_dual.  [5 x 13 = 65 tokens, K = 384]"""
    from fpqvar_amd import gemm
    name = {"e2m3": "fp6_e2m3", "e3m2": "fp6_e3m2", "e2m1": "fp_e2"}
    at, wt = pair
    K, O, B, L = 384, 384, 5, 13
    g = torch.Generator().manual_seed(7)
    lin = torch.nn.Linear(K, O)
    with torch.no_grad():
        lin.weight.copy_(torch.randn(O, K, generator=g) * 0.05)
        lin.bias.copy_(torch.randn(O, generator=g) * 0.1)
    lin = lin.to(dev)
    m = gemm.FP6GroupLinear.from_float(lin, name[wt], name[at], kmajor=kmajor).half()
    wc, wsc = _quantize(gemm, wt, lin.weight.detach().float())
    assert (m.act_table, m.w_table) == pair and m.kmajor == kmajor and m.w_scales.dtype == torch.float32
    if not kmajor:
        assert torch.equal(m.w_codes, wc) and torch.equal(m.w_scales, wsc)
    x = torch.randn(B, L, K, generator=g).half().to(dev)
    y = m(x)
    ac, asc = _quantize(gemm, at, x.view(-1, K))
    want = gemm.linear_g6(ac, asc, at, wc, wsc, wt, m.bias)
    assert y.shape == (B, L, O)
    assert_bits_equal(y.view(-1, O), want, "forward")
    assert_bits_equal(m.forward_operands(*_quantize(gemm, at, x.view(-1, K), kmajor=kmajor)), want, "forward_operands")
    gate, resid = torch.randn(B, 1, O, generator=g).half().to(dev), torch.randn(B, L, O, generator=g).half().to(dev)
    assert_bits_equal(m(x, gate=gate, residual=resid), resid + y * gate, "gate / residual")
    f = gemm.FP6GroupLinearGeluDual.from_float(lin, name[wt], name[at], kmajor=kmajor).half()
    assert f.fc2_pair == ("int_neg", "e2m3_pos")
    assert_bits_equal(f(x).view(-1, O), gemm.linear_g6_gelu_dual(ac, asc, at, wc, wsc, wt, f.bias), "the fused module")
    # mat_qkv: C = 128
    m.bias = None
    cache = torch.zeros(2, B, L + 5, 2, 64, dtype=torch.float16, device=dev)
    q = m.qkv_to_cache(x, cache, 3, L)
    qkv = gemm.linear_g6(ac, asc, at, wc, wsc, wt, None).view(B, L, 3, 128)
    assert_bits_equal(q, qkv[:, :, 0].contiguous(), "q")
    assert_bits_equal(cache[0, :, 3:3 + L].reshape(B, L, 128), qkv[:, :, 1].contiguous(), "k")
    assert_bits_equal(cache[1, :, 3:3 + L].reshape(B, L, 128), qkv[:, :, 2].contiguous(), "v")


def test_group_fp6_model_on_the_matrix_cores(dev):
    """Toy VARs of three blocks (C = 256, 150 tokens: the toy model of the host tests) converted with group_fp6=True, fuse_ffn=True.
    W6A6 with fc2's 6-bit dual pair, and W6A4 (E3M0 x E2M3) with the 4-bit one: it runs, fc1 is an FP6GroupLinearGeluDual whose
    output equals the unfused twin's - FP6GroupLinear, then GeluThenFc2Quant - bit for bit, row-major and k-major; and each
    matrix-core layer's output is close to the fake-quant layer's.

    The bound, stated before any run: the fake-quant layer multiplies the same de-quantized operands with torch's fp16 GEMM, so
    |y_fake - r| <= lim = gm.bound(r) (r: the exact product of those operands) + 2^-10 sum|a_k w_k| (the fp16 GEMM's accumulation, as
    tests/test_gpu_w6.py allows it) + 2^-10 |r| (its fp16 output rounding, with margin); the matrix-core layer is within gm.bound(r)
    of r, hence the two within 2 lim of each other."""
    from fpqvar_amd import gemm, quant_linear as ql
    C = 256
    torch.manual_seed(11)
    base = _Var(C, 3)
    for b in base.blocks:
        b.ffn.act = torch.nn.GELU(approximate="tanh")
    base = base.to(dev)
    x = torch.randn(3, 50, C, device=dev).half()
    w6a4 = dict(W6A6, a_bit=4, act_fp_type="fp_e3", fc2_fp_type="fp_e1m2_neg_e2m1_pos")
    for cfg, fc2, bits, pair in ((W6A6, "fp6_int_neg_e2m3_pos", 6, ("int_neg", "e2m3_pos")), (w6a4, "fp_e1m2_neg_e2m1_pos", 4, ("e1m2_neg", "e2m1_pos"))):
        for km in (False, True):
            fused = ql.quantize_VAR(copy.deepcopy(base), group_fp6=True, fuse_ffn=True, kmajor_operands=km, **cfg).half()
            twin = ql.quantize_VAR(copy.deepcopy(base), group_fp6=True, kmajor_operands=km, **cfg).half()
            for b in range(3):
                fb, tb = fused.blocks[b], twin.blocks[b]
                assert type(fb.ffn.fc1) is gemm.FP6GroupLinearGeluDual and type(tb.ffn.fc1) is gemm.FP6GroupLinear
                assert fb.ffn.fc1.kmajor == km and fb.ffn.fc1.fc2_pair == pair
                assert isinstance(fb.ffn.act, torch.nn.Identity) and fb.ffn.fc2.act_quant_name == "in fc1's epilogue"
                q_fused = fb.ffn.fc1(x)
                q_twin = ql.GeluThenFc2Quant("per_group", fc2, bits)(tb.ffn.fc1(x))
                assert bool(q_fused.any())
                assert_bits_equal(q_fused, q_twin, f"{fc2} block {b} kmajor {km}: the fused fc1 tail vs GeluThenFc2Quant")
                out = fb.ffn.fc2(fb.ffn.act(q_fused))              # the FFN as the reference's forward runs it
                assert_bits_equal(out, fb.ffn.fc2(q_twin), f"block {b}: the FFN output")
                assert out.shape == (3, 50, C) and bool(torch.isfinite(out).all())
    fake = ql.quantize_VAR(copy.deepcopy(base), **W6A6).half()
    real = ql.quantize_VAR(copy.deepcopy(base), group_fp6=True, **W6A6).half()
    for b in range(3):
        for path in ("ffn.fc1", "attn.mat_qkv", "attn.proj"):
            mr, mf = real.blocks[b].get_submodule(path), fake.blocks[b].get_submodule(path)
            assert type(mr) is gemm.FP6GroupLinear and type(mf) is ql.QuantizedLinear
            y_real, y_fake = mr(x).view(-1, mr.out_features), mf(x).view(-1, mr.out_features)
            ac, asc = gemm.quantize_gf6(x.view(-1, C), "e2m3")
            wc, wsc = gemm.quantize_gf6(base.blocks[b].get_submodule(path).weight.detach().float(), "e2m3")
            r = fm.reference("e2m3", "e2m3", ac, asc, wc, wsc, mr.bias)
            assert gm.ratio(y_real, r) <= 1.0, (b, path)
            a64, w64 = gemm.dequantize_gf6(ac, asc, "e2m3").double(), gemm.dequantize_gf6(wc, wsc, "e2m3").double()
            lim = gm.bound(r) + 2.0 ** -10 * (a64.abs() @ w64.abs().t()) + 2.0 ** -10 * r.out.abs()
            assert bool(((y_fake.double() - r.out).abs() <= lim).all()), (b, path)
            assert bool(((y_real.double() - y_fake.double()).abs() <= 2 * lim).all()), (b, path)
