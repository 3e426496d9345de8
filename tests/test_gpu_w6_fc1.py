"""The fc1 tail in the W6 GEMM on the GPU (fpq_gemm_w6_gelu_dual, gemm.linear_w6_gelu_dual): GELU(tanh) and fc2's dual E1M2- / E2M1+
per-group quantizer as the epilogue of the GEMM that takes E1M2 / E3M0 WEIGHTS as 6-bit codes, for all six (activation, weight)
pairs - after tests/test_gpu_a6w4_fc1.py.

The tail is the FP4 GEMM's (FPQ_GEMM_FC1_TAIL, one text for the three kernels), and its GELU is a pure function of the fp16 Linear
output - so it is TABULATED: all 65536 fp16 patterns through linear_fp4_gelu_dual, whose GELU tests/test_gpu_fc1_fused.py pins to
torch's.  Everything here is then exact: h == table[bits(y)] with y the plain W6 GEMM's output, q == the stand-alone dual quantizer
and the oracle on h, and - on weights whose levels both tables hold - the whole launch == the E2M1-weight kernels', bit for bit."""
import copy

import pytest
import torch

from oracle import fpq_oracle as orc
from tests import w6_model as wm
from tests.conftest import assert_bits_equal
from tests.test_gpu_a6w4 import _Var

pytestmark = pytest.mark.gpu

PAIRS = wm.PAIRS
IDS = [f"{a}-{w}" for a, w in PAIRS]
CFGS = (20, 30, None)    # FPQ_GEMM_CFG: 128 x 128 tiles, 64 x 128 tiles, the library's choice
# (T, K, O): G = 1 - the idle stage was never filled; even G, ragged rows, three column tiles - the XCD column rounding is live;
# odd G, a second row tile with one live row; the models' K (d30, d36) and LDS sizes
SHAPES = ((1, 128, 128), (63, 256, 384), (129, 384, 256), (300, 1920, 512), (70, 2304, 1152))
FP_NAME = {"e2m1": "fp_e2", "e1m2": "fp_e1", "e3m0": "fp_e3"}
# the levels a weight table shares with E2M1
COMMON = {"e1m2": (0.0, 0.5, 1.0, 1.5), "e3m0": (0.0, 0.5, 1.0, 2.0, 4.0)}


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "these tests need the GPU"
    return torch.device("cuda:0")


def _every(dev):
    return torch.arange(0, 65536, dtype=torch.int32).to(torch.int16).view(torch.float16).to(dev)


@pytest.fixture(scope="module")
def fp4_tail(dev):
    """(q, h) of linear_fp4_gelu_dual on T = 4, K = 128, O = 65536, zero activation codes, unit scales, bias = every fp16 pattern
    (the construction of test_fused_fc1_gelu_on_every_fp16_input): h[0] is the GELU table, indexed by the pattern of y."""
    from fpqvar_amd import gemm
    K, O = 128, 65536
    a = (torch.zeros(4, K // 2, dtype=torch.uint8, device=dev), torch.ones(4, 1, dtype=torch.float16, device=dev))
    w = (torch.zeros(O, K // 2, dtype=torch.uint8, device=dev), torch.ones(O, 1, dtype=torch.float32, device=dev))
    q, h = gemm.linear_fp4_gelu_dual(*a, *w, _every(dev), return_gelu=True)
    return q, h


@pytest.fixture(scope="module")
def gelu_table(fp4_tail):
    return fp4_tail[1][0].clone()


def _lookup(table, y):
    return table[(y.view(torch.int16).to(torch.int32) & 0xFFFF).long()]


def _dual(h):
    from fpqvar_amd import ops
    return ops.quant_rows_dual(h, "e1m2_neg", "e2m1_pos", 128, 1.0)


def _quantize_a(a_table, x):
    from fpqvar_amd import gemm
    return gemm.quantize_mx(x) if a_table == "e2m1" else gemm.quantize_g6(x, a_table)


def operands(dev, pair, T, K, O, seed):
    """activation through quantize_mx / quantize_g6, weight through quantize_g6(w.float(), w_table)"""
    from fpqvar_amd import gemm
    g = torch.Generator().manual_seed(seed)
    x = (torch.randn(T, K, generator=g) * torch.exp(0.3 * torch.randn(T, K, generator=g))).half().to(dev)
    w = (torch.randn(O, K, generator=g) * 0.05).to(dev)
    bias = (torch.randn(O, generator=g) * 0.3).half().to(dev)
    return _quantize_a(pair[0], x), gemm.quantize_g6(w.float(), pair[1]), bias


# ------------------------------------------------------------------------------------------------------------ 1. the GELU, tabulated
@pytest.mark.parametrize("pair", PAIRS, ids=IDS)
def test_the_tail_is_the_fp4_kernels_on_every_fp16_input(dev, pair, fp4_tail, gelu_table, lib_options):
    """All 65536 fp16 patterns as the Linear output (zero codes on both sides, the pattern as the bias of its own column): h and q of
    the W6 fused launch equal linear_fp4_gelu_dual's bit for bit, in every tiling - that comparison pins the GELU.  The patterns
    include the NaNs, so q is every-bit zero on both sides: its comparison checks the NaN rule, not quantized values."""
    from fpqvar_amd import gemm, ops
    a_table, w_table = pair
    K, O = 128, 65536
    every = _every(dev)
    a = (torch.zeros(4, wm.SEG[a_table], dtype=torch.uint8, device=dev), torch.ones(4, 1, dtype=torch.float16, device=dev))
    w = (torch.zeros(O, 96, dtype=torch.uint8, device=dev), torch.ones(O, 1, dtype=torch.float32, device=dev))
    q4, h4 = fp4_tail
    for cfg in CFGS:
        lib_options("FPQ_GEMM_CFG", cfg)
        y = gemm.linear_w6(*a, a_table, *w, w_table, every)
        assert_bits_equal(y[0], torch.where(every == 0, torch.zeros_like(every), every), "the Linear output is the bias (0 + -0 = +0)")
        q, h = gemm.linear_w6_gelu_dual(*a, a_table, *w, w_table, every, return_gelu=True)
        assert_bits_equal(h, h4, f"{pair} cfg {cfg}: GELU values vs the FP4 kernel's")
        assert_bits_equal(q, q4, f"{pair} cfg {cfg}: quantized values vs the FP4 kernel's")
        assert bool(torch.isnan(h).any()) and q.view(torch.int16).abs().max().item() == 0     # the NaN rule: every output +0
        assert_bits_equal(h, _lookup(gelu_table, y), f"{pair} cfg {cfg}: h == table[bits(y)]")
    torch.cuda.synchronize()
    assert not bool(ops._nan_scratch(dev).any())


# ------------------------------------------------------------------------------------------------------------ 2. fused = GEMM -> GELU -> quantizer
@pytest.mark.parametrize("T,K,O", SHAPES)
@pytest.mark.parametrize("pair", PAIRS, ids=IDS)
def test_fused_equals_gemm_gelu_quantizer(dev, pair, T, K, O, gelu_table, lib_options):
    """With y = linear_w6(...): h == table[bits(y)] exactly (the epilogue sees the plain GEMM's output and applies the same GELU), q
    bit-equal to the stand-alone dual quantizer on h and to the oracle's, the form without the GELU output the same q; every tiling,
    bias and no bias.  T = 63 / 129: the padding rows of the last tile raise no flag (a raised flag would zero q)."""
    from fpqvar_amd import gemm
    a_table, w_table = pair
    a, w, bias = operands(dev, pair, T, K, O, 11 + T)
    for cfg in CFGS:
        lib_options("FPQ_GEMM_CFG", cfg)
        for b in (bias, None):
            what = f"{pair} [{T} x {K} -> {O}] cfg {cfg} bias {b is not None}"
            y = gemm.linear_w6(*a, a_table, *w, w_table, b)
            q, h = gemm.linear_w6_gelu_dual(*a, a_table, *w, w_table, b, return_gelu=True)
            assert q.shape == h.shape == (T, O) and q.dtype == h.dtype == torch.float16
            assert_bits_equal(h, _lookup(gelu_table, y), f"{what}: h == table[bits(y)]")
            assert bool(q.any()), what
            assert_bits_equal(q, _dual(h), f"{what}: fused vs the stand-alone quantizer on the emitted GELU values")
            assert_bits_equal(q.cpu(), orc.dual_per_group_kernel_sem(h.cpu(), "e1m2_neg", "e2m1_pos", 128, 1.0), f"{what}: fused vs oracle")
            assert_bits_equal(gemm.linear_w6_gelu_dual(*a, a_table, *w, w_table, b), q, f"{what}: without the GELU output")


# ------------------------------------------------------------------------------------------------------------ 3. against the E2M1-weight kernels
def common_level_weight(dev, w_table, O, K, seed):
    """a weight whose levels both `w_table` and E2M1 hold, random fp32 group scales -> (6-bit codes of w_table, E2M1 nibbles, scales):
    the same numbers in both forms"""
    g = torch.Generator().manual_seed(seed)
    lv = torch.tensor(COMMON[w_table], dtype=torch.float64)
    assert set(COMMON[w_table]) == set(wm.LEVELS[w_table]) & set(wm.LEVELS["e2m1"])
    L = lv[torch.randint(0, len(lv), (O, K), generator=g)] * torch.where(torch.rand(O, K, generator=g) < 0.5, -1.0, 1.0).double()
    scales = (torch.rand(O, K // 128, generator=g) * 0.05 + 0.005).float()
    L = L.to(dev)
    return wm.encode_levels(w_table, L), wm.encode_levels("e2m1", L), scales.to(dev)


@pytest.mark.parametrize("T,K,O", ((63, 256, 384), (129, 384, 256)))
@pytest.mark.parametrize("pair", PAIRS, ids=IDS)
def test_common_levels_equal_the_e2m1_weight_kernels(dev, pair, T, K, O, lib_options):
    """The dots are exact and the fp32 steps identical, so on the same activation codes a weight of common levels gives the bits of
    the E2M1-weight kernels: linear_w6 == linear_fp4 / linear_a6w4, linear_w6_gelu_dual == linear_fp4_gelu_dual /
    linear_a6w4_gelu_dual (h and q)"""
    from fpqvar_amd import gemm
    a_table, w_table = pair
    a, _, bias = operands(dev, pair, T, K, O, 31 + T)
    w6, w4, sw = common_level_weight(dev, w_table, O, K, 5 + T)
    if a_table == "e2m1":
        y4 = gemm.linear_fp4(*a, w4, sw, bias)
        q4, h4 = gemm.linear_fp4_gelu_dual(*a, w4, sw, bias, return_gelu=True)
    else:
        y4 = gemm.linear_a6w4(*a, a_table, w4, sw, bias)
        q4, h4 = gemm.linear_a6w4_gelu_dual(*a, a_table, w4, sw, bias, return_gelu=True)
    assert bool(q4.any())
    for cfg in CFGS:
        lib_options("FPQ_GEMM_CFG", cfg)
        what = f"{pair} [{T} x {K} -> {O}] cfg {cfg}"
        assert_bits_equal(gemm.linear_w6(*a, a_table, w6, sw, w_table, bias), y4, f"{what}: plain vs the E2M1-weight kernel")
        q, h = gemm.linear_w6_gelu_dual(*a, a_table, w6, sw, w_table, bias, return_gelu=True)
        assert_bits_equal(h, h4, f"{what}: GELU values vs the E2M1-weight kernel")
        assert_bits_equal(q, q4, f"{what}: quantized values vs the E2M1-weight kernel")


# ------------------------------------------------------------------------------------------------------------ 4. the NaN rule
@pytest.mark.parametrize("pair", (("e2m1", "e3m0"), ("e3m0", "e1m2")), ids=("e2m1-e3m0", "e3m0-e1m2"))
def test_nan_rule_and_scratch(dev, pair):
    """One NaN in the GELU tensor (a NaN bias): every output bit zero, the 8-byte scratch zero again afterwards, the next clean call
    clean; one captured graph (a single stream, no parallel branches) replayed NaN, NaN, clean on static buffers."""
    from fpqvar_amd import gemm, ops
    a_table, w_table = pair
    a, w, bias = operands(dev, pair, 200, 256, 256, 5)
    run = lambda b: gemm.linear_w6_gelu_dual(*a, a_table, *w, w_table, b)
    clean = run(bias)
    assert bool(clean.any())
    bad = bias.clone()
    bad[77] = float("nan")
    z = run(bad)
    assert not bool(z.view(torch.int16).any())
    scratch = ops._nan_scratch(dev)
    torch.cuda.synchronize()
    assert not bool(scratch.any()), "the NaN scratch must be zero again after the fix-up launch"
    assert_bits_equal(run(bias), clean, "after a NaN call")
    sb = bad.clone()
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        run(sb)
        gr = torch.cuda.CUDAGraph()
        with torch.cuda.graph(gr, stream=s):
            out = run(sb)
    torch.cuda.current_stream().wait_stream(s)
    for _ in range(2):
        gr.replay()
        torch.cuda.synchronize()
        assert not bool(out.view(torch.int16).any())
    sb.copy_(bias)
    gr.replay()
    torch.cuda.synchronize()
    assert_bits_equal(out, clean, "graph replay without the NaN")


# ------------------------------------------------------------------------------------------------------------ 5. argument checks
def test_argument_checks_on_the_gpu(dev):
    from fpqvar_amd import gemm
    a, w, bias = operands(dev, ("e3m0", "e1m2"), 8, 128, 128, 1)
    fn = gemm.linear_w6_gelu_dual
    with pytest.raises(RuntimeError):
        fn(*a, "e3m0", w[0][:120], w[1][:120], "e1m2")                         # outs % 128 != 0
    with pytest.raises(RuntimeError):
        fn(a[0][:, :-8], a[1], "e3m0", *w, "e1m2")                              # truncated operand
    with pytest.raises(RuntimeError):
        fn(a[0].view(1, 8, 96), a[1], "e3m0", w[0].view(1, 128, 96), w[1], "e1m2")   # images: the W6 GEMM has no k-major form
    with pytest.raises(RuntimeError):
        fn(*a, "e3m0", w[0], w[1].half(), "e1m2")                               # fp16 weight scales: not compiled
    with pytest.raises(RuntimeError):
        fn(*a, "e3m0", *w, "e2m1")                                              # an E2M1 weight table
    assert fn(a[0][:0], a[1][:0], "e3m0", *w, "e1m2").shape == (0, 128)
    q, h = fn(a[0][:0], a[1][:0], "e3m0", *w, "e1m2", return_gelu=True)
    assert q.shape == h.shape == (0, 128)


# ------------------------------------------------------------------------------------------------------------ 6. the module
@pytest.mark.parametrize("pair", PAIRS, ids=IDS)
def test_fp4linear_gelu_dual_with_a_6bit_weight(dev, pair, gelu_table):
    """FP4LinearGeluDual.from_float(..., weight_fp_type=w, w6_forms=True): forward(x) == the three-step chain on the plain module of
    the same weight (its Linear output -> the tabulated GELU -> the stand-alone dual quantizer); forward_operands == forward"""
    from fpqvar_amd import gemm
    a_table, w_table = pair
    g = torch.Generator().manual_seed(7)
    lin = torch.nn.Linear(256, 384)
    with torch.no_grad():
        lin.weight.copy_(torch.randn(384, 256, generator=g) * 0.05)
        lin.bias.copy_(torch.randn(384, generator=g) * 0.1)
    lin = lin.to(dev)
    kw = dict(act_fp_type=FP_NAME[a_table], weight_fp_type=FP_NAME[w_table])
    m = gemm.FP4LinearGeluDual.from_float(lin, w6_forms=True, **kw)
    plain = gemm.FP4Linear.from_float(lin, **kw)
    assert (m.act_table, m.w_table, m.w6_forms, m.kmajor) == (a_table, w_table, True, False) and not plain.w6_forms
    assert torch.equal(m.w_codes, plain.w_codes) and torch.equal(m.w_scales, plain.w_scales)
    x = torch.randn(2, 35, 256, generator=g).half().to(dev)
    y = m(x)
    assert y.shape == (2, 35, 384) and bool(y.any())
    want = _dual(_lookup(gelu_table, plain(x).view(-1, 384)))
    assert_bits_equal(y.view(-1, 384), want, "forward vs GEMM -> GELU -> quantizer")
    ac, asc = _quantize_a(a_table, x.view(-1, 256))
    assert_bits_equal(m.forward_operands(ac, asc), want, "forward_operands")
    assert_bits_equal(gemm.linear_w6_gelu_dual(ac, asc, a_table, m.w_codes, m.w_scales, w_table, m.bias), want, "the function-level call")
    with pytest.raises(ValueError):
        gemm.FP4LinearGeluDual.from_float(lin, **kw)                          # the default is what it was
    with pytest.raises(ValueError):
        gemm.FP4LinearGeluDual.from_float(lin, kmajor=True, w6_forms=True, **kw)


# ------------------------------------------------------------------------------------------------------------ 7. a small mixed model
def test_mixed_model_fuses_the_ffn_of_6bit_weight_layers(dev):
    """A toy VAR at C = 256, three blocks whose fc1 covers the three activation formats with 6-bit weights, converted with
    w6_weights=True, fuse_ffn=True: with w6_forms=True every FFN runs fc1's GELU and fc2's quantizer in the W6 GEMM's epilogue, with
    w6_forms=False the GeluThenFc2Quant route.  That route's GELU is the kernels' own gelu_tanh_fast (quant_utils.
    gelu_fp_quant_e1m2_neg_e2m1_pos_per_group_cuda -> ops.gelu_quant_rows_dual, fpq_fast16.h), the one FPQ_GEMM_FC1_TAIL applies, so
    the two models agree bit for bit: fc2's input and every FFN's output."""
    from fpqvar_amd import gemm, quant_linear as ql
    C = 256
    torch.manual_seed(11)
    kw = dict(weight_quant="per_group", act_quant="per_group", w_bit=4, a_bit=4, activation_fp_quant=True, weight_fp_quant=True)
    pairs = (("fp_e2", "fp_e3"), ("fp_e1", "fp_e1"), ("fp_e3", "fp_e1"))

    def fmt(b, layer):
        return ("fp_e1m2_neg_e2m1_pos", "fp_e2") if layer == "fc2" else pairs[b]
    base = _Var(C, 3).to(dev)
    route = ql.quantize_VAR_mixed(copy.deepcopy(base), fmt, real_fp4=True, w6_weights=True, fuse_ffn=True, **kw).half()
    fused = ql.quantize_VAR_mixed(copy.deepcopy(base), fmt, real_fp4=True, w6_weights=True, w6_forms=True, fuse_ffn=True, **kw).half()
    x = torch.randn(3, 50, C, device=dev).half()
    for b in range(3):
        rf, ff = route.blocks[b].ffn, fused.blocks[b].ffn
        assert type(rf.fc1) is gemm.FP4Linear and type(rf.act) is ql.GeluThenFc2Quant and not rf.fc1.w6_forms
        assert type(ff.fc1) is gemm.FP4LinearGeluDual and ff.fc1.w6_forms and isinstance(ff.act, torch.nn.Identity)
        assert (ff.fc1.act_table, ff.fc1.w_table) == (rf.fc1.act_table, rf.fc1.w_table) and ff.fc1.w_table != "e2m1"
        assert type(ff.fc2) is ql.QuantizedLinear_fc2 and "in fc1's epilogue" in repr(ff.fc2)
        assert fused.blocks[b].attn.mat_qkv.w6_forms and not route.blocks[b].attn.mat_qkv.w6_forms
        hq = ff.fc1(x)
        assert hq.shape == (3, 50, 4 * C) and bool(hq.any())
        assert_bits_equal(hq, rf.act(rf.fc1(x)), f"block {b}: fc2's input")
        assert_bits_equal(ff(x), rf(x), f"block {b}: the FFN's output")
