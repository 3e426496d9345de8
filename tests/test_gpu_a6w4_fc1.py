"""The fc1 tail in the A6W4 GEMM on the GPU (fpq_gemm_a6w4_gelu_dual, gemm.linear_a6w4_gelu_dual): GELU(tanh) and fc2's dual
E1M2- / E2M1+ per-group quantizer as the epilogue of the GEMM that takes E1M2 / E3M0 activations as 6-bit codes.

The tail is the FP4 GEMM's (FPQ_GEMM_FC1_TAIL, one text for both kernels), and its GELU is a pure function of the fp16 Linear
output - so it is TABULATED: all 65536 fp16 patterns through linear_fp4_gelu_dual, whose GELU tests/test_gpu_fc1_fused.py pins to
torch's (<= 1 ulp, NaN where torch has NaN).  Everything here is then exact: h == table[bits(y)] with y the plain A6W4 GEMM's
output, q == the stand-alone dual quantizer and the oracle on h, bit for bit."""
import copy

import pytest
import torch

from oracle import fpq_oracle as orc
from tests.conftest import assert_bits_equal
from tests.test_gpu_a6w4 import _Var

pytestmark = pytest.mark.gpu

TABLES = ("e1m2", "e3m0")
CFGS = (20, 30, None)    # FPQ_GEMM_CFG: 128 x 128 tiles, 64 x 128 tiles, the library's choice
# (T, K, O): G = 1 - the idle stage was never filled; even G, ragged rows, three column tiles - the XCD column rounding is live;
# odd G, a second row tile with one live row; the models' K (d30, d36) and LDS sizes
SHAPES = ((1, 128, 128), (63, 256, 384), (129, 384, 256), (300, 1920, 512), (70, 2304, 1152))


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


def operands(dev, table, T, K, O, seed):
    from fpqvar_amd import gemm
    g = torch.Generator().manual_seed(seed)
    x = (torch.randn(T, K, generator=g) * torch.exp(0.3 * torch.randn(T, K, generator=g))).half().to(dev)
    w = (torch.randn(O, K, generator=g) * 0.05).to(dev)
    bias = (torch.randn(O, generator=g) * 0.3).half().to(dev)
    return gemm.quantize_g6(x, table), gemm.quantize_mx(w), bias


# ------------------------------------------------------------------------------------------------------------ 1. the GELU, tabulated
@pytest.mark.parametrize("table", TABLES)
def test_the_tail_is_the_fp4_kernels_on_every_fp16_input(dev, table, fp4_tail, gelu_table, lib_options):
    """All 65536 fp16 patterns as the Linear output (zero activation codes, the pattern as the bias of its own column): h of the
    A6W4 fused launch equals linear_fp4_gelu_dual's bit for bit, in both tilings - that comparison pins the GELU.  The patterns
    include the NaNs, so q is every-bit zero on both sides: its comparison checks the NaN rule, not quantized values (those are
    test_fused_equals_gemm_gelu_quantizer's)."""
    from fpqvar_amd import gemm
    K, O = 128, 65536
    every = _every(dev)
    a = (torch.zeros(4, K * 3 // 4, dtype=torch.uint8, device=dev), torch.ones(4, 1, dtype=torch.float16, device=dev))
    w = (torch.zeros(O, K // 2, dtype=torch.uint8, device=dev), torch.ones(O, 1, dtype=torch.float32, device=dev))
    q4, h4 = fp4_tail
    for cfg in CFGS:
        lib_options("FPQ_GEMM_CFG", cfg)
        y = gemm.linear_a6w4(*a, table, *w, every)
        assert_bits_equal(y[0], torch.where(every == 0, torch.zeros_like(every), every), "the Linear output is the bias (0 + -0 = +0)")
        q, h = gemm.linear_a6w4_gelu_dual(*a, table, *w, every, return_gelu=True)
        assert_bits_equal(h, h4, f"{table} cfg {cfg}: GELU values vs the FP4 kernel's")
        assert_bits_equal(q, q4, f"{table} cfg {cfg}: quantized values vs the FP4 kernel's")
        assert bool(torch.isnan(h).any()) and q.view(torch.int16).abs().max().item() == 0     # the NaN rule: every output +0
        assert_bits_equal(h, _lookup(gelu_table, y), f"{table} cfg {cfg}: h == table[bits(y)]")
    torch.cuda.synchronize()
    from fpqvar_amd import ops
    assert not bool(ops._nan_scratch(dev).any())


# ------------------------------------------------------------------------------------------------------------ 2. fused = GEMM -> GELU -> quantizer
@pytest.mark.parametrize("T,K,O", SHAPES)
@pytest.mark.parametrize("table", TABLES)
def test_fused_equals_gemm_gelu_quantizer(dev, table, T, K, O, gelu_table, lib_options):
    """With y = linear_a6w4(...): h == table[bits(y)] exactly (the epilogue sees the plain GEMM's output and applies the same
    GELU), q bit-equal to the stand-alone dual quantizer on h and to the oracle's, the form without the GELU output the same q;
    fp32 and fp16 weight scales, every tiling, bias and no bias.  T = 63 / 129: the padding rows of the last tile raise no flag
    (a raised flag would zero q)."""
    from fpqvar_amd import gemm
    a, (wc, ws), bias = operands(dev, table, T, K, O, 11 + T)
    for sw in (ws, ws.half()):
        assert sw.dtype == (torch.float32 if sw is ws else torch.float16)
        for cfg in CFGS:
            lib_options("FPQ_GEMM_CFG", cfg)
            for b in (bias, None):
                what = f"{table} [{T} x {K} -> {O}] sw {sw.dtype} cfg {cfg} bias {b is not None}"
                y = gemm.linear_a6w4(*a, table, wc, sw, b)
                q, h = gemm.linear_a6w4_gelu_dual(*a, table, wc, sw, b, return_gelu=True)
                assert q.shape == h.shape == (T, O) and q.dtype == h.dtype == torch.float16
                assert_bits_equal(h, _lookup(gelu_table, y), f"{what}: h == table[bits(y)]")
                assert bool(q.any()), what
                assert_bits_equal(q, _dual(h), f"{what}: fused vs the stand-alone quantizer on the emitted GELU values")
                assert_bits_equal(q.cpu(), orc.dual_per_group_kernel_sem(h.cpu(), "e1m2_neg", "e2m1_pos", 128, 1.0), f"{what}: fused vs oracle")
                assert_bits_equal(gemm.linear_a6w4_gelu_dual(*a, table, wc, sw, b), q, f"{what}: without the GELU output")


# ------------------------------------------------------------------------------------------------------------ 3. the NaN rule
@pytest.mark.parametrize("table", TABLES)
def test_nan_rule_and_scratch(dev, table):
    """One NaN in the GELU tensor (a NaN bias): every output bit zero, the 8-byte scratch zero again afterwards, the next clean call
    clean; one captured graph (a single stream, no parallel branches) replayed NaN, NaN, clean on static buffers."""
    from fpqvar_amd import gemm, ops
    a, w, bias = operands(dev, table, 200, 256, 256, 5)
    clean = gemm.linear_a6w4_gelu_dual(*a, table, *w, bias)
    assert bool(clean.any())
    bad = bias.clone()
    bad[77] = float("nan")
    z = gemm.linear_a6w4_gelu_dual(*a, table, *w, bad)
    assert not bool(z.view(torch.int16).any())
    scratch = ops._nan_scratch(dev)
    torch.cuda.synchronize()
    assert not bool(scratch.any()), "the NaN scratch must be zero again after the fix-up launch"
    assert_bits_equal(gemm.linear_a6w4_gelu_dual(*a, table, *w, bias), clean, "after a NaN call")
    sb = bad.clone()
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        gemm.linear_a6w4_gelu_dual(*a, table, *w, sb)
        gr = torch.cuda.CUDAGraph()
        with torch.cuda.graph(gr, stream=s):
            out = gemm.linear_a6w4_gelu_dual(*a, table, *w, sb)
    torch.cuda.current_stream().wait_stream(s)
    for _ in range(2):
        gr.replay()
        torch.cuda.synchronize()
        assert not bool(out.view(torch.int16).any())
    sb.copy_(bias)
    gr.replay()
    torch.cuda.synchronize()
    assert_bits_equal(out, clean, "graph replay without the NaN")


def test_argument_checks_on_the_gpu(dev):
    from fpqvar_amd import gemm
    a, w, bias = operands(dev, "e3m0", 8, 128, 128, 1)
    with pytest.raises(RuntimeError):
        gemm.linear_a6w4_gelu_dual(*a, "e3m0", w[0][:120], w[1][:120])          # outs % 128 != 0
    with pytest.raises(RuntimeError):
        gemm.linear_a6w4_gelu_dual(a[0][:, :-8], a[1], "e3m0", *w)               # truncated operand
    with pytest.raises(RuntimeError):
        gemm.linear_a6w4_gelu_dual(a[0].view(1, 8, 96), a[1], "e3m0", w[0].view(1, 128, 64), w[1])   # images: no k-major A6W4 form
    with pytest.raises(RuntimeError):
        gemm.linear_a6w4_gelu_dual(*a, "e2m1", *w)
    assert gemm.linear_a6w4_gelu_dual(a[0][:0], a[1][:0], "e3m0", *w).shape == (0, 128)
    q, h = gemm.linear_a6w4_gelu_dual(a[0][:0], a[1][:0], "e3m0", *w, return_gelu=True)
    assert q.shape == h.shape == (0, 128)


# ------------------------------------------------------------------------------------------------------------ 4. the modules
@pytest.mark.parametrize("act", ("fp_e1", "fp_e3"))
def test_fp4linear_gelu_dual_with_a_6bit_activation(dev, act):
    from fpqvar_amd import gemm
    table = {"fp_e1": "e1m2", "fp_e3": "e3m0"}[act]
    g = torch.Generator().manual_seed(7)
    lin = torch.nn.Linear(256, 384)
    with torch.no_grad():
        lin.weight.copy_(torch.randn(384, 256, generator=g) * 0.05)
        lin.bias.copy_(torch.randn(384, generator=g) * 0.1)
    lin = lin.to(dev)
    m = gemm.FP4LinearGeluDual.from_float(lin, act_fp_type=act)
    m4 = gemm.FP4LinearGeluDual.from_float(lin)
    assert m.act_table == table and m4.act_table == "e2m1" and not m.kmajor and not m4.kmajor
    assert torch.equal(m.w_codes, m4.w_codes) and torch.equal(m.w_scales, m4.w_scales)      # one stored weight serves both GEMMs
    x = torch.randn(2, 35, 256, generator=g).half().to(dev)
    y = m(x)
    ac, asc = gemm.quantize_g6(x.view(-1, 256), table)
    want = gemm.linear_a6w4_gelu_dual(ac, asc, table, m.w_codes, m.w_scales, m.bias)
    assert y.shape == (2, 35, 384)
    assert_bits_equal(y.view(-1, 384), want, "forward")
    assert bool(want.any())
    assert_bits_equal(m.forward_operands(ac, asc), want, "forward_operands, the module's format")
    assert_bits_equal(m4.forward_operands(ac, asc, table=table), want, "forward_operands(table=) on the fp_e2 module")
    a4 = gemm.quantize_mx(x.view(-1, 256))
    want4 = gemm.linear_fp4_gelu_dual(*a4, m4.w_codes, m4.w_scales, m4.bias)
    assert_bits_equal(m4(x).view(-1, 384), want4, "the fp_e2 module is what it was")
    assert_bits_equal(m.forward_operands(*a4, table="fp_e2"), want4, "forward_operands(table='fp_e2') on the 6-bit module")
    assert not torch.equal(want, want4)                                                   # (the two formats do quantize differently)
    with pytest.raises(ValueError):
        gemm.FP4LinearGeluDual.from_float(lin, kmajor=True, act_fp_type=act)
    mk = gemm.FP4LinearGeluDual.from_float(lin, kmajor=True)
    with pytest.raises(RuntimeError):
        mk.forward_operands(ac, asc, table=table)                                         # a k-major weight has no A6W4 form


# ------------------------------------------------------------------------------------------------------------ 5. the mixed model
def test_mixed_model_fuses_the_ffn(dev, gelu_table):
    """A toy VAR at C = 256, quantize_VAR_mixed_fp4_datatype(real_fp4=True, fuse_ffn=True) against the same call without fuse_ffn:
    blocks 0 and 1 (fc1 E3M0: the A6W4 kernel, row-major) and block 6 (fc1 E2M1: the FP4 kernel, k-major).  Per block the fused
    fc1's output is bit-equal to the dual quantizer of table[bits(y)], y the unfused model's fc1 output; the FFN output within the
    tolerance test_quantize_var_fuses_the_ffn states (torch's GELU in the unfused model is within one ulp of the table's)."""
    from fpqvar_amd import gemm, quant_linear as ql
    C = 256
    torch.manual_seed(11)
    kw = dict(weight_quant="per_group", act_quant="per_group", w_bit=4, a_bit=4, activation_fp_quant=True, weight_fp_quant=True,
              act_fp_type="fp_e2", weight_fp_type="fp_e2", fc2_fp_type="fp_e1m2_neg_e2m1_pos")
    base = _Var(C, 7).to(dev)
    plain = ql.quantize_VAR_mixed_fp4_datatype(copy.deepcopy(base), real_fp4=True, **kw).half()
    fused = ql.quantize_VAR_mixed_fp4_datatype(copy.deepcopy(base), real_fp4=True, fuse_ffn=True, **kw).half()
    x = torch.randn(3, 50, C, device=dev).half()
    for b in (0, 1, 6):
        pf, ff = plain.blocks[b].ffn, fused.blocks[b].ffn
        want_table = "e2m1" if b == 6 else "e3m0"
        assert type(pf.fc1) is gemm.FP4Linear and isinstance(pf.act, torch.nn.GELU)
        assert type(ff.fc1) is gemm.FP4LinearGeluDual and ff.fc1.act_table == pf.fc1.act_table == want_table
        assert ff.fc1.kmajor == pf.fc1.kmajor == (b == 6)
        assert isinstance(ff.act, torch.nn.Identity) and type(ff.fc2) is ql.QuantizedLinear_fc2 and "in fc1's epilogue" in repr(ff.fc2)
        y = pf.fc1(x)
        hq = ff.fc1(x)
        assert hq.shape == (3, 50, 4 * C)
        assert_bits_equal(hq.view(-1, 4 * C), _dual(_lookup(gelu_table, y.view(-1, 4 * C))), f"block {b}: fused fc1 vs quantizer(table[bits(y)])")
        ya, yb = pf(x).float(), ff(x).float()
        assert float((ya - yb).abs().max()) <= 2e-2 * float(ya.abs().max()) + 1e-3, b
    with pytest.raises(ValueError):
        ql.quantize_VAR_mixed_fp4_datatype(copy.deepcopy(base), real_fp4=True, fuse_ffn=True, **{**kw, "fc2_fp_type": "fp_e2"})
