"""The A6W4 path on k-major images on the GPU (include/fpq.h, "THE A6W4 PATH ON K-MAJOR IMAGES"): the image-writing emitter
(gemm.quantize_g6(kmajor=True)), the GEMM and its fc1 form (gemm.linear_a6w4_km, gemm.linear_a6w4_gelu_dual_km), the modules
(gemm.FP4Linear / FP4LinearGeluDual.from_float(a6w4_kmajor=True)) and the mixed model (quantize_VAR_mixed*(a6w4_kmajor=True)).

The contract everywhere is BIT EQUALITY with the row-major path, which tests/test_gpu_a6w4.py and tests/test_gpu_a6w4_fc1.py pin to
the float64 bound, the fp32 model of tests/a6w4_model.py and the oracle: no tolerance is introduced here.  The shapes are the
smallest that reach every edge of the image addressing: tokens that are no multiple of 4 (scale-image padding), below one tile and
across the 64 / 128 boundary (clamped rows), outs % 64 != 0 (weight-image padding and clamp), G = 1, 2, 3 and 15 (one stage only,
odd group counts, a last scale piece with surplus groups)."""
import copy
import math

import numpy as np
import pytest
import torch

from tests import a6w4_model as am
from tests.conftest import assert_bits_equal
from tests.test_gpu_a6w4 import _Var, _on, _same_bits
from tests.test_gpu_a6w4_fc1 import operands

pytestmark = pytest.mark.gpu

TABLES = ("e1m2", "e3m0")
CFGS = (20, 30, None)    # FPQ_GEMM_CFG: 128 x 128 tiles, 64 x 128 tiles, the library's choice
GEMM_SHAPES = ((1, 8, 128), (37, 72, 384), (65, 200, 384), (130, 136, 1920), (259, 264, 256))   # (T, O, K)
FC1_SHAPES = ((8, 128, 128), (37, 256, 384), (130, 384, 1920))                                   # (T, O, K)


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "these tests need the GPU"
    return torch.device("cuda:0")


def _images(gemm, c):
    """the row-major case `c` (tests/a6w4_model.py make_case, on the GPU) as k-major operands"""
    return (gemm.to_kmajor(c["a"], 6), gemm.to_kmajor_scales(c["a_scales"]), gemm.to_kmajor(c["w"], 4, dealt=True),
            gemm.to_kmajor_scales(c["w_scales"], weight_side=True))


def _lin(gemm, table, c, **kw):
    return gemm.linear_a6w4(c["a"], c["a_scales"], table, c["w"], c["w_scales"], c["bias"], **kw)


def _lin_km(gemm, table, c, im, **kw):
    return gemm.linear_a6w4_km(im[0], im[1], table, im[2], im[3], c["bias"], outs=c["w"].shape[0], **kw)


# ------------------------------------------------------------------------------------------------------------ 1. the emitter
def km6_image(codes: np.ndarray) -> np.ndarray:
    """include/fpq.h, "K-MAJOR OPERAND IMAGES", restated: image[(s * rows + j) * 96 + p * 16 + b] = codes[j, s * 96 + c(j, p) * 16 + b]
    with c = (p - ((j >> 3) & 1)) mod 6 - the activation side: row(j) = j, no padding."""
    rows, steps = codes.shape[0], codes.shape[1] // 96
    image = np.zeros((steps, rows, 96), dtype=np.uint8)
    for s in range(steps):
        for j in range(rows):
            for p in range(6):
                c = (p - ((j >> 3) & 1)) % 6
                image[s, j, p * 16:p * 16 + 16] = codes[j, s * 96 + c * 16:s * 96 + c * 16 + 16]
    return image


@pytest.mark.parametrize("table", TABLES)
def test_emitter_writes_the_images(dev, table):
    """rows 1, 3, 37, 130 x K 128, 384, 1920, fp16: the code image is the header's formula applied to quantize_g6's row-major codes
    (restated above in numpy) and equals to_kmajor(codes, 6); the scale image holds float32(scales)[t, g] at [g, t] and its padding
    rows are exactly 0; fp32 rows give the same images through the two-step route."""
    from fpqvar_amd import gemm
    g = torch.Generator().manual_seed(1300 + len(table))
    for rows in (1, 3, 37, 130):
        for K in (128, 384, 1920):
            x = (torch.randn(rows, K, generator=g) * torch.exp(0.7 * torch.randn(rows, K, generator=g))).half()
            x[0, :128] = 0                                              # an all-zero group: scale 0, code 0
            xd = x.to(dev)
            codes, scales = gemm.quantize_g6(xd, table)
            image, simage = gemm.quantize_g6(xd, table, kmajor=True)
            what = f"{table} [{rows} x {K}]"
            rows4 = (rows + 3) // 4 * 4
            assert image.shape == (K // 128, rows, 96) and image.dtype == torch.uint8, what
            assert simage.shape == (K // 128, rows4) and simage.dtype == torch.float32, what
            assert np.array_equal(image.cpu().numpy(), km6_image(codes.cpu().numpy())), f"{what}: code image vs the header's formula"
            assert torch.equal(image, gemm.to_kmajor(codes, 6)), f"{what}: code image vs to_kmajor"
            assert_bits_equal(simage[:, :rows], scales.float().t().contiguous(), f"{what}: scale image")
            assert not bool(simage[:, rows:].view(torch.int32).any()), f"{what}: scale image padding"
            assert torch.equal(simage, gemm.to_kmajor_scales(scales)), f"{what}: scale image vs to_kmajor_scales"
            assert float(simage[0, 0]) == 0.0 and not bool(image[0, 0].any())
            # fp32 rows: the row-major emitter + the two converters
            x32 = xd.float()
            c32, s32 = gemm.quantize_g6(x32, table)
            i32, si32 = gemm.quantize_g6(x32, table, kmajor=True)
            assert torch.equal(i32, gemm.to_kmajor(c32, 6)) and torch.equal(si32, gemm.to_kmajor_scales(s32)), f"{what}: fp32 rows"
            assert si32.dtype == torch.float32 and i32.shape == image.shape and si32.shape == simage.shape


@pytest.mark.parametrize("table", TABLES)
def test_emitter_non_finite_groups(dev, table):
    """A group holding +inf and a group holding a NaN: the non-finite value travels in the SCALE and every code is the row-major
    emitter's (a valid code), as tests/test_gpu_a6w4.py states for that emitter."""
    from fpqvar_amd import gemm
    g = torch.Generator().manual_seed(43)
    x = torch.randn(37, 384, generator=g).half()
    x[3, 5], x[17, 300], x[17, 20] = math.inf, math.nan, -1.0
    xd = x.to(dev)
    codes, scales = gemm.quantize_g6(xd, table)
    image, simage = gemm.quantize_g6(xd, table, kmajor=True)
    assert torch.equal(image, gemm.to_kmajor(codes, 6))
    assert math.isinf(float(simage[0, 3])) and float(simage[0, 3]) > 0 and math.isnan(float(simage[2, 17]))
    fin = torch.ones_like(simage, dtype=torch.bool)
    fin[0, 3] = fin[2, 17] = False
    assert bool(torch.isfinite(simage[fin]).all())
    assert _same_bits(simage[:, :37].half(), scales.t().contiguous())
    lv = am.decode_a(table, codes.cpu())
    assert set(lv.abs().unique().tolist()) <= set(am.A_LEVELS[table])


# ------------------------------------------------------------------------------------------------------------ 2. the plain GEMM
@pytest.mark.parametrize("T,O,K", GEMM_SHAPES)
@pytest.mark.parametrize("table", TABLES)
def test_gemm_equals_the_row_major_gemm(dev, table, T, O, K, lib_options):
    """Every family of the row-major sweep (non-finite scales, overflow, cancelling bias, zero ... included), each tiling:
    linear_a6w4_km on the converted operands is bit-equal to linear_a6w4 on the row-major ones; for one family per table also
    to the fp32 model am.emulate."""
    from fpqvar_amd import gemm
    assert "gauss" in am.FAMILIES   # the family that is also held to the fp32 model
    for family in am.FAMILIES:
        c = _on(am.make_case(table, family, T, O, K), dev)
        im = _images(gemm, c)
        assert im[0].shape == (K // 128, T, 96) and im[2].shape == (K // 128, (O + 63) // 64 * 64, 64)
        emu = am.emulate(table, c["a"], c["a_scales"], c["w"], c["w_scales"], c["bias"]) if family == "gauss" else None
        for cfg in CFGS:
            lib_options("FPQ_GEMM_CFG", cfg)
            what = f"{table} {family} [{T} x {K} -> {O}] cfg {cfg}"
            want, got = _lin(gemm, table, c), _lin_km(gemm, table, c, im)
            assert got.shape == (T, O) and got.dtype == torch.float16, what
            assert _same_bits(got, want), f"{what}: {int((got.view(torch.int16) != want.view(torch.int16)).sum())} elements differ"
            if emu is not None:
                assert _same_bits(got, emu), f"{what}: differs from emulate()"


# ------------------------------------------------------------------------------------------------------------ 3. the tails
@pytest.mark.parametrize("table", TABLES)
def test_bias_gate_residual_tails(dev, table, lib_options):
    """a bias at an 8-byte but not 16-byte aligned address, a gate with rows_per_gate > 1, a residual that IS the output's
    storage... each bit-equal to the row-major GEMM's result for the same tail."""
    from fpqvar_amd import gemm
    g = torch.Generator().manual_seed(77)
    for T, O, K, B in ((130, 136, 384, 5), (65, 200, 256, 1)):
        c = _on(am.make_case(table, "gauss", T, O, K, seed=5), dev)
        im = _images(gemm, c)
        store = (torch.randn(O + 8, generator=g) * 0.1).half().to(dev)
        bias8 = store[4:O + 4]
        assert bias8.data_ptr() % 16 == 8
        gate = torch.randn(B, 1, O, generator=g).half().to(dev)
        resid = torch.randn(T, O, generator=g).half().to(dev)
        for bias in (bias8, None):
            cv = dict(c, bias=bias)
            for cfg in CFGS:
                lib_options("FPQ_GEMM_CFG", cfg)
                what = (table, T, O, cfg, bias is not None)
                assert _same_bits(_lin_km(gemm, table, cv, im), _lin(gemm, table, cv)), what
                assert _same_bits(_lin_km(gemm, table, cv, im, gate=gate), _lin(gemm, table, cv, gate=gate)), what
                assert _same_bits(_lin_km(gemm, table, cv, im, residual=resid), _lin(gemm, table, cv, residual=resid)), what
                assert _same_bits(_lin_km(gemm, table, cv, im, gate=gate, residual=resid), _lin(gemm, table, cv, gate=gate, residual=resid)), what
    # the residual aliasing `out`, through the C entry point (the wrapper allocates its output)
    from fpqvar_amd._lib import GemmEpilogue, TABLE_IDS, check, lib, stream_ptr
    import ctypes
    T, O, K = 130, 136, 384
    c = _on(am.make_case(table, "gauss", T, O, K, seed=6), dev)
    im = _images(gemm, c)
    resid = torch.randn(T, O, generator=g).half().to(dev)
    want = _lin(gemm, table, c, residual=resid)
    out = resid.clone()
    ep = GemmEpilogue(None, out.data_ptr(), 1)
    check(lib().fpq_gemm_a6w4_mx_km(im[0].data_ptr(), im[1].data_ptr(), TABLE_IDS[table], im[2].data_ptr(), im[3].data_ptr(), 1,
                                    c["bias"].data_ptr() if c["bias"] is not None else None, out.data_ptr(), T, O, K, ctypes.byref(ep),
                                    stream_ptr(dev)), "fpq_gemm_a6w4_mx_km")
    torch.cuda.synchronize()
    assert _same_bits(out, want), "residual aliasing out"


# ------------------------------------------------------------------------------------------------------------ 4. the fc1 form
def _fc1_images(gemm, a, w):
    return (gemm.to_kmajor(a[0], 6), gemm.to_kmajor_scales(a[1]), gemm.to_kmajor(w[0], 4, dealt=True), gemm.to_kmajor_scales(w[1], weight_side=True))


@pytest.mark.parametrize("T,O,K", FC1_SHAPES)
@pytest.mark.parametrize("table", TABLES)
def test_fc1_form_equals_the_row_major_fc1_form(dev, table, T, O, K, lib_options):
    from fpqvar_amd import gemm
    a, w, bias = operands(dev, table, T, K, O, 11 + T)
    im = _fc1_images(gemm, a, w)
    for cfg in CFGS:
        lib_options("FPQ_GEMM_CFG", cfg)
        for b in (bias, None):
            what = f"{table} [{T} x {K} -> {O}] cfg {cfg} bias {b is not None}"
            q0, h0 = gemm.linear_a6w4_gelu_dual(*a, table, *w, b, return_gelu=True)
            q, h = gemm.linear_a6w4_gelu_dual_km(im[0], im[1], table, im[2], im[3], b, return_gelu=True)
            assert q.shape == h.shape == (T, O) and bool(q.any()), what
            assert_bits_equal(h, h0, f"{what}: GELU values")
            assert_bits_equal(q, q0, f"{what}: quantized values")
            assert_bits_equal(gemm.linear_a6w4_gelu_dual_km(im[0], im[1], table, im[2], im[3], b), q0, f"{what}: without the GELU output")


@pytest.mark.parametrize("table", TABLES)
def test_fc1_form_nan_rule_and_graph(dev, table):
    """One NaN in a live row (a NaN bias): every output +0 and the scratch zero again, as in the row-major test; one captured graph
    (a single stream) of emitter + fc1 GEMM on static buffers replays to the eager bits."""
    from fpqvar_amd import gemm, ops
    T, O, K = 37, 256, 384
    a, w, bias = operands(dev, table, T, K, O, 5)
    im = _fc1_images(gemm, a, w)
    clean = gemm.linear_a6w4_gelu_dual(*a, table, *w, bias)
    bad = bias.clone()
    bad[77] = float("nan")
    z = gemm.linear_a6w4_gelu_dual_km(im[0], im[1], table, im[2], im[3], bad)
    assert not bool(z.view(torch.int16).any())
    scratch = ops._nan_scratch(dev)
    torch.cuda.synchronize()
    assert not bool(scratch.any()), "the NaN scratch must be zero again after the fix-up launch"
    assert_bits_equal(gemm.linear_a6w4_gelu_dual_km(im[0], im[1], table, im[2], im[3], bias), clean, "after a NaN call")
    g = torch.Generator().manual_seed(9)
    x = (torch.randn(T, K, generator=g) * 1.5).half().to(dev)
    want = gemm.linear_a6w4_gelu_dual(*gemm.quantize_g6(x, table), table, *w, bias)
    xs = x.clone()
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        gemm.linear_a6w4_gelu_dual_km(*gemm.quantize_g6(xs, table, kmajor=True), table, im[2], im[3], bias)   # warm-up outside the capture
        gr = torch.cuda.CUDAGraph()
        with torch.cuda.graph(gr, stream=s):
            out = gemm.linear_a6w4_gelu_dual_km(*gemm.quantize_g6(xs, table, kmajor=True), table, im[2], im[3], bias)
    torch.cuda.current_stream().wait_stream(s)
    for _ in range(2):
        gr.replay()
        torch.cuda.synchronize()
        assert_bits_equal(out, want, "graph replay")
    xs.mul_(2)
    gr.replay()
    torch.cuda.synchronize()
    assert_bits_equal(out, gemm.linear_a6w4_gelu_dual(*gemm.quantize_g6(xs, table), table, *w, bias), "graph replay on new input")


# ------------------------------------------------------------------------------------------------------------ 5. the modules
@pytest.mark.parametrize("cls_name", ("FP4Linear", "FP4LinearGeluDual"))
@pytest.mark.parametrize("act", ("fp_e1", "fp_e3"))
def test_modules_with_a6w4_kmajor(dev, act, cls_name):
    from fpqvar_amd import gemm
    cls = getattr(gemm, cls_name)
    table = {"fp_e1": "e1m2", "fp_e3": "e3m0"}[act]
    g = torch.Generator().manual_seed(7)
    lin = torch.nn.Linear(256, 384)
    with torch.no_grad():
        lin.weight.copy_(torch.randn(384, 256, generator=g) * 0.05)
        lin.bias.copy_(torch.randn(384, generator=g) * 0.1)
    lin = lin.to(dev)
    mk = cls.from_float(lin, kmajor=True, act_fp_type=act, a6w4_kmajor=True)
    mr = cls.from_float(lin, act_fp_type=act)
    m4 = cls.from_float(lin, kmajor=True)
    assert mk.kmajor and mk.act_table == table and not mr.kmajor
    assert torch.equal(mk.w_codes, m4.w_codes) and torch.equal(mk.w_scales, m4.w_scales)      # one stored k-major weight serves both GEMMs
    assert not cls.from_float(lin, act_fp_type=act, a6w4_kmajor=True).kmajor                   # the flag alone changes nothing
    with pytest.raises(ValueError, match="no k-major form"):
        cls.from_float(lin, kmajor=True, act_fp_type=act)
    x = torch.randn(2, 35, 256, generator=g).half().to(dev)
    want = mr(x)
    assert want.shape == (2, 35, 384) and bool(want.any())
    assert_bits_equal(mk(x), want, "forward")
    image, simage = gemm.quantize_g6(x.view(-1, 256), table, kmajor=True)
    assert_bits_equal(mk.forward_operands(image, simage), want.view(-1, 384), "forward_operands on images")
    assert_bits_equal(m4.forward_operands(image, simage, table=table), want.view(-1, 384), "forward_operands(table=) on the fp_e2 k-major module")
    with pytest.raises(RuntimeError):
        mk.forward_operands(*gemm.quantize_g6(x.view(-1, 256), table))                       # 2-D codes against the k-major weight


# ------------------------------------------------------------------------------------------------------------ 6. the mixed model
def test_mixed_model_on_kmajor_images(dev):
    """The toy VAR of test_mixed_model_fuses_the_ffn (C = 256): real_fp4, fuse_ffn and a6w4_kmajor against the same call without
    the flag - per block the matrix-core modules' outputs are bit-equal, and every 6-bit layer reports kmajor."""
    from fpqvar_amd import gemm, quant_linear as ql
    C = 256
    torch.manual_seed(11)
    kw = dict(weight_quant="per_group", act_quant="per_group", w_bit=4, a_bit=4, activation_fp_quant=True, weight_fp_quant=True,
              act_fp_type="fp_e2", weight_fp_type="fp_e2", fc2_fp_type="fp_e1m2_neg_e2m1_pos")
    base = _Var(C, 7).to(dev)
    plain = ql.quantize_VAR_mixed_fp4_datatype(copy.deepcopy(base), real_fp4=True, fuse_ffn=True, **kw).half()
    km = ql.quantize_VAR_mixed_fp4_datatype(copy.deepcopy(base), real_fp4=True, fuse_ffn=True, a6w4_kmajor=True, **kw).half()
    x = torch.randn(3, 50, C, device=dev).half()
    n6 = 0
    for b in range(7):
        for path in ("ffn.fc1", "attn.mat_qkv", "attn.proj"):
            mp, mk = plain.blocks[b].get_submodule(path), km.blocks[b].get_submodule(path)
            assert type(mp) is type(mk) and isinstance(mk, gemm.FP4Linear) and mk.act_table == mp.act_table, (b, path)
            assert mk.kmajor, (b, path)
            if mk.act_table != "e2m1":
                n6 += 1
                assert not mp.kmajor, (b, path)
            assert_bits_equal(mk(x), mp(x), f"block {b} {path}")
    assert n6 == 6 + 6        # fc1: E3M0 outside blocks 6 - 20; mat_qkv: E3M0 outside blocks 0, 24, 25
    off = ql.quantize_VAR_mixed_fp4_datatype(copy.deepcopy(base), real_fp4=True, fuse_ffn=True, kmajor_operands=False, a6w4_kmajor=True, **kw)
    assert not any(m.kmajor for m in off.modules() if isinstance(m, gemm.FP4Linear))
