"""The W6 GEMM on k-major images on the GPU (fpq_gemm_w6_mx_km, _gelu_dual_km, _mx_split_km, _mx_split_qknorm_km; gemm.linear_w6_km,
linear_w6_gelu_dual_km, linear_w6_qkv_to_cache_km; FP4Linear(..., kmajor=True, w6_kmajor=True); quantize_VAR_mixed(..., w6_kmajor=True)) -
after tests/test_gpu_a6w4_km.py.

The contract everywhere is BIT EQUALITY WITH THE ROW-MAJOR W6 PATH: the k-major kernels differ from their twins in the LDS-DMA source
addresses and the scale-tile load only - same LDS image, same main loop, same epilogues.  tests/test_gpu_w6*.py pin the row-major
path to the float64 bound, the fp32 model (tests/w6_model.py) and the oracle; no tolerance is introduced here.  The shapes are the
smallest that reach every edge of the image addressing: tokens % 4 != 0 (the scale image's padding), tokens below one tile and across
the 64 / 128 boundary (clamped image rows), outs % 64 != 0 (the weight image's padding and its clamp), G = 1, 2, 3, 15 (the scale
pieces' surplus groups), each over all six pairs and both tilings."""
import copy
import ctypes

import pytest
import torch

from tests import w6_model as wm
from tests.conftest import assert_bits_equal
from tests.test_gpu_a6w4 import _Var

pytestmark = pytest.mark.gpu

PAIRS = wm.PAIRS
IDS = [f"{a}-{w}" for a, w in PAIRS]
CFGS = (20, 30, None)    # FPQ_GEMM_CFG: 128 x 128 tiles, 64 x 128 tiles, the library's choice
PLAIN_SHAPES = ((1, 8, 128), (37, 72, 384), (65, 200, 384), (130, 136, 1920), (259, 264, 256))      # (T, O, K)
FC1_SHAPES = ((8, 128, 128), (37, 256, 384), (130, 384, 1920))                                      # (T, O, K)
SPLIT_SHAPES = ((2, 1, 2), (3, 9, 2), (2, 25, 4), (5, 64, 2), (2, 169, 4))                          # (bsz, seq, heads)
FP_NAME = {"e2m1": "fp_e2", "e1m2": "fp_e1", "e3m0": "fp_e3"}
FP = ("fp_e1", "fp_e2", "fp_e3")
ONE_PER_ACT = (("e2m1", "e3m0"), ("e1m2", "e1m2"), ("e3m0", "e1m2"))     # one pair per activation format


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "these tests need the GPU"
    return torch.device("cuda:0")


def _quantize_a(a_table, x, kmajor=False):
    from fpqvar_amd import gemm
    return gemm.quantize_mx(x, kmajor=kmajor) if a_table == "e2m1" else gemm.quantize_g6(x, a_table, kmajor=kmajor)


def _images(a_table, a, sa, w, sw):
    """row-major operands of a pair -> (activation image, its scale image, dealt weight image, weight-side scale image)"""
    from fpqvar_amd import gemm
    return (gemm.to_kmajor(a, 4 if a_table == "e2m1" else 6), gemm.to_kmajor_scales(sa), gemm.to_kmajor(w, 6, dealt=True),
            gemm.to_kmajor_scales(sw, weight_side=True))


def _assert_image_shapes(a_table, im, T, O, K):
    G, Op = K // 128, (O + 63) // 64 * 64
    assert im[0].shape == (G, T, wm.SEG[a_table]) and im[0].dtype == torch.uint8
    assert im[1].shape == (G, (T + 3) // 4 * 4) and im[1].dtype == torch.float32
    assert im[2].shape == (G, Op, 96) and im[2].dtype == torch.uint8
    assert im[3].shape == (G, Op) and im[3].dtype == torch.float32


def operands(dev, pair, T, K, O, seed):
    """activation through quantize_mx / quantize_g6 (row-major and as images), weight through quantize_g6(w.float(), w_table)"""
    from fpqvar_amd import gemm
    g = torch.Generator().manual_seed(seed)
    x = (torch.randn(T, K, generator=g) * torch.exp(0.3 * torch.randn(T, K, generator=g))).half().to(dev)
    w = (torch.randn(O, K, generator=g) * 0.05).to(dev)
    bias = (torch.randn(O, generator=g) * 0.3).half().to(dev)
    wq = gemm.quantize_g6(w.float(), pair[1])
    wk = (gemm.to_kmajor(wq[0], 6, dealt=True), gemm.to_kmajor_scales(wq[1], weight_side=True))
    return _quantize_a(pair[0], x), _quantize_a(pair[0], x, kmajor=True), wq, wk, bias


# ------------------------------------------------------------------------------------------------------------ 1. the plain form
@pytest.mark.parametrize("T,O,K", PLAIN_SHAPES)
@pytest.mark.parametrize("pair", PAIRS, ids=IDS)
def test_plain_form_equals_the_row_major_gemm(dev, pair, T, O, K, lib_options):
    """every family of the row-major sweep on converted operands: linear_w6_km == linear_w6 bit for bit in every tiling; the gauss
    family also against the fp32 model"""
    from fpqvar_amd import gemm
    at, wt = pair
    for family in wm.FAMILIES:
        c = wm.make_case(at, wt, family, T, O, K, seed=3, device=dev)
        im = _images(at, c["a"], c["a_scales"], c["w"], c["w_scales"])
        _assert_image_shapes(at, im, T, O, K)
        emu = wm.emulate(at, wt, c["a"], c["a_scales"], c["w"], c["w_scales"], c["bias"]) if family == "gauss" else None
        for cfg in CFGS:
            lib_options("FPQ_GEMM_CFG", cfg)
            what = f"{pair} {family} [{T} x {K} -> {O}] cfg {cfg}"
            want = gemm.linear_w6(c["a"], c["a_scales"], at, c["w"], c["w_scales"], wt, c["bias"])
            got = gemm.linear_w6_km(im[0], im[1], at, im[2], im[3], wt, c["bias"], outs=O)
            assert got.shape == (T, O)
            assert_bits_equal(got, want, what)
            if emu is not None:
                assert_bits_equal(got, emu, what + ": the fp32 model")
    # the producers' own images are the converted ones: the quantizer's kmajor=True form feeds the GEMM as it is
    a, ak, wq, wk, bias = operands(dev, pair, T, K, O, 17 + T)
    conv = _images(at, *a, *wq)
    assert torch.equal(ak[0], conv[0]) and torch.equal(ak[1].view(torch.int32), conv[1].view(torch.int32))
    assert_bits_equal(gemm.linear_w6_km(*ak, at, *wk, wt, bias, outs=O), gemm.linear_w6(*a, at, *wq, wt, bias), f"{pair}: quantizer images")


# ------------------------------------------------------------------------------------------------------------ 2. the tails
@pytest.mark.parametrize("pair", PAIRS, ids=IDS)
def test_bias_gate_residual_tails(dev, pair, lib_options):
    """a bias at an 8- but not 16-byte-aligned address, a gate with rows_per_gate > 1, a residual - each and together; and the
    residual aliasing `out`, through the C entry point"""
    from fpqvar_amd import gemm
    at, wt = pair
    g = torch.Generator().manual_seed(77)
    for T, O, K, B in ((130, 136, 384, 2), (66, 200, 256, 3)):
        c = wm.make_case(at, wt, "gauss", T, O, K, seed=5, device=dev)
        im = _images(at, c["a"], c["a_scales"], c["w"], c["w_scales"])
        bias8 = (torch.randn(O + 8, generator=g) * 0.1).half().to(dev)[4:O + 4]
        assert bias8.data_ptr() % 16 == 8
        gate = torch.randn(B, 1, O, generator=g).half().to(dev)
        resid = torch.randn(T, O, generator=g).half().to(dev)
        row = lambda b, **kw: gemm.linear_w6(c["a"], c["a_scales"], at, c["w"], c["w_scales"], wt, b, **kw)
        km = lambda b, **kw: gemm.linear_w6_km(im[0], im[1], at, im[2], im[3], wt, b, outs=O, **kw)
        for bias in (bias8, None):
            for cfg in CFGS:
                lib_options("FPQ_GEMM_CFG", cfg)
                what = f"{pair} [{T} x {K} -> {O}] cfg {cfg} bias {bias is not None}"
                for kw in ({}, dict(gate=gate), dict(residual=resid), dict(gate=gate, residual=resid)):
                    assert_bits_equal(km(bias, **kw), row(bias, **kw), f"{what} {sorted(kw)}")
    from fpqvar_amd._lib import GemmEpilogue, TABLE_IDS, check, lib, stream_ptr
    T, O, K = 130, 136, 384
    c = wm.make_case(at, wt, "gauss", T, O, K, seed=6, device=dev)
    im = _images(at, c["a"], c["a_scales"], c["w"], c["w_scales"])
    resid = torch.randn(T, O, generator=g).half().to(dev)
    want = gemm.linear_w6(c["a"], c["a_scales"], at, c["w"], c["w_scales"], wt, c["bias"], residual=resid)
    out = resid.clone()
    ep = GemmEpilogue(None, out.data_ptr(), 1)
    check(lib().fpq_gemm_w6_mx_km(im[0].data_ptr(), im[1].data_ptr(), TABLE_IDS[at], im[2].data_ptr(), im[3].data_ptr(), 1, TABLE_IDS[wt],
                                  c["bias"].data_ptr() if c["bias"] is not None else None, out.data_ptr(), T, O, K, ctypes.byref(ep),
                                  stream_ptr(dev)), "fpq_gemm_w6_mx_km")
    torch.cuda.synchronize()
    assert_bits_equal(out, want, "residual aliasing out")


# ------------------------------------------------------------------------------------------------------------ 3. the fc1 form
@pytest.mark.parametrize("T,O,K", FC1_SHAPES)
@pytest.mark.parametrize("pair", PAIRS, ids=IDS)
def test_fc1_form_equals_the_row_major_fc1_form(dev, pair, T, O, K, lib_options):
    from fpqvar_amd import gemm
    at, wt = pair
    a, ak, wq, wk, bias = operands(dev, pair, T, K, O, 11 + T)
    assert wk[0].shape == (K // 128, O, 96)                                  # outs % 128 == 0: no padding rows
    for cfg in CFGS:
        lib_options("FPQ_GEMM_CFG", cfg)
        for b in (bias, None):
            what = f"{pair} [{T} x {K} -> {O}] cfg {cfg} bias {b is not None}"
            q, h = gemm.linear_w6_gelu_dual(*a, at, *wq, wt, b, return_gelu=True)
            qk, hk = gemm.linear_w6_gelu_dual_km(*ak, at, *wk, wt, b, return_gelu=True, outs=O)
            assert qk.shape == hk.shape == (T, O) and bool(q.any())
            assert_bits_equal(hk, h, f"{what}: gelu_out")
            assert_bits_equal(qk, q, f"{what}: quantized output")
            assert_bits_equal(gemm.linear_w6_gelu_dual_km(*ak, at, *wk, wt, b), q, f"{what}: without the GELU output")


@pytest.mark.parametrize("pair", (("e2m1", "e3m0"), ("e3m0", "e1m2")), ids=("e2m1-e3m0", "e3m0-e1m2"))
def test_fc1_nan_rule_and_graph(dev, pair):
    """a NaN bias: every output +0 and the scratch zero again; one captured single-stream graph of emitter + GEMM replays to the eager
    bits"""
    from fpqvar_amd import gemm, ops
    at, wt = pair
    T, K, O = 70, 256, 256
    _, _, wq, wk, bias = operands(dev, pair, T, K, O, 5)
    g = torch.Generator().manual_seed(9)
    x = torch.randn(T, K, generator=g).half().to(dev)
    run = lambda b: gemm.linear_w6_gelu_dual_km(*_quantize_a(at, x, kmajor=True), at, *wk, wt, b, outs=O)
    clean = run(bias)
    assert bool(clean.any())
    assert_bits_equal(clean, gemm.linear_w6_gelu_dual(*_quantize_a(at, x), at, *wq, wt, bias), "eager vs the row-major form")
    bad = bias.clone()
    bad[77] = float("nan")
    z = run(bad)
    assert not bool(z.view(torch.int16).any())
    scratch = ops._nan_scratch(dev)
    torch.cuda.synchronize()
    assert not bool(scratch.any()), "the NaN scratch must be zero again after the fix-up launch"
    assert_bits_equal(run(bias), clean, "after a NaN call")
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        run(bias)
        gr = torch.cuda.CUDAGraph()
        with torch.cuda.graph(gr, stream=s):
            out = run(bias)
    torch.cuda.current_stream().wait_stream(s)
    for _ in range(2):
        gr.replay()
        torch.cuda.synchronize()
        assert_bits_equal(out, clean, "graph replay of emitter + GEMM")


# ------------------------------------------------------------------------------------------------------------ 4. the split output
def _bias32(c, seed, dev):
    g = torch.Generator().manual_seed(seed)
    b = torch.randn(3 * c, generator=g) * 0.1
    b[c:2 * c] = 0
    return b.to(dev)


def _scale_mul(heads, seed, dev):
    g = torch.Generator().manual_seed(seed)
    sm = torch.full((1, heads, 1, 1), 4.0).log() + 0.3 * torch.randn(1, heads, 1, 1, generator=g)
    sm[0, 0] = 5.5
    return sm.to(dev)


@pytest.mark.parametrize("bsz,seq,heads", SPLIT_SHAPES)
@pytest.mark.parametrize("pair", PAIRS, ids=IDS)
def test_split_output_equals_the_row_major_split_output(dev, pair, bsz, seq, heads, lib_options):
    """q and the written cache slots bit-equal to linear_w6_qkv_to_cache, with and without the q / k norm, with and without bias;
    every cache byte outside the written rows unchanged"""
    from fpqvar_amd import gemm, kv_cache
    at, wt = pair
    c, max_len, pos = heads * 64, seq + 5, 3
    a, ak, wq, wk, bias = operands(dev, pair, bsz * seq, c, 3 * c, bsz * seq + heads)
    hs = kv_cache.qk_norm_head_scale(_scale_mul(heads, seq, dev))
    b32 = _bias32(c, heads + seq, dev)
    for cfg in CFGS:
        lib_options("FPQ_GEMM_CFG", cfg)
        for norm in (False, True):
            for b in ((b32 if norm else bias), None):
                what = f"{pair} [{bsz} x {seq}, {heads} heads] cfg {cfg} norm {norm} bias {b is not None}"
                extra = dict(qk_norm_scale=hs) if norm else {}
                want_c = torch.full((2, bsz, max_len, heads, 64), 7.5, dtype=torch.float16, device=dev)
                got_c = torch.full_like(want_c, 7.5)
                want_q = gemm.linear_w6_qkv_to_cache(*a, at, *wq, wt, b, want_c, pos, seq, **extra)
                got_q = gemm.linear_w6_qkv_to_cache_km(*ak, at, *wk, wt, b, got_c, pos, seq, **extra)
                assert got_q.shape == (bsz, seq, c)
                assert_bits_equal(got_q, want_q, f"{what}: q")
                assert_bits_equal(got_c, want_c, f"{what}: the cache")
                keep = torch.ones(max_len, dtype=torch.bool, device=dev)
                keep[pos:pos + seq] = False
                assert bool((got_c[:, :, keep] == 7.5).all()), f"{what}: the GEMM wrote outside its slots"
                assert bool((got_c[:, :, pos:pos + seq] != 7.5).any()), what


# ------------------------------------------------------------------------------------------------------------ 5. the modules
def _linear(dev, k, o, bias=True, seed=7):
    g = torch.Generator().manual_seed(seed)
    lin = torch.nn.Linear(k, o, bias=bias)
    with torch.no_grad():
        lin.weight.copy_(torch.randn(o, k, generator=g) * 0.05)
        if bias:
            lin.bias.copy_(torch.randn(o, generator=g) * 0.1)
    return lin.to(dev)


@pytest.mark.parametrize("pair", ONE_PER_ACT, ids=[f"{a}-{w}" for a, w in ONE_PER_ACT])
def test_modules_on_kmajor_images(dev, pair):
    """FP4Linear / FP4LinearGeluDual(w6_forms=True) with kmajor=True, w6_kmajor=True against their row-major twins: forward,
    forward_operands on images, qkv_to_cache, adaln_operands -> forward_operands; 2-D codes against the k-major module raise"""
    from fpqvar_amd import gemm
    at, wt = pair
    K, O = 256, 392
    kw = dict(act_fp_type=FP_NAME[at], weight_fp_type=FP_NAME[wt], w6_forms=True)
    lin = _linear(dev, K, O)
    row = gemm.FP4Linear.from_float(lin, **kw).half()
    km = gemm.FP4Linear.from_float(lin, kmajor=True, w6_kmajor=True, **kw).half()
    same = gemm.FP4Linear.from_float(lin, w6_kmajor=True, **kw)                # w6_kmajor alone changes nothing
    assert not same.kmajor and torch.equal(same.w_codes, row.w_codes) and torch.equal(same.w_scales, row.w_scales)
    assert km.kmajor and not row.kmajor and (km.act_table, km.w_table, km.w6_forms) == (at, wt, True)
    assert torch.equal(km.w_codes, gemm.to_kmajor(row.w_codes, 6, dealt=True)) and km.w_codes.shape == (K // 128, 448, 96)
    assert torch.equal(km.w_scales, gemm.to_kmajor_scales(row.w_scales, weight_side=True)) and km.w_scales.dtype == torch.float32
    g = torch.Generator().manual_seed(3)
    x = torch.randn(2, 35, K, generator=g).half().to(dev)
    gate, resid = torch.randn(2, 1, O, generator=g).half().to(dev), torch.randn(2, 35, O, generator=g).half().to(dev)
    assert_bits_equal(km(x), row(x), "forward")
    assert_bits_equal(km(x, gate=gate, residual=resid), row(x, gate=gate, residual=resid), "forward with the tail")
    ak = _quantize_a(at, x.view(-1, K), kmajor=True)
    assert_bits_equal(km.forward_operands(*ak), row(x).view(-1, O), "forward_operands on images")
    with pytest.raises(RuntimeError, match="k-major images"):
        km.forward_operands(*_quantize_a(at, x.view(-1, K)))
    sc = (torch.randn(2, 1, K, generator=g) * 0.3).half().to(dev)
    sh = (torch.randn(2, 1, K, generator=g) * 0.3).half().to(dev)
    xr = torch.randn(2, 35, K, generator=g).to(dev)
    ops_k, ops_r = km.adaln_operands(xr, sc, sh), row.adaln_operands(xr, sc, sh)
    assert ops_k[0].dim() == 3 and ops_r[0].dim() == 2
    assert_bits_equal(km.forward_operands(*ops_k), row.forward_operands(*ops_r), "adaln_operands -> forward_operands")
    assert_bits_equal(km.forward_operands(*km.rotate_operands(xr)), row.forward_operands(*row.rotate_operands(xr)), "rotate_operands")
    # fc1
    lin1 = _linear(dev, K, 384, seed=8)
    d_row = gemm.FP4LinearGeluDual.from_float(lin1, **kw).half()
    d_km = gemm.FP4LinearGeluDual.from_float(lin1, kmajor=True, w6_kmajor=True, **kw).half()
    assert d_km.kmajor and d_km.w_codes.shape == (K // 128, 384, 96)
    assert bool(d_row(x).any())
    assert_bits_equal(d_km(x), d_row(x), "fc1: forward")
    assert_bits_equal(d_km.forward_operands(*ak), d_row(x).view(-1, 384), "fc1: forward_operands on images")
    assert_bits_equal(d_km.forward_operands(*d_km.adaln_operands(xr, sc, sh)), d_row.forward_operands(*d_row.adaln_operands(xr, sc, sh)),
                      "fc1: adaln_operands -> forward_operands")
    with pytest.raises(RuntimeError, match="k-major images"):
        d_km.forward_operands(*_quantize_a(at, x.view(-1, K)))
    # mat_qkv
    heads, pos, seq = 4, 3, 35
    linq = _linear(dev, K, 3 * K, bias=False, seed=9)
    q_row = gemm.FP4Linear.from_float(linq, **kw)
    q_km = gemm.FP4Linear.from_float(linq, kmajor=True, w6_kmajor=True, **kw)
    from fpqvar_amd import kv_cache
    hs = kv_cache.qk_norm_head_scale(_scale_mul(heads, 4, dev))
    for extra in ({}, dict(qk_norm_scale=hs, bias=_bias32(K, 2, dev))):
        want_c = torch.full((2, 2, seq + 9, heads, 64), 7.5, dtype=torch.float16, device=dev)
        got_c, op_c = torch.full_like(want_c, 7.5), torch.full_like(want_c, 7.5)
        want_q = q_row.qkv_to_cache(x, want_c, pos, seq, **extra)
        assert_bits_equal(q_km.qkv_to_cache(x, got_c, pos, seq, **extra), want_q, f"qkv_to_cache {sorted(extra)}: q")
        assert_bits_equal(got_c, want_c, f"qkv_to_cache {sorted(extra)}: the cache")
        assert_bits_equal(q_km.qkv_to_cache_operands(*ak, op_c, pos, seq, **extra), want_q, f"qkv_to_cache_operands {sorted(extra)}: q")
        assert_bits_equal(op_c, want_c, f"qkv_to_cache_operands {sorted(extra)}: the cache")
    # without w6_kmajor every k-major request raises what it raised
    for bad in (dict(kmajor=True), dict(a6w4_kmajor=True), dict(kmajor=True, a6w4_kmajor=True)):
        with pytest.raises(ValueError, match="no k-major form"):
            gemm.FP4Linear.from_float(lin, **bad, **kw)


# ------------------------------------------------------------------------------------------------------------ 6. a mixed model
def test_mixed_model_on_one_layout(dev):
    """The 9-block toy VAR at C = 256, block b = 3 i + j with formats FP[i] x FP[j] on fc1, mat_qkv and proj: converted with and
    without w6_kmajor (+ a6w4_kmajor, w6_forms, fuse_ffn) the module outputs are bit-equal per block, and with it every matrix-core
    FP4Linear of the model holds k-major images"""
    from fpqvar_amd import gemm, quant_linear as ql
    C = 256
    torch.manual_seed(11)
    kw = dict(weight_quant="per_group", act_quant="per_group", w_bit=4, a_bit=4, activation_fp_quant=True, weight_fp_quant=True,
              real_fp4=True, w6_weights=True, w6_forms=True, fuse_ffn=True, a6w4_kmajor=True)

    def fmt(b, layer):
        return ("fp_e1m2_neg_e2m1_pos", "fp_e2") if layer == "fc2" else (FP[b // 3], FP[b % 3])
    base = _Var(C, 9).to(dev)
    rowm = ql.quantize_VAR_mixed(copy.deepcopy(base), fmt, **kw).half()
    kmm = ql.quantize_VAR_mixed(copy.deepcopy(base), fmt, w6_kmajor=True, **kw).half()
    off = ql.quantize_VAR_mixed(copy.deepcopy(base), fmt, w6_kmajor=True, **dict(kw, kmajor_operands=False, a6w4_kmajor=False))
    assert not any(m.kmajor for m in off.modules() if isinstance(m, gemm.FP4Linear))     # inert without kmajor_operands
    with pytest.raises(ValueError, match="w6_kmajor needs w6_weights"):
        ql.quantize_VAR_mixed(copy.deepcopy(base), fmt, w6_kmajor=True, **dict(kw, w6_weights=False, w6_forms=False))
    fp4 = [m for m in kmm.modules() if isinstance(m, gemm.FP4Linear)]
    assert len(fp4) == 27 and all(m.kmajor for m in fp4)
    x = torch.randn(3, 50, C, device=dev).half()
    inv = {v: k for k, v in FP_NAME.items()}
    for b in range(9):
        rb, kb = rowm.blocks[b], kmm.blocks[b]
        six = FP[b % 3] != "fp_e2"
        for name in ("ffn.fc1", "attn.mat_qkv", "attn.proj"):
            mr, mk = rb.get_submodule(name), kb.get_submodule(name)
            assert type(mk) is type(mr) and (mk.act_table, mk.w_table) == (mr.act_table, mr.w_table) == (inv[FP[b // 3]], inv[FP[b % 3]])
            assert mk.kmajor and mr.kmajor is (not six), (b, name)
            assert mk.w_codes.shape[2] == (96 if six else 64)
            assert_bits_equal(mk(x), mr(x), f"block {b} {name}")
        assert type(kb.ffn.fc1) is gemm.FP4LinearGeluDual
        assert_bits_equal(kb.ffn(x), rb.ffn(x), f"block {b}: the FFN's output")
        cr = torch.full((2, 3, 60, 4, 64), 7.5, dtype=torch.float16, device=dev)
        ck = torch.full_like(cr, 7.5)
        assert_bits_equal(kb.attn.mat_qkv.qkv_to_cache(x, ck, 2, 50), rb.attn.mat_qkv.qkv_to_cache(x, cr, 2, 50), f"block {b}: q")
        assert_bits_equal(ck, cr, f"block {b}: the cache")


# ------------------------------------------------------------------------------------------------------------ 7. rejections
def test_rejections_on_device_tensors(dev):
    from fpqvar_amd import gemm
    pair = ("e3m0", "e1m2")
    T, K, O = 8, 128, 136
    a, ak, wq, wk, bias = operands(dev, pair, T, K, O, 1)
    cache = torch.zeros(2, 2, 8, 2, 64, dtype=torch.float16, device=dev)
    fns = (lambda *o: gemm.linear_w6_km(*o[:2], "e3m0", *o[2:], "e1m2", outs=O),
           lambda *o: gemm.linear_w6_gelu_dual_km(*o[:2], "e3m0", *o[2:], "e1m2"),
           lambda *o: gemm.linear_w6_qkv_to_cache_km(*o[:2], "e3m0", *o[2:], "e1m2", None, cache, 0, 4))
    for fn in fns:
        with pytest.raises(RuntimeError, match="k-major images"):
            fn(*a, *wq)                                                       # row-major codes
        with pytest.raises(RuntimeError, match="k-major images"):
            fn(*a, *wk)                                                       # a mixed pair
    assert_bits_equal(gemm.linear_w6_km(*ak, "e3m0", *wk, "e1m2", bias, outs=O), gemm.linear_w6(*a, "e3m0", *wq, "e1m2", bias), "the good call")
    with pytest.raises(RuntimeError, match="multiple of 64 rows"):
        gemm.linear_w6_km(*ak, "e3m0", wk[0][:, :O].contiguous(), wk[1][:, :O].contiguous(), "e1m2", outs=O)       # unpadded weight image
    with pytest.raises(RuntimeError, match="does not belong"):
        gemm.linear_w6_km(*ak, "e3m0", *wk, "e1m2", outs=64)                  # a weight image of the wrong padded row count
    with pytest.raises(RuntimeError, match="float32"):
        gemm.linear_w6_km(*ak, "e3m0", wk[0], wk[1].half(), "e1m2", outs=O)   # fp16 weight scale image
    with pytest.raises(RuntimeError, match="float32"):
        gemm.linear_w6_km(ak[0], ak[1].half(), "e3m0", *wk, "e1m2", outs=O)   # fp16 activation scale image
    with pytest.raises(RuntimeError, match="'e1m2' and 'e3m0'"):
        gemm.linear_w6_km(*ak, "e3m0", *wk, "e2m1", outs=O)                   # an E2M1 weight table
    with pytest.raises(RuntimeError, match="k-major images"):
        gemm.linear_w6_km(*_quantize_a("e2m1", torch.zeros(T, K, dtype=torch.float16, device=dev), kmajor=True), "e3m0", *wk, "e1m2", outs=O)
    for fn in (gemm.linear_w6, gemm.linear_w6_gelu_dual):                     # the row-major functions go on refusing images
        with pytest.raises(RuntimeError, match="row-major operands only"):
            fn(*ak, "e3m0", *wk, "e1m2")
