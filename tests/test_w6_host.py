"""E1M2 / E3M0 weights on the matrix cores (the W6 GEMM, fpq_gemm_w6_mx) without a GPU: the premises of its exactness argument, the
model tests/test_gpu_w6.py holds the kernel to, the C entry point's argument checks in their stated order, FP4Linear's refusals
for a 6-bit weight and the routing of quantize_VAR_mixed(real_fp4=True, w6_weights=...)."""
import ctypes

import pytest
import torch

from tests import gemm_model as gm
from tests import w6_model as wm
from tests.test_a6w4_host import CATCHES, SHAPES, W4A4, _Var

OK, ERR_ARG, ERR_DTYPE, ERR_SHAPE, ERR_TABLE = 0, -1, -2, -3, -4
F16, F32 = 0, 1
E2M1, E1M2, E3M0, E2M3, E3M2 = 0, 1, 2, 3, 4   # enum fpq_table
PTR = 0x7000_0000_1000   # an address with every alignment the checks ask for; nothing reads it
IDS = [f"{a}-{w}" for a, w in wm.PAIRS]


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as g
    g.build_hip()
    from fpqvar_amd import _lib
    return _lib.lib()


def _args(c):
    return c["a"], c["a_scales"], c["w"], c["w_scales"], c["bias"]


# ------------------------------------------------------------------------------------------------------------ the model
@pytest.mark.parametrize("pair", wm.PAIRS, ids=IDS)
def test_products_fit_the_fp32_accumulator(pair):
    """Products are multiples of 1/8 (an E2M1 side) or 1/16, the largest is the product of the tables' largest levels, and 128 of
    them have at most 24 significant bits: the exact dot fits fp32 (include/fpq.h's table)."""
    la, lw = (torch.tensor(wm.LEVELS[t], dtype=torch.float64) for t in pair)
    prod = la.view(-1, 1) * lw.view(1, -1)
    unit = 1 / 8 if pair[0] == "e2m1" else 1 / 16
    assert bool((prod / unit == (prod / unit).round()).all())
    assert float(prod.max()) == {("e2m1", "e1m2"): 10.5, ("e2m1", "e3m0"): 96.0, ("e1m2", "e1m2"): 3.0625, ("e1m2", "e3m0"): 28.0,
                                 ("e3m0", "e1m2"): 28.0, ("e3m0", "e3m0"): 256.0}[pair]
    assert 128 * float(prod.max()) / unit < 2 ** 24
    for name, (La, Lw) in wm.exact_dot_cases(*pair).items():
        assert torch.equal(wm.decode_levels(pair[0], wm.encode_levels(pair[0], La)), La + 0.0), name
        assert torch.equal(wm.decode_levels(pair[1], wm.encode_levels(pair[1], Lw)), Lw + 0.0), name


@pytest.mark.parametrize("pair", wm.PAIRS, ids=IDS)
def test_emulated_kernel_stays_inside_the_bound(pair):
    for family in wm.FAMILIES:
        for T, O, K in SHAPES:
            c = wm.make_case(*pair, family, T, O, K)
            assert c["w_scales"].dtype == torch.float32 and c["w"].shape == (O, K * 3 // 4) and c["a"].shape == (T, K // 128 * wm.SEG[pair[0]])
            r = wm.reference(*pair, *_args(c))
            out = wm.emulate(*pair, *_args(c))
            assert gm.ratio(out, r) <= 1.0, (pair, family, T, O, K)
            assert not bool(gm.class_mismatch(out, r).any()), (pair, family, T, O, K)


@pytest.mark.parametrize("mutation", list(CATCHES))
def test_every_mutation_is_caught_on_a_family(mutation):
    """each of gm.MUTATIONS exceeds 1.5 x the bound on the family that catches it for the FP4 kernel, for every pair"""
    family, (T, O, K) = CATCHES[mutation]
    for pair in wm.PAIRS:
        c = wm.make_case(*pair, family, T, O, K)
        r = wm.reference(*pair, *_args(c))
        assert gm.ratio(wm.emulate(*pair, *_args(c)), r) <= 1.0
        rat = gm.ratio(wm.emulate(*pair, *_args(c), mutation), r)
        print(f"{pair} {mutation} {family}: {rat:.3g}")
        assert rat > 1.5, (pair, mutation, family, rat)
    assert set(CATCHES) == set(wm.MUTATIONS)


@pytest.mark.parametrize("pair", wm.PAIRS, ids=IDS)
def test_families_keep_their_meaning_on_the_tables(pair):
    c = wm.make_case(*pair, "zero", 9, 136, 384)
    out = wm.emulate(*pair, *_args(c))
    want = c["bias"].view(1, 136).expand(9, 136) if c["bias"] is not None else torch.zeros(9, 136, dtype=torch.float16)
    assert torch.equal(out.view(torch.int16), want.contiguous().view(torch.int16))
    ref = wm.reference(*pair, *_args(wm.make_case(*pair, "overflow", 65, 392, 384))).out.abs()
    assert bool((ref < 65504).any()) and bool((ref > 65520).any())
    c = wm.make_case(*pair, "max_codes", 5, 8, 256)
    assert float(wm.decode_levels(pair[0], c["a"]).abs().max()) == wm.LEVELS[pair[0]][-1]
    assert float(wm.decode_levels(pair[1], c["w"]).abs().max()) == wm.LEVELS[pair[1]][-1]


# ------------------------------------------------------------------------------------------------------------ the C ABI
def test_version_and_exports(lib):
    """(the version number is pinned at 136 by tests/test_format_search_fused_host.py: the entry point is an addition a caller looks up)"""
    assert lib.fpq_version() >= 136 and hasattr(lib, "fpq_gemm_w6_mx")


def test_gemm_checks_come_before_any_launch_in_the_stated_order(lib):
    """tables, negative sizes, (the epilogue descriptor,) w_scale_dtype, shape, empty input, NULL pointers / alignment: each refusal
    wins over everything behind it (every call hands the library addresses nothing may read)"""
    from fpqvar_amd._lib import GemmEpilogue

    def call(a=PTR, sa=PTR, a_table=E3M0, w=PTR, sw=PTR, w_dtype=F32, w_table=E1M2, bias=None, out=PTR, tokens=8, outs=128, k=128, ep=None):
        return lib.fpq_gemm_w6_mx(a, sa, a_table, w, sw, w_dtype, w_table, bias, out, tokens, outs, k, ep, None)
    for at in (E2M1, E1M2, E3M0):
        for wt in (E1M2, E3M0):
            assert call(a_table=at, w_table=wt, tokens=0) == OK and call(a_table=at, w_table=wt, outs=0) == OK
    # tables first: over negative sizes, the dtype, the shape, empty input and NULL pointers
    for t in (E2M3, E3M2, 5, 99, -1):
        assert call(a_table=t) == ERR_TABLE and call(w_table=t) == ERR_TABLE, t
    assert call(w_table=E2M1) == ERR_TABLE                                   # an E2M1 weight belongs to fpq_gemm_fp4_mx / _a6w4_mx
    assert call(w_table=E2M1, tokens=-1) == ERR_TABLE and call(a_table=7, w_dtype=F16) == ERR_TABLE
    assert call(a_table=7, k=96) == ERR_TABLE and call(w_table=7, tokens=0) == ERR_TABLE and call(w_table=7, a=None) == ERR_TABLE
    # negative sizes: over the dtype, the shape and empty input
    assert call(tokens=-4) == ERR_ARG and call(outs=-8) == ERR_ARG and call(k=-128) == ERR_ARG
    assert call(tokens=-4, w_dtype=F16) == ERR_ARG and call(k=-128, outs=0) == ERR_ARG and call(outs=-8, k=96) == ERR_ARG
    # the weight scales' dtype: fp32 only - over the shape, empty input and NULL pointers
    assert call(w_dtype=F16) == ERR_DTYPE and call(w_dtype=2) == ERR_DTYPE and call(w_dtype=9) == ERR_DTYPE
    assert call(w_dtype=F16, k=96) == ERR_DTYPE and call(w_dtype=F16, tokens=0) == ERR_DTYPE and call(w_dtype=F16, w=None) == ERR_DTYPE
    # shape: over empty input and NULL pointers
    assert call(k=96) == ERR_SHAPE and call(k=128 * 65) == ERR_SHAPE and call(outs=100) == ERR_SHAPE
    assert call(tokens=1 << 31) == ERR_SHAPE and call(outs=1 << 31) == ERR_SHAPE
    assert call(k=96, tokens=0) == ERR_SHAPE and call(outs=100, a=None) == ERR_SHAPE
    # empty input: over NULL pointers and alignment
    assert call(tokens=0, a=None, out=None) == OK and call(outs=0, w=PTR + 8) == OK and call(bias=PTR + 4, tokens=0) == OK
    # NULL pointers / alignment
    assert call(k=0) == ERR_ARG
    for name in ("a", "sa", "w", "sw", "out"):
        assert call(**{name: None}) == ERR_ARG, name
    assert call(a=PTR + 8) == ERR_ARG and call(w=PTR + 8) == ERR_ARG and call(out=PTR + 8) == ERR_ARG     # 16-byte aligned
    assert call(bias=PTR + 4) == ERR_ARG and call(sa=PTR + 1) == ERR_ARG and call(sw=PTR + 2) == ERR_ARG   # the bias: 8 bytes
    # the epilogue descriptor, as in fpq_gemm_a6w4_mx: behind the sizes, in front of the dtype
    assert call(ep=ctypes.byref(GemmEpilogue(PTR + 8, None, 4))) == ERR_ARG                              # gate / residual: 16 bytes
    assert call(ep=ctypes.byref(GemmEpilogue(None, PTR + 2, 4))) == ERR_ARG
    assert call(ep=ctypes.byref(GemmEpilogue(PTR, None, 0))) == ERR_ARG                                  # rows_per_gate >= 1
    assert call(ep=ctypes.byref(GemmEpilogue(PTR, None, 0)), w_dtype=F16) == ERR_ARG
    assert call(ep=ctypes.byref(GemmEpilogue(PTR, PTR, 4)), tokens=0) == OK


# ------------------------------------------------------------------------------------------------------------ Python
def _w6_module(gemm, cls, w_table="e1m2", act="e3m0"):
    """a module with a 6-bit weight built without the quantizer (which needs the GPU)"""
    return cls(torch.zeros(64, 192, dtype=torch.uint8), torch.ones(64, 2), None, 256, 64, act, w_table)


def test_python_wrappers_refuse_before_the_library(lib):
    from fpqvar_amd import gemm
    a6, sa = torch.zeros(4, 192, dtype=torch.uint8), torch.zeros(4, 2, dtype=torch.float16)
    w6, sw = torch.zeros(8, 192, dtype=torch.uint8), torch.zeros(8, 2)
    with pytest.raises(RuntimeError, match="GPU"):
        gemm.linear_w6(a6, sa, "e3m0", w6, sw, "e1m2")
    assert set(gemm._W6_FORMATS) == set(wm.PAIRS)
    for (a, w), fmt in gemm._W6_FORMATS.items():
        assert (fmt.seg, fmt.w_seg, fmt.gemm + "_mx" + fmt.plain) == (wm.SEG[a], 96, "fpq_gemm_w6_mx")
        assert fmt.table == (gemm.TABLE_IDS[a],) and fmt.w_table == (gemm.TABLE_IDS[w],)
    for fmt in gemm._FORMATS.values():                                       # the E2M1-weight rows are what they were
        assert fmt.w_seg == 64 and fmt.w_table == ()


def test_fp4linear_refuses_what_a_6bit_weight_has_no_form_for(lib):
    from fpqvar_amd import gemm
    lin = torch.nn.Linear(256, 64)
    for w in ("fp_e1", "fp_e3"):
        with pytest.raises(ValueError, match="no k-major form"):
            gemm.FP4Linear.from_float(lin, kmajor=True, weight_fp_type=w)
        with pytest.raises(ValueError, match="no k-major form"):
            gemm.FP4Linear.from_float(lin, kmajor=True, a6w4_kmajor=True, act_fp_type="fp_e3", weight_fp_type=w)
        with pytest.raises(ValueError, match="no k-major form"):
            gemm.FP4Linear.from_float(lin, a6w4_kmajor=True, weight_fp_type=w)
        with pytest.raises(ValueError, match="no fc1 tail"):
            gemm.FP4LinearGeluDual.from_float(lin, weight_fp_type=w)
    with pytest.raises(ValueError, match="weight_fp_type must be"):
        gemm.FP4Linear.from_float(lin, weight_fp_type="fp6_e2m3")
    m = _w6_module(gemm, gemm.FP4Linear)
    assert m.w_table == "e1m2" and not m.kmajor and "act=e3m0, w=e1m2" in m.extra_repr()
    cache = torch.zeros(2, 1, 8, 1, 64, dtype=torch.float16)
    with pytest.raises(ValueError, match="plain form only"):
        m.qkv_to_cache(torch.zeros(1, 4, 256), cache, 0, 4)
    with pytest.raises(ValueError, match="plain form only"):
        m.qkv_to_cache_operands(torch.zeros(4, 192, dtype=torch.uint8), torch.zeros(4, 2, dtype=torch.float16), cache, 0, 4)
    d = _w6_module(gemm, gemm.FP4LinearGeluDual)
    with pytest.raises(ValueError, match="plain form only"):
        d(torch.zeros(4, 256))
    with pytest.raises(ValueError, match="plain form only"):
        d.forward_operands(torch.zeros(4, 192, dtype=torch.uint8), torch.zeros(4, 2, dtype=torch.float16))
    # the default is what it was: an E2M1 weight, named as before
    assert "w=e2m1" in gemm.FP4Linear(torch.zeros(64, 128, dtype=torch.uint8), torch.ones(64, 2), None, 256, 64).extra_repr()


# ------------------------------------------------------------------------------------------------------------ the wiring
class _Marker(torch.nn.Module):
    def __init__(self, kmajor, act, weight):
        super().__init__()
        self.kmajor_arg, self.act, self.weight_type = kmajor, act, weight


@pytest.fixture
def cpu_construction(monkeypatch):
    """Quantizing a weight needs the GPU: on the CPU the weight quantizer is an identity and FP4Linear.from_float records its
    arguments, so the walk - which layer becomes what - runs as it is."""
    from fpqvar_amd import gemm, quant_linear as ql
    monkeypatch.setattr(ql, "_quantize_weight", lambda w, *a, **k: w)
    monkeypatch.setattr(gemm.FP4Linear, "from_float",
                        classmethod(lambda cls, lin, kmajor=False, act_fp_type="fp_e2", a6w4_kmajor=False, weight_fp_type="fp_e2":
                                    _Marker(kmajor, act_fp_type, weight_fp_type)))
    return ql


FP = ("fp_e1", "fp_e2", "fp_e3")
LAYERS = ("fc1", "mat_qkv", "proj")


def _formats(b, layer):
    """3 x 3: block b = 3 i + j has activation format FP[i] and weight format FP[j] on fc1, mat_qkv and proj; fc2 is the dual format
    on an E2M1 weight in even blocks and the block's own pair in odd ones"""
    if layer == "fc2" and b % 2 == 0:
        return ("fp_e1m2_neg_e2m1_pos", "fp_e2")
    return (FP[b // 3], FP[b % 3])


def _classes(model):
    return {n: type(m).__name__ for n, m in model.named_modules() if not list(m.children()) or isinstance(m, _Marker)}


def test_w6_weights_routes_the_format_table(cpu_construction):
    ql = cpu_construction
    kw = {k: v for k, v in W4A4.items() if k not in ("act_fp_type", "weight_fp_type", "fc2_fp_type")}
    torch.manual_seed(0)
    today = ql.quantize_VAR_mixed(_Var(128, 9), _formats, real_fp4=True, **kw)
    off = ql.quantize_VAR_mixed(_Var(128, 9), _formats, real_fp4=True, w6_weights=False, **kw)
    assert _classes(off) == _classes(today)                                  # without the keyword: exactly today's module types
    for b, blk in enumerate(today.blocks):
        for name in LAYERS:
            m = blk.attn.get_submodule(name) if name != "fc1" else blk.ffn.fc1
            if FP[b % 3] == "fp_e2":
                assert isinstance(m, _Marker) and m.act == FP[b // 3] and m.weight_type == "fp_e2", (b, name)
            else:
                assert type(m) is ql.QuantizedLinear, (b, name)
    on = ql.quantize_VAR_mixed(_Var(128, 9), _formats, real_fp4=True, w6_weights=True, ada_lin_formats=("fp_e2", "fp_e1"), **kw)
    for b, blk in enumerate(on.blocks):
        a, w = FP[b // 3], FP[b % 3]
        for name in LAYERS:
            m = blk.attn.get_submodule(name) if name != "fc1" else blk.ffn.fc1
            assert isinstance(m, _Marker) and (m.act, m.weight_type) == (a, w), (b, name)
            assert m.kmajor_arg == (a == "fp_e2" and w == "fp_e2"), (b, name)        # a 6-bit weight is row-major
        # fc2 and ada_lin[1] are as without the keyword
        assert type(blk.ffn.fc2).__name__ == type(today.blocks[b].ffn.fc2).__name__, b
        assert type(blk.ada_lin[1]) is ql.QuantizedLinear
    # a shape the GEMM does not take stays a QuantizedLinear
    odd = _Var(128, 1)
    odd.blocks[0].ffn.fc1 = torch.nn.Linear(192, 512)
    odd.blocks[0].attn.proj = torch.nn.Linear(128, 100)
    m = ql.quantize_VAR_mixed(odd, lambda b, layer: ("fp_e3", "fp_e1") if layer != "fc2" else ("fp_e1m2_neg_e2m1_pos", "fp_e2"),
                              real_fp4=True, w6_weights=True, **kw)
    assert type(m.blocks[0].ffn.fc1) is ql.QuantizedLinear and type(m.blocks[0].attn.proj) is ql.QuantizedLinear
    assert isinstance(m.blocks[0].attn.mat_qkv, _Marker) and m.blocks[0].attn.mat_qkv.weight_type == "fp_e1"
    with pytest.raises(ValueError, match="w6_weights needs real_fp4"):
        ql.quantize_VAR_mixed(_Var(128, 1), _formats, w6_weights=True, **kw)


def test_w6_weights_and_fuse_ffn(cpu_construction):
    """an FFN whose fc1 has a 6-bit weight has no in-GEMM tail: the one-pass GeluThenFc2Quant route"""
    ql = cpu_construction
    kw = {k: v for k, v in W4A4.items() if k not in ("act_fp_type", "weight_fp_type", "fc2_fp_type")}

    def fmt(b, layer):
        return ("fp_e1m2_neg_e2m1_pos", "fp_e2") if layer == "fc2" else ("fp_e3", "fp_e3" if b == 0 else "fp_e2")
    m = ql.quantize_VAR_mixed(_Var(128, 2), fmt, real_fp4=True, w6_weights=True, fuse_ffn=True, **kw)
    f0, f1 = m.blocks[0].ffn, m.blocks[1].ffn
    assert isinstance(f0.fc1, _Marker) and f0.fc1.weight_type == "fp_e3" and type(f0.act) is ql.GeluThenFc2Quant
    assert isinstance(f1.fc1, _Marker) and f1.fc1.weight_type == "fp_e2" and type(f1.act) is torch.nn.Identity     # in fc1's epilogue, as today


@pytest.mark.parametrize("fn", ("quantize_VAR_mixed_fp4_datatype", "quantize_VAR_use_different_datatype"))
def test_the_wrappers_pass_the_keyword(cpu_construction, fn):
    ql = cpu_construction
    kw = dict(W4A4, weight_fp_type="fp_e1")
    off = getattr(ql, fn)(_Var(128, 2), real_fp4=True, **kw)
    on = getattr(ql, fn)(_Var(128, 2), real_fp4=True, w6_weights=True, **kw)
    for b in range(2):
        assert type(off.blocks[b].attn.proj) is ql.QuantizedLinear
        p = on.blocks[b].attn.proj
        assert isinstance(p, _Marker) and (p.act, p.weight_type, p.kmajor_arg) == ("fp_e2", "fp_e1", False)
        assert isinstance(on.blocks[b].ffn.fc1, _Marker) and on.blocks[b].ffn.fc1.weight_type == "fp_e2"
