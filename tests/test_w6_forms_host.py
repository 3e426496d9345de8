"""The W6 GEMM's fc1 tail and split output (fpq_gemm_w6_gelu_dual, fpq_gemm_w6_mx_split, fpq_gemm_w6_mx_split_qknorm;
gemm.linear_w6_gelu_dual, gemm.linear_w6_qkv_to_cache; FP4Linear(..., w6_forms=True); quantize_VAR_mixed(..., w6_forms=True)) without a
GPU, after tests/test_a6w4_fc1_host.py and tests/test_a6w4_qkv_split_host.py: the three entry points' export, declaration, ctypes
signature and argument checks in their documented order (null or fake pointers - nothing is launched), the Python wrappers'
refusals, and - construction only, with marker classes - which layer of a 6-bit-weight model becomes what with and without the
keyword."""
import ctypes
import os
import re

import pytest
import torch

from tests import w6_model as wm
from tests.test_a6w4_host import W4A4, _Var

OK, ERR_ARG, ERR_DTYPE, ERR_SHAPE, ERR_TABLE = 0, -1, -2, -3, -4
F16, F32 = 0, 1
E2M1, E1M2, E3M0, E2M3, E3M2 = 0, 1, 2, 3, 4   # enum fpq_table
PTR = 0x7000_0000_1000   # an address with every alignment the checks ask for; nothing reads it
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("fpq_gemm_w6_gelu_dual", "fpq_gemm_w6_mx_split", "fpq_gemm_w6_mx_split_qknorm")
A_IDS, W_IDS = (E2M1, E1M2, E3M0), (E1M2, E3M0)


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as g
    g.build_hip()
    from fpqvar_amd import _lib
    return _lib.lib()


# ------------------------------------------------------------------------------------------------------------ the C ABI
def test_exports_declarations_and_signatures(lib):
    """(FPQ_VERSION stays 136 - tests/test_format_search_fused_host.py pins it: the entry points are additions a caller looks up)"""
    from fpqvar_amd import _lib
    assert lib.fpq_version() == 136
    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "fpq.h")).read(), flags=re.S)
    for name in NEW:
        assert hasattr(lib, name), name
        assert name in _lib._SIGS, name
        assert re.search(r"\bint\s+" + name + r"\s*\(", hdr), f"{name} is not declared in include/fpq.h"
    i, p, q = ctypes.c_int, ctypes.c_void_p, ctypes.c_int64
    assert _lib._SIGS["fpq_gemm_w6_gelu_dual"] == (i, [p, p, i, p, p, i, i, p, p, p, q, q, q, p, p])
    assert _lib._SIGS["fpq_gemm_w6_mx_split"] == (i, [p, p, i, p, p, i, i, p, q, q, q, p, p])            # no kmajor flag
    assert _lib._SIGS["fpq_gemm_w6_mx_split_qknorm"] == (i, [p, p, i, p, p, i, i, p, q, q, q, p, p, p])


def test_gelu_dual_checks_in_the_documented_order(lib):
    """tables, negative sizes, w_scale_dtype (fp32 only), shape, empty problem, then NULL pointers / alignment: each refusal wins
    over everything behind it"""
    def call(a=PTR, sa=PTR, a_table=E3M0, w=PTR, sw=PTR, w_dtype=F32, w_table=E1M2, bias=None, out=PTR, h=None, tokens=8, outs=128, k=128,
             flag=None):
        return lib.fpq_gemm_w6_gelu_dual(a, sa, a_table, w, sw, w_dtype, w_table, bias, out, h, tokens, outs, k, flag, None)
    for at in A_IDS:
        for wt in W_IDS:
            assert call(a_table=at, w_table=wt, tokens=0) == OK and call(a_table=at, w_table=wt, outs=0) == OK
    # tables first
    for t in (E2M3, E3M2, 5, 99, -1):
        assert call(a_table=t) == ERR_TABLE and call(w_table=t) == ERR_TABLE, t
    assert call(w_table=E2M1) == ERR_TABLE                                   # an E2M1 weight belongs to the FP4 / A6W4 entry points
    assert call(w_table=E2M1, tokens=-1) == ERR_TABLE and call(a_table=7, w_dtype=F16) == ERR_TABLE
    assert call(a_table=7, outs=100) == ERR_TABLE and call(w_table=7, tokens=0) == ERR_TABLE and call(w_table=7, a=None) == ERR_TABLE
    # negative sizes: over the dtype, the shape and the empty problem
    assert call(tokens=-4) == ERR_ARG and call(outs=-128) == ERR_ARG and call(k=-128) == ERR_ARG
    assert call(tokens=-4, w_dtype=F16) == ERR_ARG and call(k=-128, outs=0) == ERR_ARG and call(outs=-128, k=96) == ERR_ARG
    # the weight scales' dtype: fp32 only
    assert call(w_dtype=F16) == ERR_DTYPE and call(w_dtype=2) == ERR_DTYPE and call(w_dtype=9) == ERR_DTYPE
    assert call(w_dtype=F16, k=96) == ERR_DTYPE and call(w_dtype=F16, tokens=0) == ERR_DTYPE and call(w_dtype=F16, w=None) == ERR_DTYPE
    # shape: k % 128, k > 8192, outs % 128 (an output tile is one quantization group)
    assert call(k=96) == ERR_SHAPE and call(k=128 * 65) == ERR_SHAPE and call(outs=100) == ERR_SHAPE and call(outs=8) == ERR_SHAPE
    assert call(outs=192) == ERR_SHAPE and call(tokens=1 << 31) == ERR_SHAPE and call(outs=1 << 31) == ERR_SHAPE
    assert call(k=96, tokens=0) == ERR_SHAPE and call(outs=100, a=None) == ERR_SHAPE
    assert call(k=128 * 64, a=None) == ERR_ARG                               # the longest K still fits the LDS: on to the pointers
    # the empty problem: over NULL pointers and alignment
    assert call(tokens=0, a=None, out=None) == OK and call(outs=0, w=PTR + 8) == OK
    assert call(bias=PTR + 4, h=PTR + 8, flag=PTR + 4, tokens=0) == OK
    # NULL pointers / alignment
    assert call(k=0) == ERR_ARG
    for name in ("a", "sa", "w", "sw", "out"):
        assert call(**{name: None}) == ERR_ARG, name
    assert call(a=PTR + 8) == ERR_ARG and call(w=PTR + 8) == ERR_ARG and call(out=PTR + 8) == ERR_ARG
    assert call(h=PTR + 8) == ERR_ARG and call(flag=PTR + 4) == ERR_ARG      # a misaligned gelu_out (16 bytes) / nan_flag (8)
    assert call(bias=PTR + 4) == ERR_ARG and call(sa=PTR + 1) == ERR_ARG and call(sw=PTR + 2) == ERR_ARG


def _split(n_parts=3, part_cols=128, rpb=4, out=(PTR, PTR, PTR), stride=None):
    from fpqvar_amd._lib import GemmSplit
    sp = GemmSplit()
    sp.part_cols, sp.n_parts, sp.rows_per_batch = part_cols, n_parts, rpb
    for p in range(3):
        sp.out[p], sp.row_stride[p], sp.batch_stride[p], sp.row0[p] = out[p], part_cols if stride is None else stride, rpb, 0
    return sp


_DEFAULT = object()


def _split_call(lib, norm):
    """the entry point with harmless defaults: 8 tokens (two batch entries of 4), three parts of 128 columns, k = 128"""
    def call(a=None, sa=None, a_table=E3M0, w=None, sw=None, w_dtype=F32, w_table=E1M2, bias=None, tokens=8, outs=384, k=128, split=_DEFAULT,
             hs=PTR):
        sp = _split() if split is _DEFAULT else split
        ref = None if sp is None else ctypes.byref(sp)
        if norm:
            return lib.fpq_gemm_w6_mx_split_qknorm(a, sa, a_table, w, sw, w_dtype, w_table, bias, tokens, outs, k, ref, hs, None)
        return lib.fpq_gemm_w6_mx_split(a, sa, a_table, w, sw, w_dtype, w_table, bias, tokens, outs, k, ref, None)
    return call


@pytest.mark.parametrize("norm", (False, True))
def test_split_checks_in_the_documented_order(lib, norm):
    """tables; NULL split (and the norm form's own arguments); negative sizes; the split descriptor; the scale dtype; shape; the empty
    problem; then pointers / alignment - every call here has NULL operands, so reaching the pointers is FPQ_ERR_ARG"""
    call = _split_call(lib, norm)
    assert call() == ERR_ARG and call(tokens=0) == OK
    for at in A_IDS:
        for wt in W_IDS:
            assert call(a_table=at, w_table=wt, tokens=0) == OK
    for kw in (dict(a_table=E2M3), dict(a_table=99), dict(a_table=-1), dict(w_table=E2M1), dict(w_table=E3M2), dict(w_table=5)):
        assert call(**kw) == ERR_TABLE and call(**kw, split=None) == ERR_TABLE and call(**kw, tokens=-1) == ERR_TABLE, kw
        assert call(**kw, split=_split(n_parts=0)) == ERR_TABLE and call(**kw, w_dtype=F16) == ERR_TABLE, kw
        assert call(**kw, k=96) == ERR_TABLE and call(**kw, tokens=0) == ERR_TABLE, kw
        if norm:
            assert call(**kw, hs=None) == ERR_TABLE, kw
    # NULL split, before the sizes, the dtype and the shape
    assert call(split=None) == ERR_ARG and call(split=None, tokens=0) == ERR_ARG and call(split=None, w_dtype=F16) == ERR_ARG
    assert call(split=None, k=96) == ERR_ARG
    # negative sizes
    assert call(tokens=-1, w_dtype=F16) == ERR_ARG and call(outs=-384, k=96) == ERR_ARG and call(k=-128, w_dtype=F16) == ERR_ARG
    # the split descriptor, before the dtype and the shape
    for bad in (dict(split=_split(n_parts=0), outs=0), dict(split=_split(n_parts=4), outs=512),
                dict(split=_split(part_cols=100), outs=300),                       # part_cols % 128
                dict(outs=256), dict(outs=512),                                    # outs != n_parts * part_cols
                dict(tokens=6), dict(split=_split(rpb=3)), dict(split=_split(rpb=0)),   # tokens: not whole batch entries
                dict(split=_split(out=(None, PTR, PTR))), dict(split=_split(out=(PTR, None, PTR))), dict(split=_split(out=(PTR, PTR, None))),
                dict(split=_split(out=(PTR + 4, PTR, PTR))), dict(split=_split(out=(PTR, PTR + 4, PTR))),   # a part misaligned by 4 bytes
                dict(split=_split(out=(PTR, PTR, PTR + 4))),
                dict(split=_split(stride=64)), dict(split=_split(stride=130))):
        assert call(**bad) == ERR_ARG, bad
        assert call(**bad, w_dtype=F16) == ERR_ARG and call(**bad, k=96) == ERR_ARG, bad
    if norm:
        assert call(split=_split(n_parts=2), outs=256) == ERR_ARG and call(split=_split(n_parts=1), outs=128) == ERR_ARG
        assert call(split=_split(n_parts=2), outs=256, w_dtype=F16) == ERR_ARG
    else:   # one or two parts are fine here: on to the pointers
        assert call(split=_split(n_parts=2), outs=256) == ERR_ARG and call(split=_split(n_parts=2), outs=256, tokens=0) == OK
        assert call(split=_split(n_parts=1), outs=128, tokens=0) == OK
    assert call(split=_split(out=(PTR + 8, PTR + 8, PTR + 8)), tokens=0) == OK     # every part 8-byte aligned is enough
    # fp16 weight scales: not compiled - before the shape and the empty problem
    assert call(w_dtype=F16) == ERR_DTYPE and call(w_dtype=F16, k=96) == ERR_DTYPE and call(w_dtype=F16, tokens=0) == ERR_DTYPE
    assert call(w_dtype=7) == ERR_DTYPE
    # shape
    assert call(k=96) == ERR_SHAPE and call(k=128 * 65) == ERR_SHAPE and call(k=96, tokens=0) == ERR_SHAPE
    assert call(tokens=1 << 31, split=_split(rpb=1 << 20)) == ERR_SHAPE
    assert call(tokens=1 << 28, split=_split(rpb=1 << 20)) == ERR_ARG              # row-major: no 2^28 limit, on to the pointers
    assert call(k=0) == ERR_ARG
    assert call(tokens=0, split=_split(rpb=7)) == OK


@pytest.mark.parametrize("norm", (False, True))
def test_split_pointer_and_alignment_checks(lib, norm):
    base = _split_call(lib, norm)

    def call(**kw):
        return base(**{**dict(a=PTR, sa=PTR, w=PTR, sw=PTR), **kw})
    for name in ("a", "sa", "w", "sw"):
        assert call(**{name: None}) == ERR_ARG, name
    assert call(a=PTR + 8) == ERR_ARG and call(w=PTR + 8) == ERR_ARG
    assert call(sa=PTR + 1) == ERR_ARG and call(sw=PTR + 2) == ERR_ARG
    if norm:   # the norm form's own arguments are refused whatever else is passed - the empty problem included
        assert call(hs=None) == ERR_ARG and call(hs=PTR + 2) == ERR_ARG and call(hs=None, tokens=0) == ERR_ARG
        assert call(bias=PTR + 8) == ERR_ARG and call(bias=PTR + 4) == ERR_ARG and call(bias=PTR + 8, tokens=0) == ERR_ARG
        assert call(a=PTR + 8, w=PTR + 8, sa=PTR + 1, sw=PTR + 2, bias=PTR + 16, tokens=0) == OK
    else:
        assert call(bias=PTR + 4) == ERR_ARG
        assert call(a=PTR + 8, w=PTR + 8, sa=PTR + 1, sw=PTR + 2, bias=PTR + 4, tokens=0) == OK


# ------------------------------------------------------------------------------------------------------------ the wrappers
def _operands(a_table="e3m0", tokens=8, outs=384, k=128):
    return (torch.zeros(tokens, k // 128 * wm.SEG[a_table], dtype=torch.uint8), torch.zeros(tokens, k // 128, dtype=torch.float16),
            torch.zeros(outs, k * 3 // 4, dtype=torch.uint8), torch.zeros(outs, k // 128))


def _cache(bsz=2, max_len=10, heads=2, hd=64, dtype=torch.float16):
    return torch.zeros(2, bsz, max_len, heads, hd, dtype=dtype)


def test_python_wrappers_refuse_cpu_tensors(lib):
    from fpqvar_amd import gemm
    a, sa, w, sw = _operands()
    with pytest.raises(RuntimeError, match="GPU"):
        gemm.linear_w6_gelu_dual(a, sa, "e3m0", w, sw, "e1m2")
    with pytest.raises(RuntimeError, match="GPU"):
        gemm.linear_w6_qkv_to_cache(a, sa, "e3m0", w, sw, "e1m2", None, _cache(), 0, 4)
    for fmt in gemm._W6_FORMATS.values():                                    # float32 weight scales only, in every form
        assert fmt.split_w_f32 and fmt.gemm == "fpq_gemm_w6"


def test_python_wrappers_refusals_behind_the_gpu_check(lib, monkeypatch):
    """the refusals behind the GPU test, reached on CPU tensors with that test switched off; the messages of the A6W4 twins"""
    from fpqvar_amd import gemm
    monkeypatch.setattr(gemm, "require_gpu", lambda *a, **k: None)
    a, sa, w, sw = _operands(outs=128)
    fc1 = gemm.linear_w6_gelu_dual
    with pytest.raises(RuntimeError, match="row-major operands only"):
        fc1(a.view(1, 8, 96), sa, "e3m0", w.view(1, 128, 96), sw, "e1m2")
    with pytest.raises(RuntimeError, match="'e1m2' and 'e3m0'"):
        fc1(a, sa, "e3m0", w, sw, "e2m1")                                     # an E2M1 weight table
    with pytest.raises(RuntimeError, match="'e1m2' and 'e3m0'"):
        fc1(a, sa, "e2m3", w, sw, "e1m2")
    with pytest.raises(RuntimeError, match="weight scales must be float32"):
        fc1(a, sa, "e3m0", w, sw.half(), "e1m2")
    with pytest.raises(RuntimeError, match="multiple of 128"):
        fc1(a, sa, "e3m0", w[:120], sw[:120], "e1m2")
    with pytest.raises(RuntimeError, match="mismatch"):
        fc1(a[:, :64], sa, "e3m0", w, sw, "e1m2")
    a, sa, w, sw = _operands()
    go = lambda cache, pos=0, seq=4, bias=None, hs=None, sw_=sw: gemm.linear_w6_qkv_to_cache(a, sa, "e3m0", w, sw_, "e3m0", bias, cache, pos, seq, hs)
    for cache in (_cache(dtype=torch.float32), _cache()[0], _cache()[:, :, :, :, :32]):
        with pytest.raises(RuntimeError, match=r"contiguous float16 \[2, B, max_len, H, c\]"):
            go(cache)
    with pytest.raises(RuntimeError, match="do not fit"):                   # pos + seq > max_len
        go(_cache(), pos=7)
    with pytest.raises(RuntimeError, match="do not fit|row-major|mismatch"):     # a cache of the wrong width
        go(_cache(heads=4))
    with pytest.raises(RuntimeError, match="weight scales must be float32"):
        go(_cache(), sw_=sw.half())
    with pytest.raises(RuntimeError, match="qk_norm_scale must be"):
        go(_cache(), hs=torch.ones(3))
    with pytest.raises(RuntimeError, match="the bias must be a float32"):
        go(_cache(), hs=torch.ones(2), bias=torch.zeros(384, dtype=torch.float16))


def _w6_module(gemm, cls, w_table="e1m2", act="e3m0", outs=384, **kw):
    """a module with a 6-bit weight built without the quantizer (which needs the GPU)"""
    return cls(torch.zeros(outs, 96, dtype=torch.uint8), torch.ones(outs, 1), None, 128, outs, act, w_table, **kw)


def test_fp4linear_default_keeps_the_pinned_refusals(lib):
    """w6_forms=False (the default, spelled out or not): the three messages tests/test_w6_host.py pins; w6_forms=True: k-major still
    raises, the fc1 module constructs, the forms reach the GEMM's own GPU check"""
    from fpqvar_amd import gemm
    lin = torch.nn.Linear(128, 384)
    x, cache = torch.zeros(2, 4, 128), _cache()
    ac, asc = torch.zeros(8, 96, dtype=torch.uint8), torch.zeros(8, 1, dtype=torch.float16)
    for kw in ({}, {"w6_forms": False}):
        for w in ("fp_e1", "fp_e3"):
            with pytest.raises(ValueError, match="no fc1 tail"):
                gemm.FP4LinearGeluDual.from_float(lin, weight_fp_type=w, **kw)
            with pytest.raises(ValueError, match="no k-major form"):
                gemm.FP4Linear.from_float(lin, kmajor=True, weight_fp_type=w, **kw)
        m = _w6_module(gemm, gemm.FP4Linear, **kw)
        assert m.w6_forms is False
        with pytest.raises(ValueError, match="plain form only"):
            m.qkv_to_cache(x, cache, 0, 4)
        with pytest.raises(ValueError, match="plain form only"):
            m.qkv_to_cache_operands(ac, asc, cache, 0, 4)
        with pytest.raises(ValueError, match="plain form only"):
            m._run("qkv_to_cache", None, ac, asc, None, cache, 0, 4, None)
        d = _w6_module(gemm, gemm.FP4LinearGeluDual, **kw)
        with pytest.raises(ValueError, match="plain form only"):
            d(torch.zeros(4, 128))
        with pytest.raises(ValueError, match="plain form only"):
            d.forward_operands(ac, asc)
    for w in ("fp_e1", "fp_e3"):                                             # k-major remains unbuilt for a 6-bit weight
        for kw in (dict(kmajor=True), dict(a6w4_kmajor=True), dict(kmajor=True, a6w4_kmajor=True, act_fp_type="fp_e3")):
            with pytest.raises(ValueError, match="no k-major form"):
                gemm.FP4Linear.from_float(lin, weight_fp_type=w, w6_forms=True, **kw)
            with pytest.raises(ValueError, match="no k-major form"):
                gemm.FP4LinearGeluDual.from_float(lin, weight_fp_type=w, w6_forms=True, **kw)
    m = _w6_module(gemm, gemm.FP4Linear, w6_forms=True)
    d = _w6_module(gemm, gemm.FP4LinearGeluDual, w6_forms=True)
    assert m.w6_forms and d.w6_forms
    with pytest.raises(RuntimeError, match="GPU"):                           # past the module's refusals: on to the quantizer / the GEMM
        m.qkv_to_cache(x, cache, 0, 4)
    with pytest.raises(RuntimeError, match="linear_w6_qkv_to_cache.*GPU|GPU.*linear_w6_qkv_to_cache"):
        m.qkv_to_cache_operands(ac, asc, cache, 0, 4)
    with pytest.raises(RuntimeError, match="linear_w6_gelu_dual.*GPU|GPU.*linear_w6_gelu_dual"):
        d.forward_operands(ac, asc)
    biased = gemm.FP4Linear(torch.zeros(384, 96, dtype=torch.uint8), torch.ones(384, 1), torch.zeros(384, dtype=torch.float16), 128, 384, "e3m0",
                            "e1m2", w6_forms=True)
    with pytest.raises(RuntimeError, match="must have no bias"):             # a module bias together with the q / k norm
        biased.qkv_to_cache(x, cache, 0, 4, qk_norm_scale=torch.ones(2))


# ------------------------------------------------------------------------------------------------------------ the wiring
class _Marker(torch.nn.Module):
    def __init__(self, cls, kmajor, act, weight, w6_forms):
        super().__init__()
        self.cls_name, self.kmajor_arg, self.act, self.weight_type, self.w6_forms = cls.__name__, kmajor, act, weight, w6_forms


@pytest.fixture
def cpu_construction(monkeypatch):
    """Quantizing a weight needs the GPU: on the CPU the weight quantizer is an identity and FP4Linear.from_float (which
    FP4LinearGeluDual inherits) records the class it was asked for and its arguments, so the walk runs as it is."""
    from fpqvar_amd import gemm, quant_linear as ql
    monkeypatch.setattr(ql, "_quantize_weight", lambda w, *a, **k: w)
    monkeypatch.setattr(gemm.FP4Linear, "from_float",
                        classmethod(lambda cls, lin, kmajor=False, act_fp_type="fp_e2", a6w4_kmajor=False, weight_fp_type="fp_e2",
                                    w6_forms=False: _Marker(cls, kmajor, act_fp_type, weight_fp_type, w6_forms)))
    return ql


FP = ("fp_e1", "fp_e2", "fp_e3")
MK = {k: v for k, v in W4A4.items() if k not in ("act_fp_type", "weight_fp_type", "fc2_fp_type")}


def _formats(b, layer):
    """3 x 3: block b = 3 i + j has activation format FP[i] and weight format FP[j] on fc1, mat_qkv and proj; fc2 takes the dual
    format on an E2M1 weight"""
    if layer == "fc2":
        return ("fp_e1m2_neg_e2m1_pos", "fp_e2")
    return (FP[b // 3], FP[b % 3])


def _classes(model):
    return {n: (m.cls_name, m.kmajor_arg, m.act, m.weight_type) if isinstance(m, _Marker) else type(m).__name__
            for n, m in model.named_modules() if not list(m.children()) or isinstance(m, _Marker)}


def test_w6_forms_routes_fc1_to_the_gelu_dual_module_for_all_six_pairs(cpu_construction):
    ql = cpu_construction
    torch.manual_seed(0)
    on = ql.quantize_VAR_mixed(_Var(128, 9), _formats, real_fp4=True, w6_weights=True, w6_forms=True, fuse_ffn=True, **MK)
    x = torch.randn(3, 512)
    six = set()
    for b, blk in enumerate(on.blocks):
        a, w = FP[b // 3], FP[b % 3]
        fc1 = blk.ffn.fc1
        assert isinstance(fc1, _Marker) and fc1.cls_name == "FP4LinearGeluDual" and (fc1.act, fc1.weight_type) == (a, w), (b, fc1.cls_name)
        assert isinstance(blk.ffn.act, torch.nn.Identity), b
        assert type(blk.ffn.fc2) is ql.QuantizedLinear_fc2 and blk.ffn.fc2.act_quant_name == "in fc1's epilogue" and blk.ffn.fc2.act_quant(x) is x
        if w != "fp_e2":
            six.add((a, w))
            assert fc1.w6_forms is True and fc1.kmajor_arg is False, b
        for name in ("mat_qkv", "proj"):
            m = blk.attn.get_submodule(name)
            assert isinstance(m, _Marker) and m.cls_name == "FP4Linear" and (m.act, m.weight_type) == (a, w), (b, name)
            assert m.w6_forms is (w != "fp_e2"), (b, name)                   # an E2M1 weight is built as before
    assert len(six) == 6
    # without fuse_ffn: the same FP4Linear modules with the flag, act and fc2 untouched
    nofuse = ql.quantize_VAR_mixed(_Var(128, 9), _formats, real_fp4=True, w6_weights=True, w6_forms=True, **MK)
    for b, blk in enumerate(nofuse.blocks):
        assert blk.ffn.fc1.cls_name == "FP4Linear" and blk.ffn.fc1.w6_forms is (FP[b % 3] != "fp_e2") and isinstance(blk.ffn.act, torch.nn.GELU)
    # an fc1 whose width is no multiple of 128, or an fc2 format the tail does not compute: the one-pass route, as without the keyword
    odd = _Var(128, 1)
    odd.blocks[0].ffn.fc1 = torch.nn.Linear(128, 200)
    odd.blocks[0].ffn.fc2 = torch.nn.Linear(200, 128)
    with pytest.raises(ValueError, match="fuse_ffn needs"):
        ql.quantize_VAR_mixed(odd, lambda b, layer: ("fp_e3", "fp_e1") if layer != "fc2" else ("fp_e1m2_neg_e2m1_pos", "fp_e2"),
                              real_fp4=True, w6_weights=True, w6_forms=True, fuse_ffn=True, **MK)
    m = ql.quantize_VAR_mixed(_Var(128, 1), lambda b, layer: ("fp_e3", "fp_e1") if layer != "fc2" else ("fp4_afpq", "fp_e2"),
                              real_fp4=True, w6_weights=True, w6_forms=True, fuse_ffn=True, **MK)
    assert m.blocks[0].ffn.fc1.cls_name == "FP4Linear" and type(m.blocks[0].ffn.act) is ql.GeluThenFc2Quant


def test_without_w6_forms_the_module_types_are_todays(cpu_construction, monkeypatch):
    """default / w6_forms=False: the same classes and arguments, the GeluThenFc2Quant route for a 6-bit-weight fc1 - and from_float is
    called with today's keyword list (a from_float without the new keyword still serves)"""
    ql = cpu_construction
    from fpqvar_amd import gemm
    for fuse in (False, True):
        torch.manual_seed(0)
        today = ql.quantize_VAR_mixed(_Var(128, 9), _formats, real_fp4=True, w6_weights=True, fuse_ffn=fuse, **MK)
        off = ql.quantize_VAR_mixed(_Var(128, 9), _formats, real_fp4=True, w6_weights=True, w6_forms=False, fuse_ffn=fuse, **MK)
        assert _classes(off) == _classes(today)
        for b, blk in enumerate(off.blocks):
            assert blk.ffn.fc1.w6_forms is False and blk.attn.mat_qkv.w6_forms is False
            if fuse and FP[b % 3] != "fp_e2":
                assert blk.ffn.fc1.cls_name == "FP4Linear" and type(blk.ffn.act) is ql.GeluThenFc2Quant, b
    old = classmethod(lambda cls, lin, kmajor=False, act_fp_type="fp_e2", a6w4_kmajor=False, weight_fp_type="fp_e2":
                      _Marker(cls, kmajor, act_fp_type, weight_fp_type, None))
    monkeypatch.setattr(gemm.FP4Linear, "from_float", old)
    m = ql.quantize_VAR_mixed(_Var(128, 9), _formats, real_fp4=True, w6_weights=True, fuse_ffn=True, **MK)
    assert all(isinstance(blk.ffn.fc1, _Marker) for blk in m.blocks)


def test_w6_forms_needs_w6_weights(cpu_construction):
    ql = cpu_construction
    with pytest.raises(ValueError, match="w6_forms needs w6_weights"):
        ql.quantize_VAR_mixed(_Var(128, 1), _formats, real_fp4=True, w6_forms=True, **MK)
    with pytest.raises(ValueError, match="w6_weights needs real_fp4"):
        ql.quantize_VAR_mixed(_Var(128, 1), _formats, w6_weights=True, w6_forms=True, **MK)
    for fn in (ql.quantize_VAR_mixed_fp4_datatype, ql.quantize_VAR_use_different_datatype):
        with pytest.raises(ValueError, match="w6_forms needs w6_weights"):
            fn(_Var(128, 1), real_fp4=True, w6_forms=True, **W4A4)


@pytest.mark.parametrize("fn", ("quantize_VAR_mixed_fp4_datatype", "quantize_VAR_use_different_datatype"))
def test_the_wrappers_pass_the_keyword(cpu_construction, fn):
    ql = cpu_construction
    kw = dict(W4A4, weight_fp_type="fp_e1")
    off = getattr(ql, fn)(_Var(128, 2), real_fp4=True, w6_weights=True, **kw)
    on = getattr(ql, fn)(_Var(128, 2), real_fp4=True, w6_weights=True, w6_forms=True, **kw)
    for b in range(2):
        assert off.blocks[b].attn.proj.w6_forms is False
        p = on.blocks[b].attn.proj
        assert isinstance(p, _Marker) and (p.act, p.weight_type, p.kmajor_arg, p.w6_forms) == ("fp_e2", "fp_e1", False, True)
        assert on.blocks[b].ffn.fc1.weight_type == "fp_e2" and on.blocks[b].ffn.fc1.w6_forms is False
