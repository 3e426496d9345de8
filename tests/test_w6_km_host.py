"""The W6 GEMM on k-major images (fpq_gemm_w6_mx_km, fpq_gemm_w6_gelu_dual_km, fpq_gemm_w6_mx_split_km, fpq_gemm_w6_mx_split_qknorm_km;
gemm.linear_w6_km, linear_w6_gelu_dual_km, linear_w6_qkv_to_cache_km; FP4Linear(..., kmajor=True, w6_kmajor=True);
quantize_VAR_mixed(..., w6_kmajor=True)) without a GPU, after tests/test_w6_forms_host.py and tests/test_a6w4_km_host.py: the four entry
points' export, declaration, ctypes signature and argument checks in their documented order (null or fake pointers - every call ends
in a refusal or in the empty-problem return, nothing is launched), the Python wrappers' refusals, the module defaults, and -
construction only, with marker classes - which layer of a 6-bit-weight model is built k-major with and without the keyword."""
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
TWINS = {"fpq_gemm_w6_mx_km": "fpq_gemm_w6_mx", "fpq_gemm_w6_gelu_dual_km": "fpq_gemm_w6_gelu_dual",
         "fpq_gemm_w6_mx_split_km": "fpq_gemm_w6_mx_split", "fpq_gemm_w6_mx_split_qknorm_km": "fpq_gemm_w6_mx_split_qknorm"}
A_IDS, W_IDS = (E2M1, E1M2, E3M0), (E1M2, E3M0)
BIG = 1 << 28


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as g
    g.build_hip()
    from fpqvar_amd import _lib
    return _lib.lib()


# ------------------------------------------------------------------------------------------------------------ the C ABI
def test_exports_declarations_and_signatures(lib):
    """(FPQ_VERSION stays 136: the entry points are additions a caller looks up); each _km entry point has its twin's argument list -
    no kmajor flag on either"""
    from fpqvar_amd import _lib
    assert lib.fpq_version() == 136
    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "fpq.h")).read(), flags=re.S)
    i, p, q = ctypes.c_int, ctypes.c_void_p, ctypes.c_int64
    for name, twin in TWINS.items():
        assert hasattr(lib, name), name
        assert name in _lib._SIGS, name
        assert re.search(r"\bint\s+" + name + r"\s*\(", hdr), f"{name} is not declared in include/fpq.h"
        assert _lib._SIGS[name] == _lib._SIGS[twin], name
        decl = lambda n: re.sub(r"\b(a|w)_(codes|image)\b", r"\1_x", re.search(r"\bint\s+" + n + r"\s*\(([^)]*)\)", hdr).group(1))
        assert " ".join(decl(name).split()) == " ".join(decl(twin).split()), f"{name}: the header's argument list differs from {twin}'s"
    assert _lib._SIGS["fpq_gemm_w6_mx_km"] == (i, [p, p, i, p, p, i, i, p, p, q, q, q, p, p])
    assert _lib._SIGS["fpq_gemm_w6_gelu_dual_km"] == (i, [p, p, i, p, p, i, i, p, p, p, q, q, q, p, p])
    assert _lib._SIGS["fpq_gemm_w6_mx_split_km"] == (i, [p, p, i, p, p, i, i, p, q, q, q, p, p])
    assert _lib._SIGS["fpq_gemm_w6_mx_split_qknorm_km"] == (i, [p, p, i, p, p, i, i, p, q, q, q, p, p, p])
    text = open(os.path.join(ROOT, "include", "fpq.h")).read()
    assert "there is no k-major form" not in text and "Row-major operands only" not in text[text.index("---- W6:"):]


def test_mx_km_checks_in_the_documented_order(lib):
    """tables, negative sizes, the epilogue descriptor, w_scale_dtype (fp32 only), shape, the 2^28 rule, the empty problem, then NULL
    pointers / alignment with both scale images at 16 bytes: each refusal wins over everything behind it"""
    from fpqvar_amd._lib import GemmEpilogue

    def call(a=PTR, sa=PTR, a_table=E3M0, w=PTR, sw=PTR, w_dtype=F32, w_table=E1M2, bias=None, out=None, tokens=8, outs=128, k=128, ep=None):
        return lib.fpq_gemm_w6_mx_km(a, sa, a_table, w, sw, w_dtype, w_table, bias, out, tokens, outs, k, ep, None)
    bad_ep = ctypes.byref(GemmEpilogue(PTR + 8, None, 1))                    # a misaligned gate
    for at in A_IDS:
        for wt in W_IDS:
            assert call(a_table=at, w_table=wt, tokens=0) == OK and call(a_table=at, w_table=wt, outs=0) == OK
            assert call(a_table=at, w_table=wt) == ERR_ARG                   # out is NULL: the last check but one
    for t in (E2M3, E3M2, 5, 99, -1):
        assert call(a_table=t) == ERR_TABLE and call(w_table=t) == ERR_TABLE, t
    assert call(w_table=E2M1) == ERR_TABLE and call(w_table=E2M1, tokens=-1) == ERR_TABLE and call(a_table=7, w_dtype=F16) == ERR_TABLE
    assert call(a_table=7, ep=bad_ep) == ERR_TABLE and call(w_table=7, tokens=BIG) == ERR_TABLE
    assert call(tokens=-4) == ERR_ARG and call(outs=-128, w_dtype=F16) == ERR_ARG and call(k=-128, outs=0) == ERR_ARG
    assert call(ep=bad_ep) == ERR_ARG and call(ep=bad_ep, w_dtype=F16) == ERR_ARG and call(ep=bad_ep, tokens=0) == ERR_ARG
    assert call(w_dtype=F16) == ERR_DTYPE and call(w_dtype=9) == ERR_DTYPE and call(w_dtype=F16, k=96) == ERR_DTYPE
    assert call(w_dtype=F16, tokens=0) == ERR_DTYPE and call(w_dtype=F16, tokens=BIG) == ERR_DTYPE
    assert call(k=96) == ERR_SHAPE and call(k=128 * 65) == ERR_SHAPE and call(outs=100) == ERR_SHAPE and call(tokens=1 << 31) == ERR_SHAPE
    assert call(k=96, tokens=0) == ERR_SHAPE
    # the 2^28 rule: behind the shape rules, in front of the empty problem and the pointers
    assert call(tokens=BIG) == ERR_SHAPE and call(outs=BIG) == ERR_SHAPE and call(tokens=BIG, outs=0) == ERR_SHAPE
    assert call(outs=BIG, tokens=0) == ERR_SHAPE and call(tokens=BIG, a=None) == ERR_SHAPE
    assert call(tokens=BIG - 1) == ERR_ARG and call(outs=BIG - 8) == ERR_ARG   # below it: on to the pointers (out is NULL)
    assert lib.fpq_gemm_w6_mx(PTR, PTR, E3M0, PTR, PTR, F32, E1M2, None, None, BIG, 128, 128, None, None) == ERR_ARG   # the twin has no such rule
    # the empty problem: over NULL pointers and alignment
    assert call(tokens=0, a=None, sa=PTR + 4, sw=PTR + 8) == OK and call(outs=0, w=PTR + 8) == OK
    # NULL pointers / alignment
    out = PTR
    assert call(k=0, out=out) == ERR_ARG
    for name in ("a", "sa", "w", "sw"):
        assert call(**{name: None}, out=out) == ERR_ARG, name
    assert call(a=PTR + 8, out=out) == ERR_ARG and call(w=PTR + 8, out=out) == ERR_ARG and call(out=PTR + 8) == ERR_ARG
    assert call(bias=PTR + 4, out=out) == ERR_ARG
    for off in (2, 4, 8):                                                    # the scale images: 16 bytes, both
        assert call(sa=PTR + off, out=out) == ERR_ARG and call(sw=PTR + off, out=out) == ERR_ARG, off


def test_gelu_dual_km_checks_in_the_documented_order(lib):
    def call(a=PTR, sa=PTR, a_table=E3M0, w=PTR, sw=PTR, w_dtype=F32, w_table=E1M2, bias=None, out=None, h=None, tokens=8, outs=128, k=128,
             flag=None):
        return lib.fpq_gemm_w6_gelu_dual_km(a, sa, a_table, w, sw, w_dtype, w_table, bias, out, h, tokens, outs, k, flag, None)
    for at in A_IDS:
        for wt in W_IDS:
            assert call(a_table=at, w_table=wt, tokens=0) == OK and call(a_table=at, w_table=wt, outs=0) == OK
    for t in (E2M3, E3M2, 5, 99, -1):
        assert call(a_table=t) == ERR_TABLE and call(w_table=t) == ERR_TABLE, t
    assert call(w_table=E2M1) == ERR_TABLE and call(w_table=E2M1, tokens=-1) == ERR_TABLE and call(a_table=7, w_dtype=F16) == ERR_TABLE
    assert call(a_table=7, outs=100) == ERR_TABLE and call(w_table=7, tokens=BIG) == ERR_TABLE
    assert call(tokens=-4) == ERR_ARG and call(outs=-128) == ERR_ARG and call(k=-128) == ERR_ARG
    assert call(tokens=-4, w_dtype=F16) == ERR_ARG and call(k=-128, outs=0) == ERR_ARG and call(outs=-128, k=96) == ERR_ARG
    assert call(w_dtype=F16) == ERR_DTYPE and call(w_dtype=2) == ERR_DTYPE and call(w_dtype=F16, k=96) == ERR_DTYPE
    assert call(w_dtype=F16, tokens=0) == ERR_DTYPE and call(w_dtype=F16, tokens=BIG) == ERR_DTYPE
    assert call(k=96) == ERR_SHAPE and call(k=128 * 65) == ERR_SHAPE and call(outs=100) == ERR_SHAPE and call(outs=8) == ERR_SHAPE
    assert call(outs=192) == ERR_SHAPE and call(tokens=1 << 31) == ERR_SHAPE and call(k=96, tokens=0) == ERR_SHAPE
    assert call(tokens=BIG) == ERR_SHAPE and call(outs=BIG) == ERR_SHAPE and call(tokens=BIG, outs=0) == ERR_SHAPE
    assert call(outs=BIG, tokens=0) == ERR_SHAPE and call(tokens=BIG - 1) == ERR_ARG and call(outs=BIG - 128) == ERR_ARG
    assert lib.fpq_gemm_w6_gelu_dual(PTR, PTR, E3M0, PTR, PTR, F32, E1M2, None, None, None, BIG, 128, 128, None, None) == ERR_ARG
    assert call(k=128 * 64) == ERR_ARG                                       # the longest K still fits the LDS: on to the pointers
    assert call(tokens=0, a=None, sa=PTR + 4) == OK and call(outs=0, w=PTR + 8, sw=PTR + 8) == OK
    assert call(bias=PTR + 4, h=PTR + 8, flag=PTR + 4, tokens=0) == OK
    out = PTR
    assert call(k=0, out=out) == ERR_ARG
    for name in ("a", "sa", "w", "sw"):
        assert call(**{name: None}, out=out) == ERR_ARG, name
    assert call(a=PTR + 8, out=out) == ERR_ARG and call(w=PTR + 8, out=out) == ERR_ARG and call(out=PTR + 8) == ERR_ARG
    assert call(h=PTR + 8, out=out) == ERR_ARG and call(flag=PTR + 4, out=out) == ERR_ARG and call(bias=PTR + 4, out=out) == ERR_ARG
    for off in (2, 4, 8):
        assert call(sa=PTR + off, out=out) == ERR_ARG and call(sw=PTR + off, out=out) == ERR_ARG, off


def _split(n_parts=3, part_cols=128, rpb=4, out=(PTR, PTR, PTR), stride=None):
    from fpqvar_amd._lib import GemmSplit
    sp = GemmSplit()
    sp.part_cols, sp.n_parts, sp.rows_per_batch = part_cols, n_parts, rpb
    for p in range(3):
        sp.out[p], sp.row_stride[p], sp.batch_stride[p], sp.row0[p] = out[p], part_cols if stride is None else stride, rpb, 0
    return sp


_DEFAULT = object()


def _split_call(lib, norm):
    """the entry point with harmless defaults: 8 tokens (two batch entries of 4), three parts of 128 columns, k = 128, NULL operands"""
    def call(a=None, sa=None, a_table=E3M0, w=None, sw=None, w_dtype=F32, w_table=E1M2, bias=None, tokens=8, outs=384, k=128, split=_DEFAULT,
             hs=PTR):
        sp = _split() if split is _DEFAULT else split
        ref = None if sp is None else ctypes.byref(sp)
        if norm:
            return lib.fpq_gemm_w6_mx_split_qknorm_km(a, sa, a_table, w, sw, w_dtype, w_table, bias, tokens, outs, k, ref, hs, None)
        return lib.fpq_gemm_w6_mx_split_km(a, sa, a_table, w, sw, w_dtype, w_table, bias, tokens, outs, k, ref, None)
    return call


@pytest.mark.parametrize("norm", (False, True))
def test_split_km_checks_in_the_documented_order(lib, norm):
    """tables; NULL split (and the norm form's own arguments); negative sizes; the split descriptor; the scale dtype; shape; the 2^28
    rule; the empty problem; then pointers / alignment - the operands default to NULL, so reaching the pointers is FPQ_ERR_ARG"""
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
    assert call(split=None) == ERR_ARG and call(split=None, tokens=0) == ERR_ARG and call(split=None, w_dtype=F16) == ERR_ARG
    assert call(split=None, k=96) == ERR_ARG
    assert call(tokens=-1, w_dtype=F16) == ERR_ARG and call(outs=-384, k=96) == ERR_ARG and call(k=-128, w_dtype=F16) == ERR_ARG
    for bad in (dict(split=_split(n_parts=0), outs=0), dict(split=_split(n_parts=4), outs=512), dict(split=_split(part_cols=100), outs=300),
                dict(outs=256), dict(tokens=6), dict(split=_split(rpb=0)), dict(split=_split(out=(PTR, None, PTR))),
                dict(split=_split(out=(PTR, PTR, PTR + 4))), dict(split=_split(stride=64)), dict(split=_split(stride=130))):
        assert call(**bad) == ERR_ARG, bad
        assert call(**bad, w_dtype=F16) == ERR_ARG and call(**bad, k=96) == ERR_ARG, bad
    if norm:
        assert call(split=_split(n_parts=2), outs=256) == ERR_ARG and call(split=_split(n_parts=2), outs=256, w_dtype=F16) == ERR_ARG
    else:
        assert call(split=_split(n_parts=2), outs=256, tokens=0) == OK and call(split=_split(n_parts=1), outs=128, tokens=0) == OK
    assert call(w_dtype=F16) == ERR_DTYPE and call(w_dtype=F16, k=96) == ERR_DTYPE and call(w_dtype=F16, tokens=0) == ERR_DTYPE
    assert call(w_dtype=7) == ERR_DTYPE and call(w_dtype=F16, tokens=BIG, split=_split(rpb=1 << 20)) == ERR_DTYPE
    assert call(k=96) == ERR_SHAPE and call(k=128 * 65) == ERR_SHAPE and call(k=96, tokens=0) == ERR_SHAPE
    assert call(tokens=1 << 31, split=_split(rpb=1 << 20)) == ERR_SHAPE
    # the 2^28 rule (the row-major twin goes on to the pointers there)
    assert call(tokens=BIG, split=_split(rpb=1 << 20)) == ERR_SHAPE
    assert call(tokens=BIG - (1 << 20), split=_split(rpb=1 << 20)) == ERR_ARG
    assert call(outs=3 * (1 << 27), split=_split(part_cols=1 << 27, stride=1 << 27)) == ERR_SHAPE
    assert call(outs=3 * (1 << 27), split=_split(part_cols=1 << 27, stride=1 << 27), tokens=0) == ERR_SHAPE
    assert call(k=0) == ERR_ARG and call(tokens=0, split=_split(rpb=7)) == OK


@pytest.mark.parametrize("norm", (False, True))
def test_split_km_pointer_and_alignment_checks(lib, norm):
    base = _split_call(lib, norm)

    def call(**kw):   # one operand is always wrong in what follows
        return base(**{**dict(a=PTR, sa=PTR, w=PTR, sw=PTR), **kw})
    for name in ("a", "sa", "w", "sw"):
        assert call(**{name: None}) == ERR_ARG, name
    assert call(a=PTR + 8) == ERR_ARG and call(w=PTR + 8) == ERR_ARG
    for off in (1, 2, 4, 8):                                                 # both scale images: 16 bytes
        assert call(sa=PTR + off) == ERR_ARG and call(sw=PTR + off) == ERR_ARG, off
    if norm:
        assert call(hs=None) == ERR_ARG and call(hs=PTR + 2) == ERR_ARG and call(hs=None, tokens=0) == ERR_ARG
        assert call(bias=PTR + 8) == ERR_ARG and call(bias=PTR + 8, tokens=0) == ERR_ARG
        assert call(a=PTR + 8, w=PTR + 8, sa=PTR + 4, sw=PTR + 8, bias=PTR + 16, tokens=0) == OK
    else:
        assert call(bias=PTR + 4) == ERR_ARG
        assert call(a=PTR + 8, w=PTR + 8, sa=PTR + 4, sw=PTR + 8, bias=PTR + 4, tokens=0) == OK


# ------------------------------------------------------------------------------------------------------------ the wrappers
def _row_operands(a_table="e3m0", tokens=8, outs=384, k=128):
    return (torch.zeros(tokens, k // 128 * wm.SEG[a_table], dtype=torch.uint8), torch.zeros(tokens, k // 128, dtype=torch.float16),
            torch.zeros(outs, k * 3 // 4, dtype=torch.uint8), torch.zeros(outs, k // 128))


def _image_operands(a_table="e3m0", tokens=8, outs=384, k=128):
    g, op = k // 128, (outs + 63) // 64 * 64
    return (torch.zeros(g, tokens, wm.SEG[a_table], dtype=torch.uint8), torch.zeros(g, (tokens + 3) // 4 * 4),
            torch.zeros(g, op, 96, dtype=torch.uint8), torch.zeros(g, op))


def _cache(bsz=2, max_len=10, heads=2, hd=64):
    return torch.zeros(2, bsz, max_len, heads, hd, dtype=torch.float16)


def test_python_wrappers_refuse_cpu_tensors(lib):
    from fpqvar_amd import gemm
    a, sa, w, sw = _image_operands()
    with pytest.raises(RuntimeError, match="GPU"):
        gemm.linear_w6_km(a, sa, "e3m0", w, sw, "e1m2")
    with pytest.raises(RuntimeError, match="GPU"):
        gemm.linear_w6_gelu_dual_km(a, sa, "e3m0", w, sw, "e1m2")
    with pytest.raises(RuntimeError, match="GPU"):
        gemm.linear_w6_qkv_to_cache_km(a, sa, "e3m0", w, sw, "e1m2", None, _cache(), 0, 4)


def test_python_wrappers_refusals_behind_the_gpu_check(lib, monkeypatch):
    """the refusals behind the GPU test, reached on CPU tensors with that test switched off: every call here ends in one"""
    from fpqvar_amd import gemm
    monkeypatch.setattr(gemm, "require_gpu", lambda *a, **k: None)
    a, sa, w, sw = _image_operands(outs=136)
    ra, rsa, rw, rsw = _row_operands(outs=136)
    km = gemm.linear_w6_km
    with pytest.raises(RuntimeError, match="both operands must be k-major images"):
        km(ra, rsa, "e3m0", rw, rsw, "e1m2")                                 # row-major codes
    with pytest.raises(RuntimeError, match="both operands must be k-major images"):
        km(ra, rsa, "e3m0", w, sw, "e1m2")
    with pytest.raises(RuntimeError, match="multiple of 64 rows"):
        km(a, sa, "e3m0", w[:, :136].contiguous(), sw[:, :136].contiguous(), "e1m2", outs=136)
    with pytest.raises(RuntimeError, match=r"\[K/128, tokens, 96\] \(activation\) and \[K/128, rows, 96\] \(weight\)"):
        km(a[:, :, :64].contiguous(), sa, "e3m0", w, sw, "e1m2", outs=136)   # a 4-bit image under a 6-bit table
    with pytest.raises(RuntimeError, match=r"\[K/128, tokens, 64\] \(activation\) and \[K/128, rows, 96\] \(weight\)"):
        km(a, sa, "e2m1", w, sw, "e1m2", outs=136)
    with pytest.raises(RuntimeError, match="does not belong"):
        km(a, sa, "e3m0", w, sw, "e1m2", outs=64)
    with pytest.raises(RuntimeError, match="does not belong"):
        km(a, sa, "e3m0", w, sw, "e1m2", torch.zeros(100, dtype=torch.float16))   # the bias names the width
    with pytest.raises(RuntimeError, match="weight scales must be float32"):
        km(a, sa, "e3m0", w, sw.half(), "e1m2", outs=136)
    with pytest.raises(RuntimeError, match=r"scale image must be a contiguous float32 \[1, 8\]"):
        km(a, sa.half(), "e3m0", w, sw, "e1m2", outs=136)
    with pytest.raises(RuntimeError, match=r"scale image must be a contiguous float32 \[1, 8\]"):
        km(a, sa[:, :7].contiguous(), "e3m0", w, sw, "e1m2", outs=136)       # the scale image is not padded to 4 rows
    with pytest.raises(RuntimeError, match="'e1m2' and 'e3m0'"):
        km(a, sa, "e3m0", w, sw, "e2m1", outs=136)
    with pytest.raises(RuntimeError, match="'e1m2' and 'e3m0'"):
        km(a, sa, "e2m3", w, sw, "e1m2", outs=136)
    with pytest.raises(RuntimeError, match="bias must hold one value per output"):
        km(a, sa, "e3m0", w, sw, "e1m2", torch.zeros(100, dtype=torch.float16), outs=136)
    with pytest.raises(RuntimeError, match="multiple of 128"):
        gemm.linear_w6_gelu_dual_km(a, sa, "e3m0", w, sw, "e1m2", outs=136)
    with pytest.raises(RuntimeError, match="both operands must be k-major images"):
        gemm.linear_w6_gelu_dual_km(ra, rsa, "e3m0", rw, rsw, "e1m2")
    a, sa, w, sw = _image_operands()
    go = lambda cache, pos=0, seq=4, bias=None, hs=None, sw_=sw: gemm.linear_w6_qkv_to_cache_km(a, sa, "e3m0", w, sw_, "e3m0", bias, cache, pos, seq, hs)
    with pytest.raises(RuntimeError, match=r"contiguous float16 \[2, B, max_len, H, c\]"):
        go(_cache()[0])
    with pytest.raises(RuntimeError, match="do not fit"):
        go(_cache(), pos=7)
    with pytest.raises(RuntimeError, match="does not belong"):               # a cache of another width than the weight image's
        go(_cache(heads=4))
    with pytest.raises(RuntimeError, match="weight scales must be float32"):
        go(_cache(), sw_=sw.half())
    with pytest.raises(RuntimeError, match="qk_norm_scale must be"):
        go(_cache(), hs=torch.ones(3))
    with pytest.raises(RuntimeError, match="both operands must be k-major images"):
        gemm.linear_w6_qkv_to_cache_km(*_row_operands()[:2], "e3m0", *_row_operands()[2:], "e3m0", None, _cache(), 0, 4)
    # the row-major functions go on refusing images
    for fn in (gemm.linear_w6, gemm.linear_w6_gelu_dual):
        with pytest.raises(RuntimeError, match="row-major operands only"):
            fn(a, sa, "e3m0", w, sw, "e1m2")
    with pytest.raises(RuntimeError, match="row-major operands only"):
        gemm.linear_w6_qkv_to_cache(a, sa, "e3m0", w, sw, "e1m2", None, _cache(), 0, 4)


def test_the_gemm_call_names_the_km_entry_points(lib, monkeypatch):
    """_per_group_gemm: the W6 family has an entry point per layout in every form and passes no kmajor flag"""
    from fpqvar_amd import gemm
    calls = []

    class _Lib:
        def __getattr__(self, name):
            return lambda *args: calls.append((name, args)) or 0
    monkeypatch.setattr(gemm, "lib", lambda: _Lib())
    monkeypatch.setattr(gemm, "stream_ptr", lambda dev: None)
    fmt = gemm._W6_FORMATS["e3m0", "e1m2"]
    t = torch.zeros(1)
    for form, km, want in (("", False, "fpq_gemm_w6_mx"), ("", True, "fpq_gemm_w6_mx_km"),
                           ("gelu_dual", False, "fpq_gemm_w6_gelu_dual"), ("gelu_dual", True, "fpq_gemm_w6_gelu_dual_km"),
                           ("split", False, "fpq_gemm_w6_mx_split"), ("split", True, "fpq_gemm_w6_mx_split_km"),
                           ("split_qknorm", False, "fpq_gemm_w6_mx_split_qknorm"), ("split_qknorm", True, "fpq_gemm_w6_mx_split_qknorm_km")):
        calls.clear()
        gemm._per_group_gemm(form, fmt, km, t, t, t, t, "rest")
        (name, args), = calls
        assert name == want and args[-2] == "rest", (form, km, name)          # nothing between the form's arguments and the stream
    fp4 = gemm._FORMATS["e3m0"]                                               # the A6W4 family keeps its flag
    calls.clear()
    gemm._per_group_gemm("split", fp4, True, t, t, t, t, "rest")
    assert calls[0][0] == "fpq_gemm_a6w4_mx_split" and calls[0][1][-3:-1] == ("rest", 1)


def _w6_module(gemm, cls, kmajor, w_table="e1m2", act="e3m0", outs=384, **kw):
    """a module with a 6-bit weight built without the quantizer (which needs the GPU)"""
    if kmajor:
        return cls(torch.zeros(1, outs, 96, dtype=torch.uint8), torch.ones(1, outs), None, 128, outs, act, w_table, **kw)
    return cls(torch.zeros(outs, 96, dtype=torch.uint8), torch.ones(outs, 1), None, 128, outs, act, w_table, **kw)


def test_module_defaults_and_the_w6_kmajor_keyword(lib):
    """without w6_kmajor every kmajor / a6w4_kmajor combination with a 6-bit weight raises what it raised; w6_kmajor alone changes
    nothing; with kmajor=True it passes the refusal (on to the weight quantizer, which needs the GPU); a module that holds images
    reports kmajor and runs the _km function of the requested form"""
    from fpqvar_amd import gemm
    lin = torch.nn.Linear(128, 384)
    for cls in (gemm.FP4Linear, gemm.FP4LinearGeluDual):
        for w in ("fp_e1", "fp_e3"):
            for kw in (dict(kmajor=True), dict(a6w4_kmajor=True), dict(kmajor=True, a6w4_kmajor=True, act_fp_type="fp_e3"),
                       dict(a6w4_kmajor=True, w6_kmajor=True), dict(kmajor=True, w6_kmajor=False)):
                with pytest.raises(ValueError, match="no k-major form"):
                    cls.from_float(lin, weight_fp_type=w, w6_forms=True, **kw)
            for kw in (dict(w6_kmajor=True), dict(kmajor=True, w6_kmajor=True), dict(kmajor=True, w6_kmajor=True, a6w4_kmajor=True)):
                with pytest.raises(RuntimeError, match="GPU"):               # past the refusals: quantize_g6 of the weight
                    cls.from_float(lin, weight_fp_type=w, w6_forms=True, **kw)
    with pytest.raises(ValueError, match="no fc1 tail"):
        gemm.FP4LinearGeluDual.from_float(lin, weight_fp_type="fp_e1", kmajor=True, w6_kmajor=True)
    with pytest.raises(ValueError, match="no k-major form"):                 # an E2M1 weight ignores the keyword
        gemm.FP4Linear.from_float(lin, kmajor=True, act_fp_type="fp_e3", w6_kmajor=True)
    x, cache = torch.zeros(2, 4, 128), _cache()
    ac, asc = torch.zeros(1, 8, 96, dtype=torch.uint8), torch.zeros(1, 8)
    m = _w6_module(gemm, gemm.FP4Linear, True, w6_forms=True)
    d = _w6_module(gemm, gemm.FP4LinearGeluDual, True, w6_forms=True)
    r = _w6_module(gemm, gemm.FP4Linear, False, w6_forms=True)
    assert m.kmajor and d.kmajor and not r.kmajor
    with pytest.raises(RuntimeError, match="linear_w6_km.*GPU|GPU.*linear_w6_km"):
        m.forward_operands(ac, asc)
    with pytest.raises(RuntimeError, match="linear_w6_qkv_to_cache_km.*GPU|GPU.*linear_w6_qkv_to_cache_km"):
        m.qkv_to_cache_operands(ac, asc, cache, 0, 4)
    with pytest.raises(RuntimeError, match="linear_w6_gelu_dual_km.*GPU|GPU.*linear_w6_gelu_dual_km"):
        d.forward_operands(ac, asc)
    with pytest.raises(RuntimeError, match=r"linear_w6\b.*GPU|GPU.*linear_w6\b"):
        r.forward_operands(ac, asc)
    with pytest.raises(RuntimeError, match="GPU"):
        m(x)
    plain = _w6_module(gemm, gemm.FP4Linear, True)                            # without w6_forms: the plain form only, k-major or not
    with pytest.raises(ValueError, match="plain form only"):
        plain.qkv_to_cache_operands(ac, asc, cache, 0, 4)


# ------------------------------------------------------------------------------------------------------------ the wiring
class _Marker(torch.nn.Module):
    def __init__(self, cls, kw):
        super().__init__()
        self.cls_name, self.kw = cls.__name__, kw


@pytest.fixture
def cpu_construction(monkeypatch):
    """Quantizing a weight needs the GPU: on the CPU the weight quantizer is an identity and FP4Linear.from_float records the class it
    was asked for and the keywords it was called with"""
    from fpqvar_amd import gemm, quant_linear as ql
    monkeypatch.setattr(ql, "_quantize_weight", lambda w, *a, **k: w)
    monkeypatch.setattr(gemm.FP4Linear, "from_float", classmethod(lambda cls, lin, **kw: _Marker(cls, kw)))
    return ql


FP = ("fp_e1", "fp_e2", "fp_e3")
MK = {k: v for k, v in W4A4.items() if k not in ("act_fp_type", "weight_fp_type", "fc2_fp_type")}


def _formats(b, layer):
    """3 x 3: block b = 3 i + j has activation format FP[i] and weight format FP[j] on fc1, mat_qkv and proj"""
    return ("fp_e1m2_neg_e2m1_pos", "fp_e2") if layer == "fc2" else (FP[b // 3], FP[b % 3])


def _layers(model):
    for b, blk in enumerate(model.blocks):
        for name in ("ffn.fc1", "attn.mat_qkv", "attn.proj"):
            yield b, name, blk.get_submodule(name)


@pytest.mark.parametrize("fuse", (False, True))
def test_w6_kmajor_builds_the_6bit_weight_layers_kmajor(cpu_construction, fuse):
    ql = cpu_construction
    on = ql.quantize_VAR_mixed(_Var(128, 9), _formats, real_fp4=True, w6_weights=True, w6_forms=True, w6_kmajor=True, a6w4_kmajor=True,
                               fuse_ffn=fuse, **MK)
    for b, name, m in _layers(on):
        a, w = FP[b // 3], FP[b % 3]
        assert isinstance(m, _Marker) and m.cls_name == ("FP4LinearGeluDual" if fuse and name == "ffn.fc1" else "FP4Linear"), (b, name)
        if w != "fp_e2":
            assert m.kw == dict(act_fp_type=a, weight_fp_type=w, w6_forms=True, kmajor=True, w6_kmajor=True), (b, name, m.kw)
        else:                                                                # an E2M1 weight is built as before, without the keyword
            assert "w6_kmajor" not in m.kw and m.kw.get("kmajor") is True, (b, name, m.kw)
    # without w6_forms the plain layers are k-major too
    noforms = ql.quantize_VAR_mixed(_Var(128, 9), _formats, real_fp4=True, w6_weights=True, w6_kmajor=True, **MK)
    for b, name, m in _layers(noforms):
        if FP[b % 3] != "fp_e2":
            assert m.kw == dict(act_fp_type=FP[b // 3], weight_fp_type=FP[b % 3], kmajor=True, w6_kmajor=True), (b, name, m.kw)
    # inert when kmajor_operands is off, as a6w4_kmajor is
    inert = ql.quantize_VAR_mixed(_Var(128, 9), _formats, real_fp4=True, w6_weights=True, w6_forms=True, w6_kmajor=True, kmajor_operands=False,
                                  fuse_ffn=fuse, **MK)
    for b, name, m in _layers(inert):
        if FP[b % 3] != "fp_e2":
            assert m.kw == dict(act_fp_type=FP[b // 3], weight_fp_type=FP[b % 3], w6_forms=True), (b, name, m.kw)


def test_without_w6_kmajor_from_float_gets_todays_keyword_list(cpu_construction, monkeypatch):
    """default / w6_kmajor=False: the same calls as today - a from_float with today's keyword list (no w6_kmajor) still serves"""
    ql = cpu_construction
    from fpqvar_amd import gemm
    old = classmethod(lambda cls, lin, kmajor=False, act_fp_type="fp_e2", a6w4_kmajor=False, weight_fp_type="fp_e2", w6_forms=False:
                      _Marker(cls, dict(kmajor=kmajor, act_fp_type=act_fp_type, a6w4_kmajor=a6w4_kmajor, weight_fp_type=weight_fp_type,
                                        w6_forms=w6_forms)))
    monkeypatch.setattr(gemm.FP4Linear, "from_float", old)
    for extra in ({}, {"w6_kmajor": False}):
        for fuse in (False, True):
            m = ql.quantize_VAR_mixed(_Var(128, 9), _formats, real_fp4=True, w6_weights=True, w6_forms=True, fuse_ffn=fuse, a6w4_kmajor=True,
                                      **extra, **MK)
            for b, name, layer in _layers(m):
                assert isinstance(layer, _Marker) and layer.kw["w6_forms"] is (FP[b % 3] != "fp_e2"), (b, name)
                assert layer.kw["kmajor"] is (FP[b % 3] == "fp_e2"), (b, name)     # 6-bit weights stay row-major
    with pytest.raises(TypeError):                                           # with the keyword on, from_float must know it
        ql.quantize_VAR_mixed(_Var(128, 9), _formats, real_fp4=True, w6_weights=True, w6_kmajor=True, **MK)


def test_w6_kmajor_needs_w6_weights(cpu_construction):
    ql = cpu_construction
    with pytest.raises(ValueError, match="w6_kmajor needs w6_weights"):
        ql.quantize_VAR_mixed(_Var(128, 1), _formats, real_fp4=True, w6_kmajor=True, **MK)
    with pytest.raises(ValueError, match="w6_weights needs real_fp4"):
        ql.quantize_VAR_mixed(_Var(128, 1), _formats, w6_weights=True, w6_kmajor=True, **MK)
    for fn in (ql.quantize_VAR_mixed_fp4_datatype, ql.quantize_VAR_use_different_datatype):
        with pytest.raises(ValueError, match="w6_kmajor needs w6_weights"):
            fn(_Var(128, 1), real_fp4=True, w6_kmajor=True, **W4A4)


@pytest.mark.parametrize("fn", ("quantize_VAR_mixed_fp4_datatype", "quantize_VAR_use_different_datatype"))
def test_the_wrappers_pass_the_keyword(cpu_construction, fn):
    ql = cpu_construction
    kw = dict(W4A4, weight_fp_type="fp_e1")
    off = getattr(ql, fn)(_Var(128, 2), real_fp4=True, w6_weights=True, **kw)
    on = getattr(ql, fn)(_Var(128, 2), real_fp4=True, w6_weights=True, w6_kmajor=True, **kw)
    for b in range(2):
        assert off.blocks[b].attn.proj.kw == dict(act_fp_type="fp_e2", weight_fp_type="fp_e1")
        assert on.blocks[b].attn.proj.kw == dict(act_fp_type="fp_e2", weight_fp_type="fp_e1", kmajor=True, w6_kmajor=True)
        assert "w6_kmajor" not in on.blocks[b].ffn.fc1.kw and "weight_fp_type" not in on.blocks[b].ffn.fc1.kw   # an E2M1 weight
