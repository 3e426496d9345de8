"""The A6W4 path on k-major images (fpq_a6w4_quant_rows_codes_km, fpq_gemm_a6w4_mx_km, fpq_gemm_a6w4_gelu_dual_km; gemm.linear_a6w4_km,
gemm.linear_a6w4_gelu_dual_km; quantize_VAR_mixed*(a6w4_kmajor=True)) without a GPU: the C entry points' export, declaration and
argument checks in their documented order, the Python wrappers' refusals, the nine new kernels' register / scratch figures read
from the built library, and - construction only, with marker classes as tests/test_a6w4_fc1_host.py does - which layer is
asked for in which layout."""
import os
import re

import pytest
import torch

from tests.test_a6w4_host import W4A4, _Var
from tests.test_no_spill import LIB, kernel_metadata

OK, ERR_ARG, ERR_DTYPE, ERR_SHAPE, ERR_TABLE = 0, -1, -2, -3, -4
F16, F32 = 0, 1
E2M1, E1M2, E3M0, E2M3, E3M2 = 0, 1, 2, 3, 4   # enum fpq_table
PTR = 0x7000_0000_1000   # an address with every alignment the checks ask for; nothing reads it
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("fpq_a6w4_quant_rows_codes_km", "fpq_gemm_a6w4_mx_km", "fpq_gemm_a6w4_gelu_dual_km")


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as g
    g.build_hip()
    from fpqvar_amd import _lib
    return _lib.lib()


# ------------------------------------------------------------------------------------------------------------ the C ABI
def test_version_exports_and_declarations(lib):
    from fpqvar_amd import _lib
    assert lib.fpq_version() >= 133
    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "fpq.h")).read(), flags=re.S)
    for name in NEW:
        assert hasattr(lib, name), name
        assert name in _lib._SIGS, name
        assert re.search(r"\bint\s+" + name + r"\s*\(", hdr), f"{name} is not declared in include/fpq.h"


def test_emitter_checks_in_the_documented_order(lib):
    """negative sizes, table, dtype (fp16 rows only), shape, empty problem, then pointers / alignment - nothing is launched"""
    def call(x=None, image=None, scales=None, rows=4, cols=128, table=E3M0, dtype=F16):
        return lib.fpq_a6w4_quant_rows_codes_km(x, image, scales, rows, cols, table, dtype, None)
    assert call(rows=-1, table=E2M1) == ERR_ARG and call(cols=-128, dtype=F32) == ERR_ARG
    for t in (E2M1, E2M3, E3M2, 9, -1):
        assert call(table=t) == ERR_TABLE and call(table=t, dtype=F32) == ERR_TABLE and call(table=t, cols=100, rows=0) == ERR_TABLE, t
    assert call(dtype=F32) == ERR_DTYPE and call(dtype=2, cols=100) == ERR_DTYPE and call(dtype=F32, rows=0) == ERR_DTYPE   # fp32 rows: two steps
    assert call(cols=100) == ERR_SHAPE and call(cols=100, rows=0) == ERR_SHAPE
    assert call(rows=1 << 22, cols=1024) == ERR_SHAPE                  # 3 GiB: the image is below 2 GiB
    assert call(rows=(1 << 22) - 8, cols=640) == ERR_ARG               # just below: on to the pointers
    assert call(rows=0) == OK and call(cols=0) == OK and call(table=E1M2, rows=0) == OK
    assert call() == ERR_ARG
    for name in ("x", "image", "scales"):
        args = dict(x=PTR, image=PTR, scales=PTR)
        args[name] = None
        assert call(**args) == ERR_ARG, name
        args[name] = PTR + 8
        assert call(**args) == ERR_ARG, name
    assert call(x=PTR + 8, image=PTR + 4, scales=PTR + 2, rows=0) == OK


def _gemm_call(lib, fc1):
    def call(a=None, sa=None, w=None, sw=None, table=E3M0, w_dtype=F32, bias=None, out=None, h=None, flag=None, tokens=4, outs=128, k=128, ep=None):
        if fc1:
            return lib.fpq_gemm_a6w4_gelu_dual_km(a, sa, table, w, sw, w_dtype, bias, out, h, tokens, outs, k, flag, None)
        return lib.fpq_gemm_a6w4_mx_km(a, sa, table, w, sw, w_dtype, bias, out, tokens, outs, k, ep, None)
    return call


@pytest.mark.parametrize("fc1", (False, True))
def test_gemm_checks_with_null_pointers_in_the_documented_order(lib, fc1):
    """table, negative sizes, scale dtype (fp32 images only), shape (the row-major rules, then tokens / outs < 2^28), empty
    problem, then pointers / alignment - nothing is launched"""
    call = _gemm_call(lib, fc1)
    bad_outs = 100 if fc1 else 12           # outs % 128 (fc1: a tile is one quantization group) / outs % 8
    assert call(outs=bad_outs) == ERR_SHAPE and call() == ERR_ARG and call(tokens=0) == OK and call(outs=0) == OK
    for t in (E2M1, E2M3, E3M2, 5, 99, -1):
        assert call(table=t) == ERR_TABLE and call(table=t, tokens=-1) == ERR_TABLE and call(table=t, w_dtype=F16) == ERR_TABLE, t
        assert call(table=t, outs=bad_outs) == ERR_TABLE and call(table=t, tokens=0) == ERR_TABLE, t
    assert call(tokens=-1, w_dtype=F16) == ERR_ARG and call(outs=-128) == ERR_ARG and call(k=-128, outs=bad_outs) == ERR_ARG
    # fp16 weight scales are the ROW-MAJOR entry points': the scale images are fp32
    assert call(w_dtype=F16) == ERR_DTYPE and call(w_dtype=F16, outs=bad_outs) == ERR_DTYPE and call(w_dtype=7, tokens=0) == ERR_DTYPE
    assert call(k=96) == ERR_SHAPE and call(k=128 * 65) == ERR_SHAPE and call(tokens=1 << 31) == ERR_SHAPE
    assert call(tokens=1 << 28) == ERR_SHAPE and call(outs=1 << 28) == ERR_SHAPE and call(tokens=1 << 28, outs=0) == ERR_SHAPE
    assert call(tokens=(1 << 28) - 1) == ERR_ARG and call(outs=(1 << 28) - 128) == ERR_ARG        # on to the pointers
    assert call(outs=bad_outs, tokens=0) == ERR_SHAPE and call(table=E1M2, tokens=0) == OK
    assert call(k=0) == ERR_ARG
    if not fc1:
        assert call(outs=8, tokens=0) == OK and call(outs=72) == ERR_ARG


@pytest.mark.parametrize("fc1", (False, True))
def test_gemm_pointer_and_alignment_checks(lib, fc1):
    base = _gemm_call(lib, fc1)
    def call(**kw):
        return base(**{**dict(a=PTR, sa=PTR, w=PTR, sw=PTR, out=PTR, tokens=8), **kw})
    for name in ("a", "sa", "w", "sw", "out"):
        assert call(**{name: None}) == ERR_ARG, name
    assert call(a=PTR + 8) == ERR_ARG and call(w=PTR + 8) == ERR_ARG and call(out=PTR + 8) == ERR_ARG
    assert call(bias=PTR + 4) == ERR_ARG
    # both scale images: 16 bytes (the row-major entry points ask for the element's alignment only)
    for off in (4, 8):
        assert call(sa=PTR + off) == ERR_ARG and call(sw=PTR + off) == ERR_ARG, off
    if fc1:
        assert call(h=PTR + 8) == ERR_ARG and call(flag=PTR + 4) == ERR_ARG
        assert call(bias=PTR + 4, h=PTR + 8, flag=PTR + 4, sa=PTR + 4, tokens=0) == OK
    else:
        from fpqvar_amd._lib import GemmEpilogue
        import ctypes
        assert call(ep=ctypes.byref(GemmEpilogue(PTR + 8, None, 1))) == ERR_ARG
        assert call(ep=ctypes.byref(GemmEpilogue(PTR, None, 0))) == ERR_ARG
        assert call(ep=ctypes.byref(GemmEpilogue(PTR, None, 0)), w_dtype=F16) == ERR_ARG      # the epilogue before the dtype
        assert call(bias=PTR + 4, sa=PTR + 4, tokens=0) == OK


# ------------------------------------------------------------------------------------------------------------ the wrappers
def _km_operands(tokens=4, outs=128, groups=2):
    rows64 = (outs + 63) // 64 * 64
    return (torch.zeros(groups, tokens, 96, dtype=torch.uint8), torch.zeros(groups, (tokens + 3) // 4 * 4),
            torch.zeros(groups, rows64, 64, dtype=torch.uint8), torch.zeros(groups, rows64))


@pytest.mark.parametrize("name", ("linear_a6w4_km", "linear_a6w4_gelu_dual_km"))
def test_python_wrappers_refuse_before_the_library(lib, monkeypatch, name):
    from fpqvar_amd import gemm
    fn = getattr(gemm, name)
    a, sa, w, sw = _km_operands()
    with pytest.raises(RuntimeError, match="GPU"):
        fn(a, sa, "e3m0", w, sw)
    with pytest.raises(RuntimeError, match="GPU"):
        gemm.quantize_g6(torch.zeros(4, 128, dtype=torch.float16), "e3m0", kmajor=True)
    monkeypatch.setattr(gemm, "require_gpu", lambda *a, **k: None)
    rm_a, rm_w = torch.zeros(4, 192, dtype=torch.uint8), torch.zeros(128, 128, dtype=torch.uint8)
    for bad_a, bad_w in ((rm_a, w), (a, rm_w), (rm_a, rm_w)):               # mixed 2-D / 3-D operands, and row-major codes
        with pytest.raises(RuntimeError, match="k-major images"):
            fn(bad_a, sa, "e3m0", bad_w, sw)
    with pytest.raises(RuntimeError, match="k-major images must be"):       # wrong segment widths
        fn(a[:, :, :64], sa, "e3m0", w, sw)
    with pytest.raises(RuntimeError, match="k-major images must be"):
        fn(a, sa, "e3m0", torch.zeros(2, 128, 96, dtype=torch.uint8), sw)
    with pytest.raises(RuntimeError, match="k-major images must be"):       # another K
        fn(a[:1], sa, "e3m0", w, sw)
    with pytest.raises(RuntimeError, match="k-major images must be"):       # a weight image that is no multiple of 64 rows
        fn(a, sa, "e3m0", w[:, :120], sw)
    with pytest.raises(RuntimeError, match="scale image"):                  # dtype
        fn(a, sa.half(), "e3m0", w, sw)
    with pytest.raises(RuntimeError, match="scale image"):
        fn(a, sa, "e3m0", w, sw.half())
    with pytest.raises(RuntimeError, match="scale image"):                  # shape: row-major scales, missing padding
        fn(a, torch.zeros(4, 2), "e3m0", w, sw)
    with pytest.raises(RuntimeError, match="scale image"):
        fn(*_km_operands(tokens=5)[:1], torch.zeros(2, 5), "e3m0", w, sw)
    with pytest.raises(RuntimeError, match="scale image"):
        fn(a, sa, "e3m0", w, sw[:, :100])
    with pytest.raises(RuntimeError, match="does not belong"):
        fn(a, sa, "e3m0", w, sw, outs=64)
    with pytest.raises(RuntimeError, match="'e1m2' and 'e3m0'"):
        fn(a, sa, "e2m1", w, sw)
    if name == "linear_a6w4_gelu_dual_km":
        with pytest.raises(RuntimeError, match="multiple of 128"):
            fn(a, sa, "e3m0", w, sw, outs=120)


def test_todays_refusals_stay(lib, monkeypatch):
    """what the earlier tests pin: the row-major wrappers refuse images, from_float(kmajor=True) with a 6-bit activation refuses
    unless a6w4_kmajor asks for the k-major form"""
    from fpqvar_amd import gemm
    lin = torch.nn.Linear(256, 128)
    for cls in (gemm.FP4Linear, gemm.FP4LinearGeluDual):
        for act in ("fp_e1", "fp_e3"):
            with pytest.raises(ValueError, match="no k-major form"):
                cls.from_float(lin, kmajor=True, act_fp_type=act)
            with pytest.raises(ValueError, match="no k-major form"):
                cls.from_float(lin, kmajor=True, act_fp_type=act, a6w4_kmajor=False)
        with pytest.raises(RuntimeError, match="GPU"):                       # past the refusal: on to quantizing the weight
            cls.from_float(lin, kmajor=True, act_fp_type="fp_e3", a6w4_kmajor=True)
    monkeypatch.setattr(gemm, "require_gpu", lambda *a, **k: None)
    a, sa, w, sw = _km_operands()
    for fn in (gemm.linear_a6w4, gemm.linear_a6w4_gelu_dual):
        with pytest.raises(RuntimeError, match="row-major operands only"):
            fn(a, sa, "e3m0", w, sw)


# ------------------------------------------------------------------------------------------------------------ the kernels
def _figures_ok(n, r):
    assert int(r.get("vgpr_spill_count", 0)) == 0 and int(r.get("sgpr_spill_count", 0)) == 0, (n, r)
    assert int(r.get("private_segment_fixed_size", 0)) == 0, (n, r.get("private_segment_fixed_size"))
    assert int(r["vgpr_count"]) + int(r.get("agpr_count", 0)) <= 256, (n, r["vgpr_count"])


def test_the_new_kernels_do_not_spill(lib, tmp_path):
    """{E1M2, E3M0 activation} x {64, 128 rows} x {plain, fc1} of the k-major GEMM (fp32 scale images only): exactly 8
    instantiations, no scratch, no spill, at most 256 registers per lane, no static LDS; the k-major emitter: no scratch, no spill
    (its bucket table is static LDS, as the row-major emitter's).  The library is the one the `lib` fixture built."""
    assert os.path.exists(LIB), "libfpq_hip.so is missing after the build"
    meta = list(kernel_metadata(tmp_path))
    ks = [(n, r) for n, r in meta if "gemm_a6w4_km_kernel" in n or "gemm_a6w4_fc1_km_kernel" in n]
    assert len(ks) == 8, [n for n, _ in ks]
    got = set()
    for n, r in ks:
        m = re.search(r"gemm_a6w4_(fc1_)?km_kernelI(DF16_|f)Li(\d)ELi4ELi(\d)E", n)
        assert m, n
        got.add((m.group(1) or "", m.group(2), int(m.group(3)), int(m.group(4))))
        _figures_ok(n, r)
        assert int(r.get("group_segment_fixed_size", 0)) == 0, n
    assert got == {(f, "f", mt, fa) for f in ("", "fc1_") for mt in (2, 4) for fa in (2, 3)}
    em = [(n, r) for n, r in meta if "group6_km_emit16_kernel" in n]
    assert len(em) == 1, [n for n, _ in em]
    _figures_ok(*em[0])
    rm = [(n, r) for n, r in meta if "group6_emit16_kernel" in n]
    assert len(rm) == 1 and int(em[0][1].get("group_segment_fixed_size", 0)) == int(rm[0][1].get("group_segment_fixed_size", 0))


# ------------------------------------------------------------------------------------------------------------ the wiring
class _Marker(torch.nn.Module):
    def __init__(self, cls, lin, kmajor, act_fp_type, **kw):
        super().__init__()
        self.cls_name, self.kmajor_arg, self.act, self.kw = cls.__name__, kmajor, act_fp_type, kw


@pytest.fixture
def cpu_construction(monkeypatch):
    """as tests/test_a6w4_fc1_host.py: the weight quantizer is an identity and FP4Linear.from_float records what it was asked for -
    here with **kw, so that a keyword beyond (kmajor, act_fp_type) is seen, not refused"""
    from fpqvar_amd import gemm, quant_linear as ql
    monkeypatch.setattr(ql, "_quantize_weight", lambda w, *a, **k: w)
    monkeypatch.setattr(gemm.FP4Linear, "from_float",
                        classmethod(lambda cls, lin, kmajor=False, act_fp_type="fp_e2", **kw: _Marker(cls, lin, kmajor, act_fp_type, **kw)))
    return ql


def _calls(model):
    return {n: (m.cls_name, m.kmajor_arg, m.act, tuple(sorted(m.kw.items()))) for n, m in model.named_modules() if isinstance(m, _Marker)}


FNS = ("quantize_VAR_mixed_fp4_datatype", "quantize_VAR_use_different_datatype")


@pytest.mark.parametrize("fuse", (False, True))
@pytest.mark.parametrize("fn", FNS)
def test_a6w4_kmajor_asks_for_kmajor_6bit_layers(cpu_construction, fn, fuse):
    ql = cpu_construction
    torch.manual_seed(0)
    m = getattr(ql, fn)(_Var(128, 30), real_fp4=True, fuse_ffn=fuse, a6w4_kmajor=True, **W4A4)
    calls = _calls(m)
    assert len(calls) == 90
    n6 = 0
    for name, (cls_name, kmajor, act, kw) in calls.items():
        assert kmajor is True, name                                        # one weight layout in the model
        if act == "fp_e2":
            assert kw == (), (name, kw)                                    # exactly today's call
        else:
            n6 += 1
            assert act == "fp_e3" and kw == (("a6w4_kmajor", True),), (name, kw)
        if name.endswith("fc1"):
            assert cls_name == ("FP4LinearGeluDual" if fuse else "FP4Linear")
    qkv_e2 = 3 if fn == "quantize_VAR_mixed_fp4_datatype" else 2
    assert n6 == 15 + (30 - qkv_e2)


@pytest.mark.parametrize("fn", FNS)
def test_without_the_flag_exactly_todays_calls(cpu_construction, fn):
    """default, a6w4_kmajor=False, and the flag without kmajor_operands or without real_fp4: from_float sees (lin, kmajor=...,
    act_fp_type=...) and no other keyword, 6-bit layers with kmajor=False"""
    ql = cpu_construction
    for fuse in (False, True):
        torch.manual_seed(0)
        default = _calls(getattr(ql, fn)(_Var(128, 30), real_fp4=True, fuse_ffn=fuse, **W4A4))
        off = _calls(getattr(ql, fn)(_Var(128, 30), real_fp4=True, fuse_ffn=fuse, a6w4_kmajor=False, **W4A4))
        assert off == default and len(default) == 90
        for name, (cls_name, kmajor, act, kw) in default.items():
            assert kw == () and kmajor == (act == "fp_e2"), (name, kmajor, act, kw)
        rowmajor = _calls(getattr(ql, fn)(_Var(128, 30), real_fp4=True, fuse_ffn=fuse, kmajor_operands=False, a6w4_kmajor=True, **W4A4))
        assert len(rowmajor) == 90 and all(not k and kw == () for _, k, _, kw in rowmajor.values())
    assert _calls(getattr(ql, fn)(_Var(128, 4), a6w4_kmajor=True, **W4A4)) == {}


def test_quantize_var_mixed_passes_the_flag(cpu_construction):
    ql = cpu_construction
    mk = {k: v for k, v in W4A4.items() if k not in ("act_fp_type", "weight_fp_type", "fc2_fp_type")}
    fmt = lambda b, layer: {"fc1": ("fp_e1", "fp_e2"), "fc2": ("fp_e1m2_neg_e2m1_pos", "fp_e2")}.get(layer, ("fp_e2", "fp_e2"))
    m = ql.quantize_VAR_mixed(_Var(128, 1), fmt, real_fp4=True, fuse_ffn=True, a6w4_kmajor=True, **mk)
    fc1 = m.blocks[0].ffn.fc1
    assert fc1.cls_name == "FP4LinearGeluDual" and fc1.act == "fp_e1" and fc1.kmajor_arg is True and fc1.kw == {"a6w4_kmajor": True}
    m = ql.quantize_VAR_mixed(_Var(128, 1), fmt, real_fp4=True, fuse_ffn=True, **mk)
    assert m.blocks[0].ffn.fc1.kmajor_arg is False and m.blocks[0].ffn.fc1.kw == {}
