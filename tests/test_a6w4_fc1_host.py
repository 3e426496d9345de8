"""The fc1 tail in the A6W4 GEMM (fpq_gemm_a6w4_gelu_dual, gemm.linear_a6w4_gelu_dual) and quantize_VAR_mixed*(fuse_ffn=True),
without a GPU: the C entry point's export, declaration and argument checks in their documented order, the Python wrappers'
refusals, the eight new kernels' register / scratch figures read from the built library, and - construction only, with marker
classes as tests/test_a6w4_host.py does - which FFN becomes what."""
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


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as g
    g.build_hip()
    from fpqvar_amd import _lib
    return _lib.lib()


# ------------------------------------------------------------------------------------------------------------ the C ABI
def test_version_export_and_declaration(lib):
    assert lib.fpq_version() >= 132
    assert hasattr(lib, "fpq_gemm_a6w4_gelu_dual")
    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "fpq.h")).read(), flags=re.S)
    assert re.search(r"\bint\s+fpq_gemm_a6w4_gelu_dual\s*\(", hdr), "fpq_gemm_a6w4_gelu_dual is not declared in include/fpq.h"


def test_checks_with_null_pointers_in_the_documented_order(lib):
    """table, negative sizes, scale dtype, shape, empty problem, then pointers / alignment - nothing is launched"""
    def call(table=E3M0, w_dtype=F32, tokens=4, outs=128, k=128):
        return lib.fpq_gemm_a6w4_gelu_dual(None, None, table, None, None, w_dtype, None, None, None, tokens, outs, k, None, None)
    assert call(outs=100) == ERR_SHAPE          # before the pointers
    assert call(outs=128) == ERR_ARG
    assert call(w_dtype=7) == ERR_DTYPE
    assert call(tokens=0) == OK
    for t in (E2M1, E2M3, E3M2, 5, 99, -1):     # the table comes first: before the sizes, the dtype, the shape and the empty problem
        assert call(table=t) == ERR_TABLE and call(table=t, tokens=-1) == ERR_TABLE and call(table=t, w_dtype=7) == ERR_TABLE, t
        assert call(table=t, outs=100) == ERR_TABLE and call(table=t, tokens=0) == ERR_TABLE, t
    assert call(tokens=-1, w_dtype=7) == ERR_ARG and call(outs=-128) == ERR_ARG and call(k=-128, outs=100) == ERR_ARG
    assert call(w_dtype=7, outs=100) == ERR_DTYPE and call(w_dtype=2, tokens=0) == ERR_DTYPE
    assert call(k=96) == ERR_SHAPE and call(k=128 * 65) == ERR_SHAPE and call(outs=8) == ERR_SHAPE and call(tokens=1 << 31) == ERR_SHAPE
    assert call(outs=100, tokens=0) == ERR_SHAPE and call(outs=0) == OK and call(table=E1M2, w_dtype=F16, tokens=0) == OK
    assert call(k=0) == ERR_ARG


def test_pointer_and_alignment_checks(lib):
    def call(a=PTR, sa=PTR, w=PTR, sw=PTR, w_dtype=F32, bias=None, out=PTR, h=None, flag=None, tokens=8):
        return lib.fpq_gemm_a6w4_gelu_dual(a, sa, E3M0, w, sw, w_dtype, bias, out, h, tokens, 128, 128, flag, None)
    for name in ("a", "sa", "w", "sw", "out"):
        assert call(**{name: None}) == ERR_ARG, name
    assert call(a=PTR + 8) == ERR_ARG and call(w=PTR + 8) == ERR_ARG and call(out=PTR + 8) == ERR_ARG and call(h=PTR + 8) == ERR_ARG
    assert call(bias=PTR + 4) == ERR_ARG and call(flag=PTR + 4) == ERR_ARG
    assert call(sa=PTR + 1) == ERR_ARG and call(sw=PTR + 2) == ERR_ARG and call(sw=PTR + 1, w_dtype=F16) == ERR_ARG
    assert call(bias=PTR + 4, h=PTR + 8, flag=PTR + 4, tokens=0) == OK


# ------------------------------------------------------------------------------------------------------------ the wrappers
def test_python_wrappers_refuse_before_the_library(lib):
    from fpqvar_amd import gemm
    a, sa = torch.zeros(4, 192, dtype=torch.uint8), torch.zeros(4, 2, dtype=torch.float16)
    w, sw = torch.zeros(128, 128, dtype=torch.uint8), torch.zeros(128, 2)
    with pytest.raises(RuntimeError, match="GPU"):
        gemm.linear_a6w4_gelu_dual(a, sa, "e3m0", w, sw)
    lin = torch.nn.Linear(256, 128)
    with pytest.raises(ValueError, match="no k-major form"):
        gemm.FP4LinearGeluDual.from_float(lin, kmajor=True, act_fp_type="fp_e3")
    with pytest.raises(ValueError, match="no k-major form"):
        gemm.FP4LinearGeluDual.from_float(lin, kmajor=True, act_fp_type="fp_e1")


def test_wrapper_refuses_images_and_shapes(lib, monkeypatch):
    """the refusals behind the GPU test, reached on CPU tensors with that test switched off: 3-D operands (there is no k-major
    A6W4 form), an unknown table, outs % 128"""
    from fpqvar_amd import gemm
    monkeypatch.setattr(gemm, "require_gpu", lambda *a, **k: None)
    a, sa = torch.zeros(4, 192, dtype=torch.uint8), torch.zeros(4, 2, dtype=torch.float16)
    w, sw = torch.zeros(128, 128, dtype=torch.uint8), torch.zeros(128, 2)
    with pytest.raises(RuntimeError, match="row-major operands only"):
        gemm.linear_a6w4_gelu_dual(torch.zeros(2, 4, 96, dtype=torch.uint8), sa, "e3m0", torch.zeros(2, 128, 64, dtype=torch.uint8), sw)
    with pytest.raises(RuntimeError, match="row-major operands only"):
        gemm.linear_a6w4_gelu_dual(a, sa, "e3m0", torch.zeros(2, 128, 64, dtype=torch.uint8), sw)
    with pytest.raises(RuntimeError, match="'e1m2' and 'e3m0'"):
        gemm.linear_a6w4_gelu_dual(a, sa, "e2m1", w, sw)
    with pytest.raises(RuntimeError, match="multiple of 128"):
        gemm.linear_a6w4_gelu_dual(a, sa, "e3m0", w[:120], sw[:120])
    with pytest.raises(RuntimeError, match="mismatch"):
        gemm.linear_a6w4_gelu_dual(a[:, :96], sa, "e3m0", w, sw)


# ------------------------------------------------------------------------------------------------------------ the kernels
def test_the_eight_fc1_instantiations_do_not_spill(lib, tmp_path):
    """{E1M2, E3M0 activation} x {fp16, fp32 weight scales} x {64, 128 rows} of gemm_a6w4_fc1_kernel: no scratch, no spill, at most
    256 registers per lane (__launch_bounds__(256, 2), as the plain kernel), no static LDS.  The library is the one the `lib`
    fixture built: a missing library fails this test."""
    assert os.path.exists(LIB), "libfpq_hip.so is missing after the build"
    ks = [(n, r) for n, r in kernel_metadata(tmp_path) if "gemm_a6w4_fc1_kernel" in n]
    assert len(ks) == 8, [n for n, _ in ks]
    got = set()
    for n, r in ks:
        m = re.search(r"gemm_a6w4_fc1_kernelI(DF16_|f)Li(\d)ELi4ELi(\d)E", n)
        assert m, n
        got.add((m.group(1), int(m.group(2)), int(m.group(3))))
        assert int(r.get("vgpr_spill_count", 0)) == 0 and int(r.get("sgpr_spill_count", 0)) == 0, (n, r)
        assert int(r.get("private_segment_fixed_size", 0)) == 0, (n, r.get("private_segment_fixed_size"))
        assert int(r["vgpr_count"]) + int(r.get("agpr_count", 0)) <= 256, (n, r["vgpr_count"])
        assert int(r.get("group_segment_fixed_size", 0)) == 0, n
    assert got == {(t, mt, fa) for t in ("DF16_", "f") for mt in (2, 4) for fa in (2, 3)}


# ------------------------------------------------------------------------------------------------------------ the wiring
class _Marker(torch.nn.Module):
    def __init__(self, cls, kmajor, act):
        super().__init__()
        self.cls_name, self.kmajor_arg, self.act = cls.__name__, kmajor, act


@pytest.fixture
def cpu_construction(monkeypatch):
    """Quantizing a weight needs the GPU: on the CPU the weight quantizer is an identity and FP4Linear.from_float (which
    FP4LinearGeluDual inherits) records the class it was asked for and its arguments, so the walk runs as it is."""
    from fpqvar_amd import gemm, quant_linear as ql
    monkeypatch.setattr(ql, "_quantize_weight", lambda w, *a, **k: w)
    monkeypatch.setattr(gemm.FP4Linear, "from_float", classmethod(lambda cls, lin, kmajor=False, act_fp_type="fp_e2": _Marker(cls, kmajor, act_fp_type)))
    return ql


def _classes(model):
    return {n: (m.cls_name, m.kmajor_arg, m.act) if isinstance(m, _Marker) else type(m).__name__
            for n, m in model.named_modules() if not list(m.children()) or isinstance(m, _Marker)}


@pytest.mark.parametrize("fn", ("quantize_VAR_mixed_fp4_datatype", "quantize_VAR_use_different_datatype"))
def test_fuse_ffn_asks_for_a_gelu_dual_fc1_in_every_block(cpu_construction, fn):
    """d30-shaped, 30 blocks: fc1 is an FP4LinearGeluDual everywhere - fp_e2 and k-major in blocks 6-20, fp_e3 and row-major
    elsewhere -, `act` an Identity, fc2 a QuantizedLinear_fc2 whose quantizer is named "in fc1's epilogue" and is the identity;
    the attention Linears and ada_lin[1] are what real_fp4 alone makes them."""
    ql = cpu_construction
    torch.manual_seed(0)
    plain = getattr(ql, fn)(_Var(128, 30), real_fp4=True, **W4A4)
    fused = getattr(ql, fn)(_Var(128, 30), real_fp4=True, fuse_ffn=True, **W4A4)
    x = torch.randn(3, 512)
    for b, blk in enumerate(fused.blocks):
        want = "fp_e2" if 6 <= b <= 20 else "fp_e3"
        fc1 = blk.ffn.fc1
        assert isinstance(fc1, _Marker) and fc1.cls_name == "FP4LinearGeluDual", (b, type(fc1))
        assert fc1.act == want and fc1.kmajor_arg == (want == "fp_e2"), (b, fc1.act, fc1.kmajor_arg)
        assert isinstance(blk.ffn.act, torch.nn.Identity)
        assert type(blk.ffn.fc2) is ql.QuantizedLinear_fc2 and blk.ffn.fc2.act_quant_name == "in fc1's epilogue"
        assert "in fc1's epilogue" in repr(blk.ffn.fc2) and blk.ffn.fc2.act_quant(x) is x
        assert plain.blocks[b].ffn.fc1.cls_name == "FP4Linear" and isinstance(plain.blocks[b].ffn.act, torch.nn.GELU)
    strip = lambda d: {n: v for n, v in d.items() if ".ffn." not in n}
    assert strip(_classes(fused)) == strip(_classes(plain))
    rowmajor = getattr(ql, fn)(_Var(128, 8), real_fp4=True, fuse_ffn=True, kmajor_operands=False, **W4A4)
    assert not any(m.kmajor_arg for m in rowmajor.modules() if isinstance(m, _Marker))
    assert all(blk.ffn.fc1.cls_name == "FP4LinearGeluDual" for blk in rowmajor.blocks)


@pytest.mark.parametrize("fn", ("quantize_VAR_mixed_fp4_datatype", "quantize_VAR_use_different_datatype"))
def test_without_fuse_ffn_nothing_changes(cpu_construction, fn):
    ql = cpu_construction
    for real in (False, True):
        torch.manual_seed(0)
        default = getattr(ql, fn)(_Var(128, 30), real_fp4=real, **W4A4)
        off = getattr(ql, fn)(_Var(128, 30), real_fp4=real, fuse_ffn=False, **W4A4)
        assert _classes(off) == _classes(default)
        for blk in default.blocks:
            assert isinstance(blk.ffn.act, torch.nn.GELU) and blk.ffn.fc2.act_quant_name == "per_group"
            assert (blk.ffn.fc1.cls_name == "FP4Linear") if real else (type(blk.ffn.fc1) is ql.QuantizedLinear)


def test_fuse_ffn_one_pass_and_refusals(cpu_construction):
    ql = cpu_construction
    msg = "fuse_ffn needs an FFN with act = GELU"
    for fn in (ql.quantize_VAR_mixed_fp4_datatype, ql.quantize_VAR_use_different_datatype):
        with pytest.raises(ValueError, match=msg):
            fn(_Var(128, 1), real_fp4=True, fuse_ffn=True, **dict(W4A4, fc2_fp_type="fp_e2"))     # not a dual format
        with pytest.raises(ValueError, match=msg):
            fn(_Var(128, 1), fuse_ffn=True, **dict(W4A4, fc2_fp_type="fp_e2"))
    erf = _Var(128, 1)
    erf.blocks[0].ffn.act = torch.nn.GELU()                                                           # not GELU(tanh)
    with pytest.raises(ValueError, match=msg):
        ql.quantize_VAR_mixed_fp4_datatype(erf, real_fp4=True, fuse_ffn=True, **W4A4)
    # without real_fp4 (fake quantization), or with a dual format the GEMM's tail does not compute: GELU + quantizer in one pass
    for kw in (dict(W4A4), dict(W4A4, real_fp4=True, fc2_fp_type="fp4_afpq")):
        m = ql.quantize_VAR_mixed_fp4_datatype(_Var(128, 7), fuse_ffn=True, **kw)
        for blk in m.blocks:
            assert isinstance(blk.ffn.act, ql.GeluThenFc2Quant) and blk.ffn.act.fc2_fp_type == kw["fc2_fp_type"]
            assert blk.ffn.fc2.act_quant_name == "behind the GELU (one pass)"
            assert (blk.ffn.fc1.cls_name == "FP4Linear") if kw.get("real_fp4") else (type(blk.ffn.fc1) is ql.QuantizedLinear)
    # an fc1 the GEMM does not take (an E3M0 weight; out_features % 128) falls to the one-pass form
    mk = {k: v for k, v in W4A4.items() if k not in ("act_fp_type", "weight_fp_type", "fc2_fp_type")}
    fmt = lambda b, layer: {"fc1": ("fp_e3", "fp_e3"), "fc2": ("fp_e1m2_neg_e2m1_pos", "fp_e2")}.get(layer, ("fp_e2", "fp_e2"))
    m = ql.quantize_VAR_mixed(_Var(128, 1), fmt, real_fp4=True, fuse_ffn=True, **mk)
    assert type(m.blocks[0].ffn.fc1) is ql.QuantizedLinear and isinstance(m.blocks[0].ffn.act, ql.GeluThenFc2Quant)
    fmt1 = lambda b, layer: {"fc1": ("fp_e1", "fp_e2"), "fc2": ("fp_e1m2_neg_e2m1_pos", "fp_e2")}.get(layer, ("fp_e2", "fp_e2"))
    m = ql.quantize_VAR_mixed(_Var(128, 1), fmt1, real_fp4=True, fuse_ffn=True, **mk)
    assert m.blocks[0].ffn.fc1.cls_name == "FP4LinearGeluDual" and m.blocks[0].ffn.fc1.act == "fp_e1" and not m.blocks[0].ffn.fc1.kmajor_arg
