"""The rotate and adaLN producers emitting per-group operands on the FULL FP6 tables (fpq_gf6_rotate_quant_rows_codes,
fpq_gf6_adaln_rotate_quant_rows_codes; rotation.rotate_quant_gf6 / adaln_rotate_quant_gf6; FP6GroupLinear.adaln_operands /
rotate_operands) without a GPU: export, declaration and registration of the two entry points, their argument lists against the A6W4
twins', their argument checks in the documented order (nothing is launched: every call is refused, or has nothing to do), the Python
wrappers' refusals, which producer a module asks for, and the register / LDS figures of the rotate kernel's table-free forms."""
import ctypes
import os
import re

import pytest
import torch

OK, ERR_ARG, ERR_DTYPE, ERR_SHAPE, ERR_TABLE = 0, -1, -2, -3, -4
F16, F32, F64 = 0, 1, 2
E2M1, E1M2, E3M0, E2M3, E3M2 = 0, 1, 2, 3, 4   # enum fpq_table
PTR = 0x7000_0000_1000   # an address with every alignment the checks ask for; nothing reads it
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = {"fpq_gf6_rotate_quant_rows_codes": 11, "fpq_gf6_adaln_rotate_quant_rows_codes": 16}   # name -> arguments
TWIN = {"fpq_gf6_rotate_quant_rows_codes": "fpq_a6w4_rotate_quant_rows_codes",
        "fpq_gf6_adaln_rotate_quant_rows_codes": "fpq_a6w4_adaln_rotate_quant_rows_codes"}
MASK = (ctypes.c_uint32 * 4)(1, 2, 3, 4)


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as g
    g.build_hip()
    from fpqvar_amd import _lib
    return _lib.lib()


def test_exports_declarations_argument_counts_and_the_twins_argtypes(lib):
    from fpqvar_amd import _lib
    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "fpq.h")).read(), flags=re.S)
    assert re.search(r"#define\s+FPQ_VERSION\s+136\b", hdr), "additions are looked up by name: the version stays"
    for name, n_args in NEW.items():
        assert hasattr(lib, name), name
        assert name in _lib._SIGS and len(_lib._SIGS[name][1]) == n_args, name
        assert _lib._SIGS[name] == _lib._SIGS[TWIN[name]], f"{name}: the argument list is the A6W4 twin's"
        assert list(getattr(lib, name).argtypes) == list(getattr(lib, TWIN[name]).argtypes), name
        assert getattr(lib, name).restype is getattr(lib, TWIN[name]).restype
        decl = re.search(r"\bint\s+" + name + r"\s*\(([^)]*)\)", hdr)
        assert decl, f"{name} is not declared in include/fpq.h"
        assert len(decl.group(1).split(",")) == n_args, name
        twin = re.search(r"\bint\s+" + TWIN[name] + r"\s*\(([^)]*)\)", hdr)
        assert re.sub(r"\s+", " ", decl.group(1)) == re.sub(r"\s+", " ", twin.group(1)), f"{name}: declared with the twin's parameters"


def _call(lib, adaln):
    """the entry point with every argument valid (fake aligned pointers) unless overridden"""
    def call(x=PTR, codes=PTR, scales=PTR, rows=4, cols=256, dtype=F16, scale=PTR, shift=PTR, mod=F16, l=2, smooth=None, mask=MASK,
             table=E2M3, kmajor=0):
        if adaln:
            return lib.fpq_gf6_adaln_rotate_quant_rows_codes(x, codes, scales, rows, cols, dtype, scale, shift, mod, l, 1e-6, smooth, mask,
                                                             table, kmajor, None)
        return lib.fpq_gf6_rotate_quant_rows_codes(x, codes, scales, rows, cols, dtype, smooth, mask, table, kmajor, None)
    return call


@pytest.mark.parametrize("adaln", (False, True))
def test_every_refusal(lib, adaln):
    call = _call(lib, adaln)
    for km in (0, 1):
        for t in (E2M1, E1M2, E3M0, 9, -1):
            assert call(table=t, kmajor=km) == ERR_TABLE, t
        for table in (E2M3, E3M2):
            assert call(dtype=F64, table=table, kmajor=km) == ERR_DTYPE
            assert call(cols=100, table=table, kmajor=km) == ERR_SHAPE and call(cols=64, table=table, kmajor=km) == ERR_SHAPE
            assert call(rows=-1, table=table, kmajor=km) == ERR_ARG and call(cols=-128, table=table, kmajor=km) == ERR_ARG
            assert call(mask=None, table=table, kmajor=km) == ERR_ARG
            # accepted tables with nothing to do: FPQ_OK, nothing launched
            assert call(rows=0, table=table, kmajor=km) == OK and call(cols=0, table=table, kmajor=km) == OK
            assert call(rows=0, x=None, codes=None, scales=None, table=table, kmajor=km) == OK
            for name in ("x", "codes", "scales"):
                assert call(**{name: None}, table=table, kmajor=km) == ERR_ARG, name
                assert call(**{name: PTR + 8}, table=table, kmajor=km) == ERR_ARG, name
            assert call(smooth=PTR + 4, table=table, kmajor=km) == ERR_ARG
    assert call(rows=1 << 22, cols=1024, kmajor=1) == ERR_SHAPE             # a 3 GiB image: k-major images stay below 2 GiB
    if adaln:
        assert call(mod=F64) == ERR_DTYPE
        assert call(cols=2688) == ERR_SHAPE and call(cols=4096) == ERR_SHAPE   # the matrix-core kernel only
        assert call(l=0) == ERR_ARG and call(l=-3) == ERR_ARG
        for name in ("scale", "shift"):
            assert call(**{name: None}) == ERR_ARG, name
            assert call(**{name: PTR + 8}) == ERR_ARG, name


@pytest.mark.parametrize("kmajor", (0, 1))
@pytest.mark.parametrize("adaln", (False, True))
def test_order_of_two_simultaneous_faults(lib, adaln, kmajor):
    """negative sizes / NULL sign mask, table, dtypes, shape, nothing to do, then pointers"""
    base = _call(lib, adaln)
    call = lambda **kw: base(kmajor=kmajor, **kw)
    assert call(rows=-1, table=E2M1) == ERR_ARG and call(mask=None, table=E3M0) == ERR_ARG      # sizes / mask before the table
    assert call(table=E2M1, dtype=F64) == ERR_TABLE and call(table=E1M2, cols=100) == ERR_TABLE   # table before dtype and shape
    assert call(table=E3M0, rows=0) == ERR_TABLE
    assert call(dtype=F64, cols=100) == ERR_DTYPE and call(dtype=F64, rows=0) == ERR_DTYPE        # dtype before shape and "empty"
    assert call(cols=100, rows=0) == ERR_SHAPE and call(cols=100, x=None) == ERR_SHAPE            # shape before "empty" and pointers
    assert call(rows=0, x=PTR + 8, codes=None) == OK                                              # "empty" before the pointers
    if kmajor:
        assert call(rows=1 << 22, cols=1024, dtype=F64) == ERR_DTYPE and call(rows=1 << 22, cols=1024, x=None) == ERR_SHAPE
    if adaln:
        assert call(l=0, table=E2M1) == ERR_ARG
        assert call(mod=F64, cols=2688) == ERR_DTYPE
        assert call(cols=2688, rows=0) == ERR_SHAPE and call(cols=2688, scale=None) == ERR_SHAPE


def test_the_a6w4_names_keep_refusing_the_full_tables(lib):
    for t in (E2M3, E3M2):
        assert lib.fpq_a6w4_rotate_quant_rows_codes(PTR, PTR, PTR, 4, 256, F16, None, MASK, t, 0, None) == ERR_TABLE
        assert lib.fpq_a6w4_adaln_rotate_quant_rows_codes(PTR, PTR, PTR, 4, 256, F16, PTR, PTR, F16, 2, 1e-6, None, MASK, t, 0, None) == ERR_TABLE


# --------------------------------------------------------------------------------------------------------------- Python
def test_python_wrappers_refuse_before_the_library(lib, monkeypatch):
    from fpqvar_amd import rotation as rot
    x = torch.zeros(2, 3, 256, dtype=torch.float16)
    sc = torch.zeros(2, 1, 256, dtype=torch.float16)
    with pytest.raises(RuntimeError, match="GPU"):
        rot.rotate_quant_gf6(x)
    with pytest.raises(RuntimeError, match="GPU"):
        rot.adaln_rotate_quant_gf6(x, sc, sc)
    monkeypatch.setattr(rot, "require_gpu", lambda *a, **k: None)
    touched = []
    monkeypatch.setattr(rot, "lib", lambda: touched.append("lib"))
    monkeypatch.setattr(rot, "_native", None)
    for table in ("e1m2", "e3m0", "e2m1", "fp_e1", "nope", None):
        with pytest.raises(RuntimeError, match="'e2m3' and 'e3m2'"):
            rot.rotate_quant_gf6(x, table)
        with pytest.raises(RuntimeError, match="'e2m3' and 'e3m2'"):
            rot.adaln_rotate_quant_gf6(x, sc, sc, table)
    with pytest.raises(RuntimeError, match="multiple of 128"):
        rot.rotate_quant_gf6(torch.zeros(4, 100, dtype=torch.float16))
    with pytest.raises(RuntimeError, match="float16/float32"):
        rot.rotate_quant_gf6(x.double())
    with pytest.raises(RuntimeError, match=r"\[B, L, C\]"):
        rot.adaln_rotate_quant_gf6(x.view(6, 256), sc, sc)
    with pytest.raises(RuntimeError, match="both be float16 or both float32"):
        rot.adaln_rotate_quant_gf6(x, sc, sc.float())
    with pytest.raises(RuntimeError, match="both be float16 or both float32"):
        rot.adaln_rotate_quant_gf6(x, sc.double(), sc.double())
    with pytest.raises(RuntimeError, match="at most 2560"):
        rot.adaln_rotate_quant_gf6(torch.zeros(1, 2, 2688, dtype=torch.float16), sc, sc)
    assert not touched, "a refused call reached the library"


@pytest.mark.parametrize("name", ("e2m3", "e3m2", "fp6_e2m3", "fp6_e3m2"))
def test_python_wrappers_accept_both_spellings(monkeypatch, name):
    """the table id that reaches the library is the full table's, under either spelling"""
    from fpqvar_amd import rotation as rot
    assert rot._gf6_table_id("t", name) == (E2M3 if name.endswith("e2m3") else E3M2)


PRODUCERS = ("adaln_rotate_quant_mx", "rotate_quant_mx", "adaln_rotate_quant_g6", "rotate_quant_g6", "adaln_rotate_quant_gf6", "rotate_quant_gf6")


@pytest.mark.parametrize("kmajor", (False, True))
@pytest.mark.parametrize("cls", ("FP6GroupLinear", "FP6GroupLinearGeluDual"))
@pytest.mark.parametrize("act,weight", (("e2m3", "e2m3"), ("e3m2", "e2m1"), ("e2m3", "e2m1"), ("e3m2", "e1m2"),
                                        ("e2m1", "e2m3"), ("e1m2", "e2m3"), ("e3m0", "e2m3")))
def test_a_module_asks_for_its_own_producer(monkeypatch, act, weight, cls, kmajor):
    """adaln_operands / rotate_operands of FP6GroupLinear: the _gf6 producers with the module's table for an e2m3 / e3m2 activation,
    the parent's choice otherwise (_mx for E2M1, _g6 for E1M2 / E3M0); k-major iff the weight is an image"""
    from fpqvar_amd import gemm, rotation as rot
    calls = []
    for name in PRODUCERS:
        monkeypatch.setattr(rot, name, lambda *a, _n=name, **k: calls.append((_n, a, k)) or ("codes", "scales"))
    seg = 64 if weight == "e2m1" else 96
    w = torch.zeros((2, 128, seg) if kmajor else (128, 2 * seg), dtype=torch.uint8)
    m = getattr(gemm, cls)(w, torch.zeros(1), None, 256, 128, act, weight)
    assert m.kmajor == kmajor and m.act_table == act
    x, sc, sh, sm = object(), object(), object(), object()
    assert m.adaln_operands(x, sc, sh, smooth=sm, eps=1e-5) == ("codes", "scales")
    assert m.rotate_operands(x, smooth=sm) == ("codes", "scales")
    (n1, a1, k1), (n2, a2, k2) = calls
    if act == "e2m1":
        assert (n1, a1, n2, a2) == ("adaln_rotate_quant_mx", (x, sc, sh), "rotate_quant_mx", (x,))
    elif act in ("e1m2", "e3m0"):
        assert (n1, a1, n2, a2) == ("adaln_rotate_quant_g6", (x, sc, sh, act), "rotate_quant_g6", (x, act))
    else:
        assert (n1, a1, n2, a2) == ("adaln_rotate_quant_gf6", (x, sc, sh, act), "rotate_quant_gf6", (x, act))
    assert k1 == dict(d=None, smooth=sm, eps=1e-5, kmajor=kmajor) and k2 == dict(d=None, smooth=sm, kmajor=kmajor)


def test_fp4linear_itself_is_untouched(monkeypatch):
    """an FP4Linear never reaches the _gf6 producers: its formats are E2M1 / E1M2 / E3M0"""
    from fpqvar_amd import gemm, rotation as rot
    calls = []
    for name in PRODUCERS:
        monkeypatch.setattr(rot, name, lambda *a, _n=name, **k: calls.append(_n) or ("codes", "scales"))
    for table in ("e2m1", "e1m2", "e3m0"):
        m = gemm.FP4Linear(torch.zeros(64, 128, dtype=torch.uint8), torch.zeros(1), None, 256, 64, table)
        m.adaln_operands(object(), object(), object())
        m.rotate_operands(object())
    assert calls and not [n for n in calls if n.endswith("_gf6")]


# ------------------------------------------------------------------------------------- the table-free form of the rotate kernel
def test_hw6_forms_of_the_rotate_kernel_keep_the_register_budget(tmp_path):
    """rotate_quant_mfma_kernel<..., G6, HW6 = 1 | 2> (codes from the FP6 conversion hardware): one instantiation per row dtype,
    smoothing and table; no spill, no scratch, no LDS table (the table forms' static LDS less the 4 KiB of kLutLdsEntries); fp16 rows
    without a smoothing vector stay at 6 wavefronts per SIMD (<= 80 registers), with one at 5 (<= 96)"""
    from tests.test_no_spill import kernel_metadata
    recs = kernel_metadata(tmp_path)
    form = lambda n: re.search(r"rotate_quant_mfma_kernelI(DF16_|f)Lb0ELb([01])ELb1ELb0ELb1ELi([012])E", n)
    got = {form(n).groups(): r for n, r in recs if form(n)}
    assert sorted(got) == sorted((t, sm, hw) for t in ("DF16_", "f") for sm in "01" for hw in "012"), sorted(got)
    for (t, sm, hw), r in got.items():
        assert int(r.get("vgpr_spill_count", 0)) == 0 and int(r.get("sgpr_spill_count", 0)) == 0, (t, sm, hw)
        assert int(r.get("private_segment_fixed_size", 0)) == 0, (t, sm, hw)
        if hw != "0":
            assert int(r["group_segment_fixed_size"]) == int(got[t, sm, "0"]["group_segment_fixed_size"]) - 4096, (t, sm, hw)
            if t == "DF16_":
                assert int(r["vgpr_count"]) <= (96 if sm == "1" else 80), (t, sm, hw, r["vgpr_count"])
