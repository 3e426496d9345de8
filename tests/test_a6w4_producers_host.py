"""The rotate and adaLN producers emitting the A6W4 GEMM's activation operands (fpq_a6w4_rotate_quant_rows_codes,
fpq_a6w4_adaln_rotate_quant_rows_codes; rotation.rotate_quant_g6 / adaln_rotate_quant_g6; FP4Linear.adaln_operands /
rotate_operands / qkv_to_cache_operands) without a GPU: export, declaration and registration of the two entry points, their argument
checks in the documented order (nothing is launched: every call is refused, or has nothing to do), the Python wrappers' refusals,
and which producer a module asks for."""
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
NEW = {"fpq_a6w4_rotate_quant_rows_codes": 11, "fpq_a6w4_adaln_rotate_quant_rows_codes": 16}   # name -> arguments
MASK = (ctypes.c_uint32 * 4)(1, 2, 3, 4)


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as g
    g.build_hip()
    from fpqvar_amd import _lib
    return _lib.lib()


def test_version_exports_declarations_and_argument_counts(lib):
    from fpqvar_amd import _lib
    assert lib.fpq_version() >= 135
    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "fpq.h")).read(), flags=re.S)
    for name, n_args in NEW.items():
        assert hasattr(lib, name), name
        assert name in _lib._SIGS and len(_lib._SIGS[name][1]) == n_args, name
        decl = re.search(r"\bint\s+" + name + r"\s*\(([^)]*)\)", hdr)
        assert decl, f"{name} is not declared in include/fpq.h"
        assert len(decl.group(1).split(",")) == n_args, name


def _call(lib, adaln):
    """the entry point with every argument valid (fake aligned pointers) unless overridden"""
    def call(x=PTR, codes=PTR, scales=PTR, rows=4, cols=256, dtype=F16, scale=PTR, shift=PTR, mod=F16, l=2, smooth=None, mask=MASK,
             table=E3M0, kmajor=0):
        if adaln:
            return lib.fpq_a6w4_adaln_rotate_quant_rows_codes(x, codes, scales, rows, cols, dtype, scale, shift, mod, l, 1e-6, smooth, mask,
                                                              table, kmajor, None)
        return lib.fpq_a6w4_rotate_quant_rows_codes(x, codes, scales, rows, cols, dtype, smooth, mask, table, kmajor, None)
    return call


@pytest.mark.parametrize("adaln", (False, True))
def test_every_refusal(lib, adaln):
    call = _call(lib, adaln)
    for km in (0, 1):
        for t in (E2M1, E2M3, E3M2, 9, -1):
            assert call(table=t, kmajor=km) == ERR_TABLE, t
        assert call(dtype=F64, kmajor=km) == ERR_DTYPE
        assert call(cols=100, kmajor=km) == ERR_SHAPE and call(cols=64, kmajor=km) == ERR_SHAPE
        assert call(rows=-1, kmajor=km) == ERR_ARG and call(cols=-128, kmajor=km) == ERR_ARG
        assert call(mask=None, kmajor=km) == ERR_ARG
        for table in (E1M2, E3M0):                                        # nothing to do: FPQ_OK, nothing launched
            assert call(rows=0, table=table, kmajor=km) == OK and call(cols=0, table=table, kmajor=km) == OK
        assert call(rows=0, x=None, codes=None, scales=None, kmajor=km) == OK
        for name in ("x", "codes", "scales"):
            assert call(**{name: None}, kmajor=km) == ERR_ARG, name
            assert call(**{name: PTR + 8}, kmajor=km) == ERR_ARG, name
        assert call(smooth=PTR + 4, kmajor=km) == ERR_ARG
    assert call(rows=1 << 22, cols=1024, kmajor=1) == ERR_SHAPE             # a 3 GiB image: k-major images stay below 2 GiB
    if adaln:
        assert call(mod=F64) == ERR_DTYPE
        assert call(cols=2688) == ERR_SHAPE and call(cols=4096) == ERR_SHAPE   # the matrix-core kernel only
        assert call(l=0) == ERR_ARG and call(l=-3) == ERR_ARG
        for name in ("scale", "shift"):
            assert call(**{name: None}) == ERR_ARG, name
            assert call(**{name: PTR + 8}) == ERR_ARG, name


@pytest.mark.parametrize("adaln", (False, True))
def test_order_of_two_simultaneous_faults(lib, adaln):
    """negative sizes / NULL sign mask, table, dtypes, shape, nothing to do, then pointers"""
    call = _call(lib, adaln)
    assert call(rows=-1, table=E2M1) == ERR_ARG and call(mask=None, table=E2M3) == ERR_ARG      # sizes / mask before the table
    assert call(table=E2M1, dtype=F64) == ERR_TABLE and call(table=E2M3, cols=100) == ERR_TABLE   # table before dtype and shape
    assert call(table=E2M1, rows=0) == ERR_TABLE
    assert call(dtype=F64, cols=100) == ERR_DTYPE and call(dtype=F64, rows=0) == ERR_DTYPE        # dtype before shape and "empty"
    assert call(cols=100, rows=0) == ERR_SHAPE and call(cols=100, x=None) == ERR_SHAPE            # shape before "empty" and pointers
    assert call(rows=0, x=PTR + 8, codes=None) == OK                                              # "empty" before the pointers
    if adaln:
        assert call(l=0, table=E2M1) == ERR_ARG
        assert call(mod=F64, cols=2688) == ERR_DTYPE
        assert call(cols=2688, rows=0) == ERR_SHAPE and call(cols=2688, scale=None) == ERR_SHAPE


# --------------------------------------------------------------------------------------------------------------- Python
def test_python_wrappers_refuse_before_the_library(lib, monkeypatch):
    from fpqvar_amd import rotation as rot
    x = torch.zeros(2, 3, 256, dtype=torch.float16)
    sc = torch.zeros(2, 1, 256, dtype=torch.float16)
    with pytest.raises(RuntimeError, match="GPU"):
        rot.rotate_quant_g6(x)
    with pytest.raises(RuntimeError, match="GPU"):
        rot.adaln_rotate_quant_g6(x, sc, sc)
    monkeypatch.setattr(rot, "require_gpu", lambda *a, **k: None)
    touched = []
    monkeypatch.setattr(rot, "lib", lambda: touched.append("lib"))
    monkeypatch.setattr(rot, "_native", None)
    for table in ("e2m1", "e2m3", "fp_e2", "nope", None):
        with pytest.raises(RuntimeError, match="'e1m2' and 'e3m0'"):
            rot.rotate_quant_g6(x, table)
        with pytest.raises(RuntimeError, match="'e1m2' and 'e3m0'"):
            rot.adaln_rotate_quant_g6(x, sc, sc, table)
    with pytest.raises(RuntimeError, match="multiple of 128"):
        rot.rotate_quant_g6(torch.zeros(4, 100, dtype=torch.float16))
    with pytest.raises(RuntimeError, match="float16/float32"):
        rot.rotate_quant_g6(x.double())
    with pytest.raises(RuntimeError, match=r"\[B, L, C\]"):
        rot.adaln_rotate_quant_g6(x.view(6, 256), sc, sc)
    with pytest.raises(RuntimeError, match="both be float16 or both float32"):
        rot.adaln_rotate_quant_g6(x, sc, sc.float())
    with pytest.raises(RuntimeError, match="both be float16 or both float32"):
        rot.adaln_rotate_quant_g6(x, sc.double(), sc.double())
    with pytest.raises(RuntimeError, match="at most 2560"):
        rot.adaln_rotate_quant_g6(torch.zeros(1, 2, 2688, dtype=torch.float16), sc, sc)
    assert not touched, "a refused call reached the library"


@pytest.mark.parametrize("kmajor", (False, True))
@pytest.mark.parametrize("act,table", (("fp_e2", "e2m1"), ("fp_e1", "e1m2"), ("fp_e3", "e3m0")))
def test_a_module_asks_for_its_own_producer(monkeypatch, act, table, kmajor):
    """adaln_operands / rotate_operands: the _mx producers for an E2M1 module, the _g6 producers with the module's table otherwise,
    k-major iff the weight is an image; qkv_to_cache_operands is qkv_to_cache without the quantizer"""
    from fpqvar_amd import gemm, rotation as rot
    calls = []
    for name in ("adaln_rotate_quant_mx", "rotate_quant_mx", "adaln_rotate_quant_g6", "rotate_quant_g6"):
        monkeypatch.setattr(rot, name, lambda *a, _n=name, **k: calls.append((_n, a, k)) or ("codes", "scales"))
    w = torch.zeros((2, 64, 64) if kmajor else (64, 128), dtype=torch.uint8)
    m = gemm.FP4Linear(w, torch.zeros(1), None, 256, 64, table)
    assert m.kmajor == kmajor
    x, sc, sh, sm = object(), object(), object(), object()
    assert m.adaln_operands(x, sc, sh, smooth=sm, eps=1e-5) == ("codes", "scales")
    assert m.rotate_operands(x, smooth=sm) == ("codes", "scales")
    (n1, a1, k1), (n2, a2, k2) = calls
    if table == "e2m1":
        assert (n1, a1, n2, a2) == ("adaln_rotate_quant_mx", (x, sc, sh), "rotate_quant_mx", (x,))
    else:
        assert (n1, a1, n2, a2) == ("adaln_rotate_quant_g6", (x, sc, sh, table), "rotate_quant_g6", (x, table))
    assert k1 == dict(d=None, smooth=sm, eps=1e-5, kmajor=kmajor) and k2 == dict(d=None, smooth=sm, kmajor=kmajor)
    ran = []
    monkeypatch.setattr(m, "_run", lambda *a: ran.append(a) or "q")
    monkeypatch.setattr(m, "_quantize", lambda t: ("c", "s"))
    assert m.qkv_to_cache_operands("c", "s", "cache", 3, 5) == "q" and m.qkv_to_cache("x", "cache", 3, 5) == "q"
    assert ran[0] == ran[1] == ("qkv_to_cache", None, "c", "s", None, "cache", 3, 5, None)
    with pytest.raises(RuntimeError, match="without qk_norm_scale"):
        m.qkv_to_cache_operands("c", "s", "cache", 3, 5, bias=torch.zeros(3))
