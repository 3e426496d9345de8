"""The adaLN producers with the gated residual folded in (fpq_resid_adaln_rotate_quant_rows, _rows_codes_mx, _token_rows,
_token_rows_codes_f6; rotation.resid_adaln_rotate_quant / _mx / _token) without a GPU, in the manner of tests/test_producer_abi_host.py:
export, declaration and registration of the four entry points, their argument lists against the twins', the refusal codes in the
documented order (nothing is launched: every call is refused, or has nothing to do), the Python wrappers' refusals and what they return."""
import contextlib
import ctypes
import os
import re

import pytest
import torch

OK, ERR_ARG, ERR_DTYPE, ERR_SHAPE, ERR_TABLE = 0, -1, -2, -3, -4
F16, F32, F64 = 0, 1, 2
E2M1, E1M2, E3M0, E2M3, E3M2, E1M2_NEG = 0, 1, 2, 3, 4, 5   # enum fpq_table (5: a half table)
PTR = 0x7000_0000_1000   # an address with every alignment the checks ask for; nothing reads it
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MASK = (ctypes.c_uint32 * 4)(1, 2, 3, 4)
TWIN = {"fpq_resid_adaln_rotate_quant_rows": "fpq_adaln_rotate_quant_rows",
        "fpq_resid_adaln_rotate_quant_rows_codes_mx": "fpq_adaln_rotate_quant_rows_codes_mx",
        "fpq_resid_adaln_rotate_quant_token_rows": "fpq_adaln_rotate_quant_token_rows",
        "fpq_resid_adaln_rotate_quant_token_rows_codes_f6": "fpq_adaln_rotate_quant_token_rows_codes_f6"}
FORMS = ("rows", "mx", "token", "f6")


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as g
    g.build_hip()
    from fpqvar_amd import _lib
    return _lib.lib()


def test_exports_declarations_and_the_twins_argument_lists(lib):
    """each takes its twin's list with (y, gate, x_out) in front and `residual` in the place of x; the FP4 form an `int kmajor` more"""
    from fpqvar_amd import _lib
    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "fpq.h")).read(), flags=re.S)
    assert re.search(r"#define\s+FPQ_VERSION\s+136\b", hdr), "additions are looked up by name: the version stays"
    for name, twin in TWIN.items():
        assert hasattr(lib, name), name
        ret, args = _lib._SIGS[name]
        tret, targs = _lib._SIGS[twin]
        want = [ctypes.c_void_p] * 3 + list(targs)
        if name.endswith("_codes_mx"):
            want.insert(len(want) - 1, ctypes.c_int)   # kmajor, in front of the stream
        assert ret is tret and list(args) == want, name
        decl = re.search(r"\bint\s+" + name + r"\s*\(([^)]*)\)", hdr)
        tdecl = re.search(r"\bint\s+" + twin + r"\s*\(([^)]*)\)", hdr)
        assert decl and tdecl, name
        mine = [re.sub(r"\s+", " ", a).strip() for a in decl.group(1).split(",")]
        theirs = [re.sub(r"\s+", " ", a).strip() for a in tdecl.group(1).split(",")]
        assert mine[:4] == ["const void* y", "const void* gate", "void* x_out", "const void* residual"], name
        tail = theirs[1:]
        if name.endswith("_codes_mx"):
            tail.insert(len(tail) - 1, "int kmajor")
        assert mine[4:] == tail, name


def _call(lib, form):
    """the entry point with every argument valid (fake aligned pointers) unless overridden"""
    def call(y=PTR, gate=PTR, x_out=PTR, residual=PTR, out=PTR, h_out=None, rot=None, scales=PTR, rows=4, cols=256, dtype=F16, scale=PTR,
             shift=PTR, mod=F16, l=2, smooth=None, mask=MASK, table=None, kmajor=0):
        if form == "rows":
            return lib.fpq_resid_adaln_rotate_quant_rows(y, gate, x_out, residual, out, h_out, rot, rows, cols, dtype, scale, shift, mod, l,
                                                         1e-6, smooth, mask, E2M1 if table is None else table, None)
        if form == "mx":
            return lib.fpq_resid_adaln_rotate_quant_rows_codes_mx(y, gate, x_out, residual, out, scales, rows, cols, dtype, scale, shift, mod,
                                                                  l, 1e-6, smooth, mask, kmajor, None)
        if form == "token":
            return lib.fpq_resid_adaln_rotate_quant_token_rows(y, gate, x_out, residual, out, h_out, rot, scales, rows, cols, dtype, scale,
                                                               shift, mod, l, 1e-6, smooth, mask, E2M3 if table is None else table, None)
        return lib.fpq_resid_adaln_rotate_quant_token_rows_codes_f6(y, gate, x_out, residual, out, scales, rows, cols, dtype, scale, shift,
                                                                    mod, l, 1e-6, smooth, mask, E2M3 if table is None else table, kmajor, None)
    return call


@pytest.mark.parametrize("form", FORMS)
def test_every_refusal(lib, form):
    call = _call(lib, form)
    kms = (0, 1) if form in ("mx", "f6") else (0,)
    for km in kms:
        # the twin's own
        assert call(rows=-1, kmajor=km) == ERR_ARG and call(cols=-128, kmajor=km) == ERR_ARG
        assert call(l=0, kmajor=km) == ERR_ARG and call(mask=None, kmajor=km) == ERR_ARG
        assert call(dtype=F64, kmajor=km) == ERR_DTYPE and call(mod=F64, kmajor=km) == ERR_DTYPE
        assert call(cols=100, kmajor=km) == ERR_SHAPE and call(cols=4224, kmajor=km) == ERR_SHAPE
        assert call(rows=0, kmajor=km) == OK and call(cols=0, kmajor=km) == OK
        assert call(rows=0, y=None, gate=None, x_out=None, residual=None, out=None, kmajor=km) == OK   # nothing to do: no pointer is looked at
        for name in ("residual", "out", "scale", "shift"):
            assert call(**{name: None}, kmajor=km) == ERR_ARG, name
            assert call(**{name: PTR + 8}, kmajor=km) == ERR_ARG, name
        assert call(smooth=PTR + 4, kmajor=km) == ERR_ARG
        # the three tensors of the residual
        for name in ("y", "gate", "x_out"):
            assert call(**{name: None}, kmajor=km) == ERR_ARG, name
            assert call(**{name: PTR + 8}, kmajor=km) == ERR_ARG, name
        # the first-generation wide kernel has no fused form
        assert call(cols=2688, kmajor=km) == ERR_SHAPE and call(cols=4096, kmajor=km) == ERR_SHAPE
        assert call(cols=2560, y=None, kmajor=km) == ERR_ARG      # 2560 itself is accepted: the next check answers
        # x_out may be the residual itself
        assert call(x_out=PTR, residual=PTR, y=None, kmajor=km) == ERR_ARG
    if form in ("rows", "token"):
        assert call(table=E1M2_NEG) == ERR_TABLE and call(table=99) == ERR_TABLE
        assert call(h_out=PTR + 8) == ERR_ARG and call(rot=PTR + 8) == ERR_ARG
    if form in ("mx", "f6"):
        assert call(scales=None) == ERR_ARG
    if form == "token":
        assert call(scales=PTR + 1) == ERR_ARG
    if form == "f6":
        for t in (E2M1, E1M2, E3M0, 9):
            assert call(table=t) == ERR_TABLE
        assert call(table=E3M2, y=None) == ERR_ARG
        assert call(out=PTR + 4) == ERR_ARG
    if form == "mx":
        assert call(rows=1 << 22, cols=1024, kmajor=1) == ERR_SHAPE   # k-major images stay below 2 GiB


@pytest.mark.parametrize("form", FORMS)
def test_the_twins_checks_come_first_in_the_twins_order(lib, form):
    """sizes / mask, table, dtypes, shape, nothing to do, the twin's pointers - then y / gate / x_out NULL, their alignment, cols > 2560"""
    call = _call(lib, form)
    assert call(rows=-1, y=None) == ERR_ARG and call(dtype=F64, y=None) == ERR_DTYPE and call(dtype=F64, cols=2688) == ERR_DTYPE
    assert call(cols=100, y=None) == ERR_SHAPE and call(cols=100, rows=0) == ERR_SHAPE
    assert call(cols=4224, gate=PTR + 8) == ERR_SHAPE                   # the twin's own width limit
    assert call(rows=0, y=None, cols=2688) == OK                        # "nothing to do" is the twin's check: before everything of ours
    assert call(residual=None, cols=2688) == ERR_ARG                    # the twin's pointers before the width
    assert call(scale=PTR + 8, cols=2688) == ERR_ARG
    if form in ("rows", "mx"):
        assert call(y=None, cols=2688) == ERR_ARG and call(x_out=None, cols=4096) == ERR_ARG        # NULL before the width
        assert call(gate=PTR + 8, cols=2688) == ERR_ARG and call(x_out=PTR + 4, cols=2688) == ERR_ARG   # alignment before the width
    else:   # the per-token twins refuse such rows themselves, behind their pointer checks: that answer comes first
        assert call(y=None, cols=2688) == ERR_SHAPE and call(gate=PTR + 8, cols=4096) == ERR_SHAPE
    assert call(y=None, gate=PTR + 8) == ERR_ARG and call(x_out=PTR + 4) == ERR_ARG
    assert call(cols=2688) == ERR_SHAPE
    if form in ("rows", "token"):
        assert call(table=99, dtype=F64) == ERR_TABLE and call(table=99, y=None) == ERR_TABLE
    if form == "f6":
        assert call(table=E2M1, rows=-1) == ERR_TABLE                   # this twin looks at the table first
        assert call(scales=None, cols=100) == ERR_ARG                   # ... then at the row scales, then at cols


# --------------------------------------------------------------------------------------------------------------- Python
def _tensors(b=2, l=3, c=256, dtype=torch.float16):
    return (torch.zeros(b, l, c, dtype=torch.float16), torch.zeros(b, 1, c, dtype=torch.float16), torch.zeros(b, l, c, dtype=dtype),
            torch.zeros(b, 1, c, dtype=torch.float16), torch.zeros(b, 1, c, dtype=torch.float16))


def test_python_wrappers_refuse_before_the_library(lib, monkeypatch):
    from fpqvar_amd import rotation as rot
    fns = {"resid_adaln_rotate_quant": rot.resid_adaln_rotate_quant, "resid_adaln_rotate_quant_mx": rot.resid_adaln_rotate_quant_mx,
           "resid_adaln_rotate_quant_token": rot.resid_adaln_rotate_quant_token}
    y, g, x, sc, sh = _tensors()
    for name, fn in fns.items():
        with pytest.raises(RuntimeError, match=name + ".*GPU"):
            fn(y, g, x, sc, sh)
    monkeypatch.setattr(rot, "require_gpu", lambda *a, **k: None)
    touched = []
    monkeypatch.setattr(rot, "lib", lambda: touched.append("lib"))
    monkeypatch.setattr(rot, "_native", None)
    for name, fn in fns.items():
        with pytest.raises(RuntimeError, match=name + ": y and gate must be float16"):
            fn(y.float(), g, x, sc, sh)
        with pytest.raises(RuntimeError, match=name + ": y and gate must be float16"):
            fn(y, g.float(), x, sc, sh)
        with pytest.raises(RuntimeError, match=name + ": residual must be float16 or float32"):
            fn(y, g, x.double(), sc, sh)
        with pytest.raises(RuntimeError, match=name + r": residual must be \[B, L, C\]"):
            fn(y.view(6, 256), g, x.view(6, 256), sc, sh)
        with pytest.raises(RuntimeError, match=name + ": y .* must have the shape of residual"):
            fn(y[:, :2], g, x, sc, sh)
        with pytest.raises(RuntimeError, match=name + ": gate .* must be"):
            fn(y, g[:1], x, sc, sh)
        with pytest.raises(RuntimeError, match=name + ": gate .* must be"):
            fn(y, torch.zeros(2, 3, 256, dtype=torch.float16), x, sc, sh)
        with pytest.raises(RuntimeError, match=name + ": scale and shift must both be float16 or both float32"):
            fn(y, g, x, sc, sh.float())
        with pytest.raises(RuntimeError, match=name + ": scale and shift must be"):
            fn(y, g, x, sc[:1], sh[:1])
        with pytest.raises(RuntimeError, match=name + ": C must be a multiple of 128 and at most 2560"):
            fn(*_tensors(1, 2, 2688))
        with pytest.raises(RuntimeError, match=name + ": C must be a multiple of 128 and at most 2560"):
            fn(*_tensors(1, 2, 192))
        with pytest.raises(RuntimeError, match=name + ": inplace=True needs a contiguous residual"):
            fn(y, g, x.transpose(0, 1).contiguous().transpose(0, 1), sc, sh, inplace=True)
        with pytest.raises(RuntimeError, match=name + ": inplace=True writes x_new over residual, which must not overlap y"):
            fn(y, g, y, sc, sh, inplace=True)
        with pytest.raises(RuntimeError, match=name + ": inplace=True writes x_new over residual, which must not overlap y"):
            fn(y.view(-1)[: 3 * 256].view(1, 3, 256), g[:1], y.view(-1)[256: 4 * 256].view(1, 3, 256), sc[:1], sh[:1], inplace=True)
    with pytest.raises(RuntimeError, match="resid_adaln_rotate_quant_token: emit must be 'values' or 'fp6'"):
        rot.resid_adaln_rotate_quant_token(y, g, x, sc, sh, emit="fp8")
    with pytest.raises(RuntimeError, match="resid_adaln_rotate_quant_token: emit='fp6' writes E2M3 or E3M2 codes"):
        rot.resid_adaln_rotate_quant_token(y, g, x, sc, sh, table="e2m1", emit="fp6")
    with pytest.raises(RuntimeError, match="resid_adaln_rotate_quant_token: kmajor is a layout"):
        rot.resid_adaln_rotate_quant_token(y, g, x, sc, sh, kmajor=True)
    assert not touched, "a refused call reached the library"


class _Recorder:
    """stands in for the loaded library: every entry point records its name and reports success"""
    def __init__(self):
        self.calls = []

    def __getattr__(self, name):
        return lambda *a: self.calls.append((name, a)) or 0


@pytest.mark.parametrize("dtype", (torch.float16, torch.float32))
def test_what_the_wrappers_hand_over_and_return(monkeypatch, dtype):
    """(x_new, *what the twin returns); x_new has the residual's dtype and, in place, is the residual; the entry point and its leading
    four pointers"""
    from fpqvar_amd import rotation as rot
    rec = _Recorder()
    monkeypatch.setattr(rot, "require_gpu", lambda *a, **k: None)
    monkeypatch.setattr(rot, "lib", lambda: rec)
    monkeypatch.setattr(rot, "_native", None)
    monkeypatch.setattr(rot, "device_guard", lambda dev: contextlib.nullcontext())
    monkeypatch.setattr(rot, "stream_ptr", lambda dev: None)
    y, g, x, sc, sh = _tensors(dtype=dtype)
    cases = [
        (lambda **k: rot.resid_adaln_rotate_quant(y, g, x, sc, sh, **k), "fpq_resid_adaln_rotate_quant_rows", [(2, 3, 256)]),
        (lambda **k: rot.resid_adaln_rotate_quant(y, g, x, sc, sh, return_intermediates=True, **k), "fpq_resid_adaln_rotate_quant_rows",
         [(2, 3, 256)] * 3),
        (lambda **k: rot.resid_adaln_rotate_quant_mx(y, g, x, sc, sh, **k), "fpq_resid_adaln_rotate_quant_rows_codes_mx", [(6, 128), (6, 2)]),
        (lambda **k: rot.resid_adaln_rotate_quant_token(y, g, x, sc, sh, **k), "fpq_resid_adaln_rotate_quant_token_rows", [(2, 3, 256)]),
        (lambda **k: rot.resid_adaln_rotate_quant_token(y, g, x, sc, sh, emit="fp6", **k), "fpq_resid_adaln_rotate_quant_token_rows_codes_f6",
         [(6, 192), (6,)]),
        (lambda **k: rot.resid_adaln_rotate_quant_token(y, g, x, sc, sh, table="e3m2", emit="fp6", kmajor=True, **k),
         "fpq_resid_adaln_rotate_quant_token_rows_codes_f6", [(2, 6, 96), (6,)]),
    ]
    for fn, entry, shapes in cases:
        for inplace in (False, True):
            rec.calls.clear()
            got = fn(inplace=inplace)
            assert isinstance(got, tuple) and len(got) == 1 + len(shapes), entry
            x_new = got[0]
            assert x_new.dtype is dtype and x_new.shape == x.shape and (x_new is x) == inplace, entry
            assert [tuple(t.shape) for t in got[1:]] == shapes, entry
            (name, args), = rec.calls
            assert name == entry
            assert args[:4] == (y.data_ptr(), g.data_ptr(), x_new.data_ptr(), x.data_ptr()), entry
