"""The four per-token entry points of the full-width producers (include/fpq.h: fpq_fullrot_quant_token_rows[_codes_f6],
fpq_fullrot_adaln_quant_token_rows[_codes_f6]) without a GPU, in the manner of tests/test_fullrot_abi_host.py: every call is refused
or has no rows, so nothing is launched and the fake pointers are never read.  Which code a refused call returns, which fault of two
is reported, the ctypes signatures, and - through a recording stub in place of the library - what rotation.rotate_quant_full_token /
adaln_rotate_quant_full_token hand to the C ABI."""
import ctypes

import pytest
import torch

OK, ARG, DTYPE, SHAPE, TABLE = 0, -1, -2, -3, -4
F16, F32, F64 = 0, 1, 2
E2M1, E1M2, E3M0, E2M3, E3M2, E1M2_NEG = range(6)
PTR = 0x7000_0000_1000
WORDS = (ctypes.c_uint32 * 72)(*range(72))
BUILT = (1920, 2304)
NAMES = ("fpq_fullrot_quant_token_rows", "fpq_fullrot_quant_token_rows_codes_f6", "fpq_fullrot_adaln_quant_token_rows",
         "fpq_fullrot_adaln_quant_token_rows_codes_f6")


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as g
    g.build_hip()
    from fpqvar_amd import _lib
    return _lib.lib()


def values(lib, x=PTR, out=PTR, rot=None, rs=None, rows=4, cols=1920, dt=F16, smooth=None, sign=WORDS, table=E2M3):
    return lib.fpq_fullrot_quant_token_rows(x, out, rot, rs, rows, cols, dt, smooth, sign, table, None)


def codes(lib, x=PTR, out=PTR, rs=PTR, rows=4, cols=1920, dt=F16, smooth=None, sign=WORDS, table=E2M3, km=0):
    return lib.fpq_fullrot_quant_token_rows_codes_f6(x, out, rs, rows, cols, dt, smooth, sign, table, km, None)


def a_values(lib, x=PTR, out=PTR, h=None, rot=None, rs=None, rows=4, cols=1920, dt=F16, scale=PTR, shift=PTR, mdt=F16, rpb=2, eps=1e-6,
             smooth=None, sign=WORDS, table=E2M3):
    return lib.fpq_fullrot_adaln_quant_token_rows(x, out, h, rot, rs, rows, cols, dt, scale, shift, mdt, rpb, eps, smooth, sign, table, None)


def a_codes(lib, x=PTR, out=PTR, rs=PTR, rows=4, cols=1920, dt=F16, scale=PTR, shift=PTR, mdt=F16, rpb=2, eps=1e-6, smooth=None, sign=WORDS,
            table=E2M3, km=0):
    return lib.fpq_fullrot_adaln_quant_token_rows_codes_f6(x, out, rs, rows, cols, dt, scale, shift, mdt, rpb, eps, smooth, sign, table, km, None)


ALL = (values, codes, a_values, a_codes)


def test_names_and_signatures():
    """the argument orders mirror the per-group twins and the 128-block token forms (include/fpq.h)"""
    from fpqvar_amd import _lib
    c = ctypes
    plain = [c.c_int64, c.c_int64, c.c_int, c.c_void_p, c.POINTER(c.c_uint32)]
    adaln = [c.c_int64, c.c_int64, c.c_int, c.c_void_p, c.c_void_p, c.c_int, c.c_int64, c.c_float, c.c_void_p, c.POINTER(c.c_uint32)]
    assert _lib._SIGS[NAMES[0]] == (c.c_int, [c.c_void_p] * 4 + plain + [c.c_int, c.c_void_p])
    assert _lib._SIGS[NAMES[1]] == (c.c_int, [c.c_void_p] * 3 + plain + [c.c_int, c.c_int, c.c_void_p])
    assert _lib._SIGS[NAMES[2]] == (c.c_int, [c.c_void_p] * 5 + adaln + [c.c_int, c.c_void_p])
    assert _lib._SIGS[NAMES[3]] == (c.c_int, [c.c_void_p] * 3 + adaln + [c.c_int, c.c_int, c.c_void_p])
    assert _lib._SIGS[NAMES[2]] == _lib._SIGS["fpq_adaln_rotate_quant_token_rows"]                # the 128-block token forms' lists
    assert _lib._SIGS[NAMES[3]] == _lib._SIGS["fpq_adaln_rotate_quant_token_rows_codes_f6"]
    twin = _lib._SIGS["fpq_fullrot_quant_rows"][1]                                                  # the per-group twin + row_scales
    assert _lib._SIGS[NAMES[0]][1] == twin[:3] + [c.c_void_p] + twin[3:]


def test_the_library_exports_all_four(lib):
    for name in NAMES:
        assert hasattr(lib, name)
    assert lib.fpq_version() >= 100


def test_single_refusals(lib):
    for call in ALL:
        assert call(lib, rows=-1) == ARG
        assert call(lib, cols=-1) == ARG
        assert call(lib, sign=None) == ARG
        for t in (E2M1, E1M2, E3M0, E1M2_NEG, 9, 10, -1, 99):        # the symmetric FP6 tables only
            assert call(lib, table=t) == TABLE, t
        assert call(lib, dt=F64) == DTYPE
        assert call(lib, dt=7) == DTYPE
        for cols in (0, 128, 2048, 1984, 1280, 1536, 1024, 4096, 1920 + 32, 2304 * 2):
            assert call(lib, cols=cols) == SHAPE, cols
        assert call(lib, x=None) == ARG
        assert call(lib, out=None) == ARG
        assert call(lib, x=PTR + 8) == ARG
        assert call(lib, out=PTR + 4) == ARG
        assert call(lib, smooth=PTR + 8) == ARG
        assert call(lib, rs=PTR + 2) == ARG
    for call in (values, codes):
        assert call(lib, rows=1 << 31) == SHAPE
    for call in (a_values, a_codes):
        assert call(lib, rows=1 << 31, rpb=1) == SHAPE
        assert call(lib, rpb=0) == ARG
        assert call(lib, rpb=-3) == ARG
        assert call(lib, rows=4, rpb=3) == ARG                        # rows not a multiple of rows_per_batch
        assert call(lib, rows=4, rpb=8) == ARG
        assert call(lib, mdt=F64) == DTYPE
        assert call(lib, mdt=-1) == DTYPE
        assert call(lib, scale=None) == ARG
        assert call(lib, shift=None) == ARG
        assert call(lib, scale=PTR + 8) == ARG
        assert call(lib, shift=PTR + 2) == ARG
    assert values(lib, rot=PTR + 2) == ARG
    assert a_values(lib, rot=PTR + 2) == ARG
    assert a_values(lib, h=PTR + 2) == ARG
    assert codes(lib, rs=None) == ARG                                 # row_scales is required on the code forms
    assert a_codes(lib, rs=None) == ARG
    big = (1 << 31) // 1440 + 1                                       # a k-major image of 2 GiB or more (1920 * 3 / 4 bytes per row)
    assert codes(lib, km=1, rows=big) == SHAPE
    assert a_codes(lib, km=1, rows=big, rpb=1) == SHAPE
    assert codes(lib, km=1, rows=(1 << 31) // 1728 + 1, cols=2304) == SHAPE


def test_nothing_to_do(lib):
    for cols in BUILT:
        for dt in (F16, F32):
            for table in (E2M3, E3M2):
                assert values(lib, rows=0, cols=cols, dt=dt, table=table, x=None, out=None) == OK
                assert codes(lib, rows=0, cols=cols, dt=dt, table=table, x=None, out=None, rs=None) == OK
                assert codes(lib, rows=0, cols=cols, dt=dt, table=table, x=None, out=None, rs=None, km=1) == OK
                for mdt in (F16, F32):
                    assert a_values(lib, rows=0, cols=cols, dt=dt, mdt=mdt, table=table, x=None, out=None, scale=None, shift=None) == OK
                    assert a_codes(lib, rows=0, cols=cols, dt=dt, mdt=mdt, table=table, x=None, out=None, rs=None, scale=None, shift=None, km=1) == OK


def test_order_of_two_faults(lib):
    """ARG (sizes, the sign words, rows_per_batch) < TABLE < DTYPE < SHAPE < rows == 0 < ARG (pointers), the order include/fpq.h
    documents; the code forms look at row_scales first (rows > 0, a built width)"""
    for call in ALL:
        assert call(lib, rows=-1, table=99) == ARG
        assert call(lib, sign=None, dt=F64) == ARG
        assert call(lib, table=99, dt=F64) == TABLE
        assert call(lib, table=E2M1, cols=128) == TABLE
        assert call(lib, dt=F64, cols=128) == DTYPE
        assert call(lib, cols=128, x=None) == SHAPE
        assert call(lib, cols=128, rows=0) == SHAPE                   # the width is checked before the empty call returns
        assert call(lib, rows=0, x=PTR + 8) == OK
    for call in (a_values, a_codes):
        assert call(lib, rpb=0, table=99) == ARG
        assert call(lib, rpb=3, mdt=F64) == ARG
        assert call(lib, rpb=3, cols=128) == ARG
        assert call(lib, table=99, mdt=F64) == TABLE
        assert call(lib, mdt=F64, cols=128) == DTYPE
        assert call(lib, cols=128, scale=None) == SHAPE
        assert call(lib, rows=0, scale=None, shift=PTR + 8) == OK
        assert call(lib, rows=0, rpb=0) == ARG
    for call in (codes, a_codes):
        assert call(lib, rs=None, table=99) == ARG
        assert call(lib, rs=None, dt=F64) == ARG
        assert call(lib, rs=None, cols=2048) == SHAPE                 # ... not at another width
        assert call(lib, rs=None, rows=0) == OK
        assert call(lib, km=1, rows=(1 << 31) // 1440 + 1, x=None, **({"rpb": 1} if call is a_codes else {})) == SHAPE


class _Recorder:
    def __init__(self):
        self.calls = []

    def __getattr__(self, name):
        def f(*args):
            self.calls.append((name, args))
            return 0
        return f


@pytest.fixture()
def recorded(monkeypatch):
    """rotation._produce with the library, the GPU check and the stream lookup replaced: CPU tensors reach the ctypes call"""
    import contextlib
    from fpqvar_amd import rotation
    rec = _Recorder()
    monkeypatch.setattr(rotation, "lib", lambda: rec)
    monkeypatch.setattr(rotation, "require_gpu", lambda *a, **k: None)
    monkeypatch.setattr(rotation, "stream_ptr", lambda dev: None)
    monkeypatch.setattr(rotation, "device_guard", lambda dev: contextlib.nullcontext())
    return rec


@pytest.mark.parametrize("C", BUILT)
def test_python_hands_over_the_documented_arguments(recorded, C):
    from fpqvar_amd import rotation
    B, L = 2, 3
    x = torch.zeros(B, L, C, dtype=torch.float32)
    sc, sh = torch.zeros(B, 1, C, dtype=torch.float16), torch.ones(B, 1, C, dtype=torch.float16)
    words = rotation.full_sign_words(rotation.sign_vector(C, 42))
    # the plain form
    out, rot = rotation.rotate_quant_full_token(x, "e3m2", return_rotated=True)
    name, a = recorded.calls[-1]
    assert name == NAMES[0] and len(a) == 11
    assert a[0] == x.data_ptr() and a[1:4] == (out.data_ptr(), rot.data_ptr(), None) and a[4:7] == (B * L, C, F32) and a[7] is None
    assert tuple(a[8]) == words and a[9] == E3M2
    res = rotation.rotate_quant_full_token(x.half())
    name, a = recorded.calls[-1]
    assert isinstance(res, torch.Tensor) and res.shape == x.shape and a[1:4] == (res.data_ptr(), None, None) and a[6] == F16 and a[9] == E2M3
    d, sm = -torch.ones(C, dtype=torch.float64), torch.ones(C)
    for emit, table, tid in (("fp6", "e2m3", E2M3), ("bf6", "e3m2", E3M2)):
        for km in (False, True):
            cd, scl = rotation.rotate_quant_full_token(x, table, d=d, smooth=sm, emit=emit, kmajor=km)
            name, a = recorded.calls[-1]
            assert name == NAMES[1] and len(a) == 11
            assert a[0] == x.data_ptr() and a[1:3] == (cd.data_ptr(), scl.data_ptr()) and a[3:6] == (B * L, C, F32) and a[6] == sm.data_ptr()
            assert tuple(a[7]) == (0xFFFFFFFF,) * (C // 32) and a[8] == tid and a[9] == (1 if km else 0) and isinstance(a[9], int)
            assert tuple(cd.shape) == ((C // 128, B * L, 96) if km else (B * L, C * 3 // 4)) and cd.dtype is torch.uint8
            assert tuple(scl.shape) == (B * L,) and scl.dtype is torch.float16
    # behind the adaLN front
    out, h, rot = rotation.adaln_rotate_quant_full_token(x, sc, sh, "e2m3", eps=1e-5, return_intermediates=True)
    name, a = recorded.calls[-1]
    assert name == NAMES[2] and len(a) == 17
    assert a[0] == x.data_ptr() and a[1:5] == (out.data_ptr(), h.data_ptr(), rot.data_ptr(), None) and a[5:8] == (B * L, C, F32)
    assert a[8:12] == (sc.data_ptr(), sh.data_ptr(), F16, L) and a[12] == pytest.approx(1e-5) and a[13] is None
    assert tuple(a[14]) == words and a[15] == E2M3
    res = rotation.adaln_rotate_quant_full_token(x.half(), sc.float(), sh.float(), "e3m2")
    name, a = recorded.calls[-1]
    assert isinstance(res, torch.Tensor) and a[1:5] == (res.data_ptr(), None, None, None) and a[7] == F16 and a[10] == F32 and a[15] == E3M2
    for km in (False, True):
        cd, scl = rotation.adaln_rotate_quant_full_token(x, sc, sh, "e2m3", d=d, smooth=sm, emit="fp6", kmajor=km)
        name, a = recorded.calls[-1]
        assert name == NAMES[3] and len(a) == 16
        assert a[0] == x.data_ptr() and a[1:3] == (cd.data_ptr(), scl.data_ptr()) and a[3:6] == (B * L, C, F32)
        assert a[6:10] == (sc.data_ptr(), sh.data_ptr(), F16, L) and a[11] == sm.data_ptr()
        assert tuple(a[12]) == (0xFFFFFFFF,) * (C // 32) and a[13] == E2M3 and a[14] == (1 if km else 0)
        assert tuple(cd.shape) == ((C // 128, B * L, 96) if km else (B * L, C * 3 // 4)) and tuple(scl.shape) == (B * L,)


def test_python_refusals(recorded):
    from fpqvar_amd import rotation
    z = lambda *s, dt=torch.float16: torch.zeros(*s, dtype=dt)  # noqa: E731
    plain = lambda x, **kw: rotation.rotate_quant_full_token(x, **kw)  # noqa: E731
    adaln = lambda x, **kw: rotation.adaln_rotate_quant_full_token(x, z(2, 1, x.shape[-1]), z(2, 1, x.shape[-1]), **kw)  # noqa: E731
    for fn in (plain, adaln):
        for C in (2048, 1280, 4096):
            with pytest.raises(RuntimeError, match="widths"):
                fn(z(2, 3, C))
        with pytest.raises(RuntimeError, match="float16 or float32"):
            fn(z(2, 3, 1920, dt=torch.bfloat16))
        with pytest.raises(RuntimeError, match="unknown emit"):
            fn(z(2, 3, 1920), emit="fp8")
        with pytest.raises(RuntimeError, match="E2M3 operand format"):
            fn(z(2, 3, 1920), table="e3m2", emit="fp6")
        with pytest.raises(RuntimeError, match="E3M2 operand format"):
            fn(z(2, 3, 1920), table="e2m3", emit="bf6")
        with pytest.raises(RuntimeError, match="kmajor is a layout"):
            fn(z(2, 3, 1920), kmajor=True)
        with pytest.raises(RuntimeError, match="FP6 tables"):
            fn(z(2, 3, 1920), table="e2m1")
        with pytest.raises(RuntimeError, match="one sign per channel"):
            fn(z(2, 3, 1920), d=rotation.sign_vector(128, 42))
    with pytest.raises(RuntimeError, match="emit='values' only"):
        plain(z(2, 3, 1920), emit="fp6", return_rotated=True)
    with pytest.raises(RuntimeError, match="emit='values' only"):
        adaln(z(2, 3, 1920), emit="fp6", return_intermediates=True)
    with pytest.raises(RuntimeError, match="both be float16 or both float32"):
        rotation.adaln_rotate_quant_full_token(z(2, 3, 1920), z(2, 1, 1920), z(2, 1, 1920, dt=torch.float32))
    with pytest.raises(RuntimeError, match=r"\[B, L, C\]"):
        rotation.adaln_rotate_quant_full_token(z(6, 1920), z(2, 1, 1920), z(2, 1, 1920))
    assert not recorded.calls


def test_cpu_tensor_raises():
    from fpqvar_amd import rotation
    z = torch.zeros
    with pytest.raises(RuntimeError):
        rotation.rotate_quant_full_token(z(2, 1920))
    with pytest.raises(RuntimeError):
        rotation.adaln_rotate_quant_full_token(z(1, 2, 2304), z(1, 1, 2304).half(), z(1, 1, 2304).half())


def test_generation_batch_refuses_before_it_builds_anything():
    """GenerationBatch(rotation=...): the two refusals come before any tensor is made (no GPU here)"""
    from fpqvar_amd import var_block
    with pytest.raises(ValueError, match="fuse_residual"):
        var_block.GenerationBatch("d30-256", "w6a6", depth=1, batch_rows=2, device="cpu", rotation="full", fuse_residual=True)
    with pytest.raises(ValueError, match="'block' or 'full'"):
        var_block.GenerationBatch("d30-256", "w4a4", depth=1, batch_rows=2, device="cpu", rotation="dense")
    assert set(var_block.FULL_PRODUCERS) == set(var_block.ROWS)
