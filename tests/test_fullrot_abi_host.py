"""The full-width rotation's two entry points (include/fpq.h: fpq_fullrot_quant_rows, fpq_fullrot_quant_rows_codes_mx) without a
GPU, in the manner of tests/test_producer_abi_host.py: every call is refused or has no rows, so nothing is launched and the fake
pointers are never read.  Which code a refused call returns, which fault of two is reported, the ctypes signatures, and - through
a recording stub in place of the library - what rotation.rotate_quant_full* hand to the C ABI."""
import ctypes

import pytest
import torch

OK, ARG, DTYPE, SHAPE, TABLE = 0, -1, -2, -3, -4
F16, F32, F64 = 0, 1, 2
E2M1, E1M2, E3M0, E2M3, E3M2, E1M2_NEG = range(6)
PTR = 0x7000_0000_1000
WORDS = (ctypes.c_uint32 * 72)(*range(72))
BUILT = (1920, 2304)


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as g
    g.build_hip()
    from fpqvar_amd import _lib
    return _lib.lib()


def values(lib, x=PTR, out=PTR, rot=None, rows=4, cols=1920, dt=F16, smooth=None, sign=WORDS, table=E2M1):
    return lib.fpq_fullrot_quant_rows(x, out, rot, rows, cols, dt, smooth, sign, table, None)


def codes(lib, x=PTR, out=PTR, scales=PTR, rows=4, cols=1920, dt=F16, smooth=None, sign=WORDS, km=0):
    return lib.fpq_fullrot_quant_rows_codes_mx(x, out, scales, rows, cols, dt, smooth, sign, km, None)


def test_names_and_signatures():
    from fpqvar_amd import _lib
    c = ctypes
    want = (c.c_int, [c.c_void_p, c.c_void_p, c.c_void_p, c.c_int64, c.c_int64, c.c_int, c.c_void_p, c.POINTER(c.c_uint32), c.c_int, c.c_void_p])
    for name in ("fpq_fullrot_quant_rows", "fpq_fullrot_quant_rows_codes_mx"):
        assert _lib._SIGS[name] == want
        assert not name.startswith(("fpq_rotate_", "fpq_quant_", "fpq_adaln_"))


def test_single_refusals(lib):
    for call in (values, codes):
        assert call(lib, rows=-1) == ARG
        assert call(lib, cols=-1) == ARG
        assert call(lib, sign=None) == ARG
        assert call(lib, dt=F64) == DTYPE
        assert call(lib, dt=7) == DTYPE
        for cols in (0, 128, 2048, 1984, 1280, 1536, 1024, 4096, 1920 + 32, 2304 * 2):
            assert call(lib, cols=cols) == SHAPE, cols
        assert call(lib, rows=1 << 31) == SHAPE
        assert call(lib, x=None) == ARG
        assert call(lib, out=None) == ARG
        assert call(lib, x=PTR + 8) == ARG
        assert call(lib, out=PTR + 4) == ARG
        assert call(lib, smooth=PTR + 8) == ARG
    assert values(lib, rot=PTR + 2) == ARG
    for t in (E1M2_NEG, 9, 10, -1, 99):
        assert values(lib, table=t) == TABLE, t
    assert codes(lib, scales=None) == ARG
    assert codes(lib, scales=PTR + 8) == ARG
    assert codes(lib, km=1, rows=(1 << 31) // 960 + 1, cols=1920) == SHAPE  # a k-major image of 2 GiB or more


def test_nothing_to_do(lib):
    for cols in BUILT:
        for dt in (F16, F32):
            assert values(lib, rows=0, cols=cols, dt=dt, x=None, out=None) == OK
            assert codes(lib, rows=0, cols=cols, dt=dt, x=None, out=None, scales=None) == OK
            assert codes(lib, rows=0, cols=cols, dt=dt, x=None, out=None, scales=None, km=1) == OK
    for t in (E2M1, E1M2, E3M0, E2M3, E3M2):
        assert values(lib, rows=0, table=t) == OK


def test_order_of_two_faults(lib):
    """ARG (sizes, the sign words) < TABLE < DTYPE < SHAPE < rows == 0 < ARG (pointers), as fpq_rotate_quant_rows"""
    assert values(lib, rows=-1, table=99) == ARG
    assert values(lib, sign=None, dt=F64) == ARG
    assert values(lib, table=99, dt=F64) == TABLE
    assert values(lib, table=99, cols=128) == TABLE
    assert values(lib, dt=F64, cols=128) == DTYPE
    assert values(lib, cols=128, x=None) == SHAPE
    assert values(lib, cols=128, rows=0) == SHAPE                 # the width is checked before the empty call returns
    assert values(lib, rows=0, x=PTR + 8) == OK
    assert codes(lib, rows=-1, dt=F64) == ARG
    assert codes(lib, dt=F64, cols=2048) == DTYPE
    assert codes(lib, cols=2048, x=None) == SHAPE
    assert codes(lib, scales=None, dt=F64) == ARG                 # the codes form looks at its scales first (rows > 0, a built width)
    assert codes(lib, scales=None, cols=2048) == SHAPE            # ... not at another width
    assert codes(lib, scales=None, rows=0) == OK


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
def test_python_passes_the_long_sign_vector(recorded, C):
    from fpqvar_amd import rotation
    x = torch.zeros(3, C, dtype=torch.float16)
    out, rot = rotation.rotate_quant_full(x, "e3m0", return_rotated=True)
    name, a = recorded.calls[-1]
    assert name == "fpq_fullrot_quant_rows" and len(a) == 10
    assert a[0] == x.data_ptr() and a[1] == out.data_ptr() and a[2] == rot.data_ptr() and a[3:6] == (3, C, F16) and a[6] is None
    assert len(a[7]) == C // 32 and tuple(a[7]) == rotation.full_sign_words(rotation.sign_vector(C, 42)) and a[8] == E3M0
    assert tuple(a[7]) != rotation.sign_mask(rotation.sign_vector(128, 42)) * (C // 128)   # not the block form's vector tiled
    rotation.rotate_quant_full(x.float())
    name, a = recorded.calls[-1]
    assert a[2] is None and a[5] == F32 and a[8] == E2M1
    d = -torch.ones(C, dtype=torch.float64)
    sm = torch.ones(C)
    for km in (False, True):
        cd, sc = rotation.rotate_quant_full_mx(x, d=d, smooth=sm, kmajor=km)
        name, a = recorded.calls[-1]
        assert name == "fpq_fullrot_quant_rows_codes_mx" and len(a) == 10
        assert a[1] == cd.data_ptr() and a[2] == sc.data_ptr() and a[6] == sm.data_ptr() and a[8] == (1 if km else 0)
        assert tuple(a[7]) == (0xFFFFFFFF,) * (C // 32)
        assert tuple(cd.shape) == ((C // 128, 3, 64) if km else (3, C // 2))
        assert tuple(sc.shape) == ((C // 128, 4) if km else (3, C // 128)) and sc.dtype is (torch.float32 if km else torch.float16)


def test_python_refusals(recorded):
    from fpqvar_amd import rotation
    with pytest.raises(RuntimeError, match="widths"):
        rotation.rotate_quant_full(torch.zeros(2, 2048, dtype=torch.float16))
    with pytest.raises(RuntimeError, match="float16 or float32"):
        rotation.rotate_quant_full_mx(torch.zeros(2, 1920, dtype=torch.bfloat16))
    with pytest.raises(RuntimeError, match="one sign per channel"):
        rotation.rotate_quant_full(torch.zeros(2, 1920, dtype=torch.float16), d=rotation.sign_vector(128, 42))
    assert not recorded.calls


def test_cpu_tensor_raises():
    from fpqvar_amd import rotation
    with pytest.raises(RuntimeError):
        rotation.rotate_quant_full(torch.zeros(2, 1920, dtype=torch.float16))
    with pytest.raises(RuntimeError):
        rotation.rotate_quant_full_mx(torch.zeros(2, 2304, dtype=torch.float16))


def test_linear_rotate_operands_full_width(monkeypatch):
    from fpqvar_amd import gemm, rotation
    seen = {}

    def fake(x, d=None, smooth=None, kmajor=False):
        seen.update(d=d, smooth=smooth, kmajor=kmajor)
        return "codes", "scales"
    monkeypatch.setattr(rotation, "rotate_quant_full_mx", fake)
    lin = gemm.FP4Linear.__new__(gemm.FP4Linear)
    torch.nn.Module.__init__(lin)
    lin.act_table, lin.w_codes = "e2m1", torch.zeros(1, 1, 64, dtype=torch.uint8)       # a k-major weight image
    assert lin.rotate_operands(torch.zeros(1, 1920), full_width=True) == ("codes", "scales") and seen["kmajor"] is True
    lin.act_table = "e3m0"
    with pytest.raises(NotImplementedError, match="full-width"):
        lin.rotate_operands(torch.zeros(1, 1920), full_width=True)
