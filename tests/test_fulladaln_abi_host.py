"""The full-width adaLN producer's two entry points (include/fpq.h: fpq_fullrot_adaln_quant_rows, fpq_fullrot_adaln_quant_rows_codes_mx)
without a GPU, in the manner of tests/test_fullrot_abi_host.py: every call is refused or has no rows, so nothing is launched and the
fake pointers are never read.  Which code a refused call returns, which fault of two is reported, the ctypes signatures, and - through
a recording stub in place of the library - what rotation.adaln_rotate_quant_full* hand to the C ABI."""
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


def values(lib, x=PTR, out=PTR, h=None, rot=None, rows=4, cols=1920, dt=F16, scale=PTR, shift=PTR, mdt=F16, rpb=2, eps=1e-6, smooth=None,
           sign=WORDS, table=E2M1):
    return lib.fpq_fullrot_adaln_quant_rows(x, out, h, rot, rows, cols, dt, scale, shift, mdt, rpb, eps, smooth, sign, table, None)


def codes(lib, x=PTR, out=PTR, scales=PTR, rows=4, cols=1920, dt=F16, scale=PTR, shift=PTR, mdt=F16, rpb=2, eps=1e-6, smooth=None,
          sign=WORDS, km=0):
    return lib.fpq_fullrot_adaln_quant_rows_codes_mx(x, out, scales, rows, cols, dt, scale, shift, mdt, rpb, eps, smooth, sign, km, None)


def test_names_and_signatures():
    from fpqvar_amd import _lib
    c = ctypes
    tail = [c.c_int64, c.c_int64, c.c_int, c.c_void_p, c.c_void_p, c.c_int, c.c_int64, c.c_float, c.c_void_p, c.POINTER(c.c_uint32), c.c_int, c.c_void_p]
    assert _lib._SIGS["fpq_fullrot_adaln_quant_rows"] == (c.c_int, [c.c_void_p] * 4 + tail)
    assert _lib._SIGS["fpq_fullrot_adaln_quant_rows_codes_mx"] == (c.c_int, [c.c_void_p] * 3 + tail)
    # the values form: fpq_adaln_rotate_quant_rows' list; the codes form: fpq_fullrot_quant_rows_codes_mx's with the modulation block
    assert _lib._SIGS["fpq_fullrot_adaln_quant_rows"] == _lib._SIGS["fpq_adaln_rotate_quant_rows"]
    plain = _lib._SIGS["fpq_fullrot_quant_rows_codes_mx"][1]
    assert _lib._SIGS["fpq_fullrot_adaln_quant_rows_codes_mx"][1] == plain[:6] + tail[3:8] + plain[6:]


def test_the_library_exports_both(lib):
    for name in ("fpq_fullrot_adaln_quant_rows", "fpq_fullrot_adaln_quant_rows_codes_mx"):
        assert hasattr(lib, name)
    assert lib.fpq_version() >= 100


def test_single_refusals(lib):
    for call in (values, codes):
        assert call(lib, rows=-1) == ARG
        assert call(lib, cols=-1) == ARG
        assert call(lib, sign=None) == ARG
        assert call(lib, rpb=0) == ARG
        assert call(lib, rpb=-3) == ARG
        assert call(lib, rows=4, rpb=3) == ARG                    # rows not a multiple of rows_per_batch
        assert call(lib, rows=4, rpb=8) == ARG
        assert call(lib, dt=F64) == DTYPE
        assert call(lib, dt=7) == DTYPE
        assert call(lib, mdt=F64) == DTYPE
        assert call(lib, mdt=-1) == DTYPE
        for cols in (0, 128, 2048, 1984, 1280, 1536, 1024, 4096, 1920 + 32, 2304 * 2):
            assert call(lib, cols=cols) == SHAPE, cols
        assert call(lib, rows=1 << 31, rpb=1) == SHAPE
        assert call(lib, x=None) == ARG
        assert call(lib, out=None) == ARG
        assert call(lib, scale=None) == ARG
        assert call(lib, shift=None) == ARG
        assert call(lib, x=PTR + 8) == ARG
        assert call(lib, out=PTR + 4) == ARG
        assert call(lib, scale=PTR + 8) == ARG
        assert call(lib, shift=PTR + 2) == ARG
        assert call(lib, smooth=PTR + 8) == ARG
    assert values(lib, h=PTR + 2) == ARG
    assert values(lib, rot=PTR + 2) == ARG
    for t in (E1M2_NEG, 9, 10, -1, 99):
        assert values(lib, table=t) == TABLE, t
    assert codes(lib, scales=None) == ARG
    assert codes(lib, scales=PTR + 8) == ARG
    assert codes(lib, km=1, rows=(1 << 31) // 960 + 1, rpb=1, cols=1920) == SHAPE  # a k-major image of 2 GiB or more


def test_nothing_to_do(lib):
    for cols in BUILT:
        for dt in (F16, F32):
            for mdt in (F16, F32):
                assert values(lib, rows=0, cols=cols, dt=dt, mdt=mdt, x=None, out=None, scale=None, shift=None) == OK
                assert codes(lib, rows=0, cols=cols, dt=dt, mdt=mdt, x=None, out=None, scales=None, scale=None, shift=None) == OK
                assert codes(lib, rows=0, cols=cols, dt=dt, mdt=mdt, x=None, out=None, scales=None, scale=None, shift=None, km=1) == OK
    for t in (E2M1, E1M2, E3M0, E2M3, E3M2):
        assert values(lib, rows=0, table=t) == OK


def test_order_of_two_faults(lib):
    """ARG (sizes, the sign words, rows_per_batch) < TABLE < DTYPE (rows, modulation) < SHAPE < rows == 0 < ARG (pointers), the order
    include/fpq.h documents: fpq_fullrot_quant_rows' with fpq_adaln_rotate_quant_rows' additions"""
    assert values(lib, rows=-1, table=99) == ARG
    assert values(lib, sign=None, dt=F64) == ARG
    assert values(lib, rpb=0, table=99) == ARG
    assert values(lib, rpb=3, mdt=F64) == ARG
    assert values(lib, rpb=3, cols=128) == ARG
    assert values(lib, table=99, dt=F64) == TABLE
    assert values(lib, table=99, mdt=F64) == TABLE
    assert values(lib, table=99, cols=128) == TABLE
    assert values(lib, dt=F64, cols=128) == DTYPE
    assert values(lib, mdt=F64, cols=128) == DTYPE
    assert values(lib, cols=128, x=None) == SHAPE
    assert values(lib, cols=128, scale=None) == SHAPE
    assert values(lib, cols=128, rows=0) == SHAPE                 # the width is checked before the empty call returns
    assert values(lib, rows=0, x=PTR + 8) == OK
    assert values(lib, rows=0, scale=None, shift=PTR + 8) == OK
    assert values(lib, rows=0, rpb=0) == ARG                      # ... rows_per_batch too
    assert codes(lib, rows=-1, dt=F64) == ARG
    assert codes(lib, mdt=F64, cols=2048) == DTYPE
    assert codes(lib, cols=2048, shift=None) == SHAPE
    assert codes(lib, scales=None, mdt=F64) == ARG                # the codes form looks at its scales first (rows > 0, a built width)
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
def test_python_hands_over_the_documented_arguments(recorded, C):
    from fpqvar_amd import rotation
    B, L = 2, 3
    x = torch.zeros(B, L, C, dtype=torch.float32)
    sc, sh = torch.zeros(B, 1, C, dtype=torch.float16), torch.ones(B, 1, C, dtype=torch.float16)
    out, h, rot = rotation.adaln_rotate_quant_full(x, sc, sh, "e3m0", eps=1e-5, return_intermediates=True)
    name, a = recorded.calls[-1]
    assert name == "fpq_fullrot_adaln_quant_rows" and len(a) == 16
    assert a[0] == x.data_ptr() and a[1:4] == (out.data_ptr(), h.data_ptr(), rot.data_ptr()) and a[4:7] == (B * L, C, F32)
    assert a[7:11] == (sc.data_ptr(), sh.data_ptr(), F16, L) and a[11] == pytest.approx(1e-5) and a[12] is None
    assert len(a[13]) == C // 32 and tuple(a[13]) == rotation.full_sign_words(rotation.sign_vector(C, 42)) and a[14] == E3M0
    assert tuple(a[13]) != rotation.sign_mask(rotation.sign_vector(128, 42)) * (C // 128)   # not the block form's vector tiled
    assert out.shape == h.shape == rot.shape == x.shape and out.dtype == h.dtype == rot.dtype == torch.float16
    res = rotation.adaln_rotate_quant_full(x.half(), sc.float(), sh.float())
    name, a = recorded.calls[-1]
    assert isinstance(res, torch.Tensor) and a[1] == res.data_ptr() and a[2] is None and a[3] is None
    assert a[6] == F16 and a[9] == F32 and a[10] == L and a[11] == pytest.approx(1e-6) and a[14] == E2M1
    d = -torch.ones(C, dtype=torch.float64)
    sm = torch.ones(C)
    for km in (False, True):
        cd, scl = rotation.adaln_rotate_quant_full_mx(x, sc, sh, d=d, smooth=sm, kmajor=km)
        name, a = recorded.calls[-1]
        assert name == "fpq_fullrot_adaln_quant_rows_codes_mx" and len(a) == 15
        assert a[0] == x.data_ptr() and a[1] == cd.data_ptr() and a[2] == scl.data_ptr() and a[3:6] == (B * L, C, F32)
        assert a[6:10] == (sc.data_ptr(), sh.data_ptr(), F16, L) and a[11] == sm.data_ptr()
        assert tuple(a[12]) == (0xFFFFFFFF,) * (C // 32) and a[13] == (1 if km else 0) and isinstance(a[13], int)
        assert tuple(cd.shape) == ((C // 128, B * L, 64) if km else (B * L, C // 2))
        assert tuple(scl.shape) == ((C // 128, 8) if km else (B * L, C // 128)) and scl.dtype is (torch.float32 if km else torch.float16)


def test_python_refusals(recorded):
    from fpqvar_amd import rotation
    z = lambda *s, dt=torch.float16: torch.zeros(*s, dtype=dt)  # noqa: E731
    for fn in (rotation.adaln_rotate_quant_full, rotation.adaln_rotate_quant_full_mx):
        for C in (2048, 1280, 4096):
            with pytest.raises(RuntimeError, match="widths"):
                fn(z(2, 3, C), z(2, 1, C), z(2, 1, C))
        with pytest.raises(RuntimeError, match="both be float16 or both float32"):
            fn(z(2, 3, 1920), z(2, 1, 1920), z(2, 1, 1920, dt=torch.float32))
        with pytest.raises(RuntimeError, match="both be float16 or both float32"):
            fn(z(2, 3, 1920), z(2, 1, 1920, dt=torch.bfloat16), z(2, 1, 1920, dt=torch.bfloat16))
        with pytest.raises(RuntimeError, match="float16 or float32"):
            fn(z(2, 3, 1920, dt=torch.bfloat16), z(2, 1, 1920), z(2, 1, 1920))
        with pytest.raises(RuntimeError, match=r"\[B, L, C\]"):
            fn(z(6, 1920), z(2, 1, 1920), z(2, 1, 1920))
        with pytest.raises(RuntimeError, match="one sign per channel"):
            fn(z(2, 3, 1920), z(2, 1, 1920), z(2, 1, 1920), d=rotation.sign_vector(128, 42))
    assert not recorded.calls


def test_cpu_tensor_raises():
    from fpqvar_amd import rotation
    z = torch.zeros
    with pytest.raises(RuntimeError):
        rotation.adaln_rotate_quant_full(z(1, 2, 1920), z(1, 1, 1920).half(), z(1, 1, 1920).half())
    with pytest.raises(RuntimeError):
        rotation.adaln_rotate_quant_full_mx(z(1, 2, 2304), z(1, 1, 2304).half(), z(1, 1, 2304).half())


def _linear(cls, act_table):
    from fpqvar_amd import gemm
    lin = cls.__new__(cls)
    torch.nn.Module.__init__(lin)
    lin.act_table, lin.w_codes = act_table, torch.zeros(1, 1, 64, dtype=torch.uint8)       # a k-major weight image
    assert isinstance(lin, gemm.FP4Linear)
    return lin


def test_linear_adaln_operands_full_width(monkeypatch):
    from fpqvar_amd import gemm, rotation
    seen = {}

    def fake(x, scale, shift, d=None, smooth=None, eps=1e-6, kmajor=False):
        seen.update(d=d, smooth=smooth, eps=eps, kmajor=kmajor)
        return "codes", "scales"

    def block(*a, **k):
        raise AssertionError("the 128-block producer was called")
    monkeypatch.setattr(rotation, "adaln_rotate_quant_full_mx", fake)
    for other in ("adaln_rotate_quant_mx", "adaln_rotate_quant_g6", "adaln_rotate_quant_gf6", "resid_adaln_rotate_quant_mx"):
        monkeypatch.setattr(rotation, other, block)
    x, m = torch.zeros(1, 1, 1920), torch.zeros(1, 1, 1920)
    for cls in (gemm.FP4Linear, gemm.FP6GroupLinear):
        lin = _linear(cls, "e2m1")
        seen.clear()
        assert lin.adaln_operands(x, m, m, eps=1e-5, full_width=True) == ("codes", "scales")
        assert seen["kmajor"] is True and seen["eps"] == 1e-5
        with pytest.raises(NotImplementedError, match="pending"):
            lin.adaln_operands(x, m, m, pending=(x, m), full_width=True)
    for cls, table in ((gemm.FP4Linear, "e3m0"), (gemm.FP4Linear, "e1m2"), (gemm.FP6GroupLinear, "e2m3"), (gemm.FP6GroupLinear, "e3m2"),
                       (gemm.FP6GroupLinear, "e3m0")):
        with pytest.raises(NotImplementedError, match="full-width"):
            _linear(cls, table).adaln_operands(x, m, m, full_width=True)
