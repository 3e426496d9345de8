"""GPU: fpq_sqerr_rows_weighted against the float64 reference within the derived bound (tests/sqerr_model.py), its determinism,
its non-finite rule plane by plane, its refusals on real device pointers, and both front ends (ctypes and the compiled binding)."""
import functools

import pytest
import torch

from tests import sqerr_model as sm

pytestmark = pytest.mark.gpu

F16, F32 = torch.float16, torch.float32
# one vector; a partly filled workgroup; several workgroups; a wide matrix; a mid-sized one; the grid at its cap with three
# planes (a lane iterates 3 / 5 times); more rows than lanes in the grid, one or two vectors per row
SHAPES = ((1, 8), (3, 136), (65, 1024), (110, 5760), (1000, 1920), (13600, 640), (70001, 8))
ARG, DTYPE, SHAPE = -1, -2, -3


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


def _planes(rows, cols):
    return 3 if (rows, cols) == (13600, 640) else 4


@functools.lru_cache(maxsize=None)
def _case(family, rows, cols, dtype, planes):
    ref, y, w = sm.make_case(family, rows, cols, dtype, planes)
    return ref, y, w, sm.reference(ref, y, w)


def _worst(got, want, rows, cols, dtype, w):
    rel, floor = sm.bound(rows, cols, dtype, float(w.max()))
    return max(sm.ratio(float(got[p]), float(want[p]), rel, floor) for p in range(got.numel()))


@pytest.mark.parametrize("dtype", (F16, F32), ids=("f16", "f32"))
@pytest.mark.parametrize("rows,cols", SHAPES, ids=lambda v: str(v))
def test_kernel_within_bound_and_out_view(dev, rows, cols, dtype):
    from fpqvar_amd import ops
    planes = _planes(rows, cols)
    ref, y, w, want = _case("gauss", rows, cols, dtype, planes)
    dref, dy, dw = ref.to(dev), y.to(dev), w.to(dev)
    for P in ((planes,) if planes == 3 else (1, 2, 3, 4)):
        got = ops.sqerr_rows_weighted(dref, dy[:P], dw)
        assert got.shape == (P,) and got.dtype == torch.float32
        worst = _worst(got.cpu(), want[:P], rows, cols, dtype, w)
        print(f"[{rows} x {cols}] {dtype} P={P}: worst err / bound {worst:.3g}")
        assert worst <= 1.0, (P, got.cpu().tolist(), want[:P].tolist())
        # into a view at a non-zero offset of a larger tensor: the same bits, the neighbours untouched
        table = torch.full((3, 6), -7.0, dtype=torch.float32, device=dev)
        ret = ops.sqerr_rows_weighted(dref, dy[:P], dw, out=table[1, 1:1 + P])
        assert ret.data_ptr() == table[1, 1:].data_ptr()
        host = table.cpu()
        assert torch.equal(host[1, 1:1 + P].view(torch.int32), got.cpu().view(torch.int32))
        host[1, 1:1 + P] = -7.0
        assert bool((host == -7.0).all()), "elements beside the out view were written"
    one = ops.sqerr_rows_weighted(dref, dy[0], dw)                    # y as [rows, cols]: one plane
    assert torch.equal(one.cpu().view(torch.int32), ops.sqerr_rows_weighted(dref, dy[:1], dw).cpu().view(torch.int32))


@pytest.mark.parametrize("dtype", (F16, F32), ids=("f16", "f32"))
def test_finite_families_and_the_emulated_order(dev, dtype):
    """Every finite family within the bound, y == ref exactly 0, and - the order of operations being fixed - the very bits of the
    CPU emulation the bound was derived from, at shapes with one, several and capped workgroups."""
    from fpqvar_amd import ops
    for rows, cols in ((3, 136), (65, 1024)):
        for family in sm.FINITE_FAMILIES:
            ref, y, w, want = _case(family, rows, cols, dtype, 3)
            got = ops.sqerr_rows_weighted(ref.to(dev), y.to(dev), w.to(dev)).cpu()
            worst = _worst(got, want, rows, cols, dtype, w)
            print(f"[{rows} x {cols}] {dtype} {family}: worst err / bound {worst:.3g}")
            assert worst <= 1.0, (family, got.tolist(), want.tolist())
            if family == "equal":
                assert not bool(got.any())
            assert torch.equal(got.view(torch.int32), sm.emulate(ref, y, w).view(torch.int32)), (family, rows, cols)
    ref, y, w, _ = _case("gauss", 13600, 640, dtype, 3)
    got = ops.sqerr_rows_weighted(ref.to(dev), y.to(dev), w.to(dev)).cpu()
    assert torch.equal(got.view(torch.int32), sm.emulate(ref, y, w).view(torch.int32)), "grid at its cap"


def _raw(lib, ref, y, w, out, ws, rows, cols, planes, dtype_id):
    from fpqvar_amd import _lib
    return lib.fpq_sqerr_rows_weighted(ref, y, w, out, ws, rows, cols, planes, dtype_id, _lib.stream_ptr(torch.device("cuda:0")))


def test_deterministic_whatever_the_workspace_held(dev):
    from fpqvar_amd import _lib, ops
    lib = _lib.lib()
    for rows, cols, dtype in ((1000, 1920, F16), (13600, 640, F32), (3, 136, F16)):
        ref, y, w, _ = _case("gauss", rows, cols, dtype, 3)
        dref, dy, dw = ref.to(dev), y.to(dev), w.to(dev)
        ws = torch.zeros(_lib.SQERR_WORKSPACE_BYTES, dtype=torch.uint8, device=dev)
        outs = []
        for fill in (None, None, 0xFF):
            if fill is not None:
                ws.fill_(fill)
            out = torch.empty(3, dtype=torch.float32, device=dev)
            assert _raw(lib, dref.data_ptr(), dy.data_ptr(), dw.data_ptr(), out.data_ptr(), ws.data_ptr(), rows, cols, 3, _lib.dtype_id(dtype)) == 0
            outs.append(out.cpu().view(torch.int32))
        assert torch.equal(outs[0], outs[1]) and torch.equal(outs[0], outs[2]), [o.tolist() for o in outs]
        assert torch.equal(outs[0], ops.sqerr_rows_weighted(dref, dy, dw).cpu().view(torch.int32)), "the wrapper's own workspace"


@pytest.mark.parametrize("dtype", (F16, F32), ids=("f16", "f32"))
def test_non_finite_rule_plane_by_plane(dev, dtype):
    from fpqvar_amd import ops
    rows, cols = 65, 1024
    for family in sm.NONFINITE_FAMILIES:
        ref, y, w, want = _case(family, rows, cols, dtype, 3)
        got = ops.sqerr_rows_weighted(ref.to(dev), y.to(dev), w.to(dev)).cpu()
        classes = [sm.class_of(float(v)) for v in got]
        assert classes == sm.expected_class(ref, y), (family, classes)
        rel, floor = sm.bound(rows, cols, dtype, float(w.max()))
        for p, c in enumerate(classes):
            if c == "finite":
                assert sm.ratio(float(got[p]), float(want[p]), rel, floor) <= 1.0, (family, p)
    assert [sm.class_of(float(v)) for v in ops.sqerr_rows_weighted(*[t.to(dev) for t in _case("nan_y", rows, cols, dtype, 3)[:3]]).cpu()] == \
        ["finite", "nan", "finite"]


def test_refusals_on_device_pointers_and_no_rows(dev):
    from fpqvar_amd import _lib, ops
    lib = _lib.lib()
    ref = torch.zeros(4, 16, dtype=F16, device=dev)
    ybuf = torch.zeros(2 * 4 * 16 + 8, dtype=F16, device=dev)
    w = torch.ones(4, dtype=torch.float32, device=dev)
    out = torch.full((4,), -7.0, dtype=torch.float32, device=dev)
    ws = torch.empty(_lib.SQERR_WORKSPACE_BYTES, dtype=torch.uint8, device=dev)
    args = lambda **kw: {**dict(ref=ref.data_ptr(), y=ybuf.data_ptr(), w=w.data_ptr(), out=out.data_ptr(), ws=ws.data_ptr(), rows=4, cols=16,
                                planes=2, dtype_id=0), **kw}
    assert _raw(lib, **args(y=ybuf[1:].data_ptr())) == ARG            # y two bytes past a 16-byte boundary
    assert _raw(lib, **args(cols=12)) == SHAPE                        # 12 fp16 columns: not whole 16-byte vectors
    assert _raw(lib, **args(planes=0)) == ARG and _raw(lib, **args(planes=5)) == ARG
    assert _raw(lib, **args(dtype_id=2)) == DTYPE
    torch.cuda.synchronize()
    assert bool((out.cpu() == -7.0).all()), "a refused call wrote its output"
    assert _raw(lib, **args(rows=0, planes=3)) == 0                   # no rows: `planes` zeros, nothing else
    assert out.cpu().tolist() == [0.0, 0.0, 0.0, -7.0]
    got = ops.sqerr_rows_weighted(torch.empty(0, 16, dtype=F16, device=dev), torch.empty(2, 0, 16, dtype=F16, device=dev),
                                  torch.empty(0, dtype=torch.float32, device=dev))
    assert got.cpu().tolist() == [0.0, 0.0]
    with pytest.raises(RuntimeError):
        ops.sqerr_rows_weighted(ref, ybuf[:64].view(4, 16).float(), w)                       # dtypes differ
    with pytest.raises(RuntimeError):
        ops.sqerr_rows_weighted(ref, ybuf[:128].view(2, 4, 16), w, out=out[:3])              # out: 3 elements for 2 planes
    with pytest.raises(RuntimeError, match="fpq error -1"):
        ops.sqerr_rows_weighted(ref, ybuf[:128].view(2, 4, 16), torch.ones(8, dtype=torch.float32, device=dev)[1:5])   # row_weight 4 bytes past alignment


def test_both_front_ends_agree(dev, monkeypatch):
    from fpqvar_amd import _native, ops
    ref, y, w, _ = _case("weights", 65, 1024, F16, 3)
    dref, dy, dw = ref.to(dev), y.to(dev), w.to(dev)
    assert ops._native is _native
    a = ops.sqerr_rows_weighted(dref, dy, dw)
    with monkeypatch.context() as m:
        m.setattr(ops, "_native", None)
        b = ops.sqerr_rows_weighted(dref, dy, dw)
        e = ops.sqerr_rows_weighted(torch.empty(0, 8, dtype=F32, device=dev), torch.empty(0, 8, dtype=F32, device=dev),
                                    torch.empty(0, dtype=torch.float32, device=dev))
    assert torch.equal(a.cpu().view(torch.int32), b.cpu().view(torch.int32)) and e.cpu().tolist() == [0.0]
