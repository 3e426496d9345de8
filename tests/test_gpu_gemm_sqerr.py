"""GPU: the squared-error forms of the four matrix-core GEMM families (gemm.linear_fp4_sqerr, linear_a6w4_sqerr, linear_w6_sqerr,
linear_fp6_sqerr; include/fpq.h, fpq_gemm_*_sqerr).  For every format pair a family serves, y16 comes from the family's existing
plain Linear, and the new call's loss is held to the float64 reference of (ref, y16, w) within the bound derived in
tests/gemm_sqerr_model.py - at the smallest shapes that reach every edge (one row; partly filled tiles in both directions; more
than one row tile; a full-width one), with fp16 and fp32 references, a bias, and every tiling forced through the existing switch.
The order of operations being fixed, the loss is also the very bits of the CPU emulation the bound was derived from."""
import functools
import math

import pytest
import torch

from tests import gemm_sqerr_model as gm

pytestmark = pytest.mark.gpu

F16, F32 = torch.float16, torch.float32
SHAPES = ((1, 8, 128), (37, 200, 384), (257, 136, 128), (100, 1920, 1920))        # (tokens, outs, K)
BIAS_SHAPE = (37, 200, 384)
PAIRS = ([("fp4", "e2m1", "e2m1")] + [("a6w4", a, "e2m1") for a in ("e1m2", "e3m0")] +
         [("w6", a, w) for a in ("e2m1", "e1m2", "e3m0") for w in ("e1m2", "e3m0")] +
         [("f6_rows", a, w) for a in ("e2m3", "e3m2") for w in ("e2m3", "e3m2")])
# the tilings a call can run, by the switch that forces them (None: the launch rule's own choice - the 64-row tile for the
# per-group families and the 128-row one for the row-scaled family at every shape here)
FORCED = {"fp4": (None, 20, 10, 40), "a6w4": (None, 20), "w6": (None, 20), "f6_rows": (None, 1)}
SWITCH = {"fp4": "FPQ_GEMM_CFG", "a6w4": "FPQ_GEMM_CFG", "w6": "FPQ_GEMM_CFG", "f6_rows": "FPQ_GEMM6_CFG"}


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


def _quantize(x, fmt):
    from fpqvar_amd import gemm
    if fmt == "e2m1":
        return gemm.quantize_mx(x)
    if fmt in ("e1m2", "e3m0"):
        return gemm.quantize_g6(x, fmt)
    return gemm.quantize_fp6(x, table=fmt)


@functools.lru_cache(maxsize=None)
def _operands(family, a_fmt, w_fmt, tokens, outs, k, with_bias):
    """(activation operand, weight operand, bias or None, y16 of the family's plain Linear) on the GPU, built once per case"""
    dev = torch.device("cuda:0")
    g = torch.Generator().manual_seed(1000 * tokens + outs + k)
    x = torch.randn(tokens, k, generator=g).half().to(dev)
    wt = (torch.randn(outs, k, generator=g) * 0.05).to(dev)
    bias = (torch.randn(outs, generator=g) * 0.3).half().to(dev) if with_bias else None
    a, w = _quantize(x, a_fmt), _quantize(wt, w_fmt)
    return a, w, bias, _plain(family, a_fmt, w_fmt, a, w, bias)


def _plain(family, a_fmt, w_fmt, a, w, bias):
    from fpqvar_amd import gemm
    if family == "fp4":
        return gemm.linear_fp4(*a, *w, bias)
    if family == "a6w4":
        return gemm.linear_a6w4(*a, a_fmt, *w, bias)
    if family == "w6":
        return gemm.linear_w6(*a, a_fmt, *w, w_fmt, bias)
    return gemm.linear_fp6(*a, *w, bias, a_table=a_fmt, w_table=w_fmt)


def _sqerr(family, a_fmt, w_fmt, a, w, bias, ref, rw, **kw):
    from fpqvar_amd import gemm
    if family == "fp4":
        return gemm.linear_fp4_sqerr(*a, *w, ref, rw, bias=bias, **kw)
    if family == "a6w4":
        return gemm.linear_a6w4_sqerr(*a, a_fmt, *w, ref, rw, bias=bias, **kw)
    if family == "w6":
        return gemm.linear_w6_sqerr(*a, a_fmt, *w, w_fmt, ref, rw, bias=bias, **kw)
    return gemm.linear_fp6_sqerr(*a, *w, ref, rw, bias=bias, a_table=a_fmt, w_table=w_fmt, **kw)


@functools.lru_cache(maxsize=None)
def _ref_and_weights(tokens, outs, dtype, y16_key):
    """ref = y16 + noise of 2 % of its size, in `dtype`, and the search's row weights - on the CPU, from the y16 stored under y16_key"""
    y16 = _Y16[y16_key]
    g = torch.Generator().manual_seed(31 * tokens + outs + (0 if dtype == F16 else 1))
    noise = torch.randn(tokens, outs, generator=g, dtype=torch.float64)
    ref = (y16.double() + 0.02 * float(y16.double().abs().mean()) * noise).to(dtype).contiguous()
    return ref, gm.sample_weights(tokens, outs, g)


_Y16 = {}


def _case(family, a_fmt, w_fmt, shape, dtype, with_bias=False):
    a, w, bias, y16 = _operands(family, a_fmt, w_fmt, *shape, with_bias)
    key = (family, a_fmt, w_fmt, shape, with_bias)
    if key not in _Y16:
        _Y16[key] = y16.cpu()
    ref, rw = _ref_and_weights(shape[0], shape[1], dtype, key)
    return a, w, bias, _Y16[key], ref, rw


@pytest.mark.parametrize("family,a_fmt,w_fmt", PAIRS, ids=[f"{f}-{a}x{w}" for f, a, w in PAIRS])
def test_loss_within_the_bound_at_every_edge_and_tiling(dev, family, a_fmt, w_fmt):
    from fpqvar_amd import _lib
    for shape in SHAPES:
        tokens, outs, _ = shape
        for dtype in (F16, F32):
            for with_bias in ((False, True) if shape == BIAS_SHAPE else (False,)):
                a, w, bias, y16, ref, rw = _case(family, a_fmt, w_fmt, shape, dtype, with_bias)
                want = gm.reference(ref, y16, rw)
                dref, drw = ref.to(dev), rw.to(dev)
                bits = {}
                for forced in FORCED[family]:
                    with _lib.option(SWITCH[family], forced):
                        got = _sqerr(family, a_fmt, w_fmt, a, w, bias, dref, drw)
                        assert torch.equal(_plain(family, a_fmt, w_fmt, a, w, bias).cpu(), y16), "the plain form's bits depend on the tiling"
                    assert got.shape == (1,) and got.dtype == torch.float32
                    got = float(got.cpu())
                    bm = gm.tile_rows(family, tokens, outs, forced)
                    rel, floor = gm.bound(tokens, outs, bm, dtype, float(rw.max()))
                    r = gm.ratio(got, want, rel, floor)
                    print(f"{family} {a_fmt} x {w_fmt} {shape} ref {dtype} bias {with_bias} cfg {forced} ({bm}-row tiles): loss {got:.6g}, err / bound {r:.3g}")
                    assert r <= 1.0, (shape, dtype, forced, got, want)
                    assert got == gm.emulate(ref, y16, rw, bm), ("the emulated order", shape, dtype, forced)
                    bits[forced] = got
                if family == "fp4":
                    assert bits[40] == bits[None], "FPQ_GEMM_CFG 40 runs the 64 x 128 tile behind the two-stage ring: the same bits"


@pytest.mark.parametrize("family,a_fmt,w_fmt", [PAIRS[0], PAIRS[2], PAIRS[5], PAIRS[10]], ids=lambda v: str(v))
def test_zero_loss_out_view_workspace_and_empty_problem(dev, family, a_fmt, w_fmt):
    from fpqvar_amd import gemm
    shape = (257, 136, 128)
    a, w, bias, y16, ref, rw = _case(family, a_fmt, w_fmt, shape, F16)
    drw = rw.to(dev)
    # ref == y16: exactly 0.0, fp16 and fp32 reference
    for dtype in (F16, F32):
        assert float(_sqerr(family, a_fmt, w_fmt, a, w, bias, y16.to(dtype).to(dev), drw).cpu()) == 0.0
    # into an entry of a loss table: the same bits, the neighbours untouched
    dref = ref.to(dev)
    got = _sqerr(family, a_fmt, w_fmt, a, w, bias, dref, drw).cpu()
    table = torch.full((3, 3), -7.0, dtype=torch.float32, device=dev)
    ret = _sqerr(family, a_fmt, w_fmt, a, w, bias, dref, drw, out=table[1, 2])
    assert ret.data_ptr() == table[1, 2].data_ptr()
    host = table.cpu()
    assert host[1, 2].view(torch.int32) == got.view(torch.int32)[0]
    host[1, 2] = -7.0
    assert bool((host == -7.0).all()), "elements beside the out view were written"
    # the same bits whatever the workspace held (no memset, no atomics), and with the wrapper's own workspace
    n = gemm.sqerr_workspace_bytes(shape[0], shape[1]) // 4
    assert n == 5 * 2
    for fill in (0.0, math.nan, -1e30):
        ws = torch.full((n + 3,), fill, dtype=torch.float32, device=dev)
        again = _sqerr(family, a_fmt, w_fmt, a, w, bias, dref, drw, workspace=ws).cpu()
        assert torch.equal(again.view(torch.int32), got.view(torch.int32)), fill
    # no tokens: 0.0f, one launch
    k = shape[2]
    a0 = _quantize(torch.empty(0, k, dtype=F16, device=dev), a_fmt)
    out = torch.full((1,), -7.0, dtype=torch.float32, device=dev)
    _sqerr(family, a_fmt, w_fmt, a0, w, bias, torch.empty(0, shape[1], dtype=F16, device=dev), torch.empty(0, dtype=F32, device=dev), out=out)
    assert out.cpu().tolist() == [0.0]


@pytest.mark.parametrize("family,a_fmt,w_fmt", [PAIRS[0], PAIRS[1], PAIRS[3], PAIRS[12]], ids=lambda v: str(v))
def test_non_finite_element_in_the_last_valid_row_of_a_partly_filled_tile(dev, family, a_fmt, w_fmt):
    """row T - 1 is the row every row past T duplicates: its NaN / inf must count once, by the fp32 expression's rule"""
    shape = (37, 200, 384)
    for dtype in (F16, F32):
        a, w, bias, y16, ref, rw = _case(family, a_fmt, w_fmt, shape, dtype)
        drw = rw.to(dev)
        for col in (0, 199):
            for bad, want in ((math.nan, "nan"), (math.inf, "inf"), (-math.inf, "inf")):
                r = ref.clone()
                r[36, col] = bad
                assert gm.expected_class(r, y16) == want
                got = float(_sqerr(family, a_fmt, w_fmt, a, w, bias, r.to(dev), drw).cpu())
                assert gm.class_of(got) == want, (dtype, col, bad, got)
                assert not (want == "inf" and got < 0)


def test_refusals_are_runtime_errors_in_the_familys_order(dev):
    from fpqvar_amd import gemm
    a, w, bias, y16, ref, rw = _case("fp4", "e2m1", "e2m1", (37, 200, 384), F16)
    dref, drw = ref.to(dev), rw.to(dev)
    with pytest.raises(RuntimeError, match="expected a tensor on the GPU"):
        gemm.linear_fp4_sqerr(a[0].cpu(), a[1], *w, dref, drw)
    with pytest.raises(RuntimeError, match="row-major operands only"):
        gemm.linear_fp4_sqerr(a[0].view(3, 37, 64), a[1], *w, dref, drw)
    with pytest.raises(RuntimeError, match="operand shapes"):                                    # the operands before the form's own arguments
        gemm.linear_fp4_sqerr(a[0][:, :128], a[1], *w, dref[:1], drw)
    with pytest.raises(RuntimeError, match="ref must be"):
        gemm.linear_fp4_sqerr(*a, *w, dref[:, :192], drw)
    with pytest.raises(RuntimeError, match="ref must be"):
        gemm.linear_fp4_sqerr(*a, *w, dref.double(), drw)
    with pytest.raises(RuntimeError, match="row_weight must be"):
        gemm.linear_fp4_sqerr(*a, *w, dref, drw.half())
    with pytest.raises(RuntimeError, match="out must be"):
        gemm.linear_fp4_sqerr(*a, *w, dref, drw, out=torch.empty(2, dtype=F32, device=dev))
    with pytest.raises(RuntimeError, match="workspace must be"):
        gemm.linear_fp4_sqerr(*a, *w, dref, drw, workspace=torch.empty(0, dtype=F32, device=dev))
    with pytest.raises(RuntimeError, match="fpq error -1"):                                      # row_weight 4 bytes past alignment
        gemm.linear_fp4_sqerr(*a, *w, dref, torch.ones(41, dtype=F32, device=dev)[1:38])
    with pytest.raises(RuntimeError, match="6-bit activation tables"):
        gemm.linear_a6w4_sqerr(*a, "e2m3", *w, dref, drw)
    with pytest.raises(RuntimeError, match="weight scales must be float32"):
        gemm.linear_w6_sqerr(*a, "e2m1", w[0], w[1].half(), "e3m0", dref, drw)
    with pytest.raises(RuntimeError, match="6-bit operand formats"):
        gemm.linear_fp6_sqerr(*a, *w, dref, drw, a_table="e1m2")
