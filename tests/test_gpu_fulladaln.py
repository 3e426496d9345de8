"""The full-width adaLN producer on the GPU (rotation.adaln_rotate_quant_full / adaln_rotate_quant_full_mx, csrc/fpq_fulladaln.h):
LayerNorm + modulate, the full-width rotation and the per-group quantizer in one launch.  Run with ``-m gpu``.

Contract: the modulated row h lies within fulladaln_model.bound() of the float64 chain on every finite row and is non-finite exactly
where the chain is; everything behind h is rotate_quant_full(h) bit for bit - the rotated rows within fullrot_model.bound() of the
float64 product, the quantizer the stand-alone one, the operand form byte for byte gemm.quantize_mx of the rotated rows in both
layouts; a row's result does not depend on where in the grid it runs.

Measured on the MI355X: the figures are in the docstrings of the tests that print them (and in DESIGN.md section 4g).
"""
import itertools

import pytest
import torch

from oracle import fpq_oracle as orc
from tests import adaln_model as am
from tests import fulladaln_model as fa
from tests import fullrot_model as fm
from tests.conftest import assert_bits_equal

pytestmark = pytest.mark.gpu

F16, F32 = torch.float16, torch.float32
SHAPES = ((2, 13), (3, 1), (3, 3), (2, 17))   # L = 13: every family in one launch; L = 1, 3 with B = 3: batch boundaries inside a workgroup's rows
EPS = (1e-6, 1e-5, 1e-3)
TABLES = ("e2m1", "e1m2", "e3m0", "e2m3")
RESIDENT_ROWS = 256 * 4 * 4       # csrc/fpq_fullrot.h, fullrot_grid: kFrCUs x kFrWaves workgroups of 4 wavefronts, one row each


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "these tests need the GPU"
    return torch.device("cuda:0")


_CASES = {}


def case(B, L, C, x_dtype, mod_dtype=F16, with_smooth=True, eps=1e-6, fams=am.FAMILIES):
    """(x [B, L, C], scale, shift [B, 1, C], smooth, the float64 reference) on the CPU - computed once, shared and left unchanged"""
    key = (B, L, C, x_dtype, mod_dtype, with_smooth, eps, fams)
    if key not in _CASES:
        x, scale, shift, smooth = fa.make_case(B, L, C, x_dtype, mod_dtype, with_smooth, eps, fams=fams)
        _CASES[key] = (x.view(B, L, C), scale.view(B, 1, C), shift.view(B, 1, C), smooth, fa.reference(x, scale, shift, smooth, eps, L))
    return _CASES[key]


def on(dev, *ts):
    return [None if t is None else t.to(dev) for t in ts]


def mx_equal(got, want, kmajor):
    it = torch.int32 if kmajor else torch.int16
    return got[0].shape == want[0].shape and got[1].shape == want[1].shape and got[1].dtype == want[1].dtype and \
        torch.equal(got[0], want[0]) and torch.equal(got[1].view(it), want[1].view(it))      # the whole image, padding rows included


@pytest.mark.parametrize("C", fa.WIDTHS)
@pytest.mark.parametrize("x_dtype", (F16, F32))
def test_h_within_the_bound(dev, C, x_dtype):
    """h against the float64 chain on all 13 families, four (B, L), both modulation dtypes, with and without a smoothing vector, three
    eps.  Worst err / bound measured on the MI355X (the half-ulp term dominates; the CPU model gives 0.9993):
        C = 1920 fp16 rows 0.9993   fp32 rows 0.9986      C = 2304 fp16 rows 0.9981   fp32 rows 0.9982"""
    from fpqvar_amd import rotation as rot
    worst_all = 0.0
    for (B, L), mod_dtype, with_smooth, eps in itertools.product(SHAPES, (F16, F32), (False, True), EPS):
        x, sc, sh, s, ref = case(B, L, C, x_dtype, mod_dtype, with_smooth, eps)
        xd, scd, shd, sd = on(dev, x, sc, sh, s)
        out, h, y = rot.adaln_rotate_quant_full(xd, scd, shd, "e2m1", smooth=sd, eps=eps, return_intermediates=True)
        worst, where_ok = fa.check(h.cpu().view(B * L, C), ref, x_dtype, C)
        worst_all = max(worst_all, worst)
        assert worst <= 1.0 and where_ok, (B, L, mod_dtype, with_smooth, eps, worst, where_ok)
    print(f"fulladaln C={C} {x_dtype}: worst err / bound of h {worst_all:.4f}")


@pytest.mark.parametrize("C", fa.WIDTHS)
@pytest.mark.parametrize("x_dtype", (F16, F32))
def test_behind_h_bit_for_bit(dev, C, x_dtype):
    """rotated and out are rotate_quant_full(h)'s, the quantizer is the stand-alone one and the oracle's, and asking for the
    intermediates changes nothing - the inf and nan rows of L = 13 included."""
    from fpqvar_amd import ops, rotation as rot
    for mod_dtype, with_smooth in ((F16, True), (F32, False)):
        x, sc, sh, s, ref = case(2, 13, C, x_dtype, mod_dtype, with_smooth)
        xd, scd, shd, sd = on(dev, x, sc, sh, s)
        h0 = None
        for table in TABLES:
            out, h, y = rot.adaln_rotate_quant_full(xd, scd, shd, table, smooth=sd, return_intermediates=True)
            out2, y2 = rot.rotate_quant_full(h, table, return_rotated=True)
            assert_bits_equal(y, y2, f"{table}: rotated against rotate_quant_full(h)")
            assert_bits_equal(out, out2, f"{table}: out against rotate_quant_full(h)")
            assert_bits_equal(out, ops.quant_rows(y, table, 128), f"{table}: ops.quant_rows on the rotated rows")
            assert_bits_equal(out, orc.per_group_kernel_sem(y.cpu(), table, 128, out_dtype=torch.float16), f"{table}: oracle on the rotated rows")
            assert_bits_equal(rot.adaln_rotate_quant_full(xd, scd, shd, table, smooth=sd), out, f"{table}: return_intermediates=False")
            h0 = h if h0 is None else h0
            assert_bits_equal(h, h0, "h independent of the table")


@pytest.mark.parametrize("C", fa.WIDTHS)
@pytest.mark.parametrize("x_dtype", (F16, F32))
def test_rotated_rows(dev, C, x_dtype):
    """Rows with a finite h: within fullrot_model.bound of the float64 product of h.  A row with a non-finite h (the inf and nan
    families: LayerNorm makes the whole row NaN) is non-finite throughout, with the isfinite / isnan pattern of the float64 product."""
    from fpqvar_amd import rotation as rot
    seen_bad = 0
    for B, L in SHAPES:
        x, sc, sh, s, ref = case(B, L, C, x_dtype)
        xd, scd, shd, sd = on(dev, x, sc, sh, s)
        _, h, y = rot.adaln_rotate_quant_full(xd, scd, shd, smooth=sd, return_intermediates=True)
        h, y = h.cpu().view(B * L, C), y.cpu().view(B * L, C)
        good = torch.isfinite(h).all(dim=1)
        assert torch.equal(good, ref["finite"])
        hz = torch.where(good[:, None], h, torch.zeros((), dtype=F16))
        exact = fm.reference(hz, C)
        assert float(exact.abs().max()) < 65520.0
        assert torch.isfinite(y[good]).all()
        assert bool(((y.double() - exact).abs()[good] <= fm.bound(hz, exact, C)[good]).all())
        if (~good).any():
            bad = h[~good].double() @ fm.q_half(C)
            assert not torch.isfinite(y[~good]).any()
            assert torch.equal(torch.isfinite(y[~good]), torch.isfinite(bad)) and torch.equal(torch.isnan(y[~good]), torch.isnan(bad))
            seen_bad += int((~good).sum())
    assert seen_bad >= 4


@pytest.mark.parametrize("C", fa.WIDTHS)
@pytest.mark.parametrize("kmajor", (False, True))
def test_operands_are_quantize_mx_of_the_rotated_rows(dev, C, kmajor):
    from fpqvar_amd import gemm, rotation as rot
    for (B, L), x_dtype in itertools.product(SHAPES, (F16, F32)):
        mod_dtype, with_smooth = (F16, True) if x_dtype == F32 else (F32, False)
        x, sc, sh, s, ref = case(B, L, C, x_dtype, mod_dtype, with_smooth)
        xd, scd, shd, sd = on(dev, x, sc, sh, s)
        _, _, y = rot.adaln_rotate_quant_full(xd, scd, shd, smooth=sd, return_intermediates=True)
        got = rot.adaln_rotate_quant_full_mx(xd, scd, shd, smooth=sd, kmajor=kmajor)
        assert mx_equal(got, gemm.quantize_mx(y.view(B * L, C), kmajor=kmajor), kmajor), (B, L, x_dtype)


@pytest.mark.parametrize("C", fa.WIDTHS)
def test_more_rows_than_the_grid_holds(dev, C):
    """2 x resident + 37 = 8229 = 39 x 211 rows gathered from a 2 x 150-row case: every wavefront takes a second row and some a third,
    the batch entries are 211 rows long - their boundaries fall inside workgroups and move from one pass over the grid to the next.
    Each row's h, rotated, out, codes and scales are those of the small launch for the row with the same data and modulation."""
    from fpqvar_amd import gemm, rotation as rot
    x, sc, sh, s, ref = case(2, 150, C, F32)
    xd, scd, shd, sd = on(dev, x, sc, sh, s)
    rows, per = 2 * RESIDENT_ROWS + 37, 211
    assert rows % per == 0 and rows > 2 * RESIDENT_ROWS
    r = torch.arange(rows)
    entry = (r // per) % 2                                   # the small batch entry a big batch entry takes its modulation from
    idx = (entry * 150 + (r * 7) % 150).to(dev)              # ... and its rows
    big = xd.view(300, C)[idx].view(rows // per, per, C).contiguous()
    pick = (torch.arange(rows // per) % 2).to(dev)
    sc_b, sh_b = scd[pick].contiguous(), shd[pick].contiguous()
    out, h, y = rot.adaln_rotate_quant_full(xd, scd, shd, smooth=sd, return_intermediates=True)
    out_b, h_b, y_b = rot.adaln_rotate_quant_full(big, sc_b, sh_b, smooth=sd, return_intermediates=True)
    for name, small, large in (("h", h, h_b), ("rotated", y, y_b), ("out", out, out_b)):
        assert torch.equal(large.view(rows, C).view(torch.int16), small.view(300, C).view(torch.int16)[idx]), name
    assert_bits_equal(rot.adaln_rotate_quant_full(big, sc_b, sh_b, smooth=sd), out_b, "return_intermediates=False")
    for km in (False, True):
        assert mx_equal(rot.adaln_rotate_quant_full_mx(big, sc_b, sh_b, smooth=sd, kmajor=km), gemm.quantize_mx(y_b.view(rows, C), kmajor=km), km), km


def test_in_a_captured_graph(dev):
    """values and both operand layouts in ONE linear capture (one stream, no parallel branches); the replay equals eager"""
    from fpqvar_amd import rotation as rot
    C = 2304
    x, sc, sh, s, ref = case(1, 17, C, F32)
    xd, scd, shd, sd = on(dev, x, sc, sh, s)

    def run():
        return (rot.adaln_rotate_quant_full(xd, scd, shd, "e3m0", smooth=sd), *rot.adaln_rotate_quant_full_mx(xd, scd, shd, smooth=sd),
                *rot.adaln_rotate_quant_full_mx(xd, scd, shd, smooth=sd, kmajor=True))
    eager = run()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.stream(side):
        run()                                                   # warm-up on the capture stream
        side.synchronize()
        with torch.cuda.graph(graph, stream=side):
            got = run()
    for t in got:
        t.zero_()
    graph.replay()
    torch.cuda.synchronize()
    assert_bits_equal(got[0], eager[0], "values in the graph")
    assert torch.equal(got[1], eager[1]) and torch.equal(got[2].view(torch.int16), eager[2].view(torch.int16))
    assert torch.equal(got[3], eager[3]) and torch.equal(got[4][:, :17].view(torch.int32), eager[4][:, :17].view(torch.int32))


@pytest.mark.parametrize("C", fa.WIDTHS)
@pytest.mark.parametrize("kmajor", (False, True))
def test_linear_adaln_operands_full_width(dev, C, kmajor):
    from fpqvar_amd import gemm, rotation as rot
    x, sc, sh, s, ref = case(2, 17, C, F32)
    xd, scd, shd, sd = on(dev, x, sc, sh, s)
    g = torch.Generator().manual_seed(3)
    base = torch.nn.Linear(C, 256)
    with torch.no_grad():
        base.weight.copy_(torch.randn(256, C, generator=g) * 0.05)
        base.bias.copy_(torch.randn(256, generator=g) * 0.1)
    base = base.to(dev)
    lin = gemm.FP4Linear.from_float(base, kmajor=kmajor)
    _, _, y = rot.adaln_rotate_quant_full(xd, scd, shd, smooth=sd, return_intermediates=True)
    got = lin.forward_operands(*lin.adaln_operands(xd, scd, shd, smooth=sd, full_width=True))
    want = lin.forward_operands(*gemm.quantize_mx(y.view(-1, C), kmajor=kmajor))
    assert_bits_equal(got, want, "FP4Linear on the fused operands")
    with pytest.raises(NotImplementedError):
        gemm.FP4Linear.from_float(base, act_fp_type="fp_e3").adaln_operands(xd, scd, shd, full_width=True)
    with pytest.raises(NotImplementedError):
        lin.adaln_operands(xd, scd, shd, pending=(xd, scd), full_width=True)


@pytest.mark.parametrize("C", fa.WIDTHS)
def test_against_the_reference_op_sequence(dev, C):
    """300 fp32 rows (B = 3, L = 100) of the gauss and lognormal families.  (d) torch's layer_norm / mul / add_ / mul(smooth) / matmul(Q)
    under fp16 autocast + fp_quant_e2_per_group_cuda - the reference's online side; (e) the oracle quantizer on half(float64 product of
    half(float64 h)); (f) the fused launch.  Required: agreement(f, e) >= 0.97, the standing contract for fused producers (DESIGN.md
    section 2).  Reported, not asserted: agreement(f, e) >= agreement(d, e).  Measured on the MI355X:
        C = 1920: agreement(f, e) 0.99959, agreement(d, e) 0.99899, agreement(f, d) 0.99858
        C = 2304: agreement(f, e) 0.99967, agreement(d, e) 0.99950, agreement(f, d) 0.99950"""
    import fpqvar_amd.quant_utils as qu
    from fpqvar_amd import rotation as rot
    x, sc, sh, s, ref = case(3, 100, C, F32, fams=("gauss", "lognormal"))
    xd, scd, shd, sd = on(dev, x, sc, sh, s)
    ln = torch.nn.functional.layer_norm(xd, (C,), eps=1e-6)
    with torch.autocast("cuda", dtype=torch.float16):
        x1 = torch.matmul(ln.mul(scd.add(1)).add_(shd).mul(sd), rot.get_orthogonal_matrix(C, device=dev).float())
    d = qu.fp_quant_e2_per_group_cuda(x1, 4, 128).cpu().view(300, C)
    e = orc.per_group_kernel_sem(fm.reference(ref["h"].half(), C).half(), "e2m1", 128)
    f = rot.adaln_rotate_quant_full(xd, scd, shd, "e2m1", smooth=sd).cpu().view(300, C)

    def agreement(a, b):
        return float((a.view(torch.int16) == b.view(torch.int16)).float().mean())
    fe, de, fd = agreement(f, e), agreement(d, e), agreement(f, d)
    print(f"fulladaln C={C}: agreement fused/exact {fe:.5f}, reference chain/exact {de:.5f}, fused/reference chain {fd:.5f}; "
          f"fused at least as close as the reference chain: {fe >= de}")
    assert fe >= 0.97
