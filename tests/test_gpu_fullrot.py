"""The full-width online rotation + per-group quantizer on the GPU (rotation.rotate_quant_full / rotate_quant_full_mx,
csrc/fpq_fullrot.h) against the float64 model of tests/fullrot_model.py.  Run with ``-m gpu``.

Contract: every finite rotated value lies within fullrot_model.bound() of the float64 product with half(Q) - the matrix
rotate_model(block_rotate=False) puts into the weights; the quantizer is bit for bit the stand-alone one on the rotated rows the
kernel produced; the operand form is byte for byte gemm.quantize_mx of them, in both layouts.

Measured on the MI355X: the figures are in the docstrings of the tests that print them (and in DESIGN.md section 4g).
"""
import pytest
import torch

from oracle import fpq_oracle as orc
from tests import fullrot_model as fm
from tests.conftest import assert_bits_equal

pytestmark = pytest.mark.gpu

ROWS = (1, 3, 17, 300)
TABLES = ("e2m1", "e1m2", "e3m0", "e2m3")
RESIDENT_ROWS = 256 * 4 * 4       # csrc/fpq_fullrot.hip, fullrot_grid: kFrCUs x kFrWaves workgroups of 4 wavefronts, one row each


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "these tests need the GPU"
    return torch.device("cuda:0")


_CASES = {}


def case(C, in_dtype, with_smooth, rows=300, family="heavy"):
    """(x, smooth, h16, float64 reference) - computed once per case, shared and left unchanged"""
    key = (C, in_dtype, with_smooth, rows, family)
    if key not in _CASES:
        x = fm.FAMILIES[family](rows, C, seed=C + rows).to(in_dtype)
        g = torch.Generator().manual_seed(C + 1)
        s = (torch.rand(C, generator=g) * 1.5 + 0.25) if with_smooth else None
        h = (x.float() * s).half() if with_smooth else x.half()
        _CASES[key] = (x, s, h, fm.reference(h, C))
    return _CASES[key]


def worst_ratio(y, h, ref, C):
    y = y.double().cpu()
    fin = torch.isfinite(ref) & (ref.abs() < 65520.0)
    assert torch.isfinite(y[fin]).all(), "a non-finite output where the product is finite"
    return float(((y - ref).abs() / fm.bound(h, ref, C))[fin].max())


@pytest.mark.parametrize("C", fm.WIDTHS)
@pytest.mark.parametrize("in_dtype", (torch.float16, torch.float32))
@pytest.mark.parametrize("with_smooth", (False, True))
def test_rotated_values_within_the_bound(dev, C, in_dtype, with_smooth):
    """Worst err / bound measured on the MI355X, heavy-tailed rows, at 1 / 3 / 17 / 300 rows (fp32 rows give the same figures):
        C = 1920 no smooth 0.767 0.764 0.773 0.786      with a smoothing vector 0.745 0.754 0.780 0.820
        C = 2304 no smooth 0.763 0.785 0.790 0.801      with a smoothing vector 0.774 0.785 0.794 0.807"""
    from fpqvar_amd import rotation as rot
    for rows in ROWS:
        x, s, h, ref = case(C, in_dtype, with_smooth, rows)
        out, y = rot.rotate_quant_full(x.to(dev), "e2m1", smooth=None if s is None else s.to(dev), return_rotated=True)
        ratio = worst_ratio(y, h, ref, C)
        print(f"fullrot C={C} {in_dtype} smooth={with_smooth} rows={rows}: worst err / bound {ratio:.3f}")
        assert ratio <= 1.0
        assert_bits_equal(out, orc.per_group_kernel_sem(y.cpu(), "e2m1", 128), "quant of rotated")


@pytest.mark.parametrize("C", fm.WIDTHS)
@pytest.mark.parametrize("family", list(fm.FAMILIES))
def test_rotated_values_by_input_family(dev, C, family):
    """Worst err / bound measured on the MI355X (C = 1920 / 2304): gauss 0.698 / 0.740, heavy 0.773 / 0.790, dominant 0.973 / 0.961,
    cancelling 0.844 / 0.932 - the CPU emulation's figures (tests/test_fullrot_model_host.py) to three digits."""
    from fpqvar_amd import rotation as rot
    x, s, h, ref = case(C, torch.float16, False, 17, family)
    _, y = rot.rotate_quant_full(x.to(dev), return_rotated=True)
    ratio = worst_ratio(y, h, ref, C)
    print(f"fullrot C={C} family {family}: worst err / bound {ratio:.3f}")
    assert ratio <= 1.0


@pytest.mark.parametrize("C", fm.WIDTHS)
@pytest.mark.parametrize("in_dtype", (torch.float16, torch.float32))
def test_quantizer_is_the_stand_alone_one(dev, C, in_dtype):
    from fpqvar_amd import ops, rotation as rot
    x, s, h, ref = case(C, in_dtype, True)
    xd, sd = x.to(dev), s.to(dev)
    y0 = None
    for table in TABLES:
        out, y = rot.rotate_quant_full(xd, table, smooth=sd, return_rotated=True)
        assert_bits_equal(rot.rotate_quant_full(xd, table, smooth=sd), out, f"{table}: return_rotated=False")
        assert_bits_equal(out, orc.per_group_kernel_sem(y.cpu(), table, 128, out_dtype=torch.float16), f"{table}: oracle on the rotated rows")
        assert_bits_equal(out, ops.quant_rows(y, table, 128), f"{table}: ops.quant_rows on the rotated rows")
        y0 = y if y0 is None else y0
        assert_bits_equal(y, y0, "rotation independent of the table")


@pytest.mark.parametrize("C", fm.WIDTHS)
def test_more_rows_than_the_grid_holds(dev, C):
    """Every wavefront takes a second row and some a third; a row's result does not depend on where it runs."""
    from fpqvar_amd import gemm, rotation as rot
    x, s, h, ref = case(C, torch.float16, False)
    rows = 2 * RESIDENT_ROWS + 37
    idx = torch.arange(rows) % 300
    xd = x.to(dev)
    big = xd[idx.to(dev)].contiguous()
    out, y = rot.rotate_quant_full(xd, return_rotated=True)
    out_b, y_b = rot.rotate_quant_full(big, return_rotated=True)
    assert torch.equal(y_b.view(torch.int16), y.view(torch.int16)[idx.to(dev)]) and torch.equal(out_b.view(torch.int16), out.view(torch.int16)[idx.to(dev)])
    for km in (False, True):
        cd, sc = rot.rotate_quant_full_mx(big, kmajor=km)
        cw, sw = gemm.quantize_mx(y_b, kmajor=km)
        assert torch.equal(cd, cw) and torch.equal(sc.view(torch.int32 if km else torch.int16), sw.view(torch.int32 if km else torch.int16))


@pytest.mark.parametrize("C", fm.WIDTHS)
@pytest.mark.parametrize("kmajor", (False, True))
def test_operands_are_quantize_mx_of_the_rotated_rows(dev, C, kmajor):
    from fpqvar_amd import gemm, rotation as rot
    for in_dtype, with_smooth in ((torch.float16, False), (torch.float32, True), (torch.float16, True), (torch.float32, False)):
        for rows in ROWS:
            x, s, h, ref = case(C, in_dtype, with_smooth, rows)
            xd, sd = x.to(dev), None if s is None else s.to(dev)
            _, y = rot.rotate_quant_full(xd, smooth=sd, return_rotated=True)
            cd, sc = rot.rotate_quant_full_mx(xd, smooth=sd, kmajor=kmajor)
            cw, sw = gemm.quantize_mx(y, kmajor=kmajor)
            assert cd.shape == cw.shape and sc.shape == sw.shape and sc.dtype == sw.dtype
            assert torch.equal(cd, cw), (in_dtype, with_smooth, rows)
            it = torch.int32 if kmajor else torch.int16
            assert torch.equal(sc.view(it), sw.view(it)), (in_dtype, with_smooth, rows)      # the whole image, padding rows included


@pytest.mark.parametrize("kmajor", (False, True))
def test_operands_in_a_captured_graph(dev, kmajor):
    from fpqvar_amd import rotation as rot
    x, s, h, ref = case(2304, torch.float16, True, 17)
    xd, sd = x.to(dev), s.to(dev)
    eager = rot.rotate_quant_full_mx(xd, smooth=sd, kmajor=kmajor)
    eager_v = rot.rotate_quant_full(xd, "e3m0", smooth=sd)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.stream(side):
        rot.rotate_quant_full_mx(xd, smooth=sd, kmajor=kmajor)      # warm-up on the capture stream
        side.synchronize()
        with torch.cuda.graph(graph, stream=side):
            got = rot.rotate_quant_full_mx(xd, smooth=sd, kmajor=kmajor)
            got_v = rot.rotate_quant_full(xd, "e3m0", smooth=sd)
    for t in (*got, got_v):
        t.zero_()
    graph.replay()
    torch.cuda.synchronize()
    assert torch.equal(got[0], eager[0])
    it = torch.int32 if kmajor else torch.int16
    assert torch.equal(got[1][:, :17].view(it) if kmajor else got[1].view(it), eager[1][:, :17].view(it) if kmajor else eager[1].view(it))
    assert_bits_equal(got_v, eager_v, "values in the graph")


@pytest.mark.parametrize("C", fm.WIDTHS)
@pytest.mark.parametrize("kmajor", (False, True))
def test_linear_rotate_operands_full_width(dev, C, kmajor):
    from fpqvar_amd import gemm, rotation as rot
    x, s, h, ref = case(C, torch.float16, True, 17)
    xd, sd = x.to(dev), s.to(dev)
    g = torch.Generator().manual_seed(3)
    base = torch.nn.Linear(C, 256)
    with torch.no_grad():
        base.weight.copy_(torch.randn(256, C, generator=g) * 0.05)
        base.bias.copy_(torch.randn(256, generator=g) * 0.1)
    base = base.to(dev)
    lin = gemm.FP4Linear.from_float(base, kmajor=kmajor)
    _, y = rot.rotate_quant_full(xd, smooth=sd, return_rotated=True)
    got = lin.forward_operands(*lin.rotate_operands(xd, smooth=sd, full_width=True))
    want = lin.forward_operands(*gemm.quantize_mx(y, kmajor=kmajor))
    assert_bits_equal(got, want, "FP4Linear on the fused operands")
    lin6 = gemm.FP4Linear.from_float(base, act_fp_type="fp_e3")
    with pytest.raises(NotImplementedError):
        lin6.rotate_operands(xd, full_width=True)


@pytest.mark.parametrize("C", fm.WIDTHS)
@pytest.mark.parametrize("in_dtype", (torch.float16, torch.float32))
def test_non_finite_rows(dev, C, in_dtype):
    """In full-width mode a non-finite input poisons its whole row (the dense Q has no zero entry), in the reference too.  isfinite(y)
    is that of the float64 product with |exact| >= 65520 -> +-inf; where the product is +-inf the sign matches; a zero row stays +0."""
    from fpqvar_amd import rotation as rot
    x, s, h, ref = case(C, in_dtype, False, 17)
    x = x.clone()
    q = fm.q_half(C)
    x[1, 5] = float("nan")
    x[2, 77] = float("inf")
    x[5, 130] = float("inf")
    x[5, C - 3] = float("inf")
    x[6, 140] = float("inf")
    x[6, 1000] = float("-inf")                                  # both: every output is +-inf or NaN
    x[9] = (torch.sign(q[:, 321]) * 60000.0).to(in_dtype)       # finite inputs, ONE output overflows fp16; the others cancel to 0
    x[10] = (torch.sign(q[:, C - 1]) * -60000.0).to(in_dtype)
    x[11] = 0
    x[12, C - 1] = float("-inf")
    out, y = rot.rotate_quant_full(x.to(dev), "e2m1", return_rotated=True)
    y = y.cpu()
    exact = x.half().double() @ q
    exact = torch.where(exact.abs() >= 65520.0, exact.sign() * float("inf"), exact)
    assert torch.equal(torch.isfinite(y), torch.isfinite(exact)), "non-finite outputs in other places"
    assert torch.equal(torch.isnan(y), torch.isnan(exact))
    inf = torch.isinf(exact)
    assert inf[9].sum() == 1 and inf[10].sum() == 1 and inf[2].all() and inf[12].all() and torch.isnan(exact[1]).all()
    assert torch.equal(torch.sign(y[inf].double()), torch.sign(exact[inf])), "the sign of an infinite output"
    assert torch.equal(y[11].view(torch.int16), torch.zeros(C, dtype=torch.int16)), "a zero row: all +0.0"
    assert_bits_equal(out, orc.per_group_kernel_sem(y, "e2m1", 128), "quant of rotated, non-finite groups included")
    assert torch.equal(out[11].cpu().view(torch.int16), torch.zeros(C, dtype=torch.int16))
    fin = torch.isfinite(exact)
    hh = torch.where(torch.isfinite(x.half()), x.half(), torch.zeros((), dtype=torch.float16))
    b = fm.bound(hh, torch.where(fin, exact, torch.zeros((), dtype=torch.float64)), C)
    rows_ok = fin.all(dim=1) | (torch.arange(17) == 9) | (torch.arange(17) == 10)
    sel = fin & rows_ok[:, None]
    assert bool(((y.double() - exact).abs()[sel] <= b[sel]).all())
    cd, sc = rot.rotate_quant_full_mx(x.to(dev))
    from fpqvar_amd import gemm
    cw, sw = gemm.quantize_mx(y.to(dev))
    assert torch.equal(cd, cw) and torch.equal(sc.view(torch.int16), sw.view(torch.int16))


@pytest.mark.parametrize("C", fm.WIDTHS)
def test_against_the_reference_op_sequence(dev, C):
    """(d) torch.matmul(h, Q) under fp16 autocast + fp_quant_e2_per_group_cuda - the reference's online side; (e) the quantizer on
    the float64-exact rotated rows; (f) the fused launch.  Required: agreement(f, e) >= agreement(d, e): the fused form is at least as
    close to the exact result as the reference's own GEMM.  Measured on the MI355X (300 x C heavy-tailed rows):
        C = 1920: agreement(f, e) 0.99980, agreement(d, e) 0.99940, agreement(f, d) 0.99960
        C = 2304: agreement(f, e) 1.00000, agreement(d, e) 0.99934, agreement(f, d) 0.99934"""
    import fpqvar_amd.quant_utils as qu
    from fpqvar_amd import rotation as rot
    x, s, h, ref = case(C, torch.float16, False)
    with torch.autocast("cuda", dtype=torch.float16):
        x1 = torch.matmul(h.to(dev), rot.get_orthogonal_matrix(C, device=dev).float())
    d = qu.fp_quant_e2_per_group_cuda(x1, 4, 128).cpu()
    e = orc.per_group_kernel_sem(ref.half(), "e2m1", 128)
    f = rot.rotate_quant_full(x.to(dev), "e2m1").cpu()

    def agreement(a, b):
        return float((a.view(torch.int16) == b.view(torch.int16)).float().mean())
    fe, de, fd = agreement(f, e), agreement(d, e), agreement(f, d)
    print(f"fullrot C={C}: agreement fused/exact {fe:.5f}, reference GEMM/exact {de:.5f}, fused/reference GEMM {fd:.5f}")
    assert fe >= de
