"""The full-width producers in front of the per-token FP6 quantizer on the GPU (rotation.rotate_quant_full_token /
adaln_rotate_quant_full_token, csrc/fpq_fulltoken.h; include/fpq.h, fpq_fullrot_quant_token_rows*).  Run with ``-m gpu``.

Contracts, all bit for bit:
  rotated == rotate_quant_full(x, return_rotated=True)[1]; behind the adaLN front h and rotated ==
    adaln_rotate_quant_full(return_intermediates=True)'s - so both inherit tests/fullrot_model.py's and tests/fulladaln_model.py's bounds;
  out == quant_utils.fp6_quant_{e2m3,e3m2}_per_token_cuda(rotated, 6), row_scales == gemm.quantize_fp6(rotated)'s scales;
  (codes, scales) == gemm.quantize_fp6(rotated, kmajor=..., table=...) byte for byte over the WHOLE image - row-major [rows, C * 3 / 4]
    or k-major [C / 128, rows, 96]: neither emitter leaves a padding row, every byte of both images is compared - and decoded == out;
  all-zero, inf and NaN rows: what the stand-alone quantizer gives on the same rotated row (every NaN counts as one value, as
    everywhere in this suite); a row's scale does not depend on its neighbours (each row equals the row of a launch of its own order).
Rows: 1 and 3 (idle wavefronts in the workgroup), 17 (the k-major row swizzle over more than one 8- and 16-row period), 8229 (more
than the resident grid: a wavefront walks three rows and rewrites its LDS image)."""
import functools

import pytest
import torch

from tests.conftest import assert_bits_equal

pytestmark = pytest.mark.gpu

F16, F32 = torch.float16, torch.float32
WIDTHS = (1920, 2304)
RESIDENT_ROWS = 256 * 4 * 4       # csrc/fpq_fullrot.h, fullrot_grid: kFrCUs x kFrWaves workgroups of 4 wavefronts, one row each
STEP = RESIDENT_ROWS              # the distance of the rows one wavefront owns in turn at 8229 rows
EMITS = (("values", "e2m3"), ("values", "e3m2"), ("fp6", "e2m3"), ("bf6", "e3m2"))


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "these tests need the GPU"
    return torch.device("cuda:0")


def _signs(C, default):
    from fpqvar_amd import rotation as rot
    return None if default else rot.sign_vector(C, 7)


@functools.lru_cache(maxsize=None)
def _q(C, default):
    """float64 Q = diag(D) . H^T / sqrt(C) of the sign vector in use (CPU)"""
    from fpqvar_amd import rotation as rot
    d = rot.sign_vector(C, 42 if default else 7)
    return (d[:, None] * rot.hadamard_matrix(C).T) / float(C) ** 0.5


@functools.lru_cache(maxsize=None)
def _rows(C, n, default_signs, with_smooth):
    """(x fp32 [n, C], smooth or None, {family: row index}) on the CPU, computed once and left unchanged.  The two `max_*` rows are a
    spike along one column of Q (x = A Q[:, j] / smooth + noise, so the rotated row is ~ A e_j + noise): j in the first vector, and j
    in the LAST LIVE vector of the last pass (v = C / 8 - 1)."""
    g = torch.Generator().manual_seed(1000 + C + n)
    smooth = (torch.rand(C, generator=g) + 0.5) if with_smooth else None
    q = _q(C, default_signs)
    x = torch.randn(n, C, generator=g)
    where = {}

    def spike(j):
        row = 40.0 * q[:, j].float() * float(C) ** 0.5 / 8.0 + 0.05 * torch.randn(C, generator=g)
        return row / smooth if with_smooth else row
    plan = {1: ("gauss",), 3: ("max_last", "zero", "heavy"),
            17: ("gauss", "heavy", "max_last", "max_first", "finite", "zero", "finite", "inf", "finite", "nan", "finite")}.get(n, ("gauss", "heavy"))
    for i, fam in enumerate(plan):
        where.setdefault(fam, i)
        if fam == "heavy":
            x[i] = torch.randn(C, generator=g) * torch.exp(1.5 * torch.randn(C, generator=g))
        elif fam == "max_last":
            x[i] = spike(C - 3)
        elif fam == "max_first":
            x[i] = spike(2)
        elif fam == "zero":
            x[i] = 0.0
        elif fam == "inf":
            x[i, C // 3] = float("inf")
        elif fam == "nan":
            x[i, 5] = float("nan")
    if n > RESIDENT_ROWS:   # rows one wavefront owns in turn (r, r + STEP, r + 2 STEP) alternate in magnitude by 2^10
        x *= torch.where((torch.arange(n) // STEP) % 2 == 1, 2.0 ** -10, 1.0)[:, None]
    return x, smooth, where


def _standalone(y, table, kmajor=None):
    """the stand-alone per-token quantizer on the rotated rows y [rows, C]: values, or operands"""
    from fpqvar_amd import gemm, quant_utils as qu
    if kmajor is None:
        return (qu.fp6_quant_e2m3_per_token_cuda if table == "e2m3" else qu.fp6_quant_e3m2_per_token_cuda)(y, 6)
    return gemm.quantize_fp6(y, kmajor=kmajor, table=table)


def _check_all_forms(produce, y, what, tables=("e2m3", "e3m2")):
    """produce(table, emit, kmajor) -> the fused output, against the stand-alone quantizer on y [rows, C] for every emit form"""
    from fpqvar_amd import gemm
    rows, C = y.shape
    for emit, table in EMITS:
        if table not in tables:
            continue
        if emit == "values":
            assert_bits_equal(produce(table, emit, False).view(rows, C), _standalone(y, table), f"{what} {table} values")
            continue
        for km in (False, True):
            codes, scales = produce(table, emit, km)
            wc, ws = _standalone(y, table, km)
            assert codes.shape == wc.shape and codes.dtype == torch.uint8 and scales.shape == ws.shape == (rows,) and scales.dtype == F16
            assert torch.equal(codes, wc), f"{what} {table} codes kmajor={km}: {int((codes != wc).sum())} bytes differ"
            assert_bits_equal(scales, ws, f"{what} {table} scales kmajor={km}")
            if not km:   # on the rows with a finite y: a NaN element has a code, whose level times an infinite scale is no NaN
                fin = torch.isfinite(y).all(dim=1)
                dec = gemm.dequantize_fp6(codes, scales, table).half()[fin]
                val = produce(table, "values", False).view(rows, C)[fin]
                assert_bits_equal(torch.where(dec == 0, torch.zeros_like(dec), dec), torch.where(val == 0, torch.zeros_like(val), val),
                                  f"{what} {table}: decoded codes against the values")   # (a code has one zero; a value's is signed)


@pytest.mark.parametrize("C", WIDTHS)
@pytest.mark.parametrize("x_dtype", (F16, F32))
def test_plain_rows_every_form(dev, C, x_dtype):
    """1, 3 and 17 rows of every family, with and without smooth, the default and another sign vector, both tables, every emit form in
    both layouts; the spike rows have their maximum where they were built to have it."""
    from fpqvar_amd import rotation as rot
    for n, with_smooth, default_signs in ((1, False, True), (3, True, True), (17, True, False), (17, False, True)):
        x, smooth, where = _rows(C, n, default_signs, with_smooth)
        xd = x.to(x_dtype).to(dev)
        sd = None if smooth is None else smooth.to(dev)
        d = _signs(C, default_signs)
        _, y = rot.rotate_quant_full(xd, "e2m1", d=d, smooth=sd, return_rotated=True)
        out, y2 = rot.rotate_quant_full_token(xd, "e2m3", d=d, smooth=sd, return_rotated=True)
        assert_bits_equal(y2, y, "rotated against rotate_quant_full")
        assert_bits_equal(out, _standalone(y, "e2m3"), "values beside the rotated rows")
        yc = y.float().cpu()
        if "max_last" in where:
            assert int(yc[where["max_last"]].abs().argmax()) == C - 3 and (C - 3) // 8 == C // 8 - 1
        if "max_first" in where:
            assert int(yc[where["max_first"]].abs().argmax()) == 2
        if "zero" in where:
            assert not bool(yc[where["zero"]].any())
        for fam in ("inf", "nan"):
            if fam in where:
                assert not bool(torch.isfinite(yc[where[fam]]).any())
                assert bool(torch.isfinite(yc[where[fam] - 1]).all()) and bool(torch.isfinite(yc[where[fam] + 1]).all())
        _check_all_forms(lambda t, e, km: rot.rotate_quant_full_token(xd, t, d=d, smooth=sd, emit=e, kmajor=km), y, f"rows={n} smooth={with_smooth}")


@pytest.mark.parametrize("C", WIDTHS)
def test_row_scales_of_the_values_form_and_neighbours(dev, C):
    """The values form's row_scales output (reached through the C ABI: the Python function returns values), and every row of the
    17-row launch against a launch of that row alone: a row's scale does not depend on its neighbours."""
    from fpqvar_amd import _lib, gemm, rotation as rot
    x, smooth, where = _rows(C, 17, True, True)
    xd, sd = x.to(dev), smooth.to(dev)
    out, y = rot.rotate_quant_full_token(xd, "e2m3", smooth=sd, return_rotated=True)
    got_out, got_scales = torch.empty_like(out), torch.empty(17, dtype=F16, device=dev)
    words = rot._full_words_arg(None, C)
    _lib.check(_lib.lib().fpq_fullrot_quant_token_rows(xd.data_ptr(), got_out.data_ptr(), None, got_scales.data_ptr(), 17, C, _lib.dtype_id(F32),
                                                       sd.data_ptr(), words, _lib.TABLE_IDS["e2m3"], _lib.stream_ptr(dev)), "values + row_scales")
    torch.cuda.synchronize()
    assert_bits_equal(got_out, out, "values with row_scales asked for")
    assert_bits_equal(got_scales, gemm.quantize_fp6(y, table="e2m3")[1], "row_scales against the stand-alone quantizer's")
    codes, scales = rot.rotate_quant_full_token(xd, "e2m3", smooth=sd, emit="fp6")
    for i in range(17):
        c1, s1 = rot.rotate_quant_full_token(xd[i:i + 1], "e2m3", smooth=sd, emit="fp6")
        assert torch.equal(c1[0], codes[i]), i
        assert_bits_equal(s1[0], scales[i], f"row {i} alone")


@pytest.mark.parametrize("C", WIDTHS)
def test_more_rows_than_the_grid_holds(dev, C):
    """8229 rows: a wavefront owns rows r, r + 4096, r + 8192 in turn, whose magnitudes alternate by 2^10 - a stale image or a stale
    maximum would show in the scales and in every code."""
    from fpqvar_amd import rotation as rot
    rows = 2 * RESIDENT_ROWS + 37
    x, smooth, _ = _rows(C, rows, True, False)
    xd = x.half().to(dev)
    _, y = rot.rotate_quant_full(xd, "e2m1", return_rotated=True)
    amax = y.float().abs().amax(dim=1).cpu()
    assert float(amax[:STEP].min()) > 100 * float(amax[STEP:2 * STEP].max())       # the alternation is there
    _check_all_forms(lambda t, e, km: rot.rotate_quant_full_token(xd, t, emit=e, kmajor=km), y, f"rows={rows}", tables=("e2m3",))


@functools.lru_cache(maxsize=None)
def _adaln_case(C, B, L, x_dtype, mod_dtype):
    g = torch.Generator().manual_seed(77 + C + B * L)
    x = torch.randn(B, L, C, generator=g) * torch.exp(0.5 * torch.randn(B, L, 1, generator=g)) + 0.3 * torch.randn(B, L, 1, generator=g)
    if B * L >= 9:
        x.view(B * L, C)[4, 100] = float("inf")
        x.view(B * L, C)[7, 9] = float("nan")
    sc, sh = torch.randn(B, 1, C, generator=g) * 0.3, torch.randn(B, 1, C, generator=g) * 0.3
    return x.to(x_dtype), sc.to(mod_dtype), sh.to(mod_dtype), torch.rand(C, generator=g) + 0.5


@pytest.mark.parametrize("C", WIDTHS)
@pytest.mark.parametrize("x_dtype", (F16, F32))
def test_adaln_forms(dev, C, x_dtype):
    """(B, L) with batch entries of 1 and 3 rows (their boundaries inside a workgroup's four rows), fp16 and fp32 modulation: h and
    rotated are adaln_rotate_quant_full's, everything behind them the stand-alone quantizer's on those rotated rows."""
    from fpqvar_amd import rotation as rot
    for (B, L), mod_dtype, with_smooth in (((3, 1), F16, True), ((3, 3), F32, False), ((5, 3), F16, False), ((2, 17), F32, True)):
        x, sc, sh, smooth = (t.to(dev) for t in _adaln_case(C, B, L, x_dtype, mod_dtype))
        sd = smooth if with_smooth else None
        _, h, y = rot.adaln_rotate_quant_full(x, sc, sh, "e2m1", smooth=sd, eps=1e-5, return_intermediates=True)
        out, h2, y2 = rot.adaln_rotate_quant_full_token(x, sc, sh, "e2m3", smooth=sd, eps=1e-5, return_intermediates=True)
        assert_bits_equal(h2, h, "h against adaln_rotate_quant_full")
        assert_bits_equal(y2, y, "rotated against adaln_rotate_quant_full")
        y = y.view(B * L, C)
        assert_bits_equal(out.view(B * L, C), _standalone(y, "e2m3"), "values beside the intermediates")
        _check_all_forms(lambda t, e, km: rot.adaln_rotate_quant_full_token(x, sc, sh, t, smooth=sd, eps=1e-5, emit=e, kmajor=km), y,
                         f"adaLN B={B} L={L} {mod_dtype}")


@pytest.mark.parametrize("C", WIDTHS)
def test_adaln_more_rows_than_the_grid_holds(dev, C):
    """8229 = 39 x 211 rows: batch entries of 211 rows, whose boundaries fall inside workgroups and move from one pass over the grid
    to the next; every wavefront takes a second row and some a third."""
    from fpqvar_amd import rotation as rot
    B, L = 39, 211
    x, sc, sh, smooth = (t.to(dev) for t in _adaln_case(C, B, L, F32, F16))
    _, h, y = rot.adaln_rotate_quant_full(x, sc, sh, "e2m1", smooth=smooth, return_intermediates=True)
    out, h2, y2 = rot.adaln_rotate_quant_full_token(x, sc, sh, "e2m3", smooth=smooth, return_intermediates=True)
    assert_bits_equal(h2, h, "h")
    assert_bits_equal(y2, y, "rotated")
    _check_all_forms(lambda t, e, km: rot.adaln_rotate_quant_full_token(x, sc, sh, t, smooth=smooth, emit=e, kmajor=km), y.view(B * L, C),
                     f"adaLN rows={B * L}", tables=("e2m3",))


def test_in_a_captured_graph(dev):
    """values and both operand layouts in ONE linear capture (one stream, no parallel branches); the replay equals eager"""
    from fpqvar_amd import rotation as rot
    C = 2304
    x, sc, sh, smooth = (t.to(dev) for t in _adaln_case(C, 1, 17, F32, F16))

    def run():
        return (rot.adaln_rotate_quant_full_token(x, sc, sh, "e2m3", smooth=smooth),
                *rot.adaln_rotate_quant_full_token(x, sc, sh, "e2m3", smooth=smooth, emit="fp6"),
                *rot.adaln_rotate_quant_full_token(x, sc, sh, "e3m2", smooth=smooth, emit="bf6", kmajor=True),
                rot.rotate_quant_full_token(x, "e3m2"))
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
    for i, (g, e) in enumerate(zip(got, eager)):
        if g.dtype == torch.uint8:
            assert torch.equal(g, e), i
        else:
            assert_bits_equal(g, e, f"output {i} in the graph")


@pytest.mark.parametrize("C", WIDTHS)
@pytest.mark.parametrize("kmajor", (False, True))
def test_end_to_end_into_the_fp6_gemm(dev, C, kmajor):
    """the fused operands and quantize_fp6(rotated) against the same weight operands on gemm.linear_fp6: equal outputs"""
    from fpqvar_amd import gemm, rotation as rot
    x, sc, sh, smooth = (t.to(dev) for t in _adaln_case(C, 2, 17, F32, F16))
    x = torch.where(torch.isfinite(x), x, torch.zeros_like(x))
    g = torch.Generator().manual_seed(3)
    w = (torch.randn(256, C, generator=g) * 0.05).to(dev)
    wc, ws = gemm.quantize_fp6(w)
    if kmajor:
        wc = gemm.to_kmajor(wc, 6, dealt=True)
    bias = (torch.randn(256, generator=g) * 0.1).half().to(dev)
    _, _, y = rot.adaln_rotate_quant_full(x, sc, sh, "e2m1", smooth=smooth, return_intermediates=True)
    got = gemm.linear_fp6(*rot.adaln_rotate_quant_full_token(x, sc, sh, "e2m3", smooth=smooth, emit="fp6", kmajor=kmajor), wc, ws, bias)
    want = gemm.linear_fp6(*gemm.quantize_fp6(y.view(-1, C), kmajor=kmajor), wc, ws, bias)
    assert bool(torch.isfinite(want).all())
    assert_bits_equal(got, want, "linear_fp6 on the fused operands")
    got = gemm.linear_fp6(*rot.rotate_quant_full_token(x, "e3m2", emit="bf6", kmajor=kmajor), wc, ws, bias, a_table="e3m2")
    _, yp = rot.rotate_quant_full(x, "e2m1", return_rotated=True)
    want = gemm.linear_fp6(*gemm.quantize_fp6(yp.view(-1, C), kmajor=kmajor, table="e3m2"), wc, ws, bias, a_table="e3m2")
    assert_bits_equal(got, want, "linear_fp6 on the fused BF6 operands")


@pytest.mark.parametrize("C", WIDTHS)
def test_against_the_reference_op_sequence(dev, C):
    """Reported, not asserted (tests/test_gpu_fulladaln.py reports the same three figures for E2M1): 300 fp32 rows (B = 3, L = 100) of
    the gauss and lognormal families, W6A6.  (d) torch's layer_norm / mul / add_ / mul(smooth) / matmul(Q) under fp16 autocast +
    fp6_quant_e2m3_per_token_cuda - the reference's online side; (e) the oracle's per-token quantizer on half(float64 product of
    half(float64 h)); (f) the fused launch.  Only that the fused values are finite is required."""
    import fpqvar_amd.quant_utils as qu
    from fpqvar_amd import rotation as rot
    from oracle import fpq_oracle as orc
    from tests import fulladaln_model as fa
    from tests import fullrot_model as fm
    x, scale, shift, smooth = fa.make_case(3, 100, C, F32, F16, True, 1e-6, fams=("gauss", "lognormal"))
    ref = fa.reference(x, scale, shift, smooth, 1e-6, 100)
    xd, scd, shd, sd = x.view(3, 100, C).to(dev), scale.view(3, 1, C).to(dev), shift.view(3, 1, C).to(dev), smooth.to(dev)
    ln = torch.nn.functional.layer_norm(xd, (C,), eps=1e-6)
    with torch.autocast("cuda", dtype=torch.float16):
        x1 = torch.matmul(ln.mul(scd.add(1)).add_(shd).mul(sd), rot.get_orthogonal_matrix(C, device=dev).float())
    d = qu.fp6_quant_e2m3_per_token_cuda(x1, 6).cpu().view(300, C)
    e = orc.per_token_kernel_sem(fm.reference(ref["h"].half(), C).half(), "e2m3")
    f = rot.adaln_rotate_quant_full_token(xd, scd, shd, "e2m3", smooth=sd).cpu().view(300, C)

    def agreement(a, b):
        return float((a.view(torch.int16) == b.view(torch.int16)).float().mean())
    print(f"\nfulltoken C={C}: agreement fused/exact {agreement(f, e):.5f}, reference chain/exact {agreement(d, e):.5f}, "
          f"fused/reference chain {agreement(f, d):.5f}")
    assert bool(torch.isfinite(f).all())
