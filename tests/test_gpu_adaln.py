"""The fused LayerNorm + adaLN producer (rotation.adaln_rotate_quant and its operand forms) against the float64 reference and
the per-element bound of tests/adaln_model.py: every row family of the model in ONE launch per case - rows whose mean^2 / var
sits on either side of the kernels' switch to a centred variance, high-mean rows, a constant row, var ~ eps, 1e4 magnitudes,
inf and NaN rows - at every width class of both kernels, fp16 and fp32 rows and modulation, with and without a smoothing
vector, three eps.

(a) the emitting form: h within the bound, non-finite rows exactly the reference's, the rotated row and the values given h
    bit for bit rotate_quant(h)'s (rows wider than 2560: within a derived ulp bound);
(b) every form that runs the same statistics code: bit for bit what (a) gives;
(c) the two forms that sum a second row's statistics in another order (two rows per tile at C = 1024, the paired slot at
    C = 2176 / 2304, fp16 rows): per group of 128 either bit-equal to (a) or scale and levels adjacent to (a)'s."""
import itertools

import pytest
import torch

from oracle import fpq_oracle as orc
from tests import adaln_model as am
from tests import gemm_model as gm

pytestmark = pytest.mark.gpu

MFMA_WIDTHS = (128, 1024, 1152, 1920, 2304, 2560)      # MAXC 1 .. 5, the slot partly (2304) and fully (2560) used
WIDE_WIDTHS = (2688, 3072, 3968, 4096)                 # one workgroup per row, padded and not
OTHER_ORDER = (1024, 2176, 2304)                       # fp16 rows: the values / FP4-operand forms of (c)
B = 4
F16, F32 = torch.float16, torch.float32
E2M1_SORTED = (-6.0, -4.0, -3.0, -2.0, -1.5, -1.0, -0.5, 0.0, 0.5, 1.0, 1.5, 2.0, 3.0, 4.0, 6.0)


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "these tests need the GPU"
    return torch.device("cuda:0")


def _case(dev, L, C, x_dtype, mod_dtype, with_smooth, eps, fams=am.FAMILIES):
    x, scale, shift, smooth = am.make_case(B, L, C, x_dtype, mod_dtype, with_smooth, eps, fams=fams)
    x, scale, shift = x.to(dev), scale.to(dev), shift.to(dev)
    smooth = smooth.to(dev) if smooth is not None else None
    return x, scale, shift, smooth


def _emit(x, scale, shift, smooth, eps, L, table="e2m1"):
    from fpqvar_amd import rotation as rot
    C = x.shape[1]
    out, h, y = rot.adaln_rotate_quant(x.view(B, L, C), scale, shift, table, smooth=smooth, eps=eps, return_intermediates=True)
    return out.view(-1, C), h.view(-1, C), y.view(-1, C)


def _bits(t):
    """fp16 -> int16 bit patterns with every NaN one value"""
    return torch.where(torch.isnan(t), torch.full_like(t, float("nan")), t).view(torch.int16)


def _rows_differ(got, want):
    """indices of the rows of two fp16 [R, C] tensors that are not bit-equal (every NaN one value)"""
    assert got.shape == want.shape and got.dtype == want.dtype == F16, (got.shape, want.shape, got.dtype, want.dtype)
    return (_bits(got) != _bits(want)).any(dim=1).nonzero().flatten().tolist()


def _name(rows, R, C):
    fams = am.families(R, C)
    return sorted({fams[r] for r in rows})


def _ulp_diff_f16(a, b):
    ai, bi = a.view(torch.int16).to(torch.int32), b.view(torch.int16).to(torch.int32)
    ai = torch.where(ai < 0, -(ai & 0x7FFF), ai)
    bi = torch.where(bi < 0, -(bi & 0x7FFF), bi)
    return (ai - bi).abs()


def _kernel_key(C, x_dtype):
    return "wide" if C > am.WIDE_FROM else "adaln_mfma fp16" if x_dtype == F16 else "adaln_mfma fp32"


ALL_OPTIONS = tuple(itertools.product((1, 23), (F16, F32), (F16, F32), (False, True), (1e-6, 1e-5, 1e-2)))


def _what(L, x_dtype, mod_dtype, with_smooth, eps):
    return f"L={L} x={str(x_dtype)[6:]} mod={str(mod_dtype)[6:]} smooth={with_smooth} eps={eps}"


@pytest.mark.parametrize("C", MFMA_WIDTHS + WIDE_WIDTHS + (2176,))
def test_emitting_form_against_the_float64_reference(dev, C):
    """(a): h within adaln_model.bound of adaln_model.reference on every finite element; non-finite elements exactly where the
    reference has them (a non-finite input poisons its row and no other); the values are the oracle's quantization of the
    emitted rotated row.
    Measured on an MI355X, worst err / bound over all of this test: adaln_mfma_kernel fp16 rows 0.999, fp32 rows 0.999,
    adaln_rotate_quant16_kernel 0.999 (the fp16 rounding of h is nearly all of the bound on most elements).  The same kernel
    before padding lanes were kept out of its centred sum: 4.2 at C = 2688, 31.2 at 3072, 2.9 at 3968, 0.999 at 4096."""
    worst, bad = {}, []
    for L, x_dtype, mod_dtype, with_smooth, eps in ALL_OPTIONS:
        x, scale, shift, smooth = _case(dev, L, C, x_dtype, mod_dtype, with_smooth, eps)
        R = B * L
        what = _what(L, x_dtype, mod_dtype, with_smooth, eps)
        out, h, y = _emit(x, scale, shift, smooth, eps, L)
        ref = am.reference(x, scale, shift, smooth, eps, L)
        assert float(ref["h"][ref["finite"]].abs().max()) < 6.0e4
        err = (h.double() - ref["h"]).abs() / am.bound(ref, x_dtype, C)
        err = torch.nan_to_num(err, nan=float("inf"))[ref["finite"]]
        per_row = err.max(dim=1).values
        key = _kernel_key(C, x_dtype)
        worst[key] = max(worst.get(key, 0.0), float(per_row.max()))
        if float(per_row.max()) > 1.0:
            rows = ref["finite"].nonzero().flatten()[per_row > 1.0].tolist()
            bad.append((what, "h beyond the bound", round(float(per_row.max()), 2), _name(rows, R, C)))
        if not torch.equal(torch.isfinite(h), torch.isfinite(ref["h"])):
            bad.append((what, "non-finite elements are not where the reference has them"))
        if L == 23 and with_smooth and eps == 1e-5:
            want = orc.per_group_kernel_sem(y.cpu(), "e2m1", 128).to(out.device)
            if _rows_differ(out, want):
                bad.append((what, "values != oracle quantization of the rotated row", _name(_rows_differ(out, want), R, C)))
    print(f"\nC={C}: worst err / bound " + ", ".join(f"{k} {v:.3f}" for k, v in sorted(worst.items())))
    assert not bad, f"{len(bad)} failures, first {bad[:6]}"


@pytest.mark.parametrize("C", MFMA_WIDTHS + WIDE_WIDTHS)
def test_emitting_form_rotates_and_quantizes_as_rotate_quant(dev, C):
    """(a), given h: the rotated row and the values equal rotate_quant(h, return_rotated=True) bit for bit.  Rows wider than 2560
    rotate by fp32 butterflies where rotate_quant uses the matrix cores: there each element is within one fp16 ulp plus the two
    transforms' fp32 summation error (7 butterfly stages: 14 * 2^-24 * sum|h_i| / sqrt(128) per group; one ulp on all but
    cancelling outputs), and fewer than 1e-3 of the elements differ at all - what test_adaln_rotate_quant_wide_rows asserts.

    At C <= 2560 that covers groups 16 .. 19 of a row of 17 .. 20 groups (the slot chunk of adaln_mfma_kernel): while they were
    rotated by fp32 butterflies, 5 of 5 308 416 rotated elements at C = 2304 (1 of 5 013 504 at C = 2176), all in groups 16 / 17,
    were one fp16 ulp off rotate_quant(h) - both sides 0.48 .. 0.52 ulp from the float64 product; the slot now takes the tile's
    matrix-core transform and 0 differ.  Rows wider than 2560, measured: 8 .. 11 of 6 .. 9 million elements differ."""
    from fpqvar_amd import rotation as rot
    bad, n_el, n_diff = [], 0, 0
    for L, x_dtype, mod_dtype, with_smooth, eps in ALL_OPTIONS:
        x, scale, shift, smooth = _case(dev, L, C, x_dtype, mod_dtype, with_smooth, eps)
        R = B * L
        what = _what(L, x_dtype, mod_dtype, with_smooth, eps)
        out, h, y = _emit(x, scale, shift, smooth, eps, L)
        out2, y2 = rot.rotate_quant(h, "e2m1", return_rotated=True)
        n_el += y.numel()
        n_diff += int((_bits(y) != _bits(y2)).sum())
        if C > am.WIDE_FROM:
            fin = torch.isfinite(h).all(dim=1)
            slack = 14 * am.U * h.double().abs().view(R, -1, 128).sum(dim=2, keepdim=True).expand(R, C // 128, 128).reshape(R, C) / 128 ** 0.5
            d = (y.double() - y2.double()).abs()[fin]
            lim = (torch.maximum(am.ulp16(y.double()), am.ulp16(y2.double())) + slack)[fin]
            share = float((_bits(y) != _bits(y2)).float().mean())
            if not bool((d <= lim).all()) or share >= 1e-3 or not torch.equal(torch.isnan(y), torch.isnan(y2)):
                bad.append((what, "rotated: butterfly vs matrix cores", float((d / lim).max()), share))
        else:
            if _rows_differ(y, y2):
                bad.append((what, "rotated row != rotate_quant(h)", _name(_rows_differ(y, y2), R, C)))
            if _rows_differ(out, out2):
                bad.append((what, "values != rotate_quant(h)", _name(_rows_differ(out, out2), R, C)))
    print(f"\nC={C}: {n_diff} of {n_el} rotated elements differ from rotate_quant(h)")
    assert not bad, f"{len(bad)} failures, first {bad[:6]}"


def _forms(x3, scale, shift, smooth, eps, C, x_dtype, skip_other_order):
    """(name, values fp16 [R, C], reference key) of every non-emitting form at this width; the reference key names which of
    (a)'s outputs it must equal: a table name = the emitting form's values in that table, ("token", table) = the per-token
    quantization of (a)'s rotated row."""
    from fpqvar_amd import gemm, rotation as rot
    R = x3.shape[0] * x3.shape[1]
    kw = dict(smooth=smooth, eps=eps)
    forms = []
    paired = skip_other_order and x_dtype == F16 and C in OTHER_ORDER
    if not paired:
        forms.append(("values e2m1", lambda: rot.adaln_rotate_quant(x3, scale, shift, "e2m1", **kw).view(R, C), "e2m1"))

        def mx():
            codes, scales = rot.adaln_rotate_quant_mx(x3, scale, shift, **kw)
            return gemm.dequantize_mx(codes.view(R, -1), scales.view(R, -1)).half()
        forms.append(("mx", mx, "e2m1"))
        if C <= am.WIDE_FROM:
            def mx_km():
                codes, scales = rot.adaln_rotate_quant_mx(x3, scale, shift, kmajor=True, **kw)
                return gemm.dequantize_mx(gm.from_kmajor(codes, 4, R), scales[:, :R].t().contiguous()).half()
            forms.append(("mx k-major", mx_km, "e2m1"))
        forms.append(("values e2m3", lambda: rot.adaln_rotate_quant(x3, scale, shift, "e2m3", **kw).view(R, C), "e2m3"))
    if C <= am.WIDE_FROM:
        if not paired:   # (the table form of the values runs the paired kernels too)
            forms.append(("values e3m0", lambda: rot.adaln_rotate_quant(x3, scale, shift, "e3m0", **kw).view(R, C), "e3m0"))
        forms.append(("token e2m3", lambda: rot.adaln_rotate_quant_token(x3, scale, shift, "e2m3", **kw).view(R, C), ("token", "e2m3")))

        def tok8():
            codes, scales = rot.adaln_rotate_quant_token(x3, scale, shift, "e2m3", emit="fp8", **kw)
            return gemm.dequantize_fp8(codes, scales).half()
        forms.append(("token fp8 codes", tok8, ("token", "e2m3")))
        for km in (False, True):
            def tok6(km=km):
                codes, scales = rot.adaln_rotate_quant_token(x3, scale, shift, "e2m3", emit="fp6", kmajor=km, **kw)
                return gemm.dequantize_fp6(gm.from_kmajor(codes, 6, R) if km else codes, scales).half()
            forms.append(("token fp6 codes" + (" k-major" if km else ""), tok6, ("token", "e2m3")))
            def g6(km=km):
                codes, scales = rot.adaln_rotate_quant_g6(x3, scale, shift, "e3m0", kmajor=km, **kw)
                if km:
                    return gemm.dequantize_g6(gm.from_kmajor(codes, 6, R), scales[:, :R].t().contiguous(), "e3m0").half()
                return gemm.dequantize_g6(codes, scales, "e3m0").half()
            forms.append(("g6 e3m0" + (" k-major" if km else ""), g6, "e3m0"))
    return forms


SAME_STATS_CASES = tuple((23, xd, md, True, 1e-5) for xd in (F16, F32) for md in (F16, F32)) + ((1, F16, F32, False, 1e-2), (1, F32, F16, False, 1e-6))


@pytest.mark.parametrize("C", MFMA_WIDTHS + WIDE_WIDTHS)
def test_forms_with_the_same_statistics_code_equal_the_emitting_form(dev, C):
    """(b): values without the intermediates, per-token values and codes, FP4 operands, 6-bit group operands, row-major and as
    k-major images - decoded (dequantize_*, from_kmajor) they are bit for bit what the emitting form's rotated row quantizes to,
    on every row family; fp32 rows in every form, fp16 rows in every form but the two of (c).  The statistics code is shared:
    the options of (a) - eps, smoothing, modulation dtype - are run here in one combination each."""
    from fpqvar_amd import ops
    bad = []
    for L, x_dtype, mod_dtype, with_smooth, eps in SAME_STATS_CASES:
        x, scale, shift, smooth = _case(dev, L, C, x_dtype, mod_dtype, with_smooth, eps)
        R = B * L
        what = f"L={L} x={str(x_dtype)[6:]} mod={str(mod_dtype)[6:]}"
        want, h0 = {}, None
        for name, fn, key in _forms(x.view(B, L, C), scale, shift, smooth, eps, C, x_dtype, True):
            if key not in want:
                if isinstance(key, tuple):
                    y = _emit(x, scale, shift, smooth, eps, L)[2]
                    want[key] = ops.quant_rows(y, key[1], C, F16)
                else:
                    out, h, _ = _emit(x, scale, shift, smooth, eps, L, key)
                    h0 = h if h0 is None else h0
                    if _rows_differ(h, h0):
                        bad.append((what, f"emitting form, table {key}: another h", _name(_rows_differ(h, h0), R, C)))
                    want[key] = out
            rows = _rows_differ(fn(), want[key])
            if rows:
                bad.append((what, name, f"{len(rows)} rows", _name(rows, R, C)))
    assert not bad, f"{len(bad)} failures, first {bad[:8]}"


def _level_index(codes):
    """E2M1 nibbles [R, C/2] -> position of each element's level among the 15 distinct values, [R, C]"""
    lv = gm.decode("fp4", codes.cpu())                                        # float64 levels
    tab = torch.tensor(E2M1_SORTED, dtype=torch.float64)
    return torch.bucketize(lv, tab)


@pytest.mark.parametrize("C", OTHER_ORDER)
def test_forms_that_sum_a_second_row_in_another_order(dev, C):
    """(c): fp16 rows at C = 1024 (two rows per tile: either row's cancellation centres both, with one accumulator) and at
    C = 2176 / 2304 (every second row of a wavefront has its slot chunk on lanes 32 .. 63): the LayerNorm sums of such a row
    round in another order than the emitting form's, so its h may differ in the last bit of rare elements.  Per group of 128:
    bit-equal to (a), or its scale within 2 fp16 ulps of (a)'s and every level at most one step from (a)'s.  The values form is
    bit for bit the decoded FP4 operands.  On gauss and log-normal rows at most 1 % of the groups are not bit-equal (the model's
    two orders stay under 0.25 %: test_adaln_model_host.py).
    Measured on an MI355X: C = 1024: 2 of 2272 groups not bit-equal, both on a row with rho^2 = 57.6 whose partner centres the
    pair; C = 2176: 0 of 4828; C = 2304: 0 of 5112; on gauss and log-normal rows 0 of 1016 / 2108 / 2268."""
    from fpqvar_amd import gemm, rotation as rot
    bad, total, differ = [], 0, 0
    for L, mod_dtype, with_smooth, eps, fams in ((23, F16, True, 1e-5, am.FAMILIES), (23, F32, False, 1e-6, am.FAMILIES),
                                                 (1, F16, True, 1e-2, am.FAMILIES), (24, F16, True, 1e-6, am.SHARE_CAPPED)):
        x, scale, shift, smooth = _case(dev, L, C, F16, mod_dtype, with_smooth, eps, fams)
        R, G = B * L, C // 128
        what = f"L={L} mod={str(mod_dtype)[6:]} smooth={with_smooth}" + (" (gauss and log-normal rows only)" if fams is am.SHARE_CAPPED else "")
        out_a, h_a, _ = _emit(x, scale, shift, smooth, eps, L)
        codes_a, scales_a = rot.rotate_quant_mx(h_a)                          # (a)'s operands: bit-exact given h
        if _rows_differ(gemm.dequantize_mx(codes_a, scales_a).half(), out_a):
            bad.append((what, "rotate_quant_mx(h) does not decode to the emitting form's values"))
        codes, scales = rot.adaln_rotate_quant_mx(x.view(B, L, C), scale, shift, smooth=smooth, eps=eps)
        codes, scales = codes.view(R, -1), scales.view(R, -1)
        vals = rot.adaln_rotate_quant(x.view(B, L, C), scale, shift, "e2m1", smooth=smooth, eps=eps).view(R, C)
        if _rows_differ(vals, gemm.dequantize_mx(codes, scales).half()):
            bad.append((what, "values != decoded operands"))
        same = (codes.view(R, G, 64) == codes_a.view(R, G, 64)).all(dim=2) & (_bits(scales) == _bits(scales_a))
        same = (same | (torch.isnan(scales) & torch.isnan(scales_a))).cpu()   # a NaN scale: the group decodes to NaN whatever its codes
        sc_ok = (_ulp_diff_f16(torch.nan_to_num(scales), torch.nan_to_num(scales_a)) <= 2) & (torch.isnan(scales) == torch.isnan(scales_a))
        lv_ok = ((_level_index(codes) - _level_index(codes_a)).abs() <= 1).view(R, G, 128).all(dim=2)
        ok = same | (sc_ok.cpu() & lv_ok)
        names = am.families(R, C, fams)
        if not bool(ok.all()):
            bad.append((what, "a group neither bit-equal nor adjacent", sorted({names[r] for r in (~ok).any(dim=1).nonzero().flatten().tolist()})))
        capped = torch.tensor([f in am.SHARE_CAPPED for f in names])
        total += int(capped.sum()) * G
        differ += int((~same[capped]).sum())
        print(f"\nC={C} {what}: groups not bit-equal: {int((~same).sum())} of {same.numel()}, by family "
              f"{ {f: int((~same[[i for i, g in enumerate(names) if g == f]]).sum()) for f in sorted(set(names))} }")
    print(f"C={C}: gauss / log-normal groups not bit-equal {differ} of {total}")
    assert not bad, f"{len(bad)} failures, first {bad[:6]}"
    assert differ <= 0.01 * total, f"{differ} of {total} gauss / log-normal groups are not bit-equal"
