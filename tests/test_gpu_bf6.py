"""BF6 (E3M2) operands on the FP6 matrix-core path, alone and mixed with E2M3: the quantizers that emit them, the GEMM's two
format selectors, the split / q-k-norm epilogues and the modules on top (include/fpq.h, version 130).

Reference and bound are tests/gemm_model.py's, unchanged: every level of both 6-bit tables is an E4M3 number, so a helper here
maps dense 6-bit codes of either format to E4M3 bytes and back and gm.reference("fp8", ...) / gm.bound / gm.ratio /
gm.class_mismatch serve as they are.  Where a side holds E3M2 levels the allowance is gm.WIDE_FP8_MEASURED x the bound - the
project's figure for these levels on this matrix instruction (include/fpq.h) - and 1.0 x the bound for E2M3 x E2M3."""
import contextlib
import copy

import pytest
import torch

from oracle import fpq_oracle as orc
from tests import gemm_model as gm
from tests.conftest import assert_bits_equal
from tests.test_gpu_qk_l2norm import _assert_ulp, _bias, _reference, _scale_mul

pytestmark = pytest.mark.gpu

TABLES = ("e2m3", "e3m2")
PAIRS = (("e2m3", "e2m3"), ("e3m2", "e2m3"), ("e2m3", "e3m2"), ("e3m2", "e3m2"))      # (activations, weights)
BF6_PAIRS = PAIRS[1:]


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "these tests need the GPU"
    return torch.device("cuda:0")


# ------------------------------------------------------------------------------------------------ codes of either format
def _values(table):
    """float64 value of the 64 codes: sign bit 5; e2m3: 2 exponent bits (bias 1), 3 mantissa bits; e3m2: 3 (bias 3), 2"""
    eb, mb, bias = (2, 3, 1) if table == "e2m3" else (3, 2, 3)
    v = []
    for c in range(64):
        e, m = (c >> mb) & ((1 << eb) - 1), c & ((1 << mb) - 1)
        mag = m / (1 << mb) * 2.0 ** (1 - bias) if e == 0 else (1 + m / (1 << mb)) * 2.0 ** (e - bias)
        v.append(-mag if c & 32 else mag)
    return torch.tensor(v, dtype=torch.float64)


E3M2_LEVELS = torch.sort(_values("e3m2")[:32]).values            # 0, 1/16 .. 28


def _unpack6(codes):
    """dense 6-bit codes [rows, 3K/4] -> code indices [rows, K] (element j in bits 6j .. 6j + 5 of the row's bit string)"""
    b = codes.long().reshape(codes.shape[0], -1, 3)
    word = b[..., 0] | (b[..., 1] << 8) | (b[..., 2] << 16)
    return torch.stack([(word >> (6 * j)) & 63 for j in range(4)], dim=-1).reshape(codes.shape[0], -1)


def _lut_to_e4m3(table):
    return gm._to_idx("fp8", _values(table)).to(torch.uint8)    # (code 32, -0: the byte of +0, as the FP8 quantizer emits it)


def f6_to_e4m3(codes, table):
    """dense 6-bit codes of `table` -> one E4M3 byte per element, same values"""
    return _lut_to_e4m3(table).to(codes.device)[_unpack6(codes)]


def e4m3_to_f6(bytes8, table):
    """E4M3 bytes holding levels of `table` -> its dense 6-bit codes"""
    inv = torch.full((256,), -1, dtype=torch.long)
    lut = _lut_to_e4m3(table).long()
    for c in list(range(1, 32)) + list(range(33, 64)) + [0]:    # (both zero codes map to byte 0: byte 0 -> code 0)
        inv[lut[c]] = c
    idx = inv.to(bytes8.device)[bytes8.long()]
    assert int(idx.min()) >= 0, f"an E4M3 byte that is no {table} level"
    return gm.encode("fp6", idx)


def _levels_to_f6(levels, table):
    """exact level values (of both tables or of `table`) -> dense codes; zero of either sign -> code 0"""
    vals = _values(table)
    order = torch.argsort(vals[:32])
    i = torch.searchsorted(vals[:32][order], levels.abs().double().contiguous())
    idx = order[i.clamp(max=31)]
    assert torch.equal(vals[idx], levels.abs().double()), "not a level of the table"
    return gm.encode("fp6", torch.where(levels < 0, idx + 32, idx))


def test_code_maps_are_consistent():
    """the helper itself: values, the E4M3 map and its inverse, against gemm.dequantize_fp6 and gm's E4M3 decoder"""
    from fpqvar_amd import gemm
    all64 = gm.encode("fp6", torch.arange(64).view(1, 64))
    for table in TABLES:
        v = _values(table)
        assert torch.equal(gemm.dequantize_fp6(all64, torch.ones(1), table).double().view(64), v)
        b = f6_to_e4m3(all64, table)
        assert torch.equal(gm.decode("fp8", b).view(64), v)
        back = _unpack6(e4m3_to_f6(b, table)).view(64)
        want = torch.arange(64)
        want[32] = 0
        assert torch.equal(back, want)
    assert torch.equal(torch.sort(_values("e3m2")).values.float(), torch.sort(orc.TABLES["e3m2"]).values)


# ------------------------------------------------------------------------------------------------ 1. quantizer parity
def _rows(rows, cols, dtype, seed):
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(rows, cols, generator=g) * torch.exp(0.5 * torch.randn(rows, cols, generator=g))
    x[0] = 0
    if rows > 3:
        x[1, cols // 3] = float("inf")
        x[2, 5] = float("-inf")
        x[3, cols - 1] = float("nan")
    return x.to(dtype)


@pytest.mark.parametrize("dtype", (torch.float16, torch.float32))
def test_quantizer_parity(dev, dtype):
    """table="e3m2": the decisions of fpq_quant_rows(.., FPQ_E3M2) and of the oracle, the bytes of the FP8 emitter, the k-major
    image.  fp16 rows of 9216 and every fp32 row take the generic kernel, an unaligned fp16 base pointer too."""
    from fpqvar_amd import gemm, ops
    for rows, cols in ((70, 1920), (9, 2304), (6, 7680), (5, 9216), (7, 64), (12, 128), (5, 4096), (4, 8192)):
        x = _rows(rows, cols, dtype, 71 + cols)
        xd = x.to(dev)
        codes, scales = gemm.quantize_fp6(xd, table="e3m2")
        assert codes.shape == (rows, cols * 3 // 4) and codes.dtype == torch.uint8 and scales.shape == (rows,) and scales.dtype == dtype
        got = gemm.dequantize_fp6(codes, scales, "e3m2")
        want = ops.quant_rows(xd, "e3m2", cols, torch.float32)
        ok = ~torch.isnan(want)
        assert_bits_equal(got[ok], want[ok], f"bf6 codes vs quant_rows {cols}")
        assert bool(torch.isnan(got[~ok]).all())
        assert_bits_equal(got.cpu(), orc.per_token_kernel_sem(x, "e3m2", out_dtype=torch.float32), f"bf6 codes vs the oracle {cols}")
        c8, s8 = gemm.quantize_fp8(xd, "e3m2")
        assert torch.equal(f6_to_e4m3(codes, "e3m2"), c8), f"bf6 codes vs the E4M3 bytes {cols}"
        assert_bits_equal(scales, s8, f"scales {cols}")
        if cols % 128 == 0:
            image, s_km = gemm.quantize_fp6(xd, kmajor=True, table="e3m2")
            assert image.shape == (cols // 128, rows, 96) and torch.equal(image, gemm.to_kmajor(codes, 6)), f"k-major image {cols}"
            assert_bits_equal(s_km, scales, f"k-major scales {cols}")
        # the same input as E2M3: unchanged, and different codes
        c3, s3 = gemm.quantize_fp6(xd)
        assert torch.equal(c3, gemm.quantize_fp6(xd, table="fp6_e2m3")[0])
        assert rows <= 4 or not torch.equal(c3, codes)      # (rows 0 .. 3 are the zero / inf / NaN rows)
    xu = _rows(6, 256 + 8, torch.float16, 64).reshape(-1).to(dev)[4:4 + 6 * 256].view(6, 256)      # 8 bytes off a 16-byte boundary
    c, s = gemm.quantize_fp6(xu[:, :], table="e3m2")
    w = ops.quant_rows(xu, "e3m2", 256, torch.float32)
    ok = ~torch.isnan(w)
    assert_bits_equal(gemm.dequantize_fp6(c, s, "e3m2")[ok], w[ok], "bf6 generic path, unaligned fp16")
    with pytest.raises(RuntimeError):
        gemm.quantize_fp6(xu, table="e2m1")


@pytest.mark.parametrize("C", (128, 640, 1024, 1920, 2048, 2304))
@pytest.mark.parametrize("x_dtype", (torch.float16, torch.float32))
def test_adaln_producer_emits_bf6(dev, C, x_dtype, monkeypatch):
    """emit="bf6" == quantize_fp6(y, table="e3m2") on the rotated rows y, row-major and k-major, with and without smooth, the
    compiled binding and ctypes giving the same bytes; emit="fp6" keeps refusing E3M2, emit="bf6" refuses E2M3"""
    from fpqvar_amd import gemm, rotation as rot
    assert rot._native is not None, "the compiled binding did not load"
    g = torch.Generator().manual_seed(C + 3)
    B, L = 3, 19
    x = (torch.randn(B, L, C, generator=g) * 2 + 0.3).to(x_dtype).to(dev)
    scale = (torch.randn(B, 1, C, generator=g) * 0.3).half().to(dev)
    shift = (torch.randn(B, 1, C, generator=g) * 0.3).half().to(dev)
    for smooth in (None, (torch.rand(C, generator=g) * 1.5 + 0.25).to(dev)):
        _, _, y = rot.adaln_rotate_quant(x, scale, shift, "e2m1", smooth=smooth, return_intermediates=True)   # rotated fp16 rows
        y = y.reshape(B * L, C)
        for kmajor in (False, True):
            want_c, want_s = gemm.quantize_fp6(y, kmajor=kmajor, table="e3m2")
            outs = []
            for front in ("native", "ctypes"):
                with monkeypatch.context() as mp:
                    if front == "ctypes":
                        mp.setattr(rot, "_native", None)
                    outs.append(rot.adaln_rotate_quant_token(x, scale, shift, "e3m2", smooth=smooth, emit="bf6", kmajor=kmajor))
            for front, (c, s) in zip(("native", "ctypes"), outs):
                what = f"{front} C={C} kmajor={kmajor} smooth={smooth is not None}"
                assert c.shape == ((C // 128, B * L, 96) if kmajor else (B * L, C * 3 // 4)) and s.dtype == torch.float16, what
                assert torch.equal(c, want_c), f"codes, {what}"
                assert torch.equal(s.view(torch.int16), want_s.view(torch.int16)), f"scales, {what}"
    for front in ("native", "ctypes"):
        with monkeypatch.context() as mp:
            if front == "ctypes":
                mp.setattr(rot, "_native", None)
            with pytest.raises(RuntimeError):
                rot.adaln_rotate_quant_token(x, scale, shift, "e3m2", emit="fp6")
            with pytest.raises(RuntimeError):
                rot.adaln_rotate_quant_token(x, scale, shift, "e2m3", emit="bf6")
            with pytest.raises(RuntimeError):
                rot.adaln_rotate_quant_token(x, scale, shift, "e3m2", emit="fp8", kmajor=True)


# ------------------------------------------------------------------------------------------------ the GEMM through every form
def _runs(gemm, lib_options, a, sa, w, sw, bias, ta, tw, ctypes_e2m3=False):
    """[(what, out)]: FPQ_GEMM6_CFG 0 / 1 x row-major codes / k-major images"""
    img_a, img_w = gemm.to_kmajor(a, 6), gemm.to_kmajor(w, 6, dealt=True)
    out = []
    for cfg in (0, 1):
        lib_options("FPQ_GEMM6_CFG", cfg)
        out.append((f"row-major cfg {cfg}", _linear(gemm, a, sa, w, sw, bias, ta, tw, ctypes_e2m3)))
        out.append((f"k-major cfg {cfg}", _linear(gemm, img_a, sa, img_w, sw, bias, ta, tw, ctypes_e2m3)))
    lib_options("FPQ_GEMM6_CFG", None)
    return out


def _linear(gemm, a, sa, w, sw, bias, ta, tw, through_f6_entry=False):
    """gemm.linear_fp6 of the pair; through_f6_entry: fpq_gemm_f6_rows itself (linear_fp6 sends E2M3 x E2M3 to the entry points it
    always used)"""
    if not through_f6_entry:
        return gemm.linear_fp6(a, sa, w, sw, bias, a_table=ta, w_table=tw)
    from fpqvar_amd._lib import TABLE_IDS, check, dtype_id, lib, stream_ptr
    km = a.dim() == 3
    tokens, outs, k = (a.shape[1], sw.shape[0], a.shape[0] * 128) if km else (a.shape[0], w.shape[0], a.shape[1] * 4 // 3)
    out = torch.empty((tokens, outs), dtype=torch.float16, device=a.device)
    b = None if bias is None else bias.half().contiguous()
    check(lib().fpq_gemm_f6_rows(a.data_ptr(), sa.data_ptr(), dtype_id(sa.dtype), TABLE_IDS[ta], w.data_ptr(), sw.data_ptr(), dtype_id(sw.dtype),
                                 TABLE_IDS[tw], None if b is None else b.data_ptr(), out.data_ptr(), tokens, outs, k, None, 1 if km else 0,
                                 stream_ptr(a.device)), "fpq_gemm_f6_rows")
    return out


def _same_bits(x, y):
    """bit-equal, every NaN one value"""
    xn, yn = torch.isnan(x), torch.isnan(y)
    return bool(torch.equal(xn, yn)) and bool(torch.equal(x.masked_fill(xn, 0).view(torch.int16), y.masked_fill(yn, 0).view(torch.int16)))


# ------------------------------------------------------------------------------------------------ 2. selectors and layout, exactly
EXACT_SHAPES = {(1, 8), (17, 136), (65, 128), (128, 128), (129, 392), (255, 8), (257, 120), (300, 1928), (63, 5760), (1000, 5760),
                (4097, 6912)}
COMMON = torch.tensor([0.0, 0.25, 0.5, 1.0, 2.0, 4.0], dtype=torch.float64)      # levels of both tables


def test_format_selectors_and_operand_layout_exactly(dev, lib_options):
    """Operands whose levels are 0 and +-{1/4, 1/2, 1, 2, 4} only - in both tables, with DIFFERENT codes (E2M3 1.0 is code 8,
    E3M2 1.0 is code 12) - signs and positions random and different on the two sides, sa = 2^-2, sw = 2^-4, no bias.  Every product
    is a multiple of 2^-4 and every partial sum is below 16 K < 2^18: fp32 holds each of them in any order and the scaling is exact,
    so the output is ONE rounding of the float64 reference, ref64.float().half(), for all four format pairs, both tilings, both
    layouts.  A selector that decodes a side with the other format, or cbsz / blgp exchanged in a mixed pair, changes values."""
    from fpqvar_amd import gemm
    shapes = [(T, O, K) for _, T, O, K in gm.shape_sweep() if (T, O) in EXACT_SHAPES]
    assert len(shapes) == len(EXACT_SHAPES) and any(K == 128 for _, _, K in shapes) and sum(K >= 1920 for _, _, K in shapes) >= 4
    assert any(T >= 4096 and O >= 4096 for T, O, _ in shapes) and any(T % 128 and O % 128 for T, O, _ in shapes)
    bad = []
    for T, O, K in shapes:
        g = torch.Generator().manual_seed(T * 31 + O * 7 + K)
        draw = lambda n: COMMON[torch.randint(0, 6, (n, K), generator=g)] * torch.where(torch.rand(n, K, generator=g) < 0.5, -1.0, 1.0).double()
        La, Lw = draw(T), draw(O)
        sa = torch.full((T,), 2.0 ** -2, dtype=torch.float16, device=dev)
        sw = torch.full((O,), 2.0 ** -4, dtype=torch.float32, device=dev)
        bytes_a, bytes_w = gm.encode("fp8", gm._to_idx("fp8", La)).to(dev), gm.encode("fp8", gm._to_idx("fp8", Lw)).to(dev)
        r = gm.reference("fp8", bytes_a, sa, bytes_w, sw, None)
        assert float(r.out.abs().max()) <= 16.0 * K * 2.0 ** -6
        want = r.out.float().half()
        assert torch.equal(want.double(), r.out.float().double().half().double())
        for ta, tw in PAIRS:
            a, w = _levels_to_f6(La, ta).to(dev), _levels_to_f6(Lw, tw).to(dev)
            assert torch.equal(gemm.dequantize_fp6(a, torch.ones(T, device=dev), ta).double().cpu(), La.where(La != 0, torch.zeros_like(La)))
            for what, y in _runs(gemm, lib_options, a, sa, w, sw, None, ta, tw, ctypes_e2m3=(ta, tw) == PAIRS[0]):
                same = (y.view(torch.int16) == want.view(torch.int16)) | ((y == 0) & (want == 0))      # every element
                if not bool(same.all()):
                    bad.append((ta, tw, what, T, O, K, int((~same).sum())))
    assert not bad, f"{len(bad)} runs differ from the one-rounding reference, first {bad[:6]}"


# ------------------------------------------------------------------------------------------------ 3. full-range codes vs float64
FULL_SHAPES = ((1, 8, 128), (17, 136, 256), (129, 392, 1920), (300, 1928, 2304), (64, 128, 7680), (257, 120, 9216))
CONSTRUCTIONS = ("e3m2", "max_codes", "zero", "subnormal", "bias_cancel", "non_finite")      # "e3m2": gm's gaussian E3M2 levels


@contextlib.contextmanager
def _e3m2_value_set():
    """gm.make_case("fp8", family, ..) draws a family's levels from gm._value_set - E2M3 for every family but "e3m2" / "e4m3_full".
    Inside this block that set is E3M2's (0, 1/16 .. 28), so that make_case's constructions (max_codes: 28 against 28 and 1/16; zero;
    subnormal; bias_cancel; non_finite) are drawn on E3M2 levels, as E4M3 bytes.  gemm_model.py itself is not changed."""
    real = gm._value_set
    gm._value_set = lambda kind, family: E3M2_LEVELS.clone()
    try:
        yield
    finally:
        gm._value_set = real


def _full_case(family, T, O, K, ta, tw, dev):
    """operands of one (construction, shape, pair): an E3M2 side comes from the E3M2 draw of the construction (bias too), an E2M3 side
    from gm.make_case("fp6", ..) of the same T, O, K -> (a, sa, w, sw, bias) as dense codes, and the same as E4M3 bytes"""
    if family == "e3m2":
        c8 = gm.make_case("fp8", "e3m2", T, O, K)
        c6 = gm.make_case("fp6", "gauss", T, O, K)
    else:
        with _e3m2_value_set():
            c8 = gm.make_case("fp8", family, T, O, K)
        c6 = gm.make_case("fp6", family, T, O, K)
    assert float(gm.decode("fp8", c8["a"]).abs().max()) <= 28.0
    a, sa = (e4m3_to_f6(c8["a"], "e3m2"), c8["a_scales"]) if ta == "e3m2" else (c6["a"], c6["a_scales"])
    w, sw = (e4m3_to_f6(c8["w"], "e3m2"), c8["w_scales"]) if tw == "e3m2" else (c6["w"], c6["w_scales"])
    bias = c8["bias"] if family != "zero" else (c8["bias"] if ta == "e3m2" else c6["bias"])
    dense = tuple(None if t is None else t.to(dev) for t in (a, sa, w, sw, bias))
    as_bytes = (f6_to_e4m3(dense[0], ta), dense[1], f6_to_e4m3(dense[2], tw), dense[3], dense[4])
    return dense, as_bytes


def test_full_range_codes_against_float64(dev, lib_options):
    """E3M2 operands on the activation side, on the weight side and on both, every construction, FPQ_GEMM6_CFG 0 / 1 on row-major
    codes and k-major images: within gm.WIDE_FP8_MEASURED x the bound with the exact non-finite pattern, zero rows exactly
    fp16(bias), all four forms of a case bit-equal; E2M3 x E2M3 through fpq_gemm_f6_rows bit-equal to gemm.linear_fp6 and within
    1.0 x the bound.  Prints the worst ratio per construction and pair, and (information only) the share of elements bit-equal to
    gemm.linear_fp8 on the same levels and to gm.emulate("fp8", ..) with a nearest-even / truncating accumulator chain."""
    from fpqvar_amd import gemm
    worst, bad, agree = {}, [], {}
    for family in CONSTRUCTIONS:
        for T, O, K in FULL_SHAPES:
            for ta, tw in BF6_PAIRS:
                key = f"{family:12s} {ta} x {tw}"
                (a, sa, w, sw, bias), as_bytes = _full_case(family, T, O, K, ta, tw, dev)
                r = gm.reference("fp8", *as_bytes)
                runs = _runs(gemm, lib_options, a, sa, w, sw, bias, ta, tw)
                for what, y in runs:
                    what = f"{what} T={T} O={O} K={K}"
                    rat = gm.ratio(y, r)
                    worst[key] = max(worst.get(key, 0.0), rat)
                    if not rat <= gm.WIDE_FP8_MEASURED:
                        bad.append((key, what, rat))
                    if not _same_bits(y, runs[0][1]):
                        bad.append((key, what, "differs from row-major cfg 0"))
                    if family == "zero":
                        want = bias.view(1, O).expand_as(y).contiguous() if bias is not None else torch.zeros_like(y)
                        if not _same_bits(y, want):
                            bad.append((key, what, "zero construction: output is not exactly fp16(bias) / +0"))
                y = runs[0][1]
                y8 = gemm.linear_fp8(*as_bytes)
                eqs = {"fp8": (y.view(torch.int16) == y8.view(torch.int16)) | (torch.isnan(y) & torch.isnan(y8))}
                if T * O <= 60000:
                    for mode in ("rne", "rtz"):
                        e = gm.emulate("fp8", *as_bytes, acc_round=mode)
                        eqs[mode] = (y.view(torch.int16) == e.view(torch.int16)) | (torch.isnan(y) & torch.isnan(e))
                for name, eq in eqs.items():
                    tot, hit = agree.get((key, name), (0, 0))
                    agree[(key, name)] = (tot + eq.numel(), hit + int(eq.sum()))
    # E2M3 x E2M3 through the new entry point: the kernel linear_fp6 launches today
    for family in ("gauss", "max_codes", "non_finite", "fp16_w_scales"):
        for T, O, K in FULL_SHAPES:
            c = {k: (v.to(dev) if torch.is_tensor(v) else v) for k, v in gm.make_case("fp6", family, T, O, K).items()}
            args = (c["a"], c["a_scales"], c["w"], c["w_scales"], c["bias"])
            key = f"{family:12s} e2m3 x e2m3"
            r = gm.reference("fp6", *args)
            for (what, y), (_, y_old) in zip(_runs(gemm, lib_options, *args, "e2m3", "e2m3", ctypes_e2m3=True),
                                             _runs(gemm, lib_options, *args, "e2m3", "e2m3")):
                rat = gm.ratio(y, r)
                worst[key] = max(worst.get(key, 0.0), rat)
                if not rat <= 1.0:
                    bad.append((key, f"{what} T={T} O={O} K={K}", rat))
                if not _same_bits(y, y_old):
                    bad.append((key, f"{what} T={T} O={O} K={K}", "fpq_gemm_f6_rows(E2M3, E2M3) differs from gemm.linear_fp6"))
    print(f"\nBF6 / mixed FP6 GEMM: max err / bound (allowed: {gm.WIDE_FP8_MEASURED} with an E3M2 side, 1.0 for e2m3 x e2m3); "
          "share of elements bit-equal to linear_fp8 on the same levels and to emulate('fp8') rne / rtz")
    for key, rat in sorted(worst.items()):
        extra = "".join(f"  {name} {hit / max(tot, 1):.5f}" for (k, name), (tot, hit) in sorted(agree.items()) if k == key)
        print(f"  {key:34s} {rat:7.3f}{extra}")
    assert not bad, f"{len(bad)} failures, first {bad[:8]}"


# ------------------------------------------------------------------------------------------------ 4. split output and q / k norm
def _bits(t):
    return t.contiguous().view(torch.int16)


def _qkv_operands(tokens, c, kmajor, seed, ta, tw, dev):
    from fpqvar_amd import gemm
    torch.manual_seed(seed)
    x = torch.randn(tokens, c, device=dev).half()
    wt = torch.randn(3 * c, c, device=dev) * 0.05
    a, wq = gemm.quantize_fp6(x, table=ta), gemm.quantize_fp6(wt, table=tw)
    rm = (a, wq)
    if kmajor:
        a, wq = gemm.quantize_fp6(x, kmajor=True, table=ta), (gemm.to_kmajor(wq[0], 6, dealt=True), wq[1])
    return a, wq, rm


def _untouched(cache, pos, seq, fill):
    keep = torch.ones(cache.shape[2], dtype=torch.bool, device=cache.device)
    keep[pos:pos + seq] = False
    return bool((cache[:, :, keep] == fill).all())


@pytest.mark.parametrize("ta,tw", BF6_PAIRS + PAIRS[:1])
@pytest.mark.parametrize("bsz,seq,heads", [(3, 9, 2), (2, 169, 4), (7, 100, 30), (2, 2116, 4)])
@pytest.mark.parametrize("kmajor", [False, True])
def test_split_output_and_qk_norm(dev, ta, tw, bsz, seq, heads, kmajor, lib_options):
    """after tests/test_gpu_fp6_qkv_split.py: without the norm q, k, v are the three column parts of linear_fp6 of the same pair,
    bit for bit, nothing outside the slots written; with it q and k within one fp16 ulp of the reference's norm lines in fp32 on
    that product, v bit-equal"""
    from fpqvar_amd import gemm, kv_cache
    c, max_len, pos = heads * 64, seq + 37, 11
    a, w, rm = _qkv_operands(bsz * seq, c, kmajor, bsz * seq + heads, ta, tw, dev)
    tables = dict(a_table=ta, w_table=tw)
    for cfg in (None, 0, 1):
        lib_options("FPQ_GEMM6_CFG", cfg)
        for with_bias in (False, True):
            bias = (_bias(c, heads + seq) * 3).half() if with_bias else None
            want = gemm.linear_fp6(*rm[0], *rm[1], bias, **tables).view(bsz, seq, 3, heads, 64)
            cache = torch.full((2, bsz, max_len, heads, 64), 7.5, dtype=torch.float16, device=dev)
            q = gemm.linear_fp6_qkv_to_cache(*a, *w, bias, cache, pos, seq, **tables)
            assert q.shape == (bsz, seq, c) and q.dtype == torch.float16
            assert torch.equal(_bits(q.view(bsz, seq, heads, 64)), _bits(want[:, :, 0])), "q"
            assert torch.equal(_bits(cache[0, :, pos:pos + seq]), _bits(want[:, :, 1])), "k"
            assert torch.equal(_bits(cache[1, :, pos:pos + seq]), _bits(want[:, :, 2])), "v"
            assert _untouched(cache, pos, seq, 7.5), "the GEMM wrote outside its slots"
            # ... and with the q / k norm
            bias32 = _bias(c, heads + seq) if with_bias else None
            hs = kv_cache.qk_norm_head_scale(_scale_mul(heads, seq))
            y16 = gemm.linear_fp6(*rm[0], *rm[1], **tables)
            y = y16.float().view(bsz, seq, 3 * c) + (bias32 if with_bias else 0.0)
            want_q, want_k, want_v = _reference(y, hs, heads)
            cache = torch.full((2, bsz, max_len, heads, 64), 7.5, dtype=torch.float16, device=dev)
            q = gemm.linear_fp6_qkv_to_cache(*a, *w, bias32, cache, pos, seq, qk_norm_scale=hs, **tables)
            _assert_ulp(q.view(bsz, seq, heads, 64), want_q, "q")
            _assert_ulp(cache[0, :, pos:pos + seq], want_k, "k")
            assert torch.equal(_bits(cache[1, :, pos:pos + seq]), _bits(want_v)), "v not bit-exact"
            assert _untouched(cache, pos, seq, 7.5), "the GEMM wrote outside its slots"
    if (ta, tw) != PAIRS[0]:   # the pair matters: the same bytes decoded as E2M3 x E2M3 are another product
        lib_options("FPQ_GEMM6_CFG", None)
        assert not torch.equal(gemm.linear_fp6(*rm[0], *rm[1], **tables), gemm.linear_fp6(*rm[0], *rm[1]))


# ------------------------------------------------------------------------------------------------ 5. modules
W6 = dict(weight_quant="per_channel", act_quant="per_token", w_bit=6, a_bit=6, act_quant_sym=True, activation_fp_quant=True,
          weight_fp_quant=True)


@pytest.mark.parametrize("ta,tw", PAIRS)
@pytest.mark.parametrize("kmajor", [False, True])
def test_fp6_linear_module_pairs(dev, ta, tw, kmajor):
    from fpqvar_amd import gemm, quant_linear as ql, rotation as rot
    torch.manual_seed(5)
    lin = torch.nn.Linear(1920, 640).to(dev)
    x = torch.randn(3, 50, 1920, device=dev).half()
    fp6 = gemm.FP6Linear.from_float(lin, kmajor=kmajor, weight_fp_type="fp6_" + tw, act_fp_type="fp6_" + ta)
    assert (fp6.act_table, fp6.w_table, fp6.kmajor) == (ta, tw, kmajor)
    fake = ql.QuantizedLinear.from_float(lin, act_fp_type="fp6_" + ta, weight_fp_type="fp6_" + tw, **W6).half()
    ya, yb = fake(x).float(), fp6(x).float()
    assert yb.shape == (3, 50, 640)
    assert float((ya - yb).abs().max()) <= 2e-2 * float(ya.abs().max()) + 1e-3
    w_codes = fp6.w_codes if not kmajor else gm.from_kmajor(fp6.w_codes, 6, 640, dealt=True)
    assert_bits_equal(gemm.dequantize_fp6(w_codes, fp6.w_scales, tw).half(), fake.weight, "FP6Linear weight")
    assert w_codes.numel() == 640 * 1920 * 3 // 4
    # forward_operands: a producer's output instead of the module's own quantizer
    a = gemm.quantize_fp6(x.reshape(-1, 1920), kmajor=kmajor, table=ta)
    assert torch.equal(_bits(fp6.forward_operands(*a)), _bits(fp6(x).view(-1, 640)))
    scale = torch.zeros(3, 1, 1920, device=dev).half()
    prod = rot.adaln_rotate_quant_token(x, scale, scale, ta, emit="fp6" if ta == "e2m3" else "bf6", kmajor=kmajor)
    gate, resid = torch.randn(3, 1, 640, device=dev).half(), torch.randn(150, 640, device=dev).half()
    y = fp6.forward_operands(*prod)
    assert y.shape == (150, 640) and bool(torch.isfinite(y).all())
    assert torch.equal(_bits(fp6.forward_operands(*prod, gate, resid)), _bits(resid + (y.view(3, 50, 640) * gate).view(150, 640)))


class _FFN(torch.nn.Module):
    def __init__(self, c):
        super().__init__()
        self.fc1, self.fc2 = torch.nn.Linear(c, 2 * c), torch.nn.Linear(2 * c, c)


class _Attn(torch.nn.Module):
    def __init__(self, c):
        super().__init__()
        self.mat_qkv, self.proj = torch.nn.Linear(c, 3 * c, bias=False), torch.nn.Linear(c, c)


def test_quantize_var_packed_e3m2(dev):
    """the toy of test_quantize_var_real_fp4: with packed_e3m2 every layer with an E3M2 side is an FP6Linear of its pair; the default
    keeps FP8Linear"""
    from fpqvar_amd import gemm, quant_linear as ql

    class Toy(torch.nn.Module):
        def __init__(self):
            super().__init__()
            torch.manual_seed(3)
            self.ffn, self.attn = _FFN(256), _Attn(256)

    base = Toy().to(dev)
    x = torch.randn(70, 256, device=dev).half()
    for ta, tw in PAIRS:
        cfg = dict(W6, act_fp_type="fp6_" + ta, weight_fp_type="fp6_" + tw, fc2_fp_type="fp6_int_neg_e2m3_pos")
        fake = ql.quantize_VAR(copy.deepcopy(base), **cfg).half()
        default = ql.quantize_VAR(copy.deepcopy(base), real_fp6=True, **cfg)
        packed = ql.quantize_VAR(copy.deepcopy(base), real_fp6=True, packed_e3m2=True, **cfg)
        want_default = gemm.FP6Linear if (ta, tw) == PAIRS[0] else gemm.FP8Linear
        for name in ("ffn.fc1", "attn.mat_qkv", "attn.proj"):
            d, p, f = (m.get_submodule(name) for m in (default, packed, fake))
            assert type(d) is want_default, (name, ta, tw, type(d))
            assert type(p) is gemm.FP6Linear and (p.act_table, p.w_table) == (ta, tw) and p.kmajor, (name, ta, tw)
            ya, yb = f(x).float(), p(x).float()
            assert float((ya - yb).abs().max()) <= 2e-2 * float(ya.abs().max()) + 1e-3
        assert type(packed.ffn.fc2).__name__ == "QuantizedLinear_fc2" and type(default.ffn.fc2).__name__ == "QuantizedLinear_fc2"
    with pytest.raises(ValueError):
        ql.quantize_VAR(copy.deepcopy(base), real_fp6=True, packed_e3m2=True, **dict(W6, act_fp_type="fp_e2", weight_fp_type="fp6_e2m3"))


def test_quantize_var_mixed_fp6_datatype_on_the_matrix_cores(dev):
    """quantize_VAR_mixed_fp6_datatype(real_fp6=True) on a 30-block toy: every fc1, fc2, mat_qkv, proj an FP6Linear with the
    (activation, weight) tables the reference hard-codes for its block (as test_quantize_var_mixed_datatype_variants spells
    them), ada_lin[1] a QuantizedLinear; the default keeps today's modules; a state_dict round trip"""
    from fpqvar_amd import gemm, quant_linear as ql

    class Blk(torch.nn.Module):
        def __init__(self):
            super().__init__()
            self.ffn, self.attn = _FFN(256), _Attn(256)
            self.ada_lin = torch.nn.Sequential(torch.nn.SiLU(), torch.nn.Linear(256, 1536))

    class Toy(torch.nn.Module):
        def __init__(self, seed):
            super().__init__()
            torch.manual_seed(seed)
            self.blocks = torch.nn.ModuleList([Blk() for _ in range(30)])

    cfg6 = dict(W6, act_fp_type="fp6_e2m3", weight_fp_type="fp6_e2m3", fc2_fp_type="fp6_int_neg_e2m3_pos")
    base = Toy(9).to(dev)
    m = ql.quantize_VAR_mixed_fp6_datatype(copy.deepcopy(base), real_fp6=True, **cfg6)
    fake = ql.quantize_VAR_mixed_fp6_datatype(copy.deepcopy(base), **cfg6)
    for b in range(30):
        blk = m.blocks[b]
        want = {"ffn.fc1": "e3m2", "attn.mat_qkv": "e3m2", "ffn.fc2": "e2m3" if b in (0, 23) else "e3m2",
                "attn.proj": "e2m3" if b >= 2 else "e3m2"}
        for name, act in want.items():
            lin = blk.get_submodule(name)
            assert type(lin) is gemm.FP6Linear and (lin.act_table, lin.w_table) == (act, "e2m3") and lin.kmajor, (b, name)
            assert type(fake.blocks[b].get_submodule(name)).__name__.startswith("QuantizedLinear")
        assert type(blk.ada_lin[1]).__name__ == "QuantizedLinear"
    rm = ql.quantize_VAR_mixed_fp6_datatype(copy.deepcopy(base), real_fp6=True, kmajor_operands=False, **cfg6)
    assert not rm.blocks[4].ffn.fc1.kmajor and rm.blocks[4].ffn.fc1.act_table == "e3m2"
    x = torch.randn(5, 256, device=dev).half()
    h = torch.randn(5, 512, device=dev).half()
    for b in (0, 1, 7, 23):
        for name, inp in (("ffn.fc1", x), ("attn.mat_qkv", x), ("attn.proj", x), ("ffn.fc2", h)):
            ya = fake.blocks[b].get_submodule(name).half()(inp).float()
            yb = m.blocks[b].get_submodule(name)(inp).float()
            assert float((ya - yb).abs().max()) <= 2e-2 * float(ya.abs().max()) + 1e-3, (b, name)
            assert torch.equal(_bits(rm.blocks[b].get_submodule(name)(inp)), _bits(yb.half())), (b, name, "row-major vs k-major")
    # state_dict round trip into a model quantized from other weights
    other = ql.quantize_VAR_mixed_fp6_datatype(Toy(10).to(dev), real_fp6=True, **cfg6)
    assert not torch.equal(other.blocks[3].ffn.fc1.w_codes, m.blocks[3].ffn.fc1.w_codes)
    other.load_state_dict(m.state_dict())
    for b in (0, 3, 23):
        for name, inp in (("ffn.fc1", x), ("attn.proj", x), ("ffn.fc2", h)):
            assert torch.equal(_bits(other.blocks[b].get_submodule(name)(inp)), _bits(m.blocks[b].get_submodule(name)(inp))), (b, name)
