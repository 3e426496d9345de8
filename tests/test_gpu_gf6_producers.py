"""The rotate and adaLN producers emitting per-group operands on the FULL FP6 tables on the GPU (include/fpq.h, "THE SAME PRODUCERS
ON THE FULL FP6 TABLES"): rotation.rotate_quant_gf6 / adaln_rotate_quant_gf6, FP6GroupLinear[GeluDual].adaln_operands /
rotate_operands / qkv_to_cache_operands.

The contract is the header's: with y the fp16 rotated rows the values form emits for the same arguments and table, codes and scales
are BYTE FOR BYTE what gemm.quantize_gf6(y, table, kmajor) writes, hence level(code) * scale is the values form's `out` bit for bit -
which in turn is the oracle's per-group quantization of y.  No tolerance appears anywhere: every assertion is equality of bits, or of
NaN positions.  Shapes: every MAXC form of the adaLN kernel (C = 128 .. 2560), the width PAIR2 would take (1024), a ragged and a
full tile (1920, 2048), the slot of 1, 2 and 4 groups (2176, 2304, 2560); batch entries that leave ragged workgroups and an odd row
count.  The 6-bit group forms of the two kernels were written for the 2 x 128 / 2 x 64 buckets of E1M2 / E3M0; here they stage the 2 x
512 buckets of E2M3 and the 2 x 256 of E3M2.  The rotate kernel by default stages no table at all: it takes the codes from the FP6
conversion hardware (rq_store_codes6_hw) - every rotate case runs in that form and, under FPQ_NO_HW6 = 1, in the table form, and the
two must agree byte for byte with each other and with quantize_gf6: that equality is what establishes how the conversion packs its
32 codes."""
import functools

import pytest
import torch

from oracle import fpq_oracle as orc
from tests.conftest import assert_bits_equal

pytestmark = pytest.mark.gpu

TABLES = ("e2m3", "e3m2")
ADALN_C = (128, 1024, 1920, 2048, 2176, 2304, 2560)
ADALN_BL = ((1, 1), (3, 5), (5, 23), (2, 64))
ROTATE_SHAPES = ((1, 128), (3, 384), (7, 1920), (33, 2304), (257, 1024))   # 3 x 384: tiles spanning rows, a 9-group tail tile


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "these tests need the GPU"
    return torch.device("cuda:0")


def _bits(t):
    return t.contiguous().view(torch.int16)


def _scale_mul(heads, seed):
    """scale_mul_1H11 of a block with attn_l2_norm; head 0 above log 100: clamped"""
    g = torch.Generator().manual_seed(seed)
    sm = torch.full((1, heads, 1, 1), 4.0).log() + 0.3 * torch.randn(1, heads, 1, 1, generator=g)
    sm[0, 0] = 5.5
    return sm.to(torch.device("cuda:0"))


def _bias32(c, seed):
    """the fp32 cat(q_bias, 0, v_bias) of such a block"""
    g = torch.Generator().manual_seed(seed)
    b = torch.randn(3 * c, generator=g) * 0.1
    b[c:2 * c] = 0
    return b.to(torch.device("cuda:0"))


def _untouched_is(cache, pos, seq, value):
    untouched = torch.ones(cache.shape[2], dtype=torch.bool, device=cache.device)
    untouched[pos:pos + seq] = False
    return bool((cache[:, :, untouched] == value).all())


def _raw(t):
    """a tensor's bytes (fp16 / fp32 scales compared byte for byte, NaN payloads included)"""
    return t.contiguous().view(torch.uint8)


def from_kmajor6(image: torch.Tensor) -> torch.Tensor:
    """the activation side's 6-bit image [G][rows][96] back to row-major codes [rows, 96 G] (include/fpq.h, "K-MAJOR OPERAND
    IMAGES": image chunk p of row j holds code chunk (p - ((j >> 3) & 1)) mod 6)"""
    g, rows, _ = image.shape
    im = image.cpu().view(g, rows, 6, 16)
    j = torch.arange(rows)
    rot = (j >> 3) & 1
    out = torch.empty_like(im)
    for p in range(6):
        c = (p - rot) % 6                                   # [rows]
        out[:, j, c] = im[:, j, p]
    return out.permute(1, 0, 2, 3).reshape(rows, g * 96).contiguous().to(image.device)


def _inputs(b, l, c, x_dtype, seed=90):
    """tests/test_gpu_parity.py's producer input: seeded log-normal spread, one all-zero row, one inf, one NaN, one row x 1e-3"""
    g = torch.Generator().manual_seed(seed + c + 7 * b + l)
    x = (torch.randn(b, l, c, generator=g) * torch.exp(0.5 * torch.randn(b, l, c, generator=g))).to(x_dtype)
    rows = x.view(-1, c)
    n = rows.shape[0]
    if n > 4:
        rows[1] = 0.0
        rows[2, 77] = float("inf")
        rows[3, 5] = float("nan")
        rows[4] *= 1e-3
    sc = torch.randn(b, 1, c, generator=g) * 0.3
    sh = torch.randn(b, 1, c, generator=g) * 0.3
    sm = torch.rand(c, generator=g) + 0.5
    return x, sc, sh, sm


def _check(got, y, out, table, kmajor, what):
    """the three assertions of the contract; y, out: the values form's rotated rows and result, [rows, C] on the GPU"""
    from fpqvar_amd import gemm
    rows, c = y.shape
    codes, scales = got
    want_codes, want_scales = gemm.quantize_gf6(y, table, kmajor=kmajor)
    assert codes.shape == want_codes.shape and codes.dtype == torch.uint8, (what, codes.shape, want_codes.shape)
    assert scales.shape == want_scales.shape and scales.dtype == want_scales.dtype, (what, scales.shape, scales.dtype)
    assert torch.equal(codes, want_codes), f"{what}: codes differ from quantize_gf6 of the rotated rows"
    if kmajor:
        assert torch.equal(_raw(scales[:, :rows]), _raw(want_scales[:, :rows])), f"{what}: scale image differs on live rows"
        assert not bool(scales[:, rows:].any()), f"{what}: padding rows of the scale image were written"
        codes_rm, scales_rm = from_kmajor6(codes), scales[:, :rows].t().contiguous()
    else:
        assert torch.equal(_raw(scales), _raw(want_scales)), f"{what}: scales differ from quantize_gf6 of the rotated rows"
        codes_rm, scales_rm = codes, scales
    assert_bits_equal(gemm.dequantize_gf6(codes_rm, scales_rm, table).half(), out.cpu(), f"{what}: level(code) * scale vs the values form")


@functools.lru_cache(maxsize=None)
def _adaln_reference(b, l, c, x32, mod32, smooth, table):
    """inputs on the GPU and the values form's (out, y) as [rows, C], pinned to the oracle - once per case, never written to"""
    from fpqvar_amd import rotation as rot
    dev = torch.device("cuda:0")
    x, sc, sh, sm = _inputs(b, l, c, torch.float32 if x32 else torch.float16)
    mod = torch.float32 if mod32 else torch.float16
    x, sc, sh = x.to(dev), sc.to(mod).to(dev), sh.to(mod).to(dev)
    sm = sm.to(dev) if smooth else None
    out, _, y = rot.adaln_rotate_quant(x, sc, sh, table, smooth=sm, return_intermediates=True)
    out, y = out.view(-1, c), y.view(-1, c)
    assert_bits_equal(out.cpu(), orc.per_group_kernel_sem(y.cpu(), table, 128), "the values form vs the oracle on its rotated rows")
    return x, sc, sh, sm, out, y


# ---- 1. adaLN: the shapes at which the kernel can go wrong ----------------------------------------------------------------
@pytest.mark.parametrize("table", TABLES)
@pytest.mark.parametrize("b,l", ADALN_BL)
@pytest.mark.parametrize("c", ADALN_C)
@pytest.mark.parametrize("x32", (False, True))
def test_adaln_operands_equal_quantize_gf6_of_the_rotated_rows(dev, x32, c, b, l, table):
    from fpqvar_amd import rotation as rot
    for mod32 in (False, True):
        for smooth in (False, True):
            x, sc, sh, sm, out, y = _adaln_reference(b, l, c, x32, mod32, smooth, table)
            for kmajor in (False, True):
                got = rot.adaln_rotate_quant_gf6(x, sc, sh, table, smooth=sm, kmajor=kmajor)
                _check(got, y, out, table, kmajor, f"C={c} B={b} L={l} x32={x32} mod32={mod32} smooth={smooth} kmajor={kmajor}")


# ---- 2. workgroup cuts: results independent of how rows are dealt to workgroups ----------------------------------------------
@pytest.mark.parametrize("table", TABLES)
@pytest.mark.parametrize("c", (1920, 2304))
def test_adaln_operands_independent_of_the_workgroup_cut(dev, c, table):
    from fpqvar_amd import _lib, rotation as rot
    for b, l in ((5, 23), (2, 64)):
        for x32 in (False, True):
            x, sc, sh, sm, out, y = _adaln_reference(b, l, c, x32, False, True, table)
            for n in (1, 4, 8, 12):
                with _lib.option("FPQ_ADALN_ROWS", n):
                    for kmajor in (False, True):
                        got = rot.adaln_rotate_quant_gf6(x, sc, sh, table, smooth=sm, kmajor=kmajor)
                        _check(got, y, out, table, kmajor, f"FPQ_ADALN_ROWS={n} C={c} B={b} L={l} x32={x32} kmajor={kmajor}")


@pytest.mark.parametrize("kmajor", (False, True))
def test_adaln_operands_at_the_cut_of_large_launches(dev, kmajor):
    """[20 x 576 x 2304] fp16 rows: from 8192 rows on the library deals 8 rows to a workgroup by itself, two per wavefront.  The 6-bit
    group form pairs no rows (its contract is stated against the emitting form's rotated rows), on these tables as on E1M2 / E3M0."""
    from fpqvar_amd import gemm, rotation as rot
    g = torch.Generator().manual_seed(4)
    x = torch.randn(20, 576, 2304, generator=g).half().to(dev)
    sc = (torch.randn(20, 1, 2304, generator=g) * 0.3).half().to(dev)
    sh = (torch.randn(20, 1, 2304, generator=g) * 0.3).half().to(dev)
    sm = (torch.rand(2304, generator=g) + 0.5).to(dev)
    y = rot.adaln_rotate_quant(x, sc, sh, "e2m3", smooth=sm, return_intermediates=True)[2].view(-1, 2304)
    codes, scales = rot.adaln_rotate_quant_gf6(x, sc, sh, "e2m3", smooth=sm, kmajor=kmajor)
    want_codes, want_scales = gemm.quantize_gf6(y, "e2m3", kmajor=kmajor)
    assert torch.equal(codes, want_codes), "codes differ from quantize_gf6 of the rotated rows"
    assert torch.equal(_raw(scales), _raw(want_scales)), "scales differ from quantize_gf6 of the rotated rows"   # 11520 rows: no padding


# ---- 3. rotate -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("table", TABLES)
@pytest.mark.parametrize("rows,c", ROTATE_SHAPES)
def test_rotate_operands_equal_quantize_gf6_of_the_rotated_rows(dev, rows, c, table):
    """every case under the default (the table-free form of the kernel: codes from the FP6 conversion hardware) and under
    FPQ_NO_HW6 = 1 (the staged table): byte-equal to each other and to quantize_gf6 of the rotated rows, the all-zero, inf and NaN
    rows included (the hardware form's wave-uniform table path)"""
    from fpqvar_amd import _lib, rotation as rot
    custom_d = rot.sign_vector(128, 7)
    for x_dtype in (torch.float16, torch.float32):
        x, _, _, sm = _inputs(1, rows, c, x_dtype, seed=31)
        x, sm = x.view(rows, c).to(dev), sm.to(dev)
        for smooth in (None, sm):
            for d in (None, custom_d):   # the compiled binding / the ctypes path
                if d is not None and (smooth is None or x_dtype is torch.float32):
                    continue              # the custom sign vector once: fp16 rows with smooth
                out, y = rot.rotate_quant(x, table, d=d, smooth=smooth, return_rotated=True)
                assert_bits_equal(out.cpu(), orc.per_group_kernel_sem(y.cpu(), table, 128), "the values form vs the oracle on its rotated rows")
                for kmajor in (False, True):
                    what = f"rotate {rows}x{c} {x_dtype} smooth={smooth is not None} custom_d={d is not None} kmajor={kmajor}"
                    got = rot.rotate_quant_gf6(x, table, d=d, smooth=smooth, kmajor=kmajor)   # codes from the FP6 conversion hardware
                    with _lib.option("FPQ_NO_HW6", 1):                                        # ... and from the bucket table
                        tab = rot.rotate_quant_gf6(x, table, d=d, smooth=smooth, kmajor=kmajor)
                    _check(got, y, out, table, kmajor, what + " (conversion hardware)")
                    _check(tab, y, out, table, kmajor, what + " (FPQ_NO_HW6: table)")
                    assert torch.equal(got[0], tab[0]) and torch.equal(_raw(got[1]), _raw(tab[1])), f"{what}: the two forms differ"


@pytest.mark.parametrize("table", TABLES)
@pytest.mark.parametrize("x32", (False, True))
def test_rotate_conversion_hardware_against_the_table_on_a_wide_spread(dev, x32, table):
    """[2048 x 1024] rows over ten octaves per group and four tiers of row magnitude: 2 M quotients, so every level, ties between
    levels (a tie is an fp16 quotient: about one in 2^7 at the top binade) and quotients in (-step / 2, 0), whose hardware code is
    -0.  Both layouts, with and without a smoothing vector; once more with FPQ_ROT_WGS = 24, where every workgroup walks eleven of
    the 256 workgroup tiles (the default grid gives each one)."""
    from fpqvar_amd import _lib, gemm, rotation as rot
    g = torch.Generator().manual_seed(17 + x32)
    x = torch.randn(2048, 1024, generator=g) * torch.exp2(torch.randint(-9, 1, (2048, 1024), generator=g).float())
    x = (x * torch.tensor([1e-4, 1.0, 37.0, 600.0]).repeat(512).unsqueeze(1)).to(torch.float32 if x32 else torch.float16).to(dev)
    sm = (torch.rand(1024, generator=g) + 0.5).to(dev)
    for smooth in (None, sm):
        y = rot.rotate_quant(x, table, smooth=smooth, return_rotated=True)[1]
        for kmajor in (False, True):
            want = gemm.quantize_gf6(y, table, kmajor=kmajor)
            got = rot.rotate_quant_gf6(x, table, smooth=smooth, kmajor=kmajor)
            with _lib.option("FPQ_NO_HW6", 1):
                tab = rot.rotate_quant_gf6(x, table, smooth=smooth, kmajor=kmajor)
            with _lib.option("FPQ_ROT_WGS", 24):
                walk = rot.rotate_quant_gf6(x, table, smooth=smooth, kmajor=kmajor)
            for name, r in (("conversion hardware", got), ("table", tab), ("conversion hardware, 24 workgroups", walk)):
                assert torch.equal(r[0], want[0]), f"{name}: codes differ from quantize_gf6 of the rotated rows (smooth={smooth is not None} kmajor={kmajor})"
                assert torch.equal(_raw(r[1]), _raw(want[1])), f"{name}: scales differ (smooth={smooth is not None} kmajor={kmajor})"
            assert int((want[0] != 0).sum()) > want[0].numel() // 2, "the case lost its spread"


# ---- 4. through the modules ------------------------------------------------------------------------------------------------
T_B, T_L, K, O = 2, 35, 1920, 256   # T = 70 tokens
PAIRS = (("fp6_e2m3", "fp6_e2m3"), ("fp6_e2m3", "fp_e2"), ("fp6_e3m2", "fp_e1"))   # (activation, weight)


@functools.lru_cache(maxsize=None)
def _gemm_case(table):
    from fpqvar_amd import rotation as rot
    dev = torch.device("cuda:0")
    x, sc, sh, sm = _inputs(T_B, T_L, K, torch.float32, seed=11)
    x = torch.nan_to_num(x, nan=0.5, posinf=2.0)              # the products are compared as numbers: finite rows
    x, sc, sh, sm = x.to(dev), sc.half().to(dev), sh.half().to(dev), sm.to(dev)
    _, _, y = rot.adaln_rotate_quant(x, sc, sh, table, smooth=sm, return_intermediates=True)
    _, yr = rot.rotate_quant(x, table, smooth=sm, return_rotated=True)
    return x, sc, sh, sm, y, yr


@pytest.mark.parametrize("kmajor", (False, True))
@pytest.mark.parametrize("act,weight", PAIRS)
@pytest.mark.parametrize("cls", ("FP6GroupLinear", "FP6GroupLinearGeluDual"))
def test_operands_through_the_linears(dev, cls, act, weight, kmajor):
    """forward_operands(*adaln_operands(...)) == forward(y), rotate_operands likewise"""
    from fpqvar_amd import gemm, rotation as rot
    torch.manual_seed(5)
    lin = torch.nn.Linear(K, O).to(dev)
    m = getattr(gemm, cls).from_float(lin, weight_fp_type=weight, act_fp_type=act, kmajor=kmajor)
    assert m.act_table in TABLES and m.kmajor == kmajor
    x, sc, sh, sm, y, yr = _gemm_case(m.act_table)
    ops = m.adaln_operands(x, sc, sh, smooth=sm)
    want = rot.adaln_rotate_quant_gf6(x, sc, sh, m.act_table, smooth=sm, kmajor=kmajor)
    assert ops[0].shape == ((K // 128, T_B * T_L, 96) if kmajor else (T_B * T_L, K * 3 // 4))
    assert torch.equal(ops[0], want[0]) and torch.equal(_raw(ops[1]), _raw(want[1]))
    assert torch.equal(_bits(m.forward_operands(*ops)), _bits(m(y).view(-1, O))), "adaln_operands -> forward_operands vs forward(y)"
    rops = m.rotate_operands(x, smooth=sm)
    assert torch.equal(_bits(m.forward_operands(*rops)), _bits(m(yr).view(-1, O))), "rotate_operands -> forward_operands vs forward(y)"


@pytest.mark.parametrize("kmajor", (False, True))
@pytest.mark.parametrize("act,weight", PAIRS)
def test_producer_to_split_gemm_to_cache(dev, act, weight, kmajor):
    """qkv_to_cache_operands(*adaln_operands(...)) against qkv_to_cache(y): q and the written cache slots bit-equal, other slots
    untouched, with and without the q / k norm (mat_qkv: out_features = 3 x 128, two heads)"""
    from fpqvar_amd import gemm, kv_cache
    heads, c_out, max_len, pos = 2, 128, T_L + 5, 3
    torch.manual_seed(6)
    lin = torch.nn.Linear(K, 3 * c_out).to(dev)
    hs = kv_cache.qk_norm_head_scale(_scale_mul(heads, 3))
    for norm in (False, True):
        if norm:
            lin.bias = None
        m = gemm.FP6GroupLinear.from_float(lin, weight_fp_type=weight, act_fp_type=act, kmajor=kmajor)
        x, sc, sh, sm, y, _ = _gemm_case(m.act_table)
        extra = dict(qk_norm_scale=hs, bias=_bias32(c_out, 2)) if norm else {}
        c_want = torch.full((2, T_B, max_len, heads, 64), 7.5, dtype=torch.float16, device=dev)
        c_got = torch.full_like(c_want, 7.5)
        q_want = m.qkv_to_cache(y, c_want, pos, T_L, **extra)
        q_got = m.qkv_to_cache_operands(*m.adaln_operands(x, sc, sh, smooth=sm), c_got, pos, T_L, **extra)
        assert q_got.shape == (T_B, T_L, c_out)
        assert torch.equal(_bits(q_got), _bits(q_want)) and torch.equal(_bits(c_got), _bits(c_want)), f"norm={norm}"
        assert _untouched_is(c_got, pos, T_L, 7.5)


# ---- 5. graph --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kmajor", (False, True))
def test_adaln_operands_in_a_captured_graph(dev, kmajor):
    from fpqvar_amd import rotation as rot
    x, sc, sh, sm, out, y = _adaln_reference(5, 23, 2304, True, False, True, "e2m3")
    eager = rot.adaln_rotate_quant_gf6(x, sc, sh, "e2m3", smooth=sm, kmajor=kmajor)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.stream(side):
        rot.adaln_rotate_quant_gf6(x, sc, sh, "e2m3", smooth=sm, kmajor=kmajor)   # warm-up on the capture stream
        side.synchronize()
        with torch.cuda.graph(graph, stream=side):
            got = rot.adaln_rotate_quant_gf6(x, sc, sh, "e2m3", smooth=sm, kmajor=kmajor)
    for t in got:
        t.zero_()
    graph.replay()
    torch.cuda.synchronize()
    rows = y.shape[0]
    assert torch.equal(got[0], eager[0])
    assert torch.equal(_raw(got[1][:, :rows] if kmajor else got[1]), _raw(eager[1][:, :rows] if kmajor else eager[1]))
