"""The A6W4 path on the GPU: the per-group E1M2 / E3M0 operand emitter (gemm.quantize_g6) bit for bit against the fake quantizer
and the oracle, the GEMM (gemm.linear_a6w4) against the float64 reference, bound and fp32 model of tests/a6w4_model.py, and the
modules built on them (gemm.FP4Linear with a 6-bit activation format, quant_linear.quantize_VAR_mixed*(real_fp4=True)).

The numerics rest on one measurement, test_the_128_term_dot_is_exact: with K = 128, unit scales and no bias, dots that are fp16
numbers must come out bit for bit - the matrix core keeps every product of an E1M2 / E3M0 level and an E2M1 level.  MEASURED on
an MI355X (profiles/r09_a6w4_dot.txt): all 48 runs (2 tables x 4 constructions x 2 weight-scale dtypes x 3 tilings) bit-equal to the
exact dot, so the contract is the FP4 GEMM's unchanged - allowance 1.0, bit-equal to the fp32 model; over the shape sweep the worst
error is 1.000 x the bound (the fp16 output rounding)."""
import math

import pytest
import torch

from oracle import fpq_oracle as orc
from tests import a6w4_model as am
from tests import gemm_model as gm
from tests.conftest import assert_bits_equal

pytestmark = pytest.mark.gpu

TABLES = ("e1m2", "e3m0")
ALLOWANCE = 1.0          # x gm.bound: the FP4 contract unchanged (the dot is exact; see the module docstring)
CFGS = (20, 30, None)    # FPQ_GEMM_CFG: 128 x 128 tiles, 64 x 128 tiles, the library's choice


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "these tests need the GPU"
    return torch.device("cuda:0")


def _on(c, dev):
    return {k: (v.to(dev) if torch.is_tensor(v) else v) for k, v in c.items()}


def _args(c):
    return c["a"], c["a_scales"], c["w"], c["w_scales"], c["bias"]


def _same_bits(x, y):
    """bit-equal, every NaN one value"""
    xn, yn = torch.isnan(x), torch.isnan(y)
    return bool(torch.equal(xn, yn)) and bool(torch.equal(x.masked_fill(xn, 0).view(torch.int16), y.masked_fill(yn, 0).view(torch.int16)))


def _lin(gemm, table, c, **kw):
    return gemm.linear_a6w4(c["a"], c["a_scales"], table, c["w"], c["w_scales"], c["bias"], **kw)


# ------------------------------------------------------------------------------------------------------------ the emitter
def _fake(x, table):
    from fpqvar_amd import ops
    return ops.quant_rows(x, table, 128)


@pytest.mark.parametrize("table", TABLES)
@pytest.mark.parametrize("dtype", (torch.float16, torch.float32))
def test_emitter_reproduces_the_fake_quantizer(dev, table, dtype):
    """dequantize_g6(quantize_g6(x)) == ops.quant_rows(x, table, 128) == the oracle's fp_quant_e{1,3}_per_group_cuda, bit for bit:
    rows 1, 100, 25 600 and cols 128, 1920, 2304, 7680, with all-zero groups."""
    from fpqvar_amd import gemm
    g = torch.Generator().manual_seed(900 + len(table) + (dtype == torch.float32))
    for rows, cols in ((1, 128), (1, 7680), (100, 1920), (100, 2304), (100, 128), (100, 7680), (25600, 128), (25600, 1920), (25600, 2304),
                       (25600, 7680)):
        base = min(rows, 256)                      # 25 600 rows: a block of 256 random rows repeated, each row times a power of two
        x = (torch.randn(base, cols, generator=g) * torch.exp(0.7 * torch.randn(base, cols, generator=g))).to(dtype)
        if dtype == torch.float32:
            x = x * 0.02
        if rows > base:
            x = x.repeat(rows // base, 1) * torch.exp2((torch.arange(rows) % 5).to(dtype)).view(rows, 1)
        x[0, :128] = 0
        if rows > 3:
            x[3, cols - 128:] = 0
            x[2, 5] = 0.0
        xd = x.to(dev)
        codes, scales = gemm.quantize_g6(xd, table)
        assert codes.shape == (rows, cols * 3 // 4) and codes.dtype == torch.uint8
        assert scales.shape == (rows, cols // 128) and scales.dtype == dtype
        deq = gemm.dequantize_g6(codes, scales, table).to(dtype)            # level * scale: exact in fp32, one rounding
        fake = _fake(xd, table)
        assert_bits_equal(deq.view(rows, cols), fake.view(rows, cols), f"{table} {dtype} [{rows} x {cols}] vs quant_rows")
        if rows <= 100:
            assert_bits_equal(fake.cpu().view(rows, cols), orc.per_group_kernel_sem(x, table, 128), f"{table} {dtype} [{rows} x {cols}] vs oracle")
        # the decoded levels are levels of the table, a zero group is scale 0 and code 0
        lv = am.decode_a(table, codes[: min(rows, 64)].cpu())
        assert set(lv.abs().unique().tolist()) <= set(am.A_LEVELS[table])
        assert float(scales[0, 0]) == 0.0 and not bool(codes[0, :96].any())


@pytest.mark.parametrize("table", TABLES)
def test_emitter_scales_are_the_fp4_emitters_recipe(dev, table):
    """scale = (T)(max|x| / the table's largest level) per group, one division in x's dtype - the recipe of quantize_mx, which
    divides by E2M1's 6 (checked beside it on the same input)."""
    from fpqvar_amd import gemm
    top = am.A_LEVELS[table][-1]
    g = torch.Generator().manual_seed(41)
    for dtype in (torch.float16, torch.float32):
        x = (torch.randn(200, 1920, generator=g) * 3).to(dtype).to(dev)
        _, s = gemm.quantize_g6(x, table)
        # (tensor / tensor: a true division, as the reference's `x.abs().max(...) / table.abs().max()`; tensor / python float is
        # a multiplication by the reciprocal on this backend)
        want = x.view(200, 15, 128).abs().amax(dim=-1) / torch.tensor(top, dtype=dtype, device=dev)
        assert_bits_equal(s, want, f"{table} {dtype} scales")
        _, s4 = gemm.quantize_mx(x)
        assert_bits_equal(s4, x.view(200, 15, 128).abs().amax(dim=-1) / torch.tensor(6.0, dtype=dtype, device=dev), f"{dtype} quantize_mx scales")


@pytest.mark.parametrize("table", TABLES)
def test_emitter_non_finite_groups(dev, table):
    """Groups holding +-inf or NaN: the group's maximum is stored as its scale and level(code) * scale is what the fake quantizer
    writes (include/fpq.h); every other group is untouched."""
    from fpqvar_amd import gemm
    g = torch.Generator().manual_seed(43)
    for dtype in (torch.float16, torch.float32):
        x = torch.randn(40, 512, generator=g).to(dtype)
        x[3, 5], x[10, 200], x[17, 300], x[17, 20], x[20, 130], x[20, 131] = math.inf, -math.inf, math.nan, math.inf, math.nan, -1.0
        xd = x.to(dev)
        codes, scales = gemm.quantize_g6(xd, table)
        deq = gemm.dequantize_g6(codes, scales, table).to(dtype)
        assert_bits_equal(deq, _fake(xd, table).view(40, 512), f"{table} {dtype} non-finite groups")
        assert math.isinf(float(scales[3, 0])) and math.isinf(float(scales[10, 1])) and math.isnan(float(scales[17, 2]))
        assert math.isnan(float(scales[20, 1])) and bool(torch.isfinite(scales[0]).all())


@pytest.mark.parametrize("table", TABLES)
def test_emitter_every_fp16_pair(dev, table):
    """EVERY (group maximum, element) pair of finite fp16 values, both signs, through the emitter's fast fp16 form against the
    fake quantizer's (tests/test_gpu_parity.py pins that one to the IEEE path and the reference's op sequence on the same
    exhaustive domain)."""
    from fpqvar_amd import gemm, ops
    per, total, step = 127, 0, 512
    for lo in range(0, 0x7C00, step):
        p = torch.arange(lo, min(lo + step, 0x7C00), device=dev, dtype=torch.int64)
        n_val = 2 * (p + 1)
        n_grp = (n_val + per - 1) // per
        mx = torch.repeat_interleave(p, n_grp)
        first = torch.cumsum(n_grp, 0) - n_grp
        start = (torch.arange(mx.numel(), device=dev) - torch.repeat_interleave(first, n_grp)) * per
        idx = start[:, None] + torch.arange(per, device=dev)[None, :]
        ok = idx < (2 * (mx + 1))[:, None]
        pat = torch.where(ok, (idx >> 1) | ((idx & 1) << 15), torch.zeros_like(idx))
        x = torch.cat([mx[:, None], pat], dim=1).to(torch.int32).to(torch.int16).view(torch.float16)
        codes, scales = gemm.quantize_g6(x, table)
        deq = gemm.dequantize_g6(codes, scales, table).half()
        fake = ops.quant_rows(x, table, 128, torch.float16)
        bad = deq.view(torch.int16) != fake.view(torch.int16)
        assert not bool(bad.any()), (table, lo, x[bad][:4].tolist(), deq[bad][:4].tolist(), fake[bad][:4].tolist())
        total += int(ok.sum())
    assert total == 1_007_713_280


# ------------------------------------------------------------------------------------------------------------ the GEMM
@pytest.mark.parametrize("table", TABLES)
def test_the_128_term_dot_is_exact(dev, table, lib_options):
    """K = 128, unit scales, no bias, dots that are fp16 numbers (tests/a6w4_model.py exact_dot_cases: the largest products
    cancelling beside a few +-1/8, all 15 x 15 level pairs alone and 128-fold, the largest product beside 127 smallest): the
    output equals the exact value bit for bit, in both tilings."""
    from fpqvar_amd import gemm
    for name, (La, Lw) in am.exact_dot_cases(table).items():
        a, w = am.encode_a(table, La).to(dev), gm.encode("fp4", gm._to_idx("fp4", Lw)).to(dev)
        sa = torch.ones(La.shape[0], 1, dtype=torch.float16, device=dev)
        exact = (La @ Lw.t()).half().to(dev)
        for ws_dtype in (torch.float32, torch.float16):
            sw = torch.ones(Lw.shape[0], 1, dtype=ws_dtype, device=dev)
            for cfg in CFGS:
                lib_options("FPQ_GEMM_CFG", cfg)
                y = gemm.linear_a6w4(a, sa, table, w, sw)
                n_bad = int((y.view(torch.int16) != exact.view(torch.int16)).sum())
                worst = float((y.double() - exact.double()).abs().max())
                print(f"{table} {name} sw={ws_dtype} cfg={cfg}: {n_bad} of {y.numel()} differ, max |err| {worst:g}")
                assert n_bad == 0, (table, name, cfg, n_bad, worst)


@pytest.mark.parametrize("table", TABLES)
def test_families_over_the_shape_sweep(dev, table, lib_options):
    """gm.shape_sweep() for both weight-scale dtypes, both tilings and the default: every output within ALLOWANCE x gm.bound of
    the float64 product with the exact non-finite pattern, bit-equal to emulate(), the tilings bit-equal to each other."""
    from fpqvar_amd import gemm
    worst, bad = {}, []
    for i, (family, T, O, K) in enumerate(gm.shape_sweep(families=am.FAMILIES)):
        K = min(K, gm.FP4_MAX_K)
        c = _on(am.make_case(table, family, T, O, K), dev)
        variants = [c["w_scales"]] + ([c["w_scales"].half()] if c["w_scales"].dtype == torch.float32 and i % 2 == 0 else [])
        for ws in variants:
            cv = dict(c, w_scales=ws)
            key = f"{table} {family}" + (" w16" if ws.dtype == torch.float16 else "")
            r = am.reference(table, *_args(cv))
            emu = am.emulate(table, *_args(cv))
            first = None
            for cfg in CFGS:
                lib_options("FPQ_GEMM_CFG", cfg)
                y = _lin(gemm, table, cv)
                what = f"cfg {cfg} T={T} O={O} K={K}"
                rat = gm.ratio(y, r)
                worst[key] = max(worst.get(key, 0.0), rat)
                if not rat <= ALLOWANCE:
                    bad.append((key, what, rat))
                if not _same_bits(y, emu):
                    bad.append((key, what, f"{int((y.view(torch.int16) != emu.view(torch.int16)).sum())} elements differ from emulate()"))
                if first is None:
                    first = y
                elif not _same_bits(y, first):
                    bad.append((key, what, "tilings differ"))
                if family == "zero":
                    want = cv["bias"].view(1, O).expand_as(y) if cv["bias"] is not None else torch.zeros_like(y)
                    if not _same_bits(y, want.contiguous()):
                        bad.append((key, what, "zero family: output is not exactly fp16(bias) / +0"))
    lib_options("FPQ_GEMM_CFG", None)
    print(f"\n{table} families: max err / bound")
    for key, rat in sorted(worst.items(), key=lambda kv: -kv[1]):
        print(f"  {key:34s} {rat:.3f}")
    assert not bad, f"{len(bad)} failures, first {bad[:8]}"
    c = _on(am.make_case(table, "gauss", 4, 8, 9216), dev)
    with pytest.raises(RuntimeError):
        _lin(gemm, table, c)


@pytest.mark.parametrize("table", TABLES)
def test_ragged_tokens_and_output_edges(dev, table, lib_options):
    from fpqvar_amd import gemm
    for T in (1, 63, 100, 129):
        for O in (8, 72, 136, 264):
            c = _on(am.make_case(table, "gauss", T, O, 384, seed=3), dev)
            r = am.reference(table, *_args(c))
            emu = am.emulate(table, *_args(c))
            for cfg in CFGS:
                lib_options("FPQ_GEMM_CFG", cfg)
                y = _lin(gemm, table, c)
                assert y.shape == (T, O) and gm.ratio(y, r) <= ALLOWANCE and _same_bits(y, emu), (table, T, O, cfg)


@pytest.mark.parametrize("table", TABLES)
def test_bias_gate_residual_tails(dev, table, lib_options):
    """gate / residual in the epilogue == the two torch ops on the plain output, bit for bit; a bias at an address that is not
    16-byte aligned is taken (copied)."""
    from fpqvar_amd import gemm
    g = torch.Generator().manual_seed(77)
    for T, O, K, B in ((300, 392, 384, 6), (2048, 1928, 256, 8), (64, 128, 1920, 1)):
        c = _on(am.make_case(table, "gauss", T, O, K, seed=5), dev)
        bias_store = (torch.randn(O + 4, generator=g) * 0.1).half().to(dev)
        gate = torch.randn(B, 1, O, generator=g).half().to(dev)
        resid = torch.randn(T, O, generator=g).half().to(dev)
        for bias in (c["bias"], bias_store[1:O + 1], None):
            cv = dict(c, bias=bias)
            for cfg in CFGS:
                lib_options("FPQ_GEMM_CFG", cfg)
                plain = _lin(gemm, table, cv)
                assert _same_bits(plain, am.emulate(table, *_args(cv))), (table, T, O, cfg, "bias")
                fused = _lin(gemm, table, cv, gate=gate, residual=resid)
                want = resid + (plain.view(B, T // B, O) * gate).view(T, O)
                assert _same_bits(fused, want), (table, T, O, cfg, "gate + residual")
                assert _same_bits(_lin(gemm, table, cv, gate=gate), (plain.view(B, T // B, O) * gate).view(T, O)), (table, T, O, cfg, "gate")
                assert _same_bits(_lin(gemm, table, cv, residual=resid), resid + plain), (table, T, O, cfg, "residual")


@pytest.mark.parametrize("table", TABLES)
def test_against_the_references_fp16_path(dev, table):
    """The reference's own result, F.linear(fake_quant(x).half(), W_q) - an fp16 GEMM on de-quantized tensors - within the looser
    relation tests/test_gpu_parity.py holds the FP4 GEMM to against that path; and the emitter's operands through the GEMM inside
    the bound."""
    from fpqvar_amd import gemm, ops
    for T, O, K in ((256, 256, 1920), (1000, 5760, 1920), (130, 1928, 256), (323, 9216, 2304)):
        g = torch.Generator().manual_seed(102 + T)
        x = (torch.randn(T, K, generator=g) * torch.exp(0.3 * torch.randn(T, K, generator=g))).half().to(dev)
        w = (torch.randn(O, K, generator=g) * 0.02).to(dev)
        bias = (torch.randn(O, generator=g) * 0.1).half().to(dev)
        ac, asc = gemm.quantize_g6(x, table)
        wc, wsc = gemm.quantize_mx(w)
        y = gemm.linear_a6w4(ac, asc, table, wc, wsc, bias)
        assert gm.ratio(y, am.reference(table, ac, asc, wc, wsc, bias)) <= ALLOWANCE
        a64, w64 = gemm.dequantize_g6(ac, asc, table).double(), gemm.dequantize_mx(wc, wsc).double()
        ref = a64 @ w64.t() + bias.double()
        tol = 2.0 ** -10 * ref.abs() + 1e-5 * (a64.abs() @ w64.abs().t()) + 1e-6
        assert bool(((y.double() - ref).abs() <= tol).all())
        y_ref = torch.nn.functional.linear(ops.quant_rows(x, table, 128), ops.quant_rows(w, "e2m1", 128).half(), bias)
        err = (y.float() - y_ref.float()).abs()
        lim = 2e-2 * y_ref.float().abs() + 2e-3 * (a64.abs() @ w64.abs().t()).float() + 1e-3
        assert bool((err <= lim).all()), float((err / lim).max())


# ------------------------------------------------------------------------------------------------------------ the modules
@pytest.mark.parametrize("act", ("fp_e1", "fp_e3"))
def test_fp4linear_with_a_6bit_activation(dev, act):
    from fpqvar_amd import gemm
    table = {"fp_e1": "e1m2", "fp_e3": "e3m0"}[act]
    g = torch.Generator().manual_seed(7)
    lin = torch.nn.Linear(256, 392)
    with torch.no_grad():
        lin.weight.copy_(torch.randn(392, 256, generator=g) * 0.05)
        lin.bias.copy_(torch.randn(392, generator=g) * 0.1)
    lin = lin.to(dev)
    m = gemm.FP4Linear.from_float(lin, act_fp_type=act)
    m4 = gemm.FP4Linear.from_float(lin)
    assert m.act_table == table and m4.act_table == "e2m1" and not m.kmajor
    assert torch.equal(m.w_codes, m4.w_codes) and torch.equal(m.w_scales, m4.w_scales)      # one stored weight serves both GEMMs
    x = torch.randn(2, 35, 256, generator=g).half().to(dev)
    y = m(x)
    ac, asc = gemm.quantize_g6(x.view(-1, 256), table)
    want = gemm.linear_a6w4(ac, asc, table, m.w_codes, m.w_scales, m.bias)
    assert y.shape == (2, 35, 392) and _same_bits(y.view(-1, 392), want)
    assert _same_bits(m.forward_operands(ac, asc), want) and _same_bits(m4.forward_operands(ac, asc, table=table), want)
    a4 = gemm.quantize_mx(x.view(-1, 256))
    assert _same_bits(m.forward_operands(*a4, table="fp_e2"), m4(x).view(-1, 392))
    with pytest.raises(ValueError):
        gemm.FP4Linear.from_float(lin, kmajor=True, act_fp_type=act)


class _Ffn(torch.nn.Module):
    def __init__(self, c):
        super().__init__()
        self.fc1, self.act, self.fc2 = torch.nn.Linear(c, 4 * c), torch.nn.GELU(approximate="tanh"), torch.nn.Linear(4 * c, c)

    def forward(self, x):
        return self.fc2(self.act(self.fc1(x)))


class _Attn(torch.nn.Module):
    def __init__(self, c):
        super().__init__()
        self.mat_qkv, self.proj = torch.nn.Linear(c, 3 * c, bias=False), torch.nn.Linear(c, c)


class _Block(torch.nn.Module):
    def __init__(self, c):
        super().__init__()
        self.attn, self.ffn = _Attn(c), _Ffn(c)
        self.ada_lin = torch.nn.Sequential(torch.nn.SiLU(), torch.nn.Linear(c, 6 * c))


class _Var(torch.nn.Module):
    def __init__(self, c, depth):
        super().__init__()
        self.blocks = torch.nn.ModuleList(_Block(c) for _ in range(depth))


def test_mixed_fp4_model_on_the_matrix_cores(dev):
    """A toy VAR of two blocks (block 0: fc1 E3M0, mat_qkv E2M1; block 1: fc1 and mat_qkv E3M0 - the reference's table for those
    indices): real_fp4=True yields FP4Linear exactly where the format table says, and fc1's output stays within the GEMM bound
    of the fake-quant model's operands."""
    from fpqvar_amd import gemm, quant_linear as ql
    C = 256
    torch.manual_seed(11)
    kw = dict(weight_quant="per_group", act_quant="per_group", w_bit=4, a_bit=4, activation_fp_quant=True, weight_fp_quant=True,
              act_fp_type="fp_e2", weight_fp_type="fp_e2", fc2_fp_type="fp_e1m2_neg_e2m1_pos")
    base = _Var(C, 2).to(dev)
    import copy
    fake = ql.quantize_VAR_mixed_fp4_datatype(copy.deepcopy(base), **kw)
    real = ql.quantize_VAR_mixed_fp4_datatype(copy.deepcopy(base), real_fp4=True, **kw)
    want = {"blocks.0.ffn.fc1": "e3m0", "blocks.0.attn.mat_qkv": "e2m1", "blocks.0.attn.proj": "e2m1",
            "blocks.1.ffn.fc1": "e3m0", "blocks.1.attn.mat_qkv": "e3m0", "blocks.1.attn.proj": "e2m1"}
    got = {n: m.act_table for n, m in real.named_modules() if isinstance(m, gemm.FP4Linear)}
    assert got == want, got
    for b in range(2):
        assert type(real.blocks[b].ffn.fc2) is ql.QuantizedLinear_fc2 and type(real.blocks[b].ada_lin[1]) is ql.QuantizedLinear
        assert real.blocks[b].attn.mat_qkv.kmajor == (b == 0) and not real.blocks[b].ffn.fc1.kmajor
    x = torch.randn(3, 50, C, device=dev).half()
    fake, real = fake.half(), real.half()
    for b in range(2):
        for path in ("ffn.fc1", "attn.mat_qkv"):
            mf, mr = fake.blocks[b].get_submodule(path), real.blocks[b].get_submodule(path)
            if mr.act_table == "e2m1":
                continue
            y_fake, y_real = mf(x).view(-1, mr.out_features), mr(x).view(-1, mr.out_features)
            ac, asc = gemm.quantize_g6(x.view(-1, C), mr.act_table)
            # the fake-quant layer multiplies the same de-quantized operands in fp16: the bound of the exact product of those
            # operands, plus the fp16 GEMM's own error (2^-10 relative on the sum of magnitudes, as tests/test_gpu_parity.py allows it)
            r = am.reference(mr.act_table, ac, asc, mr.w_codes, mr.w_scales, mr.bias)
            assert gm.ratio(y_real, r) <= ALLOWANCE
            a64, w64 = gemm.dequantize_g6(ac, asc, mr.act_table).double(), gemm.dequantize_mx(mr.w_codes, mr.w_scales).double()
            lim = gm.bound(r) + 2.0 ** -10 * (a64.abs() @ w64.abs().t()) + 2.0 ** -10 * r.out.abs()
            assert bool(((y_fake.double() - r.out).abs() <= lim).all()), (b, path)
