"""E1M2 / E3M0 weights as 6-bit codes on the matrix cores (gemm.linear_w6, fpq_gemm_w6_mx) against every FP4 activation format: the
GEMM against the float64 reference, bound and fp32 model of tests/w6_model.py, and the modules built on it (gemm.FP4Linear with
weight_fp_type, quant_linear.quantize_VAR_mixed(real_fp4=True, w6_weights=True)).

The numerics rest on one measurement, test_the_128_term_dot_is_exact: with K = 128, unit scales and no bias, dots that are fp16
numbers must come out bit for bit - the matrix core keeps every product of the two levels.  MEASURED on an MI355X
(profiles/w6_dot.txt): all 72 runs (6 pairs x 4 constructions x 3 tilings) bit-equal to the exact dot, E3M0 x E3M0 included, so every
pair has the FP4 GEMM's contract unchanged - allowance 1.0, bit-equal to the fp32 model; over the shape sweep the worst error is
1.000 x the bound (the fp16 output rounding)."""
import copy

import pytest
import torch

from tests import gemm_model as gm
from tests import w6_model as wm

pytestmark = pytest.mark.gpu

PAIRS = wm.PAIRS
CFGS = (20, 30, None)    # FPQ_GEMM_CFG: 128 x 128 tiles, 64 x 128 tiles, the library's choice
# x gm.bound per (activation, weight) pair.  1.0: the 128-term dot came out exact (profiles/w6_dot.txt: it did for all six), the
# contract is the FP4 GEMM's unchanged and the output is bit-equal to wm.emulate().  (A pair that were not exact would carry 1.5 x its
# measured worst ratio here, at most gm.WIDE_FP8_MEASURED, and be held to that instead of bit equality.)
ALLOWANCE = {p: 1.0 for p in PAIRS}
EXACT = {p: ALLOWANCE[p] == 1.0 for p in PAIRS}
IDS = [f"{a}-{w}" for a, w in PAIRS]


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "these tests need the GPU"
    return torch.device("cuda:0")


def _args(c):
    return c["a"], c["a_scales"], c["w"], c["w_scales"], c["bias"]


def _same_bits(x, y):
    """bit-equal, every NaN one value"""
    xn, yn = torch.isnan(x), torch.isnan(y)
    return bool(torch.equal(xn, yn)) and bool(torch.equal(x.masked_fill(xn, 0).view(torch.int16), y.masked_fill(yn, 0).view(torch.int16)))


def _lin(gemm, pair, c, **kw):
    return gemm.linear_w6(c["a"], c["a_scales"], pair[0], c["w"], c["w_scales"], pair[1], c["bias"], **kw)


def _quantize_a(gemm, table, x):
    return gemm.quantize_mx(x) if table == "e2m1" else gemm.quantize_g6(x, table)


def _dequantize_a(gemm, table, codes, scales):
    return gemm.dequantize_mx(codes, scales) if table == "e2m1" else gemm.dequantize_g6(codes, scales, table)


# ------------------------------------------------------------------------------------------------------------ the GEMM
@pytest.mark.parametrize("pair", PAIRS, ids=IDS)
def test_the_128_term_dot_is_exact(dev, pair, lib_options):
    """K = 128, unit scales, no bias, dots that are fp16 numbers (wm.exact_dot_cases: the largest products cancelling beside a few
    smallest ones, all 15 x 15 level pairs alone and 128-fold, the largest product beside 127 smallest): the output equals the
    exact value bit for bit, in both tilings and the default - for a pair that is not exact, within its allowance instead."""
    from fpqvar_amd import gemm
    at, wt = pair
    for name, (La, Lw) in wm.exact_dot_cases(at, wt).items():
        a, w = wm.encode_levels(at, La).to(dev), wm.encode_levels(wt, Lw).to(dev)
        sa = torch.ones(La.shape[0], 1, dtype=torch.float16, device=dev)
        sw = torch.ones(Lw.shape[0], 1, dtype=torch.float32, device=dev)
        exact = (La @ Lw.t()).half().to(dev)
        r = wm.reference(at, wt, a, sa, w, sw, None)
        for cfg in CFGS:
            lib_options("FPQ_GEMM_CFG", cfg)
            y = gemm.linear_w6(a, sa, at, w, sw, wt)
            n_bad = int((y.view(torch.int16) != exact.view(torch.int16)).sum())
            worst = float((y.double() - exact.double()).abs().max())
            rat = gm.ratio(y, r)
            print(f"{at} x {wt} {name} cfg={cfg}: {n_bad} of {y.numel()} differ, max |err| {worst:g}, err / bound {rat:.3f}")
            if EXACT[pair]:
                assert n_bad == 0, (pair, name, cfg, n_bad, worst)
            else:
                assert rat <= ALLOWANCE[pair], (pair, name, cfg, rat)


# gm.shape_sweep() with K capped at the GEMM's limit, in chunks of one T with every O: a case is a few seconds, and the six pairs of a
# chunk share its CPU-built base cases (wm.make_case caches them; the pair varies fastest)
SWEEP = [(f, T, O, min(K, gm.FP4_MAX_K)) for f, T, O, K in gm.shape_sweep(families=wm.FAMILIES)]
CHUNK = len(gm.O_SWEEP)
WORST = {}


@pytest.mark.parametrize("pair", PAIRS, ids=IDS)
@pytest.mark.parametrize("chunk", range(len(SWEEP) // CHUNK))
def test_families_over_the_shape_sweep(dev, pair, chunk, lib_options):
    """gm.shape_sweep() in both tilings and the default: every output within the pair's allowance x gm.bound of the float64
    product with the exact non-finite pattern, bit-equal to emulate() where the pair is exact, the tilings bit-equal to each
    other, the zero family exactly fp16(bias) / +0."""
    from fpqvar_amd import gemm
    at, wt = pair
    bad = []
    for family, T, O, K in SWEEP[chunk * CHUNK:(chunk + 1) * CHUNK]:
        c = wm.make_case(at, wt, family, T, O, K, device=dev)
        key = f"{at} x {wt} {family}"
        r = wm.reference(at, wt, *_args(c))
        emu = wm.emulate(at, wt, *_args(c)) if EXACT[pair] else None
        first = None
        for cfg in CFGS:
            lib_options("FPQ_GEMM_CFG", cfg)
            y = _lin(gemm, pair, c)
            what = f"cfg {cfg} T={T} O={O} K={K}"
            rat = gm.ratio(y, r)
            WORST[key] = max(WORST.get(key, 0.0), rat)
            if not rat <= ALLOWANCE[pair]:
                bad.append((key, what, rat))
            if int(gm.class_mismatch(y, r).sum()):
                bad.append((key, what, "non-finite pattern"))
            if emu is not None and not _same_bits(y, emu):
                bad.append((key, what, f"{int((y.view(torch.int16) != emu.view(torch.int16)).sum())} elements differ from emulate()"))
            if first is None:
                first = y
            elif not _same_bits(y, first):
                bad.append((key, what, "tilings differ"))
            if family == "zero":
                want = c["bias"].view(1, O).expand_as(y) if c["bias"] is not None else torch.zeros_like(y)
                if not _same_bits(y, want.contiguous()):
                    bad.append((key, what, "zero family: output is not exactly fp16(bias) / +0"))
    print(f"\n{at} x {wt} families so far: max err / bound " + ", ".join(f"{k.split()[-1]} {v:.3f}" for k, v in sorted(WORST.items()) if k.startswith(f"{at} x {wt} ")))
    assert not bad, f"{len(bad)} failures, first {bad[:8]}"


@pytest.mark.parametrize("pair", PAIRS, ids=IDS)
def test_k_above_the_limit_is_refused(dev, pair):
    from fpqvar_amd import gemm
    c = wm.make_case(*pair, "gauss", 4, 8, 9216, device=dev)
    with pytest.raises(RuntimeError):
        _lin(gemm, pair, c)


@pytest.mark.parametrize("pair", PAIRS, ids=IDS)
def test_ragged_tokens_and_output_edges(dev, pair, lib_options):
    """T x O at K = 384: the smallest shapes that cross a tile edge, a super-block edge and the last-row clamp on each side"""
    from fpqvar_amd import gemm
    at, wt = pair
    for T in (1, 63, 100, 129):
        for O in (8, 72, 136, 264):
            c = wm.make_case(at, wt, "gauss", T, O, 384, seed=3, device=dev)
            r = wm.reference(at, wt, *_args(c))
            emu = wm.emulate(at, wt, *_args(c))
            first = None
            for cfg in CFGS:
                lib_options("FPQ_GEMM_CFG", cfg)
                y = _lin(gemm, pair, c)
                assert y.shape == (T, O) and gm.ratio(y, r) <= ALLOWANCE[pair], (pair, T, O, cfg)
                assert not EXACT[pair] or _same_bits(y, emu), (pair, T, O, cfg)
                first = y if first is None else first
                assert _same_bits(y, first), (pair, T, O, cfg, "tilings differ")


@pytest.mark.parametrize("pair", PAIRS, ids=IDS)
def test_bias_gate_residual_tails(dev, pair, lib_options):
    """gate / residual in the epilogue == the two torch ops on the plain output, bit for bit; a bias at an odd 2-byte offset is
    taken (copied)."""
    from fpqvar_amd import gemm
    g = torch.Generator().manual_seed(77)
    for T, O, K, B in ((300, 392, 384, 6), (64, 128, 1920, 1)):
        c = wm.make_case(*pair, "gauss", T, O, K, seed=5, device=dev)
        bias_store = (torch.randn(O + 4, generator=g) * 0.1).half().to(dev)
        gate = torch.randn(B, 1, O, generator=g).half().to(dev)
        resid = torch.randn(T, O, generator=g).half().to(dev)
        for bias in (c["bias"], bias_store[1:O + 1], None):
            cv = dict(c, bias=bias)
            for cfg in CFGS:
                lib_options("FPQ_GEMM_CFG", cfg)
                plain = _lin(gemm, pair, cv)
                if EXACT[pair]:
                    assert _same_bits(plain, wm.emulate(*pair, *_args(cv))), (pair, T, O, cfg, "bias")
                else:
                    assert gm.ratio(plain, wm.reference(*pair, *_args(cv))) <= ALLOWANCE[pair], (pair, T, O, cfg, "bias")
                fused = _lin(gemm, pair, cv, gate=gate, residual=resid)
                want = resid + (plain.view(B, T // B, O) * gate).view(T, O)
                assert _same_bits(fused, want), (pair, T, O, cfg, "gate + residual")
                assert _same_bits(_lin(gemm, pair, cv, gate=gate), (plain.view(B, T // B, O) * gate).view(T, O)), (pair, T, O, cfg, "gate")
                assert _same_bits(_lin(gemm, pair, cv, residual=resid), resid + plain), (pair, T, O, cfg, "residual")


@pytest.mark.parametrize("pair", PAIRS, ids=IDS)
def test_against_the_fake_quant_path(dev, pair):
    """The reference's own result, F.linear(fake_quant(x), fake_quant(W).half(), bias) - an fp16 GEMM on de-quantized tensors -
    within the looser relation tests/test_gpu_a6w4.py::test_against_the_references_fp16_path holds the A6W4 GEMM to against that
    path; and the quantizers' operands through the GEMM inside the bound."""
    from fpqvar_amd import gemm, ops
    at, wt = pair
    for T, O, K in ((256, 256, 1920), (130, 1928, 256)):
        g = torch.Generator().manual_seed(102 + T)
        x = (torch.randn(T, K, generator=g) * torch.exp(0.3 * torch.randn(T, K, generator=g))).half().to(dev)
        w = (torch.randn(O, K, generator=g) * 0.02).to(dev)
        bias = (torch.randn(O, generator=g) * 0.1).half().to(dev)
        ac, asc = _quantize_a(gemm, at, x)
        wc, wsc = gemm.quantize_g6(w, wt)
        assert wsc.dtype == torch.float32 and wc.shape == (O, K * 3 // 4)
        y = gemm.linear_w6(ac, asc, at, wc, wsc, wt, bias)
        assert gm.ratio(y, wm.reference(at, wt, ac, asc, wc, wsc, bias)) <= ALLOWANCE[pair]
        a64, w64 = _dequantize_a(gemm, at, ac, asc).double(), gemm.dequantize_g6(wc, wsc, wt).double()
        y_ref = torch.nn.functional.linear(ops.quant_rows(x, at, 128), ops.quant_rows(w, wt, 128).half(), bias)
        err = (y.float() - y_ref.float()).abs()
        lim = 2e-2 * y_ref.float().abs() + 2e-3 * (a64.abs() @ w64.abs().t()).float() + 1e-3
        assert bool((err <= lim).all()), float((err / lim).max())


# ------------------------------------------------------------------------------------------------------------ the modules
FP_NAME = {"e2m1": "fp_e2", "e1m2": "fp_e1", "e3m0": "fp_e3"}


@pytest.mark.parametrize("pair", PAIRS, ids=IDS)
def test_fp4linear_with_a_6bit_weight(dev, pair):
    """FP4Linear.from_float(..., weight_fp_type=...): the weight is quantize_g6's codes and fp32 scales, forward is linear_w6 on the
    module's own operands bit for bit, whatever float dtype the model is cast to"""
    from fpqvar_amd import gemm
    at, wt = pair
    g = torch.Generator().manual_seed(7)
    lin = torch.nn.Linear(256, 392)
    with torch.no_grad():
        lin.weight.copy_(torch.randn(392, 256, generator=g) * 0.05)
        lin.bias.copy_(torch.randn(392, generator=g) * 0.1)
    lin = lin.to(dev)
    m = gemm.FP4Linear.from_float(lin, act_fp_type=FP_NAME[at], weight_fp_type=FP_NAME[wt]).half()
    wc, wsc = gemm.quantize_g6(lin.weight.detach().float(), wt)
    assert (m.act_table, m.w_table) == pair and not m.kmajor and f"act={at}, w={wt}" in m.extra_repr()
    assert torch.equal(m.w_codes, wc) and torch.equal(m.w_scales, wsc) and m.w_scales.dtype == torch.float32
    x = torch.randn(2, 35, 256, generator=g).half().to(dev)
    y = m(x)
    ac, asc = _quantize_a(gemm, at, x.view(-1, 256))
    want = gemm.linear_w6(ac, asc, at, m.w_codes, m.w_scales, wt, m.bias)
    assert y.shape == (2, 35, 392) and _same_bits(y.view(-1, 392), want)
    assert _same_bits(m.forward_operands(ac, asc), want)
    gate, resid = torch.randn(2, 1, 392, generator=g).half().to(dev), torch.randn(2, 35, 392, generator=g).half().to(dev)
    assert _same_bits(m(x, gate=gate, residual=resid), resid + y * gate)
    for other in wm.A_TABLES:                                               # operands of another activation format, named
        oc, osc = _quantize_a(gemm, other, x.view(-1, 256))
        assert _same_bits(m.forward_operands(oc, osc, table=FP_NAME[other]), gemm.linear_w6(oc, osc, other, m.w_codes, m.w_scales, wt, m.bias))


from tests.test_a6w4_host import _Var   # noqa: E402  (the toy VAR of the host tests)


def test_w6_model_on_the_matrix_cores(dev):
    """A toy VAR of two blocks whose format table gives fc1 / mat_qkv / proj the six 6-bit-weight pairs: with w6_weights=True
    every one of them is an FP4Linear of exactly that pair (without it a QuantizedLinear, as today), and each layer's output
    stays within the GEMM bound of the fake-quant model's operands."""
    from fpqvar_amd import gemm, quant_linear as ql
    C = 256
    torch.manual_seed(11)
    kw = dict(weight_quant="per_group", act_quant="per_group", w_bit=4, a_bit=4, activation_fp_quant=True, weight_fp_quant=True)
    table = {(0, "fc1"): ("fp_e2", "fp_e1"), (0, "mat_qkv"): ("fp_e2", "fp_e3"), (0, "proj"): ("fp_e1", "fp_e1"),
             (1, "fc1"): ("fp_e1", "fp_e3"), (1, "mat_qkv"): ("fp_e3", "fp_e1"), (1, "proj"): ("fp_e3", "fp_e3")}

    def fmt(b, layer):
        return table.get((b, layer), ("fp_e1m2_neg_e2m1_pos", "fp_e2"))
    base = _Var(C, 2).to(dev)
    fake = ql.quantize_VAR_mixed(copy.deepcopy(base), fmt, real_fp4=True, **kw)
    real = ql.quantize_VAR_mixed(copy.deepcopy(base), fmt, real_fp4=True, w6_weights=True, **kw)
    path = {"fc1": "ffn.fc1", "mat_qkv": "attn.mat_qkv", "proj": "attn.proj"}
    inv = {v: k for k, v in FP_NAME.items()}
    got = {n: (m.act_table, m.w_table) for n, m in real.named_modules() if isinstance(m, gemm.FP4Linear)}
    assert got == {f"blocks.{b}.{path[layer]}": (inv[a], inv[w]) for (b, layer), (a, w) in table.items()}, got
    assert not [n for n, m in fake.named_modules() if isinstance(m, gemm.FP4Linear)]
    for b in range(2):
        assert type(real.blocks[b].ffn.fc2) is ql.QuantizedLinear_fc2 and isinstance(real.blocks[b].ada_lin[1], torch.nn.Linear)
    x = torch.randn(3, 50, C, device=dev).half()
    fake, real = fake.half(), real.half()
    for (b, layer), (a, w) in table.items():
        mf, mr = fake.blocks[b].get_submodule(path[layer]), real.blocks[b].get_submodule(path[layer])
        assert type(mf) is ql.QuantizedLinear
        at, wt = inv[a], inv[w]
        y_fake, y_real = mf(x).view(-1, mr.out_features), mr(x).view(-1, mr.out_features)
        ac, asc = _quantize_a(gemm, at, x.view(-1, C))
        # the fake-quant layer multiplies the same de-quantized operands in fp16: the bound of the exact product of those operands,
        # plus the fp16 GEMM's own error (2^-10 relative on the sum of magnitudes, as tests/test_gpu_a6w4.py allows it)
        r = wm.reference(at, wt, ac, asc, mr.w_codes, mr.w_scales, mr.bias)
        assert gm.ratio(y_real, r) <= ALLOWANCE[at, wt], (b, layer)
        a64, w64 = _dequantize_a(gemm, at, ac, asc).double(), gemm.dequantize_g6(mr.w_codes, mr.w_scales, wt).double()
        lim = gm.bound(r) + 2.0 ** -10 * (a64.abs() @ w64.abs().t()) + 2.0 ** -10 * r.out.abs()
        assert bool(((y_fake.double() - r.out).abs() <= lim).all()), (b, layer)


def test_the_compiled_binding_makes_the_same_call(dev):
    """_native.linear_w6 (quant_cuda_ext.cpp) == gemm.linear_w6, tail included, a misaligned bias copied"""
    from fpqvar_amd import _lib, _native, gemm
    g = torch.Generator().manual_seed(5)
    for at, wt in (("e2m1", "e3m0"), ("e3m0", "e1m2")):
        c = wm.make_case(at, wt, "gauss", 70, 136, 256, seed=9, device=dev)
        bias = (torch.randn(140, generator=g) * 0.1).half().to(dev)[1:137]
        gate, resid = torch.randn(2, 1, 136, generator=g).half().to(dev), torch.randn(70, 136, generator=g).half().to(dev)
        ids = _lib.TABLE_IDS[at], _lib.TABLE_IDS[wt]
        want = gemm.linear_w6(c["a"], c["a_scales"], at, c["w"], c["w_scales"], wt, bias, gate, resid)
        got = _native.linear_w6(c["a"], c["a_scales"], ids[0], c["w"], c["w_scales"], ids[1], bias, gate, resid)
        assert _same_bits(got, want)
        assert _same_bits(_native.linear_w6(c["a"], c["a_scales"], ids[0], c["w"], c["w_scales"], ids[1]), gemm.linear_w6(*_args(c)[:2], at, *_args(c)[2:4], wt))
        with pytest.raises(RuntimeError):
            _native.linear_w6(c["a"], c["a_scales"], ids[0], c["w"], c["w_scales"], _lib.TABLE_IDS["e2m1"])
