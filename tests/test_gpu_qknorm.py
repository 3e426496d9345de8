"""The q / k L2 norm of an attn_l2_norm block at every entry point that computes it - the split epilogues of the FP4, FP6 / BF6 and
A6W4 GEMMs (FPQ_QK_NORM_ROW) and the KV-cache step (kv16_step_qkn_kernel) - against the float64 reference and the per-element
bound of tests/qknorm_model.py, on every head family of the model in ONE launch per case: gaussian and heavy-tailed heads, one
dominant element (fp16-subnormal outputs), fp16-max and fp16-subnormal inputs, y16 ~ -bias, constant rows, norms below and on
either side of 1e-12, exact zeros, the head scale at its clamp and at 1e5 (finite and overflowing q), and heads with inf, +-inf,
NaN, inf and NaN.

Per case: err / bound <= 1 on every finite element of q and k, v bit for bit, non-finite elements exactly where the reference
has them, nothing written outside the destination slots, and within one GEMM family every tiling and layout bit-equal to the first.

The GEMMs get the families through rank-one operands (K = 128: activation row t = alpha_t on one channel, weight row o = beta_o on
the same channel, so y16[t, o] = half(alpha_t beta_o) is the plain GEMM's output for the same operands; the fp32 bias sets what a
product cannot; alpha = 40 overflows half(acc) to inf; one token's activation scale is NaN).  The KV step takes fp16 q / k / v
directly and gets every family as qknorm_model.make_case draws it.  C = 64 x 18 heads, 3 x 43 and 2 x 1 tokens: not the models' shapes.

Measured on an MI355X, worst err / bound: 0.9993 (the GEMMs), 0.9992 (the KV step) - the fp16 rounding is nearly all of the bound;
each test's docstring has its own figures.  The kernels before the residual step was guarded (fma(fma(-q, inf, y), 0, q) = NaN):
every case failed, and only on heads that hold an inf - 64 NaN where the reference has NaN at the inf elements and zeros beside
them (families inf and inf_pm; inf_nan without the bias that brings its NaN; dominant_3000 / dominant_60000 on the tokens whose
alpha overflows the dominant element) - with every other family at or below 0.9992."""
import pytest
import torch

from tests import qknorm_model as qm

pytestmark = pytest.mark.gpu

TOKENS = ((3, 43), (2, 1))                     # (batch, seq): 129 rows cross every tile height; one row per batch entry
S_H = 3.7
C, H = qm.C, qm.H


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "these tests need the GPU"
    return torch.device("cuda:0")


def _bits(t):
    """fp16 -> int16 bit patterns with every NaN one value"""
    t = t.contiguous()
    return torch.where(torch.isnan(t), torch.full_like(t, float("nan")), t).view(torch.int16)


def _rank_one(tokens, dev):
    """x fp16 [tokens, 128], w fp32 [3 C, 128] (channel 0 only), bias fp32 [3 C] (CPU), head scales, the NaN-scale token"""
    alpha, beta, bias, hs, nan_tok = qm.gemm_plan(tokens, S_H)
    x = torch.zeros(tokens, 128, dtype=torch.float16, device=dev)
    w = torch.zeros(3 * C, 128, dtype=torch.float32, device=dev)
    x[:, 0] = alpha.to(dev).half()
    w[:, 0] = beta.to(dev)
    return x, w, bias, hs, nan_tok


def _with_nan_scale(scales, nan_tok):
    if nan_tok is not None:
        scales = scales.clone()
        scales[nan_tok] = float("nan")
    return scales


def _check_case(what, q, k, v, y16, bias, hs, worst, bad):
    """q, k, v fp16 [T, C] as the kernel wrote them; y16 fp16 [T, 3 C] and bias fp32 [3 C] or None on the CPU"""
    T = y16.shape[0]
    for part, got in ((0, q), (1, k)):
        y, b = y16[:, part * C:(part + 1) * C], None if bias is None else bias[part * C:(part + 1) * C]
        assert float(qm.sum_of_squares(y, b).max()) < 2.0 ** 120 and qm.clear_of_overflow(y, b, hs, part), f"{what}: input conditions"
        ref, fin = qm.reference(y, b, hs, part)
        w, wrong = qm.check(got.reshape(T, C), ref, fin)
        for f, r in w.items():
            worst[f] = max(worst.get(f, 0.0), r)
            if r > 1.0:
                bad.append((what, "qk"[part], f, f"err / bound {r:.3g}"))
        if wrong:
            bad.append((what, "qk"[part], "non-finite elements are not where the reference has them", wrong))
    y, b = y16[:, 2 * C:], None if bias is None else bias[2 * C:]
    want_v = (y.float() + b).half() if b is not None else y
    if not torch.equal(_bits(v.reshape(T, C).cpu()), _bits(want_v)):
        bad.append((what, "v not bit for bit"))


def _report(name, worst, bad):
    print(f"\n{name}: worst err / bound " + ", ".join(f"{f} {worst[f]:.4f}" for f in qm.FAMILIES if f in worst))
    assert not bad, f"{len(bad)} failures, first {bad[:8]}"


def _run_gemm(name, dev, bsz, seq, with_bias, a_rm, w_rm, a_km, w_km, y16, bias, hs, call, option, cfgs, lib_options):
    """every tiling (cfgs of the switch `option`) x layout of one GEMM family on one operand pair"""
    y16c, bias_c = y16.cpu(), bias.cpu() if with_bias else None
    bias_d = bias.to(dev) if with_bias else None
    hs_d = hs.to(dev)
    max_len, pos = seq + 5, 3
    worst, bad, first = {}, [], None
    for cfg in cfgs:
        lib_options(option, cfg)
        for kmajor in (False, True):
            what = f"cfg={cfg} kmajor={kmajor}"
            cache = torch.full((2, bsz, max_len, H, 64), 7.5, dtype=torch.float16, device=dev)
            a, w = (a_km, w_km) if kmajor else (a_rm, w_rm)
            q = call(a, w, bias_d, cache, pos, seq, hs_d)
            assert q.shape == (bsz, seq, C) and q.dtype == torch.float16
            k, v = cache[0, :, pos:pos + seq], cache[1, :, pos:pos + seq]
            _check_case(what, q, k, v, y16c, bias_c, hs, worst, bad)
            keep = torch.ones(max_len, dtype=torch.bool, device=dev)
            keep[pos:pos + seq] = False
            if not bool((cache[:, :, keep] == 7.5).all()):
                bad.append((what, "wrote outside its slots"))
            if first is None:
                first = (what, _bits(q), _bits(cache))
            elif not (torch.equal(_bits(q), first[1]) and torch.equal(_bits(cache), first[2])):
                bad.append((what, f"bits differ from {first[0]}"))
    _report(name, worst, bad)


@pytest.mark.parametrize("with_bias", [False, True])
@pytest.mark.parametrize("bsz,seq", TOKENS)
def test_fp4_gemm(dev, bsz, seq, with_bias, lib_options):
    """gemm.linear_fp4_qkv_to_cache, FPQ_GEMM_CFG None / 10 / 20 / 30, row-major and k-major.
    Measured on an MI355X, worst err / bound: 0.9993 (a finite token row of the inf head); gauss 0.9970, heavy 0.9954, dominant
    0.9979, fp16_max 0.9955, subnormal 0.9887, cancel 0.9955, constant 0.7970, norm_tiny 0.9842, norm_straddle 0.9940, s_h = 100
    0.9967, s_h = 1e5 0.9909; all 8 tiling x layout runs of a case bit-equal."""
    from fpqvar_amd import gemm
    x, w, bias, hs, nan_tok = _rank_one(bsz * seq, dev)
    a_rm, w_rm = gemm.quantize_mx(x), gemm.quantize_mx(w)
    a_rm = (a_rm[0], _with_nan_scale(a_rm[1], nan_tok))
    a_km = (gemm.to_kmajor(a_rm[0], 4), gemm.to_kmajor_scales(a_rm[1]))
    w_km = (gemm.to_kmajor(w_rm[0], 4, dealt=True), gemm.to_kmajor_scales(w_rm[1], weight_side=True))
    y16 = gemm.linear_fp4(*a_rm, *w_rm)
    bias = qm.cancel_bias(bias, y16)
    _run_gemm("FP4 GEMM", dev, bsz, seq, with_bias, a_rm, w_rm, a_km, w_km, y16, bias, hs,
              lambda a, w, b, cache, pos, n, s: gemm.linear_fp4_qkv_to_cache(*a, *w, b, cache, pos, n, qk_norm_scale=s),
              "FPQ_GEMM_CFG", (None, 10, 20, 30), lib_options)


@pytest.mark.parametrize("a_table,w_table", [("e2m3", "e2m3"), ("e2m3", "e3m2"), ("e3m2", "e2m3"), ("e3m2", "e3m2")])
@pytest.mark.parametrize("with_bias", [False, True])
@pytest.mark.parametrize("bsz,seq", TOKENS)
def test_fp6_gemm(dev, bsz, seq, with_bias, a_table, w_table, lib_options):
    """gemm.linear_fp6_qkv_to_cache, FPQ_GEMM6_CFG None / 0 / 1, the four E2M3 / E3M2 operand pairs, row-major and k-major.
    Measured on an MI355X, worst err / bound over the four pairs: 0.9993; gauss 0.9973, heavy 0.9954, dominant 0.9979, fp16_max
    0.9955, subnormal 0.9941, cancel 0.9957, constant 0.7970, norm_tiny 0.9842, norm_straddle 0.9940, s_h = 100 0.9967, s_h = 1e5
    0.9900."""
    from fpqvar_amd import gemm
    x, w, bias, hs, nan_tok = _rank_one(bsz * seq, dev)
    a_rm, w_rm = gemm.quantize_fp6(x, table=a_table), gemm.quantize_fp6(w, table=w_table)
    a_rm = (a_rm[0], _with_nan_scale(a_rm[1], nan_tok))
    a_km, w_km = (gemm.to_kmajor(a_rm[0], 6), a_rm[1]), (gemm.to_kmajor(w_rm[0], 6, dealt=True), w_rm[1])
    y16 = gemm.linear_fp6(*a_rm, *w_rm, a_table=a_table, w_table=w_table)
    bias = qm.cancel_bias(bias, y16)
    _run_gemm(f"FP6 GEMM {a_table} x {w_table}", dev, bsz, seq, with_bias, a_rm, w_rm, a_km, w_km, y16, bias, hs,
              lambda a, w, b, cache, pos, n, s: gemm.linear_fp6_qkv_to_cache(*a, *w, b, cache, pos, n, qk_norm_scale=s, a_table=a_table,
                                                                             w_table=w_table),
              "FPQ_GEMM6_CFG", (None, 0, 1), lib_options)


@pytest.mark.parametrize("table", ["e3m0", "e1m2"])
@pytest.mark.parametrize("with_bias", [False, True])
@pytest.mark.parametrize("bsz,seq", TOKENS)
def test_a6w4_gemm(dev, bsz, seq, with_bias, table, lib_options):
    """gemm.linear_a6w4_qkv_to_cache, FPQ_GEMM_CFG None / 20 / 30, E3M0 and E1M2 activations, row-major and k-major.
    Measured on an MI355X, worst err / bound over both tables: 0.9993; gauss 0.9970, heavy 0.9956, dominant 0.9979, fp16_max
    0.9955, subnormal 0.9960, cancel 0.9955, constant 0.7970, norm_tiny 0.9842, norm_straddle 0.9940, s_h = 100 0.9967, s_h = 1e5
    0.9951."""
    from fpqvar_amd import gemm
    x, w, bias, hs, nan_tok = _rank_one(bsz * seq, dev)
    a_rm, w_rm = gemm.quantize_g6(x, table), gemm.quantize_mx(w)
    a_rm = (a_rm[0], _with_nan_scale(a_rm[1], nan_tok))
    a_km = (gemm.to_kmajor(a_rm[0], 6), gemm.to_kmajor_scales(a_rm[1]))
    w_km = (gemm.to_kmajor(w_rm[0], 4, dealt=True), gemm.to_kmajor_scales(w_rm[1], weight_side=True))
    y16 = gemm.linear_a6w4(*a_rm, table, *w_rm, None)
    bias = qm.cancel_bias(bias, y16)
    _run_gemm(f"A6W4 GEMM {table}", dev, bsz, seq, with_bias, a_rm, w_rm, a_km, w_km, y16, bias, hs,
              lambda a, w, b, cache, pos, n, s: gemm.linear_a6w4_qkv_to_cache(*a, table, *w, b, cache, pos, n, qk_norm_scale=s),
              "FPQ_GEMM_CFG", (None, 20, 30), lib_options)


@pytest.mark.parametrize("kv_bit", [6, 4])
@pytest.mark.parametrize("front", ["native", "ctypes"])
@pytest.mark.parametrize("with_bias", [False, True])
@pytest.mark.parametrize("bsz,seq", TOKENS)
def test_kv_step(dev, bsz, seq, with_bias, front, kv_bit, monkeypatch):
    """ops.kv_cache_step_qk_norm through the compiled binding and through ctypes, kv_bit 6 and 4, on strided q / k / v views of one
    buffer: every family as qknorm_model.make_case draws it, a fresh draw per token.
    Measured on an MI355X, worst err / bound: 0.9992 (dominant_60000); gauss 0.9975, heavy 0.9986, dominant_3000 0.9989, fp16_max
    0.9975, subnormal 0.9977, cancel 0.9979, constant 0.7970, norm_tiny 0.9842, norm_straddle 0.9944, s_h = 100 0.9975, s_h = 1e5
    0.9977; both fronts and both kv_bit give the same figures."""
    from fpqvar_amd import ops
    if front == "ctypes":
        monkeypatch.setattr(ops, "_native", None)
    elif ops._native is None:
        pytest.fail("the compiled binding did not load")
    T = bsz * seq
    y16, bias, hs = qm.make_case(T, S_H)
    bias = bias.reshape(-1) if with_bias else None
    prev, pos, max_len = 3, 7, 7 + seq + 5
    group, table = (64, "e2m3") if kv_bit == 6 else (128, "e2m1")
    g = torch.Generator().manual_seed(T)
    cache = (torch.randn(2, bsz, max_len, H, 64, generator=g) * 0.3).half().to(dev)
    plain = cache.clone()
    buf = torch.full((bsz, seq + 3, 3 * C + 24), 7.5, dtype=torch.float16)   # token and batch pitches that are not the rows'
    buf[:, 1:seq + 1, 8:8 + 3 * C] = y16.view(bsz, seq, 3 * C)
    buf = buf.to(dev)
    src = buf.clone()
    q, k, v = buf[:, 1:seq + 1, 8:8 + 3 * C].unflatten(-1, (3, H, 64)).unbind(2)
    q_out = ops.kv_cache_step_qk_norm(cache, prev, pos, q, k, v, pos, group, table, hs.to(dev), None if bias is None else bias.to(dev))
    assert q_out.shape == (bsz, seq, H, 64) and q_out.is_contiguous() and q_out.dtype == torch.float16
    empty = plain[0, :, :0]
    ops.kv_cache_step(plain, prev, pos, empty, empty, pos, group, table)
    worst, bad = {}, []
    _check_case(f"{front} kv_bit={kv_bit}", q_out, cache[0, :, pos:pos + seq], cache[1, :, pos:pos + seq], y16.view(T, 3 * C), bias, hs, worst, bad)
    if not torch.equal(_bits(cache[:, :, :pos]), _bits(plain[:, :, :pos])):
        bad.append("previous entries differ from fpq_kv_cache_step")
    if not torch.equal(_bits(cache[:, :, pos + seq:]), _bits(plain[:, :, pos + seq:])):
        bad.append("wrote past the new entries")
    if not torch.equal(_bits(buf), _bits(src)):
        bad.append("wrote to its source")
    _report(f"KV step {front} kv_bit={kv_bit}", worst, bad)
