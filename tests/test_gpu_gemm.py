"""The matrix-core GEMMs (gemm.linear_fp4 / linear_fp6 / linear_fp8) against the float64 reference and per-element bound of
tests/gemm_model.py, over every input family and a pairwise (T, O, K) sweep, in every tiling and operand layout; the FP4
tilings bit for bit against the fp32 model of their arithmetic.  Also the operands the quantizers emit for inputs holding
+-inf and NaN, and every GEMM call of a small GenerationBatch on path Q."""
import math

import pytest
import torch

from tests import gemm_model as gm

pytestmark = pytest.mark.gpu

FP4_CFGS = (0, 1, 2, 10, 20, 30, None)          # FPQ_GEMM_CFG: 0..2 register-staged, 10 / 20 / 30 LDS-DMA, None the default
INEXACT = ("max_codes", "e3m2", "e4m3_full")     # families whose fp6 / fp8 accumulator chain may round


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


def _note(worst, bad, key, what, out, r, limit=1.0):
    rat = gm.ratio(out, r)
    worst[key] = max(worst.get(key, 0.0), rat)
    if not rat <= limit:
        bad.append((key, what, rat))
    return rat


def _report(title, worst, bad, extra=None):
    print(f"\n{title}: max err / bound")
    for key, rat in sorted(worst.items(), key=lambda kv: -kv[1]):
        print(f"  {key:34s} {rat:.3f}" + (f"   {extra[key]}" if extra and key in extra else ""))
    assert not bad, f"{len(bad)} failures, first {bad[:8]}"


def _check_zero(bad, key, what, y, c):
    O = y.shape[1]
    want = c["bias"].view(1, O).expand_as(y) if c["bias"] is not None else torch.zeros_like(y)
    if not _same_bits(y, want.contiguous()):
        bad.append((key, what, "zero family: output is not exactly fp16(bias) / +0"))


def test_fp4_families_over_the_shape_sweep(dev, lib_options):
    """Every FPQ_GEMM_CFG on row-major operands, the LDS-DMA tilings on k-major images; fp32 weight scales everywhere, fp16 ones
    on every other case (and in fp16_w_scales).  Each output within the bound, with the exact non-finite pattern, and bit for
    bit what emulate() computes in its tiling's order.  K = 9216 is past the kernel's limit (K <= 8192, a shape error): those
    cases run at K = 8192, 64 groups, the longest accepted."""
    from fpqvar_amd import gemm
    worst, bad = {}, []
    for i, (family, T, O, K) in enumerate(gm.shape_sweep(families=gm.KIND_FAMILIES["fp4"])):
        K = min(K, gm.FP4_MAX_K)
        c = _on(gm.make_case("fp4", family, T, O, K), dev)
        variants = [c["w_scales"]] + ([c["w_scales"].half()] if c["w_scales"].dtype == torch.float32 and i % 2 == 0 else [])
        for ws in variants:
            cv = dict(c, w_scales=ws)
            key = f"fp4 {family}" + (" w16" if ws.dtype == torch.float16 else "")
            r = gm.reference("fp4", *_args(cv))
            emu = {order: gm.emulate("fp4", *_args(cv), order) for order in ("lds", "reg")}
            runs = []
            for cfg in FP4_CFGS:
                lib_options("FPQ_GEMM_CFG", cfg)
                runs.append((f"row-major cfg {cfg}", "reg" if cfg in (0, 1, 2) else "lds", gemm.linear_fp4(*_args(cv))))
            if ws.dtype == torch.float32:
                img = (gemm.to_kmajor(cv["a"], 4), gemm.to_kmajor_scales(cv["a_scales"]), gemm.to_kmajor(cv["w"], 4, dealt=True),
                       gemm.to_kmajor_scales(ws, weight_side=True))
                for cfg in (10, 20, 30, None):
                    lib_options("FPQ_GEMM_CFG", cfg)
                    runs.append((f"k-major cfg {cfg}", "lds", gemm.linear_fp4(*img, cv["bias"], outs=O)))
            for what, order, y in runs:
                what = f"{what} T={T} O={O} K={K}"
                _note(worst, bad, key, what, y, r)
                if not _same_bits(y, emu[order]):
                    n = int((y.view(torch.int16) != emu[order].view(torch.int16)).sum())
                    bad.append((key, what, f"{n} elements differ from emulate(order={order!r})"))
                if family == "zero":
                    _check_zero(bad, key, what, y, cv)
    lib_options("FPQ_GEMM_CFG", None)
    c = _on(gm.make_case("fp4", "gauss", 4, 8, 9216), dev)
    with pytest.raises(RuntimeError):
        gemm.linear_fp4(*_args(c))
    _report("fp4 families", worst, bad)


def _rows_emulation_agreement(agree, key, y, c, kind):
    """fraction of elements equal to the model with a nearest-even and with a truncating accumulator chain (information only:
    the bound does not rely on either)"""
    for mode in ("rne", "rtz"):
        e = gm.emulate(kind, *_args(c), acc_round=mode)
        eq = (y.view(torch.int16) == e.view(torch.int16)) | (torch.isnan(y) & torch.isnan(e))
        tot, hit = agree.get((key, mode), (0, 0))
        agree[(key, mode)] = (tot + eq.numel(), hit + int(eq.sum()))


def _agree_text(agree):
    out = {}
    for (key, mode), (tot, hit) in agree.items():
        out[key] = out.get(key, "") + f" {mode} {hit / max(tot, 1):.5f}"
    return out


def test_fp6_families_over_the_shape_sweep(dev, lib_options):
    """FPQ_GEMM6_CFG 0 and 1 on row-major operands and on k-major images: within the bound with the exact non-finite pattern, and
    all four bit-equal (the tilings share the K order and the epilogue)."""
    from fpqvar_amd import gemm
    worst, bad, agree = {}, [], {}
    for i, (family, T, O, K) in enumerate(gm.shape_sweep(families=gm.KIND_FAMILIES["fp6"])):
        c = _on(gm.make_case("fp6", family, T, O, K), dev)
        key = f"fp6 {family}"
        r = gm.reference("fp6", *_args(c))
        img = (gemm.to_kmajor(c["a"], 6), c["a_scales"], gemm.to_kmajor(c["w"], 6, dealt=True), c["w_scales"], c["bias"])
        runs = []
        for cfg in (0, 1):
            lib_options("FPQ_GEMM6_CFG", cfg)
            runs.append((f"row-major cfg {cfg}", gemm.linear_fp6(*_args(c))))
            runs.append((f"k-major cfg {cfg}", gemm.linear_fp6(*img)))
        for what, y in runs:
            what = f"{what} T={T} O={O} K={K}"
            _note(worst, bad, key, what, y, r)
            if not _same_bits(y, runs[0][1]):
                bad.append((key, what, "differs from row-major cfg 0"))
            if family == "zero":
                _check_zero(bad, key, what, y, c)
        if family in INEXACT or family == "gauss":
            _rows_emulation_agreement(agree, key, runs[0][1], c, "fp6")
    lib_options("FPQ_GEMM6_CFG", None)
    _report("fp6 families (agreement with the rne / rtz chain model)", worst, bad, _agree_text(agree))


def test_fp8_families_over_the_shape_sweep(dev, lib_options):
    """FPQ_GEMM8_CFG 0 and 1, with fp16 activation / fp32 weight scales and, rotating over the cases, each other combination of
    fp16 and fp32 on the two sides: within the bound with the exact non-finite pattern, both tilings bit-equal.  The E3M2 and
    full-range E4M3 families exceed the bound on this matrix core (gemm_model.bound): they are held to the measured
    WIDE_FP8_MEASURED x the bound, and the report shows how far they go."""
    from fpqvar_amd import gemm
    worst, bad, agree = {}, [], {}
    combos = ((torch.float32, torch.float32), (torch.float16, torch.float16), (torch.float32, torch.float16))
    for i, (family, T, O, K) in enumerate(gm.shape_sweep(families=gm.KIND_FAMILIES["fp8"])):
        c = _on(gm.make_case("fp8", family, T, O, K), dev)
        for da, dw in ((c["a_scales"].dtype, c["w_scales"].dtype), combos[i % 3]):
            cv = dict(c, a_scales=c["a_scales"].to(da), w_scales=c["w_scales"].to(dw))
            key = f"fp8 {family}"
            r = gm.reference("fp8", *_args(cv))
            ys = []
            for cfg in (0, 1):
                lib_options("FPQ_GEMM8_CFG", cfg)
                ys.append(gemm.linear_fp8(*_args(cv)))
                what = f"cfg {cfg} scales {da}/{dw} T={T} O={O} K={K}"
                _note(worst, bad, key, what, ys[-1], r, gm.WIDE_FP8_MEASURED if family in gm.WIDE_FP8 else 1.0)
                if family == "zero":
                    _check_zero(bad, key, what, ys[-1], cv)
            if not _same_bits(ys[0], ys[1]):
                bad.append((key, f"T={T} O={O} K={K}", "cfg 1 differs from cfg 0"))
        if family in INEXACT or family == "gauss":
            _rows_emulation_agreement(agree, key, ys[0], cv, "fp8")
    lib_options("FPQ_GEMM8_CFG", None)
    _report("fp8 families (agreement with the rne / rtz chain model)", worst, bad, _agree_text(agree))


def test_gemms_on_quantizer_output_with_non_finite_inputs(dev):
    """The operands quantize_mx / quantize_fp6 / quantize_fp8 emit for rows holding +inf, -inf and NaN: the GEMM output is
    non-finite exactly where the reference on those operands is, with the same class, and within the bound elsewhere."""
    from fpqvar_amd import gemm
    g = torch.Generator().manual_seed(9)
    T, O, K = 70, 136, 384
    x = torch.randn(T, K, generator=g)
    x[3, 5], x[10, 200], x[17, 300], x[17, 20] = math.inf, -math.inf, math.nan, math.inf
    w = torch.randn(O, K, generator=g) * 0.02
    w[7, 130], w[9, 2] = math.inf, math.nan
    bias = (torch.randn(O, generator=g) * 0.1).half().to(dev)
    xd, wd = x.half().to(dev), w.to(dev)
    worst, bad = {}, []
    for kind, quant, lin in (("fp4", gemm.quantize_mx, gemm.linear_fp4), ("fp6", gemm.quantize_fp6, gemm.linear_fp6),
                             ("fp8", gemm.quantize_fp8, gemm.linear_fp8)):
        (ac, asc), (wc, wsc) = quant(xd), quant(wd)
        r = gm.reference(kind, ac, asc, wc, wsc, bias)
        assert not bool(torch.isfinite(r.out).all()), kind
        _note(worst, bad, f"{kind} quantizer non-finite", "", lin(ac, asc, wc, wsc, bias), r)
    _report("quantizer output with +-inf / NaN inputs", worst, bad)


def _plain(kind, a, a_scales, w, w_scales, bias, out):
    """row-major operands of a call (k-major images converted back) -> (a, a_scales, w, w_scales)"""
    T, O = out.shape
    if a.dim() == 2:
        return a, a_scales, w, w_scales
    if kind == "fp4":
        return (gm.from_kmajor(a, 4, T), a_scales[:, :T].t().contiguous(), gm.from_kmajor(w, 4, O, dealt=True),
                w_scales[:, :O].t().contiguous())
    return gm.from_kmajor(a, 6, T), a_scales, gm.from_kmajor(w, 6, O, dealt=True), w_scales


@pytest.mark.parametrize("config", ("w4a4", "w6a6"))
def test_gemm_calls_of_the_model(dev, monkeypatch, config):
    """Every plain-GEMM call of a one-block GenerationBatch over its ten steps on path Q with attn_l2_norm, checked on the spot
    against the bound on the real activations (a call with a fused gate / residual is checked through its plain product)."""
    from fpqvar_amd import gemm, var_block
    worst, bad, n = {}, [], []

    def wrap(kind, real):
        def recording(a, a_scales, w, w_scales, bias=None, gate=None, residual=None, **kw):
            y = real(a, a_scales, w, w_scales, bias, **kw)
            ops = _plain(kind, a, a_scales, w, w_scales, bias, y)
            r = gm.reference(kind, *ops, bias)
            _note(worst, bad, f"{config} {kind} K={gm.decode(kind, ops[0][:1]).shape[1]}", f"T={y.shape[0]} O={y.shape[1]}", y, r)
            n.append(kind)
            return real(a, a_scales, w, w_scales, bias, gate, residual, **kw) if (gate is not None or residual is not None) else y
        return recording

    for kind, name in (("fp4", "linear_fp4"), ("fp6", "linear_fp6"), ("fp8", "linear_fp8")):
        monkeypatch.setattr(gemm, name, wrap(kind, getattr(gemm, name)))
    gb = var_block.GenerationBatch("d30-256", config, depth=1, batch_rows=2, device=dev, seed=4, attn_l2_norm=True)
    caches = gb.new_caches("Q")
    for pn in gb.patch_nums:
        assert torch.isfinite(gb.step("Q", caches, gb.new_input(pn))).all()
    assert len(n) >= len(gb.patch_nums), n
    _report(f"d30-256 {config} path Q GEMM calls", worst, bad)
