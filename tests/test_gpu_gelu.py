"""gelu_tanh_fast (fpqvar_amd/csrc/fpq_fast16.h) against its float64 definition, on every fp16 input, in every kernel it is compiled
into: the fc1 epilogue of the FP4 GEMM at each tiling and in both operand layouts, and the three stand-alone kernels of
fpq_gelu_quant_rows_dual (sub-wave groups, the U = 4 big-table form, one workgroup per row).  tests/gelu_model.py holds the
reference, the bound (derived from torch's op sequence; torch on this GPU is held to it here too) and what it was shown to
catch (tests/test_gelu_model_host.py).

The A6W4, W6 and GF6 fc1 tests take the FP4 epilogue's GELU values as their table; this file is what says the table is right:
  - every instantiation within the bound of the definition, with the definition's NaN / inf / signed-zero pattern;
  - all of them the same bits (input -0 apart: only the stand-alone kernels ever see it);
  - the epilogue a pure function of the fp16 Linear output, h == table[bits(y)], at every fragment slot of every tile shape.
tools/gelu_float64.py records the measured figures (profiles/gelu_float64.txt)."""
import pytest
import torch
import torch.nn.functional as Fn

from tests import gelu_model as gm
from tests.conftest import assert_bits_equal

pytestmark = pytest.mark.gpu

K = 128
CFGS = (None, 10, 20, 30, 40)                     # FPQ_GEMM_CFG: the library's choice, 256 / 128 / 64 x 128 LDS-DMA tiles, the deep ring
NEG_ZERO = 0x8000


# ---- the instantiations: name -> f(dev, set_option) -> (the fp16 inputs the GELU saw [65536], its fp16 results [65536]) -----------
def _fc1(cfg, kmajor):
    def run(dev, set_option):
        """zero codes and unit scales (every product is 0), the pattern as the bias of its own output column: y = 0 + bias"""
        from fpqvar_amd import gemm
        set_option("FPQ_GEMM_CFG", cfg)
        every = gm.every_fp16(dev)
        a = (torch.zeros(4, K // 2, dtype=torch.uint8, device=dev), torch.ones(4, K // 128, dtype=torch.float16, device=dev))
        w = (torch.zeros(65536, K // 2, dtype=torch.uint8, device=dev), torch.ones(65536, K // 128, dtype=torch.float32, device=dev))
        if kmajor:
            a = (gemm.to_kmajor(a[0], 4), gemm.to_kmajor_scales(a[1]))
            w = (gemm.to_kmajor(w[0], 4, dealt=True), gemm.to_kmajor_scales(w[1], weight_side=True))
        y = gemm.linear_fp4(*a, *w, every)
        _, h = gemm.linear_fp4_gelu_dual(*a, *w, every, return_gelu=True)
        for t in range(1, 4):
            assert_bits_equal(h[t], h[0], f"row {t} of the all-inputs tile")
            assert_bits_equal(y[t], y[0], f"row {t} of the Linear output")
        return y[0].clone(), h[0].clone()
    return run


def _rows(neg, pos, cols, strength):
    def run(dev, set_option):
        """whole rows of `cols`: the 65536 patterns, then as many of them again as fill the last row"""
        from fpqvar_amd import ops
        every = gm.every_fp16(dev)
        rows = -(-65536 // cols)
        y = every.repeat(2)[: rows * cols].view(rows, cols).contiguous()
        _, h = ops.gelu_quant_rows_dual(y, neg, pos, cols, strength, return_gelu=True)
        assert_bits_equal(h.view(-1)[65536:], h.view(-1)[: rows * cols - 65536], "the padding repeats the first inputs")
        return every, h.view(-1)[:65536].clone()
    return run


EPILOGUE = {f"fc1 {'k-major' if km else 'row-major'} cfg {cfg}": _fc1(cfg, km) for km in (False, True) for cfg in CFGS}
STAND_ALONE = {
    "rows e1m2-/e2m1+ per group (sub-wave)": _rows("e1m2_neg", "e2m1_pos", 128, 1.0),
    "rows int-/e2m3+ per group (big table, U = 4)": _rows("int_neg", "e2m3_pos", 128, None),
    "rows int-/e2m3+ per token 1920 (workgroup per row)": _rows("int_neg", "e2m3_pos", 1920, None),
    "rows int-/e2m3+ per token 1000 (ragged row)": _rows("int_neg", "e2m3_pos", 1000, None),
}
INSTANTIATIONS = {**EPILOGUE, **STAND_ALONE}


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "these tests need the GPU"
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def computed():
    """name -> (inputs, results) on the CPU, each instantiation run once per module"""
    return {}


def table_of(name, dev, set_option, computed):
    if name not in computed:
        x, h = INSTANTIATIONS[name](dev, set_option)
        torch.cuda.synchronize()
        computed[name] = (x.cpu(), h.cpu())
    return computed[name]


def shared_table(dev, set_option, computed) -> torch.Tensor:
    """the 65536-entry table: the epilogue's (row-major, the library's tiling); its entry for -0, an input the all-inputs GEMM cannot
    produce (0 + -0 = +0) but a product that underflows to -0 can, from the stand-alone kernel"""
    table = table_of("fc1 row-major cfg None", dev, set_option, computed)[1].clone()
    table[NEG_ZERO] = table_of(next(iter(STAND_ALONE)), dev, set_option, computed)[1][NEG_ZERO]
    return table


# ---- against the definition -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(INSTANTIATIONS))
def test_every_input_through_every_instantiation(dev, lib_options, computed, name):
    """ratio <= 1 against gelu_model.reference / bound on all 65536 inputs, none excluded; NaN exactly at NaN and -inf, +inf at
    +inf, zeros of the definition's sign (every deep negative input gives -0)."""
    x, h = table_of(name, dev, lib_options, computed)
    every = gm.every_fp16()
    if name in EPILOGUE:
        assert_bits_equal(x, torch.where(every == 0, torch.zeros_like(every), every), "the Linear output is the bias (0 + -0 = +0)")
    else:
        assert_bits_equal(x, every, "the stand-alone kernels read the pattern itself")
    bad = gm.class_mismatch(h, x)
    assert not bool(bad.any()), (name, x[bad][:8].tolist(), h[bad][:8].tolist())
    r = gm.ratios(h, x)
    worst = int(r.argmax())
    print(f"{name}: worst ratio {float(r[worst]):.4f} at x = {float(x[worst])!r}")
    assert gm.ratio(h, x) <= 1.0, (name, float(r[worst]), float(x[worst]), float(h[worst]))


def test_the_reference_on_this_gpu(dev):
    """torch's F.gelu(approximate="tanh") on the device - the comparator of the one-ulp parity tests - is itself inside the bound
    that was derived from its op sequence, so the bound owes nothing to the kernel."""
    every = gm.every_fp16(dev)
    out = Fn.gelu(every, approximate="tanh").cpu()
    x = every.cpu()
    bad = gm.class_mismatch(out, x)
    assert not bool(bad.any()), (x[bad][:8].tolist(), out[bad][:8].tolist())
    r = gm.ratios(out, x)
    worst = int(r.argmax())
    print(f"torch on the GPU: worst ratio {float(r[worst]):.4f} at x = {float(x[worst])!r}")
    assert gm.ratio(out, x) <= 1.0, (float(r[worst]), float(x[worst]), float(out[worst]))


# ---- against each other -----------------------------------------------------------------------------------------------------------------
def test_all_instantiations_give_the_same_bits(dev, lib_options, computed):
    """One function of the fp16 input, whichever kernel: every table equals the first bit for bit.  The one exception is the entry
    of input -0: the stand-alone kernels return -0 (as the definition does), the epilogue's all-inputs GEMM never sees -0."""
    first_name = next(iter(EPILOGUE))
    first = table_of(first_name, dev, lib_options, computed)[1]
    for name in INSTANTIATIONS:
        x, h = table_of(name, dev, lib_options, computed)
        if name in STAND_ALONE:
            assert int(gm.bits(x)[NEG_ZERO]) == NEG_ZERO and int(gm.bits(h)[NEG_ZERO]) == NEG_ZERO, f"{name}: gelu(-0) must be -0"
            h = h.clone()
            h[NEG_ZERO] = first[NEG_ZERO]
        else:
            assert int(gm.bits(x)[NEG_ZERO]) == 0 and int(gm.bits(h)[NEG_ZERO]) == 0, f"{name}: 0 + -0 is +0, and gelu(+0) is +0"
        assert_bits_equal(h, first, f"{name} vs {first_name}")


@pytest.mark.parametrize("kmajor", [False, True], ids=["row-major", "k-major"])
def test_position_independence_exact(dev, lib_options, computed, kmajor):
    """h == table[bits(y)] bit for bit, y = linear_fp4(...) of random operands and bias: the epilogue's GELU depends on the fp16
    Linear output alone, not on the fragment slot that holds it.  T = 1, 70, 130, 300 x O = 128, 384 at every tiling: every slot
    (m, n, i) of the 64-, 128- and 256-row tiles, more than one tile, and the ragged last one."""
    from fpqvar_amd import gemm
    table = shared_table(dev, lib_options, computed).to(dev)
    lowest = 0.0
    for T in (1, 70, 130, 300):
        for O in (128, 384):
            g = torch.Generator().manual_seed(1000 * T + O)
            x = (torch.randn(T, 256, generator=g) * torch.exp(0.3 * torch.randn(T, 256, generator=g))).half().to(dev)
            w = (torch.randn(O, 256, generator=g) * 0.15).to(dev)                 # y spreads over +-8: the deep negatives included
            bias = (torch.randn(O, generator=g) * 0.5).half().to(dev)
            a, wq = gemm.quantize_mx(x), gemm.quantize_mx(w)
            if kmajor:
                a = (gemm.to_kmajor(a[0], 4), gemm.to_kmajor_scales(a[1]))
                wq = (gemm.to_kmajor(wq[0], 4, dealt=True), gemm.to_kmajor_scales(wq[1], weight_side=True))
            for cfg in CFGS:
                lib_options("FPQ_GEMM_CFG", cfg)
                for b in (bias, None):
                    y = gemm.linear_fp4(*a, *wq, b)
                    _, h = gemm.linear_fp4_gelu_dual(*a, *wq, b, return_gelu=True)
                    assert y.shape == h.shape == (T, O)
                    assert_bits_equal(h, table[gm.bits(y)], f"T {T} O {O} cfg {cfg} bias {b is not None}: h vs table[bits(y)]")
                    lowest = min(lowest, float(y.float().min()))
    assert lowest < -5.2, "the cases do not reach the deep negatives, where the snap acts"
