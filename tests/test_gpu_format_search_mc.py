"""GPU: the format search with every candidate product on the matrix cores and its loss in the GEMM's epilogue
(search_layer(fused=True, matrix_cores=True), search_layers_fused / search_blocks_sharded_fused(matrix_cores=True)) on a seeded
layer of 5 samples of 3 .. 40 rows, C = 384, outs = 256 (tests/gemm_sqerr_model.py, search_layer_case).

- Each loss equals the one assembled from the plain matrix-core Linear of the pair plus ops.sqerr_rows_weighted, within the sum
  of the two derived bounds (both are sums of the same stored numbers in another order), and the winner is the same.
- Against fused=True - fake-quantized operands through torch's GEMM - no bound is derived: the two products are fp16 roundings
  of the same real number.  The REL = 2e-3 that tests/test_gpu_format_search_fused.py states as the search's contract between
  evaluation orders is asserted, the measured ratio is printed per pair, and the winner is compared because the layer's best
  pair leads by more than 2 REL (tests/test_gemm_sqerr_model_host.py).
  Measured on an MI355X (this layer, fp16 weight): |matrix cores - fused| / fused is at most 2.4e-4 for the pairs with an fp_e2
  or FP6 weight and 1.3e-4 .. 1.5e-3 for the pairs with an fp_e1 / fp_e3 weight - worst (fp_e1, fp_e2) at 1.51e-3 = 0.76 REL,
  then (fp_e3, fp_e3) at 1.20e-3.  The cause is the weight operand, not a GEMM: an fp16 weight's E1M2 / E3M0 codes are quantized
  from its fp32 copy (the W6 GEMM takes fp32 scales only), the fake-quantizer of fused=True works in fp16, and a few elements
  near a midpoint take the neighbouring level; both GEMMs match the exact product of their own operands, rounded once to fp16,
  in all but <= 29 of 24 320 elements.  (With every weight quantized from its fp32 copy (fp6_e2m3, fp6_e2m3) measured 2.3e-3:
  format_search._mc_operand quantizes the fp_e2 and FP6 weights in their own dtype for that reason.)"""
import pytest
import torch

from tests import gemm_sqerr_model as gm
from tests import sqerr_model as sm

pytestmark = pytest.mark.gpu

REL = 2e-3
F16, F32 = torch.float16, torch.float32


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


def _layer(dev, seed=gm.SEARCH_SEED, w_dtype=F16):
    xs, w = gm.search_layer_case(seed, w_dtype)
    return [x.to(dev) for x in xs], w.to(dev)


def _family(wf, af):
    return "f6_rows" if wf.startswith("fp6") else "w6" if wf != "fp_e2" else "a6w4" if af != "fp_e2" else "fp4"


def _plain(wf, af, a_op, w_op):
    from fpqvar_amd import gemm
    fam = _family(wf, af)
    if fam == "f6_rows":
        return gemm.linear_fp6(*a_op, *w_op, a_table=af, w_table=wf)
    if fam == "w6":
        return gemm.linear_w6(*a_op, af, *w_op, wf)
    if fam == "a6w4":
        return gemm.linear_a6w4(*a_op, af, *w_op)
    return gemm.linear_fp4(*a_op, *w_op)


@pytest.mark.parametrize("w_dtype", (F16, F32), ids=("w16", "w32"))
def test_losses_are_the_plain_linears_losses_and_the_winner_is_the_same(dev, w_dtype):
    from fpqvar_amd import format_search as fs, ops
    xs, w = _layer(dev, w_dtype=w_dtype)
    tokens, outs = sum(gm.SEARCH_ROWS), gm.SEARCH_OUTS
    x_all = torch.cat(xs)
    ref = x_all.to(w.dtype) @ w.t()
    w_row = fs.sample_row_weights(gm.SEARCH_ROWS, outs, dev)
    for formats in (fs.FP4_FORMATS, fs.FP6_FORMATS):
        wf_mc, af_mc, mc = fs.search_layer(xs, w, formats, fused=True, matrix_cores=True)
        assert set(mc) == {(a, b) for a in formats for b in formats}
        built = {}
        for wf in formats:
            w_op = fs._mc_operand(wf, w, True)
            for af in formats:
                y16 = _plain(wf, af, fs._mc_operand(af, x_all, False), w_op)
                two_step = float(ops.sqerr_rows_weighted(ref, y16.to(ref.dtype), w_row).cpu())   # (one dtype for both: exact)
                s64 = gm.reference(ref.cpu(), y16.cpu(), w_row.cpu())
                bm = gm.tile_rows(_family(wf, af), tokens, outs)
                rel1, floor1 = gm.bound(tokens, outs, bm, w.dtype, float(w_row.max()))
                rel2, floor2 = sm.bound(tokens, outs, w.dtype, float(w_row.max()))
                got = mc[(wf, af)]
                print(f"w {w_dtype} ({wf}, {af}): matrix cores {got:.8g}  plain Linear + sqerr {two_step:.8g}  float64 {s64:.8g}  "
                      f"|diff| / bound {abs(got - two_step) / ((rel1 + rel2) * s64 + floor1 + floor2):.3g}")
                assert abs(got - s64) <= rel1 * s64 + floor1, (wf, af, got, s64)
                assert abs(got - two_step) <= (rel1 + rel2) * s64 + floor1 + floor2, (wf, af, got, two_step)
                built[(wf, af)] = two_step
        assert (wf_mc, af_mc) == fs.pick_winner([[built[(a, b)] for b in formats] for a in formats], formats)


def test_against_the_fused_form_of_fake_quantized_products(dev):
    from fpqvar_amd import format_search as fs
    xs, w = _layer(dev)
    for formats in (fs.FP4_FORMATS, fs.FP6_FORMATS):
        wf_mc, af_mc, mc = fs.search_layer(xs, w, formats, fused=True, matrix_cores=True)
        wf_f, af_f, fused = fs.search_layer(xs, w, formats, fused=True)
        worst = 0.0
        for key in fused:
            r = abs(mc[key] - fused[key]) / fused[key]
            worst = max(worst, r)
            print(f"{key}: matrix cores {mc[key]:.8g}  fused {fused[key]:.8g}  rel {r:.3g}  rel / REL {r / REL:.3g}")
        assert worst <= REL, (formats, worst)
        v = sorted(fused.values())
        assert (v[1] - v[0]) / v[0] >= 2 * REL, "the layer was chosen to have a clear winner in the fused table"
        assert (wf_mc, af_mc) == (wf_f, af_f)


def test_losses_out_layers_and_shards_bit_for_bit_without_a_synchronisation(dev):
    from fpqvar_amd import format_search as fs
    layers = [_layer(dev, s) for s in range(3)]
    for formats in (fs.FP4_FORMATS, fs.FP6_FORMATS):
        nf = len(formats)
        per_layer = [fs.search_layer(xs, w, formats, fused=True, matrix_cores=True) for xs, w in layers]   # (row weights now in place)
        torch.cuda.synchronize()
        torch.cuda.set_sync_debug_mode("error")
        try:
            table = fs.search_layers_fused(iter(layers), formats, matrix_cores=True)
            one = torch.full((nf, nf), -7.0, dtype=torch.float32, device=dev)
            assert fs.search_layer(*layers[0], formats, fused=True, losses_out=one, matrix_cores=True) is None
        finally:
            torch.cuda.set_sync_debug_mode("default")
        assert table.shape == (3, nf, nf) and table.dtype == torch.float32 and table.is_cuda
        host = table.cpu()
        for k, (wf, af, losses) in enumerate(per_layer):
            want = torch.tensor([[losses[(a, b)] for b in formats] for a in formats], dtype=torch.float32)
            assert torch.equal(host[k].view(torch.int32), want.view(torch.int32)), k
            assert fs.pick_winner(host[k], formats) == (wf, af)
        assert torch.equal(one.cpu().view(torch.int32), host[0].view(torch.int32))
        got = fs.search_blocks_sharded_fused(3, lambda b: layers[b], formats, matrix_cores=True)
        assert got == [(wf, af, float(torch.tensor(losses[(wf, af)], dtype=torch.float32))) for wf, af, losses in per_layer], got
        # the keyword is passed through: without it the same call gives the fake-quantized form's table
        assert not torch.equal(fs.search_layers_fused(layers[:1], formats).cpu(), host[:1])


def test_refusals_name_the_requirement(dev):
    from fpqvar_amd import format_search as fs
    xs, w = _layer(dev)
    with pytest.raises(RuntimeError, match="fused=True"):
        fs.search_layer(xs, w, fs.FP4_FORMATS, matrix_cores=True)
    with pytest.raises(RuntimeError, match="injected `quant` is refused"):
        fs.search_layer(xs, w, fs.FP4_FORMATS, quant=lambda f: fs.quantizer(f), batched=True, fused=True, matrix_cores=True)
    with pytest.raises(RuntimeError, match="float16 activations"):
        fs.search_layer([x.float() for x in xs], w, fs.FP4_FORMATS, fused=True, matrix_cores=True)
    with pytest.raises(RuntimeError, match="K % 128 == 0"):
        fs.search_layer([x[:, :320].contiguous() for x in xs], w[:, :320].contiguous(), fs.FP6_FORMATS, fused=True, matrix_cores=True)
    with pytest.raises(RuntimeError, match="not a mix"):
        fs.search_layer(xs, w, ("fp_e2", "fp6_e2m3"), fused=True, matrix_cores=True)
    out = torch.full((3, 3), -7.0, dtype=torch.float32, device=dev)
    with pytest.raises(RuntimeError, match="float16 activations"):
        fs.search_layer([x.float() for x in xs], w, fs.FP4_FORMATS, fused=True, losses_out=out, matrix_cores=True)
    assert bool((out.cpu() == -7.0).all()), "a refused call wrote its losses"
    # the defaults are unchanged: matrix_cores is off
    a, b = fs.search_layer(xs, w, fs.FP6_FORMATS, fused=True), fs.search_layer(xs, w, fs.FP6_FORMATS, fused=True, matrix_cores=False)
    assert a == b
