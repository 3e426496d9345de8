"""The three ways GenerationBatch.step runs the reference's AdaLN block - R (its own torch op sequence), F (fused producers around
fp16 Linears), Q (operands on the matrix cores) - held to ONE independent statement of the block: the float64 model of
tests/block_model.py, written from the reference's text.

Shape: "d30-256" with depth 2 (the smallest run with a pending residual across blocks), four rows, the first four scale steps
(1, 4, 9, 16 tokens per row: a cache in which one step's entries are quantized while older ones stay).  Every batch is built from
the same seed and its inputs from the same generator seed, so every path sees the same tensors (checked); the model runs once per
(config, attn_l2_norm) and is shared by the paths.

Measure: d = ||y - y_model|| / ||y_model - x|| over all elements of all four step outputs together (block_model.deviation): the
error relative to what the steps add to the residual stream.

Limits, none fixed in advance:
  d_F <= 2 d_R and d_Q <= 2 d_R, R from the same (config, attn_l2_norm).  R is the reference's op sequence on torch's own kernels:
    its distance from the float64 block is the rounding noise of fp16 GEMMs pushed through the four quantizers' level flips.  F and Q
    draw from the same source, but another draw: two draws that add in quadrature sit sqrt(2) apart (an estimate); the rest of the
    factor is headroom for these small shapes.
  resolution: the wiring mutants of the model, recomputed on the CPU at this test's own parameters (second step; the full run costs
    a second per mutant), must stand out of that noise: a mutant is resolved in a regime when its deviation is >= 4 d_R there - the
    limit 2 d_R is then at most half of it - and every mutant has to be resolved in at least one regime.  A path R that drifts from
    the model therefore cannot loosen the limits unnoticed: d_R grows, mutants stop being resolved, the test fails.
    (That is how this file found its first bug: every path attended at SDPA's head_dim ** -0.5 where the reference passes
    0.25 / sqrt(head_dim); d_R stood at 0.22 / 0.13 in the plain regimes, R, F and Q within 0.001 of each other.)

Measured on an MI355X (profiles/block_paths_vs_model.txt), aggregate over the four steps: d_R 0.105 / 0.116 / 0.033 / 0.035 for
w4a4 / w4a4+l2 / w6a6 / w6a6+l2, d_F 0.105 / 0.125 / 0.032 / 0.038, d_Q 0.117 / 0.129 / 0.035 / 0.039.  R and F share torch's fp16
GEMMs and sit at the same distance from the model; Q's GEMMs are another draw.  W4A4 is the noisier config (a level flip of a
3-bit magnitude is a large share of the value), so most mutants are resolved by the W6A6 regimes.  Five mutants move the update by
less than 4 d_R everywhere - a step-level comparison against a float64 block cannot see them through the quantizers' noise; they
stay in the printed table as UNRESOLVED, and COVERED_ELSEWHERE names the test that does catch each of them.
"""
import functools
from types import SimpleNamespace

import pytest
import torch

from tests import block_model as bm

pytestmark = pytest.mark.gpu

MODEL, DEPTH, ROWS, N_STEPS = "d30-256", 2, 4, 4
SEED, INPUT_SEED = 3, 11
REGIMES = [(config, l2) for config in ("w4a4", "w6a6") for l2 in (False, True)]
FACTOR, RESOLVED = 2.0, 4.0
# mutants that no regime resolves (second-step deviation / 4 d_R at its best: 0.54, 0.74, 0.27, 0.34, 0.30), and what pins them instead
COVERED_ELSEWHERE = {
    "block1_reads_cache0": "test_gpu_block_step.py::test_call_trace - every cache-facing call names the slab of the block's OWN cache",
    "bias_dropped": "test_gpu_qk_l2norm.py::test_generation_batch_fused_vs_torch_norm - v without its bias fails the cache agreement",
    "clamp_dropped": "test_gpu_qknorm.py (head scale at its clamp) and test_gpu_qk_l2norm.py::test_split_gemm_edge_rows",
    "kv_quant_skipped": "test_gpu_parity.py::test_incremental_kv_equals_requantize_everything",
    "fc2_input_symmetric": "test_gpu_block_step.py::test_call_trace - fc2's input quantizer is the dual one by name, on both paths",
}


def _batch(config, l2, **options):
    from fpqvar_amd import var_block
    return var_block.GenerationBatch(MODEL, config, depth=DEPTH, batch_rows=ROWS, device="cuda:0", seed=SEED, attn_l2_norm=l2, **options)


def _inputs(gb):
    gb.gen.manual_seed(INPUT_SEED)
    return [gb.new_input(pn) for pn in gb.patch_nums[:N_STEPS]]


@functools.lru_cache(maxsize=None)
def _anchor(config, l2):
    """the model's parameters, inputs, step outputs and mutant deviations of one regime (CPU tensors, read-only)"""
    gb = _batch(config, l2)
    params = bm.params_of(gb)
    xs = [x.cpu() for x in _inputs(gb)]
    ys = bm.run(params, xs)
    mutants = {m: bm.deviation(bm.run(params, xs[:2], m)[1], ys[1], xs[1]) for m in bm.MUTANTS}
    return SimpleNamespace(params=params, xs=xs, ys=ys, mutants=mutants)


@functools.lru_cache(maxsize=None)
def _path(path, config, l2, **options):
    """(aggregate deviation from the model, per-step deviations, all finite) of one path, run once"""
    anchor = _anchor(config, l2)
    gb = _batch(config, l2, **options)
    mine = bm.params_of(gb)
    assert all(torch.equal(mine.w[n], anchor.params.w[n]) for n in mine.w), "the batches of one seed differ in their weights"
    assert all(torch.equal(a, b) for ma, mb in zip(mine.mods, anchor.params.mods) for a, b in zip(ma, mb))
    xs = _inputs(gb)
    assert all(torch.equal(x.cpu(), xa) for x, xa in zip(xs, anchor.xs)), "the paths do not see the same inputs"
    caches = gb.new_caches(path)
    ys = [gb.step(path, caches, x) for x in xs]
    torch.cuda.synchronize()
    ys = [y.cpu() for y in ys]
    assert all(y.dtype == torch.float16 and y.shape == x.shape for y, x in zip(ys, anchor.xs))
    steps = [bm.deviation(y, ym, x) for y, ym, x in zip(ys, anchor.ys, anchor.xs)]
    return bm.deviation(ys, anchor.ys, anchor.xs), steps, all(bool(torch.isfinite(y).all()) for y in ys)


def _name(config, l2, path, options=()):
    return f"{config}{'+l2' if l2 else ''} {path}" + "".join(f" {k}={v}" for k, v in options)


def _report(config, l2, path, options=()):
    d, steps, finite = _path(path, config, l2, **dict(options))
    print(f"\n{_name(config, l2, path, options):<34} d_{path} = {d:.4f}   per step " + " ".join(f"{s:.4f}" for s in steps)
          + ("" if finite else "   NOT FINITE"))
    return d, finite


@pytest.mark.parametrize("config,l2", REGIMES)
def test_reference_sequence_is_the_yardstick(config, l2):
    d_r, finite = _report(config, l2, "R")
    assert finite
    assert d_r < 1.0          # not a limit on R: a d_R of the size of the update itself would make every ratio below meaningless


CASES = ([(path, config, l2, ()) for path in ("F", "Q") for config, l2 in REGIMES]
         + [("Q", "w4a4", False, (("fused_fc1", False),)), ("F", "w4a4", False, (("sdpa_in_f", True),))])


@pytest.mark.parametrize("path,config,l2,options", CASES, ids=[_name(c, l, p, o).replace(" ", "-") for p, c, l, o in CASES])
def test_path_against_the_model(path, config, l2, options):
    d_r, _ = _report(config, l2, "R")
    d, finite = _report(config, l2, path, options)
    assert finite
    assert d <= FACTOR * d_r, f"d_{path} = {d:.4f} > {FACTOR} d_R = {FACTOR * d_r:.4f}"


def test_mutants_stand_out_of_the_noise():
    """Every wiring mutant is resolved (>= 4 d_R) in at least one regime, or is one of COVERED_ELSEWHERE; the table is printed with
    4 d_R per regime and says UNRESOLVED where it applies."""
    d_r = {r: _path("R", *r)[0] for r in REGIMES}
    table = {r: _anchor(*r).mutants for r in REGIMES}
    head = f"{'':>3} {'mutant (second step)':<30}" + "".join(f"{c + ('+l2' if l2 else ''):>12}" for c, l2 in REGIMES) + "   resolved in"
    lines = [head, f"{'':>3} {'4 d_R':<30}" + "".join(f"{RESOLVED * d_r[r]:>12.4f}" for r in REGIMES)]
    unresolved = []
    for i, m in enumerate(bm.MUTANTS):
        where = [r for r in REGIMES if table[r][m] >= RESOLVED * d_r[r]]
        lines.append(f"{i + 1:>3} {m:<30}" + "".join(f"{table[r][m]:>12.4f}" for r in REGIMES)
                     + "   " + (", ".join(c + ("+l2" if l2 else "") for c, l2 in where) or "UNRESOLVED"))
        if not where:
            unresolved.append(m)
    print("\n" + "\n".join(lines))
    for m in unresolved:
        print(f"unresolved: {m} - covered by {COVERED_ELSEWHERE.get(m, 'NOTHING')}")
    assert set(unresolved) <= set(COVERED_ELSEWHERE), f"not resolved in any regime: {sorted(set(unresolved) - set(COVERED_ELSEWHERE))}"
