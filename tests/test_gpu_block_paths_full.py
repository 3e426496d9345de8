"""tests/test_gpu_block_paths.py's protocol with GenerationBatch(rotation="full"): Q is the dense randomized Hadamard matrix of
size C (the reference's `--rotate` without `--block_rotate`), the weights are rotated by it, path R multiplies by it, and paths F
and Q run the full-width producers - W4A4: rotation.adaln_rotate_quant_full / _full_mx, W6A6: adaln_rotate_quant_full_token with
emit="values" / "fp6".  All three are held to the float64 block of tests/block_model.py, whose parameters (params_of) take Q from
the batch.

Shape, seeds, measure and factors are the block form's file's: "d30-256", depth 2, four rows, the first four scale steps, W4A4 and
W6A6 with and without attn_l2_norm; d = ||y - y_model|| / ||y_model - x|| over the four step outputs.

Limits, none fixed in advance:
  d_F <= 2 d_R and d_Q <= 2 d_R, d_R from path R of the same regime under rotation="full" (the reasoning of test_gpu_block_paths.py:
    two draws of the same rounding noise sit sqrt(2) apart, the rest is headroom for these small shapes); d_R < 1.
  resolution: the mutants activation_not_rotated, swap_smooth_act and scale_without_one of block_model.MUTANTS and one mutant of
    this file's own - the model run with Q replaced by the 128-BLOCK matrix of the same seed, the mutant that tells the two
    rotation modes apart: a producer that ran the block form against full-width weights computes exactly it - must each reach
    >= 4 d_R (second step, as the block form's file) in at least one regime.
"""
import dataclasses
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
MODEL_MUTANTS = ("activation_not_rotated", "swap_smooth_act", "scale_without_one")
BLOCK_Q = "block_q_for_full_q"          # this file's mutant: the 128-block matrix where the full-width one belongs


def _batch(config, l2, **options):
    from fpqvar_amd import var_block
    return var_block.GenerationBatch(MODEL, config, depth=DEPTH, batch_rows=ROWS, device="cuda:0", seed=SEED, attn_l2_norm=l2,
                                     rotation="full", **options)


def _inputs(gb):
    gb.gen.manual_seed(INPUT_SEED)
    return [gb.new_input(pn) for pn in gb.patch_nums[:N_STEPS]]


@functools.lru_cache(maxsize=None)
def _anchor(config, l2):
    """the model's parameters, inputs, step outputs and mutant deviations of one regime (CPU tensors, read-only)"""
    from fpqvar_amd import rotation
    gb = _batch(config, l2)
    params = bm.params_of(gb)
    full = rotation.get_orthogonal_matrix(gb.C, device="cpu").float()
    assert torch.equal(params.Q, full), "rotation='full': the batch's Q is not the full-width matrix"
    block = rotation.block_random_hadamard_matrix(gb.C, 128, "cpu", 42).float()
    assert not torch.equal(full, block)
    xs = [x.cpu() for x in _inputs(gb)]
    ys = bm.run(params, xs)
    mutants = {m: bm.deviation(bm.run(params, xs[:2], m)[1], ys[1], xs[1]) for m in MODEL_MUTANTS}
    mutants[BLOCK_Q] = bm.deviation(bm.run(dataclasses.replace(params, Q=block), xs[:2])[1], ys[1], xs[1])
    return SimpleNamespace(params=params, xs=xs, ys=ys, mutants=mutants)


@functools.lru_cache(maxsize=None)
def _path(path, config, l2):
    """(aggregate deviation from the model, per-step deviations, all finite) of one path, run once"""
    anchor = _anchor(config, l2)
    gb = _batch(config, l2)
    mine = bm.params_of(gb)
    assert all(torch.equal(mine.w[n], anchor.params.w[n]) for n in mine.w), "the batches of one seed differ in their weights"
    assert all(torch.equal(a, b) for ma, mb in zip(mine.mods, anchor.params.mods) for a, b in zip(ma, mb))
    assert torch.equal(mine.Q, anchor.params.Q)
    xs = _inputs(gb)
    assert all(torch.equal(x.cpu(), xa) for x, xa in zip(xs, anchor.xs)), "the paths do not see the same inputs"
    caches = gb.new_caches(path)
    ys = [gb.step(path, caches, x) for x in xs]
    torch.cuda.synchronize()
    ys = [y.cpu() for y in ys]
    assert all(y.dtype == torch.float16 and y.shape == x.shape for y, x in zip(ys, anchor.xs))
    steps = [bm.deviation(y, ym, x) for y, ym, x in zip(ys, anchor.ys, anchor.xs)]
    return bm.deviation(ys, anchor.ys, anchor.xs), steps, all(bool(torch.isfinite(y).all()) for y in ys)


def _name(config, l2, path):
    return f"{config}{'+l2' if l2 else ''} {path} full"


def _report(config, l2, path):
    d, steps, finite = _path(path, config, l2)
    print(f"\n{_name(config, l2, path):<34} d_{path} = {d:.4f}   per step " + " ".join(f"{s:.4f}" for s in steps)
          + ("" if finite else "   NOT FINITE"))
    return d, finite


def test_the_argument():
    from fpqvar_amd import var_block
    with pytest.raises(ValueError, match="fuse_residual"):
        var_block.GenerationBatch(MODEL, "w6a6", depth=1, batch_rows=2, device="cuda:0", rotation="full", fuse_residual=True)
    with pytest.raises(ValueError, match="rotation"):
        var_block.GenerationBatch(MODEL, "w6a6", depth=1, batch_rows=2, device="cuda:0", rotation="dense")
    assert "full-width rotation" in _batch("w6a6", False).describe()
    assert "full-width" not in var_block.GenerationBatch(MODEL, "w6a6", depth=1, batch_rows=2, device="cuda:0").describe()


@pytest.mark.parametrize("config,l2", REGIMES)
def test_reference_sequence_is_the_yardstick(config, l2):
    d_r, finite = _report(config, l2, "R")
    assert finite
    assert d_r < 1.0          # not a limit on R: a d_R of the size of the update itself would make every ratio below meaningless


CASES = [(path, config, l2) for path in ("F", "Q") for config, l2 in REGIMES]


@pytest.mark.parametrize("path,config,l2", CASES, ids=[_name(c, l, p).replace(" ", "-") for p, c, l in CASES])
def test_path_against_the_model(path, config, l2):
    d_r, _ = _report(config, l2, "R")
    d, finite = _report(config, l2, path)
    assert finite
    assert d <= FACTOR * d_r, f"d_{path} = {d:.4f} > {FACTOR} d_R = {FACTOR * d_r:.4f}"


def test_mutants_stand_out_of_the_noise():
    """Each of the four mutants is resolved (>= 4 d_R) in at least one regime; the table is printed as the block form's file prints it."""
    d_r = {r: _path("R", *r)[0] for r in REGIMES}
    table = {r: _anchor(*r).mutants for r in REGIMES}
    head = f"{'':>3} {'mutant (second step)':<30}" + "".join(f"{c + ('+l2' if l2 else ''):>12}" for c, l2 in REGIMES) + "   resolved in"
    lines = [head, f"{'':>3} {'4 d_R':<30}" + "".join(f"{RESOLVED * d_r[r]:>12.4f}" for r in REGIMES)]
    unresolved = []
    for i, m in enumerate(MODEL_MUTANTS + (BLOCK_Q,)):
        where = [r for r in REGIMES if table[r][m] >= RESOLVED * d_r[r]]
        lines.append(f"{i + 1:>3} {m:<30}" + "".join(f"{table[r][m]:>12.4f}" for r in REGIMES)
                     + "   " + (", ".join(c + ("+l2" if l2 else "") for c, l2 in where) or "UNRESOLVED"))
        if not where:
            unresolved.append(m)
    print("\n" + "\n".join(lines))
    assert not unresolved, f"not resolved in any regime: {unresolved}"
