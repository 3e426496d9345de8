"""Paths R, F and Q of GenerationBatch.step at the parameters of the reference's own recorded runs (tests/golden/reference_blocks*.npz,
made by executing the reference's AdaLNSelfAttn blocks: tests/golden/make_block_golden.py), at the fixture's size: the released widths
C = 1920 / 2304, two blocks, two rows, steps of 1 / 4 / 9 tokens.  The batch takes the fixture's unquantized weights, smoothing
vectors, modulation, scale_mul and biases through GenerationBatch(tensors=...).

Limit, for every regime and each of R, F, Q:  d_path = deviation(path, model) <= 2 d0,  d0 = deviation(reference run, model).
  The yardstick is the reference's own run against the float64 model of tests/block_model.py - neither is code under test - so path
  R, this project's re-typing of the reference's op sequence, is held to a limit too.  The factor is the one
  test_gpu_block_paths.py argues for: d0 is rounding noise pushed through the quantizers' level flips, a path draws the same noise
  again, two independent draws lie sqrt(2) apart, and the rest is headroom for small shapes.  test_block_reference_host.py shows
  that d0 resolves the model's wiring mutants (the fp32 recordings agree with the model to round-off).
Reported, not asserted: deviation(path, reference run) - two draws of the noise, neither of them the model.

The model runs on the batch's own quantized weights (block_model.params_of), as in test_gpu_block_paths.py; whether they are the
reference's bit for bit (the fixture's SHA-256) is printed.

Options: the learned-vector regimes B (VAR-d30: factors from 0.05 to 2.79) and C (VAR-d36: four negative factors, one of 0.012)
also with fuse_residual=True, the gated-residual producers; regime D is rotation="full"; A/w4a4 also with fused_fc1=False.
Measured on an MI355X: profiles/block_paths_vs_reference.txt.
"""
import functools
from types import SimpleNamespace

import pytest
import torch

from tests import block_fixture as bf
from tests import block_model as bm

pytestmark = pytest.mark.gpu

FACTOR = 2.0
MODEL_OF_WIDTH = {1920: "d30-256", 2304: "d36-512"}
REGIMES = [n for n in bf.regime_names() if not n.endswith("/fp32")]


def _batch(name, **options):
    from fpqvar_amd import var_block
    r = bf.regime(name)
    tensors = dict(w=bf.raw_weights(r.C), s_qkv=r.s_qkv, s_fc1=r.s_fc1, mods=r.mods, scale_mul=r.scale_mul, qkv_bias=r.qkv_bias)
    if not r.l2:
        del tensors["scale_mul"], tensors["qkv_bias"]
    if not r.block_rotate:
        options = dict(options, rotation="full")
    return var_block.GenerationBatch(MODEL_OF_WIDTH[r.C], r.config, depth=r.depth, batch_rows=r.rows, device="cuda:0", attn_l2_norm=r.l2,
                                     tensors=tensors, **options)


@functools.lru_cache(maxsize=None)
def _anchor(name):
    """the model's step outputs at the batch's parameters and d0, the reference run's distance from them (CPU, read-only)"""
    r = bf.regime(name)
    gb = _batch(name)
    params = bm.params_of(gb)
    assert gb.C == r.C and gb.H == r.H and all(torch.equal(a, b) for ma, mb in zip(params.mods, r.mods) for a, b in zip(ma, mb))
    assert torch.equal(params.s_qkv, r.s_qkv) and torch.equal(params.s_fc1, r.s_fc1)
    same = [n for n in bf.WEIGHT_NAMES if bf.sha256(params.w[n].half()) == bf.load()[f"regime/{name}/weight_sha256/{n}"].tobytes()]
    ys = bm.run(params, r.xs)
    d0 = bm.deviation(r.ys, ys, r.xs)
    print(f"\n{name:<34} d0 = {d0:.4f}   weights equal to the reference's, bit for bit: {', '.join(same) or 'none'}")
    return SimpleNamespace(params=params, ys=ys, d0=d0)


@functools.lru_cache(maxsize=None)
def _path(path, name, **options):
    """(deviation from the model, deviation from the reference run, per-step deviations from the model, all finite), run once"""
    r, anchor = bf.regime(name), _anchor(name)
    gb = _batch(name, **options)
    mine = bm.params_of(gb)
    assert all(torch.equal(mine.w[n], anchor.params.w[n]) for n in mine.w), "two batches of one regime differ in their weights"
    caches = gb.new_caches(path)
    ys = [gb.step(path, caches, x.to("cuda:0")) for x in r.xs]
    torch.cuda.synchronize()
    ys = [y.cpu() for y in ys]
    assert all(y.dtype == torch.float16 and y.shape == x.shape for y, x in zip(ys, r.xs))
    steps = [bm.deviation(y, ym, x) for y, ym, x in zip(ys, anchor.ys, r.xs)]
    return (bm.deviation(ys, anchor.ys, r.xs), bm.deviation(ys, [y.double() for y in r.ys], r.xs), steps,
            all(bool(torch.isfinite(y).all()) for y in ys))


def _id(path, name, options):
    return f"{name} {path}" + "".join(f" {k}={v}" for k, v in options)


CASES = [(path, name, ()) for name in REGIMES for path in ("R", "F", "Q")]
CASES += [(path, name, (("fuse_residual", True),)) for name in REGIMES if name[0] in "BC" for path in ("F", "Q")]
CASES += [("Q", "A/w4a4", (("fused_fc1", False),))]


@pytest.mark.parametrize("path,name,options", CASES, ids=[_id(*c).replace(" ", "-") for c in CASES])
def test_path_within_the_executed_references_noise(path, name, options):
    d0 = _anchor(name).d0
    d, d_ref, steps, finite = _path(path, name, **dict(options))
    print(f"\n{_id(path, name, options):<40} d_{path} = {d:.4f}   2 d0 = {FACTOR * d0:.4f}   per step " + " ".join(f"{s:.4f}" for s in steps)
          + f"   from the reference run {d_ref:.4f}" + ("" if finite else "   NOT FINITE"))
    assert finite
    assert d <= FACTOR * d0, f"d_{path} = {d:.4f} > {FACTOR} d0 = {FACTOR * d0:.4f}"
