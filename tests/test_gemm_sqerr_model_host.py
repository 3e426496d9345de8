"""CPU: the error model of the GEMMs' squared-error tail (tests/gemm_sqerr_model.py) on the shapes tests/test_gpu_gemm_sqerr.py
runs.  The emulation of the shipped order of operations is within the derived bound for every shape, tiling and reference dtype,
each deliberate mistake exceeds it where it is listed, a zero loss is met exactly, and the header states the same chain."""
import math
import os
import re

import pytest
import torch

from tests import gemm_sqerr_model as gm

F16, F32 = torch.float16, torch.float32
SHAPES = ((1, 8), (37, 200), (257, 136), (100, 1920))       # (tokens, outs) of the GPU tests
TILE_ROWS = (64, 128, 256)


def _ratio(tokens, outs, dtype, bm, family, mistake=None):
    ref, y, w = gm.make_case(tokens, outs, dtype, family)
    assert bool((w > 0).all()) and bool(torch.isfinite(w).all())
    want = gm.reference(ref, y.half(), w)
    got = gm.emulate(ref, y, w, bm, mistake)
    rel, floor = gm.bound(tokens, outs, bm, dtype, float(w.max()))
    return gm.ratio(got, want, rel, floor)


@pytest.mark.parametrize("dtype", (F16, F32), ids=("f16", "f32"))
@pytest.mark.parametrize("tokens,outs", SHAPES, ids=lambda v: str(v))
def test_emulation_of_the_shipped_order_is_within_the_bound(tokens, outs, dtype):
    for bm in TILE_ROWS:
        for family in ("gauss", "weights", "fp16_max"):
            r = _ratio(tokens, outs, dtype, bm, family)
            print(f"[{tokens} x {outs}] {dtype} {bm}-row tiles {family}: err / bound {r:.3g}")
            assert r <= 1.0, (bm, family, r)
        ref, y, w = gm.make_case(tokens, outs, dtype, "equal")
        assert gm.emulate(ref, y, w, bm) == 0.0, "ref == y16 must give exactly 0"
        assert gm.reference(ref, y.half(), w) == 0.0


# where each mistake must show: (family, tokens, outs, ref dtype, tile rows)
CAUGHT_ON = {
    "rows_past_T_counted": [("gauss", 1, 8, F16, 64), ("gauss", 37, 200, F16, 64), ("gauss", 257, 136, F32, 128), ("gauss", 100, 1920, F16, 64)],
    "cols_past_O_counted": [("gauss", 1, 8, F16, 64), ("gauss", 37, 200, F32, 128), ("gauss", 257, 136, F16, 256)],
    "clamped_row_weight": [("weights", 37, 200, F16, 64), ("weights", 257, 136, F16, 128)],
    "y_not_rounded_to_fp16": [("gauss", 37, 200, F16, 64), ("gauss", 100, 1920, F32, 128)],
    "neighbour_weight": [("weights", 37, 200, F16, 64), ("weights", 100, 1920, F16, 64)],
    # (gaussian differences mostly ARE fp16 numbers or round without a bias: the family whose differences overflow fp16 shows it)
    "diff_fp16": [("fp16_max", 37, 200, F16, 64), ("fp16_max", 257, 136, F32, 128), ("fp16_max", 100, 1920, F16, 64)],
    "partial_of_last_tile_dropped": [("gauss", 37, 200, F16, 64), ("gauss", 257, 136, F16, 128), ("gauss", 100, 1920, F32, 64)],
}


@pytest.mark.parametrize("mistake", gm.MISTAKES)
def test_each_mistake_exceeds_the_bound(mistake):
    assert set(CAUGHT_ON) == set(gm.MISTAKES)
    assert {(t, o) for cases in CAUGHT_ON.values() for _, t, o, _, _ in cases} == set(SHAPES), "every GPU shape catches something"
    for family, tokens, outs, dtype, bm in CAUGHT_ON[mistake]:
        r = _ratio(tokens, outs, dtype, bm, family, mistake)
        print(f"{mistake} on {family} [{tokens} x {outs}] {dtype} {bm}-row tiles: err / bound {r:.3g}")
        assert r > 1.0, (mistake, family, tokens, outs, r)


def test_non_finite_classes_and_the_edge_duplicates():
    """a NaN / inf in the LAST valid row of a partly filled tile: the class of the fp32 expression; the same value is what the rows
    past T duplicate - counted once, by the row itself, never through a duplicate"""
    for dtype in (F16, F32):
        ref, y, w = gm.make_case(37, 200, dtype, "gauss")
        for bad, want in ((math.nan, "nan"), (math.inf, "inf")):
            r = ref.clone()
            r[36, 199] = bad
            assert gm.expected_class(r, y.half()) == want
            assert gm.class_of(gm.emulate(r, y, w, 64)) == want == gm.class_of(gm.reference(r, y.half(), w))
        r, yy = ref.clone(), y.clone()
        r[36, 5], yy[36, 5] = math.inf, math.inf                      # inf - inf
        assert gm.class_of(gm.emulate(r, yy, w, 64)) == "nan"


def test_chain_tilings_and_workspace():
    assert gm.chain(64, 1) == (8 + 1 + 22, 3) and gm.chain(128, 4815) == (16 + 19 + 22, 3) and gm.chain(256, 257) == (32 + 2 + 22, 3)
    assert gm.tiles(13600, 5760, 128) == 107 * 45
    rel, floor = gm.bound(13600, 5760, 128, F16)
    assert math.isclose(rel, 60 * gm.U, rel_tol=1e-5) and floor == 0.0 and rel < 1e-4
    assert gm.bound(37, 200, 64, F32)[1] > 0.0
    # the launch rules (gemm_glds_tiling, gemm_fp6_rows_impl)
    assert gm.tile_rows("fp4", 100, 1920) == 64 and gm.tile_rows("fp4", 13600, 5760) == 128 and gm.tile_rows("fp4", 65536, 5760) == 256
    assert gm.tile_rows("a6w4", 65536, 5760) == 128 and gm.tile_rows("w6", 100, 1920, 20) == 128 and gm.tile_rows("a6w4", 100, 1920, 10) == 64
    assert gm.tile_rows("fp4", 100, 1920, 40) == 64 and gm.tile_rows("fp4", 100, 1920, 10) == 256
    assert gm.tile_rows("f6_rows", 100, 1920) == 128 and gm.tile_rows("f6_rows", 13600, 5760) == 256 and gm.tile_rows("f6_rows", 100, 1920, 1) == 256
    assert gm.workspace_bytes(0, 0) == 4 and gm.workspace_bytes(1, 8) == 4 and gm.workspace_bytes(257, 136) == 4 * 5 * 2


def test_search_layer_has_a_winner_margin_above_twice_the_cross_path_tolerance():
    """tests/test_gpu_format_search_mc.py asserts the same winner as fused=True, whose losses it matches to REL = 2e-3 only: the
    seeded layer's best pair must lead the runner-up by at least 2 REL - with the oracle's quantizers and float32 CPU products"""
    rel = 2e-3
    for w_dtype in (F16, F32):
        xs, w = gm.search_layer_case(gm.SEARCH_SEED, w_dtype)
        assert [x.shape[0] for x in xs] == list(gm.SEARCH_ROWS) and w.shape == (256, 384) and all(x.dtype == F16 for x in xs)
        for formats, best in ((("fp_e1", "fp_e2", "fp_e3"), (1, 1)), (("fp6_e2m3", "fp6_e3m2"), (0, 0))):
            table = gm.cpu_loss_table(xs, w, formats)
            margin = gm.winner_margin(table)
            print(f"{formats} w {w_dtype}: margin {margin:.3g}")
            assert margin >= 2 * rel, (formats, margin)
            assert divmod(int(table.reshape(-1).argmin()), len(formats)) == best


def test_header_and_source_state_the_same_chain():
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    hdr = open(os.path.join(root, "include", "fpq.h")).read()
    assert "D = 4 MT + ceil(tiles / 256) + 22,  c = 3" in hdr
    assert re.search(r"#define\s+FPQ_VERSION\s+136\b", hdr)
    src = open(os.path.join(root, "fpqvar_amd", "csrc", "fpq_gemm_fp4.h")).read()
    assert "D = 4 MT + ceil(tiles / 256) + 22" in src and "c = 3 roundings" in src
