"""CPU-only: fpq_gemm_fp4_tiling (include/fpq.h) - which LDS-DMA tiling an FP4 GEMM call runs.  The function is host arithmetic, so
everything here runs without a GPU: the export, FPQ_GEMM_CFG = 40 reaching the deep-ring kernel, its fall-through where the
ring's LDS image does not fit, the default choice at the small scale steps, and the entry points' own error codes."""
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CODES = (10, 20, 30, 40)
ERR_ARG, ERR_SHAPE = -1, -3
LDS_CAP = 160 * 1024
# the twenty (T, O) points of the small scale steps, where the FP4 GEMM's time is flat (profiles/r04_gemm_small_steps.txt): d30
# (100 pn^2 rows, C = 1920) at pn = 1 .. 4 against proj / qkv / fc1, d36-512 (20 pn^2 rows, C = 2304) at pn = 1, 2, 3, 4 against
# proj and fc1
SMALL_STEPS = [(100 * pn * pn, o, 1920) for pn in (1, 2, 3, 4) for o in (1920, 5760, 7680)] + \
              [(20 * pn * pn, o, 2304) for pn in (1, 2, 3, 4) for o in (2304, 9216)]
assert len(SMALL_STEPS) == 20


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as g
    g.build_hip()
    from fpqvar_amd import _lib
    return _lib.lib()


def _ring_stages():
    src = open(os.path.join(ROOT, "fpqvar_amd", "csrc", "fpq_gemm_fp4.h")).read()
    return int(re.search(r"#define FPQ_GEMM_RING_STAGES (\d+)", src).group(1))


def _ring_lds(k, form):
    """the deep-ring kernel's LDS image as fpq_gemm_fp4.h lays it out: S stages of a 64 x 128 tile's twelve 1 KiB blocks, the fp32
    scale tiles of K / 128 groups rounded up to four, and in the fc1 form the dual quantizer's bucket table (2^(16 - shift) fp16
    entries, shift = min(9 - mbits) over (e1m2_neg, e2m1_pos) = 7)"""
    groups = (k // 128 + 3) & ~3
    return _ring_stages() * 12 * 1024 + groups * (64 + 128) * 4 + (2 << (16 - 7) if form == 1 else 0)


def test_symbol_is_exported_and_declared(lib):
    assert hasattr(lib, "fpq_gemm_fp4_tiling")
    hdr = open(os.path.join(ROOT, "include", "fpq.h")).read()
    assert re.search(r"int fpq_gemm_fp4_tiling\(int64_t tokens, int64_t outs, int64_t k, int form\);", hdr)
    from fpqvar_amd import _lib
    assert "fpq_gemm_fp4_tiling" in _lib._SIGS


def test_switch_40_reaches_the_ring(lib, lib_options):
    from fpqvar_amd import gemm
    lib_options("FPQ_GEMM_CFG", 40)
    assert lib.fpq_gemm_fp4_tiling(100, 1920, 1920, 0) == 40
    assert lib.fpq_gemm_fp4_tiling(100, 7680, 1920, 1) == 40
    assert gemm.fp4_tiling(100, 1920, 1920) == 40 and gemm.fp4_tiling(100, 7680, 1920, form="fc1") == 40
    for cfg in (10, 20, 30):   # the tilings there were keep their codes
        lib_options("FPQ_GEMM_CFG", cfg)
        assert lib.fpq_gemm_fp4_tiling(100, 1920, 1920, 0) == cfg and lib.fpq_gemm_fp4_tiling(100, 7680, 1920, 1) == cfg


def test_ring_is_never_chosen_where_its_lds_image_does_not_fit(lib, lib_options):
    """K walked up to the limit in both forms, forced and by default: 40 only where the image computed here fits 160 KiB, and a
    forced 40 that does not fit falls through to a tiling of the existing chain."""
    for opt in (40, None):
        lib_options("FPQ_GEMM_CFG", opt)
        for form in (0, 1):
            for k in range(128, 8192 + 1, 128):
                for tokens, outs in ((100, 1920), (400, 7680), (2500, 5760)):
                    got = lib.fpq_gemm_fp4_tiling(tokens, outs, k, form)
                    assert got in CODES, (opt, form, k, tokens, outs, got)
                    fits = _ring_lds(k, form) <= LDS_CAP
                    if got == 40:
                        assert fits, (opt, form, k, _ring_lds(k, form))
                    if opt == 40:
                        assert (got == 40) == fits, (form, k, got, _ring_lds(k, form))


def test_default_choice_at_the_small_steps(lib, lib_options):
    lib_options("FPQ_GEMM_CFG", None)
    for tokens, outs, k in SMALL_STEPS:
        for form in (0, 1):
            assert lib.fpq_gemm_fp4_tiling(tokens, outs, k, form) in CODES, (tokens, outs, k, form)


def test_refused_shapes_return_the_entry_points_codes(lib, lib_options):
    from fpqvar_amd import gemm
    for opt in (None, 40):
        lib_options("FPQ_GEMM_CFG", opt)
        for form in (0, 1):
            assert lib.fpq_gemm_fp4_tiling(100, 1920, 1920 + 64, form) == ERR_SHAPE      # K % 128
            assert lib.fpq_gemm_fp4_tiling(100, 1920, 8192 + 128, form) == ERR_SHAPE     # K > 8192
            assert lib.fpq_gemm_fp4_tiling(100, 1924, 1920, form) == ERR_SHAPE           # outs % 8
            assert lib.fpq_gemm_fp4_tiling(-1, 1920, 1920, form) == ERR_ARG
            assert lib.fpq_gemm_fp4_tiling(100, 1920, 0, form) == ERR_ARG
            assert lib.fpq_gemm_fp4_tiling(0, 1920, 1920, form) == 0                     # nothing would be launched
        assert lib.fpq_gemm_fp4_tiling(100, 1928, 1920, 0) in CODES                      # outs % 8 == 0 is enough for a Linear ...
        assert lib.fpq_gemm_fp4_tiling(100, 1928, 1920, 1) == ERR_SHAPE                  # ... the fc1 form wants whole groups
        assert lib.fpq_gemm_fp4_tiling(100, 1920, 1920, 2) == ERR_ARG
    with pytest.raises(RuntimeError):
        gemm.fp4_tiling(100, 1924, 1920)
    with pytest.raises(ValueError):
        gemm.fp4_tiling(100, 1920, 1920, form="fc2")
