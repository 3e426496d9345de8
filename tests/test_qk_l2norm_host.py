"""CPU-only: the two entry points of the attn_l2_norm q / k norm (include/fpq.h, fpq_gemm_fp4_mx_split_qknorm and
fpq_kv_cache_step_qknorm) are declared, exported and registered with ctypes, and refuse bad arguments with FPQ_ERR_ARG
before anything is launched (no GPU is touched: every call below fails its checks first)."""
import ctypes
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("fpq_gemm_fp4_mx_split_qknorm", "fpq_kv_cache_step_qknorm")
FPQ_ERR_ARG = -1


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as g
    g.build_hip()
    from fpqvar_amd import _lib
    return _lib.lib()


def test_declared_exported_and_registered(lib):
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "fpq.h")).read(), flags=re.S)
    from fpqvar_amd import _lib
    for n in NAMES:
        assert re.search(r"\b" + n + r"\s*\(", src), f"{n} not declared in include/fpq.h"
        assert hasattr(lib, n), f"{n} not exported by libfpq_hip.so"
        assert n in _lib._SIGS, f"{n} has no ctypes signature"
        assert getattr(lib, n).argtypes == _lib._SIGS[n][1]
    assert len(_lib._SIGS["fpq_gemm_fp4_mx_split_qknorm"][1]) == 13
    assert len(_lib._SIGS["fpq_kv_cache_step_qknorm"][1]) == 20


def _split(n_parts=3, part_cols=128):
    from fpqvar_amd._lib import GemmSplit
    sp = GemmSplit()
    sp.part_cols, sp.n_parts, sp.rows_per_batch = part_cols, n_parts, 1
    for p in range(3):
        sp.out[p], sp.row_stride[p], sp.batch_stride[p], sp.row0[p] = 256, part_cols, 1, 0
    return sp


def test_split_qknorm_rejects_bad_arguments(lib):
    scale = (ctypes.c_float * 64)()
    p = ctypes.addressof(scale)
    fake = 4096   # never dereferenced: every call fails its argument checks first

    def call(sp, hs=p, bias=None, outs=384):
        return lib.fpq_gemm_fp4_mx_split_qknorm(fake, fake, fake, fake, 1, bias, 16, outs, 128,
                                                None if sp is None else ctypes.byref(sp), hs, 0, None)
    assert call(None) == FPQ_ERR_ARG                                   # no split
    assert call(_split(n_parts=2), outs=256) == FPQ_ERR_ARG            # q, k, v: three parts
    assert call(_split(part_cols=192), outs=576) == FPQ_ERR_ARG        # part_cols % 128
    assert call(_split(), hs=None) == FPQ_ERR_ARG                      # NULL q_head_scale
    assert call(_split(), hs=p + 2) == FPQ_ERR_ARG                     # misaligned q_head_scale
    assert call(_split(), bias=fake + 4) == FPQ_ERR_ARG                # fp32 bias not 16-byte aligned
    assert call(_split(), outs=512) == FPQ_ERR_ARG                     # outs != 3 * part_cols


def test_kv_step_qknorm_rejects_bad_arguments(lib):
    scale = (ctypes.c_float * 64)()
    p = ctypes.addressof(scale)
    fake = 4096
    table = 1   # any table id: the argument checks come first

    def call(row_elems=128, group=64, hs=p, bias=None, head_dim=64, q=fake, q_out=fake, n_new=3):
        return lib.fpq_kv_cache_step_qknorm(fake, 2, 16, row_elems, 0, 2, q, fake, fake, 3 * row_elems, 3 * row_elems, 2, n_new,
                                            group, table, q_out, hs, bias, head_dim, None)
    assert call(head_dim=128, row_elems=256) == FPQ_ERR_ARG            # head_dim 64 only
    assert call(head_dim=32) == FPQ_ERR_ARG
    assert call(row_elems=96) == FPQ_ERR_ARG                           # whole heads
    assert call(group=32) == FPQ_ERR_ARG                               # kv_bit 6 (64) or 4 (128)
    assert call(hs=None) == FPQ_ERR_ARG                                # NULL q_head_scale
    assert call(hs=None, n_new=0) == FPQ_ERR_ARG                       # ... even with nothing to copy
    assert call(bias=fake + 8) == FPQ_ERR_ARG                          # fp32 bias not 16-byte aligned
    assert call(q=None) == FPQ_ERR_ARG                                 # new q missing
    assert call(q_out=None) == FPQ_ERR_ARG
    assert call(q_out=fake + 8) == FPQ_ERR_ARG                         # q_out not 16-byte aligned
