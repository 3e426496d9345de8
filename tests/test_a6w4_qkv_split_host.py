"""mat_qkv on the A6W4 GEMM (fpq_gemm_a6w4_mx_split, fpq_gemm_a6w4_mx_split_qknorm; gemm.linear_a6w4_qkv_to_cache,
FP4Linear.qkv_to_cache) without a GPU: the two entry points' export, declaration and argument checks in their documented order
(null or fake pointers - nothing is launched), the Python wrappers' refusals, and the 16 new kernels' register / scratch figures
read from the built library."""
import ctypes
import os
import re

import pytest
import torch

from tests.test_no_spill import LIB, kernel_metadata

OK, ERR_ARG, ERR_DTYPE, ERR_SHAPE, ERR_TABLE = 0, -1, -2, -3, -4
F16, F32 = 0, 1
E2M1, E1M2, E3M0, E2M3, E3M2 = 0, 1, 2, 3, 4   # enum fpq_table
PTR = 0x7000_0000_1000   # an address with every alignment the checks ask for; nothing reads it
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("fpq_gemm_a6w4_mx_split", "fpq_gemm_a6w4_mx_split_qknorm")


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as g
    g.build_hip()
    from fpqvar_amd import _lib
    return _lib.lib()


def _split(n_parts=3, part_cols=128, rpb=4, out=(PTR, PTR, PTR), stride=None):
    from fpqvar_amd._lib import GemmSplit
    sp = GemmSplit()
    sp.part_cols, sp.n_parts, sp.rows_per_batch = part_cols, n_parts, rpb
    for p in range(3):
        sp.out[p], sp.row_stride[p], sp.batch_stride[p], sp.row0[p] = out[p], part_cols if stride is None else stride, rpb, 0
    return sp


_DEFAULT = object()


def _call(lib, norm):
    """the entry point with harmless defaults: 8 tokens (two batch entries of 4), three parts of 128 columns, k = 128"""
    def call(a=None, sa=None, w=None, sw=None, table=E3M0, w_dtype=F32, bias=None, tokens=8, outs=384, k=128, split=_DEFAULT, hs=PTR,
             km=0):
        sp = _split() if split is _DEFAULT else split
        ref = None if sp is None else ctypes.byref(sp)
        if norm:
            return lib.fpq_gemm_a6w4_mx_split_qknorm(a, sa, table, w, sw, w_dtype, bias, tokens, outs, k, ref, hs, km, None)
        return lib.fpq_gemm_a6w4_mx_split(a, sa, table, w, sw, w_dtype, bias, tokens, outs, k, ref, km, None)
    return call


# ------------------------------------------------------------------------------------------------------------ the C ABI
def test_version_exports_and_declarations(lib):
    from fpqvar_amd import _lib
    assert lib.fpq_version() >= 134
    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "fpq.h")).read(), flags=re.S)
    for name in NEW:
        assert hasattr(lib, name), name
        assert name in _lib._SIGS, name
        assert re.search(r"\bint\s+" + name + r"\s*\(", hdr), f"{name} is not declared in include/fpq.h"


@pytest.mark.parametrize("km", (0, 1))
@pytest.mark.parametrize("norm", (False, True))
def test_checks_in_the_documented_order(lib, norm, km):
    """table; NULL split (and the norm form's own arguments); negative sizes; the split descriptor; the scale dtype; shape; the empty
    problem; then pointers / alignment - every call here has NULL operands, so reaching the pointers is FPQ_ERR_ARG"""
    base = _call(lib, norm)
    call = lambda **kw: base(km=km, **kw)
    assert call() == ERR_ARG and call(tokens=0) == OK
    # the table before anything the header puts behind it
    for t in (E2M1, E2M3, E3M2, 5, 99, -1):
        assert call(table=t) == ERR_TABLE and call(table=t, split=None) == ERR_TABLE and call(table=t, tokens=-1) == ERR_TABLE, t
        assert call(table=t, split=_split(n_parts=0)) == ERR_TABLE and call(table=t, w_dtype=F16) == ERR_TABLE, t
        assert call(table=t, k=96) == ERR_TABLE and call(table=t, tokens=0) == ERR_TABLE, t
        if norm:
            assert call(table=t, hs=None) == ERR_TABLE, t
    # NULL split, before the sizes, the dtype and the shape
    assert call(split=None) == ERR_ARG and call(split=None, tokens=0) == ERR_ARG and call(split=None, w_dtype=F16) == ERR_ARG
    assert call(split=None, k=96) == ERR_ARG
    # negative sizes
    assert call(tokens=-1, w_dtype=F16) == ERR_ARG and call(outs=-384, k=96) == ERR_ARG and call(k=-128, w_dtype=F16) == ERR_ARG
    # the split descriptor, before the dtype and the shape (the dtype / shape argument alone would give another code)
    for bad in (dict(split=_split(n_parts=0), outs=0), dict(split=_split(n_parts=4), outs=512),
                dict(split=_split(part_cols=100), outs=300),                       # part_cols % 128
                dict(outs=256), dict(outs=512),                                    # outs != n_parts * part_cols
                dict(tokens=6), dict(split=_split(rpb=3)), dict(split=_split(rpb=0)),   # tokens % rows_per_batch
                dict(split=_split(out=(None, PTR, PTR))), dict(split=_split(out=(PTR, None, PTR))), dict(split=_split(out=(PTR, PTR, None))),
                dict(split=_split(out=(PTR + 4, PTR, PTR))), dict(split=_split(out=(PTR, PTR + 4, PTR))),
                dict(split=_split(out=(PTR, PTR, PTR + 4))),
                dict(split=_split(stride=64)), dict(split=_split(stride=130))):
        assert call(**bad) == ERR_ARG, bad
        assert call(**bad, w_dtype=F16) == ERR_ARG and call(**bad, k=96) == ERR_ARG, bad
    if norm:
        assert call(split=_split(n_parts=2), outs=256) == ERR_ARG and call(split=_split(n_parts=1), outs=128) == ERR_ARG
        assert call(split=_split(n_parts=2), outs=256, w_dtype=F16) == ERR_ARG
    else:   # one or two parts are fine here: on to the pointers; every part 8-byte aligned is enough (not the FP4 family's 16)
        assert call(split=_split(n_parts=2), outs=256) == ERR_ARG and call(split=_split(n_parts=2), outs=256, tokens=0) == OK
        assert call(split=_split(n_parts=1), outs=128, tokens=0) == OK
    assert call(split=_split(out=(PTR + 8, PTR + 8, PTR + 8)), tokens=0) == OK
    # fp16 weight scales: these forms are compiled for fp32 ones only - before the shape and the empty problem
    assert call(w_dtype=F16) == ERR_DTYPE and call(w_dtype=F16, k=96) == ERR_DTYPE and call(w_dtype=F16, tokens=0) == ERR_DTYPE
    assert call(w_dtype=7) == ERR_DTYPE
    # shape
    assert call(k=96) == ERR_SHAPE and call(k=128 * 65) == ERR_SHAPE and call(k=96, tokens=0) == ERR_SHAPE
    assert call(tokens=1 << 31, split=_split(rpb=1 << 20)) == ERR_SHAPE
    big = _split(rpb=1 << 20)
    if km:
        assert call(tokens=1 << 28, split=big) == ERR_SHAPE and call(tokens=1 << 30, split=big) == ERR_SHAPE
    else:
        assert call(tokens=1 << 28, split=big) == ERR_ARG                          # row-major: on to the pointers
    assert call(tokens=(1 << 28) - (1 << 20), split=big) == ERR_ARG
    assert call(k=0) == ERR_ARG
    # the empty problem
    assert call(tokens=0, table=E1M2) == OK and call(tokens=0, split=_split(rpb=7)) == OK


@pytest.mark.parametrize("km", (0, 1))
@pytest.mark.parametrize("norm", (False, True))
def test_pointer_and_alignment_checks(lib, norm, km):
    base = _call(lib, norm)
    def call(**kw):
        return base(**{**dict(a=PTR, sa=PTR, w=PTR, sw=PTR, km=km), **kw})
    for name in ("a", "sa", "w", "sw"):
        assert call(**{name: None}) == ERR_ARG, name
    assert call(a=PTR + 8) == ERR_ARG and call(w=PTR + 8) == ERR_ARG
    if km:   # both scale images: 16 bytes
        for off in (4, 8):
            assert call(sa=PTR + off) == ERR_ARG and call(sw=PTR + off) == ERR_ARG, off
    else:    # the elements' alignment
        assert call(sa=PTR + 1) == ERR_ARG and call(sw=PTR + 2) == ERR_ARG
    if norm:
        # the norm form's own arguments are refused whatever else is passed - the empty problem included
        assert call(hs=None) == ERR_ARG and call(hs=PTR + 2) == ERR_ARG and call(hs=None, tokens=0) == ERR_ARG
        assert call(bias=PTR + 8) == ERR_ARG and call(bias=PTR + 4) == ERR_ARG and call(bias=PTR + 8, tokens=0) == ERR_ARG
        assert call(a=PTR + 8, w=PTR + 8, sa=PTR + 4, sw=PTR + 4, bias=PTR + 16, tokens=0) == OK
    else:
        assert call(bias=PTR + 4) == ERR_ARG
        assert call(a=PTR + 8, w=PTR + 8, sa=PTR + 4, sw=PTR + 4, bias=PTR + 4, tokens=0) == OK


# ------------------------------------------------------------------------------------------------------------ the wrappers
def _rm_operands(tokens=8, outs=384, k=128):
    return (torch.zeros(tokens, k * 3 // 4, dtype=torch.uint8), torch.zeros(tokens, k // 128, dtype=torch.float16),
            torch.zeros(outs, k // 2, dtype=torch.uint8), torch.zeros(outs, k // 128))


def _km_operands(tokens=8, outs=384, groups=1):
    rows64 = (outs + 63) // 64 * 64
    return (torch.zeros(groups, tokens, 96, dtype=torch.uint8), torch.zeros(groups, (tokens + 3) // 4 * 4),
            torch.zeros(groups, rows64, 64, dtype=torch.uint8), torch.zeros(groups, rows64))


def _cache(bsz=2, max_len=10, heads=2, hd=64, dtype=torch.float16):
    return torch.zeros(2, bsz, max_len, heads, hd, dtype=dtype)


def test_linear_a6w4_qkv_to_cache_refuses_before_the_library(lib, monkeypatch):
    from fpqvar_amd import gemm
    fn = gemm.linear_a6w4_qkv_to_cache
    a, sa, w, sw = _rm_operands()
    ka, ksa, kw, ksw = _km_operands()
    with pytest.raises(RuntimeError, match="GPU"):
        fn(a, sa, "e3m0", w, sw, None, _cache(), 0, 4)
    with pytest.raises(RuntimeError, match="GPU"):
        fn(ka, ksa, "e3m0", kw, ksw, None, _cache(), 0, 4)
    monkeypatch.setattr(gemm, "require_gpu", lambda *a, **k: None)
    for bad in ((ka, ksa, w, sw), (a, sa, kw, ksw)):                        # mixed 2-D / 3-D operands
        with pytest.raises(RuntimeError, match="both operands must be"):
            fn(bad[0], bad[1], "e3m0", bad[2], bad[3], None, _cache(), 0, 4)
    for ops in ((a, sa, w, sw), (ka, ksa, kw, ksw)):
        go = lambda cache, pos=0, seq=4, table="e3m0", bias=None, hs=None: fn(ops[0], ops[1], table, ops[2], ops[3], bias, cache, pos, seq, hs)
        for cache in (_cache(dtype=torch.float32), _cache()[0], _cache()[:, :, :, :, :32], _cache().transpose(1, 2),
                      torch.zeros(3, 2, 10, 2, 64, dtype=torch.float16)):  # dtype, rank, a view that is not contiguous, leading 2
            with pytest.raises(RuntimeError, match=r"contiguous float16 \[2, B, max_len, H, c\]"):
                go(cache)
        with pytest.raises(RuntimeError, match="do not fit"):               # pos + seq > max_len
            go(_cache(), pos=7)
        with pytest.raises(RuntimeError, match="do not fit"):
            go(_cache(max_len=3))
        with pytest.raises(RuntimeError, match="do not fit"):               # tokens != B * seq
            go(_cache(bsz=3))
        with pytest.raises(RuntimeError, match="do not fit|does not belong"):   # outs != 3 * H * c
            go(_cache(heads=4))
        for table in ("e2m1", "fp_e2", "e2m3", None):
            with pytest.raises(RuntimeError, match="'e1m2' and 'e3m0'"):
                go(_cache(), table=table)
        with pytest.raises(RuntimeError, match="qk_norm_scale must be"):    # a head scale of the wrong length / dtype
            go(_cache(), hs=torch.ones(3))
        with pytest.raises(RuntimeError, match="qk_norm_scale must be"):
            go(_cache(), hs=torch.ones(2, dtype=torch.float16))
        with pytest.raises(RuntimeError, match="the bias must be a float32"):
            go(_cache(), hs=torch.ones(2), bias=torch.zeros(384, dtype=torch.float16))
    with pytest.raises(RuntimeError, match="weight scales must be float32"):    # fp16 weight scales: not compiled for these forms
        fn(a, sa, "e3m0", w, sw.half(), None, _cache(), 0, 4)


def test_fp4linear_qkv_to_cache_refusals(lib):
    from fpqvar_amd import gemm
    x, cache, hs = torch.zeros(2, 4, 128), _cache(), torch.ones(2)
    for act in ("e2m1", "e3m0", "e1m2"):
        a, sa, w, sw = _rm_operands()
        plain = gemm.FP4Linear(w[:, :64].contiguous(), sw, None, 128, 384, act)
        biased = gemm.FP4Linear(w[:, :64].contiguous(), sw, torch.zeros(384, dtype=torch.float16), 128, 384, act)
        for m in (plain, biased):
            with pytest.raises(RuntimeError, match="without qk_norm_scale"):    # bias= is the norm form's fp32 bias
                m.qkv_to_cache(x, cache, 0, 4, bias=torch.zeros(384))
        with pytest.raises(RuntimeError, match="must have no bias"):            # a module bias together with the norm
            biased.qkv_to_cache(x, cache, 0, 4, qk_norm_scale=hs)
        with pytest.raises(RuntimeError, match="must have no bias"):
            biased.qkv_to_cache(x, cache, 0, 4, qk_norm_scale=hs, bias=torch.zeros(384))
        with pytest.raises(RuntimeError, match="GPU"):                          # past the refusals: on to the quantizer
            plain.qkv_to_cache(x, cache, 0, 4, qk_norm_scale=hs)
        with pytest.raises(RuntimeError, match="GPU"):
            biased.qkv_to_cache(x, cache, 0, 4)


# ------------------------------------------------------------------------------------------------------------ the kernels
def test_the_new_kernels_do_not_spill(lib, tmp_path):
    """{split, qkn} x {row-major, km} x {64, 128 rows} x {E1M2, E3M0 activation}, fp32 weight scales only: exactly 16 instantiations,
    no scratch, no spill, no static LDS, at most 256 registers per lane.  The library is the one the `lib` fixture built."""
    assert os.path.exists(LIB), "libfpq_hip.so is missing after the build"
    names = ("gemm_a6w4_split_kernel", "gemm_a6w4_qkn_kernel", "gemm_a6w4_split_km_kernel", "gemm_a6w4_qkn_km_kernel")
    ks = [(n, r) for n, r in kernel_metadata(tmp_path) if any(s in n for s in names)]
    assert len(ks) == 16, [n for n, _ in ks]
    got = set()
    for n, r in ks:
        m = re.search(r"gemm_a6w4_(split|qkn)_(km_)?kernelI(DF16_|f)Li(\d)ELi4ELi(\d)E", n)
        assert m, n
        got.add((m.group(1), m.group(2) or "", m.group(3), int(m.group(4)), int(m.group(5))))
        assert int(r.get("vgpr_spill_count", 0)) == 0 and int(r.get("sgpr_spill_count", 0)) == 0, (n, r)
        assert int(r.get("private_segment_fixed_size", 0)) == 0, (n, r.get("private_segment_fixed_size"))
        assert int(r.get("group_segment_fixed_size", 0)) == 0, n
        assert int(r["vgpr_count"]) + int(r.get("agpr_count", 0)) <= 256, (n, r["vgpr_count"])
    assert got == {(form, km, "f", mt, fa) for form in ("split", "qkn") for km in ("", "km_") for mt in (2, 4) for fa in (2, 3)}
