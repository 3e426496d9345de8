"""The squared-error forms of the four GEMM families (include/fpq.h, fpq_gemm_*_sqerr) without a GPU: declared, exported and
registered alike; which code a refused call returns and, where a call has several faults, which of them is reported - the
family's own checks first, in the family's order, then the form's pointers, then the reference's dtype; the workspace size.
Every call below is refused before anything is enqueued, so the pointers (a fake address with every alignment the checks ask
for) are never read - as in tests/test_gemm_abi_host.py."""
import ctypes
import os
import re

import pytest

from tests import gemm_sqerr_model as gm

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OK, ARG, DTYPE, SHAPE, TABLE = 0, -1, -2, -3, -4
F16, F32 = 0, 1
E2M1, E1M2, E3M0, E2M3, E3M2 = 0, 1, 2, 3, 4
PTR = 0x7000_0000_1000

_TAIL = " bias ref ref_dtype row_weight loss_out workspace tokens outs k"
ENTRY = {
    "fpq_gemm_fp4_sqerr": "a sa w sw w_dtype" + _TAIL,
    "fpq_gemm_a6w4_sqerr": "a sa a_table w sw w_dtype" + _TAIL,
    "fpq_gemm_w6_sqerr": "a sa a_table w sw w_dtype w_table" + _TAIL,
    "fpq_gemm_f6_rows_sqerr": "a sa a_dtype a_table w sw w_dtype w_table" + _TAIL,
}
PLAIN = {"fpq_gemm_fp4_sqerr": "fpq_gemm_fp4_mx", "fpq_gemm_a6w4_sqerr": "fpq_gemm_a6w4_mx", "fpq_gemm_w6_sqerr": "fpq_gemm_w6_mx",
         "fpq_gemm_f6_rows_sqerr": "fpq_gemm_f6_rows"}
ALL = list(ENTRY)
PER_GROUP = ALL[:3]
TABLES = {"fpq_gemm_fp4_sqerr": {}, "fpq_gemm_a6w4_sqerr": dict(a_table=E3M0), "fpq_gemm_w6_sqerr": dict(a_table=E2M1, w_table=E1M2),
          "fpq_gemm_f6_rows_sqerr": dict(a_table=E3M2, w_table=E2M3)}


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as g
    g.build_hip()
    from fpqvar_amd import _lib
    return _lib.lib()


def _call(lib, entry, **kw):
    """`entry` with valid arguments (8 tokens, 384 outputs, K = 128) but for the overrides - which must make it a refused call"""
    assert kw, "a call without a fault would be enqueued on a fake address"
    args = dict(a=PTR, sa=PTR, w=PTR, sw=PTR, bias=None, ref=PTR, ref_dtype=F16, row_weight=PTR, loss_out=PTR, workspace=PTR,
                a_dtype=F16, w_dtype=F32, tokens=8, outs=384, k=128, **TABLES[entry])
    assert not set(kw) - set(args), kw
    args.update(kw)
    return getattr(lib, entry)(*[args[n] for n in ENTRY[entry].split()], None)


def test_declared_exported_registered_and_the_version_stays(lib):
    from fpqvar_amd import _lib
    assert lib.fpq_version() == 136
    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "fpq.h")).read(), flags=re.S)
    assert re.search(r"#define\s+FPQ_VERSION\s+136\b", hdr)
    i, p, q = ctypes.c_int, ctypes.c_void_p, ctypes.c_int64
    tail = [p, p, i, p, p, p, q, q, q, p]                 # bias, ref, ref_dtype, row_weight, loss_out, workspace, tokens, outs, k, stream
    for name, plain in PLAIN.items():
        assert hasattr(lib, name) and name in _lib._SIGS, name
        decl = re.search(r"\bint\s+" + name + r"\s*\(([^)]*)\)", hdr)
        assert decl, f"{name} is not declared in include/fpq.h"
        params = [" ".join(s.split()) for s in decl.group(1).split(",")]
        pdecl = [" ".join(s.split()) for s in re.search(r"\bint\s+" + plain + r"\s*\(([^)]*)\)", hdr).group(1).split(",")]
        n_head = pdecl.index("const void* bias") + 1
        assert params[:n_head] == pdecl[:n_head], f"{name}: the argument list up to bias differs from {plain}'s"
        assert params[n_head:] == ["const void* ref", "int ref_dtype", "const float* row_weight", "float* loss_out", "void* workspace",
                                   "int64_t tokens", "int64_t outs", "int64_t k", "fpq_stream_t stream"], name
        ret, args = _lib._SIGS[name]
        assert ret is i and list(args) == list(_lib._SIGS[plain][1][:n_head - 1]) + tail, name
        assert getattr(lib, name).argtypes == args
    assert re.search(r"\bint64_t\s+fpq_gemm_sqerr_workspace_bytes\s*\(\s*int64_t tokens,\s*int64_t outs\s*\)", hdr)
    assert _lib._SIGS["fpq_gemm_sqerr_workspace_bytes"] == (q, [q, q])
    assert "fpq_set_option" in _lib._SIGS and len(_lib.option_names()) == 14, "no new switch"


def test_workspace_sizes(lib):
    for tokens, outs in ((0, 0), (0, 384), (1, 8), (37, 200), (64, 128), (65, 129), (257, 136), (100, 1920), (13600, 5760), (1 << 20, 8192)):
        got = lib.fpq_gemm_sqerr_workspace_bytes(tokens, outs)
        assert got == gm.workspace_bytes(tokens, outs) >= 4, (tokens, outs, got)
        for family in gm.FAMILIES:                        # every tiling a launch can pick fits
            for forced in (None, 10, 20, 30, 40, 0, 1):
                assert 4 * gm.tiles(tokens, outs, gm.tile_rows(family, tokens, outs, forced)) <= max(got, 4)
    assert lib.fpq_gemm_sqerr_workspace_bytes(13600, 5760) == 4 * 213 * 45
    assert lib.fpq_gemm_sqerr_workspace_bytes(-1, 8) == ARG and lib.fpq_gemm_sqerr_workspace_bytes(8, -8) == ARG
    assert lib.fpq_gemm_sqerr_workspace_bytes(1 << 31, 8) == ARG


# (what is wrong, the entry points it is tried on, the code, the overrides - several dicts: each is a call of its own)
ONE_FAULT = [
    ("negative sizes", ALL, ARG, [dict(tokens=-4), dict(outs=-8), dict(k=-128)]),
    ("k % 128", ALL, SHAPE, [dict(k=96), dict(k=192)]),
    ("k == 0", ALL, ARG, [dict(k=0)]),
    ("k above the per-group limit", PER_GROUP, SHAPE, [dict(k=128 * 65)]),
    ("outs % 8", ALL, SHAPE, [dict(outs=380)]),
    ("tokens above 2^31", ALL, SHAPE, [dict(tokens=1 << 31)]),
    ("weight scale dtype", ALL, DTYPE, [dict(w_dtype=7), dict(w_dtype=2)]),
    ("fp16 weight scales on a 6-bit weight", ["fpq_gemm_w6_sqerr"], DTYPE, [dict(w_dtype=F16)]),
    ("activation scale dtype", ["fpq_gemm_f6_rows_sqerr"], DTYPE, [dict(a_dtype=7), dict(a_dtype=F32)]),   # (E3M2 side: fp16 only)
    ("table id", ["fpq_gemm_a6w4_sqerr"], TABLE, [dict(a_table=E2M1), dict(a_table=E2M3), dict(a_table=-1)]),
    ("table id", ["fpq_gemm_w6_sqerr"], TABLE, [dict(w_table=E2M1), dict(a_table=E2M3), dict(w_table=9)]),
    ("table id", ["fpq_gemm_f6_rows_sqerr"], TABLE, [dict(a_table=E2M1), dict(w_table=E3M0)]),
    ("NULL operand", ALL, ARG, [dict(a=None), dict(sa=None), dict(w=None), dict(sw=None)]),
    ("codes only 8-byte aligned", ALL, ARG, [dict(a=PTR + 8), dict(w=PTR + 8)]),
    ("bias not 8-byte aligned", PER_GROUP, ARG, [dict(bias=PTR + 4), dict(bias=PTR + 2)]),
    ("NULL ref / row_weight / loss_out / workspace", ALL, ARG, [dict(ref=None), dict(row_weight=None), dict(loss_out=None), dict(workspace=None)]),
    ("ref / row_weight only 8-byte aligned", ALL, ARG, [dict(ref=PTR + 8), dict(row_weight=PTR + 8)]),
    ("loss_out / workspace only 2-byte aligned", ALL, ARG, [dict(loss_out=PTR + 2), dict(workspace=PTR + 2)]),
    ("ref dtype", ALL, DTYPE, [dict(ref_dtype=2), dict(ref_dtype=7), dict(ref_dtype=-1)]),
    # an empty problem still stores its 0.0f: the output and the workspace are checked, ref and row_weight are not read
    ("empty: NULL / misaligned loss_out or workspace", ALL, ARG,
     [dict(tokens=0, loss_out=None), dict(outs=0, workspace=None), dict(tokens=0, ref=None, row_weight=None, loss_out=PTR + 2)]),
    ("empty: ref dtype", ALL, DTYPE, [dict(tokens=0, ref_dtype=2), dict(outs=0, ref=None, ref_dtype=9)]),
]


@pytest.mark.parametrize("what,entries,code,cases", ONE_FAULT, ids=[f"{f[0]} [{len(f[1])}]" for f in ONE_FAULT])
def test_one_fault(lib, what, entries, code, cases):
    for entry in entries:
        for kw in cases:
            assert _call(lib, entry, **kw) == code, (what, entry, kw)


# two faults: the first one in the documented order is the one reported
ORDER = [
    ("the table before a negative size", ["fpq_gemm_a6w4_sqerr", "fpq_gemm_w6_sqerr", "fpq_gemm_f6_rows_sqerr"], TABLE, dict(a_table=-1, tokens=-1)),
    ("a negative size before the weight scale dtype", ALL, ARG, dict(tokens=-1, w_dtype=7)),
    ("the family's dtype before the form's pointers", ALL, DTYPE, dict(w_dtype=7, loss_out=None)),
    ("the family's shape before the form's pointers", ALL, SHAPE, dict(k=96, ref=None)),
    ("the family's shape before the form's dtype", ALL, SHAPE, dict(outs=380, ref_dtype=7)),
    ("the family's operands before the form's pointers", ALL, ARG, dict(a=PTR + 8, ref_dtype=7)),
    ("the family's operands before the form's dtype", ALL, ARG, dict(w=None, ref_dtype=7)),
    ("the form's pointers before its dtype", ALL, ARG, dict(ref=PTR + 8, ref_dtype=7)),
    ("the form's pointers before its dtype", ALL, ARG, dict(workspace=None, ref_dtype=7)),
    ("the family's shape before the empty problem", ALL, SHAPE, dict(tokens=0, k=96, loss_out=None)),
    ("the empty problem before the operands", ALL, DTYPE, dict(tokens=0, a=None, w=PTR + 8, ref_dtype=7)),
]


@pytest.mark.parametrize("what,entries,code,kw", ORDER, ids=[o[0] for o in ORDER])
def test_first_fault_in_the_documented_order(lib, what, entries, code, kw):
    for entry in entries:
        assert _call(lib, entry, **kw) == code, (what, entry)


def test_fp4_refuses_what_only_the_register_staged_kernel_serves(lib):
    """the plain FP4 entry point falls back to the register-staged kernel for a bias at an odd address; that kernel has no
    squared-error form"""
    assert _call(lib, "fpq_gemm_fp4_sqerr", bias=PTR + 4) == ARG
