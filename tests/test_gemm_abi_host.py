"""The matrix-core GEMM entry points without a GPU: which code a refused call returns, and - where a call has several faults -
which of them is reported.  That order is part of the C ABI (a caller sees one code), and it is what a change of the host
dispatch in fpq_gemm.hip must leave alone.  Every call below is refused or has no tokens / no outputs, so nothing is ever
launched and the pointers (a fake address with every alignment the checks ask for) are never read - as in
tests/test_fp6_split_abi.py.  The expected codes are the ones the library returned before the entry points shared their helpers."""
import ctypes

import pytest

OK, ARG, DTYPE, SHAPE, TABLE = 0, -1, -2, -3, -4
F16, F32 = 0, 1                                      # enum fpq_dtype
E2M1, E1M2, E3M0, E2M3, E3M2 = 0, 1, 2, 3, 4          # enum fpq_table
PTR = 0x7000_0000_1000


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as g
    g.build_hip()
    from fpqvar_amd import _lib
    return _lib.lib()


# the argument list of every entry point, by the names of the defaults below (the stream is always NULL)
_FP4 = "a sa w sw w_dtype bias"
_ROWS = "a sa a_dtype w sw w_dtype bias"
_F6 = "a sa a_dtype a_table w sw w_dtype w_table bias"
ENTRY = {
    "fpq_gemm_fp4_mx": _FP4 + " out tokens outs k",
    "fpq_gemm_fp4_mx_ex": _FP4 + " out tokens outs k epilogue",
    "fpq_gemm_fp4_mx_km": _FP4 + " out tokens outs k epilogue",
    "fpq_gemm_fp4_mx_split": _FP4 + " tokens outs k split kmajor",
    "fpq_gemm_fp4_mx_split_qknorm": _FP4 + " tokens outs k split head_scale kmajor",
    "fpq_gemm_fp4_gelu_dual": _FP4 + " out gelu_out tokens outs k nan_flag",
    "fpq_gemm_fp4_gelu_dual_km": _FP4 + " out gelu_out tokens outs k nan_flag",
    "fpq_gemm_a6w4_mx": "a sa a_table w sw w_dtype bias out tokens outs k epilogue",
    "fpq_gemm_fp6_rows": _ROWS + " out tokens outs k",
    "fpq_gemm_fp6_rows_ex": _ROWS + " out tokens outs k epilogue",
    "fpq_gemm_fp6_rows_km": _ROWS + " out tokens outs k epilogue",
    "fpq_gemm_fp6_rows_split": _ROWS + " tokens outs k split kmajor",
    "fpq_gemm_fp6_rows_split_qknorm": _ROWS + " tokens outs k split head_scale kmajor",
    "fpq_gemm_f6_rows": _F6 + " out tokens outs k epilogue kmajor",
    "fpq_gemm_f6_rows_split": _F6 + " tokens outs k split kmajor",
    "fpq_gemm_f6_rows_split_qknorm": _F6 + " tokens outs k split head_scale kmajor",
    "fpq_gemm_fp8_rows": _ROWS + " out tokens outs k",
    "fpq_gemm_fp8_rows_ex": _ROWS + " out tokens outs k epilogue",
}
FP4_PLAIN = ["fpq_gemm_fp4_mx", "fpq_gemm_fp4_mx_ex", "fpq_gemm_fp4_mx_km"]
FP4_SPLIT = ["fpq_gemm_fp4_mx_split", "fpq_gemm_fp4_mx_split_qknorm"]
GELU = ["fpq_gemm_fp4_gelu_dual", "fpq_gemm_fp4_gelu_dual_km"]
A6W4 = ["fpq_gemm_a6w4_mx"]
FP6_PLAIN = ["fpq_gemm_fp6_rows", "fpq_gemm_fp6_rows_ex", "fpq_gemm_fp6_rows_km", "fpq_gemm_f6_rows"]
FP6_SPLIT = ["fpq_gemm_fp6_rows_split", "fpq_gemm_fp6_rows_split_qknorm", "fpq_gemm_f6_rows_split", "fpq_gemm_f6_rows_split_qknorm"]
F6 = ["fpq_gemm_f6_rows", "fpq_gemm_f6_rows_split", "fpq_gemm_f6_rows_split_qknorm"]
FP8 = ["fpq_gemm_fp8_rows", "fpq_gemm_fp8_rows_ex"]
FP4_FAMILY = FP4_PLAIN + FP4_SPLIT + GELU + A6W4     # per-group scales, K limited by the scale tiles
SPLIT = FP4_SPLIT + FP6_SPLIT
NORM = [e for e in SPLIT if e.endswith("qknorm")]
NO_NORM = [e for e in SPLIT if not e.endswith("qknorm")]
ROWS = FP6_PLAIN + FP6_SPLIT + FP8                    # one scale per row, a dtype per side
ALL = list(ENTRY)
WITH_OUT = [e for e, sig in ENTRY.items() if " out " in sig]
WITH_EPILOGUE = [e for e, sig in ENTRY.items() if "epilogue" in sig]
assert len(ALL) == 18 and sorted(FP4_FAMILY + ROWS) == sorted(ALL)


def _split(part_cols=128, n_parts=3, rows_per_batch=4, out=(PTR, PTR, PTR), row_stride=None):
    from fpqvar_amd._lib import GemmSplit
    sp = GemmSplit()
    sp.part_cols, sp.n_parts, sp.rows_per_batch = part_cols, n_parts, rows_per_batch
    for p in range(3):
        sp.out[p], sp.row_stride[p], sp.batch_stride[p], sp.row0[p] = out[p], row_stride or part_cols, 16, 0
    return sp


def _call(lib, entry, split=(), epilogue=None, **kw):
    """`entry` with valid arguments (8 tokens, 3 x 128 outputs, K = 128) but for the overrides.  split: keywords of _split, or
    None for a NULL descriptor; epilogue: (gate, residual, rows_per_gate) or None."""
    from fpqvar_amd._lib import GemmEpilogue
    sp = None if split is None else _split(**dict(split))
    ep = None if epilogue is None else GemmEpilogue(*epilogue)
    args = dict(a=PTR, sa=PTR, w=PTR, sw=PTR, bias=None, out=PTR, gelu_out=None, nan_flag=None, head_scale=PTR,
                a_dtype=F16, w_dtype=F32, a_table=E1M2 if entry in A6W4 else E2M3, w_table=E2M3, kmajor=0, tokens=8, k=128,
                outs=384 if sp is None else sp.n_parts * sp.part_cols,
                split=None if sp is None else ctypes.byref(sp), epilogue=None if ep is None else ctypes.byref(ep))
    assert not set(kw) - set(args), kw
    args.update(kw)
    return getattr(lib, entry)(*[args[n] for n in ENTRY[entry].split()], None)


def _each_part(bad):
    return [dict(split=dict(out=tuple(bad if q == p else PTR for q in range(3)))) for p in range(3)]


# (what is wrong, the entry points it is tried on, the code, the overrides - several dicts: each is a call of its own)
ONE_FAULT = [
    ("negative tokens", ALL, ARG, [dict(tokens=-4)]),
    ("negative outs", ALL, ARG, [dict(outs=-8)]),
    ("negative k", ALL, ARG, [dict(k=-128)]),
    ("k % 128", ALL, SHAPE, [dict(k=96), dict(k=192)]),
    ("k == 0", ALL, ARG, [dict(k=0)]),
    ("k above the FP4 limit", FP4_FAMILY, SHAPE, [dict(k=128 * 65)]),
    ("outs % 8", FP4_PLAIN + A6W4 + FP6_PLAIN + FP8, SHAPE, [dict(outs=380)]),
    ("outs % 128 (fc1 tail)", GELU, SHAPE, [dict(outs=380), dict(outs=392)]),
    ("tokens above 2^31", FP4_PLAIN + A6W4 + FP6_PLAIN + FP8 + GELU, SHAPE, [dict(tokens=1 << 31)]),
    ("weight scale dtype", ALL, DTYPE, [dict(w_dtype=7), dict(w_dtype=2)]),
    ("activation scale dtype", ROWS, DTYPE, [dict(a_dtype=7), dict(a_dtype=2)]),
    ("fp32 activation scales with an E3M2 side", F6, DTYPE,
     [dict(a_dtype=F32, a_table=E3M2), dict(a_dtype=F32, w_table=E3M2), dict(a_dtype=F32, a_table=E3M2, w_table=E3M2)]),
    ("table id", F6, TABLE, [dict(a_table=E2M1), dict(w_table=E3M0), dict(a_table=9), dict(w_table=-1)]),
    ("table id (A6W4)", A6W4, TABLE, [dict(a_table=E2M1), dict(a_table=E2M3), dict(a_table=E3M2), dict(a_table=-1)]),
    ("NULL operand", ALL, ARG, [dict(a=None), dict(sa=None), dict(w=None), dict(sw=None)]),
    ("NULL out", WITH_OUT, ARG, [dict(out=None)]),
    ("codes only 8-byte aligned", ALL, ARG, [dict(a=PTR + 8), dict(w=PTR + 8)]),
    ("out only 8-byte aligned", WITH_OUT, ARG, [dict(out=PTR + 8)]),
    ("fc1 tail: GELU output / NaN scratch misaligned", GELU, ARG, [dict(gelu_out=PTR + 8), dict(nan_flag=PTR + 4)]),
    ("bias not 8-byte aligned", ["fpq_gemm_fp4_mx_km", "fpq_gemm_fp4_mx_split"] + GELU + A6W4, ARG, [dict(bias=PTR + 4), dict(bias=PTR + 2)]),
    ("bias not 8-byte aligned (k-major split)", ["fpq_gemm_fp4_mx_split"], ARG, [dict(bias=PTR + 4, kmajor=1)]),
    ("A6W4: odd scale addresses", A6W4, ARG, [dict(sa=PTR + 1), dict(sw=PTR + 2), dict(sw=PTR + 1, w_dtype=F16)]),
    ("k-major with fp16 weight scales", ["fpq_gemm_fp4_mx_km"], DTYPE, [dict(w_dtype=F16)]),
    ("k-major with fp16 weight scales (split)", FP4_SPLIT, DTYPE, [dict(w_dtype=F16, kmajor=1)]),
    ("k-major with fp16 weight scales (fc1 tail)", ["fpq_gemm_fp4_gelu_dual_km"], ARG, [dict(w_dtype=F16)]),
    ("k-major scale images only 8-byte aligned", ["fpq_gemm_fp4_mx_km", "fpq_gemm_fp4_gelu_dual_km"], ARG, [dict(sa=PTR + 8), dict(sw=PTR + 8)]),
    ("k-major scale images only 8-byte aligned (split)", FP4_SPLIT, ARG, [dict(sa=PTR + 8, kmajor=1), dict(sw=PTR + 8, kmajor=1)]),
    ("k-major: 2^28 tokens", ["fpq_gemm_fp4_mx_km"], SHAPE, [dict(tokens=1 << 28)]),
    ("k-major: 2^28 tokens (fc1 tail)", ["fpq_gemm_fp4_gelu_dual_km"], ARG, [dict(tokens=1 << 28)]),
    ("K past the 32-bit lane offsets of a tile", FP6_PLAIN + FP6_SPLIT, SHAPE, [dict(k=128 * 200000)]),
    ("K past the 32-bit lane offsets of a tile (FP8)", FP8, SHAPE, [dict(k=128 * 140000)]),
    ("NULL split", SPLIT, ARG, [dict(split=None)]),
    ("split: rows_per_batch", SPLIT, ARG, [dict(split=dict(rows_per_batch=0)), dict(split=dict(rows_per_batch=-4)), dict(split=dict(rows_per_batch=1 << 31))]),
    ("split: part_cols", SPLIT, ARG, [dict(split=dict(part_cols=192)), dict(split=dict(part_cols=0)), dict(split=dict(part_cols=-128))]),
    ("split: outs != n_parts * part_cols", SPLIT, ARG, [dict(outs=256), dict(outs=380)]),
    ("split: n_parts", SPLIT, ARG, [dict(split=dict(n_parts=0)), dict(split=dict(n_parts=4))]),
    ("split: a NULL destination", SPLIT, ARG, _each_part(None)),
    ("split: a destination not 8-byte aligned", SPLIT, ARG, _each_part(PTR + 4) + _each_part(PTR + 2)),
    ("split: row_stride", SPLIT, ARG, [dict(split=dict(row_stride=64)), dict(split=dict(row_stride=130))]),
    ("q / k norm: n_parts != 3", NORM, ARG, [dict(split=dict(n_parts=2)), dict(split=dict(n_parts=1))]),
    ("q / k norm: head scale", NORM, ARG, [dict(head_scale=None), dict(head_scale=PTR + 2)]),
    ("q / k norm: fp32 bias not 16-byte aligned", NORM, ARG, [dict(bias=PTR + 8), dict(bias=PTR + 4)]),
    ("epilogue: rows_per_gate with a gate", WITH_EPILOGUE, ARG, [dict(epilogue=(PTR, None, 0)), dict(epilogue=(PTR, PTR, -1)), dict(epilogue=(PTR, None, 1 << 31))]),
    ("epilogue: gate / residual misaligned", WITH_EPILOGUE, ARG, [dict(epilogue=(PTR + 8, None, 1)), dict(epilogue=(None, PTR + 8, 1)), dict(epilogue=(PTR, PTR + 2, 4))]),
    # the two known differences between the families' split forms (include/fpq.h asks for 8-byte aligned destinations and
    # says nothing of whole batch entries)
    ("FP6 split: tokens % rows_per_batch", FP6_SPLIT, ARG, [dict(split=dict(rows_per_batch=3)), dict(split=dict(rows_per_batch=16))]),
    ("FP4 split: part 0 is held to 16 bytes once there are tokens", FP4_SPLIT, ARG,
     [dict(split=dict(out=(PTR + 8, PTR + 8, PTR + 8))), dict(split=dict(out=(PTR + 8, PTR, PTR)))]),
]
NOTHING_TO_DO = [
    ("no tokens", ALL, OK, [dict(tokens=0)]),
    ("no outputs", FP4_PLAIN + GELU + A6W4 + FP6_PLAIN + FP8, OK, [dict(outs=0)]),
    ("no tokens: pointers are not looked at", ALL, OK, [dict(tokens=0, a=None), dict(tokens=0, a=PTR + 8, w=PTR + 4, sw=None)]),
    ("no tokens: out is not looked at", WITH_OUT, OK, [dict(tokens=0, out=PTR + 2), dict(tokens=0, out=None)]),
    ("no tokens: 8-byte aligned destinations, all parts", SPLIT, OK, [dict(tokens=0, split=dict(out=(PTR + 8, PTR + 8, PTR + 8)))]),
    ("no tokens: fewer parts", NO_NORM, OK, [dict(tokens=0, split=dict(n_parts=2)), dict(tokens=0, split=dict(n_parts=1))]),
    ("no tokens: a 16-byte aligned fp32 bias", NORM, OK, [dict(tokens=0, bias=PTR + 16)]),
    ("no tokens: rows_per_gate is read with a gate only", WITH_EPILOGUE, OK, [dict(tokens=0, epilogue=(None, PTR, 0))]),
    ("no tokens: every E3M2 pair with fp16 activation scales", F6, OK,
     [dict(tokens=0, a_table=E3M2), dict(tokens=0, w_table=E3M2, w_dtype=F16), dict(tokens=0, a_table=E3M2, w_table=E3M2)]),
    ("no tokens: both A6W4 tables", A6W4, OK, [dict(tokens=0, a_table=E3M0), dict(tokens=0, a_table=E1M2, w_dtype=F16)]),
]
# two faults at once: the one that is reported
TWO_FAULTS = [
    ("table before sizes", F6 + A6W4, TABLE, [dict(a_table=E2M1, tokens=-4), dict(a_table=E2M1, k=96), dict(a_table=E2M1, w_dtype=7)]),
    ("table before a NULL split", ["fpq_gemm_f6_rows_split", "fpq_gemm_f6_rows_split_qknorm"], TABLE, [dict(w_table=E2M1, split=None)]),
    ("table before the head scale", ["fpq_gemm_f6_rows_split_qknorm"], TABLE, [dict(a_table=E3M0, head_scale=None)]),
    ("negative size before the epilogue", WITH_EPILOGUE, ARG, [dict(tokens=-4, k=96), dict(outs=-8, w_dtype=7)]),
    ("epilogue before dtype and shape", WITH_EPILOGUE, ARG, [dict(epilogue=(PTR, None, 0), w_dtype=7), dict(epilogue=(None, PTR + 8, 1), k=96)]),
    ("split before dtype and shape", SPLIT, ARG, [dict(split=dict(part_cols=192), w_dtype=7), dict(split=dict(row_stride=130), k=96),
                                                  dict(split=dict(n_parts=4), tokens=0)]),
    ("q / k norm arguments before sizes", NORM, ARG, [dict(head_scale=None, k=96), dict(bias=PTR + 8, w_dtype=7), dict(split=dict(n_parts=2), tokens=0)]),
    ("per-group GEMMs: dtype before shape", FP4_FAMILY, DTYPE, [dict(w_dtype=7, k=96), dict(w_dtype=7, tokens=0)]),
    ("row-scaled GEMMs: shape before dtype", ROWS, SHAPE, [dict(w_dtype=7, k=96), dict(a_dtype=7, k=96)]),
    ("row-scaled GEMMs: dtype before nothing-to-do", ROWS, DTYPE, [dict(a_dtype=7, tokens=0), dict(w_dtype=7, tokens=0)]),
    ("E3M2 pair with fp32 activation scales before nothing-to-do", F6, DTYPE, [dict(a_dtype=F32, w_table=E3M2, tokens=0)]),
    ("shape before nothing-to-do", ALL, SHAPE, [dict(k=96, tokens=0)]),
    ("shape before pointers", ALL, SHAPE, [dict(k=96, a=None), dict(k=192, w=PTR + 8)]),
    ("NULL before alignment (same code)", ALL, ARG, [dict(a=None, w=PTR + 8)]),
    ("pointers before the lane-offset bound", FP6_PLAIN + FP6_SPLIT, ARG, [dict(k=128 * 200000, a=None)]),
    ("k-major: dtype before the scale images' alignment", ["fpq_gemm_fp4_mx_km"], DTYPE, [dict(w_dtype=F16, sa=PTR + 8)]),
    ("k-major: 2^28 tokens before the scale images' alignment", ["fpq_gemm_fp4_mx_km"], SHAPE, [dict(tokens=1 << 28, sa=PTR + 8)]),
    ("k-major: scale images before k % 128", ["fpq_gemm_fp4_mx_km"], ARG, [dict(sa=PTR + 8, k=96)]),
    ("k-major split: descriptor before the weight scale dtype", FP4_SPLIT, ARG, [dict(split=dict(part_cols=0), w_dtype=F16, kmajor=1)]),
    ("fc1 tail: shape before the k-major rules", ["fpq_gemm_fp4_gelu_dual_km"], SHAPE, [dict(w_dtype=F16, outs=392)]),
    ("FP4 split: whole batch entries are not asked for", FP4_SPLIT, SHAPE, [dict(split=dict(rows_per_batch=3), k=96)]),
    ("FP6 split: whole batch entries come before shape", FP6_SPLIT, ARG, [dict(split=dict(rows_per_batch=3), k=96)]),
    ("FP4 split: bias alignment after the operand pointers' (same code), before K too long", ["fpq_gemm_fp4_mx_split"], SHAPE, [dict(bias=PTR + 4, k=128 * 65)]),
]


def _run(lib, rows):
    wrong = []
    for what, entries, code, calls in rows:
        for entry in entries:
            for kw in calls:
                got = _call(lib, entry, **kw)
                if got != code:
                    wrong.append((what, entry, kw, got, code))
    assert not wrong, "\n".join(f"{w}: {e}({k}) returned {g}, expected {c}" for w, e, k, g, c in wrong)


def test_one_fault_per_call(lib):
    _run(lib, ONE_FAULT)


def test_nothing_to_do_is_ok_and_launches_nothing(lib):
    _run(lib, NOTHING_TO_DO)


def test_two_faults_the_order_of_the_checks(lib):
    _run(lib, TWO_FAULTS)


def test_every_entry_point_is_covered():
    for rows in (ONE_FAULT, NOTHING_TO_DO, TWO_FAULTS):
        seen = {e for _, entries, _, _ in rows for e in entries}
        assert seen == set(ALL), sorted(set(ALL) - seen)
    # no row can reach a launch: it is refused (a code below zero), or it has no tokens / no outputs
    for what, _, code, calls in ONE_FAULT + NOTHING_TO_DO + TWO_FAULTS:
        assert code < 0 or all(kw.get("tokens") == 0 or kw.get("outs") == 0 for kw in calls), what
