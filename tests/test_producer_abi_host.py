"""The producer entry points (row quantizers, operand emitters, decoders, KV step and pack, rotate and adaLN front ends) without
a GPU: which code a refused call returns, and - where a call has several faults - which of them is reported.  That order is
part of the C ABI (a caller sees one code) and it is what a change of the host dispatch in fpq_kernels.hip, fpq_rotate.hip
and fpq_adaln.hip must leave alone.  The manner is that of tests/test_gemm_abi_host.py: every call below is refused or has
nothing to do (no rows, no elements, no segments), so nothing is ever launched and the pointers (a fake address with every
alignment the checks ask for) are never read.  The expected codes are the ones the library returned before the producers
shared their launch path.

Not covered, because no call can reach them without passing every check (it would then launch on the fake address):
  * fpq_absmax with n == 0 (it clears `out` first) and fpq_quant_tensor_argmin with n == 0 (it launches on one workgroup):
    only their refusals are here;
  * FPQ_ERR_TABLE for "no travelling table image" (fpq_kv_cache_step, fpq_kv_pack, the rotate and adaLN forms,
    fpq_quant_rows_codes_g6): every table pair compresses into the kernel arguments (fpq_fast16.h, lut16_compress:
    <= 1216 of 1280 entries for the widest), so no table id reaches those returns; nor adaLN's `shift < 6` (no symmetric table
    has more than 2 x 512 buckets);
  * FPQ_ERR_SHAPE inside launch_fast16 for the GELU and clamp forms at cols != 128: fpq_gelu_quant_rows_dual sends every other
    row length to the one-workgroup-per-row kernels and fpq_quant_rows_dual takes the clamp there at cols == 128 only.  The
    shape refusals these two entry points can make themselves are below."""
import ctypes

import pytest

OK, ARG, DTYPE, SHAPE, TABLE = 0, -1, -2, -3, -4
F16, F32, F64 = 0, 1, 2                                # enum fpq_dtype
E2M1, E1M2, E3M0, E2M3, E3M2, E1M2_NEG, E2M1_POS, INT_NEG, E2M3_POS, E2M1_NEG = range(10)   # enum fpq_table
PTR = 0x7000_0000_1000
SIGN = (ctypes.c_uint32 * 4)(1, 2, 3, 4)


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as g
    g.build_hip()
    from fpqvar_amd import _lib
    return _lib.lib()


# the argument list of every entry point, by the names of the defaults below (the stream is always NULL)
_ADALN = "in_dtype scale shift mod_dtype rows_per_batch eps smooth sign"
_KV = "cache batch max_len row_elems quant_start quant_stop"
_KVNEW = "new_batch_pitch new_token_pitch new_start n_new group table_id"
ENTRY = {
    "fpq_quant_nearest": "x table z n k dtype",
    "fpq_quant_nearest_argmin": "x table z n k dtype",
    "fpq_quant_nearest_builtin": "x z n table_id",
    "fpq_quant_rows": "x out rows cols table_id in_dtype out_dtype",
    "fpq_quant_rows_multi": "segs n_segments cols table_id in_dtype out_dtype",
    "fpq_quant_rows_segments": "segs n_segments max_rows cols table_id in_dtype out_dtype",
    "fpq_kv_cache_step": _KV + " new_k new_v " + _KVNEW,
    "fpq_kv_cache_step_qknorm": _KV + " new_q new_k new_v " + _KVNEW + " q_out q_head_scale bias head_dim",
    "fpq_quant_rows_argmin": "x out rows cols table_id in_dtype clamp3",
    "fpq_quant_rows_dual": "x out rows cols neg_table pos_table in_dtype out_dtype clip clip_strength nan_flag",
    "fpq_gelu_quant_rows_dual": "x out gelu_out rows cols neg_table pos_table nan_flag",
    "fpq_quant_rows_neg_reverse": "x out rows cols table_id in_dtype",
    "fpq_quant_rows_dual_argmin": "x out rows cols neg_table pos_table in_dtype clip clip_strength",
    "fpq_quant_rows_codes_mx": "x codes scales rows cols in_dtype",
    "fpq_quant_rows_codes_mx_km": "x codes scales rows cols in_dtype",
    "fpq_quant_rows_codes_g6": "x codes scales rows cols table_id in_dtype",
    "fpq_kv_pack": "codes scales kv_bit batch max_len heads head_dim pos new_k new_v new_batch_pitch new_token_pitch n_new",
    "fpq_absmax": "x n in_dtype out",
    "fpq_quant_tensor_argmin": "x out scale_out workspace n table_id in_dtype",
    "fpq_quant_rows_codes": "x codes scales rows cols table_id in_dtype pack",
    "fpq_dequant_rows_codes": "codes scales out rows cols table_id scale_dtype out_dtype pack",
    "fpq_quant_rows_codes_segments": "segs n_segments max_rows cols table_id in_dtype pack",
    "fpq_dequant_rows_codes_segments": "segs n_segments max_rows cols table_id scale_dtype out_dtype pack",
    "fpq_rotate_quant_rows": "x out rotated_out rows cols in_dtype smooth sign table_id",
    "fpq_rotate_quant_rows_codes_mx": "x codes scales rows cols in_dtype smooth sign",
    "fpq_rotate_quant_rows_codes_mx_km": "x codes scales rows cols in_dtype smooth sign",
    "fpq_quant_rows_codes_fp8": "x codes scales rows cols table_id in_dtype",
    "fpq_quant_rows_codes_fp6": "x codes scales rows cols table_id in_dtype",
    "fpq_quant_rows_codes_fp6_km": "x codes scales rows cols table_id in_dtype",
    "fpq_quant_rows_codes_f6": "x codes scales rows cols table_id in_dtype kmajor",
    "fpq_adaln_rotate_quant_rows": "x out h_out rotated_out rows cols " + _ADALN + " table_id",
    "fpq_adaln_rotate_quant_rows_codes_mx": "x codes scales rows cols " + _ADALN,
    "fpq_adaln_rotate_quant_rows_codes_mx_km": "x codes scales rows cols " + _ADALN,
    "fpq_adaln_rotate_quant_token_rows": "x out h_out rotated_out scales rows cols " + _ADALN + " table_id",
    "fpq_adaln_rotate_quant_token_rows_codes_fp8": "x codes scales rows cols " + _ADALN + " table_id",
    "fpq_adaln_rotate_quant_token_rows_codes_fp6": "x codes scales rows cols " + _ADALN + " table_id",
    "fpq_adaln_rotate_quant_token_rows_codes_fp6_km": "x codes scales rows cols " + _ADALN + " table_id",
    "fpq_adaln_rotate_quant_token_rows_codes_f6": "x codes scales rows cols " + _ADALN + " table_id kmajor",
}
ALL = list(ENTRY)
assert len(ALL) == 38


def having(*names, but=()):
    return [e for e in ALL if all(n in ENTRY[e].split() for n in names) and e not in but]


ADALN = [e for e in ALL if e.startswith("fpq_adaln")]
ADALN_TOKEN = [e for e in ADALN if "token" in e]
ROTATE = [e for e in ALL if e.startswith("fpq_rotate")]
FP6_ONLY = ["fpq_quant_rows_codes_fp6", "fpq_quant_rows_codes_fp6_km", "fpq_adaln_rotate_quant_token_rows_codes_fp6",
            "fpq_adaln_rotate_quant_token_rows_codes_fp6_km"]                      # E2M3, nothing else
F6 = ["fpq_quant_rows_codes_f6", "fpq_adaln_rotate_quant_token_rows_codes_f6"]      # E2M3 or E3M2
G6 = ["fpq_quant_rows_codes_g6"]                                                    # E1M2 or E3M0
DUAL = having("neg_table", "pos_table")
SEGMENTS = having("segs", "max_rows")
KV_STEP = ["fpq_kv_cache_step", "fpq_kv_cache_step_qknorm"]
ROWS = having("rows", "cols")                         # one tensor of rows x cols
SYMMETRIC = having("table_id", but=FP6_ONLY + F6 + G6 + ["fpq_quant_nearest_builtin"])   # any of the five symmetric tables
IN_DTYPE = having("in_dtype")
NO_EMPTY_CALL = ["fpq_absmax", "fpq_quant_tensor_argmin"]
ADALN_FP6 = [e for e in ADALN if "fp6" in e or e.endswith("_f6")]
ADALN_TABLE_FIRST = ADALN_FP6 + ["fpq_adaln_rotate_quant_token_rows_codes_fp8"]      # their own table check sits in front of the shared ones
COLS128 = ["fpq_quant_rows_codes_mx", "fpq_quant_rows_codes_mx_km"] + G6 + ROTATE + ADALN   # groups of 128
SHAPED = COLS128 + [e for e in FP6_ONLY + F6 if e not in ADALN]                             # ... or FP6 blocks of 32
EMPTY = "_nothing_to_do"   # an override that stands for _nothing_to_do(entry)


def _segments(rows=(8, 8), x=PTR, out=PTR):
    from fpqvar_amd._lib import Segment
    arr = (Segment * len(rows))()
    for i, r in enumerate(rows):
        arr[i].x, arr[i].out, arr[i].rows = x, out, r
    return arr


def _call(lib, entry, **kw):
    """`entry` with valid arguments (8 rows of 128 fp16 elements; segments: two, on the device; the KV cache: one new token behind
    four to re-quantize) but for the overrides.  host_segments: keywords of _segments (fpq_quant_rows_multi only)."""
    fp6 = entry in FP6_ONLY + F6
    args = dict(x=PTR, out=PTR, z=PTR, table=PTR, codes=PTR, scales=PTR, gelu_out=None, nan_flag=None, clip=None, clip_strength=1.0,
                rotated_out=None, h_out=None, smooth=None, sign=SIGN, scale=PTR, shift=PTR, scale_out=PTR, workspace=PTR,
                rows=8, cols=128, n=16, k=8, clamp3=0, pack=0, kmajor=0, rows_per_batch=4, eps=1e-6,
                table_id=E2M3 if fp6 else E1M2 if entry in G6 else E2M1, neg_table=E1M2_NEG, pos_table=E2M1_POS,
                dtype=F32, in_dtype=F32 if entry == "fpq_quant_rows_segments" else F16, out_dtype=F16, scale_dtype=F16, mod_dtype=F16,
                segs=PTR, n_segments=2, max_rows=8,
                cache=PTR, batch=1, max_len=16, row_elems=128, quant_start=0, quant_stop=4, new_q=PTR, new_k=PTR, new_v=PTR,
                new_batch_pitch=2048, new_token_pitch=128, new_start=4, n_new=1, group=128, q_out=PTR, q_head_scale=PTR, bias=None,
                head_dim=64, kv_bit=6, heads=2, pos=0)
    host = kw.pop("host_segments", None)
    if entry == "fpq_quant_rows_multi":
        keep = _segments(**(host or {}))
        args["segs"] = ctypes.cast(keep, ctypes.c_void_p)
    assert not set(kw) - set(args), kw
    args.update(kw)
    return getattr(lib, entry)(*[args[n] for n in ENTRY[entry].split()], None)


def _nothing_to_do(entry):
    """the override that leaves `entry` without work"""
    if entry in ROWS:
        return dict(rows=0)
    if entry in SEGMENTS or entry == "fpq_quant_rows_multi":
        return dict(n_segments=0)
    if entry in KV_STEP:
        return dict(batch=0)
    return dict(n_new=0) if entry == "fpq_kv_pack" else dict(n=0)


BIG = 1 << 37   # rows whose tiles no longer fit a grid's x dimension
# (what is wrong, the entry points it is tried on, the code, the overrides - several dicts: each is a call of its own)
ONE_FAULT = [
    ("negative rows / cols", ROWS, ARG, [dict(rows=-1), dict(cols=-128)]),
    ("negative n", having("n"), ARG, [dict(n=-1)]),
    ("negative segment count, row bound, cols", SEGMENTS, ARG, [dict(n_segments=-1), dict(max_rows=-1), dict(cols=-128)]),
    ("multi: negative counts, NULL table of segments", ["fpq_quant_rows_multi"], ARG, [dict(n_segments=-1), dict(cols=-8), dict(segs=None)]),
    ("multi: a segment with negative rows or a NULL side", ["fpq_quant_rows_multi"], ARG,
     [dict(host_segments=dict(rows=(8, -1))), dict(host_segments=dict(x=None)), dict(host_segments=dict(out=None))]),
    ("k of the scan", ["fpq_quant_nearest", "fpq_quant_nearest_argmin"], SHAPE, [dict(k=0), dict(k=257)]),
    ("dtype of the scan", ["fpq_quant_nearest"], DTYPE, [dict(dtype=F16), dict(dtype=7)]),
    ("dtype of the argmin scan", ["fpq_quant_nearest_argmin"], DTYPE, [dict(dtype=F64), dict(dtype=7)]),
    ("table id out of range", ["fpq_quant_nearest_builtin"], TABLE, [dict(table_id=-1), dict(table_id=10)]),
    ("table id: out of range or a half table", SYMMETRIC, TABLE, [dict(table_id=-1), dict(table_id=10), dict(table_id=E1M2_NEG), dict(table_id=E2M3_POS)]),
    ("table id: E2M3 only", FP6_ONLY, TABLE, [dict(table_id=E3M2), dict(table_id=E2M1), dict(table_id=-1)]),
    ("table id: E2M3 or E3M2", F6, TABLE, [dict(table_id=E2M1), dict(table_id=E3M0), dict(table_id=10)]),
    ("table id: E1M2 or E3M0", G6, TABLE, [dict(table_id=E2M1), dict(table_id=E2M3), dict(table_id=-1)]),
    ("dual pair", DUAL, TABLE, [dict(neg_table=E2M1), dict(neg_table=E2M1_POS), dict(pos_table=E1M2_NEG), dict(pos_table=E2M3), dict(neg_table=10), dict(pos_table=-1)]),
    ("input dtype", having("in_dtype", but=["fpq_quant_rows_segments"]), DTYPE, [dict(in_dtype=F64), dict(in_dtype=7)]),
    ("fp32 segments only", ["fpq_quant_rows_segments"], DTYPE, [dict(in_dtype=F16), dict(in_dtype=F64)]),
    ("output dtype", having("out_dtype"), DTYPE, [dict(out_dtype=F64), dict(out_dtype=-1)]),
    ("scale dtype", having("scale_dtype"), DTYPE, [dict(scale_dtype=F64), dict(scale_dtype=7)]),
    ("modulation dtype", ADALN, DTYPE, [dict(mod_dtype=F64), dict(mod_dtype=7)]),
    ("k-major FP4 codes from fp16 rows only", ["fpq_quant_rows_codes_mx_km"], DTYPE, [dict(in_dtype=F32)]),
    ("NULL operand", having("x", "out", but=["fpq_absmax", "fpq_quant_tensor_argmin"]), ARG, [dict(x=None), dict(out=None)]),
    ("NULL operand (codes out)", having("x", "codes", "scales"), ARG, [dict(x=None), dict(codes=None), dict(scales=None)]),
    ("NULL operand (scan)", ["fpq_quant_nearest", "fpq_quant_nearest_argmin"], ARG, [dict(x=None), dict(table=None), dict(z=None)]),
    ("NULL operand (built-in scan)", ["fpq_quant_nearest_builtin"], ARG, [dict(x=None), dict(z=None)]),
    ("NULL operand (decoder)", ["fpq_dequant_rows_codes"], ARG, [dict(codes=None), dict(scales=None), dict(out=None)]),
    ("NULL or misaligned segment table", SEGMENTS, ARG, [dict(segs=None), dict(segs=PTR + 4)]),
    ("absmax: NULL out, NULL x", ["fpq_absmax"], ARG, [dict(out=None), dict(out=None, n=0)]),
    ("per-tensor argmin: scale / workspace", ["fpq_quant_tensor_argmin"], ARG,
     [dict(scale_out=None), dict(workspace=None), dict(workspace=PTR + 2), dict(scale_out=PTR + 1), dict(scale_out=None, n=0)]),
    ("per-tensor argmin: NULL x / out with elements", ["fpq_quant_tensor_argmin"], ARG, [dict(x=None), dict(out=None)]),
    ("segments: cols != 128", SEGMENTS, SHAPE, [dict(cols=64), dict(cols=256)]),
    ("segments: more than 65535", SEGMENTS, SHAPE, [dict(n_segments=65536)]),
    ("segments: tiles past a grid's x dimension", ["fpq_quant_rows_segments", "fpq_quant_rows_codes_segments"], SHAPE,
     [dict(max_rows=BIG, in_dtype=F32)]),
    ("fp32 groups of 128: tiles past a grid's x dimension", ["fpq_quant_rows", "fpq_quant_rows_codes"], SHAPE, [dict(rows=BIG, in_dtype=F32)]),
    ("multi: tiles past a grid's x dimension", ["fpq_quant_rows_multi"], SHAPE, [dict(host_segments=dict(rows=(8, BIG)))]),
    ("nibbles cannot hold FP6 codes", having("pack"), SHAPE, [dict(pack=1, table_id=E2M3), dict(pack=1, table_id=E3M2)]),
    ("cols % 128", COLS128, SHAPE, [dict(cols=64), dict(cols=192)]),
    ("cols % 32 (FP6 operands)", FP6_ONLY + F6, SHAPE, [dict(cols=48), dict(cols=144)]),
    ("cols % 128 (k-major FP6 operands)", ["fpq_quant_rows_codes_fp6_km", "fpq_adaln_rotate_quant_token_rows_codes_fp6_km"], SHAPE, [dict(cols=160)]),
    ("cols % 128 (k-major FP6 operands, by argument)", F6, SHAPE, [dict(cols=160, kmajor=1)]),
    ("k-major image past 2^31", ["fpq_quant_rows_codes_mx_km", "fpq_quant_rows_codes_fp6_km", "fpq_rotate_quant_rows_codes_mx_km",
                                 "fpq_adaln_rotate_quant_rows_codes_mx_km", "fpq_adaln_rotate_quant_token_rows_codes_fp6_km"], SHAPE,
     [dict(rows=1 << 31), dict(rows=1 << 20, cols=4096)]),
    ("k-major image past 2^31 (by argument)", F6, SHAPE, [dict(rows=1 << 31, kmajor=1)]),
    ("adaLN k-major: rows beyond one wavefront", ["fpq_adaln_rotate_quant_rows_codes_mx_km"], SHAPE, [dict(cols=2688), dict(cols=4096)]),
    ("codes: operands not 16-byte aligned", ["fpq_quant_rows_codes_mx", "fpq_quant_rows_codes_mx_km"], ARG,
     [dict(x=PTR + 8), dict(codes=PTR + 8), dict(scales=PTR + 8)]),
    ("g6: alignment", G6, ARG, [dict(x=PTR + 8), dict(codes=PTR + 8), dict(scales=PTR + 1), dict(scales=PTR + 2, in_dtype=F32)]),
    ("FP6 codes not 8-byte aligned", FP6_ONLY + F6, ARG, [dict(codes=PTR + 4)]),
    ("rotate / adaLN: an operand not 16-byte aligned", ROTATE + ADALN, ARG, [dict(x=PTR + 8), dict(smooth=PTR + 8)]),
    ("rotate / adaLN: NULL sign masks", ROTATE + ADALN, ARG, [dict(sign=None)]),
    ("rotate / adaLN: outputs not 16-byte aligned", ["fpq_rotate_quant_rows", "fpq_adaln_rotate_quant_rows", "fpq_adaln_rotate_quant_token_rows"], ARG,
     [dict(out=PTR + 8), dict(rotated_out=PTR + 8)]),
    ("adaLN: h_out / modulation not 16-byte aligned", ["fpq_adaln_rotate_quant_rows", "fpq_adaln_rotate_quant_token_rows"], ARG, [dict(h_out=PTR + 8)]),
    ("adaLN: modulation", ADALN, ARG, [dict(scale=None), dict(shift=None), dict(scale=PTR + 8), dict(shift=PTR + 4), dict(rows_per_batch=0), dict(rows_per_batch=-4)]),
    ("adaLN: cols > 4096", ADALN, SHAPE, [dict(cols=4224)]),
    ("adaLN per token: cols > 2560", ADALN_TOKEN, SHAPE, [dict(cols=2688), dict(cols=4096)]),
    ("adaLN per token: odd address of the row scales", ["fpq_adaln_rotate_quant_token_rows"], ARG, [dict(scales=PTR + 1)]),
    ("adaLN: workgroups past a grid's x dimension", ADALN, SHAPE, [dict(rows=1 << 40, rows_per_batch=1)]),
    ("GELU form: cols", ["fpq_gelu_quant_rows_dual"], SHAPE, [dict(cols=0), dict(cols=100), dict(cols=16392)]),
    ("GELU form: alignment", ["fpq_gelu_quant_rows_dual"], ARG, [dict(x=PTR + 8), dict(out=PTR + 8), dict(gelu_out=PTR + 8), dict(nan_flag=PTR + 4)]),
    ("dual: NaN flag not 8-byte aligned", ["fpq_quant_rows_dual"], ARG, [dict(nan_flag=PTR + 4)]),
    ("KV step: sizes", KV_STEP, ARG, [dict(batch=-1), dict(max_len=-1), dict(row_elems=0), dict(n_new=-1)]),
    ("KV step: the ranges", KV_STEP, ARG, [dict(quant_start=-1), dict(quant_stop=0, quant_start=2), dict(new_start=3), dict(n_new=13)]),
    ("KV step: group", ["fpq_kv_cache_step"], SHAPE, [dict(group=24), dict(group=1024), dict(group=0)]),
    ("KV step: row_elems % group, batch", KV_STEP, SHAPE, [dict(row_elems=192), dict(batch=65536)]),
    ("KV step: pitches", KV_STEP, SHAPE, [dict(new_batch_pitch=2052), dict(new_token_pitch=132), dict(new_token_pitch=-128), dict(new_batch_pitch=-2048)]),
    ("KV step: pointers", KV_STEP, ARG, [dict(cache=None), dict(new_k=None), dict(new_v=None), dict(cache=PTR + 8), dict(new_k=PTR + 8), dict(new_v=PTR + 8)]),
    ("KV step: tiles past a grid's x dimension", KV_STEP, SHAPE, [dict(quant_stop=BIG, new_start=BIG, n_new=0, max_len=BIG * 2)]),
    ("KV step with q / k norm: head_dim, row_elems, group", ["fpq_kv_cache_step_qknorm"], ARG,
     [dict(head_dim=128), dict(row_elems=96), dict(row_elems=0), dict(group=32), dict(group=256)]),
    ("KV step with q / k norm: its own pointers", ["fpq_kv_cache_step_qknorm"], ARG,
     [dict(q_head_scale=None), dict(q_head_scale=PTR + 2), dict(bias=PTR + 8), dict(new_q=None), dict(q_out=None), dict(new_q=PTR + 8), dict(q_out=PTR + 8)]),
    ("KV pack: sizes", ["fpq_kv_pack"], ARG, [dict(batch=-1), dict(max_len=-1), dict(heads=0), dict(head_dim=128), dict(pos=-1), dict(n_new=-1),
                                             dict(pos=16), dict(kv_bit=8), dict(kv_bit=4, heads=3), dict(batch=65536), dict(heads=(1 << 20) + 2)]),
    ("KV pack: pitches", ["fpq_kv_pack"], ARG, [dict(new_batch_pitch=2052), dict(new_token_pitch=132), dict(new_token_pitch=-128)]),
    ("KV pack: pointers", ["fpq_kv_pack"], ARG, [dict(codes=None), dict(scales=None), dict(new_k=None), dict(new_v=None), dict(codes=PTR + 8), dict(new_v=PTR + 8)]),
    ("KV pack: tiles past a grid's x dimension", ["fpq_kv_pack"], ARG, [dict(n_new=1 << 40, max_len=1 << 41, heads=1 << 10)]),
]
NOTHING_TO_DO = [
    ("nothing to do", [e for e in ALL if e not in NO_EMPTY_CALL], OK, [None]),
    ("nothing to do: pointers are not looked at", having("x", but=NO_EMPTY_CALL), OK, [{"x": None, EMPTY: 1}, {"x": PTR + 2, EMPTY: 1}]),
    ("no columns", [e for e in ROWS if e != "fpq_gelu_quant_rows_dual"], OK, [dict(cols=0, rows=8, x=None)]),
    ("segments: no rows in any", SEGMENTS, OK, [dict(max_rows=0, segs=None)]),
    ("multi: no columns, or segments without rows", ["fpq_quant_rows_multi"], OK,
     [dict(cols=0, n_segments=2), dict(n_segments=2, host_segments=dict(rows=(0, 0), x=None)), dict(n_segments=2, in_dtype=F32, host_segments=dict(rows=(0, 0)))]),
    ("KV step: nothing to re-quantize and nothing new", KV_STEP, OK, [dict(quant_stop=0, new_start=0, n_new=0, batch=1, cache=None)]),
    ("KV pack: no batch", ["fpq_kv_pack"], OK, [dict(batch=0, n_new=1, codes=None)]),
]
# two faults at once: the one that is reported
TWO_FAULTS = [
    ("sizes before the table", [e for e in SYMMETRIC + G6 + FP6_ONLY if e not in ADALN_TABLE_FIRST], ARG,
     [dict(rows=-1, n=-1, n_segments=-1, batch=-1, table_id=10)]),
    ("built-in scan: n before the table", ["fpq_quant_nearest_builtin"], ARG, [dict(n=-1, table_id=10)]),
    ("the table before sizes (a table check of the entry point's own)", ["fpq_quant_rows_codes_f6"] + ADALN_TABLE_FIRST, TABLE, [dict(rows=-1, table_id=10)]),
    ("sizes before the pair", DUAL, ARG, [dict(rows=-1, neg_table=E2M1)]),
    ("the table before the dtype", having("table_id", "in_dtype"), TABLE, [dict(table_id=10, in_dtype=7)]),
    ("the pair before the dtype", ["fpq_quant_rows_dual", "fpq_quant_rows_dual_argmin"], TABLE, [dict(pos_table=E2M3, in_dtype=7)]),
    ("the dtype before nothing-to-do", [e for e in IN_DTYPE if e not in NO_EMPTY_CALL], DTYPE, [{"in_dtype": 7, EMPTY: 1}]),
    ("the dtype before the shape", having("in_dtype", "cols", but=["fpq_quant_rows_multi"] + ADALN_FP6), DTYPE, [dict(in_dtype=7, cols=200)]),
    ("adaLN FP6 operands: the shape before the dtype", ADALN_FP6, SHAPE, [dict(in_dtype=7, cols=48)]),
    ("the shape before nothing-to-do", SEGMENTS + SHAPED, SHAPE, [{"cols": 200, EMPTY: 1}]),
    ("nibbles before nothing-to-do", having("pack"), SHAPE, [{"pack": 1, "table_id": E2M3, EMPTY: 1}]),
    ("the shape before the pointers", SHAPED, SHAPE, [dict(cols=200, x=None)]),
    ("NULL before alignment (same code)", ROTATE + ADALN, ARG, [dict(x=None, smooth=PTR + 8)]),
    ("rotate / adaLN codes: the NULL scales before everything", [e for e in ROTATE + ADALN if "codes" in e and not e.endswith("_f6")], ARG,
     [dict(scales=None, in_dtype=7), dict(scales=None, cols=200), dict(scales=None, sign=None)]),
    ("adaLN operands by format: the table before the NULL scales", ["fpq_adaln_rotate_quant_token_rows_codes_f6"], TABLE, [dict(scales=None, table_id=E2M1)]),
    ("adaLN FP8 operands: the NULL scales before the table", ["fpq_adaln_rotate_quant_token_rows_codes_fp8"], ARG, [dict(scales=None, table_id=10)]),
    ("adaLN FP6 operands: the table before the shape, the shape before the codes' alignment",
     ["fpq_adaln_rotate_quant_token_rows_codes_fp6", "fpq_adaln_rotate_quant_token_rows_codes_f6"], TABLE, [dict(table_id=E2M1, cols=48)]),
    ("adaLN FP6 operands: the shape before the codes' alignment",
     ["fpq_adaln_rotate_quant_token_rows_codes_fp6", "fpq_adaln_rotate_quant_token_rows_codes_f6"], SHAPE, [dict(codes=PTR + 4, cols=48)]),
    ("adaLN: pointers before the per-token bound on cols", ADALN_TOKEN, ARG, [dict(cols=2688, x=None)]),
    ("adaLN: cols > 4096 before nothing-to-do", ADALN, SHAPE, [dict(cols=4224, rows=0)]),
    ("adaLN per token: nothing-to-do before cols > 2560", ADALN_TOKEN, OK, [dict(cols=2688, rows=0)]),
    ("k-major image before nothing-to-do is not: rows first", ["fpq_quant_rows_codes_mx_km", "fpq_quant_rows_codes_fp6_km"], ARG, [dict(rows=-1, cols=200)]),
    ("GELU form: the shape before nothing-to-do and pointers", ["fpq_gelu_quant_rows_dual"], SHAPE, [dict(cols=100, rows=0), dict(cols=100, x=None)]),
    ("GELU form: the pair before the shape", ["fpq_gelu_quant_rows_dual"], TABLE, [dict(cols=100, neg_table=E2M1)]),
    ("KV step: sizes before the table, the table before the ranges", ["fpq_kv_cache_step"], TABLE, [dict(table_id=10, new_start=3), dict(table_id=E1M2_NEG, group=24)]),
    ("KV step: the ranges before the group, the group before nothing-to-do", ["fpq_kv_cache_step"], SHAPE, [dict(group=24, batch=0), dict(group=24, cache=None)]),
    ("KV step: the ranges before the group", ["fpq_kv_cache_step"], ARG, [dict(group=24, new_start=3)]),
    ("KV step with q / k norm: its own arguments before everything", ["fpq_kv_cache_step_qknorm"], ARG,
     [dict(head_dim=128, table_id=10), dict(q_head_scale=None, batch=0), dict(group=32, row_elems=192), dict(new_q=None, new_batch_pitch=2052)]),
    ("KV step with q / k norm: no new token, so q is not looked at", ["fpq_kv_cache_step_qknorm"], SHAPE, [dict(n_new=0, new_q=None, new_token_pitch=132)]),
    ("KV pack: sizes before nothing-to-do, nothing-to-do before pointers", ["fpq_kv_pack"], ARG, [dict(kv_bit=8, batch=0), dict(new_token_pitch=132, n_new=0)]),
    ("scan: sizes before k, k before the dtype, the dtype before nothing-to-do", ["fpq_quant_nearest", "fpq_quant_nearest_argmin"], SHAPE, [dict(k=0, dtype=7), dict(k=257, n=0)]),
    ("scan: n before k", ["fpq_quant_nearest", "fpq_quant_nearest_argmin"], ARG, [dict(n=-1, k=0)]),
    ("scan: the dtype before nothing-to-do", ["fpq_quant_nearest", "fpq_quant_nearest_argmin"], DTYPE, [dict(dtype=7, n=0)]),
    ("absmax: out before the dtype", ["fpq_absmax"], ARG, [dict(out=None, in_dtype=7)]),
    ("absmax: the dtype before anything is written", ["fpq_absmax"], DTYPE, [dict(in_dtype=7), dict(in_dtype=F64, n=0)]),
    ("per-tensor argmin: the dtype before the pointers", ["fpq_quant_tensor_argmin"], DTYPE, [dict(in_dtype=7, scale_out=None)]),
    ("segments: the shape before nothing-to-do", SEGMENTS, SHAPE, [dict(cols=64, n_segments=0)]),
    ("segments: the count before the table of segments", ["fpq_quant_rows_codes_segments", "fpq_dequant_rows_codes_segments"], SHAPE, [dict(n_segments=65536, segs=None)]),
    ("fp32 segments: the table of segments before the count (which the launch checks)", ["fpq_quant_rows_segments"], ARG, [dict(n_segments=65536, segs=None)]),
    ("multi: the table before the segments are read", ["fpq_quant_rows_multi"], TABLE, [dict(table_id=10, host_segments=dict(rows=(8, -1)))]),
    ("multi: the segments before nothing-to-do", ["fpq_quant_rows_multi"], ARG, [dict(cols=0, host_segments=dict(rows=(8, -1)))]),
]


SIZES = ("rows", "cols", "n", "n_segments", "max_rows", "batch", "n_new")


def _run(lib, rows):
    wrong = []
    for what, entries, code, calls in rows:
        assert len(set(entries)) == len(entries), what
        for entry in entries:
            for kw in calls:
                kw = dict(kw or {EMPTY: 1})
                if kw.pop(EMPTY, None):
                    kw.update(_nothing_to_do(entry))
                kw = {k: v for k, v in kw.items() if k in ENTRY[entry].split() + ["host_segments"]}   # (sizes the entry point does not have)
                assert kw, (what, entry)
                # no call may pass every check: it is refused, or a size of it is zero (host segments: all without rows)
                assert code < 0 or any(kw.get(n) == 0 for n in SIZES) or set(kw.get("host_segments", {}).get("rows", (1,))) == {0}, (what, entry, kw)
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
    from fpqvar_amd import _lib
    assert set(ALL) <= set(_lib._SIGS)
    data = [e for e in _lib._SIGS if e.startswith(("fpq_quant_", "fpq_dequant_", "fpq_kv_", "fpq_absmax", "fpq_rotate_", "fpq_adaln_", "fpq_gelu_quant_"))]
    assert sorted(data) == sorted(ALL), sorted(set(data) ^ set(ALL))
    for rows in (ONE_FAULT, TWO_FAULTS):
        seen = {e for _, entries, _, _ in rows for e in entries}
        assert seen == set(ALL), sorted(set(ALL) - seen)
    seen = {e for _, entries, _, _ in NOTHING_TO_DO for e in entries}
    assert seen == set(ALL) - set(NO_EMPTY_CALL), sorted(set(ALL) - seen)
    # no row can reach a launch: it is refused (a code below zero), or it has nothing to do (_run checks the overrides)
    assert all(code < 0 for _, _, code, _ in ONE_FAULT)
