"""Full-range FP6 (E2M3 / E3M2) operands with per-group(128) scales (include/fpq.h "GF6") without a GPU: the new C entry points'
declarations and argument checks in their stated order, the paper arithmetic of every pair's products, the model
tests/test_gpu_gf6.py holds the kernels to, the Python front's call path with the library replaced by a recorder
(tests/test_linear_call_path_host.py's pattern) and the routing of quantize_VAR / quantize_VAR_mixed(group_fp6=True)."""
import copy
import ctypes
import os
import re

import pytest
import torch

from tests import gemm_model as gm
from tests import gf6_model as fm
from tests.test_a6w4_host import CATCHES, _Var
from tests.test_linear_call_path_host import NAN_FLAG, fp16, named, rec  # noqa: F401  (rec: the recording-stub fixture)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OK, ERR_ARG, ERR_DTYPE, ERR_SHAPE, ERR_TABLE = 0, -1, -2, -3, -4
F16, F32 = 0, 1
E2M1, E1M2, E3M0, E2M3, E3M2, E1M2_NEG, E2M1_POS, INT_NEG, E2M3_POS, E2M1_NEG = range(10)   # enum fpq_table
TID = {"e2m1": E2M1, "e1m2": E1M2, "e3m0": E3M0, "e2m3": E2M3, "e3m2": E3M2}
PTR = 0x7000_0000_1000   # an address with every alignment the checks ask for; nothing reads it
IDS = [f"{a}-{w}" for a, w in fm.PAIRS]
NEW = {"fpq_gf6_quant_rows_codes": 9, "fpq_gemm_a6w4_gelu_dual_pair": 17, "fpq_gemm_w6_gelu_dual_pair": 18}
REFUSED = (("e3m0", "e3m2"), ("e3m2", "e3m0"), ("e3m2", "e3m2"))
ACCEPTED = tuple(p for p in fm.PAIRS if p not in REFUSED)


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as g
    g.build_hip()
    from fpqvar_amd import _lib
    return _lib.lib()


def _args(c):
    return c["a"], c["a_scales"], c["w"], c["w_scales"], c["bias"]


# ------------------------------------------------------------------------------------------------------------ the paper arithmetic
PAPER = {("e2m3", "e2m3"): (2.0 ** -6, 56.25, 19), ("e2m3", "e2m1"): (2.0 ** -4, 45.0, 17), ("e3m2", "e2m1"): (2.0 ** -5, 168.0, 20),
         ("e3m2", "e2m3"): (2.0 ** -7, 210.0, 22), ("e2m3", "e3m2"): (2.0 ** -7, 210.0, 22), ("e3m2", "e3m2"): (2.0 ** -8, 784.0, 25)}


@pytest.mark.parametrize("pair", fm.PAIRS, ids=IDS)
def test_product_range_of_every_pair(pair):
    """Every product of two levels is a multiple of `step` and at most `largest` (checked over all level pairs, in plain Python), so
    a 128-term dot is an integer multiple of step below 2^bits; only E3M2 x E3M2 (25 bits) does not fit fp32 on paper.  The levels
    are the reference's tables, and every level is a code of the 6-bit format its operand travels in."""
    from oracle import fpq_oracle as orc
    step, largest, bits = fm.product_range(*pair)
    la, lw = fm.LEVELS[pair[0]], fm.LEVELS[pair[1]]
    for x in la:
        for y in lw:
            assert (x * y / step) == int(x * y / step) and x * y <= largest
    assert any((x * y / step) % 2 == 1 for x in la for y in lw), "the step is the finest grid"
    assert la[-1] * lw[-1] == largest and 128 * largest / step < 2 ** bits and 128 * largest / step >= 2 ** (bits - 1)
    if pair in PAPER:
        assert (step, largest, bits) == PAPER[pair]
    assert fm.FITS_FP32[pair] == (pair != ("e3m2", "e3m2"))
    for t in pair:
        assert sorted(set(abs(float(v)) for v in orc.TABLES[t])) == list(fm.LEVELS[t])
        if t != "e2m1":
            codes = set(fm.am.code_values(fm.CODE_FORMAT[t]).abs().tolist())
            assert set(fm.LEVELS[t]) <= codes
    for name, (La, Lw) in fm.exact_dot_cases(*pair).items():
        assert torch.equal(fm.decode_levels(pair[0], fm.encode_levels(pair[0], La)), La + 0.0), name
        assert torch.equal(fm.decode_levels(pair[1], fm.encode_levels(pair[1], Lw)), Lw + 0.0), name
        d = La @ Lw.t()
        assert torch.equal(d, d.half().double()), name


# ------------------------------------------------------------------------------------------------------------ the model
@pytest.mark.parametrize("pair", (("e2m3", "e2m3"), ("e3m2", "e2m1"), ("e2m1", "e3m2"), ("e2m3", "e3m0")), ids=lambda p: "-".join(p))
def test_model_stays_inside_the_bound_and_covers_the_codes(pair):
    codes_seen = {pair[0]: set(), pair[1]: set()}
    for family in fm.FAMILIES:
        for T, O, K in ((17, 136, 384), (1, 8, 128)):
            c = fm.make_case(*pair, family, T, O, K)
            assert c["w_scales"].dtype == torch.float32 and c["a"].shape == (T, K // 128 * fm.SEG[pair[0]]) and c["w"].shape == (O, K // 128 * fm.SEG[pair[1]])
            r = fm.reference(*pair, *_args(c))
            out = fm.emulate(*pair, *_args(c))
            assert gm.ratio(out, r) <= 1.0 and not bool(gm.class_mismatch(out, r).any()), (pair, family, T, O, K)
            codes_seen[pair[0]] |= set(fm.decode_levels(pair[0], c["a"]).abs().unique().tolist())
            codes_seen[pair[1]] |= set(fm.decode_levels(pair[1], c["w"]).abs().unique().tolist())
    for t in pair:
        assert codes_seen[t] == set(fm.LEVELS[t]), (t, "every level of the table occurs in the families")
    c = fm.make_case(*pair, "max_codes", 5, 8, 256)
    assert float(fm.decode_levels(pair[0], c["a"]).abs().max()) == fm.LEVELS[pair[0]][-1]
    assert float(fm.decode_levels(pair[1], c["w"]).abs().max()) == fm.LEVELS[pair[1]][-1]


@pytest.mark.parametrize("mutation", list(CATCHES))
def test_every_mutation_is_caught_on_an_fp6_pair(mutation):
    """each of gm.MUTATIONS exceeds 1.5 x the bound on the family that catches it for the FP4 kernel, for one pair per kernel family"""
    family, (T, O, K) = CATCHES[mutation]
    for pair in (("e2m3", "e2m3"), ("e3m2", "e2m1")):
        c = fm.make_case(*pair, family, T, O, K)
        r = fm.reference(*pair, *_args(c))
        assert gm.ratio(fm.emulate(*pair, *_args(c)), r) <= 1.0
        rat = gm.ratio(fm.emulate(*pair, *_args(c), mutation), r)
        assert rat > 1.5, (pair, mutation, family, rat)
    assert set(CATCHES) == set(fm.MUTATIONS)


# ------------------------------------------------------------------------------------------------------------ the C ABI
def test_exports_declarations_and_signatures(lib):
    from fpqvar_amd import _lib
    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "fpq.h")).read(), flags=re.S)
    for name, n_args in NEW.items():
        assert hasattr(lib, name), name
        assert name in _lib._SIGS and len(_lib._SIGS[name][1]) == n_args, name
        decl = re.search(r"\bint\s+" + name + r"\s*\(([^)]*)\)", hdr)
        assert decl and len(decl.group(1).split(",")) == n_args, name
        assert getattr(lib, name).argtypes == _lib._SIGS[name][1]
    assert lib.fpq_version() == 136                                           # additions a caller looks up
    i, p, q = ctypes.c_int, ctypes.c_void_p, ctypes.c_int64
    assert _lib._SIGS["fpq_gf6_quant_rows_codes"][1] == _lib._SIGS["fpq_quant_rows_codes_g6"][1][:-1] + [i, p] == [p, p, p, q, q, i, i, i, p]
    # each _pair entry point: its twin's argument list, then neg_table, pos_table, kmajor in front of the stream
    for twin in ("fpq_gemm_a6w4_gelu_dual", "fpq_gemm_w6_gelu_dual"):
        assert _lib._SIGS[twin + "_pair"][1] == _lib._SIGS[twin][1][:-1] + [i, i, i, p]


def test_emitter_checks_in_their_order(lib):
    """table first, then negative sizes, dtype (fp32 rows have no k-major form), shape, empty input, NULL pointers / alignment"""
    def call(x=PTR, codes=PTR, scales=PTR, rows=8, cols=256, table=E2M3, dtype=F16, km=0):
        return lib.fpq_gf6_quant_rows_codes(x, codes, scales, rows, cols, table, dtype, km, None)
    for t in (E2M1, E1M2, E3M0, E1M2_NEG, INT_NEG, E2M3_POS, 99, -1):
        assert call(table=t) == ERR_TABLE and call(table=t, rows=-1) == ERR_TABLE and call(table=t, dtype=7) == ERR_TABLE
        assert call(table=t, cols=100) == ERR_TABLE and call(table=t, rows=0) == ERR_TABLE and call(table=t, x=None) == ERR_TABLE
    for t in (E2M3, E3M2):
        for km in (0, 1):
            assert call(table=t, km=km, rows=-1) == ERR_ARG and call(table=t, km=km, cols=-128) == ERR_ARG
            assert call(table=t, km=km, rows=-1, dtype=7) == ERR_ARG and call(table=t, km=km, cols=-128, rows=0) == ERR_ARG
            assert call(table=t, km=km, dtype=2) == ERR_DTYPE and call(table=t, km=km, dtype=7, cols=100) == ERR_DTYPE
            assert call(table=t, km=km, cols=100) == ERR_SHAPE and call(table=t, km=km, cols=100, rows=0) == ERR_SHAPE
            assert call(table=t, km=km, cols=100, x=None) == ERR_SHAPE
            assert call(table=t, km=km, rows=0, x=None) == OK and call(table=t, km=km, cols=0, codes=PTR + 1) == OK
            for name in ("x", "codes", "scales"):
                assert call(table=t, km=km, **{name: None}) == ERR_ARG, name
            assert call(table=t, km=km, x=PTR + 8) == ERR_ARG and call(table=t, km=km, codes=PTR + 8) == ERR_ARG
        assert call(table=t, dtype=F32, km=1) == ERR_DTYPE and call(table=t, dtype=F32, km=1, cols=100) == ERR_DTYPE
        assert call(table=t, dtype=F32, km=1, rows=0) == ERR_DTYPE
        assert call(table=t, km=1, rows=1 << 31) == ERR_SHAPE and call(table=t, km=1, rows=1 << 24, cols=1024) == ERR_SHAPE   # a 2 GiB image
        assert call(table=t, scales=PTR + 1) == ERR_ARG and call(table=t, dtype=F32, scales=PTR + 2) == ERR_ARG
        assert call(table=t, km=1, scales=PTR + 8) == ERR_ARG                   # the scale image: 16 bytes


@pytest.mark.parametrize("family", ("a6w4", "w6"))
def test_pair_entry_points_check_in_the_twins_order(lib, family):
    """the operand tables and the dual pair (FPQ_ERR_TABLE) in front of everything, then the twin's checks in the twin's order: both
    accepted pairs give the twin's answer to every call, in both layouts"""
    if family == "a6w4":
        def pair(neg=INT_NEG, pos=E2M3_POS, km=0, a=PTR, sa=PTR, a_table=E1M2, w=PTR, sw=PTR, w_dtype=F32, bias=None, out=PTR, h=None,
                 tokens=8, outs=128, k=128, flag=None):
            return lib.fpq_gemm_a6w4_gelu_dual_pair(a, sa, a_table, w, sw, w_dtype, bias, out, h, tokens, outs, k, flag, neg, pos, km, None)

        def twin(km=0, a=PTR, sa=PTR, a_table=E1M2, w=PTR, sw=PTR, w_dtype=F32, bias=None, out=PTR, h=None, tokens=8, outs=128, k=128, flag=None):
            fn = lib.fpq_gemm_a6w4_gelu_dual_km if km else lib.fpq_gemm_a6w4_gelu_dual
            return fn(a, sa, a_table, w, sw, w_dtype, bias, out, h, tokens, outs, k, flag, None)
        bad_operand = dict(a_table=E2M3)
    else:
        def pair(neg=INT_NEG, pos=E2M3_POS, km=0, a=PTR, sa=PTR, a_table=E1M2, w=PTR, sw=PTR, w_dtype=F32, w_table=E3M0, bias=None, out=PTR,
                 h=None, tokens=8, outs=128, k=128, flag=None):
            return lib.fpq_gemm_w6_gelu_dual_pair(a, sa, a_table, w, sw, w_dtype, w_table, bias, out, h, tokens, outs, k, flag, neg, pos, km, None)

        def twin(km=0, a=PTR, sa=PTR, a_table=E1M2, w=PTR, sw=PTR, w_dtype=F32, w_table=E3M0, bias=None, out=PTR, h=None, tokens=8, outs=128,
                 k=128, flag=None):
            fn = lib.fpq_gemm_w6_gelu_dual_km if km else lib.fpq_gemm_w6_gelu_dual
            return fn(a, sa, a_table, w, sw, w_dtype, w_table, bias, out, h, tokens, outs, k, flag, None)
        bad_operand = dict(w_table=E2M3)
    # the pair: beside the operand tables, in front of every other check
    for neg, pos in ((E1M2_NEG, E2M3_POS), (INT_NEG, E2M1_POS), (E2M1_NEG, E2M1_POS), (E2M3, E2M3), (E2M3_POS, INT_NEG), (-1, 0), (99, 99)):
        for km in (0, 1):
            assert pair(neg, pos, km) == ERR_TABLE and pair(neg, pos, km, tokens=-1) == ERR_TABLE and pair(neg, pos, km, w_dtype=9) == ERR_TABLE
            assert pair(neg, pos, km, k=100) == ERR_TABLE and pair(neg, pos, km, tokens=0) == ERR_TABLE and pair(neg, pos, km, a=None) == ERR_TABLE
    assert pair(**bad_operand) == ERR_TABLE and pair(tokens=-1, **bad_operand) == ERR_TABLE
    # everything else: the twin's answer.  EVERY call below is one a check refuses or an empty one (nothing may be launched: the
    # addresses are not memory); `layouts`: where that holds
    both, km_only = (0, 1), (1,)
    cases = [(dict(tokens=-1), both), (dict(outs=-128), both), (dict(k=-128, w_dtype=9), both), (dict(w_dtype=9), both),
             (dict(w_dtype=9, k=100), both), (dict(w_dtype=F16), km_only), (dict(k=100), both), (dict(k=128 * 65), both), (dict(outs=136), both),
             (dict(outs=100, tokens=0), both), (dict(tokens=1 << 31), both), (dict(tokens=1 << 28), km_only), (dict(outs=1 << 28), km_only),
             (dict(tokens=0), both), (dict(outs=0, a=None), both), (dict(tokens=0, out=PTR + 8), both), (dict(k=0), both), (dict(a=None), both),
             (dict(sa=None), both), (dict(w=None), both), (dict(sw=None), both), (dict(out=None), both), (dict(a=PTR + 8), both),
             (dict(w=PTR + 8), both), (dict(out=PTR + 8), both), (dict(h=PTR + 8), both), (dict(bias=PTR + 4), both), (dict(flag=PTR + 4), both),
             (dict(sa=PTR + 1), both), (dict(sw=PTR + 2), both), (dict(sa=PTR + 8), km_only), (dict(sw=PTR + 8), km_only), (bad_operand, both)]
    seen = set()
    for kw, layouts in cases:
        for km in layouts:
            want = twin(km, **kw)
            assert want in (ERR_ARG, ERR_DTYPE, ERR_SHAPE, ERR_TABLE) or (want == OK and (kw.get("tokens") == 0 or kw.get("outs") == 0)), (kw, km, want)
            seen.add(want)
            for neg, pos in ((E1M2_NEG, E2M1_POS), (INT_NEG, E2M3_POS)):
                assert pair(neg, pos, km, **kw) == want, (kw, km, neg, pos)
    assert seen == {OK, ERR_ARG, ERR_DTYPE, ERR_SHAPE, ERR_TABLE}


def test_the_gemms_take_full_range_codes_under_the_decode_tables_only(lib):
    """nothing changed in the GEMM entry points: FPQ_E2M3 / FPQ_E3M2 are still FPQ_ERR_TABLE there, before every other check - full
    FP6 codes travel under FPQ_E1M2 / FPQ_E3M0, the ids of the hardware decode"""
    for t in (E2M3, E3M2):
        assert lib.fpq_gemm_a6w4_mx(PTR, PTR, t, PTR, PTR, F32, None, PTR, 8, 128, 128, None, None) == ERR_TABLE
        assert lib.fpq_gemm_a6w4_gelu_dual(PTR, PTR, t, PTR, PTR, F32, None, PTR, None, 8, 128, 128, None, None) == ERR_TABLE
        assert lib.fpq_gemm_w6_mx(PTR, PTR, t, PTR, PTR, F32, E1M2, None, PTR, 8, 128, 128, None, None) == ERR_TABLE
        assert lib.fpq_gemm_w6_mx(PTR, PTR, E1M2, PTR, PTR, F32, t, None, PTR, 8, 128, 128, None, None) == ERR_TABLE
        assert lib.fpq_quant_rows_codes_g6(PTR, PTR, PTR, 8, 128, t, F16, None) == ERR_TABLE
        assert lib.fpq_a6w4_quant_rows_codes_km(PTR, PTR, PTR, 8, 128, t, F16, None) == ERR_TABLE


# ------------------------------------------------------------------------------------------------------------ the Python front
T, K, G = 8, 256, 2


def _operands(at, wt, km, tokens, outs):
    sa, sw_ = fm.SEG[at], fm.SEG[wt]
    if km:
        rows64 = (outs + 63) // 64 * 64
        return (torch.zeros(G, tokens, sa, dtype=torch.uint8), torch.zeros(G, (tokens + 3) // 4 * 4),
                torch.zeros(G, rows64, sw_, dtype=torch.uint8), torch.zeros(G, rows64))
    return (torch.zeros(tokens, G * sa, dtype=torch.uint8), torch.zeros(tokens, G, dtype=torch.float16),
            torch.zeros(outs, G * sw_, dtype=torch.uint8), torch.zeros(outs, G))


def _family(at, wt):
    """-> (C family, the ids between a_scales and the weight, the ids behind the weight scales' dtype)"""
    a_id, w_id = TID[fm.DECODE[at]], TID[fm.DECODE[wt]]
    return ("fpq_gemm_a6w4", (a_id,), ()) if wt == "e2m1" else ("fpq_gemm_w6", (a_id,), (w_id,))


@pytest.mark.parametrize("km", (False, True), ids=("rows", "kmajor"))
@pytest.mark.parametrize("table", fm.FULL)
def test_quantize_gf6_call(rec, table, km):
    """one entry point for both layouts: x, codes, scales, rows, cols, the FULL table's id, dtype, the layout flag, stream; fp32 rows
    as images go the two-step way (row-major + fpq_codes_to_kmajor + fpq_scales_to_kmajor)"""
    from fpqvar_amd import gemm
    x = fp16(3, 5, K)
    codes, scales = gemm.quantize_gf6(x, table, kmajor=km)
    assert codes.shape == ((G, 15, 96) if km else (15, G * 96)) and scales.shape == ((G, 16) if km else (15, G))
    assert scales.dtype == (torch.float32 if km else torch.float16)
    assert named(rec.take(), x=x, codes=codes, scales=scales) == [
        ("fpq_gf6_quant_rows_codes", ("x", "codes", "scales", 15, K, TID[table], F16, 1 if km else 0, 0))]
    x32 = torch.zeros(15, K)
    codes, scales = gemm.quantize_gf6(x32, table, kmajor=km)
    calls = [c[0] for c in rec.take()]
    assert calls == (["fpq_gf6_quant_rows_codes", "fpq_codes_to_kmajor", "fpq_scales_to_kmajor"] if km else ["fpq_gf6_quant_rows_codes"])
    for bad in ("e1m2", "e3m0", "e2m1", "fp_e1", "int_neg", None, 3):
        with pytest.raises(RuntimeError, match="'e2m3' and 'e3m2'"):
            gemm.quantize_gf6(x, bad)
    assert not rec.take()


@pytest.mark.parametrize("km", (False, True), ids=("rows", "kmajor"))
@pytest.mark.parametrize("pair", ACCEPTED, ids=["-".join(p) for p in ACCEPTED])
def test_linear_g6_calls(rec, pair, km):
    """plain, fc1 and split forms of every accepted pair: the entry point of the pair's kernel family and layout, the DECODE
    format's selector id behind a_scales (and behind the weight scales' dtype in the W6 family), every other argument as the
    family's own functions pass it"""
    from fpqvar_amd import gemm
    at, wt = pair
    fam, a_id, w_id = _family(at, wt)
    outs = 136
    a, sa, w, sw = _operands(at, wt, km, T, outs)
    bias, gate, res = fp16(outs), fp16(2, 1, outs), fp16(2, 4, outs)
    y = gemm.linear_g6(a, sa, at, w, sw, wt, bias, outs=outs)
    assert y.shape == (T, outs)
    what = fam + ("_mx_km" if km else "_mx")
    assert named(rec.take(), a=a, sa=sa, w=w, sw=sw, bias=bias, y=y) == [
        (what, ("a", "sa", *a_id, "w", "sw", F32, *w_id, "bias", "y", T, outs, K, None, 0))]
    y = gemm.linear_g6(a, sa, at, w, sw, wt, None, gate, res, outs=outs)
    assert named(rec.take(), a=a, sa=sa, w=w, sw=sw, gate=gate, res=res, y=y) == [
        (what, ("a", "sa", *a_id, "w", "sw", F32, *w_id, None, "y", T, outs, K, ("epilogue", "gate", "res", 4), 0))]
    # the fc1 form: one entry point, the pair's ids and the layout flag behind the NaN scratch
    outs = 128
    a, sa, w, sw = _operands(at, wt, km, T, outs)
    bias = fp16(outs)
    for names, ids in ((("int_neg", "e2m3_pos"), (INT_NEG, E2M3_POS)), ("fp6_int_neg_e2m3_pos", (INT_NEG, E2M3_POS)),
                       (("e1m2_neg", "e2m1_pos"), (E1M2_NEG, E2M1_POS)), ("fp_e1m2_neg_e2m1_pos", (E1M2_NEG, E2M1_POS))):
        q, h = gemm.linear_g6_gelu_dual(a, sa, at, w, sw, wt, bias, fc2_pair=names, return_gelu=True)
        assert q.shape == h.shape == (T, outs)
        assert named(rec.take(), a=a, sa=sa, w=w, sw=sw, bias=bias, q=q, h=h, flag=NAN_FLAG) == [
            (fam + "_gelu_dual_pair", ("a", "sa", *a_id, "w", "sw", F32, *w_id, "bias", "q", "h", T, outs, K, "flag", *ids, 1 if km else 0, 0))]
    q = gemm.linear_g6_gelu_dual(a, sa, at, w, sw, wt)
    assert named(rec.take(), a=a, sa=sa, w=w, sw=sw, q=q, flag=NAN_FLAG)[0][1][-5:] == ("flag", INT_NEG, E2M3_POS, 1 if km else 0, 0)
    with pytest.raises(RuntimeError, match="fc2_pair must be"):
        gemm.linear_g6_gelu_dual(a, sa, at, w, sw, wt, fc2_pair=("e2m1_neg", "e2m1_pos"))
    # the split form: the A6W4 family takes the layout as a flag, the W6 family has an entry point per layout
    c, seq = 128, 4
    a, sa, w, sw = _operands(at, wt, km, T, 3 * c)
    cache = fp16(2, 2, 9, 2, 64)
    hs = torch.ones(2)
    for norm in (False, True):
        q = gemm.linear_g6_qkv_to_cache(a, sa, at, w, sw, wt, None, cache, 3, seq, hs if norm else None)
        (name, args), = named(rec.take(), a=a, sa=sa, w=w, sw=sw, hs=hs, q=q)
        form = "_mx_split_qknorm" if norm else "_mx_split"
        tail = (("hs",) if norm else ()) + ((1 if km else 0,) if wt == "e2m1" else ())
        assert name == fam + form + ("_km" if km and wt != "e2m1" else "")
        assert args[:len(a_id) + 5 + len(w_id)] == ("a", "sa", *a_id, "w", "sw", F32, *w_id) and args[-len(tail) - 1:] == (*tail, 0), (name, args)
        assert args[len(a_id) + 5 + len(w_id):len(a_id) + 9 + len(w_id)] == (None, T, 3 * c, K)
    assert not rec.take()


def test_linear_g6_refusals(rec):
    """a pair without an FP6 side names its owner; the three BF6 x BF6 pairs name the measurement; mixed ranks, fp16 scales of a 6-bit
    weight and unknown names are refused - all before the library is reached.  The old names keep refusing the full tables."""
    from fpqvar_amd import gemm
    a, sa, w, sw = _operands("e2m3", "e2m3", False, T, 128)
    for at, wt, owner in (("e2m1", "e2m1", "linear_fp4"), ("e3m0", "fp_e2", "linear_a6w4"), ("fp_e1", "e3m0", "linear_w6"), ("e2m1", "e1m2", "linear_w6")):
        with pytest.raises(RuntimeError, match=f"belongs to {owner}$"):
            gemm.linear_g6(a, sa, at, w, sw, wt)
    assert set(gemm.GF6_REFUSED_PAIRS) == set(REFUSED)
    for at, wt in REFUSED:
        for fn, extra in ((gemm.linear_g6, ()), (gemm.linear_g6_gelu_dual, ()), (gemm.linear_g6_qkv_to_cache, (None, fp16(2, 1, 8, 1, 64), 0, 8))):
            with pytest.raises(RuntimeError, match="profiles/gf6_gemm_bound.txt"):
                fn(a, sa, at, w, sw, wt, *extra)
    with pytest.raises(RuntimeError, match="both operands must be"):
        gemm.linear_g6(a, sa, "e2m3", w.view(G, 128, 96), sw, "e2m3")
    with pytest.raises(RuntimeError, match="must be float32"):
        gemm.linear_g6(a, sa, "e2m3", w, sw.half(), "e2m3")
    with pytest.raises(RuntimeError, match="per-group formats here"):
        gemm.linear_g6(a, sa, "e4m3", w, sw, "e2m3")
    for bad in ("e2m3", "fp6_e2m3", "e3m2"):
        with pytest.raises(RuntimeError, match="'e1m2' and 'e3m0'"):
            gemm.quantize_g6(fp16(4, K), bad)
        with pytest.raises(RuntimeError, match="'e1m2' and 'e3m0'"):
            gemm.linear_a6w4(a, sa, bad, w, sw)
        with pytest.raises(RuntimeError, match="'e1m2' and 'e3m0'"):
            gemm.linear_w6(a, sa, "e1m2", w, sw, bad)
    with pytest.raises(ValueError, match="weight_fp_type must be"):
        gemm.FP4Linear.from_float(torch.nn.Linear(256, 64), weight_fp_type="fp6_e2m3")
    assert not rec.take()


def test_dequantize_gf6_decodes_every_code():
    from fpqvar_amd import gemm
    codes = gm.encode("fp6", torch.arange(128).view(1, 128) % 64)
    for table in ("e2m3", "e3m2", "fp6_e2m3", "e1m2", "e3m0"):
        got = gemm.dequantize_gf6(codes, torch.full((1, 1), 0.5), table).double()
        assert torch.equal(got, 0.5 * fm.decode_levels(gemm._GF6_TABLES[table], codes))
    with pytest.raises(RuntimeError):
        gemm.dequantize_gf6(codes, torch.ones(1, 1), "e2m1")


# ------------------------------------------------------------------------------------------------------------ the modules
def _fake_quantizers(monkeypatch):
    """Quantizing a weight needs the GPU: on the CPU every operand quantizer returns zero codes and unit scales of the right shapes"""
    from fpqvar_amd import gemm, quant_linear as ql

    def quantize(name, table, x, kmajor=False):
        rows, k = x.reshape(-1, x.shape[-1]).shape
        seg = gemm._FORMATS[table].seg
        if kmajor:
            return torch.zeros(k // 128, rows, seg, dtype=torch.uint8), torch.ones(k // 128, (rows + 3) // 4 * 4)
        return torch.zeros(rows, k // 128 * seg, dtype=torch.uint8), torch.ones(rows, k // 128, dtype=x.dtype)
    monkeypatch.setattr(gemm, "_quantize_any", quantize)
    monkeypatch.setattr(gemm, "to_kmajor", lambda c, bits, dealt=False: torch.zeros(c.shape[1] // (64 if bits == 4 else 96), (c.shape[0] + 63) // 64 * 64 if dealt else c.shape[0], 64 if bits == 4 else 96, dtype=torch.uint8))
    monkeypatch.setattr(gemm, "to_kmajor_scales", lambda s, weight_side=False: torch.ones(s.shape[1], (s.shape[0] + 63) // 64 * 64 if weight_side else (s.shape[0] + 3) // 4 * 4))
    monkeypatch.setattr(ql, "_quantize_weight", lambda w, *a, **k: w)
    return ql


def test_modules_hold_their_pair_and_call_linear_g6(rec, monkeypatch):
    from fpqvar_amd import gemm
    _fake_quantizers(monkeypatch)
    lin = torch.nn.Linear(256, 384)
    m = gemm.FP6GroupLinear.from_float(lin, "fp6_e3m2", "fp_e1")
    assert isinstance(m, gemm.FP4Linear) and (m.act_table, m.w_table) == ("e1m2", "e3m2") and not m.kmajor
    assert set(m.state_dict()) == {"w_codes", "w_scales", "bias"} and m.w_codes.shape == (384, 192) and m.w_scales.dtype == torch.float32
    a, sa = torch.zeros(6, 192, dtype=torch.uint8), torch.zeros(6, 2, dtype=torch.float16)
    y = m.forward_operands(a, sa)
    assert named(rec.take(), a=a, sa=sa, w=m.w_codes, sw=m.w_scales, bias=m.bias, y=y) == [
        ("fpq_gemm_w6_mx", ("a", "sa", E1M2, "w", "sw", F32, E3M0, "bias", "y", 6, 384, 256, None, 0))]
    mk = gemm.FP6GroupLinear.from_float(lin, "fp_e2", "fp6_e2m3", kmajor=True)
    assert mk.kmajor and mk.w_codes.shape == (2, 384, 64) and (mk.act_table, mk.w_table) == ("e2m3", "e2m1")
    f = gemm.FP6GroupLinearGeluDual.from_float(lin, "fp6_e2m3", "fp6_e2m3")
    assert f.fc2_pair == ("int_neg", "e2m3_pos") and isinstance(f, gemm.FP6GroupLinear)
    a, sa = torch.zeros(6, 192, dtype=torch.uint8), torch.zeros(6, 2, dtype=torch.float16)
    q = f.forward_operands(a, sa)
    assert named(rec.take(), a=a, sa=sa, w=f.w_codes, sw=f.w_scales, bias=f.bias, q=q, flag=NAN_FLAG) == [
        ("fpq_gemm_w6_gelu_dual_pair", ("a", "sa", E1M2, "w", "sw", F32, E1M2, "bias", "q", None, 6, 384, 256, "flag", INT_NEG, E2M3_POS, 0, 0))]
    f4 = gemm.FP6GroupLinearGeluDual.from_float(lin, "fp_e2", "fp6_e3m2", fc2_fp_type="fp_e1m2_neg_e2m1_pos")
    q = f4.forward_operands(a, sa)
    assert rec.take()[0][0] == "fpq_gemm_a6w4_gelu_dual_pair" and f4.fc2_pair == ("e1m2_neg", "e2m1_pos")
    for kw in (dict(weight_fp_type="fp_e2", act_fp_type="fp_e3"), dict(weight_fp_type="fp8", act_fp_type="fp6_e2m3")):
        with pytest.raises(ValueError):
            gemm.FP6GroupLinear.from_float(lin, **kw)
    with pytest.raises(ValueError, match="fc2_pair must be"):
        gemm.FP6GroupLinearGeluDual.from_float(lin, fc2_fp_type="fp4_afpq")


W6A6 = dict(weight_quant="per_group", act_quant="per_group", w_bit=6, a_bit=6, activation_fp_quant=True, weight_fp_quant=True,
            act_fp_type="fp6_e2m3", weight_fp_type="fp6_e2m3", fc2_fp_type="fp6_int_neg_e2m3_pos")


def _classes(model):
    return {n: type(m).__name__ for n, m in model.named_modules() if not list(m.children())}


def test_group_fp6_routes_the_model(monkeypatch):
    """quantize_VAR(group_fp6=True): fc1 / mat_qkv / proj become FP6GroupLinear, with fuse_ffn fc1 the fused module; fc2 and ada_lin
    stay; without the keyword the model is what it was, and the keyword outside its configuration is a ValueError"""
    from fpqvar_amd import gemm
    ql = _fake_quantizers(monkeypatch)
    base = _Var(256, 3)
    for b in base.blocks:
        b.ffn.act = torch.nn.GELU(approximate="tanh")
    before = ql.quantize_VAR(copy.deepcopy(base), **W6A6)
    assert _classes(ql.quantize_VAR(copy.deepcopy(base), group_fp6=False, **W6A6)) == _classes(before)
    assert not [m for m in before.modules() if isinstance(m, gemm.FP4Linear)]
    for km in (False, True):
        real = ql.quantize_VAR(copy.deepcopy(base), group_fp6=True, kmajor_operands=km, **W6A6)
        for b in real.blocks:
            assert type(b.ffn.fc1) is type(b.attn.mat_qkv) is type(b.attn.proj) is gemm.FP6GroupLinear
            assert b.ffn.fc1.kmajor == km and (b.ffn.fc1.act_table, b.ffn.fc1.w_table) == ("e2m3", "e2m3")
            assert type(b.ffn.fc2) is ql.QuantizedLinear_fc2 and isinstance(b.ada_lin[1], torch.nn.Linear) and isinstance(b.ffn.act, torch.nn.GELU)
    fused = ql.quantize_VAR(copy.deepcopy(base), group_fp6=True, fuse_ffn=True, **W6A6)
    for b in fused.blocks:
        assert type(b.ffn.fc1) is gemm.FP6GroupLinearGeluDual and b.ffn.fc1.fc2_pair == ("int_neg", "e2m3_pos")
        assert isinstance(b.ffn.act, torch.nn.Identity) and b.ffn.fc2.act_quant_name == "in fc1's epilogue"
        assert type(b.attn.mat_qkv) is gemm.FP6GroupLinear
    w6a4 = dict(W6A6, a_bit=4, act_fp_type="fp_e3", fc2_fp_type="fp_e1m2_neg_e2m1_pos")
    for b in ql.quantize_VAR(copy.deepcopy(base), group_fp6=True, fuse_ffn=True, **w6a4).blocks:
        assert type(b.ffn.fc1) is gemm.FP6GroupLinearGeluDual and b.ffn.fc1.fc2_pair == ("e1m2_neg", "e2m1_pos")
        assert (b.ffn.fc1.act_table, b.ffn.fc1.w_table) == ("e3m0", "e2m3") and isinstance(b.ffn.act, torch.nn.Identity)
    unfused = ql.quantize_VAR(copy.deepcopy(base), fuse_ffn=True, **W6A6)           # without the keyword: the one-pass route, as today
    assert all(type(b.ffn.act) is ql.GeluThenFc2Quant and type(b.ffn.fc1) is ql.QuantizedLinear for b in unfused.blocks)
    # the refused pair stays fake-quantized
    e3 = dict(W6A6, act_fp_type="fp6_e3m2", weight_fp_type="fp6_e3m2")
    assert _classes(ql.quantize_VAR(copy.deepcopy(base), group_fp6=True, **e3)) == _classes(ql.quantize_VAR(copy.deepcopy(base), **e3))
    # W4A6: an E2M1 weight against an FP6 activation
    w4a6 = dict(W6A6, w_bit=4, weight_fp_type="fp_e2")
    m = ql.quantize_VAR(copy.deepcopy(base), group_fp6=True, **w4a6)
    assert (m.blocks[0].attn.proj.act_table, m.blocks[0].attn.proj.w_table) == ("e2m3", "e2m1")
    for bad in (dict(W6A6, act_quant="per_token"), dict(W6A6, w_bit=4, a_bit=4), dict(W6A6, weight_fp_quant=False)):
        with pytest.raises(ValueError, match="group_fp6 needs"):
            ql.quantize_VAR(copy.deepcopy(base), group_fp6=True, **bad)


def test_group_fp6_routes_the_mixed_model(monkeypatch):
    from fpqvar_amd import gemm
    ql = _fake_quantizers(monkeypatch)
    base = _Var(256, 3)
    for b in base.blocks:
        b.ffn.act = torch.nn.GELU(approximate="tanh")
    kw = {k: W6A6[k] for k in ("weight_quant", "act_quant", "w_bit", "a_bit", "activation_fp_quant", "weight_fp_quant")}
    table = {(0, "fc1"): ("fp6_e2m3", "fp6_e3m2"), (0, "mat_qkv"): ("fp6_e3m2", "fp_e2"), (0, "proj"): ("fp_e3", "fp6_e2m3"),
             (1, "fc1"): ("fp6_e3m2", "fp6_e3m2"), (1, "mat_qkv"): ("fp_e1", "fp_e3"), (1, "proj"): ("fp6_e2m3", "fp6_e2m3")}

    def fmt(b, layer):
        return table.get((b, layer), ("fp6_int_neg_e2m3_pos", "fp6_e2m3") if layer == "fc2" else ("fp6_e2m3", "fp6_e2m3"))
    before = ql.quantize_VAR_mixed(copy.deepcopy(base), fmt, **kw)
    assert not [m for m in before.modules() if isinstance(m, gemm.FP4Linear)]
    real = ql.quantize_VAR_mixed(copy.deepcopy(base), fmt, group_fp6=True, kmajor_operands=False, **kw)
    got = {n: (m.act_table, m.w_table) for n, m in real.named_modules() if isinstance(m, gemm.FP6GroupLinear)}
    assert got == {"blocks.0.ffn.fc1": ("e2m3", "e3m2"), "blocks.0.attn.mat_qkv": ("e3m2", "e2m1"), "blocks.0.attn.proj": ("e3m0", "e2m3"),
                   "blocks.1.attn.proj": ("e2m3", "e2m3"), "blocks.2.ffn.fc1": ("e2m3", "e2m3"), "blocks.2.attn.mat_qkv": ("e2m3", "e2m3"),
                   "blocks.2.attn.proj": ("e2m3", "e2m3")}, got
    assert type(real.blocks[1].ffn.fc1) is type(real.blocks[1].attn.mat_qkv) is ql.QuantizedLinear     # the refused pair; a pure FP4 pair
    fused = ql.quantize_VAR_mixed(copy.deepcopy(base), fmt, group_fp6=True, fuse_ffn=True, **kw)
    assert type(fused.blocks[0].ffn.fc1) is type(fused.blocks[2].ffn.fc1) is gemm.FP6GroupLinearGeluDual
    assert type(fused.blocks[1].ffn.fc1) is ql.QuantizedLinear and type(fused.blocks[1].ffn.act) is ql.GeluThenFc2Quant
    with pytest.raises(ValueError, match="group_fp6 needs"):
        ql.quantize_VAR_mixed(copy.deepcopy(base), fmt, group_fp6=True, **dict(kw, w_bit=8))
