"""The A6W4 path (E1M2 / E3M0 activations as 6-bit codes against FP4 weights) without a GPU: the premises of its exactness
argument, the model tests/test_gpu_a6w4.py holds the kernel to, the C entry points' argument checks, the ISA properties of the
eight instantiations of gemm_a6w4_kernel read from the built library, and the routing of quantize_VAR_mixed*(real_fp4=...)."""
import ctypes
import os
import re
import subprocess

import pytest
import torch

from tests import a6w4_model as am
from tests import gemm_model as gm
from tests.test_no_spill import LIB, _code_objects, _tool, kernel_metadata

OK, ERR_ARG, ERR_DTYPE, ERR_SHAPE, ERR_TABLE = 0, -1, -2, -3, -4
F16, F32 = 0, 1
E2M1, E1M2, E3M0, E2M3, E3M2 = 0, 1, 2, 3, 4   # enum fpq_table
PTR = 0x7000_0000_1000   # an address with every alignment the checks ask for; nothing reads it

SHAPES = ((33, 136, 384), (17, 128, 1920), (5, 8, 2304), (65, 120, 256))
# mutation -> the family and shape where the mistake must exceed 1.5 x the bound (tests/test_gemm_model_host.py's choices for the
# FP4 kernel, whose steps this kernel shares)
CATCHES = {
    "rtz_out": ("gauss", (65, 392, 256)),
    "bias_after_round": ("bias_cancel", (33, 136, 384)),
    "scale_fp16": ("group_range", (33, 136, 384)),
    "tail_group_scale": ("one_group", (17, 128, 1920)),
    "drop_last_k": ("one_group", (17, 128, 1920)),
    "sat_out": ("overflow", (33, 136, 384)),
    "w_scale_fp16": ("group_range", (33, 136, 384)),
}


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as g
    g.build_hip()
    from fpqvar_amd import _lib
    return _lib.lib()


def _args(c):
    return c["a"], c["a_scales"], c["w"], c["w_scales"], c["bias"]


# ------------------------------------------------------------------------------------------------------------ the formats
@pytest.mark.parametrize("table", ("e1m2", "e3m0"))
def test_every_level_is_a_code_of_its_6bit_format(table):
    """Every E1M2 level is an E2M3 code value and every E3M0 level an E3M2 code value; the levels are the reference's tables."""
    from oracle import fpq_oracle as orc
    vals = am.code_values(am.A_CODE_FORMAT[table])
    assert sorted(set(orc.TABLES[table].abs().tolist())) == list(am.A_LEVELS[table])
    codes = am.level_codes(table)
    assert len(set(codes.tolist())) == 8 and int(codes[0]) == 0
    for lv, c in zip(am.A_LEVELS[table], codes.tolist()):
        assert float(vals[c]) == lv and float(vals[c + 32]) == -lv
    # the code tables round-trip: levels -> dense 6-bit rows -> levels
    g = torch.Generator().manual_seed(1)
    lv = torch.tensor(am.A_LEVELS[table], dtype=torch.float64)
    L = lv[torch.randint(0, 8, (7, 256), generator=g)] * torch.where(torch.rand(7, 256, generator=g) < 0.5, 1.0, -1.0)
    rows = am.encode_a(table, L)
    assert rows.shape == (7, 192) and rows.dtype == torch.uint8
    assert torch.equal(am.decode_a(table, rows), L + 0.0)            # (-0 is stored as code 0)


def test_code_values_agree_with_the_fp6_decoders():
    """a6w4_model.code_values == gm's E2M3 table, and == gemm.dequantize_fp6 for both formats on all 64 codes"""
    from fpqvar_amd import gemm
    assert torch.equal(am.code_values("e2m3"), gm._code_values("fp6"))
    idx = torch.arange(64).view(1, 64)
    rows = gm.encode("fp6", idx)
    for fmt in ("e2m3", "e3m2"):
        got = gemm.dequantize_fp6(rows, torch.ones(1), fmt).double().view(-1)
        assert torch.equal(got, am.code_values(fmt) + 0.0), fmt


@pytest.mark.parametrize("table", ("e1m2", "e3m0"))
def test_products_are_multiples_of_an_eighth(table):
    """The premise of the exactness argument, exhaustively over the 15 x 15 signed level pairs: every product is a multiple of 1/8
    within the stated maximum, so a 128-term dot is a multiple of 1/8 of at most 128 * max: 17 significant bits at most."""
    sl_a = [s * v for v in am.A_LEVELS[table] for s in (1, -1) if not (v == 0 and s < 0)]
    sl_w = [s * v for v in gm.E2M1 for s in (1, -1) if not (v == 0 and s < 0)]
    assert len(sl_a) == 15 and len(sl_w) == 15
    worst = 0.0
    for x in sl_a:
        for y in sl_w:
            p = x * y
            assert (p * 8) == int(p * 8), (x, y)
            worst = max(worst, abs(p))
    assert worst == am.MAX_PRODUCT[table] == am.A_LEVELS[table][-1] * 6.0
    assert 128 * worst * 8 < 2 ** 17 and 128 * am.MAX_PRODUCT["e3m0"] == 12288
    for name, (La, Lw) in am.exact_dot_cases(table).items():         # (the GPU test's exact-dot inputs are what they claim)
        d = La @ Lw.t()
        assert bool((d == d.half().double()).all()) and bool((d.float().double() == d).all()), name


# ------------------------------------------------------------------------------------------------------------ the model
@pytest.mark.parametrize("table", ("e1m2", "e3m0"))
def test_emulated_kernel_stays_inside_the_bound(table):
    for family in am.FAMILIES:
        for T, O, K in SHAPES:
            c = am.make_case(table, family, T, O, K)
            assert gm.ratio(am.emulate(table, *_args(c)), am.reference(table, *_args(c))) <= 1.0, (table, family, T, O, K)


@pytest.mark.parametrize("table", ("e1m2", "e3m0"))
def test_emulated_kernel_over_the_host_shape_sweep(table):
    t = tuple(n for n in gm.T_SWEEP if n <= 65)
    o = tuple(n for n in gm.O_SWEEP if n <= 392)
    k = tuple(n for n in gm.K_SWEEP if n <= 2304)
    for family, T, O, K in gm.shape_sweep(t, o, k, am.FAMILIES):
        c = am.make_case(table, family, T, O, K)
        assert gm.ratio(am.emulate(table, *_args(c)), am.reference(table, *_args(c))) <= 1.0, (table, family, T, O, K)


@pytest.mark.parametrize("table", ("e1m2", "e3m0"))
@pytest.mark.parametrize("mutation", list(CATCHES))
def test_every_mutation_breaks_the_bound(table, mutation):
    family, (T, O, K) = CATCHES[mutation]
    c = am.make_case(table, family, T, O, K)
    r = am.reference(table, *_args(c))
    assert gm.ratio(am.emulate(table, *_args(c)), r) <= 1.0
    rat = gm.ratio(am.emulate(table, *_args(c), mutation), r)
    print(f"{table} {mutation} {family}: {rat:.3g}")
    assert rat > 1.5, (table, mutation, family, rat)


def test_every_mutation_has_a_catch():
    assert set(CATCHES) == set(am.MUTATIONS) == set(gm.MUTATIONS)


@pytest.mark.parametrize("table", ("e1m2", "e3m0"))
def test_families_keep_their_meaning_on_the_table(table):
    c = am.make_case(table, "zero", 9, 136, 384)
    out = am.emulate(table, *_args(c))
    want = c["bias"].view(1, 136).expand(9, 136) if c["bias"] is not None else torch.zeros(9, 136, dtype=torch.float16)
    assert torch.equal(out.view(torch.int16), want.contiguous().view(torch.int16))
    c = am.make_case(table, "overflow", 65, 392, 384)
    ref = am.reference(table, *_args(c)).out.abs()
    assert bool((ref < 65504).any()) and bool((ref > 65520).any())
    c = am.make_case(table, "non_finite", 40, 136, 384)
    r = am.reference(table, *_args(c))
    assert bool(torch.isnan(r.out).any()) and bool(torch.isinf(r.out).any())
    assert not bool(gm.class_mismatch(am.emulate(table, *_args(c)), r).any())
    c = am.make_case(table, "max_codes", 5, 8, 256)
    assert float(am.decode_a(table, c["a"]).abs().max()) == am.A_LEVELS[table][-1]
    assert gm.ratio(am.emulate(table, *_args(am.make_case(table, "gauss", 65, 392, 1920))),
                    am.reference(table, *_args(am.make_case(table, "gauss", 65, 392, 1920)))) >= 0.9      # the bound is not vacuous


# ------------------------------------------------------------------------------------------------------------ the C ABI
def test_version_and_exports(lib):
    assert lib.fpq_version() >= 131
    assert hasattr(lib, "fpq_quant_rows_codes_g6") and hasattr(lib, "fpq_gemm_a6w4_mx")


def test_emitter_checks_come_before_any_launch(lib):
    def call(x=PTR, codes=PTR, scales=PTR, rows=4, cols=256, table=E3M0, dtype=F16):
        return lib.fpq_quant_rows_codes_g6(x, codes, scales, rows, cols, table, dtype, None)
    assert call(rows=0) == OK and call(cols=0) == OK and call(rows=0, table=E1M2, dtype=F32) == OK
    for t in (E2M1, E2M3, E3M2, 5, 6, 99, -1):
        assert call(table=t) == ERR_TABLE, t
    assert call(cols=192) == ERR_SHAPE and call(cols=100) == ERR_SHAPE
    assert call(dtype=2) == ERR_DTYPE and call(dtype=7) == ERR_DTYPE
    assert call(rows=-1) == ERR_ARG and call(cols=-128) == ERR_ARG
    assert call(x=None) == ERR_ARG and call(codes=None) == ERR_ARG and call(scales=None) == ERR_ARG
    assert call(x=PTR + 8) == ERR_ARG and call(codes=PTR + 4) == ERR_ARG
    assert call(scales=PTR + 1) == ERR_ARG and call(scales=PTR + 2, dtype=F32) == ERR_ARG
    assert call(scales=PTR + 2, rows=0) == OK


def test_gemm_checks_come_before_any_launch(lib):
    from fpqvar_amd._lib import GemmEpilogue

    def call(a=PTR, sa=PTR, table=E3M0, w=PTR, sw=PTR, w_dtype=F32, bias=None, out=PTR, tokens=8, outs=128, k=128, ep=None):
        return lib.fpq_gemm_a6w4_mx(a, sa, table, w, sw, w_dtype, bias, out, tokens, outs, k, ep, None)
    assert call(tokens=0) == OK and call(outs=0) == OK and call(tokens=0, table=E1M2, w_dtype=F16) == OK
    for t in (E2M1, E2M3, E3M2, 5, 99, -1):
        assert call(table=t) == ERR_TABLE, t
        assert call(table=t, tokens=0) == ERR_TABLE, t
    assert call(k=96) == ERR_SHAPE and call(k=128 * 65) == ERR_SHAPE and call(outs=100) == ERR_SHAPE
    assert call(tokens=1 << 31) == ERR_SHAPE
    assert call(w_dtype=2) == ERR_DTYPE and call(w_dtype=9) == ERR_DTYPE
    assert call(tokens=-4) == ERR_ARG and call(outs=-8) == ERR_ARG and call(k=-128) == ERR_ARG and call(k=0) == ERR_ARG
    for name in ("a", "sa", "w", "sw", "out"):
        assert call(**{name: None}) == ERR_ARG, name
    assert call(a=PTR + 8) == ERR_ARG and call(w=PTR + 8) == ERR_ARG and call(out=PTR + 8) == ERR_ARG     # 16-byte aligned
    assert call(bias=PTR + 4) == ERR_ARG and call(bias=PTR + 8, tokens=0) == OK                          # the bias: 8 bytes
    assert call(ep=ctypes.byref(GemmEpilogue(PTR + 8, None, 4))) == ERR_ARG                              # gate / residual: 16 bytes
    assert call(ep=ctypes.byref(GemmEpilogue(None, PTR + 2, 4))) == ERR_ARG
    assert call(ep=ctypes.byref(GemmEpilogue(PTR, None, 0))) == ERR_ARG                                  # rows_per_gate >= 1
    assert call(ep=ctypes.byref(GemmEpilogue(PTR, PTR, 4)), tokens=0) == OK


def test_python_wrappers_refuse_before_the_library(lib):
    from fpqvar_amd import gemm
    x = torch.zeros(4, 256, dtype=torch.float16)
    with pytest.raises(RuntimeError, match="GPU"):
        gemm.quantize_g6(x, "e3m0")
    with pytest.raises(RuntimeError, match="GPU"):
        gemm.linear_a6w4(torch.zeros(4, 192, dtype=torch.uint8), torch.zeros(4, 2, dtype=torch.float16), "e3m0",
                         torch.zeros(8, 128, dtype=torch.uint8), torch.zeros(8, 2))
    lin = torch.nn.Linear(256, 64)
    with pytest.raises(ValueError, match="no k-major form"):
        gemm.FP4Linear.from_float(lin, kmajor=True, act_fp_type="fp_e3")
    with pytest.raises(RuntimeError, match="'e1m2' and 'e3m0'"):
        gemm.FP4Linear.from_float(lin, act_fp_type="fp6_e2m3")
    with pytest.raises(RuntimeError, match="'e1m2' and 'e3m0'"):
        gemm.dequantize_g6(torch.zeros(1, 96, dtype=torch.uint8), torch.ones(1, 1), "e2m1")
    # the torch decoder on the CPU: level(code) * scale of the code's group
    L = torch.tensor(am.A_LEVELS["e3m0"], dtype=torch.float64)[torch.arange(256) % 8].view(1, 256) * torch.where(torch.arange(256) % 3 == 0, -1.0, 1.0)
    got = gemm.dequantize_g6(am.encode_a("e3m0", L), torch.tensor([[0.5, 3.0]], dtype=torch.float16), "e3m0")
    assert torch.equal(got.double(), (L.view(1, 2, 128) * torch.tensor([0.5, 3.0], dtype=torch.float64).view(1, 2, 1)).view(1, 256) + 0.0)


# ------------------------------------------------------------------------------------------------------------ the kernels
def _a6w4_kernels(recs):
    return [(n, r) for n, r in recs if "gemm_a6w4_kernel" in n]


def _template_args(name):
    """(weight-scale type, MT, FA) from the mangled name gemm_a6w4_kernel<Tsw, MT, 4, FA>"""
    m = re.search(r"gemm_a6w4_kernelI(DF16_|f)Li(\d)ELi4ELi(\d)E", name)
    assert m, name
    return m.group(1), int(m.group(2)), int(m.group(3))


@pytest.mark.skipif(not os.path.exists(LIB), reason="libfpq_hip.so not built")
def test_the_eight_instantiations_do_not_spill(tmp_path):
    """{E2M3, E3M2 selector} x {fp16, fp32 weight scales} x {64, 128 rows}: no scratch, no spill, at most 256 registers per lane
    (two workgroups of four wavefronts per CU), no static LDS (the image is the launch's dynamic LDS)."""
    ks = _a6w4_kernels(kernel_metadata(tmp_path))
    assert len(ks) == 8, [n for n, _ in ks]
    assert {_template_args(n) for n, _ in ks} == {(t, mt, fa) for t in ("DF16_", "f") for mt in (2, 4) for fa in (2, 3)}
    for n, r in ks:
        assert int(r.get("vgpr_spill_count", 0)) == 0 and int(r.get("sgpr_spill_count", 0)) == 0, (n, r)
        assert int(r.get("private_segment_fixed_size", 0)) == 0, (n, r.get("private_segment_fixed_size"))
        assert int(r["vgpr_count"]) + int(r.get("agpr_count", 0)) <= 256, (n, r["vgpr_count"])
        assert int(r.get("group_segment_fixed_size", 0)) == 0, n
    emit = [(n, r) for n, r in kernel_metadata(tmp_path) if "group6_emit" in n]
    assert len(emit) == 3, [n for n, _ in emit]                      # the fp16 form, the generic one for E1M2 and for E3M0
    for n, r in emit:
        assert int(r.get("vgpr_spill_count", 0)) == 0 and int(r.get("private_segment_fixed_size", 0)) == 0, (n, r)


@pytest.mark.skipif(not os.path.exists(LIB), reason="libfpq_hip.so not built")
def test_fragment_reads_and_selectors(tmp_path):
    """Per K step: three ds_read_b64 per A fragment (MT of them), one ds_read_b128 per W fragment (4) beside the scale tiles'
    (1 + MT), never a paired read; every MFMA decodes A by the instantiation's selector and B as FP4; no vector-memory wait
    among the MFMAs (the LDS-DMA pieces are waited for once, in front of the barrier)."""
    checked = 0
    for elf in _code_objects(tmp_path):
        txt = subprocess.run([_tool("llvm-objdump"), "-d", "--no-show-raw-insn", elf], capture_output=True, text=True, check=True).stdout
        for block in re.split(r"\n(?=[0-9a-fA-F]+ <)", txt):
            head = block.split("\n", 1)[0]
            if "gemm_a6w4_kernel" not in head:
                continue
            lines = [" ".join(l.split()) for l in block.splitlines()[1:] if l.strip()]
            lines = [l.split(" //")[0] for l in lines]
            ops = [l.split()[0] for l in lines]
            _, mt, fa = _template_args(head)
            assert ops.count("ds_read_b64") == 3 * mt, (head, ops.count("ds_read_b64"))
            assert ops.count("ds_read_b128") == 4 + 1 + mt, (head, ops.count("ds_read_b128"))
            assert not [o for o in ops if o.startswith("ds_read2")], head
            assert not [o for o in ops if o.startswith("scratch_")], head
            assert not [o for o in ops if o.startswith("v_pk_") and o.endswith("_f32")], head      # FPQ_NOPK: scalar fp32 VALU
            mf = [i for i, l in enumerate(lines) if l.startswith("v_mfma")]
            assert len(mf) == 4 * mt, (head, len(mf))
            for i in mf:
                assert "v_mfma_f32_16x16x128_f8f6f4" in lines[i] and f"cbsz:{fa}" in lines[i] and "blgp:4" in lines[i], (head, lines[i])
            between = [l for l in lines[mf[0]:mf[-1] + 1] if l.startswith("s_waitcnt") and "vmcnt" in l]
            assert not between, (head, between)
            pieces = (3 * mt + 8 + 3) // 4                                   # LDS-DMA pieces per wavefront and stage (the last round may be short)
            assert ops.count("global_load_lds_dwordx4") == 2 * pieces, (head, ops.count("global_load_lds_dwordx4"))
            checked += 1
    assert checked == 8, checked


# ------------------------------------------------------------------------------------------------------------ the wiring
class _Ffn(torch.nn.Module):
    def __init__(self, c):
        super().__init__()
        self.fc1, self.act, self.fc2 = torch.nn.Linear(c, 4 * c), torch.nn.GELU(approximate="tanh"), torch.nn.Linear(4 * c, c)


class _Attn(torch.nn.Module):
    def __init__(self, c):
        super().__init__()
        self.mat_qkv, self.proj = torch.nn.Linear(c, 3 * c, bias=False), torch.nn.Linear(c, c)


class _Block(torch.nn.Module):
    def __init__(self, c):
        super().__init__()
        self.attn, self.ffn = _Attn(c), _Ffn(c)
        self.ada_lin = torch.nn.Sequential(torch.nn.SiLU(), torch.nn.Linear(c, 6 * c))


class _Var(torch.nn.Module):
    def __init__(self, c, depth):
        super().__init__()
        self.blocks = torch.nn.ModuleList(_Block(c) for _ in range(depth))


W4A4 = dict(weight_quant="per_group", act_quant="per_group", w_bit=4, a_bit=4, activation_fp_quant=True, weight_fp_quant=True,
            act_fp_type="fp_e2", weight_fp_type="fp_e2", fc2_fp_type="fp_e1m2_neg_e2m1_pos")


class _Marker(torch.nn.Module):
    def __init__(self, kmajor, act):
        super().__init__()
        self.kmajor_arg, self.act = kmajor, act


@pytest.fixture
def cpu_construction(monkeypatch):
    """Quantizing a weight needs the GPU: on the CPU the weight quantizer is an identity and FP4Linear.from_float records its
    arguments, so the walk - which layer becomes what - runs as it is."""
    from fpqvar_amd import gemm, quant_linear as ql
    monkeypatch.setattr(ql, "_quantize_weight", lambda w, *a, **k: w)
    monkeypatch.setattr(gemm.FP4Linear, "from_float", classmethod(lambda cls, lin, kmajor=False, act_fp_type="fp_e2": _Marker(kmajor, act_fp_type)))
    return ql


def _classes(model):
    return {n: type(m).__name__ for n, m in model.named_modules() if not list(m.children()) or isinstance(m, _Marker)}


@pytest.mark.parametrize("fn", ("quantize_VAR_mixed_fp4_datatype", "quantize_VAR_use_different_datatype"))
def test_real_fp4_routes_the_format_table(cpu_construction, fn):
    """d30-shaped: 30 blocks.  Without the keyword every layer is the QuantizedLinear it was; with it every E2M1-weight fc1 /
    mat_qkv / proj is an FP4Linear of its activation format - every E3M0 fc1 (15 blocks) and mat_qkv (27 or 28) among them, row-major -
    and fc2 / ada_lin[1] stay."""
    ql = cpu_construction
    torch.manual_seed(0)
    plain = getattr(ql, fn)(_Var(128, 30), **W4A4)
    names = _classes(plain)
    assert set(names.values()) == {"QuantizedLinear", "QuantizedLinear_fc2", "SiLU", "GELU"}
    assert sum(v == "QuantizedLinear_fc2" for v in names.values()) == 30 and sum(v == "QuantizedLinear" for v in names.values()) == 120
    off = getattr(ql, fn)(_Var(128, 30), real_fp4=False, **W4A4)
    assert _classes(off) == names
    real = getattr(ql, fn)(_Var(128, 30), real_fp4=True, **W4A4)
    qkv_e2 = {0, 24, 25} if fn == "quantize_VAR_mixed_fp4_datatype" else {24, 25}
    n_e3 = 0
    for b, blk in enumerate(real.blocks):
        want_fc1 = "fp_e2" if 6 <= b <= 20 else "fp_e3"
        want_qkv = "fp_e2" if b in qkv_e2 else "fp_e3"
        for m, want in ((blk.ffn.fc1, want_fc1), (blk.attn.mat_qkv, want_qkv), (blk.attn.proj, "fp_e2")):
            assert isinstance(m, _Marker) and m.act == want and m.kmajor_arg == (want == "fp_e2"), (b, m.act, want)
            n_e3 += want == "fp_e3"
        assert type(blk.ffn.fc2) is ql.QuantizedLinear_fc2 and type(blk.ada_lin[1]) is ql.QuantizedLinear
    assert n_e3 == 15 + (30 - len(qkv_e2))
    rowmajor = getattr(ql, fn)(_Var(128, 2), real_fp4=True, kmajor_operands=False, **W4A4)
    assert not any(m.kmajor_arg for m in rowmajor.modules() if isinstance(m, _Marker))


def test_real_fp4_leaves_what_does_not_fit(cpu_construction):
    ql = cpu_construction

    def fmt(b, layer):                      # an E1M2 activation, an E3M0 weight, a dual-format fc2, an E1M2 weight
        return {"fc1": ("fp_e1", "fp_e2"), "mat_qkv": ("fp_e2", "fp_e3"), "fc2": ("fp_e1m2_neg_e2m1_pos", "fp_e2"), "proj": ("fp_e3", "fp_e1")}[layer]
    kw = {k: v for k, v in W4A4.items() if k not in ("act_fp_type", "weight_fp_type", "fc2_fp_type")}
    m = ql.quantize_VAR_mixed(_Var(128, 1), fmt, real_fp4=True, **kw)
    blk = m.blocks[0]
    assert isinstance(blk.ffn.fc1, _Marker) and blk.ffn.fc1.act == "fp_e1" and blk.ffn.fc1.kmajor_arg is False
    assert type(blk.attn.mat_qkv) is ql.QuantizedLinear and type(blk.attn.proj) is ql.QuantizedLinear
    assert type(blk.ffn.fc2) is ql.QuantizedLinear_fc2 and isinstance(blk.ada_lin[1], torch.nn.Linear)
    # a shape the GEMM does not take stays a QuantizedLinear: in_features % 128, out_features % 8
    odd = _Var(128, 1)
    odd.blocks[0].ffn.fc1 = torch.nn.Linear(192, 512)
    odd.blocks[0].attn.proj = torch.nn.Linear(128, 100)
    m = ql.quantize_VAR_mixed(odd, lambda b, layer: ("fp_e3", "fp_e2") if layer != "fc2" else ("fp_e1m2_neg_e2m1_pos", "fp_e2"), real_fp4=True, **kw)
    assert type(m.blocks[0].ffn.fc1) is ql.QuantizedLinear and type(m.blocks[0].attn.proj) is ql.QuantizedLinear
    assert isinstance(m.blocks[0].attn.mat_qkv, _Marker)


def test_real_fp4_refusals(cpu_construction):
    ql = cpu_construction
    for bad in (dict(weight_quant="per_channel"), dict(act_quant="per_token"), dict(w_bit=6), dict(a_bit=8),
                dict(activation_fp_quant=False), dict(weight_fp_quant=False)):
        kw = dict(W4A4, **bad)
        for fn in (ql.quantize_VAR_mixed_fp4_datatype, ql.quantize_VAR_use_different_datatype):
            with pytest.raises(ValueError, match="real_fp4 needs weight_quant = act_quant = 'per_group', w_bit = a_bit = 4"):
                fn(_Var(128, 1), real_fp4=True, **kw)
        mk = {k: v for k, v in kw.items() if k not in ("act_fp_type", "weight_fp_type", "fc2_fp_type")}
        with pytest.raises(ValueError, match="real_fp4 needs"):
            ql.quantize_VAR_mixed(_Var(128, 1), lambda b, layer: ("fp_e3", "fp_e2"), real_fp4=True, **mk)
    # quantize_VAR's own refusal is what it was: anything but fp_e2 on both sides
    with pytest.raises(ValueError, match="fp_e2 on both sides"):
        ql.quantize_VAR(_Var(128, 1), real_fp4=True, **dict(W4A4, act_fp_type="fp_e3"))
