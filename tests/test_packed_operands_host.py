"""CPU-only: the code maps of fpq_packed_to_operands / fpq_operands_to_packed against the value tables (tests/packed_operands_model.py),
the two entry points' declaration, export, signatures and refusals in the documented order, and the Python layer's checks that need
no GPU (operands() on CPU tensors, attach's strictness, the from_float mismatches)."""
import os
import re

import numpy as np
import pytest
import torch

from fpqvar_amd import _lib, gemm, packed as pk, quant_linear as ql
from oracle import fpq_oracle as orc
from tests import packed_operands_model as pm

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = open(os.path.join(ROOT, "include", "fpq.h")).read()


def table_dedup(table):
    return np.unique(orc.TABLES[table].numpy())     # sorted, de-duplicated (the two zeros of the 64-entry tables are one level)


@pytest.mark.parametrize("table", pm.TABLES)
def test_level_of_the_mapped_code_is_the_tables_level(table):
    levels = table_dedup(table)
    assert len(levels) == 2 * pm.ZERO[table] + 1 and levels[pm.ZERO[table]] == 0
    idx = np.arange(len(levels))
    code = pm.code_of_index(table, idx)
    assert np.array_equal(pm.decode(pm.CODE_FORMAT[table], code), levels.astype(np.float32))
    assert code[pm.ZERO[table]] == 0                                     # a zero level is code 0 in every format
    # the torch decoders of the hardware formats agree (gemm.dequantize_mx / dequantize_fp6)
    c = torch.from_numpy(code.astype(np.uint8))
    if table == "e2m1":
        c16 = torch.cat([c, c.new_zeros(256 - len(c))]).view(1, 128, 2)
        got = gemm.dequantize_mx(c16[..., 0] | (c16[..., 1] << 4), torch.ones(1, 2))[0, :len(levels)]
    else:
        c64 = torch.cat([c, c.new_zeros(64 - len(c))]).view(1, 64)
        got = gemm.dequantize_fp6(torch.from_numpy(pm.pack6(c64.numpy())), torch.ones(1), pm.CODE_FORMAT[table])[0, :len(levels)]
    assert np.array_equal(got.numpy(), levels.astype(np.float32))


@pytest.mark.parametrize("table", pm.TABLES)
def test_maps_are_bijections_onto_the_quantizers_codes(table):
    n = 2 * pm.ZERO[table] + 1
    code = pm.code_of_index(table, np.arange(n))
    assert len(set(code.tolist())) == n                                   # one code per level ...
    # ... and exactly the codes the quantizers emit: the level's code in its hardware format, a zero of either sign as code 0
    fmt = pm.CODE_FORMAT[table]
    every = np.arange(16 if fmt == "e2m1" else 64)
    by_level = {float(pm.decode(fmt, c)): int(c) for c in every[::-1] if c != (8 if fmt == "e2m1" else 32)}
    assert sorted(code.tolist()) == sorted(by_level[float(v)] for v in table_dedup(table))
    assert np.array_equal(pm.index_of_code(table, code), np.arange(n))    # the inverse undoes it
    assert pm.code_of_index(table, [n])[0] == 0                           # nibble 15 / field 63: no level -> code 0
    assert pm.index_of_code(table, [pm.SIGN[table]])[0] == pm.ZERO[table] # negative zero -> the zero index
    assert pm.index_of_code(table, every).max() <= n - 1                  # any code -> an index in range


def test_packings_round_trip_and_match_the_library():
    rng = np.random.default_rng(0)
    c = rng.integers(0, 64, (5, 128), dtype=np.uint8)
    assert np.array_equal(pm.unpack6(pm.pack6(c)), c) and np.array_equal(pm.unpack4(pm.pack4(c & 15)), c & 15)
    assert np.array_equal(pk.pack6(torch.from_numpy(c)).numpy(), pm.pack6(c))
    for table in pm.TABLES:
        idx = rng.integers(0, 2 * pm.ZERO[table] + 1, (3, 256), dtype=np.uint8)
        packed = pm.pack4(idx) if table in pm.FP4_TABLES else pm.pack6(idx)
        assert np.array_equal(pm.packed_of_operands(table, pm.operands_rowmajor(table, packed)), packed)


def test_fp4_operands_agrees_with_the_model():
    """the torch lookup the project had for E2M1 is the same map (index 15 included)"""
    codes = torch.arange(256, dtype=torch.uint8).view(4, 64)
    p = pk.PackedWeight(codes, torch.ones(4, dtype=torch.float16), "e2m1", 128, (4, 128))
    assert np.array_equal(p.fp4_operands()[0].numpy(), pm.operands_rowmajor("e2m1", codes.numpy()))


def test_header_declares_both_entry_points_and_keeps_the_version():
    assert re.search(r"#define FPQ_VERSION 136\b", HEADER)
    code = re.sub(r"/\*.*?\*/", "", HEADER, flags=re.S)
    assert re.search(r"int fpq_packed_to_operands\(const uint8_t\* codes, const void\* scales, int scale_dtype,\s*uint8_t\* w_codes, "
                     r"float\* w_scales,\s*int64_t outs, int64_t k, int64_t cols, int table_id, int kmajor, fpq_stream_t stream\);", code)
    assert re.search(r"int fpq_operands_to_packed\(const uint8_t\* w_codes, const float\* w_scales,\s*uint8_t\* codes, float\* scales,\s*"
                     r"int64_t outs, int64_t k, int64_t cols, int table_id, int kmajor, fpq_stream_t stream\);", code)


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as g
    g.build_hip()
    return _lib.lib()


def test_library_exports_both_with_signatures(lib):
    import ctypes as c
    assert lib.fpq_version() == 136
    assert _lib._SIGS["fpq_packed_to_operands"] == (c.c_int, [c.c_void_p, c.c_void_p, c.c_int, c.c_void_p, c.c_void_p, c.c_int64, c.c_int64,
                                                               c.c_int64, c.c_int, c.c_int, c.c_void_p])
    assert _lib._SIGS["fpq_operands_to_packed"] == (c.c_int, [c.c_void_p, c.c_void_p, c.c_void_p, c.c_void_p, c.c_int64, c.c_int64, c.c_int64,
                                                               c.c_int, c.c_int, c.c_void_p])
    assert lib.fpq_packed_to_operands.argtypes and lib.fpq_operands_to_packed.argtypes


OK, ARG, DTYPE, SHAPE, TABLE = 0, -1, -2, -3, -4


def test_refusals_in_the_documented_order(lib):
    def fwd(outs=8, k=128, cols=128, table=0, kmajor=0, dtype=0, ptrs=(None, None, None, None)):
        return lib.fpq_packed_to_operands(ptrs[0], ptrs[1], dtype, ptrs[2], ptrs[3], outs, k, cols, table, kmajor, None)

    def inv(outs=8, k=128, cols=128, table=0, kmajor=0, ptrs=(None, None, None, None)):
        return lib.fpq_operands_to_packed(ptrs[0], ptrs[1], ptrs[2], ptrs[3], outs, k, cols, table, kmajor, None)

    for f in (fwd, inv):
        # 1. the table, before everything else (bad sizes and shapes beside it)
        assert f(table=5, outs=-1, k=100) == TABLE and f(table=-1) == TABLE and f(table=9) == TABLE
        # 2. negative sizes (with a bad shape beside them)
        assert f(outs=-1, k=100) == ARG and f(k=-128) == ARG and f(cols=-1) == ARG
        # 4. shapes
        assert f(k=100) == SHAPE and f(k=256, cols=64) == SHAPE and f(k=256, cols=100) == SHAPE
        assert f(k=256, cols=256, table=1) == SHAPE and f(k=256, cols=256, table=0) == SHAPE      # per channel is for the FP6 tables
        assert f(k=128, cols=128, table=2) == ARG and f(k=256, cols=256, table=3) == ARG          # (accepted: next stop is the pointers)
        assert f(outs=1 << 17, k=1 << 15) == SHAPE and f(outs=1 << 17, k=1 << 15, kmajor=1) == SHAPE   # 2^31 bytes of nibbles
        assert f(outs=(1 << 17) - 63, k=1 << 15) == SHAPE and f(outs=(1 << 17) - 64, k=1 << 15) == ARG   # (rows rounded up to 64)
        assert f(outs=1 << 17, k=1 << 14, table=3) == ARG                                         # 1.5 GiB of 6-bit codes: fits
        assert f(outs=1 << 17, k=1 << 15, table=3) == SHAPE
        # 5. empty, before the pointers
        assert f(outs=0) == OK and f(k=0, cols=0, table=3) == OK and f(k=0) == OK and f(outs=0, k=100) == SHAPE
        # 6. pointers: NULL, then alignment (host addresses: nothing is launched on a refusal)
        assert f() == ARG and f(ptrs=(16, 16, 32, None)) == ARG and f(ptrs=(16, 32, 48, 72)) == ARG and f(ptrs=(8, 32, 48, 64)) == ARG
        assert f(k=256, cols=256, table=3, ptrs=(16, None, 40, None)) == ARG
    # 3. the dtype of the file's scales (forward only), after the sizes and before the shapes
    assert fwd(dtype=2, k=100) == DTYPE and fwd(dtype=7) == DTYPE and fwd(dtype=2, outs=-1) == ARG and fwd(dtype=2, table=7) == TABLE


def test_header_documents_the_checks_in_that_order():
    doc = HEADER[HEADER.index("PACKED WEIGHTS <-> WEIGHT OPERANDS"):HEADER.index("int fpq_packed_to_operands(")]
    order = [doc.index(w) for w in ("FPQ_ERR_TABLE", "FPQ_ERR_ARG", "FPQ_ERR_DTYPE", "FPQ_ERR_SHAPE", "FPQ_OK", "NULL pointers")]
    assert order == sorted(order)


def test_operands_refuses_cpu_tensors():
    p = pk.PackedWeight(torch.zeros(8, 64, dtype=torch.uint8), torch.ones(8, dtype=torch.float16), "e2m1", 128, (8, 128))
    with pytest.raises(RuntimeError, match="GPU"):
        p.operands()
    with pytest.raises(RuntimeError, match="GPU"):
        p.operands(kmajor=True)
    with pytest.raises(RuntimeError, match="GPU"):
        pk.PackedWeight.from_operands(torch.zeros(8, 64, dtype=torch.uint8), torch.ones(8, 1), "e2m1", (8, 128))
    with pytest.raises(RuntimeError, match="no packed form"):
        pk.PackedWeight.from_operands(torch.zeros(8, 64, dtype=torch.uint8), torch.ones(8, 1), "int_neg", (8, 128))


class _FFN(torch.nn.Module):
    def __init__(self):
        super().__init__()
        self.fc1, self.fc2, self.gate = torch.nn.Linear(128, 256), torch.nn.Linear(256, 128), torch.nn.Linear(128, 8)


def _packed(outs, k, table="e2m1", cols=128):
    four = table in pk.FP4_TABLES
    return pk.PackedWeight(torch.zeros(outs * k // cols, cols // 2 if four else cols * 3 // 4, dtype=torch.uint8),
                           torch.ones(outs * k // cols, dtype=torch.float16), table, cols, (outs, k))


def test_attach_is_strict_about_names():
    model = torch.nn.Sequential(_FFN())
    layers = {"0.fc1": _packed(256, 128), "0.fc2": _packed(128, 256)}
    pk.attach(model, layers)
    assert model[0].fc1.packed_weight is layers["0.fc1"] and model[0].fc2.packed_weight is layers["0.fc2"]
    with pytest.raises(KeyError, match="0.fc3"):
        pk.attach(torch.nn.Sequential(_FFN()), dict(layers, **{"0.fc3": _packed(8, 128)}))
    with pytest.raises(KeyError, match="0.fc2"):
        pk.attach(torch.nn.Sequential(_FFN()), {"0.fc1": layers["0.fc1"]})
    loose = pk.attach(torch.nn.Sequential(_FFN()), {"0.fc1": layers["0.fc1"], "1.fc9": layers["0.fc2"]}, strict=False)
    assert loose[0].fc1.packed_weight is layers["0.fc1"] and not hasattr(loose[0].fc2, "packed_weight")
    with pytest.raises(ValueError, match="0.fc1"):
        pk.attach(torch.nn.Sequential(_FFN()), {"0.fc1": _packed(128, 128), "0.fc2": layers["0.fc2"]})


def test_var_layer_format():
    f = pk.var_layer_format("per_group", "fp_e3", 4)
    lin = torch.nn.Linear(256, 64)
    assert f("blocks.0.ffn.fc1", lin) == ("e3m0", 128) and f("blocks.0.ada_lin.1", lin) is None
    assert pk.var_layer_format("per_channel", "fp6_e3m2", 6)("blocks.3.attn.proj", lin) == ("e3m2", 256)
    for bad in (("per_tensor", "fp_e2", 4), ("per_group", "int4", 4), ("per_group", "fp_e2", 6)):
        with pytest.raises(ValueError):
            pk.var_layer_format(*bad)


@pytest.fixture
def stub_lib(monkeypatch):
    """every C entry point answers 0 and touches nothing (tests/test_linear_call_path_host.py's way), CPU tensors pass for GPU ones"""
    class Stub:
        def __getattr__(self, name):
            return lambda *args: 0
    for mod in (gemm, _lib, pk):
        monkeypatch.setattr(mod, "lib", lambda: Stub(), raising=False)
        monkeypatch.setattr(mod, "require_gpu", lambda t, what: None, raising=False)
        monkeypatch.setattr(mod, "stream_ptr", lambda device: 0, raising=False)
        monkeypatch.setattr(mod, "device_guard", lambda device: _lib._NO_GUARD, raising=False)


_G = dict(weight_quant="per_group", act_quant="per_group", w_bit=4, a_bit=4, activation_fp_quant=True, weight_fp_quant=True,
          act_fp_type="fp_e2")


@pytest.mark.parametrize("build,asks", [
    (lambda lin: gemm.FP4Linear.from_float(lin), "FP4Linear.*e3m0.*128.*e2m1.*128"),
    (lambda lin: gemm.FP4LinearGeluDual.from_float(lin, weight_fp_type="fp_e1", w6_forms=True), "FP4LinearGeluDual.*e3m0.*e1m2"),
    (lambda lin: gemm.FP6GroupLinear.from_float(lin, "fp6_e2m3", "fp6_e2m3"), "FP6GroupLinear.*e3m0.*e2m3"),
    (lambda lin: gemm.FP6GroupLinearGeluDual.from_float(lin, "fp6_e3m2", "fp6_e2m3"), "FP6GroupLinearGeluDual.*e3m0.*e3m2"),
    (lambda lin: gemm.FP6Linear.from_float(lin), "FP6Linear.*e3m0.*128.*e2m3.*256"),
    (lambda lin: ql.QuantizedLinear.from_float(lin, weight_fp_type="fp_e2", **_G), "QuantizedLinear.*e3m0.*e2m1"),
    (lambda lin: ql.QuantizedLinear_fc2.from_float(lin, weight_fp_type="fp_e3", **dict(_G, weight_quant="per_channel")),
     "QuantizedLinear_fc2.*rows of 128.*rows of 256"),
])
def test_from_float_refuses_a_packed_weight_of_another_format(build, asks, stub_lib):
    lin = torch.nn.Linear(256, 128)
    lin.packed_weight = _packed(128, 256, "e3m0")
    with pytest.raises(ValueError, match=asks):
        build(lin)


def test_matching_packed_weight_is_used_and_the_weight_is_not_read(stub_lib):
    lin = torch.nn.Linear(256, 128)
    lin.packed_weight = _packed(128, 256, "e3m0")
    lin.weight = None                                   # reading it would raise
    m = gemm.FP4Linear.from_float(lin, weight_fp_type="fp_e3")
    assert m.w_codes.shape == (128, 192) and m.w_scales.shape == (128, 2) and m.w_scales.dtype == torch.float32 and m.w_table == "e3m0"
    m = gemm.FP4Linear.from_float(lin, weight_fp_type="fp_e3", w6_forms=True, kmajor=True, w6_kmajor=True)
    assert m.w_codes.shape == (2, 128, 96) and m.w_scales.shape == (2, 128)
    m = gemm.FP4Linear.from_packed(_packed(72, 128, "e2m1"), kmajor=True)
    assert m.w_codes.shape == (1, 128, 64) and m.w_scales.shape == (1, 128) and (m.in_features, m.out_features) == (128, 72)
    with pytest.raises(TypeError, match="weight format"):
        gemm.FP4Linear.from_packed(_packed(72, 128), weight_fp_type="fp_e2")


def test_fp8_linear_points_to_packed_e3m2(stub_lib):
    lin = torch.nn.Linear(256, 128)
    lin.packed_weight = _packed(128, 256, "e3m2", 256)
    with pytest.raises(ValueError, match="packed_e3m2=True"):
        gemm.FP8Linear.from_float(lin, "fp6_e3m2", "fp6_e2m3")


def test_from_packed_raises_where_from_float_would(stub_lib):
    with pytest.raises(ValueError, match="k-major"):
        gemm.FP4Linear.from_packed(_packed(128, 256, "e3m0"), kmajor=True)             # a W6 weight without w6_kmajor
    with pytest.raises(ValueError, match="fc1 tail"):
        gemm.FP4LinearGeluDual.from_packed(_packed(128, 256, "e1m2"))
    with pytest.raises(ValueError, match="belongs to FP4Linear"):
        gemm.FP6GroupLinear.from_packed(_packed(128, 256, "e2m1"), act_fp_type="fp_e2")
