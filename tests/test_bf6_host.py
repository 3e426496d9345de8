"""CPU-only: the BF6 (E3M2) side of the 6-bit operand path - the decoder of gemm.dequantize_fp6, the argument contract of the
C entry points that carry a format per operand (include/fpq.h, version 130), and the model-level keyword's refusal."""
import ctypes

import pytest
import torch

from oracle import fpq_oracle as orc
from tests import gemm_model as gm

OK, ERR_ARG, ERR_TABLE = 0, -1, -4
E2M3, E3M2 = 3, 4
BAD_TABLES = (-1, 0, 2, 5, 8, 10, 99)          # E2M1, E3M0, a half table, past the end


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as g
    g.build_hip()
    from fpqvar_amd import _lib
    assert _lib.TABLE_IDS["e2m3"] == E2M3 and _lib.TABLE_IDS["e3m2"] == E3M2
    return _lib.lib()


def test_decoder_tables():
    from fpqvar_amd import gemm
    codes = gm.encode("fp6", torch.arange(64).view(1, 64))
    one = torch.ones(1)
    bf6 = gemm.dequantize_fp6(codes, one, table="e3m2").view(64)
    tab = orc.TABLES["e3m2"]
    pos = torch.sort(tab[tab > 0]).values
    assert pos.numel() == 31 and float(pos[0]) == 1 / 16 and float(pos[-1]) == 28.0
    assert torch.equal(bf6[1:32], pos) and torch.equal(bf6[33:], -pos)
    assert float(bf6[0]) == 0.0 and float(bf6[32]) == 0.0
    assert int((tab == 0).sum()) == 2 and tab.numel() == 64           # two zeros, as codes 0 and 32
    assert torch.equal(torch.sort(bf6).values, torch.sort(tab).values)
    # e2m3 unchanged: the default, by either name, equals the format definition of tests/gemm_model.py
    want = gm.decode("fp6", codes).float().view(64)
    for got in (gemm.dequantize_fp6(codes, one), gemm.dequantize_fp6(codes, one, "e2m3"), gemm.dequantize_fp6(codes, one, table="fp6_e2m3")):
        assert torch.equal(got.view(64), want)
    pos3 = torch.sort(orc.TABLES["e2m3"][orc.TABLES["e2m3"] > 0]).values
    assert torch.equal(want[1:32], pos3) and torch.equal(want[33:], -pos3)
    assert torch.equal(gemm.dequantize_fp6(codes, one, "fp6_e3m2"), gemm.dequantize_fp6(codes, one, "e3m2"))
    with pytest.raises(RuntimeError):
        gemm.dequantize_fp6(codes, one, table="e2m1")


def test_dense_packing_round_trip():
    from fpqvar_amd import gemm
    g = torch.Generator().manual_seed(6)
    idx = torch.randint(0, 64, (37, 256), generator=g)
    packed = gm.encode("fp6", idx)
    assert packed.shape == (37, 192)
    scales = torch.rand(37, generator=g) + 0.5
    for table, e_bits, m_bits, bias in (("e3m2", 3, 2, 3), ("e2m3", 2, 3, 1)):
        e, m = (idx >> m_bits) & ((1 << e_bits) - 1), (idx & ((1 << m_bits) - 1)).double()
        mag = torch.where(e == 0, m / (1 << m_bits) * 2.0 ** (1 - bias), (1 + m / (1 << m_bits)) * torch.pow(2.0, (e - bias).double()))
        want = (torch.where((idx & 32) != 0, -mag, mag).float() * scales.view(-1, 1))
        assert torch.equal(gemm.dequantize_fp6(packed, scales, table=table), want), table


def _mask():
    return (ctypes.c_uint32 * 4)(1, 2, 3, 4)


def _split():
    """a descriptor that passes every check; with tokens == 0 nothing is launched and no address is used"""
    from fpqvar_amd._lib import GemmSplit
    sp = GemmSplit()
    sp.part_cols, sp.n_parts, sp.rows_per_batch = 128, 3, 1
    for p in range(3):
        sp.out[p], sp.row_stride[p], sp.batch_stride[p], sp.row0[p] = 4096, 128, 0, 0
    return sp


def _calls(lib):
    """name -> f(table or (a_table, w_table), empty): the entry point with null data pointers; `empty`: a problem of zero rows"""
    sp = _split()
    return {
        "fpq_quant_rows_codes_f6": lambda t, empty: lib.fpq_quant_rows_codes_f6(None, None, None, 0 if empty else 4, 128, t[0], 0, 0, None),
        "fpq_quant_rows_codes_f6 (k-major)": lambda t, empty: lib.fpq_quant_rows_codes_f6(None, None, None, 0 if empty else 4, 128, t[0], 0, 1, None),
        "fpq_adaln_rotate_quant_token_rows_codes_f6": lambda t, empty: lib.fpq_adaln_rotate_quant_token_rows_codes_f6(
            None, None, None, 0 if empty else 4, 128, 0, None, None, 0, 1, 1e-6, None, _mask(), t[0], 0, None),
        "fpq_gemm_f6_rows": lambda t, empty: lib.fpq_gemm_f6_rows(None, None, 0, t[0], None, None, 1, t[1], None, None, 0 if empty else 4, 8, 128,
                                                                  None, 0, None),
        "fpq_gemm_f6_rows_split": lambda t, empty: lib.fpq_gemm_f6_rows_split(None, None, 0, t[0], None, None, 1, t[1], None, 0 if empty else 4, 384,
                                                                              128, ctypes.byref(sp), 0, None),
        "fpq_gemm_f6_rows_split_qknorm": lambda t, empty: lib.fpq_gemm_f6_rows_split_qknorm(None, None, 0, t[0], None, None, 1, t[1], None,
                                                                                            0 if empty else 4, 384, 128, ctypes.byref(sp),
                                                                                            ctypes.cast(4096, ctypes.c_void_p), 0, None),
    }


def test_new_entry_points_table_contract(lib):
    for name, f in _calls(lib).items():
        two = "gemm" in name
        for bad in BAD_TABLES:
            assert f((bad, E2M3), False) == ERR_TABLE, (name, bad)
            assert f((bad, E3M2), True) == ERR_TABLE, (name, bad, "empty")     # decided before anything else
            if two:
                assert f((E2M3, bad), False) == ERR_TABLE and f((E3M2, bad), True) == ERR_TABLE, (name, bad, "weight side")
        for ta in (E2M3, E3M2):
            for tw in ((E2M3, E3M2) if two else (E2M3,)):
                assert f((ta, tw), True) == OK, (name, ta, tw)                 # an empty problem
                assert f((ta, tw), False) == ERR_ARG, (name, ta, tw)           # null pointers


def test_gemm_f6_scale_dtypes(lib):
    """a pair with an E3M2 side takes fp16 activation scales only (include/fpq.h); E2M3 x E2M3 all four pairs"""
    ERR_DTYPE = -2
    for ta, tw in ((E3M2, E2M3), (E2M3, E3M2), (E3M2, E3M2)):
        for w_dt in (0, 1):
            assert lib.fpq_gemm_f6_rows(None, None, 1, ta, None, None, w_dt, tw, None, None, 0, 8, 128, None, 0, None) == ERR_DTYPE
            assert lib.fpq_gemm_f6_rows(None, None, 0, ta, None, None, w_dt, tw, None, None, 0, 8, 128, None, 0, None) == OK
    for a_dt in (0, 1):
        for w_dt in (0, 1):
            assert lib.fpq_gemm_f6_rows(None, None, a_dt, E2M3, None, None, w_dt, E2M3, None, None, 0, 8, 128, None, 0, None) == OK
    assert lib.fpq_gemm_f6_rows(None, None, 2, E2M3, None, None, 0, E2M3, None, None, 0, 8, 128, None, 0, None) == ERR_DTYPE


def test_old_entry_points_keep_refusing_e3m2(lib):
    assert lib.fpq_quant_rows_codes_fp6(None, None, None, 4, 128, E3M2, 0, None) == ERR_TABLE
    assert lib.fpq_quant_rows_codes_fp6(None, None, None, 0, 128, E3M2, 0, None) == ERR_TABLE
    assert lib.fpq_quant_rows_codes_fp6_km(None, None, None, 4, 128, E3M2, 0, None) == ERR_TABLE
    assert lib.fpq_quant_rows_codes_fp6(None, None, None, 0, 128, E2M3, 0, None) == OK
    assert lib.fpq_quant_rows_codes_fp6(None, None, None, -1, 128, E3M2, 0, None) == ERR_ARG      # the order of the checks stays
    for fn in (lib.fpq_adaln_rotate_quant_token_rows_codes_fp6, lib.fpq_adaln_rotate_quant_token_rows_codes_fp6_km):
        assert fn(None, None, None, 0, 128, 0, None, None, 0, 1, 1e-6, None, _mask(), E3M2, None) == ERR_TABLE
        assert fn(None, None, None, 0, 128, 0, None, None, 0, 1, 1e-6, None, _mask(), E2M3, None) == OK


def test_python_layer_refusals():
    from fpqvar_amd import gemm, quant_linear as ql
    with pytest.raises(RuntimeError, match="GPU"):
        gemm.quantize_fp6(torch.zeros(2, 128).half(), table="e3m2")
    with pytest.raises(RuntimeError):
        gemm.FP6Linear(torch.zeros(8, 96, dtype=torch.uint8), torch.ones(8), None, 128, 8, act_table="e2m1")
    lin = gemm.FP6Linear(torch.zeros(8, 96, dtype=torch.uint8), torch.ones(8), None, 128, 8)
    assert (lin.act_table, lin.w_table) == ("e2m3", "e2m3")
    lin = gemm.FP6Linear(torch.zeros(8, 96, dtype=torch.uint8), torch.ones(8), None, 128, 8, "fp6_e3m2", "e2m3")
    assert (lin.act_table, lin.w_table) == ("e3m2", "e2m3") and "act=e3m2" in repr(lin)

    class Blk(torch.nn.Module):
        def __init__(self):
            super().__init__()
            self.ffn, self.attn = torch.nn.Module(), torch.nn.Module()
            self.ffn.fc1, self.ffn.fc2 = torch.nn.Linear(128, 256), torch.nn.Linear(256, 128)
            self.attn.mat_qkv, self.attn.proj = torch.nn.Linear(128, 384, bias=False), torch.nn.Linear(128, 128)

    class Toy(torch.nn.Module):
        def __init__(self):
            super().__init__()
            self.blocks = torch.nn.ModuleList([Blk()])

    per_group = dict(weight_quant="per_group", act_quant="per_group", w_bit=4, a_bit=4, act_quant_sym=True, activation_fp_quant=True,
                     weight_fp_quant=True)
    fmt = lambda b, layer: ("fp6_e3m2", "fp6_e2m3")
    with pytest.raises(ValueError, match="real_fp6"):
        ql.quantize_VAR_mixed(Toy(), fmt, real_fp6=True, **per_group)
    with pytest.raises(ValueError, match="real_fp6"):
        ql.quantize_VAR_mixed_fp6_datatype(Toy(), real_fp6=True, act_fp_type="fp_e2", weight_fp_type="fp_e2", **per_group)
    w6 = dict(weight_quant="per_channel", act_quant="per_token", w_bit=6, a_bit=6, act_quant_sym=True, activation_fp_quant=True,
              weight_fp_quant=True)
    with pytest.raises(ValueError, match="real_fp6"):
        ql.quantize_VAR_mixed(Toy(), fmt, real_fp6=True, **{**w6, "a_bit": 8})
    with pytest.raises(ValueError, match="real_fp6"):
        ql.quantize_VAR_mixed(Toy(), fmt, real_fp6=True, **{**w6, "activation_fp_quant": False})
