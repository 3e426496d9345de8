"""The Python front of the per-group Linears (gemm.linear_fp4*, gemm.linear_a6w4*, the quantizers, FP4Linear / FP4LinearGeluDual)
without a GPU: which C entry point each call ends in and every argument it passes, with the library replaced by a recorder.
CPU tensors stand in for the operands - nothing reads them; a pointer is told by the tensor it belongs to."""
import contextlib

import pytest
import torch

from fpqvar_amd import _lib, gemm

F16, F32 = 0, 1
TID = {"e2m1": None, "e1m2": 1, "e3m0": 2}          # the table id after a_scales (enum fpq_table), none in the FP4 family
SEG = {"e2m1": 64, "e1m2": 96, "e3m0": 96}          # bytes per 128 elements
FORMATS, LAYOUTS = ("e2m1", "e1m2", "e3m0"), (False, True)
T, K, G = 8, 256, 2
GEMM = {("plain", "fp4", False): "fpq_gemm_fp4_mx_ex", ("plain", "fp4", True): "fpq_gemm_fp4_mx_km",
        ("plain", "a6w4", False): "fpq_gemm_a6w4_mx", ("plain", "a6w4", True): "fpq_gemm_a6w4_mx_km",
        ("fc1", "fp4", False): "fpq_gemm_fp4_gelu_dual", ("fc1", "fp4", True): "fpq_gemm_fp4_gelu_dual_km",
        ("fc1", "a6w4", False): "fpq_gemm_a6w4_gelu_dual", ("fc1", "a6w4", True): "fpq_gemm_a6w4_gelu_dual_km",
        ("qkv", "fp4"): "fpq_gemm_fp4_mx_split", ("qkv_norm", "fp4"): "fpq_gemm_fp4_mx_split_qknorm",
        ("qkv", "a6w4"): "fpq_gemm_a6w4_mx_split", ("qkv_norm", "a6w4"): "fpq_gemm_a6w4_mx_split_qknorm"}
QUANT = {("fp4", False): "fpq_quant_rows_codes_mx", ("fp4", True): "fpq_quant_rows_codes_mx_km",
         ("a6w4", False): "fpq_quant_rows_codes_g6", ("a6w4", True): "fpq_a6w4_quant_rows_codes_km"}


def family(fmt):
    return "fp4" if fmt == "e2m1" else "a6w4"


def _decode(arg):
    """the struct behind a ctypes.byref argument as plain values"""
    s = getattr(arg, "_obj", None)
    if isinstance(s, _lib.GemmEpilogue):
        return ("epilogue", s.gate, s.residual, s.rows_per_gate)
    if isinstance(s, _lib.GemmSplit):
        return ("split", s.part_cols, s.n_parts, s.rows_per_batch, tuple(s.out), tuple(s.row_stride), tuple(s.batch_stride), tuple(s.row0))
    return arg


class Recorder:
    def __init__(self):
        self.calls = []

    def __getattr__(self, name):
        def entry(*args):
            self.calls.append((name, tuple(_decode(a) for a in args)))
            return 0
        return entry

    def take(self):
        calls, self.calls = self.calls, []
        return calls


NAN_FLAG = torch.zeros(2, dtype=torch.int32)


@pytest.fixture
def rec(monkeypatch):
    r = Recorder()
    monkeypatch.setattr(gemm, "_native", None)
    monkeypatch.setattr(gemm, "require_gpu", lambda *a, **k: None)
    monkeypatch.setattr(gemm, "stream_ptr", lambda device: 0)
    monkeypatch.setattr(gemm, "device_guard", lambda device: contextlib.nullcontext())
    monkeypatch.setattr(gemm, "lib", lambda: r)
    monkeypatch.setattr("fpqvar_amd.ops._nan_scratch", lambda device: NAN_FLAG)
    return r


def named(calls, **tensors):
    """The recorded calls with every pointer replaced by the name of the tensor it is the address of (`tensors`: name -> tensor or
    None); the address of anything else - what the call allocated itself - becomes tmp0, tmp1, ... in the order of appearance."""
    names = {t.data_ptr(): n for n, t in tensors.items() if t is not None}
    def one(v):
        if isinstance(v, tuple):
            return tuple(one(e) for e in v)
        if isinstance(v, int) and not isinstance(v, bool) and v >= 1 << 16:
            return names.setdefault(v, f"tmp{sum(1 for n in names.values() if n.startswith('tmp'))}")
        return v
    out = []
    for name, args in calls:
        assert len(args) == len(_lib._SIGS[name][1]), (name, len(args))
        out.append((name, one(args)))
    return out


def operands(fmt, km, tokens, outs):
    """(a, a_scales, w, w_scales) of the right shapes and dtypes: row-major codes, or the k-major images with their fp32 scale images"""
    if km:
        rows64 = (outs + 63) // 64 * 64
        return (torch.zeros(G, tokens, SEG[fmt], dtype=torch.uint8), torch.zeros(G, (tokens + 3) // 4 * 4),
                torch.zeros(G, rows64, 64, dtype=torch.uint8), torch.zeros(G, rows64))
    return (torch.zeros(tokens, G * SEG[fmt], dtype=torch.uint8), torch.zeros(tokens, G, dtype=torch.float16),
            torch.zeros(outs, K // 2, dtype=torch.uint8), torch.zeros(outs, G))


def fp16(*shape):
    return torch.zeros(*shape, dtype=torch.float16)


# ---- the public function of a format and layout ----------------------------------------------------------------------------------
def plain(fmt, km, a, sa, w, sw, bias=None, gate=None, residual=None, outs=None):
    if fmt == "e2m1":
        return gemm.linear_fp4(a, sa, w, sw, bias, gate, residual, outs=outs)
    if km:
        return gemm.linear_a6w4_km(a, sa, fmt, w, sw, bias, gate, residual, outs=outs)
    return gemm.linear_a6w4(a, sa, fmt, w, sw, bias, gate, residual)


def fc1(fmt, km, a, sa, w, sw, bias=None, return_gelu=False, outs=None):
    if fmt == "e2m1":
        return gemm.linear_fp4_gelu_dual(a, sa, w, sw, bias, return_gelu, outs=outs)
    if km:
        return gemm.linear_a6w4_gelu_dual_km(a, sa, fmt, w, sw, bias, return_gelu, outs=outs)
    return gemm.linear_a6w4_gelu_dual(a, sa, fmt, w, sw, bias, return_gelu)


def qkv(fmt, a, sa, w, sw, bias, cache, pos, seq, hs=None):
    if fmt == "e2m1":
        return gemm.linear_fp4_qkv_to_cache(a, sa, w, sw, bias, cache, pos, seq, hs)
    return gemm.linear_a6w4_qkv_to_cache(a, sa, fmt, w, sw, bias, cache, pos, seq, hs)


def quantize(fmt, x, km):
    return gemm.quantize_mx(x, kmajor=km) if fmt == "e2m1" else gemm.quantize_g6(x, fmt, kmajor=km)


def tid(fmt):
    return () if TID[fmt] is None else (TID[fmt],)


# ---- the plain Linear -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("tail", (False, True))
@pytest.mark.parametrize("km", LAYOUTS)
@pytest.mark.parametrize("fmt", FORMATS)
def test_plain(rec, fmt, km, tail):
    """outs 136: from the weight's rows (row-major), or named by `outs` against an image of 192 rows.  Without the tail a bias and a
    NULL epilogue; with it no bias, gate [2, 1, outs] over 8 tokens and a residual"""
    outs = 136
    a, sa, w, sw = operands(fmt, km, T, outs)
    assert not km or w.shape[1] == 192
    bias = None if tail else fp16(outs)
    gate, res = (fp16(2, 1, outs), fp16(2, 4, outs)) if tail else (None, None)
    y = plain(fmt, km, a, sa, w, sw, bias, gate, res, outs=outs if km else None)
    assert y.shape == (T, outs) and y.dtype == torch.float16
    ep = ("epilogue", "gate", "res", 4) if tail else None
    assert named(rec.take(), a=a, sa=sa, w=w, sw=sw, bias=bias, gate=gate, res=res, y=y) == [
        (GEMM["plain", family(fmt), km], ("a", "sa", *tid(fmt), "w", "sw", F32, None if tail else "bias", "y", T, outs, K, ep, 0))]


def test_plain_other_arguments(rec):
    """fp16 weight scales (row-major): their dtype id; a residual alone: rows_per_gate 1 and a NULL gate; no tokens: still a call"""
    a, sa, w, sw = operands("e2m1", False, T, 128)
    swh, res = sw.half(), fp16(T, 128)
    y = gemm.linear_fp4(a, sa, w, swh, None, None, res)
    assert named(rec.take(), a=a, sa=sa, w=w, sw=swh, res=res, y=y) == [
        ("fpq_gemm_fp4_mx_ex", ("a", "sa", "w", "sw", F16, None, "y", T, 128, K, ("epilogue", None, "res", 1), 0))]
    y = gemm.linear_a6w4(a6 := torch.zeros(T, 192, dtype=torch.uint8), sa, "fp_e1", w, swh)
    assert named(rec.take(), a=a6, sa=sa, w=w, sw=swh, y=y) == [("fpq_gemm_a6w4_mx", ("a", "sa", 1, "w", "sw", F16, None, "y", T, 128, K, None, 0))]
    for fmt in FORMATS:
        for km in LAYOUTS:
            a, sa, w, sw = operands(fmt, km, 0, 128)
            y = plain(fmt, km, a, sa, w, sw)
            assert y.shape == (0, 128)
            (name, args), = rec.take()
            assert name == GEMM["plain", family(fmt), km] and args[-5:-2] == (0, 128, K), (fmt, km)


# ---- fc1 --------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("return_gelu", (False, True))
@pytest.mark.parametrize("km", LAYOUTS)
@pytest.mark.parametrize("fmt", FORMATS)
def test_fc1(rec, fmt, km, return_gelu):
    outs = 128
    a, sa, w, sw = operands(fmt, km, T, outs)
    bias = fp16(outs)
    got = fc1(fmt, km, a, sa, w, sw, bias, return_gelu)
    y, h = got if return_gelu else (got, None)
    assert y.shape == (T, outs) and (h is None or h.shape == (T, outs))
    assert named(rec.take(), a=a, sa=sa, w=w, sw=sw, bias=bias, y=y, h=h, flag=NAN_FLAG) == [
        (GEMM["fc1", family(fmt), km], ("a", "sa", *tid(fmt), "w", "sw", F32, "bias", "y", "h" if return_gelu else None, T, outs, K, "flag", 0))]


@pytest.mark.parametrize("km", LAYOUTS)
@pytest.mark.parametrize("fmt", FORMATS)
def test_fc1_without_tokens_launches_nothing(rec, fmt, km):
    a, sa, w, sw = operands(fmt, km, 0, 128)
    y, h = fc1(fmt, km, a, sa, w, sw, None, True)
    assert y.shape == (0, 128) and h.shape == (0, 128) and rec.take() == []


# ---- mat_qkv into the cache -------------------------------------------------------------------------------------------------------
H, C, B, SEQ, MAX_LEN, POS = 2, 64, 2, 4, 16, 3


@pytest.mark.parametrize("norm", (False, True))
@pytest.mark.parametrize("km", LAYOUTS)
@pytest.mark.parametrize("fmt", FORMATS)
def test_qkv(rec, fmt, km, norm):
    outs = 3 * H * C
    a, sa, w, sw = operands(fmt, km, B * SEQ, outs)
    cache = fp16(2, B, MAX_LEN, H, C)
    bias, hs = (torch.zeros(outs), torch.ones(H)) if norm else (fp16(outs), None)
    q = qkv(fmt, a, sa, w, sw, bias, cache, POS, SEQ, hs)
    assert q.shape == (B, SEQ, H * C) and q.dtype == torch.float16
    split = ("split", H * C, 3, SEQ, ("q", "k", "v"), (H * C,) * 3, (SEQ, MAX_LEN, MAX_LEN), (0, POS, POS))
    assert named(rec.take(), a=a, sa=sa, w=w, sw=sw, bias=bias, hs=hs, q=q, k=cache[0], v=cache[1]) == [
        (GEMM["qkv_norm" if norm else "qkv", family(fmt)],
         ("a", "sa", *tid(fmt), "w", "sw", F32, "bias", B * SEQ, outs, K, split, *(("hs",) if norm else ()), 1 if km else 0, 0))]


@pytest.mark.parametrize("km", LAYOUTS)
@pytest.mark.parametrize("fmt", FORMATS)
def test_qkv_without_tokens_launches_nothing(rec, fmt, km):
    outs = 3 * H * C
    a, sa, w, sw = operands(fmt, km, 0, outs)
    for hs in (None, torch.ones(H)):
        q = qkv(fmt, a, sa, w, sw, None, fp16(2, 0, MAX_LEN, H, C), POS, SEQ, hs)
        assert q.shape == (0, SEQ, H * C) and rec.take() == []


# ---- the quantizers ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("km", LAYOUTS)
def test_quantizers(rec, km):
    x = fp16(2, 4, K)
    for fmt in FORMATS:
        codes, scales = quantize(fmt, x, km)
        assert codes.dtype == torch.uint8 and tuple(codes.shape) == ((G, T, SEG[fmt]) if km else (T, G * SEG[fmt]))
        assert (scales.dtype, tuple(scales.shape)) == ((torch.float32, (G, T)) if km else (torch.float16, (T, G)))
        assert named(rec.take(), x=x, codes=codes, scales=scales) == [
            (QUANT[family(fmt), km], ("x", "codes", "scales", T, K, *tid(fmt), F16, 0))]
    for table, want in (("e2m3", ("fpq_quant_rows_codes_fp6_km" if km else "fpq_quant_rows_codes_fp6", ("x", "codes", "scales", T, K, 3, F16, 0))),
                        ("fp6_e3m2", ("fpq_quant_rows_codes_f6", ("x", "codes", "scales", T, K, 4, F16, 1 if km else 0, 0)))):
        codes, scales = gemm.quantize_fp6(x, kmajor=km, table=table)
        assert tuple(codes.shape) == ((G, T, 96) if km else (T, 192)) and tuple(scales.shape) == (T,)
        assert named(rec.take(), x=x, codes=codes, scales=scales) == [want]


def test_quantizers_fp32_rows(rec):
    """fp32 rows (weights): scales in fp32; the image-writing quantizers take fp16 rows, so kmajor=True is two steps"""
    x = torch.zeros(5, K)
    for fmt in FORMATS:
        codes, scales = quantize(fmt, x, False)
        assert scales.dtype == torch.float32
        assert named(rec.take(), x=x, codes=codes, scales=scales) == [(QUANT[family(fmt), False], ("x", "codes", "scales", 5, K, *tid(fmt), F32, 0))]
        codes, scales = quantize(fmt, x, True)
        assert tuple(codes.shape) == (G, 5, SEG[fmt]) and tuple(scales.shape) == (G, 8) and scales.dtype == torch.float32
        assert named(rec.take(), x=x, codes=codes, scales=scales) == [
            (QUANT[family(fmt), False], ("x", "tmp0", "tmp1", 5, K, *tid(fmt), F32, 0)),
            ("fpq_codes_to_kmajor", ("tmp0", "codes", 5, K, 4 if fmt == "e2m1" else 6, 0, 0)),
            ("fpq_scales_to_kmajor", ("tmp1", F32, "scales", 5, G, 0, 0))]


# ---- the modules make the calls of their format's public functions ---------------------------------------------------------------
def module(cls, fmt, km, outs, bias=True):
    _, _, w, sw = operands(fmt, km, T, outs)
    return cls(w, sw, fp16(outs) if bias else None, K, outs, fmt)


@pytest.mark.parametrize("km", LAYOUTS)
@pytest.mark.parametrize("fmt", FORMATS)
def test_fp4linear_forward(rec, fmt, km):
    m = module(gemm.FP4Linear, fmt, km, 136)
    assert m.kmajor == km
    x, gate, res = fp16(2, 4, K), fp16(2, 1, 136), fp16(2, 4, 136)
    names = dict(x=x, w=m.w_codes, sw=m.w_scales, bias=m.bias, gate=gate, res=res)
    for tail in ((), (gate, res)):
        y = m(x, *tail)
        assert y.shape == (2, 4, 136)
        got = named(rec.take(), **names)
        a, sa = quantize(fmt, x.view(-1, K), km)
        plain(fmt, km, a, sa, m.w_codes, m.w_scales, m.bias, *tail, outs=136)
        assert got == named(rec.take(), **names)
        assert [n for n, _ in got] == [QUANT[family(fmt), km], GEMM["plain", family(fmt), km]] and got[1][1][-5:-2] == (T, 136, K)
        # the same product from operands: the module's format by default, or the one `table` names
        for table in (None, fmt, {"e2m1": "fp_e2", "e1m2": "fp_e1", "e3m0": "fp_e3"}[fmt]):
            y = m.forward_operands(a, sa, *tail, table=table)
            assert y.shape == (T, 136)
            by_module = named(rec.take(), a=a, sa=sa, **names)
            plain(fmt, km, a, sa, m.w_codes, m.w_scales, m.bias, *tail, outs=136)
            assert by_module == named(rec.take(), a=a, sa=sa, **names)


@pytest.mark.parametrize("km", LAYOUTS)
@pytest.mark.parametrize("fmt", FORMATS)
def test_fp4linear_qkv_to_cache(rec, fmt, km):
    outs = 3 * H * C
    x, cache = fp16(B, SEQ, K), fp16(2, B, MAX_LEN, H, C)
    for norm in (False, True):
        m = module(gemm.FP4Linear, fmt, km, outs, bias=not norm)
        bias32, hs = (torch.zeros(outs), torch.ones(H)) if norm else (None, None)
        names = dict(x=x, w=m.w_codes, sw=m.w_scales, bias=bias32 if norm else m.bias, hs=hs, k=cache[0], v=cache[1])
        q = m.qkv_to_cache(x, cache, POS, SEQ, hs, bias32)
        assert q.shape == (B, SEQ, H * C)
        got = named(rec.take(), **names)
        a, sa = quantize(fmt, x.view(-1, K), km)
        qkv(fmt, a, sa, m.w_codes, m.w_scales, bias32 if norm else m.bias, cache, POS, SEQ, hs)
        assert got == named(rec.take(), **names)
        assert [n for n, _ in got] == [QUANT[family(fmt), km], GEMM["qkv_norm" if norm else "qkv", family(fmt)]]
        assert got[1][1][-2] == (1 if km else 0)


@pytest.mark.parametrize("km", LAYOUTS)
@pytest.mark.parametrize("fmt", FORMATS)
def test_fp4linear_gelu_dual(rec, fmt, km):
    m = module(gemm.FP4LinearGeluDual, fmt, km, 128)
    x = fp16(2, 4, K)
    names = dict(x=x, w=m.w_codes, sw=m.w_scales, bias=m.bias, flag=NAN_FLAG)
    y = m(x)
    assert y.shape == (2, 4, 128)
    got = named(rec.take(), **names)
    a, sa = quantize(fmt, x.view(-1, K), km)
    fc1(fmt, km, a, sa, m.w_codes, m.w_scales, m.bias, outs=128)
    assert got == named(rec.take(), **names)
    assert [n for n, _ in got] == [QUANT[family(fmt), km], GEMM["fc1", family(fmt), km]] and got[1][1][-6] is None   # no GELU output
    for table in (None, fmt):
        y = m.forward_operands(a, sa, table=table)
        assert y.shape == (T, 128)
        by_module = named(rec.take(), a=a, sa=sa, **names)
        fc1(fmt, km, a, sa, m.w_codes, m.w_scales, m.bias, outs=128)
        assert by_module == named(rec.take(), a=a, sa=sa, **names)


def test_forward_operands_in_another_format(rec):
    """`table` names the format of the codes, whatever the module's own: E3M0 codes into an E2M1 module and back"""
    for km in LAYOUTS:
        for cls, run, outs in ((gemm.FP4Linear, plain, 136), (gemm.FP4LinearGeluDual, fc1, 128)):
            for own, other in (("e2m1", "e3m0"), ("e1m2", "e2m1"), ("e3m0", "fp_e1")):
                m = module(cls, own, km, outs)
                fmt = {"fp_e1": "e1m2"}.get(other, other)
                a, sa, _, _ = operands(fmt, km, T, outs)
                names = dict(a=a, sa=sa, w=m.w_codes, sw=m.w_scales, bias=m.bias, flag=NAN_FLAG)
                m.forward_operands(a, sa, table=other)
                by_module = named(rec.take(), **names)
                run(fmt, km, a, sa, m.w_codes, m.w_scales, m.bias, outs=outs)
                assert by_module == named(rec.take(), **names) and by_module[0][0] == GEMM["plain" if run is plain else "fc1", family(fmt), km]


def test_e2m1_modules_end_in_the_compiled_binding(rec, monkeypatch):
    """with the binding loaded, the E2M1 modules hand the GEMM to it - nothing but the quantizer goes through ctypes"""
    seen = []

    class Native:
        @staticmethod
        def linear_fp4(*args):
            seen.append(("linear_fp4", args))
            return fp16(T, 136)

        @staticmethod
        def linear_fp4_gelu_dual(*args):
            seen.append(("linear_fp4_gelu_dual", args))
            return fp16(T, 128), None

    monkeypatch.setattr(gemm, "_native", Native)
    x, gate, res = fp16(2, 4, K), fp16(2, 1, 136), fp16(2, 4, 136)
    for km in LAYOUTS:
        m = module(gemm.FP4Linear, "e2m1", km, 136)
        assert m(x, gate, res).shape == (2, 4, 136)
        f = module(gemm.FP4LinearGeluDual, "e2m1", km, 128)
        assert f(x).shape == (2, 4, 128)
        assert [n for n, _ in rec.take()] == [QUANT["fp4", km]] * 2
        (n1, a1), (n2, a2) = seen
        del seen[:]
        assert n1 == "linear_fp4" and a1[2:] == (m.w_codes, m.w_scales, m.bias, gate, res, 136) and a1[0].dim() == (3 if km else 2)
        assert n2 == "linear_fp4_gelu_dual" and a2[2:] == (f.w_codes, f.w_scales, f.bias, False, 128)
        a, sa = a1[:2]
        m.forward_operands(a, sa, gate, res)
        f.forward_operands(a, sa)
        assert rec.take() == [] and [n for n, _ in seen] == ["linear_fp4", "linear_fp4_gelu_dual"]
        assert seen[0][1] == (a, sa, m.w_codes, m.w_scales, m.bias, gate, res, 136) and seen[1][1] == (a, sa, f.w_codes, f.w_scales, f.bias, False, 128)
        del seen[:]


# ---- two rules broken at once: the earlier one answers ----------------------------------------------------------------------------
def _refusals():
    rm = {f: operands(f, False, T, 128) for f in FORMATS}
    im = {f: operands(f, True, T, 128) for f in FORMATS}
    rm3, im3 = {f: operands(f, False, T, 384) for f in FORMATS}, {f: operands(f, True, T, 384) for f in FORMATS}
    cache, bad_cache = fp16(2, B, MAX_LEN, H, C), torch.zeros(2, B, MAX_LEN, H, C)
    bad_gate, bad_res, bad_bias = fp16(3, 128), fp16(7, 128), fp16(100)
    short = lambda ops: (ops[0][:, :-32].contiguous(), *ops[1:])           # activation codes of another K
    mixed = lambda f: (im[f][0], im[f][1], rm[f][2], rm[f][3])
    w136 = lambda ops: operands("e2m1" if ops[0].shape[1] == G * 64 else "e3m0", False, T, 136)   # the same, with outs 136
    half_sw = lambda ops: (*ops[:3], ops[3].half())
    a, sa, w, sw = rm["e2m1"]
    cases = [   # (label, needs the GPU rule switched off, call, message)
        ("fp4: gpu < operands", False, lambda: gemm.linear_fp4(*mixed("e2m1")), "GPU"),
        ("fp4: operands < gate", True, lambda: gemm.linear_fp4(*short(rm["e2m1"]), None, bad_gate), "mismatch"),
        ("fp4: pair < image scales", True, lambda: gemm.linear_fp4(*mixed("e2m1")[:3], sw.half()), "both operands must be"),
        ("fp4: outs < scale image", True, lambda: gemm.linear_fp4(*half_sw(im["e2m1"]), outs=64), "does not belong"),
        ("fp4: gate < residual", True, lambda: gemm.linear_fp4(a, sa, w, sw, None, bad_gate, bad_res), "gate must be"),
        ("fp4 fc1: gpu < operands", False, lambda: gemm.linear_fp4_gelu_dual(*mixed("e2m1")), "GPU"),
        ("fp4 fc1: operands < outs", True, lambda: gemm.linear_fp4_gelu_dual(*short(w136(rm["e2m1"]))), "mismatch"),
        ("fp4 fc1: outs < bias", True, lambda: gemm.linear_fp4_gelu_dual(*w136(rm["e2m1"]), bad_bias), "multiple of 128"),
        ("fp4 fc1 km: outs < bias", True, lambda: gemm.linear_fp4_gelu_dual(*im["e2m1"], bad_bias, outs=120), "multiple of 128"),
        ("fp4 qkv: gpu < cache", False, lambda: gemm.linear_fp4_qkv_to_cache(*rm3["e2m1"], None, bad_cache, 0, SEQ), "GPU"),
        ("fp4 qkv: cache < operands", True, lambda: gemm.linear_fp4_qkv_to_cache(*short(rm3["e2m1"]), None, bad_cache, 0, SEQ), "contiguous float16"),
        ("fp4 qkv: operands < fit", True, lambda: gemm.linear_fp4_qkv_to_cache(*short(rm3["e2m1"]), None, cache, 14, SEQ), "mismatch"),
        ("fp4 qkv km: operands < fit", True, lambda: gemm.linear_fp4_qkv_to_cache(*half_sw(im3["e2m1"]), None, cache, 14, SEQ), "scale image"),
        ("fp4 qkv: fit < head scale", True, lambda: gemm.linear_fp4_qkv_to_cache(*rm3["e2m1"], None, cache, 14, SEQ, torch.ones(3)), "do not fit"),
        ("fp4 qkv: head scale < bias", True, lambda: gemm.linear_fp4_qkv_to_cache(*rm3["e2m1"], fp16(384), cache, 0, SEQ, torch.ones(3)), "qk_norm_scale must be"),
        ("fp6 qkv: table < cache", True, lambda: gemm.linear_fp6_qkv_to_cache(a, sa, w, sw, None, bad_cache, 0, SEQ, a_table="e2m1"), "'e2m3' and 'e3m2'"),
        ("fp6 qkv: cache < operands", True, lambda: gemm.linear_fp6_qkv_to_cache(a, sa, w, sw, None, bad_cache, 0, SEQ), "contiguous float16"),
        ("mx: gpu < dtype", False, lambda: gemm.quantize_mx(torch.zeros(2, 100, dtype=torch.bfloat16)), "GPU"),
        ("mx: dtype < width", True, lambda: gemm.quantize_mx(torch.zeros(2, 100, dtype=torch.bfloat16)), "float16 or float32"),
        ("g6: gpu < dtype", False, lambda: gemm.quantize_g6(torch.zeros(2, 100, dtype=torch.bfloat16), "e2m1"), "GPU"),
        ("g6: dtype < table", True, lambda: gemm.quantize_g6(torch.zeros(2, 100, dtype=torch.bfloat16), "e2m1"), "float16 or float32"),
        ("g6: table < width", True, lambda: gemm.quantize_g6(torch.zeros(2, 100), "e2m1"), "'e1m2' and 'e3m0'"),
    ]
    for f in ("e1m2", "e3m0"):
        ra, rsa, rw, rsw = rm[f]
        ia, isa, iw, isw = im[f]
        for name, fn, ops, wrong_rank in (("a6w4", gemm.linear_a6w4, rm[f], "row-major operands only"),
                                          ("a6w4 km", gemm.linear_a6w4_km, im[f], "k-major images")):
            o = lambda ops, *rest: (ops[0], ops[1], f, ops[2], ops[3], *rest)
            bad = short(ops) if fn is gemm.linear_a6w4 else (ops[0][:, :, :64], *ops[1:])
            bad_msg = "mismatch" if fn is gemm.linear_a6w4 else "k-major images must be"
            other = im[f] if fn is gemm.linear_a6w4 else rm[f]
            cases += [
                (f"{name} {f}: gpu < table", False, lambda fn=fn, ops=ops: fn(ops[0], ops[1], "e2m1", ops[2], ops[3]), "GPU"),
                (f"{name} {f}: table < rank", True, lambda fn=fn, other=other: fn(other[0], other[1], "e2m1", other[2], other[3]), "'e1m2' and 'e3m0'"),
                (f"{name} {f}: rank < shapes", True, lambda fn=fn, o=o, other=other, ops=ops: fn(*o((other[0], ops[1][:1], ops[2], ops[3]))), wrong_rank),
                (f"{name} {f}: operands < gate", True, lambda fn=fn, o=o, bad=bad: fn(*o(bad, None, bad_gate)), bad_msg),
                (f"{name} {f}: gate < residual", True, lambda fn=fn, o=o, ops=ops: fn(*o(ops, None, bad_gate, bad_res)), "gate must be"),
                (f"{name} {f}: residual < bias", True, lambda fn=fn, o=o, ops=ops: fn(*o(ops, bad_bias, None, bad_res), *((128,) if fn is gemm.linear_a6w4_km else ())),
                 "residual must be"),
            ]
        cases += [
            (f"a6w4 fc1 {f}: gpu < table", False, lambda ra=ra, rsa=rsa, rw=rw, rsw=rsw: gemm.linear_a6w4_gelu_dual(ra, rsa, "e2m1", rw, rsw), "GPU"),
            (f"a6w4 fc1 {f}: table < rank", True, lambda ia=ia, isa=isa, iw=iw, isw=isw: gemm.linear_a6w4_gelu_dual(ia, isa, "e2m1", iw, isw), "'e1m2' and 'e3m0'"),
            (f"a6w4 fc1 {f}: operands < outs", True, lambda f=f: (lambda o: gemm.linear_a6w4_gelu_dual(o[0], o[1], f, o[2], o[3]))(short(w136(rm[f]))), "mismatch"),
            (f"a6w4 fc1 {f}: outs < bias", True, lambda f=f: (lambda o: gemm.linear_a6w4_gelu_dual(o[0], o[1], f, o[2], o[3], bad_bias))(w136(rm[f])), "multiple of 128"),
            (f"a6w4 fc1 km {f}: gpu < table", False, lambda ia=ia, isa=isa, iw=iw, isw=isw: gemm.linear_a6w4_gelu_dual_km(ia, isa, "e2m1", iw, isw), "GPU"),
            (f"a6w4 fc1 km {f}: table < rank", True, lambda ra=ra, rsa=rsa, rw=rw, rsw=rsw: gemm.linear_a6w4_gelu_dual_km(ra, rsa, "e2m1", rw, rsw), "'e1m2' and 'e3m0'"),
            (f"a6w4 fc1 km {f}: operands < outs", True, lambda ia=ia, isa=isa, iw=iw, isw=isw, f=f: gemm.linear_a6w4_gelu_dual_km(ia, isa.half(), f, iw, isw, outs=120), "scale image"),
            (f"a6w4 fc1 km {f}: outs < bias", True, lambda ia=ia, isa=isa, iw=iw, isw=isw, f=f: gemm.linear_a6w4_gelu_dual_km(ia, isa, f, iw, isw, bad_bias, outs=120), "multiple of 128"),
        ]
        q = lambda ops, table, *rest: gemm.linear_a6w4_qkv_to_cache(ops[0], ops[1], table, ops[2], ops[3], *rest)
        cases += [
            (f"a6w4 qkv {f}: gpu < table", False, lambda f=f, q=q: q(rm3[f], "e2m1", None, cache, 0, SEQ), "GPU"),
            (f"a6w4 qkv {f}: table < cache", True, lambda f=f, q=q: q(rm3[f], "e2m1", None, bad_cache, 0, SEQ), "'e1m2' and 'e3m0'"),
            (f"a6w4 qkv {f}: cache < operands", True, lambda f=f, q=q: q(short(rm3[f]), f, None, bad_cache, 0, SEQ), "contiguous float16"),
            (f"a6w4 qkv {f}: cache < rank", True, lambda f=f, q=q: q((im3[f][0], *rm3[f][1:]), f, None, bad_cache, 0, SEQ), "contiguous float16"),
            (f"a6w4 qkv {f}: operands < weight scales", True, lambda f=f, q=q: q(half_sw(short(rm3[f])), f, None, cache, 0, SEQ), "mismatch"),
            (f"a6w4 qkv km {f}: operands < weight scales", True, lambda f=f, q=q: q(half_sw(im3[f]), f, None, cache, 0, SEQ), "scale image"),
            (f"a6w4 qkv {f}: weight scales < fit", True, lambda f=f, q=q: q(half_sw(rm3[f]), f, None, cache, 14, SEQ), "weight scales must be float32"),
            (f"a6w4 qkv {f}: fit < head scale", True, lambda f=f, q=q: q(rm3[f], f, None, cache, 14, SEQ, torch.ones(3)), "do not fit"),
            (f"a6w4 qkv km {f}: the cache names outs, not the bias", True, lambda f=f, q=q: q(im3[f], f, fp16(330), cache, 0, SEQ), "bias must hold one value per output"),
        ]
    for cls in (gemm.FP4Linear, gemm.FP4LinearGeluDual):
        m = module(cls, "e3m0", True, 128)
        cases += [
            (f"{cls.__name__}: table < layout", True, lambda m=m: m.forward_operands(*rm["e3m0"][:2], table="e2m3"), "'e1m2' and 'e3m0'"),
            (f"{cls.__name__}: layout < operands", True, lambda m=m: m.forward_operands(rm["e3m0"][0], rm["e3m0"][1][:1]),
             cls.__name__ + r"\.forward_operands: the weight is a k-major image - 6-bit activation codes must\s+come as the k-major images"),
        ]
    return cases


_REFUSALS = _refusals()


@pytest.mark.parametrize("case", range(len(_REFUSALS)), ids=[c[0] for c in _REFUSALS])
def test_the_earlier_rule_answers(case, monkeypatch):
    _, no_gpu_rule, call, message = _REFUSALS[case]
    monkeypatch.setattr(gemm, "_native", None)
    if no_gpu_rule:
        monkeypatch.setattr(gemm, "require_gpu", lambda *a, **k: None)
    class NoLibrary:
        def __getattr__(self, name):
            raise AssertionError(f"{name} was reached")
    monkeypatch.setattr(gemm, "lib", lambda: NoLibrary())
    with pytest.raises(RuntimeError, match=message):
        call()
