"""Packed weights straight into matrix-core operands (include/fpq.h, PACKED WEIGHTS <-> WEIGHT OPERANDS; packed.PackedWeight.operands /
from_operands, the modules' from_packed / to_packed, from_float with an attached packed weight, state_dicts across layouts).

Shapes: outs 8 / 72 / 136 = a partial 64-row block, one block and a partial one, two and a partial one - rows with bit 3 set (the
6-bit chunk rotation) and all four values of (row & 15) >> 2 (the 4-bit chunk permutation); k 128 / 384 = one and several planes.

(1) is byte equality with the quantizers from_float uses; (2) is the value contract and does not depend on them."""
import copy

import pytest
import torch

from fpqvar_amd import _lib, gemm, packed as pk, quant_linear as ql

pytestmark = pytest.mark.gpu

FP4, FP6 = pk.FP4_TABLES, pk.FP6_TABLES
OUTS, KS = (8, 72, 136), (128, 384)
CASES = [(t, "group") for t in FP4 + FP6] + [(t, "channel") for t in FP6]


def _dev():
    return torch.device("cuda:0")


def _weight(outs, k, seed=0):
    g = torch.Generator().manual_seed(1000 * outs + k + seed)
    return (torch.randn(outs, k, generator=g) * 0.05).to(_dev())


def _quantizer(table, mode, w):
    """the codes and scales of the quantizer from_float uses for this format"""
    if mode == "channel":
        return gemm.quantize_fp6(w, table=table)
    if table == "e2m1":
        return gemm.quantize_mx(w)
    return gemm.quantize_g6(w, table) if table in FP4 else gemm.quantize_gf6(w, table)


def _decode(table, mode, codes, scales):
    if mode == "channel":
        return gemm.dequantize_fp6(codes, scales, table)
    if table == "e2m1":
        return gemm.dequantize_mx(codes, scales)
    return gemm.dequantize_g6(codes, scales, table) if table in FP4 else gemm.dequantize_gf6(codes, scales, table)


def _raw_operands(p, kmajor):
    """fpq_packed_to_operands into buffers prefilled with 0xFF: whatever is still 0xFF afterwards, the launch did not write"""
    outs, k = p.shape
    rows64, seg, grouped = (outs + 63) // 64 * 64, 64 if p.table == "e2m1" else 96, p.cols == 128
    w_codes = torch.full((k // 128, rows64, seg) if kmajor else (outs, k // 128 * seg), 0xFF, dtype=torch.uint8, device=_dev())
    w_scales = torch.full((k // 128, rows64) if kmajor else (outs, k // 128), float("nan"), dtype=torch.float32, device=_dev())
    w_scales.view(torch.int32).fill_(-1)
    rc = _lib.lib().fpq_packed_to_operands(p.codes.data_ptr(), p.scales.data_ptr() if grouped else None, _lib.dtype_id(p.scales.dtype),
                                           w_codes.data_ptr(), w_scales.data_ptr() if grouped else None, outs, k, p.cols,
                                           _lib.TABLE_IDS[p.table], int(kmajor), _lib.stream_ptr(_dev()))
    assert rc == 0
    return w_codes, w_scales if grouped else None


def _pad64(t):
    rows64 = (t.shape[0] + 63) // 64 * 64
    return torch.cat([t, t.new_zeros(rows64 - t.shape[0], *t.shape[1:])])


def _bits(t):
    return t.contiguous().view(torch.int32 if t.dtype == torch.float32 else torch.int16)


@pytest.mark.parametrize("table,mode", CASES)
def test_operands_equal_the_quantizers_bytes(table, mode):
    """(1): row-major operands == the format's quantizer, k-major operands == to_kmajor(dealt) / to_kmajor_scales(weight_side) of
    them over the WHOLE image, and the launch writes every byte (0xFF prefill)."""
    for outs in OUTS:
        for k in KS:
            w = _weight(outs, k)
            p = pk.pack_weight(w, table, 128 if mode == "group" else k)
            codes, scales = _quantizer(table, mode, w)
            got_c, got_s = _raw_operands(p, False)
            differ = (got_c != codes).nonzero()
            assert differ.numel() == 0, f"{table} {mode} {outs}x{k}: first differing code byte at {differ[0].tolist()}"
            api_c, api_s = p.operands(False)
            assert torch.equal(api_c, got_c) and torch.equal(_bits(api_s).reshape(-1), _bits(scales.float()).reshape(-1))
            grouped = mode == "group" or k == 128      # rows of 128 in a weight 128 wide are both: the operand carries the scales
            scales = scales.reshape(outs, -1) if grouped else scales
            bits = 4 if table == "e2m1" else 6
            img_c, img_s = _raw_operands(p, True)
            assert torch.equal(img_c, gemm.to_kmajor(_pad64(codes), bits, dealt=True)), f"{table} {mode} {outs}x{k}: code image"
            km_c, km_s = p.operands(True)
            assert torch.equal(km_c, img_c)
            if grouped:
                assert torch.equal(_bits(got_s), _bits(scales))
                assert torch.equal(_bits(img_s), _bits(gemm.to_kmajor_scales(_pad64(scales), weight_side=True))), f"{table} {outs}x{k}: scale image"
                assert torch.equal(_bits(km_s), _bits(img_s))
            else:
                assert torch.equal(_bits(km_s), _bits(scales.float())) and km_s.shape == (outs,)


def _every_index(table, mode, outs=72, k=384):
    """a packed weight that holds every index of the table in every position class, an all-zero group (row 3, group 0) and fp16 scales"""
    n = 15 if table in FP4 else 63
    g = torch.Generator().manual_seed(5)
    idx = torch.randint(0, n, (outs, k), generator=g, dtype=torch.uint8)
    idx[0, :n] = torch.arange(n, dtype=torch.uint8)
    idx[9, k - n:] = torch.arange(n, dtype=torch.uint8).flip(0)
    idx[3, :128] = n // 2
    cols = 128 if mode == "group" else k
    scales = (torch.rand(outs * k // cols, generator=g) + 0.01).half()
    if mode == "group":
        scales[3 * (k // 128)] = 0.0
    codes = idx.view(outs, k // 2, 2) if table in FP4 else None
    codes = (codes[..., 0] | (codes[..., 1] << 4)) if table in FP4 else pk.pack6(idx)
    return pk.PackedWeight(codes.reshape(outs * k // cols, -1).to(_dev()), scales.to(_dev()), table, cols, (outs, k))


@pytest.mark.parametrize("table,mode", CASES)
def test_decoded_operands_equal_the_dequantized_weight(table, mode):
    """(2): the torch decoders of the hardware formats on the row-major operands == PackedWeight.dequantize(float32), bit for bit"""
    p = _every_index(table, mode)
    codes, scales = p.operands(False)
    want = p.dequantize(torch.float32)
    got = _decode(table, mode, codes, scales)
    assert got.dtype == want.dtype and torch.equal(_bits(got), _bits(want)), f"{table} {mode}: {(_bits(got) != _bits(want)).sum().item()} values differ"
    # the k-major image is the same operand: converting the row-major codes gives it
    assert torch.equal(p.operands(True)[0], gemm.to_kmajor(codes, 4 if table == "e2m1" else 6, dealt=True))


@pytest.mark.parametrize("table", FP4 + FP6)
def test_non_finite_groups_keep_their_scale(table):
    """a group whose maximum is inf or NaN: the scale's bits arrive, every code is a valid code (any nibble / field is: decoded finite)"""
    w = _weight(8, 256)
    w[1, 5], w[2, 200] = float("inf"), float("nan")
    p = pk.pack_weight(w, table, 128)
    codes, scales = p.operands(False)
    assert torch.equal(_bits(scales.reshape(-1)), _bits(p.scales.float()))
    assert bool(torch.isfinite(_decode(table, "group", codes, torch.ones_like(scales))).all())


@pytest.mark.parametrize("table,mode", CASES)
def test_round_trips(table, mode):
    """(3): from_operands(operands(km)) gives back the codes and the fp32-widened scales, in both layouts"""
    p = _every_index(table, mode, outs=136, k=384)
    for km in (False, True):
        back = pk.PackedWeight.from_operands(*p.operands(km), table, p.shape, p.cols)
        assert torch.equal(back.codes.reshape(-1), p.codes.reshape(-1)), (table, mode, km)
        assert torch.equal(_bits(back.scales.reshape(-1)), _bits(p.scales.float().reshape(-1))), (table, mode, km)
    # a negative zero code maps to the zero index
    outs, k = p.shape
    w_codes, w_scales = p.operands(False)
    neg_zero = torch.full_like(w_codes, 0x88) if table == "e2m1" else pk.pack6(torch.full((outs, k), 32, dtype=torch.uint8, device=_dev()))
    back = pk.PackedWeight.from_operands(neg_zero, w_scales, table, p.shape, p.cols)
    zero = 7 if table in FP4 else 31
    idx = torch.stack((back.codes & 15, back.codes >> 4), -1) if table in FP4 else pk.unpack6(back.codes)
    assert bool((idx == zero).all())


# (class, from_float keywords); every class and layout from_float accepts, the W6 forms and the two GeluDual classes included
MODULES = [
    ("FP4Linear", dict()), ("FP4Linear", dict(kmajor=True)), ("FP4Linear", dict(act_fp_type="fp_e3")),
    ("FP4Linear", dict(act_fp_type="fp_e1", kmajor=True, a6w4_kmajor=True)),
    ("FP4Linear", dict(weight_fp_type="fp_e1")), ("FP4Linear", dict(weight_fp_type="fp_e3", act_fp_type="fp_e3", w6_forms=True)),
    ("FP4Linear", dict(weight_fp_type="fp_e3", w6_forms=True, kmajor=True, w6_kmajor=True)),
    ("FP4LinearGeluDual", dict()), ("FP4LinearGeluDual", dict(kmajor=True)),
    ("FP4LinearGeluDual", dict(weight_fp_type="fp_e1", w6_forms=True)),
    ("FP4LinearGeluDual", dict(weight_fp_type="fp_e3", act_fp_type="fp_e1", w6_forms=True, kmajor=True, w6_kmajor=True)),
    ("FP6GroupLinear", dict(weight_fp_type="fp6_e2m3", act_fp_type="fp6_e2m3")),
    ("FP6GroupLinear", dict(weight_fp_type="fp6_e3m2", act_fp_type="fp6_e2m3", kmajor=True)),
    ("FP6GroupLinear", dict(weight_fp_type="fp_e2", act_fp_type="fp6_e3m2", kmajor=True)),
    ("FP6GroupLinear", dict(weight_fp_type="fp_e1", act_fp_type="fp6_e2m3")),
    ("FP6GroupLinearGeluDual", dict(weight_fp_type="fp6_e2m3", act_fp_type="fp6_e2m3")),
    ("FP6GroupLinearGeluDual", dict(weight_fp_type="fp6_e3m2", act_fp_type="fp6_e2m3", kmajor=True, fc2_fp_type="fp_e1m2_neg_e2m1_pos")),
    ("FP6Linear", dict()), ("FP6Linear", dict(kmajor=True, weight_fp_type="fp6_e3m2")),
    ("FP6Linear", dict(kmajor=True, act_fp_type="fp6_e3m2")),
]


def _same_buffers(a, b):
    assert type(a) is type(b)
    sa, sb = a.state_dict(), b.state_dict()
    assert sa.keys() == sb.keys()
    for key in sa:
        assert sa[key].dtype == sb[key].dtype and sa[key].shape == sb[key].shape and torch.equal(sa[key], sb[key]), key


@pytest.fixture(scope="module")
def lin():
    torch.manual_seed(3)
    return torch.nn.Linear(256, 384).to(_dev())


@pytest.fixture(scope="module")
def x():
    return torch.randn(24, 256, generator=torch.Generator().manual_seed(4)).half().to(_dev())


@pytest.mark.parametrize("cls_name,kw", MODULES, ids=[f"{c}-{i}" for i, (c, _) in enumerate(MODULES)])
def test_from_packed_equals_from_float(cls_name, kw, lin, x):
    """(4) and the second half of (3): equal buffers, equal output bits, and operands(to_packed()) returns the module's buffers"""
    cls = getattr(gemm, cls_name)
    ref = cls.from_float(lin, **kw)
    table = pk.TABLE_OF_FP_TYPE[kw.get("weight_fp_type", "fp6_e2m3" if cls_name == "FP6Linear" else "fp_e2")]
    cols = 256 if cls_name == "FP6Linear" else 128
    p = pk.pack_weight(lin.weight, table, cols, bias=lin.bias)
    got = cls.from_packed(p, **{key: v for key, v in kw.items() if key != "weight_fp_type"})
    _same_buffers(got, ref)
    assert torch.equal(got(x), ref(x))
    # the same through from_float on a Linear whose weight is gone
    hollow = copy.deepcopy(lin)
    hollow.weight.data.zero_()
    hollow.packed_weight = p
    _same_buffers(cls.from_float(hollow, **kw), ref)
    back = ref.to_packed()
    w_codes, w_scales = back.operands(ref.kmajor)
    assert torch.equal(w_codes, ref.w_codes) and torch.equal(_bits(w_scales), _bits(ref.w_scales))
    assert back.table == table and back.cols == cols and torch.equal(back.bias, ref.bias)


@pytest.mark.parametrize("cls_name,kw_rm,kw_km", [
    ("FP4Linear", dict(), dict(kmajor=True)),
    ("FP4Linear", dict(weight_fp_type="fp_e3", w6_forms=True), dict(weight_fp_type="fp_e3", w6_forms=True, kmajor=True, w6_kmajor=True)),
    ("FP4LinearGeluDual", dict(), dict(kmajor=True)),
    ("FP6GroupLinear", dict(weight_fp_type="fp6_e3m2"), dict(weight_fp_type="fp6_e3m2", kmajor=True)),
    ("FP6GroupLinearGeluDual", dict(), dict(kmajor=True)),
    ("FP6Linear", dict(), dict(kmajor=True))])
def test_state_dict_crosses_layouts(cls_name, kw_rm, kw_km, lin):
    """(6): a row-major module's state_dict loads into its k-major twin and back; the result equals the twin built directly"""
    cls = getattr(gemm, cls_name)
    rm, km = cls.from_float(lin, **kw_rm), cls.from_float(lin, **kw_km)
    other = torch.nn.Linear(256, 384).to(_dev())
    into_km, into_rm = cls.from_float(other, **kw_km), cls.from_float(other, **kw_rm)
    into_km.load_state_dict(rm.state_dict())
    _same_buffers(into_km, km)
    into_rm.load_state_dict(km.state_dict())
    _same_buffers(into_rm, rm)
    into_rm.load_state_dict(rm.state_dict())      # equal ranks load as before
    _same_buffers(into_rm, rm)
    with pytest.raises(RuntimeError, match="size mismatch"):   # on the CPU nothing converts
        copy.deepcopy(km).cpu().load_state_dict({key: v.cpu() for key, v in rm.state_dict().items()})


# ---- (5) a model from a packed file -----------------------------------------------------------------------------------
class FFN(torch.nn.Module):
    def __init__(self):
        super().__init__()
        self.fc1, self.act, self.fc2 = torch.nn.Linear(256, 1024), torch.nn.GELU(approximate="tanh"), torch.nn.Linear(1024, 256)

    def forward(self, x):
        return self.fc2(self.act(self.fc1(x)))


class Attn(torch.nn.Module):
    def __init__(self):
        super().__init__()
        self.mat_qkv, self.proj = torch.nn.Linear(256, 768), torch.nn.Linear(256, 256)

    def forward(self, x):
        return self.proj(self.mat_qkv(x)[..., :256])


class Block(torch.nn.Module):
    def __init__(self):
        super().__init__()
        self.attn, self.ffn = Attn(), FFN()


class Toy(torch.nn.Module):
    def __init__(self):
        super().__init__()
        self.blocks = torch.nn.ModuleList([Block(), Block()])


_G4 = dict(weight_quant="per_group", act_quant="per_group", w_bit=4, a_bit=4, act_quant_sym=True, activation_fp_quant=True,
           weight_fp_quant=True)
_C6 = dict(weight_quant="per_channel", act_quant="per_token", w_bit=6, a_bit=6, act_quant_sym=True, activation_fp_quant=True,
           weight_fp_quant=True)
_W4A4 = dict(_G4, act_fp_type="fp_e2", weight_fp_type="fp_e2", fc2_fp_type="fp_e1m2_neg_e2m1_pos", real_fp4=True, fuse_ffn=True)


def _mixed_formats(b, layer):   # fp_e1 and fp_e3 weights on fc1 / mat_qkv / proj, fc2 the dual format on an fp_e2 weight
    if layer == "fc2":
        return ("fp_e1m2_neg_e2m1_pos", "fp_e2")
    return ("fp_e2" if layer == "fc1" else "fp_e3", "fp_e1" if (b + (layer == "proj")) % 2 == 0 else "fp_e3")


def _mixed_layer_format(name, linear):
    parts = name.split(".")
    return pk.TABLE_OF_FP_TYPE[_mixed_formats(int(parts[1]), parts[-1])[1]], 128


MODELS = {
    "w4a4_kmajor": (ql.quantize_VAR, (), _W4A4, None),
    "w4a4_rowmajor": (ql.quantize_VAR, (), dict(_W4A4, kmajor_operands=False), None),
    "w6a6": (ql.quantize_VAR, (), dict(_C6, act_fp_type="fp6_e2m3", weight_fp_type="fp6_e2m3", fc2_fp_type="fp6_int_neg_e2m3_pos",
                                       real_fp6=True), None),
    "w6a6_packed_e3m2": (ql.quantize_VAR, (), dict(_C6, act_fp_type="fp6_e2m3", weight_fp_type="fp6_e3m2",
                                                   fc2_fp_type="fp6_int_neg_e2m3_pos", real_fp6=True, packed_e3m2=True), None),
    "group_fp6": (ql.quantize_VAR, (), dict(_G4, w_bit=6, a_bit=6, act_fp_type="fp6_e2m3", weight_fp_type="fp6_e3m2",
                                            fc2_fp_type="fp6_int_neg_e2m3_pos", group_fp6=True), None),
    "mixed_w6": (ql.quantize_VAR_mixed, (_mixed_formats,), dict(_G4, real_fp4=True, fuse_ffn=True, w6_weights=True, w6_forms=True,
                                                                 w6_kmajor=True), _mixed_layer_format),
}


@pytest.mark.parametrize("name", list(MODELS))
def test_model_from_a_packed_file(name, tmp_path):
    fn, args, cfg, layer_format = MODELS[name]
    torch.manual_seed(21)
    base = Toy().to(_dev())
    if layer_format is None:
        layer_format = pk.var_layer_format(cfg["weight_quant"], cfg["weight_fp_type"], cfg["w_bit"])
    layers = pk.calibrate_packed(base, layer_format)
    assert sorted(layers) == sorted(n for n, m in base.named_modules() if isinstance(m, torch.nn.Linear))
    path = str(tmp_path / "toy.safetensors")
    pk.save_packed(path, layers)
    skeleton = copy.deepcopy(base)
    for m in skeleton.modules():
        if isinstance(m, torch.nn.Linear):
            m.weight.data.zero_()
    pk.attach(skeleton, pk.load_packed(path, _dev()))
    got, want = fn(skeleton, *args, **cfg), fn(copy.deepcopy(base), *args, **cfg)
    x = torch.randn(24, 256, generator=torch.Generator().manual_seed(22)).half().to(_dev())
    native = 0
    for (n1, m1), (n2, m2) in zip(got.named_modules(), want.named_modules()):
        assert n1 == n2 and type(m1) is type(m2), (n1, type(m1), type(m2))
        if isinstance(m1, (gemm._ScaledOperandModule, ql.QuantizedLinear)):
            native += isinstance(m1, gemm._ScaledOperandModule)
            for (k1, b1), (k2, b2) in zip(m1.state_dict().items(), m2.state_dict().items()):
                assert k1 == k2 and b1.dtype == b2.dtype and torch.equal(b1, b2), (n1, k1)
    assert native == 6, native     # fc1, mat_qkv and proj of both blocks run on the matrix cores
    got, want = got.half(), want.half()
    for b1, b2 in zip(got.blocks, want.blocks):
        assert torch.equal(b1.ffn(x), b2.ffn(x))
        q1, q2 = b1.attn.mat_qkv(x), b2.attn.mat_qkv(x)
        assert torch.equal(q1, q2) and torch.equal(b1.attn.proj(x), b2.attn.proj(x))
