"""Host-side mirror of the reference's quantized Linear wrappers.

``QuantizedLinear`` / ``QuantizedLinear_fc2`` / ``quantize_VAR`` keep the reference's
constructor arguments, string flags and dispatch
(models_fp_quant_transform_rotate/quant_utils.py:649-867, 870-1092, 1095-1167):
activations are fake-quantized on every forward, weights once in ``from_float``;
``forward`` is ``F.linear(act_quant(x), W, b)``.

Only the floating-point formats are wired up (``activation_fp_quant`` /
``weight_fp_quant`` = True): the INT / log2 RTN baselines of the reference are single
fused torch ops already and are out of scope here; asking
for them raises ``NotImplementedError``.
"""
from __future__ import annotations

from functools import partial

import torch
from torch import nn

from . import quant_utils as qu

_GROUP = 128   # hard-coded in every partial(...) of the reference (tr/quant_utils.py:727-735)


def _act_quantizer(act_quant, activation_fp_quant, act_fp_type, a_bit, fc2: bool):
    """tr/quant_utils.py:696-746 (QuantizedLinear) and :917-973 (QuantizedLinear_fc2)."""
    if act_quant not in ("per_token", "per_tensor", "per_group"):
        raise ValueError(f"Invalid act_quant: {act_quant}")
    if not activation_fp_quant or act_quant == "per_tensor":
        raise NotImplementedError("INT / log2 activation quantizers are out of scope (SURVEY.md section 2 row 4)")
    if act_quant == "per_token":
        table = {"fp_e1": qu.fp_quant_e1_per_token, "fp_e2": qu.fp_quant_e2_per_token,
                 "fp_e3": qu.fp_quant_e3_per_token, "fp6_e2m3": qu.fp6_quant_e2m3_per_token_cuda,
                 "fp6_e3m2": qu.fp6_quant_e3m2_per_token_cuda}
        if fc2:
            table["fp6_int_neg_e2m3_pos"] = qu.fp6_quant_int_neg_e2m3_pos_per_token_cuda
        if act_fp_type not in table:
            raise ValueError("Unsupported fp_type.")
        return partial(table[act_fp_type], n_bits=a_bit)
    table = {"fp_e1": qu.fp_quant_e1_per_group_cuda, "fp_e2": qu.fp_quant_e2_per_group_cuda,
             "fp_e3": qu.fp_quant_e3_per_group_cuda, "fp6_e2m3": qu.fp6_quant_e2m3_per_group_cuda,
             "fp6_e3m2": qu.fp6_quant_e3m2_per_group_cuda}
    if fc2:
        table["fp_e1m2_neg_e2m1_pos"] = qu.fp_quant_e1m2_neg_e2m1_pos_per_group_cuda
        table["fp6_int_neg_e2m3_pos"] = qu.fp6_quant_int_neg_e2m3_pos_per_group_cuda
        table["fp4_afpq"] = qu.fp4_afpq_per_group_cuda          # models_fp_quant/quant_utils.py:1040-1041
    if act_fp_type not in table:
        raise ValueError("Unsupported fp_type.")
    return partial(table[act_fp_type], n_bits=a_bit, group_size=_GROUP)


def _quantize_weight(w, weight_quant, weight_fp_quant, weight_fp_type, w_bit):
    """tr/quant_utils.py:794-855.  per_channel FP4 goes through the pure-torch (argmin)
    functions exactly as in the reference; per_group through the `_cuda` ones."""
    if weight_quant == "per_tensor" or not weight_fp_quant:
        raise NotImplementedError("INT weight quantizers are out of scope (SURVEY.md section 2 row 4)")
    if weight_quant == "per_channel":
        table = {"fp_e1": qu.fp_quant_e1_per_token, "fp_e2": qu.fp_quant_e2_per_token,
                 "fp_e3": qu.fp_quant_e3_per_token, "fp6_e2m3": qu.fp6_quant_e2m3_per_token_cuda,
                 "fp6_e3m2": qu.fp6_quant_e3m2_per_token_cuda}
        if weight_fp_type not in table:
            raise ValueError("Unsupported fp_type.")
        return table[weight_fp_type](w, n_bits=w_bit)
    if weight_quant == "per_group":
        table = {"fp_e1": qu.fp_quant_e1_per_group_cuda, "fp_e2": qu.fp_quant_e2_per_group_cuda,
                 "fp_e3": qu.fp_quant_e3_per_group_cuda, "fp6_e2m3": qu.fp6_quant_e2m3_per_group_cuda,
                 "fp6_e3m2": qu.fp6_quant_e3m2_per_group_cuda}
        if weight_fp_type not in table:
            raise ValueError("Unsupported fp_type.")
        return table[weight_fp_type](w, n_bits=w_bit, group_size=_GROUP)
    raise ValueError(f"Invalid weight_quant: {weight_quant}")


def _packed_weight(cls_name, module, packed, weight_quant, weight_fp_quant, weight_fp_type, w_bit):
    """What _quantize_weight returns, from the packed.PackedWeight attached to `module` (packed.attach): its de-quantized tensor,
    bit-equal to the quantizer's output on the weight it was calibrated from.  The packed format must be the one the arguments
    ask for."""
    from .packed import FP4_TABLES, TABLE_OF_FP_TYPE
    if not weight_fp_quant or weight_quant not in ("per_channel", "per_group"):
        raise NotImplementedError("INT weight quantizers are out of scope (SURVEY.md section 2 row 4)")
    table = TABLE_OF_FP_TYPE.get(weight_fp_type)
    if table is None:
        raise ValueError("Unsupported fp_type.")
    cols = _GROUP if weight_quant == "per_group" else module.in_features
    if (packed.table != table or packed.cols != cols or w_bit != (4 if table in FP4_TABLES else 6)
            or tuple(packed.shape) != (module.out_features, module.in_features)):
        raise ValueError(f"{cls_name}.from_float: the attached packed weight is {packed.table} {tuple(packed.shape)} in rows of "
                         f"{packed.cols}, the layer asks for {table} ({w_bit} bits) {(module.out_features, module.in_features)} in rows of {cols}")
    # the reference's FP6 quantizers return float16 whatever they are given (`.to(torch.float16)`), its FP4 ones the input's dtype -
    # which calibrate_packed recorded as the packed weight's out_dtype
    return packed.dequantize(None if table in FP4_TABLES else torch.float16)


class GeluThenFc2Quant(nn.Module):
    """Stands in for an FFN's `act` (GELU, approximate="tanh") when fc2's dual-format input quantizer is fused behind it:
    `forward(y)` = `fc2.act_quant(F.gelu(y, approximate="tanh"))` in ONE pass over the fc1 output (quant_utils.gelu_*), for the
    FFN.forward of the reference (`self.fc2(self.act(self.fc1(x)))`, tr/basic_var.py:120-121) - fc2's own input quantizer is
    switched off by quantize_VAR(..., fuse_ffn=True)."""
    FUSED = {("per_group", "fp_e1m2_neg_e2m1_pos"): lambda y, bits: qu.gelu_fp_quant_e1m2_neg_e2m1_pos_per_group_cuda(y, bits, _GROUP),
             ("per_group", "fp4_afpq"): lambda y, bits: qu.gelu_fp4_afpq_per_group_cuda(y, bits, _GROUP),
             ("per_group", "fp6_int_neg_e2m3_pos"): lambda y, bits: qu.gelu_fp6_quant_int_neg_e2m3_pos_per_group_cuda(y, bits, _GROUP),
             ("per_token", "fp6_int_neg_e2m3_pos"): lambda y, bits: qu.gelu_fp6_quant_int_neg_e2m3_pos_per_token_cuda(y, bits)}

    def __init__(self, act_quant: str, fc2_fp_type: str, a_bit: int):
        super().__init__()
        self.act_quant, self.fc2_fp_type, self.a_bit = act_quant, fc2_fp_type, a_bit
        self.fn = self.FUSED[(act_quant, fc2_fp_type)]

    @torch.no_grad()
    def forward(self, y):
        return self.fn(y.to(torch.float16), self.a_bit)

    def extra_repr(self):
        return f"GELU(tanh) + {self.fc2_fp_type} {self.act_quant} (one pass)"


class QuantizedLinear(nn.Module):
    _FC2 = False

    def __init__(self, in_features, out_features, bias=True, act_quant=None, quantize_output=False,
                 w_bit=8, a_bit=8, act_quant_sym=True, fc2_act_log2_quant=False, activation_fp_quant=False,
                 weight_fp_quant=False, act_fp_type=False, weight_fp_type=False):
        super().__init__()
        self.in_features = in_features
        self.out_features = out_features
        self.w_bit = w_bit
        self.a_bit = a_bit
        self.act_quant_sym = act_quant_sym
        self.fc2_act_log2_quant = fc2_act_log2_quant
        self.activation_fp_quant = activation_fp_quant
        self.weight_fp_quant = weight_fp_quant
        self.act_fp_type = act_fp_type
        self.register_buffer("weight", torch.randn(out_features, in_features, dtype=torch.float16))
        if bias:
            self.register_buffer("bias", torch.zeros((1, out_features), dtype=torch.float16))
        else:
            self.register_buffer("bias", None)
        self.act_quant_name = act_quant
        self.act_quant = _act_quantizer(act_quant, activation_fp_quant, act_fp_type, a_bit, self._FC2)
        if quantize_output:
            self.output_quant_name = self.act_quant_name
            self.output_quant = self.act_quant
        else:
            self.output_quant_name = "None"
            self.output_quant = lambda x: x
        self.weight_quant_name = None

    def to(self, *args, **kwargs):
        super().to(*args, **kwargs)
        self.weight = self.weight.to(*args, **kwargs)
        if self.bias is not None:
            self.bias = self.bias.to(*args, **kwargs)
        return self

    @torch.no_grad()
    def forward(self, x):
        q_x = self.act_quant(x)
        y = torch.functional.F.linear(q_x, self.weight, self.bias)
        return self.output_quant(y)

    @classmethod
    def from_float(cls, module, weight_quant="per_channel", act_quant="per_token", quantize_output=False,
                   w_bit=8, a_bit=8, act_quant_sym=None, fc2_act_log2_quant=False, activation_fp_quant=False,
                   weight_fp_quant=False, act_fp_type=None, weight_fp_type=None):
        assert isinstance(module, torch.nn.Linear)
        new = cls(module.in_features, module.out_features, module.bias is not None, act_quant=act_quant,
                  quantize_output=quantize_output, w_bit=w_bit, a_bit=a_bit, act_quant_sym=act_quant_sym,
                  fc2_act_log2_quant=fc2_act_log2_quant, activation_fp_quant=activation_fp_quant,
                  weight_fp_quant=weight_fp_quant, act_fp_type=act_fp_type, weight_fp_type=weight_fp_type)
        packed = getattr(module, "packed_weight", None)
        if packed is None:
            new.weight = _quantize_weight(module.weight.detach(), weight_quant, weight_fp_quant, weight_fp_type, w_bit)
        else:   # packed.attach: the fake-quantized weight is the packed one's, module.weight is not read
            new.weight = _packed_weight(cls.__name__, module, packed, weight_quant, weight_fp_quant, weight_fp_type, w_bit)
        new.weight_quant_name = weight_quant
        if module.bias is not None:
            new.bias = module.bias
        return new

    def __repr__(self):
        return (f"{type(self).__name__}{self.in_features}, {self.out_features}, bias={self.bias is not None}, "
                f"weight_quant={self.weight_quant_name}, act_quant={self.act_quant_name}, "
                f"output_quant={self.output_quant_name}, w_bit={self.w_bit}, a_bit={self.a_bit}, "
                f"act_quant_sym={self.act_quant_sym}, act_log2_quant={self.fc2_act_log2_quant},"
                f"activation_fp_quant={self.activation_fp_quant}, weight_fp_quant={self.weight_fp_quant}, "
                f"activation_quant_type={self.act_fp_type}")


class QuantizedLinear_fc2(QuantizedLinear):
    """The fc2 variant accepts the asymmetric dual formats for its (post-GELU) input
    (tr/quant_utils.py:917-973)."""
    _FC2 = True


def quantize_VAR(model, weight_quant=None, act_quant=None, quantize_bmm_input=False, w_bit=8, a_bit=8, kv_bit=8,
                 act_quant_sym=None, fc2_act_log2_quant=None, quant_kv=None, activation_fp_quant=False,
                 weight_fp_quant=False, act_fp_type=None, weight_fp_type=None, fc2_fp_type=None, real_fp4=False,
                 real_fp6=False, fuse_ffn=False, kmajor_operands=True, packed_e3m2=False, group_fp6=False):
    """tr/quant_utils.py:1095-1167.  The reference matches its own FFN / SelfAttention
    classes; here a module with Linear children ``fc1``+``fc2`` is an FFN and one with
    ``mat_qkv``+``proj`` is a self-attention block.  As in the reference,
    ``quantize_bmm_input``, ``kv_bit`` and ``quant_kv`` are accepted and ignored, the
    ada_lin Linears stay in full precision, and fc2's input format is ``fc2_fp_type``.

    ``real_fp4`` (additive, default off = the reference's behaviour): in the W4A4 per-group ``fp_e2`` configuration
    fc1 / mat_qkv / proj become ``gemm.FP4Linear`` - same quantization decisions, product on the FP4 matrix cores
    instead of an fp16 GEMM on de-quantized tensors (fc2 keeps its dual-format fake quantization).

    ``fuse_ffn`` (additive; needs an FFN whose ``act`` is GELU(tanh) and a dual-format ``fc2_fp_type``): fc2's input quantizer
    moves in front of fc2 - the FFN's own ``forward`` (``fc2(act(fc1(x)))``, tr/basic_var.py:120-121) stays as it is.
    With ``real_fp4`` and ``fp_e1m2_neg_e2m1_pos``: fc1 becomes ``gemm.FP4LinearGeluDual`` (GELU and the quantizer in the fc1
    GEMM's epilogue) and ``act`` an identity; otherwise (the fake-quant default, ``real_fp6``, the FP6 / AFPQ dual pairs) ``act``
    becomes ``GeluThenFc2Quant`` - GELU and the quantizer in one pass over the fc1 output.  fc2 multiplies its already
    quantized input either way.

    ``kmajor_operands`` (with ``real_fp4`` / ``real_fp6``'s FP4 / FP6 Linears; default on): weights are held, and activations
    quantized, as k-major operand images (include/fpq.h) - the layout the GEMMs' LDS-DMA engine reads in contiguous 1 KiB
    pieces; results are bit-identical to the row-major form, the GEMMs 4 - 30 % faster.

    ``packed_e3m2`` (with ``real_fp6``; default off): a layer with an ``fp6_e3m2`` side becomes a ``gemm.FP6Linear`` of its format pair
    too - 6-bit packed BF6 operands on the FP6 GEMM - instead of a ``gemm.FP8Linear`` with one byte per code.

    ``group_fp6`` (additive, default off; needs weight_quant = act_quant = "per_group", bit widths 6 / 6, 4 / 6 or 6 / 4 and FP
    formats on both sides, else ValueError): fc1, mat_qkv and proj whose format pair has an ``fp6_e2m3`` / ``fp6_e3m2`` side (the
    other side any of ``fp6_e2m3``, ``fp6_e3m2``, ``fp_e1``, ``fp_e2``, ``fp_e3``) become ``gemm.FP6GroupLinear`` of that pair - full
    FP6 codes with per-group scales on the A6W4 / W6 GEMMs (``gemm.linear_g6``), k-major with ``kmajor_operands``.  The three pairs
    whose operands are both decoded as BF6 E3M2 with a full-range side (``gemm.GF6_REFUSED_PAIRS``) stay QuantizedLinear: the
    matrix core does not hold them inside the GEMM contract.  With ``fuse_ffn`` and ``fc2_fp_type`` ``fp6_int_neg_e2m3_pos`` or
    ``fp_e1m2_neg_e2m1_pos`` fc1 becomes ``gemm.FP6GroupLinearGeluDual`` (GELU and fc2's quantizer in the GEMM's epilogue) under the
    conditions of the ``real_fp4`` branch.  fc2 and ``ada_lin`` are as without it."""
    g6_ok = _group_fp6_ok(group_fp6, weight_quant, act_quant, w_bit, a_bit, activation_fp_quant, weight_fp_quant)
    fp4_ok = (real_fp4 and weight_quant == "per_group" and act_quant == "per_group" and w_bit == 4 and a_bit == 4
              and activation_fp_quant and weight_fp_quant and act_fp_type == "fp_e2" and weight_fp_type == "fp_e2")
    if real_fp4 and not fp4_ok:
        raise ValueError("real_fp4 needs weight_quant = act_quant = 'per_group', w_bit = a_bit = 4, fp_e2 on both sides")
    # ``real_fp6`` (additive, default off): in the W6A6 per_channel / per_token configuration (run.sh:7) fc1 / mat_qkv /
    # proj become ``gemm.FP8Linear`` - levels stored as E4M3 bytes, one scale per row, product on the FP8 matrix cores.
    fp6_ok = (real_fp6 and weight_quant == "per_channel" and act_quant == "per_token" and w_bit == 6 and a_bit == 6
              and activation_fp_quant and weight_fp_quant and act_fp_type in ("fp6_e2m3", "fp6_e3m2")
              and weight_fp_type in ("fp6_e2m3", "fp6_e3m2"))
    if real_fp6 and not fp6_ok:
        raise ValueError("real_fp6 needs weight_quant='per_channel', act_quant='per_token', w_bit = a_bit = 6, fp6 formats")
    common = dict(weight_quant=weight_quant, act_quant=act_quant, w_bit=w_bit, a_bit=a_bit,
                  activation_fp_quant=activation_fp_quant, weight_fp_quant=weight_fp_quant,
                  weight_fp_type=weight_fp_type)
    def plain(lin, **kw):
        if g6_ok and _group_fp6_pair(lin, act_fp_type, weight_fp_type):
            from .gemm import FP6GroupLinear
            return FP6GroupLinear.from_float(lin, weight_fp_type, act_fp_type, kmajor=kmajor_operands)
        if fp4_ok and lin.in_features % 128 == 0 and lin.out_features % 8 == 0:
            from .gemm import FP4Linear
            return FP4Linear.from_float(lin, kmajor=kmajor_operands)
        if fp6_ok and lin.in_features % 128 == 0 and lin.out_features % 8 == 0:
            from .gemm import FP6Linear, FP8Linear
            if weight_fp_type == "fp6_e2m3" and act_fp_type == "fp6_e2m3":
                return FP6Linear.from_float(lin, kmajor=kmajor_operands)   # 6-bit packed operands
            if packed_e3m2:   # ... of either format per side
                return FP6Linear.from_float(lin, kmajor=kmajor_operands, weight_fp_type=weight_fp_type, act_fp_type=act_fp_type)
            return FP8Linear.from_float(lin, weight_fp_type, act_fp_type)   # mixed / E3M2: E4M3-coded levels
        return QuantizedLinear.from_float(lin, **kw)

    for _, m in list(model.named_modules()):
        fc1, fc2 = getattr(m, "fc1", None), getattr(m, "fc2", None)
        qkv, proj = getattr(m, "mat_qkv", None), getattr(m, "proj", None)
        if isinstance(fc1, nn.Linear) and isinstance(fc2, nn.Linear):
            act = getattr(m, "act", None)
            gelu_tanh = isinstance(act, nn.GELU) and getattr(act, "approximate", "none") == "tanh"
            in_gemm = (fuse_ffn and gelu_tanh and fp4_ok and fc2_fp_type == "fp_e1m2_neg_e2m1_pos"
                       and fc1.in_features % 128 == 0 and fc1.out_features % 128 == 0)
            g6_tail = (fuse_ffn and gelu_tanh and g6_ok and fc2_fp_type in _GROUP_FP6_FC2
                       and _group_fp6_pair(fc1, act_fp_type, weight_fp_type, tail=True))
            in_gemm = in_gemm or g6_tail
            one_pass = (fuse_ffn and gelu_tanh and not in_gemm and activation_fp_quant and (act_quant, fc2_fp_type) in GeluThenFc2Quant.FUSED
                        and fc1.out_features % (128 if act_quant == "per_group" else 8) == 0)
            if fuse_ffn and not (in_gemm or one_pass):
                raise ValueError("fuse_ffn needs an FFN with act = GELU(approximate='tanh') and a dual-format fc2_fp_type "
                                 "(fp_e1m2_neg_e2m1_pos / fp4_afpq per group, fp6_int_neg_e2m3_pos per group or per token)")
            m.fc2 = QuantizedLinear_fc2.from_float(fc2, act_quant_sym=False, fc2_act_log2_quant=fc2_act_log2_quant,
                                                   act_fp_type=fc2_fp_type, **common)
            if in_gemm:
                from .gemm import FP4LinearGeluDual, FP6GroupLinearGeluDual
                if g6_tail:
                    m.fc1 = FP6GroupLinearGeluDual.from_float(fc1, weight_fp_type, act_fp_type, kmajor=kmajor_operands, fc2_fp_type=fc2_fp_type)
                else:
                    m.fc1 = FP4LinearGeluDual.from_float(fc1, kmajor=kmajor_operands)
                m.act = nn.Identity()
                m.fc2.act_quant = lambda t: t                      # its input arrives quantized from fc1's epilogue
                m.fc2.act_quant_name = "in fc1's epilogue"
            else:
                m.fc1 = plain(fc1, act_quant_sym=act_quant_sym, act_fp_type=act_fp_type, **common)
                if one_pass:
                    m.act = GeluThenFc2Quant(act_quant, fc2_fp_type, a_bit)
                    m.fc2.act_quant = lambda t: t                  # ... from the activation module in front of it
                    m.fc2.act_quant_name = "behind the GELU (one pass)"
        elif isinstance(qkv, nn.Linear) and isinstance(proj, nn.Linear):
            m.mat_qkv = plain(qkv, act_quant_sym=act_quant_sym, act_fp_type=act_fp_type, **common)
            m.proj = plain(proj, act_quant_sym=act_quant_sym, act_fp_type=act_fp_type, **common)
    return model


# ---- group_fp6: the per-group 6-bit configuration (and W4A6 / W6A4) on the matrix cores ---------------------------------------
_GROUP_FP6_FULL = ("fp6_e2m3", "fp6_e3m2")
_GROUP_FP6_FORMATS = _GROUP_FP6_FULL + ("fp_e1", "fp_e2", "fp_e3")
_GROUP_FP6_FC2 = ("fp6_int_neg_e2m3_pos", "fp_e1m2_neg_e2m1_pos")   # the fc2 formats of the GEMMs' fc1 tail (gemm._GF6_FC2_PAIRS)


def _group_fp6_ok(group_fp6, weight_quant, act_quant, w_bit, a_bit, activation_fp_quant, weight_fp_quant) -> bool:
    ok = (group_fp6 and weight_quant == "per_group" and act_quant == "per_group" and (w_bit, a_bit) in ((6, 6), (4, 6), (6, 4))
          and activation_fp_quant and weight_fp_quant)
    if group_fp6 and not ok:
        raise ValueError("group_fp6 needs weight_quant = act_quant = 'per_group', (w_bit, a_bit) = (6, 6), (4, 6) or (6, 4), "
                         "fp formats on both sides")
    return bool(ok)


def _group_fp6_pair(lin, a, w, tail: bool = False) -> bool:
    """the layer is one gemm.FP6GroupLinear runs: a per-group pair with at least one fp6 side that linear_g6 accepts, a shape the GEMM
    takes (tail: the fc1 form, whose output tile is one quantization group)"""
    from .gemm import GF6_REFUSED_PAIRS, _GF6_TABLES
    return (a in _GROUP_FP6_FORMATS and w in _GROUP_FP6_FORMATS and (a in _GROUP_FP6_FULL or w in _GROUP_FP6_FULL)
            and (_GF6_TABLES[a], _GF6_TABLES[w]) not in GF6_REFUSED_PAIRS
            and lin.in_features % 128 == 0 and lin.out_features % (128 if tail else 8) == 0)


# ---- per-block mixed formats (the older variants' quantize_VAR_* functions, as data) --------------------------
def _block_index(name: str) -> int:
    """'blocks.<i>.ffn' -> i, as the reference does (int(name.split('.')[1]))."""
    return int(name.split(".")[1])


_FP6_SYMMETRIC = ("fp6_e2m3", "fp6_e3m2")


def quantize_VAR_mixed(model, layer_formats, weight_quant=None, act_quant=None, w_bit=8, a_bit=8, act_quant_sym=None,
                       fc2_act_log2_quant=None, activation_fp_quant=False, weight_fp_quant=False,
                       ada_lin_formats=None, real_fp6=False, kmajor_operands=True, real_fp4=False, fuse_ffn=False, a6w4_kmajor=False,
                       w6_weights=False, w6_forms=False, w6_kmajor=False, group_fp6=False):
    """quantize_VAR with a format pair per (block, layer): ``layer_formats(block_idx, layer)`` returns
    ``(act_fp_type, weight_fp_type)`` for layer in {"fc1", "fc2", "mat_qkv", "proj"}.  ``ada_lin_formats``:
    None leaves the AdaLN Linear in full precision (as tr/ does), a pair quantizes ``ada_lin[1]`` (as the fq/ and
    rot/ mixed variants do).  Module matching is duck-typed as in quantize_VAR.

    ``real_fp6`` (additive, default off; the W6A6 per_channel / per_token configuration as in quantize_VAR): fc1, mat_qkv, proj and
    fc2 become ``gemm.FP6Linear`` of their (activation, weight) pair wherever both formats are ``fp6_e2m3`` / ``fp6_e3m2`` and the
    shape fits the GEMM (in_features % 128 == 0, out_features % 8 == 0) - same quantization decisions, product on the FP6 matrix
    cores with a format selector per operand; ``ada_lin[1]`` stays a QuantizedLinear.  ``kmajor_operands``: as in quantize_VAR.

    ``real_fp4`` (additive, default off; the W4A4 per-group configuration as in quantize_VAR): every layer with an ``fp_e2`` weight
    and an ``fp_e1`` / ``fp_e2`` / ``fp_e3`` activation whose shape fits the GEMM becomes a ``gemm.FP4Linear`` of its activation
    format - ``fp_e2`` on the FP4 GEMM (k-major with ``kmajor_operands``), ``fp_e1`` / ``fp_e3`` as 6-bit codes on the A6W4 GEMM
    against the same stored E2M1 weight (row-major unless ``a6w4_kmajor``).  Every other layer (fc2's dual format,
    ``ada_lin[1]``, an E1M2 / E3M0 weight) stays the QuantizedLinear it is without the keyword.

    ``w6_weights`` (additive, default off; with ``real_fp4``, else ValueError): fc1, mat_qkv and proj with an ``fp_e1`` / ``fp_e3``
    WEIGHT and an ``fp_e1`` / ``fp_e2`` / ``fp_e3`` activation whose shape fits the GEMM become a ``gemm.FP4Linear`` of that pair too -
    the weight as 6-bit codes on the W6 GEMM (``gemm.linear_w6``; row-major, whatever ``kmajor_operands`` / ``a6w4_kmajor`` say, unless ``w6_kmajor``).
    All six pairs: each one's 128-term dot came out exact on the matrix core (profiles/w6_dot.txt), so none is left behind as a
    QuantizedLinear for its numerics.  fc2 and ``ada_lin[1]`` are as without the keyword; an FFN whose fc1 has such a weight has no
    in-GEMM tail without ``w6_forms``: with ``fuse_ffn`` it takes the one-pass ``GeluThenFc2Quant`` route, or raises as below.

    ``w6_forms`` (additive, default off; with ``w6_weights``, else ValueError): those ``gemm.FP4Linear`` are built with
    ``w6_forms=True``, so a mat_qkv with a 6-bit weight has ``qkv_to_cache`` / ``qkv_to_cache_operands`` (the W6 GEMM's split output,
    q / k norm included), and with ``fuse_ffn`` an FFN whose fc1 has such a weight and meets the conditions below gets the in-GEMM tail
    too: fc1 becomes ``gemm.FP4LinearGeluDual`` on the W6 GEMM (``gemm.linear_w6_gelu_dual``), ``act`` an identity and fc2's input
    quantizer is switched off - one launch where the ``GeluThenFc2Quant`` route takes three.  Row-major unless ``w6_kmajor``.

    ``w6_kmajor`` (additive, default off; with ``w6_weights``, else ValueError; inert when ``kmajor_operands`` is off, as
    ``a6w4_kmajor`` is): the 6-bit-weight fc1 / mat_qkv / proj are built with ``kmajor=True, w6_kmajor=True`` - they hold the dealt
    6-bit weight image and the fp32 weight-side scale image, quantize their activation into the k-major images of its format and run
    the W6 GEMM's k-major forms (``gemm.linear_w6_km``, ``linear_w6_gelu_dual_km``, ``linear_w6_qkv_to_cache_km``): the same bits.
    With ``a6w4_kmajor`` as well, every matrix-core layer of a 3 x 3 model is on one layout.

    ``a6w4_kmajor`` (additive, default off; with ``real_fp4`` and ``kmajor_operands``): the ``fp_e1`` / ``fp_e3`` layers hold the FP4
    GEMM's k-major weight images too and run the A6W4 GEMM's k-major form (``gemm.linear_a6w4_km``) - one weight layout in the
    model, the same bits.

    ``fuse_ffn`` (additive, default off): quantize_VAR's rules, per FFN - the FFN's ``act`` must be GELU(tanh).  With ``real_fp4``,
    where fc1 qualifies for ``gemm.FP4Linear`` with out_features % 128 == 0 and the block's fc2 activation format is
    ``fp_e1m2_neg_e2m1_pos``: fc1 becomes ``gemm.FP4LinearGeluDual`` of its activation format (GELU and fc2's input quantizer in the
    epilogue of the FP4 GEMM for ``fp_e2``, of the A6W4 GEMM for ``fp_e1`` / ``fp_e3``), ``act`` an identity and fc2's input quantizer
    is switched off.  Otherwise, where ``GeluThenFc2Quant`` covers (act_quant, fc2's activation format): ``act`` becomes that
    one-pass module.  An FFN neither applies to raises quantize_VAR's ValueError - when the walk reaches it: the model is converted
    in place (as in quantize_VAR), so the modules in front of that FFN are already replaced and the model is not to be used.

    ``group_fp6`` (additive, default off): as in quantize_VAR, per layer - fc1, mat_qkv and proj whose pair has an ``fp6_e2m3`` /
    ``fp6_e3m2`` side become ``gemm.FP6GroupLinear``; a pure FP4 pair goes where ``real_fp4`` sends it; with ``fuse_ffn`` and a block
    whose fc2 activation format is ``fp6_int_neg_e2m3_pos`` or ``fp_e1m2_neg_e2m1_pos`` such an fc1 becomes
    ``gemm.FP6GroupLinearGeluDual``.  fc2 and ``ada_lin[1]`` are as without the keyword."""
    g6_ok = _group_fp6_ok(group_fp6, weight_quant, act_quant, w_bit, a_bit, activation_fp_quant, weight_fp_quant)
    fp4_ok = (real_fp4 and weight_quant == "per_group" and act_quant == "per_group" and w_bit == 4 and a_bit == 4
              and activation_fp_quant and weight_fp_quant)
    if real_fp4 and not fp4_ok:
        raise ValueError("real_fp4 needs weight_quant = act_quant = 'per_group', w_bit = a_bit = 4, fp formats on both sides")
    fp6_ok = (real_fp6 and weight_quant == "per_channel" and act_quant == "per_token" and w_bit == 6 and a_bit == 6
              and activation_fp_quant and weight_fp_quant)
    if real_fp6 and not fp6_ok:
        raise ValueError("real_fp6 needs weight_quant='per_channel', act_quant='per_token', w_bit = a_bit = 6, fp6 formats")
    if w6_weights and not real_fp4:
        raise ValueError("w6_weights needs real_fp4")
    if w6_forms and not w6_weights:
        raise ValueError("w6_forms needs w6_weights")
    if w6_kmajor and not w6_weights:
        raise ValueError("w6_kmajor needs w6_weights")
    w6_kw = {"w6_forms": True} if w6_forms else {}   # (passed only when on: the keyword list without it is today's)
    if w6_kmajor and kmajor_operands:
        w6_kw.update(kmajor=True, w6_kmajor=True)
    common = dict(weight_quant=weight_quant, act_quant=act_quant, w_bit=w_bit, a_bit=a_bit,
                  activation_fp_quant=activation_fp_quant, weight_fp_quant=weight_fp_quant)

    def fp4_layer(cls, lin, a):   # a gemm.FP4Linear / FP4LinearGeluDual of activation format a
        if a != "fp_e2" and kmajor_operands and a6w4_kmajor:
            return cls.from_float(lin, kmajor=True, act_fp_type=a, a6w4_kmajor=True)
        return cls.from_float(lin, kmajor=kmajor_operands and a == "fp_e2", act_fp_type=a)

    def layer(cls, lin, a, w, w6=False, **kw):   # w6: the layer is one of those w6_weights / group_fp6 cover (fc1, mat_qkv, proj)
        if g6_ok and w6 and _group_fp6_pair(lin, a, w):
            from .gemm import FP6GroupLinear
            return FP6GroupLinear.from_float(lin, w, a, kmajor=kmajor_operands)
        if (fp6_ok and a in _FP6_SYMMETRIC and w in _FP6_SYMMETRIC and lin.in_features % 128 == 0 and lin.out_features % 8 == 0):
            from .gemm import FP6Linear
            return FP6Linear.from_float(lin, kmajor=kmajor_operands, weight_fp_type=w, act_fp_type=a)
        if (fp4_ok and w == "fp_e2" and a in ("fp_e1", "fp_e2", "fp_e3") and lin.in_features % 128 == 0 and lin.out_features % 8 == 0):
            from .gemm import FP4Linear
            return fp4_layer(FP4Linear, lin, a)
        if (fp4_ok and w6 and w6_weights and w in ("fp_e1", "fp_e3") and a in ("fp_e1", "fp_e2", "fp_e3") and lin.in_features % 128 == 0
                and lin.out_features % 8 == 0):
            from .gemm import FP4Linear
            return FP4Linear.from_float(lin, act_fp_type=a, weight_fp_type=w, **w6_kw)
        return cls.from_float(lin, act_fp_type=a, weight_fp_type=w, **kw, **common)

    for name, m in list(model.named_modules()):
        fc1, fc2 = getattr(m, "fc1", None), getattr(m, "fc2", None)
        qkv, proj = getattr(m, "mat_qkv", None), getattr(m, "proj", None)
        ada = getattr(m, "ada_lin", None)
        if isinstance(fc1, nn.Linear) and isinstance(fc2, nn.Linear):
            b = _block_index(name)
            a, w = layer_formats(b, "fc1")
            a2, w2 = layer_formats(b, "fc2")
            act = getattr(m, "act", None)
            gelu_tanh = isinstance(act, nn.GELU) and getattr(act, "approximate", "none") == "tanh"
            w6_tail = w6_forms and w in ("fp_e1", "fp_e3")   # the W6 GEMM's fc1 tail stands in for the FP4 / A6W4 GEMM's
            in_gemm = (fuse_ffn and gelu_tanh and fp4_ok and (w == "fp_e2" or w6_tail) and a in ("fp_e1", "fp_e2", "fp_e3")
                       and a2 == "fp_e1m2_neg_e2m1_pos" and fc1.in_features % 128 == 0 and fc1.out_features % 128 == 0)
            g6_tail = fuse_ffn and gelu_tanh and g6_ok and a2 in _GROUP_FP6_FC2 and _group_fp6_pair(fc1, a, w, tail=True)
            in_gemm = in_gemm or g6_tail
            one_pass = (fuse_ffn and gelu_tanh and not in_gemm and activation_fp_quant and (act_quant, a2) in GeluThenFc2Quant.FUSED
                        and fc1.out_features % (128 if act_quant == "per_group" else 8) == 0)
            if fuse_ffn and not (in_gemm or one_pass):
                raise ValueError("fuse_ffn needs an FFN with act = GELU(approximate='tanh') and a dual-format fc2_fp_type "
                                 "(fp_e1m2_neg_e2m1_pos / fp4_afpq per group, fp6_int_neg_e2m3_pos per group or per token)")
            if in_gemm:
                from .gemm import FP4LinearGeluDual, FP6GroupLinearGeluDual
                if g6_tail:
                    m.fc1 = FP6GroupLinearGeluDual.from_float(fc1, w, a, kmajor=kmajor_operands, fc2_fp_type=a2)
                elif w6_tail:
                    m.fc1 = FP4LinearGeluDual.from_float(fc1, act_fp_type=a, weight_fp_type=w, **w6_kw)
                else:
                    m.fc1 = fp4_layer(FP4LinearGeluDual, fc1, a)
            else:
                m.fc1 = layer(QuantizedLinear, fc1, a, w, w6=True, act_quant_sym=act_quant_sym)
            m.fc2 = layer(QuantizedLinear_fc2, fc2, a2, w2, act_quant_sym=False, fc2_act_log2_quant=fc2_act_log2_quant)
            if in_gemm:
                m.act = nn.Identity()
                m.fc2.act_quant = lambda t: t                      # its input arrives quantized from fc1's epilogue
                m.fc2.act_quant_name = "in fc1's epilogue"
            elif one_pass:
                m.act = GeluThenFc2Quant(act_quant, a2, a_bit)
                m.fc2.act_quant = lambda t: t                      # ... from the activation module in front of it
                m.fc2.act_quant_name = "behind the GELU (one pass)"
        elif isinstance(qkv, nn.Linear) and isinstance(proj, nn.Linear):
            b = _block_index(name)
            a, w = layer_formats(b, "mat_qkv")
            m.mat_qkv = layer(QuantizedLinear, qkv, a, w, w6=True, act_quant_sym=act_quant_sym)
            a, w = layer_formats(b, "proj")
            m.proj = layer(QuantizedLinear, proj, a, w, w6=True, act_quant_sym=act_quant_sym)
        if ada_lin_formats is not None and isinstance(ada, nn.Sequential) and len(ada) > 1 and isinstance(ada[1], nn.Linear):
            a, w = ada_lin_formats
            ada[1] = QuantizedLinear.from_float(ada[1], act_quant_sym=act_quant_sym, act_fp_type=a, weight_fp_type=w, **common)
    return model


def quantize_VAR_mixed_fp4_datatype(model, weight_quant=None, act_quant=None, quantize_bmm_input=False, w_bit=8,
                                    a_bit=8, kv_bit=8, act_quant_sym=None, fc2_act_log2_quant=None, quant_kv=None,
                                    activation_fp_quant=False, weight_fp_quant=False, act_fp_type=None,
                                    weight_fp_type=None, fc2_fp_type=None, real_fp4=False, kmajor_operands=True, fuse_ffn=False,
                                    a6w4_kmajor=False, w6_weights=False, w6_forms=False, w6_kmajor=False):
    """models_fp_quant/quant_utils.py:1256-1341: fc1 is E2M1 in blocks 6-20 and E3M0 elsewhere, mat_qkv E2M1 in
    blocks 0, 24, 25 and E3M0 elsewhere (activations; weights always E2M1); proj, fc2 and ada_lin[1] take the
    caller's formats.
    ``real_fp4`` / ``kmajor_operands``: as in quantize_VAR_mixed - every E2M1-weight fc1 / mat_qkv / proj on the matrix cores,
    the E3M0 activations as 6-bit codes.  ``fuse_ffn``: as in quantize_VAR_mixed - with ``real_fp4`` and ``fc2_fp_type`` =
    ``fp_e1m2_neg_e2m1_pos`` every fc1 runs its GELU and fc2's input quantizer in its GEMM's epilogue.  ``a6w4_kmajor``: as in
    quantize_VAR_mixed - the E3M0-activation layers on k-major images too.  ``w6_weights``: as in quantize_VAR_mixed - a proj whose
    ``weight_fp_type`` is ``fp_e1`` / ``fp_e3`` on the W6 GEMM; ``w6_forms`` / ``w6_kmajor``: passed through as well."""
    fc1_e2, qkv_e2 = set(range(6, 21)), {0, 24, 25}

    def fmt(b, layer):
        if layer == "fc1":
            return ("fp_e2" if b in fc1_e2 else "fp_e3", "fp_e2")
        if layer == "mat_qkv":
            return ("fp_e2" if b in qkv_e2 else "fp_e3", "fp_e2")
        if layer == "fc2":
            return (fc2_fp_type, weight_fp_type)
        return (act_fp_type, weight_fp_type)

    return quantize_VAR_mixed(model, fmt, weight_quant, act_quant, w_bit, a_bit, act_quant_sym, fc2_act_log2_quant,
                              activation_fp_quant, weight_fp_quant, ada_lin_formats=(act_fp_type, weight_fp_type),
                              real_fp4=real_fp4, kmajor_operands=kmajor_operands, fuse_ffn=fuse_ffn, a6w4_kmajor=a6w4_kmajor,
                              w6_weights=w6_weights, w6_forms=w6_forms, w6_kmajor=w6_kmajor)


def quantize_VAR_use_different_datatype(model, weight_quant=None, act_quant=None, quantize_bmm_input=False, w_bit=8,
                                        a_bit=8, kv_bit=8, act_quant_sym=None, fc2_act_log2_quant=None, quant_kv=None,
                                        activation_fp_quant=False, weight_fp_quant=False, act_fp_type=None,
                                        weight_fp_type=None, fc2_fp_type=None, real_fp4=False, kmajor_operands=True, fuse_ffn=False,
                                        a6w4_kmajor=False, w6_weights=False, w6_forms=False, w6_kmajor=False):
    """models_fp_quant_rotate/quant_utils.py:982-1066: as the mixed FP4 variant, with mat_qkv E2M1 in blocks 24, 25 only.
    ``real_fp4`` / ``kmajor_operands``: as in quantize_VAR_mixed - every E2M1-weight fc1 / mat_qkv / proj on the matrix cores,
    the E3M0 activations as 6-bit codes.  ``fuse_ffn``: as in quantize_VAR_mixed - with ``real_fp4`` and ``fc2_fp_type`` =
    ``fp_e1m2_neg_e2m1_pos`` every fc1 runs its GELU and fc2's input quantizer in its GEMM's epilogue.  ``a6w4_kmajor``: as in
    quantize_VAR_mixed - the E3M0-activation layers on k-major images too.  ``w6_weights``: as in quantize_VAR_mixed - a proj whose
    ``weight_fp_type`` is ``fp_e1`` / ``fp_e3`` on the W6 GEMM; ``w6_forms`` / ``w6_kmajor``: passed through as well."""
    fc1_e2, qkv_e2 = set(range(6, 21)), {24, 25}

    def fmt(b, layer):
        if layer == "fc1":
            return ("fp_e2" if b in fc1_e2 else "fp_e3", "fp_e2")
        if layer == "mat_qkv":
            return ("fp_e2" if b in qkv_e2 else "fp_e3", "fp_e2")
        if layer == "fc2":
            return (fc2_fp_type, weight_fp_type)
        return (act_fp_type, weight_fp_type)

    return quantize_VAR_mixed(model, fmt, weight_quant, act_quant, w_bit, a_bit, act_quant_sym, fc2_act_log2_quant,
                              activation_fp_quant, weight_fp_quant, ada_lin_formats=(act_fp_type, weight_fp_type),
                              real_fp4=real_fp4, kmajor_operands=kmajor_operands, fuse_ffn=fuse_ffn, a6w4_kmajor=a6w4_kmajor,
                              w6_weights=w6_weights, w6_forms=w6_forms, w6_kmajor=w6_kmajor)


def quantize_VAR_mixed_fp6_datatype(model, weight_quant=None, act_quant=None, quantize_bmm_input=False, w_bit=8,
                                    a_bit=8, kv_bit=8, act_quant_sym=None, fc2_act_log2_quant=None, quant_kv=None,
                                    activation_fp_quant=False, weight_fp_quant=False, act_fp_type=None,
                                    weight_fp_type=None, fc2_fp_type=None, real_fp6=False, kmajor_operands=True):
    """models_fp_quant/quant_utils.py:1344-1431: weights always E2M3; activations E3M2 for fc1 and mat_qkv, for fc2
    E2M3 in blocks 0 and 23 (E3M2 elsewhere), for proj E2M3 in blocks 2-29 (E3M2 in 0, 1); ada_lin[1] E2M3 / E2M3.
    ``real_fp6`` / ``kmajor_operands``: as in quantize_VAR_mixed - every fc1, fc2, mat_qkv and proj on the FP6 matrix cores."""
    def fmt(b, layer):
        if layer in ("fc1", "mat_qkv"):
            return ("fp6_e3m2", "fp6_e2m3")
        if layer == "fc2":
            return ("fp6_e2m3" if b in (0, 23) else "fp6_e3m2", "fp6_e2m3")
        return ("fp6_e2m3" if 2 <= b <= 29 else "fp6_e3m2", "fp6_e2m3")

    return quantize_VAR_mixed(model, fmt, weight_quant, act_quant, w_bit, a_bit, act_quant_sym, fc2_act_log2_quant,
                              activation_fp_quant, weight_fp_quant, ada_lin_formats=("fp6_e2m3", "fp6_e2m3"),
                              real_fp6=real_fp6, kmajor_operands=kmajor_operands)
