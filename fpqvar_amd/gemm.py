"""F2: real FP4 arithmetic for the W4A4 per-group E2M1 configuration.

The reference only *simulates* FP4: it de-quantizes and runs an fp16 GEMM
(tr/quant_utils.py:765-767).  Here the quantizer emits hardware E2M1 nibbles + per-group scales and
the product runs on MI355X's block-scaled FP4 matrix cores (`fpq_gemm_fp4_mx`).
"""
from __future__ import annotations

import ctypes
import os
from typing import NamedTuple, Optional, Tuple, Union

import torch

from . import ops
from ._lib import TABLE_IDS, GemmEpilogue, GemmSplit, check, dtype_id, lib, require_gpu, stream_ptr, device_guard

try:   # the compiled binding (csrc/quant_cuda_ext.cpp)
    from . import _native
except ImportError:   # pragma: no cover - build() always produces it
    _native = None
if os.environ.get("FPQ_NO_NATIVE") == "1":   # the A/B tools time variant builds of the library through ctypes (_lib.use_variant)
    _native = None

E2M1_LEVELS = (0.0, 0.5, 1.0, 1.5, 2.0, 3.0, 4.0, 6.0)


def _epilogue(name: str, tokens: int, outs: int, gate: Optional[torch.Tensor], residual: Optional[torch.Tensor],
              out: Optional[torch.Tensor], device):
    """The GEMMs' optional fused tail `residual + y * gate` (fpq_gemm_epilogue_t): gate is gamma of the AdaLN block,
    [B, 1, outs] or [B, outs] fp16 with tokens % B == 0; residual is [..., outs] fp16 with `tokens` rows.
    Returns (pointer or None, objects to keep alive until the launch, output tensor)."""
    if gate is None and residual is None:
        return None, (), torch.empty((tokens, outs), dtype=torch.float16, device=device) if out is None else out
    ep, keep = GemmEpilogue(None, None, 1), []
    if gate is not None:
        g = gate.reshape(-1, outs)
        if g.dtype != torch.float16 or g.shape[0] == 0 or tokens % g.shape[0] != 0:
            raise RuntimeError(f"{name}: gate must be float16 [B, outs] with tokens % B == 0, got {tuple(gate.shape)} {gate.dtype}")
        g = g.contiguous()
        ep.gate, ep.rows_per_gate = g.data_ptr(), max(tokens // g.shape[0], 1)
        keep.append(g)
    if residual is not None:
        r = residual.reshape(-1, outs)
        if r.dtype != torch.float16 or r.shape[0] != tokens:
            raise RuntimeError(f"{name}: residual must be float16 with {tokens} rows of {outs}, got {tuple(residual.shape)} {residual.dtype}")
        r = r.contiguous()
        ep.residual = r.data_ptr()
        keep.append(r)
    keep.append(ep)
    return ctypes.byref(ep), keep, torch.empty((tokens, outs), dtype=torch.float16, device=device) if out is None else out


# ---- k-major operand images (include/fpq.h): codes as [K / 128, image rows, 64 | 96] instead of [rows, row bytes] --------
# A 3-D uint8 tensor IS an image, a 2-D one row-major codes: the Linears below pick the entry point from the operand's shape
# (both operands must agree).  Weights: `to_kmajor(codes, bits, dealt=True)` once at load time; activations: the producers'
# `kmajor=True` forms write the image directly (to_kmajor(codes, bits) converts any other producer's output).  The per-group
# scales of an FP4 operand travel with it as an fp32 image [K/128, rows rounded up to 4 | 64] (`to_kmajor_scales`); the FP6
# operands keep their one scale per row.
def to_kmajor(codes: torch.Tensor, code_bits: int, dealt: bool = False) -> torch.Tensor:
    """Row-major operand codes [rows, K/2] (code_bits 4) or [rows, K*3/4] (6) -> the k-major image [K/128, image_rows, 64 | 96]
    (fpq_codes_to_kmajor).  dealt: the weight side's row order, image_rows = rows rounded up to 64."""
    require_gpu(codes, "to_kmajor")
    seg = {4: 64, 6: 96}.get(code_bits)
    if seg is None or codes.dim() != 2 or codes.dtype != torch.uint8 or codes.shape[1] % seg != 0:
        raise RuntimeError("to_kmajor: codes must be uint8 [rows, K/2] (code_bits 4) or [rows, K*3/4] (6) with K % 128 == 0")
    c = codes.contiguous()
    rows, steps = c.shape[0], c.shape[1] // seg
    image = torch.empty((steps, (rows + 63) // 64 * 64 if dealt else rows, seg), dtype=torch.uint8, device=c.device)
    with device_guard(c.device):
        check(lib().fpq_codes_to_kmajor(c.data_ptr(), image.data_ptr(), rows, steps * 128, code_bits, 1 if dealt else 0,
                                        stream_ptr(c.device)), "fpq_codes_to_kmajor")
    return image


def to_kmajor_scales(scales: torch.Tensor, weight_side: bool = False) -> torch.Tensor:
    """Per-group scales [rows, K/128] (fp16 / fp32) of an FP4 operand -> the fp32 k-major scale image [K/128, image_rows]
    (fpq_scales_to_kmajor): image_rows = rows rounded up to 4, or to 64 on the weight side; the padding is zero."""
    require_gpu(scales, "to_kmajor_scales")
    if scales.dim() != 2 or scales.dtype not in (torch.float16, torch.float32):
        raise RuntimeError("to_kmajor_scales: scales must be float16 / float32 [rows, K/128]")
    sc = scales.contiguous()
    rows, groups = sc.shape
    image = torch.empty((groups, (rows + 63) // 64 * 64 if weight_side else (rows + 3) // 4 * 4), dtype=torch.float32, device=sc.device)
    with device_guard(sc.device):
        check(lib().fpq_scales_to_kmajor(sc.data_ptr(), dtype_id(sc.dtype), image.data_ptr(), rows, groups, 1 if weight_side else 0,
                                         stream_ptr(sc.device)), "fpq_scales_to_kmajor")
    return image


def kmajor_mx_scales(rows: int, k: int, device) -> torch.Tensor:
    """an empty k-major scale image for `rows` activation rows ([K/128, rows rounded up to 4] fp32) with its padding zeroed -
    what the *_km producers of FP4 operands write their scales into"""
    pad = (rows + 3) // 4 * 4
    image = torch.empty((k // 128, pad), dtype=torch.float32, device=device)
    if pad != rows:
        image[:, rows:].zero_()
    return image


def _kmajor_pair(name: str, a: torch.Tensor, w: torch.Tensor, seg: int) -> bool:
    """True when both operands are k-major images (3-D), False when both are row-major codes (2-D); anything else is an error."""
    if a.dim() == 3 and w.dim() == 3:
        if a.shape[2] != seg or w.shape[2] != seg or a.shape[0] != w.shape[0] or w.shape[1] % 64 != 0:
            raise RuntimeError(f"{name}: k-major images must be [K/128, rows, {seg}] with the same K and a weight image of a multiple of 64 rows")
        return True
    if a.dim() == 2 and w.dim() == 2:
        return False
    raise RuntimeError(f"{name}: both operands must be row-major codes (2-D) or both k-major images (3-D)")


# ---- the per-group family: E2M1 nibbles on the FP4 GEMM; E1M2 / E3M0 as dense 6-bit codes on the A6W4 GEMM (include/fpq.h) --------
# Per-group scales (one per 128 elements) on both sides, the same E2M1 weight whatever the activation's format.  The reference's
# mixed W4A4 model gives fc1 / mat_qkv an E3M0 or E1M2 activation format in most blocks; the matrix instruction decodes a 6-bit
# activation fragment (E1M2 levels as FP6 E2M3 codes, E3M0 levels as BF6 E3M2 codes) against E2M1 nibbles.
#
# One row per activation format holds everything the Python side knows about it; `_per_group_operands` checks an operand pair,
# `_per_group_gemm` is the one place that names a GEMM entry point of the family, and the public Linears below are the three
# bodies (`_linear`, `_linear_gelu_dual`, `_linear_qkv_to_cache`) under their own names.  A new format is a row; a new form of
# the GEMM is a form name in `_per_group_gemm` and a body.
#
# What differs between the public functions, and stays as it is (rows of the table or arguments of the bodies, not decisions
# scattered in them):
#  - linear_fp4 and linear_fp4_gelu_dual hand the whole call to the compiled binding when it is loaded, before any check here;
#  - the bias: linear_fp4 checks no size and copies for alignment (16 bytes) only beside images (`loose_bias`); every other plain /
#    fc1 form checks that it holds `outs` values and copies to `bias_align` (16 FP4, 8 A6W4); the split forms check it and align
#    to 16, and their q / k norm form takes an fp32 bias of 3C instead (_qkv_split_args);
#  - row-major activation scales are fp16, scale images are fp32 of the padded shapes; weight scales fp16 or fp32, except that the
#    A6W4 split forms are compiled for fp32 ones only (`split_w_f32`);
#  - linear_a6w4 / _gelu_dual take row-major codes only and their _km twins images only (`layouts`); the others go by rank;
#  - the split forms take `outs` from the cache, not from the bias;
#  - the fc1 forms skip the launch when tokens == 0 or outs == 0, the split forms when tokens == 0, the plain forms never;
#  - the order of refusals: GPU, table, (cache), operands, (weight scale dtype), then the form's own arguments.
class _Format(NamedTuple):
    seg: int                   # bytes of activation codes per 128 elements
    gemm: str                  # the GEMM's C entry point family
    plain: str                 # what the plain row-major entry point adds to "<family>_mx" (the FP4 one with an epilogue is _ex)
    table: Tuple[int, ...]     # the table id that follows a_scales in every call of the family, or nothing
    quant: str                 # the quantizer's C entry points: row-major codes,
    quant_km: str              # k-major images
    quantizer: str             # the public quantizer, for its messages
    bias_align: int
    split_w_f32: bool
    w_seg: int = 64            # bytes of weight codes per 128 elements: 64 = E2M1 nibbles, 96 = dense 6-bit codes (linear_w6)
    w_table: Tuple[int, ...] = ()   # the weight's table id, which follows the weight scales' dtype in a call of the W6 family
    quant_table: Optional[Tuple[int, ...]] = None   # the quantizer's table id where it is not `table` (a full FP6 table: `table` names the decode)
    quant_flag: bool = False   # the quantizer takes the layout as a flag before the stream (one entry point for both layouts)


_FORMATS = {
    "e2m1": _Format(64, "fpq_gemm_fp4", "_ex", (), "fpq_quant_rows_codes_mx", "fpq_quant_rows_codes_mx_km", "quantize_mx", 16, False),
    "e1m2": _Format(96, "fpq_gemm_a6w4", "", (TABLE_IDS["e1m2"],), "fpq_quant_rows_codes_g6", "fpq_a6w4_quant_rows_codes_km", "quantize_g6", 8, True),
    "e3m0": _Format(96, "fpq_gemm_a6w4", "", (TABLE_IDS["e3m0"],), "fpq_quant_rows_codes_g6", "fpq_a6w4_quant_rows_codes_km", "quantize_g6", 8, True),
    # the FULL FP6 tables per group (quantize_gf6; the Linears: linear_g6*): the A6W4 kernels decode any E2M3 codes under the selector
    # id of E1M2 and any E3M2 codes under that of E3M0 (include/fpq.h, GF6), so the id that follows a_scales is the DECODE format's
    "e2m3": _Format(96, "fpq_gemm_a6w4", "", (TABLE_IDS["e1m2"],), "fpq_gf6_quant_rows_codes", "fpq_gf6_quant_rows_codes", "quantize_gf6", 8, True,
                    quant_table=(TABLE_IDS["e2m3"],), quant_flag=True),
    "e3m2": _Format(96, "fpq_gemm_a6w4", "", (TABLE_IDS["e3m0"],), "fpq_gf6_quant_rows_codes", "fpq_gf6_quant_rows_codes", "quantize_gf6", 8, True,
                    quant_table=(TABLE_IDS["e3m2"],), quant_flag=True),
}
# E1M2 / E3M0 WEIGHTS as 6-bit codes (fpq_gemm_w6_mx, _gelu_dual, _mx_split, _mx_split_qknorm, each with a _km twin for k-major
# images; fp32 weight scales only): a row per (activation, weight) pair
_W6_FORMATS = {(a, w): _FORMATS[a]._replace(gemm="fpq_gemm_w6", plain="", table=(TABLE_IDS[a],), bias_align=8, split_w_f32=True, w_seg=96,
                                            w_table=(TABLE_IDS[w],))
               for a in ("e2m1", "e1m2", "e3m0") for w in ("e1m2", "e3m0")}
_G6_TABLES = {"e1m2": "e1m2", "fp_e1": "e1m2", "e3m0": "e3m0", "fp_e3": "e3m0"}
_G6_CODE_FORMAT = {"e1m2": "e2m3", "e3m0": "e3m2"}   # the 6-bit hardware format that holds the table's levels


def _g6_table(name: str, table: str) -> str:
    try:
        return _G6_TABLES[table]
    except (KeyError, TypeError):
        raise RuntimeError(f"{name}: the per-group 6-bit activation tables are 'e1m2' and 'e3m0', got {table!r}") from None


def _g6_format(name: str, table: str) -> _Format:
    """The row of the 6-bit table a caller of the A6W4 functions named.  The shared bodies below take `fmt` as a row (the FP4
    functions and the modules pass one) or as such a name, which they resolve where the A6W4 functions have always refused a
    wrong one: after the GPU check, before the operands."""
    return _FORMATS[_g6_table(name, table)]


def _quantize_per_group(name: str, fmt: Union[_Format, str], x: torch.Tensor, kmajor: bool) -> Tuple[torch.Tensor, torch.Tensor]:
    """quantize_mx / quantize_g6: x [..., K] -> (codes, scales) of `fmt`, row-major or as the activation side's k-major images"""
    require_gpu(x, name)
    if x.dtype not in (torch.float16, torch.float32):
        raise RuntimeError(f"{name}: x must be float16 or float32, got {x.dtype}")
    if not isinstance(fmt, _Format):
        fmt = _g6_format(name, fmt)
    k = x.shape[-1]
    if k % 128 != 0:
        raise RuntimeError(f"{name}: the last dimension must be a multiple of 128")
    if kmajor and x.dtype == torch.float32:   # the image-writing quantizers take fp16 rows (activations); fp32 rows: two steps
        codes, scales = _quantize_per_group(name, fmt, x, False)
        return to_kmajor(codes, 4 if fmt.seg == 64 else 6), to_kmajor_scales(scales)
    xc, dev = x.contiguous(), x.device
    rows = xc.numel() // k
    codes = torch.empty((k // 128, rows, fmt.seg) if kmajor else (rows, k // 128 * fmt.seg), dtype=torch.uint8, device=dev)
    scales = kmajor_mx_scales(rows, k, dev) if kmajor else torch.empty((rows, k // 128), dtype=x.dtype, device=dev)
    what = fmt.quant_km if kmajor else fmt.quant
    with device_guard(dev):
        check(getattr(lib(), what)(xc.data_ptr(), codes.data_ptr(), scales.data_ptr(), rows, k,
                                   *(fmt.table if fmt.quant_table is None else fmt.quant_table), dtype_id(x.dtype),
                                   *((1 if kmajor else 0,) if fmt.quant_flag else ()), stream_ptr(dev)), what)
    return codes, scales


def quantize_mx(x: torch.Tensor, kmajor: bool = False) -> Tuple[torch.Tensor, torch.Tensor]:
    """x [..., K] fp16/fp32 (K % 128 == 0) -> (codes uint8 [rows, K/2], scales [rows, K/128] in x.dtype).
    kmajor: the activation side's k-major images - codes [K/128, rows, 64] and scales fp32 [K/128, rows rounded up to 4]."""
    return _quantize_per_group("quantize_mx", _FORMATS["e2m1"], x, kmajor)


def dequantize_mx(codes: torch.Tensor, scales: torch.Tensor) -> torch.Tensor:
    """Reference decoder in torch ops (tests / debugging): fp32 [rows, K]."""
    lv = torch.tensor(E2M1_LEVELS + tuple(-v for v in E2M1_LEVELS), dtype=torch.float32, device=codes.device)
    lo, hi = (codes & 0xF).long(), (codes >> 4).long()
    q = torch.stack((lv[lo], lv[hi]), dim=-1).reshape(codes.shape[0], -1)
    return (q.view(codes.shape[0], -1, 128) * scales.float().unsqueeze(-1)).reshape(codes.shape[0], -1)


def quantize_g6(x: torch.Tensor, table: str = "e3m0", kmajor: bool = False) -> Tuple[torch.Tensor, torch.Tensor]:
    """x [..., K] fp16/fp32 (K % 128 == 0) -> (codes uint8 [rows, K * 3 / 4]: dense 6-bit codes of the E1M2 / E3M0 levels,
    scales [rows, K/128] in x.dtype); level(code) * scale == fp_quant_e1_per_group_cuda / fp_quant_e3_per_group_cuda (x, 4, 128)
    bit for bit (fpq_quant_rows_codes_g6).
    kmajor: the activation side's k-major images instead (fpq_a6w4_quant_rows_codes_km) - codes [K/128, rows, 96] and scales fp32
    [K/128, rows rounded up to 4], what linear_a6w4_km takes."""
    return _quantize_per_group("quantize_g6", table, x, kmajor)


def dequantize_g6(codes: torch.Tensor, scales: torch.Tensor, table: str = "e3m0") -> torch.Tensor:
    """Reference decoder in torch ops (tests / debugging): fp32 [rows, K] = level(code) * scale of the code's group."""
    table = _g6_table("dequantize_g6", table)
    rows = codes.shape[0]
    lv = dequantize_fp6(codes, torch.ones(rows, dtype=torch.float32, device=codes.device), _G6_CODE_FORMAT[table])
    return (lv.view(rows, -1, 128) * scales.float().unsqueeze(-1)).reshape(rows, -1)


class _ScaledOperandModule(torch.nn.Module):
    """Base of the matrix-core Linears.  The quantization scales are fp32 in the reference (the weight is quantized in
    fp32, tr/quant_utils.py:828-837); the driver's `var.half()` (evaluate_fp_quant_transform_rotate.py:131) must not
    round them to fp16 - floating-point casts applied to the module (half(), to(dtype), float()) leave `w_scales`
    alone, device moves still apply."""

    def _apply(self, fn, recurse=True):
        keep = self._buffers.get("w_scales")
        super()._apply(fn, recurse)
        moved = self._buffers.get("w_scales")
        if keep is not None and moved is not None and moved.dtype != keep.dtype:
            self._buffers["w_scales"] = keep.to(device=moved.device)
        return self


    # ---- the packed form (packed.PackedWeight) and the other layout -------------------------------------------------------
    def _packed_cols(self) -> int:
        """the quantization row of the held weight: 128 with per-group scales, in_features with one scale per output channel"""
        return 128 if self.w_scales.dim() == 2 else self.in_features

    def to_packed(self, **header):
        """The held weight as a packed.PackedWeight (fpq_operands_to_packed): `operands(self.kmajor)` of the result returns the
        module's w_codes / w_scales.  header: out_dtype, rotate_block, rotate_seed, smooth."""
        from .packed import PackedWeight
        return PackedWeight.from_operands(self.w_codes, self.w_scales, self.w_table, (self.out_features, self.in_features),
                                          self._packed_cols(), bias=self.bias, **header)

    @classmethod
    def from_packed(cls, packed, **kwargs):
        """from_float for a packed.PackedWeight instead of an nn.Linear: the same keyword arguments but weight_fp_type - the table
        is the packed weight's - and the same ValueErrors; the buffers come from `packed.operands(kmajor)`, one launch."""
        if "weight_fp_type" in kwargs:
            raise TypeError(f"{cls.__name__}.from_packed: the weight format is the packed weight's ({packed.table}), not an argument")
        if len(packed.shape) != 2:
            raise ValueError(f"{cls.__name__}.from_packed: a Linear's weight is 2-D, the packed one has shape {tuple(packed.shape)}")
        stub = torch.nn.Linear(packed.shape[1], packed.shape[0], bias=False, device="meta")   # shapes only: no weight to read
        stub.packed_weight = packed
        return cls.from_float(stub, weight_fp_type=packed.table, **kwargs)

    def _load_from_state_dict(self, state_dict, prefix, local_metadata, strict, missing_keys, unexpected_keys, error_msgs):
        """w_codes of the other rank than the module holds (row-major codes for a k-major module, or the reverse) are converted,
        together with w_scales, through the packed form - two launches (fpq_operands_to_packed, fpq_packed_to_operands); on the CPU
        they are left as they are and the usual size mismatch is reported."""
        codes, scales = state_dict.get(prefix + "w_codes"), state_dict.get(prefix + "w_scales")
        if (isinstance(codes, torch.Tensor) and isinstance(scales, torch.Tensor) and codes.is_cuda and scales.is_cuda
                and codes.dim() != self.w_codes.dim() and codes.dim() in (2, 3) and hasattr(self, "w_table")):
            from .packed import PackedWeight
            try:
                p = PackedWeight.from_operands(codes, scales, self.w_table, (self.out_features, self.in_features), self._packed_cols())
                state_dict[prefix + "w_codes"], state_dict[prefix + "w_scales"] = p.operands(self.w_codes.dim() == 3)
            except RuntimeError:
                pass   # not this module's weight in the other layout: the size mismatch below says so
        super()._load_from_state_dict(state_dict, prefix, local_metadata, strict, missing_keys, unexpected_keys, error_msgs)


def _weight_operands(name: str, module: torch.nn.Linear, table: str, kmajor: bool, per_channel: bool = False):
    """(w_codes, w_scales, bias) of a matrix-core Linear built from `module`: quantized from module.weight.float() by the format's
    quantizer (and converted to the dealt k-major images), or - with a packed.PackedWeight attached as module.packed_weight
    (packed.attach) - taken from it in one launch without reading module.weight.  name: "<class>.from_float"."""
    cols = module.in_features if per_channel else 128
    packed = getattr(module, "packed_weight", None)
    if packed is not None:
        if packed.table != table or packed.cols != cols or tuple(packed.shape) != (module.out_features, module.in_features):
            raise ValueError(f"{name}: the attached packed weight is {packed.table} {tuple(packed.shape)} in rows of {packed.cols}, "
                             f"the layer asks for {table} {(module.out_features, module.in_features)} in rows of {cols}")
        codes, scales = packed.operands(kmajor)
        if per_channel and scales.dim() == 2:   # in_features == 128: rows of 128 are channels too, the operand came with its scales
            scales = (scales[0] if kmajor else scales.reshape(-1))[:module.out_features].contiguous()
        bias = packed.bias if packed.bias is not None else module.bias
    else:
        w = module.weight.detach().float()
        if per_channel:
            codes, scales = quantize_fp6(w, table=table)
        else:
            codes, scales = _quantize_any(name, table, w)
        if kmajor:
            codes = to_kmajor(codes, 4 if table == "e2m1" else 6, dealt=True)
            scales = scales if per_channel else to_kmajor_scales(scales, weight_side=True)
        bias = module.bias
    return codes, scales, None if bias is None else bias.detach().to(torch.float16)


def _check_operand(what: str, codes: torch.Tensor, scales: torch.Tensor, rows: int, row_bytes: int, n_scales: int,
                   device) -> None:
    """Shapes, dtypes and placement of a (codes, scales) operand BEFORE the kernel sees the pointers: a truncated or
    inconsistent operand is a Python error here, not an out-of-bounds read on the GPU."""
    if codes.dtype != torch.uint8 or not codes.is_contiguous() or codes.device != device:
        raise RuntimeError(f"{what}: codes must be a contiguous uint8 tensor on {device}")
    if codes.numel() != rows * row_bytes:
        raise RuntimeError(f"{what}: codes hold {codes.numel()} bytes, expected {rows} x {row_bytes}")
    if scales.dtype not in (torch.float16, torch.float32) or not scales.is_contiguous() or scales.device != device:
        raise RuntimeError(f"{what}: scales must be a contiguous float16 / float32 tensor on {device}")
    if scales.numel() != n_scales:
        raise RuntimeError(f"{what}: {scales.numel()} scales, expected {n_scales}")


def _check_kmajor_fp4(name: str, a_codes, a_scales, w_codes, w_scales, bias, outs):
    """shapes of a k-major FP4 operand pair -> (tokens, outs, k); `outs` (or the bias) names the Linear's width when it is not
    the weight image's row count (a multiple of 64)"""
    groups, tokens, w_rows = a_codes.shape[0], a_codes.shape[1], w_codes.shape[1]
    if outs is None:
        outs = bias.numel() if bias is not None else w_rows
    if not (w_rows - 64 < outs <= w_rows):
        raise RuntimeError(f"{name}: outs = {outs} does not belong to a weight image of {w_rows} rows")
    dev = a_codes.device
    for what, t, rows in (("activation", a_scales, (tokens + 3) // 4 * 4), ("weight", w_scales, w_rows)):
        if t.dtype != torch.float32 or tuple(t.shape) != (groups, rows) or not t.is_contiguous() or t.device != dev:
            raise RuntimeError(f"{name}({what}): the k-major scale image must be a contiguous float32 [{groups}, {rows}] tensor on {dev}")
    for what, t in (("activation", a_codes), ("weight", w_codes)):
        if t.dtype != torch.uint8 or not t.is_contiguous() or t.device != dev:
            raise RuntimeError(f"{name}({what}): the k-major image must be a contiguous uint8 tensor on {dev}")
    return tokens, outs, groups * 128


def _per_group_operands(name: str, fmt: _Format, a, a_scales, w, w_scales, bias, outs, layouts: str = "rank"):
    """An operand pair of the per-group family - activation codes of `fmt`, E2M1 weight nibbles - checked -> (km, tokens, outs, k);
    what the compiled binding's fp4_shapes does for E2M1.  layouts: "rank" - row-major codes (2-D) or k-major images (3-D, with
    their fp32 scale images), told by the operands' rank; "rows" / "images" - the public function takes that layout only.
    `outs` (or the bias) only matters for images, see _check_kmajor_fp4."""
    a_rank, w_rank = a.dim(), w.dim()
    km = a_rank == 3 and w_rank == 3
    if fmt.w_seg != 64 and layouts != "images" and (a_rank != 2 or w_rank != 2):
        raise RuntimeError(f"{name}: row-major operands only (k-major images of a 6-bit weight: the _km functions)")
    if layouts == "rows" and (a_rank != 2 or w_rank != 2):
        raise RuntimeError(f"{name}: row-major operands only (k-major images: {name}_km)")
    if layouts == "images" and not km:
        raise RuntimeError(f"{name}: both operands must be k-major images (3-D); row-major codes go to {name[:-3]}")
    if km:
        if a.shape[2] != fmt.seg or w.shape[2] != fmt.w_seg or a.shape[0] != w.shape[0] or w.shape[1] % 64 != 0:
            shapes = ("[K/128, rows, 64]" if fmt.seg == fmt.w_seg == 64 else
                      f"[K/128, tokens, {fmt.seg}] (activation) and [K/128, rows, {fmt.w_seg}] (weight)")
            raise RuntimeError(f"{name}: k-major images must be {shapes} with the same K and a weight image of a multiple of 64 rows")
        return (True, *_check_kmajor_fp4(name, a, a_scales, w, w_scales, bias, outs))
    if a_rank != 2 or w_rank != 2:
        raise RuntimeError(f"{name}: both operands must be row-major codes (2-D) or both k-major images (3-D)")
    tokens, outs, k = a.shape[0], w.shape[0], w.shape[1] * 128 // fmt.w_seg
    if k % 128 != 0 or w.shape[1] != k // 128 * fmt.w_seg or a.shape[1] != k // 128 * fmt.seg or a_scales.dtype != torch.float16:
        raise RuntimeError(f"{name}: operand shapes / activation scale dtype mismatch")
    dev = a.device
    _check_operand(f"{name}(activation)", a, a_scales, tokens, a.shape[1], tokens * (k // 128), dev)
    _check_operand(f"{name}(weight)", w, w_scales, outs, w.shape[1], outs * (k // 128), dev)
    return False, tokens, outs, k


def _per_group_gemm(form: str, fmt: _Format, km: bool, a, a_scales, w, w_scales, *rest) -> None:
    """One call of the family's C entry point of `form`: "" (plain, with the optional gate / residual tail), "gelu_dual" (fc1),
    "split" or "split_qknorm" (mat_qkv into the cache), "sqerr" (the loss against a reference, row-major only); rest: its arguments between the weight scales' dtype and the stream - or,
    for the split forms, which take the layout as a flag, the k-major flag before it (the W6 family has no flag: its split forms
    have an entry point per layout too)."""
    if form in ("split", "split_qknorm"):
        if fmt.w_seg == 64:
            what, rest = f"{fmt.gemm}_mx_{form}", (*rest, 1 if km else 0)
        else:
            what = f"{fmt.gemm}_mx_{form}_km" if km else f"{fmt.gemm}_mx_{form}"
    elif form == "gelu_dual_pair":   # the fc1 tail with its dual pair as an argument: one entry point, the layout a flag behind the pair
        what, rest = f"{fmt.gemm}_gelu_dual_pair", (*rest, 1 if km else 0)
    elif form:   # an entry point per layout
        what = f"{fmt.gemm}_{form}_km" if km else f"{fmt.gemm}_{form}"
    else:
        what = fmt.gemm + "_mx_km" if km else fmt.gemm + "_mx" + fmt.plain
    dev = a.device
    with device_guard(dev):
        check(getattr(lib(), what)(a.data_ptr(), a_scales.data_ptr(), *fmt.table, w.data_ptr(), w_scales.data_ptr(), dtype_id(w_scales.dtype),
                                   *fmt.w_table, *rest, stream_ptr(dev)), what)


def _bias_f16(name: str, bias: Optional[torch.Tensor], outs: Optional[int], device, align: int = 0) -> Optional[torch.Tensor]:
    """The bias as the kernels read it: a contiguous fp16 vector, or None.  outs: when given, it must hold that many values
    on `device`; align: when not 0, a copy is made unless the address is a multiple of it."""
    if bias is None:
        return None
    if outs is not None and (bias.numel() != outs or bias.device != device):
        raise RuntimeError(f"{name}: bias must hold one value per output ({outs}) on {device}")
    b = bias.detach().to(torch.float16).reshape(-1).contiguous()
    if align and b.data_ptr() % align:
        b = b.clone()
    return b


def _linear(name: str, fmt, layouts: str, a, a_scales, w, w_scales, bias, gate, residual, outs, loose_bias: bool = False) -> torch.Tensor:
    """The plain Linear with its optional gate / residual tail: linear_fp4, linear_a6w4, linear_a6w4_km, linear_w6, linear_w6_km"""
    require_gpu(a, name)
    if not isinstance(fmt, _Format):
        fmt = _g6_format(name, fmt)
    dev = a.device
    km, tokens, outs, k = _per_group_operands(name, fmt, a, a_scales, w, w_scales, bias, outs, layouts)
    ep, keep, out = _epilogue(name, tokens, outs, gate, residual, None, dev)
    if loose_bias:
        b = _bias_f16(name, bias, None, dev, fmt.bias_align if km else 0)
    else:
        b = _bias_f16(name, bias, outs, dev, fmt.bias_align)
    _per_group_gemm("", fmt, km, a, a_scales, w, w_scales, None if b is None else b.data_ptr(), out.data_ptr(), tokens, outs, k, ep)
    del keep
    return out


def _linear_gelu_dual(name: str, fmt, layouts: str, a, a_scales, w, w_scales, bias, return_gelu: bool, outs,
                      pair: Optional[Tuple[int, int]] = None):
    """fc1 with the GELU and the dual quantizer in the epilogue: linear_fp4_gelu_dual, linear_a6w4_gelu_dual, linear_a6w4_gelu_dual_km,
    linear_w6_gelu_dual, linear_w6_gelu_dual_km; with `pair` (the dual quantizer's table ids) linear_g6_gelu_dual"""
    require_gpu(a, name)
    if not isinstance(fmt, _Format):
        fmt = _g6_format(name, fmt)
    dev = a.device
    km, tokens, outs, k = _per_group_operands(name, fmt, a, a_scales, w, w_scales, bias, outs, layouts)
    if outs % 128 != 0:
        raise RuntimeError(f"{name}: outs must be a multiple of 128")
    out = torch.empty((tokens, outs), dtype=torch.float16, device=dev)
    h = torch.empty((tokens, outs), dtype=torch.float16, device=dev) if return_gelu else None
    b = _bias_f16(name, bias, outs, dev, fmt.bias_align)
    if tokens and outs:
        with device_guard(dev):
            flag = ops._nan_scratch(dev)
        _per_group_gemm("gelu_dual" if pair is None else "gelu_dual_pair", fmt, km, a, a_scales, w, w_scales,
                        None if b is None else b.data_ptr(), out.data_ptr(), None if h is None else h.data_ptr(), tokens, outs, k,
                        flag.data_ptr(), *(pair or ()))
    return (out, h) if return_gelu else out


def _check_cache_kv(name: str, cache_kv: torch.Tensor, device) -> None:
    if cache_kv.dim() != 5 or cache_kv.shape[0] != 2 or cache_kv.dtype != torch.float16 or not cache_kv.is_contiguous() or cache_kv.device != device:
        raise RuntimeError(f"{name}: cache_kv must be a contiguous float16 [2, B, max_len, H, c] tensor on the operands' device")


def _qkv_split_args(name: str, cache_kv: torch.Tensor, tokens: int, outs: int, bias: Optional[torch.Tensor], pos: int, seq: int,
                    qk_norm_scale: Optional[torch.Tensor]):
    """The destination side of a mat_qkv with a split output, shared by the FP4 and FP6 forms: checks that the problem fits the cache
    and the bias / head scale rules, allocates q -> (q, fpq_gemm_split_t, bias or None, head scale or None)."""
    dev = cache_kv.device
    _, bsz, max_len, heads, hd = cache_kv.shape
    c = heads * hd
    if outs != 3 * c or c % 128 != 0 or seq < 1 or tokens != bsz * seq or pos < 0 or pos + seq > max_len:
        raise RuntimeError(f"{name}: {tokens} tokens x {outs} outputs do not fit a cache of [{bsz}, {max_len}, {heads}, {hd}] at {pos} .. {pos + seq}")
    q = torch.empty((bsz, seq, c), dtype=torch.float16, device=dev)
    b = hs = None
    if qk_norm_scale is not None:
        if hd != 64:
            raise RuntimeError(f"{name}: the q / k norm needs head_dim 64, the cache has {hd}")
        if qk_norm_scale.dtype != torch.float32 or qk_norm_scale.numel() != heads or qk_norm_scale.device != dev:
            raise RuntimeError(f"{name}: qk_norm_scale must be a float32 tensor of {heads} values on the operands' device")
        hs = qk_norm_scale.detach().reshape(-1).contiguous()
        if bias is not None:
            if bias.dtype != torch.float32 or bias.numel() != outs or bias.device != dev:
                raise RuntimeError(f"{name}: with qk_norm_scale the bias must be a float32 tensor of {outs} values on the operands' device")
            b = bias.detach().reshape(-1).contiguous()
            if b.data_ptr() % 16:
                b = b.clone()
    else:
        b = _bias_f16(name, bias, outs, dev, 16)
    sp = GemmSplit()
    sp.part_cols, sp.n_parts, sp.rows_per_batch = c, 3, seq
    for p, (t, bstride, row0) in enumerate(((q, seq, 0), (cache_kv[0], max_len, pos), (cache_kv[1], max_len, pos))):
        sp.out[p], sp.row_stride[p], sp.batch_stride[p], sp.row0[p] = t.data_ptr(), c, bstride, row0
    return q, sp, b, hs


def _linear_qkv_to_cache(name: str, fmt, a, a_scales, w, w_scales, bias, cache_kv, pos: int, seq: int, qk_norm_scale,
                         layouts: str = "rank") -> torch.Tensor:
    """mat_qkv with q returned and k, v written into the cache: linear_fp4_qkv_to_cache, linear_a6w4_qkv_to_cache, linear_w6_qkv_to_cache,
    linear_w6_qkv_to_cache_km"""
    require_gpu(a, name)
    if not isinstance(fmt, _Format):
        fmt = _g6_format(name, fmt)
    _check_cache_kv(name, cache_kv, a.device)
    km, tokens, outs, k = _per_group_operands(name, fmt, a, a_scales, w, w_scales, None, 3 * cache_kv.shape[3] * cache_kv.shape[4], layouts)
    if fmt.split_w_f32 and w_scales.dtype != torch.float32:
        raise RuntimeError(f"{name}: the weight scales must be float32, got {w_scales.dtype}")
    q, sp, b, hs = _qkv_split_args(name, cache_kv, tokens, outs, bias, pos, seq, qk_norm_scale)
    if tokens:
        norm = () if hs is None else (hs.data_ptr(),)
        _per_group_gemm("split" if hs is None else "split_qknorm", fmt, km, a, a_scales, w, w_scales, None if b is None else b.data_ptr(),
                        tokens, outs, k, ctypes.byref(sp), *norm)
    return q


def sqerr_workspace_bytes(tokens: int, outs: int) -> int:
    """bytes of device scratch a linear_*_sqerr call of these sizes needs (fpq_gemm_sqerr_workspace_bytes)"""
    n = lib().fpq_gemm_sqerr_workspace_bytes(int(tokens), int(outs))
    check(min(n, 0), "fpq_gemm_sqerr_workspace_bytes")
    return n


def _sqerr_args(name: str, tokens: int, outs: int, device, ref, row_weight, out, workspace):
    """The squared-error forms' own arguments, checked behind the family's operands -> (ref pointer, its dtype id, weight pointer,
    out, workspace).  The workspace is torch's (the caching allocator hands the same block back call after call, in stream order),
    as ops.sqerr_rows_weighted's is, unless the caller passes one."""
    if ref.dtype not in (torch.float16, torch.float32) or tuple(ref.shape) != (tokens, outs) or not ref.is_contiguous() or ref.device != device:
        raise RuntimeError(f"{name}: ref must be a contiguous float16 / float32 [{tokens}, {outs}] tensor on {device}")
    if row_weight.dtype != torch.float32 or row_weight.numel() != tokens or not row_weight.is_contiguous() or row_weight.device != device:
        raise RuntimeError(f"{name}: row_weight must be a contiguous float32 tensor of {tokens} values on {device}")
    if out is None:
        out = torch.empty(1, dtype=torch.float32, device=device)
    elif out.dtype != torch.float32 or out.numel() != 1 or out.device != device:
        raise RuntimeError(f"{name}: out must be a float32 view of one element on {device}")
    need = sqerr_workspace_bytes(tokens, outs)
    if workspace is None:
        workspace = torch.empty(need // 4, dtype=torch.float32, device=device)
    elif workspace.dtype != torch.float32 or workspace.numel() * 4 < need or not workspace.is_contiguous() or workspace.device != device:
        raise RuntimeError(f"{name}: workspace must be a contiguous float32 tensor of at least {need // 4} elements on {device}")
    return ref.data_ptr(), dtype_id(ref.dtype), row_weight.data_ptr(), out, workspace


def _linear_sqerr(name: str, fmt, a, a_scales, w, w_scales, ref, row_weight, out, bias, workspace) -> torch.Tensor:
    """The plain Linear's product with the loss against `ref` in the GEMM's epilogue and no output tensor: linear_fp4_sqerr,
    linear_a6w4_sqerr, linear_w6_sqerr"""
    require_gpu(a, name)
    if not isinstance(fmt, _Format):
        fmt = _g6_format(name, fmt)
    dev = a.device
    _, tokens, outs, k = _per_group_operands(name, fmt, a, a_scales, w, w_scales, bias, None, "rows")
    b = _bias_f16(name, bias, outs, dev, fmt.bias_align)
    pr, rdt, pw, out, ws = _sqerr_args(name, tokens, outs, dev, ref, row_weight, out, workspace)
    _per_group_gemm("sqerr", fmt, False, a, a_scales, w, w_scales, None if b is None else b.data_ptr(), pr, rdt, pw, out.data_ptr(),
                    ws.data_ptr(), tokens, outs, k)
    return out


def linear_fp4_sqerr(a_codes: torch.Tensor, a_scales: torch.Tensor, w_codes: torch.Tensor, w_scales: torch.Tensor, ref: torch.Tensor,
                     row_weight: torch.Tensor, out: Optional[torch.Tensor] = None, bias: Optional[torch.Tensor] = None,
                     workspace: Optional[torch.Tensor] = None) -> torch.Tensor:
    """The format search's loss of a candidate pair, computed where its product is (fpq_gemm_fp4_sqerr): a one-element float32
    tensor, sum_t row_weight[t] sum_o (ref[t, o] - y[t, o])^2 in fp32 with y = linear_fp4(a, w, bias) bit for bit - which is never
    written.  Row-major operands; ref [tokens, outs] float16 or float32; row_weight float32 [tokens], finite and positive; out: a
    float32 view of one element (an entry of a loss table), allocated when None; workspace: float32 scratch of
    sqerr_workspace_bytes(tokens, outs), allocated when None.  Deterministic; no synchronisation."""
    return _linear_sqerr("linear_fp4_sqerr", _FORMATS["e2m1"], a_codes, a_scales, w_codes, w_scales, ref, row_weight, out, bias, workspace)


def linear_a6w4_sqerr(a_codes: torch.Tensor, a_scales: torch.Tensor, a_table: str, w_codes: torch.Tensor, w_scales: torch.Tensor,
                      ref: torch.Tensor, row_weight: torch.Tensor, out: Optional[torch.Tensor] = None, bias: Optional[torch.Tensor] = None,
                      workspace: Optional[torch.Tensor] = None) -> torch.Tensor:
    """linear_fp4_sqerr for a 6-bit activation against the E2M1 weight (fpq_gemm_a6w4_sqerr): the loss of y = linear_a6w4(a, a_table,
    w, bias) against ref."""
    return _linear_sqerr("linear_a6w4_sqerr", a_table, a_codes, a_scales, w_codes, w_scales, ref, row_weight, out, bias, workspace)


def linear_w6_sqerr(a_codes: torch.Tensor, a_scales: torch.Tensor, a_table: str, w_codes: torch.Tensor, w_scales: torch.Tensor, w_table: str,
                    ref: torch.Tensor, row_weight: torch.Tensor, out: Optional[torch.Tensor] = None, bias: Optional[torch.Tensor] = None,
                    workspace: Optional[torch.Tensor] = None) -> torch.Tensor:
    """linear_fp4_sqerr for a 6-bit WEIGHT (fpq_gemm_w6_sqerr): the loss of y = linear_w6(a, a_table, w, w_table, bias) against ref."""
    require_gpu(a_codes, "linear_w6_sqerr")
    fmt = _w6_format("linear_w6_sqerr", a_table, w_table, w_scales)
    return _linear_sqerr("linear_w6_sqerr", fmt, a_codes, a_scales, w_codes, w_scales, ref, row_weight, out, bias, workspace)


def linear_fp4(a_codes: torch.Tensor, a_scales: torch.Tensor, w_codes: torch.Tensor, w_scales: torch.Tensor,
               bias: Optional[torch.Tensor] = None, gate: Optional[torch.Tensor] = None,
               residual: Optional[torch.Tensor] = None, outs: Optional[int] = None) -> torch.Tensor:
    """fp16 [tokens, outs] = dequant(a) @ dequant(w).T + bias on the FP4 matrix cores; with gate / residual the
    AdaLN block's `residual + y.mul(gate)` (tr/basic_var.py:264) is applied in the epilogue, bit-identical to the two
    torch ops on the plain result."""
    if _native is not None:   # same checks, same C calls (fpq_gemm_fp4_mx_ex / fpq_gemm_fp4_mx_km)
        return _native.linear_fp4(a_codes, a_scales, w_codes, w_scales, bias, gate, residual, outs)
    return _linear("linear_fp4", _FORMATS["e2m1"], "rank", a_codes, a_scales, w_codes, w_scales, bias, gate, residual, outs, True)


def linear_fp4_qkv_to_cache(a_codes: torch.Tensor, a_scales: torch.Tensor, w_codes: torch.Tensor, w_scales: torch.Tensor,
                            bias: Optional[torch.Tensor], cache_kv: torch.Tensor, pos: int, seq: int,
                            qk_norm_scale: Optional[torch.Tensor] = None) -> torch.Tensor:
    """mat_qkv of an attention block with a split output (fpq_gemm_fp4_mx_split): `qkv = linear_fp4(a, w, bias)` for tokens
    [B * seq] and outs = 3 * C, but only q comes back - fp16 [B, seq, C] - while k and v are written straight into the KV cache
    `cache_kv` [2, B, max_len, H, c] (C = H * c) at token positions pos .. pos + seq: what `qkv.view(B, L, 3, H, c).unbind(2)`
    followed by the cache's copy-in (tr/basic_var.py:173-209; kv_cache.IncrementalKVCache.append) leaves there, without the copy.
    Operands row-major (2-D) or k-major images (3-D) as in linear_fp4.

    qk_norm_scale: fp32 [H] (kv_cache.qk_norm_head_scale) - the attention block has attn_l2_norm (fpq_gemm_fp4_mx_split_qknorm):
    y = float(fp16 Linear output) + bias (fp32 [3C] or None: q_bias, 0, v_bias, added after the fp16 rounding), q =
    F.normalize(y_q) * qk_norm_scale per head, k = F.normalize(y_k) into the cache, v = y_v (tr/basic_var.py:173-183), head_dim 64."""
    return _linear_qkv_to_cache("linear_fp4_qkv_to_cache", _FORMATS["e2m1"], a_codes, a_scales, w_codes, w_scales, bias, cache_kv, pos, seq,
                                qk_norm_scale)


def linear_fp4_gelu_dual(a_codes: torch.Tensor, a_scales: torch.Tensor, w_codes: torch.Tensor, w_scales: torch.Tensor,
                         bias: Optional[torch.Tensor] = None, return_gelu: bool = False, outs: Optional[int] = None):
    """fc1 of the AdaLN block's FFN up to fc2's GEMM in ONE launch (+ the dual quantizer's tiny NaN fix-up launch):
    `fp_quant_e1m2_neg_e2m1_pos_per_group_cuda(F.gelu(linear_fp4(a, w, bias), approximate="tanh"), 4, 128)`
    (tr/basic_var.py:120-121, tr/quant_utils.py:415-452,991) as the epilogue of the FP4 GEMM (fpq_gemm_fp4_gelu_dual):
    fp16 [tokens, outs], outs % 128 == 0.  return_gelu: also the GELU values the quantizer saw - the quantization is
    bit-exact on THOSE, they sit within one fp16 ulp of torch's GELU of the Linear output."""
    if _native is not None:   # same checks, same C calls, the binding's own NaN scratch
        out, h = _native.linear_fp4_gelu_dual(a_codes, a_scales, w_codes, w_scales, bias, return_gelu, outs)
        return (out, h) if return_gelu else out
    return _linear_gelu_dual("linear_fp4_gelu_dual", _FORMATS["e2m1"], "rank", a_codes, a_scales, w_codes, w_scales, bias, return_gelu, outs)


def fp4_tiling(tokens: int, outs: int, k: int, form: str = "linear") -> int:
    """The FPQ_GEMM_CFG code (10 / 20 / 30 / 40) of the LDS-DMA tiling a linear_fp4 / linear_fp4_qkv_to_cache call (form "linear")
    or a linear_fp4_gelu_dual call (form "fc1") of these sizes runs under the current FPQ_GEMM_CFG (fpq_gemm_fp4_tiling; 0 when
    tokens or outs is zero).  Host arithmetic only; raises for a shape the GEMM refuses."""
    if form not in ("linear", "fc1"):
        raise ValueError(f"fp4_tiling: form {form!r} (linear | fc1)")
    rc = lib().fpq_gemm_fp4_tiling(int(tokens), int(outs), int(k), 1 if form == "fc1" else 0)
    check(min(rc, 0), "fpq_gemm_fp4_tiling")
    return rc


def linear_a6w4(a_codes: torch.Tensor, a_scales: torch.Tensor, a_table: str, w_codes: torch.Tensor, w_scales: torch.Tensor,
                bias: Optional[torch.Tensor] = None, gate: Optional[torch.Tensor] = None,
                residual: Optional[torch.Tensor] = None) -> torch.Tensor:
    """fp16 [tokens, outs] = dequantize_g6(a) @ dequantize_mx(w).T + bias on the matrix cores (fpq_gemm_a6w4_mx): a 6-bit
    activation fragment of `a_table` ('e1m2' / 'e3m0') against the E2M1 weight nibbles `quantize_mx` emits; gate / residual as
    in linear_fp4.  Row-major operands only."""
    return _linear("linear_a6w4", a_table, "rows", a_codes, a_scales, w_codes, w_scales, bias, gate, residual, None)


def linear_a6w4_gelu_dual(a_codes: torch.Tensor, a_scales: torch.Tensor, a_table: str, w_codes: torch.Tensor, w_scales: torch.Tensor,
                          bias: Optional[torch.Tensor] = None, return_gelu: bool = False):
    """linear_fp4_gelu_dual for a 6-bit activation (fpq_gemm_a6w4_gelu_dual): fc1 of the FFN up to fc2's GEMM in one launch (+ the
    NaN fix-up launch) - `fp_quant_e1m2_neg_e2m1_pos_per_group_cuda(F.gelu(linear_a6w4(a, a_table, w, bias), approximate="tanh"),
    4, 128)` as the epilogue of the A6W4 GEMM: fp16 [tokens, outs], outs % 128 == 0.  Row-major operands only.  return_gelu: also
    the GELU values the quantizer saw - the same function of the fp16 Linear output as linear_fp4_gelu_dual's, bit for bit."""
    return _linear_gelu_dual("linear_a6w4_gelu_dual", a_table, "rows", a_codes, a_scales, w_codes, w_scales, bias, return_gelu, None)


def linear_a6w4_km(a_image: torch.Tensor, a_scales: torch.Tensor, a_table: str, w_image: torch.Tensor, w_scales: torch.Tensor,
                   bias: Optional[torch.Tensor] = None, gate: Optional[torch.Tensor] = None,
                   residual: Optional[torch.Tensor] = None, outs: Optional[int] = None) -> torch.Tensor:
    """linear_a6w4 on k-major images (fpq_gemm_a6w4_mx_km), bit for bit the same result: the activation as `quantize_g6(x, table,
    kmajor=True)` emits it, the weight exactly as a k-major FP4Linear holds it (`to_kmajor(codes, 4, dealt=True)`,
    `to_kmajor_scales(scales, weight_side=True)`).  outs: the Linear's width when it is neither the bias's length nor the weight
    image's row count (a multiple of 64), as in linear_fp4."""
    return _linear("linear_a6w4_km", a_table, "images", a_image, a_scales, w_image, w_scales, bias, gate, residual, outs)


def linear_a6w4_gelu_dual_km(a_image: torch.Tensor, a_scales: torch.Tensor, a_table: str, w_image: torch.Tensor, w_scales: torch.Tensor,
                             bias: Optional[torch.Tensor] = None, return_gelu: bool = False, outs: Optional[int] = None):
    """linear_a6w4_gelu_dual on k-major images (fpq_gemm_a6w4_gelu_dual_km), bit for bit the same result; operands as in
    linear_a6w4_km, return_gelu as in linear_a6w4_gelu_dual."""
    return _linear_gelu_dual("linear_a6w4_gelu_dual_km", a_table, "images", a_image, a_scales, w_image, w_scales, bias, return_gelu, outs)


def linear_a6w4_qkv_to_cache(a_codes: torch.Tensor, a_scales: torch.Tensor, a_table: str, w_codes: torch.Tensor, w_scales: torch.Tensor,
                             bias: Optional[torch.Tensor], cache_kv: torch.Tensor, pos: int, seq: int,
                             qk_norm_scale: Optional[torch.Tensor] = None) -> torch.Tensor:
    """linear_fp4_qkv_to_cache for a 6-bit activation (fpq_gemm_a6w4_mx_split / fpq_gemm_a6w4_mx_split_qknorm): mat_qkv of an attention
    block whose activation format is E1M2 / E3M0 - `qkv = linear_a6w4(a, a_table, w, bias)` for tokens [B * seq] and outs = 3 * C, but
    only q comes back, fp16 [B, seq, C], while k and v are written straight into `cache_kv` [2, B, max_len, H, c] at token positions
    pos .. pos + seq, bit for bit what the plain GEMM and the cache's copy-in leave there.  Operands row-major (2-D, as linear_a6w4
    takes them) or k-major images (3-D, as linear_a6w4_km takes them), both of the same kind; fp32 weight scales (what quantize_mx
    gives an fp32 weight and FP4Linear holds) - these forms are not compiled for fp16 ones.
    qk_norm_scale, and the fp32 bias that goes with it: as in linear_fp4_qkv_to_cache."""
    return _linear_qkv_to_cache("linear_a6w4_qkv_to_cache", a_table, a_codes, a_scales, w_codes, w_scales, bias, cache_kv, pos, seq, qk_norm_scale)


def linear_w6(a_codes: torch.Tensor, a_scales: torch.Tensor, a_table: str, w_codes: torch.Tensor, w_scales: torch.Tensor, w_table: str,
              bias: Optional[torch.Tensor] = None, gate: Optional[torch.Tensor] = None, residual: Optional[torch.Tensor] = None,
              outs: Optional[int] = None) -> torch.Tensor:
    """fp16 [tokens, outs] = dequantize(a) @ dequantize_g6(w, w_table).T + bias on the matrix cores (fpq_gemm_w6_mx): an E1M2 / E3M0
    WEIGHT as the dense 6-bit codes and fp32 group scales of `quantize_g6(weight.float(), w_table)`, against an activation in any of
    the three FP4 formats - a_table "e2m1": the nibbles and fp16 scales of quantize_mx; "e1m2" / "e3m0": the 6-bit codes of quantize_g6.
    Row-major operands only (k-major images: linear_w6_km).  gate / residual: the AdaLN block's tail as in linear_fp4.  outs: the
    weight's row count, when given."""
    require_gpu(a_codes, "linear_w6")
    fmt = _w6_format("linear_w6", a_table, w_table, w_scales)
    if outs is not None and w_codes.dim() == 2 and outs != w_codes.shape[0]:
        raise RuntimeError(f"linear_w6: outs = {outs}, but the weight has {w_codes.shape[0]} rows")
    return _linear("linear_w6", fmt, "rows", a_codes, a_scales, w_codes, w_scales, bias, gate, residual, None)


def _w6_format(name: str, a_table: str, w_table: str, w_scales: torch.Tensor) -> _Format:
    """the row of an (activation, weight) pair of the W6 family, and its one weight scale dtype"""
    a_table = "e2m1" if a_table in ("e2m1", "fp_e2") else _g6_table(name, a_table)
    fmt = _W6_FORMATS[a_table, _g6_table(name, w_table)]
    if w_scales.dtype != torch.float32:
        raise RuntimeError(f"{name}: the weight scales must be float32 (what quantize_g6 writes for an fp32 weight)")
    return fmt


def linear_w6_gelu_dual(a_codes: torch.Tensor, a_scales: torch.Tensor, a_table: str, w_codes: torch.Tensor, w_scales: torch.Tensor, w_table: str,
                        bias: Optional[torch.Tensor] = None, return_gelu: bool = False):
    """linear_a6w4_gelu_dual for a 6-bit WEIGHT (fpq_gemm_w6_gelu_dual): fc1 of the FFN up to fc2's GEMM in one launch (+ the NaN fix-up
    launch) - `fp_quant_e1m2_neg_e2m1_pos_per_group_cuda(F.gelu(linear_w6(a, a_table, w, w_table, bias), approximate="tanh"), 4, 128)` as
    the epilogue of the W6 GEMM: fp16 [tokens, outs], outs % 128 == 0.  Operands as linear_w6 takes them: row-major only (k-major
    images: linear_w6_gelu_dual_km), float32 weight scales.  return_gelu: also the GELU values the quantizer saw - the same function of the fp16 Linear output as
    linear_fp4_gelu_dual's, bit for bit."""
    require_gpu(a_codes, "linear_w6_gelu_dual")
    fmt = _w6_format("linear_w6_gelu_dual", a_table, w_table, w_scales)
    return _linear_gelu_dual("linear_w6_gelu_dual", fmt, "rows", a_codes, a_scales, w_codes, w_scales, bias, return_gelu, None)


def linear_w6_qkv_to_cache(a_codes: torch.Tensor, a_scales: torch.Tensor, a_table: str, w_codes: torch.Tensor, w_scales: torch.Tensor,
                           w_table: str, bias: Optional[torch.Tensor], cache_kv: torch.Tensor, pos: int, seq: int,
                           qk_norm_scale: Optional[torch.Tensor] = None) -> torch.Tensor:
    """linear_a6w4_qkv_to_cache for a 6-bit WEIGHT (fpq_gemm_w6_mx_split / fpq_gemm_w6_mx_split_qknorm): mat_qkv of an attention block
    whose weight format is E1M2 / E3M0 - `qkv = linear_w6(a, a_table, w, w_table, bias)` for tokens [B * seq] and outs = 3 * C, but only
    q comes back, fp16 [B, seq, C], while k and v are written straight into `cache_kv` [2, B, max_len, H, c] at token positions
    pos .. pos + seq, bit for bit what the plain GEMM and the cache's copy-in leave there.  Operands as linear_w6 takes them: row-major
    only (k-major images: linear_w6_qkv_to_cache_km), float32 weight scales.  qk_norm_scale, and the fp32 bias that goes with it: as in
    linear_fp4_qkv_to_cache."""
    require_gpu(a_codes, "linear_w6_qkv_to_cache")
    fmt = _w6_format("linear_w6_qkv_to_cache", a_table, w_table, w_scales)
    return _linear_qkv_to_cache("linear_w6_qkv_to_cache", fmt, a_codes, a_scales, w_codes, w_scales, bias, cache_kv, pos, seq, qk_norm_scale)


def linear_w6_km(a_image: torch.Tensor, a_scales: torch.Tensor, a_table: str, w_image: torch.Tensor, w_scales: torch.Tensor, w_table: str,
                 bias: Optional[torch.Tensor] = None, gate: Optional[torch.Tensor] = None, residual: Optional[torch.Tensor] = None,
                 outs: Optional[int] = None) -> torch.Tensor:
    """linear_w6 on k-major images (fpq_gemm_w6_mx_km), bit for bit the same result: the activation as the `kmajor=True` quantizer of
    its format emits it - a_table "e2m1": `quantize_mx(x, kmajor=True)`, codes [K/128, tokens, 64]; "e1m2" / "e3m0": `quantize_g6(x, table,
    kmajor=True)`, codes [K/128, tokens, 96]; scales fp32 [K/128, tokens rounded up to 4] in all three - and the weight as
    `to_kmajor(codes, 6, dealt=True)` [K/128, outs rounded up to 64, 96] with `to_kmajor_scales(scales, weight_side=True)` of
    `quantize_g6(weight.float(), w_table)`.  outs: the Linear's width when it is neither the bias's length nor the weight image's row
    count (a multiple of 64), as in linear_fp4."""
    require_gpu(a_image, "linear_w6_km")
    fmt = _w6_format("linear_w6_km", a_table, w_table, w_scales)
    return _linear("linear_w6_km", fmt, "images", a_image, a_scales, w_image, w_scales, bias, gate, residual, outs)


def linear_w6_gelu_dual_km(a_image: torch.Tensor, a_scales: torch.Tensor, a_table: str, w_image: torch.Tensor, w_scales: torch.Tensor,
                           w_table: str, bias: Optional[torch.Tensor] = None, return_gelu: bool = False, outs: Optional[int] = None):
    """linear_w6_gelu_dual on k-major images (fpq_gemm_w6_gelu_dual_km), bit for bit the same result; operands as in linear_w6_km,
    return_gelu as in linear_w6_gelu_dual."""
    require_gpu(a_image, "linear_w6_gelu_dual_km")
    fmt = _w6_format("linear_w6_gelu_dual_km", a_table, w_table, w_scales)
    return _linear_gelu_dual("linear_w6_gelu_dual_km", fmt, "images", a_image, a_scales, w_image, w_scales, bias, return_gelu, outs)


def linear_w6_qkv_to_cache_km(a_image: torch.Tensor, a_scales: torch.Tensor, a_table: str, w_image: torch.Tensor, w_scales: torch.Tensor,
                              w_table: str, bias: Optional[torch.Tensor], cache_kv: torch.Tensor, pos: int, seq: int,
                              qk_norm_scale: Optional[torch.Tensor] = None) -> torch.Tensor:
    """linear_w6_qkv_to_cache on k-major images (fpq_gemm_w6_mx_split_km / fpq_gemm_w6_mx_split_qknorm_km), bit for bit the same q and
    cache entries; operands as in linear_w6_km (the width is the cache's: 3 * H * c, whose weight image has exactly that many rows)."""
    require_gpu(a_image, "linear_w6_qkv_to_cache_km")
    fmt = _w6_format("linear_w6_qkv_to_cache_km", a_table, w_table, w_scales)
    return _linear_qkv_to_cache("linear_w6_qkv_to_cache_km", fmt, a_image, a_scales, w_image, w_scales, bias, cache_kv, pos, seq,
                                qk_norm_scale, "images")


# form -> the public function for E2M1 operands, for 6-bit row-major codes and for 6-bit k-major images
_FORMS = {"plain": (linear_fp4, linear_a6w4, linear_a6w4_km),
          "gelu_dual": (linear_fp4_gelu_dual, linear_a6w4_gelu_dual, linear_a6w4_gelu_dual_km),
          "qkv_to_cache": (linear_fp4_qkv_to_cache, linear_a6w4_qkv_to_cache, linear_a6w4_qkv_to_cache)}
# form -> the public function for a 6-bit weight, row-major and on k-major images (the forms beside "plain" need the module's w6_forms)
_W6_FORMS = {"plain": (linear_w6, linear_w6_km), "gelu_dual": (linear_w6_gelu_dual, linear_w6_gelu_dual_km),
             "qkv_to_cache": (linear_w6_qkv_to_cache, linear_w6_qkv_to_cache_km)}


class FP4Linear(_ScaledOperandModule):
    """Drop-in for QuantizedLinear in the W4A4 per-group `fp_e2` configuration that runs on the FP4
    matrix cores instead of simulating FP4 in fp16: weights are stored as hardware E2M1 codes + one
    fp32 scale per 128 input channels (4.25 bits per weight instead of 16), the
    activation is quantized to codes on the fly, the product is `fpq_gemm_fp4_mx`.
    Same quantization decisions as the reference (codes * scale == its fake-quantized tensors bit for
    bit); the GEMM itself is more exact than the reference's fp16 GEMM (tolerance-level agreement)."""

    def __init__(self, w_codes, w_scales, bias, in_features, out_features, act_table: str = "e2m1", w_table: str = "e2m1",
                 w6_forms: bool = False):
        super().__init__()
        self.in_features, self.out_features = in_features, out_features
        self.act_table = act_table   # "e2m1": nibbles on the FP4 GEMM; "e1m2" / "e3m0": 6-bit codes on the A6W4 GEMM, same weight
        self.w_table = w_table       # "e2m1": nibbles; "e1m2" / "e3m0": 6-bit codes on the W6 GEMM (linear_w6), any activation format
        self.w6_forms = bool(w6_forms)   # a 6-bit weight also runs the W6 GEMM's fc1 tail and split output (else: the plain form only)
        self.register_buffer("w_codes", w_codes)
        self.register_buffer("w_scales", w_scales)
        self.register_buffer("bias", bias)

    @property
    def kmajor(self) -> bool:
        """the weight is held as a k-major image (to_kmajor(..., dealt=True)): activations must come as images too"""
        return self.w_codes.dim() == 3

    @classmethod
    def from_float(cls, module: torch.nn.Linear, kmajor: bool = False, act_fp_type: str = "fp_e2", a6w4_kmajor: bool = False,
                   weight_fp_type: str = "fp_e2", w6_forms: bool = False, w6_kmajor: bool = False):
        """act_fp_type: the activation's per-group format - "fp_e2" (E2M1, the FP4 GEMM) or "fp_e1" / "fp_e3" (E1M2 / E3M0: the
        A6W4 GEMM on the same stored weight - row-major unless a6w4_kmajor, which lets kmajor=True hold the FP4 GEMM's k-major
        weight images for it and run quantize_g6(kmajor=True) + linear_a6w4_km).
        weight_fp_type: the weight's per-group format - "fp_e2" (E2M1 nibbles, as above) or "fp_e1" / "fp_e3": the weight is held as
        the 6-bit codes and fp32 scales of quantize_g6(weight.float(), table) and the product runs on linear_w6 for any of the three
        activation formats (an E2M1 activation as quantize_mx's row-major nibbles).  Row-major, plain form only: kmajor /
        a6w4_kmajor, qkv_to_cache* and FP4LinearGeluDual raise ValueError.
        w6_forms (with a 6-bit weight; an E2M1 weight ignores it): the module also runs the W6 GEMM's fc1 tail and split output -
        FP4LinearGeluDual constructs (linear_w6_gelu_dual) and qkv_to_cache* work (linear_w6_qkv_to_cache).  Row-major unless
        w6_kmajor: kmajor / a6w4_kmajor raise as before.
        w6_kmajor (with a 6-bit weight and kmajor=True; alone it changes nothing, and an E2M1 weight ignores it): the module holds the
        dealt 6-bit weight image `to_kmajor(codes, 6, dealt=True)` and `to_kmajor_scales(scales, weight_side=True)`, quantizes its
        activation with the kmajor=True quantizer of its format and runs the W6 GEMM's k-major forms (linear_w6_km,
        linear_w6_gelu_dual_km, linear_w6_qkv_to_cache_km) - the same bits as the row-major module."""
        assert isinstance(module, torch.nn.Linear) and module.in_features % 128 == 0 and module.out_features % 8 == 0
        if weight_fp_type not in ("fp_e2", "e2m1"):
            w_table = _G6_TABLES.get(weight_fp_type) if isinstance(weight_fp_type, str) else None
            if w_table is None:
                raise ValueError(f"FP4Linear.from_float: weight_fp_type must be 'fp_e2', 'fp_e1' or 'fp_e3', got {weight_fp_type!r}")
            km6 = bool(kmajor and w6_kmajor)
            if (kmajor or a6w4_kmajor) and not km6:
                raise ValueError(f"FP4Linear.from_float: weight_fp_type={weight_fp_type!r} runs on the W6 GEMM, which has no k-major form "
                                 "unless w6_kmajor=True asks for it (together with kmajor=True)")
            if issubclass(cls, FP4LinearGeluDual) and not w6_forms:
                raise ValueError(f"FP4LinearGeluDual.from_float: weight_fp_type={weight_fp_type!r} runs on the W6 GEMM, which has no fc1 tail")
            act_table = "e2m1" if act_fp_type in ("fp_e2", "e2m1") else _g6_table("FP4Linear.from_float", act_fp_type)
            codes, scales, bias = _weight_operands(f"{cls.__name__}.from_float", module, w_table, km6)
            return cls(codes, scales, bias, module.in_features, module.out_features, act_table, w_table, w6_forms=w6_forms)
        if act_fp_type in ("fp_e2", "e2m1"):
            act_table = "e2m1"
        else:
            act_table = _g6_table("FP4Linear.from_float", act_fp_type)
            if kmajor and not a6w4_kmajor:
                raise ValueError(f"FP4Linear.from_float: act_fp_type={act_fp_type!r} runs on the A6W4 GEMM, which has no k-major form "
                                 "unless a6w4_kmajor=True asks for it (kmajor=True alone needs act_fp_type='fp_e2')")
        codes, scales, bias = _weight_operands(f"{cls.__name__}.from_float", module, "e2m1", kmajor)
        return cls(codes, scales, bias, module.in_features, module.out_features, act_table)

    def extra_repr(self) -> str:
        return f"in_features={self.in_features}, out_features={self.out_features}, act={self.act_table}, w={self.w_table}"

    def _quantize(self, x) -> Tuple[torch.Tensor, torch.Tensor]:
        """x [..., in_features] -> (codes, scales) in the module's own activation format and layout"""
        fmt = _FORMATS[self.act_table]
        return _quantize_per_group(fmt.quantizer, fmt, x.to(torch.float16).reshape(-1, self.in_features), self.kmajor)

    def _run(self, form: str, table: Optional[str], a_codes, a_scales, *rest):
        """`form` of the product (a key of _FORMS) on operands whose codes are in `table` (None: the module's activation format) ->
        what the public function of that format and of the weight's layout returns; rest: its arguments from the bias up to `outs`."""
        if table is None:
            table = self.act_table
        elif table in ("e2m1", "fp_e2"):
            table = "e2m1"
        else:
            table = _g6_table(f"{type(self).__name__}.forward_operands", table)
        if self.w_table != "e2m1":   # a 6-bit weight: the W6 GEMM, in the weight's layout; the forms beside the plain one with w6_forms only
            if form != "plain" and not self.w6_forms:
                raise ValueError(f"{type(self).__name__}: a {self.w_table} weight runs on the W6 GEMM, which has the plain form only "
                                 f"(no {form} form)")
            rows, images = _W6_FORMS[form]
            if not self.kmajor:
                return rows(a_codes, a_scales, table, self.w_codes, self.w_scales, self.w_table, *rest)
            outs = () if form == "qkv_to_cache" else (self.out_features,)
            return images(a_codes, a_scales, table, self.w_codes, self.w_scales, self.w_table, *rest, *outs)
        fp4, rows, images = _FORMS[form]
        outs = () if form == "qkv_to_cache" else (self.out_features,)   # the last argument; mat_qkv's width is the cache's
        if table == "e2m1":   # the public functions: they hand the call to the compiled binding when it is loaded
            return fp4(a_codes, a_scales, self.w_codes, self.w_scales, *rest, *outs)
        if not self.kmajor:
            return rows(a_codes, a_scales, table, self.w_codes, self.w_scales, *rest)
        if a_codes.dim() != 3:
            raise RuntimeError(f"{type(self).__name__}.forward_operands: the weight is a k-major image - 6-bit activation codes must come as "
                               "the k-major images of quantize_g6(kmajor=True), not as row-major codes")
        return images(a_codes, a_scales, table, self.w_codes, self.w_scales, *rest, *outs)

    @torch.no_grad()
    def forward(self, x, gate=None, residual=None):
        """gate / residual: the AdaLN block's `residual + y.mul(gate)` fused into the GEMM (see linear_fp4)."""
        return self._run("plain", None, *self._quantize(x), self.bias, gate, residual).view(*x.shape[:-1], self.out_features)

    @torch.no_grad()
    def qkv_to_cache(self, x, cache_kv: torch.Tensor, pos: int, seq: int, qk_norm_scale: Optional[torch.Tensor] = None,
                     bias: Optional[torch.Tensor] = None) -> torch.Tensor:
        """mat_qkv with a split output: `forward(x)` for x [B, seq, in_features] and out_features = 3 * C, but only q comes back
        ([B, seq, C]) while k and v go straight into `cache_kv` [2, B, max_len, H, c] at pos .. pos + seq.  x is quantized in the
        module's own activation format and layout, and the product runs on the GEMM that format has (linear_fp4_qkv_to_cache for
        E2M1, linear_a6w4_qkv_to_cache for E1M2 / E3M0): one call drives every mat_qkv of a mixed-format model.
        Without qk_norm_scale the module's fp16 bias is added and `bias` must be None.  With qk_norm_scale (fp32 [H]: the block has
        attn_l2_norm) `bias` is the fp32 cat(q_bias, 0, v_bias) [3 * C] or None, added after the fp16 rounding, and the module itself
        must have no bias (mat_qkv has none in the reference)."""
        self._no_w6("qkv_to_cache")
        bias = self._qkv_bias("qkv_to_cache", qk_norm_scale, bias)
        return self._run("qkv_to_cache", None, *self._quantize(x), bias, cache_kv, pos, seq, qk_norm_scale)

    def _no_w6(self, form: str) -> None:
        if self.w_table != "e2m1" and not self.w6_forms:
            raise ValueError(f"{type(self).__name__}.{form}: a {self.w_table} weight runs on the W6 GEMM, which has the plain form only")

    def _qkv_bias(self, name: str, qk_norm_scale, bias):
        """the bias of the split mat_qkv: the module's own without the q / k norm, the caller's fp32 one with it"""
        if qk_norm_scale is None:
            if bias is not None:
                raise RuntimeError(f"FP4Linear.{name}: `bias` is the fp32 bias of the q / k norm form - without qk_norm_scale the "
                                   "module's own bias is used")
            return self.bias
        if self.bias is not None:
            raise RuntimeError(f"FP4Linear.{name}: with qk_norm_scale the Linear itself must have no bias (pass cat(q_bias, 0, v_bias) "
                               "as `bias`)")
        return bias

    @torch.no_grad()
    def qkv_to_cache_operands(self, a_codes: torch.Tensor, a_scales: torch.Tensor, cache_kv: torch.Tensor, pos: int, seq: int,
                              qk_norm_scale: Optional[torch.Tensor] = None, bias: Optional[torch.Tensor] = None) -> torch.Tensor:
        """`qkv_to_cache` for an activation that already is in operand form (the module's own format and layout: what
        `adaln_operands` / `rotate_operands` return): producer -> split GEMM -> cache without the activation in HBM as fp16."""
        self._no_w6("qkv_to_cache_operands")
        return self._run("qkv_to_cache", None, a_codes, a_scales, self._qkv_bias("qkv_to_cache_operands", qk_norm_scale, bias), cache_kv, pos, seq, qk_norm_scale)

    @torch.no_grad()
    def adaln_operands(self, x, scale, shift, d: Optional[torch.Tensor] = None, smooth: Optional[torch.Tensor] = None,
                       eps: float = 1e-6, pending: Optional[Tuple[torch.Tensor, torch.Tensor]] = None, full_width: bool = False):
        """The block's producer in front of this Linear - LayerNorm, adaLN modulate, smooth, rotate, per-group quantize of x [B, L,
        in_features] - in one launch, emitting (codes, scales) in the module's own activation format and layout
        (`rotation.adaln_rotate_quant_mx` for E2M1, `rotation.adaln_rotate_quant_g6` for E1M2 / E3M0; k-major iff the weight is):
        ready for `forward_operands` / `qkv_to_cache_operands`.  One call in front of every mat_qkv and fc1 of a mixed-format model.
        pending = (y, gate): a gated residual x + y.mul(gate) that has not been applied to x yet - what `ops.gate_residual(y, gate, x)`
        would compute - is applied by the same launch (`rotation.resid_adaln_rotate_quant_mx`, E2M1 activations, in_features <= 2560):
        returns (x_new, codes, scales), x_new and the operands bit for bit those of the two calls.
        full_width: the full-width rotation of `rotate_model(block_rotate=False)` instead of the 128-block form
        (`rotation.adaln_rotate_quant_full_mx`; d: in_features signs) - E2M1 activations only, no pending=."""
        from . import rotation
        if full_width:
            if self.act_table != "e2m1":
                raise NotImplementedError(f"adaln_operands(full_width=True): the fused full-width rotation emits E2M1 (FP4) operands only, "
                                          f"not {self.act_table!r} - 6-bit operand forms are outside the full-width producer's scope")
            if pending is not None:
                raise NotImplementedError("adaln_operands(full_width=True): pending= has no full-width form (the gated residual is not "
                                          "fused into the full-width producer) - apply ops.gate_residual first")
            return rotation.adaln_rotate_quant_full_mx(x, scale, shift, d=d, smooth=smooth, eps=eps, kmajor=self.kmajor)
        if pending is not None:
            if self.act_table != "e2m1":
                raise RuntimeError(f"{type(self).__name__}.adaln_operands: pending= needs an 'e2m1' activation (the 6-bit group producers "
                                   f"have no fused form), this module's is {self.act_table!r}")
            y, gate = pending
            return rotation.resid_adaln_rotate_quant_mx(y, gate, x, scale, shift, d=d, smooth=smooth, eps=eps, kmajor=self.kmajor)
        if self.act_table == "e2m1":
            return rotation.adaln_rotate_quant_mx(x, scale, shift, d=d, smooth=smooth, eps=eps, kmajor=self.kmajor)
        return rotation.adaln_rotate_quant_g6(x, scale, shift, self.act_table, d=d, smooth=smooth, eps=eps, kmajor=self.kmajor)

    @torch.no_grad()
    def rotate_operands(self, x, d: Optional[torch.Tensor] = None, smooth: Optional[torch.Tensor] = None,
                        full_width: bool = False) -> Tuple[torch.Tensor, torch.Tensor]:
        """`adaln_operands` without the LayerNorm and the modulation: smooth, rotate, per-group quantize of x [..., in_features]
        (`rotation.rotate_quant_mx` / `rotation.rotate_quant_g6`).
        full_width: the full-width rotation of `rotate_model(block_rotate=False)` instead of the 128-block form
        (`rotation.rotate_quant_full_mx`; d: in_features signs) - E2M1 activations only."""
        from . import rotation
        if full_width:
            if self.act_table != "e2m1":
                raise NotImplementedError(f"rotate_operands(full_width=True): the fused full-width rotation emits E2M1 (FP4) operands only, "
                                          f"not {self.act_table!r} - 6-bit operand forms are outside the full-width producer's scope")
            return rotation.rotate_quant_full_mx(x, d=d, smooth=smooth, kmajor=self.kmajor)
        if self.act_table == "e2m1":
            return rotation.rotate_quant_mx(x, d=d, smooth=smooth, kmajor=self.kmajor)
        return rotation.rotate_quant_g6(x, self.act_table, d=d, smooth=smooth, kmajor=self.kmajor)

    @torch.no_grad()
    def forward_operands(self, a_codes: torch.Tensor, a_scales: torch.Tensor, gate=None, residual=None, table: Optional[str] = None) -> torch.Tensor:
        """The same product for an activation that already is in operand form - what the fused producers
        `rotation.rotate_quant_mx` / `rotation.adaln_rotate_quant_mx` emit, or `quantize_g6`: fp16 [tokens, out_features].
        table: the format the codes are in (default: the module's activation format)."""
        return self._run("plain", table, a_codes, a_scales, self.bias, gate, residual)


class FP4LinearGeluDual(FP4Linear):
    """fc1 of an AdaLN block's FFN in the W4A4 per-group configuration with the FFN's GELU(tanh) AND fc2's dual-format input
    quantizer (`fp_e1m2_neg_e2m1_pos`, tr/quant_utils.py:415-452,991) in the GEMM's epilogue: `forward(x)` returns what
    `fc2.act_quant(act(fc1(x)))` returns in the reference's FFN.forward (tr/basic_var.py:120-121) - the module that follows
    must neither apply the activation nor quantize again (`quant_linear.quantize_VAR(..., real_fp4=True, fuse_ffn=True)` swaps
    the FFN's `act` for an identity and switches fc2's input quantizer off).  With an E1M2 / E3M0 activation format
    (`from_float(..., act_fp_type="fp_e1" / "fp_e3")`; row-major, or k-major with `a6w4_kmajor=True`) the same tail runs in the A6W4
    GEMM (`linear_a6w4_gelu_dual` / `linear_a6w4_gelu_dual_km`), and with an E1M2 / E3M0 weight format and `w6_forms=True` in the W6 GEMM
    (`linear_w6_gelu_dual`; `linear_w6_gelu_dual_km` with `kmajor=True, w6_kmajor=True`)."""

    @torch.no_grad()
    def forward(self, x):
        self._no_w6("forward")
        return self._run("gelu_dual", None, *self._quantize(x), self.bias, False).view(*x.shape[:-1], self.out_features)

    @torch.no_grad()
    def forward_operands(self, a_codes: torch.Tensor, a_scales: torch.Tensor, table: Optional[str] = None) -> torch.Tensor:
        """table: the format the codes are in (default: the module's activation format), as in FP4Linear.forward_operands"""
        self._no_w6("forward_operands")
        return self._run("gelu_dual", table, a_codes, a_scales, self.bias, False)


# ---- GF6: full-range FP6 (E2M3 / E3M2) operands with per-group scales - the reference's per-group W6A6, W4A6 and W6A4 ---------
# No GEMM of its own (include/fpq.h, GF6): the A6W4 and W6 kernels decode ANY E2M3 codes under the selector id of E1M2 and any E3M2
# codes under that of E3M0, so a pair with a full FP6 side is a row whose table ids name the hardware decode.  `linear_g6*` accept
# every pair with at least one e2m3 / e3m2 side and route to the A6W4 family when the weight is E2M1 and to the W6 family
# otherwise; quantize_g6, linear_a6w4* and linear_w6* keep refusing the full tables.
_GF6_TABLES = {"e2m3": "e2m3", "fp6_e2m3": "e2m3", "e3m2": "e3m2", "fp6_e3m2": "e3m2", "e2m1": "e2m1", "fp_e2": "e2m1",
               "e1m2": "e1m2", "fp_e1": "e1m2", "e3m0": "e3m0", "fp_e3": "e3m0"}
_GF6_FULL = ("e2m3", "e3m2")
_GF6_DECODE = {"e2m1": "e2m1", "e1m2": "e1m2", "e3m0": "e3m0", "e2m3": "e1m2", "e3m2": "e3m0"}   # the selector id's table
_GF6_CODE_FORMAT = {"e1m2": "e2m3", "e3m0": "e3m2", "e2m3": "e2m3", "e3m2": "e3m2"}             # the 6-bit format the codes are in
# a row per (activation, weight) pair with a 6-bit weight and at least one full FP6 side (fpq_gemm_w6_*; fp32 weight scales only);
# the pairs with an E2M1 weight are the rows "e2m3" / "e3m2" of _FORMATS (fpq_gemm_a6w4_*)
_GF6_W6_FORMATS = {(a, w): _FORMATS[a]._replace(gemm="fpq_gemm_w6", plain="", table=(TABLE_IDS[_GF6_DECODE[a]],), bias_align=8, split_w_f32=True,
                                                w_seg=96, w_table=(TABLE_IDS[_GF6_DECODE[w]],))
                   for a in ("e2m1", "e1m2", "e3m0", "e2m3", "e3m2") for w in ("e1m2", "e3m0", "e2m3", "e3m2")
                   if a in _GF6_FULL or w in _GF6_FULL}
# the fc1 tail's dual pair -> (neg table id, pos table id): fc2's per-group input format - the 6-bit configuration's INT- / E2M3+ (no
# global clamp: a NaN stays in its group; kernels of their own) or the 4-bit E1M2- / E2M1+ of the mixed W4A6 / W6A4 models
_GF6_FC2_PAIRS = {("int_neg", "e2m3_pos"): (TABLE_IDS["int_neg"], TABLE_IDS["e2m3_pos"]),
                  ("e1m2_neg", "e2m1_pos"): (TABLE_IDS["e1m2_neg"], TABLE_IDS["e2m1_pos"])}
# Pairs linear_g6* refuse for their numerics: both operands decoded as BF6 E3M2 with a full-range side.  The matrix core does not keep
# every product of such a dot (profiles/gf6_dot.txt) and over the shape sweep the error reaches 290 - 660 x the GEMM bound, far past
# the 8 x the project grants E3M2 levels on this instruction (profiles/gf6_gemm_bound.txt).  They stay fake-quantized layers.
GF6_REFUSED_PAIRS = frozenset({("e3m0", "e3m2"), ("e3m2", "e3m0"), ("e3m2", "e3m2")})
_GF6_FC2_NAMES = {"fp6_int_neg_e2m3_pos": ("int_neg", "e2m3_pos"), "fp_e1m2_neg_e2m1_pos": ("e1m2_neg", "e2m1_pos")}


def _gf6_table(name: str, table: str, full_only: bool = False) -> str:
    try:
        t = _GF6_TABLES[table]
    except (KeyError, TypeError):
        t = None
    if t is None or (full_only and t not in _GF6_FULL):
        want = "'e2m3' and 'e3m2'" if full_only else "'e2m3', 'e3m2', 'e2m1', 'e1m2' and 'e3m0'"
        raise RuntimeError(f"{name}: the per-group formats here are {want}, got {table!r}")
    return t


def _gf6_owner(a: str, w: str) -> str:
    """the function that owns a pair without a full FP6 side"""
    return "linear_fp4" if (a, w) == ("e2m1", "e2m1") else "linear_a6w4" if w == "e2m1" else "linear_w6"


def _gf6_format(name: str, a_table: str, w_table: str, a: torch.Tensor, w: torch.Tensor, w_scales: torch.Tensor) -> Tuple[_Format, str]:
    """the row of an (activation, weight) pair with at least one full FP6 side, and the layout word of _per_group_operands (the
    operands' rank decides: both 2-D, row-major codes; both 3-D, k-major images)"""
    at, wt = _gf6_table(name, a_table), _gf6_table(name, w_table)
    if at not in _GF6_FULL and wt not in _GF6_FULL:
        raise RuntimeError(f"{name}: the pair ({at}, {wt}) has no e2m3 / e3m2 side - it belongs to {_gf6_owner(at, wt)}")
    if (at, wt) in GF6_REFUSED_PAIRS:
        raise RuntimeError(f"{name}: the pair ({at}, {wt}) is not run on the matrix cores - with both operands decoded as BF6 E3M2 the "
                           "instruction drops small products and the error passes the GEMM contract's allowance "
                           "(profiles/gf6_gemm_bound.txt, profiles/gf6_dot.txt)")
    if (a.dim(), w.dim()) not in ((2, 2), (3, 3)):
        raise RuntimeError(f"{name}: both operands must be row-major codes (2-D) or both k-major images (3-D)")
    if wt == "e2m1":
        return _FORMATS[at], "rank"
    if w_scales.dtype != torch.float32:
        raise RuntimeError(f"{name}: the scales of a 6-bit weight must be float32 (what quantize_gf6 / quantize_g6 write for an fp32 weight)")
    return _GF6_W6_FORMATS[at, wt], "images" if a.dim() == 3 else "rows"


def quantize_gf6(x: torch.Tensor, table: str = "e2m3", kmajor: bool = False) -> Tuple[torch.Tensor, torch.Tensor]:
    """x [..., K] fp16/fp32 (K % 128 == 0) -> (codes uint8 [rows, K * 3 / 4]: dense 6-bit codes of the FULL E2M3 / E3M2 table,
    scales [rows, K/128] in x.dtype), one scale per group of 128 (fpq_gf6_quant_rows_codes): half(level(code) * scale) ==
    fp6_quant_e2m3_per_group_cuda / fp6_quant_e3m2_per_group_cuda (x, 6, 128) bit for bit.
    kmajor: the activation side's k-major images instead - codes [K/128, rows, 96] and scales fp32 [K/128, rows rounded up to 4]."""
    require_gpu(x, "quantize_gf6")
    return _quantize_per_group("quantize_gf6", _FORMATS[_gf6_table("quantize_gf6", table, full_only=True)], x, kmajor)


def dequantize_gf6(codes: torch.Tensor, scales: torch.Tensor, table: str = "e2m3") -> torch.Tensor:
    """Reference decoder in torch ops (tests / debugging): fp32 [rows, K] = level(code) * scale of the code's group, for row-major
    6-bit codes of any per-group table ('e2m3' / 'e3m2', and 'e1m2' / 'e3m0' as quantize_g6 codes them)."""
    table = _gf6_table("dequantize_gf6", table)
    if table == "e2m1":
        raise RuntimeError("dequantize_gf6: E2M1 operands are nibbles - dequantize_mx decodes them")
    rows = codes.shape[0]
    lv = dequantize_fp6(codes, torch.ones(rows, dtype=torch.float32, device=codes.device), _GF6_CODE_FORMAT[table])
    return (lv.view(rows, -1, 128) * scales.float().unsqueeze(-1)).reshape(rows, -1)


def linear_g6(a: torch.Tensor, a_scales: torch.Tensor, a_table: str, w: torch.Tensor, w_scales: torch.Tensor, w_table: str,
              bias: Optional[torch.Tensor] = None, gate: Optional[torch.Tensor] = None, residual: Optional[torch.Tensor] = None,
              outs: Optional[int] = None) -> torch.Tensor:
    """fp16 [tokens, outs] = dequantize(a) @ dequantize(w).T + bias on the matrix cores for a per-group pair with at least one
    full FP6 side ('e2m3' / 'e3m2'; the other side any per-group format): operands as quantize_gf6 / quantize_g6 / quantize_mx emit
    them, row-major (2-D) or k-major images (3-D: the weight `to_kmajor(codes, bits, dealt=True)` with `to_kmajor_scales(scales,
    weight_side=True)`), told by rank.  An E2M1 weight runs on fpq_gemm_a6w4_mx[_km], a 6-bit weight (float32 scales) on
    fpq_gemm_w6_mx[_km].  gate / residual: the AdaLN block's tail as in linear_fp4.  outs: the Linear's width for images whose
    row count is padded, as in linear_fp4.  Numerics per pair: include/fpq.h (GF6) and profiles/gf6_dot.txt."""
    require_gpu(a, "linear_g6")
    fmt, layouts = _gf6_format("linear_g6", a_table, w_table, a, w, w_scales)
    if outs is not None and w.dim() == 2 and outs != w.shape[0]:
        raise RuntimeError(f"linear_g6: outs = {outs}, but the weight has {w.shape[0]} rows")
    return _linear("linear_g6", fmt, layouts, a, a_scales, w, w_scales, bias, gate, residual, outs)


def linear_g6_qkv_to_cache(a: torch.Tensor, a_scales: torch.Tensor, a_table: str, w: torch.Tensor, w_scales: torch.Tensor, w_table: str,
                           bias: Optional[torch.Tensor], cache_kv: torch.Tensor, pos: int, seq: int,
                           qk_norm_scale: Optional[torch.Tensor] = None) -> torch.Tensor:
    """mat_qkv with a split output for the pairs of linear_g6 (fpq_gemm_a6w4_mx_split[_qknorm] for an E2M1 weight,
    fpq_gemm_w6_mx_split[_qknorm][_km] for a 6-bit one): `qkv = linear_g6(...)` for tokens [B * seq] and outs = 3 * C, but only q
    comes back, fp16 [B, seq, C], while k and v are written straight into `cache_kv` [2, B, max_len, H, c] at pos .. pos + seq.
    Operands row-major or k-major by rank; float32 weight scales.  qk_norm_scale and its fp32 bias: as in linear_fp4_qkv_to_cache."""
    require_gpu(a, "linear_g6_qkv_to_cache")
    fmt, layouts = _gf6_format("linear_g6_qkv_to_cache", a_table, w_table, a, w, w_scales)
    return _linear_qkv_to_cache("linear_g6_qkv_to_cache", fmt, a, a_scales, w, w_scales, bias, cache_kv, pos, seq, qk_norm_scale, layouts)


def _gf6_fc2_pair(name: str, fc2_pair) -> Tuple[str, str]:
    pair = _GF6_FC2_NAMES.get(fc2_pair, fc2_pair) if isinstance(fc2_pair, str) else fc2_pair
    try:
        pair = tuple(pair)
    except TypeError:
        pair = None
    if pair not in _GF6_FC2_PAIRS:
        raise RuntimeError(f"{name}: fc2_pair must be ('int_neg', 'e2m3_pos') / 'fp6_int_neg_e2m3_pos' or ('e1m2_neg', 'e2m1_pos') / "
                           f"'fp_e1m2_neg_e2m1_pos', got {fc2_pair!r}")
    return pair


def linear_g6_gelu_dual(a: torch.Tensor, a_scales: torch.Tensor, a_table: str, w: torch.Tensor, w_scales: torch.Tensor, w_table: str,
                        bias: Optional[torch.Tensor] = None, fc2_pair=("int_neg", "e2m3_pos"), return_gelu: bool = False,
                        outs: Optional[int] = None):
    """fc1 of the FFN up to fc2's GEMM in one launch for the pairs of linear_g6 (fpq_gemm_a6w4_gelu_dual_pair for an E2M1 weight,
    fpq_gemm_w6_gelu_dual_pair for a 6-bit one): fp16 [tokens, outs] = fc2's per-group(128) dual input quantizer applied to
    F.gelu(linear_g6(...), approximate="tanh"), outs % 128 == 0.  fc2_pair ('int_neg', 'e2m3_pos') - the per-group 6-bit
    configuration's `fp6_quant_int_neg_e2m3_pos_per_group_cuda(h, 6, 128)`, which has no global clamp: a NaN stays in its group - or
    ('e1m2_neg', 'e2m1_pos'): `fp_quant_e1m2_neg_e2m1_pos_per_group_cuda(h, 4, 128)` as linear_a6w4_gelu_dual / linear_w6_gelu_dual
    compute it (+ the NaN fix-up launch).  Operands row-major or k-major by rank; return_gelu: also the GELU values the quantizer saw."""
    require_gpu(a, "linear_g6_gelu_dual")
    fmt, layouts = _gf6_format("linear_g6_gelu_dual", a_table, w_table, a, w, w_scales)
    pair = _GF6_FC2_PAIRS[_gf6_fc2_pair("linear_g6_gelu_dual", fc2_pair)]
    return _linear_gelu_dual("linear_g6_gelu_dual", fmt, layouts, a, a_scales, w, w_scales, bias, return_gelu, outs, pair)


def _quantize_any(name: str, table: str, x: torch.Tensor, kmajor: bool = False) -> Tuple[torch.Tensor, torch.Tensor]:
    """x -> (codes, scales) in the per-group format `table` (a canonical name), by the quantizer that owns it"""
    return _quantize_per_group(_FORMATS[table].quantizer, _FORMATS[table], x, kmajor)


class FP6GroupLinear(FP4Linear):
    """FP4Linear for the per-group pairs with a full FP6 side (the reference's per-group W6A6, W4A6, W6A4): the weight is held as
    the codes and fp32 group scales of its format's quantizer (quantize_gf6 for 'e2m3' / 'e3m2', quantize_g6 for 'e1m2' / 'e3m0',
    quantize_mx for 'e2m1'), row-major or as dealt k-major images; the activation is quantized on the fly in its own format and
    the product is linear_g6.  Same buffers (w_codes, w_scales, bias) as its parent."""

    def __init__(self, w_codes, w_scales, bias, in_features, out_features, act_table: str = "e2m3", w_table: str = "e2m3"):
        super().__init__(w_codes, w_scales, bias, in_features, out_features, act_table, w_table, w6_forms=True)

    @classmethod
    def from_float(cls, module: torch.nn.Linear, weight_fp_type: str = "fp6_e2m3", act_fp_type: str = "fp6_e2m3", kmajor: bool = False):
        """weight_fp_type / act_fp_type: the reference's names - "fp6_e2m3", "fp6_e3m2", "fp_e1", "fp_e2", "fp_e3" - at least one of
        them an fp6 one.  kmajor: hold the weight as the dealt k-major image and its fp32 scale image; activations become images too."""
        name = f"{cls.__name__}.from_float"
        assert isinstance(module, torch.nn.Linear) and module.in_features % 128 == 0 and module.out_features % 8 == 0
        try:
            at, wt = _gf6_table(name, act_fp_type), _gf6_table(name, weight_fp_type)
        except RuntimeError as e:
            raise ValueError(str(e)) from None
        if at not in _GF6_FULL and wt not in _GF6_FULL:
            raise ValueError(f"{name}: the pair ({at}, {wt}) has no fp6_e2m3 / fp6_e3m2 side - it belongs to FP4Linear")
        codes, scales, bias = _weight_operands(name, module, wt, kmajor)
        return cls(codes, scales, bias, module.in_features, module.out_features, at, wt)

    def _run(self, form: str, table: Optional[str], a_codes, a_scales, *rest):
        table = self.act_table if table is None else _gf6_table(f"{type(self).__name__}.forward_operands", table)
        if form == "plain":
            return linear_g6(a_codes, a_scales, table, self.w_codes, self.w_scales, self.w_table, *rest, self.out_features)
        if form == "qkv_to_cache":
            return linear_g6_qkv_to_cache(a_codes, a_scales, table, self.w_codes, self.w_scales, self.w_table, *rest)
        raise ValueError(f"{type(self).__name__}: no {form} form")

    def _no_w6(self, form: str) -> None:   # every form exists for every pair here
        return None

    @torch.no_grad()
    def adaln_operands(self, x, scale, shift, d: Optional[torch.Tensor] = None, smooth: Optional[torch.Tensor] = None,
                       eps: float = 1e-6, pending: Optional[Tuple[torch.Tensor, torch.Tensor]] = None, full_width: bool = False):
        """FP4Linear.adaln_operands; an 'e2m3' / 'e3m2' activation comes from `rotation.adaln_rotate_quant_gf6` (byte for byte
        quantize_gf6 of the rotated rows), any other format from the parent's producer; k-major iff the weight is an image.
        full_width goes to the parent, which owns the one format that has a full-width producer ('e2m1') and refuses the others."""
        if pending is not None or full_width:   # (the parent refuses every activation format but 'e2m1')
            return super().adaln_operands(x, scale, shift, d=d, smooth=smooth, eps=eps, pending=pending, full_width=full_width)
        if self.act_table not in _GF6_FULL:
            return super().adaln_operands(x, scale, shift, d=d, smooth=smooth, eps=eps)
        from . import rotation
        return rotation.adaln_rotate_quant_gf6(x, scale, shift, self.act_table, d=d, smooth=smooth, eps=eps, kmajor=self.kmajor)

    @torch.no_grad()
    def rotate_operands(self, x, d: Optional[torch.Tensor] = None, smooth: Optional[torch.Tensor] = None) -> Tuple[torch.Tensor, torch.Tensor]:
        """FP4Linear.rotate_operands; an 'e2m3' / 'e3m2' activation comes from `rotation.rotate_quant_gf6`."""
        if self.act_table not in _GF6_FULL:
            return super().rotate_operands(x, d=d, smooth=smooth)
        from . import rotation
        return rotation.rotate_quant_gf6(x, self.act_table, d=d, smooth=smooth, kmajor=self.kmajor)


class FP6GroupLinearGeluDual(FP6GroupLinear):
    """FP4LinearGeluDual for the pairs of FP6GroupLinear: fc1 with the FFN's GELU(tanh) and fc2's per-group dual input quantizer in
    the GEMM's epilogue (linear_g6_gelu_dual) - `forward(x)` returns what `fc2.act_quant(act(fc1(x)))` returns; the module that
    follows must neither apply the activation nor quantize again.  fc2_pair: ('int_neg', 'e2m3_pos') or ('e1m2_neg', 'e2m1_pos')."""

    def __init__(self, w_codes, w_scales, bias, in_features, out_features, act_table: str = "e2m3", w_table: str = "e2m3",
                 fc2_pair=("int_neg", "e2m3_pos")):
        super().__init__(w_codes, w_scales, bias, in_features, out_features, act_table, w_table)
        self.fc2_pair = _gf6_fc2_pair("FP6GroupLinearGeluDual", fc2_pair)

    @classmethod
    def from_float(cls, module: torch.nn.Linear, weight_fp_type: str = "fp6_e2m3", act_fp_type: str = "fp6_e2m3", kmajor: bool = False,
                   fc2_fp_type="fp6_int_neg_e2m3_pos"):
        """fc2_fp_type: "fp6_int_neg_e2m3_pos" or "fp_e1m2_neg_e2m1_pos" (or the pair of table names); the rest as FP6GroupLinear"""
        assert module.out_features % 128 == 0
        try:
            pair = _gf6_fc2_pair("FP6GroupLinearGeluDual.from_float", fc2_fp_type)
        except RuntimeError as e:
            raise ValueError(str(e)) from None
        m = super().from_float(module, weight_fp_type, act_fp_type, kmajor)
        m.fc2_pair = pair
        return m

    def _run(self, form: str, table: Optional[str], a_codes, a_scales, *rest):
        if form != "gelu_dual":
            return super()._run(form, table, a_codes, a_scales, *rest)
        table = self.act_table if table is None else _gf6_table(f"{type(self).__name__}.forward_operands", table)
        bias, return_gelu = rest
        return linear_g6_gelu_dual(a_codes, a_scales, table, self.w_codes, self.w_scales, self.w_table, bias, self.fc2_pair, return_gelu,
                                   self.out_features)

    @torch.no_grad()
    def forward(self, x):
        return self._run("gelu_dual", None, *self._quantize(x), self.bias, False).view(*x.shape[:-1], self.out_features)

    @torch.no_grad()
    def forward_operands(self, a_codes: torch.Tensor, a_scales: torch.Tensor, table: Optional[str] = None) -> torch.Tensor:
        return self._run("gelu_dual", table, a_codes, a_scales, self.bias, False)


# ---- per-token activations x per-channel weights (W6A6): one scale per row, FP8-coded levels ---------------------
_FP8_TABLES = {"fp6_e2m3": "e2m3", "fp6_e3m2": "e3m2", "fp_e2": "e2m1", "fp_e1": "e1m2", "fp_e3": "e3m0",
               "e2m3": "e2m3", "e3m2": "e3m2", "e2m1": "e2m1", "e1m2": "e1m2", "e3m0": "e3m0"}


def quantize_fp8(x: torch.Tensor, table: str = "e2m3") -> Tuple[torch.Tensor, torch.Tensor]:
    """x [..., K] fp16/fp32 -> (codes uint8 [rows, K]: the level of every element as an OCP E4M3 byte,
    scales [rows] in x.dtype); one scale per row of K elements, e4m3(code) * scale == the fake-quantized value."""
    require_gpu(x, "quantize_fp8")
    if x.dtype not in (torch.float16, torch.float32):
        raise RuntimeError(f"quantize_fp8: x must be float16 or float32, got {x.dtype}")
    k = x.shape[-1]
    xc = x.contiguous()
    rows = xc.numel() // k
    codes = torch.empty((rows, k), dtype=torch.uint8, device=x.device)
    scales = torch.empty((rows,), dtype=x.dtype, device=x.device)
    with device_guard(x.device):
        check(lib().fpq_quant_rows_codes_fp8(xc.data_ptr(), codes.data_ptr(), scales.data_ptr(), rows, k,
                                             TABLE_IDS[_FP8_TABLES[table]], dtype_id(x.dtype), stream_ptr(x.device)),
              "fpq_quant_rows_codes_fp8")
    return codes, scales


def dequantize_fp8(codes: torch.Tensor, scales: torch.Tensor) -> torch.Tensor:
    """Reference decoder in torch ops (tests / debugging): fp32 [rows, K]."""
    return codes.view(torch.float8_e4m3fn).float() * scales.float().unsqueeze(-1)


def linear_fp8(a_codes: torch.Tensor, a_scales: torch.Tensor, w_codes: torch.Tensor, w_scales: torch.Tensor,
               bias: Optional[torch.Tensor] = None, gate: Optional[torch.Tensor] = None,
               residual: Optional[torch.Tensor] = None) -> torch.Tensor:
    """fp16 [tokens, outs] = dequant(a) @ dequant(w).T + bias on the FP8 matrix cores (row-scaled operands); optional
    fused `residual + y.mul(gate)` as in linear_fp4."""
    require_gpu(a_codes, "linear_fp8")
    if a_codes.dim() != 2 or w_codes.dim() != 2:
        raise RuntimeError("linear_fp8: codes must be [rows, K]")
    tokens, outs, k = a_codes.shape[0], w_codes.shape[0], a_codes.shape[1]
    if w_codes.shape[1] != k:
        raise RuntimeError("linear_fp8: operand shapes mismatch")
    _check_operand("linear_fp8(activation)", a_codes, a_scales, tokens, k, tokens, a_codes.device)
    _check_operand("linear_fp8(weight)", w_codes, w_scales, outs, k, outs, a_codes.device)
    ep, keep, out = _epilogue("linear_fp8", tokens, outs, gate, residual, None, a_codes.device)
    b = _bias_f16("linear_fp8", bias, None, a_codes.device)
    with device_guard(a_codes.device):
        check(lib().fpq_gemm_fp8_rows_ex(a_codes.data_ptr(), a_scales.data_ptr(), dtype_id(a_scales.dtype), w_codes.data_ptr(),
                                         w_scales.data_ptr(), dtype_id(w_scales.dtype), None if b is None else b.data_ptr(),
                                         out.data_ptr(), tokens, outs, k, ep, stream_ptr(a_codes.device)), "fpq_gemm_fp8_rows_ex")
    del keep
    return out


class FP8Linear(_ScaledOperandModule):
    """Drop-in for QuantizedLinear in the per_channel / per_token configurations (W6A6 `fp6_e2m3` / `fp6_e3m2`,
    run.sh:7) on the FP8 matrix cores: same quantization decisions as the reference (e4m3(code) * scale == its
    fake-quantized tensors), weights stored as one byte per element + one fp32 scale per output channel."""

    def __init__(self, w_codes, w_scales, bias, in_features, out_features, act_table):
        super().__init__()
        self.in_features, self.out_features, self.act_table = in_features, out_features, act_table
        self.register_buffer("w_codes", w_codes)
        self.register_buffer("w_scales", w_scales)
        self.register_buffer("bias", bias)

    @classmethod
    def from_float(cls, module: torch.nn.Linear, weight_fp_type: str = "fp6_e2m3", act_fp_type: str = "fp6_e2m3"):
        assert isinstance(module, torch.nn.Linear) and module.in_features % 128 == 0 and module.out_features % 8 == 0
        if getattr(module, "packed_weight", None) is not None:
            raise ValueError("FP8Linear.from_float: a packed weight has no E4M3-coded form - quantize_VAR(..., real_fp6=True, "
                             "packed_e3m2=True) builds this layer as a gemm.FP6Linear, which takes it")
        codes, scales = quantize_fp8(module.weight.detach().float(), weight_fp_type)
        bias = None if module.bias is None else module.bias.detach().to(torch.float16)
        return cls(codes, scales, bias, module.in_features, module.out_features, act_fp_type)

    @torch.no_grad()
    def forward(self, x, gate=None, residual=None):
        lead = x.shape[:-1]
        a_codes, a_scales = quantize_fp8(x.to(torch.float16).reshape(-1, self.in_features), self.act_table)
        return linear_fp8(a_codes, a_scales, self.w_codes, self.w_scales, self.bias, gate, residual).view(*lead, self.out_features)


# ---- the same with 6-bit packed operands: FP6 E2M3 (the W6A6 run configuration) or BF6 E3M2, chosen per operand ------------
_F6_TABLES = {"e2m3": "e2m3", "fp6_e2m3": "e2m3", "e3m2": "e3m2", "fp6_e3m2": "e3m2"}


def _f6_table(name: str, table: str) -> str:
    """'e2m3' / 'fp6_e2m3' -> 'e2m3', 'e3m2' / 'fp6_e3m2' -> 'e3m2': the two formats of the dense 6-bit operand form"""
    try:
        return _F6_TABLES[table]
    except (KeyError, TypeError):
        raise RuntimeError(f"{name}: the 6-bit operand formats are 'e2m3' and 'e3m2', got {table!r}") from None


def quantize_fp6(x: torch.Tensor, kmajor: bool = False, table: str = "e2m3") -> Tuple[torch.Tensor, torch.Tensor]:
    """x [..., K] fp16/fp32 (K % 32 == 0) -> (codes uint8 [rows, K * 3 / 4]: dense 6-bit E2M3 codes,
    scales [rows] in x.dtype); e2m3(code) * scale == fp6_quant_e2m3_per_token_cuda(x).
    kmajor (K % 128 == 0): the codes as the activation side's k-major image [K/128, rows, 96].
    table="e3m2": BF6 codes (sign, 3 exponent bits, 2 mantissa bits) in the same packing - fp6_quant_e3m2_per_token_cuda's
    decisions (fpq_quant_rows_codes_f6)."""
    require_gpu(x, "quantize_fp6")
    if x.dtype not in (torch.float16, torch.float32):
        raise RuntimeError(f"quantize_fp6: x must be float16 or float32, got {x.dtype}")
    table = _f6_table("quantize_fp6", table)
    k = x.shape[-1]
    if k % 32 != 0:
        raise RuntimeError("quantize_fp6: the last dimension must be a multiple of 32")
    xc = x.contiguous()
    rows = xc.numel() // k
    if kmajor and k % 128 != 0:
        raise RuntimeError("quantize_fp6(kmajor=True): the last dimension must be a multiple of 128")
    codes = torch.empty((k // 128, rows, 96) if kmajor else (rows, k * 3 // 4), dtype=torch.uint8, device=x.device)
    scales = torch.empty((rows,), dtype=x.dtype, device=x.device)
    if table != "e2m3":
        with device_guard(x.device):
            check(lib().fpq_quant_rows_codes_f6(xc.data_ptr(), codes.data_ptr(), scales.data_ptr(), rows, k, TABLE_IDS[table],
                                                dtype_id(x.dtype), 1 if kmajor else 0, stream_ptr(x.device)), "fpq_quant_rows_codes_f6")
        return codes, scales
    fn = lib().fpq_quant_rows_codes_fp6_km if kmajor else lib().fpq_quant_rows_codes_fp6
    with device_guard(x.device):
        check(fn(xc.data_ptr(), codes.data_ptr(), scales.data_ptr(), rows, k, TABLE_IDS["e2m3"], dtype_id(x.dtype),
                 stream_ptr(x.device)), "fpq_quant_rows_codes_fp6_km" if kmajor else "fpq_quant_rows_codes_fp6")
    return codes, scales


def dequantize_fp6(codes: torch.Tensor, scales: torch.Tensor, table: str = "e2m3") -> torch.Tensor:
    """Reference decoder in torch ops (tests / debugging): fp32 [rows, K].  table: the format the codes are in."""
    table = _f6_table("dequantize_fp6", table)
    b = codes.reshape(codes.shape[0], -1, 3).to(torch.int32)
    word = b[..., 0] | (b[..., 1] << 8) | (b[..., 2] << 16)
    c = torch.stack((word & 63, (word >> 6) & 63, (word >> 12) & 63, (word >> 18) & 63), dim=-1).reshape(codes.shape[0], -1)
    if table == "e3m2":   # sign, 3 exponent bits (bias 3), 2 mantissa bits
        e, m = (c >> 2) & 7, (c & 3).float()
        mag = torch.where(e == 0, m / 16.0, (1.0 + m / 4.0) * torch.pow(2.0, (e - 3).float()))
    else:                 # sign, 2 exponent bits (bias 1), 3 mantissa bits
        e, m = (c >> 3) & 3, (c & 7).float()
        mag = torch.where(e == 0, m / 8.0, (1.0 + m / 8.0) * torch.pow(2.0, (e - 1).float()))
    val = torch.where((c & 32) != 0, -mag, mag)
    return val * scales.float().unsqueeze(-1)


def _fp6_operands(name: str, a_codes, a_scales, w_codes, w_scales):
    """A row-scaled 6-bit operand pair, row-major codes (2-D) or k-major images (3-D), checked -> (km, tokens, outs, k)"""
    km = _kmajor_pair(name, a_codes, w_codes, 96)
    if km:
        tokens, outs, k = a_codes.shape[1], w_scales.shape[0], a_codes.shape[0] * 128
        w_rows, row_bytes = (outs + 63) // 64 * 64, a_codes.shape[0] * 96
    else:
        tokens, outs, k = a_codes.shape[0], w_codes.shape[0], a_codes.shape[1] * 4 // 3
        w_rows, row_bytes = outs, a_codes.shape[1]
        if w_codes.shape[1] != a_codes.shape[1]:
            raise RuntimeError(f"{name}: operand shapes mismatch")
    _check_operand(f"{name}(activation)", a_codes, a_scales, tokens, row_bytes, tokens, a_codes.device)
    _check_operand(f"{name}(weight)", w_codes, w_scales, w_rows, row_bytes, outs, a_codes.device)
    return km, tokens, outs, k


def _fp6_gemm(form: str, a_codes, a_scales, a_table: str, w_codes, w_scales, w_table: str, km: bool, *rest) -> None:
    """One call of the FP6 GEMM's C entry point of `form` ("", "_split" or "_split_qknorm"); rest: its arguments between the
    weight scales' dtype and the k-major flag.  (E2M3, E2M3) goes to fpq_gemm_fp6_rows_*, any other pair to fpq_gemm_f6_rows*
    with the two table ids."""
    a = (a_codes.data_ptr(), a_scales.data_ptr(), dtype_id(a_scales.dtype))
    w = (w_codes.data_ptr(), w_scales.data_ptr(), dtype_id(w_scales.dtype))
    if (a_table, w_table) != ("e2m3", "e2m3"):
            what, args = "fpq_gemm_f6_rows" + form, (*a, TABLE_IDS[a_table], *w, TABLE_IDS[w_table], *rest, 1 if km else 0)
    elif form:
        what, args = "fpq_gemm_fp6_rows" + form, (*a, *w, *rest, 1 if km else 0)
    else:   # the plain E2M3 x E2M3 form has an entry point per layout instead of the flag
        what, args = "fpq_gemm_fp6_rows_km" if km else "fpq_gemm_fp6_rows_ex", (*a, *w, *rest)
    with device_guard(a_codes.device):
        check(getattr(lib(), what)(*args, stream_ptr(a_codes.device)), what)


def linear_fp6(a_codes: torch.Tensor, a_scales: torch.Tensor, w_codes: torch.Tensor, w_scales: torch.Tensor,
               bias: Optional[torch.Tensor] = None, gate: Optional[torch.Tensor] = None,
               residual: Optional[torch.Tensor] = None, a_table: str = "e2m3", w_table: str = "e2m3") -> torch.Tensor:
    """fp16 [tokens, outs] = dequant(a) @ dequant(w).T + bias on the FP6 matrix cores (row-scaled operands); optional
    fused `residual + y.mul(gate)` as in linear_fp4.  a_table / w_table: the format of the activation / weight codes,
    "e2m3" (FP6) or "e3m2" (BF6) - the matrix instruction decodes each operand by its own selector (fpq_gemm_f6_rows)."""
    require_gpu(a_codes, "linear_fp6")
    a_table, w_table = _f6_table("linear_fp6", a_table), _f6_table("linear_fp6", w_table)
    if a_codes.dim() == 2 and w_codes.dim() == 2 and a_codes.shape[1] % 3 != 0:
        raise RuntimeError("linear_fp6: operand shapes mismatch")
    km, tokens, outs, k = _fp6_operands("linear_fp6", a_codes, a_scales, w_codes, w_scales)
    ep, keep, out = _epilogue("linear_fp6", tokens, outs, gate, residual, None, a_codes.device)
    b = _bias_f16("linear_fp6", bias, None, a_codes.device)
    _fp6_gemm("", a_codes, a_scales, a_table, w_codes, w_scales, w_table, km, None if b is None else b.data_ptr(), out.data_ptr(),
              tokens, outs, k, ep)
    del keep
    return out


def linear_fp6_sqerr(a_codes: torch.Tensor, a_scales: torch.Tensor, w_codes: torch.Tensor, w_scales: torch.Tensor, ref: torch.Tensor,
                     row_weight: torch.Tensor, out: Optional[torch.Tensor] = None, bias: Optional[torch.Tensor] = None,
                     a_table: str = "e2m3", w_table: str = "e2m3", workspace: Optional[torch.Tensor] = None) -> torch.Tensor:
    """linear_fp4_sqerr for the row-scaled 6-bit operands of linear_fp6 (fpq_gemm_f6_rows_sqerr): the loss of y = linear_fp6(a, w,
    bias, a_table=, w_table=) against ref, y never written.  Row-major operands only."""
    name = "linear_fp6_sqerr"
    require_gpu(a_codes, name)
    a_table, w_table = _f6_table(name, a_table), _f6_table(name, w_table)
    if a_codes.dim() != 2 or w_codes.dim() != 2:
        raise RuntimeError(f"{name}: row-major operands only")
    if a_codes.shape[1] % 3 != 0:
        raise RuntimeError(f"{name}: operand shapes mismatch")
    _, tokens, outs, k = _fp6_operands(name, a_codes, a_scales, w_codes, w_scales)
    b = _bias_f16(name, bias, None, a_codes.device)
    pr, rdt, pw, out, ws = _sqerr_args(name, tokens, outs, a_codes.device, ref, row_weight, out, workspace)
    args = (a_codes.data_ptr(), a_scales.data_ptr(), dtype_id(a_scales.dtype), TABLE_IDS[a_table], w_codes.data_ptr(), w_scales.data_ptr(),
            dtype_id(w_scales.dtype), TABLE_IDS[w_table], None if b is None else b.data_ptr(), pr, rdt, pw, out.data_ptr(), ws.data_ptr(),
            tokens, outs, k)
    with device_guard(a_codes.device):
        check(lib().fpq_gemm_f6_rows_sqerr(*args, stream_ptr(a_codes.device)), "fpq_gemm_f6_rows_sqerr")
    return out


def linear_fp6_qkv_to_cache(a_codes: torch.Tensor, a_scales: torch.Tensor, w_codes: torch.Tensor, w_scales: torch.Tensor,
                            bias: Optional[torch.Tensor], cache_kv: torch.Tensor, pos: int, seq: int,
                            qk_norm_scale: Optional[torch.Tensor] = None, a_table: str = "e2m3", w_table: str = "e2m3") -> torch.Tensor:
    """linear_fp4_qkv_to_cache for the row-scaled FP6 operands of linear_fp6 (fpq_gemm_fp6_rows_split): q comes back - fp16
    [B, seq, C] - and k, v are written straight into `cache_kv` [2, B, max_len, H, c] at token positions pos .. pos + seq, each value
    bit for bit the one linear_fp6(a, w, bias) holds there.  Operands row-major (2-D) or k-major images (3-D), scales float16 or
    float32 as in linear_fp6.  qk_norm_scale (fp32 [H]) and the fp32 bias [3C] it goes with: the q / k norm in the epilogue
    (fpq_gemm_fp6_rows_split_qknorm), exactly as linear_fp4_qkv_to_cache states it.  a_table / w_table: the operands' formats as in
    linear_fp6 (fpq_gemm_f6_rows_split / _split_qknorm)."""
    name = "linear_fp6_qkv_to_cache"
    require_gpu(a_codes, name)
    a_table, w_table = _f6_table(name, a_table), _f6_table(name, w_table)
    _check_cache_kv(name, cache_kv, a_codes.device)
    if a_codes.dim() == 2 and w_codes.dim() == 2 and a_codes.shape[1] % 96 != 0:
        raise RuntimeError(f"{name}: operand shapes mismatch")
    km, tokens, outs, k = _fp6_operands(name, a_codes, a_scales, w_codes, w_scales)
    q, sp, b, hs = _qkv_split_args(name, cache_kv, tokens, outs, bias, pos, seq, qk_norm_scale)
    if tokens:
        norm = () if hs is None else (hs.data_ptr(),)
        _fp6_gemm("_split" if hs is None else "_split_qknorm", a_codes, a_scales, a_table, w_codes, w_scales, w_table, km,
                  None if b is None else b.data_ptr(), tokens, outs, k, ctypes.byref(sp), *norm)
    return q


class FP6Linear(_ScaledOperandModule):
    """FP8Linear with 6-bit packed operands: 0.75 byte per weight.  E2M3 activations x E2M3 weights (run.sh:7) by default; `act_table`
    / `w_table` ("e2m3" or "e3m2") name the format of each side - the matrix instruction decodes them separately, so the
    mixed pairs of the reference's FP6 format search (quantize_VAR_mixed_fp6_datatype) run on the same kernel."""

    def __init__(self, w_codes, w_scales, bias, in_features, out_features, act_table: str = "e2m3", w_table: str = "e2m3"):
        super().__init__()
        self.in_features, self.out_features = in_features, out_features
        self.act_table, self.w_table = _f6_table("FP6Linear", act_table), _f6_table("FP6Linear", w_table)
        self.register_buffer("w_codes", w_codes)
        self.register_buffer("w_scales", w_scales)
        self.register_buffer("bias", bias)

    @property
    def kmajor(self) -> bool:
        return self.w_codes.dim() == 3

    @classmethod
    def from_float(cls, module: torch.nn.Linear, kmajor: bool = False, weight_fp_type: str = "fp6_e2m3", act_fp_type: str = "fp6_e2m3"):
        assert isinstance(module, torch.nn.Linear) and module.in_features % 128 == 0 and module.out_features % 8 == 0
        w_table, act_table = _f6_table("FP6Linear.from_float", weight_fp_type), _f6_table("FP6Linear.from_float", act_fp_type)
        codes, scales, bias = _weight_operands(f"{cls.__name__}.from_float", module, w_table, kmajor, per_channel=True)
        return cls(codes, scales, bias, module.in_features, module.out_features, act_table, w_table)

    def extra_repr(self) -> str:
        return f"{self.in_features}, {self.out_features}, act={self.act_table}, weight={self.w_table}, kmajor={self.kmajor}"

    @torch.no_grad()
    def forward(self, x, gate=None, residual=None):
        lead = x.shape[:-1]
        a_codes, a_scales = quantize_fp6(x.to(torch.float16).reshape(-1, self.in_features), kmajor=self.kmajor, table=self.act_table)
        return linear_fp6(a_codes, a_scales, self.w_codes, self.w_scales, self.bias, gate, residual, self.act_table,
                          self.w_table).view(*lead, self.out_features)

    @torch.no_grad()
    def forward_operands(self, a_codes: torch.Tensor, a_scales: torch.Tensor, gate=None, residual=None) -> torch.Tensor:
        """The same product for an activation that already is in operand form (codes of `act_table`, row-major or the k-major image
        as the weight is held) - what `rotation.adaln_rotate_quant_token(..., emit="fp6" / "bf6")` emits: fp16 [tokens, out_features]."""
        return linear_fp6(a_codes, a_scales, self.w_codes, self.w_scales, self.bias, gate, residual, self.act_table, self.w_table)
