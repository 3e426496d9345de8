"""Randomized-Hadamard rotation pieces (reference: rotate_utils/hadamard_utils.py:63-99,
rotate_utils/rotation_utils.py:69-104) and the fused online rotate + quant op.

The reference builds a dense block-diagonal Q (15 or 18 identical 128x128 blocks
``diag(D) . H128 / sqrt(128)``, D = +-1 drawn with ``torch.manual_seed(42)``) and
multiplies activations by it with a dense fp16 GEMM on every forward
(tr/basic_var.py:263,266).  Here Q exists only for the offline weight side and for
tests; online, ``rotate_quant`` runs the 128-point transform on the matrix cores inside the quant kernel.
"""
from __future__ import annotations

import ctypes
from typing import Callable, NamedTuple, Optional, Tuple, Union

import torch

from ._lib import TABLE_IDS, check, dtype_id, lib, require_gpu, stream_ptr, device_guard
from .gemm import _g6_table, _gf6_table, kmajor_mx_scales


def sign_vector(size: int = 128, seed: int = 42) -> torch.Tensor:
    """D of random_hadamard_matrix(size, device, seed): ``torch.manual_seed(seed);
    randint(0, 2, (size,)) * 2 - 1`` on the CPU generator (hadamard_utils.py:92-99),
    drawn from a private generator so the global RNG state is left alone."""
    g = torch.Generator(device="cpu")
    g.manual_seed(seed)
    return torch.randint(low=0, high=2, size=(size,), generator=g).to(torch.float64) * 2 - 1


def sylvester(n: int) -> torch.Tensor:
    assert n & (n - 1) == 0, "Sylvester's construction gives power-of-two sizes only"
    h = torch.ones(1, 1, dtype=torch.float64)
    while h.shape[0] < n:
        h = torch.cat([torch.cat([h, h], 1), torch.cat([h, -h], 1)], 0)
    return h


# ---- Hadamard matrices of the non-power-of-two orders the full-width rotation needs ---------------------------
# The reference keeps literal 12 .. 172-row tables (rotate_utils/hadamard_utils.py:164-4204, taken from Sloane's
# library via quip-sharp).  Eight of them ARE Paley's constructions entry for entry (checked against the reference's
# tables; fixtures in tests/golden): orders 12, 20, 60, 108, 140 = Paley I over GF(11), GF(19), GF(59), GF(107),
# GF(139); orders 36 and 28 = Paley II over GF(17) and GF(13); order 40 = [[H20, H20], [H20, -H20]].  They are
# generated here from the quadratic-residue character instead of being stored.  VAR's widths need exactly these:
# 1280 = 40 * 32 (d20), 1536 = 12 * 128 (d24), 1920 = 60 * 32 (d30), 2304 = 36 * 64 (d36).  Orders 172, 156 and 52
# (other constructions) are not provided.
def _chi(q: int):
    """Quadratic-residue character of GF(q), q an odd prime: chi[x] = +1 (non-zero square), -1 (non-square), 0."""
    squares = {(x * x) % q for x in range(1, q)}
    return [0] + [1 if x in squares else -1 for x in range(1, q)]


def paley_hadamard_i(q: int) -> torch.Tensor:
    """Order q + 1, q = 3 (mod 4) prime, normalised as the reference's tables are: first column +1, first row
    (+1, -1, ..., -1), the q x q core is the right-circulant I - S with S[i][j] = chi(j - i)."""
    assert q % 4 == 3
    chi = torch.tensor(_chi(q), dtype=torch.float64)
    idx = (torch.arange(q)[None, :] - torch.arange(q)[:, None]) % q
    h = torch.ones(q + 1, q + 1, dtype=torch.float64)
    h[0, 1:] = -1.0
    h[1:, 1:] = torch.eye(q, dtype=torch.float64) - chi[idx]
    return h


def paley_hadamard_ii(q: int) -> torch.Tensor:
    """Order 2 (q + 1), q = 1 (mod 4) prime: with C the symmetric conference matrix [[0, 1], [1, chi(j - i)]],
    H = [[C + I, C - I], [C - I, -C - I]] (the block layout of the reference's tables)."""
    assert q % 4 == 1
    chi = torch.tensor(_chi(q), dtype=torch.float64)
    idx = (torch.arange(q)[None, :] - torch.arange(q)[:, None]) % q
    c = torch.ones(q + 1, q + 1, dtype=torch.float64)
    c[0, 0] = 0.0
    c[1:, 1:] = chi[idx]
    eye = torch.eye(q + 1, dtype=torch.float64)
    return torch.cat([torch.cat([c + eye, c - eye], 1), torch.cat([c - eye, -c - eye], 1)], 0)


def williamson_hadamard(n: int, minus) -> torch.Tensor:
    """Williamson's array  [[A, B, C, D], [-B, A, -D, C], [-C, D, A, -B], [-D, -C, B, A]]  of four symmetric circulant
    +-1 matrices of order n (row i of a block = its first row rotated right by i); `minus[t]` is the bit mask of the -1
    entries of block t's first row.  AA' + BB' + CC' + DD' = 4n I makes it a Hadamard matrix of order 4n.  The reference's
    literal had52 / had156 / had172 (hadamard_utils.py:666, 2057, 2998 - Sloane's had.52.will, had.156.will,
    had.172.will) are exactly this array for n = 13, 39, 43 with the first rows below."""
    idx = (torch.arange(n).view(1, n) - torch.arange(n).view(n, 1)) % n          # [i, j] -> (j - i) mod n
    blocks = []
    for m in minus:
        row = torch.tensor([-1.0 if (m >> i) & 1 else 1.0 for i in range(n)], dtype=torch.float64)
        assert torch.equal(row[1:], row[1:].flip(0)), "a Williamson block is symmetric"
        blocks.append(row[idx])
    a, b, c, d = blocks
    return torch.cat([torch.cat([a, b, c, d], 1), torch.cat([-b, a, -d, c], 1),
                      torch.cat([-c, d, a, -b], 1), torch.cat([-d, -c, b, a], 1)], 0)


_WILLIAMSON = {52: (13, (0x161a, 0x1c0e, 0xb34, 0x1ede)),
               156: (39, (0x1afb3cdf58, 0xecf5af370, 0x1975bdae98, 0x72be247d4e)),
               172: (43, (0x730a26450ce, 0x207ac935e04, 0x14d42f42b28, 0x385b3fcda1c))}

_PALEY = {172: lambda: williamson_hadamard(*_WILLIAMSON[172]), 156: lambda: williamson_hadamard(*_WILLIAMSON[156]),
          52: lambda: williamson_hadamard(*_WILLIAMSON[52]),
          140: lambda: paley_hadamard_i(139), 108: lambda: paley_hadamard_i(107), 60: lambda: paley_hadamard_i(59),
          36: lambda: paley_hadamard_ii(17), 28: lambda: paley_hadamard_ii(13),
          40: lambda: torch.kron(sylvester(2), paley_hadamard_i(19)),          # the reference's had40 is the doubled had20
          20: lambda: paley_hadamard_i(19), 12: lambda: paley_hadamard_i(11)}


def get_hadK(n: int, transpose: bool = False):
    """(hadK, K) with the reference's decision ladder (hadamard_utils.py:7-60): the first K of 172, 156, 140, 108,
    60, 52, 36, 28, 40, 20, 12 that divides n (n / K must then be a power of two), else (None, 1) for a power of two."""
    for k in (172, 156, 140, 108, 60, 52, 36, 28, 40, 20, 12):
        if n % k == 0:
            assert (n // k) & (n // k - 1) == 0
            h = _PALEY[k]()           # every order of the reference's ladder is generated (Paley I / II, Williamson)
            return (h.T.contiguous() if transpose else h), k
    assert n & (n - 1) == 0
    return None, 1


def hadamard_matrix(n: int) -> torch.Tensor:
    """The +-1 matrix matmul_hadU applies (hadamard_utils.py:63-85): its radix-2 passes run over the LOW index bits in
    natural order and the K x K table over the rest, i.e. hadK (x) Sylvester(n / K)."""
    had_k, k = get_hadK(n)
    low = sylvester(n // k)
    return low if had_k is None else torch.kron(had_k, low)


def random_hadamard_matrix(size: int, device, seed: int) -> torch.Tensor:
    """matmul_hadU(diag(D)) = diag(D) . H_size^T / float32(sqrt(size)) in float64 (hadamard_utils.py:63-99), any size
    get_hadK accepts (every entry is +-1 over the float32 square root: no rounding depends on summation order)."""
    d = sign_vector(size, seed)
    return ((d[:, None] * hadamard_matrix(size).T) / torch.tensor(size).sqrt()).to(device)


def block_random_hadamard_matrix(total_size: int = 1920, block_size: int = 128, device="cuda", seed: int = 42
                                 ) -> torch.Tensor:
    """Block-diagonal Q with IDENTICAL blocks (every block re-seeds with `seed`,
    rotation_utils.py:69-104)."""
    assert total_size % block_size == 0
    q = random_hadamard_matrix(block_size, device, seed)
    return torch.block_diag(*([q] * (total_size // block_size)))


def sign_mask(d: torch.Tensor) -> Tuple[int, int, int, int]:
    """128 signs -> 4 x uint32, bit j set <=> d[j] == -1."""
    assert d.numel() == 128
    bits = (d.reshape(-1) < 0).to(torch.int64).tolist()
    return tuple(sum(b << k for k, b in enumerate(bits[32 * w:32 * w + 32])) for w in range(4))


def full_sign_words(d: torch.Tensor) -> Tuple[int, ...]:
    """The C signs of the full-width rotation -> C / 32 x uint32, bit j set <=> d[j] == -1 (C % 32 == 0)."""
    assert d.numel() % 32 == 0
    bits = (d.reshape(-1) < 0).to(torch.int64).tolist()
    return tuple(sum(b << k for k, b in enumerate(bits[32 * w:32 * w + 32])) for w in range(len(bits) // 32))


def rotate_weight(w: torch.Tensor, q: torch.Tensor) -> torch.Tensor:
    """Offline weight side: W <- W . Q in float64, back to W's dtype (rotation_utils.py:129-154)."""
    return (w.to(torch.float64) @ q.to(w.device, torch.float64)).to(w.dtype)


def transform_weight(w: torch.Tensor, s: torch.Tensor) -> torch.Tensor:
    """GALT smoothing, weight side: W <- W / s per input channel (transform_model_utils.py:8-28)."""
    return w / s.to(w.device)


# ---- model-level preprocessing, same names as the reference (rotate_utils/rotation_utils.py:129-154,211-243;
# learnable_transformation/transform_model_utils.py:8-28).  `layer` is one AdaLN block with .attn.mat_qkv / .ffn.fc1.
def rotate_mat_qkv(layer, Q) -> None:
    """W_q, W_k, W_v <- W . Q in float64 (row-wise, so rotating the stacked weight at once is the same arithmetic)."""
    w = layer.attn.mat_qkv.weight.data
    layer.attn.mat_qkv.weight.data = rotate_weight(w, Q)


def rotate_fc1(layer, Q) -> None:
    w = layer.ffn.fc1.weight.data
    layer.ffn.fc1.weight.data = rotate_weight(w, Q)


def get_orthogonal_matrix(size: int, mode: str = "hadamard", device=None, seed: int = 42) -> torch.Tensor:
    """rotation_utils.py:57-63 ('random' draws a QR factor from the global RNG there; only 'hadamard' is reproducible
    and used by the reference's drivers)."""
    if mode != "hadamard":
        raise ValueError(f"Unknown mode {mode}" if mode != "random" else "mode 'random' is not provided (unseeded QR)")
    return random_hadamard_matrix(size, device, seed)


def rotate_model(model, device, block_rotate: bool = True) -> None:
    """The reference's offline weight rotation for every block, mat_qkv and fc1 (rotation_utils.py:211-240):
    block_rotate=True - the run scripts' mode - with the block-diagonal Q (128-wide blocks, seed 42);
    block_rotate=False with the full-width randomized Hadamard matrix of size model.C (had60 x 2^5 for 1920, had36 x 2^6
    for 2304).  The ONLINE side of the full-width mode is `rotate_quant_full` / `rotate_quant_full_mx`: one launch that runs
    x . Q as the two small products hadK . X . Sylvester(C / K) on the matrix cores and quantizes the rotated row."""
    if block_rotate:
        q = block_random_hadamard_matrix(total_size=model.C, block_size=128, device=device, seed=42)
    else:
        q = get_orthogonal_matrix(model.C, mode="hadamard", device=device)
    for layer in model.blocks:
        rotate_mat_qkv(layer, q)
        rotate_fc1(layer, q)


def transform_mat_qkv(layer, mat_qkv_best_s) -> None:
    w = layer.attn.mat_qkv.weight.data
    layer.attn.mat_qkv.weight.data = transform_weight(w, mat_qkv_best_s).to(w.dtype)


def transform_fc1(layer, fc1_best_s) -> None:
    w = layer.ffn.fc1.weight.data
    layer.ffn.fc1.weight.data = transform_weight(w, fc1_best_s).to(w.dtype)


def transform_model(model, mat_qkv_best_s, fc1_best_s) -> None:
    """GALT smoothing, weight side: W <- W / s per block with the learned per-channel vectors."""
    for idx, layer in enumerate(model.blocks):
        transform_mat_qkv(layer, mat_qkv_best_s[idx])
        transform_fc1(layer, fc1_best_s[idx])


_DEFAULT_MASK = None
_DEFAULT_MASK_TUPLE = None

try:   # the compiled binding (csrc/quant_cuda_ext.cpp) for the hot, plain calls of the producers
    from . import _native
except ImportError:   # pragma: no cover - build() always produces it
    _native = None
if __import__("os").environ.get("FPQ_NO_NATIVE") == "1":   # the A/B tools time variant builds of the library through ctypes (_lib.use_variant)
    _native = None


def _default_mask_tuple():
    global _DEFAULT_MASK_TUPLE
    if _DEFAULT_MASK_TUPLE is None:
        _DEFAULT_MASK_TUPLE = tuple(int(v) for v in sign_mask(sign_vector(128, 42)))
    return _DEFAULT_MASK_TUPLE


def _mask_arg(d: Optional[torch.Tensor]):
    """The 128 sign bits as the C ABI takes them; the default D (seed 42) is computed once - building it costs more
    host time than the kernel runs."""
    global _DEFAULT_MASK
    if d is None:
        if _DEFAULT_MASK is None:
            _DEFAULT_MASK = (ctypes.c_uint32 * 4)(*sign_mask(sign_vector(128, 42)))   # read-only to the library: shared
        return _DEFAULT_MASK
    return (ctypes.c_uint32 * 4)(*sign_mask(d.cpu()))


_DEFAULT_FULL_WORDS = {}


def _full_words_arg(d: Optional[torch.Tensor], c: int):
    """The C sign bits of the full-width rotation as the C ABI takes them (C / 32 words); the default D (seed 42, C long) once per width."""
    if d is None:
        if c not in _DEFAULT_FULL_WORDS:
            _DEFAULT_FULL_WORDS[c] = (ctypes.c_uint32 * (c // 32))(*full_sign_words(sign_vector(c, 42)))   # read-only to the library: shared
        return _DEFAULT_FULL_WORDS[c]
    if d.numel() != c:
        raise RuntimeError(f"the full-width rotation takes one sign per channel: {c}, got {d.numel()}")
    return (ctypes.c_uint32 * (c // 32))(*full_sign_words(d.cpu()))


def _mod_rows(t: torch.Tensor, bsz: int, c: int) -> torch.Tensor:
    """[B, 1, C] / [B, C] modulation tensor as B contiguous rows (no tensor op when it already is)."""
    if t.is_contiguous() and t.numel() == bsz * c:
        return t
    return t.reshape(bsz, c).contiguous()


def _smooth_ptr(smooth, c, device):
    if smooth is None:
        return None, None
    if smooth.dtype is torch.float32 and smooth.dim() == 1 and smooth.shape[0] == c and smooth.device == device \
            and smooth.is_contiguous():
        return smooth, smooth.data_ptr()          # the usual case: no tensor ops on the host path
    sm = smooth.detach().to(device=device, dtype=torch.float32).reshape(-1).contiguous()
    if sm.numel() == 1:
        sm = sm.expand(c).contiguous()
    if sm.numel() != c:
        raise RuntimeError("smooth must have one entry per channel")
    return sm, sm.data_ptr()


def _g6_table_id(name: str, table: str) -> int:
    return TABLE_IDS[_g6_table(name, table)]


def _gf6_table_id(name: str, table: str) -> int:
    return TABLE_IDS[_gf6_table(name, table, full_only=True)]


# ---- the row producers: rotate / adaLN + rotate / gated residual + adaLN + rotate, then the quantizer (include/fpq.h) -------------
# One row per C entry point holds everything the host side knows about it.  The twelve public functions below are their own
# signatures, docstrings and the refusals that are theirs alone (an emit, a table); behind them `_rotate`, `_adaln_args` and
# `_resid_args` are the three sets of shared argument checks, `_outputs` the one place that shapes an output tensor and `_produce` the
# one call path: the compiled binding for the usual arguments, else ctypes, ending in the one `check(lib().X(...), "X")`.  A new
# operand format is a row (here and in csrc/quant_cuda_ext.cpp's PRODUCER_FORMS) and a public function of a few lines.  The hot call
# is public function -> checks -> `_produce` -> binding: positional all the way, nothing built but the tuple the checks return.
#
# Every entry point takes (x | y, gate, x_out, residual), its `slots` output pointers, rows, C, x's dtype, (scale, shift, their
# dtype, rows per batch, eps) behind an adaLN front, smooth, the sign mask, then what the row says: a table id, an `int kmajor`.
class _Family(NamedTuple):
    form: int                          # the entry point's number in the compiled binding (the index in _native.PRODUCER_ENTRY_POINTS)
    entry: str                         # the C entry point
    km: Union[None, str, bool] = None  # k-major images: None - not written; a name - by a twin entry point; True - an `int kmajor` argument
    table: bool = True                 # a table id follows the sign mask ...
    tables: Optional[Callable[[str, str], int]] = None   # ... of these only: (function, table) -> id or a refusal; None: any of TABLE_IDS
    max_c: Optional[int] = None        # the width cap
    seg: int = 0                       # bytes of codes per 128 elements (64 FP4 nibbles, 96 dense 6-bit codes, 128 E4M3 bytes); 0: fp16 values
    row_scales: bool = False           # one fp16 scale per row, not one per 128 elements
    slots: int = 2                     # output pointers: the outputs, then NULL for each intermediate that was not asked for
    full: bool = False                 # the full-width rotation: C / 32 sign words, not the 128-bit mask; ctypes only (no compiled form)


_FORMS = tuple(_native.PRODUCER_ENTRY_POINTS) if _native is not None else ()


def _family(entry: str, **kw) -> _Family:
    return _Family(_FORMS.index(entry) if entry in _FORMS else -1, entry, **kw)


_ROTATE = _family("fpq_rotate_quant_rows")
_ROTATE_MX = _family("fpq_rotate_quant_rows_codes_mx", km="fpq_rotate_quant_rows_codes_mx_km", table=False, seg=64)
_ROTATE_G6 = _family("fpq_a6w4_rotate_quant_rows_codes", km=True, tables=_g6_table_id, seg=96)
_ROTATE_GF6 = _family("fpq_gf6_rotate_quant_rows_codes", km=True, tables=_gf6_table_id, seg=96)
_ADALN = _family("fpq_adaln_rotate_quant_rows", max_c=4096, slots=3)
_ADALN_MX = _family("fpq_adaln_rotate_quant_rows_codes_mx", km="fpq_adaln_rotate_quant_rows_codes_mx_km", table=False, max_c=4096, seg=64)
_ADALN_G6 = _family("fpq_a6w4_adaln_rotate_quant_rows_codes", km=True, tables=_g6_table_id, max_c=2560, seg=96)
_ADALN_GF6 = _family("fpq_gf6_adaln_rotate_quant_rows_codes", km=True, tables=_gf6_table_id, max_c=2560, seg=96)
_TOKEN = {"values": _family("fpq_adaln_rotate_quant_token_rows", max_c=2560, slots=4),
          "fp8": _family("fpq_adaln_rotate_quant_token_rows_codes_fp8", max_c=2560, seg=128, row_scales=True),
          "fp6": _family("fpq_adaln_rotate_quant_token_rows_codes_fp6", km="fpq_adaln_rotate_quant_token_rows_codes_fp6_km", max_c=2560, seg=96,
                         row_scales=True),
          "bf6": _family("fpq_adaln_rotate_quant_token_rows_codes_f6", km=True, max_c=2560, seg=96, row_scales=True)}
_FULL = _family("fpq_fullrot_quant_rows", full=True)
_FULL_MX = _family("fpq_fullrot_quant_rows_codes_mx", km=True, table=False, seg=64, full=True)
FULL_WIDTHS = (1920, 2304)             # the widths the library builds (include/fpq.h, fpq_fullrot_quant_rows)
_FULL_ADALN = _family("fpq_fullrot_adaln_quant_rows", max_c=max(FULL_WIDTHS), slots=3, full=True)
_FULL_ADALN_MX = _family("fpq_fullrot_adaln_quant_rows_codes_mx", km=True, table=False, max_c=max(FULL_WIDTHS), seg=64, full=True)
_FULL_TOKEN = {"values": _family("fpq_fullrot_quant_token_rows", slots=3, full=True),
               "fp6": _family("fpq_fullrot_quant_token_rows_codes_f6", km=True, seg=96, row_scales=True, full=True)}
_FULL_ADALN_TOKEN = {"values": _family("fpq_fullrot_adaln_quant_token_rows", max_c=max(FULL_WIDTHS), slots=4, full=True),
                     "fp6": _family("fpq_fullrot_adaln_quant_token_rows_codes_f6", km=True, max_c=max(FULL_WIDTHS), seg=96, row_scales=True,
                                    full=True)}
_RESID = _family("fpq_resid_adaln_rotate_quant_rows", max_c=2560, slots=3)
_RESID_MX = _family("fpq_resid_adaln_rotate_quant_rows_codes_mx", km=True, table=False, max_c=2560, seg=64)
_RESID_TOKEN = {"values": _family("fpq_resid_adaln_rotate_quant_token_rows", max_c=2560, slots=4),
                "fp6": _family("fpq_resid_adaln_rotate_quant_token_rows_codes_f6", km=True, max_c=2560, seg=96, row_scales=True)}


def _outputs(fam: _Family, x: torch.Tensor, rows: int, c: int, kmajor: bool, extra: int):
    """What a producer writes: fp16 values of x's shape (and `extra` intermediates of that shape), or operand codes - row-major
    [rows, C/128 * seg], k-major [C/128, rows, seg] - with their scales: fp16 per row; per group fp16 [rows, C/128] or the fp32 scale
    image [C/128, rows rounded up to 4] with its padding zeroed."""
    if not fam.seg:
        out = torch.empty(x.shape, dtype=torch.float16, device=x.device)
        return [out] + [torch.empty_like(out) for _ in range(extra)] if extra else [out]
    codes = torch.empty((c // 128, rows, fam.seg) if kmajor else (rows, c // 128 * fam.seg), dtype=torch.uint8, device=x.device)
    if fam.row_scales:
        return [codes, torch.empty((rows,), dtype=torch.float16, device=x.device)]
    return [codes, kmajor_mx_scales(rows, c, x.device) if kmajor else torch.empty((rows, c // 128), dtype=torch.float16, device=x.device)]


def _produce(name: str, fam: _Family, x: torch.Tensor, c: int, tid: int, d, smooth, kmajor=False, extra: int = 0, sc=None, sh=None,
             seq: int = 0, eps: float = 0.0, y=None, gt=None, inplace: bool = False):
    """The one call of a checked producer.  x: the rows (behind a gated residual: the residual); sc, sh: the modulation rows of an
    adaLN front; y, gt: the gated residual's other two tensors.  The compiled binding takes the usual arguments - default sign
    vector, contiguous x (and y), float32 [C] smooth, no intermediates - everything else goes through ctypes; both end in `fam.entry`.
    Returns the outputs (behind a gated residual x_new first): one tensor as itself, more as a tuple."""
    if _native is not None and fam.form >= 0 and not fam.full and d is None and not extra and x.is_cuda and x.is_contiguous() and (
            smooth is None or (smooth.dtype is torch.float32 and smooth.dim() == 1 and smooth.shape[0] == c and
                               smooth.device == x.device and smooth.is_contiguous())) and (
            sc is None or (sc.device == x.device and sh.device == x.device)) and (y is None or y.is_contiguous()):
        return _native.producer(name, fam.form, x, y, gt, sc, sh, tid, _DEFAULT_MASK_TUPLE or _default_mask_tuple(), smooth, float(eps),
                                kmajor, inplace)
    mask = _full_words_arg(d, c) if fam.full else _mask_arg(d)
    xc = x if x.is_contiguous() else x.contiguous()
    head, first = (xc.data_ptr(),), []
    if y is not None:
        yc = y if y.is_contiguous() else y.contiguous()
        first = [xc if inplace else torch.empty_like(xc)]
        head = (yc.data_ptr(), gt.data_ptr(), first[0].data_ptr(), xc.data_ptr())
    sm, sm_ptr = _smooth_ptr(smooth, c, x.device)
    rows = x.numel() // c
    outs = _outputs(fam, x, rows, c, kmajor, extra)
    entry = fam.km if kmajor and isinstance(fam.km, str) else fam.entry
    with device_guard(x.device):
        check(getattr(lib(), entry)(
            *head, *map(torch.Tensor.data_ptr, outs), *[None] * (fam.slots - len(outs)), rows, c, dtype_id(x.dtype),
            *((sc.data_ptr(), sh.data_ptr(), dtype_id(sc.dtype), seq, float(eps)) if sc is not None else ()), sm_ptr, mask,
            *((tid,) if fam.table else ()), *((1 if kmajor else 0,) if fam.km is True else ()), stream_ptr(x.device)), entry)
    outs = first + outs
    return outs[0] if len(outs) == 1 else tuple(outs)


def _rotate(name: str, fam: _Family, x: torch.Tensor, table, d, smooth, kmajor=False, extra: int = 0):
    """The producers of plain rows, x [..., C]: their checks, then the call."""
    require_gpu(x, name)
    c = x.shape[-1]
    if fam is _ROTATE or fam.full:
        if x.dtype not in (torch.float16, torch.float32):
            raise RuntimeError(f"{name}: x must be float16 or float32, got {x.dtype}")
        if fam.full:
            if c not in FULL_WIDTHS:
                raise RuntimeError(f"{name}: the full-width rotation is built for the widths {FULL_WIDTHS}, got {c}")
        elif c % 128 != 0:
            raise RuntimeError(f"{name}: the last dimension must be a multiple of 128")
    elif x.dtype not in (torch.float16, torch.float32) or c % 128 != 0:
        raise RuntimeError(f"{name}: x must be float16/float32 with a last dimension that is a multiple of 128")
    tid = fam.tables(name, table) if fam.tables else TABLE_IDS[table] if fam.table else 0
    return _produce(name, fam, x, c, tid, d, smooth, kmajor, extra)


def _adaln_args(name: str, fam: _Family, x: torch.Tensor, scale: torch.Tensor, shift: torch.Tensor, table):
    """The checks of the producers with an adaLN front, x [B, L, C]; returns (C, L, scale rows, shift rows, the table id where the
    family takes few tables - it is refused here - or None).  The full-width families refuse x's dtype and width first, as `_rotate` does."""
    if fam.full:
        if x.dtype not in (torch.float16, torch.float32):
            raise RuntimeError(f"{name}: x must be float16 or float32, got {x.dtype}")
        if x.shape[-1] not in FULL_WIDTHS:
            raise RuntimeError(f"{name}: the full-width rotation is built for the widths {FULL_WIDTHS}, got {x.shape[-1]}")
    require_gpu(x, name)
    if x.dim() != 3:
        raise RuntimeError(f"{name}: x must be [B, L, C]")
    bsz, seq, c = x.shape
    if c % 128 != 0 or c > fam.max_c:
        raise RuntimeError(f"{name}: C must be a multiple of 128 and at most {fam.max_c}")
    if scale.dtype != shift.dtype or scale.dtype not in (torch.float16, torch.float32):
        raise RuntimeError(f"{name}: scale and shift must both be float16 or both float32")
    tid = fam.tables(name, table) if fam.tables else None
    return c, seq, _mod_rows(scale, bsz, c), _mod_rows(shift, bsz, c), tid


def rotate_quant(x: torch.Tensor, table: str = "e2m1", d: Optional[torch.Tensor] = None,
                 smooth: Optional[torch.Tensor] = None, return_rotated: bool = False):
    """out = fp_quant_*_per_group_cuda( half(x*smooth) @ half(Q_block) , 128 ) in one launch.

    x: [..., C] fp16 or fp32 on the GPU, C % 128 == 0.  Returns fp16 (and the rotated
    fp16 tensor when return_rotated)."""
    return _rotate("rotate_quant", _ROTATE, x, table, d, smooth, extra=1 if return_rotated else 0)


def rotate_quant_mx(x: torch.Tensor, d: Optional[torch.Tensor] = None, smooth: Optional[torch.Tensor] = None,
                    kmajor: bool = False) -> Tuple[torch.Tensor, torch.Tensor]:
    """rotate_quant(x, "e2m1") emitting the FP4 GEMM's operands instead of values:
    (codes uint8 [rows, C/2], scales fp16 [rows, C/128]); level(code) * scale == rotate_quant(x) bit for bit.
    kmajor: the activation side's k-major images (include/fpq.h) - codes [C/128, rows, 64], scales fp32 [C/128, rows rounded up to 4]."""
    return _rotate("rotate_quant_mx", _ROTATE_MX, x, None, d, smooth, kmajor)


def rotate_quant_full(x: torch.Tensor, table: str = "e2m1", d: Optional[torch.Tensor] = None,
                      smooth: Optional[torch.Tensor] = None, return_rotated: bool = False):
    """out = fp_quant_*_per_group_cuda( half(x*smooth) @ half(Q) , 128 ) in one launch, Q = get_orthogonal_matrix(C) - the
    FULL-WIDTH randomized Hadamard matrix (the reference's `--rotate` without `--block_rotate`; rotate_model(block_rotate=False)
    is the weight side).  x: [..., C] fp16 or fp32 on the GPU, C in FULL_WIDTHS; d: the C signs (default sign_vector(C, 42)).
    Returns fp16 (and the rotated fp16 tensor when return_rotated)."""
    return _rotate("rotate_quant_full", _FULL, x, table, d, smooth, extra=1 if return_rotated else 0)


def rotate_quant_full_mx(x: torch.Tensor, d: Optional[torch.Tensor] = None, smooth: Optional[torch.Tensor] = None,
                         kmajor: bool = False) -> Tuple[torch.Tensor, torch.Tensor]:
    """rotate_quant_full(x, "e2m1") emitting the FP4 GEMM's operands instead of values, byte for byte gemm.quantize_mx of the rotated
    rows: (codes uint8 [rows, C/2], scales fp16 [rows, C/128]), or (kmajor) the k-major images - codes [C/128, rows, 64], scales
    fp32 [C/128, rows rounded up to 4]."""
    return _rotate("rotate_quant_full_mx", _FULL_MX, x, None, d, smooth, kmajor)


def adaln_rotate_quant_full(x: torch.Tensor, scale: torch.Tensor, shift: torch.Tensor, table: str = "e2m1",
                            d: Optional[torch.Tensor] = None, smooth: Optional[torch.Tensor] = None, eps: float = 1e-6,
                            return_intermediates: bool = False):
    """act_quant( matmul( LN(x).mul(scale.add(1)).add_(shift).mul(smooth), Q ) ) in one launch, Q = get_orthogonal_matrix(C) - the
    FULL-WIDTH matrix of rotate_quant_full: adaln_rotate_quant for the reference's `--rotate` without `--block_rotate`.

    x: [B, L, C] fp16/fp32 on the GPU, C in FULL_WIDTHS; scale, shift: [B, 1, C] (or [B, C]), both fp16 or both fp32; d: the C signs
    (default sign_vector(C, 42)).  Returns fp16 [B, L, C] (plus h and the rotated tensor when return_intermediates): h as
    adaln_rotate_quant's, the rest rotate_quant_full(h) bit for bit."""
    name = "adaln_rotate_quant_full"
    c, seq, sc, sh, _ = _adaln_args(name, _FULL_ADALN, x, scale, shift, None)
    return _produce(name, _FULL_ADALN, x, c, TABLE_IDS[table], d, smooth, False, 2 if return_intermediates else 0, sc, sh, seq, eps)


def adaln_rotate_quant_full_mx(x: torch.Tensor, scale: torch.Tensor, shift: torch.Tensor, d: Optional[torch.Tensor] = None,
                               smooth: Optional[torch.Tensor] = None, eps: float = 1e-6, kmajor: bool = False
                               ) -> Tuple[torch.Tensor, torch.Tensor]:
    """adaln_rotate_quant_full(x, scale, shift, "e2m1") emitting the FP4 GEMM's operands instead of values, byte for byte
    gemm.quantize_mx of the rotated rows: (codes uint8 [B*L, C/2], scales fp16 [B*L, C/128]), or (kmajor) the k-major images - codes
    [C/128, B*L, 64], scales fp32 [C/128, B*L rounded up to 4]."""
    name = "adaln_rotate_quant_full_mx"
    c, seq, sc, sh, _ = _adaln_args(name, _FULL_ADALN_MX, x, scale, shift, None)
    return _produce(name, _FULL_ADALN_MX, x, c, 0, d, smooth, kmajor, 0, sc, sh, seq, eps)


def _full_token_form(name: str, forms, table: str, emit: str, kmajor: bool) -> _Family:
    """adaln_rotate_quant_token's refusals - emit against table, kmajor only for the code forms - and the row of the form."""
    if emit not in ("values", "fp6", "bf6"):
        raise RuntimeError(f"{name}: unknown emit {emit!r}")
    if table not in ("e2m3", "e3m2"):
        raise RuntimeError(f"{name}: the per-token quantizer runs on the FP6 tables 'e2m3' / 'e3m2', got {table!r}")
    if emit == "fp6" and table != "e2m3":
        raise RuntimeError(f"{name}: emit='fp6' is the E2M3 operand format")
    if emit == "bf6" and table != "e3m2":
        raise RuntimeError(f"{name}: emit='bf6' is the E3M2 operand format")
    if kmajor and emit == "values":
        raise RuntimeError(f"{name}: kmajor is a layout of the FP6 operand codes (emit='fp6' / 'bf6')")
    return forms["values" if emit == "values" else "fp6"]


def rotate_quant_full_token(x: torch.Tensor, table: str = "e2m3", d: Optional[torch.Tensor] = None,
                            smooth: Optional[torch.Tensor] = None, emit: str = "values", kmajor: bool = False,
                            return_rotated: bool = False):
    """rotate_quant_full for the per-token configurations (W6A6): out = fp6_quant_*_per_token_cuda( half(x*smooth) @ half(Q), 6 ) in
    one launch, Q the FULL-WIDTH matrix, ONE scale per row.  x: [..., C] fp16 or fp32 on the GPU, C in FULL_WIDTHS; d: the C signs.
    emit="values": fp16 of x's shape (and the rotated tensor with return_rotated - rotate_quant_full's bit for bit);
    emit="fp6" (table e2m3) / "bf6" (table e3m2): (dense 6-bit codes uint8 [rows, C * 3 / 4], scales fp16 [rows]) - byte for byte
    gemm.quantize_fp6 of the rotated rows, the operands of gemm.linear_fp6; kmajor: the codes as the activation side's k-major image
    [C/128, rows, 96]."""
    name = "rotate_quant_full_token"
    fam = _full_token_form(name, _FULL_TOKEN, table, emit, kmajor)
    if return_rotated and emit != "values":
        raise RuntimeError(f"{name}: the rotated rows go out with emit='values' only")
    return _rotate(name, fam, x, table, d, smooth, kmajor, 1 if return_rotated else 0)


def adaln_rotate_quant_full_token(x: torch.Tensor, scale: torch.Tensor, shift: torch.Tensor, table: str = "e2m3",
                                  d: Optional[torch.Tensor] = None, smooth: Optional[torch.Tensor] = None, eps: float = 1e-6,
                                  emit: str = "values", kmajor: bool = False, return_intermediates: bool = False):
    """adaln_rotate_quant_token with the FULL-WIDTH matrix of rotate_quant_full: LayerNorm, modulate, smooth, x . Q, then
    fp6_quant_*_per_token_cuda with one scale per token row - one launch (W6A6 under the reference's `--rotate` without
    `--block_rotate`).  x: [B, L, C], C in FULL_WIDTHS; scale, shift: [B, 1, C] (or [B, C]), both fp16 or both fp32.
    emit="values": fp16 [B, L, C] (plus h and the rotated tensor with return_intermediates: adaln_rotate_quant_full's bit for bit);
    emit="fp6" / "bf6": (dense 6-bit codes uint8 [B*L, C * 3 / 4], scales fp16 [B*L]) for gemm.linear_fp6, kmajor: the k-major image
    [C/128, B*L, 96]."""
    name = "adaln_rotate_quant_full_token"
    fam = _full_token_form(name, _FULL_ADALN_TOKEN, table, emit, kmajor)
    if return_intermediates and emit != "values":
        raise RuntimeError(f"{name}: the intermediates go out with emit='values' only")
    c, seq, sc, sh, _ = _adaln_args(name, fam, x, scale, shift, None)
    return _produce(name, fam, x, c, TABLE_IDS[table], d, smooth, kmajor, 2 if return_intermediates else 0, sc, sh, seq, eps)


def adaln_rotate_quant_mx(x: torch.Tensor, scale: torch.Tensor, shift: torch.Tensor, d: Optional[torch.Tensor] = None,
                          smooth: Optional[torch.Tensor] = None, eps: float = 1e-6, kmajor: bool = False
                          ) -> Tuple[torch.Tensor, torch.Tensor]:
    """adaln_rotate_quant(x, scale, shift, "e2m1") emitting (codes uint8 [B*L, C/2], scales fp16 [B*L, C/128]).
    kmajor (C <= 2560): the activation side's k-major images - codes [C/128, B*L, 64], scales fp32 [C/128, B*L rounded up to 4]."""
    name = "adaln_rotate_quant_mx"
    c, seq, sc, sh, _ = _adaln_args(name, _ADALN_MX, x, scale, shift, None)
    return _produce(name, _ADALN_MX, x, c, 0, d, smooth, kmajor, 0, sc, sh, seq, eps)


def rotate_quant_g6(x: torch.Tensor, table: str = "e3m0", d: Optional[torch.Tensor] = None, smooth: Optional[torch.Tensor] = None,
                    kmajor: bool = False) -> Tuple[torch.Tensor, torch.Tensor]:
    """rotate_quant(x, table) for table "e1m2" / "e3m0" emitting the A6W4 GEMM's activation operands instead of values:
    (dense 6-bit codes uint8 [rows, C * 3 / 4], scales fp16 [rows, C/128]) - byte for byte gemm.quantize_g6 of the rotated rows, so
    level(code) * scale == rotate_quant(x, table) bit for bit.
    kmajor: the activation side's k-major images (include/fpq.h) - codes [C/128, rows, 96], scales fp32 [C/128, rows rounded up to 4]."""
    return _rotate("rotate_quant_g6", _ROTATE_G6, x, table, d, smooth, kmajor)


def adaln_rotate_quant_g6(x: torch.Tensor, scale: torch.Tensor, shift: torch.Tensor, table: str = "e3m0",
                          d: Optional[torch.Tensor] = None, smooth: Optional[torch.Tensor] = None, eps: float = 1e-6,
                          kmajor: bool = False) -> Tuple[torch.Tensor, torch.Tensor]:
    """adaln_rotate_quant(x, scale, shift, table) for table "e1m2" / "e3m0" emitting the A6W4 GEMM's activation operands:
    (dense 6-bit codes uint8 [B*L, C * 3 / 4], scales fp16 [B*L, C/128]) - byte for byte gemm.quantize_g6 of the rotated rows.  C <= 2560.
    kmajor: the k-major images - codes [C/128, B*L, 96], scales fp32 [C/128, B*L rounded up to 4]."""
    name = "adaln_rotate_quant_g6"
    c, seq, sc, sh, tid = _adaln_args(name, _ADALN_G6, x, scale, shift, table)
    return _produce(name, _ADALN_G6, x, c, tid, d, smooth, kmajor, 0, sc, sh, seq, eps)


def rotate_quant_gf6(x: torch.Tensor, table: str = "e2m3", d: Optional[torch.Tensor] = None, smooth: Optional[torch.Tensor] = None,
                     kmajor: bool = False) -> Tuple[torch.Tensor, torch.Tensor]:
    """rotate_quant(x, table) for the full FP6 tables "e2m3" / "e3m2" (or "fp6_e2m3" / "fp6_e3m2") emitting per-group operands instead
    of values: (dense 6-bit codes uint8 [rows, C * 3 / 4], scales fp16 [rows, C/128]) - byte for byte gemm.quantize_gf6 of the rotated
    rows, so level(code) * scale == rotate_quant(x, table) bit for bit.  The operands of gemm.linear_g6* / FP6GroupLinear.
    kmajor: the activation side's k-major images (include/fpq.h) - codes [C/128, rows, 96], scales fp32 [C/128, rows rounded up to 4]."""
    return _rotate("rotate_quant_gf6", _ROTATE_GF6, x, table, d, smooth, kmajor)


def adaln_rotate_quant_gf6(x: torch.Tensor, scale: torch.Tensor, shift: torch.Tensor, table: str = "e2m3",
                           d: Optional[torch.Tensor] = None, smooth: Optional[torch.Tensor] = None, eps: float = 1e-6,
                           kmajor: bool = False) -> Tuple[torch.Tensor, torch.Tensor]:
    """adaln_rotate_quant(x, scale, shift, table) for the full FP6 tables "e2m3" / "e3m2" emitting per-group operands:
    (dense 6-bit codes uint8 [B*L, C * 3 / 4], scales fp16 [B*L, C/128]) - byte for byte gemm.quantize_gf6 of the rotated rows.  C <= 2560.
    kmajor: the k-major images - codes [C/128, B*L, 96], scales fp32 [C/128, B*L rounded up to 4]."""
    name = "adaln_rotate_quant_gf6"
    c, seq, sc, sh, tid = _adaln_args(name, _ADALN_GF6, x, scale, shift, table)
    return _produce(name, _ADALN_GF6, x, c, tid, d, smooth, kmajor, 0, sc, sh, seq, eps)


def adaln_rotate_quant_token(x: torch.Tensor, scale: torch.Tensor, shift: torch.Tensor, table: str = "e2m3",
                             d: Optional[torch.Tensor] = None, smooth: Optional[torch.Tensor] = None, eps: float = 1e-6,
                             emit: str = "values", kmajor: bool = False):
    """The fused producer for the per-token configurations (W6A6): LayerNorm, modulate, smooth, rotate, then
    fp6_quant_*_per_token_cuda with one scale per token row.  emit="values": fp16 [B, L, C];
    emit="fp8": (codes uint8 [B*L, C], scales fp16 [B*L]) for gemm.linear_fp8; emit="fp6" (table e2m3 only):
    (dense 6-bit codes uint8 [B*L, C * 3 / 4], scales) for gemm.linear_fp6; emit="bf6" (table e3m2 only): the same shapes with BF6
    E3M2 codes, for gemm.linear_fp6(..., a_table="e3m2").  C <= 2560.
    kmajor (emit="fp6" / "bf6" only): the codes as the activation side's k-major image [C/128, B*L, 96]."""
    name = "adaln_rotate_quant_token"
    c, seq, sc, sh, _ = _adaln_args(name, _TOKEN["values"], x, scale, shift, table)
    if emit not in _TOKEN:
        raise RuntimeError(f"{name}: unknown emit {emit!r}")
    if emit == "fp6" and table != "e2m3":
        raise RuntimeError(f"{name}: emit='fp6' is the E2M3 operand format")
    if emit == "bf6" and table != "e3m2":
        raise RuntimeError(f"{name}: emit='bf6' is the E3M2 operand format")
    if kmajor and emit not in ("fp6", "bf6"):
        raise RuntimeError(f"{name}: kmajor is a layout of the FP6 operand codes (emit='fp6' / 'bf6')")
    return _produce(name, _TOKEN[emit], x, c, TABLE_IDS[table], d, smooth, kmajor, 0, sc, sh, seq, eps)


def adaln_rotate_quant(x: torch.Tensor, scale: torch.Tensor, shift: torch.Tensor, table: str = "e2m1",
                       d: Optional[torch.Tensor] = None, smooth: Optional[torch.Tensor] = None, eps: float = 1e-6,
                       return_intermediates: bool = False):
    """act_quant( matmul( LN(x).mul(scale.add(1)).add_(shift).mul(smooth), Q_block ) ) in one launch
    (tr/basic_var.py:263,266 + tr/quant_utils.py:765 under the driver's fp16 autocast).

    x: [B, L, C] fp16/fp32 on the GPU; scale, shift: [B, 1, C] (or [B, C]), both fp16 or both fp32.
    Returns fp16 [B, L, C] (plus h and the rotated tensor when return_intermediates)."""
    name = "adaln_rotate_quant"
    c, seq, sc, sh, _ = _adaln_args(name, _ADALN, x, scale, shift, table)
    return _produce(name, _ADALN, x, c, TABLE_IDS[table], d, smooth, False, 2 if return_intermediates else 0, sc, sh, seq, eps)


# ---- the same producers with the gated residual in front of them folded in (include/fpq.h, fpq_resid_adaln_*) ----
# x_new = residual + y.mul(gate), then the twin on x_new, in one launch.  x_new is bit for bit torch's residual + y.mul(gate) (on fp16
# rows also ops.gate_residual); every other output is byte for byte what the twin returns for x_new.

def _resid_args(name: str, y: torch.Tensor, gate: torch.Tensor, residual: torch.Tensor, scale: torch.Tensor, shift: torch.Tensor,
                inplace: bool):
    """The checks the three functions share; returns (C, L, gate rows, scale rows, shift rows)."""
    require_gpu(residual, name)
    if residual.dim() != 3:
        raise RuntimeError(f"{name}: residual must be [B, L, C]")
    if residual.dtype not in (torch.float16, torch.float32):
        raise RuntimeError(f"{name}: residual must be float16 or float32, got {residual.dtype}")
    bsz, seq, c = residual.shape
    if c % 128 != 0 or c > 2560:
        raise RuntimeError(f"{name}: C must be a multiple of 128 and at most 2560")
    if y.dtype is not torch.float16 or gate.dtype is not torch.float16:
        raise RuntimeError(f"{name}: y and gate must be float16, got {y.dtype} and {gate.dtype}")
    if tuple(y.shape) != tuple(residual.shape):
        raise RuntimeError(f"{name}: y {tuple(y.shape)} must have the shape of residual {tuple(residual.shape)}")
    if gate.numel() != bsz * c or gate.shape[-1] != c:
        raise RuntimeError(f"{name}: gate {tuple(gate.shape)} must be [B, 1, C] (or [B, C]) for residual {tuple(residual.shape)}")
    if scale.dtype != shift.dtype or scale.dtype not in (torch.float16, torch.float32):
        raise RuntimeError(f"{name}: scale and shift must both be float16 or both float32")
    if scale.numel() != bsz * c or shift.numel() != bsz * c:
        raise RuntimeError(f"{name}: scale and shift must be [B, 1, C] (or [B, C]) for residual {tuple(residual.shape)}")
    if y.device != residual.device or gate.device != residual.device:
        raise RuntimeError(f"{name}: y and gate must be on the GPU of residual")
    if inplace and not residual.is_contiguous():
        raise RuntimeError(f"{name}: inplace=True needs a contiguous residual")
    if inplace and y.is_contiguous():   # include/fpq.h: x_out must not overlap y (a copy of a non-contiguous y cannot)
        y0, r0 = y.data_ptr(), residual.data_ptr()
        if y0 < r0 + residual.numel() * residual.element_size() and r0 < y0 + y.numel() * y.element_size():
            raise RuntimeError(f"{name}: inplace=True writes x_new over residual, which must not overlap y")
    return c, seq, _mod_rows(gate, bsz, c), _mod_rows(scale, bsz, c), _mod_rows(shift, bsz, c)


def resid_adaln_rotate_quant(y: torch.Tensor, gate: torch.Tensor, residual: torch.Tensor, scale: torch.Tensor, shift: torch.Tensor,
                             table: str = "e2m1", d: Optional[torch.Tensor] = None, smooth: Optional[torch.Tensor] = None,
                             eps: float = 1e-6, return_intermediates: bool = False, inplace: bool = False):
    """x_new = residual + y.mul(gate); adaln_rotate_quant(x_new, scale, shift, table, ...) - one launch.

    y: [B, L, C] fp16; gate: [B, 1, C] (or [B, C]) fp16; residual: [B, L, C] fp16 or fp32, C <= 2560.  Returns (x_new, out), or
    (x_new, out, h, rotated) with return_intermediates.  inplace: x_new is written over residual (and is that tensor)."""
    name = "resid_adaln_rotate_quant"
    c, seq, gt, sc, sh = _resid_args(name, y, gate, residual, scale, shift, inplace)
    return _produce(name, _RESID, residual, c, TABLE_IDS[table], d, smooth, False, 2 if return_intermediates else 0, sc, sh, seq, eps,
                    y, gt, inplace)


def resid_adaln_rotate_quant_mx(y: torch.Tensor, gate: torch.Tensor, residual: torch.Tensor, scale: torch.Tensor, shift: torch.Tensor,
                                d: Optional[torch.Tensor] = None, smooth: Optional[torch.Tensor] = None, eps: float = 1e-6,
                                kmajor: bool = False, inplace: bool = False):
    """x_new = residual + y.mul(gate); adaln_rotate_quant_mx(x_new, scale, shift, ...) - one launch.  Returns (x_new, codes, scales) in
    the twin's shapes (kmajor: the k-major images).  C <= 2560.  inplace: x_new is written over residual."""
    name = "resid_adaln_rotate_quant_mx"
    c, seq, gt, sc, sh = _resid_args(name, y, gate, residual, scale, shift, inplace)
    return _produce(name, _RESID_MX, residual, c, 0, d, smooth, kmajor, 0, sc, sh, seq, eps, y, gt, inplace)


def resid_adaln_rotate_quant_token(y: torch.Tensor, gate: torch.Tensor, residual: torch.Tensor, scale: torch.Tensor, shift: torch.Tensor,
                                   table: str = "e2m3", d: Optional[torch.Tensor] = None, smooth: Optional[torch.Tensor] = None,
                                   eps: float = 1e-6, emit: str = "values", kmajor: bool = False, inplace: bool = False):
    """x_new = residual + y.mul(gate); adaln_rotate_quant_token(x_new, scale, shift, table, ...) - one launch.
    emit="values": (x_new, fp16 [B, L, C]); emit="fp6": (x_new, dense 6-bit codes, row scales) in the format of `table` ("e2m3": FP6,
    "e3m2": BF6), row-major or (kmajor) the activation side's k-major image.  The FP8 form has no fused twin.  C <= 2560."""
    name = "resid_adaln_rotate_quant_token"
    c, seq, gt, sc, sh = _resid_args(name, y, gate, residual, scale, shift, inplace)
    if emit not in _RESID_TOKEN:
        raise RuntimeError(f"{name}: emit must be 'values' or 'fp6', got {emit!r}")
    if emit == "fp6" and table not in ("e2m3", "e3m2"):
        raise RuntimeError(f"{name}: emit='fp6' writes E2M3 or E3M2 codes, got table {table!r}")
    if kmajor and emit != "fp6":
        raise RuntimeError(f"{name}: kmajor is a layout of the 6-bit operand codes (emit='fp6')")
    return _produce(name, _RESID_TOKEN[emit], residual, c, TABLE_IDS[table], d, smooth, kmajor, 0, sc, sh, seq, eps, y, gt, inplace)

