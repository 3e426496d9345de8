"""What the q / k L2 norm of an attn_l2_norm block (tr/basic_var.py:173-183) must write, and how close the kernels have to come.
Two code sites compute it: FPQ_QK_NORM_ROW (fpqvar_amd/csrc/fpq_gemm_fp4.h; the split epilogues of the FP4, FP6 / BF6 and A6W4
GEMMs) and kv16_step_qkn_kernel (fpqvar_amd/csrc/fpq_fast16.h).  Everything in front of y16 - the fp16 Linear output - is pinned
elsewhere (tests/gemm_model.py); this model starts at y16.

Shared by tests/test_qknorm_model_host.py (CPU: the bound is sound for the kernels' arithmetic in both lane splits and sharp
enough to catch each of a list of plausible kernel mistakes) and tests/test_gpu_qknorm.py (the kernels).

- reference(y16, bias32, head_scale, part): the value in float64 and which elements are finite.
- bound(ref): the per-element bound on |float(kernel) - ref|, derived in its docstring.
- emulate(y16, bias32, head_scale, part, variant, mutation): an fp32 model of the kernels' lines in source order, in either
  lane split, optionally with one deliberate mistake.
- HEADS / make_case: the head families as fp16 rows (the KV step takes them as they are); gemm_plan: the same families as the
  rank-one operands of a GEMM (activation row t = alpha_t on one channel, weight row o = beta_o on the same channel).
"""
import functools
import math
from typing import Dict, Optional, Tuple

import torch

U = 2.0 ** -24                                   # unit roundoff of fp32
C_FP32 = 16                                      # roundings of fp32 between y16 and the value that is rounded to fp16: bound()
EPS = 1e-12
HALF_OVERFLOW = 65520.0                          # |value| >= this rounds to +-inf in fp16 (65504 + half an ulp of 32)
VARIANTS = ("gemm", "kv")                        # 4 values x 16 lanes (FPQ_QK_NORM_ROW), 8 values x 8 lanes (kv16_step_qkn_kernel)
MUTATIONS = ("q_half_before_scale", "bias_before_half", "eps_on_sumsq", "lane_missing", "scale_on_k", "round_toward_zero",
             "inf_residual_unguarded")
FAMILIES = ("gauss", "heavy", "dominant_3000", "dominant_60000", "fp16_max", "subnormal", "cancel", "constant", "norm_tiny",
            "norm_straddle", "zero", "scale_100", "scale_1e5", "inf", "inf_pm", "nan", "inf_nan")
HEADS = FAMILIES + ("norm_straddle",)            # one family per head of 64; an even count (part_cols % 128 == 0)
NONFINITE = ("inf", "inf_pm", "nan", "inf_nan")
H = len(HEADS)
C = 64 * H


# ---------------------------------------------------------------------------------------------------------- the reference
def reference(y16: torch.Tensor, bias32: Optional[torch.Tensor], head_scale: torch.Tensor, part: int, raw: bool = False):
    """y16 fp16 [T, C'] (one of the three column parts), bias32 fp32 [C'] or None, head_scale fp32 [C' / 64]; part 0 q, 1 k, 2 v.
    In float64:  y = y16 + b32 (exact),  n = max(sqrt(sum_head y^2), 1e-12),  q = y / n s_h,  k = y / n,  v = y.
    Heads that are not finite follow the reference's fp32 lines (F.normalize: y / norm.clamp_min(eps)): a NaN anywhere in the head
    makes the norm and so the whole head NaN; with +-inf and no NaN the norm is inf, inf / inf = NaN at the inf elements and
    finite / inf = 0 at the others.  A value of magnitude >= 65520 is expected as +-inf (the fp16 rounding of the result).
    -> (value float64 [T, C'], finite bool [T, C']); raw: the value alone, before the overflow rule"""
    y = y16.double()
    if bias32 is not None:
        y = y + bias32.double()
    if part == 2:
        val = y
    else:
        T, Cp = y.shape
        yh = y.view(T, Cp // 64, 64)
        nan_head = torch.isnan(yh).any(dim=-1, keepdim=True)
        inf_el = torch.isinf(yh)
        inf_head = inf_el.any(dim=-1, keepdim=True) & ~nan_head
        safe = torch.where(torch.isfinite(yh), yh, torch.zeros_like(yh))
        n = torch.sqrt((safe * safe).sum(dim=-1, keepdim=True)).clamp_min(EPS)
        val = safe / n
        if part == 0:
            val = val * head_scale.double().view(1, -1, 1)
        nan = torch.full_like(val, math.nan)
        val = torch.where(inf_head, torch.where(inf_el, nan, torch.zeros_like(val)), val)
        val = torch.where(nan_head, nan, val).view(T, Cp)
    if raw:
        return val
    val = torch.where(val.abs() >= HALF_OVERFLOW, torch.sign(val) * math.inf, val)
    return val, torch.isfinite(val)


def clear_of_overflow(y16, bias32, head_scale, part) -> bool:
    """no value within its bound of 65520, where the fp16 rounding turns to inf: the second input condition of bound()"""
    v = reference(y16, bias32, head_scale, part, raw=True)
    v = v[torch.isfinite(v)]
    return bool(((v.abs() - HALF_OVERFLOW).abs() > bound(v)).all())


def sum_of_squares(y16: torch.Tensor, bias32: Optional[torch.Tensor]) -> torch.Tensor:
    """sum_head y^2 in float64 over the finite heads [T, C' / 64] (0 for the others): the input condition of bound()"""
    y = y16.double() + (bias32.double() if bias32 is not None else 0.0)
    yh = y.view(y.shape[0], -1, 64)
    ss = (yh * yh).sum(dim=-1)
    return torch.where(torch.isfinite(ss), ss, torch.zeros_like(ss))


def ulp16(v: torch.Tensor) -> torch.Tensor:
    """The spacing of fp16 at magnitude v, floored at the subnormal spacing 2^-24."""
    e = torch.floor(torch.log2(v.abs().clamp_min(2.0 ** -14)))
    return torch.exp2(e - 10)


def bound(ref: torch.Tensor) -> torch.Tensor:
    """Per-element bound on |float(kernel's fp16) - ref|:   0.5 ulp16(|ref|) (1 + 2^-12) + C_FP32 2^-24 |ref|.

    Both code sites compute in fp32 and round once to fp16 at the end.  The half-ulp term is that rounding (the ulp floored at
    2^-24 for subnormal results; the factor 1 + 2^-12 covers a value the fp32 error carried over a power of two, where the spacing
    doubles).  The fp32 term counts the roundings in front of it, each a relative error of at most U = 2^-24 (first order), from
    the source of FPQ_QK_NORM_ROW / kv16_step_qkn_kernel:

    1. y = fl(y16 + b32): one rounding.  It moves the element by U and the norm by at most U (every y_i by U):          2 U
    2. the sum of squares: the first product and NT - 1 fmas in a lane, then the DPP tree.  An element passes at most
       NT + log2(64 / NT) additions / roundings: 4 + 4 = 8 in the GEMMs (4 values x 16 lanes), 8 + 3 = 11 in the KV step
       (8 values x 8 lanes).  All terms are positive, so the sum is off by at most 11 U and its root by half of that:    5.5 U
    3. the square root (correctly rounded or within an ulp: 2 U) - the clamp at 1e-12 rounds nothing:                    2 U
       where the clamp applies, 2. and 3. fall away and 1e-12f against 1e-12 is left: under 1 U.
    4. the quotient q = y inv + (y - q n) inv: the residual step takes the error of inv = fl(1 / n) out again, q is the
       correctly rounded y / n^ but for rare ties - the reciprocal costs nothing at first order:                       1 U
    5. * s_h on q rows:                                                                                                1 U
    Sum 11.5 U for q in the KV step (10 U in the GEMMs, one less for k), so C_FP32 = 16: the fp32 term stays below 1 % of the
    half ulp (16 * 2^-24 against 2^-12 at the top of a binade).  Second-order terms are ~1e-13 relative.

    Input conditions (asserted by the tests): sum_head y^2 < 2^120, so the fp32 sum cannot overflow where float64 does not; no
    finite |ref| within its bound of 65520, so the kernel's fp16 is finite exactly where ref is."""
    a = ref.abs()
    return 0.5 * ulp16(a) * (1.0 + 2.0 ** -12) + C_FP32 * U * a


def check(got: torch.Tensor, ref: torch.Tensor, finite: torch.Tensor, heads=HEADS) -> Tuple[Dict[str, float], list]:
    """got fp16 [T, 64 len(heads)] -> (worst err / bound per family over every finite element - signed zeros compare equal, a
    non-finite `got` at a finite element counts as inf; the families in which got is not NaN / +inf / -inf exactly where ref is)."""
    g = got.double().cpu()
    ratio = torch.nan_to_num((g - torch.where(finite, ref, torch.zeros_like(ref))).abs() / bound(ref), nan=math.inf, posinf=math.inf)
    ratio = torch.where(finite, ratio, torch.zeros_like(ratio)).view(g.shape[0], len(heads), 64)
    wrong = (torch.isnan(g) != torch.isnan(ref)) | (torch.isinf(g) != torch.isinf(ref)) | (torch.isinf(ref) & (torch.sign(g) != torch.sign(ref)))
    wrong = wrong.view(g.shape[0], len(heads), 64)
    worst: Dict[str, float] = {}
    for h, f in enumerate(heads):
        worst[f] = max(worst.get(f, 0.0), float(ratio[:, h].max()))
    return worst, sorted({heads[h] for h in wrong.any(dim=2).any(dim=0).nonzero().flatten().tolist()})


# ------------------------------------------------------------------------------------------------------- the fp32 model
def _fma(a, b, c):
    return (a.double() * b.double() + c.double()).float()


def _tree(v: torch.Tensor) -> torch.Tensor:
    """row_sum16 / head_sum8: quad_perm [1,0,3,2], quad_perm [2,3,0,1], row_half_mirror(, row_mirror) - partners at distance 1, 2,
    the other quad, the other half: the pairwise tree over adjacent lanes"""
    while v.shape[-1] > 1:
        v = v[..., 0::2] + v[..., 1::2]
    return v[..., 0]


def _half_toward_zero(x: torch.Tensor) -> torch.Tensor:
    h = x.half()
    over = (h.float().abs() > x.abs()) & ~torch.isnan(x)
    return (h.view(torch.int16) - over.to(torch.int16)).view(torch.float16)


def emulate(y16: torch.Tensor, bias32: Optional[torch.Tensor], head_scale: torch.Tensor, part: int, variant: str = "gemm",
            mutation: Optional[str] = None) -> torch.Tensor:
    """The kernels' lines in fp32 on the CPU, in source order (fma through float64) -> fp16 [T, C'].
    variant "gemm": a lane holds 4 consecutive values of the head, 16 lanes; "kv": 8 values, 8 lanes.
    mutation: one deliberate mistake -
      q_half_before_scale     q rounded to fp16 before * s_h            bias_before_half   y = float(half(y16 + b32))
      eps_on_sumsq            sqrt(max(sum, 1e-12))                     lane_missing       one lane left out of the row sum
      scale_on_k              k rows multiplied by s_h too              round_toward_zero  the last conversion truncates
      inf_residual_unguarded  the residual step multiplies by the norm even when it is inf / NaN (the kernels as they were)"""
    assert variant in VARIANTS and (mutation is None or mutation in MUTATIONS)
    T, Cp = y16.shape
    heads = Cp // 64
    y = y16.float()
    if bias32 is not None:
        y = (y + bias32).half().float() if mutation == "bias_before_half" else y + bias32
    to_half = _half_toward_zero if mutation == "round_toward_zero" else (lambda t: t.half())
    if part == 2:
        return to_half(y)
    nt = 4 if variant == "gemm" else 8
    v = y.view(T, heads, 64 // nt, nt)
    ss = v[..., 0] * v[..., 0]
    for n in range(1, nt):
        ss = _fma(v[..., n], v[..., n], ss)
    if mutation == "lane_missing":
        ss = ss.clone()
        ss[..., 5] = 0.0
    s = _tree(ss)
    eps = torch.tensor(EPS, dtype=torch.float32)
    if mutation == "eps_on_sumsq":
        nrm = torch.sqrt(torch.where(s < eps, eps, s))
    else:
        nrm = torch.sqrt(s)
        nrm = torch.where(nrm < eps, eps, nrm)                       # a NaN stays a NaN
    inv = 1.0 / nrm
    nrm_r = nrm if mutation == "inf_residual_unguarded" else torch.where(nrm < math.inf, nrm, torch.zeros_like(nrm))
    yh = y.view(T, heads, 64)
    inv, nrm_r = inv.unsqueeze(-1), nrm_r.unsqueeze(-1)
    q = yh * inv
    q = _fma(_fma(-q, nrm_r, yh), inv, q)
    if mutation == "q_half_before_scale":
        q = q.half().float()
    if part == 0 or mutation == "scale_on_k":
        q = q * head_scale.float().view(1, heads, 1)
    return to_half(q.reshape(T, Cp))


def torch_lines(y16: torch.Tensor, bias32: Optional[torch.Tensor], head_scale: torch.Tensor, part: int) -> torch.Tensor:
    """tr/basic_var.py:176-183 in fp32 torch ops on the CPU -> fp16 [T, C']"""
    y = y16.float() + (bias32 if bias32 is not None else 0.0)
    if part == 2:
        return y.half()
    q = torch.nn.functional.normalize(y.view(y.shape[0], -1, 64), dim=-1)
    if part == 0:
        q = q.mul(head_scale.float().view(1, -1, 1))
    return q.reshape(y.shape).half()


# ---------------------------------------------------------------------------------------------------------------- inputs
def head_scales(s_h: float) -> torch.Tensor:
    """fp32 [H]: s_h on every head but the two whose family is a head scale"""
    hs = torch.full((H,), s_h, dtype=torch.float32)
    hs[HEADS.index("scale_100")] = 100.0
    hs[HEADS.index("scale_1e5")] = 1.0e5
    return hs


def _signs(shape, g):
    return torch.randint(0, 2, shape, generator=g).double() * 2 - 1


def _spiked(T, g):
    """gauss clamped to +-2.5 with one element of +-10: y / n is 0.78 there and at most 0.2 elsewhere (times 1e5: one overflow)"""
    v = torch.randn(T, 64, generator=g, dtype=torch.float64).clamp(-2.5, 2.5)
    v[torch.arange(T), torch.randint(0, 64, (T,), generator=g)] = 10.0 * _signs((T,), g)
    return v


def _straddle(slot: int, g) -> torch.Tensor:
    """64 elements of ~1.25e-13: the norm is 1e-12 times 1 -+ 4e-3 / 1 -+ 1e-4 (slot 0 .. 3: below, below, above, above)"""
    f = (1 - 4e-3, 1 - 1e-4, 1 + 1e-4, 1 + 4e-3)[slot]
    v = 1.25e-13 * _signs((64,), g) * (1 + 1e-2 * torch.randn(64, generator=g, dtype=torch.float64))
    return v * (f * 1e-12 / float(v.norm()))


def _family_rows(fam: str, T: int, slot: int, g) -> Tuple[torch.Tensor, torch.Tensor]:
    """(y16 values float64 [T, 64] before the cast, bias float64 [64]) of one head and part; slot: 0 .. 3, which of the
    straddle heads' norms"""
    z = torch.randn(T, 64, generator=g, dtype=torch.float64)
    bias = 0.1 * torch.randn(64, generator=g, dtype=torch.float64)
    zero = torch.zeros(64, dtype=torch.float64)
    if fam in ("gauss", "scale_100"):
        return z * torch.exp(torch.randn(T, 1, generator=g, dtype=torch.float64)), bias
    if fam == "scale_1e5":
        return _spiked(T, g), zero
    if fam == "heavy":
        return (z * torch.exp(2.5 * torch.randn(T, 64, generator=g, dtype=torch.float64))).clamp(-6.0e4, 6.0e4), bias
    if fam.startswith("dominant_"):
        big, small = (3000.0, 1e-2) if fam.endswith("_3000") else (60000.0, 1e-3)
        v = small * _signs((T, 64), g) * (0.5 + torch.rand(T, 64, generator=g, dtype=torch.float64))
        v[torch.arange(T), torch.randint(0, 64, (T,), generator=g)] = big * _signs((T,), g)
        return v, zero
    if fam == "fp16_max":
        return _signs((T, 64), g) * (60000.0 + 5000.0 * torch.rand(T, 64, generator=g, dtype=torch.float64)), zero
    if fam == "subnormal":
        return _signs((T, 64), g) * 6.0e-5 * torch.rand(T, 64, generator=g, dtype=torch.float64), zero
    if fam == "cancel":                                       # every row within 2^-8 of -bias
        b = torch.randn(64, generator=g, dtype=torch.float64)
        return -b * (1 + 2.0 ** -8 * z), b
    if fam == "constant":
        return (0.75 * torch.exp2(torch.randint(-3, 4, (T, 1), generator=g).double()) * _signs((T, 1), g)).expand(T, 64).clone(), zero
    if fam == "norm_tiny":
        return torch.zeros(T, 64, dtype=torch.float64), torch.linspace(-3e-14, 4e-14, 64, dtype=torch.float64)
    if fam == "norm_straddle":
        return torch.zeros(T, 64, dtype=torch.float64), _straddle(slot, g)
    if fam == "zero":
        return torch.zeros(T, 64, dtype=torch.float64) * _signs((T, 64), g), zero
    v = z.clone()                                             # the non-finite heads: gauss rows with one or two elements replaced
    j = torch.randint(0, 32, (T,), generator=g)
    r = torch.arange(T)
    if fam in ("inf", "inf_pm", "inf_nan"):
        v[r, j] = math.inf
    if fam == "inf_pm":
        v[r, j + 32] = -math.inf
    if fam in ("nan", "inf_nan"):
        v[r, j + 16] = math.nan
    return v, bias


@functools.lru_cache(maxsize=None)
def make_case(T: int, s_h: float, seed: int = 0):
    """(y16 fp16 [T, 3, C], bias fp32 [3, C], head scales fp32 [H]) on the CPU: head h of every part holds family HEADS[h], every
    token row its own draw.  Treat them as read-only (the case is cached)."""
    g = torch.Generator().manual_seed(1000 * seed + T)
    y = torch.zeros(T, 3, C, dtype=torch.float64)
    b = torch.zeros(3, C, dtype=torch.float64)
    for part in range(3):
        seen = 0
        for h, fam in enumerate(HEADS):
            slot = 2 * seen + (part & 1)
            seen += fam == "norm_straddle"
            y[:, part, 64 * h:64 * h + 64], b[part, 64 * h:64 * h + 64] = _family_rows(fam, T, slot % 4, g)
    return y.half(), b.float(), head_scales(s_h)


# The same families as a rank-one product: y16[t, o] = half(alpha_t beta_o).  beta is the within-head pattern, the fp32 bias sets
# what a product cannot (the norms around 1e-12, NaN columns, the cancellation against token 0's row), zero operands leave y = bias
# exactly, a large alpha overflows half(acc) to inf - the way an inf really arises - and a NaN activation scale poisons a token.
ALPHAS = (1.0, -1.0, 0.5, 1.0, 0.0, 2.0, 40.0, 0.25)            # token t takes ALPHAS[t % 8] (token 0: 1.0)


@functools.lru_cache(maxsize=None)
def gemm_plan(T: int, s_h: float, seed: int = 0):
    """(alpha float32 [T], beta float32 [3 C], bias fp32 [3 C] without the cancellation head's entries, head scales fp32 [H], the
    token whose activation scale is to be NaN or None).  The cancellation head's bias comes from the GEMM's own y16 (cancel_bias)."""
    g = torch.Generator().manual_seed(77 + 1000 * seed)
    beta = torch.zeros(3, C, dtype=torch.float64)
    bias = torch.zeros(3, C, dtype=torch.float64)
    for part in range(3):
        seen = 0
        for h, fam in enumerate(HEADS):
            slot = 2 * seen + (part & 1)
            seen += fam == "norm_straddle"
            v, b = _family_rows(fam, 1, slot % 4, g)
            v = v[0]
            inf_at, nan_at = torch.isinf(v), torch.isnan(v)
            v = torch.where(inf_at, torch.sign(v) * 1.0e5, torch.where(nan_at, torch.ones_like(v), v))   # alpha 1: half(1e5) = inf
            b = torch.where(nan_at, torch.full_like(b, math.nan), b)
            if fam == "cancel":
                v, b = torch.randn(64, generator=g, dtype=torch.float64), torch.zeros(64, dtype=torch.float64)
            beta[part, 64 * h:64 * h + 64], bias[part, 64 * h:64 * h + 64] = v, b
    alpha = torch.tensor([ALPHAS[t % len(ALPHAS)] for t in range(T)], dtype=torch.float32)
    return alpha, beta.float().view(-1), bias.float().view(-1), head_scales(s_h), (T - 2 if T >= 8 else None)


def cancel_bias(bias: torch.Tensor, y16: torch.Tensor, seed: int = 0) -> torch.Tensor:
    """bias [3 C] with the cancellation head's entries set to -(token 0's y16 there) (1 + 2^-8 z): y16 ~ -bias on the tokens with
    alpha = 1.  y16: the plain GEMM's output [T, 3 C]."""
    g = torch.Generator().manual_seed(5 + seed)
    out = bias.clone()
    h = HEADS.index("cancel")
    for part in range(3):
        cols = slice(part * C + 64 * h, part * C + 64 * h + 64)
        out[cols] = (-y16[0, cols].double().cpu() * (1 + 2.0 ** -8 * torch.randn(64, generator=g, dtype=torch.float64))).float().to(out.device)
    return out
