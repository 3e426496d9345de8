"""What the full-width adaLN producer (fpqvar_amd/csrc/fpq_fulladaln.h; rotation.adaln_rotate_quant_full*) must put into its
modulated row h, and how close it has to come.  Everything behind h - the full-width rotation, the quantizer, the operands - is
rotate_quant_full(h) bit for bit and is held to tests/fullrot_model.py.

The reference, the row families and the unit roundoff are tests/adaln_model.py's; what is this kernel's own:

- depth(C): its summation depth.
- bound(ref, x_dtype, C): adaln_model.bound's derivation for this kernel's arithmetic - always centred (T = 0), the fused modulate.
- emulate(x, scale, shift, smooth, eps, L, mutation): an fp32 model of the shipped statistics and modulate in source order, lane
  by lane in the FrRow operand layout, optionally with one deliberate mistake.
- check(h, ref, x_dtype, C): adaln_model.check with this bound.

Shared by tests/test_fulladaln_model_host.py (CPU) and tests/test_gpu_fulladaln.py (the kernel).
"""
import math
from typing import Optional

import torch

from tests.adaln_model import FAMILIES, U, _fma, _tree, make_case, reference, ulp16  # noqa: F401  (re-exported to the two test files)

WIDTHS = (1920, 2304)
GEOMETRY = {1920: (60, 32), 2304: (36, 64)}      # C = K * m (csrc/fpq_fullrot.h)
MUTATIONS = ("pad_in_centred_sum", "mean_over_padded", "eps_ignored", "var_unbiased", "scale_plus_one_fp32", "batch_off_by_one",
             "smooth_after_round", "stats_of_x_smooth")


def operands(C: int) -> int:
    """KT * KS: the 16-byte operands (8 consecutive channels each) a lane holds of a row."""
    K, m = GEOMETRY[C]
    return (K + 15) // 16 * (m // 32)


def padded(C: int) -> int:
    """The row with its zero segments kj >= K: 16 KT m channels."""
    K, m = GEOMETRY[C]
    return (K + 15) // 16 * 16 * m


def depth(x_dtype, C: int) -> int:
    """Sequential fp32 additions between an element and the row's sum in the full-width adaLN front (csrc/fpq_fulladaln.h, fa_stats), counted from the source:
    8 into the operand's accumulator (fp32 rows: 8 v_add_f32; fp16 rows: 4 v_dot2_f32_f16 of 2 additions each; the centred pass: 8
    v_fma_f32), KT KS - 1 to join the operands' accumulators in turn, 6 levels of wave_sum_dpp.
    C = 1920: 8 + 3 + 6 = 17;  C = 2304: 8 + 5 + 6 = 19 - the same for both row dtypes."""
    return 8 + (operands(C) - 1) + 6


def bound_terms(ref, x_dtype, C: int):
    """(fp32 part, half-ulp part) of bound()."""
    d = depth(x_dtype, C)
    lnA, Bm, A, mabs, damp = ref["lnA"], ref["B"], ref["A"], ref["mabs"], ref["damp"]
    dmu = (d + 3) * U * mabs                                             # |mu^ - mu| rstd (with the rounding of nm)
    e_var = (d + 6) * U * damp + dmu * dmu                               # error of var^ over (var + eps); var = 0: dmu^2 alone
    e_rstd = 0.5 * e_var + 4 * U
    t = (3 * U + e_rstd) * lnA + 2 * U * Bm + dmu * A
    return t, 0.5 * ulp16(ref["h"].abs() + t)


def bound(ref, x_dtype, C: int) -> torch.Tensor:
    """Per-element bound on |float(h_kernel) - h|, first order in U = 2^-24: adaln_model.bound's derivation, step for step, with what
    fpq_fulladaln.h does at each step.  h16 = half(h32), h32 = fma(fma(x, rstd^, nm^), A^, B^) in fp32; d = depth(x_dtype, C).

    1. The final rounding: half an fp16 ulp at |h32| <= |h| + (everything below), the ulp floored at 2^-24.
    2. The mean: mu^ = sum^ * fl(1 / C), |sum^ - sum| <= d U sum|x_i| (the zero segments add exact zeros), the reciprocal and the
       product round once each, nm = -mu^ rstd^ once more:  |mu^ - mu| rstd <= (d + 3) U mean|x| rstd = dmu, on every element as dmu |A|.
    3. The variance - ALWAYS the centred pass, there is no one-pass branch (adaln_model's T = 0): sum (x - mu^)^2 = sum (x - mu)^2 +
       C (mu^ - mu)^2 exactly over the C live channels (the padding's (0 - mu^)^2 never enters, the divisor is C); each difference
       rounds once (2 U on its square), the squares are summed ((d + 2) U), fl(1 / C) and the product round: (d + 6) U relative, plus
       (mu^ - mu)^2 absolute.  Over var + eps: e_var var / (var + eps) + dmu^2.  var^ + eps rounds once, v_rsq_f32 + one Newton step
       is within 3 U:  e_rstd = (that) / 2 + 4 U, on |LN A|.
    4. The modulate, adaln_mfma_kernel's fused chain: fma(x, rstd, nm) rounds once (U |LN|), A^ = fl(half_or_float(scale + 1) s) and
       B^ = fl(shift s) once each, the final fma once (U (|LN A| + |B|)):  3 U |LN A| + 2 U |B|.  (adaln_model.bound takes 5 U |LN A|
       for the sake of its wide kernel's unfused chain; no such kernel here.)

    The summation constant is a count of additions in the source (depth()), not a fit."""
    t, half = bound_terms(ref, x_dtype, C)
    return t + half


def check(h: torch.Tensor, ref, x_dtype, C: int):
    """(worst err / bound over the elements of the finite rows, whether h is non-finite exactly where the reference is)."""
    hd = h.double()
    fin = ref["finite"]
    ratio = ((hd - ref["h"]).abs() / bound(ref, x_dtype, C))[fin]
    worst = float(torch.nan_to_num(ratio, nan=math.inf).max()) if ratio.numel() else 0.0
    return worst, bool(torch.equal(torch.isfinite(hd), torch.isfinite(ref["h"])))


def _lanes(x: torch.Tensor, C: int):
    """The kernel's register layout: [R, operands, 64 lanes, 8], operand o = T KS + s of lane 16 q + i holds the channels
    (16 T + i) m + 32 s + 8 q .. (fr_col0), zeros in the segments 16 T + i >= K; and which (operand, lane) are part of the row."""
    K, m = GEOMETRY[C]
    KT, KS = (K + 15) // 16, m // 32
    lane = torch.arange(64)
    i, q = lane % 16, lane // 16
    col = torch.stack([(16 * T + i) * m + 32 * s + 8 * q for T in range(KT) for s in range(KS)])          # [operands, 64]
    live = torch.stack([(16 * T + i) < K for T in range(KT) for _ in range(KS)])
    idx = col[:, :, None] + torch.arange(8)
    pad = torch.zeros(x.shape[0], padded(C), dtype=torch.float32)
    pad[:, :C] = x.float()
    assert int(idx[live].max()) == C - 1 and int(idx[~live].min()) >= C
    return pad[:, idx], live


def _stats(xf: torch.Tensor, C: int, mutation: Optional[str]):
    """mean, var [R] of fa_stats in fp32: xf [R, C] the values the statistics are taken of."""
    v, live = _lanes(xf, C)
    inv_c = torch.tensor(1.0 / (padded(C) if mutation == "mean_over_padded" else C), dtype=torch.float32)
    nop = v.shape[1]
    a1 = torch.zeros(v.shape[:3])
    for k in range(8):
        a1 = a1 + v[..., k]
    s1 = a1[:, 0]
    for o in range(1, nop):
        s1 = s1 + a1[:, o]
    mean = _tree(s1, True) * inv_c
    a2 = torch.zeros(v.shape[:3])
    for k in range(8):
        d0 = v[..., k] - mean.view(-1, 1, 1)
        a2 = _fma(d0, d0, a2)
    if mutation != "pad_in_centred_sum":
        a2 = a2 * live.float()                                 # the zero padding is not part of the row (whole operands per lane)
    s2 = a2[:, 0]
    for o in range(1, nop):
        s2 = s2 + a2[:, o]
    return mean, _tree(s2, True) * inv_c


def emulate(x: torch.Tensor, scale: torch.Tensor, shift: torch.Tensor, smooth: Optional[torch.Tensor], eps: float, L: int,
            mutation: Optional[str] = None) -> torch.Tensor:
    """h (fp16 [R, C]) as the full-width adaLN front computes it, in fp32 on the CPU, in source order (fa_stats, fa_modulate)."""
    assert mutation is None or mutation in MUTATIONS
    R, C = x.shape
    sm = smooth.float() if smooth is not None else None
    xf = x.float()
    mean, var = _stats(xf * sm if mutation == "stats_of_x_smooth" and sm is not None else xf, C, mutation)
    if mutation == "var_unbiased":
        var = var * torch.tensor(C / (C - 1.0), dtype=torch.float32)
    ve = var if mutation == "eps_ignored" else var + torch.tensor(eps, dtype=torch.float32)
    rstd = (1.0 / torch.sqrt(ve.double())).float()                                       # v_rsq_f32, then one Newton step
    rstd = _fma(rstd * _fma(-ve * rstd, rstd, torch.ones_like(rstd)), torch.tensor(0.5), rstd)
    r = torch.arange(R)
    b = ((r + 1) // L if mutation == "batch_off_by_one" else r // L).clamp_max(scale.shape[0] - 1)
    if scale.dtype == torch.float16 and mutation != "scale_plus_one_fp32":
        sc1 = (scale + 1).float()                                                        # pk_add_f16
    else:
        sc1 = scale.float() + 1.0
    sh = shift.float()
    late = mutation == "smooth_after_round"
    A = sc1 * sm if sm is not None and not late else sc1
    Bm = sh * sm if sm is not None and not late else sh
    mean, rstd = mean.view(R, 1), rstd.view(R, 1)
    nm = -mean * rstd
    h = _fma(_fma(xf, rstd, nm), A[b], Bm[b]).half()
    if sm is not None and late:
        h = (h.float() * sm).half()
    return h
