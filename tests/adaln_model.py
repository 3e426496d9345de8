"""What the fused LayerNorm + adaLN producer (fpqvar_amd/csrc/fpq_adaln.h) must put into its modulated row h, and how close it
has to come.  Everything downstream of h - rotation, quantizer, operands, images - is bit-exact given h and is tested as such.

Shared by tests/test_adaln_model_host.py (CPU: the bound is sound for the kernels' arithmetic in every summation order they
use, and sharp enough to catch each of a list of plausible kernel mistakes) and tests/test_gpu_adaln.py (the kernels).

- reference(x, scale, shift, smooth, eps, L): h in float64 with the magnitudes the bound needs.
- bound(ref, x_dtype, C): the per-element bound on |float(h_kernel) - h|, derived in its docstring.
- emulate(x, scale, shift, smooth, eps, L, order, mutation): an fp32 model of each kernel's arithmetic in source order,
  optionally with one deliberate mistake.
- FAMILIES / make_rows / make_case: the input rows both test files run; the families are rows of ONE tensor.
- quantized_groups(h): the stages behind h on the CPU, to count the groups two summation orders quantize differently.
"""
import functools
import math
from typing import Dict, Optional

import torch

U = 2.0 ** -24                                   # unit roundoff of fp32
ORDERS = ("lane_tree", "slot_hi", "pair2")
MUTATIONS = ("one_pass_always", "pad_subtract", "eps_ignored", "scale_plus_one_fp32", "batch_off_by_one", "var_unbiased",
             "smooth_after_round", "mean_over_padded", "second_row_takes_first_rows_stats")
WIDE_FROM = 2560                                 # C above this: adaln_rotate_quant16_kernel (one workgroup per row)
FAMILIES = ("gauss", "lognormal", "rho2_7.2", "rho2_8.8", "rho2_57.6", "rho2_70.4", "rho_30", "rho_high", "constant",
            "var_eps", "mag_1e4", "inf", "nan")
SHARE_CAPPED = ("gauss", "lognormal")            # families whose share of not-bit-equal groups is capped (test (c))


def switch_point(x_dtype) -> float:
    """T: adaln_mfma_kernel centres when !(mean^2 < T var); 0 for a kernel that always centres."""
    return 64.0 if x_dtype == torch.float16 else 8.0


def maxc(C: int) -> int:
    return (C + 511) // 512


def depth(x_dtype, C: int) -> int:
    """Sequential fp32 additions between an element and the row's sum, the longest over the kernels and orders that can run
    rows of this dtype and width (each addition rounds once: |sum^ - sum| <= depth U sum|x_i|, first order).
    adaln_mfma_kernel, fp16 rows: 4 v_dot2 of 2 additions each per chunk accumulator, MAXC - 1 to join the accumulators, 6
    levels of the wavefront tree; its PAIR2 centred pass (C = 1024) runs ONE accumulator over the row's 2 chunks: 16 + 6.
    fp32 rows: 4 additions per register accumulator, 2 MAXC - 1 to join them, 6 levels.
    adaln_rotate_quant16_kernel: 16 sequential additions per lane (2 vectors of 8; the centred pass: 8 + 2), 6 levels, 3 to join
    the 4 wavefronts."""
    if C > WIDE_FROM:
        return 16 + 6 + 3
    m = maxc(C)
    if x_dtype == torch.float16:
        return 22 if C == 1024 else 8 + (m - 1) + 6
    return 4 + (2 * m - 1) + 6


# ---------------------------------------------------------------------------------------------------------- the reference
def scale_plus_one(scale: torch.Tensor) -> torch.Tensor:
    """scale + 1 as the reference's torch op rounds it: an fp16 add for fp16 modulation, an fp32 add for fp32."""
    return (scale + 1).double()


def reference(x: torch.Tensor, scale: torch.Tensor, shift: torch.Tensor, smooth: Optional[torch.Tensor], eps: float,
              L: int) -> Dict[str, torch.Tensor]:
    """x [R, C] fp16 / fp32; scale, shift [B, C] fp16 / fp32; smooth [C] fp32 or None; row r uses batch entry r // L.
    h = ((x - mu) / sqrt(var + eps)) A + B in float64, var the biased variance, A = (scale + 1) s, B = shift s."""
    R, C = x.shape
    xd = x.double()
    s = smooth.double() if smooth is not None else torch.ones(C, dtype=torch.float64, device=x.device)
    b = torch.arange(R, device=x.device) // L
    A = (scale_plus_one(scale) * s)[b]
    Bm = (shift.double() * s)[b]
    mu = xd.mean(dim=1, keepdim=True)
    var = ((xd - mu) ** 2).mean(dim=1, keepdim=True)
    rstd = 1.0 / torch.sqrt(var + eps)
    ln = (xd - mu) * rstd
    return {"h": ln * A + Bm, "lnA": (ln * A).abs(), "B": Bm.abs(), "A": A.abs(),
            "mabs": xd.abs().mean(dim=1, keepdim=True) * rstd,          # mean|x| rstd   (times |A|: the mean's error in h)
            "rho2": mu * mu / var, "damp": var / (var + eps),           # per row [R, 1]
            "finite": torch.isfinite(xd).all(dim=1)}


def ulp16(v: torch.Tensor) -> torch.Tensor:
    """The spacing of fp16 at magnitude v, floored at the subnormal spacing 2^-24."""
    e = torch.floor(torch.log2(v.abs().clamp_min(2.0 ** -14)))
    return torch.exp2(e - 10)


def bound_terms(ref, x_dtype, C: int):
    """(fp32 part, half-ulp part) of bound()."""
    d = depth(x_dtype, C)
    T = 0.0 if C > WIDE_FROM else switch_point(x_dtype)
    lnA, Bm, A, mabs, rho2, damp = ref["lnA"], ref["B"], ref["A"], ref["mabs"], ref["rho2"], ref["damp"]
    dmu = (d + 3) * U * mabs                                             # |mu^ - mu| rstd (with the rounding of nm)
    amp = 1.0 + torch.nan_to_num(rho2, nan=0.0, posinf=math.inf).clamp_max(T)
    one_pass = (3 * (d + 2) + 1) * U * amp if T else torch.zeros_like(amp)
    e_var = torch.clamp_min(one_pass, (d + 6) * U) * damp + dmu * dmu    # error of var^ over (var + eps); var = 0: dmu^2 alone
    e_rstd = 0.5 * e_var + 4 * U
    t = (5 * U + e_rstd) * lnA + 2 * U * Bm + dmu * A
    return t, 0.5 * ulp16(ref["h"].abs() + t)


def bound(ref, x_dtype, C: int) -> torch.Tensor:
    """Per-element bound on |float(h_kernel) - h|, first order in U = 2^-24, from the source of fpq_adaln.h.

    Both kernels compute  h16 = half(h32),  h32 = (x - mu^) rstd^ A^ + B^  in fp32.  With d = depth(x_dtype, C):

    1. The final rounding: half an fp16 ulp at |h32| <= |h| + (everything below); the ulp is floored at 2^-24 (subnormals).
    2. The mean: mu^ = sum^ * fl(1 / C).  |sum^ - sum| <= d U sum|x_i|, the reciprocal and the product round once each, and
       adaln_mfma_kernel rounds nm = -mu^ rstd^ once more (relative U of |mu| <= mean|x|):  |mu^ - mu| rstd <= (d + 3) U mean|x|
       rstd = dmu.  It enters h as dmu |A| on EVERY element of the row - it scales with mean|x|, not |mu|, which is why a
       constant row comes out as B +- dmu |A| and not as B exactly.
    3. The variance, relative error e_var:
       - one pass (adaln_mfma_kernel while mean^2 < T var^; T = 64 on fp16 rows, 8 on fp32 rows):  var^ = fma(-mu^, mu^,
         fl(sum2^ / C)).  E[x^2]^ is off by (d + 2) U E[x^2], mu^^2 by 2 (d + 2) U |mu| mean|x| <= 2 (d + 2) U E[x^2] (Cauchy-
         Schwarz), the fma rounds once: absolute (3 (d + 2) + 1) U (var + mu^2), relative (3 (d + 2) + 1) U (1 + rho^2).  The kernel
         takes this branch only while rho^^2 < T, so rho^2 is capped at T; the test cannot know which side of the switch a row
         near it took and takes the larger of the two branches' errors.
       - centred (otherwise, and the wide kernel always): sum (x - mu^)^2 = sum (x - mu)^2 + C (mu^ - mu)^2 exactly; each
         difference rounds once (relative U, so 2 U on its square), the squares are summed ((d + 2) U) and fl(1/C), the product
         round: (d + 6) U, plus (mu^ - mu)^2 absolute.
       Over var + eps, which is what rstd sees: e_var var / (var + eps) + dmu^2 (dmu already carries rstd; on a constant row
       only this term is left).  Then var^ + eps rounds once, the reciprocal square root (v_rsq_f32 + one Newton step; the
       wide kernel: sqrt and divide) is within 3 U:  e_rstd = (that) / 2 + 4 U, on |LN A|.
    4. The modulate: adaln_mfma_kernel - fma(x, rstd, nm) rounds once (U |LN|), A^ = fl(half(scale + 1) s) and B^ = fl(shift s)
       once each, the final fma once (U |h| <= U (|LN A| + |B|)): 3 U |LN A| + 2 U |B|.  The wide kernel's unfused chain
       x - mu^, * rstd, * (scale + 1), + shift, * s rounds five times: 5 U |LN A| + 2 U |B|.  The bound takes the latter.

    The summation constants are counts of additions in the source (depth()), not fits."""
    t, half = bound_terms(ref, x_dtype, C)
    return t + half


# ------------------------------------------------------------------------------------------------------- the fp32 model
def _fma(a, b, c):
    return (a.double() * b.double() + c.double()).float()


def _tree(v: torch.Tensor, ascending: bool) -> torch.Tensor:
    """Butterfly sum over the last axis (64 lanes): partner distances 1, 2, .., 32 (the DPP / permlane tree of
    wave_sum2_dpp) or 32, 16, .., 1 (the __shfl_xor loop of wave_sum_f32)."""
    while v.shape[-1] > 1:
        n = v.shape[-1]
        v = v[..., 0::2] + v[..., 1::2] if ascending else v[..., : n // 2] + v[..., n // 2:]
    return v[..., 0]


def _lanes(x: torch.Tensor, x_dtype, C: int, slot_hi: bool):
    """adaln_mfma_kernel's register layout: [R, regs, 64 lanes, elements per register], zeros beyond the row; and `live`."""
    R = x.shape[0]
    m = maxc(C)
    per = 8 if x_dtype == torch.float16 else 4
    regs = m if x_dtype == torch.float16 else 2 * m
    pad = torch.zeros(R, regs * 64 * per, dtype=torch.float32)
    live = torch.zeros(regs * 64 * per, dtype=torch.bool)
    pad[:, :C] = x.float()
    live[:C] = True
    v = pad.view(R, regs, 64, per)
    live = live.view(regs, 64, per)
    if slot_hi and m == 5 and x_dtype == torch.float16:      # the slot chunk (vectors 256 ..) sits on lanes 32 .. 63
        v = v.clone()
        v[:, 4] = torch.roll(v[:, 4], 32, dims=1)
        live = live.clone()
        live[4] = torch.roll(live[4], 32, dims=0)
    return v, live


def _stats_mfma(x, x_dtype, C, order, mutation, inv_c, L):
    """mean, var [R] of adaln_mfma_kernel in fp32."""
    R = x.shape[0]
    if order == "pair2" and not (C == 1024 and x_dtype == torch.float16):
        order = "lane_tree"                                  # two rows per tile: fp16 rows of exactly 8 groups
    r = torch.arange(R)
    partner = r - r % L + ((r % L) ^ 1)
    partner = torch.where((partner % L < L) & (partner // L == r // L) & (partner < R), partner, r)
    v, live = _lanes(x, x_dtype, C, order == "slot_hi")
    regs, per = v.shape[1], v.shape[3]
    a1 = torch.zeros(R, regs, 64)
    a2 = torch.zeros(R, regs, 64)
    for k in range(per):                                     # v_dot2 (fp16 rows; squares of fp16 values are exact in fp32) / add, fma
        a1 = a1 + v[..., k]
        a2 = _fma(v[..., k], v[..., k], a2)
    s1, s2 = a1[:, 0], a2[:, 0]
    for c in range(1, regs):
        s1 = s1 + a1[:, c]
        s2 = s2 + a2[:, c]
    mean = _tree(s1, True) * inv_c
    var = _fma(-mean, mean, _tree(s2, True) * inv_c)
    T = switch_point(x_dtype)
    centre = ~(mean * mean < T * var)
    if order == "pair2":                                     # either row of a pair (rows 2j, 2j + 1 of a batch entry): both centred
        centre = centre | centre[partner]
    if mutation == "one_pass_always":
        centre = torch.zeros_like(centre)
    mu = mean.view(R, 1, 1)
    if order == "pair2":                                     # one accumulator: k outer, chunks inner, low half then high half
        ca = torch.zeros(R, 64)
        for k in range(0, per, 2):
            for c in range(regs):
                d0, d1 = v[:, c, :, k] - mu[:, 0], v[:, c, :, k + 1] - mu[:, 0]
                ca = _fma(d1, d1, _fma(d0, d0, ca))
        s2c = ca
    else:
        a2 = torch.zeros(R, regs, 64)
        for k in range(per):
            d0 = v[..., k] - mu
            a2 = _fma(d0, d0, a2)
        a2 = a2 * live[:, :, 0].float()                      # the zero padding is not part of the row (whole registers)
        s2c = a2[:, 0]
        for c in range(1, regs):
            s2c = s2c + a2[:, c]
    var_c = _tree(s2c, True) * inv_c
    return mean, torch.where(centre, var_c, var)


def _stats_wide(x, C, mutation, inv_c):
    """mean, var [R] of adaln_rotate_quant16_kernel: 256 lanes x 2 vectors of 8, always centred."""
    R = x.shape[0]
    pad = torch.zeros(R, 4096, dtype=torch.float32)
    pad[:, :C] = x.float()
    live = (torch.arange(4096) < C).view(2, 256, 8)
    v = pad.view(R, 2, 256, 8)

    def row_sum(lane_vals):                                   # [R, 256] -> [R]
        w = _tree(lane_vals.view(R, 4, 64), False)
        return ((w[:, 0] + w[:, 1]) + w[:, 2]) + w[:, 3]
    s1 = torch.zeros(R, 256)
    for c in range(2):
        for i in range(8):
            s1 = s1 + v[:, c, :, i]
    mean = row_sum(s1) * inv_c
    mu = mean.view(R, 1)
    s2 = torch.zeros(R, 256)
    if mutation == "one_pass_always":
        for c in range(2):
            for i in range(8):
                s2 = _fma(v[:, c, :, i], v[:, c, :, i], s2)
        return mean, _fma(-mean, mean, row_sum(s2) * inv_c)
    for c in range(2):
        lv = live[c, :, 0]
        p = torch.zeros(R, 256)
        for i in range(8):
            d = v[:, c, :, i] - mu
            if mutation == "pad_subtract":                    # the kernel as it was: one accumulator, padding included
                s2 = _fma(d, d, s2)
            else:
                p = _fma(d, d, p)
        if mutation == "pad_subtract":                        # padding lanes: take their (0 - mean)^2 back out
            s2 = torch.where(lv, s2, s2 - 8.0 * mu * mu)
        else:
            s2 = torch.where(lv, s2 + p, s2)                  # one partial sum per vector; the padding never enters
    return mean, row_sum(s2) * inv_c


def emulate(x: torch.Tensor, scale: torch.Tensor, shift: torch.Tensor, smooth: Optional[torch.Tensor], eps: float, L: int,
            order: str = "lane_tree", mutation: Optional[str] = None) -> torch.Tensor:
    """h (fp16 [R, C]) as the kernel for this width computes it, in fp32 on the CPU, in source order.
    order: "lane_tree" - lane-sequential accumulators + the wavefront tree (every form's first row);
           "slot_hi"   - rows of 17 .. 20 groups on fp16 rows with the slot chunk on lanes 32 .. 63 (second row of a pair);
           "pair2"     - C = 1024: the centred pass with a single accumulator, run when either row of a pair needs it.
    Rows wider than 2560 run the wide kernel whatever the order."""
    assert order in ORDERS and (mutation is None or mutation in MUTATIONS)
    R, C = x.shape
    x_dtype = x.dtype
    wide = C > WIDE_FROM
    n_pad = 4096 if wide else maxc(C) * 512
    inv_c = torch.tensor(1.0 / (n_pad if mutation == "mean_over_padded" else C), dtype=torch.float32)
    mean, var = _stats_wide(x, C, mutation, inv_c) if wide else _stats_mfma(x, x_dtype, C, order, mutation, inv_c, L)
    if mutation == "var_unbiased":
        var = var * torch.tensor(C / (C - 1.0), dtype=torch.float32)
    if mutation == "second_row_takes_first_rows_stats":
        r = torch.arange(R)
        src = torch.where((r % L) % 2 == 1, r - 1, r)
        mean, var = mean[src], var[src]
    ve = var if mutation == "eps_ignored" else var + torch.tensor(eps, dtype=torch.float32)
    if wide:
        rstd = 1.0 / torch.sqrt(ve)
    else:
        rstd = (1.0 / torch.sqrt(ve.double())).float()                                   # v_rsq_f32, then one Newton step
        rstd = _fma(rstd * _fma(-ve * rstd, rstd, torch.ones_like(rstd)), torch.tensor(0.5), rstd)
    r = torch.arange(R)
    b = (r + 1) // L if mutation == "batch_off_by_one" else r // L
    b = b.clamp_max(scale.shape[0] - 1)
    if scale.dtype == torch.float16 and mutation != "scale_plus_one_fp32":
        sc1 = (scale + 1).float()                                                        # pk_add_f16
    else:
        sc1 = scale.float() + 1.0
    sh = shift.float()
    sm = smooth.float() if smooth is not None else None
    late = mutation == "smooth_after_round"
    xf = x.float()
    mean, rstd = mean.view(R, 1), rstd.view(R, 1)
    if wide:
        t = ((xf - mean) * rstd) * sc1[b] + sh[b]
        if sm is not None and not late:
            t = t * sm
    else:
        A = sc1 * sm if sm is not None and not late else sc1
        Bm = sh * sm if sm is not None and not late else sh
        nm = -mean * rstd
        t = _fma(_fma(xf, rstd, nm), A[b], Bm[b])
    h = t.half()
    if sm is not None and late:
        h = (h.float() * sm).half()
    return h


# ---------------------------------------------------------------------------------------------------------------- inputs
def _row(fam: str, C: int, x_dtype, eps: float, g: torch.Generator) -> torch.Tensor:
    z = torch.randn(C, generator=g, dtype=torch.float64)
    z = (z - z.mean()) / z.std(unbiased=False)                # mean 0, variance 1 exactly (before the cast)
    T16 = x_dtype == torch.float16
    if fam == "gauss":
        return 1.3 * z + 0.2
    if fam == "lognormal":
        v = z * torch.exp(0.4 * torch.randn(C, generator=g, dtype=torch.float64))
        v[torch.randperm(C, generator=g)[:3]] *= 100.0
        return v
    if fam.startswith("rho2_"):
        return z + math.sqrt(float(fam[5:]))
    if fam == "rho_30":
        return z + 30.0
    if fam == "rho_high":                                     # fp16: 64 + 0.25 z, exact in fp16 up to the grid of 2^-4; fp32: rho 1000
        return 64.0 + 0.25 * z if T16 else 1000.0 + z
    if fam == "constant":
        return torch.full((C,), 3.0, dtype=torch.float64)
    if fam == "var_eps":
        return math.sqrt(eps) * z
    if fam == "mag_1e4":
        return (1.0e4 * z).clamp(-6.0e4, 6.0e4)
    v = 1.3 * z + 0.2
    v[C // 3] = math.inf if fam == "inf" else math.nan
    return v


def family_of(r: int, C: int, fams=FAMILIES) -> str:
    """Family of row r: the list in turn, started at an offset that moves with the width (launches of 4 rows then cover every
    family across the widths)."""
    return fams[(r + 5 * (C // 128)) % len(fams)]


def families(R: int, C: int, fams=FAMILIES):
    return [family_of(r, C, fams) for r in range(R)]


@functools.lru_cache(maxsize=None)
def make_rows(R: int, C: int, x_dtype, eps: float, seed: int = 0, fams=FAMILIES) -> torch.Tensor:
    g = torch.Generator().manual_seed(seed * 100003 + C * 7 + (1 if x_dtype == torch.float16 else 2))
    return torch.stack([_row(family_of(r, C, fams), C, x_dtype, eps, g) for r in range(R)]).to(x_dtype)


def make_case(B: int, L: int, C: int, x_dtype, mod_dtype, with_smooth: bool, eps: float, seed: int = 0, fams=FAMILIES):
    """(x [B L, C], scale [B, C], shift [B, C], smooth [C] or None) on the CPU; treat them as read-only (the rows are cached).
    |scale + 1| <= ~2.2, |shift| <= ~1.2, s in [0.25, 1.75], |LN| <= sqrt(C) <= 64: |h| < 6e4 on every finite row."""
    x = make_rows(B * L, C, x_dtype, eps, seed, fams)
    g = torch.Generator().manual_seed(seed * 7919 + C + 13)
    scale = (torch.randn(B, C, generator=g) * 0.3).to(mod_dtype)
    shift = (torch.randn(B, C, generator=g) * 0.3).to(mod_dtype)
    smooth = torch.rand(C, generator=g) * 1.5 + 0.25 if with_smooth else None
    return x, scale, shift, smooth


def quantized_groups(h: torch.Tensor) -> torch.Tensor:
    """What the stages behind h give for an fp16 h [R, C], on the CPU: the rotation by the block Hadamard matrix (accumulated in
    float64, rounded once to fp16) and the oracle's E2M1 per-group(128) quantizer.  Only to COUNT the groups in which two h
    differ far enough to change the result; the kernels' own stages are tested bit for bit elsewhere."""
    from oracle import fpq_oracle as orc
    R, C = h.shape
    y = orc.rotate_fp16_reference(h.reshape(-1, 128), orc.hadamard_block(128, 42).half()).view(R, C)
    return orc.per_group_kernel_sem(y, "e2m1", 128)


def check(h: torch.Tensor, ref, x_dtype, C: int):
    """(worst err / bound over the elements of the finite rows, whether h is non-finite exactly where the reference is)."""
    hd = h.double()
    fin = ref["finite"]
    ratio = ((hd - ref["h"]).abs() / bound(ref, x_dtype, C))[fin]
    worst = float(torch.nan_to_num(ratio, nan=math.inf).max()) if ratio.numel() else 0.0
    return worst, bool(torch.equal(torch.isfinite(hd), torch.isfinite(ref["h"])))
