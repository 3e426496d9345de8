"""What the per-group GEMMs must compute for FULL-RANGE FP6 operands (gemm.linear_g6: E2M3 / E3M2 codes with per-group(128) scales
on the A6W4 and W6 kernels, include/fpq.h "GF6"), in the terms of tests/gemm_model.py and tests/w6_model.py.

Shared by tests/test_gf6_host.py (CPU) and tests/test_gpu_gf6.py (the kernels).

- LEVELS: the five per-group tables; PAIRS: the sixteen (activation, weight) pairs with at least one full FP6 side; DECODE: the table
  whose selector id the C entry points take for an operand (E2M3 codes travel under E1M2's id, E3M2 codes under E3M0's); FAMILY: the
  kernel family a pair runs on ("a6w4": E2M1 weight nibbles; "w6": a 6-bit weight).
- product_range(a, w): (step, largest, bits) - every product of two levels is a multiple of `step` and at most `largest`, so the
  exact 128-term dot has at most `bits` significant bits; FITS_FP32[pair]: bits <= 24.
- decode_levels / encode_levels, reference, emulate: w6_model's, under the decode table's name (its code tables hold all 64 codes).
- make_case(a, w, family, T, O, K): gm.make_case("fp4", ...)'s families with each side's levels moved onto its table - for a full
  table zero stays zero, the largest level the largest, and the six levels between spread over ALL thirty levels between (by the
  element's position), so every code occurs.
- exact_dot_cases(a, w): w6_model.exact_dot_cases' four constructions for any pair: K = 128, unit scales, dots that are fp16
  numbers.  Where a construction of w6_model's would leave the fp16 grid, it is cut to fit and says how: "pairs_xN" repeats each
  product N = 128 times, or 64 where 128 x the largest product passes 65504 (E3M2 x E3M2); "one_large" takes for "smallest" the
  first pair of levels (ascending) for which the dot is an fp16 number.
"""
import functools
import math
from typing import Optional

import torch

from tests import a6w4_model as am
from tests import gemm_model as gm
from tests import w6_model as wm

E2M3 = tuple(float(v) for v in am.code_values("e2m3")[:32])
E3M2 = tuple(float(v) for v in am.code_values("e3m2")[:32])
LEVELS = {**wm.LEVELS, "e2m3": E2M3, "e3m2": E3M2}
FULL = ("e2m3", "e3m2")
TABLES = ("e2m1", "e1m2", "e3m0", "e2m3", "e3m2")
PAIRS = tuple((a, w) for a in TABLES for w in TABLES if a in FULL or w in FULL)
DECODE = {"e2m1": "e2m1", "e1m2": "e1m2", "e3m0": "e3m0", "e2m3": "e1m2", "e3m2": "e3m0"}
CODE_FORMAT = {"e1m2": "e2m3", "e3m0": "e3m2", "e2m3": "e2m3", "e3m2": "e3m2"}
SEG = {"e2m1": 64, "e1m2": 96, "e3m0": 96, "e2m3": 96, "e3m2": 96}
FAMILY = {p: ("a6w4" if p[1] == "e2m1" else "w6") for p in PAIRS}
MUTATIONS = gm.MUTATIONS
FAMILIES = wm.FAMILIES


def product_range(a_table: str, w_table: str):
    """(step, largest, bits): every product of a level of each table is a multiple of `step` (a power of two) and at most `largest`;
    a sum of 128 of them is an integer multiple of step below 128 * largest / step + 1, i.e. has at most `bits` significant bits"""
    la, lw = [v for v in LEVELS[a_table] if v], [v for v in LEVELS[w_table] if v]

    def grid(vals):   # the largest power of two every value is a multiple of
        e = 0
        while any((v * 2.0 ** -e) != int(v * 2.0 ** -e) for v in vals):
            e -= 1
        return 2.0 ** e
    step = grid(la) * grid(lw)
    largest = la[-1] * lw[-1]
    return step, largest, math.ceil(math.log2(128 * largest / step + 1))


FITS_FP32 = {p: product_range(*p)[2] <= 24 for p in PAIRS}


def decode_levels(table: str, codes: torch.Tensor) -> torch.Tensor:
    return wm.decode_levels(DECODE[table], codes)


def encode_levels(table: str, levels: torch.Tensor) -> torch.Tensor:
    """levels of `table` (+-, exact) [rows, K] -> the row-major codes the GEMM reads; a zero of either sign is code 0"""
    if table not in FULL:
        return wm.encode_levels(table, levels)
    lv = torch.tensor(LEVELS[table], dtype=torch.float64, device=levels.device)   # magnitude index == code (sign bit clear)
    mag = levels.abs().double().contiguous()
    i = torch.searchsorted(lv, mag)
    assert bool((lv[i.clamp(max=31)] == mag).all()), "not a level of the table"
    return gm.encode("fp6", torch.where((levels < 0) & (i > 0), i + 32, i))


def reference(a_table: str, w_table: str, a, a_scales, w, w_scales, bias) -> gm.Ref:
    return wm.reference(DECODE[a_table], DECODE[w_table], a, a_scales, w, w_scales, bias)


def emulate(a_table: str, w_table: str, a, a_scales, w, w_scales, bias, mutation: Optional[str] = None) -> torch.Tensor:
    """wm.emulate: per group d = the exact dot rounded to fp32 (exact where FITS_FP32), t = fl(d sa), acc = fma(t, sw, acc),
    y = fp16(fl(acc + b))"""
    return wm.emulate(DECODE[a_table], DECODE[w_table], a, a_scales, w, w_scales, bias, mutation)


def _onto(table: str, L4: torch.Tensor) -> torch.Tensor:
    """E2M1 levels -> the table's: wm._onto for the 8-level tables; for a full table index 0 -> 0, 7 -> 31 and index i in 1 .. 6 ->
    1 + 5 (i - 1) + (column % 5), so the thirty levels between all occur and the order of magnitudes survives"""
    if table not in FULL:
        return wm._onto(table, L4)
    lv = torch.tensor(LEVELS[table], dtype=torch.float64, device=L4.device)
    e2m1 = torch.tensor(gm.E2M1, dtype=torch.float64, device=L4.device)
    i = torch.searchsorted(e2m1, L4.abs().contiguous())
    col = torch.arange(L4.shape[1], device=L4.device).view(1, -1) % 5
    j = torch.where(i == 0, 0, torch.where(i == 7, 31, 1 + 5 * (i - 1) + col))
    return torch.where(L4 < 0, -1.0, 1.0) * lv[j]


def make_case(a_table: str, w_table: str, family: str, T: int, O: int, K: int, seed: int = 0, device=None) -> dict:
    """wm.make_case for any pair: fp32 weight scales throughout, each side's scales shrunk by 6 / its table's largest level,
    "bias_cancel"'s bias recomputed from the new levels"""
    assert family in FAMILIES, family
    c = {k: (v.to(device) if torch.is_tensor(v) and device is not None else v) for k, v in wm._base_case(family, T, O, K, seed).items()}
    La, Lw = _onto(a_table, gm.decode("fp4", c["a"])), _onto(w_table, gm.decode("fp4", c["w"]))
    sa = (c["a_scales"].double() * (gm.E2M1[-1] / LEVELS[a_table][-1])).half()
    sw = (c["w_scales"].double() * (gm.E2M1[-1] / LEVELS[w_table][-1])).float()
    out = dict(c, a=encode_levels(a_table, La), a_scales=sa, w=encode_levels(w_table, Lw), w_scales=sw)
    if family == "bias_cancel":
        G = K // 128
        a0 = (La[:1].view(1, G, 128) * sa[:1].double().view(1, G, 1)).view(1, K)
        w0 = (Lw.view(O, G, 128) * sw.double().view(O, G, 1)).view(O, K)
        out["bias"] = (-(a0 @ w0.t()).view(O).clamp(-60000, 60000)).half()
    return out


def _is_fp16(d: torch.Tensor) -> bool:
    return bool((d == d.half().double()).all())


@functools.lru_cache(maxsize=None)
def exact_dot_cases(a_table: str, w_table: str) -> dict:
    """-> {name: (La float64 [T, 128], Lw float64 [O, 128])}; O is a multiple of 8, every dot is an fp16 number (see the module's
    docstring for what differs from wm.exact_dot_cases: nothing for two 8-level tables)"""
    lv_a, lv_w = LEVELS[a_table], LEVELS[w_table]
    top_a, small_a, top_w, small_w = lv_a[-1], lv_a[1], lv_w[-1], lv_w[1]
    cases = {}
    # (1) the largest products cancelling in pairs over 120 positions, 1 .. 8 smallest ones left over at the positions k % 16 == 15
    T, O = 16, 16
    q_pos = torch.arange(15, 128, 16)
    rest = torch.tensor([k for k in range(128) if k % 16 != 15])
    La = torch.zeros(T, 128, dtype=torch.float64)
    Lw = torch.zeros(O, 128, dtype=torch.float64)
    for t in range(T):
        La[t, rest] = top_a * torch.where(torch.arange(120) % 2 == 0, 1.0, -1.0).double() * (1 if t % 4 < 2 else -1)
        La[t, q_pos[: 1 + t % 8]] = small_a * (1 if t % 2 == 0 else -1)
    for o in range(O):
        sg = 1 if o % 2 == 0 else -1
        Lw[o, rest] = top_w * sg
        Lw[o, q_pos] = small_w * (sg if o % 4 < 2 else -sg)
    cases["cancel"] = (La, Lw)
    # (2) every (activation level, weight level) pair of the signed levels alone
    sl_a = [s * v for v in lv_a for s in (1, -1) if not (v == 0 and s < 0)]
    sl_w = [s * v for v in lv_w for s in (1, -1) if not (v == 0 and s < 0)]
    n_w = (len(sl_w) + 7) // 8 * 8
    La = torch.tensor(sl_a, dtype=torch.float64).view(-1, 1).expand(len(sl_a), 128).clone()
    Lw = torch.zeros(n_w, 128, dtype=torch.float64)
    for o, v in enumerate(sl_w):
        Lw[o, (37 * o) % 128] = v
    cases["pairs_single"] = (La, Lw)
    # (3) the same pairs, each product N times: N = 128, or 64 where 128 x the largest product is past the fp16 range
    n = 128 if 128 * top_a * top_w <= 65504 else 64
    Lw = torch.zeros(n_w, 128, dtype=torch.float64)
    for o, v in enumerate(sl_w):
        Lw[o, :n] = v
    cases[f"pairs_x{n}"] = (La.clone(), Lw)
    # (4) the largest product beside 127 small ones, the large one at every k-block position; "small" = the first pair of levels,
    # ascending, that leaves every dot an fp16 number (the smallest levels themselves for two 8-level tables)
    T, O = 32, 8
    for s_a, s_w in ((x, y) for x in lv_a[1:] for y in lv_w[1:]):
        La = torch.full((T, 128), s_a, dtype=torch.float64)
        Lw = torch.full((O, 128), s_w, dtype=torch.float64)
        for t in range(T):
            La[t, (4 * t + 1) % 128] = top_a if t % 2 == 0 else -top_a
        Lw[:, 1::4] = top_w
        Lw[1::2, :] = -Lw[1::2, :]
        if _is_fp16(La @ Lw.t()):
            break
    else:
        raise AssertionError(f"{a_table} x {w_table}: no small pair leaves one_large on the fp16 grid")
    cases["one_large"] = (La, Lw)
    for name, (A, W) in cases.items():
        assert _is_fp16(A @ W.t()), f"{a_table} x {w_table} {name}: a dot is not an fp16 number"
        assert W.shape[0] % 8 == 0
    return cases
