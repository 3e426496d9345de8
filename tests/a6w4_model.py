"""What the A6W4 GEMM (fpqvar_amd/csrc/fpq_gemm_g6.h: E1M2 / E3M0 activations as dense 6-bit codes against E2M1 weight nibbles,
per-group(128) scales on both sides) must compute, in the terms of tests/gemm_model.py.

Shared by tests/test_a6w4_host.py (CPU) and tests/test_gpu_a6w4.py (the kernel).

- A_LEVELS / A_CODE_FORMAT: the two activation tables and the 6-bit hardware format that holds each one's levels
  (E1M2 -> FP6 E2M3, E3M0 -> BF6 E3M2); code_values(fmt): the float64 value of all 64 codes of a format, from its definition.
- decode_a / encode_a: dense 6-bit rows <-> levels.
- reference(table, ...): gm.Ref(kind="fp4", ...) - the per-group product in float64 with the magnitudes S and R of the FP4
  bound, so gm.bound / gm.ratio / gm.class_mismatch serve unchanged (the contract is the FP4 one: the 128-term dot is exact).
- emulate(table, ..., mutation): the fp32 model of gemm_a6w4_kernel's steps (gm.emulate's "lds" order), optionally with one of
  gm.MUTATIONS.
- make_case(table, family, T, O, K): gm.make_case("fp4", ...)'s families with the activation levels moved onto the table
  (E2M1 magnitude index i -> the table's magnitude index i: zero stays zero, the largest level the largest), codes built
  directly (no quantizer, no GPU); exact_dot_cases(table): K = 128, unit scales, dots that are fp16 numbers.
"""
import math
from typing import Optional

import torch

from tests import gemm_model as gm

A_LEVELS = {"e1m2": (0.0, 0.25, 0.5, 0.75, 1.0, 1.25, 1.5, 1.75), "e3m0": (0.0, 0.25, 0.5, 1.0, 2.0, 4.0, 8.0, 16.0)}
A_CODE_FORMAT = {"e1m2": "e2m3", "e3m0": "e3m2"}
A_SELECTOR = {"e1m2": 2, "e3m0": 3}              # the MFMA's cbsz for the activation fragment
MAX_PRODUCT = {"e1m2": 10.5, "e3m0": 96.0}       # largest |level_a * level_w|
# gm.MUTATIONS that describe a mistake gemm_a6w4_kernel could make (all of the FP4 kernel's: it shares that kernel's steps)
MUTATIONS = gm.MUTATIONS
FAMILIES = gm.KIND_FAMILIES["fp4"]


def code_values(fmt: str, device=None) -> torch.Tensor:
    """float64 value of the 64 codes of a 6-bit format: bit 5 sign, then "e2m3": 2 exponent bits (bias 1), 3 mantissa bits;
    "e3m2": 3 exponent bits (bias 3), 2 mantissa bits."""
    v = []
    for c in range(64):
        if fmt == "e2m3":
            e, m = (c >> 3) & 3, c & 7
            mag = m / 8 if e == 0 else (1 + m / 8) * 2.0 ** (e - 1)
        else:
            e, m = (c >> 2) & 7, c & 3
            mag = m / 16 if e == 0 else (1 + m / 4) * 2.0 ** (e - 3)
        v.append(-mag if c & 32 else mag)
    return torch.tensor(v, dtype=torch.float64, device=device)


def level_codes(table: str) -> torch.Tensor:
    """the 6-bit code (sign bit clear) of each of the table's 8 magnitudes, in the table's hardware format"""
    vals = code_values(A_CODE_FORMAT[table])[:32]
    out = []
    for lv in A_LEVELS[table]:
        hit = (vals == lv).nonzero().view(-1)
        assert hit.numel() == 1, (table, lv)
        out.append(int(hit[0]))
    return torch.tensor(out, dtype=torch.long)


def decode_a(table: str, codes: torch.Tensor) -> torch.Tensor:
    """dense 6-bit rows [rows, 3K/4] (element j in bits 6j .. 6j + 5 of the row's little-endian bit string) -> float64 [rows, K]"""
    tab = code_values(A_CODE_FORMAT[table], codes.device)
    b = codes.long().reshape(codes.shape[0], -1, 3)
    word = b[..., 0] | (b[..., 1] << 8) | (b[..., 2] << 16)
    idx = torch.stack([(word >> (6 * j)) & 63 for j in range(4)], dim=-1).reshape(codes.shape[0], -1)
    return tab[idx]


def encode_a(table: str, levels: torch.Tensor) -> torch.Tensor:
    """levels of the table (+-, exact) [rows, K] -> dense 6-bit rows; a zero of either sign is code 0"""
    lv = torch.tensor(A_LEVELS[table], dtype=torch.float64)
    i = torch.searchsorted(lv, levels.abs().double().contiguous())
    assert bool((lv[i.clamp(max=7)] == levels.abs()).all()), "not a level of the table"
    idx = level_codes(table)[i]
    idx = torch.where((levels < 0) & (i > 0), idx + 32, idx)
    return gm.encode("fp6", idx)


def reference(table: str, a: torch.Tensor, a_scales: torch.Tensor, w: torch.Tensor, w_scales: torch.Tensor,
              bias: Optional[torch.Tensor]) -> gm.Ref:
    """gm.reference("fp4", ...) with the activation decoded from the table's 6-bit codes: float64 on a's device.  Every product
    (a multiple of 1/8 up to 96) and every 128-term dot (|d_g| <= 12288) is exact in float64."""
    La, Lw = decode_a(table, a), gm.decode("fp4", w).to(a.device)
    T, K = La.shape
    O = Lw.shape[0]
    sa, sw = a_scales.to(a.device).double(), w_scales.to(a.device).double()
    b = bias.to(a.device).double().view(1, O) if bias is not None else torch.zeros(1, O, dtype=torch.float64, device=a.device)
    outs, Ss, Rs = [], [], []
    tc = max(1, gm.CHUNK // max(O, 1))
    for t0 in range(0, T, tc):
        A = La[t0:t0 + tc]
        acc = torch.zeros(A.shape[0], O, dtype=torch.float64, device=a.device)
        S = torch.zeros_like(acc)
        R = torch.zeros_like(acc)
        for g in range(K // 128):
            ks = slice(g * 128, (g + 1) * 128)
            term = (sa[t0:t0 + tc, g].view(-1, 1) * sw[:, g].view(1, -1)) * (A[:, ks] @ Lw[:, ks].t())
            acc += term
            S += term.abs()
            R += acc.abs()
        outs.append(acc + b)
        Ss.append(S)
        Rs.append(R)
    return gm.Ref("fp4", torch.cat(outs), torch.cat(Ss), torch.cat(Rs), b.abs())


def emulate(table: str, a: torch.Tensor, a_scales: torch.Tensor, w: torch.Tensor, w_scales: torch.Tensor,
            bias: Optional[torch.Tensor], mutation: Optional[str] = None) -> torch.Tensor:
    """fp32 model of gemm_a6w4_kernel -> fp16 [T, O] on a's device: per group d = the exact dot (17 bits at most: exact in fp32),
    t = fl(d sa), acc = fma(t, sw, acc); y = fp16(fl(acc + b)).  `mutation`: one of gm.MUTATIONS, as gm.emulate("fp4", order "lds")."""
    assert mutation is None or mutation in MUTATIONS, mutation
    La, Lw = decode_a(table, a), gm.decode("fp4", w).to(a.device)
    T, K = La.shape
    O = Lw.shape[0]
    steps = K // 128
    sa32 = a_scales.to(a.device).float()
    sw32 = w_scales.to(a.device).float()
    if mutation == "w_scale_fp16":
        sw32 = sw32.half().float()
    b32 = bias.to(a.device).float().view(1, O) if bias is not None else torch.zeros(1, O, device=a.device)
    outs = []
    tc = max(1, gm.CHUNK // max(O, 1))
    for t0 in range(0, T, tc):
        A = La[t0:t0 + tc]
        acc = torch.zeros(A.shape[0], O, dtype=torch.float32, device=a.device)
        for g in range(steps):
            if mutation == "drop_last_k" and g == steps - 1:
                break
            ks = slice(g * 128, (g + 1) * 128)
            d32 = (A[:, ks] @ Lw[:, ks].t()).float()
            gs = steps - 2 if (mutation == "tail_group_scale" and g == steps - 1 and steps > 1) else g
            sa_g, sw_g = sa32[t0:t0 + tc, gs].view(-1, 1), sw32[:, gs].view(1, -1)
            if mutation == "scale_fp16":
                acc = gm.fma32(d32, (sa_g * sw_g).half().float(), acc)
            else:
                acc = gm.fma32(d32 * sa_g, sw_g.expand_as(acc), acc)
        if mutation == "bias_after_round":
            y = (acc.half().double() + b32.half().double()).half()
        else:
            y = gm._fp16_out(acc + b32, mutation)
        outs.append(y)
    return torch.cat(outs)


def make_case(table: str, family: str, T: int, O: int, K: int, seed: int = 0) -> dict:
    """gm.make_case("fp4", family, ...) with the activation on `table`: the E2M1 magnitude of index i becomes the table's
    magnitude of index i (signs, zeros and "the largest level" survive), the activation scales shrink by 6 / the table's largest
    level so that the magnitudes the families aim at (the fp16 edge of "overflow", the partial sums of "max_codes") stay where
    they were, and "bias_cancel"'s bias is recomputed from the new levels."""
    assert family in FAMILIES, family
    c = gm.make_case("fp4", family, T, O, K, seed)
    e2m1 = torch.tensor(gm.E2M1, dtype=torch.float64)
    lv = torch.tensor(A_LEVELS[table], dtype=torch.float64)
    La4 = gm.decode("fp4", c["a"])
    La = torch.where(La4 < 0, -1.0, 1.0) * lv[torch.searchsorted(e2m1, La4.abs().contiguous())]
    sa = (c["a_scales"].double() * (gm.E2M1[-1] / A_LEVELS[table][-1])).half()
    out = dict(c, a=encode_a(table, La), a_scales=sa)
    if family == "bias_cancel":
        G = K // 128
        Lw = gm.decode("fp4", c["w"])
        a0 = (La[:1].view(1, G, 128) * sa[:1].double().view(1, G, 1)).view(1, K)
        w0 = (Lw.view(O, G, 128) * c["w_scales"].double().view(O, G, 1)).view(O, K)
        out["bias"] = (-(a0 @ w0.t()).view(O).clamp(-60000, 60000)).half()
    return out


def exact_dot_cases(table: str) -> dict:
    """K = 128, unit scales, no bias: rows of activation levels and rows of weight levels whose exact dots are fp16 numbers, so the
    GEMM's output must equal the float64 product bit for bit if - and only if - the matrix core keeps every product of the 128.
    -> {name: (La float64 [T, 128], Lw float64 [O, 128])}; O is a multiple of 8."""
    top_a, small_a = A_LEVELS[table][-1], A_LEVELS[table][1]
    top_w, small_w = gm.E2M1[-1], gm.E2M1[1]
    cases = {}
    # (1) the largest products (+-96 resp. +-10.5) cancelling in pairs over 120 positions of every k-block, 1 .. 8 smallest ones
    # (+-1/8) left over at the positions k % 16 == 15
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
    # (2) every (activation level, weight level) pair of the 15 x 15 signed levels: row t of A is constant (signed level t), row o
    # of W holds signed level o at ONE position and zero elsewhere -> the dot is the single product
    sl_a = [s * v for v in A_LEVELS[table] for s in (1, -1) if not (v == 0 and s < 0)]
    sl_w = [s * v for v in gm.E2M1 for s in (1, -1) if not (v == 0 and s < 0)]
    La = torch.tensor(sl_a, dtype=torch.float64).view(-1, 1).expand(len(sl_a), 128).clone()
    Lw = torch.zeros(16, 128, dtype=torch.float64)
    for o, v in enumerate(sl_w):
        Lw[o, (37 * o) % 128] = v
    cases["pairs_single"] = (La, Lw)
    # (3) the same pairs, each product 128 times (the dot is 128 x the product: still at most 17 bits)
    Lw = torch.zeros(16, 128, dtype=torch.float64)
    for o, v in enumerate(sl_w):
        Lw[o, :] = v
    cases["pairs_x128"] = (La.clone(), Lw)
    # (4) the largest product beside 127 smallest ones, the large one at every k-block position
    T, O = 32, 8
    La = torch.full((T, 128), small_a, dtype=torch.float64)
    Lw = torch.full((O, 128), small_w, dtype=torch.float64)
    for t in range(T):
        La[t, (4 * t + 1) % 128] = top_a if t % 2 == 0 else -top_a
    Lw[:, :] = small_w
    # the weight is large everywhere an activation row may be large (positions 4t + 1), small elsewhere: the dot is
    # +-96 (10.5) + the small-small products + top_w * small_a at the other large-weight positions - all multiples of 1/8
    Lw[:, 1::4] = top_w
    Lw[1::2, :] = -Lw[1::2, :]
    cases["one_large"] = (La, Lw)
    for name, (A, W) in cases.items():
        d = A @ W.t()
        assert bool((d == d.half().double()).all()), f"{table} {name}: a dot is not an fp16 number"
        assert W.shape[0] % 8 == 0
    return cases
