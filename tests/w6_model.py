"""What the W6 GEMM (fpqvar_amd/csrc/fpq_gemm_g6.h: E1M2 / E3M0 WEIGHTS as dense 6-bit codes against an E2M1, E1M2 or E3M0
activation, per-group(128) scales on both sides) must compute, in the terms of tests/gemm_model.py and tests/a6w4_model.py.

Shared by tests/test_w6_host.py (CPU) and tests/test_gpu_w6.py (the kernel).

- LEVELS: the three FP4 tables; PAIRS: the six (activation table, weight table) pairs the GEMM runs; SELECTOR: the MFMA's format
  selector of each table's operand form (E2M1 nibbles 4, E1M2 as FP6 E2M3 codes 2, E3M0 as BF6 E3M2 codes 3).
- decode_levels / encode_levels(table, ...): row-major codes <-> levels, nibbles for "e2m1", dense 6-bit rows otherwise.
- reference(a_table, w_table, ...): gm.Ref(kind="fp4", ...) - the per-group product in float64 with the magnitudes S and R of the
  FP4 bound, so gm.bound / gm.ratio / gm.class_mismatch serve unchanged.
- emulate(a_table, w_table, ..., mutation): the fp32 model of gemm_w6_kernel's steps (gemm_a6w4_kernel's: gm.emulate's "lds"
  order), optionally with one of gm.MUTATIONS.  Every product is a multiple of 1/16 up to 256, so a 128-term dot has at most 20
  significant bits: exact in the float64 product and in its fp32 rounding.
- make_case(a_table, w_table, family, T, O, K): gm.make_case("fp4", ...)'s families with BOTH sides' levels moved onto their
  tables (E2M1 magnitude index i -> the table's magnitude index i), codes built directly (no quantizer, no GPU), fp32 weight
  scales throughout (the kernels exist for those only); exact_dot_cases(a_table, w_table): K = 128, unit scales, dots that are
  fp16 numbers - the four constructions of a6w4_model.exact_dot_cases for a weight table.
"""
import functools
from typing import Optional

import torch

from tests import a6w4_model as am
from tests import gemm_model as gm

LEVELS = {"e2m1": gm.E2M1, **am.A_LEVELS}
A_TABLES = ("e2m1", "e1m2", "e3m0")
W_TABLES = ("e1m2", "e3m0")
PAIRS = tuple((a, w) for a in A_TABLES for w in W_TABLES)
SELECTOR = {"e2m1": 4, "e1m2": 2, "e3m0": 3}
SEG = {"e2m1": 64, "e1m2": 96, "e3m0": 96}         # bytes of codes per 128 elements
MUTATIONS = gm.MUTATIONS
# the FP4 families; "fp16_w_scales" keeps its name and its levels but carries fp32 weight scales here (see make_case)
FAMILIES = gm.KIND_FAMILIES["fp4"]


def decode_levels(table: str, codes: torch.Tensor) -> torch.Tensor:
    """row-major codes of `table` -> float64 levels [rows, K]"""
    return gm.decode("fp4", codes) if table == "e2m1" else am.decode_a(table, codes)


def encode_levels(table: str, levels: torch.Tensor) -> torch.Tensor:
    """levels of `table` (+-, exact) [rows, K] -> the row-major codes the GEMM reads, on the levels' device; a zero of either
    sign is code 0"""
    lv = torch.tensor(LEVELS[table], dtype=torch.float64, device=levels.device)
    mag = levels.abs().double().contiguous()
    i = torch.searchsorted(lv, mag)
    assert bool((lv[i.clamp(max=7)] == mag).all()), "not a level of the table"
    neg = (levels < 0) & (i > 0)
    if table == "e2m1":
        return gm.encode("fp4", torch.where(neg, i + 8, i))
    idx = am.level_codes(table).to(levels.device)[i]
    return gm.encode("fp6", torch.where(neg, idx + 32, idx))


def reference(a_table: str, w_table: str, a: torch.Tensor, a_scales: torch.Tensor, w: torch.Tensor, w_scales: torch.Tensor,
              bias: Optional[torch.Tensor]) -> gm.Ref:
    """am.reference with the weight decoded from w_table's 6-bit codes and the activation from a_table's codes: float64 on a's device"""
    La, Lw = decode_levels(a_table, a), decode_levels(w_table, w).to(a.device)
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


def emulate(a_table: str, w_table: str, a: torch.Tensor, a_scales: torch.Tensor, w: torch.Tensor, w_scales: torch.Tensor,
            bias: Optional[torch.Tensor], mutation: Optional[str] = None) -> torch.Tensor:
    """fp32 model of gemm_w6_kernel -> fp16 [T, O] on a's device: per group d = the exact dot, t = fl(d sa), acc = fma(t, sw, acc);
    y = fp16(fl(acc + b)).  `mutation`: one of gm.MUTATIONS, as am.emulate."""
    assert mutation is None or mutation in MUTATIONS, mutation
    La, Lw = decode_levels(a_table, a), decode_levels(w_table, w).to(a.device)
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


def _onto(table: str, L4: torch.Tensor) -> torch.Tensor:
    """E2M1 levels -> the table's levels of the same magnitude index and sign"""
    if table == "e2m1":
        return L4
    lv = torch.tensor(LEVELS[table], dtype=torch.float64, device=L4.device)
    e2m1 = torch.tensor(gm.E2M1, dtype=torch.float64, device=L4.device)
    return torch.where(L4 < 0, -1.0, 1.0) * lv[torch.searchsorted(e2m1, L4.abs().contiguous())]


@functools.lru_cache(maxsize=16)
def _base_case(family: str, T: int, O: int, K: int, seed: int) -> dict:
    """gm.make_case("fp4", ...) - built once per shape for the six pairs that move its levels onto their tables; never modified"""
    return gm.make_case("fp4", family, T, O, K, seed)


def make_case(a_table: str, w_table: str, family: str, T: int, O: int, K: int, seed: int = 0, device=None) -> dict:
    """gm.make_case("fp4", family, ...) with each side on its table: the E2M1 magnitude of index i becomes the table's magnitude of
    index i (signs, zeros and "the largest level" survive), each side's scales shrink by 6 / its table's largest level so that the
    magnitudes the families aim at stay where they were, "bias_cancel"'s bias is recomputed from the new levels, and the weight
    scales are fp32 in every family.  device: where the levels are moved and the codes built (the result lives there); default CPU."""
    assert family in FAMILIES, family
    c = {k: (v.to(device) if torch.is_tensor(v) and device is not None else v) for k, v in _base_case(family, T, O, K, seed).items()}
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


def exact_dot_cases(a_table: str, w_table: str) -> dict:
    """K = 128, unit scales, no bias: rows of activation levels and rows of weight levels whose exact dots are fp16 numbers, so the
    GEMM's output must equal the float64 product bit for bit if - and only if - the matrix core keeps every product of the 128.
    am.exact_dot_cases' four constructions with the weight levels of w_table.  -> {name: (La float64 [T, 128], Lw float64 [O, 128])};
    O is a multiple of 8."""
    top_a, small_a = LEVELS[a_table][-1], LEVELS[a_table][1]
    top_w, small_w = LEVELS[w_table][-1], LEVELS[w_table][1]
    cases = {}
    # (1) the largest products cancelling in pairs over 120 positions of every k-block, 1 .. 8 smallest ones left over at the
    # positions k % 16 == 15
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
    sl_a = [s * v for v in LEVELS[a_table] for s in (1, -1) if not (v == 0 and s < 0)]
    sl_w = [s * v for v in LEVELS[w_table] for s in (1, -1) if not (v == 0 and s < 0)]
    La = torch.tensor(sl_a, dtype=torch.float64).view(-1, 1).expand(len(sl_a), 128).clone()
    Lw = torch.zeros(16, 128, dtype=torch.float64)
    for o, v in enumerate(sl_w):
        Lw[o, (37 * o) % 128] = v
    cases["pairs_single"] = (La, Lw)
    # (3) the same pairs, each product 128 times (the dot is 128 x the product: at most 2^15, an fp16 number)
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
    Lw[:, 1::4] = top_w
    Lw[1::2, :] = -Lw[1::2, :]
    cases["one_large"] = (La, Lw)
    for name, (A, W) in cases.items():
        d = A @ W.t()
        assert bool((d == d.half().double()).all()), f"{a_table} x {w_table} {name}: a dot is not an fp16 number"
        assert W.shape[0] % 8 == 0
    return cases
