"""What fpq_attention_blhc (fpqvar_amd/csrc/fpq_attention.h) must compute, and how close it has to come.

Shared by tests/test_attention_model_host.py (CPU: the bound is sound for the kernel's arithmetic and sharp enough to
catch each of a list of plausible kernel mistakes) and tests/test_gpu_attention.py (the kernel itself against it).

- reference(q, k, v, scale): softmax(scale q k^T) v in float64 from the fp16 inputs, with the quantities the error
  bound needs, on the inputs' device, one batch entry at a time.
- bound(r): the per-element error bound, derived in its docstring.
- emulate(q, k, v, scale, mutation): an fp32 model of the kernel's tile loop, optionally with one deliberate mistake.
- FAMILIES / make_case / shape_sweep: the input families and shapes both test files run, the host at small sizes.
"""
import math
from typing import Callable, Dict, List, NamedTuple, Optional, Tuple

import torch

LOG2E = 1.0 / math.log(2.0)
TILE = 64                                              # keys per staged tile (kAttnKv)
MAX_SCALE_MUL = math.log(100.0)                        # kv_cache.MAX_SCALE_MUL, the clamp of attn_l2_norm's scale_mul
MUTATIONS = ("drop_last", "dup_last", "no_rescale", "half_l", "q_prescale", "p_bf16")


class Ref(NamedTuple):
    out: torch.Tensor       # softmax(s) v                    [B, Lq, H, 64] float64
    A: torch.Tensor         # softmax(s) |v|                  [B, Lq, H, 64]
    Z: torch.Tensor         # sum_j exp(s_j - max s)  (>= 1)  [B, Lq, H, 1]
    vabs: torch.Tensor      # sum_j |v_jc|                    [B, 1, H, 64]


def reference(q: torch.Tensor, k: torch.Tensor, v: torch.Tensor, scale: float) -> Ref:
    """q [B, Lq, H, 64], k / v [B, Lkv, H, 64] fp16 (any strides) -> Ref in float64 on q's device.  The scores
    s = scale q k^T come from the fp16 values exactly (their products are exact in float64, the 64-term sums lose at most
    2^-47 relative); nothing is rounded to fp16 or fp32."""
    B, Lq, H, _ = q.shape
    outs, As, Zs = [], [], []
    for b in range(B):                                  # a [H, Lq, Lkv] float64 score block per batch entry
        qb, kb, vb = (t[b].double().transpose(0, 1) for t in (q, k, v))     # [H, L, 64]
        s = torch.matmul(qb, kb.transpose(1, 2)).mul_(scale)
        s.sub_(s.amax(dim=-1, keepdim=True)).exp_()
        Z = s.sum(dim=-1, keepdim=True)
        s.div_(Z)
        outs.append(torch.matmul(s, vb).transpose(0, 1))
        As.append(torch.matmul(s, vb.abs()).transpose(0, 1))
        Zs.append(Z.transpose(0, 1))
        del s
    vabs = v.double().abs().sum(dim=1, keepdim=True)
    return Ref(torch.stack(outs), torch.stack(As), torch.stack(Zs), vabs)


def bound(r: Ref) -> torch.Tensor:
    """Per-element bound on |out - r.out| for fpq_attention_blhc:

        (2^-11 + 2^-13) (|ref| + A)  +  2^-25 sum_j |v_jc| / Z  +  2^-25

    ref = softmax(s) v and A = softmax(s) |v| (float64, s = scale q k^T exactly); Z = sum_j exp(s_j - max s) >= 1 (the
    maximum's own term is 1).  u = 2^-11 is the unit roundoff of fp16 (10 fraction bits: half an ulp is 2^-11 of a value
    just above a power of two).  The kernel computes, per query row, p_j = exp2(s_j c - m c) in fp32 (c = scale log2 e,
    m the running maximum), l = sum of the fp32 p_j, o = sum of fp16(p_j) v_j, and out = fp16(o / l).  Write the fp32
    p_j as p_j (1 + e_j) and fp16(p_j) as p_j (1 + e_j)(1 + d_j).  Then before the last rounding

        o / l - ref = sum_j p_j [e_j (v_j - ref) + d_j (1 + e_j) v_j] / sum_j p_j (1 + e_j),

    so |o / l - ref| <= max|d| A + max|e| (|ref| + A) to first order.  Term by term:

    - 2^-11 |ref|: the final fp16 rounding of out (relative u for normal results).
    - 2^-11 A: P rounded to fp16 for the P V product while l sums the unrounded fp32 p: |d_j| <= u.
    - 2^-13 (|ref| + A): every fp32 error, |e_j| <= 2^-13 whenever |scale q.k| <= 100 (the l2-norm regime's clamp
      of scale_mul; every family below stays inside it).  Per key, in log2 units: the score, four chained MFMAs of
      exact fp16 products whose partial sums are at most |q||k| (Cauchy-Schwarz), 4 * 2^-24 * 100 * log2 e = 2^-14.9;
      c rounded to fp32, 2^-24 |s - m| c <= 2^-15.8; m c and the fma's result rounded, 2^-16.8 + 2^-15.8; v_exp_f32,
      2^-23; the chain of alpha = exp2((m_old - m_new) c) rescales, 2^-23 (m_final - m_first) c + 2^-23 per rescale,
      2^-14.7 over 35 tiles; in all 2^-13.1 log2 = 2^-13.6 relative.  The fp32 sums of o (products exact; at most a
      few roundings per 16-key MFMA over 35 tiles) and of l each add under 2^-16 relative, and the second-order terms
      (the output rounding of the first-order error, 1 / (1 - e)) under 2^-20.
    - 2^-25 sum_j |v_jc| / Z: a p below 2^-14 becomes an fp16 subnormal, absolute error <= 2^-25 instead of u p, in
      units of the row's running maximum at its tile; later rescales only shrink it, and the kernel divides by
      l = Z (1 + O(2^-13)), so each key adds <= 2^-25 |v_jc| / Z.
    - 2^-25: an output below 2^-14 rounds to an fp16 subnormal, absolute error <= 2^-25 instead of u |out|.

    The first two terms together are the first-order worst case, reached only when every rounding errs by a full half
    ulp in the same direction.  Below 2^-14 the last two terms are the worst case of two roundings onto the same 2^-24
    grid, and an output there can come close to its bound.  There is no term for rounding the scores or Q to fp16: flash-attn, which the reference
    calls, does not do that, and neither does the kernel (emulate(..., "q_prescale") shows what it would cost)."""
    return (2.0 ** -11 + 2.0 ** -13) * (r.out.abs() + r.A) + 2.0 ** -25 * r.vabs / r.Z + 2.0 ** -25


def ratio(out: torch.Tensor, r: Ref, normal_only: bool = False) -> float:
    """max |out - ref| / bound over every element (normal_only: over the elements with |ref| >= 2^-14, the smallest normal
    fp16); inf when out holds a NaN or an infinity."""
    if not bool(torch.isfinite(out).all()):
        return math.inf
    rat = (out.to(r.out.device).double() - r.out).abs() / bound(r)
    if normal_only:
        rat = rat[r.out.abs() >= 2.0 ** -14]
    return float(rat.max()) if rat.numel() else 0.0


def emulate(q: torch.Tensor, k: torch.Tensor, v: torch.Tensor, scale: float, mutation: Optional[str] = None) -> torch.Tensor:
    """fp32 model of attn_fwd64_kernel's arithmetic on the CPU -> fp16 [B, Lq, H, 64].  Per (batch, head, query row) and
    64-key tile t: s = q.k in fp32 (keys past lkv at -inf), m_new = max(m, tile max), alpha = exp2((m - m_new) c),
    p = exp2(fma(s, c, -m_new c)) with c = fp32(scale log2 e), l_half = l_half alpha + (sum of the half's fp32 p),
    o = o alpha + fp16(p) v (fp32 accumulation); out = fp16(o * (1 / (l_lo + l_hi))).  A lane holds the keys with
    key mod 8 in 0..3 (lanes 0-31) or 4..7 (lanes 32-63) and writes the output channels with (c >> 2) & 1 equal to its
    half.  `mutation` makes one mistake a rebuild of the kernel could make:
      drop_last   the last real key is masked too (an off-by-one in the mask)
      dup_last    one padding key is counted: it holds key lkv - 1 again (the loads clamp to the last key)
      no_rescale  o is not multiplied by alpha when the maximum rises
      half_l      each lane divides by its own half's l (the exchange with lane l ^ 32 is missing)
      q_prescale  q scale log2 e is rounded to fp16 and the scores come from it (c = 1)
      p_bf16      P is rounded to bf16 instead of fp16"""
    assert mutation is None or mutation in MUTATIONS, mutation
    B, Lq, H, D = q.shape
    Lkv = k.shape[1]
    c32 = torch.tensor(scale * LOG2E, dtype=torch.float32)
    qf = q.float().permute(0, 2, 1, 3)                                     # [B, H, Lq, 64]
    kf, vf = (t.float().permute(0, 2, 1, 3) for t in (k, v))              # [B, H, Lkv, 64]
    if mutation == "q_prescale":
        qf = (qf * c32).half().float()
        c32 = torch.tensor(1.0, dtype=torch.float32)
    c64 = float(c32)
    m = torch.full((B, H, Lq, 1), -math.inf)
    l_half = torch.zeros(2, B, H, Lq, 1)
    o = torch.zeros(B, H, Lq, D)
    n_tiles = (Lkv + TILE - 1) // TILE
    for t in range(n_tiles):
        idx = torch.arange(t * TILE, (t + 1) * TILE)
        last = Lkv - 1 if mutation != "dup_last" else Lkv
        kt, vt = kf[:, :, idx.clamp(max=Lkv - 1)], vf[:, :, idx.clamp(max=Lkv - 1)]
        s = torch.matmul(qf, kt.transpose(2, 3))                         # [B, H, Lq, 64] fp32
        live = idx <= last if mutation != "drop_last" else idx < Lkv - 1
        s = s.masked_fill(~live, -math.inf)
        m_new = torch.maximum(m, s.amax(dim=-1, keepdim=True))
        alpha = torch.exp2(((m - m_new) * c32).float())
        mc = (m_new * c32).float()
        p = torch.exp2((s.double() * c64 - mc.double()).float())         # one rounding: the fma
        m = m_new
        hi = (idx % 8) >= 4
        psum = torch.stack((p[..., ~hi].sum(dim=-1, keepdim=True), p[..., hi].sum(dim=-1, keepdim=True)))
        l_half = l_half * alpha + psum
        p16 = (p.bfloat16() if mutation == "p_bf16" else p.half()).float()
        if mutation != "no_rescale":
            o = o * alpha
        o = o + torch.matmul(p16, vt)
    if mutation == "half_l":
        chan_hi = (torch.arange(D) >> 2) & 1
        l = torch.where(chan_hi.bool(), l_half[1], l_half[0])           # [B, H, Lq, 64]
    else:
        l = l_half[0] + l_half[1]
    out = (o * (1.0 / l)).half()
    return out.permute(0, 2, 1, 3).contiguous()


# ---------------------------------------------------------------------------------------------------------- the cases
def _randn(shape, g, std=1.0):
    return torch.randn(*shape, generator=g) * std


def _unit(x):
    return torch.nn.functional.normalize(x, dim=-1)


def l2_scale_mul(H: int, g) -> torch.Tensor:
    """attn_l2_norm's per-head multiplier of q as var_block.GenerationBatch draws it: exp(min(log 4 + 0.3 N, log 100)),
    head 0 at the clamp (100)."""
    sm = math.log(4.0) + 0.3 * torch.randn(H, generator=g)
    sm[0] = MAX_SCALE_MUL + 0.5
    return sm.clamp_max(MAX_SCALE_MUL).exp()


E2M3 = torch.tensor([i / 8 for i in range(8)] + [1 + i / 8 for i in range(8)] + [2 + i / 4 for i in range(8)]
                    + [4 + i / 2 for i in range(8)])                    # the positive e2m3 values, 0 .. 7.5


def _qk_l2(B, H, Lq, Lkv, g):
    q = _unit(_randn((B, Lq, H, 64), g)) * l2_scale_mul(H, g).view(1, 1, H, 1)
    return q, _unit(_randn((B, Lkv, H, 64), g)), 1.0


def _qk_plain(B, H, Lq, Lkv, g):      # std(s) = 0.125 * 8 * 2.7^2 = 7.3: logits out to about +-30, scale |q||k| ~ 60
    return _randn((B, Lq, H, 64), g, 2.7), _randn((B, Lkv, H, 64), g, 2.7), 0.125


def _qk_uniform(B, H, Lq, Lkv, g):
    return _randn((B, Lq, H, 64), g), _randn((B, Lkv, H, 64), g), 1e-3


def _planted(where):
    """scale 0.125, channel 0 of q at 8 and of the planted key(s) at 8: those logits are ~8 against N(0, 1) for the rest."""
    def gen(B, H, Lq, Lkv, g):
        q, k = _randn((B, Lq, H, 64), g), _randn((B, Lkv, H, 64), g)
        q[..., 0] = 8.0
        k[..., 0] = 0.0
        n_full = Lkv // TILE
        if where == "tile0":
            keys = [min(5, Lkv - 1)]
        elif where == "last_full":
            keys = [(n_full - 1) * TILE + 37 if n_full else Lkv - 1]
        elif where == "last_key":
            keys = [Lkv - 1]
        elif where in ("sub0", "sub1"):          # a key in the same 32-key sub-tile of every tile
            off = 11 if where == "sub0" else 32 + 11
            keys = [j for j in range(off, Lkv, TILE)] or [Lkv - 1]
        elif where in ("half0", "half1"):        # keys in one lane half only (key mod 8 in 0..3 or in 4..7)
            keys = [j for j in range(Lkv) if ((j % 8) >= 4) == (where == "half1") and j % 29 == 3] or [Lkv - 1]
        elif where in ("rising", "falling"):     # the maximum moves in every tile
            t = torch.arange(Lkv) // TILE
            n = (Lkv + TILE - 1) // TILE
            k[..., 0] = (1.5 * (t if where == "rising" else n - 1 - t)).view(1, Lkv, 1).float()
            return q, k, 0.125
        else:
            raise ValueError(where)
        k[:, keys, :, 0] = 8.0
        return q, k, 0.125
    return gen


def _qk_equal(B, H, Lq, Lkv, g):      # every key the same row: every logit of a query row equal
    return _randn((B, Lq, H, 64), g), _randn((B, 1, H, 64), g).expand(B, Lkv, H, 64).clone(), 0.125


def _qk_e2m3(B, H, Lq, Lkv, g):
    """q and k on the e2m3 grid, keys drawn from 8 distinct rows: exact fp32 scores with exact ties (scale 1/16)."""
    def grid(shape):
        return E2M3[torch.randint(0, 32, shape, generator=g)] * torch.where(torch.rand(*shape, generator=g) < 0.5, -1.0, 1.0)
    rows = grid((B, 8, H, 64)) * 0.25
    pick = torch.randint(0, 8, (Lkv,), generator=g)
    return grid((B, Lq, H, 64)) * 0.25, rows[:, pick], 1.0 / 16


def _v_randn(B, H, Lkv, g):
    return _randn((B, Lkv, H, 64), g)


def _v_indicator(B, H, Lkv, g):     # v_j = e_{j mod 64}: output channel c is the probability mass of the keys j = c mod 64
    v = torch.zeros(B, Lkv, H, 64)
    v[:, torch.arange(Lkv), :, torch.arange(Lkv) % 64] = 1.0
    return v


def _v_const(B, H, Lkv, g):         # one row for every key: the output is that row
    return _randn((B, 1, H, 64), g).expand(B, Lkv, H, 64).clone()


def _v_large(B, H, Lkv, g):         # |v| up to 2^14
    return (_randn((B, Lkv, H, 64), g) * 2 ** 12).clamp(-2 ** 14, 2 ** 14)


def _v_zeros(B, H, Lkv, g):         # exact zeros: half the elements, channels 0..7 entirely
    v = _randn((B, Lkv, H, 64), g)
    v[torch.rand(B, Lkv, H, 64, generator=g) < 0.5] = 0.0
    v[..., :8] = 0.0
    return v


QK: Dict[str, Callable] = {
    "l2norm": _qk_l2, "plain": _qk_plain, "uniform": _qk_uniform, "equal": _qk_equal, "e2m3_ties": _qk_e2m3,
    **{"plant_" + w: _planted(w) for w in ("tile0", "last_full", "last_key", "sub0", "sub1", "half0", "half1",
                                           "rising", "falling")},
}
V: Dict[str, Callable] = {"randn": _v_randn, "indicator": _v_indicator, "const": _v_const, "large": _v_large, "zeros": _v_zeros}

# family name -> (q/k regime, V pattern)
FAMILIES: Dict[str, Tuple[str, str]] = {
    **{name: (name, "randn") for name in QK},
    "l2norm_indicator": ("l2norm", "indicator"),
    "uniform_indicator": ("uniform", "indicator"),
    "plant_last_key_indicator": ("plant_last_key", "indicator"),
    "plant_rising_indicator": ("plant_rising", "indicator"),
    "l2norm_const": ("l2norm", "const"),
    "plain_large": ("plain", "large"),
    "l2norm_large": ("l2norm", "large"),
    "plain_zeros": ("plain", "zeros"),
    "equal_indicator": ("equal", "indicator"),
}


def make_case(family: str, B: int, H: int, Lq: int, Lkv: int, seed: int = 0):
    """-> (q, k, v, scale): fp16 [B, Lq, H, 64] / [B, Lkv, H, 64] on the CPU."""
    qk, vp = FAMILIES[family]
    g = torch.Generator().manual_seed(seed * 1_000_003 + Lq * 7919 + Lkv * 31 + B * 17 + H)
    q, k, scale = QK[qk](B, H, Lq, Lkv, g)
    v = V[vp](B, H, Lkv, g)
    return q.half(), k.half(), v.half(), scale


LKV_SWEEP = (1, 2, 31, 32, 33, 63, 64, 65, 127, 128, 129, 191, 192, 193, 2239, 2240, 2241)
LQ_SWEEP = (1, 31, 32, 33, 63, 64, 65, 95, 96, 97, 127, 128, 129, 1024)
BH_SWEEP = ((1, 1), (1, 7), (2, 4), (3, 3), (1, 17))       # B * H = 1, 7, 8, 9, 17: the grid maps 8 (batch, head) pairs per group


def shape_sweep(lkv=LKV_SWEEP, lq=LQ_SWEEP, bh=BH_SWEEP, families=tuple(FAMILIES)) -> List[Tuple[str, int, int, int, int]]:
    """Pairwise covering of (Lkv, Lq, B*H): every (Lkv, Lq) pair once, with B*H = bh[(i + j) % len(bh)] - every Lkv and
    every Lq meets every B*H as long as both lists are at least len(bh) long - and the family rotating over `families`.
    -> [(family, B, H, Lq, Lkv)]."""
    out = []
    for i, nk in enumerate(lkv):
        for j, nq in enumerate(lq):
            B, H = bh[(i + j) % len(bh)]
            out.append((families[(i * len(lq) + j) % len(families)], B, H, nq, nk))
    return out


def model_calls(patch_nums, heads: int) -> List[Tuple[int, int, int]]:
    """(H, Lq, Lkv) of attention at every step of a model: Lq = pn^2, Lkv = the running sum."""
    calls, total = [], 0
    for pn in patch_nums:
        total += pn * pn
        calls.append((heads, pn * pn, total))
    return calls
