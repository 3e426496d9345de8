"""What the squared-error forms of the matrix-core GEMMs (include/fpq.h, fpq_gemm_*_sqerr; the tail: fpqvar_amd/csrc/fpq_gemm_fp4.h,
FPQ_GEMM_SQERR_ROWS / _FINISH, and sqerr_finish_kernel of fpq_kernels.hip) must return and how close they have to come:
    loss = sum_t w[t] sum_o (f32(ref[t, o]) - f32(y16[t, o]))^2,      y16 = what the family's plain Linear stores.

Shared by tests/test_gemm_sqerr_model_host.py (CPU: the bound is sound for the kernel's order of operations and sharp enough to
catch each of a list of plausible kernel mistakes), tests/test_gpu_gemm_sqerr.py and tests/test_gpu_format_search_mc.py.

- reference(ref, y16, w): the loss in float64 from the stored inputs.
- tile_rows(family, tokens, outs, forced) / tiles(...): the tiling a launch runs and its number of tiles.
- chain(tile_rows, n_tiles) / bound(tokens, outs, tile_rows, ref_dtype, w_max): the longest chain of fp32 additions D and the
  other roundings c, read off the kernel, and the bound (relative part, absolute floor).
- emulate(ref, y, w, tile_rows, mistake): the kernel's operations in fp32 on the CPU in the kernel's order - tile by tile, lane by
  lane - optionally with one mistake.
- make_case(tokens, outs, ref_dtype, family): inputs for the CPU tests (y stands for the GEMM's fp32 accumulator + bias).
"""
import functools
import math
from typing import Optional, Tuple

import torch

U = 2.0 ** -24                      # unit roundoff of fp32
BLOCK = 256                         # lanes of the finishing workgroup
BN = 128                            # every tiling's tile is 128 outputs wide
C_ROUNDINGS = 3                     # the difference, the square, the weight
MISTAKES = ("rows_past_T_counted", "cols_past_O_counted", "clamped_row_weight", "y_not_rounded_to_fp16", "neighbour_weight",
            "diff_fp16", "partial_of_last_tile_dropped")
FAMILIES = ("fp4", "a6w4", "w6", "f6_rows")


def tile_rows(family: str, tokens: int, outs: int, forced: Optional[int] = None) -> int:
    """Rows of the tile a launch uses.  Per-group families (gemm_glds_tiling, fpq_gemm_launch.h; forced = FPQ_GEMM_CFG 10 / 20 / 30,
    40 runs 30's tile): 64 while the 128-row tiling has at most 384 tiles, 256 (fp4 only, K small enough for two tiles per CU:
    every K the tests use) from 4000 tiles of that size on, else 128.  Row-scaled family (forced = FPQ_GEMM6_CFG 0 / 1): 256 from
    4096 tokens on for outs >= 4096 and from 32768 on for any outs, else 128."""
    if family == "f6_rows":
        if forced is not None:
            return 256 if forced == 1 else 128
        return 256 if tokens >= 4096 and (outs >= 4096 or tokens >= 32768) else 128
    have_256 = family == "fp4"
    if forced in (20, 30, 40) or (forced == 10 and have_256):
        return {10: 256, 20: 128, 30: 64, 40: 64}[forced]
    col = (outs + BN - 1) // BN
    if ((tokens + 127) // 128) * col <= 384:
        return 64
    return 256 if have_256 and ((tokens + 255) // 256) * col >= 4000 else 128


def tiles(tokens: int, outs: int, bm: int) -> int:
    return ((tokens + bm - 1) // bm) * ((outs + BN - 1) // BN)


def workspace_bytes(tokens: int, outs: int) -> int:
    """fpq_gemm_sqerr_workspace_bytes: 4 bytes per tile of the smallest tiling (64 x 128), at least 4"""
    return 4 * max(1, tiles(tokens, outs, 64))


def chain(bm: int, n_tiles: int) -> Tuple[int, int]:
    """(D, c) from the kernel's source.  The fp32 additions one term passes through, in order:
      4        s += e e over the lane's four outputs of a row (the first adds to 0)
      4 MT     se_acc += select(w s) over the lane's rows, MT = tile rows / 32 (the first adds to 0)
      6        the wavefront's butterfly (lane ^ 32, 16, 8, 4, 2, 1)
      3        the workgroup's four wavefront sums, in order
      n_j      the finishing workgroup: lane i adds partials i, i + 256, ... : ceil(tiles / 256)
      6 + 3    its butterfly and its four wavefront sums
    D = 4 MT + n_j + 22.  c = 3: the roundings of e = r - y, of e e and of w s (no fused multiply-add: -ffp-contract=off)."""
    mt = bm // 32
    return 4 * mt + (n_tiles + BLOCK - 1) // BLOCK + 22, C_ROUNDINGS


def bound(tokens: int, outs: int, bm: int, ref_dtype, w_max: float = 1.0) -> Tuple[float, float]:
    """(rel, floor):  |got - S| <= rel * S + floor, S the float64 reference.
    Every term w e^2 is non-negative, so every partial sum is a sum of non-negative numbers: a rounding of relative size U anywhere
    moves the total by at most U times the part it acts on, and a term meets at most D + c of them: rel = (1 + U)^(D + c) - 1.
    fp16 ref: e is a difference of two fp16 numbers, the smallest non-zero |e| is 2^-24, e^2 >= 2^-48, and with w >= 2^-70 nothing
    goes subnormal: floor = 0, a zero loss must be met exactly.  fp32 ref: a square or a weighted row sum below 2^-126 is rounded
    with an absolute error of at most 2^-150; four squares per row of a lane pass through w: floor = (tokens outs max(w_max, 1) +
    tokens outs / 4) 2^-149, as tests/sqerr_model.py has it per element and per vector."""
    d, c = chain(bm, tiles(tokens, outs, bm))
    rel = (1.0 + U) ** (d + c) - 1.0
    floor = 0.0 if ref_dtype == torch.float16 else (tokens * outs * max(w_max, 1.0) + tokens * outs / 4) * 2.0 ** -149
    return rel, floor


def reference(ref: torch.Tensor, y16: torch.Tensor, w: torch.Tensor) -> float:
    """float64 from the stored inputs: sum_t w[t] sum_o (ref - y16)^2, the row sums first (a NaN / inf difference gives NaN / +inf,
    as in fp32: all weights are positive)"""
    assert y16.dtype == torch.float16
    if ref.numel() == 0:
        return 0.0
    return float((((ref.double() - y16.double()) ** 2).sum(dim=1) * w.double()).sum())


def expected_class(ref: torch.Tensor, y16: torch.Tensor) -> str:
    e = ref.float() - y16.float()
    return "nan" if bool(torch.isnan(e).any()) else "inf" if bool(torch.isinf(e).any()) else "finite"


def class_of(v: float) -> str:
    return "nan" if math.isnan(v) else "inf" if v == math.inf else "finite"


def ratio(got: float, ref64: float, rel: float, floor: float) -> float:
    """|got - ref64| / (rel ref64 + floor); 0 when both are exactly equal, inf when got is not finite or a zero bound is missed"""
    if not math.isfinite(got):
        return math.inf
    err = abs(got - ref64)
    if err == 0.0:
        return 0.0
    b = rel * ref64 + floor
    return err / b if b > 0.0 else math.inf


# ------------------------------------------------------------------------------------------------------- the fp32 model
def _butterfly(v: torch.Tensor) -> torch.Tensor:
    """[..., 64]: v += v[lane ^ m] for m = 32 .. 1; every lane ends with the same bits, lane 0 is returned"""
    lane = torch.arange(64)
    for m in (32, 16, 8, 4, 2, 1):
        v = v + v[..., lane ^ m]
    return v[..., 0]


def _waves_in_order(s: torch.Tensor) -> torch.Tensor:
    t = s[..., 0]
    for i in range(1, 4):
        t = t + s[..., i]
    return t


def emulate(ref: torch.Tensor, y: torch.Tensor, w: torch.Tensor, bm: int, mistake: Optional[str] = None) -> float:
    """The tail's operations in fp32 torch ops on the CPU, in the kernel's order.  y: the value the epilogue rounds - fp16 (the
    stored y16 itself) or fp32 (accumulator + bias, rounded to fp16 here as the kernel does).
    A tile is bm x 128: wavefront (wm, wn) of its 2 x 2 owns rows wm * 16 MT .., outputs wn * 64 ..; lane l holds the four
    outputs 4 (l & 15) .. + 3 of rows m * 16 + 4 (l >> 4) + i, m < MT, i < 4, and walks them m-major.  Rows past T read row T - 1
    (ref, y and weight), output groups past O read the group at O - 4: clamped duplicates, selected away.
    mistake: one deliberate error -
      rows_past_T_counted    the row half of the select is missing: the duplicates of row T - 1 count, with its weight
      cols_past_O_counted    the column half of the select is missing: the duplicates of outputs O - 4 .. O - 1 count
      clamped_row_weight     a lane reads ONE weight per 4-row block, at its first row (clamped): rows + 1 .. + 3 take that one
      y_not_rounded_to_fp16  the difference is taken from the fp32 value, not from its fp16 rounding
      neighbour_weight       w[t + 1] (the last row: w[0])
      diff_fp16              e rounded to fp16
      partial_of_last_tile_dropped   the finish adds tiles - 1 partials"""
    assert mistake is None or mistake in MISTAKES
    T, O = ref.shape
    if T == 0 or O == 0:
        return 0.0
    mt = bm // 32
    n_row, n_col = (T + bm - 1) // bm, (O + BN - 1) // BN
    t_idx = torch.arange(n_row * bm)
    o_idx = torch.arange(n_col * BN)
    tc = t_idx.clamp(max=T - 1)
    grp = o_idx // 4 * 4
    oc = torch.where(grp < O, grp, torch.full_like(grp, O - 4)) + o_idx % 4
    r = ref.float()[tc][:, oc]
    yv = y[tc][:, oc]
    yf = yv.float() if mistake == "y_not_rounded_to_fp16" else yv.half().float()
    e = r - yf
    if mistake == "diff_fp16":
        e = e.half().float()
    sq = (e * e).reshape(n_row * bm, n_col * 32, 4)
    s = torch.zeros(n_row * bm, n_col * 32, dtype=torch.float32)
    for n in range(4):
        s = s + sq[..., n]
    wf = w.float()
    if mistake == "neighbour_weight":
        wt = wf[(tc + 1) % T]
    elif mistake == "clamped_row_weight":
        wt = wf[(t_idx // 4 * 4).clamp(max=T - 1)]
    else:
        wt = wf[tc]
    ws = wt.unsqueeze(1) * s
    keep_t = torch.ones_like(t_idx, dtype=torch.bool) if mistake == "rows_past_T_counted" else t_idx < T
    keep_o = torch.ones(n_col * 32, dtype=torch.bool) if mistake == "cols_past_O_counted" else torch.arange(n_col * 32) * 4 < O
    ws = torch.where(keep_t.unsqueeze(1) & keep_o.unsqueeze(0), ws, torch.zeros_like(ws))   # the select: + 0 is exact
    # [row_blk, wm, m, q, i, col_blk, wn, l15] -> [row_blk, col_blk, wm, wn, q, l15, m, i]
    v = ws.reshape(n_row, 2, mt, 4, 4, n_col, 2, 16).permute(0, 5, 1, 6, 3, 7, 2, 4)
    acc = torch.zeros(v.shape[:6], dtype=torch.float32)
    for m in range(mt):
        for i in range(4):
            acc = acc + v[..., m, i]
    waves = _butterfly(acc.reshape(n_row, n_col, 4, 64))             # wave = wm * 2 + wn, lane = q * 16 + l15
    partials = _waves_in_order(waves).reshape(-1)                     # index row_blk * n_col + col_blk
    if mistake == "partial_of_last_tile_dropped":
        partials = partials[:-1]
    n = partials.numel()
    n_j = max(1, (n + BLOCK - 1) // BLOCK)
    f = torch.cat([partials, torch.zeros(n_j * BLOCK - n, dtype=torch.float32)]).reshape(n_j, BLOCK)
    lane = torch.zeros(BLOCK, dtype=torch.float32)
    for j in range(n_j):
        lane = lane + f[j]
    return float(_waves_in_order(_butterfly(lane.reshape(4, 64))))


# ------------------------------------------------------------------------------- the format search's layer (matrix_cores=True)
SEARCH_ROWS = (3, 7, 16, 29, 40)                       # 5 samples of 3 .. 40 rows
SEARCH_C, SEARCH_OUTS, SEARCH_SEED = 384, 256, 0
ORACLE_TABLE = {"fp_e1": "e1m2", "fp_e2": "e2m1", "fp_e3": "e3m0", "fp6_e2m3": "e2m3", "fp6_e3m2": "e3m2"}


@functools.lru_cache(maxsize=None)
def search_layer_case(seed: int = SEARCH_SEED, w_dtype=torch.float16):
    """(xs: 5 float16 samples [rows_j, 384], heavy-tailed like pre-quantization activations; w [256, 384]) on the CPU"""
    g = torch.Generator().manual_seed(4100 + seed)
    xs = tuple((torch.randn(r, SEARCH_C, generator=g) * torch.exp(0.5 * torch.randn(r, SEARCH_C, generator=g))).half() for r in SEARCH_ROWS)
    w = (torch.randn(SEARCH_OUTS, SEARCH_C, generator=g) * 0.02).to(w_dtype)
    return xs, w


def cpu_loss_table(xs, w, formats) -> torch.Tensor:
    """float64 [nf, nf] (weight index, activation index): the fused=True search's loss table with the oracle's quantizers
    (oracle/fpq_oracle.py: x in its dtype, w in its dtype) and float32 CPU products - what the winner's margin is read from"""
    from oracle import fpq_oracle as orc

    def q(fmt, t):
        name = ORACLE_TABLE[fmt]
        return orc.per_token_kernel_sem(t, name, t.dtype) if fmt.startswith("fp6") else orc.per_group_kernel_sem(t, name, 128)
    x_all = torch.cat([x.reshape(-1, w.shape[1]) for x in xs])
    rows = [x.shape[0] for x in xs]
    w_row = torch.repeat_interleave(torch.tensor([1.0 / (r * w.shape[0]) for r in rows], dtype=torch.float64), torch.tensor(rows))
    ref = x_all.float() @ w.float().t()
    out = torch.empty(len(formats), len(formats), dtype=torch.float64)
    for i, wf in enumerate(formats):
        wq = q(wf, w).float()
        for j, af in enumerate(formats):
            y = q(af, x_all).float() @ wq.t()
            out[i, j] = (((ref - y).double() ** 2).sum(dim=1) * w_row).sum()
    return out


def winner_margin(table: torch.Tensor) -> float:
    """(runner-up - best) / best of a loss table"""
    v = table.reshape(-1).sort().values
    return float((v[1] - v[0]) / v[0])


# ---------------------------------------------------------------------------------------------------------------- inputs
def sample_weights(tokens: int, outs: int, g) -> torch.Tensor:
    """the search's weights: samples of 1 .. tokens / 5 + 1 rows each, 1 / (rows_j * outs) per row, float32"""
    out, left = [], tokens
    while left:
        r = min(left, int(torch.randint(1, max(2, tokens // 5) + 1, (1,), generator=g)))
        out += [1.0 / (r * outs)] * r
        left -= r
    return torch.tensor(out, dtype=torch.float32)


@functools.lru_cache(maxsize=None)
def make_case(tokens: int, outs: int, ref_dtype, family: str = "gauss", seed: int = 0):
    """(ref [tokens, outs] of ref_dtype, y float32 [tokens, outs], w float32 [tokens]) on the CPU; read-only (cached).
      gauss    y a product of gaussian factors with a scale per row (an accumulator + bias), ref = y + noise of 2 % of its size
      equal    ref == half(y): the loss is exactly 0
      weights  gauss with weights 1e-6 .. 1, log-spaced, shuffled over the rows
      fp16_max gauss, row 0: ref = 65504, y = -65504 (every difference 131008: not an fp16 number)"""
    g = torch.Generator().manual_seed(7919 * seed + 31 * tokens + outs + (0 if ref_dtype == torch.float16 else 1))
    base = torch.randn(tokens, 16, generator=g, dtype=torch.float64) @ torch.randn(16, outs, generator=g, dtype=torch.float64) / 4.0
    base = base * torch.exp(0.5 * torch.randn(tokens, 1, generator=g, dtype=torch.float64))
    y = base.float()
    ref = (base + 0.02 * base.abs().mean() * torch.randn(tokens, outs, generator=g, dtype=torch.float64)).to(ref_dtype)
    w = sample_weights(tokens, outs, g)
    if family == "equal":
        ref = y.half().to(ref_dtype)
    elif family == "weights":
        w = torch.logspace(-6, 0, tokens, dtype=torch.float64)[torch.randperm(tokens, generator=g)].float()
    elif family == "fp16_max":
        ref, y = ref.clone(), y.clone()
        ref[0], y[0] = 65504.0, -65504.0
    else:
        assert family == "gauss", family
    return ref.contiguous(), y.contiguous(), w.contiguous()
