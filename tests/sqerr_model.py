"""What fpq_sqerr_rows_weighted (fpqvar_amd/csrc/fpq_kernels.hip: sqerr_partials_kernel, sqerr_finish_kernel) must return and how
close it has to come:   out[p] = sum_r w[r] sum_c (ref[r, c] - y[p][r, c])^2,   the format search's loss.

Shared by tests/test_sqerr_model_host.py (CPU: the bound is sound for the kernel's order of operations and sharp enough to
catch each of a list of plausible kernel mistakes) and tests/test_gpu_sqerr.py (the kernel).

- reference(ref, y, w): the loss in float64 from the same stored inputs, one value per plane.
- deal(rows, cols, dtype) / chain(rows, cols, dtype) / bound(rows, cols, dtype, w_max): how the kernel deals the vectors, the
  longest chain of fp32 additions D and the other roundings c that follow from it, and the bound (relative part, absolute floor).
- emulate(ref, y, w, mistake): the kernel's operations in fp32 on the CPU in the kernel's order, optionally with one mistake.
- expected_class(ref, y): "nan" / "inf" / "finite" per plane by the fp32 expression's rule.
- make_case(family, rows, cols, dtype, planes): the input families.
"""
import functools
import math
from typing import List, Optional, Tuple

import torch

U = 2.0 ** -24                      # unit roundoff of fp32
BLOCK = 256                         # kBlock
MAX_BLOCKS = 2048                   # kSqerrMaxBlocks = FPQ_SQERR_WORKSPACE_BYTES / 16
C_ROUNDINGS = 3                     # the difference, the square, the weight
MISTAKES = ("diff_fp16", "square_acc_fp16", "neighbour_weight", "weight_plane0_only", "drop_last_block", "planes_swapped",
            "ref_plane_offset")
FINITE_FAMILIES = ("gauss", "equal", "fp16_max", "subnormal", "weights")
NONFINITE_FAMILIES = ("inf_ref", "nan_ref", "inf_y", "nan_y", "inf_both", "nan_both")


def vec(dtype) -> int:
    return 8 if dtype == torch.float16 else 4


def deal(rows: int, cols: int, dtype) -> Tuple[int, int, int]:
    """(16-byte vectors, workgroups, a lane's iterations): vector v goes to lane v % (grid * 256), which walks v, v + grid * 256, ..."""
    n_vec = rows * cols // vec(dtype)
    grid = max(1, min((n_vec + BLOCK - 1) // BLOCK, MAX_BLOCKS))
    n_it = (n_vec + grid * BLOCK - 1) // (grid * BLOCK)
    return n_vec, grid, n_it


def chain(rows: int, cols: int, dtype) -> Tuple[int, int]:
    """(D, c) from the kernel's source.  The fp32 additions one term passes through, in order:
      V      s += e e inside its 16-byte vector (8 fp16 / 4 fp32 elements; the first adds to 0)
      n_it   acc += w s, once per vector the lane visits
      6      the wavefront's butterfly (__shfl_xor 32, 16, 8, 4, 2, 1)
      3      the workgroup's four wavefront sums, in order
      8      the finishing workgroup: lane i adds partials i, i + 256, ... (at most 2048 / 256)
      6 + 3  its butterfly and its four wavefront sums
    D = V + n_it + 26.  c = 3: the roundings of e = r - q, of e e and of w s (no fused multiply-add: -ffp-contract=off)."""
    return vec(dtype) + deal(rows, cols, dtype)[2] + 26, C_ROUNDINGS


def bound(rows: int, cols: int, dtype, w_max: float = 1.0) -> Tuple[float, float]:
    """(rel, floor):  |got - ref64| <= rel * ref64 + floor.

    Every term w e^2 is non-negative, so every partial sum is a sum of non-negative numbers: a rounding of relative size U
    anywhere moves the total by at most U times the part it acts on, and a term meets at most D + c of them.  To first order
    |got - ref64| <= (D + c) U ref64; the factor (1 + U)^(D + c) - 1 is used instead, which is the rigorous form.
    fp16 inputs: the smallest non-zero |e| is 2^-24, e^2 >= 2^-48, and with w >= 2^-70 nothing goes subnormal: floor = 0, and
    a zero reference must be met exactly.  fp32 inputs: a square or a weighted vector sum that lands below 2^-126 is rounded
    with an absolute error of at most 2^-150; V squares per vector pass through w, so floor = (rows cols w_max + n_vec) 2^-149.
    Input conditions (asserted by the tests): weights finite and positive; for fp32, |e| < 2^63 and a total below 2^127, so
    that fp32 does not overflow where float64 does not."""
    D, c = chain(rows, cols, dtype)
    rel = (1.0 + U) ** (D + c) - 1.0
    floor = 0.0 if dtype == torch.float16 else (rows * cols * max(w_max, 1.0) + deal(rows, cols, dtype)[0]) * 2.0 ** -149
    return rel, floor


def reference(ref: torch.Tensor, y: torch.Tensor, w: torch.Tensor) -> torch.Tensor:
    """float64 [planes] from the stored inputs: sum_r w[r] sum_c (ref - y[p])^2, the row sums first (a NaN / inf difference gives
    NaN / +inf, as in fp32: all weights are positive)."""
    y3 = y if y.dim() == 3 else y.unsqueeze(0)
    r64, w64 = ref.double(), w.double()
    return torch.stack([(((r64 - y3[p].double()) ** 2).sum(dim=1) * w64).sum() for p in range(y3.shape[0])])


def expected_class(ref: torch.Tensor, y: torch.Tensor) -> List[str]:
    """per plane: 'nan' if any fp32 difference is NaN (a NaN input, or inf - inf), else 'inf' if any is infinite, else 'finite'"""
    y3 = y if y.dim() == 3 else y.unsqueeze(0)
    out = []
    for p in range(y3.shape[0]):
        e = ref.float() - y3[p].float()
        out.append("nan" if bool(torch.isnan(e).any()) else "inf" if bool(torch.isinf(e).any()) else "finite")
    return out


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
    """lanes_sum64 on [..., 64]: v += v[lane ^ m] for m = 32 .. 1; every lane ends with the same bits, lane 0 is returned"""
    lane = torch.arange(64)
    for m in (32, 16, 8, 4, 2, 1):
        v = v + v[..., lane ^ m]
    return v[..., 0]


def _lanes_then_waves(v: torch.Tensor) -> torch.Tensor:
    """[..., 256] -> [...]: the butterfly in each of the four wavefronts, then their sums added in order"""
    s = _butterfly(v.reshape(*v.shape[:-1], 4, 64))
    t = s[..., 0]
    for i in range(1, 4):
        t = t + s[..., i]
    return t


def emulate(ref: torch.Tensor, y: torch.Tensor, w: torch.Tensor, mistake: Optional[str] = None) -> torch.Tensor:
    """The kernel's operations in fp32 torch ops on the CPU, in the kernel's order -> float32 [planes].
    mistake: one deliberate error -
      diff_fp16           e rounded to fp16                         square_acc_fp16   s accumulated in fp16
      neighbour_weight    w[row + 1] (the last row: w[0])           weight_plane0_only  planes > 0 take weight 1
      drop_last_block     the vectors of the last, partly filled workgroup are not added
      planes_swapped      plane p reads y[planes - 1 - p]           ref_plane_offset  plane p reads ref one row per plane further"""
    assert mistake is None or mistake in MISTAKES
    y3 = y if y.dim() == 3 else y.unsqueeze(0)
    P = y3.shape[0]
    rows, cols = ref.shape
    V = vec(ref.dtype)
    n_vec, grid, n_it = deal(rows, cols, ref.dtype)
    G = grid * BLOCK
    row_vec = cols // V
    row_of = torch.arange(n_vec) // row_vec
    w = w.float()
    r_all = ref.float().reshape(n_vec, V)
    out = torch.zeros(P, dtype=torch.float32)
    if n_vec == 0:
        return out
    for p in range(P):
        q = y3[P - 1 - p if mistake == "planes_swapped" else p].float().reshape(n_vec, V)
        r = torch.roll(r_all, -p * row_vec, 0) if mistake == "ref_plane_offset" else r_all
        wv = w[(row_of + 1) % rows] if mistake == "neighbour_weight" else w[row_of]
        if mistake == "weight_plane0_only" and p > 0:
            wv = torch.ones_like(wv)
        s = torch.zeros(n_vec, dtype=torch.float32)
        for i in range(V):
            e = r[:, i] - q[:, i]
            if mistake == "diff_fp16":
                e = e.half().float()
            s = s + e * e
            if mistake == "square_acc_fp16":
                s = s.half().float()
        t = wv * s
        if mistake == "drop_last_block" and n_vec % BLOCK:
            t[(n_vec // BLOCK) * BLOCK:] = 0.0
        t = torch.cat([t, torch.zeros(n_it * G - n_vec, dtype=torch.float32)]).reshape(n_it, G)     # + 0 is exact
        acc = t[0]
        for it in range(1, n_it):
            acc = acc + t[it]
        partials = _lanes_then_waves(acc.reshape(grid, BLOCK))                                       # [grid]
        n_j = (grid + BLOCK - 1) // BLOCK
        f = torch.cat([partials, torch.zeros(n_j * BLOCK - grid, dtype=torch.float32)]).reshape(n_j, BLOCK)
        lane = f[0]
        for j in range(1, n_j):
            lane = lane + f[j]
        out[p] = _lanes_then_waves(lane)
    return out


# ---------------------------------------------------------------------------------------------------------------- inputs
def sample_weights(rows: int, cols: int, g) -> torch.Tensor:
    """the search's weights: samples of 1 .. 2 rows / 5 + 1 rows each, 1 / (rows_j * cols) per row, float32"""
    out, left = [], rows
    while left:
        r = min(left, int(torch.randint(1, max(2, rows // 5) + 1, (1,), generator=g)))
        out += [1.0 / (r * cols)] * r
        left -= r
    return torch.tensor(out, dtype=torch.float32)


@functools.lru_cache(maxsize=None)
def make_case(family: str, rows: int, cols: int, dtype, planes: int, seed: int = 0):
    """(ref [rows, cols], y [planes, rows, cols], w float32 [rows]) on the CPU; treat them as read-only (the case is cached).
      gauss      ref a product of gaussian factors with a scale per row, y[p] = ref + noise of size 0.02 (p + 1)
      equal      y[p] == ref: the loss is exactly 0
      fp16_max   gauss, row 0: ref = 65504, y = -65504 (every difference 131008: not an fp16 number)
      subnormal  fp16: multiples of 2^-24 below 2^-14; fp32: half the rows fp32 subnormals (squares vanish), half ~1e-22 (squares
                 subnormal)
      weights    gauss with weights 1e-9 .. 1, log-spaced, shuffled over the rows
      inf_ref / nan_ref   one element of ref non-finite (every plane);  inf_y / nan_y  one element of plane min(1, planes - 1);
      inf_both   +inf in ref and in that plane at the same place (inf - inf = NaN there, +inf in the other planes);
      nan_both   NaN in both"""
    g = torch.Generator().manual_seed(7919 * seed + 31 * rows + cols + (0 if dtype == torch.float16 else 1))
    k = 16
    base = torch.randn(rows, k, generator=g, dtype=torch.float64) @ torch.randn(k, cols, generator=g, dtype=torch.float64) / 4.0
    base = base * torch.exp(0.5 * torch.randn(rows, 1, generator=g, dtype=torch.float64))
    noise = torch.randn(planes, rows, cols, generator=g, dtype=torch.float64)
    ref = base
    y = base.unsqueeze(0) + 0.02 * torch.arange(1, planes + 1, dtype=torch.float64).view(-1, 1, 1) * noise
    w = sample_weights(rows, cols, g)
    hot = min(1, planes - 1)
    if family == "equal":
        y = base.unsqueeze(0).expand(planes, rows, cols)
    elif family == "fp16_max":
        ref, y = ref.clone(), y.clone()
        ref[0], y[:, 0] = 65504.0, -65504.0
    elif family == "subnormal":
        if dtype == torch.float16:
            ref = torch.randint(-1023, 1024, (rows, cols), generator=g).double() * 2.0 ** -24
            y = torch.randint(-1023, 1024, (planes, rows, cols), generator=g).double() * 2.0 ** -24
        else:
            tiny = (torch.arange(rows) % 2 == 0).view(-1, 1)
            ref = torch.where(tiny, torch.randint(-2 ** 20, 2 ** 20, (rows, cols), generator=g).double() * 2.0 ** -149, base * 1e-22)
            y = torch.where(tiny, torch.randint(-2 ** 20, 2 ** 20, (planes, rows, cols), generator=g).double() * 2.0 ** -149, y * 1e-22)
    elif family == "weights":
        w = torch.logspace(-9, 0, rows, dtype=torch.float64)[torch.randperm(rows, generator=g)].float()
    elif family in NONFINITE_FAMILIES:
        ref, y = ref.clone(), y.clone()
        i, j = rows // 2, (cols * 2) // 3
        if family in ("inf_ref", "inf_both"):
            ref[i, j] = math.inf
        if family in ("nan_ref", "nan_both"):
            ref[i, j] = math.nan
        if family in ("inf_y", "inf_both"):
            y[hot, i, j] = math.inf
        if family in ("nan_y", "nan_both"):
            y[hot, i, j] = math.nan
    else:
        assert family == "gauss", family
    return ref.to(dtype).contiguous(), y.to(dtype).contiguous(), w.contiguous()
