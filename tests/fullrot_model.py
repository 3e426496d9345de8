"""The float64 model of the full-width online rotation (csrc/fpq_fullrot.h; rotation.rotate_quant_full*): the reference, the
per-element bound, the factorised form with its mutants, and an emulation of the shipped arithmetic lane by lane.

The reference is the product with the matrix rotate_model(block_rotate=False) puts into the weights - NOT the kernel's own
factors: ``reference(h16, C) = float64(h16) @ float64(half(float32(get_orthogonal_matrix(C))))``.

The bound.  The kernel computes, per output o = ko * m + lo (C = K * m; (K, m) = (60, 32), (36, 64)),

    P[kj][lo] = sum_lj  +-h[kj * m + lj]                     m terms, fp32 accumulator of v_mfma_f32_16x16x32_f16 (m / 32 chained)
    Y[ko][lo] = sum_kj  +-(b1 + b2 + b3)(P[kj][lo])          3 K non-zero terms, fp32 accumulator of six chained bf16 MFMAs
    y         = half(float32(c_h * Y))

* The operands are exact: h is fp16, the factors are +-1, and the three bf16 pieces of P are cut by truncation - 8 + 8 + 8 = 24
  significant bits, so b1 + b2 + b3 == P with no error and |b1| + |b2| + |b3| == |P| (the pieces carry P's sign).  The split adds
  NO absolute term (bf16 has fp32's exponent range, P is a multiple of 2^-24).
* The order in which a matrix core adds the terms of one instruction is not specified, so every addition into a non-empty
  accumulator counts as one fp32 rounding of a partial sum whose magnitude is at most the sum of the magnitudes of its terms:
  m - 1 in stage 1 (relative to sum_lj |h|), 3 K - 1 in stage 2 (relative to sum_kj |P| <= sum_j |h_j| (1 + tiny)); stage 1's
  errors pass through stage 2's +-1 unchanged.  One more for the product with c_h.
      depth = (m - 1) + (3 K - 1) + 1 = m + 3 K - 1        (211 at C = 1920, 171 at C = 2304)
      E     = depth * 2^-24 * c_h * sum_j |h_j|
* The rounding to fp16 adds half an fp16 ulp of the value being rounded, which lies within E of the reference - the ulp is taken
  at |ref| + E - and (1 + 2^-11) covers the double rounding (fp32, then fp16).
      bound = 0.5 * ulp16(|ref| + E) * (1 + 2^-11) + E
"""
import numpy as np
import torch

from fpqvar_amd import rotation

WIDTHS = (1920, 2304)          # the widths the library builds (csrc/fpq_fullrot.h, kFullRotWidths)


def factors(C):
    had_k, K = rotation.get_hadK(C)
    return had_k.double(), K, C // K


def c_h(C):
    """The one magnitude of half(float32(Q))."""
    return float(q_half(C).abs().max())


_Q = {}


def q_half(C):
    if C not in _Q:
        _Q[C] = rotation.get_orthogonal_matrix(C).float().half().double()
    return _Q[C]


def reference(h16, C):
    """float64 h @ Q_h, Q_h the fp16 matrix the offline weight side is rotated with."""
    assert h16.dtype is torch.float16 and h16.shape[-1] == C
    return h16.double().cpu() @ q_half(C)


def depth(C):
    _, K, m = factors(C)
    return m + 3 * K - 1


def ulp16(a):
    a = a.abs().clamp_min(2.0 ** -14)
    return 2.0 ** (torch.floor(torch.log2(a)).clamp_max(15.0) - 10)


def bound(h16, ref, C):
    e = depth(C) * 2.0 ** -24 * c_h(C) * h16.double().cpu().abs().sum(-1, keepdim=True)
    return 0.5 * ulp16(ref.abs() + e) * (1 + 2.0 ** -11) + e


def factorised(h16, C, d=None, had_t=False, swap=False, c=None, drop=None):
    """c . hadK . X . Sylvester(m) in float64, X[kj][lj] = (h D)[kj * m + lj].  The mutants: had_t - hadK transposed; swap - the
    Kronecker order swapped (the Sylvester part on the HIGH index bits); c - another constant; drop - one kj segment left out;
    d - another sign vector (the tiled 128-vector)."""
    had_k, K, m = factors(C)
    d = rotation.sign_vector(C, 42) if d is None else d
    rows = h16.shape[0]
    x = h16.double().cpu() * d.double()
    syl = rotation.sylvester(m).double()
    hk = had_k.T if had_t else had_k
    if drop is not None:
        hk = hk.clone()
        hk[:, drop] = 0.0
    if swap:
        y = torch.einsum("ok,rlk,pl->rpo", hk, x.view(rows, m, K), syl)
    else:
        y = torch.einsum("ok,rkl,pl->rop", hk, x.view(rows, K, m), syl)
    return y.reshape(rows, C) * (c_h(C) if c is None else c)


def _split3(p):
    """fp32 -> three bf16 pieces by truncation, as fr_split3 (finite inputs)."""
    b = p.view(np.uint32)
    t1 = (b & np.uint32(0xFFFF0000)).view(np.float32)
    r1 = p - t1
    t2 = (r1.view(np.uint32) & np.uint32(0xFFFF0000)).view(np.float32)
    r2 = r1 - t2
    t3 = (r2.view(np.uint32) & np.uint32(0xFFFF0000)).view(np.float32)
    assert np.array_equal(t3, r2), "the third piece holds what is left exactly"
    return t1, t2, t3


def _popc(v):
    return bin(int(v)).count("1") & 1


def emulate(h16, C, d=None):
    """The shipped arithmetic with the kernel's own operand mapping (csrc/fpq_fullrot.h), fp32 accumulators added term by term
    in slot order: lane (i, q) of stage 1's A operand (T, s) holds X[16 T + i][32 s + 8 q + e]; its B operand element
    (k = 8 q + e, n) is (-1)^(popcount(e & n & 7) + popcount((4 s + q) & (2 nt + n / 8))); the accumulators P[T][4 q + r][n] enter
    stage 2 as k-slot (q, e) of step tp = M-tile 2 tp + e / 4, row 4 q + e % 4, against hadK[16 mo + i][16 (2 tp + e / 4) + 4 q + e % 4]."""
    had_k, K, m = factors(C)
    d = rotation.sign_vector(C, 42) if d is None else d
    rows = h16.shape[0]
    KT, NT, KS = (K + 15) // 16, m // 16, m // 32
    x = (h16.float().cpu() * d.float()).numpy().reshape(rows, K, m)
    xp = np.zeros((rows, KT * 16, m), np.float32)
    xp[:, :K] = x
    hk = np.zeros((KT * 16, 64), np.float32)
    hk[:K, :K] = had_k.numpy()
    ch = np.float32(c_h(C))
    out = np.zeros((rows, K, m), np.float16)
    for nt in range(NT):
        P = np.zeros((rows, KT, 16, 16), np.float32)          # [T][row of the tile][n]
        for s in range(KS):
            for q in range(4):
                for e in range(8):
                    k = 32 * s + 8 * q + e
                    sgn = np.array([(-1.0) ** (_popc(e & n & 7) + _popc((4 * s + q) & (2 * nt + (n >> 3)))) for n in range(16)], np.float32)
                    assert all(sgn[n] == (-1.0) ** _popc(k & (16 * nt + n)) for n in range(16))   # = Sylvester(m)[lj][lo]
                    a = xp[:, :, k].reshape(rows, KT, 16)
                    P = (P + a[:, :, :, None] * sgn[None, None, None, :]).astype(np.float32)
        pieces = _split3(P)
        Y = np.zeros((rows, KT, 16, 16), np.float32)          # [mo][i][n]
        for tp in range(2):
            for piece in pieces:
                for q in range(4):
                    for e in range(8):
                        T, r = 2 * tp + (e >> 2), 4 * q + (e & 3)
                        if T >= KT:
                            continue
                        kj = 16 * T + r
                        a = hk[:, kj].reshape(KT, 16)                                   # hadK[16 mo + i][kj]
                        Y = (Y + a[None, :, :, None] * piece[:, T, r, None, None, :]).astype(np.float32)
        y = (Y * ch).astype(np.float32).astype(np.float16).reshape(rows, KT * 16, 16)
        out[:, :, 16 * nt:16 * nt + 16] = y[:, :K]
    return torch.from_numpy(out.reshape(rows, C))


def rows_gauss(rows, C, seed=0):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(rows, C, generator=g).half()


def rows_heavy(rows, C, seed=1):
    g = torch.Generator().manual_seed(seed)
    return (torch.randn(rows, C, generator=g) * torch.exp(0.7 * torch.randn(rows, C, generator=g))).half()


def rows_dominant(rows, C, seed=2):
    x = rows_gauss(rows, C, seed) * 0.01
    for r in range(rows):
        x[r, (r * 977 + 13) % C] = 3000.0 * (1 if r % 2 else -1)
    return x


def rows_cancelling(rows, C, seed=3):
    """Rows proportional to a column of Q plus noise 2^-12 of its size: one large output, the rest cancel."""
    q = q_half(C)
    x = torch.empty(rows, C, dtype=torch.float16)
    base = rows_gauss(rows, C, seed)
    for r in range(rows):
        x[r] = (torch.sign(q[:, (r * 131 + 7) % C]) * 8.0 + base[r].double() * 2.0 ** -9).half()
    return x


FAMILIES = {"gauss": rows_gauss, "heavy": rows_heavy, "dominant": rows_dominant, "cancelling": rows_cancelling}
