"""What gelu_tanh_fast (fpqvar_amd/csrc/fpq_fast16.h) must compute, and how close it has to come: the FFN's GELU(tanh) between fc1 and
fc2's input quantizer, in the epilogue of every fc1 GEMM form and in the stand-alone fpq_gelu_quant_rows_dual.

Shared by tests/test_gelu_model_host.py (CPU: the bound holds for the reference's own fp32 op sequence and for the kernel's, and is
sharp enough to catch each of a list of plausible mistakes), tests/test_gpu_gelu.py (every instantiation of the kernel against it, on
every fp16 input) and tests/block_model.py (the block's GELU is `reference`).  The domain is finite - 65536 fp16 patterns - so every
statement here is checked on all of it.

- reference(x): the definition in float64.
- bound(x16): the per-element error bound, derived in its docstring from the reference's op sequence.
- emulate(x16, snap, mutation): an fp32 model of gelu_tanh_fast step by step, optionally with one deliberate mistake.
- ratio / class_mismatch: how a result is held to reference and bound.
- every_fp16() / correctly_rounded(): all inputs, and the fp16 nearest to the float64 value.
"""
import math
from typing import Optional

import numpy as np
import torch

from tests.gemm_model import fma32

KAPPA = 0.044715
BETA = math.sqrt(2.0 / math.pi)
MUTATIONS = ("kappa", "beta", "erf", "sigmoid", "w_fp16", "exp_for_exp2", "ftz_out", "rtz_out")
ALTERNATIVES = ("erf", "sigmoid")                # mutations that replace the function itself: they apply to the reference


def every_fp16(device=None) -> torch.Tensor:
    """all 65536 fp16 bit patterns in order: element i has the bits i"""
    return torch.arange(0, 65536, dtype=torch.int32, device=device).to(torch.int16).view(torch.float16)


def bits(h: torch.Tensor) -> torch.Tensor:
    """fp16 -> its bit pattern 0 .. 65535 (int64: an index into a 65536-entry table)"""
    return h.contiguous().view(torch.int16).to(torch.int64) & 0xFFFF


# ------------------------------------------------------------------------------------------------------------ reference
def reference(x: torch.Tensor) -> torch.Tensor:
    """0.5 x (1 + tanh(sqrt(2 / pi) (x + 0.044715 x^3))) in float64 (F.gelu(x, approximate="tanh") by its definition), of an fp16
    tensor or of float64 values.  NaN -> NaN, +inf -> +inf, -inf -> NaN (0.5 * -inf * (1 + -1)); a finite x below about -7.3 gives
    -0: float64's tanh is -1 there and the true value, below 2^-50, is nowhere near the fp16 grid.  1 + tanh(u) cancels for
    negative x, with an absolute error of 2^-53: at most 2^-54 |x| < 2^-37 in the result, 2^-12 of the smallest term of bound()."""
    x = x.double()
    return 0.5 * x * (1.0 + torch.tanh(math.sqrt(2.0 / math.pi) * (x + 0.044715 * x ** 3)))


def ulp16(g: torch.Tensor) -> torch.Tensor:
    """the spacing of fp16 at |g| (float64): 2^(e - 10) for 2^e <= |g| < 2^(e + 1), 2^-24 below 2^-14, 32 from 32768 on"""
    e = torch.frexp(g.abs().clamp_min(2.0 ** -14))[1].double() - 1.0        # frexp: |g| = m 2^exp, m in [0.5, 1)
    return torch.exp2(e.clamp_max(15.0) - 10.0)


def bound(x16: torch.Tensor) -> torch.Tensor:
    """Per-element bound on |out - reference(x16)| for a finite fp16 input x with g = reference(x):

        B(x) = 1.001 * ulp16(g) / 2  +  1.5 * 2^-24 |x|  +  2^-22 |g|

    Derived from the REFERENCE's op sequence, not from the kernel's.  torch (aten/src/ATen/native/cuda/ActivationGeluKernel.cu,
    approximate == tanh, opmath float) computes in fp32, one rounding each (relative 2^-24 =: u),

        x3 = x x x;  inner = kBeta (x + kKappa x3);  t = tanhf(inner);  g32 = 0.5 x (1 + t);  out = fp16(g32).

    - ulp16(g) / 2: the one rounding to fp16, nearest-even: half a spacing of the grid at g (2^-25 for a subnormal result; g never
      reaches the overflow edge: |g| <= |x| <= 65504).  The factor 1.001 covers the second order - the spacing at g32 instead of at
      g when the fp32 error carries it across a power of two, where the spacing doubles: the terms below are under 2^-10 of it.
    - 1.5 * 2^-24 |x| = |x| / 2 times the absolute error of s = 1 + t, at most 3 * 2^-24:
        2 * 2^-24   tanhf is allowed 2 ulps (the device library documents 2 for tanhf); |t| < 1, so its ulp is at most 2^-24;
        2^-24       the addition rounds to half an ulp of a sum in [1, 2) (x > 0); for x < 0 the sum is in [0, 1], its half ulp at
                    most 2^-25, and for t <= -0.5 it is exact (Sterbenz) - that is where the deep negatives live, and where
                    this term is what the result is made of: s is a small multiple of 2^-24 and g32 = 0.5 x s steps by 2^-25 |x|.
    - 2^-22 |g| = 4 u |g|: 0.5 x is exact; the last product rounds once, u |g|.  The other 3 u |g| belong to the argument.
      inner carries a relative error of at most 3 u on the whole (the sum, the constant kBeta, the product with it) and 3 u
      more on its cubic part (x x is exact for an fp16 x; x3 rounds once, the constant kKappa, the product with it), and tanh
      passes a relative error on times |inner| sech^2(inner) <= 0.448: t moves by less than 2.7 u and g by 1.35 u |x|.  For
      x > 0, |x| <= 2 |g| and 3 u |g| >= 1.5 u |x| holds it.  For x < 0, where |g| is small, it is paid out of what the
      second term does not use there: the addition is exact for t <= -0.5, tanhf's 2 ulps are ulps of 2^-25 or less for
      |t| < 0.5, and |inner| sech^2(inner) falls below 0.1 beyond |x| = 2.5.  bound_terms() adds the separate terms up for
      each input without these simplifications, and test_gelu_model_host.py checks that B dominates it on every input.

    No term for rounding anything to fp16 before the end, for exp2 / rcp in place of tanhf (the kernel's two hardware
    approximations, 1 ulp each, come out of tanhf's 2 ulps) or for a snap: the kernel gets the reference's bound, no factor.

    Non-finite x: the bound is NaN where g is (NaN, -inf) and inf at +inf; class_mismatch() holds those inputs."""
    x = x16.double()
    g = reference(x16)
    return 1.001 * 0.5 * ulp16(g) + 1.5 * 2.0 ** -24 * x.abs() + 2.0 ** -22 * g.abs()


def bound_terms(x16: torch.Tensor) -> torch.Tensor:
    """The accounting of bound()'s docstring without its simplifications, per input: half a spacing of fp16, |x| / 2 times (tanhf's
    2 ulps at t + the half ulp of 1 + t, zero where Sterbenz makes the sum exact + the argument's 3 u, and 3 u more on its cubic
    part, passed through tanh), and the last product's u |g|.  bound() must dominate it."""
    u = 2.0 ** -24
    x = x16.double()
    g = reference(x16)
    cubic = KAPPA * x ** 3
    inner = BETA * (x + cubic)
    t = torch.tanh(inner)
    ulp32 = lambda v: torch.exp2(torch.frexp(v.abs().clamp_min(2.0 ** -126))[1].double() - 24.0)      # spacing of fp32 at |v|
    s = 1.0 + t
    add = torch.where(t <= -0.5, torch.zeros_like(t), 0.5 * ulp32(s))
    arg_rel = 3.0 * u + 3.0 * u * (cubic / (x + cubic)).nan_to_num(0.0).abs()
    arg = inner.abs() * (1.0 - t * t) * arg_rel
    return 0.5 * ulp16(g) + 0.5 * x.abs() * (2.0 * ulp32(t.abs().clamp_max(1.0 - 2.0 ** -25)) + add + arg) + u * g.abs()


def correctly_rounded(x16: torch.Tensor) -> torch.Tensor:
    """fp16 nearest to reference(x16), rounded ONCE from float64: the cast through fp32 (torch's) rounds twice - at x = +-2^-24 the
    value is 2^-25 (1 + 4.7e-8), fp32 makes it the tie 2^-25 and nearest-even then 0, where the nearest fp16 is 2^-24 - so the
    nearer of that cast and its two neighbours on the fp16 grid is taken (no float64 value of the reference is an exact tie)."""
    g = reference(x16)
    h = g.float().half()
    b = bits(h)
    o = torch.where(b >= 0x8000, 0x8000 - b, b)                                   # integers that grow with the value
    best = h
    for d in (-1, 1):
        n = (o + d).clamp(-0x7C00, 0x7C00)
        n = torch.where(n < 0, 0x8000 - n, n).to(torch.int16).view(torch.float16)
        n = torch.where(n == 0, torch.copysign(torch.zeros_like(n), g.half()), n)
        best = torch.where(torch.isfinite(g) & ((n.double() - g).abs() < (best.double() - g).abs()), n, best)
    return best


def tie_distance(x16: torch.Tensor) -> torch.Tensor:
    """how far reference(x16) is from the nearest rounding tie of fp16 (the midpoint of two neighbours), relative to |g|: below
    2^-24 an fp32 computation cannot tell on which side of the tie the value lies"""
    g = reference(x16)
    c = correctly_rounded(x16).double()
    return ((c - g).abs() - 0.5 * ulp16(torch.minimum(c.abs(), g.abs()))).abs() / g.abs()


def class_mismatch(out: torch.Tensor, x16: torch.Tensor) -> torch.Tensor:
    """Inputs whose result has the wrong class: NaN exactly where the reference is NaN (NaN and -inf), +inf exactly at +inf, and a
    zero result carries the sign of the reference (x < 0 underflows to -0, as 0.5 x (1 + t) does in any precision; -0 -> -0)."""
    o = out.to(x16.device)
    g = reference(x16)
    bad = torch.isnan(o) != torch.isnan(g)
    bad |= torch.isinf(o) != torch.isinf(g)
    bad |= torch.isinf(o) & torch.isinf(g) & (o.double() != g)
    bad |= (o == 0) & ~torch.isnan(g) & (torch.signbit(o) != torch.signbit(g))
    return bad


def ratios(out: torch.Tensor, x16: torch.Tensor) -> torch.Tensor:
    """|out - reference| / bound per input, 0 where the reference is not finite"""
    g = reference(x16)
    r = (out.to(x16.device).double() - g).abs() / bound(x16)
    return torch.where(torch.isfinite(g) & torch.isfinite(out.to(x16.device).double()), r, torch.zeros_like(r))


def ratio(out: torch.Tensor, x16: torch.Tensor) -> float:
    """max |out - reference| / bound over the inputs where both are finite; inf when the class of any result is wrong"""
    if bool(class_mismatch(out, x16).any()):
        return math.inf
    return float(ratios(out, x16).max())


# ------------------------------------------------------------------------------------------------------------ the model
def _fp16_out(y32: torch.Tensor, mutation: Optional[str]) -> torch.Tensor:
    h = y32.half()
    if mutation == "rtz_out":            # toward zero: step a rounded-up magnitude back by one code
        up = h.float().abs() > y32.abs()
        h = torch.where(up, (h.view(torch.int16) - 1).view(torch.float16), h)
    elif mutation == "ftz_out":          # no fp16 subnormals: a result below 2^-14 becomes a zero of its sign
        h = torch.where(h.float().abs() < 2.0 ** -14, torch.copysign(torch.zeros_like(h), h), h)
    return h


def emulate(x16: torch.Tensor, snap: bool = True, mutation: Optional[str] = None) -> torch.Tensor:
    """fp32 model of gelu_tanh_fast on the CPU -> fp16, in the order of its source:

        kBeta = fp32(sqrt2 * 2/sqrt(pi) * 0.5), kKappa = fp32(0.044715);  c0 = fl(fp32(-2 log2 e) kBeta), c1 = fl(c0 kKappa)
        m = fl(x fma(fl(x x), c1, c0));  e = exp2(m);  w = 1 / fl(1 + e);  snap: w = fl(fl(w - 0.5) + 0.5);  out = fp16(fl(x w))

    with exp2 and the reciprocal correctly rounded (the hardware's v_exp_f32 and v_rcp_f32 are allowed one ulp each).  snap=False
    leaves the snap out.  `mutation` makes one mistake - in the model, or (ALTERNATIVES) computes another function in float64:
      kappa         kKappa = 0.04471
      beta          kBeta = 0.798
      erf           the exact GELU, 0.5 x (1 + erf(x / sqrt 2))
      sigmoid       x sigmoid(1.702 x)
      w_fp16        w rounded to fp16 before the multiply
      exp_for_exp2  e = exp(m): the base-2 constant without the base-2 exponential
      ftz_out       an fp16-subnormal result flushed to zero
      rtz_out       the final conversion truncates"""
    assert mutation is None or mutation in MUTATIONS, mutation
    assert x16.dtype == torch.float16
    if mutation == "erf":
        xd = x16.double()
        return (0.5 * xd * (1.0 + torch.erf(xd / math.sqrt(2.0)))).float().half()
    if mutation == "sigmoid":
        xd = x16.double()
        return (xd * torch.sigmoid(1.702 * xd)).float().half()
    f32 = lambda v: torch.tensor(v, dtype=torch.float32)
    k_beta = f32(0.798 if mutation == "beta" else 1.41421356237309504880 * 1.12837916709551257390 * 0.5)
    k_kappa = f32(0.04471 if mutation == "kappa" else 0.044715)
    c0 = f32(-2.8853900817779268) * k_beta
    c1 = c0 * k_kappa
    x = x16.float()
    m = x * fma32(x * x, c1.expand_as(x), c0.expand_as(x))
    md = m.double()
    e = (torch.exp(md) if mutation == "exp_for_exp2" else torch.exp2(md)).float()
    w = (1.0 / (1.0 + e).double()).float()
    if mutation == "w_fp16":
        w = w.half().float()
    if snap:
        w = (w - 0.5) + 0.5
    return _fp16_out(x * w, mutation)
