"""The FP4 GEMM's deep-ring small-M kernel (gemm_fp4_ring_kernel, FPQ_GEMM_CFG 40; fpq_gemm_fp4.h): the 64 x 128 tile of
FPQ_GEMM_CFG 30 behind a ring of S stage buffers whose LDS-DMA loads span the loop's barrier.  It does cfg 30's arithmetic in
cfg 30's order, so every output - the plain Linear, the gate / residual tail, the split output with and without the q / k norm,
the fc1 tail - must be cfg 30's bit for bit, in both operand layouts, with the group count G on either side of every point at
which the ring's prologue, steady loop and drain change shape (G around S - 1 and 2 S, G = 1, 2, 64).  A wait placed one group
early passes all of that whenever the DMA happens to land first, hence the screen at the end: 200 launches back to back over
rotating operand sets."""
import ctypes
import math
import os
import re

import pytest
import torch

from fpqvar_amd import _lib
from tests import gemm_model as gm

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
S = int(re.search(r"#define FPQ_GEMM_RING_STAGES (\d+)", open(os.path.join(ROOT, "fpqvar_amd", "csrc", "fpq_gemm_fp4.h")).read()).group(1))
T_SET = (1, 63, 64, 65, 130)
O_SET = (8, 120, 128, 136, 392)
G_SET = tuple(sorted({1, 2, S - 2, S - 1, S, S + 1, 2 * S - 1, 2 * S, 15, 18, 64}))
FAMILIES = gm.KIND_FAMILIES["fp4"]


def _cases(i):
    """the cases of T_SET[i]: every O, and over the O's twice round G_SET - every (T, G) and every (O, G) pair occurs as long as
    G_SET has at most 2 len(O_SET) values; the family rotates over all cases"""
    assert len(G_SET) <= 2 * len(O_SET)
    out = []
    for j, o in enumerate(O_SET):
        for h in (0, 1):
            n = (i * len(O_SET) + j) * 2 + h
            out.append((FAMILIES[n % len(FAMILIES)], T_SET[i], o, G_SET[(2 * (i + j) + h) % len(G_SET)], n))
    return out


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "these tests need the GPU"
    return torch.device("cuda:0")


def _on(c, dev):
    return {k: (v.to(dev) if torch.is_tensor(v) else v) for k, v in c.items()}


def _bits(x):
    """fp16 -> int16 patterns, every NaN one value"""
    return x.masked_fill(torch.isnan(x), 0).view(torch.int16), torch.isnan(x)


def _same_bits(x, y):
    (xb, xn), (yb, yn) = _bits(x), _bits(y)
    return bool(torch.equal(xn, yn)) and bool(torch.equal(xb, yb))


def _images(c):
    from fpqvar_amd import gemm
    return (gemm.to_kmajor(c["a"], 4), gemm.to_kmajor_scales(c["a_scales"]), gemm.to_kmajor(c["w"], 4, dealt=True),
            gemm.to_kmajor_scales(c["w_scales"], weight_side=True))


def _mx(ops, bias, out, km, gate=None, resid=None, rows_per_gate=1):
    """fpq_gemm_fp4_mx_ex / _km straight through the C ABI into `out` (the residual may BE the output, which the Python wrappers
    never arrange)"""
    a, asc, w, wsc = ops
    T, O = out.shape
    K = (a.shape[0] * 128) if km else a.shape[1] * 2
    ep = None
    if gate is not None or resid is not None:
        ep = _lib.GemmEpilogue(None if gate is None else gate.data_ptr(), None if resid is None else resid.data_ptr(), rows_per_gate)
    fn = _lib.lib().fpq_gemm_fp4_mx_km if km else _lib.lib().fpq_gemm_fp4_mx_ex
    _lib.check(fn(a.data_ptr(), asc.data_ptr(), w.data_ptr(), wsc.data_ptr(), _lib.dtype_id(wsc.dtype), None if bias is None else bias.data_ptr(),
                  out.data_ptr(), T, O, K, None if ep is None else ctypes.byref(ep), _lib.stream_ptr(out.device)), "fpq_gemm_fp4_mx")
    return out


@pytest.mark.parametrize("ti", range(len(T_SET)))
def test_ring_equals_cfg30_the_model_and_the_reference(dev, ti, lib_options):
    """Pairwise over T x O x G, the families in rotation, fp32 weight scales everywhere and fp16 ones on every other case
    (row-major: the k-major scale image is fp32).  At cfg 40, row-major and k-major: bit-equal to cfg 30, bit-equal to
    gm.emulate(..., "lds"), inside gm.reference's bound with the exact non-finite pattern.  Then with bias + gate + residual, the
    residual aliasing the output: bit-equal to cfg 30 and to the fp16 tail `residual + y * gate` of the model's y (each
    operation rounded once, as the epilogue does it) - exact fp16 operations on a y that the first half held to the bound."""
    from fpqvar_amd import gemm
    bad = []
    for family, T, O, G, n in _cases(ti):
        K = 128 * G
        c = _on(gm.make_case("fp4", family, T, O, K), dev)
        variants = [c["w_scales"]] + ([c["w_scales"].half()] if c["w_scales"].dtype == torch.float32 and n % 2 == 0 else [])
        for ws in variants:
            cv = dict(c, w_scales=ws)
            what = f"{family} T={T} O={O} G={G}" + (" w16" if ws.dtype == torch.float16 else "")
            rm = (cv["a"], cv["a_scales"], cv["w"], ws)
            layouts = [("row-major", rm, False)] + ([("k-major", _images(cv), True)] if ws.dtype == torch.float32 else [])
            r = gm.reference("fp4", *rm, cv["bias"])
            emu = gm.emulate("fp4", *rm, cv["bias"], "lds")
            # the tail's operands: a gate row per 3 tokens, values around 1; the residual of the output's size
            g = torch.Generator().manual_seed(n)
            bias_t = (torch.randn(O, generator=g) * 0.1).half().to(dev)
            gate = (1.0 + 0.25 * torch.randn((T + 2) // 3, O, generator=g)).half().to(dev)
            resid = torch.randn(T, O, generator=g).half().to(dev)
            emu_t = gm.emulate("fp4", *rm, bias_t, "lds")
            want_t = resid + emu_t * gate.repeat_interleave(3, dim=0)[:T]
            for name, ops, km in layouts:
                got = {}
                for cfg in (30, 40):
                    lib_options("FPQ_GEMM_CFG", cfg)
                    y = gemm.linear_fp4(*ops, cv["bias"], outs=O)
                    buf = resid.clone()
                    got[cfg] = (y, _mx(ops, bias_t, buf, km, gate, buf, 3))
                y30, t30 = got[30]
                y40, t40 = got[40]
                rat = gm.ratio(y40, r)
                print(f"{what} {name}: err / bound {rat:.3f}")
                if not rat <= 1.0:
                    bad.append((what, name, f"err / bound {rat}"))
                if not _same_bits(y40, y30):
                    bad.append((what, name, "cfg 40 differs from cfg 30"))
                if not _same_bits(y40, emu):
                    bad.append((what, name, "cfg 40 differs from emulate(lds)"))
                if not _same_bits(t40, t30):
                    bad.append((what, name, "tail: cfg 40 differs from cfg 30"))
                if not _same_bits(t40, want_t):
                    bad.append((what, name, "tail: cfg 40 differs from residual + emulate(lds) * gate"))
    assert not bad, f"{len(bad)} failures, first {bad[:8]}"


def _qkv_operands(dev, G, seed):
    from fpqvar_amd import gemm
    g = torch.Generator().manual_seed(seed)
    T, C, K = 130, 128, 128 * G
    x = (torch.randn(T, K, generator=g) * torch.exp(0.3 * torch.randn(T, K, generator=g))).half().to(dev)
    w = (torch.randn(3 * C, K, generator=g) * 0.05).to(dev)
    a, wq = gemm.quantize_mx(x), gemm.quantize_mx(w)
    a_km = (gemm.to_kmajor(a[0], 4), gemm.to_kmajor_scales(a[1]))
    w_km = (gemm.to_kmajor(wq[0], 4, dealt=True), gemm.to_kmajor_scales(wq[1], weight_side=True))
    return (a, wq), (a_km, w_km), g


@pytest.mark.parametrize("G", (S - 1, S + 1, 15))
@pytest.mark.parametrize("qk_norm", (False, True))
def test_qkv_to_cache(dev, G, qk_norm, lib_options):
    """linear_fp4_qkv_to_cache at T = 130 (two batch entries of 65 rows: tiles that straddle an entry), O = 384, both layouts: q and
    the cache - its untouched slots included - bit-equal to cfg 30's."""
    from fpqvar_amd import gemm
    rm, km, g = _qkv_operands(dev, G, 40 + G)
    bsz, seq, H, pos, max_len = 2, 65, 2, 3, 75
    if qk_norm:
        bias = (torch.randn(3 * 128, generator=g) * 0.1).to(dev)                   # fp32: added behind the fp16 rounding
        hs = torch.exp(torch.randn(H, generator=g) * 0.5).to(dev)
    else:
        bias, hs = (torch.randn(3 * 128, generator=g) * 0.1).half().to(dev), None
    for name, (a, w) in (("row-major", rm), ("k-major", km)):
        got = {}
        for cfg in (30, 40):
            lib_options("FPQ_GEMM_CFG", cfg)
            cache = torch.full((2, bsz, max_len, H, 64), 7.5, dtype=torch.float16, device=dev)
            q = gemm.linear_fp4_qkv_to_cache(*a, *w, bias, cache, pos, seq, qk_norm_scale=hs)
            got[cfg] = (q, cache)
        assert got[40][0].shape == (bsz, seq, 128)
        assert bool(got[30][0].float().abs().sum() > 0) and bool((got[30][1][:, :, pos:pos + seq] != 7.5).any()), name
        assert _same_bits(got[40][0], got[30][0]), f"{name}: q differs from cfg 30"
        assert _same_bits(got[40][1], got[30][1]), f"{name}: the cache differs from cfg 30"


def _fc1(ops, bias, T, O, K, km, flag, dev):
    a, asc, w, wsc = ops
    out = torch.empty(T, O, dtype=torch.float16, device=dev)
    h = torch.empty(T, O, dtype=torch.float16, device=dev)
    fn = _lib.lib().fpq_gemm_fp4_gelu_dual_km if km else _lib.lib().fpq_gemm_fp4_gelu_dual
    _lib.check(fn(a.data_ptr(), asc.data_ptr(), w.data_ptr(), wsc.data_ptr(), _lib.dtype_id(wsc.dtype), bias.data_ptr(), out.data_ptr(),
                  h.data_ptr(), T, O, K, flag.data_ptr(), _lib.stream_ptr(dev)), "fpq_gemm_fp4_gelu_dual")
    return out, h


@pytest.mark.parametrize("T,O", ((65, 256), (130, 384)))
@pytest.mark.parametrize("G", (S - 1, S + 1, 15))
def test_gelu_dual(dev, T, O, G, lib_options):
    """The fc1 form (its exchange area and row scales live in a stage buffer of the ring), both layouts: the quantized output and
    the GELU tensor bit-equal to cfg 30's.  At one shape a NaN activation scale in one row: the whole result is zero and the
    8-byte flag scratch is zero again afterwards."""
    from fpqvar_amd import gemm
    g = torch.Generator().manual_seed(T + G)
    K = 128 * G
    x = (torch.randn(T, K, generator=g) * torch.exp(0.3 * torch.randn(T, K, generator=g))).half().to(dev)
    w = (torch.randn(O, K, generator=g) * 0.05).to(dev)
    bias = (torch.randn(O, generator=g) * 0.3).half().to(dev)
    a, wq = gemm.quantize_mx(x), gemm.quantize_mx(w)
    flag = torch.zeros(2, dtype=torch.int32, device=dev)
    for nan_row in ((None, T - 2) if (T, G) == (130, S + 1) else (None,)):
        asc = a[1].clone()
        if nan_row is not None:
            asc[nan_row, G - 1] = math.nan
        rm = (a[0], asc, wq[0], wq[1])
        km = (gemm.to_kmajor(a[0], 4), gemm.to_kmajor_scales(asc), gemm.to_kmajor(wq[0], 4, dealt=True),
              gemm.to_kmajor_scales(wq[1], weight_side=True))
        for name, ops, is_km in (("row-major", rm, False), ("k-major", km, True)):
            got = {}
            for cfg in (30, 40):
                lib_options("FPQ_GEMM_CFG", cfg)
                got[cfg] = _fc1(ops, bias, T, O, K, is_km, flag, dev)
                torch.cuda.synchronize()
                assert not bool(flag.any()), f"{name} cfg {cfg}: the flag scratch must be zero after the call"
            assert _same_bits(got[40][0], got[30][0]), f"{name}: the quantized output differs from cfg 30"
            assert _same_bits(got[40][1], got[30][1]), f"{name}: the GELU tensor differs from cfg 30"
            if nan_row is None:
                assert bool(got[40][0].view(torch.int16).any()), name
            else:
                assert bool(torch.isnan(got[40][1][nan_row]).all()) and not bool(torch.isnan(got[40][1][:nan_row]).any()), name
                assert not bool(got[40][0].view(torch.int16).any()), f"{name}: a NaN in one row must zero the whole result"


@pytest.mark.parametrize("T,O,K,km", ((130, 392, 2304, False), (130, 392, 2304, True), (100, 5760, 1920, False), (100, 5760, 1920, True)))
def test_timing_sensitivity_screen(dev, T, O, K, km, lib_options):
    """A read placed in front of the wait that retires its stage is right whenever the DMA lands first.  Eight distinct operand
    sets, used in rotation so that a launch's inputs are not the ones just read, 200 launches of cfg 40 back to back on one
    stream, each into its own output: every output bit-equal to cfg 30's for its set.  One pass, not retried."""
    sets, want = [], []
    lib_options("FPQ_GEMM_CFG", 30)
    for s in range(8):
        c = _on(gm.make_case("fp4", "gauss", T, O, K, seed=s + 1), dev)
        ops = _images(c) if km else (c["a"], c["a_scales"], c["w"], c["w_scales"])
        sets.append((ops, c["bias"]))
        want.append(_mx(ops, c["bias"], torch.empty(T, O, dtype=torch.float16, device=dev), km))
    assert not _same_bits(want[0], want[1])
    lib_options("FPQ_GEMM_CFG", 40)
    outs = torch.full((200, T, O), math.nan, dtype=torch.float16, device=dev)
    torch.cuda.synchronize()
    for i in range(200):
        ops, bias = sets[i % 8]
        _mx(ops, bias, outs[i], km)
    torch.cuda.synchronize()
    wrong = [i for i in range(200) if not _same_bits(outs[i], want[i % 8])]
    assert not wrong, f"{len(wrong)} of 200 launches differ from cfg 30, first {wrong[:8]}"


@pytest.mark.parametrize("T,O,K", ((130, 392, 1024), (2600, 2560, 256)))
@pytest.mark.parametrize("table", ("e3m0", "e1m2"))
def test_a6w4_reads_40_as_not_set(dev, T, O, K, table, lib_options):
    """The A6W4 GEMM has no ring kernel: FPQ_GEMM_CFG = 40 gives the bits of the unset switch (where the default is the 64 x 128
    tile and where it is the 128 x 128 one)."""
    from fpqvar_amd import gemm
    g = torch.Generator().manual_seed(K + O)
    x = torch.randn(T, K, generator=g).half().to(dev)
    w4 = gemm.quantize_mx((torch.randn(O, K, generator=g) * 0.05).to(dev))
    bias = (torch.randn(O, generator=g) * 0.3).half().to(dev)
    a6 = gemm.quantize_g6(x, table)
    lib_options("FPQ_GEMM_CFG", None)
    want = gemm.linear_a6w4(*a6, table, *w4, bias)
    lib_options("FPQ_GEMM_CFG", 40)
    got = gemm.linear_a6w4(*a6, table, *w4, bias)
    assert bool(want.float().abs().sum() > 0) and _same_bits(got, want)
