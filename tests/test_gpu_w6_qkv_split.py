"""mat_qkv on the W6 GEMM (fpq_gemm_w6_mx_split, fpq_gemm_w6_mx_split_qknorm; include/fpq.h): an E1M2 / E3M0 WEIGHT as 6-bit codes
against any FP4 activation format, q written to its own tensor and k, v straight into the KV cache's slots - bit-identical to the
plain W6 GEMM followed by the cache's copy-in; with the q / k L2 norm in the epilogue q and k sit within one fp16 ulp of the
reference's lines (tr/basic_var.py:176-183) in fp32 on the fp16 Linear output (the contract tests/test_gpu_a6w4_qkv_split.py states
for this epilogue: its _reference and _assert_ulp), v is bit for bit, and on weights whose levels E2M1 holds too the whole launch
equals the E2M1-weight kernels' bit for bit.  After tests/test_gpu_a6w4_qkv_split.py; the shapes are the smallest at which each
mechanism of the store can fail, not the models' own."""
import functools

import pytest
import torch

from tests import w6_model as wm
from tests.test_gpu_a6w4_qkv_split import _assert_ulp, _bias32, _bits, _reference, _scale_mul, _untouched_is
from tests.test_gpu_w6_fc1 import FP_NAME, _quantize_a, common_level_weight

pytestmark = pytest.mark.gpu

SHAPES = [(2, 1, 2), (3, 9, 2), (2, 25, 4), (5, 64, 2), (2, 169, 4), (7, 100, 30)]
PAIRS = wm.PAIRS
IDS = [f"{a}-{w}" for a, w in PAIRS]
CFGS = (20, 30, None)


def _dev():
    return torch.device("cuda:0")


@functools.lru_cache(maxsize=None)
def _problem(tokens, c, pair, seed, zero_head=None):
    """the operands of (x, w) for the pair, the fp16 bias and the plain GEMM's outputs with and without it - computed once per shape
    and pair, shared by every case that needs them, never written to"""
    from fpqvar_amd import gemm
    a_table, w_table = pair
    torch.manual_seed(seed)
    x = torch.randn(tokens, c, device=_dev()).half()
    w = torch.randn(3 * c, c, device=_dev()) * 0.05
    if zero_head is not None:   # all weight rows of one head of q and of k are zero
        w[zero_head * 64:(zero_head + 1) * 64] = 0
        w[c + zero_head * 64:c + (zero_head + 1) * 64] = 0
    bias = (torch.randn(3 * c, device=_dev()) * 0.1).half()
    a, wq = _quantize_a(a_table, x), gemm.quantize_g6(w.float(), w_table)
    return dict(a=a, w=wq, bias=bias, y_bias=gemm.linear_w6(*a, a_table, *wq, w_table, bias), y16=gemm.linear_w6(*a, a_table, *wq, w_table, None))


# ---- 1. the split output == the plain GEMM + the copy, bit for bit -------------------------------------------------------
@pytest.mark.parametrize("bsz,seq,heads", SHAPES)
@pytest.mark.parametrize("pair", PAIRS, ids=IDS)
def test_qkv_to_cache_equals_plain_gemm_plus_copy(bsz, seq, heads, pair, lib_options):
    from fpqvar_amd import gemm
    a_table, w_table = pair
    c, max_len, pos = heads * 64, seq + 37, 11
    p = _problem(bsz * seq, c, pair, bsz * seq + heads)
    for cfg in CFGS:
        lib_options("FPQ_GEMM_CFG", cfg)
        for with_bias in (True, False):
            qkv = p["y_bias" if with_bias else "y16"]
            want_q, want_k, want_v = qkv.view(bsz, seq, 3, heads, 64).unbind(2)
            cache = torch.full((2, bsz, max_len, heads, 64), 7.5, dtype=torch.float16, device=_dev())
            q = gemm.linear_w6_qkv_to_cache(*p["a"], a_table, *p["w"], w_table, p["bias"] if with_bias else None, cache, pos, seq)
            what = f"cfg {cfg} bias {with_bias}"
            assert q.shape == (bsz, seq, c) and torch.equal(_bits(q.view(bsz, seq, heads, 64)), _bits(want_q)), what
            assert torch.equal(_bits(cache[0, :, pos:pos + seq]), _bits(want_k)), what
            assert torch.equal(_bits(cache[1, :, pos:pos + seq]), _bits(want_v)), what
            assert _untouched_is(cache, pos, seq, 7.5), f"{what}: the GEMM wrote outside its slots"


# ---- 2. the q / k norm in that epilogue ------------------------------------------------------------------------------------
@pytest.mark.parametrize("bsz,seq,heads", SHAPES)
@pytest.mark.parametrize("pair", PAIRS, ids=IDS)
@pytest.mark.parametrize("with_bias", [False, True])
def test_split_gemm_with_qk_norm(bsz, seq, heads, pair, with_bias, lib_options):
    """q and k within one fp16 ulp of the fp32 reference, v bit for bit; FPQ_GEMM_CFG 20, 30 and the default bit-identical to each other"""
    from fpqvar_amd import gemm, kv_cache
    a_table, w_table = pair
    c, max_len, pos = heads * 64, seq + 37, 11
    p = _problem(bsz * seq, c, pair, bsz * seq + heads)
    bias = _bias32(c, heads + seq) if with_bias else None
    hs = kv_cache.qk_norm_head_scale(_scale_mul(heads, seq))
    y = p["y16"].float().view(bsz, seq, 3 * c) + (bias if with_bias else 0.0)
    want_q, want_k, want_v = _reference(y, hs, heads)
    first = None
    for cfg in CFGS:
        lib_options("FPQ_GEMM_CFG", cfg)
        cache = torch.full((2, bsz, max_len, heads, 64), 7.5, dtype=torch.float16, device=_dev())
        q = gemm.linear_w6_qkv_to_cache(*p["a"], a_table, *p["w"], w_table, bias, cache, pos, seq, qk_norm_scale=hs)
        assert q.shape == (bsz, seq, c)
        _assert_ulp(q.view(bsz, seq, heads, 64), want_q, f"q (cfg {cfg})")
        _assert_ulp(cache[0, :, pos:pos + seq], want_k, f"k (cfg {cfg})")
        assert torch.equal(_bits(cache[1, :, pos:pos + seq]), _bits(want_v)), "v not bit-exact"
        assert _untouched_is(cache, pos, seq, 7.5), "the GEMM wrote outside its slots"
        if first is None:
            first = (cfg, q, cache)
        assert torch.equal(_bits(q), _bits(first[1])) and torch.equal(_bits(cache), _bits(first[2])), f"cfg={cfg} differs from cfg={first[0]}"


@pytest.mark.parametrize("bsz,seq,heads", SHAPES)
@pytest.mark.parametrize("pair", PAIRS, ids=IDS)
def test_common_levels_equal_the_e2m1_weight_kernels(bsz, seq, heads, pair, lib_options):
    """a weight of levels both tables hold (tests/test_gpu_w6_fc1.py): linear_w6_qkv_to_cache(qk_norm_scale=hs, bias=b32) is bit-equal to
    linear_fp4_qkv_to_cache / linear_a6w4_qkv_to_cache on the same problem expressed with an E2M1 weight - the W6 epilogue is the
    shipped one exactly; without the norm too"""
    from fpqvar_amd import gemm, kv_cache
    a_table, w_table = pair
    c, max_len, pos = heads * 64, seq + 5, 3
    tokens = bsz * seq
    torch.manual_seed(tokens + heads)
    a = _quantize_a(a_table, torch.randn(tokens, c, device=_dev()).half())
    w6, w4, sw = common_level_weight(_dev(), w_table, 3 * c, c, 17 + heads)
    hs = kv_cache.qk_norm_head_scale(_scale_mul(heads, seq))
    b32 = _bias32(c, heads + seq)
    b16 = (torch.randn(3 * c, device=_dev()) * 0.1).half()
    for norm in (True, False):
        bias, scale = (b32, hs) if norm else (b16, None)
        c_want = torch.full((2, bsz, max_len, heads, 64), 7.5, dtype=torch.float16, device=_dev())
        if a_table == "e2m1":
            q_want = gemm.linear_fp4_qkv_to_cache(*a, w4, sw, bias, c_want, pos, seq, scale)
        else:
            q_want = gemm.linear_a6w4_qkv_to_cache(*a, a_table, w4, sw, bias, c_want, pos, seq, scale)
        assert bool(q_want.any())
        for cfg in CFGS:
            lib_options("FPQ_GEMM_CFG", cfg)
            c_got = torch.full_like(c_want, 7.5)
            q_got = gemm.linear_w6_qkv_to_cache(*a, a_table, w6, sw, w_table, bias, c_got, pos, seq, scale)
            assert torch.equal(_bits(q_got), _bits(q_want)) and torch.equal(_bits(c_got), _bits(c_want)), f"norm {norm} cfg {cfg}"


# ---- 3. edge rows ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("pair", PAIRS, ids=IDS)
def test_split_gemm_edge_rows(pair):
    """a head whose q / k weight rows are all zero: exact zeros without bias, the eps branch with a tiny bias; a head whose
    scale_mul_1H11 exceeds log 100 is clamped to 100"""
    from fpqvar_amd import gemm, kv_cache
    a_table, w_table = pair
    bsz, seq, heads = 3, 20, 4
    c = heads * 64
    p = _problem(bsz * seq, c, pair, 5, 1)
    a, w, y16 = p["a"], p["w"], p["y16"]
    sm = _scale_mul(heads, 1)
    hs = kv_cache.qk_norm_head_scale(sm)
    assert float(sm[0, 0]) > kv_cache.MAX_SCALE_MUL and abs(float(hs[0]) - 100.0) < 1e-4
    cache = torch.zeros(2, bsz, seq, heads, 64, dtype=torch.float16, device=_dev())
    q = gemm.linear_w6_qkv_to_cache(*a, a_table, *w, w_table, None, cache, 0, seq, qk_norm_scale=hs).view(bsz, seq, heads, 64)
    assert bool((q[:, :, 1] == 0).all()) and bool((cache[0, :, :, 1] == 0).all()), "zero head: not exact zeros"
    assert not bool(torch.isnan(q).any() or torch.isnan(cache).any())
    want_q, want_k, _ = _reference(y16.float().view(bsz, seq, 3 * c), hs, heads)
    _assert_ulp(q, want_q, "q")
    _assert_ulp(cache[0], want_k, "k")
    nq = q[:, :, 0].float().norm(dim=-1)   # head 0 clamped to 100: its q rows have norm 100
    assert bool(((nq - 100).abs() < 0.2).all()), float((nq - 100).abs().max())
    # tiny bias on the zero head: norm < 1e-12, q = y / 1e-12 * s
    bias = torch.zeros(3 * c, device=_dev())
    bias[64:128] = torch.linspace(-3e-14, 4e-14, 64, device=_dev())
    bias[c + 64:c + 128] = torch.linspace(2e-14, -1e-14, 64, device=_dev())
    q = gemm.linear_w6_qkv_to_cache(*a, a_table, *w, w_table, bias, cache, 0, seq, qk_norm_scale=hs).view(bsz, seq, heads, 64)
    want_q, want_k, _ = _reference(y16.float().view(bsz, seq, 3 * c) + bias, hs, heads)
    assert float(want_k[:, :, 1].float().abs().max()) > 0.005   # the eps branch: y / 1e-12
    _assert_ulp(q, want_q, "q (tiny norm)")
    _assert_ulp(cache[0], want_k, "k (tiny norm)")


# ---- 4. FP4Linear.qkv_to_cache / qkv_to_cache_operands with w6_forms ------------------------------------------------------------
@pytest.mark.parametrize("pair", PAIRS, ids=IDS)
def test_fp4linear_qkv_to_cache_with_w6_forms(pair):
    from fpqvar_amd import gemm, kv_cache
    a_table, w_table = pair
    bsz, seq, heads, c = 3, 9, 4, 256
    torch.manual_seed(7)
    lin = torch.nn.Linear(c, 3 * c).to(_dev())
    kw = dict(act_fp_type=FP_NAME[a_table], weight_fp_type=FP_NAME[w_table], w6_forms=True)
    mod = gemm.FP4Linear.from_float(lin, **kw)
    assert mod.w6_forms and not mod.kmajor and (mod.act_table, mod.w_table) == pair
    x = torch.randn(bsz, seq, c, device=_dev()).half()
    x2 = x.reshape(-1, c)
    max_len, pos = seq + 5, 3
    # without the norm: the function-level call, which is forward(x) unbound into q, k, v plus the copy
    want_q, want_k, want_v = mod(x).view(bsz, seq, 3, heads, 64).unbind(2)
    c_want = torch.full((2, bsz, max_len, heads, 64), 7.5, dtype=torch.float16, device=_dev())
    ac, asc = _quantize_a(a_table, x2)
    q_want = gemm.linear_w6_qkv_to_cache(ac, asc, a_table, mod.w_codes, mod.w_scales, w_table, mod.bias, c_want, pos, seq)
    assert torch.equal(_bits(q_want.view(bsz, seq, heads, 64)), _bits(want_q)) and torch.equal(_bits(c_want[0, :, pos:pos + seq]), _bits(want_k))
    assert torch.equal(_bits(c_want[1, :, pos:pos + seq]), _bits(want_v))
    for call in (lambda cache: mod.qkv_to_cache(x, cache, pos, seq), lambda cache: mod.qkv_to_cache_operands(ac, asc, cache, pos, seq)):
        cache = torch.full_like(c_want, 7.5)
        q = call(cache)
        assert q.shape == (bsz, seq, c) and torch.equal(_bits(q), _bits(q_want)) and torch.equal(_bits(cache), _bits(c_want))
    # with the norm
    lin.bias = None
    mod = gemm.FP4Linear.from_float(lin, **kw)
    hs = kv_cache.qk_norm_head_scale(_scale_mul(heads, 3))
    for bias in (None, _bias32(c, 2)):
        c_want = torch.full_like(c_want, 7.5)
        q_want = gemm.linear_w6_qkv_to_cache(ac, asc, a_table, mod.w_codes, mod.w_scales, w_table, bias, c_want, pos, seq, hs)
        for call in (lambda cache: mod.qkv_to_cache(x, cache, pos, seq, qk_norm_scale=hs, bias=bias),
                     lambda cache: mod.qkv_to_cache_operands(ac, asc, cache, pos, seq, qk_norm_scale=hs, bias=bias)):
            c_got = torch.full_like(c_want, 7.5)
            q_got = call(c_got)
            assert torch.equal(_bits(q_got), _bits(q_want)) and torch.equal(_bits(c_got), _bits(c_want))
            assert _untouched_is(c_got, pos, seq, 7.5)
    # one step of a generation on two caches: append(k, v) against the split GEMM + commit_written
    ca = kv_cache.IncrementalKVCache(bsz, seq + 3, heads, 64, 6, device=_dev())
    cb = kv_cache.IncrementalKVCache(bsz, seq + 3, heads, 64, 6, device=_dev())
    ca.kv.zero_()
    cb.kv.zero_()
    _, k, v = mod(x).view(bsz, seq, 3, heads, 64).unbind(2)
    ka, va = ca.append(k, v)
    mod.qkv_to_cache(x, cb.kv, cb.len, seq)
    kb, vb = cb.commit_written(seq)
    assert torch.equal(_bits(ka), _bits(kb)) and torch.equal(_bits(va), _bits(vb))
    assert torch.equal(ca.kv, cb.kv) and ca.len == cb.len == seq
    # the default module still refuses
    with pytest.raises(ValueError):
        gemm.FP4Linear.from_float(lin, **{**kw, "w6_forms": False}).qkv_to_cache(x, cache, pos, seq)


# ---- 5. rejections on device tensors ---------------------------------------------------------------------------------------
def test_rejections_on_device_tensors():
    from fpqvar_amd import gemm, kv_cache
    bsz, seq, heads = 2, 9, 2
    c = heads * 64
    pair = ("e3m0", "e1m2")
    hs = kv_cache.qk_norm_head_scale(_scale_mul(heads, 0))
    p = _problem(bsz * seq, c, pair, 1)
    a, w = p["a"], p["w"]
    fn = lambda *rest, w_=w, **kw: gemm.linear_w6_qkv_to_cache(*a, "e3m0", *w_, "e1m2", *rest, **kw)
    cache = torch.full((2, bsz, 20, heads, 64), 7.5, dtype=torch.float16, device=_dev())
    with pytest.raises(RuntimeError):                                                     # fp16 weight scales: not compiled
        fn(None, cache, 0, seq, w_=(w[0], w[1].half()))
    with pytest.raises(RuntimeError):                                                     # a cache of the wrong width
        fn(None, torch.full((2, bsz, 20, heads + 2, 64), 7.5, dtype=torch.float16, device=_dev()), 0, seq)
    with pytest.raises(RuntimeError):
        fn(None, cache, 12, seq)                                                          # 12 + 9 > max_len
    with pytest.raises(RuntimeError):
        fn(None, cache[:, :, :10], 0, seq)                                                # a view that is not contiguous
    with pytest.raises(RuntimeError):                                                     # qk_norm_scale of the wrong length
        fn(None, cache, 0, seq, qk_norm_scale=torch.ones(heads + 1, device=_dev()))
    lin = torch.nn.Linear(c, 3 * c).to(_dev())
    mod = gemm.FP4Linear.from_float(lin, act_fp_type="fp_e3", weight_fp_type="fp_e1", w6_forms=True)
    with pytest.raises(RuntimeError, match="must have no bias"):                          # a module bias together with qk_norm_scale
        mod.qkv_to_cache(torch.zeros(bsz, seq, c, device=_dev()).half(), cache, 0, seq, qk_norm_scale=hs)
    assert bool((cache == 7.5).all()), "a refused call wrote to the cache"
