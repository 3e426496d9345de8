"""mat_qkv on the A6W4 GEMM (fpq_gemm_a6w4_mx_split, fpq_gemm_a6w4_mx_split_qknorm; include/fpq.h): a 6-bit E3M0 / E1M2 activation
against the stored FP4 weight, q written to its own tensor and k, v straight into the KV cache's slots - bit-identical to the plain
A6W4 GEMM followed by the cache's copy-in; with the q / k L2 norm in the epilogue q and k sit within one fp16 ulp of the
reference's lines (tr/basic_var.py:176-183) in fp32 on the fp16 Linear output, v is bit for bit.  Row-major operands and k-major
images, both tilings.  The shapes are the smallest at which each mechanism of the store can fail, not the models' own."""
import functools

import pytest
import torch
import torch.nn.functional as Fn

pytestmark = pytest.mark.gpu

SHAPES = [(2, 1, 2), (3, 9, 2), (2, 25, 4), (5, 64, 2), (2, 169, 4), (3, 256, 2), (100, 1, 30), (7, 100, 30)]
TABLES = ["e3m0", "e1m2"]


def _dev():
    return torch.device("cuda:0")


# ---- the helpers of tests/test_gpu_qk_l2norm.py ---------------------------------------------------------------------------
def _ord(h):
    """fp16 -> integers in value order (the distance of two is their distance in ulps; +0 and -0 coincide)"""
    i = h.contiguous().view(torch.int16).int()
    return torch.where(i < 0, -(i & 0x7FFF), i)


def _assert_ulp(got, want, what, max_ulp=1):
    assert got.shape == want.shape and got.dtype == want.dtype == torch.float16, what
    d = (_ord(got) - _ord(want)).abs()
    n1 = int((d > 0).sum())
    assert not bool(torch.isnan(got).any()), f"{what}: NaN"
    assert int(d.max()) <= max_ulp, f"{what}: max {int(d.max())} ulp, {n1} of {d.numel()} elements off by >= 1 ulp"


def _reference(y, head_scale, heads):
    """tr/basic_var.py:176-183 in fp32 (flash layout) on y [B, L, 3C]: fp16 q, k, v as they leave for attention / the cache"""
    B, L = y.shape[0], y.shape[1]
    q, k, v = y.view(B, L, 3, heads, 64).unbind(2)
    q = Fn.normalize(q, dim=-1).mul(head_scale.view(1, 1, heads, 1))
    k = Fn.normalize(k, dim=-1)
    return q.half(), k.half(), v.half()


def _scale_mul(heads, seed):
    g = torch.Generator().manual_seed(seed)
    sm = torch.full((1, heads, 1, 1), 4.0).log() + 0.3 * torch.randn(1, heads, 1, 1, generator=g)
    sm[0, 0] = 5.5   # > log 100: clamped
    return sm.to(_dev())


def _bias32(c, seed):
    g = torch.Generator().manual_seed(seed)
    b = torch.randn(3 * c, generator=g) * 0.1
    b[c:2 * c] = 0   # zero_k_bias
    return b.to(_dev())


def _bits(t):
    return t.contiguous().view(torch.int16)


# ---- operands: as tests/test_gpu_qkv_split.py builds its own, the activation through quantize_g6, C = K = 64 * heads -------
@functools.lru_cache(maxsize=None)
def _problem(tokens, c, table, seed, zero_head=None):
    """x, the row-major and k-major operand forms of (x, w), the fp16 bias and the plain GEMM's outputs with and without it -
    computed once per shape and table, shared by every case that needs them, never written to"""
    from fpqvar_amd import gemm
    torch.manual_seed(seed)
    x = torch.randn(tokens, c, device=_dev()).half()
    w = torch.randn(3 * c, c, device=_dev()) * 0.05
    if zero_head is not None:   # all weight rows of one head of q and of k are zero
        w[zero_head * 64:(zero_head + 1) * 64] = 0
        w[c + zero_head * 64:c + (zero_head + 1) * 64] = 0
    bias = (torch.randn(3 * c, device=_dev()) * 0.1).half()
    wq = gemm.quantize_mx(w)
    a = gemm.quantize_g6(x, table)
    a_km = gemm.quantize_g6(x, table, kmajor=True)
    w_km = (gemm.to_kmajor(wq[0], 4, dealt=True), gemm.to_kmajor_scales(wq[1], weight_side=True))
    return dict(a={False: a, True: a_km}, w={False: wq, True: w_km}, bias=bias,
                y_bias=gemm.linear_a6w4(*a, table, *wq, bias), y16=gemm.linear_a6w4(*a, table, *wq, None))


def _untouched_is(cache, pos, seq, value):
    untouched = torch.ones(cache.shape[2], dtype=torch.bool, device=cache.device)
    untouched[pos:pos + seq] = False
    return bool((cache[:, :, untouched] == value).all())


# ---- 1. the split output == the plain GEMM + the copy, bit for bit -------------------------------------------------------
@pytest.mark.parametrize("bsz,seq,heads", SHAPES)
@pytest.mark.parametrize("table", TABLES)
@pytest.mark.parametrize("kmajor", [False, True])
@pytest.mark.parametrize("cfg", [None, 20, 30])
@pytest.mark.parametrize("with_bias", [True, False])
def test_qkv_to_cache_equals_plain_gemm_plus_copy(bsz, seq, heads, table, kmajor, cfg, with_bias, lib_options):
    from fpqvar_amd import gemm
    c, max_len, pos = heads * 64, seq + 37, 11
    p = _problem(bsz * seq, c, table, bsz * seq + heads)
    a, w, bias = p["a"][kmajor], p["w"][kmajor], p["bias"] if with_bias else None
    if kmajor:   # the reference of this case is the k-major plain GEMM (bit-equal to the row-major one: tests/test_gpu_a6w4_km.py)
        qkv = gemm.linear_a6w4_km(*a, table, *w, bias, outs=3 * c)
        assert torch.equal(qkv, p["y_bias" if with_bias else "y16"])
    else:
        qkv = p["y_bias" if with_bias else "y16"]
    if cfg is not None:
        lib_options("FPQ_GEMM_CFG", cfg)
    want_q, want_k, want_v = qkv.view(bsz, seq, 3, heads, 64).unbind(2)
    cache = torch.full((2, bsz, max_len, heads, 64), 7.5, dtype=torch.float16, device=_dev())
    q = gemm.linear_a6w4_qkv_to_cache(*a, table, *w, bias, cache, pos, seq)
    assert q.shape == (bsz, seq, c) and torch.equal(q.view(bsz, seq, heads, 64), want_q)
    assert torch.equal(cache[0, :, pos:pos + seq], want_k) and torch.equal(cache[1, :, pos:pos + seq], want_v)
    assert _untouched_is(cache, pos, seq, 7.5), "the GEMM wrote outside its slots"


# ---- 2. the q / k norm in that epilogue ------------------------------------------------------------------------------------
_NORM_SEEN = {}   # (shape, table, bias) -> the (q, cache) of the first (layout, tiling) that ran: every other one must give the same bits


@pytest.mark.parametrize("bsz,seq,heads", SHAPES)
@pytest.mark.parametrize("table", TABLES)
@pytest.mark.parametrize("kmajor", [False, True])
@pytest.mark.parametrize("cfg", [None, 20, 30])
@pytest.mark.parametrize("with_bias", [False, True])
def test_split_gemm_with_qk_norm(bsz, seq, heads, table, kmajor, cfg, with_bias, lib_options):
    """q and k within one fp16 ulp of the fp32 reference, v bit for bit; and row-major against k-major, FPQ_GEMM_CFG 20 against 30
    (and against the default): bit-identical to each other"""
    from fpqvar_amd import gemm, kv_cache
    c, max_len, pos = heads * 64, seq + 37, 11
    p = _problem(bsz * seq, c, table, bsz * seq + heads)
    bias = _bias32(c, heads + seq) if with_bias else None
    hs = kv_cache.qk_norm_head_scale(_scale_mul(heads, seq))
    y = p["y16"].float().view(bsz, seq, 3 * c) + (bias if with_bias else 0.0)
    want_q, want_k, want_v = _reference(y, hs, heads)
    if cfg is not None:
        lib_options("FPQ_GEMM_CFG", cfg)
    cache = torch.full((2, bsz, max_len, heads, 64), 7.5, dtype=torch.float16, device=_dev())
    q = gemm.linear_a6w4_qkv_to_cache(*p["a"][kmajor], table, *p["w"][kmajor], bias, cache, pos, seq, qk_norm_scale=hs)
    assert q.shape == (bsz, seq, c)
    _assert_ulp(q.view(bsz, seq, heads, 64), want_q, "q")
    _assert_ulp(cache[0, :, pos:pos + seq], want_k, "k")
    assert torch.equal(_bits(cache[1, :, pos:pos + seq]), _bits(want_v)), "v not bit-exact"
    assert _untouched_is(cache, pos, seq, 7.5), "the GEMM wrote outside its slots"
    first = _NORM_SEEN.setdefault((bsz, seq, heads, table, with_bias), (kmajor, cfg, q, cache))
    assert torch.equal(_bits(q), _bits(first[2])) and torch.equal(_bits(cache), _bits(first[3])), \
        f"kmajor={kmajor} cfg={cfg} differs from kmajor={first[0]} cfg={first[1]}"


@pytest.mark.parametrize("table", TABLES)
@pytest.mark.parametrize("kmajor", [False, True])
def test_split_gemm_edge_rows(table, kmajor):
    """a head whose q / k weight rows are all zero: exact zeros without bias, the eps branch with a tiny bias; a head whose
    scale_mul_1H11 exceeds log 100 is clamped to 100"""
    from fpqvar_amd import gemm, kv_cache
    bsz, seq, heads = 3, 20, 4
    c = heads * 64
    p = _problem(bsz * seq, c, table, 5, 1)
    a, w, y16 = p["a"][kmajor], p["w"][kmajor], p["y16"]
    sm = _scale_mul(heads, 1)
    hs = kv_cache.qk_norm_head_scale(sm)
    assert float(sm[0, 0]) > kv_cache.MAX_SCALE_MUL and abs(float(hs[0]) - 100.0) < 1e-4
    cache = torch.zeros(2, bsz, seq, heads, 64, dtype=torch.float16, device=_dev())
    q = gemm.linear_a6w4_qkv_to_cache(*a, table, *w, None, cache, 0, seq, qk_norm_scale=hs).view(bsz, seq, heads, 64)
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
    q = gemm.linear_a6w4_qkv_to_cache(*a, table, *w, bias, cache, 0, seq, qk_norm_scale=hs).view(bsz, seq, heads, 64)
    want_q, want_k, _ = _reference(y16.float().view(bsz, seq, 3 * c) + bias, hs, heads)
    assert float(want_k[:, :, 1].float().abs().max()) > 0.005   # the eps branch: y / 1e-12
    _assert_ulp(q, want_q, "q (tiny norm)")
    _assert_ulp(cache[0], want_k, "k (tiny norm)")


# ---- 3. five generation steps ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kmajor", [False, True])
def test_incremental_cache_commit_written_equals_append(kmajor):
    """five steps of a generation on two caches: append(k, v) against the split GEMM + commit_written - same views at every step,
    same cache contents and length at the end"""
    from fpqvar_amd import kv_cache
    from fpqvar_amd import gemm
    bsz, heads, c = 3, 4, 256
    steps = (1, 4, 9, 16, 25)
    ca = kv_cache.IncrementalKVCache(bsz, sum(steps), heads, 64, 6, device=_dev())
    cb = kv_cache.IncrementalKVCache(bsz, sum(steps), heads, 64, 6, device=_dev())
    ca.kv.zero_()
    cb.kv.zero_()
    for i, seq in enumerate(steps):
        p = _problem(bsz * seq, c, "e3m0", 100 + i)
        _, k, v = p["y_bias"].view(bsz, seq, 3, heads, 64).unbind(2)
        ka, va = ca.append(k, v)
        gemm.linear_a6w4_qkv_to_cache(*p["a"][kmajor], "e3m0", *p["w"][kmajor], p["bias"], cb.kv, cb.len, seq)
        kb, vb = cb.commit_written(seq)
        assert torch.equal(ka, kb) and torch.equal(va, vb), i
    assert torch.equal(ca.kv, cb.kv) and ca.len == cb.len == sum(steps)


# ---- 4. FP4Linear.qkv_to_cache: one call for every activation format ---------------------------------------------------------
@pytest.mark.parametrize("act", ["fp_e2", "fp_e3", "fp_e1"])
@pytest.mark.parametrize("kmajor", [False, True])
def test_fp4linear_qkv_to_cache(act, kmajor):
    from fpqvar_amd import gemm, kv_cache
    bsz, seq, heads, c = 3, 9, 4, 256
    torch.manual_seed(7)
    lin = torch.nn.Linear(c, 3 * c).to(_dev())
    kw = dict(a6w4_kmajor=True) if kmajor and act != "fp_e2" else {}
    mod = gemm.FP4Linear.from_float(lin, kmajor=kmajor, act_fp_type=act, **kw)
    assert mod.kmajor == kmajor
    x = torch.randn(bsz, seq, c, device=_dev()).half()
    max_len, pos = seq + 5, 3
    # without the norm: forward(x) unbound into q, k, v plus the copy, bit for bit
    want_q, want_k, want_v = mod(x).view(bsz, seq, 3, heads, 64).unbind(2)
    cache = torch.full((2, bsz, max_len, heads, 64), 7.5, dtype=torch.float16, device=_dev())
    q = mod.qkv_to_cache(x, cache, pos, seq)
    assert q.shape == (bsz, seq, c) and torch.equal(_bits(q.view(bsz, seq, heads, 64)), _bits(want_q))
    assert torch.equal(_bits(cache[0, :, pos:pos + seq]), _bits(want_k)) and torch.equal(_bits(cache[1, :, pos:pos + seq]), _bits(want_v))
    assert _untouched_is(cache, pos, seq, 7.5)
    # with the norm: the matching linear_*_qkv_to_cache called directly on the module's operands
    lin.bias = None
    mod = gemm.FP4Linear.from_float(lin, kmajor=kmajor, act_fp_type=act, **kw)
    hs = kv_cache.qk_norm_head_scale(_scale_mul(heads, 3))
    x2 = x.reshape(-1, c)
    for bias in (None, _bias32(c, 2)):
        c_want = torch.full_like(cache, 7.5)
        if act == "fp_e2":
            q_want = gemm.linear_fp4_qkv_to_cache(*gemm.quantize_mx(x2, kmajor=kmajor), mod.w_codes, mod.w_scales, bias, c_want, pos, seq, hs)
        else:
            q_want = gemm.linear_a6w4_qkv_to_cache(*gemm.quantize_g6(x2, mod.act_table, kmajor=kmajor), mod.act_table, mod.w_codes, mod.w_scales,
                                                   bias, c_want, pos, seq, hs)
        c_got = torch.full_like(cache, 7.5)
        q_got = mod.qkv_to_cache(x, c_got, pos, seq, qk_norm_scale=hs, bias=bias)
        assert torch.equal(_bits(q_got), _bits(q_want)) and torch.equal(_bits(c_got), _bits(c_want))
        assert _untouched_is(c_got, pos, seq, 7.5)


# ---- 5. a PackedKVCache staging slab as the destination --------------------------------------------------------------------
@pytest.mark.parametrize("kmajor", [False, True])
def test_staging_slab_as_destination(kmajor):
    from fpqvar_amd import gemm, kv_cache
    bsz, heads, c, steps = 3, 4, 256, (4, 9)
    staging = kv_cache.PackedKVCache.new_staging(bsz, max(steps), heads, device=_dev())
    pa = kv_cache.PackedKVCache(bsz, sum(steps), heads, 64, 6, _dev())
    pb = kv_cache.PackedKVCache(bsz, sum(steps), heads, 64, 6, _dev(), staging)
    for i, seq in enumerate(steps):
        p = _problem(bsz * seq, c, "e3m0", 300 + i)
        q, k, v = p["y_bias"].view(bsz, seq, 3, heads, 64).unbind(2)
        want = pa.attend(q, k, v, 0.125)
        staging.fill_(float("nan"))
        qb = gemm.linear_a6w4_qkv_to_cache(*p["a"][kmajor], "e3m0", *p["w"][kmajor], p["bias"], pb.staging, 0, seq).view(bsz, seq, heads, 64)
        got = pb.attend_staged(qb, seq, 0.125)
        assert torch.equal(_bits(qb), _bits(q)) and torch.equal(_bits(got), _bits(want)), i
    assert pa.len == pb.len == sum(steps)


# ---- 6. rejections on device tensors ---------------------------------------------------------------------------------------
def test_rejections_on_device_tensors():
    from fpqvar_amd import gemm, kv_cache
    bsz, seq, heads = 2, 9, 2
    c = heads * 64
    hs = kv_cache.qk_norm_head_scale(_scale_mul(heads, 0))
    for kmajor in (False, True):
        p = _problem(bsz * seq, c, "e3m0", 1)
        a, w = p["a"][kmajor], p["w"][kmajor]
        cache = torch.full((2, bsz, 20, heads, 64), 7.5, dtype=torch.float16, device=_dev())
        with pytest.raises(RuntimeError):
            gemm.linear_a6w4_qkv_to_cache(*a, "e3m0", *w, None, cache, 12, seq)            # 12 + 9 > max_len
        with pytest.raises(RuntimeError):
            gemm.linear_a6w4_qkv_to_cache(*a, "e3m0", *w, None, cache[:, :, :10], 0, seq)   # a view that is not contiguous
        with pytest.raises(RuntimeError):
            gemm.linear_a6w4_qkv_to_cache(*a, "e3m0", *w, None, cache.float(), 0, seq)
        with pytest.raises(RuntimeError):                                                     # qk_norm_scale of the wrong length
            gemm.linear_a6w4_qkv_to_cache(*a, "e3m0", *w, None, cache, 0, seq, qk_norm_scale=torch.ones(heads + 1, device=_dev()))
        with pytest.raises(RuntimeError):                                                     # fp16 weight scales: not compiled
            gemm.linear_a6w4_qkv_to_cache(*p["a"][False], "e3m0", p["w"][False][0], p["w"][False][1].half(), None, cache, 0, seq)
        assert bool((cache == 7.5).all()), "a refused call wrote to the cache"
