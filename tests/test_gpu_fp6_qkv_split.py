"""mat_qkv of a W6A6 attention block with a split output (fpq_gemm_fp6_rows_split) and with the q / k L2 norm in that epilogue
(fpq_gemm_fp6_rows_split_qknorm); gemm.linear_fp6_qkv_to_cache and GenerationBatch(config="w6a6", qkv_to_cache=True) on top.
Ground truth is never the code under test: the plain FP6 GEMM (gemm.linear_fp6, pinned to a float64 reference by
tests/test_gpu_gemm.py) for the fp16 Linear output, torch in fp32 for the reference's norm lines (include/fpq.h states the
contract: q and k within one fp16 ulp, v bit for bit), the oracle quantizer for the cache's entries."""
import ctypes

import pytest
import torch

from tests.test_gpu_qk_l2norm import CACHE_AGREEMENT, STEP_RMS, _assert_ulp, _bias, _oracle_quant, _reference, _scale_mul

pytestmark = pytest.mark.gpu

SHAPES = [(2, 1, 2), (3, 9, 2), (2, 25, 4), (5, 64, 2), (2, 169, 4), (3, 256, 2), (100, 1, 30), (7, 100, 30), (2, 2116, 4)]   # test_split_gemm_with_qk_norm's


def _dev():
    return torch.device("cuda:0")


def _operands(tokens, c, kmajor, seed, a_dtype=torch.float16, zero_head=None):
    """((a codes, a scales), (w codes, w scales), y16 = linear_fp6 of the row-major operands without bias, the row-major pair)"""
    from fpqvar_amd import gemm
    torch.manual_seed(seed)
    x = torch.randn(tokens, c, device=_dev()).to(a_dtype)
    w = torch.randn(3 * c, c, device=_dev()) * 0.05
    if zero_head is not None:   # all weight rows of one head of q and of k are zero
        w[zero_head * 64:(zero_head + 1) * 64] = 0
        w[c + zero_head * 64:c + (zero_head + 1) * 64] = 0
    a, wq = gemm.quantize_fp6(x), gemm.quantize_fp6(w)
    rm = (a, wq)
    if kmajor:
        a, wq = gemm.quantize_fp6(x, kmajor=True), (gemm.to_kmajor(wq[0], 6, dealt=True), wq[1])
    return a, wq, gemm.linear_fp6(*rm[0], *rm[1]), rm


def _untouched(cache, pos, seq, fill):
    keep = torch.ones(cache.shape[2], dtype=torch.bool, device=cache.device)
    keep[pos:pos + seq] = False
    return bool((cache[:, :, keep] == fill).all())


def _bits(t):
    return t.contiguous().view(torch.int16)


@pytest.mark.parametrize("bsz,seq,heads", SHAPES)
@pytest.mark.parametrize("kmajor", [False, True])
@pytest.mark.parametrize("cfg", [None, 0, 1])
@pytest.mark.parametrize("with_bias", [False, True])
@pytest.mark.parametrize("a_dtype", [torch.float16, torch.float32])
def test_split_gemm_exact(bsz, seq, heads, kmajor, cfg, with_bias, a_dtype, lib_options):
    """q and the cache's slots are, as bit patterns, the three column parts of linear_fp6 on the same operands"""
    from fpqvar_amd import gemm
    if cfg is not None:
        lib_options("FPQ_GEMM6_CFG", cfg)
    c, max_len, pos = heads * 64, seq + 37, 11
    a, w, _, rm = _operands(bsz * seq, c, kmajor, bsz * seq + heads, a_dtype)
    bias = (_bias(c, heads + seq) * 3).half() if with_bias else None
    want = gemm.linear_fp6(*rm[0], *rm[1], bias).view(bsz, seq, 3, heads, 64)
    cache = torch.full((2, bsz, max_len, heads, 64), 7.5, dtype=torch.float16, device=_dev())
    q = gemm.linear_fp6_qkv_to_cache(*a, *w, bias, cache, pos, seq)
    assert q.shape == (bsz, seq, c) and q.dtype == torch.float16
    assert torch.equal(_bits(q.view(bsz, seq, heads, 64)), _bits(want[:, :, 0])), "q"
    assert torch.equal(_bits(cache[0, :, pos:pos + seq]), _bits(want[:, :, 1])), "k"
    assert torch.equal(_bits(cache[1, :, pos:pos + seq]), _bits(want[:, :, 2])), "v"
    assert _untouched(cache, pos, seq, 7.5), "the GEMM wrote outside its slots"


def _split(c, n_parts, seq, dests):
    from fpqvar_amd._lib import GemmSplit
    sp = GemmSplit()
    sp.part_cols, sp.n_parts, sp.rows_per_batch = c, n_parts, seq
    for p, (ptr, stride, bstride, row0) in enumerate(dests):
        sp.out[p], sp.row_stride[p], sp.batch_stride[p], sp.row0[p] = ptr, stride, bstride, row0
    return sp


def test_split_gemm_wide_rows_through_the_c_abi():
    """row_stride > part_cols, destinations 8- but not 16-byte aligned: every part lands in its columns of wider rows, the
    columns beside them keep their fill"""
    from fpqvar_amd._lib import dtype_id, lib, stream_ptr
    bsz, seq, heads = 3, 20, 2
    c, stride, tokens = heads * 64, heads * 64 + 24, bsz * seq
    a, w, y16, _ = _operands(tokens, c, False, 9)
    bufs = [torch.full((bsz, seq + 2, stride), 7.5, dtype=torch.float16, device=_dev()) for _ in range(3)]
    sp = _split(c, 3, seq, [(b.data_ptr() + 8, stride, seq + 2, 1) for b in bufs])   # column 4 on, row 1 on
    rc = lib().fpq_gemm_fp6_rows_split(a[0].data_ptr(), a[1].data_ptr(), dtype_id(a[1].dtype), w[0].data_ptr(), w[1].data_ptr(),
                                       dtype_id(w[1].dtype), None, tokens, 3 * c, c, ctypes.byref(sp), 0, stream_ptr(_dev()))
    assert rc == 0
    want = y16.view(bsz, seq, 3, c)
    for p, b in enumerate(bufs):
        assert torch.equal(_bits(b[:, 1:seq + 1, 4:4 + c]), _bits(want[:, :, p])), f"part {p}"
        b[:, 1:seq + 1, 4:4 + c] = 7.5
        assert bool((b == 7.5).all()), f"part {p}: wrote outside its rows / columns"


@pytest.mark.parametrize("bsz,seq,heads", SHAPES)
@pytest.mark.parametrize("kmajor", [False, True])
@pytest.mark.parametrize("cfg", [None, 0, 1])
@pytest.mark.parametrize("with_bias", [False, True])
@pytest.mark.parametrize("a_dtype", [torch.float16, torch.float32])
def test_split_gemm_with_qk_norm(bsz, seq, heads, kmajor, cfg, with_bias, a_dtype, lib_options):
    from fpqvar_amd import gemm, kv_cache
    if cfg is not None:
        lib_options("FPQ_GEMM6_CFG", cfg)
    c, max_len, pos = heads * 64, seq + 37, 11
    a, w, y16, _ = _operands(bsz * seq, c, kmajor, bsz * seq + heads, a_dtype)
    bias = _bias(c, heads + seq) if with_bias else None
    hs = kv_cache.qk_norm_head_scale(_scale_mul(heads, seq))
    y = y16.float().view(bsz, seq, 3 * c) + (bias if with_bias else 0.0)
    want_q, want_k, want_v = _reference(y, hs, heads)
    cache = torch.full((2, bsz, max_len, heads, 64), 7.5, dtype=torch.float16, device=_dev())
    q = gemm.linear_fp6_qkv_to_cache(*a, *w, bias, cache, pos, seq, qk_norm_scale=hs)
    assert q.shape == (bsz, seq, c)
    _assert_ulp(q.view(bsz, seq, heads, 64), want_q, "q")
    _assert_ulp(cache[0, :, pos:pos + seq], want_k, "k")
    assert not bool(torch.isnan(cache[1, :, pos:pos + seq]).any())
    assert torch.equal(_bits(cache[1, :, pos:pos + seq]), _bits(want_v)), "v not bit-exact"
    assert _untouched(cache, pos, seq, 7.5), "the GEMM wrote outside its slots"


@pytest.mark.parametrize("kmajor", [False, True])
def test_split_gemm_edge_rows(kmajor):
    """a head whose q / k weight rows are all zero: exact zeros without bias, the eps branch with a tiny bias; a head whose
    scale_mul_1H11 exceeds log 100 is clamped to 100"""
    from fpqvar_amd import gemm, kv_cache
    bsz, seq, heads = 3, 20, 4
    c = heads * 64
    a, w, y16, _ = _operands(bsz * seq, c, kmajor, 5, zero_head=1)
    sm = _scale_mul(heads, 1)
    hs = kv_cache.qk_norm_head_scale(sm)
    assert float(sm[0, 0]) > kv_cache.MAX_SCALE_MUL and abs(float(hs[0]) - 100.0) < 1e-4
    cache = torch.zeros(2, bsz, seq, heads, 64, dtype=torch.float16, device=_dev())
    q = gemm.linear_fp6_qkv_to_cache(*a, *w, None, cache, 0, seq, qk_norm_scale=hs).view(bsz, seq, heads, 64)
    assert bool((q[:, :, 1] == 0).all()) and bool((cache[0, :, :, 1] == 0).all()), "zero head: not exact zeros"
    assert not bool(torch.isnan(q).any() or torch.isnan(cache).any())
    want_q, want_k, _ = _reference(y16.float().view(bsz, seq, 3 * c), hs, heads)
    _assert_ulp(q, want_q, "q")
    _assert_ulp(cache[0], want_k, "k")
    nq = q[:, :, 0].float().norm(dim=-1)   # head 0 clamped to 100: its q rows have norm 100
    assert bool(((nq - 100).abs() < 0.2).all()), float((nq - 100).abs().max())
    bias = torch.zeros(3 * c, device=_dev())   # tiny bias on the zero head: norm < 1e-12, q = y / 1e-12 * s
    bias[64:128] = torch.linspace(-3e-14, 4e-14, 64, device=_dev())
    bias[c + 64:c + 128] = torch.linspace(2e-14, -1e-14, 64, device=_dev())
    q = gemm.linear_fp6_qkv_to_cache(*a, *w, bias, cache, 0, seq, qk_norm_scale=hs).view(bsz, seq, heads, 64)
    want_q, want_k, _ = _reference(y16.float().view(bsz, seq, 3 * c) + bias, hs, heads)
    assert float(want_k[:, :, 1].float().abs().max()) > 0.005   # the eps branch: y / 1e-12
    _assert_ulp(q, want_q, "q (tiny norm)")
    _assert_ulp(cache[0], want_k, "k (tiny norm)")


def _pack_fp4(levels):
    """E2M1 level indices 0..15 [rows, K] -> the FP4 GEMM's nibble codes [rows, K / 2] (element 2j in the low nibble)"""
    return (levels[:, 0::2] | (levels[:, 1::2] << 4)).to(torch.uint8).contiguous()


def _pack_fp6(codes6):
    """6-bit codes [rows, K] -> the dense little-endian packing [rows, K * 3 / 4] (element j in bits 6j .. 6j + 5)"""
    c = codes6.to(torch.int32).view(codes6.shape[0], -1, 4)
    word = c[..., 0] | (c[..., 1] << 6) | (c[..., 2] << 12) | (c[..., 3] << 18)
    return torch.stack((word & 255, (word >> 8) & 255, (word >> 16) & 255), dim=-1).reshape(codes6.shape[0], -1).to(torch.uint8).contiguous()


# E2M1 level index (sign bit 3, magnitudes 0, 0.5, 1, 1.5, 2, 3, 4, 6) -> the E2M3 code of the same value (sign bit 5, exponent
# bias 1, three mantissa bits): 0.5 = 4/8 subnormal, 1 = 1.000 x 2^0, 1.5 = 1.100 x 2^0, 2, 3 = x 2^1, 4, 6 = x 2^2
_E2M1_AS_E2M3 = [0b000000, 0b000100, 0b001000, 0b001100, 0b010000, 0b010100, 0b011000, 0b011100]


def test_both_gemms_answer_one_contract():
    """Hand-built operands that are the same matrices for the FP4 and the FP6 GEMM (every E2M1 level is an E2M3 level, all
    scales 1, K = 128: every sum is exact in fp32): the two *_split_qknorm entry points write identical bits."""
    from fpqvar_amd import gemm, kv_cache
    bsz, seq, heads, K = 3, 50, 2, 128
    c, tokens = heads * 64, bsz * seq
    g = torch.Generator().manual_seed(4)
    la, lw = torch.randint(0, 16, (tokens, K), generator=g), torch.randint(0, 16, (3 * c, K), generator=g)
    table = torch.tensor(_E2M1_AS_E2M3)

    def to6(levels):
        return table[levels & 7] | ((levels >> 3) << 5)
    dev = _dev()
    a4, w4 = (_pack_fp4(la).to(dev), torch.ones(tokens, 1, dtype=torch.float16, device=dev)), (_pack_fp4(lw).to(dev), torch.ones(3 * c, 1, device=dev))
    a6, w6 = (_pack_fp6(to6(la)).to(dev), torch.ones(tokens, dtype=torch.float16, device=dev)), (_pack_fp6(to6(lw)).to(dev), torch.ones(3 * c, device=dev))
    da, dw = gemm.dequantize_mx(*a4), gemm.dequantize_mx(*w4)
    assert torch.equal(da, gemm.dequantize_fp6(*a6)) and torch.equal(dw, gemm.dequantize_fp6(*w6)), "the two operand pairs are not the same matrices"
    assert int(da.unique().numel()) == 15 and float((da @ dw.T).abs().max()) < 2 ** 24 / 4   # all levels; sums of quarters, exact in fp32
    assert torch.equal(gemm.linear_fp4(*a4, *w4), gemm.linear_fp6(*a6, *w6))
    hs = kv_cache.qk_norm_head_scale(_scale_mul(heads, 3))
    bias = _bias(c, 8)
    out = {}
    for name, fn, a, w in (("fp4", gemm.linear_fp4_qkv_to_cache, a4, w4), ("fp6", gemm.linear_fp6_qkv_to_cache, a6, w6)):
        cache = torch.zeros(2, bsz, seq + 3, heads, 64, dtype=torch.float16, device=dev)
        out[name] = (fn(*a, *w, bias, cache, 2, seq, qk_norm_scale=hs), cache)
    assert torch.equal(_bits(out["fp4"][0]), _bits(out["fp6"][0])), "q"
    assert torch.equal(_bits(out["fp4"][1][0]), _bits(out["fp6"][1][0])), "k"
    assert torch.equal(_bits(out["fp4"][1][1]), _bits(out["fp6"][1][1])), "v"
    assert float(out["fp6"][1][0].float().abs().max()) > 0


@pytest.mark.parametrize("kv_bit", [6, 4])
@pytest.mark.parametrize("l2", [False, True])
def test_generation_steps_quantize_what_was_emitted(kv_bit, l2):
    """five steps of linear_fp6_qkv_to_cache + commit_written: after each, the entries of the step before are the oracle
    quantizer applied to the fp16 values the GEMM emitted into the cache, bit for bit"""
    from fpqvar_amd import gemm, kv_cache
    B, H = 3, 4
    C = H * 64
    steps = (1, 4, 9, 16, 25)
    cache = kv_cache.IncrementalKVCache(B, sum(steps), H, 64, kv_bit, device=_dev())
    cache.kv.zero_()
    hs = kv_cache.qk_norm_head_scale(_scale_mul(H, 2)) if l2 else None
    bias = _bias(C, 3) if l2 else None
    emitted = None
    for i, seq in enumerate(steps):
        start = cache.len
        a, w, _, _ = _operands(B * seq, C, True, 200 + i)
        gemm.linear_fp6_qkv_to_cache(*a, *w, bias, cache.kv, cache.len, seq, qk_norm_scale=hs)
        kc, vc = cache.commit_written(seq)
        if emitted is not None:
            a0, b0, ek, ev = emitted
            for got, raw in ((kc[:, a0:b0], ek), (vc[:, a0:b0], ev)):
                want = _oracle_quant(raw, kv_bit)
                assert torch.equal(got.cpu().view(torch.int16), want.view(torch.int16)), f"step {i}: quantized entries differ from the oracle"
        emitted = (start, cache.len, cache.k[:, start:cache.len].clone(), cache.v[:, start:cache.len].clone())
        assert float(emitted[2].float().abs().max()) > 0
        if l2:
            nk = emitted[2].float().norm(dim=-1)
            assert bool(((nk - 1).abs() < 2e-3).all()), "cached k rows are not unit rows"


def _run(gb, path="Q", steps=6):
    caches = gb.new_caches(path)
    torch.manual_seed(0)
    gb.gen.manual_seed(11)
    ys = [gb.step(path, caches, gb.new_input(pn)) for pn in gb.patch_nums[:steps]]
    return ys, caches


def _batch(**kw):
    from fpqvar_amd import var_block
    return var_block.GenerationBatch("d30-256", "w6a6", depth=2, batch_rows=4, device="cuda:0", seed=3, **kw)


def _cache_bits(c):
    if hasattr(c, "codes"):   # PackedKVCache
        return torch.cat((c.codes[:, :, :c.len].reshape(-1), c.scales[:, :, :c.len].contiguous().view(torch.uint8).reshape(-1)))
    return c.kv[:, :, :c.len].contiguous().view(torch.uint8).reshape(-1)


@pytest.mark.parametrize("kv_storage,kmajor", [("fp16", True), ("fp16", False), ("codes", True)])
def test_generation_batch_split_equals_copy_in(kv_storage, kmajor):
    """without the norm the split form emits the values the copy-in form copies: step outputs and caches bit-identical"""
    outs = {form: _run(_batch(qkv_to_cache=form, kv_storage=kv_storage, kmajor=kmajor)) for form in (True, False)}
    for i, (y0, y1) in enumerate(zip(outs[True][0], outs[False][0])):
        assert torch.equal(_bits(y0), _bits(y1)), f"step {i} output"
    for b, (c0, c1) in enumerate(zip(outs[True][1], outs[False][1])):
        assert c0.len == c1.len and torch.equal(_cache_bits(c0), _cache_bits(c1)), f"block {b} cache"


@pytest.mark.parametrize("kv_storage", ["fp16", "codes"])
def test_generation_batch_split_norm_vs_torch_norm(kv_storage):
    """with attn_l2_norm: the norm in the GEMM's epilogue against the reference's torch lines between the existing kernels, under
    the two limits of tests/test_gpu_qk_l2norm.py (explained there)"""
    fused = _batch(attn_l2_norm=True, qk_norm="fused", kv_storage=kv_storage)
    assert fused.qkv_to_cache and fused.W6
    outs = {"fused": _run(fused), "torch": _run(_batch(attn_l2_norm=True, qk_norm="torch", kv_storage=kv_storage))}
    errs = [float((y0.float() - y1.float()).norm() / y1.float().norm()) for y0, y1 in zip(outs["fused"][0], outs["torch"][0])]
    print(f"w6a6 Q split, {kv_storage} cache: step output relative RMS error max {max(errs):.2e}")
    for y0 in outs["fused"][0]:
        assert torch.isfinite(y0).all()
    assert max(errs) <= STEP_RMS, errs
    if kv_storage == "fp16":   # (element-wise agreement is a statement about fp16 entries, not about packed bytes)
        agree = [float((c0.kv[:, :, :c0.len] == c1.kv[:, :, :c1.len]).float().mean()) for c0, c1 in zip(outs["fused"][1], outs["torch"][1])]
        print(f"w6a6 Q split, fp16 cache: cache agreement min {min(agree):.5f}")
        assert min(agree) >= CACHE_AGREEMENT, f"cache agreement {agree}"


@pytest.mark.parametrize("l2", [False, True])
def test_generation_batch_graphs_equal_eager(l2):
    gb = _batch(attn_l2_norm=l2)
    caches = gb.new_caches("Q")
    gb.gen.manual_seed(11)
    eager = [gb.step("Q", caches, gb.new_input(pn)).clone() for pn in gb.patch_nums]
    gb.gen.manual_seed(11)
    graphs, keep = gb.capture("Q")
    gb.replay(graphs)
    for i, (y0, (_, y1)) in enumerate(zip(eager, keep[1:])):
        assert torch.equal(_bits(y0), _bits(y1)), f"step {i}: replayed graph differs from the eager step"
    assert torch.equal(_cache_bits(caches[-1]), _cache_bits(keep[0][-1]))


def test_the_split_entry_point_runs(monkeypatch):
    """GenerationBatch(config="w6a6") reaches linear_fp6_qkv_to_cache once per block and step and mat_qkv no longer goes through
    linear_fp6; with qkv_to_cache=False it never does"""
    from fpqvar_amd import gemm
    calls = {"split": 0, "plain": 0}
    real_split, real_plain = gemm.linear_fp6_qkv_to_cache, gemm.linear_fp6

    def split(*a, **k):
        calls["split"] += 1
        return real_split(*a, **k)

    def plain(*a, **k):
        calls["plain"] += 1
        return real_plain(*a, **k)
    monkeypatch.setattr(gemm, "linear_fp6_qkv_to_cache", split)
    monkeypatch.setattr(gemm, "linear_fp6", plain)
    _run(_batch(attn_l2_norm=True), steps=3)
    assert calls == {"split": 6, "plain": 12}, calls   # per block and step: mat_qkv split; proj and fc1 plain
    calls.update(split=0, plain=0)
    _run(_batch(attn_l2_norm=True, qkv_to_cache=False), steps=3)
    assert calls == {"split": 0, "plain": 18}, calls


def test_argument_rejection():
    from fpqvar_amd import gemm, kv_cache
    bsz, seq, heads = 2, 9, 2
    c = heads * 64
    a, w, _, rm = _operands(bsz * seq, c, True, 1)
    hs = kv_cache.qk_norm_head_scale(_scale_mul(heads, 0))
    cache = torch.zeros(2, bsz, 20, heads, 64, dtype=torch.float16, device=_dev())
    f = gemm.linear_fp6_qkv_to_cache
    with pytest.raises(RuntimeError):   # cache dtype
        f(*a, *w, None, cache.float(), 0, seq)
    with pytest.raises(RuntimeError):   # cache rank
        f(*a, *w, None, cache[0], 0, seq)
    with pytest.raises(RuntimeError):   # cache device
        f(*a, *w, None, cache.cpu(), 0, seq)
    with pytest.raises(RuntimeError):   # pos + seq > max_len
        f(*a, *w, None, cache, 12, seq)
    with pytest.raises(RuntimeError):   # head_dim != 64 with the norm
        f(*a, *w, None, torch.zeros(2, bsz, 20, 1, 128, dtype=torch.float16, device=_dev()), 0, seq, qk_norm_scale=hs[:1])
    with pytest.raises(RuntimeError):   # fp16 bias where the norm needs fp32
        f(*a, *w, _bias(c, 0).half(), cache, 0, seq, qk_norm_scale=hs)
    with pytest.raises(RuntimeError):   # fp16 head scale
        f(*a, *w, None, cache, 0, seq, qk_norm_scale=hs.half())
    with pytest.raises(RuntimeError):   # a k-major activation image with row-major weight codes
        f(*a, *rm[1], None, cache, 0, seq)
    with pytest.raises(RuntimeError):   # a truncated scale vector
        f(a[0], a[1][:-1], *w, None, cache, 0, seq)
    assert bool((cache == 0).all()), "a rejected call wrote to the cache"
    # the packed cache's staging slab at pos 0, as GenerationBatch(kv_storage="codes") passes it
    staging = kv_cache.PackedKVCache.new_staging(bsz, 16, heads, 64, _dev())
    q = f(*a, *w, None, staging, 0, seq)
    want = gemm.linear_fp6(*rm[0], *rm[1]).view(bsz, seq, 3, heads, 64)
    assert torch.equal(_bits(staging[1, :, :seq]), _bits(want[:, :, 2])) and torch.equal(_bits(q.view(bsz, seq, heads, 64)), _bits(want[:, :, 0]))
