"""The q / k L2 norm of an attention block with attn_l2_norm=True (the released models' setting; tr/basic_var.py:160-183) in the
qkv-to-cache path: the FP4 GEMM's split epilogue (fpq_gemm_fp4_mx_split_qknorm) and the KV-cache step (fpq_kv_cache_step_qknorm).
Ground truth: torch on the GPU running the reference's lines in fp32 on the same y = float(fp16 Linear output) + fp32 bias
(include/fpq.h states the contract): q and k within one fp16 ulp, v bit for bit, zero rows exact zeros."""
import pytest
import torch
import torch.nn.functional as Fn

pytestmark = pytest.mark.gpu


def _dev():
    return torch.device("cuda:0")


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


def _operands(tokens, c, kmajor, seed, zero_head=None):
    from fpqvar_amd import gemm
    torch.manual_seed(seed)
    x = torch.randn(tokens, c, device=_dev()).half()
    w = torch.randn(3 * c, c, device=_dev()) * 0.05
    if zero_head is not None:   # all weight rows of one head of q and of k are zero
        w[zero_head * 64:(zero_head + 1) * 64] = 0
        w[c + zero_head * 64:c + (zero_head + 1) * 64] = 0
    wq = gemm.quantize_mx(w)
    y16 = gemm.linear_fp4(*gemm.quantize_mx(x), *wq)
    if kmajor:
        return gemm.quantize_mx(x, kmajor=True), (gemm.to_kmajor(wq[0], 4, dealt=True), gemm.to_kmajor_scales(wq[1], weight_side=True)), y16
    return gemm.quantize_mx(x), wq, y16


def _bias(c, seed):
    g = torch.Generator().manual_seed(seed)
    b = torch.randn(3 * c, generator=g) * 0.1
    b[c:2 * c] = 0   # zero_k_bias
    return b.to(_dev())


@pytest.mark.parametrize("bsz,seq,heads", [(2, 1, 2), (3, 9, 2), (2, 25, 4), (5, 64, 2), (2, 169, 4), (3, 256, 2), (100, 1, 30), (7, 100, 30), (2, 2116, 4)])
@pytest.mark.parametrize("kmajor", [False, True])
@pytest.mark.parametrize("cfg", [None, 10, 20, 30])
@pytest.mark.parametrize("with_bias", [False, True])
def test_split_gemm_with_qk_norm(bsz, seq, heads, kmajor, cfg, with_bias, lib_options):
    from fpqvar_amd import gemm, kv_cache
    if cfg is not None:
        lib_options("FPQ_GEMM_CFG", cfg)
    c, max_len, pos = heads * 64, seq + 37, 11
    a, w, y16 = _operands(bsz * seq, c, kmajor, bsz * seq + heads)
    bias = _bias(c, heads + seq) if with_bias else None
    hs = kv_cache.qk_norm_head_scale(_scale_mul(heads, seq))
    y = y16.float().view(bsz, seq, 3 * c) + (bias if with_bias else 0.0)
    want_q, want_k, want_v = _reference(y, hs, heads)
    cache = torch.full((2, bsz, max_len, heads, 64), 7.5, dtype=torch.float16, device=_dev())
    q = gemm.linear_fp4_qkv_to_cache(*a, *w, bias, cache, pos, seq, qk_norm_scale=hs)
    assert q.shape == (bsz, seq, c)
    _assert_ulp(q.view(bsz, seq, heads, 64), want_q, "q")
    _assert_ulp(cache[0, :, pos:pos + seq], want_k, "k")
    assert torch.equal(cache[1, :, pos:pos + seq].view(torch.int16), want_v.view(torch.int16)), "v not bit-exact"
    untouched = torch.ones(max_len, dtype=torch.bool, device=_dev())
    untouched[pos:pos + seq] = False
    assert bool((cache[:, :, untouched] == 7.5).all()), "the GEMM wrote outside its slots"


@pytest.mark.parametrize("kmajor", [False, True])
def test_split_gemm_edge_rows(kmajor):
    """a head whose q / k weight rows are all zero: exact zeros without bias, the eps branch with a tiny bias; a head whose
    scale_mul_1H11 exceeds log 100 is clamped to 100"""
    from fpqvar_amd import gemm, kv_cache
    bsz, seq, heads = 3, 20, 4
    c = heads * 64
    a, w, y16 = _operands(bsz * seq, c, kmajor, 5, zero_head=1)
    sm = _scale_mul(heads, 1)
    hs = kv_cache.qk_norm_head_scale(sm)
    assert float(sm[0, 0]) > kv_cache.MAX_SCALE_MUL and abs(float(hs[0]) - 100.0) < 1e-4
    cache = torch.zeros(2, bsz, seq, heads, 64, dtype=torch.float16, device=_dev())
    q = gemm.linear_fp4_qkv_to_cache(*a, *w, None, cache, 0, seq, qk_norm_scale=hs).view(bsz, seq, heads, 64)
    assert bool((q[:, :, 1] == 0).all()) and bool((cache[0, :, :, 1] == 0).all()), "zero head: not exact zeros"
    assert not bool(torch.isnan(q).any() or torch.isnan(cache).any())
    want_q, want_k, _ = _reference(y16.float().view(bsz, seq, 3 * c), hs, heads)
    _assert_ulp(q, want_q, "q")
    _assert_ulp(cache[0], want_k, "k")
    # head 0 clamped to 100: its q rows have norm 100
    nq = q[:, :, 0].float().norm(dim=-1)
    assert bool(((nq - 100).abs() < 0.2).all()), float((nq - 100).abs().max())
    # tiny bias on the zero head: norm < 1e-12, q = y / 1e-12 * s
    bias = torch.zeros(3 * c, device=_dev())
    bias[64:128] = torch.linspace(-3e-14, 4e-14, 64, device=_dev())
    bias[c + 64:c + 128] = torch.linspace(2e-14, -1e-14, 64, device=_dev())
    q = gemm.linear_fp4_qkv_to_cache(*a, *w, bias, cache, 0, seq, qk_norm_scale=hs).view(bsz, seq, heads, 64)
    want_q, want_k, _ = _reference(y16.float().view(bsz, seq, 3 * c) + bias, hs, heads)
    assert float(want_k[:, :, 1].float().abs().max()) > 0.005   # the eps branch: y / 1e-12
    _assert_ulp(q, want_q, "q (tiny norm)")
    _assert_ulp(cache[0], want_k, "k (tiny norm)")


def _qkv_views(B, n, H, seed):
    """q, k, v as views of one [B, n, 3, H, 64] tensor inside a larger buffer: token and batch pitches that are not the rows'"""
    g = torch.Generator().manual_seed(seed)
    C = H * 64
    buf = torch.zeros(B, n + 3, 3 * C + 24, dtype=torch.float16)
    buf[:, 1:n + 1, 8:8 + 3 * C] = torch.randn(B, n, 3 * C, generator=g).half()
    buf = buf.to(_dev())
    qkv = buf[:, 1:n + 1, 8:8 + 3 * C].unflatten(-1, (3, H, 64))
    return qkv.unbind(2)


@pytest.mark.parametrize("kv_bit", [6, 4])
@pytest.mark.parametrize("front", ["native", "ctypes"])
@pytest.mark.parametrize("with_bias", [False, True])
@pytest.mark.parametrize("B,H,n", [(2, 2, 1), (3, 4, 9), (4, 30, 25), (2, 2, 169)])
def test_kv_step_with_qk_norm(kv_bit, front, with_bias, B, H, n, monkeypatch):
    from fpqvar_amd import kv_cache, ops
    if front == "ctypes":
        monkeypatch.setattr(ops, "_native", None)
    elif ops._native is None:
        pytest.fail("the compiled binding did not load")
    C, prev, pos, max_len = H * 64, 3, 7, 7 + n + 5
    group, table = (64, "e2m3") if kv_bit == 6 else (128, "e2m1")
    g = torch.Generator().manual_seed(B * 100 + n)
    cache = (torch.randn(2, B, max_len, H, 64, generator=g) * 0.3).half().to(_dev())
    plain = cache.clone()
    q, k, v = _qkv_views(B, n, H, n + H)
    bias = _bias(C, n) if with_bias else None
    hs = kv_cache.qk_norm_head_scale(_scale_mul(H, n))
    q_out = ops.kv_cache_step_qk_norm(cache, prev, pos, q, k, v, pos, group, table, hs, bias)
    empty = plain[0, :, :0]
    ops.kv_cache_step(plain, prev, pos, empty, empty, pos, group, table)
    assert torch.equal(cache[:, :, :pos].view(torch.int16), plain[:, :, :pos].view(torch.int16)), "previous entries differ from fpq_kv_cache_step"
    y = torch.stack((q, k, v), dim=2).reshape(B, n, 3 * C).float()
    if with_bias:
        y = y + bias
    want_q, want_k, want_v = _reference(y, hs, H)
    assert q_out.shape == (B, n, H, 64) and q_out.is_contiguous()
    _assert_ulp(q_out, want_q, "q_out")
    _assert_ulp(cache[0, :, pos:pos + n], want_k, "k")
    assert torch.equal(cache[1, :, pos:pos + n].view(torch.int16), want_v.view(torch.int16)), "v not bit-exact"
    assert torch.equal(cache[:, :, pos + n:].view(torch.int16), plain[:, :, pos + n:].view(torch.int16)), "wrote past the new entries"


def _oracle_quant(x, kv_bit):
    from oracle import fpq_oracle as orc
    x = x.cpu()
    if kv_bit == 6:
        return orc.per_token_kernel_sem(x, "e2m3")
    return orc.per_group_kernel_sem(x.reshape(-1, 128), "e2m1", 128).view(x.shape)


@pytest.mark.parametrize("kv_bit", [6, 4])
@pytest.mark.parametrize("producer", ["append_qk_norm", "split"])
def test_generation_steps_quantize_what_was_emitted(kv_bit, producer):
    """five steps: after each, the entries of the step before are the oracle quantizer applied to the fp16 values that the
    norm emitted into the cache, bit for bit (IncrementalKVCache's guarantee, now on unit-norm k)"""
    from fpqvar_amd import gemm, kv_cache
    B, H = 3, 4
    C = H * 64
    steps = (1, 4, 9, 16, 25)
    cache = kv_cache.IncrementalKVCache(B, sum(steps), H, 64, kv_bit, device=_dev())
    cache.kv.zero_()
    hs = kv_cache.qk_norm_head_scale(_scale_mul(H, 2))
    bias = _bias(C, 3)
    emitted = None
    for i, seq in enumerate(steps):
        start = cache.len
        if producer == "split":
            a, w, _ = _operands(B * seq, C, True, 200 + i)
            gemm.linear_fp4_qkv_to_cache(*a, *w, bias, cache.kv, cache.len, seq, qk_norm_scale=hs)
            kc, vc = cache.commit_written(seq)
        else:
            q, k, v = _qkv_views(B, seq, H, 300 + i)
            _, kc, vc = cache.append_qk_norm(q, k, v, hs, bias)
        if emitted is not None:
            a0, b0, ek, ev = emitted
            for got, raw in ((kc[:, a0:b0], ek), (vc[:, a0:b0], ev)):
                want = _oracle_quant(raw, kv_bit)
                assert torch.equal(got.cpu().view(torch.int16), want.view(torch.int16)), f"step {i}: quantized entries differ from the oracle"
        if producer == "split":   # (the split form writes, commit_written quantizes at the next step: the emitted values are these)
            emitted = (start, cache.len, cache.k[:, start:cache.len].clone(), cache.v[:, start:cache.len].clone())
        else:
            emitted = (start, cache.len, kc[:, start:].clone(), vc[:, start:].clone())
        nk = emitted[2].float().norm(dim=-1)
        assert bool(((nk - 1).abs() < 2e-3).all()), "cached k rows are not unit rows"


# Fused and torch forms of the norm differ by at most one fp16 ulp in q / k (another summation order).  Downstream, the block's FP4 /
# FP6 activation quantizers turn such a difference now and then into a whole quantization level - and a group whose maximum
# moved gets another scale for all its elements - so the step outputs cannot meet an element-wise bound like the attention
# tests' 2e-3 x max|v| (tests/test_gpu_parity.py).  They are compared by the relative RMS error of the whole step output instead.
# Measured on the first GPU runs (six steps, two blocks): 1.15e-2 (W4A4 path Q), 2.5e-3 (W6A6 path Q), 0 (path F, bit-identical);
# STEP_RMS keeps 2.6x margin over the worst.  CACHE_AGREEMENT: the issue's guess was 0.999; measured minima 0.9946 (W4A4 Q),
# 0.9973 (W6A6 Q), 1.0 (F) - an ulp on a row's maximum changes the scale of all its 64 elements - so the bound sits at the
# floor of 0.99.
STEP_RMS = 3e-2
CACHE_AGREEMENT = 0.99


@pytest.mark.parametrize("config,path", [("w4a4", "Q"), ("w6a6", "Q"), ("w4a4", "F")])
def test_generation_batch_fused_vs_torch_norm(config, path):
    from fpqvar_amd import var_block
    outs = {}
    for form in ("fused", "torch"):
        gb = var_block.GenerationBatch("d30-256", config, depth=2, batch_rows=4, device="cuda:0", seed=3, attn_l2_norm=True, qk_norm=form)
        caches = gb.new_caches(path)
        torch.manual_seed(0)
        gb.gen.manual_seed(11)
        ys = [gb.step(path, caches, gb.new_input(pn)) for pn in gb.patch_nums[:6]]
        outs[form] = (ys, [c.kv[:, :, :c.len].clone() for c in caches])
    errs = [float((y0.float() - y1.float()).norm() / y1.float().norm()) for y0, y1 in zip(outs["fused"][0], outs["torch"][0])]
    agree = [float((c0 == c1).float().mean()) for c0, c1 in zip(outs["fused"][1], outs["torch"][1])]
    print(f"{config} {path}: step output relative RMS error max {max(errs):.2e}, cache agreement min {min(agree):.5f}")
    for y0 in outs["fused"][0]:
        assert torch.isfinite(y0).all()
    assert max(errs) <= STEP_RMS, errs
    assert min(agree) >= CACHE_AGREEMENT, f"cache agreement {agree}"


def test_generation_batch_l2_norm_runs_reference_path():
    from fpqvar_amd import var_block
    gb = var_block.GenerationBatch("d30-256", "w4a4", depth=1, batch_rows=2, device="cuda:0", seed=1, attn_l2_norm=True)
    caches = gb.new_caches("R")
    for pn in gb.patch_nums[:3]:
        y = gb.step("R", caches, gb.new_input(pn))
        assert torch.isfinite(y).all()
    assert caches[0][0].dtype == torch.float32, "the reference caches fp32 k under attn_l2_norm"


def test_argument_rejection():
    from fpqvar_amd import gemm, kv_cache, ops
    bsz, seq, heads = 2, 9, 2
    c = heads * 64
    a, w, _ = _operands(bsz * seq, c, True, 1)
    hs = kv_cache.qk_norm_head_scale(_scale_mul(heads, 0))
    cache = torch.zeros(2, bsz, 20, heads, 64, dtype=torch.float16, device=_dev())
    with pytest.raises(RuntimeError):   # head_dim != 64
        gemm.linear_fp4_qkv_to_cache(*a, *w, None, torch.zeros(2, bsz, 20, 1, 128, dtype=torch.float16, device=_dev()), 0, seq,
                                     qk_norm_scale=hs[:1])
    with pytest.raises(RuntimeError):   # wrong-length qk_norm_scale
        gemm.linear_fp4_qkv_to_cache(*a, *w, None, cache, 0, seq, qk_norm_scale=torch.ones(heads + 1, device=_dev()))
    with pytest.raises(RuntimeError):   # fp16 scale
        gemm.linear_fp4_qkv_to_cache(*a, *w, None, cache, 0, seq, qk_norm_scale=hs.half())
    with pytest.raises(RuntimeError):   # fp16 bias where fp32 is required
        gemm.linear_fp4_qkv_to_cache(*a, *w, _bias(c, 0).half(), cache, 0, seq, qk_norm_scale=hs)
    # n_parts != 3 (the C entry point; the Python front end always passes three parts)
    from fpqvar_amd._lib import GemmSplit, lib
    sp = GemmSplit()
    sp.part_cols, sp.n_parts, sp.rows_per_batch = c, 2, seq
    for p in range(3):
        sp.out[p], sp.row_stride[p], sp.batch_stride[p], sp.row0[p] = cache.data_ptr(), c, 20, 0
    import ctypes
    assert lib().fpq_gemm_fp4_mx_split_qknorm(a[0].data_ptr(), a[1].data_ptr(), w[0].data_ptr(), w[1].data_ptr(), 1, None,
                                              bsz * seq, 2 * c, c, ctypes.byref(sp), hs.data_ptr(), 1, None) == -1
    q, k, v = _qkv_views(bsz, 3, heads, 0)
    for front in ("native", "ctypes"):
        saved = ops._native
        if front == "ctypes":
            ops._native = None
        try:
            with pytest.raises(RuntimeError):   # head_dim != 64
                ops.kv_cache_step_qk_norm(torch.zeros(2, bsz, 20, 4, 32, dtype=torch.float16, device=_dev()), 0, 0,
                                          q.reshape(bsz, 3, 4, 32), k.reshape(bsz, 3, 4, 32), v.reshape(bsz, 3, 4, 32), 0, 64, "e2m3",
                                          torch.ones(4, device=_dev()))
            with pytest.raises(RuntimeError):   # wrong-length head scale
                ops.kv_cache_step_qk_norm(cache, 0, 0, q, k, v, 0, 64, "e2m3", torch.ones(heads + 1, device=_dev()))
            with pytest.raises(RuntimeError):   # fp16 bias
                ops.kv_cache_step_qk_norm(cache, 0, 0, q, k, v, 0, 64, "e2m3", hs, _bias(c, 0).half())
        finally:
            ops._native = saved
