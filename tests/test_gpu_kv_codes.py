"""The packed KV cache (include/fpq.h; kv_cache.PackedKVCache): FP6 / FP4 codes + fp16 scales in place of the fake-quantized fp16
cache.  Pinned bit for bit to the fp16 path: the pack (fpq_kv_pack) against IncrementalKVCache and the oracle, attention over
codes + fresh rows (fpq_attention_blhc_kvcodes) against fpq_attention_blhc on the IncrementalKVCache views at every step of both
models, the producers that write into the shared staging slab, whole GenerationBatch runs eager and captured, and the memory
it gives back."""
import pytest
import torch

from tests.conftest import assert_bits_equal

pytestmark = pytest.mark.gpu

MODELS = {"d30-256": (30, (1, 2, 3, 4, 5, 6, 8, 10, 13, 16)), "d36-512": (36, (1, 2, 3, 4, 6, 9, 13, 18, 24, 32))}


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "these tests need the GPU"
    return torch.device("cuda:0")


def _rows(family, B, n, H, g):
    """fp16 [B, n, H, 64] of one input family (CPU)."""
    x = torch.randn(B, n, H, 64, generator=g)
    if family == "zeros":
        x = torch.zeros(B, n, H, 64)
    elif family == "tiny":        # max |row| < 4e-4: the fp16 scale (max / 7.5 or / 6) is subnormal
        x = x * 3e-5
    elif family == "large":
        x = x * 8000.0
    elif family == "signed_zeros":
        x = torch.where(torch.rand(B, n, H, 64, generator=g) < 0.4, torch.zeros(()), x)
        x = torch.where(torch.rand(B, n, H, 64, generator=g) < 0.5, -x, x)   # -0.0 among the zeros
    elif family == "mixed":       # rows of every family next to each other
        f = torch.randint(0, 4, (B, n, H, 1), generator=g)
        x = torch.where(f == 0, torch.zeros(()), torch.where(f == 1, x * 3e-5, torch.where(f == 2, x * 8000.0, x)))
    return x.half()


def _as_qkv_views(q, k, v, dev):
    """q, k, v as the three views of a [B, L, 3, H, 64] qkv output whose other slots are NaN."""
    B, L, H, _ = k.shape
    qkv = torch.full((B, L, 3, H, 64), float("nan"), dtype=torch.float16, device=dev)
    qkv[:, :, 0], qkv[:, :, 1], qkv[:, :, 2] = q.to(dev), k.to(dev), v.to(dev)
    return qkv[:, :, 0], qkv[:, :, 1], qkv[:, :, 2]


def _poison_tail(pc):
    """NaN scales and all-ones codes in every slot at and past len: nothing there may be read."""
    pc.scales[:, :, pc.len:] = float("nan")
    pc.codes[:, :, pc.len:] = 0xFF


@pytest.mark.parametrize("kv_bit,H", [(6, 7), (6, 30), (4, 30), (4, 2)])
@pytest.mark.parametrize("family", ["random", "zeros", "tiny", "large", "signed_zeros", "mixed"])
@pytest.mark.parametrize("views", [False, True])
def test_pack_equals_incremental_cache(dev, kv_bit, H, family, views):
    from fpqvar_amd import kv_cache, ops
    B, steps = 3, (1, 4, 9, 70, 3)
    g = torch.Generator().manual_seed(100 * kv_bit + H + 7 * len(family) + int(views))
    inc = kv_cache.IncrementalKVCache(B, sum(steps), H, 64, kv_bit, device=dev)
    pc = kv_cache.PackedKVCache(B, sum(steps), H, 64, kv_bit, dev)
    for n in steps:
        k, v = _rows(family, B, n, H, g), _rows(family, B, n, H, g)
        if views:
            _, k, v = _as_qkv_views(k, k, v, dev)
        else:
            k, v = k.to(dev), v.to(dev)
        inc.append(k, v)
        ops.kv_pack(pc.codes, pc.scales, kv_bit, pc.len, k, v)
        pc.len += n
    inc.commit_written(0)   # quantizes the last step's entries
    K, V = pc.dequantize()
    assert_bits_equal(K, inc.k[:, :inc.len], f"K kv_bit {kv_bit} {family}")
    assert_bits_equal(V, inc.v[:, :inc.len], f"V kv_bit {kv_bit} {family}")


@pytest.mark.parametrize("kv_bit", [6, 4])
@pytest.mark.parametrize("family", ["random", "zeros", "large", "signed_zeros"])
def test_pack_equals_oracle(dev, kv_bit, family):
    from fpqvar_amd import kv_cache, ops
    from oracle import fpq_oracle as orc
    B, n, H = 2, 37, 6
    g = torch.Generator().manual_seed(11 + kv_bit)
    k, v = _rows(family, B, n, H, g), _rows(family, B, n, H, g)
    pc = kv_cache.PackedKVCache(B, n + 5, H, 64, kv_bit, dev)
    ops.kv_pack(pc.codes, pc.scales, kv_bit, 0, k.to(dev), v.to(dev))
    pc.len = n
    K, V = pc.dequantize()
    for got, x in ((K, k), (V, v)):
        if kv_bit == 6:
            want = orc.per_token_kernel_sem(x.reshape(-1, 64), "e2m3").view(x.shape)
        else:
            want = orc.per_group_kernel_sem(x.reshape(-1, 128), "e2m1", 128).view(x.shape)
        assert_bits_equal(got, want, f"kv_bit {kv_bit} {family} vs oracle")


def test_pack_leaves_other_slots_alone(dev):
    from fpqvar_amd import kv_cache, ops
    pc = kv_cache.PackedKVCache(2, 20, 4, 64, 6, dev)
    pc.codes.fill_(0xA5)
    pc.scales.fill_(3.0)
    before_c, before_s = pc.codes.clone(), pc.scales.clone()
    k = torch.randn(2, 5, 4, 64, device=dev).half()
    ops.kv_pack(pc.codes, pc.scales, 6, 7, k, k)
    assert torch.equal(pc.codes[:, :, :7], before_c[:, :, :7]) and torch.equal(pc.codes[:, :, 12:], before_c[:, :, 12:])
    assert torch.equal(pc.scales[:, :, :7], before_s[:, :, :7]) and torch.equal(pc.scales[:, :, 12:], before_s[:, :, 12:])


@pytest.mark.parametrize("model", list(MODELS))
@pytest.mark.parametrize("kv_bit", [6, 4])
@pytest.mark.parametrize("qk_norm_scale", [False, True])
def test_attention_over_codes_equals_fp16_cache_every_step(dev, model, kv_bit, qk_norm_scale):
    """Every scale step of the model (real H, B = 2): PackedKVCache.attend == attention_blhc on IncrementalKVCache.append's views.
    q / k / v are views of a NaN-filled qkv output; the packed slots at and past n_packed hold NaN scales."""
    from fpqvar_amd import kv_cache, ops
    H, pns = MODELS[model]
    B, total = 2, sum(p * p for p in pns)
    scale = 1.0 if qk_norm_scale else 64 ** -0.5
    g = torch.Generator().manual_seed(5 + kv_bit)
    inc = kv_cache.IncrementalKVCache(B, total, H, 64, kv_bit, device=dev)
    pc = kv_cache.PackedKVCache(B, total, H, 64, kv_bit, dev)
    for pn in pns:
        L = pn * pn
        q, k, v = (torch.randn(B, L, H, 64, generator=g) for _ in range(3))
        if qk_norm_scale:   # unit-norm q / k scaled as the attn_l2_norm blocks do, scale 1
            q = torch.nn.functional.normalize(q, dim=-1) * 4.0
            k = torch.nn.functional.normalize(k, dim=-1)
        q, k, v = _as_qkv_views(q.half(), k.half(), v.half(), dev)
        want = ops.attention_blhc(q, *inc.append(k, v), scale)
        _poison_tail(pc)
        got = pc.attend(q, k, v, scale)
        assert_bits_equal(got, want, f"{model} kv_bit {kv_bit} step {pn}")
    assert pc.len == inc.len == total


@pytest.mark.parametrize("kv_bit", [6, 4])
def test_attention_over_codes_edges(dev, kv_bit):
    """n_packed from 0 to past a tile, L = 1, lkv < 64, lkv a multiple of 64, an all-packed tile boundary, B * H not a multiple of 8."""
    from fpqvar_amd import kv_cache, ops
    B, H = 3, 6
    steps = (1, 1, 30, 32, 64, 1, 63, 2, 128, 129)
    g = torch.Generator().manual_seed(77)
    inc = kv_cache.IncrementalKVCache(B, sum(steps), H, 64, kv_bit, device=dev)
    pc = kv_cache.PackedKVCache(B, sum(steps), H, 64, kv_bit, dev)
    for L in steps:
        q, k, v = (torch.randn(B, L, H, 64, generator=g).half().to(dev) for _ in range(3))
        want = ops.attention_blhc(q, *inc.append(k, v), 0.125)
        _poison_tail(pc)
        assert_bits_equal(pc.attend(q, k, v, 0.125), want, f"kv_bit {kv_bit} L {L} n_packed {pc.len - L}")
    # no fresh rows at all: attention over the packed entries alone
    K, V = pc.dequantize()
    q = torch.randn(B, 5, H, 64, generator=g).half().to(dev)
    empty = torch.empty(B, 0, H, 64, dtype=torch.float16, device=dev)
    assert_bits_equal(ops.attention_blhc_kvcodes(q, pc.codes, pc.scales, kv_bit, pc.len, empty, empty, 0.125),
                      ops.attention_blhc(q, K, V, 0.125), "n_new = 0")


def _split_operands(B, L, H, seed, dev):
    from fpqvar_amd import gemm
    C = 64 * H
    torch.manual_seed(seed)
    x = torch.randn(B * L, C, device=dev).half()
    w = torch.randn(3 * C, C, device=dev) * 0.05
    return gemm.quantize_mx(x, kmajor=True), (lambda wq: (gemm.to_kmajor(wq[0], 4, dealt=True), gemm.to_kmajor_scales(wq[1], weight_side=True)))(gemm.quantize_mx(w))


@pytest.mark.parametrize("l2", [False, True])
def test_split_gemm_into_staging_equals_commit_written(dev, l2):
    from fpqvar_amd import gemm, kv_cache, ops
    B, H, steps = 3, 4, (1, 4, 9, 16, 25)
    inc = kv_cache.IncrementalKVCache(B, sum(steps), H, 64, 6, device=dev)
    staging = kv_cache.PackedKVCache.new_staging(B, max(steps), H, device=dev)
    pc = kv_cache.PackedKVCache(B, sum(steps), H, 64, 6, dev, staging)
    bias = torch.randn(3 * H * 64, device=dev) * 0.1 if l2 else None
    hs = torch.rand(H, device=dev) * 3 + 1 if l2 else None
    scale = 1.0 if l2 else 0.125
    for i, L in enumerate(steps):
        a, w = _split_operands(B, L, H, 200 + i, dev)
        qa = gemm.linear_fp4_qkv_to_cache(*a, *w, bias, inc.kv, inc.len, L, qk_norm_scale=hs).view(B, L, H, 64)
        want = ops.attention_blhc(qa, *inc.commit_written(L), scale)
        staging.fill_(float("nan"))
        qb = gemm.linear_fp4_qkv_to_cache(*a, *w, bias, staging, 0, L, qk_norm_scale=hs).view(B, L, H, 64)
        assert_bits_equal(qb, qa, f"q step {i}")
        _poison_tail(pc)
        assert_bits_equal(pc.attend_staged(qb, L, scale), want, f"step {i}")


def test_qk_norm_producer_into_staging_equals_append_qk_norm(dev):
    from fpqvar_amd import kv_cache, ops
    B, H, steps = 2, 6, (1, 4, 9, 16, 25, 36)
    inc = kv_cache.IncrementalKVCache(B, sum(steps), H, 64, 6, device=dev)
    staging = kv_cache.PackedKVCache.new_staging(B, max(steps), H, device=dev)
    pc = kv_cache.PackedKVCache(B, sum(steps), H, 64, 6, dev, staging)
    g = torch.Generator().manual_seed(3)
    bias = (torch.randn(3 * H * 64, generator=g) * 0.1).to(dev)
    hs = (torch.rand(H, generator=g) * 3 + 1).to(dev)
    for L in steps:
        q, k, v = _as_qkv_views(*(torch.randn(B, L, H, 64, generator=g).half() for _ in range(3)), dev)
        qa, K, V = inc.append_qk_norm(q, k, v, hs, bias)
        want = ops.attention_blhc(qa, K, V, 1.0)
        staging.fill_(float("nan"))
        qb = pc.stage_qk_norm(q, k, v, hs, bias)
        assert_bits_equal(qb, qa, f"q L {L}")
        _poison_tail(pc)
        assert_bits_equal(pc.attend_staged(qb, L, 1.0), want, f"L {L}")


def _final(gb, path, graphs):
    if not graphs:
        caches = gb.new_caches(path)
        for pn in gb.patch_nums:
            y = gb.step(path, caches, gb.new_input(pn))
        return y.clone()
    gr, keep = gb.capture(path)
    gb.replay(gr)
    y = keep[-1][1].clone()
    del gr, keep
    return y


CASES = [(m, p, c, l2) for m in MODELS for p in ("F", "Q") for c in ("w4a4", "w6a6") for l2 in (False, True)]


@pytest.mark.parametrize("model,path,config,l2", CASES)
def test_generation_batch_codes_equals_fp16(dev, model, path, config, l2):
    from fpqvar_amd import var_block
    outs = {}
    for st in ("fp16", "codes"):
        gb = var_block.GenerationBatch(model, config, depth=2, batch_rows=4, device=dev, attn_l2_norm=l2, kv_storage=st)
        graphs = (path == "Q" or config == "w6a6")   # captured for 12 of the 16 cases, eager for the rest
        outs[st] = (_final(gb, path, False), _final(gb, path, True) if graphs else None)
        if st == "codes":
            assert "FP6 codes" in gb.describe()
        else:
            assert "codes" not in gb.describe()
        del gb
    assert_bits_equal(outs["codes"][0], outs["fp16"][0], f"{model} {path} {config} l2={l2} eager")
    if outs["fp16"][1] is not None:
        assert_bits_equal(outs["codes"][1], outs["fp16"][1], f"{model} {path} {config} l2={l2} graphs")


def test_generation_batch_codes_refuses_path_r(dev):
    from fpqvar_amd import var_block
    gb = var_block.GenerationBatch("d30-256", "w4a4", depth=1, batch_rows=2, device=dev, kv_storage="codes")
    with pytest.raises(ValueError):
        gb.new_caches("R")
    with pytest.raises(ValueError):
        var_block.GenerationBatch("d30-256", "w4a4", depth=1, batch_rows=2, device=dev, kv_storage="codes", sdpa_in_f=True)


@pytest.mark.parametrize("kv_bit", [6, 4])
def test_nbytes_matches_the_layout(dev, kv_bit):
    from fpqvar_amd import kv_cache
    B, T, H = 3, 50, 30
    pc = kv_cache.PackedKVCache(B, T, H, 64, kv_bit, dev)
    per_row = 50 if kv_bit == 6 else 33   # bytes per (token, head) row of 64: codes + (share of) the fp16 scale
    assert pc.nbytes == 2 * B * T * H * per_row
    assert pc.codes.numel() + 2 * pc.scales.numel() == pc.nbytes


def test_codes_storage_gives_memory_back(dev):
    """One d30-256 batch (B = 100, 680 tokens, C = 1920) at depth 4: the peak allocation of the run drops by at least 0.9 x
    (fp16 slabs - packed slabs - the shared staging slab)."""
    from fpqvar_amd import var_block
    depth = 4
    peaks = {}
    for st in ("fp16", "codes"):
        gb = var_block.GenerationBatch("d30-256", "w4a4", depth=depth, device=dev, kv_storage=st)
        torch.cuda.synchronize()
        base = torch.cuda.memory_allocated(dev)
        torch.cuda.reset_peak_memory_stats(dev)
        caches = gb.new_caches("Q")
        for pn in gb.patch_nums:
            gb.step("Q", caches, gb.new_input(pn))
        torch.cuda.synchronize()
        peaks[st] = torch.cuda.max_memory_allocated(dev) - base
        B, T, H, max_step = gb.B, gb.max_len, gb.H, max(p * p for p in gb.patch_nums)
        del caches, gb
        torch.cuda.empty_cache()
    fp16 = depth * 2 * B * T * H * 64 * 2
    packed = depth * 2 * B * T * H * 50
    staging = 2 * B * max_step * H * 64 * 2
    assert peaks["fp16"] - peaks["codes"] >= 0.9 * (fp16 - packed - staging), (peaks, fp16, packed, staging)


def test_everything_is_capturable(dev):
    """attend / attend_staged / stage_qk_norm inside one captured graph replay to the eager results."""
    from fpqvar_amd import kv_cache
    B, H, L = 2, 4, 9
    g = torch.Generator().manual_seed(9)
    q, k, v = (torch.randn(B, L, H, 64, generator=g).half().to(dev) for _ in range(3))
    eager = kv_cache.PackedKVCache(B, 3 * L, H, 64, 6, dev)
    want = [eager.attend(q, k, v, 0.125) for _ in range(3)]
    pc = kv_cache.PackedKVCache(B, 3 * L, H, 64, 6, dev)
    gr = torch.cuda.CUDAGraph()
    with torch.cuda.graph(gr):
        outs = [pc.attend(q, k, v, 0.125) for _ in range(3)]
    gr.replay()
    torch.cuda.synchronize()
    for i in range(3):
        assert_bits_equal(outs[i], want[i], f"step {i}")


def test_wrappers_reject_bad_arguments(dev):
    from fpqvar_amd import kv_cache, ops
    pc = kv_cache.PackedKVCache(2, 8, 4, 64, 4, dev)
    k = torch.randn(2, 3, 4, 64, device=dev).half()
    with pytest.raises(RuntimeError):
        ops.kv_pack(pc.codes, pc.scales, 6, 0, k, k)          # layout of kv_bit 4 handed over as kv_bit 6
    with pytest.raises(RuntimeError):
        ops.kv_pack(pc.codes, pc.scales, 4, 6, k, k)          # past max_len
    with pytest.raises(RuntimeError):
        ops.kv_pack(pc.codes, pc.scales, 4, 0, k.float(), k.float())
    with pytest.raises(RuntimeError):
        kv_cache.PackedKVCache(2, 8, 3, 64, 4, dev)           # odd H with kv_bit 4
    long = torch.randn(2, 9, 4, 64, device=dev).half()
    with pytest.raises(RuntimeError):
        pc.attend(long, long, long, 0.125)                    # 9 tokens > max_len 8
    with pytest.raises(RuntimeError):
        ops.attention_blhc_kvcodes(k, pc.codes, pc.scales, 4, 9, k, k, 0.125)   # n_packed > max_len
    with pytest.raises(RuntimeError):
        pc.attend_staged(k, 3, 0.125)                         # no staging slab
