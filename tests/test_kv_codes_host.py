"""CPU-only checks of the packed KV cache (include/fpq.h): the C entry points refuse bad arguments with FPQ_ERR_ARG before any
launch, the new kernels spill nothing, the Python layer refuses CPU tensors, and the decode tables are the OCP formats."""
import pytest
import torch

ARG = -1


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as g
    g.build_hip()
    from fpqvar_amd import _lib
    return _lib.lib()


def _pack(lib, codes=16, scales=16, kv_bit=6, batch=2, max_len=8, heads=4, head_dim=64, pos=0, k=16, v=16, bp=2048, tp=256, n=3):
    return lib.fpq_kv_pack(codes, scales, kv_bit, batch, max_len, heads, head_dim, pos, k, v, bp, tp, n, None)


def test_kv_pack_argument_checks(lib):
    assert _pack(lib, kv_bit=5) == ARG
    assert _pack(lib, kv_bit=8) == ARG
    assert _pack(lib, kv_bit=4, heads=3) == ARG          # one scale per 128 elements: H even
    assert _pack(lib, head_dim=128) == ARG
    assert _pack(lib, pos=6, n=3) == ARG                 # past max_len
    assert _pack(lib, pos=-1) == ARG
    assert _pack(lib, n=-1) == ARG
    assert _pack(lib, batch=-1) == ARG
    assert _pack(lib, batch=70000) == ARG
    assert _pack(lib, tp=252) == ARG                     # pitch not a multiple of 8
    assert _pack(lib, bp=-8) == ARG
    assert _pack(lib, codes=None) == ARG
    assert _pack(lib, scales=None) == ARG
    assert _pack(lib, k=None) == ARG
    assert _pack(lib, codes=20) == ARG                   # not 16-byte aligned
    assert _pack(lib, v=24) == ARG
    assert _pack(lib, n=0, codes=None, k=None) == 0       # nothing to do
    assert _pack(lib, batch=0, codes=None) == 0


def _attn(lib, q=16, codes=16, scales=16, kv_bit=6, max_len=8, n_packed=4, k=16, v=16, bp=2048, tp=256, n_new=2, out=16, batch=2,
          lq=3, heads=4, head_dim=64, qb=2048, qt=256, scale=0.125):
    return lib.fpq_attention_blhc_kvcodes(q, codes, scales, kv_bit, max_len, n_packed, k, v, bp, tp, n_new, out, batch, lq, heads,
                                          head_dim, qb, qt, scale, None)


def test_attention_kvcodes_argument_checks(lib):
    assert _attn(lib, kv_bit=5) == ARG
    assert _attn(lib, kv_bit=4, heads=5) == ARG
    assert _attn(lib, head_dim=32) == ARG
    assert _attn(lib, n_packed=9) == ARG                 # past max_len
    assert _attn(lib, n_packed=-1) == ARG
    assert _attn(lib, n_new=-1) == ARG
    assert _attn(lib, n_packed=0, n_new=0) == ARG        # softmax over nothing
    assert _attn(lib, scale=0.0) == ARG
    assert _attn(lib, scale=float("nan")) == ARG
    assert _attn(lib, q=None) == ARG
    assert _attn(lib, out=None) == ARG
    assert _attn(lib, codes=None) == ARG
    assert _attn(lib, scales=None) == ARG
    assert _attn(lib, k=None) == ARG
    assert _attn(lib, out=8) == ARG                      # not 16-byte aligned
    assert _attn(lib, scales=18) == ARG
    assert _attn(lib, qt=100) == ARG                     # pitch not a multiple of 8
    assert _attn(lib, tp=-8) == ARG
    assert _attn(lib, heads=0) == ARG
    assert _attn(lib, batch=0, q=None) == 0              # nothing to do
    assert _attn(lib, lq=0, q=None) == 0


def test_new_kernels_do_not_spill(tmp_path, lib):
    from tests.test_no_spill import kernel_metadata
    recs = kernel_metadata(tmp_path)
    new = [(n, r) for n, r in recs if "kv_pack_kernel" in n or "AttnCodesSrc" in n]
    assert len(new) == 4, [n for n, _ in new]   # kv_pack_kernel<6 | 4>, attn_fwd64_kernel<AttnCodesSrc<6 | 4>>
    for n, r in new:
        assert int(r.get("vgpr_spill_count", 0)) == 0 and int(r.get("sgpr_spill_count", 0)) == 0, n
        assert int(r.get("private_segment_fixed_size", 0)) == 0, n
    # the fp16 instantiation keeps the register budget of three workgroups per CU (__launch_bounds__(256, 3)): <= 168 VGPRs
    for n, r in recs:
        if "attn_fwd64_kernel" in n:
            assert int(r["vgpr_count"]) <= 168, (n, r["vgpr_count"])


def test_python_layer_refuses_cpu_tensors():
    from fpqvar_amd import kv_cache, ops
    with pytest.raises(RuntimeError):
        kv_cache.PackedKVCache(2, 8, 4, 64, 6, "cpu")
    codes = torch.zeros(2, 2, 8, 4, 48, dtype=torch.uint8)
    scales = torch.zeros(2, 2, 8, 4, dtype=torch.float16)
    k = torch.zeros(2, 3, 4, 64, dtype=torch.float16)
    with pytest.raises(RuntimeError):
        ops.kv_pack(codes, scales, 6, 0, k, k)
    with pytest.raises(RuntimeError):
        ops.attention_blhc_kvcodes(k, codes, scales, 6, 2, k, k, 0.125)


def test_generation_batch_kv_storage_is_checked_before_any_device_work():
    from fpqvar_amd import var_block
    with pytest.raises(ValueError):
        var_block.GenerationBatch("d30-256", "w4a4", depth=1, kv_storage="fp8")
    with pytest.raises(ValueError):
        var_block.GenerationBatch("d30-256", "w4a4", depth=1, kv_storage="codes", sdpa_in_f=True)


def test_decode_tables_are_the_ocp_formats():
    """The level tables PackedKVCache.dequantize decodes with: every code's value is the oracle table's entry of that magnitude,
    with the code's sign."""
    from fpqvar_amd import kv_cache
    from oracle import fpq_oracle as orc
    for levels, name, sign_bit in ((kv_cache._e2m3_levels(), "e2m3", 32), (kv_cache._e2m1_levels(), "e2m1", 8)):
        pos = levels[:sign_bit]
        assert torch.equal(pos, torch.sort(pos).values) and pos[0] == 0
        table = orc.TABLES[name].float()
        assert torch.equal(torch.sort(table[table >= 0]).values.unique(), pos.unique()), name
        assert torch.equal(levels[sign_bit:], -pos)
