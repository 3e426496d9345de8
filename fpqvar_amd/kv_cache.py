"""KV-cache fake quantization as the reference does it inside SelfAttention.forward
(models_fp_quant_transform_rotate/basic_var.py:186-209): at every step after the first
the WHOLE cached K and V are re-quantized before the new k / v are appended -
kv_bit 6: FP6-E2M3, one scale per (token, head) row of head_dim (=64) channels;
kv_bit 4: FP4-E2M1 on consecutive groups of 128 elements of the flattened cache.
Both are single launches of the fused kernels (8 or 16 lanes own a row).
"""
from __future__ import annotations

import math
from typing import Optional, Tuple

import torch

from . import ops, quant_utils as qu


KV_TABLE = {6: "e2m3", 4: "e2m1"}   # the quantizer table of a kv_bit
MAX_SCALE_MUL = math.log(100)   # SelfAttention.max_scale_mul (tr/basic_var.py:140), torch.log(torch.tensor(100)).item()


def qk_norm_head_scale(scale_mul_1H11: torch.Tensor) -> torch.Tensor:
    """The per-head multiplier of q in a block with attn_l2_norm: `scale_mul_1H11.clamp_max(max_scale_mul).exp()`
    (tr/basic_var.py:178) as fp32 [H] - computed once at load time, the argument of IncrementalKVCache.append_qk_norm and of
    gemm.linear_fp4_qkv_to_cache(..., qk_norm_scale=)."""
    return scale_mul_1H11.detach().float().clamp_max(MAX_SCALE_MUL).exp().reshape(-1).contiguous()


def quantize_kv(t: torch.Tensor, kv_bit: int) -> torch.Tensor:
    """basic_var.py:193-200.  kv_bit 6 needs a contiguous cache (the reference's
    x.view(-1) raises on the permuted BHLc layout too); the result is fp16."""
    if kv_bit == 6:
        return qu.fp6_quant_e2m3_per_token_cuda(t, kv_bit)
    if kv_bit == 4:
        return qu.fp_quant_e2_per_group_cuda(t, kv_bit)
    raise NotImplementedError


def quantize_kv_pair(k: torch.Tensor, v: torch.Tensor, kv_bit: int) -> Tuple[torch.Tensor, torch.Tensor]:
    """quantize_kv on the cached K and the cached V (basic_var.py:193-200 quantizes them back to back): one launch for
    the pair when both are fp16 (fpq_quant_rows_multi), same results and the same layout rule as the single calls."""
    if k.dtype == v.dtype == torch.float16 and k.device == v.device and kv_bit in (4, 6):
        if kv_bit == 6:
            qu._require_viewable(k)
            qu._require_viewable(v)
        if kv_bit == 4 or k.shape[-1] == v.shape[-1]:
            return tuple(ops.quant_rows_multi([k, v], KV_TABLE[kv_bit], k.shape[-1] if kv_bit == 6 else 128))
    return quantize_kv(k, kv_bit), quantize_kv(v, kv_bit)


def update_kv_cache(cached_k: Optional[torch.Tensor], cached_v: Optional[torch.Tensor], k: torch.Tensor,
                    v: torch.Tensor, quant_KV: bool, kv_bit: int, dim_cat: int, check_finite: bool = True
                    ) -> Tuple[torch.Tensor, torch.Tensor]:
    """One caching step: returns the new (cached_k, cached_v), which are also the k / v
    attention runs on.  `check_finite` keeps the reference's asserts on the new k / v
    (they synchronise the host, as they do in the reference)."""
    if cached_k is None:
        return k, v
    if quant_KV:
        cached_k, cached_v = quantize_kv_pair(cached_k, cached_v, kv_bit)
        if check_finite:
            assert not torch.isnan(k).any(), "Tensor contains NaN values!"
            assert not torch.isinf(k).any(), "Tensor contains inf values!"
            assert not torch.isnan(v).any(), "Tensor contains NaN values!"
            assert not torch.isinf(v).any(), "Tensor contains inf values!"
    return torch.cat((cached_k, k), dim=dim_cat), torch.cat((cached_v, v), dim=dim_cat)


class IncrementalKVCache:
    """F3: the same K / V the reference's re-quantize-everything loop produces,
    with every cache entry quantized exactly ONCE.

    Why this is exact: re-quantizing an already fake-quantized row returns it unchanged (same scale,
    same levels) whenever the row's fp16 scale is a normal number, i.e. max|row| >= ~4e-4 - proven by
    exhaustion over every fp16 row maximum and every level in tests/test_kv_idempotence.py.  The
    reference quantizes the cache BEFORE appending the new k / v (tr/basic_var.py:192-209), so at
    step t the entries of step t-1 are quantized for the first time and all older ones are
    re-quantized to themselves; here only the former happens.  Rows below that magnitude (not seen
    with unit-norm keys / O(1) values) may differ in their last bits.

    Layout: flash layout [B, L, H, c] (`dim_cat` = 1), as the reference's published KV runs use; with
    kv_bit 4 a 128-group then never straddles tokens as long as H*c is a multiple of 128.
    Buffers are allocated once for `max_len` tokens; `append` returns views of the filled prefix.

    One step of a block, the protocol PackedKVCache shares (each returns the attention output, fp16 [B, L, H, c]):
      slots(n)                                          (slab [2, B, *, H, c], first token): where a producer writes the step's k / v
      attend(q, k, v, scale)                            fresh k / v handed over: `append`, then attention
      attend_written(q, n, scale)                       k / v already sit in slots(n): `commit_written`, then attention
      attend_qk_norm(q, k, v, head_scale, bias, scale)  the fused q / k norm on an fp16 qkv: `append_qk_norm`, then attention
    `attention`: the function (q, K, V, scale) that attends; None: ops.attention_blhc, off the cache views.
    """

    def __init__(self, batch: int, max_len: int, heads: int, head_dim: int, kv_bit: int,
                 dtype=torch.float16, device="cuda", attention=None):
        assert kv_bit in (4, 6)
        assert kv_bit == 6 or (heads * head_dim) % 128 == 0
        self.kv_bit, self._table, self._attention = kv_bit, KV_TABLE[kv_bit], attention
        self.kv = torch.empty(2, batch, max_len, heads, head_dim, dtype=dtype, device=device)   # K and V in one slab
        self.k, self.v = self.kv[0], self.kv[1]
        self.len = 0
        self._prev = 0              # entries [_prev, len) were appended by the last step and are still unquantized
        # one launch per step (fpq_kv_cache_step) when the rows fit the fused kernels' lanes
        group = head_dim if kv_bit == 6 else 128
        self._group = group if (dtype == torch.float16 and group in (8, 16, 32, 64, 128, 256, 512)) else None

    @torch.no_grad()
    def commit_written(self, n: int) -> Tuple[torch.Tensor, torch.Tensor]:
        """`append` for k / v that the producer has ALREADY written into the cache's slots [len, len + n) (the qkv GEMM with a
        split output, gemm.linear_fp4_qkv_to_cache(..., cache.kv, cache.len, n)): quantizes the previous step's entries - one launch,
        nothing copied - and returns the same views."""
        assert self.len + n <= self.k.shape[1], "IncrementalKVCache: max_len exceeded"
        if self._group is None:
            self._quantize_previous()
        elif self.len > self._prev:
            empty = self.kv[0, :, :0]
            ops.kv_cache_step(self.kv, self._prev, self.len, empty, empty, self.len, self._group, self._table)
        return self._advance(n)

    def _quantize_previous(self) -> None:
        """Without the fused kernel: what the reference's quantize-the-cache does NEW work on, the previous step's entries."""
        a, b = self._prev, self.len
        if b > a:
            self.k[:, a:b].copy_(quantize_kv(self.k[:, a:b].contiguous(), self.kv_bit))
            self.v[:, a:b].copy_(quantize_kv(self.v[:, a:b].contiguous(), self.kv_bit))

    def _advance(self, n: int) -> Tuple[torch.Tensor, torch.Tensor]:
        self._prev = self.len
        self.len += n
        return self.k[:, :self.len], self.v[:, :self.len]

    @torch.no_grad()
    def append(self, k: torch.Tensor, v: torch.Tensor) -> Tuple[torch.Tensor, torch.Tensor]:
        """k, v: [B, n, H, c] (views of a fused qkv output are fine).  Returns the K / V attention runs on at this
        step: everything older than the previous step's entries as quantized before, the previous step's entries
        quantized now, the new ones as they are - what the reference's quantize-then-concatenate produces."""
        n = k.shape[1]
        assert self.len + n <= self.k.shape[1], "IncrementalKVCache: max_len exceeded"
        if self._group is not None and k.dtype == v.dtype == torch.float16 and ops.rows_viewable(k, v):
            ops.kv_cache_step(self.kv, self._prev, self.len, k, v, self.len, self._group, self._table)
        else:
            self._quantize_previous()
            self.k[:, self.len:self.len + n].copy_(k)
            self.v[:, self.len:self.len + n].copy_(v)
        return self._advance(n)

    @torch.no_grad()
    def append_qk_norm(self, q: torch.Tensor, k: torch.Tensor, v: torch.Tensor, head_scale: torch.Tensor,
                       bias: Optional[torch.Tensor] = None) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor]:
        """`append` for a block with attn_l2_norm, q / k / v the fp16 [B, n, H, 64] parts of mat_qkv's output WITHOUT its bias
        (views of one qkv tensor are fine): adds the fp32 bias [3C] (q_bias, 0, v_bias, or None), L2-normalizes k per head on
        its way into the cache and returns (q normalized and scaled by head_scale - qk_norm_head_scale -, K, V) - one launch
        (fpq_kv_cache_step_qknorm, include/fpq.h holds the numerics)."""
        n = k.shape[1]
        assert self.len + n <= self.k.shape[1], "IncrementalKVCache: max_len exceeded"
        if self._group not in (64, 128) or self.k.shape[-1] != 64:
            raise RuntimeError("IncrementalKVCache.append_qk_norm: needs an fp16 cache with head_dim 64 (kv_bit 6 or 4)")
        if not ops.rows_viewable(q, k, v):
            q, k, v = q.contiguous(), k.contiguous(), v.contiguous()
        qn = ops.kv_cache_step_qk_norm(self.kv, self._prev, self.len, q, k, v, self.len, self._group, self._table, head_scale, bias)
        return (qn, *self._advance(n))

    def slots(self, n: int) -> Tuple[torch.Tensor, int]:
        assert self.len + n <= self.k.shape[1], "IncrementalKVCache: max_len exceeded"
        return self.kv, self.len

    def _attend(self, q: torch.Tensor, K: torch.Tensor, V: torch.Tensor, scale: float) -> torch.Tensor:
        return (self._attention or ops.attention_blhc)(q, K, V, scale)

    def attend(self, q: torch.Tensor, k: torch.Tensor, v: torch.Tensor, scale: float) -> torch.Tensor:
        return self._attend(q, *self.append(k, v), scale)

    def attend_written(self, q: torch.Tensor, n: int, scale: float) -> torch.Tensor:
        return self._attend(q, *self.commit_written(n), scale)

    def attend_qk_norm(self, q: torch.Tensor, k: torch.Tensor, v: torch.Tensor, head_scale: torch.Tensor, bias: Optional[torch.Tensor], scale: float):
        return self._attend(*self.append_qk_norm(q, k, v, head_scale, bias), scale)


def _e2m3_levels() -> torch.Tensor:
    """The 64 OCP E2M3 codes' values (sign bit 5, exponent bits 4..3, mantissa bits 2..0), fp32."""
    c = torch.arange(64)
    e, m = (c >> 3) & 3, (c & 7).float()
    mag = torch.where(e == 0, m / 8, (1 + m / 8) * torch.exp2((e - 1).float()))
    return torch.where(c >= 32, -mag, mag)


def _e2m1_levels() -> torch.Tensor:
    """The 16 OCP E2M1 codes' values (sign bit 3, exponent bits 2..1, mantissa bit 0), fp32."""
    c = torch.arange(16)
    e, m = (c >> 1) & 3, (c & 1).float()
    mag = torch.where(e == 0, m / 2, (1 + m / 2) * torch.exp2((e - 1).float()))
    return torch.where(c >= 8, -mag, mag)


class PackedKVCache:
    """The KV cache of IncrementalKVCache stored as what it holds: quantization codes + fp16 scales (include/fpq.h, "the packed
    KV cache") - 50 bytes per (token, head) row of 64 with kv_bit 6 (E2M3 codes, one scale per row), 33 with kv_bit 4 (E2M1
    nibbles, one scale per 128 elements = two heads), against 128 in fp16.

    A step is two launches (`attend`): attention over the packed entries [0, len) followed by the fresh fp16 k / v of the step
    (fpq_attention_blhc_kvcodes: the reference attends to the new k / v unquantized), then the pack of k / v into slots
    [len, len + L) (fpq_kv_pack: the quantization IncrementalKVCache applies to them at the next step).  Every attention output
    is bit for bit `ops.attention_blhc(q, *IncrementalKVCache.append(k, v), scale)`.

    `staging`: an fp16 [2, B, max_step, H, 64] slab that producers write a step's k / v into (gemm.linear_fp4_qkv_to_cache(...,
    staging, 0, L); `stage_qk_norm`) before `attend_staged` - one slab serves every block's cache, since a block's fresh entries
    are packed before the next block runs (new_staging).

    The step protocol is IncrementalKVCache's: `slots(n)` = (staging, 0), `attend`, `attend_written` = `attend_staged`,
    `attend_qk_norm` = `stage_qk_norm` + `attend_staged`.
    """

    def __init__(self, batch: int, max_len: int, heads: int, head_dim: int = 64, kv_bit: int = 6, device="cuda",
                 staging: Optional[torch.Tensor] = None):
        dev = torch.device(device)
        if dev.type != "cuda":
            raise RuntimeError(f"PackedKVCache: expected a GPU device, got {dev} (fpqvar_amd has no CPU path)")
        if head_dim != 64:
            raise RuntimeError(f"PackedKVCache: head_dim must be 64, got {head_dim}")
        if kv_bit not in (4, 6) or (kv_bit == 4 and heads % 2):
            raise RuntimeError(f"PackedKVCache: kv_bit 6, or kv_bit 4 with an even number of heads (H * 64 % 128 == 0); got {kv_bit}, H = {heads}")
        if staging is not None and (staging.dtype != torch.float16 or staging.dim() != 5 or staging.shape[0] != 2 or staging.shape[1] != batch
                                    or tuple(staging.shape[3:]) != (heads, head_dim) or not staging.is_contiguous() or staging.device != dev):
            raise RuntimeError(f"PackedKVCache: staging must be a contiguous float16 [2, {batch}, max_step, {heads}, {head_dim}] tensor on {dev}")
        self.kv_bit, self.batch, self.max_len, self.heads = kv_bit, batch, max_len, heads
        self.codes = torch.empty(2, batch, max_len, heads, 48 if kv_bit == 6 else 32, dtype=torch.uint8, device=dev)
        self.scales = torch.empty(2, batch, max_len, heads if kv_bit == 6 else heads // 2, dtype=torch.float16, device=dev)
        self.staging = staging
        self.len = 0

    @staticmethod
    def new_staging(batch: int, max_step: int, heads: int, head_dim: int = 64, device="cuda") -> torch.Tensor:
        """The fp16 [2, B, max_step, H, 64] slab a model's caches share (`staging=`)."""
        return torch.empty(2, batch, max_step, heads, head_dim, dtype=torch.float16, device=device)

    @property
    def nbytes(self) -> int:
        """Bytes of the packed slabs (codes + scales; a shared staging slab is not counted)."""
        return self.codes.numel() + 2 * self.scales.numel()

    @torch.no_grad()
    def attend(self, q: torch.Tensor, k: torch.Tensor, v: torch.Tensor, scale: float) -> torch.Tensor:
        """softmax(q K^T * scale) V over the packed entries and the fresh k / v [B, L, H, 64] (views of a fused qkv output are
        fine), then k / v packed into slots [len, len + L): out fp16 [B, L, H, 64]."""
        n = k.shape[1]
        if self.len + n > self.max_len:
            raise RuntimeError("PackedKVCache: max_len exceeded")
        out = ops.attention_blhc_kvcodes(q, self.codes, self.scales, self.kv_bit, self.len, k, v, scale)
        ops.kv_pack(self.codes, self.scales, self.kv_bit, self.len, k, v)
        self.len += n
        return out

    def staged(self, n: int) -> Tuple[torch.Tensor, torch.Tensor]:
        """The views [B, n, H, 64] of the staging slab's first n tokens (k, v)."""
        if self.staging is None:
            raise RuntimeError("PackedKVCache: no staging slab (staging=)")
        if n > self.staging.shape[2]:
            raise RuntimeError(f"PackedKVCache: {n} tokens do not fit the staging slab's {self.staging.shape[2]}")
        return self.staging[0, :, :n], self.staging[1, :, :n]

    @torch.no_grad()
    def attend_staged(self, q: torch.Tensor, n: int, scale: float) -> torch.Tensor:
        """`attend` on the k / v a producer wrote into the staging slab's first n tokens."""
        return self.attend(q, *self.staged(n), scale)

    @torch.no_grad()
    def stage_qk_norm(self, q: torch.Tensor, k: torch.Tensor, v: torch.Tensor, head_scale: torch.Tensor,
                      bias: Optional[torch.Tensor] = None) -> torch.Tensor:
        """IncrementalKVCache.append_qk_norm's producer into the staging slab (fpq_kv_cache_step_qknorm with nothing to quantize):
        k normalized and v (+ bias) land in the slab's first n tokens, q normalized and scaled comes back; `attend_staged` next."""
        if self.staging is None:
            raise RuntimeError("PackedKVCache: no staging slab (staging=)")
        if not ops.rows_viewable(q, k, v):
            q, k, v = q.contiguous(), k.contiguous(), v.contiguous()
        return ops.kv_cache_step_qk_norm(self.staging, 0, 0, q, k, v, 0, 64, "e2m3", head_scale, bias)

    def slots(self, n: int) -> Tuple[torch.Tensor, int]:
        self.staged(n)   # its refusals
        return self.staging, 0

    attend_written = attend_staged

    def attend_qk_norm(self, q: torch.Tensor, k: torch.Tensor, v: torch.Tensor, head_scale: torch.Tensor, bias: Optional[torch.Tensor], scale: float):
        return self.attend_staged(self.stage_qk_norm(q, k, v, head_scale, bias), k.shape[1], scale)

    @torch.no_grad()
    def dequantize(self) -> Tuple[torch.Tensor, torch.Tensor]:
        """(K, V) fp16 [B, len, H, 64]: the packed entries decoded as include/fpq.h defines them, (half)(level * scale) - for
        tests and debugging (torch ops, not a hot path)."""
        B, H, n = self.batch, self.heads, self.len
        c = self.codes[:, :, :n].to(torch.int32)
        if self.kv_bit == 6:   # 3 bytes = 4 codes, little-endian
            c = c.view(2, B, n, H, 16, 3)
            w = c[..., 0] | (c[..., 1] << 8) | (c[..., 2] << 16)
            idx = torch.stack([(w >> (6 * i)) & 63 for i in range(4)], dim=-1).view(2, B, n, H, 64)
            lv = _e2m3_levels().to(c.device)[idx.long()]
            sc = self.scales[:, :, :n].float().unsqueeze(-1)
        else:                  # element 2i in the low nibble of byte i; one scale per two heads
            idx = torch.stack([c & 15, c >> 4], dim=-1).view(2, B, n, H, 64)
            lv = _e2m1_levels().to(c.device)[idx.long()]
            sc = self.scales[:, :, :n].float().repeat_interleave(2, dim=3).unsqueeze(-1)
        kv = (lv * sc).half()   # the fp32 product of a 4-bit and an 11-bit significand is exact: one rounding
        return kv[0], kv[1]
