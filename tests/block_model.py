"""A plain float64 model of one scale step of the reference's quantized AdaLN blocks: the independent statement that the three
paths of GenerationBatch.step (R, F, Q) are held to.  CPU only.

Written from the reference's text, not from fpqvar_amd/var_block.py, and held to the reference's blocks RUNNING by
tests/test_block_reference_host.py (tests/golden/reference_blocks*.npz: in fp32 the model reproduces the executed reference to
float32 round-off).  tr/ = models_fp_quant_transform_rotate/:
  block      tr/basic_var.py:253-269   gamma1, gamma2, scale1, scale2, shift1, shift2;  x_1 = (LN(x) (1 + scale1) + shift1) s_qkv . Q,
                                       x = x + attn(x_1) gamma1;  x_2 = (LN(x) (1 + scale2) + shift2) s_fc1 . Q,  x = x + ffn(x_2) gamma2
  attention  tr/basic_var.py:136-142   softmax scale 0.25 / sqrt(head_dim); under attn_l2_norm 1, with scale_mul_1H11 clamped at log 100
             tr/basic_var.py:166-211   qkv = mat_qkv(x) + (q_bias, 0, v_bias); q, k normalized per head, q times exp(scale_mul); the WHOLE
                                       cache re-quantized (kv_bit 6: E2M3, one scale per row of head_dim = 64) before the step's k / v
                                       are appended; attention over cache + step
  FFN        tr/basic_var.py:120-121   fc2(gelu_tanh(fc1(x)))
  Linear     tr/quant_utils.py:764-769 act_quant on the input, then the fp16 Linear on the fake-quantized weight
  quantizers oracle/fpq_oracle.py      W4A4: per-group(128) E2M1, fc2's input the dual E1M2- / E2M1+ with the global clamp;
                                       W6A6: per-token E2M3, fc2's input INT- / E2M3+ without a clamp

Arithmetic is float64.  A value is rounded to fp16 once wherever the reference (under its fp16 autocast, with the fp16 residual
stream of the generation harness) holds an fp16 tensor: scale + 1 (an fp16 add), the modulated row and the rotation matrix as the
fp16 matmul casts them, the rotated row (half(h) . half(Q) exactly, rounded once: oracle.rotate_fp16_reference), every quantizer's
input and output (the oracle's *_kernel_sem on fp16 tensors), every Linear's output, the attention output, GELU's output and the
residual stream after each x + y gamma.  Float64 stays where the reference holds fp32: LayerNorm, modulate and smoothing; under
attn_l2_norm the biased qkv, the normalized q / k, v and the cache (whose quantizer still hard-casts its result to fp16,
tr/quant_utils.py:516).

Each wiring mutant (MUTANTS) is one line of `step` / `_producer` / `_attention`: what a plausible mistake in a path's host code
would compute instead.  `deviation` measures a path against the model relative to what the steps ADD to the residual stream.
"""
import math
from dataclasses import dataclass
from typing import Dict, List, Optional, Sequence

import torch

from oracle import fpq_oracle as orc
from tests.gelu_model import reference as gelu_tanh          # the one float64 GELU(tanh) the kernel tests are held to as well

MUTANTS = (
    "swap_sc_sh",                    # 1  (scale1, shift1) <-> (scale2, shift2)
    "swap_gates",                    # 2  gamma1 <-> gamma2
    "swap_smooth_act",               # 3  s_qkv <-> s_fc1 on the activation side only
    "scale_without_one",             # 4  mul(scale) instead of mul(1 + scale)
    "ffn_residual_on_block_input",   # 5  x_in + ffn(..) gamma2: the attention update is lost
    "blocks_swap_modulation",        # 6  block b runs with block b + 1's modulation (depth 2: each other's)
    "own_keys_only",                 # 7  attention over the step's own k / v only
    "cache_shifted_by_one",          # 8  attention reads the cached entries from position 1 on (the oldest entry is missed)
    "block1_reads_cache0",           # 9  block 1 takes the earlier steps' K / V from block 0's cache
    "attention_scale_swapped",       # 10 the other regime's softmax scale: plain 1, attn_l2_norm 0.25 / sqrt(head_dim)
    "bias_dropped",                  # 11 attn_l2_norm: q_bias / v_bias not added
    "clamp_dropped",                 # 12 attn_l2_norm: scale_mul not clamped at log 100
    "kv_quant_skipped",              # 13 the cache is never quantized
    "activation_not_rotated",        # 14 the online rotation is skipped (the weights stay rotated)
    "fc2_input_symmetric",           # 15 fc2's input through the other Linears' symmetric quantizer
)
MAX_SCALE_MUL = float(torch.log(torch.tensor(100)))          # tr/basic_var.py:140
EPS = 1e-6                                                   # norm_layer = partial(nn.LayerNorm, eps=1e-6)

# the config rows (run.sh): the symmetric activation quantizer, fc2's input quantizer and the weights' quantizer, on fp16 / fp32 tensors
CONFIGS = {
    "w4a4": dict(act=lambda t: orc.per_group_kernel_sem(t, "e2m1", 128),
                 fc2=lambda t: orc.dual_per_group_kernel_sem(t, "e1m2_neg", "e2m1_pos", 128, clipping_strength=1.0),
                 weight=lambda w: orc.per_group_kernel_sem(w, "e2m1", 128).half()),
    "w6a6": dict(act=lambda t: orc.per_token_kernel_sem(t, "e2m3"),
                 fc2=lambda t: orc.dual_per_token_kernel_sem(t, "int_neg", "e2m3_pos"),
                 weight=lambda w: orc.per_token_kernel_sem(w, "e2m3")),
}


@dataclass
class BlockParams:
    """Everything a step depends on, as plain CPU tensors.  w: "qkv" [3C, C], "proj" [C, C], "fc1" [hidden, C], "fc2" [C, hidden],
    the fake-quantized weights (one set shared by every block, as GenerationBatch has it); mods: per block (gamma1, gamma2, scale1,
    scale2, shift1, shift2), each fp16 [B, 1, C]; s_qkv / s_fc1 [C] and Q [C, C]: activation-side smoothing and rotation (None: not
    applied); scale_mul (per block [1, H, 1, 1]) and qkv_bias (per block [3C]) select attn_l2_norm when given.  ideal: no quantizer
    and no fp16 rounding anywhere - the block in exact arithmetic, for the compensation check.  fp32: the quantizers stay (on fp32
    tensors) and the fp16 roundings go - what the reference holds when it runs without autocast on fp32 inputs; w is then the
    weight quantizer's fp32 output (the KV quantizer's result is fp16 even so, tr/quant_utils.py:516)."""
    C: int
    H: int
    config: str
    w: Dict[str, torch.Tensor]
    mods: List[Sequence[torch.Tensor]]
    s_qkv: Optional[torch.Tensor] = None
    s_fc1: Optional[torch.Tensor] = None
    Q: Optional[torch.Tensor] = None
    scale_mul: Optional[List[torch.Tensor]] = None
    qkv_bias: Optional[List[torch.Tensor]] = None
    ideal: bool = False
    fp32: bool = False


def params_of(gb) -> BlockParams:
    """The record of a fpqvar_amd.var_block.GenerationBatch - the only place that touches the product."""
    cpu = lambda t: t.detach().cpu()
    l2 = bool(gb.attn_l2_norm)
    return BlockParams(C=gb.C, H=gb.H, config=gb.config, w={n: cpu(w) for n, w in gb.wq.items()},
                       mods=[[cpu(t) for t in m] for m in gb.mods], s_qkv=cpu(gb.s_qkv), s_fc1=cpu(gb.s_fc1), Q=cpu(gb.q32),
                       scale_mul=[cpu(t) for t in gb.scale_mul] if l2 else None,
                       qkv_bias=[cpu(t) for t in gb.qkv_bias] if l2 else None)


def deviation(y, y_model, x) -> float:
    """||y - y_model|| / ||y_model - x|| over ALL elements of the given step outputs together (tensors or lists of tensors, one per
    step): the error relative to what the steps add to the residual stream."""
    flat = lambda t: torch.cat([s.detach().cpu().double().reshape(-1) for s in (t if isinstance(t, (list, tuple)) else [t])])
    y, y_model, x = flat(y), flat(y_model), flat(x)
    return float((y - y_model).norm() / (y_model - x).norm())


class BlockModel:
    """`depth = len(params.mods)` blocks with their KV caches; `step` advances every cache by the step's tokens."""

    def __init__(self, params: BlockParams):
        p = self.p = params
        assert p.config in CONFIGS and p.C % p.H == 0
        self.depth, self.hd, self.l2 = len(p.mods), p.C // p.H, p.scale_mul is not None
        self.w = {n: w.double() for n, w in p.w.items()}
        self.s = {"qkv": None if p.s_qkv is None else p.s_qkv.double(), "fc1": None if p.s_fc1 is None else p.s_fc1.double()}
        self.Q = None if p.Q is None else self._r(p.Q.double())          # the fp16 matmul's cast of Q
        self.caches: List[Optional[tuple]] = [None] * self.depth

    # ---- roundings and quantizers ------------------------------------------------------------------------------------------------
    def _r(self, t: torch.Tensor) -> torch.Tensor:
        """where the reference holds an fp16 tensor"""
        return t if self.p.ideal or self.p.fp32 else t.half().double()

    def _quant(self, which: str, t: torch.Tensor) -> torch.Tensor:
        if self.p.ideal:
            return t
        return CONFIGS[self.p.config][which](t.float() if self.p.fp32 else t.half()).double()

    def quantize_cache(self, t: torch.Tensor) -> torch.Tensor:
        """fp6_quant_e2m3_per_token_cuda on a cached K or V [B, n, H, head_dim] (tr/basic_var.py:194-195): an fp16 cache in the plain
        regime, an fp32 one (here float64) under attn_l2_norm; the result is fp16 either way."""
        if self.p.ideal:
            return t
        return orc.per_token_kernel_sem(t if self.l2 else t.float() if self.p.fp32 else t.half(), "e2m3").double()

    def _linear(self, t: torch.Tensor, name: str) -> torch.Tensor:
        return self._r(t @ self.w[name].T)

    # ---- the pieces of a block -----------------------------------------------------------------------------------------------------
    def _producer(self, x, scale, shift, s, m):
        """(LN(x) (1 + scale) + shift) s . Q as the Linear's act_quant receives it"""
        mu = x.mean(dim=-1, keepdim=True)
        ln = (x - mu) / torch.sqrt(((x - mu) ** 2).mean(dim=-1, keepdim=True) + EPS)
        one_plus = (scale.double() + 1.0) if self.p.ideal or self.p.fp32 else (scale + 1).double()   # scale1.add(1): an fp16 add
        h = ln * (scale.double() if m == "scale_without_one" else one_plus) + shift.double()
        h = self._r(h if s is None else h * s)
        return h if self.Q is None or m == "activation_not_rotated" else self._r(h @ self.Q)

    def _attention(self, qkv, b, m):
        p, H, hd = self.p, self.p.H, self.hd
        B, L = qkv.shape[0], qkv.shape[1]
        if self.l2:
            bias = p.qkv_bias[b].double() * (0.0 if m == "bias_dropped" else 1.0)
            q, k, v = (qkv + bias).view(B, L, 3, H, hd).unbind(2)
            sm = p.scale_mul[b].double() if m == "clamp_dropped" else p.scale_mul[b].double().clamp_max(MAX_SCALE_MUL)
            q = q / q.norm(dim=-1, keepdim=True).clamp_min(1e-12) * sm.exp().view(1, 1, H, 1)          # F.normalize, 1H11 -> 11H1
            k = k / k.norm(dim=-1, keepdim=True).clamp_min(1e-12)
        else:
            q, k, v = qkv.view(B, L, 3, H, hd).unbind(2)
        scale = 1.0 if self.l2 != (m == "attention_scale_swapped") else 0.25 / math.sqrt(hd)
        old = self.caches[b]
        if old is not None and m != "kv_quant_skipped":
            old = (self.quantize_cache(old[0]), self.quantize_cache(old[1]))
        K, V = (k, v) if old is None else (torch.cat((old[0], k), dim=1), torch.cat((old[1], v), dim=1))
        self.caches[b] = (K, V)
        if old is not None and m == "own_keys_only":
            K, V = k, v
        if old is not None and m == "cache_shifted_by_one":
            K, V = K[:, 1:], V[:, 1:]
        if old is not None and m == "block1_reads_cache0" and b == 1:
            n = old[0].shape[1]
            K, V = torch.cat((self.caches[0][0][:, :n], k), dim=1), torch.cat((self.caches[0][1][:, :n], v), dim=1)
        prob = torch.softmax(torch.einsum("blhc,bmhc->bhlm", q, K) * scale, dim=-1)
        return self._r(torch.einsum("bhlm,bmhc->blhc", prob, V).reshape(B, L, p.C))

    # ---- one scale step -------------------------------------------------------------------------------------------------------------
    def step(self, x: torch.Tensor, mutate: Optional[str] = None) -> torch.Tensor:
        """x [B, L, C] (fp16 values) -> the residual stream after `depth` blocks, float64 holding fp16 values.  A mutated model is
        its own instance from the first step on: its caches hold what the mutant wrote."""
        m = mutate
        assert m is None or m in MUTANTS, m
        x = x.detach().cpu().double()
        for b in range(self.depth):
            g1, g2, sc1, sc2, sh1, sh2 = self.p.mods[(b + 1) % self.depth if m == "blocks_swap_modulation" else b]
            if m == "swap_sc_sh":
                sc1, sh1, sc2, sh2 = sc2, sh2, sc1, sh1
            if m == "swap_gates":
                g1, g2 = g2, g1
            s1, s2 = (self.s["fc1"], self.s["qkv"]) if m == "swap_smooth_act" else (self.s["qkv"], self.s["fc1"])
            x_in = x
            qkv = self._linear(self._quant("act", self._producer(x, sc1, sh1, s1, m)), "qkv")
            a = self._linear(self._quant("act", self._attention(qkv, b, m)), "proj")
            x = self._r(x + a * g1.double())
            f = self._r(gelu_tanh(self._linear(self._quant("act", self._producer(x, sc2, sh2, s2, m)), "fc1")))
            y = self._linear(self._quant("act" if m == "fc2_input_symmetric" else "fc2", f), "fc2")
            x = self._r((x_in if m == "ffn_residual_on_block_input" else x) + y * g2.double())
        return x


def run(params: BlockParams, xs: Sequence[torch.Tensor], mutate: Optional[str] = None) -> List[torch.Tensor]:
    """The outputs of a fresh model over the steps xs."""
    model = BlockModel(params)
    return [model.step(x, mutate) for x in xs]


def mutant_table(params: BlockParams, xs: Sequence[torch.Tensor], base: Optional[List[torch.Tensor]] = None) -> Dict[str, float]:
    """name -> deviation of the mutated model from the unmutated one over the steps xs."""
    base = run(params, xs) if base is None else base
    return {m: deviation(run(params, xs, m), base, xs) for m in MUTANTS}
