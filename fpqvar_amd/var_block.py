"""The transformer part of one generation batch of the reference's W4A4 / W6A6 runs, at the shapes of BASELINE.json
configs 3 and 5: ten scale steps (tr/var.py:175), `depth` AdaLN blocks per step
(tr/basic_var.py:253-269), B = images x CFG rows per token, random weights (no checkpoints exist offline; every block
shares one set of weight tensors), KV cache in FP6 (run.sh:4).  Word embedding, class conditioning, sampling and the
VQVAE decoder are not part of the quantized path and are left out: this is the host logic that strings the path's
kernels together the way the model does, for the model-level figures of bench.py (`generation`) and
tools/bench_model.py - the VAR model itself stays the reference's vendored code.

Three ways to run everything around the attention core:
  R  the reference's own op sequence on this GPU (Level 0 of INTEGRATION.md): its ~11 torch ops per quantizer around
     quant_cuda.quant (tr/quant_utils.py:313-330,415-452,503-517), the dense fp16 GEMM with the block-diagonal Q
     (tr/basic_var.py:263,266), fp16 Linears on de-quantized tensors (tr/quant_utils.py:767), the whole KV cache
     re-quantized at every step (tr/basic_var.py:186-209)
  F  one launch per quantizer, the fused LayerNorm / modulate / smooth / rotate / quant producer, incremental KV cache, GELU
     fused in front of fc2's input quantizer, attention by fpq_attention_blhc off the cache views (the reference calls
     flash_attn_func there, tr/basic_var.py:211; rounds 1 - 4 timed this path with torch's SDPA: sdpa_in_f=True); the Linears
     stay fp16 GEMMs on fake-quantized values (the reference's numerics)
  Q  F with mat_qkv / proj / fc1 on the FP4 (W6A6: FP6) matrix cores - the producers emit the GEMM operands, proj applies
     the block's gate and residual in its epilogue, fc1 applies GELU and fc2's dual-format input quantizer in its epilogue
     (gemm.linear_fp4_gelu_dual; W4A4 only) - and attention by fpq_attention_blhc straight off the cache views
"""
from __future__ import annotations

import os
import time
from types import SimpleNamespace
from typing import Dict, List, Optional, Sequence

import torch
import torch.nn.functional as Fn

from . import gemm, kv_cache, ops, quant_utils as qu, rotation as rot

MODELS = {   # name: (heads = depth, patch_nums, rows per token = images x CFG); SURVEY.md section 8 header, configs C3 / C5
    "d30-256": (30, (1, 2, 3, 4, 5, 6, 8, 10, 13, 16), 100),
    "d36-512": (36, (1, 2, 3, 4, 6, 9, 13, 18, 24, 32), 20),
}
WHAT = {
    "d30-256": "VAR-d30 256x256, 50 images with CFG (evaluate_fp_quant_transform_rotate.py:187-199)",
    "d36-512": "VAR-d36 512x512, 10 images with CFG (evaluate_fp_quant_transform_rotate_512x512.py:54,62,192-214)",
}
PATHS = ("R", "F", "Q")
TUNED_GEMMS = os.path.join(os.path.dirname(os.path.abspath(__file__)), "tunableop_gfx950.csv")


class tuned_torch_gemms:
    """`with tuned_torch_gemms():` - torch's OWN GEMMs (fc2 on every path; every Linear and the rotation of paths F / R) pick
    their kernel from selections recorded once on an MI355X for the shapes of the two models (torch's TunableOp: the fastest of
    the hipBLASLt / rocBLAS solutions per shape; `fpqvar_amd/tunableop_gfx950.csv`, made by running tools/bench_model.py under
    PYTORCH_TUNABLEOP_TUNING=1).  Nothing is tuned at run time; a file whose validators (torch / hipBLASLt / rocBLAS versions,
    gfx950) do not match the box is ignored by torch, which then selects as it does by default."""

    def __init__(self, path: str = TUNED_GEMMS):
        self.path = path

    def __enter__(self):
        import torch.cuda.tunable as tn
        self.before = (tn.is_enabled(), tn.tuning_is_enabled())
        self.active = os.path.exists(self.path)
        if self.active:
            # torch works on a private copy: it may rewrite its results file when the process ends, and the recorded file is source
            import shutil
            import tempfile
            self.copy = os.path.join(tempfile.gettempdir(), f"fpq_tunableop_{os.getpid()}.csv")
            shutil.copyfile(self.path, self.copy)
            tn.enable(True)
            tn.tuning_enable(False)
            tn.set_filename(self.copy, False)
            self.active = bool(tn.read_file(self.copy))
            if not self.active:
                tn.enable(self.before[0])
        return self

    def __exit__(self, *exc):
        import torch.cuda.tunable as tn
        tn.enable(self.before[0])
        tn.tuning_enable(self.before[1])
        return False


def _ref_sym(x, grid, group=None, out_dtype=None):
    """fp_quant_e2_per_group_cuda / fp6_quant_e2m3_per_token_cuda as the reference spells them (tr/quant_utils.py:313-330,503-517)."""
    import quant_cuda
    shape = x.shape
    xs = x.reshape(-1, group) if group else x
    scale = xs.abs().max(dim=-1, keepdim=True)[0] / grid.abs().max()
    q, _ = quant_cuda.quant((xs / scale).view(-1).to(torch.float32), grid)
    return (q.view(xs.shape) * scale).view(shape).to(out_dtype or x.dtype)


def _ref_dual(x, gneg, gpos, group=128, clip=True):
    """fp_quant_e1m2_neg_e2m1_pos_per_group_cuda (tr/quant_utils.py:415-452; the FP6 twin :577-646 has no global clip)."""
    import quant_cuda
    if clip:
        c = 1.0 * x.abs().max()
        x = torch.clamp(x, -c, c)
    shape = x.shape
    xs = x.reshape(-1, group) if group else x
    zeros = torch.zeros_like(xs)
    xn_, xp_ = torch.where(xs <= 0, xs, zeros), torch.where(xs > 0, xs, zeros)
    sn = xn_.abs().max(dim=-1, keepdim=True)[0] / gneg.abs().max()
    sp = xp_.abs().max(dim=-1, keepdim=True)[0] / gpos.abs().max()
    qa, _ = quant_cuda.quant((xn_ / sn).view(-1).to(torch.float32), gneg)
    qb, _ = quant_cuda.quant((xp_ / sp).view(-1).to(torch.float32), gpos)
    return (qa.view(xs.shape) * sn + qb.view(xs.shape) * sp).view(shape).to(x.dtype)


def _mx_weight(w, km):
    c, sc = gemm.quantize_mx(w)
    return (gemm.to_kmajor(c, 4, dealt=True), gemm.to_kmajor_scales(sc, weight_side=True)) if km else (c, sc)


def _fp6_weight(w, km):
    c, sc = gemm.quantize_fp6(w)
    return (gemm.to_kmajor(c, 6, dealt=True), sc) if km else (c, sc)


# What differs between the two runs, one row per config; a GenerationBatch picks its row once (`self.row`).  Every entry reaches
# quant_utils / rotation / gemm through the module at call time.  r_*: (batch, t), the reference's op sequence (path R); the producers:
# (x, scale, shift, sm=smooth[, km=kmajor]), their gated-residual forms with (y, gate) in front; linear_gelu_dual: fc1 with GELU and
# fc2's quantizer in the GEMM epilogue, where the config has one.
ROWS = {
    "w4a4": SimpleNamespace(
        r_act=lambda gb, t: _ref_sym(t, gb.e2m1, 128), r_fc2=lambda gb, t: _ref_dual(t, gb.gneg, gb.gpos),
        act=lambda t: qu.fp_quant_e2_per_group_cuda(t, 4, 128),
        fc2=lambda t: qu.fp_quant_e1m2_neg_e2m1_pos_per_group_cuda(t, 4, 128),
        gelu_fc2=lambda y: qu.gelu_fp_quant_e1m2_neg_e2m1_pos_per_group_cuda(y, 4, 128),
        values=lambda *a, sm: rot.adaln_rotate_quant(*a, "e2m1", smooth=sm),
        operands=lambda *a, sm, km: rot.adaln_rotate_quant_mx(*a, smooth=sm, kmajor=km),
        resid_values=lambda *a, sm: rot.resid_adaln_rotate_quant(*a, "e2m1", smooth=sm),
        resid_operands=lambda *a, sm, km: rot.resid_adaln_rotate_quant_mx(*a, smooth=sm, kmajor=km),
        quantize=lambda t, km: gemm.quantize_mx(t, kmajor=km), linear=lambda *a: gemm.linear_fp4(*a),
        linear_split=lambda *a, **kw: gemm.linear_fp4_qkv_to_cache(*a, **kw), linear_gelu_dual=lambda *a: gemm.linear_fp4_gelu_dual(*a),
        weight=lambda w: qu.fp_quant_e2_per_group_cuda(w, 4, 128).half(), weight_operands=_mx_weight),
    "w6a6": SimpleNamespace(
        r_act=lambda gb, t: _ref_sym(t, gb.e2m3, None, torch.float16), r_fc2=lambda gb, t: _ref_dual(t, gb.ineg, gb.e2m3p, None, clip=False),
        act=lambda t: qu.fp6_quant_e2m3_per_token_cuda(t, 6),
        fc2=lambda t: qu.fp6_quant_int_neg_e2m3_pos_per_token_cuda(t, 6),
        gelu_fc2=lambda y: qu.gelu_fp6_quant_int_neg_e2m3_pos_per_token_cuda(y, 6),
        values=lambda *a, sm: rot.adaln_rotate_quant_token(*a, "e2m3", smooth=sm),
        operands=lambda *a, sm, km: rot.adaln_rotate_quant_token(*a, "e2m3", smooth=sm, emit="fp6", kmajor=km),
        resid_values=lambda *a, sm: rot.resid_adaln_rotate_quant_token(*a, "e2m3", smooth=sm),
        resid_operands=lambda *a, sm, km: rot.resid_adaln_rotate_quant_token(*a, "e2m3", smooth=sm, emit="fp6", kmajor=km),
        quantize=lambda t, km: gemm.quantize_fp6(t, kmajor=km), linear=lambda *a: gemm.linear_fp6(*a),
        linear_split=lambda *a, **kw: gemm.linear_fp6_qkv_to_cache(*a, **kw), linear_gelu_dual=None,
        weight=lambda w: qu.fp6_quant_e2m3_per_token_cuda(w, 6), weight_operands=_fp6_weight),
}
# rotation="full": Q is the dense randomized Hadamard matrix (the reference's `--rotate` without `--block_rotate`), so the two adaLN
# producers of a config's row are the full-width ones; every other entry stays.  No gated-residual full-width producer exists.
FULL_PRODUCERS = {
    "w4a4": dict(values=lambda *a, sm: rot.adaln_rotate_quant_full(*a, "e2m1", smooth=sm),
                 operands=lambda *a, sm, km: rot.adaln_rotate_quant_full_mx(*a, smooth=sm, kmajor=km)),
    "w6a6": dict(values=lambda *a, sm: rot.adaln_rotate_quant_full_token(*a, "e2m3", smooth=sm),
                 operands=lambda *a, sm, km: rot.adaln_rotate_quant_full_token(*a, "e2m3", smooth=sm, emit="fp6", kmajor=km)),
}


class GenerationBatch:
    """Weights, modulation vectors and the step function of one model-shaped batch on `device`."""

    def __init__(self, model: str = "d30-256", config: str = "w4a4", depth: Optional[int] = None,
                 batch_rows: Optional[int] = None, device=None, seed: int = 0, fused_fc1: bool = True, sdpa_in_f: bool = False,
                 kmajor: bool = True, qkv_to_cache: bool = True, attn_l2_norm: bool = False, qk_norm: str = "fused",
                 kv_storage: str = "fp16", fuse_residual: bool = False, rotation: str = "block", tensors: Optional[dict] = None):
        assert model in MODELS and config in ("w4a4", "w6a6") and qk_norm in ("fused", "torch")
        if rotation not in ("block", "full"):
            raise ValueError(f"rotation must be 'block' or 'full', got {rotation!r}")
        if rotation == "full" and fuse_residual:
            raise ValueError("rotation='full' has no gated-residual producer: not with fuse_residual")
        if kv_storage not in ("fp16", "codes"):
            raise ValueError(f"kv_storage must be 'fp16' or 'codes', got {kv_storage!r}")
        if kv_storage == "codes" and sdpa_in_f:
            raise ValueError("kv_storage='codes' attends with fpq_attention_blhc_kvcodes: not with sdpa_in_f")
        # "codes": every block's KV cache is a PackedKVCache (FP6 codes + scales, include/fpq.h) - same results, bit for bit, as the
        # fp16 IncrementalKVCache; paths F and Q only (path R keeps the reference's whole-cache loop)
        self.kv_storage = kv_storage
        self.model, self.config = model, config
        heads, self.patch_nums, rows = MODELS[model]
        dev = self.dev = torch.device("cuda", torch.cuda.current_device()) if device is None else torch.device(device)
        self.C, self.H = 64 * heads, heads
        self.HID, self.B, self.depth = 4 * self.C, batch_rows or rows, depth or heads
        self.hd = self.C // self.H
        self.max_len = sum(p * p for p in self.patch_nums)
        self.W6, self.row = config == "w6a6", ROWS[config]
        # "block": Q = 128-wide blocks (the run scripts' --block_rotate); "full": the dense randomized Hadamard matrix of size C,
        # online through the full-width producers (C in rotation.FULL_WIDTHS)
        self.rotation = rotation
        if rotation == "full":
            self.row = SimpleNamespace(**{**vars(self.row), **FULL_PRODUCERS[config], "resid_values": None, "resid_operands": None})
        self.fused_fc1 = fused_fc1 and self.row.linear_gelu_dual is not None
        self.sdpa_in_f = sdpa_in_f                              # path F with torch's SDPA instead of fpq_attention_blhc (rounds 1 - 4 timed it that way)
        self.fused_gelu_quant = fused_fc1                       # path F: GELU + fc2's input quantizer in one pass over the fc1 output
        self.kmajor = kmajor                                    # path Q: operands as k-major images (include/fpq.h): contiguous LDS-DMA pieces
        # path Q: mat_qkv writes k and v straight into the KV cache's slots (fpq_gemm_fp4_mx_split, W6A6: fpq_gemm_fp6_rows_split):
        # no copy-in pass
        self.qkv_to_cache = bool(qkv_to_cache)
        # every x = x + y.mul(gamma) whose y comes out of a torch GEMM (path F: proj's and fc2's tail, path Q: fc2's) is applied by the
        # adaLN producer that follows it (rotation.resid_adaln_rotate_quant*) instead of a launch of its own; the last block of a
        # step ends with the plain gate_residual.  Same results, bit for bit.  Off by default.
        self.fuse_residual = bool(fuse_residual)
        C, HID, B = self.C, self.HID, self.B
        # tensors: the batch's parameters from outside instead of the draws below (a recorded run of the reference, tests) - "w": the
        # four UNQUANTIZED fp32 weights qkv [3C, C], proj [C, C], fc1 [4C, C], fc2 [C, 4C] before smoothing and rotation, "s_qkv" /
        # "s_fc1" [C], "mods": per block the six [B, 1, C] fp16 tensors (gamma1, gamma2, scale1, scale2, shift1, shift2), and with
        # attn_l2_norm "scale_mul": per block [1, H, 1, 1], "qkv_bias": per block [3C] = cat(q_bias, 0, v_bias).  All or nothing;
        # without it every draw below happens as before, in the same order.
        ext = self._check_tensors(tensors, attn_l2_norm)
        g = torch.Generator(device=dev).manual_seed(seed)
        self.gen = g
        if ext is None:
            self.s_qkv = torch.rand(C, device=dev, generator=g) + 0.5
            self.s_fc1 = torch.rand(C, device=dev, generator=g) + 0.5
        else:
            self.s_qkv, self.s_fc1 = (ext[n].detach().to(dev, torch.float32).contiguous() for n in ("s_qkv", "s_fc1"))
        q64 = rot.get_orthogonal_matrix(C, device=dev) if rotation == "full" else rot.block_random_hadamard_matrix(C, 128, dev, 42)
        self.q32 = q64.float()

        def lin_w(name, o, i, smooth=None, rotate=False):
            w = torch.randn(o, i, device=dev, generator=g) * 0.02 if ext is None else ext["w"][name].detach().to(dev, torch.float32)
            assert w.shape == (o, i), f"{name}: {tuple(w.shape)}, expected {(o, i)}"
            if smooth is not None:
                w = rot.transform_weight(w, smooth)
            return rot.rotate_weight(w, q64) if rotate else w

        w32 = {"qkv": lin_w("qkv", 3 * C, C, self.s_qkv, True), "proj": lin_w("proj", C, C), "fc1": lin_w("fc1", HID, C, self.s_fc1, True),
               "fc2": lin_w("fc2", C, HID)}
        self.wq = {n: self.row.weight(w) for n, w in w32.items()}
        self.wop = {n: self.row.weight_operands(w32[n], kmajor) for n in ("qkv", "proj", "fc1")}   # operands of the matrix-core GEMMs
        del w32
        if ext is None:
            self.mods = [[(torch.randn(B, 1, C, device=dev, generator=g) * 0.2).half() for _ in range(6)] for _ in range(self.depth)]
        else:
            self.mods = [[t.detach().to(dev, torch.float16).contiguous() for t in m] for m in ext["mods"]]
            assert len(self.mods) == self.depth and all(len(m) == 6 and all(t.shape == (B, 1, C) for t in m) for m in self.mods)
        self.e2m1 = qu.fp4_e2m1_grid.to(dev)
        self.e2m3 = qu.fp6_e2m3_grid.to(dev)
        self.gneg = torch.tensor([-1.75, -1.5, -1.25, -1.0, -0.75, -0.5, -0.25, 0.0], device=dev)
        self.gpos = torch.tensor([0.0, 0.5, 1.0, 1.5, 2.0, 3.0, 4.0, 6.0], device=dev)
        self.ineg, self.e2m3p = qu.int_neg_grid.to(dev), qu.e2m3_pos_grid.to(dev)
        # attn_l2_norm (the released models' setting, tr/basic_var.py:136-140,173-183): per block a scale_mul_1H11 around log 4 with
        # head 0 above log 100 (its clamp is exercised) and the fp32 bias cat(q_bias, 0, v_bias); attention at scale 1.  Drawn from
        # a generator of their own: every other tensor is the same with and without the flag.  qk_norm: "fused" - paths F / Q
        # normalize inside the qkv-to-cache kernels; "torch" - the reference's lines between the existing kernels (A/B, tests).
        self.attn_l2_norm, self.qk_norm = attn_l2_norm, qk_norm
        if attn_l2_norm and ext is not None:
            self.scale_mul = [t.detach().to(dev, torch.float32).reshape(1, heads, 1, 1).contiguous() for t in ext["scale_mul"]]
            self.qkv_bias = [t.detach().to(dev, torch.float32).reshape(3 * C).contiguous() for t in ext["qkv_bias"]]
            assert len(self.scale_mul) == self.depth == len(self.qkv_bias)
            self.head_scale = [kv_cache.qk_norm_head_scale(sm) for sm in self.scale_mul]
        elif attn_l2_norm:
            gn = torch.Generator(device=dev).manual_seed(seed + 7919)
            self.scale_mul = []
            for _ in range(self.depth):
                sm = torch.full((1, heads, 1, 1), 4.0, device=dev).log() + 0.3 * torch.randn(1, heads, 1, 1, device=dev, generator=gn)
                sm[0, 0] = kv_cache.MAX_SCALE_MUL + 0.5
                self.scale_mul.append(sm)
            self.head_scale = [kv_cache.qk_norm_head_scale(sm) for sm in self.scale_mul]
            self.qkv_bias = [torch.cat((torch.randn(C, device=dev, generator=gn) * 0.1, torch.zeros(C, device=dev),
                                        torch.randn(C, device=dev, generator=gn) * 0.1)) for _ in range(self.depth)]

    @staticmethod
    def _check_tensors(tensors, attn_l2_norm):
        """the `tensors` argument, complete, or None"""
        if tensors is None:
            return None
        need = {"w", "s_qkv", "s_fc1", "mods"} | ({"scale_mul", "qkv_bias"} if attn_l2_norm else set())
        if not need <= set(tensors) or set(tensors["w"]) != {"qkv", "proj", "fc1", "fc2"}:
            raise ValueError(f"tensors must hold {sorted(need)}, and w the four weights qkv, proj, fc1, fc2")
        return tensors

    # ---- the quantizers and Linears of paths F and Q, through the config's row --------------------------------------------------
    def act_then_fc2_quant(self, y):
        """`fc2.act_quant(act(y))` for an fc1 output y: one pass (GELU in front of the dual quantizer) or GELU, then the quantizer."""
        return self.row.gelu_fc2(y) if self.fused_gelu_quant else self.row.fc2(Fn.gelu(y, approximate="tanh"))

    def q_operands(self, t, sc, sh, sm):
        return self.row.operands(t, sc, sh, sm=sm, km=self.kmajor)

    def resid_producer(self, path, pend, x, sc, sh, sm):
        """fuse_residual: the pending x + y.mul(gate), pend = (y, gate), and the producer behind it in one launch.  Returns
        (x_new, what the path's producer returns for x_new): path F - the quantized values, path Q - (codes, scales)."""
        if path == "F":
            return self.row.resid_values(*pend, x, sc, sh, sm=sm)
        x_new, *operands = self.row.resid_operands(*pend, x, sc, sh, sm=sm, km=self.kmajor)
        return x_new, tuple(operands)

    def q_producer_linear(self, t, sc, sh, sm, name, operands=None):
        """operands: the producer's output when it has run already (fuse_residual)"""
        return self.row.linear(*(operands or self.q_operands(t, sc, sh, sm)), *self.wop[name])

    def q_qkv_to_cache(self, x, sc1, sh1, b, cache_kv, pos, operands=None):
        """mat_qkv of block b with the split output: q [B, L, H, hd] comes back, k and v land in cache_kv at pos (with attn_l2_norm:
        normalized in the GEMM's epilogue)"""
        bias, hs = (self.qkv_bias[b], self.head_scale[b]) if self.attn_l2_norm else (None, None)
        q = self.row.linear_split(*(operands or self.q_operands(x, sc1, sh1, self.s_qkv)), *self.wop["qkv"], bias, cache_kv, pos, x.shape[1],
                                  qk_norm_scale=hs)
        return q.view(self.B, x.shape[1], self.H, self.hd)

    def q_proj(self, t2d, gate, resid):       # x + proj(a).mul(gamma1), gate and residual applied in the GEMM epilogue
        return self.row.linear(*self.row.quantize(t2d, self.kmajor), *self.wop["proj"], None, gate, resid)

    @property
    def attn_scale(self):
        """SelfAttention.scale (tr/basic_var.py:137-142): 1 under attn_l2_norm, else 0.25 / sqrt(head_dim) - not SDPA's head_dim ** -0.5"""
        return 1.0 if self.attn_l2_norm else 0.25 * self.hd ** -0.5

    def attend(self, q, kc, vc, scale=None):   # q [B,L,H,c]; kc, vc [B,Ltot,H,c] (flash layout, as the KV runs use)
        if scale is None:
            scale = self.attn_scale
        o = Fn.scaled_dot_product_attention(q.transpose(1, 2), kc.transpose(1, 2), vc.transpose(1, 2), scale=scale)
        return o.transpose(1, 2).reshape(q.shape[0], q.shape[1], self.C)

    def qk_norm_torch(self, qkv, b):
        """the reference's lines (tr/basic_var.py:173-183, flash layout) on an fp16 qkv [B, L, 3C] without its bias: fp32 q, k, v"""
        B, L = qkv.shape[0], qkv.shape[1]
        q, k, v = (qkv + self.qkv_bias[b]).view(B, L, 3, self.H, self.hd).unbind(2)
        scale_mul = self.scale_mul[b].clamp_max(kv_cache.MAX_SCALE_MUL).exp().transpose(1, 2)   # 1H11 -> 11H1
        return Fn.normalize(q, dim=-1).mul(scale_mul), Fn.normalize(k, dim=-1), v

    def new_caches(self, path):
        """One cache per block; both classes offer the step protocol that `attention_half` runs against (kv_cache.py)."""
        if path == "R":
            if self.kv_storage == "codes":
                raise ValueError("kv_storage='codes' runs on paths F and Q; path R is the reference's own cache loop")
            return [None] * self.depth
        if self.kv_storage == "codes":   # one staging slab for the step's fresh k / v, shared by every block's cache
            staging = kv_cache.PackedKVCache.new_staging(self.B, max(p * p for p in self.patch_nums), self.H, self.hd, self.dev)
            return [kv_cache.PackedKVCache(self.B, self.max_len, self.H, self.hd, 6, self.dev, staging) for _ in range(self.depth)]
        sdpa = (lambda q, k, v, scale: self.attend(q, k, v, scale).view(q.shape)) if path == "F" and self.sdpa_in_f else None
        return [kv_cache.IncrementalKVCache(self.B, self.max_len, self.H, self.hd, 6, device=self.dev, attention=sdpa) for _ in range(self.depth)]

    def new_input(self, pn):
        return torch.randn(self.B, pn * pn, self.C, device=self.dev, generator=self.gen).half()

    def attention_half(self, path, cache, x, b, scale, prod=None):
        """The attention half of block b against the cache's step protocol: mat_qkv writes k / v into the cache's slots (path Q with
        the split output), or a plain mat_qkv and k / v handed over - as they are, through the fused q / k norm, or after the
        reference's torch lines.  Returns [B, L, H, 64].  prod: the first producer's output when it has run already (fuse_residual)."""
        B, L, H, hd = self.B, x.shape[1], self.H, self.hd
        g1, g2, sc1, sc2, sh1, sh2 = self.mods[b]
        l2 = self.attn_l2_norm
        if path == "Q" and self.qkv_to_cache and not (l2 and self.qk_norm == "torch"):
            return cache.attend_written(self.q_qkv_to_cache(x, sc1, sh1, b, *cache.slots(L), prod), L, scale)
        if path == "F":
            qkv = Fn.linear(self.row.values(x, sc1, sh1, sm=self.s_qkv) if prod is None else prod, self.wq["qkv"])
        else:
            qkv = self.q_producer_linear(x, sc1, sh1, self.s_qkv, "qkv", prod)
        if l2 and self.qk_norm == "torch":
            return cache.attend(*(t.half() for t in self.qk_norm_torch(qkv.view(B, L, 3 * self.C), b)), scale)
        q, k, v = qkv.view(B, L, 3, H, hd).unbind(2)
        return cache.attend_qk_norm(q, k, v, self.head_scale[b], self.qkv_bias[b], scale) if l2 else cache.attend(q, k, v, scale)

    # ---- one scale step: `depth` blocks over x [B, pn^2, C] ----------------------------------------------------------
    def step(self, path, caches, x):
        B, C, H, hd, HID = self.B, self.C, self.H, self.hd, self.HID
        L = x.shape[1]
        pend = None   # fuse_residual: (y, gate) of an x = x + y.mul(gate) that the next producer applies
        for b in range(self.depth):
            g1, g2, sc1, sc2, sh1, sh2 = self.mods[b]
            if path == "R":
                with torch.autocast("cuda", dtype=torch.float16):
                    x1 = torch.matmul(Fn.layer_norm(x, (C,), eps=1e-6).mul(sc1.add(1)).add_(sh1).mul(self.s_qkv), self.q32)
                    if self.attn_l2_norm:                      # fp32 q, k, v (the fp32 bias promotes) and an fp32 cache, as the reference
                        q, k, v = self.qk_norm_torch(Fn.linear(self.row.r_act(self, x1), self.wq["qkv"]), b)
                    else:
                        q, k, v = Fn.linear(self.row.r_act(self, x1), self.wq["qkv"]).view(B, L, 3, H, hd).unbind(2)
                    cache_dtype = None if self.attn_l2_norm else torch.float16
                    if caches[b] is None:
                        kc, vc = k, v
                    else:                                        # tr/basic_var.py:186-209: whole cache, every step
                        ck, cv = caches[b]
                        ck = _ref_sym(ck.contiguous(), self.e2m3, None, cache_dtype)
                        cv = _ref_sym(cv.contiguous(), self.e2m3, None, cache_dtype)
                        kc, vc = torch.cat((ck, k), dim=1), torch.cat((cv, v), dim=1)
                    caches[b] = (kc, vc)
                    a = Fn.linear(self.row.r_act(self, self.attend(q, kc, vc)), self.wq["proj"])
                    x = x + a.mul(g1)
                    x2 = torch.matmul(Fn.layer_norm(x, (C,), eps=1e-6).mul(sc2.add(1)).add_(sh2).mul(self.s_fc1), self.q32)
                    h = Fn.gelu(Fn.linear(self.row.r_act(self, x2), self.wq["fc1"]), approximate="tanh")
                    x = x + Fn.linear(self.row.r_fc2(self, h), self.wq["fc2"]).mul(g2)
                continue
            scale = self.attn_scale
            prod = None
            if pend is not None:   # the previous block's fc2 tail, applied by this block's first producer
                x, prod = self.resid_producer(path, pend, x, sc1, sh1, self.s_qkv)
                pend = None
            a = self.attention_half(path, caches[b], x, b, scale, prod).view(B, L, C)
            if path == "F":
                proj = Fn.linear(self.row.act(a), self.wq["proj"])
                if self.fuse_residual:   # proj's tail, applied by the fc1 producer
                    x, h2 = self.resid_producer(path, (proj, g1), x, sc2, sh2, self.s_fc1)
                else:
                    x = ops.gate_residual(proj, g1, x)
                    h2 = self.row.values(x, sc2, sh2, sm=self.s_fc1)
                hq = self.act_then_fc2_quant(Fn.linear(h2, self.wq["fc1"]))
            else:
                x = self.q_proj(a.view(B * L, C), g1, x).view(B, L, C)
                if self.fused_fc1:   # fc2's quantized input straight out of the fc1 GEMM
                    hq = self.row.linear_gelu_dual(*self.q_operands(x, sc2, sh2, self.s_fc1), *self.wop["fc1"]).view(B, L, HID)
                else:
                    hq = self.act_then_fc2_quant(self.q_producer_linear(x, sc2, sh2, self.s_fc1, "fc1").view(B, L, HID))
            if self.fuse_residual and b + 1 < self.depth:
                pend = (Fn.linear(hq, self.wq["fc2"]), g2)
            else:
                x = ops.gate_residual(Fn.linear(hq, self.wq["fc2"]), g2, x)
        return x

    # ---- timing ----------------------------------------------------------------------------------------------------
    def run_eager(self, path) -> float:
        """ms for the ten steps launched eagerly (host launch costs included)."""
        caches = self.new_caches(path)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for pn in self.patch_nums:
            self.step(path, caches, self.new_input(pn))
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3

    def capture(self, path):
        """One hipGraph per scale step (static shapes), captured in step order so that the KV-cache bookkeeping on the
        host advances exactly as in an eager run; a batch is then ten graph launches."""
        caches = self.new_caches(path)
        pool = torch.cuda.graph_pool_handle()
        graphs, keep = [], [caches]
        for pn in self.patch_nums:
            x = self.new_input(pn)
            g = torch.cuda.CUDAGraph()
            with torch.cuda.graph(g, pool=pool):
                y = self.step(path, caches, x)
            graphs.append(g)
            keep.append((x, y))
        return graphs, keep

    @staticmethod
    def replay(graphs) -> float:
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for g in graphs:
            g.replay()
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3

    def time_path(self, path, reps: int = 3, graphs: bool = True) -> Dict[str, float]:
        """One eager warm-up batch (allocator, kernel load), then - graphs: capture + best of `reps` replays; eager: best of
        `reps` eager batches."""
        out = {"warmup_eager_ms": round(self.run_eager(path), 1)}
        torch.cuda.empty_cache()
        if graphs:
            gr, keep = self.capture(path)
            self.replay(gr)                                                  # first replay: graph upload
            out["ms_per_batch"] = round(min(self.replay(gr) for _ in range(reps)), 2)
            out["clock"] = "ten hipGraph replays (one per scale step), host wall clock around them, best of %d" % reps
            del gr, keep
        else:
            out["ms_per_batch"] = round(min(self.run_eager(path) for _ in range(reps)), 2)
            out["clock"] = "eager launches, host wall clock, best of %d" % reps
        torch.cuda.empty_cache()
        out["images_per_s"] = round((self.B // 2) / (out["ms_per_batch"] / 1e3), 1)
        return out

    def describe(self) -> str:
        return (f"VAR-{self.model} transformer part, {self.depth} blocks x {len(self.patch_nums)} steps ({self.max_len} tokens), "
                f"B={self.B} rows per token (CFG), {self.config.upper()} + FP6 KV cache, random weights"
                + (", full-width rotation" if self.rotation == "full" else "")
                + (f", attn_l2_norm (q / k norm: {self.qk_norm})" if self.attn_l2_norm else "")
                + (", KV cache stored as FP6 codes + scales (PackedKVCache)" if self.kv_storage == "codes" else ""))


def generation_record(models: Sequence[str] = ("d30-256", "d36-512"), paths: Sequence[str] = PATHS, config: str = "w4a4",
                      reps: int = 3, device=None, seed: int = 0, depth: Optional[int] = None, tuned_gemms: bool = True) -> List[dict]:
    """bench.py's `generation` entries (this rank's replica): one record per (model, path).  tuned_gemms: torch's own GEMMs
    - the same ones on every path - run with the recorded TunableOp selections (tuned_torch_gemms), and the record says so."""
    out = []
    for model in models:
        gb = GenerationBatch(model, config, depth=depth, device=device, seed=seed)
        for path in paths:
            rec = {"model": model, "path": path, "config": config, "images_per_batch": gb.B // 2, "what": WHAT[model]}
            if path == "Q":
                rec["operands"] = "k-major images (include/fpq.h)" if gb.kmajor else "row-major codes"
                rec["kv_cache"] = (f"k, v written into the cache's slots by mat_qkv's GEMM ({'fpq_gemm_fp6_rows_split' if gb.W6 else 'fpq_gemm_fp4_mx_split'}), one quantization pass per step"
                                   if gb.qkv_to_cache else "one launch per step: quantization pass + copy-in of k, v")
            try:
                if tuned_gemms:
                    with tuned_torch_gemms() as tg:
                        rec.update(gb.time_path(path, reps))
                    rec["torch_gemms"] = ("TunableOp selections recorded for these shapes (fpqvar_amd/tunableop_gfx950.csv), no tuning at run time"
                                          if tg.active else "torch's default selection (the recorded TunableOp file did not validate on this box)")
                else:
                    rec.update(gb.time_path(path, reps))
                    rec["torch_gemms"] = "torch's default selection"
            except Exception as e:   # one failing path must not hide the others
                rec["error"] = repr(e)[:200]
                torch.cuda.empty_cache()
            out.append(rec)
        del gb
        torch.cuda.empty_cache()
    return out
