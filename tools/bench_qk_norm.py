#!/usr/bin/env python3
"""Cost of the attn_l2_norm q / k norm in the qkv-to-cache kernels at the largest step of a model (--model d30-256: 100 rows x 256
tokens = 25 600 tokens, C = 1920, 30 heads; d36-512: 20 rows x 1024 tokens = 20 480 tokens, C = 2304, 36 heads): the split FP4 GEMM
(k-major operands) with and without the norm epilogue, the FP6 GEMM of the W6A6 configuration as one [tokens, 3C] tensor, split,
and split with the norm, and the KV-cache step (previous step's entries quantized, the new rows copied in) with and without the
norm (+ q_out).  HIP events around `reps` back-to-back launches, median of `trials`, interleaved A/B.

    python tools/bench_qk_norm.py [--model d30-256] [--reps 50] [--trials 7]
"""
import argparse
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

from fpqvar_amd import gemm, kv_cache, ops, var_block  # noqa: E402


def timer(fn, reps):
    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    s.record()
    for _ in range(reps):
        fn()
    e.record()
    e.synchronize()
    return s.elapsed_time(e) / reps * 1e3   # us per call


def ab(fns, reps, trials):
    for f in fns.values():
        f()
    torch.cuda.synchronize()
    t = {k: [] for k in fns}
    for _ in range(trials):
        for k, f in fns.items():
            t[k].append(timer(f, reps))
    return {k: round(statistics.median(v), 2) for k, v in t.items()}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--model", default="d30-256", choices=tuple(var_block.MODELS))
    ap.add_argument("--reps", type=int, default=50)
    ap.add_argument("--trials", type=int, default=7)
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    torch.manual_seed(0)
    H, patch_nums, B = var_block.MODELS[args.model]
    L, prev = patch_nums[-1] ** 2, patch_nums[-2] ** 2
    C = 64 * H
    max_len = sum(p * p for p in patch_nums)
    x = torch.randn(B * L, C, device=dev).half()
    w = torch.randn(3 * C, C, device=dev) * 0.02
    a = gemm.quantize_mx(x, kmajor=True)
    wc, ws = gemm.quantize_mx(w)
    wk = (gemm.to_kmajor(wc, 4, dealt=True), gemm.to_kmajor_scales(ws, weight_side=True))
    bias = torch.randn(3 * C, device=dev) * 0.1
    hs = kv_cache.qk_norm_head_scale(torch.full((1, H, 1, 1), 4.0, device=dev).log())
    cache = torch.zeros(2, B, max_len, H, 64, dtype=torch.float16, device=dev)
    pos = max_len - L - 13
    res = {"shape": f"split GEMM {B * L} x {3 * C} x {C} (FP4 per-group: split_gemm_us, FP6 per-token: fp6_gemm_us); KV step B={B}, {prev} entries quantized, {L} new tokens, {H} heads",
           "clock": f"HIP events around {args.reps} launches, median of {args.trials} interleaved trials, us per launch",
           "device": torch.cuda.get_device_name(0)}
    res["split_gemm_us"] = ab({
        "plain": lambda: gemm.linear_fp4_qkv_to_cache(*a, *wk, None, cache, pos, L),
        "qk_norm": lambda: gemm.linear_fp4_qkv_to_cache(*a, *wk, bias, cache, pos, L, qk_norm_scale=hs),
    }, args.reps, args.trials)
    a6 = gemm.quantize_fp6(x, kmajor=True)
    wc6, ws6 = gemm.quantize_fp6(w)
    wk6 = (gemm.to_kmajor(wc6, 6, dealt=True), ws6)
    res["fp6_gemm_us"] = ab({
        "one_tensor": lambda: gemm.linear_fp6(*a6, *wk6),
        "plain": lambda: gemm.linear_fp6_qkv_to_cache(*a6, *wk6, None, cache, pos, L),
        "qk_norm": lambda: gemm.linear_fp6_qkv_to_cache(*a6, *wk6, bias, cache, pos, L, qk_norm_scale=hs),
    }, args.reps, args.trials)
    qkv = torch.randn(B, L, 3, H, 64, device=dev).half()
    q, k, v = qkv.unbind(2)
    res["kv_step_us"] = ab({
        "plain": lambda: ops.kv_cache_step(cache, pos - prev, pos, k, v, pos, 64, "e2m3"),
        "qk_norm": lambda: ops.kv_cache_step_qk_norm(cache, pos - prev, pos, q, k, v, pos, 64, "e2m3", hs, bias),
    }, args.reps, args.trials)
    for key in ("split_gemm_us", "fp6_gemm_us", "kv_step_us"):
        r = res[key]
        r["extra_pct"] = round(100.0 * (r["qk_norm"] / r["plain"] - 1), 2)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
