#!/usr/bin/env python3
"""Two measurements behind INTEGRATION.md's attn_l2_norm row (one GPU):

  dtypes     the reference's lines (tr/basic_var.py:173-183) under torch.autocast("cuda", float16) on random tensors: the
             dtypes of qkv, q, k, v - the fp32 flow the contract of fpq_gemm_fp4_mx_split_qknorm / fpq_kv_cache_step_qknorm rests on;
  deviation  the reference keeps that fp32 k / v in its cache and quantizes them in fp32; this project's cache is fp16.  At d30
             shapes (100 rows, 30 heads, the ten steps' token counts) the fraction of cached K / V elements whose quantized value
             differs: the reference's fp32 result rounded to fp16 against the fp16 cache's result, and exact in fp32.

    python tools/qk_norm_checks.py [--out FILE]
"""
import argparse
import json
import math
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch
import torch.nn.functional as F


def dtype_flow(dev):
    torch.manual_seed(0)
    B, L, H, C = 2, 16, 30, 1920
    mat_qkv = torch.nn.Linear(C, 3 * C, bias=False).to(dev)
    q_bias, v_bias, zero_k_bias = torch.randn(C, device=dev) * 0.1, torch.randn(C, device=dev) * 0.1, torch.zeros(C, device=dev)
    scale_mul_1H11 = torch.full((1, H, 1, 1), 4.0, device=dev).log()
    x = torch.randn(B, L, C, device=dev)
    with torch.autocast("cuda", dtype=torch.float16):
        qkv = mat_qkv(x) + torch.cat((q_bias, zero_k_bias, v_bias))
        q, k, v = qkv.view(B, L, 3, H, 64).unbind(dim=2)
        scale_mul = scale_mul_1H11.clamp_max(math.log(100)).exp().transpose(1, 2)
        q = F.normalize(q, dim=-1).mul(scale_mul)
        k = F.normalize(k, dim=-1)
        lin = mat_qkv(x)
    return {"linear_out": str(lin.dtype), "qkv": str(qkv.dtype), "q": str(q.dtype), "k": str(k.dtype), "v": str(v.dtype)}


def deviation(dev):
    from fpqvar_amd import kv_cache, var_block
    from fpqvar_amd import quant_utils as qu
    e2m3 = qu.fp6_e2m3_grid.to(dev)
    g = torch.Generator(device=dev).manual_seed(1)
    B, H = 100, 30
    C = 64 * H
    out = {}
    tot = {"k": [0, 0, 0, 0], "v": [0, 0, 0, 0]}

    def ordered(h):   # fp16 -> integers in value order: differences in ulps
        i = h.contiguous().view(torch.int16).int()
        return torch.where(i < 0, -(i & 0x7FFF), i)
    for pn in (1, 2, 3, 4, 5, 6, 8, 10, 13, 16):
        L = pn * pn
        y16 = (torch.randn(B, L, 3 * C, device=dev, generator=g) * 0.5).half()            # the fp16 Linear output
        bias = torch.cat((torch.randn(C, device=dev, generator=g) * 0.1, torch.zeros(C, device=dev), torch.randn(C, device=dev, generator=g) * 0.1))
        y = y16.float() + bias
        _, k32, v32 = y.view(B, L, 3, H, 64).unbind(2)
        k32 = F.normalize(k32, dim=-1)
        for name, t32 in (("k", k32), ("v", v32)):
            ref = var_block._ref_sym(t32.contiguous(), e2m3, None, None)                      # fp32 cache, fp32 quantization
            ours = kv_cache.quantize_kv(t32.half().contiguous(), 6)                           # fp16 cache
            tot[name][0] += ref.numel()
            tot[name][1] += int((ref.half() != ours).sum())
            tot[name][2] += int((ref != ours.float()).sum())
            tot[name][3] += int(((ordered(ref.half()) - ordered(ours)).abs() > 1).sum())
    for name, (n, d16, d32, d2) in tot.items():
        out[name] = {"elements": n, "differ_after_fp16_rounding": d16, "fraction_fp16": d16 / n,
                     "differ_by_more_than_1_ulp": d2, "fraction_more_than_1_ulp": d2 / n,
                     "differ_in_fp32": d32, "fraction_fp32": d32 / n}
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    res = {"dtype_flow_under_autocast_fp16": dtype_flow(dev), "fp32_cache_deviation_d30_kv6": deviation(dev),
           "device": torch.cuda.get_device_name(0)}
    txt = json.dumps(res, indent=1)
    print(txt)
    if args.out:
        with open(args.out, "w") as f:
            f.write(txt + "\n")


if __name__ == "__main__":
    main()
