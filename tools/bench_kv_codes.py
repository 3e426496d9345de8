#!/usr/bin/env python3
"""The packed KV cache against the fp16 one, kernel by kernel, at every scale step of both models (real B, H; one block's cache):
  attention  fpq_attention_blhc over the fp16 cache views   vs  fpq_attention_blhc_kvcodes over codes + the step's fresh rows
  cache      fpq_kv_cache_step (quantize the previous step's entries in place, n_new = 0: the split GEMM wrote k / v)
             vs  fpq_kv_pack (quantize the step's fresh rows into their code slots)
kv_bit 6 (the models' FP6 KV cache) and 4.  Each kernel: HIP events around `--iters` back-to-back launches on warmed buffers, best
of `--reps`; the two forms of a step run in the same process on the same inputs.  One JSON line per (model, kv_bit), then totals."""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

from fpqvar_amd import _lib, kv_cache, ops, var_block  # noqa: E402


def timed(fn, iters, reps):
    fn()
    best = float("inf")
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(iters):
            fn()
        b.record()
        b.synchronize()
        best = min(best, a.elapsed_time(b) / iters)
    return best * 1e3   # us


def one(model, kv_bit, iters, reps, dev):
    H, pns, B = var_block.MODELS[model]
    T = sum(p * p for p in pns)
    g = torch.Generator(device=dev).manual_seed(0)
    inc = kv_cache.IncrementalKVCache(B, T, H, 64, kv_bit, device=dev)
    pc = kv_cache.PackedKVCache(B, T, H, 64, kv_bit, dev)
    inc.kv.copy_(torch.randn(inc.kv.shape, device=dev, generator=g).half())
    ops.kv_pack(pc.codes, pc.scales, kv_bit, 0, inc.k, inc.v)   # every slot holds valid codes
    group, table = (64, "e2m3") if kv_bit == 6 else (128, "e2m1")
    rows, pos, prev = [], 0, 0
    for pn in pns:
        L = pn * pn
        qkv = torch.randn(B, L, 3, H, 64, device=dev, generator=g).half()
        q, k, v = qkv.unbind(2)
        K, V = inc.k[:, :pos + L], inc.v[:, :pos + L]
        empty = inc.kv[0, :, :0]
        t_attn = timed(lambda: ops.attention_blhc(q, K, V, 0.125), iters, reps)
        t_attn_c = timed(lambda: ops.attention_blhc_kvcodes(q, pc.codes, pc.scales, kv_bit, pos, k, v, 0.125), iters, reps)
        t_step = timed(lambda: ops.kv_cache_step(inc.kv, prev, pos, empty, empty, pos, group, table), iters, reps) if pos > prev else 0.0
        t_pack = timed(lambda: ops.kv_pack(pc.codes, pc.scales, kv_bit, pos, k, v), iters, reps)
        rows.append({"pn": pn, "L": L, "n_packed": pos, "attn_fp16_us": round(t_attn, 1), "attn_codes_us": round(t_attn_c, 1),
                     "kv_cache_step_us": round(t_step, 1), "kv_pack_us": round(t_pack, 1)})
        prev, pos = pos, pos + L
    tot = {k: round(sum(r[k] for r in rows), 1) for k in ("attn_fp16_us", "attn_codes_us", "kv_cache_step_us", "kv_pack_us")}
    return {"model": model, "kv_bit": kv_bit, "B": B, "H": H, "tokens": T, "steps": rows, "per_block_batch_us": tot,
            "fp16_cache_bytes": inc.kv.numel() * 2, "packed_cache_bytes": pc.nbytes}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--models", default="d30-256,d36-512")
    ap.add_argument("--kv-bits", default="6,4")
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    print(json.dumps({"library": _lib.build_tag(), "device": torch.cuda.get_device_name(0), "iters": args.iters, "reps": args.reps,
                      "clock": "HIP events around iters back-to-back launches, best of reps, us per launch"}))
    for m in args.models.split(","):
        for kb in (int(x) for x in args.kv_bits.split(",")):
            print(json.dumps(one(m, kb, args.iters, args.reps, dev)))
            torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
