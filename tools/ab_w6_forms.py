#!/usr/bin/env python3
"""The W6 GEMM's fc1 tail and split output (gemm.linear_w6_gelu_dual, gemm.linear_w6_qkv_to_cache) beside the launches they replace, at
the ten scale steps of d30 (rows = 100 pn^2), for one E2M1-activation pair and one 6-bit-activation pair; operands already quantized
(the producer in front is the same in every form), row-major, fp32 weight scales, a bias:

  fc1 [rows x 1920 -> 7680]
    (a)  linear_w6_gelu_dual                                                     one launch (+ the NaN fix-up launch)
    (b)  linear_w6 + F.gelu(approximate="tanh") + ops.quant_rows_dual             the three launches it replaces
    (c)  linear_w6 + ops.gelu_quant_rows_dual                                     the GeluThenFc2Quant route (quantize_VAR_mixed without w6_forms)
  mat_qkv [rows x 1920 -> 5760], 100 batch entries, q / k norm
    (a)  linear_w6_qkv_to_cache(qk_norm_scale=...)                                one launch
    (b)  linear_w6 + torch's F.normalize of q and k (fp32) + the copy of k, v into the cache     (tr/basic_var.py:173-209)

One process; every form works through a ring of operand sets larger than the 256 MiB of L2 + Infinity Cache (cold operands); a
form's sweep over its ring is captured once as a HIP graph and replayed; the forms alternate, best of 5 replays, HIP events around
each.
usage: ab_w6_forms.py [--rows 100,400,...]"""
import argparse
import hashlib
import os
import subprocess
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402
import torch.nn.functional as F  # noqa: E402

from fpqvar_amd import _lib, gemm, kv_cache, ops  # noqa: E402

dev = torch.device("cuda:0")
torch.manual_seed(0)
ROWS = tuple(100 * pn * pn for pn in (1, 2, 3, 4, 5, 6, 8, 10, 13, 16))   # tools/bench_small_steps.py, d30
BSZ, K, HEADS = 100, 1920, 30
PAIRS = (("e2m1", "e3m0"), ("e3m0", "e1m2"))
RING_BYTES = 640 << 20


def quantize(table, x):
    return gemm.quantize_mx(x) if table == "e2m1" else gemm.quantize_g6(x, table)


def ring_of(per_set):
    return max(2, min(32, RING_BYTES // per_set + 1))


def build_fc1(pair, tokens):
    at, wt = pair
    outs = 4 * K
    ring = ring_of(tokens * K + outs * K + tokens * outs * 2)             # codes of both operands (at most a byte per element), the output
    acts = [quantize(at, torch.randn(tokens, K, device=dev).half()) for _ in range(ring)]
    w6 = [gemm.quantize_g6(torch.randn(outs, K, device=dev) * 0.02, wt) for _ in range(ring)]
    bias = (torch.randn(outs, device=dev) * 0.1).half()
    calls = {
        "a": lambda i: gemm.linear_w6_gelu_dual(*acts[i], at, *w6[i], wt, bias),
        "b": lambda i: ops.quant_rows_dual(F.gelu(gemm.linear_w6(*acts[i], at, *w6[i], wt, bias), approximate="tanh"), "e1m2_neg", "e2m1_pos", 128, 1.0),
        "c": lambda i: ops.gelu_quant_rows_dual(gemm.linear_w6(*acts[i], at, *w6[i], wt, bias), "e1m2_neg", "e2m1_pos"),
    }
    return calls, ring


def build_qkv(pair, tokens):
    at, wt = pair
    outs, c, seq = 3 * K, K, tokens // BSZ
    ring = ring_of(tokens * K + outs * K + tokens * outs * 2)
    acts = [quantize(at, torch.randn(tokens, K, device=dev).half()) for _ in range(ring)]
    w6 = [gemm.quantize_g6(torch.randn(outs, K, device=dev) * 0.02, wt) for _ in range(ring)]
    caches = [torch.zeros(2, BSZ, seq, HEADS, 64, dtype=torch.float16, device=dev) for _ in range(ring)]
    hs = kv_cache.qk_norm_head_scale(torch.full((1, HEADS, 1, 1), 4.0, device=dev).log())
    b32 = torch.cat([torch.randn(c, device=dev) * 0.1, torch.zeros(c, device=dev), torch.randn(c, device=dev) * 0.1])

    def unfused(i):
        y = gemm.linear_w6(*acts[i], at, *w6[i], wt, None).float().add_(b32)
        q, k, v = y.view(BSZ, seq, 3, HEADS, 64).unbind(2)
        q = F.normalize(q, dim=-1).mul(hs.view(1, 1, HEADS, 1)).half()
        caches[i][0].copy_(F.normalize(k, dim=-1))
        caches[i][1].copy_(v)
        return q
    calls = {
        "a": lambda i: gemm.linear_w6_qkv_to_cache(*acts[i], at, *w6[i], wt, b32, caches[i], 0, seq, qk_norm_scale=hs),
        "b": unfused,
    }
    return calls, ring


def capture(calls, ring):
    graphs, keep = {}, []
    side = torch.cuda.Stream()
    for f, call in calls.items():
        with torch.cuda.stream(side):                                      # warm-up on the capture stream: code objects, allocations
            for i in range(ring):
                call(i)
        torch.cuda.synchronize()
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g, stream=side):
            keep.append([call(i) for i in range(ring)])
        graphs[f] = g
    return graphs, keep


def measure(graphs, ring, rounds=5):
    best = {f: 1e30 for f in graphs}
    for f in graphs:
        graphs[f].replay()
    torch.cuda.synchronize()
    for _ in range(rounds):
        for f in graphs:
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            graphs[f].replay()
            e1.record()
            torch.cuda.synchronize()
            best[f] = min(best[f], e0.elapsed_time(e1) / ring * 1e3)
    return best


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", default=",".join(str(r) for r in ROWS))
    rows = [int(r) for r in ap.parse_args().rows.split(",")]
    try:
        commit = subprocess.run(["git", "rev-parse", "--short", "HEAD"], capture_output=True, text=True, cwd=os.path.dirname(__file__)).stdout.strip()
    except OSError:
        commit = ""
    sha = hashlib.sha256(open(_lib.LIB_PATH, "rb").read()).hexdigest()[:16]
    print(f"# tools/ab_w6_forms.py: commit {commit or '(working tree)'}, libfpq_hip.so sha256 {sha}, build tag {_lib.build_tag()}, {torch.cuda.get_device_name(0)}")
    print("# us per call chain, best of 5 alternating graph replays, cold operands (ring > 256 MiB), row-major operands, activations already quantized")
    for what, build, forms in (("fc1", build_fc1, "abc"), ("mat_qkv", build_qkv, "ab")):
        outs = 4 * K if what == "fc1" else 3 * K
        print(f"# {what}: (a) fused" + ("  (b) GEMM + GELU + dual quantizer  (c) GEMM + one-pass GELU-quantizer" if what == "fc1" else
                                       "  (b) GEMM + normalize + copy into the cache"))
        print("#    rows     K  outs  act  x weight  ring   " + "  ".join(f"      ({f})" for f in forms) + "  " + "  ".join(f"  {f}/a" for f in forms[1:]))
        for tokens in rows:
            for pair in PAIRS:
                calls, ring = build(pair, tokens)
                graphs, keep = capture(calls, ring)
                r = measure(graphs, ring)
                print(f"{tokens:9d} {K:5d} {outs:5d}  {pair[0]} x {pair[1]}     {ring:2d}   " + "  ".join(f"{r[f]:9.1f}" for f in forms) + "  " +
                      "  ".join(f"{r[f] / r['a']:5.2f}" for f in forms[1:]), flush=True)
                del graphs, keep, calls
                torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
