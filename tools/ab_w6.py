#!/usr/bin/env python3
"""E1M2 / E3M0 weights on the matrix cores as 6-bit codes (gemm.linear_w6) for the six (activation, weight) format pairs, beside what
such a layer ran before and beside the E2M1-weight layer of the same activation format; producer + GEMM each, row-major operands,
fp32 weight scales, a bias:

  (a)  the activation's quantizer (quantize_mx / quantize_g6) + linear_w6          the W6 path
  (b)  ops.quant_rows(x, a_table, 128) + torch's fp16 F.linear on the de-quantized weight   what the layer is as a QuantizedLinear
  (c)  the same quantizer + linear_fp4 (E2M1 activation) / linear_a6w4 (E1M2, E3M0) on an E2M1 weight: only the weight bytes differ,
       64 against 96 per row and group

mat_qkv of d30 [K = 1920 -> 5760] at 25 600 and at 100 rows.  One process; every form works through a ring of operand sets larger
than the 256 MiB of L2 + Infinity Cache (cold operands); a form's sweep over its ring is captured once as a HIP graph and replayed;
the forms alternate, best of 5 replays, HIP events around each.
usage: ab_w6.py"""
import hashlib
import os
import subprocess
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

from fpqvar_amd import _lib, gemm, ops  # noqa: E402

dev = torch.device("cuda:0")
torch.manual_seed(0)
SHAPES = ((25600, 1920, 5760), (100, 1920, 5760))
PAIRS = tuple((a, w) for a in ("e2m1", "e1m2", "e3m0") for w in ("e1m2", "e3m0"))
RING_BYTES = 640 << 20
FORMS = ("a", "b", "c")


def quantize(table, x):
    return gemm.quantize_mx(x) if table == "e2m1" else gemm.quantize_g6(x, table)


def build(pair, tokens, k, outs):
    """{form: graph replaying one call per ring entry}, ring length"""
    at, wt = pair
    per_set = tokens * k * 2 + outs * k * 2 + tokens * outs * 2           # the largest form's cold bytes per call: x, the fp16 weight, the output
    ring = max(2, min(32, RING_BYTES // per_set + 1))
    xs = [torch.randn(tokens, k, device=dev).half() for _ in range(ring)]
    ws = [torch.randn(outs, k, device=dev) * 0.02 for _ in range(ring)]
    bias = (torch.randn(outs, device=dev) * 0.1).half()
    w6 = [gemm.quantize_g6(w, wt) for w in ws]
    w4 = [gemm.quantize_mx(w) for w in ws]
    w16 = [ops.quant_rows(w, wt, 128).half() for w in ws]
    del ws
    calls = {
        "a": lambda i: gemm.linear_w6(*quantize(at, xs[i]), at, *w6[i], wt, bias),
        "b": lambda i: torch.nn.functional.linear(ops.quant_rows(xs[i], at, 128), w16[i], bias),
        "c": (lambda i: gemm.linear_fp4(*gemm.quantize_mx(xs[i]), *w4[i], bias)) if at == "e2m1" else
             (lambda i: gemm.linear_a6w4(*gemm.quantize_g6(xs[i], at), at, *w4[i], bias)),
    }
    graphs, keep = {}, []
    side = torch.cuda.Stream()
    for f in FORMS:
        with torch.cuda.stream(side):                                      # warm-up on the capture stream: code objects, GEMM algorithm choice
            for i in range(ring):
                calls[f](i)
        torch.cuda.synchronize()
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g, stream=side):
            keep.append([calls[f](i) for i in range(ring)])
        graphs[f] = g
    return graphs, ring, keep


def measure(graphs, ring, rounds=5):
    best = {f: 1e30 for f in FORMS}
    for f in FORMS:
        graphs[f].replay()
    torch.cuda.synchronize()
    for _ in range(rounds):
        for f in FORMS:
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            graphs[f].replay()
            e1.record()
            torch.cuda.synchronize()
            best[f] = min(best[f], e0.elapsed_time(e1) / ring * 1e3)
    return best


def main():
    try:
        commit = subprocess.run(["git", "rev-parse", "--short", "HEAD"], capture_output=True, text=True, cwd=os.path.dirname(__file__)).stdout.strip()
    except OSError:
        commit = ""
    sha = hashlib.sha256(open(_lib.LIB_PATH, "rb").read()).hexdigest()[:16]
    print(f"# tools/ab_w6.py: commit {commit or '(working tree)'}, libfpq_hip.so sha256 {sha}, build tag {_lib.build_tag()}, {torch.cuda.get_device_name(0)}")
    print("# us per producer + GEMM, best of 5 alternating graph replays, cold operands (ring > 256 MiB), row-major operands")
    print("#  tokens     K  outs  act  x weight  ring          (a)        (b)        (c)      b/a    a/c")
    for tokens, k, outs in SHAPES:
        for pair in PAIRS:
            graphs, ring, keep = build(pair, tokens, k, outs)
            r = measure(graphs, ring)
            print(f"{tokens:7d} {k:5d} {outs:5d}  {pair[0]} x {pair[1]}     {ring:2d}   " + "  ".join(f"{r[f]:9.1f}" for f in FORMS) +
                  f"    {r['b'] / r['a']:5.2f}  {r['a'] / r['c']:5.2f}", flush=True)
            del graphs, keep
            torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
