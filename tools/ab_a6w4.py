#!/usr/bin/env python3
"""E3M0 / E1M2 activations on the matrix cores against FP4 weights (gemm.quantize_g6 + gemm.linear_a6w4) beside what such a layer ran
before and beside the all-E2M1 layer, producer + GEMM each, row-major operands, fp32 weight scales, a bias:

  (a)  quantize_g6(x, table) + linear_a6w4                                  the A6W4 path
  (b)  ops.quant_rows(x, table, 128) + torch's fp16 F.linear on the fake-quantized weight   what the mixed W4A4 model runs for the layer today
  (c)  quantize_mx(x) + linear_fp4                                          the E2M1 layer on the same shape: (a)'s ceiling - only the activation
                                                                            bytes grow, 96 against 64 per row and group
d30 (K = 1920 -> 5760, 7680) and d36 (K = 2304 -> 6912, 9216) at the ten scale-step row counts of a B = 100 batch and at 65 536 rows.
One process; every form works through a ring of operand sets larger than the 256 MiB of L2 + Infinity Cache (cold operands); a form's
sweep over its ring is captured once as a HIP graph and replayed; the forms alternate, best of 5 replays, HIP events around each.
Then the emitter alone beside the FP4 emitter (rows16_codes_mx_kernel) at [65536 x 1920] fp16: time and share of 8 TB/s.
usage: ab_a6w4.py [--quick] [--table e3m0|e1m2]"""
import hashlib
import os
import subprocess
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

from fpqvar_amd import _lib, gemm, ops  # noqa: E402

QUICK = "--quick" in sys.argv
TABLE = sys.argv[sys.argv.index("--table") + 1] if "--table" in sys.argv else "e3m0"
dev = torch.device("cuda:0")
torch.manual_seed(0)
B = 100
PN = (1, 2, 3, 4, 5, 6, 8, 10, 13, 16)
LAYERS = (("d30 qkv", 1920, 5760), ("d30 fc1", 1920, 7680), ("d36 qkv", 2304, 6912), ("d36 fc1", 2304, 9216))
RING_BYTES = 640 << 20
FORMS = ("a", "b", "c")
HBM_BYTES_PER_S = 8.0e12


def build(tokens, k, outs):
    """{form: graph replaying one call per ring entry}, ring length"""
    per_set = tokens * k * 2 + outs * k * 2 + tokens * outs * 2           # the largest form's cold bytes per call: x, the fp16 weight, the output
    ring = max(2, min(32, RING_BYTES // per_set + 1))
    xs = [torch.randn(tokens, k, device=dev).half() for _ in range(ring)]
    ws = [torch.randn(outs, k, device=dev) * 0.02 for _ in range(ring)]
    bias = (torch.randn(outs, device=dev) * 0.1).half()
    w4 = [gemm.quantize_mx(w) for w in ws]
    w16 = [ops.quant_rows(w, "e2m1", 128).half() for w in ws]
    del ws
    calls = {
        "a": lambda i: gemm.linear_a6w4(*gemm.quantize_g6(xs[i], TABLE), TABLE, *w4[i], bias),
        "b": lambda i: torch.nn.functional.linear(ops.quant_rows(xs[i], TABLE, 128), w16[i], bias),
        "c": lambda i: gemm.linear_fp4(*gemm.quantize_mx(xs[i]), *w4[i], bias),
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


def line(tokens, name, k, outs):
    graphs, ring, keep = build(tokens, k, outs)
    r = measure(graphs, ring)
    print(f"{tokens:7d} {name:8s} {k:5d} {outs:5d}  ring {ring:2d}   " + "  ".join(f"{r[f]:9.1f}" for f in FORMS) +
          f"    {r['b'] / r['a']:5.2f}  {r['a'] / r['c']:5.2f}", flush=True)
    del graphs, keep
    torch.cuda.empty_cache()
    return r


def emitters():
    rows, k = 65536, 1920
    xs = [torch.randn(rows, k, device=dev).half() for _ in range(4)]     # 4 x 252 MB: cold
    forms = {"quantize_g6 (group6_emit16_kernel)": (lambda x: gemm.quantize_g6(x, TABLE), 2 + 0.75 + 2 / 128),
             "quantize_mx (rows16_codes_mx_kernel)": (lambda x: gemm.quantize_mx(x), 2 + 0.5 + 2 / 128)}
    best = {n: 1e30 for n in forms}
    for n, (fn, _) in forms.items():
        for x in xs:
            fn(x)
    torch.cuda.synchronize()
    for _ in range(5):
        for n, (fn, _) in forms.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for x in xs:
                fn(x)
            e1.record()
            torch.cuda.synchronize()
            best[n] = min(best[n], e0.elapsed_time(e1) / len(xs) * 1e3)
    print(f"# the emitters alone, fp16 [{rows} x {k}], cold input, eager launches (output allocation included), best of 5:")
    for n, (_, bpe) in forms.items():
        byts = rows * k * bpe
        print(f"#   {n:40s} {best[n]:8.1f} us   {byts / 1e6:7.1f} MB moved   {byts / (best[n] * 1e-6) / HBM_BYTES_PER_S * 100:5.1f} % of 8 TB/s")


def main():
    try:
        commit = subprocess.run(["git", "rev-parse", "--short", "HEAD"], capture_output=True, text=True, cwd=os.path.dirname(__file__)).stdout.strip()
    except OSError:
        commit = ""
    sha = hashlib.sha256(open(_lib.LIB_PATH, "rb").read()).hexdigest()[:16]
    print(f"# tools/ab_a6w4.py{' --quick' if QUICK else ''} --table {TABLE}: commit {commit or '(working tree)'}, libfpq_hip.so sha256 {sha}, "
          f"build tag {_lib.build_tag()}, {torch.cuda.get_device_name(0)}")
    print("# us per producer + GEMM, best of 5 alternating graph replays, cold operands (ring > 256 MiB), row-major operands")
    print("#  tokens layer        K  outs  ring          (a)        (b)        (c)      b/a    a/c")
    tot = {f: 0.0 for f in FORMS}
    steps = PN[-3:] if QUICK else PN
    layers = LAYERS[:2] if QUICK else LAYERS
    for name, k, outs in layers:
        for pn in steps:
            r = line(B * pn * pn, name, k, outs)
            if name.startswith("d30"):
                for f in FORMS:
                    tot[f] += r[f]
        line(65536, name, k, outs)
    print("# sum over the d30 steps (qkv + fc1): " + "  ".join(f"({f}) {tot[f]:9.1f}" for f in FORMS) +
          f"   b/a {tot['b'] / tot['a']:.3f}  a/c {tot['a'] / tot['c']:.3f}")
    emitters()


if __name__ == "__main__":
    main()
