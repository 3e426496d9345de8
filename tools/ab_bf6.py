#!/usr/bin/env python3
"""BF6 (E3M2) operands on the FP6 matrix-core path against E2M3 and against the FP8 path E3M2 layers took before, k-major operands,
at the row counts of a VAR-d30 generation batch (B = 100 rows per token, C = 1920) and at [65536 x 1920 -> 5760], for the mat_qkv /
fc1 / proj widths.  One process; every variant works through a ring of operand sets larger than the 256 MiB of L2 + Infinity Cache
(cold operands), HIP events around bursts, the variants alternating, best of 5 bursts.

  (a)  E2M3 x E2M3, gemm.linear_fp6 as it always ran - measured twice, (a1) and (a2): the A/A spread of this tool
  (b)  E3M2 activations x E2M3 weights      (c)  E3M2 x E3M2
  (d)  what an E3M2 layer ran before: quantize_fp8(x, "e3m2") + linear_fp8 (row-major E4M3 bytes)
GEMM alone, and producer + GEMM (producer: the per-token quantizer of an fp16 [tokens, C] activation, k-major for a - c).
usage: ab_bf6.py [--quick]"""
import os
import subprocess
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

from fpqvar_amd import _lib, gemm  # noqa: E402

QUICK = "--quick" in sys.argv
dev = torch.device("cuda:0")
torch.manual_seed(0)
B, C = 100, 1920
PN = (1, 2, 3, 4, 5, 6, 8, 10, 13, 16)
WIDTHS = (("qkv", 3 * C), ("fc1", 4 * C), ("proj", C))
RING_BYTES = 640 << 20
VARIANTS = ("a1", "a2", "b", "c", "d")
TABLES = {"a1": ("e2m3", "e2m3"), "a2": ("e2m3", "e2m3"), "b": ("e3m2", "e2m3"), "c": ("e3m2", "e3m2"), "d": ("e3m2", "e2m3")}


def burst(fn, n):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for i in range(n):
        fn(i)
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / n * 1e3


def alternate(fns, n):
    """{name: best us per call} - every variant warmed, then 5 rounds of one burst each, in turn"""
    best = {k: 1e30 for k in fns}
    for k, f in fns.items():
        f(0)
    for _ in range(5):
        for k, f in fns.items():
            best[k] = min(best[k], burst(f, n))
    return best


def build(tokens, outs):
    """per variant: a ring of (activation, activation operand, weight operand) sets -> (gemm_only(i), producer_and_gemm(i))"""
    fns_g, fns_pg = {}, {}
    for v in VARIANTS:
        ta, tw = TABLES[v]
        row_bytes = C if v == "d" else C * 3 // 4
        ring = max(2, min(64, RING_BYTES // ((tokens + outs) * row_bytes + tokens * C * 2) + 1))
        sets = []
        for _ in range(ring):
            x = torch.randn(tokens, C, device=dev).half()
            wt = torch.randn(outs, C, device=dev) * 0.02
            if v == "d":
                sets.append((x, gemm.quantize_fp8(x, ta), gemm.quantize_fp8(wt, tw)))
            else:
                wc, ws = gemm.quantize_fp6(wt, table=tw)
                sets.append((x, gemm.quantize_fp6(x, kmajor=True, table=ta), (gemm.to_kmajor(wc, 6, dealt=True), ws)))
        if v == "d":
            fns_g[v] = lambda i, s=sets: gemm.linear_fp8(*s[i % len(s)][1], *s[i % len(s)][2])
            fns_pg[v] = lambda i, s=sets, ta=ta: gemm.linear_fp8(*gemm.quantize_fp8(s[i % len(s)][0], ta), *s[i % len(s)][2])
        else:
            fns_g[v] = lambda i, s=sets, ta=ta, tw=tw: gemm.linear_fp6(*s[i % len(s)][1], *s[i % len(s)][2], a_table=ta, w_table=tw)
            fns_pg[v] = lambda i, s=sets, ta=ta, tw=tw: gemm.linear_fp6(*gemm.quantize_fp6(s[i % len(s)][0], kmajor=True, table=ta),
                                                                      *s[i % len(s)][2], a_table=ta, w_table=tw)
    return fns_g, fns_pg


def line(tokens, name, outs, n):
    fns_g, fns_pg = build(tokens, outs)
    g, pg = alternate(fns_g, n), alternate(fns_pg, n)
    fmt = lambda r: "  ".join(f"{r[v]:8.1f}" for v in VARIANTS) + f"   {r['b'] / r['a1']:5.3f} {r['c'] / r['a1']:5.3f} {r['d'] / r['b']:5.3f}  {abs(r['a2'] / r['a1'] - 1) * 100:4.1f}%"
    print(f"{tokens:7d} {name:5s} {outs:5d}  GEMM      {fmt(g)}")
    print(f"{tokens:7d} {name:5s} {outs:5d}  prod+GEMM {fmt(pg)}", flush=True)
    return g, pg


def main():
    try:
        commit = subprocess.run(["git", "rev-parse", "--short", "HEAD"], capture_output=True, text=True, cwd=os.path.dirname(__file__)).stdout.strip()
    except OSError:
        commit = ""
    import hashlib
    sha = hashlib.sha256(open(_lib.LIB_PATH, "rb").read()).hexdigest()[:16]
    print(f"# tools/ab_bf6.py{' --quick' if QUICK else ''}: commit {commit or '(working tree)'}, libfpq_hip.so sha256 {sha}, build tag {_lib.build_tag()}, "
          f"{torch.cuda.get_device_name(0)}")
    print("# us per call, best of 5 alternating bursts, cold operands (ring > 256 MiB); k-major operands for a - c")
    print("#  tokens layer  outs  what         (a1)      (a2)       (b)       (c)       (d)     b/a1  c/a1   d/b   A/A")
    tot = {w: {v: 0.0 for v in VARIANTS} for w in ("GEMM", "prod+GEMM")}
    steps = PN[-3:] if QUICK else PN
    for pn in steps:
        tokens = B * pn * pn
        for name, outs in WIDTHS:
            g, pg = line(tokens, name, outs, 20 if tokens <= 10000 else 10)
            for v in VARIANTS:
                tot["GEMM"][v] += g[v]
                tot["prod+GEMM"][v] += pg[v]
    for w in tot:
        r = tot[w]
        print(f"# sum over the d30 steps, three layers, {w:9s}: " + "  ".join(f"({v}) {r[v]:9.1f}" for v in VARIANTS) +
              f"   b/a1 {r['b'] / r['a1']:.3f}  c/a1 {r['c'] / r['a1']:.3f}  d/b {r['d'] / r['b']:.3f}  A/A {abs(r['a2'] / r['a1'] - 1) * 100:.1f}%")
    print("# the large problem")
    line(65536, "qkv", 3 * C, 10)


if __name__ == "__main__":
    main()
