#!/usr/bin/env python3
"""A layer of a mixed-format W4A4 block with a 6-bit activation on the A6W4 GEMM, row-major operands against k-major images,
producer included, fp32 weight scales, a bias:

  (r)   quantize_g6(x, table)              + linear_a6w4 / linear_a6w4_gelu_dual             row-major codes and scales
  (r')  the same again                                                                       the tool's own A/A spread
  (k)   quantize_g6(x, table, kmajor=True) + linear_a6w4_km / linear_a6w4_gelu_dual_km        k-major images (the weight's made once)
  (k')  the same again
  (er) (er') (ek) (ek')  the two emitters alone

Two layers per model: "qkv", the plain form (d30: K = 1920 -> 5760, B = 100; d36-512: K = 2304 -> 6912, B = 20), and "fc1", the
form with the fc1 tail (-> 7680 / 9216), at the ten scale-step row counts and at 65 536 rows.
One process; every form works through a ring of operand sets larger than the 256 MiB of L2 + Infinity Cache (cold operands); a
form's sweep over its ring is captured once as a HIP graph and replayed; the forms alternate, best of 5 replays, HIP events
around each.  Per model and layer: the sums over the ten steps, the A/A spread (the larger of |r - r'| and |k - k'| of the sums)
and the verdict - a layout is ahead only if the sums differ by more than that spread.  The outputs of (r) and (k) are compared bit
for bit on every ring entry before anything is timed.
usage: ab_a6w4_km.py [--quick] [--table e3m0|e1m2]"""
import hashlib
import json
import os
import subprocess
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

from fpqvar_amd import _lib, gemm  # noqa: E402

QUICK = "--quick" in sys.argv
TABLE = sys.argv[sys.argv.index("--table") + 1] if "--table" in sys.argv else "e3m0"
dev = torch.device("cuda:0")
torch.manual_seed(0)
MODELS = (("d30", 1920, 100, (1, 2, 3, 4, 5, 6, 8, 10, 13, 16)), ("d36", 2304, 20, (1, 2, 3, 4, 6, 9, 13, 18, 24, 32)))
LAYERS = (("qkv", 3, False), ("fc1", 4, True))     # name, outs / K, the fc1 tail
RING_BYTES = 640 << 20
GEMMS = ("r", "r'", "k", "k'")
EMITTERS = ("er", "er'", "ek", "ek'")
FORMS = GEMMS + EMITTERS


def build(tokens, k, outs, fc1):
    """{form: graph replaying one call per ring entry}, ring length"""
    per_set = tokens * k * 2 + outs * k // 2 + tokens * outs * 2          # cold bytes per call: x, the weight codes, the output
    ring = max(2, min(32, RING_BYTES // per_set + 1))
    xs = [torch.randn(tokens, k, device=dev).half() for _ in range(ring)]
    w4 = [gemm.quantize_mx(torch.randn(outs, k, device=dev) * 0.02) for _ in range(ring)]
    wk = [(gemm.to_kmajor(c, 4, dealt=True), gemm.to_kmajor_scales(s, weight_side=True)) for c, s in w4]
    bias = (torch.randn(outs, device=dev) * 0.1).half()
    lin_r, lin_k = (gemm.linear_a6w4_gelu_dual, gemm.linear_a6w4_gelu_dual_km) if fc1 else (gemm.linear_a6w4, gemm.linear_a6w4_km)
    row = lambda i: lin_r(*gemm.quantize_g6(xs[i], TABLE), TABLE, *w4[i], bias)
    km = lambda i: lin_k(*gemm.quantize_g6(xs[i], TABLE, kmajor=True), TABLE, *wk[i], bias)
    emit_r = lambda i: gemm.quantize_g6(xs[i], TABLE)
    emit_k = lambda i: gemm.quantize_g6(xs[i], TABLE, kmajor=True)
    calls = {"r": row, "r'": row, "k": km, "k'": km, "er": emit_r, "er'": emit_r, "ek": emit_k, "ek'": emit_k}
    for i in range(ring):                                                  # faster and different is not faster
        a, b = row(i), km(i)
        if not torch.equal(a.view(torch.int16), b.view(torch.int16)):
            raise SystemExit(f"[{tokens} x {k} -> {outs}] fc1={fc1}: the k-major result differs from the row-major one")
    graphs, keep = {}, []
    side = torch.cuda.Stream()
    for f in FORMS:
        with torch.cuda.stream(side):                                      # warm-up on the capture stream
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


def line(tokens, name, layer, k, outs, fc1):
    graphs, ring, keep = build(tokens, k, outs, fc1)
    r = measure(graphs, ring)
    aa = max(abs(r["r"] - r["r'"]) / r["r"], abs(r["k"] - r["k'"]) / r["k"]) * 100
    print(f"{tokens:7d} {name:4s} {layer:4s} {k:5d} {outs:5d}  ring {ring:2d}   " + "  ".join(f"{r[f]:9.1f}" for f in FORMS) +
          f"    {r['r'] / r['k']:5.2f}  {r['er'] / r['ek']:5.2f}   {aa:4.1f} %", flush=True)
    del graphs, keep
    torch.cuda.empty_cache()
    return r


def verdict(tot, a, b):
    """sums of forms a, a', b, b' -> (spread, 'k-major ahead' / 'row-major ahead' / 'inside the spread')"""
    spread = max(abs(tot[a] - tot[a + "'"]), abs(tot[b] - tot[b + "'"]))
    ra, kb = min(tot[a], tot[a + "'"]), min(tot[b], tot[b + "'"])
    return spread, ("k-major ahead" if ra - kb > spread else "row-major ahead" if kb - ra > spread else "inside the spread")


def main():
    try:
        commit = subprocess.run(["git", "rev-parse", "--short", "HEAD"], capture_output=True, text=True, cwd=os.path.dirname(__file__)).stdout.strip()
    except OSError:
        commit = ""
    sha = hashlib.sha256(open(_lib.LIB_PATH, "rb").read()).hexdigest()[:16]
    print(f"# tools/ab_a6w4_km.py{' --quick' if QUICK else ''} --table {TABLE}: commit {commit or '(working tree)'}, libfpq_hip.so sha256 {sha}, "
          f"build tag {_lib.build_tag()}, {torch.cuda.get_device_name(0)}")
    print("# us per producer + GEMM (and per producer alone), best of 5 alternating graph replays, cold operands (ring > 256 MiB); (r) == (k) bit for bit")
    print("#  tokens model layer   K  outs  ring          (r)       (r')        (k)       (k')       (er)      (er')       (ek)      (ek')      r/k  er/ek    A/A")
    verdicts = {}
    for name, k, batch, pns in MODELS:
        for layer, mult, fc1 in LAYERS:
            tot = {f: 0.0 for f in FORMS}
            for pn in (pns[-3:] if QUICK else pns):
                r = line(batch * pn * pn, name, layer, k, mult * k, fc1)
                for f in FORMS:
                    tot[f] += r[f]
            big = line(65536, name, layer, k, mult * k, fc1)
            spread, who = verdict(tot, "r", "k")
            e_spread, e_who = verdict(tot, "er", "ek")
            print(f"# {name} {layer}: sum over the steps  " + "  ".join(f"({f}) {tot[f]:9.1f}" for f in GEMMS) +
                  f"   A/A spread {spread:.1f} us ({spread / tot['r'] * 100:.2f} %)   row-major / k-major {tot['r'] / tot['k']:.3f}   {who}")
            print(f"# {name} {layer}: the emitter alone   " + "  ".join(f"({f}) {tot[f]:9.1f}" for f in EMITTERS) +
                  f"   A/A spread {e_spread:.1f} us   row-major / k-major {tot['er'] / tot['ek']:.3f}   {e_who}")
            verdicts[f"{name} {layer}"] = {"sum_us": {f: round(tot[f], 1) for f in FORMS}, "aa_spread_us": round(spread, 1), "verdict": who,
                                           "emitter_aa_spread_us": round(e_spread, 1), "emitter_verdict": e_who,
                                           "at_65536_us": {f: round(big[f], 1) for f in FORMS}}
    print(json.dumps({"table": TABLE, "quick": QUICK, "layers": verdicts}))


if __name__ == "__main__":
    main()
