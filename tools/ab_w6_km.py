#!/usr/bin/env python3
"""A layer of a format-search model with a 6-bit WEIGHT on the W6 GEMM, row-major operands against k-major images, the activation
quantizer included, fp32 weight scales, a bias:

  (r)   quantize_mx / quantize_g6(x)              + the row-major form        row-major codes and scales
  (r')  the same again                                                        the tool's own A/A spread
  (k)   quantize_mx / quantize_g6(x, kmajor=True) + the form's _km twin       k-major images (the weight's made once)
  (k')  the same again

Three layers of d30 (K = 1920, B = 100) at its ten scale-step row counts: "qkv" -> 5760, the split output with the q / k norm into
a KV cache (linear_w6_qkv_to_cache / _km); "fc1" -> 7680, the form with the fc1 tail (linear_w6_gelu_dual / _km); "proj" -> 1920,
the plain form (linear_w6 / _km).  One (activation, weight) pair per activation format.
One process, one library; every form works through a ring of operand sets larger than the 256 MiB of L2 + Infinity Cache (cold
operands; the weights of a layer are made once and shared by its steps); a form's sweep over its ring is captured once as a HIP
graph and replayed; the forms alternate, best of 5 replays, HIP events around each.  Per pair and layer: the sums over the ten
steps, the A/A spread (the larger of |r - r'| and |k - k'| of the sums) and the verdict - a layout is ahead only if the sums differ
by more than that spread.  The outputs of (r) and (k) are compared bit for bit on every ring entry before anything is timed.
usage: ab_w6_km.py [--quick]"""
import hashlib
import json
import os
import subprocess
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

from fpqvar_amd import _lib, gemm, kv_cache  # noqa: E402

QUICK = "--quick" in sys.argv
dev = torch.device("cuda:0")
torch.manual_seed(0)
K, BATCH, HEADS = 1920, 100, 30
PNS = (1, 2, 3, 4, 5, 6, 8, 10, 13, 16)
LAYERS = (("qkv", 3 * K), ("fc1", 4 * K), ("proj", K))
PAIRS = (("e2m1", "e3m0"), ("e1m2", "e1m2"), ("e3m0", "e1m2"))     # one per activation format
RING_BYTES = 320 << 20
RING_MAX = 128
FORMS = ("r", "r'", "k", "k'")


def quantize_a(table, x, kmajor):
    return gemm.quantize_mx(x, kmajor=kmajor) if table == "e2m1" else gemm.quantize_g6(x, table, kmajor=kmajor)


def ring_len(tokens, outs):
    per_set = tokens * K * 2 + outs * K * 3 // 4 + tokens * outs * 2      # cold bytes per call: x, the weight codes, the output
    return max(2, min(RING_MAX, RING_BYTES // per_set + 1))


def weights(layer, outs, w_table):
    """the layer's ring of weights, both layouts, for its smallest step (the longest ring)"""
    n = ring_len(BATCH, outs)
    w6 = [gemm.quantize_g6(torch.randn(outs, K, device=dev) * 0.02, w_table) for _ in range(n)]
    wk = [(gemm.to_kmajor(c, 6, dealt=True), gemm.to_kmajor_scales(s, weight_side=True)) for c, s in w6]
    return w6, wk


def build(pn, layer, outs, pair, w6, wk):
    """{form: graph replaying one call per ring entry}, ring length"""
    at, wt = pair
    seq = pn * pn
    tokens = BATCH * seq
    ring = min(ring_len(tokens, outs), len(w6))
    xs = [torch.randn(tokens, K, device=dev).half() for _ in range(ring)]
    if layer == "qkv":
        bias = torch.randn(outs, device=dev) * 0.1
        bias[K:2 * K] = 0
        hs = kv_cache.qk_norm_head_scale(torch.full((1, HEADS, 1, 1), 4.0, device=dev).log())
        caches = {f: torch.zeros(2, BATCH, seq, HEADS, 64, dtype=torch.float16, device=dev) for f in ("r", "k")}
        row = lambda i: gemm.linear_w6_qkv_to_cache(*quantize_a(at, xs[i], False), at, *w6[i], wt, bias, caches["r"], 0, seq, hs)
        km = lambda i: gemm.linear_w6_qkv_to_cache_km(*quantize_a(at, xs[i], True), at, *wk[i], wt, bias, caches["k"], 0, seq, hs)
    else:
        bias = (torch.randn(outs, device=dev) * 0.1).half()
        caches = None
        lin_r, lin_k = (gemm.linear_w6_gelu_dual, gemm.linear_w6_gelu_dual_km) if layer == "fc1" else (gemm.linear_w6, gemm.linear_w6_km)
        row = lambda i: lin_r(*quantize_a(at, xs[i], False), at, *w6[i], wt, bias)
        km = lambda i: lin_k(*quantize_a(at, xs[i], True), at, *wk[i], wt, bias)
    calls = {"r": row, "r'": row, "k": km, "k'": km}
    for i in range(ring):                                                  # faster and different is not faster
        a, b = row(i), km(i)
        same = torch.equal(a.view(torch.int16), b.view(torch.int16))
        if caches is not None:
            same = same and torch.equal(caches["r"].view(torch.int16), caches["k"].view(torch.int16))
        if not same:
            raise SystemExit(f"{pair} {layer} [{tokens} x {K} -> {outs}]: the k-major result differs from the row-major one")
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
    return graphs, ring, (keep, xs, caches)


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


def line(pn, layer, outs, pair, w6, wk):
    graphs, ring, keep = build(pn, layer, outs, pair, w6, wk)
    r = measure(graphs, ring)
    aa = max(abs(r["r"] - r["r'"]) / r["r"], abs(r["k"] - r["k'"]) / r["k"]) * 100
    print(f"{BATCH * pn * pn:7d} {pair[0]}-{pair[1]} {layer:4s} {K:5d} {outs:5d}  ring {ring:3d}   " + "  ".join(f"{r[f]:9.1f}" for f in FORMS) +
          f"    {r['r'] / r['k']:5.2f}   {aa:4.1f} %", flush=True)
    del graphs, keep
    torch.cuda.empty_cache()
    return r


def verdict(tot):
    """sums of forms r, r', k, k' -> (spread, 'k-major ahead' / 'row-major ahead' / 'inside the spread')"""
    spread = max(abs(tot["r"] - tot["r'"]), abs(tot["k"] - tot["k'"]))
    ra, kb = min(tot["r"], tot["r'"]), min(tot["k"], tot["k'"])
    return spread, ("k-major ahead" if ra - kb > spread else "row-major ahead" if kb - ra > spread else "inside the spread")


def main():
    try:
        commit = subprocess.run(["git", "rev-parse", "--short", "HEAD"], capture_output=True, text=True, cwd=os.path.dirname(__file__)).stdout.strip()
    except OSError:
        commit = ""
    sha = hashlib.sha256(open(_lib.LIB_PATH, "rb").read()).hexdigest()[:16]
    print(f"# tools/ab_w6_km.py{' --quick' if QUICK else ''}: commit {commit or '(working tree)'}, libfpq_hip.so sha256 {sha}, "
          f"build tag {_lib.build_tag()}, {torch.cuda.get_device_name(0)}")
    print("# us per activation quantizer + GEMM, best of 5 alternating graph replays, cold operands (ring > 256 MiB); (r) == (k) bit for bit")
    print("#  tokens pair      layer   K  outs  ring            (r)       (r')        (k)       (k')      r/k    A/A")
    verdicts = {}
    for pair in PAIRS:
        for layer, outs in LAYERS:
            w6, wk = weights(layer, outs, pair[1])
            tot = {f: 0.0 for f in FORMS}
            steps = {}
            for pn in (PNS[-3:] if QUICK else PNS):
                r = line(pn, layer, outs, pair, w6, wk)
                steps[BATCH * pn * pn] = round(r["r"] / r["k"], 3)
                for f in FORMS:
                    tot[f] += r[f]
            spread, who = verdict(tot)
            print(f"# {pair[0]}-{pair[1]} {layer}: sum over the steps  " + "  ".join(f"({f}) {tot[f]:9.1f}" for f in FORMS) +
                  f"   A/A spread {spread:.1f} us ({spread / tot['r'] * 100:.2f} %)   row-major / k-major {tot['r'] / tot['k']:.3f}   {who}", flush=True)
            verdicts[f"{pair[0]}-{pair[1]} {layer}"] = {"sum_us": {f: round(tot[f], 1) for f in FORMS}, "aa_spread_us": round(spread, 1),
                                                        "verdict": who, "r_over_k_per_step": steps}
            del w6, wk
            torch.cuda.empty_cache()
    print(json.dumps({"quick": QUICK, "layers": verdicts}))


if __name__ == "__main__":
    main()
