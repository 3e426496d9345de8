#!/usr/bin/env python3
"""The producer in front of a mixed-format W4A4 block's mat_qkv / fc1 with an E3M0 / E1M2 activation - LayerNorm, adaLN modulate,
smooth, rotate, per-group quantize to the A6W4 GEMM's operands - as one launch against the cheapest chain the library offered
before it:

  (a)   rotation.adaln_rotate_quant_g6(x, sc, sh, table, smooth, kmajor)                          one launch, operands out
  (a')  the same again                                                                             the tool's own A/A spread
  (b)   gemm.quantize_g6(rotation.adaln_rotate_quant(x, sc, sh, table, smooth), table, kmajor)     two launches, fp16 rows between them
  (b')  the same again

(b) is a timing baseline only: it quantizes already quantized values, which is not promised to give (a)'s bytes.  What (a) is
checked against, on every ring entry before anything is timed, is its contract: gemm.quantize_g6 of the rotated rows the values
form emits.
Per table (e3m0, e1m2) and layout (row-major, k-major), C = 1920 (d30, B = 100) and 2304 (d36-512, B = 20) at the ten scale-step
row counts (tools/bench_small_steps.py).  One process; every form works through a ring of inputs larger than
the 256 MiB of L2 + Infinity Cache (cold rows); a form's sweep over its ring is captured once as a HIP graph and replayed; the
forms alternate, best of 5 replays, HIP events around each.  Per model, table and layout: the sums over the ten steps, the A/A
spread (the larger of |a - a'| and |b - b'| of the sums) and the verdict - a chain is ahead only if the sums differ by more than
that spread.
The header names the commit: `git rev-parse`, or FPQ_GIT_HEAD where the tree is no git checkout (tools/collect_profiles.sh).
usage: ab_g6_producers.py [--quick] [--big] [--rows fp16|fp32]      --big: a line at 65 536 rows per chain too"""
import hashlib
import json
import os
import subprocess
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

from fpqvar_amd import _lib, gemm, rotation as rot  # noqa: E402

QUICK = "--quick" in sys.argv
BIG = "--big" in sys.argv
ROWS = sys.argv[sys.argv.index("--rows") + 1] if "--rows" in sys.argv else "fp32"   # fp32: the model's residual stream
dev = torch.device("cuda:0")
torch.manual_seed(0)
MODELS = (("d30", 1920, 100, (1, 2, 3, 4, 5, 6, 8, 10, 13, 16)), ("d36", 2304, 20, (1, 2, 3, 4, 6, 9, 13, 18, 24, 32)))
TABLES = ("e3m0", "e1m2")
RING_BYTES = 640 << 20
FORMS = ("a", "a'", "b", "b'")


def build(batch, seq, c, table, kmajor):
    """{form: graph replaying one call per ring entry}, ring length"""
    x_bytes = 4 if ROWS == "fp32" else 2
    per_set = batch * seq * c * x_bytes + batch * seq * c * 3 // 4          # cold bytes per call: the rows, the codes
    ring = max(2, min(32, RING_BYTES // per_set + 1))
    xs = [torch.randn(batch, seq, c, device=dev) if ROWS == "fp32" else torch.randn(batch, seq, c, device=dev).half() for _ in range(ring)]
    sc = (torch.randn(batch, 1, c, device=dev) * 0.3).half()
    sh = (torch.randn(batch, 1, c, device=dev) * 0.3).half()
    sm = torch.rand(c, device=dev) + 0.5
    one = lambda i: rot.adaln_rotate_quant_g6(xs[i], sc, sh, table, smooth=sm, kmajor=kmajor)
    two = lambda i: gemm.quantize_g6(rot.adaln_rotate_quant(xs[i], sc, sh, table, smooth=sm).view(-1, c), table, kmajor=kmajor)
    calls = {"a": one, "a'": one, "b": two, "b'": two}
    rows = batch * seq
    for i in range(ring):                                                  # faster and different is not faster: (a) against its contract
        y = rot.adaln_rotate_quant(xs[i], sc, sh, table, smooth=sm, return_intermediates=True)[2].view(-1, c)
        got, want = one(i), gemm.quantize_g6(y, table, kmajor=kmajor)
        live = (lambda s: s[:, :rows]) if kmajor else (lambda s: s)
        if not (torch.equal(got[0], want[0]) and torch.equal(live(got[1]).contiguous().view(torch.uint8), live(want[1]).contiguous().view(torch.uint8))):
            raise SystemExit(f"[{batch} x {seq} x {c}] {table} kmajor={kmajor}: (a) differs from quantize_g6 of the rotated rows")
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


def line(batch, seq, name, c, table, kmajor):
    graphs, ring, keep = build(batch, seq, c, table, kmajor)
    r = measure(graphs, ring)
    aa = max(abs(r["a"] - r["a'"]) / r["a"], abs(r["b"] - r["b'"]) / r["b"]) * 100
    print(f"{batch * seq:7d} {name:4s} {c:5d} {table:5s} {'k-major' if kmajor else 'row-major':9s} ring {ring:2d}   " +
          "  ".join(f"{r[f]:9.1f}" for f in FORMS) + f"    {r['b'] / r['a']:5.2f}   {aa:4.1f} %", flush=True)
    del graphs, keep
    torch.cuda.empty_cache()
    return r


def verdict(tot):
    spread = max(abs(tot["a"] - tot["a'"]), abs(tot["b"] - tot["b'"]))
    a, b = min(tot["a"], tot["a'"]), min(tot["b"], tot["b'"])
    return spread, ("one launch ahead" if b - a > spread else "two launches ahead" if a - b > spread else "inside the spread")


def main():
    try:
        commit = subprocess.run(["git", "rev-parse", "--short", "HEAD"], capture_output=True, text=True, cwd=os.path.dirname(__file__)).stdout.strip()
    except OSError:
        commit = ""
    commit = commit or os.environ.get("FPQ_GIT_HEAD", "")
    sha = hashlib.sha256(open(_lib.LIB_PATH, "rb").read()).hexdigest()[:16]
    print(f"# tools/ab_g6_producers.py{' --quick' if QUICK else ''}{' --big' if BIG else ''} --rows {ROWS}: commit {commit or 'unknown (no .git here: set FPQ_GIT_HEAD)'}, libfpq_hip.so sha256 {sha}, "
          f"build tag {_lib.build_tag()}, {torch.cuda.get_device_name(0)}")
    print("# us per call of the producer chain, best of 5 alternating graph replays, cold rows (ring > 256 MiB), fp16 modulation, a smoothing vector;")
    print("# (a) one launch: adaln_rotate_quant_g6; (b) two launches: adaln_rotate_quant + quantize_g6; (a) == quantize_g6(rotated rows) byte for byte")
    print("#   rows model    C table layout    ring          (a)       (a')        (b)       (b')     b/a    A/A")
    verdicts = {}
    for name, c, batch, pns in MODELS:
        for table in TABLES:
            for kmajor in (False, True):
                tot = {f: 0.0 for f in FORMS}
                for pn in (pns[-3:] if QUICK else pns):
                    r = line(batch, pn * pn, name, c, table, kmajor)
                    for f in FORMS:
                        tot[f] += r[f]
                big = line(64, 1024, name, c, table, kmajor) if BIG else None
                spread, who = verdict(tot)
                key = f"{name} {table} {'k-major' if kmajor else 'row-major'}"
                print(f"# {key}: sum over the steps  " + "  ".join(f"({f}) {tot[f]:9.1f}" for f in FORMS) +
                      f"   A/A spread {spread:.1f} us ({spread / tot['a'] * 100:.2f} %)   two launches / one launch {tot['b'] / tot['a']:.3f}   {who}")
                verdicts[key] = {"sum_us": {f: round(tot[f], 1) for f in FORMS}, "aa_spread_us": round(spread, 1), "verdict": who,
                                 "at_65536_us": {f: round(big[f], 1) for f in FORMS} if big else None}
    print(json.dumps({"rows": ROWS, "quick": QUICK, "chains": verdicts}))


if __name__ == "__main__":
    main()
