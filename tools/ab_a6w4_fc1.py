#!/usr/bin/env python3
"""fc1 of a mixed-format W4A4 block with a 6-bit activation: the fc1 tail fused into the A6W4 GEMM beside the two sequences such a
layer ran before, producer included, row-major operands, fp32 weight scales, a bias:

  (f)   quantize_g6(x, table) + linear_a6w4_gelu_dual                                   one GEMM launch (+ the NaN fix-up launch)
  (f')  the same again                                                                  the tool's own A/A spread
  (u3)  quantize_g6 + linear_a6w4 + F.gelu(approximate="tanh") + ops.quant_rows_dual    GEMM, torch's GELU, the dual quantizer
  (u1)  quantize_g6 + linear_a6w4 + ops.gelu_quant_rows_dual                            GEMM, GELU + quantizer in one pass

d30 (K = 1920 -> 7680, B = 100) and d36-512 (K = 2304 -> 9216, B = 20) at the ten scale-step row counts and at 65 536 rows.
One process; every form works through a ring of operand sets larger than the 256 MiB of L2 + Infinity Cache (cold operands); a
form's sweep over its ring is captured once as a HIP graph and replayed; the forms alternate, best of 5 replays, HIP events
around each.  Per model: the sums over the ten steps, the A/A spread |f - f'| of the sums, and the verdict - the fused form
loses only if it is slower than the better of (u3), (u1) by more than that spread.
usage: ab_a6w4_fc1.py [--quick] [--table e3m0|e1m2]"""
import hashlib
import json
import os
import subprocess
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402
import torch.nn.functional as Fn  # noqa: E402

from fpqvar_amd import _lib, gemm, ops  # noqa: E402

QUICK = "--quick" in sys.argv
TABLE = sys.argv[sys.argv.index("--table") + 1] if "--table" in sys.argv else "e3m0"
dev = torch.device("cuda:0")
torch.manual_seed(0)
MODELS = (("d30", 1920, 100, (1, 2, 3, 4, 5, 6, 8, 10, 13, 16)), ("d36", 2304, 20, (1, 2, 3, 4, 6, 9, 13, 18, 24, 32)))
RING_BYTES = 640 << 20
FORMS = ("f", "f'", "u3", "u1")


def build(tokens, k, outs):
    """{form: graph replaying one call per ring entry}, ring length"""
    per_set = tokens * k * 2 + outs * k // 2 + 3 * tokens * outs * 2      # (u3)'s cold bytes per call: x, the weight codes, y, h and q
    ring = max(2, min(32, RING_BYTES // per_set + 1))
    xs = [torch.randn(tokens, k, device=dev).half() for _ in range(ring)]
    w4 = [gemm.quantize_mx(torch.randn(outs, k, device=dev) * 0.02) for _ in range(ring)]
    bias = (torch.randn(outs, device=dev) * 0.1).half()
    fused = lambda i: gemm.linear_a6w4_gelu_dual(*gemm.quantize_g6(xs[i], TABLE), TABLE, *w4[i], bias)
    plain = lambda i: gemm.linear_a6w4(*gemm.quantize_g6(xs[i], TABLE), TABLE, *w4[i], bias)
    calls = {
        "f": fused,
        "f'": fused,
        "u3": lambda i: ops.quant_rows_dual(Fn.gelu(plain(i), approximate="tanh"), "e1m2_neg", "e2m1_pos", 128, 1.0),
        "u1": lambda i: ops.gelu_quant_rows_dual(plain(i)),
    }
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


def line(tokens, name, k, outs):
    graphs, ring, keep = build(tokens, k, outs)
    r = measure(graphs, ring)
    better = min(r["u3"], r["u1"])
    print(f"{tokens:7d} {name:4s} {k:5d} {outs:5d}  ring {ring:2d}   " + "  ".join(f"{r[f]:9.1f}" for f in FORMS) +
          f"    {r['u3'] / r['f']:5.2f}  {r['u1'] / r['f']:5.2f}   {abs(r['f'] - r[FORMS[1]]) / r['f'] * 100:4.1f} %   {better / r['f']:5.2f}", flush=True)
    del graphs, keep
    torch.cuda.empty_cache()
    return r


def main():
    try:
        commit = subprocess.run(["git", "rev-parse", "--short", "HEAD"], capture_output=True, text=True, cwd=os.path.dirname(__file__)).stdout.strip()
    except OSError:
        commit = ""
    sha = hashlib.sha256(open(_lib.LIB_PATH, "rb").read()).hexdigest()[:16]
    print(f"# tools/ab_a6w4_fc1.py{' --quick' if QUICK else ''} --table {TABLE}: commit {commit or '(working tree)'}, libfpq_hip.so sha256 {sha}, "
          f"build tag {_lib.build_tag()}, {torch.cuda.get_device_name(0)}")
    print("# us per producer + fc1 + GELU + dual quantizer, best of 5 alternating graph replays, cold operands (ring > 256 MiB), row-major operands")
    print("#  tokens model     K  outs  ring          (f)       (f')       (u3)       (u1)     u3/f   u1/f    A/A   better/f")
    verdicts = {}
    for name, k, batch, pns in MODELS:
        tot = {f: 0.0 for f in FORMS}
        for pn in (pns[-3:] if QUICK else pns):
            r = line(batch * pn * pn, name, k, 4 * k)
            for f in FORMS:
                tot[f] += r[f]
        line(65536, name, k, 4 * k)
        spread = abs(tot["f"] - tot["f'"])
        better = min(("u3", "u1"), key=lambda f: tot[f])
        loses = min(tot["f"], tot["f'"]) - tot[better] > spread
        print(f"# {name}: sum over the steps  " + "  ".join(f"({f}) {tot[f]:9.1f}" for f in FORMS) +
              f"   A/A spread {spread:.1f} us ({spread / tot['f'] * 100:.2f} %)   better parent sequence ({better}) / fused {tot[better] / tot['f']:.3f}"
              f"   fused {'LOSES' if loses else 'does not lose'} outside the spread")
        verdicts[name] = {"sum_us": {f: round(tot[f], 1) for f in FORMS}, "aa_spread_us": round(spread, 1), "better_parent": better,
                          "better_over_fused": round(tot[better] / tot["f"], 3), "fused_loses": bool(loses)}
    print(json.dumps({"table": TABLE, "quick": QUICK, "models": verdicts}))


if __name__ == "__main__":
    main()
