#!/usr/bin/env python3
"""The gated residual x = x + y.mul(gate) and the adaLN producer that reads the row it just wrote, as one launch against the two
(three) launches the library ran before (tools/ab_gf6_producers.py is the method):

  (a)   rotation.resid_adaln_rotate_quant_mx / _token(y, gate, x, sc, sh, ...)                  one launch: x_new and the operands out
  (a')  the same again                                                                         the tool's own A/A spread
  (b)   fp16 rows: ops.gate_residual(y, gate, x), then the twin producer on its result         two launches
        fp32 rows: torch's y.mul(gate) and x + that (fpq_gate_residual refuses fp32 rows), then the twin      three launches
  (b')  the same again

(a) is checked against its contract on every ring entry before anything is timed: x_new bit for bit torch's x + y.mul(gate), the
operands byte for byte the twin's on x_new.
Per row dtype (fp32: the model's residual stream under autocast; fp16) and form - FP4 operands row-major and k-major, per-token fp6
codes (E2M3, row-major) - C = 1920 (d30, B = 100) and 2304 (d36-512, B = 20) at the ten scale-step row counts.  One process; every
form works through a ring of inputs larger than the 256 MiB of L2 + Infinity Cache (cold rows); a form's sweep over its ring is
captured once as a HIP graph and replayed; the forms alternate, best of 5 replays, HIP events around each.  Per model, dtype and
form: the sums over the ten steps, the A/A spread (the larger of |a - a'| and |b - b'|) and one of three statements - (a) ahead by
more than the spread, inside it, or behind - for the sum and for every row count; every row count that is behind is listed.
Nothing is routed by these numbers (fuse_residual and pending= are off by default): no threshold is derived.
The header names the commit: `git rev-parse`, or FPQ_GIT_HEAD where the tree is no git checkout.
usage: ab_resid_adaln.py [--quick] [--rows fp16|fp32|both]"""
import hashlib
import json
import os
import subprocess
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

from fpqvar_amd import _lib, ops, rotation as rot  # noqa: E402

QUICK = "--quick" in sys.argv
ROWS = sys.argv[sys.argv.index("--rows") + 1] if "--rows" in sys.argv else "both"
dev = torch.device("cuda:0")
torch.manual_seed(0)
MODELS = (("d30", 1920, 100, (1, 2, 3, 4, 5, 6, 8, 10, 13, 16)), ("d36", 2304, 20, (1, 2, 3, 4, 6, 9, 13, 18, 24, 32)))
KINDS = ("fp4 row-major", "fp4 k-major", "token fp6")
RING_BYTES = 640 << 20
FORMS = ("a", "a'", "b", "b'")


def producers(kind, sc, sh, sm):
    """(fused(y, gate, x) -> (x_new, *operands), twin(x) -> operands)"""
    if kind.startswith("fp4"):
        km = kind.endswith("k-major")
        return (lambda y, g, x: rot.resid_adaln_rotate_quant_mx(y, g, x, sc, sh, smooth=sm, kmajor=km),
                lambda x: rot.adaln_rotate_quant_mx(x, sc, sh, smooth=sm, kmajor=km))
    return (lambda y, g, x: rot.resid_adaln_rotate_quant_token(y, g, x, sc, sh, "e2m3", smooth=sm, emit="fp6"),
            lambda x: rot.adaln_rotate_quant_token(x, sc, sh, "e2m3", smooth=sm, emit="fp6"))


def build(batch, seq, c, kind, rows_dtype):
    """{form: graph replaying one call per ring entry}, ring length"""
    x_bytes = 4 if rows_dtype == "fp32" else 2
    per_set = batch * seq * c * (2 * x_bytes + 2) + batch * seq * c * 3 // 4   # cold bytes per call: x in and out, y, the codes
    ring = max(2, min(32, RING_BYTES // per_set + 1))
    xs = [torch.randn(batch, seq, c, device=dev) if rows_dtype == "fp32" else torch.randn(batch, seq, c, device=dev).half() for _ in range(ring)]
    ys = [torch.randn(batch, seq, c, device=dev).half() for _ in range(ring)]
    gate = (torch.randn(batch, 1, c, device=dev) * 0.5).half()
    sc = (torch.randn(batch, 1, c, device=dev) * 0.3).half()
    sh = (torch.randn(batch, 1, c, device=dev) * 0.3).half()
    sm = torch.rand(c, device=dev) + 0.5
    fused, twin = producers(kind, sc, sh, sm)
    one = lambda i: fused(ys[i], gate, xs[i])
    if rows_dtype == "fp32":
        def chain(i):
            x_new = xs[i] + ys[i].mul(gate)
            return (x_new, *twin(x_new))
    else:
        def chain(i):
            x_new = ops.gate_residual(ys[i], gate, xs[i])
            return (x_new, *twin(x_new))
    calls = {"a": one, "a'": one, "b": chain, "b'": chain}
    for i in range(ring):                                                  # faster and different is not faster: (a) against its contract
        got = one(i)
        x_new = xs[i] + ys[i].mul(gate)
        want = (x_new, *twin(x_new))
        for p, q in zip(got, want):
            if not (p.dtype == q.dtype and torch.equal(p.contiguous().view(torch.uint8), q.contiguous().view(torch.uint8))):
                raise SystemExit(f"[{batch} x {seq} x {c}] {rows_dtype} {kind}: (a) differs from torch's x + y.mul(gate) and the twin on it")
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


def measure(graphs, ring, rounds=5, forms=FORMS):
    best = {f: 1e30 for f in forms}
    for f in forms:
        graphs[f].replay()
    torch.cuda.synchronize()
    for _ in range(rounds):
        for f in forms:
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            graphs[f].replay()
            e1.record()
            torch.cuda.synchronize()
            best[f] = min(best[f], e0.elapsed_time(e1) / ring * 1e3)
    return best


def verdict(t):
    """(spread, statement) for a line or a sum"""
    spread = max(abs(t["a"] - t["a'"]), abs(t["b"] - t["b'"]))
    a, b = min(t["a"], t["a'"]), min(t["b"], t["b'"])
    return spread, ("(a) ahead" if b - a > spread else "(a) BEHIND" if a - b > spread else "inside the spread")


def line(batch, seq, name, c, kind, rows_dtype):
    graphs, ring, keep = build(batch, seq, c, kind, rows_dtype)
    r = measure(graphs, ring)
    spread, who = verdict(r)
    print(f"{batch * seq:7d} {name:4s} {c:5d} {rows_dtype:4s} {kind:13s} ring {ring:2d}   " + "  ".join(f"{r[f]:9.1f}" for f in FORMS) +
          f"    {r['b'] / r['a']:5.2f}   {spread:6.1f}   {who}", flush=True)
    del graphs, keep
    torch.cuda.empty_cache()
    return r, who


def main():
    try:
        commit = subprocess.run(["git", "rev-parse", "--short", "HEAD"], capture_output=True, text=True, cwd=os.path.dirname(__file__)).stdout.strip()
    except OSError:
        commit = ""
    commit = commit or os.environ.get("FPQ_GIT_HEAD", "")
    sha = hashlib.sha256(open(_lib.LIB_PATH, "rb").read()).hexdigest()[:16]
    print(f"# tools/ab_resid_adaln.py{' --quick' if QUICK else ''} --rows {ROWS}: commit {commit or 'unknown (no .git here: set FPQ_GIT_HEAD)'}, libfpq_hip.so sha256 {sha}, "
          f"build tag {_lib.build_tag()}, {torch.cuda.get_device_name(0)}")
    print("# us per call of the chain, best of 5 alternating graph replays, cold rows (ring > 256 MiB), fp16 modulation, a smoothing vector;")
    print("# (a) one launch: resid_adaln_rotate_quant_*; (b) gate_residual (fp32 rows: torch's mul, add) + the twin producer; (a) == (b) byte for byte")
    print("#   rows model    C rows form          ring          (a)       (a')        (b)       (b')     b/a   spread  statement")
    out = {}
    for rows_dtype in (("fp32", "fp16") if ROWS == "both" else (ROWS,)):
        for name, c, batch, pns in MODELS:
            for kind in KINDS:
                tot = {f: 0.0 for f in FORMS}
                behind = []
                for pn in (pns[-3:] if QUICK else pns):
                    r, who = line(batch, pn * pn, name, c, kind, rows_dtype)
                    for f in FORMS:
                        tot[f] += r[f]
                    if "BEHIND" in who:
                        behind.append(batch * pn * pn)
                spread, who = verdict(tot)
                key = f"{name} {rows_dtype} {kind}"
                print(f"# {key}: sum over the steps  " + "  ".join(f"({f}) {tot[f]:9.1f}" for f in FORMS) +
                      f"   A/A spread {spread:.1f} us ({spread / tot['a'] * 100:.2f} %)   (b) / (a) {tot['b'] / tot['a']:.3f}   {who}; "
                      f"row counts behind: {behind if behind else 'none'}")
                out[key] = {"sum_us": {f: round(tot[f], 1) for f in FORMS}, "aa_spread_us": round(spread, 1), "statement": who, "rows_behind": behind}
    print(json.dumps({"rows": ROWS, "quick": QUICK, "chains": out}))


if __name__ == "__main__":
    main()
