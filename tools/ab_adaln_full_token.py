#!/usr/bin/env python3
"""tools/ab_adaln_full.py's measurement for the PER-TOKEN configuration (W6A6) in the FULL-WIDTH mode: the producer in front of
mat_qkv / fc1 - LN(x).mul(scale.add(1)).add_(shift), rotate with the C x C randomized Hadamard matrix, fp6_quant_e2m3_per_token -
as one launch against what a W6A6 full-width user ran before it:

  (f)   rotation.adaln_rotate_quant_full_token(x, scale, shift) / (..., emit="fp6", kmajor=True)              one launch
  (f')  the same again                                                                                      the tool's own A/A spread
  (a)   torch's layer_norm / mul(scale.add(1)) / add_(shift), matmul with half(Q), then fp6_quant_e2m3_per_token_cuda (values) or
        gemm.quantize_fp6(kmajor=True) (operands)                                                           today's chain
  (a')  the same again
  (b)   rotation.adaln_rotate_quant_full(return_intermediates=True), then the stand-alone quantizer on `rotated`
  (y)   rotation.adaln_rotate_quant_token / (..., emit="fp6", kmajor=True): the 128-block form - ANOTHER rotation, the memory-bound yardstick

(f) is checked against its contract on every ring entry before anything is timed: bit for bit (b)'s output.
C = 1920 (d30, B = 100) and 2304 (d36-512, B = 20) at the ten scale-step row counts [B, pn^2, C]: fp32 rows, fp16 modulation (the
model's case), no smoothing vector.  One process; every form works through a ring of inputs larger than the 256 MiB of L2 + Infinity
Cache (cold rows); a form's sweep over its ring is captured once as a HIP graph and replayed; the forms alternate, best of 5 replays,
HIP events around each.  Per model and output: the sums over the ten steps, the A/A spread (the largest |form - form'| of the sums)
and every step where (f) is not ahead of (a) by more than the step's own A/A difference.  --big: a line at [65536 x 1920] (B = 64).
The header names the commit: `git rev-parse`, or FPQ_GIT_HEAD where the tree is no git checkout.
usage: ab_adaln_full_token.py [--quick] [--big]"""
import hashlib
import json
import os
import subprocess
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

from fpqvar_amd import _lib, gemm, quant_utils as qu, rotation as rot  # noqa: E402

QUICK = "--quick" in sys.argv
BIG = "--big" in sys.argv
dev = torch.device("cuda:0")
torch.manual_seed(0)
MODELS = (("d30", 1920, 100, (1, 2, 3, 4, 5, 6, 8, 10, 13, 16)), ("d36", 2304, 20, (1, 2, 3, 4, 6, 9, 13, 18, 24, 32)))
RING_BYTES = 640 << 20
FORMS = ("f", "f'", "a", "a'", "b", "y")
HBM = 8e12
_Q = {}


def q_half(c):
    if c not in _Q:
        _Q[c] = rot.get_orthogonal_matrix(c, device=dev).float().half()
    return _Q[c]


def out_bytes(rows, c, ops):
    return rows * c * 3 // 4 + rows * 2 if ops else rows * c * 2


def build(batch, seq, c, ops):
    """{form: graph replaying one call per ring entry}, ring length"""
    rows = batch * seq
    per_set = rows * c * 4 + out_bytes(rows, c, ops)                       # cold bytes per call: the fp32 rows, what is written
    ring = max(2, min(32, RING_BYTES // per_set + 1))
    xs = [torch.randn(batch, seq, c, device=dev) * 1.3 + 0.2 for _ in range(ring)]
    sc = (torch.randn(batch, 1, c, device=dev) * 0.3).half()
    sh = (torch.randn(batch, 1, c, device=dev) * 0.3).half()
    q = q_half(c)
    alone = (lambda y: gemm.quantize_fp6(y.view(rows, c), kmajor=True)) if ops else (lambda y: qu.fp6_quant_e2m3_per_token_cuda(y, 6))

    def chain(i):
        with torch.autocast("cuda", dtype=torch.float16):
            return torch.matmul(torch.nn.functional.layer_norm(xs[i], (c,), eps=1e-6).mul(sc.add(1)).add_(sh), q)
    if ops:
        fused = lambda i: rot.adaln_rotate_quant_full_token(xs[i], sc, sh, emit="fp6", kmajor=True)
        block = lambda i: rot.adaln_rotate_quant_token(xs[i], sc, sh, emit="fp6", kmajor=True)
    else:
        fused = lambda i: rot.adaln_rotate_quant_full_token(xs[i], sc, sh)
        block = lambda i: rot.adaln_rotate_quant_token(xs[i], sc, sh)
    today = lambda i: alone(chain(i))
    two = lambda i: alone(rot.adaln_rotate_quant_full(xs[i], sc, sh, return_intermediates=True)[2])
    calls = {"f": fused, "f'": fused, "a": today, "a'": today, "b": two, "y": block}
    for i in range(ring):                                                  # faster and different is not faster: (f) against its contract
        got, want = fused(i), two(i)
        same = (torch.equal(got[0], want[0]) and torch.equal(got[1].view(torch.int16), want[1].view(torch.int16))) if ops else \
            torch.equal(got.view(torch.int16), want.view(torch.int16))
        if not same:
            raise SystemExit(f"[{batch} x {seq} x {c}] operands={ops}: (f) differs from the stand-alone quantizer behind adaln_rotate_quant_full")
        del got, want
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


def line(batch, seq, name, c, ops):
    graphs, ring, keep = build(batch, seq, c, ops)
    r = measure(graphs, ring)
    aa = max(abs(r[f] - r[f + "'"]) / r[f] for f in ("f", "a")) * 100
    print(f"{batch * seq:7d} {name:4s} {c:5d} {'operands' if ops else 'values':8s} ring {ring:2d}   " + "  ".join(f"{r[f]:9.1f}" for f in FORMS) +
          f"    {r['a'] / r['f']:6.2f}  {r['b'] / r['f']:6.2f}  {r['f'] / r['y']:6.2f}   {aa:4.1f} %", flush=True)
    del graphs, keep
    torch.cuda.empty_cache()
    return r


def main():
    try:
        commit = subprocess.run(["git", "rev-parse", "--short", "HEAD"], capture_output=True, text=True, cwd=os.path.dirname(__file__)).stdout.strip()
    except OSError:
        commit = ""
    commit = commit or os.environ.get("FPQ_GIT_HEAD", "")
    sha = hashlib.sha256(open(_lib.LIB_PATH, "rb").read()).hexdigest()[:16]
    print(f"# tools/ab_adaln_full_token.py{' --quick' if QUICK else ''}{' --big' if BIG else ''}: commit {commit or 'unknown (no .git here: set FPQ_GIT_HEAD)'}, "
          f"libfpq_hip.so sha256 {sha}, build tag {_lib.build_tag()}, {torch.cuda.get_device_name(0)}")
    print("# us per call, best of 5 alternating graph replays, cold fp32 rows (ring > 256 MiB), fp16 modulation, per-token E2M3, no smoothing vector;")
    print("# (f) one launch: adaln_rotate_quant_full_token; (a) torch layer_norm / mul / add_ + matmul(half(Q)) + the stand-alone quantizer; "
          "(b) adaln_rotate_quant_full + the stand-alone quantizer; (y) the 128-block form adaln_rotate_quant_token; operands: k-major FP6 image")
    print("#   rows model    C output   ring          (f)       (f')        (a)       (a')        (b)        (y)      a/f     b/f     f/y    A/A")
    verdicts = {}
    for name, c, batch, pns in MODELS:
        for ops in (False, True):
            tot, lost = {f: 0.0 for f in FORMS}, []
            for pn in (pns[-3:] if QUICK else pns):
                r = line(batch, pn * pn, name, c, ops)
                for f in FORMS:
                    tot[f] += r[f]
                if min(r["a"], r["a'"]) - max(r["f"], r["f'"]) <= max(abs(r[f] - r[f + "'"]) for f in ("f", "a")):
                    lost.append(batch * pn * pn)
            spread = max(abs(tot[f] - tot[f + "'"]) for f in ("f", "a"))
            fu, a = min(tot["f"], tot["f'"]), min(tot["a"], tot["a'"])
            who = "one launch ahead" if a - fu > spread else "today's chain ahead" if fu - a > spread else "inside the spread"
            key = f"{name} {'operands' if ops else 'values'}"
            print(f"# {key}: sum over the steps  " + "  ".join(f"({f}) {tot[f]:9.1f}" for f in FORMS) +
                  f"   A/A spread {spread:.1f} us   (a) / (f) {tot['a'] / tot['f']:.2f}   (b) / (f) {tot['b'] / tot['f']:.2f}   (f) / (y) {tot['f'] / tot['y']:.2f}   "
                  f"{who}; steps where (f) is not ahead of (a) by more than the spread: {lost or 'none'}")
            verdicts[key] = {"sum_us": {f: round(tot[f], 1) for f in FORMS}, "aa_spread_us": round(spread, 1), "verdict": who, "f_not_ahead_at_rows": lost}
    if BIG:
        for ops in (False, True):
            r = line(64, 1024, "big", 1920, ops)
            traffic = 65536 * 1920 * 4 + out_bytes(65536, 1920, ops)
            print(f"# [65536 x 1920] {'operands' if ops else 'values'}: {traffic / 1e6:.0f} MB per call; (f) {traffic / (r['f'] * 1e-6) / HBM:.2f} of 8 TB/s, "
                  f"(y) {traffic / (r['y'] * 1e-6) / HBM:.2f}, (a) {r['a']:.1f} us, (a) / (f) {r['a'] / r['f']:.2f}, (b) / (f) {r['b'] / r['f']:.2f}")
            verdicts[f"big {'operands' if ops else 'values'}"] = {"us": {f: round(r[f], 1) for f in FORMS}, "f_fraction_of_8TBs": round(traffic / (r["f"] * 1e-6) / HBM, 3)}
    print(json.dumps({"quick": QUICK, "chains": verdicts}))


if __name__ == "__main__":
    main()
