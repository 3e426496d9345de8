#!/usr/bin/env python3
"""The producer in front of mat_qkv / fc1 in the FULL-WIDTH mode (the reference's `--rotate` without `--block_rotate`) -
LN(x).mul(scale.add(1)).add_(shift), rotate with the C x C randomized Hadamard matrix, per-group quantize - as one launch against what
a full-width user ran before it, and against the 128-block producer as the memory-bound yardstick:

  (a)   rotation.adaln_rotate_quant_full(x, scale, shift) / adaln_rotate_quant_full_mx(..., kmajor=True)      one launch
  (a')  the same again                                                                                      the tool's own A/A spread
  (b)   torch's layer_norm / mul(scale.add(1)) / add_(shift), then rotation.rotate_quant_full / rotate_quant_full_mx(kmajor=True)
  (b')  the same again
  (c)   rotation.adaln_rotate_quant / adaln_rotate_quant_mx(kmajor=True)          the 128-block form: ANOTHER rotation, the HBM-bound yardstick
  (c')  the same again

(a) is checked against its contract on every ring entry before anything is timed: the rotated rows and the values are
rotate_quant_full's of the h it emits, bit for bit, and the operand form is gemm.quantize_mx of those rotated rows, byte for byte.
C = 1920 (d30, B = 100) and 2304 (d36-512, B = 20) at the ten scale-step row counts [B, pn^2, C]: fp32 rows, fp16 modulation (the
model's case), no smoothing vector ((b) would spend one more pass on it).  One process; every form works through a ring of inputs
larger than the 256 MiB of L2 + Infinity Cache (cold rows); a form's sweep over its ring is captured once as a HIP graph and
replayed; the forms alternate, best of 5 replays, HIP events around each.  Per model and output: the sums over the ten steps, the A/A
spread (the largest |f - f'| of the sums) and the verdict - a chain is ahead only if the sums differ by more than that spread; every
step where (a) is not ahead of (b) by more than the step's own A/A difference is listed.  --big: a line at [65536 x 1920] (B = 64)
with the fraction of 8 TB/s (a) and (c) reach.
The header names the commit: `git rev-parse`, or FPQ_GIT_HEAD where the tree is no git checkout.
usage: ab_adaln_full.py [--quick] [--big]"""
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
dev = torch.device("cuda:0")
torch.manual_seed(0)
MODELS = (("d30", 1920, 100, (1, 2, 3, 4, 5, 6, 8, 10, 13, 16)), ("d36", 2304, 20, (1, 2, 3, 4, 6, 9, 13, 18, 24, 32)))
RING_BYTES = 640 << 20
FORMS = ("a", "a'", "b", "b'", "c", "c'")
HBM = 8e12


def out_bytes(rows, c, mx):
    return rows * c // 2 + rows * c // 128 * 4 if mx else rows * c * 2


def build(batch, seq, c, mx):
    """{form: graph replaying one call per ring entry}, ring length"""
    rows = batch * seq
    per_set = rows * c * 4 + out_bytes(rows, c, mx)                        # cold bytes per call: the fp32 rows, what is written
    ring = max(2, min(32, RING_BYTES // per_set + 1))
    xs = [torch.randn(batch, seq, c, device=dev) * 1.3 + 0.2 for _ in range(ring)]
    sc = (torch.randn(batch, 1, c, device=dev) * 0.3).half()
    sh = (torch.randn(batch, 1, c, device=dev) * 0.3).half()

    def chain(i):
        return torch.nn.functional.layer_norm(xs[i], (c,), eps=1e-6).mul(sc.add(1)).add_(sh)
    if mx:
        full = lambda i: rot.adaln_rotate_quant_full_mx(xs[i], sc, sh, kmajor=True)
        torch_then = lambda i: rot.rotate_quant_full_mx(chain(i), kmajor=True)
        block = lambda i: rot.adaln_rotate_quant_mx(xs[i], sc, sh, kmajor=True)
    else:
        full = lambda i: rot.adaln_rotate_quant_full(xs[i], sc, sh)
        torch_then = lambda i: rot.rotate_quant_full(chain(i))
        block = lambda i: rot.adaln_rotate_quant(xs[i], sc, sh)
    calls = {"a": full, "a'": full, "b": torch_then, "b'": torch_then, "c": block, "c'": block}
    for i in range(ring):                                                  # faster and different is not faster: (a) against its contract
        out, h, y = rot.adaln_rotate_quant_full(xs[i], sc, sh, return_intermediates=True)
        out2, y2 = rot.rotate_quant_full(h, return_rotated=True)
        same = torch.equal(y.view(torch.int16), y2.view(torch.int16)) and torch.equal(out.view(torch.int16), out2.view(torch.int16))
        got = full(i)
        if mx:
            want = gemm.quantize_mx(y.view(rows, c), kmajor=True)
            same = same and torch.equal(got[0], want[0]) and torch.equal(got[1].view(torch.int32), want[1].view(torch.int32))
        else:
            same = same and torch.equal(got.view(torch.int16), out.view(torch.int16))
        if not same:
            raise SystemExit(f"[{batch} x {seq} x {c}] mx={mx}: (a) differs from rotate_quant_full / quantize_mx behind its own h")
        del out, h, y, out2, y2, got
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


def line(batch, seq, name, c, mx):
    graphs, ring, keep = build(batch, seq, c, mx)
    r = measure(graphs, ring)
    aa = max(abs(r[f] - r[f + "'"]) / r[f] for f in ("a", "b", "c")) * 100
    print(f"{batch * seq:7d} {name:4s} {c:5d} {'operands' if mx else 'values':8s} ring {ring:2d}   " + "  ".join(f"{r[f]:9.1f}" for f in FORMS) +
          f"    {r['b'] / r['a']:6.2f}  {r['a'] / r['c']:6.2f}   {aa:4.1f} %", flush=True)
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
    print(f"# tools/ab_adaln_full.py{' --quick' if QUICK else ''}{' --big' if BIG else ''}: commit {commit or 'unknown (no .git here: set FPQ_GIT_HEAD)'}, "
          f"libfpq_hip.so sha256 {sha}, build tag {_lib.build_tag()}, {torch.cuda.get_device_name(0)}")
    print("# us per call, best of 5 alternating graph replays, cold fp32 rows (ring > 256 MiB), fp16 modulation, E2M1, no smoothing vector;")
    print("# (a) one launch: adaln_rotate_quant_full[_mx]; (b) torch layer_norm / mul / add_ + rotate_quant_full[_mx]; (c) the 128-block form "
          "adaln_rotate_quant[_mx]; operands: k-major images")
    print("#   rows model    C output   ring          (a)       (a')        (b)       (b')        (c)       (c')      b/a     a/c    A/A")
    verdicts = {}
    for name, c, batch, pns in MODELS:
        for mx in (False, True):
            tot, lost = {f: 0.0 for f in FORMS}, []
            for pn in (pns[-3:] if QUICK else pns):
                r = line(batch, pn * pn, name, c, mx)
                for f in FORMS:
                    tot[f] += r[f]
                if min(r["b"], r["b'"]) - max(r["a"], r["a'"]) <= max(abs(r[f] - r[f + "'"]) for f in ("a", "b")):
                    lost.append(batch * pn * pn)
            spread = max(abs(tot[f] - tot[f + "'"]) for f in ("a", "b", "c"))
            a, b = min(tot["a"], tot["a'"]), min(tot["b"], tot["b'"])
            who = "one launch ahead" if b - a > spread else "torch chain + rotate_quant_full ahead" if a - b > spread else "inside the spread"
            key = f"{name} {'operands' if mx else 'values'}"
            print(f"# {key}: sum over the steps  " + "  ".join(f"({f}) {tot[f]:9.1f}" for f in FORMS) +
                  f"   A/A spread {spread:.1f} us   (b) / (a) {tot['b'] / tot['a']:.2f}   (a) / (c) {tot['a'] / tot['c']:.2f}   {who}; "
                  f"steps where (a) is not ahead of (b) by more than the spread: {lost or 'none'}")
            verdicts[key] = {"sum_us": {f: round(tot[f], 1) for f in FORMS}, "aa_spread_us": round(spread, 1), "verdict": who, "a_not_ahead_at_rows": lost}
    if BIG:
        for mx in (False, True):
            r = line(64, 1024, "big", 1920, mx)
            traffic = 65536 * 1920 * 4 + out_bytes(65536, 1920, mx)
            print(f"# [65536 x 1920] {'operands' if mx else 'values'}: {traffic / 1e6:.0f} MB per call; (a) {traffic / (r['a'] * 1e-6) / HBM:.2f} of 8 TB/s, "
                  f"(c) {traffic / (r['c'] * 1e-6) / HBM:.2f}, (b) {r['b']:.1f} us, (b) / (a) {r['b'] / r['a']:.2f}")
            verdicts[f"big {'operands' if mx else 'values'}"] = {"us": {f: round(r[f], 1) for f in FORMS}, "a_fraction_of_8TBs": round(traffic / (r["a"] * 1e-6) / HBM, 3)}
    print(json.dumps({"quick": QUICK, "chains": verdicts}))


if __name__ == "__main__":
    main()
