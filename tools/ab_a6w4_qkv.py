#!/usr/bin/env python3
"""mat_qkv of a mixed-format W4A4 block with a 6-bit activation: the A6W4 GEMM writing q, k, v to their destinations beside the
sequence such a layer ran before, producer and KV step included, E3M0 activation, fp32 weight scales, an IncrementalKVCache
(kv_bit 6) standing at the step's position:

  (s)   quantize_g6(x) + linear_a6w4_qkv_to_cache(..., cache.kv, cache.len, L) + cache.commit_written(L)
  (s')  the same again                                                            the tool's own A/A spread
  (p)   quantize_g6(x) + linear_a6w4 + cache.append(k, v)                         one [tokens, 3C] tensor, the cache copies k, v in

and with the q / k L2 norm (attn_l2_norm): (s) linear_a6w4_qkv_to_cache(qk_norm_scale=, fp32 bias) + commit_written against
(p) linear_a6w4 + cache.append_qk_norm.  Row-major operands and k-major images.

d30 (C = 1920, B = 100) and d36-512 (C = 2304, B = 20) at the ten scale-step row counts.  One process; every form works through a
ring of operand sets and caches larger than the 256 MiB of L2 + Infinity Cache (cold operands); a form's sweep over its ring is
captured once as a HIP graph and replayed; the forms alternate, best of 5 replays, HIP events around each.  Before anything is
timed, (s) and (p) without the norm are compared bit for bit at every row count: q, the returned K / V views and the whole cache.
Per model: the sums over the ten steps, the A/A spread |s - s'| of the sums, and whether any row loses by more than its spread.
usage: ab_a6w4_qkv.py [--quick]"""
import hashlib
import json
import os
import subprocess
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

from fpqvar_amd import _lib, gemm, kv_cache  # noqa: E402

QUICK = "--quick" in sys.argv
TABLE = "e3m0"
dev = torch.device("cuda:0")
torch.manual_seed(0)
MODELS = (("d30", 1920, 100, (1, 2, 3, 4, 5, 6, 8, 10, 13, 16)), ("d36", 2304, 20, (1, 2, 3, 4, 6, 9, 13, 18, 24, 32)))
RING_BYTES = 640 << 20
FORMS = ("s", "s'", "p")


def make_cache(bsz, heads, prev, pos, seq):
    """a cache whose entries [prev, pos) are the previous step's, still unquantized, with room for this step's seq"""
    c = kv_cache.IncrementalKVCache(bsz, pos + seq, heads, 64, 6, device=dev)
    c.kv.copy_(torch.randn(c.kv.shape, device=dev) * 0.5)
    return c


def calls(xs, w, w_km, caches, bsz, heads, prev, pos, seq, km, norm, hs, b16, b32):
    """{form: i -> one step on ring entry i}"""
    c3 = 3 * heads * 64

    def at_step(i):
        c = caches[i]
        c.len, c._prev = pos, prev
        return c

    def split(i):
        c = at_step(i)
        a = gemm.quantize_g6(xs[i], TABLE, kmajor=km)
        ww = w_km[i] if km else w[i]
        q = gemm.linear_a6w4_qkv_to_cache(*a, TABLE, *ww, b32 if norm else b16, c.kv, c.len, seq, qk_norm_scale=hs if norm else None)
        return (q, *c.commit_written(seq))

    def plain(i):
        c = at_step(i)
        a = gemm.quantize_g6(xs[i], TABLE, kmajor=km)
        bias = None if norm else b16
        qkv = gemm.linear_a6w4_km(*a, TABLE, *w_km[i], bias, outs=c3) if km else gemm.linear_a6w4(*a, TABLE, *w[i], bias)
        q, k, v = qkv.view(bsz, seq, 3, heads, 64).unbind(2)
        if norm:
            return c.append_qk_norm(q, k, v, hs, b32)
        return (q, *c.append(k, v))

    return {"s": split, "s'": split, "p": plain}


def operands(bsz, heads, prev, pos, seq, ring):
    k = heads * 64
    tokens = bsz * seq
    xs = [torch.randn(tokens, k, device=dev).half() for _ in range(ring)]
    w0 = gemm.quantize_mx(torch.randn(3 * k, k, device=dev) * 0.02)
    w = [tuple(t.clone() for t in w0) for _ in range(ring)]
    wk0 = (gemm.to_kmajor(w0[0], 4, dealt=True), gemm.to_kmajor_scales(w0[1], weight_side=True))
    w_km = [tuple(t.clone() for t in wk0) for _ in range(ring)]
    caches = [make_cache(bsz, heads, prev, pos, seq) for _ in range(ring)]
    return xs, w, w_km, caches


def check_bits(bsz, heads, prev, pos, seq, km, b16):
    """(s) == (p) without the norm: q, the returned views, the whole cache"""
    xs, w, w_km, caches = operands(bsz, heads, prev, pos, seq, 2)
    caches[1].kv.copy_(caches[0].kv)
    xs[1], w[1], w_km[1] = xs[0], w[0], w_km[0]
    f = calls(xs, w, w_km, caches, bsz, heads, prev, pos, seq, km, False, None, b16, None)
    qs, ks, vs = f["s"](0)
    qp, kp, vp = f["p"](1)
    torch.cuda.synchronize()
    ok = torch.equal(qs.view(-1), qp.reshape(-1)) and torch.equal(ks, kp) and torch.equal(vs, vp) and torch.equal(caches[0].kv, caches[1].kv)
    if not ok:
        raise SystemExit(f"(s) != (p) at B {bsz} L {seq} heads {heads} kmajor {km}: nothing timed")


def build(bsz, heads, prev, pos, seq, km, norm, hs, b16, b32):
    k, tokens = heads * 64, bsz * seq
    per_set = tokens * k * 2 + 3 * k * k // 2 + 2 * 3 * tokens * k * 2 + 2 * bsz * (pos - prev) * k * 2   # (p)'s cold bytes per call
    ring = max(2, min(32, RING_BYTES // per_set + 1))
    ops = operands(bsz, heads, prev, pos, seq, ring)
    f = calls(*ops, bsz, heads, prev, pos, seq, km, norm, hs, b16, b32)
    graphs, keep = {}, [ops]
    side = torch.cuda.Stream()
    for form in FORMS:
        with torch.cuda.stream(side):                                      # warm-up on the capture stream
            for i in range(ring):
                f[form](i)
        torch.cuda.synchronize()
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g, stream=side):
            keep.append([f[form](i) for i in range(ring)])
        graphs[form] = g
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
    print(f"# tools/ab_a6w4_qkv.py{' --quick' if QUICK else ''}: commit {commit or '(working tree)'}, libfpq_hip.so sha256 {sha}, "
          f"build tag {_lib.build_tag()}, {torch.cuda.get_device_name(0)}")
    print(f"# us per producer + mat_qkv + KV step, {TABLE} activation, best of 5 alternating graph replays, cold operands (ring > 256 MiB)")
    steps = []
    for name, k, bsz, pns in MODELS:
        pos = 0
        prev = 0
        for pn in pns:
            steps.append((name, k // 64, bsz, prev, pos, pn * pn))
            prev, pos = pos, pos + pn * pn
    if QUICK:
        steps = [s for s in steps if s[5] in (169, 256, 576, 1024)]
    b16 = {k: (torch.randn(3 * k, device=dev) * 0.1).half() for _, k, _, _ in MODELS}
    b32 = {k: torch.randn(3 * k, device=dev) * 0.1 for _, k, _, _ in MODELS}
    hs = {k: torch.rand(k // 64, device=dev) * 3 + 1 for _, k, _, _ in MODELS}
    for km in (False, True):
        for name, heads, bsz, prev, pos, seq in steps:
            check_bits(bsz, heads, prev, pos, seq, km, b16[heads * 64])
        torch.cuda.empty_cache()
    print("# (s) == (p) bit for bit without the norm at every row count, row-major and k-major: q, the K / V views, the whole cache")
    results = {}
    for norm in (False, True):
        for km in (False, True):
            label = f"{'norm' if norm else 'plain'} {'k-major' if km else 'row-major'}"
            print(f"# ---- {label}")
            print("#  tokens model     C  ring          (s)       (s')        (p)     p/s    A/A   verdict")
            tot = {m[0]: {f: 0.0 for f in FORMS} for m in MODELS}
            losing = {m[0]: [] for m in MODELS}
            for name, heads, bsz, prev, pos, seq in steps:
                k = heads * 64
                graphs, ring, keep = build(bsz, heads, prev, pos, seq, km, norm, hs[k], b16[k], b32[k])
                r = measure(graphs, ring)
                aa = abs(r["s"] - r["s'"])
                loses = min(r["s"], r["s'"]) - r["p"] > aa
                if loses:
                    losing[name].append(bsz * seq)
                print(f"{bsz * seq:7d} {name:4s} {k:5d}  ring {ring:2d}   " + "  ".join(f"{r[f]:9.1f}" for f in FORMS) +
                      f"   {r['p'] / r['s']:5.2f}  {aa / r['s'] * 100:4.1f} %   {'LOSES' if loses else 'ok'}", flush=True)
                for f in FORMS:
                    tot[name][f] += r[f]
                del graphs, keep
                torch.cuda.empty_cache()
            for name, t in tot.items():
                spread = abs(t["s"] - t["s'"])
                loses = min(t["s"], t["s'"]) - t["p"] > spread
                print(f"# {name} {label}: sum over the steps  " + "  ".join(f"({f}) {t[f]:9.1f}" for f in FORMS) +
                      f"   A/A spread {spread:.1f} us ({spread / t['s'] * 100:.2f} %)   (p) / (s) {t['p'] / t['s']:.3f}"
                      f"   split {'LOSES' if loses else 'does not lose'} outside the spread; rows that lose by more than their own spread: "
                      f"{losing[name] or 'none'}")
                results[f"{name} {label}"] = {"sum_us": {f: round(t[f], 1) for f in FORMS}, "aa_spread_us": round(spread, 1),
                                              "p_over_s": round(t["p"] / t["s"], 3), "split_loses": bool(loses), "losing_rows": losing[name]}
    print(json.dumps({"table": TABLE, "quick": QUICK, "results": results}))


if __name__ == "__main__":
    main()
