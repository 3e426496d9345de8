#!/usr/bin/env python3
"""The per-group 6-bit Linears on the matrix cores (gemm.quantize_gf6 + gemm.linear_g6*) beside what such a layer runs today and
beside the per-token W6A6 path on the same shape, for the three matrix-core layers of a d30 block (K = 1920), producer included:

  (a)  quantize_gf6(x) + the GEMM: mat_qkv -> 5760 into the KV cache with the q / k norm (linear_g6_qkv_to_cache), proj -> 1920
       (linear_g6), fc1 -> 7680 with the GELU and fc2's INT- / E2M3+ quantizer in the epilogue (linear_g6_gelu_dual)
  (b)  the fake-quant path: ops.quant_rows(x, table, 128) + torch's fp16 F.linear on the de-quantized weight (+ normalize and the
       copy into the cache / + the same one-pass GELU quantizer)
  (c)  the per-token W6A6 path: quantize_fp6(x) + linear_fp6 / linear_fp6_qkv_to_cache (+ the per-token GELU quantizer)

for the pairs E2M3 x E2M3 (W6A6) and E2M3 x E2M1 (W4A6; (c) is the same W6A6 per-token run), at d30's ten scale-step row counts and
at 65 536 rows.  One process; every form works through a ring of operand sets larger than the 256 MiB of L2 + Infinity Cache (cold
operands); a form's sweep over its ring is captured once as a HIP graph and replayed; every form is captured TWICE (x and x', its
A/A twin: the spread between the two is the noise floor of the row), the graphs alternate, best of 5 replays, HIP events around
each.  (a) is checked against its contract on the first 256 rows of ring set 0 before anything is timed: the GEMM within 1.0 x the
bound of tests/gf6_model; for mat_qkv v and the un-normed q, k bit-equal to linear_g6's columns and q, k with the norm inside
tests/qknorm_model.bound; for fc1 the fused output bit-equal to the stand-alone quantizer on the GELU values it emits.
usage: ab_gf6.py [--rows 100,400,...] > profiles/gf6_ab.txt"""
import argparse
import hashlib
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402
import torch.nn.functional as F  # noqa: E402

from fpqvar_amd import _lib, gemm, kv_cache, ops, quant_utils as qu  # noqa: E402
from tests import gemm_model as gm  # noqa: E402
from tests import gf6_model as fm  # noqa: E402
from tests import qknorm_model as qm  # noqa: E402

dev = torch.device("cuda:0")
torch.manual_seed(0)
ROWS = tuple(100 * pn * pn for pn in (1, 2, 3, 4, 5, 6, 8, 10, 13, 16)) + (65536,)   # d30's scale steps (batch 100), a large batch
K, HEADS = 1920, 30
PAIRS = (("e2m3", "e2m3"), ("e2m3", "e2m1"))
LAYERS = (("mat_qkv", 3 * K), ("proj", K), ("fc1", 4 * K))
RING_BYTES = 640 << 20
FORMS = ("a", "b", "c")


def quantize_w(table, w):
    return gemm.quantize_mx(w) if table == "e2m1" else gemm.quantize_gf6(w, table)


def ring_of(per_set):
    return max(2, min(16, RING_BYTES // per_set + 1))


def build(layer, outs, pair, tokens):
    at, wt = pair
    bsz = 100 if tokens % 100 == 0 else 64
    seq = tokens // bsz
    ring = ring_of(tokens * K * 2 + outs * K * 2 + tokens * outs * 2)
    xs = [torch.randn(tokens, K, device=dev).half() for _ in range(ring)]
    ws = [torch.randn(outs, K, device=dev) * 0.02 for _ in range(ring)]
    wg = [quantize_w(wt, w) for w in ws]                                     # (a): the pair's weight operand
    w16 = [ops.quant_rows(w, wt, 128).half() for w in ws]                    # (b): the fake-quantized weight
    wt6 = [gemm.quantize_fp6(w) for w in ws]                                 # (c): per-channel E2M3
    del ws
    bias = (torch.randn(outs, device=dev) * 0.1).half()
    # the contract of (a), before anything is timed
    n = min(tokens, 256)
    ac, asc = gemm.quantize_gf6(xs[0][:n], at)
    rat = gm.ratio(gemm.linear_g6(ac, asc, at, *wg[0], wt, bias), fm.reference(at, wt, ac, asc, *wg[0], bias))
    assert rat <= 1.0, (layer, pair, tokens, rat)
    if layer == "fc1":
        q, h = gemm.linear_g6_gelu_dual(ac, asc, at, *wg[0], wt, bias, return_gelu=True)
        assert torch.equal(q.view(torch.int16), ops.quant_rows_dual(h, "int_neg", "e2m3_pos", 128, None).view(torch.int16)), (layer, pair, tokens)
    if layer == "mat_qkv":
        nb = max(1, n // 4)
        a4, s4 = ac[:nb * 4], asc[:nb * 4]
        hs_c = kv_cache.qk_norm_head_scale(torch.full((1, HEADS, 1, 1), 4.0, device=dev).log())
        y16 = gemm.linear_g6(a4, s4, at, *wg[0], wt, None)
        cache = torch.zeros(2, nb, 4, HEADS, 64, dtype=torch.float16, device=dev)
        q = gemm.linear_g6_qkv_to_cache(a4, s4, at, *wg[0], wt, None, cache, 0, 4)
        got = torch.stack((q.view(-1, K), cache[0].reshape(-1, K), cache[1].reshape(-1, K)), dim=1)
        assert torch.equal(got.view(torch.int16), y16.view(-1, 3, K).view(torch.int16)), (layer, pair, tokens, "split output")
        q = gemm.linear_g6_qkv_to_cache(a4, s4, at, *wg[0], wt, None, cache, 0, 4, qk_norm_scale=hs_c)
        yc = y16.view(-1, 3, K).cpu()
        for part, got in ((0, q.view(-1, K)), (1, cache[0].reshape(-1, K))):
            ref, fin = qm.reference(yc[:, part].contiguous(), None, hs_c.cpu(), part)
            worst, wrong = qm.check(got.cpu(), ref, fin, heads=("gauss",) * HEADS)
            assert not wrong and max(worst.values()) <= 1.0, (layer, pair, tokens, part, worst)
        assert torch.equal(cache[1].reshape(-1, K).view(torch.int16), y16.view(-1, 3, K)[:, 2].contiguous().view(torch.int16)), "v"
    if layer == "mat_qkv":
        caches = [torch.zeros(2, bsz, seq, HEADS, 64, dtype=torch.float16, device=dev) for _ in range(ring)]
        hs = kv_cache.qk_norm_head_scale(torch.full((1, HEADS, 1, 1), 4.0, device=dev).log())
        b32 = torch.cat([torch.randn(K, device=dev) * 0.1, torch.zeros(K, device=dev), torch.randn(K, device=dev) * 0.1])

        def fake(i):
            y = F.linear(ops.quant_rows(xs[i], at, 128), w16[i]).float().add_(b32)
            q, k, v = y.view(bsz, seq, 3, HEADS, 64).unbind(2)
            q = F.normalize(q, dim=-1).mul(hs.view(1, 1, HEADS, 1)).half()
            caches[i][0].copy_(F.normalize(k, dim=-1))
            caches[i][1].copy_(v)
            return q
        calls = {"a": lambda i: gemm.linear_g6_qkv_to_cache(*gemm.quantize_gf6(xs[i], at), at, *wg[i], wt, b32, caches[i], 0, seq, qk_norm_scale=hs),
                 "b": fake,
                 "c": lambda i: gemm.linear_fp6_qkv_to_cache(*gemm.quantize_fp6(xs[i]), *wt6[i], b32, caches[i], 0, seq, qk_norm_scale=hs)}
    elif layer == "proj":
        calls = {"a": lambda i: gemm.linear_g6(*gemm.quantize_gf6(xs[i], at), at, *wg[i], wt, bias),
                 "b": lambda i: F.linear(ops.quant_rows(xs[i], at, 128), w16[i], bias),
                 "c": lambda i: gemm.linear_fp6(*gemm.quantize_fp6(xs[i]), *wt6[i], bias)}
    else:
        calls = {"a": lambda i: gemm.linear_g6_gelu_dual(*gemm.quantize_gf6(xs[i], at), at, *wg[i], wt, bias),
                 "b": lambda i: qu.gelu_fp6_quant_int_neg_e2m3_pos_per_group_cuda(F.linear(ops.quant_rows(xs[i], at, 128), w16[i], bias), 6, 128),
                 "c": lambda i: qu.gelu_fp6_quant_int_neg_e2m3_pos_per_token_cuda(gemm.linear_fp6(*gemm.quantize_fp6(xs[i]), *wt6[i], bias), 6)}
    return calls, ring, rat


def capture(calls, ring):
    graphs, keep = {}, []
    side = torch.cuda.Stream()
    for f, call in calls.items():
        with torch.cuda.stream(side):                                      # warm-up on the capture stream: code objects, allocations
            for i in range(ring):
                call(i)
        torch.cuda.synchronize()
        for name in (f, f + "'"):                                          # the form and its A/A twin
            g = torch.cuda.CUDAGraph()
            with torch.cuda.graph(g, stream=side):
                keep.append([call(i) for i in range(ring)])
            graphs[name] = g
    return graphs, keep


def measure(graphs, ring, rounds=5):
    best = {f: 1e30 for f in graphs}
    for f in graphs:
        graphs[f].replay()
    torch.cuda.synchronize()
    for _ in range(rounds):
        for f in graphs:
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            graphs[f].replay()
            e1.record()
            torch.cuda.synchronize()
            best[f] = min(best[f], e0.elapsed_time(e1) / ring * 1e3)
    return best


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", default=",".join(str(r) for r in ROWS))
    rows = [int(r) for r in ap.parse_args().rows.split(",")]
    sha = hashlib.sha256(open(_lib.LIB_PATH, "rb").read()).hexdigest()[:16]
    print(f"# tools/ab_gf6.py: libfpq_hip.so sha256 {sha}, build tag {_lib.build_tag()}, {torch.cuda.get_device_name(0)}")
    print("# us per producer + GEMM chain, best of 5 alternating graph replays, cold operands (ring > 256 MiB), row-major operands;")
    print("# x' = the A/A twin of form x (the same chain captured again); err/bound: (a)'s GEMM against its contract on 256 rows")
    for layer, outs in LAYERS:
        print(f"# {layer}: K {K} -> {outs}")
        print("#    rows  act  x weight  ring  err/bound " + "  ".join(f"      ({f})      ({f}')" for f in FORMS) + "    b/a    c/a")
        for tokens in rows:
            for pair in PAIRS:
                calls, ring, rat = build(layer, outs, pair, tokens)
                graphs, keep = capture(calls, ring)
                r = measure(graphs, ring)
                best = {f: min(r[f], r[f + "'"]) for f in FORMS}
                times = "  ".join(f"{r[f]:9.1f}  {r[f + chr(39)]:9.1f}" for f in FORMS)
                print(f"{tokens:9d}  {pair[0]} x {pair[1]}     {ring:2d}     {rat:6.3f} {times}  {best['b'] / best['a']:5.2f}  {best['c'] / best['a']:5.2f}",
                      flush=True)
                del graphs, keep, calls
                torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
