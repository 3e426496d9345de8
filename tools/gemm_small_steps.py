#!/usr/bin/env python3
"""FP4 GEMM at the token counts of the ten scale steps (VAR-d30: 2 x 50 x pn^2 rows; the three Linears fed by per-group FP4
activations), per tile configuration (the library switches FPQ_GEMM_CFG / FPQ_GEMM6_CFG / FPQ_GEMM8_CFG, set through fpq_set_option).
usage: gemm_small_steps.py [fp4|fp6|fp8] [kmajor] [graph] [k=K] [rows=R] [pns=1,2,..] [lib=PATH] [cfg ...]
  kmajor: the operands as k-major images (include/fpq.h; fp4 / fp6);  graph: each burst of 20 calls replayed as one hipGraph (the
  host's launch rate is out of the window: at the first steps a call is about as long as its enqueue);  k, rows, pns: K (1920),
  the rows per pn^2 (100; d36-512: k=2304 rows=20) and the steps' pn;  lib: a variant build (tools/build_variant.sh) instead of the
  stock library.  A cfg is a value of the switch or `default`; the same cfg twice gives the run-to-run spread."""
import os
import sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
opts = dict(a.split("=", 1) for a in sys.argv[1:] if "=" in a)
if "lib" in opts:
    os.environ["FPQ_NO_NATIVE"] = "1"   # (before fpqvar_amd is imported: _lib.use_variant)
import torch
from fpqvar_amd import _lib, gemm

if "lib" in opts:
    _lib.use_variant(opts["lib"])
words = [a for a in sys.argv[1:] if "=" not in a]
kind = words[0] if words and words[0] in ("fp4", "fp6", "fp8") else "fp4"
KM, GRAPH = "kmajor" in words, "graph" in words
cfgs = [a for a in words if a not in ("fp4", "fp6", "fp8", "kmajor", "graph")] or {"fp4": ["default", "20", "30"], "fp6": ["default", "0", "1"], "fp8": ["default", "0", "1"]}[kind]
quant, linear, env = {"fp4": (gemm.quantize_mx, gemm.linear_fp4, "FPQ_GEMM_CFG"), "fp6": (gemm.quantize_fp6, gemm.linear_fp6, "FPQ_GEMM6_CFG"),
                      "fp8": (gemm.quantize_fp8, gemm.linear_fp8, "FPQ_GEMM8_CFG")}[kind]
dev = torch.device("cuda:0")
torch.manual_seed(0)
K, ROWS = int(opts.get("k", 1920)), int(opts.get("rows", 100))
PNS = [int(p) for p in opts["pns"].split(",")] if "pns" in opts else [1, 2, 3, 4, 5, 6, 8, 10, 13, 16]
print(f"# {_lib.build_tag()}: {kind}{' k-major' if KM else ''}{' hipGraph bursts' if GRAPH else ''}, K = {K}, rows = {ROWS} pn^2, best of 3 bursts of 20")
tot = [0.0 for _ in cfgs]


def burst():
    for _ in range(20):
        linear(ac, asc, wc, wsc)


for O in (3 * K, K, 4 * K):
    w = torch.randn(O, K, device=dev) * 0.02
    wc, wsc = quant(w)
    if KM:
        wc = gemm.to_kmajor(wc, 4 if kind == "fp4" else 6, dealt=True)
        if kind == "fp4":
            wsc = gemm.to_kmajor_scales(wsc, weight_side=True)
    for pn in PNS:
        T = ROWS * pn * pn
        x = torch.randn(T, K, device=dev).half()
        ac, asc = quant(x, kmajor=True) if KM else quant(x)
        row = []
        for i, c in enumerate(cfgs):
            _lib.set_option(env, None if c == "default" else int(c))
            for _ in range(5):
                linear(ac, asc, wc, wsc)
            torch.cuda.synchronize()
            run = burst
            if GRAPH:   # (the tiling is chosen at capture)
                graph = torch.cuda.CUDAGraph()
                with torch.cuda.graph(graph):
                    burst()
                run = graph.replay
                run()
                torch.cuda.synchronize()
            best = 1e9
            for _ in range(3):
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                run()
                e1.record()
                torch.cuda.synchronize()
                best = min(best, e0.elapsed_time(e1) / 20 * 1e3)
            row.append(best)
            tot[i] += best
        _lib.set_option(env, None)
        chose = f"  (default = {gemm.fp4_tiling(T, O, K)})" if kind == "fp4" and hasattr(_lib.lib(), "fpq_gemm_fp4_tiling") else ""
        print(f"O={O:5d} T={T:6d} " + "  ".join(f"{c}: {t:7.1f} us" for c, t in zip(cfgs, row)) + chose, flush=True)
print(f"sum over the {3 * len(PNS)} calls: " + "  ".join(f"{c}: {t:8.1f} us" for c, t in zip(cfgs, tot)))
