#!/usr/bin/env python3
"""What a call of a per-group Linear costs on the host before the library is entered: the Python front of gemm.py timed on the CPU
with the library replaced by a stub that returns at once (the stubs of tests/test_linear_call_path_host.py: no GPU rule, no
compiled binding, stream 0, no device guard, a CPU tensor as NaN scratch).  CPU tensors stand in for the operands; nothing reads
them.  The eight public Linears, the two quantizers and FP4Linear.forward (E3M0, row-major) at tokens 8, K 256, outs 128 / 384:
the median over batches of the mean time per call.

To compare two trees, run it on each in turn on the same machine, and one of them twice: the spread between the twin runs is what
a difference has to exceed.
usage: linear_call_overhead.py REPOSITORY_ROOT [--batches N] [--calls N]"""
import argparse
import contextlib
import statistics
import sys
import time

ap = argparse.ArgumentParser()
ap.add_argument("root", help="the checkout whose fpqvar_amd is imported")
ap.add_argument("--batches", type=int, default=201)
ap.add_argument("--calls", type=int, default=250)
args = ap.parse_args()
sys.path.insert(0, args.root)

import torch  # noqa: E402

from fpqvar_amd import gemm, ops  # noqa: E402

torch.set_num_threads(1)


class Stub:
    def __getattr__(self, name):
        fn = lambda *a: 0
        setattr(self, name, fn)
        return fn


stub, flag, guard = Stub(), torch.zeros(2, dtype=torch.int32), contextlib.nullcontext()
gemm.lib = lambda: stub
gemm._native = None
gemm.require_gpu = lambda *a, **k: None
gemm.stream_ptr = lambda device: 0
gemm.device_guard = lambda device: guard
ops._nan_scratch = lambda device: flag

T, K, G, O = 8, 256, 2, 128
H, C, B, SEQ = 2, 64, 2, 4
u8 = lambda *s: torch.zeros(*s, dtype=torch.uint8)
f16 = lambda *s: torch.zeros(*s, dtype=torch.float16)
f32 = lambda *s: torch.zeros(*s)
sa, sak = f16(T, G), f32(G, T)
a4, a6, a4k, a6k = u8(T, K // 2), u8(T, K * 3 // 4), u8(G, T, 64), u8(G, T, 96)
w, sw, wk, swk = u8(O, K // 2), f32(O, G), u8(G, O, 64), f32(G, O)
w3, sw3, w3k, sw3k = u8(3 * H * C, K // 2), f32(3 * H * C, G), u8(G, 3 * H * C, 64), f32(G, 3 * H * C)
bias, bias3, cache, x = f16(O), f16(3 * H * C), f16(2, B, 16, H, C), f16(T, K)
module = gemm.FP4Linear(w, sw, bias, K, O, "e3m0")

CASES = (
    ("linear_fp4", lambda: gemm.linear_fp4(a4, sa, w, sw, bias)),
    ("linear_fp4 (images)", lambda: gemm.linear_fp4(a4k, sak, wk, swk, bias)),
    ("linear_fp4_gelu_dual", lambda: gemm.linear_fp4_gelu_dual(a4, sa, w, sw, bias)),
    ("linear_fp4_qkv_to_cache", lambda: gemm.linear_fp4_qkv_to_cache(a4, sa, w3, sw3, bias3, cache, 3, SEQ)),
    ("linear_a6w4", lambda: gemm.linear_a6w4(a6, sa, "e3m0", w, sw, bias)),
    ("linear_a6w4_km", lambda: gemm.linear_a6w4_km(a6k, sak, "e3m0", wk, swk, bias)),
    ("linear_a6w4_gelu_dual", lambda: gemm.linear_a6w4_gelu_dual(a6, sa, "e3m0", w, sw, bias)),
    ("linear_a6w4_gelu_dual_km", lambda: gemm.linear_a6w4_gelu_dual_km(a6k, sak, "e3m0", wk, swk, bias)),
    ("linear_a6w4_qkv_to_cache", lambda: gemm.linear_a6w4_qkv_to_cache(a6, sa, "e3m0", w3, sw3, bias3, cache, 3, SEQ)),
    ("linear_a6w4_qkv_to_cache (images)", lambda: gemm.linear_a6w4_qkv_to_cache(a6k, sak, "e3m0", w3k, sw3k, bias3, cache, 3, SEQ)),
    ("quantize_mx", lambda: gemm.quantize_mx(x)),
    ("quantize_g6", lambda: gemm.quantize_g6(x, "e3m0")),
    ("FP4Linear.forward (e3m0)", lambda: module(x)),
)


def batch_us(fn):
    t0 = time.perf_counter()
    for _ in range(args.calls):
        fn()
    return (time.perf_counter() - t0) / args.calls * 1e6


# the cases take turns, one batch each per round: a slow spell of the machine falls on all of them alike
times = {name: [] for name, _ in CASES}
for name, fn in CASES:
    batch_us(fn)
for _ in range(args.batches):
    for name, fn in CASES:
        times[name].append(batch_us(fn))
print(f"# tools/linear_call_overhead.py {args.root}: us per call on the host, library stubbed; median (and minimum) of {args.batches} batches of "
      f"{args.calls} calls, the cases taking turns; torch {torch.__version__}, one thread")
for name, _ in CASES:
    print(f"{name:36s} {statistics.median(times[name]):8.2f}   (min {min(times[name]):6.2f})")
