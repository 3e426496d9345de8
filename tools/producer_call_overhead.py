#!/usr/bin/env python3
"""What a call of a row producer costs on the host before the library is entered: the Python front of rotation.py timed on the CPU
with the library replaced by a stub that returns at once (the stubs of tests/test_producer_call_path_host.py: no GPU rule, no
compiled binding, stream 0, no device guard).  CPU tensors stand in for the operands; nothing reads them.  The twelve public
producers on rows [2, 3, 256] with fp16 modulation and a float32 smooth vector, the forms with two layouts in both: the median over
batches of the mean time per call.

To compare two trees, run it on each in turn on the same machine, and one of them twice: the spread between the twin runs is what
a difference has to exceed.
usage: producer_call_overhead.py REPOSITORY_ROOT [--batches N] [--calls N]"""
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

from fpqvar_amd import rotation as rot  # noqa: E402

torch.set_num_threads(1)


class Stub:
    def __getattr__(self, name):
        fn = lambda *a: 0
        setattr(self, name, fn)
        return fn


stub, guard = Stub(), contextlib.nullcontext()
rot.lib = lambda: stub
rot._native = None
rot.require_gpu = lambda *a, **k: None
rot.stream_ptr = lambda device: 0
rot.device_guard = lambda device: guard

B, L, C = 2, 3, 256
f16 = lambda *s: torch.zeros(*s, dtype=torch.float16)
x, y, res = f16(B, L, C), f16(B, L, C), torch.zeros(B, L, C)
gate, sc, sh, sm = f16(B, 1, C), f16(B, 1, C), f16(B, 1, C), torch.ones(C)

CASES = (
    ("rotate_quant", lambda: rot.rotate_quant(x, "e2m1", smooth=sm)),
    ("rotate_quant_mx", lambda: rot.rotate_quant_mx(x, smooth=sm)),
    ("rotate_quant_mx (images)", lambda: rot.rotate_quant_mx(x, smooth=sm, kmajor=True)),
    ("rotate_quant_g6", lambda: rot.rotate_quant_g6(x, "e3m0", smooth=sm)),
    ("rotate_quant_gf6 (images)", lambda: rot.rotate_quant_gf6(x, "e2m3", smooth=sm, kmajor=True)),
    ("adaln_rotate_quant", lambda: rot.adaln_rotate_quant(x, sc, sh, "e2m1", smooth=sm)),
    ("adaln_rotate_quant (intermediates)", lambda: rot.adaln_rotate_quant(x, sc, sh, "e2m1", smooth=sm, return_intermediates=True)),
    ("adaln_rotate_quant_mx", lambda: rot.adaln_rotate_quant_mx(x, sc, sh, smooth=sm)),
    ("adaln_rotate_quant_mx (images)", lambda: rot.adaln_rotate_quant_mx(x, sc, sh, smooth=sm, kmajor=True)),
    ("adaln_rotate_quant_g6", lambda: rot.adaln_rotate_quant_g6(x, sc, sh, "e3m0", smooth=sm)),
    ("adaln_rotate_quant_g6 (images)", lambda: rot.adaln_rotate_quant_g6(x, sc, sh, "e3m0", smooth=sm, kmajor=True)),
    ("adaln_rotate_quant_gf6", lambda: rot.adaln_rotate_quant_gf6(x, sc, sh, "e2m3", smooth=sm)),
    ("adaln_rotate_quant_token", lambda: rot.adaln_rotate_quant_token(x, sc, sh, "e2m3", smooth=sm)),
    ("adaln_rotate_quant_token (fp8)", lambda: rot.adaln_rotate_quant_token(x, sc, sh, "e2m3", smooth=sm, emit="fp8")),
    ("adaln_rotate_quant_token (fp6, image)", lambda: rot.adaln_rotate_quant_token(x, sc, sh, "e2m3", smooth=sm, emit="fp6", kmajor=True)),
    ("adaln_rotate_quant_token (bf6)", lambda: rot.adaln_rotate_quant_token(x, sc, sh, "e3m2", smooth=sm, emit="bf6")),
    ("resid_adaln_rotate_quant", lambda: rot.resid_adaln_rotate_quant(y, gate, res, sc, sh, "e2m1", smooth=sm)),
    ("resid_adaln_rotate_quant_mx (images, in place)", lambda: rot.resid_adaln_rotate_quant_mx(y, gate, res, sc, sh, smooth=sm, kmajor=True, inplace=True)),
    ("resid_adaln_rotate_quant_token", lambda: rot.resid_adaln_rotate_quant_token(y, gate, res, sc, sh, "e2m3", smooth=sm)),
    ("resid_adaln_rotate_quant_token (fp6)", lambda: rot.resid_adaln_rotate_quant_token(y, gate, res, sc, sh, "e3m2", smooth=sm, emit="fp6")),
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
print(f"# tools/producer_call_overhead.py {args.root}: us per call on the host, library stubbed; median (and minimum) of {args.batches} batches of "
      f"{args.calls} calls, the cases taking turns; torch {torch.__version__}, one thread")
for name, _ in CASES:
    print(f"{name:48s} {statistics.median(times[name]):8.2f}   (min {min(times[name]):6.2f})")
