#!/usr/bin/env python3
"""Load time of a packed weight as a matrix-core operand, at the four Linear shapes of VAR-d30, per table:
  (a) PackedWeight.operands(kmajor=True)                                    one launch (fpq_packed_to_operands)
  (b) e2m1 only: fp4_operands() + to_kmajor(dealt) + to_kmajor_scales       the torch lookup and the two converters
  (c) from_float(kmajor=True) on the fp32 weight                            calibration again: the quantizer and the two converters
us per layer on COLD operands: every call takes the next weight of a ring larger than 256 MiB (L2 + MALL hold none of it when
its turn comes again); a whole pass over the ring is one captured graph, timed with HIP events around a replay, best of three.  (a) also as bytes moved
(file codes and scales read, operand images written) over time, as a fraction of 8 TB/s.  Last: the sum over d30's 120 Linears.
usage: bench_packed_load.py [table ...]"""
import hashlib
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

from fpqvar_amd import _lib, gemm, packed as pk  # noqa: E402

SHAPES = ((5760, 1920), (1920, 1920), (7680, 1920), (1920, 7680))     # mat_qkv, proj, fc1, fc2: [out, in]
RING_BYTES = 320 << 20
PEAK = 8e12
dev = torch.device("cuda:0")


def best(fns, passes=3, eager=False):
    """us per call: one pass over the ring - each call on its own (cold) weight, into buffers of its own - captured as a graph
    (the host needs ~10 us to issue one of these calls, about what the kernel takes: eager timing would measure Python) and
    replayed `passes` times between HIP events.  eager: issued call by call instead - (b)'s fp4_operands uploads its lookup
    table from the host on every call, which a capture refuses; its six launches and that copy are what the route costs."""
    fns[0]()            # the first call of a kind: module load, lazily built tables
    torch.cuda.synchronize()
    if not eager:
        graph, keep = torch.cuda.CUDAGraph(), []
        with torch.cuda.graph(graph):
            for f in fns:
                keep.append(f())
    times = []
    for _ in range(passes):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        if eager:
            for f in fns:
                f()
        else:
            graph.replay()
        e1.record()
        torch.cuda.synchronize()
        times.append(e0.elapsed_time(e1) / len(fns) * 1e3)
    return min(times)


def from_float(table, lin):
    if table in pk.FP4_TABLES:
        kw = {} if table == "e2m1" else dict(weight_fp_type=table, w6_forms=True, w6_kmajor=True)
        return gemm.FP4Linear.from_float(lin, kmajor=True, **kw)
    return gemm.FP6GroupLinear.from_float(lin, table, "fp6_e2m3", kmajor=True)


def parent_route(p):
    codes, scales = p.fp4_operands()
    return gemm.to_kmajor(codes, 4, dealt=True), gemm.to_kmajor_scales(scales, weight_side=True)


def main():
    tables = sys.argv[1:] or list(pk.FP4_TABLES + pk.FP6_TABLES)
    sha = hashlib.sha256(open(_lib.LIB_PATH, "rb").read()).hexdigest()[:16]
    print(f"# tools/bench_packed_load.py: libfpq_hip.so sha256 {sha}, build tag {_lib.build_tag()}, {torch.cuda.get_device_name(0)}")
    print(f"# us per layer, cold operands (ring > {RING_BYTES >> 20} MiB), best of 3 replays of a captured pass; (a) operands(kmajor=True), (b) fp4_operands + "
          "to_kmajor + to_kmajor_scales, (c) from_float(kmajor=True) on the fp32 weight; of peak: (a)'s bytes / time / 8 TB/s; eager: issued call by call (host-bound for (a): ~10 us per call)")
    print("#   table  out x in       ring     (a) us   MB moved  of peak  (a) eager  (b) eager  b/a(e)     (c) us    c/a")
    torch.manual_seed(0)
    model = {t: [0.0, 0.0] for t in tables}
    for outs, k in SHAPES:
        n32 = max(2, RING_BYTES // (outs * k * 4) + 1)
        lins = [torch.nn.Linear(k, outs, bias=False, device=dev) for _ in range(n32)]
        for table in tables:
            cols = 128
            one = pk.pack_weight(lins[0].weight, table, cols)
            w_codes, w_scales = one.operands(True)
            moved = one.codes.numel() + one.scales.numel() * one.scales.element_size() + w_codes.numel() + w_scales.numel() * 4
            n = max(2, RING_BYTES // moved + 1)
            ring = [pk.pack_weight(lins[i % n32].weight, table, cols) for i in range(n)]
            del one, w_codes, w_scales
            a = best([(lambda p=p: p.operands(True)) for p in ring])
            ae = best([(lambda p=p: p.operands(True)) for p in ring], eager=True)   # issued as (b) is: the like-for-like figure
            b = best([(lambda p=p: parent_route(p)) for p in ring], eager=True) if table == "e2m1" else None
            c = best([(lambda m=m: from_float(table, m)) for m in lins])
            model[table][0] += 30 * a
            model[table][1] += 30 * c
            print(f"    {table:5s}  {outs:4d} x {k:4d}   {n:5d}   {a:8.1f}   {moved / 1e6:8.2f}   {moved / (a * 1e-6) / PEAK:6.3f}   "
                  + f"{ae:8.1f}   " + (f"{b:8.1f}  {b / ae:5.2f}" if b is not None else "       -      -") + f"   {c:8.1f}  {c / a:5.2f}", flush=True)
            del ring
        del lins
        torch.cuda.empty_cache()
    print("# whole model: the 120 Linears of d30 (30 blocks x the four shapes), ms")
    print("#   table   (a) ms    (c) ms    c/a")
    for table in tables:
        a, c = model[table]
        print(f"    {table:5s}  {a / 1e3:7.2f}   {c / 1e3:7.2f}  {c / a:5.2f}")


if __name__ == "__main__":
    main()
