#!/usr/bin/env python3
"""The producer in front of a per-group W6A6 / W4A6 block's mat_qkv / fc1 with a full-range FP6 activation (E2M3 / E3M2) -
LayerNorm, adaLN modulate, smooth, rotate, per-group quantize to the operands of linear_g6* - as one launch against the cheapest
chain the library offered before it (tools/ab_g6_producers.py is the same measurement for the E1M2 / E3M0 tables):

  (a)   rotation.adaln_rotate_quant_gf6(x, sc, sh, table, smooth, kmajor)                          one launch, operands out
  (a')  the same again                                                                             the tool's own A/A spread
  (b)   gemm.quantize_gf6(rotation.adaln_rotate_quant(x, sc, sh, table, smooth), table, kmajor)    two launches, fp16 rows between them
  (b')  the same again

(b) is a timing baseline only: it quantizes already quantized values, which is not promised to give (a)'s bytes.  What (a) is
checked against, on every ring entry before anything is timed, is its contract: gemm.quantize_gf6 of the rotated rows the values
form emits.
Per row dtype (fp32: the model's residual stream; fp16), table (e2m3, e3m2) and layout (row-major, k-major), C = 1920 (d30, B = 100)
and 2304 (d36-512, B = 20) at the ten scale-step row counts (tools/bench_small_steps.py).  One process; every form works through a
ring of inputs larger than the 256 MiB of L2 + Infinity Cache (cold rows); a form's sweep over its ring is captured once as a HIP
graph and replayed; the forms alternate, best of 5 replays, HIP events around each.  Per model, table and layout: the sums over the
ten steps, the A/A spread (the larger of |a - a'| and |b - b'| of the sums) and the verdict - a chain is ahead only if the sums
differ by more than that spread.  Nothing is routed by these numbers (the producers are opt-in methods): no threshold is derived.
--hw6: instead, the two forms of the rotate kernel behind rotation.rotate_quant_gf6, in the same process by the same method:

  (h)   the default: codes from the FP6 conversion hardware, no table staged, the short-workgroup grid
  (h')  the same again
  (t)   under _lib.option("FPQ_NO_HW6", 1): the staged bucket -> code table        (the switch is read when the graph is captured)
  (t')  the same again

on the rows of the ten scale steps and at [65536 x C], without and with a smoothing vector; (h) and (t) are compared byte for byte
on every ring entry first.  The criterion the table-free form is kept by: not slower than the table form beyond the A/A spread on
every step sum and at [65536 x 1920]; the lines at [65536 x 2304] are printed beside them and any loss there is named too.
--grid: the workgroup count of the table-free form (FPQ_ROT_WGS: workgroups per generation; `hw`: the built-in choice) at [65536 x
1920 / 2304], E3M2, fp16 and fp32 rows, both layouts, without and with a smoothing vector, beside the table form at its own grid:
one graph per setting over a ring of three inputs, best of 9 replays - what the built-in choice for a smoothing vector was read from.
The header names the commit: `git rev-parse`, or FPQ_GIT_HEAD where the tree is no git checkout (tools/collect_profiles.sh).
usage: ab_gf6_producers.py [--quick] [--rows fp16|fp32|both] [--hw6 | --grid]"""
import hashlib
import json
import os
import subprocess
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

from fpqvar_amd import _lib, gemm, rotation as rot  # noqa: E402

QUICK = "--quick" in sys.argv
HW6 = "--hw6" in sys.argv
GRID = "--grid" in sys.argv
ROWS = sys.argv[sys.argv.index("--rows") + 1] if "--rows" in sys.argv else "both"
dev = torch.device("cuda:0")
torch.manual_seed(0)
MODELS = (("d30", 1920, 100, (1, 2, 3, 4, 5, 6, 8, 10, 13, 16)), ("d36", 2304, 20, (1, 2, 3, 4, 6, 9, 13, 18, 24, 32)))
TABLES = ("e2m3", "e3m2")
RING_BYTES = 640 << 20
FORMS = ("a", "a'", "b", "b'")


def build(batch, seq, c, table, kmajor, rows_dtype):
    """{form: graph replaying one call per ring entry}, ring length"""
    x_bytes = 4 if rows_dtype == "fp32" else 2
    per_set = batch * seq * c * x_bytes + batch * seq * c * 3 // 4          # cold bytes per call: the rows, the codes
    ring = max(2, min(32, RING_BYTES // per_set + 1))
    xs = [torch.randn(batch, seq, c, device=dev) if rows_dtype == "fp32" else torch.randn(batch, seq, c, device=dev).half() for _ in range(ring)]
    sc = (torch.randn(batch, 1, c, device=dev) * 0.3).half()
    sh = (torch.randn(batch, 1, c, device=dev) * 0.3).half()
    sm = torch.rand(c, device=dev) + 0.5
    one = lambda i: rot.adaln_rotate_quant_gf6(xs[i], sc, sh, table, smooth=sm, kmajor=kmajor)
    two = lambda i: gemm.quantize_gf6(rot.adaln_rotate_quant(xs[i], sc, sh, table, smooth=sm).view(-1, c), table, kmajor=kmajor)
    calls = {"a": one, "a'": one, "b": two, "b'": two}
    rows = batch * seq
    for i in range(ring):                                                  # faster and different is not faster: (a) against its contract
        y = rot.adaln_rotate_quant(xs[i], sc, sh, table, smooth=sm, return_intermediates=True)[2].view(-1, c)
        got, want = one(i), gemm.quantize_gf6(y, table, kmajor=kmajor)
        live = (lambda s: s[:, :rows]) if kmajor else (lambda s: s)
        if not (torch.equal(got[0], want[0]) and torch.equal(live(got[1]).contiguous().view(torch.uint8), live(want[1]).contiguous().view(torch.uint8))):
            raise SystemExit(f"[{batch} x {seq} x {c}] {table} kmajor={kmajor}: (a) differs from quantize_gf6 of the rotated rows")
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


def build_hw6(rows, c, table, kmajor, rows_dtype, smooth):
    """the same for the two forms of the rotate kernel: {h, h', t, t'}"""
    x_bytes = 4 if rows_dtype == "fp32" else 2
    per_set = rows * c * x_bytes + rows * c * 3 // 4
    ring = max(2, min(32, RING_BYTES // per_set + 1))
    xs = [torch.randn(rows, c, device=dev) if rows_dtype == "fp32" else torch.randn(rows, c, device=dev).half() for _ in range(ring)]
    sm = torch.rand(c, device=dev) + 0.5 if smooth else None
    call = lambda i: rot.rotate_quant_gf6(xs[i], table, smooth=sm, kmajor=kmajor)
    for i in range(ring):
        got = call(i)
        with _lib.option("FPQ_NO_HW6", 1):
            want = call(i)
        if not (torch.equal(got[0], want[0]) and torch.equal(got[1].view(torch.uint8), want[1].view(torch.uint8))):
            raise SystemExit(f"[{rows} x {c}] {table} kmajor={kmajor}: the conversion-hardware form differs from the table form")
    graphs, keep = {}, []
    side = torch.cuda.Stream()
    for f in FORMS:
        with _lib.option("FPQ_NO_HW6", 1 if f.startswith("b") else None):   # slots (b), (b') carry the table form
            with torch.cuda.stream(side):
                for i in range(ring):
                    call(i)
            torch.cuda.synchronize()
            g = torch.cuda.CUDAGraph()
            with torch.cuda.graph(g, stream=side):
                keep.append([call(i) for i in range(ring)])
        graphs[f] = g
    return graphs, ring, keep


def line_hw6(rows, name, c, table, kmajor, rows_dtype, smooth):
    graphs, ring, keep = build_hw6(rows, c, table, kmajor, rows_dtype, smooth)
    r = measure(graphs, ring)
    aa = max(abs(r["a"] - r["a'"]) / r["a"], abs(r["b"] - r["b'"]) / r["b"]) * 100
    print(f"{rows:7d} {name:4s} {c:5d} {rows_dtype:4s} {table:5s} {'k-major' if kmajor else 'row-major':9s} {'smooth' if smooth else 'plain ':6s} ring {ring:2d}   " +
          "  ".join(f"{r[f]:9.1f}" for f in FORMS) + f"    {r['b'] / r['a']:5.2f}   {aa:4.1f} %", flush=True)
    del graphs, keep
    torch.cuda.empty_cache()
    return r


def verdict_hw6(tot):
    """(spread, word) for sums or a single line: (a) = conversion hardware, (b) = table"""
    spread = max(abs(tot["a"] - tot["a'"]), abs(tot["b"] - tot["b'"]))
    h, t = min(tot["a"], tot["a'"]), min(tot["b"], tot["b'"])
    return spread, ("hardware ahead" if t - h > spread else "TABLE AHEAD" if h - t > spread else "inside the spread")


def main_hw6(header):
    print(header)
    print("# us per call of rotation.rotate_quant_gf6, best of 5 alternating graph replays, cold rows (ring > 256 MiB);")
    print("# (h) default: codes from the FP6 conversion hardware; (t) FPQ_NO_HW6 = 1: the staged table; (h) == (t) byte for byte")
    print("#   rows model    C rows table layout    vector ring          (h)       (h')        (t)       (t')     t/h    A/A")
    out, lost, noted = {}, [], []
    for rows_dtype in (("fp16", "fp32") if ROWS == "both" else (ROWS,)):
        for smooth in (False, True):
            for name, c, batch, pns in MODELS:
                for table in TABLES:
                    for kmajor in (False, True):
                        tot = {f: 0.0 for f in FORMS}
                        for pn in (pns[-3:] if QUICK else pns):
                            r = line_hw6(batch * pn * pn, name, c, table, kmajor, rows_dtype, smooth)
                            for f in FORMS:
                                tot[f] += r[f]
                        big = line_hw6(65536, name, c, table, kmajor, rows_dtype, smooth)
                        (spread, who), (bspread, bwho) = verdict_hw6(tot), verdict_hw6(big)
                        key = f"{name} {rows_dtype} {table} {'k-major' if kmajor else 'row-major'} {'smooth' if smooth else 'plain'}"
                        print(f"# {key}: sum over the steps  " + "  ".join(f"({n}) {tot[f]:9.1f}" for n, f in zip(("h", "h'", "t", "t'"), FORMS)) +
                              f"   A/A spread {spread:.1f} us   table / hardware {tot['b'] / tot['a']:.3f}   {who};   at 65536 rows: {big['b'] / big['a']:.3f}, "
                              f"spread {bspread:.1f} us, {bwho}")
                        out[key] = {"sum_us": {f: round(tot[f], 1) for f in FORMS}, "verdict": who, "at_65536_us": {f: round(big[f], 1) for f in FORMS},
                                    "verdict_65536": bwho}
                        if "TABLE" in who or ("TABLE" in bwho and c == 1920):
                            lost.append(key)
                        elif "TABLE" in bwho:
                            noted.append(f"{key} at [65536 x {c}]")
    print("# VERDICT (step sums and [65536 x 1920]): the table-free form is " +
          ("slower than the table form beyond the A/A spread in: " + "; ".join(lost) if lost else "nowhere slower than the table form beyond the A/A spread") +
          ("; outside the criterion the table is ahead in: " + "; ".join(noted) if noted else ""))
    print(json.dumps({"rows": ROWS, "quick": QUICK, "hw6": out, "table_ahead": lost, "table_ahead_outside_the_criterion": noted}))


def main_grid(header):
    print(header)
    print("# us per call of rotation.rotate_quant_gf6(x [65536 x C], 'e3m2'), best of 9 graph replays over a ring of 3 inputs;")
    print("# table: FPQ_NO_HW6 = 1 at its own grid; hw: the table-free form at the built-in grid; hwN: under FPQ_ROT_WGS = N")

    def timed(call, ring):
        side = torch.cuda.Stream()
        with torch.cuda.stream(side):
            for i in range(ring):
                call(i)
        torch.cuda.synchronize()
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g, stream=side):
            keep = [call(i) for i in range(ring)]
        t = measure({f: g for f in FORMS[:1]}, ring, rounds=9, forms=FORMS[:1])["a"]
        del g, keep
        return t

    for c in (1920, 2304):
        for dtype in (torch.float16, torch.float32):
            ring = 3
            xs = [torch.randn(65536, c, device=dev).to(dtype) for _ in range(ring)]
            sm = torch.rand(c, device=dev) + 0.5
            for kmajor in (True, False):
                for smooth in (sm, None):
                    call = lambda i: rot.rotate_quant_gf6(xs[i], "e3m2", smooth=smooth, kmajor=kmajor)
                    with _lib.option("FPQ_NO_HW6", 1):
                        res = {"table": timed(call, ring)}
                    for wgs in (None, 1280, 2560, 3072, 3840, 5120, 8192, 12288):
                        with _lib.option("FPQ_ROT_WGS", wgs):
                            res[f"hw{wgs or ''}"] = timed(call, ring)
                    torch.cuda.empty_cache()
                    print(f"C={c} {'fp16' if dtype is torch.float16 else 'fp32'} {'k-major' if kmajor else 'row-major':9s} {'smooth' if smooth is not None else 'plain ':6s} " +
                          "  ".join(f"{k} {v:6.1f}" for k, v in res.items()), flush=True)


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


def line(batch, seq, name, c, table, kmajor, rows_dtype):
    graphs, ring, keep = build(batch, seq, c, table, kmajor, rows_dtype)
    r = measure(graphs, ring)
    aa = max(abs(r["a"] - r["a'"]) / r["a"], abs(r["b"] - r["b'"]) / r["b"]) * 100
    print(f"{batch * seq:7d} {name:4s} {c:5d} {rows_dtype:4s} {table:5s} {'k-major' if kmajor else 'row-major':9s} ring {ring:2d}   " +
          "  ".join(f"{r[f]:9.1f}" for f in FORMS) + f"    {r['b'] / r['a']:5.2f}   {aa:4.1f} %", flush=True)
    del graphs, keep
    torch.cuda.empty_cache()
    return r


def verdict(tot):
    spread = max(abs(tot["a"] - tot["a'"]), abs(tot["b"] - tot["b'"]))
    a, b = min(tot["a"], tot["a'"]), min(tot["b"], tot["b'"])
    return spread, ("one launch ahead" if b - a > spread else "two launches ahead" if a - b > spread else "inside the spread")


def main():
    try:
        commit = subprocess.run(["git", "rev-parse", "--short", "HEAD"], capture_output=True, text=True, cwd=os.path.dirname(__file__)).stdout.strip()
    except OSError:
        commit = ""
    commit = commit or os.environ.get("FPQ_GIT_HEAD", "")
    sha = hashlib.sha256(open(_lib.LIB_PATH, "rb").read()).hexdigest()[:16]
    if GRID:
        return main_grid(f"# tools/ab_gf6_producers.py --grid: commit {commit or 'unknown (no .git here: set FPQ_GIT_HEAD)'}, libfpq_hip.so sha256 {sha}, "
                         f"build tag {_lib.build_tag()}, {torch.cuda.get_device_name(0)}")
    if HW6:
        return main_hw6(f"# tools/ab_gf6_producers.py{' --quick' if QUICK else ''} --rows {ROWS} --hw6: commit {commit or 'unknown (no .git here: set FPQ_GIT_HEAD)'}, "
                        f"libfpq_hip.so sha256 {sha}, build tag {_lib.build_tag()}, {torch.cuda.get_device_name(0)}")
    print(f"# tools/ab_gf6_producers.py{' --quick' if QUICK else ''} --rows {ROWS}: commit {commit or 'unknown (no .git here: set FPQ_GIT_HEAD)'}, libfpq_hip.so sha256 {sha}, "
          f"build tag {_lib.build_tag()}, {torch.cuda.get_device_name(0)}")
    print("# us per call of the producer chain, best of 5 alternating graph replays, cold rows (ring > 256 MiB), fp16 modulation, a smoothing vector;")
    print("# (a) one launch: adaln_rotate_quant_gf6; (b) two launches: adaln_rotate_quant + quantize_gf6; (a) == quantize_gf6(rotated rows) byte for byte")
    print("#   rows model    C rows table layout    ring          (a)       (a')        (b)       (b')     b/a    A/A")
    verdicts = {}
    for rows_dtype in (("fp32", "fp16") if ROWS == "both" else (ROWS,)):
        for name, c, batch, pns in MODELS:
            for table in TABLES:
                for kmajor in (False, True):
                    tot = {f: 0.0 for f in FORMS}
                    worst = None
                    for pn in (pns[-3:] if QUICK else pns):
                        r = line(batch, pn * pn, name, c, table, kmajor, rows_dtype)
                        for f in FORMS:
                            tot[f] += r[f]
                        ratio = min(r["b"], r["b'"]) / min(r["a"], r["a'"])
                        if worst is None or ratio < worst[0]:
                            worst = (ratio, batch * pn * pn)
                    spread, who = verdict(tot)
                    key = f"{name} {rows_dtype} {table} {'k-major' if kmajor else 'row-major'}"
                    print(f"# {key}: sum over the steps  " + "  ".join(f"({f}) {tot[f]:9.1f}" for f in FORMS) +
                          f"   A/A spread {spread:.1f} us ({spread / tot['a'] * 100:.2f} %)   two launches / one launch {tot['b'] / tot['a']:.3f}   {who}; "
                          f"least step ratio {worst[0]:.2f} at {worst[1]} rows")
                    verdicts[key] = {"sum_us": {f: round(tot[f], 1) for f in FORMS}, "aa_spread_us": round(spread, 1), "verdict": who,
                                     "least_step_ratio": round(worst[0], 3), "least_step_rows": worst[1]}
    print(json.dumps({"rows": ROWS, "quick": QUICK, "chains": verdicts}))


if __name__ == "__main__":
    main()
