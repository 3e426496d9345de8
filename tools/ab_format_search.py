#!/usr/bin/env python3
"""A/B of the format search's two batched forms on one GPU, in ONE process, alternating after warm-up:

  (b)  format_search.search_layer(xs, w, formats)               the default: fp32 detour, five torch passes per pair
  (f)  format_search.search_layer(xs, w, formats, fused=True)   one stacked GEMM and one fpq_sqerr_rows_weighted pass per weight format

on one d30 mat_qkv layer at BASELINE config 4's size (100 samples, 13 600 rows, w [5760 x 1920]), FP6 2 x 2 and FP4 3 x 3; the
30-layer loop of (b) against format_search.search_layers_fused with its single read-back; and the kernel alone at
[13600 x 5760] fp16 for 1, 2 and 3 planes, its bytes taken from the shape as (1 + P) rows cols 2, beside the plain-copy ceiling
README.md records (0.80 - 0.81 of 8 TB/s).  Every figure is device-event time around work that ends in a synchronise; every
form is timed in several bursts and its own spread (max - min over its bursts, the A/A figure) is printed beside it.

    python tools/ab_format_search.py [--quick] [--out FILE]
"""
import argparse
import hashlib
import os
import subprocess
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

from fpqvar_amd import _lib, format_search as fs, ops  # noqa: E402

HBM_PEAK = 8.0e12
COPY_CEILING = "0.80-0.81"


def config4_layer(dev, block=0, n=100):
    """the layer tests/test_gpu_configs.py::_config4_search_layer makes"""
    g = torch.Generator(device=dev).manual_seed(400 + block)
    pns = (1, 2, 3, 4, 5, 6, 8, 10, 13, 16)
    xs = []
    for j in range(n):
        shape = (2, pns[j % 10] ** 2, 1920)
        xs.append((torch.randn(shape, device=dev, generator=g) * torch.exp(0.5 * torch.randn(shape, device=dev, generator=g))).half())
    w = (torch.randn(5760, 1920, device=dev, generator=g) * 0.02).half()
    return xs, w


def timed(fn, reps):
    """ms per call: events around `reps` calls, then a synchronise"""
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / reps


def alternate(forms, reps, bursts, warm=2):
    """{name: [ms per call, one per burst]}: every form warmed, then the forms taking turns burst by burst"""
    for fn in forms.values():
        for _ in range(warm):
            fn()
    torch.cuda.synchronize()
    res = {n: [] for n in forms}
    for _ in range(bursts):
        for n, fn in forms.items():
            res[n].append(timed(fn, reps))
    return res


def line(label, res, a, b, emit):
    ma, mb = min(res[a]), min(res[b])
    sa, sb = max(res[a]) - ma, max(res[b]) - mb
    gap, spread = ma - mb, max(sa, sb)
    verdict = "fused ahead" if gap > spread else "fused behind" if -gap > spread else "inside the spread"
    emit(f"{label:<34} {ma:9.3f} {sa:7.3f} {mb:9.3f} {sb:7.3f} {ma / mb:7.2f}x   {verdict}")
    emit(f"{'':<34} bursts ({a}) {' '.join(f'{v:.3f}' for v in res[a])} | ({b}) {' '.join(f'{v:.3f}' for v in res[b])}")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--quick", action="store_true", help="fewer bursts and a 6-layer loop")
    ap.add_argument("--out", default=None, help="also write the table to this file")
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    lines = []

    def emit(s):
        print(s, flush=True)
        lines.append(s)

    try:
        commit = subprocess.run(["git", "rev-parse", "--short", "HEAD"], capture_output=True, text=True, cwd=os.path.dirname(os.path.abspath(__file__))).stdout.strip()
    except OSError:
        commit = ""
    sha = hashlib.sha256(open(_lib.LIB_PATH, "rb").read()).hexdigest()[:16]
    emit(f"# tools/ab_format_search.py{' --quick' if a.quick else ''}: commit {commit or '(working tree)'}, libfpq_hip.so sha256 {sha}, "
         f"build tag {_lib.build_tag()}, {torch.cuda.get_device_name(0)}")
    emit("# ms per call (best burst) and each form's own spread over its bursts (A/A); the forms alternate burst by burst in one process")
    bursts, reps = (3, 2) if a.quick else (5, 3)
    xs, w = config4_layer(dev)
    emit(f"# one d30 mat_qkv layer, {sum(x.numel() // 1920 for x in xs)} rows, w [5760 x 1920] fp16; {bursts} bursts of {reps} calls")
    emit(f"{'':<34} {'(b) ms':>9} {'A/A':>7} {'(f) ms':>9} {'A/A':>7} {'b/f':>8}")
    for name, formats in (("FP6 2 x 2", fs.FP6_FORMATS), ("FP4 3 x 3", fs.FP4_FORMATS)):
        res = alternate({"b": lambda: fs.search_layer(xs, w, formats), "f": lambda: fs.search_layer(xs, w, formats, fused=True)}, reps, bursts)
        line(f"search_layer {name}", res, "b", "f", emit)
    n_layers = 6 if a.quick else 30
    layers = [(xs, w)] * n_layers                      # the same tensors for every layer: the loop's launches and read-backs are what differs
    for name, formats in (("FP6 2 x 2", fs.FP6_FORMATS), ("FP4 3 x 3", fs.FP4_FORMATS)):
        def loop_b():
            return [fs.search_layer(x, ww, formats) for x, ww in layers]

        def loop_f():
            host = fs.search_layers_fused(layers, formats).cpu()
            return [fs.pick_winner(host[k], formats) for k in range(n_layers)]
        res = alternate({"b": loop_b, "f": loop_f}, 1, bursts, warm=1)
        line(f"{n_layers} layers {name} (ms per loop)", res, "b", "f", emit)
    del layers
    emit("#")
    emit(f"# fpq_sqerr_rows_weighted alone, [13600 x 5760] fp16, bytes = (1 + P) rows cols 2; plain 16-byte copy of README.md: {COPY_CEILING} of 8 TB/s")
    emit(f"{'planes':>6} {'MB':>8} {'us':>9} {'A/A us':>8} {'TB/s':>7} {'of 8 TB/s':>10}")
    rows, cols = 13600, 5760
    g = torch.Generator(device=dev).manual_seed(1)
    ref = torch.randn(rows, cols, device=dev, generator=g).half()
    y = (ref.float().unsqueeze(0) + 0.05 * torch.randn(3, rows, cols, device=dev, generator=g)).half()
    wr = fs.sample_row_weights([rows], cols, dev)
    out = torch.empty(3, dtype=torch.float32, device=dev)
    for P in (1, 2, 3):
        res = alternate({"k": lambda: ops.sqerr_rows_weighted(ref, y[:P], wr, out=out[:P])}, 20, bursts, warm=5)["k"]
        us = min(res) * 1e3
        nbytes = (1 + P) * rows * cols * 2
        emit(f"{P:>6} {nbytes / 1e6:8.1f} {us:9.1f} {(max(res) - min(res)) * 1e3:8.1f} {nbytes / us / 1e6:7.2f} {nbytes / (us * 1e-6) / HBM_PEAK:10.3f}")
    # the launch floor of the call: both launches on a single vector, and on a grid at its cap with little to read
    for label, r, c in (("[1 x 8]", 1, 8), ("[2048 x 2048]", 2048, 2048)):
        res = alternate({"k": lambda: ops.sqerr_rows_weighted(ref.view(-1)[:r * c].view(r, c), y[0].view(-1)[:r * c].view(1, r, c), wr[:r], out=out[:1])},
                        50, bursts, warm=5)["k"]
        emit(f"# both launches, {label} fp16, 1 plane: {min(res) * 1e3:.1f} us per call (A/A {(max(res) - min(res)) * 1e3:.1f})")
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
